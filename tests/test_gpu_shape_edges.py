"""Frames and tiles at the kernels' unit sizes on the GPU (tests/shape_sets.py: the table, its
cameras and its references; tests/test_shape_edges.py ties the emulations used here to the oracle
and to numpy on the CPU).

Every comparison is exact: the oracle's bits (or the emulation's, for the calls that have no
oracle form), RGBA8 as image.to_srgb8 with alpha 255, zero words in tile rows past the frame, and
the prefill in every byte the output description does not cover.

  routes        every kind of frame_sequences.KINDS (and direct, pipe_list and pixel on the depth-9
                tree) on every shape of groups A-H and every tile, ONE context per kind: the state
                keyed by the frame's shape (hints, cost slots, class lists, speculation buffers) is
                crossed between tiny shapes too
  speculation   three frames, a turn of half a degree and the way back, per shape
  swizzle       the four XCD orders around their group sizes (groups G, H, I)
  outputs       RGBA8, pitched rows, frame placement
  queries       count_traffic, trace_camera, pick
  accumulations plain, moments, adaptive in passes (1, 1, rest)
  denoise       images of 1 to 25 pixels and around a 256-pixel segment
  group         more ranks than bands
  row limit     tiles past pixel row 2^31 - 1 are refused and leave their outputs alone
  LDS scene     the resident scene at exactly its 2048-unit budget, one unit over it, and a depth-8
                tree inside it

An ORT_ERR_HIP ends the session (pytest.exit): nothing more starts on the GPU."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import chart_scenes as CS
import denoise_sets as ds
import frame_sequences as FS
import shape_sets as SS
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.image import to_srgb8

pytestmark = pytest.mark.gpu

F = np.float32
AH = SS.cases("ABCDEFGH", tiles=True)
DEEP = {"deep_direct": "direct", "deep_pipe_list": "pipe_list", "deep_pixel": "pixel"}
ROUTES = list(FS.KINDS) + list(DEEP)
THR, MIN, FLOOR = 0.05, 2, 0.05   # tests/test_gpu_adaptive.py's criterion
ACC_SHAPE = (5, 4)                # (num_samples, max_depth) of the accumulations
ACC_PASSES = (1, 1, 3)            # (1, 1, rest)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@contextlib.contextmanager
def hip_errors_end_the_session(what):
    try:
        yield
    except L.OrtError as e:
        if e.code == L.ORT_ERR_HIP:
            pytest.exit(f"ORT_ERR_HIP in {what}: {e}\n  read the cause from the code; do not run it again", returncode=3)
        raise


# ---- one context per route, kept while the tests of that route run -------------------------------------
_open = {"key": None, "ad": None}


def close_context():
    if _open["ad"] is not None:
        _open["ad"].close()
    _open.update(key=None, ad=None)


@pytest.fixture(scope="module", autouse=True)
def _contexts_are_closed():
    yield
    close_context()


def context(ort, key, kind_name=None, scene_name="d4", options=()):
    """The adapter of `key`: opened (and the one before it closed) when the key changes, with the
    kind's options over frame_sequences' defaults and the scene uploaded."""
    if _open["key"] != key:
        close_context()
        ad = FS.GpuAdapter(ort)
        kind = FS.KINDS[kind_name] if kind_name else FS.Kind(())
        opts = dict(FS.OPTION_DEFAULTS)
        opts.update(kind.options)
        opts.update(options)
        for name, value in opts.items():
            ad.set_option(name, value)
        ad.set_option("force_layout", 1 if kind.explicit else 0)
        ad.upload(*SS.scene(scene_name))
        _open.update(key=key, ad=ad)
    return _open["ad"]


def render_and_check(ad, case_id, shape, use_octree=1, scene_name="d4", fmt="rgb32f", form="host", turn=0.0, what=""):
    """One frame of the case into a prefilled buffer: every byte is the expected one."""
    c = SS.CASES[case_id]
    d = SS.describe(case_id, fmt, form)
    ref = SS.frame(case_id, shape, use_octree, scene_name, turn)
    with hip_errors_end_the_session(f"{what} {case_id} {shape}"):
        buf = ad.render(SS.params(case_id, shape, use_octree, turn), c.tile, d)
        got = ad.read(buf)
    want = SS.expected_buffer(case_id, ref, d)
    assert got.shape == want.shape and np.array_equal(got, want), \
        f"{what} {case_id} {shape} {fmt} {form}: " + SS.differences(got, want, d)


# ---- 1. routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,case_id", [pytest.param(r, c, id=f"{r}-{c}") for r in ROUTES for c in AH])
def test_route_on_shape(ort, route, case_id):
    kind_name = DEEP.get(route, route)
    scene_name = "deep" if route in DEEP else "d4"
    kind = FS.KINDS[kind_name]
    ad = context(ort, "route:" + route, kind_name, scene_name)
    assert ad.r.info()["layout"] == ("explicit" if kind.explicit else "compact")
    render_and_check(ad, case_id, kind.shapes[-1], kind.use_octree, scene_name, what=route)


# ---- 2. speculation on tiny frames -------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", SS.cases("ABCDEFGH"))
def test_speculation_on_tiny_frames(ort, case_id):
    """pixel_spec: the shape's first frame runs whole chains (1 launch), the second and third
    speculate (3).  Then the camera turns by half a degree and comes back: below 1000 pixels one
    moved pixel already exceeds moved x 1000 <= pixels, so the fall-back runs on every turn (a
    fall-back decided on the device is three launches as well: the count is 1 or 3).  Every frame
    is the oracle's."""
    kind = FS.KINDS["pixel_spec"]
    shape = kind.shapes[-1]
    assert shape[0] >= 5, "more than one chunk of 4 samples: the frames speculate"
    ad = context(ort, "spec", "pixel_spec")
    seen = []
    for turn in (0.0, 0.0, 0.0, 0.5, 0.0):
        render_and_check(ad, case_id, shape, turn=turn, what=f"pixel_spec frame {len(seen)}")
        seen.append(ad.r.frame_trace_times_ms(1)[0][1])
    print(f"{case_id}: launches per frame {seen}")
    assert seen[:3] == [1, 3, 3] and all(n in (1, 3) for n in seen[3:]), (case_id, seen)


# ---- 3. swizzle ------------------------------------------------------------------------------------------------
SWIZZLED = ([(k, c) for k in ("direct_plain", "direct_pairs") for c in SS.cases("GHI")] +
            [("pipe_list", c) for c in SS.cases("GH")])


@pytest.mark.parametrize("kind_name,case_id", [pytest.param(k, c, id=f"{k}-{c}") for k, c in SWIZZLED])
def test_xcd_swizzle_around_its_group_sizes(ort, kind_name, case_id):
    kind = FS.KINDS[kind_name]
    ad = context(ort, "swizzle:" + kind_name, kind_name)
    shape = (1, 1) if SS.CASES[case_id].group == "I" else kind.shapes[-1]
    assert kind_name == "pipe_list" or shape == (1, 1)
    try:
        for mode in (0, 1, 2, -1):
            ad.set_option("xcd_swizzle", mode)
            render_and_check(ad, case_id, shape, what=f"{kind_name} xcd_swizzle={mode}")
    finally:
        ad.set_option("xcd_swizzle", -1)


# ---- 4. outputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", SS.cases("ABCD", tiles=True))
def test_output_formats_pitch_and_placement(ort, case_id):
    ad = context(ort, "outputs")
    for shape in ((1, 1), (2, 4)):
        for fmt, form in (("rgba8", "host"), ("rgb32f", "pitch"), ("rgba8", "pitch"), ("rgb32f", "frame"), ("rgba8", "frame"),
                          ("rgb32f", "device")):
            render_and_check(ad, case_id, shape, fmt=fmt, form=form, what="outputs")


# ---- 5. queries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", SS.cases("ABCDEF"))
def test_count_traffic(ort, case_id):
    ad = context(ort, "outputs")
    c = SS.CASES[case_id]
    for shape, use_octree in (((1, 1), 1), ((2, 3), 1), ((1, 1), 0), ((2, 3), 0)):
        with hip_errors_end_the_session(f"count_traffic {case_id}"):
            got = ad.count(SS.params(case_id, shape, use_octree), c.tile)
        assert got == SS.counters(case_id, shape, use_octree), (case_id, shape, use_octree)


@pytest.mark.parametrize("case_id", SS.cases("ABCDEF", tiles=True))
def test_trace_camera_and_pick(ort, case_id):
    ad = context(ort, "outputs")
    r = ad.r
    c = SS.CASES[case_id]
    x0, w, y0, rows, bh, bs = c.tile
    ys = FS.pixel_rows(c.tile)
    for which, ns in (("first_sample", 1), ("first_sample", 5), ("pixel_centre", 1)):
        rays, t, sphere, normals = SS.camera(case_id, which, ns)
        p = SS.params(case_id, (ns, 1))
        with hip_errors_end_the_session(f"trace_camera {case_id}"):
            gt, gs, gn, gr = r.trace_camera(p, c.ort_tile(), which=which, rays=True, normals=True)
        assert same_bits(gr, rays) and same_bits(gt, t) and same_bits(gs, sphere) and same_bits(gn, normals), (case_id, which, ns)
        assert same_bits(r.trace_camera(p, c.ort_tile(), which=which, rays=True, hits=False), rays), (case_id, which, ns)
        pad = ys >= c.size[1]
        assert (gs[pad] == -1).all() and (gt[pad] == 0).all() and (gr[pad] == 0).all() and (gn[pad] == 0).all()
        for j, i in {(0, 0), (rows - 1, w - 1), (rows // 2, w // 2)}:
            if pad[j]:
                continue
            with hip_errors_end_the_session(f"pick {case_id}"):
                ps, pt, point = r.pick(p, x0 + i, int(ys[j]), which=which)
            o, d = rays[j, i, :3], rays[j, i, 3:]
            assert ps == int(sphere[j, i]) and F(pt).tobytes() == t[j, i].tobytes(), (case_id, which, j, i)
            assert same_bits(point, (o + (t[j, i] * d).astype(F)).astype(F))


# ---- 6. accumulations ------------------------------------------------------------------------------------------
def picture(mean, inside, fmt="rgb32f"):
    """The preview of a linear mean: its gamma, zeros in the rows past the frame."""
    from octreeraytracer_amd.renderer import gamma_host
    pic = gamma_host(mean)
    pic[~inside] = 0
    if fmt == "rgb32f":
        return pic
    out = np.full(pic.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = to_srgb8(pic)
    out[~inside] = 0
    return out


@pytest.mark.parametrize("case_id", SS.cases("ABCD", tiles=True, only_tiles=SS.BAND_TILES))
def test_accumulations(ort, case_id):
    ad = context(ort, "outputs")
    r = ad.r
    c = SS.CASES[case_id]
    p, tile, inside = SS.params(case_id, ACC_SHAPE), c.ort_tile(), c.inside()
    N = ACC_SHAPE[0]
    n_inside = int(inside.sum()) * c.tile[1]
    with hip_errors_end_the_session(f"accumulations {case_id}"):
        with r.accumulate(p, tile) as plain, r.accumulate(p, tile, moments=True) as mom, \
                r.accumulate(p, tile, adaptive=True) as ada, r.accumulate(p, tile, adaptive=True) as free:
            assert (ada.counts() == 0).all()
            st = ada.adaptive_stats(THR, MIN, FLOOR)
            assert (st["pixels"], st["samples"], st["pending"]) == (n_inside, 0, n_inside)
            done, passes = 0, []
            for i, n in enumerate(ACC_PASSES):
                done += n
                passes.append((n, MIN, THR, FLOOR))
                what = f"{case_id} after pass {i}"
                fmt = "rgba8" if i == 1 else "rgb32f"
                want = SS.preview(case_id, ACC_SHAPE, done)
                assert same_bits(plain.step(n), want), what
                assert same_bits(mom.step(n, format=fmt), picture(SS.moments(case_id, ACC_SHAPE, done)[0], inside, fmt)), what
                assert same_bits(picture(SS.moments(case_id, ACC_SHAPE, done)[0], inside), want), what
                gm, gv = mom.moments()
                wm, wv = SS.moments(case_id, ACC_SHAPE, done)
                assert same_bits(gm, wm) and same_bits(gv, wv), what
                # adaptive without a criterion: the moments accumulation
                assert same_bits(free.step_adaptive(n, 0.0, 0, FLOOR), want), what
                fm, fv = free.moments()
                assert same_bits(fm, wm) and same_bits(fv, wv) and (free.counts()[inside] == done).all(), what
                # adaptive with the criterion: the emulation's counts, moments and preview
                wc, wm, wv = SS.adaptive(case_id, ACC_SHAPE, tuple(passes))
                pic = ada.step_adaptive(n, THR, MIN, FLOOR, format=fmt)
                am, av = ada.moments()
                assert np.array_equal(ada.counts(), wc) and same_bits(am, wm) and same_bits(av, wv), what
                assert same_bits(pic, picture(wm, inside, fmt)), what
                st = ada.adaptive_stats(THR, MIN, FLOOR)
                assert (st["pixels"], st["samples"]) == (n_inside, int(wc[inside].sum())), what
                nxt = SS.adaptive(case_id, ACC_SHAPE, tuple(passes) + ((1, MIN, THR, FLOOR),))[0]
                assert st["pending"] == int((nxt != wc).sum()), what
                if n_inside:
                    assert (st["min_count"], st["max_count"]) == (int(wc[inside].min()), int(wc[inside].max())), what
            assert plain.finished and mom.finished and free.finished and done == N
            assert same_bits(plain.step(1), SS.frame(case_id, ACC_SHAPE))
            assert (ada.counts()[~inside] == 0).all()


# ---- 7. denoise ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SS.DENOISE_SMALL + SS.DENOISE_SEGMENT, ids=lambda v: str(v))
def test_denoise_on_a_few_pixels_and_around_a_segment(ort, w, h):
    import torch
    ad = context(ort, "outputs")
    r = ad.r
    img, t, sph, nrm = SS.denoise_inputs(w, h)
    guides = ((t, sph), nrm)
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(np.array(img)).to(dev)
    d_guides = (torch.from_numpy(ds.records(t, sph)).to(dev), torch.from_numpy(np.array(nrm)).to(dev))
    d_var = torch.from_numpy(np.array(SS.denoise_variance(w, h))).to(dev)
    torch.cuda.synchronize()
    with hip_errors_end_the_session(f"denoise {w}x{h}"):
        for iterations in (1, 3, 6):
            for terms in ("off", "on"):
                kw = dict(SS.TERMS_ON if terms == "on" else SS.TERMS_OFF, iterations=iterations)
                what = (w, h, iterations, terms)
                want = SS.denoised(w, h, iterations, terms)
                assert same_bits(r.denoise(np.array(img), guides, **kw), want), what
                got = r.denoise(d_img, d_guides, **kw)
                torch.cuda.synchronize()
                assert same_bits(got.cpu().numpy(), want), what
                if iterations != 3:
                    continue
                want8 = SS.denoised(w, h, iterations, terms, fmt="rgba8")
                assert same_bits(r.denoise(np.array(img), guides, format="rgba8", **kw), want8), what
                got = r.denoise(d_img, d_guides, format="rgba8", **kw)
                torch.cuda.synchronize()
                assert same_bits(got.cpu().numpy(), want8), what
                buf = np.array(img)                                   # in place, host and device
                assert r.denoise(buf, guides, out=buf, **kw) is buf and same_bits(buf, want), what
                d_buf = d_img.clone()
                torch.cuda.synchronize()
                r.denoise(d_buf, d_guides, out=d_buf, **kw)
                torch.cuda.synchronize()
                assert same_bits(d_buf.cpu().numpy(), want), what
                # ort_denoise_ex: the variance term and the gamma
                for fmt in ("rgb32f", "rgba8"):
                    wantx = SS.denoised(w, h, iterations, terms, variance=True, gamma=True, fmt=fmt)
                    kx = dict(kw, variance=np.array(SS.denoise_variance(w, h)), sigma_variance=2.0, gamma=True, format=fmt)
                    assert same_bits(r.denoise(np.array(img), guides, **kx), wantx), what + (fmt,)
                    got = r.denoise(d_img, d_guides, **dict(kx, variance=d_var))
                    torch.cuda.synchronize()
                    assert same_bits(got.cpu().numpy(), wantx), what + (fmt,)


# ---- 8. the group: more ranks than bands -------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,world", [(20, 5, 3), (7, 17, 3), (33, 16, 8)], ids=lambda v: str(v))
def test_group_with_more_ranks_than_bands(ort, oracle, w, h, world):
    import torch
    from octreeraytracer_amd.group import TRANSPORT_COPY, RenderGroup
    close_context()
    s, t = SS.scene()
    shape = (2, 4)
    turns = (0.0, 0.5, 1.0, 1.5)
    ps = [CS.chart_params(ort, w, h, num_samples=shape[0], max_depth=shape[1], yaw=CS.YAW + turn) for turn in turns]
    refs = [oracle.render(s, t, p) for p in ps]

    def want(k, fmt):
        if fmt == "rgb32f":
            return refs[k]
        px = np.full((h, w, 4), 255, np.uint8)
        px[..., :3] = to_srgb8(refs[k])
        return px

    with hip_errors_end_the_session(f"group {w}x{h} x{world}"):
        with ort.Renderer(0) as single:
            single.upload(s, t)
            for k, p in enumerate(ps):
                assert same_bits(single.render(p), refs[k]), "the single-context render"
        with RenderGroup([0] * world, TRANSPORT_COPY) as g:
            g.upload(s, t)
            for fmt in ("rgb32f", "rgba8"):
                t_dtype = torch.float32 if fmt == "rgb32f" else torch.uint8
                for k, p in enumerate(ps[:2]):
                    assert same_bits(g.render(p, format=fmt), want(k, fmt)), (fmt, k, "host")
                    out = torch.full(want(k, fmt).shape, 7, dtype=t_dtype, device="cuda:0")
                    torch.cuda.synchronize()
                    g.render(p, out=out, format=fmt)
                    assert same_bits(out.cpu().numpy(), want(k, fmt)), (fmt, k, "device")
        with RenderGroup([0] * world, TRANSPORT_COPY, inflight=2) as g:
            g.upload(s, t)
            for fmt in ("rgb32f", "rgba8"):
                t_dtype = torch.float32 if fmt == "rgb32f" else torch.uint8
                outs = [torch.full(want(k, fmt).shape, 7, dtype=t_dtype, device="cuda:0") if k % 2 else
                        np.full(want(k, fmt).shape, 7, want(k, fmt).dtype) for k in range(4)]
                torch.cuda.synchronize()
                tickets = [g.submit(p, out, format=fmt) for p, out in zip(ps, outs)]   # four frames before the first wait
                for k, tk in enumerate(tickets):
                    g.wait(tk)
                    got = outs[k].cpu().numpy() if k % 2 else outs[k]
                    assert same_bits(got, want(k, fmt)), (fmt, k, "pipelined")


# ---- 9. the row limit ------------------------------------------------------------------------------------------------
def limit_params(ort, shape=(1, 1)):
    return CS.chart_params(ort, *SS.LIMIT_FRAME, num_samples=shape[0], max_depth=shape[1])


@pytest.mark.parametrize("name", SS.REFUSED_TILES)
def test_tiles_past_the_row_limit_are_refused(ort, oracle, name):
    """ORT_PLACE_TILE and host outputs only: every call returns ORT_ERR_INVALID_ARG before anything
    is allocated or launched and leaves its prefilled output alone; the next frame is the oracle's."""
    ad = context(ort, "outputs")
    r = ad.r
    tl = SS.REFUSED_TILES[name]
    tile = ort.Tile(*tl)
    rows, w = tl[3], tl[1]
    s, t = SS.scene()
    for shape in ((1, 1), (2, 3)):
        p = limit_params(ort, shape)
        pc, tc = p.to_c(), tile.to_c()
        for fmt, dtype, ch in (("rgb32f", F, 3), ("rgba8", np.uint8, 4)):
            out = np.full((rows, w, ch), 7, dtype)
            with pytest.raises(ort.OrtError) as e:
                r.render(p, tile, out=out, format=fmt)
            assert e.value.code == L.ORT_ERR_INVALID_ARG and "2^31 - 1" in str(e.value), str(e.value)
            assert (out == 7).all(), (name, fmt)
        counts = (C.c_uint64 * L.ORT_COUNT_N)(*([99] * L.ORT_COUNT_N))
        assert r._lib.ort_count_traffic(r._ctx, C.byref(pc), C.byref(tc), counts) == L.ORT_ERR_INVALID_ARG
        assert list(counts) == [99] * L.ORT_COUNT_N and b"2^31 - 1" in r._lib.ort_last_error(r._ctx)
        rec = np.full((rows * w, 2), 7, np.int32)
        with pytest.raises(ort.OrtError) as e:
            r.trace_camera(p, tile, out=rec)
        assert e.value.code == L.ORT_ERR_INVALID_ARG and (rec == 7).all()
        for kw in (dict(), dict(moments=True), dict(adaptive=True)):
            with pytest.raises(ort.OrtError) as e:
                r.accumulate(p, tile, **kw)
            assert e.value.code == L.ORT_ERR_INVALID_ARG and "2^31 - 1" in str(e.value)
        if tl[4] == 0:  # denoise's tile form (a banded tile is the wrapper's own refusal): its guides' camera query
            img = np.full((rows, w, 3), F(0.5))
            with pytest.raises(ort.OrtError) as e:
                r.denoise(img, None, params=p, tile=tile)
            assert e.value.code == L.ORT_ERR_INVALID_ARG and "2^31 - 1" in str(e.value) and (img == F(0.5)).all()
        with hip_errors_end_the_session("the frame after a refusal"):
            assert same_bits(r.render(p), oracle.render(s, t, p)), (name, shape)


@pytest.mark.parametrize("name", SS.LARGEST_TILES)
def test_the_largest_accepted_tiles_are_all_zeros(ort, name):
    ad = context(ort, "outputs")
    r = ad.r
    tl = SS.LARGEST_TILES[name]
    tile = ort.Tile(*tl)
    rows, w = tl[3], tl[1]
    with hip_errors_end_the_session(f"largest tile {name}"):
        for shape in ((1, 1), (2, 3), (5, 4)):
            p = limit_params(ort, shape)
            for fmt, dtype, ch in (("rgb32f", F, 3), ("rgba8", np.uint8, 4)):
                out = np.full((rows + 1, w, ch), 7, dtype)
                r.render(p, tile, out=out, format=fmt)
                assert (out[:rows].view(np.uint8) == 0).all() and (out[rows:] == 7).all(), (name, shape, fmt)
            assert set(r.count_traffic(p, tile).values()) == {0}
            gt, gs, gn, gr = r.trace_camera(p, tile, rays=True, normals=True)
            assert (gt == 0).all() and (gs == -1).all() and (gn == 0).all() and (gr == 0).all()
        with r.accumulate(p, tile, adaptive=True) as acc:
            assert (acc.step_adaptive(2, THR, MIN, FLOOR).view(np.uint8) == 0).all()
            m, v = acc.moments()
            assert (acc.counts() == 0).all() and (m == 0).all() and (v == F(-1)).all()
            assert acc.adaptive_stats(THR, MIN, FLOOR)["pixels"] == 0


# ---- 10. the LDS-resident scene at its budget -----------------------------------------------------------------------------
LDS_UNITS = 2048   # ORT_OPT_PIXEL_LDS_SCENE: 32 KB of 16-byte units


def lds_scene(ort, name):
    """(spheres, tree, takes the LDS walk, tree depth or None)."""
    if name == "just_over":      # 1257 + 681 + 111 = 2049 units
        s = ort.random_spheres(111, 42)
        return s, ort.build_octree(s, 4, 1), False, None
    if name == "exactly_at":     # 1017 + 845 + 186 = 2048 units (found by a search over seeds 1-50)
        s = ort.random_spheres(186, 5)
        return s, ort.build_octree(s, 4, 2), True, None
    # depth 8 inside the budget: 10 spheres, two of them small and overlapping, so that the nodes
    # that hold both split down to the depth limit (705 + 651 + 10 = 1366 units)
    s = ort.random_spheres(10, 42)
    cr = s.center_radius.copy()
    cr[1, :3] = cr[0, :3] + F(0.015)
    cr[0, 3] = cr[1, 3] = F(0.03)
    s = ort.SphereSet(cr, s.mat_albedo.copy(), s.fuzz_ri.copy())
    return s, ort.build_octree(s, 8, 1), True, 8


@pytest.mark.parametrize("name", ("just_over", "exactly_at", "depth_8"))
def test_pixel_paths_lds_scene_at_its_budget(ort, oracle, name):
    import ray_sets
    from octreeraytracer_amd.renderer import radiance_rays_host, rng_states
    close_context()
    s, t, resident, depth = lds_scene(ort, name)
    units = t.n_nodes + t.n_indices + s.n
    assert (16 * units <= 32768) == resident                     # the budget rule decides which walk runs
    assert units == {"just_over": LDS_UNITS + 1, "exactly_at": LDS_UNITS, "depth_8": 1366}[name]
    p = ort.FrameParams.default_camera(97, 63, num_samples=4, max_depth=8)
    ref = oracle.render(s, t, p)
    rays = ray_sets.make_rays(ort, oracle, s, t, 77)
    if depth:  # and rays aimed at the overlapping pair, where the tree is deepest
        rng = np.random.default_rng(5)
        u = rng.normal(size=(200, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        c = s.center_radius[0, :3].astype(np.float64)
        rays = np.ascontiguousarray(np.concatenate([rays, np.concatenate([c + 0.5 * u, -u], axis=1).astype(F)]))
    states = rng_states(len(rays), 3)
    want = radiance_rays_host(s, t, rays, states, max_depth=8, paths=2)
    with hip_errors_end_the_session(f"lds scene {name}"):
        with ort.Renderer(0) as r:
            r.upload(s, t)
            if depth:
                assert r.info()["tree_depth"] == depth == FS.tree_depth(t)
            r.set_pixel_paths(1)
            for on in (1, 0, 1):
                r.set_pixel_lds_scene(on)
                assert same_bits(r.render(p), ref), f"{name} lds_scene={on}"
                assert r.frame_trace_times_ms(1)[0][1] == 1
                assert same_bits(r.trace_radiance(rays, states, max_depth=8, paths=2), want), f"{name} lds_scene={on} radiance"
