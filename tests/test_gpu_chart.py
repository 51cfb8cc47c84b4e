"""The material chart (tests/chart_scenes.py) on the GPU: the code that decides what a hit does --
bsdf, refract_vec, schlick, the FINAL shortcuts, hit_record's division by the radius, the
importance cut, the default: material branch -- at values the seeded scenes never reach, through
every kernel family that shades: the camera-ray kernels that shade themselves, the per-bounce
pipeline, whole-pixel paths with and without the LDS scene copy, speculating frames, RGBA8 and
band-tile output, the counting kernels, ray queries and the GPU octree builder.

Every frame is compared on its float32 bits with oracle.render; a frame that is a case of
tests/golden/glsl/canonical.json also with the SHA-256 of the reference's own shader.  The module
renders on a Renderer of its own and every test puts back the options it sets.

Also here: frames without bounces (max_depth <= 0: every channel 1.0) and the refusal of frames
without samples (num_samples <= 0: ORT_ERR_INVALID_ARG from every entry point that renders, the
output untouched)."""
import contextlib
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import chart_scenes as CS
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.image import to_srgb8
from test_glsl_parity import CANON, frame_sha

pytestmark = pytest.mark.gpu

G = Path(__file__).resolve().parent / "golden"
DEFAULTS = {"tile_pairs": -1, "cost_order": 1, "split_heavy": -1, "sort_paths": 2, "persistent": 2, "kid_skip": 1,
            "pixel_paths": -1, "pixel_lds_scene": 1, "pixel_speculate": -1, "pixel_heavy_first": -1}
FILL = 0xA5


@pytest.fixture(scope="module")
def cr(ort):
    r = ort.Renderer(0)
    yield r
    r.close()


@contextlib.contextmanager
def options(r, **kw):
    """Renderer.set_<name>(value) for the block, the defaults put back after it."""
    try:
        for k, v in kw.items():
            getattr(r, "set_" + k)(v)
        yield r
    finally:
        for k in kw:
            getattr(r, "set_" + k)(DEFAULTS[k])


def upload(r, key=(4, 1), explicit=False):
    s, t = CS.scene(*key)
    r.set_layout(L.ORT_LAYOUT_EXPLICIT if explicit else -1)
    try:
        r.upload(s, t)
    finally:
        r.set_layout(-1)
    assert r.info()["layout"] == ("explicit" if explicit else "compact")
    return s, t


@pytest.fixture(scope="module")
def want(ort, oracle):
    """(tree key, W, H, samples, bounces, use_octree, yaw) -> the oracle's frame, rendered once."""
    done = {}

    def get(key, W, H, ns, md, use_octree=1, yaw=CS.YAW):
        k = (key, W, H, ns, md, use_octree, yaw)
        if k not in done:
            s, t = CS.scene(*key)
            p = CS.chart_params(ort, W, H, num_samples=ns, max_depth=md, use_octree=use_octree, yaw=yaw)
            done[k] = oracle.render(s, t if use_octree else None, p)
            done[k].setflags(write=False)
        return done[k]

    return get


def assert_bits(img, ref, what):
    assert img.shape == ref.shape and img.dtype == np.float32, what
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} of {img.shape[0] * img.shape[1]} pixels differ from the oracle's bits"


def assert_canonical(img, name, p, key):
    """The frame is the reference shader's (canonical.json), and the case is the frame rendered."""
    c = CANON["cases"][name]
    assert (c["W"], c["H"], c["spp"], c["md"], c["oct"], c["depth"], c["m"]) == (
        p.width, p.height, p.num_samples, p.max_depth, p.use_octree) + tuple(key), name
    assert frame_sha(img) == c["sha256"], f"{name}: not the reference shader's frame"


def launches(r):
    return r.frame_trace_times_ms(1)[0][1]


# ---- camera-ray kernels that shade themselves: 1 sample, 1 bounce ---------------------------------

@pytest.mark.parametrize("variant", ["pairs0", "pairs1", "cost_order0", "split_heavy", "explicit", "brute", "d6m0"])
def test_camera_ray_kernels(ort, cr, want, variant):
    """Every chart sphere meets shade_bounce<true> (the FINAL shortcuts) here."""
    key = (6, 0) if variant == "d6m0" else (4, 1)
    upload(cr, key, explicit=variant == "explicit")
    use_octree = int(variant != "brute")
    p = CS.chart_params(ort, 96, 64, use_octree=use_octree)
    ref = want(key, 96, 64, 1, 1, use_octree)
    opts = {"pairs0": {"tile_pairs": 0}, "pairs1": {"tile_pairs": 1}, "cost_order0": {"cost_order": 0},
            "split_heavy": {"split_heavy": 20}}.get(variant, {})
    with options(cr, **opts):
        for k in range(3 if variant == "split_heavy" else 2):  # (split walks: from the second frame on)
            img = cr.render(p)
            assert_bits(img, ref, f"{variant}, frame {k + 1}")
            if use_octree and key == (4, 1):
                assert_canonical(img, "chart_b1", p, key)


# ---- the per-bounce pipeline -----------------------------------------------------------------------

PIPE_FRAMES = {"1x2": (96, 64, 1, 2, None), "2x8": (96, 64, 2, 8, "chart_spp2_b8"), "7x3": (48, 32, 7, 3, "chart_spp7_b3")}


@pytest.mark.parametrize("sort", [0, 1, 2])
@pytest.mark.parametrize("frame", list(PIPE_FRAMES))
def test_pipeline(ort, cr, want, frame, sort):
    W, H, ns, md, canon = PIPE_FRAMES[frame]
    upload(cr)
    p = CS.chart_params(ort, W, H, num_samples=ns, max_depth=md)
    ref = want((4, 1), W, H, ns, md)
    for persistent in (0, 2):
        with options(cr, pixel_paths=0, sort_paths=sort, persistent=persistent):
            for k in range(2):  # (the second frame sorts by the first one's list lengths)
                img = cr.render(p)
                assert_bits(img, ref, f"pipeline {frame}, sort {sort}, persistent {persistent}, frame {k + 1}")
            if canon:
                assert_canonical(img, canon, p, (4, 1))


def test_pipeline_kid_skip(ort, cr, want):
    """One-sphere leaves holding the concentric and the identical pairs: what the rejected-sphere
    skip keys on (kid_table.h)."""
    upload(cr)
    p = CS.chart_params(ort, 96, 64, num_samples=2, max_depth=8)
    ref = want((4, 1), 96, 64, 2, 8)
    for skip in (0, 2, 1):
        with options(cr, pixel_paths=0, kid_skip=skip):
            assert_bits(cr.render(p), ref, f"kid skip {skip}")


def test_pipeline_explicit_and_brute_force(ort, cr, want):
    upload(cr, explicit=True)
    with options(cr, pixel_paths=0):
        p = CS.chart_params(ort, 96, 64, num_samples=2, max_depth=8)
        assert_bits(cr.render(p), want((4, 1), 96, 64, 2, 8), "explicit 2 x 8")
        p = CS.chart_params(ort, 64, 48, num_samples=2, max_depth=6, use_octree=0)
        img = cr.render(p)
        assert_bits(img, want((4, 1), 64, 48, 2, 6, 0), "brute force 2 x 6")
        assert_canonical(img, "chart_brute_spp2_b6", p, (4, 1))


# ---- whole-pixel paths ------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [(96, 64, 2, 8), (97, 63, 5, 6)], ids=["2x8", "odd_5x6"])
@pytest.mark.parametrize("variant", ["d4m1_lds1", "d4m1_lds0", "d6m0"])
def test_whole_pixel_paths(ort, cr, want, variant, frame):
    """d4 m1 (105 nodes, 30 spheres) fits the 32 KB LDS scene copy; d6 m0 does not."""
    W, H, ns, md = frame
    key = (6, 0) if variant == "d6m0" else (4, 1)
    upload(cr, key)
    p = CS.chart_params(ort, W, H, num_samples=ns, max_depth=md)
    ref = want(key, W, H, ns, md)
    with options(cr, pixel_paths=1, pixel_speculate=0, pixel_lds_scene=0 if variant.endswith("lds0") else 1):
        img = cr.render(p)
        assert launches(cr) == 1
        assert_bits(img, ref, f"whole-pixel paths, {variant}")
        if key == (4, 1):
            assert_canonical(img, "chart_spp2_b8" if ns == 2 else "chart_odd_spp5_b6", p, key)


def test_whole_pixel_paths_d6m0_canonical(ort, cr, want):
    upload(cr, (6, 0))
    p = CS.chart_params(ort, 96, 64, num_samples=2, max_depth=4)
    for mode in (1, 0):
        with options(cr, pixel_paths=mode):
            img = cr.render(p)
            assert_bits(img, want((6, 0), 96, 64, 2, 4), f"d6 m0, pixel paths {mode}")
            assert_canonical(img, "chart_d6m0_spp2_b4", p, (6, 0))


def test_whole_pixel_paths_heavy_first(ort, cr, want):
    """A repeated frame: from the second one on the blocks go by the frame before's class lists."""
    upload(cr)
    p = CS.chart_params(ort, 96, 64, num_samples=2, max_depth=8)
    with options(cr, pixel_paths=1, pixel_speculate=0, pixel_heavy_first=1):
        for k in range(3):
            assert_bits(cr.render(p), want((4, 1), 96, 64, 2, 8), f"heavy first, frame {k + 1}")


# ---- speculating frames -----------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [(97, 63, 5, 6), (96, 64, 8, 6)], ids=["odd_5x6", "8x6"])
def test_speculating_frames(ort, want, frame):
    """Four frames of one pose on one context: from the second on the samples are traced in
    parallel from the frame before's RNG end states (three launches) -- each material draws
    another number of random numbers, and the absorbed paths none after their end.  Then the
    camera turns by half a degree for a frame and comes back."""
    W, H, ns, md = frame
    s, t = CS.scene(4, 1)
    p = CS.chart_params(ort, W, H, num_samples=ns, max_depth=md)
    turned = CS.chart_params(ort, W, H, num_samples=ns, max_depth=md, yaw=CS.YAW + 0.5)
    ref = want((4, 1), W, H, ns, md)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_pixel_paths(1)
        r.set_pixel_speculate(1)
        seen = []
        for k in range(4):
            img = r.render(p)
            seen.append(launches(r))
            assert_bits(img, ref, f"speculating {ns} x {md}, frame {k + 1}")
            if ns == 5:
                assert_canonical(img, "chart_odd_spp5_b6", p, (4, 1))
        print(f"chart {ns} x {md}: launches per frame {seen}")
        assert seen[0] == 1 and seen[1:] == [3, 3, 3], seen
        assert_bits(r.render(turned), want((4, 1), W, H, ns, md, 1, CS.YAW + 0.5), "turned by half a degree")
        assert_bits(r.render(p), ref, "back at the first pose")
        assert_bits(r.render(p), ref, "back at the first pose, second frame")


# ---- output formats ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1], ids=["pipeline", "pixel_paths"])
def test_rgba8_and_band_tile(ort, cr, want, mode):
    from octreeraytracer_amd.distributed import rank_tile
    upload(cr)
    p = CS.chart_params(ort, 96, 64, num_samples=2, max_depth=8)
    ref = want((4, 1), 96, 64, 2, 8)
    with options(cr, pixel_paths=mode):
        rgba = cr.render(p, format="rgba8")
        assert rgba.dtype == np.uint8 and rgba.shape == (64, 96, 4)
        assert np.array_equal(rgba[..., :3], to_srgb8(ref)) and (rgba[..., 3] == 255).all()
        tile = rank_tile(96, 64, 1, 3)  # bands of rows 16-31 and 64-79: the second lies past the frame
        ys = tile.pixel_rows(64)
        inside = ys < 64
        assert inside.sum() == 16 and (~inside).sum() == 16
        band = np.full((tile.rows, 96, 3), np.float32(7.0))
        cr.render(p, tile, out=band)
        assert_bits(band[inside], ref[ys[inside]], "band tile")
        assert not band[~inside].view(np.uint32).any(), "band tile: padding rows"
        band8 = np.full((tile.rows, 96, 4), FILL, np.uint8)
        cr.render(p, tile, out=band8, format="rgba8")
        assert np.array_equal(band8[inside], rgba[ys[inside]]) and not band8[~inside].any()


# ---- counters ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("explicit", [False, True], ids=["compact", "explicit"])
def test_count_traffic(ort, oracle, cr, explicit):
    s, t = upload(cr, explicit=explicit)
    for ns, md in ((1, 1), (2, 4)):
        p = CS.chart_params(ort, 96, 64, num_samples=ns, max_depth=md)
        _, rc = oracle.render(s, t, p, counts=True)
        assert cr.count_traffic(p) == rc, (ns, md)
        assert rc["accepted_hits"] > 0 and (md == 1 or rc["traversals"] > rc["pixels"])


# ---- ray queries ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CS.QUERY_CONFIGS))
def test_ray_queries(cr, name):
    """t against the oracle's intersectScene, sphere and normal against the host query emulation,
    all exact; with and without ORT_QUERY_SORT."""
    depth, m, explicit, use_octree = CS.QUERY_CONFIGS[name]
    upload(cr, (depth, m), explicit=explicit)
    rays, _ = CS.query_rays()
    ref, (et, es, en) = CS.query_reference(name)
    for sort in (False, True):
        tt, sph, nrm = cr.trace_rays(rays, use_octree=use_octree, sort=sort, normals=True)
        hit = sph >= 0
        assert np.array_equal(hit, ref[:, 0] == 1), (name, sort)
        assert np.array_equal(tt.view(np.int32)[hit], ref[hit, 1]), (name, sort)
        assert (tt.view(np.int32)[~hit] == 0).all() and (sph[~hit] == -1).all() and not nrm[~hit].view(np.int32).any()
        bad = np.nonzero(sph != es)[0]
        assert bad.size == 0, (name, sort, bad[:5], sph[bad[:5]], es[bad[:5]])
        assert np.array_equal(tt.view(np.int32), et.view(np.int32)), (name, sort)
        assert np.array_equal(nrm.view(np.int32), en.view(np.int32)), (name, sort)


# ---- the GPU octree builder -------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(CS.TREES), ids=lambda k: f"d{k[0]}m{k[1]}")
def test_gpu_builder(ort, cr, want, key):
    """A negative radius shrinks the sphere's centre +- radius bounds; the two concentric pairs
    and the identical pair tie in sphereIntersectsBox."""
    from test_gpu_build import same_tree, sha
    s, host = CS.scene(*key)
    cr.build_scene(s, key[0], key[1], keep_tree=True)
    t = cr.export_octree()
    assert (t.n_nodes, t.n_indices) == CS.TREES[key]
    assert same_tree(t, host)
    e = json.loads((G / "manifest.json").read_text())["trees"][f"chart_d{key[0]}_m{key[1]}"]
    assert (e["nodes"], e["indices"]) == CS.TREES[key] and sha(t.gpu_records(), t.object_indices) == e["sha256"]
    assert cr.info()["layout"] == "compact"
    ns, md, canon = (2, 8, "chart_spp2_b8") if key == (4, 1) else (2, 4, "chart_d6m0_spp2_b4")
    p = CS.chart_params(ort, 96, 64, num_samples=ns, max_depth=md)
    img = cr.render(p)
    assert_bits(img, want(key, 96, 64, ns, md), "frame of the GPU-built scene")
    assert_canonical(img, canon, p, key)


# ---- frames without bounces -------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["compact", "explicit", "brute"])
def test_no_bounce_frames(ort, oracle, cr, want, variant):
    """max_depth <= 0 (PipeArgs::nobounce; whole-pixel paths refuse max_depth < 1, so these are
    pipeline frames): every channel 1.0, RGBA8 all 255, band padding zero, the oracle's counters;
    and an ordinary pipeline frame before and after on the same context keeps its bits -- the
    frame in between must leave the counter sets and lists as the next one expects them."""
    s, t = upload(cr, explicit=variant == "explicit")
    use_octree = int(variant != "brute")
    plain = CS.chart_params(ort, 96, 64, num_samples=2, max_depth=4, use_octree=use_octree)
    plain_ref = want((4, 1), 96, 64, 2, 4, use_octree)
    tile = ort.Tile(0, 48, 16, 32, 16, 32)  # two bands: rows 16-31, then rows 48-63, past the frame
    ys = tile.pixel_rows(32)
    assert (ys < 32).sum() == 16 and (ys >= 32).sum() == 16
    with options(cr, pixel_paths=0):
        assert_bits(cr.render(plain), plain_ref, f"{variant}: the frame before")
        for ns in (1, 3):
            for md in (0, -1):
                what = f"{variant}, {ns} samples, max_depth {md}"
                p = CS.chart_params(ort, 48, 32, num_samples=ns, max_depth=md, use_octree=use_octree)
                img = cr.render(p)
                assert img.shape == (32, 48, 3) and (img.view(np.uint32) == 0x3F800000).all(), what
                rgba = cr.render(p, format="rgba8")
                assert rgba.shape == (32, 48, 4) and (rgba == 255).all(), what
                band = np.full((tile.rows, 48, 3), np.float32(7.0))
                cr.render(p, tile, out=band)
                assert (band[ys < 32].view(np.uint32) == 0x3F800000).all(), what
                assert not band[ys >= 32].view(np.uint32).any(), what + ": padding rows"
                _, rc = oracle.render(s, t if use_octree else None, p, counts=True)
                assert cr.count_traffic(p) == rc, what
                assert_bits(cr.render(plain), plain_ref, f"{what}: the frame after")
    if variant == "compact":
        p0 = CS.chart_params(ort, 48, 32, num_samples=3, max_depth=0)
        assert_canonical(cr.render(p0), "chart_md0_spp3", p0, (4, 1))


# ---- frames without samples are refused -------------------------------------------------------------

REFUSAL = "num_samples must be at least 1"


def sentinel(n_bytes):
    import torch
    buf = torch.full((n_bytes,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return buf


def untouched(buf):
    import torch
    torch.cuda.synchronize()
    return bool((buf == FILL).all().item())


@pytest.mark.parametrize("ns", [0, -2])
def test_no_samples_is_refused(ort, cr, want, ns):
    """ort_render, ort_render_ex and ort_count_traffic: ORT_ERR_INVALID_ARG with the message, a
    sentinel-filled device output unchanged, the next valid frame bit-exact.  On a final_out frame
    (compact layout, max_depth > 1, pixel paths off) and on the others."""
    upload(cr)
    lib, ctx = cr._lib, cr._ctx
    good = CS.chart_params(ort, 96, 64, num_samples=2, max_depth=4)
    ref = want((4, 1), 96, 64, 2, 4)
    buf = sentinel(64 * 96 * 12)
    for mode in (0, -1):
        for md in (4, 1, 0):
            with options(cr, pixel_paths=mode):
                bad = CS.chart_params(ort, 96, 64, num_samples=ns, max_depth=md)
                pc, tc = bad.to_c(), ort.Tile.full(bad).to_c()
                what = f"num_samples {ns}, max_depth {md}, pixel paths {mode}"
                rc = lib.ort_render(ctx, C.byref(pc), C.byref(tc), C.c_void_p(buf.data_ptr()), 1, None)
                assert rc == L.ORT_ERR_INVALID_ARG and REFUSAL in lib.ort_last_error(ctx).decode(), what
                for fmt in (L.ORT_FORMAT_RGB32F, L.ORT_FORMAT_RGBA8):
                    o = L.OrtOutput(buf.data_ptr(), 1, fmt, L.ORT_PLACE_TILE, 0, 0)
                    rc = lib.ort_render_ex(ctx, C.byref(pc), C.byref(tc), C.byref(o), None)
                    assert rc == L.ORT_ERR_INVALID_ARG and REFUSAL in lib.ort_last_error(ctx).decode(), what
                counts = (C.c_uint64 * L.ORT_COUNT_N)(*([77] * L.ORT_COUNT_N))
                rc = lib.ort_count_traffic(ctx, C.byref(pc), C.byref(tc), counts)
                assert rc == L.ORT_ERR_INVALID_ARG and REFUSAL in lib.ort_last_error(ctx).decode(), what
                assert list(counts) == [77] * L.ORT_COUNT_N, what
                with pytest.raises(ort.OrtError, match=REFUSAL) as e:  # host output: Renderer.render
                    cr.render(bad)
                assert e.value.code == L.ORT_ERR_INVALID_ARG
                with pytest.raises(ort.OrtError, match=REFUSAL):
                    cr.count_traffic(bad)
                assert untouched(buf), what
                assert_bits(cr.render(good), ref, f"the frame after a refused {what}")


@pytest.mark.parametrize("ns", [0, -2])
def test_no_samples_is_refused_by_a_group(ort, want, ns):
    """ort_group_submit[_fmt] and ort_group_render[_fmt] on [0, 0] with the copy transport: refused
    before any rank has rendered; the group and its slot stay usable."""
    import torch
    from octreeraytracer_amd.group import TRANSPORT_COPY, RenderGroup
    s, t = CS.scene(4, 1)
    good = CS.chart_params(ort, 96, 64, num_samples=2, max_depth=4)
    ref = want((4, 1), 96, 64, 2, 4)
    bad = CS.chart_params(ort, 96, 64, num_samples=ns, max_depth=4).to_c()
    buf = sentinel(64 * 96 * 12)
    ptr = C.c_void_p(buf.data_ptr())
    with RenderGroup([0, 0], TRANSPORT_COPY) as g:
        g.upload(s, t)
        lib, gp = g._lib, g._g
        for round_ in range(2):
            rendered = [len(g.frame_trace_times_ms(rank, 8)) for rank in (0, 1)]
            tk = C.c_int64(-5)
            calls = {"ort_group_submit": lambda: lib.ort_group_submit(gp, C.byref(bad), ptr, 1, C.byref(tk)),
                     "ort_group_submit_fmt": lambda: lib.ort_group_submit_fmt(gp, C.byref(bad), ptr, 1, L.ORT_FORMAT_RGBA8,
                                                                              C.byref(tk)),
                     "ort_group_render": lambda: lib.ort_group_render(gp, C.byref(bad), ptr, 1),
                     "ort_group_render_fmt": lambda: lib.ort_group_render_fmt(gp, C.byref(bad), ptr, 1, L.ORT_FORMAT_RGB32F)}
            for name, call in calls.items():
                assert call() == L.ORT_ERR_INVALID_ARG, name
                assert REFUSAL in lib.ort_group_last_error(gp).decode(), name
                assert tk.value == -5, name  # no ticket was given out
            assert untouched(buf)
            assert [len(g.frame_trace_times_ms(rank, 8)) for rank in (0, 1)] == rendered  # no rank rendered
            # the group and its slot go on: a synchronous frame, then a submitted one
            assert_bits(g.render(good), ref, f"group frame after the refusals, round {round_ + 1}")
            out = torch.zeros((64, 96, 3), dtype=torch.float32, device="cuda:0")
            g.wait(g.submit(good, out))
            assert_bits(out.cpu().numpy(), ref, f"submitted group frame, round {round_ + 1}")
