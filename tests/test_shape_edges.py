"""Frames and tiles at the kernels' unit sizes, on the CPU (no GPU needed): the host emulation of
the kernels' per-pixel code against the oracle, bit for bit, on every shape and tile of
tests/shape_sets.py; the table's camera condition; the group's partition with more ranks than
bands; the denoiser and the accumulations' moments on images of a few pixels; and the row limit of
include/ort.h (ort_tile): tiles whose rows pass pixel row 2^31 - 1 are refused by the emulation and
the oracle alike, the largest accepted ones are all zeros."""
import numpy as np
import pytest

import denoise_sets as ds
import shape_sets as SS
import variance_sets as vs
from octreeraytracer_amd import _lib as L

F = np.float32
ALL = SS.cases("ABCDEFGHI", tiles=True)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- the emulation equals the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("case_id,shape", [pytest.param(c, s, id=f"{c}-{s[0]}spp{s[1]}b") for c in ALL for s in SS.SAMPLES
                                           if SS.CASES[c].group != "I" or s == (1, 1)])  # group I: primary rays only
def test_emulation_equals_the_oracle(ort, case_id, shape):
    from octreeraytracer_amd.renderer import emulate_render_host
    c = SS.CASES[case_id]
    s, t = SS.scene()
    for use_octree in (1, 0):
        ref = SS.frame(case_id, shape, use_octree)
        assert np.isfinite(ref).all() and ref.shape == (c.tile[3], c.tile[1], 3)
        assert (ref[~c.inside()] == 0).all()
        for layout in (L.ORT_LAYOUT_COMPACT, L.ORT_LAYOUT_EXPLICIT):
            got, counts = emulate_render_host(s, t if use_octree else None, SS.params(case_id, shape, use_octree), c.ort_tile(),
                                              layout=layout)
            bad = int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
            assert bad == 0, f"{case_id} {shape} octree={use_octree} layout={layout}: {bad} pixels differ from the oracle"
            assert np.isfinite(got).all()
            assert counts["pixels"] == int(c.inside().sum()) * c.tile[1]


@pytest.mark.parametrize("case_id", SS.cases("ABCDEFGHI"))
def test_every_shapes_camera_sees_spheres(case_id):
    c = SS.CASES[case_id]
    seen = []
    for ns in (1, 2, 5):
        _, _, sphere, _ = SS.camera(case_id, "first_sample", ns)
        assert SS.camera_condition(c.pixels, sphere) == "", (case_id, ns)
        seen.append((int((sphere >= 0).sum()), len(np.unique(sphere[sphere >= 0]))))
    print(f"{case_id}: pitch {c.pitch} zoom {c.zoom} yaw {c.yaw:+}: (hits, spheres) at 1, 2, 5 samples {seen}")


def test_the_chart_camera_misses_on_the_extreme_shapes(ort):
    """Why the table has cameras: under the chart's own these shapes compare sky with sky."""
    import chart_scenes as CS
    from octreeraytracer_amd.renderer import camera_query_host
    s, t = SS.scene()
    for w, h in ((1, 1), (1, 2), (2, 1), (31, 1), (300, 1), (256, 1)):
        _, _, sphere = camera_query_host(s, t, CS.chart_params(ort, w, h))
        assert (sphere < 0).all(), (w, h)


# ---- the group: more ranks than bands ------------------------------------------------------------------
@pytest.mark.parametrize("w,h,world", [(20, 5, 3), (33, 16, 8), (1, 1, 2), (7, 17, 4)])
def test_group_emulation_with_ranks_past_the_frame(ort, oracle, w, h, world):
    import chart_scenes as CS
    from octreeraytracer_amd.distributed import rank_tile
    from octreeraytracer_amd.group import emulate_group_host
    s, t = SS.scene()
    past = [r for r in range(world) if (rank_tile(w, h, r, world).pixel_rows(h) >= h).all()]
    assert past, "some ranks' tiles lie wholly past the frame"
    for shape in ((1, 1), (2, 4)):
        p = CS.chart_params(ort, w, h, num_samples=shape[0], max_depth=shape[1])
        assert same_bits(emulate_group_host(s, t, p, world), oracle.render(s, t, p)), (w, h, world, shape)


# ---- the denoiser on a few pixels ----------------------------------------------------------------------
@pytest.mark.parametrize("iterations", (1, 3, 6))
@pytest.mark.parametrize("w,h", SS.DENOISE_SMALL, ids=lambda v: str(v))
def test_denoise_emulation_equals_numpy_on_a_few_pixels(w, h, iterations):
    img, t, sph, n = SS.denoise_inputs(w, h)
    for terms in (SS.TERMS_OFF, SS.TERMS_ON):
        want = ds.atrous(img, t, sph, n, iterations=iterations, **terms)
        got = ds.host(img, t, sph, n, iterations=iterations, **terms)
        assert ds.same(got, want), (w, h, iterations, terms)
        assert ds.same(SS.denoised(w, h, iterations, "on" if terms is SS.TERMS_ON else "off"), want)
    for name in ("same_sphere", "normal_power", "sigma_color", "sigma_depth"):  # each term alone
        kw = dict(SS.TERMS_OFF, **{name: SS.TERMS_ON[name]})
        assert ds.same(ds.host(img, t, sph, n, iterations=iterations, **kw), ds.atrous(img, t, sph, n, iterations=iterations, **kw)), name
    v = SS.denoise_variance(w, h)
    assert ds.same(vs.host_var(img, t, sph, n, v, 2.0, iterations=iterations, **SS.TERMS_ON),
                   vs.atrous_var(img, t, sph, n, v, 2.0, iterations=iterations, **SS.TERMS_ON))


# ---- moments and adaptive counts at the unit sizes -----------------------------------------------------
THR, MIN, FLOOR = 0.05, 2, 0.05   # tests/test_gpu_adaptive.py's criterion


@pytest.mark.parametrize("case_id", SS.cases("ABCD"))
def test_moments_and_adaptive_agree_with_the_preview(case_id):
    """As tests/test_variance.py at its sizes: gamma(mean) after k samples is the preview emulation's
    picture bit for bit, the variance is -1 at k = 1 and finite and >= 0 after; an adaptive run of
    passes (1, 1, rest) without a criterion is the moments accumulation, and with one every pixel's
    moments are its own count's prefix."""
    N, depth = 5, 4
    shape = (N, depth)
    for k in range(1, N + 1):
        mean, var = SS.moments(case_id, shape, k)
        assert ds.same(vs.gamma(mean), SS.preview(case_id, shape, k)), (case_id, k)
        assert (var == F(-1)).all() if k == 1 else (np.isfinite(var).all() and (var >= 0).all()), (case_id, k)
    assert same_bits(SS.preview(case_id, shape, N), SS.frame(case_id, shape))
    plain = SS.adaptive(case_id, shape, ((1, 0, 0.0, FLOOR), (1, 0, 0.0, FLOOR), (N - 2, 0, 0.0, FLOOR)))
    assert (plain[0] == N).all() and same_bits(plain[1], SS.moments(case_id, shape, N)[0])
    assert same_bits(plain[2], SS.moments(case_id, shape, N)[1])
    counts, mean, var = SS.adaptive(case_id, shape, ((1, MIN, THR, FLOOR), (1, MIN, THR, FLOOR), (N - 2, MIN, THR, FLOOR)))
    assert ((counts == 2) | (counts == N)).all(), np.unique(counts)
    for k in np.unique(counts):
        at = counts == k
        m, v = SS.moments(case_id, shape, int(k))
        assert same_bits(mean[at], m[at]) and same_bits(var[at], v[at]), (case_id, int(k))


# ---- the row limit ---------------------------------------------------------------------------------------
def limit_params(ort, shape=(1, 1), use_octree=1):
    import chart_scenes as CS
    return CS.chart_params(ort, *SS.LIMIT_FRAME, num_samples=shape[0], max_depth=shape[1], use_octree=use_octree)


def emulation_calls(ort, tile):
    """name -> call: every emulation entry point that takes a tile."""
    from octreeraytracer_amd import renderer as R
    s, t = SS.scene()
    p = limit_params(ort, (2, 2))
    return {
        "emulate_render": lambda: R.emulate_render_host(s, t, p, tile),
        "emulate_render_explicit": lambda: R.emulate_render_host(s, t, p, tile, layout=L.ORT_LAYOUT_EXPLICIT),
        "emulate_render_brute": lambda: R.emulate_render_host(s, None, limit_params(ort, (1, 1), 0), tile),
        "emulate_render_prefix": lambda: R.emulate_render_host(s, t, p, tile, samples_done=1),
        "camera_query": lambda: R.camera_query_host(s, t, p, tile, normals=True),
        "camera_rays": lambda: R.camera_query_host(None, None, p, tile, hits=False),
        "accum_moments": lambda: R.accum_moments_host(s, t, p, tile, samples_done=1),
        "accum_adaptive": lambda: R.accum_adaptive_host(s, t, p, tile, passes=[(1, 0, 0.0, FLOOR)]),
    }


@pytest.mark.parametrize("name", SS.REFUSED_TILES)
def test_tiles_past_the_row_limit_are_refused(ort, oracle, name):
    tile = ort.Tile(*SS.REFUSED_TILES[name])
    ys = tile.pixel_rows(SS.LIMIT_FRAME[1])
    assert ys.dtype == np.int64 and ys.max() > SS.INT_MAX and (np.diff(ys) > 0).all()
    for what, call in emulation_calls(ort, tile).items():
        with pytest.raises(ort.OrtError) as e:
            call()
        assert e.value.code == L.ORT_ERR_INVALID_ARG and "2^31 - 1" in str(e.value), (name, what, str(e.value))
    s, t = SS.scene()
    x0, w, y0, rows, bh, bs = SS.REFUSED_TILES[name]
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        oracle.render(s, t, limit_params(ort), x0, y0, w, rows, bh, bs)
    # the C entry point itself refuses too, and leaves the output alone
    import ctypes as C
    out = np.full((rows, w, 3), F(-7.0))
    keep = SS.scene()
    sc = oracle.OracleScene()
    pr = oracle.make_params(limit_params(ort, (1, 1)))
    pr.use_octree = 0
    cr = [np.ascontiguousarray(a, F) for a in (keep[0].center_radius, keep[0].mat_albedo, keep[0].fuzz_ri)]
    sc.sphere_center_radius, sc.sphere_mat_albedo, sc.sphere_fuzz_ri = (a.ctypes.data_as(C.POINTER(C.c_float)) for a in cr)
    sc.n_spheres = cr[0].shape[0]
    rc = oracle.lib().oracle_render(C.byref(sc), C.byref(pr), x0, y0, w, rows, bh, bs, out.ctypes.data_as(C.POINTER(C.c_float)),
                                    None, 1)
    assert rc != 0 and (out == F(-7.0)).all()


def test_a_refused_emulation_leaves_its_output_untouched(ort):
    import ctypes as C
    s, t = SS.scene()
    lib = L.analysis_lib()
    p = limit_params(ort).to_c()
    for name, tl in SS.REFUSED_TILES.items():
        tile = ort.Tile(*tl).to_c()
        out = np.full((tl[3], tl[1], 3), F(-7.0))
        counts = (C.c_uint64 * L.ORT_COUNT_N)(*([99] * L.ORT_COUNT_N))
        cr, ma, fr = (np.ascontiguousarray(a, F) for a in (s.center_radius, s.mat_albedo, s.fuzz_ri))
        rc = lib.ort_debug_emulate_render(L.fptr(cr), L.fptr(ma), L.fptr(fr), s.n, None, None, None, None, None, 0, None, 0,
                                          L.ORT_LAYOUT_COMPACT, C.byref(p), C.byref(tile), L.fptr(out), counts)
        assert rc == L.ORT_ERR_INVALID_ARG and (out == F(-7.0)).all() and list(counts) == [99] * L.ORT_COUNT_N, name


@pytest.mark.parametrize("name", SS.LARGEST_TILES)
def test_the_largest_accepted_tiles_are_all_zeros(ort, oracle, name):
    tl = SS.LARGEST_TILES[name]
    tile = ort.Tile(*tl)
    ys = tile.pixel_rows(SS.LIMIT_FRAME[1])
    assert ys.max() == SS.INT_MAX and ys.min() >= SS.LIMIT_FRAME[1]
    s, t = SS.scene()
    x0, w, y0, rows, bh, bs = tl
    ref = oracle.render(s, t, limit_params(ort, (2, 2)), x0, y0, w, rows, bh, bs)
    assert ref.shape == (rows, w, 3) and (ref.view(np.uint32) == 0).all()
    for what, call in emulation_calls(ort, tile).items():
        got = call()
        if what.startswith("emulate_render"):
            assert (got[0].view(np.uint32) == 0).all() and got[1]["pixels"] == 0, (name, what)
        elif what == "camera_query":
            rays, tt, sph, nrm = got
            assert (rays == 0).all() and (tt == 0).all() and (sph == -1).all() and (nrm == 0).all(), name
        elif what == "camera_rays":
            assert (got == 0).all(), name
        elif what == "accum_moments":
            assert (got[0] == 0).all() and (got[1] == F(-1)).all(), name
        else:
            assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == F(-1)).all(), name
