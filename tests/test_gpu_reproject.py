"""Temporal reprojection on the GPU (ort_history_*, include/ort.h): the kernel's records and outputs
equal the host emulation's bit for bit (which tests/test_reproject.py pins to the numpy restatement)
on every sequence of tests/reproject_sets.py after every update -- host pointers, device tensors, a
colour pitch, a caller's stream, outputs partly left out, guard cells behind every output; two
histories on one context; frames, queries, denoises and accumulation passes around an update are the
ones without it; reset and scene upload; the refusals; the moving-camera loop end to end.  Every
comparison is exact (two NaNs in the same place are equal)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import denoise_sets as ds
import ray_sets
import reproject_sets as rs
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import (camera_query_host, denoise_host, history_update_host, radiance_rays_host,
                                           rng_states)
from reproject_sets import same
from test_gpu_ray_query import make_renderer

pytestmark = pytest.mark.gpu

F = np.float32
VARIANTS = ("host", "device", "pitch", "stream", "partial")
ALPHA, TOL = 0.2, 0.1
GUARD = 7


@pytest.fixture(scope="module")
def bare(ort):
    """A renderer without a scene: an update needs none."""
    r = ort.Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("seq", rs.sequence_names())
def test_gpu_equals_the_emulation(bare, seq, variant):
    """All three outputs after every update: the colour and the length are the {r, g, b, n} record, and
    the moments and the stored hit records show in the next updates' variance and tap tests."""
    import torch
    r = bare
    em = rs.emulated(seq, ALPHA, TOL)
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")  # noqa: E731
    p0, tile0 = rs.sequence(seq)[0][:2]
    rows, width = tile0.rows, tile0.width
    n = rows * width
    stream = torch.cuda.Stream(device="cuda:0") if variant == "stream" else None
    s_arg = dict(stream=stream.cuda_stream) if stream else {}
    with r.history(width, rows) as hist:
        assert hist.info()["device_bytes"] == 64 * n and hist.info()["updates"] == 0
        for k, (p, tile, img, rays, t, sph) in enumerate(rs.sequence(seq)):
            _, e_col, e_var, e_len = em[k]
            what = (seq, variant, rs.STEPS[k])
            rec = ds.records(t, sph)
            kw = dict(alpha=ALPHA, depth_tolerance=TOL)
            if variant == "host":
                src, g_r, g_t, g_s = np.array(img), np.array(rays), np.array(t), np.array(sph)
                col = np.full(3 * n + GUARD, -7.0, F)
                var = np.full(n + GUARD, -7.0, F)
                ln = np.full(n + GUARD, -7.0, F)
                got = hist.update(src, p, tile, (g_r, (g_t, g_s)), out=col, variance=var, length=ln, **kw)
                assert got[0] is col and got[1] is var and got[2] is ln
                assert same(src, img) and same(g_r, rays) and same(g_t, t) and np.array_equal(g_s, sph), what
                o_col, o_var, o_len = col, var, ln
            else:
                if variant == "pitch":
                    wide = torch.full((rows, width + 5, 3), float("nan"), dtype=torch.float32, device="cuda:0")
                    wide[:, :width] = dev(img)
                    d_img = wide[:, :width]
                else:
                    d_img = dev(img)
                d_rays, d_rec = dev(rays), dev(rec)
                col = torch.full((3 * n + GUARD,), -7.0, dtype=torch.float32, device="cuda:0")
                var = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device="cuda:0")
                ln = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device="cuda:0")
                torch.cuda.synchronize()
                if variant == "partial":  # each output left out in turn; the history advances all the same
                    leave = k % 3
                    got = hist.update(d_img, p, tile, (d_rays, d_rec), out=False if leave == 0 else col,
                                      variance=False if leave == 1 else var, length=False if leave == 2 else ln, **kw)
                    assert len(got) == 2
                else:
                    hist.update(d_img, p, tile, (d_rays, d_rec), out=col, variance=var, length=ln, **kw, **s_arg)
                (stream or torch.cuda).synchronize()
                assert same(d_img.cpu().numpy(), img) and same(d_rays.cpu().numpy(), rays), what
                assert np.array_equal(d_rec.cpu().numpy(), rec), what
                o_col, o_var, o_len = col.cpu().numpy(), var.cpu().numpy(), ln.cpu().numpy()
                if variant == "partial":
                    left = (o_col, o_var, o_len)[k % 3]
                    assert (left == -7.0).all(), what
            for o, e, m in ((o_col, e_col, 3 * n), (o_var, e_var, n), (o_len, e_len, n)):
                assert (o[m:] == -7.0).all(), what + ("guard cells",)
                if variant == "partial" and (o[:m] == -7.0).all():
                    continue
                assert same(o[:m], e.reshape(-1)), what
            assert hist.info()["updates"] == k + 1
            assert hist.last_update_ms() > 0.0
        assert hist.info()["device_bytes"] == 64 * n + (n * (12 + 24 + 8 + 12 + 4 + 4) if variant == "host" else 0)


def test_two_histories_on_one_context_do_not_disturb_each_other(bare):
    a_seq, b_seq = "compact5-37x21", "brute-64x8"
    em_a, em_b = rs.emulated(a_seq, ALPHA, TOL), rs.emulated(b_seq, ALPHA, TOL)
    with bare.history(37, 21) as ha, bare.history(64, 8) as hb:
        for k in range(5):
            for hist, seq, em in ((ha, a_seq, em_a), (hb, b_seq, em_b)):
                p, tile, img, rays, t, sph = rs.sequence(seq)[k]
                col, var, ln = hist.update(np.array(img), p, tile, (np.array(rays), (t, sph)), alpha=ALPHA, depth_tolerance=TOL,
                                           length=True)
                assert same(col, em[k][1]) and same(var, em[k][2]) and same(ln, em[k][3]), (seq, k)


def test_work_around_an_update_is_the_work_without_it(ort):
    name = "compact10"
    p = dataclasses.replace(ds.params(name, 64, 8), num_samples=4)
    img, t, sph, nrm = ds.inputs(name, 64, 8)
    seq = rs.sequence("compact10-64x8")
    r = make_renderer(ort, name)
    try:
        frame0 = r.render(p)
        q0 = r.trace_camera(p, normals=True, rays=True)
        d0 = r.denoise(np.array(img), ((t, sph), nrm), iterations=3)
        with r.accumulate(p) as acc, r.history(64, 8) as hist:
            a0 = acc.step(2)
            for pp, tile, im, rays, tt, ss in seq[:3]:
                hist.update(np.array(im), pp, tile, (np.array(rays), (tt, ss)))
            a1 = acc.step(2)
            hist.update(np.array(seq[3][2]), seq[3][0], seq[3][1])   # guides traced here: a camera query of its own
        frame1 = r.render(p)
        q1 = r.trace_camera(p, normals=True, rays=True)
        d1 = r.denoise(np.array(img), ((t, sph), nrm), iterations=3)
        assert same(frame0, frame1) and same(a1, frame0) and not same(a0, a1) and same(d0, d1)
        for x, y in zip(q0, q1):
            assert same(x, y)
    finally:
        r.close()


def test_reset_and_scene_upload_make_a_first_update(ort):
    name = "compact5"
    seq = rs.sequence("compact5-37x21")
    em = rs.emulated("compact5-37x21", ALPHA, TOL)
    s, tree, _ = ray_sets.scene(name)
    r = make_renderer(ort, name)
    kw = dict(alpha=ALPHA, depth_tolerance=TOL, length=True)

    def upd(hist, k):
        p, tile, img, rays, t, sph = seq[k]
        return hist.update(np.array(img), p, tile, (np.array(rays), (t, sph)), **kw)

    try:
        with r.history(37, 21) as hist:
            first = rs.host(None, *seq[1][2:], seq[1][0], seq[1][1], ALPHA, TOL)
            for how in ("reset", "upload", "build"):
                got = upd(hist, 0)
                assert same(got[0], em[0][1]) and (got[2] == 1).all()
                got = upd(hist, 1)
                assert same(got[0], em[1][1]) and same(got[1], em[1][2]) and hist.info()["updates"] == 2
                if how == "reset":
                    hist.reset()
                elif how == "upload":
                    r.upload(s, tree)
                else:
                    r.build_scene(s, 5, 1)
                assert hist.info()["updates"] == 0
                got = upd(hist, 1)   # the same frame again, now without a previous one
                assert same(got[0], first[1]) and same(got[1], first[2]) and same(got[2], first[3]), how
                hist.reset()
    finally:
        r.close()


def test_refusals_leave_the_outputs_and_the_history_untouched(ort, bare):
    r = bare
    lib = r._lib
    seq = rs.sequence("compact5-37x21")
    em = rs.emulated("compact5-37x21", ALPHA, TOL)
    p, tile, img, rays, t, sph = seq[0]
    h = C.c_void_p()
    for w, rows in ((-1, 4), (4, -1), (1 << 16, (1 << 14) + 1)):
        assert lib.ort_history_begin(r._ctx, w, rows, C.byref(h)) == L.ORT_ERR_INVALID_ARG and not h
    assert lib.ort_history_begin(None, 4, 4, C.byref(h)) == L.ORT_ERR_INVALID_ARG
    assert lib.ort_history_begin(r._ctx, 4, 4, None) == L.ORT_ERR_INVALID_ARG
    assert lib.ort_history_free(r._ctx, None) == L.ORT_OK
    other = ort.Renderer(0)
    try:
        with r.history(37, 21) as hist, other.history(37, 21) as foreign:
            kw = dict(alpha=ALPHA, depth_tolerance=TOL)
            hist.update(np.array(img), p, tile, (np.array(rays), (t, sph)), **kw)
            out = np.full((21, 37, 3), F(-3.0))
            var = np.full((21, 37), F(-3.0))
            g = (np.array(seq[1][3]), (seq[1][4], seq[1][5]))
            im1, p1, tile1 = np.array(seq[1][2]), seq[1][0], seq[1][1]
            bad = [dict(alpha=1.5), dict(alpha=-0.1), dict(alpha=float("nan")), dict(depth_tolerance=-1.0),
                   dict(depth_tolerance=float("nan"))]
            for b in bad:
                with pytest.raises(ort.OrtError) as e:
                    hist.update(im1, p1, tile1, g, out=out, variance=var, **dict(kw, **b))
                assert e.value.code == 1, b
            for bad_tile, image in ((ort.Tile(0, 36, 0, 21), im1[:, :36]), (ort.Tile(0, 37, 0, 20), im1[:20]),
                                    (ort.Tile(0, 37, 0, 21, band_height=7, band_stride=14), im1),
                                    (ort.Tile(1, 37, 0, 21), im1)):
                gg = (g[0][:image.shape[0], :image.shape[1]], (g[1][0][:image.shape[0], :image.shape[1]],
                                                              g[1][1][:image.shape[0], :image.shape[1]]))
                with pytest.raises(ort.OrtError) as e:
                    hist.update(np.ascontiguousarray(image), p1, bad_tile, (np.ascontiguousarray(gg[0]), gg[1]),
                                out=out.reshape(-1), variance=var.reshape(-1), **kw)
                assert e.value.code == 1, bad_tile
            with pytest.raises(ort.OrtError) as e:   # params that ort_render refuses
                hist.update(im1, dataclasses.replace(p1, num_samples=0), tile1, g, out=out, variance=var, **kw)
            assert e.value.code == 1
            # the raw frame: flags, reserved, alignment, a bad pitch, NULL inputs, a history of another context
            rec = ds.records(seq[1][4], seq[1][5])
            pc, tc = p1.to_c(), tile1.to_c()

            def frame():
                f = L.OrtHistoryFrame()
                f.params, f.tile = C.pointer(pc), C.pointer(tc)
                f.color, f.rays, f.hits = im1.ctypes.data, g[0].ctypes.data, rec.ctypes.data
                f.out_color, f.out_variance = out.ctypes.data, var.ctypes.data
                f.alpha, f.depth_tolerance = ALPHA, TOL
                return f

            cases = []
            f = frame(); f.flags = 2; cases.append(f)
            f = frame(); f.reserved[0] = 1; cases.append(f)
            f = frame(); f.color = im1.ctypes.data + 2; cases.append(f)
            f = frame(); f.out_color = out.ctypes.data + 1; cases.append(f)
            f = frame(); f.color_pitch_bytes = 12 * 37 - 4; cases.append(f)
            f = frame(); f.color_pitch_bytes = 12 * 37 + 2; cases.append(f)
            f = frame(); f.color = None; cases.append(f)
            f = frame(); f.rays = None; cases.append(f)
            f = frame(); f.hits = None; cases.append(f)
            f = frame(); f.params = None; cases.append(f)
            f = frame(); f.tile = None; cases.append(f)
            for i, f in enumerate(cases):
                assert lib.ort_history_update(r._ctx, hist._h, C.byref(f), None) == L.ORT_ERR_INVALID_ARG, i
            f = frame()
            assert lib.ort_history_update(r._ctx, foreign._h, C.byref(f), None) == L.ORT_ERR_INVALID_ARG
            assert lib.ort_history_update(r._ctx, hist._h, None, None) == L.ORT_ERR_INVALID_ARG
            assert lib.ort_history_update(r._ctx, None, C.byref(f), None) == L.ORT_ERR_INVALID_ARG
            assert lib.ort_history_update(None, hist._h, C.byref(f), None) == L.ORT_ERR_INVALID_ARG
            assert lib.ort_history_reset(r._ctx, foreign._h) == L.ORT_ERR_INVALID_ARG
            assert lib.ort_history_free(r._ctx, foreign._h) == L.ORT_ERR_INVALID_ARG
            assert (out == F(-3.0)).all() and (var == F(-3.0)).all()
            assert hist.info()["updates"] == 1
            # the history is where the first update left it: the second update is the emulation's second
            col, v = hist.update(im1, p1, tile1, g, **kw)
            assert same(col, em[1][1]) and same(v, em[1][2])
            # all three outputs left out is allowed and advances the history
            p2, tile2, img2, rays2, t2, sph2 = seq[2]
            assert hist.update(np.array(img2), p2, tile2, (np.array(rays2), (t2, sph2)), out=False, variance=False, **kw) is None
            p3, tile3, img3, rays3, t3, sph3 = seq[3]
            col, v = hist.update(np.array(img3), p3, tile3, (np.array(rays3), (t3, sph3)), **kw)
            assert same(col, em[3][1]) and same(v, em[3][2])
    finally:
        other.close()


def test_a_history_of_no_pixels_launches_nothing(ort, bare):
    p = ds.params("compact5", 37, 21)
    with bare.history(37, 0) as hist:
        assert hist.info() == {"width": 37, "rows": 0, "updates": 0, "device_bytes": 0}
        out = hist.update(np.zeros((0, 37, 3), F), p, ort.Tile(0, 37, 0, 0),
                          (np.zeros((0, 37, 6), F), np.zeros((0, 37, 2), np.int32)), length=True)
        assert [o.shape for o in out] == [(0, 37, 3), (0, 37), (0, 37)]
        assert hist.info()["updates"] == 1
        with pytest.raises(ort.OrtError) as e:
            hist.last_update_ms()
        assert e.value.code == 1


@pytest.mark.parametrize("name", ("compact5", "brute"))
def test_moving_camera_loop_end_to_end(ort, name):
    """sample -> trace_camera -> update -> denoise(variance, gamma) on device tensors equals the same
    chain through the host twins, pose after pose."""
    import torch
    w, h = 37, 21
    s, tree, _ = ray_sets.scene(name)
    use_octree = rs.CONFIGS[name][1]
    r = make_renderer(ort, name)
    try:
        with r.history(w, h) as hist:
            state = None
            for k, pose in enumerate(rs.poses(name)[:4]):
                p = rs.params(name, w, h, pose)
                # the host twins
                first, _, _ = camera_query_host(s, tree if use_octree else None, p, which="first_sample")
                st = rng_states(w * h, seed=k)
                rad = radiance_rays_host(s, tree if use_octree else None, first.reshape(-1, 6), st, max_depth=ds.DEPTH,
                                         use_octree=bool(use_octree)).reshape(h, w, 3)
                rays, tt, sph, nrm = camera_query_host(s, tree if use_octree else None, p, which="pixel_centre", normals=True)
                state, col, var, _ = history_update_host(state, rad, p, None, (rays, (tt, sph)))
                want = denoise_host(col, ((tt, sph), nrm), variance=var, gamma=True)
                # the device
                d_rays1 = torch.empty((h, w, 6), dtype=torch.float32, device="cuda:0")
                r.trace_camera(p, which="first_sample", rays=d_rays1, hits=False)
                d_rad = r.trace_radiance(d_rays1.reshape(-1, 6), torch.from_numpy(st).to("cuda:0"), max_depth=ds.DEPTH,
                                         use_octree=bool(use_octree)).reshape(h, w, 3)
                d_hits, d_nrm, d_rays = r.trace_camera(p, which="pixel_centre", rays=True, normals=True,
                                                       out=torch.empty((h, w, 2), dtype=torch.int32, device="cuda:0"))
                d_col, d_var = hist.update(d_rad, p, None, (d_rays, d_hits))
                got = r.denoise(d_col, (d_hits, d_nrm), variance=d_var, gamma=True)
                torch.cuda.synchronize()
                assert same(d_rad.cpu().numpy(), rad), (name, k)
                assert same(d_col.cpu().numpy(), col) and same(d_var.cpu().numpy(), var), (name, k)
                assert same(got.cpu().numpy(), want), (name, k)
    finally:
        r.close()
