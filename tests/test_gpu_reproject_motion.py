"""Temporal reprojection that follows moving spheres, on the GPU (ort_history_update_ex with
ORT_HISTORY_MOTION, include/ort.h): the kernel's outputs equal the host emulation's bit for bit (which
tests/test_reproject_motion.py pins to the numpy restatement) after every update of every animated
sequence of tests/reproject_motion_sets.py -- host pointers, device tensors, a colour pitch, a
caller's stream, guard cells behind every output, the scene uploaded or built anew before every
update; the snapshot's 16 bytes per sphere; flags 0 is the plain call; the state rules against the host
twin with every `updates` value; the refusals; the work around a MOTION update; the animated loop end
to end and what it buys.  Every comparison is exact (two NaNs in the same place are equal)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import denoise_sets as ds
import ray_sets
import reproject_motion_sets as ms
import reproject_sets as rs
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import denoise_host, gamma_host, history_update_host
from reproject_motion_sets import same
from test_gpu_ray_query import make_renderer
from test_ray_query import CONFIGS

pytestmark = pytest.mark.gpu

F = np.float32
VARIANTS = ("host", "device", "pitch", "stream", "built")
GUARD = 7
KW = dict(alpha=ms.ALPHA, depth_tolerance=ms.TOL)


def renderer_for(ort, name):
    r = ort.Renderer(0)
    if CONFIGS[name][0] == L.ORT_LAYOUT_EXPLICIT:
        r.set_layout(L.ORT_LAYOUT_EXPLICIT)
    return r


# ("built": the scene built on the GPU before every update; brute force has no tree to build)
CASES = [(seq, v) for seq in ms.sequence_names() for v in VARIANTS if v != "built" or CONFIGS[ms.SEQUENCES[seq][0]][1]]


@pytest.mark.parametrize("seq,variant", CASES)
def test_gpu_equals_the_emulation(ort, seq, variant):
    import torch
    name = ms.SEQUENCES[seq][0]
    em = ms.emulated(seq)
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")  # noqa: E731
    tile0 = ms.inputs(seq, 0)[1]
    rows, width = tile0.rows, tile0.width
    n = rows * width
    stream = torch.cuda.Stream(device="cuda:0") if variant == "stream" else None
    s_arg = dict(stream=stream.cuda_stream) if stream else {}
    _, _, depth, per_node = ray_sets.SCENES[name]
    r = renderer_for(ort, name)
    try:
        with r.history(width, rows) as hist:
            assert hist.info()["device_bytes"] == 64 * n
            for k, (p, tile, img, rays, t, sph, now) in enumerate(ms.sequence(seq)):
                s, tree = ms.spheres_at(seq, k)
                if variant == "built":   # the GPU builder keeps the upload order of the spheres too
                    r.build_scene(s, depth, per_node)
                else:
                    r.upload(s, tree)
                assert hist.info()["updates"] == 0
                _, e_col, e_var, e_len = em[k]
                what = (seq, variant, ms.STEPS[k])
                rec = ds.records(t, sph)
                if variant == "host":
                    col, var, ln = (np.full(m * n + GUARD, -7.0, F) for m in (3, 1, 1))
                    hist.update(np.array(img), p, tile, (np.array(rays), (np.array(t), np.array(sph))), out=col, variance=var,
                                length=ln, motion=True, **KW)
                    o_col, o_var, o_len = col, var, ln
                else:
                    if variant == "pitch":
                        wide = torch.full((rows, width + 5, 3), float("nan"), dtype=torch.float32, device="cuda:0")
                        wide[:, :width] = dev(img)
                        d_img = wide[:, :width]
                    else:
                        d_img = dev(img)
                    d_rays, d_rec = dev(rays), dev(rec)
                    col, var, ln = (torch.full((m * n + GUARD,), -7.0, dtype=torch.float32, device="cuda:0") for m in (3, 1, 1))
                    torch.cuda.synchronize()
                    hist.update(d_img, p, tile, (d_rays, d_rec), out=col, variance=var, length=ln, motion=True, **KW, **s_arg)
                    (stream or torch.cuda).synchronize()
                    assert same(d_img.cpu().numpy(), img) and same(d_rays.cpu().numpy(), rays), what
                    assert np.array_equal(d_rec.cpu().numpy(), rec), what
                    o_col, o_var, o_len = col.cpu().numpy(), var.cpu().numpy(), ln.cpu().numpy()
                for o, e, m in ((o_col, e_col, 3 * n), (o_var, e_var, n), (o_len, e_len, n)):
                    assert (o[m:] == -7.0).all(), what + ("guard cells",)
                    assert same(o[:m], e.reshape(-1)), what
                assert hist.info()["updates"] == k + 1
                assert hist.last_update_ms() > 0.0
                # the snapshot: 16 bytes per sphere from the first MOTION update on, and nothing more later
                staging = n * (12 + 24 + 8 + 12 + 4 + 4) if variant == "host" else 0
                assert hist.info()["device_bytes"] == 64 * n + 16 * len(now) + staging, what
    finally:
        r.close()


def _raw_frame(seq_step, col, var, ln):
    p, tile, img, rays, t, sph = seq_step[:6]
    keep = dict(p=p.to_c(), tile=tile.to_c(), img=np.array(img), rays=np.array(rays), rec=ds.records(t, sph))
    f = L.OrtHistoryFrameEx()
    b = f.base
    b.params, b.tile = C.pointer(keep["p"]), C.pointer(keep["tile"])
    b.color, b.rays, b.hits = keep["img"].ctypes.data, keep["rays"].ctypes.data, keep["rec"].ctypes.data
    b.out_color, b.out_variance, b.out_length = col.ctypes.data, var.ctypes.data, ln.ctypes.data
    b.alpha, b.depth_tolerance = ms.ALPHA, ms.TOL
    return f, keep


def test_flags_0_is_the_plain_call_bit_for_bit(ort):
    """Records (seen through the next updates), outputs, state and `updates`, with and without a scene,
    across a scene upload (both forget) and on the sequences of the plain call's own tests."""
    r = ort.Renderer(0)
    lib = r._lib
    try:
        for seq in ("compact5-37x21", "synthetic", "tile"):
            steps = rs.sequence(seq)
            em = rs.emulated(seq, ms.ALPHA, ms.TOL)
            tile0 = steps[0][1]
            n = tile0.rows * tile0.width
            with r.history(tile0.width, tile0.rows) as hx, r.history(tile0.width, tile0.rows) as hp:
                for k, step in enumerate(steps):
                    outs = []
                    for h, ex in ((hx, True), (hp, False)):
                        col, var, ln = np.full(3 * n, -7.0, F), np.full(n, -7.0, F), np.full(n, -7.0, F)
                        f, keep = _raw_frame(step, col, var, ln)
                        if ex:
                            rc = lib.ort_history_update_ex(r._ctx, h._h, C.byref(f), None)
                        else:
                            rc = lib.ort_history_update(r._ctx, h._h, C.byref(f.base), None)
                        assert rc == L.ORT_OK, (seq, k, ex)
                        outs.append((col, var, ln))
                    for x, y, e in zip(outs[0], outs[1], em[k][1:]):
                        assert same(x, y) and same(x, e.reshape(-1)), (seq, k)
                    assert hx.info() == hp.info() and hx.info()["updates"] == k + 1
                    if k == 2 and seq == "compact5-37x21":
                        s, tree, _ = ray_sets.scene("compact5")
                        r.upload(s, tree)
                        assert hx.info()["updates"] == 0 and hp.info()["updates"] == 0
                        break
                if seq == "compact5-37x21":   # after the upload both start again, as today
                    col = hx.update(np.array(steps[1][2]), steps[1][0], steps[1][1], (np.array(steps[1][3]), steps[1][4:6]),
                                    length=True, **KW)
                    assert (col[2] == 1).all() and hx.info()["updates"] == 1
    finally:
        r.close()


SCRIPT = (
    # (op, step): the state rules of include/ort.h, one after another on one history
    ("upload", 0), ("motion", 0), ("upload", 1), ("motion", 1),            # revived
    ("upload", 2), ("upload", 3), ("upload", 2), ("motion", 2),            # several uploads in a row: still revived
    ("motion", 2),                                                          # not stale: the snapshot equals the scene
    ("fewer", 3), ("motion", 3),                                            # another sphere count: no previous frame
    ("upload", 4), ("motion", 4),                                           # the count of the snapshot before last: none either
    ("upload", 3), ("plain", 3), ("motion", 3),                             # a plain update forgets, then no snapshot
    ("plain", 3), ("upload", 4), ("motion", 4),                             # ... and drops the stale mark's chance
    ("motion", 4), ("reset", 0), ("motion", 4),                             # reset clears everything
    ("motion", 4), ("upload", 0), ("reset", 0), ("motion", 0),              # stale, then reset
)
SCRIPT_UPDATES = (0, 1, 0, 2, 0, 0, 0, 3, 4, 0, 1, 0, 1, 0, 1, 2, 3, 0, 1, 2, 0, 1, 2, 0, 0, 1)


def test_the_state_rules_against_the_host_twin(ort):
    seq = "compact5-37x21"
    name = ms.SEQUENCES[seq][0]
    twin = ms.HostHistory()
    r = renderer_for(ort, name)
    try:
        with r.history(37, 21) as hist:
            for i, (op, k) in enumerate(SCRIPT):
                s, tree = ms.spheres_at(seq, k)
                p, tile, img, rays, t, sph, now = ms.inputs(seq, k)
                if op in ("upload", "fewer"):
                    if op == "fewer":   # the last sphere left out: none of A, B, C, and in no leaf the tile sees first
                        cut = ort.SphereSet(s.center_radius[:-1].copy(), s.mat_albedo[:-1].copy(), s.fuzz_ri[:-1].copy())
                        r.upload(cut, ort.build_octree(cut, *ray_sets.SCENES[name][2:]))
                        twin.upload(cut.center_radius)
                    else:
                        r.upload(s, tree)
                        twin.upload(now)
                elif op == "reset":
                    hist.reset()
                    twin.reset()
                else:
                    got = hist.update(np.array(img), p, tile, (np.array(rays), (t, sph)), length=True, motion=op == "motion", **KW)
                    want = twin.update(img, rays, t, sph, p, tile, op == "motion")
                    for x, y in zip(got, want):
                        assert same(x, y), (i, op, k)
                assert hist.info()["updates"] == twin.updates == SCRIPT_UPDATES[i], (i, op, k)
    finally:
        r.close()


def test_refusals_leave_the_outputs_and_the_history_untouched(ort):
    seq = "compact5-37x21"
    em = ms.emulated(seq)
    steps = ms.sequence(seq)
    n = 37 * 21
    r = renderer_for(ort, "compact5")
    lib = r._lib
    try:
        with r.history(37, 21) as hist:
            col, var, ln = np.full(3 * n, -3.0, F), np.full(n, -3.0, F), np.full(n, -3.0, F)
            # MOTION without a scene: ORT_ERR_NO_SCENE, nothing allocated
            f, keep = _raw_frame(steps[0], col, var, ln)
            f.base.flags = L.ORT_HISTORY_MOTION
            assert lib.ort_history_update_ex(r._ctx, hist._h, C.byref(f), None) == L.ORT_ERR_NO_SCENE
            assert hist.info()["updates"] == 0 and hist.info()["device_bytes"] == 64 * n
            with pytest.raises(ort.OrtError) as e:
                hist.update(np.array(steps[0][2]), steps[0][0], steps[0][1], (np.array(steps[0][3]), steps[0][4:6]), motion=True)
            assert e.value.code == L.ORT_ERR_NO_SCENE
            r.upload(*ms.spheres_at(seq, 0))
            assert lib.ort_history_update_ex(r._ctx, hist._h, C.byref(f), None) == L.ORT_OK
            assert same(col, em[0][1].reshape(-1)) and hist.info()["updates"] == 1
            col[:], var[:], ln[:] = -3.0, -3.0, -3.0
            r.upload(*ms.spheres_at(seq, 1))
            cases = []
            f, k1 = _raw_frame(steps[1], col, var, ln); f.base.flags = 2; cases.append(f)
            f, k2 = _raw_frame(steps[1], col, var, ln); f.base.flags = 3; cases.append(f)
            f, k3 = _raw_frame(steps[1], col, var, ln); f.base.flags = 1; f.reserved[0] = 1; cases.append(f)
            f, k4 = _raw_frame(steps[1], col, var, ln); f.base.flags = 1; f.reserved[3] = 1; cases.append(f)
            f, k5 = _raw_frame(steps[1], col, var, ln); f.base.flags = 1; f.base.reserved[2] = 1; cases.append(f)
            f, k6 = _raw_frame(steps[1], col, var, ln); f.base.flags = 1; f.base.alpha = 2.0; cases.append(f)
            for i, f in enumerate(cases):
                assert lib.ort_history_update_ex(r._ctx, hist._h, C.byref(f), None) == L.ORT_ERR_INVALID_ARG, i
            f, k7 = _raw_frame(steps[1], col, var, ln)
            f.base.flags = L.ORT_HISTORY_MOTION   # the plain call still refuses the flag
            assert lib.ort_history_update(r._ctx, hist._h, C.byref(f.base), None) == L.ORT_ERR_INVALID_ARG
            assert lib.ort_history_update_ex(r._ctx, hist._h, None, None) == L.ORT_ERR_INVALID_ARG
            assert lib.ort_history_update_ex(r._ctx, None, C.byref(f), None) == L.ORT_ERR_INVALID_ARG
            assert lib.ort_history_update_ex(None, hist._h, C.byref(f), None) == L.ORT_ERR_INVALID_ARG
            assert (col == -3.0).all() and (var == -3.0).all() and (ln == -3.0).all()
            assert hist.info()["updates"] == 0
            # untouched: the stale history is still revived, and the update is the emulation's second
            assert lib.ort_history_update_ex(r._ctx, hist._h, C.byref(f), None) == L.ORT_OK
            assert same(col, em[1][1].reshape(-1)) and same(var, em[1][2].reshape(-1)) and hist.info()["updates"] == 2
    finally:
        r.close()


def test_work_around_a_motion_update_is_the_work_without_it(ort):
    name = "compact10"
    seq = "compact10-37x21"
    p = dataclasses.replace(ds.params(name, 64, 8), num_samples=4)
    img, t, sph, nrm = ds.inputs(name, 64, 8)
    steps = ms.sequence(seq)
    r = make_renderer(ort, name)
    try:
        frame0 = r.render(p)
        q0 = r.trace_camera(p, normals=True, rays=True)
        d0 = r.denoise(np.array(img), ((t, sph), nrm), iterations=3)
        with r.accumulate(p) as acc, r.history(37, 21) as hist:
            a0 = acc.step(2)
            for pp, tile, im, rays, tt, ss, _ in steps[:2]:   # (the resident scene is step 0's: every sphere unmoved)
                hist.update(np.array(im), pp, tile, (np.array(rays), (tt, ss)), motion=True)
            a1 = acc.step(2)
            hist.update(np.array(steps[0][2]), steps[0][0], steps[0][1], motion=True)   # guides traced here
            assert hist.info()["updates"] == 3
        frame1 = r.render(p)
        q1 = r.trace_camera(p, normals=True, rays=True)
        d1 = r.denoise(np.array(img), ((t, sph), nrm), iterations=3)
        assert same(frame0, frame1) and same(a1, frame0) and not same(a0, a1) and same(d0, d1)
        for x, y in zip(q0, q1):
            assert same(x, y)
    finally:
        r.close()


def test_a_history_of_no_pixels_still_keeps_its_state(ort):
    seq = "compact5-37x21"
    p = ms.inputs(seq, 0)[0]
    r = renderer_for(ort, "compact5")
    try:
        with r.history(37, 0) as hist:
            args = (np.zeros((0, 37, 3), F), p, ort.Tile(0, 37, 0, 0), (np.zeros((0, 37, 6), F), np.zeros((0, 37, 2), np.int32)))
            for k in range(2):
                r.upload(*ms.spheres_at(seq, k))
                hist.update(*args, motion=True)
                assert hist.info() == {"width": 37, "rows": 0, "updates": k + 1, "device_bytes": 16 * 2000}
    finally:
        r.close()


def test_animated_loop_end_to_end_and_what_it_buys(ort):
    """build_scene(new spheres) -> trace_camera -> trace_radiance(rng_states(n, seed=frame)) ->
    update(motion=True) -> denoise(variance, gamma) on device tensors equals the chain through the host
    twins frame after frame, and the figures of DESIGN.md 4.18 hold on the GPU: the MOTION history's
    error is below the one-sample picture's (which is also what a history that forgets at every upload
    shows), by the recorded ratio rounded up to the next 0.05."""
    import torch
    from octreeraytracer_amd.renderer import rng_states
    name, w, h = ms.QUALITY["name"], ms.QUALITY["w"], ms.QUALITY["h"]
    _, _, depth, per_node = ray_sets.SCENES[name]
    raw, motion, raw_dn, motion_dn = [], [], [], []
    state, snap = None, None
    r = ort.Renderer(0)
    try:
        with r.history(w, h) as hist:
            for k, (p, rad, rays, tt, sph, nrm, now, ref, _) in enumerate(ms.quality_frames()):
                # the host twins
                state, col, var, _ = history_update_host(state, rad, p, None, (rays, (tt, sph)), motion=(now, snap))
                snap = now
                want = denoise_host(col, ((tt, sph), nrm), variance=var, gamma=True)
                # the device
                r.build_scene(ms.quality_scene(k)[0], depth, per_node)
                d_first = torch.empty((h, w, 6), dtype=torch.float32, device="cuda:0")
                r.trace_camera(p, which="first_sample", rays=d_first, hits=False)
                d_rad = r.trace_radiance(d_first.reshape(-1, 6), torch.from_numpy(rng_states(w * h, seed=k)).to("cuda:0"),
                                         max_depth=ds.DEPTH).reshape(h, w, 3)
                d_hits, d_nrm, d_rays = r.trace_camera(p, which="pixel_centre", rays=True, normals=True,
                                                       out=torch.empty((h, w, 2), dtype=torch.int32, device="cuda:0"))
                d_col, d_var = hist.update(d_rad, p, None, (d_rays, d_hits), motion=True)
                got = r.denoise(d_col, (d_hits, d_nrm), variance=d_var, gamma=True)
                d_plain = r.denoise(d_rad, (d_hits, d_nrm), gamma=True)
                torch.cuda.synchronize()
                assert hist.info()["updates"] == k + 1
                assert same(d_rad.cpu().numpy(), rad), k
                assert same(d_col.cpu().numpy(), col) and same(d_var.cpu().numpy(), var), k
                assert same(got.cpu().numpy(), want), k
                raw.append(ds.mse(gamma_host(d_rad.cpu().numpy()), ref))
                motion.append(ds.mse(gamma_host(d_col.cpu().numpy()), ref))
                raw_dn.append(ds.mse(d_plain.cpu().numpy(), ref))
                motion_dn.append(ds.mse(got.cpu().numpy(), ref))
    finally:
        r.close()
    a, b = float(np.mean(raw)), float(np.mean(motion))
    print(f"MSE against the 256-sample frames, mean over the 8 steps: one sample {a:.6f}, MOTION history {b:.6f} "
          f"(ratio {b / a:.4f}); denoised {float(np.mean(raw_dn)):.6f} -> {float(np.mean(motion_dn)):.6f}")
    assert b < a
    assert b / a <= ms.QUALITY_RATIO_BOUND
    assert float(np.mean(motion_dn)) < float(np.mean(raw_dn))
