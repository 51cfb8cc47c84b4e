"""Temporal reprojection on the CPU (ort_history_update, include/ort.h): the host emulation
(ort_debug_history_update: reproject.inc's reproject_pixel, the kernel's own per-pixel function) equals
the float32 numpy restatement of tests/reproject_sets.py bit for bit on every sequence after every
update; the camera steps leave neither all nor none of the history; the running mean, the reset, a
non-finite sample, untouched inputs; every refusal of a frame; and what the history buys on a slowly
moving camera.  No GPU needed."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import denoise_sets as ds
import ray_sets
import reproject_sets as rs
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import (DEFAULT_DEPTH_TOLERANCE, DEFAULT_HISTORY_ALPHA, camera_query_host, denoise_host,
                                           gamma_host, history_update_host, radiance_rays_host, rng_states)
from reproject_sets import same

F = np.float32


@pytest.mark.parametrize("depth_tolerance", rs.DEPTH_TOLERANCES)
@pytest.mark.parametrize("alpha", rs.ALPHAS)
@pytest.mark.parametrize("seq", rs.sequence_names())
def test_emulation_equals_the_restatement(seq, alpha, depth_tolerance):
    em = rs.emulated(seq, alpha, depth_tolerance)
    state = None
    for k, (p, tile, img, rays, t, sph) in enumerate(rs.sequence(seq)):
        state, col, var, length, _ = rs.update(state, img, rays, t, sph, p, tile, alpha, depth_tolerance)
        e_state, e_col, e_var, e_len = em[k]
        what = (seq, alpha, depth_tolerance, rs.STEPS[k])
        assert same(e_state[2], state[2]), what + ("{r, g, b, n}",)
        assert same(e_state[3], state[3]), what + ("{m1, m2, t, sphere}",)
        assert same(e_col, col) and same(e_var, var) and same(e_len, length), what + ("outputs",)


@pytest.mark.parametrize("depth_tolerance", rs.DEPTH_TOLERANCES)
@pytest.mark.parametrize("seq", [s for s in rs.sequence_names() if s.split("-")[0] in rs.SCENES])
def test_the_camera_steps_keep_some_history_and_lose_some(seq, depth_tolerance):
    """On the restatement itself: a test of all-reset frames, or of frames that never reset, would
    pass on much less."""
    state, share = None, {}
    for k, (p, tile, img, rays, t, sph) in enumerate(rs.sequence(seq)):
        state, _, _, length, have = rs.update(state, img, rays, t, sph, p, tile, 0.2, depth_tolerance)
        share[rs.STEPS[k]] = float(have.mean())  # (every pixel of these frames is inside the frame)
    print(seq, depth_tolerance, share)
    assert share["first"] == 0.0
    for step in ("translation", "rotation"):
        assert 0.5 <= share[step] <= 0.99, (seq, step, share)
    assert share["same"] == 1.0
    assert share["jump"] <= 0.5, share


def test_same_camera_with_alpha_0_is_the_running_mean():
    p, tile, _, rays, t, sph = rs.sequence("compact5-37x21")[0]
    rng = np.random.default_rng(5)
    samples = [rng.random((tile.rows, tile.width, 3), dtype=F) for _ in range(9)]
    state = None
    for k, s in enumerate(samples, 1):
        state, col, var, length = rs.host(state, s, rays, t, sph, p, tile, 0.0, 0.1)
        assert (length == k).all()
        mean = np.mean(np.stack(samples[:k]).astype(np.float64), axis=0)
        # k blends of one rounding each and the rounded weights 1/n: a few ulp of values below 1
        assert np.abs(col - mean).max() <= 4 * k * np.finfo(F).eps
        assert ((var == -1) if k == 1 else (var >= 0)).all()
    # the variance of the mean, as ort_accum_read_moments defines it: (m2/k - m1^2) / (k - 1)
    lum = np.stack([rs.lum(s) for s in samples]).astype(np.float64)
    want = ((lum ** 2).mean(axis=0) - lum.mean(axis=0) ** 2) / (len(samples) - 1)
    assert np.abs(var - want).max() <= 1e-5


def test_a_reset_makes_a_first_update():
    """Stateless emulation: no state is a first update whatever came before; the history objects'
    reset and scene upload are tests/test_gpu_reproject.py's."""
    seq = rs.sequence("compact10-37x21")
    p, tile, img, rays, t, sph = seq[2]
    first = rs.host(None, img, rays, t, sph, p, tile, 0.2, 0.1)
    assert (first[3] == 1).all() and (first[2] == -1).all() and same(first[1], img)
    after = rs.emulated("compact10-37x21", 0.2, 0.1)[2]
    assert not same(after[1], first[1])


def test_a_non_finite_sample_leaves_the_previous_values():
    p, tile, img, rays, t, sph = rs.sequence("brute-37x21")[0]
    state, col0, _, _ = rs.host(None, img, rays, t, sph, p, tile, 0.2, 0.1)
    bad = np.array(img)
    bad[3, 4, 1] = np.nan
    bad[5, 6, 2] = np.inf
    state2, col, var, length = rs.host(state, bad, rays, t, sph, p, tile, 0.2, 0.1)
    for y, x in ((3, 4), (5, 6)):
        assert same(state2[2][y, x], state[2][y, x]) and same(state2[3][y, x, :2], state[3][y, x, :2])
        assert length[y, x] == 1 and same(col[y, x], col0[y, x])
    assert (length[0] == 2).all()
    # without history: zeros and n = 0
    state3, col3, var3, len3 = rs.host(None, bad, rays, t, sph, p, tile, 0.2, 0.1)
    assert (col3[3, 4] == 0).all() and len3[3, 4] == 0 and var3[3, 4] == -1 and (state3[3][3, 4, :2] == 0).all()


def test_inputs_are_never_written():
    for seq in ("synthetic", "tile"):
        state = None
        for p, tile, img, rays, t, sph in rs.sequence(seq):
            keep = [np.array(a) for a in (img, rays, t, sph)]
            given = [np.array(a) for a in keep]
            before = state
            prev = None if state is None else (np.array(state[2]), np.array(state[3]))
            state, *_ = rs.host(state, *given, p, tile, 0.2, 0.1)
            for a, b in zip(keep, given):
                assert same(a, b)
            if prev is not None:  # the previous records neither
                assert same(prev[0], before[2]) and same(prev[1], before[3])


def _frame(p, tile, img, rays, rec, col, var, length):
    f = L.OrtHistoryFrame()
    f.params, f.tile = C.pointer(p), C.pointer(tile)
    f.color, f.rays, f.hits = img.ctypes.data, rays.ctypes.data, rec.ctypes.data
    f.out_color, f.out_variance, f.out_length = col.ctypes.data, var.ctypes.data, length.ctypes.data
    f.alpha, f.depth_tolerance = 0.2, 0.1
    return f


REFUSALS = ("alpha_high", "alpha_negative", "alpha_nan", "tolerance_negative", "tolerance_nan", "flags", "reserved",
            "misaligned_color", "misaligned_out", "pitch_short", "pitch_odd", "banded", "tile_outside", "no_samples",
            "zero_height", "null_params", "null_tile", "null_color", "null_rays", "null_hits", "null_frame", "on_device")


@pytest.mark.parametrize("case", REFUSALS)
def test_the_emulation_refuses_what_the_update_refuses(case):
    """ORT_ERR_INVALID_ARG with the outputs and the next records untouched.  (The refusals that need a
    history object -- its shape, its context, its size at begin -- are tests/test_gpu_reproject.py's.)"""
    lib = L.analysis_lib()
    pp, tl, img, rays, t, sph = rs.sequence("compact5-37x21")[1]
    img, rays, rec = np.array(img), np.array(rays), ds.records(t, sph)
    n = tl.rows * tl.width
    col, var, length = (np.full(k * n + 1, -3.0, F) for k in (3, 1, 1))
    na, nb = np.full(4 * n, -3.0, F), np.full(4 * n, -3.0, F)
    prev = rs.emulated("compact5-37x21", 0.2, 0.1)[0][0]
    p, tile = pp.to_c(), tl.to_c()
    f = _frame(p, tile, img, rays, rec, col, var, length)
    fp = C.byref(f)
    if case == "alpha_high":
        f.alpha = 1.0001
    elif case == "alpha_negative":
        f.alpha = -0.1
    elif case == "alpha_nan":
        f.alpha = float("nan")
    elif case == "tolerance_negative":
        f.depth_tolerance = -1e-3
    elif case == "tolerance_nan":
        f.depth_tolerance = float("nan")
    elif case == "flags":
        f.flags = 1
    elif case == "reserved":
        f.reserved[2] = 7
    elif case == "misaligned_color":
        f.color = img.ctypes.data + 2
    elif case == "misaligned_out":
        f.out_variance = var.ctypes.data + 1
    elif case == "pitch_short":
        f.color_pitch_bytes = 12 * tl.width - 4
    elif case == "pitch_odd":
        f.color_pitch_bytes = 12 * tl.width + 2
    elif case == "banded":
        tile.band_height, tile.band_stride = 7, 14
    elif case == "tile_outside":
        tile.x0 = 1
    elif case == "no_samples":
        p.num_samples = 0
    elif case == "zero_height":
        p.height = 0
    elif case == "null_params":
        f.params = None
    elif case == "null_tile":
        f.tile = None
    elif case == "null_color":
        f.color = None
    elif case == "null_rays":
        f.rays = None
    elif case == "null_hits":
        f.hits = None
    elif case == "null_frame":
        fp = None
    elif case == "on_device":
        f.on_device = 1
    prev_p = prev[0].to_c()
    rc = lib.ort_debug_history_update(C.byref(prev_p), 0, 0, L.fptr(np.array(prev[2])), L.fptr(np.array(prev[3])), fp,
                                      L.fptr(na), L.fptr(nb))
    assert rc == L.ORT_ERR_INVALID_ARG, case
    for a in (col, var, length, na, nb):
        assert (a == -3.0).all(), case


def test_all_outputs_null_still_makes_the_records_and_no_pixels_is_ok():
    lib = L.analysis_lib()
    pp, tl, img, rays, t, sph = rs.sequence("compact5-37x21")[0]
    img, rays, rec = np.array(img), np.array(rays), ds.records(t, sph)
    n = tl.rows * tl.width
    na, nb = np.empty((tl.rows, tl.width, 4), F), np.empty((tl.rows, tl.width, 4), F)
    p, tile = pp.to_c(), tl.to_c()
    f = _frame(p, tile, img, rays, rec, np.empty(1, F), np.empty(1, F), np.empty(1, F))
    f.out_color = f.out_variance = f.out_length = None
    assert lib.ort_debug_history_update(None, 0, 0, None, None, C.byref(f), L.fptr(na), L.fptr(nb)) == L.ORT_OK
    want = rs.emulated("compact5-37x21", 0.2, 0.1)[0][0]
    assert same(na, want[2]) and same(nb, want[3])
    tile.rows = 0
    f.color = f.rays = f.hits = None
    assert lib.ort_debug_history_update(None, 0, 0, None, None, C.byref(f), None, None) == L.ORT_OK


# ---- what it buys: compact5 at 96 x 64, a slow translation over 8 poses, per-frame-seeded one-path
# samples of 8 bounces; the last update against the oracle's 256-sample frame at the last pose.
BUYS = dict(name="compact5", w=96, h=64, poses=8, step=(0.02, 0.005, 0.0))
# integrated / raw MSE (through the gamma) that the emulation gives here with the defaults: it is
# deterministic, the margin is for later changes of the defaults only
BUYS_RATIO = 0.2359


@functools.lru_cache(maxsize=None)
def buys_frames():
    from oracle import oracle
    name, w, h = BUYS["name"], BUYS["w"], BUYS["h"]
    s, t, _ = ray_sets.scene(name)
    base = rs.poses(name)[0]
    out = []
    for k in range(BUYS["poses"]):
        pose = dict(base, position=tuple(float(a + k * b) for a, b in zip(base["position"], BUYS["step"])))
        p = rs.params(name, w, h, pose)
        first, _, _ = camera_query_host(s, t, p, which="first_sample")
        rad = radiance_rays_host(s, t, first.reshape(-1, 6), rng_states(w * h, seed=k), max_depth=ds.DEPTH).reshape(h, w, 3)
        rays, tt, sph, nrm = camera_query_host(s, t, p, which="pixel_centre", normals=True)
        out.append((p, rad, rays, tt, sph, nrm))
    ref = np.asarray(oracle.render(s, t, dataclasses.replace(out[-1][0], num_samples=256)), F).reshape(h, w, 3)
    return out, ref


def test_what_the_history_buys_on_a_slowly_moving_camera():
    frames, ref = buys_frames()
    assert (DEFAULT_HISTORY_ALPHA, DEFAULT_DEPTH_TOLERANCE) == (0.1, 0.1)
    state = None
    for p, rad, rays, tt, sph, nrm in frames:
        state, col, var, length = history_update_host(state, rad, p, None, (rays, (tt, sph)))
    raw = ds.mse(gamma_host(rad), ref)
    integrated = ds.mse(gamma_host(col), ref)
    plain = ds.mse(denoise_host(rad, ((tt, sph), nrm), gamma=True), ref)
    chain = ds.mse(denoise_host(col, ((tt, sph), nrm), variance=var, gamma=True), ref)
    print(f"MSE against the 256-sample frame: raw {raw:.6f}, integrated {integrated:.6f} (ratio {integrated / raw:.4f}); "
          f"denoised one sample {plain:.6f}, update -> denoise {chain:.6f} (ratio {chain / plain:.4f}); "
          f"mean history length {float(length.mean()):.2f}")
    assert integrated / raw < 1.0
    assert integrated / raw <= BUYS_RATIO * 1.25
    assert chain < plain  # (recorded in DESIGN.md 4.17; the filter after the history must not undo it)
