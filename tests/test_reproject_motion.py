"""Temporal reprojection that follows moving spheres, on the CPU (ort_history_update_ex with
ORT_HISTORY_MOTION, include/ort.h): the host emulation (ort_debug_history_update_ex: reproject.inc's
reproject_pixel<true>, the kernel's own per-pixel function) equals the float32 numpy restatement of
tests/reproject_motion_sets.py bit for bit on every animated sequence after every update; the chosen
spheres are in view and are followed; pixels of unmoved spheres and misses are the plain update's;
sphere ids outside the scene; the state rules with every `updates` value; the refusals; and what the
history buys on an animated scene.  No GPU needed."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_sets as ds
import reproject_motion_sets as ms
import reproject_sets as rs
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import denoise_host, gamma_host, history_update_host
from reproject_motion_sets import same

F = np.float32


def test_the_library_has_the_call():
    assert "ort_history_update_ex" in L.EXPORTED_SYMBOLS and hasattr(L.analysis_lib(), "ort_history_update_ex")


@pytest.mark.parametrize("depth_tolerance", (0.0, 0.1))
@pytest.mark.parametrize("alpha", (0.0, 0.2))
@pytest.mark.parametrize("seq", ms.sequence_names())
def test_emulation_equals_the_restatement(seq, alpha, depth_tolerance):
    em = ms.emulated(seq, alpha, depth_tolerance)
    state, snap = None, None
    for k, (p, tile, img, rays, t, sph, now) in enumerate(ms.sequence(seq)):
        state, col, var, length, _, _ = ms.update(state, img, rays, t, sph, p, tile, alpha, depth_tolerance, now, snap)
        snap = now
        e_state, e_col, e_var, e_len = em[k]
        what = (seq, alpha, depth_tolerance, ms.STEPS[k])
        assert same(e_state[2], state[2]), what + ("{r, g, b, n}",)
        assert same(e_state[3], state[3]), what + ("{m1, m2, t, sphere}",)
        assert same(e_col, col) and same(e_var, var) and same(e_len, length), what + ("outputs",)


@pytest.mark.parametrize("seq", ms.sequence_names())
def test_the_chosen_spheres_are_in_view_and_are_followed(seq):
    """On the restatement itself: a sequence whose moved spheres nobody sees would pass on much less.
    A moved sphere's pixels keep most of their history under MOTION and, where the camera rests, would
    keep a history that belongs to another place of the sphere (or to none) without it."""
    a, b, c = ms.chosen(seq)
    state, snap, share = None, None, {}
    for k, (p, tile, img, rays, t, sph, now) in enumerate(ms.sequence(seq)):
        state, _, _, _, have, moved = ms.update(state, img, rays, t, sph, p, tile, ms.ALPHA, ms.TOL, now, snap)
        snap = now
        step = ms.STEPS[k]
        seen = {int(i) for i in np.unique(sph)}
        share[step] = (int(moved.sum()), float(have[moved].mean()) if moved.any() else None)
        if step == "first":
            assert {a, b, c} <= seen and not moved.any()
        elif step == "resting":   # A and B moved; the camera is bitwise the first one
            assert rs.same_camera(ms.inputs(seq, 0)[0], 0, 0, p, 0, 0)
            assert set(np.unique(sph[moved])) == {a, b} & seen and {a, b} & seen
        elif step == "radius":    # A moved on, C changed its radius; the camera moved
            assert set(np.unique(sph[moved])) == {a, c} & seen and {a, c} & seen
        elif step == "away":      # B is nowhere in the tile
            assert b not in seen and not moved.any()
        else:                     # B is back: it differs from the snapshot and finds nothing where it was
            assert b in seen and set(np.unique(sph[moved])) == {b} and not have[moved].any()
    print(seq, share)
    for step in ("resting", "radius"):
        n, followed = share[step]
        assert n >= 3 and followed >= 0.5, (seq, step, share)


@pytest.mark.parametrize("seq", ms.sequence_names())
def test_unmoved_spheres_and_misses_are_the_plain_update(seq):
    em = ms.emulated(seq)
    state, snap = None, None
    for k, (p, tile, img, rays, t, sph, now) in enumerate(ms.sequence(seq)):
        plain = ms.host(state, img, rays, t, sph, p, tile, ms.ALPHA, ms.TOL)
        keep = ~ms.moved_mask(sph, now, snap) if state is not None else np.ones(sph.shape, bool)
        got = em[k]
        for x, y in ((got[0][2], plain[0][2]), (got[0][3], plain[0][3]), (got[1], plain[1]), (got[2], plain[2]),
                     (got[3], plain[3])):
            assert same(x[keep], y[keep]), (seq, ms.STEPS[k])
        if k in (1, 2):   # ... and the moved ones are not: the test above would pass on a flag that does nothing
            assert not same(got[1][~keep], plain[1][~keep]), (seq, ms.STEPS[k])
        state, snap = got[0], now


def test_without_a_snapshot_every_sphere_counts_as_unmoved():
    seq = "compact5-37x21"
    em = ms.emulated(seq)
    p, tile, img, rays, t, sph, now = ms.inputs(seq, 1)
    plain = ms.host(em[0][0], img, rays, t, sph, p, tile, ms.ALPHA, ms.TOL)
    got = ms.host(em[0][0], img, rays, t, sph, p, tile, ms.ALPHA, ms.TOL, (now, None))
    for x, y in zip((got[0][2], got[0][3]) + got[1:], (plain[0][2], plain[0][3]) + plain[1:]):
        assert same(x, y)


def test_sphere_ids_outside_the_scene_count_as_unmoved():
    """Caller-made hit records with ids >= n, -1 and other negative ids: no sphere is read (the arrays
    handed over hold exactly n records) and the pixels are the plain update's."""
    seq = "compact5-37x21"
    em = ms.emulated(seq)
    p, tile, img, rays, t, sph, now = ms.inputs(seq, 1)
    snap = ms.inputs(seq, 0)[6]
    n = len(now)
    odd = np.array(sph)
    ids = (n, n + 5, 2 ** 31 - 1, -1, -7, -2 ** 31)
    cells = [(2 + i, 3 * i + 1) for i in range(len(ids))]
    for (y, x), i in zip(cells, ids):
        odd[y, x] = i
    prev = (em[0][0][0], em[0][0][1], np.array(em[0][0][2]), np.array(em[0][0][3]))
    for (y, x), i in zip(cells, ids):   # a previous record of the same id, so that the pixel has a history to find
        prev[3][y, x, 3] = np.array([i], np.int64).astype(np.int32).view(F)[0]
    got = ms.host(prev, img, rays, t, odd, p, tile, ms.ALPHA, ms.TOL, (now, snap))
    want = ms.update(prev, img, rays, t, odd, p, tile, ms.ALPHA, ms.TOL, now, snap)
    plain = ms.host(prev, img, rays, t, odd, p, tile, ms.ALPHA, ms.TOL)
    assert same(got[0][2], want[0][2]) and same(got[0][3], want[0][3]) and same(got[1], want[1]) and same(got[2], want[2])
    for y, x in cells:
        assert not want[5][y, x]
        assert same(got[0][2][y, x], plain[0][2][y, x]) and same(got[0][3][y, x], plain[0][3][y, x])
        assert got[3][y, x] == 2   # (the resting camera: its own record, same id)


def test_a_scale_that_is_not_finite_leaves_the_pixel_without_history():
    seq = "compact5-37x21"
    em = ms.emulated(seq)
    a = ms.chosen(seq)[0]
    p, tile, img, rays, t, sph, now = ms.inputs(seq, 1)
    for radius, snap_radius in ((0.0, 1.0), (0.0, 0.0), (np.nan, 1.0), (1.0, np.inf)):
        now2, snap = np.array(now), np.array(ms.inputs(seq, 0)[6])
        now2[a, 3], snap[a, 3] = radius, snap_radius
        got = ms.host(em[0][0], img, rays, t, sph, p, tile, ms.ALPHA, ms.TOL, (now2, snap))
        want = ms.update(em[0][0], img, rays, t, sph, p, tile, ms.ALPHA, ms.TOL, now2, snap)
        assert same(got[0][2], want[0][2]) and same(got[2], want[2])
        assert (got[3][sph == a] == 1).all() and (sph == a).any(), (radius, snap_radius)


def test_flags_0_is_the_plain_update():
    lib = L.analysis_lib()
    seq = "compact10-37x21"
    em = ms.emulated(seq)
    pp, tl, img, rays, t, sph, now = ms.inputs(seq, 2)
    plain = ms.host(em[1][0], img, rays, t, sph, pp, tl, ms.ALPHA, ms.TOL)
    f, keep = _frame_ex(pp, tl, img, rays, t, sph)
    f.base.flags = 0
    na, nb = np.empty((tl.rows, tl.width, 4), F), np.empty((tl.rows, tl.width, 4), F)
    prev = em[1][0]
    prev_p = prev[0].to_c()
    # the spheres are not read without the flag: none are given
    assert lib.ort_debug_history_update_ex(C.byref(prev_p), 0, 0, L.fptr(np.array(prev[2])), L.fptr(np.array(prev[3])),
                                           C.byref(f), None, None, 0, L.fptr(na), L.fptr(nb)) == L.ORT_OK
    assert same(na, plain[0][2]) and same(nb, plain[0][3])
    assert same(keep["col"][:-1].reshape(plain[1].shape), plain[1]) and same(keep["var"][:-1].reshape(plain[2].shape), plain[2])


# ---- the state rules: HostHistory drives ort_debug_history_state, the histories' own transitions ----
def _upd(h, seq, k, motion):
    p, tile, img, rays, t, sph, _ = ms.inputs(seq, k)
    return h.update(img, rays, t, sph, p, tile, motion)


def test_state_an_upload_then_a_motion_update_revives():
    seq = "compact5-37x21"
    em = ms.emulated(seq)
    h = ms.HostHistory()
    assert h.updates == 0
    for k in range(3):
        h.upload(ms.inputs(seq, k)[6])
        assert h.updates == 0
        col, var, ln = _upd(h, seq, k, True)
        assert h.updates == k + 1
        assert same(col, em[k][1]) and same(var, em[k][2]) and same(ln, em[k][3])
    assert ln.max() == 3


def test_state_an_upload_with_another_sphere_count_has_no_previous_frame():
    seq = "compact5-37x21"
    h = ms.HostHistory()
    h.upload(ms.inputs(seq, 0)[6])
    _upd(h, seq, 0, True)
    _upd(h, seq, 0, True)
    assert h.updates == 2
    h.upload(ms.inputs(seq, 1)[6][:-1])   # one sphere fewer (the last one is none of A, B, C)
    assert h.updates == 0
    col, var, ln = _upd(h, seq, 1, True)
    assert h.updates == 1 and (ln == 1).all() and (var == -1).all()
    h.upload(ms.inputs(seq, 2)[6][:-1])   # the same count again: revived from the update after the mismatch
    col, var, ln = _upd(h, seq, 2, True)
    assert h.updates == 2 and ln.max() == 2


def test_state_two_uploads_in_a_row_still_revive():
    seq = "brute-37x21"
    em = ms.emulated(seq)
    h = ms.HostHistory()
    h.upload(ms.inputs(seq, 0)[6])
    _upd(h, seq, 0, True)
    h.upload(ms.inputs(seq, 3)[6])
    h.upload(ms.inputs(seq, 2)[6])
    h.upload(ms.inputs(seq, 1)[6])
    assert h.updates == 0
    col, var, ln = _upd(h, seq, 1, True)
    assert h.updates == 2
    assert same(col, em[1][1]) and same(var, em[1][2]) and same(ln, em[1][3])


def test_state_a_plain_update_forgets_as_before_and_drops_the_snapshot():
    seq = "compact5-37x21"
    em = ms.emulated(seq)
    h = ms.HostHistory()
    h.upload(ms.inputs(seq, 0)[6])
    _upd(h, seq, 0, True)
    h.upload(ms.inputs(seq, 1)[6])
    col, var, ln = _upd(h, seq, 1, False)   # a plain update after an upload: a first frame, as today
    assert h.updates == 1 and (ln == 1).all()
    # the next MOTION update has a previous frame and no snapshot: every sphere counts as unmoved
    p, tile, img, rays, t, sph, now = ms.inputs(seq, 1)
    want = ms.host(h.state, img, rays, t, sph, p, tile, ms.ALPHA, ms.TOL)
    col, var, ln = _upd(h, seq, 1, True)
    assert h.updates == 2 and same(col, want[1]) and same(ln, want[3])
    # ... and after a plain update a replacement is final: the stale mark went with the snapshot
    _upd(h, seq, 1, False)
    assert h.updates == 3
    h.upload(ms.inputs(seq, 2)[6])
    col, var, ln = _upd(h, seq, 2, True)
    assert h.updates == 1 and (ln == 1).all()
    assert not same(col, em[2][1])


def test_state_reset_clears_everything():
    seq = "compact5-37x21"
    h = ms.HostHistory()
    h.upload(ms.inputs(seq, 0)[6])
    _upd(h, seq, 0, True)
    _upd(h, seq, 0, True)
    h.reset()
    assert h.updates == 0 and list(h.st) == [0] * 4 + [0, h.st[5]]
    col, var, ln = _upd(h, seq, 1, True)
    assert h.updates == 1 and (ln == 1).all()
    _upd(h, seq, 1, True)
    h.upload(ms.inputs(seq, 2)[6])
    h.reset()                               # stale, then reset: nothing to revive
    col, var, ln = _upd(h, seq, 2, True)
    assert h.updates == 1 and (ln == 1).all()


# ---- refusals -----------------------------------------------------------------------------------------
def _frame_ex(pp, tl, img, rays, t, sph):
    n = tl.rows * tl.width
    keep = dict(p=pp.to_c(), tile=tl.to_c(), img=np.array(img), rays=np.array(rays), rec=ds.records(t, sph),
                col=np.full(3 * n + 1, -3.0, F), var=np.full(n + 1, -3.0, F), len=np.full(n + 1, -3.0, F))
    f = L.OrtHistoryFrameEx()
    b = f.base
    b.params, b.tile = C.pointer(keep["p"]), C.pointer(keep["tile"])
    b.color, b.rays, b.hits = keep["img"].ctypes.data, keep["rays"].ctypes.data, keep["rec"].ctypes.data
    b.out_color, b.out_variance, b.out_length = keep["col"].ctypes.data, keep["var"].ctypes.data, keep["len"].ctypes.data
    b.alpha, b.depth_tolerance = ms.ALPHA, ms.TOL
    b.flags = L.ORT_HISTORY_MOTION
    return f, keep


REFUSALS = ("flags_2", "flags_3", "flags_high", "reserved_base", "reserved_ex", "reserved_ex_last", "no_scene", "alpha",
            "null_color")


@pytest.mark.parametrize("case", REFUSALS)
def test_the_emulation_refuses_what_the_update_refuses(case):
    lib = L.analysis_lib()
    seq = "compact5-37x21"
    pp, tl, img, rays, t, sph, now = ms.inputs(seq, 1)
    f, keep = _frame_ex(pp, tl, img, rays, t, sph)
    now, snap = np.array(now), np.array(ms.inputs(seq, 0)[6])
    now_p, want = L.fptr(now), L.ORT_ERR_INVALID_ARG
    if case == "flags_2":
        f.base.flags = 2
    elif case == "flags_3":
        f.base.flags = 3
    elif case == "flags_high":
        f.base.flags = L.ORT_HISTORY_MOTION | (1 << 30)
    elif case == "reserved_base":
        f.base.reserved[1] = 1
    elif case == "reserved_ex":
        f.reserved[0] = 1
    elif case == "reserved_ex_last":
        f.reserved[3] = -1
    elif case == "no_scene":
        now_p, want = None, L.ORT_ERR_NO_SCENE
    elif case == "alpha":
        f.base.alpha = 1.5
    elif case == "null_color":
        f.base.color = None
    n = tl.rows * tl.width
    na, nb = np.full(4 * n, -3.0, F), np.full(4 * n, -3.0, F)
    prev = ms.emulated(seq)[0][0]
    prev_p = prev[0].to_c()
    rc = lib.ort_debug_history_update_ex(C.byref(prev_p), 0, 0, L.fptr(np.array(prev[2])), L.fptr(np.array(prev[3])),
                                         C.byref(f), now_p, L.fptr(snap), len(now), L.fptr(na), L.fptr(nb))
    assert rc == want, case
    for a in (keep["col"], keep["var"], keep["len"], na, nb):
        assert (a == -3.0).all(), case


def test_the_plain_call_still_refuses_the_flag():
    lib = L.analysis_lib()
    pp, tl, img, rays, t, sph, _ = ms.inputs("compact5-37x21", 0)
    f, keep = _frame_ex(pp, tl, img, rays, t, sph)
    n = tl.rows * tl.width
    na, nb = np.full(4 * n, -3.0, F), np.full(4 * n, -3.0, F)
    assert f.base.flags == 1
    assert lib.ort_debug_history_update(None, 0, 0, None, None, C.byref(f.base), L.fptr(na), L.fptr(nb)) == L.ORT_ERR_INVALID_ARG
    assert (na == -3.0).all() and (keep["col"] == -3.0).all()


# ---- what it buys -------------------------------------------------------------------------------------
def test_what_the_motion_history_buys_on_an_animated_scene():
    q = quality()
    print("MSE against the 256-sample frames, mean over the 8 steps: "
          f"one sample {q['raw']:.6f}, MOTION history {q['motion']:.6f} (ratio {q['motion'] / q['raw']:.4f}); "
          f"denoised one sample {q['raw_denoised']:.6f}, history -> denoise {q['motion_denoised']:.6f} "
          f"(ratio {q['motion_denoised'] / q['raw_denoised']:.4f}); on the moved spheres' pixels "
          f"one sample {q['raw_moved']:.6f}, MOTION {q['motion_moved']:.6f}, a history that is told nothing {q['blind_moved']:.6f}")
    assert q["motion"] < q["raw"]
    assert q["motion"] / q["raw"] <= ms.QUALITY_RATIO_BOUND
    assert q["motion_denoised"] < q["raw_denoised"]
    assert q["motion_moved"] < q["raw_moved"]


@functools.lru_cache(maxsize=None)
def quality():
    """The figures of DESIGN.md 4.18 by the emulation (bit-identical to the GPU)."""
    frames = ms.quality_frames()
    state, snap, blind = None, None, None
    out = {k: [] for k in ("raw", "motion", "raw_denoised", "motion_denoised", "raw_moved", "motion_moved", "blind_moved")}
    for p, rad, rays, tt, sph, nrm, now, ref, moved in frames:
        state, col, var, _ = history_update_host(state, rad, p, None, (rays, (tt, sph)), motion=(now, snap))
        # a history that survives the uploads and is told nothing: plain updates on the same frames
        blind, bcol, _, _ = history_update_host(blind, rad, p, None, (rays, (tt, sph)))
        snap = now
        out["raw"].append(ds.mse(gamma_host(rad), ref))
        out["motion"].append(ds.mse(gamma_host(col), ref))
        out["raw_denoised"].append(ds.mse(denoise_host(rad, ((tt, sph), nrm), gamma=True), ref))
        out["motion_denoised"].append(ds.mse(denoise_host(col, ((tt, sph), nrm), variance=var, gamma=True), ref))
        if moved.any():
            out["raw_moved"].append(ds.mse(gamma_host(rad)[moved], ref[moved]))
            out["motion_moved"].append(ds.mse(gamma_host(col)[moved], ref[moved]))
            out["blind_moved"].append(ds.mse(gamma_host(bcol)[moved], ref[moved]))
    return {k: float(np.mean(v)) for k, v in out.items()}
