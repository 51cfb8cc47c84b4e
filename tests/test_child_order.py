"""The depth <= 8 camera walk's child test from twelve order bits and two 64-byte tables
(render_core.h child_order_keep, Masks64::kOrderBits) against the eight min3/max3 tests it
replaces (child_drops), on the host: no GPU needed.

(a) a native sweep over every ordering of the nine slab values from a five-value grid, ties
    included, crossed with t_min and closest below, inside and above the grid: wherever the node's
    exit X is >= its entry E the two forms keep the same children;
(b) the same on random finite floats: denormals, +-0, values one ulp apart, closest = ORT_MAXFLOAT;
(c) where X < E under the folds -- which only a root can show -- child_drops keeps no child, and the
    host walk of such rays (an eye beyond the field, looking away) keeps none either;
(d) the two order tables against the kill sets of the twelve conditions, restated here;
(e) host-emulation frames against the oracle, bit for bit, with no visit breaking tN <= tM <= tF
    and none below the root with X < E."""
import ctypes as C

import numpy as np
import pytest

import pop_table_cases as cases
from oracle import oracle
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import emulate_render_host

ORT_MAXFLOAT = np.float32(3.402823466e38)
TABLE = 64
# condition -> (axes on which the killed children are the near half, ... the far half); A = 2, B = 1,
# C = 4 are the rank's bits; the issue's table, conditions 1..12
A, B, Cc = 2, 1, 4
KILLS = [(A, 0), (B, 0), (Cc, 0), (0, A), (0, B), (0, Cc),
         (A, B), (B, A), (A, Cc), (Cc, A), (B, Cc), (Cc, B)]


def child_order(mode, arr, n, tmins=None, closests=None, n_out=4):
    lib = L.analysis_lib()
    lib.ort_debug_child_order.restype = C.c_int
    lib.ort_debug_child_order.argtypes = [C.c_int32, L._fp, C.c_int64, L._fp, C.c_int32, L._fp, C.c_int32,
                                          C.POINTER(C.c_uint64)]
    out = np.zeros(n_out, np.uint64)
    f = lambda a: (L.fptr(a), len(a)) if a is not None else (None, 0)
    (tp, tn), (cp, cn) = f(tmins), f(closests)
    L.acheck(lib.ort_debug_child_order(mode, L.fptr(arr) if arr is not None else None, n, tp, tn, cp, cn,
                                       out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def visits(reset):
    return [int(v) for v in child_order(2, None, 1 if reset else 0, n_out=6)]


def test_order_bits_are_on():
    assert visits(False)[5] == 1, "Masks64::kOrderBits is off in this build"


def test_grid_sweep_forms_agree():
    grid = np.array([0.25, 0.5, 1.0, 2.0, 4.0], np.float32)
    # t_min and closest below the grid, on and between its values, above it, and the walk's own
    tmins = np.array([0.001, 0.125, 0.5, 0.75, 2.0, 8.0], np.float32)
    closests = np.array([0.125, 0.5, 1.5, 2.0, 4.0, 8.0, ORT_MAXFLOAT], np.float32)
    out = child_order(1, grid, len(grid), tmins, closests)
    total = 35 ** 3 * len(tmins) * len(closests)
    print(f"cases {total}: X >= E {int(out[0])} (disagree {int(out[1])}), X < E {int(out[2])} "
          f"(child_drops keeps a child in {int(out[3])})")
    assert int(out[0]) + int(out[2]) == total and int(out[0]) > 500_000 and int(out[2]) > 100_000
    assert int(out[1]) == 0
    assert int(out[3]) == 0  # (c): the premise fails => no child survives the old test either


def _folded(rng, pool, n):
    """n cases {tNA, tNB, tMA, tMB, tFA, tFB, nN, nF, cN, cF} with each axis sorted, values drawn
    from pool, and folds drawn from it too (or closest = ORT_MAXFLOAT in a third of them).  t_min is
    drawn from the positive values, denormals included: the walk's is 0.001, and with E >= t_min > 0
    a difference of two zeros of unlike sign, (-0) - (+0) = -0, can only kill what E already kills."""
    ax = np.sort(rng.choice(pool, (n, 3, 3)), axis=2)  # [case, axis, N/M/F]
    tmin = rng.choice(pool[pool > 0], n)
    closest = np.where(rng.random(n) < 1 / 3, ORT_MAXFLOAT, rng.choice(pool, n)).astype(np.float32)
    c = ax[:, 2]
    v = np.stack([ax[:, 0, 0], ax[:, 1, 0], ax[:, 0, 1], ax[:, 1, 1], ax[:, 0, 2], ax[:, 1, 2],
                  np.maximum(c[:, 0], tmin), np.maximum(c[:, 1], tmin),
                  np.minimum(c[:, 1], closest), np.minimum(c[:, 2], closest)], axis=1)
    return np.ascontiguousarray(v, np.float32)


def test_boundary_values_forms_agree():
    rng = np.random.default_rng(7)
    u = lambda bits: np.array(bits, np.uint32).view(np.float32)
    base = rng.standard_normal(6).astype(np.float32) * np.float32(3.0)
    near = np.concatenate([(base.view(np.uint32) + np.uint32(k)).view(np.float32) for k in (0, 1, 2)])  # one ulp apart
    pool = np.concatenate([near, u([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff,
                                    0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff, 0x3a83126f]),
                           (rng.standard_normal(8) * 1e-41).astype(np.float32),  # denormals
                           np.float32(10.0) ** rng.integers(-30, 30, 8).astype(np.float32)]).astype(np.float32)
    assert np.isfinite(pool).all()
    n = 400_000
    v = _folded(rng, pool, n)
    out = child_order(0, v.reshape(-1), n, n_out=2 * n).reshape(n, 2)
    E = np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 6])
    X = np.minimum(np.minimum(v[:, 4], v[:, 5]), v[:, 9])
    ok = X >= E
    print(f"X >= E in {int(ok.sum())} of {n}; ties X == E {int((X == E).sum())}")
    assert ok.sum() > n // 20 and (~ok).sum() > n // 20 and (X == E).sum() > 100
    bad = ok & (out[:, 0] != out[:, 1])
    assert not bad.any(), (v[bad][:3], out[bad][:3])
    assert not out[~ok, 0].any()  # (c)


def test_ties_keep_the_child():
    """Every value equal: all twelve differences are +0, every child is kept by both forms."""
    v = np.full(10, 1.5, np.float32)
    assert [int(x) for x in child_order(0, v, 1, n_out=2)] == [0xff, 0xff]


def table_entry(table, index):
    keep = 0xff
    for j in range(6):
        if (index >> (5 - j)) & 1:  # condition 6 table + j + 1 is false
            near, far = KILLS[6 * table + j]
            for rank in range(8):
                if (rank & far) == far and (rank & near) == 0:
                    keep &= ~(0x80 >> rank)
    return keep


def order_tables(device=False):
    """The 128 table bytes (table 0, then table 1): the host's, or those in device memory."""
    return [int(x) for x in child_order(4 if device else 3, None, 0, n_out=128)]


def test_tables_are_the_kill_sets():
    assert order_tables() == [table_entry(t, i) for t in (0, 1) for i in range(TABLE)]


def test_kill_sets_by_hand():
    """A few entries worked out from the condition table alone (rank 0 at bit 7)."""
    assert table_entry(0, 0) == 0xff and table_entry(1, 0) == 0xff
    assert table_entry(0, 0b100000) == 0b00110011  # 1 false: no A-near child (ranks 0, 1, 4, 5 go)
    assert table_entry(0, 0b000001) == 0b11110000  # 6 false: no C-far child (ranks 4-7 go)
    assert table_entry(1, 0b100000) == 0b10111011  # 7 false: A near and B far (ranks 1, 5) go
    assert table_entry(1, 0b000001) == 0b10101111  # 12 false: B far and C near (ranks 1, 3) go


DEPTHS = (1, 2, 3, 8)
SIZES = ((16, 16), (40, 24))


@pytest.fixture(scope="module")
def host_frames():
    frames = {}
    visits(True)
    for depth in DEPTHS:
        for m in (0, 1):
            s, t = cases.scene(depth, m)
            for size in SIZES:
                for diag in cases.DIAGONALS:
                    frames[depth, m, size, diag] = emulate_render_host(s, t, cases.pose(_ort(), size, diag))[0]
    return frames, visits(True)


def _ort():
    import octreeraytracer_amd
    return octreeraytracer_amd


@pytest.mark.parametrize("depth", DEPTHS)
def test_host_frames_are_the_oracles(host_frames, depth):
    frames, _ = host_frames
    for m in (0, 1):
        for size in SIZES:
            for diag in cases.DIAGONALS:
                ref = cases.reference(depth, m, size, diag)
                got = frames[depth, m, size, diag]
                assert cases.same_bits(got, ref), (depth, m, size, diag, int((got != ref).any(axis=2).sum()))


def test_host_walks_keep_the_premises(host_frames):
    _, v = host_frames
    print(f"internal-node visits {v[0]}: order broken {v[1]}, X < E below the root {v[2]}, forms differ {v[3]}")
    assert v[0] > 10_000
    assert v[1] == 0 and v[2] == 0 and v[3] == 0


def test_root_behind_the_ray_keeps_no_child():
    """An eye past the field looking away: the root box lies behind t_min for some rays, whose root
    test (no folds) still passes where the line of the ray meets the box.  Such roots are counted;
    child_drops keeps none of their children (the sweeps above), the walk keeps none either (the
    premise is a condition of the root's visit: fast_begin), and the frames are the oracle's."""
    ort = _ort()
    s, t = cases.scene(3, 0)
    visits(True)
    for pos, yaw in (((60.0, 1.0, 0.0), 0.0), ((-60.0, 1.0, 0.0), 180.0), ((0.0, 1.0, 60.0), 90.0)):
        p = ort.FrameParams.default_camera(16, 16, num_samples=1, max_depth=1, position=pos, yaw=yaw, pitch=0.0)
        got = emulate_render_host(s, t, p)[0]
        assert cases.same_bits(got, oracle.render(s, t, p))
    v = visits(True)
    print(f"visits {v[0]}, roots with X < E {v[4]}")
    # each pose looks straight away from the field, so at least the rays through the frame's centre have
    # the box on their line, behind them: one such root per pose is the least that can be
    assert v[4] >= 3 and v[2] == 0 and v[3] == 0
