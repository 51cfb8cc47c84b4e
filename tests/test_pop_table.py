"""The pop table of the depth <= 8 LDS image (render_core.h lds_layout / pop_table_word) and the
camera walk that reads it (fast_pop under Masks64::kPopTable), on the host: no GPU needed.

The table's entries against the closed forms the pop computed per lane and step before the table
existed; the rest of the image byte for byte against the layout without the table; and the host
walk (the kernels' own fast_pop, reading the table from the host image) against the oracle on the
cases of tests/pop_table_cases.py, with the coverage those cases are there for asserted: every
mask bit the table holds popped, under every direction-sign mask."""
import ctypes as C

import numpy as np
import pytest

import pop_table_cases as cases
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import emulate_render_host

M32 = 0xFFFFFFFF


def lds_image(depth, fwd):
    """(image words, layout) of ort_debug_lds_image for forward tables fwd[3][2^depth + 1]."""
    lib = L.analysis_lib()
    lib.ort_debug_lds_image.restype = C.c_int
    lib.ort_debug_lds_image.argtypes = [C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int64,
                                        C.POINTER(C.c_int32)]
    lay = (C.c_int32 * 7)()
    fwd = np.ascontiguousarray(fwd, np.float32)
    L.acheck(lib.ort_debug_lds_image(depth, L.fptr(fwd), None, 0, lay))
    img = np.zeros(lay[0] // 4, np.uint32)
    L.acheck(lib.ort_debug_lds_image(depth, L.fptr(fwd), img.ctypes.data_as(C.POINTER(C.c_uint32)), img.size, lay))
    return img, dict(zip(("size", "lut", "plane_bytes", "pop", "pop2", "entries", "mode"), [int(v) for v in lay]))


def pop_coverage(reset):
    lib = L.analysis_lib()
    lib.ort_debug_pop_coverage.restype = C.c_int
    lib.ort_debug_pop_coverage.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int32]
    hb, m = np.zeros(64, np.uint64), np.zeros(8, np.uint64)
    L.acheck(lib.ort_debug_pop_coverage(hb.ctypes.data_as(C.POINTER(C.c_uint64)), m.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        1 if reset else 0))
    return hb, m


def forward_tables(depth):
    """Three strictly increasing plane tables with distinct, recognisable values."""
    n = (1 << depth) + 1
    return np.stack([np.linspace(-3.0 - a, 5.0 + 2 * a, n, dtype=np.float32) for a in range(3)])


def closed_form(depth, hb):
    """fast_pop's level arithmetic as it stood before the table: (m8, offA, offB, offC), (w4, h4, bit lo, bit hi)."""
    lvl, rk = hb >> 3, ~hb & 7
    w4 = 4 << (depth - 1 - lvl)
    s = depth + 1 - lvl  # log2(w4)
    first = (~(2 * w4 - 1) & M32, ((rk >> 1) & 1) << s, (rk & 1) << s, ((rk >> 2) & 1) << s)
    return first, (w4, w4 >> 1, (1 << hb) & M32, (1 << hb) >> 32)


def image_without_table(depth, fwd):
    """The image as the layout stood without the pop table: per axis the forward table and, 256
    floats further, the reversed one, in blocks of 768 floats (the last block ends with its
    reversed table), zeros between; then, from the next multiple of 16 bytes, the rank LUT."""
    p1 = (1 << depth) + 1
    n = 7 * 256 + p1
    pb = (4 * n + 15) & ~15
    img = np.zeros((pb + 2048) // 4, np.uint32)
    f = fwd.view(np.uint32)
    for a in range(3):
        img[768 * a:768 * a + p1] = f[a]
        img[768 * a + 256:768 * a + 256 + p1] = f[a][::-1]
    lib = L.analysis_lib()
    lut = np.zeros(2048, np.uint8)
    order = (C.c_int32 * 8)()
    for m in range(8):
        row = (C.c_uint8 * 256)()
        L.acheck(lib.ort_debug_fast_order(m, order, row))
        lut[256 * m:256 * m + 256] = np.frombuffer(row, np.uint8)
    img[pb // 4:] = lut.view(np.uint32)
    return img, pb


@pytest.mark.parametrize("depth", range(1, 9))
def test_entries_are_the_pops_closed_forms(depth):
    img, lay = lds_image(depth, forward_tables(depth))
    assert lay["entries"] == 56 and lay["pop"] % 16 == 0 and lay["pop2"] % 16 == 0
    assert lay["pop"] >= 4 * (256 + (1 << depth) + 1), "the table overlaps axis 0's reversed table"
    assert lay["pop"] + 16 * lay["entries"] <= 4 * 768 and lay["pop2"] == lay["pop"] + 4 * 768
    t1 = img[lay["pop"] // 4:lay["pop"] // 4 + 4 * 56].reshape(56, 4)
    t2 = img[lay["pop2"] // 4:lay["pop2"] // 4 + 4 * 56].reshape(56, 4)
    for hb in range(56):
        if hb < 8 * (depth - 1):
            first, second = closed_form(depth, hb)
            assert tuple(int(v) for v in t1[hb]) == first, (depth, hb)
            assert tuple(int(v) for v in t2[hb]) == second, (depth, hb)
        else:  # a level the camera walk never pops: its children are level-depth leaves
            assert not t1[hb].any() and not t2[hb].any(), (depth, hb)


@pytest.mark.parametrize("depth", range(1, 9))
def test_image_outside_the_table_is_unchanged(depth):
    fwd = forward_tables(depth)
    img, lay = lds_image(depth, fwd)
    old, pb = image_without_table(depth, fwd)
    assert lay["size"] == 4 * old.size == pb + 2048 and lay["lut"] == pb
    assert lay["plane_bytes"] == 4 * (7 * 256 + (1 << depth) + 1)
    table = np.zeros(img.size, bool)
    for off in (lay["pop"], lay["pop2"]):
        table[off // 4:off // 4 + 4 * lay["entries"]] = True
    assert not old[table].any(), "the table's bytes were zeros of a gap"
    assert np.array_equal(img[~table], old[~table])


@pytest.mark.parametrize("depth", (9, 10))
def test_deep_image_has_no_table(depth):
    fwd = forward_tables(depth)
    img, lay = lds_image(depth, fwd)
    p1 = (1 << depth) + 1
    pb = (4 * 3 * p1 + 15) & ~15
    assert (lay["pop"], lay["pop2"], lay["entries"]) == (-1, -1, 0)
    assert lay["size"] == pb + 2048 and lay["lut"] == pb
    assert np.array_equal(img[:3 * p1], fwd.view(np.uint32).reshape(-1))


@pytest.fixture(scope="module")
def host_walks():
    """Every case walked on the host once: {(depth, m, size, diag): frame}, and per depth the pop
    counts (hb[64], sign mask[8]) of the depth <= 8 camera walk over its cases."""
    frames, cover = {}, {}
    for depth in cases.DEPTHS:
        pop_coverage(True)
        for m in (0, 1):
            s, t = cases.scene(depth, m)
            for size in cases.SIZES:
                for diag in cases.DIAGONALS:
                    p = cases.pose(_ort(), size, diag)
                    frames[depth, m, size, diag] = emulate_render_host(s, t, p)[0]
        cover[depth] = pop_coverage(True)
    return frames, cover


def _ort():
    import octreeraytracer_amd
    return octreeraytracer_amd


@pytest.mark.parametrize("depth", cases.DEPTHS)
def test_host_walk_is_the_oracles(host_walks, depth):
    frames, _ = host_walks
    assert cases.N_SPHERES[depth] <= 2000
    for m in (0, 1):
        for size in cases.SIZES:
            for diag in cases.DIAGONALS:
                ref = cases.reference(depth, m, size, diag)
                got = frames[depth, m, size, diag]
                assert cases.same_bits(got, ref), (depth, m, size, diag, int((got != ref).any(axis=2).sum()))


@pytest.mark.parametrize("depth", cases.DEPTHS)
def test_cases_pop_every_entry_under_every_sign_mask(host_walks, depth):
    _, cover = host_walks
    hb, m = cover[depth]
    n = max(8 * (depth - 1), 0)
    print(f"depth {depth}: pops per hb {[int(v) for v in hb[:n]]}, per sign mask {[int(v) for v in m]}")
    assert not hb[n:].any(), "the camera walk popped a level-depth leaf: the table has no entry for it"
    if depth == 1:  # the root's children are leaves, tested inline: nothing is ever popped
        assert not hb.any() and not m.any()
        return
    if depth in (3, 5, 8):
        assert hb[:n].all(), [i for i in range(n) if not hb[i]]
        assert m.all(), [i for i in range(8) if not m[i]]
