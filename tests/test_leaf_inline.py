"""The 16-byte leaf records of the depth <= 8 camera walk (render_core.h leaf16_record /
leaf16_tests under Masks64::kLeafInline), on the host: no GPU needed.

The derived array word for word against node[] and leaf_sph[]; the host walk (the kernels' own
leaf_kids, reading the records the same function derived) bit for bit against the oracle on the
scenes of tests/pop_table_cases.py, with both record forms shown to be reached (tested, rejected
and accepted); the entry recovered for a hit in an inline-form leaf against the exact walk's; and
radii at the edges of the inline form: r^2 huge, +inf, 0 and NaN."""
import ctypes as C

import numpy as np
import pytest

import pop_table_cases as cases
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import emulate_render_host
from leaf_inline_cases import TAG, _tree_args, expected_records, layout_arrays
from test_emulation import extreme_root_scene

MIXED = (2, 3, 5)   # depths whose trees hold both record forms (asserted below)
PURE = {8: "inline", 1: "list"}  # depth 8: one-sphere leaves only; depth 1: multi-sphere only


def leaf_forms(reset):
    """{inline tests, inline hits, list tests, list hits} of the host's camera walks since the last reset."""
    lib = L.analysis_lib()
    lib.ort_debug_leaf_forms.restype = C.c_int
    lib.ort_debug_leaf_forms.argtypes = [C.POINTER(C.c_uint64), C.c_int32]
    out = (C.c_uint64 * 4)()
    L.acheck(lib.ort_debug_leaf_forms(out, 1 if reset else 0))
    return [int(v) for v in out]


@pytest.mark.parametrize("m", (0, 1))
@pytest.mark.parametrize("depth", cases.DEPTHS)
def test_records_are_the_node_and_sphere_words(depth, m):
    s, t = cases.scene(depth, m)
    node, sph, l16 = layout_arrays(s, t)
    assert len(l16) == len(node) == t.n_nodes
    exp, internal, inline = expected_records(node, sph)
    leaf = ~internal
    assert np.array_equal(l16[leaf], exp[leaf])
    assert not (l16[inline, 3] & TAG).any() and (l16[leaf & ~inline, 3] & TAG).all()
    n_inline = int(inline.sum())
    n_list = int((leaf & ~inline & (node[:, 1] > 0)).sum())
    print(f"depth {depth} m {m}: {n_inline} inline leaves, {n_list} non-empty list leaves")
    if m == 0 and depth in MIXED:
        assert n_inline > 0 and n_list > 0
    if m == 0 and depth == 3:
        assert (n_inline, n_list) == (106, 261)
    if m == 0 and depth == 5:
        assert (n_inline, n_list) == (7600, 1712)
    if m == 0 and depth in PURE:
        assert (n_list == 0) if PURE[depth] == "inline" else (n_inline == 0)


def test_deep_trees_have_no_records(ort):
    s = ort.random_spheres(300, 42)
    _, _, l16 = layout_arrays(s, ort.build_octree(s, 9, 0))
    assert len(l16) == 0


@pytest.fixture(scope="module")
def host_walks(ort):
    """Every case walked on the host once: {(depth, m, size, diag): frame} and per (depth, m) the
    walk's tests and hits per record form."""
    frames, forms = {}, {}
    for depth in cases.DEPTHS:
        for m in (0, 1):
            s, t = cases.scene(depth, m)
            leaf_forms(True)
            for size in cases.SIZES:
                for diag in cases.DIAGONALS:
                    frames[depth, m, size, diag] = emulate_render_host(s, t, cases.pose(ort, size, diag))[0]
            forms[depth, m] = leaf_forms(True)
    return frames, forms


@pytest.mark.parametrize("depth", cases.DEPTHS)
def test_host_walk_is_the_oracles(host_walks, depth):
    frames, _ = host_walks
    for m in (0, 1):
        for size in cases.SIZES:
            for diag in cases.DIAGONALS:
                ref = cases.reference(depth, m, size, diag)
                got = frames[depth, m, size, diag]
                assert cases.same_bits(got, ref), (depth, m, size, diag, int((got != ref).any(axis=2).sum()))


@pytest.mark.parametrize("m", (0, 1))
@pytest.mark.parametrize("depth", cases.DEPTHS)
def test_walks_reach_both_forms(host_walks, depth, m):
    """Over a mixed scene's poses each form is tested, rejects a sphere and accepts one; the pure
    scenes never meet the other form."""
    _, forms = host_walks
    it, ih, lt, lh = forms[depth, m]
    print(f"depth {depth} m {m}: inline {it} tests / {ih} hits, list {lt} tests / {lh} hits")
    if depth in MIXED:
        assert ih >= 1 and it - ih >= 1, (it, ih)
        assert lh >= 1 and lt - lh >= 1, (lt, lh)
    elif m == 0 and PURE[depth] == "inline":
        assert ih >= 1 and it - ih >= 1 and lt == 0
    elif m == 0:
        assert lh >= 1 and lt - lh >= 1 and it == 0


def _trace_rays(s, t, rays):
    lib = L.analysis_lib()
    keep, args = _tree_args(s, t)
    rays = np.ascontiguousarray(rays, np.float32)
    out = np.zeros((len(rays), 5), np.int32)
    L.acheck(lib.ort_debug_trace_rays(*args, L.fptr(rays), len(rays), 0, L.iptr(out)))
    del keep
    return out


@pytest.mark.parametrize("depth", (3, 5, 8))
def test_inline_hits_report_the_leafs_entry(depth):
    """The camera walk's entry (an inline-form hit: recovered from the leaf's record after the
    walk) is the exact walk's, which reads node[] and leaf_sph[] as before."""
    s, t = cases.scene(depth, 0)
    rng = np.random.default_rng(7)
    d = rng.normal(size=(4000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    rays = np.concatenate([np.tile(np.asarray(cases.EYE, np.float32), (len(d), 1)), d], axis=1)
    out = _trace_rays(s, t, rays)
    fast = out[:, 0] == 1
    assert fast.sum() > 3000
    assert np.array_equal(out[fast, 1], out[fast, 3]) and np.array_equal(out[fast, 2], out[fast, 4])
    # a one-sphere leaf's entry lies in the per-sphere tail, from n_indices on
    tail = fast & (out[:, 1] >= t.n_indices)
    assert tail.sum() >= 10, int(tail.sum())
    assert (out[fast, 1] < 0x40000000).all()


def _with_radius(ort, s, index, radius):
    cr = np.array(s.center_radius, np.float32)
    ma = np.asarray(s.mat_albedo, np.float32)
    fr = np.asarray(s.fuzz_ri, np.float32)
    cr[index, 3] = radius
    return ort.SphereSet.from_arrays(cr[:, :3], cr[:, 3], ma[:, 0].astype(np.int32), ma[:, 1:4], fr[:, 0], fr[:, 1])


def test_huge_radii(ort, oracle):
    """extreme_root_scene: r = 1e18 and 1e19, r^2 finite but huge."""
    s = extreme_root_scene(ort)
    t = ort.build_octree(s, 5, 0)
    p = ort.FrameParams.default_camera(64, 40, max_depth=4)
    assert cases.same_bits(emulate_render_host(s, t, p)[0], oracle.render(s, t, p))
    node, sph, l16 = layout_arrays(s, t)
    _, _, inline = expected_records(node, sph)
    assert (l16[inline, 3].view(np.float32) > 1e35).any()  # an inline record carries a huge r^2


def test_infinite_r2_is_inline(ort, oracle):
    """r = 2e19 > 1.85e19: r * r = +inf in fp32, an ordinary inline record."""
    s = _with_radius(ort, extreme_root_scene(ort), 2, 2e19)
    t = ort.build_octree(s, 5, 0)
    p = ort.FrameParams.default_camera(64, 40, max_depth=4)
    node, sph, l16 = layout_arrays(s, t)
    exp, internal, inline = expected_records(node, sph)
    assert np.array_equal(l16[~internal], exp[~internal])
    assert (l16[inline, 3] == 0x7F800000).any()
    assert cases.same_bits(emulate_render_host(s, t, p)[0], oracle.render(s, t, p))


def test_zero_radius_is_inline(ort, oracle):
    s0, _ = cases.scene(3, 0)
    s = _with_radius(ort, s0, 5, 0.0)
    t = ort.build_octree(s, 3, 0)
    node, sph, l16 = layout_arrays(s, t)
    exp, internal, inline = expected_records(node, sph)
    assert np.array_equal(l16[~internal], exp[~internal])
    zero = sph[:, 3] == 0
    assert zero.any()
    leaves = np.flatnonzero(inline)
    assert not len(leaves) or not (l16[leaves, 3] & TAG).any()
    for diag in cases.DIAGONALS[:2]:
        p = cases.pose(ort, (48, 32), diag)
        assert cases.same_bits(emulate_render_host(s, t, p)[0], oracle.render(s, t, p))


def test_nan_radius_keeps_the_list_form(ort, oracle):
    """The upload accepts a NaN radius; r^2 = NaN is no inline record (its bits could carry the
    tag), so the sphere's one-sphere leaves keep the list form, and the frame is the oracle's."""
    s0, t = cases.scene(3, 0)
    node, sph, _ = layout_arrays(s0, t)
    one = np.flatnonzero(((node[:, 1] & TAG) == 0) & (node[:, 1] == 1))
    sphere = int(node[one[0], 0]) - t.n_indices  # a sphere alone in a leaf: its entry lies in the per-sphere tail
    assert 0 <= sphere < s0.n
    s = _with_radius(ort, s0, sphere, float("nan"))
    node, sph, l16 = layout_arrays(s, t)
    exp, internal, inline = expected_records(node, sph)
    assert np.array_equal(l16[~internal], exp[~internal])
    nan_leaves = one[np.isnan(sph[node[one, 0], 3].view(np.float32))]
    assert len(nan_leaves) >= 1 and not inline[nan_leaves].any()
    assert (l16[nan_leaves] == np.array([[0, 1, 0, TAG | 1]], np.uint32))[:, 1:].all()
    assert np.array_equal(l16[nan_leaves, 0], node[nan_leaves, 0])
    for diag in cases.DIAGONALS[:2]:
        p = cases.pose(ort, (48, 32), diag)
        assert cases.same_bits(emulate_render_host(s, t, p)[0], oracle.render(s, t, p))


def test_root_leaf_and_brute_force(ort, oracle):
    s = ort.random_spheres(40, 42)
    t = ort.build_octree(s, 0, 0)  # depth 0: the root is a leaf, popped as a node
    p = cases.pose(ort, (48, 32), cases.DIAGONALS[0])
    leaf_forms(True)
    assert cases.same_bits(emulate_render_host(s, t, p)[0], oracle.render(s, t, p))
    assert leaf_forms(True) == [0, 0, 0, 0]
    pb = ort.FrameParams.default_camera(48, 32, use_octree=0)
    assert cases.same_bits(emulate_render_host(s, None, pb)[0], oracle.render(s, None, pb))
    assert leaf_forms(True) == [0, 0, 0, 0]
