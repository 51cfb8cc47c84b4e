"""The host's compact layout (octreeraytracer_amd/csrc/layout.cpp buildCompactLayout, and the leaf16
records and LDS images the host emulation derives from it) against rules stated in numpy from the
tree itself (tests/layout_cases.py): node[] with its leaf-children mask and leafkids flag, the
safety rule of the rejected-sphere skip entries kid[], planes[] reading back every node's box bit
for bit, leaf_sph[] / leaf_idx[] with the per-sphere tail, leaf16 on every node, and nk.  The
scenes are the ones tests/test_gpu_layout.py compares the device builder's layout on, so what
holds here for the host's arrays holds there for the device's; the forms of record the set must
reach are asserted here, on the CPU."""
import numpy as np
import pytest

import layout_cases as cases


@pytest.mark.parametrize("name", cases.SCENE_NAMES)
def test_host_layout_follows_the_rules(name):
    s, t, h = cases.host_case(name)
    bad = cases.host_violations(s, t, h)
    assert not bad, [(rule, list(np.asarray(ids)[:5])) for rule, ids in bad]
    assert h["nk"].shape == (t.n_nodes, 4)
    assert np.array_equal(h["nk"][:, :2], h["node"]) and np.array_equal(h["nk"][:, 2:], h["kid"])


def test_scene_set_reaches_every_form():
    assert cases.coverage_missing() == []
    assert not cases.host_case(cases.INVERTED)[2]["ordered"]
    others = [n for n in cases.scenes() if n != cases.INVERTED]
    assert all(cases.host_case(n)[2]["ordered"] for n in others)
    h = cases.host_case("three_d0_m0")[2]
    assert h["depth"] == 0 and h["planes"].size == 6 and h["node"].shape == (1, 2)


def test_signed_zero_scene_keeps_the_lower_index(ort):
    """The root's min.x is -0 (sphere 1) and +0 (sphere 2): the sequential fold keeps the first, and
    planes[] carries the sign bit."""
    s, t, h = cases.host_case("signed_zero_d2_m0")
    assert t.node_min[0, 0].view(np.uint32) == 0x80000000
    assert h["planes"][0] == 0x80000000


@pytest.mark.parametrize("side", ["min", "max"])
def test_host_root_keeps_the_zero_of_the_lower_index(ort, side):
    """The scenes tests/test_gpu_build.py holds the device builder's root fold to: the host tree's
    root bound on x is the zero of the lower-indexed of the two spheres, and no other sphere reaches 0."""
    from test_gpu_build import NEG0, POS0, ZERO_CASES, zero_bounds
    for n, at, d, m in ZERO_CASES:
        s = zero_bounds(ort, n, at, side)
        cr = s.center_radius
        bound = cr[:, 0] - cr[:, 3] if side == "min" else cr[:, 0] + cr[:, 3]
        rest = np.delete(bound, at)
        assert (rest >= 1).all() if side == "min" else (rest <= -1).all()
        assert list(bound[list(at)].view(np.uint32)) == [NEG0, POS0]
        t = ort.build_octree(s, d, m)
        root = (t.node_min if side == "min" else t.node_max)[0, 0].view(np.uint32)
        assert root == (NEG0 if at[0] < at[1] else POS0), (n, at)


def handmade(ort):
    """A depth-2 tree whose last internal node's children run past n_nodes: node 8 (octant 7 of the
    root) has children 9, 10, 11 of its eight.  Built trees never have this."""
    s = cases._plain(ort, [(2.5, 2.5, 2.5), (2.5, 3.5, 2.5), (1.0, 1.0, 1.0)], [0.25, 0.25, 0.5])
    n = 12
    mn, mx = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    mx[0] = 4
    for k in range(8):
        hi = np.array([(k >> 1) & 1, k & 1, (k >> 2) & 1], np.float32)
        mn[1 + k], mx[1 + k] = 2 * hi, 2 * hi + 2
    for k in range(3):
        hi = np.array([(k >> 1) & 1, k & 1, (k >> 2) & 1], np.float32)
        mn[9 + k], mx[9 + k] = 2 + hi, 3 + hi
    co = np.full(n, -1, np.int32)
    co[0], co[8] = 1, 9
    oo = np.full(n, -1, np.int32)
    cnt = np.zeros(n, np.int32)
    oo[1], cnt[1] = 0, 1    # sphere 2
    oo[9], cnt[9] = 1, 1    # sphere 0
    oo[10], cnt[10] = 2, 2  # spheres 0 and 1
    idx = np.array([2, 0, 0, 1], np.int32)
    return s, ort.FlatOctree(mn, mx, co, oo, cnt, idx)


def test_children_past_the_last_node(ort):
    s, t = handmade(ort)
    h = cases.host_layout(s, t)
    assert cases.host_violations(s, t, h) == []
    sh = cases.Shape(t)
    assert sh.depth == 2 and list(sh.kids[8]) == [9, 10, 11, -1, -1, -1, -1, -1]
    # node 8: children 0 and 1 hold spheres, child 2 is an empty leaf, 3-7 do not exist
    assert list(h["node"][8]) == [9, cases.INTERNAL | cases.LEAFKIDS | 0x0300 | 0x03]
    assert list(h["kid"][8]) == [0 | 1 << 24, 0]
    # x: node 8's children set slots 2, 3, 4, the root's 0, 2, 4: slot 1 is nobody's
    _, is_set = cases.planes_violations(t, sh, h["planes"])
    assert not is_set.all() and not is_set[0, 1] and h["planes"][1] == cases.QNAN
    assert list(h["planes"][:5].view(np.float32)[[0, 2, 3, 4]]) == [0.0, 2.0, 3.0, 4.0]


def test_the_rules_bite(ort):
    """A wrong word in any one array is a violation (the rules are no tautology)."""
    s, t, h = cases.host_case("pop_d3_m1")
    sh = cases.Shape(t)
    two = int(np.flatnonzero(h["kid"][:, 1] != 0)[0])
    for word, xor in ((0, 1), (0, 1 << 24), (0, 0xFF << 24), (1, 1), (1, 0xFFFFFFFF)):
        kid = h["kid"].copy()
        kid[two, word] ^= np.uint32(xor)
        assert cases.kid_violations(t, sh, kid), (word, xor)
    leaf =int(np.flatnonzero(t.children_offset == -1)[0])
    kid = h["kid"].copy()
    kid[leaf, 0] = 5 | 1 << 24
    assert cases.kid_violations(t, sh, kid)
    for name, at in (("node", (two, 1)), ("planes", 3), ("leaf_sph", (0, 3)), ("leaf_idx", t.n_indices), ("leaf16", (two, 3))):
        g = dict(h)
        g[name] = h[name].copy()
        g[name][at] ^= np.uint32(1 << 9)
        assert cases.host_violations(s, t, g), name


@pytest.mark.parametrize("name", ["twins_d9_m1", "twins_d10_m1", "pop_d5_m0"])
def test_lds_images(name):
    """The default image is ort_debug_lds_image's; the reversed-table image of a depth 9-10 tree holds
    each axis's planes forward from word 3T a and backward from word 3T a + T (T = 2^depth)."""
    from test_pop_table import lds_image
    _, _, h = cases.host_case(name)
    D = h["depth"]
    fwd = h["planes"].reshape(3, -1)
    img = cases.lds_image(D, h["planes"], False)
    assert np.array_equal(img, lds_image(D, fwd.view(np.float32))[0])
    if D <= 8:
        assert np.array_equal(cases.lds_image(D, h["planes"], True), img)  # already the reversed tables
        return
    rev = cases.lds_image(D, h["planes"], True)
    T, P1 = 1 << D, (1 << D) + 1
    assert rev.size != img.size
    for a in range(3):
        assert np.array_equal(rev[3 * T * a:3 * T * a + P1], fwd[a])
        assert np.array_equal(rev[3 * T * a + T:3 * T * a + T + P1], fwd[a][::-1])
        assert np.array_equal(img[P1 * a:P1 * (a + 1)], fwd[a])
