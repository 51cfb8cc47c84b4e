"""Helpers shared by tests/test_layout.py (the host's compact layout against rules stated here in
numpy from the tree itself) and tests/test_gpu_layout.py (the device builder's layout against the
host's): the arrays of the compact layout through the analysis library's export hooks, the rules
node[], kid[], planes[], leaf_sph[] / leaf_idx[] and the derived arrays follow, and the scenes
that reach every form of record.

Run as a program (with ORT_LIB naming the analysis library, in a process of its own: the hooks are
not part of libort.so) it builds every scene on the GPU, reads the device's arrays, and compares
them byte for byte with the ones the host derives from the host-built tree; then uploads the host
tree into the same renderer and compares again.  One verdict line per scene; exit status 0 only if
all hold."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from octreeraytracer_amd import _lib as L  # noqa: E402

from leaf_inline_cases import _tree_args, expected_records  # noqa: E402

INTERNAL = 0x80000000
LEAFKIDS = 0x40000000
QNAN = 0x7FC00000
HOST_ARRAYS = ("node", "kid", "leaf_sph", "leaf_idx", "planes", "leaf16")
DEVICE_ARRAYS = HOST_ARRAYS + ("nk", "lds_img", "lds_rev")
SCALARS = ("depth", "ordered", "layout")
_SHAPE = {"node": 2, "kid": 2, "leaf_sph": 4, "leaf16": 4, "nk": 4}  # words per record; others flat
_U32P = C.POINTER(C.c_uint32)


def _shaped(name, words):
    return words.reshape(-1, _SHAPE[name]) if name in _SHAPE else words


# ---- the export hooks --------------------------------------------------------------------------
def host_layout(s, t):
    """What HostScene::build holds for a tree under the compact layout: the arrays of HOST_ARRAYS
    as uint32 words (leaf16 empty for a tree deeper than 8), nk as node and kid interleaved, and the
    scalars depth and ordered."""
    lib = L.analysis_lib()
    lib.ort_debug_layout.restype = C.c_int
    lib.ort_debug_layout.argtypes = [L._fp, C.c_int32, L._fp, L._fp, L._ip, L._ip, L._ip, C.c_int32, L._ip, C.c_int64,
                                     C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    keep, args = _tree_args(s, t)
    out = {}
    for name in HOST_ARRAYS + ("depth", "ordered"):
        n = C.c_int64()
        L.acheck(lib.ort_debug_layout(*args, name.encode(), None, 0, C.byref(n)))
        a = np.zeros(n.value // 4, np.uint32)
        if n.value:
            L.acheck(lib.ort_debug_layout(*args, name.encode(), a.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        out[name] = _shaped(name, a) if name in HOST_ARRAYS else int(a[0])
    del keep
    out["nk"] = np.concatenate([out["node"], out["kid"]], axis=1)
    return out


def lds_image(depth, planes, rev):
    """The workgroup LDS image of a tree's plane tables as uint32 words: the default one (rev False:
    fast_rev_planes(depth)'s choice) or the reversed-table image of a depth 9-10 scene."""
    lib = L.analysis_lib()
    lib.ort_debug_lds_image_rev.restype = C.c_int
    lib.ort_debug_lds_image_rev.argtypes = [C.c_int32, L._fp, C.c_int32, _U32P, C.c_int64, C.POINTER(C.c_int32)]
    lay = (C.c_int32 * 7)()
    fwd = np.ascontiguousarray(planes).view(np.float32)
    L.acheck(lib.ort_debug_lds_image_rev(depth, L.fptr(fwd), int(rev), None, 0, lay))
    img = np.zeros(lay[0] // 4, np.uint32)
    L.acheck(lib.ort_debug_lds_image_rev(depth, L.fptr(fwd), int(rev), img.ctypes.data_as(_U32P), img.size, lay))
    return img


def device_layout(r):
    """Every array and scalar of a renderer's scene through the context hook (the library ORT_LIB
    names: the analysis library)."""
    lib = L.lib()
    lib.ort_debug_ctx_array.restype = C.c_int
    lib.ort_debug_ctx_array.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    out = {}
    for name in DEVICE_ARRAYS + SCALARS:
        n = C.c_int64()
        L.check(lib.ort_debug_ctx_array(r._ctx, name.encode(), None, 0, C.byref(n)), r._ctx)
        a = np.zeros(n.value // 4, np.uint32)
        if n.value:
            L.check(lib.ort_debug_ctx_array(r._ctx, name.encode(), a.ctypes.data_as(C.c_void_p), n.value, C.byref(n)),
                    r._ctx)
        out[name] = _shaped(name, a) if name in DEVICE_ARRAYS else int(a.view(np.int32)[0])
    return out


# ---- the tree, as the rules below read it ------------------------------------------------------
class Shape:
    """Per node of a FlatOctree: kids[n, 8] (child ids, -1 where the node is a leaf or the id runs
    past n_nodes), level[n], cell[n, 3] (x, y, z; octant bit 1 = x, bit 0 = y, bit 2 = z), and the
    tree's depth.  Children found level by level from the root."""

    def __init__(self, t):
        n = t.n_nodes
        co = np.asarray(t.children_offset, np.int64)
        ids = co[:, None] + np.arange(8)[None, :]
        self.kids = np.where((co[:, None] != -1) & (ids < n), ids, -1)
        self.level = np.full(n, -1, np.int64)
        self.cell = np.zeros((n, 3), np.int64)
        front = np.array([0])
        self.level[0] = 0
        bit = np.stack([(np.arange(8) >> 1) & 1, np.arange(8) & 1, (np.arange(8) >> 2) & 1], axis=1)  # [octant, axis]
        d = 0
        while True:
            k = self.kids[front]
            have = k >= 0
            if not have.any():
                break
            child = k[have]
            parent = np.broadcast_to(front[:, None], k.shape)[have]
            octant = np.broadcast_to(np.arange(8)[None, :], k.shape)[have]
            assert (self.level[child] == -1).all(), "node reachable twice"
            d += 1
            self.level[child] = d
            self.cell[child] = 2 * self.cell[parent] + bit[octant]
            front = child
        self.depth = d
        self.reached = self.level >= 0


def one_sphere_kids(t, sh):
    """sid[n, 8]: the sphere of child k where it is a leaf holding exactly one sphere, else -1."""
    co, cnt, oo = (np.asarray(a, np.int64) for a in (t.children_offset, t.object_count, t.objects_offset))
    k = np.maximum(sh.kids, 0)
    one = (sh.kids >= 0) & (co[k] == -1) & (cnt[k] == 1)
    idx = np.asarray(t.object_indices, np.int64)
    return np.where(one, idx[np.where(one, oo[k], 0)] if len(idx) else -1, -1)


# ---- the rules -----------------------------------------------------------------------------------
def expected_node(t, sh):
    """node[n, 2] from the tree."""
    n = t.n_nodes
    co, cnt, oo = (np.asarray(a, np.int64) for a in (t.children_offset, t.object_count, t.objects_offset))
    idx = np.asarray(t.object_indices, np.int64)
    internal = co != -1
    k = np.maximum(sh.kids, 0)
    have = sh.kids >= 0
    kid_internal = have & (co[k] != -1)
    kid_leaf = have & (co[k] == -1)
    nonempty = have & ~(kid_leaf & (oo[k] == -1))
    w = (1 << np.arange(8))[None, :]
    y_int = (INTERNAL | (nonempty * w).sum(1) | ((nonempty & kid_leaf) * w).sum(1) << 8
             | np.where(kid_internal.any(1), 0, LEAFKIDS))
    c = np.maximum(cnt, 0)
    first = idx[np.where(c > 0, oo, 0)] if len(idx) else np.zeros(n, np.int64)
    x_leaf = np.where(c == 0, 0, np.where(c == 1, t.n_indices + first, oo))
    return np.stack([np.where(internal, co, x_leaf), np.where(internal, y_int, c)], axis=1).astype(np.uint32)


def kid_violations(t, sh, kid):
    """The safety rule of kid[] (kid_table.h), as a list of (rule, node ids that break it)."""
    co = np.asarray(t.children_offset, np.int64)
    internal = co != -1
    sid = one_sphere_kids(t, sh)
    word = kid.astype(np.int64)                      # [n, 2]
    ident, mask = word & 0xFFFFFF, word >> 24
    used = word != 0
    bits = ((mask[:, :, None] >> np.arange(8)) & 1) == 1          # [n, entry, octant]
    holds = sid[:, None, :] == ident[:, :, None]                    # child is a one-sphere leaf of the entry's id
    same = (sid[:, :, None] == sid[:, None, :]) & (sid[:, :, None] >= 0)
    count = same.sum(2)                                             # [n, octant]: children holding this child's sphere
    count0 = np.where(used[:, 0], holds[:, 0].sum(1), 0)
    named = ((sid[:, :, None] == ident[:, None, :]) & used[:, None, :]).any(2)
    bad = {
        "a mask bit on a child that is no one-sphere leaf of the entry's sphere": (bits & ~holds).any((1, 2)),
        "a used entry without a mask bit": (used & (mask == 0)).any(1),
        "an entry missing one of its sphere's children": (used[:, :, None] & holds & ~bits).any((1, 2)),
        "both entries name one sphere": used[:, 0] & used[:, 1] & (ident[:, 0] == ident[:, 1]),
        "a sphere in more children than entry 0's is missing": ((sid >= 0) & (count > count0[:, None]) & ~named).any(1),
        "a leaf with an entry": ~internal & used.any(1),
        "one-sphere children but no entry": internal & (sid >= 0).any(1) & ~used.any(1),
        "an entry beyond the node's own": ~used[:, 0] & used[:, 1],
    }
    return [(rule, np.flatnonzero(v & sh.reached)) for rule, v in bad.items() if (v & sh.reached).any()]


def planes_violations(t, sh, planes):
    """Every reached node's box must read back bit for bit; a slot nobody sets is the quiet NaN.
    Returns (violations, which slots [axis, slot] a node sets)."""
    D = sh.depth
    P1 = (1 << D) + 1
    out = []
    if planes.size != 3 * P1:
        return [("planes has %d entries, not 3 (2^%d + 1)" % (planes.size, D), np.array([0]))], None
    pl = planes.reshape(3, P1)
    ids = np.flatnonzero(sh.reached)
    s = D - sh.level[ids]
    is_set = np.zeros((3, P1), bool)
    for a in range(3):
        lo, hi = sh.cell[ids, a] << s, (sh.cell[ids, a] + 1) << s
        is_set[a, lo] = True
        is_set[a, hi] = True
        mn = np.ascontiguousarray(t.node_min[ids, a]).view(np.uint32)
        mx = np.ascontiguousarray(t.node_max[ids, a]).view(np.uint32)
        wrong = (pl[a, lo] != mn) | (pl[a, hi] != mx)
        if wrong.any():
            out.append(("box does not read back on axis %d" % a, ids[wrong]))
    stray = ~is_set & (pl != QNAN)
    if stray.any():
        out.append(("an unset slot is not the NaN 0x7fc00000", np.flatnonzero(stray)))
    return out, is_set


def expected_leaf_entries(s, t):
    """(leaf_sph[e, 4] words, leaf_idx[e]): objectIndices, then every sphere in order; .w = r * r in fp32."""
    which = np.concatenate([np.asarray(t.object_indices, np.int64), np.arange(s.n)])
    cr = np.ascontiguousarray(s.center_radius, np.float32)[which]
    sph = cr.copy()
    sph[:, 3] = cr[:, 3] * cr[:, 3]  # float32 * float32: rounded once
    return sph.view(np.uint32), which.astype(np.uint32)


def expected_leaf16(node, leaf_sph):
    """leaf16 by leaf_inline_cases.expected_records' rule, which is defined on every node: a record
    that is no clean one-sphere leaf (internal nodes among them) is (x, y, 0, y | tag)."""
    return expected_records(node, leaf_sph)[0]


def host_violations(s, t, h):
    """Every rule above against a host layout h; [] when all hold."""
    sh = Shape(t)
    bad = []
    if h["depth"] != sh.depth:
        bad.append(("depth %d, the tree's is %d" % (h["depth"], sh.depth), []))
    exp = expected_node(t, sh)
    wrong = (h["node"] != exp).any(1) & sh.reached if h["node"].shape == exp.shape else np.ones(1, bool)
    if wrong.any():
        bad.append(("node record", np.flatnonzero(wrong)))
    bad += kid_violations(t, sh, h["kid"]) if h["kid"].shape == exp.shape else [("kid size", [])]
    bad += planes_violations(t, sh, h["planes"])[0]
    sph, idx = expected_leaf_entries(s, t)
    if not (h["leaf_sph"].shape == sph.shape and np.array_equal(h["leaf_sph"], sph)):
        bad.append(("leaf_sph", []))
    if not np.array_equal(h["leaf_idx"], idx):
        bad.append(("leaf_idx", []))
    ordered = bool((t.node_min[sh.reached] <= t.node_max[sh.reached]).all())
    if bool(h["ordered"]) != ordered:
        bad.append(("ordered %d, the boxes say %d" % (h["ordered"], ordered), []))
    if sh.depth <= 8:
        if not np.array_equal(h["leaf16"], expected_leaf16(h["node"], h["leaf_sph"])):
            bad.append(("leaf16", []))
    elif len(h["leaf16"]):
        bad.append(("leaf16 on a tree deeper than 8", []))
    return bad


# ---- the scenes ----------------------------------------------------------------------------------
def _plain(ort, centres, radii):
    n = len(radii)
    return ort.SphereSet.from_arrays(np.asarray(centres, np.float32), radii, [0] * n, np.full((n, 3), 0.5), [0.0] * n,
                                     [1.5] * n)


def signed_zero_trio(ort):
    """The root's min.x is a zero of both signs: -0 from sphere 1, +0 from sphere 2.  The reference's
    sequential fold keeps the first."""
    return _plain(ort, [(2.0, 2, 2), (-0.0, 3, 3), (0.5, 3, 3)], [1.0, 0.0, 0.5])


def inverted(ort):
    """Every radius negative and the centres closer together than twice |r|: min = c + |r| lies above
    max = c - |r| on every axis, so the root box, and every box under it, is inverted."""
    return _plain(ort, [(0.0, 1.0, 0.0), (0.5, 1.3, 0.2), (0.2, 1.6, 0.4), (0.4, 1.1, 0.7)], [-1.0] * 4)


def coincident(ort):
    """tests/test_gpu_build.py's six: shared centres, spheres tangent to split planes."""
    c = np.array([[0, 0, 0], [0, 0, 0], [1, 1, 1], [-1, -1, -1], [0.5, 0, 0], [0, 0.25, 0]], np.float32)
    return ort.SphereSet.from_arrays(c, [0.5, 0.5, 0.25, 0.25, 0.5, 0.25], [0, 1, 2, 0, 1, 2], np.full((6, 3), 0.5),
                                     [0, 0.1, 0, 0, 0.2, 0], [1, 1, 1.5, 1, 1, 1.5])


def twins(ort):
    """tests/test_gpu_explicit.py's barely overlapping pairs: random_spheres(100, 42) plus a copy of
    each of its last 8 spheres moved 1.999 radii along +x.  Under maxSpheresPerNode 1 the builder
    splits down to its depth limit between the two of a pair and nowhere else: a deep, small tree
    (1000 random spheres stop splitting above level 9)."""
    s = ort.random_spheres(100, 42)
    cr = s.center_radius[-8:].copy()
    cr[:, 0] += np.float32(1.999) * cr[:, 3]
    return ort.SphereSet(np.concatenate([s.center_radius, cr]), np.concatenate([s.mat_albedo, s.mat_albedo[-8:]]),
                         np.concatenate([s.fuzz_ri, s.fuzz_ri[-8:]]))


INVERTED = "inverted_d3_m0"
FRAME = (64, 40)
# scenes()'s names, for a test to parametrise over without building a scene at collection
SCENE_NAMES = tuple(["pop_d%d_m%d" % (d, m) for d in (1, 2, 3, 5, 8) for m in (0, 1)] + [
    "chart_d6_m0", "chart_d4_m1", "coincident_d3_m0", "coincident_d5_m1", "coincident_d8_m2", "rand2000_d6_m0",
    "rand2000_d7_m5", "rand1000_d10_m1", "twins_d9_m1", "twins_d10_m1", "one_d4_m0", "three_d0_m0", "signed_zero_d2_m0",
    INVERTED])


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (spheres, depth limit, maxSpheresPerNode), in the order they run."""
    import octreeraytracer_amd as ort
    import pop_table_cases
    from chart_scenes import chart
    out = {}
    for d in pop_table_cases.DEPTHS:
        for m in (0, 1):
            out["pop_d%d_m%d" % (d, m)] = (pop_table_cases.scene(d, m)[0], d, m)
    out["chart_d6_m0"] = (chart(ort), 6, 0)
    out["chart_d4_m1"] = (chart(ort), 4, 1)
    for d, m in ((3, 0), (5, 1), (8, 2)):
        out["coincident_d%d_m%d" % (d, m)] = (coincident(ort), d, m)
    out["rand2000_d6_m0"] = (ort.random_spheres(2000, 7), 6, 0)
    out["rand2000_d7_m5"] = (ort.random_spheres(2000, 7), 7, 5)
    out["rand1000_d10_m1"] = (ort.random_spheres(1000, 3), 10, 1)
    out["twins_d9_m1"] = (twins(ort), 9, 1)  # depth 9 and 10: the scenes with a reversed-table image
    out["twins_d10_m1"] = (twins(ort), 10, 1)
    out["one_d4_m0"] = (ort.random_spheres(1, 1), 4, 0)
    out["three_d0_m0"] = (ort.random_spheres(3, 2), 0, 0)
    out["signed_zero_d2_m0"] = (signed_zero_trio(ort), 2, 0)
    out[INVERTED] = (inverted(ort), 3, 0)
    assert tuple(out) == SCENE_NAMES
    return out


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(spheres, host-built tree, host layout) of a scene, built once and read-only."""
    import octreeraytracer_amd as ort
    s, d, m = scenes()[name]
    t = ort.build_octree(s, d, m)
    h = host_layout(s, t)
    for a in h.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s, t, h


def coverage(h):
    """Which of the forms the scene set must reach a host layout has."""
    node, kid = h["node"], h["kid"]
    internal = (node[:, 1] & INTERNAL) != 0
    masks = np.concatenate([kid[:, 0] >> 24, kid[:, 1] >> 24])
    two_bits = (masks & (masks - 1)) != 0
    return {
        "a second kid entry": bool((kid[:, 1] != 0).any()),
        "a kid mask of two or more bits": bool(two_bits.any()),
        "a kid entry naming sphere 0": bool(((kid != 0) & ((kid & 0xFFFFFF) == 0)).any()),
        "an empty leaf": bool((~internal & (node[:, 1] == 0)).any()),
        "a one-sphere leaf": bool((~internal & (node[:, 1] == 1)).any()),
        "a list leaf": bool((~internal & (node[:, 1] >= 2)).any()),
        "an internal node with leafkids": bool((internal & ((node[:, 1] & LEAFKIDS) != 0)).any()),
        "an internal node without leafkids": bool((internal & ((node[:, 1] & LEAFKIDS) == 0)).any()),
        "a tree of depth 9 or more": h["depth"] >= 9,
    }


def coverage_missing():
    """The forms no scene reaches (must be none)."""
    got = {}
    for name in scenes():
        for form, there in coverage(host_case(name)[2]).items():
            got[form] = got.get(form, False) or there
    return [form for form, there in got.items() if not there]


# ---- the device route against the host route (run as a program) ---------------------------------
def differences(dev, h):
    """Names of what a device layout (device_layout) does not share with a host layout, byte for byte."""
    depth = h["depth"]
    want = dict(h)
    want["layout"] = L.ORT_LAYOUT_COMPACT
    want["lds_img"] = lds_image(depth, h["planes"], False)
    want["lds_rev"] = lds_image(depth, h["planes"], True) if depth > 8 else np.zeros(0, np.uint32)
    bad = []
    for name in DEVICE_ARRAYS:
        if dev[name].shape != want[name].shape:
            bad.append("%s (%d words, the host's has %d)" % (name, dev[name].size, want[name].size))
        elif not np.array_equal(dev[name], want[name]):
            at = np.flatnonzero(dev[name].ravel() != want[name].ravel())
            bad.append("%s (%d of %d words, the first at %d: %#x, the host's %#x)" % (
                name, at.size, want[name].size, at[0], dev[name].ravel()[at[0]], want[name].ravel()[at[0]]))
    for name in SCALARS:
        if int(dev[name]) != int(want[name]):
            bad.append("%s %d / %d" % (name, dev[name], want[name]))
    return bad


def main():
    import octreeraytracer_amd as ort
    from oracle import oracle
    from pop_table_cases import same_bits
    failed = 0
    missing = coverage_missing()
    print("forms no scene reaches: %s" % (missing or "none"))
    failed += len(missing)
    with ort.Renderer(0) as r:
        for name, (s, d, m) in scenes().items():
            _, t, h = host_case(name)
            bad = []  # (the host's arrays against the rules: tests/test_layout.py)
            r.build_scene(s, d, m, keep_tree=True)
            built = r.export_octree()
            if not (np.array_equal(built.gpu_records(), t.gpu_records())
                    and np.array_equal(built.object_indices, t.object_indices)):
                bad.append("built: tree")
            bad += ["built: " + x for x in differences(device_layout(r), h)]
            if name == INVERTED:
                p = ort.FrameParams.default_camera(*FRAME)
                if h["ordered"] or device_layout(r)["ordered"]:
                    bad.append("ordered set on inverted boxes")
                if not same_bits(r.render(p), oracle.render(s, t, p)):
                    bad.append("built: frame differs from the oracle's")
            r.upload(s, t)
            bad += ["uploaded: " + x for x in differences(device_layout(r), h)]
            print("%-20s %8d nodes depth %2d: %s" % (name, t.n_nodes, h["depth"], "equal" if not bad else "; ".join(bad)))
            failed += len(bad)
    print("all equal: %s" % (failed == 0))
    return 0 if failed == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
