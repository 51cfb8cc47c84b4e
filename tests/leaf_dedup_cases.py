"""Helpers shared by tests/test_leaf_dedup.py (host walk) and tests/test_gpu_leaf_dedup.py (kernels):
the camera walk's records with repeat masks (KScene::cam_node: render_core.h leaf_repeat_masks /
cam_record) through the analysis library's export hooks, the rule they follow restated in Python,
the hook that counts the leaf children the host walk tested and dropped, and the scenes: a hand-made
depth-2 tree whose leaf-children nodes hold every grouping the rule distinguishes, eight spheres
large against the leaf cell, and a seeded 2,000-sphere depth-6 tree.

Run as a program (with ORT_LIB naming the analysis library, in a process of its own: the export
hooks are not part of libort.so) it uploads the hand-made tree and the depth-6 tree, builds the
latter on the GPU too, and compares the device's cam_node with the host's word for word."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from octreeraytracer_amd import _lib as L  # noqa: E402

from leaf_inline_cases import TAG, _tree_args, layout_arrays  # noqa: E402

INTERNAL = 0x80000000
LEAFKIDS = 0x40000000
MASK_BITS = 0x00FFFF00
_U64P = C.POINTER(C.c_uint64)


# ---- the hooks -----------------------------------------------------------------------------------
def dedup_counts(reset=True):
    """(leaf children tested, leaf children dropped untested by a repeat mask, the build's
    Masks64::kLeafDedup) of the host's non-counting camera walks since the last reset."""
    lib = L.analysis_lib()
    lib.ort_debug_leaf_dedup.restype = C.c_int
    lib.ort_debug_leaf_dedup.argtypes = [_U64P, C.c_int32]
    out = (C.c_uint64 * 3)()
    L.acheck(lib.ort_debug_leaf_dedup(out, 1 if reset else 0))
    return int(out[0]), int(out[1]), int(out[2])


def host_cam_node(s, t):
    """cam_node[n, 2] as HostScene::build derives it (empty for a tree deeper than 8)."""
    lib = L.analysis_lib()
    lib.ort_debug_layout.restype = C.c_int
    lib.ort_debug_layout.argtypes = [L._fp, C.c_int32, L._fp, L._fp, L._ip, L._ip, L._ip, C.c_int32, L._ip, C.c_int64,
                                     C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    keep, args = _tree_args(s, t)
    n = C.c_int64()
    L.acheck(lib.ort_debug_layout(*args, b"cam_node", None, 0, C.byref(n)))
    a = np.zeros(n.value // 4, np.uint32)
    if n.value:
        L.acheck(lib.ort_debug_layout(*args, b"cam_node", a.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    del keep
    return a.reshape(-1, 2)


def device_cam_node(r):
    """A renderer's device cam_node[n, 2] (the library ORT_LIB names: the analysis library)."""
    lib = L.lib()
    lib.ort_debug_ctx_array.restype = C.c_int
    lib.ort_debug_ctx_array.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    n = C.c_int64()
    L.check(lib.ort_debug_ctx_array(r._ctx, b"cam_node", None, 0, C.byref(n)), r._ctx)
    a = np.zeros(n.value // 4, np.uint32)
    if n.value:
        L.check(lib.ort_debug_ctx_array(r._ctx, b"cam_node", a.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), r._ctx)
    return a.reshape(-1, 2)


def trace_rays(s, t, rays):
    """Per ray (fast walk taken, its entry, its t bits, the exact walk's entry, its t bits): the
    camera walk (Masks64, with the repeat masks) beside the exact compact walk, which has none."""
    lib = L.analysis_lib()
    keep, args = _tree_args(s, t)
    rays = np.ascontiguousarray(rays, np.float32)
    out = np.zeros((len(rays), 5), np.int32)
    L.acheck(lib.ort_debug_trace_rays(*args, L.fptr(rays), len(rays), 0, L.iptr(out)))
    del keep
    return out


# ---- the rule ------------------------------------------------------------------------------------
def repeat_masks(records, child_mask):
    """(A, B) octant masks of one node from its eight children's leaf16 records [8, 4]: the largest
    and the next largest set of at least two existing children with inline-form records equal in
    all four words; equal sizes go to the set holding the lowest octant."""
    groups = {}
    for o in range(8):
        if (child_mask >> o) & 1 and not (int(records[o, 3]) & TAG):
            groups.setdefault(records[o].tobytes(), []).append(o)
    sets = sorted((g for g in groups.values() if len(g) >= 2), key=lambda g: (-len(g), g[0]))
    masks = [sum(1 << o for o in g) for g in sets[:2]] + [0, 0]
    return masks[0], masks[1]


def expected_cam_node(node, l16):
    """cam_node from node[] and leaf16[] by the rule: node[], except that a leaf-children node has A in
    bits 8-15 and B in bits 16-23 of .y (both 0 where its eight children run past the arrays)."""
    cam = node.copy()
    n = len(node)
    lk = ((node[:, 1] & INTERNAL) != 0) & ((node[:, 1] & LEAFKIDS) != 0)
    for i in np.flatnonzero(lk):
        co = int(node[i, 0])
        a = b = 0
        if co + 8 <= n:
            a, b = repeat_masks(l16[co:co + 8], int(node[i, 1]) & 0xFF)
        cam[i, 1] = (int(node[i, 1]) & ~MASK_BITS & 0xFFFFFFFF) | (a << 8) | (b << 16)
    return cam


# ---- the scenes ----------------------------------------------------------------------------------
def _spheres(ort, cr):
    cr = np.asarray(cr, np.float32)
    n = len(cr)
    return ort.SphereSet.from_arrays(cr[:, :3], cr[:, 3], [0] * n, np.full((n, 3), 0.5), [0.0] * n, [1.5] * n)


def hand_tree(ort, kids, size=4.0):
    """A depth-2 tree over the box [0, size]^3.  kids[k], k = root octant: None for an empty leaf, a
    list of sphere ids for a leaf, or a list of eight such entries for an internal node whose
    children are those leaves.  Octant bit 1 = x, bit 0 = y, bit 2 = z, as the builder numbers them."""
    from octreeraytracer_amd.scene import FlatOctree
    bit = lambda k: np.array([(k >> 1) & 1, k & 1, (k >> 2) & 1], np.float32)  # noqa: E731
    lo, hi, co, oo, cnt, idx = [[0, 0, 0]], [[size] * 3], [1], [-1], [0], []

    def leaf(box_lo, w, ids):
        lo.append(list(box_lo))
        hi.append(list(box_lo + w))
        co.append(-1)
        oo.append(len(idx) if ids else -1)
        cnt.append(len(ids) if ids else 0)
        idx.extend(ids or [])

    inner = []
    for k in range(8):
        box = bit(k) * (size / 2)
        if kids[k] is not None and len(kids[k]) == 8 and all(e is None or isinstance(e, (list, tuple)) for e in kids[k]):
            lo.append(list(box))
            hi.append(list(box + size / 2))
            co.append(-2)  # (set below)
            oo.append(-1)
            cnt.append(0)
            inner.append((k, len(co) - 1, box))
        else:
            leaf(box, size / 2, kids[k])
    for k, at, box in inner:
        co[at] = len(co)
        for j in range(8):
            leaf(box + bit(j) * (size / 4), size / 4, kids[k][j])
    return FlatOctree(np.array(lo, np.float32), np.array(hi, np.float32), np.array(co, np.int32), np.array(oo, np.int32),
                      np.array(cnt, np.int32), np.array(idx, np.int32))


# sphere ids of the grouping tree: 0 and 1 the repeated ones; 2 with a NaN radius; 3 and 4 share a
# centre, not a radius; 5 and 6 are the same bits under two ids; 7-9 fill in
GROUP_SPHERES = [(0.5, 0.5, 0.5, 0.3), (1.5, 0.5, 0.5, 0.25), (0.5, 1.5, 0.5, float("nan")), (2.5, 0.5, 0.5, 0.2),
                 (2.5, 0.5, 0.5, 0.21), (0.5, 2.5, 0.5, 0.2), (0.5, 2.5, 0.5, 0.2), (2.5, 2.5, 0.5, 0.2), (0.5, 0.5, 2.5, 0.2),
                 (2.5, 0.5, 2.5, 0.2)]
# root octant -> (the node's eight leaves, expected A, expected B)
GROUP_NODES = {
    # three children with sphere 0, two with sphere 1, a two-sphere leaf, an empty leaf, a NaN one-sphere leaf
    0: ([[2], [1], [0], [0, 1], [1], [0], None, [0]], 0b10100100, 0b00010010),
    # equal in centre but not in radius: no set
    1: ([[3], [4], None, None, None, None, None, None], 0, 0),
    # two sphere ids with identical bits: one set
    2: ([None, None, [5], [6], None, None, None, None], 0b00001100, 0),
    # a tie of sizes goes to the lowest octant
    3: ([[0], [1], [1], [0], None, None, None, None], 0b00001001, 0b00000110),
    # three sets of two: the two holding the lowest octants
    4: ([[7], [7], [1], [1], [0], [0], None, None], 0b00000011, 0b00001100),
    # the larger set wins although it starts at a higher octant
    5: ([[0], [0], [1], [1], [1], None, [8], None], 0b00011100, 0b00000011),
    # no repeated sphere
    6: ([[0], [1], [3], [5], [7], [8], [9], [0, 1]], 0, 0),
}


@functools.lru_cache(maxsize=None)
def group_scene():
    """(spheres, tree) of the grouping tree: root octants 0-6 the nodes of GROUP_NODES, octant 7 a
    one-sphere leaf of the root (so the root is no leaf-children node)."""
    import octreeraytracer_amd as ort
    kids = [GROUP_NODES[k][0] for k in range(7)] + [[9]]
    return _spheres(ort, GROUP_SPHERES), hand_tree(ort, kids)


@functools.lru_cache(maxsize=None)
def behind_scene():
    """A leaf-children node (root octant 0, the box [0, 2]^3, leaves of side 1) seen along (+, +, +):
    set A = octants 0, 1, 2, 4 holds sphere 0, which lies in a corner no ray below comes near; set
    B = octants 3, 5, 6 holds sphere 1, which sits in octant 7's cell; octant 7 lists both.  A ray
    from below the origin towards sphere 1 rejects A's sphere once and hits in a B member or in
    the list-form leaf behind them."""
    import octreeraytracer_amd as ort
    s = _spheres(ort, [(0.1, 1.9, 0.1, 0.05), (1.5, 1.5, 1.5, 0.45)])
    node = [[0], [0], [0], [1], [0], [1], [1], [0, 1]]
    return s, hand_tree(ort, [node] + [None] * 7)


def behind_rays(n=400, seed=5):
    rng = np.random.default_rng(seed)
    o = np.array([-0.9, -1.1, -1.0], np.float32) + rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
    target = np.array([1.5, 1.5, 1.5], np.float32) + rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return np.concatenate([o, d.astype(np.float32)], axis=1)


BIG_CENTRE = (0.3, 1.7, -0.4)  # pop_table_cases.EYE: the eight DIAGONALS poses look at one sphere each


@functools.lru_cache(maxsize=None)
def big_scene():
    """Eight spheres of radius about a quarter of the world around BIG_CENTRE, one per diagonal, in a
    depth-4 tree: a sphere fills many leaf cells, so sibling leaves repeat it."""
    import octreeraytracer_amd as ort
    rng = np.random.default_rng(11)
    cr = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                c = np.array(BIG_CENTRE) + 1.2 * np.array([sx, sy, sz]) + rng.uniform(-0.1, 0.1, 3)
                cr.append((*c, rng.uniform(0.9, 1.1)))
    s = _spheres(ort, cr)
    return s, ort.build_octree(s, 4, 0)


@functools.lru_cache(maxsize=None)
def seeded_scene(depth=6):
    import octreeraytracer_amd as ort
    s = ort.random_spheres(2000, 7)
    return s, ort.build_octree(s, depth, 0)


# ---- the device's array against the host's (run as a program) -------------------------------------
def main():
    import octreeraytracer_amd as ort
    failed = 0
    with ort.Renderer(0) as r:
        for name, (s, t), built in (("grouping tree", group_scene(), None), ("2000 spheres depth 6", seeded_scene(), (6, 0))):
            host = host_cam_node(s, t)
            node, _, l16 = layout_arrays(s, t)
            r.upload(s, t)
            routes = [("uploaded", device_cam_node(r))]
            if built:
                r.build_scene(s, *built)
                routes.append(("built", device_cam_node(r)))
            ok = len(host) == t.n_nodes and np.array_equal(host, expected_cam_node(node, l16))
            ok = ok and all(d.shape == host.shape and np.array_equal(d, host) for _, d in routes)
            masks = int((host != node).any(axis=1).sum()) if host.shape == node.shape else -1
            print("%-22s %7d nodes, %6d records differ from node[], %s: %s" % (
                name, t.n_nodes, masks, " and ".join(n for n, _ in routes), "equal" if ok else "DIFFERENT"))
            failed += 0 if ok else 1
    print("cam_node all equal: %s" % (failed == 0))
    return 0 if failed == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
