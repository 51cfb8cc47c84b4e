"""Helpers shared by tests/test_leaf_inline.py (host walk) and tests/test_gpu_leaf_inline.py
(kernels): the compact layout's arrays and the 16-byte leaf records derived from them through the
analysis library, and the rule those records follow.  Run as a program (with ORT_LIB naming the
analysis library, in a process of its own: the export hook is not part of libort.so) it builds
the benchmark's 100k-sphere depth-8 scene on the GPU and compares the device's records with the
ones derived from the host-built tree."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from octreeraytracer_amd import _lib as L  # noqa: E402

TAG = 0x80000000
_U32P = C.POINTER(C.c_uint32)


def _tree_args(s, t):
    keep = [np.ascontiguousarray(a, d) for a, d in (
        (s.center_radius, np.float32), (t.node_min, np.float32), (t.node_max, np.float32),
        (t.children_offset, np.int32), (t.objects_offset, np.int32), (t.object_count, np.int32),
        (t.object_indices, np.int32))]
    return keep, (L.fptr(keep[0]), s.n, L.fptr(keep[1]), L.fptr(keep[2]), L.iptr(keep[3]), L.iptr(keep[4]),
                  L.iptr(keep[5]), t.n_nodes, L.iptr(keep[6]), t.n_indices)


def layout_arrays(s, t):
    """(node[n, 2], leaf_sph[e, 4], leaf16[n, 4]) of the compact layout as the host emulation walks it."""
    lib = L.analysis_lib()
    lib.ort_debug_leaf16.restype = C.c_int
    lib.ort_debug_leaf16.argtypes = [L._fp, C.c_int32, L._fp, L._fp, L._ip, L._ip, L._ip, C.c_int32, L._ip, C.c_int64,
                                     _U32P, _U32P, _U32P, C.POINTER(C.c_int64)]
    keep, args = _tree_args(s, t)
    sizes = (C.c_int64 * 3)()
    L.acheck(lib.ort_debug_leaf16(*args, None, None, None, sizes))
    node = np.zeros((sizes[0], 2), np.uint32)
    sph = np.zeros((sizes[1], 4), np.uint32)
    l16 = np.zeros((sizes[2], 4), np.uint32)
    L.acheck(lib.ort_debug_leaf16(*args, node.ctypes.data_as(_U32P), sph.ctypes.data_as(_U32P),
                                  l16.ctypes.data_as(_U32P), sizes))
    del keep
    return node, sph, l16


def expected_records(node, sph):
    """leaf16 from node[] and leaf_sph[] by the rule of the layout, and which leaves are inline."""
    internal = (node[:, 1] & TAG) != 0
    one = ~internal & (node[:, 1] == 1)
    w = np.zeros(len(node), np.uint32)
    w[one] = sph[node[one, 0], 3]
    clean = one & (w <= 0x7F800000)  # sign clear and not NaN: +0 .. +inf
    exp = np.stack([node[:, 0], node[:, 1], np.zeros(len(node), np.uint32), node[:, 1] | np.uint32(TAG)], axis=1)
    exp[clean] = sph[node[clean, 0]]
    return exp.astype(np.uint32), internal, clean



def main():
    import octreeraytracer_amd as ort
    s = ort.random_spheres(100_000, 42)
    t = ort.build_octree(s, 8, 0)
    node, sph, host = layout_arrays(s, t)
    exp, internal, inline = expected_records(node, sph)
    lib = L.lib()
    lib.ort_debug_ctx_leaf16.restype = C.c_int
    lib.ort_debug_ctx_leaf16.argtypes = [C.c_void_p, _U32P, C.c_int64, C.POINTER(C.c_int64)]
    with ort.Renderer(0) as r:
        r.build_scene(s, 8, 0)
        n = C.c_int64()
        L.check(lib.ort_debug_ctx_leaf16(r._ctx, None, 0, C.byref(n)), r._ctx)
        dev = np.zeros((n.value, 4), np.uint32)
        L.check(lib.ort_debug_ctx_leaf16(r._ctx, dev.ctypes.data_as(_U32P), n.value, C.byref(n)), r._ctx)
    leaf = ~internal
    ok = len(dev) == len(host) == t.n_nodes and np.array_equal(dev[leaf], host[leaf]) and np.array_equal(host[leaf], exp[leaf])
    print(f"leaf records: {len(dev)} device, {len(host)} host, {int(inline.sum())} inline, equal on leaves: {ok}")
    return 0 if ok and inline.sum() > 1_000_000 else 1


if __name__ == "__main__":
    sys.exit(main())
