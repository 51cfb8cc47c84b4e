"""Lockstep cost model of the repeat masks (analysis only; based on tools/walk_sim.py): replays the
per-lane step records of sampled 8x8 primary-ray blocks under walk_sim's schedule (A) -- pop +
internal-node block every iteration, the leaf-children loop as long as any lane has a surviving
leaf child, the sphere loop as long as any lane has a sphere -- once from the counting walk (every
surviving leaf child tested: the walk without masks) and once from the non-counting walk of the
library loaded, whose leaf_kids drops what repeat mask A names (the variant ort_debug_leaf_dedup
reports: 1; the builds without masks and with masks A and B, the table's other rows in
profiles/leaf_dedup/ab.md, existed up to commit 83a4824).
Prints per ray the steps, leaf-child visits and sphere tests, and per 64-lane block the leaf-loop
trips and the model's VALU, with the walk's own totals from ort_debug_leaf_dedup beside them.
usage: [ORT_LIB=<analysis library>] python tools/leaf_dedup_sim.py [config] [block_step]"""
import ctypes as C
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import octreeraytracer_amd as ort  # noqa: E402
from octreeraytracer_amd import _lib as L  # noqa: E402

POP, INTERNAL, KID, OBJ = 45, 63, 15, 45  # walk_sim.py's constants (VALU instructions)
# what a trip of leaf_kids spends on the masks (v_bfe_i32, v_and_b32, v_bfi_b32; with set B also
# v_lshrrev_b32, v_bfe_i32, v_and_or_b32 in place of nothing), and a leaf-children node on their
# rank bits (address and ds_read_u8 per mask)
MASK_TRIP = {0: 0, 1: 3, 2: 6}
MASK_NODE = {0: 0, 1: 3, 2: 7}


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "c3"
    step = int(sys.argv[2]) if len(sys.argv) > 2 else 37
    W, H, N, D, M, NS, MD = bench.CONFIGS[cfg]
    s = ort.random_spheres(N, 42)
    t = ort.build_octree(s, D, M)
    p = ort.FrameParams.default_camera(W, H, num_samples=NS, max_depth=MD)
    lib = C.CDLL(os.environ["ORT_LIB"]) if os.environ.get("ORT_LIB") else L.analysis_lib()
    f = lib.ort_debug_walk_steps_ex
    f.restype = C.c_int64
    fp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    arr = [np.ascontiguousarray(x) for x in (s.center_radius, s.mat_albedo, s.fuzz_ri)]
    tt = [np.ascontiguousarray(x) for x in (t.node_min, t.node_max, t.children_offset, t.objects_offset,
                                             t.object_count, t.object_indices)]
    nw = ((W + 7) // 8 * ((H + 7) // 8) + step - 1) // step
    lib.ort_debug_leaf_dedup.restype = C.c_int
    totals = (C.c_uint64 * 3)()

    def walk(production):
        lens = np.zeros(nw * 64, np.int32)
        cap = nw * 64 * 200
        steps = np.zeros(cap, np.uint16)
        lib.ort_debug_leaf_dedup(totals, C.c_int32(1))
        n = f(fp(arr[0]), fp(arr[1]), fp(arr[2]), C.c_int32(s.n), fp(tt[0]), fp(tt[1]), fp(tt[2]), fp(tt[3]), fp(tt[4]),
              C.c_int32(len(t.children_offset)), fp(tt[5]), C.c_int64(len(t.object_indices)), C.byref(p.to_c()),
              C.c_int32(step), C.c_int32(production), fp(lens), C.c_int64(len(lens)), fp(steps), C.c_int64(cap))
        assert n >= 0, n
        lib.ort_debug_leaf_dedup(totals, C.c_int32(0))
        return lens, steps[:n], (int(totals[0]), int(totals[1]), int(totals[2]))

    def replay(lens, steps, variant):
        offs = np.concatenate([[0], np.cumsum(lens)])
        objs = (steps & 0xff).astype(np.int64)
        kids = ((steps >> 8) & 0xf).astype(np.int64)
        lk = (steps & 0x8000) != 0
        valu = trips = blocks = 0
        for w in range(nw):
            seqs = [(objs[a:b], kids[a:b], lk[a:b]) for a, b in ((offs[64 * w + l], offs[64 * w + l + 1]) for l in range(64))
                    if b > a]
            if not seqs:
                continue
            blocks += 1
            for k in range(max(len(o) for o, _, _ in seqs)):
                mo = mk = 0
                any_lk = False
                for o, kd, f_lk in seqs:
                    if k < len(o):
                        mo, mk, any_lk = max(mo, o[k]), max(mk, kd[k]), any_lk or bool(f_lk[k])
                valu += POP + INTERNAL + (MASK_NODE[variant] if any_lk else 0)
                if mk:
                    valu += (KID + MASK_TRIP[variant]) * mk + OBJ * mo
                    trips += mk
        rays = int(np.count_nonzero(lens))
        return {"blocks": blocks, "rays": rays, "steps": len(steps) / rays, "visits": kids.sum() / rays,
                "tests": objs.sum() / rays, "trips": trips / blocks, "valu": valu / blocks}

    base_lens, base_steps, _ = walk(0)
    base = replay(base_lens, base_steps, 0)
    lens, steps, (tested, dropped, variant) = walk(1)
    got = replay(lens, steps, variant)
    print(f"{cfg}: {base['blocks']} blocks, {base['rays']} walking rays (every {step}th 8x8 block)")
    for name, r in (("no masks (the counting walk)", base), (f"repeat masks, variant {variant} (this library)", got)):
        print(f"{name:36s} per ray: {r['steps']:.1f} steps, {r['visits']:.2f} leaf-child visits, {r['tests']:.2f} sphere tests; "
              f"per block: {r['trips']:.1f} leaf-loop trips, model VALU {r['valu']:,.0f} "
              f"({100 * (r['valu'] / base['valu'] - 1):+.1f} %)")
    print(f"the walk's own count (ort_debug_leaf_dedup): {tested} leaf children tested, {dropped} dropped by a mask "
          f"({dropped / max(got['rays'], 1):.2f} per ray)")


if __name__ == "__main__":
    main()
