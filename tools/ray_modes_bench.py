"""Query-mode throughput (ort_trace_rays_ex: NEAREST, ANY) beside DRAWN (ort_trace_rays), in one
process on one GPU: tools/ray_query_bench.py's scene, ray sets and timing.

The C3 scene (100k spheres, depth 8, built by ort_build_scene); 2^22 rays, device in and out; 3
warm-up and 20 timed calls per variant, the variants alternating call by call; the time is
ort_last_query_ms.  Ray sets pinhole, pinhole8x8 and inside as in tools/ray_query_bench.py, sort off.
Variants:
  drawn        ort_trace_rays, the comparison
  nearest      the default interval (0.001, MAXFLOAT)
  any          the default interval: the walk ends at the first hit
  any_segment  intervals (0.001, f * t_near), f uniform in (0, 2) per ray and t_near the ray's
               nearest t (the root box's diagonal for a miss): about half of the hit rays' intervals
               end before the nearest sphere, and those rays walk their whole interval and miss
Checks on the way: NEAREST's hit flags equal ANY's under the default interval, and NEAREST equals
brute force (ort_trace_rays, use_octree = 0) on the first 2^14 rays of every set.

Writes throughput.md and throughput.json into --out (default profiles/ray_modes).
usage: python tools/ray_modes_bench.py [--calls 20] [--warmup 3] [--log2-rays 22] [--commit HASH] [--out DIR]     (GPU)
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

import octreeraytracer_amd as ort  # noqa: E402
from ray_query_bench import DEPTH, H, SPHERES, W, block_order, inside_rays, pct, pinhole_rays  # noqa: E402

VARIANTS = ("drawn", "nearest", "any", "any_segment")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2-rays", type=int, default=22)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ray_modes"))
    a = ap.parse_args()
    side = 1 << (a.log2_rays // 2)
    n = side * side
    s = ort.random_spheres(SPHERES, 42)
    p = ort.FrameParams.default_camera(W, H)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "rays": n, "calls": a.calls, "warmup": a.warmup, "sets": {}}
    ok = True
    with ort.Renderer(0) as r:
        r.build_scene(s, DEPTH, 0, keep_tree=True)
        tree = r.export_octree()
        lo, hi = tree.node_min[0].astype(np.float64), tree.node_max[0].astype(np.float64)
        diag = float(np.linalg.norm(hi - lo))
        pin = pinhole_rays(p, side)
        sets = {"pinhole": pin, "pinhole8x8": block_order(pin, side), "inside": inside_rays(lo, hi, n)}
        dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in sets.items()}
        out = {(k, v): torch.empty((n, 2), dtype=torch.int32, device="cuda:0") for k in sets for v in VARIANTS}
        seg = {}
        rng = np.random.default_rng(3)
        for k in sets:  # the segments' intervals, from one NEAREST call
            o = r.trace_rays(dev[k], mode="nearest", out=out[(k, "nearest")]).cpu().numpy()
            t_near = np.where(o[:, 1] >= 0, np.ascontiguousarray(o[:, 0]).view(np.float32), np.float32(diag)).astype(np.float64)
            iv = np.stack([np.full(n, 0.001), t_near * rng.uniform(0.0, 2.0, n)], axis=1).astype(np.float32)
            seg[k] = torch.from_numpy(iv).to("cuda:0")
        torch.cuda.synchronize()

        def call(k, v):
            if v == "drawn":
                r.trace_rays(dev[k], out=out[(k, v)])
            elif v == "any_segment":
                r.trace_rays(dev[k], out=out[(k, v)], mode="any", t_range=seg[k])
            else:
                r.trace_rays(dev[k], out=out[(k, v)], mode=v)

        ms = {key: [] for key in out}
        for i in range(a.warmup + a.calls):  # alternating: set by set, variant by variant
            for key in out:
                call(*key)
                if i >= a.warmup:
                    ms[key].append(r.last_query_ms())
        m = 1 << 14
        for k in sets:
            o = {v: out[(k, v)].cpu().numpy() for v in VARIANTS}
            brute = r.trace_rays(dev[k][:m].contiguous(), use_octree=False).cpu().numpy()
            row = {"nearest_equals_brute_force_prefix": bool(np.array_equal(o["nearest"][:m], brute)),
                   "any_flags_equal_nearest": bool(np.array_equal(o["any"][:, 1] >= 0, o["nearest"][:, 1] >= 0)),
                   "drawn_differs_from_nearest": int((o["drawn"] != o["nearest"]).any(axis=1).sum())}
            ok = ok and row["nearest_equals_brute_force_prefix"] and row["any_flags_equal_nearest"]
            for v in VARIANTS:
                t = ms[(k, v)]
                row[v] = {"hit_share": float((o[v][:, 1] >= 0).mean()), "ms_median": pct(t, 0.5), "ms_p10": pct(t, 0.1),
                          "ms_p90": pct(t, 0.9), "mrays_median": n / pct(t, 0.5) / 1e3, "mrays_p10": n / pct(t, 0.9) / 1e3,
                          "mrays_p90": n / pct(t, 0.1) / 1e3}
            res["sets"][k] = row
    lines = [f"Query modes on the C3 scene ({SPHERES} spheres, depth {DEPTH}), {n} rays, device in/out, sort off, {a.warmup} warm-up + "
             f"{a.calls} timed calls per variant, alternating, one process, {res['device']}" +
             (f", commit {a.commit}" if a.commit else "") + ".",
             "Query time: ort_last_query_ms.  Mrays/s: median (p10-p90).  vs drawn: the variant's median time over DRAWN's, same set.", "",
             "| ray set | variant | hit share | ms median | ms p10-p90 | Mrays/s | vs drawn |", "|---|---|---|---|---|---|---|"]
    for k, row in res["sets"].items():
        for v in VARIANTS:
            q = row[v]
            lines.append(f"| {k} | {v} | {q['hit_share']:.3f} | {q['ms_median']:.3f} | {q['ms_p10']:.3f}-{q['ms_p90']:.3f} | "
                         f"{q['mrays_median']:.0f} ({q['mrays_p10']:.0f}-{q['mrays_p90']:.0f}) | "
                         f"{q['ms_median'] / row['drawn']['ms_median']:.2f}x |")
    lines += ["", "Checks: " + "; ".join(
        f"{k}: NEAREST equals brute force on the first {m} rays {row['nearest_equals_brute_force_prefix']}, ANY's flags equal "
        f"NEAREST's {row['any_flags_equal_nearest']}, rays whose DRAWN record differs from NEAREST's {row['drawn_differs_from_nearest']}"
        for k, row in res["sets"].items()) + "."]
    text = "\n".join(lines)
    print(text, flush=True)
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "throughput.md").write_text(text + "\n")
    (outdir / "throughput.json").write_text(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
