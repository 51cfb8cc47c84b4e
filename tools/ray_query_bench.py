"""Ray-query throughput (ort_trace_rays) beside the render path's, in one process on one GPU.

The C3 scene (100k spheres, depth 8, built by ort_build_scene); 2^22 rays, device in and out;
3 warm-up and 20 timed calls per variant, the variants alternating call by call so that drift
hits all alike; the time is ort_last_query_ms (HIP events around the query's kernels, the sort's
included).  Three ray sets:
  pinhole  through the pixel centres of C3's camera (3840 x 2160), the centred 2048 x 2048
           window in raster order, directions normalised
  pinhole8x8  the same rays, every 64 consecutive ones an 8 x 8 pixel block (a wave of the render
           path's camera-ray kernel holds such a block), the blocks in raster order
  inside   origins uniform in the root box, directions uniform on the sphere (incoherent)
each with ORT_QUERY_SORT off and on.  Then, same process, the render path for the same camera (1
sample, 1 bounce), its camera-ray trace kernel (ort_last_trace_ms) as rays per second: the
2048 x 2048 window as a tile -- the pixels whose centres the pinhole rays go through -- and the
whole C3 frame.

Writes throughput.md and throughput.json into --out (default profiles/ray_query).
usage: python tools/ray_query_bench.py [--calls 20] [--warmup 3] [--log2-rays 22] [--out DIR]     (GPU)
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import octreeraytracer_amd as ort  # noqa: E402
from oracle import oracle  # noqa: E402

W, H, SPHERES, DEPTH = 3840, 2160, 100_000, 8


def pinhole_rays(p, side):
    cam = oracle.camera(p)[:12].astype(np.float64).reshape(4, 3)  # origin, lower-left, horizontal, vertical
    x0, y0 = (W - side) // 2, (H - side) // 2
    u = (np.arange(x0, x0 + side) + 0.5) / W
    v = (np.arange(y0, y0 + side) + 0.5) / H
    d = cam[1] + u[None, :, None] * cam[2] + v[:, None, None] * cam[3] - cam[0]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    rays = np.empty((side * side, 6), np.float32)
    rays[:, :3] = cam[0]
    rays[:, 3:] = d.reshape(-1, 3)
    return rays


def block_order(rays, side):
    """Raster order -> 8 x 8 blocks (each block's 64 rays consecutive, rows first), blocks in raster order."""
    r = rays.reshape(side // 8, 8, side // 8, 8, 6).transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(r).reshape(-1, 6)


def inside_rays(lo, hi, n, seed=1):
    rng = np.random.default_rng(seed)
    rays = np.empty((n, 6), np.float32)
    rays[:, :3] = lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return rays


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2-rays", type=int, default=22)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ray_query"))
    a = ap.parse_args()
    side = 1 << (a.log2_rays // 2)
    n = side * side
    s = ort.random_spheres(SPHERES, 42)
    p = ort.FrameParams.default_camera(W, H)
    res = {"device": torch.cuda.get_device_name(0), "rays": n, "calls": a.calls, "warmup": a.warmup, "sets": {}}
    with ort.Renderer(0) as r:
        r.build_scene(s, DEPTH, 0, keep_tree=True)
        tree = r.export_octree()
        lo, hi = tree.node_min[0].astype(np.float64), tree.node_max[0].astype(np.float64)
        pin = pinhole_rays(p, side)
        sets = {"pinhole": pin, "pinhole8x8": block_order(pin, side), "inside": inside_rays(lo, hi, n)}
        dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in sets.items()}
        out = {(k, srt): torch.empty((n, 2), dtype=torch.int32, device="cuda:0") for k in sets for srt in (False, True)}
        torch.cuda.synchronize()
        ms = {key: [] for key in out}
        for i in range(a.warmup + a.calls):  # alternating: set by set, sort off then on
            for key in out:
                r.trace_rays(dev[key[0]], sort=key[1], out=out[key])
                if i >= a.warmup:
                    ms[key].append(r.last_query_ms())
        for k in sets:
            o0, o1 = out[(k, False)].cpu().numpy(), out[(k, True)].cpu().numpy()
            same = bool(np.array_equal(o0, o1))
            row = {"hit_share": float((o0[:, 1] >= 0).mean()), "sorted_equals_unsorted": same}
            for srt in (False, True):
                v = ms[(k, srt)]
                row["sort_on" if srt else "sort_off"] = {
                    "ms_median": pct(v, 0.5), "ms_p10": pct(v, 0.1), "ms_p90": pct(v, 0.9),
                    "mrays_median": n / pct(v, 0.5) / 1e3, "mrays_p10": n / pct(v, 0.9) / 1e3,
                    "mrays_p90": n / pct(v, 0.1) / 1e3}
            res["sets"][k] = row
        # the render path on the same camera: the camera-ray trace kernel of the window tile (the
        # pinhole set's own pixels) and of the whole C3 frame
        x0, y0 = (W - side) // 2, (H - side) // 2
        for name, tile, pixels in (("render_window", ort.Tile(x0, side, y0, side), n), ("render_c3", None, W * H)):
            frame = torch.empty((tile.rows if tile else H, tile.width if tile else W, 3), dtype=torch.float32, device="cuda:0")
            tr, fr = [], []
            for i in range(a.warmup + a.calls):
                r.render(p, tile, out=frame)
                if i >= a.warmup:
                    tr.append(r.last_trace_ms())
                    fr.append(r.last_kernel_ms())
            res[name] = {"pixels": pixels, "trace_ms_median": pct(tr, 0.5), "trace_ms_p10": pct(tr, 0.1),
                         "trace_ms_p90": pct(tr, 0.9), "frame_ms_median": pct(fr, 0.5),
                         "trace_mrays_median": pixels / pct(tr, 0.5) / 1e3, "trace_mrays_p10": pixels / pct(tr, 0.9) / 1e3,
                         "trace_mrays_p90": pixels / pct(tr, 0.1) / 1e3, "frame_mrays_median": pixels / pct(fr, 0.5) / 1e3}
    lines = [f"Ray queries on the C3 scene ({SPHERES} spheres, depth {DEPTH}), {n} rays, device in/out, {a.warmup} warm-up + "
             f"{a.calls} timed calls per variant, alternating, one process, {res['device']}.",
             "Query time: ort_last_query_ms (the sort's kernels included).  Mrays/s: median (p10-p90).", "",
             "| ray set | hit share | sort | ms median | ms p10-p90 | Mrays/s |", "|---|---|---|---|---|---|"]
    for k, row in res["sets"].items():
        for srt in ("sort_off", "sort_on"):
            q = row[srt]
            lines.append(f"| {k} | {row['hit_share']:.3f} | {srt[5:]} | {q['ms_median']:.3f} | {q['ms_p10']:.3f}-{q['ms_p90']:.3f} | "
                         f"{q['mrays_median']:.0f} ({q['mrays_p10']:.0f}-{q['mrays_p90']:.0f}) |")
    lines += ["", "Render path, same process and camera, 1 sample, 1 bounce; camera-ray trace kernel (ort_last_trace_ms, shading "
              "fused) and the whole frame (ort_last_kernel_ms):", "",
              "| tile | pixels | trace ms median | p10-p90 | trace Mrays/s | frame ms | frame Mrays/s |", "|---|---|---|---|---|---|---|"]
    for name, what in (("render_window", f"the pinhole set's {side} x {side} window"), ("render_c3", f"whole frame {W} x {H}")):
        c = res[name]
        lines.append(f"| {what} | {c['pixels']} | {c['trace_ms_median']:.3f} | {c['trace_ms_p10']:.3f}-{c['trace_ms_p90']:.3f} | "
                     f"{c['trace_mrays_median']:.0f} ({c['trace_mrays_p10']:.0f}-{c['trace_mrays_p90']:.0f}) | "
                     f"{c['frame_ms_median']:.3f} | {c['frame_mrays_median']:.0f} |")
    lines += ["",
              "Sorted and unsorted records equal: " +
              ", ".join(f"{k} {row['sorted_equals_unsorted']}" for k, row in res["sets"].items()) + "."]
    text = "\n".join(lines)
    print(text, flush=True)
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "throughput.md").write_text(text + "\n")
    (outdir / "throughput.json").write_text(json.dumps(res, indent=1) + "\n")
    return 0 if all(row["sorted_equals_unsorted"] for row in res["sets"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
