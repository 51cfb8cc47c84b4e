"""Camera-query throughput (ort_trace_camera) beside the ways to the same records, in one process
on one GPU.

The C3 scene (100k spheres, depth 8, built by ort_build_scene), its 3840 x 2160 frame and the
centred 2048 x 2048 window of it, 1 sample per pixel, device output; --warmup warm-up and --calls
timed rounds, every round running the four variants one after the other so that drift hits all
alike:
  (a) ort_trace_camera, hits only                                   ort_last_query_ms
  (b) ort_trace_camera with rays and normals                        ort_last_query_ms
  (c) the rays by ort_trace_camera's ray-only mode, then ort_trace_rays over them
                                                                    the two ort_last_query_ms summed
  (d) ort_render of the 1 sample x 1 bounce frame of the same tile  ort_last_kernel_ms
(d) is the yardstick: the render path's own walk of the same rays, plus shading.  Then (a) again
under ORT_OPT_REFILL 16 (the default), 32, 48 and 64, alternating call by call.

Writes throughput.md and throughput.json into --out (default profiles/camera_query).
usage: python tools/camera_query_bench.py [--calls 20] [--warmup 3] [--out DIR]     (GPU)
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

W, H, SPHERES, DEPTH, SIDE = 3840, 2160, 100_000, 8, 2048
REFILLS = (16, 32, 48, 64)
VARIANTS = ("a_hits", "b_hits_rays_normals", "c_gen_then_trace_rays", "d_render_1x1")


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "camera_query"))
    a = ap.parse_args()
    s = ort.random_spheres(SPHERES, 42)
    p = ort.FrameParams.default_camera(W, H)
    tiles = {"frame_3840x2160": ort.Tile.full(p), "window_2048x2048": ort.Tile((W - SIDE) // 2, SIDE, (H - SIDE) // 2, SIDE)}
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "warmup": a.warmup, "tiles": {}}
    ok = True
    with ort.Renderer(0) as r:
        r.build_scene(s, DEPTH, 0)
        for tname, tile in tiles.items():
            n = tile.rows * tile.width
            dev = torch.device("cuda", 0)
            hits_a = torch.empty((n, 2), dtype=torch.int32, device=dev)
            hits_b = torch.empty((n, 2), dtype=torch.int32, device=dev)
            hits_c = torch.empty((n, 2), dtype=torch.int32, device=dev)
            rays_b = torch.empty((n, 6), dtype=torch.float32, device=dev)
            rays_c = torch.empty((n, 6), dtype=torch.float32, device=dev)
            nrm_b = torch.empty((n, 3), dtype=torch.float32, device=dev)
            frame = torch.empty((tile.rows, tile.width, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ms = {v: [] for v in VARIANTS}
            for i in range(a.warmup + a.calls):
                r.trace_camera(p, tile, out=hits_a)
                t_a = r.last_query_ms()
                r.trace_camera(p, tile, out=hits_b, rays=rays_b, normals=nrm_b)
                t_b = r.last_query_ms()
                r.trace_camera(p, tile, rays=rays_c, hits=False)
                t_c = r.last_query_ms()
                r.trace_rays(rays_c, out=hits_c)
                t_c += r.last_query_ms()
                r.render(p, tile, out=frame)
                t_d = r.last_kernel_ms()
                if i >= a.warmup:
                    for v, t in zip(VARIANTS, (t_a, t_b, t_c, t_d)):
                        ms[v].append(t)
            ha = hits_a.cpu().numpy()
            same = bool(np.array_equal(ha, hits_b.cpu().numpy()) and np.array_equal(ha, hits_c.cpu().numpy()) and
                        np.array_equal(rays_b.cpu().numpy().view(np.int32), rays_c.cpu().numpy().view(np.int32)))
            ok = ok and same
            row = {"pixels": n, "hit_share": float((ha[:, 1] >= 0).mean()), "variants_agree": same}
            for v in VARIANTS:
                row[v] = {"ms_median": pct(ms[v], 0.5), "ms_p10": pct(ms[v], 0.1), "ms_p90": pct(ms[v], 0.9),
                          "mrays_median": n / pct(ms[v], 0.5) / 1e3}
            # (a) again by ORT_OPT_REFILL (16 is the default): a lane makes its ray at refill, while the
            # wave's busy lanes wait, so the threshold sets how many lanes share that time
            by_refill = {k: [] for k in REFILLS}
            for i in range(a.warmup + a.calls):
                for k in REFILLS:
                    r.set_refill(k)
                    r.trace_camera(p, tile, out=hits_b)
                    if i >= a.warmup:
                        by_refill[k].append(r.last_query_ms())
            r.set_refill(REFILLS[0])
            row["a_by_refill"] = {str(k): {"ms_median": pct(v, 0.5), "ms_p10": pct(v, 0.1), "ms_p90": pct(v, 0.9)}
                                  for k, v in by_refill.items()}
            res["tiles"][tname] = row
            del hits_a, hits_b, hits_c, rays_b, rays_c, nrm_b, frame
    lines = [f"Camera queries on the C3 scene ({SPHERES} spheres, depth {DEPTH}), camera of the {W} x {H} frame, 1 sample, device "
             f"output, {a.warmup} warm-up + {a.calls} timed rounds of all four variants in turn, one process, {res['device']}.",
             "Times: ort_last_query_ms for (a)-(c) ((c): ray generation + ort_trace_rays summed), ort_last_kernel_ms for (d).", "",
             "| tile | pixels | hit share | variant | ms median | ms p10-p90 | Mrays/s | median / (d) |", "|---|---|---|---|---|---|---|---|"]
    for tname, row in res["tiles"].items():
        d = row["d_render_1x1"]["ms_median"]
        for v in VARIANTS:
            q = row[v]
            lines.append(f"| {tname} | {row['pixels']} | {row['hit_share']:.3f} | {v} | {q['ms_median']:.3f} | "
                         f"{q['ms_p10']:.3f}-{q['ms_p90']:.3f} | {q['mrays_median']:.0f} | {q['ms_median'] / d:.3f} |")
    lines += ["", "(a) by ORT_OPT_REFILL (default 16), the settings alternating call by call, ms median (p10-p90):", "",
              "| tile | " + " | ".join(f"refill {k}" for k in REFILLS) + " |", "|---|" + "---|" * len(REFILLS)]
    for tname, row in res["tiles"].items():
        lines.append(f"| {tname} | " + " | ".join(
            f"{q['ms_median']:.3f} ({q['ms_p10']:.3f}-{q['ms_p90']:.3f})" for q in row["a_by_refill"].values()) + " |")
    lines += ["", "Records of (a), (b) and (c) equal, rays of (b) and (c) equal: " +
              ", ".join(f"{k} {row['variants_agree']}" for k, row in res["tiles"].items()) + "."]
    text = "\n".join(lines)
    print(text, flush=True)
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "throughput.md").write_text(text + "\n")
    (outdir / "throughput.json").write_text(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
