"""Radiance-query throughput (ort_trace_radiance) beside the render path's trace of the same paths,
in one process on one GPU.

config.h's default scene (100 spheres, seed 42, depth 3) and frame (800 x 600) at 1 sample x 8
bounces, device pointers; --warmup warm-up and --calls timed rounds, every round running the
variants one after the other so that drift hits all alike:
  (a) ort_trace_radiance over the frame's first-sample rays (ort_trace_camera's) and six-draw
      states, paths = 1, ORT_RADIANCE_GAMMA                          ort_last_query_ms
  (b) ort_render of that frame with ORT_OPT_PIXEL_PATHS 1            ort_last_kernel_ms
  (a_sort)    (a) with ORT_QUERY_SORT (the sort's kernels included)  ort_last_query_ms
  (a_paths16) (a) with paths = 16                                    ort_last_query_ms
(b) is the yardstick: the same paths by the same loop, without the 32 B read and 12-20 B write per
ray.  (a)'s records must equal (b)'s frame bit for bit.

Writes throughput.md and throughput.json into --out (default profiles/radiance_query); --bench-log
appends the lines of a file (the plain bench.py runs on this change and on its parent) to the .md.
usage: python tools/radiance_query_bench.py [--calls 30] [--warmup 5] [--out DIR]     (GPU)
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

W, H, SPHERES, SEED, DEPTH, BOUNCES = 800, 600, 100, 42, 3, 8
VARIANTS = ("a_radiance", "b_render_pixel_paths", "a_sort", "a_paths16")
F = np.float32


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def rand2d(x, y):
    """The shader's rand2D on arrays of states, in float32 and uint32 as ort_rand2D does it:
    returns the new (x, y); y is the draw."""
    with np.errstate(over="ignore"):
        total = ((x * F(1664525.0)).astype(F) + (y * F(1013904192.0)).astype(F)).astype(F)
        s = total.astype(np.uint32) + np.uint32(1013904223)
        s ^= s >> np.uint32(16)
        s *= np.uint32(0x85ebca6b)
        s ^= s >> np.uint32(13)
        s *= np.uint32(0xc2b2ae35)
        s ^= s >> np.uint32(16)
    nx = (y * F(1664525.0)).astype(F)
    nx = (nx - np.floor(nx)).astype(F)
    ny = (s.astype(F) / F(4294967296.0)).astype(F)
    ny = (ny - np.floor(ny)).astype(F)
    return nx, ny


def six_draw_states(w, h):
    """(w * h, 2): every pixel's seed ((x + 0.5) / w, (y + 0.5) / h) advanced by the six draws that
    make its first-sample ray (2 stratum, 2 jitter, 2 disk), rows bottom-up as the frame's."""
    xs = ((np.arange(w, dtype=F) + F(0.5)) / F(w)).astype(F)
    ys = ((np.arange(h, dtype=F) + F(0.5)) / F(h)).astype(F)
    x, y = np.tile(xs, h), np.repeat(ys, w)
    for _ in range(6):
        x, y = rand2d(x, y)
    return np.ascontiguousarray(np.stack([x, y], axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "radiance_query"))
    ap.add_argument("--bench-log", default="")
    a = ap.parse_args()
    s = ort.random_spheres(SPHERES, SEED)
    p = ort.FrameParams.default_camera(W, H, num_samples=1, max_depth=BOUNCES)
    n = W * H
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "warmup": a.warmup, "rays": n}
    with ort.Renderer(0) as r:
        r.build_scene(s, DEPTH, 0)
        r.set_pixel_paths(1)
        rays = torch.empty((n, 6), dtype=torch.float32, device=dev)
        r.trace_camera(p, rays=rays, hits=False)
        states = torch.from_numpy(six_draw_states(W, H)).to(dev)
        out = {v: torch.empty((n, 3), dtype=torch.float32, device=dev) for v in VARIANTS}
        torch.cuda.synchronize()
        ms = {v: [] for v in VARIANTS}
        for i in range(a.warmup + a.calls):
            r.trace_radiance(rays, states, max_depth=BOUNCES, gamma=True, out=out["a_radiance"])
            t_a = r.last_query_ms()
            r.render(p, out=out["b_render_pixel_paths"].view(H, W, 3))
            t_b = r.last_kernel_ms()
            r.trace_radiance(rays, states, max_depth=BOUNCES, gamma=True, sort=True, out=out["a_sort"])
            t_s = r.last_query_ms()
            r.trace_radiance(rays, states, max_depth=BOUNCES, gamma=True, paths=16, out=out["a_paths16"])
            t_p = r.last_query_ms()
            if i >= a.warmup:
                for v, t in zip(VARIANTS, (t_a, t_b, t_s, t_p)):
                    ms[v].append(t)
        img = {v: o.cpu().numpy().view(np.int32) for v, o in out.items()}
        same = bool(np.array_equal(img["a_radiance"], img["b_render_pixel_paths"]) and np.array_equal(img["a_radiance"], img["a_sort"]))
        res["a_equals_b"] = same
        res["info"] = r.info()
    for v in VARIANTS:
        paths = 16 if v == "a_paths16" else 1
        res[v] = {"ms_median": pct(ms[v], 0.5), "ms_p10": pct(ms[v], 0.1), "ms_p90": pct(ms[v], 0.9),
                  "mpaths_median": n * paths / pct(ms[v], 0.5) / 1e3}
    b = res["b_render_pixel_paths"]
    res["a_over_b"] = res["a_radiance"]["ms_median"] / b["ms_median"]
    res["a_inside_b_spread"] = bool(b["ms_p10"] <= res["a_radiance"]["ms_median"] <= b["ms_p90"])
    lines = [f"Radiance queries on config.h's default scene ({SPHERES} spheres, seed {SEED}, depth {DEPTH}) and frame ({W} x {H}), "
             f"1 sample x {BOUNCES} bounces, device pointers, {a.warmup} warm-up + {a.calls} timed rounds of all variants in turn, "
             f"one process, {res['device']}.",
             "Times: ort_last_query_ms for the (a) rows, ort_last_kernel_ms for (b).", "",
             "| variant | paths | ms median | ms p10-p90 | Mpaths/s | median / (b) |", "|---|---|---|---|---|---|"]
    for v in VARIANTS:
        q = res[v]
        lines.append(f"| {v} | {n * (16 if v == 'a_paths16' else 1)} | {q['ms_median']:.4f} | {q['ms_p10']:.4f}-{q['ms_p90']:.4f} | "
                     f"{q['mpaths_median']:.0f} | {q['ms_median'] / b['ms_median']:.3f} |")
    lines += ["", f"(a) / (b) = {res['a_over_b']:.3f}; (a)'s median inside (b)'s p10-p90: {res['a_inside_b_spread']}.",
              f"Records of (a) and (a_sort) equal (b)'s frame bit for bit: {same}."]
    if a.bench_log and Path(a.bench_log).exists():
        lines += ["", "bench.py --gpus 1 on this change and on its parent (the parent's library through ORT_LIB), alternating:", "", "```"]
        lines += Path(a.bench_log).read_text().splitlines() + ["```"]
    text = "\n".join(lines)
    print(text, flush=True)
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "throughput.md").write_text(text + "\n")
    (outdir / "throughput.json").write_text(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
