"""Temporal reprojection timings (ort_history_update) beside a device-to-device copy of its compulsory
bytes, and what an update adds to the preview, in one process on one GPU.

Points: 1280 x 720 and 3840 x 2160, device pointers, the library's defaults, on a seeded random
picture with a synthetic hit field (discs of distinct sphere ids over a sky of misses; the pixel-centre
rays are ort_trace_camera's without hits, so no scene is needed).  The camera alternates between two
poses a fraction of a pixel apart, so that every update projects and loads its four taps; a second
column times the same-camera path (one tap).  --warmup warm-up and --calls timed rounds, every round
running all points and their copies one after the other so that drift hits all alike.
  update    ort_history_last_update_ms: the one kernel (HIP events on the call's stream)
  copy      one device-to-device copy that reads and writes the update's compulsory bytes -- per pixel
            12 + 24 + 8 B read from the caller (sample, ray, hit record), 32 B of history read and 32 B
            written, 12 + 4 + 4 B written out (colour, variance, length): 128 B, so a copy of 64 B a
            pixel (it reads and writes each byte once), timed with events around it.  (The projecting
            update reads up to four previous records of each kind per pixel; for a slow camera they are
            its neighbours' and come from the cache, so 32 B stays the compulsory figure.)
Context: config.h's default scene (100 spheres, seed 42, depth 3) and frame (800 x 600), 8 bounces: a
one-sample accumulation pass, the pixel-centre camera query with rays, the update and the
variance-guided denoise with gamma of its colour, beside the plain denoise of the one-sample picture.

Writes ab.md and ab.json into --out (default profiles/reproject); --bench-log appends the lines of a
file (the plain bench.py runs on this change and on its parent) to the .md.
usage: python tools/reproject_ab.py [--calls 50] [--warmup 5] [--out DIR]     (GPU)
"""
import argparse
import dataclasses
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

import octreeraytracer_amd as ort  # noqa: E402
from denoise_ab import guide_field, pct  # noqa: E402

SIZES = ((1280, 720), (3840, 2160))
BYTES_PER_PIXEL = (12 + 24 + 8) + 32 + 32 + (12 + 4 + 4)
W, H, SPHERES, SEED, DEPTH, BOUNCES = 800, 600, 100, 42, 3, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "reproject"))
    ap.add_argument("--bench-log", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "warmup": a.warmup, "bytes_per_pixel": BYTES_PER_PIXEL,
           "points": []}
    points = []
    with ort.Renderer(0) as r:
        for (w, h) in SIZES:
            img = torch.rand((h, w, 3), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            rec, _, share = guide_field(w, h, dev)
            base = ort.FrameParams.default_camera(w, h)
            moved = ort.FrameParams.default_camera(w, h, position=(0.002, 2.5, -10.0))
            cams = []
            for p in (base, moved):
                rays = torch.empty((h, w, 6), dtype=torch.float32, device=dev)
                r.trace_camera(p, which="pixel_centre", rays=rays, hits=False)
                cams.append((p, rays))
            half = BYTES_PER_PIXEL * w * h // 2
            points.append(dict(w=w, h=h, img=img, rec=rec, cams=cams, share=share, hist=r.history(w, h),
                               col=torch.empty((h, w, 3), dtype=torch.float32, device=dev),
                               var=torch.empty((h, w), dtype=torch.float32, device=dev),
                               ln=torch.empty((h, w), dtype=torch.float32, device=dev),
                               src=torch.empty(half, dtype=torch.uint8, device=dev),
                               dst=torch.empty(half, dtype=torch.uint8, device=dev), ms=[], same=[], copy=[], found=0.0))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(a.warmup + a.calls):
            for q in points:
                p, rays = q["cams"][i & 1]
                kw = dict(out=q["col"], variance=q["var"], length=q["ln"])
                q["hist"].update(q["img"], p, None, (rays, q["rec"]), **kw)      # the other pose: projects
                t_u = q["hist"].last_update_ms()
                q["hist"].update(q["img"], p, None, (rays, q["rec"]), **kw)      # the same pose again: one tap
                t_s = q["hist"].last_update_ms()
                e0.record()
                q["dst"].copy_(q["src"])
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    q["ms"].append(t_u)
                    q["same"].append(t_s)
                    q["copy"].append(e0.elapsed_time(e1))
        for q in points:
            p, rays = q["cams"][0]
            q["hist"].update(q["img"], q["cams"][1][0], None, (q["cams"][1][1], q["rec"]), out=q["col"], variance=q["var"], length=q["ln"])
            q["hist"].update(q["img"], p, None, (rays, q["rec"]), out=q["col"], variance=q["var"], length=q["ln"])
            torch.cuda.synchronize()
            q["found"] = float((q["ln"] > 1).float().mean().item())   # the share of pixels the projecting update found history for
            q["hist"].close()
        # the preview: a one-sample pass of the default frame, its guides with rays, the update, the denoise
        s = ort.random_spheres(SPHERES, SEED)
        r.build_scene(s, DEPTH, 0)
        pa = ort.FrameParams.default_camera(W, H, num_samples=1, max_depth=BOUNCES)
        pb = dataclasses.replace(ort.FrameParams.default_camera(W, H, num_samples=1, max_depth=BOUNCES, position=(0.01, 2.5, -10.0)))
        pic = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        flt = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        col = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        var = torch.empty((H, W), dtype=torch.float32, device=dev)
        hits = torch.empty((H, W, 2), dtype=torch.int32, device=dev)
        nrm = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        rays = torch.empty((H, W, 6), dtype=torch.float32, device=dev)
        t = dict(pass_ms=[], guides_ms=[], update_ms=[], plain_denoise_ms=[], var_denoise_ms=[])
        with r.accumulate(pa, moments=True) as acc, r.history(W, H) as hist:
            torch.cuda.synchronize()
            for i in range(a.warmup + a.calls):
                p = pb if i & 1 else pa
                row = {}
                acc.restart(p)
                acc.step(1, out=False)
                row["pass_ms"] = acc.last_pass_ms()
                acc.moments(out_mean=pic, variance=False)
                r.trace_camera(p, which="pixel_centre", rays=rays, normals=nrm, out=hits)
                row["guides_ms"] = r.last_query_ms()
                hist.update(pic, p, None, (rays, hits), out=col, variance=var)
                row["update_ms"] = hist.last_update_ms()
                r.denoise(pic, (hits, nrm), out=flt, gamma=True)
                row["plain_denoise_ms"] = r.last_denoise_ms()
                r.denoise(col, (hits, nrm), out=flt, variance=var, gamma=True)
                row["var_denoise_ms"] = r.last_denoise_ms()
                if i >= a.warmup:
                    for k, v in row.items():
                        t[k].append(v)
    lines = [f"ort_history_update (one kernel, one lane per pixel), library defaults, device pointers, {a.warmup} warm-up + "
             f"{a.calls} timed rounds of all points in turn, one process, {res['device']}.",
             "update: ort_history_last_update_ms on a camera that moved (four taps); same camera: the one-tap path.  copy: a "
             f"device-to-device copy reading and writing the update's compulsory {BYTES_PER_PIXEL} B a pixel (half each way), "
             "events around it.", "",
             "| size | update ms median | p10-p90 | same camera ms median | p10-p90 | compulsory MB | copy ms median | p10-p90 | "
             "update / copy | pixels with history |", "|---|---|---|---|---|---|---|---|---|---|"]
    for q in points:
        d, sm, c = pct(q["ms"], 0.5), pct(q["same"], 0.5), pct(q["copy"], 0.5)
        mb = BYTES_PER_PIXEL * q["w"] * q["h"] / 1e6
        res["points"].append(dict(w=q["w"], h=q["h"], hit_share=q["share"], found_share=q["found"],
                                  update_ms=dict(median=d, p10=pct(q["ms"], 0.1), p90=pct(q["ms"], 0.9)),
                                  same_camera_ms=dict(median=sm, p10=pct(q["same"], 0.1), p90=pct(q["same"], 0.9)),
                                  copy_ms=dict(median=c, p10=pct(q["copy"], 0.1), p90=pct(q["copy"], 0.9)),
                                  compulsory_mb=mb, update_over_copy=d / c))
        lines.append(f"| {q['w']} x {q['h']} | {d:.4f} | {pct(q['ms'], 0.1):.4f}-{pct(q['ms'], 0.9):.4f} | {sm:.4f} | "
                     f"{pct(q['same'], 0.1):.4f}-{pct(q['same'], 0.9):.4f} | {mb:.1f} | {c:.4f} | "
                     f"{pct(q['copy'], 0.1):.4f}-{pct(q['copy'], 0.9):.4f} | {d / c:.2f} | {q['found']:.3f} |")
    res["preview"] = dict(frame=[W, H], bounces=BOUNCES,
                          **{k: dict(median=pct(v, 0.5), p10=pct(v, 0.1), p90=pct(v, 0.9)) for k, v in t.items()})
    lines += ["", f"The moving-camera preview at config.h's default frame ({W} x {H}, {SPHERES} spheres, {BOUNCES} bounces), the camera "
              "stepping between two poses, ms median (p10-p90):", ""]
    for k, label in (("pass_ms", "one-sample accumulation pass"), ("guides_ms", "pixel-centre camera query (rays, hits, normals)"),
                     ("update_ms", "ort_history_update"), ("plain_denoise_ms", "ort_denoise_ex of the one-sample picture (gamma)"),
                     ("var_denoise_ms", "ort_denoise_ex of the integrated colour (variance, gamma)")):
        lines.append(f"- {label}: {pct(t[k], 0.5):.4f} ({pct(t[k], 0.1):.4f}-{pct(t[k], 0.9):.4f})")
    if a.bench_log and Path(a.bench_log).exists():
        lines += ["", "bench.py --gpus 1 on this change and on its parent (the parent's library through ORT_LIB), alternating:", "", "```"]
        lines += Path(a.bench_log).read_text().splitlines() + ["```"]
    text = "\n".join(lines)
    print(text, flush=True)
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "ab.md").write_text(text + "\n")
    (outdir / "ab.json").write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
