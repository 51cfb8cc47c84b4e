"""Denoiser timings (ort_denoise) beside a device-to-device copy of its compulsory bytes, and the
preview's cost with and without it, in one process on one GPU.

Points: 1280 x 720 and 3840 x 2160, 3 and 5 iterations, RGB32F and RGBA8 output, device pointers,
the library's defaults (no colour or depth term, normal_power 5, same_sphere) on a seeded random
image with a synthetic guide field (discs of distinct sphere ids over a sky of misses: the timing
does not depend on the scene).  --warmup warm-up and --calls timed rounds, every round running all
points and their copies one after the other so that drift hits all alike.
  denoise   ort_last_denoise_ms: the pack pass and the iterations (HIP events on the call's stream)
  copy      one device-to-device copy that reads and writes the filter's compulsory bytes -- per
            pixel the pack pass's 32 B read (colour 12, hit 8, normal 12) and 32 B written (two
            16-byte records), then per iteration 32 B read (a colour and a guide record) and 16 B
            written, the last iteration 12 or 4 B in the caller's format: a copy of half that sum
            (it reads and writes each byte once), timed with events around it
The kernel in the tree is the direct form (each lane loads its 25 taps from global memory); the
LDS row-window form lost the alternating comparison recorded in profiles/denoise/forms.md and was
removed, so this tool times one form.
Context: config.h's default scene (100 spheres, seed 42, depth 3) and frame (800 x 600), 8 bounces:
the device time of a one-sample accumulation pass (ort_accum_last_pass_ms) beside the denoise of
that picture with the accumulation's guides.

Writes ab.md and ab.json into --out (default profiles/denoise); --bench-log appends the lines of a
file (the plain bench.py runs on this change and on its parent) to the .md.
usage: python tools/denoise_ab.py [--calls 50] [--warmup 5] [--out DIR]     (GPU)
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

SIZES = ((1280, 720), (3840, 2160))
ITERATIONS = (3, 5)
FORMATS = ("rgb32f", "rgba8")
W, H, SPHERES, SEED, DEPTH, BOUNCES = 800, 600, 100, 42, 3, 8


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def compulsory_bytes(pixels, iterations, fmt):
    """Bytes read plus bytes written per call (see the module text)."""
    last = 12 if fmt == "rgb32f" else 4
    return pixels * (32 + 32 + iterations * 32 + (iterations - 1) * 16 + last)


def guide_field(w, h, dev):
    """{t bits, sphere} records and normals: 40 discs of their own ids and normals over misses."""
    rng = np.random.default_rng(3)
    sphere = np.full((h, w), -1, np.int32)
    t = np.zeros((h, w), np.float32)
    nrm = np.zeros((h, w, 3), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(40):
        cx, cy, rad = rng.integers(0, w), rng.integers(0, h), rng.integers(h // 12, h // 4)
        m = (xx - cx) ** 2 + (yy - cy) ** 2 < rad * rad
        d = np.stack([(xx - cx) / rad, (yy - cy) / rad], axis=-1).astype(np.float32)
        z = np.sqrt(np.maximum(0.0, 1.0 - (d * d).sum(-1))).astype(np.float32)
        sphere[m], t[m] = k, (5.0 + k - z)[m]
        nrm[m] = np.concatenate([d, z[..., None]], axis=-1)[m]
    rec = np.ascontiguousarray(np.stack([t.view(np.int32), sphere], axis=-1))
    return torch.from_numpy(rec).to(dev), torch.from_numpy(nrm).to(dev), float((sphere >= 0).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise"))
    ap.add_argument("--bench-log", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "warmup": a.warmup, "kernel": "direct", "points": []}
    points = []
    with ort.Renderer(0) as r:
        for (w, h) in SIZES:
            img = torch.rand((h, w, 3), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            rec, nrm, share = guide_field(w, h, dev)
            for n_it in ITERATIONS:
                for fmt in FORMATS:
                    out = torch.empty((h, w, 3 if fmt == "rgb32f" else 4), dtype=torch.float32 if fmt == "rgb32f" else torch.uint8,
                                      device=dev)
                    half = compulsory_bytes(w * h, n_it, fmt) // 2
                    points.append(dict(w=w, h=h, iterations=n_it, format=fmt, img=img, rec=rec, nrm=nrm, out=out, share=share,
                                       src=torch.empty(half, dtype=torch.uint8, device=dev),
                                       dst=torch.empty(half, dtype=torch.uint8, device=dev), ms=[], copy=[]))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(a.warmup + a.calls):
            for q in points:
                r.denoise(q["img"], (q["rec"], q["nrm"]), iterations=q["iterations"], format=q["format"], out=q["out"])
                t_d = r.last_denoise_ms()
                e0.record()
                q["dst"].copy_(q["src"])
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    q["ms"].append(t_d)
                    q["copy"].append(e0.elapsed_time(e1))
        # the preview: a one-sample pass of the default frame, then its denoise
        s = ort.random_spheres(SPHERES, SEED)
        p = ort.FrameParams.default_camera(W, H, num_samples=1, max_depth=BOUNCES)
        r.build_scene(s, DEPTH, 0)
        pic = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        flt = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        pass_ms, den_ms = [], []
        with r.accumulate(p) as acc:
            g = acc.guides()
            torch.cuda.synchronize()
            for i in range(a.warmup + a.calls):
                acc.restart(p)
                acc.step(1, out=pic)
                t_p = acc.last_pass_ms()
                r.denoise(pic, g, out=flt)
                t_d = r.last_denoise_ms()
                if i >= a.warmup:
                    pass_ms.append(t_p)
                    den_ms.append(t_d)
            r.trace_camera(p, which="pixel_centre", normals=g[1], out=g[0])
            guides_ms = r.last_query_ms()
    lines = [f"ort_denoise (direct form: each lane loads its 25 taps from global memory), library defaults, device pointers, "
             f"{a.warmup} warm-up + {a.calls} timed rounds of all points in turn, one process, {res['device']}.",
             "denoise: ort_last_denoise_ms (pack pass + iterations).  copy: a device-to-device copy reading and writing the "
             "filter's compulsory bytes (half of them each way), events around it.", "",
             "| size | iterations | format | denoise ms median | p10-p90 | compulsory MB | copy ms median | p10-p90 | denoise / copy |",
             "|---|---|---|---|---|---|---|---|---|"]
    for q in points:
        d, c = pct(q["ms"], 0.5), pct(q["copy"], 0.5)
        mb = compulsory_bytes(q["w"] * q["h"], q["iterations"], q["format"]) / 1e6
        res["points"].append(dict(w=q["w"], h=q["h"], iterations=q["iterations"], format=q["format"], hit_share=q["share"],
                                  denoise_ms=dict(median=d, p10=pct(q["ms"], 0.1), p90=pct(q["ms"], 0.9)),
                                  copy_ms=dict(median=c, p10=pct(q["copy"], 0.1), p90=pct(q["copy"], 0.9)),
                                  compulsory_mb=mb, denoise_over_copy=d / c))
        lines.append(f"| {q['w']} x {q['h']} | {q['iterations']} | {q['format']} | {d:.4f} | {pct(q['ms'], 0.1):.4f}-{pct(q['ms'], 0.9):.4f} | "
                     f"{mb:.1f} | {c:.4f} | {pct(q['copy'], 0.1):.4f}-{pct(q['copy'], 0.9):.4f} | {d / c:.2f} |")
    res["preview"] = dict(frame=[W, H], bounces=BOUNCES, pass_ms=pct(pass_ms, 0.5), denoise_ms=pct(den_ms, 0.5), guides_ms=guides_ms)
    lines += ["", f"The preview at config.h's default frame ({W} x {H}, {SPHERES} spheres, {BOUNCES} bounces): one-sample accumulation "
              f"pass {pct(pass_ms, 0.5):.4f} ms (p10-p90 {pct(pass_ms, 0.1):.4f}-{pct(pass_ms, 0.9):.4f}), its denoise (3 iterations) "
              f"{pct(den_ms, 0.5):.4f} ms (p10-p90 {pct(den_ms, 0.1):.4f}-{pct(den_ms, 0.9):.4f}); the guides, traced once per camera, "
              f"{guides_ms:.4f} ms."]
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
