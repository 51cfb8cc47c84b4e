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
--variance adds, at every point and in the same rounds, ort_denoise_ex with a seeded
variance plane (the variance-guided term on, sigma_variance at its default) right after the plain
ort_denoise, the ratio of the two per round, and the rest loop at config.h's default frame: a
one-sample moments pass, ort_accum_read_moments and the variance-guided denoise with gamma of its
mean, beside the plain pass and the plain denoise of its picture.  The variance plane is 4 B a pixel
beside the records: 4 B more read by the pack pass and 4 B written, then 4 B read and 4 B written per
iteration but the last, which only reads.  Write it somewhere else: --out profiles/variance.
usage: python tools/denoise_ab.py [--calls 50] [--warmup 5] [--out DIR] [--variance]     (GPU)
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


def variance_bytes(pixels, iterations):
    """The bytes the variance plane adds to compulsory_bytes (see the module text)."""
    return pixels * (4 + 4 + iterations * 4 + (iterations - 1) * 4)


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
    ap.add_argument("--variance", action="store_true", help="also ort_denoise_ex with a variance plane, and the rest loop")
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
                                       dst=torch.empty(half, dtype=torch.uint8, device=dev), ms=[], copy=[], vms=[],
                                       var=torch.rand((h, w), dtype=torch.float32, device=dev,
                                                      generator=torch.Generator(device=dev).manual_seed(2)) * 0.05))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(a.warmup + a.calls):
            for q in points:
                r.denoise(q["img"], (q["rec"], q["nrm"]), iterations=q["iterations"], format=q["format"], out=q["out"])
                t_d = r.last_denoise_ms()
                if a.variance:
                    r.denoise(q["img"], (q["rec"], q["nrm"]), iterations=q["iterations"], format=q["format"], out=q["out"],
                              variance=q["var"])
                    if i >= a.warmup:
                        q["vms"].append(r.last_denoise_ms())
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
    rest = None
    if a.variance:  # the rest loop: moments pass, read, variance-guided denoise; beside the plain pass and denoise
        with ort.Renderer(0) as r:
            r.build_scene(s, DEPTH, 0)
            p16 = ort.FrameParams.default_camera(W, H, num_samples=16, max_depth=BOUNCES)
            mean = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
            var = torch.empty((H, W), dtype=torch.float32, device=dev)
            ts = torch.cuda.Stream(device=dev)
            t = dict(plain_pass=[], moments_pass=[], read=[], plain_denoise=[], var_denoise=[])
            with r.accumulate(p16) as plain, r.accumulate(p16, moments=True) as mom:
                g = mom.guides()
                torch.cuda.synchronize()
                for i in range(a.warmup + a.calls):
                    row = {}
                    for acc, key in ((plain, "plain_pass"), (mom, "moments_pass")) if i % 2 == 0 else ((mom, "moments_pass"), (plain, "plain_pass")):
                        acc.restart(p16)
                        acc.step(1, out=False)
                        acc.step(1, out=pic)           # the second one-sample pass: a variance exists after it
                        row[key] = acc.last_pass_ms()
                    torch.cuda.synchronize()
                    e0.record(ts)
                    mom.moments(out_mean=mean, out_variance=var, stream=ts.cuda_stream)
                    e1.record(ts)
                    e1.synchronize()
                    row["read"] = e0.elapsed_time(e1)
                    r.denoise(pic, g, out=flt)
                    row["plain_denoise"] = r.last_denoise_ms()
                    r.denoise(mean, g, out=flt, variance=var, gamma=True)
                    row["var_denoise"] = r.last_denoise_ms()
                    if i >= a.warmup:
                        for k, v in row.items():
                            t[k].append(v)
            rest = {k: dict(median=pct(v, 0.5), p10=pct(v, 0.1), p90=pct(v, 0.9)) for k, v in t.items()}
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
    if a.variance:
        lines += ["", "ort_denoise_ex with a variance plane (the variance-guided term on) right after ort_denoise, every round:", "",
                  "| size | iterations | format | plain ms median | with variance ms median | p10-p90 | ratio median (p10-p90) | "
                  "B / pixel / iteration plain -> with variance | with variance / copy of its bytes |", "|---|---|---|---|---|---|---|---|---|"]
        res["variance_points"] = []
        for q in points:
            d, v = pct(q["ms"], 0.5), pct(q["vms"], 0.5)
            ratios = [x / y for x, y in zip(q["vms"], q["ms"])]
            px = q["w"] * q["h"]
            b0 = compulsory_bytes(px, q["iterations"], q["format"])
            b1 = b0 + variance_bytes(px, q["iterations"])
            c = pct(q["copy"], 0.5) * b1 / b0   # the measured copy scaled to the larger byte count
            res["variance_points"].append(dict(w=q["w"], h=q["h"], iterations=q["iterations"], format=q["format"], plain_ms=d,
                                               variance_ms=dict(median=v, p10=pct(q["vms"], 0.1), p90=pct(q["vms"], 0.9)),
                                               ratio=dict(median=pct(ratios, 0.5), p10=pct(ratios, 0.1), p90=pct(ratios, 0.9)),
                                               bytes_per_pixel_iteration=[b0 / px / q["iterations"], b1 / px / q["iterations"]],
                                               variance_over_scaled_copy=v / c))
            lines.append(f"| {q['w']} x {q['h']} | {q['iterations']} | {q['format']} | {d:.4f} | {v:.4f} | {pct(q['vms'], 0.1):.4f}-"
                         f"{pct(q['vms'], 0.9):.4f} | {pct(ratios, 0.5):.3f} ({pct(ratios, 0.1):.3f}-{pct(ratios, 0.9):.3f}) | "
                         f"{b0 / px / q['iterations']:.1f} -> {b1 / px / q['iterations']:.1f} | {v / c:.2f} |")
        res["rest_loop"] = dict(frame=[W, H], bounces=BOUNCES, **rest)
        lines += ["", f"The rest loop at config.h's default frame ({W} x {H}, {SPHERES} spheres, {BOUNCES} bounces, 16-sample target), "
                  "second one-sample pass, ms median (p10-p90):", ""]
        for k, label in (("plain_pass", "plain pass"), ("moments_pass", "moments pass"), ("read", "ort_accum_read_moments (mean and variance, device)"),
                         ("plain_denoise", "ort_denoise of the picture"), ("var_denoise", "ort_denoise_ex of the mean: variance, gamma")):
            lines.append(f"- {label}: {rest[k]['median']:.4f} ({rest[k]['p10']:.4f}-{rest[k]['p90']:.4f})")
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
