#!/usr/bin/env python3
"""What accumulating a frame in passes costs: the one-shot whole-pixel frame
without speculation (ort_last_kernel_ms) against the sum of ort_accum_last_pass_ms over the passes
of one frame -- 16 x 1, 4 x 4 and 1 x 16 samples, without and with a float picture per pass --
on config_default and stats114.  Median (min-max) of --reps repetitions after --warmup; every
accumulated frame is checked against the case's canonical SHA-256.  Prints one JSON line.
Run it on two builds alternately to compare their one-shot frames.
--moments times instead the passes of an accumulation that keeps luminance moments
(Renderer.accumulate(moments=True)) against the plain accumulation's, the two alternating repetition
by repetition in one process: 1 pass of N and N passes of 1, no picture; *_ratio is the median of the
per-repetition moments / plain ratios.
--adaptive times the passes of an adaptive accumulation (Renderer.accumulate(adaptive=True)):
(a) all traced (threshold 0) against the moments accumulation's, alternating as --moments does, 1 pass of N
and N passes of 1; (b) the rest loop -- one-sample passes at threshold 0.05, min_samples 4, floor 0.05 until
nothing is pending -- per pass the traced pixels, the pass's time and its time per traced sample relative to
the uniform one-sample moments passes', and the loop's total time and samples against the uniform frame's; then a pass that holds every pixel.
--moments-only times the moments accumulation alone (what a build from before --adaptive can run too: the
other side of a build-against-build comparison, process by process)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--cases", default="config_default,stats114")
    ap.add_argument("--moments", action="store_true", help="moments passes against plain passes (see above)")
    ap.add_argument("--adaptive", action="store_true", help="adaptive passes against moments passes (see above)")
    ap.add_argument("--moments-only", action="store_true", help="the moments accumulation's passes alone")
    a = ap.parse_args(argv)
    import torch

    import octreeraytracer_amd as ort
    from test_glsl_parity import CANON, frame_sha, inputs

    def summary(ms):
        return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]

    res = {}
    for name in a.cases.split(","):
        c = CANON["cases"][name]
        s, t, p = inputs(ort, c)
        dev = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda:0")
        with ort.Renderer(0) as r:
            r.upload(s, t)
            r.set_pixel_paths(1)
            r.set_pixel_speculate(0)
            if a.moments_only:
                n = p.num_samples
                for passes in (1, n):
                    split = [n // passes] * passes
                    tot = []
                    with r.accumulate(p, moments=True) as mom:
                        for i in range(a.warmup + a.reps):
                            mom.restart(p)
                            sm = 0.0
                            for k in split:
                                mom.step(k, out=False)
                                sm += mom.last_pass_ms()
                            if i >= a.warmup:
                                tot.append(sm)
                    res[f"{name}.accum_{passes}x{n // passes}_moments_ms"] = summary(tot)
                continue
            if a.adaptive:
                n = p.num_samples
                uniform_1 = None
                for passes in (1, n):  # (a) all traced against moments
                    split = [n // passes] * passes
                    tot = {False: [], True: []}
                    with r.accumulate(p, moments=True) as mom, r.accumulate(p, adaptive=True) as ada:
                        for i in range(a.warmup + a.reps):
                            for acc, key in ((mom, False), (ada, True)) if i % 2 == 0 else ((ada, True), (mom, False)):
                                acc.restart(p)
                                sm = 0.0
                                for k in split:
                                    if key:
                                        acc.step_adaptive(k, 0.0, 0, 0.05, out=False)
                                    else:
                                        acc.step(k, out=False)
                                    sm += acc.last_pass_ms()
                                if i >= a.warmup:
                                    tot[key].append(sm)
                        for acc in (mom, ada):
                            acc.step(1, out=dev)
                            torch.cuda.synchronize()
                            assert frame_sha(dev.cpu().numpy()) == c["sha256"], (name, split)
                    tag = f"{name}.accum_{passes}x{n // passes}"
                    res[f"{tag}_moments_ms"] = summary(tot[False])
                    res[f"{tag}_adaptive_ms"] = summary(tot[True])
                    res[f"{tag}_ratio"] = summary([m / q for m, q in zip(tot[True], tot[False])])
                    if passes == n:
                        uniform_1 = statistics.median(tot[False]) / n  # a uniform one-sample pass
                crit = (0.05, 4, 0.05)  # (b) the rest loop
                pixels = p.width * p.height
                per_pass, totals, traced, samples = {}, [], [], 0
                with r.accumulate(p, adaptive=True) as ada:
                    for i in range(a.warmup + a.reps):
                        ada.restart(p)
                        traced, sm, k = [], 0.0, 0
                        while True:
                            pending = ada.adaptive_stats(*crit)["pending"]
                            if not pending:
                                break
                            traced.append(pending)
                            ada.step_adaptive(1, *crit, out=False)
                            ms = ada.last_pass_ms()
                            sm += ms
                            if i >= a.warmup:
                                per_pass.setdefault(k, []).append(ms)
                            k += 1
                        if i >= a.warmup:
                            totals.append(sm)
                    samples = ada.adaptive_stats(*crit)["samples"]
                    held = []  # a pass that holds every pixel (threshold +inf): what the skip alone costs
                    for i in range(a.warmup + a.reps):
                        ada.step_adaptive(1, float("inf"), 0, 0.05, out=False)
                        if i >= a.warmup:
                            held.append(ada.last_pass_ms())
                    assert ada.adaptive_stats(*crit)["samples"] == samples
                res[f"{name}.all_held_pass_ms"] = summary(held)
                res[f"{name}.uniform_pass_ms"] = round(uniform_1, 4)
                res[f"{name}.rest_loop"] = [
                    {"pass": k, "traced": traced[k], "ms": summary(per_pass[k]),
                     "per_sample_vs_uniform": round(statistics.median(per_pass[k]) / traced[k] / (uniform_1 / pixels), 3)}
                    for k in range(len(traced))]
                res[f"{name}.rest_loop_total_ms"] = summary(totals)
                res[f"{name}.rest_loop_samples"] = [samples, n * pixels]
                res[f"{name}.rest_loop_vs_uniform"] = {"time": round(statistics.median(totals) / (uniform_1 * n), 3),
                                                       "samples": round(samples / (n * pixels), 3)}
                continue
            if a.moments:
                n = p.num_samples
                for passes in (1, n):
                    split = [n // passes] * passes
                    tot = {False: [], True: []}
                    with r.accumulate(p) as plain, r.accumulate(p, moments=True) as mom:
                        for i in range(a.warmup + a.reps):
                            for acc, key in ((plain, False), (mom, True)) if i % 2 == 0 else ((mom, True), (plain, False)):
                                acc.restart(p)
                                sm = 0.0
                                for k in split:
                                    acc.step(k, out=False)
                                    sm += acc.last_pass_ms()
                                if i >= a.warmup:
                                    tot[key].append(sm)
                        for acc in (plain, mom):
                            acc.step(1, out=dev)
                            torch.cuda.synchronize()
                            assert frame_sha(dev.cpu().numpy()) == c["sha256"], (name, split)
                    tag = f"{name}.accum_{passes}x{n // passes}"
                    res[f"{tag}_plain_ms"] = summary(tot[False])
                    res[f"{tag}_moments_ms"] = summary(tot[True])
                    res[f"{tag}_ratio"] = summary([m / q for m, q in zip(tot[True], tot[False])])
                continue
            ms = []
            for i in range(a.warmup + a.reps):
                r.render(p, out=dev)
                if i >= a.warmup:
                    ms.append(r.last_kernel_ms())
            torch.cuda.synchronize()
            assert frame_sha(dev.cpu().numpy()) == c["sha256"], name
            res[f"{name}.oneshot_ms"] = summary(ms)
            n = p.num_samples
            for passes in (n, 4, 1):
                split = [n // passes] * passes
                for pic in (False, True):
                    tot = []
                    with r.accumulate(p) as acc:
                        for i in range(a.warmup + a.reps):
                            acc.restart(p)
                            sm = 0.0
                            for k in split:
                                acc.step(k, out=dev if pic else False)
                                sm += acc.last_pass_ms()
                            if i >= a.warmup:
                                tot.append(sm)
                        acc.step(1, out=dev)  # finished: the frame from the stored sums
                        torch.cuda.synchronize()
                        assert frame_sha(dev.cpu().numpy()) == c["sha256"], (name, split)
                    res[f"{name}.accum_{passes}x{n // passes}_{'pic' if pic else 'nopic'}_ms"] = summary(tot)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
