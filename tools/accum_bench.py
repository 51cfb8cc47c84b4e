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
per-repetition moments / plain ratios."""
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
