#!/usr/bin/env python3
"""What accumulating a frame in passes costs: the one-shot whole-pixel frame
without speculation (ort_last_kernel_ms) against the sum of ort_accum_last_pass_ms over the passes
of one frame -- 16 x 1, 4 x 4 and 1 x 16 samples, without and with a float picture per pass --
on config_default and stats114.  Median (min-max) of --reps repetitions after --warmup; every
accumulated frame is checked against the case's canonical SHA-256.  Prints one JSON line.
Run it on two builds alternately to compare their one-shot frames."""
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
