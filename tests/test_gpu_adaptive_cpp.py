"""Raytracer's adaptive rest loop (setProgressiveAdaptive, pendingPixels, readSampleCounts, readMoments)
through build/adaptive (tests/cpp/adaptive.cpp): one-sample adaptive passes of the prebuilt scene until no
pixel is pending -- the pending pixels of every pass, and the hashes of the final counts, mean, variance
and preview, against the Python path's on the same accumulation, bit for bit."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_denoise_cpp import fnv1a

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "build" / "adaptive"


def test_adaptive_binary_built():
    assert EXE.exists(), "make examples"


@pytest.mark.gpu
def test_the_rest_loop_is_the_python_paths(ort):
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    passes = [l.split() for l in res.stdout.splitlines() if l.startswith("pass ")]
    end = [l.split() for l in res.stdout.splitlines() if l.startswith("end ")]
    assert len(end) == 1 and 4 <= len(passes) <= 16 and int(end[0][2]) == len(passes)
    s = ort.prebuilt_spheres()
    p = ort.FrameParams.default_camera(96, 64, num_samples=16, max_depth=8)
    crit = dict(threshold=0.05, min_samples=4, luminance_floor=0.05)
    with ort.Renderer(0) as r:
        r.upload(s, ort.build_octree(s, 3, 0))  # RaytracerConfig's maxDepth, maxSpheresPerNode
        with r.accumulate(p, adaptive=True) as acc:
            pic = None
            for i, line in enumerate(passes):
                pending = acc.adaptive_stats(**crit)["pending"]
                assert (int(line[1]), int(line[3])) == (i, pending) and pending > 0
                pic = acc.step_adaptive(1, **crit)
                assert int(line[5]) == acc.done
            st = acc.adaptive_stats(**crit)
            assert st["pending"] == 0 and st["samples"] == int(end[0][4]) < 16 * 96 * 64
            counts, (mean, var) = acc.counts(), acc.moments()
            assert counts.min() >= 4 and len(np.unique(counts)) >= 4
            got = {end[0][k]: int(end[0][k + 1], 16) for k in (5, 7, 9, 11)}
            assert got == {"counts": fnv1a(counts.tobytes()), "mean": fnv1a(mean.tobytes()), "variance": fnv1a(var.tobytes()),
                           "preview": fnv1a(pic.tobytes())}
            print(f"{len(passes)} passes, {st['samples']} of {16 * 96 * 64} samples, counts {counts.min()}..{counts.max()}")
