"""Raytracer's rest loop (setProgressiveMoments, readMoments, the variance-guided denoise overload)
through build/denoise_variance (tests/cpp/denoise_variance.cpp): passes of 1, 1, 2 and 4 samples of the
prebuilt scene with the moments kept, and from 2 samples on a variance-guided denoise with gamma -- each
filtered picture's hash against the Python path's on the same accumulation."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_denoise_cpp import fnv1a

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "build" / "denoise_variance"


def test_denoise_variance_binary_built():
    assert EXE.exists(), "make examples"


@pytest.mark.gpu
def test_the_rest_loop_prints_the_python_pictures(ort):
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = [l.split() for l in res.stdout.splitlines() if l.startswith("pass ")]
    assert [int(l[1]) for l in lines] == [2, 4, 8]
    s = ort.prebuilt_spheres()
    p = ort.FrameParams.default_camera(96, 64, num_samples=16, max_depth=8)
    with ort.Renderer(0) as r:
        r.upload(s, ort.build_octree(s, 3, 0))  # RaytracerConfig's maxDepth, maxSpheresPerNode
        with r.accumulate(p, moments=True) as acc:
            for n, line in zip((2, 2, 4), lines):
                acc.step(n, out=False)
                mean, var = acc.moments()
                out = r.denoise(mean, params=p, variance=var, sigma_variance=4.0, gamma=True)
                assert np.isfinite(out).all()
                assert int(line[3], 16) == fnv1a(np.ascontiguousarray(out).tobytes()), acc.done
                before, after = float(line[5]), float(line[6])
                print(f"{acc.done} samples: MSE against the 256-sample frame {before:.6f} -> {after:.6f}")
                assert 0.0 < after and 0.0 < before   # (the quality is tests/test_variance.py's, on the CPU)
