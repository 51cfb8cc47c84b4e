"""Raytracer::denoise (octreeraytracer_amd/csrc/raytracer.{h,cpp}) through build/denoise
(tests/cpp/denoise.cpp): one accumulated sample of the prebuilt scene, denoised -- the picture's hash
against Renderer.denoise on the same frame, and the error against the 64-sample frame going down."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "build" / "denoise"


def fnv1a(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_denoise_binary_built():
    assert EXE.exists(), "make examples"


@pytest.mark.gpu
def test_denoise_prints_the_python_picture_and_a_smaller_error(ort):
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = {l.split()[0]: l.split()[1:] for l in res.stdout.splitlines() if l.strip()}
    s = ort.prebuilt_spheres()
    p = ort.FrameParams.default_camera(96, 64, num_samples=1, max_depth=8)
    with ort.Renderer(0) as r:
        r.upload(s, ort.build_octree(s, 3, 0))  # RaytracerConfig's maxDepth, maxSpheresPerNode
        with r.accumulate(p) as acc:
            noisy = acc.step(1)
        out = r.denoise(noisy, params=p)
    assert int(lines["hash"][0], 16) == fnv1a(np.ascontiguousarray(out).tobytes())
    before, after = (float(v) for v in lines["mse"])
    print(f"MSE against the 64-sample frame: {before:.6f} -> {after:.6f}")
    assert np.isfinite(out).all() and 0.0 < after < before
