"""Raytracer::reproject (octreeraytracer_amd/csrc/raytracer.{h,cpp}) through build/reproject
(tests/cpp/reproject.cpp): a camera moved over four poses of the prebuilt scene, a one-sample linear
picture blended into the history at each -- the hashes of the integrated colour and variance against
History.update on the same pictures, and the error against the 64-sample mean going down."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_denoise_cpp import fnv1a

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "build" / "reproject"
POSES = ((0.0, 0.0, 45.0), (0.05, 0.0, 45.0), (0.05, 2.0, 47.0), (0.1, 2.0, 47.0))   # x offset, yaw offset, zoom


def test_reproject_binary_built():
    assert EXE.exists(), "make examples"


@pytest.mark.gpu
def test_reproject_prints_the_python_records_and_a_smaller_error(ort):
    from octreeraytracer_amd.scene import DEFAULT_PITCH, DEFAULT_YAW
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = [l.split() for l in res.stdout.splitlines() if l.strip()]
    hashes = {int(l[1]): int(l[3], 16) for l in lines if l[0] == "pose"}
    s = ort.prebuilt_spheres()
    with ort.Renderer(0) as r:
        r.upload(s, ort.build_octree(s, 3, 0))  # RaytracerConfig's maxDepth, maxSpheresPerNode
        with r.history(96, 64) as hist:
            for k, (dx, dyaw, zoom) in enumerate(POSES):
                p = ort.FrameParams.default_camera(96, 64, num_samples=1, max_depth=8, position=(0.0 + dx, 2.5, -10.0),
                                                   yaw=DEFAULT_YAW + dyaw, pitch=DEFAULT_PITCH, zoom=zoom)
                with r.accumulate(p, moments=True) as acc:
                    acc.step(1)
                    sample = acc.moments(variance=False)
                col, var = hist.update(np.ascontiguousarray(sample), p)
                assert hashes[k] == fnv1a(np.ascontiguousarray(col).tobytes() + np.ascontiguousarray(var).tobytes()), k
    before, after = (float(v) for v in next(l for l in lines if l[0] == "mse")[1:])
    print(f"MSE against the 64-sample mean: {before:.6f} -> {after:.6f}")
    assert 0.0 < after < before
