"""Raytracer::setHistoryMotion and moveSpheres (octreeraytracer_amd/csrc/raytracer.{h,cpp}) through
build/reproject_motion (tests/cpp/reproject_motion.cpp): three spheres of the prebuilt scene moved over
four steps under a resting camera, the scene replaced and a one-sample linear picture blended into the
history at each -- the hashes of the integrated colour and variance against History.update(motion=True)
on the same scenes and pictures, and the error against the 64-sample mean going down."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_denoise_cpp import fnv1a

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "build" / "reproject_motion"
F = np.float32


def test_reproject_motion_binary_built():
    assert EXE.exists(), "make examples"


def placed(ort, base, k):
    """tests/cpp/reproject_motion.cpp's placed(): one float32 operation each."""
    cr = np.array(base.center_radius, F)
    cr[80, 0] = cr[80, 0] + F(0.1) * F(k)
    cr[81, 3] = cr[81, 3] * (F(1.0) + F(0.02) * F(k))
    cr[82, 1] = cr[82, 1] + F(0.05) * F(k)
    return ort.SphereSet(cr, base.mat_albedo, base.fuzz_ri)


@pytest.mark.gpu
def test_reproject_motion_prints_the_python_records_and_a_smaller_error(ort):
    from octreeraytracer_amd.scene import DEFAULT_PITCH, DEFAULT_YAW
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = [l.split() for l in res.stdout.splitlines() if l.strip()]
    hashes = {int(l[1]): int(l[3], 16) for l in lines if l[0] == "step"}
    base = ort.prebuilt_spheres()
    p = ort.FrameParams.default_camera(96, 64, num_samples=1, max_depth=8, position=(0.0, 2.5, -10.0), yaw=DEFAULT_YAW,
                                       pitch=DEFAULT_PITCH, zoom=45.0)
    with ort.Renderer(0) as r, r.history(96, 64) as hist:
        for k in range(4):
            s = placed(ort, base, k)
            r.upload(s, ort.build_octree(s, 3, 0))  # RaytracerConfig's maxDepth, maxSpheresPerNode
            with r.accumulate(p, moments=True) as acc:
                acc.step(1)
                sample = acc.moments(variance=False)
            col, var, ln = hist.update(np.ascontiguousarray(sample), p, length=True, motion=True)
            assert hist.info()["updates"] == k + 1 and ln.max() == k + 1
            assert hashes[k] == fnv1a(np.ascontiguousarray(col).tobytes() + np.ascontiguousarray(var).tobytes()), k
    before, after = (float(v) for v in next(l for l in lines if l[0] == "mse")[1:])
    print(f"MSE against the 64-sample mean: {before:.6f} -> {after:.6f}")
    assert 0.0 < after < before
