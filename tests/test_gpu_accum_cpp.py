"""Raytracer::renderProgressive (octreeraytracer_amd/csrc/raytracer.{h,cpp}) through
build/progressive (tests/cpp/progressive.cpp): the interactive loop's call against render()."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "build" / "progressive"


def test_progressive_binary_built():
    assert EXE.exists(), "make examples"


@pytest.mark.gpu
def test_render_progressive():
    """Same camera 3 x 2 samples of 6 ends as render()'s frame and samplesDone follows; a call on the
    finished frame writes it again; a camera that turned or zoomed in between starts the frame again."""
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    steps = {}
    for line in res.stdout.splitlines():
        f = line.split()
        if f and f[0] == "step":
            steps[f[1]] = tuple(int(x) for x in f[2:])  # (rc, samples done, equals render())
    print(steps)
    assert steps == {
        "a1": (0, 2, 0), "a2": (0, 4, 0), "a3": (0, 6, 1),  # 3 x 2 samples: previews, then render()'s frame
        "a4": (0, 6, 1),                                      # finished: the frame again
        "b1": (0, 2, 0),                                      # the camera turned: from sample 0
        "c1": (0, 2, 0),                                      # ... and back: again
        "d1": (0, 2, 0), "d2": (0, 4, 0), "d3": (0, 6, 1),  # the turned pose to its end (5 asked, 2 left)
        "e1": (0, 1, 0),                                      # another zoom: again
    }
