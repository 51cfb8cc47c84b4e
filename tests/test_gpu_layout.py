"""The device builder's compact layout (gpuCompactLayout in octreeraytracer_amd/csrc/gpu_build.hip:
k_compact_nodes, k_leaf_gather, k_fill_nan, k_planes) and what k_lds_image, k_interleave_nk and
k_leaf16 derive from it, against the host's (layout.cpp, held to its rules by tests/test_layout.py):
node, kid, leaf_sph, leaf_idx, planes, nk, leaf16 on every node, the LDS image and, at depth 9-10,
the reversed-table image, byte for byte, with depth, ordered and layout; first after
build_scene, then after an upload of the host tree into the same renderer.  The scenes are
tests/layout_cases.py's; the one with inverted boxes also renders a frame against the oracle."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

import layout_cases as cases
from octreeraytracer_amd import _lib as L


@pytest.mark.gpu
def test_gpu_built_layout_is_the_hosts():
    """The export hooks live in the analysis library, which a GPU process must not load beside
    libort.so (both carry the kernels): one process of its own, with the analysis library as its
    only one (tests/layout_cases.py run as a program)."""
    here = Path(__file__).resolve().parent
    env = dict(os.environ, ORT_LIB=str(L.ANALYSIS_LIB_PATH))
    res = subprocess.run([sys.executable, str(here / "layout_cases.py")], env=env, capture_output=True, text=True,
                         timeout=120)
    print(res.stdout, res.stderr[-2000:])
    assert res.returncode == 0, res.stdout + res.stderr[-2000:]
    assert "forms no scene reaches: none" in res.stdout
    for name in cases.SCENE_NAMES:
        line = [x for x in res.stdout.splitlines() if x.startswith(name + " ")]
        assert len(line) == 1 and line[0].endswith(": equal"), (name, line)
    assert "all equal: True" in res.stdout
