"""The depth <= 8 camera kernels' child test from twelve order bits and two order tables in device
memory (child_order_keep, Masks64::kOrderBits) on the GPU: trees of depth 1, 3 and 8 of
tests/pop_table_cases.py, seen along the eight diagonals at 16x16 and 40x24, through
ort_trace_compact (one tile per workgroup) and ort_trace_pair (tile pairs forced), first and second
frame (the second is dealt to the waves by the first one's walk costs), RGB32F, bit for bit
against the oracle; and the two tables as the device holds them against the host's."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

import pop_table_cases as cases
from octreeraytracer_amd import _lib as L

DEPTHS = (1, 3, 8)
SIZES = ((16, 16), (40, 24))


@pytest.mark.gpu
@pytest.mark.parametrize("pairs", (0, 1), ids=("trace_compact", "trace_pair"))
def test_camera_frames_are_the_oracles(ort, pairs):
    with ort.Renderer(0) as r:
        r.set_tile_pairs(pairs)
        for depth in DEPTHS:
            for m in (0, 1):
                s, t = cases.scene(depth, m)
                r.upload(s, t)
                assert r.info()["layout"] == "compact"
                for size in SIZES:
                    for diag in cases.DIAGONALS:
                        p = cases.pose(ort, size, diag)
                        ref = cases.reference(depth, m, size, diag)
                        for frame in (1, 2):
                            img = r.render(p)
                            assert cases.same_bits(img, ref), (pairs, depth, m, size, diag, frame,
                                                               int((img != ref).any(axis=2).sum()))


@pytest.mark.gpu
def test_device_tables_are_the_hosts():
    """In a process of its own, with the analysis library as its only one (tests/child_order_image.py)."""
    here = Path(__file__).resolve().parent
    env = dict(os.environ, ORT_LIB=str(L.ANALYSIS_LIB_PATH))
    res = subprocess.run([sys.executable, str(here / "child_order_image.py")], env=env, capture_output=True, text=True,
                         timeout=120)
    print(res.stdout, res.stderr[-2000:])
    assert res.returncode == 0, res.stdout + res.stderr[-2000:]
    assert res.stdout.count(": equal") == 2 and "all equal: True" in res.stdout
