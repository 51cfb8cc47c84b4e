"""A sphere shared by sibling leaves tested once per node (leaf_kids under Masks64::kLeafDedup, the
records of k_cam_node) on the GPU: the device-built cam_node against the host's on the hand-made
grouping tree and the seeded depth-6 tree; ort_render frames of 2,000 spheres at depth 6 and depth 8
against the host emulation, bit for bit -- frame 1 and the cost-ordered frame 2, one tile per
workgroup and tile pairs, the uploaded tree and the GPU-built one; the big-sphere scene, whose
host walk is shown to drop children (tests/test_leaf_dedup.py), against the oracle; and trace_camera
against its host emulation."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pop_table_cases as cases
from leaf_dedup_cases import big_scene, seeded_scene
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import camera_query_host, emulate_render_host


@pytest.mark.gpu
def test_gpu_built_records_are_the_host_derived_ones():
    """The export hook lives in the analysis library, which a GPU process must not load beside
    libort.so (both carry the kernels): a process of its own, with the analysis library as its
    only one (tests/leaf_dedup_cases.py)."""
    here = Path(__file__).resolve().parent
    env = dict(os.environ, ORT_LIB=str(L.ANALYSIS_LIB_PATH))
    res = subprocess.run([sys.executable, str(here / "leaf_dedup_cases.py")], env=env, capture_output=True, text=True,
                         timeout=120)
    print(res.stdout, res.stderr[-2000:])
    assert res.returncode == 0, res.stdout + res.stderr[-2000:]
    assert "cam_node all equal: True" in res.stdout


@pytest.fixture(scope="module")
def host_frames(ort):
    """depth -> (spheres, tree, params, the host emulation's 128 x 96 frame), computed once."""
    out = {}
    for depth in (6, 8):
        s, t = seeded_scene(depth)
        p = ort.FrameParams.default_camera(128, 96)
        ref = emulate_render_host(s, t, p)[0]
        ref.flags.writeable = False
        out[depth] = (s, t, p, ref)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("route", ("uploaded", "built"))
@pytest.mark.parametrize("pairs", (0, 1), ids=("one_tile", "tile_pairs"))
@pytest.mark.parametrize("depth", (6, 8))
def test_frames_are_the_host_emulations(ort, host_frames, depth, pairs, route):
    s, t, p, ref = host_frames[depth]
    with ort.Renderer(0) as r:
        r.set_tile_pairs(pairs)
        if route == "uploaded":
            r.upload(s, t)
        else:
            r.build_scene(s, depth, 0)
        assert r.info()["layout"] == "compact"
        assert r.info()["device_bytes"] >= 24 * t.n_nodes  # leaf16 and cam_node are counted with the scene
        for frame in (1, 2):  # frame 2 is cost-ordered
            img = r.render(p)
            assert cases.same_bits(img, ref), (depth, pairs, route, frame, int((img != ref).any(axis=2).sum()))
    assert len(np.unique(np.asarray(ref).reshape(-1, 3), axis=0)) > 100  # (spheres and sky, not one colour)


@pytest.mark.gpu
def test_big_sphere_frames_are_the_oracles(ort, oracle):
    s, t = big_scene()
    with ort.Renderer(0) as r:
        r.upload(s, t)
        for diag in cases.DIAGONALS:
            p = cases.pose(ort, (64, 64), diag)
            ref = oracle.render(s, t, p)
            for frame in (1, 2):
                assert cases.same_bits(r.render(p), ref), (diag, frame)


@pytest.mark.gpu
def test_trace_camera_is_the_host_emulations(ort):
    s, t = seeded_scene()
    p = ort.FrameParams.default_camera(64, 48)
    _, tt, sph = camera_query_host(s, t, p)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        got_t, got_sph = r.trace_camera(p)
    assert cases.same_bits(got_t, tt) and np.array_equal(got_sph, sph)
    assert (sph >= 0).sum() > 100  # (rays that hit spheres, not sky alone)
