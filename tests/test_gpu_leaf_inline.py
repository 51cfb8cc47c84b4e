"""The depth <= 8 camera kernels' inline leaf children reading the 16-byte leaf records
(leaf_kids under Masks64::kLeafInline, the records of k_leaf16) on the GPU: the scenes of
tests/pop_table_cases.py -- trees of depth 1 (list-form leaves only), 2, 3, 5 (both forms, both
reached: tests/test_leaf_inline.py) and 8 (inline-form only) -- through ort_render, bit for bit
against the oracle: one tile per workgroup, tile pairs forced, and 1 sample x 3 bounces through
the per-bounce pipeline; two frames of each (the second is cost-ordered).  trace_camera on a mixed
scene against its host emulation; one frame of the benchmark's 100k-sphere depth-8 tree, built on
the GPU, against the host walk; and that scene's device records against the host-derived ones."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pop_table_cases as cases
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import camera_query_host, emulate_render_host
from test_emulation import extreme_root_scene

# name -> (tile pairs, samples, bounces)
MODES = {"one_tile": (0, 1, 1), "tile_pairs": (1, 1, 1), "pipeline_3_bounces": (0, 1, 3)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_camera_kernels_are_the_oracles(ort, mode):
    pairs, samples, bounces = MODES[mode]
    with ort.Renderer(0) as r:
        r.set_tile_pairs(pairs)
        r.set_pixel_paths(0)  # bounces > 1: the per-bounce pipeline, not whole-pixel paths
        for depth in cases.DEPTHS:
            for m in (0, 1):
                s, t = cases.scene(depth, m)
                r.upload(s, t)
                assert r.info()["layout"] == "compact"
                for size in cases.SIZES:
                    for diag in cases.DIAGONALS:
                        p = cases.pose(ort, size, diag, samples, bounces)
                        ref = cases.reference(depth, m, size, diag, samples, bounces)
                        for frame in (1, 2):
                            img = r.render(p)
                            assert cases.same_bits(img, ref), (mode, depth, m, size, diag, frame,
                                                               int((img != ref).any(axis=2).sum()))


@pytest.mark.gpu
def test_extreme_radii_on_the_gpu(ort, oracle):
    """r^2 huge (1e36, 1e38) in inline records, 4 bounces through the per-bounce pipeline."""
    s = extreme_root_scene(ort)
    t = ort.build_octree(s, 5, 0)
    p = ort.FrameParams.default_camera(64, 40, max_depth=4)
    ref = oracle.render(s, t, p)
    with ort.Renderer(0) as r:
        r.set_pixel_paths(0)
        r.upload(s, t)
        for frame in (1, 2):
            assert cases.same_bits(r.render(p), ref), frame


@pytest.mark.gpu
def test_trace_camera_is_the_host_emulations(ort):
    s, t = cases.scene(5, 0)  # both record forms
    p = cases.pose(ort, (48, 32), cases.DIAGONALS[3])
    _, tt, sph = camera_query_host(s, t, p)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        got_t, got_sph = r.trace_camera(p)
    assert cases.same_bits(got_t, tt) and np.array_equal(got_sph, sph)
    assert (sph >= 0).sum() > 100  # (rays that hit spheres, not sky alone)


@pytest.mark.gpu
def test_c3_tree_frame_is_the_host_walks(ort):
    s = ort.random_spheres(100_000, 42)
    t = ort.build_octree(s, 8, 0)
    p = ort.FrameParams.default_camera(256, 144)
    ref, _ = emulate_render_host(s, t, p)
    with ort.Renderer(0) as r:
        r.build_scene(s, 8, 0)
        before = r.info()["device_bytes"]
        for frame in (1, 2):
            img = r.render(p)
            assert cases.same_bits(img, ref), (frame, int((img != ref).any(axis=2).sum()))
        assert before >= 16 * t.n_nodes  # the records are counted with the scene's memory
    assert float(np.asarray(ref).std()) > 0.01  # (a frame with spheres in it, not sky alone)


@pytest.mark.gpu
def test_gpu_built_records_are_the_host_derived_ones():
    """The export hook lives in the analysis library, which a GPU process must not load beside
    libort.so (both carry the kernels): a process of its own, with the analysis library as its
    only one (tests/leaf_inline_cases.py)."""
    here = Path(__file__).resolve().parent
    env = dict(os.environ, ORT_LIB=str(L.ANALYSIS_LIB_PATH))
    res = subprocess.run([sys.executable, str(here / "leaf_inline_cases.py")], env=env, capture_output=True, text=True,
                         timeout=120)
    print(res.stdout, res.stderr[-2000:])
    assert res.returncode == 0, res.stdout + res.stderr[-2000:]
    assert "equal on leaves: True" in res.stdout
