"""The depth <= 8 camera kernels' pop (fast_pop reading the LDS image's pop table) on the GPU:
the cases of tests/pop_table_cases.py -- trees of depth 1, 2, 3, 5 and 8 seen from inside the
field along the eight diagonals, which tests/test_pop_table.py shows pop every table entry under
every direction-sign mask -- through ort_render, bit for bit against the oracle: with one tile per
workgroup, with tile pairs forced, and at 1 sample x 3 bounces through the per-bounce pipeline
(the camera kernel that shades bounce 0 itself).  Two frames of each: the second is dealt to the
waves by the first one's walk costs.  And one frame on the benchmark's 100k-sphere depth-8 tree,
built on the GPU, against the host emulation."""
import numpy as np
import pytest

import pop_table_cases as cases
from octreeraytracer_amd.renderer import emulate_render_host

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
def test_c3_tree_frame_is_the_host_walks(ort):
    s = ort.random_spheres(100_000, 42)
    t = ort.build_octree(s, 8, 0)
    p = ort.FrameParams.default_camera(256, 144)
    ref, _ = emulate_render_host(s, t, p)
    with ort.Renderer(0) as r:
        r.build_scene(s, 8, 0)
        for frame in (1, 2):
            img = r.render(p)
            assert cases.same_bits(img, ref), (frame, int((img != ref).any(axis=2).sum()))
    assert float(np.asarray(ref).std()) > 0.01  # (a frame with spheres in it, not sky alone)
