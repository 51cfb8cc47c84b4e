"""Frames after a shape's first, pinned to the REFERENCE'S OWN shaders.

tests/test_gpu_parity.py renders each case of tests/golden/glsl/canonical.json once, on a fresh
upload: always the whole-chain launch of ort_pixel_paths.  The reference itself draws one static
pose frame after frame, and here every whole-pixel frame after the first takes another route
(render_pixel_paths): it reads the heavy-first class lists the frame before wrote, and with 5 or
more samples (spec_nch > 1: chunks of at least 4 samples, more than one chunk) it speculates --
the samples traced in parallel from last frame's RNG end states, a resolve, a fixup list: three
launches.  These tests render the canonical poses repeatedly on one context and require the
reference shader's SHA-256 of every frame; a camera that turns away and comes back; and a scene
swapped for another of equal counts, which the frame signature cannot tell apart."""
import dataclasses

import numpy as np
import pytest

from test_glsl_parity import CANON, frame_sha, inputs
from test_gpu_build import same_tree
from test_gpu_parity import assert_same, pixel_paths

SPECULATING = ["config_default", "stats114"]  # 16 samples: 4 chunks of 4
# 2 to 4 samples: one chunk, never speculated; their later frames differ by heavy-first order only
ONE_CHUNK = ["ms0_row68", "prebuilt_spp4_d8", "c2_full_spp4_d8", "c3tree_spp3_b5", "deep_d9_m1_spp2_b3"]


def launches(r):
    return r.frame_trace_times_ms(1)[0][1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SPECULATING + ONE_CHUNK)
def test_repeated_frames_are_the_reference_shaders(ort, name):
    c = CANON["cases"][name]
    assert (c["spp"] >= 5) == (name in SPECULATING)
    s, t, p = inputs(ort, c)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_pixel_paths(1)  # (auto would take the pipeline on the C3 and depth-9 trees)
        if name in SPECULATING:
            r.set_pixel_speculate(1)
        seen = []
        for k in range(5):
            img = r.render(p)
            seen.append(launches(r))
            assert frame_sha(img) == c["sha256"], f"{name}: frame {k + 1} is not the reference shader's"
        print(f"{name}: launches per frame {seen}")
        assert seen == ([1, 3, 3, 3, 3] if name in SPECULATING else [1] * 5), (name, seen)
    if name not in SPECULATING:
        return
    # auto: the choice rests on event timings, so either count is right on any frame but the first
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_pixel_paths(1)
        r.set_pixel_speculate(-1)
        seen = []
        for k in range(8):
            img = r.render(p)
            seen.append(launches(r))
            assert frame_sha(img) == c["sha256"], f"{name}: auto frame {k + 1} is not the reference shader's"
        print(f"{name}: auto, launches per frame {seen}")
        assert seen[0] == 1 and all(n in (1, 3) for n in seen), (name, seen)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SPECULATING)
def test_turn_and_return_is_the_reference_shaders(ort, name):
    """The canonical pose twice, three frames of a camera turning by half a degree each (their
    pixels are tests/test_gpu_parity.py test_pixel_speculate's business), the canonical pose four
    times: the fall-back while pixels move, the moved count, and speculation taken up again from
    states a fall-back frame recorded.  By the last two frames the frame before found no moved
    pixel (ort_sample_decide speculates once moved x 1000 <= pixels): three launches.  (A frame
    that falls back on the device's decision is three launches too -- every pixel on the fixup
    list -- so the counts here show the route the host took, the hashes what came of it.)"""
    from octreeraytracer_amd.scene import DEFAULT_PITCH, DEFAULT_YAW, camera_view
    c = CANON["cases"][name]
    s, t, p = inputs(ort, c)
    yaw, pitch = DEFAULT_YAW + c["dyaw"], DEFAULT_PITCH + c["dpitch"]
    turned = [dataclasses.replace(p, view=camera_view(p.camera_position, yaw + d, pitch)) for d in (0.5, 1.0, 1.5)]
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_pixel_paths(1)
        r.set_pixel_speculate(1)
        seen = []
        for k, fp in enumerate([p, p] + turned + [p] * 4):
            img = r.render(fp)
            seen.append(launches(r))
            if fp is p:
                assert frame_sha(img) == c["sha256"], f"{name}: frame {k + 1} is not the reference shader's"
        print(f"{name}: turn and return, launches per frame {seen}")
        assert seen[0] == 1 and all(n in (1, 3) for n in seen) and seen[-2:] == [3, 3], (name, seen)


@pytest.fixture(scope="module")
def swap(ort, oracle):
    """Two scenes the frame signature cannot tell apart: the same spheres, tree and counts, the
    materials dealt to other spheres.  With the frame and the oracle's render of each."""
    s = ort.random_spheres(100, 42)
    t = ort.build_octree(s, 3, 0)
    perm = np.random.default_rng(7).permutation(s.n)
    s2 = ort.SphereSet(s.center_radius.copy(), s.mat_albedo[perm].copy(), s.fuzz_ri[perm].copy())
    # from just in front of the field (z >= -2.72): main.cpp's pose, 10 units back, has sky in 85 %
    # of its pixels, which no material changes; from here two pixels in three differ
    p = ort.FrameParams.default_camera(160, 120, num_samples=8, max_depth=6, position=(0.0, 1.0, -3.0))
    refs =[oracle.render(x, t, p) for x in (s, s2)]
    for a in refs:
        a.flags.writeable = False
    return (s, s2), t, p, refs


def test_same_signature_scenes_differ(ort, swap):
    """No GPU: the swap below changes more than half the frame, and nothing the signature holds."""
    (s, s2), t, _, refs = swap
    assert np.array_equal(s.center_radius, s2.center_radius) and s.n == s2.n
    assert not np.array_equal(s.mat_albedo, s2.mat_albedo)
    assert same_tree(ort.build_octree(s2, 3, 0), t)  # the geometry is unchanged: t is s2's tree too
    differ = float((refs[0] != refs[1]).any(axis=-1).mean())
    assert differ > 0.5, differ


@pytest.mark.gpu
def test_same_signature_scene_swap(ort, swap):
    """frame_sig holds counts, not contents, and an upload keeps the signatures of the recorded
    RNG end states: after a scene of equal counts is uploaded, the next frame speculates from the
    OLD scene's states.  The per-chunk end-state check must catch every sample that no longer
    follows, whichever way the swap goes."""
    scenes, t, p, refs = swap
    assert float((refs[0] != refs[1]).any(axis=-1).mean()) > 0.5
    with ort.Renderer(0) as r:
        with pixel_paths(r, 1):
            r.set_pixel_speculate(1)
            seen = []
            for which, frames in ((0, 2), (1, 3), (0, 2)):
                r.upload(scenes[which], t)
                for k in range(frames):
                    img = r.render(p)
                    seen.append(launches(r))
                    assert_same(img, refs[which], f"scene {which}, frame {k + 1} after its upload")
            print(f"scene swap: launches per frame {seen}")
            assert seen[:2] == [1, 3] and all(n in (1, 3) for n in seen), seen
