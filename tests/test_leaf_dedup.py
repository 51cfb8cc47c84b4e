"""A sphere shared by sibling leaves tested once per node (render_core.h leaf_repeat_masks, cam_record
and leaf_kids under Masks64::kLeafDedup), on the host: no GPU needed.

The repeat masks of hand-made leaf-children nodes against the expected sets, and of whole trees
against the rule restated in Python; emulated frames -- the host walk reading the masks the same
functions derived -- bit for bit against the oracle, with the analysis hook showing that children
were in fact dropped; and the edges: a camera inside a sphere, rays grazing a sphere, a set that is
rejected in front of a sibling that hits, rays with zero direction components."""
import numpy as np
import pytest

import pop_table_cases as cases
from leaf_dedup_cases import (BIG_CENTRE, GROUP_NODES, INTERNAL, LEAFKIDS, behind_rays, behind_scene, big_scene,
                              dedup_counts, expected_cam_node, group_scene, host_cam_node, seeded_scene, trace_rays)
from leaf_inline_cases import TAG, layout_arrays
from octreeraytracer_amd.renderer import emulate_render_host


def _build_dedups():
    return dedup_counts(False)[2]


def test_build_has_repeat_masks():
    """The build ships the skip (Masks64::kLeafDedup, reported as 1): everything below relies on it."""
    assert _build_dedups() in (1, 2)


# ---- the masks -----------------------------------------------------------------------------------
def test_masks_of_the_grouping_tree():
    s, t = group_scene()
    node, sph, l16 = layout_arrays(s, t)
    cam = host_cam_node(s, t)
    assert cam.shape == node.shape == (t.n_nodes, 2)
    root = int(node[0, 0])
    for k, (_, a, b) in GROUP_NODES.items():
        i = root + k
        assert node[i, 1] & INTERNAL and node[i, 1] & LEAFKIDS, k
        got_a, got_b = (int(cam[i, 1]) >> 8) & 0xFF, (int(cam[i, 1]) >> 16) & 0xFF
        assert (got_a, got_b) == (a, b), (k, bin(got_a), bin(got_b))
        assert cam[i, 0] == node[i, 0] and (int(cam[i, 1]) & 0xFF0000FF) == (int(node[i, 1]) & 0xFF0000FF), k
    # the cases the sets rest on: the NaN leaf keeps the list form, the twin ids share their bits
    first = int(node[root, 0])
    assert l16[first + 0, 3] & TAG and not l16[first + 2, 3] & TAG
    twin = int(node[root + 2, 0])
    assert np.array_equal(l16[twin + 2], l16[twin + 3]) and node[twin + 2, 0] != node[twin + 3, 0]
    near = int(node[root + 1, 0])
    assert np.array_equal(l16[near + 0, :3], l16[near + 1, :3]) and l16[near + 0, 3] != l16[near + 1, 3]
    # every other record -- the root (children of its own that are internal), the leaves -- is node[]'s
    plain = np.ones(t.n_nodes, bool)
    plain[[root + k for k in GROUP_NODES]] = False
    assert not (node[0, 1] & LEAFKIDS) and np.array_equal(cam[plain], node[plain])
    assert np.array_equal(cam, expected_cam_node(node, l16))


@pytest.mark.parametrize("scene", ("big", "seeded", "pop_d3", "pop_d8"))
def test_masks_follow_the_rule(scene):
    s, t = {"big": big_scene, "seeded": seeded_scene, "pop_d3": lambda: cases.scene(3, 0),
            "pop_d8": lambda: cases.scene(8, 0)}[scene]()
    node, _, l16 = layout_arrays(s, t)
    cam = host_cam_node(s, t)
    assert np.array_equal(cam, expected_cam_node(node, l16))
    lk = ((node[:, 1] & INTERNAL) != 0) & ((node[:, 1] & LEAFKIDS) != 0)
    assert np.array_equal(cam[~lk], node[~lk])
    with_a = int((((cam[lk, 1] >> 8) & 0xFF) != 0).sum())
    with_b = int((((cam[lk, 1] >> 16) & 0xFF) != 0).sum())
    print(f"{scene}: {int(lk.sum())} leaf-children nodes, {with_a} with a set A, {with_b} with a set B")
    if scene in ("big", "seeded"):  # (the big spheres lie apart: no node of theirs sees two of them alone twice)
        assert with_a > 0 and (with_b > 0 or scene == "big")


def test_deep_trees_have_no_records(ort):
    s = ort.random_spheres(300, 42)
    assert len(host_cam_node(s, ort.build_octree(s, 9, 0))) == 0


# ---- frames --------------------------------------------------------------------------------------
@pytest.mark.parametrize("diag", cases.DIAGONALS)
def test_big_sphere_frames_are_the_oracles(ort, oracle, diag):
    s, t = big_scene()
    p = cases.pose(ort, (64, 64), diag)
    dedup_counts(True)
    got = emulate_render_host(s, t, p)[0]
    tested, dropped, _ = dedup_counts(True)
    print(f"{diag}: {tested} leaf children tested, {dropped} dropped")
    assert dropped > 0 and tested > 0
    assert cases.same_bits(got, oracle.render(s, t, p))
    # (spheres in the frame and sky beside them: one bounce shades every sphere pixel alike, the sky varies)
    _, n_alike = np.unique(np.asarray(got).reshape(-1, 3), axis=0, return_counts=True)
    assert 0.05 * 64 * 64 < n_alike.max() < 64 * 64 and len(n_alike) >= 3


def test_seeded_depth6_frame_is_the_oracles(ort, oracle):
    s, t = seeded_scene()
    p = ort.FrameParams.default_camera(96, 64)
    dedup_counts(True)
    got = emulate_render_host(s, t, p)[0]
    tested, dropped, _ = dedup_counts(True)
    print(f"{tested} leaf children tested, {dropped} dropped")
    assert dropped > 0
    assert cases.same_bits(got, oracle.render(s, t, p))


# ---- edges ---------------------------------------------------------------------------------------
def test_camera_inside_a_sphere(ort, oracle):
    s, t = big_scene()
    c = np.asarray(s.center_radius[0, :3], np.float64) + (0.1, 0.2, 0.05)
    for diag in cases.DIAGONALS[:3]:
        yaw, pitch = _yaw_pitch(diag)
        p = ort.FrameParams.default_camera(48, 32, position=tuple(float(v) for v in c), yaw=yaw, pitch=pitch)
        dedup_counts(True)
        got = emulate_render_host(s, t, p)[0]
        # (from inside, a ray's first leaf holds the sphere and its far root is accepted there: the
        # sets drop siblings only for the rays that leave through a gap in the frame's corners, if any)
        assert dedup_counts(True)[0] > 48 * 32 // 2
        assert cases.same_bits(got, oracle.render(s, t, p)), diag


def _yaw_pitch(diag):
    import math
    sx, sy, sz = diag
    return math.degrees(math.atan2(sz, sx)), math.degrees(math.asin(sy / math.sqrt(3.0)))


def _fast_equals_exact(out):
    fast = out[:, 0] == 1
    assert np.array_equal(out[fast, 1], out[fast, 3]) and np.array_equal(out[fast, 2], out[fast, 4])
    return fast


def test_grazing_rays():
    """Rays from BIG_CENTRE at points of each sphere's silhouette and a few ulps to either side of it:
    the discriminant is around 0, the camera walk's answer is the exact walk's either way."""
    s, t = big_scene()
    eye = np.asarray(BIG_CENTRE, np.float64)
    rays = []
    rng = np.random.default_rng(3)
    for c4 in np.asarray(s.center_radius, np.float64):
        c, r = c4[:3], c4[3]
        oc = c - eye
        dist = np.linalg.norm(oc)
        axis = oc / dist
        # tangent points: on the sphere, where the radius is perpendicular to the line of sight
        along, off = dist - r * r / dist, r * np.sqrt(1.0 - (r / dist) ** 2)
        for _ in range(24):
            u = np.cross(axis, rng.normal(size=3))
            u /= np.linalg.norm(u)
            for scale in (1.0, 1.0 - 3e-7, 1.0 + 3e-7, 1.0 - 1e-6, 1.0 + 1e-6):
                d = along * axis + scale * off * u
                rays.append(np.concatenate([eye, d / np.linalg.norm(d)]))
    dedup_counts(True)
    out = trace_rays(s, t, np.asarray(rays, np.float32))
    tested, dropped, _ = dedup_counts(True)
    fast = _fast_equals_exact(out)
    hits = int((out[fast, 1] >= 0).sum())
    print(f"{int(fast.sum())} grazing rays, {hits} hit; {tested} leaf children tested, {dropped} dropped")
    assert fast.sum() > 900 and 50 < hits < fast.sum() - 50 and dropped > 0


def test_a_rejected_set_in_front_of_a_sibling_that_hits():
    s, t = behind_scene()
    node, _, l16 = layout_arrays(s, t)
    cam = host_cam_node(s, t)
    lk = int(node[0, 0])  # root octant 0
    assert ((int(cam[lk, 1]) >> 8) & 0xFF, (int(cam[lk, 1]) >> 16) & 0xFF) == (0b00010111, 0b01101000)
    rays = behind_rays()
    dedup_counts(True)
    out = trace_rays(s, t, rays)
    tested, dropped, build = dedup_counts(True)
    fast = _fast_equals_exact(out)
    hit = fast & (out[:, 1] >= 0)
    print(f"{int(fast.sum())} rays, {int(hit.sum())} hit; {tested} leaf children tested, {dropped} dropped")
    assert fast.sum() > 350 and hit.sum() > 150 and dropped > 0
    # every hit is sphere 1's: through a one-sphere leaf of set B (its entry in the per-sphere tail) or
    # through the two-sphere leaf behind (entry 1 of its list); sphere 0, set A's, is never hit
    entries = set(int(e) for e in out[hit, 1])
    list_leaf = int(node[lk, 0]) + 7
    assert entries <= {t.n_indices + 1, int(node[list_leaf, 0]) + 1}, entries
    assert t.n_indices + 1 in entries


def test_zero_direction_components():
    s, t = big_scene()
    eye = np.asarray(BIG_CENTRE, np.float32)
    dirs = []
    for a in range(3):
        for sgn in (1.0, -1.0):
            d = np.zeros(3, np.float32)
            d[a] = sgn
            dirs.append(d)                      # two zero components
            for b in range(3):
                if b != a:
                    for sb in (0.75, -0.75):
                        e = d.copy()
                        e[b] = sb
                        dirs.append(e / np.linalg.norm(e))  # one zero component
    rays = []
    for off in ((0, 0, 0), (0.4, -0.3, 0.2), (-1.1, 0.9, 1.3), (1.3, 1.2, -1.0)):
        for d in dirs:
            rays.append(np.concatenate([eye + np.asarray(off, np.float32), d]))
    dedup_counts(True)
    out = trace_rays(s, t, np.asarray(rays, np.float32))
    tested, dropped, _ = dedup_counts(True)
    fast = _fast_equals_exact(out)
    print(f"{len(rays)} rays, {int(fast.sum())} on the fast walk, {int((out[fast, 1] >= 0).sum())} hit; "
          f"{tested} leaf children tested, {dropped} dropped")
    assert fast.sum() >= len(rays) // 2 and (out[fast, 1] >= 0).sum() > 10 and dropped > 0
