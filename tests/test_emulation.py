"""The kernel's per-pixel code (render_core.h: frame-per-level traversal over the compact
layout, and the explicit reference-layout walk) compiled for the HOST and compared with the
independent oracle.  Validates the traversal logic without a GPU; the GPU runs the same
source (tests/test_gpu_parity.py)."""
import numpy as np
import pytest

from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import emulate_render_host


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("layout", [L.ORT_LAYOUT_COMPACT, L.ORT_LAYOUT_EXPLICIT])
def test_c1_primary(ort, oracle, scene_c1, layout):
    s, t = scene_c1
    p = ort.FrameParams.default_camera(256, 256)
    ref, rc = oracle.render(s, t, p, counts=True)
    img, c = emulate_render_host(s, t, p, layout=layout)
    assert same_bits(img, ref)
    assert c == rc


def test_bounces_and_samples(ort, oracle, scene_c1):
    s, t = scene_c1
    p = ort.FrameParams.default_camera(72, 40, num_samples=9, max_depth=8)
    ref, rc = oracle.render(s, t, p, counts=True)
    img, c = emulate_render_host(s, t, p)
    assert same_bits(img, ref) and c == rc


@pytest.mark.parametrize("n,d,m,seed", [(1, 4, 0, 1), (3, 0, 0, 2), (200, 7, 0, 3), (1000, 5, 1, 4), (300, 10, 0, 5),
                                        (4000, 10, 1, 6), (4000, 8, 1, 7)])
def test_scene_shapes(ort, oracle, n, d, m, seed):
    s = ort.random_spheres(n, seed)
    t = ort.build_octree(s, d, m)
    p = ort.FrameParams.default_camera(64, 48, max_depth=3)
    ref = oracle.render(s, t, p)
    img, _ = emulate_render_host(s, t, p)
    assert same_bits(img, ref)


@pytest.mark.parametrize("d", [8, 10])
def test_rejected_sphere_skip_bounces(ort, oracle, d):
    """Bounce rays walk like the GPU bounce kernel (Masks64Plain / Masks96Lean) with the
    rejected-sphere skip (kid_table.h): on maxSpheresPerNode-1 trees, where a sphere sits in
    many leaves, every skip must leave the pixels bit-identical and the counted reference
    work unchanged (the counting walk never skips)."""
    s = ort.random_spheres(6000, 11)
    t = ort.build_octree(s, d, 1)
    p = ort.FrameParams.default_camera(80, 48, num_samples=2, max_depth=5)
    ref, rc = oracle.render(s, t, p, counts=True)
    img, c = emulate_render_host(s, t, p)
    assert same_bits(img, ref) and c == rc


def test_debug_and_prebuilt_scenes(ort, oracle):
    for s, d, m, pos in ((ort.debug_spheres(), 3, 2, (30.0, 20.0, -50.0)), (ort.prebuilt_spheres(), 5, 1, None)):
        t = ort.build_octree(s, d, m)
        p = ort.FrameParams.default_camera(80, 60, max_depth=4) if pos is None else \
            ort.FrameParams.default_camera(80, 60, max_depth=4, position=pos)
        assert same_bits(emulate_render_host(s, t, p)[0], oracle.render(s, t, p))


def test_axis_aligned_rays(ort, oracle):
    """Zero direction components (inf inverse, NaN slabs) and rays grazing split planes."""
    s = ort.SphereSet.from_arrays([[0, 0, 5], [1, 0, 5], [0, 1, 6], [0.5, 0.5, 7]], [0.5, 0.5, 0.5, 0.25],
                                  [0, 1, 2, 0], np.full((4, 3), 0.5), [0, 0.1, 0, 0], [1, 1, 1.5, 1])
    t = ort.build_octree(s, 6, 0)
    for yaw, pitch in ((90.0, 0.0), (-90.0, 0.0), (0.0, 0.0), (90.0, 89.0)):
        p = ort.FrameParams.default_camera(33, 17, max_depth=3, position=(0.0, 0.0, 0.0), yaw=yaw, pitch=pitch)
        assert same_bits(emulate_render_host(s, t, p)[0], oracle.render(s, t, p)), (yaw, pitch)


def test_brute_force(ort, oracle, scene_c1):
    s, _ = scene_c1
    p = ort.FrameParams.default_camera(48, 48, use_octree=0, max_depth=4)
    ref, rc = oracle.render(s, None, p, counts=True)
    img, c = emulate_render_host(s, None, p)
    assert same_bits(img, ref) and c == rc


def test_c2_crop(ort, oracle, scene_c2):
    s, t = scene_c2
    p = ort.FrameParams.default_camera(1920, 1080)
    tile = ort.Tile(900, 120, 400, 64)
    ref = oracle.render(s, t, p, 900, 400, 120, 64)
    img, _ = emulate_render_host(s, t, p, tile)
    assert same_bits(img, ref)


def test_non_derivable_tree_falls_back_to_explicit(ort, oracle, scene_c1):
    """A tree whose boxes are not midpoint splits cannot use the compact layout."""
    s, t = scene_c1
    bad = ort.FlatOctree(t.node_min.copy(), t.node_max.copy(), t.children_offset, t.objects_offset, t.object_count,
                         t.object_indices)
    bad.node_max[5, 1] += np.float32(0.25)
    p = ort.FrameParams.default_camera(32, 32)
    with pytest.raises(ort.OrtError):
        emulate_render_host(s, bad, p, layout=L.ORT_LAYOUT_COMPACT)
    img, _ = emulate_render_host(s, bad, p, layout=L.ORT_LAYOUT_EXPLICIT)
    assert same_bits(img, oracle.render(s, bad, p))


def test_inverted_or_nan_boxes_take_the_exact_walk(ort, oracle):
    """A box with min > max (or a NaN coordinate) is still a valid compact layout, but the
    sign-decided fast walk would misorder its slabs: such scenes take the exact walk."""
    s = ort.random_spheres(50, 11)
    t = ort.build_octree(s, 0, 0)  # the root is the only (leaf) node
    p = ort.FrameParams.default_camera(40, 30, max_depth=2)
    for bad in ("swap", "nan"):
        u = ort.FlatOctree(t.node_min.copy(), t.node_max.copy(), t.children_offset, t.objects_offset,
                           t.object_count, t.object_indices)
        if bad == "swap":
            u.node_min[0, 0], u.node_max[0, 0] = t.node_max[0, 0], t.node_min[0, 0]
        else:
            u.node_min[0, 2] = np.float32("nan")
        img, _ = emulate_render_host(s, u, p, layout=L.ORT_LAYOUT_COMPACT)
        assert same_bits(img, oracle.render(s, u, p)), bad


@pytest.mark.parametrize("name", ["deep11", "deep13", "grown", "forced"])
def test_explicit_walk_on_the_gpu_suites_scenes(ort, oracle, scene_c2, name):
    """The scenes of tests/test_gpu_explicit.py -- trees of 11 and 13 levels, C2's tree with grown
    boxes, C2's own tree under the forced layout -- through the explicit walk on the host, with
    samples and bounces; and what the compact layout says to each."""
    from test_gpu_explicit import TWINS_TREES, explicit_scenes
    s, t, d, refusal = explicit_scenes(scene_c2)[name]
    if d is not None:
        assert (t.n_nodes, t.n_indices) == TWINS_TREES[d]
    p = ort.FrameParams.default_camera(160, 96, num_samples=3, max_depth=5)
    ref = oracle.render(s, t, p)
    img, _ = emulate_render_host(s, t, p, layout=L.ORT_LAYOUT_EXPLICIT)
    assert same_bits(img, ref)
    if refusal is None:
        assert same_bits(emulate_render_host(s, t, p, layout=L.ORT_LAYOUT_COMPACT)[0], ref)
    else:
        with pytest.raises(ort.OrtError, match=refusal):
            emulate_render_host(s, t, p, layout=L.ORT_LAYOUT_COMPACT)


def extreme_root_scene(ort):
    """Sphere-root edge cases for the fast walk's quotient/sqrt shortcuts (render_core.h
    qdiv/qsqrt): the camera inside a sphere (near root negative, far root taken), a sphere
    whose surface passes by the lens (roots near 0), one far enough that half_b^2 overflows
    (disc = inf: the IEEE division path), one whose disc exceeds 2^100 (the IEEE sqrt path),
    and ordinary spheres in front."""
    return ort.SphereSet.from_arrays(
        [[0, 2.5, -10], [0, 2.5, -12], [0.5, 2.5, -1e20], [0, 2.5, -2e18], [0, 2.5, -20], [1.5, 2, -16],
         [-1, 3, -25]],
        [3.0, 2.0, 1e19, 1e18, 1.0, 0.5, 0.75], [2, 1, 0, 0, 0, 1, 2],
        [[0.9, 0.9, 0.9], [0.8, 0.6, 0.2], [0.2, 0.4, 0.8], [0.5, 0.9, 0.3], [0.7, 0.1, 0.1], [0.3, 0.3, 0.9],
         [0.9, 0.9, 0.6]],
        [0, 0.2, 0, 0, 0, 0.1, 0], [1.5, 1, 1, 1, 1, 1, 1.3])


@pytest.mark.parametrize("use_octree", [1, 0])
def test_extreme_sphere_roots(ort, oracle, use_octree):
    s = extreme_root_scene(ort)
    t = ort.build_octree(s, 5, 0) if use_octree else None
    p = ort.FrameParams.default_camera(64, 40, max_depth=4, use_octree=use_octree)
    assert same_bits(emulate_render_host(s, t, p)[0], oracle.render(s, t, p))


def test_walk_steps_analysis_matches_counters(ort, oracle, scene_c1):
    """ort_debug_walk_steps (tools/walk_sim.py's input, analysis only) replays the kernel's own
    fast walk: over every 8x8 block its per-step object counts add up to the oracle's."""
    import ctypes as C
    from octreeraytracer_amd import _lib as L
    s, t = scene_c1
    p = ort.FrameParams.default_camera(256, 256)
    _, rc = oracle.render(s, t, p, counts=True)
    f = L.analysis_lib().ort_debug_walk_steps
    f.restype = C.c_int64
    fp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    arr = [np.ascontiguousarray(x) for x in (s.center_radius, s.mat_albedo, s.fuzz_ri)]
    tt = [np.ascontiguousarray(x) for x in (t.node_min, t.node_max, t.children_offset, t.objects_offset,
                                             t.object_count, t.object_indices)]
    lens = np.zeros(32 * 32 * 64, np.int32)
    steps = np.zeros(256 * 256 * 200, np.uint16)
    n = f(fp(arr[0]), fp(arr[1]), fp(arr[2]), C.c_int32(s.n), fp(tt[0]), fp(tt[1]), fp(tt[2]), fp(tt[3]),
          fp(tt[4]), C.c_int32(t.n_nodes), fp(tt[5]), C.c_int64(t.n_indices), C.byref(p.to_c()), C.c_int32(1),
          fp(lens), C.c_int64(len(lens)), fp(steps), C.c_int64(len(steps)))
    assert n == int(lens.sum()) > 0
    assert int((steps[:n] & 0xff).astype(np.int64).sum()) == rc["leaf_objects"]
    assert 0 < int(np.count_nonzero(lens)) <= rc["traversals"]  # root-box misses take no step


def _trace_rays(ort, s, t, rays, bounce):
    from octreeraytracer_amd import _lib as L
    lib = L.analysis_lib()
    arr = [np.ascontiguousarray(a, d) for a, d in (
        (s.center_radius, np.float32), (t.node_min, np.float32), (t.node_max, np.float32),
        (t.children_offset, np.int32), (t.objects_offset, np.int32), (t.object_count, np.int32),
        (t.object_indices, np.int32))]
    rays = np.ascontiguousarray(rays, np.float32)
    out = np.zeros((len(rays), 5), np.int32)
    L.acheck(lib.ort_debug_trace_rays(L.fptr(arr[0]), s.n, L.fptr(arr[1]), L.fptr(arr[2]), L.iptr(arr[3]),
                                     L.iptr(arr[4]), L.iptr(arr[5]), t.n_nodes, L.iptr(arr[6]), t.n_indices,
                                     L.fptr(rays), len(rays), int(bounce), L.iptr(out)))
    return out


@pytest.mark.parametrize("d,m,bounce", [(5, 1, 0), (5, 1, 1), (8, 0, 0), (8, 0, 1), (10, 1, 1)])
def test_zero_direction_components_take_the_fast_walk(ort, oracle, d, m, bounce):
    """Rays with exactly zero direction components (+0 and -0, one or two axes): the fast walk
    takes them (inv = +-inf signed by the shader's order table for that sign vector) and finds
    the exact walk's hit -- same entry, same t bits -- unless the origin lies exactly on a split
    plane of a zero axis (NaN slabs), which it refuses (deferred to the exact walk)."""
    s = ort.random_spheres(2000, 7)
    t = ort.build_octree(s, d, m)
    rng = np.random.default_rng(d * 10 + m + bounce)
    lo, hi = t.node_min[0].astype(np.float64), t.node_max[0].astype(np.float64)
    n = 3000
    o = lo + (hi - lo) * rng.uniform(-0.05, 1.05, (n, 3))
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    kinds = rng.integers(0, 6, n)
    for i, k in enumerate(kinds):  # zero out one or two axes, with either zero sign
        axes = [k % 3] if k < 3 else [k % 3, (k + 1) % 3]
        for a in axes:
            dirs[i, a] = -0.0 if rng.random() < 0.5 else 0.0
        nz = [a for a in range(3) if a not in axes]
        dirs[i, nz] /= np.linalg.norm(dirs[i, nz])
    # a tenth of the origins exactly on a split plane of a zero axis (a node box's min)
    on_plane = rng.random(n) < 0.1
    for i in np.nonzero(on_plane)[0]:
        a = next(a for a in range(3) if dirs[i, a] == 0.0)
        o[i, a] = t.node_min[rng.integers(0, t.n_nodes), a]
    rays = np.concatenate([o, dirs], axis=1).astype(np.float32)
    out = _trace_rays(ort, s, t, rays, bounce)
    fast = out[:, 0] == 1
    # the exact walk (what the deferred rays get) against the oracle's traverseOctree
    ref = oracle.trace_rays(s, t, rays)
    assert ((out[:, 3] >= 0) == (ref[:, 0] == 1)).all() and (out[ref[:, 0] == 1, 4] == ref[ref[:, 0] == 1, 1]).all()
    assert not fast[on_plane].any(), "a ray with NaN slabs took the fast walk"
    assert fast[~on_plane].mean() > 0.95
    agree = (out[:, 1] == out[:, 3]) & ((out[:, 1] < 0) | (out[:, 2] == out[:, 4]))
    bad = np.nonzero(fast & ~agree)[0]
    assert bad.size == 0, (bad[:5], rays[bad[:3]], out[bad[:3]])
    assert (out[fast, 1] >= 0).sum() > 20  # some of them hit spheres


def test_ordinary_rays_fast_equals_exact(ort):
    """The same check for ordinary rays (no zero components), as a control."""
    s = ort.random_spheres(2000, 7)
    t = ort.build_octree(s, 6, 0)
    rng = np.random.default_rng(5)
    lo, hi = t.node_min[0].astype(np.float64), t.node_max[0].astype(np.float64)
    o = lo + (hi - lo) * rng.uniform(0, 1, (2000, 3))
    dirs = rng.normal(size=(2000, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    out = _trace_rays(ort, s, t, np.concatenate([o, dirs], axis=1), 0)
    assert (out[:, 0] == 1).all()
    assert (out[:, 1] == out[:, 3]).all() and (out[out[:, 1] >= 0, 2] == out[out[:, 1] >= 0, 4]).all()


def _split_rays(ort, s, t, rays, level, lanes):
    from octreeraytracer_amd import _lib as L
    lib = L.analysis_lib()
    arr = [np.ascontiguousarray(a, d) for a, d in (
        (s.center_radius, np.float32), (t.node_min, np.float32), (t.node_max, np.float32),
        (t.children_offset, np.int32), (t.objects_offset, np.int32), (t.object_count, np.int32),
        (t.object_indices, np.int32))]
    rays = np.ascontiguousarray(rays, np.float32)
    out = np.zeros((len(rays), 4), np.int32)
    L.acheck(lib.ort_debug_split_rays(L.fptr(arr[0]), s.n, L.fptr(arr[1]), L.fptr(arr[2]), L.iptr(arr[3]),
                                     L.iptr(arr[4]), L.iptr(arr[5]), t.n_nodes, L.iptr(arr[6]), t.n_indices,
                                     L.fptr(rays), len(rays), int(level), int(lanes), L.iptr(out)))
    return out


@pytest.mark.parametrize("n,d,m", [(2000, 5, 0), (10_000, 8, 0), (2000, 8, 1), (3000, 10, 1)])
def test_split_walk_equals_the_walk(ort, oracle, n, d, m):
    """The split walk of ort_trace_split (render_core.h traverse_split): one ray's walk dealt over
    several lanes by its level-L subtrees, the lanes' first hits merged by DFS position, finds the
    walk's own hit (entry and t bits) -- for every split level, lane count, camera rays (with the
    field's longest, grazing walks) and random rays from inside the scene."""
    s = ort.random_spheres(n, 11)
    t = ort.build_octree(s, d, m)
    rng = np.random.default_rng(n + d + m)
    p = ort.FrameParams.default_camera(320, 180)
    cam = oracle.camera(p)[:12].astype(np.float64).reshape(4, 3)  # origin, lower-left, horizontal, vertical
    u, v = rng.uniform(0, 1, (2, 1500))
    org = np.broadcast_to(cam[0], (1500, 3))
    dirs = cam[1] + u[:, None] * cam[2] + v[:, None] * cam[3] - cam[0]
    lo, hi = t.node_min[0].astype(np.float64), t.node_max[0].astype(np.float64)
    o2 = lo + (hi - lo) * rng.uniform(0, 1, (1500, 3))
    d2 = rng.normal(size=(1500, 3))
    rays = np.concatenate([np.concatenate([org, dirs], 1), np.concatenate([o2, d2], 1)]).astype(np.float32)
    rays[:, 3:] /= np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    want = _trace_rays(ort, s, t, rays, 0)
    fast = want[:, 0] == 1
    assert fast.mean() > 0.99
    one = None  # the walk's own steps (one lane walks it all)
    for level in range(1, d + 1):
        for lanes in (1, 3, 8):
            got = _split_rays(ort, s, t, rays, level, lanes)
            assert np.array_equal(got[fast, 0], want[fast, 1]), (level, lanes)
            hit = want[fast, 1] >= 0
            assert np.array_equal(got[fast, 1][hit], want[fast, 2][hit]), (level, lanes)
            # the steps ort_trace_split records for the next frame (the longest stretch above the
            # level + the lanes' own subtree steps): the walk's own count when it misses (every
            # lane walks to the end), at least that when a hit ends it early
            if one is None:
                one = got[:, 3].copy()
            assert np.array_equal(got[fast, 3][~hit], one[fast][~hit]), (level, lanes)
            assert (got[fast, 3] >= one[fast]).all(), (level, lanes)
            if lanes == 1:
                assert np.array_equal(got[:, 3], one), level
    # and the oracle's traverseOctree on a sample
    ref = oracle.trace_rays(s, t, rays[:400])
    got = _split_rays(ort, s, t, rays[:400], max(1, d - 5), 8)
    sel = fast[:400]
    assert np.array_equal((got[sel, 0] >= 0).astype(np.int32), ref[sel, 0])
    hit = ref[sel, 0] == 1
    assert np.array_equal(got[sel, 1][hit], ref[sel, 1][hit])
    assert hit.mean() > 0.05

