"""The explicit (reference-layout) GPU path -- ort_trace_kernel<1, ...> with its per-lane stack and
the unfused pipeline behind it (hit records, ort_shade_kernel, the three path orders,
ort_finalize_kernel) -- on the trees that take it: deeper than the compact layout's 10 levels,
boxes that are no midpoint splits, and a midpoint tree under ORT_OPT_FORCE_LAYOUT.  Bounces,
samples, tiles and bands, the counters and the GPU builder, every frame bit for bit the CPU
oracle's on the same tree.  The exact compact walk on inverted / NaN boxes closes the file.

The scenes are proved on the CPU first: tests/test_emulation.py runs them through the host
emulation of the same walk, and test_explicit_scenes_are_refused_by_the_compact_layout (no GPU)
pins the refusals."""
import numpy as np
import pytest

import octreeraytracer_amd as ort_pkg
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import emulate_render_host
from test_gpu_build import same_tree
from test_gpu_parity import assert_same

# twins(100, 42, 8, 1.999) under maxSpheresPerNode 1, by the host builder: depth limit ->
# (nodes, indices); the tree reaches the limit (in the thin lens where a pair overlaps)
TWINS = (100, 42, 8, 1.999)
TWINS_TREES = {11: (19_473, 17_310), 13: (67_097, 66_162)}
TOO_DEEP = "tree deeper than the compact layout supports"
NOT_DERIVABLE = "node box not derivable from split planes"
SCENES = ["deep11", "deep13", "grown", "forced"]


def twins(n, seed, k, gap):
    """random_spheres(n, seed) plus a copy of each of its last k spheres moved gap radii along
    +x.  With gap just below 2 each pair barely overlaps: under maxSpheresPerNode 1 the builder
    splits down to its depth limit there and nowhere else, so the tree is deep and small."""
    s = ort_pkg.random_spheres(n, seed)
    cr = s.center_radius[-k:].copy()
    cr[:, 0] += np.float32(gap) * cr[:, 3]
    return ort_pkg.SphereSet(np.concatenate([s.center_radius, cr]),
                             np.concatenate([s.mat_albedo, s.mat_albedo[-k:]]),
                             np.concatenate([s.fuzz_ri, s.fuzz_ri[-k:]]))


def grown_boxes(t):
    """t with every box but the root's grown by 1/64 on all six faces (float32): no midpoint
    octree any more, the same topology."""
    g = np.float32(1.0 / 64.0)
    nmin, nmax = t.node_min.copy(), t.node_max.copy()
    nmin[1:] -= g
    nmax[1:] += g
    return ort_pkg.FlatOctree(nmin, nmax, t.children_offset, t.objects_offset, t.object_count, t.object_indices)


def explicit_scenes(c2):
    """name -> (spheres, tree, builder depth or None, the compact layout's refusal or None);
    c2: the scene_c2 fixture.  `forced` is the only one the compact layout accepts."""
    tw = twins(*TWINS)
    s2, t2 = c2
    return {"deep11": (tw, ort_pkg.build_octree(tw, 11, 1), 11, TOO_DEEP),
            "deep13": (tw, ort_pkg.build_octree(tw, 13, 1), 13, TOO_DEEP),
            "grown": (s2, grown_boxes(t2), None, NOT_DERIVABLE),
            "forced": (s2, t2, None, None)}


@pytest.fixture(scope="module")
def scenes(scene_c2):
    return explicit_scenes(scene_c2)


FULL = dict(num_samples=2, max_depth=5)
ODD = (13, 77, 29, 51)
BAND = (0, 320, 150, 64, 16, 64)  # rows y = 150 + 64 (j / 16) + j % 16: those from j = 16 on past the frame
_refs = {}


def oracle_frames(oracle, scenes, name):
    """The oracle's frames of a scene, rendered once and shared (read-only)."""
    if name not in _refs:
        s, t = scenes[name][:2]
        p = ort_pkg.FrameParams.default_camera(320, 180, **FULL)
        p1 = ort_pkg.FrameParams.default_camera(320, 180)
        r = {"full": oracle.render(s, t, p), "odd": oracle.render(s, t, p, ODD[0], ODD[2], ODD[1], ODD[3]),
             "band": oracle.render(s, t, p, 0, 150, 320, 64, band_height=16, band_stride=64),
             "primary": oracle.render(s, t, p1)}
        for a in r.values():
            a.flags.writeable = False
        _refs[name] = r
    return _refs[name]


def upload_explicit(r, scenes, name):
    s, t, _, refusal = scenes[name]
    if refusal is None:
        r.set_layout(L.ORT_LAYOUT_EXPLICIT)
    r.upload(s, t)
    i = r.info()
    assert i["layout"] == "explicit" and (i["n_nodes"], i["n_indices"]) == (t.n_nodes, t.n_indices), name
    return s, t


def test_explicit_scenes_are_refused_by_the_compact_layout(ort, scenes):
    """No GPU: the node counts the GPU tests rely on, and the compact layout's refusals."""
    p = ort.FrameParams.default_camera(8, 8)
    for name in SCENES:
        s, t, d, refusal = scenes[name]
        if d is not None:
            assert (t.n_nodes, t.n_indices) == TWINS_TREES[d], name
        if refusal is None:
            emulate_render_host(s, t, p, layout=L.ORT_LAYOUT_COMPACT)
        else:
            with pytest.raises(ort.OrtError, match=refusal):
                emulate_render_host(s, t, p, layout=L.ORT_LAYOUT_COMPACT)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [0, 1, 2])
@pytest.mark.parametrize("name", SCENES)
def test_explicit_layout_bounces(ort, oracle, scenes, name, sort):
    """2 samples x 5 bounces on the explicit layout: the bounce launches of the stack walk
    (PRIMARY = false, rays read through the path list), mode-1 shading and each order of the
    alive paths (the list sort keyed from this tree's root box); a full frame, an odd tile and a
    band tile with padding rows.  The options that choose among the compact layout's kernels
    (persistent bounce walks, whole-pixel paths) change nothing here, and a primary-ray frame
    after the larger ones sees none of their path state."""
    ref = oracle_frames(oracle, scenes, name)
    p = ort.FrameParams.default_camera(320, 180, **FULL)
    with ort.Renderer(0) as r:
        upload_explicit(r, scenes, name)
        r.set_sort_paths(sort)
        what = f"explicit {name} sort={sort}"
        assert_same(r.render(p), ref["full"], what)
        assert_same(r.render(p, ort.Tile(*ODD)), ref["odd"], f"{what} odd tile")
        band = r.render(p, ort.Tile(*BAND))
        assert_same(band, ref["band"], f"{what} band")
        assert float(np.abs(band[16:]).max()) == 0.0  # rows past the frame
        for persistent in (0, 2):
            r.set_persistent(persistent)
            for pp in (-1, 0, 1):
                r.set_pixel_paths(pp)
                assert_same(r.render(p), ref["full"], f"{what} persistent={persistent} pixel_paths={pp}")
                assert r.frame_trace_times_ms(1)[0][1] > 1  # the pipeline: a launch per bounce
        assert_same(r.render(ort.FrameParams.default_camera(320, 180)), ref["primary"], f"{what} primary after")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep11", "deep13"])
def test_explicit_layout_uploaded_and_gpu_built_agree(ort, oracle, scenes, name):
    """The GPU builder on trees deeper than 10 levels: the host builder's tree, the explicit
    layout, and the frame of the uploaded tree and of the oracle."""
    s, t, d, _ = scenes[name]
    ref = oracle_frames(oracle, scenes, name)["full"]
    p = ort.FrameParams.default_camera(320, 180, **FULL)
    with ort.Renderer(0) as r:
        upload_explicit(r, scenes, name)
        uploaded = r.render(p)
        r.build_scene(s, d, 1, keep_tree=True)
        i = r.info()
        assert (i["n_nodes"], i["n_indices"]) == TWINS_TREES[d]
        assert i["tree_depth"] == d and i["layout"] == "explicit"
        assert same_tree(r.export_octree(), t)
        built = r.render(p)
    assert_same(built, uploaded, f"{name}: GPU-built against uploaded")
    assert_same(built, ref, f"{name}: GPU-built against the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep11", "grown"])
def test_explicit_layout_counters(ort, oracle, scenes, name):
    """The counting stack walk: nodes popped, child records, leaf spheres and accepted hits of a
    primary-ray frame -- and of a bounced one, where a bounce launch that walked any slot outside
    its path list would count work the reference never does."""
    s, t = scenes[name][:2]
    with ort.Renderer(0) as r:
        upload_explicit(r, scenes, name)
        for ns, md in ((1, 1), (2, 3)):
            p = ort.FrameParams.default_camera(160, 96, num_samples=ns, max_depth=md)
            _, want = oracle.render(s, t, p, counts=True)
            assert r.count_traffic(p) == want, (name, ns, md)


@pytest.mark.gpu
def test_exact_walk_on_inverted_and_nan_boxes_gpu(ort, oracle):
    """tests/test_emulation.py test_inverted_or_nan_boxes_take_the_exact_walk on the GPU: a root
    box with min > max, or a NaN coordinate, keeps the compact layout and takes the exact walk
    (the sign-decided fast walk would misorder its slabs), in the pipeline and in whole-pixel
    paths."""
    from test_gpu_parity import pixel_paths
    s = ort.random_spheres(50, 11)
    t = ort.build_octree(s, 0, 0)  # the root is the only (leaf) node
    for bad in ("swap", "nan"):
        u = ort.FlatOctree(t.node_min.copy(), t.node_max.copy(), t.children_offset, t.objects_offset,
                           t.object_count, t.object_indices)
        if bad == "swap":
            u.node_min[0, 0], u.node_max[0, 0] = t.node_max[0, 0], t.node_min[0, 0]
        else:
            u.node_min[0, 2] = np.float32("nan")
        with ort.Renderer(0) as r:
            r.upload(s, u)
            assert r.info()["layout"] == "compact"
            for ns, md in ((1, 1), (2, 4)):
                p = ort.FrameParams.default_camera(40, 30, num_samples=ns, max_depth=md)
                ref = oracle.render(s, u, p)
                for mode in (0, 1):
                    with pixel_paths(r, mode):
                        assert_same(r.render(p), ref, f"{bad} box {ns} x {md} pixel_paths={mode}")
