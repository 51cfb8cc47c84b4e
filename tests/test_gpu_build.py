"""GPU octree builder (ort_build_scene, octreeraytracer_amd/csrc/gpu_build.hip) against the
REFERENCE builder: the committed fixtures and SHA-256 hashes tools/make_golden.py took from
the reference's own src/octree.cpp (tests/golden/manifest.json), the host restatement
(octree.cpp, itself pinned to those fixtures) for shapes the manifest does not hold, and the
rendered frame against the CPU oracle.  Builder edges against the host restatement, bit for bit:
root bounds that are zero with both signs (the reference's sequential fold keeps the first of
equal values; within a block, across blocks and across trips of k_bounds' grid-stride loop),
sphere counts around a block of 256, and one renderer through builds and an upload.

NaN or infinite sphere fields stay out of scope, as tests/chart_scenes.py already declares them:
NaN payloads differ between x86 and the GPU, and the reference leaves the case undefined."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = Path(__file__).resolve().parent / "golden"
MANIFEST = json.loads((G / "manifest.json").read_text())


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scene(ort, name):
    if name == "debug":
        return ort.debug_spheres()
    if name == "prebuilt":
        return ort.prebuilt_spheres()
    if name == "chart":  # tests/chart_scenes.py: a negative radius, concentric and identical spheres
        from chart_scenes import chart
        return chart(ort)
    return ort.random_spheres(int(name.replace("rand", "").replace("k", "000")), 42)


def same_tree(a, b):
    return (np.array_equal(a.gpu_records(), b.gpu_records())
            and np.array_equal(a.object_indices, b.object_indices))


@pytest.mark.parametrize("key", sorted(k for k, e in MANIFEST["trees"].items() if not e.get("hash_only")))
def test_gpu_builder_matches_reference(ort, renderer, key):
    name, d, m = key.split("_")
    d, m = int(d[1:]), int(m[1:])
    s = scene(ort, name)
    renderer.build_scene(s, d, m, keep_tree=True)
    t = renderer.export_octree()
    e = MANIFEST["trees"][key]
    assert (t.n_nodes, t.n_indices) == (e["nodes"], e["indices"]), key
    assert sha(t.gpu_records(), t.object_indices) == e["sha256"], key
    if "file" in e:
        fx = np.load(G / e["file"])
        assert np.array_equal(t.gpu_records(), fx["records"]) and np.array_equal(t.object_indices, fx["indices"])
    assert renderer.info()["layout"] == "compact"
    assert renderer.last_build_ms() > 0


@pytest.mark.parametrize("n,d,m,seed", [(1, 4, 0, 1), (3, 0, 0, 2), (50, 3, -1, 3), (200, 7, 5, 4),
                                        ("twins", 11, 1, 42), (5000, 6, 100000, 6)])
def test_gpu_builder_matches_host_builder(ort, renderer, n, d, m, seed):
    """Edge shapes: one sphere, depth 0, negative / huge maxSpheresPerNode (size_t compare),
    a depth-11 tree (beyond the compact layout: explicit layout on the device).  The last is
    tests/test_gpu_explicit.py's scene of barely overlapping pairs: 1000 random spheres under a
    depth limit of 11 stop splitting at 10 levels or fewer, and the compact layout takes them."""
    if n == "twins":
        from test_gpu_explicit import TWINS, TWINS_TREES, twins
        assert (TWINS[1], m) == (seed, 1)
        s = twins(*TWINS)
    else:
        s = ort.random_spheres(n, seed)
    host = ort.build_octree(s, d, m)
    renderer.build_scene(s, d, m, keep_tree=True)
    assert same_tree(renderer.export_octree(), host)
    depth = renderer.info()["tree_depth"]
    assert renderer.info()["layout"] == ("compact" if depth <= 10 else "explicit")
    if n == "twins":
        assert (host.n_nodes, host.n_indices) == TWINS_TREES[d]
        assert depth == 11 and renderer.info()["layout"] == "explicit"


def test_gpu_builder_coincident_and_touching_spheres(ort, renderer):
    """Spheres sharing centers and tangent to split planes (ties in sphereIntersectsBox)."""
    c = np.array([[0, 0, 0], [0, 0, 0], [1, 1, 1], [-1, -1, -1], [0.5, 0, 0], [0, 0.25, 0]], np.float32)
    s = ort.SphereSet.from_arrays(c, [0.5, 0.5, 0.25, 0.25, 0.5, 0.25], [0, 1, 2, 0, 1, 2], np.full((6, 3), 0.5),
                                  [0, 0.1, 0, 0, 0.2, 0], [1, 1, 1.5, 1, 1, 1.5])
    for d, m in ((3, 0), (5, 1), (8, 2)):
        renderer.build_scene(s, d, m, keep_tree=True)
        assert same_tree(renderer.export_octree(), ort.build_octree(s, d, m)), (d, m)


NEG0, POS0 = 0x80000000, 0x00000000


def zero_bounds(ort, n, at, side):
    """n spheres whose root bound on x (side "min" or "max") is a zero of both signs: spheres at[0]
    and at[1] give -0 and +0, in that order.  min: centre -0 radius 0 (-0 - 0 = -0) and centre 0.5
    radius 0.5; max, mirrored: centre -0 radius -0 (-0 + -0 = -0) and centre -0.5 radius 0.5.  The
    rest: the issue's sphere 0 of the trio, or random_spheres shifted so that no other bound on
    that side reaches 0.  The reference's sequential fold keeps the zero of the lower index."""
    sign = 1.0 if side == "min" else -1.0
    if n == 3:
        cr = np.array([(2 * sign, 2, 2, 1)] * 3, np.float32)
    else:
        cr = ort.random_spheres(n, 11).center_radius.copy()
        bound = cr[:, 0] - sign * cr[:, 3]
        cr[:, 0] += np.float32(2 * sign - (bound.min() if side == "min" else bound.max()))  # every bound beyond +-1
    cr[at[0]] = (-0.0, 3, 3, 0.0 if side == "min" else -0.0)
    cr[at[1]] = (0.5 * sign, 3, 3, 0.5)
    s = ort.SphereSet.empty(n)
    s.center_radius[:] = cr
    s.mat_albedo[:, 1:] = 0.5
    s.fuzz_ri[:, 1] = 1.5
    return s


# (spheres, indices of the -0 and the +0 bound, depth limit, maxSpheresPerNode): the trio and its
# order-swapped variant; the zeros in different blocks of k_bounds; the -0 bound in lane 0 of block
# 0's second trip of the grid-stride loop (1024 blocks of 256), the +0 bound in its first
ZERO_CASES = [(3, (1, 2), 2, 0), (3, (2, 1), 2, 0), (300, (10, 290), 2, 0), (300, (290, 10), 2, 0),
              (262_145, (262_144, 5), 1, 0)]


@pytest.mark.parametrize("side", ["min", "max"])
@pytest.mark.parametrize("n,at,d,m", ZERO_CASES, ids=["trio", "trio_swapped", "two_blocks", "two_blocks_swapped",
                                                      "second_trip"])
def test_gpu_builder_signed_zero_root_bounds(ort, renderer, n, at, d, m, side):
    s = zero_bounds(ort, n, at, side)
    host = ort.build_octree(s, d, m)
    root = (host.node_min if side == "min" else host.node_max)[0, 0].view(np.uint32)
    assert root == (NEG0 if at[0] < at[1] else POS0)  # the host tree: the zero of the lower index
    renderer.build_scene(s, d, m, keep_tree=True)
    t = renderer.export_octree()
    got, want = t.gpu_records().view(np.uint32), host.gpu_records().view(np.uint32)
    # on failure: (node, word of its 9, the device's, the host's) of the first records that differ
    assert same_tree(t, host), [(int(i), int(w), hex(int(got[i, w])), hex(int(want[i, w])))
                                for i, w in np.argwhere(got != want)[:6]]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_gpu_builder_block_boundaries(ort, renderer, n):
    """Sphere counts around one block of 256: the bounds' reduction, the pair lists and the scans."""
    s = ort.random_spheres(n, 5)
    renderer.build_scene(s, 3, 0, keep_tree=True)
    assert same_tree(renderer.export_octree(), ort.build_octree(s, 3, 0))


def test_gpu_builder_one_renderer_through_a_sequence(ort):
    """Builds and an upload one after another in one context: every kept tree is the host's, info()
    follows each step, and a tree that was not kept (or was replaced by an upload) is not exported."""
    from layout_cases import Shape
    big, small = ort.random_spheres(2000, 7), ort.random_spheres(3, 2)
    up = ort.random_spheres(50, 3)
    trees = {"big": ort.build_octree(big, 6, 0), "small": ort.build_octree(small, 0, 0), "up": ort.build_octree(up, 3, 1)}

    def check_info(r, s, t):
        i = r.info()
        assert (i["n_spheres"], i["n_nodes"], i["n_indices"], i["tree_depth"], i["layout"]) == \
               (s.n, t.n_nodes, t.n_indices, Shape(t).depth, "compact")

    with ort.Renderer(0) as r:
        for s, name, d, m in ((big, "big", 6, 0), (small, "small", 0, 0)):
            r.build_scene(s, d, m, keep_tree=True)
            assert same_tree(r.export_octree(), trees[name]), name
            check_info(r, s, trees[name])
        r.upload(up, trees["up"])
        check_info(r, up, trees["up"])
        with pytest.raises(ort.OrtError, match="no GPU-built tree kept"):
            r.export_octree()
        r.build_scene(big, 6, 0, keep_tree=True)
        assert same_tree(r.export_octree(), trees["big"])
        check_info(r, big, trees["big"])
        r.build_scene(small, 0, 0, keep_tree=False)
        check_info(r, small, trees["small"])
        with pytest.raises(ort.OrtError, match="no GPU-built tree kept"):
            r.export_octree()


def test_gpu_built_scene_renders_like_the_oracle(ort, oracle, renderer, scene_c2):
    s, t = scene_c2
    renderer.build_scene(s, 6, 0)
    p = ort.FrameParams.default_camera(1920, 1080)
    img = renderer.render(p)
    ref = oracle.render(s, t, p)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    p2 = ort.FrameParams.default_camera(1920, 1080, num_samples=2, max_depth=3)
    tile = ort.Tile(600, 256, 380, 96)
    assert np.array_equal(renderer.render(p2, tile).view(np.uint32),
                          oracle.render(s, t, p2, 600, 380, 256, 96).view(np.uint32))


def test_gpu_builder_errors(ort, renderer):
    with pytest.raises(ort.OrtError, match="Sphere list is empty"):
        renderer.build_scene(ort.SphereSet.empty(0), 4, 0)
    with pytest.raises(ort.OrtError):
        ort.Renderer(0).export_octree()  # nothing built


def test_gpu_builder_c5_counts(ort, renderer):
    """C5: 1M spheres, depth 10, maxSpheresPerNode 1 -- SURVEY.md 8(d) measured the reference
    at 239,220,401 nodes / 172,356,841 indices (and 132 s of CPU build).  The tree's SHA-256
    against the reference builder's (manifest rand1M_d10_m1) is asserted by
    tests/test_gpu_c5.py, which exports the tree once for the oracle."""
    s = ort.random_spheres(1_000_000, 42)
    renderer.build_scene(s, 10, 1)
    i = renderer.info()
    e = MANIFEST["trees"]["rand1M_d10_m1"]
    assert (i["n_nodes"], i["n_indices"], i["layout"]) == (e["nodes"], e["indices"], "compact")
    assert (e["nodes"], e["indices"]) == (239_220_401, 172_356_841)
    print(f"C5 GPU build {renderer.last_build_ms():.1f} ms")
