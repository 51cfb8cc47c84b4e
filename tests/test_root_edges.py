"""The fast walk's root and slab shortcuts at their numeric edges, without a GPU: the families of
tests/root_sets.py reach the edges they are named for (asserted with the float32 restatement alone),
and on every family the host emulation (ort_debug_query_rays: the kernels' per-ray function with the
host forms of qdiv, qsqrt and the slab min/max) equals the oracle bit for bit -- brute force, the
sphere as a depth-0 tree, the nine-sphere tree of one-sphere leaves, both layouts, and the tie rays
on the compact5 tree.  The GPU runs the device forms (tests/test_gpu_root_edges.py)."""
import numpy as np
import pytest

import ray_sets
import root_sets as R
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import query_rays_host

F = np.float32
TWO100, TWO_96, TWO_60, TWO_126 = F(2.0 ** 100), F(2.0 ** -96), F(2.0 ** -60), F(2.0 ** -126)

# (kind of scene, layout, use_octree)
CONFIGS = {
    "brute": ("one", L.ORT_LAYOUT_COMPACT, False),
    "root_leaf": ("one", L.ORT_LAYOUT_COMPACT, True),
    "inline": ("inline", L.ORT_LAYOUT_COMPACT, True),
    "explicit_root_leaf": ("one", L.ORT_LAYOUT_EXPLICIT, True),
    "explicit_inline": ("inline", L.ORT_LAYOUT_EXPLICIT, True),
}


def ulps_from_tmin(t):
    return R.bits(t).astype(np.int64) - R.bits1(R.TMIN)


# ---------------------------------------------------------------- coverage (the restatement alone)

@pytest.mark.parametrize("name,root", [("tmin_far", "t2"), ("tmin_near", "t1")])
def test_tmin_families_straddle_t_min(name, root):
    """The designed root (far from inside, near from outside) lies 1..4 ulp below 0.001f for >= 50
    rays, 1..4 ulp above for >= 50, exactly on it for >= 10; every a is in [1/8, 8]."""
    (k, rays), = R.family(name)
    r, = R.restated(name)
    assert k == 0 and len(rays) == 16384
    assert (r["a"] >= 0.125).all() and (r["a"] <= 8).all()
    assert (r["disc"] > 0).all()
    u = ulps_from_tmin(r[root])
    assert ((u >= -4) & (u <= -1)).sum() >= 50
    assert ((u >= 1) & (u <= 4)).sum() >= 50
    assert (u == 0).sum() >= 10
    if name == "tmin_far":  # the near root is behind the origin: far root or nothing
        assert (r["t1"] < 0).all()
        assert np.array_equal(~np.isnan(r["accepted"]), r["t2"] > R.TMIN)
    else:  # the far root is across the sphere: a rejected near root turns into the far one
        assert (~np.isnan(r["accepted"])).all()


def test_graze_sweeps_the_discriminant():
    (k, rays), = R.family("graze")
    r, = R.restated("graze")
    assert len(rays) == 16384
    pos = r["disc"] > 0
    assert pos.mean() >= 0.85
    e = R.exponent(r["disc"][pos])
    assert int(e.max()) - int(e.min()) >= 20
    assert np.array_equal(~np.isnan(r["accepted"]), pos)  # every positive disc has an accepted root
    assert (r["a"] >= 0.125).all() and (r["a"] <= 8).all()


def test_scale_straddles_two_to_the_100():
    fam, res = R.family("scale"), R.restated("scale")
    assert tuple(k for k, _ in fam) == R.SCALE_K
    for (k, rays), r in zip(fam, res):
        assert len(rays) == 1024
        d = r["disc"]
        assert (r["a"] >= 0.125).all() and (r["a"] <= 8).all()
        if 49 <= k <= 52:
            assert (d > TWO100).any() and ((d > 0) & (d <= TWO100)).any(), k
        if k <= 60:
            assert (~np.isnan(r["accepted"])).mean() >= 0.85, k
        if k >= 63:
            assert (~np.isfinite(d)).any(), k


def test_a_edges_hold_every_named_value():
    (k, rays), = R.family("a_edges")
    r, = R.restated("a_edges")
    low, high = R.a_edge_values()
    assert (len(high), len(low)) == (142, 186)
    for name, v in R.A_EDGE_NAMED.items():
        assert (r["a"] == v).sum() >= 8, name
    for x in np.concatenate([low, high]):
        assert (r["a"] == F(x) * F(x)).sum() >= 8, x
    m = R.bits(r["a"]) & 0x7FFFFF
    assert ((m >= 0x7FFFC0).sum() >= 8 * 142) and ((m <= 0x3F).sum() >= 8 * 186)
    # whole waves inside the range, then one wave outside it
    inside = (r["a"] >= 0.125) & (r["a"] <= 8)
    assert inside[:-R.WAVE].all() and not inside[-R.WAVE:].any()
    # hits and grazes and misses
    hit = ~np.isnan(r["accepted"])
    assert 0.5 <= hit.mean() <= 0.9
    assert ((r["disc"] > 0) & (r["disc"] < r["a"] * F(2.0 ** -10))).sum() >= 100


def test_tiny_reaches_the_small_thresholds():
    fam, res = R.family("tiny"), R.restated("tiny")
    assert tuple(k for k, _ in fam) == R.TINY_K
    disc = np.concatenate([r["disc"] for r in res])
    n_abs = np.concatenate([np.minimum(np.abs(r["n1"]), np.abs(r["n2"])) for r in res])
    assert (disc >= TWO_96).sum() >= 100 and ((disc > 0) & (disc < TWO_96)).sum() >= 100
    assert ((disc > 0) & (disc < TWO_126)).sum() >= 100
    assert (n_abs < TWO_60).sum() >= 100
    for r in res:  # every record is a miss
        assert np.isnan(r["accepted"]).all()


def test_mixed_has_lanes_out_of_range_in_every_wave():
    rays, idx = R.mixed()
    r, = R.restated("mixed")
    inside = (r["a"] >= 0.125) & (r["a"] <= 8)
    want = np.zeros(len(rays), bool)
    want[idx] = True
    assert np.array_equal(inside, want)
    per_wave = inside.reshape(-1, R.WAVE).sum(axis=1)
    assert (per_wave == R.MIXED_IN).all() and len(idx) % R.WAVE == 0
    hit = ~np.isnan(r["accepted"])
    assert 0.3 <= hit[idx].mean() <= 0.9


def test_ties_tie():
    rays, corner, tied = R.ties()
    n3 = 8 * R.TIES_PER_OCTANT
    assert n3 >= 4096 and len(rays) == n3 + R.TIES_TWO_AXIS
    assert tied[:n3].all() and (tied[n3:].sum(axis=1) == 2).all()
    assert (np.bincount(R.octants(rays[:n3]), minlength=8) == R.TIES_PER_OCTANT).all()
    assert (np.bincount(R.octants(rays[n3:]), minlength=8) > 0).all()
    sv = R.bits(R.slab_values(corner, rays))
    assert (sv[:n3] == sv[:n3, :1]).all()
    for i in range(n3, len(rays)):
        a, b = np.nonzero(tied[i])[0]
        assert sv[i, a] == sv[i, b]
    assert (R.slab_values(corner, rays)[tied] > 0).all()  # the tie is ahead of the origin
    d = np.abs(rays[:, 3:])
    assert np.isin(d[tied], [0.5, 1.0, 2.0]).all()
    a = R.sphere_hit(rays, [0.0, 0.0, 0.0, 1.0])["a"]
    assert (a >= 0.125).all() and (a <= 8).all()
    # every corner is a corner of a node of the tree
    _, t, _ = ray_sets.scene("compact5")
    planes = [np.unique(np.concatenate([t.node_min[:, k], t.node_max[:, k]])) for k in range(3)]
    for k in range(3):
        assert np.isin(corner[:, k][tied[:, k]], planes[k]).all()


def test_the_inline_scene_holds_the_target_in_one_sphere_leaves(ort):
    """build_octree(s, 2, 1) of the sphere and its eight fillers: the root and its eight children are
    internal, and the target is the only sphere of eight depth-2 leaves (one per octant)."""
    for k in (0, 20, -70):
        s, t = R.scene(k, "inline")
        assert s.n == 9 and t.n_nodes == 1 + 8 + 64
        assert (t.children_offset[:9] >= 0).all() and (t.children_offset[9:] == -1).all()
        leaves = np.nonzero(t.object_count == 1)[0]
        with_target = [i for i in leaves if t.object_indices[t.objects_offset[i]] == 0]
        assert len(with_target) == 8 and len(leaves) == 16
        assert (t.object_count[np.setdiff1d(np.arange(9, 73), leaves)] == 0).all()


# ---------------------------------------------------------------- the host emulation against the oracle

@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", R.ONE_SPHERE)
def test_emulation_equals_the_oracle(ort, oracle, name, config):
    kind, layout, use_octree = CONFIGS[config]
    refs = R.oracle_records(name, kind)
    for (k, rays), ref in zip(R.parts(name, kind), refs):
        s, t = R.scene(k, kind)
        got = query_rays_host(s, t if use_octree else None, rays, layout=layout, use_octree=use_octree, normals=True)
        R.check_records(ort, oracle, s, rays, ref, got, (name, config, k))
    if name not in ("tiny", "scale", "a_edges"):
        assert sum(int(r[:, 0].sum()) for r in refs) >= 1000  # (the families made of hits do hit)


def test_the_restatement_agrees_with_the_oracle():
    """Not a reference, but it must describe the same arithmetic: the restated accepted root is the
    oracle's record on every ray of every one-sphere family."""
    for name in R.ONE_SPHERE:
        for r, ref in zip(R.restated(name), R.oracle_records(name, "one")):
            hit = ~np.isnan(r["accepted"])
            assert np.array_equal(hit, ref[:, 0] == 1), name
            assert np.array_equal(R.bits(r["accepted"])[hit], ref[hit, 1]), name


@pytest.mark.parametrize("layout", [L.ORT_LAYOUT_COMPACT, L.ORT_LAYOUT_EXPLICIT])
def test_emulation_equals_the_oracle_on_ties(ort, oracle, layout):
    s, t, _ = ray_sets.scene("compact5")
    rays = R.ties()[0]
    ref, = R.oracle_records("ties", "tree")
    assert 0.05 <= (ref[:, 0] == 1).mean() <= 0.95  # the tie rays hit and miss
    if layout == L.ORT_LAYOUT_COMPACT:
        got = R.ties_emulated()
        R.check_records(ort, oracle, s, rays, ref, got, "ties")
    else:
        got = query_rays_host(s, t, rays, layout=layout, normals=True)
        assert R.same_records(got, R.ties_emulated())


def test_ties_nearest_emulation_equals_the_yardstick():
    s, t, _ = ray_sets.scene("compact5")
    rays = R.ties()[0]
    yt, ys = R.ties_nearest()
    tt, sph, nrm = query_rays_host(s, t, rays, normals=True, mode="nearest")
    assert np.array_equal(R.bits(tt), R.bits(yt)) and np.array_equal(sph, ys)
    assert np.array_equal(R.bits(nrm), R.bits(ray_sets.numpy_normals(s, rays, yt, ys)))
    tb, sb = query_rays_host(s, None, rays, use_octree=False, mode="nearest")
    assert np.array_equal(R.bits(tb), R.bits(yt)) and np.array_equal(sb, ys)


@pytest.mark.parametrize("config", ["brute", "root_leaf", "inline"])
def test_radiance_emulation_sees_the_oracles_hits(config):
    """The radiance emulation the GPU suite compares with (paths 1, depth 2, grey Lambertian of albedo
    0.5 under the shader's sky, whose blue is (1 - t) + t): a ray the oracle misses returns the sky,
    blue about 1; a ray it hits returns at most half of it."""
    kind = "inline" if config == "inline" else "one"
    rad = R.radiance_emulated(kind, config != "brute")
    hit = np.concatenate([R.oracle_records(n, kind)[0][:, 0] == 1 for n in R.RADIANCE_FAMILIES])
    assert hit.sum() >= 16384 and (~hit).sum() >= 1000
    assert (rad[hit, 2] <= 0.5 + 1e-6).all() and (rad[~hit, 2] >= 0.99).all()
