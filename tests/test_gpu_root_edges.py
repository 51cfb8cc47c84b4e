"""The fast walk's root and slab shortcuts at their numeric edges, on the GPU: the device forms of
qsqrt (hardware estimate and two residual tests), qdiv (Markstein quotient) and the raw min3 / max3
slab tests exist only there.  Renderer.trace_rays over the families of tests/root_sets.py against
the oracle's records: brute force on one sphere (traverse_brute runs sphere_hit_fast for every ray
of a wave whose lanes all meet its preconditions), the sphere as a depth-0 tree, a nine-sphere tree
whose one-sphere leaves are tested inline, the explicit layout (the exact sphere_hit_t), the
traversal options, waves of mixed preconditions, rays through node corners and edges, device
pointers on a stream, and radiance queries against the host emulation.  Every comparison is exact;
tests/test_root_edges.py shows that the families reach their edges."""
import numpy as np
import pytest

import ray_sets
import root_sets as R
from octreeraytracer_amd import _lib as L
from root_sets import bits, same_records

pytestmark = pytest.mark.gpu


class Scenes:
    """One context per layout; the scene of (k, kind) is uploaded when it is not the current one."""

    def __init__(self, ort):
        self.ort, self.made, self.current = ort, {}, {}

    def get(self, layout, k, kind):
        if layout not in self.made:
            r = self.ort.Renderer(0)
            if layout == L.ORT_LAYOUT_EXPLICIT:
                r.set_layout(L.ORT_LAYOUT_EXPLICIT)
            self.made[layout] = r
        r = self.made[layout]
        if self.current.get(layout) != (k, kind):
            r.upload(*R.scene(k, kind))
            self.current[layout] = (k, kind)
            assert r.info()["layout"] == ("explicit" if layout == L.ORT_LAYOUT_EXPLICIT else "compact")
        return r

    def close(self):
        for r in self.made.values():
            r.close()


@pytest.fixture(scope="module")
def scenes(ort):
    sc = Scenes(ort)
    yield sc
    sc.close()


def check_family(ort, oracle, scenes, name, kind, layout, use_octree, **kw):
    """Every part of the family on its scene against the oracle's records.  Returns the records."""
    out = []
    for (k, rays), ref in zip(R.parts(name, kind), R.oracle_records(name, kind)):
        r = scenes.get(layout, k, kind)
        got = r.trace_rays(np.array(rays), use_octree=use_octree, normals=True, **kw)
        R.check_records(ort, oracle, R.scene(k, kind)[0], rays, ref, got, (name, kind, layout, use_octree, k, kw))
        out.append(got)
    return out


@pytest.mark.parametrize("name", R.ONE_SPHERE)
def test_brute_force_is_sphere_hit_fast(ort, oracle, scenes, name):
    """One sphere, use_octree=False: one sphere_hit_fast per ray."""
    check_family(ort, oracle, scenes, name, "one", L.ORT_LAYOUT_COMPACT, False)


@pytest.mark.parametrize("name", R.ONE_SPHERE)
def test_root_leaf(ort, oracle, scenes, name):
    """The same sphere as a depth-0 tree, compact layout; in coherence order too."""
    plain = check_family(ort, oracle, scenes, name, "one", L.ORT_LAYOUT_COMPACT, True)
    sorted_ = check_family(ort, oracle, scenes, name, "one", L.ORT_LAYOUT_COMPACT, True, sort=True)
    assert all(same_records(a, b) for a, b in zip(plain, sorted_))


@pytest.mark.parametrize("name", R.ONE_SPHERE)
def test_inline_leaves(ort, oracle, scenes, name):
    """The nine-sphere tree: the target in one-sphere leaf children (inline leaf records, kid skip)."""
    assert check_family(ort, oracle, scenes, name, "inline", L.ORT_LAYOUT_COMPACT, True)


@pytest.mark.parametrize("kind", ["one", "inline"])
@pytest.mark.parametrize("name", R.ONE_SPHERE)
def test_explicit_layout(ort, oracle, scenes, name, kind):
    """The exact sphere_hit_t on the device (IEEE division and sqrtf): the same records."""
    check_family(ort, oracle, scenes, name, kind, L.ORT_LAYOUT_EXPLICIT, True)


@pytest.mark.parametrize("kind", ["one", "inline"])
@pytest.mark.parametrize("name", R.ONE_SPHERE)
def test_options_leave_the_records_alone(ort, oracle, name, kind):
    """ORT_OPT_EXACT_TRAVERSAL 0 / 1 and ORT_OPT_KID_SKIP 0 / 1 / 2: the oracle's records under each."""
    with ort.Renderer(0) as r:
        for (k, rays), ref in zip(R.parts(name, kind), R.oracle_records(name, kind)):
            s, t = R.scene(k, kind)
            r.upload(s, t)
            rays = np.array(rays)
            for exact in (False, True):
                r.set_exact_traversal(exact)
                for skip in (0, 1, 2):
                    r.set_kid_skip(skip)
                    got = r.trace_rays(rays, normals=True)
                    R.check_records(ort, oracle, s, rays, ref, got, (name, kind, k, "exact", exact, "kid skip", skip))


@pytest.mark.parametrize("config", ["brute", "root_leaf", "inline"])
def test_mixed_waves(ort, oracle, scenes, config):
    """Waves in which 16 lanes fail a_in_qdiv_range: the in-range rays' records are those of the same
    rays alone in whole waves (where the wave-uniform guards pass), and both are the oracle's."""
    kind = "inline" if config == "inline" else "one"
    use_octree = config != "brute"
    rays, idx = R.mixed()
    ref, = R.oracle_records("mixed", kind)
    r = scenes.get(L.ORT_LAYOUT_COMPACT, 0, kind)
    s = R.scene(0, kind)[0]
    both = r.trace_rays(np.array(rays), use_octree=use_octree, normals=True)
    R.check_records(ort, oracle, s, rays, ref, both, ("mixed", config))
    alone_rays = np.ascontiguousarray(rays[idx])
    assert len(alone_rays) % R.WAVE == 0
    alone = r.trace_rays(alone_rays, use_octree=use_octree, normals=True)
    R.check_records(ort, oracle, s, alone_rays, ref[idx], alone, ("mixed alone", config))
    assert same_records(alone, [a[idx] for a in both])
    assert (alone[1] >= 0).sum() >= 1000


@pytest.mark.parametrize("variant", ["compact", "compact_sorted", "explicit", "exact_traversal"])
def test_ties(ort, scenes, variant):
    """Rays through node corners and edges of the compact5 tree (slab values bit-equal on three or two
    axes): the oracle's hit flag and t, the emulation's sphere and normals."""
    s, t, _ = ray_sets.scene("compact5")
    rays = np.array(R.ties()[0])
    ref, = R.oracle_records("ties", "tree")
    with ort.Renderer(0) as r:
        if variant == "explicit":
            r.set_layout(L.ORT_LAYOUT_EXPLICIT)
        r.upload(s, t)
        if variant == "exact_traversal":
            r.set_exact_traversal(True)
        got = r.trace_rays(rays, sort=variant == "compact_sorted", normals=True)
    R.check_records(ort, None, s, rays, ref, got, ("ties", variant), spheres=False)
    assert same_records(got, R.ties_emulated())
    assert (got[1] >= 0).sum() >= 256


@pytest.mark.parametrize("use_octree", [True, False])
def test_ties_nearest(ort, use_octree):
    """trace_rays_ex NEAREST over the tie rays against ray_mode_sets' every-sphere reference."""
    s, t, _ = ray_sets.scene("compact5")
    rays = np.array(R.ties()[0])
    yt, ys = R.ties_nearest()
    with ort.Renderer(0) as r:
        r.upload(s, t)
        tt, sph, nrm = r.trace_rays(rays, use_octree=use_octree, normals=True, mode="nearest")
    bad = np.nonzero((bits(tt) != bits(yt)) | (sph != ys))[0]
    assert bad.size == 0, (bad[:8], tt[bad[:8]], yt[bad[:8]], sph[bad[:8]], ys[bad[:8]])
    assert np.array_equal(bits(nrm), bits(ray_sets.numpy_normals(s, rays, yt, ys)))


def test_device_pointers_on_a_stream(ort, oracle, scenes):
    """tmin_far with rays, records and normals as device pointers, ordered on a torch stream."""
    import torch
    (k, rays), = R.family("tmin_far")
    ref, = R.oracle_records("tmin_far", "one")
    n = len(rays)
    r = scenes.get(L.ORT_LAYOUT_COMPACT, 0, "one")
    d_rays = torch.from_numpy(np.array(rays)).to("cuda:0")
    out = torch.full((n + 1, 2), -7, dtype=torch.int32, device="cuda:0")
    nrm = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device="cuda:0")
    st = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    for use_octree in (False, True):
        r.trace_rays(d_rays.data_ptr(), n=n, use_octree=use_octree, out=out.data_ptr(), normals=nrm.data_ptr(),
                     stream=st.cuda_stream)
        st.synchronize()
        o, nr = out.cpu().numpy(), nrm.cpu().numpy()
        assert (o[n:] == -7).all() and (nr[n:] == -7.0).all()  # nothing written past the records
        got = (np.ascontiguousarray(o[:n, 0]).view(np.float32), np.ascontiguousarray(o[:n, 1]), np.ascontiguousarray(nr[:n]))
        R.check_records(ort, oracle, R.scene(0, "one")[0], rays, ref, got, ("pointers", use_octree))


@pytest.mark.parametrize("config", ["brute", "root_leaf", "inline"])
def test_radiance_reaches_the_same_sphere_test(ort, scenes, config):
    """trace_radiance (the whole-pixel kernels' copy of the sphere test), paths 1, depth 2, over
    tmin_near + graze: the host emulation's radiance bit for bit (two NaNs in one place are equal)."""
    kind = "inline" if config == "inline" else "one"
    use_octree = config != "brute"
    rays, states = R.radiance_set()
    want = R.radiance_emulated(kind, use_octree)
    r = scenes.get(L.ORT_LAYOUT_COMPACT, 0, kind)
    got = r.trace_radiance(np.array(rays), np.array(states), max_depth=2, paths=1, use_octree=use_octree)
    bad = np.nonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
    assert bad.size == 0, (config, int(bad.size), bad[:5], got[bad[:3]], want[bad[:3]])
