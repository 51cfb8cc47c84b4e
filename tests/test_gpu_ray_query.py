"""Ray queries on the GPU (ort_trace_rays, include/ort.h): the records of the ray set of
tests/ray_sets.py equal the independent oracle's intersectScene bit for bit, and the host
emulation's (tests/test_ray_query.py) in sphere index and normal, on every walk: the persistent
fast walk with its deferred exact walk (compact layout, depth 5, 6 and 10), the explicit layout's
stack walk and brute force.  Every comparison is exact."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ray_sets
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import query_rays_host
from test_ray_query import CONFIGS, bits, emulate

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def make_renderer(ort, name):
    s, t, _ = ray_sets.scene(name)
    layout, use_octree = CONFIGS[name]
    r = ort.Renderer(0)
    if layout == L.ORT_LAYOUT_EXPLICIT:
        r.set_layout(L.ORT_LAYOUT_EXPLICIT)
    r.upload(s, t)
    assert r.info()["layout"] == ("explicit" if layout == L.ORT_LAYOUT_EXPLICIT else "compact")
    return r


@pytest.fixture(scope="module")
def renderers(ort):
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_renderer(ort, name)
        return made[name]

    yield get
    for r in made.values():
        r.close()


@pytest.fixture(scope="module")
def full(renderers):
    """name -> the 3001-ray result (t, sphere, normals) of the plain host call (read-only)."""
    done = {}

    def get(name):
        if name not in done:
            _, _, rays = ray_sets.scene(name)
            res = renderers(name).trace_rays(rays, use_octree=CONFIGS[name][1], normals=True)
            for a in res:
                a.flags.writeable = False
            done[name] = res
        return done[name]

    return get


def same_records(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_records_equal_the_oracle_and_the_emulation(ort, oracle, full, name):
    s, _, rays = ray_sets.scene(name)
    ref = ray_sets.oracle_hits(name)
    tt, sph, nrm = full(name)
    hit = sph >= 0
    assert np.array_equal(hit, ref[:, 0] == 1)
    assert np.array_equal(bits(tt)[hit], ref[hit, 1])
    assert (bits(tt)[~hit] == 0).all() and (sph[~hit] == -1).all() and (bits(nrm)[~hit] == 0).all()
    ray_sets.assert_hit_floors(hit)
    et, es, en = emulate(name)
    assert np.array_equal(sph, es) and np.array_equal(bits(tt), bits(et)) and np.array_equal(bits(nrm), bits(en))
    if name == "brute":
        assert np.array_equal(sph, ref[:, 2])


@pytest.mark.parametrize("name", ["compact5", "compact10", "explicit", "brute"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 129])
def test_prefixes(renderers, full, name, n):
    _, _, rays = ray_sets.scene(name)
    got = renderers(name).trace_rays(np.ascontiguousarray(rays[:n]), use_octree=CONFIGS[name][1], normals=True)
    assert got[0].shape == (n,) and got[1].shape == (n,) and got[2].shape == (n, 3)
    assert same_records(got, [a[:n] for a in full(name)])


@pytest.mark.parametrize("name", ["compact5", "compact10", "explicit", "brute"])
def test_without_normals_and_into_out(renderers, full, name):
    _, _, rays = ray_sets.scene(name)
    out = np.full((len(rays) + 3, 2), 0x5A5A5A5A, np.int32)
    tt, sph = renderers(name).trace_rays(rays, use_octree=CONFIGS[name][1], out=out)
    assert same_records((tt, sph), full(name)[:2])
    assert np.array_equal(out[:len(rays), 0], bits(tt)) and np.array_equal(out[:len(rays), 1], sph)
    assert (out[len(rays):] == 0x5A5A5A5A).all()  # nothing written past the records


@pytest.mark.parametrize("name", ["compact5", "compact10", "explicit", "brute"])
@pytest.mark.parametrize("sort", [False, True])
def test_device_in_out_and_streams(renderers, full, name, sort):
    """Torch tensors in and out equal host in and out; a stream-ordered call on a torch stream,
    then a synchronise, gives the same; so does a raw-pointer call."""
    import torch
    _, _, rays = ray_sets.scene(name)
    r, use_octree = renderers(name), CONFIGS[name][1]
    want = full(name)
    d_rays = torch.from_numpy(np.array(rays)).to("cuda:0")
    torch.cuda.synchronize()

    def check(out, nrm, what):
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[:, 0], bits(want[0])) and np.array_equal(o[:, 1], want[1]), what
        if nrm is not None:
            assert np.array_equal(bits(nrm.cpu().numpy()), bits(want[2])), what

    out, nrm = r.trace_rays(d_rays, use_octree=use_octree, sort=sort, normals=True)
    assert out.shape == (len(rays), 2) and out.dtype == torch.int32 and nrm.shape == (len(rays), 3)
    check(out, nrm, "device")
    out2 = r.trace_rays(d_rays, use_octree=use_octree, sort=sort)
    check(out2, None, "device, no normals")
    st = torch.cuda.Stream(device="cuda:0")
    out3 = torch.full((len(rays), 2), -7, dtype=torch.int32, device="cuda:0")
    nrm3 = torch.full((len(rays), 3), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    got = r.trace_rays(d_rays, use_octree=use_octree, sort=sort, normals=nrm3, out=out3, stream=st.cuda_stream)
    assert got[0] is out3 and got[1] is nrm3
    st.synchronize()
    check(out3, nrm3, "stream-ordered")
    out4 = torch.full((len(rays), 2), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    r.trace_rays(d_rays.data_ptr(), n=len(rays), use_octree=use_octree, sort=sort, out=out4.data_ptr())
    check(out4, None, "pointers")
    assert r.last_query_ms() > 0.0


@pytest.mark.parametrize("name", ["compact5", "compact10", "compact6"])
def test_sort_gives_the_same_records_in_the_same_order(renderers, full, name):
    _, _, rays = ray_sets.scene(name)
    got = renderers(name).trace_rays(rays, sort=True, normals=True)
    assert same_records(got, full(name))
    # and on a prefix that is no multiple of anything
    got = renderers(name).trace_rays(np.ascontiguousarray(rays[:1031]), sort=True, normals=True)
    assert same_records(got, [a[:1031] for a in full(name)])


@pytest.mark.parametrize("name", ["compact5", "compact10"])
@pytest.mark.parametrize("sort", [False, True])
def test_more_rays_than_the_resident_waves_take_singly(renderers, full, name, sort):
    """2^23 + 1 rays: at least ORT_CHUNK_ADAPT (1024) items per resident wave on any grid (at most
    6 waves/SIMD x 4 SIMDs x 256 CUs = 6144 waves), so the persistent loop draws its doubled
    chunks.  The 3001-ray set tiled on the device; every record equals the tiled 3001-ray record."""
    import torch
    _, _, rays = ray_sets.scene(name)
    n = (1 << 23) + 1
    idx = torch.arange(n, device="cuda:0") % len(rays)
    d_rays = torch.from_numpy(np.array(rays)).to("cuda:0")[idx].contiguous()
    tt, sph, nrm = full(name)
    want = torch.from_numpy(np.stack([bits(tt).view(np.int32), sph.astype(np.int32)], axis=1)).to("cuda:0")[idx]
    want_nrm = torch.from_numpy(np.array(bits(nrm))).to("cuda:0")[idx]
    out, got_nrm = renderers(name).trace_rays(d_rays, sort=sort, normals=True)
    torch.cuda.synchronize()
    assert out.shape == (n, 2) and got_nrm.shape == (n, 3)
    assert torch.equal(out, want)
    assert torch.equal(got_nrm.view(torch.int32), want_nrm)


@pytest.mark.parametrize("name", ["compact5", "compact10"])
def test_options_leave_the_records_alone(ort, full, name):
    """ORT_OPT_KID_SKIP 0 / 1 / 2, ORT_OPT_EXACT_TRAVERSAL 1 and ORT_OPT_REFILL: same records."""
    s, t, rays = ray_sets.scene(name)
    want = full(name)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        for skip in (0, 2, 1):
            r.set_kid_skip(skip)
            assert same_records(r.trace_rays(rays, normals=True), want), f"kid skip {skip}"
        for refill in (1, 64, 16):
            r.set_refill(refill)
            assert same_records(r.trace_rays(rays, normals=True), want), f"refill {refill}"
        r.set_exact_traversal(True)
        assert same_records(r.trace_rays(rays, normals=True), want), "exact traversal"
        assert same_records(r.trace_rays(rays, sort=True, normals=True), want), "exact traversal, sorted"


@pytest.mark.parametrize("ns,depth", [(1, 1), (2, 4)])
def test_render_query_render(ort, scene_c1, ns, depth):
    """A query between two frames changes neither: both equal the frame of a context that never
    queried; and the query repeated gives the same records."""
    s, t = scene_c1
    p = ort.FrameParams.default_camera(4, 8, num_samples=ns, max_depth=depth)
    _, _, rays = ray_sets.scene("explicit")  # (the same 100 spheres and tree as scene_c1)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        plain = r.render(p)
        plain2 = r.render(p)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        a = r.render(p)
        q1 = r.trace_rays(rays, normals=True)
        q1s = r.trace_rays(rays, normals=True, sort=True)
        b = r.render(p)
        q2 = r.trace_rays(rays, normals=True)
        c = r.render(p)
    for f in (plain2, a, b, c):
        assert np.array_equal(f.view(np.uint32), plain.view(np.uint32))
    assert same_records(q1, q2) and same_records(q1, q1s)
    assert (q1[1] >= 0).mean() >= 0.10


@pytest.mark.parametrize("name", list(CONFIGS))
def test_degenerate_rays_miss(renderers, oracle, name):
    """Zero, infinite, NaN and hugely scaled rays: ORT_OK and a miss for each, sorted or not --
    after the host emulation, which runs the same per-ray code, has terminated with all misses."""
    s, t, _ = ray_sets.scene(name)
    rays = ray_sets.degenerate_rays()
    layout, use_octree = CONFIGS[name]
    et, es, en = query_rays_host(s, t if use_octree else None, rays, layout=layout, use_octree=use_octree, normals=True)
    assert (es == -1).all() and (bits(et) == 0).all() and (bits(en) == 0).all()
    for sort in (False, True):
        tt, sph, nrm = renderers(name).trace_rays(rays, use_octree=use_octree, sort=sort, normals=True)
        assert (sph == -1).all() and (bits(tt) == 0).all() and (bits(nrm) == 0).all()


def raw_query(r, rays, hits, n, **kw):
    q = L.OrtRayQuery(rays.ctypes.data_as(C.c_void_p) if rays is not None else None, n,
                      hits.ctypes.data_as(C.c_void_p) if hits is not None else None, None, 0,
                      kw.get("use_octree", 1), kw.get("flags", 0), kw.get("reserved", 0))
    return r._lib.ort_trace_rays(r._ctx, C.byref(q), None)


def test_error_codes(ort):
    s, t, rays = ray_sets.scene("explicit")
    rays = np.array(rays[:16])
    hits = np.full((16, 2), 0x5A5A5A5A, np.int32)
    with ort.Renderer(0) as r:
        assert raw_query(r, rays, hits, 16) == L.ORT_ERR_NO_SCENE
        with pytest.raises(ort.OrtError) as e:
            r.last_query_ms()
        assert e.value.code == L.ORT_ERR_NO_SCENE
        r.upload(s, t)
        assert raw_query(r, rays, hits, 16, reserved=1) == L.ORT_ERR_INVALID_ARG
        assert raw_query(r, rays, hits, 16, flags=2) == L.ORT_ERR_INVALID_ARG
        assert raw_query(r, rays, hits, 16, flags=L.ORT_QUERY_SORT | 4) == L.ORT_ERR_INVALID_ARG
        assert raw_query(r, rays, hits, -1) == L.ORT_ERR_INVALID_ARG
        assert raw_query(r, rays, hits, (1 << 30) + 1) == L.ORT_ERR_INVALID_ARG
        assert raw_query(r, rays, None, 16) == L.ORT_ERR_INVALID_ARG
        assert raw_query(r, None, hits, 16) == L.ORT_ERR_INVALID_ARG
        assert r._lib.ort_trace_rays(r._ctx, None, None) == L.ORT_ERR_INVALID_ARG
        odd = np.zeros(16 * 24 + 4, np.uint8)[1:1 + 16 * 24]  # not 4-byte aligned
        assert odd.ctypes.data % 4 != 0
        assert raw_query(r, odd, hits, 16) == L.ORT_ERR_INVALID_ARG
        assert (hits == 0x5A5A5A5A).all()  # refused before anything was launched
        assert raw_query(r, None, None, 0) == L.ORT_OK  # nothing to do
        assert raw_query(r, rays, hits, 16) == L.ORT_OK
        assert (hits != 0x5A5A5A5A).all()
        r.upload(s, None)  # no tree: the octree walk is refused as ort_render refuses it
        assert raw_query(r, rays, hits, 16) == L.ORT_ERR_NO_SCENE
        with pytest.raises(ort.OrtError) as e:
            r.render(ort.FrameParams.default_camera(8, 8))
        assert e.value.code == L.ORT_ERR_NO_SCENE
        assert raw_query(r, rays, hits, 16, use_octree=0) == L.ORT_OK


def cpp_example_rays():
    """The rays of tests/cpp/trace_rays.cpp, in its float32 arithmetic."""
    f = np.float32
    centres = np.array([[-10, -10, -10], [10, 10, 10], [-10, 10, -10]], f)
    o = [30.0, 20.0, -50.0]
    rows = [o + [(c[0] + f(2.5) * f(i)) - f(30), (c[1] + f(2.5) * f(j)) - f(20), c[2] + f(50)]
            for c in centres for j in (-1, 0, 1) for i in (-1, 0, 1)]
    rows += [o + [0.0, 0.0, -1.0], o + [0.0, 1.0, 0.0], [10.0, 50.0, 10.0, 0.0, -1.0, 0.0]]
    return np.array(rows, np.float32)


@pytest.mark.parametrize("brute", [False, True])
def test_cpp_trace_rays_prints_the_python_records(ort, brute):
    """build/trace_rays (Raytracer::traceRays on the DEBUG scene) against Renderer.trace_rays."""
    exe = ROOT / "build" / "trace_rays"
    assert exe.exists(), "make examples"
    res = subprocess.run([str(exe)] + (["--brute"] if brute else []), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    rows = [l.split()[1:] for l in res.stdout.splitlines() if l.startswith("ray ")]
    rays = cpp_example_rays()
    assert len(rows) == len(rays) == 30
    s = ort.debug_spheres()
    with ort.Renderer(0) as r:
        r.upload(s, ort.build_octree(s, 3, 2))  # RaytracerConfig's debugDepth, debugSpheresPerNode
        tt, sph, nrm = r.trace_rays(rays, use_octree=not brute, normals=True)
    assert (sph >= 0).sum() >= 9 and (sph < 0).sum() >= 2
    for i, row in enumerate(rows):
        assert int(row[0]) == i and int(row[1]) == int(sph[i] >= 0) and int(row[2]) == sph[i], (i, row)
        assert [int(x, 16) for x in row[3:]] == [int(v) for v in np.concatenate([tt[i:i + 1], nrm[i]]).view(np.uint32)], (i, row)
