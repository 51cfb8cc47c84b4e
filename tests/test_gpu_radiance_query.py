"""Radiance queries on the GPU (ort_trace_radiance, include/ort.h): the kernels' records equal the
host emulation's bit for bit (which tests/test_radiance_query.py pins to the oracle's frames) on
every walk variant -- brute force, the deep compact walk, the plain compact walk, the LDS-resident
scene -- under every option, with host and device pointers and a caller's stream; over a frame's
first-sample rays they equal Renderer.render's 1-sample frames; queries leave frames and
accumulations alone; and the entry point's refusals.  Every comparison is exact (two NaNs in the
same place are equal)."""
import ctypes as C

import numpy as np
import pytest

import camera_sets as cs
import radiance_sets as rs
import ray_sets
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import radiance_rays_host, rng_states
from radiance_sets import bits, same
from test_gpu_ray_query import make_renderer

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
COMBOS = [(paths, depth, st) for paths in (1, 5) for depth in (1, 8) for st in (False, True)]
VARIANTS = ("default", "sort", "exact", "kid_skip_0", "kid_skip_2", "lds_scene_0", "device", "stream")


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


def check_combo(name, paths, depth, with_states, rad, st, what=""):
    want, want_st = rs.emulated(name, paths, depth)
    bad = np.nonzero(~((bits(rad) == bits(want)) | (np.isnan(rad) & np.isnan(want))).all(axis=1))[0]
    assert same(rad, want), (name, what, paths, depth, bad[:5], rad[bad[:2]], want[bad[:2]])
    if with_states:
        assert same(st, want_st), (name, what, paths, depth)
    else:
        assert st is None


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", rs.SCENES)
def test_gpu_equals_the_emulation(ort, renderers, name, variant):
    """The 3001 rays and the 12 degenerate ones, paths 1 and 5, depth 1 and 8, states_out on and
    off: the records of the emulation, whatever the option, the pointers or the stream."""
    rays, states = rs.ray_set(name)
    s, t, use_octree = rs.scene(name)
    kw = dict(use_octree=use_octree)
    own = None
    if variant in ("default", "device", "stream"):
        r = renderers(name)
    else:
        r = own = ort.Renderer(0)
        if variant == "exact":
            r.set_exact_traversal(True)
        elif variant.startswith("kid_skip"):
            r.set_kid_skip(int(variant[-1]))
        elif variant == "lds_scene_0":
            r.set_pixel_lds_scene(0)
        elif variant == "sort":
            kw["sort"] = True
        r.upload(s, ray_sets.scene(name)[1])
    try:
        for paths, depth, with_states in COMBOS:
            if variant in ("device", "stream"):
                import torch
                d_rays = torch.from_numpy(np.array(rays)).to("cuda:0")
                d_states = torch.from_numpy(np.array(states)).to("cuda:0")
                out = torch.full((len(rays) + 3, 3), -7.0, dtype=torch.float32, device="cuda:0")
                stream = torch.cuda.Stream(device="cuda:0") if variant == "stream" else None
                torch.cuda.synchronize()
                got = r.trace_radiance(d_rays, d_states, max_depth=depth, paths=paths, states_out=with_states, out=out,
                                       stream=stream.cuda_stream if stream else None, **kw)
                (stream or torch.cuda).synchronize()
                d_out, d_st = got if with_states else (got, None)
                assert d_out is out and (out[len(rays):].cpu().numpy() == -7.0).all()
                assert torch.equal(d_states.cpu(), torch.from_numpy(np.array(states)))  # the input states stay
                check_combo(name, paths, depth, with_states, out[:len(rays)].cpu().numpy(),
                            d_st.cpu().numpy() if with_states else None, variant)
                if with_states:  # in place: states_out is states
                    got = r.trace_radiance(d_rays, d_states, max_depth=depth, paths=paths, states_out=d_states, **kw)
                    torch.cuda.synchronize()
                    assert got[1] is d_states
                    check_combo(name, paths, depth, True, got[0].cpu().numpy(), d_states.cpu().numpy(), variant + " in place")
            else:
                got = r.trace_radiance(rays, states, max_depth=depth, paths=paths, states_out=with_states, **kw)
                rad, st = got if with_states else (got, None)
                check_combo(name, paths, depth, with_states, rad, st, variant)
        if variant == "default":
            alias = np.array(states)
            rad, st = r.trace_radiance(rays, alias, max_depth=8, paths=5, states_out=alias, **kw)
            assert st is alias
            check_combo(name, 5, 8, True, rad, alias, "host in place")
            assert r.last_query_ms() > 0.0
    finally:
        if own is not None:
            own.close()


@pytest.mark.parametrize("lds", [1, 0])
def test_a_small_scene_walks_from_lds(ort, oracle, scene_c1, lds):
    """100 spheres in a depth-4 tree fit the LDS budget (ORT_OPT_PIXEL_LDS_SCENE 1: the LDS-resident
    walk; 0: the plain compact walk): the emulation's records either way, flags included."""
    s, t = scene_c1
    rays = np.ascontiguousarray(np.concatenate([ray_sets.make_rays(ort, oracle, s, t, 5), ray_sets.degenerate_rays()]))
    states = rng_states(len(rays), 11)
    with ort.Renderer(0) as r:
        r.set_pixel_lds_scene(lds)
        r.upload(s, t)
        assert r.info()["layout"] == "compact"
        for kw in (dict(max_depth=8, paths=5), dict(max_depth=1), dict(max_depth=4, paths=2, gamma=True, normalize=True, sort=True)):
            got = r.trace_radiance(rays, states, states_out=True, **kw)
            want = radiance_rays_host(s, t, rays, states, states_out=True, **kw)
            assert same(got[0], want[0]) and same(got[1], want[1]), kw


@pytest.mark.parametrize("name", rs.SCENES)
def test_flags_and_invalid_states(renderers, name):
    rays, states = rs.ray_set(name)
    s, t, use_octree = rs.scene(name)
    r = renderers(name)
    rays, states = np.array(rays[:700]), np.array(states[:700])
    rays[:, 3:] = (rays[:, 3:] * np.float32(3.0)).astype(np.float32)
    for i, c, v in [(3, 0, 1.0), (10, 1, 1.0), (11, 0, -0.25), (64, 1, -0.25), (65, 0, np.nan), (699, 1, np.nan)]:
        states[i, c] = v
    for kw in (dict(normalize=True), dict(gamma=True), dict(normalize=True, gamma=True, sort=True)):
        got = r.trace_radiance(rays, states, max_depth=4, paths=3, states_out=True, use_octree=use_octree, **kw)
        want = rs.emulate(name, rays, states, max_depth=4, paths=3, states_out=True, **kw)
        assert same(got[0], want[0]) and same(got[1], want[1]), kw
        assert (bits(got[0][[3, 10, 11, 64, 65, 699]]) == 0).all()


@pytest.mark.parametrize("name", rs.SCENES)
def test_identity_with_render(ort, renderers, name):
    """A 1-sample frame's pixel is pow(radiance(first-sample ray), 1/2.2) from the six-draw state:
    trace_radiance(gamma) over trace_camera's rays equals Renderer.render of the frame, by the
    whole-pixel kernel and by the pipeline (ORT_OPT_PIXEL_PATHS 1 and 0), at depth 1, 2, 4 and 8."""
    r = renderers(name)
    s, t, use_octree = rs.scene(name)
    try:
        for w, h in rs.FRAMES:
            rays, states = rs.frame_inputs(name, w, h)
            cam = r.trace_camera(cs.params(name, w, h, 1), rays=True, hits=False).reshape(-1, 6)
            assert same(cam, rays)
            for depth in rs.DEPTHS:
                got = r.trace_radiance(rays, states, max_depth=depth, gamma=True, use_octree=use_octree)
                assert same(got, rs.oracle_frame(name, w, h, depth)), (w, h, depth)
                for mode in (1, 0):
                    r.set_pixel_paths(mode)
                    frame = r.render(rs.params(name, w, h, depth)).reshape(-1, 3)
                    assert same(got, frame), (w, h, depth, mode)
    finally:
        r.set_pixel_paths(-1)


@pytest.mark.parametrize("name", rs.SCENES)
def test_more_rays_than_lanes(renderers, name):
    """The ray set tiled 100 times (300,100 rays, depth 8): more rays than the resident grid has
    lanes, so every wave draws several chunks and refills; the records are the single set's, tiled.
    Device-resident."""
    import torch
    rays, states = rs.ray_set(name)
    rays, states = rays[:ray_sets.N_RAYS], states[:ray_sets.N_RAYS]
    s, t, use_octree = rs.scene(name)
    want, want_st = (a[:ray_sets.N_RAYS] for a in rs.emulated(name, 1, 8))
    d_rays = torch.from_numpy(np.array(rays)).to("cuda:0").repeat(100, 1)
    d_states = torch.from_numpy(np.array(states)).to("cuda:0").repeat(100, 1)
    assert d_rays.shape == (300100, 6) and d_rays.is_contiguous()
    for sort in (False, True):
        out, st = renderers(name).trace_radiance(d_rays, d_states, max_depth=8, use_octree=use_octree, states_out=True, sort=sort)
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), np.tile(want, (100, 1))), sort
        assert same(st.cpu().numpy(), np.tile(want_st, (100, 1))), sort


@pytest.mark.parametrize("ns,depth", [(1, 1), (4, 8)])
def test_render_query_render(ort, oracle, scene_c1, ns, depth):
    """A radiance query between two frames changes neither, and the query repeated gives the same
    records; an accumulation stepped around queries finishes as render()'s frame."""
    s, t = scene_c1
    p = ort.FrameParams.default_camera(37, 21, num_samples=ns, max_depth=depth, **cs.CAMERAS["brute"])
    rays = np.ascontiguousarray(ray_sets.make_rays(ort, oracle, s, t, 5)[:1000])
    states = rng_states(1000, 3)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        plain = r.render(p)
        plain2 = r.render(p)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        a = r.render(p)
        q1 = r.trace_radiance(rays, states, max_depth=8, paths=3, states_out=True)
        b = r.render(p)
        q2 = r.trace_radiance(rays, states, max_depth=8, paths=3, states_out=True, sort=True)
        c = r.render(p)
        with r.accumulate(p) as acc:
            acc.step(1)
            q3 = r.trace_radiance(rays, states, max_depth=8, paths=3, states_out=True)
            got = acc.step(ns)
            assert acc.finished
    for f in (plain2, a, b, c, got):
        assert np.array_equal(f.view(np.uint32), plain.view(np.uint32))
    want = radiance_rays_host(s, t, rays, states, max_depth=8, paths=3, states_out=True)
    for q in (q1, q2, q3):
        assert same(q[0], want[0]) and same(q[1], want[1])


def raw(r, rays, states, radiance, states_out=None, n=None, on_device=0, use_octree=1, max_depth=2, paths=1, flags=0,
        reserved=0, null_q=False):
    def ptr(a):
        if a is None or isinstance(a, int):
            return a
        return a.ctypes.data_as(C.c_void_p)
    n = len(rays) if n is None else n
    q = L.OrtRadianceQuery(ptr(rays), n, ptr(states), ptr(radiance), ptr(states_out), on_device, use_octree, max_depth, paths,
                           flags, reserved)
    return r._lib.ort_trace_radiance(r._ctx, None if null_q else C.byref(q), None)


def test_error_codes(ort):
    s, t, all_rays = ray_sets.scene("explicit")
    rays = np.ascontiguousarray(all_rays[:32])
    states = rng_states(32, 1)
    given = states.copy()
    rad = np.full((32, 3), FILL, np.int32)
    out = np.full((40, 2), FILL, np.int32)
    bad = L.ORT_ERR_INVALID_ARG

    def untouched():
        return (rad == FILL).all() and (out == FILL).all() and np.array_equal(bits(states), bits(given))

    with ort.Renderer(0) as r:
        assert raw(r, rays, states, rad, out) == L.ORT_ERR_NO_SCENE
        r.upload(s, t)
        assert r.info()["layout"] == "compact"
        assert raw(r, rays, states, rad, out, null_q=True) == bad
        assert raw(r, rays, states, rad, out, n=-1) == bad
        assert raw(r, rays, states, rad, out, n=(1 << 30) + 1) == bad
        assert raw(r, None, states, rad, out, n=32) == bad
        assert raw(r, rays, None, rad, out) == bad
        assert raw(r, rays, states, None, out) == bad
        assert raw(r, rays, states, rad, out, max_depth=0) == bad
        assert raw(r, rays, states, rad, out, max_depth=-3) == bad
        assert raw(r, rays, states, rad, out, paths=0) == bad
        assert raw(r, rays, states, rad, out, paths=65537) == bad
        assert raw(r, rays, states, rad, out, flags=8) == bad
        assert raw(r, rays, states, rad, out, flags=-1) == bad
        assert raw(r, rays, states, rad, out, reserved=1) == bad
        both = np.zeros((40, 2), np.float32)  # states_out overlapping states without being equal to it
        assert raw(r, rays, both[:32], rad, both[4:36]) == bad
        assert raw(r, rays, both[4:36], rad, both[:32]) == bad
        for k in range(4):  # each pointer misaligned in turn
            odd = np.zeros(32 * 24 + 4, np.uint8)[1:1 + 32 * 24]
            assert odd.ctypes.data % 4 != 0
            args = [rays, states, rad, out]
            args[k] = odd
            assert raw(r, *args) == bad
        assert untouched()
        assert raw(r, rays, states, rad, out, n=0) == L.ORT_OK and untouched()      # nothing to do
        assert raw(r, None, None, None, None, n=0) == L.ORT_OK
        assert raw(r, rays, states, rad, out, paths=65536, max_depth=1, n=1) == L.ORT_OK
        assert (rad[0] != FILL).all() and (rad[1:] == FILL).all() and (out[1:] == FILL).all()
        r.upload(s, None)  # no tree: the octree walk is refused, brute force works
        rad[:] = FILL
        out[:] = FILL
        assert raw(r, rays, states, rad, out) == L.ORT_ERR_NO_SCENE and untouched()
        assert raw(r, rays, states, rad, out, use_octree=0) == L.ORT_OK
        assert (rad != FILL).all() and (out[:32] != FILL).all() and (out[32:] == FILL).all()
    with ort.Renderer(0) as r:  # the explicit layout: no whole-pixel walk; brute force works
        r.set_layout(L.ORT_LAYOUT_EXPLICIT)
        r.upload(s, t)
        assert r.info()["layout"] == "explicit"
        rad[:] = FILL
        out[:] = FILL
        assert raw(r, rays, states, rad, out) == L.ORT_ERR_UNSUPPORTED and untouched()
        assert "explicit layout" in r._lib.ort_last_error(r._ctx).decode()
        with pytest.raises(ort.OrtError) as e:
            r.trace_radiance(rays, states, max_depth=2)
        assert e.value.code == L.ORT_ERR_UNSUPPORTED
        got = r.trace_radiance(rays, states, max_depth=8, paths=2, use_octree=False)
        assert same(got, radiance_rays_host(s, None, rays, states, max_depth=8, paths=2, use_octree=False))
