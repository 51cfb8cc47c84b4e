"""Ray queries (ort_trace_rays) without a GPU: the kernels' per-ray function (render_core.h
query_ray) compiled for the host (ort_debug_query_rays, analysis library) against the independent
oracle's intersectScene on the ray set of tests/ray_sets.py, and the bindings' early checks.
The GPU runs the same source (tests/test_gpu_ray_query.py)."""
import ctypes

import numpy as np
import pytest

import ray_sets
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import query_rays_host

CONFIGS = {  # name -> (layout, use_octree)
    "compact5": (L.ORT_LAYOUT_COMPACT, True),
    "compact10": (L.ORT_LAYOUT_COMPACT, True),
    "compact6": (L.ORT_LAYOUT_COMPACT, True),
    "explicit": (L.ORT_LAYOUT_EXPLICIT, True),
    "brute": (L.ORT_LAYOUT_COMPACT, False),
}


def emulate(name, rays=None, normals=True):
    s, t, base = ray_sets.scene(name)
    layout, use_octree = CONFIGS[name]
    return query_rays_host(s, t if use_octree else None, base if rays is None else rays, layout=layout,
                           use_octree=use_octree, normals=normals)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_emulation_equals_the_oracle(ort, oracle, name):
    """Hit flag and t bits of every ray equal the oracle's; a miss is {0.0, -1, zeros}; the sphere
    index is the one whose one-sphere scene the oracle hits at the same t; the normals equal the
    float32 restatement bit for bit; the hit shares stay above the floors."""
    s, t, rays = ray_sets.scene(name)
    ref = ray_sets.oracle_hits(name)
    tt, sph, nrm = emulate(name)
    hit = sph >= 0
    assert np.array_equal(hit, ref[:, 0] == 1)
    assert np.array_equal(bits(tt)[hit], ref[hit, 1])
    assert (bits(tt)[~hit] == 0).all() and (sph[~hit] == -1).all()
    ray_sets.assert_hit_floors(hit)
    if name == "brute":
        assert np.array_equal(sph, ref[:, 2])  # the nearest sphere, the lowest index among equals
    ray_sets.check_spheres_against_the_oracle(ort, oracle, s, rays, bits(tt), sph)
    assert np.array_equal(bits(nrm), bits(ray_sets.numpy_normals(s, rays, tt, sph)))
    assert (bits(nrm)[~hit] == 0).all()
    t2, s2 = emulate(name, normals=False)
    assert np.array_equal(bits(t2), bits(tt)) and np.array_equal(s2, sph)


@pytest.mark.parametrize("name", ["compact5", "compact10", "compact6"])
def test_part_of_the_set_takes_the_exact_walk(ort, name):
    """Between 0.05 and 0.95 of the set is refused by fast_prepare (the kernels defer it to the
    exact walk): both walks are exercised -- and agree, entry and t bits, where the fast one runs."""
    from test_emulation import _trace_rays
    s, t, rays = ray_sets.scene(name)
    out = _trace_rays(ort, s, t, rays, 1)
    fast = out[:, 0] == 1
    assert 0.05 <= 1.0 - fast.mean() <= 0.95, fast.mean()
    sl = ray_sets.class_slices()
    assert fast[sl["scaled"]].mean() < 0.5 and fast[sl["inside"]].all()
    agree = (out[:, 1] == out[:, 3]) & ((out[:, 1] < 0) | (out[:, 2] == out[:, 4]))
    assert agree[fast].all()
    # the emulated query reports the sphere of that entry
    tt, sph = emulate(name, normals=False)
    assert np.array_equal(sph >= 0, out[:, 3] >= 0)
    assert np.array_equal(bits(tt)[sph >= 0], out[sph >= 0, 4])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_degenerate_rays_terminate_and_miss(oracle, name):
    """Zero, infinite and NaN directions and origins, directions of length 1e-30 and 1e+-20: the
    oracle and the emulation terminate and report a miss for each."""
    s, t, _ = ray_sets.scene(name)
    rays = ray_sets.degenerate_rays()
    assert rays.shape == (12, 6)
    if name != "brute":
        assert (oracle.trace_rays(s, t, rays)[:, 0] == 0).all()
    assert (s.center_radius[:, :3].max() + s.center_radius[:, 3].max()) < 1000.0  # (the two far rays point away)
    tt, sph, nrm = emulate(name, rays)
    assert (sph == -1).all() and (bits(tt) == 0).all() and (bits(nrm) == 0).all()


def test_struct_sizes_match_the_header():
    assert ctypes.sizeof(L.OrtRay) == 24
    assert ctypes.sizeof(L.OrtRayHit) == 8
    assert ctypes.sizeof(L.OrtRayQuery) == 48
    assert L.ORT_QUERY_SORT == 1


def contextless_renderer(ort):
    r = object.__new__(ort.Renderer)  # no GPU context needed: the checks come first
    r._ctx = ctypes.c_void_p()
    r._lib = None
    r.device = 0
    return r


@pytest.mark.parametrize("bad", ["float64", "shape5", "flat", "strided", "short_out", "out_dtype", "n_mismatch",
                                 "normals_array"])
def test_trace_rays_rejects_bad_arguments_before_the_abi(ort, bad):
    """Renderer.trace_rays checks dtype, shape, contiguity and the size of `out` with ValueError
    before anything reaches ort_trace_rays (a wrong buffer would be overrun)."""
    r = contextless_renderer(ort)
    rays = np.zeros((10, 6), np.float32)
    kw = {}
    if bad == "float64":
        rays = np.zeros((10, 6), np.float64)
    elif bad == "shape5":
        rays = np.zeros((10, 5), np.float32)
    elif bad == "flat":
        rays = np.zeros(60, np.float32)
    elif bad == "strided":
        rays = np.zeros((10, 12), np.float32)[:, ::2]
    elif bad == "short_out":
        kw["out"] = np.zeros((9, 2), np.int32)
    elif bad == "out_dtype":
        kw["out"] = np.zeros((10, 2), np.float32)
    elif bad == "n_mismatch":
        kw["n"] = 11
    elif bad == "normals_array":
        kw["normals"] = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError):
        r.trace_rays(rays, **kw)


@pytest.mark.parametrize("bad", ["no_n", "no_out", "normals_true", "list"])
def test_trace_rays_rejects_bad_device_arguments_before_the_abi(ort, bad):
    r = contextless_renderer(ort)
    with pytest.raises(ValueError):
        if bad == "no_n":
            r.trace_rays(4096, out=8192)
        elif bad == "no_out":
            r.trace_rays(4096, n=4)
        elif bad == "normals_true":
            r.trace_rays(4096, n=4, out=8192, normals=True)
        else:
            r.trace_rays([[0.0] * 6], n=1, out=8192)


def test_debug_entry_point_is_in_the_analysis_library_only(ort):
    assert hasattr(L.analysis_lib(), "ort_debug_query_rays")
    assert not hasattr(ort.lib(), "ort_debug_query_rays")
    for name in ("ort_trace_rays", "ort_last_query_ms"):
        assert hasattr(ort.lib(), name) and name in L.EXPORTED_SYMBOLS
