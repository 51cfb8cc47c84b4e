"""Radiance queries on the CPU (ort_debug_radiance_rays, the host emulation of ort_trace_radiance):
over a 1-sample frame's first-sample rays and six-draw RNG states the emulation equals the
oracle's frame bit for bit; chains of paths equal single paths chained through states_out; the
flags, the invalid states, the degenerate rays and the sky; the binding's checks.  Every
comparison is exact (two NaNs in the same place are equal)."""
import ctypes as C

import numpy as np
import pytest

import camera_sets as cs
import radiance_sets as rs
import ray_sets
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import rng_states
from radiance_sets import bits, same
from test_ray_query import contextless_renderer

F = np.float32


@pytest.mark.parametrize("w,h", rs.FRAMES)
@pytest.mark.parametrize("name", rs.SCENES)
def test_the_oracles_frames_are_worth_comparing(name, w, h):
    """The deeper bounces change the oracle's own frames: depth 2 differs from depth 1 in >= 0.25
    of the pixels, 4 from 2 in >= 0.10, 8 from 4 in >= 0.01, and no pixel is NaN (measured:
    0.30-0.63, 0.15-0.27, 0.014-0.049)."""
    f = {d: rs.oracle_frame(name, w, h, d) for d in rs.DEPTHS}
    for d in rs.DEPTHS:
        assert not np.isnan(f[d]).any()

    def differ(a, b):
        return float((bits(f[a]) != bits(f[b])).any(axis=1).mean())

    shares = (differ(2, 1), differ(4, 2), differ(8, 4))
    print(name, (w, h), "pixels that differ: depth 2/1 %.3f, 4/2 %.3f, 8/4 %.3f" % shares)
    assert shares[0] >= 0.25 and shares[1] >= 0.10 and shares[2] >= 0.01, shares


@pytest.mark.parametrize("depth", rs.DEPTHS)
@pytest.mark.parametrize("w,h", rs.FRAMES)
@pytest.mark.parametrize("name", rs.SCENES)
def test_identity_with_the_reference(name, w, h, depth):
    """radiance(first-sample ray) from the six-draw state, through pow(x, 1/2.2), is the 1-sample
    frame's pixel: with gamma the emulation equals oracle.render; without it oracle_pow of the
    result does."""
    rays, states = rs.frame_inputs(name, w, h)
    want = rs.oracle_frame(name, w, h, depth)
    got = rs.emulate(name, rays, states, max_depth=depth, gamma=True)
    assert same(got, want), np.nonzero((bits(got) != bits(want)).any(axis=1))[0][:5]
    lin = rs.emulate(name, rays, states, max_depth=depth)
    assert same(rs.oracle_pow(lin, F(1.0) / F(2.2)), want)
    assert not same(lin, want)


def test_the_restated_state_continues_the_sequence(oracle):
    """Draws 7..9 of a pixel's sequence equal draws 1..3 from the restated six-draw state."""
    _, states = rs.frame_inputs("compact5", 37, 21)
    for x, y in ((0, 0), (36, 20), (17, 3)):
        sx, sy = F(F(F(x) + F(0.5)) / F(37)), F(F(F(y) + F(0.5)) / F(21))
        full = oracle.rand_sequence(float(sx), float(sy), 9)
        st = states[y * 37 + x]
        assert np.array_equal(bits(oracle.rand_sequence(float(st[0]), float(st[1]), 3)), bits(full[6:]))


@pytest.mark.parametrize("name", rs.SCENES)
def test_paths_are_single_paths_chained(name):
    """paths = 5 equals five paths = 1 calls chained through states_out, their radiance summed in
    order in float32 and divided by 5; states_out equal; states_out aliased to states the same."""
    rays, states = rs.ray_set(name)
    rays, states = rays[:ray_sets.N_RAYS], states[:ray_sets.N_RAYS]
    assert np.array_equal(states, rng_states(3013, 7)[:3001])
    rad5, st5 = rs.emulated(name, 5, 8)
    rad5, st5 = rad5[:3001], st5[:3001]
    st = states
    col = np.zeros((3001, 3), F)
    with np.errstate(all="ignore"):
        for _ in range(5):
            c, st = rs.emulate(name, rays, st, max_depth=8, states_out=True)
            col = (col + c).astype(F)
        mean = (col / F(5.0)).astype(F)
    assert same(mean, rad5) and same(st, st5)
    assert not same(st5, states)
    alias = states.copy()
    rad, out = rs.emulate(name, rays, alias, max_depth=8, paths=5, states_out=alias)
    assert out is alias and same(rad, rad5) and same(alias, st5)
    finite = np.isfinite(rad5).all(axis=1)
    assert finite.mean() > 0.8 and (rad5[finite] > 0).any()


@pytest.mark.parametrize("name", rs.SCENES)
def test_normalize_is_the_shaders(name):
    rays, states = rs.ray_set(name)
    rays, states = rays[:500], states[:500]
    scaled = rays.copy()
    scaled[:, 3:] = (rays[:, 3:] * F(3.0)).astype(F)
    unit = scaled.copy()
    with np.errstate(all="ignore"):
        for i in range(len(unit)):
            unit[i, 3:] = cs._norm(scaled[i, 3:])
    got = rs.emulate(name, scaled, states, max_depth=4, paths=2, normalize=True, states_out=True)
    want = rs.emulate(name, unit, states, max_depth=4, paths=2, states_out=True)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert not same(got[0], rs.emulate(name, scaled, states, max_depth=4, paths=2))


@pytest.mark.parametrize("name", rs.SCENES)
def test_an_invalid_state_is_not_traced(name):
    """A component of 1.0, -0.25 or NaN: zeros, and the state echoed back; the rays between them
    are traced as ever."""
    rays, states = rs.ray_set(name)
    rays, states = rays[:64], states[:64].copy()
    want, want_st = rs.emulate(name, rays, states, max_depth=4, paths=3, states_out=True)
    cases = [(3, 0, 1.0), (10, 1, 1.0), (11, 0, -0.25), (40, 1, -0.25), (41, 0, np.nan), (63, 1, np.nan)]
    for i, c, v in cases:
        states[i, c] = v
    got, got_st = rs.emulate(name, rays, states, max_depth=4, paths=3, gamma=False, states_out=True)
    bad = np.array([i for i, _, _ in cases])
    ok = np.setdiff1d(np.arange(64), bad)
    assert (bits(got[bad]) == 0).all() and same(got_st[bad], states[bad])
    assert same(got[ok], want[ok]) and same(got_st[ok], want_st[ok])
    g = rs.emulate(name, rays, states, max_depth=4, paths=3, gamma=True)
    assert (bits(g[bad]) == 0).all()
    states[:] = np.nextafter(F(1.0), F(0.0))  # the largest valid component
    states[:, 0] = 0.0
    traced = rs.emulate(name, rays, states, max_depth=1)
    assert (traced != 0).any(axis=1).mean() > 0.5


@pytest.mark.parametrize("name", rs.SCENES)
def test_degenerate_rays_terminate(name):
    rays, states = rs.ray_set(name)
    rad, st = rs.emulated(name, 5, 8)
    assert rad.shape == (3013, 3) and st.shape == (3013, 2)
    one, st1 = rs.emulated(name, 1, 1)
    # the ray of direction zero misses and sees the sky's horizon: t = 0.5 (0 + 1)
    assert same(one[3001], rs.numpy_sky(F(0.0)))
    assert same(st1[3001], states[3001])  # a miss draws nothing


@pytest.mark.parametrize("name", rs.SCENES)
def test_a_miss_at_depth_one_is_the_sky(name):
    rays, states = rs.ray_set(name)
    sl = ray_sets.class_slices()["outside"]
    rad, st = rs.emulated(name, 1, 1)
    sky = rs.numpy_sky(rays[sl, 4])
    assert same(rad[sl], sky) and same(st[sl], states[sl])
    assert len(np.unique(bits(sky[:, 0]))) > 100


def test_struct_and_symbols(ort):
    assert C.sizeof(L.OrtRadianceQuery) == 64
    assert (L.ORT_QUERY_SORT, L.ORT_RADIANCE_NORMALIZE, L.ORT_RADIANCE_GAMMA) == (1, 2, 4)
    assert hasattr(L.analysis_lib(), "ort_debug_radiance_rays")
    assert not hasattr(ort.lib(), "ort_debug_radiance_rays")
    assert hasattr(ort.lib(), "ort_trace_radiance") and "ort_trace_radiance" in L.EXPORTED_SYMBOLS


def test_rng_states():
    a = rng_states(1000, 3)
    assert a.shape == (1000, 2) and a.dtype == np.float32 and (a >= 0).all() and (a < 1).all()
    assert np.array_equal(a, rng_states(1000, 3)) and not np.array_equal(a, rng_states(1000, 4))
    assert np.array_equal(rng_states(5), rng_states(5, 0)) and rng_states(0).shape == (0, 2)


def test_the_emulation_refuses_what_the_entry_point_refuses(ort):
    s, t, _ = rs.scene("compact5")
    rays, states = (a[:4] for a in rs.ray_set("compact5"))
    from octreeraytracer_amd.renderer import radiance_rays_host
    for kw in (dict(max_depth=0), dict(max_depth=1, paths=0), dict(max_depth=1, paths=65537)):
        with pytest.raises(ort.OrtError) as e:
            radiance_rays_host(s, t, rays, states, **kw)
        assert e.value.code == L.ORT_ERR_INVALID_ARG
    assert radiance_rays_host(s, t, rays, states, max_depth=1, paths=65536).shape == (4, 3)
    with pytest.raises(ort.OrtError) as e:
        radiance_rays_host(s, t, rays, states, max_depth=1, layout=L.ORT_LAYOUT_EXPLICIT)
    assert e.value.code == L.ORT_ERR_UNSUPPORTED
    assert same(radiance_rays_host(s, None, rays, states, max_depth=2, layout=L.ORT_LAYOUT_EXPLICIT, use_octree=False),
                radiance_rays_host(s, None, rays, states, max_depth=2, use_octree=False))
    assert radiance_rays_host(s, t, rays[:0], states[:0], max_depth=1).shape == (0, 3)
    with pytest.raises(ValueError):
        radiance_rays_host(s, t, rays, states[:3], max_depth=1)


@pytest.mark.parametrize("bad", ["float64", "shape5", "flat", "strided", "n_mismatch", "states_dtype", "states_shape",
                                 "states_short", "states_strided", "states_list", "short_out", "out_dtype", "out_list",
                                 "states_out_shape", "states_out_dtype", "pointer_without_n", "pointer_without_out",
                                 "pointer_states_out_true", "pointer_float"])
def test_trace_radiance_rejects_bad_arguments_before_the_abi(ort, bad):
    """dtype, shape, contiguity and size raise ValueError before anything reaches
    ort_trace_radiance (the contextless renderer's _lib is None: reaching it would raise
    AttributeError)."""
    r = contextless_renderer(ort)
    rays, states = np.zeros((10, 6), F), np.zeros((10, 2), F)
    kw = dict(max_depth=2)
    if bad == "float64":
        rays = np.zeros((10, 6), np.float64)
    elif bad == "shape5":
        rays = np.zeros((10, 5), F)
    elif bad == "flat":
        rays = np.zeros(60, F)
    elif bad == "strided":
        rays = np.zeros((10, 12), F)[:, ::2]
    elif bad == "n_mismatch":
        kw["n"] = 9
    elif bad == "states_dtype":
        states = np.zeros((10, 2), np.float64)
    elif bad == "states_shape":
        states = np.zeros((10, 3), F)
    elif bad == "states_short":
        states = np.zeros((9, 2), F)
    elif bad == "states_strided":
        states = np.zeros((10, 4), F)[:, ::2]
    elif bad == "states_list":
        states = [[0.0, 0.0]] * 10
    elif bad == "short_out":
        kw["out"] = np.zeros((9, 3), F)
    elif bad == "out_dtype":
        kw["out"] = np.zeros((10, 3), np.int32)
    elif bad == "out_list":
        kw["out"] = [0.0] * 30
    elif bad == "states_out_shape":
        kw["states_out"] = np.zeros((11, 2), F)
    elif bad == "states_out_dtype":
        kw["states_out"] = np.zeros((10, 2), np.float64)
    elif bad == "pointer_without_n":
        rays, states, kw["out"] = 4096, 8192, 12288
    elif bad == "pointer_without_out":
        rays, states, kw["n"] = 4096, 8192, 4
    elif bad == "pointer_states_out_true":
        rays, states, kw["n"], kw["out"], kw["states_out"] = 4096, 8192, 4, 12288, True
    elif bad == "pointer_float":
        rays, states, kw["n"], kw["out"] = 4096, 8192.0, 4, 12288
    with pytest.raises(ValueError):
        r.trace_radiance(rays, states, **kw)
