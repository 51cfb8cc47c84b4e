"""Camera queries (ort_trace_camera) without a GPU: the kernels' per-pixel ray and per-ray walk
compiled for the host (ort_debug_camera_query, analysis library) against the independent oracle
-- its camera, RNG sequence, sin / cos, intersectScene and its own frame -- and the bindings' early
checks.  The GPU runs the same source (tests/test_gpu_camera_query.py).  Every comparison is exact.

The oracle's share of hit pixels of the 37 x 21 first-sample frame, by scene and its camera
(camera_sets.CAMERAS): compact5 0.524, compact10 0.512, explicit 0.588, brute 0.588."""
import ctypes

import numpy as np
import pytest

import camera_sets as cs
import ray_sets
from camera_sets import bits
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import camera_query_host
from test_ray_query import CONFIGS, contextless_renderer


def oracle_records(ort, oracle, name, rays):
    """{hit, t bits} of the rays by the oracle: intersectScene on the scene's tree, or for brute
    force the smallest t over every sphere's one-sphere scene (ray_sets.oracle_hits' way)."""
    s, t, _ = ray_sets.scene(name)
    rays = np.ascontiguousarray(rays.reshape(-1, 6))
    if name != "brute":
        return oracle.trace_rays(s, t, rays)
    best = np.full(len(rays), np.inf, np.float32)
    for k in range(s.n):
        one, tree = ray_sets.one_sphere_scene(ort, s, k)
        r = oracle.trace_rays(one, tree, rays)
        tk = np.ascontiguousarray(r[:, 1]).view(np.float32)
        best = np.where((r[:, 0] == 1) & (tk < best), tk, best)
    hit = np.isfinite(best)
    return np.stack([hit.astype(np.int32), np.where(hit, best.view(np.int32), 0)], axis=1)


@pytest.mark.parametrize("which", cs.WHICH)
@pytest.mark.parametrize("ns", cs.SAMPLES)
@pytest.mark.parametrize("w,h", cs.FRAMES)
def test_rays_equal_the_float32_restatement(oracle, which, ns, w, h):
    """Every pixel's ray, bit for bit: the shader's camera ray restated in float32 numpy on the
    oracle's camera, RNG sequence, sin and cos; ray generation alone needs no scene."""
    p = cs.params("compact5", w, h, ns)
    got = camera_query_host(None, None, p, which=which, hits=False)
    assert got.shape == (h, w, 6)
    assert np.array_equal(bits(got), bits(cs.numpy_rays(oracle, p, which)))
    if which == "pixel_centre":  # no draw: the same for every sample count, the camera's own origin
        assert np.array_equal(bits(got), bits(camera_query_host(None, None, cs.params("compact5", w, h, 1), which=which,
                                                                hits=False)))
        assert (got[..., :3] == np.asarray(p.camera_position, np.float32)).all()
    else:  # the lens offset moves the origin, and another stratum count moves the ray
        assert (got[..., :3] != np.asarray(p.camera_position, np.float32)).any(axis=2).mean() > 0.9
    norm = np.linalg.norm(got[..., 3:].astype(np.float64), axis=2)
    assert np.abs(norm - 1.0).max() < 1e-6


def test_the_first_sample_ray_depends_on_the_stratum_count(oracle):
    a = camera_query_host(None, None, cs.params("compact5", ns=1), hits=False)
    b = camera_query_host(None, None, cs.params("compact5", ns=4), hits=False)
    c = camera_query_host(None, None, cs.params("compact5", ns=5), hits=False)
    assert not np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(b), bits(c))  # (int)sqrt(4) == (int)sqrt(5): sample 0 is the same ray


@pytest.mark.parametrize("which", cs.WHICH)
@pytest.mark.parametrize("name", cs.SCENES)
def test_emulation_equals_the_oracle(ort, oracle, name, which):
    """The records of the 37 x 21 frame: the rays are the restated ones; hit flag and t bits equal
    the oracle's intersectScene over them; a miss is {0.0, -1, zeros}; the sphere is the one whose
    one-sphere scene the oracle hits at the same t; the normals equal the float32 restatement; the
    oracle's own hit share lies in 0.2 .. 0.8."""
    s, _, _ = ray_sets.scene(name)
    rays, tt, sph, nrm = cs.emulated(name, which=which)
    assert np.array_equal(bits(rays), bits(cs.numpy_rays(oracle, cs.params(name), which)))
    ref = oracle_records(ort, oracle, name, rays)
    share = float((ref[:, 0] == 1).mean())
    print(name, which, "oracle hit share", share)
    assert 0.2 <= share <= 0.8, share
    flat = np.ascontiguousarray(rays.reshape(-1, 6))
    t1, s1, n1 = tt.reshape(-1), sph.reshape(-1), nrm.reshape(-1, 3)
    hit = s1 >= 0
    assert np.array_equal(hit, ref[:, 0] == 1)
    assert np.array_equal(bits(t1)[hit], ref[hit, 1])
    assert (bits(t1)[~hit] == 0).all() and (s1[~hit] == -1).all() and (bits(n1)[~hit] == 0).all()
    ray_sets.check_spheres_against_the_oracle(ort, oracle, s, flat, bits(t1), s1)
    assert np.array_equal(bits(n1), bits(ray_sets.numpy_normals(s, flat, t1, s1)))
    assert len(np.unique(s1[hit])) >= 10  # many spheres, not one


@pytest.mark.parametrize("name", cs.SCENES)
@pytest.mark.parametrize("w,h,ns", [(64, 8, 4), (64, 8, 5), (37, 21, 4)])
def test_other_frames_equal_the_oracle(ort, oracle, name, w, h, ns):
    rays, tt, sph, nrm = cs.emulated(name, w, h, ns)
    ref = oracle_records(ort, oracle, name, rays)
    hit = sph.reshape(-1) >= 0
    assert np.array_equal(hit, ref[:, 0] == 1) and np.array_equal(bits(tt).reshape(-1)[hit], ref[hit, 1])
    assert 0.02 <= hit.mean() <= 0.98


def lambert_scene(ort, scene_c1):
    """scene_c1 with every material Lambertian and a distinct albedo per sphere."""
    s, t = scene_c1
    ma = np.zeros_like(s.mat_albedo)
    k = np.arange(s.n, dtype=np.float32)
    ma[:, 1], ma[:, 2], ma[:, 3] = (k + 1) / np.float32(s.n + 1), np.float32(1.0) - k / np.float32(2 * s.n), \
        np.float32(0.25) + (k % 7) / np.float32(16)
    assert len({tuple(r) for r in ma[:, 1:]}) == s.n
    return ort.SphereSet(s.center_radius.copy(), ma, s.fuzz_ri.copy()), t


def recomputed_frame(oracle, spheres, rays, sph):
    """The 1 sample x 1 bounce frame from the query's records, in the shader's float32 order:
    albedo[sphere] where the pixel hit, skyColor(ray.d.y) where it missed (glsl:592-595), then
    pow(., 1/2.2) (glsl:659-661)."""
    f = np.float32
    dy = rays[..., 4].astype(f)
    t = (f(0.5) * (dy + f(1.0)).astype(f)).astype(f)
    one_t = (f(1.0) - t).astype(f)
    sky = np.stack([((one_t * f(1.0)).astype(f) + (t * f(c)).astype(f)).astype(f) for c in (0.5, 0.7, 1.0)], axis=-1)
    col = np.where((sph >= 0)[..., None], spheres.mat_albedo[np.maximum(sph, 0), 1:], sky).astype(f)
    g = float(f(1.0) / f(2.2))
    powf = oracle.lib().oracle_pow
    return np.array([powf(float(v), g) for v in col.reshape(-1)], f).reshape(col.shape)


def test_the_records_give_the_oracles_frame(ort, oracle, scene_c1):
    """Ids and miss directions tied to the oracle's own picture: every pixel of its 1 x 1 frame of
    an all-Lambertian scene with distinct albedos is albedo[sphere] or the sky of the ray."""
    s, t = lambert_scene(ort, scene_c1)
    p = ort.FrameParams.default_camera(37, 21, num_samples=1, max_depth=1, **cs.CAMERAS["explicit"])
    rays, tt, sph = camera_query_host(s, t, p, layout=L.ORT_LAYOUT_EXPLICIT)
    frame = oracle.render(s, t, p)
    assert 0.2 <= (sph >= 0).mean() <= 0.8
    assert np.array_equal(bits(recomputed_frame(oracle, s, rays, sph)), bits(frame))
    r2, t2, s2 = camera_query_host(s, t, p, layout=L.ORT_LAYOUT_COMPACT)
    assert np.array_equal(bits(r2), bits(rays)) and np.array_equal(bits(t2), bits(tt)) and np.array_equal(s2, sph)


@pytest.mark.parametrize("which", cs.WHICH)
def test_any_tiling_gives_the_frames_records(ort, which):
    """Left / right at an odd column, a banded tile, a tile reaching 2 rows past the frame: the
    full frame's records (the seed and the camera use the frame's size), zeros past the frame."""
    name = "compact5"
    s, t, _ = ray_sets.scene(name)
    p = cs.params(name, ns=4)
    full = cs.emulated(name, ns=4, which=which)

    def q(tile):
        return camera_query_host(s, t, p, tile, which=which, normals=True)

    left, right = q(ort.Tile(0, 13, 0, 21)), q(ort.Tile(13, 24, 0, 21))
    for a, b, c in zip(left, right, full):
        assert np.array_equal(bits(np.concatenate([a, b], axis=1)), bits(c))
    band = ort.Tile(5, 20, 1, 9, 3, 7)
    ys = band.pixel_rows(21)
    assert list(ys) == [1, 2, 3, 8, 9, 10, 15, 16, 17]
    for a, c in zip(q(band), full):
        assert np.array_equal(bits(a), bits(c[ys, 5:25]))
    over = q(ort.Tile(0, 37, 17, 6))
    for a, c in zip(over, full):
        assert np.array_equal(bits(a[:4]), bits(c[17:]))
        assert (bits(a[4:]) == (-1 if a.dtype == np.int32 else 0)).all()
    assert (over[2][4:] == -1).all() and (bits(over[1][4:]) == 0).all() and (bits(over[0][4:]) == 0).all()


def test_struct_size_and_constants_match_the_header():
    assert ctypes.sizeof(L.OrtCameraQuery) == 40
    assert (L.ORT_CAMERA_FIRST_SAMPLE, L.ORT_CAMERA_PIXEL_CENTRE) == (0, 1)
    assert L.CAMERA_RAYS == {"first_sample": 0, "pixel_centre": 1}


def test_entry_points_are_where_they_belong(ort):
    assert hasattr(L.analysis_lib(), "ort_debug_camera_query")
    assert not hasattr(ort.lib(), "ort_debug_camera_query")
    assert hasattr(ort.lib(), "ort_trace_camera") and "ort_trace_camera" in L.EXPORTED_SYMBOLS


@pytest.mark.parametrize("bad", ["samples", "tile", "which"])
def test_the_emulation_refuses_what_the_call_refuses(ort, bad):
    s, t, _ = ray_sets.scene("explicit")
    p = cs.params("explicit", ns=0 if bad == "samples" else 1)
    tile = ort.Tile(30, 8, 0, 4) if bad == "tile" else None
    lib = L.analysis_lib()
    if bad == "which":
        pc, tc = p.to_c(), ort.Tile.full(p).to_c()
        rays = np.zeros((21 * 37, 6), np.float32)
        rc = lib.ort_debug_camera_query(None, 0, None, None, None, None, None, 0, None, 0, 0, ctypes.byref(pc),
                                        ctypes.byref(tc), 2, L.fptr(rays), None, None)
        assert rc == L.ORT_ERR_INVALID_ARG and not rays.any()
        return
    with pytest.raises(ort.OrtError) as e:
        camera_query_host(s, t, p, tile, layout=L.ORT_LAYOUT_EXPLICIT)
    assert e.value.code == L.ORT_ERR_INVALID_ARG


@pytest.mark.parametrize("bad", ["which", "rays_only_without_rays", "rays_only_with_normals", "rays_only_with_out",
                                 "short_out", "out_dtype", "rays_array", "list"])
def test_trace_camera_rejects_bad_arguments_before_the_abi(ort, bad):
    """Renderer.trace_camera checks its arguments with ValueError before anything reaches
    ort_trace_camera (a wrong buffer would be overrun)."""
    r = contextless_renderer(ort)
    p = ort.FrameParams.default_camera(8, 4)
    kw = {
        "which": dict(which="centre"),
        "rays_only_without_rays": dict(hits=False),
        "rays_only_with_normals": dict(hits=False, rays=True, normals=True),
        "rays_only_with_out": dict(hits=False, rays=True, out=np.zeros((32, 2), np.int32)),
        "short_out": dict(out=np.zeros((31, 2), np.int32)),
        "out_dtype": dict(out=np.zeros((32, 2), np.float32)),
        "rays_array": dict(rays=np.zeros((32, 6), np.float32)),
        "list": dict(out=[0] * 64),
    }[bad]
    with pytest.raises(ValueError):
        r.trace_camera(p, **kw)
