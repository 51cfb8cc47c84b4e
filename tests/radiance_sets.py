"""What the radiance-query tests share (tests/test_radiance_query.py, tests/test_gpu_radiance_query.py):
the scenes (tests/ray_sets.py) with their cameras (tests/camera_sets.py), the rays and RNG states
of a 1-sample frame's pixels, the oracle's frames, and the host emulation's records of the ray
set (computed once per process, read-only)."""
import dataclasses
import functools

import numpy as np

import camera_sets as cs
import ray_sets
from test_ray_query import CONFIGS

SCENES = ("compact5", "compact10", "brute")
FRAMES = cs.FRAMES                     # (37, 21) and (64, 8)
DEPTHS = (1, 2, 4, 8)
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b):
    """Bit for bit; two NaNs in the same place are equal."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def numpy_sky(dy):
    """The shader's sky colour for direction.y, restated in float32: t = 0.5 (d.y + 1),
    (1 - t) * 1 + t * (0.5, 0.7, 1.0)."""
    dy = np.asarray(dy, F)
    with np.errstate(all="ignore"):
        t = (F(0.5) * (dy + F(1.0)).astype(F)).astype(F)
        a = ((F(1.0) - t).astype(F) * F(1.0)).astype(F)
        return np.stack([(a + (t * F(k)).astype(F)).astype(F) for k in (0.5, 0.7, 1.0)], axis=-1)


def scene(name):
    """(spheres, tree or None as the walk takes it, use_octree)."""
    s, t, _ = ray_sets.scene(name)
    layout, use_octree = CONFIGS[name]
    assert layout == 0
    return s, (t if use_octree else None), use_octree


def params(name, w, h, depth):
    return dataclasses.replace(cs.params(name, w, h, 1), max_depth=depth)


def fract32(x):
    x = F(x)
    return F(x - np.floor(x, dtype=F))


@functools.lru_cache(maxsize=None)
def frame_inputs(name, w, h):
    """The rays radiance() receives for the pixels of the 1-sample w x h frame (row-major, GL rows)
    and the RNG state it starts from: the pixel's seed advanced by the six draws that made the ray
    (2 stratum, 2 jitter, 2 disk), restated from the oracle's sequence r as
    (fract(r[4] * 1664525), r[5]) -- rand2D leaves x = fract(previous y * 1664525), y = its result."""
    from oracle import oracle
    from octreeraytracer_amd.renderer import camera_query_host
    rays = camera_query_host(None, None, cs.params(name, w, h, 1), hits=False).reshape(-1, 6)
    states = np.empty((w * h, 2), F)
    for y in range(h):
        for x in range(w):
            sx, sy = F(F(F(x) + F(0.5)) / F(w)), F(F(F(y) + F(0.5)) / F(h))
            r = oracle.rand_sequence(float(sx), float(sy), 6)
            states[y * w + x] = (fract32(F(r[4]) * F(1664525.0)), r[5])
    rays = np.ascontiguousarray(rays)
    rays.setflags(write=False)
    states.setflags(write=False)
    return rays, states


@functools.lru_cache(maxsize=None)
def oracle_frame(name, w, h, depth):
    """The oracle's 1-sample frame, (w * h, 3) in frame_inputs' order."""
    from oracle import oracle
    s, t, _ = ray_sets.scene(name)
    img = oracle.render(s, t, params(name, w, h, depth)).reshape(-1, 3)
    img.setflags(write=False)
    return img


def oracle_pow(x, y):
    from oracle import oracle
    lib = oracle.lib()
    return np.array([lib.oracle_pow(float(v), float(y)) for v in np.asarray(x, F).reshape(-1)], F).reshape(np.shape(x))


def emulate(name, rays, states, **kw):
    from octreeraytracer_amd.renderer import radiance_rays_host
    s, t, use_octree = scene(name)
    return radiance_rays_host(s, t, rays, states, use_octree=use_octree, **kw)


@functools.lru_cache(maxsize=None)
def ray_set(name):
    """The scene's 3001 rays, then the 12 degenerate ones, and rng_states(3013, 7)."""
    from octreeraytracer_amd.renderer import rng_states
    rays = np.ascontiguousarray(np.concatenate([ray_sets.scene(name)[2], ray_sets.degenerate_rays()]))
    states = rng_states(len(rays), 7)
    rays.setflags(write=False)
    states.setflags(write=False)
    return rays, states


@functools.lru_cache(maxsize=None)
def emulated(name, paths, depth):
    """(radiance, end states) of ray_set(name) by the host emulation."""
    rays, states = ray_set(name)
    rad, st = emulate(name, rays, states, max_depth=depth, paths=paths, states_out=True)
    rad.setflags(write=False)
    st.setflags(write=False)
    return rad, st
