"""The ray families of the root-edge tests (tests/test_root_edges.py, tests/test_gpu_root_edges.py):
rays aimed at the numeric edges of the fast walk's sphere test (render_core.h sphere_hit_fast: qsqrt,
qdiv, a_in_qdiv_range) and of its slab shortcuts (child_drops, fmax3 / fmin3), the scenes they run
on, a float32 restatement of Sphere_hit that proves each family reaches its edge, and the shared
references (computed once per process).

Every one-sphere family is a list of parts (k, rays): rays (n, 6) float32 against the sphere of
radius 2^k at the origin, n a multiple of 64 so that a family fills whole waves.  The expected
records always come from the oracle; the restatement only counts coverage.

The restatement rounds once per operation in the shader's order (tests/ray_mode_sets.py's header):
oc = o - c; half_b = dot(oc, d); c = dot(oc, oc) - r * r; a = dot(d, d); disc = half_b * half_b - a * c;
for disc > 0 the numerators n1 = -half_b - sqrt(disc), n2 = -half_b + sqrt(disc) and the roots n1 / a,
n2 / a; dot(u, v) = (ux vx + uy vy) + uz vz."""
import functools

import numpy as np

import ray_sets

F = np.float32
TMIN = F(0.001)
MAXFLOAT = np.finfo(np.float32).max
WAVE = 64
SCALE_K = (-9, 0, 20, 40, 48, 49, 50, 51, 52, 60, 62, 63, 64)
TINY_K = (-30, -48, -50, -60, -70)
ONE_SPHERE = ("tmin_far", "tmin_near", "graze", "scale", "a_edges", "tiny", "mixed")
INLINE_MAX_K = 20  # the nine-sphere tree: families with scale <= 2^20 only
N_TMIN = N_GRAZE = 16384
N_PER_SCALE = 1024
SEEDS = {"tmin_far": 101, "tmin_near": 100, "graze": 103, "scale": 104, "a_edges": 105, "tiny": 106, "mixed": 107,
         "ties": 108}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def bits1(x):
    """The bits of one value rounded to float32, a Python int."""
    return int(np.array([x], F).view(np.int32)[0])


# ---------------------------------------------------------------- the restatement of Sphere_hit

def _dot(u, v):
    return ((u[:, 0] * v[:, 0]).astype(F) + (u[:, 1] * v[:, 1]).astype(F)).astype(F) + (u[:, 2] * v[:, 2]).astype(F)


def sphere_hit(rays, center_radius):
    """Sphere_hit(ray, 0.001, MAXFLOAT) of each ray against one sphere (center_radius (4,)) or its own
    ((n, 4)), float32, one rounding per operation: a dict of a, half_b, c, disc, n1, n2, t1, t2 (NaN
    where disc is not > 0) and `accepted`, the root the shader returns (NaN for a miss)."""
    rays = np.asarray(rays, F)
    cr = np.broadcast_to(np.asarray(center_radius, F), (len(rays), 4))
    nan = F(np.nan)
    with np.errstate(all="ignore"):
        o, d = rays[:, :3], rays[:, 3:]
        oc = (o - cr[:, :3]).astype(F)
        half_b = _dot(oc, d).astype(F)
        c = (_dot(oc, oc).astype(F) - (cr[:, 3] * cr[:, 3]).astype(F)).astype(F)
        a = _dot(d, d).astype(F)
        disc = ((half_b * half_b).astype(F) - (a * c).astype(F)).astype(F)
        pos = disc > 0
        sq = np.sqrt(np.where(pos, disc, F(0))).astype(F)
        n1 = np.where(pos, ((-half_b).astype(F) - sq).astype(F), nan).astype(F)
        n2 = np.where(pos, ((-half_b).astype(F) + sq).astype(F), nan).astype(F)
        t1, t2 = (n1 / a).astype(F), (n2 / a).astype(F)
        ok1 = pos & (t1 < MAXFLOAT) & (t1 > TMIN)
        ok2 = pos & (t2 < MAXFLOAT) & (t2 > TMIN)
        accepted = np.where(ok1, t1, np.where(ok2, t2, nan)).astype(F)
    return dict(a=a, half_b=half_b, c=c, disc=disc, n1=n1, n2=n2, t1=t1, t2=t2, accepted=accepted)


def exponent(x):
    """The binary exponent field of float32 x, unbiased (subnormals and zero: -127)."""
    return ((bits(np.asarray(x, F)) >> 23) & 0xFF) - 127


# ---------------------------------------------------------------- generators

def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, e):
    w = _unit(rng, len(e))
    w -= (w * e).sum(axis=1, keepdims=True) * e
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def _rays(o, d):
    return np.ascontiguousarray(np.concatenate([o, d], axis=1), F)


def _tmin_rays(rng, n, outward):
    """Through a point p of the unit sphere, the origin 0.001 (1 + delta) direction lengths before
    it, delta uniform in +-3e-6; directions of length uniform [0.36, 2.8] (a in [1/8, 8]), at least
    0.2 of it along the normal.  outward: from inside, p is the exit (the far root); else from
    outside, p is the entry (the near root)."""
    u = _unit(rng, n)
    d = u * rng.uniform(0.36, 2.8, (n, 1))
    cos = rng.uniform(0.2, 1.0, (n, 1))
    p = (cos if outward else -cos) * u + np.sqrt(1.0 - cos * cos) * _perp(rng, u)
    t = 0.001 * (1.0 + rng.uniform(-3e-6, 3e-6, (n, 1)))
    return _rays(p - t * d, d)


def _graze_rays(rng, n):
    """From distance 5 of the unit sphere's centre past it at impact parameter sqrt(1 - u),
    u = 2^U(-22, 0): disc = a u.  Direction lengths as above."""
    e = _unit(rng, n)
    h = np.sqrt(1.0 - 2.0 ** rng.uniform(-22.0, 0.0, (n, 1)))
    sin = h / 5.0
    d = (-np.sqrt(1.0 - sin * sin) * e + sin * _perp(rng, e)) * rng.uniform(0.36, 2.8, (n, 1))
    return _rays(5.0 * e, d)


def _scaled(rays, k):
    """The geometry times 2^k (exact in float32): the origins; the directions stay."""
    out = rays.copy()
    out[:, :3] *= F(2.0) ** F(k)
    return out


@functools.lru_cache(maxsize=None)
def a_edge_values():
    """(low, high): the floats x in [0.36, 2.8] whose a = RN(x * x) has a mantissa <= 0x3f, >= 0x7fffc0."""
    lo, hi = bits1(0.36), bits1(2.8)
    low, high = [], []
    step = 1 << 22
    for at in range(lo, hi + 1, step):
        x = np.arange(at, min(at + step, hi + 1), dtype=np.int32).view(F)
        m = bits(x * x) & 0x7FFFFF
        low.append(x[m <= 0x3F])
        high.append(x[m >= 0x7FFFC0])
    return np.concatenate(low), np.concatenate(high)


def _find_direction(target):
    """d = (x, y, 0) whose restated a is exactly `target`: x searched among the floats about
    sqrt(target - y * y), y = 0 first, then small powers of two."""
    target = F(target)
    for y in [0.0] + [2.0 ** -j for j in range(4, 24)]:
        x0 = bits1(np.sqrt(float(target) - y * y))
        x = np.arange(x0 - 256, x0 + 257, dtype=np.int32).view(F)
        a = ((x * x).astype(F) + F(y) * F(y)).astype(F)
        found = np.nonzero(a == target)[0]
        if found.size:
            return np.array([x[found[0]], y, 0.0], F)
    raise AssertionError(f"no direction with a = {target!r}")


A_EDGE_NAMED = {
    "0.125": F(0.125), "8": F(8.0),
    "0.125-": np.nextafter(F(0.125), F(0)), "0.125+": np.nextafter(F(0.125), F(1)),
    "8-": np.nextafter(F(8.0), F(0)), "8+": np.nextafter(F(8.0), F(16)),
}
A_EDGE_OUTSIDE = ("0.125-", "8+")  # a outside a_in_qdiv_range: kept in waves of their own


@functools.lru_cache(maxsize=None)
def a_edge_directions():
    """(inside, outside): (m, 3) float32 directions with a in [1/8, 8] -- 0.125 from (.25, .25, 0), 8
    from (2, 2, 0), the floats next to each end inside the range, every (x, 0, 0) of a_edge_values --
    and the two whose a is the float just outside each end."""
    low, high = a_edge_values()
    inside = [np.array([0.25, 0.25, 0.0], F), np.array([2.0, 2.0, 0.0], F), _find_direction(A_EDGE_NAMED["0.125+"]),
              _find_direction(A_EDGE_NAMED["8-"])]
    inside += [np.array([x, 0.0, 0.0], F) for x in np.concatenate([low, high])]
    outside = [_find_direction(A_EDGE_NAMED[k]) for k in A_EDGE_OUTSIDE]
    return np.stack(inside), np.stack(outside)


def _aimed(rng, d):
    """One ray per direction at the unit sphere: from 1.5 .. 100 back along the direction, offset
    sideways by an impact parameter from dead centre over grazes to a near miss; the direction's
    sign and the axes' order vary (a does not: the zero terms add exactly)."""
    n = len(d)
    d = d.astype(np.float64) * rng.choice([-1.0, 1.0], (n, 1))
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    back = rng.choice([1.5, 3.0, 5.0, 20.0, 100.0], (n, 1))
    h = rng.choice([0.0, 0.5, 0.9, np.sqrt(1 - 2.0 ** -6), np.sqrt(1 - 2.0 ** -12), np.sqrt(1 - 2.0 ** -18), 1.0, 1.001],
                   (n, 1))
    o = -back * u + h * _perp(rng, u)
    roll = rng.integers(0, 3, n)
    for i in range(n):
        o[i], d[i] = np.roll(o[i], roll[i]), np.roll(d[i], roll[i])
    return _rays(o, d)


def _a_edge_rays(rng):
    inside, outside = a_edge_directions()
    n_in = -(-8 * len(inside) // WAVE) * WAVE  # eight origins per direction, rounded up to whole waves
    return np.concatenate([_aimed(rng, inside[np.arange(n_in) % len(inside)]),
                           _aimed(rng, outside[np.arange(WAVE) % len(outside)])])


MIXED_WAVES = 64
MIXED_IN = 48  # in-range rays of each wave: 24 of tmin_far, 24 of graze; the other 16 have a out of range


def _mixed_rays(rng):
    """64 waves of 24 tmin_far + 24 graze rays and 16 of either kind whose direction is times 10 or
    0.1 (a out of a_in_qdiv_range), at random lanes.  Returns (rays, indices of the in-range rays)."""
    n_in, n_out = MIXED_WAVES * MIXED_IN // 2, MIXED_WAVES * (WAVE - MIXED_IN) // 2
    far, graze = _tmin_rays(rng, n_in + n_out, True), _graze_rays(rng, n_in + n_out)
    out_rays = np.concatenate([far[n_in:], graze[n_in:]])
    out_rays[:, 3:] *= rng.choice([F(10.0), F(0.1)], (len(out_rays), 1))
    rays = np.empty((MIXED_WAVES * WAVE, 6), F)
    in_range = np.zeros(len(rays), bool)
    for w in range(MIXED_WAVES):
        lanes = rng.permutation(WAVE)
        at = w * WAVE + lanes
        h = MIXED_IN // 2
        rays[at[:h]] = far[w * h:(w + 1) * h]
        rays[at[h:2 * h]] = graze[w * h:(w + 1) * h]
        rays[at[2 * h:]] = out_rays[w * (WAVE - MIXED_IN):(w + 1) * (WAVE - MIXED_IN)]
        in_range[at[:2 * h]] = True
    return rays, np.nonzero(in_range)[0]


@functools.lru_cache(maxsize=None)
def mixed():
    rays, idx = _mixed_rays(np.random.default_rng(SEEDS["mixed"]))
    rays.setflags(write=False)
    idx.setflags(write=False)
    return rays, idx


@functools.lru_cache(maxsize=None)
def family(name):
    """The parts [(k, rays)] of a one-sphere family; read-only."""
    rng = np.random.default_rng(SEEDS[name])
    if name == "tmin_far":
        parts = [(0, _tmin_rays(rng, N_TMIN, True))]
    elif name == "tmin_near":
        parts = [(0, _tmin_rays(rng, N_TMIN, False))]
    elif name == "graze":
        parts = [(0, _graze_rays(rng, N_GRAZE))]
    elif name == "scale":
        parts = [(k, _scaled(_graze_rays(rng, N_PER_SCALE), k)) for k in SCALE_K]
    elif name == "tiny":
        parts = [(k, _scaled(_graze_rays(rng, N_PER_SCALE), k)) for k in TINY_K]
    elif name == "a_edges":
        parts = [(0, _a_edge_rays(rng))]
    elif name == "mixed":
        parts = [(0, np.array(mixed()[0]))]
    else:
        raise KeyError(name)
    for _, rays in parts:
        assert rays.dtype == F and rays.shape[1] == 6 and len(rays) % WAVE == 0, name
        rays.setflags(write=False)
    return tuple(parts)


def restated(name):
    """sphere_hit of every part of a family against its sphere."""
    return [sphere_hit(rays, [0.0, 0.0, 0.0, 2.0 ** k]) for k, rays in family(name)]


# ---------------------------------------------------------------- ties: slab values equal on two or three axes

TIES_PER_OCTANT = 512
TIES_TWO_AXIS = 1024


def slab_values(corner, rays):
    """The three float32 slab values (corner - o) * (1 / d) of each ray."""
    o, d = rays[:, :3].astype(F), rays[:, 3:].astype(F)
    with np.errstate(all="ignore"):
        return ((corner.astype(F) - o).astype(F) * (F(1) / d).astype(F)).astype(F)


def octants(rays):
    d = rays[:, 3:]
    return (d[:, 0] < 0).astype(int) | ((d[:, 1] < 0).astype(int) << 1) | ((d[:, 2] < 0).astype(int) << 2)


@functools.lru_cache(maxsize=None)
def ties():
    """Rays of ray_sets' compact5 scene through a corner (three equal slab values) or an edge (two) of
    a random node: d = +-2^j per tied axis, j in {-1, 0, 1}, a <= 8, o = corner - 2^m d, m in 0..3;
    kept where o is exact in float32 and the tied slab values are bit-equal.  Returns (rays, corners,
    tied): 512 corner rays per sign octant, then 1024 edge rays (third component of o and d arbitrary);
    tied (n, 3) bool says which axes tie."""
    _, t, _ = ray_sets.scene("compact5")
    rng = np.random.default_rng(SEEDS["ties"])
    lo, hi = t.node_min[0].astype(np.float64), t.node_max[0].astype(np.float64)
    kept = {k: [] for k in range(9)}  # octants 0..7 of the corner rays; 8: the edge rays
    want = {k: TIES_PER_OCTANT for k in range(8)}
    want[8] = TIES_TWO_AXIS
    B = 8192
    while any(sum(len(x[0]) for x in kept[k]) < want[k] for k in kept):
        node = rng.integers(0, t.n_nodes, B)
        corner = np.where(rng.integers(0, 2, (B, 3)) == 1, t.node_max[node], t.node_min[node]).astype(np.float64)
        d = rng.choice([-1.0, 1.0], (B, 3)) * 2.0 ** rng.integers(-1, 2, (B, 3))
        o = corner - 2.0 ** rng.integers(0, 4, (B, 1)) * d
        tied = np.ones((B, 3), bool)
        edge = rng.random(B) < 0.25
        free = rng.integers(0, 3, B)
        rows = np.nonzero(edge)[0]
        tied[rows, free[rows]] = False
        d[rows, free[rows]] = rng.choice([-1.0, 1.0], len(rows)) * rng.uniform(0.05, 1.0, len(rows))
        o[rows, free[rows]] = (lo + (hi - lo) * rng.random((B, 3)))[rows, free[rows]]
        rays = _rays(o, d)
        exact = ((rays[:, :3].astype(np.float64) == o) | ~tied).all(axis=1)
        a = sphere_hit(rays, [0.0, 0.0, 0.0, 1.0])["a"]
        sv = bits(slab_values(corner, rays))
        first = np.argmax(tied, axis=1)
        equal = ((sv == sv[np.arange(B), first][:, None]) | ~tied).all(axis=1)
        ok = exact & equal & (a <= 8) & (a >= 0.125)
        group = np.where(edge, 8, octants(rays))
        for k in kept:
            sel = np.nonzero(ok & (group == k))[0]
            kept[k].append((rays[sel], corner[sel].astype(F), tied[sel]))
    parts = []
    for k in range(9):
        parts.append([np.concatenate([x[i] for x in kept[k]])[:want[k]] for i in range(3)])
    out = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    assert len(out[0]) % WAVE == 0
    for x in out:
        x.setflags(write=False)
    return out


# ---------------------------------------------------------------- scenes and references

FILLER = 40.0  # the inline-leaf scene's eight filler spheres: centres (+-40, +-40, +-40) 2^k, radius 2^k / 2


@functools.lru_cache(maxsize=None)
def scene(k, kind):
    """(spheres, tree) at scale 2^k.  "one": the sphere of radius 2^k at the origin as a depth-0 tree (a
    single leaf root).  "inline": that sphere and eight small fillers far off every axis under
    build_octree(s, 2, 1): the root's eight children split once more, and the target is the only sphere
    of each child's sub-octant at the origin (eight one-sphere leaves under leaf-children nodes).
    Lambertian grey, so that radiance queries scatter."""
    import octreeraytracer_amd as ort
    n = 1 if kind == "one" else 9
    s = ort.SphereSet.empty(n)
    s.center_radius[0] = (0.0, 0.0, 0.0, 1.0)
    for i in range(1, n):
        j = i - 1
        s.center_radius[i] = (FILLER * (1 - 2 * (j & 1)), FILLER * (1 - 2 * ((j >> 1) & 1)), FILLER * (1 - 2 * (j >> 2)), 0.5)
    s.center_radius *= F(2.0) ** F(k)
    s.mat_albedo[:] = (0.0, 0.5, 0.5, 0.5)
    t = ort.build_octree(s, 0, 0) if kind == "one" else ort.build_octree(s, 2, 1)
    for a in (s.center_radius, s.mat_albedo, s.fuzz_ri, t.node_min, t.node_max, t.children_offset, t.objects_offset,
              t.object_count, t.object_indices):
        a.setflags(write=False)
    return s, t


def parts(name, kind):
    """The parts of a family that run on scenes of `kind`."""
    return [(k, rays) for k, rays in family(name) if kind == "one" or k <= INLINE_MAX_K]


@functools.lru_cache(maxsize=None)
def oracle_records(name, kind):
    """The oracle's (n, 2) int32 {hit, t bits} of each part of parts(name, kind) on scene(k, kind);
    name "ties": of the tie rays on the compact5 scene (kind ignored)."""
    from oracle import oracle
    if name == "ties":
        s, t, _ = ray_sets.scene("compact5")
        out = [oracle.trace_rays(s, t, ties()[0])]
    else:
        out = [oracle.trace_rays(*scene(k, kind), rays) for k, rays in parts(name, kind)]
    for r in out:
        r.setflags(write=False)
    return tuple(out)


def check_records(ort, oracle, s, rays, ref, got, label, spheres=True):
    """(t, sphere, normals) against the oracle's records ref: hit flag and t bits of every ray, a miss
    {0.0f, -1, zeros}; the reported sphere is one the oracle hits at that t in its one-sphere scene
    (spheres=False: left to the caller); the normals equal the float32 restatement bit for bit."""
    tt, sph, nrm = got
    hit = sph >= 0
    bad = np.nonzero((hit != (ref[:, 0] == 1)) | (hit & (bits(tt) != ref[:, 1])))[0]
    assert bad.size == 0, (label, int(bad.size), bad[:6], rays[bad[:3]], tt[bad[:6]],
                           np.ascontiguousarray(ref[bad[:6], 1]).view(F), ref[bad[:6], 0])
    assert (bits(tt)[~hit] == 0).all() and (sph[~hit] == -1).all() and (bits(nrm)[~hit] == 0).all(), label
    assert (sph[hit] < s.n).all(), label
    if spheres:
        ray_sets.check_spheres_against_the_oracle(ort, oracle, s, rays, bits(tt), sph)
    assert np.array_equal(bits(nrm), bits(ray_sets.numpy_normals(s, rays, tt, sph))), label


def same_records(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def ties_emulated():
    """The host emulation's (t, sphere, normals) of the tie rays on compact5 (tests/test_root_edges.py
    pins it to the oracle): the GPU suite's sphere indices and normals."""
    from octreeraytracer_amd.renderer import query_rays_host
    s, t, _ = ray_sets.scene("compact5")
    out = query_rays_host(s, t, ties()[0], normals=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ties_nearest():
    """ray_mode_sets' NEAREST record (t, sphere) of the tie rays under the default interval."""
    import ray_mode_sets as rms
    s, _, _ = ray_sets.scene("compact5")
    rays = ties()[0]
    out = rms.nearest_of(rms.sphere_roots(s, rays), len(rays), None)
    for a in out:
        a.setflags(write=False)
    return out


RADIANCE_FAMILIES = ("tmin_near", "graze")


@functools.lru_cache(maxsize=None)
def radiance_set():
    """(rays, states) of the radiance comparison: tmin_near then graze, one RNG chain per ray."""
    from octreeraytracer_amd.renderer import rng_states
    rays = np.concatenate([family(n)[0][1] for n in RADIANCE_FAMILIES])
    states = rng_states(len(rays), 9)
    rays.setflags(write=False)
    states.setflags(write=False)
    return rays, states


@functools.lru_cache(maxsize=None)
def radiance_emulated(kind, use_octree):
    """ort_debug_radiance_rays of radiance_set() on scene(0, kind): paths 1, depth 2."""
    from octreeraytracer_amd.renderer import radiance_rays_host
    s, t = scene(0, kind)
    rays, states = radiance_set()
    out = radiance_rays_host(s, t if use_octree else None, rays, states, max_depth=2, paths=1, use_octree=use_octree)
    out.setflags(write=False)
    return out
