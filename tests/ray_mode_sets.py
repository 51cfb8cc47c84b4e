"""The yardstick of the query-mode tests (tests/test_ray_modes.py, tests/test_gpu_ray_modes.py): a
numpy float32 restatement of the two roots of Sphere_hit (glsl:224-273) for every (ray, sphere)
pair of a tests/ray_sets.py scene, the NEAREST record and the ANY flag derived from them for any
per-ray interval, and the seeded interval generator.  No tree, no walk: every sphere, every ray.

One rounded operation at a time, in the shader's order: oc = o - c; half_b = dot(oc, d);
c = dot(oc, oc) - r * r; a = dot(d, d); disc = half_b * half_b - a * c; for disc > 0 the roots
(-half_b - sqrt(disc)) / a and (-half_b + sqrt(disc)) / a; dot(u, v) = (ux vx + uy vy) + uz vz."""
import functools

import numpy as np

import ray_sets

F = np.float32
MAXFLOAT = np.finfo(np.float32).max
DEFAULT = (F(0.001), MAXFLOAT)
CHUNK = 256  # spheres per block of the (ray, sphere) grid


def _dot(ax, ay, az, bx, by, bz):
    return ((ax * bx).astype(F) + (ay * by).astype(F)).astype(F) + (az * bz).astype(F)


def sphere_roots(spheres, rays):
    """Every (ray, sphere) pair with disc > 0, sorted by ray, then sphere: (ray index, sphere index,
    near root, far root), the roots float32."""
    o = [rays[:, k:k + 1].astype(F) for k in range(3)]
    d = [rays[:, 3 + k:4 + k].astype(F) for k in range(3)]
    cr = spheres.center_radius.astype(F)
    ri, ki, near, far = [], [], [], []
    with np.errstate(all="ignore"):
        a = _dot(*d, *d).astype(F)
        for k0 in range(0, spheres.n, CHUNK):
            c = cr[k0:k0 + CHUNK]
            oc = [(o[k] - c[None, :, k]).astype(F) for k in range(3)]
            hb = _dot(*oc, *d).astype(F)
            cc = (_dot(*oc, *oc).astype(F) - (c[None, :, 3] * c[None, :, 3]).astype(F)).astype(F)
            disc = ((hb * hb).astype(F) - (a * cc).astype(F)).astype(F)
            r, k = np.nonzero(disc > 0)
            sq = np.sqrt(disc[r, k]).astype(F)
            nhb, ar = (-hb[r, k]).astype(F), a[r, 0]
            ri.append(r)
            ki.append(k + k0)
            near.append(((nhb - sq).astype(F) / ar).astype(F))
            far.append(((nhb + sq).astype(F) / ar).astype(F))
    ri, ki, near, far = (np.concatenate(x) for x in (ri, ki, near, far))
    order = np.lexsort((ki, ri))
    return ri[order].astype(np.int64), ki[order].astype(np.int64), near[order], far[order]


@functools.lru_cache(maxsize=None)
def roots(name):
    s, _, rays = ray_sets.scene(name)
    out = sphere_roots(s, rays)
    for a in out:
        a.setflags(write=False)
    return out


def clean_interval(t_range, n):
    """(t_min, t_max, valid) per ray as the library takes an interval: None is (0.001, MAXFLOAT);
    valid iff 0 <= t_min < t_max (NaN: not valid); t_max = +inf is MAXFLOAT."""
    if t_range is None:
        return np.full(n, DEFAULT[0], F), np.full(n, DEFAULT[1], F), np.ones(n, bool)
    t_range = np.asarray(t_range, F)
    assert t_range.shape == (n, 2)
    tmin, tmax = t_range[:, 0].copy(), t_range[:, 1].copy()
    with np.errstate(invalid="ignore"):
        valid = (tmin >= 0) & (tmin < tmax)
    tmax[tmax > MAXFLOAT] = MAXFLOAT
    return tmin, tmax, valid


def accepted(near, far, tmin, tmax, valid):
    """c_k per pair: the near root if it lies in the open interval, else the far root if that one
    does, else +inf."""
    with np.errstate(invalid="ignore"):
        c = np.where((near < tmax) & (near > tmin), near, np.where((far < tmax) & (far > tmin), far, F(np.inf))).astype(F)
    c[~valid] = np.inf
    return c


def nearest_of(table, n, t_range):
    """The NEAREST record of each of n rays from a roots table: t = min c_k, the lowest sphere
    attaining it; (0.0, -1) for a miss.  Returns (t float32 (n,), sphere int32 (n,))."""
    ri, ki, near, far = table
    tmin, tmax, valid = clean_interval(t_range, n)
    c = accepted(near, far, tmin[ri], tmax[ri], valid[ri])
    order = np.lexsort((ki, c, ri))  # by ray, then c_k, then sphere
    first = np.ones(len(ri), bool)
    first[1:] = ri[order][1:] != ri[order][:-1]
    sel = order[first]
    t = np.zeros(n, F)
    sph = np.full(n, -1, np.int32)
    hit = c[sel] < np.inf
    t[ri[sel][hit]] = c[sel][hit]
    sph[ri[sel][hit]] = ki[sel][hit]
    return t, sph


def nearest(name, t_range=None):
    return nearest_of(roots(name), ray_sets.N_RAYS, t_range)


def any_flags(name, t_range=None):
    """ANY's hit-or-miss: does any sphere have a c_k in the ray's interval?"""
    return nearest(name, t_range)[1] >= 0


def accepted_for(name, t_range, sphere):
    """c_k of the sphere each ray reports (sphere (n,), -1 none) for the ray's interval: +inf where
    that sphere has no accepted root, NaN where sphere is -1."""
    ri, ki, near, far = roots(name)
    n = ray_sets.N_RAYS
    s, _, _ = ray_sets.scene(name)
    tmin, tmax, valid = clean_interval(t_range, n)
    out = np.full(n, np.nan, F)
    rows = np.nonzero(sphere >= 0)[0]
    key = ri * s.n + ki  # sorted: by ray, then sphere
    want = rows * s.n + sphere[rows]
    at = np.searchsorted(key, want)
    found = (at < len(key)) & (key[np.minimum(at, len(key) - 1)] == want)
    out[rows] = np.inf
    r, a = rows[found], at[found]
    out[r] = accepted(near[a], far[a], tmin[r], tmax[r], valid[r])
    return out


# Rays of every scene whose interval is set by hand (indices into the ray set, class "inside"):
# {t_min, t_max} below; HAND_VALID says which are intervals at all.
HAND = {
    3: (0.0, np.inf),
    11: (0.0, MAXFLOAT),
    19: (0.001, np.inf),
    27: (-0.0, 5.0),
    35: (np.nan, MAXFLOAT),
    43: (0.001, np.nan),
    51: (-1.0, MAXFLOAT),
    59: (-1e-30, 5.0),
    67: (2.0, 2.0),
    75: (np.inf, np.inf),
}
HAND_INVALID = (35, 43, 51, 59, 67, 75)


@functools.lru_cache(maxsize=None)
def intervals(name):
    """(3001, 2) float32 {t_min, t_max} for scene(name)'s rays, default_rng(5).  t_near is the
    default-interval nearest t, or 10 for a miss.  t_min is 0.001 for half the rays, else
    t_near * U(0, 1.2); t_max is MAXFLOAT for 30 % of the rays, else t_near * U(0.3, 3.0).  Inverted
    intervals occur and stay: they must miss.  HAND's rays are set by hand on top."""
    n = ray_sets.N_RAYS
    rng = np.random.default_rng(5)
    t, sph = nearest(name)
    t_near = np.where(sph >= 0, t, F(10)).astype(np.float64)
    tmin = np.where(rng.random(n) < 0.5, 0.001, t_near * rng.uniform(0.0, 1.2, n))
    tmax = np.where(rng.random(n) < 0.3, float(MAXFLOAT), t_near * rng.uniform(0.3, 3.0, n))
    out = np.stack([tmin, tmax], axis=1).astype(F)
    for i, (a, b) in HAND.items():
        out[i] = (a, b)
    out.setflags(write=False)
    return out
