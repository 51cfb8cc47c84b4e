"""What the reprojection tests share (tests/test_reproject.py, tests/test_gpu_reproject.py): the
float32 numpy restatement of ort_history_update's arithmetic (include/ort.h), one operation per numpy
operation on the oracle's camera frame, and the camera sequences it is compared on: the scenes and
frames of tests/denoise_sets.py under moving cameras (the oracle's one-sample frames, the host
emulation's pixel-centre rays and hit records) and a seeded synthetic 300 x 70 image with made-up
hit records (computed once per process, read-only).

The shapes: denoise_sets' (37 columns are less than a wave, 8 rows less than a block row count of
anything); 300 columns cross a 256-pixel segment and are no multiple of 64.  Every sequence has five
updates: a first frame, a translation, a rotation with a zoom change, the same camera again (the
same-camera path) and a jump that leaves most of the frame without history."""
import functools

import numpy as np

import camera_sets as cs
import denoise_sets as ds
import ray_sets
from test_ray_query import CONFIGS

F = np.float32
SCENES = ds.SCENES
FRAMES = ds.FRAMES
SYNTHETIC = ds.SYNTHETIC
ALPHAS = (0.0, 0.2, 1.0)
DEPTH_TOLERANCES = (0.0, 0.1)
STEPS = ("first", "translation", "rotation", "same", "jump")
# the translation per scene: the spheres are small and near, so that a tenth of a unit already
# uncovers a tenth of the frame (tests/test_reproject.py asserts the shares)
SHIFT = {"compact5": (0.09, 0.03, 0.0), "compact10": (0.09, 0.03, 0.0), "brute": (0.025, 0.008, 0.0)}

same = ds.same
bits = ds.bits


def poses(name):
    """The five cameras of a scene's sequence: dicts for FrameParams.default_camera."""
    import octreeraytracer_amd.scene as sc
    base = dict(position=sc.DEFAULT_CAMERA_POSITION, yaw=sc.DEFAULT_YAW, pitch=sc.DEFAULT_PITCH, zoom=sc.DEFAULT_ZOOM)
    base.update(cs.CAMERAS[name])
    moved = dict(base, position=tuple(float(a + b) for a, b in zip(base["position"], SHIFT[name])))
    turned = dict(moved, yaw=moved["yaw"] + 3.0, pitch=moved["pitch"] - 1.0, zoom=moved["zoom"] * 1.1)
    jumped = dict(turned, yaw=turned["yaw"] + 150.0)
    return (base, moved, turned, dict(turned), jumped)


def params(name, w, h, pose):
    import octreeraytracer_amd as ort
    return ort.FrameParams.default_camera(w, h, num_samples=1, max_depth=ds.DEPTH,
                                          use_octree=1 if CONFIGS[name][1] else 0, **pose)


@functools.lru_cache(maxsize=None)
def frame_inputs(name, w, h, k, tile=None, height=None):
    """(params, tile, image, rays, t, sphere) of update k of a scene's sequence at w x h: the oracle's
    one-sample frame and the emulation's pixel-centre guides of the tile (default: the whole frame).
    tile: (x0, width, y0, rows); height: another frame height for this update."""
    import octreeraytracer_amd as ort
    from octreeraytracer_amd.renderer import camera_query_host
    from oracle import oracle
    s, t, _ = ray_sets.scene(name)
    layout, use_octree = CONFIGS[name]
    p = params(name, w, height or h, poses(name)[k])
    tl = ort.Tile(tile[0], tile[1], tile[2], tile[3]) if tile else ort.Tile.full(p)
    img = np.ascontiguousarray(oracle.render(s, t, p, x0=tl.x0, y0=tl.y0, width=tl.width, rows=tl.rows), F)
    img = img.reshape(tl.rows, tl.width, 3)
    rays, tt, sph = camera_query_host(s, t if use_octree else None, p, tl, which="pixel_centre", layout=layout)
    for a in (img, rays, tt, sph):
        a.setflags(write=False)
    return p, tl, img, rays, tt, sph


@functools.lru_cache(maxsize=None)
def synthetic_inputs(k):
    """Update k of the synthetic sequence: a seeded 300 x 70 image with NaN and infinite samples, the
    pixel-centre rays of compact5's cameras at that size, and made-up hit records: sphere ids in
    16 x 8 blocks, distances 5 .. 15 that drift with k, a few NaN distances, and an all-miss region
    right of column 200."""
    import octreeraytracer_amd as ort
    from octreeraytracer_amd.renderer import camera_query_host
    w, h = SYNTHETIC
    p = params("compact5", w, h, poses("compact5")[k])
    tl = ort.Tile.full(p)
    rng = np.random.default_rng(100 + k)
    img = rng.random((h, w, 3), dtype=F)
    bad = rng.random((h, w)) < 0.03
    img[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    rays = camera_query_host(None, None, p, tl, which="pixel_centre", hits=False)
    Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    sph = ((X // 16 + 3 * (Y // 8)) % 7).astype(np.int32)
    tt = (F(5.0) + F(10.0) * np.random.default_rng(7).random((h, w), dtype=F) * F(0.02) + (sph.astype(F) + F(0.05 * k))).astype(F)
    tt[np.random.default_rng(8).random((h, w)) < 0.01] = np.nan
    miss = X > 200
    sph[miss] = -1
    tt[miss] = 0.0
    for a in (img, rays, tt, sph):
        a.setflags(write=False)
    return p, tl, img, rays, tt, sph


# the sequences: name -> the five updates' inputs
TILE_SEQ = ((5, 64, 40, 30), (9, 64, 38, 30), (9, 64, 38, 30), (9, 64, 38, 30), (0, 64, 45, 30))
HEIGHT_SEQ = (64, 48, 48, 64, 64)


def sequence_names():
    out = [f"{n}-{w}x{h}" for n in SCENES for w, h in FRAMES]
    return out + ["synthetic", "tile", "height"]


def sequence(seq):
    """The five updates of a sequence: a list of (params, tile, image, rays, t, sphere)."""
    if seq == "synthetic":
        return [synthetic_inputs(k) for k in range(5)]
    if seq == "tile":  # a tile off the origin that reaches past the 96 x 64 frame and moves
        return [frame_inputs("compact5", 96, 64, k, tile=TILE_SEQ[k]) for k in range(5)]
    if seq == "height":  # the frame's height changes between updates; the tile keeps 64 rows
        return [frame_inputs("compact5", 96, 64, k, tile=(0, 96, 0, 64), height=HEIGHT_SEQ[k]) for k in range(5)]
    name, shape = seq.split("-")
    w, h = (int(v) for v in shape.split("x"))
    return [frame_inputs(name, w, h, k) for k in range(5)]


def lum(c):
    return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]).astype(F)


def dotc(a, b):
    """dot of a field of vectors with one vector (or field): (a.x b.x + a.y b.y) + a.z b.z."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def same_camera(p, x0, y0, q, qx0, qy0):
    v = lambda a: np.asarray(a, F).reshape(-1).view(np.int32)  # noqa: E731
    return (p.width == q.width and p.height == q.height and x0 == qx0 and y0 == qy0 and
            np.array_equal(v(p.view), v(q.view)) and np.array_equal(v(p.camera_position), v(q.camera_position)) and
            np.array_equal(v([p.camera_zoom]), v([q.camera_zoom])))


def update(state, image, rays, t, sphere, p, tile, alpha, depth_tolerance):
    """One ort_history_update restated.  state: None, or the first thing the previous call returned.
    Returns (state, colour, variance, length, have) -- have: the pixels that found history."""
    from oracle import oracle
    alpha, tol = F(alpha), F(depth_tolerance)
    s = np.asarray(image, F)
    t, sphere, rays = np.asarray(t, F), np.asarray(sphere, np.int32), np.asarray(rays, F)
    rows, width = t.shape
    pad = (tile.y0 + np.arange(rows)) >= p.height
    with np.errstate(all="ignore"):
        l = lum(s)
        ok = np.isfinite(s).all(axis=2)
        have = np.zeros((rows, width), bool)
        prev = [np.zeros((rows, width), F) for _ in range(6)]  # r, g, b, m1, m2, n
        if state is not None:
            pp, (px0, py0), qa, qb = state
            qid = bits(qb[..., 3])

            def planes(a, b):
                return [a[..., 0], a[..., 1], a[..., 2], b[..., 0], b[..., 1], a[..., 3]]

            if same_camera(pp, px0, py0, p, tile.x0, tile.y0):
                have = (qa[..., 3] > 0) & (qid == sphere)
                prev = [np.where(have, x, F(0)).astype(F) for x in planes(qa, qb)]
            else:
                cam = oracle.camera(pp).astype(F)
                O, LL, hor, ver, w = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[18:21]
                hh, vv = dotc(hor, hor), dotc(ver, ver)
                o, d = rays[..., :3], rays[..., 3:]
                hit = sphere >= 0
                e = np.where(hit[..., None], ((o + t[..., None] * d).astype(F) - O).astype(F), d).astype(F)
                z = (-dotc(e, w)).astype(F)
                k = (F(10.0) / z).astype(F)
                q = ((k[..., None] * e + O).astype(F) - LL).astype(F)
                a = (dotc(q, hor) / hh).astype(F)
                b = (dotc(q, ver) / vv).astype(F)
                fx = ((a * F(pp.width) - F(0.5)) - F(px0)).astype(F)
                fy = ((b * F(pp.height) - F(0.5)) - F(py0)).astype(F)
                valid = ((z > 0) & np.isfinite(fx) & np.isfinite(fy) & (fx >= F(-1)) & (fx < F(width)) &
                         (fy >= F(-1)) & (fy < F(rows)))
                flx, fly = np.floor(fx).astype(F), np.floor(fy).astype(F)
                wx, wy = (fx - flx).astype(F), (fy - fly).astype(F)
                ux, uy = (F(1) - wx).astype(F), (F(1) - wy).astype(F)
                ix = np.where(valid, flx, F(0)).astype(np.int64)
                iy = np.where(valid, fly, F(0)).astype(np.int64)
                depth = hit & (tol > 0)
                dist = np.sqrt(dotc(e, e)).astype(F)
                tolv = (tol * dist).astype(F)
                ws = np.zeros((rows, width), F)
                for n in range(4):
                    tx, ty = ix + (n & 1), iy + (n >> 1)
                    inside = valid & (tx >= 0) & (tx < width) & (ty >= 0) & (ty < rows)
                    cx, cy = np.clip(tx, 0, width - 1), np.clip(ty, 0, rows - 1)
                    ta, tb = qa[cy, cx], qb[cy, cx]
                    counts = inside & (ta[..., 3] > 0) & (qid[cy, cx] == sphere)
                    counts &= ~depth | (np.abs(tb[..., 2] - dist) <= tolv)
                    wt = ((wx if n & 1 else ux) * (wy if n >> 1 else uy)).astype(F)
                    ws = np.where(counts, ws + wt, ws).astype(F)
                    prev = [np.where(counts, acc + wt * x, acc).astype(F) for acc, x in zip(prev, planes(ta, tb))]
                have = valid & (ws >= F(0.01))
                prev = [np.where(have, acc / ws, F(0)).astype(F) for acc in prev]
        new = [s[..., 0], s[..., 1], s[..., 2], l, (l * l).astype(F)]
        n = np.where(ok, prev[5] + F(1), prev[5]).astype(F)
        a = (F(1) / n).astype(F)
        a = np.where(a < alpha, alpha, a).astype(F)
        hist = [np.where(ok, px + a * (nx - px), px).astype(F) for px, nx in zip(prev[:5], new)]
        first = [np.where(ok, nx, F(0)).astype(F) for nx in new]
        X = [np.where(have, hx, fx_).astype(F) for hx, fx_ in zip(hist, first)]
        n = np.where(have, n, np.where(ok, F(1), F(0))).astype(F)
        ne = (F(1) / a).astype(F)
        v = (X[4] - X[3] * X[3]).astype(F)
        v = np.where(v < 0, F(0), v).astype(F)
        rv = (v / (ne - F(1))).astype(F)
        var = np.where(have & (ne > 1) & np.isfinite(rv), rv, F(-1)).astype(F)
    na = np.stack([X[0], X[1], X[2], n], axis=-1).astype(F)
    nb = np.stack([X[3], X[4], t, sphere.view(F)], axis=-1).astype(F)
    na[pad] = 0
    nb[pad] = np.array([0, 0, 0, np.array([-1], np.int32).view(F)[0]], F)
    var[pad] = -1
    have = have & ~pad[:, None]
    return (p, (tile.x0, tile.y0), na, nb), na[..., :3].copy(), var, na[..., 3].copy(), have


def host(state, image, rays, t, sphere, p, tile, alpha, depth_tolerance):
    """The host emulation's update: (state, colour, variance, length)."""
    from octreeraytracer_amd.renderer import history_update_host
    return history_update_host(state, image, p, tile, (rays, (t, sphere)), alpha=alpha, depth_tolerance=depth_tolerance)


@functools.lru_cache(maxsize=None)
def emulated(seq, alpha, depth_tolerance):
    """The emulation's five updates of a sequence: a list of (state, colour, variance, length), read-only."""
    out, state = [], None
    for p, tile, img, rays, t, sph in sequence(seq):
        state, col, var, length = host(state, img, rays, t, sph, p, tile, alpha, depth_tolerance)
        for a in (state[2], state[3], col, var, length):
            a.setflags(write=False)
        out.append((state, col, var, length))
    return out
