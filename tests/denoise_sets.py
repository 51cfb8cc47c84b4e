"""What the denoiser tests share (tests/test_denoise.py, tests/test_gpu_denoise.py): the float32
numpy restatement of the a-trous filter (include/ort.h, ort_denoise), the oracle's 1-sample frames
of the scenes of tests/ray_sets.py under the cameras of tests/camera_sets.py with the host
emulation's pixel-centre guides, and a seeded synthetic image (computed once per process, read-only).

The shapes: 37 columns are less than a wave; 300 cross a 256-pixel segment and are no multiple of
64; 8 and 21 rows are below 2 s from iteration 2 and 3 on, so every tap row but the centre's leaves
the image; 70 rows let s = 32 (6 iterations) reach real rows."""
import dataclasses
import functools

import numpy as np

import camera_sets as cs
import ray_sets

SCENES = ("compact5", "compact10", "brute")
FRAMES = ((37, 21), (64, 8), (96, 64))   # (width, height)
SYNTHETIC = (300, 70)
DEPTH = 8
F = np.float32
H5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
DEFAULTS = dict(iterations=3, sigma_color=0.0, sigma_depth=0.0, normal_power=5, same_sphere=True)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b):
    """Bit for bit; two NaNs in the same place are equal."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def clamp01(x):
    return np.where(x < F(0), F(0), np.where(x > F(1), F(1), x)).astype(F)


def atrous(color, t, sphere, normals, *, iterations=3, sigma_color=0.0, sigma_depth=0.0, normal_power=5, same_sphere=True):
    """The filter of include/ort.h restated: every operation one float32 numpy operation, in the
    header's order.  color (rows, width, 3), t and sphere (rows, width), normals (rows, width, 3)."""
    cur = np.array(color, F)
    t, sphere, n = np.asarray(t, F), np.asarray(sphere, np.int32), np.asarray(normals, F)
    rows, width = t.shape
    Y, X = np.meshgrid(np.arange(rows), np.arange(width), indexing="ij")
    hit = sphere >= 0
    sigma_color, sigma_depth = F(sigma_color), F(sigma_depth)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            if sigma_depth > 0:
                inv_z = F(1) / (sigma_depth * F(s))
            if sigma_color > 0:
                sc = sigma_color * F(2.0 ** -i)
                inv_c = F(1) / (sc * sc)
            sw = np.zeros((rows, width), F)
            sc3 = np.zeros((rows, width, 3), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = Y + s * dy, X + s * dx
                    inside = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < width)
                    qy, qx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, width - 1)
                    cq, hq, idq = cur[qy, qx], hit[qy, qx], sphere[qy, qx]
                    w = np.full((rows, width), H5[dy + 2] * H5[dx + 2], F)
                    both = hit & hq
                    nq = n[qy, qx]
                    a = clamp01((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                    for _ in range(normal_power):
                        a = a * a
                    w = np.where(both, w * a, w)
                    if sigma_depth > 0:
                        w = np.where(both, w * clamp01(F(1) - np.abs(t - t[qy, qx]) * inv_z), w)
                    if sigma_color > 0:
                        d = cur - cq
                        dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                        wc = clamp01(F(1) - dc * inv_c)
                        w = w * (wc * wc)
                    # the taps that add nothing: w = 0, and a non-finite cur_q is never multiplied
                    nothing = ~inside | (hit != hq) | np.isnan(cq).any(axis=2) | np.isinf(cq).any(axis=2)
                    if same_sphere:
                        nothing |= sphere != idq
                    w = np.where(nothing, F(0), w).astype(F)
                    sw = sw + w
                    sc3 = sc3 + np.where(nothing[..., None], F(0), w[..., None] * cq).astype(F)
            through = ~np.isfinite(cur).all(axis=2)
            cur = np.where(through[..., None], cur, sc3 / sw[..., None]).astype(F)
    return cur


def params(name, w, h, ns=1):
    return dataclasses.replace(cs.params(name, w, h, ns), max_depth=DEPTH)


@functools.lru_cache(maxsize=None)
def frame(name, w, h, ns=1):
    """The oracle's ns-sample, 8-bounce frame (h, w, 3)."""
    from oracle import oracle
    s, t, _ = ray_sets.scene(name)
    img = np.ascontiguousarray(oracle.render(s, t, params(name, w, h, ns)), F).reshape(h, w, 3)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def guides(name, w, h):
    """(t, sphere, normals) of the frame's pixel centres by the host emulation."""
    _, t, sphere, normals = cs.emulated(name, w, h, 1, "pixel_centre")
    return t, sphere, normals


@functools.lru_cache(maxsize=None)
def synthetic():
    """A seeded 300 x 70 image of random colours, with the pixel-centre guides of compact5 at that size."""
    w, h = SYNTHETIC
    img = np.random.default_rng(11).random((h, w, 3), dtype=F)
    img.setflags(write=False)
    return (img,) + guides("compact5", w, h)


def inputs(name, w=None, h=None):
    """(image, t, sphere, normals) of a scene's frame, or of "synthetic"."""
    if name == "synthetic":
        return synthetic()
    return (frame(name, w, h),) + guides(name, w, h)


def records(t, sphere):
    """ort_trace_camera's {t bits, sphere} records of a guide pair, (rows, width, 2) int32."""
    return np.ascontiguousarray(np.stack([bits(np.asarray(t, F)), np.asarray(sphere, np.int32)], axis=-1))


def host(image, t, sphere, normals, **kw):
    from octreeraytracer_amd.renderer import denoise_host
    return denoise_host(image, ((t, sphere), normals), **kw)


def mse(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float((d * d).mean())
