"""Adaptive accumulations, restated: the decision of include/ort.h ("adaptive sampling") in numpy
float32, and a driver that derives each pixel's count for a list of passes from the plain moments
emulation (accum_moments_host at k = 1 .. N) -- code the device pass, the stats kernel and
ort_debug_emulate_adaptive do not share.

A pixel's chain depends on the pixel alone, so its state at count k is the k-sample prefix's: the
counts follow from the prefixes' (mean, variance) and the passes' parameters, nothing else."""
import dataclasses
import functools

import numpy as np

f32 = np.float32

# (name, N, tile or None): the canonical chart cases of tests/test_gpu_accum.py with num_samples raised
CPU_INPUTS = [("chart_spp7_b3", 16, None), ("chart_brute_spp2_b6", 9, None), ("chart_odd_spp5_b6", 16, None),
              ("chart_odd_spp5_b6", 16, (16, 50, 5, 48, 16, 32))]  # the band tile that runs past the frame
FLOOR = 0.05
PASS_LISTS = {"ones": None, "2+3+4+7": (2, 3, 4, 7), "5+16": (5, 16)}  # ones: N passes of 1 sample


def pass_list(key, N, min_samples, threshold, floor=FLOOR):
    ns = (1,) * N if PASS_LISTS[key] is None else PASS_LISTS[key]
    return [(n, min_samples, threshold, floor) for n in ns]


def traced_np(k, N, min_samples, threshold, floor, mean, variance):
    """The decision for pixels that all hold k samples: mean (..., 3) and variance (...) as
    ort_accum_read_moments writes them at k (not read for k == 0).  True: traced."""
    shape = variance.shape
    if k >= N:
        return np.zeros(shape, bool)
    if k < min_samples or threshold == 0 or k < 2:
        return np.ones(shape, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        L = (f32(0.2126) * mean[..., 0] + f32(0.7152) * mean[..., 1]) + f32(0.0722) * mean[..., 2]
        ref = np.where(L > f32(floor), L, f32(floor)).astype(f32)
        tol = (f32(threshold) * ref).astype(f32)
        held = variance <= (tol * tol).astype(f32)
    return (variance < 0) | ~held


def in_frame(tile, params):
    """(rows, 1) bool: the tile's rows inside the frame."""
    return (tile.pixel_rows(params.height) < params.height)[:, None]


def counts_np(prefix, N, passes, inside):
    """Each pixel's count after `passes` ((n_samples, min_samples, threshold, floor) tuples).
    prefix: {k: (mean, variance)} for k = 1 .. N, accum_moments_host's; inside: in_frame's mask."""
    shape = prefix[1][1].shape
    counts = np.zeros(shape, np.int32)
    for n, min_samples, threshold, floor in passes:
        new = counts.copy()
        for k in np.unique(counts):
            at = (counts == k) & inside
            if k == 0:
                tr = np.ones(shape, bool)
            else:
                tr = traced_np(int(k), N, min_samples, threshold, floor, *prefix[int(k)])
            new[at & tr] = min(int(k) + n, N)
        counts = new
    return counts


def moments_at(prefix, counts):
    """(mean, variance) with every pixel at its own count (count 0: mean 0, variance -1)."""
    mean = np.zeros(counts.shape + (3,), f32)
    var = np.full(counts.shape, -1, f32)
    for k in np.unique(counts):
        if k == 0:
            continue
        at = counts == k
        mean[at] = prefix[int(k)][0][at]
        var[at] = prefix[int(k)][1][at]
    return mean, var


@functools.lru_cache(maxsize=None)
def scene(name, N, tile=None):
    """(spheres, tree or None, params with num_samples N, tile, prefix moments k = 1 .. N), read-only."""
    import octreeraytracer_amd as ort
    from octreeraytracer_amd.renderer import accum_moments_host
    from test_gpu_accum import case
    c, s, t, p = case(name)
    p = dataclasses.replace(p, num_samples=N)
    tree = t if c["oct"] else None
    tl = ort.Tile(*tile[:4], band_height=tile[4], band_stride=tile[5]) if tile else ort.Tile.full(p)
    prefix = {k: accum_moments_host(s, tree, p, tl, samples_done=k) for k in range(1, N + 1)}
    for m, v in prefix.values():
        m.flags.writeable = False
        v.flags.writeable = False
    return s, tree, p, tl, prefix


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
