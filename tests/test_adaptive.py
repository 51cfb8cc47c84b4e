"""Adaptive accumulations on the CPU: the host emulation (ort_debug_emulate_adaptive: the kernel's
per-pixel chain and the decision the device pass shares) against the numpy restatement of
tests/adaptive_sets.py, which derives every pixel's count from the plain moments emulation.

Every comparison is exact: counts as integers, means and variances as bits.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import adaptive_sets as A
from adaptive_sets import FLOOR, same_bits

INF = float("inf")
IDS = [f"{n}-N{N}{'-band' if t else ''}" for n, N, t in A.CPU_INPUTS]


def host(inp, passes):
    from octreeraytracer_amd.renderer import accum_adaptive_host
    s, tree, p, tile, _ = A.scene(*inp)
    return accum_adaptive_host(s, tree, p, tile, passes=passes)


@pytest.mark.parametrize("inp", A.CPU_INPUTS, ids=IDS)
@pytest.mark.parametrize("split", sorted(A.PASS_LISTS))
@pytest.mark.parametrize("min_samples", (0, 2, 4))
@pytest.mark.parametrize("threshold", (0.0, 0.05, INF))
def test_emulation_is_the_restatement(inp, split, min_samples, threshold):
    s, tree, p, tile, prefix = A.scene(*inp)
    N = p.num_samples
    inside = A.in_frame(tile, p)
    passes = A.pass_list(split, N, min_samples, threshold)
    counts, mean, var = host(inp, passes)
    want = A.counts_np(prefix, N, passes, inside)
    assert np.array_equal(counts, want)
    assert (counts[~np.broadcast_to(inside, counts.shape)] == 0).all()
    wm, wv = A.moments_at(prefix, want)  # each pixel's moments are the plain emulation's at its own count
    assert same_bits(mean, wm) and same_bits(var, wv)
    if threshold == 0.0:  # never held: a moments accumulation
        k = min(N, sum(n for n, *_ in passes))
        assert (counts[np.broadcast_to(inside, counts.shape)] == k).all()
        assert same_bits(mean, prefix[k][0]) and same_bits(var, prefix[k][1])
    if threshold == INF:  # whatever has an estimate is held: nobody passes max(min_samples, 2) by more than a pass
        assert counts.max() <= max(min_samples, 2) + max(n for n, *_ in passes) - 1


HISTOGRAMS = {  # counts 1 .. N after one-sample passes, threshold 0.05, floor 0.05, min_samples 2 (this tree's emulation)
    ("chart_spp7_b3", 16): [0, 1131, 59, 13, 3, 3, 4, 6, 2, 7, 9, 6, 4, 1, 1, 287],
    ("chart_brute_spp2_b6", 9): [0, 2265, 122, 27, 6, 4, 4, 6, 638],
}


@pytest.mark.parametrize("inp", A.CPU_INPUTS[:3], ids=IDS[:3])
def test_the_counts_are_not_vacuous(inp):
    """Conditions, not measurements: the criterion holds a good share of the picture at once, keeps a
    good share to the end, and spreads the rest over the counts between."""
    name, N, _ = inp
    counts, _, _ = host(inp, A.pass_list("ones", N, 2, 0.05))
    hist = np.bincount(counts.ravel(), minlength=N + 1)[1:]
    print(name, "counts 1..N:", " ".join(map(str, hist)))
    assert hist[1] >= 0.1 * counts.size and hist[N - 1] >= 0.1 * counts.size
    assert np.count_nonzero(hist[2:N - 1]) >= 5
    if (name, N) in HISTOGRAMS:
        assert hist.tolist() == HISTOGRAMS[(name, N)]
    else:
        assert (hist[1], hist[N - 1]) == (4643, 1097) and (hist[1:] > 0).all()
    counts4, _, _ = host(inp, A.pass_list("ones", N, 4, 0.05))
    hist4 = np.bincount(counts4.ravel(), minlength=N + 1)[1:]
    assert (hist4[:3] == 0).all() and (hist4[3:] > 0).all(), hist4


def test_decision_edges():
    """The decision on stored states chosen by hand, against the restatement: a non-finite sum is
    never held (below N), k >= N always is, a zero variance is held at any positive threshold."""
    from octreeraytracer_amd.renderer import adaptive_decision_host as dec
    crit = (1, 0, 0.05, FLOOR)
    grey = [2.0, 2.0, 2.0]  # 4 samples of luminance 0.5: m2 = 4 * 0.25 = 1 is zero variance
    assert dec(4, 16, crit, grey, 1.0) == 0
    assert dec(4, 16, (1, 5, 0.05, FLOOR), grey, 1.0) == 1      # below min_samples
    assert dec(4, 16, (1, 0, 0.0, FLOOR), grey, 1.0) == 1       # threshold 0: never held
    assert dec(16, 16, (1, 99, 0.0, FLOOR), grey, 1.0) == 0     # k >= N: held whatever the rest
    assert dec(1, 16, (1, 0, INF, FLOOR), grey, 1.0) == 1 and dec(0, 16, (1, 0, INF, FLOOR), grey, 1.0) == 1  # no estimate
    for bad in (float("nan"), INF, -INF):
        for col, m2 in (([bad, 2.0, 2.0], 1.0), ([2.0, bad, 2.0], 1.0), ([2.0, 2.0, bad], 1.0), (grey, bad)):
            if m2 == -INF:
                continue  # (a sum of squares)
            for thr in (0.05, 1e30, INF):
                assert dec(4, 16, (1, 0, thr, FLOOR), col, m2) == 1, (col, m2, thr)
            assert dec(16, 16, crit, col, m2) == 0
    # a sweep over variances around the tolerance, against the restatement, bits for bits
    rng = np.random.default_rng(7)
    for _ in range(2000):
        k = int(rng.integers(2, 12))
        col = (rng.random(3) * k * rng.choice([0.01, 0.2, 1.0])).astype(np.float32)
        mean = (col / np.float32(k)).astype(np.float32)
        L = (np.float32(0.2126) * mean[0] + np.float32(0.7152) * mean[1]) + np.float32(0.0722) * mean[2]
        m2 = np.float32(k) * (L * L) * np.float32(1.0 + rng.random() * 0.05)
        e2 = np.float32(m2 / np.float32(k))
        d = np.float32(e2 - L * L)
        var = np.float32(max(d, np.float32(0)) / np.float32(k - 1))
        thr = float(rng.choice([0.02, 0.05, 0.1]))
        want = A.traced_np(k, 16, 0, thr, FLOOR, mean[None], np.array([var], np.float32))[0]
        assert dec(k, 16, (1, 0, thr, FLOOR), col, float(m2)) == int(want)


BAD_CRITERIA = {"n_samples 0": (0, 0, 0.05, FLOOR), "negative min_samples": (1, -1, 0.05, FLOOR),
                "negative threshold": (1, 0, -0.5, FLOOR), "nan threshold": (1, 0, float("nan"), FLOOR),
                "zero floor": (1, 0, 0.05, 0.0), "negative floor": (1, 0, 0.05, -1.0), "inf floor": (1, 0, 0.05, INF),
                "nan floor": (1, 0, 0.05, float("nan"))}


@pytest.mark.parametrize("what", sorted(BAD_CRITERIA))
def test_refused_criteria(what):
    from octreeraytracer_amd import OrtError
    from octreeraytracer_amd.renderer import adaptive_decision_host
    assert adaptive_decision_host(4, 16, BAD_CRITERIA[what], [1.0, 1.0, 1.0], 1.0) == -1
    with pytest.raises(OrtError) as e:
        host(A.CPU_INPUTS[0], [(1, 0, 0.05, FLOOR), BAD_CRITERIA[what]])
    assert e.value.code == 1 and "pass 1" in str(e.value)


def test_refusals_that_need_no_gpu(ort):
    """NULL arguments are answered before any context is touched, and a reserved field is refused."""
    from octreeraytracer_amd import _lib as L
    lib = ort.lib()
    a = L.OrtAccumAdaptive(1, 0, 0.05, FLOOR)
    st = L.OrtAccumAdaptiveStats()
    counts = np.full(4, -7, np.int32)
    assert lib.ort_accum_render_adaptive(None, None, C.byref(a), None, None) == L.ORT_ERR_INVALID_ARG
    assert lib.ort_accum_read_counts(None, None, counts.ctypes.data, 0, None) == L.ORT_ERR_INVALID_ARG
    assert lib.ort_accum_adaptive_stats(None, None, C.byref(a), C.byref(st)) == L.ORT_ERR_INVALID_ARG
    assert (counts == -7).all() and st.pixels == 0
    assert C.sizeof(L.OrtAccumAdaptive) == 32 and C.sizeof(L.OrtAccumAdaptiveStats) == 40
    import re
    from pathlib import Path
    header = (Path(__file__).resolve().parents[1] / "include" / "ort.h").read_text()
    flags = {k: int(v) for k, v in re.findall(r"#define\s+(ORT_ACCUM_[A-Z]+)\s+(\d+)", header)}
    assert flags == {"ORT_ACCUM_MOMENTS": L.ORT_ACCUM_MOMENTS, "ORT_ACCUM_ADAPTIVE": L.ORT_ACCUM_ADAPTIVE} and flags["ORT_ACCUM_ADAPTIVE"] == 4
    alib = L.analysis_lib()
    for i in range(4):
        b = L.OrtAccumAdaptive(1, 0, 0.05, FLOOR)
        b.reserved[i] = 1
        assert alib.ort_debug_adaptive_decision(4, 16, C.byref(b), L.fptr(np.ones(3, np.float32)), C.c_float(1.0)) == -1
    s, tree, p, tile, _ = A.scene(*A.CPU_INPUTS[0])
    from octreeraytracer_amd.renderer import accum_adaptive_host
    counts, mean, var = accum_adaptive_host(s, tree, p, tile, passes=[])  # no pass: nothing sampled
    assert (counts == 0).all() and (mean == 0).all() and (var == -1).all()


# ---- what it buys -------------------------------------------------------------------------------------
# measured: (MSE of the adaptive picture) / (MSE of the uniform picture at the nearest equal sample count),
# against the oracle's 256-sample frame: (share of the 16 x pixels samples, uniform k, plain, denoised)
BUYS = {("compact5", 0.02): (0.654, 10, 0.999, 1.089), ("compact5", 0.05): (0.583, 9, 1.321, 1.506),
        ("compact5", 0.1): (0.497, 8, 0.643, 0.699), ("compact10", 0.02): (0.639, 10, 0.933, 1.011),
        ("compact10", 0.05): (0.573, 9, 1.168, 1.286), ("compact10", 0.1): (0.493, 8, 0.690, 0.740),
        ("brute", 0.02): (0.680, 11, 0.872, 1.122), ("brute", 0.05): (0.579, 9, 0.939, 1.350),
        ("brute", 0.1): (0.466, 7, 0.723, 0.954)}


@pytest.mark.parametrize("name", ("compact5", "compact10", "brute"))
def test_what_adaptive_sampling_buys_at_equal_samples(name):
    """96 x 64, 8 bounces, N = 16, one-sample passes to the end with min_samples 4 and floor 0.05, at
    thresholds 0.02, 0.05 and 0.1; the uniform picture is the k-sample frame (its own strata) with k
    the adaptive picture's mean count, rounded; both also through the variance-guided denoise with
    gamma.  MSE against the oracle's 256-sample frame, adaptive / uniform (measured):

        scene      threshold  samples  uniform k  plain  denoised
        compact5   0.02       65 %     10         0.999  1.089
        compact5   0.05       58 %      9         1.321  1.506
        compact5   0.1        50 %      8         0.643  0.699
        compact10  0.02       64 %     10         0.933  1.011
        compact10  0.05       57 %      9         1.168  1.286
        compact10  0.1        49 %      8         0.690  0.740
        brute      0.02       68 %     11         0.872  1.122
        brute      0.05       58 %      9         0.939  1.350
        brute      0.1        47 %      7         0.723  0.954

    Adaptive sampling does NOT beat uniform sampling at equal samples everywhere.  The uniform k-sample
    frame is stratified for its own k -- at k = 9 perfectly, 3 x 3 -- while a pixel stopped at k < N has
    covered only the first k of N's 16 strata (the known limit, include/ort.h); the uniform column swings
    by 2.6 x between k = 8 and k = 9 for that reason alone, which is what makes 0.1 look good and 0.05
    bad.  After the denoise the uniform picture wins or ties at 0.02 and 0.05: the filter already spends
    its smoothing where the variance is high.  0.02, the wrappers' default, is the one threshold that is
    not worse than uniform without the filter on any scene, for two thirds of the samples.  The bound
    is the measured ratio plus 0.1."""
    import dataclasses

    import camera_sets as cs
    import denoise_sets as ds
    import ray_sets
    import variance_sets as vs
    from octreeraytracer_amd.renderer import (DEFAULT_ADAPTIVE_THRESHOLD, accum_adaptive_host, accum_moments_host,
                                               denoise_host)
    from test_ray_query import CONFIGS
    assert DEFAULT_ADAPTIVE_THRESHOLD == 0.02
    N, W, H = 16, 96, 64
    s, t, _ = ray_sets.scene(name)
    tree = t if CONFIGS[name][1] else None
    ref = ds.frame(name, W, H, 256)
    tt, sph, n = ds.guides(name, W, H)
    guides = ((tt, sph), n)
    p = dataclasses.replace(cs.params(name, W, H, N), max_depth=ds.DEPTH)
    for thr in (0.02, 0.05, 0.1):
        share, k, plain, filtered = BUYS[(name, thr)]
        c, m, v = accum_adaptive_host(s, tree, p, passes=[(1, 4, thr, 0.05)] * N)
        assert max(1, int(round(c.sum() / c.size))) == k and abs(c.sum() / (N * c.size) - share) < 0.001
        um, uv = accum_moments_host(s, tree, dataclasses.replace(p, num_samples=k), samples_done=k)
        got = ds.mse(vs.gamma(m), ref) / ds.mse(vs.gamma(um), ref)
        got_f = (ds.mse(denoise_host(m, guides, **ds.DEFAULTS, variance=v, gamma=True), ref) /
                 ds.mse(denoise_host(um, guides, **ds.DEFAULTS, variance=uv, gamma=True), ref))
        print(f"{name} threshold {thr}: {c.sum() / (N * c.size):.3f} of the samples, uniform k = {k}: "
              f"adaptive / uniform MSE {got:.3f}, denoised {got_f:.3f}")
        assert got <= plain + 0.1 and got_f <= filtered + 0.1
