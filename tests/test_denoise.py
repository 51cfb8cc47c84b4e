"""The guided denoiser on the CPU (no GPU needed): the host emulation (ort_debug_denoise: the kernels'
own per-pixel function) against the float32 numpy restatement of include/ort.h's arithmetic
(tests/denoise_sets.py), bit for bit; the edge cases; the refusals; and that it denoises."""
import ctypes as C

import numpy as np
import pytest

import denoise_sets as ds

F = np.float32
SMALL = [(name, w, h) for name in ds.SCENES for (w, h) in ds.FRAMES]


def lib_and_types():
    from octreeraytracer_amd import _lib as L
    return L.analysis_lib(), L


def check_equal(inp, **kw):
    img, t, sph, n = inp
    want = ds.atrous(img, t, sph, n, **kw)
    got = ds.host(img, t, sph, n, **kw)
    assert ds.same(got, want), f"{int((ds.bits(got) != ds.bits(want)).any(axis=2).sum())} pixels differ ({kw})"


@pytest.mark.parametrize("name,w,h", SMALL)
@pytest.mark.parametrize("iterations", (1, 2, 3, 4, 5))
def test_emulation_equals_numpy_on_the_frames(name, w, h, iterations):
    check_equal(ds.inputs(name, w, h), iterations=iterations)                       # the defaults
    check_equal(ds.inputs(name, w, h), iterations=iterations, same_sphere=False, normal_power=0,
                sigma_color=1.0, sigma_depth=0.5)


@pytest.mark.parametrize("same_sphere", (True, False))
@pytest.mark.parametrize("sigma_color", (0.0, 1.0, 0.5))
@pytest.mark.parametrize("sigma_depth", (0.0, 1.0, 0.5))
@pytest.mark.parametrize("normal_power", (0, 5))
def test_emulation_equals_numpy_under_every_term(same_sphere, sigma_color, sigma_depth, normal_power):
    kw = dict(same_sphere=same_sphere, sigma_color=sigma_color, sigma_depth=sigma_depth, normal_power=normal_power)
    check_equal(ds.inputs("compact10", 37, 21), iterations=3, **kw)
    check_equal(ds.inputs("brute", 64, 8), iterations=4, **kw)


@pytest.mark.parametrize("kw", (dict(), dict(same_sphere=False, sigma_color=1.0, sigma_depth=1.0),
                                dict(sigma_color=0.5, normal_power=0)))
def test_emulation_equals_numpy_with_six_iterations_on_300x70(kw):
    check_equal(ds.inputs("synthetic"), iterations=6, **kw)


# ---- edge cases ---------------------------------------------------------------------------------
def test_non_finite_pixels_pass_through_and_are_skipped_as_taps():
    img, t, sph, n = ds.inputs("compact5", 37, 21)
    img = img.copy()
    bad = [(0, 0, F("nan")), (10, 18, F("inf")), (11, 18, -F("inf")), (20, 36, F("nan")), (5, 7, F("inf"))]
    for k, (y, x, v) in enumerate(bad):
        img[y, x, k % 3] = v
    for kw in (dict(iterations=3), dict(iterations=2, sigma_color=1.0, same_sphere=False)):
        got = ds.host(img, t, sph, n, **kw)
        assert ds.same(got, ds.atrous(img, t, sph, n, **kw))
        mask = np.zeros(img.shape[:2], bool)
        for y, x, _ in bad:
            mask[y, x] = True
            assert ds.same(got[y, x], img[y, x])          # copied through
        assert np.isfinite(got[~mask]).all()               # and never a tap of a neighbour
    # the same image with those pixels' colour replaced by anything else: every other pixel is unchanged
    other = img.copy()
    for y, x, _ in bad:
        other[y, x] = (F("nan"), F(3.0), F(-2.0))
    a, b = ds.host(img, t, sph, n), ds.host(other, t, sph, n)
    assert ds.same(a[~mask], b[~mask])


def test_all_miss_and_all_one_sphere_images():
    img = ds.synthetic()[0][:21, :37].copy()
    n = np.zeros((21, 37, 3), F)
    miss_t, miss_s = np.zeros((21, 37), F), np.full((21, 37), -1, np.int32)
    got = ds.host(img, miss_t, miss_s, n)
    assert ds.same(got, ds.atrous(img, miss_t, miss_s, n))
    assert np.isfinite(got).all() and ds.mse(got, 0.5) < ds.mse(img, 0.5)   # a plain blur of uniform noise
    rng = np.random.default_rng(3)
    nrm = rng.normal(size=(21, 37, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True).astype(F)
    one_t, one_s = (F(2.0) + rng.random((21, 37), dtype=F)), np.full((21, 37), 7, np.int32)
    for kw in (dict(), dict(sigma_depth=0.5, normal_power=2)):
        assert ds.same(ds.host(img, one_t, one_s, nrm, **kw), ds.atrous(img, one_t, one_s, nrm, **kw))


def test_colour_pitch_in_place_and_output_pitch():
    img, t, sph, n = ds.inputs("compact10", 37, 21)
    want = ds.host(img, t, sph, n)
    wide = np.full((21, 50, 3), F("nan"))
    wide[:, :37] = img
    assert ds.same(ds.host(wide[:, :37], t, sph, n), want)                     # a colour pitch
    for iterations in (1, 3):                                                   # in place
        buf = img.copy()
        res = ds.host(buf, t, sph, n, iterations=iterations, out=buf)
        assert res is buf and ds.same(buf, ds.atrous(img, t, sph, n, iterations=iterations))
    flat = np.full(21 * 160, F(-7.0))                                           # an output pitch: 640 bytes
    ds.host(img, t, sph, n, out=flat, row_pitch=640)
    rows = flat.reshape(21, 160)
    assert ds.same(rows[:, :111].reshape(21, 37, 3), want) and (rows[:, 111:] == F(-7.0)).all()


@pytest.mark.parametrize("name,w,h", [("compact5", 37, 21), ("brute", 64, 8)])
def test_rgba8_is_the_packed_rgb32f_result(name, w, h):
    lib, L = lib_and_types()
    img, t, sph, n = ds.inputs(name, w, h)
    img = img.copy()
    img[3, 5] = (F("nan"), F(2.0), F(-1.0))                                    # passes through, then quantised
    f32 = ds.host(img, t, sph, n)
    want = np.empty(w * h, np.uint32)
    L.acheck(lib.ort_debug_pack_rgba8(L.fptr(np.ascontiguousarray(f32)), w * h, want.ctypes.data_as(C.POINTER(C.c_uint32))))
    got = ds.host(img, t, sph, n, format="rgba8")
    assert got.dtype == np.uint8 and got.shape == (h, w, 4)
    assert np.array_equal(got.reshape(-1).view(np.uint32), want)
    pitched = np.full(h * (4 * w + 8), 9, np.uint8)
    ds.host(img, t, sph, n, format="rgba8", out=pitched, row_pitch=4 * w + 8)
    rows = pitched.reshape(h, 4 * w + 8)
    assert np.array_equal(rows[:, :4 * w].reshape(-1).view(np.uint32), want) and (rows[:, 4 * w:] == 9).all()


# ---- arguments ----------------------------------------------------------------------------------
def make_call(L, w=8, h=4):
    """A valid (desc, output) pair over arrays kept alive in the returned dict."""
    rng = np.random.default_rng(5)
    k = dict(color=rng.random((h, w, 3), dtype=F), hits=np.zeros((h, w, 2), np.int32),
             normals=np.zeros((h, w, 3), F), out=np.full((h, w, 3), F(-3.0)))
    d = L.OrtDenoiseDesc()
    d.color, d.hits, d.normals = k["color"].ctypes.data, k["hits"].ctypes.data, k["normals"].ctypes.data
    d.width, d.rows, d.iterations, d.normal_power = w, h, 3, 5
    d.flags = L.ORT_DENOISE_SAME_SPHERE
    o = L.OrtOutput(k["out"].ctypes.data, 0, L.ORT_FORMAT_RGB32F, L.ORT_PLACE_TILE, 0, 0)
    return d, o, k


def setter(target, **fields):
    def apply(d, o):
        obj = d if target == "d" else o
        for name, v in fields.items():
            if name.startswith("reserved") and target == "d":
                obj.reserved[int(name[-1])] = v
            else:
                setattr(obj, name, v)
    return apply


REFUSED = {
    "null color": setter("d", color=None), "null hits": setter("d", hits=None), "null normals": setter("d", normals=None),
    "null output data": setter("o", data=None),
    "negative width": setter("d", width=-1), "negative rows": setter("d", rows=-1),
    "too many pixels": setter("d", width=1 << 16, rows=(1 << 14) + 1),
    "iterations 0": setter("d", iterations=0), "iterations 7": setter("d", iterations=7),
    "normal_power -1": setter("d", normal_power=-1), "normal_power 8": setter("d", normal_power=8),
    "negative sigma_color": setter("d", sigma_color=-0.5), "nan sigma_color": setter("d", sigma_color=float("nan")),
    "negative sigma_depth": setter("d", sigma_depth=-1.0), "nan sigma_depth": setter("d", sigma_depth=float("nan")),
    "unknown flags": setter("d", flags=2), "reserved 0": setter("d", reserved0=1), "reserved 1": setter("d", reserved1=1),
    "colour pitch below the row": setter("d", color_pitch_bytes=92), "colour pitch odd": setter("d", color_pitch_bytes=98),
    "colour pitch 2^31": setter("d", color_pitch_bytes=1 << 31),
    "frame placement": setter("o", placement=1), "unknown format": setter("o", format=2),
    "output reserved": setter("o", reserved=1), "output pitch below the row": setter("o", row_pitch_bytes=92),
    "output pitch odd": setter("o", row_pitch_bytes=98),
    "on_device disagrees": setter("d", on_device=1), "is_device disagrees": setter("o", is_device=1),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_arguments_leave_the_output_untouched(what):
    lib, L = lib_and_types()
    d, o, k = make_call(L)
    REFUSED[what](d, o)
    assert lib.ort_debug_denoise(C.byref(d), C.byref(o)) == L.ORT_ERR_INVALID_ARG, what
    assert (k["out"] == F(-3.0)).all()


def test_misaligned_pointers_and_null_structs_are_refused():
    lib, L = lib_and_types()
    for field in ("color", "hits", "normals"):
        d, o, k = make_call(L)
        setattr(d, field, getattr(d, field) + 2)
        assert lib.ort_debug_denoise(C.byref(d), C.byref(o)) == L.ORT_ERR_INVALID_ARG
    d, o, k = make_call(L)
    o.data = o.data + 2
    assert lib.ort_debug_denoise(C.byref(d), C.byref(o)) == L.ORT_ERR_INVALID_ARG
    assert lib.ort_debug_denoise(None, C.byref(o)) == L.ORT_ERR_INVALID_ARG
    assert lib.ort_debug_denoise(C.byref(d), None) == L.ORT_ERR_INVALID_ARG
    assert (k["out"] == F(-3.0)).all()


@pytest.mark.parametrize("w,h", [(0, 4), (8, 0), (0, 0)])
def test_an_empty_image_is_ok_and_writes_nothing(w, h):
    lib, L = lib_and_types()
    d, o, k = make_call(L)
    d.width, d.rows = w, h
    assert lib.ort_debug_denoise(C.byref(d), C.byref(o)) == L.ORT_OK
    d.color = d.hits = d.normals = None          # (NULL pointers are accepted for it)
    o.data = None
    assert lib.ort_debug_denoise(C.byref(d), C.byref(o)) == L.ORT_OK
    assert (k["out"] == F(-3.0)).all()


def test_a_valid_call_is_accepted():
    lib, L = lib_and_types()
    d, o, k = make_call(L)
    assert lib.ort_debug_denoise(C.byref(d), C.byref(o)) == L.ORT_OK
    assert not (k["out"] == F(-3.0)).any()


# ---- it denoises --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ds.SCENES)
def test_the_defaults_denoise_a_one_sample_frame(name):
    """MSE against the oracle's 256-sample frame: filtered / unfiltered <= 0.8 at 96 x 64 (a float32
    numpy prototype of the same arithmetic measured 0.591, 0.559 and 0.172)."""
    img, t, sph, n = ds.inputs(name, 96, 64)
    ref, ref64 = ds.frame(name, 96, 64, 256), ds.frame(name, 96, 64, 64)
    assert np.isfinite(img).all() and np.isfinite(ref).all()
    noisy = ds.mse(img, ref)
    assert noisy >= 10 * ds.mse(ref64, ref), "the 1-sample frame is not worth filtering"
    share = float((sph >= 0).mean())
    assert 0.2 < share < 0.8, share                  # hits and misses are both exercised
    got = ds.host(img, t, sph, n, **ds.DEFAULTS)
    ratio = ds.mse(got, ref) / noisy
    print(f"{name}: hit share {share:.3f}, 1-sample MSE {noisy:.5f}, filtered / unfiltered {ratio:.3f}")
    assert ratio <= 0.8
