"""Display-format output without a GPU: the kernels' RGBA8 quantiser (render_core.h pack_rgba8,
through the analysis library) against image.to_srgb8, the ort_output bindings against the
header, Renderer.render's argument checks, and the Python side (assemble, the writers) on uint8
frames.  The GPU half is tests/test_gpu_output_format.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from octreeraytracer_amd import image

ROOT = Path(__file__).resolve().parents[1]


def pack(rgb):
    """ort_debug_pack_rgba8 of an (n, 3) float32 array -> (n, 4) uint8 (memory order)."""
    from octreeraytracer_amd import _lib
    lib = _lib.analysis_lib()
    rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    out = np.empty(len(rgb), np.uint32)
    _lib.acheck(lib.ort_debug_pack_rgba8(_lib.fptr(rgb), len(rgb), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
    return out.view(np.uint8).reshape(-1, 4)


def check_values(ort, x):
    """Every value of the float32 array x in each of the three channels."""
    x = np.asarray(x, np.float32).ravel()
    n = -(-len(x) // 3) * 3
    x = np.concatenate([x, np.zeros(n - len(x), np.float32)])
    for shift in range(3):  # each value passes through R, G and B
        rgb = np.roll(x, shift).reshape(-1, 3)
        got = pack(rgb)
        want = image.to_srgb8(rgb)
        assert want.dtype == np.uint8 and want.shape == rgb.shape
        assert np.array_equal(got[:, :3], want), rgb[(got[:, :3] != want).any(axis=1)][:4]
        assert (got[:, 3] == 255).all()


def test_quantiser_random(ort):
    x = np.random.default_rng(20261019).uniform(-0.5, 1.5, 1_000_000).astype(np.float32)
    check_values(ort, x)


def threshold(ort, k):
    """The smallest float32 in [0, 1] that to_srgb8 maps to k + 1 (bisection over the bit
    patterns: positive floats order as their bits do)."""
    q = lambda bits: int(image.to_srgb8(np.array([bits], np.uint32).view(np.float32))[0])
    lo, hi = int(np.float32(0.0).view(np.uint32)), int(np.float32(1.0).view(np.uint32))
    assert q(lo) <= k < q(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if q(mid) <= k:
            lo = mid
        else:
            hi = mid
    return hi


def test_quantiser_thresholds(ort):
    """to_srgb8 is monotone, so agreement at each of its 255 steps (and two floats either side)
    is agreement on [0, 1]."""
    bits = []
    for k in range(255):
        t = threshold(ort, k)
        step = image.to_srgb8(np.array([t - 1, t], np.uint32).view(np.float32))
        assert list(step) == [k, k + 1]
        bits += [t - 2, t - 1, t, t + 1, t + 2]
    check_values(ort, np.array(bits, np.uint32).view(np.float32))


def test_quantiser_special_values(ort):
    one = np.float32(1.0)
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1.0, np.nextafter(one, np.float32(2.0)),
                  np.nextafter(one, np.float32(0.0)), 0.5, -1.0, 2.0, 3.4e38, -3.4e38], np.float32)
    with np.errstate(all="ignore"):
        check_values(ort, x)
    got = pack(np.array([[np.nan, np.inf, -np.inf], [1.0, 0.0, 1e-40]], np.float32))
    assert got.tolist() == [[0, 255, 0, 255], [255, 0, 0, 255]]


def test_output_constants_and_struct_match_the_header():
    from octreeraytracer_amd import _lib
    text = (ROOT / "include" / "ort.h").read_text()
    defs = dict(re.findall(r"#define\s+(ORT_(?:FORMAT|PLACE)_[A-Z0-9_]+)\s+(-?\d+)\b", text))
    assert sorted(defs) == ["ORT_FORMAT_RGB32F", "ORT_FORMAT_RGBA8", "ORT_PLACE_FRAME", "ORT_PLACE_TILE"]
    for k, v in defs.items():
        assert getattr(_lib, k) == int(v), k
    # typedef struct ort_output: a pointer, four int32, an int64
    body = re.search(r"typedef struct ort_output \{(.*?)\} ort_output;", re.sub(r"/\*.*?\*/", "", text, flags=re.S),
                     flags=re.S).group(1)
    fields = re.findall(r"(void\*|int32_t|int64_t)\s+(\w+);", body)
    assert fields == [("void*", "data"), ("int32_t", "is_device"), ("int32_t", "format"), ("int32_t", "placement"),
                      ("int32_t", "reserved"), ("int64_t", "row_pitch_bytes")]
    assert [f[0] for f in _lib.OrtOutput._fields_] == [n for _, n in fields]
    assert ctypes.sizeof(_lib.OrtOutput) == ctypes.sizeof(ctypes.c_void_p) + 4 * 4 + 8 == 32
    assert _lib.OrtOutput.row_pitch_bytes.offset == 24
    for name in ("ort_render_ex", "ort_group_submit_fmt", "ort_group_render_fmt"):
        assert name in _lib.EXPORTED_SYMBOLS


def bare_renderer(ort):
    r = object.__new__(ort.Renderer)  # no GPU context needed: the checks come first
    r._ctx = ctypes.c_void_p()
    r._lib = None
    r.device = 0
    return r


@pytest.mark.parametrize("bad", ["float32_for_rgba8", "uint8_for_rgb32f", "short", "short_for_pitch", "pitch_odd",
                                 "pitch_small", "frame_numpy", "frame_none", "format", "place"])
def test_render_rejects_a_bad_description_before_the_abi(ort, bad):
    r = bare_renderer(ort)
    p = ort.FrameParams.default_camera(32, 16)
    kw = {"float32_for_rgba8": dict(out=np.empty((16, 32, 4), np.float32), format="rgba8"),
          "uint8_for_rgb32f": dict(out=np.empty((16, 32, 12), np.uint8)),
          "short": dict(out=np.empty((15, 32, 4), np.uint8), format="rgba8"),
          "short_for_pitch": dict(out=np.empty((16, 32, 4), np.uint8), format="rgba8", row_pitch=36 * 4),
          "pitch_odd": dict(out=np.empty((16, 34, 4), np.uint8), format="rgba8", row_pitch=32 * 4 + 2),
          "pitch_small": dict(out=np.empty((16, 32, 4), np.uint8), format="rgba8", row_pitch=31 * 4),
          "frame_numpy": dict(out=np.empty((16, 32, 4), np.uint8), format="rgba8", place="frame"),
          "frame_none": dict(format="rgba8", place="frame"),
          "format": dict(format="rgb8"),
          "place": dict(place="window")}[bad]
    with pytest.raises(ValueError):
        r.render(p, **kw)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_assemble_uint8_frames(ort, world):
    from octreeraytracer_amd.distributed import assemble, rank_tile
    H, W = 40, 8
    frame = np.random.default_rng(world).integers(0, 256, (H, W, 4), dtype=np.uint8)
    tiles = []
    for r in range(world):
        t = rank_tile(W, H, r, world)
        tile = np.zeros((t.rows, W, 4), np.uint8)
        for j, y in enumerate(t.pixel_rows(H)):
            if 0 <= y < H:
                tile[j] = frame[y]
        tiles.append(tile)
    rows = tiles[0].shape[0]
    assert all(t.shape[0] == rows for t in tiles)
    if world > 1:
        assert H % 16 != 0 and rows * world > H  # some rank's last band is cut by the frame's end
    got = assemble(np.stack(tiles), H, world)
    assert got.dtype == np.uint8 and got.shape == (H, W, 4)
    assert np.array_equal(got, frame)
    out = np.empty((H, W, 4), np.uint8)
    assert assemble(np.stack(tiles), H, world, out=out) is out and np.array_equal(out, frame)


def test_writers_take_rgba8_frames(ort, tmp_path):
    x = np.random.default_rng(5).uniform(-0.2, 1.2, (12, 20, 3)).astype(np.float32)
    rgba = np.empty((12, 20, 4), np.uint8)
    rgba[..., :3] = image.to_srgb8(x)
    rgba[..., 3] = 255
    assert np.array_equal(image.to_srgb8(rgba), rgba[..., :3])
    for writer, ext in ((image.write_png, "png"), (image.write_ppm, "ppm")):
        writer(tmp_path / f"f.{ext}", x)
        writer(tmp_path / f"u.{ext}", rgba)
        assert (tmp_path / f"f.{ext}").read_bytes() == (tmp_path / f"u.{ext}").read_bytes()
