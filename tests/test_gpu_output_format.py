"""Display-format output on the GPU (ort_render_ex, include/ort.h): RGBA8 quantised by the
kernels, a row pitch, and tiles placed into a whole frame.

Every comparison is exact.  The yardstick of a case is the float frame the existing call renders
on the same context (pinned to the reference shaders by tests/test_gpu_parity.py and
tests/test_gpu_repeat_frames.py): the RGBA8 frame must be image.to_srgb8 of it with alpha 255, a
pitched or frame-placed float frame its bit patterns.  The cases are chosen so that each of the
kernels' pixel store sites (ort_kernel.hip store_pixel / store_padding callers) runs in RGBA8:

  shade_direct (trace kernel, tile pairs, split walks)   test_one_bounce_compact, test_split_walks
  shade_direct_padding                                   test_band_tile_padding[compact_b1, pipeline_b2]
  shade_state DIRECT, shade_slot's padding               test_one_bounce_explicit, test_band_tile_padding[explicit_b1]
  shade_state, a path's end in the last sample           test_pipeline_*, test_band_tile_padding[pipeline_b2]
  ort_finalize_kernel (pixel and padding)                test_band_tile_padding[explicit_b2]
  ort_pixel_paths (pixel and padding)                    test_brute_force, test_whole_pixel_paths,
                                                         test_band_tile_padding[pixel_paths_b2]
  ort_sample_resolve (pixel and padding), fixup launch   test_speculating_frames

(Band tiles: rank 1 of 3 of a 177-row frame ends at row 175, so rank 2's tile, 15 padding rows, is
rendered beside it.  Outputs other than ort_render's run ort_shade_first_any at bounce 0 of the
explicit-layout and brute-force pipeline: test_band_tile_padding[explicit_b2].)

Every prefilled buffer is at least as large as its description says, so a wrong address shows
as a failed comparison."""
import ctypes as C

import numpy as np
import pytest

from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.image import to_srgb8
from test_glsl_parity import CANON, inputs

pytestmark = pytest.mark.gpu

FILL = 0xA5
BPP = {"rgb32f": 12, "rgba8": 4}


def check_rgba(rgba, f32, what):
    assert rgba.dtype == np.uint8 and rgba.shape == f32.shape[:2] + (4,), what
    want = to_srgb8(f32)
    bad = int((rgba[..., :3] != want).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels are not to_srgb8 of the float frame"
    assert (rgba[..., 3] == 255).all(), f"{what}: alpha"


def both(r, p, what, tile=None):
    """The float frame by the existing call, then RGBA8 on the same context, compared."""
    f32 = r.render(p, tile)
    rgba = r.render(p, tile, format="rgba8")
    check_rgba(rgba, f32, what)
    return f32, rgba


def device_bytes(n):
    import torch
    return torch.full((n,), FILL, dtype=torch.uint8, device="cuda:0")


def as_out(buf, fmt):
    """The byte buffer as the tensor Renderer.render takes for fmt."""
    import torch
    return buf.view(torch.float32) if fmt == "rgb32f" else buf


def host(buf, rows, pitch):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:rows * pitch].reshape(rows, pitch)


@pytest.fixture(scope="module")
def odd(ort):
    """m8_d7_odd_b2's scene and shape (333 x 177: no multiple of the 16 x 16 tile or the band)."""
    c = CANON["cases"]["m8_d7_odd_b2"]
    s, t, p = inputs(ort, c)
    assert (p.width, p.height, p.num_samples, p.max_depth) == (333, 177, 1, 2)
    return s, t, p


@pytest.fixture(scope="module")
def c1_frames(ort, scene_c1):
    """scene_c1 at 192 x 144, 1 x 1: the float frame and the RGBA8 frame, tight (read-only)."""
    s, t = scene_c1
    p = ort.FrameParams.default_camera(192, 144)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        f32, rgba = both(r, p, "c1")
    f32.flags.writeable = False
    rgba.flags.writeable = False
    return p, f32, rgba


@pytest.fixture(scope="module")
def odd_frames(ort, odd):
    """The 333 x 177 frame (1 bounce), float and RGBA8, tight (read-only)."""
    import dataclasses
    s, t, p = odd
    p = dataclasses.replace(p, max_depth=1)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        f32, rgba = both(r, p, "odd")
    f32.flags.writeable = False
    rgba.flags.writeable = False
    return p, f32, rgba


@pytest.mark.parametrize("pairs", [0, 1])
def test_one_bounce_compact(ort, scene_c1, c1_frames, pairs):
    s, t = scene_c1
    p, f32_ref, _ = c1_frames
    with ort.Renderer(0) as r:
        r.upload(s, t)
        assert r.info()["layout"] == "compact"
        r.set_tile_pairs(pairs)
        f32, _ = both(r, p, f"compact 1 x 1, tile pairs {pairs}")
        assert np.array_equal(f32.view(np.uint32), f32_ref.view(np.uint32))


def test_one_bounce_explicit(ort, scene_c1, c1_frames):
    s, t = scene_c1
    p, f32_ref, _ = c1_frames
    with ort.Renderer(0) as r:
        r.set_layout(L.ORT_LAYOUT_EXPLICIT)
        r.upload(s, t)
        assert r.info()["layout"] == "explicit"
        f32, _ = both(r, p, "explicit 1 x 1")
        assert np.array_equal(f32.view(np.uint32), f32_ref.view(np.uint32))


def test_brute_force(ort):
    c = CANON["cases"]["brute_d4"]
    s, t, p = inputs(ort, c)
    assert (p.width, p.height, p.max_depth, p.use_octree) == (128, 96, 4, 0)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        both(r, p, "brute force, 4 bounces")


def test_split_walks(ort, scene_c2):
    s, t = scene_c2
    p = ort.FrameParams.default_camera(320, 180)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_split_heavy(20)
        f32 = r.render(p)  # records the walks' steps: the next frames split the heavy ones
        for k in range(2):
            check_rgba(r.render(p, format="rgba8"), f32, f"split walks, RGBA8 frame {k + 1}")
        assert np.array_equal(r.render(p).view(np.uint32), f32.view(np.uint32))


def test_pipeline_two_bounces_odd_size(ort, odd):
    s, t, p = odd
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_pixel_paths(0)
        both(r, p, "pipeline, 333 x 177, 2 bounces")


def test_pipeline_two_samples_four_bounces(ort, scene_c2):
    s, t = scene_c2
    p = ort.FrameParams.default_camera(192, 108, num_samples=2, max_depth=4)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_pixel_paths(0)
        both(r, p, "pipeline, 2 samples x 4 bounces")


def test_whole_pixel_paths(ort):
    c = CANON["cases"]["prebuilt_spp4_d8"]
    s, t, p = inputs(ort, c)
    assert (p.width, p.height) == (160, 120)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_pixel_paths(1)
        both(r, p, "whole-pixel paths, 4 samples x 8 bounces")


def test_speculating_frames(ort):
    """config.h's default scene, 16 samples x 8 bounces: from the second frame of the shape on the
    samples are traced in parallel (three launches) and ort_sample_resolve or the fixup launch
    writes the pixel.  Then a band tile of the same frame, whose padding rows ort_sample_resolve
    writes."""
    from octreeraytracer_amd.distributed import rank_tile
    c = CANON["cases"]["config_default"]
    s, t, p = inputs(ort, c)
    import dataclasses
    p = dataclasses.replace(p, width=200, height=150)
    assert (p.num_samples, p.max_depth, s.n) == (16, 8, 100)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.set_pixel_paths(1)
        r.set_pixel_speculate(1)
        f32 = r.render(p)
        seen = []
        for k in range(3):
            rgba = r.render(p, format="rgba8")
            seen.append(r.frame_trace_times_ms(1)[0][1])
            check_rgba(rgba, f32, f"speculating, RGBA8 frame {k + 1}")
        assert seen[1:] == [3, 3], seen
        tile = rank_tile(p.width, p.height, 1, 3)
        ys = tile.pixel_rows(p.height)
        assert (ys >= p.height).any()
        for k in range(3):
            band = r.render(p, tile, format="rgba8")
            n = r.frame_trace_times_ms(1)[0][1]
            inside = ys < p.height
            check_rgba(band[inside], f32[ys[inside]], f"speculating band tile, frame {k + 1}")
            assert not band[~inside].any(), f"speculating band tile, frame {k + 1}: padding rows"
        assert n == 3, n


@pytest.mark.parametrize("variant", ["pipeline_b2", "compact_b1", "explicit_b1", "explicit_b2", "pixel_paths_b2"])
def test_band_tile_padding(ort, odd, variant):
    """The band tiles of ranks 1 and 2 of 3 of the 333 x 177 frame, tile placement: the rows past
    the frame are all-zero words (alpha included), the others the full frame's rows.  (Rank 1's
    last band is rows 160-175, all inside the frame; rank 2's is rows 176-191: one row of the
    frame and 15 padding rows.)"""
    import dataclasses
    from octreeraytracer_amd.distributed import rank_tile
    s, t, p = odd
    p = dataclasses.replace(p, max_depth=1 if variant.endswith("b1") else 2)
    with ort.Renderer(0) as r:
        if variant.startswith("explicit"):
            r.set_layout(L.ORT_LAYOUT_EXPLICIT)
        r.upload(s, t)
        r.set_pixel_paths(1 if variant.startswith("pixel_paths") else 0)
        full_f32, full_rgba = both(r, p, f"{variant}: full frame")
        for rank in (1, 2):
            tile = rank_tile(p.width, p.height, rank, 3)
            ys = tile.pixel_rows(p.height)
            inside = ys < p.height
            assert inside.any() and (~inside).sum() == (0, 0, 15)[rank]
            band = np.full((tile.rows, tile.width, 4), FILL, np.uint8)
            r.render(p, tile, out=band, format="rgba8")
            assert np.array_equal(band[inside], full_rgba[ys[inside]]), (variant, rank)
            assert not band[~inside].any(), f"{variant}, rank {rank}: padding rows are not zero words"
            # the float band tile is untouched by the new path: the full frame's bit patterns, zeros
            fband = r.render(p, tile)
            assert np.array_equal(fband[inside].view(np.uint32), full_f32[ys[inside]].view(np.uint32))
            assert not fband[~inside].view(np.uint32).any()


@pytest.mark.parametrize("fmt", ["rgb32f", "rgba8"])
def test_pitch(ort, scene_c1, c1_frames, fmt):
    s, t = scene_c1
    p, f32, rgba = c1_frames
    tight = (f32.view(np.uint8) if fmt == "rgb32f" else rgba).reshape(144, 192 * BPP[fmt])
    pitch = (192 + 5) * BPP[fmt]
    buf = device_bytes(144 * pitch)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.render(p, out=as_out(buf, fmt), format=fmt, row_pitch=pitch)
        got = host(buf, 144, pitch)
    assert np.array_equal(got[:, :192 * BPP[fmt]], tight)
    assert (got[:, 192 * BPP[fmt]:] == FILL).all()


@pytest.mark.parametrize("fmt", ["rgb32f", "rgba8"])
def test_frame_placement_of_band_tiles(ort, odd, odd_frames, fmt):
    """The three ranks' band tiles of world 3 rendered into one frame: the full-frame render, bit
    for bit; 16 spare rows after the frame stay as prefilled (padding rows write nothing)."""
    from octreeraytracer_amd.distributed import rank_tile
    s, t, _ = odd
    p, f32, rgba = odd_frames
    W, H, bpp = p.width, p.height, BPP[fmt]
    want = (f32.view(np.uint8) if fmt == "rgb32f" else rgba).reshape(H, W * bpp)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        for spare in (0, 16):
            buf = device_bytes((H + spare) * W * bpp)
            for rank in range(3):
                r.render(p, rank_tile(W, H, rank, 3), out=as_out(buf, fmt), format=fmt, place="frame")
            got = host(buf, H + spare, W * bpp)
            assert np.array_equal(got[:H], want), (fmt, spare)
            assert (got[H:] == FILL).all(), (fmt, spare)


@pytest.mark.parametrize("fmt", ["rgb32f", "rgba8"])
def test_sub_rectangle_into_a_frame(ort, odd, odd_frames, fmt):
    s, t, _ = odd
    p, f32, rgba = odd_frames
    W, H, bpp = p.width, p.height, BPP[fmt]
    full = (f32.view(np.uint8) if fmt == "rgb32f" else rgba).reshape(H, W, bpp)
    want = np.full((H, W, bpp), FILL, np.uint8)
    want[20:70, 37:137] = full[20:70, 37:137]
    buf = device_bytes(H * W * bpp)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        r.render(p, ort.Tile(37, 100, 20, 50), out=as_out(buf, fmt), format=fmt, place="frame")
        got = host(buf, H, W * bpp).reshape(H, W, bpp)
    assert np.array_equal(got, want)


def test_host_output(ort, scene_c1, c1_frames):
    s, t = scene_c1
    p, _, rgba = c1_frames
    with ort.Renderer(0) as r:
        r.upload(s, t)
        out = np.full((144, 192, 4), FILL, np.uint8)
        assert r.render(p, out=out, format="rgba8") is out
        assert np.array_equal(out, rgba)
        pitch = (192 + 5) * 4
        out = np.full((144, pitch), FILL, np.uint8)
        r.render(p, out=out, format="rgba8", row_pitch=pitch)
        assert np.array_equal(out[:, :192 * 4].reshape(144, 192, 4), rgba)
        assert (out[:, 192 * 4:] == FILL).all()


def test_invalid_descriptions(ort, scene_c1, c1_frames):
    s, t = scene_c1
    p, _, rgba = c1_frames
    buf = device_bytes(144 * 192 * 4 + 16)
    hbuf = np.empty((144, 192, 4), np.uint8)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        pc, tc = p.to_c(), ort.Tile.full(p).to_c()

        def call(data, is_device, fmt, place, reserved, pitch):
            o = L.OrtOutput(data, is_device, fmt, place, reserved, pitch)
            return r._lib.ort_render_ex(r._ctx, C.byref(pc), C.byref(tc), C.byref(o), None)

        dev, hst = buf.data_ptr(), hbuf.ctypes.data
        cases = {"format": (dev, 1, 7, L.ORT_PLACE_TILE, 0, 0),
                 "placement": (dev, 1, L.ORT_FORMAT_RGBA8, 5, 0, 0),
                 "reserved": (dev, 1, L.ORT_FORMAT_RGBA8, L.ORT_PLACE_TILE, 1, 0),
                 "row_pitch_bytes": (dev, 1, L.ORT_FORMAT_RGBA8, L.ORT_PLACE_TILE, 0, 192 * 4 + 2),
                 "row_pitch_bytes ": (dev, 1, L.ORT_FORMAT_RGBA8, L.ORT_PLACE_TILE, 0, 191 * 4),
                 "data": (dev + 2, 1, L.ORT_FORMAT_RGBA8, L.ORT_PLACE_TILE, 0, 0),
                 "placement ": (hst, 0, L.ORT_FORMAT_RGBA8, L.ORT_PLACE_FRAME, 0, 0)}
        for field, args in cases.items():
            assert call(*args) == L.ORT_ERR_INVALID_ARG, field
            msg = r._lib.ort_last_error(r._ctx).decode()
            assert field.strip() in msg, (field, msg)
            assert np.array_equal(r.render(p, format="rgba8"), rgba), f"the render after a refused {field}"
        import torch
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == FILL).all()  # nothing was launched


@pytest.mark.parametrize("devices,transport", [([0, 0, 0], L.ORT_GROUP_TRANSPORT_COPY), ([0], L.ORT_GROUP_TRANSPORT_RCCL)])
def test_group(ort, scene_c2, devices, transport):
    import torch
    from octreeraytracer_amd.group import RenderGroup
    s, t = scene_c2
    p = ort.FrameParams.default_camera(320, 180)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        f32, rgba = both(r, p, "single context")
    with RenderGroup(devices, transport) as g:
        g.upload(s, t)
        assert np.array_equal(g.render(p, format="rgba8"), rgba)
        dev = torch.full((180, 320, 4), FILL, dtype=torch.uint8, device="cuda:0")
        g.render(p, out=dev, format="rgba8")
        assert np.array_equal(dev.cpu().numpy(), rgba)
        hout = np.full((180, 320, 4), FILL, np.uint8)
        tk = g.submit(p, hout, format="rgba8")
        g.wait(tk)
        assert np.array_equal(hout, rgba)
        assert np.array_equal(g.render(p).view(np.uint32), f32.view(np.uint32))  # a float frame afterwards
