"""Frames and tiles at the kernels' unit sizes: the table, the cameras and the references that
tests/test_shape_edges.py (host) and tests/test_gpu_shape_edges.py (GPU) share.

The kernels cut a frame into 8 x 8 wave blocks, 16 x 16 tiles, pairs of tiles and 256-pixel
segments (the denoiser, the resolves, the adaptive reduce); the swizzle orders deal workgroups in
groups of 8 or 512, the group deals 16-row bands to ranks.  SHAPES brackets each of these units
with full frames of the chart (chart_scenes.scene(4, 1); frame_sequences.SCENES["deep"] where a
test says "deep"), TILES cuts a 97 x 63 frame into single pixels, rows, columns and band tiles that
run past it.

Under the chart's own camera the extreme shapes see no sphere at all (1x1, 1x2, 2x1, 31x1, 300x1 and
256x1 hit nothing), so every shape has a camera of its own: pitch, zoom and a yaw offset from
chart_scenes.YAW, the first of the grid pitch (0, 5, -5, 10, -10, -15) x zoom (45, 20, 5, 1) x yaw
offset (0, 6, -6, -11) under which the first-sample camera rays of 1, 2 and 5 samples (the
emulation's camera_query_host) meet camera_condition(): at least min(pixels, 4) pixels hit a
sphere, from 2 pixels up at least 2 distinct spheres, from 64 pixels up at least one miss.
tests/test_shape_edges.py asserts it for every shape.

References are the oracle's (oracle.render and its counters) and, for the calls without an oracle
form, the host emulations'; each is computed once per process and read-only."""
import dataclasses
import functools

import numpy as np

import chart_scenes as CS
import frame_sequences as FS

INT_MAX = 2**31 - 1

# "WxH": (group, pitch, zoom, yaw offset)
SHAPES = {
    # A: below a wave block
    "1x1": ("A", 0.0, 1.0, 6.0), "1x2": ("A", 10.0, 20.0, 6.0), "2x1": ("A", 10.0, 5.0, -6.0), "3x5": ("A", 0.0, 45.0, 0.0),
    # B: the 8 x 8 wave block
    "7x9": ("B", 0.0, 45.0, 0.0), "8x8": ("B", 0.0, 45.0, 0.0), "9x7": ("B", 0.0, 45.0, 0.0),
    # C: the 16 x 16 tile
    "15x17": ("C", 0.0, 45.0, 0.0), "16x16": ("C", 0.0, 45.0, 0.0), "17x15": ("C", 0.0, 45.0, 0.0),
    # D: a tile pair, and its hole
    "31x1": ("D", 0.0, 5.0, 6.0), "32x2": ("D", 0.0, 20.0, 0.0), "33x3": ("D", 0.0, 45.0, 6.0),
    # E: a single column or row of tiles
    "1x300": ("E", 0.0, 45.0, 6.0), "300x1": ("E", 0.0, 5.0, 0.0),
    # F: the 256-pixel segment or block
    "255x2": ("F", 0.0, 20.0, 6.0), "256x1": ("F", 0.0, 5.0, 0.0), "257x3": ("F", 0.0, 45.0, 6.0),
    # G: 7, 8 or 9 tiles -- the swizzle's 8-workgroup group
    "112x16": ("G", 0.0, 45.0, 0.0), "128x16": ("G", 0.0, 45.0, 0.0), "144x16": ("G", 0.0, 45.0, 0.0),
    # H: run length 2 of swizzle 2 -- 60 tiles, three groups of 16 and a partial one
    "480x17": ("H", 0.0, 45.0, 0.0),
    # I: 511, 512 or 513 tiles -- swizzle 1's groups; primary rays only
    "8176x16": ("I", 0.0, 45.0, 0.0), "8192x16": ("I", 0.0, 45.0, 0.0), "8208x16": ("I", 0.0, 45.0, 0.0),
}
TILE_FRAME = (97, 63)
# of the 97 x 63 frame, under the chart's own camera: (x0, width, y0, rows, band_height, band_stride)
TILES = {
    "corner_bl": (0, 1, 0, 1, 0, 0), "corner_br": (96, 1, 0, 1, 0, 0), "corner_tl": (0, 1, 62, 1, 0, 0),
    "corner_tr": (96, 1, 62, 1, 0, 0),
    "last_column": (96, 1, 0, 63, 0, 0),
    "top_row": (0, 97, 62, 1, 0, 0),
    "two_by_two": (15, 2, 15, 2, 0, 0),
    "every_other_row": (0, 97, 0, 40, 1, 2),     # past the frame from tile row 32 on
    "band_past_frame": (0, 97, 63, 16, 0, 0),    # wholly past the frame
    "band_first_row_in": (0, 97, 62, 4, 1, 5),   # only its first row inside
}
BAND_TILES = ("every_other_row", "band_past_frame", "band_first_row_in")
SAMPLES = ((1, 1), (2, 4), (5, 6))  # (num_samples, max_depth) of the host comparison

# The row limit (include/ort.h ort_tile): tiles whose last row's pixel row passes 2^31 - 1 are
# refused, (x0, width, y0, rows, band_height, band_stride) of a 48 x 32 frame ...
REFUSED_TILES = {
    "y0_plus_rows": (0, 8, 2147483640, 16, 0, 0),
    "band_stride_2^30": (0, 8, 0, 3, 1, 1 << 30),
    "band_stride_int_max": (0, 8, 40, 4, 2, 2147483647),
    "one_past": (0, 8, 2147483647, 2, 0, 0),
}
# ... and the largest accepted ones, all zeros (the last: rows 40, 41, INT_MAX - 1 and INT_MAX)
LARGEST_TILES = {
    "one_row_at_int_max": (0, 8, 2147483647, 1, 0, 0),
    "eight_rows_to_int_max": (0, 8, 2147483640, 8, 0, 0),
    "band_last_row_int_max": (0, 8, 40, 4, 2, 2147483606),
}
LIMIT_FRAME = (48, 32)


@dataclasses.dataclass(frozen=True)
class Case:
    """A full frame of SHAPES or a tile of TILES: what one call renders."""
    id: str
    group: str       # "A" .. "I", or "T" for a tile
    size: tuple      # (W, H) of the full frame
    tile: tuple      # (x0, width, y0, rows, band_height, band_stride)
    pitch: float = 0.0
    zoom: float = 45.0
    yaw: float = 0.0  # offset from the chart's

    @property
    def pixels(self):
        return self.tile[1] * self.tile[3]

    def ort_tile(self):
        import octreeraytracer_amd as ort
        return ort.Tile(*self.tile)

    def inside(self):
        """(rows,) bool: the tile's rows inside the frame."""
        return FS.pixel_rows(self.tile) < self.size[1]


def _cases():
    out = {}
    for name, (group, pitch, zoom, yaw) in SHAPES.items():
        w, h = (int(v) for v in name.split("x"))
        out[name] = Case(name, group, (w, h), (0, w, 0, h, 0, 0), pitch, zoom, yaw)
    for name, tile in TILES.items():
        out[name] = Case(name, "T", TILE_FRAME, tile)
    return out


CASES = _cases()


def cases(groups, tiles=False, only_tiles=None):
    """The ids of the shapes of `groups` (a string of group letters), then those of the tiles."""
    ids = [c.id for c in CASES.values() if c.group in groups]
    if tiles:
        ids += [n for n in TILES if only_tiles is None or n in only_tiles]
    return ids


def params(case_id, shape=(1, 1), use_octree=1, turn=0.0):
    """FrameParams of the case's camera; turn: degrees of yaw added."""
    import octreeraytracer_amd as ort
    c = CASES[case_id]
    return CS.chart_params(ort, c.size[0], c.size[1], num_samples=shape[0], max_depth=shape[1], use_octree=use_octree,
                           yaw=CS.YAW + c.yaw + turn, pitch=c.pitch, zoom=c.zoom)


def scene(name="d4"):
    return FS.scene(name)


def camera_condition(pixels, sphere):
    """'' or which part of the condition the first hits `sphere` (any shape, -1: a miss) fail."""
    hit = sphere[sphere >= 0]
    if hit.size < min(pixels, 4):
        return f"{hit.size} pixels hit a sphere, fewer than {min(pixels, 4)}"
    if pixels >= 2 and len(np.unique(hit)) < 2:
        return "fewer than 2 distinct spheres"
    if pixels >= 64 and hit.size == sphere.size:
        return "no miss"
    return ""


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def frame(case_id, shape=(1, 1), use_octree=1, scene_name="d4", turn=0.0):
    """(rows, width, 3) float32 of the case: oracle.render; rows past the frame are zeros."""
    from oracle import oracle
    s, t = scene(scene_name)
    x0, w, y0, rows, bh, bs = CASES[case_id].tile
    return _frozen(oracle.render(s, t if use_octree else None, params(case_id, shape, use_octree, turn), x0, y0, w, rows, bh, bs))


@functools.lru_cache(maxsize=None)
def counters(case_id, shape=(1, 1), use_octree=1):
    from oracle import oracle
    s, t = scene()
    x0, w, y0, rows, bh, bs = CASES[case_id].tile
    return oracle.render(s, t if use_octree else None, params(case_id, shape, use_octree), x0, y0, w, rows, bh, bs,
                         counts=True)[1]


@functools.lru_cache(maxsize=None)
def camera(case_id, which="first_sample", num_samples=1, use_octree=1):
    """(rays, t, sphere, normals) of the case's pixels by the host emulation (camera_query_host)."""
    from octreeraytracer_amd.renderer import camera_query_host
    s, t = scene()
    c = CASES[case_id]
    return _frozen(*camera_query_host(s, t if use_octree else None, params(case_id, (num_samples, 1), use_octree),
                                      c.ort_tile(), which=which, normals=True))


@functools.lru_cache(maxsize=None)
def moments(case_id, shape, k):
    """(mean, variance) after k samples of the case's shape[0]-sample chain (accum_moments_host)."""
    from octreeraytracer_amd.renderer import accum_moments_host
    s, t = scene()
    return _frozen(*accum_moments_host(s, t, params(case_id, shape), CASES[case_id].ort_tile(), samples_done=k))


@functools.lru_cache(maxsize=None)
def preview(case_id, shape, k):
    """The picture after k samples (emulate_render_host(samples_done=k))."""
    from octreeraytracer_amd.renderer import emulate_render_host
    s, t = scene()
    return _frozen(emulate_render_host(s, t, params(case_id, shape), CASES[case_id].ort_tile(), samples_done=k)[0])


@functools.lru_cache(maxsize=None)
def adaptive(case_id, shape, passes):
    """(counts, mean, variance) after `passes` (accum_adaptive_host)."""
    from octreeraytracer_amd.renderer import accum_adaptive_host
    s, t = scene()
    return _frozen(*accum_adaptive_host(s, t, params(case_id, shape), CASES[case_id].ort_tile(), passes=list(passes)))


# ---- the denoiser's images ---------------------------------------------------------------------------
DENOISE_SMALL = ((1, 1), (1, 7), (7, 1), (2, 2), (4, 3), (5, 5))           # (W, H)
DENOISE_SEGMENT = ((255, 2), (256, 1), (257, 3), (1, 300))                 # the 256-pixel segment
TERMS_OFF = dict(same_sphere=False, normal_power=0, sigma_color=0.0, sigma_depth=0.0)
TERMS_ON = dict(same_sphere=True, normal_power=5, sigma_color=1.0, sigma_depth=0.5)


def denoise_camera(w, h):
    """The case whose camera guides a w x h image: the shape itself where SHAPES has it, else 17x15's
    camera (the chart's own, which sees a dozen spheres in a few pixels)."""
    return f"{w}x{h}" if f"{w}x{h}" in SHAPES else "17x15"


@functools.lru_cache(maxsize=None)
def denoise_inputs(w, h):
    """(image, t, sphere, normals) of a w x h image: seeded random colours, the pixel-centre guides of
    the shape's camera query."""
    import octreeraytracer_amd as ort
    from octreeraytracer_amd.renderer import camera_query_host
    c = CASES[denoise_camera(w, h)]
    s, t = scene()
    p = CS.chart_params(ort, w, h, yaw=CS.YAW + c.yaw, pitch=c.pitch, zoom=c.zoom)
    _, tt, sph, nrm = camera_query_host(s, t, p, which="pixel_centre", normals=True)
    img = np.random.default_rng(100 * w + h).random((h, w, 3), dtype=np.float32)
    return _frozen(img, tt, sph, nrm)


@functools.lru_cache(maxsize=None)
def denoise_variance(w, h):
    """A seeded (h, w) variance with a pixel that has no estimate (-1) where there is room."""
    v = (np.random.default_rng(7 * w + h).random((h, w), dtype=np.float32) * np.float32(0.02)).astype(np.float32)
    if w * h > 1:
        v.reshape(-1)[w * h // 2] = -1.0
    return _frozen(v)


@functools.lru_cache(maxsize=None)
def denoised(w, h, iterations=3, terms="off", variance=False, gamma=False, fmt="rgb32f"):
    """denoise_host of denoise_inputs(w, h)."""
    from octreeraytracer_amd.renderer import denoise_host
    img, t, sph, nrm = denoise_inputs(w, h)
    kw = dict(TERMS_ON if terms == "on" else TERMS_OFF, iterations=iterations, format=fmt, gamma=gamma)
    if variance:
        kw.update(variance=denoise_variance(w, h), sigma_variance=2.0)
    return _frozen(denoise_host(img, ((t, sph), nrm), **kw))


# ---- output buffers ----------------------------------------------------------------------------------
def describe(case_id, fmt="rgb32f", form="host"):
    """frame_sequences' output description of the case: form "host" (tight, host memory), "device"
    (tight), "pitch" (device, rows 20 bytes apart from tight) or "frame" (placed into a whole frame)."""
    c = CASES[case_id]
    W, H = c.size
    x0, w, y0, rows, bh, bs = c.tile
    bpp = FS.BPP[fmt]
    d = {"fmt": fmt, "place": "frame" if form == "frame" else "tile", "device": form != "host", "pitch": None}
    if form == "frame":
        d.update(row_bytes=W * bpp, stride=W * bpp, rows=H)
    else:
        d.update(row_bytes=w * bpp, stride=w * bpp, rows=rows)
        if form == "pitch":
            d.update(pitch=w * bpp + 20, stride=w * bpp + 20)
    d["nbytes"] = d["rows"] * d["stride"]
    return d


def expected_buffer(case_id, ref, d):
    """Every byte of the buffer after the call: FS.FILL but for the pixels the description covers
    (the float picture's bits or its RGBA8 form; zero words in the rows past the frame under tile
    placement, nothing written for them under frame placement)."""
    c = CASES[case_id]
    H = c.size[1]
    x0, w, y0, rows, bh, bs = c.tile
    want = np.full(d["nbytes"] + FS.SLACK, FS.FILL, np.uint8)
    ys = FS.pixel_rows(c.tile)
    px = FS.pixel_bytes(ref, d["fmt"], ys >= H)
    grid = want[:d["nbytes"]].reshape(d["rows"], d["stride"])
    if d["place"] == "tile":
        grid[:, :d["row_bytes"]] = px
    else:
        at = x0 * FS.BPP[d["fmt"]]
        grid[ys[ys < H], at:at + px.shape[1]] = px[ys < H]
    return want


def differences(got, want, d):
    return FS.first_differences(got, want, d)
