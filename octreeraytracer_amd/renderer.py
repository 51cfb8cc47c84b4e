"""Device renderer: the GL path of the reference replaced by the gfx950 kernel (libort.so).

``Renderer`` owns one ort_ctx (one GPU).  ``upload`` = setupBuffers (src/raytracer.cpp:74-152),
``render`` = the per-frame uniforms + glDrawArrays (src/raytracer.cpp:491-499) followed by a
read of the frame (the reference never reads pixels back; this returns them).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from .scene import (DEFAULT_CAMERA_POSITION, DEFAULT_PITCH, DEFAULT_YAW, DEFAULT_ZOOM, FlatOctree, SphereSet,
                    camera_view)


@dataclass
class FrameParams:
    """The shader uniforms (glsl:13-18, 48-53)."""

    width: int
    height: int
    num_samples: int = 1
    max_depth: int = 1
    use_octree: int = 1
    view: np.ndarray = field(default_factory=lambda: camera_view())
    camera_position: tuple = DEFAULT_CAMERA_POSITION
    camera_zoom: float = DEFAULT_ZOOM

    def to_c(self) -> L.OrtParams:
        p = L.OrtParams()
        p.width, p.height = int(self.width), int(self.height)
        p.num_samples, p.max_depth, p.use_octree = int(self.num_samples), int(self.max_depth), int(self.use_octree)
        v = np.asarray(self.view, np.float32).reshape(16)
        for i in range(16):
            p.view[i] = float(v[i])
        for i in range(3):
            p.camera_position[i] = float(self.camera_position[i])
        p.camera_zoom = float(self.camera_zoom)
        return p

    @staticmethod
    def default_camera(width, height, num_samples=1, max_depth=1, use_octree=1, position=DEFAULT_CAMERA_POSITION,
                       yaw=DEFAULT_YAW, pitch=DEFAULT_PITCH, zoom=DEFAULT_ZOOM) -> "FrameParams":
        return FrameParams(width, height, num_samples, max_depth, use_octree, camera_view(position, yaw, pitch),
                           tuple(position), zoom)


@dataclass
class Tile:
    """Rows/columns to render; see ort_tile in include/ort.h.  Output row j is pixel row
    y0 + (j // band_height) * band_stride + j % band_height (GL rows: y = 0 at the bottom)."""

    x0: int
    width: int
    y0: int
    rows: int
    band_height: int = 0
    band_stride: int = 0

    @staticmethod
    def full(p: FrameParams) -> "Tile":
        return Tile(0, p.width, 0, p.height)

    def to_c(self) -> L.OrtTile:
        t = L.OrtTile()
        t.x0, t.width, t.y0, t.rows = int(self.x0), int(self.width), int(self.y0), int(self.rows)
        t.band_height, t.band_stride = int(self.band_height), int(self.band_stride)
        return t

    def pixel_rows(self, height: int) -> np.ndarray:
        j = np.arange(self.rows, dtype=np.int64)  # 64-bit: a refused tile's rows pass 2^31 - 1 (ort_tile)
        y =self.y0 + (j // self.band_height) * self.band_stride + j % self.band_height if self.band_height > 0 \
            else self.y0 + j
        return y


class Renderer:
    def __init__(self, device: int = 0):
        self._lib = L.lib()
        self._ctx = C.c_void_p()
        L.check(self._lib.ort_create(device, C.byref(self._ctx)))
        self.device = device

    # -- lifecycle -------------------------------------------------------------------
    def close(self):
        if self._ctx:
            self._lib.ort_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        L.check(rc, self._ctx)

    # -- scene -----------------------------------------------------------------------
    def set_layout(self, layout: int):
        """Force ORT_LAYOUT_COMPACT / ORT_LAYOUT_EXPLICIT (-1 = auto) for the next upload."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_FORCE_LAYOUT, int(layout)))

    def set_exact_traversal(self, on: bool):
        """Disable (True) / enable the sign-specialised fast walk; pixels are identical either way."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_EXACT_TRAVERSAL, int(bool(on))))

    def set_launch_times(self, on: int):
        """ORT_OPT_LAUNCH_TIMES: 1 (default) times every trace launch (last_trace_ms, trace_times_ms);
        0 times only the frame (last_kernel_ms) -- fewer event packets per frame; same pixels."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_LAUNCH_TIMES, int(on)))

    def set_pixel_paths(self, mode: int):
        """ORT_OPT_PIXEL_PATHS: -1 (default) auto, 0 the per-bounce pipeline, 1 whole-pixel paths in one
        launch wherever they apply (same pixels)."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_PIXEL_PATHS, int(mode)))

    def set_pixel_lds_scene(self, on: int):
        """ORT_OPT_PIXEL_LDS_SCENE: 1 (default) small scenes walked from LDS copies in whole-pixel paths."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_PIXEL_LDS_SCENE, int(on)))

    def set_pixel_speculate(self, mode: int):
        """ORT_OPT_PIXEL_SPECULATE: whole-pixel paths trace a pixel's samples in parallel from last
        frame's per-sample RNG end states (checked, re-traced where they moved); -1 (default) / 1
        on, 0 off."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_PIXEL_SPECULATE, int(mode)))

    def set_pixel_heavy_first(self, mode: int):
        """ORT_OPT_PIXEL_HEAVY_FIRST: whole-pixel paths take the previous frame's heaviest 8x8
        blocks first; -1 (default) for frames of 2+ samples, 0 off, 1 on."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_PIXEL_HEAVY_FIRST, int(mode)))

    def set_xcd_swizzle(self, mode: int):
        """Workgroup -> tile order (ORT_OPT_XCD_SWIZZLE): 2 runs of raster tiles per XCD, 1
        128x128-pixel super-tiles per XCD, 0 raster, -1 (default) raster on small one-tile-workgroup
        tiles and runs otherwise; same pixels."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_XCD_SWIZZLE, int(mode)))

    def set_sort_paths(self, mode: int):
        """Order of the alive paths between bounces (same pixels): 0 slot order, 1 radix sort of
        every slot by coherence key, 2 (default) full-key radix sort of the appended alive list,
        sized by the same bounce's list length in the previous frame of this shape (+1/64 + 1024;
        a longer list goes on unsorted) -- no host wait (include/ort.h ORT_OPT_SORT_PATHS)."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_SORT_PATHS, int(mode)))

    def set_persistent(self, on):
        """Persistent trace kernel with lane refill for the bounce >= 1 traces: 2 (default) on, 0 off
        (same pixels).  1 (every trace persistent) was removed: OrtError."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_PERSISTENT, int(on)))

    def set_kid_skip(self, mode: int):
        """Rejected-sphere skip of one-sphere leaf children (kid_table.h); same pixels.  0 off,
        1 on (node records and kid entries from the interleaved copy), 2 on with the two
        separate arrays (testing)."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_KID_SKIP, int(mode)))

    def set_sort_bound(self, bound: int):
        """Testing (ORT_OPT_SORT_BOUND): force the list sort's size; 0 = the previous-frame hint."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_SORT_BOUND, int(bound)))

    def set_heavy_first(self, steps: int):
        """ORT_OPT_HEAVY_FIRST: bounce lists ordered by last frame's walk steps in classes >= 4T, >= 2T,
        >= T (T = steps, default 64), the rest last; 0 off (coherence order only).  Same pixels."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_HEAVY_FIRST, int(steps)))

    def set_heavy_prio(self, steps: int):
        """ORT_OPT_HEAVY_PRIO: camera-ray waves holding a walk of >= steps (last frame) run at raised
        issue priority; 0 off (default 150).  Same pixels."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_HEAVY_PRIO, int(steps)))

    def set_split_heavy(self, steps: int):
        """ORT_OPT_SPLIT_HEAVY: camera rays whose walk took >= steps (last frame) are walked by 8 lanes
        each, their subtrees dealt round robin, beside the per-tile kernel; 0 off; -1 (default) 200 on
        tiles of at most 2^21 pixels, off on larger ones.  Same pixels."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_SPLIT_HEAVY, int(steps)))

    def set_split_level(self, level: int):
        """ORT_OPT_SPLIT_LEVEL: the level of the subtrees a split walk deals (0: depth - 5)."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_SPLIT_LEVEL, int(level)))

    def set_tile_pairs(self, on: int):
        """ORT_OPT_TILE_PAIRS: camera-ray workgroups of two tiles, each wave a heavy and a light 64-pixel
        block by last frame's walk steps; 0 a tile per workgroup; -1 (default) pairs on tiles of more
        than 2^21 pixels.  Same pixels."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_TILE_PAIRS, int(on)))

    def set_debug_flags(self, flags: int):
        """ORT_OPT_DEBUG_FLAGS (analysis, A/B only): 1 no trace-timing events, 2 no queued heavy scan."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_DEBUG_FLAGS, int(flags)))

    def set_cost_order(self, on: int):
        """ORT_OPT_COST_ORDER: 1 (default) camera rays dealt to waves by last frame's walk cost; 0 fixed blocks."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_COST_ORDER, int(on)))

    def set_refill(self, lanes: int):
        """Persistent trace: refill a wave once at least `lanes` of its 64 lanes are idle."""
        self._check(self._lib.ort_set_option(self._ctx, L.ORT_OPT_REFILL, int(lanes)))

    def upload(self, spheres: SphereSet, tree: FlatOctree | None):
        cr = np.ascontiguousarray(spheres.center_radius, np.float32)
        ma = np.ascontiguousarray(spheres.mat_albedo, np.float32)
        fr = np.ascontiguousarray(spheres.fuzz_ri, np.float32)
        if tree is None:
            self._check(self._lib.ort_upload_scene(self._ctx, L.fptr(cr), L.fptr(ma), L.fptr(fr), spheres.n,
                                                   None, None, None, None, None, 0, None, 0))
            return
        nmin = np.ascontiguousarray(tree.node_min, np.float32)
        nmax = np.ascontiguousarray(tree.node_max, np.float32)
        co = np.ascontiguousarray(tree.children_offset, np.int32)
        oo = np.ascontiguousarray(tree.objects_offset, np.int32)
        cnt = np.ascontiguousarray(tree.object_count, np.int32)
        idx = np.ascontiguousarray(tree.object_indices, np.int32)
        self._check(self._lib.ort_upload_scene(self._ctx, L.fptr(cr), L.fptr(ma), L.fptr(fr), spheres.n,
                                               L.fptr(nmin), L.fptr(nmax), L.iptr(co), L.iptr(oo), L.iptr(cnt),
                                               tree.n_nodes, L.iptr(idx), tree.n_indices))

    def build_scene(self, spheres: SphereSet, max_depth: int, max_spheres_per_node: int, keep_tree: bool = False):
        """Build the octree on the GPU (ort_build_scene: the reference builder's exact output)
        and make it this renderer's scene.  keep_tree: keep the reference-layout tree on the
        device for export_octree()."""
        cr = np.ascontiguousarray(spheres.center_radius, np.float32)
        ma = np.ascontiguousarray(spheres.mat_albedo, np.float32)
        fr = np.ascontiguousarray(spheres.fuzz_ri, np.float32)
        self._check(self._lib.ort_build_scene(self._ctx, L.fptr(cr), L.fptr(ma), L.fptr(fr), spheres.n,
                                              int(max_depth), int(max_spheres_per_node), int(bool(keep_tree))))

    def export_octree(self) -> FlatOctree:
        """The kept GPU-built tree (build_scene(keep_tree=True)) as a host FlatOctree."""
        i = self.info()
        n, k = i["n_nodes"], i["n_indices"]
        nmin = np.empty((n, 3), np.float32)
        nmax = np.empty((n, 3), np.float32)
        co = np.empty(n, np.int32)
        oo = np.empty(n, np.int32)
        cnt = np.empty(n, np.int32)
        idx = np.empty(max(k, 1), np.int32)
        self._check(self._lib.ort_scene_export_octree(self._ctx, L.fptr(nmin), L.fptr(nmax), L.iptr(co), L.iptr(oo),
                                                      L.iptr(cnt), L.iptr(idx)))
        return FlatOctree(nmin, nmax, co, oo, cnt, idx[:k])

    def stream_handle(self) -> int:
        """The context's own (non-blocking) HIP stream, e.g. for torch.cuda.ExternalStream."""
        h = C.c_void_p()
        self._check(self._lib.ort_get_stream(self._ctx, C.byref(h)))
        return h.value or 0

    def last_build_ms(self) -> float:
        ms = C.c_float()
        self._check(self._lib.ort_last_build_ms(self._ctx, C.byref(ms)))
        return ms.value

    def info(self) -> dict:
        i = L.OrtSceneInfo()
        self._check(self._lib.ort_scene_get_info(self._ctx, C.byref(i)))
        return {"n_spheres": i.n_spheres, "n_nodes": i.n_nodes, "n_indices": i.n_indices,
                "layout": "compact" if i.layout == L.ORT_LAYOUT_COMPACT else "explicit",
                "tree_depth": i.tree_depth, "device_bytes": i.device_bytes}

    # -- frames ----------------------------------------------------------------------
    def render(self, params: FrameParams, tile: Tile | None = None, out=None, stream=None, *,
               format: str = "rgb32f", row_pitch: int | None = None, place: str = "tile"):
        """Render a tile.  out: None (returns a new (rows, width, 3) float32 numpy array),
        a numpy array, or a device pointer (int) / torch CUDA tensor on this device.
        stream: None (synchronous) or a hipStream_t handle (int), e.g.
        torch.cuda.Stream().cuda_stream.  The null stream (handle 0, torch's default
        stream) cannot be told apart from "no stream": it renders synchronously.

        format: "rgb32f" (3 float32 per pixel) or "rgba8" (4 uint8: R, G, B, A = 255, each
        channel ``image.to_srgb8`` of the float pixel, quantised by the kernel; out=None then
        returns a (rows, width, 4) uint8 array).  row_pitch: bytes from one output row to the
        next (a multiple of 4, at least the row's bytes; None: tight); the bytes between rows
        are left untouched.  place: "tile" (output row j is tile row j) or "frame" (out is a
        whole width x height frame on the device, the pixel (x, y) lands at row y, column x, and
        band padding rows are not written): ort_render_ex (include/ort.h)."""
        tile = tile or Tile.full(params)
        p, t = params.to_c(), tile.to_c()
        s = C.c_void_p(int(stream)) if stream else None
        o, out = self._output("render", params, tile, out, format, row_pitch, place)
        self._check(self._lib.ort_render_ex(self._ctx, C.byref(p), C.byref(t), C.byref(o), s))
        return out

    def _output(self, what, params, tile, out, format, row_pitch, place):
        """The ort_output of a call `what` (render, Accumulation.step) that writes the tile into out
        -- None (a new numpy array), a numpy array, a device pointer or a torch CUDA tensor -- and
        the object the call returns: the buffer checked against the bytes the description covers."""
        if format not in L.FORMATS:
            raise ValueError(f"{what}: format must be one of {sorted(L.FORMATS)} (got {format!r})")
        if place not in L.PLACEMENTS:
            raise ValueError(f"{what}: place must be one of {sorted(L.PLACEMENTS)} (got {place!r})")
        fmt, plc = L.FORMATS[format], L.PLACEMENTS[place]
        bpp = L.FORMAT_BPP[fmt]
        np_dtype, channels = (np.float32, 3) if fmt == L.ORT_FORMAT_RGB32F else (np.uint8, 4)
        # the bytes the description covers: rows of row_bytes, pitch apart
        row_bytes = (params.width if plc == L.ORT_PLACE_FRAME else tile.width) * bpp
        n_rows = params.height if plc == L.ORT_PLACE_FRAME else tile.rows
        pitch = row_bytes if row_pitch is None else int(row_pitch)
        if pitch % 4 != 0:
            raise ValueError(f"{what}: row_pitch must be a multiple of 4 (got {pitch})")
        if pitch < row_bytes:
            raise ValueError(f"{what}: row_pitch {pitch} is below the row's {row_bytes} bytes")
        need = (n_rows - 1) * pitch + row_bytes if n_rows > 0 else 0
        if out is None:
            if plc == L.ORT_PLACE_FRAME or row_pitch is not None:
                raise ValueError(f"{what}: place='frame' and row_pitch describe a caller's buffer: pass out")
            out = np.empty((tile.rows, tile.width, channels), np_dtype)
        o = L.OrtOutput(None, 0, fmt, plc, 0, 0 if row_pitch is None else pitch)
        if isinstance(out, np.ndarray):
            if plc == L.ORT_PLACE_FRAME:
                raise ValueError(f"{what}: place='frame' writes device memory: out must be a device pointer or tensor")
            if out.dtype != np_dtype or not out.flags.c_contiguous or out.nbytes < need:
                raise ValueError(f"{what}: out must be a C-contiguous {np.dtype(np_dtype).name} array of >= {need} "
                                 f"bytes (got {out.dtype}, {out.nbytes} bytes, contiguous={out.flags.c_contiguous})")
            o.data = out.ctypes.data_as(C.c_void_p)
            return o, out
        ptr = out.data_ptr() if hasattr(out, "data_ptr") else int(out)
        if hasattr(out, "numel"):  # a torch tensor: the format's dtype, contiguous, on this context's GPU
            import torch
            t_dtype = torch.float32 if fmt == L.ORT_FORMAT_RGB32F else torch.uint8
            nbytes = out.numel() * out.element_size()
            if out.dtype != t_dtype or not out.is_contiguous() or nbytes < need:
                raise ValueError(f"{what}: out must be a contiguous {t_dtype} tensor of >= {need} bytes "
                                 f"(got {out.dtype}, {nbytes} bytes, contiguous={out.is_contiguous()})")
            if out.device.type != "cuda" or out.device.index != self.device:
                raise ValueError(f"{what}: out is on {out.device}, the context renders on cuda:{self.device}")
        o.data, o.is_device = C.c_void_p(ptr), 1
        return o, out

    # -- progressive frames -----------------------------------------------------------
    def accumulate(self, params: FrameParams, tile: Tile | None = None, moments: bool = False,
                   adaptive: bool = False) -> "Accumulation":
        """Begin accumulating the frame `params` (its num_samples is the target N) over several
        calls: ort_accum_begin (include/ort.h).  Allocates the per-pixel state, traces nothing.
        moments: the passes also keep each pixel's sum of squared sample luminances (ort_accum_begin_ex
        with ORT_ACCUM_MOMENTS, 4 bytes more per path slot), which ``Accumulation.moments`` turns
        into a per-pixel variance; the pictures are the same bit for bit.
        adaptive: ORT_ACCUM_ADAPTIVE (it implies moments, 4 bytes more again): every pixel keeps its
        own sample count, and ``Accumulation.step_adaptive`` traces only the pixels whose mean is
        still noisy; ``step`` traces them all, as on a moments accumulation."""
        return Accumulation(self, params, tile or Tile.full(params), moments, adaptive)

    def history(self, width: int, rows: int) -> "History":
        """A preview's history across camera moves for tiles of rows x width pixels (ort_history_begin,
        include/ort.h): allocates 64 bytes per pixel, launches nothing.  ``History.update`` reprojects
        it into each new frame and blends the frame's sample in."""
        return History(self, width, rows)

    # -- ray queries ------------------------------------------------------------------
    def _device_arg(self, who, x, what, dtype_name, need):
        """The device address of x, a torch CUDA tensor on this device or a pointer (int)."""
        if hasattr(x, "data_ptr"):
            nbytes = x.numel() * x.element_size()
            if str(x.dtype) != "torch." + dtype_name or not x.is_contiguous() or nbytes < need:
                raise ValueError(f"{who}: {what} must be a contiguous {dtype_name} tensor of >= {need} bytes "
                                 f"(got {x.dtype}, {nbytes} bytes, contiguous={x.is_contiguous()})")
            if x.device.type != "cuda" or x.device.index != self.device:
                raise ValueError(f"{who}: {what} is on {x.device}, the context traces on cuda:{self.device}")
            return x.data_ptr()
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise ValueError(f"{who}: {what} must be a torch CUDA tensor or a device pointer (int)")
        return int(x)

    def trace_rays(self, rays, *, use_octree=True, sort=False, normals=False, out=None, stream=None, n=None,
                   mode="drawn", t_range=None):
        """What does each ray hit, and where (ort_trace_rays, include/ort.h): per ray the shader's
        intersectScene(ray, 0.001, MAXFLOAT) -- t (in units of the direction's length; directions
        are used as given) and the index of the hit sphere in the uploaded arrays, (0.0, -1) for a
        miss; with normals the unit-sphere normal ((o + t d) - c) / r, zeros for a miss.  With
        use_octree the walk is the one the pixels are made with: it leaves the tree after the first
        leaf holding a hit, so the sphere is the one drawn, not always the nearest.

        rays: a C-contiguous (n, 6) float32 numpy array (origin, direction) -> returns
        (t float32 (n,), sphere int32 (n,)) and, with normals=True, an (n, 3) float32 array; out
        may be an (n, 2) int32 array to receive the records {t bits, sphere}.
        rays: a contiguous (n, 6) float32 torch CUDA tensor on this device, or a device pointer
        (int) with n -> everything stays on the device: returns out, an (n, 2) int32 tensor of
        {t bits, sphere} (allocated when None; a pointer needs out given), and with normals the
        (n, 3) float32 normals tensor (normals=True allocates it; a tensor or pointer is used).
        sort: walk the rays in coherence order (ORT_QUERY_SORT; same records, same order).
        stream: as render().

        mode: "drawn" (the above), "nearest" -- the nearest hit inside the ray's interval, the lowest
        sphere index among equals, the same record with and without the octree -- or "any" -- some
        sphere with a hit inside the interval, the first one found (ort_trace_rays_ex).
        t_range: None = (0.001, MAXFLOAT) for every ray, else {t_min, t_max} per ray, in units of the
        direction's length: with host rays a C-contiguous (n, 2) float32 array, with device rays a
        contiguous (n, 2) float32 CUDA tensor or a device pointer.  0 <= t_min < t_max, else the ray
        misses; not with mode="drawn", whose interval is the shader's."""
        flags = L.ORT_QUERY_SORT if sort else 0
        s = C.c_void_p(int(stream)) if stream else None
        if mode not in L.QUERY_MODES:
            raise ValueError(f"trace_rays: mode must be one of {sorted(L.QUERY_MODES)} (got {mode!r})")
        if t_range is not None and mode == "drawn":
            raise ValueError('trace_rays: t_range needs mode="nearest" or "any": the drawn record is the shader\'s interval')
        ex = mode != "drawn"
        qx = L.OrtRayQueryEx(L.OrtRayQuery(None, 0, None, None, 0, 1 if use_octree else 0, flags, 0), None,
                             L.QUERY_MODES[mode], (C.c_int32 * 3)(0, 0, 0))
        q = qx.base

        def trace():  # the defaults call ort_trace_rays as ever
            if ex:
                return self._lib.ort_trace_rays_ex(self._ctx, C.byref(qx), s)
            return self._lib.ort_trace_rays(self._ctx, C.byref(q), s)
        if isinstance(rays, np.ndarray):
            if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 6 or not rays.flags.c_contiguous:
                raise ValueError(f"trace_rays: rays must be a C-contiguous (n, 6) float32 array (got {rays.dtype}, "
                                 f"shape {rays.shape}, contiguous={rays.flags.c_contiguous})")
            nr = rays.shape[0]
            if n is not None and int(n) != nr:
                raise ValueError(f"trace_rays: n = {n} but rays holds {nr}")
            if out is None:
                out = np.empty((nr, 2), np.int32)
            if (not isinstance(out, np.ndarray) or out.dtype != np.int32 or not out.flags.c_contiguous or
                    out.nbytes < 8 * nr):
                raise ValueError(f"trace_rays: out must be a C-contiguous int32 numpy array of >= {8 * nr} bytes")
            if not isinstance(normals, (bool, np.bool_)):
                raise ValueError("trace_rays: with host rays, normals is True or False")
            if t_range is not None:
                if (not isinstance(t_range, np.ndarray) or t_range.dtype != np.float32 or t_range.ndim != 2 or
                        t_range.shape != (nr, 2) or not t_range.flags.c_contiguous):
                    raise ValueError(f"trace_rays: with host rays, t_range must be a C-contiguous ({nr}, 2) float32 array "
                                     f"(got {getattr(t_range, 'dtype', type(t_range))}, shape {getattr(t_range, 'shape', None)})")
                qx.t_range = t_range.ctypes.data_as(C.c_void_p)
            nrm = np.zeros((nr, 3), np.float32) if normals else None
            q.rays, q.n_rays = rays.ctypes.data_as(C.c_void_p), nr
            q.hits = out.ctypes.data_as(C.c_void_p)
            q.normals = nrm.ctypes.data_as(C.c_void_p) if normals else None
            self._check(trace())
            rec = out.reshape(-1)[:2 * nr].reshape(nr, 2)
            t, sph = np.ascontiguousarray(rec[:, 0]).view(np.float32), np.ascontiguousarray(rec[:, 1])
            return (t, sph, nrm) if normals else (t, sph)

        if hasattr(rays, "data_ptr"):
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise ValueError(f"trace_rays: rays must have shape (n, 6) (got {tuple(rays.shape)})")
            nr = rays.shape[0]
            if n is not None and int(n) != nr:
                raise ValueError(f"trace_rays: n = {n} but rays holds {nr}")
        else:
            if n is None or int(n) < 0:
                raise ValueError("trace_rays: a device pointer needs n, the number of rays")
            nr = int(n)
            if out is None or (isinstance(normals, (bool, np.bool_)) and normals):
                raise ValueError("trace_rays: a device pointer needs out (and normals, where wanted) given")
        q.rays, q.n_rays = C.c_void_p(self._device_arg("trace_rays", rays, "rays", "float32", 24 * nr)), nr
        if out is None or (isinstance(normals, (bool, np.bool_)) and normals):
            import torch
            dev = torch.device("cuda", self.device)
            if out is None:
                out = torch.empty((nr, 2), dtype=torch.int32, device=dev)
            if isinstance(normals, (bool, np.bool_)) and normals:
                normals = torch.empty((nr, 3), dtype=torch.float32, device=dev)
        want_normals = not isinstance(normals, (bool, np.bool_))
        q.hits = C.c_void_p(self._device_arg("trace_rays", out, "out", "int32", 8 * nr))
        q.normals = C.c_void_p(self._device_arg("trace_rays", normals, "normals", "float32", 12 * nr)) if want_normals else None
        if t_range is not None:
            if hasattr(t_range, "data_ptr") and (t_range.dim() != 2 or tuple(t_range.shape) != (nr, 2)):
                raise ValueError(f"trace_rays: t_range must have shape ({nr}, 2) (got {tuple(t_range.shape)})")
            qx.t_range = C.c_void_p(self._device_arg("trace_rays", t_range, "t_range", "float32", 8 * nr))
        q.on_device = 1
        self._check(trace())
        return (out, normals) if want_normals else out

    def occluded(self, origins, targets, *, eps=1e-3, use_octree=True):
        """Segment visibility: per pair (a, b) of the (n, 3) host arrays, is any sphere hit strictly
        between the two points?  One ORT_QUERY_ANY ray per pair from a along the unit direction
        (b - a) / |b - a| with the interval (eps, |b - a| - eps), all formed in float32.  Returns a
        bool array (n,); a pair with |b - a| <= 2 eps (coincident points among them) is not occluded."""
        a = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
        if a.shape != b.shape:
            raise ValueError(f"occluded: {a.shape[0]} origins but {b.shape[0]} targets")
        eps = np.float32(eps)
        if not eps >= 0:
            raise ValueError(f"occluded: eps must be >= 0 (got {eps})")
        d = b - a
        with np.errstate(all="ignore"):
            length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
            ok = length > np.float32(2) * eps  # (NaN: not ok)
            unit = np.where(ok[:, None], d / np.where(ok, length, np.float32(1))[:, None], np.float32(0)).astype(np.float32)
        rays = np.ascontiguousarray(np.concatenate([a, unit], axis=1), np.float32)
        t_range = np.empty((len(a), 2), np.float32)
        t_range[:, 0] = eps
        t_range[:, 1] = np.where(ok, length - eps, np.float32(0))  # (eps, 0) or (0, 0): an empty interval, a miss
        if len(a) == 0:
            return np.zeros(0, bool)
        _, sph = self.trace_rays(rays, use_octree=use_octree, mode="any", t_range=t_range)
        return (sph >= 0) & ok

    # -- camera queries ---------------------------------------------------------------
    def trace_camera(self, params: FrameParams, tile: Tile | None = None, *, which: str = "first_sample", rays=False,
                     normals=False, out=None, stream=None, hits: bool = True):
        """Each tile pixel's camera ray and what it hits (ort_trace_camera, include/ort.h): the ray
        the shader makes for the pixel, walked as ``trace_rays`` walks a caller's ray.

        which: "first_sample" -- the ray of sample 0 of params.num_samples, RNG draws, jitter and
        lens offset included: with num_samples = 1 the first intersection of the pixel's only
        path -- or "pixel_centre", the pinhole ray through the pixel centre (no RNG, the same for
        every num_samples).  Records are in the tile's output order (row j as ``Tile.pixel_rows``
        maps it, GL rows); rows past the frame hold a miss, a zero normal and a zero ray.

        Host (out None or a numpy array, rays and normals True / False): returns t float32 and
        sphere int32, each (rows, width) -- (0.0, -1) for a miss -- then, where asked, normals
        (rows, width, 3) and rays (rows, width, 6: origin, direction).  out may be a C-contiguous
        int32 array of at least 2 * rows * width elements to receive the records {t bits, sphere}.
        Device (any of out, rays, normals a torch CUDA tensor on this device or a device pointer):
        everything stays on the device; out receives {t bits, sphere} int32 records, rays 6 and
        normals 3 float32 per pixel; rays=True / normals=True / out=None allocate tensors shaped
        (rows, width, 2 | 6 | 3).  Returns out, then normals, then rays, those that were asked for
        (one object when it is the only one).
        hits=False with rays: ray generation only -- nothing is walked, no scene is needed;
        returns the rays.  stream: as render()."""
        tile = tile or Tile.full(params)
        if which not in L.CAMERA_RAYS:
            raise ValueError(f"trace_camera: which must be one of {sorted(L.CAMERA_RAYS)} (got {which!r})")
        rows, width = int(tile.rows), int(tile.width)
        if rows < 0 or width < 0:
            raise ValueError("trace_camera: negative tile size")
        n = rows * width
        is_flag = lambda x: isinstance(x, (bool, np.bool_))  # noqa: E731
        want_rays = not is_flag(rays) or bool(rays)
        want_normals = not is_flag(normals) or bool(normals)
        if not hits and (not want_rays or want_normals or out is not None):
            raise ValueError("trace_camera: hits=False is ray generation only: rays, and neither normals nor out")
        p, t = params.to_c(), tile.to_c()
        s = C.c_void_p(int(stream)) if stream else None
        q = L.OrtCameraQuery(None, None, None, 0, L.CAMERA_RAYS[which])
        device = any(x is not None and not is_flag(x) and not isinstance(x, np.ndarray) for x in (out, rays, normals))
        if not device:
            if not is_flag(rays) or not is_flag(normals):
                raise ValueError("trace_camera: with host output, rays and normals are True or False")
            if hits:
                if out is None:
                    out = np.empty((n, 2), np.int32)
                if out.dtype != np.int32 or not out.flags.c_contiguous or out.nbytes < 8 * n:
                    raise ValueError(f"trace_camera: out must be a C-contiguous int32 numpy array of >= {8 * n} bytes")
                q.hits = out.ctypes.data_as(C.c_void_p)
            nrm = np.zeros((rows, width, 3), np.float32) if want_normals else None
            ray = np.zeros((rows, width, 6), np.float32) if want_rays else None
            q.normals = nrm.ctypes.data_as(C.c_void_p) if want_normals else None
            q.rays = ray.ctypes.data_as(C.c_void_p) if want_rays else None
            self._check(self._lib.ort_trace_camera(self._ctx, C.byref(p), C.byref(t), C.byref(q), s))
            if not hits:
                return ray
            rec = out.reshape(-1)[:2 * n].reshape(n, 2)
            res = (np.ascontiguousarray(rec[:, 0]).view(np.float32).reshape(rows, width),
                   np.ascontiguousarray(rec[:, 1]).reshape(rows, width))
            return res + ((nrm,) if want_normals else ()) + ((ray,) if want_rays else ())

        def allocate(last, dtype_name):
            import torch
            return torch.empty((rows, width, last), dtype=getattr(torch, dtype_name), device=torch.device("cuda", self.device))

        if hits and out is None:
            out = allocate(2, "int32")
        if is_flag(rays) and rays:
            rays = allocate(6, "float32")
        if is_flag(normals) and normals:
            normals = allocate(3, "float32")
        if hits:
            q.hits = C.c_void_p(self._device_arg("trace_camera", out, "out", "int32", 8 * n))
        if want_normals:
            q.normals = C.c_void_p(self._device_arg("trace_camera", normals, "normals", "float32", 12 * n))
        if want_rays:
            q.rays = C.c_void_p(self._device_arg("trace_camera", rays, "rays", "float32", 24 * n))
        q.on_device = 1
        self._check(self._lib.ort_trace_camera(self._ctx, C.byref(p), C.byref(t), C.byref(q), s))
        res = ((out,) if hits else ()) + ((normals,) if want_normals else ()) + ((rays,) if want_rays else ())
        return res[0] if len(res) == 1 else res

    def pick(self, params: FrameParams, x: int, y: int, *, which: str = "pixel_centre"):
        """The sphere under pixel (x, y): (sphere, t, point) from a one-pixel camera query --
        sphere the index in the uploaded arrays (-1: nothing there, t = 0.0 and point = the ray's
        origin), point = origin + t * direction in float32, shape (3,).  y is a GL row (0 at the bottom):
        for a cursor at window row wy, top row 0, pass y = params.height - 1 - wy.  which: as
        ``trace_camera``; the default is the ray through the pixel centre, "first_sample" with
        num_samples = 1 picks what a one-sample frame drew at the pixel."""
        t, sphere, ray = self.trace_camera(params, Tile(int(x), 1, int(y), 1), which=which, rays=True)
        o, d = ray[0, 0, :3], ray[0, 0, 3:]
        point = (o + (t[0, 0] * d).astype(np.float32)).astype(np.float32)
        return int(sphere[0, 0]), float(t[0, 0]), point

    def trace_radiance(self, rays, states, *, max_depth, paths=1, use_octree=True, sort=False, normalize=False,
                       gamma=False, states_out=False, out=None, stream=None, n=None):
        """What each ray sees (ort_trace_radiance, include/ort.h): per ray the mean of `paths`
        evaluations of the shader's radiance() of at most max_depth bounces, chained through the
        ray's RNG state as a pixel's samples are -- bit for bit what the frames are made of.

        rays: (n, 6) float32 (origin, direction; unit directions, or normalize=True for the
        shader's normalize).  states: (n, 2) float32, each component in [0, 1) (``rng_states``); a
        ray whose state is not gets zeros and its state back.  gamma: pow(mean, 1/2.2) as the last
        lines of the shader's main().  sort: walk the rays in coherence order (same records).
        Host (numpy arrays): returns the (n, 3) float32 radiance -- out may be a C-contiguous
        float32 array of >= 3 n elements to receive it -- and with states_out=True also the (n, 2)
        end states; states_out may be an (n, 2) float32 array, `states` itself included.
        Device (torch CUDA tensors on this device, or device pointers with n): everything stays on
        the device; returns out, an (n, 3) float32 tensor (allocated when None; pointers need out
        given), and with states_out (True allocates it; a tensor -- `states` itself is allowed --
        or a pointer is used) the end states.  stream: as render()."""
        who = "trace_radiance"
        max_depth, paths = int(max_depth), int(paths)  # (their ranges: the ABI's refusal)
        flags = ((L.ORT_QUERY_SORT if sort else 0) | (L.ORT_RADIANCE_NORMALIZE if normalize else 0) |
                 (L.ORT_RADIANCE_GAMMA if gamma else 0))
        s = C.c_void_p(int(stream)) if stream else None
        q = L.OrtRadianceQuery(None, 0, None, None, None, 0, 1 if use_octree else 0, max_depth, paths, flags, 0)
        is_flag = lambda x: isinstance(x, (bool, np.bool_))  # noqa: E731
        want_states = not is_flag(states_out) or bool(states_out)

        def host_array(x, what, cols, nr):
            if (not isinstance(x, np.ndarray) or x.dtype != np.float32 or x.ndim != 2 or x.shape != (nr, cols) or
                    not x.flags.c_contiguous):
                raise ValueError(f"{who}: {what} must be a C-contiguous ({nr}, {cols}) float32 array "
                                 f"(got {getattr(x, 'dtype', type(x))}, shape {getattr(x, 'shape', None)})")
            return x

        if isinstance(rays, np.ndarray):
            if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 6 or not rays.flags.c_contiguous:
                raise ValueError(f"{who}: rays must be a C-contiguous (n, 6) float32 array (got {rays.dtype}, "
                                 f"shape {rays.shape}, contiguous={rays.flags.c_contiguous})")
            nr = rays.shape[0]
            if n is not None and int(n) != nr:
                raise ValueError(f"{who}: n = {n} but rays holds {nr}")
            host_array(states, "with host rays, states", 2, nr)
            if out is None:
                out = np.empty((nr, 3), np.float32)
            if (not isinstance(out, np.ndarray) or out.dtype != np.float32 or not out.flags.c_contiguous or
                    out.nbytes < 12 * nr):
                raise ValueError(f"{who}: out must be a C-contiguous float32 numpy array of >= {12 * nr} bytes")
            if is_flag(states_out):
                states_out = np.empty((nr, 2), np.float32) if states_out else None
            else:
                host_array(states_out, "with host rays, states_out", 2, nr)
            q.rays, q.n_rays = rays.ctypes.data_as(C.c_void_p), nr
            q.states = states.ctypes.data_as(C.c_void_p)
            q.radiance = out.ctypes.data_as(C.c_void_p)
            q.states_out = states_out.ctypes.data_as(C.c_void_p) if want_states else None
            self._check(self._lib.ort_trace_radiance(self._ctx, C.byref(q), s))
            rad = out.reshape(-1)[:3 * nr].reshape(nr, 3)
            return (rad, states_out) if want_states else rad

        if hasattr(rays, "data_ptr"):
            if rays.dim() != 2 or rays.shape[1] != 6:
                raise ValueError(f"{who}: rays must have shape (n, 6) (got {tuple(rays.shape)})")
            nr = rays.shape[0]
            if n is not None and int(n) != nr:
                raise ValueError(f"{who}: n = {n} but rays holds {nr}")
        else:
            if n is None or int(n) < 0:
                raise ValueError(f"{who}: a device pointer needs n, the number of rays")
            nr = int(n)
            if out is None or (is_flag(states_out) and states_out):
                raise ValueError(f"{who}: a device pointer needs out (and states_out, where wanted) given")
        if hasattr(states, "data_ptr") and (states.dim() != 2 or tuple(states.shape) != (nr, 2)):
            raise ValueError(f"{who}: states must have shape ({nr}, 2) (got {tuple(states.shape)})")
        q.rays, q.n_rays = C.c_void_p(self._device_arg(who, rays, "rays", "float32", 24 * nr)), nr
        q.states = C.c_void_p(self._device_arg(who, states, "states", "float32", 8 * nr))
        if out is None or (is_flag(states_out) and states_out):
            import torch
            dev = torch.device("cuda", self.device)
            if out is None:
                out = torch.empty((nr, 3), dtype=torch.float32, device=dev)
            if is_flag(states_out) and states_out:
                states_out = torch.empty((nr, 2), dtype=torch.float32, device=dev)
        q.radiance = C.c_void_p(self._device_arg(who, out, "out", "float32", 12 * nr))
        q.states_out = C.c_void_p(self._device_arg(who, states_out, "states_out", "float32", 8 * nr)) if want_states else None
        q.on_device = 1
        self._check(self._lib.ort_trace_radiance(self._ctx, C.byref(q), s))
        return (out, states_out) if want_states else out

    # -- denoiser ---------------------------------------------------------------------
    def denoise(self, image, guides=None, *, params: FrameParams | None = None, tile: Tile | None = None,
                iterations: int = 3, sigma_color: float = 0.0, sigma_depth: float = 0.0, normal_power: int = 5,
                same_sphere: bool = True, format: str = "rgb32f", row_pitch: int | None = None, out=None, stream=None,
                variance=None, sigma_variance: float | None = None, gamma: bool = False):
        """Filter a few-sample picture with the guided a-trous filter (ort_denoise, include/ort.h):
        `iterations` passes of a 5x5 B3-spline kernel with step 1, 2, 4, ..., whose taps are weighted
        by the guides -- normals (normal_power squarings of the clamped dot product), depth
        (sigma_depth > 0) and, with sigma_color > 0, the colours themselves -- and, with same_sphere,
        never cross from one sphere (or the sky) to another.  Made for the one-sample preview of a
        moving camera; with many samples it blurs more than it removes unless sigma_color is on.

        image: (rows, width, 3) float32, a numpy array or a torch CUDA tensor on this device (then
        everything stays there); rows may be a pitch apart (a column slice of a wider array).
        guides: (hits, normals) as ``trace_camera`` returns them for the same pixels -- hits an int32
        array of {t bits, sphere} records or the pair (t, sphere), normals (rows, width, 3) float32
        -- of the image's kind (numpy or tensors).  None: the pixel-centre guides of params and tile,
        traced here (``trace_camera(params, tile, which="pixel_centre", normals=True)``).
        params, tile: the frame and tile the image was rendered with.  A banded tile is refused: its
        rows are not neighbours in the frame.  Rows with y >= height are neither filtered nor used
        as taps and come out as ``render`` writes them (zeros).  Within 2 (2^iterations - 1) pixels
        of the tile's border the result differs from the whole frame's filter.
        format, row_pitch, out, stream: as ``render`` (place is "tile"); out may be the image itself
        (in place).
        variance: None, or the (rows, width) float32 variance of the image's luminance, of the image's
        kind, as ``Accumulation.moments`` returns it beside the linear mean: adds the variance-guided
        term of ort_denoise_ex, which only takes taps within sigma_variance (default
        DEFAULT_SIGMA_VARIANCE) standard deviations of the pixel's luminance and so closes itself as
        the picture converges.  gamma: the output is pow(result, 1/2.2), the render path's: filter
        the linear mean and get the display picture.  Without all three the call is ort_denoise.
        Returns out."""
        who = "denoise"
        device = not isinstance(image, np.ndarray)
        rows, width, pitch, color = _denoise_image(who, image, self.device if device else None)
        real = rows
        if tile is not None and params is None:
            raise ValueError(f"{who}: tile needs params")
        if params is not None:
            tile = tile or Tile.full(params)
            real = _denoise_tile_rows(who, params, tile, rows, width)
        if guides is None:
            if params is None:
                raise ValueError(f"{who}: guides=None traces the guides of params (and tile): pass params")
            if device:
                import torch
                dev = torch.device("cuda", self.device)
                hits = torch.empty((rows, width, 2), dtype=torch.int32, device=dev)
                nrm = torch.empty((rows, width, 3), dtype=torch.float32, device=dev)
                self.trace_camera(params, tile, which="pixel_centre", normals=nrm, out=hits, stream=stream)
            else:
                t, sph, nrm = self.trace_camera(params, tile, which="pixel_centre", normals=True, stream=stream)
                hits = (t, sph)
            guides = (hits, nrm)
        hits, nrm, keep = _denoise_guides(who, guides, rows, width, self if device else None)
        if out is None and device:
            import torch
            fmt_t, ch = (torch.float32, 3) if format == "rgb32f" else (torch.uint8, 4)
            if row_pitch is not None:
                raise ValueError(f"{who}: row_pitch describes a caller's buffer: pass out")
            out = torch.empty((rows, width, ch), dtype=fmt_t, device=torch.device("cuda", self.device))
        if device and isinstance(out, np.ndarray):
            raise ValueError(f"{who}: a device image needs a device out (a torch CUDA tensor or a pointer)")
        if not device and out is not None and not isinstance(out, np.ndarray):
            raise ValueError(f"{who}: a host image needs a numpy out")
        o, out = self._output(who, None, Tile(0, width, 0, rows), out, format, row_pitch, "tile")
        if real < rows and not isinstance(out, np.ndarray) and not hasattr(out, "numel"):
            raise ValueError(f"{who}: a tile reaching past the frame needs out as a tensor (its padding rows are zeroed)")
        d = _denoise_desc(color, pitch, hits, nrm, width, real, device, iterations, sigma_color, sigma_depth, normal_power,
                          same_sphere)
        s = C.c_void_p(int(stream)) if stream else None
        if variance is None and sigma_variance is None and not gamma:
            self._check(self._lib.ort_denoise(self._ctx, C.byref(d), C.byref(o), s))
        else:
            x, keep_v = _denoise_desc_ex(who, d, variance, sigma_variance, gamma, rows, width, real, self if device else None)
            self._check(self._lib.ort_denoise_ex(self._ctx, C.byref(x), C.byref(o), s))
            del keep_v
        del keep
        if real < rows:  # after the call: a refused one leaves out untouched
            _denoise_zero_rows(who, out, real, rows, o.row_pitch_bytes or width * L.FORMAT_BPP[o.format],
                               width * L.FORMAT_BPP[o.format], self.device if device else None)
        return out

    def last_denoise_ms(self) -> float:
        """The last denoise's kernels (the pack pass and the iterations), from HIP events on its stream."""
        ms = C.c_float()
        self._check(self._lib.ort_last_denoise_ms(self._ctx, C.byref(ms)))
        return ms.value

    def last_query_ms(self) -> float:
        """The last trace_rays', trace_camera's or trace_radiance's kernels (a sort included), from HIP events on its stream."""
        ms = C.c_float()
        self._check(self._lib.ort_last_query_ms(self._ctx, C.byref(ms)))
        return ms.value

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._check(self._lib.ort_last_kernel_ms(self._ctx, C.byref(ms)))
        return ms.value

    def last_trace_ms(self) -> float:
        """First trace kernel of the last frame (camera rays + octree walk; the dominant kernel)."""
        ms = C.c_float()
        self._check(self._lib.ort_last_trace_ms(self._ctx, C.byref(ms)))
        return ms.value

    def trace_times_ms(self, n: int) -> list:
        """Trace-kernel durations (ms) of the last n frames (n <= 64), oldest first."""
        buf = (C.c_float * max(1, n))()
        k = self._lib.ort_trace_times_ms(self._ctx, int(n), buf)
        if k < 0:
            L.check(-k, self._ctx)
        return [buf[i] for i in range(k)]

    def frame_trace_times_ms(self, n: int):
        """Per frame (last n <= 64, oldest first): (summed ms of all its trace kernels, launches)."""
        buf = (C.c_float * max(1, n))()
        nl = (C.c_int32 * max(1, n))()
        k = self._lib.ort_frame_trace_times_ms(self._ctx, int(n), buf, nl)
        if k < 0:
            L.check(-k, self._ctx)
        return [(buf[i], nl[i]) for i in range(k)]

    def count_traffic(self, params: FrameParams, tile: Tile | None = None) -> dict:
        tile = tile or Tile.full(params)
        p, t = params.to_c(), tile.to_c()
        counts = (C.c_uint64 * L.ORT_COUNT_N)()
        self._check(self._lib.ort_count_traffic(self._ctx, C.byref(p), C.byref(t), counts))
        return dict(zip(L.COUNT_NAMES, [int(v) for v in counts]))


class Accumulation:
    """A frame's samples accumulated over several calls (``Renderer.accumulate``; ort_accum_* in
    include/ort.h).  ``step(n)`` traces the next n samples of every pixel and returns the picture
    of the samples done so far -- divided by the samples done, so every step's picture is a
    frame; with all of them done it is ``Renderer.render``'s frame bit for bit, whatever the steps.
    A context manager: leaving it frees the state (as ``close`` does; the renderer's ``close``
    frees what is left)."""

    def __init__(self, renderer: Renderer, params: FrameParams, tile: Tile, moments: bool = False, adaptive: bool = False):
        self._r = renderer
        self._h = C.c_void_p()
        self.params, self.tile = params, tile
        self.is_adaptive = bool(adaptive)
        self.keeps_moments = bool(moments) or self.is_adaptive
        self._guides = None
        p, t = params.to_c(), tile.to_c()
        if self.keeps_moments:
            flags = L.ORT_ACCUM_ADAPTIVE if self.is_adaptive else L.ORT_ACCUM_MOMENTS
            renderer._check(renderer._lib.ort_accum_begin_ex(renderer._ctx, C.byref(p), C.byref(t), flags,
                                                             C.byref(self._h)))
        else:
            renderer._check(renderer._lib.ort_accum_begin(renderer._ctx, C.byref(p), C.byref(t), C.byref(self._h)))

    def close(self):
        if self._h and self._r._ctx:
            self._r._check(self._r._lib.ort_accum_free(self._r._ctx, self._h))
        self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        i = L.OrtAccumInfo()
        self._r._check(self._r._lib.ort_accum_get_info(self._h, C.byref(i)))
        return {"samples_done": i.samples_done, "samples_total": i.samples_total, "device_bytes": i.device_bytes}

    @property
    def done(self) -> int:
        return self.info()["samples_done"]

    @property
    def total(self) -> int:
        return self.info()["samples_total"]

    @property
    def finished(self) -> bool:
        i = self.info()
        return i["samples_done"] >= i["samples_total"]

    def step(self, n: int = 1, out=None, stream=None, *, format: str = "rgb32f", row_pitch: int | None = None,
             place: str = "tile"):
        """Trace the next min(n, total - done) samples of every pixel and write the picture of the
        samples done so far; on a finished accumulation, write the finished frame again.  out,
        stream, format, row_pitch, place: as ``Renderer.render``, which this returns like;
        out=False accumulates without a picture and returns None."""
        r = self._r
        s = C.c_void_p(int(stream)) if stream else None
        if out is False:
            r._check(r._lib.ort_accum_render(r._ctx, self._h, int(n), None, s))
            return None
        o, out = r._output("step", self.params, self.tile, out, format, row_pitch, place)
        r._check(r._lib.ort_accum_render(r._ctx, self._h, int(n), C.byref(o), s))
        return out

    @staticmethod
    def _criterion(n, threshold, min_samples, luminance_floor):
        a = L.OrtAccumAdaptive()
        a.n_samples, a.min_samples = int(n), int(min_samples)
        a.threshold, a.luminance_floor = float(threshold), float(luminance_floor)
        return a

    def step_adaptive(self, n: int = 1, threshold: float | None = None, min_samples: int | None = None,
                      luminance_floor: float | None = None, out=None, stream=None, *,
                      format: str = "rgb32f", row_pitch: int | None = None, place: str = "tile"):
        """An adaptive pass (``accumulate(..., adaptive=True)``; ort_accum_render_adaptive in
        include/ort.h): every pixel that holds fewer than min_samples samples, or whose mean
        luminance's standard error is still above threshold x max(luminance, luminance_floor), gets
        its next min(n, total - its count) samples; every other pixel is held, untouched.  The
        picture shows every pixel at its own count.  threshold, min_samples, luminance_floor: None
        takes DEFAULT_ADAPTIVE_*.  out, stream, format, row_pitch, place: as ``step``, which this
        returns like."""
        r = self._r
        a = self._criterion(n, *_adaptive_defaults(threshold, min_samples, luminance_floor))
        s = C.c_void_p(int(stream)) if stream else None
        if out is False:
            r._check(r._lib.ort_accum_render_adaptive(r._ctx, self._h, C.byref(a), None, s))
            return None
        o, out = r._output("step_adaptive", self.params, self.tile, out, format, row_pitch, place)
        r._check(r._lib.ort_accum_render_adaptive(r._ctx, self._h, C.byref(a), C.byref(o), s))
        return out

    def counts(self, out=None, stream=None):
        """The samples each pixel holds, int32 (rows, width), 0 in rows past the frame:
        ort_accum_read_counts.  Returns a numpy array, or, given a torch CUDA tensor (or a device
        pointer) as out, writes and returns that."""
        r = self._r
        rows, width = int(self.tile.rows), int(self.tile.width)
        n = rows * width
        s = C.c_void_p(int(stream)) if stream else None
        if out is None or isinstance(out, np.ndarray):
            if out is None:
                out = np.empty((rows, width), np.int32)
            if out.dtype != np.int32 or not out.flags.c_contiguous or out.size != n:
                raise ValueError(f"counts: out must be a C-contiguous int32 array of {n} elements")
            r._check(r._lib.ort_accum_read_counts(r._ctx, self._h, C.c_void_p(out.ctypes.data), 0, s))
            return out
        ptr = r._device_arg("counts", out, "out", "int32", 4 * n)
        r._check(r._lib.ort_accum_read_counts(r._ctx, self._h, C.c_void_p(ptr), 1, s))
        return out

    def adaptive_stats(self, threshold: float | None = None, min_samples: int | None = None,
                       luminance_floor: float | None = None, n: int = 1) -> dict:
        """The counts in short (ort_accum_adaptive_stats, synchronous): the tile's pixels inside the
        frame, the sum and the extremes of their counts, and pending: the pixels a ``step_adaptive``
        with this criterion would trace now.  The loop of a camera at rest ends at pending == 0.
        It takes no stream and runs on the renderer's own: passes queued with ``stream=`` must have
        finished (synchronize that stream first), or it reads counts that are still being written."""
        r = self._r
        a = self._criterion(n, *_adaptive_defaults(threshold, min_samples, luminance_floor))
        st = L.OrtAccumAdaptiveStats()
        r._check(r._lib.ort_accum_adaptive_stats(r._ctx, self._h, C.byref(a), C.byref(st)))
        return {"pixels": st.pixels, "samples": st.samples, "pending": st.pending, "min_count": st.min_count,
                "max_count": st.max_count}

    def moments(self, mean: bool = True, variance: bool = True, out_mean=None, out_variance=None, stream=None):
        """The linear mean (rows, width, 3) of the samples done so far -- the picture before its gamma
        -- and the variance (rows, width) of that mean's luminance, -1 where there is no estimate
        (fewer than 2 samples, rows past the frame): ort_accum_read_moments (include/ort.h).  The
        variance needs ``accumulate(..., moments=True)``.  Returns numpy arrays, or, given torch CUDA
        tensors (or device pointers) as out_mean / out_variance, writes and returns those; both
        outputs are of one kind.  Returns (mean, variance), or the one asked for."""
        r = self._r
        who = "moments"
        if not mean and not variance:
            raise ValueError(f"{who}: ask for the mean, the variance or both")
        if (out_mean is not None and not mean) or (out_variance is not None and not variance):
            raise ValueError(f"{who}: an out for something that was not asked for")
        rows, width = int(self.tile.rows), int(self.tile.width)
        n = rows * width
        given = [o for o in (out_mean, out_variance) if o is not None]
        device = any(not isinstance(o, np.ndarray) for o in given)
        if device and any(isinstance(o, np.ndarray) for o in given):
            raise ValueError(f"{who}: out_mean and out_variance must both be numpy arrays or both live on the device")
        m = L.OrtAccumMoments()
        m.on_device = 1 if device else 0
        outs = []
        for want, out, what, ch in ((mean, out_mean, "out_mean", 3), (variance, out_variance, "out_variance", 1)):
            if not want:
                continue
            shape = (rows, width, 3) if ch == 3 else (rows, width)
            if device:
                if out is None:
                    import torch
                    out = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", r.device))
                ptr = r._device_arg(who, out, what, "float32", 4 * ch * n)
            else:
                if out is None:
                    out = np.empty(shape, np.float32)
                if out.dtype != np.float32 or not out.flags.c_contiguous or out.size != ch * n:
                    raise ValueError(f"{who}: {what} must be a C-contiguous float32 array of {ch * n} elements")
                ptr = out.ctypes.data
            if ch == 3:
                m.mean = C.c_void_p(ptr)
            else:
                m.variance = C.c_void_p(ptr)
            outs.append(out)
        s = C.c_void_p(int(stream)) if stream else None
        r._check(r._lib.ort_accum_read_moments(r._ctx, self._h, C.byref(m), s))
        return tuple(outs) if len(outs) == 2 else outs[0]

    def restart(self, params: FrameParams):
        """A new camera for the same shape (width, height, num_samples, max_depth, use_octree):
        samples done back to 0, nothing allocated.  Also what makes the accumulation usable again
        after the renderer's scene changed."""
        p = params.to_c()
        self._r._check(self._r._lib.ort_accum_restart(self._r._ctx, self._h, C.byref(p)))
        self.params = params
        self._guides = None

    def guides(self):
        """The pixel-centre guides of the accumulation's params and tile for ``Renderer.denoise``:
        (hits, normals), torch CUDA tensors (rows, width, 2) int32 {t bits, sphere} and (rows, width,
        3) float32 -- ``trace_camera(params, tile, which="pixel_centre", normals=True)`` on the
        device, traced once and kept until ``restart`` (a new camera) drops them."""
        if self._guides is None:
            import torch
            dev = torch.device("cuda", self._r.device)
            rows, width = int(self.tile.rows), int(self.tile.width)
            hits = torch.empty((rows, width, 2), dtype=torch.int32, device=dev)
            nrm = torch.empty((rows, width, 3), dtype=torch.float32, device=dev)
            self._r.trace_camera(self.params, self.tile, which="pixel_centre", normals=nrm, out=hits)
            self._guides = (hits, nrm)
        return self._guides

    def last_pass_ms(self) -> float:
        """The last step's kernels, from HIP events on its stream."""
        ms = C.c_float()
        self._r._check(self._r._lib.ort_accum_last_pass_ms(self._r._ctx, self._h, C.byref(ms)))
        return ms.value


# ``Accumulation.step_adaptive``'s defaults: a relative standard error of 2 % of the mean luminance, taken
# absolute below a luminance of 0.05, never judged before 4 samples.
DEFAULT_ADAPTIVE_THRESHOLD = 0.02
DEFAULT_ADAPTIVE_MIN_SAMPLES = 4
DEFAULT_ADAPTIVE_LUMINANCE_FLOOR = 0.05


# History.update's defaults, chosen on the small frames of tests/test_reproject.py:
# the least weight of a new sample, and the relative depth difference a tap may have.
DEFAULT_HISTORY_ALPHA = 0.1
DEFAULT_DEPTH_TOLERANCE = 0.1


def _history_guides(who, guides, rows, width, renderer):
    """(rays address, hits address, objects to keep alive) of guides = (rays, hits or (t, sphere));
    renderer: None for numpy arrays, else the Renderer whose device the tensors live on."""
    try:
        rays, hits = guides
    except (TypeError, ValueError):
        raise ValueError(f"{who}: guides must be (rays, hits or (t, sphere))") from None
    n = rows * width
    if renderer is None:
        if isinstance(hits, (tuple, list)):
            t, sph = hits
            t, sph = np.ascontiguousarray(t, np.float32), np.ascontiguousarray(sph, np.int32)
            if t.size != n or sph.size != n:
                raise ValueError(f"{who}: t and sphere must hold {n} pixels each")
            rec = np.empty((n, 2), np.int32)
            rec[:, 0] = t.reshape(-1).view(np.int32)
            rec[:, 1] = sph.reshape(-1)
            hits = rec
        if not isinstance(hits, np.ndarray) or hits.dtype != np.int32 or not hits.flags.c_contiguous or hits.size != 2 * n:
            raise ValueError(f"{who}: hits must be a C-contiguous int32 array of {n} {{t bits, sphere}} records")
        if not isinstance(rays, np.ndarray) or rays.dtype != np.float32 or not rays.flags.c_contiguous or rays.size != 6 * n:
            raise ValueError(f"{who}: rays must be a C-contiguous float32 array of 6 x {n} elements")
        return rays.ctypes.data, hits.ctypes.data, (rays, hits)
    if isinstance(hits, (tuple, list)):
        import torch
        t, sph = hits
        if t.numel() != n or sph.numel() != n:
            raise ValueError(f"{who}: t and sphere must hold {n} pixels each")
        hits = torch.stack((t.contiguous().view(torch.int32).reshape(-1), sph.reshape(-1)), dim=1).contiguous()
        torch.cuda.current_stream(renderer.device).synchronize()  # (made on torch's stream, read on the call's)
    if hasattr(hits, "numel") and hits.numel() != 2 * n:
        raise ValueError(f"{who}: hits must hold {n} {{t bits, sphere}} records")
    if hasattr(rays, "numel") and rays.numel() != 6 * n:
        raise ValueError(f"{who}: rays must hold 6 x {n} elements")
    return (renderer._device_arg(who, rays, "rays", "float32", 24 * n),
            renderer._device_arg(who, hits, "hits", "int32", 8 * n), (rays, hits))


def _history_frame(p, t, color, pitch, rays, hits, width, device, alpha, depth_tolerance):
    f = L.OrtHistoryFrame()
    f.params, f.tile = C.pointer(p), C.pointer(t)
    f.color, f.rays, f.hits = C.c_void_p(color), C.c_void_p(rays), C.c_void_p(hits)
    f.color_pitch_bytes = 0 if pitch == 12 * width else int(pitch)
    f.on_device = 1 if device else 0
    f.alpha = float(DEFAULT_HISTORY_ALPHA if alpha is None else alpha)
    f.depth_tolerance = float(DEFAULT_DEPTH_TOLERANCE if depth_tolerance is None else depth_tolerance)
    return f


class History:
    """A preview's history carried across camera moves (``Renderer.history``; ort_history_* in
    include/ort.h): per pixel an integrated linear colour, its history length and two luminance
    moments.  ``update`` finds each pixel's surface point in the previous update's frame, fetches
    that history where it is the same sphere, blends the new sample in and returns the integrated
    colour and a variance for ``Renderer.denoise``.  A context manager: leaving it frees the state
    (as ``close`` does; the renderer's ``close`` frees what is left)."""

    def __init__(self, renderer: Renderer, width: int, rows: int):
        self._r = renderer
        self._h = C.c_void_p()
        self.width, self.rows = int(width), int(rows)
        renderer._check(renderer._lib.ort_history_begin(renderer._ctx, self.width, self.rows, C.byref(self._h)))

    def close(self):
        if self._h and self._r._ctx:
            self._r._check(self._r._lib.ort_history_free(self._r._ctx, self._h))
        self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        i = L.OrtHistoryInfo()
        self._r._check(self._r._lib.ort_history_get_info(self._h, C.byref(i)))
        return {"width": i.width, "rows": i.rows, "updates": i.updates, "device_bytes": i.device_bytes}

    def reset(self):
        """The next update has no previous frame (nothing launched)."""
        self._r._check(self._r._lib.ort_history_reset(self._r._ctx, self._h))

    def last_update_ms(self) -> float:
        """The last update's kernel, from HIP events on its stream."""
        ms = C.c_float()
        self._r._check(self._r._lib.ort_history_last_update_ms(self._r._ctx, self._h, C.byref(ms)))
        return ms.value

    def update(self, image, params: FrameParams, tile: Tile | None = None, guides=None, *, alpha: float | None = None,
               depth_tolerance: float | None = None, variance=True, length=False, out=None, stream=None,
               motion: bool = False):
        """Reproject the history into the frame `params` and blend the frame's sample in
        (ort_history_update, include/ort.h).

        motion=True (ort_history_update_ex with ORT_HISTORY_MOTION): the history survives ``upload`` and
        ``build_scene`` of the same spheres at new places -- the caller vouches that sphere k stays
        sphere k -- and a pixel's surface point is moved back with its sphere before it is projected
        into the previous frame, a resting camera included.  Needs a resident scene.

        image: this frame's LINEAR (rows, width, 3) float32 sample picture (``trace_radiance`` without
        gamma, ``Accumulation.moments``' mean), a numpy array or a torch CUDA tensor on the renderer's
        device (then everything stays there); rows may be a pitch apart.
        params, tile: the frame and the tile of the image; the tile has the history's shape, its
        origin may move between updates.
        guides: (rays, hits) as ``trace_camera(params, tile, which="pixel_centre", rays=True)`` returns
        them -- rays (rows, width, 6) float32, hits an int32 array of {t bits, sphere} records or the
        pair (t, sphere) -- of the image's kind.  None: traced here.
        alpha: the least weight of the new sample (0: the running mean; default DEFAULT_HISTORY_ALPHA);
        depth_tolerance: the relative depth difference a tap may have (0: no test; default
        DEFAULT_DEPTH_TOLERANCE).
        out: None allocates the (rows, width, 3) integrated colour, an array or tensor receives it,
        False leaves it out.  variance, length: True allocates the (rows, width) float32 plane -- the
        variance of the colour's luminance (-1: no estimate), the history length -- an array or tensor
        receives it, False leaves it out.  Returns colour, variance, length, those that were asked
        for (one object when it is the only one, None when none).  stream: as ``render``."""
        who = "History.update"
        r = self._r
        device = not isinstance(image, np.ndarray)
        rows, width, pitch, color = _denoise_image(who, image, r.device if device else None)
        tile = tile or Tile.full(params)
        if guides is None:
            if device:
                import torch
                dev = torch.device("cuda", r.device)
                hits = torch.empty((rows, width, 2), dtype=torch.int32, device=dev)
                rays = torch.empty((rows, width, 6), dtype=torch.float32, device=dev)
                r.trace_camera(params, tile, which="pixel_centre", rays=rays, out=hits, stream=stream)
            else:
                t_, sph, rays = r.trace_camera(params, tile, which="pixel_centre", rays=True, stream=stream)
                hits = (t_, sph)
            guides = (rays, hits)
        rays_p, hits_p, keep = _history_guides(who, guides, rows, width, r if device else None)
        is_flag = lambda x: x is None or isinstance(x, (bool, np.bool_))  # noqa: E731
        n = rows * width

        def plane(x, want_default, last, what):
            """(address or None, the object returned) of an output plane."""
            if is_flag(x):
                if not (want_default if x is None else bool(x)):
                    return None, None
                shape = (rows, width, last) if last > 1 else (rows, width)
                if device:
                    import torch
                    x = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", r.device))
                else:
                    x = np.empty(shape, np.float32)
            if device:
                return r._device_arg(who, x, what, "float32", 4 * last * n), x
            if not isinstance(x, np.ndarray) or x.dtype != np.float32 or not x.flags.c_contiguous or x.nbytes < 4 * last * n:
                raise ValueError(f"{who}: {what} must be a C-contiguous float32 numpy array of >= {4 * last * n} bytes")
            return x.ctypes.data, x

        oc, out = plane(out, True, 3, "out")
        ov, variance = plane(variance, False, 1, "variance")
        ol, length = plane(length, False, 1, "length")
        p, t = params.to_c(), tile.to_c()
        f = _history_frame(p, t, color, pitch, rays_p, hits_p, width, device, alpha, depth_tolerance)
        f.out_color = C.c_void_p(oc) if oc is not None else None
        f.out_variance = C.c_void_p(ov) if ov is not None else None
        f.out_length = C.c_void_p(ol) if ol is not None else None
        s = C.c_void_p(int(stream)) if stream else None
        if motion:
            fx = L.OrtHistoryFrameEx()
            fx.base = f
            fx.base.flags = L.ORT_HISTORY_MOTION
            r._check(r._lib.ort_history_update_ex(r._ctx, self._h, C.byref(fx), s))
        else:
            r._check(r._lib.ort_history_update(r._ctx, self._h, C.byref(f), s))
        del keep
        res = tuple(x for x in (out, variance, length) if x is not None)
        return None if not res else (res[0] if len(res) == 1 else res)


def history_update_host(state, image, params: FrameParams, tile: Tile | None = None, guides=None, *,
                        alpha: float | None = None, depth_tolerance: float | None = None, motion=None):
    """TEST-ONLY: ``History.update`` on the host CPU, stateless (ort_debug_history_update: reproject.inc's
    reproject_pixel, the kernel's own per-pixel function).  motion: None, or (now, snap) for
    ``update(motion=True)`` (ort_debug_history_update_ex) -- the scene's (n, 4) float32
    sphere_center_radius and the one at the previous MOTION update (None: no snapshot).  state: None (no previous frame), or what
    the previous call returned first: (params, (x0, y0), a, b) with the record planes a = {r, g, b, n}
    and b = {m1, m2, t, sphere}, (rows, width, 4) float32 each.  image, guides: numpy arrays as there
    (guides are needed).  Returns (next state, colour (rows, width, 3), variance, length (rows, width))."""
    lib = L.analysis_lib()
    who = "history_update_host"
    if not isinstance(image, np.ndarray):
        raise ValueError(f"{who}: image must be a numpy array")
    rows, width, pitch, color = _denoise_image(who, image, None)
    tile = tile or Tile.full(params)
    rays_p, hits_p, keep = _history_guides(who, guides, rows, width, None)
    p, t = params.to_c(), tile.to_c()
    f = _history_frame(p, t, color, pitch, rays_p, hits_p, width, False, alpha, depth_tolerance)
    col = np.empty((rows, width, 3), np.float32)
    var = np.empty((rows, width), np.float32)
    length = np.empty((rows, width), np.float32)
    f.out_color, f.out_variance, f.out_length = (C.c_void_p(x.ctypes.data) for x in (col, var, length))
    na = np.empty((rows, width, 4), np.float32)
    nb = np.empty((rows, width, 4), np.float32)
    if state is None:
        pp, x0, y0, pa, pb = None, 0, 0, None, None
    else:
        prev_params, (x0, y0), pa, pb = state
        pp = C.byref(prev_params.to_c())
        pa, pb = np.ascontiguousarray(pa, np.float32), np.ascontiguousarray(pb, np.float32)
        if pa.size != 4 * rows * width or pb.size != 4 * rows * width:
            raise ValueError(f"{who}: the state's record planes must hold {rows} x {width} x 4 floats each")
    if motion is None:
        L.acheck(lib.ort_debug_history_update(pp, int(x0), int(y0), L.fptr(pa), L.fptr(pb), C.byref(f), L.fptr(na), L.fptr(nb)))
    else:
        now, snap = motion
        now = np.ascontiguousarray(now, np.float32).reshape(-1, 4)
        if snap is not None:
            snap = np.ascontiguousarray(snap, np.float32).reshape(-1, 4)
            if snap.shape != now.shape:
                raise ValueError(f"{who}: the snapshot must hold the scene's {len(now)} spheres")
        fx = L.OrtHistoryFrameEx()
        fx.base = f
        fx.base.flags = L.ORT_HISTORY_MOTION
        L.acheck(lib.ort_debug_history_update_ex(pp, int(x0), int(y0), L.fptr(pa), L.fptr(pb), C.byref(fx), L.fptr(now),
                                                 L.fptr(snap), len(now), L.fptr(na), L.fptr(nb)))
    del keep
    return (params, (int(tile.x0), int(tile.y0)), na, nb), col, var, length


def _adaptive_defaults(threshold, min_samples, luminance_floor):
    return (DEFAULT_ADAPTIVE_THRESHOLD if threshold is None else threshold,
            DEFAULT_ADAPTIVE_MIN_SAMPLES if min_samples is None else min_samples,
            DEFAULT_ADAPTIVE_LUMINANCE_FLOOR if luminance_floor is None else luminance_floor)


# Reference-layout record bytes touched, SURVEY.md 8(d): the algorithmic traffic model.
BYTES_PER = {"nodes_popped": 36, "child_records": 32, "leaf_objects": 20, "accepted_hits": 32, "pixels": 12}


def algorithmic_bytes(counts: dict) -> int:
    return sum(BYTES_PER[k] * int(counts[k]) for k in BYTES_PER)


def emulate_render_host(spheres: SphereSet, tree: FlatOctree | None, params: FrameParams, tile: Tile | None = None,
                        layout: int = L.ORT_LAYOUT_COMPACT, samples_done: int | None = None):
    """TEST-ONLY: run the kernel's per-pixel code (render_core.h) on the host CPU.
    Used by the CPU test suite to validate the kernel's traversal logic against the
    independent oracle without a GPU.  ``Renderer.render`` never calls this.
    samples_done = k: the picture an ``Accumulation`` of params shows after k samples -- the
    first k samples of each pixel's num_samples-sample chain, divided by k."""
    lib = L.analysis_lib()
    tile = tile or Tile.full(params)
    out = np.empty((tile.rows, tile.width, 3), np.float32)
    counts = (C.c_uint64 * L.ORT_COUNT_N)()
    p, t = params.to_c(), tile.to_c()
    cr = np.ascontiguousarray(spheres.center_radius, np.float32)
    ma = np.ascontiguousarray(spheres.mat_albedo, np.float32)
    fr = np.ascontiguousarray(spheres.fuzz_ri, np.float32)
    if tree is None:
        keep = ()
        args = (None, None, None, None, None, 0, None, 0)
    else:
        keep = tuple(np.ascontiguousarray(a, t) for a, t in (
            (tree.node_min, np.float32), (tree.node_max, np.float32), (tree.children_offset, np.int32),
            (tree.objects_offset, np.int32), (tree.object_count, np.int32), (tree.object_indices, np.int32)))
        args = (L.fptr(keep[0]), L.fptr(keep[1]), L.iptr(keep[2]), L.iptr(keep[3]), L.iptr(keep[4]),
                tree.n_nodes, L.iptr(keep[5]), tree.n_indices)
    if samples_done is None:
        L.acheck(lib.ort_debug_emulate_render(L.fptr(cr), L.fptr(ma), L.fptr(fr), spheres.n, *args, layout,
                                             C.byref(p), C.byref(t), L.fptr(out), counts))
    else:
        L.acheck(lib.ort_debug_emulate_render_prefix(L.fptr(cr), L.fptr(ma), L.fptr(fr), spheres.n, *args, layout,
                                                    C.byref(p), C.byref(t), int(samples_done), L.fptr(out), counts))
    del keep
    return out, dict(zip(L.COUNT_NAMES, [int(v) for v in counts]))


def query_rays_host(spheres: SphereSet, tree: FlatOctree | None, rays, *, layout: int = L.ORT_LAYOUT_COMPACT,
                    use_octree: bool = True, normals: bool = False, mode: str | None = None, t_range=None):
    """TEST-ONLY: ``Renderer.trace_rays`` on the host CPU (ort_debug_query_rays: render_core.h
    query_ray, the kernels' own per-ray function).  Returns (t, sphere[, normals]).  With mode
    ("drawn", "nearest", "any") ort_debug_query_rays_ex: query_ray_mode over t_range, None or (n, 2)."""
    lib = L.analysis_lib()
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    if mode is not None and mode not in L.QUERY_MODES:
        raise ValueError(f"query_rays_host: mode must be one of {sorted(L.QUERY_MODES)} (got {mode!r})")
    if t_range is not None:
        if mode is None or mode == "drawn":
            raise ValueError('query_rays_host: t_range needs mode="nearest" or "any"')
        t_range = np.ascontiguousarray(t_range, np.float32)
        if t_range.shape != (n, 2):
            raise ValueError(f"query_rays_host: t_range must have shape ({n}, 2) (got {t_range.shape})")
    cr = np.ascontiguousarray(spheres.center_radius, np.float32)
    if tree is None:
        keep = ()
        args = (None, None, None, None, None, 0, None, 0)
    else:
        keep = tuple(np.ascontiguousarray(a, t) for a, t in (
            (tree.node_min, np.float32), (tree.node_max, np.float32), (tree.children_offset, np.int32),
            (tree.objects_offset, np.int32), (tree.object_count, np.int32), (tree.object_indices, np.int32)))
        args = (L.fptr(keep[0]), L.fptr(keep[1]), L.iptr(keep[2]), L.iptr(keep[3]), L.iptr(keep[4]),
                tree.n_nodes, L.iptr(keep[5]), tree.n_indices)
    rec = np.empty((n, 2), np.int32)
    nrm = np.zeros((n, 3), np.float32) if normals else None
    if mode is None:
        L.acheck(lib.ort_debug_query_rays(L.fptr(cr), spheres.n, *args, int(layout), 1 if use_octree else 0, L.fptr(rays), n,
                                         rec.ctypes.data_as(C.c_void_p), L.fptr(nrm)))
    else:
        L.acheck(lib.ort_debug_query_rays_ex(L.fptr(cr), spheres.n, *args, int(layout), 1 if use_octree else 0, L.fptr(rays),
                                            n, L.QUERY_MODES[mode], L.fptr(t_range), rec.ctypes.data_as(C.c_void_p),
                                            L.fptr(nrm)))
    del keep
    t, sph = np.ascontiguousarray(rec[:, 0]).view(np.float32), np.ascontiguousarray(rec[:, 1])
    return (t, sph, nrm) if normals else (t, sph)


def camera_query_host(spheres: SphereSet | None, tree: FlatOctree | None, params: FrameParams, tile: Tile | None = None,
                      *, which: str = "first_sample", layout: int = L.ORT_LAYOUT_COMPACT, hits: bool = True,
                      normals: bool = False):
    """TEST-ONLY: ``Renderer.trace_camera`` on the host CPU (ort_debug_camera_query: the kernels' own
    per-pixel ray, then render_core.h query_ray by params.use_octree).  Returns (rays (rows, width,
    6), t, sphere (rows, width)[, normals (rows, width, 3)]); with hits=False the rays alone, and
    spheres may be None."""
    lib = L.analysis_lib()
    tile = tile or Tile.full(params)
    rows, width = int(tile.rows), int(tile.width)
    p, t = params.to_c(), tile.to_c()
    rays = np.zeros((rows, width, 6), np.float32)
    rec = np.zeros((rows * width, 2), np.int32) if hits else None
    nrm = np.zeros((rows, width, 3), np.float32) if normals else None
    cr = np.ascontiguousarray(spheres.center_radius, np.float32) if spheres is not None else None
    if tree is None or not hits:
        keep = ()
        args = (None, None, None, None, None, 0, None, 0)
    else:
        keep = tuple(np.ascontiguousarray(a, t_) for a, t_ in (
            (tree.node_min, np.float32), (tree.node_max, np.float32), (tree.children_offset, np.int32),
            (tree.objects_offset, np.int32), (tree.object_count, np.int32), (tree.object_indices, np.int32)))
        args = (L.fptr(keep[0]), L.fptr(keep[1]), L.iptr(keep[2]), L.iptr(keep[3]), L.iptr(keep[4]),
                tree.n_nodes, L.iptr(keep[5]), tree.n_indices)
    L.acheck(lib.ort_debug_camera_query(L.fptr(cr), spheres.n if spheres is not None else 0, *args, int(layout),
                                       C.byref(p), C.byref(t), L.CAMERA_RAYS[which], L.fptr(rays),
                                       rec.ctypes.data_as(C.c_void_p) if hits else None, L.fptr(nrm)))
    del keep
    if not hits:
        return rays
    tt = np.ascontiguousarray(rec[:, 0]).view(np.float32).reshape(rows, width)
    sph = np.ascontiguousarray(rec[:, 1]).reshape(rows, width)
    return (rays, tt, sph, nrm) if normals else (rays, tt, sph)


def rng_states(n: int, seed: int = 0) -> np.ndarray:
    """(n, 2) float32 RNG states for ``Renderer.trace_radiance``, each component in [0, 1), from
    np.random.default_rng(seed): one independent chain per ray."""
    return np.random.default_rng(seed).random((int(n), 2), dtype=np.float32)


def radiance_rays_host(spheres: SphereSet, tree: FlatOctree | None, rays, states, *, max_depth: int, paths: int = 1,
                       layout: int = L.ORT_LAYOUT_COMPACT, use_octree: bool = True, sort: bool = False,
                       normalize: bool = False, gamma: bool = False, states_out=False):
    """TEST-ONLY: ``Renderer.trace_radiance`` on the host CPU (ort_debug_radiance_rays: the kernels'
    own per-bounce functions, one ray's chain after another).  Returns the (n, 3) radiance, and with
    states_out (True, or an (n, 2) float32 array to receive them, `states` itself allowed) the end states."""
    lib = L.analysis_lib()
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    states = np.ascontiguousarray(states, np.float32)
    if states.shape != (n, 2):
        raise ValueError(f"radiance_rays_host: states must have shape ({n}, 2) (got {states.shape})")
    if isinstance(states_out, (bool, np.bool_)):
        st_out = np.empty((n, 2), np.float32) if states_out else None
    else:
        st_out = states_out
        if (not isinstance(st_out, np.ndarray) or st_out.dtype != np.float32 or st_out.shape != (n, 2) or
                not st_out.flags.c_contiguous):
            raise ValueError(f"radiance_rays_host: states_out must be a C-contiguous ({n}, 2) float32 array")
    flags = ((L.ORT_QUERY_SORT if sort else 0) | (L.ORT_RADIANCE_NORMALIZE if normalize else 0) |
             (L.ORT_RADIANCE_GAMMA if gamma else 0))
    cr = np.ascontiguousarray(spheres.center_radius, np.float32)
    ma = np.ascontiguousarray(spheres.mat_albedo, np.float32)
    fr = np.ascontiguousarray(spheres.fuzz_ri, np.float32)
    if tree is None:
        keep = ()
        args = (None, None, None, None, None, 0, None, 0)
    else:
        keep = tuple(np.ascontiguousarray(a, t) for a, t in (
            (tree.node_min, np.float32), (tree.node_max, np.float32), (tree.children_offset, np.int32),
            (tree.objects_offset, np.int32), (tree.object_count, np.int32), (tree.object_indices, np.int32)))
        args = (L.fptr(keep[0]), L.fptr(keep[1]), L.iptr(keep[2]), L.iptr(keep[3]), L.iptr(keep[4]),
                tree.n_nodes, L.iptr(keep[5]), tree.n_indices)
    rad = np.empty((n, 3), np.float32)
    L.acheck(lib.ort_debug_radiance_rays(L.fptr(cr), L.fptr(ma), L.fptr(fr), spheres.n, *args, int(layout),
                                        1 if use_octree else 0, L.fptr(rays), L.fptr(states), n, int(max_depth), int(paths),
                                        flags, L.fptr(rad), L.fptr(st_out)))
    del keep
    return (rad, st_out) if st_out is not None else rad


def _denoise_image(who, image, device):
    """rows, width, the rows' pitch in bytes and the address of a (rows, width, 3) float32 image: a
    numpy array, or (device: the GPU's index) a torch CUDA tensor; rows may be a pitch apart."""
    if device is None:
        if image.dtype != np.float32 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"{who}: image must be a (rows, width, 3) float32 array (got {image.dtype}, shape {image.shape})")
        rows, width = image.shape[:2]
        strides, ptr = image.strides, image.ctypes.data
    else:
        if not hasattr(image, "data_ptr"):
            raise ValueError(f"{who}: image must be a numpy array or a torch CUDA tensor")
        if str(image.dtype) != "torch.float32" or image.dim() != 3 or image.shape[2] != 3:
            raise ValueError(f"{who}: image must be a (rows, width, 3) float32 tensor (got {image.dtype}, shape {tuple(image.shape)})")
        if image.device.type != "cuda" or image.device.index != device:
            raise ValueError(f"{who}: image is on {image.device}, the context filters on cuda:{device}")
        rows, width = int(image.shape[0]), int(image.shape[1])
        strides, ptr = tuple(4 * int(v) for v in image.stride()), image.data_ptr()
    if rows * width == 0:
        return rows, width, 0, ptr
    if (width > 1 and strides[1] != 12) or strides[2] != 4 or (rows > 1 and (strides[0] < 12 * width or strides[0] % 4)):
        raise ValueError(f"{who}: image pixels must be 12 bytes apart and rows at least 12 * width (strides {strides})")
    return rows, width, (strides[0] if rows > 1 else 12 * width), ptr


def _denoise_tile_rows(who, params, tile, rows, width):
    """The rows of the image that lie inside the frame; refuses a banded tile and a tile of another shape."""
    if tile.band_height > 0 and tile.rows > tile.band_height:
        raise ValueError(f"{who}: a banded tile's rows are not neighbours in the frame: denoise the assembled frame")
    if (int(tile.rows), int(tile.width)) != (rows, width):
        raise ValueError(f"{who}: image is {rows} x {width} but the tile is {tile.rows} x {tile.width}")
    return max(0, min(rows, int(params.height) - int(tile.y0)))


def _denoise_guides(who, guides, rows, width, renderer):
    """(hits address, normals address, objects to keep alive) of guides = (hits or (t, sphere), normals);
    renderer: None for numpy arrays, else the Renderer whose device the tensors live on."""
    try:
        hits, nrm = guides
    except (TypeError, ValueError):
        raise ValueError(f"{who}: guides must be (hits or (t, sphere), normals)") from None
    n = rows * width
    if renderer is None:
        if isinstance(hits, (tuple, list)):
            t, sph = hits
            t, sph = np.ascontiguousarray(t, np.float32), np.ascontiguousarray(sph, np.int32)
            if t.size != n or sph.size != n:
                raise ValueError(f"{who}: t and sphere must hold {n} pixels each")
            rec = np.empty((n, 2), np.int32)
            rec[:, 0] = t.reshape(-1).view(np.int32)
            rec[:, 1] = sph.reshape(-1)
            hits = rec
        if not isinstance(hits, np.ndarray) or hits.dtype != np.int32 or not hits.flags.c_contiguous or hits.size != 2 * n:
            raise ValueError(f"{who}: hits must be a C-contiguous int32 array of {n} {{t bits, sphere}} records")
        if (not isinstance(nrm, np.ndarray) or nrm.dtype != np.float32 or not nrm.flags.c_contiguous or nrm.size != 3 * n):
            raise ValueError(f"{who}: normals must be a C-contiguous float32 array of 3 x {n} elements")
        return hits.ctypes.data, nrm.ctypes.data, (hits, nrm)
    if isinstance(hits, (tuple, list)):
        import torch
        t, sph = hits
        if t.numel() != n or sph.numel() != n:
            raise ValueError(f"{who}: t and sphere must hold {n} pixels each")
        hits = torch.stack((t.contiguous().view(torch.int32).reshape(-1), sph.reshape(-1)), dim=1).contiguous()
        torch.cuda.current_stream(renderer.device).synchronize()  # (made on torch's stream, read on the call's)
    if hasattr(hits, "numel") and hits.numel() != 2 * n:
        raise ValueError(f"{who}: hits must hold {n} {{t bits, sphere}} records")
    if hasattr(nrm, "numel") and nrm.numel() != 3 * n:
        raise ValueError(f"{who}: normals must hold 3 x {n} elements")
    return (renderer._device_arg(who, hits, "hits", "int32", 8 * n),
            renderer._device_arg(who, nrm, "normals", "float32", 12 * n), (hits, nrm))


def _denoise_zero_rows(who, out, first, rows, pitch, row_bytes, device):
    """Rows first .. rows-1 of out as ``render`` writes the rows past the frame: zero bytes."""
    if isinstance(out, np.ndarray):
        b = out.reshape(-1).view(np.uint8)
        for r in range(first, rows):
            b[r * pitch:r * pitch + row_bytes] = 0
        return
    if not hasattr(out, "numel"):
        raise ValueError(f"{who}: a tile reaching past the frame needs out as a tensor (its padding rows are zeroed)")
    import torch
    b = out.view(torch.uint8).reshape(-1)
    for r in range(first, rows):
        b[r * pitch:r * pitch + row_bytes] = 0
    torch.cuda.current_stream(device).synchronize()


def _denoise_desc(color, pitch, hits, normals, width, rows, device, iterations, sigma_color, sigma_depth, normal_power,
                  same_sphere):
    d = L.OrtDenoiseDesc()
    d.color, d.hits, d.normals = C.c_void_p(color), C.c_void_p(hits), C.c_void_p(normals)
    d.color_pitch_bytes = 0 if pitch == 12 * width else int(pitch)
    d.width, d.rows, d.on_device = int(width), int(rows), 1 if device else 0
    d.iterations, d.normal_power = int(iterations), int(normal_power)
    d.sigma_color, d.sigma_depth = float(sigma_color), float(sigma_depth)
    d.flags = L.ORT_DENOISE_SAME_SPHERE if same_sphere else 0
    return d


# Renderer.denoise's sigma_variance when a variance is given: taps further than this many standard
# deviations of the pixel's luminance add nothing (chosen from a sweep over 1, 2, 4 and 8: DESIGN.md 4.15).
DEFAULT_SIGMA_VARIANCE = 4.0


def _denoise_desc_ex(who, d, variance, sigma_variance, gamma, rows, width, real, renderer):
    """The ort_denoise_desc_ex over the description d, and what to keep alive during the call."""
    x = L.OrtDenoiseDescEx()
    x.base = d
    if gamma:
        x.base.flags |= L.ORT_DENOISE_GAMMA
    keep = None
    if variance is None:
        if sigma_variance is not None:
            raise ValueError(f"{who}: sigma_variance needs a variance")
        return x, keep
    n = rows * width
    if renderer is None:
        if (not isinstance(variance, np.ndarray) or variance.dtype != np.float32 or not variance.flags.c_contiguous or
                variance.size != n):
            raise ValueError(f"{who}: variance must be a C-contiguous float32 array of {n} elements")
        x.variance = C.c_void_p(variance.ctypes.data)
    else:
        if hasattr(variance, "numel") and variance.numel() != n:
            raise ValueError(f"{who}: variance must hold {n} elements")
        x.variance = C.c_void_p(renderer._device_arg(who, variance, "variance", "float32", 4 * n))
    x.sigma_variance = float(DEFAULT_SIGMA_VARIANCE if sigma_variance is None else sigma_variance)
    return x, variance


def denoise_host(image, guides, *, iterations: int = 3, sigma_color: float = 0.0, sigma_depth: float = 0.0,
                 normal_power: int = 5, same_sphere: bool = True, format: str = "rgb32f", row_pitch: int | None = None,
                 out=None, variance=None, sigma_variance: float | None = None, gamma: bool = False):
    """TEST-ONLY: ``Renderer.denoise`` on the host CPU (ort_debug_denoise: denoise.inc's denoise_pixel,
    the kernels' own per-pixel function).  image, guides, format, row_pitch, out: as there, numpy
    arrays; out may be the image itself.  Returns out."""
    lib = L.analysis_lib()
    who = "denoise_host"
    if not isinstance(image, np.ndarray):
        raise ValueError(f"{who}: image must be a numpy array")
    rows, width, pitch, color = _denoise_image(who, image, None)
    hits, nrm, keep = _denoise_guides(who, guides, rows, width, None)
    o, out = Renderer._output(None, who, None, Tile(0, width, 0, rows), out, format, row_pitch, "tile")
    d = _denoise_desc(color, pitch, hits, nrm, width, rows, False, iterations, sigma_color, sigma_depth, normal_power,
                      same_sphere)
    if variance is None and sigma_variance is None and not gamma:
        L.acheck(lib.ort_debug_denoise(C.byref(d), C.byref(o)))
    else:  # ort_debug_denoise_ex: the emulation of ort_denoise_ex
        x, keep_v = _denoise_desc_ex(who, d, variance, sigma_variance, gamma, rows, width, rows, None)
        L.acheck(lib.ort_debug_denoise_ex(C.byref(x), C.byref(o)))
        del keep_v
    del keep
    return out


def accum_moments_host(spheres: SphereSet, tree: FlatOctree | None, params: FrameParams, tile: Tile | None = None,
                       layout: int = L.ORT_LAYOUT_COMPACT, samples_done: int | None = None):
    """TEST-ONLY: ``Accumulation.moments`` after samples_done (default: all) samples on the host CPU
    (ort_debug_emulate_moments: the kernel's per-pixel code with its colour sum and second moment).
    Returns (mean (rows, width, 3), variance (rows, width))."""
    lib = L.analysis_lib()
    tile = tile or Tile.full(params)
    mean = np.empty((tile.rows, tile.width, 3), np.float32)
    var = np.empty((tile.rows, tile.width), np.float32)
    p, t = params.to_c(), tile.to_c()
    cr = np.ascontiguousarray(spheres.center_radius, np.float32)
    ma = np.ascontiguousarray(spheres.mat_albedo, np.float32)
    fr = np.ascontiguousarray(spheres.fuzz_ri, np.float32)
    if tree is None:
        keep = ()
        args = (None, None, None, None, None, 0, None, 0)
    else:
        keep = tuple(np.ascontiguousarray(a, t_) for a, t_ in (
            (tree.node_min, np.float32), (tree.node_max, np.float32), (tree.children_offset, np.int32),
            (tree.objects_offset, np.int32), (tree.object_count, np.int32), (tree.object_indices, np.int32)))
        args = (L.fptr(keep[0]), L.fptr(keep[1]), L.iptr(keep[2]), L.iptr(keep[3]), L.iptr(keep[4]),
                tree.n_nodes, L.iptr(keep[5]), tree.n_indices)
    k = params.num_samples if samples_done is None else int(samples_done)
    L.acheck(lib.ort_debug_emulate_moments(L.fptr(cr), L.fptr(ma), L.fptr(fr), spheres.n, *args, layout, C.byref(p),
                                          C.byref(t), k, L.fptr(mean), L.fptr(var)))
    del keep
    return mean, var


def accum_adaptive_host(spheres: SphereSet, tree: FlatOctree | None, params: FrameParams, tile: Tile | None = None,
                        layout: int = L.ORT_LAYOUT_COMPACT, passes=()):
    """TEST-ONLY: an adaptive accumulation driven by `passes` on the host CPU (ort_debug_emulate_adaptive:
    the kernel's per-pixel code and the shared decision).  passes: (n_samples, min_samples, threshold,
    luminance_floor) tuples.  Returns (counts (rows, width) int32, mean (rows, width, 3), variance
    (rows, width)) as ``Accumulation.counts`` and ``Accumulation.moments`` return them afterwards."""
    lib = L.analysis_lib()
    tile = tile or Tile.full(params)
    counts = np.empty((tile.rows, tile.width), np.int32)
    mean = np.empty((tile.rows, tile.width, 3), np.float32)
    var = np.empty((tile.rows, tile.width), np.float32)
    p, t = params.to_c(), tile.to_c()
    cr = np.ascontiguousarray(spheres.center_radius, np.float32)
    ma = np.ascontiguousarray(spheres.mat_albedo, np.float32)
    fr = np.ascontiguousarray(spheres.fuzz_ri, np.float32)
    if tree is None:
        keep = ()
        args = (None, None, None, None, None, 0, None, 0)
    else:
        keep = tuple(np.ascontiguousarray(a, t_) for a, t_ in (
            (tree.node_min, np.float32), (tree.node_max, np.float32), (tree.children_offset, np.int32),
            (tree.objects_offset, np.int32), (tree.object_count, np.int32), (tree.object_indices, np.int32)))
        args = (L.fptr(keep[0]), L.fptr(keep[1]), L.iptr(keep[2]), L.iptr(keep[3]), L.iptr(keep[4]),
                tree.n_nodes, L.iptr(keep[5]), tree.n_indices)
    passes = list(passes)
    arr = (L.OrtAccumAdaptive * max(len(passes), 1))()
    for a, (n, min_samples, threshold, floor) in zip(arr, passes):
        a.n_samples, a.min_samples, a.threshold, a.luminance_floor = int(n), int(min_samples), float(threshold), float(floor)
    L.acheck(lib.ort_debug_emulate_adaptive(L.fptr(cr), L.fptr(ma), L.fptr(fr), spheres.n, *args, layout, C.byref(p),
                                           C.byref(t), arr, len(passes), L.iptr(counts), L.fptr(mean), L.fptr(var)))
    del keep
    return counts, mean, var


def adaptive_decision_host(k: int, n_total: int, criterion, col, m2: float) -> int:
    """TEST-ONLY: the shared decision for one stored pixel state (ort_debug_adaptive_decision): 1
    traced, 0 held, -1 a refused criterion.  criterion: (n_samples, min_samples, threshold, floor)."""
    lib = L.analysis_lib()
    a = L.OrtAccumAdaptive()
    a.n_samples, a.min_samples, a.threshold, a.luminance_floor = (int(criterion[0]), int(criterion[1]), float(criterion[2]),
                                                                  float(criterion[3]))
    c = np.ascontiguousarray(col, np.float32)
    return int(lib.ort_debug_adaptive_decision(int(k), int(n_total), C.byref(a), L.fptr(c), C.c_float(m2)))


def gamma_host(rgb):
    """TEST-ONLY: pow(x, 1/2.2) per channel as the kernels compute it (ort_debug_gamma: finish_pixel)."""
    lib = L.analysis_lib()
    a = np.ascontiguousarray(rgb, np.float32)
    out = np.empty_like(a)
    L.acheck(lib.ort_debug_gamma(L.fptr(a), a.size // 3, L.fptr(out)))
    return out
