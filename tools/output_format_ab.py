"""RGB32F against RGBA8 output (Renderer.render format=): in one process on one GPU, alternating
frames of the two formats of C3 (3840x2160, 100k spheres, depth 8, 1 x 1) and of config.h's
default (800x600, 100 spheres, depth 3, 16 x 8).  Per format: the device time of a frame
(ort_last_kernel_ms; device output), median and spread, and the wall time of a synchronous
render into pinned host memory (the frame, its copy to the host and the wait).  The RGBA8
frame is compared with to_srgb8 of the float frame.

usage: python tools/output_format_ab.py [--frames 50] [--md out.md] [c3] [config_default]     (GPU)
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import octreeraytracer_amd as ort  # noqa: E402
from octreeraytracer_amd.image import to_srgb8  # noqa: E402

# name: spheres, depth, maxSpheresPerNode, W, H, spp, bounces
CASES = {
    "c3": (100000, 8, 0, 3840, 2160, 1, 1),
    "config_default": (100, 3, 0, 800, 600, 16, 8),  # src/config.h:10-28
}
FORMATS = {"rgb32f": (3, torch.float32), "rgba8": (4, torch.uint8)}


def stats(v):
    v = sorted(v)
    return statistics.median(v), v[0], v[len(v) // 10], v[-1 - len(v) // 10], v[-1]


def run(name, frames):
    n, d, m, W, H, spp, md = CASES[name]
    s = ort.random_spheres(n, 42)
    p = ort.FrameParams.default_camera(W, H, num_samples=spp, max_depth=md)
    dev = {f: torch.empty((H, W, c), dtype=t, device="cuda") for f, (c, t) in FORMATS.items()}
    pin = {f: torch.empty((H, W, c), dtype=t).pin_memory() for f, (c, t) in FORMATS.items()}
    kernel = {f: [] for f in FORMATS}
    readback = {f: [] for f in FORMATS}
    with ort.Renderer(0) as r:
        r.build_scene(s, d, m)
        for f in FORMATS:  # warm up each format (and its host path)
            for _ in range(5):
                r.render(p, out=dev[f], format=f)
                r.render(p, out=pin[f].numpy(), format=f)
        for _ in range(frames):  # alternating: drift hits both alike
            for f in FORMATS:
                r.render(p, out=dev[f], format=f)
                kernel[f].append(r.last_kernel_ms())
        for _ in range(frames):
            for f in FORMATS:
                out = pin[f].numpy()
                t0 = time.perf_counter()
                r.render(p, out=out, format=f)
                readback[f].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    f32, rgba = dev["rgb32f"].cpu().numpy(), dev["rgba8"].cpu().numpy()
    same = bool(np.array_equal(rgba[..., :3], to_srgb8(f32)) and (rgba[..., 3] == 255).all()
                and np.array_equal(pin["rgba8"].numpy(), rgba)
                and np.array_equal(pin["rgb32f"].numpy().view(np.uint32), f32.view(np.uint32)))
    rows = []
    for f, (c, t) in FORMATS.items():
        bpp = 12 if f == "rgb32f" else 4
        k, h = stats(kernel[f]), stats(readback[f])
        rows.append(f"| {name} | {f} | {W * H * bpp / 1e6:.1f} | {k[0]:.3f} | {k[1]:.3f} | {k[2]:.3f}-{k[3]:.3f} | "
                    f"{k[4]:.3f} | {h[0]:.3f} | {h[1]:.3f} | {h[2]:.3f}-{h[3]:.3f} | {h[4]:.3f} |")
    rows.append(f"| {name} | rgba8 == to_srgb8(rgb32f), host == device | {same} | | | | | | | | |")
    return rows, same


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--md", default=None, help="also write the table to this file")
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    head = [f"{a.frames} frames per format, alternating, one process, {torch.cuda.get_device_name(0)}; ms",
            "",
            "| case | format | frame MB | device median | min | p10-p90 | max | to pinned host median | min | p10-p90 | max |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    lines, ok = list(head), True
    for nm in a.names or list(CASES):
        rows, same = run(nm, a.frames)
        lines += rows
        ok = ok and same
    text = "\n".join(lines)
    print(text, flush=True)
    if a.md:
        Path(a.md).parent.mkdir(parents=True, exist_ok=True)
        Path(a.md).write_text(text + "\n")
    sys.exit(0 if ok else 1)
