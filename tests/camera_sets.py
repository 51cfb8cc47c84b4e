"""What the camera-query tests share (tests/test_camera_query.py, tests/test_gpu_camera_query.py):
the camera of every scene of tests/ray_sets.py, the frames, the float32 restatement of the
shader's camera rays, and the host emulation's records (computed once per process, read-only)."""
import functools

import numpy as np

import ray_sets
from test_ray_query import CONFIGS

SCENES = ("compact5", "compact10", "explicit", "brute")
FRAMES = ((37, 21), (64, 8))          # odd width, both aspect orders (pixelRadius takes max(W, H))
SAMPLES = (1, 4, 5)                   # sqrt_ns 1, 2, and 2 with a remainder
WHICH = ("first_sample", "pixel_centre")

# One camera per scene: the default pose, or one moved in and zoomed, so that the oracle's share of hit
# pixels of the 37 x 21 first-sample frame lies in 0.2 .. 0.8 (test_camera_query.py asserts it).
CAMERAS = {
    "compact5": dict(position=(0.0, 2.5, -10.0)),
    "compact10": dict(position=(0.0, 2.5, -10.0)),
    "explicit": dict(position=(0.0, 1.0, -3.0), zoom=30.0),
    "brute": dict(position=(0.0, 1.0, -3.0), zoom=30.0),
}

F = np.float32


def params(name, w=37, h=21, ns=1):
    import octreeraytracer_amd as ort
    return ort.FrameParams.default_camera(w, h, num_samples=ns, max_depth=1, use_octree=1 if CONFIGS[name][1] else 0,
                                          **CAMERAS[name])


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _norm(v):
    """render_core.h / oracle normalize: s = 1 / sqrt((x x + y y) + z z), v * s."""
    d = F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2]))
    s = F(F(1.0) / np.sqrt(d, dtype=F))
    return np.array([F(v[0] * s), F(v[1] * s), F(v[2] * s)], F)


def numpy_rays(oracle, p, which, tile=None):
    """The camera ray of every tile pixel (rows, width, 6), restated from the shader in float32
    numpy, one rounded operation at a time (glsl:640, 647-654, 205-221, 602), on the oracle's
    camera, RNG sequence, sin and cos.  Rows past the frame are zero."""
    import octreeraytracer_amd as ort
    tile = tile or ort.Tile.full(p)
    cam = oracle.camera(p)
    org, ll, hor, ver, cu, cv = (cam[3 * k:3 * k + 3].astype(F) for k in range(6))
    lens = F(cam[21])
    lib = oracle.lib()
    W, H = F(p.width), F(p.height)
    sqrt_ns = int(np.sqrt(F(p.num_samples), dtype=F))
    out = np.zeros((tile.rows, tile.width, 6), F)
    for j, y in enumerate(tile.pixel_rows(p.height)):
        if y >= p.height:
            continue
        for c in range(tile.width):
            x = tile.x0 + c
            fx, fy = F(F(x) + F(0.5)), F(F(y) + F(0.5))
            if which == "pixel_centre":
                a, b = F(fx / W), F(fy / H)
                off = np.zeros(3, F)
                o = org.copy()
            else:
                r = oracle.rand_sequence(float(F(fx / W)), float(F(fy / H)), 6)
                # stratum (0, 0): i = j = 0
                u = F(F(fx + F(F(F(0.0) + r[0]) / F(sqrt_ns))) / W)
                v = F(F(fy + F(F(F(0.0) + r[1]) / F(sqrt_ns))) / H)
                pr = F(F(0.5) / max(W, H))
                jx, jy = F(pr * F(r[2] - F(0.5))), F(pr * F(r[3] - F(0.5)))
                spx, spy = F(F(F(2.0) * r[4]) - F(1.0)), F(F(F(2.0) * r[5]) - F(1.0))
                if spx > -spy:
                    if spx > spy:
                        rr, phi = spx, F(spy / spx)
                    else:
                        rr, phi = spy, F(F(2.0) - F(spx / spy))
                else:
                    if spx < spy:
                        rr, phi = F(-spx), F(F(4.0) + F(spy / spx))
                    else:
                        rr = F(-spy)
                        phi = F(F(6.0) - F(spx / spy)) if spy != 0.0 else F(0.0)
                phi = F(phi * F(F(3.14159265359) / F(4.0)))
                dx, dy = F(rr * F(lib.oracle_cos(float(phi)))), F(rr * F(lib.oracle_sin(float(phi))))
                rdx, rdy = F(lens * dx), F(lens * dy)
                off = np.array([F(F(cu[k] * rdx) + F(cv[k] * rdy)) for k in range(3)], F)
                o = np.array([F(org[k] + off[k]) for k in range(3)], F)
                a, b = F(u + jx), F(v + jy)
            d = [F(F(F(ll[k] + F(a * hor[k])) + F(b * ver[k])) - org[k]) for k in range(3)]
            if which != "pixel_centre":
                d = [F(d[k] - off[k]) for k in range(3)]
            out[j, c, :3] = o
            out[j, c, 3:] = _norm(_norm(d))  # Camera_getRay's normalize, then radiance()'s
    return out


@functools.lru_cache(maxsize=None)
def emulated(name, w=37, h=21, ns=1, which="first_sample"):
    """(rays, t, sphere, normals) of the whole frame by the host emulation (read-only)."""
    from octreeraytracer_amd.renderer import camera_query_host
    s, t, _ = ray_sets.scene(name)
    layout, use_octree = CONFIGS[name]
    res = camera_query_host(s, t if use_octree else None, params(name, w, h, ns), which=which, layout=layout, normals=True)
    for a in res:
        a.setflags(write=False)
    return res
