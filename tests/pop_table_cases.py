"""Scenes, poses and oracle frames shared by tests/test_pop_table.py (host walk) and
tests/test_gpu_pop_table.py (kernels): small trees of depth 1, 2, 3, 5 and 8, seen from inside
the sphere field along the eight (+-1, +-1, +-1) diagonals, so that the depth <= 8 camera walk
pops every mask bit hb = 8 L + 7 - rank its pop table holds, under every direction-sign mask."""
import functools
import math

import numpy as np

DEPTHS = (1, 2, 3, 5, 8)
# (depth, maxSpheresPerNode) -> spheres: the smallest counts at which the host walk of the parent
# commit popped every hb < 8 (depth - 1) at depth 3, 5 and 8 over the poses below
N_SPHERES = {1: 60, 2: 120, 3: 400, 5: 1200, 8: 2000}
SIZES = ((48, 32), (33, 17))
DIAGONALS = tuple((sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1))
# inside the field of random_spheres (a slab around the origin, centres 0.2 to 4.2 high), at
# middle height, so that the upward and the downward diagonals both look through spheres
EYE = (0.3, 1.7, -0.4)


def pose(ort, size, diag, samples=1, bounces=1):
    """Camera at EYE looking along diag (yaw / pitch of the reference's camera: front =
    (cos yaw cos pitch, sin pitch, sin yaw cos pitch))."""
    sx, sy, sz = diag
    yaw = math.degrees(math.atan2(sz, sx))
    pitch = math.degrees(math.asin(sy / math.sqrt(3.0)))
    return ort.FrameParams.default_camera(size[0], size[1], num_samples=samples, max_depth=bounces, position=EYE,
                                          yaw=yaw, pitch=pitch)


@functools.lru_cache(maxsize=None)
def scene(depth, m):
    import octreeraytracer_amd as ort
    s = ort.random_spheres(N_SPHERES[depth], 42)
    return s, ort.build_octree(s, depth, m)


@functools.lru_cache(maxsize=None)
def reference(depth, m, size, diag, samples=1, bounces=1):
    """The oracle's frame of a case (computed once per process, read-only)."""
    import octreeraytracer_amd as ort
    from oracle import oracle
    s, t = scene(depth, m)
    img = oracle.render(s, t, pose(ort, size, diag, samples, bounces))
    img.flags.writeable = False
    return img


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
