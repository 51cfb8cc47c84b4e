"""Sequences of calls on one context: the plan and the runner (tests/test_call_sequences.py on the
host, tests/test_gpu_call_sequences.py on the GPU).

tests/frame_sequences.py takes one context through every render route after every other.  This
plan does the same for the call families that came later and share state inside ort_ctx: the four
query calls (one grow-only QueryState), the two denoise calls (their staging buffers), the plain,
moments and adaptive accumulations (the whole-pixel pass kernel, the adaptive staging buffer) and
the scene actions that invalidate them.  Its pieces -- scenes, cameras, tiles, describe_output,
expected_buffer, Mismatch, the Runner loop, GpuAdapter, run_in_turn -- are frame_sequences'.

The calls ("names"): six stateful frame kinds as frame_sequences draws them; rays, rays_nearest,
rays_any, camera, radiance; denoise, denoise_var; pass_plain, pass_moments, pass_adaptive,
read_moments, read_counts, stats on three accumulations kept open through a sequence; reupload,
twin, build; and refused, one call that must fail with its documented code and write nothing.

The plan is a seeded, deterministic walk made of
  chains    for every name A and every other X the sandwich (A, X, A), both A with the same arguments
  variants  for every query and denoise name (A small, A much larger, A small) and (A on host
            pointers, A on device pointers, A on host pointers): the stale tail of a grow-only buffer
  tours     every name in shuffled order three times over, on the 181,769-node tree and on the tree
            of depth 9 (chains and variants run on the 105-node tree)
  large     the accumulations alone on a 272 x 248 frame: 17 x 16 = 272 workgroups of 16 x 16, more
            than the 256 the adaptive statistics kernel launches, so its stride loop is taken
  sweep     more draws of whatever value of a drawn dimension occurred fewer than ten times
cut into sequences of at most MAX_STEPS steps, each run on a fresh context and named by its seed.
A draw whose output equals the output of the step before or after it over the same buffer shape is
rejected, so a stale result is always visible.

Every output buffer is prefilled with FS.FILL and FS.SLACK bytes more than the call may write and is
compared byte for byte: the records' bits, zero words and miss records in padding rows, the prefill
after the last record and between pitched rows.  Where the header leaves the reported sphere open
(the drawn walk, ANY), the record is checked as frame_sequences.check_query checks it -- the t bits
and hit-or-miss are the reference's, the reported sphere traced alone gives that t -- and the bytes
after the records are still compared.

The references, computed once per argument set: oracle.render for frames and previews;
oracle.trace_rays and the one-sphere construction for rays and camera hits; ray_mode_sets' roots for
NEAREST and ANY; camera_sets.numpy_rays; ray_sets.numpy_normals; denoise_sets.atrous and
variance_sets.atrous_var (gamma through gamma_host); adaptive_sets.counts_np and traced_np for counts
and statistics.  Two references are the host emulation itself, which tests/test_radiance_query.py
and tests/test_variance.py tie to the oracle on the CPU: radiance with paths > 1, without GAMMA or
over rays that are no frame's (radiance_rays_host; end states always), and the moments
(accum_moments_host), from which a preview at a count whose strata no frame has is taken through
gamma_host.  Every name but read_moments has drawn variants whose reference is not the emulation
(non_emulation_names()); read_moments' mean, taken through gamma_host, is compared with the oracle's
frame wherever one exists (moments_tie()).

Out of scope, as for frame_sequences: groups and RCCL, the C++ Raytracer layer, and tiles with more
slots than the resident lanes of the pass kernel (only test_restart_does_not_wait covers them, GPU
against GPU).

replay(seed, first, last) runs a slice of a sequence on a fresh context from a Python prompt, to
shorten a failing sequence by hand (a mismatch only: a HIP error is read from the code, not run again)."""
import dataclasses
import functools
import random

import numpy as np

import adaptive_sets
import camera_sets
import denoise_sets
import frame_sequences as FS
import ray_mode_sets
import ray_sets
import variance_sets

FILL, SLACK = FS.FILL, FS.SLACK
MAX_STEPS = 250
BASE_SEED = 31730
assert BASE_SEED != FS.BASE_SEED

FRAMES = ("direct", "pipe_list", "pixel", "pixel_spec", "brute_pixel", "explicit_pipe")
QUERIES = ("rays", "rays_nearest", "rays_any", "camera", "radiance")
DENOISE = ("denoise", "denoise_var")
PASSES = ("pass_plain", "pass_moments", "pass_adaptive")
ACCUM = PASSES + ("read_moments", "read_counts", "stats")
SCENE_ACTIONS = ("reupload", "twin", "build")
NAMES = FRAMES + QUERIES + DENOISE + ACCUM + SCENE_ACTIONS + ("refused",)
SIZED = QUERIES + DENOISE     # the names of the size and pointer variants
VARIANTS = ("larger", "pointers")

N_RAYS = (1, 63, 129, 1000, 3001)
RADIANCE_FRAME = (97, 63)     # the frame whose pixels' rays and states radiance queries take
ACC = {False: (FS.ACC_SIZE, FS.ACC_N, FS.ACC_DEPTH), True: ((272, 248), 4, 2)}   # big: (size, N, depth)
FLOOR = adaptive_sets.FLOOR
THRESHOLDS = {"hold": 0.1, "zero": 0.0, "inf": float("inf")}
SIGMA_VARIANCE = 4.0
WANTS = (("rays",), ("hits",), ("hits", "rays"), ("hits", "normals"), ("hits", "normals", "rays"))

# refused: variant -> (family, the documented code's name)
REFUSALS = {
    "t_range_drawn": ("rays", "ORT_ERR_INVALID_ARG"),
    "normals_without_hits": ("camera", "ORT_ERR_INVALID_ARG"),
    "paths_0": ("radiance", "ORT_ERR_INVALID_ARG"),
    "iterations_7": ("denoise", "ORT_ERR_INVALID_ARG"),
    "variance_plain": ("accum", "ORT_ERR_INVALID_ARG"),
    "adaptive_on_plain": ("accum", "ORT_ERR_INVALID_ARG"),
    "radiance_explicit": ("explicit", "ORT_ERR_UNSUPPORTED"),
    "begin_explicit": ("explicit", "ORT_ERR_UNSUPPORTED"),
}

# What each name draws: dimension -> values (test_call_sequences.py counts every value).
BOOL = (0, 1)
DIMS = {
    "rays": {"device": BOOL, "sort": BOOL, "normals": BOOL, "use_octree": BOOL, "n": N_RAYS},
    "rays_nearest": {"device": BOOL, "sort": BOOL, "normals": BOOL, "use_octree": BOOL, "n": N_RAYS, "trange": BOOL},
    "rays_any": {"device": BOOL, "sort": BOOL, "normals": BOOL, "use_octree": BOOL, "n": N_RAYS, "trange": BOOL},
    "camera": {"device": BOOL, "which": camera_sets.WHICH, "tile": tuple(FS.TILES), "want": WANTS, "use_octree": BOOL,
               "size": FS.SIZES, "ns": (1, 4)},
    "radiance": {"device": BOOL, "sort": BOOL, "use_octree": BOOL, "n": N_RAYS, "source": ("set", "frame"), "paths": (1, 3),
                 "depth": (1, 4), "normalize": BOOL, "gamma": BOOL, "states_out": ("null", "separate", "equal")},
    "denoise": {"device": BOOL, "cols": (37, 300), "rows": (8, 21, 70), "fmt": ("rgb32f", "rgba8"), "pitched": BOOL,
                "inplace": BOOL, "iterations": (1, 3, 6)},
    "denoise_var": {"device": BOOL, "cols": (37, 300), "rows": (8, 21, 70), "fmt": ("rgb32f", "rgba8"), "pitched": BOOL,
                    "inplace": BOOL, "iterations": (1, 3, 6), "gamma": BOOL},
    "pass_plain": {"n": (2, 3, 4), "output": FS.OUTPUTS},
    "pass_moments": {"n": (2, 3, 4), "output": FS.OUTPUTS},
    "pass_adaptive": {"n": (2, 3, 4), "output": FS.OUTPUTS, "threshold": tuple(THRESHOLDS), "min_samples": (1, 3)},
    "read_moments": {"acc": ("plain", "moments", "adaptive"), "device": BOOL, "parts": ("mean", "variance", "both")},
    "read_counts": {"device": BOOL},
    "stats": {"threshold": tuple(THRESHOLDS), "min_samples": (1, 3), "n": (2, 3, 4)},
    "refused": {"variant": tuple(REFUSALS)},
}


@dataclasses.dataclass(frozen=True)
class Step:
    name: str
    scene: str = "d4"
    frame: FS.Step = None     # a frame name: the step as frame_sequences draws it
    args: tuple = ()          # sorted (dimension, value)
    tag: str = ""

    @property
    def a(self):
        return dict(self.args)

    @property
    def is_frame(self):
        return self.frame is not None

    def recipe(self):
        """What the two A of a sandwich share."""
        return dataclasses.replace(self, tag="")


def make(name, scene_name, tag="", **args):
    return Step(name, scene_name, None, tuple(sorted(args.items())), tag)


def acc_of(st):
    """The accumulation a step works on: "plain", "moments", "adaptive" or None."""
    if st.name in ("pass_plain", "pass_moments"):
        return st.name[5:]
    if st.name in ("pass_adaptive", "read_counts", "stats"):
        return "adaptive"
    if st.name == "read_moments":
        return st.a["acc"]
    if st.name == "refused" and REFUSALS[st.a["variant"]][0] == "accum":
        return "plain"
    return None


def criterion(a):
    return (a["n"], a["min_samples"], THRESHOLDS[a["threshold"]], FLOOR)


# ---- the state a sequence carries: shared by the generator and the runner ------------------------------
class State:
    """Which scene is uploaded and where the three accumulations stand.  advance(step) returns what
    the step implies before its own call: {"upload": (scene, twin, explicit, how) or None, "begin" /
    "restart": bool, "prime": the passes without a picture that come before a read of an
    accumulation that holds nothing yet}, and moves on."""

    def __init__(self):
        self.scene = None      # (name, twin, explicit)
        self.acc = {"plain": None, "moments": None, "adaptive": None}   # {"camera", "big", "passes", "valid"}

    def copy(self):
        c = State()
        c.scene = self.scene
        c.acc = {k: dict(v, passes=list(v["passes"])) if v else None for k, v in self.acc.items()}
        return c

    def advance(self, st):
        twin = self.scene[1] if self.scene else False
        do = {"upload": None, "begin": False, "restart": False, "prime": ()}
        n, which, how = st.name, acc_of(st), "upload"
        if st.is_frame:
            want = (st.scene, twin, FS.KINDS[n].explicit)
        elif n == "twin":
            want = (st.scene, not twin, False)
        elif n in ("reupload", "build"):
            want, how = (st.scene, twin, False), "build" if n == "build" else "upload"
        elif n == "refused" and REFUSALS[st.a["variant"]][0] == "explicit":
            want = (st.scene, twin, True)
        elif which or (n == "radiance" and st.a["use_octree"]):   # the whole-pixel walk: the compact layout
            want = (st.scene, twin, False)
        else:
            want = self.scene or (st.scene, False, False)
        if want != self.scene or n in SCENE_ACTIONS:
            do["upload"] = want + (how,)
            self.scene = want
            for a in self.acc.values():
                if a:
                    a["valid"] = False
        if which:
            a, is_pass = self.acc[which], n in PASSES
            fresh = {"camera": st.a["camera"], "big": st.a["big"], "passes": [], "valid": True}
            if a is None:
                do["begin"], a = True, fresh
            elif not a["valid"] or (is_pass and self.done(which) >= ACC[a["big"]][1]):
                do["restart"], a = True, fresh
            self.acc[which] = a
            if is_pass:
                a["passes"].append(criterion(st.a) if n == "pass_adaptive" else (st.a["n"], 0, 0.0, FLOOR))
            elif not a["passes"]:
                if a["big"]:
                    do["prime"] = ((1, 0, 0.0, FLOOR),)
                elif which == "adaptive":   # two samples, then two more where the criterion holds nothing: two counts
                    do["prime"] = ((2, 0, 0.0, FLOOR), (2, 1, THRESHOLDS["hold"], FLOOR))
                else:   # 4 of 7: a count whose strata a frame has, so the oracle has a say
                    do["prime"] = ((4, 0, 0.0, FLOOR),)
                a["passes"].extend(do["prime"])
        return do

    def done(self, which):
        a = self.acc[which]
        return min(ACC[a["big"]][1], sum(p[0] for p in a["passes"]))


# ---- references: computed once, read-only -----------------------------------------------------------------
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def ray_source(scene_name, source):
    """(rays (n, 6), states (n, 2)) of a source: ("set",) -- ray_sets.make_rays for the scene with
    rng_states(n, 7) -- or ("frame", camera): the rays and RNG states radiance() starts from for the
    pixels of the 1-sample RADIANCE_FRAME (radiance_sets.frame_inputs' construction on this camera)."""
    import octreeraytracer_amd as ort
    from oracle import oracle
    from octreeraytracer_amd.renderer import camera_query_host, rng_states
    if source[0] == "set":
        s, t = FS.scene(scene_name)
        rays = ray_sets.make_rays(ort, oracle, s, t, 1000 + FS.SCENES[scene_name][0])
        return _ro(rays, rng_states(len(rays), 7))
    w, h = RADIANCE_FRAME
    rays = camera_query_host(None, None, FS.frame_params(RADIANCE_FRAME, (1, 1), 1, source[1]), hits=False).reshape(-1, 6)
    return _ro(np.ascontiguousarray(rays), frame_states(w, h))


@functools.lru_cache(maxsize=None)
def frame_states(w, h):
    from oracle import oracle
    from radiance_sets import fract32
    F = np.float32
    states = np.empty((w * h, 2), F)
    for y in range(h):
        for x in range(w):
            r = oracle.rand_sequence(float(F(F(F(x) + F(0.5)) / F(w))), float(F(F(F(y) + F(0.5)) / F(h))), 6)
            states[y * w + x] = (fract32(F(r[4]) * F(1664525.0)), r[5])
    return states


def selection(a):
    return np.arange(a["n"]) * a["stride"]


def drawn_records(scene_name, rays):
    """The oracle's {hit, t bits} of rays through the tree, (n, 2), and through the one-sphere scene
    of every sphere, (spheres, n, 2): frame_sequences.query_reference for any rays."""
    import octreeraytracer_amd as ort
    from oracle import oracle
    s, t = FS.scene(scene_name)
    rays = np.ascontiguousarray(rays)
    if not len(rays):
        return np.zeros((0, 2), np.int32), np.zeros((s.n, 0, 2), np.int32)
    return oracle.trace_rays(s, t, rays), np.stack([oracle.trace_rays(*ray_sets.one_sphere_scene(ort, s, k), rays)
                                                    for k in range(s.n)])


@functools.lru_cache(maxsize=None)
def set_records(scene_name):
    return _ro(*drawn_records(scene_name, ray_source(scene_name, ("set",))[0]))


def check_drawn(rec, tree, each, use_octree, inside=None):
    """'' or what is wrong with the (n, 2) int32 records {t bits, sphere}: frame_sequences.check_query
    over any rays; records where `inside` is False (rows past the frame) must be the miss record."""
    n = len(tree)
    if rec.shape != (n, 2):
        return f"query records of shape {rec.shape}"
    if inside is None:
        inside = np.ones(n, bool)
    t_bits, sphere = rec[:, 0], rec[:, 1]
    if use_octree:
        hit, want_bits = tree[:, 0] == 1, np.where(tree[:, 0] == 1, tree[:, 1], 0)
    else:
        t_each = np.where(each[:, :, 0] == 1, each[:, :, 1].view(np.float32), np.inf)
        best = t_each.argmin(axis=0) if n else np.zeros(0, np.int64)
        hit = np.isfinite(t_each[best, np.arange(n)])
        want_bits = np.where(hit, each[best, np.arange(n), 1], 0)
        bad = np.nonzero(inside & hit & (sphere != best))[0]
        if len(bad):
            return f"rays {bad[:5].tolist()} report spheres {sphere[bad[:5]].tolist()}, brute force {best[bad[:5]].tolist()}"
    hit = hit & inside
    want_bits = np.where(inside, want_bits, 0)
    bad = np.nonzero((t_bits != want_bits) | ((sphere >= 0) != hit))[0]
    if len(bad):
        return (f"{len(bad)} records are not the oracle's, first rays {bad[:5].tolist()}: t bits "
                f"{t_bits[bad[:5]].tolist()} want {want_bits[bad[:5]].tolist()}, sphere {sphere[bad[:5]].tolist()}")
    if (sphere[hit] >= each.shape[0]).any() or (sphere[~hit] != -1).any():
        return "sphere indices out of range"
    alone = each[sphere[hit], np.nonzero(hit)[0]]
    bad = np.nonzero(hit)[0][(alone[:, 0] != 1) | (alone[:, 1] != t_bits[hit])]
    if len(bad):
        return f"rays {bad[:5].tolist()} report spheres {sphere[bad[:5]].tolist()} that they do not hit at that t"
    return ""


@functools.lru_cache(maxsize=None)
def intervals(scene_name):
    """{t_min, t_max} for the scene's ray set: ray_mode_sets.intervals' recipe (default_rng(5), HAND's
    rays on top) over this scene's default-interval nearest hits."""
    rm, F = ray_mode_sets, np.float32
    s, _ = FS.scene(scene_name)
    rays = ray_source(scene_name, ("set",))[0]
    n = len(rays)
    rng = np.random.default_rng(5)
    t, sph = rm.nearest_of(rm.sphere_roots(s, rays), n, None)
    t_near = np.where(sph >= 0, t, F(10)).astype(np.float64)
    tmin = np.where(rng.random(n) < 0.5, 0.001, t_near * rng.uniform(0.0, 1.2, n))
    tmax = np.where(rng.random(n) < 0.3, float(rm.MAXFLOAT), t_near * rng.uniform(0.3, 3.0, n))
    out = np.stack([tmin, tmax], axis=1).astype(F)
    for i, (a, b) in rm.HAND.items():
        out[i] = (a, b)
    return _ro(out)


def mode_inputs(scene_name, a):
    idx = selection(a)
    rays = np.ascontiguousarray(ray_source(scene_name, ("set",))[0][idx])
    t_range = np.ascontiguousarray(intervals(scene_name)[idx]) if a.get("trange") else None
    return rays, t_range


@functools.lru_cache(maxsize=None)
def nearest_records(scene_name, n, stride, trange):
    """NEAREST's records (n, 2) int32 {t bits, sphere} and the roots table they come from."""
    s, _ = FS.scene(scene_name)
    rays, t_range = mode_inputs(scene_name, {"n": n, "stride": stride, "trange": trange})
    table = ray_mode_sets.sphere_roots(s, rays)
    t, sph = ray_mode_sets.nearest_of(table, n, t_range)
    return _ro(np.ascontiguousarray(np.stack([t.view(np.int32), sph], axis=1))), table


def check_any(rec, scene_name, a):
    """ANY: hit-or-miss is NEAREST's; the reported sphere's accepted root in the ray's interval is t."""
    rm = ray_mode_sets
    s, _ = FS.scene(scene_name)
    want, (ri, ki, near, far) = nearest_records(scene_name, a["n"], a["stride"], a.get("trange", 0))
    n = a["n"]
    if rec.shape != (n, 2):
        return f"records of shape {rec.shape}"
    t, sphere = np.ascontiguousarray(rec[:, 0]).view(np.float32), rec[:, 1]
    bad = np.nonzero((sphere >= 0) != (want[:, 1] >= 0))[0]
    if len(bad):
        return f"rays {bad[:5].tolist()}: hit-or-miss is not NEAREST's (spheres {sphere[bad[:5]].tolist()})"
    if (sphere >= s.n).any() or (sphere < -1).any() or (rec[sphere < 0, 0] != 0).any():
        return "sphere indices out of range, or a miss with t bits"
    _, t_range = mode_inputs(scene_name, a)
    tmin, tmax, valid = rm.clean_interval(t_range, n)
    rows = np.nonzero(sphere >= 0)[0]
    key, wanted = ri * s.n + ki, rows * s.n + sphere[rows]
    at = np.minimum(np.searchsorted(key, wanted), max(len(key) - 1, 0))
    ck = np.full(len(rows), np.inf, np.float32)
    if len(key):
        found = key[at] == wanted
        ck[found] = rm.accepted(near[at[found]], far[at[found]], tmin[rows[found]], tmax[rows[found]], valid[rows[found]])
    bad = rows[ck.view(np.int32) != t[rows].view(np.int32)]
    if len(bad):
        return f"rays {bad[:5].tolist()} report spheres {sphere[bad[:5]].tolist()} whose accepted root is not t"
    return ""


def normals_of(scene_name, rays, rec):
    s, _ = FS.scene(scene_name)
    t, sphere = np.ascontiguousarray(rec[:, 0]).view(np.float32), np.ascontiguousarray(rec[:, 1])
    return ray_sets.numpy_normals(s, rays, t, sphere)


def camera_params(a):
    return FS.frame_params(a["size"], (a["ns"], 1), a["use_octree"], a["camera"])


@functools.lru_cache(maxsize=None)
def camera_frame(scene_name, camera, size, which, ns):
    """The whole frame's camera rays (H, W, 6) by camera_sets.numpy_rays and their drawn records."""
    from oracle import oracle
    rays = camera_sets.numpy_rays(oracle, FS.frame_params(size, (ns if which == "first_sample" else 1, 1), 1, camera), which)
    tree, each = drawn_records(scene_name, rays.reshape(-1, 6))
    return _ro(rays, tree, each)


def camera_reference(scene_name, a):
    """(rays (n, 6), tree (n, 2), each (S, n, 2), inside (n,)) of the tile's pixels in output order."""
    W, H = a["size"]
    x0, w, y0, rows, bh, bs = FS.TILES[a["tile"]](W, H)
    full, tree, each = camera_frame(scene_name, a["camera"], a["size"], a["which"], a["ns"])
    ys = FS.pixel_rows((x0, w, y0, rows, bh, bs))
    inside = np.repeat(ys < H, w)
    px = (np.minimum(ys, H - 1)[:, None] * W + x0 + np.arange(w)[None, :]).reshape(-1)
    rays = np.where(inside[:, None], full.reshape(-1, 6)[px], np.float32(0)).astype(np.float32)
    return rays, tree[px], each[:, px], inside


def radiance_inputs(scene_name, a):
    source = ("set",) if a["source"] == "set" else ("frame", a["camera"])
    rays, states = ray_source(scene_name, source)
    idx = selection(a)
    return np.ascontiguousarray(rays[idx]), np.ascontiguousarray(states[idx])


def radiance_by_oracle(a):
    return a["source"] == "frame" and a["paths"] == 1 and a["gamma"] and not a["normalize"]


@functools.lru_cache(maxsize=None)
def _radiance_reference(scene_name, twin, args):
    from octreeraytracer_amd.renderer import radiance_rays_host
    a = dict(args)
    s, t = FS.scene(scene_name, twin)
    rays, states = radiance_inputs(scene_name, a)
    rad, end = radiance_rays_host(s, t if a["use_octree"] else None, rays, states, max_depth=a["depth"], paths=a["paths"],
                                  use_octree=bool(a["use_octree"]), normalize=bool(a["normalize"]), gamma=bool(a["gamma"]),
                                  states_out=True)
    if radiance_by_oracle(a):  # the oracle's 1-sample frame: the same pixels
        frame = FS.frame_reference(scene_name, twin, a["camera"], RADIANCE_FRAME, (1, a["depth"]), a["use_octree"],
                                   FS.TILES["full"](*RADIANCE_FRAME))
        rad = np.ascontiguousarray(frame.reshape(-1, 3)[selection(a)])
    return _ro(rad, end)


def radiance_reference(scene_name, twin, a):
    """(radiance (n, 3), end states (n, 2)): the oracle's frame where radiance_by_oracle, else (and the
    end states always) radiance_rays_host."""
    keys = ("source", "camera", "n", "stride", "use_octree", "depth", "paths", "normalize", "gamma")
    return _radiance_reference(scene_name, twin, tuple((k, a[k]) for k in keys))


def denoise_inputs(a):
    """(image, t, sphere, normals, variance or None) (rows, cols[, 3]): the top left of
    denoise_sets.synthetic(), its channels rolled by a["img"], its guides mirrored by a["gflip"]."""
    img, t, sph, nrm = denoise_sets.synthetic()
    rows, cols = a["rows"], a["cols"]
    img = np.roll(img[:rows, :cols], a["img"], axis=2)
    g = [x[:rows, :cols][:, ::-1] if a["gflip"] else x[:rows, :cols] for x in (t, sph, nrm)]
    var = variance_sets.synthetic_variance(cols, rows) if "gamma" in a else None
    return (np.ascontiguousarray(img),) + tuple(np.ascontiguousarray(x) for x in g) + (var,)


@functools.lru_cache(maxsize=None)
def _denoise_reference(rows, cols, img, gflip, iterations, var, gamma):
    a = {"rows": rows, "cols": cols, "img": img, "gflip": gflip}
    if var:
        a["gamma"] = gamma
    image, t, sph, nrm, variance = denoise_inputs(a)
    if not var:
        return _ro(denoise_sets.atrous(image, t, sph, nrm, iterations=iterations))
    out = variance_sets.atrous_var(image, t, sph, nrm, variance, SIGMA_VARIANCE, iterations=iterations)
    return _ro(np.ascontiguousarray(variance_sets.gamma(out) if gamma else out))


def denoise_reference(a):
    return _denoise_reference(a["rows"], a["cols"], a["img"], a["gflip"], a["iterations"], "gamma" in a, a.get("gamma", 0))


def denoise_description(a):
    """As frame_sequences.describe_output: how the filtered picture is written."""
    bpp = FS.BPP[a["fmt"]]
    stride = (a["cols"] + 3 if a["pitched"] else a["cols"]) * bpp
    return {"fmt": a["fmt"], "place": "tile", "device": bool(a["device"]), "pitch": stride if a["pitched"] else None,
            "row_bytes": a["cols"] * bpp, "stride": stride, "rows": a["rows"], "nbytes": a["rows"] * stride}


def picture_step(size, output="host_f32"):
    """A frame_sequences step that stands for a whole picture of `size` written as `output`."""
    return FS.Step("accum", size=size, tile="full", output=output)


def acc_params(acc):
    size, N, depth = ACC[acc["big"]]
    return FS.frame_params(size, (N, depth), 1, acc["camera"])


@functools.lru_cache(maxsize=None)
def prefix(scene_name, twin, camera, big):
    """{k: (mean, variance)} after k = 1 .. N uniform samples: accum_moments_host."""
    import octreeraytracer_amd as ort
    from octreeraytracer_amd.renderer import accum_moments_host
    s, t = FS.scene(scene_name, twin)
    size, N, depth = ACC[big]
    p = FS.frame_params(size, (N, depth), 1, camera)
    out = {k: accum_moments_host(s, t, p, ort.Tile.full(p), samples_done=k) for k in range(1, N + 1)}
    for m, v in out.values():
        _ro(m, v)
    return out


def counts_of(state, which):
    """Each pixel's count (H, W) int32 of an accumulation: adaptive_sets.counts_np over the prefixes."""
    name, twin, _ = state.scene
    acc = state.acc[which]
    (W, H), N, _ = ACC[acc["big"]]
    if which != "adaptive":
        return np.full((H, W), state.done(which), np.int32)
    return _counts(name, twin, acc["camera"], acc["big"], tuple(acc["passes"]))


@functools.lru_cache(maxsize=None)
def _counts(name, twin, camera, big, passes):
    (W, H), N, _ = ACC[big]
    if all(p[1] == 0 and p[2] == 0.0 for p in passes):  # uniform passes: no prefix is read
        return _ro(np.full((H, W), min(N, sum(p[0] for p in passes)), np.int32))
    return _ro(adaptive_sets.counts_np(prefix(name, twin, camera, big), N, passes, np.ones((H, 1), bool)))


def preview(state, which):
    """(picture (H, W, 3), by_oracle): the preview of an accumulation where it stands.  A pixel at a
    count k with (int)sqrt(k) == (int)sqrt(N) is the oracle's k-sample frame's; a picture with any
    other count is the moments emulation's mean through gamma_host (a plain pass: the prefix emulation)."""
    from octreeraytracer_amd.renderer import emulate_render_host, gamma_host
    import octreeraytracer_amd as ort
    name, twin, _ = state.scene
    acc = state.acc[which]
    size, N, depth = ACC[acc["big"]]
    counts = counts_of(state, which)
    ks = [int(k) for k in np.unique(counts)]
    if all(FS.isqrt(k) == FS.isqrt(N) for k in ks):
        pic = np.zeros(counts.shape + (3,), np.float32)
        for k in ks:
            ref = FS.frame_reference(name, twin, acc["camera"], size, (k, depth), 1, FS.TILES["full"](*size))
            pic[counts == k] = ref[counts == k]
        return pic, True
    if which == "plain":
        s, t = FS.scene(name, twin)
        p = acc_params(acc)
        return emulate_render_host(s, t, p, ort.Tile.full(p), samples_done=ks[0])[0], False
    mean, _ = adaptive_sets.moments_at(prefix(name, twin, acc["camera"], acc["big"]), counts)
    return gamma_host(mean).reshape(mean.shape), False


def moments_reference(state, which):
    name, twin, _ = state.scene
    acc = state.acc[which]
    return adaptive_sets.moments_at(prefix(name, twin, acc["camera"], acc["big"]), counts_of(state, which))


def stats_reference(state, crit):
    """ort_accum_adaptive_stats' record from the counts and adaptive_sets.traced_np."""
    name, twin, _ = state.scene
    acc = state.acc["adaptive"]
    N = ACC[acc["big"]][1]
    counts = counts_of(state, "adaptive")
    pre = prefix(name, twin, acc["camera"], acc["big"])
    pending = 0
    for k in np.unique(counts):
        at = counts == k
        if k == 0:
            pending += int(at.sum())
        else:
            pending += int((adaptive_sets.traced_np(int(k), N, crit[1], crit[2], crit[3], *pre[int(k)]) & at).sum())
    return {"pixels": int(counts.size), "samples": int(counts.sum(dtype=np.int64)), "pending": pending,
            "min_count": int(counts.min()), "max_count": int(counts.max())}


def moments_tie(state, which):
    """True where the reference mean of read_moments, through gamma_host, is the oracle's frame (None
    where the counts have no frame): what ties read_moments' emulated reference to the oracle."""
    from octreeraytracer_amd.renderer import gamma_host
    pic, by_oracle = preview(state, which)
    if not by_oracle:
        return None
    mean, _ = moments_reference(state, which)
    return not FS.differs(gamma_host(mean).reshape(mean.shape), pic)


# ---- what a step must write ------------------------------------------------------------------------------
@dataclasses.dataclass
class Out:
    key: str            # the buffer's name in what the adapter returns
    nbytes: int         # the bytes the call may write; SLACK prefilled bytes follow
    want: object = None   # uint8 (nbytes,), or None where `check` judges the records
    check: object = None  # f(got uint8 (nbytes,), all buffers) -> '' or what is wrong
    emulated: bool = False  # the reference is the host emulation's


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _records(got):
    return got.view(np.int32).reshape(-1, 2)


def expect(state, st):
    """(outs, primary): the buffers the step's call gets, with what they must hold afterwards, and
    the reference array that a neighbouring step's is compared with (None: nothing to compare)."""
    a, name = st.a, st.name
    scene_name, twin, _ = state.scene
    if name == "rays":
        tree, each = set_records(scene_name)
        idx = selection(a)
        tree, each = tree[idx], each[:, idx]
        rays = ray_source(scene_name, ("set",))[0][idx]
        outs = [Out("hits", 8 * a["n"], check=lambda got, all_: check_drawn(_records(got), tree, each, a["use_octree"]))]
        if a["normals"]:
            outs.append(Out("normals", 12 * a["n"], check=lambda got, all_: _same(
                got, normals_of(scene_name, rays, _records(all_["hits"][:8 * a["n"]])), "normals")))
        return outs, np.ascontiguousarray(tree[:, 1])
    if name in ("rays_nearest", "rays_any"):
        want, _ = nearest_records(scene_name, a["n"], a["stride"], a["trange"])
        rays, _ = mode_inputs(scene_name, a)
        if name == "rays_nearest":
            outs = [Out("hits", 8 * a["n"], _u8(want))]
        else:
            outs = [Out("hits", 8 * a["n"], check=lambda got, all_: check_any(_records(got), scene_name, a))]
        if a["normals"]:
            outs.append(Out("normals", 12 * a["n"], check=lambda got, all_: _same(
                got, normals_of(scene_name, rays, _records(all_["hits"][:8 * a["n"]])), "normals")))
        return outs, np.ascontiguousarray(want[:, 0])
    if name == "camera":
        rays, tree, each, inside = camera_reference(scene_name, a)
        n = len(rays)
        outs = []
        if "rays" in a["want"]:
            outs.append(Out("rays", 24 * n, _u8(rays)))
        if "hits" in a["want"]:
            outs.append(Out("hits", 8 * n, check=lambda got, all_: check_drawn(_records(got), tree, each, a["use_octree"], inside)))
        if "normals" in a["want"]:
            outs.append(Out("normals", 12 * n, check=lambda got, all_: _same(
                got, normals_of(scene_name, rays, _records(all_["hits"][:8 * n])), "normals")))
        return outs, (rays if "rays" in a["want"] else np.ascontiguousarray(tree[:, 1])) if n else None
    if name == "radiance":
        rad, end = radiance_reference(scene_name, twin, a)
        outs = [Out("radiance", 12 * a["n"], _u8(rad), emulated=not radiance_by_oracle(a))]
        if a["states_out"] != "null":
            outs.append(Out("states_out", 8 * a["n"], _u8(end), emulated=True))
        return outs, rad
    if name in DENOISE:
        d = denoise_description(a)
        ref = denoise_reference(a)
        want = FS.expected_buffer(picture_step((a["cols"], a["rows"])), ref, d)
        return [Out("out", d["nbytes"], want[:d["nbytes"]])], ref
    if name in PASSES:
        which = acc_of(st)
        size = ACC[a["big"]][0]
        pic, by_oracle = preview(state, which)
        fs = picture_step(size, a["output"])
        d = FS.describe_output(fs)
        want = FS.expected_buffer(fs, pic, d)
        return [Out("out", d["nbytes"], want[:d["nbytes"]], emulated=not by_oracle)], pic
    if name == "read_moments":
        mean, var = moments_reference(state, a["acc"])
        outs = []
        if a["parts"] in ("mean", "both"):
            outs.append(Out("mean", mean.nbytes, _u8(mean), emulated=True))
        if a["parts"] in ("variance", "both"):
            outs.append(Out("variance", var.nbytes, _u8(var), emulated=True))
        return outs, mean if a["parts"] != "variance" else var
    if name == "read_counts":
        counts = counts_of(state, "adaptive")
        return [Out("counts", counts.nbytes, _u8(counts))], counts
    if name == "stats":
        want = stats_reference(state, criterion(a))
        return [Out("stats", 0, want)], np.array(list(want.values()), np.int64)
    if name == "refused":
        return [], None
    return [], None


def _same(got, want, what):
    want = _u8(want)
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = np.nonzero(got[:len(want)] != want[:len(got)])[0]
        return f"{what}: {len(bad)} bytes differ, the first at byte {int(bad[0]) if len(bad) else min(len(got), len(want))}"
    return ""


def primary(state, st):
    """After advance(st): the reference array the step's main output is made of, or None."""
    if st.is_frame:
        name, twin, _ = state.scene
        f = st.frame
        ref = FS.frame_reference(name, twin, f.camera, f.size, f.shape, f.use_octree, FS.tile_of(f))
        return ref if ref.size else None
    return expect(state, st)[1]


def differs(a, b):
    if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
        return True
    return not np.array_equal(_u8(a), _u8(b))


# ---- the generator -------------------------------------------------------------------------------------
def _draw(rng, name, scene_name, tag="", big=False, force=None):
    """A step of the call `name`, its free dimensions drawn (force: dimension -> value)."""
    force = force or {}
    if name in FRAMES:
        f = FS._draw(rng, name, scene_name)
        return Step(name, scene_name, f, (), tag)
    if name in SCENE_ACTIONS:
        return Step(name, scene_name, None, (), tag)
    a = {k: force[k] if k in force else rng.choice(v) for k, v in DIMS[name].items()}
    misc = {k: rng.choice(v) for k, v in FS.MISC.items()}
    a["options"] = tuple(sorted((k, v) for k, v in misc.items() if FS.OPTION_DEFAULTS[k] != v))
    if "n" in a and name in QUERIES:
        total = RADIANCE_FRAME[0] * RADIANCE_FRAME[1] if a.get("source") == "frame" else ray_sets.N_RAYS
        a["stride"] = rng.choice([k for k in (1, 2, 3) if (a["n"] - 1) * k < total])
    if name == "camera":
        a["camera"] = rng.choice(tuple(FS.CAMERAS))
    if name == "radiance":
        a["camera"] = rng.choice(("chart", "turned"))
        if a["source"] == "frame" and rng.random() < 0.6 and not {"paths", "gamma", "normalize"} & set(force):
            a.update(paths=1, gamma=1, normalize=0)   # the variant whose reference is the oracle's frame
    if name in DENOISE:
        a["img"], a["gflip"] = rng.choice((0, 1, 2)), rng.choice(BOOL)
        if a["inplace"] and "inplace" in force:
            a["fmt"] = "rgb32f"
        a["inplace"] = int(a["inplace"] and a["fmt"] == "rgb32f")   # (in place: the image's format)
    if name in ACCUM or name == "refused":
        a["camera"], a["big"] = rng.choice(("chart", "turned")), big
    if big and "n" in a and "n" not in force:
        a["n"] = rng.choice((1, 2))
    if name == "read_moments":
        if force.get("parts", "mean") != "mean" and "acc" not in force:
            a["acc"] = rng.choice(("moments", "adaptive"))
        if a["acc"] == "plain":   # (an accumulation without moments has a mean only)
            a["parts"] = "mean"
    return make(name, scene_name, tag, **a)


class _Walk:
    """One sequence being written: its steps, its state, the reference of its last step."""

    def __init__(self, rng):
        self.rng, self.steps, self.state, self.last = rng, [], State(), None

    def add(self, st):
        self.state.advance(st)
        self.last = primary(self.state, st)
        self.steps.append(st)

    def fits(self, make_step, then=None, tries=400):
        for _ in range(tries):
            st = make_step()
            state = self.state.copy()
            state.advance(st)
            ref = primary(state, st)
            if not differs(self.last, ref):
                continue
            if then is not None:
                state.advance(then)
                if not differs(ref, primary(state, then)):
                    continue
            return st
        if tries < 400:
            return None
        raise AssertionError("no draw differs from its neighbours")

    def sandwich(self, a, make_x):
        """(A,) X, A -- A is already the last step."""
        self.add(self.fits(make_x, then=a))
        self.add(a)


def _chain(w, a_name, scene_name):
    rng = w.rng
    others = [n for n in NAMES if n != a_name]
    rng.shuffle(others)
    tag = f"chain:{a_name}"
    force = {"tile": rng.choice(("full", "band", "sub"))} if a_name == "camera" else None
    if a_name == "pass_adaptive":  # (passes that hold some pixels, and four of them to the finished frame)
        force = {"threshold": "hold", "n": 2}
    a = w.fits(lambda: _draw(rng, a_name, scene_name, tag, force=force))
    w.add(a)
    for x in others:
        w.sandwich(a, lambda: _draw(rng, x, scene_name, tag))


LARGER = {"rays": ({"n": 63}, {"n": 3001}), "rays_nearest": ({"n": 129}, {"n": 3001}), "rays_any": ({"n": 1}, {"n": 3001}),
          "camera": ({"size": (48, 32), "tile": "sub"}, {"size": (97, 63), "tile": "full"}),
          "radiance": ({"n": 63}, {"n": 3001}),
          "denoise": ({"cols": 37, "rows": 8}, {"cols": 300, "rows": 70}),
          "denoise_var": ({"cols": 37, "rows": 21}, {"cols": 300, "rows": 70})}


def _variants(w, name, scene_name):
    rng = w.rng
    for v in VARIANTS:
        tag = f"variant:{v}:{name}"
        small, other = LARGER[name] if v == "larger" else ({"device": 0}, {"device": 1})
        if v == "pointers" and "n" in DIMS[name]:
            small = dict(small, n=rng.choice((63, 129, 1000)))
        a = w.fits(lambda: _draw(rng, name, scene_name, tag, force=small))
        w.add(a)
        if v == "larger" and "stride" in a.a:
            other = dict(other, stride=1)
        elif v == "pointers":  # the same size through the other kind of pointer, over other rays or another image
            if "stride" in a.a:
                other = dict(other, stride=a.a["stride"] % 3 + 1)
            elif name == "camera":
                other = dict(other, camera="turned" if a.a["camera"] != "turned" else "chart")
            else:
                other = dict(other, img=(a.a["img"] + 1) % 3)
        x = make(name, scene_name, tag, **dict(a.a, **other))
        w.sandwich(a, lambda: x)


def _tour(w, scene_name):
    rng = w.rng
    for rep in range(3):
        names = list(NAMES)
        rng.shuffle(names)
        for n in names:
            w.add(w.fits(lambda: _draw(rng, n, scene_name, f"tour:{scene_name}")))


HOLD = {"threshold": "hold", "min_samples": 1}
LARGE_ROUND = (("pass_adaptive", {"n": 2, "threshold": "zero"}), ("stats", HOLD), ("pass_adaptive", dict(HOLD, n=1)),
               ("read_counts", {}), ("stats", HOLD), ("read_moments", {"acc": "adaptive"}), ("pass_moments", {}),
               ("read_moments", {"acc": "moments"}), ("pass_adaptive", dict(HOLD, n=1)), ("stats", {}), ("read_counts", {}),
               ("read_moments", {"acc": "adaptive"}), ("pass_adaptive", {"n": 2, "threshold": "zero"}), ("stats", {}))


def _large(w, scene_name):
    """The accumulations alone on the 272 x 248 frame, three times over: two samples for every pixel,
    then passes that hold the converged pixels, with counts, statistics and moments read in between,
    and a last pass that finishes the frame (the next round restarts it)."""
    rng = w.rng
    for rep in range(3):
        for n, force in LARGE_ROUND:
            w.add(w.fits(lambda: _draw(rng, n, scene_name, "large", big=True, force=force)))


# Names that draw a dimension alike count its values together.
FAMILY = {"rays": "rays", "rays_nearest": "rays", "rays_any": "rays", "radiance": "rays", "denoise": "denoise",
          "denoise_var": "denoise", "pass_plain": "pass", "pass_moments": "pass", "pass_adaptive": "pass", "stats": "pass"}


def occurrences(seqs):
    """Counter of (family, dimension, value) over the steps of sequences."""
    import collections
    seen = collections.Counter()
    for steps in seqs:
        for st in steps:
            if st.name in DIMS and st.tag != "large":
                seen.update((FAMILY.get(st.name, st.name), k, st.a[k]) for k in DIMS[st.name])
    return seen


@functools.lru_cache(maxsize=None)
def plan():
    """{seed: tuple of steps}: every sequence of the plan, the same on every call."""
    parts = [("chain", n) for n in NAMES] + [("variants", n) for n in SIZED]
    seqs, w = {}, None

    def close():
        if w is not None and w.steps:
            seqs[BASE_SEED + len(seqs)] = tuple(w.steps)

    def fresh():
        return _Walk(random.Random(BASE_SEED + len(seqs)))

    for what, name in parts:
        need = 2 * len(NAMES) - 1 if what == "chain" else 3 * len(VARIANTS)
        if w is None or len(w.steps) + need > MAX_STEPS:
            close()
            w = fresh()
        (_chain if what == "chain" else _variants)(w, name, "d4")
    close()
    for scene_name in ("d6", "deep"):
        w = fresh()
        _tour(w, scene_name)
        close()
    w = fresh()
    _large(w, "d4")
    close()
    # sweep: every value of every drawn dimension at least ten times
    w = fresh()
    seen = occurrences(seqs.values())
    for name, dims in DIMS.items():
        for k, values in dims.items():
            for v in values:
                for _ in range(max(0, 10 - seen[(FAMILY.get(name, name), k, v)])):
                    if len(w.steps) >= MAX_STEPS:
                        close()
                        w = fresh()
                    st = w.fits(lambda: _draw(w.rng, name, "d4", "sweep", force={k: v}), tries=20)
                    if st is None:  # every such draw repeats the output before it: a frame in between
                        w.add(_draw(w.rng, "direct", "d4", "sweep"))
                        st = w.fits(lambda: _draw(w.rng, name, "d4", "sweep", force={k: v}))
                    w.add(st)
                    seen.update((FAMILY.get(name, name), kk, st.a[kk]) for kk in DIMS[name])
    close()
    assert distinct_count_steps(seqs) >= 10, "the adaptive accumulation seldom holds two distinct counts"
    return seqs


def distinct_count_steps(seqs):
    """The checked steps at which the small adaptive accumulation holds at least two distinct counts."""
    found = 0
    for steps in seqs.values():
        state = State()
        for st in steps:
            state.advance(st)
            if acc_of(st) == "adaptive" and not st.a["big"]:
                found += len(np.unique(counts_of(state, "adaptive"))) >= 2
    return found


def seeds():
    return tuple(plan())


def large_seed():
    return next(seed for seed, steps in plan().items() if steps[0].tag == "large")


# Sequences that once failed, cut down by hand: name -> steps.
REGRESSIONS = {}


def walk(steps):
    """(step, state after its advance) along a sequence."""
    state = State()
    for st in steps:
        state.advance(st)
        yield st, state


def totals():
    """(sequences, steps, distinct references) of the plan."""
    refs = set()
    for steps in plan().values():
        for st, state in walk(steps):
            ref = primary(state, st)
            if ref is not None:
                refs.add(_u8(ref).tobytes())
    return len(plan()), sum(len(s) for s in plan().values()), len(refs)


def non_emulation_names():
    """The names with at least one step in the plan none of whose references is the emulation's."""
    names = set(FRAMES) | set(SCENE_ACTIONS)
    for steps in plan().values():
        for st, state in walk(steps):
            if not st.is_frame and st.name not in SCENE_ACTIONS:
                outs = expect(state, st)[0]
                if st.name == "refused" or (outs and not any(o.emulated for o in outs)):
                    names.add(st.name)
    return names


# ---- the runner -------------------------------------------------------------------------------------------
Mismatch = FS.Mismatch


class Runner(FS.Runner):
    """frame_sequences.Runner over this plan's steps: the same loop, batches and ending on a HIP error."""

    def __init__(self, adapter, steps, seed=None, first=0, batch=1):
        super().__init__(adapter, steps, seed, first, batch)
        self.state = State()

    def fail(self, index, state, text):
        i = index - self.first
        before = "\n".join(f"    {self.first + j}: {self.all[j]}" for j in range(max(0, i - 8), i))
        raise Mismatch(self.seed, index, f"seed {self.seed}, step {index}: {text}\n  step: {self.all[i]}\n"
                       f"  scene (name, twin, explicit): {state.scene}; accumulations: {state.acc}\n"
                       f"  the steps before it:\n{before}\n"
                       f"  call_sequences.replay({self.seed}, first, {index}) runs a slice again")

    def issue(self, index, st):
        ad = self.adapter
        opts = dict(FS.OPTION_DEFAULTS)
        opts.update(st.frame.options if st.is_frame else st.a.get("options", ()))
        for k, v in opts.items():
            if self.set.get(k) != v:
                ad.set_option(k, v)
                self.set[k] = v
        do = self.state.advance(st)
        state = self.state.copy()
        if do["upload"]:
            name, twin, explicit, how = do["upload"]
            s, t = FS.scene(name, twin)
            ad.set_option("force_layout", 1 if explicit else 0)
            if how == "build":
                ad.upload(s, None, build=FS.SCENES[name])
            else:
                ad.upload(s, t)
        name, twin, _ = state.scene
        if st.is_frame:
            f = st.frame
            d = FS.describe_output(f)
            ref = FS.frame_reference(name, twin, f.camera, f.size, f.shape, f.use_octree, FS.tile_of(f))
            h = ad.render(FS.frame_params(f.size, f.shape, f.use_octree, f.camera), FS.tile_of(f), d)
            self.pending.append((index, st, state, "frame", h, (ref, d)))
            return
        if st.name in SCENE_ACTIONS:
            return
        which = acc_of(st)
        if which:
            acc = state.acc[which]
            if do["begin"]:
                ad.acc_begin(which, acc_params(acc), FS.TILES["full"](*ACC[acc["big"]][0]))
            elif do["restart"]:
                ad.acc_restart(which, acc_params(acc))
            for c in do["prime"]:
                ad.acc_pass(which, c[0], c if which == "adaptive" else None, None)
        outs, _ = expect(state, st)
        h = ad.call(st, state, {o.key: o.nbytes for o in outs})
        self.pending.append((index, st, state, "call", h, outs))

    def collect(self):
        if not self.pending:
            return
        self.adapter.sync()
        pending, self.pending = self.pending, []
        for index, st, state, what, h, ref in pending:
            if what == "frame":
                pic, d = ref
                got = self.adapter.read(h)
                if got is None:
                    assert FS.tile_of(st.frame)[1] * FS.tile_of(st.frame)[3] == 0
                    continue
                want = FS.expected_buffer(st.frame, pic, d)
                if got.shape != want.shape or not np.array_equal(got, want):
                    self.fail(index, state, f"the {d['fmt']} picture ({st.frame.output}) is not the oracle's: "
                              + FS.first_differences(got, want, d))
                continue
            got = self.adapter.read_all(h)
            if st.name == "refused":
                from octreeraytracer_amd import _lib as L
                code, bufs = got
                want_code = getattr(L, REFUSALS[st.a["variant"]][1])
                if code != want_code:
                    self.fail(index, state, f"refused ({st.a['variant']}): returned {code}, the header says {want_code}")
                for key, buf in bufs.items():
                    if (buf != FILL).any():
                        self.fail(index, state, f"refused ({st.a['variant']}): {int((buf != FILL).sum())} bytes of {key} were written")
                continue
            for o in ref:
                if o.key == "stats":
                    if got["stats"] != o.want:
                        self.fail(index, state, f"adaptive_stats {got['stats']} is not the reference's {o.want}")
                    continue
                buf = got.get(o.key)
                if buf is None or buf.shape != (o.nbytes + SLACK,):
                    self.fail(index, state, f"{st.name}: buffer {o.key} is {None if buf is None else buf.shape}")
                if (buf[o.nbytes:] != FILL).any():
                    at = o.nbytes + int(np.nonzero(buf[o.nbytes:] != FILL)[0][0])
                    self.fail(index, state, f"{st.name}: {o.key} is written after its last record (byte {at} of {o.nbytes} + {SLACK})")
                text = _same(buf[:o.nbytes], o.want, o.key) if o.want is not None else o.check(buf[:o.nbytes], got)
                if text:
                    self.fail(index, state, f"{st.name}: {text}" + (" (reference: the host emulation)" if o.emulated else ""))
            extra = set(got) - {o.key for o in ref}
            for key in extra:   # a buffer the call was not asked to write
                if (got[key] != FILL).any():
                    self.fail(index, state, f"{st.name}: {key}, which the call was not given, was written")


def run(adapter, steps, seed=None, first=0, batch=1):
    Runner(adapter, steps, seed, first, batch).run()


run_in_turn = FS.run_in_turn


# ---- the adapter over a Renderer ---------------------------------------------------------------------------
class GpuAdapter(FS.GpuAdapter):
    """frame_sequences.GpuAdapter with the later calls, made through the C ABI on prefilled byte
    buffers.  stream=True: every call that takes a stream runs on the one caller's stream, host
    pointers turned into device pointers, nothing waited for until sync(); uploads, ort_accum_begin
    and ort_accum_adaptive_stats take no stream: the adapter waits for the stream before them."""

    def __init__(self, ort, stream=None):
        super().__init__(ort, stream)
        self.accs = {}

    def close(self):
        self.sync()
        for a in self.accs.values():
            a.close()
        self.accs = {}
        super().close()

    # buffers
    def _device(self, asked):
        return bool(asked) or self.stream is not None

    def _on_stream(self):
        """What torch work of this adapter runs under: the caller's stream, or torch's own."""
        import contextlib
        return self.torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _out(self, nbytes, device):
        if self._device(device):
            with self._on_stream():
                return self.torch.full((nbytes + SLACK,), FILL, dtype=self.torch.uint8, device="cuda:0")
        return np.full(nbytes + SLACK, FILL, np.uint8)

    def _in(self, array, device):
        array = np.ascontiguousarray(array)
        if self._device(device):
            with self._on_stream():
                return self.torch.from_numpy(array.copy()).to("cuda:0")
        return array.copy()

    def _ready(self):
        if self.stream is None:
            self.torch.cuda.current_stream().synchronize()   # the context's stream does not wait for torch's

    @staticmethod
    def _p(buf):
        import ctypes as C
        if buf is None:
            return None
        return C.c_void_p(buf.ctypes.data if isinstance(buf, np.ndarray) else buf.data_ptr())

    def _s(self):
        import ctypes as C
        return C.c_void_p(self._handle()) if self._handle() else None

    def read_all(self, h):
        code, bufs = h
        out = {k: (v if isinstance(v, (np.ndarray, dict)) else v.cpu().numpy()) for k, v in bufs.items() if not k.startswith("_")}
        return (code, out) if code is not None else out

    # accumulations
    def acc_begin(self, which, params, tile):
        self.sync()
        self.accs[which] = self.r.accumulate(params, self.ort.Tile(*tile), moments=which == "moments", adaptive=which == "adaptive")

    def acc_restart(self, which, params):
        self.accs[which].restart(params)

    def acc_pass(self, which, n, crit, d):
        """A pass of n samples (crit: the adaptive criterion, or None for ort_accum_render) with its
        preview written as d says (None: no picture).  Returns the prefilled buffer."""
        acc = self.accs[which]
        buf, out = (None, False) if d is None else self._buffer(d, 1)
        kw = {} if d is None else dict(format=d["fmt"], row_pitch=d["pitch"], place=d["place"])
        if crit is None:
            acc.step(n, out=out, stream=self._handle(), **kw)
        else:
            acc.step_adaptive(crit[0], crit[2], crit[1], crit[3], out=out, stream=self._handle(), **kw)
        return buf

    def call(self, st, state, sizes):
        import ctypes as C
        from octreeraytracer_amd import _lib as L
        a, name, lib, ctx = st.a, st.name, self.r._lib, self.r._ctx
        check = self.r._check
        scene_name = state.scene[0]
        if name in ("rays", "rays_nearest", "rays_any"):
            dev = a["device"]
            if name == "rays":
                rays, t_range = ray_source(scene_name, ("set",))[0][selection(a)], None
            else:
                rays, t_range = mode_inputs(scene_name, a)
            bufs = {"_rays": self._in(rays, dev), "hits": self._out(8 * a["n"], dev),
                    "normals": self._out(12 * a["n"], dev)}
            if t_range is not None:
                bufs["_t_range"] = self._in(t_range, dev)
            self._ready()
            q = L.OrtRayQuery(self._p(bufs["_rays"]), a["n"], self._p(bufs["hits"]),
                              self._p(bufs["normals"]) if a["normals"] else None, int(self._device(dev)), a["use_octree"],
                              L.ORT_QUERY_SORT if a["sort"] else 0, 0)
            if name == "rays":
                check(lib.ort_trace_rays(ctx, C.byref(q), self._s()))
            else:
                qx = L.OrtRayQueryEx(q, self._p(bufs.get("_t_range")), L.QUERY_MODES[name[5:]], (C.c_int32 * 3)(0, 0, 0))
                check(lib.ort_trace_rays_ex(ctx, C.byref(qx), self._s()))
            return None, bufs
        if name == "camera":
            dev = a["device"]
            x0, w, y0, rows, bh, bs = tile = FS.TILES[a["tile"]](*a["size"])
            n = w * rows
            bufs = {k: self._out(m * n, dev) for k, m in (("rays", 24), ("hits", 8), ("normals", 12))}
            self._ready()
            q = L.OrtCameraQuery(*(self._p(bufs[k]) if k in a["want"] else None for k in ("rays", "hits", "normals")),
                                 int(self._device(dev)), L.CAMERA_RAYS[a["which"]])
            p, t = camera_params(a).to_c(), self.ort.Tile(*tile).to_c()
            check(lib.ort_trace_camera(ctx, C.byref(p), C.byref(t), C.byref(q), self._s()))
            return None, bufs
        if name == "radiance":
            dev = a["device"]
            rays, states = radiance_inputs(scene_name, a)
            n = a["n"]
            bufs = {"_rays": self._in(rays, dev), "radiance": self._out(12 * n, dev)}
            st_in = self._out(8 * n, dev)   # the states, with prefilled bytes after them
            if isinstance(st_in, np.ndarray):
                st_in[:8 * n] = _u8(states)
            else:
                with self._on_stream():
                    st_in[:8 * n] = self.torch.from_numpy(_u8(states).copy()).to("cuda:0")
            bufs["_states"] = st_in
            if a["states_out"] == "separate":
                bufs["states_out"] = self._out(8 * n, dev)
            elif a["states_out"] == "equal":
                bufs["states_out"] = st_in
            self._ready()
            flags = ((L.ORT_QUERY_SORT if a["sort"] else 0) | (L.ORT_RADIANCE_NORMALIZE if a["normalize"] else 0) |
                     (L.ORT_RADIANCE_GAMMA if a["gamma"] else 0))
            q = L.OrtRadianceQuery(self._p(bufs["_rays"]), n, self._p(st_in), self._p(bufs["radiance"]),
                                   self._p(bufs.get("states_out")), int(self._device(dev)), a["use_octree"], a["depth"],
                                   a["paths"], flags, 0)
            check(lib.ort_trace_radiance(ctx, C.byref(q), self._s()))
            return None, bufs
        if name in DENOISE:
            code, bufs = self._denoise(a, a["iterations"])
            check(code)
            return None, bufs
        if name in PASSES:
            fs = picture_step(ACC[a["big"]][0], a["output"])
            return None, {"out": self.acc_pass(acc_of(st), a["n"], criterion(a) if name == "pass_adaptive" else None,
                                               FS.describe_output(fs))}
        if name == "read_moments":
            acc = self.accs[a["acc"]]
            bufs = {k: self._out(sizes[k], a["device"]) for k in sizes}
            self._ready()
            m = L.OrtAccumMoments(self._p(bufs.get("mean")), self._p(bufs.get("variance")), int(self._device(a["device"])))
            check(lib.ort_accum_read_moments(ctx, acc._h, C.byref(m), self._s()))
            return None, bufs
        if name == "read_counts":
            bufs = {"counts": self._out(sizes["counts"], a["device"])}
            self._ready()
            check(lib.ort_accum_read_counts(ctx, self.accs["adaptive"]._h, self._p(bufs["counts"]),
                                            int(self._device(a["device"])), self._s()))
            return None, bufs
        if name == "stats":
            self.sync()   # it runs on the context's stream, which waits for no other
            c = criterion(a)
            return None, {"stats": self.accs["adaptive"].adaptive_stats(c[2], c[1], c[3], n=c[0])}
        if name == "refused":
            code, bufs = self._refused(a, state)
            if code == L.ORT_ERR_HIP:
                check(code)
            return code, bufs
        raise AssertionError(name)

    def _denoise(self, a, iterations):
        """(return code, buffers) of ort_denoise / ort_denoise_ex over denoise_inputs(a)."""
        import ctypes as C
        from octreeraytracer_amd import _lib as L
        from octreeraytracer_amd import renderer as R
        dev = a["device"]
        d = denoise_description(a)
        image, t, sph, nrm, var = denoise_inputs(a)
        rows, cols = a["rows"], a["cols"]
        in_stride = (cols + 3 if a["pitched"] else cols) * 12
        src = np.full(rows * in_stride + SLACK, FILL, np.uint8)
        src[:rows * in_stride].reshape(rows, in_stride)[:, :cols * 12] = image.view(np.uint8).reshape(rows, cols * 12)
        color = self._in(src, dev)
        bufs = {"_hits": self._in(denoise_sets.records(t, sph), dev), "_normals": self._in(nrm, dev)}
        bufs["out"] = color if a["inplace"] else self._out(d["nbytes"], dev)
        if not a["inplace"]:
            bufs["_color"] = color
        if var is not None:
            bufs["_variance"] = self._in(var, dev)
        self._ready()
        desc = R._denoise_desc(self._p(color).value, in_stride, self._p(bufs["_hits"]).value, self._p(bufs["_normals"]).value,
                               cols, rows, self._device(dev), iterations, 0.0, 0.0, 5, True)
        o = L.OrtOutput(self._p(bufs["out"]), int(self._device(dev)), L.FORMATS[a["fmt"]], L.ORT_PLACE_TILE, 0, d["pitch"] or 0)
        if var is None:
            return self.r._lib.ort_denoise(self.r._ctx, C.byref(desc), C.byref(o), self._s()), bufs
        x = L.OrtDenoiseDescEx()
        x.base = desc
        if a["gamma"]:
            x.base.flags |= L.ORT_DENOISE_GAMMA
        x.variance, x.sigma_variance = self._p(bufs["_variance"]), SIGMA_VARIANCE
        return self.r._lib.ort_denoise_ex(self.r._ctx, C.byref(x), C.byref(o), self._s()), bufs

    def _refused(self, a, state):
        import ctypes as C
        from octreeraytracer_amd import _lib as L
        lib, ctx, v = self.r._lib, self.r._ctx, a["variant"]
        scene_name = state.scene[0]
        rays, states = ray_source(scene_name, ("set",))
        rays, states, n = rays[:63], states[:63], 63
        if v == "t_range_drawn":
            bufs = {"_rays": self._in(rays, 0), "_t": self._in(intervals(scene_name)[:n], 0), "hits": self._out(8 * n, 0)}
            self._ready()
            q = L.OrtRayQuery(self._p(bufs["_rays"]), n, self._p(bufs["hits"]), None, int(self._device(0)), 1, 0, 0)
            qx = L.OrtRayQueryEx(q, self._p(bufs["_t"]), L.ORT_QUERY_DRAWN, (C.c_int32 * 3)(0, 0, 0))
            return lib.ort_trace_rays_ex(ctx, C.byref(qx), self._s()), bufs
        if v == "normals_without_hits":
            bufs = {"rays": self._out(24 * 48 * 32, 0), "normals": self._out(12 * 48 * 32, 0)}
            self._ready()
            q = L.OrtCameraQuery(self._p(bufs["rays"]), None, self._p(bufs["normals"]), int(self._device(0)), 0)
            p = FS.frame_params((48, 32), (1, 1), 1, a["camera"]).to_c()
            t = self.ort.Tile(0, 48, 0, 32).to_c()
            return lib.ort_trace_camera(ctx, C.byref(p), C.byref(t), C.byref(q), self._s()), bufs
        if v in ("paths_0", "radiance_explicit"):
            bufs = {"_rays": self._in(rays, 0), "_states": self._in(states, 0), "radiance": self._out(12 * n, 0),
                    "states_out": self._out(8 * n, 0)}
            self._ready()
            q = L.OrtRadianceQuery(self._p(bufs["_rays"]), n, self._p(bufs["_states"]), self._p(bufs["radiance"]),
                                   self._p(bufs["states_out"]), int(self._device(0)), 1, 2, 0 if v == "paths_0" else 1, 0, 0)
            return lib.ort_trace_radiance(ctx, C.byref(q), self._s()), bufs
        if v == "iterations_7":
            b = {"device": 0, "cols": 37, "rows": 8, "fmt": "rgb32f", "pitched": 0, "inplace": 0, "img": 0, "gflip": 0}
            return self._denoise(b, 7)
        if v == "variance_plain":
            (W, H), _, _ = ACC[a["big"]]
            bufs = {"mean": self._out(12 * W * H, 0), "variance": self._out(4 * W * H, 0)}
            self._ready()
            m = L.OrtAccumMoments(self._p(bufs["mean"]), self._p(bufs["variance"]), int(self._device(0)))
            return lib.ort_accum_read_moments(ctx, self.accs["plain"]._h, C.byref(m), self._s()), bufs
        if v == "adaptive_on_plain":
            d = FS.describe_output(picture_step(ACC[a["big"]][0], "pitch_f32"))
            buf = self._out(d["nbytes"], 1)
            self._ready()
            c = self.accs["plain"]._criterion(2, 0.1, 1, FLOOR)
            o = L.OrtOutput(self._p(buf), 1, L.ORT_FORMAT_RGB32F, L.ORT_PLACE_TILE, 0, d["pitch"])
            return lib.ort_accum_render_adaptive(ctx, self.accs["plain"]._h, C.byref(c), C.byref(o), self._s()), {"out": buf}
        if v == "begin_explicit":
            self.sync()
            p = FS.frame_params((48, 32), (4, 2), 1, a["camera"]).to_c()
            t = self.ort.Tile(0, 48, 0, 32).to_c()
            h = C.c_void_p()
            code = lib.ort_accum_begin(ctx, C.byref(p), C.byref(t), C.byref(h))
            if code == 0:
                lib.ort_accum_free(ctx, h)
            return code, {}
        raise AssertionError(v)


def replay(seed, first=0, last=None, stream=False, batch=None):
    """Run steps first..last of sequence `seed` on a fresh context (a slice begins with the upload
    its first step implies).  Raises Mismatch, or returns the number of steps run."""
    import octreeraytracer_amd as ort
    steps = plan()[seed][first:None if last is None else last + 1]
    with GpuAdapter(ort, stream=stream or None) as ad:
        run(ad, steps, seed, first, batch or (FS.BATCH if stream else 1))
    return len(steps)
