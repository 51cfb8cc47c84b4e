"""Sequences of frames on one context: the plan and the runner (tests/test_frame_sequences.py on
the host, tests/test_gpu_frame_sequences.py on the GPU).

A context carries state from one frame to the next -- the alternating counter sets, the queued
heavy list, the last camera, the per-slot walk steps, the list-length hints, the whole-pixel class
lists, the speculation buffers, the timing slots, a dozen grow-only buffers -- and render_impl /
render_pixel_paths pick each frame's route from it.  Most of it is keyed by frame_sig, which holds
sizes and counts only.  The rest of the suite renders almost always on a fresh upload; here one
context is taken through every route after every other.

The plan is a seeded, deterministic walk made of

  chains    for every kind or action A and every other X the sandwich (A, X, A): A, X1, A, X2, A, ...
            Both A of a sandwich have the same params, tile, output and options (one signature), X
            draws its own.  Every ordered pair of routes follows from the sandwiches.
  variants  for every stateful kind K the sandwiches (K, X, K) with X = K under a turned camera,
            the upload of the twin scene, K with one option changed that the signature does not
            hold (and the camera turned, so that the frame differs), and K on a larger tile.
  tours     every kind and action in shuffled order on the 181,769-node tree and on a tree of
            depth 9 (the chains and variants run on the 105-node tree).

cut into sequences of at most MAX_STEPS steps, each run on a fresh context and named by its seed.
The generator rejects a draw whose picture equals the picture of the step before it (or the one
after it) over the same output shape, so a stale frame is always visible.

Every reference is the oracle's: oracle.render for frames and previews, its counters for
count_traffic, oracle.trace_rays for queries (cached per arguments, read-only).

run(adapter, steps) drives an adapter -- GpuAdapter over a Renderer, or the test's fake over the
host emulation -- and compares every byte of every output buffer: the pixels' bits, RGBA8 as
image.to_srgb8 with alpha 255, zero words in padding rows, the prefill everywhere else (between
pitched rows, around a tile placed into a frame, after the last row).  replay(seed, first, last)
runs a slice of a sequence on a fresh context from a Python prompt, to shorten a failing sequence
by hand (a mismatch only: a HIP error is read from the code, not run again)."""
import dataclasses
import functools
import random

import numpy as np

import chart_scenes as CS
import ray_sets

FILL = 0xA5
SLACK = 64       # prefilled bytes after the last described one
MAX_STEPS = 250
BATCH = 6        # steps in flight on a caller's stream
BASE_SEED = 20260

# ---- scenes -----------------------------------------------------------------------------------------
SCENES = {"d4": (4, 1), "d6": (6, 0), "deep": (9, 1)}  # the chart under build_octree(depth, m)
SIZES = ((48, 32), (97, 63))
CAMERAS = {"chart": {}, "turned": {"yaw": CS.YAW + 0.5}, "sky": {"pitch": -89.0}}
TILES = {
    "full": lambda W, H: (0, W, 0, H, 0, 0),
    "band": lambda W, H: (0, W, 16, 48, 16, 32),   # rows 16-31, 48-63, 80-95: padding rows past the frame
    "sub": lambda W, H: (13, W - 30, 5, 23, 0, 0),
    "pixel": lambda W, H: (W - 1, 1, H - 1, 1, 0, 0),
    "none": lambda W, H: (0, W, 0, 0, 0, 0),
}
OUTPUTS = ("host_f32", "host_rgba8", "pitch_f32", "pitch_rgba8", "frame_f32", "frame_rgba8")
BPP = {"rgb32f": 12, "rgba8": 4}

# ort_set_option by name; the defaults of ort_create
OPTION_DEFAULTS = {
    "exact_traversal": 0, "refill": 16, "persistent": 2, "sort_paths": 2, "xcd_swizzle": -1, "kid_skip": 1,
    "sort_bound": 0, "cost_order": 1, "heavy_first": 64, "heavy_prio": 150, "split_heavy": -1, "split_level": 0,
    "tile_pairs": -1, "launch_times": 1, "pixel_paths": -1, "pixel_lds_scene": 1, "pixel_heavy_first": -1,
    "pixel_speculate": -1,
}
# drawn per frame: the same pixels under every value
MISC = {
    "kid_skip": (0, 1, 2), "exact_traversal": (0, 1), "refill": (1, 16, 64), "xcd_swizzle": (-1, 0, 1, 2),
    "launch_times": (0, 1), "pixel_lds_scene": (0, 1), "pixel_heavy_first": (-1, 0, 1), "sort_bound": (0, 1, 1000),
}


@dataclasses.dataclass(frozen=True)
class Kind:
    """A frame recipe: the options that force its route, the (samples, bounces) it draws from."""
    shapes: tuple
    options: tuple = ()
    explicit: bool = False
    use_octree: int = 1
    size: tuple = None
    changed: tuple = ()   # the options, one per variant, that its "option" variants change


PIPE = (("pixel_paths", 0),)
KINDS = {
    "direct": Kind(((1, 1),), changed=(("cost_order", 0), ("split_heavy", 0))),  # (split 0: auto tile pairs)
    "direct_split": Kind(((1, 1),), (("split_heavy", 20),), changed=(("split_level", 2),)),
    "direct_pairs": Kind(((1, 1),), (("tile_pairs", 1),), changed=(("split_heavy", 0),)),
    "direct_plain": Kind(((1, 1),), (("cost_order", 0), ("tile_pairs", 0), ("split_heavy", 0)),
                         changed=(("cost_order", 1),)),
    "pipe_list": Kind(((1, 3), (2, 4)), PIPE + (("sort_paths", 2), ("persistent", 2), ("heavy_first", 8)),
                      changed=(("heavy_first", 0),)),
    "pipe_slots": Kind(((1, 3), (2, 4)), PIPE + (("sort_paths", 1),), changed=(("sort_paths", 2),)),
    "pipe_unsorted": Kind(((1, 3), (2, 4)), PIPE + (("sort_paths", 0), ("persistent", 0)), changed=(("persistent", 2),)),
    # more than 64 hint indices, 16 timed launches and 8 recorded bounces in one frame
    "pipe_long": Kind(((9, 8),), PIPE, size=(48, 32), changed=(("kid_skip", 0),)),
    "pixel": Kind(((2, 4),), (("pixel_paths", 1), ("pixel_speculate", 0)), changed=(("kid_skip", 0),)),
    "pixel_spec": Kind(((8, 6),), (("pixel_paths", 1), ("pixel_speculate", 1)), changed=(("kid_skip", 2),)),
    "brute_direct": Kind(((1, 1),), use_octree=0, changed=(("cost_order", 0),)),
    "brute_pipe": Kind(((2, 3),), PIPE, use_octree=0, changed=(("sort_paths", 0),)),
    "brute_pixel": Kind(((2, 4),), (("pixel_paths", 1),), use_octree=0, changed=(("pixel_speculate", 0),)),
    "explicit_direct": Kind(((1, 1),), explicit=True, changed=(("kid_skip", 0),)),
    "explicit_pipe": Kind(((2, 4),), explicit=True, changed=(("sort_paths", 0),)),
    "no_bounce": Kind(((3, 0),)),
}
STATEFUL = tuple(k for k in KINDS if k != "no_bounce")
ACTIONS = ("count", "query", "accum", "reupload", "twin", "build")
NAMES = tuple(KINDS) + ACTIONS
VARIANTS = ("camera", "twin", "option", "larger")

ACC_SIZE, ACC_N, ACC_DEPTH = (48, 32), 7, 3   # the accumulation kept open through a sequence
N_QUERY_RAYS = 129


@dataclasses.dataclass(frozen=True)
class Step:
    name: str                  # a kind or an action
    scene: str = "d4"
    size: tuple = (48, 32)
    shape: tuple = (1, 1)      # (num_samples, max_depth)
    use_octree: int = 1
    camera: str = "chart"
    tile: str = "full"
    output: str = "host_f32"
    options: tuple = ()        # (name, value), sorted: what differs from OPTION_DEFAULTS
    sort: bool = False         # query: ORT_QUERY_SORT
    n: int = 0                 # accum: the samples of the pass
    tag: str = ""              # which part of the plan the step belongs to

    @property
    def is_frame(self):
        return self.name in KINDS

    def recipe(self):
        """What the two A of a sandwich share."""
        return dataclasses.replace(self, tag="")


def isqrt(k):
    return int(np.sqrt(np.float32(k)))


def twin_of(s):
    """The same spheres and tree, materials and fuzz/ri dealt to other spheres: one signature."""
    import octreeraytracer_amd as ort
    perm = np.random.default_rng(7).permutation(s.n)
    return ort.SphereSet(s.center_radius.copy(), s.mat_albedo[perm].copy(), s.fuzz_ri[perm].copy())


@functools.lru_cache(maxsize=None)
def scene(name, twin=False):
    s, t = CS.scene(*SCENES[name])
    if twin:
        s = twin_of(s)
        for a in (s.center_radius, s.mat_albedo, s.fuzz_ri):
            a.setflags(write=False)
    return s, t


def tree_depth(t):
    """The deepest node level (root = 0), as ort_scene_info.tree_depth."""
    level, nodes = 0, np.array([0])
    while True:
        first = t.children_offset[nodes]
        first = first[first >= 0]
        if not len(first):
            return level
        nodes = (first[:, None] + np.arange(8)[None, :]).reshape(-1)
        level += 1


def frame_params(size, shape, use_octree, camera):
    import octreeraytracer_amd as ort
    return CS.chart_params(ort, size[0], size[1], num_samples=shape[0], max_depth=shape[1], use_octree=use_octree,
                           **CAMERAS[camera])


def tile_of(step):
    return TILES[step.tile](*step.size)


def pixel_rows(tile):
    x0, w, y0, rows, bh, bs = tile
    j = np.arange(rows)
    return y0 + (j // bh) * bs + j % bh if bh > 0 else y0 + j


# ---- references: the oracle's, computed once ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame_reference(scene_name, twin, camera, size, shape, use_octree, tile):
    """(rows, width, 3) float32 of the tile: oracle.render; padding rows zero."""
    from oracle import oracle
    s, t = scene(scene_name, twin)
    x0, w, y0, rows, bh, bs = tile
    if w * rows == 0:
        img = np.zeros((rows, w, 3), np.float32)
    else:
        img = oracle.render(s, t if use_octree else None, frame_params(size, shape, use_octree, camera), x0, y0, w, rows,
                            bh, bs)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def count_reference(scene_name, twin, camera, size, shape, use_octree, tile):
    from oracle import oracle
    s, t = scene(scene_name, twin)
    x0, w, y0, rows, bh, bs = tile
    if w * rows == 0:  # nothing is launched: every counter is zero
        return dict.fromkeys(oracle.COUNT_NAMES, 0)
    _, counts = oracle.render(s, t if use_octree else None, frame_params(size, shape, use_octree, camera), x0, y0, w,
                              rows, bh, bs, counts=True)
    return counts


@functools.lru_cache(maxsize=None)
def query_rays(scene_name):
    """129 rays of ray_sets' generator for the scene (read-only): 64 spread over its first five
    classes and 65 of its last, which start on the spheres' surfaces and so reach many of them."""
    import octreeraytracer_amd as ort
    from oracle import oracle
    s, t = scene(scene_name)
    rays = ray_sets.make_rays(ort, oracle, s, t, 1000 + SCENES[scene_name][0])
    n_surface = dict(ray_sets.CLASSES)["surface"]
    rays = np.ascontiguousarray(np.concatenate([rays[:-n_surface][::46][:64], rays[-n_surface:][:65]]))
    assert rays.shape == (N_QUERY_RAYS, 6)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def query_reference(scene_name):
    """The oracle's records {hit, t bits} of query_rays through the tree, (n, 2) int32, and through
    the one-sphere scene of every sphere, (spheres, n, 2): brute force is the smallest t among
    those, the lowest index attaining it (the shader's test is a strict <)."""
    import octreeraytracer_amd as ort
    from oracle import oracle
    s, t = scene(scene_name)
    rays = query_rays(scene_name)
    tree = oracle.trace_rays(s, t, rays)
    each = np.stack([oracle.trace_rays(*ray_sets.one_sphere_scene(ort, s, k), rays) for k in range(s.n)])
    for a in (tree, each):
        a.setflags(write=False)
    return tree, each


# ---- the state a sequence carries: shared by the generator and the runner ------------------------------
class State:
    """Which scene is uploaded and where the open accumulation stands.  advance(step) returns what
    the step implies before its own call: {"upload": (scene, twin, explicit, how) or None,
    "begin" / "restart": bool (accum)}, and moves on."""

    def __init__(self):
        self.scene = None      # (name, twin, explicit)
        self.acc = None        # {"camera", "done", "valid"}

    def copy(self):
        c = State()
        c.scene, c.acc = self.scene, dict(self.acc) if self.acc else None
        return c

    def advance(self, st):
        twin = self.scene[1] if self.scene else False
        do = {"upload": None, "begin": False, "restart": False}
        if st.is_frame:
            want, how = (st.scene, twin, KINDS[st.name].explicit), "upload"
        elif st.name in ("count", "query"):
            want, how = self.scene or (st.scene, False, False), "upload"
        elif st.name == "twin":
            want, how = (st.scene, not twin, False), "upload"
        else:  # accum, reupload, build: the compact layout
            want, how = (st.scene, twin, False), "build" if st.name == "build" else "upload"
        if want != self.scene or st.name in ("reupload", "twin", "build"):
            do["upload"] = want + (how,)
            self.scene = want
            if self.acc:
                self.acc["valid"] = False
        if st.name == "accum":
            if self.acc is None:
                do["begin"] = True
                self.acc = {"camera": st.camera, "done": 0, "valid": True}
            elif not self.acc["valid"] or self.acc["done"] >= ACC_N:
                do["restart"] = True
                self.acc = {"camera": st.camera, "done": 0, "valid": True}
            self.acc["done"] += min(st.n, ACC_N - self.acc["done"])
        return do

    def picture(self, st):
        """After advance(st): the float picture the step must write, or None (no picture, no
        pixels, or a preview that no frame equals)."""
        name, twin, _ = self.scene
        if st.is_frame:
            ref = frame_reference(name, twin, st.camera, st.size, st.shape, st.use_octree, tile_of(st))
            return ref if ref.size else None
        if st.name == "accum" and isqrt(self.acc["done"]) == isqrt(ACC_N):
            return frame_reference(name, twin, self.acc["camera"], ACC_SIZE, (self.acc["done"], ACC_DEPTH), 1,
                                   TILES["full"](*ACC_SIZE))
        return None


def differs(a, b):
    return a is None or b is None or a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the generator ----------------------------------------------------------------------------------
def _options(kind, misc, changed=()):
    o = dict(misc)
    o.update(KINDS[kind].options)
    o.update(changed)
    return tuple(sorted((k, v) for k, v in o.items() if OPTION_DEFAULTS[k] != v))


def _draw(rng, name, scene_name, tiles=tuple(TILES), cameras=tuple(CAMERAS), tag=""):
    """A step of the kind or action `name`, its free dimensions drawn."""
    misc = {k: rng.choice(v) for k, v in MISC.items()}
    if name in KINDS:
        k = KINDS[name]
        return Step(name, scene_name, k.size or rng.choice(SIZES), rng.choice(k.shapes), k.use_octree, rng.choice(cameras),
                    rng.choice(tiles), rng.choice(OUTPUTS), _options(name, misc), tag=tag)
    opts = tuple(sorted((k, v) for k, v in misc.items() if OPTION_DEFAULTS[k] != v))
    if name == "count":
        return Step(name, scene_name, rng.choice(SIZES), rng.choice(((1, 1), (2, 3))), rng.choice((1, 1, 0)),
                    rng.choice(cameras), rng.choice(tiles), options=opts, tag=tag)
    if name == "query":
        return Step(name, scene_name, use_octree=rng.choice((1, 1, 0)), options=opts, sort=rng.choice((False, True)), tag=tag)
    if name == "accum":
        return Step(name, scene_name, ACC_SIZE, (ACC_N, ACC_DEPTH), 1, rng.choice(("chart", "turned")), "full",
                    rng.choice(OUTPUTS[:2]), opts, n=rng.choice((2, 3, 4)), tag=tag)
    return Step(name, scene_name, tag=tag)


class _Walk:
    """One sequence being written: its steps, its state, the picture of its last step."""

    def __init__(self, rng):
        self.rng, self.steps, self.state, self.last = rng, [], State(), None

    def add(self, st):
        self.state.advance(st)
        self.last = self.state.picture(st)
        self.steps.append(st)

    def fits(self, make, then=None, tries=400):
        """A step by make() whose picture differs from the last step's and, where `then` (the
        step that follows) is given, from that one's too."""
        for _ in range(tries):
            st = make()
            state = self.state.copy()
            state.advance(st)
            pic = state.picture(st)
            if not differs(self.last, pic):
                continue
            if then is not None:
                state.advance(then)
                if not differs(pic, state.picture(then)):
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
    a = w.fits(lambda: _draw(rng, a_name, scene_name, tiles=("full", "band", "sub"), tag=tag))
    if a_name == "accum":  # (two passes to the finished frame: most X that upload a scene still leave some to finish)
        a = dataclasses.replace(a, n=4)
    w.add(a)
    for x in others:
        w.sandwich(a, lambda: _draw(rng, x, scene_name, tag=tag))


def _variants(w, kind, scene_name):
    rng = w.rng
    k = KINDS[kind]
    for v in VARIANTS:
        for changed in (k.changed if v == "option" else ((),)):
            tag = f"variant:{v}:{kind}"
            small = v == "larger" or k.size is not None

            def make_a():
                while True:
                    a = _draw(rng, kind, scene_name, tiles=("sub",) if v == "larger" else ("full", "band", "sub"),
                              cameras=("chart",), tag=tag)
                    if not changed or dict(OPTION_DEFAULTS, **dict(a.options))[changed[0]] != changed[1]:
                        return dataclasses.replace(a, size=(48, 32)) if small else a

            a = w.fits(make_a, tries=40)
            if a is None:  # every A of this variant repeats the picture before it: another frame in between
                w.add(w.fits(lambda: _draw(rng, "no_bounce", scene_name, tiles=("full", "band", "sub"), tag=tag)))
                a = w.fits(make_a)
            w.add(a)
            if v == "camera":
                x = dataclasses.replace(a, camera="turned")
            elif v == "twin":
                x = Step("twin", scene_name, tag=tag)
            elif v == "option":
                o = dict(a.options)
                o[changed[0]] = changed[1]
                x = dataclasses.replace(a, camera="turned",
                                        options=tuple(sorted((n, val) for n, val in o.items() if OPTION_DEFAULTS[n] != val)))
            else:  # the grow-only buffers are freed and allocated again
                x = dataclasses.replace(a, size=(97, 63) if k.size is None else k.size, tile="full")
            w.sandwich(a, lambda: x)


def _tour(w, scene_name):
    rng = w.rng
    for rep in range(3):
        names = list(NAMES)
        rng.shuffle(names)
        for n in names:
            w.add(w.fits(lambda: _draw(rng, n, scene_name, tag=f"tour:{scene_name}")))


@functools.lru_cache(maxsize=None)
def plan():
    """{seed: tuple of steps}: every sequence of the plan, the same on every call."""
    parts = [("chain", n, "d4") for n in NAMES] + [("variants", k, "d4") for k in STATEFUL]
    seqs, w = {}, None

    def close():
        if w is not None and w.steps:
            seqs[BASE_SEED + len(seqs)] = tuple(w.steps)

    for what, name, scene_name in parts:
        need = 2 * len(NAMES) - 1 if what == "chain" else 4 * (len(VARIANTS) - 1 + len(KINDS[name].changed))
        if w is None or len(w.steps) + need > MAX_STEPS:
            close()
            w = _Walk(random.Random(BASE_SEED + len(seqs)))
        (_chain if what == "chain" else _variants)(w, name, scene_name)
    close()
    for scene_name in ("d6", "deep"):
        w = _Walk(random.Random(BASE_SEED + len(seqs)))
        _tour(w, scene_name)
        close()
    return seqs


def seeds():
    return tuple(plan())


# Sequences that once failed, cut down by hand: name -> steps.
REGRESSIONS = {
    # ort_count_traffic cleared its counters on the context's stream and, for a tile of no pixels,
    # copied them back without waiting for that stream: the counters of the count before it.  (Seen
    # with a second context busy on the device; found by seed 20263, step 111, two contexts in turn.)
    "count_of_no_pixels_after_a_count": (
        Step("count", "d4", (97, 63), (2, 3), 1, "chart", "sub"),
        Step("count", "d4", (97, 63), (1, 1), 1, "turned", "none"),
        Step("count", "d4", (48, 32), (1, 1), 1, "chart", "full"),
        Step("count", "d4", (48, 32), (2, 3), 0, "sky", "none"),
        Step("direct", "d4", (48, 32), (1, 1), 1, "chart", "band", "pitch_rgba8"),
    ),
}


def totals():
    """(sequences, steps, distinct reference frames) of the plan."""
    frames = set()
    for steps in plan().values():
        state = State()
        for st in steps:
            state.advance(st)
            pic = state.picture(st)
            if pic is not None:
                frames.add(pic.tobytes())
    return len(plan()), sum(len(s) for s in plan().values()), len(frames)


# ---- the runner -------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    def __init__(self, seed, index, text):
        super().__init__(text)
        self.seed, self.index = seed, index


def describe_output(st):
    """How the step's picture is written: {"fmt", "place", "device", "pitch" (None: tight),
    "row_bytes", "stride" (bytes from row to row), "rows" (of the buffer), "nbytes"}."""
    W, H = st.size
    x0, w, y0, rows, bh, bs = tile_of(st)
    form, fmt = st.output.split("_")
    fmt = "rgb32f" if fmt == "f32" else "rgba8"
    bpp = BPP[fmt]
    d = {"fmt": fmt, "place": "frame" if form == "frame" else "tile", "device": form != "host", "pitch": None}
    if form == "frame":
        d.update(row_bytes=W * bpp, stride=W * bpp, rows=H)
    else:
        d.update(row_bytes=w * bpp, stride=w * bpp, rows=rows)
        if form == "pitch":
            d.update(pitch=(w + 3) * bpp, stride=(w + 3) * bpp)
    d["nbytes"] = d["rows"] * d["stride"]
    return d


def pixel_bytes(ref, fmt, padding):
    """(rows, width * bpp) uint8 of the float picture in fmt; padding rows are zero words."""
    from octreeraytracer_amd.image import to_srgb8
    rows, w = ref.shape[:2]
    if fmt == "rgb32f":
        px = np.ascontiguousarray(ref).view(np.uint8).reshape(rows, w * 12).copy()
    else:
        px = np.full((rows, w, 4), 255, np.uint8)
        px[..., :3] = to_srgb8(ref)
        px = px.reshape(rows, w * 4)
    px[padding] = 0
    return px


def expected_buffer(st, ref, d):
    """The whole buffer after the step: FILL but for the pixels the description covers."""
    W, H = st.size
    x0, w, y0, rows, bh, bs = tile_of(st)
    want = np.full(d["nbytes"] + SLACK, FILL, np.uint8)
    if w * rows == 0:
        return want
    ys = pixel_rows((x0, w, y0, rows, bh, bs))
    px = pixel_bytes(ref, d["fmt"], ys >= H)
    grid = want[:d["nbytes"]].reshape(d["rows"], d["stride"])
    if d["place"] == "tile":
        grid[:, :d["row_bytes"]] = px
    else:
        at = x0 * BPP[d["fmt"]]
        grid[ys[ys < H], at:at + px.shape[1]] = px[ys < H]
    return want


def first_differences(got, want, d, limit=5):
    bad = np.nonzero(got != want)[0]
    bpp = BPP[d["fmt"]]
    out, seen = [], set()
    for off in bad:
        off = int(off)
        row, col = (off // d["stride"], (off % d["stride"]) // bpp) if off < d["nbytes"] else (-1, -1)
        if (row, col) in seen:
            continue
        seen.add((row, col))
        at = off - off % 4 if row < 0 else row * d["stride"] + col * bpp
        where = "after the last row" if row < 0 else ("between rows" if col * bpp >= d["row_bytes"] else "")
        out.append(f"buffer row {row} column {col} {where}: got {got[at:at + bpp].tobytes().hex()} "
                   f"want {want[at:at + bpp].tobytes().hex()}")
        if len(out) == limit:
            break
    return f"{len(bad)} bytes differ; " + "; ".join(out)


class Runner:
    """Runs steps on an adapter and checks every result; `batch` steps are issued before their
    results are read (1: each step is checked before the next starts).  steps() is a generator
    that yields after each step, so that two runners can take turns."""

    def __init__(self, adapter, steps, seed=None, first=0, batch=1):
        self.adapter, self.all, self.seed, self.first, self.batch = adapter, tuple(steps), seed, first, batch
        self.state, self.set, self.pending, self.zero_before = State(), {}, [], False

    def fail(self, index, state, text):
        i = index - self.first
        before = "\n".join(f"    {self.first + j}: {self.all[j]}" for j in range(max(0, i - 8), i))
        raise Mismatch(self.seed, index, f"seed {self.seed}, step {index}: {text}\n  step: {self.all[i]}\n"
                       f"  scene (name, twin, explicit): {state.scene}; accumulation: {state.acc}\n"
                       f"  the steps before it:\n{before}\n"
                       f"  frame_sequences.replay({self.seed}, first, {index}) runs a slice again")

    def steps(self):
        try:
            for i, st in enumerate(self.all):
                self.adapter.step_index = self.first + i
                self.issue(self.first + i, st)
                if len(self.pending) >= self.batch:
                    self.collect()
                yield self.first + i
            self.collect()
        except Exception as e:  # a HIP error ends the session: nothing more may start on the GPU
            from octreeraytracer_amd import _lib as L
            if getattr(e, "code", None) == L.ORT_ERR_HIP:
                import pytest
                pytest.exit(f"ORT_ERR_HIP in seed {self.seed} at step {self.adapter.step_index}: {e}\n"
                            f"  step: {self.all[self.adapter.step_index - self.first]}\n"
                            "  read the cause from the code; do not run it again", returncode=3)
            raise

    def run(self):
        for _ in self.steps():
            pass

    def issue(self, index, st):
        ad = self.adapter
        opts = dict(OPTION_DEFAULTS)
        opts.update(st.options)
        for k, v in opts.items():
            if self.set.get(k) != v:
                ad.set_option(k, v)
                self.set[k] = v
        do = self.state.advance(st)
        state = self.state.copy()
        if do["upload"]:
            name, twin, explicit, how = do["upload"]
            s, t = scene(name, twin)
            ad.set_option("force_layout", 1 if explicit else 0)
            if how == "build":
                ad.upload(s, None, build=SCENES[name])
            else:
                ad.upload(s, t)
        name, twin, _ = state.scene
        if st.is_frame:
            d = describe_output(st)
            x0, w, y0, rows, bh, bs = tile_of(st)
            ref = frame_reference(name, twin, st.camera, st.size, st.shape, st.use_octree, tile_of(st))
            h = ad.render(frame_params(st.size, st.shape, st.use_octree, st.camera), tile_of(st), d)
            self.pending.append((index, st, state, "frame", h, (ref, d)))
        elif st.name == "count":
            got = ad.count(frame_params(st.size, st.shape, st.use_octree, st.camera), tile_of(st))
            want = count_reference(name, twin, st.camera, st.size, st.shape, st.use_octree, tile_of(st))
            self.pending.append((index, st, state, "count", None, (got, want)))
        elif st.name == "query":
            h = ad.query(query_rays(name), bool(st.use_octree), st.sort)
            self.pending.append((index, st, state, "query", h, name))
        elif st.name == "accum":
            p = frame_params(ACC_SIZE, (ACC_N, ACC_DEPTH), 1, state.acc["camera"])
            if do["begin"]:
                ad.accum("begin", p, TILES["full"](*ACC_SIZE))
            elif do["restart"]:
                ad.accum("restart", p)
            d = describe_output(st)
            h = ad.accum("step", st.n, d)
            self.pending.append((index, st, state, "accum", h, (state.picture(st), d)))

    def collect(self):
        if not self.pending:
            return
        self.adapter.sync()
        pending, self.pending = self.pending, []
        for index, st, state, what, h, ref in pending:
            if what in ("frame", "accum"):
                pic, d = ref
                got = self.adapter.read(h)
                if what == "accum" and pic is None:
                    continue  # a preview with other strata than any frame's
                if got is None:  # no pixels and no buffer: the call returned ORT_OK
                    assert tile_of(st)[1] * tile_of(st)[3] == 0
                    continue
                want = expected_buffer(st, pic, d)
                if got.shape != want.shape or not np.array_equal(got, want):
                    self.fail(index, state, f"the {d['fmt']} picture ({st.output}) is not the oracle's: "
                              + first_differences(got, want, d))
            elif what == "count":
                got, want = ref
                if got != want:
                    self.fail(index, state, f"count_traffic {got} is not the oracle's {want}")
            elif what == "query":
                rec = self.adapter.read(h)
                text = check_query(rec, ref, bool(st.use_octree))
                if text:
                    self.fail(index, state, text)


def check_query(rec, scene_name, use_octree):
    """'' or what is wrong with the (n, 2) int32 records {t bits, sphere}."""
    tree, each = query_reference(scene_name)
    n = len(tree)
    if rec.shape != (n, 2):
        return f"query records of shape {rec.shape}"
    t_bits, sphere = rec[:, 0], rec[:, 1]
    if use_octree:
        hit, want_bits = tree[:, 0] == 1, np.where(tree[:, 0] == 1, tree[:, 1], 0)
    else:
        t_each = np.where(each[:, :, 0] == 1, each[:, :, 1].view(np.float32), np.inf)
        best = t_each.argmin(axis=0)  # (the first index among equals)
        hit = np.isfinite(t_each[best, np.arange(n)])
        want_bits = np.where(hit, each[best, np.arange(n), 1], 0)
        bad = np.nonzero(hit & (sphere != best))[0]
        if len(bad):
            return f"query: rays {bad[:5].tolist()} report spheres {sphere[bad[:5]].tolist()}, brute force {best[bad[:5]].tolist()}"
    bad = np.nonzero((t_bits != want_bits) | ((sphere >= 0) != hit))[0]
    if len(bad):
        return (f"query: {len(bad)} records are not the oracle's, first rays {bad[:5].tolist()}: t bits "
                f"{t_bits[bad[:5]].tolist()} want {want_bits[bad[:5]].tolist()}, sphere {sphere[bad[:5]].tolist()}")
    if (sphere[hit] >= each.shape[0]).any() or (sphere[~hit] != -1).any():
        return "query: sphere indices out of range"
    alone = each[sphere[hit], np.nonzero(hit)[0]]  # the reported sphere, traced alone, is hit at the same t
    bad = np.nonzero(hit)[0][(alone[:, 0] != 1) | (alone[:, 1] != t_bits[hit])]
    if len(bad):
        return f"query: rays {bad[:5].tolist()} report spheres {sphere[bad[:5]].tolist()} that they do not hit at that t"
    return ""


def run(adapter, steps, seed=None, first=0, batch=1):
    Runner(adapter, steps, seed, first, batch).run()


def run_in_turn(runners):
    """The runners' steps, one of each in turn, until all are through."""
    its = [r.steps() for r in runners]
    while its:
        for it in list(its):
            if next(it, None) is None:
                its.remove(it)


# ---- the adapter over a Renderer ---------------------------------------------------------------------
OPTION_IDS = {
    "force_layout": 1, "exact_traversal": 2, "refill": 3, "persistent": 4, "sort_paths": 6, "xcd_swizzle": 8, "kid_skip": 9,
    "sort_bound": 10, "cost_order": 11, "heavy_first": 12, "heavy_prio": 13, "split_heavy": 14, "split_level": 15,
    "tile_pairs": 16, "launch_times": 19, "pixel_paths": 20, "pixel_lds_scene": 21, "pixel_heavy_first": 22,
    "pixel_speculate": 23,
}


class GpuAdapter:
    """A Renderer on device 0.  stream=None: every call on the context's own stream, synchronous.
    stream=True: every frame, pass and query on one torch.cuda.Stream, host pictures turned into
    tight device buffers, nothing waited for until sync().  (Uploads and count_traffic are not
    stream-ordered calls: the adapter waits for the stream before them.)"""

    def __init__(self, ort, stream=None):
        import torch
        self.ort, self.torch = ort, torch
        self.r = ort.Renderer(0)
        self.stream = torch.cuda.Stream(device=0) if stream else None
        self.acc = None
        self.step_index = -1

    def close(self):
        self.sync()
        if self.acc is not None:
            self.acc.close()
            self.acc = None
        self.r.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        if self.stream is not None:
            self.stream.synchronize()

    def _handle(self):
        return self.stream.cuda_stream if self.stream is not None else None

    def set_option(self, name, value):
        self.r._check(self.r._lib.ort_set_option(self.r._ctx, OPTION_IDS[name], int(value)))

    def upload(self, spheres, tree, build=None):
        self.sync()
        if build:
            self.r.build_scene(spheres, *build)
        else:
            self.r.upload(spheres, tree)

    def count(self, params, tile):
        self.sync()
        return self.r.count_traffic(params, self.ort.Tile(*tile))

    def _buffer(self, d, pixels):
        """The prefilled buffer of a description and the `out` to pass; (None, None) for a host
        picture of no pixels (a NULL output is accepted)."""
        torch = self.torch
        n = d["nbytes"] + SLACK
        if not d["device"] and not pixels:
            return None, None
        if d["device"] or self.stream is not None:
            if self.stream is not None:
                with torch.cuda.stream(self.stream):
                    buf = torch.full((n,), FILL, dtype=torch.uint8, device="cuda:0")
            else:
                buf = torch.full((n,), FILL, dtype=torch.uint8, device="cuda:0")
                torch.cuda.current_stream().synchronize()  # the context's stream does not wait for torch's
            return buf, buf.view(torch.float32) if d["fmt"] == "rgb32f" else buf
        buf = np.full(n, FILL, np.uint8)
        return buf, buf.view(np.float32) if d["fmt"] == "rgb32f" else buf

    def render(self, params, tile, d):
        import ctypes as C
        from octreeraytracer_amd import _lib as L
        buf, out = self._buffer(d, tile[1] * tile[3])
        if buf is None:
            p, t = params.to_c(), self.ort.Tile(*tile).to_c()
            o = L.OrtOutput(None, 0, L.FORMATS[d["fmt"]], L.PLACEMENTS[d["place"]], 0, 0)
            s = C.c_void_p(self._handle()) if self._handle() else None
            self.r._check(self.r._lib.ort_render_ex(self.r._ctx, C.byref(p), C.byref(t), C.byref(o), s))
            return None
        self.r.render(params, self.ort.Tile(*tile), out=out, stream=self._handle(), format=d["fmt"], row_pitch=d["pitch"],
                      place=d["place"])
        return buf

    def accum(self, what, *args):
        if what == "begin":
            params, tile = args
            self.acc = self.r.accumulate(params, self.ort.Tile(*tile))
        elif what == "restart":
            self.acc.restart(args[0])
        else:
            n, d = args
            buf, out = self._buffer(d, 1)
            self.acc.step(n, out=out, stream=self._handle(), format=d["fmt"], row_pitch=d["pitch"], place=d["place"])
            return buf

    def query(self, rays, use_octree, sort):
        torch = self.torch
        if self.stream is None:
            t, sphere = self.r.trace_rays(np.ascontiguousarray(rays), use_octree=use_octree, sort=sort)
            return np.stack([t.view(np.int32), sphere], axis=1)
        with torch.cuda.stream(self.stream):
            dev = torch.from_numpy(np.array(rays)).to("cuda:0")
            out = torch.full((len(rays), 2), -7, dtype=torch.int32, device="cuda:0")
        self.r.trace_rays(dev, use_octree=use_octree, sort=sort, out=out, stream=self._handle())
        return dev, out

    def read(self, h):
        if h is None or isinstance(h, np.ndarray):
            return h
        if isinstance(h, tuple):
            return h[1].cpu().numpy()
        return h.cpu().numpy()


def replay(seed, first=0, last=None, stream=False, batch=None):
    """Run steps first..last of sequence `seed` on a fresh context (a slice begins with the upload
    its first step implies).  Raises Mismatch, or returns the number of steps run."""
    import octreeraytracer_amd as ort
    steps = plan()[seed][first:None if last is None else last + 1]
    with GpuAdapter(ort, stream=stream or None) as ad:
        run(ad, steps, seed, first, batch or (BATCH if stream else 1))
    return len(steps)
