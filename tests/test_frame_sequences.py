"""The plan of tests/frame_sequences.py and its runner, without a GPU.

The plan is deterministic and covers what its docstring says.  A faithful fake adapter, built on
the host emulation of the kernels' per-pixel code (emulate_render_host, query_rays_host and the
prefix emulation for accumulation passes), runs the whole plan and passes: that proves the
references and the runner's tile, pitch, placement and format arithmetic -- the fake places its
pixels with code of its own.  Faulty fakes, each wrong in one way at one step, must be caught at
exactly that step."""
import collections
import dataclasses

import numpy as np
import pytest

import frame_sequences as FS
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.image import to_srgb8
from octreeraytracer_amd.renderer import emulate_render_host, query_rays_host

PLAN = FS.plan()
SEEDS = FS.seeds()


class Fake:
    """What a context must do, restated on the host: no state but the scene and the accumulation."""

    def __init__(self, ort):
        self.ort, self.options, self.scene, self.acc, self.step_index = ort, {}, None, None, -1

    def sync(self):
        pass

    def set_option(self, name, value):
        assert name in FS.OPTION_IDS, name
        self.options[name] = value

    def upload(self, spheres, tree, build=None):
        if build:
            tree = self.ort.build_octree(spheres, *build)
        layout = L.ORT_LAYOUT_EXPLICIT if self.options["force_layout"] == 1 else L.ORT_LAYOUT_COMPACT
        self.scene = (spheres, tree, layout)
        if self.acc:
            self.acc["valid"] = False

    def picture(self, params, tile, samples_done=None):
        s, t, layout = self.scene
        return emulate_render_host(s, t if params.use_octree else None, params, self.ort.Tile(*tile), layout=layout,
                                   samples_done=samples_done)

    def place(self, img, height, tile, d):
        """The prefilled buffer with the picture written as the description says, row by row."""
        buf = np.full(d["nbytes"] + FS.SLACK, FS.FILL, np.uint8)
        x0, w, y0, rows, bh, bs = tile
        bpp = 12 if d["fmt"] == "rgb32f" else 4
        pitch = d["pitch"] or (params_width(d, w) * bpp)
        for j in range(rows):
            y = y0 + (j // bh) * bs + j % bh if bh > 0 else y0 + j
            if d["fmt"] == "rgb32f":
                row = img[j].astype(np.float32).tobytes()
            else:
                row = np.concatenate([to_srgb8(img[j]), np.full((w, 1), self.alpha(), np.uint8)], axis=1).tobytes()
            if y >= height:
                if d["place"] == "frame":
                    continue
                row = self.padding_row(len(row))
            at = j * pitch if d["place"] == "tile" else y * pitch + x0 * bpp
            buf[at:at + len(row)] = np.frombuffer(row, np.uint8)
        return buf

    def alpha(self):
        return 255

    def padding_row(self, n):
        return bytes(n)

    def render(self, params, tile, d):
        if tile[1] * tile[3] == 0:
            return None if not d["device"] else np.full(d["nbytes"] + FS.SLACK, FS.FILL, np.uint8)
        d = dict(d, frame_width=params.width)
        img, _ = self.picture(params, tile)
        return self.place(self.shade(img, params, tile), params.height, tile, d)

    def shade(self, img, params, tile):
        return img

    def count(self, params, tile):
        if tile[1] * tile[3] == 0:
            return dict.fromkeys(L.COUNT_NAMES, 0)
        return self.picture(params, tile)[1]

    def query(self, rays, use_octree, sort):
        s, t, layout = self.scene
        tt, sphere = query_rays_host(s, t, rays, layout=layout, use_octree=use_octree)
        return np.stack([tt.view(np.int32), sphere], axis=1)

    def accum(self, what, *args):
        if what == "begin":
            self.acc = {"params": args[0], "tile": args[1], "done": 0, "valid": True}
        elif what == "restart":
            self.acc.update(params=args[0], done=0, valid=True)
        else:
            n, d = args
            a = self.acc
            assert a["valid"], "a pass on an accumulation whose scene changed"
            a["done"] += min(n, a["params"].num_samples - a["done"])
            img, _ = self.picture(a["params"], a["tile"], samples_done=self.divisor(a))
            return self.place(img, a["params"].height, a["tile"], dict(d, frame_width=a["params"].width))

    def divisor(self, a):
        return a["done"]

    def read(self, h):
        return h


def params_width(d, tile_width):
    return d["frame_width"] if d["place"] == "frame" else tile_width


# ---- the plan -----------------------------------------------------------------------------------------
def test_the_plan_is_deterministic():
    FS.plan.cache_clear()
    again = FS.plan()
    assert again == PLAN and list(again) == list(PLAN)
    assert all(len(s) <= FS.MAX_STEPS for s in PLAN.values())
    n_seq, n_steps, n_frames = FS.totals()
    print(f"{n_seq} sequences, {n_steps} steps, {n_frames} distinct reference frames")
    assert n_seq == len(SEEDS) and n_steps > 1000 and n_frames > 100


def test_every_sandwich_is_there():
    have = set()
    for steps in PLAN.values():
        for a, x, b in zip(steps, steps[1:], steps[2:]):
            if a.recipe() == b.recipe() and a.name != x.name:
                have.add((a.name, x.name))
    want = {(a, x) for a in FS.NAMES for x in FS.NAMES if a != x}
    assert len(FS.KINDS) == 16 and len(FS.ACTIONS) == 6
    assert not want - have, sorted(want - have)[:10]


def test_every_variant_is_there():
    for kind in FS.STATEFUL:
        for v in FS.VARIANTS:
            found = []
            for steps in PLAN.values():
                for a, x, b in zip(steps, steps[1:], steps[2:]):
                    if x.tag == f"variant:{v}:{kind}" and a.name == kind and a.recipe() == b.recipe() and a is not x:
                        found.append((a, x))
            assert found, (kind, v)
            for a, x in found:
                if v == "camera":
                    assert x == dataclasses.replace(a, camera="turned") and a.camera == "chart"
                elif v == "twin":
                    assert x.name == "twin"
                elif v == "option":  # one option the signature does not hold, and the camera
                    changed = set(dict(a.options).items()) ^ set(dict(x.options).items())
                    assert len({k for k, _ in changed}) == 1, changed
                    assert {k for k, _ in changed} <= {"cost_order", "split_heavy", "split_level", "heavy_first", "persistent",
                                                       "sort_paths", "kid_skip", "pixel_speculate"}
                    assert dataclasses.replace(x, options=a.options, camera=a.camera) == a
                else:  # more slots than A's: the grow-only buffers are reallocated
                    ta, tx = FS.tile_of(a), FS.tile_of(x)
                    assert tx[1] * tx[3] > ta[1] * ta[3] and x.shape == a.shape
            if v == "option":
                assert len(found) == len(FS.KINDS[kind].changed)


def test_every_value_of_every_dimension_occurs():
    frames = [s for steps in PLAN.values() for s in steps if s.is_frame]
    seen = collections.Counter()
    for s in frames:
        seen.update([("size", s.size), ("camera", s.camera), ("tile", s.tile), ("output", s.output)])
        o = dict(FS.OPTION_DEFAULTS)
        o.update(s.options)
        seen.update((k, o[k]) for k in FS.MISC)
    want = ([("size", v) for v in FS.SIZES] + [("camera", v) for v in FS.CAMERAS] + [("tile", v) for v in FS.TILES] +
            [("output", v) for v in FS.OUTPUTS] + [(k, v) for k, vs in FS.MISC.items() for v in vs])
    low = {k: seen[k] for k in want if seen[k] < 10}
    assert not low, low
    for a in FS.ACTIONS:
        assert sum(s.name == a for steps in PLAN.values() for s in steps) >= 10, a
    assert {s.scene for steps in PLAN.values() for s in steps} == set(FS.SCENES)


def test_the_scenes_are_what_the_plan_says(ort, oracle):
    s, t = FS.scene("d4")
    assert t.n_nodes == 105 and FS.scene("d6")[1].n_nodes == 181_769
    assert 16 * t.n_nodes + 16 * (t.n_indices + s.n) <= 32768  # resident in LDS for whole-pixel paths
    assert FS.tree_depth(FS.scene("deep")[1]) > 8 and FS.tree_depth(t) == 4
    s2, t2 = FS.scene("d4", True)
    assert t2 is t and np.array_equal(s2.center_radius, s.center_radius) and not np.array_equal(s2.mat_albedo, s.mat_albedo)
    key = ("chart", (97, 63), (2, 4), 1, FS.TILES["full"](97, 63))
    a, b = FS.frame_reference("d4", False, *key), FS.frame_reference("d4", True, *key)
    assert (a != b).any(axis=-1).mean() > 0.5  # the twin changes more than half the frame
    c = FS.frame_reference("d4", False, "turned", *key[1:])
    assert (a != c).any(axis=-1).mean() > 0.5  # and so does half a degree of yaw
    # the sky pose: no ray is ever accepted, so every bounce list is empty
    counts = FS.count_reference("d4", False, "sky", (48, 32), (2, 4), 1, FS.TILES["full"](48, 32))
    assert counts["accepted_hits"] == 0 and counts["traversals"] == 2 * 48 * 32
    # the long frame: more than 64 hint indices, 16 timed launches, 8 recorded bounces
    ns, md = FS.KINDS["pipe_long"].shapes[0]
    assert ns * md > 64 and ns * md > 16 and ns > 8 and md >= 8
    tree, each = FS.query_reference("d4")
    assert 0.1 < (tree[:, 0] == 1).mean() < 0.9 and (each[:, :, 0] == 1).any(axis=1).sum() >= 20, (each[:, :, 0] == 1).any(axis=1).sum()


def test_no_picture_equals_the_one_before_it():
    compared = 0
    for seed, steps in PLAN.items():
        state, last = FS.State(), None
        for i, st in enumerate(steps):
            state.advance(st)
            pic = state.picture(st)
            if last is not None and pic is not None and last.shape == pic.shape:
                compared += 1
                assert FS.differs(last, pic), (seed, i, st)
            last = pic
    assert compared >= 100, compared


# ---- the faithful fake ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_the_faithful_fake_passes(ort, seed):
    """(The whole plan takes about ten seconds on the host, so no sequence is left to `slow`.)"""
    FS.run(Fake(ort), PLAN[seed], seed, batch=FS.BATCH if seed % 2 else 1)


@pytest.mark.parametrize("name", list(FS.REGRESSIONS))
def test_the_faithful_fake_passes_the_regression_cases(ort, name):
    FS.run(Fake(ort), FS.REGRESSIONS[name], name)


def test_two_fakes_in_turn(ort):
    a, b = SEEDS[-1], SEEDS[-2]
    FS.run_in_turn([FS.Runner(Fake(ort), PLAN[a][:40], a), FS.Runner(Fake(ort), PLAN[b][:25], b, batch=FS.BATCH)])


# ---- faulty fakes ---------------------------------------------------------------------------------------
def where(pred, after=1):
    """(seed, index) of the first step of the plan, with at least `after` steps before it, that
    pred(steps, index) accepts."""
    for seed, steps in PLAN.items():
        for i in range(after, len(steps)):
            if pred(steps, i):
                return seed, i
    raise AssertionError("the plan holds no such step")


def caught(ort, fake_class, seed, index, lead=12, batch=1):
    """Run the slice around `index` on the faulty fake: the mismatch must name that step."""
    first = max(0, index - lead)
    steps = PLAN[seed][first:index + 3]
    fake = fake_class(ort)
    fake.bad = index
    with pytest.raises(FS.Mismatch) as e:
        FS.run(fake, steps, seed, first, batch)
    assert (e.value.seed, e.value.index) == (seed, index), str(e.value)
    text = str(e.value)
    assert f"seed {seed}, step {index}:" in text and "the steps before it" in text and str(PLAN[seed][index]) in text
    FS.run(Fake(ort), steps, seed, first, batch)  # the faithful fake passes the same slice
    return text


def is_float_frame(steps, i):
    return steps[i].is_frame and steps[i].output.endswith("f32") and steps[i].tile in ("full", "sub")


@pytest.mark.parametrize("batch", [1, FS.BATCH])
def test_a_stale_frame_is_caught(ort, batch):
    """The frame of the same signature rendered two steps earlier, returned again."""
    class Stale(Fake):
        def picture(self, params, tile, samples_done=None):
            kept = self.__dict__.setdefault("kept", {})
            key = (params.width, params.height, params.num_samples, params.max_depth, tile)
            if self.step_index != self.bad:
                kept[key] = Fake.picture(self, params, tile, samples_done)
            return kept[key]

    seed, i = where(lambda s, i: s[i - 1].tag.startswith("variant:camera:") and s[i - 1].camera == "turned", 2)
    assert PLAN[seed][i].recipe() == PLAN[seed][i - 2].recipe()
    text = caught(ort, Stale, seed, i, batch=batch)
    assert "is not the oracle's" in text and "buffer row" in text


def test_one_ulp_is_caught(ort):
    class Ulp(Fake):
        def shade(self, img, params, tile):
            if self.step_index == self.bad:
                img = img.copy()
                v = img[-1, -1, 1:2].view(np.uint32)
                v += 1
            return img

    assert "buffer row" in caught(ort, Ulp, *where(is_float_frame))


def test_padding_rows_left_unwritten_are_caught(ort):
    class NoPadding(Fake):
        def padding_row(self, n):
            return bytes([FS.FILL] * n) if self.step_index == self.bad else bytes(n)

    caught(ort, NoPadding, *where(lambda s, i: s[i].is_frame and s[i].tile == "band" and not s[i].output.startswith("frame")))


def test_a_pixel_past_a_pitched_row_is_caught(ort):
    class PastTheRow(Fake):
        def place(self, img, height, tile, d):
            buf = Fake.place(self, img, height, tile, d)
            if self.step_index == self.bad:
                bpp = 12 if d["fmt"] == "rgb32f" else 4
                at = tile[1] * bpp  # just after row 0's pixels
                buf[at:at + bpp] = buf[at - bpp:at]
            return buf

    text = caught(ort, PastTheRow, *where(lambda s, i: s[i].is_frame and s[i].output.startswith("pitch") and
                                          s[i].tile in ("full", "sub", "band")))
    assert "between rows" in text


def test_alpha_254_is_caught(ort):
    class Alpha(Fake):
        def alpha(self):
            return 254 if self.step_index == self.bad else 255

    caught(ort, Alpha, *where(lambda s, i: s[i].is_frame and s[i].output.endswith("rgba8") and s[i].tile != "none"))


def test_a_counter_off_by_one_is_caught(ort):
    class Counter(Fake):
        def count(self, params, tile):
            c = dict(Fake.count(self, params, tile))
            if self.step_index == self.bad:
                c["leaf_objects"] += 1
            return c

    assert "count_traffic" in caught(ort, Counter, *where(lambda s, i: s[i].name == "count"))


@pytest.mark.parametrize("use_octree", [1, 0])
def test_a_neighbouring_rays_record_is_caught(ort, use_octree):
    class Neighbour(Fake):
        def query(self, rays, use_octree, sort):
            rec = Fake.query(self, rays, use_octree, sort)
            if self.step_index == self.bad:
                hit = np.nonzero(rec[:-1, 1] != rec[1:, 1])[0][0]
                rec[hit] = rec[hit + 1]
            return rec

    assert "query" in caught(ort, Neighbour, *where(lambda s, i: s[i].name == "query" and s[i].use_octree == use_octree))


def test_a_preview_divided_by_n_is_caught(ort):
    """The prefix emulation divides by the samples done: asked for all N it divides by N."""
    class ByN(Fake):
        def accum(self, what, *args):
            if what != "step" or self.step_index != self.bad:
                return Fake.accum(self, what, *args)
            n, d = args
            a = self.acc
            a["done"] += min(n, a["params"].num_samples - a["done"])
            k, N = a["done"], a["params"].num_samples
            img, _ = self.picture(a["params"], a["tile"], samples_done=k)
            linear = img.astype(np.float64) ** 2.2 * k / N  # the sum over k samples, divided by N
            return self.place((linear ** (1 / 2.2)).astype(np.float32), a["params"].height, a["tile"],
                              dict(d, frame_width=a["params"].width))

    # the checked previews are those after 4, 5 or 6 of 7 samples: find a pass that ends on one in the slice
    for seed, steps in PLAN.items():
        for i, st in enumerate(steps):
            if st.name != "accum":
                continue
            first = max(0, i - 12)
            state = FS.State()
            for s in steps[first:i + 1]:
                state.advance(s)
            if FS.isqrt(state.acc["done"]) == FS.isqrt(FS.ACC_N) and state.acc["done"] < FS.ACC_N:
                caught(ort, ByN, seed, i)
                return
    raise AssertionError("no checked preview in the plan")


def test_a_finished_accumulation_is_checked():
    """Over the plan: passes that end on a checked preview, and on the finished frame."""
    previews = finished = 0
    for steps in PLAN.values():
        state = FS.State()
        for st in steps:
            state.advance(st)
            if st.name == "accum" and state.picture(st) is not None:
                previews += state.acc["done"] < FS.ACC_N
                finished += state.acc["done"] == FS.ACC_N
    assert previews >= 10 and finished >= 5, (previews, finished)
