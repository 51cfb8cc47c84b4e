"""The plan of tests/call_sequences.py and its runner, without a GPU.

The plan is deterministic and covers what its docstring says.  A faithful fake adapter, built on
the host emulations of the kernels' per-ray and per-pixel code (emulate_render_host,
query_rays_host, camera_query_host, radiance_rays_host, denoise_host, accum_moments_host,
accum_adaptive_host), runs the whole plan and passes: that proves the references against the
emulations and the runner's record, padding, pitch and slack arithmetic -- the fake has no state
but the scene and the three accumulations and places its records with code of its own.  Faulty
fakes, each wrong in one way at one step, must be caught at exactly that step."""
import collections

import numpy as np
import pytest

import call_sequences as CQ
import frame_sequences as FS
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd import renderer as R
from test_frame_sequences import Fake as FrameFake

PLAN = CQ.plan()
SEEDS = CQ.seeds()


def filled(nbytes, payload=None):
    buf = np.full(nbytes + CQ.SLACK, CQ.FILL, np.uint8)
    if payload is not None:
        payload = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        assert len(payload) == nbytes, (len(payload), nbytes)
        buf[:nbytes] = payload
    return buf


def records(t, sphere):
    return np.stack([np.ascontiguousarray(t).view(np.int32).reshape(-1), np.asarray(sphere, np.int32).reshape(-1)], axis=1)


class Fake(FrameFake):
    """What a context must do, restated on the host: no state but the scene and the accumulations."""
    REFUSED = {"t_range_drawn": 1, "normals_without_hits": 1, "paths_0": 1, "iterations_7": 1, "variance_plain": 1,
               "adaptive_on_plain": 1, "radiance_explicit": 5, "begin_explicit": 5}

    def __init__(self, ort):
        super().__init__(ort)
        self.accs = {}

    def upload(self, spheres, tree, build=None):
        super().upload(spheres, tree, build)
        for a in self.accs.values():
            a["valid"] = False

    def read_all(self, h):
        return h

    # accumulations
    def acc_begin(self, which, params, tile):
        self.accs[which] = {"params": params, "tile": self.ort.Tile(*tile), "passes": [], "valid": True}

    def acc_restart(self, which, params):
        self.accs[which].update(params=params, passes=[], valid=True)

    def acc_state(self, which, passes=None):
        """(counts, mean, variance) of an accumulation after its passes."""
        a = self.accs[which]
        s, t, layout = self.scene
        passes = a["passes"] if passes is None else passes
        if which == "adaptive":
            return R.accum_adaptive_host(s, t, a["params"], a["tile"], layout, passes)
        k = min(a["params"].num_samples, sum(p[0] for p in passes))
        mean, var = R.accum_moments_host(s, t, a["params"], a["tile"], layout, samples_done=k)
        return np.full(var.shape, k, np.int32), mean, var

    def acc_pass(self, which, n, crit, d):
        a = self.accs[which]
        assert a["valid"], "a pass on an accumulation whose scene changed"
        a["passes"].append(tuple(crit) if crit else (n, 0, 0.0, CQ.FLOOR))
        if d is None:
            return None
        if which == "adaptive":
            img = R.gamma_host(self.acc_state(which)[1]).reshape(a["tile"].rows, a["tile"].width, 3)
        else:
            k = min(a["params"].num_samples, sum(p[0] for p in a["passes"]))
            img, _ = self.picture(a["params"], (0, a["params"].width, 0, a["params"].height, 0, 0), samples_done=k)
        t = a["tile"]
        return self.place(img, a["params"].height, (t.x0, t.width, t.y0, t.rows, t.band_height, t.band_stride),
                          dict(d, frame_width=a["params"].width))

    # the calls
    def query(self, scene_name, name, a):
        s, t, layout = self.scene
        if name == "rays":
            rays, t_range, mode = CQ.ray_source(scene_name, ("set",))[0][CQ.selection(a)], None, None
        else:
            (rays, t_range), mode = CQ.mode_inputs(scene_name, a), name[5:]
        return R.query_rays_host(s, t, rays, layout=layout, use_octree=bool(a["use_octree"]), normals=True, mode=mode,
                                 t_range=t_range)

    def camera(self, a):
        s, t, layout = self.scene if self.scene else (None, None, 0)
        p = CQ.camera_params(a)
        tile = self.ort.Tile(*FS.TILES[a["tile"]](*a["size"]))
        if "hits" not in a["want"]:
            return R.camera_query_host(None, None, p, tile, which=a["which"], hits=False), None, None, None
        return R.camera_query_host(s, t if a["use_octree"] else None, p, tile, which=a["which"], layout=layout, normals=True)

    def radiance(self, scene_name, a, scene=None):
        s, t, layout = scene or self.scene
        rays, states = CQ.radiance_inputs(scene_name, a)
        return R.radiance_rays_host(s, t if a["use_octree"] else None, rays, states, max_depth=a["depth"], paths=a["paths"],
                                    layout=layout, use_octree=bool(a["use_octree"]), sort=bool(a["sort"]),
                                    normalize=bool(a["normalize"]), gamma=bool(a["gamma"]), states_out=True)

    def denoise(self, a, guides=None):
        """The call's output buffer: the filtered picture, tight, placed row by row."""
        image, t, sph, nrm, var = CQ.denoise_inputs(a)
        t, sph, nrm = guides or (t, sph, nrm)
        kw = dict(variance=var, sigma_variance=CQ.SIGMA_VARIANCE, gamma=bool(a["gamma"])) if var is not None else {}
        out = R.denoise_host(image, ((t, sph), nrm), iterations=a["iterations"], format=a["fmt"], **kw)
        bpp = 12 if a["fmt"] == "rgb32f" else 4
        pitch = (a["cols"] + 3 if a["pitched"] else a["cols"]) * bpp
        buf = filled(a["rows"] * pitch)
        for j in range(a["rows"]):
            row = out[j].tobytes()
            buf[j * pitch:j * pitch + len(row)] = np.frombuffer(row, np.uint8)
        return buf

    def stats(self, crit):
        a = self.accs["adaptive"]
        counts, _, _ = self.acc_state("adaptive")
        after, _, _ = self.acc_state("adaptive", a["passes"] + [tuple(crit)])
        inside = (a["tile"].pixel_rows(a["params"].height) < a["params"].height)[:, None] & np.ones(counts.shape, bool)
        c = counts[inside]
        return {"pixels": int(inside.sum()), "samples": int(c.sum(dtype=np.int64)), "pending": int((after != counts)[inside].sum()),
                "min_count": int(c.min()) if c.size else 0, "max_count": int(c.max()) if c.size else 0}

    def call(self, st, state, sizes):
        a, name, scene_name = st.a, st.name, state.scene[0]
        if name in ("rays", "rays_nearest", "rays_any"):
            t, sph, nrm = self.query(scene_name, name, a)
            return {"hits": filled(8 * a["n"], records(t, sph)),
                    "normals": filled(12 * a["n"], nrm) if a["normals"] else filled(12 * a["n"])}
        if name == "camera":
            rays, t, sph, nrm = self.camera(a)
            n = rays.shape[0] * rays.shape[1]
            return {"rays": filled(24 * n, rays) if "rays" in a["want"] else filled(24 * n),
                    "hits": filled(8 * n, records(t, sph)) if "hits" in a["want"] else filled(8 * n),
                    "normals": filled(12 * n, nrm) if "normals" in a["want"] else filled(12 * n)}
        if name == "radiance":
            rad, end = self.radiance(scene_name, a)
            out = {"radiance": filled(12 * a["n"], rad)}
            if a["states_out"] != "null":
                out["states_out"] = filled(8 * a["n"], end)
            return out
        if name in CQ.DENOISE:
            return {"out": self.denoise(a)}
        if name in CQ.PASSES:
            fs = CQ.picture_step(CQ.ACC[a["big"]][0], a["output"])
            return {"out": self.acc_pass(CQ.acc_of(st), a["n"], CQ.criterion(a) if name == "pass_adaptive" else None,
                                         FS.describe_output(fs))}
        if name == "read_moments":
            assert self.accs[a["acc"]]["valid"]
            _, mean, var = self.acc_state(a["acc"])
            out = {}
            if a["parts"] != "variance":
                out["mean"] = filled(mean.nbytes, mean)
            if a["parts"] != "mean":
                out["variance"] = filled(var.nbytes, var)
            return out
        if name == "read_counts":
            assert self.accs["adaptive"]["valid"]
            counts = self.acc_state("adaptive")[0]
            return {"counts": filled(counts.nbytes, counts)}
        if name == "stats":
            return {"stats": self.stats(CQ.criterion(a))}
        if name == "refused":
            v = a["variant"]
            if v in ("radiance_explicit", "begin_explicit"):
                assert self.scene[2] == L.ORT_LAYOUT_EXPLICIT
            if v in ("variance_plain", "adaptive_on_plain"):
                assert self.accs["plain"]["valid"] and self.accs["plain"]["passes"]
            bufs = {"t_range_drawn": ("hits",), "normals_without_hits": ("rays", "normals"), "paths_0": ("radiance", "states_out"),
                    "radiance_explicit": ("radiance", "states_out"), "iterations_7": ("out",), "variance_plain": ("mean", "variance"),
                    "adaptive_on_plain": ("out",), "begin_explicit": ()}[v]
            return self.REFUSED[v], {k: filled(256) for k in bufs}
        raise AssertionError(name)


# ---- the plan -----------------------------------------------------------------------------------------
def test_the_plan_is_deterministic():
    CQ.plan.cache_clear()
    again = CQ.plan()
    assert again == PLAN and list(again) == list(PLAN)
    assert all(len(s) <= CQ.MAX_STEPS for s in PLAN.values())
    assert not set(PLAN) & set(FS.plan()) and CQ.REGRESSIONS == {}
    n_seq, n_steps, n_refs = CQ.totals()
    print(f"{n_seq} sequences, {n_steps} steps, {n_refs} distinct references")
    assert n_seq == len(SEEDS) and n_steps > 1000 and n_refs > 200


def test_the_names_are_the_issues():
    assert len(CQ.NAMES) == 23 == len(set(CQ.NAMES))
    for name in CQ.FRAMES:   # as they stand in frame_sequences, drawn by its _draw
        assert name in FS.KINDS
    for steps in PLAN.values():
        for st in steps:
            if st.is_frame:
                assert st.frame.name == st.name and dict(FS.KINDS[st.name].options).items() <= dict(
                    FS.OPTION_DEFAULTS, **dict(st.frame.options)).items()


def test_every_sandwich_is_there():
    have = set()
    for steps in PLAN.values():
        for a, x, b in zip(steps, steps[1:], steps[2:]):
            if a.recipe() == b.recipe() and a.name != x.name:
                have.add((a.name, x.name))
    want = {(a, x) for a in CQ.NAMES for x in CQ.NAMES if a != x}
    assert not want - have, sorted(want - have)[:10]


def test_every_size_variant_is_there():
    for name in CQ.SIZED:
        for v in CQ.VARIANTS:
            found = [(a, x) for steps in PLAN.values() for a, x, b in zip(steps, steps[1:], steps[2:])
                     if x.tag == f"variant:{v}:{name}" and a.recipe() == b.recipe() and a.name == x.name == name and a != x]
            assert found, (name, v)
            for a, x in found:
                if v == "pointers":
                    assert a.a["device"] == 0 and x.a["device"] == 1
                    assert {k for k in a.a if a.a[k] != x.a[k]} <= {"device", "stride", "camera", "img"}
                elif name == "camera":
                    ta, tx = FS.TILES[a.a["tile"]](*a.a["size"]), FS.TILES[x.a["tile"]](*x.a["size"])
                    assert tx[1] * tx[3] >= 10 * ta[1] * ta[3]
                elif name in CQ.DENOISE:
                    assert x.a["cols"] * x.a["rows"] >= 10 * a.a["cols"] * a.a["rows"]
                else:
                    assert x.a["n"] == 3001 and a.a["n"] <= 129


def test_every_value_of_every_dimension_occurs():
    seen = CQ.occurrences(PLAN.values())
    low = {(CQ.FAMILY.get(n, n), k, v): seen[(CQ.FAMILY.get(n, n), k, v)] for n, dims in CQ.DIMS.items() for k, vs in dims.items()
           for v in vs if seen[(CQ.FAMILY.get(n, n), k, v)] < 10}
    assert not low, low
    names = collections.Counter(st.name for steps in PLAN.values() for st in steps)
    assert all(names[n] >= 10 for n in CQ.NAMES), names
    frames = [st.frame for steps in PLAN.values() for st in steps if st.is_frame]
    for dim, values in (("tile", FS.TILES), ("output", FS.OUTPUTS), ("camera", FS.CAMERAS), ("size", FS.SIZES)):
        c = collections.Counter(getattr(f, dim) for f in frames)
        assert all(c[v] >= 10 for v in values), (dim, c)
    assert {st.scene for steps in PLAN.values() for st in steps} == set(FS.SCENES)
    tours = {st.scene: collections.Counter() for steps in PLAN.values() for st in steps if st.tag.startswith("tour:")}
    for steps in PLAN.values():
        for st in steps:
            if st.tag.startswith("tour:"):
                tours[st.scene][st.name] += 1
    assert set(tours) == {"d6", "deep"} and all(c[n] == 3 for c in tours.values() for n in CQ.NAMES)


def test_no_output_equals_its_neighbours():
    compared = 0
    for seed, steps in PLAN.items():
        last = None
        for i, (st, state) in enumerate(CQ.walk(steps)):
            ref = CQ.primary(state, st)
            if last is not None and ref is not None and last.shape == ref.shape and last.dtype == ref.dtype:
                compared += 1
                assert CQ.differs(last, ref), (seed, i, st)
            last = ref
    assert compared >= 2 * len(CQ.SIZED), compared   # (at least the pointer variants: the same shape three times)


def test_the_adaptive_accumulation_holds_distinct_counts():
    assert CQ.distinct_count_steps(PLAN) >= 10
    steps = PLAN[CQ.large_seed()]
    (W, H), N, depth = CQ.ACC[True]
    assert all(st.tag == "large" and st.a["big"] and st.name in CQ.ACCUM for st in steps)
    assert ((W + 15) // 16) * ((H + 15) // 16) == 272 > 256 and (N, depth) == (4, 2)   # more workgroups than kAdaptiveStatBlocks
    checked = collections.Counter()
    for st, state in CQ.walk(steps):
        if st.name == "stats":
            want = CQ.stats_reference(state, CQ.criterion(st.a))
            assert want["pixels"] == W * H
            checked["stats"] += 1
            checked["pending"] += 0 < want["pending"] < W * H
            checked["spread"] += want["min_count"] < want["max_count"]
    assert checked["stats"] >= 5 and checked["pending"] >= 2 and checked["spread"] >= 2, checked


def test_where_the_reference_is_the_emulation():
    assert CQ.non_emulation_names() == set(CQ.NAMES) - {"read_moments"}
    tied = 0
    for steps in PLAN.values():
        for st, state in CQ.walk(steps):
            if st.name == "read_moments" and st.a["parts"] != "variance" and not st.a["big"]:
                tie = CQ.moments_tie(state, st.a["acc"])
                assert tie is not False, st
                tied += tie is True
    assert tied >= 10, tied


# ---- the faithful fake ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_the_faithful_fake_passes(ort, seed):
    """(The whole plan takes about 14 seconds on the host, after the 11 seconds in which the module
    makes the plan and with it most references; the 272 x 248 sequence is 8 seconds of the 14.)"""
    CQ.run(Fake(ort), PLAN[seed], seed, batch=FS.BATCH if seed % 2 else 1)


def test_the_faithful_fake_passes_the_regression_cases(ort):
    for name, steps in CQ.REGRESSIONS.items():
        CQ.run(Fake(ort), steps, name)


def test_two_fakes_in_turn(ort):
    a, b = SEEDS[1], SEEDS[2]
    CQ.run_in_turn([CQ.Runner(Fake(ort), PLAN[a][:40], a), CQ.Runner(Fake(ort), PLAN[b][:25], b, batch=FS.BATCH)])


# ---- faulty fakes ---------------------------------------------------------------------------------------
LEAD = 12


def slice_of(seed, index, lead=LEAD):
    """(first, [(i, step, state after it, what it implied)]) of the slice a faulty fake runs."""
    first = max(0, index - lead)
    state, out = CQ.State(), []
    for i, st in enumerate(PLAN[seed][first:index + 3], first):
        do = state.advance(st)
        out.append((i, st, state.copy(), do))
    return first, out


def where(pred, after=1):
    """(seed, index) of the first step of the plan, with at least `after` steps before it, that
    pred(steps, index) accepts."""
    for seed, steps in PLAN.items():
        for i in range(after, len(steps)):
            if pred(steps, i, seed):
                return seed, i
    raise AssertionError("the plan holds no such step")


def caught(ort, fake_class, seed, index, at=None, batch=1, lead=LEAD):
    """Run the slice around `index` on the faulty fake (wrong at step `at`, default `index`): the
    mismatch must name step `index`, and the faithful fake passes the same slice."""
    first = max(0, index - lead)
    steps = PLAN[seed][first:index + 3]
    fake = fake_class(ort)
    fake.bad = index if at is None else at
    with pytest.raises(CQ.Mismatch) as e:
        CQ.run(fake, steps, seed, first, batch)
    assert (e.value.seed, e.value.index) == (seed, index), str(e.value)
    text = str(e.value)
    assert f"seed {seed}, step {index}:" in text and "the steps before it" in text and str(PLAN[seed][index]) in text
    CQ.run(Fake(ort), steps, seed, first, batch)
    return text


@pytest.mark.parametrize("batch", [1, FS.BATCH])
def test_records_of_the_larger_query_before_are_caught(ort, batch):
    """A query that leaves the previous, larger query's records after its own n: the slack is written."""
    class Tail(Fake):
        def call(self, st, state, sizes):
            out = Fake.call(self, st, state, sizes)
            if st.name == "rays":
                if self.step_index == self.bad:
                    n = 8 * st.a["n"]
                    out["hits"][n:] = self.kept[n:n + CQ.SLACK]
                self.kept = out["hits"].copy()
            return out

    seed, i = where(lambda s, i, _: s[i].tag == "variant:larger:rays" and s[i - 1].tag == s[i].tag and s[i - 1].a["n"] > s[i].a["n"])
    assert "written after its last record" in caught(ort, Tail, seed, i, batch=batch)


def test_camera_rays_of_the_previous_tile_are_caught(ort):
    class PreviousTile(Fake):
        def camera(self, a):
            mine = Fake.camera(self, a)
            if self.step_index == self.bad:
                old = Fake.camera(self, dict(a, tile=self.kept["tile"], size=self.kept["size"]))[0].reshape(-1)
                rays = np.resize(old, mine[0].size).reshape(mine[0].shape).astype(np.float32)
                mine = (rays,) + tuple(mine[1:])
            self.kept = a
            return mine

    def pred(s, i, seed):
        if s[i].name != "camera" or "rays" not in s[i].a["want"] or s[i].a["tile"] in ("none", "pixel"):
            return False
        before = [x for x in s[max(0, i - LEAD):i] if x.name == "camera"]
        return bool(before) and (before[-1].a["tile"], before[-1].a["size"]) != (s[i].a["tile"], s[i].a["size"]) and \
            before[-1].a["tile"] != "none"

    assert "camera: rays" in caught(ort, PreviousTile, *where(pred))


def test_states_out_left_as_given_is_caught(ort):
    class NoEndStates(Fake):
        def radiance(self, scene_name, a, scene=None):
            rad, end = Fake.radiance(self, scene_name, a, scene)
            if self.step_index == self.bad:
                end = CQ.radiance_inputs(scene_name, a)[1].copy()
            return rad, end

    for mode in ("separate", "equal"):
        text = caught(ort, NoEndStates, *where(lambda s, i, _: s[i].name == "radiance" and s[i].a["states_out"] == mode))
        assert "radiance: states_out" in text


@pytest.mark.parametrize("by_oracle", [True, False])
def test_a_radiance_record_one_ulp_off_is_caught(ort, by_oracle):
    class Ulp(Fake):
        def radiance(self, scene_name, a, scene=None):
            rad, end = Fake.radiance(self, scene_name, a, scene)
            if self.step_index == self.bad:
                v = rad[-1, 1:2].view(np.uint32)
                v += 1
            return rad, end

    text = caught(ort, Ulp, *where(lambda s, i, _: s[i].name == "radiance" and CQ.radiance_by_oracle(s[i].a) == by_oracle))
    assert "radiance: radiance" in text and ("host emulation" in text) != by_oracle


def test_the_previous_denoise_guides_are_caught(ort):
    class OldGuides(Fake):
        def denoise(self, a, guides=None):
            mine = CQ.denoise_inputs(a)[1:4]
            if self.step_index == self.bad:
                guides = tuple(np.resize(g, m.shape).astype(m.dtype) for g, m in zip(self.kept, mine))
            self.kept = mine
            return Fake.denoise(self, a, guides)

    def pred(s, i, seed):
        if s[i].name not in CQ.DENOISE:
            return False
        before = [x for x in s[max(0, i - LEAD):i] if x.name in CQ.DENOISE]
        return bool(before) and any(before[-1].a[k] != s[i].a[k] for k in ("rows", "cols", "gflip"))

    assert "out:" in caught(ort, OldGuides, *where(pred))


def test_the_variance_of_one_sample_less_is_caught(ort):
    class OneLess(Fake):
        def acc_state(self, which, passes=None):
            if self.step_index == self.bad and passes is None:
                p = list(self.accs[which]["passes"])
                p[-1] = (p[-1][0] - 1,) + tuple(p[-1][1:])
                var = Fake.acc_state(self, which, [q for q in p if q[0] > 0])[2]
                c, m, _ = Fake.acc_state(self, which)
                return c, m, var
            return Fake.acc_state(self, which, passes)

    def pred(s, i, seed):
        if s[i].name != "read_moments" or s[i].a["acc"] != "moments" or s[i].a["parts"] == "mean":
            return False
        _, sl = slice_of(seed, i)
        state = [x for x in sl if x[0] == i][0][2]
        return 2 < state.done("moments") < CQ.ACC[False][1]

    assert "read_moments: variance" in caught(ort, OneLess, *where(pred))


def test_a_held_pixel_traced_anyway_is_caught(ort):
    class Traced(Fake):
        def call(self, st, state, sizes):
            out = Fake.call(self, st, state, sizes)
            if self.step_index == self.bad:
                c = out["counts"][:-CQ.SLACK].view(np.int32)
                c[np.argmin(c)] += 1
            return out

    def pred(s, i, seed):
        if s[i].name != "read_counts" or s[i].a["big"]:
            return False
        _, sl = slice_of(seed, i, 40)
        state = [x for x in sl if x[0] == i][0][2]
        return len(np.unique(CQ.counts_of(state, "adaptive"))) >= 2

    assert "read_counts: counts" in caught(ort, Traced, *where(pred), lead=40)


def test_pending_off_by_one_on_the_large_tile_is_caught(ort):
    class Pending(Fake):
        def stats(self, crit):
            out = Fake.stats(self, crit)
            if self.step_index == self.bad:
                out["pending"] += 1
            return out

    seed = CQ.large_seed()
    i = next(i for i, st in enumerate(PLAN[seed]) if st.name == "stats" and i >= 8)
    assert "adaptive_stats" in caught(ort, Pending, seed, i)


def test_a_pass_that_advances_another_accumulation_is_caught(ort):
    """The fault is made at a pass_plain step; it shows, and is caught, at the next step on the moments
    accumulation, and nowhere before."""
    class Both(Fake):
        def acc_pass(self, which, n, crit, d):
            if self.step_index == self.bad and which == "plain" and "moments" in self.accs:
                self.accs["moments"]["passes"].append((n, 0, 0.0, CQ.FLOOR))
            return Fake.acc_pass(self, which, n, crit, d)

    def pred(s, i, seed):
        if s[i].name != "pass_moments" or s[i - 1].name != "pass_plain":
            return False
        _, sl = slice_of(seed, i)
        (_, _, state, do), (_, _, before, _) = [x for x in sl if x[0] == i][0], [x for x in sl if x[0] == i - 1][0]
        return (before.acc["moments"] is not None and before.acc["moments"]["valid"] and not do["restart"] and not do["begin"]
                and state.done("moments") < CQ.ACC[False][1])

    seed, i = where(pred, after=2)
    caught(ort, Both, seed, i, at=i - 1)


def test_a_query_for_the_old_materials_is_caught(ort):
    class OldScene(Fake):
        def upload(self, spheres, tree, build=None):
            self.old = self.scene
            Fake.upload(self, spheres, tree, build)

        def radiance(self, scene_name, a, scene=None):
            return Fake.radiance(self, scene_name, a, self.old if self.step_index == self.bad else None)

    seed, i = where(lambda s, i, _: s[i].name == "radiance" and s[i - 1].name == "twin" and s[i - 2].name == "radiance", after=2)
    assert "radiance: radiance" in caught(ort, OldScene, seed, i)


@pytest.mark.parametrize("variant", [v for v in CQ.REFUSALS if v != "begin_explicit"])
def test_a_refused_call_that_writes_is_caught(ort, variant):
    class Writes(Fake):
        def call(self, st, state, sizes):
            out = Fake.call(self, st, state, sizes)
            if self.step_index == self.bad:
                sorted(out[1].items())[0][1][5] = 0
            return out

    assert "were written" in caught(ort, Writes, *where(lambda s, i, _: s[i].name == "refused" and s[i].a["variant"] == variant))


def test_a_refused_call_that_succeeds_is_caught(ort):
    class Accepts(Fake):
        def call(self, st, state, sizes):
            out = Fake.call(self, st, state, sizes)
            return (0, out[1]) if self.step_index == self.bad else out

    assert "the header says" in caught(ort, Accepts, *where(lambda s, i, _: s[i].name == "refused"))
