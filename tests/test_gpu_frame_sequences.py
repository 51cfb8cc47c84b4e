"""Sequences of frames on the GPU (tests/frame_sequences.py): one context taken through every
render route after every other, every output compared byte for byte with the oracle's.

  synchronously    each sequence on the context's own stream, each step checked before the next
  stream-ordered   each sequence on one caller's stream in batches of 6 steps into distinct device
                   buffers, nothing waited for inside a batch: several shapes in flight at once,
                   more than the four hint banks
  two contexts     two sequences on two contexts of one process, stepping in turn: state that
                   lived outside ort_ctx would show

A mismatch names the seed and the step; frame_sequences.replay(seed, first, last) runs a slice
again.  An ORT_ERR_HIP ends the session (pytest.exit): nothing more starts on the GPU.

Groups are out of scope (test_group_pipelined_frames streams changing frames through slot
contexts), and so is RCCL."""
import pytest

import frame_sequences as FS

pytestmark = pytest.mark.gpu

PLAN = FS.plan()
SEEDS = FS.seeds()


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_synchronously(ort, seed):
    with FS.GpuAdapter(ort) as ad:
        FS.run(ad, PLAN[seed], seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_stream_ordered(ort, seed):
    with FS.GpuAdapter(ort, stream=True) as ad:
        FS.run(ad, PLAN[seed], seed, batch=FS.BATCH)


@pytest.mark.parametrize("a,b", list(zip(SEEDS[0::2], SEEDS[1::2])))
def test_two_contexts_in_turn(ort, a, b):
    with FS.GpuAdapter(ort) as one, FS.GpuAdapter(ort, stream=True) as two:
        FS.run_in_turn([FS.Runner(one, PLAN[a], a), FS.Runner(two, PLAN[b], b, batch=FS.BATCH)])


@pytest.mark.parametrize("mode", ["synchronously", "stream_ordered", "beside_a_busy_context"])
@pytest.mark.parametrize("name", list(FS.REGRESSIONS))
def test_regression_case(ort, name, mode):
    """The sequences that once failed, cut down by hand (frame_sequences.REGRESSIONS), five times
    over; the third mode steps in turn with a second context that renders a generated sequence."""
    steps = FS.REGRESSIONS[name] * 5
    with FS.GpuAdapter(ort, stream=mode == "stream_ordered") as ad:
        mine = FS.Runner(ad, steps, name, batch=FS.BATCH if mode == "stream_ordered" else 1)
        if mode != "beside_a_busy_context":
            mine.run()
            return
        with FS.GpuAdapter(ort, stream=True) as busy:
            FS.run_in_turn([mine, FS.Runner(busy, PLAN[SEEDS[0]][:len(steps)], SEEDS[0], batch=FS.BATCH)])


@pytest.mark.parametrize("scene_name", list(FS.SCENES))
def test_the_kinds_take_their_routes(ort, scene_name):
    """Each kind's options force its route: three frames of it on a fresh context, and the trace
    launches the context timed for each -- one for a direct frame and for whole-pixel paths, one
    per sample and bounce for the pipeline (at most 16 are timed), three for a speculating frame
    from the shape's second frame on, none where nothing is traced."""
    import dataclasses
    for kind, k in FS.KINDS.items():
        ns, md = k.shapes[-1]
        st = dataclasses.replace(FS.Step(kind, scene_name, k.size or (97, 63), (ns, md), k.use_octree),
                                 options=FS._options(kind, {}))
        with FS.GpuAdapter(ort) as ad:
            seen = []
            for _ in FS.Runner(ad, [st] * 3).steps():
                timed = ad.r.frame_trace_times_ms(1)
                seen.append(timed[0][1] if timed else 0)
        if md == 0:
            want = [0, 0, 0]
        elif kind == "pixel_spec":
            want = [1, 3, 3]
        elif dict(k.options).get("pixel_paths") == 1 or (ns, md) == (1, 1):
            want = [1, 1, 1]
        else:
            want = [min(ns * md, 16)] * 3
        assert seen == want, (scene_name, kind, seen, want)


def test_the_deep_scene_is_deep(ort):
    s, t = FS.scene("deep")
    with ort.Renderer(0) as r:
        r.upload(s, t)
        assert r.info()["tree_depth"] > 8 and r.info()["tree_depth"] == FS.tree_depth(t)
        assert r.info()["layout"] == "compact"
