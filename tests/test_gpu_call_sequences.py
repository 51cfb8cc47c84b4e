"""Sequences of calls on the GPU (tests/call_sequences.py): one context taken through the query,
denoise and accumulation calls after one another and after the stateful frame routes, every output
buffer compared byte for byte with its reference, the prefilled bytes around the records included.

  synchronously    each sequence on the context's own stream, each step checked before the next
  stream-ordered   each sequence on one caller's stream in batches of 6 steps into distinct device
                   buffers, nothing waited for inside a batch (uploads, ort_accum_begin and
                   ort_accum_adaptive_stats take no stream: the adapter waits before them)
  two contexts     two sequences on two contexts of one process, stepping in turn

A mismatch names the seed and the step; call_sequences.replay(seed, first, last) runs a slice
again.  An ORT_ERR_HIP ends the session (pytest.exit): nothing more starts on the GPU.

Groups, RCCL and the C++ Raytracer layer are out of scope, as for tests/test_gpu_frame_sequences.py."""
import pytest

import call_sequences as CQ
import frame_sequences as FS

pytestmark = pytest.mark.gpu

PLAN = CQ.plan()
SEEDS = CQ.seeds()


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_synchronously(ort, seed):
    with CQ.GpuAdapter(ort) as ad:
        CQ.run(ad, PLAN[seed], seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_stream_ordered(ort, seed):
    with CQ.GpuAdapter(ort, stream=True) as ad:
        CQ.run(ad, PLAN[seed], seed, batch=FS.BATCH)


@pytest.mark.parametrize("a,b", list(zip(SEEDS[0::2], SEEDS[1::2])))
def test_two_contexts_in_turn(ort, a, b):
    with CQ.GpuAdapter(ort) as one, CQ.GpuAdapter(ort, stream=True) as two:
        CQ.run_in_turn([CQ.Runner(one, PLAN[a], a), CQ.Runner(two, PLAN[b], b, batch=FS.BATCH)])


@pytest.mark.parametrize("mode", ["synchronously", "stream_ordered", "beside_a_busy_context"])
def test_regression_cases(ort, mode):
    """The sequences that once failed, cut down by hand (call_sequences.REGRESSIONS; none so far), five
    times over; the third mode steps in turn with a second context that runs a generated sequence."""
    for name, case in CQ.REGRESSIONS.items():
        steps = case * 5
        with CQ.GpuAdapter(ort, stream=mode == "stream_ordered") as ad:
            mine = CQ.Runner(ad, steps, name, batch=FS.BATCH if mode == "stream_ordered" else 1)
            if mode != "beside_a_busy_context":
                mine.run()
                continue
            with CQ.GpuAdapter(ort, stream=True) as busy:
                CQ.run_in_turn([mine, CQ.Runner(busy, PLAN[SEEDS[0]][:len(steps)], SEEDS[0], batch=FS.BATCH)])


def test_the_large_tile_strides(ort):
    """The large tour's accumulation has more 16 x 16 workgroups than the statistics kernel launches."""
    (W, H), N, depth = CQ.ACC[True]
    assert ((W + 15) // 16) * ((H + 15) // 16) > 256
    with CQ.GpuAdapter(ort) as ad:
        s, t = FS.scene("d4")
        ad.upload(s, t)
        p = FS.frame_params((W, H), (N, depth), 1, "chart")
        ad.acc_begin("adaptive", p, FS.TILES["full"](W, H))
        ad.acc_pass("adaptive", 1, None, None)
        assert ad.accs["adaptive"].adaptive_stats(0.0, 0, CQ.FLOOR) == {
            "pixels": W * H, "samples": W * H, "pending": W * H, "min_count": 1, "max_count": 1}
