"""Adaptive accumulations on the GPU (ORT_ACCUM_ADAPTIVE, Accumulation.step_adaptive): after every
pass the counts, the moments and the preview are the host emulation's (ort_debug_emulate_adaptive,
which tests/test_adaptive.py ties to the numpy restatement), bit for bit, on the four walk variants
of the whole-pixel kernel, a holed tile and a band tile past the frame.  Driven without a criterion
an adaptive accumulation is a moments accumulation, and its finished frame has the reference
shader's SHA-256.  Outputs, options, isolation, state changes, refusals and the rest loop follow."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import adaptive_sets as A
from adaptive_sets import FLOOR
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.image import to_srgb8
from octreeraytracer_amd.renderer import accum_adaptive_host, accum_moments_host, denoise_host, gamma_host
from test_glsl_parity import frame_sha
from test_gpu_accum import case, same_bits, turned

pytestmark = pytest.mark.gpu

F = np.float32
THR, MIN = 0.05, 2
BAND = (16, 50, 5, 48, 16, 32)  # rows 5-20, 37-52, 69-84 of 63 (the last band: padding)
# key: (case, N, tile, the passes' n_samples) -- criterion: threshold 0.05, floor 0.05, min_samples 2
RUNS = {
    "lds": ("chart_spp7_b3", 16, None, (1,) * 16),
    "global": ("chart_d6m0_spp2_b4", 9, None, (2, 1, 3, 1, 2)),          # 181 k nodes: the compact walk from global memory
    "deep": ("deep_d9_m1_spp2_b3", 9, (112, 64, 60, 48, 0, 0), (2, 1, 3, 1, 2)),  # depth 9: DEEP, a tile at an offset
    "brute": ("chart_brute_spp2_b6", 9, None, (1,) * 9),
    "holed": ("chart_odd_spp5_b6", 16, None, (2, 3, 4, 7)),               # 97 x 63: hole slots
    "band": ("chart_odd_spp5_b6", 16, BAND, (1, 1, 2, 3, 4, 5)),
}


def passes_of(key, threshold=THR, min_samples=MIN):
    return [(n, min_samples, threshold, FLOOR) for n in RUNS[key][3]]


def setup(key):
    name, N, tile, _ = RUNS[key]
    return A.scene(name, N, tile)[:4] + (case(name)[2],)


@functools.lru_cache(maxsize=None)
def want(key, i, threshold=THR, min_samples=MIN):
    """The emulation after passes 0 .. i of the run: (counts, mean, variance), read-only."""
    s, tree, p, tile, _ = setup(key)
    out = accum_adaptive_host(s, tree, p, tile, passes=passes_of(key, threshold, min_samples)[:i + 1])
    for a in out:
        a.setflags(write=False)
    return out


def picture(mean, inside, fmt="rgb32f"):
    """The preview of a linear mean: its gamma, zeros in the rows past the frame."""
    pic = gamma_host(mean)
    pic[~np.broadcast_to(inside, pic.shape[:2])] = 0
    if fmt == "rgb32f":
        return pic
    out = np.zeros(pic.shape[:2] + (4,), np.uint8)
    out[..., :3] = to_srgb8(pic)
    out[..., 3] = 255
    out[~np.broadcast_to(inside, pic.shape[:2])] = 0
    return out


def check_state(acc, w, what):
    counts, (mean, var) = acc.counts(), acc.moments()
    assert np.array_equal(counts, w[0]), f"{what}: counts"
    assert same_bits(mean, w[1]) and same_bits(var, w[2]), f"{what}: moments"


# ---- 1. every pass is the emulation's ----------------------------------------------------------
@pytest.mark.parametrize("key", sorted(RUNS))
def test_every_pass_is_the_emulation(ort, key):
    s, tree, p, tile, t = setup(key)
    inside = A.in_frame(tile, p)
    passes = passes_of(key)
    N = p.num_samples
    slots = ((tile.width + 15) // 16) * ((tile.rows + 15) // 16) * 256
    with ort.Renderer(0) as r:
        r.upload(s, t)
        with r.accumulate(p, tile, adaptive=True) as acc:
            assert acc.is_adaptive and acc.keeps_moments and acc.info()["device_bytes"] == 28 * slots + 64
            assert (acc.counts() == 0).all()
            st = acc.adaptive_stats(THR, MIN, FLOOR)
            assert (st["pixels"], st["samples"], st["pending"]) == (int(inside.sum()) * tile.width, 0, st["pixels"])
            done = 0
            for i, (n, *_) in enumerate(passes):
                fmt = "rgba8" if i % 2 else "rgb32f"
                pic = acc.step_adaptive(n, THR, MIN, FLOOR, format=fmt)
                done = min(N, done + n)
                w = want(key, i)
                what = f"{key} after pass {i} ({n} samples)"
                assert acc.done == done and acc.finished == (done == N), what
                check_state(acc, w, what)
                assert np.array_equal(pic, picture(w[1], inside, fmt)) and pic.dtype == (np.uint8 if i % 2 else F), what
                if fmt == "rgb32f":
                    assert same_bits(pic, picture(w[1], inside)), what
                st = acc.adaptive_stats(THR, MIN, FLOOR)
                at = np.broadcast_to(inside, w[0].shape)
                nxt = accum_adaptive_host(s, tree, p, tile, passes=passes[:i + 1] + [(1, MIN, THR, FLOOR)])[0]
                assert st == {"pixels": int(at.sum()), "samples": int(w[0][at].sum()), "pending": int((nxt != w[0]).sum()),
                              "min_count": int(w[0][at].min()), "max_count": int(w[0][at].max())}, what
                assert acc.adaptive_stats(0.0, 0, FLOOR)["pending"] == int((w[0][at] < N).sum()), what
            hist = np.bincount(w[0][at], minlength=N + 1)
            print(key, "counts 0..N:", " ".join(map(str, hist)))
            assert hist[2:N].sum() > 0 and hist[N] > 0, "the run holds pixels and finishes others"


# ---- 2. without a criterion it is a moments accumulation -----------------------------------------
@pytest.mark.parametrize("name,split", [("chart_spp7_b3", (2, 2, 3)), ("chart_spp7_b3", (1,) * 7), ("chart_d6m0_spp2_b4", (1, 1)),
                                        ("deep_d9_m1_spp2_b3", (1, 1)), ("chart_brute_spp2_b6", (1, 1)),
                                        ("chart_odd_spp5_b6", (1, 4))])
def test_threshold_zero_and_step_alone_are_a_moments_accumulation(ort, name, split):
    c, s, t, p = case(name)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        with r.accumulate(p, moments=True) as ref, r.accumulate(p, adaptive=True) as a, r.accumulate(p, adaptive=True) as b:
            for n in split:
                pic = ref.step(n)
                assert same_bits(a.step(n), pic) and same_bits(b.step_adaptive(n, 0.0, 0, FLOOR), pic), (name, ref.done)
                assert a.done == b.done == ref.done
                m, v = ref.moments()
                for acc in (a, b):
                    am, av = acc.moments()
                    assert same_bits(am, m) and same_bits(av, v) and (acc.counts() == ref.done).all(), (name, ref.done)
            assert frame_sha(pic) == c["sha256"] and a.finished and b.finished
            for acc in (a, b):  # finished: the frame again (a pass that holds every pixel), and nothing moves
                assert frame_sha(acc.step(1)) == c["sha256"]
                assert np.array_equal(acc.step_adaptive(3, THR, MIN, FLOOR, format="rgba8"), ref.step(1, format="rgba8"))
                assert acc.step(1, out=False) is None and (acc.counts() == p.num_samples).all()
                assert acc.adaptive_stats(0.0, 0, FLOOR)["pending"] == 0


def test_held_pixels_keep_their_state(ort):
    """chart_spp7_b3 at its own N = 7: three adaptive passes hold most of the picture; the held
    pixels' counts and moments are the same before and after each pass, and step(7) then brings
    every pixel to N from whatever state it was held in -- the reference shader's frame, so the
    held pixels' RNG states and sums were the uniform chain's."""
    c, s, t, p = case("chart_spp7_b3")
    with ort.Renderer(0) as r:
        r.upload(s, t)
        with r.accumulate(p, adaptive=True) as acc:
            acc.step_adaptive(2, THR, MIN, FLOOR, out=False)
            for _ in range(3):
                c0, (m0, v0) = acc.counts(), acc.moments()
                acc.step_adaptive(1, THR, MIN, FLOOR, out=False)
                c1, (m1, v1) = acc.counts(), acc.moments()
                held = c1 == c0
                assert held.any() and not held.all()
                assert same_bits(m1[held], m0[held]) and same_bits(v1[held], v0[held])
            assert len(np.unique(c1)) >= 3 and acc.done == 5
            assert frame_sha(acc.step(7)) == c["sha256"] and (acc.counts() == 7).all()
            m, v = acc.moments()
            wm, wv = accum_moments_host(s, t, p, samples_done=7)
            assert same_bits(m, wm) and same_bits(v, wv)


@pytest.mark.parametrize("option", ["lds_scene_off", "kid_skip_off", "exact_traversal"])
def test_options_switched_mid_accumulation(ort, option):
    s, tree, p, tile, t = setup("lds")
    with ort.Renderer(0) as r:
        r.upload(s, t)
        with r.accumulate(p, adaptive=True) as acc:
            for i in range(8):
                if i == 3:
                    if option == "lds_scene_off":
                        r.set_pixel_lds_scene(0)
                    elif option == "kid_skip_off":
                        r.set_kid_skip(0)
                    else:
                        r.set_exact_traversal(True)
                acc.step_adaptive(1, THR, MIN, FLOOR, out=False)
                if i in (2, 4, 7):
                    check_state(acc, want("lds", i), f"{option} after pass {i}")


# ---- 3. outputs ----------------------------------------------------------------------------------
def test_device_outputs_stream_pitch_and_frame_placement(ort):
    import torch
    s, tree, p, tile, t = setup("band")
    inside = A.in_frame(tile, p)
    W, H = p.width, p.height
    ys = tile.pixel_rows(H)
    FILL = 0xA5
    with ort.Renderer(0) as r:
        r.upload(s, t)
        with r.accumulate(p, tile, adaptive=True) as acc:
            stream = torch.cuda.Stream(device="cuda:0")
            assert acc.step_adaptive(1, THR, MIN, FLOOR, out=False, stream=stream.cuda_stream) is None   # pass 0, no picture
            dev = torch.full((tile.rows + 1, tile.width, 3), -7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            assert acc.step_adaptive(1, THR, MIN, FLOOR, out=dev, stream=stream.cuda_stream) is dev       # pass 1: device, a stream
            dcounts = torch.full((tile.rows + 1, tile.width), -7, dtype=torch.int32, device="cuda:0")
            assert acc.counts(out=dcounts, stream=stream.cuda_stream) is dcounts
            stream.synchronize()
            w = want("band", 1)
            got = dev.cpu().numpy()
            assert same_bits(got[:tile.rows], picture(w[1], inside)) and (got[tile.rows:] == -7.0).all()
            got = dcounts.cpu().numpy()
            assert np.array_equal(got[:tile.rows], w[0]) and (got[tile.rows:] == -7).all()
            for i, fmt in ((2, "rgb32f"), (3, "rgba8")):                                                   # passes 2, 3: pitched
                bpp = L.FORMAT_BPP[L.FORMATS[fmt]]
                pitch = (tile.width + 3) * bpp
                buf = torch.full((tile.rows * pitch,), FILL, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                acc.step_adaptive(RUNS["band"][3][i], THR, MIN, FLOOR, out=buf.view(torch.float32) if fmt == "rgb32f" else buf,
                                  format=fmt, row_pitch=pitch)
                torch.cuda.synchronize()
                rows = buf.cpu().numpy().reshape(tile.rows, pitch)
                tight = picture(want("band", i)[1], inside, fmt).view(np.uint8).reshape(tile.rows, tile.width * bpp)
                assert np.array_equal(rows[:, :tile.width * bpp], tight) and (rows[:, tile.width * bpp:] == FILL).all(), fmt
            frame = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")                      # pass 4: frame placement
            torch.cuda.synchronize()
            acc.step_adaptive(RUNS["band"][3][4], THR, MIN, FLOOR, out=frame, place="frame")
            torch.cuda.synchronize()
            expect = np.full((H, W, 3), -1.0, F)
            expect[ys[ys < H], tile.x0:tile.x0 + tile.width] = picture(want("band", 4)[1], inside)[ys < H]
            assert same_bits(frame.cpu().numpy(), expect)
            check_state(acc, want("band", 4), "after the five outputs")


# ---- 4. isolation and state changes ----------------------------------------------------------------
def test_isolation_device_bytes_restart_and_scene_change(ort):
    s, tree, p, tile, t = setup("lds")
    c = case("chart_spp7_b3")[0]
    p7 = dataclasses.replace(p, num_samples=7)
    slots = ((p.width + 15) // 16) * ((p.height + 15) // 16) * 256
    rays = np.zeros((4, 6), F)
    rays[:, 2], rays[:, 5] = 5.0, -1.0
    with ort.Renderer(0) as r:
        r.upload(s, t)
        with r.accumulate(p, adaptive=True) as acc, r.accumulate(p7) as plain, r.accumulate(p7, moments=True) as mom, \
                r.accumulate(p, adaptive=True) as twin:
            assert acc.info()["device_bytes"] == 28 * slots + 64
            assert mom.info()["device_bytes"] == 24 * slots + 64 and plain.info()["device_bytes"] == 20 * slots + 64
            frames = []
            for i in range(6):  # frames, queries and other accumulations between the passes
                acc.step_adaptive(1, THR, MIN, FLOOR, out=False)
                if i % 2 == 0:
                    plain.step(1, out=False)
                    mom.step(2, out=False)
                    frames.append(r.render(p7))
                    r.trace_rays(rays)
                    twin.step_adaptive(3, 0.1, 0, FLOOR, out=False)
                check_state(acc, want("lds", i), f"interleaved, pass {i}")
            assert all(frame_sha(f) == c["sha256"] for f in frames)
            assert frame_sha(plain.step(4)) == c["sha256"] and frame_sha(mom.step(1)) == c["sha256"]
            solo = accum_adaptive_host(s, tree, p, passes=[(3, 0, 0.1, FLOOR)] * 3)
            check_state(twin, solo, "the other adaptive accumulation")
            staged = acc.info()["device_bytes"]
            assert staged > 28 * slots + 64  # host staging counts
            # restart: counts back to 0 with the sums, nothing allocated, passes queued behind it
            p2 = turned(p, c, 20.0)
            acc.step_adaptive(1, THR, MIN, FLOOR, out=False)
            acc.restart(p2)
            assert acc.done == 0 and (acc.counts() == 0).all() and acc.info()["device_bytes"] == staged
            with pytest.raises(ort.OrtError) as e:
                acc.moments()
            assert e.value.code == L.ORT_ERR_INVALID_ARG
            crit = [(2, MIN, THR, FLOOR), (1, MIN, THR, FLOOR), (1, MIN, THR, FLOOR)]
            for n, *_ in crit:
                acc.step_adaptive(n, THR, MIN, FLOOR, out=False)
            check_state(acc, accum_adaptive_host(s, tree, p2, passes=crit), "after a restart")
            assert len(np.unique(acc.counts())) >= 2
            # a scene change invalidates, a restart revives
            r.upload(s, t)
            keep = np.full((p.height, p.width), -7, np.int32)
            for call in (lambda: acc.step_adaptive(1, THR, MIN, FLOOR), lambda: acc.counts(out=keep),
                         lambda: acc.adaptive_stats(THR, MIN, FLOOR), lambda: acc.moments()):
                with pytest.raises(ort.OrtError) as e:
                    call()
                assert e.value.code == L.ORT_ERR_NO_SCENE
            assert (keep == -7).all()
            acc.restart(p)
            for i in range(3):
                acc.step_adaptive(1, THR, MIN, FLOOR, out=False)
            check_state(acc, want("lds", 2), "after a scene change and a restart")


# ---- 5. refusals -----------------------------------------------------------------------------------
def test_refusals_leave_counts_and_outputs_untouched(ort):
    s, tree, p, tile, t = setup("lds")
    n = p.width * p.height
    with ort.Renderer(0) as r, ort.Renderer(0) as other:
        r.upload(s, t)
        other.upload(s, t)
        with r.accumulate(p, adaptive=True) as acc, r.accumulate(p, moments=True) as mom, \
                r.accumulate(p, ort.Tile(0, 0, 0, 0), adaptive=True) as empty:
            for i in range(3):
                acc.step_adaptive(1, THR, MIN, FLOOR, out=False)
            mom.step(3, out=False)
            lib = r._lib
            out = np.full((p.height, p.width, 3), F(-3.0))
            counts = np.full(n + 1, -7, np.int32)
            st = L.OrtAccumAdaptiveStats()
            st.pending = -7

            def crit(n_samples=1, min_samples=0, threshold=THR, floor=FLOOR, reserved=None):
                a = L.OrtAccumAdaptive(n_samples, min_samples, threshold, floor)
                if reserved is not None:
                    a.reserved[reserved] = 1
                return a

            def output(**kw):
                o = L.OrtOutput(out.ctypes.data, 0, L.ORT_FORMAT_RGB32F, L.ORT_PLACE_TILE, 0, 0)
                for k, v in kw.items():
                    setattr(o, k, v)
                return o

            def render(ctx=r, h=acc._h, a=crit(), o=output()):
                return lib.ort_accum_render_adaptive(ctx._ctx if ctx else None, h, C.byref(a) if a else None,
                                                     C.byref(o) if o else None, None)

            def stats(ctx=r, h=acc._h, a=crit(), res=st):
                return lib.ort_accum_adaptive_stats(ctx._ctx if ctx else None, h, C.byref(a) if a else None,
                                                    C.byref(res) if res else None)

            def read(ctx=r, h=acc._h, ptr=counts.ctypes.data):
                return lib.ort_accum_read_counts(ctx._ctx if ctx else None, h, ptr, 0, None)

            bad = [crit(n_samples=0), crit(n_samples=-1), crit(min_samples=-1), crit(threshold=-0.5), crit(threshold=float("nan")),
                   crit(floor=0.0), crit(floor=-1.0), crit(floor=float("inf")), crit(floor=float("nan"))] + \
                  [crit(reserved=i) for i in range(4)]
            for a in bad:
                assert render(a=a) == L.ORT_ERR_INVALID_ARG and stats(a=a) == L.ORT_ERR_INVALID_ARG
            for kw in (dict(ctx=None), dict(h=None), dict(a=None), dict(h=mom._h), dict(ctx=other)):
                assert render(**kw) == L.ORT_ERR_INVALID_ARG, kw
                assert stats(**kw) == L.ORT_ERR_INVALID_ARG, kw
            assert stats(res=None) == L.ORT_ERR_INVALID_ARG
            for o in (output(format=2), output(placement=2), output(reserved=1), output(row_pitch_bytes=8), output(data=None)):
                assert render(o=o) == L.ORT_ERR_INVALID_ARG             # an output ort_render_ex refuses
            for kw in (dict(ctx=None), dict(h=None), dict(ptr=None), dict(h=mom._h), dict(ctx=other),
                       dict(ptr=counts.ctypes.data + 2)):
                assert read(**kw) == L.ORT_ERR_INVALID_ARG, kw
            assert lib.ort_accum_render(r._ctx, acc._h, 0, None, None) == L.ORT_ERR_INVALID_ARG
            assert (out == F(-3.0)).all() and (counts == -7).all() and st.pending == -7
            assert acc.done == 3
            check_state(acc, want("lds", 2), "after the refusals")
            assert render(a=crit(threshold=float("inf"))) == L.ORT_OK and not (out == F(-3.0)).any()   # +inf is valid
            check_state(acc, accum_adaptive_host(s, tree, p, passes=passes_of("lds")[:3] + [(1, 0, float("inf"), FLOOR)]),
                        "threshold +inf: whatever has an estimate is held")
            # the flag is bit 2: bit 1 and bit 3 stay unknown bits, and it may come with ORT_ACCUM_MOMENTS
            assert L.ORT_ACCUM_ADAPTIVE == 4
            pc, tc = p.to_c(), ort.Tile.full(p).to_c()
            for flags, code in ((2, L.ORT_ERR_INVALID_ARG), (8, L.ORT_ERR_INVALID_ARG), (4 | 2, L.ORT_ERR_INVALID_ARG), (4 | 1, L.ORT_OK)):
                h = C.c_void_p()
                assert lib.ort_accum_begin_ex(r._ctx, C.byref(pc), C.byref(tc), flags, C.byref(h)) == code, flags
                if code == L.ORT_OK:
                    assert lib.ort_accum_read_counts(r._ctx, h, counts.ctypes.data, 0, None) == L.ORT_OK and (counts[:n] == 0).all()
                    counts[:] = -7
                    assert lib.ort_accum_free(r._ctx, h) == L.ORT_OK
                else:
                    assert not h.value
            # a tile of no pixels: valid, launches nothing, writes nothing
            empty.step_adaptive(2, THR, MIN, FLOOR, out=False)
            assert empty.done == 2 and read(h=empty._h) == L.ORT_OK and (counts == -7).all()
            assert empty.adaptive_stats(THR, MIN, FLOOR) == {"pixels": 0, "samples": 0, "pending": 0, "min_count": 0, "max_count": 0}
            assert read() == L.ORT_OK and (counts[:n] >= 2).all() and counts[n] == -7


# ---- 6. the rest loop end to end -------------------------------------------------------------------
def test_rest_loop_end_to_end(ort):
    """config_default at a reduced size: adaptive passes of one sample under the wrappers' defaults
    until nothing is pending, then the variance-guided denoise with gamma of the mean, on the device,
    against the emulation's counts, mean and variance through denoise_host."""
    import torch
    from octreeraytracer_amd.renderer import (DEFAULT_ADAPTIVE_LUMINANCE_FLOOR, DEFAULT_ADAPTIVE_MIN_SAMPLES,
                                               DEFAULT_ADAPTIVE_THRESHOLD)
    c, s, t, p0 = case("config_default")
    p = dataclasses.replace(p0, width=96, height=54, num_samples=16)
    tree = t if c["oct"] else None
    crit = (1, DEFAULT_ADAPTIVE_MIN_SAMPLES, DEFAULT_ADAPTIVE_THRESHOLD, DEFAULT_ADAPTIVE_LUMINANCE_FLOOR)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        with r.accumulate(p, adaptive=True) as acc:
            hits, nrm = acc.guides()
            passes = 0
            while acc.adaptive_stats()["pending"]:
                acc.step_adaptive(1, out=False)
                passes += 1
                assert passes <= 16
            st = acc.adaptive_stats()
            wc, wm, wv = accum_adaptive_host(s, tree, p, passes=[crit] * passes)
            assert np.array_equal(acc.counts(), wc) and st["samples"] == int(wc.sum()) < 16 * wc.size
            assert (st["min_count"], st["max_count"]) == (int(wc.min()), int(wc.max())) and st["min_count"] >= crit[1]
            more = accum_adaptive_host(s, tree, p, passes=[crit] * (passes + 1))[0]
            assert np.array_equal(more, wc), "pending == 0: another pass would trace nothing"
            mean, var = acc.moments(out_mean=torch.empty((54, 96, 3), device="cuda:0"),
                                    out_variance=torch.empty((54, 96), device="cuda:0"))
            got = r.denoise(mean, (hits, nrm), variance=var, gamma=True)
            torch.cuda.synchronize()
            assert same_bits(mean.cpu().numpy(), wm) and same_bits(var.cpu().numpy(), wv)
            guides = (hits.cpu().numpy(), nrm.cpu().numpy())
            assert same_bits(got.cpu().numpy(), denoise_host(wm, guides, variance=wv, gamma=True))
            print(f"rest loop: {passes} passes, {st['samples']} of {16 * wc.size} samples, counts {st['min_count']}..{st['max_count']}")


def test_restart_does_not_wait(ort):
    """A long pass is queued on a caller's stream and restart is called behind it: the pass is still
    pending when restart returns (restart neither waits nor launches), the counts read 0 at once,
    nothing is allocated, and the passes queued after it on the same stream give the state of a fresh
    accumulation of the new pose driven by the same passes, bit for bit."""
    import torch
    c, s, t, p0 = case("config_default")
    p = dataclasses.replace(p0, width=1920, height=1080, num_samples=64)   # 64 samples of 2 M pixels: tens of ms
    p2 = turned(p, c, 20.0)
    with ort.Renderer(0) as r:
        r.upload(s, t)
        with r.accumulate(p, adaptive=True) as acc, r.accumulate(p2, adaptive=True) as fresh:
            acc.step_adaptive(4, THR, MIN, FLOOR, out=False)
            acc.step_adaptive(1, THR, MIN, FLOOR, out=False)               # (a list pass: the list is allocated)
            assert len(np.unique(acc.counts())) == 2
            before = acc.info()["device_bytes"]
            stream = torch.cuda.Stream(device="cuda:0")
            torch.cuda.synchronize()
            acc.step(64, out=False, stream=stream.cuda_stream)
            acc.restart(p2)
            pending = not stream.query()
            assert pending, "the queued pass had finished when restart returned: restart waited (or the pass is too short)"
            assert acc.done == 0 and (acc.counts() == 0).all() and acc.info()["device_bytes"] == before
            assert acc.adaptive_stats(THR, MIN, FLOOR)["pending"] == p.width * p.height
            for n in (2, 1, 1):                                            # behind the old pass, on its stream
                acc.step_adaptive(n, THR, MIN, FLOOR, out=False, stream=stream.cuda_stream)
                fresh.step_adaptive(n, THR, MIN, FLOOR, out=False)
            stream.synchronize()
            counts = acc.counts()
            assert np.array_equal(counts, fresh.counts()) and len(np.unique(counts)) >= 2 and counts.max() == 4
            (m, v), (fm, fv) = acc.moments(), fresh.moments()
            assert same_bits(m, fm) and same_bits(v, fv)
