"""The material chart (tests/chart_scenes.py) on the host: the chart reaches the frame (coverage),
the kernels' per-pixel code compiled for the host (render_core.h) equals the oracle bit for bit on
it -- both layouts, both trees, brute force, with the counters -- and the ray-query set says what
it was built to say.  The reference's own shader pins the oracle on the chart in
tests/test_glsl_parity.py (the chart_* cases of canonical.json), the reference builder pins its
trees in tests/test_octree.py; tests/test_gpu_chart.py runs the HIP kernels on all of it."""
import numpy as np
import pytest

import chart_scenes as CS
from octreeraytracer_amd import _lib as L
from octreeraytracer_amd.renderer import emulate_render_host

# samples per pixel of the tests' frames at each size (tests/test_gpu_chart.py, canonical.json)
FEWEST_SAMPLES = {(96, 64): 1, (97, 63): 5, (64, 48): 1, (48, 32): 7}


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("size", CS.FRAME_SIZES)
def test_every_visible_sphere_is_reached(ort, oracle, size):
    """Every chart sphere but the three hidden ones is the first hit of at least 30 pixel-centre
    camera rays (float64 numpy, no kernel involved): at least 67 at 96x64, 65 at 97x63, 38 at
    64x48.  48x32 has 16 pixel centres on the smallest row: a frame of that size is only ever
    rendered at 7 samples per pixel (7 * 16 = 112 camera rays per sphere) or without bounces
    (max_depth <= 0 traces nothing), so there the bound holds for camera rays, not pixel centres."""
    W, H = size
    c = CS.coverage(ort, oracle, W, H)
    visible = [k for k in range(CS.N) if k not in CS.HIDDEN]
    assert (c[list(CS.HIDDEN)] == 0).all(), c
    print(f"{W}x{H}: fewest first hits {int(c[visible].min())} (sphere {visible[int(c[visible].argmin())]})")
    if size == (48, 32):
        assert (c[visible] * FEWEST_SAMPLES[size] >= CS.MIN_FIRST_HITS).all(), c
        assert (c[visible] >= 16).all(), c
    else:
        assert (c[visible] >= CS.MIN_FIRST_HITS).all(), c


def test_chart_is_what_the_table_says(ort):
    s = CS.chart(ort)
    assert s.n == 30
    assert s.center_radius[13, 3] == np.float32(-0.5) and (np.delete(s.center_radius[:, 3], 13) > 0).all()
    assert s.mat_albedo[20:26, 0].tolist() == [3.0, -1.0, np.float32(1.9), 2.5, 0.5, 7.0]
    assert np.array_equal(s.center_radius[28], s.center_radius[29]) and s.mat_albedo[28, 0] != s.mat_albedo[29, 0]
    assert s.fuzz_ri[1:7, 0].tolist() == [0.0, 0.5, 1.0, 2.0, 0.0, 0.25]
    assert s.fuzz_ri[7:12, 1].tolist() == [1.0, 0.5, 1.5, np.float32(2.4), np.float32(1 / 1.5)]
    for key, counts in CS.TREES.items():
        t = CS.scene(*key)[1]
        assert (t.n_nodes, t.n_indices) == counts, key


FRAMES = [(96, 64, 1, 1), (96, 64, 1, 2), (96, 64, 2, 8), (96, 64, 5, 6), (48, 32, 7, 3)]


@pytest.fixture(scope="module")
def oracle_frames(ort, oracle):
    """(tree key or "brute", frame) -> the oracle's (frame, counts), rendered once (the oracle's
    frame does not depend on the layout the tree is walked in)."""
    done = {}

    def get(key, frame):
        if (key, frame) not in done:
            W, H, ns, md = frame
            s, t = CS.scene(*(key if key != "brute" else (4, 1)))
            p = CS.chart_params(ort, W, H, num_samples=ns, max_depth=md, use_octree=int(key != "brute"))
            img, c = oracle.render(s, t if key != "brute" else None, p, counts=True)
            img.setflags(write=False)
            done[(key, frame)] = (img, c)
        return done[(key, frame)]

    return get


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "{}x{}_spp{}_b{}".format(*f))
@pytest.mark.parametrize("layout", [L.ORT_LAYOUT_COMPACT, L.ORT_LAYOUT_EXPLICIT], ids=["compact", "explicit"])
@pytest.mark.parametrize("key", sorted(CS.TREES), ids=lambda k: f"d{k[0]}m{k[1]}")
def test_emulation_equals_the_oracle(ort, oracle_frames, key, layout, frame):
    W, H, ns, md = frame
    s, t = CS.scene(*key)
    p = CS.chart_params(ort, W, H, num_samples=ns, max_depth=md)
    ref, rc = oracle_frames(key, frame)
    img, c = emulate_render_host(s, t, p, layout=layout)
    assert same_bits(img, ref), int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
    assert c == rc


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "{}x{}_spp{}_b{}".format(*f))
def test_emulation_equals_the_oracle_brute_force(ort, oracle_frames, frame):
    W, H, ns, md = frame
    s, _ = CS.scene(4, 1)
    p = CS.chart_params(ort, W, H, num_samples=ns, max_depth=md, use_octree=0)
    ref, rc = oracle_frames("brute", frame)
    img, c = emulate_render_host(s, None, p)
    assert same_bits(img, ref) and c == rc


@pytest.mark.parametrize("md", [0, -1])
@pytest.mark.parametrize("use_octree", [1, 0])
def test_no_bounce_frames_are_all_ones(ort, oracle, md, use_octree):
    """max_depth <= 0: radiance() returns (1, 1, 1) without tracing; oracle and emulation."""
    s, t = CS.scene(4, 1)
    p = CS.chart_params(ort, 48, 32, num_samples=3, max_depth=md, use_octree=use_octree)
    ref, rc = oracle.render(s, t if use_octree else None, p, counts=True)
    assert (ref == np.float32(1.0)).all()
    for layout in (L.ORT_LAYOUT_COMPACT, L.ORT_LAYOUT_EXPLICIT) if use_octree else (L.ORT_LAYOUT_COMPACT,):
        img, c = emulate_render_host(s, t if use_octree else None, p, layout=layout)
        assert same_bits(img, ref) and c == rc


@pytest.mark.parametrize("ns,what", [(0, "nan"), (-2, "zero")])
def test_frames_without_samples_stay_the_shaders(ort, oracle, ns, what):
    """The shader's restatements keep its answer for num_samples <= 0 (NaN for 0 / 0, +0 for a
    negative count); the device entry points refuse such a frame (tests/test_gpu_chart.py)."""
    s, t = CS.scene(4, 1)
    p = CS.chart_params(ort, 16, 8, num_samples=ns, max_depth=2)
    ref = oracle.render(s, t, p)
    img, _ = emulate_render_host(s, t, p)
    if what == "nan":
        assert np.isnan(ref).all() and np.isnan(img).all()
    else:
        assert (ref.view(np.uint32) == 0).all() and (img.view(np.uint32) == 0).all()


# ---- the ray-query set ------------------------------------------------------------------------

def test_query_rays_say_what_they_were_built_for():
    """No GPU value here: brute force reports sphere 28 and never its equal twin 29; at least 50
    rays report the negative-radius shell 13, each with a normal pointing toward its centre; the
    classes have the sizes the GPU tests count on."""
    rays, sl = CS.query_rays()
    assert sl["camera"] == slice(0, 64 * 48) and sl["shell"].stop - sl["shell"].start == CS.N_SHELL
    assert sl["second"].stop - sl["second"].start >= 1000
    s, _ = CS.scene(4, 1)
    for name in CS.QUERY_CONFIGS:
        _, (tt, sph, nrm) = CS.query_reference(name)
        assert (sph == 29).sum() == 0, name
        assert (sph == 28).sum() >= 30, name
        k13 = np.nonzero(sph == 13)[0]
        assert len(k13) >= 50, (name, len(k13))
        o, d = rays[k13, :3].astype(np.float64), rays[k13, 3:].astype(np.float64)
        outward = o + tt[k13, None].astype(np.float64) * d - s.center_radius[13, :3].astype(np.float64)
        assert ((nrm[k13].astype(np.float64) * outward).sum(-1) < 0).all(), name
        # every visible sphere is reported by the camera class (hidden ones only by later classes)
        seen = np.bincount(sph[sl["camera"]][sph[sl["camera"]] >= 0], minlength=CS.N)
        assert (seen[[k for k in range(CS.N) if k not in CS.HIDDEN]] >= CS.MIN_FIRST_HITS).all(), (name, seen)


@pytest.mark.parametrize("name", list(CS.QUERY_CONFIGS))
def test_query_emulation_equals_the_oracle(name):
    """Hit or miss and the bits of t: the host query emulation against the oracle's intersectScene."""
    ref, (tt, sph, nrm) = CS.query_reference(name)
    hit = sph >= 0
    assert np.array_equal(hit, ref[:, 0] == 1)
    assert np.array_equal(tt.view(np.int32)[hit], ref[hit, 1])
    assert (tt.view(np.int32)[~hit] == 0).all() and (nrm.view(np.int32)[~hit] == 0).all()
    assert 0.25 <= hit.mean() <= 0.9
