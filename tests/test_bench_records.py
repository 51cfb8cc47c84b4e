"""bench.py's record-keeping helpers (CPU only).

* device_sha: the hash a PMC record is keyed by covers the gfx950 code objects' instructions
  and kernel descriptors only, so the same sources built in another directory (where the
  compilation-unit id, derived from the source path, changes the code objects' symbol strings)
  hash alike, while any change of device code does not.
* sample_rows: the CPU baseline's row sample spans the whole frame height for every sample
  size (an integer stride collapsed to 1 beyond half the height and sampled the first rows only).
"""
import hashlib
import shutil
import subprocess
from pathlib import Path

import pytest

import bench

ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-w"]


def _fatbin_sha(path):
    return hashlib.sha256(bench._elf_sections(Path(path).read_bytes())[".hip_fatbin"]).hexdigest()[:16]


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_device_sha_is_build_path_independent(tmp_path):
    # the smallest HIP translation unit of the library, compiled once by a relative path from a
    # copy of the tree and once by an absolute path from another directory
    src = ROOT / "octreeraytracer_amd" / "csrc"
    a, b = tmp_path / "a", tmp_path / "b" / "deeper"
    for d in (a, b):
        shutil.copytree(src, d / "pkg" / "csrc")  # (the sources include ../../include/ort.h)
        shutil.copytree(ROOT / "include", d / "include")
    libs = []
    for d, srcpath in ((a, "pkg/csrc/group.hip"), (b, str(b / "pkg" / "csrc" / "group.hip"))):
        obj = d / "group.o"
        subprocess.run([HIPCC, *FLAGS, "-c", srcpath, "-o", str(obj)], cwd=d, check=True)
        lib = d / "libg.so"
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(lib), str(obj), "-ldl"],
                       cwd=d, check=True)
        libs.append(lib)
    assert len(bench.gfx950_code_objects(libs[0].read_bytes())) == 1
    # the whole fatbin differs (compilation-unit id), the device code does not
    assert _fatbin_sha(libs[0]) != _fatbin_sha(libs[1])
    assert bench.device_sha(libs[0]) == bench.device_sha(libs[1]) != ""
    # ... and a change of device code changes it
    (b / "pkg" / "csrc" / "group.hip").write_text((b / "pkg" / "csrc" / "group.hip").read_text().replace(
        "d[i] = s[i];", "d[i] = s[i] + 0.0f * (float)y;"))
    subprocess.run([HIPCC, *FLAGS, "-c", "pkg/csrc/group.hip", "-o", "group2.o"], cwd=b, check=True)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", "libg2.so", "group2.o", "-ldl"],
                   cwd=b, check=True)
    assert bench.device_sha(b / "libg2.so") != bench.device_sha(libs[0])


def test_device_sha_of_the_shipped_library_matches_its_code_objects():
    lib = ROOT / "octreeraytracer_amd" / "lib" / "libort.so"
    if not lib.exists():
        pytest.skip("libort.so not built")
    cos = bench.gfx950_code_objects(lib.read_bytes())
    assert len(cos) == 3  # ort_kernel.hip, gpu_build.hip, group.hip
    assert all(bench._elf_sections(co)[".text"] for co in cos)
    assert len(bench.device_sha()) == 16


@pytest.mark.parametrize("height", [7, 100, 1080, 2160, 4320])
def test_sample_rows_spans_the_frame(height):
    for n in sorted({1, 2, 3, height // 3, height // 2, height // 2 + 1, (2 * height) // 3, height - 1, height,
                     height + 5}):
        y0, rows, bh, bs = bench.sample_rows(height, n)
        ys = [y0 + (j // bh) * bs + j % bh for j in range(rows)]
        assert len(set(ys)) == rows and min(ys) >= 0 and max(ys) < height, (height, n)
        want = max(1, min(n, height))
        assert abs(rows - want) <= max(2, want // 10), (height, n, rows)  # about the asked size
        if want >= 4:  # evenly spread: rows in both the bottom and the top eighth of the frame
            assert min(ys) < height / 8 + bs and max(ys) >= height * 7 / 8 - bs, (height, n, ys[:3], ys[-3:])


@pytest.mark.parametrize("pixels,split_ok,pairs,split", [
    (3840 * 2160, True, True, False),   # full C3 frame: tile pairs
    (3840 * 1080, True, True, False),   # 1/2 band (> 2^21 px)
    (3840 * 544, True, False, True),    # 1/4 band: split walks at one frame in flight
    (3840 * 272, True, False, True),    # 1/8 band
    (3840 * 272, False, True, False),   # frames in flight: split walks off, pairs
])
def test_trace_kernel_names_follow_the_tile_rules(pixels, split_ok, pairs, split):
    """The roofline's kernel list names what render_impl launches by default (tile pairs above
    2^21 px or with split walks off, split walks at or below it)."""
    names = bench.trace_kernel_names("c3", {"tree_depth": 8, "n_nodes": 10_953_681}, 1, 1, pixels, split_ok=split_ok)
    assert names[0].startswith("ort_trace_pair<" if pairs else "ort_trace_compact<")
    assert any(n.startswith("ort_trace_split<false, 1>") for n in names) == split
    deep = bench.trace_kernel_names("c5", {"tree_depth": 10, "n_nodes": 239_220_401}, 4, 1, 7680 * 4320)
    assert deep[0].startswith("ort_trace_pair_deep<false, 2>") and deep[-1].startswith("ort_trace_persistent<false, true>")
    # the reference's default config (a 585-node tree, 16 x 8): whole-pixel paths, one kernel
    small = bench.trace_kernel_names("ref_default", {"tree_depth": 3, "n_nodes": 585}, 8, 16, 800 * 600)
    assert len(small) == 3 and small[0].startswith("ort_pixel_paths<0, false, ..., 1>")  # samples in parallel
    assert small[1].startswith("ort_sample_resolve") and small[2].startswith("ort_pixel_paths<0, false, ..., 2>")
    one = bench.trace_kernel_names("c2", {"tree_depth": 6, "n_nodes": 209_000}, 4, 1, 1920 * 1080)
    assert one == [one[0]] and one[0].startswith("ort_pixel_paths<0, false>")  # one sample: whole pixels


def test_dump_outputs_whole_frame_and_seeded_sample(tmp_path):
    """--dump-outputs: a frame within the size limit is written whole; a larger one as the same
    seeded pixel sample in every run, with the pixels' flat indices, within the limit in all."""
    import numpy as np
    small = np.arange(5 * 7 * 3, dtype=np.float32).reshape(5, 7, 3)
    bench.dump_outputs(str(tmp_path / "s"), small)
    got = np.load(tmp_path / "s" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    assert not (tmp_path / "s" / "frame_index.npy").exists()
    h, w = 2401, 2399  # 69 MB of float32 RGB: above the limit, odd sizes
    big = np.arange(h * w * 3, dtype=np.float32).reshape(h, w, 3)  # (exact below 2^24 only: compared to itself)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    idx = np.load(tmp_path / "a" / "frame_index.npy")
    px = np.load(tmp_path / "a" / "frame.npy")
    assert idx.dtype == np.float64 and px.dtype == np.float32 and px.shape == (len(idx), 3)
    i = idx.astype(np.int64)
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < h * w and np.array_equal(i.astype(np.float64), idx)
    assert np.array_equal(px, big.reshape(-1, 3)[i])
    assert len(i) > 3_000_000  # most of what the limit allows
    files = [tmp_path / "a" / n for n in ("frame.npy", "frame_index.npy")]
    assert sum(f.stat().st_size for f in files) <= 64_000_000
    for f in files:  # the same sample, byte for byte, in a second run
        assert f.read_bytes() == (tmp_path / "b" / f.name).read_bytes()


def test_plain_line_is_lean_and_full_adds_the_rest(tmp_path, monkeypatch, capsys):
    """A plain run prints the headline keys only and, with --dump-outputs, writes the last step's
    frame; --full adds the frame check (here through --emulate: the host build of the kernel code)."""
    import json
    import sys

    import numpy as np
    import octreeraytracer_amd as ort
    from oracle import oracle
    lines = {}
    for extra in ([], ["--full"]):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--emulate", "--config", "c1", "--steps", "2",
                                          "--warmup", "0", "--dump-outputs", str(tmp_path / "out")] + extra)
        bench.main()
        lines[bool(extra)] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for line in lines.values():
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "Mrays/s" and line["dtype"] == "f32"
        assert line["higher_is_better"] is True and line["value"] > 0
    assert "parity" not in lines[False] and lines[True]["parity"]["bit_identical"]
    s = ort.random_spheres(100, 42)
    ref = oracle.render(s, ort.build_octree(s, 4, 0), ort.FrameParams.default_camera(256, 256))
    got = np.load(tmp_path / "out" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
