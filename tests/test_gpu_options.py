"""ort_set_option through the raw binding: every ORT_OPT_* of include/ort.h takes both ends of its
range, refuses the values just outside with ORT_ERR_INVALID_ARG and a message, and the special
cases answer as documented.  No scene, no kernel: a context of its own, closed at the end, so the
session renderer's options stay as they are.

The ranges are literals (the values the library has always accepted), not read from the library's
option table."""
import re
from pathlib import Path

import pytest

import octreeraytracer_amd as ort
from octreeraytracer_amd import _lib as L

pytestmark = pytest.mark.gpu

# option name -> inclusive range [lo, hi]
RANGES = {
    "FORCE_LAYOUT": (-1, 1),
    "REFILL": (1, 64),
    "SORT_PATHS": (0, 2),
    "XCD_SWIZZLE": (-1, 2),
    "KID_SKIP": (0, 2),
    "COST_ORDER": (0, 1),
    "HEAVY_FIRST": (0, 65535),
    "HEAVY_PRIO": (0, 65535),
    "SPLIT_HEAVY": (-1, 65535),
    "SPLIT_LEVEL": (0, 10),
    "TILE_PAIRS": (-1, 1),
    "LAUNCH_TIMES": (0, 1),
    "PIXEL_PATHS": (-1, 1),
    "PIXEL_LDS_SCENE": (0, 1),
    "PIXEL_HEAVY_FIRST": (-1, 1),
    "PIXEL_SPECULATE": (-1, 1),
}
# checked one by one below
SPECIAL = {"PERSISTENT", "EXACT_TRAVERSAL", "SORT_BOUND", "DEBUG_FLAGS"}
RETIRED = (5, 7, 17)


def header_options():
    """{name: id} of every `#define ORT_OPT_<NAME> <id>` in include/ort.h."""
    text = (Path(__file__).resolve().parent.parent / "include" / "ort.h").read_text()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define ORT_OPT_([A-Z0-9_]+)\s+(-?\d+)\b", text, re.M)}


@pytest.fixture(scope="module")
def setopt():
    r = ort.Renderer(0)

    def call(option, value):
        """(return code, ort_last_error after the call)"""
        rc = r._lib.ort_set_option(r._ctx, int(option), int(value))
        msg = r._lib.ort_last_error(r._ctx)
        return rc, (msg.decode() if msg else "")

    yield call
    r.close()


def test_every_header_option_is_covered():
    opts = header_options()
    assert set(opts) == set(RANGES) | SPECIAL, "include/ort.h and this test's option list differ"
    assert not set(opts.values()) & set(RETIRED)
    for name, oid in opts.items():
        assert getattr(L, "ORT_OPT_" + name) == oid, name


@pytest.mark.parametrize("name", sorted(RANGES))
def test_range_ends_and_neighbours(setopt, name):
    oid = header_options()[name]
    lo, hi = RANGES[name]
    for v in (lo, hi):
        rc, msg = setopt(oid, v)
        assert rc == L.ORT_OK, f"{name} = {v}: {rc} {msg}"
    for v in (lo - 1, hi + 1):
        rc, msg = setopt(oid, v)
        assert rc == L.ORT_ERR_INVALID_ARG, f"{name} = {v}: {rc}"
        assert msg, f"{name} = {v}: no message"


def test_persistent(setopt):
    oid = header_options()["PERSISTENT"]
    assert setopt(oid, 0)[0] == L.ORT_OK
    assert setopt(oid, 2)[0] == L.ORT_OK
    rc, msg = setopt(oid, 1)
    assert rc == L.ORT_ERR_UNSUPPORTED and msg
    for v in (-1, 3):
        rc, msg = setopt(oid, v)
        assert rc == L.ORT_ERR_INVALID_ARG and msg, v


def test_exact_traversal_takes_any_value(setopt):
    oid = header_options()["EXACT_TRAVERSAL"]
    for v in (0, 1, 7, -1):
        assert setopt(oid, v)[0] == L.ORT_OK, v
    assert setopt(oid, 0)[0] == L.ORT_OK


def test_sort_bound_has_no_upper_end(setopt):
    oid = header_options()["SORT_BOUND"]
    assert setopt(oid, 2**31 - 1)[0] == L.ORT_OK
    rc, msg = setopt(oid, -1)
    assert rc == L.ORT_ERR_INVALID_ARG and msg
    assert setopt(oid, 0)[0] == L.ORT_OK


@pytest.mark.parametrize("oid", RETIRED)
def test_retired_ids(setopt, oid):
    for v in (0, 1):
        rc, msg = setopt(oid, v)
        assert rc == L.ORT_ERR_UNSUPPORTED and msg, (oid, v)


def test_debug_flags_is_analysis_only(setopt):
    for v in (0, 1, 4):
        rc, msg = setopt(header_options()["DEBUG_FLAGS"], v)
        assert rc == L.ORT_ERR_UNSUPPORTED and msg, v


def test_unknown_option(setopt):
    rc, msg = setopt(999, 0)
    assert rc == L.ORT_ERR_INVALID_ARG and msg
