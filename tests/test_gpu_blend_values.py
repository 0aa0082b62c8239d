"""The blend kernels at the ends of the value range: frames of 0 and 255 (blend_ref.PATTERNS) on
small translation rigs (blend_ref.CASES), against the NumPy restatement of the specification
(blend_ref.blend_ref; held against oracle/orc_blend.c by test_blend_ref_cpu.py), and on one
rotated rig against the oracle.  Bar: max |diff| == 0.

The frames of every other blend test come from rig.texture (bytes within 2..238): their
multi-band results never reach the final clamp and no pyramid level its largest value, so the
headroom the kernels' packed and 24-/32-bit arithmetic relies on is never used.  Here it is:
test_blend_ref_cpu.py asserts the shares of clamped values and the level maxima on the same
frames.

Paths: the prepared multi-band by the band pass (+ mb_levels under 128 px) and by the sweep, the
direct multi-band, the prepared and the direct feather.  Device results come back from
sentinel-filled buffers (test_gpu_direct_multiband._stitch).
"""
import functools
import time

import pytest

from blend_ref import (CASES, FEATHER, MULTIBAND, PATTERNS, ROTATED, blend_ref, make_plan,
                       pattern_frames)
from conftest import check_mb_path
from oracle import oracle
from test_gpu_direct_multiband import _diff, _stitch

pytestmark = pytest.mark.gpu

ALL = dict(CASES, ROT=ROTATED)
# the cases the sweep takes: at most 3 channels, at least 128 px a side
SWEEP = ["T2c1", "T2c3", "T6", "ROT"]
GRID = [(c, p) for c in ALL for p in PATTERNS]
GRID_SWEEP = [(c, p) for c in SWEEP for p in PATTERNS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from multicamera_stitching_amd import _capi
    assert _capi.device_count() >= 1, "GPU tests need an MI355X (no HIP device visible)"


def _plan(case, blend, sweep=None, monkeypatch=None):
    """A plan of the case; sweep (True / False): prepared with MCS_MB_SWEEP set to it."""
    c = dict(case if isinstance(case, dict) else ALL[case])
    plan = make_plan(blend=blend, **c)
    if sweep is not None:
        monkeypatch.setenv("MCS_MB_SWEEP", "1" if sweep else "0")
        plan.prepare()
    return plan


@functools.lru_cache(maxsize=None)
def _want(case, pattern, mode):
    """The reference mosaic, computed once: the restatement, the oracle on the rotated case."""
    plan = make_plan(**ALL[case])
    flat = plan.describe()
    plan.close()
    frames = pattern_frames(ALL[case], pattern)
    if case == "ROT":
        want = oracle.blend_stitch(flat, frames, mode)
    else:
        want = blend_ref(flat, frames, mode)[0]
    want.setflags(write=False)
    return want


def _check(got, case, pattern, mode, path):
    d = _diff(got, _want(case, pattern, mode))
    print(f"{path}: {case} {pattern}: max |diff| {d}")
    assert d == 0, (path, case, pattern, d)


def _banded(plan):
    return min(plan.out_w, plan.out_h) >= 128


# ---- every case x pattern through every path -----------------------------------------------------
@pytest.mark.parametrize("case, pattern", GRID)
def test_prepared_band_pass(case, pattern, monkeypatch):
    plan = _plan(case, MULTIBAND, False, monkeypatch)
    got = _stitch(plan, [pattern_frames(ALL[case], pattern)], "stitch_device")[0]
    st = plan.stats()
    check_mb_path(st, "bands")
    assert st["blend"] == MULTIBAND and st["blend_tiles"] > 0
    assert (st["mb_bands"] > 0) == _banded(plan), st
    _check(got, case, pattern, MULTIBAND,
           f"prepared multi-band, band pass ({st['mb_bands']} bands, {st['mb_bands_lds']} on the "
           f"LDS ring)")
    plan.close()


@pytest.mark.parametrize("case, pattern", GRID_SWEEP)
def test_prepared_sweep(case, pattern, monkeypatch):
    plan = _plan(case, MULTIBAND, True, monkeypatch)
    got = _stitch(plan, [pattern_frames(ALL[case], pattern)], "stitch_device")[0]
    st = plan.stats()
    check_mb_path(st, "sweep")
    assert st["mb_sweep_strips"] > 0, st
    _check(got, case, pattern, MULTIBAND, "prepared multi-band, sweep")
    plan.close()


@pytest.mark.parametrize("case, pattern", GRID)
def test_direct_multiband(case, pattern):
    plan = _plan(case, MULTIBAND)
    got = _stitch(plan, [pattern_frames(ALL[case], pattern)])[0]
    assert not plan.stats()["prepared"]
    _check(got, case, pattern, MULTIBAND, "direct multi-band")
    plan.close()


@pytest.mark.parametrize("case, pattern", GRID)
def test_feather_prepared_and_direct(case, pattern):
    plan = _plan(case, FEATHER)
    frames = pattern_frames(ALL[case], pattern)
    _check(_stitch(plan, [frames], "stitch_direct")[0], case, pattern, FEATHER, "direct feather")
    assert not plan.stats()["prepared"]
    _check(_stitch(plan, [frames], "stitch_device")[0], case, pattern, FEATHER,
           "prepared feather")
    st = plan.stats()
    assert st["prepared"] and st["blend"] == FEATHER and st["blend_tiles"] > 0
    plan.close()


# ---- one launch of captures that differ in kind --------------------------------------------------
MIXED = ["bits", "flat255", "alt0_255", "noise"]


@pytest.mark.parametrize("path", ["bands", "sweep", "direct-multiband", "direct-feather"])
@pytest.mark.parametrize("case", ["T2c3", "T3"])
def test_one_launch_of_different_captures(case, path, monkeypatch):
    """Four captures of four patterns in one launch, each equal to its own reference: a value the
    compiler (or the code) keeps across the capture loop shows here and nowhere else -- every
    other batched test rolls one frame set."""
    if path == "sweep" and case not in SWEEP:
        plan = _plan(case, MULTIBAND, True, monkeypatch)      # not taken: the band pass again
        assert plan.stats()["mb_sweep_strips"] == 0
    elif path in ("bands", "sweep"):
        plan = _plan(case, MULTIBAND, path == "sweep", monkeypatch)
        check_mb_path(plan.stats(), path)
    else:
        plan = _plan(case, MULTIBAND if path == "direct-multiband" else FEATHER)
    method = {"bands": "stitch_device", "sweep": "stitch_device",
              "direct-multiband": "stitch_direct_multiband", "direct-feather": "stitch_direct"}
    mode = FEATHER if path == "direct-feather" else MULTIBAND
    got = _stitch(plan, [pattern_frames(ALL[case], p) for p in MIXED], method[path])
    for f, p in enumerate(MIXED):
        _check(got[f], case, p, mode, f"{path}, capture {f} of {len(MIXED)}")
    plan.close()


# ---- the LDS-ring form of the band pass ----------------------------------------------------------
# The smallest such rig, found by stepping down from 4 x 1920x1080 on an MI355X.  A band takes the
# ring only when its camera's rows are a multiple of 4 bytes and at least 256 long (mcs_prepare.cpp
# band_lds_tables): 88 px at 3 channels, and 84 px gave none.  At that width plans of 143 rows and
# more reported ring bands (2 of the 6 bands of this 140 x 143 mosaic), plans of 142 and fewer none.
RING = dict(n=2, w=88, h=143, ch=3, step=52)


def test_band_pass_lds_ring(monkeypatch):
    """A plan with some bands on the LDS ring and the others on global windows, flat255 and bits
    in one launch of two captures."""
    plan = _plan(RING, MULTIBAND, False, monkeypatch)
    flat = plan.describe()
    batch = [pattern_frames(RING, p) for p in ("flat255", "bits")]
    got = _stitch(plan, batch, "stitch_device")
    st = plan.stats()
    print(f"ring rig {RING}: mosaic {plan.out_w} x {plan.out_h}, stats {st}")
    check_mb_path(st, "bands")
    assert st["mb_bands_lds"] > 0, st
    assert 0 < st["mb_bands_lds"] < st["mb_bands"], st
    for f, p in enumerate(("flat255", "bits")):
        t0 = time.perf_counter()
        want = blend_ref(flat, batch[f], MULTIBAND)[0]
        print(f"restatement of {p}: {time.perf_counter() - t0:.2f} s")
        d = _diff(got[f], want)
        print(f"band pass on the LDS ring, capture {f} ({p}): max |diff| {d}")
        assert d == 0, (p, d)
    plan.close()


# ---- the largest feather quotient ----------------------------------------------------------------
BIG = dict(n=2, w=1920, h=1080, ch=3, step=640)


@pytest.mark.parametrize("pattern", ["flat255", "bits"])
def test_largest_feather_quotient(pattern):
    """2 x 1920x1080, 640 px apart: the largest D the bench's frame size gives (both cameras
    539 px from an edge), with the largest numerator (255 D) on flat255."""
    plan = _plan(BIG, FEATHER)
    flat = plan.describe()
    frames = pattern_frames(BIG, pattern)
    t0 = time.perf_counter()
    want = blend_ref(flat, frames, FEATHER)[0]
    print(f"restatement ({plan.out_w} x {plan.out_h}): {time.perf_counter() - t0:.2f} s")
    if pattern == "flat255":
        assert (want == 255).all()
    for method, path in (("stitch_direct", "direct feather"),
                         ("stitch_device", "prepared feather")):
        d = _diff(_stitch(plan, [frames], method)[0], want)
        print(f"{path}, largest quotient, {pattern}: max |diff| {d}")
        assert d == 0, (path, d)
    plan.close()
