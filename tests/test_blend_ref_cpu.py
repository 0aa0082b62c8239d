"""The blend oracle (oracle/orc_blend.c) against its independent NumPy restatement
(blend_ref.blend_ref, written from the oracle's header comment), on frames that drive the
arithmetic to the ends of its range.  Bar: difference 0 and equal owner maps, for every
translation case x pattern x mode.

Also, on the restatement alone: known answers, and the conditions that make
test_gpu_blend_values.py mean something -- the share of values that the final clamp changes
(R0 < -0.5 or R0 >= 255.5), the dense tiles of T5, and the largest values of the pyramid levels.
"""
import functools

import numpy as np
import pytest

from blend_ref import (CASES, FEATHER, MULTIBAND, PATTERNS, SEAM, _slots, blend_ref,
                       make_plan, pattern_frames)
from oracle import oracle

MODES = {"seam": SEAM, "feather": FEATHER, "multiband": MULTIBAND}


@functools.lru_cache(maxsize=None)
def _flat(case):
    plan = make_plan(**CASES[case])
    flat = plan.describe()
    plan.close()
    return flat


@functools.lru_cache(maxsize=None)
def _ref(case, pattern):
    """{mode: (out, owner, r0)} of the restatement and the info of its MULTIBAND, computed once."""
    frames = pattern_frames(CASES[case], pattern)
    info = {}
    res = {m: blend_ref(_flat(case), frames, m, info if m == MULTIBAND else None)
           for m in MODES.values()}
    for out, owner, r0 in res.values():
        for a in (out, owner, r0):
            if a is not None:
                a.setflags(write=False)
    return res, info


def _shares(case, pattern):
    """(share of the covered channel values with R0 < -0.5, with R0 >= 255.5)."""
    r0 = _ref(case, pattern)[0][MULTIBAND][2]
    covered = _ref(case, pattern)[0][MULTIBAND][1] != 255
    n = covered.sum() * (r0.size // covered.size)
    with np.errstate(invalid="ignore"):
        return float((r0 < -0.5).sum() / n), float((r0 >= 255.5).sum() / n)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_equals_restatement(case, pattern):
    frames = pattern_frames(CASES[case], pattern)
    for name, mode in MODES.items():
        want, want_owner, _ = _ref(case, pattern)[0][mode]
        got, owner = oracle.blend_stitch(_flat(case), frames, mode, want_owner=True)
        assert got.shape == want.shape
        diff = int(np.abs(got.astype(np.int16) - want.astype(np.int16)).max())
        assert diff == 0, (name, diff)
        assert np.array_equal(owner, want_owner), name
    lo, hi = _shares(case, pattern)
    print(f"{case} {pattern}: R0 < -0.5 on {100 * lo:.3f} %, R0 >= 255.5 on {100 * hi:.3f} % of "
          f"the covered channel values")


# ---- known answers, on the restatement alone -----------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_flat255_stays_255(case):
    res, _ = _ref(case, "flat255")
    for name, mode in MODES.items():
        out, owner, r0 = res[mode]
        covered = owner != 255
        assert covered.any() and (out[covered] == 255).all(), name
        assert (out[~covered] == 0).all(), name
        if r0 is not None:
            assert (r0[covered][~np.isnan(r0[covered])] == 255.0).all()


@pytest.mark.parametrize("pattern", ["alt0_255", "checker1"])
@pytest.mark.parametrize("case", list(CASES))
def test_feather_lies_between_the_cameras(case, pattern):
    """Every feathered value lies between the smallest and the largest sample of the cameras
    that cover the pixel."""
    c = CASES[case]
    frames = [f.reshape(c["h"], c["w"], -1) for f in pattern_frames(c, pattern)]
    flat = _flat(case)
    out, owner, _ = _ref(case, pattern)[0][FEATHER]
    out = out.reshape(owner.shape + (-1,)).astype(int)
    lo = np.full(out.shape, 256)
    hi = np.full(out.shape, -1)
    for cam, x0, y0 in _slots(flat):     # camera pixel (0, 0) lies at mosaic (-x0, -y0)
        ya, xa = max(-y0, 0), max(-x0, 0)
        yb, xb = min(c["h"] - y0, out.shape[0]), min(c["w"] - x0, out.shape[1])
        src = frames[cam][ya + y0:yb + y0, xa + x0:xb + x0].astype(int)
        lo[ya:yb, xa:xb] = np.minimum(lo[ya:yb, xa:xb], src)
        hi[ya:yb, xa:xb] = np.maximum(hi[ya:yb, xa:xb], src)
    covered = owner != 255
    assert (hi[covered] >= 0).all() and (hi[~covered] == -1).all()
    assert ((out >= lo) & (out <= hi))[covered].all()
    if pattern == "alt0_255":       # (checker1: on some rigs the cameras agree in the overlaps)
        mixed = covered[..., None] & (lo != hi)
        assert mixed.any() and ((out > lo) & (out < hi))[mixed].any()


def test_quotients_at_one_half():
    """alt0_1: cameras of 0 and 1 on T2 (camera 1 starts at column 90).  In row 5 both cameras are
    5 px from their top edge, so from column 95 to 144 their weights are equal and FEATHER is
    (d + (2 d) / 2) / (2 d) = 1, one half rounded up; at column 93 camera 1 weighs 3 against 5 and
    the quotient (96 + 128) / 256 is 0."""
    out = _ref("T2c3", "alt0_1")[0][FEATHER][0]
    assert set(np.unique(out)) == {0, 1}
    assert (out[5, 95:145] == 1).all() and (out[5, 93] == 0).all()
    assert (out[5, :90] == 0).all() and (out[5, 150:] == 1).all()


# ---- what the GPU test relies on -----------------------------------------------------------------
@pytest.mark.parametrize("case", ["T1", "T2c1", "T2c3", "T2c4", "T3"])
def test_bits_clamp_on_both_sides(case):
    lo, hi = _shares(case, "bits")
    print(f"{case} bits: below {100 * lo:.3f} %, above {100 * hi:.3f} %")
    assert lo >= 0.005 and hi >= 0.005, (lo, hi)


@pytest.mark.parametrize("case", ["T4", "T5", "T6"])
def test_bits_clamp_on_the_larger_rigs(case):
    lo, hi = _shares(case, "bits")
    print(f"{case} bits: below {100 * lo:.3f} %, above {100 * hi:.3f} %")
    assert lo > 0 and hi > 0, (lo, hi)


@pytest.mark.parametrize("pattern", ["checker4", "noise"])
@pytest.mark.parametrize("case", ["T1", "T2c1", "T2c3", "T2c4", "T3"])
def test_checker4_and_noise_clamp(case, pattern):
    lo, hi = _shares(case, pattern)
    print(f"{case} {pattern}: below {100 * lo:.3f} %, above {100 * hi:.3f} %")
    assert lo > 0 and hi > 0, (lo, hi)


def test_t5_has_dense_and_other_tiles():
    dense = _ref("T5", "bits")[1]["dense"]
    print(f"T5: {int(dense.sum())} of {dense.size} blend tiles take the feather rule")
    assert dense.any() and not dense.all()
    for case in CASES:
        if case != "T5":
            assert not _ref(case, "flat255")[1]["dense"].any(), case


def test_pyramid_levels_reach_their_largest_values():
    g1 = max(_ref(case, "flat255")[1]["max_g1"] for case in CASES)
    g2 = max(_ref(case, "flat255")[1]["max_g2"] for case in CASES)
    assert g1 == 256 * 255 == 65280 and g2 == 65536 * 255 == 16711680, (g1, g2)
