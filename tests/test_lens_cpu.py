"""Lensed plans on the CPU (mcs_plan_set_lens, mcs_lens_map_host): the host lens map against the
numpy specification tests/lens_ref.py bit for bit, against the undistortion map the package
already has, the identity lens, host validation, pickles, and the specification itself against
the two-step path (cv2.undistort, then stitch) on references only."""
import pickle

import numpy as np
import pytest

from multicamera_stitching_amd import _capi, rig
from multicamera_stitching_amd.StitcherClass import _stage_desc
from oracle import oracle

import lens_ref
from test_undistort_cpu import CASES

FOLD = dict(K=CASES[0]["K"], d=[-0.35, 0.12, 0, 0, -0.02], w=640, h=480)   # folds back
LENSES = CASES + [FOLD]


@pytest.mark.parametrize("case", LENSES)
def test_host_map_equals_numpy_specification(case):
    """10,000 seeded points per lens, well past the frame (and past the fold-back radius where
    there is one): equal bit for bit, NaN beyond r2max, r2max equal."""
    rng = np.random.default_rng(7)
    w, h = case["w"], case["h"]
    uv = np.stack([rng.uniform(-1.5 * w, 2.5 * w, 10000), rng.uniform(-1.5 * h, 2.5 * h, 10000)],
                  axis=1)
    got, r2 = _capi.lens_map_host(case["K"], case["d"], uv, with_r2max=True)
    want_r2 = lens_ref.r2max(case["d"])
    assert r2 == want_r2
    xr, yr = lens_ref.lens_apply(case["K"], case["d"], uv[:, 0], uv[:, 1])
    assert np.array_equal(got[:, 0], xr, equal_nan=True)
    assert np.array_equal(got[:, 1], yr, equal_nan=True)
    K = np.asarray(case["K"], np.float64)
    x, y = (uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1]
    beyond = ~(x * x + y * y <= want_r2)
    assert np.array_equal(np.isnan(got[:, 0]), beyond) and np.array_equal(np.isnan(got[:, 1]), beyond)
    if case is FOLD:
        assert r2 == 2.4049224853515625 and beyond.sum() > 100
    else:
        assert r2 == np.inf


@pytest.mark.parametrize("case", CASES[:4])
def test_lens_at_pixel_centres_vs_undistort_map(case):
    """rint(32 lens) at the integer positions of the whole frame against mcs_undistort_map_host:
    at most 1 unit apart (cv::initUndistortRectifyMap accumulates _x += ir[0] along a row, the
    per-position lens does not)."""
    w, h = case["w"], case["h"]
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    xy = _capi.lens_map_host(case["K"], case["d"], np.stack([u, v], axis=-1))
    i = np.rint(xy * 32).astype(np.int64)
    mine = (i >> 5).astype(np.int16).astype(np.int64) * 32 + (i & 31)
    tab = _capi.undistort_map_host(case["K"], case["d"], w, h).astype(np.int64)
    diff = np.abs(mine - tab)
    print("positions off by one unit: %d of %d" % (int((diff > 0).sum()), diff.size))
    assert diff.max() <= 1


def test_identity_lens_returns_its_input():
    p = np.random.default_rng(3).uniform(-5000, 5000, (100000, 2))
    got, r2 = _capi.lens_map_host(np.eye(3), None, p, with_r2max=True)
    assert np.array_equal(got, p) and r2 == np.inf
    xr, yr = lens_ref.lens_apply(np.eye(3), None, p[:, 0], p[:, 1])
    assert np.array_equal(xr, p[:, 0]) and np.array_equal(yr, p[:, 1])


def _chain(n=3, w=160, h=120, ch=3, interp=1, **kw):
    st, images, _ = rig.calibrated_stitcher(n, w, h, ch, seed=0, **kw)
    cams = [images[label] for label in st.img_labels]
    plan = _capi.Plan([_stage_desc(sb) for sb in st.stitchers], w, h, ch, interp)
    return st, images, cams, plan


def test_host_validation_is_a_status():
    """Plan creation and set_lens touch no device; everything refused is a status."""
    _, _, _, plan = _chain()
    K, d = CASES[0]["K"], CASES[0]["d"]
    assert plan.stats()["lens_cams"] == 0
    plan.set_lens(0, K, d).set_lens(2, np.eye(3))
    assert plan.stats()["lens_cams"] == 2
    plan.set_lens(2, None).set_lens(1, None)          # (camera 1 had none: not an error)
    assert plan.stats()["lens_cams"] == 1
    skew = [[500.0, 0.3, 320.0], [0, 500.0, 240.0], [0, 0, 1]]
    tilt = [0.0] * 12 + [0.01, 0.0]
    for bad_k, bad_d, code in ((skew, d, _capi.MCS_E_UNSUPPORTED),
                               (K, tilt, _capi.MCS_E_UNSUPPORTED),
                               (K, [0.1, 0.2, 0.3], _capi.MCS_E_UNSUPPORTED),
                               (K, [np.nan, 0, 0, 0], _capi.MCS_E_INVALID),
                               ([[np.inf, 0, 1], [0, 1, 1], [0, 0, 1]], d, _capi.MCS_E_INVALID)):
        with pytest.raises(_capi.McsError) as e:
            plan.set_lens(0, bad_k, bad_d)
        assert e.value.code == code
        with pytest.raises(_capi.McsError) as e:
            _capi.lens_map_host(bad_k, bad_d, np.zeros((1, 2)))
        assert e.value.code == code
    for cam in (-1, 3, 16):
        with pytest.raises(_capi.McsError) as e:
            plan.set_lens(cam, K, d)
        assert e.value.code == _capi.MCS_E_INVALID
    assert plan.stats()["lens_cams"] == 1             # a refused call changes nothing
    und = _capi.Plan.undistort(K, d, 640, 480, 3)
    with pytest.raises(_capi.McsError) as e:
        und.set_lens(0, K, d)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED
    L = _capi.load()
    assert L.mcs_plan_set_lens(None, 0, None, None, 0) == _capi.MCS_E_INVALID
    assert L.mcs_lens_map_host(None, None, 0, None, 0, None, None) == _capi.MCS_E_INVALID
    warp = _capi.Plan.warp(np.eye(3), 64, 48, 64, 48, 3)
    assert warp.set_lens(0, K, d).stats()["lens_cams"] == 1
    cams, _, g = rig.cylinder_rig(3, 96, 64, 60.0, 1, seed=6)
    cyl = _capi.Plan.cylindrical(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"], g["v0"], 1)
    for c in range(3):
        cyl.set_lens(c, K, d)
    assert cyl.stats()["lens_cams"] == 3


def test_pickles_are_byte_equal_with_and_without_lenses():
    st, _, _, _ = _chain()
    for s in st.stitchers:
        s.params_to_list()
    before = pickle.dumps(st, pickle.HIGHEST_PROTOCOL)
    st.set_lenses({"CAM1": (CASES[0]["K"], CASES[0]["d"]), "CAM3": (np.eye(3), None),
                   "CAM2": None})
    assert sorted(st.__dict__["_mcs_lenses"]) == [0, 2]
    assert pickle.dumps(st, pickle.HIGHEST_PROTOCOL) == before
    with pytest.raises(KeyError):
        st.set_lenses({"CAM9": (np.eye(3), None)})
    st.set_lenses({})
    assert "_mcs_lenses" not in st.__dict__
    assert pickle.dumps(st, pickle.HIGHEST_PROTOCOL) == before


def test_specification_agrees_with_undistort_then_stitch():
    """The fused mosaic (lens_ref paste of the raw frames) against the two-step one
    (oracle.flat_stitch of oracle.undistort-ed frames), where all taps of both lie inside the
    frames (found by pushing all-255 frames through both: 255 comes out only where every tap is
    inside).  They differ by the second resampling only.  Measured on these two references:
    mean |fused - two-step| = 0.4662 grey levels over 98.9 % of the mosaic (rig.texture carries
    +-8 levels of per-pixel noise), and 3.9489 with the lens left out of lens_ref (8.5 x).  The
    bounds: at most 2 x the measured value, and without the lens at least 5 x it, so that a sign
    or direction error of the lens cannot pass."""
    measured = 0.4662
    _, _, cams, plan = _chain()
    flat = plan.describe()
    K = [[140.0, 0, 79.5], [0, 140.0, 59.5], [0, 0, 1]]
    d = [-0.2, 0.05, 0.001, -0.0005]
    lenses = {i: (K, d) for i in range(3)}

    def fused(frames, ls):
        pos, slot_cams, rects = lens_ref.chain_positions(flat, 1, ls)
        return lens_ref.render_paste(pos, slot_cams, rects, frames)

    def two_step(frames):
        return oracle.flat_stitch(flat, [oracle.undistort(f, K, d) for f in frames])

    ones = [np.full_like(c, 255) for c in cams]
    inside = (fused(ones, lenses) == 255).all(-1) & (two_step(ones) == 255).all(-1)
    assert inside.mean() > 0.9
    want = two_step(cams).astype(np.int64)
    with_lens = np.abs(fused(cams, lenses).astype(np.int64) - want)[inside].mean()
    without = np.abs(fused(cams, {}).astype(np.int64) - want)[inside].mean()
    print("mean |fused - two-step| = %.4f, without the lens %.4f" % (with_lens, without))
    assert with_lens <= 2 * measured
    assert without >= 5 * measured
