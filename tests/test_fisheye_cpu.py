"""The fisheye lens model on the CPU (mcs_lens_map_host_model, MCS_LENS_FISHEYE): the host map
against the numpy specification tests/fisheye_ref.py bit for bit, answers known without either
(atan(1) = pi / 4, atan(sqrt 3) = pi / 3), the arctangent against math.atan, the valid angle,
host validation, and the four older entry points against their _model(MCS_LENS_PINHOLE) forms."""
import ctypes
import math

import numpy as np
import pytest

from multicamera_stitching_amd import _capi, rig
from multicamera_stitching_amd.StitcherClass import _stage_desc

import fisheye_ref
from test_undistort_cpu import CASES

W, H = 96, 64
ZERO = dict(K=[[60.0, 0, 47.5], [0, 60.0, 31.5], [0, 0, 1]], d=None)
MILD = dict(K=[[70.0, 0, 47.2], [0, 71.0, 31.9], [0, 0, 1]], d=[-0.03, 0.01, -0.002, 0.0005])
# td = t (1 - 0.6 t^2) stops growing at t = 0.745: r = 0.92, the frame's corner is at r = 1.42
FOLD = dict(K=[[40.0, 0, 47.5], [0, 40.0, 31.5], [0, 0, 1]], d=[-0.6, 0.0, 0.0, 0.0])
LENSES = [ZERO, MILD, FOLD]
UNIT = np.eye(3)


def _grid():
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    far = [[-1e4, 3.0], [5e3, -7e3], [1e9, 1e9], [-1e300, 2.0], [1e200, 1e200],
           [np.nan, 1.0], [1.0, np.nan], [np.inf, 0.0], [0.0, -np.inf], [np.inf, np.inf]]
    return np.concatenate([np.stack([u.ravel(), v.ravel()], axis=1), np.array(far)])


@pytest.mark.parametrize("case", LENSES, ids=["zero", "mild", "fold"])
def test_host_map_equals_numpy_specification(case):
    uv = _grid()
    got, limit = _capi.lens_map_host(case["K"], case["d"], uv, with_r2max=True, model="fisheye")
    assert limit == fisheye_ref.tmax(case["d"])
    xr, yr = fisheye_ref.lens_apply(case["K"], case["d"], uv[:, 0], uv[:, 1])
    assert np.array_equal(got[:, 0], xr, equal_nan=True)
    assert np.array_equal(got[:, 1], yr, equal_nan=True)
    assert np.isnan(got[-5:]).all()                       # NaN and inf positions: outside
    inside = ~np.isnan(got[:W * H, 0])
    if case is FOLD:
        assert limit == 763 / 1024.0
        assert 0 < inside.sum() < W * H                   # the valid angle falls inside the frame
    else:
        assert limit == np.inf and inside.all()
        assert not np.isnan(got[W * H:W * H + 3]).any()   # far positions map ...
        assert np.isnan(got[W * H + 3:-5]).all()          # ... until their radius overflows


def test_known_answers():
    """Equidistant model with D = 0 and fx = fy = f: normalised radius 1 lands at raw radius
    f pi / 4, sqrt(3) at f pi / 3 (4 ulp of the result); the principal point maps to itself."""
    f = 64.0
    K = [[f, 0, 0.0], [0, f, 0.0], [0, 0, 1]]
    s3 = math.sqrt(3.0)
    uv = np.array([[f, 0.0], [0.0, f], [-f, 0.0], [f * s3, 0.0], [0.0, -f * s3]])
    got = _capi.lens_map_host(K, None, uv, model="fisheye")
    want = np.array([[f * math.pi / 4, 0.0], [0.0, f * math.pi / 4], [-f * math.pi / 4, 0.0],
                     [f * math.pi / 3, 0.0], [0.0, -f * math.pi / 3]])
    ulps = np.abs(got - want) / np.spacing(np.abs(want).max(axis=1))[:, None]
    print("known answers, ulp:", ulps.max(axis=1))
    assert ulps.max() <= 4
    assert np.array_equal(got == 0.0, want == 0.0)
    for case in LENSES:
        K = np.asarray(case["K"])
        pp = np.array([[K[0, 2], K[1, 2]]])
        assert np.array_equal(_capi.lens_map_host(case["K"], case["d"], pp, model="fisheye"), pp)


def _atan_grid():
    g = [i / 4096.0 for i in range(32769)] + [2.0 ** k for k in range(-60, 61)]
    for b in fisheye_ref.BREAKS:
        g += [float(np.nextafter(b, 0.0)), b, float(np.nextafter(b, 9.0))]
    return np.array(sorted(set(g)))


def test_restated_lens_atan_against_libm():
    """The numpy restatement's arctangent (the library's is tied to it bit for bit by
    test_library_arctangent_is_the_specification and by tests/native/fisheye_check.cpp, which
    also holds the library's own against libm): at most 4 ulp from math.atan (1 for reduction
    plus polynomial, 1 for libm, doubled); non-decreasing over the grid, the breakpoints' neighbours included; atan(0) = 0."""
    g = _atan_grid()
    got = fisheye_ref.lens_atan(g)
    want = np.array([math.atan(v) for v in g])
    ulps = np.abs(got - want) / np.spacing(want)
    print("lens_atan against math.atan: max %.3f ulp" % ulps[1:].max())
    assert got[0] == 0.0 and not np.signbit(got[0])
    assert ulps[1:].max() <= 4
    assert np.all(np.diff(got) >= 0)
    assert fisheye_ref.lens_atan(np.inf) == math.pi / 2 and np.isnan(fisheye_ref.lens_atan(np.nan))


def test_library_arctangent_is_the_specification():
    """The library's arctangent is reached through the map: with K = I and D = 0 the raw x of
    (r, 0) is r (t / r); equal to the restatement's over the arctangent's whole test grid."""
    g = _atan_grid()
    uv = np.stack([g, np.zeros_like(g)], axis=1)
    got = _capi.lens_map_host(UNIT, None, uv, model="fisheye")
    with np.errstate(all="ignore"):
        t = fisheye_ref.lens_atan(g)
        want = np.where(g == 0.0, 0.0, g * (t / g))
    xr, _ = fisheye_ref.lens_apply(UNIT, None, g, np.zeros_like(g))
    assert np.array_equal(got[:, 0], xr) and np.array_equal(xr, want)


def test_valid_angle_edge():
    """The last radius whose angle is inside tmax maps, the next double gives NaN."""
    d = FOLD["d"]
    tm = fisheye_ref.tmax(d)
    lo, hi = 0.5, 2.0                                   # atan(0.5) < tmax < atan(2)
    assert fisheye_ref.lens_atan(lo) <= tm < fisheye_ref.lens_atan(hi)
    while np.nextafter(lo, 9.0) < hi:                   # lens_atan is monotone
        mid = 0.5 * (lo + hi)
        if fisheye_ref.lens_atan(mid) <= tm:
            lo = mid
        else:
            hi = mid
    for axis in (0, 1):
        uv = np.zeros((2, 2))
        uv[:, axis] = [lo, hi]
        got = _capi.lens_map_host(UNIT, d, uv, model="fisheye")
        assert np.isfinite(got[0]).all() and np.isnan(got[1]).all()
    # a lens whose angle never stops growing has no limit; one that shrinks from the start has 0
    assert _capi.lens_map_host(UNIT, [0.1, 0, 0, 0], np.zeros((1, 2)), True, "fisheye")[1] == np.inf
    out, lim = _capi.lens_map_host(UNIT, [-1e9, 0, 0, 0], np.array([[0.0, 0.0], [1e-3, 0.0]]),
                                   True, "fisheye")
    assert lim == 0.0 == fisheye_ref.tmax([-1e9, 0, 0, 0])
    assert np.array_equal(out[0], [0.0, 0.0]) and np.isnan(out[1]).all()


def _chain(n=3, w=160, h=120, ch=3):
    st, images, _ = rig.calibrated_stitcher(n, w, h, ch, seed=0)
    return st, _capi.Plan([_stage_desc(sb) for sb in st.stitchers], w, h, ch, 1)


def test_host_validation_is_a_status():
    K, d = MILD["K"], MILD["d"]
    st, plan = _chain()
    one = np.zeros((1, 2))
    for nd in (1, 2, 3, 5, 8, 12, 14):
        for call in (lambda: _capi.lens_map_host(K, [0.0] * nd, one, model="fisheye"),
                     lambda: _capi.lens_unmap_host(K, [0.0] * nd, one, model="fisheye"),
                     lambda: plan.set_lens(0, K, [0.0] * nd, model="fisheye")):
            with pytest.raises(_capi.McsError) as e:
                call()
            assert e.value.code == _capi.MCS_E_UNSUPPORTED
    for model in (2, -1, 255):
        for call in (lambda: _capi.lens_map_host(K, d, one, model=model),
                     lambda: _capi.lens_unmap_host(K, d, one, model=model),
                     lambda: plan.set_lens(0, K, d, model=model)):
            with pytest.raises(_capi.McsError) as e:
                call()
            assert e.value.code == _capi.MCS_E_INVALID
    with pytest.raises(ValueError):
        plan.set_lens(0, K, d, model="equidistant")
    skew = [[70.0, 0.3, 47.0], [0, 70.0, 31.0], [0, 0, 1]]
    with pytest.raises(_capi.McsError) as e:
        plan.set_lens(0, skew, d, model="fisheye")
    assert e.value.code == _capi.MCS_E_UNSUPPORTED
    assert plan.stats()["lens_cams"] == 0                # a refused call changes nothing
    plan.set_lens(0, K, d, model="fisheye").set_lens(1, CASES[0]["K"], CASES[0]["d"])
    plan.set_lens(2, K, None, model=_capi.MCS_LENS_FISHEYE)
    assert plan.stats()["lens_cams"] == 3                # a mixed rig
    plan.set_lens(0, None)
    assert plan.stats()["lens_cams"] == 2
    und = _capi.Plan.undistort(CASES[0]["K"], CASES[0]["d"], 640, 480, 3)
    with pytest.raises(_capi.McsError) as e:
        und.set_lens(0, K, d, model="fisheye")
    assert e.value.code == _capi.MCS_E_UNSUPPORTED
    L = _capi.load()
    assert L.mcs_plan_set_lens_model(None, 0, 1, None, None, 0) == _capi.MCS_E_INVALID
    assert L.mcs_rig_job_set_lens_model(None, 0, 1, None, None, 0) == _capi.MCS_E_INVALID
    assert L.mcs_lens_map_host_model(1, None, None, 0, None, 0, None, None) == _capi.MCS_E_INVALID
    assert L.mcs_lens_unmap_host_model(1, None, None, 0, None, 0, None) == _capi.MCS_E_INVALID
    # the Python API takes (K, D, "fisheye") beside (K, D)
    st.set_lenses({"CAM1": (K, d, "fisheye"), "CAM2": (CASES[0]["K"], CASES[0]["d"])})
    table = st.__dict__["_mcs_lenses"]
    assert table[0][2] == _capi.MCS_LENS_FISHEYE and table[1][2] == _capi.MCS_LENS_PINHOLE


@pytest.mark.parametrize("case", CASES)
def test_old_entry_points_are_their_model_0_forms(case):
    """mcs_lens_map_host / mcs_lens_unmap_host and the _model forms with MCS_LENS_PINHOLE: the
    same status, limit and bits; mcs_plan_set_lens / mcs_rig_job_set_lens: the same status and
    the same plan state."""
    L = _capi.load()
    vp = ctypes.c_void_p
    k, d = _capi._lens_args(case["K"], case["d"])
    dp = d.ctypes.data_as(vp) if d.size else None
    rng = np.random.default_rng(11)
    w, h = case["w"], case["h"]
    pts = np.ascontiguousarray(np.stack([rng.uniform(-0.5 * w, 1.5 * w, 4000),
                                         rng.uniform(-0.5 * h, 1.5 * h, 4000)], axis=1))
    a, b = np.empty_like(pts), np.empty_like(pts)
    la, lb = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    assert L.mcs_lens_map_host(k.ctypes.data_as(vp), dp, d.size, pts.ctypes.data_as(vp), 4000,
                               a.ctypes.data_as(vp), ctypes.byref(la)) == 0
    assert L.mcs_lens_map_host_model(0, k.ctypes.data_as(vp), dp, d.size, pts.ctypes.data_as(vp),
                                     4000, b.ctypes.data_as(vp), ctypes.byref(lb)) == 0
    assert la.value == lb.value and a.tobytes() == b.tobytes()
    assert L.mcs_lens_unmap_host(k.ctypes.data_as(vp), dp, d.size, pts.ctypes.data_as(vp), 4000,
                                 a.ctypes.data_as(vp)) == 0
    assert L.mcs_lens_unmap_host_model(0, k.ctypes.data_as(vp), dp, d.size,
                                       pts.ctypes.data_as(vp), 4000, b.ctypes.data_as(vp)) == 0
    assert a.tobytes() == b.tobytes() and np.isfinite(a).any()
    _, p0 = _chain()
    _, p1 = _chain()
    assert L.mcs_plan_set_lens(p0._h, 1, k.ctypes.data_as(vp), dp, d.size) == 0
    assert L.mcs_plan_set_lens_model(p1._h, 1, 0, k.ctypes.data_as(vp), dp, d.size) == 0
    assert p0.stats() == p1.stats() and p0.stats()["lens_cams"] == 1
    bad = (ctypes.c_double * 3)(0.1, 0.2, 0.3)
    assert (L.mcs_plan_set_lens(p0._h, 1, k.ctypes.data_as(vp), bad, 3)
            == L.mcs_plan_set_lens_model(p1._h, 1, 0, k.ctypes.data_as(vp), bad, 3)
            == _capi.MCS_E_UNSUPPORTED)
    assert (L.mcs_rig_job_set_lens(None, 0, k.ctypes.data_as(vp), dp, d.size)
            == L.mcs_rig_job_set_lens_model(None, 0, 0, k.ctypes.data_as(vp), dp, d.size)
            == _capi.MCS_E_INVALID)
