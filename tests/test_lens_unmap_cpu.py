"""The inverse lens map on the CPU (mcs_lens_unmap_host, csrc/mcs_lens_core.h lens_invert) against
its numpy specification tests/lens_inv_ref.py bit for bit, its round trip through
mcs_lens_map_host, the lenses with and without raw pixels that have no preimage, the identity
lens, host validation, and mcs_rig_job_set_lens's argument checks on a job that never touches a
device."""
import ctypes

import numpy as np
import pytest

from multicamera_stitching_amd import _capi

import lens_inv_ref
from lens_inv_ref import NOPRE
from test_lens_cpu import FOLD
from test_undistort_cpu import CASES

FULL = CASES + [FOLD]            # every in-frame raw position has a preimage
LENSES = FULL + [NOPRE]
TOL = 2.0 ** -20


@pytest.fixture(scope="module")
def unmapped():
    """(grid, mcs_lens_unmap_host of it) per lens, computed once."""
    out = []
    for case in LENSES:
        g = lens_inv_ref.grid(case)
        out.append((g, _capi.lens_unmap_host(case["K"], case["d"], g)))
    return out


@pytest.mark.parametrize("i", range(len(LENSES)))
def test_host_unmap_equals_numpy_specification(unmapped, i):
    case, (g, got) = LENSES[i], unmapped[i]
    u, v = lens_inv_ref.lens_invert(case["K"], case["d"], g[:, 0], g[:, 1])
    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(got[:, 1]))
    assert np.array_equal(got[:, 0], u, equal_nan=True)
    assert np.array_equal(got[:, 1], v, equal_nan=True)


@pytest.mark.parametrize("i", range(len(LENSES)))
def test_valid_results_round_trip_through_the_lens(unmapped, i):
    case, (g, got) = LENSES[i], unmapped[i]
    ok = ~np.isnan(got[:, 0])
    assert ok.any()
    back = _capi.lens_map_host(case["K"], case["d"], got[ok])
    err = np.abs(back - g[ok]).max()
    print("%dx%d: %d of %d valid, worst round trip %.3g px" % (case["w"], case["h"], ok.sum(),
                                                               ok.size, err))
    assert not np.isnan(back).any() and err <= TOL
    if case is NOPRE:
        w, h = case["w"], case["h"]
        nan = np.isnan(got[:, 0]).reshape(h, w)
        assert nan[0, 0] and nan[0, w - 1] and nan[h - 1, 0] and nan[h - 1, w - 1]
        assert not nan[h // 2 - 32:h // 2 + 32, w // 2 - 32:w // 2 + 32].any()
    else:
        assert ok.all()


@pytest.mark.parametrize("dist", [None, [0.0] * 5, [0.0] * 8, [0.0] * 12])
def test_identity_lens_returns_its_input_as_float(dist):
    K = [[700.0, 0, 320.0], [0, 700.0, 240.0], [0, 0, 1]]
    y, x = np.mgrid[0:480, 0:640].astype(np.float64)
    p = np.stack([x.ravel(), y.ravel()], axis=1)
    got = _capi.lens_unmap_host(K, dist, p)
    assert np.array_equal(got.astype(np.float32), p.astype(np.float32))


def test_host_validation_is_a_status():
    K, d = CASES[0]["K"], CASES[0]["d"]
    skew = [[500.0, 0.3, 320.0], [0, 500.0, 240.0], [0, 0, 1]]
    tilt = [0.0] * 12 + [0.01, 0.0]
    for bad_k, bad_d, code in ((skew, d, _capi.MCS_E_UNSUPPORTED),
                               (K, tilt, _capi.MCS_E_UNSUPPORTED),
                               (K, [0.1, 0.2, 0.3], _capi.MCS_E_UNSUPPORTED),
                               (K, [np.nan, 0, 0, 0], _capi.MCS_E_INVALID),
                               ([[np.inf, 0, 1], [0, 1, 1], [0, 0, 1]], d, _capi.MCS_E_INVALID),
                               ([[0.0, 0, 1], [0, 1, 1], [0, 0, 1]], d, _capi.MCS_E_INVALID)):
        with pytest.raises(_capi.McsError) as e:
            _capi.lens_unmap_host(bad_k, bad_d, np.zeros((1, 2)))
        assert e.value.code == code
        with pytest.raises(_capi.McsError) as e2:
            _capi.lens_map_host(bad_k, bad_d, np.zeros((1, 2)))
        assert e2.value.code == code
    L = _capi.load()
    assert L.mcs_lens_unmap_host(None, None, 0, None, 0, None) == _capi.MCS_E_INVALID
    k = np.asarray(K, np.float64).reshape(9)
    kp = k.ctypes.data_as(ctypes.c_void_p)
    assert L.mcs_lens_unmap_host(kp, None, 4, None, 0, None) == _capi.MCS_E_INVALID   # NULL dist
    assert L.mcs_lens_unmap_host(kp, None, 0, None, 1, None) == _capi.MCS_E_INVALID   # NULL xy
    assert L.mcs_lens_unmap_host(kp, None, 0, None, -1, None) == _capi.MCS_E_INVALID
    assert L.mcs_lens_unmap_host(kp, None, 0, None, 0, None) == _capi.MCS_OK
    with pytest.raises(ValueError):
        _capi.lens_unmap_host(K, d, np.zeros((4, 3)))
    # non-finite positions are NaN, not an error
    got = _capi.lens_unmap_host(K, d, [[np.nan, 1.0], [np.inf, 1.0], [10.0, 20.0]])
    assert np.isnan(got[:2]).all() and not np.isnan(got[2]).any()


def test_rig_job_set_lens_argument_checks():
    """A job that is never submitted touches no device: set_lens is host state only."""
    K, d = CASES[0]["K"], CASES[0]["d"]
    job = _capi.RigJob(3, 320, 240, 3, nfeatures=100)
    try:
        for cam in (-1, 3, 16):
            with pytest.raises(_capi.McsError) as e:
                job.set_lens(cam, K, d)
            assert e.value.code == _capi.MCS_E_INVALID
        with pytest.raises(_capi.McsError) as e:
            job.set_lens(0, K, [0.0] * 12 + [0.01, 0.0])
        assert e.value.code == _capi.MCS_E_UNSUPPORTED
        with pytest.raises(_capi.McsError) as e:
            job.set_lens(0, K, [0.1, 0.2, 0.3])
        assert e.value.code == _capi.MCS_E_UNSUPPORTED
        with pytest.raises(_capi.McsError) as e:
            job.set_lens(0, [[500.0, 0.3, 320.0], [0, 500.0, 240.0], [0, 0, 1]], d)
        assert e.value.code == _capi.MCS_E_UNSUPPORTED
        with pytest.raises(_capi.McsError) as e:
            job.set_lens(0, K, [np.nan, 0, 0, 0])
        assert e.value.code == _capi.MCS_E_INVALID
        job.set_lens(0, K, d).set_lens(2, np.eye(3)).set_lens(1, K, [0.0] * 14)
        job.set_lens(0, None).set_lens(0, None).set_lens(2, None)   # (none left on 0: no error)
        L = _capi.load()
        assert L.mcs_rig_job_set_lens(None, 0, None, None, 0) == _capi.MCS_E_INVALID
        k = np.asarray(K, np.float64).reshape(9)
        assert L.mcs_rig_job_set_lens(job._h, 0, k.ctypes.data_as(ctypes.c_void_p), None,
                                      5) == _capi.MCS_E_INVALID     # NULL dist
    finally:
        job.close()
    # a batch job's cameras are those of one capture
    batch = _capi.RigJob(2, 320, 240, 3, nfeatures=100, captures=2)
    try:
        batch.set_lens(1, K, d)
        with pytest.raises(_capi.McsError) as e:
            batch.set_lens(2, K, d)
        assert e.value.code == _capi.MCS_E_INVALID
    finally:
        batch.close()
