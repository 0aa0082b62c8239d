"""The table-free overlap statistics and the rig job's exposure step without a GPU: the entry
points are declared, exported and bound; their argument checks as status codes (every check
returns before any HIP call: the pointers are never used); the rig job's exposure setting and its
gains before any capture; the library embeds the new kernels."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from multicamera_stitching_amd import _capi, build, estimate, rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcs_plan_overlap_stats_direct", "mcs_plan_overlap_stats_direct_async",
       "mcs_rig_job_set_exposure", "mcs_rig_job_gains")


@functools.lru_cache(maxsize=None)
def _descs():
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, _, _ = rig.calibrated_stitcher(3, 96, 64, 3, seed=0, overlap=0.6)
    return [_stage_desc(sb) for sb in st.stitchers]


def _plan():
    return _capi.Plan(_descs(), 96, 64, 3)


def _call(plan, n_frames=1, k=2, cams=(4096, 4096, 4096), sync=True, N=True, S=True, stats=4096):
    """The raw entry point's status code."""
    L = _capi.load()
    h = plan._h if plan is not None else None
    n = len(cams) if cams is not None else 3
    ptrs = (ctypes.c_void_p * n)(*[p or None for p in cams]) if cams is not None else None
    strides = (ctypes.c_int64 * n)(*([96 * 64 * 3] * n)) if cams is not None else None
    if sync:
        Nb = np.zeros((n, n), np.int64)
        Sb = np.zeros((max(n_frames, 1), n, n), np.int64)
        return L.mcs_plan_overlap_stats_direct(h, ptrs, strides, n_frames, k,
                                               Nb.ctypes.data if N else None,
                                               Sb.ctypes.data if S else None, None)
    return L.mcs_plan_overlap_stats_direct_async(h, ptrs, strides, n_frames, k,
                                                 ctypes.c_void_p(stats) if stats else None, None)


def test_header_exports_and_bindings():
    header = open(os.path.join(ROOT, "include", "mcs.h")).read()
    L = _capi.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.EXPORTS
        assert getattr(L, name).restype is ctypes.c_int
    assert L.mcs_abi_version() == 1                 # functions added: the ABI version stands
    assert list(L.mcs_plan_overlap_stats_direct.argtypes) == list(
        L.mcs_plan_overlap_stats.argtypes)
    for method in ("overlap_stats_direct", "overlap_stats_direct_async"):
        assert callable(getattr(_capi.Plan, method))
    assert callable(_capi.RigJob.set_exposure) and callable(_capi.RigJob.gains)
    # the wait_stitch comment states the one synchronise of the exposure step
    comment = header.split("int mcs_rig_job_wait_stitch(")[0].rsplit("/*", 1)[1]
    assert "mcs_rig_job_set_exposure" in comment and "synchronise" in comment


@pytest.mark.parametrize("sync", [True, False])
def test_statistics_argument_checks(sync):
    plan = _plan()
    E = _capi.MCS_E_INVALID
    assert _call(None, sync=sync) == E
    assert _call(plan, cams=None, sync=sync) == E
    if sync:
        assert _call(plan, N=False) == E
        assert _call(plan, S=False) == E
    else:
        assert _call(plan, sync=False, stats=0) == E
    for k in (-1, 5, 99):
        assert _call(plan, k=k, sync=sync) == E, k
    for nf in (0, -3, 65536):
        assert _call(plan, n_frames=nf, sync=sync) == E, nf
    assert _call(plan, cams=(4096, 0, 4096), sync=sync) == E      # a camera the mosaic needs
    assert "d_cams[1]" in _capi.load().mcs_last_error().decode()


@pytest.mark.parametrize("sync", [True, False])
def test_single_camera_plans_are_unsupported(sync):
    warp = _capi.Plan.warp(np.eye(3), 64, 48, 64, 48, 3)
    und = _capi.Plan.undistort([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]],
                               [-0.2, 0.05, 0, 0, 0], 64, 48, 3)
    for plan in (warp, und):
        assert _call(plan, cams=(4096,), sync=sync) == _capi.MCS_E_UNSUPPORTED
        # (as the table path answers)
        with pytest.raises(_capi.McsError) as e:
            plan.overlap_stats([4096], [64 * 48 * 3], 1, 2)
        assert e.value.code == _capi.MCS_E_UNSUPPORTED


def test_rig_job_exposure_setting_and_fresh_gains():
    L = _capi.load()
    assert L.mcs_rig_job_set_exposure(None, 2, 0.0, 0.0) == _capi.MCS_E_INVALID
    assert L.mcs_rig_job_gains(None, None, None, None) == _capi.MCS_E_INVALID
    for captures in (1, 2):
        job = _capi.RigJob(3, 96, 64, 3, captures=captures)
        try:
            g, q, on = job.gains()                  # a fresh job: identity, disabled
            shape = (3,) if captures == 1 else (2, 3)
            assert g.shape == shape and q.shape == shape and not on
            assert np.all(g == 1.0) and np.all(q == 256)
            for k in range(5):
                job.set_exposure(k)
                assert job.gains()[2]
            job.set_exposure(2, 0.02, 50.0)
            for k in (5, 6, 99):
                with pytest.raises(_capi.McsError) as e:
                    job.set_exposure(k)
                assert e.value.code == _capi.MCS_E_INVALID, k
                assert job.gains()[2]               # a refused call changes nothing
            for bad in (float("nan"), float("inf")):
                with pytest.raises(_capi.McsError) as e:
                    job.set_exposure(2, bad, 0.0)
                assert e.value.code == _capi.MCS_E_INVALID
            g, q, on = job.gains()                  # enabled, no capture stitched yet
            assert on and np.all(g == 1.0) and np.all(q == 256)
            job.set_exposure(-1)
            assert not job.gains()[2]
            job.set_exposure(-7)                    # any negative step disables
            assert not job.gains()[2]
            assert L.mcs_rig_job_gains(job._h, None, None, None) == _capi.MCS_OK
        finally:
            job.close()


def test_capture_estimator_exposure_option():
    est = estimate.CaptureEstimator(3, 96, 64, 3)
    assert est.exposure is None and np.all(est.gains == 1.0)
    est.close()
    est = estimate.CaptureEstimator(3, 96, 64, 3, blend=_capi.MCS_BLEND_FEATHER, exposure=2)
    assert est.exposure == 2 and est.gains.shape == (3,)
    assert est._job(0).gains()[2]                   # the setting reaches the job
    est.close()
    for bad in (-1, 5):
        with pytest.raises(ValueError):
            estimate.CaptureEstimator(3, 96, 64, 3, exposure=bad)


def test_library_embeds_the_direct_overlap_kernels():
    blob = open(build.LIB, "rb").read()
    for c in (1, 2, 3, 4):
        for i in (0, 1):
            assert b"mcs_direct_overlap_c%d_i%d\0" % (c, i) in blob
