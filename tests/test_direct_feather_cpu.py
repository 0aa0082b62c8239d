"""Feather on the direct stitch path without a GPU: mcs_rig_job_set_blend is declared, exported
and bound; its argument checks; mcs_stitch_direct[_gained] accepts a FEATHER plan (its argument
checks come first and still hold), refuses MULTIBAND; the library embeds the new kernels.  Every
check returns before any HIP call (the pointers are never used)."""
import ctypes
import functools
import os
import re

import pytest

from multicamera_stitching_amd import _capi, build, estimate, rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _descs():
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, _, _ = rig.calibrated_stitcher(3, 96, 64, 3, seed=0, overlap=0.6)
    return [_stage_desc(sb) for sb in st.stitchers]


def _plan(blend):
    plan = _capi.Plan(_descs(), 96, 64, 3)
    plan.set_blend(blend)
    return plan


def test_header_and_binding_carry_the_rig_job_blend():
    header = open(os.path.join(ROOT, "include", "mcs.h")).read()
    assert re.search(r"\bint mcs_rig_job_set_blend\(mcs_rig_job \*job, int mode\);", header)
    assert "mcs_rig_job_set_blend" in _capi.EXPORTS
    fn = _capi.load().mcs_rig_job_set_blend
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_int]
    assert callable(_capi.RigJob.set_blend)
    assert _capi.load().mcs_abi_version() == 1      # a function added: the ABI version stands
    assert "MCS_BLEND_FEATHER" in header.split("int mcs_stitch_direct(")[0].split(
        "mcs_stitch_device without prepared tables")[1]          # the mcs_stitch_direct comment


def test_rig_job_set_blend_argument_checks():
    L = _capi.load()
    assert L.mcs_rig_job_set_blend(None, _capi.MCS_BLEND_FEATHER) == _capi.MCS_E_INVALID
    job = _capi.RigJob(3, 96, 64, 3)
    try:
        for mode in (_capi.MCS_BLEND_NONE, _capi.MCS_BLEND_SEAM, _capi.MCS_BLEND_FEATHER,
                     _capi.MCS_BLEND_NONE):
            job.set_blend(mode)
        for mode in (_capi.MCS_BLEND_MULTIBAND, -1, 4, 99):
            with pytest.raises(_capi.McsError) as e:
                job.set_blend(mode)
            assert e.value.code == _capi.MCS_E_INVALID, mode
    finally:
        job.close()


def test_capture_estimator_takes_the_direct_blend_modes_only():
    for mode in (_capi.MCS_BLEND_NONE, _capi.MCS_BLEND_SEAM, _capi.MCS_BLEND_FEATHER):
        est = estimate.CaptureEstimator(3, 96, 64, 3, blend=mode)
        assert est.blend == mode
        est.close()
    assert estimate.CaptureEstimator(3, 96, 64, 3).blend == _capi.MCS_BLEND_NONE
    with pytest.raises(ValueError):
        estimate.CaptureEstimator(3, 96, 64, 3, blend=_capi.MCS_BLEND_MULTIBAND)


@pytest.mark.parametrize("entry", ["stitch_direct", "stitch_direct_gained"])
def test_a_feather_plan_passes_the_argument_checks(entry):
    """n_frames = 0 returns after every check and before the first HIP call: MCS_OK now,
    MCS_E_UNSUPPORTED on the parent."""
    plan = _plan(_capi.MCS_BLEND_FEATHER)
    sizes = [96 * 64 * 3] * 3
    getattr(plan, entry)([4096] * 3, sizes, 4096, plan.out_w * 3, 0, 0)
    for kw in (dict(n_frames=-1), dict(n_frames=65536), dict(out_pitch=plan.out_w * 3 - 1)):
        with pytest.raises(_capi.McsError) as e:
            getattr(plan, entry)([4096] * 3, sizes, 4096, kw.get("out_pitch", plan.out_w * 3), 0,
                                 kw.get("n_frames", 1))
        assert e.value.code == _capi.MCS_E_INVALID, kw


@pytest.mark.parametrize("entry", ["stitch_direct", "stitch_direct_gained"])
def test_multiband_stays_refused(entry):
    plan = _plan(_capi.MCS_BLEND_MULTIBAND)
    with pytest.raises(_capi.McsError) as e:
        getattr(plan, entry)([4096] * 3, [96 * 64 * 3] * 3, 4096, plan.out_w * 3, 0, 0)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED and "mcs_stitch_device" in str(e.value)


def test_stitch_direct_on_a_gained_feather_plan_is_still_refused():
    plan = _plan(_capi.MCS_BLEND_FEATHER).set_gains([1.37, 1.0, 0.61])
    with pytest.raises(_capi.McsError) as e:
        plan.stitch_direct([4096] * 3, [96 * 64 * 3] * 3, 4096, plan.out_w * 3, 0, 0)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED and "mcs_gain_apply_device" in str(e.value)


def test_library_embeds_the_direct_feather_kernels():
    blob = open(build.LIB, "rb").read()
    for name in (b"mcs_direct_feather_c3_i1\0", b"mcs_direct_feather_c3_i1_g\0",
                 b"mcs_direct_feather_c1_i0\0", b"mcs_direct_feather_c4_i1_g\0"):
        assert name in blob, name
