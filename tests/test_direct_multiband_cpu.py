"""The direct multi-band path without a GPU: mcs_direct_multiband_work_size,
mcs_stitch_direct_multiband[_gained] and mcs_rig_job_set_multiband are declared, exported and
bound; their argument checks (every one returns before any HIP call: the pointers are never
used); the work area's size; CaptureEstimator(multiband=); the library embeds the new kernels in a
fourth code object that stays out of mcs_build_id."""
import ctypes
import functools
import os
import re

import pytest

from multicamera_stitching_amd import _capi, build, estimate, rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["stitch_direct_multiband", "stitch_direct_multiband_gained"]
SIZES = [96 * 64 * 3] * 3


@functools.lru_cache(maxsize=None)
def _descs():
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, _, _ = rig.calibrated_stitcher(3, 96, 64, 3, seed=0, overlap=0.6)
    return [_stage_desc(sb) for sb in st.stitchers]


def _plan(blend=_capi.MCS_BLEND_MULTIBAND):
    plan = _capi.Plan(_descs(), 96, 64, 3)
    if blend != _capi.MCS_BLEND_NONE:
        plan.set_blend(blend)
    return plan


def _call(plan, entry, n_frames=0, out_pitch=None, work_ptr=4096, work_bytes=None):
    if work_bytes is None:
        work_bytes = plan.direct_multiband_work_size()
    getattr(plan, entry)([4096] * 3, SIZES, 4096,
                         plan.out_w * 3 if out_pitch is None else out_pitch, 0, n_frames,
                         work_ptr, work_bytes)


def test_header_exports_and_signatures():
    header = open(os.path.join(ROOT, "include", "mcs.h")).read()
    assert re.search(r"\bint mcs_direct_multiband_work_size\(const mcs_plan \*plan, "
                     r"int64_t \*bytes\);", header)
    assert re.search(r"\bint mcs_rig_job_set_multiband\(mcs_rig_job \*job, int on\);", header)
    for name in ("mcs_stitch_direct_multiband", "mcs_stitch_direct_multiband_gained"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        args = " ".join(m.group(1).split())
        assert args == ("mcs_plan *plan, const uint8_t *const *d_cams, "
                        "const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch, "
                        "int64_t out_frame_stride, int n_frames, void *d_work, "
                        "int64_t work_bytes, void *stream"), args
    # the new declarations come after mcs_stitch_direct_gained
    assert header.index("int mcs_stitch_direct_gained(") < \
        header.index("int mcs_direct_multiband_work_size(")
    L = _capi.load()
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    want = {
        "mcs_direct_multiband_work_size": [P, ctypes.POINTER(I64)],
        "mcs_stitch_direct_multiband": [P, ctypes.POINTER(P), ctypes.POINTER(I64), P, I64, I64, I,
                                        P, I64, P],
        "mcs_stitch_direct_multiband_gained": [P, ctypes.POINTER(P), ctypes.POINTER(I64), P, I64,
                                               I64, I, P, I64, P],
        "mcs_rig_job_set_multiband": [P, I],
    }
    for name, argtypes in want.items():
        assert name in _capi.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is I and list(fn.argtypes) == argtypes, name
    assert L.mcs_abi_version() == 1      # functions added: the ABI version stands
    for method in ENTRIES + ["direct_multiband_work_size"]:
        assert callable(getattr(_capi.Plan, method))
    assert callable(_capi.RigJob.set_multiband)
    # the mcs_stitch_direct comment points at the new entry point
    comment = header.split("int mcs_stitch_direct(")[0].split(
        "mcs_stitch_device without prepared tables")[1]
    assert "mcs_stitch_direct_multiband" in comment


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_return_before_any_hip_call(entry):
    plan = _plan()
    _call(plan, entry, n_frames=0)                         # MCS_OK
    _call(plan, entry, n_frames=0, work_ptr=0, work_bytes=0)   # nothing to render: no area asked
    # device_kparams' checks, as on mcs_stitch_direct
    for kw in (dict(n_frames=-1), dict(n_frames=65536), dict(out_pitch=plan.out_w * 3 - 1)):
        with pytest.raises(_capi.McsError) as e:
            _call(plan, entry, **{"n_frames": 1, **kw})
        assert e.value.code == _capi.MCS_E_INVALID, kw
    # the work area: NULL, or one byte short -- the needed size is in the message
    need = plan.direct_multiband_work_size()
    for kw in (dict(work_ptr=0), dict(work_bytes=need - 1), dict(work_bytes=0)):
        with pytest.raises(_capi.McsError) as e:
            _call(plan, entry, n_frames=1, **kw)
        assert e.value.code == _capi.MCS_E_INVALID and str(need) in str(e.value), kw
    plan.close()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("blend", [_capi.MCS_BLEND_NONE, _capi.MCS_BLEND_FEATHER,
                                   _capi.MCS_BLEND_SEAM])
def test_other_blend_modes_are_invalid_and_name_mcs_stitch_direct(entry, blend):
    plan = _plan(blend)
    for n_frames in (0, 1):
        with pytest.raises(_capi.McsError) as e:
            _call(plan, entry, n_frames=n_frames)
        assert e.value.code == _capi.MCS_E_INVALID and "mcs_stitch_direct" in str(e.value)
    # device_kparams' checks still come first
    with pytest.raises(_capi.McsError) as e:
        _call(plan, entry, n_frames=-1)
    assert "n_frames" in str(e.value)
    plan.close()


def test_single_camera_plans_are_refused():
    """A warp / undistort plan takes no blend mode, so it is never a MULTIBAND plan."""
    K = [[100.0, 0, 47.5], [0, 100.0, 31.5], [0, 0, 1]]
    plan = _capi.Plan.undistort(K, [0.1, -0.05, 0, 0, 0], 96, 64, 3)
    with pytest.raises(_capi.McsError) as e:
        plan.stitch_direct_multiband([4096], [96 * 64 * 3], 4096, plan.out_w * 3, 0, 1, 4096,
                                     plan.direct_multiband_work_size())
    assert e.value.code == _capi.MCS_E_INVALID
    plan.close()


def test_gained_plan_through_the_ungained_entry_is_unsupported():
    plan = _plan().set_gains([1.37, 1.0, 0.61])
    for n_frames in (0, 1):
        with pytest.raises(_capi.McsError) as e:
            _call(plan, "stitch_direct_multiband", n_frames=n_frames)
        assert e.value.code == _capi.MCS_E_UNSUPPORTED and "mcs_gain_apply_device" in str(e.value)
    _call(plan, "stitch_direct_multiband_gained", n_frames=0)      # the gained form takes it
    plan.close()


def test_null_arguments():
    L = _capi.load()
    n = ctypes.c_int64(-1)
    assert L.mcs_direct_multiband_work_size(None, ctypes.byref(n)) == _capi.MCS_E_INVALID
    plan = _plan()
    assert L.mcs_direct_multiband_work_size(plan._h, None) == _capi.MCS_E_INVALID
    assert L.mcs_stitch_direct_multiband(None, None, None, None, 0, 0, 0, None, 0, None) == \
        _capi.MCS_E_INVALID
    assert L.mcs_rig_job_set_multiband(None, 1) == _capi.MCS_E_INVALID
    plan.close()


def _warp_plan(w, h):
    """A plan whose mosaic is w x h: the size is all the work area depends on."""
    return _capi.Plan.warp([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], 8, 8, w, h, 3)


@pytest.mark.parametrize("w, h, want", [
    (1, 1, 4), (16, 16, 4), (17, 17, 16), (33, 16, 12), (16, 65, 20),
])
def test_work_size_is_four_bytes_per_16x16_cell(w, h, want):
    plan = _warp_plan(w, h)
    assert (plan.out_w, plan.out_h) == (w, h)
    assert plan.direct_multiband_work_size() == want == 4 * (-(-w // 16)) * (-(-h // 16))
    plan.close()


def test_work_size_of_the_c2_mosaic():
    """BASELINE configs[1] (4 x 1920x1080, bench.py's rig): 4 bytes per cell, about 107 KB."""
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, _, _ = rig.calibrated_stitcher(4, 1920, 1080, 3, seed=0)
    plan = _capi.Plan([_stage_desc(sb) for sb in st.stitchers], 1920, 1080, 3, 1)
    need = plan.direct_multiband_work_size()
    assert need == 4 * (-(-plan.out_w // 16)) * (-(-plan.out_h // 16))
    assert 90_000 < need < 130_000, (plan.out_w, plan.out_h, need)
    plan.set_blend(_capi.MCS_BLEND_MULTIBAND)
    assert plan.direct_multiband_work_size() == need      # the mosaic's size only
    plan.close()


def test_rig_job_set_multiband_keeps_the_blend_mode_checks():
    job = _capi.RigJob(3, 96, 64, 3)
    try:
        job.set_multiband(True)
        job.set_blend(_capi.MCS_BLEND_FEATHER)         # kept for after set_multiband(False)
        with pytest.raises(_capi.McsError) as e:
            job.set_blend(_capi.MCS_BLEND_MULTIBAND)   # not a mode of set_blend, as before
        assert e.value.code == _capi.MCS_E_INVALID
        job.set_multiband(False)
        job.set_multiband(1)
        job.set_exposure(2)
        job.set_multiband(0)
    finally:
        job.close()


def test_capture_estimator_multiband_switch():
    est = estimate.CaptureEstimator(3, 96, 64, 3)
    assert est.multiband is False and est.blend == _capi.MCS_BLEND_NONE
    est.close()
    est = estimate.CaptureEstimator(3, 96, 64, 3, multiband=True)
    assert est.multiband is True and est.blend == _capi.MCS_BLEND_NONE
    est.close()
    est = estimate.CaptureEstimator(3, 96, 64, 3, multiband=True, exposure=2)
    assert est.multiband and est.exposure == 2
    est.close()
    for mode in (_capi.MCS_BLEND_SEAM, _capi.MCS_BLEND_FEATHER):
        with pytest.raises(ValueError):
            estimate.CaptureEstimator(3, 96, 64, 3, blend=mode, multiband=True)
        est = estimate.CaptureEstimator(3, 96, 64, 3, blend=mode, multiband=False)
        assert est.blend == mode and not est.multiband
        est.close()
    with pytest.raises(ValueError):                     # as before: not a blend= mode
        estimate.CaptureEstimator(3, 96, 64, 3, blend=_capi.MCS_BLEND_MULTIBAND)


def test_library_embeds_the_direct_multiband_kernels():
    blob = open(build.LIB, "rb").read()
    for name in (b"mcs_direct_mb_own_c3_i1\0", b"mcs_direct_mb_tile_c3_i1\0",
                 b"mcs_direct_mb_own_c3_i1_g\0", b"mcs_direct_mb_tile_c4_i0_g\0",
                 b"mcs_direct_mb_own_c1_i0\0", b"mcs_direct_mb_tile_c1_i0\0"):
        assert name in blob, name


def test_fourth_code_object_stays_out_of_the_build_id():
    here = os.path.dirname(build.LIB)
    assert build.DEVICE["direct_mb"] == "mcs_direct_mb.hip"
    assert tuple(build.ID_OBJECTS) == ("features", "stitch", "sweep")
    obj = os.path.join(here, f"mcs_direct_mb.{build.ARCH}.hsaco")
    assert os.path.exists(obj), "the build made no direct multi-band code object"
    secs = build._elf_sections(obj)
    assert len(secs[".text"]) > 0 and b"mcs_direct_mb_tile_c3_i1" in open(obj, "rb").read()
    three = [os.path.join(here, f"mcs_{n}.{build.ARCH}.hsaco")
             for n in ("features", "kernels", "sweep")]
    lib = open(build.LIB, "rb").read()
    assert build.code_id(three).encode() in lib
    assert _capi.load().mcs_build_id().decode() == build.code_id(three)
    assert build.code_id(sorted(three + [obj])).encode() not in lib
