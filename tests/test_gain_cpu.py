"""Exposure gain compensation on the CPU: the host solver against the numpy reference
(tests/gain_ref.py), the gains a plan carries (quantisation, enabling, validation -- host state
only, no device), and Stitcher.set_gains."""
import ctypes
import functools

import numpy as np
import pytest

from multicamera_stitching_amd import _capi, rig

import gain_ref

SCALES = (0.8, 1.0, 1.25)


@functools.lru_cache(maxsize=None)
def scaled_rig():
    """The 3 x 96 x 64 x 3 chain at 60 % overlap (every camera pair overlaps), its world frames
    with camera i's exposure scaled by SCALES[i], and the reference statistics at every pixel
    (step_log2 = 0; the mosaic is 172 x 64 and N[0, 2] = 1197: the outer pair overlaps too)."""
    st, _, C = rig.calibrated_stitcher(3, 96, 64, 3, seed=0, overlap=0.6)
    frames = [np.clip(np.rint(f.astype(np.float64) * s), 0, 255).astype(np.uint8)
              for f, s in zip(rig.world_frames(C, 96, 64, 3, seed=0), SCALES)]
    plan = st.plan(3)
    N, S = gain_ref.chain_stats(plan.describe(), [frames], 0)
    return st, frames, N, S[0]


def test_solver_equals_reference_on_the_scaled_rig():
    st, frames, N, S = scaled_rig()
    plan = st.plan(3)
    assert (plan.out_w, plan.out_h) == (172, 64)
    assert N[0, 2] > 0            # the first and the last camera overlap: a triple-covered band
    assert (N == N.T).all() and (np.diag(N) >= N.max(axis=1)).all()
    want = gain_ref.solve(N, S, 3)
    got = _capi.gain_solve(N, S, 3)
    print("N =", N.tolist(), "gains =", got.tolist())
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
    # other constants, and one channel's worth of the same sums
    for alpha, beta, ch in ((0.05, 10.0, 3), (1.0, 1.0, 1), (0.01, 100.0, 4)):
        np.testing.assert_allclose(_capi.gain_solve(N, S, ch, alpha, beta),
                                   gain_ref.solve(N, S, ch, alpha, beta), rtol=1e-9, atol=0)


def test_solved_gains_reduce_the_mismatch():
    _, _, N, S = scaled_rig()
    g = _capi.gain_solve(N, S, 3)
    assert g[0] > g[1] > g[2]      # inverse to the injected 0.8, 1.0, 1.25
    before = gain_ref.mismatch(N, S, 3, np.ones(3))
    after = gain_ref.mismatch(N, S, 3, g)
    print("mismatch: %.1f with ones, %.1f with the solved gains" % (before, after))
    assert after < before


def test_solver_edge_cases():
    _, _, N, S = scaled_rig()
    # a camera that covers no grid point: left out of the system, gain 1
    N4 = np.zeros((4, 4), np.int64)
    S4 = np.zeros((4, 4), np.int64)
    keep = [0, 1, 3]
    N4[np.ix_(keep, keep)] = N
    S4[np.ix_(keep, keep)] = S
    g4 = _capi.gain_solve(N4, S4, 3)
    assert g4[2] == 1.0
    np.testing.assert_allclose(g4[keep], _capi.gain_solve(N, S, 3), rtol=1e-12)
    np.testing.assert_allclose(g4, gain_ref.solve(N4, S4, 3), rtol=1e-9)
    # no overlaps at all
    z = np.zeros((3, 3), np.int64)
    assert (_capi.gain_solve(z, z, 3) == 1.0).all()
    # cameras that cover points but share none: the prior alone, gain 1 each
    d = np.diag([10, 20, 30]).astype(np.int64)
    np.testing.assert_allclose(_capi.gain_solve(d, d * 300, 3), np.ones(3), rtol=1e-12)
    L = _capi.load()
    g = np.ones(3)
    assert L.mcs_gain_solve_host(3, None, None, 3, 0.01, 100.0, g.ctypes.data) == _capi.MCS_E_INVALID
    for bad in (dict(n=0), dict(ch=5), dict(alpha=float("nan")), dict(beta=-1.0)):
        rc = L.mcs_gain_solve_host(bad.get("n", 3), N.ctypes.data, S.ctypes.data, bad.get("ch", 3),
                                   bad.get("alpha", 0.01), bad.get("beta", 100.0), g.ctypes.data)
        assert rc == _capi.MCS_E_INVALID, bad


def test_quantisation_round_half_even_and_clamps():
    st, _, _, _ = scaled_rig()
    plan = st.plan(3)
    # 256 g at exact halves: 0.001953125 * 256 = 0.5 -> 0 -> clamped to 1; 1.001953125 -> 256.5
    # -> 256; 1.005859375 -> 257.5 -> 258; 1.298828125 -> 332.5 -> 332; 1.302734375 -> 333.5 -> 334
    cases = [(0.001953125, 1), (1.001953125, 256), (1.005859375, 258), (1.298828125, 332),
             (1.302734375, 334), (1.0, 256), (1e-9, 1), (255.998046875, 65535), (300.0, 65535),
             (1e300, 65535), (1.37, 351), (0.61, 156)]
    for i in range(0, len(cases), 3):
        chunk = cases[i:i + 3]
        plan.set_gains([g for g, _ in chunk])
        q, on = plan.gains()
        assert on and q.dtype == np.uint16
        assert q.tolist() == [w for _, w in chunk], chunk
        assert q.tolist() == [gain_ref.quantise(g) for g, _ in chunk]


def test_set_gains_enables_disables_and_validates():
    st, _, _, _ = scaled_rig()
    plan = st.plan(3)
    plan.set_gains(None)
    q, on = plan.gains()
    assert not on and q.tolist() == [256, 256, 256]
    plan.set_gains([1.0, 1.0, 1.0])               # identity is never dropped
    q, on = plan.gains()
    assert on and q.tolist() == [256, 256, 256]
    plan.set_gains([1.37, 1.0, 0.61])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_capi.McsError) as e:
            plan.set_gains([1.0, bad, 1.0])
        assert e.value.code == _capi.MCS_E_INVALID
        assert plan.gains()[0].tolist() == [351, 256, 156]   # a refused call changes nothing
    with pytest.raises(ValueError):
        plan.set_gains([1.0, 1.0])
    L = _capi.load()
    assert L.mcs_plan_set_gains(None, None) == _capi.MCS_E_INVALID
    assert L.mcs_plan_gains(None, None, None) == _capi.MCS_E_INVALID
    on = ctypes.c_int(-1)
    assert L.mcs_plan_gains(plan.handle, None, ctypes.byref(on)) == 0 and on.value == 1
    plan.set_gains(None)
    assert not plan.gains()[1]


@pytest.mark.parametrize("entry", ["stitch_device", "stitch_direct"])
def test_device_entry_points_refuse_a_gained_plan_without_a_device(entry):
    """They read the caller's frames and never write them; the refusal comes before any HIP
    call, so it is a status on a machine without a GPU too (the pointers are never used)."""
    st, _, _, _ = scaled_rig()
    plan = _capi.Plan([_capi_desc(sb) for sb in st.stitchers], 96, 64, 3)
    plan.set_gains([1.0, 1.0, 1.0])
    with pytest.raises(_capi.McsError) as e:
        getattr(plan, entry)([4096] * 3, [96 * 64 * 3] * 3, 4096, plan.out_w * 3, 0, 1)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED
    assert "mcs_gain_apply_device" in str(e.value)


def _capi_desc(sb):
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    return _stage_desc(sb)


def test_host_validation_of_stats_and_apply():
    """Everything refused before a device is touched."""
    L = _capi.load()
    N = np.zeros(9, np.int64)
    ptrs = (ctypes.c_void_p * 3)(4096, 4096, 4096)
    warp = _capi.Plan.warp(np.eye(3), 32, 24, 32, 24, 3)
    rc = L.mcs_plan_overlap_stats(warp.handle, ptrs, None, 1, 2, N.ctypes.data, N.ctypes.data, None)
    assert rc == _capi.MCS_E_UNSUPPORTED
    assert L.mcs_plan_overlap_stats_host(warp.handle, ptrs, 2, N.ctypes.data,
                                         N.ctypes.data) == _capi.MCS_E_UNSUPPORTED
    st, _, _, _ = scaled_rig()
    plan = st.plan(3)
    for n_frames, k in ((0, 2), (1, -1), (1, 5)):
        rc = L.mcs_plan_overlap_stats(plan.handle, ptrs, None, n_frames, k, N.ctypes.data,
                                      N.ctypes.data, None)
        assert rc == _capi.MCS_E_INVALID, (n_frames, k)
    assert L.mcs_plan_overlap_stats(plan.handle, None, None, 1, 2, N.ctypes.data, N.ctypes.data,
                                    None) == _capi.MCS_E_INVALID
    assert L.mcs_plan_overlap_stats_host(plan.handle, ptrs, 7, N.ctypes.data,
                                         N.ctypes.data) == _capi.MCS_E_INVALID
    apply = L.mcs_gain_apply_device
    assert apply(None, 4096, 16, 0, 0, 1, 256, 0, None) == _capi.MCS_E_INVALID
    assert apply(4096, 4096, 0, 0, 0, 1, 256, 0, None) == _capi.MCS_E_INVALID
    assert apply(4096, 4096, 16, 0, 0, 0, 256, 0, None) == _capi.MCS_E_INVALID
    assert apply(4096, 4096, 16, 0, 0, 1, 0, 0, None) == _capi.MCS_E_INVALID
    assert apply(4096, 4096 + 8, 16, 0, 0, 1, 256, 0, None) == _capi.MCS_E_INVALID   # partial overlap
    assert apply(4096, 4096, 16, 16, 32, 2, 256, 0, None) == _capi.MCS_E_INVALID     # other strides
    assert apply(4096, 8192, 16, 8, 0, 2, 256, 0, None) == _capi.MCS_E_INVALID       # stride < frame


def test_stitcher_set_gains(tmp_path):
    st, _, _ = rig.calibrated_stitcher(3, 96, 64, 3, seed=0, overlap=0.6)
    assert not st.plan(3).gains()[1]
    st.set_gains({"CAM3": 0.61, "CAM1": 1.37})      # sorted-label order: CAM1, CAM2, CAM3
    q, on = st.plan(3).gains()
    assert on and q.tolist() == [351, 256, 156]
    with pytest.raises(KeyError):
        st.set_gains({"CAM9": 1.0})
    with pytest.raises(ValueError):
        st.set_gains({"CAM1": 0.0})
    assert st.plan(3).gains()[0].tolist() == [351, 256, 156]
    # a rebuilt plan (the cache dropped, as after a calibration) carries the gains again
    first = st.plan(3)
    st._cache().key = None
    again = st.plan(3)
    assert again is not first and again.gains()[0].tolist() == [351, 256, 156]
    # not pickled: a loaded stitcher has no gains
    path = str(tmp_path / "Stitcher_config.pkl")
    st.save_stitcher(path)
    loaded = st.load_stitcher(path)
    assert loaded is not st and "_mcs_gains" not in loaded.__dict__
    assert not loaded.plan(3).gains()[1]
    assert st.plan(3).gains()[1]
    st.set_gains(None)
    assert not st.plan(3).gains()[1]
