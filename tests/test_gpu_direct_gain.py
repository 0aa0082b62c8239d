"""The table-free overlap statistics (mcs_plan_overlap_stats_direct[_async], kernels
mcs_direct_overlap_c*_i*) against the numpy reference (tests/gain_ref.py) and against the table
path (mcs_plan_overlap_stats), exactly: the arithmetic is integer throughout.  Then the rig job's
exposure step (mcs_rig_job_set_exposure: estimate, compensate, stitch in one call per capture)
against the oracle's feather of the pre-gained frames, with the gains the table path gives."""
import functools

import numpy as np
import pytest

from oracle import oracle

import gain_ref
import lens_ref
from test_gpu_gain import OV_FRAMES, SCALES, _captures, _chain_plan, _cyl, _cyl_plan, _lens1
from test_gpu_direct_feather import CASES_1, _diff
from test_gpu_direct_feather import _plan as _texture_plan

pytestmark = pytest.mark.gpu

FEATHER = 1
GUARD = 8                      # int64 guard words on each side of the _async buffer
GUARD_WORD = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from multicamera_stitching_amd import _capi
    assert _capi.device_count() >= 1, "GPU tests need an MI355X (no HIP device visible)"


def _torch():
    import torch
    return torch


def _upload(captures):
    """Device copies of the captures with test_gpu_gain._device_stats' frame strides: camera 0's
    frames dense, camera 1's 5 bytes apart (no multiple of 16), the others 48 bytes apart.
    Returns (buffers to keep alive, pointers, strides)."""
    torch = _torch()
    n_cams, F = len(captures[0]), len(captures)
    bufs, ptrs, strides = [], [], []
    for c in range(n_cams):
        nb = captures[0][c].size
        stride = nb + (0, 5, 48)[min(c, 2)]
        host = np.zeros(F * stride + 64, np.uint8)
        for f in range(F):
            host[f * stride:f * stride + nb] = captures[f][c].reshape(-1)
        t = torch.from_numpy(host).cuda()
        bufs.append(t)
        ptrs.append(t.data_ptr())
        strides.append(stride)
    torch.cuda.synchronize()
    return bufs, ptrs, strides


# ---- 1, 2. the statistics: reference and table path ----------------------------------------------
# (w, h, ch, interp, k, F, lens) of the 3-camera chain; "cyl": the 8-camera cylinder (k, F)
CHAIN = [(96, 64, 3, interp, k, F, False)
         for interp in (1, 0) for k in (0, 2) for F in (1, OV_FRAMES + 1)]
CHAIN += [
    (97, 61, 1, 1, 0, 1, False),                 # mosaic 174 x 61: no multiple of the step
    (97, 61, 1, 1, 2, OV_FRAMES + 1, False),
    (96, 64, 3, 1, 4, 2, False),                 # fewer grid points than one wave
    (96, 64, 4, 1, 2, 3, False),                 # 4 channels
    (96, 64, 4, 0, 0, 1, False),
    (96, 64, 3, 1, 0, 2, True),                  # the lensed camera 1
    (96, 64, 3, 1, 2, 1, True),
]
CASES = [("chain",) + c for c in CHAIN] + [("cyl", 0, OV_FRAMES + 1), ("cyl", 2, 1)]


def _case_id(case):
    if case[0] == "cyl":
        return "cyl-k%d-F%d" % case[1:]
    _, w, h, ch, interp, k, F, lens = case
    return "%dx%dx%d-i%d-k%d-F%d%s" % (w, h, ch, interp, k, F, "-lens" if lens else "")


def _build(case):
    """(plan, captures, k) of a case; a fresh plan per call."""
    if case[0] == "cyl":
        _, k, F = case
        _, frames, _ = _cyl()
        return _cyl_plan(), _captures(frames, F), k
    _, w, h, ch, interp, k, F, lens = case
    plan, frames = _chain_plan(w, h, ch, interp)
    if lens:
        plan.set_lens(1, *_lens1(w, h)[1])
    return plan, _captures(frames, F), k


@functools.lru_cache(maxsize=None)
def _want(case):
    """gain_ref's (N, S) of a case, computed once; with the guards of test_gpu_gain."""
    plan, caps, k = _build(case)
    if case[0] == "cyl":
        cams, _, g = _cyl()
        N, S = gain_ref.cyl_stats(cams, g, caps, k)
        assert N[0, 7] > 0 and N[0, 1] > 0 and N[0, 4] == 0      # the wrap; an empty pair
    else:
        _, w, h, ch, interp, _, _, lens = case
        if (w, h) == (97, 61):
            assert (plan.out_w, plan.out_h) == (174, 61)
        if k == 4:
            assert ((plan.out_w + 15) >> 4) * ((plan.out_h + 15) >> 4) < 64
        N, S = gain_ref.chain_stats(plan.describe(), caps, k, interp,
                                    _lens1(w, h) if lens else None)
        assert N[0, 2] > 0                                       # the triple-covered band
    F = len(caps)
    assert F == 1 or not np.array_equal(S[0], S[-1])             # the captures differ
    plan.close()
    N.setflags(write=False)
    S.setflags(write=False)
    return N, S


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_direct_stats_equal_reference(case):
    want_N, want_S = _want(case)
    plan, caps, k = _build(case)
    bufs, ptrs, strides = _upload(caps)
    N, S = plan.overlap_stats_direct(ptrs, strides, len(caps), k)
    assert np.array_equal(N, want_N), (N.tolist(), want_N.tolist())
    assert np.array_equal(S, want_S), (S - want_S).tolist()
    plan.close()


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_direct_stats_equal_table_path_and_leave_the_table_alone(case):
    """direct, table, direct, table on one plan and the same frames: all four equal.  The first
    direct call runs on a plan without a table, the second on one with it; the table call after
    it gives what it gave before (a dropped or damaged table would be rebuilt or differ)."""
    plan, caps, k = _build(case)
    bufs, ptrs, strides = _upload(caps)
    F = len(caps)
    before = plan.overlap_stats_direct(ptrs, strides, F, k)
    table = plan.overlap_stats(ptrs, strides, F, k)
    after = plan.overlap_stats_direct(ptrs, strides, F, k)
    again = plan.overlap_stats(ptrs, strides, F, k)
    for got in (before, after, again):
        assert np.array_equal(got[0], table[0]) and np.array_equal(got[1], table[1])
    # another step through the direct call does not touch the table of step k either
    other = plan.overlap_stats_direct(ptrs, strides, F, 3 if k != 3 else 1)
    assert not np.array_equal(other[0], table[0])
    again = plan.overlap_stats(ptrs, strides, F, k)
    assert np.array_equal(again[0], table[0]) and np.array_equal(again[1], table[1])
    plan.close()


# ---- 3. many contributors ------------------------------------------------------------------------
def test_dense_rig_every_pair_iteration():
    """The 6-camera rig at 85 % overlap: some grid point is covered by 5 and more cameras, so the
    pair loops run with most pairs live in one wave."""
    case = CASES_1["6x67x45x3-dense"]
    plan, frames = _texture_plan(**case)
    flat = plan.describe()
    pos, slot_cams, _ = lens_ref.chain_positions(flat)
    sizes = {c: (case["w"], case["h"]) for c in range(case["n"])}
    dist = lens_ref.distances(pos, slot_cams, sizes)
    for k in (0, 1):
        cover = sum((gain_ref.grid(d, k) >= 0).astype(np.int32) for d in dist)
        assert cover.max() >= 5, cover.max()
        caps = _captures(list(frames), 2)
        want_N, want_S = gain_ref.chain_stats(flat, caps, k)
        assert np.count_nonzero(want_N) >= 6 + 2 * 10                # most camera pairs overlap
        bufs, ptrs, strides = _upload(caps)
        N, S = plan.overlap_stats_direct(ptrs, strides, 2, k)
        assert np.array_equal(N, want_N), (N.tolist(), want_N.tolist())
        assert np.array_equal(S, want_S)
    plan.close()


# ---- 4. an unused camera -------------------------------------------------------------------------
def test_unused_camera_has_zero_rows_and_gain_one():
    """A chain whose last pair is uncalibrated: camera 2 is not in the mosaic.  Its rows and
    columns are zero (its frame pointer may be NULL) and the solver leaves it at gain 1."""
    from multicamera_stitching_amd import _capi, estimate, rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    from test_gpu_gain import _chain
    _, _, frames = _chain()
    C = rig.camera_models(3, 96, 64, seed=0, overlap=0.6)
    T = np.linalg.inv(C[0]) @ C[1]               # camera 1 -> camera 0
    pair_H = [T / T[2, 2], None]
    stages = estimate.chain_stages(pair_H, [(64, 96, 3)] * 3, False)
    plan = _capi.Plan([_stage_desc(sb) for sb in stages], 96, 64, 3, 1)
    caps = _captures(frames, 2)
    want_N, want_S = gain_ref.chain_stats(plan.describe(), caps, 1)
    assert want_N[0, 1] > 0 and not want_N[2].any() and not want_N[:, 2].any()
    bufs, ptrs, strides = _upload(caps)
    ptrs[2] = 0
    N, S = plan.overlap_stats_direct(ptrs, strides, 2, 1)
    assert np.array_equal(N, want_N) and np.array_equal(S, want_S)
    assert not S[:, 2].any() and not S[:, :, 2].any()
    g = _capi.gain_solve(N, S[0], 3)
    assert g[2] == 1.0 and g[0] != 1.0 and g[1] != 1.0
    np.testing.assert_allclose(g, gain_ref.solve(N, S[0], 3), rtol=1e-9, atol=0)
    plan.close()


# ---- 5. the enqueue-only form --------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1], CASES[-2]], ids=_case_id)
def test_async_equals_sync_inside_guards_and_outlives_the_plan(case):
    torch = _torch()
    plan, caps, k = _build(case)
    bufs, ptrs, strides = _upload(caps)
    F, n = len(caps), plan.n_cams
    want_N, want_S = plan.overlap_stats_direct(ptrs, strides, F, k)
    words = (1 + F) * n * n
    for destroy in (False, True):
        # (garbage in the body: the call zeroes it)
        buf = torch.full((GUARD + words + GUARD,), GUARD_WORD, dtype=torch.int64, device="cuda")
        if destroy:
            plan.close()
            plan, _, _ = _build(case)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        plan.overlap_stats_direct_async(ptrs, strides, F, k, buf.data_ptr() + 8 * GUARD, stream)
        if destroy:
            plan.close()                           # right after the enqueue
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:GUARD] == GUARD_WORD).all() and (got[-GUARD:] == GUARD_WORD).all()
        body = got[GUARD:GUARD + words]
        assert np.array_equal(body[:n * n].reshape(n, n), want_N), destroy
        assert np.array_equal(body[n * n:].reshape(F, n, n), want_S), destroy


# ---- 6, 7. the rig job ---------------------------------------------------------------------------
W, H, NC = 960, 540, 4
RIG_SCALES = SCALES + (1.0,)
PITCH = 4096 * 3


@functools.lru_cache(maxsize=None)
def _rig_frames(order):
    """The estimation rig's frames with camera i's exposure scaled by RIG_SCALES[order[i]]."""
    from multicamera_stitching_amd import rig
    _, frames, _ = rig.estimation_rig(NC, W, H, 3, seed=2)
    return tuple(np.clip(np.rint(f.astype(np.float64) * RIG_SCALES[o]), 0, 255).astype(np.uint8)
                 for f, o in zip(frames, order))


def _estimator(**kw):
    from multicamera_stitching_amd import _capi, estimate
    return estimate.CaptureEstimator(NC, W, H, 3, nfeatures=1000, blend=_capi.MCS_BLEND_FEATHER,
                                     **kw)


def _mosaic(out, shape):
    oh, ow = shape
    return out[:oh, :ow * 3].cpu().numpy().reshape(oh, ow, 3)


def test_rig_job_exposure_end_to_end():
    """CaptureEstimator(blend=FEATHER, exposure=2).collect_stitch: the mosaic is the oracle's
    feather of the frames pre-gained with the q that mcs_gain_solve_host gives on the table
    path's statistics of a Python-built plan for the same homographies."""
    torch = _torch()
    from multicamera_stitching_amd import _capi
    frames = _rig_frames((0, 1, 2, 3))
    d = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in d]
    a, b = _estimator(exposure=2), _estimator()
    try:
        out_a = torch.zeros((1024, PITCH), dtype=torch.uint8, device="cuda")
        out_b = torch.zeros_like(out_a)
        a.submit(ptrs, 0, 0)
        shape = a.collect_stitch(0, out_a.data_ptr(), PITCH, out_a.numel())
        b.submit(ptrs, 0, 0)
        assert b.collect_stitch(0, out_b.data_ptr(), PITCH, out_b.numel()) == shape
        torch.cuda.synchronize()
        pair_H = a.homographies()
        assert all(h is not None for h in pair_H), a.stats
        for x, y in zip(pair_H, b.homographies()):
            assert np.array_equal(x, y)
        plan, _ = a.plan(pair_H)
        plan.set_blend(FEATHER)
        assert (plan.out_h, plan.out_w) == shape
        flat = plan.describe()
        # on the CPU first: the scales give at least two cameras a q other than the identity
        ref_N, ref_S = gain_ref.chain_stats(flat, [list(frames)], 2)
        ref_g = gain_ref.solve(ref_N, ref_S[0], 3)
        ref_q = [gain_ref.quantise(g) for g in ref_g]
        print("reference gains", ref_g.tolist(), "q", ref_q)
        assert sum(q != 256 for q in ref_q) >= 2, ref_q
        # the table path's statistics of the Python-built plan, the library's solver
        N, S = plan.overlap_stats(ptrs, [f.size for f in frames], 1, 2)
        assert np.array_equal(N, ref_N) and np.array_equal(S, ref_S)
        gains = _capi.gain_solve(N, S[0], 3)
        q, _ = plan.set_gains(gains).gains()
        print("gains", gains.tolist(), "q", q.tolist())
        assert np.array_equal(a.gains, gains), (a.gains.tolist(), gains.tolist())
        assert np.array_equal(a.gains_q, q) and q.tolist() == ref_q
        np.testing.assert_allclose(a.gains, ref_g, rtol=1e-9, atol=0)
        job_g, job_q, on = a._jobs[0].gains()
        assert on and np.array_equal(job_g, gains) and np.array_equal(job_q, q)
        pre = [gain_ref.apply_q(f, qi) for f, qi in zip(frames, q)]
        got = _mosaic(out_a, shape)
        assert _diff(got, oracle.blend_stitch(flat, pre, FEATHER)) == 0
        plain = _mosaic(out_b, shape)
        assert _diff(plain, oracle.blend_stitch(flat, list(frames), FEATHER)) == 0
        assert not np.array_equal(got, plain)
        plan.close()
    finally:
        a.close()
        b.close()


def test_rig_job_exposure_batch_of_two_equals_two_single_jobs():
    torch = _torch()
    caps = [_rig_frames((0, 1, 2, 3)), _rig_frames((2, 1, 0, 3))]
    d = [[torch.from_numpy(f).cuda() for f in frames] for frames in caps]
    torch.cuda.synchronize()
    ptrs = [[t.data_ptr() for t in ds] for ds in d]
    one, two = _estimator(exposure=2), _estimator(exposure=2, captures_per_job=2)
    try:
        outs1 = [torch.zeros((1024, PITCH), dtype=torch.uint8, device="cuda") for _ in range(2)]
        outs2 = [torch.zeros_like(o) for o in outs1]
        shapes1, gains1, q1 = [], [], []
        for f in range(2):
            one.submit(ptrs[f], 0, 0)
            shapes1.append(one.collect_stitch(0, outs1[f].data_ptr(), PITCH, outs1[f].numel()))
            gains1.append(one.gains.copy())
            q1.append(one.gains_q.copy())
        two.submit(ptrs[0] + ptrs[1], 0, 0)
        shapes2 = two.collect_stitch(0, [o.data_ptr() for o in outs2], PITCH, outs2[0].numel())
        torch.cuda.synchronize()
        assert list(shapes2) == shapes1
        g2, q2, on = two._jobs[0].gains()
        assert on and g2.shape == (2, NC)
        assert np.array_equal(g2, np.stack(gains1)) and np.array_equal(q2, np.stack(q1))
        assert not np.array_equal(q2[0], q2[1]) and (q2 != 256).sum() >= 4
        assert np.array_equal(two.gains, gains1[1])
        for f in range(2):
            assert torch.equal(outs1[f], outs2[f]), f
        assert not torch.equal(outs2[0], outs2[1])
    finally:
        one.close()
        two.close()


def test_rig_job_exposure_off_is_todays_path():
    """A job never given set_exposure, and one given set_exposure(2) then set_exposure(-1): the
    mosaic of the Python path (Plan + stitch_direct) for the same homographies, gains 1."""
    torch = _torch()
    frames = _rig_frames((0, 1, 2, 3))
    d = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in d]
    ref, never, off = _estimator(), _estimator(), _estimator()
    try:
        out_r = torch.zeros((1024, PITCH), dtype=torch.uint8, device="cuda")
        pair_H = ref.estimate(ptrs)
        plan = ref.stitch(ptrs, pair_H, out_r.data_ptr(), PITCH, out_r.numel())
        off._job(0).set_exposure(2)
        off._job(0).set_exposure(-1)
        for est in (never, off):
            out = torch.zeros_like(out_r)
            est.submit(ptrs, 0, 0)
            shape = est.collect_stitch(0, out.data_ptr(), PITCH, out.numel())
            torch.cuda.synchronize()
            assert shape == (plan.out_h, plan.out_w)
            assert torch.equal(out, out_r)
            g, q, on = est._jobs[0].gains()
            assert not on and np.all(g == 1.0) and np.all(q == 256)
            assert np.all(est.gains == 1.0)
        plan.close()
    finally:
        ref.close()
        never.close()
        off.close()
