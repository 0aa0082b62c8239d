"""Rig jobs on raw frames (mcs_rig_job_set_lens, CaptureEstimator(lenses=...)): the estimator is
fed the frames distorted cameras deliver, carries the matched keypoints through the inverse lens
(csrc/mcs_lens_core.h lens_invert; numpy specification tests/lens_inv_ref.py) and stitches with a
lensed per-capture plan.  The device path (one launch chain), the per-call path
(MCS_RIG_PATH=calls) and the steps issued from Python agree bit for bit; the identity lens changes
nothing; matches without a valid inverse are dropped and counted out; a batch job takes camera
c's lens for camera c of every capture; collect_stitch renders what the Python-built lensed plan
renders and what tests/lens_ref.py specifies; and the homographies found on the raw frames are as
good as the ones the lens-free job finds on the clean frames.

Raw frames are made here from rig.estimation_rig's clean frames (lens_inv_ref.raw_frame):
raw[p] = bilinear(clean, lens_inv_ref.lens_invert(p)), zero where the inverse is NaN, the clean
view's nearest edge pixel where a barrel lens sees past its edge."""
import functools

import numpy as np
import pytest

import gain_ref
import lens_inv_ref
import lens_ref
from lens_inv_ref import NOPRE
from test_gpu_estimate import _reproj_err
from test_gpu_lens import DISTS, IDENTITY, _diff, _lens

pytestmark = pytest.mark.gpu

W, H, N, NF = 640, 360, 4, 1000
SEED = 2
PITCH = 4096 * 3
NONE, FEATHER = 0, 1
# a different lens per camera (5, 8 and 12 coefficients), camera 2 left without
LENSES = {0: _lens(W, H, DISTS[0]), 1: _lens(W, H, DISTS[1]), 3: _lens(W, H, DISTS[2])}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from multicamera_stitching_amd import _capi
    assert _capi.device_count() >= 1, "GPU tests need an MI355X (no HIP device visible)"


@functools.lru_cache(maxsize=None)
def _rig(w=W, h=H):
    from multicamera_stitching_amd import rig
    _, frames, truth = rig.estimation_rig(N, w, h, 3, seed=SEED)
    return tuple(frames), tuple(truth)


@functools.lru_cache(maxsize=None)
def _raw(w=W, h=H):
    """The raw frames of LENSES' cameras (camera 2: its clean frame)."""
    clean, _ = _rig(w, h)
    out = tuple(lens_inv_ref.raw_frame(f, *LENSES[c]) if c in LENSES else f
                for c, f in enumerate(clean))
    for f in out:
        f.setflags(write=False)
    return out


def _upload(frames):
    import torch
    d = [torch.from_numpy(np.array(f, np.uint8)).cuda() for f in frames]
    torch.cuda.synchronize()
    return d, [t.data_ptr() for t in d]


def _estimator(w=W, h=H, **kw):
    from multicamera_stitching_amd import estimate
    return estimate.CaptureEstimator(N, w, h, 3, nfeatures=NF, **kw)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        assert x is None or np.array_equal(x, y)


def _fresh(est, ptrs):
    """One capture through est's rig job, with no estimate carried over: (pair_H, stats)."""
    est.last_H = [None] * (N - 1)
    pair_H = est.estimate(ptrs)
    return pair_H, dict(est.stats)


# ---- 1. the three paths ----------------------------------------------------------------------
def test_device_path_equals_call_path_equals_python_steps(monkeypatch):
    monkeypatch.delenv("MCS_RIG_PATH", raising=False)
    bufs, ptrs = _upload(_raw())
    est, plain = _estimator(lenses=LENSES), _estimator()
    try:
        py = est.estimate_from(est.features(ptrs))
        py_stats = dict(est.stats)
        print("python-issued", py_stats)
        assert all(h is not None for h in py), py_stats
        job, job_stats = _fresh(est, ptrs)
        assert est._jobs[0].counts() == (1, 0)
        assert job_stats == py_stats
        _same(py, job)
        monkeypatch.setenv("MCS_RIG_PATH", "calls")
        calls, calls_stats = _fresh(est, ptrs)
        monkeypatch.delenv("MCS_RIG_PATH")
        assert est._jobs[0].counts() == (1, 1)
        assert calls_stats == py_stats
        _same(py, calls)
        # replays of the captured graph: the lens table and the positions' buffer are the job's
        for i in range(4):
            again, again_stats = _fresh(est, ptrs)
            assert again_stats == py_stats
            _same(py, again)
        assert est._jobs[0].counts() == (5, 1)
        # the lenses matter on these frames, and removing them gives the lens-free job
        want, want_stats = _fresh(plain, ptrs)
        assert any(not np.array_equal(a, b) for a, b in zip(want, py))
        est.set_lenses({})
        got, got_stats = _fresh(est, ptrs)
        assert est._jobs[0].counts() == (6, 1)
        assert got_stats == want_stats
        _same(want, got)
        est.last_H = [None] * (N - 1)
        _same(want, est.estimate_from(est.features(ptrs)))
        assert dict(est.stats) == want_stats
        # and setting them again gives the lensed result again (a new graph with the table)
        est.set_lenses(LENSES)
        back, back_stats = _fresh(est, ptrs)
        assert back_stats == py_stats
        _same(py, back)
        # while a capture is in flight a lens is refused, and the capture is not disturbed (a
        # capture takes milliseconds, the call microseconds: it is in flight here)
        from multicamera_stitching_amd import _capi
        est.last_H = [None] * (N - 1)
        est.submit(ptrs)
        with pytest.raises(_capi.McsError) as e:
            est._jobs[0].set_lens(2, *LENSES[0])
        assert e.value.code == _capi.MCS_E_INVALID
        _same(py, est.collect())
        assert est.stats == py_stats
    finally:
        est.close()
        plain.close()


# ---- 2. the identity lens --------------------------------------------------------------------
def test_identity_lens_changes_nothing(monkeypatch):
    monkeypatch.delenv("MCS_RIG_PATH", raising=False)
    clean, _ = _rig()
    bufs, ptrs = _upload(clean)
    ident = {0: _lens(W, H, None), 1: _lens(W, H, [0.0] * 5), 2: IDENTITY,
             3: _lens(W, H, [0.0] * 12)}
    est, plain = _estimator(lenses=ident), _estimator()
    try:
        want, want_stats = _fresh(plain, ptrs)
        got, got_stats = _fresh(est, ptrs)
        assert all(h is not None for h in want), want_stats
        assert est._jobs[0].counts() == (1, 0) and plain._jobs[0].counts() == (1, 0)
        assert got_stats == want_stats
        _same(want, got)
        monkeypatch.setenv("MCS_RIG_PATH", "calls")
        calls, calls_stats = _fresh(est, ptrs)
        assert est._jobs[0].counts() == (1, 1)
        assert calls_stats == want_stats
        _same(want, calls)
    finally:
        est.close()
        plain.close()


# ---- 3. matches without a valid inverse ------------------------------------------------------
def _predicted_matches(est, feats, lenses):
    """Per pair: (matches the ratio test passes, those of them both of whose positions
    lens_inv_ref inverts) from the capture's features."""
    from multicamera_stitching_amd import _capi, estimate
    out = []
    for k in range(N - 1):
        fa, fb = feats[k + 1], feats[k]
        idx, dist = _capi.match_hamming_knn2(fa["desc"], fb["desc"])
        q = estimate.ratio_filter(idx, dist, est.ratio)
        keep = np.ones(len(q), bool)
        for cam, xy in ((k + 1, fa["xy"][q]), (k, fb["xy"][idx[q, 0]])):
            if cam in lenses:
                xy = np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2)
                u, _ = lens_inv_ref.lens_invert(*lenses[cam], xy[:, 0], xy[:, 1])
                keep &= ~np.isnan(u)
        out.append((len(q), int(keep.sum())))
    return out


def test_matches_without_an_inverse_are_dropped(monkeypatch):
    """NOPRE on camera 1 only, 320 x 240: the matches of pairs 0 and 1 whose camera-1 position has
    no preimage are dropped, on both paths, and n_matches is what lens_inv_ref predicts.

    Camera 1 is fed its CLEAN frame here, not lens_inv_ref.raw_frame of it: NOPRE's valid disc
    (radius 0.703 x 200 px) ends where the clean frame's corners land (radius 1.0 -> 0.700), so
    the frame raw_frame makes is black everywhere outside the disc and ORB finds nothing there
    (measured: 0 of 628 keypoints without an inverse, the case passes vacuously).  The estimator
    cannot tell what a frame shows; with the clean frame camera 1 has keypoints in its corners,
    beyond the disc, that match its neighbours' (measured: 1 of 25 and 3 of 36 ratio-passing
    matches).  This case counts matches; the geometry is test_lensed_job_finds_...'s."""
    monkeypatch.delenv("MCS_RIG_PATH", raising=False)
    w, h = NOPRE["w"], NOPRE["h"]
    lenses = {1: (NOPRE["K"], NOPRE["d"])}
    clean, _ = _rig(w, h)
    frames = list(clean)
    spec = lens_inv_ref.raw_frame(clean[1], *lenses[1])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, _ = lens_inv_ref.lens_invert(*lenses[1], x, y)
    assert np.isnan(u).any() and not spec[np.isnan(u)].any()     # (black beyond the disc)
    bufs, ptrs = _upload(frames)
    est, plain = _estimator(w, h, lenses=lenses), _estimator(w, h)
    try:
        pred = _predicted_matches(est, est.features(ptrs), lenses)
        print("ratio-passing / with an inverse, per pair:", pred)
        # pairs 0 and 1 use camera 1; it cannot pass vacuously: matches of both have no inverse
        assert pred[0][1] < pred[0][0] and pred[1][1] < pred[1][0], pred
        assert pred[2][1] == pred[2][0]
        _, free_stats = _fresh(plain, ptrs)
        assert free_stats["matches"] == [p[0] for p in pred]
        dev, dev_stats = _fresh(est, ptrs)
        assert est._jobs[0].counts() == (1, 0)
        assert dev_stats["matches"] == [p[1] for p in pred]
        assert all(a < b for a, b in zip(dev_stats["matches"][:2], free_stats["matches"][:2]))
        monkeypatch.setenv("MCS_RIG_PATH", "calls")
        calls, calls_stats = _fresh(est, ptrs)
        assert est._jobs[0].counts() == (1, 1)
        assert calls_stats == dev_stats
        _same(dev, calls)
        monkeypatch.delenv("MCS_RIG_PATH")
        est.last_H = [None] * (N - 1)
        py = est.estimate_from(est.features(ptrs))
        assert dict(est.stats) == dev_stats
        _same(dev, py)
    finally:
        est.close()
        plain.close()


# ---- 4. a batch job --------------------------------------------------------------------------
def test_batch_job_takes_each_cameras_lens_in_every_capture():
    import torch
    from multicamera_stitching_amd import _capi
    bufs, ptrs0 = _upload(_raw())
    rolled = [torch.roll(t, shifts=(5, 7), dims=(0, 1)).contiguous() for t in bufs]
    torch.cuda.synchronize()
    caps = [ptrs0, [t.data_ptr() for t in rolled]]
    single, batch = _capi.RigJob(N, W, H, 3, NF), _capi.RigJob(N, W, H, 3, NF, captures=2)
    try:
        for job in (single, batch):
            for cam, (K, d) in LENSES.items():
                job.set_lens(cam, K, d)
        want = []
        for q in range(2):
            single.submit(caps[q])
            want.append(single.wait())
        batch.submit(caps[0] + caps[1])
        got = batch.wait()
        assert single.counts() == (2, 0) and batch.counts() == (1, 0)
        assert len(got) == 2
        for (Hw, sw), (Hg, sg) in zip(want, got):
            assert sw == sg
            assert all(h is not None for h in Hw), sw
            _same(Hw, Hg)
        assert not np.array_equal(want[0][0][0], want[1][0][0])      # the captures differ
    finally:
        single.close()
        batch.close()


# ---- 5. the stitch ---------------------------------------------------------------------------
def _mosaic(out, shape):
    oh, ow = shape
    return out[:oh, :ow * 3].cpu().numpy().reshape(oh, ow, 3)


@pytest.mark.parametrize("mode", [NONE, FEATHER], ids=["paste", "feather"])
def test_collect_stitch_renders_the_lensed_plan(mode):
    import torch
    raw = _raw()
    bufs, ptrs = _upload(raw)
    a, b = _estimator(lenses=LENSES, blend=mode), _estimator(lenses=LENSES, blend=mode)
    try:
        out_a = torch.zeros((768, PITCH), dtype=torch.uint8, device="cuda")
        out_b = torch.zeros_like(out_a)
        pair_H = a.estimate(ptrs)
        assert all(h is not None for h in pair_H), a.stats
        plan = a.stitch(ptrs, pair_H, out_a.data_ptr(), PITCH, out_a.numel())
        assert plan.stats()["lens_cams"] == len(LENSES)
        b.submit(ptrs, 0, 0)
        shape = b.collect_stitch(0, out_b.data_ptr(), PITCH, out_b.numel())
        torch.cuda.synchronize()
        assert shape == (plan.out_h, plan.out_w)
        _same(pair_H, b.homographies())
        assert torch.equal(out_a, out_b)
        flat = plan.describe()
        pos, slot_cams, rects = lens_ref.chain_positions(flat, 1, LENSES)
        if mode == NONE:
            want = lens_ref.render_paste(pos, slot_cams, rects, list(raw))
        else:
            want = lens_ref.render_blend(pos, slot_cams, list(raw), "feather")
        assert want.any() and _diff(_mosaic(out_b, shape), want) == 0
        plan.close()
    finally:
        a.close()
        b.close()


def test_collect_stitch_with_exposure_equals_the_two_steps():
    """exposure=2: the gains are the solver's on the table path's statistics of the Python-built
    lensed plan, and the mosaic is the specification's feather of the pre-gained raw frames (and
    what that plan renders with the gains set)."""
    import torch
    from multicamera_stitching_amd import _capi
    scales = (0.8, 1.0, 1.25, 1.0)
    raw = [np.clip(np.rint(f.astype(np.float64) * s), 0, 255).astype(np.uint8)
           for f, s in zip(_raw(), scales)]
    bufs, ptrs = _upload(raw)
    a = _estimator(lenses=LENSES, blend=FEATHER, exposure=2)
    try:
        out_a = torch.zeros((768, PITCH), dtype=torch.uint8, device="cuda")
        out_b = torch.zeros_like(out_a)
        a.submit(ptrs, 0, 0)
        shape = a.collect_stitch(0, out_a.data_ptr(), PITCH, out_a.numel())
        torch.cuda.synchronize()
        pair_H = a.homographies()
        assert all(h is not None for h in pair_H), a.stats
        plan, _ = a.plan(pair_H)
        plan.set_blend(FEATHER)
        assert (plan.out_h, plan.out_w) == shape and plan.stats()["lens_cams"] == len(LENSES)
        Nn, S = plan.overlap_stats(ptrs, [f.size for f in raw], 1, 2)
        gains = _capi.gain_solve(Nn, S[0], 3)
        q, _ = plan.set_gains(gains).gains()
        print("gains", gains.tolist(), "q", q.tolist())
        assert sum(int(v) != 256 for v in q) >= 2
        assert np.array_equal(a.gains, gains) and np.array_equal(a.gains_q, q)
        plan.stitch_direct_gained(ptrs, [f.size for f in raw], out_b.data_ptr(), PITCH,
                                  PITCH * plan.out_h, 1)
        torch.cuda.synchronize()
        assert torch.equal(out_a[:shape[0]], out_b[:shape[0]])
        flat = plan.describe()
        pos, slot_cams, _ = lens_ref.chain_positions(flat, 1, LENSES)
        pre = [gain_ref.apply_q(f, qi) for f, qi in zip(raw, q)]
        want = lens_ref.render_blend(pos, slot_cams, pre, "feather")
        assert _diff(_mosaic(out_a, shape), want) == 0
        plan.close()
    finally:
        a.close()


# ---- 6. the geometry -------------------------------------------------------------------------
def test_lensed_job_finds_the_clean_rigs_geometry():
    """Per pair: e_lens, the reprojection error against the rig's truth of the lensed job on the
    raw frames, against e_clean, that of the lens-free job on the clean frames (same seeds):
    e_lens <= max(2 e_clean, e_clean + 1 px).  Printed beside them, not asserted: the lens-free
    job on the raw frames -- what the caller had without the lenses.
    Measured on an MI355X, pairs 0, 1, 2 (DESIGN.md section 5 "Rig lens"): e_clean 1.765 / 7.525 /
    1.253 px, e_lens 1.447 / 3.331 / 0.918 px, lens-free on the raw frames 19.180 / 6.401 /
    24.483 px.  With the raw frames black where the lens sees past the clean view (instead of
    its edge pixel, see lens_inv_ref.raw_frame) pair 0 has 11 matches fewer and e_lens = 3.854 px,
    over its bound of 3.530 px; pairs 1 and 2 are the same."""
    clean, truth = _rig()
    cb, cptrs = _upload(clean)
    rb, rptrs = _upload(_raw())
    lensed, plain = _estimator(lenses=LENSES), _estimator()
    try:
        Hc, sc = _fresh(plain, cptrs)
        Hn, sn = _fresh(plain, rptrs)
        Hl, sl = _fresh(lensed, rptrs)
        print("clean frames, no lens:", sc)
        print("raw frames, lenses:   ", sl)
        print("raw frames, no lens:  ", sn)
        errs = []
        for k in range(N - 1):
            assert Hc[k] is not None and Hl[k] is not None, (k, sc, sl)
            e_clean = _reproj_err(Hc[k], truth[k], W, H)
            e_lens = _reproj_err(Hl[k], truth[k], W, H)
            e_none = _reproj_err(Hn[k], truth[k], W, H) if Hn[k] is not None else float("nan")
            print("pair %d: e_clean %.4f px, e_lens %.4f px, lens-free on raw %.4f px"
                  % (k, e_clean, e_lens, e_none))
            errs.append((k, e_clean, e_lens))
        for k, e_clean, e_lens in errs:
            assert e_lens <= max(2 * e_clean, e_clean + 1.0), errs
    finally:
        lensed.close()
        plain.close()
