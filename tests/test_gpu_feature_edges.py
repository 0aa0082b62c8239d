"""The feature kernels at their size, quota, tie and degenerate edges (the table of
tests/feature_edges.py; test_feature_edges_cpu.py holds every case to its property on the oracle):

ORB through mcs_orb_detect_host against the CPU restatement -- count, level, position, response and
descriptors bit for bit -- on levels of 1 px to 600 x 800, widths of every residue mod 4, the
reflecting and the interior tiles, the one-launch pyramid and the per-level resize chain, 64|65,
128|129 and 4096|4097 candidates on a level (the sort network's sizes; device | host ranking) with
and without ties, thresholds 0 .. 255, the zero-moment orientation, and nfeatures so small that
OpenCV's rounded quotas add up to more than nfeatures (nothing may be written past nfeatures
entries); device-resident frames at odd sizes and byte offsets.  Hamming kNN-2 at distance 256 and
train indices past 2^16, L2 kNN-2 at its largest distances and on small float sets, RANSAC on
degenerate sets and at hypothesis / point counts around the wave and block sizes, and the rig job
at pairs of 0 .. 5 matches against the per-call path."""
import ctypes

import numpy as np
import pytest

import feature_edges as fe
from oracle import oracle

pytestmark = pytest.mark.gpu


def _same_as_oracle(got, want):
    assert len(got["xy"]) == len(want["xy"])
    assert np.array_equal(got["level"], want["level"])
    assert np.array_equal(got["xy"], want["xy"])
    assert np.array_equal(got["response"], want["response"].astype(np.float32))
    assert np.array_equal(got["desc"], want["desc"])
    ang = np.rad2deg(np.arctan2(want["cs_sn"][:, 1], want["cs_sn"][:, 0])) % 360
    assert np.allclose(got["angle"], ang, atol=1e-3)


_ORACLE = {}


def _oracle_orb(case):
    """The oracle's result of a table case, computed once and left unchanged."""
    if case["name"] not in _ORACLE:
        _ORACLE[case["name"]] = oracle.orb_detect(case["image"](), threshold=case["threshold"],
                                                  **fe.orb_kwargs(case))
    return _ORACLE[case["name"]]


@pytest.mark.parametrize("name", [c["name"] for c in fe.ORB_CASES])
def test_orb_edge_vs_oracle(name):
    from multicamera_stitching_amd import _capi
    case = fe.ORB_BY_NAME[name]
    got = _capi.orb_detect(case["image"](), fast_threshold=case["threshold"], **fe.orb_kwargs(case))
    want = _oracle_orb(case)
    fe.check_orb_property(case, want)
    _same_as_oracle(got, want)
    if "cs_sn" in case:      # the zero-moment orientation (1, 0): exactly 0 degrees
        assert got["angle"][0] == 0.0


GUARD = 0xA5


@pytest.mark.parametrize("name", fe.NFEATURES_CASES)
@pytest.mark.parametrize("device_input", [False, True])
def test_orb_writes_nothing_past_nfeatures(name, device_input):
    """The output arrays hold nfeatures entries and a guard tail: at most nfeatures keypoints come
    back, the tail is untouched, and the entries are the oracle's."""
    import torch
    from multicamera_stitching_amd import _capi
    case = fe.ORB_BY_NAME[name]
    img = np.ascontiguousarray(case["image"]())
    h, w = img.shape
    nf, tail = case["nfeatures"], 16
    L = _capi.load()
    bufs = {k: np.full(((nf + tail) * per,), GUARD, np.uint8)
            for k, per in [("xy", 8), ("response", 4), ("angle", 4), ("level", 4), ("desc", 32)]}
    n = ctypes.c_int(-1)
    if device_input:
        d = torch.from_numpy(img).to("cuda:0")
        torch.cuda.synchronize()
        fn, src = L.mcs_orb_detect_device, ctypes.c_void_p(d.data_ptr())
    else:
        fn, src = L.mcs_orb_detect_host, img.ctypes.data
    _capi.check(fn(src, w, h, 1, nf, case["nlevels"], float(case["scale_factor"]),
                   case["threshold"], bufs["xy"].ctypes.data, bufs["response"].ctypes.data,
                   bufs["angle"].ctypes.data, bufs["level"].ctypes.data, bufs["desc"].ctypes.data,
                   ctypes.byref(n), 0))
    assert 0 <= n.value <= nf
    for k, per in [("xy", 8), ("response", 4), ("angle", 4), ("level", 4), ("desc", 32)]:
        assert (bufs[k][nf * per:] == GUARD).all(), k
    want = _oracle_orb(case)
    k = n.value
    got = dict(xy=bufs["xy"][:8 * k].view(np.float32).reshape(k, 2),
               response=bufs["response"][:4 * k].view(np.float32),
               angle=bufs["angle"][:4 * k].view(np.float32),
               level=bufs["level"][:4 * k].view(np.int32),
               desc=bufs["desc"][:32 * k].reshape(k, 32))
    _same_as_oracle(got, want)


def test_device_and_host_ranking_agree_at_the_boundary():
    """4096 candidates rank on the device, 4097 on the host: the 4097-dot lattice gives the
    4096-dot lattice's keypoints, in its order, plus the extra dot (descriptors compared away from
    the extra dot, which lies inside its neighbours' patches)."""
    from multicamera_stitching_amd import _capi
    a = _capi.orb_detect(fe.lattice(4096), nfeatures=5000, nlevels=1)
    b = _capi.orb_detect(fe.lattice(4097), nfeatures=5000, nlevels=1)
    assert len(a["xy"]) == 4096 and len(b["xy"]) == 4097
    extra = fe.lattice_xy(4097)[4096]
    assert np.array_equal(b["xy"][4096], extra)
    for key in ("xy", "level", "response"):
        assert np.array_equal(a[key], b[key][:4096]), key
    far = np.abs(a["xy"] - extra).max(axis=1) > 40
    assert far.sum() > 4000
    assert np.array_equal(a["desc"][far], b["desc"][:4096][far])
    assert np.array_equal(a["angle"][far], b["angle"][:4096][far])


def _bgr_of(gray):
    """A BGR frame with distinct channels whose OpenCV gray is close to `gray`."""
    g = gray.astype(np.int32)
    return np.clip(np.stack([g + 9, g - 2, g + 1], axis=-1), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("h,w,seed", [(67, 65, 14), (65, 65, 3)])
def test_orb_gray_tail_pixels(h, w, seed):
    """w h = 3 and 1 mod 4: the gray conversion's last thread converts byte by byte.  Device input
    equals host input equals the oracle on OpenCV's gray."""
    import torch
    from multicamera_stitching_amd import _capi
    assert (w * h) % 4 in (1, 3)
    gray = fe.noise(h, w, seed)
    gray[31, 31] = 255     # (a bright dot on an eligible pixel: a keypoint whatever the noise gives)
    bgr = _bgr_of(gray)
    want = oracle.orb_detect(fe.opencv_gray(bgr), nfeatures=100, nlevels=2)
    assert len(want["xy"]) > 0
    host = _capi.orb_detect(bgr, nfeatures=100, nlevels=2)
    d = torch.from_numpy(bgr).to("cuda:0")
    torch.cuda.synchronize()
    dev = _capi.orb_detect_device(d.data_ptr(), w, h, 3, nfeatures=100, nlevels=2)
    _same_as_oracle(host, want)
    for key in ("xy", "response", "angle", "level", "desc"):
        assert np.array_equal(host[key], dev[key]), key


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_orb_device_frame_at_byte_offset(channels, offset):
    """A 200 x 240 frame at byte offsets 1, 2, 3 inside a device buffer: the gray conversion's
    byte path (3 channels), an unaligned level-0 copy (1 channel)."""
    import torch
    from multicamera_stitching_amd import _capi
    w, h = 200, 240
    gray = fe.noise(h, w)
    frame = _bgr_of(gray) if channels == 3 else gray
    want = oracle.orb_detect(fe.opencv_gray(frame) if channels == 3 else gray, nfeatures=300,
                             nlevels=3)
    assert len(want["xy"]) == 300
    buf = torch.zeros(frame.size + 8, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 4 == 0
    buf[offset:offset + frame.size] = torch.from_numpy(frame.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    dev = _capi.orb_detect_device(buf.data_ptr() + offset, w, h, channels, nfeatures=300,
                                  nlevels=3)
    host = _capi.orb_detect(frame, nfeatures=300, nlevels=3)
    _same_as_oracle(dev, want)
    for key in ("xy", "response", "angle", "level", "desc"):
        assert np.array_equal(host[key], dev[key]), key


# ---- Hamming -------------------------------------------------------------------------------------

def test_hamming_distance_256():
    from multicamera_stitching_amd import _capi
    q, t, idx, dist = fe.hamming_complement()
    gi, gd = _capi.match_hamming_knn2(q, t)
    assert np.array_equal(gi, idx) and np.array_equal(gd, dist)


@pytest.mark.parametrize("nq", [1, 65])
def test_hamming_train_indices_past_2_16(nq):
    from multicamera_stitching_amd import _capi
    q, t, idx, dist = fe.hamming_far_indices(nq)
    gi, gd = _capi.match_hamming_knn2(q, t)
    assert np.array_equal(gi, idx) and np.array_equal(gd, dist)
    wi, wd = oracle.hamming_knn2(q, t)
    assert np.array_equal(gi, wi) and np.array_equal(gd, wd)


def test_hamming_ties_straddling_2_16():
    from multicamera_stitching_amd import _capi
    q, t, idx, dist = fe.hamming_straddle()
    gi, gd = _capi.match_hamming_knn2(q, t)
    assert np.array_equal(gi, idx) and np.array_equal(gd, dist)


# ---- L2 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 64, 128, 256])
def test_l2_largest_distance(dim):
    from multicamera_stitching_amd import _capi
    q, t, idx, far = fe.l2_extremes(dim)
    gi, gd, exact = _capi.match_l2_knn2(q, t)
    wi, wd, _ = oracle.l2_knn2(q, t)
    assert exact
    assert np.array_equal(gi, idx) and np.array_equal(gi, wi)
    assert (gd[:, 0] == 0).all() and (gd[:, 1] == far).all()
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("nt", [1, 15, 17, 257])
@pytest.mark.parametrize("dim", [1, 33, 200, 256])
def test_l2_float_path_small_sets(dim, nt):
    """The f32 path (one non-integer value in the train set alone takes the call off the exact
    path; negative values) against the float64 brute force, at test_l2_float_path_tolerance's
    tolerances."""
    from multicamera_stitching_amd import _capi
    q, t = fe.l2_float_case(dim, nt)
    idx, dist, exact = _capi.match_l2_knn2(q, t)
    assert not exact
    true = np.sqrt(((q[:, None, :].astype(np.float64) - t[None]) ** 2).sum(-1))
    k = min(2, nt)
    srt = np.sort(true, axis=1)[:, :k]
    assert (idx[:, :k] >= 0).all() and (idx[:, :k] < nt).all()
    got_true = np.take_along_axis(true, idx[:, :k].astype(np.int64), 1)
    err = np.abs(got_true - srt).max(), np.abs(dist[:, :k] - got_true).max()
    print(f"dim {dim} nt {nt}: neighbour error {err[0]:.3g}, distance error {err[1]:.3g}")
    assert np.allclose(got_true, srt, rtol=1e-4, atol=1e-4)        # true nearest two
    assert np.allclose(dist[:, :k], got_true, rtol=1e-4, atol=1e-3)  # their distances
    if nt == 1:
        assert (idx[:, 1] == -1).all() and (dist[:, 1] == -1).all()
    else:
        assert (idx[:, 0] != idx[:, 1]).all()


# ---- RANSAC --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", fe.RANSAC_DEGENERATE + fe.RANSAC_SIZES)
def test_ransac_edge_vs_oracle(name):
    from multicamera_stitching_amd import _capi
    src, dst, iters, seed, has_model = fe.ransac_case(name)
    H, mask = _capi.ransac_homography(src, dst, 3.0, iters=iters, seed=seed)
    Hw, maskw, best, _ = oracle.ransac_homography(src, dst, 3.0, iters=iters, seed=seed)
    if has_model is not None:
        assert (Hw is not None) == has_model
    assert (H is None) == (Hw is None)
    assert np.array_equal(mask.reshape(-1), maskw)
    if H is not None:
        assert np.array_equal(H, Hw), H - Hw


# ---- the rig job at small counts -----------------------------------------------------------------

def _job_equals_calls(frames, w, h, channels, **kw):
    """CaptureEstimator's rig job (one launch chain) against its per-call steps issued from
    Python: homographies, their None-ness and the keypoint / match / inlier counts."""
    import torch
    from multicamera_stitching_amd import estimate
    n = len(frames)
    d = [torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0") for f in frames]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in d]
    est = estimate.CaptureEstimator(n, w, h, channels, **kw)
    try:
        py = est.estimate_from(est.features(ptrs))
        py_stats = dict(est.stats)
        est.last_H = [None] * (n - 1)
        job = est.estimate(ptrs)
        job_stats = dict(est.stats)
        # the job ran as the launch chain, not through its per-call fallback
        assert est._jobs[0].counts() == (1, 0)
        assert job_stats == py_stats, (job_stats, py_stats)
        for a, b in zip(py, job):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(a, b)
        return py, py_stats
    finally:
        est.close()


def test_rig_job_lattice_cameras():
    """Five cameras holding 0, 1, 2, 5 and 40 lattice dots: a pair without train keypoints, one
    without a second neighbour, and pairs whose equal descriptors tie (no match passes the strict
    ratio test): every pair is refused in mcs_rig_hyp / mcs_rig_ransac / mcs_rig_best."""
    frames = fe.lattice_rig()
    h, w = frames[0].shape
    kps, pairs = fe.oracle_pairs(frames, nfeatures=64, nlevels=1)
    py, stats = _job_equals_calls(frames, w, h, 1, nfeatures=64, nlevels=1, iters=100)
    assert stats["keypoints"] == kps == [0, 1, 2, 5, 40]
    assert stats["matches"] == [len(s) for s, _ in pairs] == [0, 0, 0, 0]
    assert stats["inliers"] == [0, 0, 0, 0] and all(H is None for H in py)


@pytest.mark.parametrize("w,h,seed,nfeatures", fe.RIG_SMALL)
def test_rig_job_small_rigs(w, h, seed, nfeatures):
    """Three-camera rigs so small that the pairs have a handful of matches (feature_edges.RIG_SMALL
    lists what each comes to): the n <= 4 refusals, every hypothesis rejected, and the
    first-of-the-maximum rule among tied scores whose models differ.  The job equals the per-call
    steps, and both the oracle's keypoint and match counts and its RANSAC."""
    from multicamera_stitching_amd import rig
    _, frames, _ = rig.estimation_rig(3, w, h, 3, seed=seed)
    kps, pairs = fe.oracle_pairs(frames, nfeatures, 3)
    py, stats = _job_equals_calls(frames, w, h, 3, nfeatures=nfeatures, nlevels=3)
    print(w, h, seed, nfeatures, stats)
    assert stats["keypoints"] == kps
    assert stats["matches"] == [len(s) for s, _ in pairs]
    for k, (src, dst) in enumerate(pairs):
        Hw, maskw = None, np.zeros(0)
        if len(src) > 4:
            Hw, maskw, _, _ = oracle.ransac_homography(src, dst, 3.0, iters=2000, seed=0)
        assert (py[k] is None) == (Hw is None)
        assert stats["inliers"][k] == int(maskw.sum())
        if Hw is not None:
            assert np.array_equal(py[k], Hw)
    if (w, h, seed, nfeatures) in fe.RIG_TIED:
        assert py[0] is not None and stats["inliers"][0] == 4


def test_rig_job_resize_chain():
    """A three-camera job whose levels step by 2.0 (feature_edges.RIG_CHAIN): the one-launch
    pyramid declines, so the job issues the per-level resize with a frame stride over the cameras
    and plain launches instead of its graph.  The job equals the per-call steps (asserted with
    counts() == (1, 0) in _job_equals_calls), and both the oracle's keypoint and match counts and
    its RANSAC."""
    from multicamera_stitching_amd import rig
    w, h, seed, nfeatures = fe.RIG_CHAIN
    _, frames, _ = rig.estimation_rig(3, w, h, 3, seed=seed)
    kps, pairs = fe.oracle_pairs(frames, nfeatures, 3, scale_factor=2.0)
    py, stats = _job_equals_calls(frames, w, h, 3, nlevels=3, scale_factor=2.0,
                                  nfeatures=nfeatures)
    print(w, h, seed, nfeatures, stats)
    assert stats["keypoints"] == kps == fe.RIG_CHAIN_KEYPOINTS
    assert stats["matches"] == [len(s) for s, _ in pairs] == fe.RIG_CHAIN_MATCHES
    for k, (src, dst) in enumerate(pairs):
        Hw, maskw, _, _ = oracle.ransac_homography(src, dst, 3.0, iters=2000, seed=0)
        assert (py[k] is None) == (Hw is None)
        assert stats["inliers"][k] == int(maskw.sum())
        if Hw is not None:
            assert np.array_equal(py[k], Hw)
