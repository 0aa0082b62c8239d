"""Feather on the direct stitch path (mcs_stitch_direct[_gained] on a FEATHER plan, kernels
mcs_direct_feather_c*_i*[_g]; the stitch of mcs_rig_job_wait_stitch after mcs_rig_job_set_blend)
against its specification oracle/orc_blend.c and against the prepared path.  Bar: max |diff| == 0.

The frames are rig.make_frames -- independent textures per camera -- so that the feather mosaic
differs from the seam mosaic wherever two cameras overlap: every oracle-compared rig first
asserts, on the oracle alone, that the two differ on at least 10 % of the mosaic's pixels (a
kernel that wrote owners only could not pass).  The rig-job test is the exception: ORB needs the
cameras to see one world, so its overlaps nearly agree.

Device results come back from sentinel-filled buffers; every byte outside the mosaic rows must
keep the sentinel.
"""
import functools

import numpy as np
import pytest

import gain_ref
from oracle import oracle
from test_undistort_cpu import CASES

pytestmark = pytest.mark.gpu

NONE, FEATHER, MULTIBAND, SEAM = 0, 1, 2, 3
SENTINEL = 0xA5
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from multicamera_stitching_amd import _capi
    assert _capi.device_count() >= 1, "GPU tests need an MI355X (no HIP device visible)"


def _diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.size == b.size, (a.shape, b.shape)
    return int(np.abs(a.reshape(b.shape).astype(np.int16) - b.astype(np.int16)).max())


# ---- rigs ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rig(n, w, h, ch, seed, super_mode=False, **kw):
    """(stage descriptors, frames) of a chain rig calibrated with exact homographies; the frames
    are independent textures (rig.make_frames)."""
    from multicamera_stitching_amd import rig
    from multicamera_stitching_amd.StitcherClass import Stitcher, _stage_desc
    C = rig.camera_models(n, w, h, seed=seed, **kw)
    frames = rig.make_frames(n, w, h, ch, seed=seed)
    images = dict(zip(rig.labels(n), frames))
    st = Stitcher(images, super_mode=super_mode)
    st.calibrate_stitcher(images, save=False,
                          homographies=rig.homography_provider(C, lambda: st.stitchers))
    return [_stage_desc(sb) for sb in st.stitchers], [images[label] for label in st.img_labels]


def _plan(n, w, h, ch, seed, interp=1, blend=FEATHER, **kw):
    from multicamera_stitching_amd import _capi
    descs, frames = _rig(n, w, h, ch, seed, **kw)
    plan = _capi.Plan(descs, w, h, ch, interp)
    if blend != NONE:
        plan.set_blend(blend)
    return plan, frames


def _frames(n, w, h, ch, seed):
    from multicamera_stitching_amd import rig
    return rig.make_frames(n, w, h, ch, seed=seed)


def _feather_differs_from_seam(feather, seam):
    f = np.asarray(feather).reshape(seam.shape[0], seam.shape[1], -1)
    s = np.asarray(seam).reshape(f.shape)
    return float((f != s).any(axis=-1).mean())


# ---- device calls --------------------------------------------------------------------------------
def _upload(frames, off=0, pad=0):
    import torch
    n = frames[0].size
    stride = n + pad
    host = np.full(GUARD + off + len(frames) * stride + GUARD, SENTINEL, np.uint8)
    for f, fr in enumerate(frames):
        at = GUARD + off + f * stride
        host[at:at + n] = np.ascontiguousarray(fr).reshape(-1)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + GUARD + off, stride


def _stitch(plan, batch, method="stitch_direct", out_off=0, pitch_pad=0, cam_pads=None):
    """batch[f][i]: frame f of camera i.  The batch through Plan.<method> into a sentinel-filled
    buffer (mosaic base out_off bytes past the guard, rows pitch_pad bytes longer than the
    mosaic's, camera i's frames cam_pads[i] bytes apart beyond their size): (F, out_h, row)."""
    import torch
    F, n_cams = len(batch), len(batch[0])
    row = plan.out_w * plan.channels
    pitch = row + pitch_pad
    fstride = plan.out_h * pitch
    cam_pads = cam_pads or [0] * n_cams
    ups = [_upload([batch[f][i] for f in range(F)], 0, cam_pads[i]) for i in range(n_cams)]
    out = torch.full((GUARD + out_off + F * fstride + GUARD,), SENTINEL, dtype=torch.uint8,
                     device="cuda")
    getattr(plan, method)([u[1] for u in ups], [u[2] for u in ups],
                          out.data_ptr() + GUARD + out_off, pitch, fstride, F,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    body = got[GUARD + out_off:GUARD + out_off + F * fstride].reshape(F, plan.out_h, pitch)
    assert (got[:GUARD + out_off] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
    assert (body[:, :, row:] == SENTINEL).all(), "the kernel wrote outside the mosaic rows"
    return body[:, :, :row].copy()


# ---- 1. against the oracle -----------------------------------------------------------------------
CASES_1 = {
    "4x320x180x3": dict(n=4, w=320, h=180, ch=3, seed=3),
    "3x200x120x1-rot-persp": dict(n=3, w=200, h=120, ch=1, seed=4, rot_deg=4.0, persp=1e-4),
    "2x150x90x4-rot": dict(n=2, w=150, h=90, ch=4, seed=5, rot_deg=2.0),
    "3x160x100x3-nearest": dict(n=3, w=160, h=100, ch=3, seed=6, interp=0),
    "3x180x100x3-super": dict(n=3, w=180, h=100, ch=3, seed=7, super_mode=True, rot_deg=3.0),
    "2x40x20x2-narrow": dict(n=2, w=40, h=20, ch=2, seed=8, overlap=0.5),
    "3x202x110x3-unaligned": dict(n=3, w=202, h=110, ch=3, seed=13),
    "6x67x45x3-dense": dict(n=6, w=67, h=45, ch=3, seed=11, overlap=0.85),
}


@functools.lru_cache(maxsize=None)
def _want(name):
    """(feather, seam) of the oracle for a case of CASES_1, computed once."""
    case = dict(CASES_1[name])
    interp = case.get("interp", 1)
    plan, frames = _plan(**case)
    flat = plan.describe()
    plan.close()
    return (oracle.blend_stitch(flat, frames, FEATHER, interp),
            oracle.blend_stitch(flat, frames, SEAM, interp))


@pytest.mark.parametrize("name", list(CASES_1))
def test_direct_feather_vs_oracle(name):
    want, seam = _want(name)
    frac = _feather_differs_from_seam(want, seam)
    print(f"{name}: mosaic {want.shape}, feather != seam on {frac:.3f} of the pixels")
    assert frac >= 0.10, frac
    plan, frames = _plan(**CASES_1[name])
    got = _stitch(plan, [frames])[0]
    assert _diff(got, want) == 0
    plan.close()


def test_dense_rig_has_pixels_with_five_and_more_contributors():
    """The 6-camera rig at 85 % overlap: the oracle's contributor count per pixel (feather of
    indicator frames: camera j 255, the others 0 -- non-zero where camera j contributes) reaches
    5 and more, so a contributor limit or an accumulator mistake would show in its diff."""
    case = CASES_1["6x67x45x3-dense"]
    plan, frames = _plan(**case)
    flat = plan.describe()
    count = 0
    for j in range(case["n"]):
        ind = [np.full_like(f, 255 if i == j else 0) for i, f in enumerate(frames)]
        count = count + (oracle.blend_stitch(flat, ind, FEATHER)[..., 0] > 0).astype(np.int32)
    hist = np.bincount(count.ravel(), minlength=case["n"] + 1)
    print("contributors per pixel (0..6):", hist.tolist())
    assert hist[5:].sum() > 0 and plan.out_w < 128
    # the indicator frames through the kernel: the same counts
    got = 0
    for j in range(case["n"]):
        ind = [np.full_like(f, 255 if i == j else 0) for i, f in enumerate(frames)]
        got = got + (_stitch(plan, [ind])[0].reshape(count.shape + (3,))[..., 0] > 0)
    assert np.array_equal(got, count)
    plan.close()


# ---- 2. batches ----------------------------------------------------------------------------------
BATCH = dict(n=3, w=96, h=64, ch=3, seed=0, overlap=0.6)


@functools.lru_cache(maxsize=None)
def _batch_want(f):
    plan, _ = _plan(**BATCH)
    flat = plan.describe()
    plan.close()
    frames = _frames(3, 96, 64, 3, 20 + f)
    want, seam = (oracle.blend_stitch(flat, frames, m) for m in (FEATHER, SEAM))
    assert _feather_differs_from_seam(want, seam) >= 0.10
    return frames, want


@pytest.mark.parametrize("cam_pads", [None, [0, 5, 0]], ids=["dense", "padded-camera-1"])
@pytest.mark.parametrize("F", [1, 4, 5, 9])
def test_batches_every_capture_vs_oracle(F, cam_pads):
    """Distinct frames per capture; F = 9 spans three blocks of kDirectFrames captures.  Dense
    strides: one launch.  One camera's frame stride padded: the per-frame launches."""
    plan, _ = _plan(**BATCH)
    batch = [_batch_want(f)[0] for f in range(F)]
    got = _stitch(plan, batch, cam_pads=cam_pads)
    for f in range(F):
        assert _diff(got[f], _batch_want(f)[1]) == 0, f
    plan.close()


# ---- 3. output edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x202x110x3-unaligned", "2x150x90x4-rot", "2x40x20x2-narrow"])
def test_output_pitch_and_odd_base(name):
    """out_pitch larger than the row bytes and the mosaic base at an odd byte offset: the byte
    stores; everything outside the mosaic rows keeps the sentinel (_stitch checks it)."""
    plan, frames = _plan(**CASES_1[name])
    want = _want(name)[0]
    got = _stitch(plan, [frames, frames], out_off=1, pitch_pad=7)
    assert _diff(got[0], want) == 0 and _diff(got[1], want) == 0
    got = _stitch(plan, [frames], out_off=4, pitch_pad=4)     # aligned again: the dword stores
    assert _diff(got[0], want) == 0
    plan.close()


# ---- 4. equal to the prepared path ---------------------------------------------------------------
def _lens(w, h, dist, f=0.9):
    return ([[f * w, 0, w / 2 - 0.5 + 1.3], [0, f * w, h / 2 - 0.5 - 0.7], [0, 0, 1]], dist)


DISTS = [CASES[0]["d"], CASES[2]["d"], CASES[3]["d"]]     # 5, 8 and 12 coefficients


@pytest.mark.parametrize("lensed", [False, True], ids=["chain", "lensed-chain"])
@pytest.mark.parametrize("interp", [1, 0])
def test_direct_equals_prepared_chain(lensed, interp):
    """On one plan: stitch_direct == stitch_device (mcs_feather_* over the prepared tile list).
    Lensed: a non-trivial lens on every camera, camera 0 included."""
    case = dict(n=3, w=160, h=120, ch=3, seed=1, rot_deg=2.0, persp=5e-5, interp=interp)
    plan, frames = _plan(**case)
    if lensed:
        for c in range(3):
            plan.set_lens(c, *_lens(160, 120, DISTS[c]))
        assert plan.stats()["lens_cams"] == 3
    batch = [frames, _frames(3, 160, 120, 3, 31)]
    a = _stitch(plan, batch)
    b = _stitch(plan, batch, "stitch_device")
    assert np.array_equal(a, b)
    assert plan.stats()["blend"] == FEATHER and plan.stats()["blend_tiles"] > 0
    if not lensed:
        want = oracle.blend_stitch(plan.describe(), frames, FEATHER, interp)
        assert _diff(a[0], want) == 0
    plan.close()


def test_direct_equals_prepared_chain_with_seam_hints():
    """Graph-cut labels on the plan: where D == 0 the owner is the label's camera."""
    plan, frames = _plan(3, 160, 120, 3, seed=1, rot_deg=2.0, persp=5e-5)
    plan.find_seams(frames, scale_log2=2)
    lab = plan.seam_labels()
    assert lab is not None
    a = _stitch(plan, [frames])
    b = _stitch(plan, [frames], "stitch_device")
    assert np.array_equal(a, b)
    want = oracle.blend_stitch(plan.describe(), frames, FEATHER, seam_k=2, seam_labels=lab)
    assert _diff(a[0], want) == 0
    plan.close()


@functools.lru_cache(maxsize=None)
def _cyl():
    from multicamera_stitching_amd import rig
    cams, _, g = rig.cylinder_rig(8, 64, 36, 37.0, 3, seed=0)
    return cams, _frames(8, 64, 36, 3, 41), g


@pytest.mark.parametrize("hints", [False, True], ids=["distance", "graphcut-hints"])
def test_direct_equals_prepared_and_oracle_cylinder(hints):
    from multicamera_stitching_amd import _capi
    cams, frames, g = _cyl()
    geom = (g["out_w"], g["out_h"], g["f_cyl"], g["u0"], g["v0"])
    plan = _capi.Plan.cylindrical(cams, *geom, 3)
    plan.set_blend(FEATHER)
    kw = {}
    if hints:
        plan.find_seams(frames, scale_log2=2)
        kw = dict(seam_k=2, seam_labels=plan.seam_labels())
        assert kw["seam_labels"] is not None
    want = oracle.blend_stitch_cyl(cams, *geom, frames, FEATHER, **kw)
    seam = oracle.blend_stitch_cyl(cams, *geom, frames, SEAM, **kw)
    assert _feather_differs_from_seam(want, seam) >= 0.10
    a = _stitch(plan, [frames, frames[::-1]])
    b = _stitch(plan, [frames, frames[::-1]], "stitch_device")
    assert np.array_equal(a, b)
    assert _diff(a[0], want) == 0
    plan.set_blend(SEAM)           # a cylindrical SEAM plan takes the direct path as before
    assert _diff(_stitch(plan, [frames])[0], seam) == 0
    plan.close()


# ---- 5. gains ------------------------------------------------------------------------------------
GAINS = [1.37, 1.0, 0.61]


@pytest.mark.parametrize("interp", [1, 0])
def test_gained_direct_feather_vs_oracle_of_pregained_frames(interp):
    from multicamera_stitching_amd import _capi
    plan, _ = _plan(interp=interp, **BATCH)
    F = 5
    batch = [_batch_want(f)[0] for f in range(F)]
    plain = _stitch(plan, batch)
    # gains disabled, and enabled with every q = 256: the ungained launch
    assert np.array_equal(_stitch(plan, batch, "stitch_direct_gained"), plain)
    plan.set_gains([1.0, 1.0, 1.0])
    assert np.array_equal(_stitch(plan, batch, "stitch_direct_gained"), plain)
    plan.set_gains(GAINS)
    got = _stitch(plan, batch, "stitch_direct_gained")
    flat = plan.describe()
    for f in range(F):
        pre = [gain_ref.apply_gain(c, g) for c, g in zip(batch[f], GAINS)]
        assert _diff(got[f], oracle.blend_stitch(flat, pre, FEATHER, interp)) == 0, f
    assert not np.array_equal(got, plain)
    # padded strides: the per-frame launches carry the gains too
    assert np.array_equal(_stitch(plan, batch, "stitch_direct_gained", cam_pads=[3, 0, 0]), got)
    # the ungained entry point never applies gains: refused as ever
    with pytest.raises(_capi.McsError) as e:
        _stitch(plan, batch)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED
    plan.close()


def test_gained_direct_feather_four_channels_lensed():
    """The _g twin through a lens, 4 channels: equal to the prepared path's gained feather."""
    plan, frames = _plan(2, 150, 90, 4, seed=5, rot_deg=2.0)
    plan.set_lens(1, *_lens(150, 90, DISTS[0]))
    plan.set_gains([0.8, 1.25])
    a = _stitch(plan, [frames], "stitch_direct_gained")
    b = _stitch(plan, [frames], "stitch_device_gained")
    assert np.array_equal(a, b)
    plan.close()


# ---- 6. the rig job ------------------------------------------------------------------------------
def test_rig_job_feather_equals_python_path_and_oracle():
    """mcs_rig_job_set_blend(FEATHER): wait_stitch renders what CaptureEstimator.stitch renders
    from the same homographies with blend=FEATHER, which is the oracle's feather of that geometry;
    a job without set_blend still pastes."""
    import torch
    from multicamera_stitching_amd import _capi, estimate, rig
    W, H, N = 960, 540, 4
    _, frames, _ = rig.estimation_rig(N, W, H, 3, seed=2)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(f).to(dev) for f in frames]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in d]
    pitch = 4096 * 3
    a = estimate.CaptureEstimator(N, W, H, 3, nfeatures=1000, blend=_capi.MCS_BLEND_FEATHER)
    b = estimate.CaptureEstimator(N, W, H, 3, nfeatures=1000, blend=_capi.MCS_BLEND_FEATHER)
    c = estimate.CaptureEstimator(N, W, H, 3, nfeatures=1000)
    try:
        out_a = torch.zeros((1024, pitch), dtype=torch.uint8, device=dev)
        out_b, out_c = torch.zeros_like(out_a), torch.zeros_like(out_a)
        pair_H = a.estimate(ptrs)
        assert all(h is not None for h in pair_H), a.stats
        plan = a.stitch(ptrs, pair_H, out_a.data_ptr(), pitch, out_a.numel())
        b.submit(ptrs, 0, 0)
        oh, ow = b.collect_stitch(0, out_b.data_ptr(), pitch, out_b.numel())
        c.submit(ptrs, 0, 0)
        assert c.collect_stitch(0, out_c.data_ptr(), pitch, out_c.numel()) == (oh, ow)
        torch.cuda.synchronize()
        assert (oh, ow) == (plan.out_h, plan.out_w)
        for x, y in zip(pair_H, b.homographies()):
            assert np.array_equal(x, y)
        assert torch.equal(out_a[:oh], out_b[:oh])
        flat = plan.describe()
        got = out_b[:oh, :ow * 3].cpu().numpy().reshape(oh, ow, 3)
        assert _diff(got, oracle.blend_stitch(flat, frames, FEATHER)) == 0
        paste = out_c[:oh, :ow * 3].cpu().numpy().reshape(oh, ow, 3)
        assert _diff(paste, oracle.flat_stitch(flat, frames)) == 0
        assert not np.array_equal(paste, got)
        plan.close()
    finally:
        a.close()
        b.close()
        c.close()
