"""Multi-band on the direct stitch path (mcs_stitch_direct_multiband[_gained], kernels
mcs_direct_mb_own_* / mcs_direct_mb_tile_*; the stitch of mcs_rig_job_wait_stitch after
mcs_rig_job_set_multiband) against its specification oracle/orc_blend.c and against the prepared
path.  Bar: max |diff| == 0.

The frames are rig.make_frames -- independent textures per camera: on frames of one world the
multi-band mosaic nearly equals the seam mosaic, and a kernel that stopped after its owner pass
would pass.  Every oracle-compared case first asserts, on the oracle alone, that MULTIBAND differs
from SEAM on at least 3 % of the mosaic's pixels and from FEATHER on at least 10 %.  The rig-job
test is the exception (ORB needs the cameras to see one world): there one camera's frame is
brightened, and the oracle's MULTIBAND and SEAM are asserted to differ.

Device results come back from sentinel-filled buffers; every byte outside the mosaic rows, and
the guards around the work area, must keep the sentinel.
"""
import functools

import numpy as np
import pytest

import gain_ref
from oracle import oracle
from test_gpu_direct_feather import (BATCH, DISTS, GUARD, SENTINEL, _diff, _frames, _lens, _plan,
                                     _upload)

pytestmark = pytest.mark.gpu

NONE, FEATHER, MULTIBAND, SEAM = 0, 1, 2, 3
TILE_W, TILE_H = 32, 64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from multicamera_stitching_amd import _capi
    assert _capi.device_count() >= 1, "GPU tests need an MI355X (no HIP device visible)"


def _differs(a, b):
    """Fraction of the mosaic's pixels on which two mosaics differ."""
    a = np.asarray(a)
    a = a.reshape(a.shape[0], a.shape[1], -1)
    return float((a != np.asarray(b).reshape(a.shape)).any(axis=-1).mean())


def _check_preconditions(mb, seam, feather, name=""):
    fs, ff = _differs(mb, seam), _differs(mb, feather)
    print(f"{name}: mosaic {np.asarray(mb).shape}, multiband != seam on {fs:.4f}, "
          f"!= feather on {ff:.4f} of the pixels")
    assert fs >= 0.03, fs
    assert ff >= 0.10, ff


# ---- device calls --------------------------------------------------------------------------------
def _work(nbytes, fill):
    import torch
    return torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")


def _check_work_guards(work, fill):
    got = work.cpu().numpy()
    assert (got[:GUARD] == fill).all() and (got[-GUARD:] == fill).all(), \
        "the kernel wrote outside the work area"


def _stitch(plan, batch, method="stitch_direct_multiband", out_off=0, pitch_pad=0, cam_pads=None,
            work=None, work_fill=SENTINEL):
    """batch[f][i]: frame f of camera i.  The batch through Plan.<method> into a sentinel-filled
    buffer (see test_gpu_direct_feather._stitch); the multi-band entry points get a work area of
    exactly the needed size between guards, pre-filled with work_fill (or the caller's `work`, a
    buffer of _work())."""
    import torch
    F, n_cams = len(batch), len(batch[0])
    row = plan.out_w * plan.channels
    pitch = row + pitch_pad
    fstride = plan.out_h * pitch
    cam_pads = cam_pads or [0] * n_cams
    ups = [_upload([batch[f][i] for f in range(F)], 0, cam_pads[i]) for i in range(n_cams)]
    out = torch.full((GUARD + out_off + F * fstride + GUARD,), SENTINEL, dtype=torch.uint8,
                     device="cuda")
    args = [[u[1] for u in ups], [u[2] for u in ups], out.data_ptr() + GUARD + out_off, pitch,
            fstride, F]
    if "multiband" in method:
        need = plan.direct_multiband_work_size()
        if work is None:
            work = _work(need, work_fill)
        assert work.numel() >= need + 2 * GUARD
        args += [work.data_ptr() + GUARD, work.numel() - 2 * GUARD]
    getattr(plan, method)(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if "multiband" in method:
        _check_work_guards(work, work_fill)
    got = out.cpu().numpy()
    body = got[GUARD + out_off:GUARD + out_off + F * fstride].reshape(F, plan.out_h, pitch)
    assert (got[:GUARD + out_off] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
    assert (body[:, :, row:] == SENTINEL).all(), "the kernel wrote outside the mosaic rows"
    return body[:, :, :row].copy()


# ---- 1. against the oracle -----------------------------------------------------------------------
CASES_1 = {
    # the eight rigs of test_gpu_blend.py::test_blend_vs_oracle
    "4x320x180x3": dict(n=4, w=320, h=180, ch=3, seed=3),
    "3x200x120x1-rot-persp": dict(n=3, w=200, h=120, ch=1, seed=4, rot_deg=4.0, persp=1e-4),
    "2x150x90x4-rot": dict(n=2, w=150, h=90, ch=4, seed=5, rot_deg=2.0),
    "3x160x100x3-nearest": dict(n=3, w=160, h=100, ch=3, seed=6, interp=0),
    "3x180x100x3-super": dict(n=3, w=180, h=100, ch=3, seed=7, super_mode=True, rot_deg=3.0),
    "2x40x20x2-narrow": dict(n=2, w=40, h=20, ch=2, seed=8, overlap=0.5),
    "4x64x48x3-overlap0.8": dict(n=4, w=64, h=48, ch=3, seed=10, overlap=0.8),
    "3x202x110x3-unaligned": dict(n=3, w=202, h=110, ch=3, seed=13),
    # narrow seams: 5 and 7 owners in one neighbourhood
    "5x40x30x3-step6": dict(n=5, w=40, h=30, ch=3, seed=11, step=6),
    "8x64x30x3-step5": dict(n=8, w=64, h=30, ch=3, seed=11, step=5),
    # dense: one tile with more than 8 owners in its neighbourhood takes the feather rule
    "10x64x30x3-step4-dense": dict(n=10, w=64, h=30, ch=3, seed=11, step=4),
    "12x48x30x3-step3-dense": dict(n=12, w=48, h=30, ch=3, seed=11, step=3),
}
DENSE = {"10x64x30x3-step4-dense": 4, "12x48x30x3-step3-dense": 3}     # blend tiles of the mosaic


@functools.lru_cache(maxsize=None)
def _want(name):
    """(multiband, seam, feather, owner map) of the oracle for a case of CASES_1, computed once."""
    case = dict(CASES_1[name])
    interp = case.get("interp", 1)
    plan, frames = _plan(blend=MULTIBAND, **case)
    flat = plan.describe()
    plan.close()
    mb, owner = oracle.blend_stitch(flat, frames, MULTIBAND, interp, want_owner=True)
    return (mb, oracle.blend_stitch(flat, frames, SEAM, interp),
            oracle.blend_stitch(flat, frames, FEATHER, interp), owner)


def _dense_tiles(owner):
    """The oracle's dense-seam rule on its owner map: blend tiles (32 x 64) whose neighbourhood
    (grown by 16 px, clipped) holds more than 8 owners; and the tile count."""
    oh, ow = owner.shape
    gx, gy = -(-ow // TILE_W), -(-oh // TILE_H)
    dense = []
    for ty in range(gy):
        for tx in range(gx):
            nb = owner[max(ty * TILE_H - 16, 0):ty * TILE_H + TILE_H + 16,
                       max(tx * TILE_W - 16, 0):tx * TILE_W + TILE_W + 16]
            if len(set(np.unique(nb).tolist()) - {255}) > 8:
                dense.append((tx, ty))
    return dense, gx * gy


@pytest.mark.parametrize("name", list(CASES_1))
def test_direct_multiband_vs_oracle(name):
    want, seam, feather, owner = _want(name)
    _check_preconditions(want, seam, feather, name)
    plan, frames = _plan(blend=MULTIBAND, **CASES_1[name])
    got = _stitch(plan, [frames])[0]
    assert _diff(got, want) == 0
    if name in DENSE:
        dense, n_tiles = _dense_tiles(owner)
        assert len(dense) == 1 and n_tiles == DENSE[name], (dense, n_tiles)
        tx, ty = dense[0]
        box = (slice(ty * TILE_H, (ty + 1) * TILE_H), slice(tx * TILE_W, (tx + 1) * TILE_W))
        got = got.reshape(want.shape)
        assert np.array_equal(got[box], feather[box]), "the dense tile is not feathered"
        rest = np.ones(want.shape[:2], bool)
        rest[box] = False
        assert not np.array_equal(got[rest], feather[rest]), "every tile is feathered"
    plan.close()


def test_cases_cover_one_owner_tiles_uncovered_pixels_and_tile_rows():
    """What the rigs above are chosen for, checked on the oracle's owner maps."""
    owner = _want("4x320x180x3")[3]
    oh, ow = owner.shape
    assert oh > 2 * TILE_H                           # several tile rows
    gx, gy = -(-ow // TILE_W), -(-oh // TILE_H)
    single = 0
    for ty in range(gy):
        for tx in range(gx):
            nb = owner[max(ty * TILE_H - 16, 0):ty * TILE_H + TILE_H + 16,
                       max(tx * TILE_W - 16, 0):tx * TILE_W + TILE_W + 16]
            single += len(set(np.unique(nb).tolist()) - {255}) <= 1
    print(f"4x320x180x3: {single} of {gx * gy} blend tiles with at most one owner")
    assert 0 < single < gx * gy
    uncovered = max(float((_want(n)[3] == 255).mean()) for n in CASES_1)
    print(f"most uncovered pixels of a case: {uncovered:.3f}")
    assert uncovered > 0.1
    narrow = _want("2x40x20x2-narrow")[3].shape
    assert narrow[0] < TILE_H and narrow[1] < 2 * TILE_W


# ---- 2. batches ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_want(f):
    plan, _ = _plan(blend=MULTIBAND, **BATCH)
    flat = plan.describe()
    plan.close()
    frames = _frames(3, 96, 64, 3, 20 + f)
    mb, seam, fea = (oracle.blend_stitch(flat, frames, m) for m in (MULTIBAND, SEAM, FEATHER))
    _check_preconditions(mb, seam, fea, f"batch capture {f}")
    return frames, mb


@pytest.mark.parametrize("cam_pads", [None, [0, 5, 0]], ids=["dense", "padded-camera-1"])
@pytest.mark.parametrize("F", [1, 4, 5, 9])
def test_batches_every_capture_vs_oracle(F, cam_pads):
    """Distinct frames per capture; F = 9 spans three blocks of kDirectFrames captures of the
    owner pass.  Dense strides: one pair of launches.  One camera's frame stride padded: a pair
    per frame."""
    plan, _ = _plan(blend=MULTIBAND, **BATCH)
    batch = [_batch_want(f)[0] for f in range(F)]
    got = _stitch(plan, batch, cam_pads=cam_pads)
    for f in range(F):
        assert _diff(got[f], _batch_want(f)[1]) == 0, f
    plan.close()


# ---- 3. output edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x202x110x3-unaligned", "2x150x90x4-rot", "2x40x20x2-narrow"])
def test_output_pitch_and_odd_base(name):
    """out_pitch larger than the row bytes and the mosaic base at an odd byte offset: the byte
    stores of both kernels; everything outside the mosaic rows keeps the sentinel."""
    plan, frames = _plan(blend=MULTIBAND, **CASES_1[name])
    want = _want(name)[0]
    got = _stitch(plan, [frames, frames], out_off=1, pitch_pad=7)
    assert _diff(got[0], want) == 0 and _diff(got[1], want) == 0
    got = _stitch(plan, [frames], out_off=4, pitch_pad=4)     # aligned again: the dword stores
    assert _diff(got[0], want) == 0
    plan.close()


# ---- 4. the work area ----------------------------------------------------------------------------
def test_work_area_needs_no_initialisation_and_is_reusable():
    """0xFF- and 0x00-filled areas give the same mosaic; one area serves a second plan of another
    geometry right after (same stream); its guard bytes keep their fill (_stitch checks)."""
    a_name, b_name = "4x320x180x3", "4x64x48x3-overlap0.8"
    plan_a, frames_a = _plan(blend=MULTIBAND, **CASES_1[a_name])
    plan_b, frames_b = _plan(blend=MULTIBAND, **CASES_1[b_name])
    for fill in (0xFF, 0x00):
        assert _diff(_stitch(plan_a, [frames_a], work_fill=fill)[0], _want(a_name)[0]) == 0
        assert _diff(_stitch(plan_b, [frames_b], work_fill=fill)[0], _want(b_name)[0]) == 0
    need_a, need_b = plan_a.direct_multiband_work_size(), plan_b.direct_multiband_work_size()
    assert need_a > need_b
    work = _work(need_a, 0x5C)
    for plan, frames, name in ((plan_a, frames_a, a_name), (plan_b, frames_b, b_name),
                               (plan_a, frames_a, a_name)):
        got = _stitch(plan, [frames], work=work, work_fill=0x5C)[0]
        assert _diff(got, _want(name)[0]) == 0, name
    plan_a.close()
    plan_b.close()


# ---- 5. equal to the prepared path ---------------------------------------------------------------
@pytest.mark.parametrize("lensed", [False, True], ids=["chain", "lensed-chain"])
@pytest.mark.parametrize("interp", [1, 0])
def test_direct_equals_prepared_chain(lensed, interp):
    """On one plan: stitch_direct_multiband == stitch_device after prepare.  Lensed: a
    non-trivial lens on every camera, camera 0 included."""
    case = dict(n=3, w=160, h=120, ch=3, seed=1, rot_deg=2.0, persp=5e-5, interp=interp)
    plan, frames = _plan(blend=MULTIBAND, **case)
    if lensed:
        for c in range(3):
            plan.set_lens(c, *_lens(160, 120, DISTS[c]))
        assert plan.stats()["lens_cams"] == 3
    batch = [frames, _frames(3, 160, 120, 3, 31)]
    a = _stitch(plan, batch)
    plan.prepare()
    b = _stitch(plan, batch, "stitch_device")
    assert np.array_equal(a, b)
    assert plan.stats()["blend"] == MULTIBAND and plan.stats()["blend_tiles"] > 0
    assert np.array_equal(_stitch(plan, batch), a)       # and again with the tables in place
    if not lensed:
        flat = plan.describe()
        want, seam, fea = (oracle.blend_stitch(flat, frames, m, interp)
                           for m in (MULTIBAND, SEAM, FEATHER))
        _check_preconditions(want, seam, fea, f"chain interp {interp}")
        assert _diff(a[0], want) == 0
    plan.close()


def test_direct_equals_prepared_chain_with_seam_hints():
    """Graph-cut labels on the plan: the owner is the label's camera where it covers the pixel."""
    plan, frames = _plan(3, 160, 120, 3, seed=1, rot_deg=2.0, persp=5e-5, blend=MULTIBAND)
    plan.find_seams(frames, scale_log2=2)
    lab = plan.seam_labels()
    assert lab is not None
    a = _stitch(plan, [frames])
    b = _stitch(plan, [frames], "stitch_device")
    assert np.array_equal(a, b)
    flat = plan.describe()
    want, seam, fea = (oracle.blend_stitch(flat, frames, m, seam_k=2, seam_labels=lab)
                       for m in (MULTIBAND, SEAM, FEATHER))
    _check_preconditions(want, seam, fea, "chain with hints")
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
    plan.set_blend(MULTIBAND)
    kw = {}
    if hints:
        plan.find_seams(frames, scale_log2=2)
        kw = dict(seam_k=2, seam_labels=plan.seam_labels())
        assert kw["seam_labels"] is not None
    want, seam, fea = (oracle.blend_stitch_cyl(cams, *geom, frames, m, **kw)
                       for m in (MULTIBAND, SEAM, FEATHER))
    _check_preconditions(want, seam, fea, f"cylinder hints={hints}")
    a = _stitch(plan, [frames, frames[::-1]])
    b = _stitch(plan, [frames, frames[::-1]], "stitch_device")
    assert np.array_equal(a, b)
    assert _diff(a[0], want) == 0
    plan.close()


# ---- 6. gains ------------------------------------------------------------------------------------
GAINS = [1.37, 1.0, 0.61]


@pytest.mark.parametrize("interp", [1, 0])
def test_gained_direct_multiband_vs_oracle_of_pregained_frames(interp):
    from multicamera_stitching_amd import _capi
    plan, _ = _plan(interp=interp, blend=MULTIBAND, **BATCH)
    F = 5
    batch = [_batch_want(f)[0] for f in range(F)]
    plain = _stitch(plan, batch)
    # gains disabled, and enabled with every q = 256: the ungained launch
    assert np.array_equal(_stitch(plan, batch, "stitch_direct_multiband_gained"), plain)
    plan.set_gains([1.0, 1.0, 1.0])
    assert np.array_equal(_stitch(plan, batch, "stitch_direct_multiband_gained"), plain)
    plan.set_gains(GAINS)
    got = _stitch(plan, batch, "stitch_direct_multiband_gained")
    flat = plan.describe()
    for f in range(F):
        pre = [gain_ref.apply_gain(c, g) for c, g in zip(batch[f], GAINS)]
        assert _diff(got[f], oracle.blend_stitch(flat, pre, MULTIBAND, interp)) == 0, f
    assert not np.array_equal(got, plain)
    # padded strides: the per-frame launches carry the gains too
    assert np.array_equal(
        _stitch(plan, batch, "stitch_direct_multiband_gained", cam_pads=[3, 0, 0]), got)
    # the ungained entry point never applies gains: refused
    with pytest.raises(_capi.McsError) as e:
        _stitch(plan, batch)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED
    plan.close()


def test_gained_direct_multiband_four_channels_lensed():
    """The _g twins through a lens, 4 channels: equal to the prepared path's gained multi-band."""
    plan, frames = _plan(2, 150, 90, 4, seed=5, rot_deg=2.0, blend=MULTIBAND)
    plan.set_lens(1, *_lens(150, 90, DISTS[0]))
    plan.set_gains([0.8, 1.25])
    a = _stitch(plan, [frames], "stitch_direct_multiband_gained")
    b = _stitch(plan, [frames], "stitch_device_gained")
    assert np.array_equal(a, b)
    plan.set_gains(None)
    assert not np.array_equal(_stitch(plan, [frames]), a)
    plan.close()


# ---- 7. the rig job ------------------------------------------------------------------------------
@pytest.mark.parametrize("exposure", [None, 2], ids=["plain", "exposure"])
def test_rig_job_multiband_equals_python_path_and_oracle(exposure):
    """mcs_rig_job_set_multiband(1): wait_stitch renders what CaptureEstimator(multiband=True)
    .stitch renders from the same homographies, which is the oracle's MULTIBAND of that geometry;
    a job without it still pastes.  One camera's frame is brightened by 24 (saturating) so that
    the blend shows on frames of one world: FAST and the rBRIEF comparisons do not see a constant
    offset.  exposure: the job's gained form equals the Python-issued gained path with the job's
    gains."""
    import torch
    from multicamera_stitching_amd import estimate, rig
    W, H, N = 960, 540, 4
    _, frames, _ = rig.estimation_rig(N, W, H, 3, seed=2)
    frames = [np.ascontiguousarray(f) for f in frames]
    frames[1] = np.minimum(frames[1].astype(np.int16) + 24, 255).astype(np.uint8)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(f).to(dev) for f in frames]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in d]
    pitch = 4096 * 3
    kw = dict(nfeatures=1000, exposure=exposure)
    a = estimate.CaptureEstimator(N, W, H, 3, multiband=True, **kw)
    b = estimate.CaptureEstimator(N, W, H, 3, multiband=True, **kw)
    c = estimate.CaptureEstimator(N, W, H, 3, **kw)
    try:
        out_a = torch.zeros((1024, pitch), dtype=torch.uint8, device=dev)
        out_b, out_c = torch.zeros_like(out_a), torch.zeros_like(out_a)
        b.submit(ptrs, 0, 0)
        oh, ow = b.collect_stitch(0, out_b.data_ptr(), pitch, out_b.numel())
        c.submit(ptrs, 0, 0)
        assert c.collect_stitch(0, out_c.data_ptr(), pitch, out_c.numel()) == (oh, ow)
        pair_H = a.estimate(ptrs)
        assert all(h is not None for h in pair_H), a.stats
        for x, y in zip(pair_H, b.homographies()):
            assert np.array_equal(x, y)
        stream = torch.cuda.current_stream().cuda_stream
        if exposure is None:
            plan = a.stitch(ptrs, pair_H, out_a.data_ptr(), pitch, out_a.numel(), stream)
            used = frames
        else:
            # the Python-issued gained path: the same plan, the job's gains, the gained entry
            plan, _ = a.plan(pair_H)
            plan.set_blend(MULTIBAND)
            plan.set_gains(b.gains)
            assert np.array_equal(plan.gains()[0], b.gains_q) and (b.gains_q != 256).any()
            work = a._mb_work(plan.direct_multiband_work_size())
            plan.stitch_direct_multiband_gained(ptrs, [W * H * 3] * N, out_a.data_ptr(), pitch,
                                                pitch * plan.out_h, 1, work.data_ptr(),
                                                work.numel(), stream)
            used = [gain_ref.apply_gain(f, g) for f, g in zip(frames, b.gains)]
        torch.cuda.synchronize()
        assert (oh, ow) == (plan.out_h, plan.out_w)
        assert torch.equal(out_a[:oh], out_b[:oh])
        flat = plan.describe()
        got = out_b[:oh, :ow * 3].cpu().numpy().reshape(oh, ow, 3)
        want = oracle.blend_stitch(flat, used, MULTIBAND)
        seam = oracle.blend_stitch(flat, used, SEAM)
        n_diff = int((want != seam).any(axis=-1).sum())
        print(f"rig job ({oh} x {ow}): multiband != seam on {n_diff} pixels")
        assert n_diff > 0
        assert _diff(got, want) == 0
        if exposure is None:
            paste = out_c[:oh, :ow * 3].cpu().numpy().reshape(oh, ow, 3)
            assert _diff(paste, oracle.flat_stitch(flat, frames)) == 0
            assert not np.array_equal(paste, got)
        plan.close()
    finally:
        a.close()
        b.close()
        c.close()
