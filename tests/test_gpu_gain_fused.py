"""Exposure gains fused into the stitch kernels (mcs_stitch_device_gained,
mcs_stitch_direct_gained): the gained stitch of the caller's RAW device frames against the
ungained stitch of frames pre-gained in numpy (tests/gain_ref.py apply_q) -- a second plan of the
same geometry -- and, once per blend mode, against the oracle on the pre-gained frames.  Every
comparison is for equality.  Every case also checks that the caller's device frames are unchanged
by the call, that the result differs from the ungained stitch of the raw frames, and (before the
GPU is used) that at least one source byte clamps at 255 under its camera's q.

The shapes are the smallest that reach each kernel: the streaming kernel and its frame-edge byte
stores, the large-footprint and direct-gather side lists, the feather kernel, the multi-band
levels kernel (mosaics under 128 rows), the band pass in its LDS-ring and global-window forms, the
wider blend kernels' plans, the cylinder map and a lensed camera."""
import functools

import numpy as np
import pytest

from oracle import oracle

import gain_ref

pytestmark = pytest.mark.gpu

NONE, FEATHER, MULTIBAND, SEAM = 0, 1, 2, 3
GAINS = [1.37, 1.0, 0.61]                 # q = 351, 256, 156: brighter, identity, darker
MORE_GAINS = GAINS + [1.21, 0.83, 1.09, 0.74, 1.3]
EXTRA = (0, 5, 48)                        # frame stride - frame bytes of camera 0, 1, 2 (and up)


@pytest.fixture(autouse=True)
def _band_pass(monkeypatch):
    """The default multi-band path (the sweep is opt-in; its test sets the variable itself)."""
    monkeypatch.setenv("MCS_MB_SWEEP", "0")


def _torch():
    import torch
    return torch


def _full_range(frame):
    """The frame's levels stretched to 0..255 (the rigs' textures stop well short of 255: under
    q = 351 nothing would clamp)."""
    lo, hi = int(frame.min()), int(frame.max())
    return np.rint((frame.astype(np.float64) - lo) * (255.0 / max(hi - lo, 1))).astype(np.uint8)


def _captures(frames, n):
    """n captures of the full-range frames, each with different frames (the others: capture 0
    rolled sideways, every camera by its own amount)."""
    frames = [_full_range(c) for c in frames]
    return [[np.ascontiguousarray(np.roll(c, 5 * f + i * f, axis=1)) if f else c
             for i, c in enumerate(frames)] for f in range(n)]


def _pre(captures, gains):
    return [[gain_ref.apply_gain(c, g) for c, g in zip(frames, gains)] for frames in captures]


def _clamps(captures, gains):
    """Some source byte clamps at 255 under its camera's q (numpy only)."""
    for frames in captures:
        for c, g in zip(frames, gains):
            if (((c.astype(np.int64) * gain_ref.quantise(g) + 128) >> 8) > 255).any():
                return True
    return False


def _stitch(plan, method, captures, extra=EXTRA):
    """getattr(plan, method) on device copies of the captures (camera c's frames extra[min(c, 2)]
    bytes apart beyond their size): the mosaics (F, out_h, out_w * ch), after checking that the
    call left every byte of the camera buffers as it was."""
    torch = _torch()
    F, n = len(captures), len(captures[0])
    ch = captures[0][0].shape[2] if captures[0][0].ndim == 3 else 1
    hosts, bufs, strides = [], [], []
    for c in range(n):
        nb = captures[0][c].size
        stride = nb + extra[min(c, len(extra) - 1)]
        host = np.full(F * stride + 64, 0xA5, np.uint8)
        for f in range(F):
            host[f * stride:f * stride + nb] = captures[f][c].reshape(-1)
        hosts.append(host)
        bufs.append(torch.from_numpy(host).cuda())
        strides.append(stride)
    out = torch.zeros((F, plan.out_h, plan.out_w * ch), dtype=torch.uint8, device="cuda")
    getattr(plan, method)([b.data_ptr() for b in bufs], strides, out.data_ptr(), plan.out_w * ch,
                          out[0].numel(), F, 0)
    torch.cuda.synchronize()
    for b, host in zip(bufs, hosts):
        assert np.array_equal(b.cpu().numpy(), host), "the call wrote the caller's frames"
    return out.cpu().numpy()


def _check(make, captures, gains, mode, method="stitch_device", extra=EXTRA, want_oracle=None):
    """The common assertions; returns the gained plan (for stats)."""
    assert _clamps(captures, gains)
    pre = _pre(captures, gains)
    plan = make().set_gains(gains)
    plain = make()
    if mode != NONE:
        plan.set_blend(mode)
        plain.set_blend(mode)
    got = _stitch(plan, method + "_gained", captures, extra)
    want = _stitch(plain, method, pre, extra)
    raw = _stitch(plain, method, captures, extra)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    assert not np.array_equal(got, raw)
    if want_oracle is not None:
        ref = want_oracle(pre[0])
        assert np.array_equal(got[0].reshape(ref.shape), ref)
    plain.close()
    return plan


# ---- rigs ----------------------------------------------------------------------------------------
SCALES = (0.8, 1.0, 1.25)


@functools.lru_cache(maxsize=None)
def _chain(w=96, h=64, ch=3):
    """The 3-camera chain at 60 % overlap (every pair overlaps), camera i's exposure scaled."""
    from multicamera_stitching_amd import rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, _, C = rig.calibrated_stitcher(3, w, h, ch, seed=0, overlap=0.6)
    frames = [np.clip(np.rint(f.astype(np.float64) * s), 0, 255).astype(np.uint8)
              for f, s in zip(rig.world_frames(C, w, h, ch, seed=0), SCALES)]
    return [_stage_desc(sb) for sb in st.stitchers], frames


def _chain_maker(w=96, h=64, ch=3, interp=1, lenses=None):
    from multicamera_stitching_amd import _capi
    descs, frames = _chain(w, h, ch)

    def make():
        plan = _capi.Plan(descs, w, h, ch, interp)
        for c, (K, d) in sorted((lenses or {}).items()):
            plan.set_lens(c, K, d)
        return plan
    return make, frames


@functools.lru_cache(maxsize=None)
def _world(n, w, h, ch, seed, **kw):
    from multicamera_stitching_amd import rig
    from multicamera_stitching_amd.StitcherClass import Stitcher, _stage_desc
    C = rig.camera_models(n, w, h, seed=seed, **kw)
    frames = rig.world_frames(C, w, h, ch, seed=seed)
    images = dict(zip(rig.labels(n), frames))
    st = Stitcher(images)
    st.calibrate_stitcher(images, save=False,
                          homographies=rig.homography_provider(C, lambda: st.stitchers))
    return [_stage_desc(sb) for sb in st.stitchers], [images[label] for label in st.img_labels]


def _world_maker(n, w, h, ch, seed, interp=1, **kw):
    from multicamera_stitching_amd import _capi
    descs, frames = _world(n, w, h, ch, seed, **kw)
    return (lambda: _capi.Plan(descs, w, h, ch, interp)), frames


def _chain_oracle(make, mode, interp=1):
    plan = make()
    flat = plan.describe()
    plan.close()
    if mode == NONE:
        return lambda pre: oracle.flat_stitch(flat, pre, interp)
    return lambda pre: oracle.blend_stitch(flat, pre, mode, interp)


def _lens1(w=96, h=64):
    return {1: ([[0.9 * w, 0, w / 2 - 0.5 + 1.3], [0, 0.9 * w, h / 2 - 0.5 - 0.7], [0, 0, 1]],
                [-0.21, 0.06, 0.001, -0.0007, 0.0])}


# ---- 1. the chain, every mode, both interpolations -----------------------------------------------
@pytest.mark.parametrize("interp", [1, 0])
@pytest.mark.parametrize("mode", [NONE, SEAM, FEATHER, MULTIBAND])
def test_chain_every_mode(mode, interp):
    make, frames = _chain_maker(interp=interp)
    plan = _check(make, _captures(frames, 5), GAINS, mode,
                  want_oracle=_chain_oracle(make, mode, interp))
    st = plan.stats()
    print(st)
    if mode in (FEATHER, MULTIBAND):
        assert st["blend_tiles"] > 0
    if mode == MULTIBAND:
        assert st["mb_bands"] == 0          # a mosaic of 64 rows: the levels kernel


# ---- 2. odd sizes --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [NONE, FEATHER, MULTIBAND])
def test_odd_one_channel_chain(mode):
    """97 x 61 x 1 (mosaic 174 x 61): the frame-edge lanes' byte stores, rows of 97 bytes."""
    make, frames = _chain_maker(97, 61, 1)
    plan = make()
    assert (plan.out_w, plan.out_h) == (174, 61)
    plan.close()
    _check(make, _captures(frames, 3), GAINS, mode, want_oracle=_chain_oracle(make, mode))


@pytest.mark.parametrize("mode", [NONE, FEATHER, MULTIBAND])
@pytest.mark.parametrize("case", [
    dict(n=2, w=40, h=20, ch=2, seed=8, overlap=0.5),
    dict(n=2, w=150, h=90, ch=4, seed=5, rot_deg=2.0),
])
def test_two_and_four_channels(case, mode):
    make, frames = _world_maker(**case)
    _check(make, _captures(frames, 2), [1.37, 0.61], mode, want_oracle=_chain_oracle(make, mode))


# ---- 3. / 4. the band pass -----------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 5])
def test_band_pass_lds_ring(F):
    """4 x 320 x 180 x 3, dense dword-aligned frames: the aligned launch, whose bands take the
    LDS ring (a wave takes 2 captures: F = 5 leaves an odd tail)."""
    make, frames = _world_maker(4, 320, 180, 3, seed=3)
    plan = _check(make, _captures(frames, F), MORE_GAINS[:4], MULTIBAND, extra=(0,),
                  want_oracle=_chain_oracle(make, MULTIBAND))
    st = plan.stats()
    print(st)
    assert st["mb_bands"] > 0 and st["mb_bands_lds"] > 0, st


def test_band_pass_unaligned_launch_of_an_aligned_plan():
    """The same rig with camera 1's frames 5 bytes apart beyond their size: the launch takes the
    unaligned global-window kernels (band_form in mcs_launch.cpp) although the plan has ring
    bands."""
    make, frames = _world_maker(4, 320, 180, 3, seed=3)
    plan = _check(make, _captures(frames, 3), MORE_GAINS[:4], MULTIBAND, extra=(0, 5, 0))
    assert plan.stats()["mb_bands"] > 0


def test_band_pass_global_form():
    """3 x 202 x 130 x 3: rows of 606 bytes, no multiple of 4 -- no band takes the ring and every
    launch runs the unaligned global-window kernels.  (The 202 x 110 rig of test_blend_vs_oracle
    does not reach them: the band pass needs a mosaic of 128 rows, below that the levels kernel
    runs; 130 rows is the smallest round size above.)"""
    make, frames = _world_maker(3, 202, 130, 3, seed=13)
    plan = _check(make, _captures(frames, 3), GAINS, MULTIBAND, extra=(0,),
                  want_oracle=_chain_oracle(make, MULTIBAND))
    st = plan.stats()
    print(st)
    assert st["mb_bands"] > 0 and st["mb_bands_lds"] == 0, st


# ---- 5. the wider blend kernels' plans -----------------------------------------------------------
def test_three_to_four_owners_per_tile():
    make, frames = _world_maker(4, 64, 48, 3, seed=10, overlap=0.8)
    plan = _check(make, _captures(frames, 2), MORE_GAINS[:4], MULTIBAND,
                  want_oracle=_chain_oracle(make, MULTIBAND))
    assert 3 <= plan.stats()["mb_owners"] <= 4, plan.stats()


def test_more_than_four_owners_per_tile():
    make, frames = _world_maker(5, 40, 30, 3, seed=11, step=6)
    for mode in (MULTIBAND, FEATHER):
        plan = _check(make, _captures(frames, 2), MORE_GAINS[:5], mode,
                      want_oracle=_chain_oracle(make, mode))
        if mode == MULTIBAND:
            assert plan.stats()["mb_owners"] > 4, plan.stats()


# ---- 6. the cylinder -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [SEAM, MULTIBAND])
def test_cylinder(mode):
    from multicamera_stitching_amd import _capi, rig
    cams, frames, g = rig.cylinder_rig(8, 64, 36, 37.0, 3, seed=0)
    gains = [1.0 + 0.07 * ((3 * c) % 8 - 3.5) for c in range(8)]
    assert len({gain_ref.quantise(v) for v in gains}) == 8

    def make():
        return _capi.Plan.cylindrical(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"], g["v0"], 3)

    def want(pre):
        return oracle.blend_stitch_cyl(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"], g["v0"],
                                       pre, mode)
    _check(make, _captures(frames, 2), gains, mode, want_oracle=want)


# ---- 7. a lens and gains together ----------------------------------------------------------------
@pytest.mark.parametrize("mode", [NONE, FEATHER])
def test_lens_and_gains(mode):
    make, frames = _chain_maker(lenses=_lens1())
    plan = _check(make, _captures(frames, 2), GAINS, mode)
    assert plan.stats()["lens_cams"] == 1


# ---- 8. the side lists ---------------------------------------------------------------------------
@pytest.mark.parametrize("M, src, dst, path", [
    ([[1.0, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, 1.0]], (400, 1000), (400, 200), "big_tiles"),
    ([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, 1.0]], (3000, 1000), (300, 200), "direct_tiles"),
])
def test_side_lists(M, src, dst, path):
    """The warp plans of test_warp_plan_side_paths_vs_oracle (one camera, one gain): tiles on the
    large-footprint streaming list and on the direct-gather list."""
    from multicamera_stitching_amd import _capi, rig
    img = rig.texture(src[1], src[0], 3, seed=5)

    def make():
        return _capi.Plan.warp(np.array(M), src[0], src[1], dst[0], dst[1], 3)
    plan = _check(make, [[img], [np.ascontiguousarray(img[::-1])]], [1.37], NONE, extra=(0,),
                  want_oracle=lambda pre: oracle.warp_perspective(pre[0], M, dst, 1))
    assert plan.stats()[path] > 0, plan.stats()


# ---- 9. mcs_stitch_direct_gained -----------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 9])              # 9: more than two blocks of kDirectFrames = 4
@pytest.mark.parametrize("mode", [NONE, SEAM])
def test_stitch_direct_gained(mode, F):
    make, frames = _chain_maker()
    _check(make, _captures(frames, F), GAINS, mode, method="stitch_direct",
           want_oracle=_chain_oracle(make, mode))


def test_stitch_direct_gained_uniform_strides_and_nearest():
    """Dense frames (one launch for the batch, not one per capture) and the nearest map."""
    make, frames = _chain_maker(interp=0)
    _check(make, _captures(frames, 5), GAINS, NONE, method="stitch_direct", extra=(0,),
           want_oracle=_chain_oracle(make, NONE, 0))


# ---- 10. identity --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [NONE, MULTIBAND])
def test_identity_gains_and_no_gains(mode):
    make, frames = _chain_maker()
    caps = _captures(frames, 2)
    plain = make()
    plan = make()
    if mode:
        plain.set_blend(mode)
        plan.set_blend(mode)
    want = _stitch(plain, "stitch_device", caps)
    assert np.array_equal(_stitch(plan, "stitch_device_gained", caps), want)     # gains disabled
    if mode == NONE:
        assert np.array_equal(_stitch(plan, "stitch_direct_gained", caps), want)
    plan.set_gains([1.0, 1.0, 1.0])
    assert np.array_equal(_stitch(plan, "stitch_device_gained", caps), want)     # every q = 256
    if mode == NONE:
        assert np.array_equal(_stitch(plan, "stitch_direct_gained", caps), want)
    from multicamera_stitching_amd import _capi
    with pytest.raises(_capi.McsError) as e:                   # the ungained entry still refuses
        _stitch(plan, "stitch_device", caps)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED


# ---- 11. gains changed between two launches ------------------------------------------------------
@pytest.mark.parametrize("mode", [NONE, MULTIBAND])
def test_a_launch_keeps_the_gains_it_was_launched_with(mode):
    torch = _torch()
    make, frames = _chain_maker()
    ga, gb = GAINS, [0.7, 1.5, 1.1]
    plan, plain = make(), make()
    if mode:
        plan.set_blend(mode)
        plain.set_blend(mode)
    frames = _captures(frames, 1)[0]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    ptrs, strides = [d.data_ptr() for d in dev], [d.numel() for d in dev]
    outs = [torch.zeros((plan.out_h, plan.out_w * 3), dtype=torch.uint8, device="cuda")
            for _ in range(2)]
    plan.stitch_device(ptrs, strides, outs[0].data_ptr(), plan.out_w * 3, outs[0].numel(), 1, 0)
    torch.cuda.synchronize()                                   # (tables prepared, kernels loaded)
    plan.set_gains(ga)
    plan.stitch_device_gained(ptrs, strides, outs[0].data_ptr(), plan.out_w * 3, outs[0].numel(),
                              1, 0)
    plan.set_gains(gb)                                         # A's launch is in flight
    plan.stitch_device_gained(ptrs, strides, outs[1].data_ptr(), plan.out_w * 3, outs[1].numel(),
                              1, 0)
    torch.cuda.synchronize()
    for out, g in zip(outs, (ga, gb)):
        want = _stitch(plain, "stitch_device", _pre([frames], g), extra=(0,))
        assert np.array_equal(out.cpu().numpy(), want[0])
    assert not torch.equal(outs[0], outs[1])


# ---- 12. the sweep -------------------------------------------------------------------------------
def test_sweep_plans_are_refused(monkeypatch):
    from multicamera_stitching_amd import _capi
    monkeypatch.setenv("MCS_MB_SWEEP", "1")
    make, frames = _world_maker(4, 320, 180, 3, seed=3)
    plan = make()
    plan.set_blend(MULTIBAND)
    plan.prepare()
    assert plan.stats()["mb_sweep_strips"] > 0, plan.stats()
    plan.set_gains(MORE_GAINS[:4])
    with pytest.raises(_capi.McsError) as e:
        _stitch(plan, "stitch_device_gained", [frames], extra=(0,))
    assert e.value.code == _capi.MCS_E_UNSUPPORTED and "sweep" in str(e.value)
    plan.set_gains(None)
    got = _stitch(plan, "stitch_device", [frames], extra=(0,))
    want = oracle.blend_stitch(plan.describe(), frames, MULTIBAND)
    assert np.array_equal(got[0].reshape(want.shape), want)
