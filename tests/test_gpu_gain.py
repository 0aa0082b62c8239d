"""Exposure gain compensation on the GPU: the overlap statistics against the numpy reference
(tests/gain_ref.py) exactly, the gain kernel against numpy exactly, and the gained stitch paths
(host, sized, cylinder, stream, Stitcher) against the same paths -- and the oracle -- on numpy
pre-gained frames.  Every comparison is for equality: the arithmetic is integer throughout."""
import functools

import numpy as np
import pytest

from oracle import oracle

import gain_ref
import lens_ref

pytestmark = pytest.mark.gpu

OV_FRAMES = 4          # csrc/mcs_kparams.h kOvFrames: captures per block of the sum kernel
SCALES = (0.8, 1.0, 1.25)
GAINS = [1.37, 1.0, 0.61]
NONE, FEATHER, MULTIBAND = 0, 1, 2


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _chain(w=96, h=64, ch=3):
    """The 3-camera chain at 60 % overlap (every pair of cameras overlaps) and its world frames,
    camera i's exposure scaled by SCALES[i]."""
    from multicamera_stitching_amd import rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, _, C = rig.calibrated_stitcher(3, w, h, ch, seed=0, overlap=0.6)
    frames = [np.clip(np.rint(f.astype(np.float64) * s), 0, 255).astype(np.uint8)
              for f, s in zip(rig.world_frames(C, w, h, ch, seed=0), SCALES)]
    return st, [_stage_desc(sb) for sb in st.stitchers], frames


def _chain_plan(w=96, h=64, ch=3, interp=1):
    from multicamera_stitching_amd import _capi
    _, descs, frames = _chain(w, h, ch)
    return _capi.Plan(descs, w, h, ch, interp), frames


@functools.lru_cache(maxsize=None)
def _cyl():
    from multicamera_stitching_amd import rig
    return rig.cylinder_rig(8, 64, 36, 37.0, 3, seed=0)


def _cyl_plan():
    from multicamera_stitching_amd import _capi
    cams, frames, g = _cyl()
    return _capi.Plan.cylindrical(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"], g["v0"], 3)


def _captures(frames, n):
    """n captures, each with different frames (capture 0: the frames themselves)."""
    return [[np.ascontiguousarray(np.roll(c, 5 * f + i * f, axis=1)) if f else c
             for i, c in enumerate(frames)] for f in range(n)]


def _device_stats(plan, captures, k):
    """Plan.overlap_stats on device copies of the captures.  Camera 0's frames are dense,
    camera 1's 5 bytes apart (a stride that is no multiple of 16), the others 48 bytes apart."""
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
    N, S = plan.overlap_stats(ptrs, strides, F, k)
    del bufs
    return N, S


def _lens1(w=96, h=64):
    return {1: ([[0.9 * w, 0, w / 2 - 0.5 + 1.3], [0, 0.9 * w, h / 2 - 0.5 - 0.7], [0, 0, 1]],
                [-0.21, 0.06, 0.001, -0.0007, 0.0])}


@pytest.mark.parametrize("w,h,ch,interp,k,F,lens", [
    (96, 64, 3, 1, 0, 1, False),
    (96, 64, 3, 1, 2, OV_FRAMES + 1, False),
    (96, 64, 3, 0, 0, OV_FRAMES + 1, False),
    (96, 64, 3, 0, 2, 1, False),
    (97, 61, 1, 1, 2, OV_FRAMES + 1, False),     # mosaic 174 x 61: no multiple of the step
    (97, 61, 1, 1, 0, 1, False),
    (96, 64, 3, 1, 0, 2, True),
    (96, 64, 3, 1, 2, 1, True),
])
def test_chain_stats_equal_reference(w, h, ch, interp, k, F, lens):
    plan, frames = _chain_plan(w, h, ch, interp)
    lenses = _lens1(w, h) if lens else None
    if lens:
        plan.set_lens(1, *lenses[1])
    if (w, h) == (97, 61):
        assert (plan.out_w, plan.out_h) == (174, 61)
    caps = _captures(frames, F)
    want_N, want_S = gain_ref.chain_stats(plan.describe(), caps, k, interp, lenses)
    assert want_N[0, 2] > 0                              # the triple-covered band is there
    assert F == 1 or not np.array_equal(want_S[0], want_S[-1])   # the captures differ
    N, S = _device_stats(plan, caps, k)
    assert np.array_equal(N, want_N), (N.tolist(), want_N.tolist())
    assert np.array_equal(S, want_S), (S - want_S).tolist()


@pytest.mark.parametrize("k,F", [(0, OV_FRAMES + 1), (2, 1)])
def test_cylinder_stats_equal_reference(k, F):
    """Eight cameras around the circle: most pairs are empty, neighbours overlap, the first and
    the last wrap around."""
    cams, frames, g = _cyl()
    plan = _cyl_plan()
    caps = _captures(frames, F)
    want_N, want_S = gain_ref.cyl_stats(cams, g, caps, k)
    assert want_N[0, 7] > 0 and want_N[0, 1] > 0 and want_N[0, 4] == 0
    N, S = _device_stats(plan, caps, k)
    assert np.array_equal(N, want_N), (N.tolist(), want_N.tolist())
    assert np.array_equal(S, want_S)


def test_table_follows_step_and_lens_and_host_entry():
    """One plan: another step rebuilds the table, set_lens drops it, blend changes keep it; the
    host entry equals the device entry."""
    plan, frames = _chain_plan()
    flat = plan.describe()
    caps = [frames]
    for k in (2, 0, 2):
        want_N, want_S = gain_ref.chain_stats(flat, caps, k)
        N, S = _device_stats(plan, caps, k)
        assert np.array_equal(N, want_N) and np.array_equal(S, want_S), k
    plan.set_blend(FEATHER)
    N, S = plan.overlap_stats_host(frames, 2)
    assert np.array_equal(N, want_N) and np.array_equal(S, want_S[0])
    lenses = _lens1()
    plan.set_lens(1, *lenses[1])
    lens_N, lens_S = gain_ref.chain_stats(flat, caps, 2, lenses=lenses)
    assert not np.array_equal(lens_N, want_N)
    N, S = plan.overlap_stats_host(frames, 2)
    assert np.array_equal(N, lens_N) and np.array_equal(S, lens_S[0])
    N, S = _device_stats(plan, caps, 2)
    assert np.array_equal(N, lens_N) and np.array_equal(S, lens_S)
    plan.set_lens(1, None)
    N, S = plan.overlap_stats_host(frames, 2)
    assert np.array_equal(N, want_N) and np.array_equal(S, want_S[0])


# ---- the gain kernel ----------------------------------------------------------------------------
SIZES = (1, 15, 16, 17, 256, 97 * 61 * 3)
QS = (1, 255, 256, 257, 333, 65535)
PAD = 64


def _frame_bytes(nb, f):
    if nb == 256:
        return np.roll(np.arange(256, dtype=np.uint8), 7 * f)     # the 0..255 ramp
    return np.random.default_rng(nb * 31 + f).integers(0, 256, nb, dtype=np.uint8)


@pytest.mark.parametrize("in_place", [False, True])
def test_apply_equals_numpy(in_place):
    """Every size x source alignment x q: 3 frames (source stride bytes + 5), the whole
    destination buffer -- the frames, the 64 sentinel bytes before and after them and the gaps
    between them -- against numpy."""
    from multicamera_stitching_amd import _capi
    torch = _torch()
    F = 3
    for nb in SIZES:
        for off in range(4):
            ss = nb + 5
            ds = ss if in_place else nb + 133      # (out of place: >= 64 bytes around each frame)
            doff = off if in_place else (5 * off + 1) % 16
            src = np.full(PAD + off + F * ss + PAD + 16, 0xA5, np.uint8)
            for f in range(F):
                src[PAD + off + f * ss:PAD + off + f * ss + nb] = _frame_bytes(nb, f)
            for q in QS:
                dst = src.copy() if in_place else np.full(PAD + doff + F * ds + PAD + 16, 0x5A,
                                                          np.uint8)
                want = dst.copy()
                for f in range(F):
                    o = PAD + doff + f * ds
                    want[o:o + nb] = gain_ref.apply_q(src[PAD + off + f * ss:][:nb], q)
                d_src = torch.from_numpy(src).cuda()
                d_dst = d_src if in_place else torch.from_numpy(dst).cuda()
                assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
                _capi.gain_apply_device(d_src.data_ptr() + PAD + off, d_dst.data_ptr() + PAD + doff,
                                        nb, q, F, ss, ds)
                torch.cuda.synchronize()
                got = d_dst.cpu().numpy()
                assert np.array_equal(got, want), (nb, off, q, np.flatnonzero(got != want)[:8])
                if not in_place:
                    assert np.array_equal(d_src.cpu().numpy(), src)
    assert np.array_equal(gain_ref.apply_q(np.arange(256), 256), np.arange(256))   # the identity


# ---- stitching with gains -----------------------------------------------------------------------
def _pre(frames, gains=GAINS):
    return [gain_ref.apply_gain(f, g) for f, g in zip(frames, gains)]


@pytest.mark.parametrize("mode", [NONE, FEATHER, MULTIBAND])
def test_stitch_host_equals_stitch_of_pregained_frames(mode):
    plan, frames = _chain_plan()
    plain, _ = _chain_plan()
    plan.set_blend(mode)
    plain.set_blend(mode)
    pre = _pre(frames)
    assert any(not np.array_equal(a, b) for a, b in zip(pre, frames))
    ungained = plan.stitch_host(frames)
    assert plan.stats()["prepared"]
    plan.set_gains(GAINS)
    assert plan.stats()["prepared"]            # host state only: the tables stand
    got = plan.stitch_host(frames)
    assert not np.array_equal(got, ungained)
    assert np.array_equal(got, plain.stitch_host(pre))
    flat = plan.describe()
    want = oracle.flat_stitch(flat, pre) if mode == NONE else oracle.blend_stitch(flat, pre, mode)
    assert np.array_equal(got, want)
    plan.set_gains([1.0, 1.0, 1.0])            # identity gains run the kernel and change nothing
    assert np.array_equal(plan.stitch_host(frames), ungained)
    plan.set_gains(None)
    assert np.array_equal(plan.stitch_host(frames), ungained)


def test_sized_path_applies_the_gain_after_the_resize():
    plan, frames = _chain_plan()
    plain, _ = _chain_plan()
    half = oracle.resize_linear(frames[1], (48, 32))
    sizes = [(96, 64), (48, 32), (96, 64)]
    plan.set_gains(GAINS)
    got = plan.stitch_host([frames[0], half, frames[2]], sizes)
    pre = _pre([frames[0], oracle.resize_linear(half, (96, 64)), frames[2]])
    assert np.array_equal(got, plain.stitch_host(pre))
    assert np.array_equal(got, oracle.flat_stitch(plan.describe(), pre))


def test_cylinder_multiband_with_gains():
    cams, frames, g = _cyl()
    gains = [1.0 + 0.07 * ((3 * c) % 8 - 3.5) for c in range(8)]
    plan = _cyl_plan().set_gains(gains)
    pre = _pre(frames, gains)
    got = plan.stitch_host(frames)
    assert np.array_equal(got, _cyl_plan().stitch_host(pre))
    want = oracle.blend_stitch_cyl(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"], g["v0"], pre,
                                   oracle.BLEND_MULTIBAND)
    assert np.array_equal(got, want)


# ---- streams --------------------------------------------------------------------------------------
def _stream_rig():
    from multicamera_stitching_amd import _capi, rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, images, _ = rig.calibrated_stitcher(2, 64, 48, 3, seed=13)
    cams = [images[label] for label in st.img_labels]
    descs = [_stage_desc(sb) for sb in st.stitchers]
    return (lambda: _capi.Plan(descs, 64, 48, 3, 1)), cams


def test_stream_captures_keep_the_gains_they_were_submitted_with():
    from multicamera_stitching_amd import _capi
    make, cams = _stream_rig()
    plain = make()
    ga, gb = [1.2, 0.9], [0.7, 1.5]
    shot_a, shot_b = cams, [np.ascontiguousarray(np.roll(c, 9, axis=1)) for c in cams]
    plan = make().set_gains(ga)
    pipe = _capi.StreamPipeline(plan, depth=2, use_graphs=True)
    a = pipe.submit(shot_a)
    plan.set_gains(gb)                         # B's gains; A is in flight with the old ones
    b = pipe.submit(shot_b)
    got_a, got_b = pipe.wait(a), pipe.wait(b)
    assert np.array_equal(got_a, plain.stitch_host(_pre(shot_a, ga)))
    assert np.array_equal(got_b, plain.stitch_host(_pre(shot_b, gb)))
    a = pipe.submit(shot_a)                    # the slots again, with B's gains still set
    assert np.array_equal(pipe.wait(a), plain.stitch_host(_pre(shot_a, gb)))
    plan.set_gains(None)                       # disabled later: the stream's kernels run q = 256
    a = pipe.submit(shot_a)
    assert np.array_equal(pipe.wait(a), plain.stitch_host(shot_a))
    pipe.close()


def test_stream_created_without_gains():
    """Identity gains set later leave it alone; other values are refused at submit (the gain
    kernels are part of the slots' graphs or they are not: fixed at creation)."""
    from multicamera_stitching_amd import _capi
    make, cams = _stream_rig()
    plan = make()
    want = plan.stitch_host(cams)
    pipe = _capi.StreamPipeline(plan, depth=2, use_graphs=True)
    plan.set_gains([1.0, 1.0])
    assert np.array_equal(pipe.wait(pipe.submit(cams)), want)
    plan.set_gains([1.1, 1.0])
    with pytest.raises(_capi.McsError) as e:
        pipe.submit(cams)
    assert e.value.code == _capi.MCS_E_INVALID
    plan.set_gains(None)
    assert np.array_equal(pipe.wait(pipe.submit(cams)), want)
    pipe.close()


# ---- the drop-in ---------------------------------------------------------------------------------
def test_stitcher_compensate_exposure():
    from multicamera_stitching_amd import rig
    _, _, frames = _chain()
    st, _, _ = rig.calibrated_stitcher(3, 96, 64, 3, seed=0, overlap=0.6)
    other, _, _ = rig.calibrated_stitcher(3, 96, 64, 3, seed=0, overlap=0.6)
    images = dict(zip(st.img_labels, frames))
    gains = st.compensate_exposure(images, step_log2=2)
    N, S = gain_ref.chain_stats(st.plan(3).describe(), [frames], 2)
    want = gain_ref.solve(N, S[0], 3)
    got = np.array([gains[label] for label in st.img_labels])
    print("gains", got.tolist())
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
    assert got[0] > got[1] > got[2]
    pre = {label: gain_ref.apply_gain(images[label], gains[label]) for label in st.img_labels}
    assert np.array_equal(st.stitch(images), other.stitch(pre))
    assert not np.array_equal(st.stitch(images), other.stitch(images))
