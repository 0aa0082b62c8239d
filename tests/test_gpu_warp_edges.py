"""The paste-path kernels (mcs_prepare_*, mcs_stream_*, mcs_stream_big_*, mcs_direct_*) at the
edges of geometry, size and alignment -- the table of tests/warp_edges.py and the side paths at
their smallest shapes.  Bar: max |diff| == 0 against the CPU oracle.

Every device result comes through Plan.stitch_device (or stitch_direct) on torch buffers whose
pitch padding, frame gaps and surroundings hold a sentinel the kernels must leave untouched, and
every test asserts from Plan.stats() that the case took the path it is there for.
"""
import ctypes
import functools

import numpy as np
import pytest

import warp_edges as we
from oracle import oracle

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64                 # sentinel bytes before and after every buffer


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from multicamera_stitching_amd import _capi
    assert _capi.device_count() >= 1, "GPU tests need an MI355X (no HIP device visible)"


def _diff(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max()) if a.size else 0


def _upload(frames, off=0, pad=0):
    """F frames of one camera in a device buffer, the first at byte `off` past the guard, `pad`
    bytes between frames: (tensor, pointer of frame 0, frame stride)."""
    import torch
    n = frames[0].size
    stride = n + pad
    host = np.full(GUARD + off + len(frames) * stride + GUARD, SENTINEL, np.uint8)
    for f, fr in enumerate(frames):
        at = GUARD + off + f * stride
        host[at:at + n] = np.ascontiguousarray(fr).reshape(-1)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + GUARD + off, stride


def device_stitch(plan, batch, out_off=0, pitch_pad=0, fstride_pad=0, cam_offs=None, cam_pad=0,
                  n_frames=None, direct=False):
    """batch[f][i]: frame f of camera i.  Stitches the batch with Plan.stitch_device (or
    stitch_direct) into a sentinel-filled buffer -- mosaic base `out_off` bytes past the guard,
    rows `pitch_pad` bytes apart beyond the mosaic's own, frames `fstride_pad` further -- and
    returns the mosaics (F, out_h, out_w * C) after checking every other byte of the buffer."""
    import torch
    F = len(batch)
    n_cams = len(batch[0])
    ch = plan.channels
    row = plan.out_w * ch
    pitch = row + pitch_pad
    fstride = plan.out_h * pitch + fstride_pad
    cam_offs = cam_offs or [0] * n_cams
    ups = [_upload([batch[f][i] for f in range(F)], cam_offs[i], cam_pad) for i in range(n_cams)]
    out = torch.full((GUARD + out_off + F * fstride + GUARD,), SENTINEL, dtype=torch.uint8,
                     device="cuda")
    call = plan.stitch_direct if direct else plan.stitch_device
    call([u[1] for u in ups], [u[2] for u in ups], out.data_ptr() + GUARD + out_off, pitch,
         fstride, F if n_frames is None else n_frames, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    mosaic = np.zeros(got.shape, bool)
    for f in range(F if n_frames is None else n_frames):
        at = GUARD + out_off + f * fstride
        for y in range(plan.out_h):
            mosaic[at + y * pitch:at + y * pitch + row] = True
    assert (got[~mosaic] == SENTINEL).all(), "the kernel wrote outside the mosaic rows"
    for u in ups:      # the frames are only read
        cam = u[0].cpu().numpy()
        assert (cam[:GUARD] == SENTINEL).all() and (cam[-GUARD:] == SENTINEL).all()
    res = np.zeros((F, plan.out_h, row), np.uint8)
    for f in range(F):
        at = GUARD + out_off + f * fstride
        for y in range(plan.out_h):
            res[f, y] = got[at + y * pitch:at + y * pitch + row]
    return res


# ---- a. geometry ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case_ref(name, ch, interp):
    case = we.BY_NAME[name]
    (sw, sh), dst = case["src"], case["dst"]
    src = we.texture(sh, sw, ch, seed=7)
    want = oracle.warp_perspective(src, case["M"], dst, interp)
    src.setflags(write=False)
    want.setflags(write=False)
    return src, want


def _check_path(name, st):
    """The path each case exists for (Plan.stats of the prepared plan)."""
    tiles, lds, direct = st["tiles"], st["lds_tiles"], st["direct_tiles"]
    assert lds + direct == tiles and st["big_tiles"] == 0, st
    if name == "horizon_tall":
        # the tile above the horizon reads source rows 32..399: the direct gather
        assert direct > 0, st
    elif name in ("tiny_7x40c1", "tiny_2x40c3"):
        # the tiles whose footprints reach the frame's last rows (a 16-byte DMA chunk of row
        # h - 2 would end past the frame) take the direct gather, the others stream through LDS
        assert 0 < direct < tiles, st
    elif name.startswith("tiny_"):
        # frames of 8..16 bytes: every DMA chunk would leave the frame
        assert direct == tiles, st
    else:
        # A footprint counts live taps only and is clipped to the frame: the sources of the other
        # horizon and huge_* cases (at most 100 x 60) fit one tile's LDS slot whole, however far
        # the map throws the remaining pixels, so these stream through LDS; their horizon runs
        # through the direct gather in horizon_tall and in every case's stitch_direct pass.
        assert lds == tiles, st


GEOMETRY_PARAMS = [(c["name"], ch) for c in we.CASES
                   for ch in we.case_channels(c, (1, 2, 3, 4) if c["name"] in we.HORIZON
                                              else (1, 3))]


@pytest.mark.parametrize("interp", [1, 0])
@pytest.mark.parametrize("name, ch", GEOMETRY_PARAMS)
def test_geometry(name, ch, interp):
    """Every case of the table: stitch_host, stitch_device (padded pitch, F = 2) and
    stitch_direct (the map evaluated in the direct kernel for every tile) equal the oracle."""
    case = we.BY_NAME[name]
    src, want = _case_ref(name, ch, interp)
    plan = we.case_plan(case, ch, interp)
    try:
        got = plan.stitch_host([src])
        assert _diff(got.reshape(want.shape), want) == 0
        _check_path(name, plan.stats())
        src2 = np.ascontiguousarray(src[::-1])
        want2 = oracle.warp_perspective(src2, case["M"], case["dst"], interp)
        for direct in (False, True):
            dev = device_stitch(plan, [[src], [src2]], pitch_pad=5, fstride_pad=3, direct=direct)
            assert _diff(dev[0].reshape(want.shape), want) == 0, direct
            assert _diff(dev[1].reshape(want.shape), want2) == 0, direct
    finally:
        plan.close()


# ---- b. side paths at their smallest shapes -------------------------------------------------

SIDE = {
    # vertical zoom-out x5: a 16-row tile reads 80 source rows -- more than the 64 of the main
    # block, at most the 128 of mcs_stream_big
    "big_tiles": dict(M=[[1.0, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, 1.0]], src=(160, 200),
                      dst=(160, 40)),
    # horizontal x0.1: 1280 source columns per tile row, over 1 KiB per DMA row for every
    # channel count -- the direct gather
    "direct_tiles": dict(M=[[0.1, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 1.0]], src=(1500, 60),
                         dst=(150, 30)),
}


@functools.lru_cache(maxsize=None)
def _side_ref(path, ch, interp, f):
    c = SIDE[path]
    src = we.texture(c["src"][1], c["src"][0], ch, seed=50 + f)
    want = oracle.warp_perspective(src, c["M"], c["dst"], interp)
    src.setflags(write=False)
    want.setflags(write=False)
    return src, want


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("force64", [0, 1])
@pytest.mark.parametrize("interp", [1, 0])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
@pytest.mark.parametrize("path", list(SIDE))
def test_side_paths(path, ch, interp, force64, F):
    """The large-footprint and direct-gather tiles for every channel count, both interpolations
    and both address forms; F = 5 makes the direct launch's second frame group and splits the
    large-footprint tiles into min(8, F) capture ranges, with padded frame strides (0 and 3
    bytes) and a padded mosaic pitch."""
    from multicamera_stitching_amd import _capi
    L = _capi.load()
    c = SIDE[path]
    refs = [_side_ref(path, ch, interp, f) for f in range(F)]
    plan = _capi.Plan.warp(np.array(c["M"]), c["src"][0], c["src"][1], c["dst"][0], c["dst"][1],
                           ch, interp)
    L.mcs__force_off64(ctypes.c_int(force64))
    try:
        for cam_pad in ((0,) if F == 1 else (0, 3)):
            got = device_stitch(plan, [[r[0]] for r in refs], pitch_pad=0 if F == 1 else 7,
                                fstride_pad=0 if F == 1 else 2, cam_pad=cam_pad)
            for f in range(F):
                assert _diff(got[f].reshape(refs[f][1].shape), refs[f][1]) == 0, (cam_pad, f)
        st = plan.stats()
        assert st[path] > 0, st
    finally:
        L.mcs__force_off64(ctypes.c_int(0))
        plan.close()


# ---- c. store alignment ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _chain_ref(ch):
    from multicamera_stitching_amd import rig
    plan, cams, stages = we.chain_plan(ch)
    plan.close()
    F = 3
    batch = [[rig.texture(c.shape[0], c.shape[1], ch, seed=31 + 100 * f + i)
              for i, c in enumerate(cams)] for f in range(F)]
    wants = [oracle.cascade_stitch(stages, b, oracle.INTER_LINEAR) for b in batch]
    return batch, wants


@pytest.mark.parametrize("out_off", [0, 1, 2, 3])
@pytest.mark.parametrize("ch", [1, 3])
def test_store_alignment(ch, out_off):
    """The three store forms of the streaming kernel (wave-wide, per-lane wide, per-byte) are
    chosen from the alignment of the mosaic base, its pitch and its frame stride: a mosaic base
    0..3 bytes off a dword, pitches of out_w C + {0, 1, 3}, a frame stride that is no multiple
    of 4 (and one that is), camera frames 0..3 bytes off a dword -- F = 3, all equal to the
    oracle, every byte around the mosaic rows untouched."""
    batch, wants = _chain_ref(ch)
    plan, _, _ = we.chain_plan(ch)
    try:
        for pitch_pad in (0, 1, 3):
            for cam_off in (0, 1, 3):
                pitch = plan.out_w * ch + pitch_pad
                odd = 1 if (plan.out_h * pitch + 1) % 4 else 2
                pads = (odd,) if cam_off else (odd, (-plan.out_h * pitch) % 4)
                for fstride_pad in pads:
                    got = device_stitch(plan, batch, out_off=out_off, pitch_pad=pitch_pad,
                                        fstride_pad=fstride_pad,
                                        cam_offs=[(cam_off * (i + 1)) % 4 for i in range(3)],
                                        cam_pad=cam_off)
                    for f in range(3):
                        assert _diff(got[f].reshape(wants[f].shape), wants[f]) == 0, \
                            (pitch_pad, cam_off, fstride_pad, f)
        st = plan.stats()
        assert st["direct_tiles"] == 0 and st["lds_tiles"] == st["tiles"] > 1, st
    finally:
        plan.close()


# ---- d. more than kTileCams cameras in one paste-mode tile ------------------------------------

def test_dense_rig_paste_mode():
    """Eight cameras 5 px apart under the paste rule: more than four meet in one 128 x 16 tile,
    which sends it to the direct gather -- stitch_host, stitch_device and stitch_direct equal the
    flattened-chain oracle."""
    plan, cams = we.dense_plan()
    try:
        want = oracle.flat_stitch(plan.describe(), cams)
        assert want.any()
        assert _diff(plan.stitch_host(cams).reshape(want.shape), want) == 0
        st = plan.stats()
        assert st["direct_tiles"] > 0, st
        for direct in (False, True):
            got = device_stitch(plan, [cams], pitch_pad=3, direct=direct)
            assert _diff(got[0].reshape(want.shape), want) == 0, direct
    finally:
        plan.close()


# ---- e. an empty batch ------------------------------------------------------------------------

@pytest.mark.parametrize("direct", [False, True])
def test_zero_frames_is_a_no_op(direct):
    """n_frames = 0 returns OK and leaves the mosaic buffer untouched."""
    case = we.BY_NAME["narrow_w"]
    src, _ = _case_ref("narrow_w", 3, 1)
    plan = we.case_plan(case, 3, 1)
    try:
        # (device_stitch checks every byte outside the mosaics of n_frames captures: all of it)
        device_stitch(plan, [[src]], n_frames=0, direct=direct)
    finally:
        plan.close()
