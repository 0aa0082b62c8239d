"""Lensed plans on the GPU (mcs_plan_set_lens): raw frames in, one pass.  Every mode and path
against the numpy specification tests/lens_ref.py, and -- with the identity lens, which must run
the lens arithmetic and return its input bit for bit -- against the existing oracle.  The bar is
max |diff| = 0 throughout."""
import functools

import numpy as np
import pytest

from oracle import oracle

import lens_ref
from test_undistort_cpu import CASES

pytestmark = pytest.mark.gpu

NONE, FEATHER, MULTIBAND, SEAM = 0, 1, 2, 3
DISTS = [CASES[0]["d"], CASES[2]["d"], CASES[3]["d"]]     # 5, 8 and 12 coefficients
IDENTITY = (np.eye(3), None)


def _diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.size == b.size, (a.shape, b.shape)
    return int(np.abs(a.reshape(b.shape).astype(np.int16) - b.astype(np.int16)).max())


def _lens(w, h, dist, f=0.9):
    return ([[f * w, 0, w / 2 - 0.5 + 1.3], [0, f * w, h / 2 - 0.5 - 0.7], [0, 0, 1]], dist)


@functools.lru_cache(maxsize=None)
def _chain_rig(n, w, h, ch, super_mode=False):
    from multicamera_stitching_amd import rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, images, _ = rig.calibrated_stitcher(n, w, h, ch, super_mode=super_mode, seed=1,
                                            rot_deg=2.0, persp=5e-5)
    cams = [images[label] for label in st.img_labels]
    return st, images, cams, [_stage_desc(sb) for sb in st.stitchers]


def _chain_plan(n, w, h, ch, interp=1, super_mode=False, lenses=None):
    from multicamera_stitching_amd import _capi
    _, _, cams, descs = _chain_rig(n, w, h, ch, super_mode)
    plan = _capi.Plan(descs, w, h, ch, interp)
    for c, (K, d) in sorted((lenses or {}).items()):
        plan.set_lens(c, K, d)
    assert plan.stats()["lens_cams"] == len(lenses or {})
    return plan, cams


def _chain_want(flat, cams, interp, lenses, mode, **kw):
    pos, slot_cams, rects = lens_ref.chain_positions(flat, interp, lenses, **kw)
    if mode == NONE:
        return lens_ref.render_paste(pos, slot_cams, rects, cams)
    return lens_ref.render_blend(pos, slot_cams, cams, "seam" if mode == SEAM else "feather")


CHAINS = {
    "3x160x120x3": dict(n=3, w=160, h=120, ch=3),
    "4x128x96x1-nearest": dict(n=4, w=128, h=96, ch=1, interp=0),
    "3x96x64x4": dict(n=3, w=96, h=64, ch=4),
    "2x200x150x2-super": dict(n=2, w=200, h=150, ch=2, super_mode=True),
}


def _variant(which, n, w, h):
    cams = {"all": range(n), "cam0": [0], "cam1": [1]}[which]
    return {c: _lens(w, h, DISTS[c % 3]) for c in cams}


@pytest.mark.parametrize("which", ["all", "cam0", "cam1"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_vs_lens_ref(name, which):
    """Paste, SEAM and FEATHER of lensed chain plans through stitch_host."""
    case = dict(CHAINS[name])
    interp = case.pop("interp", 1)
    lenses = _variant(which, case["n"], case["w"], case["h"])
    plan, cams = _chain_plan(interp=interp, lenses=lenses, **case)
    flat = plan.describe()
    for mode in (NONE, SEAM, FEATHER):
        plan.set_blend(mode)
        want = _chain_want(flat, cams, interp, lenses, mode)
        assert _diff(plan.stitch_host(cams), want) == 0, mode
    assert want.any()


def test_fold_back_radius_keeps_ghost_coverage_out():
    """k1 = -0.3 at f = 0.6 w folds back just past the frame corner (r2max about 1.11, the
    corner's r2 about 1.08): without the valid-radius rule the far rays of a camera land inside
    its raw frame again, in its neighbours' part of the mosaic."""
    w, h = 160, 120
    dist = [-0.3, 0, 0, 0]
    lenses = {c: _lens(w, h, dist, f=0.6) for c in range(3)}
    assert 1.0 < lens_ref.r2max(dist) < 1.2
    plan, cams = _chain_plan(3, w, h, 3, lenses=lenses)
    flat = plan.describe()
    sizes = {c: (w, h) for c in range(3)}
    owners = []
    for rule in (True, False):
        pos, slot_cams, _ = lens_ref.chain_positions(flat, 1, lenses, use_r2max=rule)
        owners.append(lens_ref.owner_map(lens_ref.distances(pos, slot_cams, sizes), slot_cams))
    assert (owners[0] != owners[1]).sum() > 0      # the rule matters on this rig
    for mode in (SEAM, FEATHER):
        plan.set_blend(mode)
        assert _diff(plan.stitch_host(cams), _chain_want(flat, cams, 1, lenses, mode)) == 0, mode


CYLS = {
    "4x128x96x2": dict(n=4, w=128, h=96, f=70.0, ch=2, seed=5),
    "8x320x180x3": dict(n=8, w=320, h=180, f=185.0, ch=3, seed=2, jitter_deg=2.0),
}
CYL_DIST = [-0.12, 0.03, 0.0005, -0.0003]


@functools.lru_cache(maxsize=None)
def _cyl_rig(name, seed=None):
    from multicamera_stitching_amd import rig
    case = dict(CYLS[name])
    if seed is not None:
        case.update(seed=seed, jitter_deg=0.0)
    n, w, h, f, ch = (case.pop(k) for k in ("n", "w", "h", "f", "ch"))
    cams, frames, g = rig.cylinder_rig(n, w, h, f, ch, **case)
    lenses = {c: ([[k["f"], 0, k["cx"]], [0, k["f"], k["cy"]], [0, 0, 1]], CYL_DIST)
              for c, k in enumerate(cams)}
    return cams, frames, g, lenses, ch


def _cyl_plan(cams, g, ch, lenses):
    from multicamera_stitching_amd import _capi
    plan = _capi.Plan.cylindrical(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"], g["v0"], ch)
    for c, (K, d) in sorted(lenses.items()):
        plan.set_lens(c, K, d)
    assert plan.stats()["lens_cams"] == len(lenses)
    return plan


@functools.lru_cache(maxsize=None)
def _cyl_ref(name):
    """(seam mosaic, feather mosaic, owner map) of the lensed rig, computed once."""
    cams, frames, g, lenses, _ = _cyl_rig(name)
    pos, slot_cams = lens_ref.cyl_positions(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"],
                                            g["v0"], 1, lenses)
    seam, own = lens_ref.render_blend(pos, slot_cams, frames, "seam", want_owner=True)
    return seam, lens_ref.render_blend(pos, slot_cams, frames, "feather"), own


@pytest.mark.parametrize("name", list(CYLS))
def test_cylinder_vs_lens_ref(name):
    cams, frames, g, lenses, ch = _cyl_rig(name)
    plan = _cyl_plan(cams, g, ch, lenses)
    seam, feather, _ = _cyl_ref(name)
    for mode, want in ((SEAM, seam), (FEATHER, feather)):
        plan.set_blend(mode)
        assert _diff(plan.stitch_host(frames), want) == 0, mode
    assert seam.any()


# ---- identity lens: the whole lens plumbing against the existing oracle ----------------------
@pytest.mark.parametrize("mode", [NONE, SEAM, FEATHER])
def test_identity_lens_chain_equals_oracle(mode):
    plan, cams = _chain_plan(3, 160, 120, 3, lenses={c: IDENTITY for c in range(3)})
    plan.set_blend(mode)
    flat = plan.describe()
    want = oracle.flat_stitch(flat, cams) if mode == NONE else oracle.blend_stitch(flat, cams, mode)
    assert _diff(plan.stitch_host(cams), want) == 0


def test_identity_lens_chain_multiband_equals_oracle(mb_path):
    plan, cams = _chain_plan(3, 160, 120, 3, lenses={c: IDENTITY for c in range(3)})
    plan.set_blend(MULTIBAND)
    want = oracle.blend_stitch(plan.describe(), cams, MULTIBAND)
    assert _diff(plan.stitch_host(cams), want) == 0


def _identity_cyl():
    cams, frames, g, _, ch = _cyl_rig("8x320x180x3", seed=1)
    plan = _cyl_plan(cams, g, ch, {c: IDENTITY for c in range(len(cams))})
    ref = functools.partial(oracle.blend_stitch_cyl, cams, g["out_w"], g["out_h"], g["f_cyl"],
                            g["u0"], g["v0"], frames)
    return plan, frames, ref


@pytest.mark.parametrize("mode", [SEAM, FEATHER])
def test_identity_lens_cylinder_equals_oracle(mode):
    plan, frames, ref = _identity_cyl()
    plan.set_blend(mode)
    assert _diff(plan.stitch_host(frames), ref(mode)) == 0


def test_identity_lens_cylinder_multiband_equals_oracle(mb_path):
    plan, frames, ref = _identity_cyl()
    assert plan.stats()["lens_cams"] == 8
    assert _diff(plan.stitch_host(frames), ref(MULTIBAND)) == 0


def test_identity_lens_cylinder_graphcut_equals_oracle(mb_path):
    plan, frames, ref = _identity_cyl()
    plan.find_seams(frames, scale_log2=2)
    want, lab = ref(MULTIBAND, seam_k=2, want_seams=True)
    assert np.array_equal(plan.seam_labels(), lab)
    assert _diff(plan.stitch_host(frames), want) == 0


# ---- multi-band with a real lens --------------------------------------------------------------
def _single_owner_windows(own, r=16):
    """Pixels whose +-r window of the owner map (clipped at the mosaic edge) holds one value
    other than 255."""
    lo, hi = own.copy(), own.copy()
    for axis in (0, 1):
        pad = [(r, r) if a == axis else (0, 0) for a in (0, 1)]
        pl, ph = np.pad(lo, pad, mode="edge"), np.pad(hi, pad, mode="edge")
        n = own.shape[axis]
        sl = [np.take(pl, range(k, k + n), axis=axis) for k in range(2 * r + 1)]
        sh = [np.take(ph, range(k, k + n), axis=axis) for k in range(2 * r + 1)]
        lo, hi = np.minimum.reduce(sl), np.maximum.reduce(sh)
    return (lo == hi) & (lo != lens_ref.NONE)


def test_multiband_with_a_real_lens(mb_path):
    """Away from the seams (one owner within the pyramid's 16 px reach, kBlendHalo) the
    multi-band mosaic is the owner's sample, i.e. the lens_ref SEAM mosaic; then a device batch
    of 3 different captures equals the single-capture results."""
    import torch
    name = "8x320x180x3"
    cams, frames, g, lenses, ch = _cyl_rig(name)
    seam, _, own = _cyl_ref(name)
    quiet = _single_owner_windows(own)
    assert quiet.mean() >= 0.4, quiet.mean()       # the check covers enough of the mosaic
    plan = _cyl_plan(cams, g, ch, lenses)
    got = plan.stitch_host(frames).reshape(seam.shape)
    assert _diff(got[quiet], seam[quiet]) == 0
    assert (got != seam).any()                      # (and the seams are blended)
    F = 3
    shots = [[np.roll(c, 5 * f, axis=1) for c in frames] for f in range(F)]
    dev = [torch.from_numpy(np.stack([shots[f][i] for f in range(F)])).cuda()
           for i in range(len(frames))]
    out = torch.zeros((F, plan.out_h, plan.out_w * ch), dtype=torch.uint8, device="cuda")
    plan.stitch_device([d.data_ptr() for d in dev], [d[0].numel() for d in dev],
                       out.data_ptr(), plan.out_w * ch, out[0].numel(), F, 0)
    torch.cuda.synchronize()
    batch = out.cpu().numpy()
    for f in range(F):
        assert _diff(batch[f], plan.stitch_host(shots[f])) == 0, f


# ---- direct path, side paths, drop-in ---------------------------------------------------------
@pytest.mark.parametrize("mode", [NONE, SEAM])
def test_direct_path_equals_device_equals_lens_ref(mode):
    import torch
    n, w, h, ch = 3, 160, 120, 3
    lenses = _variant("all", n, w, h)
    plan, cams = _chain_plan(n, w, h, ch, lenses=lenses)
    plan.set_blend(mode)
    want = _chain_want(plan.describe(), cams, 1, lenses, mode)
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cams]
    outs = []
    for fn in (plan.stitch_direct, plan.stitch_device):
        out = torch.zeros((plan.out_h, plan.out_w * ch), dtype=torch.uint8, device="cuda")
        fn([d.data_ptr() for d in dev], [d.numel() for d in dev], out.data_ptr(),
           plan.out_w * ch, out.numel(), 1, 0)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert _diff(outs[0], want) == 0 and _diff(outs[1], want) == 0


def test_strong_lens_reaches_the_side_paths():
    """A warp plan whose wide-angle lens (f = 0.35 w; k2 stretches the corners, whose r2 reaches
    2.7) grows and curves the footprints of the corner tiles past the streaming block's budget
    (a CPU model of prepare_tile's rule puts 14 of the 450 tiles on the large-footprint list):
    those tiles take the large-footprint or the direct-gather kernel, and the mosaic still equals
    the specification."""
    from multicamera_stitching_amd import _capi, rig
    w, h, ch = 1280, 720, 3
    frame = rig.texture(h, w, ch, seed=11)
    M = np.array([[1.0, 0.02, -3.0], [-0.015, 1.0, 2.0], [1e-6, -2e-6, 1.0]])
    lens = ([[0.35 * w, 0, w / 2 - 0.5 + 1.3], [0, 0.35 * w, h / 2 - 0.5 - 0.7], [0, 0, 1]],
            CASES[0]["d"])
    plan = _capi.Plan.warp(M, w, h, w, h, ch)
    plan.set_lens(0, *lens)
    got = plan.stitch_host([frame])
    st = plan.stats()
    print("tiles %d, big-footprint %d, direct %d" % (st["tiles"], st["big_tiles"],
                                                     st["direct_tiles"]))
    pos, slot_cams, rects = lens_ref.chain_positions(plan.describe(), 1, {0: lens}, single=True)
    want = lens_ref.render_paste(pos, slot_cams, rects, [frame])
    assert _diff(got, want) == 0
    assert st["big_tiles"] + st["direct_tiles"] >= 1, st


@pytest.mark.parametrize("which", ["all", "cam1"])
def test_footprint_of_a_lensed_plan(which):
    """mcs_plan_footprint (the roofline's touched source pixels) follows the lens: per camera
    the distinct raw pixels the paste mosaic reads with a non-zero weight."""
    n, w, h, ch = 3, 160, 120, 3
    lenses = _variant(which, n, w, h)
    plan, _ = _chain_plan(n, w, h, ch, lenses=lenses)
    pos, slot_cams, rects = lens_ref.chain_positions(plan.describe(), 1, lenses)
    sel = lens_ref.paste_owner(rects, pos[0][0].shape)
    want = [0] * n
    for s, ((x32, y32), cam) in enumerate(zip(pos, slot_cams)):
        x32, y32 = x32[sel == s], y32[sel == s]
        sx, sy, fx, fy = x32 >> 5, y32 >> 5, x32 & 31, y32 & 31
        taps = [(sx, sy, fx >= 0), (sx + 1, sy, fx > 0), (sx, sy + 1, fy > 0),
                (sx + 1, sy + 1, (fx > 0) & (fy > 0))]
        hit = np.zeros((h, w), bool)
        for tx, ty, live in taps:
            ok = live & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            hit[ty[ok], tx[ok]] = True
        want[cam] += int(hit.sum())
    assert plan.footprint() == want and min(want) > 0


def test_drop_in_set_lenses():
    """Stitcher.set_lenses, then stitch(raw frames): the lensed plan's mosaic; without it the
    drop-in's output is what it was."""
    n, w, h, ch = 3, 160, 120, 3
    st, images, cams, _ = _chain_rig(n, w, h, ch)
    plain, _ = _chain_plan(n, w, h, ch)
    unlensed = oracle.flat_stitch(plain.describe(), cams)
    assert _diff(st.stitch(images), unlensed) == 0
    lenses = _variant("all", n, w, h)
    try:
        st.set_lenses({label: lenses[i] for i, label in enumerate(st.img_labels)})
        want = _chain_want(plain.describe(), cams, 1, lenses, NONE)
        assert _diff(st.stitch(images), want) == 0
        st.set_lenses({st.img_labels[1]: lenses[1], st.img_labels[0]: None})
        want = _chain_want(plain.describe(), cams, 1, {1: lenses[1]}, NONE)
        assert _diff(st.stitch(images), want) == 0
    finally:
        st.set_lenses({})
    assert _diff(st.stitch(images), unlensed) == 0
