"""Fisheye lenses on the GPU (mcs_plan_set_lens_model, MCS_LENS_FISHEYE): raw fisheye frames in,
one pass.  Every mode and path against the numpy specification tests/fisheye_ref.py, rigs that mix
fisheye, polynomial and lens-free cameras included.  The bar is max |diff| = 0 throughout."""
import functools

import numpy as np
import pytest

import fisheye_ref
import gain_ref
from test_undistort_cpu import CASES

pytestmark = pytest.mark.gpu

NONE, FEATHER, MULTIBAND, SEAM = 0, 1, 2, 3
FISH_D = [[-0.03, 0.01, -0.002, 0.0005], [0.02, -0.004, 0.001, 0.0], None]


def _diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.size == b.size, (a.shape, b.shape)
    return int(np.abs(a.reshape(b.shape).astype(np.int16) - b.astype(np.int16)).max())


def _K(w, h, f):
    return [[f * w, 0, w / 2 - 0.5 + 1.3], [0, f * w, h / 2 - 0.5 - 0.7], [0, 0, 1]]


def _fish(w, h, dist, f=0.7):
    return (_K(w, h, f), dist, "fisheye")


@functools.lru_cache(maxsize=None)
def _chain_rig(n, w, h, ch, super_mode=False):
    from multicamera_stitching_amd import rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    st, images, _ = rig.calibrated_stitcher(n, w, h, ch, super_mode=super_mode, seed=1,
                                            rot_deg=2.0, persp=5e-5)
    cams = [images[label] for label in st.img_labels]
    return st, images, cams, [_stage_desc(sb) for sb in st.stitchers]


def _set(plan, lenses):
    for c, lens in sorted(lenses.items()):
        plan.set_lens(c, *lens)
    assert plan.stats()["lens_cams"] == len(lenses)
    return plan


def _chain_plan(n, w, h, ch, interp=1, super_mode=False, lenses=None):
    from multicamera_stitching_amd import _capi
    _, _, cams, descs = _chain_rig(n, w, h, ch, super_mode)
    return _set(_capi.Plan(descs, w, h, ch, interp), lenses or {}), cams


def _chain_want(flat, cams, interp, lenses, mode, **kw):
    pos, slot_cams, rects = fisheye_ref.chain_positions(flat, interp, lenses, **kw)
    if mode == NONE:
        return fisheye_ref.render_paste(pos, slot_cams, rects, cams)
    return fisheye_ref.render_blend(pos, slot_cams, cams, "seam" if mode == SEAM else "feather")


CHAINS = {
    "3x160x120x3": dict(n=3, w=160, h=120, ch=3),
    "4x128x96x1-nearest": dict(n=4, w=128, h=96, ch=1, interp=0),
    "3x96x64x4": dict(n=3, w=96, h=64, ch=4),
    "2x200x150x2-super": dict(n=2, w=200, h=150, ch=2, super_mode=True),
}


def _variant(which, n, w, h):
    if which == "all":
        return {c: _fish(w, h, FISH_D[c % 3]) for c in range(n)}
    if which == "cam0":
        return {0: _fish(w, h, FISH_D[0])}
    # mixed: camera 0 polynomial, camera 1 fisheye, the rest lens-free
    return {0: (_K(w, h, 0.9), CASES[0]["d"]), 1: _fish(w, h, FISH_D[1])}


@pytest.mark.parametrize("which", ["all", "cam0", "mixed"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_vs_fisheye_ref(name, which):
    """Paste, SEAM and FEATHER of fisheye chain plans through stitch_host."""
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
    # the lens is not a no-op on this rig
    plain = _chain_want(flat, cams, interp, {}, FEATHER)
    assert _diff(want, plain) > 0


@functools.lru_cache(maxsize=None)
def _cyl_rig():
    from multicamera_stitching_amd import rig
    cams, frames, g = rig.cylinder_rig(4, 128, 96, 70.0, 2, seed=5)
    lenses = {c: ([[k["f"], 0, k["cx"]], [0, k["f"], k["cy"]], [0, 0, 1]], FISH_D[c % 3], "fisheye")
              for c, k in enumerate(cams)}
    return cams, frames, g, lenses


def test_cylinder_vs_fisheye_ref():
    from multicamera_stitching_amd import _capi
    cams, frames, g, lenses = _cyl_rig()
    plan = _set(_capi.Plan.cylindrical(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"],
                                       g["v0"], 2), lenses)
    pos, slot_cams = fisheye_ref.cyl_positions(cams, g["out_w"], g["out_h"], g["f_cyl"], g["u0"],
                                               g["v0"], 1, lenses)
    for mode, name in ((SEAM, "seam"), (FEATHER, "feather")):
        plan.set_blend(mode)
        want = fisheye_ref.render_blend(pos, slot_cams, frames, name)
        assert _diff(plan.stitch_host(frames), want) == 0, mode
    assert want.any()
    # a cylinder plan has no paste rule: the third mode is SEAM through the direct path
    import torch
    plan.set_blend(SEAM)
    want = fisheye_ref.render_blend(pos, slot_cams, frames, "seam")
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in frames]
    out = torch.zeros((plan.out_h, plan.out_w * 2), dtype=torch.uint8, device="cuda")
    plan.stitch_direct([d.data_ptr() for d in dev], [d.numel() for d in dev], out.data_ptr(),
                       plan.out_w * 2, out.numel(), 1, 0)
    torch.cuda.synchronize()
    assert _diff(out.cpu().numpy(), want) == 0


def test_fold_back_angle_keeps_ghost_coverage_out():
    """k1 = -0.3 at f = 0.6 w: theta_d stops growing at theta = 1.054 (r = 1.76), inside the
    part of the mosaic its neighbours cover; without the valid-angle rule the far rays of a
    camera land inside its raw frame again."""
    w, h = 160, 120
    dist = [-0.3, 0, 0, 0]
    lenses = {c: _fish(w, h, dist, f=0.6) for c in range(3)}
    assert 1.0 < fisheye_ref.tmax(dist) < 1.1
    plan, cams = _chain_plan(3, w, h, 3, lenses=lenses)
    flat = plan.describe()
    sizes = {c: (w, h) for c in range(3)}
    owners = []
    for rule in (True, False):
        pos, slot_cams, _ = fisheye_ref.chain_positions(flat, 1, lenses, use_limit=rule)
        owners.append(fisheye_ref.owner_map(fisheye_ref.distances(pos, slot_cams, sizes),
                                            slot_cams))
    assert (owners[0] != owners[1]).sum() > 0      # the rule matters on this rig
    for mode in (SEAM, FEATHER):
        plan.set_blend(mode)
        assert _diff(plan.stitch_host(cams), _chain_want(flat, cams, 1, lenses, mode)) == 0, mode


# ---- the device paths on one all-fisheye rig ---------------------------------------------------
N, W, H, CH = 3, 160, 120, 3


def _upload(cams):
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cams]
    return dev, [d.data_ptr() for d in dev], [d.numel() for d in dev]


def _run(plan, fn, ptrs, strides, *extra):
    import torch
    out = torch.zeros((plan.out_h, plan.out_w * CH), dtype=torch.uint8, device="cuda")
    fn(ptrs, strides, out.data_ptr(), plan.out_w * CH, out.numel(), 1, *extra)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _multiband(plan, fn, ptrs, strides):
    import torch
    work = torch.empty(max(plan.direct_multiband_work_size(), 1), dtype=torch.uint8, device="cuda")
    return _run(plan, fn, ptrs, strides, work.data_ptr(), work.numel())


@pytest.mark.parametrize("mode", [NONE, SEAM, FEATHER, MULTIBAND])
def test_device_paths_equal_host_path(mode):
    """stitch_device after prepare and stitch_direct (multi-band: stitch_direct_multiband, written
    independently of the prepared kernels) equal stitch_host."""
    lenses = _variant("all", N, W, H)
    plan, cams = _chain_plan(N, W, H, CH, lenses=lenses)
    plan.set_blend(mode)
    want = plan.stitch_host(cams).reshape(plan.out_h, plan.out_w * CH)
    if mode != MULTIBAND:
        assert _diff(want, _chain_want(plan.describe(), cams, 1, lenses, mode)) == 0
    bufs, ptrs, strides = _upload(cams)
    plan.prepare()
    assert _diff(_run(plan, plan.stitch_device, ptrs, strides), want) == 0
    fresh, _ = _chain_plan(N, W, H, CH, lenses=lenses)      # (never prepared)
    fresh.set_blend(mode)
    if mode == MULTIBAND:
        got = _multiband(fresh, fresh.stitch_direct_multiband, ptrs, strides)
        plain, _ = _chain_plan(N, W, H, CH)
        plain.set_blend(mode)
        assert _diff(plain.stitch_host(cams), want) > 0     # the lens reaches the multi-band path
    else:
        got = _run(fresh, fresh.stitch_direct, ptrs, strides)
    assert _diff(got, want) == 0


@pytest.mark.parametrize("mode", [NONE, FEATHER, MULTIBAND])
def test_gained_forms_equal_the_stitch_of_pre_gained_frames(mode):
    gains = [1.25, 0.8, 1.1]
    assert all(gain_ref.quantise(g) != 256 for g in gains)
    lenses = _variant("all", N, W, H)
    plan, cams = _chain_plan(N, W, H, CH, lenses=lenses)
    plan.set_blend(mode)
    pre = [gain_ref.apply_gain(c, g) for c, g in zip(cams, gains)]
    want = plan.stitch_host(pre).reshape(plan.out_h, plan.out_w * CH)
    assert _diff(want, plan.stitch_host(cams)) > 0
    plan.set_gains(gains)
    bufs, ptrs, strides = _upload(cams)
    assert _diff(_run(plan, plan.stitch_device_gained, ptrs, strides), want) == 0
    fresh, _ = _chain_plan(N, W, H, CH, lenses=lenses)
    fresh.set_blend(mode)
    fresh.set_gains(gains)
    if mode == MULTIBAND:
        got = _multiband(fresh, fresh.stitch_direct_multiband_gained, ptrs, strides)
    else:
        got = _run(fresh, fresh.stitch_direct_gained, ptrs, strides)
    assert _diff(got, want) == 0


def test_overlap_statistics_follow_the_lens():
    lenses = _variant("all", N, W, H)
    plan, cams = _chain_plan(N, W, H, CH, lenses=lenses)
    k = 2
    pos, slot_cams, _ = fisheye_ref.chain_positions(plan.describe(), 1, lenses)
    want_N, want_S = gain_ref.overlap_stats(pos, slot_cams, [cams], k, N)
    assert want_N[0, 1] > 0 and want_N[1, 2] > 0
    plain = gain_ref.chain_stats(plan.describe(), [cams], k)
    assert not np.array_equal(plain[0], want_N)             # the lens moves the overlaps
    bufs, ptrs, strides = _upload(cams)
    for fn in (plan.overlap_stats_direct, plan.overlap_stats, plan.overlap_stats_direct):
        got_N, got_S = fn(ptrs, strides, 1, k)
        assert np.array_equal(got_N, want_N), (got_N.tolist(), want_N.tolist())
        assert np.array_equal(got_S, want_S)


def test_drop_in_set_lenses_takes_a_model():
    st, images, cams, _ = _chain_rig(N, W, H, CH)
    lenses = _variant("mixed", N, W, H)
    plain, _ = _chain_plan(N, W, H, CH)
    try:
        st.set_lenses({label: lenses.get(i) for i, label in enumerate(st.img_labels)})
        want = _chain_want(plain.describe(), cams, 1, lenses, NONE)
        assert _diff(st.stitch(images), want) == 0
    finally:
        st.set_lenses({})
