"""The multi-band blend kernel's per-tile work records (mcs_kparams.h "Blend work records":
built once per plan by mcs_mb_prep_*, read by mcs_mb_blend_c*_s*) at the sizes where a record can
be wrong: mosaic borders in both directions and both parities of every level size (the records
hold reflected and clamped indices), lists that run into a second and a third iteration per
thread, every (channels, owner slots) specialisation, and several captures per launch.  The bar
is the CPU restatement orc_blend.c, difference 0: the blend's arithmetic is IEEE double over exact
integers, so the records change where an operand is read from, never its value.

Not asserted here: a listed tile without a mixed pixel (the block's early exit behind loads it has
already issued).  plan.stats() gives the lists' totals, not a tile's counts, so no test can name
such a tile; the full-size plans of test_gpu_blend.py list 177 tiles around three seams and are
the likeliest to hold one."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

MULTIBAND = 2


@pytest.fixture(autouse=True)
def _band_pass_and_blend(monkeypatch):
    """The blend kernel runs on the default path only (the opt-in sweep kernel replaces it)."""
    monkeypatch.setenv("MCS_MB_SWEEP", "0")


def _world_plan(n, w, h, ch, seed, interp=1, **kw):
    from multicamera_stitching_amd import rig, _capi
    from multicamera_stitching_amd.StitcherClass import Stitcher, _stage_desc
    C = rig.camera_models(n, w, h, seed=seed, **kw)
    frames = rig.world_frames(C, w, h, ch, seed=seed)
    images = dict(zip(rig.labels(n), frames))
    st = Stitcher(images)
    st.calibrate_stitcher(images, save=False,
                          homographies=rig.homography_provider(C, lambda: st.stitchers))
    cams = [images[label] for label in st.img_labels]
    plan = _capi.Plan([_stage_desc(sb) for sb in st.stitchers], w, h, ch, interp)
    plan.set_blend(MULTIBAND)
    return plan, cams


def _diff(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max()) if a.size else 0


def _check_host(plan, cams):
    got = plan.stitch_host(cams)
    want = oracle.blend_stitch(plan.describe(), cams, MULTIBAND)
    assert _diff(got.reshape(want.shape), want) == 0
    st = plan.stats()
    assert st["blend"] == MULTIBAND and st["blend_tiles"] > 0 and st["mb_sweep_strips"] == 0, st
    # (the plan counts its mixed pixels where it plans a band pass: mosaics of >= 128 px a side)
    if min(plan.out_w, plan.out_h) >= 128:
        assert st["mb_mixed_px"] > 0 and st["mb_bands"] > 0, st
    else:
        assert st["mb_bands"] == 0, st
    return st


# Frames whose mosaics put every blend tile on a border: lower than 96 rows (every tile an edge
# tile in y: the 16-px halo of a 64-row tile leaves the mosaic at the top or the bottom), one tile
# column, odd and even sizes.  (w1, h1) = level-1 size, (w2, h2) = level-2 size of the mosaic.
BORDER_CASES = [
    dict(n=2, w=150, h=90, ch=3, seed=5, rot_deg=2.0),
    dict(n=3, w=151, h=91, ch=3, seed=21),
    dict(n=3, w=202, h=110, ch=3, seed=13),
    dict(n=4, w=64, h=48, ch=3, seed=10, overlap=0.8),    # < 128 px a side: mb_levels feeds the blend
    dict(n=2, w=20, h=70, ch=3, seed=22, overlap=0.5, rot_deg=0.0, persp=0.0),   # one tile column
    dict(n=2, w=21, h=67, ch=3, seed=23, overlap=0.5, rot_deg=0.0, persp=0.0),
    dict(n=3, w=153, h=93, ch=3, seed=24, rot_deg=1.0),
    dict(n=2, w=148, h=94, ch=3, seed=25, rot_deg=0.0, persp=0.0),
]


@pytest.mark.parametrize("case", BORDER_CASES)
def test_records_reflect_at_every_border(case):
    plan, cams = _world_plan(**case)
    _check_host(plan, cams)


def test_border_cases_cover_sizes_and_parities():
    """What the cases above are there for, checked on their own mosaics: both parities of W, H,
    w1, h1, w2 and h2, mosaics lower than 96 rows, mosaics of one tile column, and mosaics under
    128 px a side (no band pass: mb_levels computes the levels the blend kernel reads)."""
    seen = {k: set() for k in ("W", "H", "w1", "h1", "w2", "h2")}
    low = one_col = small = 0
    for case in BORDER_CASES:
        plan, _cams = _world_plan(**case)
        W, H = plan.out_w, plan.out_h
        plan.close()
        w1, h1 = (W + 1) // 2, (H + 1) // 2
        sizes = dict(W=W, H=H, w1=w1, h1=h1, w2=(w1 + 1) // 2, h2=(h1 + 1) // 2)
        for k, v in sizes.items():
            seen[k].add(v & 1)
        low += H < 96
        one_col += W <= 32
        small += max(W, H) < 128
    assert all(v == {0, 1} for v in seen.values()), seen
    assert low >= 4 and one_col >= 2 and small >= 1, (low, one_col, small)


# Dense-seam rigs: many owners a few pixels apart make almost every pixel of a tile a mixed one.
# (Unrotated, so the mosaic is 128 rows: two full tile rows.)
MANY_R1 = dict(n=8, w=72, h=128, ch=3, seed=11, step=10, rot_deg=0.0, persp=0.0)
MANY_PX = MANY_R1


def test_records_second_r1_iteration():
    """More than 256 listed R1 entries per tile on average: some tile's threads run a second
    iteration of R1 records."""
    plan, cams = _world_plan(**MANY_R1)
    st = _check_host(plan, cams)
    assert st["mb_r1_entries"] / st["blend_tiles"] > 256, st


def test_records_third_pixel_iteration():
    """More than 512 listed mixed pixels per tile on average: some tile's threads run a third
    iteration of pixel records."""
    plan, cams = _world_plan(**MANY_PX)
    st = _check_host(plan, cams)
    assert st["mb_mixed_px"] / st["blend_tiles"] > 512, st


# (cameras, frame width, camera step) whose neighbourhoods hold <= 2, <= 4 and <= 8 owners: the
# plans that select mcs_mb_blend_c*_s2, _s4 and _s8.
SLOT_RIGS = {2: dict(n=2, w=72, h=40, overlap=0.4),
             4: dict(n=4, w=64, h=48, overlap=0.8),
             8: dict(n=8, w=64, h=30, step=5)}


@pytest.mark.parametrize("ch", [1, 2, 3, 4])
@pytest.mark.parametrize("slots", [2, 4, 8])
def test_records_every_specialisation(slots, ch):
    plan, cams = _world_plan(ch=ch, seed=11, **SLOT_RIGS[slots])
    st = _check_host(plan, cams)
    lo = {2: 2, 4: 3, 8: 5}[slots]
    assert lo <= st["mb_owners"] <= slots, st


@pytest.mark.parametrize("F", [1, 3])
def test_records_several_captures_per_launch(F):
    """One stitch_device launch of F distinct captures (the band pass works on pairs of captures,
    the blend per capture): every capture against the restatement."""
    import torch
    plan, cams = _world_plan(3, 160, 140, 3, seed=12)
    rng = np.random.default_rng(7)
    shots = [cams] + [[rng.integers(1, 256, size=c.shape, dtype=np.uint8) for c in cams]
                      for _ in range(F - 1)]
    dev = [torch.from_numpy(np.stack([shots[f][i] for f in range(F)])).cuda()
           for i in range(len(cams))]
    pitch = (plan.out_w * 3 + 63) // 64 * 64
    out = torch.zeros((F, plan.out_h, pitch), dtype=torch.uint8, device="cuda")
    plan.stitch_device([d.data_ptr() for d in dev], [d[0].numel() for d in dev],
                       out.data_ptr(), pitch, out[0].numel(), F, 0)
    torch.cuda.synchronize()
    got = out[:, :, :plan.out_w * 3].cpu().numpy()
    st = plan.stats()
    assert st["blend_tiles"] > 0 and st["mb_bands"] > 0 and st["mb_sweep_strips"] == 0, st
    for f in range(F):
        want = oracle.blend_stitch(plan.describe(), shots[f], MULTIBAND)
        assert _diff(got[f].reshape(want.shape), want) == 0, f


@pytest.mark.parametrize("ch", [1, 2, 4])
def test_band_pass_other_channel_counts(ch):
    """The band pass at 1, 2 and 4 channels (every other case with those channel counts has a
    mosaic under 128 px a side and takes mcs_mb_levels).  The plan's own aligned launch first;
    then one launch of F = 3 captures (an odd tail for the band pass's pairs of captures) whose
    camera pointers start one byte off a 4-byte boundary, so the band pass takes its unaligned
    window form -- every capture against the restatement."""
    import torch
    plan, cams = _world_plan(3, 160, 140, ch, seed=12)
    st = _check_host(plan, cams)
    assert st["mb_bands"] > 0, st
    print("mb_bands", st["mb_bands"], "mb_bands_lds", st["mb_bands_lds"])
    F, shift = 3, 1
    rng = np.random.default_rng(7)
    shots = [cams] + [[rng.integers(1, 256, size=c.shape, dtype=np.uint8) for c in cams]
                      for _ in range(F - 1)]
    fb = cams[0].size
    dev = []
    for i in range(len(cams)):
        buf = torch.zeros(shift + F * fb + 16, dtype=torch.uint8)
        for f in range(F):
            buf[shift + f * fb: shift + (f + 1) * fb] = torch.from_numpy(shots[f][i].reshape(-1))
        dev.append(buf.cuda())
    pitch = (plan.out_w * ch + 63) // 64 * 64
    out = torch.zeros((F, plan.out_h, pitch), dtype=torch.uint8, device="cuda")
    plan.stitch_device([d.data_ptr() + shift for d in dev], [fb] * len(dev),
                       out.data_ptr(), pitch, out[0].numel(), F, 0)
    torch.cuda.synchronize()
    got = out[:, :, :plan.out_w * ch].cpu().numpy()
    for f in range(F):
        want = oracle.blend_stitch(plan.describe(), shots[f], MULTIBAND)
        assert _diff(got[f].reshape(want.shape), want) == 0, f
