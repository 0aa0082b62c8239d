"""What a blended stitch of ONE capture with its own geometry costs on the C3 rig (4 x 1920x1080x3
from rig.calibrated_stitcher, frames resident on the device) -- a fresh plan per call, as config 3
builds one per capture:

  (a) direct paste     Plan + mcs_stitch_direct                                   (mcs_direct_*)
  (b) direct seam      Plan + set_blend(SEAM) + mcs_stitch_direct                 (mcs_direct_*)
  (c) direct feather   Plan + set_blend(FEATHER) + mcs_stitch_direct      (mcs_direct_feather_*)
  (d) prepared feather Plan + set_blend(FEATHER) + mcs_plan_prepare + mcs_stitch_device +
                       mcs_plan_destroy: the only route to a feathered capture before (c)
  (e) direct multi-band   Plan + set_blend(MULTIBAND) + mcs_stitch_direct_multiband, the work
                          area allocated once outside the loop            (mcs_direct_mb_own_* +
                                                                           mcs_direct_mb_tile_*)
  (f) prepared multi-band Plan + set_blend(MULTIBAND) + mcs_plan_prepare + mcs_stitch_device +
                          mcs_plan_destroy: the only route to a multi-band capture before (e)

Every variant is timed with a host clock from before the plan is created to after a device
synchronise (prepare is host-driven, so only this clock compares them); (a) to (c) and (e) also
with HIP events around the stitch call alone (both launches of (e) together; a kernel trace of
this tool gives them apart).  --warmup rounds, then --steps repeats with the variants
alternated inside each round; median (min-max) in ms.  Prints the lines and, with --out, writes
them to a file.

    python tools/direct_blend_bench.py --out profiles/direct_multiband_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ms):
    ms = np.asarray(ms, np.float64)
    return "%.4f (%.4f-%.4f)" % (float(np.median(ms)), float(ms.min()), float(ms.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from multicamera_stitching_amd import _capi, rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    n, w, h, C = 4, args.width, args.height, 3
    st, images, _ = rig.calibrated_stitcher(n, w, h, C, seed=0)
    descs = [_stage_desc(sb) for sb in st.stitchers]
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(images[label]).to(dev) for label in st.img_labels]
    ptrs = [t.data_ptr() for t in d]
    strides = [t.numel() for t in d]
    probe = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
    ow, oh = probe.out_w, probe.out_h
    mb_work = probe.direct_multiband_work_size()
    probe.close()
    pitch = (ow * C + 255) // 256 * 256
    out = torch.empty((oh, pitch), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def direct(mode):
        def run():
            t0 = time.perf_counter()
            plan = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
            if mode != _capi.MCS_BLEND_NONE:
                plan.set_blend(mode)
            ev0.record()
            plan.stitch_direct(ptrs, strides, out.data_ptr(), pitch, pitch * oh, 1, stream)
            ev1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            plan.close()
            return (t1 - t0) * 1e3, ev0.elapsed_time(ev1)
        return run

    def prepared(mode):
        def run():
            t0 = time.perf_counter()
            plan = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
            plan.set_blend(mode)
            plan.prepare(stream)
            plan.stitch_device(ptrs, strides, out.data_ptr(), pitch, pitch * oh, 1, stream)
            torch.cuda.synchronize()
            plan.close()
            return (time.perf_counter() - t0) * 1e3, None
        return run

    # the multi-band work area: the caller's, allocated once (its size depends on the mosaic only)
    work = torch.empty(mb_work, dtype=torch.uint8, device=dev)

    def direct_multiband():
        t0 = time.perf_counter()
        plan = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
        plan.set_blend(_capi.MCS_BLEND_MULTIBAND)
        ev0.record()
        plan.stitch_direct_multiband(ptrs, strides, out.data_ptr(), pitch, pitch * oh, 1,
                                     work.data_ptr(), work.numel(), stream)
        ev1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        plan.close()
        return (t1 - t0) * 1e3, ev0.elapsed_time(ev1)

    variants = [("a direct paste", direct(_capi.MCS_BLEND_NONE)),
                ("b direct seam", direct(_capi.MCS_BLEND_SEAM)),
                ("c direct feather", direct(_capi.MCS_BLEND_FEATHER)),
                ("d prepared feather (prepare + stitch_device + destroy)",
                 prepared(_capi.MCS_BLEND_FEATHER)),
                ("e direct multi-band (work area: %d bytes)" % mb_work, direct_multiband),
                ("f prepared multi-band (prepare + stitch_device + destroy)",
                 prepared(_capi.MCS_BLEND_MULTIBAND))]
    host = {name: [] for name, _ in variants}
    devt = {name: [] for name, _ in variants}
    for step in range(args.warmup + args.steps):
        for name, fn in variants:
            th, td = fn()
            if step >= args.warmup:
                host[name].append(th)
                if td is not None:
                    devt[name].append(td)
    lines = ["direct blend bench: %d x %dx%dx%d, mosaic %dx%d, one capture per call, a fresh plan "
             "per call; %d warm-up rounds, %d repeats, variants alternated; ms, median (min-max); "
             "build %s" % (n, w, h, C, ow, oh, args.warmup, args.steps, _capi.build_id())]
    for name, _ in variants:
        lines.append("%-56s host %s%s" % (name, spread(host[name]),
                                          "   device %s" % spread(devt[name]) if devt[name]
                                          else ""))
    med = {name[0]: float(np.median(host[name])) for name, _ in variants}
    dmed = {name[0]: float(np.median(devt[name])) for name, _ in variants if devt[name]}
    d_min = float(np.min(host[variants[3][0]]))
    f_min = float(np.min(host[variants[5][0]]))
    lines.append("c - b: host %.4f ms, device %.4f ms;  c - a: host %.4f ms, device %.4f ms;  "
                 "c / b: device %.2f" % (med["c"] - med["b"], dmed["c"] - dmed["b"],
                                         med["c"] - med["a"], dmed["c"] - dmed["a"],
                                         dmed["c"] / dmed["b"]))
    lines.append("bar (c median below d minimum): %.4f < %.4f: %s" % (
        med["c"], d_min, "holds" if med["c"] < d_min else "MISSED"))
    lines.append("e - b: host %.4f ms, device %.4f ms;  e - a: host %.4f ms, device %.4f ms;  "
                 "e / b: device %.2f" % (med["e"] - med["b"], dmed["e"] - dmed["b"],
                                         med["e"] - med["a"], dmed["e"] - dmed["a"],
                                         dmed["e"] / dmed["b"]))
    lines.append("bar (e median below f minimum): %.4f < %.4f: %s" % (
        med["e"], f_min, "holds" if med["e"] < f_min else "MISSED"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if med["c"] < d_min and med["e"] < f_min else 1


if __name__ == "__main__":
    sys.exit(main())
