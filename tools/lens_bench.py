"""What the fused lens costs and saves: the bench's C2 rig (4 x 1920x1080, 64 resident captures,
multi-band) stitched from raw frames three ways, alternated step by step in one process:

  a  the unlensed plan (frames taken as already undistorted: the floor);
  b  the lensed plan (mcs_plan_set_lens): raw frames in, one pass;
  c  four undistort plans' stitch_device into scratch frames, then a: what a caller of
     cv2.undistort + Stitcher.stitch pays today.

HIP events around every launch (or launch group), warm-up rounds, then per variant the median and
spread of --steps launches, with the plan stats that explain them (streaming DMA bytes, large-
footprint and direct-gather tiles, blend tiles).  --blend seam times the streaming launch alone
(no blend kernels).  --model fisheye gives every camera a cv2.fisheye lens instead (default D
[0.25, 0, 0, 0]: the corner and the edge centres move as under the polynomial default); variant c's
undistort pass is then an identity warp plan with the fisheye lens, since there is no fisheye table
plan.  Also reported: mcs_plan_prepare of the unlensed and the lensed plan (host clock, first
prepare of a fresh plan, synchronised) and the table-free direct stitch (paste) per capture of
both.  One JSON line; --out also writes it to a file.

    python tools/lens_bench.py --steps 20 --out profiles/lens_bench.json
    python tools/lens_bench.py --model fisheye --out profiles/fisheye_lens_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the bench's mild lens (also tools/estimate_bench.py --lens)
FOCAL = 1100.0
DIST = (-0.12, 0.03, 0.0, 0.0)
# theta_d / r at the corner (r = 1.0) is 0.907 and at the edge centre (r = 0.87) 0.928, against
# the polynomial's 0.910 and 0.926
FISH_DIST = (0.25, 0.0, 0.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--focal", type=float, default=FOCAL)
    ap.add_argument("--dist", type=float, nargs="*", default=None)
    ap.add_argument("--model", choices=["pinhole", "fisheye"], default="pinhole")
    ap.add_argument("--blend", choices=["multiband", "feather", "seam", "none"],
                    default="multiband", help="seam / none: the streaming launch alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.dist is None:
        args.dist = list(FISH_DIST if args.model == "fisheye" else DIST)

    import time

    import torch
    from multicamera_stitching_amd import _capi, rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc

    n, w, h, C, F = 4, args.width, args.height, 3, args.frames
    st, images, _ = rig.calibrated_stitcher(n, w, h, C, seed=0)
    cams = [images[label] for label in st.img_labels]
    descs = [_stage_desc(sb) for sb in st.stitchers]
    K = [[args.focal, 0, (w - 1) / 2.0], [0, args.focal, (h - 1) / 2.0], [0, 0, 1]]

    def chain(lensed, blend=args.blend):
        p = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
        p.set_blend({"multiband": _capi.MCS_BLEND_MULTIBAND, "feather": _capi.MCS_BLEND_FEATHER,
                     "seam": _capi.MCS_BLEND_SEAM, "none": _capi.MCS_BLEND_NONE}[blend])
        if lensed:
            for c in range(n):
                p.set_lens(c, K, args.dist, args.model)
        return p

    def undistort_plan():
        if args.model == "pinhole":
            return _capi.Plan.undistort(K, args.dist, w, h, C)
        return _capi.Plan.warp(np.eye(3), w, h, w, h, C).set_lens(0, K, args.dist, "fisheye")

    plain, fused = chain(False), chain(True)
    undist = [undistort_plan() for _ in range(n)]

    dev = torch.device("cuda", 0)
    d_cams = []
    for c in cams:
        base = torch.from_numpy(c).to(dev)
        d_cams.append(torch.stack([torch.roll(base, shifts=f % h, dims=0)
                                   for f in range(F)]).contiguous())
    d_und = [torch.empty_like(t) for t in d_cams]
    out_w, out_h = plain.out_w, plain.out_h
    pitch = (out_w * C + 255) // 256 * 256
    d_out = torch.empty((F, out_h, pitch), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    chain(False).prepare(stream.cuda_stream)    # (kernel lookup and first-use costs: not timed)
    chain(True).prepare(stream.cuda_stream)
    torch.cuda.synchronize()
    prepare_ms = {}
    for name, p in (("a_unlensed", plain), ("b_fused", fused)):
        t0 = time.perf_counter()
        p.prepare(stream.cuda_stream)
        torch.cuda.synchronize()
        prepare_ms[name] = round((time.perf_counter() - t0) * 1e3, 3)
    for p in undist:
        p.prepare(stream.cuda_stream)
    torch.cuda.synchronize()

    def stitch(plan, src):
        plan.stitch_device([t.data_ptr() for t in src], [t[0].numel() for t in src],
                           d_out.data_ptr(), pitch, d_out[0].numel(), F, stream.cuda_stream)

    def two_step():
        for c in range(n):
            undist[c].stitch_device([d_cams[c].data_ptr()], [d_cams[c][0].numel()],
                                    d_und[c].data_ptr(), w * C, d_und[c][0].numel(), F,
                                    stream.cuda_stream)
        stitch(plain, d_und)

    # the table-free path (a plan that lives for one capture): paste, never prepared
    direct = {"direct_unlensed": chain(False, "none"), "direct_lensed": chain(True, "none")}

    def stitch_direct(plan):
        plan.stitch_direct([t.data_ptr() for t in d_cams], [t[0].numel() for t in d_cams],
                           d_out.data_ptr(), pitch, d_out[0].numel(), F, stream.cuda_stream)

    variants = {"a_unlensed": lambda: stitch(plain, d_cams),
                "b_fused": lambda: stitch(fused, d_cams),
                "c_undistort_then_stitch": two_step,
                "direct_unlensed": lambda: stitch_direct(direct["direct_unlensed"]),
                "direct_lensed": lambda: stitch_direct(direct["direct_lensed"])}
    for _ in range(args.warmup):
        for run in variants.values():
            run()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(args.steps)] for k in variants}
    for i in range(args.steps):
        for k, run in variants.items():     # alternated: drift hits every variant alike
            ev[k][i][0].record(stream)
            run()
            ev[k][i][1].record(stream)
    torch.cuda.synchronize()

    def summary(k):
        ms = np.array([a.elapsed_time(b) for a, b in ev[k]])
        q1, med, q3 = np.percentile(ms, [25, 50, 75])
        return {"ms_median": round(float(med), 4), "ms_min": round(float(ms.min()), 4),
                "ms_max": round(float(ms.max()), 4), "ms_iqr": round(float(q3 - q1), 4)}

    def stats(p):
        s = p.stats()
        return {"stream_dma_bytes_per_capture": int(s["dma_bytes_per_capture"]),
                "tiles": int(s["tiles"]), "big_tiles": int(s["big_tiles"]),
                "direct_tiles": int(s["direct_tiles"]), "blend_tiles": int(s["blend_tiles"]),
                "lens_cams": int(s["lens_cams"])}

    line = {"tool": "lens_bench", "rig": "%d x %dx%dx%d" % (n, w, h, C), "frames": F,
            "blend": args.blend, "steps": args.steps, "warmup": args.warmup, "focal": args.focal,
            "dist": args.dist, "model": args.model, "prepare_ms": prepare_ms,
            "direct_unlensed": dict(summary("direct_unlensed"),
                                    us_per_capture=round(1e3 * summary("direct_unlensed")["ms_median"] / F, 3)),
            "direct_lensed": dict(summary("direct_lensed"),
                                  us_per_capture=round(1e3 * summary("direct_lensed")["ms_median"] / F, 3)),
            "mosaic": [out_w, out_h], "build_id": _capi.load().mcs_build_id().decode(),
            "source_bytes_per_launch": n * w * h * C * F,
            "a_unlensed": dict(summary("a_unlensed"), plan=stats(plain)),
            "b_fused": dict(summary("b_fused"), plan=stats(fused)),
            "c_undistort_then_stitch": dict(summary("c_undistort_then_stitch"),
                                            undistort_plan=stats(undist[0]))}
    a, b, c = (line[k]["ms_median"] for k in ("a_unlensed", "b_fused", "c_undistort_then_stitch"))
    line["b_minus_a_ms"] = round(b - a, 4)
    line["c_minus_a_ms"] = round(c - a, 4)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
