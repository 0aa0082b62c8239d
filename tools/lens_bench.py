"""What the fused lens costs and saves: the bench's C2 rig (4 x 1920x1080, 64 resident captures,
multi-band) stitched from raw frames three ways, alternated step by step in one process:

  a  the unlensed plan (frames taken as already undistorted: the floor);
  b  the lensed plan (mcs_plan_set_lens): raw frames in, one pass;
  c  four undistort plans' stitch_device into scratch frames, then a: what a caller of
     cv2.undistort + Stitcher.stitch pays today.

HIP events around every launch (or launch group), warm-up rounds, then per variant the median and
spread of --steps launches, with the plan stats that explain them (streaming DMA bytes, large-
footprint and direct-gather tiles, blend tiles).  --blend seam times the streaming launch alone
(no blend kernels).  One JSON line; --out also writes it to a file.

    python tools/lens_bench.py --steps 20 --out profiles/lens_bench.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--focal", type=float, default=FOCAL)
    ap.add_argument("--dist", type=float, nargs="*", default=list(DIST))
    ap.add_argument("--blend", choices=["multiband", "feather", "seam", "none"],
                    default="multiband", help="seam / none: the streaming launch alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from multicamera_stitching_amd import _capi, rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc

    n, w, h, C, F = 4, args.width, args.height, 3, args.frames
    st, images, _ = rig.calibrated_stitcher(n, w, h, C, seed=0)
    cams = [images[label] for label in st.img_labels]
    descs = [_stage_desc(sb) for sb in st.stitchers]
    K = [[args.focal, 0, (w - 1) / 2.0], [0, args.focal, (h - 1) / 2.0], [0, 0, 1]]

    def chain(lensed):
        p = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
        p.set_blend({"multiband": _capi.MCS_BLEND_MULTIBAND, "feather": _capi.MCS_BLEND_FEATHER,
                     "seam": _capi.MCS_BLEND_SEAM, "none": _capi.MCS_BLEND_NONE}[args.blend])
        if lensed:
            for c in range(n):
                p.set_lens(c, K, args.dist)
        return p

    plain, fused = chain(False), chain(True)
    undist = [_capi.Plan.undistort(K, args.dist, w, h, C) for _ in range(n)]

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
    for p in [plain, fused] + undist:
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

    variants = {"a_unlensed": lambda: stitch(plain, d_cams),
                "b_fused": lambda: stitch(fused, d_cams),
                "c_undistort_then_stitch": two_step}
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
            "dist": args.dist,
            "mosaic": [out_w, out_h], "build_id": _capi.load().mcs_build_id().decode(),
            "source_bytes_per_launch": n * w * h * C * F,
            "a_unlensed": dict(summary("a_unlensed"), plan=stats(plain)),
            "b_fused": dict(summary("b_fused"), plan=stats(fused)),
            "c_undistort_then_stitch": dict(summary("c_undistort_then_stitch"),
                                            undistort_plan=stats(undist[0]))}
    a, b, c = (line[k]["ms_median"] for k in variants)
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
