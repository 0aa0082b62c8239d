"""What exposure compensation costs on the bench's C2 rig (4 x 1920x1080x3, 64 resident captures):

  prep   the overlap table of a (plan, step), built by the first mcs_plan_overlap_stats call:
         that call's wall time minus a steady call's;
  stats  mcs_plan_overlap_stats over the 64 captures per grid step (accumulator memset, the
         mcs_overlap_sum launch, the copy back of S): HIP events around the call, and its wall time;
  apply  mcs_gain_apply_device over every camera's 64 frames, in place (reads and writes every
         source byte once), with the bandwidth that makes.

Warm-up rounds, then --steps event-timed repeats; median, min, max and interquartile range.  A
step whose table passes the library's 64 MiB limit is reported as refused.  Prints the lines and,
with --out, writes them to a file.

    python tools/gain_bench.py --steps 20 --out profiles/gain_bench.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ms):
    ms = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"ms_median": round(float(med), 4), "ms_min": round(float(ms.min()), 4),
            "ms_max": round(float(ms.max()), 4), "ms_iqr": round(float(q3 - q1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid-steps", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from multicamera_stitching_amd import _capi, rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc

    n, w, h, C, F = 4, args.width, args.height, 3, args.frames
    st, images, _ = rig.calibrated_stitcher(n, w, h, C, seed=0)
    cams = [images[label] for label in st.img_labels]
    plan = _capi.Plan([_stage_desc(sb) for sb in st.stitchers], w, h, C, _capi.MCS_INTER_LINEAR)
    dev = torch.device("cuda", 0)
    d_cams = []
    for c in cams:
        base = torch.from_numpy(c).to(dev)
        d_cams.append(torch.stack([torch.roll(base, shifts=f % h, dims=0)
                                   for f in range(F)]).contiguous())
    ptrs = [t.data_ptr() for t in d_cams]
    strides = [t[0].numel() for t in d_cams]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    lines = [{"tool": "gain_bench", "rig": "%d x %dx%dx%d" % (n, w, h, C), "frames": F,
              "mosaic": [plan.out_w, plan.out_h], "steps": args.steps, "warmup": args.warmup,
              "build_id": _capi.build_id(), "device": torch.cuda.get_device_name(0)}]

    for k in args.grid_steps:
        def call():
            t0 = time.perf_counter()
            N, _ = plan.overlap_stats(ptrs, strides, F, k, stream.cuda_stream)
            return (time.perf_counter() - t0) * 1e3, N
        try:
            first_ms, N = call()        # builds the table
        except _capi.McsError as e:
            lines.append({"step_log2": k, "refused": str(e)})
            continue
        for _ in range(args.warmup):
            call()
        ev, wall = [], []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            wall.append(call()[0])
            b.record(stream)
            ev.append((a, b))
        torch.cuda.synchronize()
        steady = float(np.median(wall))
        pairs = int(np.triu(N, 1).sum())
        own = int(np.trace(N))
        lines.append({"step_log2": k, "pair_entries": pairs, "camera_entries": own,
                      "table_bytes": 16 * pairs + 8 * own,
                      "prep_ms_once": round(first_ms - steady, 3),
                      "stats_call_events": spread([a.elapsed_time(b) for a, b in ev]),
                      "stats_call_wall": spread(wall),
                      "samples_per_call": (2 * pairs + own) * F})

    def apply():
        for t in d_cams:
            _capi.gain_apply_device(t.data_ptr(), t.data_ptr(), t[0].numel(), 300, F, 0, 0, 0,
                                    stream.cuda_stream)
    for _ in range(args.warmup):
        apply()
    torch.cuda.synchronize()
    ev = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        apply()
        b.record(stream)
        ev.append((a, b))
    torch.cuda.synchronize()
    s = spread([a.elapsed_time(b) for a, b in ev])
    nbytes = sum(t.numel() for t in d_cams)
    lines.append({"apply_all_cameras_in_place": s, "source_bytes": nbytes,
                  "read_plus_write_tb_per_s": round(2 * nbytes / (s["ms_median"] * 1e-3) / 1e12, 3)})

    text = "\n".join(json.dumps(line) for line in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
