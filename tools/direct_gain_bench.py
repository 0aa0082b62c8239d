"""What the overlap statistics of ONE capture with its own geometry cost on the C3 rig (4 x
1920x1080x3 from rig.calibrated_stitcher, frames resident on the device) -- a fresh plan per call,
as config 3 builds one per capture:

  (a) direct k   Plan + mcs_plan_overlap_stats_direct (one mcs_direct_overlap_* launch, no table)
                 + destroy, at step_log2 k = 2, 1 and 0
  (b) table k    Plan + mcs_plan_overlap_stats (table build: two mcs_overlap_prep_* launches, a
                 count read back, the host's prefix sum, a hipMalloc; then mcs_overlap_sum_*)
                 + destroy, at k = 2 and 1: the only route to a capture's statistics before (a)
  (c) kept k     mcs_plan_overlap_stats on a plan that is kept (its table stands): the steady
                 state of a fixed rig, for context
  (d) async k    Plan + mcs_plan_overlap_stats_direct_async into a caller's buffer + destroy, HIP
                 events around the call alone: the launch's device time (memset + kernel)

Every call runs on one stream of the caller's (a call without one would create the plan's own
stream, per fresh plan).  Every variant is timed with a host clock from before the plan is created
to after the call has returned (the calls synchronise; (d): to after a device synchronise);
--warmup rounds, then --steps repeats with the variants alternated inside each round; median
(min-max) in ms.  The table path refuses k = 0 on this rig only when the table passes 64 MiB; the
line says which.  Prints the lines and, with --out, writes them to a file.

    python tools/direct_gain_bench.py --out profiles/direct_gain_bench.txt
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
    tstream = torch.cuda.Stream()
    stream = tstream.cuda_stream
    stats = torch.zeros(2 * n * n, dtype=torch.int64, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kept = {k: _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR) for k in (2, 1)}
    ow, oh = kept[2].out_w, kept[2].out_h
    results = {}

    def fresh(k, direct):
        def run():
            t0 = time.perf_counter()
            plan = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
            fn = plan.overlap_stats_direct if direct else plan.overlap_stats
            res = fn(ptrs, strides, 1, k, stream)
            plan.close()
            t1 = time.perf_counter()
            results[(k, direct)] = res
            return (t1 - t0) * 1e3, None
        return run

    def steady(k):
        def run():
            t0 = time.perf_counter()
            kept[k].overlap_stats(ptrs, strides, 1, k, stream)
            return (time.perf_counter() - t0) * 1e3, None
        return run

    def enqueue(k):
        def run():
            t0 = time.perf_counter()
            plan = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
            ev0.record(tstream)
            plan.overlap_stats_direct_async(ptrs, strides, 1, k, stats.data_ptr(), stream)
            ev1.record(tstream)
            plan.close()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, ev0.elapsed_time(ev1)
        return run

    # whether the table path takes k = 0 here (a table over 64 MiB is refused)
    table0 = None
    probe = _capi.Plan(descs, w, h, C, _capi.MCS_INTER_LINEAR)
    try:
        probe.overlap_stats(ptrs, strides, 1, 0, stream)
        table0 = "accepted"
    except _capi.McsError as e:
        table0 = "refused (%s)" % str(e).splitlines()[0][:120]
    probe.close()

    variants = [("a direct k=2", fresh(2, True)), ("a direct k=1", fresh(1, True)),
                ("a direct k=0", fresh(0, True)),
                ("b table k=2 (fresh plan: table build + sums)", fresh(2, False)),
                ("b table k=1 (fresh plan: table build + sums)", fresh(1, False)),
                ("c kept plan k=2 (table stands: sums only)", steady(2)),
                ("c kept plan k=1 (table stands: sums only)", steady(1)),
                ("d direct async k=2 (enqueue; device: memset + kernel)", enqueue(2)),
                ("d direct async k=1 (enqueue; device: memset + kernel)", enqueue(1)),
                ("d direct async k=0 (enqueue; device: memset + kernel)", enqueue(0))]
    host = {name: [] for name, _ in variants}
    devt = {name: [] for name, _ in variants}
    for step in range(args.warmup + args.steps):
        for name, fn in variants:
            th, td = fn()
            if step >= args.warmup:
                host[name].append(th)
                if td is not None:
                    devt[name].append(td)
    equal = all(np.array_equal(results[(k, True)][0], results[(k, False)][0]) and
                np.array_equal(results[(k, True)][1], results[(k, False)][1]) for k in (2, 1))
    lines = ["direct gain bench: %d x %dx%dx%d, mosaic %dx%d, one capture per call, a fresh plan "
             "per call in (a), (b), (d); %d warm-up rounds, %d repeats, variants alternated; ms, "
             "median (min-max); build %s" % (n, w, h, C, ow, oh, args.warmup, args.steps,
                                             _capi.build_id())]
    for name, _ in variants:
        lines.append("%-56s host %s%s" % (name, spread(host[name]),
                                          "   device %s" % spread(devt[name]) if devt[name]
                                          else ""))
    lines.append("direct and table statistics equal at k = 2 and 1: %s" % equal)
    lines.append("table path at k = 0 on this rig: %s" % table0)
    ok = equal
    for k in (2, 1):
        a = float(np.median(host["a direct k=%d" % k]))
        b = float(np.min(host["b table k=%d (fresh plan: table build + sums)" % k]))
        lines.append("bar k=%d (a median below b minimum): %.4f < %.4f: %s" % (
            k, a, b, "holds" if a < b else "MISSED"))
        ok = ok and a < b
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for p in kept.values():
        p.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
