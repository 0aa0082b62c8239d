"""bench.py on the GPU at a small size: a plain run is lean (the headline line only) and
--dump-outputs writes what its last timed step computed, checked here against the CPU
restatement; --full brings back parity, the paste-only launch and roofline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "3",
         "--width", "320", "--height", "180"]


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_its_dump_equals_the_restatement(tmp_path):
    from multicamera_stitching_amd import _capi, rig
    from multicamera_stitching_amd.StitcherClass import _stage_desc
    from oracle import oracle
    res = _bench(SMALL + ["--dump-outputs", str(tmp_path)])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "MPix/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    out_h, out_w, C = res["config"]["mosaic"]
    # value = the mosaic pixels of one step over ms_per_step (both rounded in the line)
    want = 3 * out_h * out_w / 1e6 / (res["ms_per_step"] * 1e-3)
    assert res["ms_per_step"] > 0 and abs(res["value"] - want) <= 2e-3 * want
    for moved in ("also", "max_abs_diff", "checked_captures", "roofline", "cpu_baseline"):
        assert moved not in res, moved
    assert "paste_only_launch_ms" not in res["kernels"]
    assert sorted(res["outputs"]) == ["mosaic_row_sums.npy", "mosaics_sample.npy"]
    sample = np.load(tmp_path / "mosaics_sample.npy")
    rows = np.load(tmp_path / "mosaic_row_sums.npy")
    # (3 small mosaics: below bench.DUMP_SAMPLE elements, so the batch is written whole)
    assert sample.dtype == np.float32 and sample.shape == (3, out_h, out_w * C)
    assert rows.dtype == np.float64
    assert np.array_equal(rows, sample.astype(np.float64).sum(axis=2))
    # the same seeded rig, capture f = the frames rolled by f rows, through the CPU restatement
    st, images, _ = rig.calibrated_stitcher(4, 320, 180, 3, seed=0)
    cams = [images[label] for label in st.img_labels]
    plan = _capi.Plan([_stage_desc(sb) for sb in st.stitchers], 320, 180, 3,
                      _capi.MCS_INTER_LINEAR)
    flat = plan.describe()
    plan.close()
    for f in range(3):
        ref = oracle.blend_stitch(flat, [np.roll(c, f, axis=0) for c in cams],
                                  oracle.BLEND_MULTIBAND, _capi.MCS_INTER_LINEAR)
        assert ref.shape == (out_h, out_w, C)
        assert np.array_equal(sample[f].reshape(out_h, out_w, C), ref.astype(np.float32)), f


def test_full_run_reports_parity_and_roofline():
    res = _bench(SMALL + ["--full", "--no-also", "--no-cpu-baseline"])
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert res["max_abs_diff"] == 0
    assert res["checked_captures"]["per_rank"] == [0, 1, 2]
    assert res["kernels"]["paste_only_launch_ms"] > 0
    assert res["roofline"]["kernel_ms_per_launch"] == res["kernels"]["launch_ms"]
    assert res["cpu_baseline"] is None and "also" not in res
