"""The table-free overlap statistics and the rig job's exposure step as a stand-alone program
(tests/native/direct_gain_check.cpp, g++, a stub HIP runtime that records every launch, memset,
copy and synchronise in order): mcs_plan_overlap_stats_direct is memset + one launch + copy +
synchronise and leaves the plan's table alone, the _async form enqueues only; the grid keeps a
block's 32-bit partials from wrapping (16 cameras, step 0, a 65535-wide mosaic); a rig job with
exposure runs two statistics launches, one synchronise, then two _g stitch launches per batch of
two captures, and exactly the parent's launches with exposure off."""
import os
import subprocess

from multicamera_stitching_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicamera_stitching_amd", "csrc")
# every host source but the two the program stubs (the runtime binding, the module loader)
SOURCES = [s for s in build.HOST_SRC if s not in ("hip_rt.cpp", "mcs_runtime.cpp")]


def test_direct_gain_launch_path(tmp_path):
    exe = str(tmp_path / "direct_gain_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           '-DMCS_BUILD_ID="check"',
                           "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", "direct_gain_check.cpp"),
                           *[os.path.join(CSRC, s) for s in SOURCES],
                           "-o", exe, "-ldl", "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
