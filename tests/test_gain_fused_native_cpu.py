"""The fused-gain launch path as a stand-alone program (tests/native/gain_fused_check.cpp, g++, a
stub HIP runtime that records every launch): the gained launch takes the _g twin of every kernel
that reads source bytes, the q in the kernel arguments is the plan's as of the launch, identity
gains are inactive, and a sweep plan is refused before anything is launched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicamera_stitching_amd", "csrc")


def test_gain_fused_launch_path(tmp_path):
    exe = str(tmp_path / "gain_fused_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", "gain_fused_check.cpp"),
                           *[os.path.join(CSRC, s) for s in
                             ("mcs_gain.cpp", "mcs_prepare.cpp", "mcs_sweep_host.cpp",
                              "mcs_launch.cpp")],
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
