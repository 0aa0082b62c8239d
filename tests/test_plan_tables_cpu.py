"""The plan's prepared tables on the host (tests/native/tables_check.cpp, g++, a stub HIP runtime):
what mcs_plan::Tables allocates is freed exactly once by release_tables -- after a complete
prepare, after one that failed at any allocation, after an early drop -- aliases are never freed,
a fresh plan allocates nothing, and a failed prepare() leaves the plan as it was."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicamera_stitching_amd", "csrc")


def test_tables_ownership(tmp_path):
    exe = str(tmp_path / "tables_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", "tables_check.cpp"),
                           *[os.path.join(CSRC, s) for s in
                             ("mcs_prepare.cpp", "mcs_sweep_host.cpp", "mcs_launch.cpp")],
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
