"""The inverse lens map as a stand-alone host program (tests/native/lens_invert_check.cpp, g++,
the library's own -ffp-contract=off): lens_invert over the frames of the lens tests' cameras,
every valid result taken back by lens_apply to within 2^-20 px, no invalid position where every
pixel has a preimage, NOPRE's corners invalid.  Built plain and with -fsanitize=address,undefined
(a program with its own main; nothing is preloaded); each build runs once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicamera_stitching_amd", "csrc")
NAMES = ("case0", "case1", "case2", "case3", "case4", "fold", "nopre")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "sanitized"])
def test_lens_invert_round_trips(tmp_path, flags):
    exe = str(tmp_path / "lens_invert_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off",
                           "-fno-fast-math", *flags, "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", "lens_invert_check.cpp"),
                           os.path.join(CSRC, "mcs_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    # (a sanitizer's report goes to stderr and ends the run with a non-zero status)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines and lines[-1] == "ok", out.stdout[-4000:]
    # no empty loop: every lens was walked and had valid positions
    assert [ln.split(":")[0] for ln in lines[:-1]] == list(NAMES), out.stdout
