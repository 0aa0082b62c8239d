"""Call-lifetime device memory on the host, as two stand-alone programs on the stub HIP runtime
(tests/native/stub_hip.h, g++): tests/native/scratch_check.cpp checks the call-scoped owner
(csrc/mcs_scratch.h) -- freed once, keep(), a failing allocation at any position, one synchronise
before the first free unless the call synchronised itself, no call from an owner that never
allocated --, tests/native/host_calls_check.cpp drives the entry points that use it through the C
ABI: a clean run's log, then every runtime call of that run failing in turn, with nothing left
allocated, nothing freed twice and a clean retry each time.  Both are built plain and with
-fsanitize=address,undefined (programs with their own main; nothing is preloaded) and each build
runs once."""
import os
import re
import subprocess

import pytest

from multicamera_stitching_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicamera_stitching_amd", "csrc")
# every host source but the two the stub stands in for (the runtime binding, the module loader)
HOST = [s for s in build.HOST_SRC if s not in ("hip_rt.cpp", "mcs_runtime.cpp")]
PROGRAMS = {"scratch_check": [], "host_calls_check": HOST}
SCENARIOS = ("seams", "footprint", "graphcut", "overlap", "match", "orb", "rig", "stitch")


def run_program(tmp_path, name, flags):
    exe = str(tmp_path / name)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", *flags, "-D__HIP_PLATFORM_AMD__",
                           '-DMCS_BUILD_ID="check"',
                           "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", name + ".cpp"),
                           *[os.path.join(CSRC, s) for s in PROGRAMS[name]],
                           "-o", exe, "-ldl", "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    # (a sanitizer's report goes to stderr and ends the run with a non-zero status)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines and lines[-1] == "ok", out.stdout[-4000:]
    return lines


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "sanitized"])
def test_scratch_owner(tmp_path, flags):
    run_program(tmp_path, "scratch_check", flags)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "sanitized"])
def test_host_calls_under_failure(tmp_path, flags):
    lines = run_program(tmp_path, "host_calls_check", flags)
    ran = {}
    for line in lines:
        m = re.fullmatch(r"scenario (\w+): calls (\d+), failed (\d+), discarded (\d+)", line)
        if m:
            ran[m.group(1)] = tuple(int(v) for v in m.group(2, 3, 4))
    assert set(ran) == set(SCENARIOS), ran
    for name, (calls, failed, discarded) in ran.items():
        # no empty loop: every scenario made runtime calls and failed each of them in turn
        assert calls >= 1 and failed >= 1 and failed + discarded == calls, (name, ran[name])
