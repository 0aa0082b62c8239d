"""ORB's level geometry as a stand-alone program (tests/native/orb_geom_check.cpp, g++, the host
sources, a stub runtime that is never called): orb_geom's quotas add up to n_bound <= nfeatures
over nfeatures 0..3000 x 1..12 levels x seven scale factors and are OpenCV's wherever OpenCV's
stay within nfeatures; pyramid_args declines exactly the pyramids with a 2x level step or with
regions too large for LDS, and what it accepts fits 64 KB with one block per tile of the last
level; a Hamming train set of 2^23 descriptors is refused on its arguments."""
import os
import subprocess

from multicamera_stitching_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicamera_stitching_amd", "csrc")
# every host source but the two the program stubs (the runtime binding, the module loader)
SOURCES = [s for s in build.HOST_SRC if s not in ("hip_rt.cpp", "mcs_runtime.cpp")]


def test_orb_geometry_host_code(tmp_path):
    exe = str(tmp_path / "orb_geom_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           '-DMCS_BUILD_ID="check"', "-ffp-contract=off",
                           "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", "orb_geom_check.cpp"),
                           *[os.path.join(CSRC, s) for s in SOURCES],
                           "-o", exe, "-ldl", "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
