"""The smallest camera frame (include/mcs.h "Smallest frame"): every plan kind refuses a frame
under 8 bytes at creation with MCS_E_UNSUPPORTED -- the kernels read 8-byte windows that end inside
the frame -- and accepts one of exactly 8.  Plan creation only: no HIP call, no GPU."""
import numpy as np
import pytest

from multicamera_stitching_amd import _capi

# (w, h, channels) of 7 and of 8 bytes
SEVEN = [(7, 1, 1), (1, 7, 1), (2, 2, 1), (1, 1, 4), (1, 2, 3), (1, 3, 2), (2, 1, 3)]
EIGHT = [(8, 1, 1), (1, 8, 1), (2, 4, 1), (1, 2, 4), (2, 1, 4), (4, 1, 2), (1, 4, 2)]
K = [[300.0, 0, 0.5], [0, 300.0, 0.5], [0, 0, 1]]


def _warp(w, h, c):
    return _capi.Plan.warp(np.eye(3), w, h, 16, 16, c)


def _undistort(w, h, c):
    return _capi.Plan.undistort(K, [-0.1, 0.01, 0.0, 0.0], w, h, c)


def _cylindrical(w, h, c):
    big = dict(R=np.eye(3), f=40.0, cx=20.0, cy=15.0, w=40, h=30)
    small = dict(R=np.eye(3), f=40.0, cx=0.5, cy=0.5, w=w, h=h)
    return _capi.Plan.cylindrical([big, small], 64, 32, 40.0, 32.0, 16.0, c)


MAKERS = [_warp, _undistort, _cylindrical]


@pytest.mark.parametrize("make", MAKERS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("w, h, c", SEVEN)
def test_frames_under_8_bytes_are_refused(make, w, h, c):
    with pytest.raises(_capi.McsError) as e:
        make(w, h, c)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED
    assert "bytes (< 8)" in str(e.value)


@pytest.mark.parametrize("make", MAKERS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("w, h, c", EIGHT)
def test_frames_of_8_bytes_are_accepted(make, w, h, c):
    plan = make(w, h, c)
    assert plan.channels == c and plan.cam_shapes[-1] == (h, w)
    plan.close()


def test_chain_plans_refuse_them_too():
    """(mcs_plan_create has had the check all along; the other plan kinds now word it alike)"""
    d = _capi.StageDesc()
    d.H[:] = [1, 0, 1, 0, 1, 0, 0, 0, 1]
    d.calibrated = 1
    d.canvas_w, d.canvas_h = 3, 2
    d.b_x, d.b_y, d.b_w, d.b_h = 0, 0, 2, 2
    d.a_w, d.a_h = 2, 2
    with pytest.raises(_capi.McsError) as e:
        _capi.Plan([d], 2, 2, 1)
    assert e.value.code == _capi.MCS_E_UNSUPPORTED and "bytes (< 8)" in str(e.value)
