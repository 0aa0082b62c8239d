"""The warp edge-case table on the CPU: oracle.warp_perspective equals the NumPy restatement
(tests/warp_edges.py) byte for byte, and every case shows its property on the reference alone --
so that a GPU comparison on the same table cannot pass on an all-black image."""
import numpy as np
import pytest

import warp_edges as we
from oracle import oracle


@pytest.mark.parametrize("interp", [oracle.INTER_LINEAR, oracle.INTER_NEAREST])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
@pytest.mark.parametrize("name", [c["name"] for c in we.CASES])
def test_oracle_equals_numpy_restatement(name, ch, interp):
    case = we.BY_NAME[name]
    (sw, sh), (dw, dh) = case["src"], case["dst"]
    src = we.texture(sh, sw, ch, seed=7)
    want = oracle.warp_perspective(src, case["M"], (dw, dh), interp)
    Minv = oracle.invert3x3(case["M"])
    got, X, Y, W = we.np_warp(src, Minv, dw, dh, interp, want_map=True)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert (got == want).all(), int(np.abs(got.astype(np.int16) - want.astype(np.int16)).max())
    we.check_property(case, src, got, X, Y, W, interp, Minv)


def test_exact_horizon_inverse():
    """The library's inverse of horizon_exact's M is exact, so W is exactly 0 on row 32."""
    inv = oracle.invert3x3(we.BY_NAME["horizon_exact"]["M"])
    assert (inv == np.array([[1, 0, 0], [0, 1, 0], [0, -1 / 32, 1]])).all()
