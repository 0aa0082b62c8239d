"""numpy specification of the inverse lens map (csrc/mcs_lens_core.h lens_invert, the rig job's
lenses): a raw-frame position -> the position in the camera's undistorted image.

float64 numpy only, one ufunc per operation, in lens_invert's operation order: six Newton steps
on the lens polynomial (lens_ref._lens_raw) from the raw position itself, forward-difference
Jacobian of step 1 / 1024 px, Cramer's rule.  NaN where the result is not valid: not finite,
beyond the valid radius, or not taken back by lens_ref.lens_apply to within 2^-20 px.
"""
import numpy as np

import lens_ref

ITERS = 6
TOL = 2.0 ** -20

NOPRE = dict(K=[[200.0, 0, 159.5], [0, 200.0, 119.5], [0, 0, 1]], d=[-0.3, 0, 0, 0], w=320, h=240)


def lens_invert(K, dist, xr, yr):
    """(xr, yr) raw -> (u, v) undistorted, NaN, NaN where lens_invert returns false."""
    xr = np.asarray(xr, np.float64)
    yr = np.asarray(yr, np.float64)
    h, ih = 1.0 / 1024.0, 1024.0
    u, v = xr.copy(), yr.copy()
    with np.errstate(all="ignore"):
        for _ in range(ITERS):
            fx0, fy0, _ = lens_ref._lens_raw(K, dist, u, v)
            fx1, fy1, _ = lens_ref._lens_raw(K, dist, u + h, v)
            fx2, fy2, _ = lens_ref._lens_raw(K, dist, u, v + h)
            a = (fx1 - fx0) * ih
            b = (fx2 - fx0) * ih
            c = (fy1 - fy0) * ih
            d = (fy2 - fy0) * ih
            ex = fx0 - xr
            ey = fy0 - yr
            det = a * d - b * c
            u = u - (d * ex - b * ey) / det
            v = v - (a * ey - c * ex) / det
        bx, by = lens_ref.lens_apply(K, dist, u, v)
        dx = bx - xr
        dy = by - yr
        ok = np.isfinite(u) & np.isfinite(v) & ~np.isnan(bx)
        ok &= (dx <= TOL) & (dx >= -TOL) & (dy <= TOL) & (dy >= -TOL)
    return np.where(ok, u, np.nan), np.where(ok, v, np.nan)


def grid(case):
    """The integer pixels of the case's frame (a 3-px grid for frames larger than 640 x 480) as
    (n, 2) float64 x, y."""
    w, h = case["w"], case["h"]
    step = 3 if w * h > 640 * 480 else 1
    y, x = np.mgrid[0:h:step, 0:w:step].astype(np.float64)
    return np.stack([x.ravel(), y.ravel()], axis=1)


def _bilinear(img, u, v):
    """Plain float64 bilinear sample of img (h, w, C) at (u, v), 0 outside and where NaN."""
    h, w = img.shape[:2]
    ok = np.isfinite(u) & np.isfinite(v)
    u = np.where(ok, u, -10.0)
    v = np.where(ok, v, -10.0)
    x0 = np.floor(u).astype(np.int64)
    y0 = np.floor(v).astype(np.int64)
    ax = (u - x0)[..., None]
    ay = (v - y0)[..., None]
    acc = np.zeros(u.shape + (img.shape[2],), np.float64)
    for dx, dy, wt in ((0, 0, (1 - ax) * (1 - ay)), (1, 0, ax * (1 - ay)),
                       (0, 1, (1 - ax) * ay), (1, 1, ax * ay)):
        xx, yy = x0 + dx, y0 + dy
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        val = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.float64)
        acc += np.where(inside[..., None], val, 0.0) * wt
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def raw_frame(clean, K, dist):
    """The raw frame a camera with lens (K, dist) delivers of the undistorted view `clean`:
    raw[p] = bilinear(clean, lens_invert(p)), zero where the inverse is NaN.  A barrel lens sees
    past the clean view's edge; a position there takes the view's nearest edge pixel (a real
    frame has scene up to its border: a black band with a hard curved edge would be a row of
    FAST corners no camera delivers, and they take their share of the nfeatures quota)."""
    h, w = clean.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = lens_invert(K, dist, x, y)
    return _bilinear(clean, np.clip(u, 0, w - 1), np.clip(v, 0, h - 1))   # (NaN stays NaN)
