"""numpy specification of the fisheye lens model (csrc/mcs_lens_core.h, model 1:
cv2.fisheye.initUndistortRectifyMap with R = I and P = K): the arctangent, the forward map, the
valid angle, the inverse, the per-slot positions of chain and cylinder plans whose cameras each
have their own model, and raw fisheye frames rendered from clean ones.

float64 numpy only, one ufunc per operation (so no fused multiply-add), in the header's operation
order.  The samplers and renderers are tests/lens_ref.py's: positions in, mosaics out.

A lens is (K, dist) -- the polynomial model of lens_ref -- or (K, dist, "fisheye").
"""
import math

import numpy as np

import lens_ref
from lens_inv_ref import _bilinear, lens_invert as _poly_invert
from lens_ref import (INTER_LINEAR, INTER_NEAREST, distances, owner_map,  # noqa: F401
                      render_blend, render_paste, sample_border0, sample_replicate)

ITERS = 10
TOL = 2.0 ** -20

# lens_atan: the reduction breakpoints, per interval the reference angle as hi + lo, and the
# coefficients of the odd polynomial (even-indexed and odd-indexed halves).  The constants are
# those of fdlibm's s_atan.c, as in csrc/mcs_lens_core.h, whose notice reads:
#   ====================================================
#   Copyright (C) 1993 by Sun Microsystems, Inc. All rights reserved.
#
#   Developed at SunPro, a Sun Microsystems, Inc. business.
#   Permission to use, copy, modify, and distribute this
#   software is freely granted, provided that this notice
#   is preserved.
#   ====================================================
BREAKS = (0.4375, 0.6875, 1.1875, 2.4375)
_HI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
       1.57079632679489655800e+00)
_LO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
       6.12323399573676603587e-17)
_A = (3.33333333333329318027e-01, 1.42857142725034663711e-01, 9.09088713343650656196e-02,
      6.66107313738753120669e-02, 4.97687799461593236017e-02, 1.62858201153657823623e-02)
_B = (-1.99999999998764832476e-01, -1.11111104054623557880e-01, -7.69187620504482999495e-02,
      -5.83357013379057348645e-02, -3.65315727442169155270e-02)


def lens_atan(r):
    """atan(r), r >= 0, with + - * / only (lens_atan of the header)."""
    r = np.asarray(r, np.float64)
    with np.errstate(all="ignore"):
        c0, c1, c2, c3 = (r < b for b in BREAKS)

        def pick(v0, v1, v2, v3, v4):
            return np.where(c0, v0, np.where(c1, v1, np.where(c2, v2, np.where(c3, v3, v4))))

        num = pick(r, 2.0 * r - 1.0, r - 1.0, r - 1.5, -1.0)
        den = pick(1.0, 2.0 + r, r + 1.0, 1.0 + 1.5 * r, r)
        hi = pick(0.0, *_HI)
        lo = pick(0.0, *_LO)
        x = num / den
        z = x * x
        w = z * z
        s1 = z * (_A[0] + w * (_A[1] + w * (_A[2] + w * (_A[3] + w * (_A[4] + w * _A[5])))))
        s2 = w * (_B[0] + w * (_B[1] + w * (_B[2] + w * (_B[3] + w * _B[4]))))
        return hi - ((x * (s1 + s2) - lo) - x)


def _coeffs(dist):
    d = np.zeros(0) if dist is None else np.asarray(dist, np.float64).reshape(-1)
    assert d.size in (0, 4)
    return [float(v) for v in d] if d.size else [0.0] * 4


def _td(k, t):
    k1, k2, k3, k4 = k
    t2 = t * t
    t4 = t2 * t2
    t6 = t4 * t2
    t8 = t4 * t4
    return t * (1 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8)


def tmax(dist):
    """Valid angle: the scan of lens_tmax (Python floats are IEEE doubles)."""
    k = _coeffs(dist)
    f_prev = 0.0
    for i in range(1, 1609):
        f = _td(k, i / 1024.0)
        if not (f > 0) or not (f > f_prev):
            return (i - 1) / 1024.0
        f_prev = f
    return float("inf")


def _kparts(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _fish_raw(K, dist, u, v):
    """The fisheye map: (xr, yr, t, r) without the valid-angle rule."""
    fx, fy, cx, cy = _kparts(K)
    k = _coeffs(dist)
    u = np.asarray(u, np.float64)
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        x = (u - cx) / fx
        y = (v - cy) / fy
        r = np.sqrt(x * x + y * y)
        t = lens_atan(r)
        td = _td(k, t)
        s = np.where(r == 0.0, 1.0, td / r)
        xr = fx * (x * s) + cx
        yr = fy * (y * s) + cy
    return xr, yr, t, r


def _outside(dist, t, r, use_tmax):
    with np.errstate(all="ignore"):
        return ~(t <= (tmax(dist) if use_tmax else np.inf)) | ~np.isfinite(r)


def lens_apply(K, dist, u, v, use_tmax=True):
    """(u, v) undistorted -> (xr, yr) raw; NaN where !(t <= tmax) or r is not finite."""
    xr, yr, t, r = _fish_raw(K, dist, u, v)
    out = _outside(dist, t, r, use_tmax)
    return np.where(out, np.nan, xr), np.where(out, np.nan, yr)


def lens_invert(K, dist, xr, yr):
    """(xr, yr) raw -> (u, v) undistorted; NaN, NaN where lens_invert returns false."""
    fx, fy, cx, cy = _kparts(K)
    k1, k2, k3, k4 = _coeffs(dist)
    xr = np.asarray(xr, np.float64)
    yr = np.asarray(yr, np.float64)
    with np.errstate(all="ignore"):
        xd = (xr - cx) / fx
        yd = (yr - cy) / fy
        td = np.sqrt(xd * xd + yd * yd)
        r = td
        for _ in range(ITERS):
            t = lens_atan(r)
            t2 = t * t
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            g = t * (1 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8) - td
            dg = (1 + 3 * k1 * t2 + 5 * k2 * t4 + 7 * k3 * t6 + 9 * k4 * t8) / (1 + r * r)
            r = r - g / dg
        s = np.where(td == 0.0, 1.0, r / td)
        u = fx * (xd * s) + cx
        v = fy * (yd * s) + cy
        bx, by = lens_apply(K, dist, u, v)
        dx = bx - xr
        dy = by - yr
        ok = np.isfinite(u) & np.isfinite(v) & ~np.isnan(bx)
        ok &= (dx <= TOL) & (dx >= -TOL) & (dy <= TOL) & (dy >= -TOL)
    return np.where(ok, u, np.nan), np.where(ok, v, np.nan)


def is_fisheye(lens):
    return len(lens) > 2 and lens[2] in ("fisheye", 1)


def invert_any(lens, xr, yr):
    """The inverse of either model."""
    if is_fisheye(lens):
        return lens_invert(lens[0], lens[1], xr, yr)
    return _poly_invert(lens[0], lens[1], xr, yr)


def _through_lens(lens, u, v, interp, use_limit):
    """Undistorted position (doubles) -> map value of the raw frame, either model."""
    if not is_fisheye(lens):
        return lens_ref._through_lens(lens[:2], u, v, interp, use_limit)
    k = 32.0 if interp == INTER_LINEAR else 1.0
    xr, yr, t, r = _fish_raw(lens[0], lens[1], u, v)
    out = _outside(lens[1], t, r, use_limit)
    with np.errstate(all="ignore"):
        X = np.where(out, lens_ref._far(interp), lens_ref._round_clamped(xr * k))
        Y = np.where(out, lens_ref._far(interp), lens_ref._round_clamped(yr * k))
    return X, Y


def chain_positions(flat, interp=INTER_LINEAR, lenses=None, use_limit=True):
    """lens_ref.chain_positions with a model per camera: the positions of lens-free and
    polynomial cameras are lens_ref's own, a fisheye camera's undistorted position (the
    arithmetic of map_exact_uv) goes through the fisheye map."""
    lenses = lenses or {}
    poly = {c: l[:2] for c, l in lenses.items() if not is_fisheye(l)}
    pos, cams, rects = lens_ref.chain_positions(flat, interp, poly, use_limit)
    n = int(flat["n_stages"])
    ow, oh = int(flat["out_w"]), int(flat["out_h"])
    y, x = np.mgrid[0:oh, 0:ow].astype(np.int64)
    for s, cam in enumerate(cams):
        if cam not in lenses or not is_fisheye(lenses[cam]):
            continue
        if s == 0:
            u = (x + int(flat["off_x"][n])).astype(np.float64)
            v = (y + int(flat["off_y"][n])).astype(np.float64)
        else:
            j = s - 1
            m = [float(a) for a in flat["minv"][j]]
            bw0 = int(flat["bw0"][j])
            X, Y = x + int(flat["off_x"][j]), y + int(flat["off_y"][j])
            if bw0 & (bw0 - 1) == 0:
                xb = (X // bw0) * bw0
            else:
                xb = np.where(X >= 0, X // bw0, -((-X) // bw0)) * bw0
            dxb, dy, dx1 = xb.astype(np.float64), Y.astype(np.float64), (X - xb).astype(np.float64)
            Xa = m[0] * dxb + m[1] * dy + m[2]
            Ya = m[3] * dxb + m[4] * dy + m[5]
            Wa = m[6] * dxb + m[7] * dy + m[8]
            W = Wa + m[6] * dx1
            with np.errstate(all="ignore"):
                Wi = np.where(W != 0.0, 1.0 / W, 0.0)
                u = (Xa + m[0] * dx1) * Wi
                v = (Ya + m[3] * dx1) * Wi
        pos[s] = lens_ref._fixed(*_through_lens(lenses[cam], u, v, interp, use_limit), interp)
    return pos, cams, rects


def cyl_positions(rig, out_w, out_h, f_cyl, u0, v0, interp=INTER_LINEAR, lenses=None,
                  use_limit=True):
    """lens_ref.cyl_positions with a model per camera."""
    lenses = lenses or {}
    poly = {c: l[:2] for c, l in lenses.items() if not is_fisheye(l)}
    pos, cams = lens_ref.cyl_positions(rig, out_w, out_h, f_cyl, u0, v0, interp, poly, use_limit)
    sn = np.array([math.sin((u - u0) / f_cyl) for u in range(out_w)])[None, :]
    cs = np.array([math.cos((u - u0) / f_cyl) for u in range(out_w)])[None, :]
    hv = np.array([(v - v0) / f_cyl for v in range(out_h)])[:, None]
    for c, cam in enumerate(rig):
        if c not in lenses or not is_fisheye(lenses[c]):
            continue
        R = [float(a) for a in np.asarray(cam["R"], np.float64).reshape(9)]
        f, cx, cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
        dx = (R[0] * sn + R[1] * hv) + R[2] * cs
        dy = (R[3] * sn + R[4] * hv) + R[5] * cs
        dz = (R[6] * sn + R[7] * hv) + R[8] * cs
        behind = ~(dz > 0.0)
        with np.errstate(all="ignore"):
            sx = (f * dx) / dz + cx
            sy = (f * dy) / dz + cy
        Xi, Yi = _through_lens(lenses[c], np.where(behind, 0.0, sx), np.where(behind, 0.0, sy),
                               interp, use_limit)
        Xi = np.where(behind, lens_ref._far(interp), Xi)
        Yi = np.where(behind, lens_ref._far(interp), Yi)
        pos[c] = lens_ref._fixed(Xi, Yi, interp)
    return pos, cams


def raw_frame(clean, K, dist):
    """The raw frame a fisheye camera (K, dist) delivers of the undistorted view `clean`:
    raw[p] = bilinear(clean, lens_invert(p)), zero where the inverse is NaN; a position past the
    clean view's edge takes the view's nearest edge pixel (as lens_inv_ref.raw_frame)."""
    h, w = clean.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = lens_invert(K, dist, x, y)
    img = clean if clean.ndim == 3 else clean[..., None]
    out = _bilinear(img, np.clip(u, 0, w - 1), np.clip(v, 0, h - 1))   # (NaN stays NaN)
    return out if clean.ndim == 3 else out[..., 0]
