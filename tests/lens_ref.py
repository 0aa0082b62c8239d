"""numpy specification of lensed plans (mcs_plan_set_lens): the per-camera lens composed into
every stage map, and the paste / SEAM / FEATHER mosaics that follow from the raw-frame positions.

float64 numpy only, one ufunc per operation (so no fused multiply-add), in the operation order of
csrc/mcs_lens_core.h, csrc/mcs_dev.h (map_exact, stage_map) and oracle/orc_blend.c:14-22.  The
oracle package cannot express a lens, so this module is the reference of the lens tests.

Positions are per camera slot (chain plans: slot 0 = camera 0, slot j + 1 = stage j; cylinder
plans: slot s = camera s) and per mosaic pixel, in 1/32 px of the camera's RAW frame
(x32 = sat_i16(X >> 5) * 32 + (X & 31); nearest: sat_i16(X) * 32).
"""
import math

import numpy as np

INTER_NEAREST, INTER_LINEAR = 0, 1
NONE = 255


def _coeffs(dist):
    k = np.zeros(12)
    d = np.zeros(0) if dist is None else np.asarray(dist, np.float64).reshape(-1)
    assert d.size in (0, 4, 5, 8, 12, 14) and not np.any(d[12:])
    k[:min(d.size, 12)] = d[:12]
    return [float(v) for v in k]


def r2max(dist):
    """Valid radius squared: the scan of mcs_lens_core.h lens_r2max (Python floats are IEEE
    doubles, one rounding per operation)."""
    k1, k2, _, _, k3, k4, k5, k6 = _coeffs(dist)[:8]
    f_prev = 0.0
    for i in range(1, 2049):
        r = i / 256.0
        r2 = r * r
        den = 1 + ((k6 * r2 + k5) * r2 + k4) * r2
        num = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        f = r * (num / den) if den != 0 else float("nan")
        if not (den > 0) or not (f > f_prev):
            return ((i - 1) / 256.0) ** 2
        f_prev = f
    return float("inf")


def _lens_raw(K, dist, u, v):
    """The lens polynomial: (xr, yr, r2) without the valid-radius rule."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coeffs(dist)
    u = np.asarray(u, np.float64)
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        x = (u - cx) / fx
        y = (v - cy) / fy
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
        xr = fx * xd + cx
        yr = fy * yd + cy
    return xr, yr, r2


def lens_apply(K, dist, u, v, use_r2max=True):
    """(u, v) of the undistorted image -> (xr, yr) of the raw frame; NaN where !(r2 <= r2max)."""
    xr, yr, r2 = _lens_raw(K, dist, u, v)
    if use_r2max:
        with np.errstate(all="ignore"):
            out = ~(r2 <= r2max(dist))
        xr = np.where(out, np.nan, xr)
        yr = np.where(out, np.nan, yr)
    return xr, yr


def _round_clamped(v):
    """cv_round_clamped: clamp to the int32 range (a NaN takes the upper bound, as the device's
    compare-and-select does), round half to even."""
    v = np.where(np.isnan(v), 2147483647.0, v)
    return np.rint(np.clip(v, -2147483648.0, 2147483647.0)).astype(np.int64)


def _sat16(v):
    return np.clip(v, -32768, 32767)


def _far(interp):
    return -(1 << 25) if interp == INTER_LINEAR else -(1 << 20)


def _fixed(X, Y, interp):
    """map value (X, Y) -> (x32, y32)."""
    if interp == INTER_NEAREST:
        return _sat16(X) * 32, _sat16(Y) * 32
    return _sat16(X >> 5) * 32 + (X & 31), _sat16(Y >> 5) * 32 + (Y & 31)


def _through_lens(lens, u, v, interp, use_r2max):
    """Undistorted position (doubles) -> map value of the raw frame."""
    k = 32.0 if interp == INTER_LINEAR else 1.0
    xr, yr, r2 = _lens_raw(lens[0], lens[1], u, v)
    with np.errstate(all="ignore"):
        out = ~(r2 <= (r2max(lens[1]) if use_r2max else np.inf))
        X = np.where(out, _far(interp), _round_clamped(xr * k))
        Y = np.where(out, _far(interp), _round_clamped(yr * k))
    return X, Y


def chain_positions(flat, interp=INTER_LINEAR, lenses=None, use_r2max=True, single=False):
    """Per slot (x32, y32) over the mosaic of a chain / warp plan's describe() dict.
    lenses: {camera index: (K, dist)}.  Returns (positions, slot cameras, rects).  single: a
    Plan.warp plan, which has no integer-placed camera 0 (slot 0's camera is None)."""
    lenses = lenses or {}
    n = int(flat["n_stages"])
    ow, oh = int(flat["out_w"]), int(flat["out_h"])
    y, x = np.mgrid[0:oh, 0:ow].astype(np.int64)
    pos, cams = [], []
    # slot 0: camera 0 at its integer offset
    X0, Y0 = x + int(flat["off_x"][n]), y + int(flat["off_y"][n])
    if 0 in lenses and not single:
        pos.append(_fixed(*_through_lens(lenses[0], X0.astype(np.float64),
                                         Y0.astype(np.float64), interp, use_r2max), interp))
    else:
        pos.append((X0 * 32, Y0 * 32))
    cams.append(None if single else 0)
    k = 32.0 if interp == INTER_LINEAR else 1.0
    for j in range(n):
        m = [float(v) for v in flat["minv"][j]]
        bw0 = int(flat["bw0"][j])
        cam = int(flat["cam"][j])
        X, Y = x + int(flat["off_x"][j]), y + int(flat["off_y"][j])
        if bw0 & (bw0 - 1) == 0:      # map_exact: a shift for power-of-two blocks,
            xb = (X // bw0) * bw0
        else:                         # else C's truncating division
            xb = np.where(X >= 0, X // bw0, -((-X) // bw0)) * bw0
        dxb, dy, dx1 = xb.astype(np.float64), Y.astype(np.float64), (X - xb).astype(np.float64)
        Xa = m[0] * dxb + m[1] * dy + m[2]
        Ya = m[3] * dxb + m[4] * dy + m[5]
        Wa = m[6] * dxb + m[7] * dy + m[8]
        W = Wa + m[6] * dx1
        with np.errstate(all="ignore"):
            if cam in lenses:
                Wi = np.where(W != 0.0, 1.0 / W, 0.0)
                u = (Xa + m[0] * dx1) * Wi
                v = (Ya + m[3] * dx1) * Wi
                Xi, Yi = _through_lens(lenses[cam], u, v, interp, use_r2max)
            else:
                Wk = np.where(W != 0.0, k / W, 0.0)
                Xi = _round_clamped((Xa + m[0] * dx1) * Wk)
                Yi = _round_clamped((Ya + m[3] * dx1) * Wk)
        pos.append(_fixed(Xi, Yi, interp))
        cams.append(cam)
    return pos, cams, [list(r) for r in flat["rect"]]


def cyl_positions(rig, out_w, out_h, f_cyl, u0, v0, interp=INTER_LINEAR, lenses=None,
                  use_r2max=True):
    """Per camera (x32, y32) over the panorama of a cylindrical plan (libm sin / cos per column,
    as the host table)."""
    lenses = lenses or {}
    sn = np.array([math.sin((u - u0) / f_cyl) for u in range(out_w)])[None, :]
    cs = np.array([math.cos((u - u0) / f_cyl) for u in range(out_w)])[None, :]
    hv = np.array([(v - v0) / f_cyl for v in range(out_h)])[:, None]
    k = 32.0 if interp == INTER_LINEAR else 1.0
    pos = []
    for c, cam in enumerate(rig):
        R = [float(v) for v in np.asarray(cam["R"], np.float64).reshape(9)]
        f, cx, cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
        dx = (R[0] * sn + R[1] * hv) + R[2] * cs
        dy = (R[3] * sn + R[4] * hv) + R[5] * cs
        dz = (R[6] * sn + R[7] * hv) + R[8] * cs
        behind = ~(dz > 0.0)
        with np.errstate(all="ignore"):
            sx = (f * dx) / dz + cx
            sy = (f * dy) / dz + cy
            if c in lenses:
                Xi, Yi = _through_lens(lenses[c], np.where(behind, 0.0, sx),
                                       np.where(behind, 0.0, sy), interp, use_r2max)
            else:
                Xi = _round_clamped(np.where(behind, 0.0, sx * k))
                Yi = _round_clamped(np.where(behind, 0.0, sy * k))
        Xi = np.where(behind, _far(interp), Xi)
        Yi = np.where(behind, _far(interp), Yi)
        pos.append(_fixed(Xi, Yi, interp))
    return pos, list(range(len(rig)))


def _img3(img):
    img = np.asarray(img, np.uint8)
    return img if img.ndim == 3 else img[..., None]


def _weights(x32, y32):
    fx, fy = x32 & 31, y32 & 31
    return [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]


def sample_border0(img, x32, y32):
    """remapBilinear with BORDER_CONSTANT 0 at (x32, y32) (the paste rule's sample)."""
    img = _img3(img)
    h, w, _ = img.shape
    sx, sy = x32 >> 5, y32 >> 5
    acc = np.zeros(x32.shape + (img.shape[2],), np.int64)
    for wt, (dx, dy) in zip(_weights(x32, y32), ((0, 0), (1, 0), (0, 1), (1, 1))):
        xx, yy = sx + dx, sy + dy
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        v = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64)
        acc += np.where(ok[..., None], v, 0) * wt[..., None]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def sample_replicate(img, x32, y32):
    """I_s: the same sample with the taps clamped into the image (BORDER_REPLICATE)."""
    img = _img3(img)
    h, w, _ = img.shape
    sx, sy = x32 >> 5, y32 >> 5
    acc = np.zeros(x32.shape + (img.shape[2],), np.int64)
    for wt, (dx, dy) in zip(_weights(x32, y32), ((0, 0), (1, 0), (0, 1), (1, 1))):
        v = img[np.clip(sy + dy, 0, h - 1), np.clip(sx + dx, 0, w - 1)].astype(np.int64)
        acc += v * wt[..., None]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def distances(pos, slot_cams, sizes):
    """d_s per slot: distance to the raw frame's edge in 1/32 px, -1 where not covered.
    sizes[camera] = (w, h)."""
    out = []
    for (x32, y32), cam in zip(pos, slot_cams):
        if cam is None:
            out.append(np.full(x32.shape, -1, np.int64))
            continue
        w, h = sizes[cam]
        xm, ym = 32 * (w - 1) - x32, 32 * (h - 1) - y32
        d = np.minimum(np.minimum(x32, y32), np.minimum(xm, ym))
        out.append(np.where((x32 < 0) | (y32 < 0) | (xm < 0) | (ym < 0), -1, d))
    return out


def owner_map(dist, slot_cams):
    """Covering slot with the largest d, ties to the lower camera index; NONE where uncovered."""
    best = np.full(dist[0].shape, NONE, np.int64)
    bestd = np.full(dist[0].shape, -1, np.int64)
    bestcam = np.zeros(dist[0].shape, np.int64)
    for s, (d, cam) in enumerate(zip(dist, slot_cams)):
        if cam is None:
            continue
        take = (d >= 0) & ((d > bestd) | ((d == bestd) & (cam < bestcam)))
        best = np.where(take, s, best)
        bestd = np.where(take, d, bestd)
        bestcam = np.where(take, cam, bestcam)
    return best.astype(np.uint8)


def paste_owner(rects, shape):
    """owner() of mcs_dev.h as a slot: the outermost stage whose paste rect does not contain
    the pixel (slot j + 1), slot 0 when every rect contains it."""
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    sel = np.zeros(shape, np.int64)
    inside = np.ones(shape, bool)
    for s in range(len(rects) - 1, -1, -1):
        r = rects[s]
        c = (x >= r[0]) & (x < r[2]) & (y >= r[1]) & (y < r[3])
        sel = np.where(inside & ~c, s + 1, sel)
        inside &= c
    return sel


def _shape_like(out, cams):
    return out if np.asarray(cams[0]).ndim == 3 else out[..., 0]


def render_paste(pos, slot_cams, rects, cams):
    """Paste mosaic (MCS_BLEND_NONE): every pixel is its paste owner's border-0 sample."""
    shape = pos[0][0].shape
    sel = paste_owner(rects, shape)
    out = np.zeros(shape + (_img3(cams[0]).shape[2],), np.uint8)
    for s, ((x32, y32), cam) in enumerate(zip(pos, slot_cams)):
        if cam is None:
            continue
        out = np.where((sel == s)[..., None], sample_border0(cams[cam], x32, y32), out)
    return _shape_like(out, cams)


def render_blend(pos, slot_cams, cams, mode, want_owner=False):
    """mode "seam": the owner's I_s; "feather": (sum d_s I_s + D / 2) / D over the slots at
    positive distance, D == 0 -> the owner's sample; 0 where no slot covers the pixel."""
    sizes = {c: (_img3(im).shape[1], _img3(im).shape[0]) for c, im in enumerate(cams)}
    dist = distances(pos, slot_cams, sizes)
    own = owner_map(dist, slot_cams)
    cn = _img3(cams[0]).shape[2]
    seam = np.zeros(own.shape + (cn,), np.int64)
    num = np.zeros(own.shape + (cn,), np.int64)
    den = np.zeros(own.shape, np.int64)
    for s, ((x32, y32), cam) in enumerate(zip(pos, slot_cams)):
        if cam is None:
            continue
        I = sample_replicate(cams[cam], x32, y32).astype(np.int64)
        seam = np.where((own == s)[..., None], I, seam)
        dpos = np.where(dist[s] > 0, dist[s], 0)
        num += dpos[..., None] * I
        den += dpos
    if mode == "seam":
        out = seam
    else:
        assert mode == "feather"
        D = np.where(den == 0, 1, den)[..., None]
        out = np.where((den == 0)[..., None], seam, (num + D // 2) // D)
    out = np.where((own == NONE)[..., None], 0, out).astype(np.uint8)
    out = _shape_like(out, cams)
    return (out, own) if want_owner else out
