// mcs_lens_core.h -- the per-camera lens map, shared by the gfx950 kernels (mcs_dev.h) and the
// host (mcs_plan.cpp: mcs_lens_map_host, the valid-radius scan).
//
// A lens takes a position (u, v) of a camera's UNDISTORTED image to the position in its RAW
// frame: cv::initUndistortRectifyMap's model with R = I and newCameraMatrix = K (rational radial
// + tangential + thin-prism terms, tilt identity), evaluated per position instead of accumulated
// along a row.  IEEE double, every operation rounded once, in the order written below (both
// compilers build it with -ffp-contract=off); tests/lens_ref.py restates it in numpy.
//
// Valid radius: a polynomial with k1 < 0 folds back (far rays land inside the raw frame again),
// which would give a camera ghost coverage in its neighbours' part of the mosaic.  lens_r2max()
// scans r = i / 256, i = 1..2048, for the first radius at which the denominator is not positive
// or the distorted radius r * num / den stops growing; positions with !(r2 <= r2max) -- NaN
// included -- are outside the lens.
//
// Fisheye (model 1, cv2.fisheye.initUndistortRectifyMap with R = I and P = K): the equidistant
// model theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), theta the angle
// of the ray, lens_atan(r) of the normalised radius.  lens_atan is this file's own arctangent:
// + - * / on doubles in one fixed order, so that the host, the device and numpy give the same
// bits (libm's and the device library's atan differ).  The radius is a correctly rounded FP64
// square root on both sides.  Valid angle: lens_tmax() scans theta = i / 1024, i = 1..1608
// (below pi / 2), for the first angle at which theta_d is not positive or stops growing, and
// goes one step back; it is kept in the r2max slot, and positions with !(theta <= tmax) or a
// radius that is not finite are outside the lens.  tests/fisheye_ref.py restates it in numpy.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MCS_LENS_HD __host__ __device__ __forceinline__
#else
#define MCS_LENS_HD static inline
#endif

// MCS_LENS_MODELS 1: lens_apply, lens_poly and lens_invert read the row's model.  0: they are the
// polynomial model alone -- the device code objects a plan without a fisheye camera runs are
// built so (build.py), which keeps their registers where they were: with the branch,
// mcs_direct_* and mcs_prepare_* take 20 VGPRs more and go to scratch.  The host, the feature
// code object (mcs_rig_unlens) and the *_fish code objects read the model.
#ifndef MCS_LENS_MODELS
#define MCS_LENS_MODELS 1
#endif

namespace mcs {

// One row of the device lens table (KParams.lens_tab), kLensDoubles doubles per camera.
struct Lens {
    double fx, fy, cx, cy;
    double k[12];        // OpenCV order: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4; fisheye: k1 k2 k3 k4
    double r2max;        // lens_r2max(), fisheye: lens_tmax(); +inf: no limit
    double model;        // 0: the polynomial model, 1: fisheye (a zeroed row is polynomial)
};
constexpr int kLensDoubles = 18;
static_assert(sizeof(Lens) == kLensDoubles * sizeof(double), "Lens layout");

// Numerator and denominator of the radial factor at r2.
MCS_LENS_HD double lens_num(const Lens &L, double r2)
{
    return 1 + ((L.k[4] * r2 + L.k[1]) * r2 + L.k[0]) * r2;
}
MCS_LENS_HD double lens_den(const Lens &L, double r2)
{
    return 1 + ((L.k[7] * r2 + L.k[6]) * r2 + L.k[5]) * r2;
}

// atan(r) for r >= 0 (NaN for a NaN; pi / 2 for +inf).  Argument reduction at the fixed
// breakpoints 7/16, 11/16, 19/16 and 39/16 to |x| < 7/16 -- atan(r) = atan(c) + atan((r - c) /
// (1 + r c)) for c = 0.5, 1, 1.5, and pi / 2 - atan(1 / r) above the last --, the reference
// angle as a hi + lo pair, and an odd polynomial of degree 23 in x, split into its even and odd
// halves in x^2.  The scheme, the hi / lo constants and the coefficients are those of fdlibm's
// s_atan.c, whose notice reads:
//   ====================================================
//   Copyright (C) 1993 by Sun Microsystems, Inc. All rights reserved.
//
//   Developed at SunPro, a Sun Microsystems, Inc. business.
//   Permission to use, copy, modify, and distribute this
//   software is freely granted, provided that this notice
//   is preserved.
//   ====================================================
// One quotient serves the five intervals (r / 1 is r).  Measured against a 60-digit arctangent
// on r = i / 4096 (i = 0..32768), 2^k (k = -60..60) and the breakpoints' neighbours: at most
// 0.75 ulp; non-decreasing over all of them.
MCS_LENS_HD double lens_atan(double r)
{
    double num = r, den = 1.0, hi = 0.0, lo = 0.0;
    if (!(r < 0.4375)) {
        if (r < 0.6875) {
            num = 2.0 * r - 1.0;
            den = 2.0 + r;
            hi = 4.63647609000806093515e-01;
            lo = 2.26987774529616870924e-17;
        } else if (r < 1.1875) {
            num = r - 1.0;
            den = r + 1.0;
            hi = 7.85398163397448278999e-01;
            lo = 3.06161699786838301793e-17;
        } else if (r < 2.4375) {
            num = r - 1.5;
            den = 1.0 + 1.5 * r;
            hi = 9.82793723247329054082e-01;
            lo = 1.39033110312309984516e-17;
        } else {
            num = -1.0;
            den = r;
            hi = 1.57079632679489655800e+00;
            lo = 6.12323399573676603587e-17;
        }
    }
    const double x = num / den;
    const double z = x * x, w = z * z;
    const double s1 =
        z * (3.33333333333329318027e-01 +
             w * (1.42857142725034663711e-01 +
                  w * (9.09088713343650656196e-02 +
                       w * (6.66107313738753120669e-02 +
                            w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 =
        w * (-1.99999999998764832476e-01 +
             w * (-1.11111104054623557880e-01 +
                  w * (-7.69187620504482999495e-02 +
                       w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    return hi - ((x * (s1 + s2) - lo) - x);
}

// Fisheye: the distorted angle theta_d of the angle t.
MCS_LENS_HD double lens_fish_td(const Lens &L, double t)
{
    const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    return t * (1 + L.k[0] * t2 + L.k[1] * t4 + L.k[2] * t6 + L.k[3] * t8);
}

// Fisheye lens_apply (rule: the valid-angle rule applies) and lens_poly (rule == false).
MCS_LENS_HD bool lens_fish(const Lens &L, bool rule, double u, double v, double &xr, double &yr)
{
    const double x = (u - L.cx) / L.fx, y = (v - L.cy) / L.fy;
    const double r = __builtin_sqrt(x * x + y * y);
    const double t = lens_atan(r);
    if (rule && (!(t <= L.r2max) || !(r - r == 0.0))) return false;
    const double td = lens_fish_td(L, t);
    const double s = (r == 0.0) ? 1.0 : td / r;
    xr = L.fx * (x * s) + L.cx;
    yr = L.fy * (y * s) + L.cy;
    return true;
}

// (u, v) of the undistorted image -> (xr, yr) of the raw frame; false (xr, yr untouched) when
// the position lies outside the valid radius.
MCS_LENS_HD bool lens_apply(const Lens &L, double u, double v, double &xr, double &yr)
{
#if MCS_LENS_MODELS
    if (L.model != 0.0) return lens_fish(L, true, u, v, xr, yr);
#endif
    const double x = (u - L.cx) / L.fx, y = (v - L.cy) / L.fy;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    if (!(r2 <= L.r2max)) return false;
    const double kr = lens_num(L, r2) / lens_den(L, r2);
    const double xd = x * kr + L.k[2] * _2xy + L.k[3] * (r2 + 2 * x2) + L.k[8] * r2 +
                      L.k[9] * r2 * r2;
    const double yd = y * kr + L.k[2] * (r2 + 2 * y2) + L.k[3] * _2xy + L.k[10] * r2 +
                      L.k[11] * r2 * r2;
    xr = L.fx * xd + L.cx;
    yr = L.fy * yd + L.cy;
    return true;
}

// The lens polynomial alone, lens_apply's arithmetic without the valid-radius rule (the iterates
// of lens_invert may leave the radius on their way).
MCS_LENS_HD void lens_poly(const Lens &L, double u, double v, double &xr, double &yr)
{
#if MCS_LENS_MODELS
    if (L.model != 0.0) {
        (void)lens_fish(L, false, u, v, xr, yr);
        return;
    }
#endif
    const double x = (u - L.cx) / L.fx, y = (v - L.cy) / L.fy;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = lens_num(L, r2) / lens_den(L, r2);
    const double xd = x * kr + L.k[2] * _2xy + L.k[3] * (r2 + 2 * x2) + L.k[8] * r2 +
                      L.k[9] * r2 * r2;
    const double yd = y * kr + L.k[2] * (r2 + 2 * y2) + L.k[3] * _2xy + L.k[10] * r2 +
                      L.k[11] * r2 * r2;
    xr = L.fx * xd + L.cx;
    yr = L.fy * yd + L.cy;
}

// Acceptance bound of both inverses, on both axes.
constexpr double kLensInvTol = 1.0 / 1048576.0;   // 2^-20 px (half a float ulp at x >= 1024: 2^-14)

// The fisheye inverse is radial: the raw position's normalised radius is theta_d.  Solved for
// the undistorted radius r by kFishInvIters Newton steps on g(r) = td(lens_atan(r)) - theta_d
// from r = theta_d, with the analytic derivative (P(t) + t P'(t)) / (1 + r r); the position is
// the raw one scaled by r / theta_d.  Acceptance as lens_invert's, below.  A fixed count, so
// host and device run the same operations: every pixel with a preimage of the three 160 x 120
// lenses of tests/native/fisheye_check.cpp inverts from 8 steps on (4 without fold-back; the
// steps are slowest next to the angle where theta_d stops growing), and two more are run.  Worst
// round trip there: 5.7e-14 px.  lens_fish_invert_n is the same with the count as an argument,
// for that program.
constexpr int kFishInvIters = 10;
MCS_LENS_HD bool lens_fish_invert_n(const Lens &L, int iters, double xr, double yr, double &u,
                                    double &v)
{
    const double xd = (xr - L.cx) / L.fx, yd = (yr - L.cy) / L.fy;
    const double td = __builtin_sqrt(xd * xd + yd * yd);
    double r = td;
    for (int it = 0; it < iters; it++) {
        const double t = lens_atan(r);
        const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        const double g = t * (1 + L.k[0] * t2 + L.k[1] * t4 + L.k[2] * t6 + L.k[3] * t8) - td;
        const double dg = (1 + 3 * L.k[0] * t2 + 5 * L.k[1] * t4 + 7 * L.k[2] * t6 +
                           9 * L.k[3] * t8) / (1 + r * r);
        r = r - g / dg;
    }
    const double s = (td == 0.0) ? 1.0 : r / td;
    const double pu = L.fx * (xd * s) + L.cx, pv = L.fy * (yd * s) + L.cy;
    if (!(pu - pu == 0.0 && pv - pv == 0.0)) return false;   // inf or NaN
    double bx, by;
    if (!lens_fish(L, true, pu, pv, bx, by)) return false;
    const double dx = bx - xr, dy = by - yr;
    if (!(dx <= kLensInvTol && dx >= -kLensInvTol && dy <= kLensInvTol && dy >= -kLensInvTol))
        return false;
    u = pu;
    v = pv;
    return true;
}
MCS_LENS_HD bool lens_fish_invert(const Lens &L, double xr, double yr, double &u, double &v)
{
    return lens_fish_invert_n(L, kFishInvIters, xr, yr, u, v);
}

// The inverse: (xr, yr) of the raw frame -> (u, v) of the undistorted image (mcs_rig_job_set_lens:
// matched keypoints of raw frames carried into the image their homography is estimated in).
// kLensInvIters Newton steps on lens_poly from the raw position itself, the Jacobian by forward
// differences of 1 / 1024 px (a power of two: the quotient is a product), the 2 x 2 solve by
// Cramer's rule; a fixed count, so host and device run the same operations.  Valid iff the result
// is finite, inside the valid radius, and lens_apply takes it back to within kLensInvTol px of
// (xr, yr) on both axes -- which rejects raw positions without a preimage inside the radius, where
// the iteration ends somewhere arbitrary.  false: u, v untouched.
constexpr int kLensInvIters = 6;
MCS_LENS_HD bool lens_invert(const Lens &L, double xr, double yr, double &u, double &v)
{
#if MCS_LENS_MODELS
    if (L.model != 0.0) return lens_fish_invert(L, xr, yr, u, v);
#endif
    const double h = 1.0 / 1024.0, ih = 1024.0;
    double pu = xr, pv = yr;
    for (int it = 0; it < kLensInvIters; it++) {
        double fx0, fy0, fx1, fy1, fx2, fy2;
        lens_poly(L, pu, pv, fx0, fy0);
        lens_poly(L, pu + h, pv, fx1, fy1);
        lens_poly(L, pu, pv + h, fx2, fy2);
        const double a = (fx1 - fx0) * ih, b = (fx2 - fx0) * ih;
        const double c = (fy1 - fy0) * ih, d = (fy2 - fy0) * ih;
        const double ex = fx0 - xr, ey = fy0 - yr;
        const double det = a * d - b * c;
        pu = pu - (d * ex - b * ey) / det;
        pv = pv - (a * ey - c * ex) / det;
    }
    if (!(pu - pu == 0.0 && pv - pv == 0.0)) return false;   // inf or NaN
    double bx, by;
    if (!lens_apply(L, pu, pv, bx, by)) return false;
    const double dx = bx - xr, dy = by - yr;
    if (!(dx <= kLensInvTol && dx >= -kLensInvTol && dy <= kLensInvTol && dy >= -kLensInvTol))
        return false;
    u = pu;
    v = pv;
    return true;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The valid radius squared of L's radial polynomial (L.r2max is not read).
static inline double lens_r2max(const Lens &L)
{
    double f_prev = 0.0;
    for (int i = 1; i <= 2048; i++) {
        const double r = i / 256.0, r2 = r * r;
        const double den = lens_den(L, r2);
        const double f = r * (lens_num(L, r2) / den);
        if (!(den > 0) || !(f > f_prev)) {
            const double rp = (i - 1) / 256.0;
            return rp * rp;
        }
        f_prev = f;
    }
    return __builtin_inf();
}

// The valid angle of a fisheye L (L.r2max is not read).
static inline double lens_tmax(const Lens &L)
{
    double f_prev = 0.0;
    for (int i = 1; i <= 1608; i++) {
        const double f = lens_fish_td(L, i / 1024.0);
        if (!(f > 0) || !(f > f_prev)) return (i - 1) / 1024.0;
        f_prev = f;
    }
    return __builtin_inf();
}
#endif

}  // namespace mcs
