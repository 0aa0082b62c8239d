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
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MCS_LENS_HD __host__ __device__ __forceinline__
#else
#define MCS_LENS_HD static inline
#endif

namespace mcs {

// One row of the device lens table (KParams.lens_tab), kLensDoubles doubles per camera.
struct Lens {
    double fx, fy, cx, cy;
    double k[12];        // OpenCV order: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
    double r2max;        // lens_r2max(); +inf: no limit
};
constexpr int kLensDoubles = 17;
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

// (u, v) of the undistorted image -> (xr, yr) of the raw frame; false (xr, yr untouched) when
// the position lies outside the valid radius.
MCS_LENS_HD bool lens_apply(const Lens &L, double u, double v, double &xr, double &yr)
{
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

// The inverse: (xr, yr) of the raw frame -> (u, v) of the undistorted image (mcs_rig_job_set_lens:
// matched keypoints of raw frames carried into the image their homography is estimated in).
// kLensInvIters Newton steps on lens_poly from the raw position itself, the Jacobian by forward
// differences of 1 / 1024 px (a power of two: the quotient is a product), the 2 x 2 solve by
// Cramer's rule; a fixed count, so host and device run the same operations.  Valid iff the result
// is finite, inside the valid radius, and lens_apply takes it back to within kLensInvTol px of
// (xr, yr) on both axes -- which rejects raw positions without a preimage inside the radius, where
// the iteration ends somewhere arbitrary.  false: u, v untouched.
constexpr int kLensInvIters = 6;
constexpr double kLensInvTol = 1.0 / 1048576.0;   // 2^-20 px (half a float ulp at x >= 1024: 2^-14)
MCS_LENS_HD bool lens_invert(const Lens &L, double xr, double yr, double &u, double &v)
{
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
#endif

}  // namespace mcs
