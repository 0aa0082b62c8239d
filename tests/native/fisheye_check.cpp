// Host check of the fisheye lens model (built and run by tests/test_fisheye_native_cpu.py):
// mcs::lens_atan against libm, and mcs::lens_invert (csrc/mcs_lens_core.h) over every pixel of
// 160 x 120 frames under three fisheye lenses -- D = 0, a mild D, and a D with k1 < 0 whose
// distorted angle folds back inside the frame.  Every valid result must be finite, inside the
// valid angle and taken back by lens_apply to within 2^-20 px; the two lenses without fold-back
// must have no invalid pixel; an invalid result must leave its outputs untouched.  The smallest
// Newton step count at which every pixel that has a preimage (one that inverts after 64 steps)
// inverts is printed, and kFishInvIters must be that count plus two.  argv[1], when given,
// receives the fold-back lens' map of rejected pixels (w * h bytes, 1 = rejected), which the test
// compares with tests/fisheye_ref.py's.  Links mcs_plan.cpp (lens_from).  Prints "ok" or the
// failed checks, and exits non-zero on any.
#include <cmath>
#include <cstdio>
#include <vector>

#include "mcs_common.h"

static int g_bad = 0;

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            if (g_bad < 20) printf("line %d: %s\n", __LINE__, #cond);                          \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

struct Case {
    const char *name;
    double K[9];
    std::vector<double> d;
    bool full;   // every in-frame raw position has a preimage
};

static double ulps(double got, double want)
{
    const double u = std::nextafter(std::fabs(want), HUGE_VAL) - std::fabs(want);
    return std::fabs(got - want) / u;
}

int main(int argc, char **argv)
{
    const int w = 160, h = 120;
    // the arctangent: 0..8 in steps of 1 / 4096, the powers of two, the breakpoints' neighbours
    {
        double worst = 0.0, prev = -1.0;
        CHECK(mcs::lens_atan(0.0) == 0.0 && !std::signbit(mcs::lens_atan(0.0)));
        for (int i = 0; i <= 32768; i++) {
            const double r = i / 4096.0, a = mcs::lens_atan(r);
            CHECK(a >= prev);
            prev = a;
            if (i) worst = std::fmax(worst, ulps(a, std::atan(r)));
        }
        for (int k = -60; k <= 60; k++) {
            const double r = std::ldexp(1.0, k);
            worst = std::fmax(worst, ulps(mcs::lens_atan(r), std::atan(r)));
        }
        const double br[4] = {0.4375, 0.6875, 1.1875, 2.4375};
        for (double b : br) {
            const double lo = std::nextafter(b, 0.0), hi = std::nextafter(b, 9.0);
            CHECK(mcs::lens_atan(lo) <= mcs::lens_atan(b) && mcs::lens_atan(b) <= mcs::lens_atan(hi));
            worst = std::fmax(worst, ulps(mcs::lens_atan(lo), std::atan(lo)));
            worst = std::fmax(worst, ulps(mcs::lens_atan(b), std::atan(b)));
            worst = std::fmax(worst, ulps(mcs::lens_atan(hi), std::atan(hi)));
        }
        printf("lens_atan: worst %.3f ulp from libm\n", worst);
        CHECK(worst <= 4.0);
        CHECK(std::isnan(mcs::lens_atan(std::nan(""))));
    }
    const std::vector<Case> cases = {
        {"zero", {96.0, 0, 79.5, 0, 96.0, 59.5, 0, 0, 1}, {}, true},
        {"mild", {100.0, 0, 80.3, 0, 101.0, 59.1, 0, 0, 1}, {-0.03, 0.01, -0.002, 0.0005}, true},
        {"fold", {96.0, 0, 79.5, 0, 96.0, 59.5, 0, 0, 1}, {-0.3, 0.0, 0.0, 0.0}, false},
    };
    const double tol = 1.0 / 1048576.0;
    int need = 0;
    for (const Case &c : cases) {
        mcs::Lens L;
        CHECK(mcs::lens_from(c.K, c.d.data(), (int)c.d.size(), &L, MCS_LENS_FISHEYE) == MCS_OK);
        CHECK(L.model == 1.0 && (c.full ? std::isinf(L.r2max) : L.r2max < 1.5));
        long valid = 0, invalid = 0;
        double worst = 0.0;
        std::vector<unsigned char> rejected((size_t)w * h, 0);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                double u = -12345.0, v = -54321.0;
                if (!mcs::lens_invert(L, (double)x, (double)y, u, v)) {
                    invalid++;
                    rejected[(size_t)y * w + x] = 1;
                    CHECK(u == -12345.0 && v == -54321.0);
                    continue;
                }
                valid++;
                CHECK(std::isfinite(u) && std::isfinite(v));
                double bx = 0.0, by = 0.0;
                const bool in = mcs::lens_apply(L, u, v, bx, by);
                CHECK(in);
                const double e = std::fmax(std::fabs(bx - x), std::fabs(by - y));
                CHECK(in && e <= tol);
                if (in && e > worst) worst = e;
            }
        // the smallest step count that inverts every pixel with a preimage
        int least = 0;
        for (int n = 1; n <= 64 && !least; n++) {
            bool all = true;
            for (int y = 0; y < h && all; y++)
                for (int x = 0; x < w && all; x++) {
                    double u, v, u2, v2;
                    if (mcs::lens_fish_invert_n(L, 64, (double)x, (double)y, u, v))
                        all = mcs::lens_fish_invert_n(L, n, (double)x, (double)y, u2, v2);
                }
            if (all) least = n;
        }
        CHECK(least > 0);
        if (least > need) need = least;
        printf("%s: %ld valid, %ld invalid, worst round trip %.3g px, inverts from %d steps\n",
               c.name, valid, invalid, worst, least);
        CHECK(valid > 0);
        if (c.full) {
            CHECK(invalid == 0);
        } else {
            double u, v;
            const int xs[2] = {0, w - 1}, ys[2] = {0, h - 1};
            for (int i = 0; i < 4; i++)
                CHECK(!mcs::lens_invert(L, (double)xs[i & 1], (double)ys[i >> 1], u, v));
            for (int y = h / 2 - 32; y < h / 2 + 32; y++)
                for (int x = w / 2 - 32; x < w / 2 + 32; x++)
                    CHECK(mcs::lens_invert(L, (double)x, (double)y, u, v));
            CHECK(invalid > 0);
            if (argc > 1) {
                FILE *f = fopen(argv[1], "wb");
                CHECK(f && fwrite(rejected.data(), 1, rejected.size(), f) == rejected.size());
                if (f) fclose(f);
            }
        }
    }
    printf("steps: %d needed, %d run\n", need, mcs::kFishInvIters);
    CHECK(mcs::kFishInvIters == need + 2);
    // non-finite input: invalid, never a trap
    {
        mcs::Lens L;
        CHECK(mcs::lens_from(cases[1].K, cases[1].d.data(), 4, &L, MCS_LENS_FISHEYE) == MCS_OK);
        double u = 1.0, v = 2.0;
        CHECK(!mcs::lens_invert(L, std::nan(""), 0.0, u, v) && u == 1.0 && v == 2.0);
        CHECK(!mcs::lens_invert(L, 0.0, HUGE_VAL, u, v) && u == 1.0 && v == 2.0);
        // the principal point is its own inverse
        CHECK(mcs::lens_invert(L, L.cx, L.cy, u, v) && u == L.cx && v == L.cy);
    }
    if (g_bad) {
        printf("%d checks failed\n", g_bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
