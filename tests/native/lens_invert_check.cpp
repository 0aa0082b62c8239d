// Host check of the inverse lens map (built and run by tests/test_lens_invert_native_cpu.py, also
// with -fsanitize=address,undefined): mcs::lens_invert (csrc/mcs_lens_core.h) over the frames of
// the lens tests' cameras -- the five CASES of tests/test_undistort_cpu.py, FOLD of
// tests/test_lens_cpu.py and NOPRE of tests/lens_inv_ref.py; every integer pixel, a 3-px grid for
// frames larger than 640 x 480.  Every valid result must be finite, inside the valid radius and
// taken back by lens_apply to within 2^-20 px; the six lenses other than NOPRE must have no
// invalid in-frame position; NOPRE's corners must be invalid and its centre 64 x 64 block valid; an
// invalid result must leave its outputs untouched.  Links mcs_plan.cpp (lens_from).  Prints "ok"
// or the failed checks, and exits non-zero on any.
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
    int w, h;
    bool full;   // every in-frame raw position has a preimage
};

int main()
{
    const std::vector<Case> cases = {
        {"case0", {500.0, 0, 319.5, 0, 505.0, 239.5, 0, 0, 1}, {-0.28, 0.09, 0.001, -0.0005, 0.0},
         640, 480, true},
        {"case1", {1100.0, 0, 955.2, 0, 1098.0, 541.7, 0, 0, 1}, {-0.12, 0.03, 0.0, 0.0}, 1920, 1080,
         true},
        {"case2", {300.0, 0, 160.0, 0, 300.0, 120.0, 0, 0, 1},
         {0.1, -0.05, 0.002, 0.001, 0.01, 0.02, -0.01, 0.005}, 320, 240, true},
        {"case3", {250.0, 0, 100.3, 0, 260.0, 80.1, 0, 0, 1},
         {-0.2, 0.05, 0, 0, 0, 0, 0, 0, 0.001, 0.0002, -0.001, 0.0003}, 200, 150, true},
        {"case4", {420.0, 0, 209.5, 0, 420.0, 11.5, 0, 0, 1}, {}, 420, 24, true},
        {"fold", {500.0, 0, 319.5, 0, 505.0, 239.5, 0, 0, 1}, {-0.35, 0.12, 0, 0, -0.02}, 640, 480,
         true},
        {"nopre", {200.0, 0, 159.5, 0, 200.0, 119.5, 0, 0, 1}, {-0.3, 0, 0, 0}, 320, 240, false},
    };
    const double tol = 1.0 / 1048576.0;
    for (const Case &c : cases) {
        mcs::Lens L;
        CHECK(mcs::lens_from(c.K, c.d.data(), (int)c.d.size(), &L) == MCS_OK);
        const int step = (long)c.w * c.h > 640L * 480 ? 3 : 1;
        long valid = 0, invalid = 0;
        double worst = 0.0;
        for (int y = 0; y < c.h; y += step)
            for (int x = 0; x < c.w; x += step) {
                double u = -12345.0, v = -54321.0;
                if (!mcs::lens_invert(L, (double)x, (double)y, u, v)) {
                    invalid++;
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
        printf("%s: %ld valid, %ld invalid, worst round trip %.3g px\n", c.name, valid, invalid,
               worst);
        CHECK(valid > 0);
        if (c.full) CHECK(invalid == 0);
        else {
            double u, v;
            const int xs[2] = {0, c.w - 1}, ys[2] = {0, c.h - 1};
            for (int i = 0; i < 4; i++)
                CHECK(!mcs::lens_invert(L, (double)xs[i & 1], (double)ys[i >> 1], u, v));
            for (int y = c.h / 2 - 32; y < c.h / 2 + 32; y++)
                for (int x = c.w / 2 - 32; x < c.w / 2 + 32; x++)
                    CHECK(mcs::lens_invert(L, (double)x, (double)y, u, v));
            CHECK(invalid > 0);
        }
    }
    // non-finite input: invalid, never a trap
    {
        mcs::Lens L;
        CHECK(mcs::lens_from(cases[0].K, cases[0].d.data(), 5, &L) == MCS_OK);
        double u = 1.0, v = 2.0;
        CHECK(!mcs::lens_invert(L, std::nan(""), 0.0, u, v) && u == 1.0 && v == 2.0);
        CHECK(!mcs::lens_invert(L, 0.0, HUGE_VAL, u, v) && u == 1.0 && v == 2.0);
    }
    if (g_bad) {
        printf("%d checks failed\n", g_bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
