// Host check of ORB's level geometry (built and run by tests/test_orb_geom_native_cpu.py, also
// with -fsanitize=address,undefined): mcs::feat::orb_geom's per-level quotas over every nfeatures
// 0..3000 x 1..12 levels x seven scale factors -- they add up to n_bound <= nfeatures, none is
// negative, and they are OpenCV's uncapped roundings wherever those stay within nfeatures -- and
// mcs::feat::pyramid_args over a grid of frame sizes: it declines (0 blocks) whenever a level step
// is 2x or more, otherwise only when its regions really do not fit LDS, and what it accepts fits
// 64 KB of LDS with one block per tile of the last level.
// Also the argument-only refusal of a Hamming train set of 2^23 descriptors (the key packs the
// index into 23 bits).  Links every host source but hip_rt.cpp and mcs_runtime.cpp; the runtime
// is never called.  Prints "ok" or the failed checks.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcs_common.h"
#include "mcs_feat_int.h"
#include "mcs_fparams.h"

static mcs::rt::Api g_api = {};
static int g_bad = 0;

// what the linked sources need of hip_rt.cpp and mcs_runtime.cpp
const mcs::rt::Api *mcs::rt::api() { return &g_api; }
const char *mcs::rt::runtime_name() { return "stub"; }
int mcs::module_function(const rt::Api *, int, Module, const char *, hipFunction_t *out)
{
    *out = nullptr;
    return MCS_OK;
}

#define CHECK(cond, ...)                                                                       \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            if (g_bad < 20) {                                                                  \
                printf("line %d: %s: ", __LINE__, #cond);                                      \
                printf(__VA_ARGS__);                                                           \
                printf("\n");                                                                  \
            }                                                                                  \
            g_bad++;                                                                           \
        }                                                                                      \
    } while (0)

static const float kScales[] = {1.05f, 1.1f, 1.2f, 1.5f, 1.99f, 2.0f, 3.0f};

// OpenCV's split (ORB_Impl::detectAndCompute), uncapped: the sum it gives.
static int opencv_quotas(int nfeatures, int nlevels, float scale, int *q)
{
    const float factor = (float)(1.0 / scale);
    float per = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; l++) {
        q[l] = (int)std::lrint(per);
        sum += q[l];
        per *= factor;
    }
    q[nlevels - 1] = nfeatures - sum > 0 ? nfeatures - sum : 0;
    return sum + q[nlevels - 1];
}

static void check_quotas()
{
    int over = 0, worst = 0;
    for (float scale : kScales)
        for (int nl = 1; nl <= 12; nl++) {
            // (the largest frame the entry points take: every level has a pixel, except the
            // twelfth at 3.0, which no frame has -- orb_geom refuses it)
            mcs::feat::OrbGeom probe;
            const bool empty = std::lrint(65535.f / (float)std::pow((double)scale, nl - 1.0)) < 1;
            if (empty) {
                CHECK(mcs::feat::orb_geom(65535, 65535, 100, nl, scale, &probe) == MCS_E_INVALID,
                      "scale %g levels %d", (double)scale, nl);
                continue;
            }
            for (int nf = 0; nf <= 3000; nf++) {
                mcs::feat::OrbGeom g;
                if (mcs::feat::orb_geom(65535, 65535, nf, nl, scale, &g) != MCS_OK) {
                    CHECK(false, "orb_geom refused scale %g levels %d nfeatures %d", (double)scale,
                          nl, nf);
                    continue;
                }
                int sum = 0, q[12];
                bool neg = false;
                for (int l = 0; l < nl; l++) sum += g.quota[l], neg = neg || g.quota[l] < 0;
                CHECK(!neg, "scale %g levels %d nfeatures %d", (double)scale, nl, nf);
                CHECK(sum == g.n_bound && g.n_bound <= nf, "scale %g levels %d nfeatures %d: sum %d "
                      "n_bound %d", (double)scale, nl, nf, sum, g.n_bound);
                const int old = opencv_quotas(nf, nl, scale, q);
                if (old <= nf)
                    CHECK(std::memcmp(q, g.quota, nl * sizeof(int)) == 0,
                          "scale %g levels %d nfeatures %d: quotas changed", (double)scale, nl, nf);
                else
                    over++, worst = old - nf > worst ? old - nf : worst;
            }
        }
    // the table is not vacuous: the uncapped split does overshoot (by up to 3) on this grid
    CHECK(over > 0 && worst == 3, "uncapped sums above nfeatures: %d, worst +%d", over, worst);
    // the cases of the defect: 14 features on 11 levels and 88 on 12 at 1.5 summed to 15 and 90
    int q[12];
    CHECK(opencv_quotas(14, 11, 1.2f, q) == 15 && opencv_quotas(88, 12, 1.5f, q) == 90 &&
          opencv_quotas(7, 8, 1.2f, q) == 8, "the known overshoots");
}

static void check_pyramid()
{
    std::vector<int> sizes;
    for (int v = 1; v <= 300; v += 13) sizes.push_back(v);   // (13 = 1 mod 4: every residue)
    for (int v : {2, 3, 4, 62, 63, 64, 65, 131, 132, 255, 256, 257, 300}) sizes.push_back(v);
    int res[4] = {0, 0, 0, 0}, fused = 0, declined_2x = 0, declined_lds = 0;
    for (int v : sizes) res[v & 3]++;
    CHECK(res[0] && res[1] && res[2] && res[3], "size residues mod 4");
    std::vector<std::pair<int, int>> frames;
    for (int w : sizes)
        for (int h : sizes) frames.push_back({w, h});
    frames.push_back({640, 480});
    frames.push_back({1920, 1080});
    for (const auto &f : frames)
        for (float scale : kScales)
            for (int nl = 1; nl <= 12; nl++) {
                const int w = f.first, h = f.second;
                mcs::feat::OrbGeom g;
                if (mcs::feat::orb_geom(w, h, 500, nl, scale, &g) != MCS_OK) continue;
                mcs::KOrbBuildArgs a;
                const unsigned blocks = mcs::feat::pyramid_args(g, nullptr, a);
                bool step2 = false;
                for (int l = 1; l < nl; l++)
                    step2 = step2 || 2 * g.lw[l] <= g.lw[l - 1] || 2 * g.lh[l] <= g.lh[l - 1];
                if (step2) {
                    CHECK(blocks == 0, "%dx%d scale %g levels %d: a 2x step taken", w, h,
                          (double)scale, nl);
                    declined_2x++;
                    continue;
                }
                const size_t lds = 2 * (size_t)a.lds_w * a.lds_h + 16;
                if (blocks == 0) {
                    // declined without a 2x step: only because the regions do not fit LDS (a last
                    // level of one tile under many levels, e.g. 261 x 300 at 1.5 from 10 levels
                    // on: the tile's region is all of level 1)
                    CHECK(lds > 65536, "%dx%d scale %g levels %d: declined with %zu bytes of LDS",
                          w, h, (double)scale, nl, lds);
                    declined_lds++;
                    continue;
                }
                fused++;
                CHECK(lds <= 65536 && a.lds_w >= 1 && a.lds_h >= 1, "%dx%d scale %g levels %d: "
                      "%zu bytes of LDS", w, h, (double)scale, nl, lds);
                const int L = nl - 1;
                const unsigned tiles = (unsigned)((g.lw[L] + a.tw - 1) / a.tw) *
                                       (unsigned)((g.lh[L] + a.th - 1) / a.th);
                CHECK(blocks == tiles && a.gx == (g.lw[L] + a.tw - 1) / a.tw && a.nlevels == nl,
                      "%dx%d scale %g levels %d: %u blocks, %u tiles", w, h, (double)scale, nl,
                      blocks, tiles);
                // a staged region is never larger than the level it is a region of
                int mw = 1, mh = 1;
                for (int l = 1; l < L; l++) mw = g.lw[l] > mw ? g.lw[l] : mw, mh = g.lh[l] > mh ? g.lh[l] : mh;
                CHECK(a.lds_w <= mw && a.lds_h <= mh, "%dx%d scale %g levels %d: region %dx%d", w,
                      h, (double)scale, nl, a.lds_w, a.lds_h);
            }
    CHECK(fused > 1000 && declined_2x > 1000 && declined_lds > 0, "fused %d, declined for a 2x step %d, for LDS %d",
          fused, declined_2x, declined_lds);
}

static void check_train_limit()
{
    static_assert(mcs::kKnnMaxTrain == 1 << 23, "the Hamming key's index field");
    uint8_t d[32] = {0};
    int32_t out[4];
    CHECK(mcs_match_hamming_knn2_host(d, 1, d, 1 << 23, out, out + 2, 0) == MCS_E_INVALID,
          "2^23 train descriptors accepted");
    const char *m = mcs_last_error();
    CHECK(m && std::strstr(m, "n_train=8388608"), "refused for another reason: %s", m ? m : "");
    CHECK(mcs_match_hamming_knn2(d, 1, d, 1 << 23, out, out + 2, 0, nullptr) == MCS_E_INVALID,
          "2^23 train descriptors accepted (device form)");
}

int main()
{
    check_quotas();
    check_pyramid();
    check_train_limit();
    if (g_bad) {
        printf("%d checks failed\n", g_bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
