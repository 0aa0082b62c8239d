/*
 * orc_orb.c -- TEST INFRASTRUCTURE ONLY (the parity checker), never the product path.
 *
 * CPU restatement of the ORB specified in multicamera_stitching_amd/csrc/mcs_orb_core.h
 * (the per-frame replacement of detectAndDescribe,
 * PostScripts/Stitcher/StitcherClass.py:356-403, which uses OpenCV SIFT).  OpenCV's ORB is
 * third-party and not installed here: this checks the GPU against our specification, written
 * independently of the product code.  Pyramid levels come from orc_resize_linear (the OpenCV 3.4
 * INTER_LINEAR restatement) of the previous level; the rBRIEF pattern is OpenCV's
 * bit_pattern_31_ (passed in by the caller, 256 x 4 ints).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

int orc_resize_linear(const uint8_t *src, int sw, int sh, long sstep, int cn, uint8_t *dst,
                      int dw, int dh, long dstep);

static const int circle[16][2] = {{0, 3},  {1, 3},  {2, 2},  {3, 1},   {3, 0},   {3, -1},
                                  {2, -2}, {1, -3}, {0, -3}, {-1, -3}, {-2, -2}, {-3, -1},
                                  {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};
static const int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
static const int bk[7] = {18, 34, 49, 54, 49, 34, 18};

typedef struct {
    int x, y;
    double r;
} cand_t;

static int cmp_cand(const void *a, const void *b)
{
    const cand_t *p = (const cand_t *)a, *q = (const cand_t *)b;
    if (p->r != q->r) return p->r > q->r ? -1 : 1;
    if (p->y != q->y) return p->y < q->y ? -1 : 1;
    return p->x < q->x ? -1 : (p->x > q->x);
}

static int fast_score(const uint8_t *p, int step)
{
    int d[16], best = -255;
    for (int i = 0; i < 16; i++) d[i] = (int)p[circle[i][1] * step + circle[i][0]] - p[0];
    for (int s = 0; s < 16; s++) {
        int lo = 255, hi = 255;
        for (int k = 0; k < 9; k++) {
            int v = d[(s + k) & 15];
            if (v < lo) lo = v;
            if (-v < hi) hi = -v;
        }
        int m = lo > hi ? lo : hi;
        if (m > best) best = m;
    }
    return best;
}

static double harris(const uint8_t *p, int st)
{
    int64_t a = 0, b = 0, c = 0;
    for (int v = -3; v <= 3; v++)
        for (int u = -3; u <= 3; u++) {
            const uint8_t *q = p + v * st + u;
            int ix = (q[-st + 1] + 2 * q[1] + q[st + 1]) - (q[-st - 1] + 2 * q[-1] + q[st - 1]);
            int iy = (q[st - 1] + 2 * q[st] + q[st + 1]) - (q[-st - 1] + 2 * q[-st] + q[-st + 1]);
            a += (int64_t)ix * ix;
            b += (int64_t)iy * iy;
            c += (int64_t)ix * iy;
        }
    double t = (double)(a + b);
    return (double)(a * b - c * c) - 0.04 * (t * t);
}

/* reflect-101; on a level narrower than the blur's 4 taps the position is first held to the one
 * reflection the image has (levels that small carry no keypoint, so no value of theirs is used) */
static int refl(int i, int n)
{
    if (i < -(n - 1)) i = -(n - 1);
    if (i > 2 * n - 2) i = 2 * n - 2;
    return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

/* Returns the number of keypoints written (<= nfeatures).  kp_level/xy/response/cs_sn may be
 * used for parity: cs_sn holds the orientation's (cos, sin). */
int orc_orb_detect(const uint8_t *gray, int w, int h, int nfeatures, int nlevels,
                   float scale_factor, int threshold, const int *pattern, float *kp_xy,
                   double *kp_response, int *kp_level, double *cs_sn, uint8_t *desc)
{
    if (nlevels < 1 || nlevels > 12) return -1;
    int lw[12], lh[12], quota[12];
    float lscale[12];
    uint8_t *lv[12];
    for (int l = 0; l < nlevels; l++) {
        lscale[l] = (float)pow((double)scale_factor, (double)l);
        lw[l] = (int)lrintf((float)w / lscale[l]);
        lh[l] = (int)lrintf((float)h / lscale[l]);
        lv[l] = (uint8_t *)malloc((size_t)lw[l] * lh[l]);
        if (l == 0) memcpy(lv[0], gray, (size_t)w * h);
        else orc_resize_linear(lv[l - 1], lw[l - 1], lh[l - 1], lw[l - 1], 1, lv[l], lw[l], lh[l],
                               lw[l]);
    }
    {
        float factor = (float)(1.0 / scale_factor);
        float per = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
        /* a level takes its rounded share, or what the levels before it left of nfeatures */
        int left = nfeatures;
        for (int l = 0; l < nlevels - 1; l++) {
            const int share = (int)lrintf(per);
            quota[l] = share < left ? share : left;
            left -= quota[l];
            per *= factor;
        }
        quota[nlevels - 1] = left;
    }
    int n = 0;
    const int E = 31;
    for (int l = 0; l < nlevels; l++) {
        const int W = lw[l], H = lh[l];
        const uint8_t *I = lv[l];
        /* blur: horizontal (exact) then vertical, one rounding */
        int *hb = (int *)malloc(sizeof(int) * (size_t)W * H);
        uint8_t *B = (uint8_t *)malloc((size_t)W * H);
        uint8_t *S = (uint8_t *)calloc((size_t)W * H, 1);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                int s = 0;
                for (int i = 0; i < 7; i++) s += bk[i] * I[y * W + refl(x + i - 3, W)];
                hb[y * W + x] = s;
            }
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                int s = 0;
                for (int j = 0; j < 7; j++) s += bk[j] * hb[refl(y + j - 3, H) * W + x];
                B[y * W + x] = (uint8_t)((s + 32768) >> 16);
            }
        for (int y = E - 1; y < H - (E - 1); y++)
            for (int x = E - 1; x < W - (E - 1); x++) {
                int sc = fast_score(I + y * W + x, W);
                S[y * W + x] = (uint8_t)(sc > threshold ? sc : 0);
            }
        int nc = 0, capc = 1024;
        cand_t *cs = (cand_t *)malloc(sizeof(cand_t) * capc);
        for (int y = E; y < H - E; y++)
            for (int x = E; x < W - E; x++) {
                int c = S[y * W + x], keep = c > 0;
                for (int dy = -1; dy <= 1 && keep; dy++)
                    for (int dx = -1; dx <= 1; dx++)
                        if ((dx || dy) && !(c > S[(y + dy) * W + x + dx])) keep = 0;
                if (!keep) continue;
                if (nc == capc) cs = (cand_t *)realloc(cs, sizeof(cand_t) * (capc *= 2));
                cs[nc].x = x, cs[nc].y = y, cs[nc].r = harris(I + y * W + x, W);
                nc++;
            }
        qsort(cs, (size_t)nc, sizeof(cand_t), cmp_cand);
        const int take = nc < quota[l] ? nc : quota[l];
        for (int i = 0; i < take; i++, n++) {
            const int x = cs[i].x, y = cs[i].y;
            const uint8_t *p = I + y * W + x;
            int64_t m10 = 0, m01 = 0;
            for (int u = -15; u <= 15; u++) m10 += u * p[u];
            for (int v = 1; v <= 15; v++) {
                int64_t vs = 0;
                for (int u = -umax[v]; u <= umax[v]; u++) {
                    int a = p[u + v * W], b = p[u - v * W];
                    vs += a - b;
                    m10 += (int64_t)u * (a + b);
                }
                m01 += v * vs;
            }
            double fx = (double)m10, fy = (double)m01, r = sqrt(fx * fx + fy * fy);
            double c = r > 0.0 ? fx / r : 1.0, s = r > 0.0 ? fy / r : 0.0;
            const uint8_t *bp = B + y * W + x;
            uint8_t *d = desc + 32 * (size_t)n;
            memset(d, 0, 32);
            for (int q = 0; q < 256; q++) {
                const int *t = pattern + 4 * q;
                int x1 = (int)rint((double)t[0] * c - (double)t[1] * s);
                int y1 = (int)rint((double)t[0] * s + (double)t[1] * c);
                int x2 = (int)rint((double)t[2] * c - (double)t[3] * s);
                int y2 = (int)rint((double)t[2] * s + (double)t[3] * c);
                if (bp[y1 * W + x1] < bp[y2 * W + x2]) d[q >> 3] |= (uint8_t)(1u << (q & 7));
            }
            kp_xy[2 * n] = (float)x * lscale[l];
            kp_xy[2 * n + 1] = (float)y * lscale[l];
            kp_response[n] = cs[i].r;
            kp_level[n] = l;
            cs_sn[2 * n] = c;
            cs_sn[2 * n + 1] = s;
        }
        free(cs); free(hb); free(B); free(S);
    }
    for (int l = 0; l < nlevels; l++) free(lv[l]);
    return n;
}
