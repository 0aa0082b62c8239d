// mcs_launch.cpp -- the per-launch scheduling of a prepared plan: which kernels of the stitch and
// sweep modules run for a batch of captures, on which of the plan's streams, in what order.
#include <algorithm>
#include <cstdlib>

#include "mcs_common.h"
#include "mcs_plan_state.h"

namespace mcs {
namespace host {

void need_mask(const mcs_flat_desc &fd, bool *need)
{
    for (int i = 0; i < MCS_MAX_CAMS; i++) need[i] = false;
    need[0] = true;
    for (int j = 0; j < fd.n_stages; j++) need[fd.st[j].cam] = true;
}

// Lowest used camera address for frame 0 of `kp`, and whether every used byte of that frame lies
// within 4 GiB above it (then the kernel addresses taps as SGPR base + 32-bit offsets).
static int g_force_off64 = 0;   // test hook: exercise the 64-bit-address kernels

bool offset_base(const mcs_plan *p, const mcs::KParams &kp, const uint8_t **base)
{
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    uintptr_t lo = UINTPTR_MAX, hi = 0;
    for (int i = 0; i < p->fd.n_cams; i++) {
        if (!need[i]) continue;
        const uintptr_t a = (uintptr_t)kp.cams[i];
        const uintptr_t e = a + (uintptr_t)p->fd.cam_w[i] * p->fd.cam_h[i] * p->fd.channels;
        lo = a < lo ? a : lo;
        hi = e > hi ? e : hi;
    }
    const bool off32 = !g_force_off64 && hi - lo < (uintptr_t(1) << 32);
    *base = off32 ? (const uint8_t *)lo : nullptr;
    return off32;
}

// The streaming kernel's DMA base: when every byte of every capture of every used camera lies in
// [base, base + 4 GiB) the footprint rows are read through one buffer resource with 32-bit
// offsets (mcs_stream_c*_b32).  Captures are fstride = cam_fstride[0] apart (the stream kernel's
// layout).
static bool stream_base(const mcs_plan *p, const mcs::KParams &kp, int n_frames,
                        const uint8_t **base)
{
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    uintptr_t lo = UINTPTR_MAX, hi = 0;
    const uintptr_t span = (uintptr_t)(n_frames > 0 ? n_frames - 1 : 0) * kp.cam_fstride[0];
    for (int i = 0; i < p->fd.n_cams; i++) {
        if (!need[i]) continue;
        const uintptr_t a = (uintptr_t)kp.cams[i];
        const uintptr_t e = a + span + (uintptr_t)p->fd.cam_w[i] * p->fd.cam_h[i] * p->fd.channels;
        lo = a < lo ? a : lo;
        hi = e > hi ? e : hi;
    }
    const bool b32 = !g_force_off64 && lo <= hi && hi - lo < (uintptr_t(1) << 32);
    *base = b32 ? (const uint8_t *)lo : kp.base;
    return b32;
}

int launch_args(const Api *A, hipFunction_t f, unsigned gx, unsigned gy, unsigned bx,
                unsigned by, void *args, size_t sz, hipStream_t s, unsigned gz, unsigned lds)
{
    void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                   HIP_LAUNCH_PARAM_END};
    HIP_TRY(A->hipModuleLaunchKernel(f, gx, gy, gz, bx, by, 1, lds, s, nullptr, cfg));
    return MCS_OK;
}

void mb_args(const mcs_plan *p, const mcs::KParams &P, mcs::KMbArgs &a)
{
    a.P = P;
    a.owner = p->t.d_owner;
    a.list = p->t.d_blist;
    a.desc = p->t.d_mbdesc;
    a.tab = p->t.d_mbtab;
    a.foot = p->t.d_mbfoot;
    a.g1 = p->t.d_mbg1;
    a.g2 = p->t.d_mbg2;
    a.slots = p->t.mb_slots;
    a.chunk = p->t.mb_chunk;
    a.f0 = 0;
    a.nf = 0;
    a.list0 = 0;
    a.n_list = p->t.n_blend;
    a.rec = p->t.d_mbrec;
}

void band_args(const mcs_plan *p, const mcs::KParams &P, mcs::KMbBandArgs &a)
{
    a.P = P;
    a.list = p->t.d_blist;
    a.tile_bt = p->t.d_tile_bt;
    a.bands = p->t.d_bands;
    a.bdesc = p->t.d_bdesc;
    a.bgrp = p->t.d_bgrp;
    a.bdesc16 = p->t.d_bdesc16;
    a.g1 = p->t.d_mbg1;
    a.g2 = p->t.d_mbg2;
    a.slots = p->t.mb_slots;
    a.chunk = p->t.mb_chunk;
    a.f0 = 0;
    a.nf = 0;
    a.gxb = p->t.gxb;
    a.band0 = 0;
    a.n_in = p->t.n_bands_in;
    a.band1 = p->t.n_bands_in;
    a.nb = p->t.n_bands;
}

// 1-D grid of an XCD-grouped launch of n units (mcs_blend.h xcd_unit): 8 * ceil(n / 8) blocks.
static unsigned xcd_grid(int64_t n) { return 8u * (unsigned)((n + 7) / 8); }

// The band pass's dword-aligned window form (mb_bands AL, mb_desc's sh) applies when every used
// camera's rows and frames are multiples of 4 bytes, its frames start at 4-byte boundaries and hold
// at least pitch + 12 bytes; otherwise the unaligned 8-byte form.
static int band_form(const mcs_plan *p, const mcs::KParams &P)
{
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    const int C = p->fd.channels;
    for (int i = 0; i < p->fd.n_cams; i++) {
        if (!need[i]) continue;
        const int64_t pitch = (int64_t)p->fd.cam_w[i] * C, fb = pitch * p->fd.cam_h[i];
        if (pitch % 4 || fb % 4 || fb < pitch + 12 || P.cam_fstride[i] % 4 ||
            (uintptr_t)P.cams[i] % 4)
            return 0;
    }
    return 1;
}

// Multi-band level pyramids of captures [f0, f0 + nf) on stream s: the band pass when the plan
// has one (interior and bottom / right edge bands in ONE launch, blocks below n_in interior, so
// the edge bands run beside the interior ones), else mb_levels.
static int launch_mb_levels(const Api *A, const mcs_plan *p, const Kernels *k, mcs::KMbArgs &m,
                            int f0, int nf, hipStream_t s, bool gained)
{
    m.f0 = f0;
    m.nf = nf;
    if (p->t.n_bands > 0) {
        mcs::KMbBandArgs b;
        band_args(p, m.P, b);
        b.f0 = f0;
        b.nf = nf;
        const unsigned gy = (unsigned)((nf + mcs::kMbBandFrames - 1) / mcs::kMbBandFrames);
        const int form = band_form(p, b.P);
        const int kind = p->t.n_bands_in == 0 ? 1 : (p->t.n_bands > p->t.n_bands_in ? 2 : 0);
        if (kind == 1) b.band0 = 0;
        return launch_args(A, (gained ? k->mb_bands_g : k->mb_bands)[p->fd.channels][form][kind],
                           xcd_grid((int64_t)p->t.n_bands * gy), 1, mcs::kMbBandLanes, 1, &b,
                           sizeof(b), s);
    }
    const unsigned gz = (unsigned)((nf + mcs::kMbLvFrames - 1) / mcs::kMbLvFrames);
    return launch_args(A, (gained ? k->mb_levels_g : k->mb_levels)[p->fd.channels],
                       (unsigned)p->t.n_blend,
                       (unsigned)p->t.mb_slots, mcs::kMbLvThreads, 1, &m, sizeof(m), s, gz);
}

// Multi-band tiles degraded to the feather rule (more than kBlendSlots owners in their
// neighbourhood): the feather kernel over d_dense, on stream s after the mosaic is written.
static int launch_dense(const Api *A, const mcs_plan *p, const Kernels *k, const mcs::KParams &P,
                        int n_frames, hipStream_t s, bool gained)
{
    if (p->blend != MCS_BLEND_MULTIBAND || p->t.n_dense <= 0) return MCS_OK;
    mcs::KBlendArgs b;
    b.P = P;
    b.owner = p->t.d_owner;
    b.list = p->t.d_dense;
    b.n_frames = n_frames;
    b.pad_ = 0;
    return launch_args(A, (gained ? k->feather_g : k->feather)[p->fd.channels][p->fd.interp],
                       p->t.n_dense, n_frames, 256, 1, &b, sizeof(b), s);
}

// The multi-band blend kernel for the plan's owner count (<= 2, <= 4, <= 8 per neighbourhood).
static int launch_mb_blend(const Api *A, const mcs_plan *p, const Kernels *k, mcs::KMbArgs &m,
                           int f0, int nf, hipStream_t s)
{
    m.f0 = f0;
    m.nf = nf;
    const int v = p->t.mb_slots <= 2 ? 0 : (p->t.mb_slots <= 4 ? 1 : 2);
    m.list0 = 0;
    m.n_list = p->t.n_blend;
    return launch_args(A, k->mb_blend[p->fd.channels][v], xcd_grid((int64_t)p->t.n_blend * nf), 1,
                       mcs::kMbBlThreads, 1, &m, sizeof(m), s);
}

// Capture ranges per large-footprint tile (mcs_stream_big).  Same-box C4 A/B over 1 / 2 / 4 / 8
// parts (profiles/r06_big_parts_ab.txt): the paste launch gains with more parts (0.734 -> 0.720
// ms at 8), the multi-band launch loses (1.297 -> 1.349 ms: the extra blocks take CUs from the
// band pass and blend running beside them).  MCS_BIG_PARTS overrides both.
static int big_parts(bool multiband)
{
    static const int v = [] {
        const char *e = getenv("MCS_BIG_PARTS");
        const int n = e ? atoi(e) : 0;
        return n >= 1 && n <= 64 ? n : 0;
    }();
    return v ? v : multiband ? 1 : 8;
}

// One launch (stream over all tiles, + direct over the fallback tiles, + the blend passes) for
// n_frames captures that share one frame stride.  Work that does not read the mosaic -- the
// direct-gather tiles and the first multi-band chunk's level pyramids -- runs on two side streams,
// concurrently with the HBM-bound streaming kernel.  gained: every kernel of the pair that reads
// source bytes is its _g twin (stream, big, direct, feather, bands, levels; the multi-band blend
// reads the mosaic and the scratch) and applies P.gain_q to its taps.
static int launch_pair(const Api *A, const mcs_plan *p, const Kernels *k, mcs::KParams &P,
                       int n_frames, hipStream_t s, bool gained)
{
    // multi-band: the sweep (strips) or the band pass + blend
    const bool sweep = p->blend == MCS_BLEND_MULTIBAND && p->t.n_strips > 0;
    const bool mb = !sweep && p->blend == MCS_BLEND_MULTIBAND && p->t.n_blend > 0;
    // side work beside the main streaming launch: the large-footprint tiles and the
    // direct-gather tiles (tiles the main launch skips), on p->side
    const bool aside = p->t.n_fallback > 0 || p->t.n_big > 0;
    const bool fork = aside || mb || sweep;
    mcs::KMbArgs m;
    if (mb) mb_args(p, P, m);
    mcs::KStreamArgs args;
    args.P = P;
    const bool b32 = stream_base(p, P, n_frames, &args.P.base);
    args.tiles = p->t.d_tiles;
    args.desc = p->t.d_desc;
    args.desc4 = p->t.d_desc4;
    args.spans = p->t.d_spans;
    args.n_frames = n_frames;
    args.parts = 1;
    args.pad2_ = 0;
    if (fork) HIP_TRY(A->hipEventRecord(p->ev_fork, s));
    if (aside) HIP_TRY(A->hipStreamWaitEvent(p->side, p->ev_fork, 0));
    auto big_launch = [&](hipStream_t q) -> int {
        mcs::KStreamArgs bg = args;
        bg.order = p->t.d_big + 1;
        bg.n_order = p->t.n_big;
        // each large-footprint tile as `parts` blocks over capture ranges: one block per CU per
        // tile otherwise streams the whole batch and sets the launch's tail (C4: 31 tiles)
        bg.parts = std::max(1, std::min(big_parts(mb || sweep), n_frames));
        const auto &big = gained ? k->stream_big_g : k->stream_big;
        return launch_args(A, big[p->fd.channels][b32 ? 1 : 0],
                           8u * (((unsigned)(p->t.n_big * bg.parts) + 7u) / 8u), 1, mcs::kWave,
                           mcs::kWavesPerBlock, &bg, sizeof(bg), q, 1,
                           (unsigned)mcs::kBigStreamLds);
    };
    if (p->t.n_big > 0) {
        const int rc = big_launch(p->side);
        if (rc) return rc;
    }
    if (p->t.n_fallback > 0) {
        mcs::KDirectArgs da;
        da.P = P;
        const bool off32 = offset_base(p, da.P, &da.P.base);
        da.fallback = p->t.d_fallback;
        da.n_frames = n_frames;
        da.pad_ = 0;
        const unsigned gy = (unsigned)((n_frames + mcs::kDirectFrames - 1) / mcs::kDirectFrames);
        const int rc = launch_args(
            A, (gained ? k->direct_g : k->direct)[p->fd.channels][p->fd.interp][off32 ? 1 : 0],
            p->t.n_fallback, gy, mcs::kWave, mcs::kWavesPerBlock, &da, sizeof(da), p->side);
        if (rc) return rc;
    }
    if (aside) HIP_TRY(A->hipEventRecord(p->ev_join, p->side));
    // split (multi-band, one scratch chunk): streaming tiles under mixed pixels first, then the
    // blend on side2 (after the band pass, those tiles and the side tiles) beside the remaining
    // streaming tiles (same-box A/B, round 2: C2 1.009 -> 0.985 ms)
    const bool split = mb && p->t.d_order && p->t.n_early > 0 && n_frames <= p->t.mb_chunk;
    if (sweep) {
        // the sweep writes only its regions' pixels, the streaming tiles every other pixel: the
        // two run side by side from the start, no ordering between them
        HIP_TRY(A->hipStreamWaitEvent(p->side2, p->ev_fork, 0));
        mcs::KMbSweepArgs a;
        a.P = P;
        a.strips = p->t.d_strips;
        a.sdesc = p->t.d_sdesc;
        a.region = p->t.d_region;
        a.owner = p->t.d_owner;
        a.n_strips = p->t.n_strips;
        a.f0 = 0;
        a.nf = n_frames;
        a.pad_ = 0;
        const int al = band_form(p, P);
        int rc = launch_args(A, k->mb_sweep[p->fd.channels][al][p->t.sw_jb == 4 ? 1 : 0],
                             xcd_grid((int64_t)p->t.n_strips * n_frames), 1,
                             (unsigned)(mcs::kSwCols * p->t.sw_jb), 1, &a, sizeof(a), p->side2);
        if (rc) return rc;
        HIP_TRY(A->hipEventRecord(p->ev_join2, p->side2));
    }
    if (mb) {
        HIP_TRY(A->hipStreamWaitEvent(p->side2, p->ev_fork, 0));
        int rc = launch_mb_levels(A, p, k, m, 0, std::min(p->t.mb_chunk, n_frames), p->side2,
                                  gained);
        if (rc) return rc;
        if (!split) HIP_TRY(A->hipEventRecord(p->ev_join2, p->side2));
    }
    // 1-D grid dealt over the 8 XCDs; the kernel maps block -> tile (XCD-contiguous bands)
    const unsigned lds = (unsigned)mcs::lds_stream_bytes(p->fd.channels);
    auto stream_launch = [&](const int *order, int n_items) -> int {
        args.order = order;
        args.n_order = n_items;
        const unsigned grid = 8u * (((unsigned)n_items + 7u) / 8u);
        return launch_args(A, (gained ? k->stream_g : k->stream)[p->fd.channels][b32 ? 1 : 0],
                           grid, 1, mcs::kWave, mcs::kWavesPerBlock, &args, sizeof(args), s, 1,
                           lds);
    };
    if (split) {
        int rc = stream_launch(p->t.d_order, p->t.n_early);
        if (rc) return rc;
        HIP_TRY(A->hipEventRecord(p->ev_early, s));
        HIP_TRY(A->hipStreamWaitEvent(p->side2, p->ev_early, 0));
        if (aside) HIP_TRY(A->hipStreamWaitEvent(p->side2, p->ev_join, 0));
        rc = launch_mb_blend(A, p, k, m, 0, n_frames, p->side2);
        if (rc) return rc;
        HIP_TRY(A->hipEventRecord(p->ev_join2, p->side2));
        if (p->t.n_list > p->t.n_early) {
            rc = stream_launch(p->t.d_order + p->t.n_early, p->t.n_list - p->t.n_early);
            if (rc) return rc;
        }
        if (aside) HIP_TRY(A->hipStreamWaitEvent(s, p->ev_join, 0));
        HIP_TRY(A->hipStreamWaitEvent(s, p->ev_join2, 0));
        return launch_dense(A, p, k, P, n_frames, s, gained);
    }
    {
        // (d_order: the tile order of prepare / prepare_bands; NULL: row-major grid order)
        const int rc = p->t.d_order ? stream_launch(p->t.d_order, p->t.n_list)
                                  : stream_launch(nullptr, p->gx * p->gy);
        if (rc) return rc;
    }
    if (aside) HIP_TRY(A->hipStreamWaitEvent(s, p->ev_join, 0));
    if (mb || sweep) HIP_TRY(A->hipStreamWaitEvent(s, p->ev_join2, 0));
    if (p->t.n_blend > 0 && !sweep) {
        // recompute the blended tiles over the owner-sampled mosaic (same stream: ordered)
        int rc = MCS_OK;
        if (p->blend == MCS_BLEND_FEATHER) {
            mcs::KBlendArgs b;
            b.P = P;
            b.owner = p->t.d_owner;
            b.list = p->t.d_blist;
            b.n_frames = n_frames;
            b.pad_ = 0;
            rc = launch_args(A, (gained ? k->feather_g : k->feather)[p->fd.channels][p->fd.interp],
                             p->t.n_blend, n_frames, 256, 1, &b, sizeof(b), s);
        } else {
            // multi-band: per chunk of captures (scratch stride mb_chunk) levels (chunk 0's
            // already ran on the side stream) then blend
            for (int f0 = 0; f0 < n_frames && rc == MCS_OK; f0 += p->t.mb_chunk) {
                const int nf = std::min(p->t.mb_chunk, n_frames - f0);
                if (f0 > 0) rc = launch_mb_levels(A, p, k, m, f0, nf, s, gained);
                if (rc == MCS_OK) rc = launch_mb_blend(A, p, k, m, f0, nf, s);
            }
        }
        if (rc) return rc;
    }
    return launch_dense(A, p, k, P, n_frames, s, gained);
}

// Side streams + fork/join events for the direct-gather tiles and the multi-band levels (created
// once per plan, when needed).
static int ensure_side(const Api *A, mcs_plan *p)
{
    const bool mb = p->blend == MCS_BLEND_MULTIBAND && p->t.n_blend > 0;
    const bool aside = p->t.n_fallback > 0 || p->t.n_big > 0;
    int least = 0, greatest = 0;
    if (aside && !p->side) HIP_TRY(A->hipDeviceGetStreamPriorityRange(&least, &greatest));
    if ((aside || mb) && !p->ev_fork)
        HIP_TRY(A->hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    if (aside && !p->side) {
        HIP_TRY(A->hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
        // (the least priority: a stream of its own priority level does not share a hardware
        // queue with side2, whose band pass otherwise waited behind the large-footprint tiles --
        // C4 multi-band launch 1.345-1.352 -> 1.315-1.317 ms same box, round 5)
        HIP_TRY(A->hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, least));
    }
    if (mb && !p->side2) {
        HIP_TRY(A->hipEventCreateWithFlags(&p->ev_join2, hipEventDisableTiming));
        HIP_TRY(A->hipEventCreateWithFlags(&p->ev_early, hipEventDisableTiming));
        HIP_TRY(A->hipStreamCreateWithFlags(&p->side2, hipStreamNonBlocking));
    }
    return MCS_OK;
}

// cv2.resize(INTER_LINEAR) of n_frames device images (same size: OpenCV copies).
int launch_resize(const Api *A, const Kernels *k, const uint8_t *src, int sw, int sh,
                  int64_t src_pitch, int64_t src_fstride, uint8_t *dst, int dw, int dh,
                  int64_t dst_pitch, int64_t dst_fstride, int C, int n_frames, hipStream_t s)
{
    if (sw == dw && sh == dh) {
        for (int f = 0; f < n_frames; f++)
            HIP_TRY(A->hipMemcpy2DAsync(dst + f * dst_fstride, (size_t)dst_pitch,
                                        src + f * src_fstride, (size_t)src_pitch, (size_t)dw * C,
                                        dh, hipMemcpyDeviceToDevice, s));
        return MCS_OK;
    }
    mcs::KResizeArgs a;
    a.src = src;
    a.dst = dst;
    a.src_pitch = src_pitch;
    a.src_fstride = src_fstride;
    a.dst_pitch = dst_pitch;
    a.dst_fstride = dst_fstride;
    a.scale_x = 1. / ((double)dw / sw);
    a.scale_y = 1. / ((double)dh / sh);
    a.sw = sw;
    a.sh = sh;
    a.dw = dw;
    a.dh = dh;
    a.n_frames = n_frames;
    a.area2x = a.scale_x == 2. && a.scale_y == 2.;
    return launch_args(A, k->resize[C], (dw + mcs::kResizeBlock - 1) / mcs::kResizeBlock, dh,
                       mcs::kResizeBlock, 1, &a, sizeof(a), s, n_frames);
}

bool gains_active(const mcs_plan *p)
{
    if (!p->gains_on) return false;
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    for (int i = 0; i < p->fd.n_cams; i++)
        if (need[i] && p->gain_q[i] != 256) return true;
    return false;
}

void fill_gain_q(const mcs_plan *p, mcs::KParams *kp)
{
    for (int i = 0; i < MCS_MAX_CAMS; i++)
        kp->gain_q[i] = p->gains_on && i < p->fd.n_cams ? p->gain_q[i] : (uint16_t)256;
}

// All five for every caller.  A call's KParams starts as a copy of p->kp, taken before
// upload_plan_tables / prepare ran for it, and those set cyl_tab, map_tab, lens_tab and (sweep
// plans) skip on first use; seam_hint changes only in mcs_plan_find_seams.  A pointer that the
// call's path left alone is copied onto an equal one: no caller keeps a list of its own.
// (launch_stitch below still copies its four by hand.)
void plan_table_pointers(const mcs_plan *p, mcs::KParams *P)
{
    P->cyl_tab = p->kp.cyl_tab;
    P->map_tab = p->kp.map_tab;
    P->lens_tab = p->kp.lens_tab;
    P->seam_hint = p->kp.seam_hint;
    P->skip = p->kp.skip;
}

int launch_stitch(const Api *A, mcs_plan *p, const mcs::KParams &kp, int n_frames, hipStream_t s,
                  bool gained)
{
    if (kp.out_w <= 0 || kp.out_h <= 0 || n_frames <= 0) return MCS_OK;
    const Kernels *k = nullptr;
    int rc = kernels(A, p, &k);
    if (rc) return rc;
    rc = prepare(A, p, s);
    if (rc) return rc;
    rc = ensure_side(A, p);
    if (rc) return rc;
    // the kernels walk the batch with one frame stride for every camera: split otherwise
    bool uniform = true;
    for (int j = 0; j < p->fd.n_stages; j++)
        uniform = uniform && kp.cam_fstride[p->fd.st[j].cam] == kp.cam_fstride[0];
    mcs::KParams P = kp;
    P.cyl_tab = p->kp.cyl_tab;   // set by prepare on a cylindrical plan's first use
    P.map_tab = p->kp.map_tab;   // (table plans)
    P.lens_tab = p->kp.lens_tab; // (lensed plans)
    P.skip = p->kp.skip;         // (multi-band sweep plans: set by prepare)
    if (gained) {
        // (the sweep kernel has no _g twin: its pixels would come out ungained)
        if (p->t.n_strips > 0)
            return mcs::fail(MCS_E_UNSUPPORTED,
                             "the plan's multi-band tables were prepared for the sweep "
                             "(MCS_MB_SWEEP=1), whose kernel has no fused-gain variant: apply the "
                             "gains with mcs_gain_apply_device, or prepare without the sweep");
        fill_gain_q(p, &P);     // by value in every launch's arguments: the gains as of this call
    }
    if (uniform) return launch_pair(A, p, k, P, n_frames, s, gained);
    for (int f = 0; f < n_frames; f++) {
        for (int i = 0; i < p->fd.n_cams; i++)
            P.cams[i] = kp.cams[i] ? kp.cams[i] + (int64_t)f * kp.cam_fstride[i] : nullptr;
        P.out = kp.out + (int64_t)f * kp.out_fstride;
        rc = launch_pair(A, p, k, P, 1, s, gained);
        if (rc) return rc;
    }
    return MCS_OK;
}

}  // namespace host
}  // namespace mcs

// Test hook (not in mcs.h): force the 64-bit-address kernel variants.
extern "C" void mcs__force_off64(int on) { mcs::host::g_force_off64 = on; }
