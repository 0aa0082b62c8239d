// mcs_prepare.cpp -- what a plan prepares once: the kernel lookup per device, the plan-lifetime
// uploads (cylinder table, map, lens rows) and the prepared tables (mcs_plan::Tables) of the
// stitch, blend and multi-band band-pass kernels.  The sweep's tables: mcs_sweep_host.cpp.
#include <algorithm>
#include <cstdio>
#include <mutex>
#include <vector>

#include "mcs_common.h"
#include "mcs_plan_state.h"

namespace mcs {
namespace host {

static Kernels g_k[kMaxDevices][2];   // [device][fisheye build]
static std::mutex g_k_mu;

static int kernels_of(const Api *A, int device, bool fish, const Kernels **out)
{
    if (device < 0 || device >= kMaxDevices) return mcs::fail(MCS_E_INVALID, "device %d", device);
    std::lock_guard<std::mutex> lk(g_k_mu);
    Kernels &k = g_k[device][fish ? 1 : 0];
    const mcs::Module m_stitch = fish ? mcs::kModStitchFish : mcs::kModStitch;
    const mcs::Module m_sweep = fish ? mcs::kModSweepFish : mcs::kModSweep;
    const mcs::Module m_direct_mb = fish ? mcs::kModDirectMbFish : mcs::kModDirectMb;
    if (!k.loaded) {
        auto fn = [&](const char *name, hipFunction_t *f) {
            return mcs::module_function(A, device, m_stitch, name, f);
        };
        char name[64];
        int rc = MCS_OK;
        for (int c = 1; c <= 4 && rc == MCS_OK; c++) {
            snprintf(name, sizeof(name), "mcs_stream_c%d", c);
            rc = fn(name, &k.stream[c][0]);
            snprintf(name, sizeof(name), "mcs_stream_c%d_b32", c);
            if (rc == MCS_OK) rc = fn(name, &k.stream[c][1]);
            snprintf(name, sizeof(name), "mcs_stream_big_c%d", c);
            if (rc == MCS_OK) rc = fn(name, &k.stream_big[c][0]);
            snprintf(name, sizeof(name), "mcs_stream_big_c%d_b32", c);
            if (rc == MCS_OK) rc = fn(name, &k.stream_big[c][1]);
            for (int b = 0; b < 2; b++) {   // the fused-gain twins
                snprintf(name, sizeof(name), "mcs_stream_c%d%s_g", c, b ? "_b32" : "");
                if (rc == MCS_OK) rc = fn(name, &k.stream_g[c][b]);
                snprintf(name, sizeof(name), "mcs_stream_big_c%d%s_g", c, b ? "_b32" : "");
                if (rc == MCS_OK) rc = fn(name, &k.stream_big_g[c][b]);
            }
            snprintf(name, sizeof(name), "mcs_mb_levels_c%d_g", c);
            if (rc == MCS_OK) rc = fn(name, &k.mb_levels_g[c]);
            snprintf(name, sizeof(name), "mcs_resize_c%d", c);
            if (rc == MCS_OK) rc = fn(name, &k.resize[c]);
            snprintf(name, sizeof(name), "mcs_mb_levels_c%d", c);
            if (rc == MCS_OK) rc = fn(name, &k.mb_levels[c]);
            for (int al = 0; al < 2; al++) {
                const char *sfx = al ? "_a" : "";
                snprintf(name, sizeof(name), "mcs_mb_bands%s_c%d", sfx, c);
                if (rc == MCS_OK) rc = fn(name, &k.mb_bands[c][al][0]);
                snprintf(name, sizeof(name), "mcs_mb_bands_br%s_c%d", sfx, c);
                if (rc == MCS_OK) rc = fn(name, &k.mb_bands[c][al][1]);
                snprintf(name, sizeof(name), "mcs_mb_bands_all%s_c%d", sfx, c);
                if (rc == MCS_OK) rc = fn(name, &k.mb_bands[c][al][2]);
                snprintf(name, sizeof(name), "mcs_mb_bands%s_c%d_g", sfx, c);
                if (rc == MCS_OK) rc = fn(name, &k.mb_bands_g[c][al][0]);
                snprintf(name, sizeof(name), "mcs_mb_bands_br%s_c%d_g", sfx, c);
                if (rc == MCS_OK) rc = fn(name, &k.mb_bands_g[c][al][1]);
                snprintf(name, sizeof(name), "mcs_mb_bands_all%s_c%d_g", sfx, c);
                if (rc == MCS_OK) rc = fn(name, &k.mb_bands_g[c][al][2]);
            }
            snprintf(name, sizeof(name), "mcs_mb_blend_c%d_s2", c);
            if (rc == MCS_OK) rc = fn(name, &k.mb_blend[c][0]);
            snprintf(name, sizeof(name), "mcs_mb_blend_c%d_s4", c);
            if (rc == MCS_OK) rc = fn(name, &k.mb_blend[c][1]);
            snprintf(name, sizeof(name), "mcs_mb_blend_c%d_s8", c);
            if (rc == MCS_OK) rc = fn(name, &k.mb_blend[c][2]);
            for (int i = 0; i < 2 && rc == MCS_OK; i++) {
                snprintf(name, sizeof(name), "mcs_prepare_c%d_i%d", c, i);
                rc = fn(name, &k.prepare[c][i]);
                snprintf(name, sizeof(name), "mcs_feather_c%d_i%d", c, i);
                if (rc == MCS_OK) rc = fn(name, &k.feather[c][i]);
                snprintf(name, sizeof(name), "mcs_feather_c%d_i%d_g", c, i);
                if (rc == MCS_OK) rc = fn(name, &k.feather_g[c][i]);
                snprintf(name, sizeof(name), "mcs_mb_prep_c%d_i%d", c, i);
                if (rc == MCS_OK) rc = fn(name, &k.mb_prep[c][i]);
                snprintf(name, sizeof(name), "mcs_mb_bdesc_c%d_i%d", c, i);
                if (rc == MCS_OK) rc = fn(name, &k.mb_bdesc[c][i]);
                snprintf(name, sizeof(name), "mcs_seam_sample_c%d_i%d", c, i);
                if (rc == MCS_OK) rc = fn(name, &k.seam_sample[c][i]);
                snprintf(name, sizeof(name), "mcs_direct_feather_c%d_i%d", c, i);
                if (rc == MCS_OK) rc = fn(name, &k.direct_feather[c][i]);
                snprintf(name, sizeof(name), "mcs_direct_feather_c%d_i%d_g", c, i);
                if (rc == MCS_OK) rc = fn(name, &k.direct_feather_g[c][i]);
                for (int o = 0; o < 2 && rc == MCS_OK; o++) {
                    snprintf(name, sizeof(name), "mcs_direct_c%d_i%d_o%d", c, i, o ? 32 : 64);
                    rc = fn(name, &k.direct[c][i][o]);
                    snprintf(name, sizeof(name), "mcs_direct_c%d_i%d_o%d_g", c, i, o ? 32 : 64);
                    if (rc == MCS_OK) rc = fn(name, &k.direct_g[c][i][o]);
                }
            }
        }
        for (int c = 1; c <= 3 && rc == MCS_OK; c++)
            for (int al = 0; al < 2 && rc == MCS_OK; al++) {
                for (int jb = 0; jb < 2 && rc == MCS_OK; jb++) {
                    snprintf(name, sizeof(name), "mcs_mb_sweep%s_c%d_j%d", al ? "_a" : "", c,
                             jb ? 4 : 2);
                    rc = mcs::module_function(A, device, m_sweep, name,
                                              &k.mb_sweep[c][al][jb]);
                }
                snprintf(name, sizeof(name), "mcs_mb_sweep_desc_c%d_i%d", c, al);
                if (rc == MCS_OK)
                    rc = mcs::module_function(A, device, m_sweep, name,
                                              &k.mb_sweep_desc[c][al]);
            }
        if (rc == MCS_OK) rc = fn("mcs_footprint_i0", &k.footprint[0]);
        if (rc == MCS_OK) rc = fn("mcs_footprint_i1", &k.footprint[1]);
        if (rc == MCS_OK) rc = fn("mcs_blend_owner_i0", &k.blend_owner[0]);
        if (rc == MCS_OK) rc = fn("mcs_blend_owner_i1", &k.blend_owner[1]);
        if (rc == MCS_OK) rc = fn("mcs_blend_classify", &k.blend_classify);
        if (rc == MCS_OK) rc = fn("mcs_overlap_prep_i0", &k.overlap_prep[0]);
        if (rc == MCS_OK) rc = fn("mcs_overlap_prep_i1", &k.overlap_prep[1]);
        for (int c = 1; c <= 4 && rc == MCS_OK; c++) {
            snprintf(name, sizeof(name), "mcs_overlap_sum_c%d", c);
            rc = fn(name, &k.overlap_sum[c]);
        }
        if (rc == MCS_OK) rc = fn("mcs_gain_apply", &k.gain_apply);
        for (int c = 1; c <= 4 && rc == MCS_OK; c++)
            for (int i = 0; i < 2 && rc == MCS_OK; i++) {
                snprintf(name, sizeof(name), "mcs_direct_overlap_c%d_i%d", c, i);
                rc = fn(name, &k.direct_overlap[c][i]);
            }
        for (int g = 0; g < 2 && rc == MCS_OK; g++)
            for (int c = 1; c <= 4 && rc == MCS_OK; c++)
                for (int i = 0; i < 2 && rc == MCS_OK; i++) {
                    snprintf(name, sizeof(name), "mcs_direct_mb_own_c%d_i%d%s", c, i, g ? "_g" : "");
                    rc = mcs::module_function(A, device, m_direct_mb, name,
                                              &k.direct_mb_own[g][c][i]);
                    snprintf(name, sizeof(name), "mcs_direct_mb_tile_c%d_i%d%s", c, i, g ? "_g" : "");
                    if (rc == MCS_OK)
                        rc = mcs::module_function(A, device, m_direct_mb, name,
                                                  &k.direct_mb_tile[g][c][i]);
                }
        if (rc) return rc;
        k.loaded = true;
    }
    *out = &k;
    return MCS_OK;
}

int kernels(const Api *A, int device, const Kernels **out)
{
    return kernels_of(A, device, false, out);
}

int kernels(const Api *A, const mcs_plan *p, const Kernels **out)
{
    return kernels_of(A, p->device, p->fish_mask != 0, out);
}

// Launch list of the streaming kernel for tiles in launch order: stream_tile deals a list to the
// 8 XCDs in equal contiguous slices (XCD x: entries [x * per, (x + 1) * per)), each walked in
// order, so an XCD holds a band of whole tile rows (horizontal neighbours share its L2; measured
// faster than vertical strips, round 3); slices padded to one length with -1.
static std::vector<int> launch_list(const std::vector<int> &tiles)
{
    const size_t n = tiles.size(), per = (n + 7) / 8;
    std::vector<int> out(8 * per, -1);
    for (size_t i = 0; i < n; i++) out[i] = tiles[i];
    return out;
}

// LDS-ring form of the band pass (mb_bands_body mode 2), once per plan: from the device-built
// window descriptors (mb_bdesc) of every band, the band's source rows [y0, y1] (both taps of
// every lane and row), per row the byte span its samples read and the 256-byte window of the row
// staged for it (16-byte aligned, moved back to end inside the frame), the group table (LDS-DMA
// source offsets of rows 4g .. 4g + 3 per lane) and the descriptors rewritten to ring offsets.
// A band takes the ring only when its rows fit the schedule of mb_bands_body: every row's groups
// issued >= kMbLdsGLead rows before it and still resident (rows advancing with the band's rows, at
// most kMbLdsRows in flight); the rest keep the global-window form.
static int band_lds_tables(const Api *A, mcs_plan *p, std::vector<mcs::MbBand> &bands,
                           hipStream_t s)
{
    const size_t nb = bands.size();
    const int C = p->fd.channels, R = mcs::kMbBandRows, DR = mcs::kMbBandDescRows;
    const int L = mcs::kMbBandLanes, NG = mcs::kMbLdsGroups, K = mcs::kMbLdsRows;
    const int SP = mcs::kMbLdsSpan, D4 = mcs::kMbLdsLead / 4;
    p->t.n_bands_lds = 0;
    std::vector<uint64_t> desc(nb * DR * L);
    HIP_TRY(A->hipMemcpyAsync(desc.data(), p->t.d_bdesc, desc.size() * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, s));
    HIP_TRY(A->hipStreamSynchronize(s));
    std::vector<uint32_t> grp(nb * NG * L, 0u);
    const int DL = mcs::kMbLdsDescRows;
    std::vector<uint4> d16(nb * DL * L, make_uint4(0u, 0u, 0u, 0u));
    // row r's loop position at which group g is issued (prologue groups: the kMbLdsDescRing
    // descriptor DMAs of the prologue follow them before row 0)
    auto issue = [&](int g) { return g <= D4 ? -mcs::kMbLdsDescRing : 4 * (g - D4 - 1); };
    for (size_t i = 0; i < nb; i++) {
        const int slot = bands[i].slot;
        const int w = slot == 0 ? p->kp.cam0_w : p->kp.st[slot - 1].src_w;
        const int h = slot == 0 ? p->kp.cam0_h : p->kp.st[slot - 1].src_h;
        const int64_t pitch = (int64_t)w * C, fb = pitch * h;
        if (pitch % 4 || pitch < SP) continue;
        uint64_t *d = desc.data() + i * DR * L;
        int y0 = INT32_MAX, y1 = -1;
        bool ok = true;
        for (int e = 0; e < R * L && ok; e++) {
            const uint32_t dx = (uint32_t)d[e], sh = (uint32_t)(d[e] >> 47) & 15u;
            const int64_t oa = dx & 0x7fffffffu;
            const int ya = (int)(oa / pitch), yb = ya + (int)(dx >> 31);
            ok = sh != 15u && yb < h;
            y0 = std::min(y0, ya);
            y1 = std::max(y1, yb);
        }
        if (!ok || y1 - y0 + 1 > 4 * (NG - 2)) continue;
        const int nr = y1 - y0 + 1;
        std::vector<int64_t> lo(nr, INT64_MAX), hi(nr, -1), bs(nr, 0);
        std::vector<int> glo(R, INT32_MAX), ghi(R, -1);
        for (int r = 0; r < R; r++)
            for (int l = 0; l < L; l++) {
                const uint32_t dx = (uint32_t)d[r * L + l];
                const int64_t oa = dx & 0x7fffffffu, cb = oa % pitch;
                const int ya = (int)(oa / pitch) - y0, yb = ya + (int)(dx >> 31);
                for (int y : {ya, yb}) {
                    lo[y] = std::min(lo[y], cb);
                    hi[y] = std::max(hi[y], cb + 2 * C);
                }
                glo[r] = std::min(glo[r], ya / 4);
                ghi[r] = std::max(ghi[r], yb / 4);
            }
        // staged window of every row: 16-byte aligned at its first byte, moved back so that its
        // 256 bytes end inside the frame (4-byte steps: pitch is a multiple of 4)
        for (int y = 0; y < nr && ok; y++) {
            const int64_t room = fb - (int64_t)(y0 + y) * pitch - SP;
            bs[y] = std::min(hi[y] < 0 ? 0 : lo[y] & ~(int64_t)15, room);
            ok = bs[y] >= 0 && (hi[y] < 0 || hi[y] - bs[y] <= SP);
        }
        if (!ok) continue;
        for (int r = 0; r < R && ok; r++)
            ok = issue(ghi[r]) <= r - mcs::kMbLdsGLead && issue(glo[r] + K / 4) >= r;
        if (!ok) continue;
       
        // group table: lane l loads chunk l % 16 of row 4g + l / 16; chunks no sample of the row
        // reads, rows no sample reads and rows past the band: an offset past the frame (the
        // kernel's buffer load fetches nothing for them)
        uint32_t *gt = grp.data() + i * NG * L;
        for (int g = 0; g < NG; g++)
            for (int l = 0; l < L; l++) {
                const int y = 4 * g + l / 16, c = l % 16;
                const bool need = y < nr && hi[y] >= 0 && 16 * c < hi[y] - bs[y];
                gt[g * L + l] = need ? (uint32_t)((int64_t)(y0 + y) * pitch + bs[y] + 16 * c)
                                     : 0xfffffff0u;
            }
        // descriptors: .x = ring offsets of the tap-a / tap-b windows (4-byte aligned), .y keeps
        // the weights and takes the window shift sh = tap byte & 3.  Rows 0 .. R - 1 only: the
        // descriptor rows past them repeat row R - 1 (read through min(r, R - 1) below), and
        // rewriting them here too would decode row R - 1's already rewritten value as a frame
        // offset and index bs[] far outside its rows
        for (int r = 0; r < R; r++)
            for (int l = 0; l < L; l++) {
                const uint64_t v = d[r * L + l];
                const uint32_t dx = (uint32_t)v, dy = (uint32_t)(v >> 32);
                const int64_t oa = dx & 0x7fffffffu, cb = oa % pitch;
                const int ya = (int)(oa / pitch) - y0, yb = ya + (int)(dx >> 31);
                const uint32_t wa = (uint32_t)((ya % K) * SP + ((cb & ~(int64_t)3) - bs[ya]));
                const uint32_t wb = (uint32_t)((yb % K) * SP + ((cb & ~(int64_t)3) - bs[yb]));
                const uint32_t ny = (dy & ~(15u << 15)) | ((uint32_t)(cb & 3) << 15);
                d[r * L + l] = (uint64_t)(wa | (wb << 16)) | ((uint64_t)ny << 32);
            }
        // the 16-byte descriptors the kernel stages by LDS-DMA: .x = the windows' ring offsets
        // (12 bits each) with the byte shift in bits 14-15, .y / .w = the doubled bilinear
        // weights of rows a / b as u16 pairs (mb_weights2, precomputed here once per plan
        // instead of per row and wave), .z on rows r % 4 == 0 the lane's source offset of the
        // group issued after row r
        for (int r = 0; r < DL; r++)
            for (int l = 0; l < L; l++) {
                const uint64_t v = d[std::min(r, R - 1) * L + l];
                const uint32_t x = (uint32_t)v, meta = (uint32_t)(v >> 32);
                const uint32_t sh = (meta >> 15) & 3u, fx = meta & 63u, fy = (meta >> 6) & 31u;
                const uint32_t ya = (32u - fy) << 6, yb = fy << 6;
                const uint32_t wa = std::min((32u - fx) * ya, 65535u) |
                                    (std::min(fx * ya, 65535u) << 16);
                const uint32_t wb = std::min((32u - fx) * yb, 65535u) |
                                    (std::min(fx * yb, 65535u) << 16);
                const int g = r / 4 + D4 + 1;
                const uint32_t z = (r < R && r % 4 == 0 && g < NG) ? gt[g * L + l] : 0u;
                d16[(i * DL + r) * L + l] = make_uint4(x | (sh << 14), wa, z, wb);
            }
        bands[i].pad_ |= 1;
        p->t.n_bands_lds++;
    }
    if (p->t.n_bands_lds == 0) return MCS_OK;
    HIP_TRY(p->t.alloc(A, &p->t.d_bgrp, grp.size()));
    HIP_TRY(A->hipMemcpyAsync(p->t.d_bgrp, grp.data(), grp.size() * sizeof(uint32_t),
                              hipMemcpyHostToDevice, s));
    // (d_bdesc keeps the frame-offset descriptors: the ring offsets live only in d_bdesc16, so
    // a launch that takes the unaligned form -- band_form() == 0, decided per launch from the
    // frame pointers and strides -- reads valid descriptors for every band)
    HIP_TRY(p->t.alloc(A, &p->t.d_bdesc16, d16.size()));
    HIP_TRY(A->hipMemcpyAsync(p->t.d_bdesc16, d16.data(), d16.size() * sizeof(uint4),
                              hipMemcpyHostToDevice, s));
    HIP_TRY(A->hipMemcpyAsync(p->t.d_bands, bands.data(), nb * sizeof(mcs::MbBand),
                              hipMemcpyHostToDevice, s));
    HIP_TRY(A->hipStreamSynchronize(s));
    return MCS_OK;
}

// The band pass of a multi-band plan (after mb_prep): per (owner slot, blend-tile row) the
// level-1 / level-2 mosaic columns the tiles of that row read from that owner (mb_prep's per-slot
// ranges), merged where they overlap and covered by 64-column windows kMbBandStride apart; then
// the windows' sample descriptors (once).  Mosaics under 128 px a side (a unit would reach past
// two opposite edges) and plans whose camera frames are too small for the 8-byte window loads
// stay with mb_levels.
static int prepare_bands(const Api *A, mcs_plan *p, const Kernels *k, hipStream_t s)
{
    const int n = p->t.n_blend, S = p->t.mb_slots, C = p->fd.channels;
    const int W = p->fd.out_w, H = p->fd.out_h;
    p->t.gxb = (W + mcs::kBlendTileW - 1) / mcs::kBlendTileW;
    const int gyb = (H + mcs::kBlendTileH - 1) / mcs::kBlendTileH;
    const mcs::KParams &P = p->kp;
    for (int c = 0; c <= P.n_stages; c++) {
        if (c == 0 && P.cam0_w == 0) continue;     // (cylindrical plans: no slot-0 camera)
        const int64_t w = c == 0 ? P.cam0_w : P.st[c - 1].src_w;
        const int64_t h = c == 0 ? P.cam0_h : P.st[c - 1].src_h;
        if ((h - 1) * w * C < 16) return MCS_OK;   // (mb_levels' guarded window loads)
    }
    if (W < 128 || H < 128) return MCS_OK;
    std::vector<int> list(1 + 2 * (size_t)n);
    std::vector<int> cnt((size_t)n * mcs::kMbTabCounts);
    const size_t words = (size_t)mcs::mb_tab_words(S);
    const size_t cnt_at = (size_t)S * (mcs::kMbNRX * mcs::kMbNRY + mcs::kMbN2X * mcs::kMbN2Y) +
                          mcs::kMbNRX * mcs::kMbNRY + mcs::kMbN2X * mcs::kMbN2Y;
    HIP_TRY(A->hipMemcpyAsync(list.data(), p->t.d_blist, list.size() * sizeof(int),
                              hipMemcpyDeviceToHost, s));
    HIP_TRY(A->hipMemcpy2DAsync(cnt.data(), mcs::kMbTabCounts * sizeof(int), p->t.d_mbtab + cnt_at,
                                words * sizeof(int), mcs::kMbTabCounts * sizeof(int), (size_t)n,
                                hipMemcpyDeviceToHost, s));
    HIP_TRY(A->hipStreamSynchronize(s));
    // per (plan slot, tile row): the level-1 / level-2 column intervals of its tiles
    struct Need { int q1lo, q1hi, z2lo, z2hi; };
    constexpr int kSlots = 32;   // plan slots: bits of a tile's owner mask
    std::vector<std::vector<Need>> need((size_t)kSlots * gyb);
    std::vector<int> tile_bt((size_t)p->t.gxb * gyb, -1);
    for (int i = 0; i < n; i++) {
        const int t = list[1 + 2 * i];
        const uint32_t mask = (uint32_t)list[2 + 2 * i];
        tile_bt[t] = i;
        const int Y0 = (t / p->t.gxb) * mcs::kBlendTileH;
        const int *c = cnt.data() + (size_t)i * mcs::kMbTabCounts + mcs::kMbTabRanges;
        uint32_t m = mask;
        for (int j = 0; m; j++, m &= m - 1) {
            const int slot = __builtin_ctz(m);
            Need q{c[4 * j], c[4 * j + 1], c[4 * j + 2], c[4 * j + 3]};
            if (q.q1lo > q.q1hi && q.z2lo > q.z2hi) continue;
            need[(size_t)slot * gyb + Y0 / mcs::kBlendTileH].push_back(q);
        }
    }
    // per capture: the blend pixels and R1 entries the blend kernel computes (counted before the
    // band list: a plan whose tiles need no band still blends its mixed pixels)
    p->t.mb_mixed_px = p->t.mb_r1 = 0;
    for (int i = 0; i < n; i++) {
        p->t.mb_mixed_px += cnt[(size_t)i * mcs::kMbTabCounts];
        p->t.mb_r1 += cnt[(size_t)i * mcs::kMbTabCounts + 1];
    }
    std::vector<mcs::MbBand> bands;
    const int big = 1 << 30;
    for (int slot = 0; slot < kSlots; slot++)
        for (int row = 0; row < gyb; row++) {
            std::vector<Need> &v = need[(size_t)slot * gyb + row];
            if (v.empty()) continue;
            // (a column interval in level-0 terms: its lowest needed level-0 column)
            auto lo0 = [&](const Need &q) {
                return std::min(q.z2lo <= q.z2hi ? 4 * q.z2lo : big,
                                q.q1lo <= q.q1hi ? 2 * q.q1lo : big);
            };
            std::sort(v.begin(), v.end(), [&](const Need &a, const Need &b) {
                return lo0(a) < lo0(b);
            });
            size_t i = 0;
            while (i < v.size()) {
                Need u = v[i++];
                auto hi0 = [&](const Need &q) {
                    return std::max(q.z2lo <= q.z2hi ? 4 * q.z2hi : -big,
                                    q.q1lo <= q.q1hi ? 2 * q.q1hi : -big);
                };
                // merge intervals that overlap or nearly touch (one window covers the gap)
                while (i < v.size() && lo0(v[i]) <= hi0(u) + 2 * mcs::kMbBandStride) {
                    const Need &q = v[i++];
                    if (q.q1lo <= q.q1hi)
                        u.q1lo = std::min(u.q1lo, q.q1lo), u.q1hi = std::max(u.q1hi, q.q1hi);
                    if (q.z2lo <= q.z2hi)
                        u.z2lo = std::min(u.z2lo, q.z2lo), u.z2hi = std::max(u.z2hi, q.z2hi);
                }
                // windows: c0 emits level-1 columns [c0/2 + 1, c0/2 + 30] and level-2 columns
                // [c0/4 + 2, c0/4 + 14] (mb_bands' complete lanes)
                int c0 = std::min(u.z2lo <= u.z2hi ? 4 * (u.z2lo - 2) : big,
                                  u.q1lo <= u.q1hi ? 2 * (u.q1lo - 1) : big);
                c0 = c0 >= 0 ? c0 & ~3 : -((-c0 + 3) & ~3);
                for (;;) {
                    bands.push_back(mcs::MbBand{slot, row, c0, 0});
                    const bool z_ok = u.z2lo > u.z2hi || c0 / 4 + 14 >= u.z2hi;
                    const bool q_ok = u.q1lo > u.q1hi || c0 / 2 + 30 >= u.q1hi;
                    if (z_ok && q_ok) break;
                    c0 += mcs::kMbBandStride;
                }
            }
        }
    if (bands.empty()) return MCS_OK;
    {
        // streaming tiles under the blend tiles that have mixed pixels: launched first, so the
        // blend (which overwrites those pixels) can run beside the other streaming tiles
        std::vector<char> early((size_t)p->gx * p->gy, 0);
        for (int i = 0; i < n; i++) {
            if (cnt[(size_t)i * mcs::kMbTabCounts] == 0) continue;
            const int t = list[1 + 2 * i];
            const int X0 = (t % p->t.gxb) * mcs::kBlendTileW;
            const int Y0 = (t / p->t.gxb) * mcs::kBlendTileH;
            const int x1 = std::min(X0 + mcs::kBlendTileW, W) - 1;
            const int y1 = std::min(Y0 + mcs::kBlendTileH, H) - 1;
            for (int ty = Y0 / mcs::kTileH; ty <= y1 / mcs::kTileH; ty++)
                for (int tx = X0 / mcs::kTileW; tx <= x1 / mcs::kTileW; tx++)
                    early[(size_t)ty * p->gx + tx] = 1;
        }
        std::vector<int> first, late;
        for (size_t t = 0; t < early.size(); t++)
            (early[t] ? first : late).push_back((int)t);
        std::vector<int> order = launch_list(first);
        p->t.n_early = (int)order.size();
        const std::vector<int> rest = launch_list(late);
        order.insert(order.end(), rest.begin(), rest.end());
        p->t.n_list = (int)order.size();
        p->t.drop(A, &p->t.d_order);
        HIP_TRY(p->t.alloc(A, &p->t.d_order, order.size()));
        HIP_TRY(A->hipMemcpyAsync(p->t.d_order, order.data(), order.size() * sizeof(int),
                                  hipMemcpyHostToDevice, s));
    }
    // bands whose rows or columns reach past the bottom / right mosaic edge: the _br kernel
    auto br = [&](const mcs::MbBand &b) {
        return b.row * mcs::kBlendTileH - mcs::kBlendHalo + mcs::kMbFirst + mcs::kMbUsedY > H ||
               b.c0 + mcs::kMbBandLanes > W;
    };
    std::stable_sort(bands.begin(), bands.end(),
                     [](const mcs::MbBand &a, const mcs::MbBand &b) { return a.row < b.row; });
    std::stable_partition(bands.begin(), bands.end(), [&](const mcs::MbBand &b) { return !br(b); });
    p->t.n_bands_in = (int)(std::find_if(bands.begin(), bands.end(), br) - bands.begin());
    const size_t nb = bands.size();
    HIP_TRY(p->t.alloc(A, &p->t.d_bands, nb));
    HIP_TRY(p->t.alloc(A, &p->t.d_tile_bt, tile_bt.size()));
    HIP_TRY(p->t.alloc(A, &p->t.d_bdesc, nb * mcs::kMbBandDescRows * mcs::kMbBandLanes));
    HIP_TRY(A->hipMemcpyAsync(p->t.d_bands, bands.data(), nb * sizeof(mcs::MbBand),
                              hipMemcpyHostToDevice, s));
    HIP_TRY(A->hipMemcpyAsync(p->t.d_tile_bt, tile_bt.data(), tile_bt.size() * sizeof(int),
                              hipMemcpyHostToDevice, s));
    p->t.n_bands = (int)nb;
    mcs::KMbBandArgs a;
    band_args(p, p->kp, a);
    int rc = launch_args(A, k->mb_bdesc[C][p->fd.interp], (unsigned)nb, 1, 256, 1, &a, sizeof(a),
                         s);
    if (rc) return rc;
    rc = band_lds_tables(A, p, bands, s);
    if (rc) return rc;
    // the band pass writes only the entries the blend reads: the rest of the scratch holds
    // zeros (or an earlier capture's value of the same entry), never stale garbage
    const size_t slots = (size_t)n * S * p->t.mb_chunk;
    HIP_TRY(A->hipMemsetAsync(p->t.d_mbg1, 0, slots * mcs::kMbNRX * mcs::kMbNRY * 8, s));
    HIP_TRY(A->hipMemsetAsync(p->t.d_mbg2, 0, slots * mcs::kMbN2X * mcs::kMbN2Y * C * 4, s));
    HIP_TRY(A->hipStreamSynchronize(s));
    return MCS_OK;
}

// Multi-band: per (tile, owner) level-0 sample windows and per-tile masks (once), and the level
// scratch for chunks of mb_chunk captures (budget kMbScratchBytes).
static int prepare_multiband(const Api *A, mcs_plan *p, const Kernels *k, hipStream_t s)
{
    const int n = p->t.n_blend, S = p->t.mb_slots, C = p->fd.channels;
    const mcs::KParams &P = p->kp;
    for (int c = 0; c <= P.n_stages; c++) {
        const int64_t w = c == 0 ? P.cam0_w : P.st[c - 1].src_w;
        const int64_t h = c == 0 ? P.cam0_h : P.st[c - 1].src_h;
        if (w * h * C >= (int64_t(1) << 31))
            return mcs::fail(MCS_E_UNSUPPORTED, "multi-band: camera frames must be < 2 GiB");
    }
    const int64_t per_f = (int64_t)n * S * (mcs::kMbNRX * mcs::kMbNRY * 8 +
                                            mcs::kMbN2X * mcs::kMbN2Y * C * 4);
    int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(64, mcs::kMbScratchBytes / per_f));
    if (chunk > mcs::kMbLvFrames) chunk -= chunk % mcs::kMbLvFrames;
    const int64_t samples = (int64_t)mcs::kMbUsedX * mcs::kMbUsedY;
    HIP_TRY(p->t.alloc(A, &p->t.d_mbdesc, (size_t)(n * S * samples)));
    HIP_TRY(p->t.alloc(A, &p->t.d_mbtab, (size_t)n * mcs::mb_tab_words(S)));
    HIP_TRY(p->t.alloc(A, &p->t.d_mbfoot, (size_t)n * S * 8));
    HIP_TRY(p->t.alloc(A, &p->t.d_mbrec, (size_t)n * mcs::mb_rec_words(S)));
    // (level 1: 8 bytes an entry, level 2: C int32 an entry)
    HIP_TRY(p->t.alloc(A, &p->t.d_mbg1, (size_t)n * S * chunk * mcs::kMbNRX * mcs::kMbNRY * 4));
    HIP_TRY(p->t.alloc(A, &p->t.d_mbg2, (size_t)n * S * chunk * mcs::kMbN2X * mcs::kMbN2Y * C));
    p->t.mb_chunk = chunk;
    mcs::KMbArgs a;
    mb_args(p, p->kp, a);
    int rc = launch_args(A, k->mb_prep[C][p->fd.interp], (unsigned)n, 1,
                         mcs::kMbPrepThreads, 1, &a, sizeof(a), s);
    if (rc) return rc;
    rc = prepare_sweep(A, p, k, s);
    if (rc || p->t.n_strips > 0) return rc;
    return prepare_bands(A, p, k, s);
}

// Blended modes: the owner map and the list of 32-px tiles the blend kernels recompute.
static int prepare_blend(const Api *A, mcs_plan *p, const Kernels *k, hipStream_t s)
{
    const int W = p->fd.out_w, H = p->fd.out_h;
    const int bx = (W + mcs::kBlendTileW - 1) / mcs::kBlendTileW;
    const int by = (H + mcs::kBlendTileH - 1) / mcs::kBlendTileH;
    const size_t nt = (size_t)bx * by;
    HIP_TRY(p->t.alloc(A, &p->t.d_owner, (size_t)W * H));
    HIP_TRY(p->t.alloc(A, &p->t.d_binfo, nt * 2));
    HIP_TRY(p->t.alloc(A, &p->t.d_blist, 4 * nt + 4));
    HIP_TRY(A->hipMemsetAsync(p->t.d_blist, 0, (4 * nt + 4) * sizeof(int), s));
    mcs::KBlendPrepArgs a;
    a.P = p->kp;
    a.owner = p->t.d_owner;
    a.info = p->t.d_binfo;
    a.list = p->t.d_blist;
    a.overflow = p->t.d_blist + 2 * nt + 1;
    a.list2 = p->t.d_blist + 2 * nt + 3;
    a.mode = p->blend;
    a.pad_ = 0;
    int rc = launch_args(A, k->blend_owner[p->fd.interp], bx, by, 256, 1, &a, sizeof(a), s);
    if (rc == MCS_OK) rc = launch_args(A, k->blend_classify, (unsigned)nt, 1, 256, 1, &a,
                                       sizeof(a), s);
    if (rc) return rc;
    int n = 0, tail[3] = {0, 0, 0};
    HIP_TRY(A->hipMemcpyAsync(&n, p->t.d_blist, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(A->hipMemcpyAsync(tail, p->t.d_blist + 2 * nt + 1, 3 * sizeof(int),
                              hipMemcpyDeviceToHost, s));
    HIP_TRY(A->hipStreamSynchronize(s));
    // tail[0]: multi-band tiles with more than kBlendSlots owners (degraded to the feather rule),
    // tail[2]: those of them with pixels to feather (listed in d_dense)
    if (n > 1) {
        // the list in tile order (classify appends in arrival order)
        std::vector<int> l(1 + 2 * (size_t)n);
        HIP_TRY(A->hipMemcpyAsync(l.data(), p->t.d_blist, l.size() * sizeof(int),
                                  hipMemcpyDeviceToHost, s));
        HIP_TRY(A->hipStreamSynchronize(s));
        std::vector<std::pair<int, int>> e((size_t)n);
        for (int i = 0; i < n; i++) e[i] = {l[1 + 2 * i], l[2 + 2 * i]};
        std::sort(e.begin(), e.end());
        for (int i = 0; i < n; i++) l[1 + 2 * i] = e[i].first, l[2 + 2 * i] = e[i].second;
        HIP_TRY(A->hipMemcpyAsync(p->t.d_blist, l.data(), l.size() * sizeof(int),
                                  hipMemcpyHostToDevice, s));
        HIP_TRY(A->hipStreamSynchronize(s));
    }
    p->t.mb_slots = tail[1];
    p->t.n_degraded = p->blend == MCS_BLEND_MULTIBAND ? tail[0] : 0;
    p->t.n_dense = tail[2];
    p->t.d_dense = p->t.d_blist + 2 * nt + 3;
    p->t.n_blend = n;
    if (p->blend == MCS_BLEND_MULTIBAND && n > 0) return prepare_multiband(A, p, k, s);
    return MCS_OK;
}

void release_tables(const Api *A, mcs_plan *p)
{
    if (p->stream) (void)A->hipStreamSynchronize(p->stream);
    if (p->side) (void)A->hipStreamSynchronize(p->side);
    if (p->side2) (void)A->hipStreamSynchronize(p->side2);
    for (void *q : p->t.owned) (void)A->hipFree(q);
    p->t = mcs_plan::Tables{};
    p->kp.skip = nullptr;
}

// Cylindrical plans: the per-column / per-row table on the plan's device (once); table plans:
// their map; lensed plans: the lens rows (again after every mcs_plan_set_lens).
int upload_plan_tables(const Api *A, mcs_plan *p, hipStream_t s)
{
    if (p->kp.lens_mask && (!p->d_lens || p->lens_stale)) {
        if (!p->d_lens) HIP_TRY(A->hipMalloc((void **)&p->d_lens, sizeof(p->lens)));
        HIP_TRY(A->hipMemcpyAsync(p->d_lens, p->lens, sizeof(p->lens), hipMemcpyHostToDevice, s));
        HIP_TRY(A->hipStreamSynchronize(s));
        p->lens_stale = false;
        p->kp.lens_tab = p->d_lens;
    }
    if (!p->map_tab.empty() && !p->d_map) {
        const size_t bytes = p->map_tab.size() * sizeof(int32_t);
        HIP_TRY(A->hipMalloc((void **)&p->d_map, bytes));
        HIP_TRY(A->hipMemcpyAsync(p->d_map, p->map_tab.data(), bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(A->hipStreamSynchronize(s));
        p->kp.map_tab = p->d_map;
    }
    if (!p->cyl || p->d_cyl) return MCS_OK;
    const size_t bytes = p->cyl_tab.size() * sizeof(double);
    HIP_TRY(A->hipMalloc((void **)&p->d_cyl, bytes));
    HIP_TRY(A->hipMemcpyAsync(p->d_cyl, p->cyl_tab.data(), bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(A->hipStreamSynchronize(s));
    p->kp.cyl_tab = p->d_cyl;
    return MCS_OK;
}

// Prepared tables of a plan: one prepare launch, then the fallback-tile count is read back.
static int build_tables(const Api *A, mcs_plan *p, hipStream_t s)
{
    const Kernels *k = nullptr;
    int rc = kernels(A, p, &k);
    if (rc) return rc;
    p->gx = (p->fd.out_w + mcs::kTileW - 1) / mcs::kTileW;
    p->gy = (p->fd.out_h + mcs::kTileH - 1) / mcs::kTileH;
    const size_t tiles = (size_t)p->gx * p->gy;
    if (tiles == 0) {
        p->t.prepared = true;
        return MCS_OK;
    }
    rc = upload_plan_tables(A, p, s);
    if (rc) return rc;
    if (p->blend == MCS_BLEND_FEATHER || p->blend == MCS_BLEND_MULTIBAND) {
        rc = prepare_blend(A, p, k, s);
        if (rc) return rc;
    }
    HIP_TRY(p->t.alloc(A, &p->t.d_tiles, tiles));
    HIP_TRY(p->t.alloc(A, &p->t.d_desc, tiles * mcs::kTilePx * mcs::kDescWords));
    HIP_TRY(p->t.alloc(A, &p->t.d_desc4, tiles * mcs::kTilePx));
    HIP_TRY(p->t.alloc(A, &p->t.d_spans, tiles * mcs::kMaxTileJobs));
    HIP_TRY(p->t.alloc(A, &p->t.d_fallback, 2 * (tiles + 1)));
    p->t.d_big = p->t.d_fallback + tiles + 1;
    HIP_TRY(A->hipMemsetAsync(p->t.d_fallback, 0, sizeof(int), s));
    HIP_TRY(A->hipMemsetAsync(p->t.d_big, 0, sizeof(int), s));
    mcs::KPrepareArgs args;
    args.P = p->kp;
    args.tiles = p->t.d_tiles;
    args.desc = p->t.d_desc;
    args.desc4 = p->t.d_desc4;
    args.fallback = p->t.d_fallback;
    args.big = p->t.d_big;
    args.spans = p->t.d_spans;
    rc = launch_args(A, k->prepare[p->fd.channels][p->fd.interp], p->gx, p->gy, mcs::kWave,
                     mcs::kWavesPerBlock, &args, sizeof(args), s);
    if (rc) return rc;
    int nf = 0, nb = 0;
    HIP_TRY(A->hipMemcpyAsync(&nf, p->t.d_fallback, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(A->hipMemcpyAsync(&nb, p->t.d_big, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(A->hipStreamSynchronize(s));
    p->t.n_fallback = nf;
    p->t.n_big = nb;
    {
        // the streaming launch's read volume per capture, from the tables just built (once)
        std::vector<mcs::TileHdr> th(tiles);
        std::vector<uint16_t> sp(tiles * mcs::kMaxTileJobs);
        HIP_TRY(A->hipMemcpyAsync(th.data(), p->t.d_tiles, tiles * sizeof(mcs::TileHdr),
                                  hipMemcpyDeviceToHost, s));
        HIP_TRY(A->hipMemcpyAsync(sp.data(), p->t.d_spans, sp.size() * sizeof(uint16_t),
                                  hipMemcpyDeviceToHost, s));
        HIP_TRY(A->hipStreamSynchronize(s));
        p->t.dma_bytes = p->t.box_bytes = 0;
        for (size_t t = 0; t < tiles; t++) {
            const mcs::TileHdr &h = th[t];
            if (h.fits == 0) continue;
            for (int k = 0; k < h.ncam; k++) {
                const int rows = h.jobstart[k + 1] - h.jobstart[k];
                p->t.box_bytes += (int64_t)rows * 16 * ((h.stride[k] >> 16) & 0xff);
            }
            for (int j = 0; j < h.njobs && j < mcs::kMaxTileJobs; j++)
                p->t.dma_bytes += 16 * (int64_t)((sp[t * mcs::kMaxTileJobs + j] >> 8) & 0xff);
        }
    }
    if (!p->t.d_order) {
        // one launch list of every tile (the multi-band split builds its own, early tiles first)
        std::vector<int> tl(tiles);
        for (size_t t = 0; t < tiles; t++) tl[t] = (int)t;
        const std::vector<int> order = launch_list(tl);
        HIP_TRY(p->t.alloc(A, &p->t.d_order, order.size()));
        HIP_TRY(A->hipMemcpyAsync(p->t.d_order, order.data(), order.size() * sizeof(int),
                                  hipMemcpyHostToDevice, s));
        HIP_TRY(A->hipStreamSynchronize(s));
        p->t.n_early = 0;
        p->t.n_list = (int)order.size();
    }
    p->t.prepared = true;
    return MCS_OK;
}

int prepare(const Api *A, mcs_plan *p, hipStream_t s)
{
    if (p->t.prepared) return MCS_OK;
    const int rc = build_tables(A, p, s);
    if (rc) {
        // nothing half-built stays behind: the next call starts from a fresh Tables
        (void)A->hipStreamSynchronize(s);
        release_tables(A, p);
    }
    return rc;
}

}  // namespace host
}  // namespace mcs
