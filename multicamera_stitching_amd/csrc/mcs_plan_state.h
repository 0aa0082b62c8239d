// mcs_plan_state.h -- the plan behind the C ABI's mcs_plan handle, and the host functions that
// build its tables (mcs_prepare.cpp, mcs_sweep_host.cpp) and schedule its launches
// (mcs_launch.cpp) for the entry points (mcs_capi.cpp, mcs_stitch.cpp, mcs_seam.cpp).  Host only.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hip_rt.h"
#include "mcs.h"
#include "mcs_kparams.h"
#include "mcs_lens_core.h"

struct mcs_plan {
    // What prepare() builds, once per plan state (blend mode, lenses, seams); release_tables()
    // frees it and puts a fresh Tables in its place.  Device memory allocated through alloc() is
    // owned (freed by release_tables or drop); d_big and d_dense point into another table's
    // allocation.  A fresh Tables holds no host memory either.
    struct Tables {
        std::vector<void *> owned;
        bool prepared = false;
        // tile headers, per-pixel LDS descriptors, fallback list
        int n_fallback = 0;
        int n_big = 0;                    // large-footprint tiles (mcs_stream_big, listed in d_big)
        int *d_big = nullptr;             // (the second half of d_fallback's allocation)
        mcs::TileHdr *d_tiles = nullptr;
        uint32_t *d_desc = nullptr;
        uint32_t *d_desc4 = nullptr;      // compact per-pixel words (the streaming kernel's)
        uint16_t *d_spans = nullptr;      // per tile footprint row: the chunks its windows read
        int *d_fallback = nullptr;
        // the streaming kernel's launch list; multi-band: the tiles under mixed blend pixels run
        // first (d_order[0, n_early)), then the blend starts on side2 beside the rest
        int *d_order = nullptr;
        int n_early = 0;              // launch-list items of the early launch (multi-band split)
        int n_list = 0;               // items of the whole list (d_order; 0: none, grid order)
        // blended modes (mcs_plan_set_blend): owner map, 32-px tile info, per-frame tile list
        int n_blend = 0, mb_slots = 0;
        // multi-band: tiles degraded to the feather rule (d_blist + 2 * blend tiles + 3: count,
        // then (tile, feather mask) pairs)
        int n_dense = 0, n_degraded = 0;
        int *d_dense = nullptr;
        uint8_t *d_owner = nullptr;
        uint32_t *d_binfo = nullptr;
        int *d_blist = nullptr;
        // multi-band: per (tile, owner) sample windows, per-tile masks, level scratch per chunk
        uint64_t *d_mbdesc = nullptr;
        int32_t *d_mbtab = nullptr;
        int32_t *d_mbfoot = nullptr;
        uint32_t *d_mbrec = nullptr;   // blend work records (mcs_kparams.h, mb_rec_words)
        uint16_t *d_mbg1 = nullptr;
        int32_t *d_mbg2 = nullptr;
        int mb_chunk = 0;
        // multi-band band pass: bands (the first n_bands_in reach no bottom / right mosaic edge),
        // blend-tile grid -> list index, descriptors; without bands mb_levels computes the levels
        int n_bands = 0, n_bands_in = 0, gxb = 0;
        mcs::MbBand *d_bands = nullptr;
        int *d_tile_bt = nullptr;
        uint64_t *d_bdesc = nullptr;
        uint32_t *d_bgrp = nullptr;    // LDS-ring band pass: group source offsets (band_lds_tables)
        uint4 *d_bdesc16 = nullptr;    // LDS-ring band pass: descriptors + group offsets per row
        int n_bands_lds = 0;
        int64_t mb_mixed_px = 0, mb_r1 = 0;   // per capture: blend pixels computed, R1 entries
        // multi-band sweep (mcs_sweep.hip, prepare_sweep): strips, their output regions (one int
        // per output row), window descriptors, the per-pixel skip map of the stitch kernels
        // (mirrored in kp.skip); n_strips = 0: the band pass + blend kernels instead
        int n_strips = 0, sw_jb = 0;
        mcs::MbStrip *d_strips = nullptr;
        int *d_region = nullptr;
        uint64_t *d_sdesc = nullptr;
        uint8_t *d_skip = nullptr;
        int64_t sw_px = 0, sw_desc_rows = 0;   // per capture: pixels written; descriptor rows
        // per capture, streaming tiles: bytes the footprint DMAs read (row spans, 16-byte chunks)
        // and the bytes of the footprint boxes (every row at its camera's full box width)
        int64_t dma_bytes = 0, box_bytes = 0;

        // Device memory for `count` elements at *ptr, owned by these tables.
        template <class T>
        hipError_t alloc(const mcs::rt::Api *A, T **ptr, size_t count)
        {
            void *q = nullptr;
            const hipError_t e = A->hipMalloc(&q, count * sizeof(T));
            if (e != hipSuccess) return e;
            owned.push_back(q);
            *ptr = static_cast<T *>(q);
            return hipSuccess;
        }
        // Frees one owned table ahead of release_tables and nulls its pointer.
        template <class T>
        void drop(const mcs::rt::Api *A, T **ptr)
        {
            const auto it = std::find(owned.begin(), owned.end(), static_cast<void *>(*ptr));
            if (it != owned.end()) {
                (void)A->hipFree(*it);
                owned.erase(it);
            }
            *ptr = nullptr;
        }
    };

    mcs_flat_desc fd;
    mcs::KParams kp;
    int device = 0;
    hipStream_t stream = nullptr;
    // device buffers for the host-array path (allocated on first use)
    uint8_t *d_cams[MCS_MAX_CAMS] = {};
    uint8_t *d_out = nullptr;
    int64_t out_pitch = 0;
    // prepared tables (mcs_plan_prepare); gx, gy: the streaming tile grid they were built for
    Tables t;
    int gx = 0, gy = 0;
    // side stream for the direct-gather tiles, forked from / joined to the caller's stream
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // second side stream: the multi-band level pyramids (concurrent with both of the above)
    hipStream_t side2 = nullptr;
    hipEvent_t ev_join2 = nullptr;
    // multi-band split: the early streaming tiles are done (the blend on side2 waits for it)
    hipEvent_t ev_early = nullptr;
    // host path with frames off their calibrated size: upload buffers for the resize pre-pass
    uint8_t *d_raw[MCS_MAX_CAMS] = {};
    size_t raw_bytes[MCS_MAX_CAMS] = {};
    int blend = MCS_BLEND_NONE;
    // cylindrical plans: per-column (sin, cos) and per-row h, host copy and device table
    bool cyl = false;
    std::vector<double> cyl_tab;
    double *d_cyl = nullptr;
    // graph-cut seam labels (mcs_plan_find_seams): host copy and device grid
    std::vector<uint8_t> seam_lab;
    int seam_w = 0, seam_h = 0, seam_k = 0;
    // device max-flow: pairs, push / relabel launches, global relabels, microseconds
    int64_t seam_stats[5] = {0, 0, 0, 0, 0};
    uint8_t *d_seam = nullptr;
    // single-camera remap plans (warp / undistort): blend modes refused; table plans' map
    bool single = false;
    std::vector<int32_t> map_tab;
    int32_t *d_map = nullptr;
    // lenses (mcs_plan_set_lens): host rows of the cameras in kp.lens_mask, the device table
    // (MCS_MAX_CAMS rows, allocated once) and whether it lags the host rows
    // fish_mask: the cameras whose lens is a fisheye one; any: the plan runs the kernels of the
    // code objects built with the fisheye model (host::kernels)
    mcs::Lens lens[MCS_MAX_CAMS] = {};
    uint32_t fish_mask = 0;
    double *d_lens = nullptr;
    bool lens_stale = false;
    // exposure gains (mcs_plan_set_gains): q = the gain in 1/256 per camera; enabled by any
    // non-NULL array, identity included.  Host state only: the prepared tables do not depend on it.
    bool gains_on = false;
    uint16_t gain_q[MCS_MAX_CAMS] = {};
    // overlap table of mcs_plan_overlap_stats (mcs_gain.cpp), built for grid step ov.step.  Not
    // part of Tables: it depends on the geometry and the lenses only, so blend and seam changes
    // keep it; mcs_plan_set_lens and mcs_plan_destroy drop it (drop_overlap).
    struct Overlap {
        int step = -1;                    // -1: none
        uint8_t *d_table = nullptr;       // segments, then the units (one allocation)
        mcs::OvUnit *d_units = nullptr;
        int n_units = 0;
        int64_t table_bytes = 0;
        int64_t N[MCS_MAX_CAMS * MCS_MAX_CAMS] = {};   // [i * MCS_MAX_CAMS + j]
        unsigned long long *d_S = nullptr;             // the sums' accumulators (grown on demand)
        size_t s_bytes = 0;
    } ov;
};

namespace mcs {
namespace host {

using rt::Api;

struct Kernels {
    bool loaded = false;
    hipFunction_t prepare[5][2] = {};     // [channels][interp]
    hipFunction_t stream[5][2] = {};      // [channels][buffer-resource DMA]
    hipFunction_t stream_big[5][2] = {};  // large-footprint tiles, as stream
    hipFunction_t direct[5][2][2] = {};   // [channels][interp][32-bit offsets]
    hipFunction_t footprint[2] = {};
    hipFunction_t resize[5] = {};         // [channels]
    hipFunction_t blend_owner[2] = {};    // [interp]
    hipFunction_t blend_classify = nullptr;
    hipFunction_t seam_sample[5][2] = {};  // [channels][interp]
    hipFunction_t feather[5][2] = {};     // [channels][interp]
    hipFunction_t mb_prep[5][2] = {};     // [channels][interp]
    hipFunction_t mb_levels[5] = {};      // [channels]
    hipFunction_t mb_blend[5][3] = {};    // [channels][<= 2 owners, <= 4, <= 8]
    // [channels][unaligned / dword-aligned windows][interior, bottom / right edge, both]
    hipFunction_t mb_bands[5][2][3] = {};
    hipFunction_t mb_bdesc[5][2] = {};    // [channels][interp]
    // multi-band sweep (module kModSweep): [channels][dword-aligned windows][2 / 4 owners]
    hipFunction_t mb_sweep[4][2][2] = {};
    hipFunction_t mb_sweep_desc[4][2] = {};   // [channels][interp]
    hipFunction_t overlap_prep[2] = {};   // [interp]
    hipFunction_t overlap_sum[5] = {};    // [channels]
    hipFunction_t gain_apply = nullptr;
    // the fused-gain twins (suffix _g: the camera gains of KParams::gain_q on the taps) of every
    // kernel that reads source bytes per launch, indexed as their twins.  (mb_blend has none: it
    // reads the mosaic and the level scratch.)
    hipFunction_t stream_g[5][2] = {};
    hipFunction_t stream_big_g[5][2] = {};
    hipFunction_t direct_g[5][2][2] = {};
    hipFunction_t feather_g[5][2] = {};
    hipFunction_t mb_levels_g[5] = {};
    hipFunction_t mb_bands_g[5][2][3] = {};
    // direct feather (mcs_stitch_direct on a FEATHER plan): [channels][interp], and its _g twins
    hipFunction_t direct_feather[5][2] = {};
    hipFunction_t direct_feather_g[5][2] = {};
    // table-free overlap statistics (mcs_plan_overlap_stats_direct): [channels][interp]
    hipFunction_t direct_overlap[5][2] = {};
    // direct multi-band (module kModDirectMb, mcs_stitch_direct_multiband): the owner pass and the
    // tile pass, [gained][channels][interp]
    hipFunction_t direct_mb_own[2][5][2] = {};
    hipFunction_t direct_mb_tile[2][5][2] = {};
};

// mcs_prepare.cpp
// The stitch, sweep and direct multi-band modules' kernels on `device` (looked up once per device).
int kernels(const Api *A, int device, const Kernels **out);
// The kernels plan p runs: those of the code objects built with the fisheye model when any of its
// cameras has a fisheye lens, the ones above otherwise (the same names, the same arguments).
int kernels(const Api *A, const mcs_plan *p, const Kernels **out);
// The plan-lifetime device tables (cylinder table, map, lens rows), uploaded when missing / stale.
int upload_plan_tables(const Api *A, mcs_plan *p, hipStream_t s);
// Builds p->t unless it stands.  Allocates and synchronises: call before graph capture (the
// stitch entry points call it lazily).  On failure the plan is as before the call.
int prepare(const Api *A, mcs_plan *p, hipStream_t s);
// Frees the prepared tables (they are rebuilt on next use): p->t is a fresh Tables afterwards.
void release_tables(const Api *A, mcs_plan *p);

// mcs_capi.cpp
// The plan's own stream and the device buffers of the host-array path, created on first use.
int ensure_stream(const Api *A, mcs_plan *p);
int ensure_host_buffers(const Api *A, mcs_plan *p);

// mcs_gain.cpp
// Frees the overlap table and its accumulators (the next mcs_plan_overlap_stats rebuilds them).
void drop_overlap(const Api *A, mcs_plan *p);
// q[cam] on `bytes` source bytes of n_frames frames (in place when dst == src); d_q: a device q
// read at run time instead (streams).
int launch_gain(const Api *A, const Kernels *k, const uint8_t *src, uint8_t *dst, int64_t bytes,
                int64_t src_fstride, int64_t dst_fstride, int n_frames, uint32_t q,
                const uint16_t *d_q, hipStream_t s);

// mcs_sweep_host.cpp
int prepare_sweep(const Api *A, mcs_plan *p, const Kernels *k, hipStream_t s);

// mcs_launch.cpp
// One module launch of `f` with the argument block [args, args + sz).
int launch_args(const Api *A, hipFunction_t f, unsigned gx, unsigned gy, unsigned bx, unsigned by,
                void *args, size_t sz, hipStream_t s, unsigned gz = 1, unsigned lds = 0);
// need[i]: camera i contributes to the mosaic (a passthrough stage's A is never read).
void need_mask(const mcs_flat_desc &fd, bool *need);
bool offset_base(const mcs_plan *p, const KParams &kp, const uint8_t **base);
void mb_args(const mcs_plan *p, const KParams &P, KMbArgs &a);
void band_args(const mcs_plan *p, const KParams &P, KMbBandArgs &a);
int launch_resize(const Api *A, const Kernels *k, const uint8_t *src, int sw, int sh,
                  int64_t src_pitch, int64_t src_fstride, uint8_t *dst, int dw, int dh,
                  int64_t dst_pitch, int64_t dst_fstride, int C, int n_frames, hipStream_t s);
// Camera i's frame stride in bytes: the caller's, or without one its frames back to back.
inline int64_t cam_fstride(const mcs_flat_desc &fd, const int64_t *strides, int i)
{
    return strides ? strides[i] : (int64_t)fd.cam_w[i] * fd.cam_h[i] * fd.channels;
}
// The plan's device-table pointers into a call's P, after upload_plan_tables / prepare.
void plan_table_pointers(const mcs_plan *p, KParams *P);
// The frame runs of a batch.  The kernels walk the captures of a launch with one frame stride:
// when every used camera has cam_fstride[0], body(kp, n_frames) once; else body(P, 1) per capture
// f with P's cams (a NULL one stays NULL) and out advanced to capture f, cam_fstride and
// out_fstride as given.  Returns the first status that is not MCS_OK.
template <class Body>
int for_frame_runs(const mcs_plan *p, const KParams &kp, int n_frames, Body body)
{
    bool uniform = true;
    for (int j = 0; j < p->fd.n_stages; j++)
        uniform = uniform && kp.cam_fstride[p->fd.st[j].cam] == kp.cam_fstride[0];
    if (uniform) return body(kp, n_frames);
    KParams P = kp;
    for (int f = 0; f < n_frames; f++) {
        for (int i = 0; i < p->fd.n_cams; i++)
            P.cams[i] = kp.cams[i] ? kp.cams[i] + (int64_t)f * kp.cam_fstride[i] : nullptr;
        P.out = kp.out + (int64_t)f * kp.out_fstride;
        const int rc = body(P, 1);
        if (rc) return rc;
    }
    return MCS_OK;
}
// gained: the _g kernels for every launch of the batch, with the plan's gain_q as of this call in
// their kernel arguments (mcs_stitch_device_gained); the caller has ruled out sweep plans.
int launch_stitch(const Api *A, mcs_plan *p, const KParams &kp, int n_frames, hipStream_t s,
                  bool gained = false);
// Whether a gained launch of the plan needs the _g kernels: gains enabled and some used camera's
// q other than 256 (q = 256 is the identity bit for bit: the ungained kernels are exact).
bool gains_active(const mcs_plan *p);
// The plan's q per camera into kp.gain_q (256 where gains are disabled).
void fill_gain_q(const mcs_plan *p, KParams *kp);

}  // namespace host
}  // namespace mcs
