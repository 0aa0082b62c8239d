// mcs_stitch.cpp -- the entry points that render a mosaic from device-resident frames (declared
// in include/mcs.h): the batch through the plan's prepared tables and the table-free direct
// forms, each with its fused-gain twin.  Scheduling: mcs_launch.cpp.
#include "mcs_common.h"
#include "mcs_plan_state.h"

using namespace mcs::host;

namespace {

// Kernel parameters of a device-resident batch (mcs_stitch_device / mcs_stitch_direct).
int device_kparams(const mcs_plan *p, const uint8_t *const *d_cams,
                   const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch,
                   int64_t out_frame_stride, int n_frames, mcs::KParams *kp)
{
    if (!p || !d_cams || !d_out) return mcs::fail(MCS_E_INVALID, "NULL plan/d_cams/d_out");
    if (n_frames < 0 || n_frames > 65535) return mcs::fail(MCS_E_INVALID, "n_frames=%d", n_frames);
    const int C = p->fd.channels;
    if (out_pitch < (int64_t)p->fd.out_w * C)
        return mcs::fail(MCS_E_INVALID, "out_pitch %lld < row bytes %lld", (long long)out_pitch,
                         (long long)p->fd.out_w * C);
    *kp = p->kp;
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    for (int i = 0; i < p->fd.n_cams; i++) {
        if (need[i] && !d_cams[i]) return mcs::fail(MCS_E_INVALID, "d_cams[%d] NULL", i);
        kp->cams[i] = d_cams[i];
        kp->cam_fstride[i] = cam_fstride(p->fd, cam_frame_stride, i);
    }
    kp->out = d_out;
    kp->out_pitch = out_pitch;
    kp->out_fstride = out_frame_stride ? out_frame_stride : out_pitch * p->fd.out_h;
    return MCS_OK;
}

// The device entry points read caller memory and never write it, so they cannot apply gains.
int refuse_gains(const mcs_plan *p, const char *entry)
{
    if (!p || !p->gains_on) return MCS_OK;
    return mcs::fail(MCS_E_UNSUPPORTED, "%s reads the caller's frames and never writes them: on a "
                     "plan with gains (mcs_plan_set_gains) apply them to the frames first with "
                     "mcs_gain_apply_device and stitch with a plan without gains", entry);
}

// Whether a direct call of checked arguments has nothing to render.
bool nothing_to_render(const mcs::KParams &kp, int n_frames)
{
    return kp.out_w <= 0 || kp.out_h <= 0 || n_frames == 0;
}

// What the table-free forms share once their own refusals have passed.  gained: the _g kernels
// with the plan's q as of this call in their arguments, unless the plan has no gains or every
// used camera's q is the identity.  The plan-lifetime tables (cylinder / table / lensed plans) are
// uploaded once.
template <class Body>
int direct_launch(mcs_plan *p, mcs::KParams kp, int n_frames, void *stream, Body body)
{
    const bool gained = gains_active(p);
    if (gained) fill_gain_q(p, &kp);
    if (nothing_to_render(kp, n_frames)) return MCS_OK;
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    const Kernels *k = nullptr;
    int rc = kernels(A, p, &k);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = upload_plan_tables(A, p, s);
    if (rc) return rc;
    plan_table_pointers(p, &kp);
    return for_frame_runs(p, kp, n_frames, [&](const mcs::KParams &P, int nf) {
        return body(A, k, s, gained, P, nf);
    });
}

}  // namespace

// mcs_stitch_device(_gained) after the refusals: the checks, the device, the launch.
int mcs::stitch_device_frames(mcs_plan *p, const uint8_t *const *d_cams,
                              const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch,
                              int64_t out_frame_stride, int n_frames, void *stream, bool gained)
{
    mcs::KParams kp;
    int rc = device_kparams(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                            n_frames, &kp);
    if (rc) return rc;
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    // (identity gains, or none: exactly the ungained launch)
    return launch_stitch(A, p, kp, n_frames, (hipStream_t)stream, gained && gains_active(p));
}

extern "C" {

int mcs_stitch_device(mcs_plan *p, const uint8_t *const *d_cams, const int64_t *cam_frame_stride,
                      uint8_t *d_out, int64_t out_pitch, int64_t out_frame_stride, int n_frames,
                      void *stream)
{
    const int rc = refuse_gains(p, "mcs_stitch_device");
    if (rc) return rc;
    return mcs::stitch_device_frames(p, d_cams, cam_frame_stride, d_out, out_pitch,
                                     out_frame_stride, n_frames, stream);
}

int mcs_stitch_direct(mcs_plan *p, const uint8_t *const *d_cams, const int64_t *cam_frame_stride,
                      uint8_t *d_out, int64_t out_pitch, int64_t out_frame_stride, int n_frames,
                      void *stream)
{
    const int rc = refuse_gains(p, "mcs_stitch_direct");
    if (rc) return rc;
    return mcs_stitch_direct_gained(p, d_cams, cam_frame_stride, d_out, out_pitch,
                                    out_frame_stride, n_frames, stream);
}

int mcs_direct_multiband_work_size(const mcs_plan *p, int64_t *bytes)
{
    mcs::clear_error();
    if (!p || !bytes) return mcs::fail(MCS_E_INVALID, "NULL plan/bytes");
    *bytes = mcs::direct_mb_work_bytes(p->fd.out_w, p->fd.out_h);
    return MCS_OK;
}

int mcs_stitch_direct_multiband(mcs_plan *p, const uint8_t *const *d_cams,
                                const int64_t *cam_frame_stride, uint8_t *d_out,
                                int64_t out_pitch, int64_t out_frame_stride, int n_frames,
                                void *d_work, int64_t work_bytes, void *stream)
{
    const int rc = refuse_gains(p, "mcs_stitch_direct_multiband");
    if (rc) return rc;
    return mcs_stitch_direct_multiband_gained(p, d_cams, cam_frame_stride, d_out, out_pitch,
                                              out_frame_stride, n_frames, d_work, work_bytes,
                                              stream);
}

// The fused forms: the plan's gains inside the kernels, on the taps (csrc/mcs_dev.h gain_half);
// the caller's frames are only read.  On a plan without gains they make the plain forms' launches,
// so a plain direct form is its refusal of a plan with gains, then the fused form.
int mcs_stitch_device_gained(mcs_plan *p, const uint8_t *const *d_cams,
                             const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch,
                             int64_t out_frame_stride, int n_frames, void *stream)
{
    return mcs::stitch_device_frames(p, d_cams, cam_frame_stride, d_out, out_pitch,
                                     out_frame_stride, n_frames, stream, true);
}

int mcs_stitch_direct_gained(mcs_plan *p, const uint8_t *const *d_cams,
                             const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch,
                             int64_t out_frame_stride, int n_frames, void *stream)
{
    mcs::KParams kp;
    int rc = device_kparams(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                            n_frames, &kp);
    if (rc) return rc;
    if (p->blend != MCS_BLEND_NONE && p->blend != MCS_BLEND_SEAM && p->blend != MCS_BLEND_FEATHER)
        return mcs::fail(MCS_E_UNSUPPORTED, "mcs_stitch_direct renders paste / seam / feather "
                         "plans; multi-band plans need their prepared tables (mcs_stitch_device)");
    const bool feather = p->blend == MCS_BLEND_FEATHER;
    const int C = p->fd.channels, I = p->fd.interp;
    const int gx = (p->fd.out_w + mcs::kTileW - 1) / mcs::kTileW;
    const int gy = (p->fd.out_h + mcs::kTileH - 1) / mcs::kTileH;
    return direct_launch(p, kp, n_frames, stream,
                         [&](const Api *A, const Kernels *k, hipStream_t s, bool g,
                             const mcs::KParams &P, int nf) {
        mcs::KDirectArgs args;
        args.P = P;
        const bool off32 = offset_base(p, args.P, &args.P.base);
        args.fallback = nullptr;   // every tile
        args.n_frames = nf;
        args.pad_ = 0;
        const unsigned fy = (unsigned)((nf + mcs::kDirectFrames - 1) / mcs::kDirectFrames);
        // (feather: the one-pass blend kernel over the same grid; it addresses frames by pointer)
        const hipFunction_t fn = feather ? (g ? k->direct_feather_g : k->direct_feather)[C][I]
                                         : (g ? k->direct_g : k->direct)[C][I][off32 ? 1 : 0];
        return launch_args(A, fn, (unsigned)(gx * gy), fy, mcs::kWave, mcs::kWavesPerBlock, &args,
                           sizeof(args), s);
    });
}

// Two launches per run of frames (csrc/mcs_direct_mb.hip), the caller's work area between them.
int mcs_stitch_direct_multiband_gained(mcs_plan *p, const uint8_t *const *d_cams,
                                       const int64_t *cam_frame_stride, uint8_t *d_out,
                                       int64_t out_pitch, int64_t out_frame_stride, int n_frames,
                                       void *d_work, int64_t work_bytes, void *stream)
{
    mcs::KParams kp;
    int rc = device_kparams(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                            n_frames, &kp);
    if (rc) return rc;
    if (p->blend != MCS_BLEND_MULTIBAND)
        return mcs::fail(MCS_E_INVALID, "mcs_stitch_direct_multiband renders multi-band plans "
                         "(mcs_plan_set_blend MCS_BLEND_MULTIBAND); paste / seam / feather plans "
                         "are mcs_stitch_direct's");
    const int64_t need = mcs::direct_mb_work_bytes(kp.out_w, kp.out_h);
    if (!nothing_to_render(kp, n_frames) && (!d_work || work_bytes < need))
        return mcs::fail(MCS_E_INVALID, "mcs_stitch_direct_multiband: the work area (%s, %lld "
                         "bytes) must hold %lld bytes (mcs_direct_multiband_work_size)",
                         d_work ? "given" : "NULL", (long long)work_bytes, (long long)need);
    kp.base = nullptr;   // (the kernels address frames by pointer)
    const int C = p->fd.channels, I = p->fd.interp;
    const int gx = (kp.out_w + mcs::kTileW - 1) / mcs::kTileW;
    const int gy = (kp.out_h + mcs::kTileH - 1) / mcs::kTileH;
    return direct_launch(p, kp, n_frames, stream,
                         [&](const Api *A, const Kernels *k, hipStream_t s, bool g,
                             const mcs::KParams &P, int nf) {
        mcs::KDirectMbArgs args;
        args.P = P;
        args.cells = static_cast<uint32_t *>(d_work);
        args.n_frames = nf;
        args.gxb = (kp.out_w + mcs::kBlendTileW - 1) / mcs::kBlendTileW;
        args.gyb = (kp.out_h + mcs::kBlendTileH - 1) / mcs::kBlendTileH;
        args.cgx = mcs::dmb_cells(kp.out_w);
        args.cgy = mcs::dmb_cells(kp.out_h);
        args.pad_ = 0;
        const unsigned fy = (unsigned)((nf + mcs::kDirectFrames - 1) / mcs::kDirectFrames);
        const int rc = launch_args(A, k->direct_mb_own[g][C][I], (unsigned)(gx * gy), fy,
                                   mcs::kWave, mcs::kWavesPerBlock, &args, sizeof(args), s);
        if (rc) return rc;
        return launch_args(A, k->direct_mb_tile[g][C][I], (unsigned)(args.gxb * args.gyb),
                           (unsigned)nf, mcs::kDmbTileThreads, 1, &args, sizeof(args), s, 1,
                           (unsigned)mcs::dmb_lds(C).bytes);
    });
}

}  // extern "C"
