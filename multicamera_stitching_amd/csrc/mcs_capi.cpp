// mcs_capi.cpp -- the extern "C" boundary of libmcs.so (declared in include/mcs.h).
//
// Replaces, for a calibrated chain, the per-frame work of Stitcher.stitch
// (PostScripts/Stitcher/StitcherClass.py:114-136).  No exception crosses this boundary: every
// entry point returns an MCS_* status and leaves a message in mcs_last_error().  The plan and
// what the entry points call are declared in mcs_plan_state.h.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "mcs_common.h"
#include "mcs_plan_state.h"
#include "mcs_scratch.h"

int mcs::plan_device(const mcs_plan *plan) { return plan ? plan->device : 0; }

#define MCS_VERSION_STRING "mcs 0.1.0 (gfx950 code object, HIP module launch)"

using namespace mcs::host;
using mcs::kMaxDevices;

namespace mcs {
namespace host {

int ensure_stream(const Api *A, mcs_plan *p)
{
    if (!p->stream) HIP_TRY(A->hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    return MCS_OK;
}

int ensure_host_buffers(const Api *A, mcs_plan *p)
{
    const int C = p->fd.channels;
    for (int i = 0; i < p->fd.n_cams; i++) {
        if (p->d_cams[i]) continue;
        const size_t bytes = (size_t)p->fd.cam_w[i] * p->fd.cam_h[i] * C;
        HIP_TRY(A->hipMalloc((void **)&p->d_cams[i], bytes > 0 ? bytes : 1));
    }
    if (!p->d_out && p->fd.out_w > 0 && p->fd.out_h > 0) {
        p->out_pitch = ((int64_t)p->fd.out_w * C + 63) / 64 * 64;
        HIP_TRY(A->hipMalloc((void **)&p->d_out, (size_t)p->out_pitch * p->fd.out_h));
    }
    return MCS_OK;
}

}  // namespace host
}  // namespace mcs

extern "C" {

const char *mcs_version(void) { return MCS_VERSION_STRING; }

int mcs_abi_version(void) { return MCS_ABI_VERSION; }

#ifndef MCS_BUILD_ID
#define MCS_BUILD_ID "unknown"
#endif
const char *mcs_build_id(void) { return MCS_BUILD_ID; }

const char *mcs_hip_runtime(void)
{
    (void)mcs::rt::api();
    return mcs::rt::runtime_name();
}

const char *mcs_last_error(void) { return mcs::last_error(); }

int mcs_device_count(int *n)
{
    if (!n) return mcs::fail(MCS_E_INVALID, "n is NULL");
    *n = 0;
    const Api *A = mcs::rt::api();
    if (!A) return MCS_E_HIP;
    int c = 0;
    hipError_t e = A->hipGetDeviceCount(&c);
    if (e != hipSuccess)
        return mcs::fail(MCS_E_HIP, "hipGetDeviceCount: %s", A->hipGetErrorString(e));
    *n = c;
    return MCS_OK;
}

int mcs_plan_create(const mcs_stage_desc *stages, int n_stages, int cam0_w, int cam0_h,
                    int channels, int interp, int device, mcs_plan **out)
{
    mcs::clear_error();
    if (!stages || !out) return mcs::fail(MCS_E_INVALID, "NULL stages/out");
    *out = nullptr;
    if (device < 0 || device >= kMaxDevices) return mcs::fail(MCS_E_INVALID, "device=%d", device);
    mcs_plan *p = new (std::nothrow) mcs_plan();
    if (!p) return mcs::fail(MCS_E_NOMEM, "plan allocation");
    int rc = mcs::build_flat(stages, n_stages, cam0_w, cam0_h, channels, interp, &p->fd);
    if (rc != MCS_OK) {
        delete p;
        return rc;
    }
    mcs::fill_kparams(p->fd, &p->kp);
    p->device = device;
    *out = p;
    return MCS_OK;
}

int mcs_plan_create_cylindrical(const mcs_cyl_camera *cams, int n_cams, int out_w, int out_h,
                                double f_cyl, double u0, double v0, int channels, int interp,
                                int device, mcs_plan **out)
{
    mcs::clear_error();
    if (!cams || !out) return mcs::fail(MCS_E_INVALID, "NULL cams/out");
    *out = nullptr;
    if (device < 0 || device >= kMaxDevices) return mcs::fail(MCS_E_INVALID, "device=%d", device);
    if (n_cams < 1 || n_cams > MCS_MAX_STAGES)
        return mcs::fail(MCS_E_INVALID, "n_cams %d (1..%d)", n_cams, MCS_MAX_STAGES);
    if (channels < 1 || channels > 4) return mcs::fail(MCS_E_INVALID, "channels %d", channels);
    if (interp != MCS_INTER_NEAREST && interp != MCS_INTER_LINEAR)
        return mcs::fail(MCS_E_INVALID, "interp %d", interp);
    if (out_w < 1 || out_h < 1 || (int64_t)out_w * out_h * channels > ((int64_t)1 << 31))
        return mcs::fail(MCS_E_SHAPE, "panorama %dx%d", out_w, out_h);
    if (!(f_cyl > 0.0) || !std::isfinite(u0) || !std::isfinite(v0))
        return mcs::fail(MCS_E_INVALID, "f_cyl / u0 / v0");
    for (int c = 0; c < n_cams; c++) {
        const mcs_cyl_camera &k = cams[c];
        if (k.w < 1 || k.h < 1 || k.w > 32767 || k.h > 32767)
            return mcs::fail(MCS_E_SHAPE, "camera %d: %dx%d", c, k.w, k.h);
        if ((long)k.w * k.h * channels < 8)
            return mcs::fail(MCS_E_UNSUPPORTED, "camera %d: camera frame of %ld bytes (< 8)", c,
                             (long)k.w * k.h * channels);
        bool fin = std::isfinite(k.f) && k.f > 0.0 && std::isfinite(k.cx) && std::isfinite(k.cy);
        for (double r : k.R) fin = fin && std::isfinite(r);
        if (!fin) return mcs::fail(MCS_E_INVALID, "camera %d: R / f / cx / cy", c);
    }
    mcs_plan *p = new (std::nothrow) mcs_plan();
    if (!p) return mcs::fail(MCS_E_NOMEM, "plan allocation");
    mcs_flat_desc &fd = p->fd;
    memset(&fd, 0, sizeof(fd));
    fd.n_stages = n_cams;
    fd.out_w = out_w;
    fd.out_h = out_h;
    fd.channels = channels;
    fd.interp = interp;
    fd.n_cams = n_cams;
    for (int c = 0; c < n_cams; c++) {
        fd.cam_w[c] = cams[c].w;
        fd.cam_h[c] = cams[c].h;
        mcs_flat_stage &st = fd.st[c];
        memcpy(st.minv, cams[c].R, sizeof(st.minv));   // the rotation (describe: R, not H^-1)
        st.rect[2] = out_w;
        st.rect[3] = out_h;
        st.bw0 = 1;
        st.cam = c;
    }
    mcs::fill_kparams(fd, &p->kp);
    p->kp.cam0_w = p->kp.cam0_h = 0;   // no integer-placed camera: every camera is a stage
    for (int c = 0; c < n_cams; c++) {
        mcs::KStage &k = p->kp.st[c];
        k.kind = mcs::kStageCylinder;
        k.f = cams[c].f;
        k.cx = cams[c].cx;
        k.cy = cams[c].cy;
    }
    p->cyl = true;
    p->cyl_tab.resize(2 * (size_t)out_w + out_h);
    for (int u = 0; u < out_w; u++) {
        const double t = ((double)u - u0) / f_cyl;
        p->cyl_tab[2 * u] = std::sin(t);
        p->cyl_tab[2 * u + 1] = std::cos(t);
    }
    for (int v = 0; v < out_h; v++) p->cyl_tab[2 * (size_t)out_w + v] = ((double)v - v0) / f_cyl;
    p->blend = MCS_BLEND_MULTIBAND;
    p->kp.blend = MCS_BLEND_MULTIBAND;
    p->device = device;
    *out = p;
    return MCS_OK;
}

namespace {

// Single-camera plan: stage 0 samples camera 0 everywhere (empty paste rect, paste rule).
mcs_plan *single_plan(int src_w, int src_h, int dst_w, int dst_h, int channels, int interp,
                      int device, const double *minv, int kind)
{
    mcs_plan *p = new (std::nothrow) mcs_plan();
    if (!p) return nullptr;
    mcs_flat_desc &fd = p->fd;
    memset(&fd, 0, sizeof(fd));
    fd.n_stages = 1;
    fd.out_w = dst_w;
    fd.out_h = dst_h;
    fd.channels = channels;
    fd.interp = interp;
    fd.n_cams = 1;
    fd.cam_w[0] = src_w;
    fd.cam_h[0] = src_h;
    if (minv) memcpy(fd.st[0].minv, minv, sizeof(fd.st[0].minv));
    fd.st[0].bw0 = mcs::block_width(dst_w, dst_h);
    fd.st[0].cam = 0;
    mcs::fill_kparams(fd, &p->kp);
    p->kp.cam0_w = p->kp.cam0_h = 0;
    p->kp.st[0].kind = kind;
    p->single = true;
    p->device = device;
    return p;
}

int check_single_args(int src_w, int src_h, int dst_w, int dst_h, int channels, int device)
{
    if (device < 0 || device >= kMaxDevices) return mcs::fail(MCS_E_INVALID, "device=%d", device);
    if (channels < 1 || channels > 4) return mcs::fail(MCS_E_INVALID, "channels %d", channels);
    if (src_w < 1 || src_h < 1 || src_w > 32767 || src_h > 32767)
        return mcs::fail(MCS_E_SHAPE, "source %dx%d", src_w, src_h);
    // (the direct gather moves each 8-byte window left so that it ends inside the frame)
    if ((long)src_w * src_h * channels < 8)
        return mcs::fail(MCS_E_UNSUPPORTED, "camera frame of %ld bytes (< 8)",
                         (long)src_w * src_h * channels);
    if (dst_w < 1 || dst_h < 1 || (int64_t)dst_w * dst_h * channels > ((int64_t)1 << 31))
        return mcs::fail(MCS_E_SHAPE, "destination %dx%d", dst_w, dst_h);
    return MCS_OK;
}

}  // namespace

int mcs_plan_create_warp(const double *M, int src_w, int src_h, int dst_w, int dst_h,
                         int channels, int interp, int device, mcs_plan **out)
{
    mcs::clear_error();
    if (!M || !out) return mcs::fail(MCS_E_INVALID, "NULL M/out");
    *out = nullptr;
    int rc = check_single_args(src_w, src_h, dst_w, dst_h, channels, device);
    if (rc) return rc;
    if (interp != MCS_INTER_NEAREST && interp != MCS_INTER_LINEAR)
        return mcs::fail(MCS_E_INVALID, "interp %d", interp);
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(M[i])) return mcs::fail(MCS_E_INVALID, "M[%d] not finite", i);
    double minv[9];
    mcs::invert3x3_cv(M, minv);   // warpPerspective inverts M (no WARP_INVERSE_MAP)
    mcs_plan *p = single_plan(src_w, src_h, dst_w, dst_h, channels, interp, device, minv,
                              mcs::kStageHomography);
    if (!p) return mcs::fail(MCS_E_NOMEM, "plan allocation");
    *out = p;
    return MCS_OK;
}

int mcs_plan_create_undistort(const double *K, const double *dist, int n_dist, int w, int h,
                              int channels, int device, mcs_plan **out)
{
    mcs::clear_error();
    if (!K || !out || (n_dist > 0 && !dist)) return mcs::fail(MCS_E_INVALID, "NULL K/dist/out");
    *out = nullptr;
    int rc = check_single_args(w, h, w, h, channels, device);
    if (rc) return rc;
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(K[i])) return mcs::fail(MCS_E_INVALID, "K[%d] not finite", i);
    std::vector<int32_t> tab(2 * (size_t)w * h);
    if (!mcs::undistort_map(K, dist, n_dist, w, h, tab.data()))
        return mcs::fail(MCS_E_UNSUPPORTED, "distortion vector of %d coefficients (0, 4, 5, 8, "
                         "12 or 14 with tau = 0)", n_dist);
    mcs_plan *p = single_plan(w, h, w, h, channels, MCS_INTER_LINEAR, device, nullptr,
                              mcs::kStageTable);
    if (!p) return mcs::fail(MCS_E_NOMEM, "plan allocation");
    p->map_tab.swap(tab);
    *out = p;
    return MCS_OK;
}

int mcs_undistort_map_host(const double *K, const double *dist, int n_dist, int w, int h,
                           int32_t *map)
{
    mcs::clear_error();
    if (!K || !map || (n_dist > 0 && !dist)) return mcs::fail(MCS_E_INVALID, "NULL K/dist/map");
    if (w < 1 || h < 1 || w > 32767 || h > 32767) return mcs::fail(MCS_E_SHAPE, "%dx%d", w, h);
    if (!mcs::undistort_map(K, dist, n_dist, w, h, map))
        return mcs::fail(MCS_E_UNSUPPORTED, "distortion vector of %d coefficients", n_dist);
    return MCS_OK;
}

int mcs_plan_destroy(mcs_plan *p)
{
    if (!p) return MCS_OK;
    bool touched = p->stream || p->d_out || !p->t.owned.empty() || p->side || p->side2 ||
                   p->d_lens || p->d_cyl || p->d_map || p->d_seam || p->ov.d_table || p->ov.d_S;
    for (int i = 0; i < MCS_MAX_CAMS; i++) touched = touched || p->d_cams[i];
    if (touched) {
        const mcs::Entry A(p->device);
        if (A) {
            if (p->stream) (void)A->hipStreamSynchronize(p->stream);
            for (int i = 0; i < MCS_MAX_CAMS; i++)
                if (p->d_cams[i]) (void)A->hipFree(p->d_cams[i]);
            if (p->d_out) (void)A->hipFree(p->d_out);
            for (int i = 0; i < MCS_MAX_CAMS; i++)
                if (p->d_raw[i]) (void)A->hipFree(p->d_raw[i]);
            release_tables(A, p);
            drop_overlap(A, p);
            if (p->d_cyl) (void)A->hipFree(p->d_cyl);
            if (p->d_seam) (void)A->hipFree(p->d_seam);
            if (p->d_map) (void)A->hipFree(p->d_map);
            if (p->d_lens) (void)A->hipFree(p->d_lens);
            if (p->side) (void)A->hipStreamSynchronize(p->side);
            if (p->side2) (void)A->hipStreamSynchronize(p->side2);
            if (p->stream) (void)A->hipStreamDestroy(p->stream);
            if (p->side) (void)A->hipStreamDestroy(p->side);
            if (p->side2) (void)A->hipStreamDestroy(p->side2);
            if (p->ev_fork) (void)A->hipEventDestroy(p->ev_fork);
            if (p->ev_join) (void)A->hipEventDestroy(p->ev_join);
            if (p->ev_join2) (void)A->hipEventDestroy(p->ev_join2);
            if (p->ev_early) (void)A->hipEventDestroy(p->ev_early);
        }
    }
    delete p;
    return MCS_OK;
}

int mcs_plan_out_shape(const mcs_plan *p, int *w, int *h, int *channels)
{
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    if (w) *w = p->fd.out_w;
    if (h) *h = p->fd.out_h;
    if (channels) *channels = p->fd.channels;
    return MCS_OK;
}

int mcs_plan_describe(const mcs_plan *p, mcs_flat_desc *out)
{
    if (!p || !out) return mcs::fail(MCS_E_INVALID, "NULL plan/out");
    *out = p->fd;
    return MCS_OK;
}

int mcs_stitch_host(mcs_plan *p, const uint8_t *const *cams, uint8_t *out)
{
    return mcs_stitch_host_sized(p, cams, nullptr, nullptr, out);
}

int mcs_stitch_host_sized(mcs_plan *p, const uint8_t *const *cams, const int *cam_w,
                          const int *cam_h, uint8_t *out)
{
    mcs::clear_error();
    if (!p || !cams || !out) return mcs::fail(MCS_E_INVALID, "NULL plan/cams/out");
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    const int C = p->fd.channels;
    int rc = ensure_stream(A, p);
    if (rc) return rc;
    rc = ensure_host_buffers(A, p);
    if (rc) return rc;
    if (p->fd.out_w <= 0 || p->fd.out_h <= 0) return MCS_OK;
    const Kernels *k = nullptr;
    rc = kernels(A, p->device, &k);
    if (rc) return rc;
    // only cameras that contribute are uploaded (a passthrough stage's A is never read); a frame
    // off its calibrated size is resized on the device first (StitcherClass.py:226-233)
    bool need[MCS_MAX_CAMS];
    need_mask(p->fd, need);
    for (int i = 0; i < p->fd.n_cams; i++) {
        if (!need[i]) continue;
        if (!cams[i]) return mcs::fail(MCS_E_INVALID, "cams[%d] NULL", i);
        const int cw = p->fd.cam_w[i], ch = p->fd.cam_h[i];
        const int w = cam_w ? cam_w[i] : cw, h = cam_h ? cam_h[i] : ch;
        if (w <= 0 || h <= 0) return mcs::fail(MCS_E_INVALID, "cams[%d] size %dx%d", i, w, h);
        // exposure gains act on the frame the stitch samples: after the upload and the resize
        const auto gain = [&]() {
            if (!p->gains_on) return (int)MCS_OK;
            return launch_gain(A, k, p->d_cams[i], p->d_cams[i], (int64_t)cw * ch * C, 0, 0, 1,
                               p->gain_q[i], nullptr, p->stream);
        };
        if (w == cw && h == ch) {
            HIP_TRY(A->hipMemcpyAsync(p->d_cams[i], cams[i], (size_t)cw * ch * C,
                                      hipMemcpyHostToDevice, p->stream));
            rc = gain();
            if (rc) return rc;
            continue;
        }
        const size_t bytes = (size_t)w * h * C;
        if (p->raw_bytes[i] < bytes) {
            if (p->d_raw[i]) {
                HIP_TRY(A->hipStreamSynchronize(p->stream));
                HIP_TRY(A->hipFree(p->d_raw[i]));
                p->d_raw[i] = nullptr;
                p->raw_bytes[i] = 0;
            }
            HIP_TRY(A->hipMalloc((void **)&p->d_raw[i], bytes));
            p->raw_bytes[i] = bytes;
        }
        HIP_TRY(A->hipMemcpyAsync(p->d_raw[i], cams[i], bytes, hipMemcpyHostToDevice, p->stream));
        rc = launch_resize(A, k, p->d_raw[i], w, h, (int64_t)w * C, 0, p->d_cams[i], cw, ch,
                           (int64_t)cw * C, 0, C, 1, p->stream);
        if (rc == MCS_OK) rc = gain();
        if (rc) return rc;
    }
    mcs::KParams kp = p->kp;
    for (int i = 0; i < p->fd.n_cams; i++) {
        kp.cams[i] = p->d_cams[i];
        kp.cam_fstride[i] = 0;
    }
    kp.out = p->d_out;
    kp.out_pitch = p->out_pitch;
    kp.out_fstride = 0;
    rc = launch_stitch(A, p, kp, 1, p->stream);
    if (rc) return rc;
    const size_t row = (size_t)p->fd.out_w * C;
    HIP_TRY(A->hipMemcpy2DAsync(out, row, p->d_out, (size_t)p->out_pitch, row, p->fd.out_h,
                                hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(A->hipStreamSynchronize(p->stream));
    return MCS_OK;
}

int mcs_resize_linear_device(const uint8_t *d_src, int src_w, int src_h, int64_t src_pitch,
                             int64_t src_frame_stride, uint8_t *d_dst, int dst_w, int dst_h,
                             int64_t dst_pitch, int64_t dst_frame_stride, int channels,
                             int n_frames, int device, void *stream)
{
    mcs::clear_error();
    if (!d_src || !d_dst) return mcs::fail(MCS_E_INVALID, "NULL src/dst");
    if (channels < 1 || channels > 4) return mcs::fail(MCS_E_UNSUPPORTED, "channels=%d", channels);
    if (src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0)
        return mcs::fail(MCS_E_INVALID, "sizes %dx%d -> %dx%d", src_w, src_h, dst_w, dst_h);
    if (dst_h > 65535 || n_frames < 0 || n_frames > 65535)
        return mcs::fail(MCS_E_INVALID, "dst_h=%d n_frames=%d", dst_h, n_frames);
    if (src_pitch < (int64_t)src_w * channels || dst_pitch < (int64_t)dst_w * channels)
        return mcs::fail(MCS_E_INVALID, "pitch smaller than a row");
    if (n_frames == 0) return MCS_OK;
    const mcs::Entry A(device);
    if (A.status) return A.status;
    const Kernels *k = nullptr;
    int rc = kernels(A, device, &k);
    if (rc) return rc;
    const int64_t sfs = src_frame_stride ? src_frame_stride : src_pitch * src_h;
    const int64_t dfs = dst_frame_stride ? dst_frame_stride : dst_pitch * dst_h;
    return launch_resize(A, k, d_src, src_w, src_h, src_pitch, sfs, d_dst, dst_w, dst_h, dst_pitch,
                         dfs, channels, n_frames, (hipStream_t)stream);
}

// Kernel parameters of a device-resident batch (mcs_stitch_device / mcs_stitch_direct).
static int device_kparams(const mcs_plan *p, const uint8_t *const *d_cams,
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
        kp->cam_fstride[i] = cam_frame_stride ? cam_frame_stride[i]
                                              : (int64_t)p->fd.cam_w[i] * p->fd.cam_h[i] * C;
    }
    kp->out = d_out;
    kp->out_pitch = out_pitch;
    kp->out_fstride = out_frame_stride ? out_frame_stride : out_pitch * p->fd.out_h;
    return MCS_OK;
}

// The device entry points read caller memory and never write it, so they cannot apply gains.
static int refuse_gains(const mcs_plan *p, const char *entry)
{
    if (!p || !p->gains_on) return MCS_OK;
    return mcs::fail(MCS_E_UNSUPPORTED, "%s reads the caller's frames and never writes them: on a "
                     "plan with gains (mcs_plan_set_gains) apply them to the frames first with "
                     "mcs_gain_apply_device and stitch with a plan without gains", entry);
}

int mcs_stitch_device(mcs_plan *p, const uint8_t *const *d_cams, const int64_t *cam_frame_stride,
                      uint8_t *d_out, int64_t out_pitch, int64_t out_frame_stride, int n_frames,
                      void *stream)
{
    const int rc = refuse_gains(p, "mcs_stitch_device");
    if (rc) return rc;
    return mcs::stitch_device_frames(p, d_cams, cam_frame_stride, d_out, out_pitch,
                                     out_frame_stride, n_frames, stream);
}

}  // extern "C"

// mcs_stitch_device(_gained) after the refusals: the checks, the device, the launch.
static int stitch_device_launch(mcs_plan *p, const uint8_t *const *d_cams,
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

int mcs::stitch_device_frames(mcs_plan *p, const uint8_t *const *d_cams,
                              const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch,
                              int64_t out_frame_stride, int n_frames, void *stream)
{
    return stitch_device_launch(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                                n_frames, stream, false);
}

// mcs_stitch_direct(_gained) after the refusals.  gained: the _g kernels with the plan's q as of
// this call in their arguments, unless every used camera's q is the identity.
static int stitch_direct_launch(mcs_plan *p, const uint8_t *const *d_cams,
                                const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch,
                                int64_t out_frame_stride, int n_frames, void *stream, bool gained)
{
    mcs::KParams kp;
    int rc = device_kparams(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                            n_frames, &kp);
    if (rc) return rc;
    if (p->blend != MCS_BLEND_NONE && p->blend != MCS_BLEND_SEAM && p->blend != MCS_BLEND_FEATHER)
        return mcs::fail(MCS_E_UNSUPPORTED, "mcs_stitch_direct renders paste / seam / feather "
                         "plans; multi-band plans need their prepared tables (mcs_stitch_device)");
    const bool feather = p->blend == MCS_BLEND_FEATHER;
    gained = gained && gains_active(p);
    if (gained) fill_gain_q(p, &kp);
    if (kp.out_w <= 0 || kp.out_h <= 0 || n_frames == 0) return MCS_OK;
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    const Kernels *k = nullptr;
    rc = kernels(A, p->device, &k);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = upload_plan_tables(A, p, s);   // (cylinder / table plans: their device tables, once)
    if (rc) return rc;
    kp.cyl_tab = p->kp.cyl_tab;
    kp.map_tab = p->kp.map_tab;
    kp.lens_tab = p->kp.lens_tab;
    kp.seam_hint = p->kp.seam_hint;
    const int gx = (p->fd.out_w + mcs::kTileW - 1) / mcs::kTileW;
    const int gy = (p->fd.out_h + mcs::kTileH - 1) / mcs::kTileH;
    // one frame stride for every camera per launch (the kernel's walk), else frame by frame
    bool uniform = true;
    for (int j = 0; j < p->fd.n_stages; j++)
        uniform = uniform && kp.cam_fstride[p->fd.st[j].cam] == kp.cam_fstride[0];
    const int runs = uniform ? 1 : n_frames;
    for (int f = 0; f < runs; f++) {
        mcs::KDirectArgs args;
        args.P = kp;
        if (!uniform) {
            for (int i = 0; i < p->fd.n_cams; i++)
                args.P.cams[i] = kp.cams[i] ? kp.cams[i] + (int64_t)f * kp.cam_fstride[i] : nullptr;
            args.P.out = kp.out + (int64_t)f * kp.out_fstride;
        }
        const bool off32 = offset_base(p, args.P, &args.P.base);
        args.fallback = nullptr;   // every tile
        args.n_frames = uniform ? n_frames : 1;
        args.pad_ = 0;
        const unsigned fy = (unsigned)((args.n_frames + mcs::kDirectFrames - 1) / mcs::kDirectFrames);
        // (feather: the one-pass blend kernel over the same grid; it addresses frames by pointer)
        const hipFunction_t fn =
            feather ? (gained ? k->direct_feather_g : k->direct_feather)[p->fd.channels][p->fd.interp]
                    : (gained ? k->direct_g : k->direct)[p->fd.channels][p->fd.interp][off32 ? 1 : 0];
        rc = launch_args(A, fn, (unsigned)(gx * gy), fy, mcs::kWave, mcs::kWavesPerBlock, &args,
                         sizeof(args), s);
        if (rc) return rc;
    }
    return MCS_OK;
}

// mcs_stitch_direct_multiband(_gained) after the gains refusal: two launches per run of frames
// (csrc/mcs_direct_mb.hip), the caller's work area between them.
static int stitch_direct_mb_launch(mcs_plan *p, const uint8_t *const *d_cams,
                                   const int64_t *cam_frame_stride, uint8_t *d_out,
                                   int64_t out_pitch, int64_t out_frame_stride, int n_frames,
                                   void *d_work, int64_t work_bytes, void *stream, bool gained)
{
    mcs::KParams kp;
    int rc = device_kparams(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                            n_frames, &kp);
    if (rc) return rc;
    if (p->blend != MCS_BLEND_MULTIBAND)
        return mcs::fail(MCS_E_INVALID, "mcs_stitch_direct_multiband renders multi-band plans "
                         "(mcs_plan_set_blend MCS_BLEND_MULTIBAND); paste / seam / feather plans "
                         "are mcs_stitch_direct's");
    if (kp.out_w <= 0 || kp.out_h <= 0 || n_frames == 0) return MCS_OK;
    const int64_t need = mcs::direct_mb_work_bytes(kp.out_w, kp.out_h);
    if (!d_work || work_bytes < need)
        return mcs::fail(MCS_E_INVALID, "mcs_stitch_direct_multiband: the work area (%s, %lld "
                         "bytes) must hold %lld bytes (mcs_direct_multiband_work_size)",
                         d_work ? "given" : "NULL", (long long)work_bytes, (long long)need);
    gained = gained && gains_active(p);
    if (gained) fill_gain_q(p, &kp);
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    const Kernels *k = nullptr;
    rc = kernels(A, p->device, &k);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = upload_plan_tables(A, p, s);   // (cylinder / lensed plans: their device tables, once)
    if (rc) return rc;
    kp.cyl_tab = p->kp.cyl_tab;
    kp.map_tab = p->kp.map_tab;
    kp.lens_tab = p->kp.lens_tab;
    kp.seam_hint = p->kp.seam_hint;
    kp.base = nullptr;   // (the kernels address frames by pointer)
    const int C = p->fd.channels, I = p->fd.interp;
    const int gx = (kp.out_w + mcs::kTileW - 1) / mcs::kTileW;
    const int gy = (kp.out_h + mcs::kTileH - 1) / mcs::kTileH;
    // one frame stride for every camera per launch, else frame by frame (as mcs_stitch_direct)
    bool uniform = true;
    for (int j = 0; j < p->fd.n_stages; j++)
        uniform = uniform && kp.cam_fstride[p->fd.st[j].cam] == kp.cam_fstride[0];
    const int runs = uniform ? 1 : n_frames;
    for (int f = 0; f < runs; f++) {
        mcs::KDirectMbArgs args;
        args.P = kp;
        if (!uniform) {
            for (int i = 0; i < p->fd.n_cams; i++)
                args.P.cams[i] = kp.cams[i] ? kp.cams[i] + (int64_t)f * kp.cam_fstride[i] : nullptr;
            args.P.out = kp.out + (int64_t)f * kp.out_fstride;
        }
        args.cells = static_cast<uint32_t *>(d_work);
        args.n_frames = uniform ? n_frames : 1;
        args.gxb = (kp.out_w + mcs::kBlendTileW - 1) / mcs::kBlendTileW;
        args.gyb = (kp.out_h + mcs::kBlendTileH - 1) / mcs::kBlendTileH;
        args.cgx = mcs::dmb_cells(kp.out_w);
        args.cgy = mcs::dmb_cells(kp.out_h);
        args.pad_ = 0;
        const unsigned fy = (unsigned)((args.n_frames + mcs::kDirectFrames - 1) / mcs::kDirectFrames);
        rc = launch_args(A, k->direct_mb_own[gained][C][I], (unsigned)(gx * gy), fy, mcs::kWave,
                         mcs::kWavesPerBlock, &args, sizeof(args), s);
        if (rc) return rc;
        rc = launch_args(A, k->direct_mb_tile[gained][C][I], (unsigned)(args.gxb * args.gyb),
                         (unsigned)args.n_frames, mcs::kDmbTileThreads, 1, &args, sizeof(args), s, 1,
                         (unsigned)mcs::dmb_lds(C).bytes);
        if (rc) return rc;
    }
    return MCS_OK;
}

extern "C" {

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
    return stitch_direct_mb_launch(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                                   n_frames, d_work, work_bytes, stream, false);
}

int mcs_stitch_direct_multiband_gained(mcs_plan *p, const uint8_t *const *d_cams,
                                       const int64_t *cam_frame_stride, uint8_t *d_out,
                                       int64_t out_pitch, int64_t out_frame_stride, int n_frames,
                                       void *d_work, int64_t work_bytes, void *stream)
{
    return stitch_direct_mb_launch(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                                   n_frames, d_work, work_bytes, stream, true);
}

int mcs_stitch_direct(mcs_plan *p, const uint8_t *const *d_cams, const int64_t *cam_frame_stride,
                      uint8_t *d_out, int64_t out_pitch, int64_t out_frame_stride, int n_frames,
                      void *stream)
{
    const int rc = refuse_gains(p, "mcs_stitch_direct");
    if (rc) return rc;
    return stitch_direct_launch(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                                n_frames, stream, false);
}

// The fused forms: the plan's gains inside the kernels, on the taps (csrc/mcs_dev.h gain_half);
// the caller's frames are only read.
int mcs_stitch_device_gained(mcs_plan *p, const uint8_t *const *d_cams,
                             const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch,
                             int64_t out_frame_stride, int n_frames, void *stream)
{
    return stitch_device_launch(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                                n_frames, stream, true);
}

int mcs_stitch_direct_gained(mcs_plan *p, const uint8_t *const *d_cams,
                             const int64_t *cam_frame_stride, uint8_t *d_out, int64_t out_pitch,
                             int64_t out_frame_stride, int n_frames, void *stream)
{
    return stitch_direct_launch(p, d_cams, cam_frame_stride, d_out, out_pitch, out_frame_stride,
                                n_frames, stream, true);
}

int mcs_plan_prepare(mcs_plan *p, void *stream)
{
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    if (p->fd.out_w <= 0 || p->fd.out_h <= 0) return MCS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (!s) {
        int rc = ensure_stream(A, p);
        if (rc) return rc;
        s = p->stream;
    }
    return prepare(A, p, s);
}

int mcs_plan_set_blend(mcs_plan *p, int mode)
{
    mcs::clear_error();
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    if (mode != MCS_BLEND_NONE && mode != MCS_BLEND_FEATHER && mode != MCS_BLEND_MULTIBAND &&
        mode != MCS_BLEND_SEAM)
        return mcs::fail(MCS_E_INVALID, "blend mode %d", mode);
    if (p->single && mode != MCS_BLEND_NONE)
        return mcs::fail(MCS_E_INVALID, "a single-camera remap plan (warp / undistort) has "
                         "nothing to blend: blend mode NONE only");
    if (p->cyl && mode == MCS_BLEND_NONE)
        return mcs::fail(MCS_E_INVALID, "a cylindrical plan has no paste order: blend mode "
                         "NONE is not defined for it (use SEAM, FEATHER or MULTIBAND)");
    if (mode == p->blend) return MCS_OK;
    if (p->t.prepared) {
        const mcs::Entry A(p->device);
        if (A.status) return A.status;
        release_tables(A, p);
    }
    p->blend = mode;
    p->kp.blend = mode;
    return MCS_OK;
}

int mcs_plan_set_lens(mcs_plan *p, int cam, const double *K, const double *dist, int n_dist)
{
    mcs::clear_error();
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    if (!p->map_tab.empty())
        return mcs::fail(MCS_E_UNSUPPORTED, "an undistort (table) plan is its own lens");
    if (cam < 0 || cam >= p->fd.n_cams)
        return mcs::fail(MCS_E_INVALID, "camera %d (0..%d)", cam, p->fd.n_cams - 1);
    mcs::Lens L;
    if (K) {
        if (n_dist < 0 || (n_dist > 0 && !dist)) return mcs::fail(MCS_E_INVALID, "NULL dist");
        const int rc = mcs::lens_from(K, dist, n_dist, &L);
        if (rc) return rc;
    } else if (!((p->kp.lens_mask >> cam) & 1u)) {
        return MCS_OK;   // none to remove
    }
    // (the overlap table holds positions through the lenses)
    if (p->t.prepared || p->ov.d_table || p->ov.d_S) {
        const mcs::Entry A(p->device);
        if (A.status) return A.status;
        if (p->t.prepared) release_tables(A, p);
        if (p->ov.d_table || p->ov.d_S) drop_overlap(A, p);
    }
    if (K) {
        p->lens[cam] = L;
        p->kp.lens_mask |= 1u << cam;
    } else {
        p->lens[cam] = mcs::Lens();
        p->kp.lens_mask &= ~(1u << cam);
    }
    p->lens_stale = true;
    return MCS_OK;
}

int mcs_lens_map_host(const double *K, const double *dist, int n_dist, const double *uv, int n,
                      double *xy, double *r2max)
{
    mcs::clear_error();
    if (!K || (n_dist > 0 && !dist) || n < 0 || (n > 0 && (!uv || !xy)))
        return mcs::fail(MCS_E_INVALID, "NULL K/dist/uv/xy");
    mcs::Lens L;
    const int rc = mcs::lens_from(K, dist, n_dist < 0 ? 0 : n_dist, &L);
    if (rc) return rc;
    if (r2max) *r2max = L.r2max;
    for (int i = 0; i < n; i++) {
        double x = std::nan(""), y = std::nan("");
        (void)mcs::lens_apply(L, uv[2 * i], uv[2 * i + 1], x, y);
        xy[2 * i] = x;
        xy[2 * i + 1] = y;
    }
    return MCS_OK;
}

int mcs_lens_unmap_host(const double *K, const double *dist, int n_dist, const double *xy, int n,
                        double *uv)
{
    mcs::clear_error();
    if (!K || (n_dist > 0 && !dist) || n < 0 || (n > 0 && (!xy || !uv)))
        return mcs::fail(MCS_E_INVALID, "NULL K/dist/xy/uv");
    mcs::Lens L;
    const int rc = mcs::lens_from(K, dist, n_dist < 0 ? 0 : n_dist, &L);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        double u = std::nan(""), v = std::nan("");
        (void)mcs::lens_invert(L, xy[2 * i], xy[2 * i + 1], u, v);
        uv[2 * i] = u;
        uv[2 * i + 1] = v;
    }
    return MCS_OK;
}

int mcs_plan_find_seams(mcs_plan *p, const uint8_t *const *cams, int method, int scale_log2)
{
    mcs::clear_error();
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    for (int64_t &v : p->seam_stats) v = 0;   // (only the device max-flow fills them in)
    if (method != MCS_SEAM_DISTANCE && method != MCS_SEAM_GRAPHCUT)
        return mcs::fail(MCS_E_INVALID, "seam method %d", method);
    if (method == MCS_SEAM_GRAPHCUT && (!cams || scale_log2 < 0 || scale_log2 > 4))
        return mcs::fail(MCS_E_INVALID, "graph-cut seams need cams and scale_log2 in 0..4");
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    release_tables(A, p);
    if (p->d_seam) (void)A->hipFree(p->d_seam);
    p->d_seam = nullptr;
    p->kp.seam_hint = nullptr;
    p->seam_lab.clear();
    p->seam_w = p->seam_h = p->seam_k = 0;
    if (method == MCS_SEAM_DISTANCE || p->fd.out_w <= 0 || p->fd.out_h <= 0) return MCS_OK;
    int rc = ensure_stream(A, p);
    if (rc == MCS_OK) rc = ensure_host_buffers(A, p);
    if (rc == MCS_OK) rc = upload_plan_tables(A, p, p->stream);
    const Kernels *k = nullptr;
    if (rc == MCS_OK) rc = kernels(A, p->device, &k);
    if (rc) return rc;
    const int C = p->fd.channels, n = p->fd.n_cams;
    for (int i = 0; i < n; i++) {
        if (!cams[i]) return mcs::fail(MCS_E_INVALID, "NULL cams[%d]", i);
        HIP_TRY(A->hipMemcpyAsync(p->d_cams[i], cams[i],
                                  (size_t)p->fd.cam_w[i] * p->fd.cam_h[i] * C,
                                  hipMemcpyHostToDevice, p->stream));
    }
    const int kk = scale_log2;
    const int gw = (p->fd.out_w + (1 << kk) - 1) >> kk, gh = (p->fd.out_h + (1 << kk) - 1) >> kk;
    const size_t np = (size_t)gw * gh;
    mcs::KSeamArgs a;
    memset(&a, 0, sizeof(a));
    a.P = p->kp;
    for (int i = 0; i < n; i++) {
        a.P.cams[i] = p->d_cams[i];
        a.P.cam_fstride[i] = 0;
    }
    a.gw = gw;
    a.gh = gh;
    a.k = kk;
    std::vector<uint8_t> lab(np), smp;   // (smp: host Dinic only)
    std::vector<uint16_t> cov(np);
    static const char what[] = "seam finding";
    mcs::Scratch sc(A, p->stream);
    HIP_TRY_AS(what, sc.dev(&a.label, np));
    HIP_TRY_AS(what, sc.dev(&a.cov, np));
    HIP_TRY_AS(what, sc.dev(&a.samples, np * C * n));
    HIP_TRY_AS(what, A->hipMemsetAsync(a.samples, 0, np * C * n, p->stream));
    rc = launch_args(A, k->seam_sample[C][p->fd.interp], (unsigned)((np + 255) / 256), 1, 256, 1,
                     &a, sizeof(a), p->stream);
    if (rc) return rc;
    // the pairwise cuts: push-relabel on the device (default), or the host Dinic
    // (MCS_SEAM_FLOW=host; the checker of the device path)
    static const bool host_flow =
        getenv("MCS_SEAM_FLOW") && !strcmp(getenv("MCS_SEAM_FLOW"), "host");
    HIP_TRY_AS(what, A->hipMemcpyAsync(cov.data(), a.cov, np * 2, hipMemcpyDeviceToHost,
                                       p->stream));
    if (host_flow) {
        HIP_TRY_AS(what, A->hipMemcpyAsync(lab.data(), a.label, np, hipMemcpyDeviceToHost,
                                           p->stream));
        smp.resize(np * C * n);
        HIP_TRY_AS(what, A->hipMemcpyAsync(smp.data(), a.samples, np * C * n,
                                           hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY_AS(what, sc.sync());
    if (host_flow) {
        rc = mcs::seam_graphcut(n, gw, gh, lab.data(), cov.data(), smp.data(), C);
        if (rc) return rc;
        HIP_TRY_AS(what, A->hipMemcpyAsync(a.label, lab.data(), np, hipMemcpyHostToDevice,
                                           p->stream));
    } else {
        rc = mcs::seam_graphcut_device(p->device, p->stream, n, gw, gh, a.label, a.cov, a.samples,
                                       C, cov.data(), p->seam_stats);
        if (rc) return rc;
        HIP_TRY_AS(what, A->hipMemcpyAsync(lab.data(), a.label, np, hipMemcpyDeviceToHost,
                                           p->stream));
    }
    HIP_TRY_AS(what, sc.sync());
    p->d_seam = sc.keep(a.label);   // the device labels (the seam grid the stitch kernels read)
    p->seam_lab.swap(lab);
    p->seam_w = gw;
    p->seam_h = gh;
    p->seam_k = kk;
    p->kp.seam_hint = p->d_seam;
    p->kp.seam_w = gw;
    p->kp.seam_shift = kk;
    return MCS_OK;
}

int mcs_seam_graphcut_host(int n_cams, int gw, int gh, uint8_t *labels, const uint16_t *cover,
                           const uint8_t *samples, int channels)
{
    mcs::clear_error();
    if (!labels || !cover || !samples) return mcs::fail(MCS_E_INVALID, "NULL input");
    if (n_cams < 1 || n_cams > 16 || gw < 1 || gh < 1 || channels < 1 || channels > 4 ||
        (int64_t)gw * gh > (int64_t)1 << 28)
        return mcs::fail(MCS_E_INVALID, "n_cams %d, grid %dx%d, channels %d", n_cams, gw, gh,
                         channels);
    return mcs::seam_graphcut(n_cams, gw, gh, labels, cover, samples, channels);
}

// mcs_seam_graphcut_device on its stream s, after the checks.
static int graphcut_on_stream(const Api *A, hipStream_t s, int n_cams, int gw, int gh,
                              uint8_t *labels, const uint16_t *cover, const uint8_t *samples,
                              int channels, int device, int64_t *stats)
{
    static const char what[] = "seam graph cut";
    const size_t np = (size_t)gw * gh, sb = np * n_cams * channels;
    mcs::Scratch sc(A, s);
    uint8_t *buf = nullptr;
    HIP_TRY_AS(what, sc.dev(&buf, np * 3 + sb + 16));
    uint8_t *d_lab = buf, *d_smp = buf + np * 3 + 16;
    uint16_t *d_cov = reinterpret_cast<uint16_t *>(buf + ((np + 7) & ~(size_t)7));
    HIP_TRY_AS(what, A->hipMemcpyAsync(d_lab, labels, np, hipMemcpyHostToDevice, s));
    HIP_TRY_AS(what, A->hipMemcpyAsync(d_cov, cover, np * 2, hipMemcpyHostToDevice, s));
    HIP_TRY_AS(what, A->hipMemcpyAsync(d_smp, samples, sb, hipMemcpyHostToDevice, s));
    const int rc = mcs::seam_graphcut_device(device, s, n_cams, gw, gh, d_lab, d_cov, d_smp,
                                             channels, cover, stats);
    if (rc) return rc;
    HIP_TRY_AS(what, A->hipMemcpyAsync(labels, d_lab, np, hipMemcpyDeviceToHost, s));
    HIP_TRY_AS(what, sc.sync());
    // (this entry point has always synchronised twice here: the runtime sees the calls it saw)
    HIP_TRY_AS(what, sc.sync());
    return MCS_OK;
}

int mcs_seam_graphcut_device(int n_cams, int gw, int gh, uint8_t *labels, const uint16_t *cover,
                             const uint8_t *samples, int channels, int device, int64_t *stats)
{
    mcs::clear_error();
    if (!labels || !cover || !samples) return mcs::fail(MCS_E_INVALID, "NULL input");
    if (n_cams < 1 || n_cams > 16 || gw < 1 || gh < 1 || channels < 1 || channels > 4 ||
        (int64_t)gw * gh > (int64_t)1 << 28)
        return mcs::fail(MCS_E_INVALID, "n_cams %d, grid %dx%d, channels %d", n_cams, gw, gh,
                         channels);
    const mcs::Entry A(device);
    if (A.status) return A.status;
    hipStream_t s = nullptr;
    HIP_TRY(A->hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const int rc = graphcut_on_stream(A, s, n_cams, gw, gh, labels, cover, samples, channels,
                                      device, stats);
    (void)A->hipStreamDestroy(s);
    return rc;
}

int mcs_plan_seam_stats(const mcs_plan *p, int64_t *stats)
{
    if (!p || !stats) return mcs::fail(MCS_E_INVALID, "NULL plan/stats");
    for (int j = 0; j < 5; j++) stats[j] = p->seam_stats[j];
    return MCS_OK;
}

int mcs_plan_seam_labels(const mcs_plan *p, uint8_t *out, int *w, int *h)
{
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    if (w) *w = p->seam_w;
    if (h) *h = p->seam_h;
    if (out && !p->seam_lab.empty()) memcpy(out, p->seam_lab.data(), p->seam_lab.size());
    return MCS_OK;
}

int mcs_plan_stats(const mcs_plan *p, int64_t *stats, int n)
{
    if (!p || !stats) return mcs::fail(MCS_E_INVALID, "NULL plan/stats");
    const int64_t tiles = (int64_t)p->gx * p->gy;
    int lens_cams = 0;
    for (int c = 0; c < MCS_MAX_CAMS; c++) lens_cams += (p->kp.lens_mask >> c) & 1u;
    const int64_t v[21] = {p->t.prepared ? 1 : 0, tiles, tiles - p->t.n_fallback, p->t.n_fallback,
                           tiles * (int64_t)(sizeof(mcs::TileHdr) +
                                             mcs::kTilePx * (mcs::kDescWords + 1) * 4) +
                               (p->t.d_mbrec ? (int64_t)p->t.n_blend *
                                                   mcs::mb_rec_words(p->t.mb_slots) * 4 : 0),
                           p->blend, p->t.n_blend, p->t.mb_slots, p->t.n_degraded, p->t.n_bands,
                           p->t.n_bands_lds, p->t.n_big, p->t.mb_mixed_px, p->t.mb_r1,
                           p->t.dma_bytes, p->t.box_bytes, p->t.n_strips, p->t.sw_px,
                           (int64_t)mcs::kSwCols * p->t.sw_jb, p->t.sw_desc_rows, lens_cams};
    for (int i = 0; i < n; i++) stats[i] = i < 21 ? v[i] : 0;
    return MCS_OK;
}

int mcs_plan_footprint(mcs_plan *p, int64_t *touched_px, int n_cams)
{
    if (!p || !touched_px) return mcs::fail(MCS_E_INVALID, "NULL plan/touched_px");
    if (n_cams < p->fd.n_cams)
        return mcs::fail(MCS_E_INVALID, "n_cams %d < %d", n_cams, p->fd.n_cams);
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    int rc = ensure_stream(A, p);
    if (rc) return rc;
    const Kernels *k = nullptr;
    rc = kernels(A, p->device, &k);
    if (rc) return rc;
    rc = upload_plan_tables(A, p, p->stream);
    if (rc) return rc;
    const int n = p->fd.n_cams;
    static const char what[] = "footprint";
    uint8_t *masks[MCS_MAX_CAMS] = {};
    uint8_t **d_masks = nullptr;
    unsigned long long *d_counts = nullptr;
    unsigned long long counts[MCS_MAX_CAMS] = {};
    mcs::Scratch sc(A, p->stream);
    for (int i = 0; i < n; i++) {
        const size_t px = (size_t)p->fd.cam_w[i] * p->fd.cam_h[i];
        const size_t bytes = px > 0 ? (px + 3) / 4 * 4 : 4;
        HIP_TRY_AS(what, sc.dev(&masks[i], bytes));
        HIP_TRY_AS(what, A->hipMemsetAsync(masks[i], 0, bytes, p->stream));
    }
    HIP_TRY_AS(what, sc.dev(&d_masks, MCS_MAX_CAMS));
    HIP_TRY_AS(what, sc.dev(&d_counts, MCS_MAX_CAMS));
    HIP_TRY_AS(what, A->hipMemcpyAsync(d_masks, masks, sizeof(masks), hipMemcpyHostToDevice,
                                       p->stream));
    HIP_TRY_AS(what, A->hipMemsetAsync(d_counts, 0, sizeof(counts), p->stream));
    if (p->fd.out_w > 0 && p->fd.out_h > 0) {
        mcs::KFootprintArgs args;
        args.P = p->kp;
        args.masks = d_masks;
        args.counts = d_counts;
        rc = launch_args(A, k->footprint[p->fd.interp], (p->fd.out_w + 255) / 256, p->fd.out_h,
                         256, 1, &args, sizeof(args), p->stream);
        if (rc) return rc;
    }
    HIP_TRY_AS(what, A->hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost,
                                       p->stream));
    HIP_TRY_AS(what, sc.sync());
    for (int i = 0; i < n_cams; i++) touched_px[i] = i < n ? (int64_t)counts[i] : 0;
    return MCS_OK;
}

}  // extern "C"

// Test hook (not in mcs.h): the prepared streaming tables of a plan, copied to host buffers --
// tiles_out: TileHdr per tile, spans_out: kMaxTileJobs u16 per tile, desc_out: the full-form
// descriptors, kTilePx * kDescWords u32 per tile.  Returns the tile count (the buffers are filled
// only when all three are given and max_tiles holds it), or a negative status: the plan must be
// prepared (mcs_plan_prepare).  Reads only: the plan and its tables stay as they are.
extern "C" int mcs__plan_tile_tables(const mcs_plan *p, void *tiles_out, uint16_t *spans_out,
                                     uint32_t *desc_out, int max_tiles)
{
    mcs::clear_error();
    if (!p) return mcs::fail(MCS_E_INVALID, "NULL plan");
    if (!p->t.prepared) return mcs::fail(MCS_E_INVALID, "the plan is not prepared");
    const mcs::Entry A(p->device);
    if (A.status) return A.status;
    const size_t tiles = (size_t)p->gx * p->gy;
    if (!tiles_out || !spans_out || !desc_out || (size_t)std::max(max_tiles, 0) < tiles ||
        tiles == 0)
        return (int)tiles;
    // (prepare synchronised after building them; the copies run on the null stream)
    HIP_TRY(A->hipMemcpyAsync(tiles_out, p->t.d_tiles, tiles * sizeof(mcs::TileHdr),
                              hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(A->hipMemcpyAsync(spans_out, p->t.d_spans,
                              tiles * mcs::kMaxTileJobs * sizeof(uint16_t), hipMemcpyDeviceToHost,
                              nullptr));
    HIP_TRY(A->hipMemcpyAsync(desc_out, p->t.d_desc,
                              tiles * mcs::kTilePx * mcs::kDescWords * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(A->hipStreamSynchronize(nullptr));
    return (int)tiles;
}
