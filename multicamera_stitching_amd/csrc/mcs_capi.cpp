// mcs_capi.cpp -- the extern "C" boundary of libmcs.so (declared in include/mcs.h), but for the
// device-resident stitch entry points (mcs_stitch.cpp) and those of the seams (mcs_seam.cpp).
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
    rc = kernels(A, p, &k);
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
    return mcs_plan_set_lens_model(p, cam, MCS_LENS_PINHOLE, K, dist, n_dist);
}

int mcs_plan_set_lens_model(mcs_plan *p, int cam, int model, const double *K, const double *dist,
                            int n_dist)
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
        const int rc = mcs::lens_from(K, dist, n_dist, &L, model);
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
        p->fish_mask = (p->fish_mask & ~(1u << cam)) | (model == MCS_LENS_FISHEYE ? 1u << cam : 0u);
    } else {
        p->lens[cam] = mcs::Lens();
        p->kp.lens_mask &= ~(1u << cam);
        p->fish_mask &= ~(1u << cam);
    }
    p->lens_stale = true;
    return MCS_OK;
}

int mcs_lens_map_host(const double *K, const double *dist, int n_dist, const double *uv, int n,
                      double *xy, double *r2max)
{
    return mcs_lens_map_host_model(MCS_LENS_PINHOLE, K, dist, n_dist, uv, n, xy, r2max);
}

int mcs_lens_map_host_model(int model, const double *K, const double *dist, int n_dist,
                            const double *uv, int n, double *xy, double *r2max)
{
    mcs::clear_error();
    if (!K || (n_dist > 0 && !dist) || n < 0 || (n > 0 && (!uv || !xy)))
        return mcs::fail(MCS_E_INVALID, "NULL K/dist/uv/xy");
    mcs::Lens L;
    const int rc = mcs::lens_from(K, dist, n_dist < 0 ? 0 : n_dist, &L, model);
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
    return mcs_lens_unmap_host_model(MCS_LENS_PINHOLE, K, dist, n_dist, xy, n, uv);
}

int mcs_lens_unmap_host_model(int model, const double *K, const double *dist, int n_dist,
                              const double *xy, int n, double *uv)
{
    mcs::clear_error();
    if (!K || (n_dist > 0 && !dist) || n < 0 || (n > 0 && (!xy || !uv)))
        return mcs::fail(MCS_E_INVALID, "NULL K/dist/xy/uv");
    mcs::Lens L;
    const int rc = mcs::lens_from(K, dist, n_dist < 0 ? 0 : n_dist, &L, model);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        double u = std::nan(""), v = std::nan("");
        (void)mcs::lens_invert(L, xy[2 * i], xy[2 * i + 1], u, v);
        uv[2 * i] = u;
        uv[2 * i + 1] = v;
    }
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
    rc = kernels(A, p, &k);
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
