// mcs_feat_int.h -- internals of the estimation module shared by its host files
// (mcs_features.cpp: the per-call entry points; mcs_rig.cpp: a whole rig capture per launch
// chain).  Not part of the C ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "mcs_common.h"
#include "mcs_fparams.h"

namespace mcs {
namespace feat {

// The feature code object's kernels on one device (looked up once).
struct FeatureKernels {
    bool loaded = false;
    hipFunction_t knn2 = nullptr, knn2_finalize = nullptr;
    hipFunction_t ransac_score = nullptr, ransac_mask = nullptr;
    hipFunction_t orb_gray = nullptr, orb_level = nullptr, orb_describe = nullptr;
    hipFunction_t orb_pyramid = nullptr;
    hipFunction_t orb_select = nullptr;
    hipFunction_t l2_prep = nullptr, l2_i8 = nullptr, l2_f32 = nullptr, l2_finalize = nullptr;
    hipFunction_t rig_knn2 = nullptr, rig_match = nullptr, rig_ransac = nullptr,
                  rig_best = nullptr, rig_hyp = nullptr, rig_unlens = nullptr;
    hipFunction_t seam_init = nullptr, seam_hinit = nullptr, seam_push = nullptr,
                  seam_active = nullptr, seam_label = nullptr, seam_relabel_lds = nullptr;
};
int feature_kernels(const rt::Api *A, int device, const FeatureKernels **out);
// hipModuleLaunchKernel with the argument block passed by value (grid gx x gy x gz).
int launch(const rt::Api *A, hipFunction_t f, unsigned gx, unsigned gy, unsigned bx, void *args,
           size_t sz, hipStream_t s, unsigned gz = 1, unsigned lds = 0);

// ORB's level geometry, as OpenCV's ORB computes it (float arithmetic): level sizes, scales and
// per-level keypoint quotas; the level images' pixel offsets (256-aligned) and the candidate
// buffer's per-level capacity / offset.
struct OrbGeom {
    int nlevels = 0;
    int lw[12] = {0}, lh[12] = {0}, quota[12] = {0};
    float lscale[12] = {0};
    size_t off[13] = {0};
    size_t cap[12] = {0}, coff[13] = {0}, cap_total = 0;
    int n_bound = 0;   // sum of the quotas: keypoints per frame at most
};
int orb_geom(int w, int h, int nfeatures, int nlevels, float scale_factor, OrbGeom *g);
// mcs_orb_pyramid's arguments for the levels of `g` (level images at lvl + off[l]); the block
// count, 0 when the one-launch pyramid does not apply (the per-level resize chain then does).
unsigned pyramid_args(const OrbGeom &g, uint8_t *lvl, KOrbBuildArgs &a);

// The device buffers of an ORB chain over n_frames frames, laid out by the caller; frame c's part:
// lvl / blur + c geo.off[nlevels], cand + c geo.cap_total, ncand + c kOrbMaxLevels, kp + 3 c K,
// resp + c K, desc + 32 c K, orient + 2 c K, sel + 2 c.
struct OrbBuffers {
    uint8_t *lvl, *blur;
    OrbCand *cand;
    int *ncand, *kp;
    double *resp;
    uint8_t *desc;
    double *orient;
    int *sel;   // [n, overflow] per frame
};
// ORB's launch chain for n_frames equal frames (grid.y = frame): gray, pyramid (one launch, or
// the per-level resize chain when pyr_blocks == 0), mcs_orb_level, mcs_orb_select,
// mcs_orb_describe.  The per-call entry points are its n_frames = 1 case, the rig job its
// n_frames = cameras case.
struct OrbChain {
    OrbGeom geo;
    int w = 0, h = 0, n_frames = 0;
    int K = 0;   // keypoints per frame at most (>= 1): the per-frame stride
    unsigned pyr_blocks = 0;
    KGrayArgs ga;
    KOrbBuildArgs ba;
    KOrbPyrArgs pa;
    KOrbSelArgs sa;
    KOrbDescArgs da;
};
// Fills the chain for the buffers `b` -- the one place the five argument blocks are filled.
// c->geo is orb_geom's of the frames already (the caller lays its buffers out from it).
void orb_chain(OrbChain *c, int w, int h, int fast_threshold, int n_frames, const OrbBuffers &b);
// Enqueues the chain on stream s for n_frames device frames of 1 or 3 channels.  The candidate
// counts are zero on entry (the reset is the caller's); the argument blocks stay in the chain (a
// captured graph's kernel nodes keep them for replays).
int orb_enqueue(const rt::Api *A, const FeatureKernels *k, OrbChain &c,
                const uint8_t *const *frames, int channels, int device, hipStream_t s);

// The Hamming kNN-2's grid for `queries` descriptors against `train`, `pairs` such sets in one
// launch: enough (query wave x train chunk x pair) blocks to fill the chip twice over (16384
// waves: 16 per SIMD, the compare loop's LDS-read latency needs them; 4096 left waves waiting on
// it half their cycles) with chunks of >= 64 descriptors (3 atomics per query and chunk).
struct KnnShape {
    unsigned qblocks, chunks;   // chunks == 0: no train descriptor, no launch
    int per_chunk;
};
KnnShape knn_shape(int queries, int pairs, int train);

}  // namespace feat
}  // namespace mcs
