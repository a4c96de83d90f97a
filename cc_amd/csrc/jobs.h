// "Job table" launches: ONE kernel launch over a list of same-kind work items of different sizes -- the (pyramid level,
// reference frame) terms of a loss (loss_functions.py loops `for scale ... for ref ...`, 24-36 terms per loss per step).
// A job = 8 pointer-sized slots + (H, W); the table travels in the kernel arguments (< 2 KB), blocks are dealt to jobs by a
// prefix table, so the six pyramid levels (212 992 ... 208 pixels per image) share one well-filled grid instead of six
// launches of which the small ones are pure launch latency.
#pragma once
#include "cc_common.h"

namespace ccjobs {

constexpr int MAXJOBS = 24;
constexpr int SLOTS = 8;
constexpr int JOB_LONGS = SLOTS + 2;        // host layout of one job: slots[8], H, W

struct JobTab {
    int n, B;
    int blk_end[MAXJOBS];       // cumulative block count (job j owns blocks [blk_end[j-1], blk_end[j]))
    int H[MAXJOBS], W[MAXJOBS];
    long slot[MAXJOBS][SLOTS];
};

// blocks per (job, batch item): pixel kernels use ceil(H*W / 256) -- ceil(that / PPT) where a work-item takes PPT pixels, 256 apart;
// tile kernels ceil(W/T)*ceil(H/T)
inline int pix_blocks(int H, int W) { return (H * W + 255) / 256; }
template <int PPT>
inline int pix_blocks_ppt(int H, int W) { return (pix_blocks(H, W) + PPT - 1) / PPT; }

// fill a table from the host job array; blocks_per_image(H, W) -> blocks one image of that size needs; -> total blocks
template <class F>
inline int fill(JobTab& t, const long* jobs, int njobs, int B, F blocks_per_image) {
    t.n = njobs;
    t.B = B;
    int tot = 0;
    for (int j = 0; j < njobs; j++) {
        const long* q = jobs + (long)j * JOB_LONGS;
        for (int k = 0; k < SLOTS; k++) t.slot[j][k] = q[k];
        t.H[j] = (int)q[SLOTS];
        t.W[j] = (int)q[SLOTS + 1];
        tot += B * blocks_per_image(t.H[j], t.W[j]);
        t.blk_end[j] = tot;
    }
    return tot;
}

// the argument check of every *_jobs entry point, then fill -> total blocks, or -1
template <class F>
inline int table(JobTab& t, const long* jobs, int njobs, int B, F blocks_per_image) {
    if (!jobs || njobs <= 0 || njobs > MAXJOBS || B <= 0) return -1;
    return fill(t, jobs, njobs, B, blocks_per_image);
}

// block index -> (job, first block of the job).  n <= 24: a scalar linear scan
__device__ __forceinline__ int find(const JobTab& t, int bx, int& first) {
    int j = 0;
    first = 0;
    for (int q = 0; q + 1 < t.n; q++)
        if (bx >= t.blk_end[q]) { j = q + 1; first = t.blk_end[q]; }
    return j;
}

// ... -> (job, index of the block INSIDE the job in XCD order, cc_common.h): a job's blocks are consecutive pieces of its images, so
// every XCD works through a contiguous band of rows -- the rows a bilinear gather or a stencil shares with the piece above / below
// are then fetched into ONE L2 (the warp kernels moved 1.3-1.7x their distinct bytes with the blocks dealt round-robin)
__device__ __forceinline__ int find_xcd(const JobTab& t, int bx, int& local) {
    int first;
    const int j = find(t, bx, first);
    local = (CC_XCD_MASK & 8) ? cc_xcd_order(bx - first, t.blk_end[j] - first) : bx - first;
    return j;
}

template <class T>
__device__ __forceinline__ T* ptr(const JobTab& t, int j, int k) { return reinterpret_cast<T*>(t.slot[j][k]); }

// Where this workgroup's pixels are.  A job's images (table B of them: batch items or planes) are cut into nb 256-pixel pieces; a
// workgroup owns PPT consecutive pieces of image b, from piece blk * PPT on (tables filled with pix_blocks_ppt<PPT>).  XCD: the
// job's workgroups in XCD order (find_xcd) or in launch order (find).
struct Pieces { int j, b, H, W, HW, nb, blk; };
template <int PPT, bool XCD>
__device__ __forceinline__ Pieces pieces(const JobTab& t) {
    Pieces w;
    int first, local;
    if (XCD) {
        w.j = find_xcd(t, (int)blockIdx.x, local);
    } else {
        w.j = find(t, (int)blockIdx.x, first);
        local = (int)blockIdx.x - first;
    }
    w.H = t.H[w.j];
    w.W = t.W[w.j];
    w.HW = w.H * w.W;
    w.nb = (w.HW + 255) >> 8;
    const int per_image = (w.nb + PPT - 1) / PPT;
    w.b = local / per_image;
    w.blk = local - w.b * per_image;
    return w;
}
// ... one piece per workgroup: p = this work-item's pixel (>= HW beyond the end of a ragged last piece)
struct Piece { int j, b, H, W, HW, nb, p; };
template <bool XCD>
__device__ __forceinline__ Piece piece(const JobTab& t) {
    const Pieces w = pieces<1, XCD>(t);
    return {w.j, w.b, w.H, w.W, w.HW, w.nb, w.blk * 256 + (int)threadIdx.x};
}

// ---- pixel functions with a kernel in more than one file
// loss_functions.py:343-352 occlusion_masks: occ = sum_c(f_fw + f_bw) > 0.08*(|f_fw|^2 + |f_bw|^2) + 1
// (signed sum; occ_fw == occ_bw).  -> (1 - occ), the factor the losses multiply by.
__device__ __forceinline__ float noocc(float bu, float bv, float fu, float fv) {
    const float mag = (fu * fu + fv * fv) + (bu * bu + bv * bv);
    const float thr = 0.08f * mag + 1.0f;
    const float s = (fu + bu) + (fv + bv);
    return (s > thr) ? 0.f : 1.f;
}

// loss_functions.py:189-193: target = (wrig * min(err_cf, err_cb) * (valid_cf OR valid_cb) <= err_ff + 1e-8), element i
__device__ __forceinline__ void consensus_combine_px(const float* __restrict__ err_cf, const float* __restrict__ err_cb,
                                                     const float* __restrict__ err_ff, const float* __restrict__ v_cf,
                                                     const float* __restrict__ v_cb, float* __restrict__ target, float wrig, size_t i) {
    const float valid = 1.f - (1.f - v_cf[i]) * (1.f - v_cb[i]);
    const float cam_err = fminf(err_cf[i], err_cb[i]) * valid;
    target[i] = (wrig * cam_err <= (err_ff[i] + 1e-8f)) ? 1.f : 0.f;
}

}  // namespace ccjobs
