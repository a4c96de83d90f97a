// Validation metrics (reference loss_functions.py:355-467, consumed by train.py:588-777): flow end-point
// errors / Fl outliers (flow_diff, compute_epe, outlier_err, compute_all_epes) and the Eigen depth errors (compute_errors) on the
// device, without a host synchronisation, so that a validation pass can be captured into a hipGraph.
//
// Determinism: float sums are fp64 per-thread accumulators, a fixed LDS tree per workgroup (cc::block_tree), a per-workgroup slab in the caller's
// workspace and a fixed-order final reduce; only the integer radix histograms of the exact depth medians use global atomics.
// The bilinear resizes follow F.interpolate(mode='bilinear', align_corners=False) tap for tap (the build keeps -ffp-contract=off).
#include <hip/hip_runtime.h>
#include "cc_common.h"
#include "radix_select.h"
#include "../../include/ccengine.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFlowSums = 7;        // per rigidity mask: epe, valid, rigid epe, rigid valid, non-rigid epe, non-rigid valid, outliers
constexpr int kMaxMasks = 2;
constexpr int kMaxFlowBlocks = 512;
constexpr int kDepthSums = 6;       // per sample: sum |d|, sum |d|/gt, sum d^2/gt, counts of thresh < 1.25, 1.25^2, 1.25^3
constexpr int kMaxDepthBlocks = 64; // per sample
using ccradix::kBins;

// upsample_bilinear2d, align_corners=False: src = max(scale*(dst+0.5)-0.5, 0), i1 = i0+1 only while i0 < in-1
struct Tap {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Tap tap_of(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Tap t;
    t.i0 = (int)src;
    if (t.i0 > in - 1) t.i0 = in - 1;
    t.i1 = t.i0 + ((t.i0 < in - 1) ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

__device__ __forceinline__ float lerp2(const Tap& ty, const Tap& tx, float v00, float v01, float v10, float v11) {
    return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

struct MaskIn {
    const float* m;     // [B,1,H,W]
    int H, W, inv;      // inv: the mask is 1 - m (the ground-truth object map of validate_flow_with_gt, train.py:748)
};

__device__ __forceinline__ float mask_at(const MaskIn& k, long base, int y, int x) {
    const float v = k.m[base + (long)y * k.W + x];
    return k.inv ? 1.f - v : v;
}

// the mask resized to (Ho, Wo), at output pixel (y, x) of image b
__device__ __forceinline__ float mask_resized(const MaskIn& k, int b, int y, int x, int Ho, int Wo) {
    const Tap ty = tap_of(y, k.H, Ho), tx = tap_of(x, k.W, Wo);
    const long base = (long)b * k.H * k.W;
    return lerp2(ty, tx, mask_at(k, base, ty.i0, tx.i0), mask_at(k, base, ty.i0, tx.i1), mask_at(k, base, ty.i1, tx.i0),
                 mask_at(k, base, ty.i1, tx.i1));
}

struct FlowArgs {
    const float* gt;            // [B,Cg,Hg,Wg]
    const float* rigid;         // [B,2,Hp,Wp]
    const float* non_rigid;     // [B,2,Hp,Wp] or NULL (no mask)
    MaskIn mask[kMaxMasks];
    int nmasks, B, Cg, Hg, Wg, Hp, Wp;
    float thresh, tau_px, tau_rel;
    float* epe_map;             // [B,Hg,Wg] or NULL
};

__device__ __forceinline__ float epe_of(float ug, float vg, float up, float vp) {
    const float du = ug - up, dv = vg - vp;
    return sqrtf(du * du + dv * dv);
}

__host__ __device__ inline int flow_blocks(int B, int Hg, int Wg) {
    const long n = (long)B * Hg * Wg;
    const long nb = (n + kThreads - 1) / kThreads;
    return (int)(nb < kMaxFlowBlocks ? nb : kMaxFlowBlocks);
}

// cc_flow_metrics_samples: the ground truth of sample s of the launch is row idx[s] of a device table, so one launch shape serves
// batches whose ground truths differ in size
struct FlowTable {
    const float* flow_pool;     // (u, v, valid) planes, [3,Hg,Wg] per sample at its flow offset
    const float* obj_pool;      // object maps, [Hg,Wg] per sample at its obj-map offset
    const long* table;          // [N,4] {flow offset, obj-map offset, Hg, Wg}, offsets in floats
    const int* idx;             // [B] table rows of this batch
    long flow_floats, obj_floats, max_px;
    int N, slab;                // slab: the workgroups (partial slots) a sample owns = flow_blocks(1, max_px)
};

// row idx[s] of the table; false for a row that is outside the table, larger than max_px or reaches outside a pool
__device__ __forceinline__ bool table_row(const FlowTable& t, int s, long& fo, long& oo, int& Hg, int& Wg) {
    const int r = t.idx[s];
    if (r < 0 || r >= t.N) return false;
    const long* row = t.table + 4 * (long)r;
    fo = row[0];
    oo = row[1];
    const long h = row[2], w = row[3];
    if (h <= 0 || w <= 0 || h > t.max_px || w > t.max_px || h * w > t.max_px) return false;     // max_px < 2^31: no overflow
    if (fo < 0 || oo < 0 || fo > t.flow_floats - 3 * h * w || oo > t.obj_floats - h * w) return false;
    Hg = (int)h;
    Wg = (int)w;
    return true;
}

// one pass over the ground-truth pixels; per mask k the seven sums of compute_all_epes (loss_functions.py:411-429), or with no
// mask the epe / valid / outlier sums of compute_epe and outlier_err (:368-409) in the same slots
// NV = max(nmasks, 1), a template argument so that the accumulators stay in registers
// TABLE: workgroup (x, s) of a kMaxFlowBlocks-wide grid works on sample s alone, as workgroup x of the flow_blocks(1, Hg, Wg) that
// cc_flow_metrics launches for that sample at B = 1 -- the same stride, accumulators and tree, hence the same sums; the surplus
// workgroups return at once
template <int NV, bool TABLE>
__global__ __launch_bounds__(kThreads) void k_flow_metrics(FlowArgs a, FlowTable t, double* partial) {
    __shared__ double red[kThreads];
    int nblk = gridDim.x;
    if (TABLE) {
        const int s = blockIdx.y;
        long fo, oo;
        int Hg, Wg;
        if (!table_row(t, s, fo, oo, Hg, Wg)) return;
        nblk = flow_blocks(1, Hg, Wg);
        if ((int)blockIdx.x >= nblk) return;
        const long HWp = (long)a.Hp * a.Wp;
        a.gt = t.flow_pool + fo;
        a.rigid += (long)s * 2 * HWp;
        a.non_rigid += (long)s * 2 * HWp;
        a.mask[0].m += (long)s * a.mask[0].H * a.mask[0].W;
        a.mask[1] = MaskIn{t.obj_pool + oo, Hg, Wg, 1};
        a.B = 1;
        a.Cg = 3;
        a.Hg = Hg;
        a.Wg = Wg;
        partial += (long)s * t.slab * NV * kFlowSums;
    }
    double acc[NV * kFlowSums];
#pragma unroll
    for (int i = 0; i < NV * kFlowSums; i++) acc[i] = 0.0;
    const long HWg = (long)a.Hg * a.Wg, HWp = (long)a.Hp * a.Wp, n = (long)a.B * HWg;
    const float su = (float)((double)a.Wg / (double)a.Wp), sv = (float)((double)a.Hg / (double)a.Hp);
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)nblk * kThreads) {
        const int b = (int)(i / HWg);
        const long p = i - (long)b * HWg;
        const int y = (int)(p / a.Wg), x = (int)(p - (long)y * a.Wg);
        const float* g = a.gt + (long)b * a.Cg * HWg + p;
        const float ug = g[0], vg = g[HWg];
        const float valid = a.Cg == 3 ? g[2 * HWg] : 1.f;
        const Tap ty = tap_of(y, a.Hp, a.Hg), tx = tap_of(x, a.Wp, a.Wg);
        const long q[4] = {(long)ty.i0 * a.Wp + tx.i0, (long)ty.i0 * a.Wp + tx.i1, (long)ty.i1 * a.Wp + tx.i0,
                           (long)ty.i1 * a.Wp + tx.i1};
        const int qy[4] = {ty.i0, ty.i0, ty.i1, ty.i1}, qx[4] = {tx.i0, tx.i1, tx.i0, tx.i1};
        const float* r = a.rigid + (long)b * 2 * HWp;
        const float mag = sqrtf(ug * ug + vg * vg);
#pragma unroll
        for (int k = 0; k < NV; k++) {
            float ru[4], rv[4], nu[4] = {0.f, 0.f, 0.f, 0.f}, nvv[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < 4; j++) {
                ru[j] = r[q[j]];
                rv[j] = r[HWp + q[j]];
            }
            float wg_r = 0.f, wg_n = 0.f;
            if (a.nmasks > 0) {
                const float* nr = a.non_rigid + (long)b * 2 * HWp;
                for (int j = 0; j < 4; j++) {
                    // (mask resized to the prediction > THRESH) * pred, loss_functions.py:418-419
                    const float mp = mask_resized(a.mask[k], b, qy[j], qx[j], a.Hp, a.Wp);
                    const float wr = mp > a.thresh ? 1.f : 0.f, wn = mp <= a.thresh ? 1.f : 0.f;
                    ru[j] = wr * ru[j];
                    rv[j] = wr * rv[j];
                    nu[j] = wn * nr[q[j]];
                    nvv[j] = wn * nr[HWp + q[j]];
                }
                const float mg = mask_resized(a.mask[k], b, y, x, a.Hg, a.Wg);
                wg_r = mg > a.thresh ? 1.f : 0.f;
                wg_n = mg <= a.thresh ? 1.f : 0.f;
            }
            float tu[4], tv[4];
            for (int j = 0; j < 4; j++) {
                tu[j] = a.nmasks > 0 ? nu[j] + ru[j] : ru[j];          // total_pred = non_rigid_pred + rigid_pred, :420
                tv[j] = a.nmasks > 0 ? nvv[j] + rv[j] : rv[j];
            }
            const float up = lerp2(ty, tx, tu[0], tu[1], tu[2], tu[3]) * su;
            const float vp = lerp2(ty, tx, tv[0], tv[1], tv[2], tv[3]) * sv;
            const float e = epe_of(ug, vg, up, vp);
            if (a.epe_map && k == 0) a.epe_map[i] = e;
            const float ev = e * valid;
            double* s = acc + k * kFlowSums;
            s[0] += (double)ev;
            s[1] += (double)valid;
            // outlier_err, :390-409: (epe > 3) * (epe / (|gt| + 1e-8) > 0.05) * valid with epe = epe * valid
            if (ev > a.tau_px && ev / (mag + 1e-8f) > a.tau_rel) s[6] += (double)valid;
            if (a.nmasks > 0) {
                // gt_rigid / gt_non_rigid: the ground-truth-size mask on every channel of gt, :422-423
                const float rup = lerp2(ty, tx, ru[0], ru[1], ru[2], ru[3]) * su;
                const float rvp = lerp2(ty, tx, rv[0], rv[1], rv[2], rv[3]) * sv;
                const float nup = lerp2(ty, tx, nu[0], nu[1], nu[2], nu[3]) * su;
                const float nvp = lerp2(ty, tx, nvv[0], nvv[1], nvv[2], nvv[3]) * sv;
                const float vr = a.Cg == 3 ? wg_r * valid : 1.f, vn = a.Cg == 3 ? wg_n * valid : 1.f;
                s[2] += (double)(epe_of(wg_r * ug, wg_r * vg, rup, rvp) * vr);
                s[3] += (double)vr;
                s[4] += (double)(epe_of(wg_n * ug, wg_n * vg, nup, nvp) * vn);
                s[5] += (double)vn;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NV * kFlowSums; j++) {
        const double t = cc::block_tree<kThreads, cc::Sum>(acc[j], red);
        if (threadIdx.x == 0) partial[(long)blockIdx.x * NV * kFlowSums + j] = t;
    }
}

// the workgroups' partials summed in workgroup order -> the metrics of one cc_flow_metrics call (one workgroup of 64 threads)
__device__ __forceinline__ void flow_finish(const double* partial, int nblocks, int nmasks, int Cg, long npix, float* out, double* tot) {
    const int nv = nmasks > 0 ? nmasks : 1, ns = nv * kFlowSums;
    const int t = threadIdx.x;
    if (t < ns) {
        double s = 0.0;
        for (int blk = 0; blk < nblocks; blk++) s += partial[(long)blk * ns + t];
        tot[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    // compute_epe, :379-385: sum(epe * valid) / (sum(valid) + 1e-8) with a validity channel, else the plain mean
    auto epe = [&](double e, double v) { return Cg == 3 ? (float)(e / (v + 1e-8)) : (float)(e / (double)npix); };
    const float nan = __int_as_float(0x7fc00000);
    for (int k = 0; k < nv; k++) {
        const double* s = tot + k * kFlowSums;
        const float outl = Cg == 3 ? (float)(s[6] / (s[1] + 1e-8)) : nan;
        if (nmasks == 0) {
            out[0] = epe(s[0], s[1]);
            out[1] = outl;
        } else {
            out[4 * k + 0] = epe(s[0], s[1]);
            out[4 * k + 1] = epe(s[2], s[3]);
            out[4 * k + 2] = epe(s[4], s[5]);
            out[4 * k + 3] = outl;
        }
    }
}

__global__ __launch_bounds__(64) void k_flow_finish(const double* partial, int nblocks, int nmasks, int Cg, long npix, float* out) {
    __shared__ double tot[kMaxMasks * kFlowSums];
    flow_finish(partial, nblocks, nmasks, Cg, npix, out, tot);
}

// workgroup s: row s of out [B,8] from the sample's own partials; NaN for a row that table_row refuses
__global__ __launch_bounds__(64) void k_flow_finish_samples(const double* partial, FlowTable t, float* out) {
    __shared__ double tot[kMaxMasks * kFlowSums];
    const int s = blockIdx.x;
    long fo, oo;
    int Hg, Wg;
    if (!table_row(t, s, fo, oo, Hg, Wg)) {
        if (threadIdx.x < 2 * 4) out[(long)s * 8 + threadIdx.x] = __int_as_float(0x7fc00000);
        return;
    }
    flow_finish(partial + (long)s * t.slab * 2 * kFlowSums, flow_blocks(1, Hg, Wg), 2, 3, (long)Hg * Wg, out + (long)s * 8, tot);
}

// the meter: one workgroup adds the B rows to the running fp64 sums in sample order, and B to the count
__global__ __launch_bounds__(64) void k_flow_accumulate(const float* out, int B, double* sums, long* count) {
    const int t = threadIdx.x;
    if (t < 8) {
        double s = sums[t];
        for (int b = 0; b < B; b++) s += (double)out[(long)b * 8 + t];
        sums[t] = s;
    }
    if (t == 0) count[0] += (long)B;
}

// ------------------------------------------------------------------------------------------------------------- depth errors
// workspace: hist [B][2][kBins] u32 | state [B][2][4] u32 (prefix, rank, count, nan count) | partial [B][nblk][kDepthSums] f64
struct DepthArgs {
    const float* gt;        // [B,H,W]
    const float* pred;      // [B,H,W]
    int B, H, W, y1, y2, x1, x2;
};

__device__ __forceinline__ float clamp_depth(float p) {       // torch.clamp(p, 1e-3, 80): NaN stays NaN
    return p != p ? p : (p < 1e-3f ? 1e-3f : (p > 80.f ? 80.f : p));
}

// radix-select pass `pass` (radix_select.h) of the lower medians of valid gt and valid clamped pred: histogram of the keys that
// match the digits selected so far.  Valid keys are positive fp32, so their bits order as integers.
__global__ __launch_bounds__(kThreads) void k_depth_hist(DepthArgs a, unsigned* hist, unsigned* state, int pass) {
    __shared__ unsigned h[2 * kBins];
    ccradix::clear<kThreads>(h, 2 * kBins);
    const int b = blockIdx.y;
    unsigned* st = state + (long)b * 8;
    const unsigned pre_g = st[0], pre_p = st[4];
    const int bw = a.x2 - a.x1;
    const long n = (long)(a.y2 - a.y1) * bw;
    unsigned nan_p = 0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        const int y = a.y1 + (int)(i / bw), x = a.x1 + (int)(i - (long)(i / bw) * bw);
        const long o = (long)b * a.H * a.W + (long)y * a.W + x;
        const float g = a.gt[o];
        if (!(g > 0.f && g < 80.f)) continue;
        const float p = clamp_depth(a.pred[o]);
        ccradix::count_key(h, __float_as_uint(g), pre_g, pass);
        if (p != p) {
            nan_p++;
            continue;
        }
        ccradix::count_key(h + kBins, __float_as_uint(p), pre_p, pass);
    }
    if (pass == 0 && nan_p) atomicAdd(&st[7], nan_p);
    ccradix::flush<kThreads>(h, hist + (long)b * 2 * kBins, 2 * kBins);
}

// one thread per (sample, array): torch.median's lower median
__global__ __launch_bounds__(64) void k_depth_select(unsigned* hist, unsigned* state, int B, int pass) {
    const int t = threadIdx.x + blockIdx.x * 64;
    if (t >= 2 * B) return;
    ccradix::select(hist + (long)t * kBins, state + (long)t * 4, pass, false);
}

// compute_errors, loss_functions.py:446-465: per-pixel terms of the median-scaled prediction -> per-workgroup fp64 partials
__global__ __launch_bounds__(kThreads) void k_depth_terms(DepthArgs a, const unsigned* state, double* partial) {
    __shared__ double red[kThreads];
    const int b = blockIdx.y;
    const float mg = ccradix::median_of(state + (long)b * 8), mp = ccradix::median_of(state + (long)b * 8 + 4);
    const int bw = a.x2 - a.x1;
    const long n = (long)(a.y2 - a.y1) * bw;
    double acc[kDepthSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        const int y = a.y1 + (int)(i / bw), x = a.x1 + (int)(i - (long)(i / bw) * bw);
        const long o = (long)b * a.H * a.W + (long)y * a.W + x;
        const float g = a.gt[o];
        if (!(g > 0.f && g < 80.f)) continue;
        const float p = (clamp_depth(a.pred[o]) * mg) / mp;
        const float r0 = g / p, r1 = p / g;
        const float th = (r0 != r0 || r1 != r1) ? __int_as_float(0x7fc00000) : (r0 > r1 ? r0 : r1);   // torch.max propagates NaN
        const float d = fabsf(g - p), d2 = (g - p) * (g - p);
        acc[0] += (double)d;
        acc[1] += (double)(d / g);
        acc[2] += (double)(d2 / g);
        acc[3] += th < 1.25f ? 1.0 : 0.0;
        acc[4] += th < 1.5625f ? 1.0 : 0.0;
        acc[5] += th < 1.953125f ? 1.0 : 0.0;
    }
    for (int j = 0; j < kDepthSums; j++) {
        const double t = cc::block_tree<kThreads, cc::Sum>(acc[j], red);
        if (threadIdx.x == 0) partial[((long)b * gridDim.x + blockIdx.x) * kDepthSums + j] = t;
    }
}

// six means per sample, summed over samples in order and divided by B (fp32, as the reference's running `+=` and `/ batch_size`)
__global__ __launch_bounds__(64) void k_depth_finish(const double* partial, const unsigned* state, int B, int nblk, float* out) {
    if (threadIdx.x != 0) return;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; b++) {
        double s[kDepthSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int blk = 0; blk < nblk; blk++)
            for (int j = 0; j < kDepthSums; j++) s[j] += partial[((long)b * nblk + blk) * kDepthSums + j];
        const unsigned cnt = state[(long)b * 8 + 2];
        const double nd = (double)cnt;
        const float nf = (float)cnt;
        const float m[6] = {(float)(s[0] / nd), (float)(s[1] / nd), (float)(s[2] / nd), (float)s[3] / nf, (float)s[4] / nf,
                            (float)s[5] / nf};
        for (int j = 0; j < 6; j++) acc[j] = b == 0 ? m[j] : acc[j] + m[j];
    }
    for (int j = 0; j < 6; j++) out[j] = acc[j] / (float)B;
}

int depth_blocks(int H, int W) {
    const long nb = ((long)H * W + kThreads - 1) / kThreads;
    return (int)(nb < kMaxDepthBlocks ? nb : kMaxDepthBlocks);
}

size_t depth_counts_bytes(int B) { return (size_t)B * 2 * (kBins + 4) * sizeof(unsigned); }

}  // namespace

extern "C" {

size_t cc_flow_metrics_ws(int B, int Hg, int Wg, int nmasks) {
    if (B <= 0 || Hg <= 0 || Wg <= 0 || nmasks < 0 || nmasks > kMaxMasks) return 0;
    const int nv = nmasks > 0 ? nmasks : 1;
    return (size_t)flow_blocks(B, Hg, Wg) * nv * kFlowSums * sizeof(double);
}

int cc_flow_metrics(const float* gt, int Cg, int Hg, int Wg, const float* rigid_pred, const float* non_rigid_pred, int Hp, int Wp,
                    const float* mask0, int Hm0, int Wm0, int inv0, const float* mask1, int Hm1, int Wm1, int inv1, float thresh,
                    float tau_px, float tau_rel, int B, float* epe_map, float* out, void* ws, void* stream) {
    const int nmasks = mask0 ? (mask1 ? 2 : 1) : 0;
    if (!gt || !rigid_pred || !out || !ws || B <= 0 || (Cg != 2 && Cg != 3) || Hg <= 0 || Wg <= 0 || Hp <= 0 || Wp <= 0)
        return CC_ERR_ARG;
    if (mask1 && !mask0) return CC_ERR_ARG;
    if ((nmasks > 0) != (non_rigid_pred != nullptr)) return CC_ERR_ARG;
    if ((mask0 && (Hm0 <= 0 || Wm0 <= 0)) || (mask1 && (Hm1 <= 0 || Wm1 <= 0))) return CC_ERR_ARG;
    FlowArgs a;
    a.gt = gt;
    a.rigid = rigid_pred;
    a.non_rigid = non_rigid_pred;
    a.mask[0] = MaskIn{mask0, Hm0, Wm0, inv0};
    a.mask[1] = MaskIn{mask1, Hm1, Wm1, inv1};
    a.nmasks = nmasks;
    a.B = B;
    a.Cg = Cg;
    a.Hg = Hg;
    a.Wg = Wg;
    a.Hp = Hp;
    a.Wp = Wp;
    a.thresh = thresh;
    a.tau_px = tau_px;
    a.tau_rel = tau_rel;
    a.epe_map = epe_map;
    const int nblk = flow_blocks(B, Hg, Wg);
    double* partial = (double*)ws;
    if (nmasks == 2)
        hipLaunchKernelGGL((k_flow_metrics<2, false>), dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, a, FlowTable{}, partial);
    else
        hipLaunchKernelGGL((k_flow_metrics<1, false>), dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, a, FlowTable{}, partial);
    CC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_flow_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partial, nblk, nmasks, Cg,
                       (long)B * Hg * Wg, out);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

size_t cc_flow_metrics_samples_ws(int B, long max_px) {
    if (B <= 0 || max_px < 1 || max_px > 0x7fffffffL) return 0;
    return (size_t)B * flow_blocks(1, 1, (int)max_px) * 2 * kFlowSums * sizeof(double);
}

int cc_flow_metrics_samples(const float* flow_pool, long flow_floats, const float* obj_pool, long obj_floats, const long* table, int N,
                            const int* idx, int B, long max_px, const float* rigid_pred, const float* non_rigid_pred, int Hp, int Wp,
                            const float* mask0, int Hm0, int Wm0, float thresh, float tau_px, float tau_rel, float* out,
                            double* acc_sums, long* acc_count, void* ws, void* stream) {
    if (!flow_pool || !obj_pool || !table || !idx || !rigid_pred || !non_rigid_pred || !mask0 || !out || !ws) return CC_ERR_ARG;
    if ((acc_sums != nullptr) != (acc_count != nullptr)) return CC_ERR_ARG;
    if (B <= 0 || B > 65535 || N <= 0 || max_px < 1 || max_px > 0x7fffffffL || flow_floats < 3 || obj_floats < 1) return CC_ERR_ARG;
    if (Hp <= 0 || Wp <= 0 || Hm0 <= 0 || Wm0 <= 0) return CC_ERR_ARG;
    FlowArgs a;
    a.gt = nullptr;
    a.rigid = rigid_pred;
    a.non_rigid = non_rigid_pred;
    a.mask[0] = MaskIn{mask0, Hm0, Wm0, 0};
    a.mask[1] = MaskIn{nullptr, 0, 0, 1};
    a.nmasks = 2;
    a.B = 1;
    a.Cg = 3;
    a.Hg = a.Wg = 0;
    a.Hp = Hp;
    a.Wp = Wp;
    a.thresh = thresh;
    a.tau_px = tau_px;
    a.tau_rel = tau_rel;
    a.epe_map = nullptr;
    FlowTable t;
    t.flow_pool = flow_pool;
    t.obj_pool = obj_pool;
    t.table = table;
    t.idx = idx;
    t.flow_floats = flow_floats;
    t.obj_floats = obj_floats;
    t.max_px = max_px;
    t.N = N;
    t.slab = flow_blocks(1, 1, (int)max_px);
    double* partial = (double*)ws;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((k_flow_metrics<2, true>), dim3(t.slab, B), dim3(kThreads), 0, s, a, t, partial);
    CC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_flow_finish_samples, dim3(B), dim3(64), 0, s, (const double*)partial, t, out);
    CC_CHECK_LAUNCH();
    if (acc_sums) {
        hipLaunchKernelGGL(k_flow_accumulate, dim3(1), dim3(64), 0, s, (const float*)out, B, acc_sums, acc_count);
        CC_CHECK_LAUNCH();
    }
    return CC_OK;
}

size_t cc_depth_errors_ws(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return depth_counts_bytes(B) + (size_t)B * depth_blocks(H, W) * kDepthSums * sizeof(double);
}

int cc_depth_errors(const float* gt, const float* pred, int B, int H, int W, int y1, int y2, int x1, int x2, float* out6, void* ws,
                    void* stream) {
    if (!gt || !pred || !out6 || !ws || B <= 0 || H <= 0 || W <= 0) return CC_ERR_ARG;
    if (y1 < 0 || x1 < 0 || y2 > H || x2 > W || y1 > y2 || x1 > x2) return CC_ERR_ARG;
    const hipStream_t s = (hipStream_t)stream;
    unsigned* hist = (unsigned*)ws;
    unsigned* state = hist + (size_t)B * 2 * kBins;
    double* partial = (double*)((char*)ws + depth_counts_bytes(B));   // 8-byte aligned: (kBins + 4) * 2 * 4 bytes per sample
    if (hipMemsetAsync(ws, 0, depth_counts_bytes(B), s) != hipSuccess) return CC_ERR_LAUNCH;
    const DepthArgs a = {gt, pred, B, H, W, y1, y2, x1, x2};
    const int nblk = depth_blocks(H, W);
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(k_depth_hist, dim3(nblk, B), dim3(kThreads), 0, s, a, hist, state, pass);
        CC_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_depth_select, dim3((2 * B + 63) / 64), dim3(64), 0, s, hist, state, B, pass);
        CC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_depth_terms, dim3(nblk, B), dim3(kThreads), 0, s, a, (const unsigned*)state, partial);
    CC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_depth_finish, dim3(1), dim3(64), 0, s, (const double*)partial, (const unsigned*)state, B, nblk, out6);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
