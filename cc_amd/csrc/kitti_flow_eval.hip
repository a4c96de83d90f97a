// KITTI 2015 flow and motion-segmentation evaluation (reference test_flow.py, test_mask.py, datasets/validation_flow.py,
// flowutils/flow_io.py): the 16-bit flow ground truth decoded from the inflated PNG scanlines, the rigidity composition of
// test_mask.py:129-138 whose census mask is normalised by the sample's largest flow difference, and mask_error's tp / fp / fn
// counts at the ground truth's resolution.
//
// Same conventions as kitti_eval.hip: nothing allocates or synchronises with the host, the only atomics are integer ones (a
// maximum over fp32 bit patterns, 64-bit count sums), workspaces are cleared by a kernel on the stream, and every entry can be
// captured into a graph.  The build keeps -ffp-contract=off, so du*du + dv*dv below is a rounded product, a rounded product and
// a rounded sum, as (flow_cam - flow_fwd).pow(2).sum(dim=1) is in torch; sqrt, the divide and the compares are correctly rounded
// on both sides, which makes the masks bit-exact.
#include <hip/hip_runtime.h>
#include "cc_common.h"
#include "../../include/ccengine.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kDecodeThreads = 512;     // rows of a PNG band: KITTI's 375 rows are one band
constexpr int kMaxPngWidth = 8000;      // one u64 per pixel of the carried row in LDS: 62.5 KB
constexpr int kCounts = 18;             // three masks x (tp, fp, fn of class 0, then of class 1)
constexpr int kMaxMaxBlocks = 64;       // workgroups per sample of the maximum pass
constexpr int kMaxCountBlocks = 256;

__global__ __launch_bounds__(64) void k_zero_u32(unsigned* p, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// ---------------------------------------------------------------------------------------- (a) 16-bit RGB PNG scanlines -> flow
// One pixel = 6 bytes (R, G, B samples, most significant byte first), byte k in bits 8k of a u64.  With 6 bytes per pixel the
// "left" byte of every filter is the same byte of the pixel to the left, so the six bytes of a pixel are independent.
// Predictors of the PNG specification (section 9): Sub a, Up b, Average floor((a + b) / 2), Paeth the neighbour nearest to
// a + b - c with ties in the order a, b, c (|p - a| = |b - c|, |p - b| = |a - c|, |p - c| = |a + b - 2c|).  Type 0 and any
// unknown type (which the host rejects) predict 0.  Selects instead of branches: the lanes of a wave hold rows of different types.
__device__ __forceinline__ u64 unfilter_pixel(unsigned ft, u64 raw, u64 a, u64 b, u64 c) {
    const unsigned rl = (unsigned)raw, rh = (unsigned)(raw >> 32), al = (unsigned)a, ah = (unsigned)(a >> 32);
    const unsigned bl = (unsigned)b, bh = (unsigned)(b >> 32), cl = (unsigned)c, ch = (unsigned)(c >> 32);
    unsigned ol = 0u, oh = 0u;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int sh = 8 * (k & 3);
        const int x = (int)(((k < 4 ? rl : rh) >> sh) & 255u), ak = (int)(((k < 4 ? al : ah) >> sh) & 255u);
        const int bk = (int)(((k < 4 ? bl : bh) >> sh) & 255u), ck = (int)(((k < 4 ? cl : ch) >> sh) & 255u);
        const int pa = abs(bk - ck), pb = abs(ak - ck), pc = abs(ak + bk - 2 * ck);
        const int paeth = (pa <= pb && pa <= pc) ? ak : (pb <= pc ? bk : ck);
        int pred = 0;
        pred = ft == 1u ? ak : pred;
        pred = ft == 2u ? bk : pred;
        pred = ft == 3u ? ((ak + bk) >> 1) : pred;
        pred = ft == 4u ? paeth : pred;
        const unsigned v = (unsigned)((x + pred) & 255) << sh;
        if (k < 4) ol |= v; else oh |= v;
    }
    return (u64)ol | ((u64)oh << 32);
}

__device__ __forceinline__ u64 load_pixel(const unsigned char* row, int x, int W) {
    if (row == nullptr || x < 0 || x >= W) return 0;
    const unsigned short* p = (const unsigned short*)(row + 6 * (long)x);      // rows are 8-byte aligned, 6x is even
    return (u64)p[0] | ((u64)p[1] << 16) | ((u64)p[2] << 32);
}

// One workgroup per image, one work-item per row of a band of kDecodeThreads rows, a diagonal wavefront: at step t work-item r
// reconstructs pixel t - r of its row.  The pixel above is what work-item r-1 produced one step earlier -- one __shfl_up inside
// a wave, and across a wave boundary the last lane's output, which it leaves in LDS (two slots per wave, alternating by step,
// one barrier per step); the pixel above-left is what arrived the step before; the pixel to the left is the work-item's own
// last output.  The last row of a band stays in LDS for the first row of the next band.  W + rows - 1 dependent steps per band
// instead of rows * W.  Every work-item runs every step: the shuffle and the barrier stay outside divergent control flow.
__global__ __launch_bounds__(kDecodeThreads) void k_png16_flow_decode(const unsigned char* __restrict__ ftype,
                                                                      const unsigned char* __restrict__ rows, int H, int W,
                                                                      int stride, float* __restrict__ gt) {
    HIP_DYNAMIC_SHARED(u64, carry)                                  // [W] the last row of the previous band
    __shared__ u64 edge[kDecodeThreads / kWave][2];                 // the last lane's output of every wave, by step parity
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long HW = (long)H * W;
    float* out = gt + (long)n * 3 * HW;
    for (int y0 = 0; y0 < H; y0 += kDecodeThreads) {
        const int band_rows = H - y0 < kDecodeThreads ? H - y0 : kDecodeThreads;
        const int y = y0 + tid;
        const bool live = y < H;
        const unsigned char* row = live ? rows + ((long)n * H + y) * stride : nullptr;
        const unsigned ft = live ? (unsigned)ftype[(long)n * H + y] : 0u;
        u64 cur = 0, above_left = 0;
        u64 raw = load_pixel(row, -tid, W);
        for (int t = 0; t < W + band_rows - 1; t++) {
            const int x = t - tid;
            const u64 raw_next = load_pixel(row, x + 1, W);         // issued a step ahead of its use
            u64 above = __shfl_up(cur, 1);
            const bool in = live && x >= 0 && x < W;
            if (lane == 0) {
                if (wave > 0) above = edge[wave - 1][(t + 1) & 1];  // written at step t - 1
                else above = (y0 > 0 && in) ? carry[x] : 0;
            }
            if (in) {
                const bool first = x == 0;
                cur = unfilter_pixel(ft, raw, first ? 0 : cur, above, first ? 0 : above_left);
                const unsigned R = ((unsigned)(cur & 255u) << 8) | (unsigned)((cur >> 8) & 255u);
                const unsigned G = ((unsigned)((cur >> 16) & 255u) << 8) | (unsigned)((cur >> 24) & 255u);
                const unsigned B = ((unsigned)((cur >> 32) & 255u) << 8) | (unsigned)((cur >> 40) & 255u);
                const long o = (long)y * W + x;
                out[o] = ((float)R - 32768.f) / 64.f;               // flow_io.py:114-115, exact in fp32
                out[HW + o] = ((float)G - 32768.f) / 64.f;
                out[2 * HW + o] = (float)B;
                // index t - (kDecodeThreads - 1): work-item 0 read it that many steps ago
                if (tid == kDecodeThreads - 1) carry[x] = cur;
            }
            if (lane == kWave - 1) edge[wave][t & 1] = cur;
            above_left = above;
            raw = raw_next;
            __syncthreads();
        }
    }
}

// -------------------------------------------------------------------------------- (b) test_mask.py:129-138, per-sample maximum
// pass 1: max over the sample of du*du + dv*dv as an unsigned maximum of the bit pattern with the sign cleared: non-negative
// floats order as their bits, and a NaN (exponent all ones, mantissa non-zero) beats +inf, as it wins torch.max
__global__ __launch_bounds__(kThreads) void k_census_max(const float* __restrict__ flow_cam, const float* __restrict__ flow_fwd,
                                                         int HW, unsigned* smax) {
    __shared__ unsigned red[kThreads];
    const int b = blockIdx.y;
    const float* c = flow_cam + (long)b * 2 * HW;
    const float* f = flow_fwd + (long)b * 2 * HW;
    unsigned m = 0u;
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < HW; p += gridDim.x * kThreads) {
        const float du = c[p] - f[p], dv = c[p + HW] - f[p + HW];
        const unsigned key = __float_as_uint(du * du + dv * dv) & 0x7fffffffu;
        m = key > m ? key : m;
    }
    m = cc::block_tree<kThreads, cc::Max>(m, red);
    if (threadIdx.x == 0) atomicMax(&smax[b], m);
}

struct NormOut {
    float* bare;            // [B,1,H,W]  test_mask.py:129
    float* census;          // [B,1,H,W]  :130-132
    float* combined;        // [B,1,H,W]  :134
    float* flow_non_rigid;  // [B,2,H,W]  :136
    float* flow_rigid;      // [B,2,H,W]  :137
    float* total_flow;      // [B,2,H,W]  :138
};

// pass 2.  max == 0 gives 0/0 = NaN and a NaN anywhere in the sample gives a NaN maximum: `NaN > thresh` is false, so the
// census mask is all zero in both cases, as in torch.
__global__ __launch_bounds__(kThreads) void k_rigidity_compose_norm(const float* __restrict__ exp_mask, int MC,
                                                                    const float* __restrict__ flow_cam,
                                                                    const float* __restrict__ flow_fwd, NormOut o, float thresh,
                                                                    int B, int HW, const unsigned* __restrict__ smax) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long)B * HW) return;
    const int b = (int)(i / HW), p = (int)(i - (long)b * HW);
    const float* m = exp_mask + (long)b * MC * HW + p;
    const float m1 = m[HW], m2 = m[2 * HW];
    const long f = (long)b * 2 * HW + p;
    const float cu = flow_cam[f], cv = flow_cam[f + HW], fu = flow_fwd[f], fv = flow_fwd[f + HW];
    const float bare = (1.f - (1.f - m1) * (1.f - m2)) > 0.5f ? 1.f : 0.f;
    const float du = cu - fu, dv = cv - fv;
    const float soft = 1.f - __fsqrt_rn(du * du + dv * dv) / __fsqrt_rn(__uint_as_float(smax[b]));
    const float cen = soft > thresh ? 1.f : 0.f;
    const float comb = 1.f - (1.f - bare) * (1.f - cen);
    const float nu = (1.f - comb) * fu, nv = (1.f - comb) * fv, ru = comb * cu, rv = comb * cv;
    if (o.bare) o.bare[i] = bare;
    if (o.census) o.census[i] = cen;
    if (o.combined) o.combined[i] = comb;
    if (o.flow_non_rigid) { o.flow_non_rigid[f] = nu; o.flow_non_rigid[f + HW] = nv; }
    if (o.flow_rigid) { o.flow_rigid[f] = ru; o.flow_rigid[f + HW] = rv; }
    if (o.total_flow) { o.total_flow[f] = ru + nu; o.total_flow[f + HW] = rv + nv; }
}

// ------------------------------------------------------------------------------------------------ (c) mask_error's counts
struct IouArgs {
    const unsigned char* obj_map;       // [Hg,Wg]
    const unsigned char* semantic;      // [Hg,Wg]
    const float* pred[3];               // [h,w] each, or NULL
    int Hg, Wg, h, w;
    double zy, zx;                      // (h-1)/(Hg-1), (w-1)/(Wg-1): scipy.ndimage.zoom's per-axis step
};

// zoom(order=0) along one axis: coordinate o * zoom in double, nearest = floor(c + 0.5); beyond the last input sample (a
// rounding excess of the product at the last output index) SciPy's mode 'constant' yields cval = 0 -> -1
__device__ __forceinline__ int nearest_index(int o, int n_in, double zoom) {
    const double cc = (double)o * zoom;
    if (cc > (double)(n_in - 1)) return -1;
    return (int)floor(cc + 0.5);
}

__global__ __launch_bounds__(kThreads) void k_mask_iou_counts(IouArgs a, u64* counts) {
    __shared__ unsigned tot[kCounts];
    if (threadIdx.x < kCounts) tot[threadIdx.x] = 0u;
    __syncthreads();
    unsigned acc[kCounts];
    for (int j = 0; j < kCounts; j++) acc[j] = 0u;
    const long n = (long)a.Hg * a.Wg;
    for (long q = (long)blockIdx.x * kThreads + threadIdx.x; q < n; q += (long)gridDim.x * kThreads) {
        if (a.semantic[q] != 26) continue;                          // label 255: ignored (test_mask.py:232)
        const int label = a.obj_map[q] != 0 ? 1 : 0;                // :230
        const int i = (int)(q / a.Wg), j = (int)(q - (long)i * a.Wg);
        const int yi = nearest_index(i, a.h, a.zy), xi = nearest_index(j, a.w, a.zx);
        for (int k = 0; k < 3; k++) {
            if (!a.pred[k]) continue;
            const float m = (yi < 0 || xi < 0) ? 0.f : a.pred[k][(long)yi * a.w + xi];
            const int cls = (m >= 1.f - m) ? 0 : 1;                 // argmax of [m, 1 - m], the first maximum wins (:241-246)
            unsigned* c = acc + 6 * k;
            if (cls == label) {
                c[3 * label] += 1u;                                 // tp
            } else {
                c[3 * cls + 1] += 1u;                               // fp of the predicted class
                c[3 * label + 2] += 1u;                             // fn of the true class
            }
        }
    }
    for (int j = 0; j < kCounts; j++)
        if (acc[j]) atomicAdd(&tot[j], acc[j]);
    __syncthreads();
    if (threadIdx.x < kCounts && tot[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (u64)tot[threadIdx.x]);
}

}  // namespace

extern "C" {

int cc_png16_flow_decode(const unsigned char* ftype, const unsigned char* rows, int N, int H, int W, int stride, float* gt,
                         void* stream) {
    if (!ftype || !rows || !gt || N <= 0 || H <= 0 || W <= 0 || W > kMaxPngWidth) return CC_ERR_ARG;
    if (stride < 6 * W || (stride & 7) != 0) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_png16_flow_decode, dim3(N), dim3(kDecodeThreads), (size_t)W * sizeof(u64), (hipStream_t)stream, ftype, rows, H, W,
                       stride, gt);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

size_t cc_rigidity_compose_norm_ws(int B) { return B > 0 ? (size_t)B * sizeof(unsigned) : 0; }

int cc_rigidity_compose_norm(const float* exp_mask, int MC, const float* flow_cam, const float* flow_fwd, float* bare,
                             float* census, float* combined, float* flow_non_rigid, float* flow_rigid, float* total_flow,
                             float thresh, int B, int H, int W, void* ws, void* stream) {
    if (!exp_mask || !flow_cam || !flow_fwd || !ws || MC < 3 || B <= 0 || H <= 0 || W <= 0) return CC_ERR_ARG;
    if ((long)H * W > 0x3fffffffl) return CC_ERR_ARG;
    const hipStream_t s = (hipStream_t)stream;
    const int HW = H * W;
    unsigned* smax = (unsigned*)ws;
    hipLaunchKernelGGL(k_zero_u32, dim3((B + 63) / 64), dim3(64), 0, s, smax, B);
    CC_CHECK_LAUNCH();
    int nblk = (HW + kThreads - 1) / kThreads;
    nblk = nblk < kMaxMaxBlocks ? nblk : kMaxMaxBlocks;
    hipLaunchKernelGGL(k_census_max, dim3(nblk, B), dim3(kThreads), 0, s, flow_cam, flow_fwd, HW, smax);
    CC_CHECK_LAUNCH();
    NormOut o = {bare, census, combined, flow_non_rigid, flow_rigid, total_flow};
    const long n = (long)B * HW;
    hipLaunchKernelGGL(k_rigidity_compose_norm, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, exp_mask, MC,
                       flow_cam, flow_fwd, o, thresh, B, HW, (const unsigned*)smax);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_mask_iou_counts(const unsigned char* obj_map, const unsigned char* semantic, int Hg, int Wg, const float* pred0,
                       const float* pred1, const float* pred2, int h, int w, unsigned long long* counts, void* stream) {
    if (!obj_map || !semantic || !counts || Hg < 2 || Wg < 2 || h < 2 || w < 2) return CC_ERR_ARG;
    IouArgs a;
    a.obj_map = obj_map;
    a.semantic = semantic;
    a.pred[0] = pred0;
    a.pred[1] = pred1;
    a.pred[2] = pred2;
    a.Hg = Hg;
    a.Wg = Wg;
    a.h = h;
    a.w = w;
    a.zy = (double)(h - 1) / (double)(Hg - 1);
    a.zx = (double)(w - 1) / (double)(Wg - 1);
    long nblk = ((long)Hg * Wg + kThreads - 1) / kThreads;
    nblk = nblk < kMaxCountBlocks ? nblk : kMaxCountBlocks;
    hipLaunchKernelGGL(k_mask_iou_counts, dim3((unsigned)nblk), dim3(kThreads), 0, (hipStream_t)stream, a, counts);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
