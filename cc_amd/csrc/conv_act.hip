// Activation backward and bias gradients of the convolution layers: geff = gy * act'(y) fused with the per-channel sums of the
// bias gradient (k_act_bwd + k_bias_reduce), and the bias gradients a backward stage has parked, in one launch (k_bias_table).
#include <stddef.h>
#include "cc_common.h"
#include "conv_internal.h"
#include "conv_tail.h"
#include "../../include/ccengine.h"

namespace {

using namespace cctail;
using ccint::MAXGRP;

// ------------------------------------------------------------------ activation backward + bias gradient
// geff = gy * act'(y) (in place allowed);  partial[m][n*cpp + chunk] = sum over the chunk of geff.
// grid (cpp, C, B): one (image, channel) plane chunk per workgroup -> no per-element index arithmetic, float4 accesses
// when the plane size allows (HBM-bound: 2 reads + 1 write per element).

struct AB {      // up to MAXGRP same-shaped problems per launch: blockIdx.z = problem * zper + image
    const float* gy[MAXGRP]; const float* y[MAXGRP]; float* geff[MAXGRP]; float* partial[MAXGRP]; float* gbias_direct[MAXGRP];
    int zper;
};

template <bool VEC4>
__global__ __launch_bounds__(256) void k_act_bwd(AB t, int HW, long gy_bs, long y_bs, long ge_bs, int act, float act_a,
                                                 float act_b, int nb, int accum) {
    __shared__ float red[4];
    const int grp = (int)blockIdx.z / t.zper, zimg = (int)blockIdx.z - grp * t.zper;
    const float* __restrict__ gy = t.gy[grp];
    const float* __restrict__ y = t.y[grp];
    float* __restrict__ geff = t.geff[grp];
    float* __restrict__ partial = t.partial[grp];
    float* __restrict__ gbias_direct = t.gbias_direct[grp];
    const int m = blockIdx.y, cpp = gridDim.x;
    float s[1] = {0.f};
    // nb == 1: this workgroup owns image zimg; nb == B (small maps, zper == 1): it walks all images itself and
    // writes the channel's bias gradient directly (no second-stage launch)
    for (int nn = 0; nn < nb; nn++) {
        const int n = zimg + nn;
        const float* __restrict__ gp = gy + (long)n * gy_bs + (long)m * HW;
        const float* __restrict__ yp = (act != ACT_NONE) ? y + (long)n * y_bs + (long)m * HW : nullptr;
        float* __restrict__ ep = geff ? geff + (long)n * ge_bs + (long)m * HW : nullptr;
        if (VEC4) {
            // four iterations' loads (up to 8 x 16 bytes) in flight per work item; same element order as a one-by-one loop
            const int nq = HW >> 2, stp = cpp * 256;
            for (int q0 = blockIdx.x * 256 + threadIdx.x; q0 < nq; q0 += 4 * stp) {
                float4 gg[4], vv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int q = q0 + u * stp;
                    gg[u] = (q < nq) ? ((const float4*)gp)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                    vv[u] = (q < nq && act != ACT_NONE) ? ((const float4*)yp)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int q = q0 + u * stp;
                    if (q < nq) {
                        float4 g = gg[u];
                        if (act != ACT_NONE) {
                            g.x = act_grad(g.x, vv[u].x, act, act_a, act_b);
                            g.y = act_grad(g.y, vv[u].y, act, act_a, act_b);
                            g.z = act_grad(g.z, vv[u].z, act, act_a, act_b);
                            g.w = act_grad(g.w, vv[u].w, act, act_a, act_b);
                        }
                        if (ep) ((float4*)ep)[q] = g;
                        s[0] += (g.x + g.y) + (g.z + g.w);
                    }
                }
            }
        } else {
            for (int e = blockIdx.x * 256 + threadIdx.x; e < HW; e += cpp * 256) {
                float g = gp[e];
                if (act != ACT_NONE) g = act_grad(g, yp[e], act, act_a, act_b);
                if (ep) ep[e] = g;
                s[0] += g;
            }
        }
    }
    cc::block_sum_256<1>(s, red);
    if (threadIdx.x == 0) {
        if (gbias_direct) gbias_direct[m] = accum ? (gbias_direct[m] + s[0]) : s[0];
        else if (partial) partial[(long)m * (cpp * t.zper) + zimg * cpp + blockIdx.x] = s[0];
    }
}

struct BR { const float* partial[MAXGRP]; float* gbias[MAXGRP]; };

__global__ __launch_bounds__(64) void k_bias_reduce(BR t, int nchunk, int accum) {
    const float* __restrict__ partial = t.partial[blockIdx.y];
    float* __restrict__ gbias = t.gbias[blockIdx.y];
    const int m = blockIdx.x;
    float s = 0.f;
    for (int k = threadIdx.x; k < nchunk; k += 64) s += partial[(long)m * nchunk + k];
    s = cc::wave_sum(s);
    if (threadIdx.x == 0) gbias[m] = accum ? (gbias[m] + s) : s;
}

}  // namespace

extern "C" {

// Bias gradients of a whole backward stage in ONE launch.  With the activation derivative applied in the data-gradient epilogues
// (planned backward), the per-layer pass left over is a pure reduction of the pre-activation gradient over (B, H, W): 84 launches
// of 5-8 us per step.  The trainer parks them (the gradients stay alive for the parked weight-gradient launches anyway) and
// cc_bias_grad_table sums up to NBJ layers per launch; per-chunk partials are finished by cc_wgrad_reduce_table (kind 4), small
// maps are written directly -- block decomposition and summation order are k_act_bwd's.
constexpr int NBJ = 32;
struct BJ {
    const float* gy; float* partial; float* gbias; long gy_bs;
    int B, C, HW, cpp, single, accum, vec4, blk_end;
};
struct BT { BJ j[NBJ]; int n; };

__global__ __launch_bounds__(256) void k_bias_table(BT t) {
    __shared__ float red[4];
    int k = 0, first = 0;
#pragma unroll 1
    for (int q = 0; q + 1 < t.n; q++)
        if ((int)blockIdx.x >= t.j[q].blk_end) { k = q + 1; first = t.j[q].blk_end; }
    const BJ& j = t.j[k];
    const int bid = (int)blockIdx.x - first;
    const int per_m = j.single ? 1 : j.B * j.cpp;                 // workgroups per channel
    const int m = bid / per_m, rem = bid - m * per_m;
    const int zimg = j.single ? 0 : rem / j.cpp, chunk = j.single ? 0 : rem - zimg * j.cpp;
    const int cpp = j.single ? 1 : j.cpp, nb = j.single ? j.B : 1, HW = j.HW;
    float s[1] = {0.f};
    for (int nn = 0; nn < nb; nn++) {
        const float* __restrict__ gp = j.gy + (long)(zimg + nn) * j.gy_bs + (long)m * HW;
        if (j.vec4) {
            const int nq = HW >> 2, stp = cpp * 256;
            for (int q0 = chunk * 256 + threadIdx.x; q0 < nq; q0 += 4 * stp) {
                float4 gg[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int q = q0 + u * stp;
                    gg[u] = (q < nq) ? ((const float4*)gp)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (q0 + u * stp < nq) s[0] += (gg[u].x + gg[u].y) + (gg[u].z + gg[u].w);
            }
        } else {
            for (int e = chunk * 256 + threadIdx.x; e < HW; e += cpp * 256) s[0] += gp[e];
        }
    }
    cc::block_sum_256<1>(s, red);
    if (threadIdx.x == 0) {
        if (j.single) j.gbias[m] = j.accum ? (j.gbias[m] + s[0]) : s[0];
        else j.partial[(long)m * (j.cpp * j.B) + zimg * j.cpp + chunk] = s[0];
    }
}

size_t cc_act_bwd_ws_bytes(int C) { return (size_t)C * 64 * sizeof(float); }

/* geff = gy * act'(y) (geff may alias gy or be null), gbias[c] = sum_{n,p} geff (gbias may be null).
 * Group form: G (<= 4) same-shaped problems per launch; gy / y / geff / gbias: HOST arrays of device addresses (0 = null,
 * uniformly over the group); ws: G areas of cc_act_bwd_ws_bytes(C) each. */
static int act_bwd_bias_impl(int G, const long* gy, const long* y, const long* geff, const long* gbias, float* ws, int B, int C, int H,
                             int W, long gy_bs, long y_bs, long geff_bs, int act, float act_a, float act_b, int accumulate_bias,
                             void* stream, ccint::RedSink* sink) {
    if (G <= 0 || G > MAXGRP || B <= 0 || C <= 0) return CC_ERR_ARG;
    const bool has_y = y && y[0], has_ge = geff && geff[0], has_gb = gbias && gbias[0];
    if (act != ACT_NONE && !has_y) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W;
    int cpp = (HW + 8191) / 8192;                       // chunks per (image, channel) plane; B * cpp <= 64 partials per channel
    const int cap = 64 / B > 0 ? 64 / B : 1;
    cpp = cpp < 1 ? 1 : (cpp > cap ? cap : cpp);
    if (B > 64) return CC_ERR_ARG;
    bool vec4 = (HW % 4 == 0) && (gy_bs % 4 == 0) && (y_bs % 4 == 0) && (geff_bs % 4 == 0);
    for (int k = 0; k < G; k++)
        vec4 = vec4 && ((((uintptr_t)gy[k]) | (uintptr_t)(has_y ? y[k] : 0) | (uintptr_t)(has_ge ? geff[k] : 0)) % 16 == 0);
    // small maps with enough channels to occupy the chip: one workgroup per channel, bias gradient written in place
    const bool single = ((long)B * HW <= 32768) && ((long)C * B * HW * G <= (1l << 22) || (long)C * G >= 128);
    const int nb = single ? B : 1;
    const size_t wstride = cc_act_bwd_ws_bytes(C) / sizeof(float);
    AB t = {};
    BR r = {};
    t.zper = single ? 1 : B;
    for (int k = 0; k < G; k++) {
        t.gy[k] = (const float*)gy[k];
        t.y[k] = has_y ? (const float*)y[k] : nullptr;
        t.geff[k] = has_ge ? (float*)geff[k] : nullptr;
        t.gbias_direct[k] = (single && has_gb) ? (float*)gbias[k] : nullptr;
        t.partial[k] = (has_gb && !single) ? ws + k * wstride : nullptr;
        r.partial[k] = t.partial[k];
        r.gbias[k] = has_gb ? (float*)gbias[k] : nullptr;
    }
    dim3 grid(single ? 1 : cpp, C, (single ? 1 : B) * G);
    const int nchunk = single ? 1 : cpp * B;
    if (vec4)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_act_bwd<true>), grid, dim3(256), 0, s, t, HW, gy_bs, y_bs, geff_bs, act, act_a, act_b,
                           nb, accumulate_bias);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_act_bwd<false>), grid, dim3(256), 0, s, t, HW, gy_bs, y_bs, geff_bs, act, act_a, act_b,
                           nb, accumulate_bias);
    if (has_gb && !single) {
        if (sink) {      // second stage parked: kind 4 of the reduce table (same per-channel summation as k_bias_reduce)
            for (int k = 0; k < G; k++) {
                const long d[ccint::RD_LONGS] = {4, (long)r.partial[k], (long)r.gbias[k], nchunk, accumulate_bias, 0, 0, C};
                if (ccint::wgrad_reduce_emit(sink, d, 1, s) != CC_OK) return CC_ERR_ARG;
            }
        } else {
            hipLaunchKernelGGL(k_bias_reduce, dim3(C, G), dim3(64), 0, s, r, nchunk, accumulate_bias);
        }
    }
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_act_bwd_bias_group(int G, const long* gy, const long* y, const long* geff, const long* gbias, float* ws, int B, int C, int H,
                          int W, long gy_bs, long y_bs, long geff_bs, int act, float act_a, float act_b, int accumulate_bias,
                          void* stream) {
    return act_bwd_bias_impl(G, gy, y, geff, gbias, ws, B, C, H, W, gy_bs, y_bs, geff_bs, act, act_a, act_b, accumulate_bias, stream,
                             nullptr);
}

/* ... with the second stage of the bias gradient (sum of the per-chunk partials in ws) left to the caller: descriptors for
 * cc_wgrad_reduce_table (16 longs each, at most G, none when the kernel wrote gbias itself) go to red_host[0 .. *nred_host);
 * ws must stay untouched until that call. */
int cc_act_bwd_bias_group_defer(int G, const long* gy, const long* y, const long* geff, const long* gbias, float* ws, int B, int C,
                                int H, int W, long gy_bs, long y_bs, long geff_bs, int act, float act_a, float act_b,
                                int accumulate_bias, long* red_host, int red_cap, int* nred_host, void* stream) {
    if (!red_host || !nred_host || red_cap < G) return CC_ERR_ARG;
    ccint::RedSink sink = {red_host, red_cap, 0};
    const int rc = act_bwd_bias_impl(G, gy, y, geff, gbias, ws, B, C, H, W, gy_bs, y_bs, geff_bs, act, act_a, act_b, accumulate_bias,
                                     stream, &sink);
    *nred_host = sink.n;
    return rc;
}

/* Bias gradient gbias[c] (+)= sum_{n,h,w} gy[n,c,h,w], parked: nothing is launched.  job_host[12] receives the job for
 * cc_bias_grad_table; when the map is large enough to be summed in chunks, red_host[16] receives the descriptor of the second
 * stage for cc_wgrad_reduce_table and *nred_host = 1 (else 0).  ws: cc_act_bwd_ws_bytes(C) bytes, untouched until both ran. */
int cc_bias_grad_defer(const float* gy, float* gbias, float* ws, int B, int C, int H, int W, long gy_bs, int accumulate,
                       long* job_host, long* red_host, int* nred_host) {
    if (!gy || !gbias || !job_host || !red_host || !nred_host || B <= 0 || B > 64 || C <= 0 || H <= 0 || W <= 0) return CC_ERR_ARG;
    const int HW = H * W;
    int cpp = (HW + 8191) / 8192;                       // as act_bwd_bias_impl
    const int cap = 64 / B > 0 ? 64 / B : 1;
    cpp = cpp < 1 ? 1 : (cpp > cap ? cap : cpp);
    const bool vec4 = (HW % 4 == 0) && (gy_bs % 4 == 0) && (((uintptr_t)gy) % 16 == 0);
    // one workgroup per channel (no second stage) only where it walks <= 4096 elements: in a table launch the longest job
    // sets the duration (k_act_bwd's own threshold is 32768: there a second launch would cost more than the walk)
    const bool single = (long)B * HW <= 4096;
    if (!single && !ws) return CC_ERR_ARG;
    const long job[12] = {(long)gy, single ? 0 : (long)ws, (long)gbias, gy_bs, B, C, HW, cpp, single ? 1 : 0, accumulate ? 1 : 0,
                          vec4 ? 1 : 0, 0};
    for (int i = 0; i < 12; i++) job_host[i] = job[i];
    *nred_host = 0;
    if (!single) {
        const long d[ccint::RD_LONGS] = {4, (long)ws, (long)gbias, (long)cpp * B, accumulate ? 1 : 0, 0, 0, C};
        for (int i = 0; i < ccint::RD_LONGS; i++) red_host[i] = d[i];
        *nred_host = 1;
    }
    return CC_OK;
}

/* Run n parked bias-gradient jobs (12 longs each, from cc_bias_grad_defer): one launch per 32. */
int cc_bias_grad_table(const long* jobs_host, int n, void* stream) {
    if (!jobs_host || n <= 0) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    for (int j0 = 0; j0 < n; j0 += NBJ) {
        BT t = {};
        int bx = 0;
        t.n = n - j0 < NBJ ? n - j0 : NBJ;
        for (int k = 0; k < t.n; k++) {
            const long* d = jobs_host + (long)(j0 + k) * 12;
            BJ& j = t.j[k];
            j.gy = (const float*)d[0]; j.partial = (float*)d[1]; j.gbias = (float*)d[2]; j.gy_bs = d[3];
            j.B = (int)d[4]; j.C = (int)d[5]; j.HW = (int)d[6]; j.cpp = (int)d[7]; j.single = (int)d[8]; j.accum = (int)d[9];
            j.vec4 = (int)d[10];
            if (!j.gy || !j.gbias || j.B <= 0 || j.C <= 0 || j.HW <= 0 || j.cpp <= 0 || (!j.single && !j.partial)) return CC_ERR_ARG;
            bx += j.single ? j.C : j.C * j.B * j.cpp;
            j.blk_end = bx;
        }
        hipLaunchKernelGGL(k_bias_table, dim3((unsigned)bx), dim3(256), 0, s, t);
    }
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_act_bwd_bias(const float* gy, const float* y_or_null, float* geff_or_null, float* gbias_or_null, float* ws, int B,
                    int C, int H, int W, long gy_bs, long y_bs, long geff_bs, int act, float act_a, float act_b,
                    int accumulate_bias, void* stream) {
    const long a = (long)gy, b = (long)y_or_null, c = (long)geff_or_null, d = (long)gbias_or_null;
    return cc_act_bwd_bias_group(1, &a, &b, &c, &d, ws, B, C, H, W, gy_bs, y_bs, geff_bs, act, act_a, act_b, accumulate_bias, stream);
}

}  // extern "C"
