// Per-parameter-tensor statistics of the flat buckets: for every parameter, the L2 norm of its gradient and of its weights, the
// largest |gradient| and the number of gradient elements that are NaN / Inf -- what a training log plots per layer and what answers
// "which layer blew up" (the gradient guard, grad_guard.hip, reports per NETWORK).  One sweep over flat_g and flat_p, two launches,
// no host sync, no atomics, nothing cleared beforehand, the same bits on every call:
//   k_param_chunk   one workgroup per chunk (<= CC_PARAM_STATS_CHUNK floats of ONE parameter, host-built table): fp64 accumulation,
//                   a fixed assignment of elements to work-items and a fixed reduction tree (cc::block_tree); every workgroup stores its four
//                   partials unconditionally.  A parameter starts at any offset of the bucket (only a network's start is 256-byte
//                   aligned): 16-byte loads on the aligned interior, scalar loads on the <= 3 elements in front of and behind it.
//                   HBM-bound (2 x 297 MB for the four networks): like k_grad_sumsq, a work-item has kLoads independent 16-byte
//                   loads of each bucket in flight before it consumes the first.
//   k_param_finish  one work-item per parameter sums its chunks' partials in chunk order.
#include "cc_common.h"
#include "../../include/ccengine.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLoads = 4;               // independent 16-byte loads per bucket a work-item issues before it consumes the first one
constexpr long kChunk = CC_PARAM_STATS_CHUNK;

struct Acc {
    double gs, ps;
    float mx;
    int nf;
};

__device__ __forceinline__ void add1(Acc& a, float g, float p) {
    a.gs += (double)g * (double)g;
    a.ps += (double)p * (double)p;
    const float m = fabsf(g);
    if (m > a.mx) a.mx = m;                             // (a NaN compares false: it is counted, not propagated)
    if (!(m <= 3.402823466e+38f)) a.nf += 1;
}

__device__ __forceinline__ void add4(Acc& a, const float4 g, const float4 p) {
    add1(a, g.x, p.x);
    add1(a, g.y, p.y);
    add1(a, g.z, p.z);
    add1(a, g.w, p.w);
}

__global__ __launch_bounds__(kThreads) void k_param_chunk(const float* __restrict__ g, const float* __restrict__ p, long n,
                                                          const long* __restrict__ chunks, double* __restrict__ partials) {
    __shared__ double red[kThreads];
    const int t = threadIdx.x;
    const long off = chunks[2 * (long)blockIdx.x], len = chunks[2 * (long)blockIdx.x + 1];
    double* out = partials + 4 * (long)blockIdx.x;
    if (off < 0 || len < 0 || len > kChunk || off > n - len) {           // a table that does not fit the bucket: nothing is read
        if (t == 0) out[0] = out[1] = out[2] = out[3] = (double)__int_as_float(0x7fc00000);
        return;
    }
    const float* gc = g + off;
    const float* pc = p + off;
    int head = (int)((4 - (off & 3)) & 3);              // elements in front of the first 16-byte boundary (both buckets: same offset)
    if (head > len) head = (int)len;
    const int n4 = (int)((len - head) >> 2), tail0 = head + 4 * n4, tail = (int)len - tail0;
    Acc a = {0.0, 0.0, 0.f, 0};
    if (t < head) add1(a, gc[t], pc[t]);
    if (t < tail) add1(a, gc[tail0 + t], pc[tail0 + t]);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(gc + head);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(pc + head);
    int i = t;
    for (; i + (kLoads - 1) * kThreads < n4; i += kLoads * kThreads) {
        float4 x[kLoads], y[kLoads];
#pragma unroll
        for (int k = 0; k < kLoads; k++) x[k] = g4[i + k * kThreads];
#pragma unroll
        for (int k = 0; k < kLoads; k++) y[k] = p4[i + k * kThreads];
#pragma unroll
        for (int k = 0; k < kLoads; k++) add4(a, x[k], y[k]);
    }
    for (; i < n4; i += kThreads) add4(a, g4[i], p4[i]);
    const double gs = cc::block_tree<kThreads, cc::Sum>(a.gs, red);
    const double ps = cc::block_tree<kThreads, cc::Sum>(a.ps, red);
    const double mx = cc::block_tree<kThreads, cc::Max>((double)a.mx, red);
    const double nf = cc::block_tree<kThreads, cc::Sum>((double)a.nf, red);
    if (t == 0) {
        out[0] = gs;
        out[1] = ps;
        out[2] = mx;
        out[3] = nf;
    }
}

__global__ __launch_bounds__(kThreads) void k_param_finish(const double* __restrict__ partials, const long* __restrict__ param_first,
                                                           int nparams, float grad_scale, double* __restrict__ stats) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= nparams) return;
    double gs = 0.0, ps = 0.0, mx = 0.0, nf = 0.0;
    for (long c = param_first[j]; c < param_first[j + 1]; c++) {
        const double* q = partials + 4 * c;
        gs += q[0];
        ps += q[1];
        if (q[2] > mx) mx = q[2];
        nf += q[3];
    }
    stats[4 * (long)j + 0] = (double)grad_scale * sqrt(gs);
    stats[4 * (long)j + 1] = sqrt(ps);
    stats[4 * (long)j + 2] = mx;
    stats[4 * (long)j + 3] = nf;
}

}  // namespace

extern "C" {

int cc_param_stats_chunks(const float* flat_g, const float* flat_p, long n, const long* chunks, int nchunks, double* partials,
                          void* stream) {
    if (!flat_g || !flat_p || n <= 0 || !chunks || nchunks <= 0 || !partials || (((uintptr_t)flat_g | (uintptr_t)flat_p) & 15) != 0)
        return CC_ERR_ARG;
    hipLaunchKernelGGL(k_param_chunk, dim3((unsigned)nchunks), dim3(kThreads), 0, (hipStream_t)stream, flat_g, flat_p, n, chunks,
                       partials);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_param_stats_finish(const double* partials, const long* param_first, int nparams, float grad_scale, double* stats,
                          void* stream) {
    if (!partials || !param_first || nparams <= 0 || !stats) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_param_finish, dim3((unsigned)((nparams + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       partials, param_first, nparams, grad_scale, stats);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
