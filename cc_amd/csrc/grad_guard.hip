// Gradient guard of the in-graph Adam step, per network: the L2 norm of the network's segment of the gradient bucket, clipping to
// a per-network max_grad_norm (torch.nn.utils.clip_grad_norm_'s formula) and an exact no-op when the segment holds a NaN or Inf.
// Three launches on the network's stream, no host sync, no atomics, nothing cleared beforehand:
//   k_grad_sumsq   stage 1 of a deterministic two-stage reduction: a fixed grid sweeps the segment (HBM-bound, up to 55 M floats
//                  for DispResNet6), squares and accumulates in fp64 (|g| > 1.8e19 does not overflow: a finite gradient has a
//                  finite sum) and every workgroup stores ONE fp64 partial, unconditionally;
//   k_guard_finish one workgroup sums the partials in a fixed order and writes the network's guard row
//                  {norm, coef, finite, skipped, 0, 0, 0, 0} (skipped is a running count: += 1 per non-finite step);
//   k_adam_guard   k_adam_hyper's update of one row -- the one body of adam_update.h -- with the gradient multiplied by coef, the
//                  bias corrections taken at t = step - skipped (a skipped step does not count for this network) and NO store at
//                  all when finite == 0.
// With coef == 1 and skipped == 0 the update is k_adam_hyper's bit for bit (x * 1.0f and t - 0.0f are exact, -ffp-contract=off).
#include "adam_update.h"
#include "../../include/ccengine.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLoads = 4;               // independent 16-byte loads a work-item issues before it consumes the first one
constexpr int kMaxBlocks = CC_GRAD_GUARD_MAX_BLOCKS;      // 4 workgroups (16 waves, 64 KB of loads in flight) per CU on 256 CUs

__device__ __forceinline__ double sumsq4(double acc, const float4 x) {
    acc += (double)x.x * (double)x.x;
    acc += (double)x.y * (double)x.y;
    acc += (double)x.z * (double)x.z;
    acc += (double)x.w * (double)x.w;
    return acc;
}

// g: 16-byte aligned.  Work-item w of the grid's T = gridDim.x * 256 owns the float4s w, w + T, w + 2T, ...: a set that depends on
// (n, grid) only, summed in that order -> the same bits on every call.  The n % 4 elements behind the last float4 go to work-item 0.
__global__ __launch_bounds__(kThreads) void k_grad_sumsq(const float* __restrict__ g, long n, double* __restrict__ partials) {
    __shared__ double red[kThreads];
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    const long n4 = n >> 2, T = (long)gridDim.x * kThreads;
    long i = (long)blockIdx.x * kThreads + threadIdx.x;
    double acc = 0.0;
    for (; i + (kLoads - 1) * T < n4; i += kLoads * T) {
        float4 x[kLoads];
#pragma unroll
        for (int k = 0; k < kLoads; k++) x[k] = g4[i + k * T];
#pragma unroll
        for (int k = 0; k < kLoads; k++) acc = sumsq4(acc, x[k]);
    }
    for (; i < n4; i += T) acc = sumsq4(acc, g4[i]);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long j = n4 << 2; j < n; j++) acc += (double)g[j] * (double)g[j];
    const double s = cc::block_tree<kThreads, cc::Sum>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void k_guard_finish(const double* __restrict__ partials, int nblocks,
                                                           const float* __restrict__ hyper_row, float grad_scale,
                                                           float* __restrict__ guard_row) {
    __shared__ double red[kThreads];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kThreads) acc += partials[b];
    const double sumsq = cc::block_tree<kThreads, cc::Sum>(acc, red);
    if (threadIdx.x != 0) return;
    const bool finite = sumsq <= 1.7976931348623157e308;          // (a sum of squares: >= 0, +Inf or NaN)
    const float norm = (float)((double)grad_scale * sqrt(sumsq));
    const float max_norm = hyper_row[5];
    float coef = 0.f;
    if (finite) {
        coef = 1.f;
        if (max_norm > 0.f && max_norm < __int_as_float(0x7f800000)) coef = fminf(1.f, max_norm / (norm + 1e-6f));
    }
    guard_row[0] = norm;
    guard_row[1] = coef;
    guard_row[2] = finite ? 1.f : 0.f;
    guard_row[3] += finite ? 0.f : 1.f;
    guard_row[4] = guard_row[5] = guard_row[6] = guard_row[7] = 0.f;
}

__global__ __launch_bounds__(kThreads) void k_adam_guard(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, long n, const float* __restrict__ h,
                                                         const float* __restrict__ guard, const float* __restrict__ step,
                                                         float grad_scale) {
    const long i4 = ((long)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (guard[2] == 0.f) return;            // a NaN / Inf in this network's gradient: p, m, v keep their bits
    const bool full = i4 + 3 < n;
    ccadam::Quad q;
    if (full) ccadam::load4(q, p, g, m, v, i4);
    const ccadam::Coefs c = ccadam::coefs(h[0], h[1], h[2], h[3], h[4], step[0] - guard[3], grad_scale, guard[1]);
    ccadam::update4<true, true>(p, g, m, v, i4, n, full, q, c);
}

int sumsq_blocks(long n) {
    const long per = (long)kThreads * 4 * kLoads;           // floats one workgroup reads per turn of the unrolled loop
    const long nb = (n + per - 1) / per;
    return (int)(nb < 1 ? 1 : (nb > kMaxBlocks ? kMaxBlocks : nb));
}

}  // namespace

extern "C" {

int cc_grad_sumsq(const float* g, long n, double* partials, int* nblocks_out, void* stream) {
    if (n <= 0 || !g || !partials || ((uintptr_t)g & 15) != 0) return CC_ERR_ARG;
    const int nb = sumsq_blocks(n);
    if (nblocks_out) *nblocks_out = nb;
    hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, g, n, partials);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_grad_guard_finish(const double* partials, int nblocks, const float* hyper_row, float grad_scale, float* guard_row,
                         void* stream) {
    if (!partials || nblocks <= 0 || nblocks > kMaxBlocks || !hyper_row || !guard_row) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_guard_finish, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, partials, nblocks, hyper_row, grad_scale,
                       guard_row);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_adam_step_segment_guard(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const float* step_dev, long n,
                               const float* hyper_row, const float* guard_row, float grad_scale, void* stream) {
    if (n <= 0 || !hyper_row || !guard_row || !step_dev) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_adam_guard, dim3((unsigned)((n + 1023) / 1024)), dim3(kThreads), 0, (hipStream_t)stream, params, grads,
                       exp_avg, exp_avg_sq, n, hyper_row, guard_row, step_dev, grad_scale);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
