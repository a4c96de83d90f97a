// Fused Adam over the flat fp32 parameter bucket (torch.optim.Adam of train.py:307-310,568: lr, betas, eps, weight_decay in its L2
// form, no amsgrad) instead of ~460 per-tensor update chains.  HBM-bound: 4 reads + 3 writes of 4 B per parameter (28 B), float4
// accesses.  The step counter lives on the device so the launches can sit inside a hipGraph -- and so do the hyperparameters of the
// table-driven entries the trainer uses (k_adam_hyper: cc_adam_step_hyper for the whole bucket, cc_adam_step_segment_hyper for one
// network's segment): one row {lr, beta1, beta2, eps, weight_decay, 0, 0, 0} per network, written by the host between two replays,
// so that a captured step follows an lr schedule without being captured again.  k_adam (cc_adam_step, cc_adam_step_segment) is the
// same update with the values as launch arguments and no weight decay.
#include "cc_common.h"
#include "../../include/ccengine.h"

namespace {

__global__ void k_adam_tick(float* step) { step[0] += 1.0f; }

__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                              const float* __restrict__ step, float grad_scale) {
    const float t = step[0];
    const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
    const float step_size = lr / bc1, rs2 = 1.f / sqrtf(bc2);
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 + 3 < n) {
        float4 pp = *reinterpret_cast<float4*>(p + i4);
        const float4 gg = *reinterpret_cast<const float4*>(g + i4);
        float4 mm = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
        float* P = &pp.x; const float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float gr = G[k] * grad_scale;
            M[k] = b1 * M[k] + (1.f - b1) * gr;
            V[k] = b2 * V[k] + (1.f - b2) * gr * gr;
            P[k] -= step_size * (M[k] / (sqrtf(V[k]) * rs2 + eps));
        }
        *reinterpret_cast<float4*>(p + i4) = pp;
        *reinterpret_cast<float4*>(m + i4) = mm;
        *reinterpret_cast<float4*>(v + i4) = vv;
    } else {
        for (long i = i4; i < n; i++) {
            const float gr = g[i] * grad_scale;
            m[i] = b1 * m[i] + (1.f - b1) * gr;
            v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
            p[i] -= step_size * (m[i] / (sqrtf(v[i]) * rs2 + eps));
        }
    }
}

// k_adam with lr / betas / eps / weight decay read from device memory.  hyper: rows x 8 floats; bounds: rows + 1 element offsets, row r
// owns [bounds[r], bounds[r + 1]) -- every interior bound a multiple of 4, so a float4 (and the scalar tail, which lies behind the last
// interior bound) has ONE row; bounds == nullptr: the range has one row, hyper points at it.  The row index is built from compares
// against the interior bounds only, so it stays inside the table whatever the bounds hold.  The loads of the row are uniform over a
// wave except where a bound cuts it.  Same operations in the same order as k_adam (-ffp-contract=off): with weight_decay == 0 and
// the same values the results are the same bits.  weight_decay: torch.optim.Adam's L2 form, g += wd * p with p before the update.
__global__ __launch_bounds__(256) void k_adam_hyper(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, const float* __restrict__ hyper,
                                                    const long* __restrict__ bounds, int rows, const float* __restrict__ step,
                                                    float grad_scale) {
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    // (the element loads are issued first: they do not depend on the table, whose look-up is a chain of two dependent loads)
    const bool full = i4 + 3 < n;
    float4 pp, gg, mm, vv;
    if (full) {
        pp = *reinterpret_cast<float4*>(p + i4);
        gg = *reinterpret_cast<const float4*>(g + i4);
        mm = *reinterpret_cast<float4*>(m + i4);
        vv = *reinterpret_cast<float4*>(v + i4);
    }
    int r = 0;
    if (bounds != nullptr)
        for (int k = 1; k < rows; k++) r += (i4 >= bounds[k]) ? 1 : 0;
    const float* h = hyper + 8 * r;
    const float lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
    const float t = step[0];
    const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
    const float step_size = lr / bc1, rs2 = 1.f / sqrtf(bc2);
    if (full) {
        float* P = &pp.x; const float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float gr = G[k] * grad_scale;
            if (wd != 0.f) gr = gr + wd * P[k];
            M[k] = b1 * M[k] + (1.f - b1) * gr;
            V[k] = b2 * V[k] + (1.f - b2) * gr * gr;
            P[k] -= step_size * (M[k] / (sqrtf(V[k]) * rs2 + eps));
        }
        *reinterpret_cast<float4*>(p + i4) = pp;
        *reinterpret_cast<float4*>(m + i4) = mm;
        *reinterpret_cast<float4*>(v + i4) = vv;
    } else {
        for (long i = i4; i < n; i++) {
            float gr = g[i] * grad_scale;
            if (wd != 0.f) gr = gr + wd * p[i];
            m[i] = b1 * m[i] + (1.f - b1) * gr;
            v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
            p[i] -= step_size * (m[i] / (sqrtf(v[i]) * rs2 + eps));
        }
    }
}

__global__ __launch_bounds__(256) void k_fill(float* __restrict__ p, long n, float value) {
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 + 3 < n) *reinterpret_cast<float4*>(p + i4) = make_float4(value, value, value, value);
    else for (long i = i4; i < n; i++) p[i] = value;
}

}  // namespace

extern "C" {

int cc_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, long n, float lr,
                 float beta1, float beta2, float eps, float grad_scale, void* stream) {
    if (n <= 0) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, s, step_dev);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, n,
                       lr, beta1, beta2, eps, (const float*)step_dev, grad_scale);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

/* The same update on a sub-range of the bucket (the caller passes the range's base pointers); tick = 0 leaves the step counter as
 * it is: the second and later segments of one optimizer step.  Lets the update of a segment whose gradients have arrived run
 * while the all-reduce of the next segment is still in flight. */
int cc_adam_step_segment(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, long n, float lr,
                         float beta1, float beta2, float eps, float grad_scale, int tick, void* stream) {
    if (n <= 0) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (tick) hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, s, step_dev);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, n,
                       lr, beta1, beta2, eps, (const float*)step_dev, grad_scale);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

/* The whole bucket, every element with the hyperparameters of the row that owns it (one launch for all networks). */
int cc_adam_step_hyper(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, long n,
                       const float* hyper, const long* bounds, int rows, float grad_scale, void* stream) {
    if (n <= 0 || rows <= 0 || !hyper || !bounds) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, s, step_dev);
    hipLaunchKernelGGL(k_adam_hyper, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, n,
                       hyper, bounds, rows, (const float*)step_dev, grad_scale);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

/* A sub-range that lies inside one row (base pointers of the range, pointer to its row); tick as in cc_adam_step_segment. */
int cc_adam_step_segment_hyper(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, long n,
                               const float* hyper_row, float grad_scale, int tick, void* stream) {
    if (n <= 0 || !hyper_row) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (tick) hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, s, step_dev);
    hipLaunchKernelGGL(k_adam_hyper, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, n,
                       hyper_row, (const long*)nullptr, 1, (const float*)step_dev, grad_scale);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_adam_tick(float* step_dev, void* stream) {
    if (!step_dev) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_fill(float* p, long n, float value, void* stream) {
    if (n <= 0) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, p, n, value);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
