// Fused Adam over the flat fp32 parameter bucket (torch.optim.Adam of train.py:307-310,568: lr, betas, eps, weight_decay in its L2
// form, no amsgrad) instead of ~460 per-tensor update chains.  HBM-bound: 4 reads + 3 writes of 4 B per parameter (28 B), float4
// accesses.  The step counter lives on the device so the launches can sit inside a hipGraph -- and so do the hyperparameters of the
// table-driven entries the trainer uses (k_adam_hyper: cc_adam_step_hyper for the whole bucket, cc_adam_step_segment_hyper for one
// network's segment): one row {lr, beta1, beta2, eps, weight_decay, 0, 0, 0} per network, written by the host between two replays,
// so that a captured step follows an lr schedule without being captured again.  k_adam (cc_adam_step, cc_adam_step_segment) is the
// same update with the values as launch arguments and no weight decay.  The update itself -- one element, and the float4 body /
// scalar tail around it -- is written once, in adam_update.h, for these two kernels and k_adam_guard (grad_guard.hip).
#include "adam_update.h"
#include "../../include/ccengine.h"

namespace {

__global__ void k_adam_tick(float* step) { step[0] += 1.0f; }

__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                              const float* __restrict__ step, float grad_scale) {
    const ccadam::Coefs c = ccadam::coefs(lr, b1, b2, eps, 0.f, step[0], grad_scale, 1.f);
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    const bool full = i4 + 3 < n;
    ccadam::Quad q;
    if (full) ccadam::load4(q, p, g, m, v, i4);
    ccadam::update4<false, false>(p, g, m, v, i4, n, full, q, c);
}

// k_adam with lr / betas / eps / weight decay read from device memory.  hyper: rows x 8 floats; bounds: rows + 1 element offsets, row r
// owns [bounds[r], bounds[r + 1]) -- every interior bound a multiple of 4, so a float4 (and the scalar tail, which lies behind the last
// interior bound) has ONE row; bounds == nullptr: the range has one row, hyper points at it.  The row index is built from compares
// against the interior bounds only, so it stays inside the table whatever the bounds hold.  The loads of the row are uniform over a
// wave except where a bound cuts it.  k_adam's update (adam_update.h): with weight_decay == 0 and the same values the results are
// the same bits.  weight_decay: torch.optim.Adam's L2 form, g += wd * p with p before the update.
__global__ __launch_bounds__(256) void k_adam_hyper(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, const float* __restrict__ hyper,
                                                    const long* __restrict__ bounds, int rows, const float* __restrict__ step,
                                                    float grad_scale) {
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    // (the element loads are issued first: they do not depend on the table, whose look-up is a chain of two dependent loads)
    const bool full = i4 + 3 < n;
    ccadam::Quad q;
    if (full) ccadam::load4(q, p, g, m, v, i4);
    int r = 0;
    if (bounds != nullptr)
        for (int k = 1; k < rows; k++) r += (i4 >= bounds[k]) ? 1 : 0;
    const float* h = hyper + 8 * r;
    const ccadam::Coefs c = ccadam::coefs(h[0], h[1], h[2], h[3], h[4], step[0], grad_scale, 1.f);
    ccadam::update4<true, false>(p, g, m, v, i4, n, full, q, c);
}

__global__ __launch_bounds__(256) void k_fill(float* __restrict__ p, long n, float value) {
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 + 3 < n) *reinterpret_cast<float4*>(p + i4) = make_float4(value, value, value, value);
    else for (long i = i4; i < n; i++) p[i] = value;
}

// the launch of k_adam / k_adam_hyper behind their two entries each; tick: count the step first
int launch_adam(float* p, const float* g, float* m, float* v, float* step_dev, long n, float lr, float b1, float b2, float eps,
                float grad_scale, int tick, void* stream) {
    if (n <= 0) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (tick) hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, s, step_dev);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, p, g, m, v, n, lr, b1, b2, eps,
                       (const float*)step_dev, grad_scale);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int launch_adam_hyper(float* p, const float* g, float* m, float* v, float* step_dev, long n, const float* hyper, const long* bounds,
                      int rows, float grad_scale, int tick, void* stream) {
    if (n <= 0 || !hyper) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (tick) hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, s, step_dev);
    hipLaunchKernelGGL(k_adam_hyper, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, p, g, m, v, n, hyper, bounds, rows,
                       (const float*)step_dev, grad_scale);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // namespace

extern "C" {

int cc_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, long n, float lr,
                 float beta1, float beta2, float eps, float grad_scale, void* stream) {
    return launch_adam(params, grads, exp_avg, exp_avg_sq, step_dev, n, lr, beta1, beta2, eps, grad_scale, 1, stream);
}

/* The same update on a sub-range of the bucket (the caller passes the range's base pointers); tick = 0 leaves the step counter as
 * it is: the second and later segments of one optimizer step.  Lets the update of a segment whose gradients have arrived run
 * while the all-reduce of the next segment is still in flight. */
int cc_adam_step_segment(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, long n, float lr,
                         float beta1, float beta2, float eps, float grad_scale, int tick, void* stream) {
    return launch_adam(params, grads, exp_avg, exp_avg_sq, step_dev, n, lr, beta1, beta2, eps, grad_scale, tick, stream);
}

/* The whole bucket, every element with the hyperparameters of the row that owns it (one launch for all networks). */
int cc_adam_step_hyper(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, long n,
                       const float* hyper, const long* bounds, int rows, float grad_scale, void* stream) {
    if (rows <= 0 || !bounds) return CC_ERR_ARG;
    return launch_adam_hyper(params, grads, exp_avg, exp_avg_sq, step_dev, n, hyper, bounds, rows, grad_scale, 1, stream);
}

/* A sub-range that lies inside one row (base pointers of the range, pointer to its row); tick as in cc_adam_step_segment. */
int cc_adam_step_segment_hyper(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_dev, long n,
                               const float* hyper_row, float grad_scale, int tick, void* stream) {
    return launch_adam_hyper(params, grads, exp_avg, exp_avg_sq, step_dev, n, hyper_row, nullptr, 1, grad_scale, tick, stream);
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
