// Step ledger: one row of 32 floats per training step, appended on the device as the step's last launch, so that the per-step losses
// (train.py:563,574-576 reads them back with .item() every iteration), the NaN flags, the learning rates the Adam launches read and
// the gradient guard's rows survive the next replay of the captured step without a host sync between two replays.
//   k_ledger_append  one workgroup of 64 work-items: work-item s < 32 gathers slot s of the row from where the value already lives
//                    and stores it into row head % capacity of the ring; work-item 0 then folds the loss columns into the fp64
//                    aggregates {sum of n * value, sum of n, min, max} (AverageMeter.update(value, n)) and stores head + 1.
//                    No atomics: the read-modify-write is done by one work-item of one workgroup on one stream.
//   k_ledger_reset   the aggregates of a new epoch (the reference makes a new AverageMeter per epoch), ordered on the stream.
// The sources change address with every capture: they travel in the kernel's arguments, by value (the *_jobs idiom, jobs.h).
#include "cc_common.h"
#include "../../include/ccengine.h"

namespace {

constexpr int kThreads = 64;
constexpr int kSlots = CC_LEDGER_SLOTS;
constexpr int kAgg = CC_LEDGER_AGG_ROWS;            // slots 1 .. 7: loss, loss_1 .. loss_5, the NaN indicator
constexpr int kFlags0 = CC_LEDGER_SRC_FLAGS;
constexpr int kMaxSrc = CC_LEDGER_MAX_SOURCES;

struct LedgerSrc {
    long addr[kMaxSrc];     // [0] step, [1..6] losses, [7] hyper table, [8] guard table, [9 .. n) NaN flags; 0 = absent
    int n;
};

__device__ __forceinline__ const float* src(const LedgerSrc& s, int k) { return reinterpret_cast<const float*>(s.addr[k]); }

__global__ __launch_bounds__(kThreads) void k_ledger_append(LedgerSrc s, int hyper_rows, int n, float* __restrict__ ring,
                                                            int capacity, long* __restrict__ head, double* __restrict__ agg) {
    __shared__ float row[kSlots];
    const int t = threadIdx.x;
    const long h = head[0];                                   // (every work-item reads it before work-item 0 stores h + 1)
    const float qnan = __int_as_float(0x7fc00000);
    if (t < kSlots) {
        float v = 0.f;
        if (t <= 6) {
            if (src(s, t)) v = src(s, t)[0];
        } else if (t == 7) {
            for (int k = kFlags0; k < s.n; k++)
                if (src(s, k) && !(src(s, k)[0] == 0.f)) v = 1.f;
        } else if (t < 12) {
            if (src(s, 7) && t - 8 < hyper_rows) v = src(s, 7)[8 * (t - 8)];
        } else if (t < 24) {
            const int col = (t - 12) >> 2, r = (t - 12) & 3;                  // 0 norm, 1 coef, 2 finite
            if (!src(s, 8)) v = qnan;
            else if (r < hyper_rows) v = src(s, 8)[8 * r + col];
        }
        row[t] = v;
        ring[(h & (long)(capacity - 1)) * kSlots + t] = v;
    }
    __syncthreads();
    if (t != 0) return;
    const double w = (double)n;
    for (int k = 0; k < kAgg; k++) {
        const double v = (double)row[1 + k];
        double* a = agg + 4 * k;
        a[0] = a[0] + w * v;
        a[1] = a[1] + w;
        if (v < a[2]) a[2] = v;
        if (v > a[3]) a[3] = v;
    }
    head[0] = h + 1;
}

__global__ __launch_bounds__(kThreads) void k_ledger_reset(double* __restrict__ agg) {
    const int t = threadIdx.x;
    if (t >= kAgg) return;
    const float inf = __int_as_float(0x7f800000);
    agg[4 * t + 0] = 0.0;
    agg[4 * t + 1] = 0.0;
    agg[4 * t + 2] = (double)inf;
    agg[4 * t + 3] = -(double)inf;
}

}  // namespace

extern "C" {

int cc_ledger_append(const long* sources_host, int nsources, int hyper_rows, int n, float* ring, int capacity, long* head,
                     double* agg, void* stream) {
    if (!sources_host || nsources < kFlags0 || nsources > kMaxSrc || hyper_rows < 0 || hyper_rows > 4 || n <= 0 || !ring || !head ||
        !agg || capacity <= 0 || (capacity & (capacity - 1)) != 0)
        return CC_ERR_ARG;
    LedgerSrc s;
    for (int k = 0; k < kMaxSrc; k++) s.addr[k] = k < nsources ? sources_host[k] : 0;
    s.n = nsources;
    hipLaunchKernelGGL(k_ledger_append, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, s, hyper_rows, n, ring, capacity, head, agg);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_ledger_reset_agg(double* agg, void* stream) {
    if (!agg) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_ledger_reset, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, agg);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
