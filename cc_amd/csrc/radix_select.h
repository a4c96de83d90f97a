// Exact k-th element of positive fp32 keys (their bits order as integers) by a 4-pass, 8-bit radix select: the medians of
// cc_depth_errors (metrics.hip) and cc_eigen_errors (kitti_eval.hip).  Per pass a histogram kernel counts, over the keys that match
// the digits chosen so far, the next digit (LDS histogram, flushed to global with integer atomics); a select kernel picks the bin that
// holds the remaining rank, extends the prefix and clears the histogram.  The kernels own their validity predicates and NaN counts;
// the pieces below are what they share.  State of one selection: 4 u32 {prefix, rank, count, aux}, zero before pass 0.
#pragma once
#include "cc_common.h"

namespace ccradix {

constexpr int kBins = 256;          // radix-select digit: 8 bits, 4 passes over the fp32 key

// zero the workgroup's LDS histogram(s) h[0..n)
template <int THREADS>
__device__ __forceinline__ void clear(unsigned* h, int n) {
    for (int j = threadIdx.x; j < n; j += THREADS) h[j] = 0u;
    __syncthreads();
}

// pass `pass` (digit = bits [24-8*pass, 32-8*pass)): count `key` in the LDS histogram h if its higher digits are those of `pre`
__device__ __forceinline__ void count_key(unsigned* h, unsigned key, unsigned pre, int pass) {
    const int shift = 24 - 8 * pass;
    if (pass == 0 || (key >> (shift + 8)) == (pre >> (shift + 8))) atomicAdd(&h[(key >> shift) & (kBins - 1)], 1u);
}

// add the workgroup's LDS histogram(s) h[0..n) to the global ones
template <int THREADS>
__device__ __forceinline__ void flush(const unsigned* h, unsigned* gh, int n) {
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += THREADS)
        if (h[j]) atomicAdd(&gh[j], h[j]);
}

// one work-item per selection: in pass 0 the count and the rank of the middle element (upper: c / 2, else the lower (c - 1) / 2,
// torch.median's), then pick the bin that holds the remaining rank, extend the prefix, clear the histogram
__device__ __forceinline__ void select(unsigned* h, unsigned* st, int pass, bool upper) {
    if (pass == 0) {
        unsigned c = 0;
        for (int j = 0; j < kBins; j++) c += h[j];
        st[2] = c;
        st[1] = c > 0 ? (upper ? c / 2 : (c - 1) / 2) : 0;
    }
    const int shift = 24 - 8 * pass;
    unsigned cum = 0;
    const unsigned rank = st[1];
    for (int j = 0; j < kBins; j++) {
        const unsigned c = h[j];
        if (c > 0 && rank < cum + c) {
            st[0] |= (unsigned)j << shift;
            st[1] = rank - cum;
            break;
        }
        cum += c;
    }
    for (int j = 0; j < kBins; j++) h[j] = 0u;
}

// the selected value after pass 3; NaN for an empty selection or one whose aux (a count of NaN keys) is not zero
__device__ __forceinline__ float median_of(const unsigned* st) {
    return (st[2] == 0 || st[3] != 0) ? __int_as_float(0x7fc00000) : __uint_as_float(st[0]);
}

}  // namespace ccradix
