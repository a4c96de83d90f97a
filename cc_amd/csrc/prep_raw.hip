// Data preparation, device side (cc_amd/datasets/prepare.py): the resize of data/prepare_train_data.py's loaders --
// scipy.misc.imresize(img, (h, w)) of a uint8 frame (kitti_raw_loader.py:114, cityscapes_loader.py:118) = Pillow's 8-bit bilinear
// resampler (Resample.c) WITHOUT the byte-scale that float frames get, and the result stays uint8: it is what goes to the JPEG
// encoder and into the resident stores.  The arithmetic is prep.hip's (k_frames_resize_h / _v): horizontal pass -> uint8 ->
// vertical pass, 22-bit fixed-point coefficients built on the host (resample_table), accumulate from 1 << 21, shift, clip -- with
// one table and one tap count per axis, and only the first h_keep output rows written (Cityscapes drops the bottom quarter).
// Read once / write once; the pipeline around it is bound by the host's PNG decode, so: the plain two-pass form, one thread per
// output pixel.  Frame offsets are 64-bit.  Tap positions are clamped into the frame: padding taps carry weight 0, and a bad
// table cannot read outside the frame.
#include "cc_common.h"
#include "../../include/ccengine.h"

namespace {

constexpr int PREC = 22;         // Pillow PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// tmp[n, y, xo, :] = sum_i htab.weights[xo][i] * src[n, y, first[xo] + i, :]
__global__ __launch_bounds__(256) void k_raw_resize_h(const unsigned char* __restrict__ src, unsigned char* __restrict__ tmp,
                                                      const int* __restrict__ htab, int KH, int H, int W, int w) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * w) return;
    const int y = p / w, xo = p - y * w;
    const int* kk = htab + w + (size_t)xo * KH;
    const int x0 = htab[xo];
    const unsigned char* row = src + ((size_t)n * H + y) * W * 3;
    int acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
    for (int i = 0; i < KH; i++) {
        const int k = kk[i];
        const unsigned char* px = row + (size_t)clampi(x0 + i, W - 1) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] += k * (int)px[c];
    }
    unsigned char* d = tmp + ((size_t)n * H * w + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) d[c] = (unsigned char)clip8(acc[c] >> PREC);
}

// dst[n, y, x, :] = sum_i vtab.weights[y][i] * tmp[n, first[y] + i, x, :],  y < h_keep
__global__ __launch_bounds__(256) void k_raw_resize_v(const unsigned char* __restrict__ tmp, unsigned char* __restrict__ dst,
                                                      const int* __restrict__ vtab, int KV, int H, int h, int w, int h_keep) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= h_keep * w) return;
    const int y = p / w, x = p - y * w;
    const int* kk = vtab + h + (size_t)y * KV;
    const int y0 = vtab[y];
    const unsigned char* col = tmp + ((size_t)n * H * w + x) * 3;
    int acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
    for (int i = 0; i < KV; i++) {
        const int k = kk[i];
        const unsigned char* px = col + (size_t)clampi(y0 + i, H - 1) * w * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] += k * (int)px[c];
    }
    unsigned char* d = dst + ((size_t)n * h_keep * w + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) d[c] = (unsigned char)clip8(acc[c] >> PREC);
}

}  // namespace

extern "C" {

size_t cc_frames_resize_u8_ws(int N, int H, int w) {
    if (N <= 0 || H <= 0 || w <= 0) return 0;
    return (size_t)N * H * w * 3;
}

int cc_frames_resize_u8(const void* src, void* dst, const int* htab, int KH, const int* vtab, int KV, void* ws, int N, int H, int W,
                        int h, int w, int h_keep, void* stream) {
    if (!src || !dst || !htab || !vtab || !ws || N <= 0 || N > 65535 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || KH <= 0 || KV <= 0 ||
        h_keep <= 0 || h_keep > h || (long)H * w >= (1L << 31) - 256 || (long)h_keep * w >= (1L << 31) - 256)
        return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    unsigned char* tmp = (unsigned char*)ws;
    hipLaunchKernelGGL(k_raw_resize_h, dim3((unsigned)(((long)H * w + 255) / 256), (unsigned)N), dim3(256), 0, s,
                       (const unsigned char*)src, tmp, htab, KH, H, W, w);
    hipLaunchKernelGGL(k_raw_resize_v, dim3((unsigned)(((long)h_keep * w + 255) / 256), (unsigned)N), dim3(256), 0, s,
                       (const unsigned char*)tmp, (unsigned char*)dst, vtab, KV, H, h, w, h_keep);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
