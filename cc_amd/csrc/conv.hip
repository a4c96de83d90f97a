// fp32 convolutions of the four CC networks on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32:
// exact fp32, bit-equal to an fmaf chain, 157 TFLOP/s peak).  Replaces cuDNN/MIOpen's conv2d,
// conv_transpose2d and convolution_backward (219 forward + 297 backward calls per step).
//
// Every problem here is ONE implicit GEMM, described by a GG: conv forward, conv data-gradient, transposed-conv forward and
// transposed-conv data-gradient are
//      Y[n, m, P(t)] = epilogue( sum_{c, i, j}  A[m, (c,i,j)] * X[n, c, si*ty + dy(i), si*tx + dx(j)] )
//   * output pixels t = (ty, tx) live on a lattice  P(t) = (oy0 + so*ty, ox0 + so*tx)   (so = 2 selects one
//     parity class of a stride-2 transposed conv / stride-2 data-gradient, so no MFMA work is spent on
//     structurally-zero taps);
//   * the taps form a regular Rt x St grid: dy(i) = dy0 + i*dstep, dx(j) = dx0 + j*dstep, and the weight of
//     (m, c, i, j) sits at  w[w0 + m*w_sm + c*w_sc + i*w_ri + j*w_sj]  -- strides express [K,C,R,S] weights,
//     their transpose/flip for data-gradients, and ConvTranspose2d's [Cin,Cout,R,S] layout without repacking.
// GEMM view: M = output channels, N = B*OHt*OWt lattice pixels (contiguous in NCHW -> coalesced stores, and
// MFMA D columns map to lanes = pixels), K = Cin*Rt*St gathered on the fly (im2col never materialised).
// The epilogue fuses bias, residual add, ReLU / LeakyReLU(0.2) / a*sigmoid+b and the activation backward (conv_tail.h).
//
// Map of this file, in its order:
//   kernels   k_gather_gemm        the FALLBACK (index math per element, no workspace): a patch beyond the LDS, a call without
//                                  workspace, a misaligned Winograd input
//             k_repack_w / _table  weight images [tap][c][m], per call / all of a network's in one launch
//             k_conv_patch*        the MAIN path, patch-staged; _stk = stacked tiny maps, _multi = up to MAXCLS problems per launch
//             k_splitk_epilogue*   deterministic second stage of split-K (also of wino.hip's launches); k_pad_rows is next to its launch
//   planning  plan_conv            one ConvPlan per problem, in named steps (plan_wino_padded ... plan_balance)
//   launch    launch_gg            one problem: head kernels (conv_heads.hip), Winograd (wino.hip), patch kernel, fallback
//             classes_form, launch_classes   several problems in one launch: the form decided (nothing launched), then run
//             kernel_name          the one place that formats a kernel's name: timing scopes and name queries
//   C ABI     forward; TProblem / for_each_class (the transposed arithmetic and its parity classes), data-gradient; lists; name queries
//
// Weight gradients: conv_wgrad.hip (and the kernels it dispatches to); activation backward / bias gradients: conv_act.hip;
// the timing registry behind cctiming::Scope: timing.hip.
#include <stdio.h>
#include <stdlib.h>
#include <stddef.h>
#include <string.h>
#include "cc_common.h"
#include "conv_internal.h"
#include "cc_tools.h"
#include "conv_tail.h"
#include "wino_weights.h"
#include "../../include/ccengine.h"
#include <vector>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// BM = 16 (layers with <= 16 output channels: the full-resolution ends of the nets, prediction heads, their data-gradients):
// v_mfma_f32_16x16x4_f32 tiles, so that no MFMA row is spent on channels that do not exist (a 32-row tile wastes half)
inline int pick_bm_fwd(int M) {
    static const int no16 = cctools::env_flag("CC_CONV_NO_BM16");
    return M > 64 ? 128 : (M > 32 ? 64 : ((M > 16 || no16) ? 32 : 16));
}

using ccint::BK;
using ccint::BN;
using ccint::MAXGRP;
using ccint::pick_bm;

using namespace cctail;

struct GG {
    const float* x; const float* w; const float* bias; const float* res; float* y;
    int B, Cin, IH, IW; long x_bs;
    int M; long w_sm, w_sc; int w0, w_ri, w_sj;
    int Rt, St, dy0, dx0, dstep, si;
    int OHt, OWt, so, oy0, ox0, OH, OW; long y_bs, res_bs;
    int act; float act_a, act_b;
    int res_mul;
    const float* add; long add_bs;      // res_mul mode only: tensor of y's shape added before act'(res) is applied (may alias y)
};

template <int BM>
__global__ __launch_bounds__(256) void k_gather_gemm(GG g) {
    constexpr int WM = (BM >= 64) ? BM / 2 : 32;     // wave tile rows
    constexpr int WN = (BM >= 64) ? 64 : 32;         // wave tile cols
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int AP = BM + 4;                        // padded A row (k-major: As[k][m])
    constexpr int AQ = BM / 16;                       // A elements per thread per chunk
    __shared__ float As[2][BK * AP];
    __shared__ float Bs[2][BK * BN];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = (BM >= 64) ? (wid >> 1) : 0;
    const int wn = (BM >= 64) ? (wid & 1) : wid;
    const int m0 = blockIdx.y * BM;
    const long p0 = (long)blockIdx.x * BN;
    const int HWt = g.OHt * g.OWt;
    const long Ntot = (long)g.B * HWt;
    const int RS = g.Rt * g.St;
    const int Ktot = g.Cin * RS;
    const int x_cs = g.IH * g.IW;

    // ---- loader roles
    // B: pixel column jb, k rows kr0 + 2q
    const int jb = tid & (BN - 1);
    const int kr0 = __builtin_amdgcn_readfirstlane(tid >> 7);
    const long pb = p0 + jb;
    const bool pvalid = pb < Ntot;
    int iy0 = 0, ix0 = 0;
    long xbase = 0;
    if (pvalid) {
        const int n = (int)(pb / HWt);
        const int t = (int)(pb - (long)n * HWt);
        const int ty = t / g.OWt, tx = t - ty * g.OWt;
        iy0 = g.si * ty;
        ix0 = g.si * tx;
        xbase = (long)n * g.x_bs;
    }
    float ra[AQ], rb[8];

    auto load_chunk = [&](int kbase) {
        // A tile: element e = tid + 256q -> (m = e>>4, kk = e&15 = tid&15): one (c,i,j) decode per chunk
        {
            const int k = kbase + (tid & 15);
            const bool kv = k < Ktot;
            const int c = k / RS, rem = k - c * RS;
            const int i = rem / g.St, j = rem - i * g.St;
            const long woff = (long)g.w0 + (long)c * g.w_sc + i * g.w_ri + j * g.w_sj;
#pragma unroll
            for (int q = 0; q < AQ; q++) {
                const int m = m0 + (tid >> 4) + 16 * q;
                ra[q] = (kv && m < g.M) ? g.w[woff + (long)m * g.w_sm] : 0.f;
            }
        }
        // B tile: k wave-uniform
        int k = kbase + kr0;
        int c = k / RS, rem = k - c * RS;
        int i = rem / g.St, j = rem - i * g.St;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            float v = 0.f;
            if (pvalid && k < Ktot) {
                const int iy = iy0 + g.dy0 + i * g.dstep, ix = ix0 + g.dx0 + j * g.dstep;
                if ((unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW)
                    v = g.x[xbase + (long)c * x_cs + iy * g.IW + ix];
            }
            rb[q] = v;
            k += 2;
            j += 2;
            while (j >= g.St) { j -= g.St; i++; }
            while (i >= g.Rt) { i -= g.Rt; c++; }
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int q = 0; q < AQ; q++) {
            const int e = tid + 256 * q;
            As[buf][(e & 15) * AP + (e >> 4)] = ra[q];
        }
#pragma unroll
        for (int q = 0; q < 8; q++) Bs[buf][(kr0 + 2 * q) * BN + jb] = rb[q];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; a++)
#pragma unroll
        for (int b = 0; b < TN; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

    const int nchunks = (Ktot + BK - 1) / BK;
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    const int l31 = lane & 31, lk = lane >> 5;
    for (int ch = 0; ch < nchunks; ch++) {
        const int buf = ch & 1;
        if (ch + 1 < nchunks) load_chunk((ch + 1) * BK);
#pragma unroll
        for (int ks = 0; ks < BK / 2; ks++) {
            float af[TM], bf[TN];
#pragma unroll
            for (int a = 0; a < TM; a++) af[a] = As[buf][(2 * ks + lk) * AP + wm * WM + a * 32 + l31];
#pragma unroll
            for (int b = 0; b < TN; b++) bf[b] = Bs[buf][(2 * ks + lk) * BN + wn * WN + b * 32 + l31];
#pragma unroll
            for (int a = 0; a < TM; a++)
#pragma unroll
                for (int b = 0; b < TN; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a], bf[b], acc[a][b], 0, 0, 0);
        }
        if (ch + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: D col = lane&31 -> pixel, row = (r&3) + 8*(r>>2) + 4*(lane>>5) -> channel
    const int y_cs = g.OH * g.OW;
#pragma unroll
    for (int b = 0; b < TN; b++) {
        const long p = p0 + wn * WN + b * 32 + l31;
        if (p >= Ntot) continue;
        const int n = (int)(p / HWt);
        const int t = (int)(p - (long)n * HWt);
        const int ty = t / g.OWt, tx = t - ty * g.OWt;
        const long pix = (long)(g.oy0 + g.so * ty) * g.OW + (g.ox0 + g.so * tx);
        float* yb = g.y + (long)n * g.y_bs + pix;
        const float* rbp = g.res ? g.res + (long)n * g.res_bs + pix : nullptr;
        const float* abp = g.add ? g.add + (long)n * g.add_bs + pix : nullptr;
#pragma unroll
        for (int a = 0; a < TM; a++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + wm * WM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m < g.M) {
                    float v = acc[a][b][r];
                    if (g.bias) v += g.bias[m];
                    yb[(long)m * y_cs] = conv_tail(v, rbp != nullptr, rbp ? rbp[(long)m * y_cs] : 0.f, g.res_mul, g.act, g.act_a, g.act_b,
                                                   abp ? abp[(long)m * y_cs] : 0.f);
                }
            }
        }
    }
}

// ------------------------------------------------------------------ patch-staged implicit GEMM (main path)
// Same GEMM as k_gather_gemm, restructured so that neither operand needs per-element index math:
//   * the output tile is a 4 x 32 block of lattice pixels of ONE image; for a chunk of CK input channels the
//     input PATCH that all Rt x St taps of that tile touch is staged in LDS once (zero-filled outside the
//     image) and every tap's B fragment is a shifted ds_read of it -> global->LDS traffic / tap count;
//   * weights are repacked per call to wp[tap][c][m] (m contiguous, zero padded to CK / BM multiples), so an
//     A tile is CK contiguous rows;
//   * both are moved by LDS-DMA (global_load_lds: no staging VGPRs, no ds_write, fully asynchronous) and
//     double-buffered: A per (chunk, tap) stage, patch per chunk; one barrier per stage (= CK/2 MFMA k-steps
//     x TM x TN MFMAs per wave);
//   * deep layers on small maps get split-K over channel chunks (grid.z) with a deterministic second pass.
// Two tile shapes of 128 lattice pixels: 4 rows x 32 columns, or 8 x 16 (CP::tw16) -- whichever pads the map less
// (208 columns = 6.5 x 32 but 13 x 16; 104 = 3.25 x 32 but 6.5 x 16).  The 32 MFMA columns of a wave are one row of 32 pixels
// or two rows of 16: only the per-lane patch offset differs.
constexpr int TH = 4, TW = 32;

struct CP {
    const float* x; const float* wp; const float* zeros; const float* bias; const float* res; float* y; float* part;
    int B, Cin, IH, IW; long x_bs;
    int M, Mpad, Cpad;
    int Rt, St, si, dstep, dy_base, dx_base, ymin, xmin;
    int PH, PWr, PS;
    int tw16;              // tile = 8 rows x 16 columns instead of 4 x 32
    int ipt, phi;          // ipt > 1: maps of <= 4 lattice rows -- the 8 tile rows stack the rows of ipt consecutive images, each with
                           // its own phi patch rows (halo included) in the LDS patch
    int aligned, shift;    // aligned: patch rows start on a 16-byte boundary of x (PWr = padded row length) -> dwordx4 LDS-DMA
    int OHt, OWt, so, oy0, ox0, OH, OW; long y_bs, res_bs;
    int tiles_x, tiles_y;
    int nsplit, cps; long part_stride;
    int act; float act_a, act_b;
    int res_mul;
    const float* add; long add_bs;
    int vec4;              // fused epilogue may use 16-byte accesses: unit lattice stride, rows 16-byte aligned in y / res / add
    int wmajor;            // XCD order of the launch (conv_xcd_blocks): 0 = an XCD's run of work shares INPUT tiles, 1 = it shares WEIGHT
                           // blocks (layers whose weights are the larger operand: the 8x26 ... 2x7 maps of the 256-1024 channel layers)
};

// wp[(t*Cpad + c)*Mpad + m] = w[w0 + m*w_sm + c*w_sc + i*w_ri + j*w_sj]  (0 beyond Cin / M), t = i*St + j
__global__ __launch_bounds__(256) void k_repack_w(const float* __restrict__ w, float* __restrict__ wp, float* __restrict__ zeros,
                                                  int M, int Cin, int Mpad, int Cpad, int T, int St, long w_sm, long w_sc,
                                                  int w0, int w_ri, int w_sj) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 64) zeros[threadIdx.x] = 0.f;
    const long tot = (long)T * Cpad * Mpad;
    if (e >= tot) return;
    const int m = (int)(e % Mpad);
    const long r = e / Mpad;
    const int c = (int)(r % Cpad), t = (int)(r / Cpad);
    const int i = t / St, j = t - i * St;
    wp[e] = (m < M && c < Cin) ? w[(long)w0 + (long)m * w_sm + (long)c * w_sc + i * w_ri + j * w_sj] : 0.f;
}

// All weight repacks of a training step in ONE launch: desc[d] = 16 longs
//   {src, dst, M, Cin, Mpad, Cpad, T, St, w_sm, w_sc, w0, w_ri, w_sj, nfloats, first_block, nblocks}
// (the per-call k_repack_w launches were ~540 tiny kernels = 3 ms of launch latency per step).
// It is a transpose ([m][c][tap] or [c][m][tap] in memory -> [tap][c][m]) of ~600 MB per step, so it goes through an
// LDS tile: one workgroup = 64 m x CT c x all T taps, read in SOURCE memory order (tap fastest, then whichever of c / m
// has the smaller stride), written in destination order (m fastest): both sides coalesced.
__host__ __device__ inline int repack_ct(int T) { const int ct = 72 / T; return ct < 1 ? 1 : (ct > 64 ? 64 : ct); }
inline long repack_blocks(int Mpad, int Cpad, int T) {
    const int ct = repack_ct(T);
    return (long)((Mpad + 63) / 64) * ((Cpad + ct - 1) / ct);
}

// TC > 0: the tap count as a compile-time constant (the index arithmetic of the two loops is three integer divisions per
// element: with run-time divisors they -- not memory -- bound the kernel, 0.6 ms per step for 890 MB)
template <int TC>
__device__ __forceinline__ void repack_body(const long* __restrict__ d, float* tile, int bid) {
    const float* __restrict__ w = reinterpret_cast<const float*>(d[0]);
    float* __restrict__ wp = reinterpret_cast<float*>(d[1]);
    const int M = (int)d[2], Cin = (int)d[3], Mpad = (int)d[4], Cpad = (int)d[5], St = (int)d[7];
    const int T = TC > 0 ? TC : (int)d[6];
    const long w_sm = d[8], w_sc = d[9], w0 = d[10], w_ri = d[11], w_sj = d[12];
    const int CT = repack_ct(T);
    const int nmt = (Mpad + 63) / 64;
    const int m0 = (bid % nmt) * 64, c0 = (bid / nmt) * CT;
    const int CTT = CT * T, n = 64 * CTT;
    const bool m_slow = w_sm > w_sc;
    // eight loads in flight per work item (one load, wait, LDS store per iteration leaves the kernel at 1.6 TB/s: latency-bound)
    for (int e0 = threadIdx.x; e0 < n; e0 += 8 * 256) {
        float v[8];
        int li[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int e = e0 + u * 256;
            v[u] = 0.f;
            li[u] = -1;
            if (e < n) {
                int m_, c_, t;
                if (m_slow) { m_ = e / CTT; const int r = e - m_ * CTT; c_ = r / T; t = r - c_ * T; }
                else { c_ = e / (64 * T); const int r = e - c_ * 64 * T; m_ = r / T; t = r - m_ * T; }
                const int m = m0 + m_, c = c0 + c_;
                li[u] = (t * CT + c_) * 65 + m_;
                if (m < M && c < Cin) {
                    const int i = t / St, j = t - i * St;
                    v[u] = w[w0 + (long)m * w_sm + (long)c * w_sc + i * w_ri + j * w_sj];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (li[u] >= 0) tile[li[u]] = v[u];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256) {
        const int m_ = e & 63, r = e >> 6;
        const int t = r / CT, c_ = r - t * CT;
        if (m0 + m_ < Mpad && c0 + c_ < Cpad) wp[((long)t * Cpad + c0 + c_) * Mpad + m0 + m_] = tile[r * 65 + m_];
    }
}

__global__ __launch_bounds__(256) void k_repack_table(const long* __restrict__ desc, int ndesc) {
    __shared__ float tile[72 * 65 + 64 * 65];
    // binary search the descriptor whose block range contains blockIdx.x
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[16 * mid + 14] <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const long* d = desc + 16 * lo;
    const int bid = (int)((long)blockIdx.x - d[14]);
    if (bid >= (int)d[15]) return;
    if ((int)d[6] == ccwino::WINO_T) {         // Winograd layers: U = G g G^T in the staging layout of wino.hip (d[7] < 0: flipped taps)
        ccwino::wino_weight_body(reinterpret_cast<const float*>(d[0]), reinterpret_cast<float*>(d[1]), (int)d[2], (int)d[3], (int)d[5],
                                 d[8], d[9], d[10], d[11], d[12], d[7] < 0 ? 1 : 0, bid);
        return;
    }
    switch ((int)d[6]) {                       // tap counts of the CC networks (3x3, 7x7, 5x5, 4x4 and their parity classes)
        case 9: repack_body<9>(d, tile, bid); break;
        case 1: repack_body<1>(d, tile, bid); break;
        case 2: repack_body<2>(d, tile, bid); break;
        case 4: repack_body<4>(d, tile, bid); break;
        case 49: repack_body<49>(d, tile, bid); break;
        case 25: repack_body<25>(d, tile, bid); break;
        case 16: repack_body<16>(d, tile, bid); break;
        case 6: repack_body<6>(d, tile, bid); break;
        case 12: repack_body<12>(d, tile, bid); break;
        default: repack_body<0>(d, tile, bid); break;
    }
}

// TPS = taps per pipeline stage: one barrier (+ DMA wait) per TPS*CK/2*TM*TN MFMAs per wave.  With TPS = 1 a stage is only
// 32 MFMAs (2 k cycles) and the LDS-read latency + barrier skew at every stage boundary costs ~10-15 %; TPS = 3 (a whole
// tap row of a 3x3) amortises it 3x for 32 KB more LDS (still two workgroups per CU).
// SPLIT: 0 = whole reduction in this workgroup (fused epilogue), 1 = split-K partial slabs, 2 = decided per class at run time
#if defined(CC_ABLATE_DMA) || defined(CC_ABLATE_LDS) || defined(CC_ABLATE_BARRIER) || defined(CC_ABLATE_MFMA)
// ablation builds compute garbage: keep it finite and tiny so that the rest of the step runs at its normal speed
__device__ __forceinline__ float abl_fix(float v) { return (v == v && fabsf(v) < 1e30f) ? 1e-6f * fminf(fmaxf(v, -1.f), 1.f) : 0.f; }
#else
__device__ __forceinline__ float abl_fix(float v) { return v; }
#endif

// STK: the tile stacks the rows of CP::ipt images (maps of <= 4 lattice rows); a separate instantiation -- the row mapping costs
// scalar registers the common kernels do not have (they sit at the SGPR limit: +10 spills and -6 % measured with it compiled in)
template <int BM, int CK, int TPS, int SPLIT, int STK>
__device__ __forceinline__ void conv_patch_body(const CP& g, const int bx_in, const int by_in, const int bz_in) {
    constexpr int WM = (BM >= 64) ? BM / 2 : 32;
    constexpr int TM = WM / 32;
    constexpr int TN = (BM >= 64) ? 2 : 1;           // lattice rows of the tile per wave
    HIP_DYNAMIC_SHARED(float, smem)
    float* As = smem;                          // [2][TPS][CK][BM]
    float* Ps = smem + 2 * TPS * CK * BM;      // [2][CK][PS]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = (BM >= 64) ? (wid >> 1) : 0;
    const int row0 = (BM >= 64) ? 2 * (wid & 1) : wid;       // first lattice row (0..3) of this wave
    const int l31 = lane & 31, lk = lane >> 5;

    int bx = bx_in;
    const int tile_x = bx % g.tiles_x;
    bx /= g.tiles_x;
    const int tile_y = bx % g.tiles_y;
    const int ipt = STK ? g.ipt : 1;
    const int n = (bx / g.tiles_y) * ipt;                       // (first) image of the tile
    const int n_tile = n;
    const int rowstep = g.tw16 ? 2 : 1;                         // lattice rows per MFMA column group
    const int lr = g.tw16 ? (l31 >> 4) : 0, lc = g.tw16 ? (l31 & 15) : l31;     // this lane's row / column inside the group
    const int ty0 = tile_y * (g.tw16 ? 8 : TH), tx0 = tile_x * (g.tw16 ? 16 : TW);
    const int gy0 = g.si * ty0 + g.ymin, gx0 = g.si * tx0 + g.xmin;
    const int m0 = by_in * BM;
    const int T = g.Rt * g.St;
    const int nchunk = g.Cpad / CK;
    const int c_beg = bz_in * g.cps;
    int c_end = c_beg + g.cps;
    if (c_end > nchunk) c_end = nchunk;
    const int x_cs = g.IH * g.IW;
    const int R = g.PS >> 6;
    const float* xn = g.x + (long)n * g.x_bs;
    // tile row -> (image of the tile, lattice row); rows past the stacked images are dead (their results are not stored)
    auto rowmap = [&](int tyv, int& j, int& ty) -> bool {
        if (!STK || ipt <= 1) { j = 0; ty = tyv; return true; }
        j = tyv / g.OHt;
        ty = tyv - j * g.OHt;
        return j < ipt && n + j < g.B;
    };
    // patch offset of a tile row's first pixel (dead rows read row 0: any finite address inside the patch)
    auto prow = [&](int tr) -> int {
        if (!STK || ipt <= 1) return g.si * tr * g.PWr;
        int j, ty;
        return rowmap(tr, j, ty) ? (j * g.phi + g.si * ty) * g.PWr : 0;
    };

    auto load_patch = [&](int chunk, int buf) {
        float* dst = Ps + buf * CK * g.PS;
        if (g.aligned) {
            // 16-byte LDS-DMA: lane = one 4-float chunk of a patch row (rows are 16-byte aligned in x, see plan_conv);
            // a chunk is entirely inside or outside the image because IW % 4 == 0
            const int cpr = g.PWr >> 2;                       // chunks per patch row
            const int nq = g.PS >> 2;                         // chunks per channel (multiple of 16)
            for (int q0 = 0; q0 < nq; q0 += 64) {
                const int q = q0 + lane;
                const int pyt = q / cpr, qx = q - pyt * cpr;
                const int pj = (STK && ipt > 1) ? pyt / g.phi : 0, py = pyt - pj * g.phi;       // stacked images: patch rows [image][phi]
                const int iy = gy0 + py, ix = gx0 - g.shift + 4 * qx;
                const bool ok = (q < nq) && (pyt < g.PH) && (!STK || n + pj < g.B) && ((unsigned)iy < (unsigned)g.IH) && ((unsigned)ix < (unsigned)g.IW);
                const long go = (STK ? (long)pj * g.x_bs : 0l) + (long)iy * g.IW + ix;
#pragma unroll
                for (int k = 0; k < CK / 4; k++) {
                    const int cl = wid + 4 * k;
                    const int c = chunk * CK + cl;
                    const float* src = (ok && c < g.Cin) ? xn + (long)c * x_cs + go : g.zeros;
                    __builtin_amdgcn_global_load_lds(CC_GLOBAL_PTR(src), CC_LDS_PTR(dst + cl * g.PS + 4 * q0), 16, 0, 0);
                }
            }
            return;
        }
        for (int r = 0; r < R; r++) {
            const int pos = lane + 64 * r;
            const int pyt = pos / g.PWr, px = pos - pyt * g.PWr;
            const int pj = (STK && ipt > 1) ? pyt / g.phi : 0, py = pyt - pj * g.phi;
            const int iy = gy0 + py, ix = gx0 + px;
            const bool ok = (pyt < g.PH) && (!STK || n + pj < g.B) && ((unsigned)iy < (unsigned)g.IH) && ((unsigned)ix < (unsigned)g.IW);
            const long go = (STK ? (long)pj * g.x_bs : 0l) + (long)iy * g.IW + ix;
#pragma unroll
            for (int k = 0; k < CK / 4; k++) {
                const int cl = wid + 4 * k;
                const int c = chunk * CK + cl;
                const float* src = (ok && c < g.Cin) ? xn + (long)c * x_cs + go : g.zeros + lane;
                __builtin_amdgcn_global_load_lds(CC_GLOBAL_PTR(src), CC_LDS_PTR(dst + cl * g.PS + 64 * r), 4, 0, 0);
            }
        }
    };
    auto load_A = [&](int chunk, int tap0, int buf) {
        // per tap: CK rows of BM contiguous floats: wp[((tap*Cpad + chunk*CK + kk) * Mpad) + m0 + mm]
        constexpr int N4 = CK * BM / 4;                        // float4 count of one tap
#pragma unroll
        for (int tt = 0; tt < TPS; tt++) {
            if (tap0 + tt < T) {
                const float* base = g.wp + ((long)(tap0 + tt) * g.Cpad + (long)chunk * CK) * g.Mpad + m0;
                float* dst = As + (buf * TPS + tt) * CK * BM;
#pragma unroll
                for (int q = 0; q < (N4 + 255) / 256; q++) {
                    const int w4 = q * 256 + wid * 64;         // first float4 of this wave (uniform)
                    if (w4 < N4 && (N4 % 64 == 0 || w4 + lane < N4)) {        // BM = 16, CK = 8: half a wave (EXEC-masked DMA)
                        const int f = 4 * (w4 + lane);
                        const int kk = f / BM, mm = f - kk * BM;
                        __builtin_amdgcn_global_load_lds(CC_GLOBAL_PTR(base + (long)kk * g.Mpad + mm), CC_LDS_PTR(dst + 4 * w4), 16, 0, 0);
                    }
                }
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; a++)
#pragma unroll
        for (int b = 0; b < TN; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
    f32x4 acc16[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};      // BM == 16 only

    // patch offsets of this lane's pixels (one per lattice-row group of the wave)
    int poff[2] = {0, 0};
    if constexpr (STK && BM == 16) {
        const int l15 = lane & 15;
        poff[0] = prow(rowstep * row0) + g.si * l15;
        poff[1] = g.tw16 ? prow(rowstep * row0 + 1) + g.si * l15 : poff[0] + g.si * 16;
    } else if constexpr (STK != 0) {
#pragma unroll
        for (int b = 0; b < 2; b++) poff[b] = prow(rowstep * (row0 + (b < TN ? b : 0)) + lr) + g.si * lc;
    }
    if (c_beg < c_end) {
        load_patch(c_beg, c_beg & 1);
        load_A(c_beg, 0, 0);
        CC_WAIT_VMCNT0();
        __syncthreads();
        int s = 0;
        for (int chunk = c_beg; chunk < c_end; chunk++) {
            const float* Pb = Ps + (chunk & 1) * CK * g.PS;
            int ti = 0, tj = 0;
            for (int tap0 = 0; tap0 < T; tap0 += TPS, s++) {
                // prefetch the next stage's operands (other buffers; their last readers passed the previous barrier)
#ifndef CC_ABLATE_DMA          // ablation builds (tools/ablate_conv.sh): timing only, results are garbage
                if (tap0 + TPS < T) load_A(chunk, tap0 + TPS, (s + 1) & 1);
                else if (chunk + 1 < c_end) load_A(chunk + 1, 0, (s + 1) & 1);
                if (tap0 == 0 && chunk + 1 < c_end) load_patch(chunk + 1, (chunk + 1) & 1);
#endif
#pragma unroll
                for (int tt = 0; tt < TPS; tt++) {
                    if (tap0 + tt < T) {
                        const float* Ab = As + ((s & 1) * TPS + tt) * CK * BM;
                        const int tapoff = (g.dy_base + ti * g.dstep) * g.PWr + (g.dx_base + tj * g.dstep) + g.shift;
                        if constexpr (BM == 16) {
                            // 16x16x4: lane (i = lane & 15, k = lane >> 4) feeds A[m = i][k] and B[k][pixel = i]; two 16-pixel
                            // halves of the wave's lattice row -> two independent accumulators (40-cycle dependent latency)
                            const int l15 = lane & 15, l4 = lane >> 4;
                            const float* Pl = Pb + l4 * g.PS + (STK ? 0 : (g.si * rowstep * row0) * g.PWr + g.si * l15) + tapoff;
                            const float* Al = Ab + l4 * BM + l15;
                            const int half = g.tw16 ? g.si * g.PWr : g.si * 16;      // second 16-pixel half: next row / next 16 columns
                            float af[CK / 4], bf[CK / 4][2];
#pragma unroll
                            for (int ks = 0; ks < CK / 4; ks++) {
                                af[ks] = Al[(4 * ks) * BM];
                                bf[ks][0] = Pl[(4 * ks) * g.PS + (STK ? poff[0] : 0)];
                                bf[ks][1] = Pl[(4 * ks) * g.PS + (STK ? poff[1] : half)];
                            }
#pragma unroll
                            for (int ks = 0; ks < CK / 4; ks++) {
                                acc16[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ks], bf[ks][0], acc16[0], 0, 0, 0);
                                acc16[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ks], bf[ks][1], acc16[1], 0, 0, 0);
                            }
                            if (++tj == g.St) { tj = 0; ti++; }
                            continue;
                        }
                        const float* Pl = Pb + lk * g.PS + (STK ? 0 : (g.si * (rowstep * row0 + lr)) * g.PWr + g.si * lc) + tapoff;
                        const float* Al = Ab + lk * BM + wm * WM + l31;
                        // all fragments of a tap are fetched up front (2*(TM+TN)*CK/2 VGPRs): one exposed LDS latency per
                        // tap instead of one per k-step; the MFMAs then issue back to back behind counted lgkmcnt waits
                        float af[CK / 2][TM], bf[CK / 2][TN];
#pragma unroll
                        for (int ks = 0; ks < CK / 2; ks++) {
#ifdef CC_ABLATE_LDS
#pragma unroll
                            for (int a = 0; a < TM; a++) af[ks][a] = 1e-3f * (float)((lane & 7) + a);
#pragma unroll
                            for (int b = 0; b < TN; b++) bf[ks][b] = 1e-3f * (float)((lane & 3) + b);
#else
#pragma unroll
                            for (int a = 0; a < TM; a++) af[ks][a] = Al[(2 * ks) * BM + a * 32];
#pragma unroll
                            for (int b = 0; b < TN; b++) bf[ks][b] = Pl[(2 * ks) * g.PS + (STK ? poff[b] : (g.si * rowstep * b) * g.PWr)];
#endif
                        }
#pragma unroll
                        for (int ks = 0; ks < CK / 2; ks++) {
#pragma unroll
                            for (int a = 0; a < TM; a++)
#pragma unroll
                                for (int b = 0; b < TN; b++)
#ifdef CC_ABLATE_MFMA      // one VALU multiply-add instead of the 64-cycle matrix instruction: what the step costs WITHOUT the matrix work
                                    acc[a][b][0] = fmaf(af[ks][a], bf[ks][b], acc[a][b][0]);
#else
                                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ks][a], bf[ks][b], acc[a][b], 0, 0, 0);
#endif
                        }
                        if (++tj == g.St) { tj = 0; ti++; }
                    }
                }
                CC_WAIT_VMCNT0();
#ifndef CC_ABLATE_BARRIER
                __syncthreads();
#endif
            }
        }
    }

    const int y_cs = g.OH * g.OW;
    if constexpr (BM == 16) {
        // D col = lane & 15 -> pixel of the half, row = 4 * (lane >> 4) + r -> channel
        const int HWt = g.OHt * g.OWt;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            int ej, ty;
            if (!rowmap(ty0 + rowstep * row0 + (g.tw16 ? h : 0), ej, ty)) continue;
            const int tx = tx0 + (g.tw16 ? 0 : 16 * h) + (lane & 15);
            if (ty >= g.OHt || tx >= g.OWt) continue;
            const int n = STK ? n_tile + ej : n_tile;                          // (shadows the tile's first image)
            const long pix = (long)(g.oy0 + g.so * ty) * g.OW + (g.ox0 + g.so * tx);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = m0 + 4 * (lane >> 4) + r;
                if (m >= g.M) continue;
                if (SPLIT == 1 || (SPLIT == 2 && g.nsplit > 1)) {
                    const int Wp16 = g.tiles_x * (g.tw16 ? 16 : TW), Hp16 = g.tiles_y * (g.tw16 ? 8 : TH);      // padded slab rows
                    g.part[(long)bz_in * g.part_stride + (((long)n * g.M + m) * Hp16 + ty) * Wp16 + tx] = abl_fix(acc16[h][r]);
                } else {
                    float v = abl_fix(acc16[h][r]);
                    if (g.bias) v += g.bias[m];
                    const long o = (long)n * g.y_bs + pix + (long)m * y_cs;
                    const bool hr = g.res != nullptr;
                    g.y[o] = conv_tail(v, hr, hr ? g.res[(long)n * g.res_bs + pix + (long)m * y_cs] : 0.f, g.res_mul, g.act, g.act_a, g.act_b,
                                       g.add ? g.add[(long)n * g.add_bs + pix + (long)m * y_cs] : 0.f);
                }
            }
        }
        return;
    }
    // ---- epilogue (round 3): 16-byte stores.  The MFMA result has one PIXEL per lane and 16 channel rows per register set: storing
    // it as it lies costs 16 scalar stores per 32x32 tile (64 per wave).  Each tile goes through a wave-private 4 KB LDS block
    // (free after the main loop's last barrier) and comes back as float4 = 4 consecutive pixels of one channel row: 4 dwordx4
    // stores per tile; residual / add / mul operands are read as float4 the same way (same-box A/B: -0.22 ms/step).
    //   write: lane (pixel c = lane & 31, half lk) -> T[row][c], row = (r & 3) + 8 * (r >> 2) + 4 * lk   (32 consecutive floats per
    //          32-lane group: conflict-free);  read k = 0..3: lane -> row 8k + (lane >> 3), columns 4 * (lane & 7) .. +3.
    // Partial slabs (split-K) are padded to whole tiles, [split][n][m][tiles_y * th][tiles_x * tw]: every 16-byte store is aligned and
    // in bounds without a guard.
    float* Tt = smem + wid * 1024;
    const int c4 = (lane & 7) * 4, rsub = lane >> 3;
    const int lr4 = g.tw16 ? (c4 >> 4) : 0, lc4 = g.tw16 ? (c4 & 15) : c4;
    const int tx = tx0 + lc4;
    const int Wp = g.tiles_x * (g.tw16 ? 16 : TW), Hp = g.tiles_y * (g.tw16 ? 8 : TH);
    const bool split = (SPLIT == 1 || (SPLIT == 2 && g.nsplit > 1));
    const bool vec = g.vec4 != 0;       // 16-byte path of the fused epilogue (decided on the host, make_cp)
    // One 32x32 accumulator tile at a time, called with literal (a, b): a loop over acc[a][b] that the compiler does not fully unroll
    // sends the accumulators to scratch memory -- in the MAIN loop as well.  Split and fused forms are separate code paths behind one
    // uniform branch, so that neither keeps the other's operands alive (the multi-problem kernel is at the SGPR limit).
    auto stage = [&](const f32x16& A) {
#pragma unroll
        for (int r = 0; r < 16; r++) Tt[((r & 3) + 8 * (r >> 2) + 4 * lk) * 32 + l31] = abl_fix(A[r]);
        __builtin_amdgcn_wave_barrier();
    };
    if (split) {
        auto tile = [&](const f32x16& A, const int a, const int b) {
            stage(A);
            int ej, ty;
            const bool rowok = rowmap(ty0 + rowstep * (row0 + b) + lr4, ej, ty);
            // the slab is padded so that every store is aligned and in bounds, but the padding is never read: quads that start
            // outside the image are not written (the 2x7 / 4x13 layers would otherwise write 5-18x their partial sums)
            const bool live = rowok && ty < g.OHt && tx < g.OWt;
            float* pb = g.part + (long)bz_in * g.part_stride + (((long)(n + ej) * g.M + (m0 + wm * WM + a * 32 + rsub)) * Hp + ty) * Wp + tx;
            const long mstep = (long)8 * Hp * Wp;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float4 v = *reinterpret_cast<const float4*>(&Tt[(8 * k + rsub) * 32 + c4]);
                if (m0 + wm * WM + a * 32 + 8 * k + rsub < g.M && live) {
                    *reinterpret_cast<float4*>(pb + k * mstep) = v;
#ifdef CC_ABLATE_STORE
                    *reinterpret_cast<volatile float4*>(pb + k * mstep) = v;
#endif
                }
            }
            __builtin_amdgcn_wave_barrier();
        };
        tile(acc[0][0], 0, 0);
        if constexpr (TN > 1) tile(acc[0][1], 0, 1);
        if constexpr (TM > 1) {
            tile(acc[1][0], 1, 0);
            if constexpr (TN > 1) tile(acc[1][1], 1, 1);
        }
        return;
    }
    const bool hr = g.res != nullptr, ha = g.add != nullptr;
    auto tile = [&](const f32x16& A, const int a, const int b) {
        stage(A);
        int ej, ty;
        const bool rowok = rowmap(ty0 + rowstep * (row0 + b) + lr4, ej, ty);
        const bool inside = rowok && ty < g.OHt && tx < g.OWt;
        const int n = STK ? n_tile + ej : n_tile;                              // (shadows the tile's first image)
        const long pix = (long)(g.oy0 + g.so * ty) * g.OW + (g.ox0 + g.so * tx);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float4 v = *reinterpret_cast<const float4*>(&Tt[(8 * k + rsub) * 32 + c4]);
            const int m = m0 + wm * WM + a * 32 + 8 * k + rsub;
            if (m < g.M && inside) {
                const long o = (long)m * y_cs + pix;
                const float bias = g.bias ? g.bias[m] : 0.f;
                const float v0 = v.x + bias, v1 = v.y + bias, v2 = v.z + bias, v3 = v.w + bias;
                if (vec && tx + 3 < g.OWt) {
                    float4 rr = make_float4(0.f, 0.f, 0.f, 0.f), aa = rr;
                    if (hr) rr = *reinterpret_cast<const float4*>(g.res + (long)n * g.res_bs + o);
                    if (ha) aa = *reinterpret_cast<const float4*>(g.add + (long)n * g.add_bs + o);
                    float4 out;
                    out.x = conv_tail(v0, hr, rr.x, g.res_mul, g.act, g.act_a, g.act_b, aa.x);
                    out.y = conv_tail(v1, hr, rr.y, g.res_mul, g.act, g.act_a, g.act_b, aa.y);
                    out.z = conv_tail(v2, hr, rr.z, g.res_mul, g.act, g.act_a, g.act_b, aa.z);
                    out.w = conv_tail(v3, hr, rr.w, g.res_mul, g.act, g.act_a, g.act_b, aa.w);
                    *reinterpret_cast<float4*>(g.y + (long)n * g.y_bs + o) = out;
#ifdef CC_ABLATE_STORE
                    *reinterpret_cast<volatile float4*>(g.y + (long)n * g.y_bs + o) = out;
#endif
                } else {
                    const long st = g.so;
                    float* yo = g.y + (long)n * g.y_bs + o;
                    const float* ro = hr ? g.res + (long)n * g.res_bs + o : nullptr;
                    const float* ao = ha ? g.add + (long)n * g.add_bs + o : nullptr;
                    yo[0] = conv_tail(v0, hr, hr ? ro[0] : 0.f, g.res_mul, g.act, g.act_a, g.act_b, ao ? ao[0] : 0.f);
                    if (tx + 1 < g.OWt) yo[st] = conv_tail(v1, hr, hr ? ro[st] : 0.f, g.res_mul, g.act, g.act_a, g.act_b, ao ? ao[st] : 0.f);
                    if (tx + 2 < g.OWt) yo[2 * st] = conv_tail(v2, hr, hr ? ro[2 * st] : 0.f, g.res_mul, g.act, g.act_a, g.act_b, ao ? ao[2 * st] : 0.f);
                    if (tx + 3 < g.OWt) yo[3 * st] = conv_tail(v3, hr, hr ? ro[3 * st] : 0.f, g.res_mul, g.act, g.act_a, g.act_b, ao ? ao[3 * st] : 0.f);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    tile(acc[0][0], 0, 0);
    if constexpr (TN > 1) tile(acc[0][1], 0, 1);
    if constexpr (TM > 1) {
        tile(acc[1][0], 1, 0);
        if constexpr (TN > 1) tile(acc[1][1], 1, 1);
    }
}

// Workgroup -> (tile, channel block, split) in XCD order (cc_common.h).  Input-major (wmajor 0): the tiles in XCD order, channel block
// and split as dispatched -- an XCD's L2 sees a contiguous run of tiles (shared halos) and, whenever gridDim.x is a multiple of 8, all
// channel blocks and splits of a tile (same input patch).  Weight-major (wmajor 1): the whole grid in XCD order, tiles fastest -- an
// XCD works through ALL tiles of a contiguous range of (channel block, split) pairs, so a slice of the weight image is streamed from
// HBM by one XCD instead of by all eight (512 -> 512 3x3 on 8x26: 9.4 MB of weights against 1.7 MB of input).
__device__ __forceinline__ void conv_xcd_blocks(int wmajor, int& bx, int& by, int& bz) {
    bx = (int)blockIdx.x; by = (int)blockIdx.y; bz = (int)blockIdx.z;
    if constexpr (!(CC_XCD_MASK & 1)) return;
    if (wmajor < 0) return;
    if (wmajor) {
        const int gx = (int)gridDim.x, gy = (int)gridDim.y;
        const int w = cc_xcd_order(bx + gx * (by + gy * bz), gx * gy * (int)gridDim.z);
        const int r = w / gx;
        bx = w - r * gx;
        bz = r / gy;
        by = r - bz * gy;
    } else {
        bx = cc_xcd_order(bx, (int)gridDim.x);
    }
}

// min 4 waves per SIMD (<= 128 registers): the accumulators then live in VGPRs (95-99 registers in total, no spill) instead of
// 64 AGPRs + 72-85 VGPRs, and four 40 KB workgroups fit a CU (CC_PATCH_LB: A/B builds, tools/)
#ifndef CC_PATCH_LB
#define CC_PATCH_LB 4
#endif
template <int BM, int CK, int TPS, int SPLIT>
__global__ __launch_bounds__(256, CC_PATCH_LB) void k_conv_patch(CP g) {
    int bx, by, bz;
    conv_xcd_blocks(g.wmajor, bx, by, bz);
    conv_patch_body<BM, CK, TPS, SPLIT, 0>(g, bx, by, bz);
}
template <int BM, int TPS, int SPLIT>          // stacked tiny maps (8-channel chunks only)
__global__ __launch_bounds__(256, CC_PATCH_LB) void k_conv_patch_stk(CP g) {
    int bx, by, bz;
    conv_xcd_blocks(g.wmajor, bx, by, bz);
    conv_patch_body<BM, 8, TPS, SPLIT, 1>(g, bx, by, bz);
}

// The (up to) four output-parity classes of a stride-2 data-gradient / transposed convolution in ONE launch:
// blockIdx.x ranges over the classes' tiles back to back (each class has its own geometry, weight image and partial
// slabs; the small-map layers are launch-bound, and four quarter-size grids in a row under-fill the chip).
// ... and, more generally, up to MAXCLS independent problems of one tile configuration in ONE launch: the G same-shaped
// convolutions of a network's parallel branches (Back2Future's decoder_fwd / decoder_bwd / decoder_occ at one pyramid level,
// its a / b / c feature streams) times their parity classes.  The deep pyramid levels are 1-4 GFLOP problems: one launch per
// group instead of one per branch triples the work per launch, needs a third of the split-K (partial-slab traffic) and
// removes two thirds of the ~5 us launch floors.
constexpr int MAXCLS = 12;
struct CPM {
    CP c[MAXCLS];
    int n;
    int bx_end[MAXCLS];
    int wmajor;            // as CP::wmajor, for the launch (the classes' weights against their inputs)
};

// (a macro, not a function taking the argument block by reference: the kernel reads its class descriptor from the kernel-argument
// segment, and the wrapper cost nine more scalar spills)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CC_HIPEMU)
#define CC_MULTI_DESC(a, k) (*(reinterpret_cast<const CP*>((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(CPM, c)) + (k)))
#else
#define CC_MULTI_DESC(a, k) ((a).c[k])
#endif
// the class descriptor is read straight from the kernel-argument segment (scalar loads at a run-time offset): indexing the
// by-value argument `a.c[k]` makes the compiler copy descriptors to scratch memory once the body is large
#define CC_MULTI_BODY(BM_, CK_, TPS_, STK_)                                                                                   \
    int bx, by, bz;                                                                                                           \
    conv_xcd_blocks(a.wmajor ? 1 : -1, bx, by, bz);      /* -1: as dispatched (the class's tiles are put in XCD order below) */  \
    int k = 0, first = 0, end = a.bx_end[0];                                                                                  \
    _Pragma("unroll") for (int q = 0; q < MAXCLS - 1; q++)                                                                    \
        if (q + 1 < a.n && bx >= a.bx_end[q]) { k = q + 1; first = a.bx_end[q]; end = a.bx_end[q + 1]; }                      \
    const CP& g = CC_MULTI_DESC(a, k);                                                                                        \
    if (bz >= g.nsplit || by * BM_ >= g.Mpad) return;     /* grid.y / grid.z are the launch's maxima */                        \
    bx -= first;                                                                                                              \
    if ((CC_XCD_MASK & 1) && !a.wmajor) bx = cc_xcd_order(bx, end - first);                                                   \
    conv_patch_body<BM_, CK_, TPS_, 2, STK_>(g, bx, by, bz);

template <int BM, int CK, int TPS>
__global__ __launch_bounds__(256, CC_PATCH_LB) void k_conv_patch_multi(CPM a) { CC_MULTI_BODY(BM, CK, TPS, 0) }
template <int BM, int TPS>                     // at least one class with stacked tiny maps (the others have ipt = 1)
__global__ __launch_bounds__(256, CC_PATCH_LB) void k_conv_patch_multi_stk(CPM a) { CC_MULTI_BODY(BM, 8, TPS, 1) }

// y[lattice pixel] = act(bias + res + sum_k part[k])  (second, deterministic stage of split-K)
__global__ __launch_bounds__(256) void k_splitk_epilogue(const float* __restrict__ part, int nsplit, long part_stride,
                                                         const float* __restrict__ bias, const float* __restrict__ res,
                                                         float* __restrict__ y, int M, int OHt, int OWt, int so, int oy0,
                                                         int ox0, int OH, int OW, long y_bs, long res_bs, long total,
                                                         int act, float act_a, float act_b, int res_mul,
                                                         const float* add, long add_bs, int Hp, int Wp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int HWt = OHt * OWt;
    const long per = (long)M * HWt;
    const int n = (int)(e / per);
    const long r = e - (long)n * per;
    const int m = (int)(r / HWt);
    const int t = (int)(r - (long)m * HWt);
    const int ty = t / OWt, tx = t - ty * OWt;
    // the slabs are padded to whole tiles: [split][n][m][Hp][Wp]
    const long po = (((long)n * M + m) * Hp + ty) * Wp + tx;
    // eight partial loads in flight, added in split order (a one-by-one loop is a chain of nsplit dependent HBM/L2 latencies and
    // this kernel is nothing else)
    float v = 0.f;
    {
        for (int k = 0; k < nsplit; k += 8) {
            float p8[8];
#pragma unroll
            for (int u = 0; u < 8; u++) p8[u] = (k + u < nsplit) ? part[(long)(k + u) * part_stride + po] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (k + u < nsplit) v += p8[u];
        }
    }
    const long o = (long)m * OH * OW + (long)(oy0 + so * ty) * OW + (ox0 + so * tx);
    if (bias) v += bias[m];
    y[(long)n * y_bs + o] = conv_tail(v, res != nullptr, res ? res[(long)n * res_bs + o] : 0.f, res_mul, act, act_a, act_b,
                                      add ? add[(long)n * add_bs + o] : 0.f);
}

// every class carries its own geometry and epilogue (round 3: the problems of one launch may come from different layers of
// different networks -- cc_conv2d_list)
struct EPC {
    const float* part; const float* bias; const float* res; const float* add; float* y;
    int nsplit; long part_stride; int OHt, OWt, oy0, ox0; long total;
    int Hp, Wp;                      // padded slab rows / pitch (whole tiles)
    int M, so, OH, OW; long y_bs, res_bs, add_bs;
    int act; float act_a, act_b;
    int res_mul;
};
struct EPM {
    EPC c[MAXCLS];
    int n;
    int bx_end[MAXCLS];
};

__global__ __launch_bounds__(256) void k_splitk_epilogue_multi(EPM a) {
    int k = 0, first = 0;
#pragma unroll
    for (int q = 0; q < MAXCLS - 1; q++)
        if (q + 1 < a.n && (int)blockIdx.x >= a.bx_end[q]) { k = q + 1; first = a.bx_end[q]; }
    const EPC& c = a.c[k];
    const long e = (long)((int)blockIdx.x - first) * 256 + threadIdx.x;
    if (e >= c.total) return;
    const int HWt = c.OHt * c.OWt;
    const long per = (long)c.M * HWt;
    const int n = (int)(e / per);
    const long r = e - (long)n * per;
    const int m = (int)(r / HWt);
    const int t = (int)(r - (long)m * HWt);
    const int ty = t / c.OWt, tx = t - ty * c.OWt;
    const long po = (((long)n * c.M + m) * c.Hp + ty) * c.Wp + tx;
    float v = 0.f;
    {
        for (int z = 0; z < c.nsplit; z += 8) {      // see k_splitk_epilogue
            float p8[8];
#pragma unroll
            for (int u = 0; u < 8; u++) p8[u] = (z + u < c.nsplit) ? c.part[(long)(z + u) * c.part_stride + po] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (z + u < c.nsplit) v += p8[u];
        }
    }
    const long o = (long)m * c.OH * c.OW + (long)(c.oy0 + c.so * ty) * c.OW + (c.ox0 + c.so * tx);
    if (c.bias) v += c.bias[m];
    c.y[(long)n * c.y_bs + o] = conv_tail(v, c.res != nullptr, c.res ? c.res[(long)n * c.res_bs + o] : 0.f, c.res_mul, c.act, c.act_a, c.act_b,
                                          c.add ? c.add[(long)n * c.add_bs + o] : 0.f);
}

// ------------------------------------------------------------------ planning (host)
struct ConvPlan {
    bool use_patch;
    int wino;                  // Winograd F(2x2, 3x3) kernel (wino.hip): wn holds its plan, wp_floats the size of the U image
    ccint::WinoPlan wn;
    int Hp, Wp;                // rows / pitch of the split-K partial slabs [split][n][m][Hp][Wp]
    int tw16;
    int ipt, phi;              // stacked tiny maps (CP::ipt)
    int bm, ck, tps, Mpad, Cpad, PH, PWr, PS, ymin, xmin, tiles_x, tiles_y, nsplit, cps, aligned, shift;
    size_t smem, wp_floats, part_floats;
    int wpad;                  // Winograd over a zero-padded copy of the input (maps whose width is not a multiple of 4): its row pitch
    size_t pad_floats;         // ... and size (behind the partial slabs in the workspace)
};

// pixel tiles of a problem (grid.x of its launch): stacked tiny maps take one tile per ipt images
inline long conv_tiles(const GG& g, const ConvPlan& p) { return (long)((g.B + p.ipt - 1) / p.ipt) * p.tiles_x * p.tiles_y; }

// workgroups before split-K; mult: number of same-shaped problems that share the launch (split-K only has to fill what they leave empty)
inline long conv_blocks(const GG& g, const ConvPlan& p, int mult) { return conv_tiles(g, p) * (p.Mpad / p.bm) * (mult > 1 ? mult : 1); }

// dynamic LDS of a patch-kernel workgroup with `tps` taps per stage: A buffers [2][tps][ck][bm] + patch buffers [2][ck][PS]; the
// epilogue transposes one 32x32 tile per wave through LDS (4 KB per wave)
inline size_t patch_smem(const ConvPlan& p, int tps) {
    const size_t b = (size_t)(2 * tps * p.ck * p.bm + 2 * p.ck * p.PS) * sizeof(float);
    return (p.bm >= 32 && b < 16384) ? 16384 : b;
}

// split-K over the nchunk channel chunks into (about) `want` slices; the slabs are padded to whole tiles (p.Hp x p.Wp)
inline void set_split(ConvPlan& p, const GG& g, int nchunk, long want) {
    p.nsplit = 1; p.cps = nchunk;
    if (want >= 2) {
        p.cps = (int)((nchunk + want - 1) / want);
        p.nsplit = (nchunk + p.cps - 1) / p.cps;
    }
    p.part_floats = p.nsplit > 1 ? (size_t)p.nsplit * g.B * g.M * p.Hp * p.Wp : 0;
}

// 3x3 / stride 1 / pad 1 on the full lattice, taps forwards (conv2d) or backwards (its data-gradient)
inline bool wino_geometry(const GG& g) {
    return g.Rt == 3 && g.St == 3 && g.si == 1 && g.so == 1 && g.oy0 == 0 && g.ox0 == 0 && (g.dstep == 1 || g.dstep == -1) &&
           g.dy0 == -g.dstep && g.dx0 == -g.dstep && g.IH == g.OH && g.IW == g.OW && g.OHt == g.OH && g.OWt == g.OW && g.Cin > 0 &&
           (long)g.B * g.Cin * g.IH * g.IW < (1l << 26);
}

// the plan of the Winograd kernel as the problem's plan; wpad: row pitch of the zero-padded input copy it runs over (0: the input itself)
inline void adopt_wino(ConvPlan& p, const ccint::WinoPlan& w, const GG& g, int wpad = 0) {
    p.wino = 1;
    p.wn = w;
    p.use_patch = true;
    p.bm = ccwino::WBM; p.ck = ccwino::WCK; p.tps = 1;
    p.Mpad = w.Mpad; p.Cpad = w.Cpad;
    p.nsplit = w.nsplit; p.cps = w.cps;
    p.Hp = w.Hp; p.Wp = w.Wp;
    p.wp_floats = w.u_floats;
    p.part_floats = w.part_floats;
    p.wpad = wpad;
    p.pad_floats = wpad ? ((size_t)g.B * g.Cin * g.IH * wpad + 3) & ~(size_t)3 : 0;
}

// step 2, Winograd over a padded copy.  Maps whose width is not a multiple of 4 (the 8x26 level of DispResNet6: 512- / 1024-channel
// layers, 4 GFLOP each on the direct kernel + a split-K epilogue): the Winograd kernel stages aligned 16-byte row pieces, so the input
// is first copied into rows padded with zeros to the next width it takes (k_pad_rows; zero columns ARE the convolution's padding) and
// the launch is always split-K: the partial slabs have the padded pitch, and the deterministic epilogue kernel that sums them writes
// the real output.  Large layers only (the copy, 23 % empty tile columns and the forced second pass have to pay), never for the
// grouped launches of parallel branches (they share one direct launch today).
inline bool plan_wino_padded(ConvPlan& p, const GG& g, int mult) {
    if (cctools::env_flag("CC_NO_WINO_PAD") || (g.IW % 4) == 0 || g.IH < 2 || g.M < cctools::env_int("CC_WINOP_MINM", 256) ||
        g.Cin < cctools::env_int("CC_WINOP_MINC", 256))
        return false;
    int wp = (g.IW + 3) & ~3;
    while (!(wp / 2 >= 16 || wp / 2 == 8)) wp += 4;
    if (!(4 * (wp - g.IW) <= wp && (long)g.B * ((g.IH + 1) / 2) * (wp / 2) >= cctools::env_int("CC_WINOP_MINQ", 64))) return false;
    ccint::WinoPlan wq = ccint::wino_plan(g.B, g.Cin, g.IH, wp, g.M, mult);
    if (!wq.ok) return false;
    if (wq.nsplit < 2) {                    // the epilogue pass is what un-pads the output
        if (wq.tile == 2) wq.tile = 1;      // (the eight-wave instance halves the reduction itself: no slices across workgroups)
        wq.cps = (wq.nchunk + 1) / 2;
        wq.nsplit = (wq.nchunk + wq.cps - 1) / wq.cps;
        wq.part_floats = (size_t)wq.nsplit * g.B * g.M * wq.Hp * wq.Wp;
    }
    if (wq.nsplit < 2) return false;
    adopt_wino(p, wq, g, wp);
    return true;
}

// step 3, channel tile
inline void plan_channel_tile(ConvPlan& p, const GG& g) {
    p.bm = pick_bm_fwd(g.M);
    // a narrower channel tile when it saves >= 25 % of the PADDED output channels: M = 65 / 96 -> 3 x 32 instead of 128,
    // 129 -> 3 x 64 instead of 256, 260 -> 9 x 32 instead of 384 (concatenations with a 1-2 channel map, the 96-channel
    // decoder layers): -0.33 ms/step (r3s3 A/B; thresholds 12-25 % equal, 35 % loses it)
    const int thr = cctools::env_int("CC_CONV_BM_PADSAVE", 25);
    if (thr > 0 && p.bm > 32) {
        const int cur = ((g.M + p.bm - 1) / p.bm) * p.bm;
        for (int b2 = p.bm / 2; b2 >= 32; b2 /= 2) {
            const int m2 = ((g.M + b2 - 1) / b2) * b2;
            if ((cur - m2) * 100 >= thr * cur) { p.bm = b2; break; }
        }
    }
}

// step 4, pixel tile / stacking (and the channel tile once more, now that the tile count is known)
inline void plan_pixel_tile(ConvPlan& p, const GG& g) {
    {   // tile shape: 4 x 32 or 8 x 16 lattice pixels, whichever covers the map with fewer padded pixels
        const long a32 = (long)((g.OWt + 31) / 32) * 32 * (((g.OHt + 3) / 4) * 4);
        const long a16 = (long)((g.OWt + 15) / 16) * 16 * (((g.OHt + 7) / 8) * 8);
        // ties (all maps of <= 16x52: both shapes pad them equally) go to 8 x 16: -0.07 ms/step (r3s3)
        p.tw16 = ((a16 < a32 || (a16 == a32 && cctools::env_int("CC_CONV_TW16_TIES", 1))) && !cctools::env_flag("CC_CONV_NO_TW16")) ? 1 : 0;
    }
    // Maps of <= 4 lattice rows (DispResNet6's 4x13 / 2x7 / 1x4 levels and their parity classes): one image fills 1-4 of the 8 tile
    // rows and the matrix cores multiply padding (a 2x7 map: 14 live pixels of 128).  The 8 x 16 tile then stacks the rows of
    // 8 / OHt consecutive images, each with its own halo rows in the patch.
    p.ipt = 1;
    if (g.OHt <= 4 && g.B >= 2 && cctools::env_int("CC_CONV_STACK", 1) && !cctools::env_flag("CC_CONV_CK16")) {
        p.tw16 = 1;
        p.ipt = 8 / g.OHt < g.B ? 8 / g.OHt : g.B;
    }
    const int th = p.tw16 ? 8 : TH, tw = p.tw16 ? 16 : TW;
    p.tiles_x = (g.OWt + tw - 1) / tw;
    p.tiles_y = (g.OHt + th - 1) / th;
    // partial slabs are padded to whole tiles (16-byte stores without guards): [split][n][m][tiles_y * th][tiles_x * tw]
    p.Hp = p.tiles_y * th;
    p.Wp = p.tiles_x * tw;
    {   // few pixel tiles: shrink the channel tile (more workgroups, every one over the whole reduction) before resorting to
        // split-K (partial slabs + an epilogue launch); CC_CONV_BM_MINBLOCKS: block count below which the tile is halved
        const long tiles = (long)g.B * p.tiles_x * p.tiles_y;
        const int thr = cctools::env_int("CC_CONV_BM64_BELOW", 0);
        if (p.bm == 128 && tiles * ((g.M + 127) / 128) < thr) p.bm = 64;
        const int minb = cctools::env_int("CC_CONV_BM_MINBLOCKS", 0);
        while (p.bm > 32 && tiles * ((g.M + p.bm - 1) / p.bm) < minb) p.bm /= 2;
    }
}

// step 5, patch geometry and LDS
inline void plan_patch(ConvPlan& p, const GG& g) {
    const int th = p.tw16 ? 8 : TH, tw = p.tw16 ? 16 : TW;
    const int ylast = g.dy0 + (g.Rt - 1) * g.dstep, xlast = g.dx0 + (g.St - 1) * g.dstep;
    p.ymin = g.dy0 < ylast ? g.dy0 : ylast;
    p.xmin = g.dx0 < xlast ? g.dx0 : xlast;
    const int ymax = g.dy0 < ylast ? ylast : g.dy0, xmax = g.dx0 < xlast ? xlast : g.dx0;
    p.PH = (th - 1) * g.si + (ymax - p.ymin) + 1;
    p.phi = 0;
    if (p.ipt > 1) {
        p.phi = (g.OHt - 1) * g.si + (ymax - p.ymin) + 1;
        p.PH = p.ipt * p.phi;
    }
    p.PWr = (tw - 1) * g.si + (xmax - p.xmin) + 1;
    // 16-byte aligned variant: start every patch row at the 4-float boundary at or below its first column
    p.aligned = (g.IW % 4 == 0) && !cctools::env_flag("CC_NO_ALIGNED_PATCH");
    p.shift = 0;
    if (p.aligned) {
        p.shift = ((p.xmin % 4) + 4) % 4;                  // si * tx0 is a multiple of 4
        p.PWr = ((p.shift + p.PWr + 3) / 4) * 4;
    }
    p.PS = ((p.PH * p.PWr + 63) / 64) * 64;
    if (p.aligned) p.PS = ((p.PH * p.PWr + 255) / 256) * 256;     // whole 64-lane x 16-byte DMA instructions per channel
    // 8-channel chunks: 20-40 KB of LDS per workgroup -> 3 (BM = 128, register-limited) to 7 workgroups per CU.  Measured
    // against 16-channel chunks (80 KB, two per CU, half as many barriers): -0.8 ms/step in total (r02g-r02i A/Bs);
    // CC_CONV_CK16=1 restores the round-1 plan (16 wherever one stage fits in 64 KB).
    p.ck = 16;
    if (!(cctools::env_flag("CC_CONV_CK16") && patch_smem(p, 1) <= 64 * 1024)) p.ck = 8;
    // three taps per pipeline stage when the extra weight buffers still leave two workgroups per CU (2 x 80 KB)
    p.tps = (g.Rt * g.St >= 3 && patch_smem(p, 3) <= 80 * 1024 && !cctools::env_flag("CC_CONV_TPS1")) ? 3 : 1;
    p.smem = patch_smem(p, p.tps);
    p.use_patch = (p.smem <= 150 * 1024) && g.Cin > 0;
    p.Mpad = ((g.M + p.bm - 1) / p.bm) * p.bm;
    p.Cpad = ((g.Cin + p.ck - 1) / p.ck) * p.ck;
    p.wp_floats = (size_t)g.Rt * g.St * p.Cpad * p.Mpad;
}

// step 6, split-K: launches that leave the chip empty slice the reduction
inline void plan_split(ConvPlan& p, const GG& g, int mult) {
    const long blocks = conv_blocks(g, p, mult);
    const int nchunk = p.Cpad / p.ck;
    long want = 1;
    if (blocks < cctools::env_int("CC_CONV_SPLIT_BELOW", 384) && nchunk >= 4 && !(g.so != 1 && cctools::env_flag("CC_DBG_NO_PARITY_SPLIT"))) {
        want = (cctools::env_int("CC_CONV_SPLIT_TARGET", 512) + blocks - 1) / blocks;
        if (want > nchunk / cctools::env_int("CC_CONV_MINCHUNKS", 1)) want = nchunk / cctools::env_int("CC_CONV_MINCHUNKS", 1);
        if (want > cctools::env_int("CC_CONV_MAXSPLIT", 32)) want = cctools::env_int("CC_CONV_MAXSPLIT", 32);
    }
    set_split(p, g, nchunk, want);
}

// step 7, balance.  Wave quantisation (round 3): a launch of 257..~1000 workgroups runs as ceil(blocks / 256) "rounds" on the 256 CUs
// -- the MFMA pipes of a CU are saturated by one workgroup, so k co-resident workgroups take k times as long -- e.g. the 336
// workgroups of Back2Future's level-3 decoder groups (32x104 maps, G = 3) cost two rounds for 1.3 rounds of work.  A modest
// split-K re-balances them when the reduction is long enough to pay for the partial slabs.  Cost model (microseconds):
//   T(ns) = ceil(blocks * ns / 256) * (stages / ns) * t_stage(BM) + 2.5  [+ 2 * ns * out_bytes / 3 TB/s + 5 when ns > 1]
// calibrated on the split-K launches of the step (512->512 on 8x26: model 59 us, measured 63).
inline void plan_balance(ConvPlan& p, const GG& g, int mult) {
    const long blocks = conv_blocks(g, p, mult);
    const int nchunk = p.Cpad / p.ck;
    if (!(blocks >= 256 && nchunk >= 8 && cctools::env_int("CC_CONV_BALANCE", 1))) return;
    const int T = g.Rt * g.St;
    const double mfma_cyc = (p.bm == 128 ? 3072.0 : p.bm == 64 ? 1536.0 : p.bm == 32 ? 768.0 : 384.0) * (p.tps == 3 ? 1.0 : 1.0 / 3.0);
    const double t_stage = mfma_cyc / 2100.0;
    const double stages = (double)nchunk * ((T + p.tps - 1) / p.tps);
    const double out_bytes = 4.0 * g.B * g.M * g.OHt * g.OWt * (mult > 1 ? mult : 1);
    auto cost = [&](int ns) {
        const double k = (double)((blocks * ns + 255) / 256);
        double t = k * (stages / ns) * t_stage + 2.5;
        if (ns > 1) t += 2.0 * ns * out_bytes / 3.0e6 + 5.0;
        return t;
    };
    int best = 1;
    const int cap = nchunk / 4 < 8 ? nchunk / 4 : 8;
    for (int ns = 2; ns <= cap; ns++)
        if (cost(ns) < cost(best)) best = ns;
    if (best > 1 && cost(best) < 0.01 * cctools::env_int("CC_CONV_BALANCE_PCT", 97) * cost(1)) set_split(p, g, nchunk, best);
}

inline ConvPlan plan_conv(const GG& g, int mult = 1) {
    ConvPlan p = {};
    p.ipt = 1;
    if (wino_geometry(g)) {     // step 1, Winograd: a function of the geometry alone (the weight image is laid out for it); `mult` only moves split-K
        const ccint::WinoPlan w = ccint::wino_plan(g.B, g.Cin, g.IH, g.IW, g.M, mult);
        if (w.ok) adopt_wino(p, w, g);
        if (w.ok || plan_wino_padded(p, g, mult)) return p;
    }
    plan_channel_tile(p, g);
    plan_pixel_tile(p, g);
    plan_patch(p, g);
    plan_split(p, g, mult);
    plan_balance(p, g, mult);
    return p;
}

// ---- workspace area of one problem: [64 zeros][weight image (unless the call brings a prepacked one)][partial slabs][padded input
// copy]; sized by conv_ws_floats.  A prepacked image has the same head: [64 zeros][weight image(s)].
inline size_t conv_ws_floats(const ConvPlan& p) { return 64 + p.wp_floats + p.part_floats + p.pad_floats; }
template <class F> inline F* ws_image(F* area) { return area + 64; }
inline float* ws_slabs(float* area, size_t image_floats) { return area + 64 + image_floats; }

// ------------------------------------------------------------------ launch (host)
inline void launch_gg_flat(const GG& g, hipStream_t s) {
    const long Ntot = (long)g.B * g.OHt * g.OWt;
    const int bm = pick_bm(g.M);
    dim3 grid((unsigned)((Ntot + BN - 1) / BN), (unsigned)((g.M + bm - 1) / bm));
    if (bm == 128) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gather_gemm<128>), grid, dim3(256), 0, s, g);
    else if (bm == 64) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gather_gemm<64>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gather_gemm<32>), grid, dim3(256), 0, s, g);
}

// one launch of the kernel instance KERN; > 64 KB of dynamic LDS has to be requested once per kernel (the flag is per instance)
template <auto KERN, class ARGS>
inline void launch_instance(const ARGS& c, dim3 grid, size_t smem, hipStream_t s) {
    static bool big_lds_enabled = false;
    if (smem > 64 * 1024 && !big_lds_enabled) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        big_lds_enabled = true;
    }
    hipLaunchKernelGGL(KERN, grid, dim3(256), smem, s, c);
}

inline bool stacked(const CPM& a) {
    for (int k = 0; k < a.n; k++)
        if (a.c[k].ipt > 1) return true;
    return false;
}

template <int BM, int CK, int TPS>
inline void launch_patch(const CP& c, dim3 grid, size_t smem, hipStream_t s) {
    if constexpr (CK == 8) {
        if (c.ipt > 1) {
            if (c.nsplit > 1) launch_instance<&k_conv_patch_stk<BM, TPS, 1>>(c, grid, smem, s);
            else launch_instance<&k_conv_patch_stk<BM, TPS, 0>>(c, grid, smem, s);
            return;
        }
    }
    if (c.nsplit > 1) launch_instance<&k_conv_patch<BM, CK, TPS, 1>>(c, grid, smem, s);
    else launch_instance<&k_conv_patch<BM, CK, TPS, 0>>(c, grid, smem, s);
}

template <int BM, int CK, int TPS>
inline void launch_patch(const CPM& c, dim3 grid, size_t smem, hipStream_t s) {
    if constexpr (CK == 8) {
        if (stacked(c)) { launch_instance<&k_conv_patch_multi_stk<BM, TPS>>(c, grid, smem, s); return; }
    }
    launch_instance<&k_conv_patch_multi<BM, CK, TPS>>(c, grid, smem, s);
}

template <int CK, int TPS, class ARGS>
inline void dispatch_bm(int bm, const ARGS& c, dim3 grid, size_t smem, hipStream_t s) {
    if (bm == 128) launch_patch<128, CK, TPS>(c, grid, smem, s);
    else if (bm == 64) launch_patch<64, CK, TPS>(c, grid, smem, s);
    else if (bm == 32) launch_patch<32, CK, TPS>(c, grid, smem, s);
    else launch_patch<16, CK, TPS>(c, grid, smem, s);
}
template <class ARGS>
inline void dispatch_patch(int bm, int ck, int tps, const ARGS& c, dim3 grid, size_t smem, hipStream_t s) {
    if (tps == 3 && ck == 16) dispatch_bm<16, 3>(bm, c, grid, smem, s);
    else if (tps == 3) dispatch_bm<8, 3>(bm, c, grid, smem, s);
    else if (ck == 16) dispatch_bm<16, 1>(bm, c, grid, smem, s);
    else dispatch_bm<8, 1>(bm, c, grid, smem, s);
}

inline CP make_cp(const GG& g, const ConvPlan& p, const float* zeros, const float* wp, float* part) {
    CP c = {};
    c.x = g.x; c.wp = wp; c.zeros = zeros; c.bias = g.bias; c.res = g.res; c.y = g.y; c.part = part;
    c.B = g.B; c.Cin = g.Cin; c.IH = g.IH; c.IW = g.IW; c.x_bs = g.x_bs;
    c.M = g.M; c.Mpad = p.Mpad; c.Cpad = p.Cpad;
    c.Rt = g.Rt; c.St = g.St; c.si = g.si; c.dstep = g.dstep;
    c.dy_base = g.dy0 - p.ymin; c.dx_base = g.dx0 - p.xmin; c.ymin = p.ymin; c.xmin = p.xmin;
    c.PH = p.PH; c.PWr = p.PWr; c.PS = p.PS; c.tw16 = p.tw16; c.ipt = p.ipt; c.phi = p.phi; c.aligned = p.aligned; c.shift = p.shift;
    c.OHt = g.OHt; c.OWt = g.OWt; c.so = g.so; c.oy0 = g.oy0; c.ox0 = g.ox0; c.OH = g.OH; c.OW = g.OW;
    c.y_bs = g.y_bs; c.res_bs = g.res_bs;
    c.tiles_x = p.tiles_x; c.tiles_y = p.tiles_y;
    c.nsplit = p.nsplit; c.cps = p.cps;
    c.part_stride = (long)g.B * g.M * p.Hp * p.Wp;      // padded slabs
    c.act = g.act; c.act_a = g.act_a; c.act_b = g.act_b; c.res_mul = g.res_mul;
    c.add = g.add; c.add_bs = g.add_bs;
#ifndef CC_CONV_WMAJOR
#define CC_CONV_WMAJOR 1
#endif
    c.wmajor = (CC_CONV_WMAJOR && (long)g.M * g.Rt * g.St > (long)g.B * g.IH * g.IW) ? 1 : 0;      // weights M Cin T floats, input B Cin IH IW
    c.vec4 = (g.so == 1) && ((g.OW & 3) == 0) && ((g.ox0 & 3) == 0) && ((((uintptr_t)g.y) & 15) == 0) && ((g.y_bs & 3) == 0) &&
             (!g.res || ((((uintptr_t)g.res) & 15) == 0 && (g.res_bs & 3) == 0)) &&
             (!g.add || ((((uintptr_t)g.add) & 15) == 0 && (g.add_bs & 3) == 0));
    return c;
}

// ---- second stage of split-K.  The epilogue record of a problem whose partial slabs are at `part`; a class no tap reaches
// (g.Cin == 0) has no slabs: its result is the epilogue of zero (nsplit 0, dense rows)
inline EPC fill_epc(const GG& g, const ConvPlan& p, const float* part) {
    const bool empty = g.Cin == 0;
    EPC c = {};
    c.part = empty ? nullptr : part; c.bias = g.bias; c.res = g.res; c.add = g.add; c.y = g.y;
    c.Hp = empty ? g.OHt : p.Hp;
    c.Wp = empty ? g.OWt : p.Wp;
    c.part_stride = (long)g.B * g.M * c.Hp * c.Wp;
    c.nsplit = empty ? 0 : p.nsplit;
    c.OHt = g.OHt; c.OWt = g.OWt; c.oy0 = g.oy0; c.ox0 = g.ox0;
    c.total = (empty || p.nsplit > 1) ? (long)g.B * g.M * g.OHt * g.OWt : 0;
    c.M = g.M; c.so = g.so; c.OH = g.OH; c.OW = g.OW; c.y_bs = g.y_bs; c.res_bs = g.res_bs; c.add_bs = g.add_bs;
    c.act = g.act; c.act_a = g.act_a; c.act_b = g.act_b; c.res_mul = g.res_mul;
    return c;
}

// ... of ONE problem as a launch of its own (a split single-problem launch, or the epilogue of zero)
inline void launch_splitk_epilogue(const EPC& c, hipStream_t s) {
    hipLaunchKernelGGL(k_splitk_epilogue, dim3((unsigned)((c.total + 255) / 256)), dim3(256), 0, s, c.part, c.nsplit, c.part_stride, c.bias,
                       c.res, c.y, c.M, c.OHt, c.OWt, c.so, c.oy0, c.ox0, c.OH, c.OW, c.y_bs, c.res_bs, c.total, c.act, c.act_a, c.act_b,
                       c.res_mul, c.add, c.add_bs, c.Hp, c.Wp);
}

// ---- Winograd path (wino.hip): nprob same-shaped problems of geometry g[0] in one launch
inline ccint::WinoGeom wino_geom(const GG& g) {
    ccint::WinoGeom w = {};
    w.B = g.B; w.Cin = g.Cin; w.H = g.IH; w.W = g.IW; w.x_bs = g.x_bs; w.M = g.M; w.y_bs = g.y_bs; w.res_bs = g.res_bs; w.add_bs = g.add_bs;
    w.act = g.act; w.act_a = g.act_a; w.act_b = g.act_b; w.res_mul = g.res_mul;
    return w;
}

// MFMA FLOPs the Winograd kernel executes: 16 multiply-adds per 2x2 output tile and channel pair (the direct form: 36)
inline double wino_gflop(const GG& g, const ConvPlan& p) { return 2e-9 * 16.0 * g.B * p.wn.TY * p.wn.TX * (double)g.M * g.Cin; }

inline int wino_flip(const GG& g) { return g.dstep < 0 ? 1 : 0; }

// ---- 3x3 / stride-1 layers on maps whose width is not a multiple of 4 (8x26, 4x13: the deep levels): the Winograd weight-gradient
// kernel moves rows as 16-byte pieces, so dY and the input are first copied into rows padded with zeros to a multiple of 4 (zero
// dY columns add nothing, zero input columns are the convolution's own padding) -- two 1-2 MB copies in one launch against half
// the time of the im2col kernel on these 512-channel layers (profiles/r04_ab_round4.txt).
struct PadTab { ccint::PadJob j[2 * MAXGRP]; int n, B, W, Wp; long row_end[2 * MAXGRP]; };     // row_end: cumulative B * rows_per_image
__global__ __launch_bounds__(256) void k_pad_rows(PadTab t) {
    const int q4 = t.Wp >> 2;                                  // float4s per padded row
    const long e = (long)blockIdx.x * 256 + threadIdx.x;       // one float4 of one padded row
    const long row = e / q4;
    const int c4 = (int)(e - row * q4) * 4;
    int k = 0;
    long first = 0;
#pragma unroll
    for (int q = 0; q < 2 * MAXGRP - 1; q++)
        if (q + 1 < t.n && row >= t.row_end[q]) { k = q + 1; first = t.row_end[q]; }
    if (row >= t.row_end[t.n - 1]) return;
    const ccint::PadJob& j = t.j[k];
    const long r = row - first;
    const int n = (int)(r / j.rows_per_image);
    const long rr = r - (long)n * j.rows_per_image;
    const float* s = j.src + (long)n * j.bs + rr * t.W;
    float4 v;
    v.x = c4 + 0 < t.W ? s[c4 + 0] : 0.f;
    v.y = c4 + 1 < t.W ? s[c4 + 1] : 0.f;
    v.z = c4 + 2 < t.W ? s[c4 + 2] : 0.f;
    v.w = c4 + 3 < t.W ? s[c4 + 3] : 0.f;
    *reinterpret_cast<float4*>(j.dst + (r * t.Wp + c4)) = v;
}
}  // namespace

void ccint::pad_rows_launch(const PadJob* jobs, int n, int B, int W, int Wp, hipStream_t s) {
    PadTab t = {};
    t.n = n; t.B = B; t.W = W; t.Wp = Wp;
    long rows = 0;
    for (int k = 0; k < n; k++) {
        t.j[k] = jobs[k];
        rows += (long)B * jobs[k].rows_per_image;
        t.row_end[k] = rows;
    }
    const long nf4 = rows * (Wp >> 2);
    hipLaunchKernelGGL(k_pad_rows, dim3((unsigned)((nf4 + 255) / 256)), dim3(256), 0, s, t);
}

namespace {

// n problems in ONE conv launch (+ ONE split-K epilogue launch): the parity classes of a stride-2 data-gradient, the
// same-shaped convolutions of parallel branches, and (round 3, cc_conv2d_list) independent layers of DIFFERENT networks --
// every class carries its own geometry, channel count and epilogue; what the classes of a launch share is the tile
// configuration (BM, CK) of the kernel instance.  Needs prepacked weight images.  zeros / wp / part: the 64-float zero block,
// weight image and partial-slab area of the class.
struct ClsIn { GG g; ConvPlan p; const float* zeros; const float* wp; float* part; };

// Winograd over zero-padded copies of the inputs (ConvPlan::wpad) of n same-shaped problems: each copy goes behind its problem's
// partial slabs (rows of wpad floats, dense [B][Cin][H][wpad]), 2 * MAXGRP jobs per copy launch; pr / wg are re-pointed at them
inline void wino_pad_inputs(const ClsIn* cs, int n, hipStream_t s, ccint::WinoProb* pr, ccint::WinoGeom& wg) {
    const GG& g0 = cs[0].g;
    const ConvPlan& p = cs[0].p;
    for (int k0 = 0; k0 < n; k0 += 2 * MAXGRP) {
        ccint::PadJob jobs[2 * MAXGRP];
        int nj = 0;
        for (int k = k0; k < n && k < k0 + 2 * MAXGRP; k++) {
            float* xpad = cs[k].part + p.part_floats;
            jobs[nj++] = ccint::PadJob{cs[k].g.x, xpad, cs[k].g.x_bs, g0.Cin * g0.IH};
            pr[k].x = xpad;
        }
        ccint::pad_rows_launch(jobs, nj, g0.B, g0.IW, p.wpad, s);
    }
    wg.W = p.wpad;
    wg.x_bs = (long)g0.Cin * g0.IH * p.wpad;
    if (cctools::env_flag("CC_WINO_TRACE"))
        fprintf(stderr, "wino padded input, %d problems: B%d M%d C%d %dx%d -> pitch %d, nsplit %d dstep %d\n", n, g0.B, g0.M, g0.Cin, g0.IH,
                g0.IW, p.wpad, p.nsplit, g0.dstep);
}

// A 3x3 / stride-1 / pad-1 problem with <= 4 channels on one side (a prediction head or its data-gradient, a layer with <= 4 inputs)
// as the conv_heads.hip description: 1 = few reduction channels (k_conv_thinc), 2 = few output channels (k_conv_thinm), 0 = neither
inline int head_kernel_of(const GG& g, ccint::HeadConv& h) {
    static const int off = cctools::env_int("CC_NO_HEAD_KERNELS", 0);       // tools: 1 = none, 2 = no thinm, 3 = no thinc
    if (off == 1 || (g.Cin > 4 && g.M > 4) || g.Cin < 1 || g.Rt != 3 || g.St != 3 || g.si != 1 || g.so != 1 || g.oy0 != 0 || g.ox0 != 0) return 0;
    if (g.OHt != g.OH || g.OWt != g.OW || g.OH != g.IH || g.OW != g.IW || g.w_ri != 3 || g.w_sj != 1) return 0;
    if (!((g.dstep == 1 && g.dy0 == -1 && g.dx0 == -1) || (g.dstep == -1 && g.dy0 == 1 && g.dx0 == 1))) return 0;
    if (g.res_mul && !g.res) return 0;
    h = ccint::HeadConv{g.x, g.w, g.bias, g.res, g.res_mul ? g.add : nullptr, g.y, g.B, g.Cin, g.IH, g.IW, g.M, g.x_bs, g.y_bs, g.res_bs,
                        g.add_bs, g.w_sm, g.w_sc, (long)g.w0, g.dstep, g.act, g.act_a, g.act_b, g.res_mul};
    if (g.Cin <= 4 && off != 3 && ccint::head_conv_thinc_vec(h) != 0) return 1;
    if (g.M <= 4 && off != 2 && ccint::head_conv_thinm_ok(h)) return 2;
    return 0;
}

// What launch_classes does with a list of classes, decided without launching anything (the launch and the name query read it)
struct ClassForm {
    bool ok;                   // false: the classes do not share a launch (the caller launches them one by one)
    bool wino;                 // all of them Winograd problems of one shape: one wino.hip launch
    int ref;                   // first class with taps: its (bm, ck) are the kernel instance's (-1: no class has taps)
    int tps, maxy, maxsplit;   // launch-wide: taps per stage, grid y / z (the maxima over the classes)
    int nc;                    // classes of the conv launch (those with taps)
    bool stk;                  // the stacked instance (a class stacks tiny maps)
    bool epi;                  // an epilogue launch follows: a class is split, or no tap reaches it
    size_t smem;
};

// ---- kernel names: the strings the timing scopes record (bench.py groups its timings by them, profiles/ is compared across rounds
// by them) and the cc_conv2d_*_kernel queries answer, formatted HERE only.  hk: the head kernel of head_kernel_of (0: none);
// f: the merged form whose reference class (g, p) is (nullptr: a launch of its own)
inline int kernel_name(int hk, const GG& g, const ConvPlan& p, const ClassForm* f, char* nm, int cap) {
    const int split = p.nsplit > 1 ? 1 : 0;
    if (hk) return snprintf(nm, cap, hk == 1 ? "k_conv_thinc<%d>" : "k_conv_thinm<%d>", hk == 1 ? g.Cin : g.M);
    if (f && !f->wino && f->nc == 0) return snprintf(nm, cap, "k_splitk_epilogue_multi");      // no class has taps: the epilogue is all there is
    if (g.Cin == 0) return snprintf(nm, cap, "k_splitk_epilogue");                             // a class no tap reaches, on its own
    if (!p.use_patch) return snprintf(nm, cap, "k_gather_gemm<%d>", pick_bm(g.M));
    if (p.wino) return p.wn.tile ? snprintf(nm, cap, "k_wino_f2x3_s<%d, %d>", p.wn.tile, split) : snprintf(nm, cap, "k_wino_f2x3<%d>", split);
    if (f) return f->stk ? snprintf(nm, cap, "k_conv_patch_multi_stk<%d, %d>", p.bm, f->tps)
                         : snprintf(nm, cap, "k_conv_patch_multi<%d, %d, %d>", p.bm, p.ck, f->tps);
    return p.ipt > 1 ? snprintf(nm, cap, "k_conv_patch_stk<%d, %d, %d>", p.bm, p.tps, split)
                     : snprintf(nm, cap, "k_conv_patch<%d, %d, %d, %d>", p.bm, p.ck, p.tps, split);
}

// scope name of a Winograd launch of nprob problems of geometry g
inline void wino_scope_name(const GG& g, const ConvPlan& p, int nprob, char* nm, int cap) {
    const int nl = kernel_name(0, g, p, nullptr, nm, cap);
    if (cctools::env_flag("CC_TIMING_DETAIL"))
        snprintf(nm + nl, cap - nl, " %dx[B%d M%d C%d %dx%d%s t9 k%d] wg%d", nprob, g.B, g.M, g.Cin, g.OH, g.OW, p.wpad ? "(pad)" : "", p.nsplit,
                 nprob * p.wn.nqb * p.wn.nmb * p.nsplit);
}

// ws: the problem's workspace area (ws_image / ws_slabs), sized by conv_ws_floats(plan_conv(g)); plan: plan_conv(g) where the caller has
// it; prepacked (optional): weight image produced earlier by k_repack_table, pre_zeros its 64 zeros -> no repack launch here
inline void launch_gg(const GG& g, float* ws, hipStream_t s, const float* prepacked = nullptr, const float* pre_zeros = nullptr,
                      const ConvPlan* plan = nullptr) {
    ccint::HeadConv h;
    const int hk = head_kernel_of(g, h);
    if (hk) {
        char nm[96];
        const int nl = kernel_name(hk, g, ConvPlan(), nullptr, nm, sizeof nm);
        if (cctools::env_flag("CC_TIMING_DETAIL"))
            snprintf(nm + nl, sizeof nm - nl, " B%d M%d C%d %dx%d t9", g.B, g.M, g.Cin, g.OHt, g.OWt);
        cctiming::Scope tsc(nm, 2e-9 * g.B * g.OHt * g.OWt * (double)g.M * g.Cin * 9, s);
        if (cctools::env_flag("CC_HEAD_TRACE"))
            fprintf(stderr, "head kernel %d: B%d M%d C%d %dx%d dstep %d\n", hk, g.B, g.M, g.Cin, g.OHt, g.OWt, g.dstep);
        if (hk == 1 ? ccint::head_conv_thinc_launch(h, s) : ccint::head_conv_thinm_launch(h, s)) return;
    }
    const ConvPlan p = plan ? *plan : plan_conv(g);
    if (!p.use_patch || ws == nullptr) { launch_gg_flat(g, s); return; }
    float* part = ws_slabs(ws, prepacked ? 0 : p.wp_floats);
    char nm[128];
    if (p.wino) {
        if (!prepacked)
            ccint::wino_weights_launch(g.w, ws_image(ws), g.M, g.Cin, p.Cpad, p.Mpad, g.w_sm, g.w_sc, g.w0, g.w_ri, g.w_sj, wino_flip(g), s);
        ccint::WinoProb pr = {g.x, prepacked ? prepacked : ws_image(ws), g.bias, g.res, g.add, g.y, part};
        ccint::WinoGeom wg = wino_geom(g);
        const ClsIn one = {g, p, nullptr, pr.U, part};
        if (p.wpad) wino_pad_inputs(&one, 1, s, &pr, wg);
        bool ok;
        {
            wino_scope_name(g, p, 1, nm, sizeof nm);
            cctiming::Scope tsc(nm, wino_gflop(g, p), s);
            ok = ccint::wino_launch(wg, p.wn, &pr, 1, s);
        }
        if (!ok) { launch_gg_flat(g, s); return; }      // x not 16-byte aligned (an odd view): the gather kernel reads the weights as they lie
        if (p.nsplit > 1) launch_splitk_epilogue(fill_epc(g, p, part), s);
        return;
    }
    const float* zeros = prepacked ? pre_zeros : ws;
    const float* wp = prepacked ? prepacked : ws_image(ws);
    if (!prepacked)
        hipLaunchKernelGGL(k_repack_w, dim3((unsigned)((p.wp_floats + 255) / 256)), dim3(256), 0, s, g.w, ws_image(ws), ws, g.M, g.Cin,
                           p.Mpad, p.Cpad, g.Rt * g.St, g.St, g.w_sm, g.w_sc, g.w0, g.w_ri, g.w_sj);
    const CP c = make_cp(g, p, zeros, wp, part);
    dim3 grid((unsigned)conv_tiles(g, p), (unsigned)(p.Mpad / p.bm), (unsigned)p.nsplit);
    {
        const int nl = kernel_name(0, g, p, nullptr, nm, sizeof nm);
        if (cctools::env_flag("CC_TIMING_DETAIL"))
            snprintf(nm + nl, sizeof nm - nl, " B%d M%d C%d %dx%d t%d k%d wg%d", g.B, g.M, g.Cin, g.OHt, g.OWt, g.Rt * g.St, p.nsplit,
                     (int)(grid.x * grid.y * grid.z));
        cctiming::Scope tsc(nm, 2e-9 * g.B * g.OHt * g.OWt * (double)g.M * g.Cin * g.Rt * g.St, s);
        dispatch_patch(p.bm, p.ck, p.tps, c, grid, p.smem, s);
    }
    if (p.nsplit > 1) launch_splitk_epilogue(fill_epc(g, p, part), s);
}

// same geometry and epilogue form (the Winograd launch shares them between its problems)
inline bool same_problem_shape(const GG& a, const GG& b) {
    return a.B == b.B && a.Cin == b.Cin && a.IH == b.IH && a.IW == b.IW && a.x_bs == b.x_bs && a.M == b.M && a.y_bs == b.y_bs &&
           a.res_bs == b.res_bs && a.add_bs == b.add_bs && a.act == b.act && a.act_a == b.act_a && a.act_b == b.act_b &&
           a.res_mul == b.res_mul && a.dstep == b.dstep;
}

inline ClassForm classes_form(const ClsIn* cs, int n, bool idle_taps) {
    ClassForm f = {};
    f.ref = -1;
    if (n < 1 || n > MAXCLS) return f;
    // Winograd problems: all of the launch or none (a mixed list goes back to the caller, which launches one by one)
    int nw = 0;
    for (int k = 0; k < n; k++) nw += cs[k].p.wino ? 1 : 0;
    if (nw) {
        if (nw != n) return f;
        const ConvPlan& p = cs[0].p;
        for (int k = 0; k < n; k++) {
            const GG& g = cs[k].g;
            if (!cs[k].wp || !same_problem_shape(g, cs[0].g) || cs[k].p.nsplit != p.nsplit || cs[k].p.cps != p.cps) {
                if (cctools::env_flag("CC_WINO_TRACE"))
                    fprintf(stderr, "wino classes declined: k %d wp %p same %d nsplit %d/%d cps %d/%d\n", k, (const void*)cs[k].wp,
                            (int)same_problem_shape(g, cs[0].g), cs[k].p.nsplit, p.nsplit, cs[k].p.cps, p.cps);
                return f;
            }
            // zero-padded input copies (same shape: same plan) live behind each problem's slabs
            if (p.wpad && (cs[k].p.wpad != p.wpad || cs[k].p.part_floats != p.part_floats || !cs[k].part)) return f;
        }
        f.ok = f.wino = true;
        f.nc = n; f.maxsplit = p.nsplit; f.epi = p.nsplit > 1;
        return f;
    }
    f.tps = 3; f.maxsplit = 1; f.maxy = 1;
    if (cctools::env_int("CC_CONV_IDLE_TAPS", 1)) idle_taps = true;
    for (int k = 0; k < n; k++) {
        const ConvPlan& p = cs[k].p;
        // a class no tap reaches (the odd output parities of a 1x1 stride-2 data-gradient: DispResNet6's shortcut convolutions):
        // its result is the epilogue of zero -- it takes no workgroup of the conv launch, only a slot of the epilogue launch
        if (cs[k].g.Cin == 0) { f.epi = true; continue; }
        if (f.ref < 0) f.ref = k;
        if (!p.use_patch || p.bm != cs[f.ref].p.bm || p.ck != cs[f.ref].p.ck || !cs[k].wp) return f;
        // three taps per stage launch-wide unless a class's patch does not leave room (a class with fewer taps idles the slots)
        if (p.tps != 3 && !(idle_taps && cs[k].g.Rt * cs[k].g.St < 3 && patch_smem(p, 3) <= 80 * 1024)) f.tps = 1;
        if (p.nsplit > f.maxsplit) f.maxsplit = p.nsplit;
        if (p.Mpad / p.bm > f.maxy) f.maxy = p.Mpad / p.bm;
        if (p.nsplit > 1) f.epi = true;
        if (p.ipt > 1) f.stk = true;
        f.nc++;
    }
    for (int k = 0; k < n; k++) {
        if (cs[k].g.Cin == 0) continue;
        const size_t sm = patch_smem(cs[k].p, f.tps);          // A buffers follow the launch-wide TPS, the patch buffers this class's PS
        if (sm > f.smem) f.smem = sm;
    }
    f.ok = f.smem <= 80 * 1024;
    return f;
}

inline bool launch_wino_classes(const ClsIn* cs, int n, hipStream_t s) {
    ccint::WinoProb pr[MAXCLS];
    EPM e = {};
    e.n = n;
    int ebx = 0;
    const ConvPlan& p = cs[0].p;
    for (int k = 0; k < n; k++) {
        const GG& g = cs[k].g;
        pr[k] = ccint::WinoProb{g.x, cs[k].wp, g.bias, g.res, g.add, g.y, cs[k].part};
        e.c[k] = fill_epc(g, p, cs[k].part);
        ebx += (int)((e.c[k].total + 255) / 256);
        e.bx_end[k] = ebx;
    }
    ccint::WinoGeom wg = wino_geom(cs[0].g);
    if (p.wpad) wino_pad_inputs(cs, n, s, pr, wg);
    {
        char nm[128];
        wino_scope_name(cs[0].g, p, n, nm, sizeof nm);
        cctiming::Scope tsc(nm, n * wino_gflop(cs[0].g, p), s);
        if (!ccint::wino_launch(wg, p.wn, pr, n, s)) return false;
    }
    if (p.nsplit > 1) hipLaunchKernelGGL(k_splitk_epilogue_multi, dim3((unsigned)ebx), dim3(256), 0, s, e);
    return true;
}

inline bool launch_classes(const ClsIn* cs, int n, const ClassForm& f, hipStream_t s) {
    if (!f.ok) return false;
    if (f.wino) return launch_wino_classes(cs, n, s);
    CPM a = {};        // ~3 KB + ~1.5 KB of host stack, passed to the launches by value
    EPM e = {};
    e.n = n;
    int bx = 0, ebx = 0, nc = 0;
    double gf = 0, wf = 0, xf = 0;
    for (int k = 0; k < n; k++) {
        const GG& g = cs[k].g;
        const ConvPlan& p = cs[k].p;
        e.c[k] = fill_epc(g, p, cs[k].part);
        ebx += (int)((e.c[k].total + 255) / 256);
        e.bx_end[k] = ebx;
        if (g.Cin == 0) continue;
        a.c[nc] = make_cp(g, p, cs[k].zeros, cs[k].wp, cs[k].part);
        bx += (int)conv_tiles(g, p);
        a.bx_end[nc] = bx;
        nc++;
        gf += 2e-9 * g.B * g.OHt * g.OWt * (double)g.M * g.Cin * g.Rt * g.St;
        wf += (double)g.M * g.Cin * g.Rt * g.St;
        xf += (double)g.B * g.Cin * g.IH * g.IW;
    }
    a.n = nc;
    a.wmajor = (CC_CONV_WMAJOR && wf > xf) ? 1 : 0;      // launch-wide XCD order: weight-major when the classes' weights outweigh their inputs
    if (nc > 0) {
        dim3 grid((unsigned)bx, (unsigned)f.maxy, (unsigned)f.maxsplit);
        char nm[224];
        int nl = kernel_name(0, cs[f.ref].g, cs[f.ref].p, &f, nm, sizeof nm);
        if (cctools::env_flag("CC_TIMING_DETAIL")) {
            // classes with the same geometry are counted, not repeated
            for (int k = 0; k < n && nl < (int)sizeof nm - 48; k++) {
                const GG& g = cs[k].g;
                if (g.Cin == 0) continue;
                int same = 0, first = 1;
                for (int j = 0; j < n; j++) {
                    const GG& h = cs[j].g;
                    const bool eq = h.Cin == g.Cin && h.M == g.M && h.OHt == g.OHt && h.OWt == g.OWt && h.Rt * h.St == g.Rt * g.St &&
                                    cs[j].p.nsplit == cs[k].p.nsplit;
                    if (eq) { same++; if (j < k) first = 0; }
                }
                if (!first) continue;
                nl += snprintf(nm + nl, sizeof nm - nl, " %dx[B%d M%d C%d %dx%d t%d k%d]", same, g.B, g.M, g.Cin, g.OHt, g.OWt,
                               g.Rt * g.St, cs[k].p.nsplit);
            }
            snprintf(nm + nl, sizeof nm - nl, " wg%d", (int)(grid.x * grid.y * grid.z));
        }
        cctiming::Scope tsc(nm, gf, s);
        dispatch_patch(cs[f.ref].p.bm, cs[f.ref].p.ck, f.tps, a, grid, f.smem, s);
    }
    if (f.epi) hipLaunchKernelGGL(k_splitk_epilogue_multi, dim3((unsigned)ebx), dim3(256), 0, s, e);
    return true;
}

inline bool launch_classes(const ClsIn* cs, int n, hipStream_t s, bool idle_taps = false) {
    return launch_classes(cs, n, classes_form(cs, n, idle_taps), s);
}

// ---- the transposed arithmetic and its parity classes
/* Transposed-convolution arithmetic  gx[n, c, iy, ix] = sum_{k,r,s} wT(k,c,r,s) * gy[n, k, oy, ox],  iy = oy*stride - pad + r: the
 * data-gradient of conv2d and the forward of ConvTranspose2d (include/ccengine.h: cc_conv2d_dgrad, cc_conv2d_dgrad_group[_add]),
 * one output parity class at a time so that no structurally-zero tap is multiplied.  gy: [B,K,OH,OW]; gx: [B,C,IH,IW]. */
struct TProblem {
    const float* gy; const float* w; const float* bias; float* gx; const float* mul; const float* add;
    int B, K, OH, OW; long gy_bs;
    int C, R, S, stride, pad, IH, IW; long gx_bs, mul_bs, add_bs;
    long w_k_stride, w_c_stride;
    int act; float act_a, act_b;
};

// a transposed problem without its operands; the host-only queries plan with the geometry alone
inline TProblem tr_problem(int B, int K, int OH, int OW, int C, int R, int S, int stride, int pad, int IH, int IW, long w_k_stride,
                           long w_c_stride, long gy_bs = 0, long gx_bs = 0, long mul_bs = 0, long add_bs = 0, int act = 0, float act_a = 1.f,
                           float act_b = 0.f) {
    TProblem t = {};
    t.B = B; t.K = K; t.OH = OH; t.OW = OW; t.C = C; t.R = R; t.S = S; t.stride = stride; t.pad = pad; t.IH = IH; t.IW = IW;
    t.w_k_stride = w_k_stride; t.w_c_stride = w_c_stride;
    t.gy_bs = gy_bs; t.gx_bs = gx_bs; t.mul_bs = mul_bs; t.add_bs = add_bs;
    t.act = act; t.act_a = act_a; t.act_b = act_b;
    return t;
}

// output parity class (py, px) of t as a gather-GEMM problem; false: the class has no output pixel
inline bool make_dgrad_class(GG& g, const TProblem& t, int py, int px) {
    const int stride = t.stride, pad = t.pad, R = t.R, S = t.S;
    // taps r with (py + pad - r) % stride == 0, r ascending: r = r0 + stride*i
    const int r0 = (py + pad) % stride, s0 = (px + pad) % stride;
    const int Rt = (r0 < R) ? (R - r0 + stride - 1) / stride : 0;
    const int St = (s0 < S) ? (S - s0 + stride - 1) / stride : 0;
    const int OHt = (t.IH - py + stride - 1) / stride, OWt = (t.IW - px + stride - 1) / stride;
    if (OHt <= 0 || OWt <= 0) return false;
    g = GG();
    g.x = t.gy; g.w = t.w; g.bias = t.bias; g.y = t.gx;
    g.res = t.mul; g.res_bs = t.mul_bs; g.res_mul = t.mul ? 1 : 0;
    if (t.add) {        // the epilogue's `add` operand exists next to mul only; alone it is a plain residual: gx = act(sum + add)
        if (t.mul) { g.add = t.add; g.add_bs = t.add_bs; }
        else { g.res = t.add; g.res_bs = t.add_bs; g.res_mul = 0; }
    }
    g.B = t.B; g.Cin = t.K; g.IH = t.OH; g.IW = t.OW; g.x_bs = t.gy_bs;
    g.M = t.C; g.w_sm = t.w_c_stride; g.w_sc = t.w_k_stride;
    g.w0 = r0 * S + s0; g.w_ri = stride * S; g.w_sj = stride;
    g.Rt = Rt > 0 ? Rt : 1; g.St = St > 0 ? St : 1;
    // oy = (iy + pad - r)/stride with iy = py + stride*ty, r = r0 + stride*i  ->  oy = ty + (py + pad - r0)/stride - i
    g.dy0 = (py + pad - r0) / stride; g.dx0 = (px + pad - s0) / stride; g.dstep = -1; g.si = 1;
    if (Rt == 0 || St == 0) g.Cin = 0;   // no tap reaches this parity class: output = act(bias)
    g.OHt = OHt; g.OWt = OWt; g.so = stride; g.oy0 = py; g.ox0 = px; g.OH = t.IH; g.OW = t.IW; g.y_bs = t.gx_bs;
    g.act = t.act; g.act_a = t.act_a; g.act_b = t.act_b;
    return true;
}

// The parity classes of a transposed problem, in the order every caller walks them (py, then px), with the plan for `mult` problems
// per launch.  Two rules every caller keeps:
//   * a class no tap reaches (g.Cin == 0: the odd parities of a 1x1 stride 2) takes no weight image and no slabs, but it is a class
//     of the problem: it is counted, and its result is the epilogue of zero;
//   * a class without output pixels (`lattice` false: IH or IW smaller than the stride) is skipped -- except by the merged launch,
//     which declines: its class list is the stride^2 classes of every problem.
struct TClass {
    GG g; ConvPlan p;
    bool lattice;              // the class has output pixels (g / p are valid)
    long img_off;              // its weight image inside the problem's prepacked image, floats (the 64 zeros come first)
    long slab_off;             // its partial slabs (+ padded input copy) inside the problem's slab area when all classes are live at once
};
template <class F>             // f(const TClass&) -> bool: false stops the walk (and is what for_each_class returns)
inline bool for_each_class(const TProblem& t, int mult, F&& f) {
    TClass c = {};
    c.img_off = 64;
    for (int py = 0; py < t.stride; py++)
        for (int px = 0; px < t.stride; px++) {
            c.lattice = make_dgrad_class(c.g, t, py, px);
            if (c.lattice) c.p = plan_conv(c.g, mult);
            if (!f(c)) return false;
            if (c.lattice) {
                c.img_off += (long)c.p.wp_floats;
                c.slab_off += (long)(c.p.part_floats + c.p.pad_floats);
            }
        }
    return true;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" {

static GG make_fwd(const float* x, const float* w, const float* bias, const float* res, float* y, int B, int Cin, int IH,
                   int IW, long x_bs, int Cout, int R, int S, int stride, int pad, int OH, int OW, long y_bs, long res_bs,
                   int act, float act_a, float act_b) {
    GG g = {};
    g.x = x; g.w = w; g.bias = bias; g.res = res; g.y = y;
    g.B = B; g.Cin = Cin; g.IH = IH; g.IW = IW; g.x_bs = x_bs;
    g.M = Cout; g.w_sm = (long)Cin * R * S; g.w_sc = (long)R * S; g.w0 = 0; g.w_ri = S; g.w_sj = 1;
    g.Rt = R; g.St = S; g.dy0 = -pad; g.dx0 = -pad; g.dstep = 1; g.si = stride;
    g.OHt = OH; g.OWt = OW; g.so = 1; g.oy0 = 0; g.ox0 = 0; g.OH = OH; g.OW = OW; g.y_bs = y_bs; g.res_bs = res_bs;
    g.act = act; g.act_a = act_a; g.act_b = act_b;
    return g;
}

// the geometry of a forward problem (what the host-only queries plan with)
static GG fwd_shape(int B, int Cin, int IH, int IW, int Cout, int R, int S, int stride, int pad, int OH, int OW) {
    return make_fwd(nullptr, nullptr, nullptr, nullptr, nullptr, B, Cin, IH, IW, 0, Cout, R, S, stride, pad, OH, OW, 0, 0, 0, 1.f, 0.f);
}

static void fill_desc(const GG& g, const ConvPlan& p, long src, long dst, long* d) {
    d[0] = src; d[1] = dst; d[2] = g.M; d[3] = g.Cin; d[4] = p.Mpad; d[5] = p.Cpad; d[6] = (long)g.Rt * g.St; d[7] = g.St;
    d[8] = g.w_sm; d[9] = g.w_sc; d[10] = g.w0; d[11] = g.w_ri; d[12] = g.w_sj; d[13] = (long)p.wp_floats; d[14] = 0;
    d[15] = repack_blocks(p.Mpad, p.Cpad, g.Rt * g.St);
    if (p.wino) {        // U = G g G^T (wino_weights.h); d[6] marks the descriptor, the sign of d[7] the tap direction
        d[6] = ccwino::WINO_T; d[7] = wino_flip(g) ? -3 : 3;
        d[15] = ccwino::wino_weight_blocks(p.Mpad, p.Cpad);
    }
}

/* Per-step weight prepack (include/ccengine.h): an image is [64 zeros][tap][c][m], for dgrad one [tap][c][m] per parity class with taps */
size_t cc_conv2d_fwd_pack_floats(int B, int Cin, int IH, int IW, int Cout, int R, int S, int stride, int pad, int OH, int OW) {
    const ConvPlan p = plan_conv(fwd_shape(B, Cin, IH, IW, Cout, R, S, stride, pad, OH, OW));
    return (p.use_patch && R * S <= 136) ? 64 + p.wp_floats : 0;      // 136 = tile rows of k_repack_table
}

int cc_conv2d_fwd_pack_desc(int B, int Cin, int IH, int IW, int Cout, int R, int S, int stride, int pad, int OH, int OW,
                            long src_ptr, long pack_base_ptr, long* desc_out_host) {
    const GG g = fwd_shape(B, Cin, IH, IW, Cout, R, S, stride, pad, OH, OW);
    const ConvPlan p = plan_conv(g);
    if (!p.use_patch) return 0;
    fill_desc(g, p, src_ptr, pack_base_ptr + 64 * (long)sizeof(float), desc_out_host);
    return 1;
}

size_t cc_conv2d_fwd_ws_bytes(int B, int Cin, int IH, int IW, int Cout, int R, int S, int stride, int pad, int OH, int OW) {
    return conv_ws_floats(plan_conv(fwd_shape(B, Cin, IH, IW, Cout, R, S, stride, pad, OH, OW))) * sizeof(float);
}

int cc_conv2d_fwd(const float* x, const float* w, const float* bias_or_null, const float* res_or_null, float* y, float* ws,
                  const float* prepacked_or_null, int B, int Cin, int IH, int IW, long x_bs, int Cout, int R, int S, int stride,
                  int pad, int OH, int OW, long y_bs, long res_bs, int act, float act_a, float act_b, void* stream) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || R <= 0 || S <= 0 || stride <= 0) return CC_ERR_ARG;
    GG g = make_fwd(x, w, bias_or_null, res_or_null, y, B, Cin, IH, IW, x_bs, Cout, R, S, stride, pad, OH, OW, y_bs, res_bs,
                    act, act_a, act_b);
    launch_gg(g, ws, (hipStream_t)stream, prepacked_or_null ? ws_image(prepacked_or_null) : nullptr, prepacked_or_null);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

/* G same-shaped convolutions (parallel branches of a network) in one launch; ws: G consecutive areas of *_group_ws_bytes / G */
size_t cc_conv2d_fwd_group_ws_bytes(int G, int B, int Cin, int IH, int IW, int Cout, int R, int S, int stride, int pad, int OH,
                                    int OW) {
    const GG g = fwd_shape(B, Cin, IH, IW, Cout, R, S, stride, pad, OH, OW);
    const size_t a = conv_ws_floats(plan_conv(g, G)), b = conv_ws_floats(plan_conv(g));
    return (size_t)G * (a > b ? a : b) * sizeof(float);
}

int cc_conv2d_fwd_group(int G, const long* x, const long* w, const long* bias, const long* res, const long* y, float* ws,
                        const long* prepacked, int B, int Cin, int IH, int IW, long x_bs, int Cout, int R, int S, int stride,
                        int pad, int OH, int OW, long y_bs, long res_bs, int act, float act_a, float act_b, void* stream) {
    if (G <= 0 || G > MAXCLS || B <= 0 || Cin <= 0 || Cout <= 0 || R <= 0 || S <= 0 || stride <= 0) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t stride_f = cc_conv2d_fwd_group_ws_bytes(G, B, Cin, IH, IW, Cout, R, S, stride, pad, OH, OW) / sizeof(float) / G;
    ClsIn cs[MAXCLS];
    bool packed = true;
    for (int k = 0; k < G; k++) {
        cs[k].g = make_fwd((const float*)x[k], (const float*)w[k], bias ? (const float*)bias[k] : nullptr,
                           res ? (const float*)res[k] : nullptr, (float*)y[k], B, Cin, IH, IW, x_bs, Cout, R, S, stride, pad, OH,
                           OW, y_bs, res_bs, act, act_a, act_b);
        const float* pk = prepacked ? (const float*)prepacked[k] : nullptr;
        if (!pk) packed = false;
        cs[k].zeros = pk;
        cs[k].wp = pk ? ws_image(pk) : nullptr;
        cs[k].part = ws_slabs(ws + k * stride_f, 0);
    }
    // one launch for the group (split-K planned for all of it), or one problem after the other
    bool merged = false;
    if (G > 1 && packed && ws && !cctools::env_flag("CC_NO_CLASS_MERGE")) {
        for (int k = 0; k < G; k++) cs[k].p = plan_conv(cs[k].g, G);
        merged = launch_classes(cs, G, s);
    }
    if (!merged)
        for (int k = 0; k < G; k++) launch_gg(cs[k].g, ws ? ws + k * stride_f : nullptr, s, cs[k].wp, cs[k].zeros);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

size_t cc_conv2d_dgrad_pack_floats(int B, int K, int OH, int OW, int C, int R, int S, int stride, int pad, int IH, int IW,
                                   long w_k_stride, long w_c_stride) {
    if (R * S > 136) return 0;
    size_t tot = 64;
    const bool ok = for_each_class(tr_problem(B, K, OH, OW, C, R, S, stride, pad, IH, IW, w_k_stride, w_c_stride), 1, [&](const TClass& c) {
        if (!c.lattice || c.g.Cin == 0) return true;
        if (!c.p.use_patch) return false;
        tot += c.p.wp_floats;
        return true;
    });
    return ok ? tot : 0;
}

int cc_conv2d_dgrad_pack_desc(int B, int K, int OH, int OW, int C, int R, int S, int stride, int pad, int IH, int IW,
                              long w_k_stride, long w_c_stride, long src_ptr, long pack_base_ptr, long* desc_out_host) {
    int n = 0;
    const bool ok = for_each_class(tr_problem(B, K, OH, OW, C, R, S, stride, pad, IH, IW, w_k_stride, w_c_stride), 1, [&](const TClass& c) {
        if (!c.lattice || c.g.Cin == 0) return true;
        if (!c.p.use_patch) return false;
        fill_desc(c.g, c.p, src_ptr, pack_base_ptr + c.img_off * (long)sizeof(float), desc_out_host + 16 * n++);
        return true;
    });
    return ok ? n : 0;
}

int cc_repack_table(const long* table_dev, int ndesc, long total_blocks, void* stream) {
    if (ndesc <= 0 || total_blocks <= 0) return CC_ERR_ARG;
    hipLaunchKernelGGL(k_repack_table, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, ndesc);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

size_t cc_conv2d_dgrad_group_ws_bytes(int G, int B, int K, int OH, int OW, int C, int R, int S, int stride, int pad, int IH, int IW) {
    const TProblem t = tr_problem(B, K, OH, OW, C, R, S, stride, pad, IH, IW, (long)C * R * S, (long)R * S);
    size_t best = 0;
    for (int mult = 1; mult <= G; mult += (G > 1 ? G - 1 : 1)) {
        size_t wmax = 0, psum = 0;        // the merged launch keeps every class's partial slabs alive at once
        for_each_class(t, mult, [&](const TClass& c) {
            if (!c.lattice) return true;
            if (c.p.wp_floats > wmax) wmax = c.p.wp_floats;
            psum += c.p.part_floats + c.p.pad_floats;
            return true;
        });
        const size_t tot = 64 + wmax + psum;
        if (tot > best) best = tot;
    }
    return (size_t)G * best * sizeof(float);
}

size_t cc_conv2d_dgrad_ws_bytes(int B, int K, int OH, int OW, int C, int R, int S, int stride, int pad, int IH, int IW) {
    return cc_conv2d_dgrad_group_ws_bytes(1, B, K, OH, OW, C, R, S, stride, pad, IH, IW);
}

// The merged form of a call: every parity class of its G problems in ONE launch (launch_classes).  -> the number of classes put
// into cs (and their launch form in f), or 0: the call runs class by class.  Merged when every problem brings a prepacked image
// (pk) and a workspace, there are 2 .. MAXCLS classes, each with output pixels, and launch_classes takes them.
// ws: G consecutive areas of stride_f floats.
static int dgrad_merged(const TProblem* ts, int G, const float* const* pk, float* ws, size_t stride_f, ClsIn* cs, ClassForm& f) {
    const int ncls = ts[0].stride * ts[0].stride;
    if (!ws || G * ncls < 2 || G * ncls > MAXCLS || cctools::env_flag("CC_NO_CLASS_MERGE")) return 0;
    int n = 0;
    for (int k = 0; k < G; k++) {
        if (!pk[k]) return 0;
        float* slabs = ws_slabs(ws + k * stride_f, 0);
        const bool all = for_each_class(ts[k], G, [&](const TClass& c) {
            if (!c.lattice) return false;
            cs[n++] = ClsIn{c.g, c.p, pk[k], pk[k] + c.img_off, slabs + c.slab_off};
            return true;
        });
        if (!all) return 0;
    }
    f = classes_form(cs, n, false);
    return f.ok ? n : 0;
}

static int dgrad_group_impl(int G, const long* gy, const long* w, const long* bias, const long* gx, const long* mul,
                            const long* add, float* ws, const long* prepacked, TProblem t, void* stream) {
    if (G <= 0 || G > MAXCLS || t.B <= 0 || t.K <= 0 || t.C <= 0 || t.stride <= 0) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t stride_f = cc_conv2d_dgrad_group_ws_bytes(G, t.B, t.K, t.OH, t.OW, t.C, t.R, t.S, t.stride, t.pad, t.IH, t.IW) / sizeof(float) / G;
    TProblem ts[MAXCLS];
    const float* pk[MAXCLS];
    for (int k = 0; k < G; k++) {
        auto at = [k](const long* a) { return a ? (const float*)a[k] : nullptr; };       // (array pointer null = all null)
        ts[k] = t;
        ts[k].gy = at(gy); ts[k].w = at(w); ts[k].gx = (float*)gx[k]; ts[k].bias = at(bias); ts[k].mul = at(mul); ts[k].add = at(add);
        pk[k] = at(prepacked);
    }
    ClsIn cs[MAXCLS];
    ClassForm f;
    const int n = dgrad_merged(ts, G, pk, ws, stride_f, cs, f);
    if (n && launch_classes(cs, n, f, s)) {
        CC_CHECK_LAUNCH();
        return CC_OK;
    }
    for (int k = 0; k < G; k++) {
        float* wk = ws ? ws + k * stride_f : nullptr;
        for_each_class(ts[k], 1, [&](const TClass& c) {
            if (!c.lattice) return true;
            if (c.g.Cin == 0) launch_splitk_epilogue(fill_epc(c.g, c.p, nullptr), s);       // result = epilogue of zero
            else launch_gg(c.g, wk, s, pk[k] ? pk[k] + c.img_off : nullptr, pk[k], &c.p);
            return true;
        });
    }
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_conv2d_dgrad_group(int G, const long* gy, const long* w, const long* bias, const long* gx, const long* mul, float* ws,
                          const long* prepacked, int B, int K, int OH, int OW, long gy_bs, int C, int R, int S, int stride,
                          int pad, int IH, int IW, long gx_bs, long mul_bs, long w_k_stride, long w_c_stride, int act, float act_a,
                          float act_b, void* stream) {
    return dgrad_group_impl(G, gy, w, bias, gx, mul, nullptr, ws, prepacked,
                            tr_problem(B, K, OH, OW, C, R, S, stride, pad, IH, IW, w_k_stride, w_c_stride, gy_bs, gx_bs, mul_bs, 0, act, act_a, act_b),
                            stream);
}

int cc_conv2d_dgrad_group_add(int G, const long* gy, const long* w, const long* gx, const long* mul, const long* add, float* ws,
                              const long* prepacked, int B, int K, int OH, int OW, long gy_bs, int C, int R, int S, int stride,
                              int pad, int IH, int IW, long gx_bs, long mul_bs, long add_bs, long w_k_stride, long w_c_stride,
                              int act, float act_a, float act_b, void* stream) {
    return dgrad_group_impl(G, gy, w, nullptr, gx, mul, add, ws, prepacked,
                            tr_problem(B, K, OH, OW, C, R, S, stride, pad, IH, IW, w_k_stride, w_c_stride, gy_bs, gx_bs, mul_bs, add_bs, act, act_a, act_b),
                            stream);
}

int cc_conv2d_dgrad(const float* gy, const float* w, const float* bias_or_null, float* gx, float* ws,
                    const float* prepacked_or_null, int B, int K, int OH, int OW, long gy_bs, int C, int R, int S, int stride,
                    int pad, int IH, int IW, long gx_bs, long w_k_stride, long w_c_stride, int act, float act_a, float act_b,
                    void* stream) {
    const long gyp = (long)gy, wp = (long)w, bp = (long)bias_or_null, gxp = (long)gx, pk = (long)prepacked_or_null;
    return cc_conv2d_dgrad_group(1, &gyp, &wp, &bp, &gxp, nullptr, ws, &pk, B, K, OH, OW, gy_bs, C, R, S, stride, pad, IH, IW, gx_bs,
                                 0, w_k_stride, w_c_stride, act, act_a, act_b, stream);
}

/* ---- heterogeneous launch lists (round 3): n independent problems in as few launches as their tile configurations allow --
 * problems whose kernel instance (BM, CK) agrees share ONE k_conv_patch_multi launch (+ one split-K epilogue launch), <= MAXCLS
 * classes per launch, split-K planned for the launch as a whole.  Records of CL_LONGS longs: include/ccengine.h. */
constexpr int CL_LONGS = 32;
struct ListCls { ClsIn c; int prob; };

static float bits_to_float(long v) { unsigned u = (unsigned)v; float f; memcpy(&f, &u, 4); return f; }

// -> classes of all problems in order (plans: no split yet), or -1 on a malformed record
static int list_classes(int n, const long* d, std::vector<ListCls>& out) {
    for (int i = 0; i < n; i++) {
        const long* r = d + (long)i * CL_LONGS;
        const float act_a = bits_to_float(r[24]), act_b = bits_to_float(r[25]);
        const int B = (int)r[8], Ci = (int)r[9], H0 = (int)r[10], W0 = (int)r[11], Co = (int)r[13], R = (int)r[14], S = (int)r[15];
        const int stride = (int)r[16], pad = (int)r[17], H1 = (int)r[18], W1 = (int)r[19];
        if (B <= 0 || Ci <= 0 || Co <= 0 || R <= 0 || S <= 0 || stride <= 0 || !r[6]) return -1;
        const float* pk = (const float*)r[6];
        if (r[0] == 0) {
            ListCls lc = {};
            lc.c.g = make_fwd((const float*)r[1], (const float*)r[2], (const float*)r[3], (const float*)r[4], (float*)r[5], B, Ci, H0, W0,
                              r[12], Co, R, S, stride, pad, H1, W1, r[20], r[21], (int)r[23], act_a, act_b);
            lc.c.p = plan_conv(lc.c.g);
            lc.c.zeros = pk; lc.c.wp = ws_image(pk); lc.prob = i;
            out.push_back(lc);
        } else {
            if (r[7] && !r[4]) return -1;          // raw accumulation is res (kind 0 form) or add WITH mul
            TProblem t = tr_problem(B, Ci, H0, W0, Co, R, S, stride, pad, H1, W1, r[26], r[27], r[12], r[20], r[21], r[22], (int)r[23], act_a, act_b);
            t.gy = (const float*)r[1]; t.w = (const float*)r[2]; t.bias = (const float*)r[3]; t.gx = (float*)r[5];
            t.mul = (const float*)r[4]; t.add = (const float*)r[7];
            for_each_class(t, 1, [&](const TClass& c) {
                if (!c.lattice) return true;
                ListCls lc = {};
                lc.c.g = c.g; lc.c.p = c.p;
                lc.c.g.add_bs = r[22];
                lc.c.zeros = pk; lc.c.wp = pk + c.img_off; lc.prob = i;
                out.push_back(lc);
                return true;
            });
        }
    }
    return (int)out.size();
}

// split-K of the classes of ONE launch: fill the chip with all of them together, then cut classes whose workgroups would run
// much longer than the launch as a whole (a 512-channel layer on an 8x26 map next to a 128-channel one on 64x208)
static void list_plan_splits(ListCls** cls, int n, int target) {
    long fill = 0;
    double work = 0;
    for (int k = 0; k < n; k++) {
        const ConvPlan& p = cls[k]->c.p;
        const GG& g = cls[k]->c.g;
        const long blocks = conv_blocks(g, p, 1);
        fill += blocks;
        work += (double)blocks * (p.Cpad / p.ck) * ((g.Rt * g.St + 2) / 3);
    }
    const long slots = fill < 256 ? 256 : (fill > 1024 ? 1024 : fill);
    const double t_ideal = work / (double)slots;            // stages per workgroup slot if the launch were perfectly balanced
    for (int k = 0; k < n; k++) {
        ConvPlan& p = cls[k]->c.p;
        const GG& g = cls[k]->c.g;
        const int nchunk = p.Cpad / p.ck;
        long want = 1;
        if (fill < cctools::env_int("CC_CONV_FILL_BELOW", 256) && nchunk >= 4) want = (target + fill - 1) / fill;
        else if (nchunk >= 8) {
            const double len = (double)nchunk * ((g.Rt * g.St + 2) / 3);
            const double cmin = cctools::env_int("CC_CONV_CLASS_STAGES", 24);
            const double cap = t_ideal > cmin ? t_ideal : cmin;
            if (len > 2 * cap) want = (long)(len / cap + 0.999);
        }
        if (want > nchunk / cctools::env_int("CC_CONV_MINCHUNKS", 1)) want = nchunk / cctools::env_int("CC_CONV_MINCHUNKS", 1);
        if (want > cctools::env_int("CC_CONV_MAXSPLIT", 32)) want = cctools::env_int("CC_CONV_MAXSPLIT", 32);
        set_split(p, g, nchunk, want);
    }
}

// groups the classes into launches (same (bm, ck), <= MAXCLS, list order kept inside a launch), plans the splits, assigns the
// partial-slab areas; launches when `launch` (ws != nullptr).  -> floats of workspace needed / used, -1: error
static long list_run(int n, const long* d, float* ws, int target, bool launch, hipStream_t s) {
    std::vector<ListCls> all;
    if (list_classes(n, d, all) < 0) return -1;
    std::vector<char> done(all.size(), 0);
    long off = 64;
    for (size_t i = 0; i < all.size(); i++) {
        if (done[i]) continue;
        if (!all[i].c.p.use_patch) {
            done[i] = 1;
            if (launch) launch_gg_flat(all[i].c.g, s);
            continue;
        }
        if (all[i].c.p.wino) {       // Winograd problems keep the plan of their own geometry: one launch each
            done[i] = 1;
            all[i].c.part = ws ? ws + off : nullptr;
            off += (long)(all[i].c.p.part_floats + all[i].c.p.pad_floats);
            if (launch && !launch_classes(&all[i].c, 1, s)) return -1;
            continue;
        }
        ListCls* grp[MAXCLS];
        int m = 0;
        for (size_t j = i; j < all.size() && m < MAXCLS; j++)
            if (!done[j] && all[j].c.p.use_patch && !all[j].c.p.wino && all[j].c.p.bm == all[i].c.p.bm && all[j].c.p.ck == all[i].c.p.ck) {
                grp[m++] = &all[j];
                done[j] = 1;
            }
        list_plan_splits(grp, m, target);
        ClsIn cs[MAXCLS];
        for (int k = 0; k < m; k++) {
            grp[k]->c.part = ws ? ws + off : nullptr;
            off += (long)grp[k]->c.p.part_floats;
            cs[k] = grp[k]->c;
        }
        if (launch && !launch_classes(cs, m, s, true)) return -1;
    }
    return off;
}

size_t cc_conv2d_list_ws_bytes(int n, const long* desc_host, int split_target) {
    if (n <= 0 || !desc_host) return 0;
    const long f = list_run(n, desc_host, nullptr, split_target > 0 ? split_target : 512, false, nullptr);
    return f < 0 ? 0 : (size_t)f * sizeof(float);
}

int cc_conv2d_list(int n, const long* desc_host, float* ws, int split_target, void* stream) {
    if (n <= 0 || !desc_host || !ws) return CC_ERR_ARG;
    if (list_run(n, desc_host, ws, split_target > 0 ? split_target : 512, true, (hipStream_t)stream) < 0) return CC_ERR_ARG;
    CC_CHECK_LAUNCH();
    return CC_OK;
}

/* ---- introspection (bench.py groups its per-call timings by the kernel a call dispatches to): the name the call's timing scope
 * records (kernel_name of the plan and form the launch itself computes), with "+splitk" appended when a split-K epilogue launch follows.
 * The queries describe a call whose operands are all present and aligned. */
// (g, p): the problem of a launch of its own, or the reference class of the merged form f
static int answer_name(const GG& g, const ConvPlan& p, const ClassForm* f, void* name_out_host, int cap) {
    ccint::HeadConv h;
    const int hk = f ? 0 : head_kernel_of(g, h);         // launch_gg: head kernels first, then the plan
    char nm[128];
    kernel_name(hk, g, p, f, nm, sizeof nm);
    const bool epilogue = f ? f->epi : (!hk && g.Cin > 0 && p.use_patch && p.nsplit > 1);
    snprintf((char*)name_out_host, cap, "%s%s", nm, epilogue ? "+splitk" : "");
    return CC_OK;
}

int cc_conv2d_fwd_kernel(int B, int Cin, int IH, int IW, int Cout, int R, int S, int stride, int pad, int OH, int OW,
                         void* name_out_host, int cap) {
    const GG g = fwd_shape(B, Cin, IH, IW, Cout, R, S, stride, pad, OH, OW);
    return answer_name(g, plan_conv(g), nullptr, name_out_host, cap);
}

/* prepacked: the merged launch of all parity classes where cc_conv2d_dgrad makes one (dgrad_merged).  A call that runs one launch
 * per class (stride > 1 without a prepacked image, or a declined merge) cannot be named by one string: the answer is the kernel of
 * class (0, 0).  A launch without any conv workgroup is named by its epilogue kernel. */
int cc_conv2d_dgrad_kernel(int B, int K, int OH, int OW, int C, int R, int S, int stride, int pad, int IH, int IW,
                           int prepacked, void* name_out_host, int cap) {
    if (cap > 0) ((char*)name_out_host)[0] = 0;
    const TProblem t = tr_problem(B, K, OH, OW, C, R, S, stride, pad, IH, IW, (long)C * R * S, (long)R * S);
    alignas(16) static float operand[64];            // stands for the prepacked image and the workspace: never dereferenced
    if (prepacked) {
        ClsIn cs[MAXCLS];
        ClassForm f;
        const float* pk = operand;
        if (dgrad_merged(&t, 1, &pk, operand, 0, cs, f)) {
            const ClsIn& ref = cs[f.ref < 0 ? 0 : f.ref];
            return answer_name(ref.g, ref.p, &f, name_out_host, cap);
        }
    }
    for_each_class(t, 1, [&](const TClass& c) {
        if (!c.lattice) return true;
        answer_name(c.g, c.p, nullptr, name_out_host, cap);
        return false;
    });
    return CC_OK;
}

}  // extern "C"
