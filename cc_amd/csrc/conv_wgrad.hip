// Weight gradients of the convolutions:
//      gw[m, c, r, s] = sum_{n, ty, tx} a[n, m, ty, tx] * x[n, c, si*ty - pad + r, si*tx - pad + s]
// (conv2d: a = dY, x = the input; ConvTranspose2d: a = the input, x = dY).  GEMM view: M = channels of a, N = (c, r, s),
// K = pixels, split over pixel ranges with a deterministic second-stage reduction (wgrad_reduce.hip; no atomics).
//
// This file holds the two MFMA kernels that take whatever the specialised kernels decline -- the im2col-style k_wgrad (any
// geometry) and the per-tap k_wgrad3x3 (3x3 / stride 1 / pad 1) -- and the host side of ALL weight-gradient paths: the selection
// (wgrad_candidates: which kernels a geometry may run on, in order of preference; the launch, the workspace size and the name
// query all read that one list), the dispatcher, and the C entry points.  The other kernels live in wino_wgrad.hip (Winograd),
// conv_heads.hip (prediction heads) and wgrad_thin.hip (few channels, many pixels).
#include <stdio.h>
#include <stddef.h>
#include <string.h>
#include "cc_common.h"
#include "conv_internal.h"
#include "cc_tools.h"
#include "../../include/ccengine.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

using ccint::BK;
using ccint::BN;
using ccint::MAXGRP;
using ccint::pick_bm;

// ------------------------------------------------------------------ generic weight gradient (im2col-style gather GEMM)
struct WG {
    const float* a;   // "dY-like" tensor [B, M, AH, AW] (batch stride a_bs), sampled on the full lattice (ty, tx)
    const float* x;   // gathered tensor [B, Cin, IH, IW]
    float* out;       // partial tiles ws[split][M][N] (or the final gradient when nsplit == 1 -> strided store)
    const float* ga[MAXGRP]; const float* gxp[MAXGRP]; float* gout[MAXGRP];   // per-problem pointers (blockIdx.z / nsplit)
    int nsplit;
    int B, M, AH, AW; long a_bs;
    int Cin, IH, IW; long x_bs;
    int Rt, St, dy0, dx0, dstep, si;
    long o_sm, o_sc; int o_ri, o_sj;     // gradient strides (used when direct == 1)
    int direct, accum;
    int pix_per_split;
};

template <int BM>
__device__ __forceinline__ void wgrad_body(const WG& g, const int bx_, const int by_, const int bz_) {
    const int grp = bz_ / g.nsplit, zsplit = bz_ - grp * g.nsplit;
    const float* __restrict__ a_ = g.ga[grp];
    const float* __restrict__ x_ = g.gxp[grp];
    float* __restrict__ out_ = g.gout[grp];
    constexpr int WM = (BM >= 64) ? BM / 2 : 32;
    constexpr int WN = (BM >= 64) ? 64 : 32;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int AP = BM + 4, BP = BN + 4;
    constexpr int AQ = BM / 16;
    __shared__ float As[2][BK * AP];   // As[pp][m]
    __shared__ float Bs[2][BK * BP];   // Bs[pp][jn]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = (BM >= 64) ? (wid >> 1) : 0;
    const int wn = (BM >= 64) ? (wid & 1) : wid;
    const int m0 = by_ * BM;
    const int n0 = bx_ * BN;
    const int RS = g.Rt * g.St;
    const int Ntot = g.Cin * RS;
    const int HWa = g.AH * g.AW;
    const long Ptot = (long)g.B * HWa;
    const long pbeg = (long)zsplit * g.pix_per_split;
    long pend = pbeg + g.pix_per_split;
    if (pend > Ptot) pend = Ptot;
    const int x_cs = g.IH * g.IW;

    // loader roles: pp = tid & 15 (pixel within the chunk), row group = tid >> 4 (16 groups)
    const int pp = tid & 15, rgp = tid >> 4;
    // B columns handled by this thread: jn = rgp + 16*q  -> constant over the pixel loop
    int xoff[8], tdy[8], tdx[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int jn = n0 + rgp + 16 * q;
        if (jn < Ntot) {
            const int c = jn / RS, rem = jn - c * RS;
            const int i = rem / g.St, j = rem - i * g.St;
            tdy[q] = g.dy0 + i * g.dstep;
            tdx[q] = g.dx0 + j * g.dstep;
            xoff[q] = c * x_cs + tdy[q] * g.IW + tdx[q];
        } else {
            tdy[q] = -(1 << 28);
            tdx[q] = 0;
            xoff[q] = 0;
        }
    }
    float ra[AQ], rb[8];
    unsigned okA = 0, okB = 0;
    // branch-free loads: invalid elements read element 0 of their tensor and are zeroed by a select AT STORE TIME
    // (hipcc otherwise wraps every predicated load in its own s_cbranch_execz block; and a select placed right after
    // the load would force s_waitcnt vmcnt(0) ahead of the MFMAs of the current chunk)
    auto load_chunk = [&](long pbase) {
        okA = 0;
        okB = 0;
        const long p = pbase + pp;
        const bool pv = p < pend;
        const long ps = pv ? p : 0;
        const int n = (int)(ps / HWa);
        const int t = (int)(ps - (long)n * HWa);
        const int ty = t / g.AW, tx = t - ty * g.AW;
        const long abase = (long)n * g.a_bs + ty * g.AW + tx;
#pragma unroll
        for (int q = 0; q < AQ; q++) {
            const int m = m0 + rgp + 16 * q;
            const bool ok = pv && (m < g.M);
            ra[q] = a_[ok ? abase + (long)m * HWa : 0];
            okA |= (ok ? 1u : 0u) << q;
        }
        const int iy0 = g.si * ty, ix0 = g.si * tx;
        const long xb = (long)n * g.x_bs + (long)iy0 * g.IW + ix0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int iy = iy0 + tdy[q], ix = ix0 + tdx[q];
            const bool ok = pv && ((unsigned)iy < (unsigned)g.IH) && ((unsigned)ix < (unsigned)g.IW);
            rb[q] = x_[ok ? xb + xoff[q] : 0];
            okB |= (ok ? 1u : 0u) << q;
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int q = 0; q < AQ; q++) As[buf][pp * AP + rgp + 16 * q] = ((okA >> q) & 1u) ? ra[q] : 0.f;
#pragma unroll
        for (int q = 0; q < 8; q++) Bs[buf][pp * BP + rgp + 16 * q] = ((okB >> q) & 1u) ? rb[q] : 0.f;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; a++)
#pragma unroll
        for (int b = 0; b < TN; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

    const int l31 = lane & 31, lk = lane >> 5;
    const long nchunks = (pend > pbeg) ? (pend - pbeg + BK - 1) / BK : 0;
    if (nchunks > 0) {
        load_chunk(pbeg);
        store_chunk(0);
    }
    __syncthreads();
    for (long ch = 0; ch < nchunks; ch++) {
        const int buf = (int)(ch & 1);
        if (ch + 1 < nchunks) load_chunk(pbeg + (ch + 1) * BK);
        {
            float af[BK / 2][TM], bf[BK / 2][TN];
#pragma unroll
            for (int ks = 0; ks < BK / 2; ks++) {
#pragma unroll
                for (int a = 0; a < TM; a++) af[ks][a] = As[buf][(2 * ks + lk) * AP + wm * WM + a * 32 + l31];
#pragma unroll
                for (int b = 0; b < TN; b++) bf[ks][b] = Bs[buf][(2 * ks + lk) * BP + wn * WN + b * 32 + l31];
            }
#pragma unroll
            for (int ks = 0; ks < BK / 2; ks++)
#pragma unroll
                for (int a = 0; a < TM; a++)
#pragma unroll
                    for (int b = 0; b < TN; b++)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ks][a], bf[ks][b], acc[a][b], 0, 0, 0);
        }
        if (ch + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }
    // epilogue: D col = lane&31 -> (c,i,j) column, row -> channel m
#pragma unroll
    for (int b = 0; b < TN; b++) {
        const int jn = n0 + wn * WN + b * 32 + l31;
        if (jn >= Ntot) continue;
        long obase;
        if (g.direct) {
            const int c = jn / RS, rem = jn - c * RS;
            const int i = rem / g.St, j = rem - i * g.St;
            obase = (long)c * g.o_sc + i * g.o_ri + j * g.o_sj;
        } else {
            obase = (long)zsplit * g.M * Ntot + jn;
        }
#pragma unroll
        for (int a = 0; a < TM; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + wm * WM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m < g.M) {
                    float* o = out_ + obase + (g.direct ? (long)m * g.o_sm : (long)m * Ntot);
                    *o = (g.direct && g.accum) ? (*o + acc[a][b][r]) : acc[a][b][r];
                }
            }
    }
}

template <int BM>
__global__ __launch_bounds__(256) void k_wgrad(WG g) {
    if constexpr (CC_XCD_MASK & 4) {
        // XCD order (cc_common.h) over the flattened grid, x fastest: the tiles of one (problem, pixel range) -- which gather the same
        // slices of dY and x -- run on one XCD
        const int gx = (int)gridDim.x, gy = (int)gridDim.y;
        const int b = cc_xcd_order((int)blockIdx.x + gx * ((int)blockIdx.y + gy * (int)blockIdx.z), gx * gy * (int)gridDim.z);
        const int r = b / gx;
        wgrad_body<BM>(g, b - r * gx, r % gy, r / gy);
    } else {
        wgrad_body<BM>(g, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
    }
}

// Problems of DIFFERENT shapes in one launch (the single-layer weight gradients a backward stage leaves parked until its end -- the
// stride-2 / 1x1 / small-map layers: 15-40 us launches of 30-600 workgroups each, mostly ramp-up and drain; cc_conv2d_wgrad_list).
// blockIdx.x ranges over the classes' grids back to back; a class's grid is flattened x-fastest.
constexpr int MAXWCLS = 12;
struct WGM { WG c[MAXWCLS]; int n; int bx_end[MAXWCLS]; int gx[MAXWCLS], gy[MAXWCLS]; };
template <int BM>
__global__ __launch_bounds__(256) void k_wgrad_multi(WGM a) {
    int k = 0, first = 0, end = a.bx_end[0];
#pragma unroll
    for (int q = 0; q < MAXWCLS - 1; q++)
        if (q + 1 < a.n && (int)blockIdx.x >= a.bx_end[q]) { k = q + 1; first = a.bx_end[q]; end = a.bx_end[q + 1]; }
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CC_HIPEMU)
    const WG& g = *(reinterpret_cast<const WG*>((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(WGM, c)) + k);
#else
    const WG& g = a.c[k];
#endif
    const int b = (CC_XCD_MASK & 4) ? cc_xcd_order((int)blockIdx.x - first, end - first) : (int)blockIdx.x - first;      // (as k_wgrad)
    const int gx = a.gx[k], gy = a.gy[k];
    const int bx = b % gx, r = b / gx;
    wgrad_body<BM>(g, bx, r % gy, r / gy);
}

// ------------------------------------------------------------------ weight gradient of 3x3 / stride 1 / pad 1 convs (main path)
// The layers that carry ~85 % of the step's weight-gradient FLOPs.  ONE GEMM PER TAP over the input patch shifted by that tap
// (never materialised; every MFMA is useful work, no im2col padding):
//   D_(i,j)[m][c] += dY[m][pixel] * X[c][pixel + (i-1, j-1)]
// Every byte moves by 16-byte LDS-DMA (4x fewer DMA instructions than the dword form, which is issue-bound, measured) and
// every MFMA operand comes from a conflict-free ds_read_b128:
//   * dY tile [BM m][2 x 32 px] as 16-byte chunks, XOR-swizzled by (m & 15) through the SOURCE address of the DMA
//     (LDS image stays lane-linear); a chunk = 4 pixels = the A operand of two k-steps (lane>>5 picks the pixel);
//   * input patch [32 c][4 rows][40 cols] (cols tx0-4 .. tx0+35: 16-byte aligned in global memory), channel stride 41
//     chunks (odd -> 16 consecutive channels hit 16 different bank quads); three chunks of one patch row hold the B
//     operands of the 3 taps of that row for 4 pixels;
//   * one wave per (tap row i, 32-row m tile): 3 accumulator tiles, 4 ds_read_b128 per 6 MFMAs.
constexpr int W3_PC = 41;       // chunks per channel in the patch (40 used + 1 pad)

struct W3 {
    const float* a; const float* x; const float* zeros; float* ws;
    const float* ga[MAXGRP]; const float* gxp[MAXGRP]; float* gws[MAXGRP];      // per-problem pointers (blockIdx.y)
    int B, M, AH, AW; long a_bs;
    int Cin; long x_bs;
    int tiles_x, tiles_y, ntiles, tiles_per_split, nsplit, Cpad, dbg;
};

// Workgroup = 4 waves (a 3- or 6-wave workgroup lands 2+2+1+1 on the SIMDs and caps at 75 % of the MFMA rate:
// tools/mfma_probe.hip measures 116 vs 155 TFLOP/s).  It covers MT m-tiles x CT channel-tiles (MT*CT = 4) x 3 tap rows
// = 12 (tap row, tile) groups, three per wave = 9 accumulators; every k-step pair costs 4 ds_read_b128 per 12 MFMAs.
template <int MT, int CT>
__global__ __launch_bounds__(256, 2) void k_wgrad3x3(W3 g) {
    const float* __restrict__ a_ = g.ga[blockIdx.y];
    const float* __restrict__ x_ = g.gxp[blockIdx.y];
    float* __restrict__ ws_ = g.gws[blockIdx.y];
    constexpr int BM = 32 * MT, BC = 32 * CT;
    constexpr int A_SLOTS = BM * 16;                           // 16-byte slots of the dY tile
    constexpr int P_SLOTS = ((BC * W3_PC + 63) / 64) * 64;     // rounded up so that every DMA instruction runs all 64 lanes
    HIP_DYNAMIC_SHARED(float, smem)
    float4* As = reinterpret_cast<float4*>(smem);              // [A_SLOTS]
    float4* Ps = reinterpret_cast<float4*>(smem) + A_SLOTS;    // [P_SLOTS]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lk = lane >> 5;
    const int ctiles = g.Cpad / BC;
    const int ctile = blockIdx.x % ctiles, mtile = blockIdx.x / ctiles;
    const int m0 = mtile * BM, c0 = ctile * BC;
    const int HW = g.AH * g.AW;
    const int pt_beg = blockIdx.z * g.tiles_per_split;
    int pt_end = pt_beg + g.tiles_per_split;
    if (pt_end > g.ntiles) pt_end = g.ntiles;

    // this wave's three groups: gidx = wid + 4k -> tap row gidx % 3, tile gidx / 3 -> (mt, ct)
    int g_row[3], g_mt[3], g_ct[3];
    f32x16 acc[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int gi = wid + 4 * k;
        g_row[k] = gi % 3;
        const int tl = gi / 3;
        g_mt[k] = tl % MT;
        g_ct[k] = tl / MT;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[k][j][r] = 0.f;
    }

    auto load_tile = [&](int pt) {
        const int tile_x = pt % g.tiles_x;
        const int r2 = pt / g.tiles_x;
        const int tile_y = r2 % g.tiles_y;
        const int n = r2 / g.tiles_y;
        const int ty0 = tile_y * 2, tx0 = tile_x * 32;
        // dY: LDS slot s = m*16 + sc holds pixel chunk pc = sc ^ (m & 15) of row m  (pc = row*8 + col4)
        for (int s0 = wid * 64; s0 < A_SLOTS; s0 += 256) {
            const int sl = s0 + lane;
            const int mm = sl >> 4, sc = sl & 15;
            const int pc = sc ^ (mm & 15);
            const int ty = ty0 + (pc >> 3), tx = tx0 + 4 * (pc & 7);
            const int m = m0 + mm;
            const bool ok = (m < g.M) && (ty < g.AH) && (tx < g.AW);
            const float* src = ok ? a_ + (long)n * g.a_bs + (long)m * HW + (long)ty * g.AW + tx : g.zeros;
            __builtin_amdgcn_global_load_lds(CC_GLOBAL_PTR(src), CC_LDS_PTR(As + s0), 16, 0, 0);
        }
        // patch: LDS slot s = c*41 + r, r = py*10 + ch (r == 40: pad)
        for (int s0 = wid * 64; s0 < P_SLOTS; s0 += 256) {
            const int sl = s0 + lane;
            const int cc = sl / W3_PC, r = sl - cc * W3_PC;
            const int py = r / 10, ch = r - py * 10;
            const int iy = ty0 - 1 + py, ix = tx0 - 4 + 4 * ch;
            const int c = c0 + cc;
            const bool ok = (cc < BC) && (r < 40) && (c < g.Cin) && ((unsigned)iy < (unsigned)g.AH) && ((unsigned)ix < (unsigned)g.AW);
            const float* src = ok ? x_ + (long)n * g.x_bs + (long)c * HW + (long)iy * g.AW + ix : g.zeros;
            __builtin_amdgcn_global_load_lds(CC_GLOBAL_PTR(src), CC_LDS_PTR(Ps + s0), 16, 0, 0);
        }
    };

    for (int pt = pt_beg; pt < pt_end; pt++) {
        if (pt > pt_beg) __syncthreads();                                 // everyone is done reading the previous tile
        if (!(g.dbg & 1) || pt == pt_beg) load_tile(pt);
        CC_WAIT_VMCNT0();
        __syncthreads();
        // MFMA k index (lane>>5) <-> the two HALVES of a 32-pixel row: lanes 0-31 take pixel chunk pq, lanes 32-63 chunk
        // pq+4, each through its own ds_read_b128 address -> element e of every chunk feeds MFMA e directly
        if (g.dbg & 2) continue;
#pragma unroll
        for (int row = 0; row < 2; row++) {
#pragma unroll 2
            for (int pq = 0; pq < 4; pq++) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int mrow = g_mt[k] * 32 + l31;
                    float4 av = As[mrow * 16 + ((row * 8 + pq + 4 * lk) ^ (mrow & 15))];
                    const float4* Pr = Ps + (g_ct[k] * 32 + l31) * W3_PC + (row + g_row[k]) * 10 + 4 * lk + pq;
                    float4 w0 = Pr[0], w1 = Pr[1], w2 = Pr[2];
                    CC_KEEP4(av); CC_KEEP4(w0); CC_KEEP4(w1); CC_KEEP4(w2);
                    const float a[4] = {av.x, av.y, av.z, av.w};
                    const float w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
#pragma unroll
                    for (int e = 0; e < 4; e++)
#pragma unroll
                        for (int j = 0; j < 3; j++)
                            acc[k][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], w[3 + j + e], acc[k][j], 0, 0, 0);
                }
            }
        }
    }
    // partial slabs ws[split][t][m][c], t = tap_row*3 + j   (the layout of the Winograd kernel's slabs -> same reduce kernel)
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float* o = ws_ + (((long)blockIdx.z * 9 + (g_row[k] * 3 + j)) * g.M) * g.Cpad + c0 + g_ct[k] * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + g_mt[k] * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m < g.M) o[(long)m * g.Cpad] = acc[k][j][r];
            }
        }
    }
}

__global__ void k_zero64(float* p) { p[threadIdx.x] = 0.f; }

// ------------------------------------------------------------------ selection
// pad / IH / IW are not part of a workspace query (`sizing`): conditions on them are then taken to hold -- the launch checks them
struct WgGeom { int B, M, AH, AW, Cin, IH, IW, R, S, si, pad; };

struct W3Plan { bool ok; int mt, nbuf, tiles_x, tiles_y, ntiles, nsplit, tps, Cp32; size_t smem, ws_floats; };

inline W3Plan plan_w3(int B, int M, int AH, int AW, int Cin, int R, int S, int si, int pad, int IH, int IW, int G = 1) {
    W3Plan p = {};
    p.ok = (R == 3 && S == 3 && si == 1 && pad == 1 && IH == AH && IW == AW && (AW % 4) == 0 && AW >= 16 && Cin >= 32 &&
            M >= cctools::env_int("CC_W3_MINM", 64) &&
            !cctools::env_flag("CC_NO_WGRAD3X3"));   // measured (tools/wgrad_ablate.py): wins for M > 64 (1.2-1.45x), loses below 64;
                                                     // M = 64 (<2, 2> tiles): -0.2 ms/step against the thin / generic kernels (r3o A/B)
    if (!p.ok) return p;
    p.mt = (M > 64) ? 4 : ((M > 32 && Cin > 32) ? 2 : ((Cin > 64) ? 1 : 2));
    p.nbuf = 1;
    const int BM = 32 * p.mt, BC = 32 * (4 / p.mt);
    p.Cp32 = ((Cin + BC - 1) / BC) * BC;
    p.tiles_x = (AW + 31) / 32;
    p.tiles_y = (AH + 1) / 2;
    p.ntiles = B * p.tiles_x * p.tiles_y;
    const long base = (long)((M + BM - 1) / BM) * (p.Cp32 / BC) * (G > 1 ? G : 1);
    long nsplit = (cctools::env_int("CC_W3_SPLIT", 512) + base - 1) / base;      // 512: measured -0.27 ms/step vs 256 (r02f A/B)
    const long mt_ = cctools::env_int("CC_W3_MINTILES", 3);
    const long cap = (p.ntiles + mt_ - 1) / mt_;  // >= 6 pixel tiles per split: every split writes a 9*M*Cpad partial slab
    if (nsplit > cap) nsplit = cap;
    if (nsplit > p.ntiles) nsplit = p.ntiles;
    if (nsplit < 1) nsplit = 1;
    p.tps = (int)((p.ntiles + nsplit - 1) / nsplit);
    p.nsplit = (p.ntiles + p.tps - 1) / p.tps;
    p.smem = (size_t)(BM * 16 + ((BC * W3_PC + 63) / 64) * 64) * 16;
    p.ws_floats = 64 + (size_t)p.nsplit * 9 * M * p.Cp32;
    return p;
}

// Winograd over copies of dY and the input with rows zero-padded to a multiple of 4 (see ccint::pad_rows_launch)
struct WinoPadPlan { bool ok; int Wp; ccint::WinoWgradPlan wp; size_t pad_floats; };     // pad_floats: padded x + dY of ONE problem
inline WinoPadPlan wino_pad_plan(int B, int M, int AH, int AW, int Cin, int G) {
    WinoPadPlan p = {};
    if ((AW % 4) == 0 || AH < 2 || cctools::env_flag("CC_NO_WINO_WGRAD_PAD")) return p;
    // large weight matrices only: the copies and the kernel's per-workgroup epilogue have to pay (measured per shape)
    if (M < cctools::env_int("CC_WWP_MINM", 96) || Cin < cctools::env_int("CC_WWP_MINC", 96)) return p;
    p.Wp = (AW + 3) & ~3;
    p.wp = ccint::wino_wgrad_plan(B, M, AH, p.Wp, Cin, G, cctools::env_int("CC_WWP_MINQ", 64));
    p.ok = p.wp.ok != 0;
    p.pad_floats = ((size_t)B * (Cin + M) * AH * p.Wp + 3) & ~(size_t)3;
    return p;
}

// Pixel ranges of the generic kernel for `tiles` output tiles (all problems of the launch) over P pixels.  A problem that will
// share a launch with others (`parked`: cc_conv2d_wgrad_list) does not have to fill the chip alone: fewer, longer pixel ranges --
// fewer 64 KB partial tiles written, reduced and paid for in epilogues (never more splits than stand-alone: the workspace is
// sized for that).  Measured (profiles/r04_ab_round4.txt): target 256 / ranges >= 64 pixels -0.13 ms against the stand-alone
// plan; much longer chains lose again (target 64: +0.5 ms, 32: +1.6 ms -- the kernel is slow per k-step)
inline long generic_nsplit(long tiles, long P, bool parked) {
    const long target = parked ? cctools::env_int("CC_WGRAD_PARK_TARGET", 256) : cctools::env_int("CC_WGRAD_SPLIT_TARGET", 512);
    long nsplit = (target + tiles - 1) / tiles;
    const long mr = parked ? cctools::env_int("CC_WGRAD_PARK_MINRANGE", 64) : cctools::env_int("CC_WGRAD_MINRANGE", 32);
    const long maxsplit = (P + mr - 1) / mr;  // small maps still need >= 256 workgroups: split down to 32-pixel ranges (-0.16 ms/step against 64, r3s3)
    if (nsplit > maxsplit) nsplit = maxsplit;
    return nsplit < 1 ? 1 : nsplit;
}

// The kernels a geometry may run on, in order of preference.  The launch takes the first candidate that really launches (the
// Winograd, head and thin kernels can still turn a problem away for its alignment; the last candidate takes everything), a
// problem's workspace is the largest need over the list and all group sizes, the name query answers with the first entry.
enum WgPath { WG_WINO, WG_WINO_PAD, WG_HEAD, WG_THIN, WG_W3, WG_GENERIC };
struct WgCand {
    WgPath path;
    size_t ws_floats;                       // workspace of one problem
    char name[64];                          // kernel name (timing scope, cc_conv2d_wgrad_kernel)
    ccint::WinoWgradPlan wino; int Wp;      // WG_WINO / WG_WINO_PAD (Wp: padded row length)
    ccint::HeadWgradPlan head;              // WG_HEAD
    W3Plan w3;                              // WG_W3
};
constexpr int WG_MAXCAND = 5;

static int wgrad_candidates(const WgGeom& g, int G, bool sizing, WgCand* out) {
    int n = 0;
    auto add = [&](WgPath path, size_t ws_floats) -> WgCand& {
        out[n] = WgCand{};
        out[n].path = path;
        out[n].ws_floats = ws_floats;
        return out[n++];
    };
    const int pad = sizing ? 1 : g.pad, IH = sizing ? g.AH : g.IH, IW = sizing ? g.AW : g.IW;
    if (g.R == 3 && g.S == 3 && g.si == 1 && pad == 1 && IH == g.AH && IW == g.AW) {
        // Winograd F(3x3, 2x2): 16 instead of 36 multiply-adds per 2x2 tile (wino_wgrad.hip); same slab layout / reduction as k_wgrad3x3
        const ccint::WinoWgradPlan wp = ccint::wino_wgrad_plan(g.B, g.M, g.AH, g.AW, g.Cin, G);
        if (wp.ok) {
            WgCand& c = add(WG_WINO, wp.ws_floats);
            c.wino = wp;
            snprintf(c.name, sizeof c.name, "k_wino_wgrad");
        }
        const WinoPadPlan pp = wino_pad_plan(g.B, g.M, g.AH, g.AW, g.Cin, G);
        if (pp.ok) {
            WgCand& c = add(WG_WINO_PAD, pp.wp.ws_floats + pp.pad_floats);
            c.wino = pp.wp;
            c.Wp = pp.Wp;
            snprintf(c.name, sizeof c.name, "k_wino_wgrad");
        }
        // weight gradient of a prediction head: HBM-bound VALU kernel (conv_heads.hip), one launch per problem
        const ccint::HeadWgradPlan hp = g.M <= 2 ? ccint::head_wgrad_plan(g.B, g.M, g.AH, g.AW, g.Cin) : ccint::HeadWgradPlan{};
        if (hp.ok) {
            WgCand& c = add(WG_HEAD, hp.ws_floats);
            c.head = hp;
            snprintf(c.name, sizeof c.name, "k_wgrad_thinm<%d>", g.M);
        }
    }
    {   // thin layers (wgrad_thin.hip)
        char nm[64] = "";
        if (!sizing) ccint::wgrad_thin_name(g.B, g.M, g.AH, g.AW, g.Cin, g.IH, g.IW, g.R, g.S, g.si, g.pad, nm, sizeof nm);
        const size_t wf = ccint::wgrad_thin_ws_floats(g.B, g.M, g.AH, g.AW, g.Cin, g.R, g.S, g.si);
        if (wf && (sizing || nm[0])) memcpy(add(WG_THIN, wf).name, nm, sizeof nm);
    }
    const W3Plan q = plan_w3(g.B, g.M, g.AH, g.AW, g.Cin, g.R, g.S, g.si, pad, IH, IW, G);
    if (q.ok) {
        WgCand& c = add(WG_W3, q.ws_floats);
        c.w3 = q;
        snprintf(c.name, sizeof c.name, "k_wgrad3x3<%d, %d>", q.mt, 4 / q.mt);
    } else {
        // partial tiles ws[split][M][Cin * R * S] of the stand-alone plan (nothing when the kernel writes the gradient itself)
        const long Ntot = (long)g.Cin * g.R * g.S;
        const int bm = pick_bm(g.M);
        const long nsplit = generic_nsplit(((Ntot + BN - 1) / BN) * ((g.M + bm - 1) / bm), (long)g.B * g.AH * g.AW, false);
        WgCand& c = add(WG_GENERIC, nsplit <= 1 ? 4 : (size_t)nsplit * g.M * Ntot);
        snprintf(c.name, sizeof c.name, "k_wgrad<%d>", bm);
    }
    return n;
}

// launches of the generic kernel collected by cc_conv2d_wgrad_list instead of issued one by one
struct WgradParked { WG g; int bm; dim3 grid; double gflop; };
struct WgradCollector { WgradParked* p; int cap, n; ccint::WinoWgradParked* wino; };      // wino: parked Winograd problems (or null)

static void launch_wgrad_parked(const WgradCollector& c, hipStream_t s) {
    for (int bm = 128; bm >= 32; bm /= 2) {
        int i = 0;
        while (i < c.n) {
            WGM m = {};
            long blk = 0;
            double gf = 0;
            for (; i < c.n && m.n < MAXWCLS; i++) {
                if (c.p[i].bm != bm) continue;
                const dim3& gr = c.p[i].grid;
                const long nb = (long)gr.x * gr.y * gr.z;
                if (m.n && blk + nb >= (1l << 31)) break;          // (a problem that large goes into a launch of its own: never dropped)
                m.c[m.n] = c.p[i].g;
                m.gx[m.n] = (int)gr.x; m.gy[m.n] = (int)gr.y;
                blk += nb;
                m.bx_end[m.n] = (int)blk;
                gf += c.p[i].gflop;
                m.n++;
            }
            if (!m.n) break;
            char nm[64];
            snprintf(nm, sizeof nm, "k_wgrad_multi<%d>%s", bm, "");
            cctiming::Scope tsc(nm, gf, s);
            if (bm == 128) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad_multi<128>), dim3((unsigned)blk), dim3(256), 0, s, m);
            else if (bm == 64) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad_multi<64>), dim3((unsigned)blk), dim3(256), 0, s, m);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad_multi<32>), dim3((unsigned)blk), dim3(256), 0, s, m);
        }
    }
}

// ------------------------------------------------------------------ the launches
struct WgCall {      // one group call: G same-shaped problems (a / x / gw: host arrays of device addresses)
    int G; const long *a, *x, *gw;
    float* ws; size_t stride_f;             // problem k owns ws + k * stride_f (cc_conv2d_wgrad_ws_bytes() each)
    WgGeom g; long a_bs, x_bs, o_sm, o_sc; int accumulate;
    hipStream_t s; ccint::RedSink* sink; const float* zeros64; WgradCollector* park;
    float* area(int k) const { return ws + k * stride_f; }
};
constexpr int WG_DECLINED = 1;      // a path's answer when it launched nothing (else CC_OK / CC_ERR_ARG)

// second stage of the G problems over per-tap slabs slabs[k][split][tap 9][m][Cp] (reduce kind 1: Winograd, k_wgrad3x3)
static int emit_slab_reduce(const WgCall& c, float* const* slabs, int nsplit, int Cp) {
    long rd[MAXGRP][ccint::RD_LONGS];
    for (int k = 0; k < c.G; k++) {
        const long d[ccint::RD_LONGS] = {1, (long)slabs[k], (long)c.gw[k], nsplit, c.accumulate, c.o_sm, c.o_sc, 9, c.g.M, c.g.Cin, Cp};
        memcpy(rd[k], d, sizeof d);
    }
    return ccint::wgrad_reduce_emit(c.sink, &rd[0][0], c.G, c.s);
}

// ... over partial tiles [split][M][Cin * R * S] at the start of each problem's area (reduce kind 0: head kernel, k_wgrad)
static int emit_tile_reduce(const WgCall& c, long nsplit) {
    const WgGeom& g = c.g;
    long rd[MAXGRP][ccint::RD_LONGS];
    for (int k = 0; k < c.G; k++) {
        const long d[ccint::RD_LONGS] = {0, (long)c.area(k), (long)c.gw[k], nsplit, c.accumulate, c.o_sm, c.o_sc, g.M,
                                         (long)g.Cin * g.R * g.S, g.R * g.S, g.S, g.S, 1};
        memcpy(rd[k], d, sizeof d);
    }
    return ccint::wgrad_reduce_emit(c.sink, &rd[0][0], c.G, c.s);
}

// Winograd, on the tensors themselves or (WG_WINO_PAD) on zero-padded copies behind the problem's slabs
static int run_wino(const WgCall& c, const WgCand& cd) {
    const WgGeom& g = c.g;
    const bool padded = cd.path == WG_WINO_PAD;
    const int W = padded ? cd.Wp : g.AW;                // row length the kernel sees
    ccint::WinoWgradParked* wpark = c.park ? c.park->wino : nullptr;
    const bool parks = wpark && wpark->n + c.G <= ccint::WINO_WGRAD_PARK_CAP;
    const ccint::WinoWgradPlan wp = parks ? ccint::wino_wgrad_plan_parked(cd.wino, g.M) : cd.wino;
    const size_t slabs = (cd.wino.ws_floats + 3) & ~(size_t)3;      // the padded copies keep their place behind the stand-alone plan's slabs
    const float *ap[MAXGRP], *xp[MAXGRP];
    float* wsp[MAXGRP];
    ccint::PadJob jobs[2 * MAXGRP];
    for (int k = 0; k < c.G; k++) {
        ap[k] = (const float*)c.a[k]; xp[k] = (const float*)c.x[k]; wsp[k] = c.area(k) + 64;
        if (padded) {
            float* xpad = c.area(k) + slabs;
            float* apad = xpad + (size_t)g.B * g.Cin * g.AH * W;
            jobs[2 * k] = ccint::PadJob{xp[k], xpad, c.x_bs, g.Cin * g.AH};
            jobs[2 * k + 1] = ccint::PadJob{ap[k], apad, c.a_bs, g.M * g.AH};
            xp[k] = xpad; ap[k] = apad;
        }
    }
    char nm[128];
    int nl = snprintf(nm, sizeof nm, "%s", cd.name);
    if (cctools::env_flag("CC_TIMING_DETAIL")) {
        nl += snprintf(nm + nl, sizeof nm - nl, " G%d B%d M%d C%d %dx%d", c.G, g.B, g.M, g.Cin, g.AH, g.AW);
        if (padded) nl += snprintf(nm + nl, sizeof nm - nl, "(pad %d)", W);
        snprintf(nm + nl, sizeof nm - nl, " k%d wg%d", wp.nsplit, wp.nmb * wp.ncb * c.G * wp.nsplit);
    }
    bool ok;
    {
        cctiming::Scope tsc(nm, 2e-9 * 16.0 * c.G * g.B * ((g.AH + 1) / 2) * ((W + 1) / 2) * (double)g.M * g.Cin, c.s, !parks);
        if (padded) ccint::pad_rows_launch(jobs, 2 * c.G, g.B, g.AW, W, c.s);
        ok = ccint::wino_wgrad_launch(wp, ap, xp, wsp, c.G, g.B, g.M, g.AH, W, padded ? (long)g.M * g.AH * W : c.a_bs, g.Cin,
                                      padded ? (long)g.Cin * g.AH * W : c.x_bs, c.s, wpark);
    }
    return ok ? emit_slab_reduce(c, wsp, wp.nsplit, wp.Cp) : WG_DECLINED;
}

static int run_head(const WgCall& c, const WgCand& cd) {
    const WgGeom& g = c.g;
    const ccint::HeadWgradPlan& hp = cd.head;
    char nm[128];
    const int nl = snprintf(nm, sizeof nm, "%s", cd.name);
    if (cctools::env_flag("CC_TIMING_DETAIL"))
        snprintf(nm + nl, sizeof nm - nl, " G%d B%d M%d C%d %dx%d r3 s1 k%d", c.G, g.B, g.M, g.Cin, g.AH, g.AW, hp.nblk);
    bool ok = true;
    {
        cctiming::Scope tsc(nm, 2e-9 * c.G * g.B * g.AH * g.AW * (double)g.M * g.Cin * 9, c.s);
        for (int k = 0; k < c.G && ok; k++)
            ok = ccint::head_wgrad_launch(hp, (const float*)c.a[k], (const float*)c.x[k], c.area(k), g.B, g.M, g.AH, g.AW, c.a_bs, g.Cin,
                                          c.x_bs, c.s);
    }
    if (!ok) return WG_DECLINED;
    if (cctools::env_flag("CC_HEAD_TRACE"))
        fprintf(stderr, "head wgrad: G%d B%d M%d C%d %dx%d R%d nblk %d\n", c.G, g.B, g.M, g.Cin, g.AH, g.AW, hp.R, hp.nblk);
    return emit_tile_reduce(c, hp.nblk);
}

// thin layers fill the chip on their own: one launch per problem (which emits its own reduce descriptor)
static int run_thin(const WgCall& c, const WgCand& cd) {
    const WgGeom& g = c.g;
    char nm[128];
    const int nl = snprintf(nm, sizeof nm, "%s", cd.name);
    if (cctools::env_flag("CC_TIMING_DETAIL"))
        snprintf(nm + nl, sizeof nm - nl, " G%d B%d M%d C%d %dx%d r%d s%d", c.G, g.B, g.M, g.Cin, g.AH, g.AW, g.R, g.si);
    // (alignment can still turn a problem away, then the record brackets nothing)
    cctiming::Scope tsc(nm, 2e-9 * c.G * g.B * g.AH * g.AW * (double)g.M * g.Cin * g.R * g.S, c.s, !ccint::wgrad_thin_parking());
    bool thin = true;
    for (int k = 0; k < c.G && thin; k++)
        thin = ccint::wgrad_thin_launch((const float*)c.a[k], (const float*)c.x[k], (float*)c.gw[k], c.area(k), g.B, g.M, g.AH, g.AW,
                                        c.a_bs, g.Cin, g.IH, g.IW, c.x_bs, g.R, g.S, g.si, g.pad, c.o_sm, c.o_sc, c.accumulate, c.s,
                                        c.sink);
    // eligibility depends on the geometry (and 16-byte alignment of the pointers): all problems or none, in practice
    return thin ? CC_OK : WG_DECLINED;
}

static int run_w3(const WgCall& c, const WgCand& cd) {
    const WgGeom& g = c.g;
    const W3Plan& q = cd.w3;
    W3 w = {};
    w.zeros = c.zeros64 ? c.zeros64 : c.ws;
    for (int k = 0; k < c.G; k++) { w.ga[k] = (const float*)c.a[k]; w.gxp[k] = (const float*)c.x[k]; w.gws[k] = c.area(k) + 64; }
    w.B = g.B; w.M = g.M; w.AH = g.AH; w.AW = g.AW; w.a_bs = c.a_bs; w.Cin = g.Cin; w.x_bs = c.x_bs;
    w.tiles_x = q.tiles_x; w.tiles_y = q.tiles_y; w.ntiles = q.ntiles; w.tiles_per_split = q.tps; w.nsplit = q.nsplit;
    w.Cpad = q.Cp32;
    if (!c.zeros64) hipLaunchKernelGGL(k_zero64, dim3(1), dim3(64), 0, c.s, c.ws);      // the LDS-DMA halo source (a kernel, not a memset node)
    const int BM = 32 * q.mt, BC = 32 * (4 / q.mt);
    dim3 grid((unsigned)(((g.M + BM - 1) / BM) * (q.Cp32 / BC)), (unsigned)c.G, (unsigned)q.nsplit);
    w.dbg = cctools::env_int("CC_W3_DBG", 0);
    {
        char nm[128];
        const int nl = snprintf(nm, sizeof nm, "%s", cd.name);
        if (cctools::env_flag("CC_TIMING_DETAIL"))
            snprintf(nm + nl, sizeof nm - nl, " G%d B%d M%d C%d %dx%d k%d wg%d", c.G, g.B, g.M, g.Cin, g.AH, g.AW, q.nsplit,
                     (int)(grid.x * grid.y * grid.z));
        cctiming::Scope tsc(nm, 2e-9 * c.G * g.B * g.AH * g.AW * (double)g.M * g.Cin * 9, c.s);
        if (q.mt == 4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad3x3<4, 1>), grid, dim3(256), q.smem, c.s, w);
        else if (q.mt == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad3x3<2, 2>), grid, dim3(256), q.smem, c.s, w);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad3x3<1, 4>), grid, dim3(256), q.smem, c.s, w);
    }
    return emit_slab_reduce(c, w.gws, q.nsplit, q.Cp32);
}

static int run_generic(const WgCall& c, const WgCand& cd) {
    const WgGeom& g = c.g;
    const long Ntot = (long)g.Cin * g.R * g.S;
    const long P = (long)g.B * g.AH * g.AW;
    const int bm = pick_bm(g.M);
    const bool parked = c.park && c.park->n < c.park->cap;
    long nsplit = generic_nsplit(((Ntot + BN - 1) / BN) * ((g.M + bm - 1) / bm) * c.G, P, parked);
    long pps = (P + nsplit - 1) / nsplit;
    pps = ((pps + BK - 1) / BK) * BK;
    nsplit = (P + pps - 1) / pps;
    WG w = {};
    w.B = g.B; w.M = g.M; w.AH = g.AH; w.AW = g.AW; w.a_bs = c.a_bs;
    w.Cin = g.Cin; w.IH = g.IH; w.IW = g.IW; w.x_bs = c.x_bs;
    w.Rt = g.R; w.St = g.S; w.dy0 = -g.pad; w.dx0 = -g.pad; w.dstep = 1; w.si = g.si;
    w.o_sm = c.o_sm; w.o_sc = c.o_sc; w.o_ri = g.S; w.o_sj = 1;
    w.direct = (nsplit == 1);
    w.accum = c.accumulate;
    w.nsplit = (int)nsplit;
    for (int k = 0; k < c.G; k++) {
        w.ga[k] = (const float*)c.a[k]; w.gxp[k] = (const float*)c.x[k];
        w.gout[k] = w.direct ? (float*)c.gw[k] : c.area(k);
    }
    w.pix_per_split = (int)pps;
    dim3 grid((unsigned)((Ntot + BN - 1) / BN), (unsigned)((g.M + bm - 1) / bm), (unsigned)(nsplit * c.G));
    const double gflop = 2e-9 * c.G * g.B * g.AH * g.AW * (double)g.M * g.Cin * g.R * g.S;
    if (parked) {
        c.park->p[c.park->n++] = WgradParked{w, bm, grid, gflop};
    } else {
        char nm[128];
        const int nl = snprintf(nm, sizeof nm, "%s", cd.name);
        if (cctools::env_flag("CC_TIMING_DETAIL"))
            snprintf(nm + nl, sizeof nm - nl, " G%d B%d M%d C%d %dx%d r%d s%d k%ld wg%d", c.G, g.B, g.M, g.Cin, g.AH, g.AW, g.R, g.si,
                     (long)nsplit, (int)(grid.x * grid.y * grid.z));
        cctiming::Scope tsc(nm, gflop, c.s);
        if (bm == 128) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad<128>), grid, dim3(256), 0, c.s, w);
        else if (bm == 64) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad<64>), grid, dim3(256), 0, c.s, w);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wgrad<32>), grid, dim3(256), 0, c.s, w);
    }
    return w.direct ? CC_OK : emit_tile_reduce(c, nsplit);
}

}  // namespace

extern "C" {

size_t cc_conv2d_wgrad_ws_bytes(int B, int M, int AH, int AW, int Cin, int R, int S, int si) {
    // pad and the input size are confirmed at launch: size for every path the geometry may take AND what it would fall back to
    const WgGeom g = {B, M, AH, AW, Cin, 0, 0, R, S, si, 0};
    WgCand c[WG_MAXCAND];
    size_t floats = 0;
    for (int G = 1; G <= MAXGRP; G++) {       // every group size: the split search of the Winograd plans is not monotonic in G
        const int n = wgrad_candidates(g, G, true, c);
        for (int i = 0; i < n; i++)
            if (c[i].ws_floats > floats) floats = c[i].ws_floats;
    }
    return (floats * sizeof(float) + 15) & ~(size_t)15;        // (the areas of a group's problems follow each other: keep them 16-byte aligned)
}

/* gw[m, c, r, s] (strides o_*) = sum_{n,ty,tx} a[n, m, ty, tx] * x[n, c, si*ty - pad + r, si*tx - pad + s].
 * conv2d weight-gradient: a = dY [B,Cout,OH,OW], x = input, si = stride, o strides of [Cout,Cin,R,S];
 * ConvTranspose2d weight-gradient: a = input [B,Cin,IH,IW], x = dY, si = stride, o strides of [Cin,Cout,R,S].
 * Group form: G (<= 4) same-shaped problems in one launch (+ one reduction launch); a / x / gw: HOST arrays of device
 * addresses; ws: G consecutive areas of cc_conv2d_wgrad_ws_bytes() each. */
static int wgrad_group_impl(int G, const long* a, const long* x, const long* gw, float* ws, int B, int M, int AH, int AW, long a_bs,
                            int Cin, int IH, int IW, long x_bs, int R, int S, int si, int pad, long o_sm, long o_sc, int accumulate,
                            void* stream, ccint::RedSink* sink, const float* zeros64 = nullptr, WgradCollector* park = nullptr) {
    if (G <= 0 || G > MAXGRP || B <= 0 || M <= 0 || Cin <= 0) return CC_ERR_ARG;
    const WgCall c = {G, a, x, gw, ws, cc_conv2d_wgrad_ws_bytes(B, M, AH, AW, Cin, R, S, si) / sizeof(float),
                      WgGeom{B, M, AH, AW, Cin, IH, IW, R, S, si, pad}, a_bs, x_bs, o_sm, o_sc, accumulate,
                      (hipStream_t)stream, sink, zeros64, park};
    WgCand cand[WG_MAXCAND];
    const int n = wgrad_candidates(c.g, G, false, cand);
    for (int i = 0; i < n; i++) {
        const WgCand& cd = cand[i];
        const int r = cd.path == WG_WINO || cd.path == WG_WINO_PAD ? run_wino(c, cd)
                      : cd.path == WG_HEAD ? run_head(c, cd)
                      : cd.path == WG_THIN ? run_thin(c, cd)
                      : cd.path == WG_W3   ? run_w3(c, cd)
                                           : run_generic(c, cd);
        if (r == WG_DECLINED) continue;
        if (r != CC_OK) return CC_ERR_ARG;
        CC_CHECK_LAUNCH();
        return CC_OK;
    }
    return CC_ERR_ARG;      // (not reached: the last candidate takes every problem)
}

int cc_conv2d_wgrad_group(int G, const long* a, const long* x, const long* gw, float* ws, int B, int M, int AH, int AW, long a_bs,
                          int Cin, int IH, int IW, long x_bs, int R, int S, int si, int pad, long o_sm, long o_sc, int accumulate,
                          void* stream) {
    return wgrad_group_impl(G, a, x, gw, ws, B, M, AH, AW, a_bs, Cin, IH, IW, x_bs, R, S, si, pad, o_sm, o_sc, accumulate, stream,
                            nullptr);
}

/* ... with the reductions of the partial slabs left to the caller: their descriptors (16 longs each, at most G) are written to
 * red_host[0 .. *nred_host) and ws must stay untouched until cc_wgrad_reduce_table has run on them.  zeros64_or_null: 64 zero
 * floats that outlive the launch (the LDS-DMA source of halo pixels; without it a fill launch precedes the kernel). */
int cc_conv2d_wgrad_group_defer(int G, const long* a, const long* x, const long* gw, float* ws, int B, int M, int AH, int AW,
                                long a_bs, int Cin, int IH, int IW, long x_bs, int R, int S, int si, int pad, long o_sm, long o_sc,
                                int accumulate, const float* zeros64_or_null, long* red_host, int red_cap, int* nred_host,
                                void* stream) {
    if (!red_host || !nred_host || red_cap < G) return CC_ERR_ARG;
    ccint::RedSink sink = {red_host, red_cap, 0};
    const int r = wgrad_group_impl(G, a, x, gw, ws, B, M, AH, AW, a_bs, Cin, IH, IW, x_bs, R, S, si, pad, o_sm, o_sc, accumulate,
                                   stream, &sink, zeros64_or_null);
    *nred_host = sink.n;
    return r;
}

/* n groups of DIFFERENT shapes (what a backward stage has parked at its end): desc_host = n x 32 longs
 *   {G, a[4], x[4], gw[4], ws, B, M, AH, AW, a_bs, Cin, IH, IW, x_bs, R, S, si, pad, o_sm, o_sc, accumulate, 0, 0}
 * -- each group exactly as one cc_conv2d_wgrad_group_defer call (same kernels, same arithmetic, same reduce descriptors, in list
 * order), except that the groups the planner sends to the generic kernel share launches (k_wgrad_multi: up to 12 per launch). */
int cc_conv2d_wgrad_list(int n, const long* desc_host, const float* zeros64_or_null, long* red_host, int red_cap, int* nred_host,
                         void* stream) {
    if (n <= 0 || !desc_host || !red_host || !nred_host) return CC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    constexpr int CAP = 64;
    static thread_local WgradParked parked[CAP];
    static thread_local ccint::WinoWgradParked wino_parked;
    wino_parked.n = 0;
    WgradCollector col = {parked, CAP, 0, cctools::env_flag("CC_NO_WINO_WGRAD_LIST") ? nullptr : &wino_parked};
    ccint::RedSink sink = {red_host, red_cap, 0};
    // the thin weight gradients of the list share launches too (wgrad_thin.hip: per kernel instance); launched when this call ends
    struct ThinPark {
        hipStream_t s; bool was;
        explicit ThinPark(hipStream_t st) : s(st), was(ccint::wgrad_thin_park(true)) {}
        ~ThinPark() {
            const double gf = ccint::wgrad_thin_parked_gflop();
            if (gf > 0) {
                cctiming::Scope tsc("k_wgrad_thin_multi", gf, s);
                ccint::wgrad_thin_flush(s);
            }
            ccint::wgrad_thin_park(was);
        }
    } thin_park(s);
    for (int i = 0; i < n; i++) {
        const long* d = desc_host + 32l * i;
        const int G = (int)d[0];
        // on an error in the middle of the list: what was collected is launched (its reduce descriptors describe slabs that are then
        // really written) and the descriptors emitted so far are handed back, so that the caller's state stays consistent
        auto bail = [&](int code) {
            launch_wgrad_parked(col, s);
            if (wino_parked.n > 0) ccint::wino_wgrad_launch_parked(&wino_parked, s);
            *nred_host = sink.n;
            return code;
        };
        if (G <= 0 || G > MAXGRP || sink.n + G > red_cap) return bail(CC_ERR_ARG);
        const int before = col.n;
        const int r = wgrad_group_impl(G, d + 1, d + 5, d + 9, (float*)d[13], (int)d[14], (int)d[15], (int)d[16], (int)d[17], d[18],
                                       (int)d[19], (int)d[20], (int)d[21], d[22], (int)d[23], (int)d[24], (int)d[25], (int)d[26], d[27],
                                       d[28], (int)d[29], stream, &sink, zeros64_or_null, &col);
        if (r != CC_OK) return bail(r);
        if (col.n > before && col.p[before].g.direct) {
            // a problem that writes its gradient itself (no split): it must not share a launch with an earlier one of the same target
            bool dup = false;
            for (int j = 0; j < before && !dup; j++)
                if (col.p[j].g.direct)
                    for (int u = 0; u < MAXGRP && !dup; u++)
                        for (int v = 0; v < MAXGRP; v++)
                            if (col.p[j].g.gout[u] && col.p[j].g.gout[u] == col.p[before].g.gout[v]) { dup = true; break; }
            if (dup) {
                const WgradParked keep = col.p[before];
                col.n = before;
                launch_wgrad_parked(col, s);
                col.p[0] = keep;
                col.n = 1;
            }
        }
    }
    launch_wgrad_parked(col, s);
    if (wino_parked.n > 0) {
        double gf = 0;
        for (int i = 0; i < wino_parked.n; i++) gf += wino_parked.d[i].gflop;
        cctiming::Scope tsc("k_wino_wgrad_multi", gf, s);
        ccint::wino_wgrad_launch_parked(&wino_parked, s);
    }
    *nred_host = sink.n;
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_conv2d_wgrad(const float* a, const float* x, float* gw, float* ws, int B, int M, int AH, int AW, long a_bs, int Cin,
                    int IH, int IW, long x_bs, int R, int S, int si, int pad, long o_sm, long o_sc, int accumulate, void* stream) {
    const long ap = (long)a, xp = (long)x, gp = (long)gw;
    return cc_conv2d_wgrad_group(1, &ap, &xp, &gp, ws, B, M, AH, AW, a_bs, Cin, IH, IW, x_bs, R, S, si, pad, o_sm, o_sc, accumulate,
                                 stream);
}

/* the kernel a weight-gradient call of this geometry goes to first (bench.py groups its per-call timings by it): the name its
 * timing scope carries */
int cc_conv2d_wgrad_kernel(int B, int M, int AH, int AW, int Cin, int IH, int IW, int R, int S, int si, int pad,
                           void* name_out_host, int cap) {
    WgCand c[WG_MAXCAND];
    wgrad_candidates(WgGeom{B, M, AH, AW, Cin, IH, IW, R, S, si, pad}, 1, false, c);
    snprintf((char*)name_out_host, cap, "%s", c[0].name);
    return CC_OK;
}

}  // extern "C"
