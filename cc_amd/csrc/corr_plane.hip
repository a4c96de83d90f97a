// 21x21 / dilation-2 cost volume of FlowNetC6 (models/FlowNetC6.py:18-30) as GEMMs on the fp32 matrix cores.
//
// A displacement of the D-dilated grid never changes a pixel's residue (y mod D, x mod D): the volume on H x W is D*D independent
// dilation-1 volumes on the residue planes (D = 2: four planes of H/2 x W/2).  Inside a plane, for a tile of TY x TX pixels p and
// the (TY + 20) x (TX + 20) window of candidates q around it,
//   forward   G[p, q]  = sum_c f1[c, p] f2[c, q]                 (M = tile, N = window, K = C), kept where |q - p| <= 10 per axis
//   backward  g1[c, p] = sum_q A[p, q] f2[c, q], A[p, q] = gout[d(p, q), p]  (M = channels, N = tile, K = window; A masked in LDS)
//             g2[c, q] = sum_p A'[q, p] f1[c, p], A'[q, p] = gout[d(p, q), p]  (the same kernel with the window mirrored)
// on v_mfma_f32_16x16x4_f32, whose result is a k-ordered fmaf chain per output element.  The K order of every GEMM is the order
// the gather kernels (corr.hip k_corrp_fwd / k_corrp_bwd) sum in -- channels ascending; displacements ascending, which for g2 is the
// window walked backwards -- and the terms they skip (outside the map) are here fmaf(0, 0, acc) or fmaf(0, x, acc) == acc, so the three
// results carry the gather kernels' bits.  No atomics; every output element is written once by one work-item.
//
// Predicate of the entry points (plane_ok below; ops.correlate_patch applies the same one): patch == 21, dilation == 2, H and W even,
// B <= 65535.  Any C >= 1.  Every other shape stays with cc_corr_patch_{fwd,bwd}.
#include "cc_common.h"
#include "../../include/ccengine.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int P = 21, RAD = 10, ND = P * P;
constexpr int TY = 4, TX = 4, TM = TY * TX;                    // tile of plane pixels = one MFMA dimension of 16
constexpr int WY = TY + 2 * RAD, WX = TX + 2 * RAD, NW = WY * WX;   // 24 x 24 = 576 candidates = 36 MFMA tiles of 16
static_assert(TM == 16 && NW % 64 == 0, "tile / window must fill whole 16-wide MFMA tiles, nine per wave");

// ---------------------------------------------------------------------------------------------------------------- forward
constexpr int FKC = 16;            // channels per LDS stage
constexpr int FS = NW + 16;        // row stride of f2s[k][n] / Gs[m][n]: the four k rows of a B fragment land in four bank groups
constexpr int FNT = NW / 64;       // window tiles per wave (9)

__global__ __launch_bounds__(256) void k_cpl_fwd(const float* __restrict__ f1, const float* __restrict__ f2,
                                                 float* __restrict__ out, int C, int H, int W) {
    __shared__ float sm[FKC * FS + FKC * TM];          // 38.9 KB: f2s[FKC][FS] | f1s[FKC][TM]; afterwards Gs[TM][FS]
    float* f2s = sm;
    float* f1s = sm + FKC * FS;
    const int Hp = H >> 1, Wp = W >> 1, HW = H * W, tilesX = (Wp + TX - 1) / TX;
    const int ty0 = ((int)blockIdx.x / tilesX) * TY, tx0 = ((int)blockIdx.x % tilesX) * TX;
    const int ry = blockIdx.y >> 1, rx = blockIdx.y & 1, b = blockIdx.z;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    // this thread's candidates n = t, t + 256, t + 512 and its tile pixel t & 15: offsets in the full map, -1 outside the plane
    int off2[3];
#pragma unroll
    for (int s = 0; s < 3; s++) {
        const int n = t + 256 * s;
        off2[s] = -1;
        if (n < NW) {
            const int qy = ty0 - RAD + n / WX, qx = tx0 - RAD + n % WX;
            if (qy >= 0 && qy < Hp && qx >= 0 && qx < Wp) off2[s] = (2 * qy + ry) * W + 2 * qx + rx;
        }
    }
    int off1 = -1;
    {
        const int m = t & 15, py = ty0 + m / TX, px = tx0 + m % TX;
        if (py < Hp && px < Wp) off1 = (2 * py + ry) * W + 2 * px + rx;
    }
    // window tiles whose rows all lie outside the plane stay zero without any MFMA (wave-uniform)
    bool live[FNT];
#pragma unroll
    for (int j = 0; j < FNT; j++) {
        const int n0 = (wv * FNT + j) * 16;
        const int qa = ty0 - RAD + n0 / WX, qb = ty0 - RAD + (n0 + 15) / WX;
        live[j] = (qa >= 0 && qa < Hp) || (qb >= 0 && qb < Hp);
    }
    const float* a = f1 + (size_t)b * C * HW;
    const float* bb = f2 + (size_t)b * C * HW;
    f32x4 acc[FNT];
#pragma unroll
    for (int j = 0; j < FNT; j++) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the next stage's operands are loaded into registers while the matrix cores work on this one
    float pa, pb[FKC][3];
    auto load_stage = [&](int c0) {
        const int c = c0 + (t >> 4);
        pa = (c < C && off1 >= 0) ? a[(size_t)c * HW + off1] : 0.f;                 // f1s[k = t >> 4][m = t & 15]
#pragma unroll
        for (int k = 0; k < FKC; k++) {
            const bool cin = c0 + k < C;                                            // channels past C are staged as zeros
            const float* row = bb + (size_t)(cin ? c0 + k : 0) * HW;
#pragma unroll
            for (int s = 0; s < 3; s++) pb[k][s] = (cin && off2[s] >= 0) ? row[off2[s]] : 0.f;
        }
    };
    auto store_stage = [&]() {
        f1s[t] = pa;
#pragma unroll
        for (int k = 0; k < FKC; k++)
#pragma unroll
            for (int s = 0; s < 3; s++) {
                const int n = t + 256 * s;
                if (n < NW) f2s[k * FS + n] = pb[k][s];
            }
    };
    load_stage(0);
    for (int c0 = 0; c0 < C; c0 += FKC) {
        __syncthreads();
        store_stage();
        __syncthreads();
        if (c0 + FKC < C) load_stage(c0 + FKC);
        const int ksteps = ((C - c0 < FKC ? C - c0 : FKC) + 3) >> 2;
        for (int ks = 0; ks < ksteps; ks++) {
            const int k = ks * 4 + (lane >> 4);
            const float av = f1s[k * TM + (lane & 15)];
#pragma unroll
            for (int j = 0; j < FNT; j++) {
                if (live[j]) {
                    const float bv = f2s[k * FS + (wv * FNT + j) * 16 + (lane & 15)];
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();
    float* Gs = sm;                                    // G[m][n]: lane holds rows (lane >> 4) * 4 + r of column lane & 15
#pragma unroll
    for (int j = 0; j < FNT; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) Gs[((lane >> 4) * 4 + r) * FS + (wv * FNT + j) * 16 + (lane & 15)] = acc[j][r];
    __syncthreads();
    const float fC = (float)C;
    for (int e = t; e < ND * TM; e += 256) {
        const int m = e & 15, d = e >> 4;
        const int i = d / P, j = d - i * P;
        const int my = m / TX, mx = m % TX;
        const int py = ty0 + my, px = tx0 + mx;
        if (py < Hp && px < Wp) {
            const int qy = py + i - RAD, qx = px + j - RAD;
            const bool in = qy >= 0 && qy < Hp && qx >= 0 && qx < Wp;
            const float v = Gs[m * FS + (my + i) * WX + mx + j];                    // window position of q: (my + i, mx + j)
            out[((size_t)b * ND + d) * HW + (2 * py + ry) * W + 2 * px + rx] = in ? v / fC : 0.f;
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
constexpr int BSA = NW + 4;        // row stride of As[m][n]: the 16 m x 4 k of a fragment read 64 different banks
constexpr int BCH = 64;            // channels per pass: one 16-channel MFMA tile per wave
constexpr int BKQ = 4 * WX;        // candidates per LDS stage: four window rows (96)
constexpr int BSS = BKQ + 4;       // row stride of Ss[c][k] (same bank rule)

// FLIP = false: g = g1, src = f2; the window position (wy, wx) is candidate (ty0 - 10 + wy, tx0 - 10 + wx), gout is read at the tile
// pixel.  FLIP = true: g = g2, src = f1; the window is walked from its far corner, (ty0 + TY + 9 - wy, tx0 + TX + 9 - wx), and gout
// is read at the window pixel -- ascending window index = ascending displacement index in both.
template <bool FLIP>
__global__ __launch_bounds__(256) void k_cpl_bwd(const float* __restrict__ gout, const float* __restrict__ src,
                                                 float* __restrict__ g, int C, int H, int W) {
    __shared__ float As[TM * BSA];                     // 37.1 KB
    __shared__ float Ss[BCH * BSS];                    // 25.6 KB
    __shared__ int woff[NW];                           // 2.3 KB
    const int Hp = H >> 1, Wp = W >> 1, HW = H * W, tilesX = (Wp + TX - 1) / TX;
    const int ty0 = ((int)blockIdx.x / tilesX) * TY, tx0 = ((int)blockIdx.x % tilesX) * TX;
    const int ry = blockIdx.y >> 1, rx = blockIdx.y & 1, b = blockIdx.z;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wy_org = FLIP ? ty0 + TY - 1 + RAD : ty0 - RAD, wx_org = FLIP ? tx0 + TX - 1 + RAD : tx0 - RAD;
    constexpr int SGN = FLIP ? -1 : 1;
    // offsets of the window's candidates in the full map (-1 outside the plane), shared by every channel
    for (int n = t; n < NW; n += 256) {
        const int qy = wy_org + SGN * (n / WX), qx = wx_org + SGN * (n % WX);
        woff[n] = (qy >= 0 && qy < Hp && qx >= 0 && qx < Wp) ? (2 * qy + ry) * W + 2 * qx + rx : -1;
    }
    for (int e = t; e < TM * BSA; e += 256) As[e] = 0.f;
    __syncthreads();
    // A[m][n] = gout[d(m, n), p]: all of a half's loads in flight before the first LDS store
    constexpr int AIT = (ND * TM + 255) / 256;         // 28
#pragma unroll
    for (int h = 0; h < 2; h++) {
        float gv[AIT / 2];
        int at[AIT / 2];
#pragma unroll
        for (int it = 0; it < AIT / 2; it++) {
            const int e = t + 256 * (h * (AIT / 2) + it);
            const int m = e & 15, d = e >> 4;
            const int i = d / P, j = d - i * P;
            const int my = m / TX, mx = m % TX;
            const int py = ty0 + my, px = tx0 + mx;                               // tile pixel
            const int wy = i + (FLIP ? TY - 1 - my : my), wx = j + (FLIP ? TX - 1 - mx : mx);
            const int qy = wy_org + SGN * wy, qx = wx_org + SGN * wx;             // window pixel
            at[it] = -1;
            gv[it] = 0.f;
            if (e < ND * TM && py < Hp && px < Wp && qy >= 0 && qy < Hp && qx >= 0 && qx < Wp) {
                const int gy = FLIP ? qy : py, gx = FLIP ? qx : px;
                at[it] = m * BSA + wy * WX + wx;
                gv[it] = gout[((size_t)b * ND + d) * HW + (2 * gy + ry) * W + 2 * gx + rx];
            }
        }
#pragma unroll
        for (int it = 0; it < AIT / 2; it++)
            if (at[it] >= 0) As[at[it]] = gv[it];
    }
    const float* s = src + (size_t)b * C * HW;
    const float fC = (float)C;
    int offm = -1;                                                                // this lane's tile pixel in the full map
    {
        const int m = lane & 15, py = ty0 + m / TX, px = tx0 + m % TX;
        if (py < Hp && px < Wp) offm = (2 * py + ry) * W + 2 * px + rx;
    }
    // stages = (64 channels) x (four window rows); four rows outside the plane are skipped: A and the operand are zero there
    // (block-uniform).  The loads of the next stage are in flight while the matrix cores work on this one.
    unsigned livemask = 0;
#pragma unroll
    for (int ch = 0; ch < NW / BKQ; ch++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int qy = wy_org + SGN * (ch * 4 + r);
            if (qy >= 0 && qy < Hp) livemask |= 1u << ch;
        }
    constexpr int SIT = BCH * BKQ / 256;               // 24 elements per thread and stage
    float sv[SIT];
    auto load_stage = [&](int cg, int ch) {
#pragma unroll
        for (int it = 0; it < SIT; it++) {
            const int e = t + 256 * it;
            const int cl = e / BKQ, kq = e - cl * BKQ;
            const int off = woff[ch * BKQ + kq], c = cg + cl;
            sv[it] = (c < C && off >= 0) ? s[(size_t)c * HW + off] : 0.f;
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int it = 0; it < SIT; it++) {
            const int e = t + 256 * it;
            const int cl = e / BKQ, kq = e - cl * BKQ;
            Ss[cl * BSS + kq] = sv[it];
        }
    };
    int cg = 0, ch = __builtin_ctz(livemask);          // (the tile's own rows are in the plane: the mask is never empty)
    __syncthreads();                                   // woff
    load_stage(cg, ch);
    store_stage();
    __syncthreads();                                   // As, Ss
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    while (true) {
        int ncg = cg, nch = ch;
        do {
            nch++;
            if (nch == NW / BKQ) { nch = 0; ncg += BCH; }
        } while (!((livemask >> nch) & 1u));
        const bool more = ncg < C;
        if (more) load_stage(ncg, nch);
        const bool active = cg + wv * 16 < C;                                     // wave-uniform
        if (active) {
#pragma unroll 4
            for (int ks = 0; ks < BKQ / 4; ks++) {
                const int k = ks * 4 + (lane >> 4);
                const float av = Ss[(wv * 16 + (lane & 15)) * BSS + k];
                const float bv = As[(lane & 15) * BSA + ch * BKQ + k];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
            }
        }
        if (ncg != cg) {                               // the channel group is complete
            if (active && offm >= 0) {                 // D[c][m]: lane holds channels (lane >> 4) * 4 + r of tile pixel lane & 15
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int c = cg + wv * 16 + (lane >> 4) * 4 + r;
                    if (c < C) g[((size_t)b * C + c) * HW + offm] = acc[r] / fC;
                }
            }
            acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if (!more) break;
        __syncthreads();
        store_stage();
        __syncthreads();
        cg = ncg;
        ch = nch;
    }
}

// the predicate of both entries (ops._corr_plane_ok is its twin on the host side)
bool plane_ok(int B, int C, int H, int W, int patch, int dilation) {
    return B >= 1 && B <= 65535 && C >= 1 && H >= 2 && W >= 2 && patch == P && dilation == 2 && (H % 2) == 0 && (W % 2) == 0;
}

}  // namespace

extern "C" {

int cc_corr_plane_fwd(const float* f1, const float* f2, float* out, int B, int C, int H, int W, int patch, int dilation,
                      void* stream) {
    if (!plane_ok(B, C, H, W, patch, dilation)) return CC_ERR_ARG;
    const int tiles = ((H / 2 + TY - 1) / TY) * ((W / 2 + TX - 1) / TX);
    hipLaunchKernelGGL(k_cpl_fwd, dim3(tiles, 4, B), dim3(256), 0, (hipStream_t)stream, f1, f2, out, C, H, W);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_corr_plane_bwd(const float* gout, const float* f1, const float* f2, float* g1_or_null, float* g2_or_null, int B, int C,
                      int H, int W, int patch, int dilation, void* stream) {
    if (!plane_ok(B, C, H, W, patch, dilation)) return CC_ERR_ARG;
    const int tiles = ((H / 2 + TY - 1) / TY) * ((W / 2 + TX - 1) / TX);
    if (g1_or_null)
        hipLaunchKernelGGL(k_cpl_bwd<false>, dim3(tiles, 4, B), dim3(256), 0, (hipStream_t)stream, gout, f2, g1_or_null, C, H, W);
    if (g2_or_null)
        hipLaunchKernelGGL(k_cpl_bwd<true>, dim3(tiles, 4, B), dim3(256), 0, (hipStream_t)stream, gout, f1, g2_or_null, C, H, W);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
