// KITTI evaluation (reference kitti_eval/depth_evaluation_utils.py, test_disp.py, test_pose.py): the sparse ground-truth depth
// map from velodyne points (generate_depth_map), scipy.ndimage.zoom(order=3, mode='constant') of a prediction plus the clip, the
// per-image Eigen errors with np.median scaling, and the odometry snippet errors (pose_vec2mat, relative composition,
// compute_pose_error) of a whole sequence in one launch.
//
// Same conventions as metrics.hip: workspaces come from the caller, nothing allocates or synchronises with the host, float sums
// are fp64 per-workgroup partials reduced in a fixed order and only integer atomics are used, so results are bit-reproducible.
// The build keeps -ffp-contract=off: every product and sum below rounds where the reference's NumPy expression rounds.
#include <hip/hip_runtime.h>
#include "cc_common.h"
#include "pose_mat.h"
#include "radix_select.h"
#include "../../include/ccengine.h"

namespace {

constexpr int kThreads = 256;
using ccradix::kBins;
constexpr int kSel = 4;                 // selections: gt lower, gt upper, pred lower, pred upper middle element
constexpr int kEigenSums = 7;           // per row: |d|/gt, d^2/gt, d^2, (log gt - log p)^2, thresh < 1.25, 1.25^2, 1.25^3
constexpr int kMaxEigenBlocks = 64;
constexpr int kMaxSnippet = 16;

// ------------------------------------------------------------------------------------------------ (a) velodyne -> depth map
// fp32 bits -> u32 that orders as the float, inverted: the largest key is the smallest float (a min through atomicMax)
__device__ __forceinline__ unsigned min_key(float f) {
    const unsigned b = __float_as_uint(f);
    return ~((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}

__device__ __forceinline__ float min_key_value(unsigned k) {
    const unsigned o = ~k;
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// depth_evaluation_utils.py:167-180 for point i: x >= 0, project with P_velo2im in double, u/z and v/z rounded half to even
// (np.round), minus 1, inside the image.  -> false when the point is dropped.
__device__ __forceinline__ bool velo_project(const float* pts, long i, const double* P, int H, int W, int& u, int& v, double& z) {
    const float* p = pts + 4 * i;
    if (!(p[0] >= 0.f)) return false;
    const double X = p[0], Y = p[1], Z = p[2];
    double r[3];
    for (int k = 0; k < 3; k++) r[k] = ((P[4 * k] * X + P[4 * k + 1] * Y) + P[4 * k + 2] * Z) + P[4 * k + 3];
    const double uu = rint(r[0] / r[2]) - 1.0, vv = rint(r[1] / r[2]) - 1.0;
    if (!(uu >= 0.0 && vv >= 0.0 && uu < (double)W && vv < (double)H)) return false;
    u = (int)uu;
    v = (int)vv;
    z = r[2];
    return true;
}

struct VeloWs {
    unsigned *last, *first_pix, *first_key, *count, *zmin;     // [H*W], [H*W], [K], [K], [K] with K = H*(W-1)+1
};

__device__ __forceinline__ VeloWs velo_ws(void* ws, int H, int W) {
    const long HW = (long)H * W, K = (long)H * (W - 1) + 1;
    unsigned* b = (unsigned*)ws;
    return VeloWs{b, b + HW, b + 2 * HW, b + 2 * HW + K, b + 2 * HW + 2 * K};
}

// pass 1, one work-item per point: the last point per pixel (file order), the first point per pixel and per sub2ind key, the
// key's point count and its minimum z.  sub2ind (:145-146) = v*(W-1) + u - 1; stored at v*(W-1) + u >= 0.
__global__ __launch_bounds__(kThreads) void k_velo_scatter(const float* pts, long N, const double* P, int H, int W, void* ws) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    int u, v;
    double z;
    if (!velo_project(pts, i, P, H, W, u, v, z)) return;
    const VeloWs w = velo_ws(ws, H, W);
    const long pix = (long)v * W + u, key = (long)v * (W - 1) + u;
    atomicMax(&w.last[pix], (unsigned)i + 1u);
    atomicMax(&w.first_pix[pix], ~(unsigned)i);
    atomicMax(&w.first_key[key], ~(unsigned)i);
    atomicAdd(&w.count[key], 1u);
    atomicMax(&w.zmin[key], min_key((float)z));
}

// pass 2, one work-item per pixel: plain assignment (the last point wins, :182), then the duplicate pass (:185-190): for a key
// held by more than one point, the pixel of its first point gets the minimum z of all of them; then depth[depth < 0] = 0.
__global__ __launch_bounds__(kThreads) void k_velo_resolve(const float* pts, const double* P, int H, int W, const void* ws,
                                                           float* depth) {
    const long pix = (long)blockIdx.x * kThreads + threadIdx.x;
    if (pix >= (long)H * W) return;
    const VeloWs w = velo_ws((void*)ws, H, W);
    const unsigned last = w.last[pix];
    float d = 0.f;
    if (last != 0u) {
        const int v = (int)(pix / W), u = (int)(pix - (long)v * W);
        const long key = (long)v * (W - 1) + u;
        if (w.count[key] > 1u && w.first_pix[pix] == w.first_key[key]) {
            d = min_key_value(w.zmin[key]);
        } else {
            int uu, vv;
            double z = 0.0;
            velo_project(pts, (long)last - 1, P, H, W, uu, vv, z);
            d = (float)z;
        }
        d = d < 0.f ? 0.f : d;
    }
    depth[pix] = d;
}

// ----------------------------------------------------------------------------------- (b) zoom(order=3, mode='constant') + clip
// SciPy's cubic B-spline prefilter of one line (ni_splines.c, mirror boundary): gain, causal filter with the full-sum mirror
// initialisation, anticausal filter.  c: n doubles at stride s.
__device__ void prefilter_line(double* c, int n, long s) {
    const double z = sqrt(3.0) - 2.0;
    const double gain = (1.0 - z) * (1.0 - 1.0 / z);
    for (int i = 0; i < n; i++) c[i * s] *= gain;
    const double zn1 = pow(z, (double)(n - 1));
    double c0 = c[0] + zn1 * c[(n - 1) * s];
    double zi = z;
    for (int i = 1; i < n - 1; i++) {
        c0 += zi * (c[i * s] + zn1 * c[(n - 1 - i) * s]);
        zi *= z;
    }
    c[0] = c0 / (1.0 - zn1 * zn1);
    double prev = c[0];
    for (int i = 1; i < n; i++) {
        prev = c[i * s] + z * prev;
        c[i * s] = prev;
    }
    double next = z / (z * z - 1.0) * (z * c[(n - 2) * s] + c[(n - 1) * s]);
    c[(n - 1) * s] = next;
    for (int i = n - 2; i >= 0; i--) {
        next = z * (next - c[i * s]);
        c[i * s] = next;
    }
}

// axis 0 first (spline_filter's order): one work-item per column (b, x), fp32 source -> fp64 coefficients
__global__ __launch_bounds__(kThreads) void k_zoom_prefilter_cols(const float* src, double* c, int B, int h, int w) {
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long)B * w) return;
    const int b = (int)(t / w), x = (int)(t - (long)b * w);
    const long base = (long)b * h * w + x;
    for (int y = 0; y < h; y++) c[base + (long)y * w] = (double)src[base + (long)y * w];
    prefilter_line(c + base, h, w);
}

// then axis 1: one work-item per row (b, y)
__global__ __launch_bounds__(kThreads) void k_zoom_prefilter_rows(double* c, int B, int h, int w) {
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long)B * h) return;
    prefilter_line(c + t * w, w, 1);
}

struct AxisTaps {
    int idx[4];
    double wt[4];
    bool out;
};

// NI_ZoomShift along one axis (grid_mode=False): coordinate o * ((n_in-1)/(n_out-1)); outside [0, n_in-1] -> cval; otherwise
// the four taps from floor - 1, mirrored at the edges, with get_spline_interpolation_weights' cubic weights
__device__ __forceinline__ AxisTaps axis_taps(int o, int n_in, double zoom) {
    AxisTaps a;
    const double cc = (double)o * zoom;
    a.out = cc < 0.0 || cc > (double)(n_in - 1);
    const double fl = floor(cc);
    const int start = (int)fl - 1;
    const double y = cc - fl, zz = 1.0 - y;
    a.wt[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    a.wt[2] = (zz * zz * (zz - 2.0) * 3.0 + 4.0) / 6.0;
    a.wt[0] = zz * zz * zz / 6.0;
    a.wt[3] = ((1.0 - a.wt[0]) - a.wt[1]) - a.wt[2];
    const int s2 = 2 * n_in - 2;
    for (int k = 0; k < 4; k++) {
        int i = start + k;
        i = i < 0 ? -i : i;
        i = i >= n_in ? s2 - i : i;
        a.idx[k] = i;
    }
    return a;
}

// one work-item per output pixel: 16 taps accumulated y-outer, x-inner as (wy*wx)*c in double, cast to fp32, clipped
__global__ __launch_bounds__(kThreads) void k_zoom_interp(const double* c, float* dst, int B, int h, int w, int H, int W, double zy,
                                                         double zx, float lo, float hi) {
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long)B * H * W) return;
    const int b = (int)(t / ((long)H * W));
    const long p = t - (long)b * H * W;
    const int Y = (int)(p / W), X = (int)(p - (long)Y * W);
    const AxisTaps ty = axis_taps(Y, h, zy), tx = axis_taps(X, w, zx);
    double acc = 0.0;
    if (!ty.out && !tx.out) {
        const double* cb = c + (long)b * h * w;
        for (int a = 0; a < 4; a++) {
            const double* row = cb + (long)ty.idx[a] * w;
            for (int k = 0; k < 4; k++) acc += (ty.wt[a] * tx.wt[k]) * row[tx.idx[k]];
        }
    }
    const float v = (float)acc;
    dst[t] = v < lo ? lo : (v > hi ? hi : v);           // np.clip: NaN stays NaN
}

// ------------------------------------------------------------------------------------------------ (c) per-image Eigen errors
// workspace: hist [kSel][kBins] u32 | state [kSel][4] u32 (prefix, rank, count, -) | partial [nblk][2][kEigenSums] f64
struct EigenArgs {
    const float* gt;
    const float* pred;
    int H, W, y1, y2, x1, x2;
    double lo, hi;
    const double* disp;         // [R] displacements (the reader's) or NULL
    const float* pose_norm;     // [R] |pose[:3]| of the pose network's output or NULL
    int R;
};

__device__ __forceinline__ bool eigen_valid(const EigenArgs& a, long i, long bw, float& g, float& p) {
    const int y = a.y1 + (int)(i / bw), x = a.x1 + (int)(i - (i / bw) * bw);
    const long o = (long)y * a.W + x;
    g = a.gt[o];
    p = a.pred[o];
    return (double)g > a.lo && (double)g < a.hi;          // generate_mask (:194-206) inside the Garg crop
}

// radix-select pass `pass` (radix_select.h) of the four middle elements (np.median averages the two middle values of an even count):
// selections 0/1 over the valid gt, 2/3 over the prediction at the same pixels.  Valid keys are positive fp32.
__global__ __launch_bounds__(kThreads) void k_eigen_hist(EigenArgs a, unsigned* hist, const unsigned* state, int pass) {
    __shared__ unsigned h[kSel * kBins];
    ccradix::clear<kThreads>(h, kSel * kBins);
    unsigned pre[kSel];
    for (int s = 0; s < kSel; s++) pre[s] = state[4 * s];
    const long bw = a.x2 - a.x1, n = (long)(a.y2 - a.y1) * bw;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        float g, p;
        if (!eigen_valid(a, i, bw, g, p)) continue;
        const unsigned key[2] = {__float_as_uint(g), __float_as_uint(p)};
        for (int s = 0; s < kSel; s++) ccradix::count_key(h + s * kBins, key[s >> 1], pre[s], pass);
    }
    ccradix::flush<kThreads>(h, hist, kSel * kBins);
}

// one work-item per selection: even selections the lower, odd ones the upper middle element
__global__ __launch_bounds__(64) void k_eigen_select(unsigned* hist, unsigned* state, int pass) {
    const int s = threadIdx.x;
    if (s >= kSel) return;
    ccradix::select(hist + s * kBins, state + 4 * s, pass, (s & 1) != 0);
}

// the two scale factors: row 0 the PoseNet one (test_disp.py:130-136; 0 without displacements > 0), row 1 the median ratio
// (:138) with np.median's mean of the middle pair -- fp64 for the fp64 ground truth, fp32 for the fp32 prediction
__device__ __forceinline__ void eigen_scales(const EigenArgs& a, const unsigned* state, double& s0, double& s1) {
    s0 = 0.0;
    if (a.disp) {
        double sum = 0.0;
        int n = 0;
        for (int r = 0; r < a.R; r++)
            if (a.disp[r] > 0.0) {
                sum += a.disp[r] / (double)a.pose_norm[r];
                n++;
            }
        s0 = n > 0 ? sum / (double)n : 0.0;
    }
    const unsigned cnt = state[2];
    if (cnt == 0) {
        s1 = __builtin_nan("");
        return;
    }
    const float g0 = __uint_as_float(state[0]), g1 = __uint_as_float(state[4]);
    const float p0 = __uint_as_float(state[8]), p1 = __uint_as_float(state[12]);
    const double mg = (cnt & 1u) ? (double)g0 : ((double)g0 + (double)g1) / 2.0;
    const float mp = (cnt & 1u) ? p0 : (p0 + p1) / 2.f;
    s1 = mg / (double)mp;
}

// compute_errors (:171-187) terms of both rows per pixel -> per-workgroup fp64 partials
__global__ __launch_bounds__(kThreads) void k_eigen_terms(EigenArgs a, const unsigned* state, double* partial) {
    __shared__ double red[kThreads];
    double s[2];
    eigen_scales(a, state, s[0], s[1]);
    double acc[2 * kEigenSums];
    for (int j = 0; j < 2 * kEigenSums; j++) acc[j] = 0.0;
    const long bw = a.x2 - a.x1, n = (long)(a.y2 - a.y1) * bw;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        float gf, pf;
        if (!eigen_valid(a, i, bw, gf, pf)) continue;
        const double g = (double)gf, lg = log(g);
        for (int r = 0; r < 2; r++) {
            const double p = (double)pf * s[r];
            const double r0 = g / p, r1 = p / g;
            const double th = (r0 != r0 || r1 != r1) ? r0 + r1 : (r0 > r1 ? r0 : r1);   // np.maximum propagates NaN
            const double d = g - p, d2 = d * d, dl = lg - log(p);
            double* t = acc + r * kEigenSums;
            t[0] += fabs(d) / g;
            t[1] += d2 / g;
            t[2] += d2;
            t[3] += dl * dl;
            t[4] += th < 1.25 ? 1.0 : 0.0;
            t[5] += th < 1.5625 ? 1.0 : 0.0;
            t[6] += th < 1.953125 ? 1.0 : 0.0;
        }
    }
    for (int j = 0; j < 2 * kEigenSums; j++) {
        const double t = cc::block_tree<kThreads, cc::Sum>(acc[j], red);
        if (threadIdx.x == 0) partial[(long)blockIdx.x * 2 * kEigenSums + j] = t;
    }
}

// seven means per row in a fixed order -> out [2,7] = abs_rel, sq_rel, rms, log_rms, a1, a2, a3; row 0 stays 0 without
// displacements (the reference's errors[0] is never written then)
__global__ __launch_bounds__(64) void k_eigen_finish(const double* partial, int nblk, const unsigned* state, int have_pose,
                                                     double* out) {
    const int j = threadIdx.x;
    if (j >= 2 * kEigenSums) return;
    double s = 0.0;
    for (int b = 0; b < nblk; b++) s += partial[(long)b * 2 * kEigenSums + j];
    const double m = s / (double)state[2];
    const int k = j % kEigenSums;
    const double v = (k == 2 || k == 3) ? sqrt(m) : m;
    out[j] = (j < kEigenSums && !have_pose) ? 0.0 : v;
}

int eigen_blocks(int H, int W) {
    const long nb = ((long)H * W + kThreads - 1) / kThreads;
    return (int)(nb < kMaxEigenBlocks ? nb : kMaxEigenBlocks);
}

size_t eigen_counts_bytes() { return (size_t)kSel * (kBins + 4) * sizeof(unsigned); }

// -------------------------------------------------------------------------------------------------- (d) odometry snippets
__device__ __forceinline__ double det3(const double* A) {
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// general 3x3 inverse (adjugate / determinant) of the rotation block of a row-major 3x4 (stride 4) or 3x3 (stride 3)
__device__ __forceinline__ void inv3(const double* M, int ld, double (&I)[9]) {
    const double A[9] = {M[0], M[1], M[2], M[ld], M[ld + 1], M[ld + 2], M[2 * ld], M[2 * ld + 1], M[2 * ld + 2]};
    const double d = det3(A);
    I[0] = (A[4] * A[8] - A[5] * A[7]) / d;
    I[1] = (A[2] * A[7] - A[1] * A[8]) / d;
    I[2] = (A[1] * A[5] - A[2] * A[4]) / d;
    I[3] = (A[5] * A[6] - A[3] * A[8]) / d;
    I[4] = (A[0] * A[8] - A[2] * A[6]) / d;
    I[5] = (A[2] * A[3] - A[0] * A[5]) / d;
    I[6] = (A[3] * A[7] - A[4] * A[6]) / d;
    I[7] = (A[1] * A[6] - A[0] * A[7]) / d;
    I[8] = (A[0] * A[4] - A[1] * A[3]) / d;
}

// pose_vec2mat (inverse_warp.py:146-162) in fp32 of pose i of the snippet with the zero pose inserted at L/2
// (test_pose.py:74-76), promoted to double (:77) -> T [3,4]
__device__ __forceinline__ void snippet_pose(const float* pred, int L, int i, int quat, double (&T)[12]) {
    float p[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int m = L / 2;
    if (i != m) {
        const float* q = pred + 6 * (i < m ? i : i - 1);
        for (int k = 0; k < 6; k++) p[k] = q[k];
    }
    float R[9];
    if (quat) {
        ccpose::quat(p, R);
    } else {
        ccpose::Rot r;
        ccpose::euler(p, r);
        for (int k = 0; k < 9; k++) R[k] = r.R[k];
    }
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = (double)R[3 * r + c];
        T[4 * r + 3] = (double)p[r];
    }
}

struct PoseArgs {
    const float* pred;          // [S, L-1, 6]
    const double* gt;           // [F, 3, 4]
    const int* first;           // [S]
    int S, L, F, step, quat;
    double* err;                // [S, 2]
    double* final_poses;        // [S, L, 3, 4] or NULL
};

// one work-item per snippet, all in fp64 after pose_vec2mat
__global__ __launch_bounds__(64) void k_pose_snippets(PoseArgs a) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.S) return;
    const int L = a.L, f0 = a.first[s];
    double* e = a.err + 2 * (long)s;
    if (f0 < 0 || (long)f0 + (long)(L - 1) * a.step >= a.F) {
        e[0] = e[1] = __builtin_nan("");
        return;
    }
    const float* pred = a.pred + (long)s * (L - 1) * 6;
    double A0[12];                                                  // first_inv_transform (:83)
    snippet_pose(pred, L, 0, a.quat, A0);
    const double* P0 = a.gt + (long)f0 * 12;                         // compensation (pose_evaluation_utils.py:20-23)
    double R0i[9];
    inv3(P0, 4, R0i);
    double pt[kMaxSnippet][3], gtt[kMaxSnippet][3];
    double re = 0.0;
    for (int i = 0; i < L; i++) {
        double T[12], Ri[9];
        snippet_pose(pred, L, i, a.quat, T);
        inv3(T, 4, Ri);                                             // rot_matrices = inv(...) (:79)
        double tr[3];                                               // tr_vectors = -rot @ t (:80)
        for (int r = 0; r < 3; r++) tr[r] = -(Ri[3 * r] * T[3] + Ri[3 * r + 1] * T[7] + Ri[3 * r + 2] * T[11]);
        double Fm[12];                                              // final = A0[:, :3] @ [rot | tr], + A0[:, 3] (:84-85)
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Fm[4 * r + c] = A0[4 * r] * Ri[c] + A0[4 * r + 1] * Ri[3 + c] + A0[4 * r + 2] * Ri[6 + c];
            Fm[4 * r + 3] = (A0[4 * r] * tr[0] + A0[4 * r + 1] * tr[1] + A0[4 * r + 2] * tr[2]) + A0[4 * r + 3];
        }
        if (a.final_poses)
            for (int k = 0; k < 12; k++) a.final_poses[((long)s * L + i) * 12 + k] = Fm[k];
        const double* Pi = a.gt + ((long)f0 + (long)i * a.step) * 12;
        double G[12];                                               // inv(R0) @ [R_i | t_i - t_0]
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) G[4 * r + c] = R0i[3 * r] * Pi[c] + R0i[3 * r + 1] * Pi[4 + c] + R0i[3 * r + 2] * Pi[8 + c];
            G[4 * r + 3] = R0i[3 * r] * (Pi[3] - P0[3]) + R0i[3 * r + 1] * (Pi[7] - P0[7]) + R0i[3 * r + 2] * (Pi[11] - P0[11]);
        }
        for (int r = 0; r < 3; r++) {
            pt[i][r] = Fm[4 * r + 3];
            gtt[i][r] = G[4 * r + 3];
        }
        double Fi[9], Q[9];                                         // compute_pose_error's residual rotation (:113-120)
        inv3(Fm, 4, Fi);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Q[3 * r + c] = G[4 * r] * Fi[c] + G[4 * r + 1] * Fi[3 + c] + G[4 * r + 2] * Fi[6 + c];
        const double v0 = Q[1] - Q[3], v1 = Q[5] - Q[7], v2 = Q[2] - Q[6];
        const double sn = sqrt(v0 * v0 + v1 * v1 + v2 * v2), cs = Q[0] + Q[4] + Q[8] - 1.0;
        re += atan2(sn, cs);
    }
    double num = 0.0, den = 0.0;                                    // least-squares scale (:110)
    for (int i = 0; i < L; i++)
        for (int r = 0; r < 3; r++) {
            num += gtt[i][r] * pt[i][r];
            den += pt[i][r] * pt[i][r];
        }
    const double sc = num / den;
    double ate = 0.0;
    for (int i = 0; i < L; i++)
        for (int r = 0; r < 3; r++) {
            const double d = gtt[i][r] - sc * pt[i][r];
            ate += d * d;
        }
    e[0] = sqrt(ate) / (double)L;
    e[1] = re / (double)L;
}

}  // namespace

extern "C" {

size_t cc_velo_depth_ws(int H, int W) {
    if (H <= 0 || W <= 1) return 0;
    return (size_t)(2 * (long)H * W + 3 * ((long)H * (W - 1) + 1)) * sizeof(unsigned);
}

int cc_velo_depth(const float* points, long N, const double* P_velo2im, float* depth, int H, int W, void* ws, void* stream) {
    if (!P_velo2im || !depth || !ws || N < 0 || (N > 0 && !points) || H <= 0 || W <= 1) return CC_ERR_ARG;
    if (N >= 0xffffffffl) return CC_ERR_ARG;                          // point indices + 1 are u32
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, cc_velo_depth_ws(H, W), s) != hipSuccess) return CC_ERR_LAUNCH;
    if (N > 0) {
        hipLaunchKernelGGL(k_velo_scatter, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, points, N,
                           P_velo2im, H, W, ws);
        CC_CHECK_LAUNCH();
    }
    const long HW = (long)H * W;
    hipLaunchKernelGGL(k_velo_resolve, dim3((unsigned)((HW + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, points, P_velo2im, H,
                       W, (const void*)ws, depth);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

size_t cc_spline_zoom_ws(int B, int h, int w) {
    if (B <= 0 || h <= 1 || w <= 1) return 0;
    return (size_t)B * h * w * sizeof(double);
}

int cc_spline_zoom(const float* src, int B, int h, int w, float* dst, int H, int W, float lo, float hi, void* ws, void* stream) {
    if (!src || !dst || !ws || B <= 0 || h <= 1 || w <= 1 || H <= 1 || W <= 1) return CC_ERR_ARG;
    const hipStream_t s = (hipStream_t)stream;
    double* c = (double*)ws;
    const long ncol = (long)B * w, nrow = (long)B * h, nout = (long)B * H * W;
    hipLaunchKernelGGL(k_zoom_prefilter_cols, dim3((unsigned)((ncol + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, src, c, B, h, w);
    CC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_zoom_prefilter_rows, dim3((unsigned)((nrow + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, c, B, h, w);
    CC_CHECK_LAUNCH();
    // the zoom factors of scipy's zoom: (in - 1) / (out - 1) per axis, in double
    const double zy = (double)(h - 1) / (double)(H - 1), zx = (double)(w - 1) / (double)(W - 1);
    hipLaunchKernelGGL(k_zoom_interp, dim3((unsigned)((nout + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const double*)c, dst, B,
                       h, w, H, W, zy, zx, lo, hi);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

size_t cc_eigen_errors_ws(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return eigen_counts_bytes() + (size_t)eigen_blocks(H, W) * 2 * kEigenSums * sizeof(double);
}

int cc_eigen_errors(const float* gt, const float* pred, int H, int W, double min_depth, double max_depth, const double* disp,
                    const float* pose_norm, int R, double* out, void* ws, void* stream) {
    if (!gt || !pred || !out || !ws || H <= 0 || W <= 0) return CC_ERR_ARG;
    if ((disp != nullptr) != (pose_norm != nullptr) || (disp && R <= 0)) return CC_ERR_ARG;
    const hipStream_t s = (hipStream_t)stream;
    unsigned* hist = (unsigned*)ws;
    unsigned* state = hist + kSel * kBins;
    double* partial = (double*)((char*)ws + eigen_counts_bytes());   // 8-byte aligned: kSel * (kBins + 4) * 4 bytes
    if (hipMemsetAsync(ws, 0, eigen_counts_bytes(), s) != hipSuccess) return CC_ERR_LAUNCH;
    EigenArgs a;
    a.gt = gt;
    a.pred = pred;
    a.H = H;
    a.W = W;
    // Garg crop of generate_mask: the float products truncated by astype(np.int32)
    a.y1 = (int)(0.40810811 * H);
    a.y2 = (int)(0.99189189 * H);
    a.x1 = (int)(0.03594771 * W);
    a.x2 = (int)(0.96405229 * W);
    a.lo = min_depth;
    a.hi = max_depth;
    a.disp = disp;
    a.pose_norm = pose_norm;
    a.R = R;
    const int nblk = eigen_blocks(H, W);
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(k_eigen_hist, dim3(nblk), dim3(kThreads), 0, s, a, hist, (const unsigned*)state, pass);
        CC_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_eigen_select, dim3(1), dim3(64), 0, s, hist, state, pass);
        CC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_eigen_terms, dim3(nblk), dim3(kThreads), 0, s, a, (const unsigned*)state, partial);
    CC_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_eigen_finish, dim3(1), dim3(64), 0, s, (const double*)partial, nblk, (const unsigned*)state, disp ? 1 : 0, out);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

int cc_pose_snippet_errors(const float* pred, const double* gt_seq, const int* first, int S, int L, int F, int step,
                           int rotation_mode, double* err, double* final_or_null, void* stream) {
    if (!pred || !gt_seq || !first || !err || S <= 0 || L < 2 || L > kMaxSnippet || F <= 0 || step <= 0) return CC_ERR_ARG;
    if (rotation_mode != 0 && rotation_mode != 1) return CC_ERR_ARG;
    PoseArgs a = {pred, gt_seq, first, S, L, F, step, rotation_mode, err, final_or_null};
    hipLaunchKernelGGL(k_pose_snippets, dim3((S + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
    CC_CHECK_LAUNCH();
    return CC_OK;
}

}  // extern "C"
