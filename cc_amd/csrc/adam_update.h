// The ONE Adam update (torch.optim.Adam: betas, eps, weight decay in its L2 form, no amsgrad) of k_adam, k_adam_hyper (optim.hip)
// and k_adam_guard (grad_guard.hip).  The kernels differ in their prologues only -- where lr / betas / eps / weight decay and t
// come from, when the element loads are issued, an early return -- so "the same bits" between the entries is this file, not three
// texts kept alike.  The build keeps -ffp-contract=off: every product and sum below rounds where it is written.
#pragma once
#include "cc_common.h"

namespace ccadam {

struct Coefs {
    float b1, b2, eps, wd, step_size, rs2, grad_scale, coef;
};

// t: the step count of the bias corrections.  wd / coef: read only where WD / COEF is set.
__device__ __forceinline__ Coefs coefs(float lr, float b1, float b2, float eps, float wd, float t, float grad_scale, float coef) {
    const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
    return Coefs{b1, b2, eps, wd, lr / bc1, 1.f / sqrtf(bc2), grad_scale, coef};
}

struct PMV {
    float p, m, v;
};

// One element, by value: the caller stores the result.  WD: weight decay g += wd * p (p before the update) unless the row's wd is
// 0; COEF: the gradient times the guard's clip factor.  Compile-time, so that a kernel without them executes no multiply for them.
template <bool WD, bool COEF>
__device__ __forceinline__ PMV update1(float P, const float G, float M, float V, const Coefs& c) {
    float gr = G * c.grad_scale;
    if (COEF) gr = gr * c.coef;
    if (WD && c.wd != 0.f) gr = gr + c.wd * P;
    const float b1 = c.b1, b2 = c.b2;
    M = b1 * M + (1.f - b1) * gr;
    V = b2 * V + (1.f - b2) * gr * gr;
    P -= c.step_size * (M / (sqrtf(V) * c.rs2 + c.eps));
    return PMV{P, M, V};
}

struct Quad {
    float4 p, g, m, v;
};

__device__ __forceinline__ void load4(Quad& q, const float* p, const float* g, const float* m, const float* v, long i4) {
    q.p = *reinterpret_cast<const float4*>(p + i4);
    q.g = *reinterpret_cast<const float4*>(g + i4);
    q.m = *reinterpret_cast<const float4*>(m + i4);
    q.v = *reinterpret_cast<const float4*>(v + i4);
}

// Elements [i4, i4 + 4) of the range from q (full: all four lie below n and load4 has run), or the scalar tail [i4, n).
template <bool WD, bool COEF>
__device__ __forceinline__ void update4(float* p, const float* g, float* m, float* v, long i4, long n, bool full, Quad& q,
                                        const Coefs& c) {
    if (full) {
        float* P = &q.p.x; const float* G = &q.g.x; float* M = &q.m.x; float* V = &q.v.x;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const PMV r = update1<WD, COEF>(P[k], G[k], M[k], V[k], c);
            P[k] = r.p, M[k] = r.m, V[k] = r.v;
        }
        *reinterpret_cast<float4*>(p + i4) = q.p;
        *reinterpret_cast<float4*>(m + i4) = q.m;
        *reinterpret_cast<float4*>(v + i4) = q.v;
    } else {
        for (long i = i4; i < n; i++) {
            const PMV r = update1<WD, COEF>(p[i], g[i], m[i], v[i], c);
            m[i] = r.m, v[i] = r.v, p[i] = r.p;
        }
    }
}

}  // namespace ccadam
