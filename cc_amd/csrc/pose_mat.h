// pose_vec2mat's rotations in fp32 (inverse_warp.py:82-143): shared by the training step's projections (pose.hip) and the
// odometry evaluation (kitti_eval.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ccpose {

struct Rot { float R[9]; float cx, sx, cy, sy, cz, sz; };

// euler2mat, :82-119: (Rx.Ry).Rz of p[3..5] = (rx, ry, rz)
__device__ __forceinline__ void euler(const float* p, Rot& r) {
    r.cx = cosf(p[3]); r.sx = sinf(p[3]);
    r.cy = cosf(p[4]); r.sy = sinf(p[4]);
    r.cz = cosf(p[5]); r.sz = sinf(p[5]);
    // (Rx.Ry).Rz
    const float a00 = r.cy, a01 = 0.f, a02 = r.sy;
    const float a10 = r.sx * r.sy, a11 = r.cx, a12 = -r.sx * r.cy;
    const float a20 = -r.cx * r.sy, a21 = r.sx, a22 = r.cx * r.cy;
    r.R[0] = a00 * r.cz + a01 * r.sz; r.R[1] = -a00 * r.sz + a01 * r.cz; r.R[2] = a02;
    r.R[3] = a10 * r.cz + a11 * r.sz; r.R[4] = -a10 * r.sz + a11 * r.cz; r.R[5] = a12;
    r.R[6] = a20 * r.cz + a21 * r.sz; r.R[7] = -a20 * r.sz + a21 * r.cz; r.R[8] = a22;
}

// quat2mat, :122-143: q = p[3..5] = (x, y, z), w = 1 before normalisation
__device__ __forceinline__ void quat(const float* p, float (&R)[9]) {
    const float n = sqrtf(1.f + p[3] * p[3] + p[4] * p[4] + p[5] * p[5]);
    const float w = 1.f / n, x = p[3] / n, y = p[4] / n, z = p[5] / n;
    const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    R[0] = w2 + x2 - y2 - z2; R[1] = 2.f * xy - 2.f * wz; R[2] = 2.f * wy + 2.f * xz;
    R[3] = 2.f * wz + 2.f * xy; R[4] = w2 - x2 + y2 - z2; R[5] = 2.f * yz - 2.f * wx;
    R[6] = 2.f * xz - 2.f * wy; R[7] = 2.f * wx + 2.f * yz; R[8] = w2 - x2 - y2 + z2;
}

}  // namespace ccpose
