// rec_quat.hpp -- the unit-quaternion helpers shared by recording.hip (seeme_stitch_windows), track.hip (seeme_track_filter) and
// headset.hip (seeme_head_rot_cost): one definition of "the quaternion of an axis-angle vector" and of a rot6d pair, of the blend of two
// of them, of their product and of the way back (include/seeme_hip.h).
#pragma once
#include "api_util.hpp"

struct RecQuat { float w, x, y, z; };

__device__ __forceinline__ RecQuat rec_normalize(RecQuat q) {
    const float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    return {q.w / n, q.x / n, q.y / n, q.z / n};
}

// the Hamilton product p (x) q: the rotation q, then the rotation p
__device__ __forceinline__ RecQuat rec_mul(RecQuat p, RecQuat q) {
    return {p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z, p.w * q.x + p.x * q.w + p.y * q.z - p.z * q.y,
            p.w * q.y - p.x * q.z + p.y * q.w + p.z * q.x, p.w * q.z + p.x * q.y - p.y * q.x + p.z * q.w};
}

__device__ __forceinline__ RecQuat rec_conj(RecQuat q) { return {q.w, -q.x, -q.y, -q.z}; }

__device__ __forceinline__ RecQuat rec_aa_to_quat(const float* a) {
    const float th = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const float k = th > 1e-6f ? sinf(0.5f * th) / th : 0.5f - th * th / 48.f;
    return {cosf(0.5f * th), k * a[0], k * a[1], k * a[2]};
}

__device__ __forceinline__ void rec_quat_to_aa(RecQuat q, float* a) {
    if (q.w < 0.f) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; }           // angle in [0, pi]
    const float vn = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z);
    const float k = vn > 1e-12f ? 2.f * atan2f(vn, q.w) / vn : 2.f;
    a[0] = k * q.x; a[1] = k * q.y; a[2] = k * q.z;
}

// the later one flipped onto the earlier one's hemisphere, slerp, normalised lerp above SEEME_STITCH_NLERP_DOT
__device__ __forceinline__ RecQuat rec_blend(RecQuat p, RecQuat q, float u) {
    float dt = p.w * q.w + p.x * q.x + p.y * q.y + p.z * q.z;
    if (dt < 0.f) { dt = -dt; q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; }
    float kp = 1.f - u, kq = u;
    if (!(dt > SEEME_STITCH_NLERP_DOT)) {
        const float th = acosf(dt), s = sinf(th);
        kp = sinf((1.f - u) * th) / s;
        kq = sinf(u * th) / s;
    }
    return rec_normalize({kp * p.w + kq * q.w, kp * p.x + kq * q.x, kp * p.y + kq * q.y, kp * p.z + kq * q.z});
}

// model-side rot6d (geometry.rot6d_to_rotmat 'prohmr'): a1 = x[0:3], a2 = x[3:6], Gram-Schmidt, columns b1, b2, b1 x b2
__device__ __forceinline__ RecQuat rec_rot6d_to_quat(const float* x) {
    const float n1 = fmaxf(sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), 1e-12f);
    const float b1[3] = {x[0] / n1, x[1] / n1, x[2] / n1};
    const float dd = b1[0] * x[3] + b1[1] * x[4] + b1[2] * x[5];
    const float u[3] = {x[3] - dd * b1[0], x[4] - dd * b1[1], x[5] - dd * b1[2]};
    const float n2 = fmaxf(sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12f);
    const float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    const float b3[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
    // R[r][c]: column 0 = b1, 1 = b2, 2 = b3; the largest of w, x, y, z first (Shepperd)
    const float m00 = b1[0], m10 = b1[1], m20 = b1[2], m01 = b2[0], m11 = b2[1], m21 = b2[2], m02 = b3[0], m12 = b3[1], m22 = b3[2];
    const float tr = m00 + m11 + m22;
    RecQuat q;
    if (tr > 0.f) {
        const float s = sqrtf(tr + 1.f) * 2.f;
        q = {0.25f * s, (m21 - m12) / s, (m02 - m20) / s, (m10 - m01) / s};
    } else if (m00 > m11 && m00 > m22) {
        const float s = sqrtf(1.f + m00 - m11 - m22) * 2.f;
        q = {(m21 - m12) / s, 0.25f * s, (m01 + m10) / s, (m02 + m20) / s};
    } else if (m11 > m22) {
        const float s = sqrtf(1.f + m11 - m00 - m22) * 2.f;
        q = {(m02 - m20) / s, (m01 + m10) / s, 0.25f * s, (m12 + m21) / s};
    } else {
        const float s = sqrtf(1.f + m22 - m00 - m11) * 2.f;
        q = {(m10 - m01) / s, (m02 + m20) / s, (m12 + m21) / s, 0.25f * s};
    }
    return rec_normalize(q);
}

__device__ __forceinline__ void rec_quat_to_rot6d(RecQuat q, float* x) {             // the first two columns of the rotation matrix
    const float w = q.w, a = q.x, b = q.y, c = q.z;
    x[0] = 1.f - 2.f * (b * b + c * c); x[1] = 2.f * (a * b + w * c); x[2] = 2.f * (a * c - w * b);
    x[3] = 2.f * (a * b - w * c); x[4] = 1.f - 2.f * (a * a + c * c); x[5] = 2.f * (b * c + w * a);
}
