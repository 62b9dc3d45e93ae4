// rec_quat.hpp -- the unit-quaternion helpers shared by recording.hip (seeme_stitch_windows) and track.hip (seeme_track_filter): one
// definition of "the quaternion of an axis-angle vector", of the blend of two of them and of the way back (include/seeme_hip.h).
#pragma once
#include "api_util.hpp"

struct RecQuat { float w, x, y, z; };

__device__ __forceinline__ RecQuat rec_normalize(RecQuat q) {
    const float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    return {q.w / n, q.x / n, q.y / n, q.z / n};
}

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
