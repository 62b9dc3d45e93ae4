// headset.hip -- the headset's own path as evidence about the wearer: how far the head of every hypothesis strays from the shape of the
// device's trajectory over its window (seeme_head_path_cost, a unary term of seeme_path_select) and the shift that puts the stitched
// motion's head onto the device's path (seeme_head_anchor); and the headset's orientation: how far a hypothesis' head turns against
// the device over its window, up to a constant mount rotation (seeme_head_rot_cost, a unary term as well).  Definitions:
// include/seeme_hip.h; the plain-torch twins are in seeme_amd/recording.py.  fp32 throughout, no atomics: every result is bitwise
// reproducible.
#include "api_util.hpp"
#include "rec_quat.hpp"
#include <math.h>
#include <stdint.h>

#define HS_KMAX 32
#define HS_ROW 72                  // 24 joints x 3 floats
#define HS_HEAD (3 * SEEME_HEAD_JOINT)
#define HS_THREADS 256
#define HS_WAVES (HS_THREADS / 64)
#define HS_RMAX SEEME_HEAD_ANCHOR_RMAX
#define HS_NF (HS_THREADS + 2 * HS_RMAX)

// every lane gets the sum over the wave's 64 lanes: a butterfly of six exchanges, the same tree on every lane (x + y == y + x)
__device__ __forceinline__ float hs_wave_sum(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// ------------------------------------------------------------------ head-path cost
// Partition: one wave per (window w, hypothesis k), HS_WAVES of them to a workgroup.  Lane l owns the frames t = l, l + 64, ... < n and
// adds them in increasing t; the 64 partial sums meet in hs_wave_sum.  Pass 1: o = mean of r_t = head_t - path_t.  Pass 2: the mean of
// |r_t - o|; the frames are read again (a window's 196 head rows and path rows stay in L2).  Only joint 15 of a frame and only frames
// t < n are read.
__global__ __launch_bounds__(HS_THREADS) void k_head_path_cost(const float* __restrict__ jts, const float* __restrict__ path,
                                                               const int32_t* __restrict__ lengths, int WK, int K, int T,
                                                               float* __restrict__ cost) {
    const int lane = threadIdx.x & 63;
    const int wk = blockIdx.x * HS_WAVES + (threadIdx.x >> 6);         // uniform over the wave
    if (wk >= WK) return;
    const int w = wk / K;
    const int n = min(max(lengths[w], 0), T);
    if (n <= 1) {
        if (lane == 0) cost[wk] = 0.f;
        return;
    }
    const float* h = jts + (size_t)wk * T * HS_ROW + HS_HEAD;
    const float* p = path + (size_t)w * T * 3;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int t = lane; t < n; t += 64) {
        const float* a = h + (size_t)t * HS_ROW;
        const float* b = p + (size_t)t * 3;
        sx += a[0] - b[0]; sy += a[1] - b[1]; sz += a[2] - b[2];
    }
    const float fn = (float)n;
    const float ox = hs_wave_sum(sx) / fn, oy = hs_wave_sum(sy) / fn, oz = hs_wave_sum(sz) / fn;
    float s = 0.f;
    for (int t = lane; t < n; t += 64) {
        const float* a = h + (size_t)t * HS_ROW;
        const float* b = p + (size_t)t * 3;
        const float ex = (a[0] - b[0]) - ox, ey = (a[1] - b[1]) - oy, ez = (a[2] - b[2]) - oz;
        s += sqrtf(ex * ex + ey * ey + ez * ez);
    }
    s = hs_wave_sum(s);
    if (lane == 0) cost[wk] = 1000.f * (s / fn);
}

extern "C" int seeme_head_path_cost(const float* jts, const float* path, const int32_t* lengths, int W, int K, int T, float* cost,
                                    void* stream) {
    if (W < 1 || W > 65536) return seeme_fail("head_path_cost: W must be in 1..65536");
    if (K < 1 || K > HS_KMAX) return seeme_fail("head_path_cost: K must be in 1..32");
    if (T < 1 || T > (1 << 20)) return seeme_fail("head_path_cost: T must be in 1..2^20");
    if (!jts || !path || !lengths || !cost) return seeme_fail("head_path_cost: null pointer");
    if (((uintptr_t)jts | (uintptr_t)path | (uintptr_t)lengths | (uintptr_t)cost) & 3)
        return seeme_fail("head_path_cost: every pointer must be 4-byte aligned");
    const int WK = W * K;
    hipLaunchKernelGGL(k_head_path_cost, dim3((WK + HS_WAVES - 1) / HS_WAVES), dim3(HS_THREADS), 0, (hipStream_t)stream, jts, path,
                       lengths, WK, K, T, cost);
    return seeme_check_launch("k_head_path_cost");
}

// ------------------------------------------------------------------ head-rotation cost
// h_t: the quaternion product along the chain 0 -> 3 -> 6 -> 9 -> 12 -> 15 (joint 3c, c = 0..5) of one frame's feature row; each joint
// quaternion is the one seeme_stitch_windows forms (rec_quat.hpp).  Only these six units of the row are read.
__device__ __forceinline__ RecQuat hs_head_quat(const float* row, bool rot6d) {
    RecQuat h = rot6d ? rec_rot6d_to_quat(row) : rec_aa_to_quat(row);
#pragma unroll
    for (int c = 1; c <= SEEME_HEAD_JOINT / 3; ++c)
        h = rec_mul(h, rot6d ? rec_rot6d_to_quat(row + 18 * c) : rec_aa_to_quat(row + 9 * c));
    return h;
}

__device__ __forceinline__ RecQuat hs_shfl(RecQuat q, int src) {
    return {__shfl(q.w, src), __shfl(q.x, src), __shfl(q.y, src), __shfl(q.z, src)};
}

// Partition: as k_head_path_cost, one wave per (w, k) and lane l on the frames t = l, l + 64, ... < n in increasing t.  Pass 1: d_t =
// conj(h_t) (x) dev_t, the device seen from the head; d_0 comes from lane 0 by a shuffle, every d_t is put on its side (s_t) and
// summed, the 64 partial sums meet in hs_wave_sum and m is the normalised sum.  Pass 2: the angle of conj(m) (x) d_t per frame (the
// rows are read and d_t is formed again, by the same expressions), its mean, and zeros for the frames t >= n of angle.
__global__ __launch_bounds__(HS_THREADS) void k_head_rot_cost(const float* __restrict__ feats, int rot6d, int F,
                                                              const float* __restrict__ dev_quat, const int32_t* __restrict__ lengths,
                                                              int WK, int K, int T, float* __restrict__ cost, float* __restrict__ angle) {
    const int lane = threadIdx.x & 63;
    const int wk = blockIdx.x * HS_WAVES + (threadIdx.x >> 6);         // uniform over the wave
    if (wk >= WK) return;
    const int w = wk / K;
    const int n = min(max(lengths[w], 0), T);
    float* ang = angle ? angle + (size_t)wk * T : nullptr;
    if (n <= 1) {
        if (lane == 0) cost[wk] = 0.f;
        if (ang)
            for (int t = lane; t < T; t += 64) ang[t] = 0.f;
        return;
    }
    const float* f = feats + (size_t)wk * T * F;
    const float* q = dev_quat + (size_t)w * T * 4;
    auto seen = [&](int t) {
        const float* b = q + (size_t)t * 4;
        return rec_mul(rec_conj(hs_head_quat(f + (size_t)t * F, rot6d != 0)), RecQuat{b[0], b[1], b[2], b[3]});
    };
    const RecQuat first = lane < n ? seen(lane) : RecQuat{0.f, 0.f, 0.f, 0.f};
    const RecQuat d0 = hs_shfl(first, 0);                             // n >= 2: lane 0 owns frame 0
    RecQuat m = {0.f, 0.f, 0.f, 0.f};
    for (int t = lane; t < n; t += 64) {
        const RecQuat d = t == lane ? first : seen(t);
        const float s = d.w * d0.w + d.x * d0.x + d.y * d0.y + d.z * d0.z < 0.f ? -1.f : 1.f;
        m.w += s * d.w; m.x += s * d.x; m.y += s * d.y; m.z += s * d.z;
    }
    m = rec_normalize({hs_wave_sum(m.w), hs_wave_sum(m.x), hs_wave_sum(m.y), hs_wave_sum(m.z)});
    const RecQuat mc = rec_conj(m);
    float s = 0.f;
    for (int t = lane; t < n; t += 64) {
        const RecQuat r = rec_mul(mc, t == lane ? first : seen(t));
        const float a = 2.f * atan2f(sqrtf(r.x * r.x + r.y * r.y + r.z * r.z), fabsf(r.w)) * 57.29577951308232f;
        s += a;
        if (ang) ang[t] = a;
    }
    if (ang)
        for (int t = n + lane; t < T; t += 64) ang[t] = 0.f;
    s = hs_wave_sum(s);
    if (lane == 0) cost[wk] = s / (float)n;
}

extern "C" int seeme_head_rot_cost(const float* feats, int layout, int F, const float* dev_quat, const int32_t* lengths, int W, int K,
                                   int T, float* cost, float* angle, void* stream) {
    if (W < 1 || W > 65536) return seeme_fail("head_rot_cost: W must be in 1..65536");
    if (K < 1 || K > HS_KMAX) return seeme_fail("head_rot_cost: K must be in 1..32");
    if (T < 1 || T > (1 << 20)) return seeme_fail("head_rot_cost: T must be in 1..2^20");
    bool ok = false;                                                  // the chain ends at joint 15: 16 joint rotations at least
    if (layout == SEEME_STITCH_ROT6D) ok = F == 144;
    else if (layout == SEEME_STITCH_ANGLE) ok = F % 3 == 0 && F >= 3 * (SEEME_HEAD_JOINT + 1);
    else if (layout == SEEME_STITCH_ANGLE_TRANSL) ok = F % 3 == 0 && F >= 3 * (SEEME_HEAD_JOINT + 1) + 3;
    if (!ok) {
        char msg[256];
        snprintf(msg, sizeof(msg), "head_rot_cost: layout %d with F = %d: expected SEEME_STITCH_ANGLE (0) with F = J x 3, "
                 "SEEME_STITCH_ANGLE_TRANSL (1) with F = J x 3 + 3 (J >= 16), or SEEME_STITCH_ROT6D (2) with F = 144", layout, F);
        return seeme_fail(msg);
    }
    if (!feats || !dev_quat || !lengths || !cost) return seeme_fail("head_rot_cost: null pointer");
    if (((uintptr_t)feats | (uintptr_t)dev_quat | (uintptr_t)lengths | (uintptr_t)cost | (uintptr_t)angle) & 3)
        return seeme_fail("head_rot_cost: every pointer must be 4-byte aligned");
    const int WK = W * K;
    hipLaunchKernelGGL(k_head_rot_cost, dim3((WK + HS_WAVES - 1) / HS_WAVES), dim3(HS_THREADS), 0, (hipStream_t)stream, feats,
                       layout == SEEME_STITCH_ROT6D ? 1 : 0, F, dev_quat, lengths, WK, K, T, cost, angle);
    return seeme_check_launch("k_head_rot_cost");
}

// ------------------------------------------------------------------ anchoring the stitched motion to the device's path
// Partition: one workgroup per HS_THREADS output frames n0 .. n0+255; its halo is the 256 + 2R frames n0-R .. n0+255+R, of which those
// inside 0..L-1 exist.  Step 1, one lane per halo frame: r = path - head into LDS (rows of 3 floats: a stride coprime to the banks).
// Step 2, one lane per output frame: the taps over the LDS rows in increasing frame order, the sum of the taps beside them.
struct HsTaps { float t[HS_RMAX + 1]; };

__global__ __launch_bounds__(HS_THREADS) void k_head_anchor(const float* __restrict__ joints, const float* __restrict__ path, int L,
                                                            HsTaps taps, int R, float* __restrict__ shift, float* __restrict__ residual) {
    __shared__ float rr[HS_NF][3];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * HS_THREADS, m0 = n0 - R;              // halo row f is frame m0 + f
    const int nf = HS_THREADS + 2 * R;
    for (int f = tid; f < nf; f += HS_THREADS) {
        const int m = m0 + f;
        if (m < 0 || m >= L) continue;
        const float* h = joints + (size_t)m * HS_ROW + HS_HEAD;
        const float* p = path + (size_t)m * 3;
        rr[f][0] = p[0] - h[0]; rr[f][1] = p[1] - h[1]; rr[f][2] = p[2] - h[2];
    }
    __syncthreads();
    const int n = n0 + tid;
    if (n >= L) return;
    const int fc = tid + R;                                           // the output frame's own halo row
    float ax = 0.f, ay = 0.f, az = 0.f, ws = 0.f;
    for (int d = -R; d <= R; ++d) {                                   // increasing frame order; the tap index is uniform over the lanes
        const int m = n + d;
        if (m < 0 || m >= L) continue;
        const float k = taps.t[d < 0 ? -d : d];
        ws += k;
        ax += k * rr[fc + d][0]; ay += k * rr[fc + d][1]; az += k * rr[fc + d][2];
    }
    const float qx = ax / ws, qy = ay / ws, qz = az / ws;
    shift[(size_t)n * 3] = qx; shift[(size_t)n * 3 + 1] = qy; shift[(size_t)n * 3 + 2] = qz;
    const float ex = rr[fc][0] - qx, ey = rr[fc][1] - qy, ez = rr[fc][2] - qz;
    residual[n] = 1000.f * sqrtf(ex * ex + ey * ey + ez * ez);
}

extern "C" int seeme_head_anchor(const float* joints, const float* path, int L, const float* taps_host, int R, float* shift,
                                 float* residual, void* stream) {
    if (L < 1 || L > (1 << 20)) return seeme_fail("head_anchor: L must be in 1..2^20");
    if (R < 0 || R > HS_RMAX) return seeme_fail("head_anchor: R must be in 0..30");
    if (!joints || !path || !taps_host || !shift || !residual) return seeme_fail("head_anchor: null pointer");
    if (((uintptr_t)joints | (uintptr_t)path | (uintptr_t)shift | (uintptr_t)residual) & 3)
        return seeme_fail("head_anchor: every pointer must be 4-byte aligned");
    HsTaps taps;
    for (int d = 0; d <= HS_RMAX; ++d) taps.t[d] = 0.f;
    for (int d = 0; d <= R; ++d) {
        const float t = taps_host[d];
        if (!isfinite(t) || t < 0.f) return seeme_fail("head_anchor: every tap must be finite and >= 0");
        taps.t[d] = t;
    }
    if (!(taps.t[0] > 0.f)) return seeme_fail("head_anchor: taps[0] must be > 0");
    const int blocks = (L + HS_THREADS - 1) / HS_THREADS;
    hipLaunchKernelGGL(k_head_anchor, dim3(blocks), dim3(HS_THREADS), 0, (hipStream_t)stream, joints, path, L, taps, R, shift, residual);
    return seeme_check_launch("k_head_anchor");
}
