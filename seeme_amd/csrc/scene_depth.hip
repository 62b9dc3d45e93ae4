// scene_depth.hip -- the body against the scene, per candidate frame: how deep the capsules round a hypothesis' bones reach into the
// scene's points (seeme_scene_depth: depth per frame, and its mean and the count of penetrating frames per hypothesis, a unary term of
// seeme_path_select).  Definition: include/seeme_hip.h; the plain-torch twin is seeme_amd/recording.py scene_depth_torch.  fp32.
// depth is a maximum, exact and free of order, of values that ONE expression (sd_pair, called from one place) computes; everything
// else in this file only decides which triples are skipped, and skips none whose computed value is > 0.
#include "api_util.hpp"
#include <math.h>
#include <stdint.h>

#define SD_NBMAX SEEME_SCENE_DEPTH_NBMAX
#define SD_FC SEEME_SCENE_DEPTH_CHUNK        // frames of one workgroup
#define SD_THREADS 256
#define SD_WAVES (SD_THREADS / 64)
#define SD_RING 512                          // slots of the point queue: fewer than SD_THREADS wait, at most SD_THREADS arrive
#define SD_PER 4                             // points a thread has in flight per tile of the cloud
#define SD_TILE (SD_THREADS * SD_PER)
// The margin of the boxes.  Claim: a triple whose computed value radius[b] - dist is > 0 has its point inside the frame's box, the
// box of the joints the segments name grown by rmax + margin.  With s in [0,1] (clamped, exact) the real point a + s (c - a) lies in
// the joints' box, and the computed v differs from p - (a + s (c - a)) per coordinate by the roundings of c - a, p - a, s e and
// q - s e: under 8 x 2^-24 x (the largest difference of two coordinates involved).  A value > 0 means |v| <= dist < rmax, so those
// differences stay below 2 (M + rmax), M the largest |coordinate| of the box: the error is below 1e-6 (M + rmax), and the
// square root adds 3 x 2^-24 rmax.  margin = 1 mm + 1e-5 (M + rmax) is ten times that plus a millimetre, which also covers the
// rounding of the grown box itself (one ulp of M).  A chunk's box is the union of its frames' boxes.
#define SD_MARGIN_ABS 1e-3f
#define SD_MARGIN_REL 1e-5f

struct SdTable { float radius[SD_NBMAX]; int s0[SD_NBMAX], s1[SD_NBMAX]; };

// radius - distance of p from the segment a .. a + e.  t0 = (a.x, a.y, a.z, e.x), t1 = (e.y, e.z, ee > 0 ? 1 / ee : 0, radius).
// fmaxf / fminf return the operand that is not a NaN: 0 x inf (a subnormal ee) gives s = 0.
__device__ __forceinline__ float sd_pair(float px, float py, float pz, float4 t0, float4 t1) {
    const float qx = px - t0.x, qy = py - t0.y, qz = pz - t0.z;
    const float qe = fmaf(qz, t1.y, fmaf(qy, t1.x, qx * t0.w));
    const float s = fminf(fmaxf(qe * t1.z, 0.f), 1.f);
    const float vx = fmaf(-s, t0.w, qx), vy = fmaf(-s, t1.x, qy), vz = fmaf(-s, t1.y, qz);
    return t1.w - sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx)));
}

// Partition: one workgroup per chunk of SD_FC consecutive frames of one (w,k); blockIdx.x = w K + k, blockIdx.y = the chunk.
//  1. lane = frame, wave = segment (b = wave, wave + 4, ..): (a, e, 1/ee, radius) of every (segment, frame) into LDS, 32 B each, and
//     the box of the joints named; then the frames' grown boxes and the chunk's.
//  2. the cloud streams through the workgroup once, SD_TILE points per round with the next round's loads in flight; a point inside
//     the chunk's box goes into the ring (wave ballot, the four waves' counts through LDS: no atomics, a fixed order).  With
//     SD_THREADS points waiting the ring is drained: nothing is dropped and there is no cap, all N may pass.
//  3. draining: one lane per queued point, the frame index uniform over the workgroup; a point inside the frame's box meets the NB
//     segments (LDS reads of one address: broadcasts), and a lane with a value > 0 raises the frame's maximum in LDS with an integer
//     max (a non-negative float keeps its order as an unsigned integer).
__global__ __launch_bounds__(SD_THREADS) void k_scene_depth(const float* __restrict__ jts, const int32_t* __restrict__ lengths,
                                                            const float* __restrict__ points, int K, int T, int J, int N,
                                                            SdTable tab, int NB, float rmax, float* __restrict__ depth) {
    __shared__ float4 s_tab[SD_NBMAX * SD_FC * 2];
    __shared__ float s_pbox[SD_WAVES][SD_FC][6];
    __shared__ float s_fbox[SD_FC][6];
    __shared__ float s_cbox[6];
    __shared__ float s_q[3][SD_RING];
    __shared__ unsigned s_dmax[SD_FC];
    __shared__ int s_wcnt[2][SD_WAVES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = blockIdx.x, t0 = blockIdx.y * SD_FC;
    const int n = min(max(lengths[wk / K], 0), T);
    const int nf = min(max(n - t0, 0), SD_FC);                         // frames of this chunk that exist
    float* out = depth + (size_t)wk * T + t0;
    if (nf == 0) {                                                      // (uniform over the workgroup)
        if (tid < min(SD_FC, T - t0)) out[tid] = 0.f;
        return;
    }
    const float inf = __builtin_inff();

    // ---- 1. the segments of the chunk's frames
    {
        float lx = inf, ly = inf, lz = inf, hx = -inf, hy = -inf, hz = -inf;
        if (lane < nf) {
            const float* fr = jts + ((size_t)wk * T + t0 + lane) * J * 3;
            for (int b = wave; b < NB; b += SD_WAVES) {
                const float* pa = fr + tab.s0[b] * 3;
                const float* pc = fr + tab.s1[b] * 3;
                const float ax = pa[0], ay = pa[1], az = pa[2], cx = pc[0], cy = pc[1], cz = pc[2];
                const float ex = cx - ax, ey = cy - ay, ez = cz - az;
                const float ee = fmaf(ez, ez, fmaf(ey, ey, ex * ex));
                s_tab[(b * SD_FC + lane) * 2] = make_float4(ax, ay, az, ex);
                s_tab[(b * SD_FC + lane) * 2 + 1] = make_float4(ey, ez, ee > 0.f ? 1.f / ee : 0.f, tab.radius[b]);
                lx = fminf(lx, fminf(ax, cx)); ly = fminf(ly, fminf(ay, cy)); lz = fminf(lz, fminf(az, cz));
                hx = fmaxf(hx, fmaxf(ax, cx)); hy = fmaxf(hy, fmaxf(ay, cy)); hz = fmaxf(hz, fmaxf(az, cz));
            }
        }
        if (lane < SD_FC) {
            float* pb = s_pbox[wave][lane];
            pb[0] = lx; pb[1] = ly; pb[2] = lz; pb[3] = hx; pb[4] = hy; pb[5] = hz;
        }
    }
    __syncthreads();
    if (tid < SD_FC) {
        float bx[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            bx[c] = fminf(fminf(s_pbox[0][tid][c], s_pbox[1][tid][c]), fminf(s_pbox[2][tid][c], s_pbox[3][tid][c]));
            bx[c + 3] = fmaxf(fmaxf(s_pbox[0][tid][c + 3], s_pbox[1][tid][c + 3]), fmaxf(s_pbox[2][tid][c + 3], s_pbox[3][tid][c + 3]));
        }
        float M = 0.f;
#pragma unroll
        for (int c = 0; c < 6; ++c) M = fmaxf(M, fabsf(bx[c]));
        const float pad = rmax + (SD_MARGIN_ABS + SD_MARGIN_REL * (M + rmax));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s_fbox[tid][c] = bx[c] - pad;
            s_fbox[tid][c + 3] = bx[c + 3] + pad;
        }
        s_dmax[tid] = 0u;
    }
    __syncthreads();
    if (tid < 6) {
        float v = s_fbox[0][tid];
        for (int f = 1; f < nf; ++f) v = tid < 3 ? fminf(v, s_fbox[f][tid]) : fmaxf(v, s_fbox[f][tid]);
        s_cbox[tid] = v;
    }
    __syncthreads();
    const float c0 = s_cbox[0], c1 = s_cbox[1], c2 = s_cbox[2], c3 = s_cbox[3], c4 = s_cbox[4], c5 = s_cbox[5];

    // ---- 3. (used by 2.) the first cnt <= SD_THREADS queued points against the chunk's frames
    int head = 0, tail = 0, par = 0;                                    // the same on every thread
    auto drain = [&](int cnt) {
        if (tid >= cnt) return;
        const int slot = (head + tid) & (SD_RING - 1);
        const float px = s_q[0][slot], py = s_q[1][slot], pz = s_q[2][slot];
        for (int f = 0; f < nf; ++f) {
            const float* fb = s_fbox[f];
            if (px >= fb[0] && px <= fb[3] && py >= fb[1] && py <= fb[4] && pz >= fb[2] && pz <= fb[5]) {
                float m = 0.f;
                for (int b = 0; b < NB; ++b)
                    m = fmaxf(m, sd_pair(px, py, pz, s_tab[(b * SD_FC + f) * 2], s_tab[(b * SD_FC + f) * 2 + 1]));
                if (m > 0.f) atomicMax(&s_dmax[f], __float_as_uint(m));
            }
        }
    };
    // ---- 2. one point per thread: into the ring when it is inside the chunk's box (a NaN is not); a full ring is drained
    auto step = [&](float x, float y, float z, bool have) {
        const bool in = have && x >= c0 && x <= c3 && y >= c1 && y <= c4 && z >= c2 && z <= c5;
        const unsigned long long bal = __ballot(in);
        if (lane == 0) s_wcnt[par][wave] = __popcll(bal);
        __syncthreads();
        const int n0 = s_wcnt[par][0], n1 = s_wcnt[par][1], n2 = s_wcnt[par][2], n3 = s_wcnt[par][3];
        if (in) {
            const int before = (wave > 0 ? n0 : 0) + (wave > 1 ? n1 : 0) + (wave > 2 ? n2 : 0);
            const int slot = (tail + before + __popcll(bal & ((1ull << lane) - 1ull))) & (SD_RING - 1);
            s_q[0][slot] = x; s_q[1][slot] = y; s_q[2][slot] = z;
        }
        tail += n0 + n1 + n2 + n3;
        par ^= 1;
        if (tail - head >= SD_THREADS) {                                // (uniform) the slots drained here are written again only
            __syncthreads();                                            // after the next step's barrier, which every wave reaches
            drain(SD_THREADS);                                          // after its part of the drain
            head += SD_THREADS;
        }
    };
    float cx[SD_PER], cy[SD_PER], cz[SD_PER], nx[SD_PER], ny[SD_PER], nz[SD_PER];
#pragma unroll
    for (int j = 0; j < SD_PER; ++j) {
        const int i = j * SD_THREADS + tid;
        cx[j] = cy[j] = cz[j] = 0.f;
        if (i < N) { cx[j] = points[i * 3]; cy[j] = points[i * 3 + 1]; cz[j] = points[i * 3 + 2]; }
    }
    for (int tile = 0; tile < N; tile += SD_TILE) {
#pragma unroll
        for (int j = 0; j < SD_PER; ++j) {                              // the next round's points: in flight during this round
            const int i = tile + SD_TILE + j * SD_THREADS + tid;
            nx[j] = ny[j] = nz[j] = 0.f;
            if (i < N) { nx[j] = points[i * 3]; ny[j] = points[i * 3 + 1]; nz[j] = points[i * 3 + 2]; }
        }
#pragma unroll
        for (int j = 0; j < SD_PER; ++j) step(cx[j], cy[j], cz[j], tile + j * SD_THREADS + tid < N);
#pragma unroll
        for (int j = 0; j < SD_PER; ++j) { cx[j] = nx[j]; cy[j] = ny[j]; cz[j] = nz[j]; }
    }
    __syncthreads();
    drain(tail - head);
    __syncthreads();
    if (tid < min(SD_FC, T - t0)) out[tid] = tid < nf ? 1000.f * __uint_as_float(s_dmax[tid]) : 0.f;
}

// cost and hits of one (w,k) from its depths: one wave each, a lane adds its frames t = lane, lane + 64, ... < n in increasing t, the
// 64 partial sums meet in a butterfly (the same tree on every lane).
__global__ __launch_bounds__(SD_THREADS) void k_scene_cost(const float* __restrict__ depth, const int32_t* __restrict__ lengths, int WK,
                                                           int K, int T, float* __restrict__ cost, int32_t* __restrict__ hits) {
    const int lane = threadIdx.x & 63;
    const int wk = blockIdx.x * SD_WAVES + (threadIdx.x >> 6);         // uniform over the wave
    if (wk >= WK) return;
    const int n = min(max(lengths[wk / K], 0), T);
    const float* d = depth + (size_t)wk * T;
    float s = 0.f;
    int h = 0;
    for (int t = lane; t < n; t += 64) {
        const float v = d[t];
        s += v;
        h += v > 0.f ? 1 : 0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s += __shfl_xor(s, m);
        h += __shfl_xor(h, m);
    }
    if (lane == 0) {
        cost[wk] = n > 0 ? s / (float)n : 0.f;
        hits[wk] = h;
    }
}

extern "C" int seeme_scene_depth(const float* jts, const int32_t* lengths, const float* points, int W, int K, int T, int J, int N,
                                 const int32_t* segs_host, const float* radius_host, int NB, float* depth, float* cost, int32_t* hits,
                                 void* stream) {
    if (W < 1 || W > 65536) return seeme_fail("scene_depth: W must be in 1..65536");
    if (K < 1 || K > 32) return seeme_fail("scene_depth: K must be in 1..32");
    if (T < 1 || T > (1 << 20)) return seeme_fail("scene_depth: T must be in 1..2^20");
    if (J < 1 || J > 32) return seeme_fail("scene_depth: J must be in 1..32");
    if (N < 1 || N > (1 << 24)) return seeme_fail("scene_depth: N must be in 1..2^24");
    if (NB < 1 || NB > SD_NBMAX) return seeme_fail("scene_depth: NB must be in 1..32");
    if (!jts || !lengths || !points || !segs_host || !radius_host || !depth || !cost || !hits)
        return seeme_fail("scene_depth: null pointer");
    if (((uintptr_t)jts | (uintptr_t)lengths | (uintptr_t)points | (uintptr_t)depth | (uintptr_t)cost | (uintptr_t)hits) & 3)
        return seeme_fail("scene_depth: every pointer must be 4-byte aligned");
    const int chunks = (T + SD_FC - 1) / SD_FC;
    if ((long long)W * K * chunks >= (1ll << 24)) return seeme_fail("scene_depth: W x K x ceil(T / 32) must be below 2^24");
    SdTable tab;
    float rmax = 0.f;
    for (int b = 0; b < SD_NBMAX; ++b) {
        tab.radius[b] = 0.f;
        tab.s0[b] = tab.s1[b] = 0;
    }
    for (int b = 0; b < NB; ++b) {
        const int i0 = segs_host[2 * b], i1 = segs_host[2 * b + 1];
        const float r = radius_host[b];
        if (i0 < 0 || i0 >= J || i1 < 0 || i1 >= J) return seeme_fail("scene_depth: every segment index must be in 0..J-1");
        if (!isfinite(r) || r < 0.f) return seeme_fail("scene_depth: every radius must be finite and >= 0");
        tab.s0[b] = i0; tab.s1[b] = i1; tab.radius[b] = r;
        rmax = fmaxf(rmax, r);
    }
    const int WK = W * K;
    hipLaunchKernelGGL(k_scene_depth, dim3(WK, chunks), dim3(SD_THREADS), 0, (hipStream_t)stream, jts, lengths, points, K, T, J, N, tab,
                       NB, rmax, depth);
    if (int rc = seeme_check_launch("k_scene_depth")) return rc;
    hipLaunchKernelGGL(k_scene_cost, dim3((WK + SD_WAVES - 1) / SD_WAVES), dim3(SD_THREADS), 0, (hipStream_t)stream, depth, lengths, WK,
                       K, T, cost, hits);
    return seeme_check_launch("k_scene_cost");
}
