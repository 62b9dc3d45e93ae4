// social_metrics.hip -- the interaction between the camera wearer and the interactee, per sequence and per hypothesis: pelvis-to-pelvis
// distance, closest approach of the two bodies and the angle between their gaze directions, for the reference body (what the
// evaluation is binned by) and for each of the K hypotheses (how well a hypothesis reproduces the interaction).
//
// Definitions: include/seeme_hip.h (seeme_social_metrics).  No alignment of any kind: the two people share the batch's frame.
//
// Partition: one workgroup (256 lanes) per (sequence b, chunk of SEEME_SOCIAL_FRAME_CHUNK frames); the chunk size is a constant, so a
// sequence's values do not depend on B.  A frame's K hypotheses, the reference (row K) and the interactee (row K+1) live in LDS as
// [K+2] rows of 72 floats, loaded as float4 (rows are 288 B); two slots, the next frame's loads in flight while the current one is
// reduced.  Work items (body row, joint i) are dealt over the lanes: an item takes the minimum of the SQUARED distance over the
// interactee's 24 joints (read as broadcasts) and the root of that -- sqrtf is monotone and correctly rounded, so this is the minimum
// of the distances, bit for bit, and a minimum is exact in any order.  Lane r <= K then reduces row r's 24 minima, takes the pelvis
// distance and does the row's quaternion work; the three values of every row pass through LDS, so that the reference's values are
// computed ONCE (a hypothesis posed with the reference orientation has a gaze-angle error of exactly 0).  Lane k < K sums its five
// numbers over the chunk's frames in frame order, lane K the reference's three, and they go to the workspace as 5K+3 partial sums.
// A second small launch adds a sequence's chunks in chunk order and normalises.  No atomics: bitwise reproducible.
#include "api_util.hpp"
#include <stdint.h>

#define SOC_KMAX 32
#define SOC_NJ 24
#define SOC_ROW 72                 // 24 joints x 3 floats = 288 B = 18 float4
#define SOC_Q 18
#define SOC_THREADS 256
#define SOC_FC SEEME_SOCIAL_FRAME_CHUNK
#define SOC_NLD (((SOC_KMAX + 2) * SOC_Q + SOC_THREADS - 1) / SOC_THREADS)        // float4 loads of one frame per lane (3)
#define SOC_NIT (((SOC_KMAX + 1) * SOC_NJ + SOC_THREADS - 1) / SOC_THREADS)       // (row, joint) items per lane (4)
#define SOC_CST (SOC_NJ + 1)       // stride of a row's 24 minima: odd, so the K+1 lanes that reduce them sit on distinct banks
#define SOC_NHYP 5
#define SOC_NSEQ 3

// gaze direction: third column of the rotation matrix of q = (w,x,y,z), normalised as EgoMetrics.quat_to_rotmat does it
// (q * sqrt(2 / |q|^2)); |q|^2 < 1e-15 is the identity.  No contraction into fused multiply-adds: the compiler would otherwise fuse
// the two inlined copies (own and interactee's quaternion) differently, and equal rotations would not give equal bits.
__device__ __forceinline__ void soc_gaze(const float4 q, float g[3]) {
#pragma clang fp contract(off)
    const float w = q.x, x = q.y, y = q.z, z = q.w;
    const float n = w * w + x * x + y * y + z * z;
    if (n < 1e-15f) { g[0] = 0.f; g[1] = 0.f; g[2] = 1.f; return; }
    const float s = 2.0f / n;
    g[0] = s * (x * z + y * w);
    g[1] = s * (y * z - x * w);
    g[2] = 1.0f - s * (x * x + y * y);
}

// angle between two gaze directions in degrees, in [0, 180]: atan2(|g x h|, g . h).  Every product of the cross product is rounded
// on its own (contraction into a fused multiply-add is switched off for this function), so that parallel and antiparallel directions give a cross product of exactly 0.
__device__ __forceinline__ float soc_angle(const float g[3], const float h[3]) {
#pragma clang fp contract(off)
    const float cx = g[1] * h[2] - g[2] * h[1];
    const float cy = g[2] * h[0] - g[0] * h[2];
    const float cz = g[0] * h[1] - g[1] * h[0];
    const float cn = sqrtf(cx * cx + cy * cy + cz * cz);
    const float dt = g[0] * h[0] + g[1] * h[1] + g[2] * h[2];
    return fminf(atan2f(cn, dt) * 57.29577951308232f, 180.0f);
}

__global__ __launch_bounds__(SOC_THREADS) void k_social_partial(const float* __restrict__ pred, const float* __restrict__ ref,
                                                                const float* __restrict__ intr, const float* __restrict__ qpred,
                                                                const float* __restrict__ qref, const float* __restrict__ qint,
                                                                const int32_t* __restrict__ lengths, int K, int T,
                                                                float* __restrict__ slab) {
    __shared__ __attribute__((aligned(16))) float rows[2][SOC_KMAX + 2][SOC_ROW];   // row K the reference, row K+1 the interactee
    __shared__ float cmin[(SOC_KMAX + 1) * SOC_CST];     // closest interactee joint of every (row, joint)
    __shared__ float rowv[3][SOC_KMAX + 1];              // d, c, a of every body row

    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x, NC = gridDim.x;
    const int W = SOC_NHYP * K + SOC_NSEQ;
    const int len = lengths[b];
    const int nvalid = len < 0 ? 0 : (len > T ? T : len);
    const int t0 = chunk * SOC_FC, t1 = min(t0 + SOC_FC, nvalid);
    float* out = slab + ((size_t)b * NC + chunk) * W;
    if (t0 >= nvalid) {                                  // nothing valid here: the workspace is not zeroed by anyone else
        for (int i = tid; i < W; i += SOC_THREADS) out[i] = 0.f;
        return;
    }
    const float* predb = pred + (size_t)b * K * T * SOC_ROW;
    const float* refb = ref + (size_t)b * T * SOC_ROW;
    const float* intb = intr + (size_t)b * T * SOC_ROW;
    const float4* qrow = (const float4*)(tid < K ? qpred + ((size_t)b * K + tid) * T * 4 : qref + (size_t)b * T * 4);
    const float4* qintb = (const float4*)(qint + (size_t)b * T * 4);
    const int nld = (K + 2) * SOC_Q, nit = (K + 1) * SOC_NJ;

    static_assert(SOC_NLD == 3, "issue() and commit() spell out three float4 loads per lane");
    float4 v0, v1, v2, qv = make_float4(1.f, 0.f, 0.f, 0.f), qi = qv;
    v0 = v1 = v2 = qv;
    auto ld = [&](int e, int f, float4& v) {
        if (e < nld) {
            const int row = e / SOC_Q, q = e - row * SOC_Q;
            const float* base = row < K ? predb + (size_t)row * T * SOC_ROW : (row == K ? refb : intb);
            v = ((const float4*)(base + (size_t)f * SOC_ROW))[q];
        }
    };
    auto st = [&](int e, int slot, const float4& v) {
        if (e < nld) {
            const int row = e / SOC_Q, q = e - row * SOC_Q;
            *(float4*)&rows[slot][row][q * 4] = v;
        }
    };
    auto issue = [&](int f) {
        ld(tid, f, v0); ld(tid + SOC_THREADS, f, v1); ld(tid + 2 * SOC_THREADS, f, v2);
        if (tid <= K) { qv = qrow[f]; qi = qintb[f]; }
    };
    auto commit = [&](int slot) {
        st(tid, slot, v0); st(tid + SOC_THREADS, slot, v1); st(tid + 2 * SOC_THREADS, slot, v2);
    };

    float acc[SOC_NHYP];
#pragma unroll
    for (int i = 0; i < SOC_NHYP; ++i) acc[i] = 0.f;

    issue(t0);
    for (int f = t0; f < t1; ++f) {
        const int s = (f - t0) & 1;
        commit(s);
        const float4 qf = qv, qif = qi;                           // this frame's quaternions: issue() overwrites qv / qi
        __syncthreads();                                          // slot s complete; every lane is done with slot s^1 (frame f-1)
        if (f + 1 < t1) issue(f + 1);
        const float* in = rows[s][K + 1];
#pragma unroll
        for (int r = 0; r < SOC_NIT; ++r) {
            const int e = tid + r * SOC_THREADS;
            if (e < nit) {
                const int row = e / SOC_NJ, i = e - row * SOC_NJ;
                const float x = rows[s][row][3 * i], y = rows[s][row][3 * i + 1], z = rows[s][row][3 * i + 2];
                float m = __builtin_inff();
#pragma unroll 8
                for (int j3 = 0; j3 < SOC_ROW; j3 += 3) {
                    const float ex = x - in[j3], ey = y - in[j3 + 1], ez = z - in[j3 + 2];
                    m = fminf(m, ex * ex + ey * ey + ez * ez);
                }
                cmin[row * SOC_CST + i] = sqrtf(m);
            }
        }
        __syncthreads();
        if (tid <= K) {
            float c = cmin[tid * SOC_CST];
            for (int j = 1; j < SOC_NJ; ++j) c = fminf(c, cmin[tid * SOC_CST + j]);
            const float dx = rows[s][tid][0] - in[0], dy = rows[s][tid][1] - in[1], dz = rows[s][tid][2] - in[2];
            float g[3], h[3];
            soc_gaze(qf, g);
            soc_gaze(qif, h);
            rowv[0][tid] = sqrtf(dx * dx + dy * dy + dz * dz);
            rowv[1][tid] = c;
            rowv[2][tid] = soc_angle(g, h);
        }
        __syncthreads();
        if (tid < K) {
            const float d = rowv[0][tid], c = rowv[1][tid], a = rowv[2][tid];
            acc[0] += fabsf(d - rowv[0][K]);
            acc[1] += c;
            acc[2] += fabsf(c - rowv[1][K]);
            acc[3] += a;
            acc[4] += fabsf(a - rowv[2][K]);
        } else if (tid == K) {
            acc[0] += rowv[0][K];
            acc[1] += rowv[1][K];
            acc[2] += rowv[2][K];
        }
        // (rowv and cmin are next written after the following frame's barriers)
    }
    if (tid < K) {
#pragma unroll
        for (int m = 0; m < SOC_NHYP; ++m) out[m * K + tid] = acc[m];
    } else if (tid == K) {
#pragma unroll
        for (int m = 0; m < SOC_NSEQ; ++m) out[SOC_NHYP * K + m] = acc[m];
    }
}

// chunks of a sequence in chunk order (one lane per partial sum), then the mean over the nvalid frames; metres -> mm for the distances
__global__ __launch_bounds__(192) void k_social_final(const float* __restrict__ slab, const int32_t* __restrict__ lengths, int B, int K,
                                                      int T, int NC, float* __restrict__ per_hyp, float* __restrict__ per_seq) {
    const int b = blockIdx.x, v = threadIdx.x, W = SOC_NHYP * K + SOC_NSEQ;
    if (v >= W) return;
    const float* s = slab + (size_t)b * NC * W + v;
    float x = 0.f;
#pragma unroll 4
    for (int c = 0; c < NC; ++c) x += s[(size_t)c * W];
    const int len = lengths[b];
    const int nvalid = len < 0 ? 0 : (len > T ? T : len);
    const float y = nvalid > 0 ? x / (float)nvalid : 0.f;
    if (v < SOC_NHYP * K) {
        const int m = v / K, k = v - m * K;
        per_hyp[((size_t)m * B + b) * K + k] = m < 3 ? y * 1000.f : y;
    } else {
        const int w = v - SOC_NHYP * K;
        per_seq[(size_t)w * B + b] = w < 2 ? y * 1000.f : y;
    }
}

extern "C" size_t seeme_social_metrics_workspace_bytes(int B, int K, int T) {
    if (B < 1 || K < 1 || K > SOC_KMAX || T < 1) return 0;
    return (size_t)B * ((T + SOC_FC - 1) / SOC_FC) * (SOC_NHYP * K + SOC_NSEQ) * sizeof(float);
}

extern "C" int seeme_social_metrics(const float* jts_pred, const float* jts_ref, const float* jts_int, const float* quat_pred,
                                    const float* quat_ref, const float* quat_int, const int32_t* lengths, int B, int K, int T,
                                    float* per_hyp, float* per_seq, void* ws, size_t ws_bytes, void* stream) {
    if (B < 1 || B > 65535) return seeme_fail("social_metrics: B must be in 1..65535");
    if (K < 1 || K > SOC_KMAX) return seeme_fail("social_metrics: K must be in 1..32");
    if (T < 1) return seeme_fail("social_metrics: T must be >= 1");
    if (!jts_pred || !jts_ref || !jts_int || !quat_pred || !quat_ref || !quat_int || !lengths || !per_hyp || !per_seq || !ws)
        return seeme_fail("social_metrics: null pointer");
    if (((uintptr_t)jts_pred | (uintptr_t)jts_ref | (uintptr_t)jts_int | (uintptr_t)quat_pred | (uintptr_t)quat_ref |
         (uintptr_t)quat_int) & 15)
        return seeme_fail("social_metrics: joints and quaternions must be 16-byte aligned");
    if (((uintptr_t)lengths | (uintptr_t)per_hyp | (uintptr_t)per_seq | (uintptr_t)ws) & 3)
        return seeme_fail("social_metrics: lengths, outputs and workspace must be 4-byte aligned");
    if (ws_bytes < seeme_social_metrics_workspace_bytes(B, K, T)) return seeme_fail("social_metrics: workspace too small");
    const int NC = (T + SOC_FC - 1) / SOC_FC;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_social_partial, dim3(NC, B), dim3(SOC_THREADS), 0, st, jts_pred, jts_ref, jts_int, quat_pred, quat_ref,
                       quat_int, lengths, K, T, (float*)ws);
    if (int rc = seeme_check_launch("k_social_partial")) return rc;
    hipLaunchKernelGGL(k_social_final, dim3(B), dim3(192), 0, st, (const float*)ws, lengths, B, K, T, NC, per_hyp, per_seq);
    return seeme_check_launch("k_social_final");
}
