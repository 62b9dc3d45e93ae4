// mesh_metrics.hip -- per-frame mesh metrics of the K-hypothesis evaluation: Procrustes-aligned joint error (PA-MPJPE), per-vertex
// error (V2V) and the squared distance between the posed mesh and the scene cloud (contact).  Definitions: EgoHMR's
// test_egohmr.py:463-492 (PA-MPJPE through utils/pose_utils.py:11-59, V2V :485) and :540-549 (contact: k-NN `dists`, squared).
//
// All three are frame-level primitives: one output float per frame, a frame whose map entry is negative is skipped and gets 0, the
// host averages over the valid frames of a sequence.  No atomics; every reduction runs in a fixed order (sums) or is a min / max
// (exact, order-free), so the results are bitwise reproducible and a frame's value does not depend on the other frames of a launch.
//
// seeme_scene_min_dist2 is the hot one: V x P pairs per frame (6890 x 20 000 = 1.38e8).  It runs as a FILTER on the matrix cores
// followed by an exact re-evaluation of the few scene points that can hold the minimum:
//
//   k_scene_filter   one workgroup per (frame, slice of the scene).  Both operands are centred on the frame's centre c (the midpoint
//                    of the vertices' bounding box: the entry point takes no joints, and this is the centre with the smallest body
//                    radius; it stands in for the pelvis).  The expansion |v|^2 + |s|^2 - 2 v.s maps onto v_mfma_f32_16x16x4_f32:
//                      A row  (vertex)      = [-2vx, -2vy, -2vz, |v|^2]      (centred; 16 vertices per tile)
//                      B col  (scene point) = [  sx,   sy,   sz,    1  ]      (centred; 16 points per tile)
//                    so D[v][s] = |v|^2 - 2 v.s with a zero C: no accumulator chain, every MFMA is independent.  The frame's A
//                    tiles sit in LDS (V/16 tiles x 256 B = 110 KB for SMPL, laid out so that one ds_read_b128 per lane feeds four
//                    MFMAs); a wave holds four B tiles (64 scene points) in registers and walks all vertex tiles: 16 MFMAs per LDS
//                    read.  The lane's four results fold into its running min per scene point (v_minimum3_f32, hidden under the 32-cycle
//                    issue interval); |s|^2 is added after the min over the vertices.  Output: approx[f][p], the approximate min over
//                    the vertices of d^2 for every scene point, and per slice the min of approx + eps.
//   k_scene_exact    one workgroup per frame.  U = min over the slices = an upper bound of the true min.  Every scene point with
//                    approx[p] - eps_p <= U is a candidate and is evaluated against all V vertices in DIRECT form
//                    (dx^2 + dy^2 + dz^2 on the coordinates as given) by one wave, as it is found: there is no candidate buffer, so
//                    no cap the result could depend on.  out[f] = min of those values.
//
// The bound.  u = 2^-24.  Let |v|, |s| be the centred norms, |v| <= rv (the frame's largest).  approx differs from the real d^2 by
//   3u|v|^2 + 3u|s|^2     the two squared norms (three roundings each at most),
//   4u(2|v||s| + |v|^2)   the four fma steps of the MFMA chain, each partial result bounded by 2|v||s| + |v|^2,
//   u(|v| + |s|)^2        the final |s|^2 + min,
//   2u(|v| + |s|)^2       centring itself (one rounding per coordinate, first order in d <= |v| + |s|),
// in total <= 10u(|v| + |s|)^2; the direct form's own error is <= 4u d^2 <= 4u(|v| + |s|)^2.  eps_p = 16u (rv + |s_p|)^2 covers
// both, so the point whose direct-form value is the smallest always satisfies approx - eps <= real <= U and is a candidate: the output
// equals the min over ALL V x P pairs of the direct-form value.  eps is per point: near the body |s_p| ~ rv ~ 1 m and eps ~ 5e-6 m^2,
// while a far wall of the room does not widen the candidate set.  With one eps for all points the rule reads approx <= m + 2 eps.
#include "api_util.hpp"
#include <math.h>
#include <stdint.h>

typedef float mm_f32x4 __attribute__((ext_vector_type(4)));

#define MM_NJ 24
#define MM_THREADS 256
#define MM_BIG 1.0e30f
#define MM_INF __builtin_huge_valf()

// ----------------------------------------------------------------------------------------------------------------- PA-MPJPE
// One lane per frame.  The rotation is Horn's closed form: the unit quaternion of the best PROPER rotation is the eigenvector of the
// largest eigenvalue of a symmetric 4x4 matrix built from K = X1 X2^T.  That rotation is V diag(1, 1, sign det) U^T of
// pose_utils.py:39-45 (the reflection correction is built in: a mirrored prediction gets the best rotation, not the reflection).
// The eigenvectors come from cyclic Jacobi with a fixed number of sweeps: no data-dependent loop, so a degenerate frame cannot hang.
template <int P, int Q>
__device__ __forceinline__ void mm_jacobi_rotate(float (&a)[4][4], float (&v)[4][4]) {
    const float apq = a[P][Q];
    if (apq == 0.f) return;
    const float theta = (a[Q][Q] - a[P][P]) / (2.f * apq);
    const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const float arp = a[r][P], arq = a[r][Q];
            a[r][P] = a[P][r] = c * arp - s * arq;
            a[r][Q] = a[Q][r] = s * arp + c * arq;
        }
        const float vrp = v[r][P], vrq = v[r][Q];
        v[r][P] = c * vrp - s * vrq;
        v[r][Q] = s * vrp + c * vrq;
    }
}

__global__ __launch_bounds__(64) void k_pa_mpjpe(const float* __restrict__ jp, const float* __restrict__ jr,
                                                 const int32_t* __restrict__ ref_of_frame, int F, float* __restrict__ out) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    const int r = ref_of_frame[f];
    if (r < 0) { out[f] = 0.f; return; }
    const float* x = jp + (size_t)f * MM_NJ * 3;
    const float* y = jr + (size_t)r * MM_NJ * 3;
    float m1[3] = {0.f, 0.f, 0.f}, m2[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < MM_NJ; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { m1[c] += x[j * 3 + c]; m2[c] += y[j * 3 + c]; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { m1[c] /= (float)MM_NJ; m2[c] /= (float)MM_NJ; }
    float S[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, var1 = 0.f;      // S[a][b] = sum X1_a X2_b  (= K)
    for (int j = 0; j < MM_NJ; ++j) {
        float a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] = x[j * 3 + c] - m1[c]; b[c] = y[j * 3 + c] - m2[c]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            var1 += a[c] * a[c];
#pragma unroll
            for (int d = 0; d < 3; ++d) S[c][d] += a[c] * b[d];
        }
    }
    float n[4][4], v[4][4];
    n[0][0] = S[0][0] + S[1][1] + S[2][2];
    n[1][1] = S[0][0] - S[1][1] - S[2][2];
    n[2][2] = -S[0][0] + S[1][1] - S[2][2];
    n[3][3] = -S[0][0] - S[1][1] + S[2][2];
    n[0][1] = n[1][0] = S[1][2] - S[2][1];
    n[0][2] = n[2][0] = S[2][0] - S[0][2];
    n[0][3] = n[3][0] = S[0][1] - S[1][0];
    n[1][2] = n[2][1] = S[0][1] + S[1][0];
    n[1][3] = n[3][1] = S[2][0] + S[0][2];
    n[2][3] = n[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.f : 0.f;
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {
        mm_jacobi_rotate<0, 1>(n, v); mm_jacobi_rotate<0, 2>(n, v); mm_jacobi_rotate<0, 3>(n, v);
        mm_jacobi_rotate<1, 2>(n, v); mm_jacobi_rotate<1, 3>(n, v); mm_jacobi_rotate<2, 3>(n, v);
    }
    float best = n[0][0], q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        if (n[i][i] > best) {
            best = n[i][i];
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = v[c][i];
        }
    }
    const float qn = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float w = q[0] * qn, qx = q[1] * qn, qy = q[2] * qn, qz = q[3] * qn;
    float R[3][3];
    R[0][0] = 1.f - 2.f * (qy * qy + qz * qz); R[0][1] = 2.f * (qx * qy - qz * w); R[0][2] = 2.f * (qx * qz + qy * w);
    R[1][0] = 2.f * (qx * qy + qz * w); R[1][1] = 1.f - 2.f * (qx * qx + qz * qz); R[1][2] = 2.f * (qy * qz - qx * w);
    R[2][0] = 2.f * (qx * qz - qy * w); R[2][1] = 2.f * (qy * qz + qx * w); R[2][2] = 1.f - 2.f * (qx * qx + qy * qy);
    float tr = 0.f;                                        // trace(R K)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) tr += R[a][b] * S[b][a];
    const float scale = tr / var1;                         // var1 = 0 (all joints of the prediction equal): whatever IEEE gives
    float sum = 0.f;
    for (int j = 0; j < MM_NJ; ++j) {
        float a[3], e[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = x[j * 3 + c] - m1[c];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            e[c] = scale * (R[c][0] * a[0] + R[c][1] * a[1] + R[c][2] * a[2]) - (y[j * 3 + c] - m2[c]);
        sum += sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    }
    out[f] = sum / (float)MM_NJ;
}

// ----------------------------------------------------------------------------------------------------------------- V2V
// One workgroup per frame; tiles of 1024 vertices of the prediction and of its reference are staged in LDS with 16-byte loads (a
// frame of 6890 vertices starts on a 8-byte boundary only, so the tile is loaded from the 16-byte boundary below it and read back at
// its own offset; elements outside the frame are never touched).  A lane sums its vertices in index order, then lanes and waves are
// added in a fixed order.
#define V2V_TV 1024
#define V2V_LDS (3 * V2V_TV + 8)

__device__ __forceinline__ int mm_stage(const float* __restrict__ base, size_t e0, int cnt, float* lds, int tid) {
    const size_t ea = e0 & ~(size_t)3;
    const int sh = (int)(e0 - ea), nq = (sh + cnt + 3) >> 2;
    for (int q = tid; q < nq; q += MM_THREADS) {
        const size_t lo = ea + (size_t)q * 4;
        if (lo >= e0 && lo + 4 <= e0 + cnt) {
            ((float4*)lds)[q] = *(const float4*)(base + lo);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t idx = lo + i;
                lds[q * 4 + i] = (idx >= e0 && idx < e0 + cnt) ? base[idx] : 0.f;
            }
        }
    }
    return sh;
}

__global__ __launch_bounds__(MM_THREADS) void k_mesh_v2v(const float* __restrict__ vp, const float* __restrict__ pp,
                                                         const float* __restrict__ vr, const float* __restrict__ pr,
                                                         const int32_t* __restrict__ ref_of_frame, int V, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tp[V2V_LDS];
    __shared__ __attribute__((aligned(16))) float tr[V2V_LDS];
    __shared__ float red[MM_THREADS / 64];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int r = ref_of_frame[f];
    if (r < 0) {
        if (tid == 0) out[f] = 0.f;
        return;
    }
    const size_t ap = (size_t)f * V * 3, ar = (size_t)r * V * 3;
    const float p0 = pp[(size_t)f * 3], p1 = pp[(size_t)f * 3 + 1], p2 = pp[(size_t)f * 3 + 2];
    const float q0 = pr[(size_t)r * 3], q1 = pr[(size_t)r * 3 + 1], q2 = pr[(size_t)r * 3 + 2];
    float acc = 0.f;
    for (int n0 = 0; n0 < V; n0 += V2V_TV) {
        const int nv = min(V2V_TV, V - n0);
        const int shp = mm_stage(vp, ap + (size_t)n0 * 3, nv * 3, tp, tid);
        const int shr = mm_stage(vr, ar + (size_t)n0 * 3, nv * 3, tr, tid);
        __syncthreads();
        for (int j = tid; j < nv; j += MM_THREADS) {
            const float* a = tp + shp + 3 * j;
            const float* b = tr + shr + 3 * j;
            const float dx = (a[0] - p0) - (b[0] - q0), dy = (a[1] - p1) - (b[1] - q1), dz = (a[2] - p2) - (b[2] - q2);
            acc += sqrtf(dx * dx + dy * dy + dz * dz);
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int w = 0; w < MM_THREADS / 64; ++w) s += red[w];
        out[f] = s / (float)V;
    }
}

// ----------------------------------------------------------------------------------------------------------------- scene distance
#define SC_EPS (16.f * 5.9604645e-8f)       // 16 u, u = 2^-24: see the bound at the top of the file
#define SC_BLOCK 256                        // scene points per workgroup step: 4 waves x 4 B tiles x 16 points
#define SC_VMAX 10112                       // 158 groups of 64 vertices x 1 KiB = 158 KiB of LDS

// slices of the scene per frame: one when the frames alone fill the chip twice, otherwise enough to get there
static int scene_slices(int F, int P) {
    const int nblk = (P + SC_BLOCK - 1) / SC_BLOCK;
    const int want = (512 + F - 1) / F;
    return want < 1 ? 1 : (want > nblk ? nblk : want);
}

__device__ __forceinline__ float mm_wave_min(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ float mm_wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}

// IEEE-754-2019 minimum (NaN-propagating, v_minimum3_f32 on gfx950): unlike fminf it needs no canonicalisation of the MFMA results
// first, which would be four more VALU operations per MFMA
__device__ __forceinline__ float mm_fold(float run, mm_f32x4 d) {
    run = __builtin_elementwise_minimum(__builtin_elementwise_minimum(run, d[0]), d[1]);
    return __builtin_elementwise_minimum(__builtin_elementwise_minimum(run, d[2]), d[3]);
}

// (two waves per SIMD as the register budget: at most 256 VGPRs, which keeps the MFMA results in VGPRs and out of AGPRs)
__global__ __launch_bounds__(MM_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_scene_filter(
    const float* __restrict__ verts, const float* __restrict__ scene, const int32_t* __restrict__ scene_of_frame, int V, int S, int P,
    int NS, int NG, float* __restrict__ hdr, float* __restrict__ smin, float* __restrict__ approx) {
    extern __shared__ __attribute__((aligned(16))) float a_lds[];        // [NG][lane 64][4 tiles]: the A operands of the frame
    __shared__ float red[7][MM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x / NS, sl = blockIdx.x - f * NS;
    const int sc = scene_of_frame[f];
    if (sc < 0 || sc >= S) return;                                       // skipped frame (k_scene_exact writes its 0)
    const float* vf = verts + (size_t)f * V * 3;
    const float* sp = scene + (size_t)sc * P * 3;

    // the centre: midpoint of the bounding box (min and max are exact, so every slice of the frame gets the same bits)
    float lo0 = MM_INF, lo1 = MM_INF, lo2 = MM_INF, hi0 = -MM_INF, hi1 = -MM_INF, hi2 = -MM_INF;
    for (int n = tid; n < V; n += MM_THREADS) {
        const float x = vf[3 * n], y = vf[3 * n + 1], z = vf[3 * n + 2];
        lo0 = fminf(lo0, x); lo1 = fminf(lo1, y); lo2 = fminf(lo2, z);
        hi0 = fmaxf(hi0, x); hi1 = fmaxf(hi1, y); hi2 = fmaxf(hi2, z);
    }
    lo0 = mm_wave_min(lo0); lo1 = mm_wave_min(lo1); lo2 = mm_wave_min(lo2);
    hi0 = mm_wave_max(hi0); hi1 = mm_wave_max(hi1); hi2 = mm_wave_max(hi2);
    if (lane == 0) {
        red[0][wave] = lo0; red[1][wave] = lo1; red[2][wave] = lo2;
        red[3][wave] = hi0; red[4][wave] = hi1; red[5][wave] = hi2;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < MM_THREADS / 64; ++w) {
        lo0 = fminf(lo0, red[0][w]); lo1 = fminf(lo1, red[1][w]); lo2 = fminf(lo2, red[2][w]);
        hi0 = fmaxf(hi0, red[3][w]); hi1 = fmaxf(hi1, red[4][w]); hi2 = fmaxf(hi2, red[5][w]);
    }
    const float c0 = 0.5f * (lo0 + hi0), c1 = 0.5f * (lo1 + hi1), c2 = 0.5f * (lo2 + hi2);

    // A operands: vertex n = 16 t + r sits in tile t, row r; lane 16 k + r of the MFMA reads component k of it
    float maxw = 0.f;
    for (int n = tid; n < NG * 64; n += MM_THREADS) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = MM_BIG;                 // padding rows: D = 1e30, never the min
        if (n < V) {
            const float x = vf[3 * n] - c0, y = vf[3 * n + 1] - c1, z = vf[3 * n + 2] - c2;
            a3 = x * x + y * y + z * z;
            a0 = -2.f * x; a1 = -2.f * y; a2 = -2.f * z;
            maxw = fmaxf(maxw, a3);
        }
        const int t = n >> 4, r = n & 15, g = t >> 2, j = t & 3;
        float* dst = a_lds + ((g * 64 + r) * 4 + j);
        dst[0] = a0; dst[64] = a1; dst[128] = a2; dst[192] = a3;
    }
    maxw = mm_wave_max(maxw);
    if (lane == 0) red[6][wave] = maxw;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < MM_THREADS / 64; ++w) maxw = fmaxf(maxw, red[6][w]);
    const float rv = sqrtf(maxw);
    if (sl == 0 && tid == 0) {
        float* h = hdr + (size_t)f * 4;
        h[0] = c0; h[1] = c1; h[2] = c2; h[3] = rv;
    }

    const int nblk = (P + SC_BLOCK - 1) / SC_BLOCK;
    const int b0 = (int)((long)sl * nblk / NS), b1 = (int)((long)(sl + 1) * nblk / NS);
    const int k = lane >> 4, r = lane & 15;
    const float ck = k == 0 ? c0 : (k == 1 ? c1 : c2);
    const mm_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float4* a4 = (const float4*)a_lds + lane;
    float* apx = approx + (size_t)f * P;
    float ub = MM_INF;                                                   // min of approx + eps over this lane's points
    for (int blk = b0; blk < b1; ++blk) {
        const int base = blk * SC_BLOCK + wave * 64;
        if (base >= P) continue;                                         // wave-uniform
        float b[4], s2[4], run[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = base + j * 16 + r;
            float val = 0.f;
            if (p < P) val = k < 3 ? sp[(size_t)p * 3 + k] - ck : 1.f;
            b[j] = val;
            const float sq = k < 3 ? val * val : 0.f;
            s2[j] = (__shfl(sq, r, 64) + __shfl(sq, 16 + r, 64)) + __shfl(sq, 32 + r, 64);
            run[j] = 3.0e38f;
        }
        for (int g = 0; g < NG; ++g) {
            const float4 a = a4[g * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                run[j] = mm_fold(run[j], __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[j], zero, 0, 0, 0));
                run[j] = mm_fold(run[j], __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[j], zero, 0, 0, 0));
                run[j] = mm_fold(run[j], __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[j], zero, 0, 0, 0));
                run[j] = mm_fold(run[j], __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[j], zero, 0, 0, 0));
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float m = run[j];                                            // rows 4 (lane >> 4) + reg of every tile: fold the four lane groups
            m = fminf(m, __shfl_xor(m, 16, 64));
            m = fminf(m, __shfl_xor(m, 32, 64));
            const int p = base + j * 16 + r;
            if (lane < 16 && p < P) {
                const float ap = s2[j] + m;
                const float e = rv + sqrtf(s2[j]);
                apx[p] = ap;
                ub = fminf(ub, ap + SC_EPS * e * e);
            }
        }
    }
    ub = mm_wave_min(ub);
    __syncthreads();                                                     // red[0] is free again
    if (lane == 0) red[0][wave] = ub;
    __syncthreads();
    if (tid == 0) {
        float m = red[0][0];
        for (int w = 1; w < MM_THREADS / 64; ++w) m = fminf(m, red[0][w]);
        smin[(size_t)f * NS + sl] = m;
    }
}

__global__ __launch_bounds__(MM_THREADS) void k_scene_exact(const float* __restrict__ verts, const float* __restrict__ scene,
                                                            const int32_t* __restrict__ scene_of_frame, int V, int S, int P, int NS,
                                                            const float* __restrict__ hdr, const float* __restrict__ smin,
                                                            const float* __restrict__ approx, float* __restrict__ out) {
    __shared__ float red[MM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const int sc = scene_of_frame[f];
    if (sc < 0 || sc >= S) {
        if (tid == 0) out[f] = 0.f;
        return;
    }
    const float* vf = verts + (size_t)f * V * 3;
    const float* sp = scene + (size_t)sc * P * 3;
    const float* apx = approx + (size_t)f * P;
    float U = MM_INF;
    for (int i = 0; i < NS; ++i) U = fminf(U, smin[(size_t)f * NS + i]);
    const float c0 = hdr[(size_t)f * 4], c1 = hdr[(size_t)f * 4 + 1], c2 = hdr[(size_t)f * 4 + 2], rv = hdr[(size_t)f * 4 + 3];
    float best = MM_INF;
    for (int base = wave * 64; base < P; base += MM_THREADS) {           // wave-uniform trip count
        const int p = base + lane;
        bool cand = false;
        if (p < P) {
            const float x = sp[(size_t)p * 3] - c0, y = sp[(size_t)p * 3 + 1] - c1, z = sp[(size_t)p * 3 + 2] - c2;
            const float e = rv + sqrtf(x * x + y * y + z * z);
            cand = apx[p] - SC_EPS * e * e <= U;
        }
        unsigned long long m = __ballot(cand);
        while (m) {                                                      // the whole wave takes one candidate against all vertices
            const int i = __ffsll((long long)m) - 1;
            m &= m - 1;
            const size_t pc = (size_t)(base + i) * 3;
            const float sx = sp[pc], sy = sp[pc + 1], sz = sp[pc + 2];
            for (int n = lane; n < V; n += 64) {
                const float dx = vf[3 * n] - sx, dy = vf[3 * n + 1] - sy, dz = vf[3 * n + 2] - sz;
                best = fminf(best, dx * dx + dy * dy + dz * dz);
            }
        }
    }
    best = mm_wave_min(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (tid == 0) {
        float m = red[0];
        for (int w = 1; w < MM_THREADS / 64; ++w) m = fminf(m, red[w]);
        out[f] = m;
    }
}

// ----------------------------------------------------------------------------------------------------------------- C-ABI
extern "C" int seeme_pa_mpjpe_frames(const float* j_pred, const float* j_ref, const int32_t* ref_of_frame, int F, float* out,
                                     void* stream) {
    if (F < 1) return seeme_fail("pa_mpjpe_frames: F must be >= 1");
    if (!j_pred || !j_ref || !ref_of_frame || !out) return seeme_fail("pa_mpjpe_frames: null pointer");
    hipLaunchKernelGGL(k_pa_mpjpe, dim3((F + 63) / 64), dim3(64), 0, (hipStream_t)stream, j_pred, j_ref, ref_of_frame, F, out);
    return seeme_check_launch("k_pa_mpjpe");
}

extern "C" int seeme_mesh_v2v_frames(const float* v_pred, const float* pel_pred, const float* v_ref, const float* pel_ref,
                                     const int32_t* ref_of_frame, int F, int V, float* out, void* stream) {
    if (F < 1) return seeme_fail("mesh_v2v_frames: F must be >= 1");
    if (V < 1) return seeme_fail("mesh_v2v_frames: V must be >= 1");
    if (!v_pred || !pel_pred || !v_ref || !pel_ref || !ref_of_frame || !out) return seeme_fail("mesh_v2v_frames: null pointer");
    if (((uintptr_t)v_pred | (uintptr_t)v_ref) & 15) return seeme_fail("mesh_v2v_frames: vertices must be 16-byte aligned");
    hipLaunchKernelGGL(k_mesh_v2v, dim3(F), dim3(MM_THREADS), 0, (hipStream_t)stream, v_pred, pel_pred, v_ref, pel_ref, ref_of_frame,
                       V, out);
    return seeme_check_launch("k_mesh_v2v");
}

extern "C" size_t seeme_scene_min_dist2_workspace_bytes(int F, int V, int S, int P) {
    if (F < 1 || V < 1 || V > SC_VMAX || S < 1 || P < 1) return 0;
    return ((size_t)F * 4 + (size_t)F * scene_slices(F, P) + (size_t)F * P) * sizeof(float);
}

extern "C" int seeme_scene_min_dist2(const float* verts, const float* scene, const int32_t* scene_of_frame, int F, int V, int S, int P,
                                     float* out_d2, void* ws, size_t ws_bytes, void* stream) {
    if (F < 1) return seeme_fail("scene_min_dist2: F must be >= 1");
    if (V < 1 || V > SC_VMAX) return seeme_fail("scene_min_dist2: V must be in 1..10112");
    if (S < 1) return seeme_fail("scene_min_dist2: S must be >= 1");
    if (P < 1) return seeme_fail("scene_min_dist2: P must be >= 1");
    if (!verts || !scene || !scene_of_frame || !out_d2 || !ws) return seeme_fail("scene_min_dist2: null pointer");
    if ((uintptr_t)ws & 15) return seeme_fail("scene_min_dist2: workspace must be 16-byte aligned");
    if (ws_bytes < seeme_scene_min_dist2_workspace_bytes(F, V, S, P)) return seeme_fail("scene_min_dist2: workspace too small");
    const int NS = scene_slices(F, P), NG = (V + 63) / 64;
    if ((long)F * NS > 0x7fffffffL) return seeme_fail("scene_min_dist2: too many frames for one launch");
    float* hdr = (float*)ws;
    float* smin = hdr + (size_t)F * 4;
    float* approx = smin + (size_t)F * NS;
    const size_t lds = (size_t)NG * 64 * 4 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    SEEME_HIP(hipFuncSetAttribute((const void*)k_scene_filter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_scene_filter, dim3(F * NS), dim3(MM_THREADS), lds, st, verts, scene, scene_of_frame, V, S, P, NS, NG, hdr, smin,
                       approx);
    if (int rc = seeme_check_launch("k_scene_filter")) return rc;
    hipLaunchKernelGGL(k_scene_exact, dim3(F), dim3(MM_THREADS), 0, st, verts, scene, scene_of_frame, V, S, P, NS, (const float*)hdr,
                       (const float*)smin, (const float*)approx, out_d2);
    return seeme_check_launch("k_scene_exact");
}
