// track.hip -- one coherent interactee track from the flow head's samples at sparse key frames: the random-walk transition costs between
// the samples of neighbouring key frames (seeme_track_cost; the path through them is seeme_path_select of recording.hip) and the filled,
// filtered motion of the chosen samples (seeme_track_filter).  Definitions: include/seeme_hip.h; the plain-torch twins are in
// seeme_amd/track.py.  fp32 throughout, no atomics: every result is bitwise reproducible.
#include "api_util.hpp"
#include "rec_quat.hpp"
#include <math.h>
#include <stdint.h>

#define TRK_SMAX 32
#define TRK_ROW 72                 // 24 joints x 3 floats = 288 B = 18 float4
#define TRK_Q 18
#define TRK_PROW (TRK_ROW + 1)     // odd LDS stride: a dword read's bank is (address / 4) mod 32, so the S <= 32 rows that the lanes of one
                                   // 32-lane group touch at one coordinate sit on 32 distinct banks (72 = 8 mod 32 would fold them onto 4)
#define TRK_THREADS 256
#define TRK_LD ((2 * TRK_SMAX * TRK_Q + TRK_THREADS - 1) / TRK_THREADS)      // float4 loads of the two key frames per lane (5)
#define TRK_NPL ((TRK_SMAX * TRK_SMAX + TRK_THREADS - 1) / TRK_THREADS)      // (i, j) pairs per lane (4)
#define TRK_RMAX 32
#define TRK_JMAX 32
#define TRK_UC 17                  // units per pass of k_track_filter: 33 units at the limits take two passes, (64 + 64) x 17 x 16 B = 34 KB
#define TRK_NF (SEEME_TRACK_TILE + 2 * TRK_RMAX)

// ------------------------------------------------------------------ transition costs
// One workgroup per pair of neighbouring key frames (l, l+1): the S rows of frame l and the S rows of frame l+1 in LDS as [2S][72]
// (stride 73).  A lane owns whole ordered pairs p = i*S + j (S = 32 has 1024: four per lane; consecutive lanes differ in j, so the
// reads of frame l's row are broadcasts) and walks the 24 joints in joint order.
__global__ __launch_bounds__(TRK_THREADS) void k_track_cost(const float* __restrict__ jts, const int32_t* __restrict__ idx, int S,
                                                            float weight, float* __restrict__ cost) {
    __shared__ float rows[2 * TRK_SMAX][TRK_PROW];
    const int tid = threadIdx.x, l = blockIdx.x;
    const int P = S * S, nld = 2 * S * TRK_Q;
    const float4* src = (const float4*)(jts + (size_t)l * S * TRK_ROW);       // frames l and l+1 are contiguous: [2S][72]
#pragma unroll
    for (int q = 0; q < TRK_LD; ++q) {
        const int e = tid + q * TRK_THREADS;
        if (e < nld) {
            const int row = e / TRK_Q, c = e - row * TRK_Q;
            const float4 v = src[e];
            float* d = &rows[row][c * 4];
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
    const float gap = (float)(idx[l + 1] - idx[l]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TRK_NPL; ++q) {
        const int p = tid + q * TRK_THREADS;
        if (p < P) {
            const int i = p / S, j = p - i * S;
            const float* a = rows[i];
            const float* b = rows[S + j];
            float x = 0.f;
#pragma unroll 8
            for (int j3 = 0; j3 < TRK_ROW; j3 += 3) {
                const float ex = a[j3] - b[j3], ey = a[j3 + 1] - b[j3 + 1], ez = a[j3 + 2] - b[j3 + 2];
                x += ex * ex + ey * ey + ez * ez;
            }
            cost[(size_t)l * P + p] = weight * x / gap;
        }
    }
}

extern "C" int seeme_track_cost(const float* jts, const int32_t* idx, int Lf, int S, float weight, float* cost, void* stream) {
    if (Lf < 1 || Lf > 65536) return seeme_fail("track_cost: Lf must be in 1..65536");
    if (S < 1 || S > TRK_SMAX) return seeme_fail("track_cost: S must be in 1..32");
    if (!jts || !idx) return seeme_fail("track_cost: null pointer");
    if ((uintptr_t)jts & 15) return seeme_fail("track_cost: joints must be 16-byte aligned");
    if ((uintptr_t)idx & 3) return seeme_fail("track_cost: idx must be 4-byte aligned");
    if (Lf == 1) return 0;                                            // no pair of key frames: nothing to write
    if (!cost) return seeme_fail("track_cost: null pointer");
    hipLaunchKernelGGL(k_track_cost, dim3(Lf - 1), dim3(TRK_THREADS), 0, (hipStream_t)stream, jts, idx, S, weight, cost);
    return seeme_check_launch("k_track_cost");
}

// ------------------------------------------------------------------ fill between the keys, then the symmetric FIR
// One workgroup per SEEME_TRACK_TILE output frames n0 .. n0+TILE-1; its halo is the TILE + 2R frames n0-R .. n0+TILE-1+R, of which those
// inside 0..L-1 exist.  Step 1, one lane per halo frame: the key interval by binary search in idx (ka = the key at or before the frame,
// ku = the blend weight towards key ka+1; ku < 0 marks a frame that takes key ka as it is: a key itself, or a hold before the first /
// after the last key).  Step 2, per pass of TRK_UC units, one lane per (halo frame, unit): fill as a quaternion (the translation as
// (x, y, z, 0)) into LDS.  Step 3, one lane per (output frame, unit): the taps over the LDS rows in increasing frame order.
struct TrkTaps { float t[TRK_RMAX + 1]; };

__global__ __launch_bounds__(TRK_THREADS) void k_track_filter(const float* __restrict__ pose, const float* __restrict__ transl,
                                                              const int32_t* __restrict__ idx, int Lf, int L, int J, TrkTaps taps, int R,
                                                              float* __restrict__ pose_out, float* __restrict__ transl_out) {
    __shared__ float4 fq[TRK_NF][TRK_UC];
    __shared__ int ka[TRK_NF];
    __shared__ float ku[TRK_NF];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * SEEME_TRACK_TILE, m0 = n0 - R;        // halo row f is frame m0 + f
    const int nf = SEEME_TRACK_TILE + 2 * R;
    const int U = J + (transl ? 1 : 0);

    if (tid < nf) {
        const int m = m0 + tid;
        int a = 0;
        float u = -1.f;
        if (m >= 0 && m < L) {
            if (m <= idx[0]) {
                a = 0;
            } else if (m >= idx[Lf - 1]) {
                a = Lf - 1;
            } else {                                                  // idx[0] < m < idx[Lf-1]: the last key at or before m
                int lo = 0, hi = Lf - 1;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (idx[mid] <= m) lo = mid; else hi = mid;
                }
                a = lo;
                const int at = idx[a];
                if (m != at) u = (float)(m - at) / (float)(idx[a + 1] - at);
            }
        }
        ka[tid] = a;
        ku[tid] = u;
    }
    __syncthreads();

    for (int u0 = 0; u0 < U; u0 += TRK_UC) {
        const int nu = min(TRK_UC, U - u0);
        for (int it = tid; it < nf * nu; it += TRK_THREADS) {
            const int f = it / nu, uc = it - f * nu, un = u0 + uc, m = m0 + f;
            if (m < 0 || m >= L) continue;
            const int a = ka[f];
            const float u = ku[f];
            float4 v;
            if (un == J) {                                            // the translation
                const float* p = transl + (size_t)a * 3;
                if (u < 0.f) {
                    v = make_float4(p[0], p[1], p[2], 0.f);
                } else {
                    const float* q = p + 3;
                    v = make_float4(p[0] + u * (q[0] - p[0]), p[1] + u * (q[1] - p[1]), p[2] + u * (q[2] - p[2]), 0.f);
                }
            } else {
                const float* p = pose + ((size_t)a * J + un) * 3;
                RecQuat q = rec_aa_to_quat(p);
                if (!(u < 0.f)) q = rec_blend(q, rec_aa_to_quat(p + (size_t)J * 3), u);
                v = make_float4(q.w, q.x, q.y, q.z);
            }
            fq[f][uc] = v;
        }
        __syncthreads();
        for (int it = tid; it < SEEME_TRACK_TILE * nu; it += TRK_THREADS) {
            const int t = it / nu, uc = it - t * nu, un = u0 + uc, n = n0 + t;
            if (n >= L) continue;
            const int fc = t + R;                                     // the output frame's own halo row
            float* o = un == J ? transl_out + (size_t)n * 3 : pose_out + ((size_t)n * J + un) * 3;
            if (R == 0 && ka[fc] >= 0 && idx[ka[fc]] == n) {          // a key frame without a filter: bit for bit
                const float* p = un == J ? transl + (size_t)ka[fc] * 3 : pose + ((size_t)ka[fc] * J + un) * 3;
                o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
                continue;
            }
            const float4 c = fq[fc][uc];
            float aw = 0.f, ax = 0.f, ay = 0.f, az = 0.f, ws = 0.f;
            for (int d = -R; d <= R; ++d) {                           // increasing frame order; the tap index is uniform over the lanes
                const int m = n + d;
                if (m < 0 || m >= L) continue;
                const float4 q = fq[fc + d][uc];
                float k = taps.t[d < 0 ? -d : d];
                ws += k;
                if (un != J && q.x * c.x + q.y * c.y + q.z * c.z + q.w * c.w < 0.f) k = -k;
                aw += k * q.x; ax += k * q.y; ay += k * q.z; az += k * q.w;
            }
            if (un == J) {
                o[0] = aw / ws; o[1] = ax / ws; o[2] = ay / ws;
            } else {
                float y[3];
                rec_quat_to_aa(rec_normalize({aw, ax, ay, az}), y);
                o[0] = y[0]; o[1] = y[1]; o[2] = y[2];
            }
        }
        __syncthreads();                                              // every lane is done with this pass's rows
    }
}

extern "C" int seeme_track_filter(const float* pose, const float* transl, const int32_t* idx, int Lf, int L, int J,
                                  const float* taps_host, int R, float* pose_out, float* transl_out, void* stream) {
    if (J < 1 || J > TRK_JMAX) return seeme_fail("track_filter: J must be in 1..32");
    if (L < 1 || L > (1 << 20)) return seeme_fail("track_filter: L must be in 1..2^20");
    if (Lf < 1 || Lf > L) return seeme_fail("track_filter: Lf must be in 1..L (a key per recording frame at most)");
    if (R < 0 || R > TRK_RMAX) return seeme_fail("track_filter: R must be in 0..32");
    if (!pose || !idx || !taps_host || !pose_out) return seeme_fail("track_filter: null pointer");
    if ((transl == nullptr) != (transl_out == nullptr))
        return seeme_fail("track_filter: null pointer (transl and transl_out go together: both or neither)");
    if ((uintptr_t)idx & 3) return seeme_fail("track_filter: idx must be 4-byte aligned");
    TrkTaps taps;
    for (int d = 0; d <= TRK_RMAX; ++d) taps.t[d] = 0.f;
    for (int d = 0; d <= R; ++d) {
        const float t = taps_host[d];
        if (!isfinite(t) || t < 0.f) return seeme_fail("track_filter: every tap must be finite and >= 0");
        taps.t[d] = t;
    }
    if (!(taps.t[0] > 0.f)) return seeme_fail("track_filter: taps[0] must be > 0");
    const int blocks = (L + SEEME_TRACK_TILE - 1) / SEEME_TRACK_TILE;
    hipLaunchKernelGGL(k_track_filter, dim3(blocks), dim3(TRK_THREADS), 0, (hipStream_t)stream, pose, transl, idx, Lf, L, J, taps, R,
                       pose_out, transl_out);
    return seeme_check_launch("k_track_filter");
}
