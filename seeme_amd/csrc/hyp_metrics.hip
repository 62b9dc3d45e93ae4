// hyp_metrics.hip -- K hypotheses per sequence: per-hypothesis errors (MPJPE, root error, acceleration error) and the diversity of
// the K draws (APD and standard deviation of the joints) in ONE pass over the joints.
//
// Definitions: the alignment and the three errors are EgoMetrics.per_sequence (seeme_amd/mld.py; compute.py:364-399,243-271,470-474)
// for hypothesis k against its sequence's reference; the two diversity numbers are the EgoHMR forms (test_egohmr.py:494-497 joint
// standard deviation, :515-520 APD of the joints) on the K aligned predictions of a frame, averaged over the valid frames.
//
// Partition: one workgroup (256 lanes) per (sequence b, chunk of HYP_FC_* frames).  The K aligned predictions and the aligned
// reference of a frame live in LDS ([K+1] rows of 72 floats); three such slots form a ring so that the second difference over frames
// t-1, t, t+1 needs no second read (a chunk reads one halo frame on each side).  The next frame's float4 loads are in flight while
// the current one is reduced.  Work items -- (k, joint) for the errors and for APD, one coordinate for the standard deviation -- are
// dealt over the lanes: a (k, joint) lane keeps its joint in registers, takes the error against the reference, then walks the partners
// k+1 .. k+(K-1)/2 (mod K; and k+K/2 for k < K/2 when K is even), so every unordered pair is met exactly once and the pair work is as
// parallel as the error work.  Every lane sums its own items over the chunk's frames in registers, then the
// workgroup adds them in a fixed order and writes 3K+2 partial sums to the workspace.  A second small launch adds the chunks of a
// sequence in chunk order and normalises.  No atomics anywhere: the result is bitwise reproducible.
#include "api_util.hpp"
#include <stdint.h>

#define HYP_KMAX 32
#define HYP_NJ 24
#define HYP_ROW 72                 // 24 joints x 3 floats = 288 B = 18 float4
#define HYP_Q 18
#define HYP_THREADS 256
#define HYP_LD ((HYP_KMAX + 1) * HYP_Q)                                    // float4 loads of one frame: K predictions + reference
#define HYP_NLD ((HYP_LD + HYP_THREADS - 1) / HYP_THREADS)                 // ... per lane (3)
#define HYP_NIT ((HYP_KMAX * HYP_NJ + HYP_THREADS - 1) / HYP_THREADS)      // (k, joint) items per lane (3)
#define HYP_FC_LONG 8
#define HYP_FC_SHORT 4

// frames per workgroup: 8 (one halo frame in four) when that still gives the chip two workgroups per CU, otherwise 4
static int hyp_chunk_frames(int B, int T) {
    return (long)B * ((T + HYP_FC_LONG - 1) / HYP_FC_LONG) >= 512 ? HYP_FC_LONG : HYP_FC_SHORT;
}

__global__ __launch_bounds__(HYP_THREADS) void k_hyp_partial(const float* __restrict__ pred, const float* __restrict__ ref,
                                                             const int32_t* __restrict__ lengths, int K, int T, int FC,
                                                             float* __restrict__ slab) {
    __shared__ float ring[3][HYP_KMAX + 1][HYP_ROW];     // aligned joints; row K is the reference
    __shared__ float pel[3][HYP_KMAX + 1][3];            // pelvis after the first-frame head alignment
    __shared__ float hd[HYP_KMAX + 1][3];                // first frame's joint 15
    __shared__ float red_it[2][HYP_KMAX * HYP_NJ];
    __shared__ float red_w[2][HYP_THREADS / 64];
    __shared__ float red_sd[HYP_ROW];

    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x, NC = gridDim.x;
    const int len = lengths[b];
    const int nvalid = len < 0 ? 0 : (len > T ? T : len);
    const int t0 = chunk * FC, t1 = min(t0 + FC, nvalid);
    float* out = slab + ((size_t)b * NC + chunk) * (3 * K + 2);
    if (t0 >= nvalid) {                                  // nothing valid here: the workspace is not zeroed by anyone else
        for (int i = tid; i < 3 * K + 2; i += HYP_THREADS) out[i] = 0.f;
        return;
    }
    const float* predb = pred + (size_t)b * K * T * HYP_ROW;
    const float* refb = ref + (size_t)b * T * HYP_ROW;
    const int nld = (K + 1) * HYP_Q, nit = K * HYP_NJ;
    const int nd = (K - 1) / 2, khalf = (K & 1) ? 0 : K / 2;     // partners of hypothesis i: i+1 .. i+nd (mod K), and i+K/2 for i < K/2

    if (tid <= K) {
        const float* r0 = (tid < K ? predb + (size_t)tid * T * HYP_ROW : refb) + 15 * 3;
        hd[tid][0] = r0[0]; hd[tid][1] = r0[1]; hd[tid][2] = r0[2];
    }

    float4 v[HYP_NLD], p0[HYP_NLD];
    auto issue = [&](int f) {
#pragma unroll
        for (int r = 0; r < HYP_NLD; ++r) {
            const int e = tid + r * HYP_THREADS;
            if (e < nld) {
                const int row = e / HYP_Q, q = e - row * HYP_Q;
                const float4* src = (const float4*)((row < K ? predb + (size_t)row * T * HYP_ROW : refb) + (size_t)f * HYP_ROW);
                v[r] = src[q];
                p0[r] = src[0];
            }
        }
    };
    auto commit = [&](int slot) {
#pragma unroll
        for (int r = 0; r < HYP_NLD; ++r) {
            const int e = tid + r * HYP_THREADS;
            if (e < nld) {
                const int row = e / HYP_Q, q = e - row * HYP_Q;
                const float h0 = hd[row][0], h1 = hd[row][1], h2 = hd[row][2];
                const float g0 = p0[r].x - h0, g1 = p0[r].y - h1, g2 = p0[r].z - h2;      // pelvis - head(frame 0)
                const float vv[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
                int c = (q * 4) % 3;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float h = c == 0 ? h0 : (c == 1 ? h1 : h2);
                    const float g = c == 0 ? g0 : (c == 1 ? g1 : g2);
                    ring[slot][row][q * 4 + i] = (vv[i] - h) - g;
                    c = c == 2 ? 0 : c + 1;
                }
                if (q == 0) { pel[slot][row][0] = g0; pel[slot][row][1] = g1; pel[slot][row][2] = g2; }
            }
        }
    };

    float a_mp[HYP_NIT], a_ac[HYP_NIT], a_root = 0.f, a_apd = 0.f, a_sd = 0.f;
#pragma unroll
    for (int r = 0; r < HYP_NIT; ++r) a_mp[r] = a_ac[r] = 0.f;

    const int fs = max(t0 - 1, 0), fe = min(t1, nvalid - 1);      // halo frames for the second difference
    issue(fs);
    __syncthreads();                                              // hd
    for (int f = fs; f <= fe; ++f) {
        const int s0 = f % 3;
        commit(s0);
        __syncthreads();
        if (f < fe) issue(f + 1);
        const bool own = f >= t0 && f < t1;
        const int c = f - 1;                                      // centre of the second difference that frame f completes
        const bool acc = c >= t0 && c < t1 && c >= 1;
        const int s1 = (f + 2) % 3, s2 = (f + 1) % 3;             // frames f-1, f-2
        if (own || acc) {
#pragma unroll
            for (int r = 0; r < HYP_NIT; ++r) {
                const int e = tid + r * HYP_THREADS;
                if (e < nit) {
                    const int k = e / HYP_NJ, j3 = (e - k * HYP_NJ) * 3;
                    if (own) {
                        const float x = ring[s0][k][j3], y = ring[s0][k][j3 + 1], z = ring[s0][k][j3 + 2];
                        const float dx = x - ring[s0][K][j3], dy = y - ring[s0][K][j3 + 1], dz = z - ring[s0][K][j3 + 2];
                        a_mp[r] += sqrtf(dx * dx + dy * dy + dz * dz);
                        // APD: this joint of hypothesis k against its partners -- every unordered pair exactly once (the EgoHMR
                        // sum runs over ordered pairs and halves: test_egohmr.py:519-520)
                        int j = k;
                        for (int d = 0; d < nd; ++d) {
                            j = j + 1 == K ? 0 : j + 1;
                            const float ex = x - ring[s0][j][j3], ey = y - ring[s0][j][j3 + 1], ez = z - ring[s0][j][j3 + 2];
                            a_apd += sqrtf(ex * ex + ey * ey + ez * ez);
                        }
                        if (k < khalf) {
                            j = k + khalf;
                            const float ex = x - ring[s0][j][j3], ey = y - ring[s0][j][j3 + 1], ez = z - ring[s0][j][j3 + 2];
                            a_apd += sqrtf(ex * ex + ey * ey + ez * ez);
                        }
                    }
                    if (acc) {
                        float d[3];
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const float ap = (ring[s2][k][j3 + i] - 2.f * ring[s1][k][j3 + i]) + ring[s0][k][j3 + i];
                            const float ar = (ring[s2][K][j3 + i] - 2.f * ring[s1][K][j3 + i]) + ring[s0][K][j3 + i];
                            d[i] = ap - ar;
                        }
                        a_ac[r] += sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                    }
                }
            }
        }
        if (own) {
            if (tid < K) {
                const float dx = pel[s0][tid][0] - pel[s0][K][0], dy = pel[s0][tid][1] - pel[s0][K][1],
                            dz = pel[s0][tid][2] - pel[s0][K][2];
                a_root += sqrtf(dx * dx + dy * dy + dz * dz);
            }
            // unbiased standard deviation over K of one joint coordinate (test_egohmr.py:496); the last 72 lanes take it
            const int cf = tid - (HYP_THREADS - HYP_ROW);
            if (cf >= 0 && K > 1) {
                float m = 0.f;
                for (int k = 0; k < K; ++k) m += ring[s0][k][cf];
                m /= (float)K;
                float s = 0.f;
                for (int k = 0; k < K; ++k) { const float d = ring[s0][k][cf] - m; s += d * d; }
                a_sd += sqrtf(s / (float)(K - 1));
            }
        }
        __syncthreads();                                          // slot (f+1)%3 is overwritten next
    }

    // workgroup sums, fixed order
#pragma unroll
    for (int r = 0; r < HYP_NIT; ++r) {
        const int e = tid + r * HYP_THREADS;
        if (e < nit) { red_it[0][e] = a_mp[r]; red_it[1][e] = a_ac[r]; }
    }
    {
        const int cf = tid - (HYP_THREADS - HYP_ROW);
        if (cf >= 0) red_sd[cf] = a_sd;
        float x = a_apd;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if ((tid & 63) == 0) red_w[0][tid >> 6] = x;
    }
    __syncthreads();
    if (tid < K) {
        float m = 0.f, a = 0.f;
        for (int j = 0; j < HYP_NJ; ++j) { m += red_it[0][tid * HYP_NJ + j]; a += red_it[1][tid * HYP_NJ + j]; }
        out[tid] = m;
        out[K + tid] = a_root;
        out[2 * K + tid] = a;
    } else if (tid == 64) {
        float x = 0.f;
        for (int w = 0; w < HYP_THREADS / 64; ++w) x += red_w[0][w];
        out[3 * K] = x;
    } else if (tid == 128) {
        float x = 0.f;
        for (int i = 0; i < HYP_ROW; ++i) x += red_sd[i];
        out[3 * K + 1] = x;
    }
}

// chunks of a sequence in chunk order (one lane per partial sum, the loads of four chunks in flight), then the normalisation of
// per_sequence / the EgoHMR forms (x1000: metres -> mm)
__global__ __launch_bounds__(128) void k_hyp_final(const float* __restrict__ slab, const int32_t* __restrict__ lengths, int B, int K,
                                                  int NC, float* __restrict__ per_hyp, float* __restrict__ per_seq) {
    const int b = blockIdx.x, v = threadIdx.x, W = 3 * K + 2;
    if (v >= W) return;
    const float* s = slab + (size_t)b * NC * W + v;
    float x = 0.f;
#pragma unroll 4
    for (int c = 0; c < NC; ++c) x += s[(size_t)c * W];
    const int len = lengths[b];
    const float flen = (float)len;
    if (v < 3 * K) {
        const int m = v / K, k = v - m * K;
        const float y = m == 0 ? x / (float)HYP_NJ / flen : (m == 1 ? x / flen : x / (float)HYP_NJ / (float)max(len - 2, 1));
        per_hyp[((size_t)m * B + b) * K + k] = y * 1000.f;
    } else {
        const int w = v - 3 * K;
        // APD: sum over unordered pairs / 24 / K / (K-1)  (= ordered sum / 24 / K / (K-1) / 2); STD: mean over 72 coordinates
        const float den = w == 0 ? (float)HYP_NJ * (float)K * (float)(K - 1) : (float)HYP_ROW;
        per_seq[(size_t)w * B + b] = K > 1 ? x / den / flen * 1000.f : 0.f;
    }
}

extern "C" size_t seeme_hyp_metrics_workspace_bytes(int B, int K, int T) {
    if (B < 1 || K < 1 || K > HYP_KMAX || T < 1) return 0;
    const int FC = hyp_chunk_frames(B, T);
    return (size_t)B * ((T + FC - 1) / FC) * (3 * K + 2) * sizeof(float);
}

extern "C" int seeme_hyp_metrics(const float* jts_pred, const float* jts_ref, const int32_t* lengths, int B, int K, int T,
                                 float* per_hyp, float* per_seq, void* ws, size_t ws_bytes, void* stream) {
    if (B < 1 || B > 65535) return seeme_fail("hyp_metrics: B must be in 1..65535");
    if (K < 1 || K > HYP_KMAX) return seeme_fail("hyp_metrics: K must be in 1..32");
    if (T < 1) return seeme_fail("hyp_metrics: T must be >= 1");
    if (!jts_pred || !jts_ref || !lengths || !per_hyp || !per_seq || !ws) return seeme_fail("hyp_metrics: null pointer");
    if (((uintptr_t)jts_pred | (uintptr_t)jts_ref) & 15) return seeme_fail("hyp_metrics: joints must be 16-byte aligned");
    if (ws_bytes < seeme_hyp_metrics_workspace_bytes(B, K, T)) return seeme_fail("hyp_metrics: workspace too small");
    const int FC = hyp_chunk_frames(B, T), NC = (T + FC - 1) / FC;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hyp_partial, dim3(NC, B), dim3(HYP_THREADS), 0, st, jts_pred, jts_ref, lengths, K, T, FC, (float*)ws);
    if (int rc = seeme_check_launch("k_hyp_partial")) return rc;
    hipLaunchKernelGGL(k_hyp_final, dim3(B), dim3(128), 0, st, (const float*)ws, lengths, B, K, NC, per_hyp, per_seq);
    return seeme_check_launch("k_hyp_final");
}

// ------------------------------------------------------------------ pairwise distances of the K hypotheses and their medoid
// dist[b,i,j] = 1000 x the mean over the nvalid = clamp(len, 0, T) frames and the 24 joints of |a_i - a_j|, a_k the prediction of
// hypothesis k aligned as above; medoid[b] = argmin_i sum_j dist[b,i,j] (fp32, j order, lowest index on a tie).
//
// Partition: one workgroup (256 lanes) per (sequence b, chunk of FC frames, the rule of hyp_chunk_frames).  The K aligned rows of a
// frame live in LDS as [K][72] (stride 73: odd, so the K <= 32 rows a wave touches at one coordinate sit on distinct banks); two
// slots, the next frame's float4 loads in flight while the current one is reduced.  There is no second difference, so no halo frame
// and no ring.  A lane owns whole pairs (i < j, row-major; K = 32 has 496, so lanes 0..239 own two) and loops over the 24 joints;
// it sums its pairs over the chunk's frames in registers and writes them to the workspace [B][chunks][pairs] -- no cross-lane
// reduction.  k_hyp_pair_final adds the chunks in chunk order, normalises, mirrors the matrix and takes the argmin.  No atomics.
#define HYP_PAIRS_MAX (HYP_KMAX * (HYP_KMAX - 1) / 2)                        // 496
#define HYP_NPL ((HYP_PAIRS_MAX + HYP_THREADS - 1) / HYP_THREADS)            // pairs per lane (2)
#define HYP_PROW (HYP_ROW + 1)
#define HYP_PLD ((HYP_KMAX * HYP_Q + HYP_THREADS - 1) / HYP_THREADS)         // float4 loads of one frame per lane (3)

__global__ __launch_bounds__(HYP_THREADS) void k_hyp_pair_partial(const float* __restrict__ pred, const int32_t* __restrict__ lengths,
                                                                  int K, int T, int FC, float* __restrict__ slab) {
    __shared__ float rows[2][HYP_KMAX][HYP_PROW];        // aligned joints of the K hypotheses
    __shared__ float hd[HYP_KMAX][3];                    // first frame's joint 15

    const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x, NC = gridDim.x;
    const int len = lengths[b];
    const int nvalid = len < 0 ? 0 : (len > T ? T : len);
    const int t0 = chunk * FC, t1 = min(t0 + FC, nvalid);
    const int P = K * (K - 1) / 2;
    float* out = slab + ((size_t)b * NC + chunk) * P;
    if (t0 >= nvalid) {                                  // nothing valid here: the workspace is not zeroed by anyone else
        for (int i = tid; i < P; i += HYP_THREADS) out[i] = 0.f;
        return;
    }
    const float* predb = pred + (size_t)b * K * T * HYP_ROW;
    const int nld = K * HYP_Q;

    if (tid < K) {
        const float* r0 = predb + (size_t)tid * T * HYP_ROW + 15 * 3;
        hd[tid][0] = r0[0]; hd[tid][1] = r0[1]; hd[tid][2] = r0[2];
    }
    // this lane's pairs: p = tid + r * 256 -> (i, j), i < j, row-major over the upper triangle
    int pi[HYP_NPL], pj[HYP_NPL];
#pragma unroll
    for (int r = 0; r < HYP_NPL; ++r) {
        int rem = tid + r * HYP_THREADS, i = 0;
        if (rem < P) {
            while (rem >= K - 1 - i) { rem -= K - 1 - i; ++i; }
            pi[r] = i; pj[r] = i + 1 + rem;
        } else {
            pi[r] = pj[r] = -1;
        }
    }

    float4 v[HYP_PLD], p0[HYP_PLD];
    auto issue = [&](int f) {
#pragma unroll
        for (int r = 0; r < HYP_PLD; ++r) {
            const int e = tid + r * HYP_THREADS;
            if (e < nld) {
                const int row = e / HYP_Q, q = e - row * HYP_Q;
                const float4* src = (const float4*)(predb + ((size_t)row * T + f) * HYP_ROW);
                v[r] = src[q];
                p0[r] = src[0];
            }
        }
    };
    auto commit = [&](int slot) {
#pragma unroll
        for (int r = 0; r < HYP_PLD; ++r) {
            const int e = tid + r * HYP_THREADS;
            if (e < nld) {
                const int row = e / HYP_Q, q = e - row * HYP_Q;
                const float h0 = hd[row][0], h1 = hd[row][1], h2 = hd[row][2];
                const float g0 = p0[r].x - h0, g1 = p0[r].y - h1, g2 = p0[r].z - h2;      // pelvis - head(frame 0)
                const float vv[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
                int c = (q * 4) % 3;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float h = c == 0 ? h0 : (c == 1 ? h1 : h2);
                    const float g = c == 0 ? g0 : (c == 1 ? g1 : g2);
                    rows[slot][row][q * 4 + i] = (vv[i] - h) - g;
                    c = c == 2 ? 0 : c + 1;
                }
            }
        }
    };

    float acc[HYP_NPL];
#pragma unroll
    for (int r = 0; r < HYP_NPL; ++r) acc[r] = 0.f;

    issue(t0);
    __syncthreads();                                              // hd
    for (int f = t0; f < t1; ++f) {
        const int s = (f - t0) & 1;
        commit(s);
        __syncthreads();                                          // slot s complete; every lane is done with slot s^1 (frame f-1)
        if (f + 1 < t1) issue(f + 1);
#pragma unroll
        for (int r = 0; r < HYP_NPL; ++r) {
            if (pi[r] >= 0) {
                const float* a = rows[s][pi[r]];
                const float* c = rows[s][pj[r]];
                float x = 0.f;
#pragma unroll 8
                for (int j3 = 0; j3 < HYP_ROW; j3 += 3) {
                    const float ex = a[j3] - c[j3], ey = a[j3 + 1] - c[j3 + 1], ez = a[j3 + 2] - c[j3 + 2];
                    x += sqrtf(ex * ex + ey * ey + ez * ez);
                }
                acc[r] += x;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < HYP_NPL; ++r) {
        const int p = tid + r * HYP_THREADS;
        if (p < P) out[p] = acc[r];
    }
}

// one workgroup per sequence, one lane per pair: the chunks in chunk order, x1000 / 24 / nvalid, both halves of the matrix and a zero
// diagonal; then the row sums in j order and the lowest index of the smallest one
__global__ __launch_bounds__(512) void k_hyp_pair_final(const float* __restrict__ slab, const int32_t* __restrict__ lengths, int K, int T,
                                                        int NC, float* __restrict__ dist, int32_t* __restrict__ medoid) {
    __shared__ float D[HYP_KMAX][HYP_KMAX + 1];
    __shared__ float rs[HYP_KMAX];
    const int b = blockIdx.x, p = threadIdx.x, P = K * (K - 1) / 2;
    const int len = lengths[b];
    const int nvalid = len < 0 ? 0 : (len > T ? T : len);
    float* db = dist + (size_t)b * K * K;
    if (p < P) {
        const float* s = slab + (size_t)b * NC * P + p;
        float x = 0.f;
#pragma unroll 4
        for (int c = 0; c < NC; ++c) x += s[(size_t)c * P];
        const float d = nvalid > 0 ? x / (float)HYP_NJ / (float)nvalid * 1000.f : 0.f;
        int rem = p, i = 0;
        while (rem >= K - 1 - i) { rem -= K - 1 - i; ++i; }
        const int j = i + 1 + rem;
        D[i][j] = d; D[j][i] = d;
        db[i * K + j] = d; db[j * K + i] = d;
    }
    if (p < K) { D[p][p] = 0.f; db[p * K + p] = 0.f; }
    __syncthreads();
    if (p < K) {
        float x = 0.f;
        for (int j = 0; j < K; ++j) x += D[p][j];
        rs[p] = x;
    }
    __syncthreads();
    if (p == 0) {
        int best = 0;
        for (int i = 1; i < K; ++i) if (rs[i] < rs[best]) best = i;
        medoid[b] = best;
    }
}

extern "C" size_t seeme_hyp_pairdist_workspace_bytes(int B, int K, int T) {
    if (B < 1 || K < 1 || K > HYP_KMAX || T < 1) return 0;
    const int FC = hyp_chunk_frames(B, T), P = K * (K - 1) / 2;
    return (size_t)B * ((T + FC - 1) / FC) * (P > 0 ? P : 1) * sizeof(float);       // K = 1 has no pair: one unused float per chunk
}

extern "C" int seeme_hyp_pairdist(const float* jts_pred, const int32_t* lengths, int B, int K, int T, float* dist, int32_t* medoid,
                                  void* ws, size_t ws_bytes, void* stream) {
    if (B < 1 || B > 65535) return seeme_fail("hyp_pairdist: B must be in 1..65535");
    if (K < 1 || K > HYP_KMAX) return seeme_fail("hyp_pairdist: K must be in 1..32");
    if (T < 1) return seeme_fail("hyp_pairdist: T must be >= 1");
    if (!jts_pred || !lengths || !dist || !medoid || !ws) return seeme_fail("hyp_pairdist: null pointer");
    if (((uintptr_t)jts_pred | (uintptr_t)ws) & 15) return seeme_fail("hyp_pairdist: joints and workspace must be 16-byte aligned");
    if (ws_bytes < seeme_hyp_pairdist_workspace_bytes(B, K, T)) return seeme_fail("hyp_pairdist: workspace too small");
    const int FC = hyp_chunk_frames(B, T), NC = (T + FC - 1) / FC;
    hipStream_t st = (hipStream_t)stream;
    if (K > 1) {                                                                  // K = 1: no pair, nothing to sum
        hipLaunchKernelGGL(k_hyp_pair_partial, dim3(NC, B), dim3(HYP_THREADS), 0, st, jts_pred, lengths, K, T, FC, (float*)ws);
        if (int rc = seeme_check_launch("k_hyp_pair_partial")) return rc;
    }
    hipLaunchKernelGGL(k_hyp_pair_final, dim3(B), dim3(512), 0, st, (const float*)ws, lengths, K, T, NC, dist, medoid);
    return seeme_check_launch("k_hyp_pair_final");
}
