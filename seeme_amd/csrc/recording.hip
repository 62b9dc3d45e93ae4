// recording.hip -- a whole recording from W overlapping windows of T frames with K hypotheses each: the disagreement of neighbouring
// windows on the frames they share (seeme_overlap_cost), the one path through the W x K hypotheses that agrees with itself best
// (seeme_path_select) and the stitched motion of that path (seeme_stitch_windows).  Definitions: include/seeme_hip.h; the plain-torch
// twins are in seeme_amd/recording.py.  fp32 throughout, no atomics: every result is bitwise reproducible.
#include "api_util.hpp"
#include "rec_quat.hpp"
#include <stdint.h>

#define REC_KMAX 32
#define REC_NJ 24
#define REC_ROW 72                 // 24 joints x 3 floats = 288 B = 18 float4
#define REC_Q 18
#define REC_PROW (REC_ROW + 1)     // odd LDS stride: the K <= 32 rows a wave touches at one coordinate sit on distinct banks
#define REC_THREADS 256
#define REC_FC 4                   // shared frames per workgroup of k_overlap_partial
#define REC_LD ((2 * REC_KMAX * REC_Q + REC_THREADS - 1) / REC_THREADS)      // float4 loads of one shared frame per lane (5)
#define REC_NPL ((REC_KMAX * REC_KMAX + REC_THREADS - 1) / REC_THREADS)      // (i, j) pairs per lane (4)

// ------------------------------------------------------------------ overlap cost
// Partition: one workgroup (256 lanes) per (seam w, chunk of REC_FC shared frames).  The K rows of window w at frame T-O+r and the K
// rows of window w+1 at frame r live in LDS as [2K][72] (stride 73); two slots, the next frame's float4 loads in flight while the
// current one is reduced.  A lane owns whole ordered pairs p = i*K + j (K = 32 has 1024: four per lane; consecutive lanes differ in
// j, so the reads of window w's row are broadcasts) and loops over the 24 joints; it sums its pairs over the chunk's frames in
// registers and writes them to the workspace [W-1][chunks][K*K] -- no cross-lane reduction.  k_overlap_final adds the chunks in
// chunk order and normalises.
__global__ __launch_bounds__(REC_THREADS) void k_overlap_partial(const float* __restrict__ jts, int K, int T, int O,
                                                                 float* __restrict__ slab) {
    __shared__ float rows[2][2 * REC_KMAX][REC_PROW];

    const int tid = threadIdx.x, w = blockIdx.y, chunk = blockIdx.x, NC = gridDim.x;
    const int r0 = chunk * REC_FC, r1 = min(r0 + REC_FC, O);          // r0 < O by the grid
    const int P = K * K, nld = 2 * K * REC_Q;
    float* out = slab + ((size_t)w * NC + chunk) * P;
    const float* wa = jts + (size_t)w * K * T * REC_ROW;              // window w, read at frames T-O+r
    const float* wb = wa + (size_t)K * T * REC_ROW;                   // window w+1, read at frames r

    float4 v[REC_LD];
    auto issue = [&](int r) {
#pragma unroll
        for (int q = 0; q < REC_LD; ++q) {
            const int e = tid + q * REC_THREADS;
            if (e < nld) {
                const int row = e / REC_Q, c = e - row * REC_Q;
                const float* src = row < K ? wa + ((size_t)row * T + (T - O + r)) * REC_ROW : wb + ((size_t)(row - K) * T + r) * REC_ROW;
                v[q] = ((const float4*)src)[c];
            }
        }
    };
    auto commit = [&](int slot) {
#pragma unroll
        for (int q = 0; q < REC_LD; ++q) {
            const int e = tid + q * REC_THREADS;
            if (e < nld) {
                const int row = e / REC_Q, c = e - row * REC_Q;
                float* d = &rows[slot][row][c * 4];
                d[0] = v[q].x; d[1] = v[q].y; d[2] = v[q].z; d[3] = v[q].w;
            }
        }
    };

    float acc[REC_NPL];
#pragma unroll
    for (int q = 0; q < REC_NPL; ++q) acc[q] = 0.f;

    issue(r0);
    for (int r = r0; r < r1; ++r) {
        const int s = (r - r0) & 1;
        commit(s);
        __syncthreads();                                              // slot s complete; every lane is done with slot s^1 (frame r-1)
        if (r + 1 < r1) issue(r + 1);
#pragma unroll
        for (int q = 0; q < REC_NPL; ++q) {
            const int p = tid + q * REC_THREADS;
            if (p < P) {
                const int i = p / K, j = p - i * K;
                const float* a = rows[s][i];
                const float* b = rows[s][K + j];
                float x = 0.f;
#pragma unroll 8
                for (int j3 = 0; j3 < REC_ROW; j3 += 3) {
                    const float ex = a[j3] - b[j3], ey = a[j3 + 1] - b[j3 + 1], ez = a[j3 + 2] - b[j3 + 2];
                    x += sqrtf(ex * ex + ey * ey + ez * ez);
                }
                acc[q] += x;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < REC_NPL; ++q) {
        const int p = tid + q * REC_THREADS;
        if (p < P) out[p] = acc[q];
    }
}

// one workgroup per seam, lanes over the K*K pairs: the chunks in chunk order, x1000 / 24 / O
__global__ __launch_bounds__(REC_THREADS) void k_overlap_final(const float* __restrict__ slab, int K, int O, int NC,
                                                               float* __restrict__ cost) {
    const int w = blockIdx.x, P = K * K;
    for (int p = threadIdx.x; p < P; p += REC_THREADS) {
        const float* s = slab + (size_t)w * NC * P + p;
        float x = 0.f;
#pragma unroll 4
        for (int c = 0; c < NC; ++c) x += s[(size_t)c * P];
        cost[(size_t)w * P + p] = x / (float)REC_NJ / (float)O * 1000.f;
    }
}

extern "C" size_t seeme_overlap_cost_workspace_bytes(int W, int K, int T, int O) {
    if (W < 1 || K < 1 || K > REC_KMAX || T < 1 || O < 0 || 2 * (long)O > T) return 0;
    if (W == 1 || O == 0) return 16;                                  // nothing is launched; a workspace is still passed
    return (size_t)(W - 1) * ((O + REC_FC - 1) / REC_FC) * K * K * sizeof(float);
}

extern "C" int seeme_overlap_cost(const float* jts, int W, int K, int T, int O, float* cost, void* ws, size_t ws_bytes, void* stream) {
    if (W < 1 || W > 65536) return seeme_fail("overlap_cost: W must be in 1..65536");
    if (K < 1 || K > REC_KMAX) return seeme_fail("overlap_cost: K must be in 1..32");
    if (T < 1) return seeme_fail("overlap_cost: T must be >= 1");
    if (O < 0 || 2 * (long)O > T) return seeme_fail("overlap_cost: the overlap must satisfy 0 <= O and 2*O <= T");
    if (!jts || !ws) return seeme_fail("overlap_cost: null pointer");
    if (((uintptr_t)jts | (uintptr_t)ws) & 15) return seeme_fail("overlap_cost: joints and workspace must be 16-byte aligned");
    if (ws_bytes < seeme_overlap_cost_workspace_bytes(W, K, T, O)) return seeme_fail("overlap_cost: workspace too small");
    if (W == 1 || O == 0) return 0;                                   // no seam, or nothing shared: nothing to write
    if (!cost) return seeme_fail("overlap_cost: null pointer");
    const int NC = (O + REC_FC - 1) / REC_FC;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_overlap_partial, dim3(NC, W - 1), dim3(REC_THREADS), 0, st, jts, K, T, O, (float*)ws);
    if (int rc = seeme_check_launch("k_overlap_partial")) return rc;
    hipLaunchKernelGGL(k_overlap_final, dim3(W - 1), dim3(REC_THREADS), 0, st, (const float*)ws, K, O, NC, cost);
    return seeme_check_launch("k_overlap_final");
}

// ------------------------------------------------------------------ min-sum path
// One workgroup of one wave; lane j < K is end state j.  d[j] = the smallest sum of a path that ends in hypothesis j of the current
// window, kept in LDS.  Step w -> w+1: lane j takes cand_i = d[i] + cost[w,i,j] for i = 0..K-1 (its column of the transition matrix,
// coalesced over the lanes; the column of the NEXT step is loaded before the current one is reduced, it does not depend on d), keeps
// the lowest i of the smallest one, stores it as the back-pointer in the workspace and adds unary[w+1,j].  Lane 0 then takes the
// lowest index of the smallest d and walks the back-pointers; the lanes write the seam costs.  A column of candidates (or the final
// d) that holds a NaN has no minimum: index 0 and a NaN sum.
__device__ __forceinline__ void rec_argmin(float x, int i, float& best, int& at, bool& bad) {
    bad = bad || x != x;
    if (x < best) { best = x; at = i; }
}

__global__ __launch_bounds__(64) void k_path_select(const float* __restrict__ cost, const float* __restrict__ unary, int W, int K,
                                                    int32_t* __restrict__ path, float* __restrict__ seam, float* __restrict__ total,
                                                    int32_t* __restrict__ back) {
    __shared__ float d[REC_KMAX];
    const int j = threadIdx.x;
    const bool lane = j < K;
    const float qnan = __int_as_float(0x7fc00000);
    if (lane) d[j] = unary ? unary[j] : 0.f;
    float cn[REC_KMAX];
    auto load = [&](int w) {
#pragma unroll
        for (int i = 0; i < REC_KMAX; ++i)
            if (lane && i < K) cn[i] = cost[((size_t)w * K + i) * K + j];
    };
    if (W > 1) load(0);
    __syncthreads();
    for (int w = 0; w + 1 < W; ++w) {
        float c[REC_KMAX];
#pragma unroll
        for (int i = 0; i < REC_KMAX; ++i) c[i] = cn[i];
        if (w + 2 < W) load(w + 1);
        float best = 0.f;
        int at = 0;
        bool bad = false;
        if (lane) {
            best = d[0] + c[0];
            bad = best != best;
#pragma unroll
            for (int i = 1; i < REC_KMAX; ++i)
                if (i < K) rec_argmin(d[i] + c[i], i, best, at, bad);
            if (bad) { best = qnan; at = 0; }
            if (unary) best += unary[(size_t)(w + 1) * K + j];
            back[(size_t)w * K + j] = at;
        }
        __syncthreads();                                              // every lane has read d
        if (lane) d[j] = best;
        __syncthreads();
    }
    if (j == 0) {
        float best = d[0];
        int at = 0;
        bool bad = best != best;
        for (int i = 1; i < K; ++i) rec_argmin(d[i], i, best, at, bad);
        if (bad) { best = qnan; at = 0; }
        total[0] = best;
        path[W - 1] = at;
        for (int w = W - 2; w >= 0; --w) {                            // (this workgroup's own stores, ordered by the barriers above)
            at = back[(size_t)w * K + at];
            path[w] = at;
        }
    }
    __syncthreads();
    for (int w = j; w + 1 < W; w += 64) seam[w] = cost[((size_t)w * K + path[w]) * K + path[w + 1]];
}

extern "C" size_t seeme_path_select_workspace_bytes(int W, int K) {
    if (W < 1 || K < 1 || K > REC_KMAX) return 0;
    return W > 1 ? (size_t)(W - 1) * K * sizeof(int32_t) : 16;
}

extern "C" int seeme_path_select(const float* cost, const float* unary, int W, int K, int32_t* path, float* seam, float* total,
                                 void* ws, size_t ws_bytes, void* stream) {
    if (W < 1) return seeme_fail("path_select: W must be >= 1");
    if (K < 1 || K > REC_KMAX) return seeme_fail("path_select: K must be in 1..32");
    if (!path || !total || !ws || (W > 1 && (!cost || !seam))) return seeme_fail("path_select: null pointer");
    if ((uintptr_t)ws & 3) return seeme_fail("path_select: workspace must be 4-byte aligned");
    if (ws_bytes < seeme_path_select_workspace_bytes(W, K)) return seeme_fail("path_select: workspace too small");
    hipLaunchKernelGGL(k_path_select, dim3(1), dim3(64), 0, (hipStream_t)stream, cost, unary, W, K, path, seam, total, (int32_t*)ws);
    return seeme_check_launch("k_path_select");
}

// ------------------------------------------------------------------ stitching
// One lane per (frame n of the recording, unit): a unit is one joint rotation (3 axis-angle or 6 rot6d values) or the translation.
// Frame n belongs to window w = min(n / S, W-1), S = T - O, at local frame t = n - w*S; when w >= 1 and t < O it is also frame t + S
// of window w-1 and the two are blended with weight u = (t+1)/(O+1) for window w, otherwise the unit is copied.
// (RecQuat, rec_normalize, rec_aa_to_quat, rec_quat_to_aa and rec_blend: rec_quat.hpp, shared with track.hip)
// (rec_rot6d_to_quat and rec_quat_to_rot6d, the model-side rot6d: rec_quat.hpp as well, shared with headset.hip)
__global__ __launch_bounds__(REC_THREADS) void k_stitch_windows(const float* __restrict__ feats, int W, int T, int O, int n_frames,
                                                                int F, int layout, float* __restrict__ out) {
    const int rot6d = layout == SEEME_STITCH_ROT6D;
    const int U = rot6d ? REC_NJ : F / 3, uw = rot6d ? 6 : 3;         // units of a frame, floats of a unit
    const long item = (long)blockIdx.x * REC_THREADS + threadIdx.x;
    if (item >= (long)n_frames * U) return;
    const int n = (int)(item / U), un = (int)(item - (long)n * U);
    const int S = T - O;
    const int w = min(n / S, W - 1), t = n - w * S;
    const float* b = feats + ((size_t)w * T + t) * F + un * uw;       // the later (or only) window
    float* o = out + (size_t)n * F + un * uw;
    float y[6];
    if (w >= 1 && t < O) {
        const float* a = feats + ((size_t)(w - 1) * T + t + S) * F + un * uw;
        const float u = (float)(t + 1) / (float)(O + 1);
        if (rot6d) {
            rec_quat_to_rot6d(rec_blend(rec_rot6d_to_quat(a), rec_rot6d_to_quat(b), u), y);
        } else if (layout == SEEME_STITCH_ANGLE_TRANSL && un == U - 1) {
            for (int i = 0; i < 3; ++i) y[i] = a[i] + u * (b[i] - a[i]);
        } else {
            rec_quat_to_aa(rec_blend(rec_aa_to_quat(a), rec_aa_to_quat(b), u), y);
        }
    } else {
        for (int i = 0; i < uw; ++i) y[i] = b[i];
    }
    for (int i = 0; i < uw; ++i) o[i] = y[i];
}

extern "C" int seeme_stitch_windows(const float* feats, int W, int T, int O, int n_frames, int F, int layout, float* out, void* stream) {
    if (W < 1 || T < 1 || n_frames < 1) return seeme_fail("stitch_windows: W, T and n_frames must be >= 1");
    if (O < 0 || 2 * (long)O > T) return seeme_fail("stitch_windows: the overlap must satisfy 0 <= O and 2*O <= T");
    const int S = T - O;
    const long plan = n_frames <= T ? 1 : ((long)n_frames - T + S - 1) / S + 1;
    if (plan != W) return seeme_fail("stitch_windows: W is not the window plan of n_frames (ceil((n_frames - T) / (T - O)) + 1)");
    if (layout == SEEME_STITCH_ROT6D) {
        if (F != 6 * REC_NJ) return seeme_fail("stitch_windows: rot6d features are 24 x 6 = 144 wide");
    } else if (layout == SEEME_STITCH_ANGLE || layout == SEEME_STITCH_ANGLE_TRANSL) {
        if (F < 3 || F % 3 || (layout == SEEME_STITCH_ANGLE_TRANSL && F < 6))
            return seeme_fail("stitch_windows: axis-angle features are J x 3 (+ 3 translation values) wide");
    } else {
        return seeme_fail("stitch_windows: unknown layout");
    }
    if (!feats || !out) return seeme_fail("stitch_windows: null pointer");
    const int U = layout == SEEME_STITCH_ROT6D ? REC_NJ : F / 3;
    const long blocks = ((long)n_frames * U + REC_THREADS - 1) / REC_THREADS;
    if (blocks > 0x7fffffffL) return seeme_fail("stitch_windows: too many frames for one launch");
    hipLaunchKernelGGL(k_stitch_windows, dim3((unsigned)blocks), dim3(REC_THREADS), 0, (hipStream_t)stream, feats, W, T, O, n_frames, F,
                       layout, out);
    return seeme_check_launch("k_stitch_windows");
}
