// collision.hip -- point-in-mesh test of the body-scene collision ratio (EgoHMR egohmr.py:511-538, eval_coll): how many points of
// the scene cloud lie inside the posed body.  The reference asks a learned occupancy network; its target has an exact form, the
// winding number of the closed mesh around the point:
//
//   a, b, c = the corners of a face minus p
//   Omega   = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)          (Van Oosterom-Strackee)
//   w(p)    = sum over the faces of Omega / 4 pi,      p is inside iff |w(p)| >= 0.5
//
// A face with two equal indices, or with an index outside 0..V-1, contributes 0 (it is never read); a face with a corner vector
// of squared length 0 contributes 0, never NaN.  A point outside the closed bounding box of the frame's vertices has w = 0 and is
// not evaluated (the reference's filter, egohmr.py:527-531).
//
//   k_mesh_winding   w for every point, no prefilter: the primitive the accuracy is measured on.
//   k_inside_count   one workgroup per (frame, slice of the cloud): bounding box, then the slice is walked 512 points at a time and
//                    the survivors are compacted into a queue in LDS; whenever 512 are queued they are evaluated, one point per
//                    lane (waves without a point skip the walk).  The queue holds two rounds, so all 512 points of a step may survive: no cap.
//   k_inside_finish  out[f] = sum of the slices' counts.
//
// Both kernels keep the frame's vertices in LDS (12 bytes each: 83 KB for SMPL, 121 KB at the limit V = 10112) and call ONE device
// function, wn_point: a lane owns a point and walks the faces in table order, so the face indices are wave-uniform (scalar loads
// from a table every frame shares) and the three vertex reads are LDS broadcasts; everything else is VALU work, about 60 operations
// and one arctangent per (point, face) pair, summed in a float64 accumulator.  The sum of a point runs in table order in one lane
// whatever the launch shape, lane or queue slot, and the count is an integer: results are bitwise reproducible and independent of
// F, of the slicing and of chunking.
// No atomics.
#include "api_util.hpp"
#include <math.h>
#include <stdint.h>

#define WN_THREADS 512                      // two waves per SIMD; one workgroup per CU (the vertices fill most of the LDS)
#define WN_WAVES (WN_THREADS / 64)
#define WN_VMAX 10112                       // the limit of seeme_scene_min_dist2
#define WN_QUEUE (2 * WN_THREADS)
#define WN_INF __builtin_huge_valf()
#define WN_INV_2PI 0.15915494309189535      // w = sum of atan2 / (2 pi)

// atan2 term of one face: half its solid angle.  The lengths use the bare v_sqrt_f32 (1 ulp).
__device__ __forceinline__ float wn_face(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
    const float a2 = ax * ax + ay * ay + az * az, b2 = bx * bx + by * by + bz * bz, c2 = cx * cx + cy * cy + cz * cz;
    const float la = __builtin_amdgcn_sqrtf(a2), lb = __builtin_amdgcn_sqrtf(b2), lc = __builtin_amdgcn_sqrtf(c2);
    const float num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
    const float ab = ax * bx + ay * by + az * bz, bc = bx * cx + by * cy + bz * cz, ca = cx * ax + cy * ay + cz * az;
    const float den = la * lb * lc + ab * lc + bc * la + ca * lb;
    const float h = atan2f(num, den);
    return fminf(fminf(a2, b2), c2) == 0.f ? 0.f : h;
}

// w of the point (px, py, pz) around the mesh whose vertices sit in LDS.  NF, V and the table are wave-uniform.
__device__ __forceinline__ float wn_point(const float* vl, const int32_t* __restrict__ faces, int NF, int V, float px, float py,
                                          float pz) {
    double acc = 0.0;                                                    // 13 776 terms: an fp32 sum would lose more than the terms do
    int n0 = faces[0], n1 = faces[1], n2 = faces[2];
    for (int j = 0; j < NF; ++j) {
        const int i0 = n0, i1 = n1, i2 = n2;
        const int jn = j + 1 < NF ? j + 1 : j;                           // the next face's indices travel while this one is computed
        n0 = faces[3 * jn]; n1 = faces[3 * jn + 1]; n2 = faces[3 * jn + 2];
        // branch-free: a face that does not count reads vertex 0 three times and adds 0
        const bool ok = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V && i0 != i1 && i1 != i2 &&
                        i0 != i2;
        const float* a = vl + (ok ? 3 * i0 : 0);
        const float* b = vl + (ok ? 3 * i1 : 0);
        const float* c = vl + (ok ? 3 * i2 : 0);
        const float h = wn_face(a[0] - px, a[1] - py, a[2] - pz, b[0] - px, b[1] - py, b[2] - pz, c[0] - px, c[1] - py, c[2] - pz);
        acc += (double)(ok ? h : 0.f);
    }
    return (float)(acc * WN_INV_2PI);
}

// the frame's 3 V floats into LDS (the caller synchronises)
__device__ __forceinline__ void wn_load_frame(const float* __restrict__ vf, int V, float* vl, int tid) {
    for (int e = tid; e < 3 * V; e += WN_THREADS) vl[e] = vf[e];
}

__device__ __forceinline__ float wn_wave_min(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ float wn_wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}

// slices of the cloud per frame: one when the frames alone fill the chip twice, otherwise enough to get there
static int wn_slices(int F, int P) {
    const int nblk = (P + WN_THREADS - 1) / WN_THREADS;
    const int want = (512 + F - 1) / F;
    return want < 1 ? 1 : (want > nblk ? nblk : want);
}

__global__ __launch_bounds__(WN_THREADS) void k_mesh_winding(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                             int NF, const float* __restrict__ points,
                                                             const int32_t* __restrict__ points_of_frame, int V, int S, int P, int NS,
                                                             float* __restrict__ out_w) {
    extern __shared__ __attribute__((aligned(16))) float wn_lds[];       // [3 V] the frame's vertices
    const int tid = threadIdx.x;
    const int f = blockIdx.x / NS, sl = blockIdx.x - f * NS;
    const int sc = points_of_frame[f];
    const int nblk = (P + WN_THREADS - 1) / WN_THREADS;
    const int b0 = (int)((long)sl * nblk / NS), b1 = (int)((long)(sl + 1) * nblk / NS);
    float* wf = out_w + (size_t)f * P;
    if (sc < 0 || sc >= S) {                                             // skipped frame: zeros
        for (int blk = b0; blk < b1; ++blk) {
            const int p = blk * WN_THREADS + tid;
            if (p < P) wf[p] = 0.f;
        }
        return;
    }
    wn_load_frame(verts + (size_t)f * V * 3, V, wn_lds, tid);
    __syncthreads();
    const float* pp = points + (size_t)sc * P * 3;
    for (int blk = b0; blk < b1; ++blk) {
        const int base = blk * WN_THREADS + (tid & ~63);
        if (base >= P) continue;                                         // wave-uniform
        const int p = base + (tid & 63);
        const int q = p < P ? p : P - 1;                                 // lanes past the end repeat the last point, store nothing
        const float w = wn_point(wn_lds, faces, NF, V, pp[(size_t)q * 3], pp[(size_t)q * 3 + 1], pp[(size_t)q * 3 + 2]);
        if (p < P) wf[p] = w;
    }
}

__global__ __launch_bounds__(WN_THREADS) void k_inside_count(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                             int NF, const float* __restrict__ scene,
                                                             const int32_t* __restrict__ scene_of_frame, int V, int S, int P, int NS,
                                                             int32_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float wn_lds[];       // [3 V] vertices, then [WN_QUEUE][3] the queued points
    __shared__ float red[6][WN_WAVES];
    __shared__ int wcnt[WN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x / NS, sl = blockIdx.x - f * NS;
    const int sc = scene_of_frame[f];
    if (sc < 0 || sc >= S) {                                             // skipped frame
        if (tid == 0) partial[blockIdx.x] = 0;
        return;
    }
    float* queue = wn_lds + 3 * V;
    wn_load_frame(verts + (size_t)f * V * 3, V, wn_lds, tid);
    __syncthreads();

    // the closed bounding box (min and max are exact: every slice of the frame gets the same bits)
    float lo0 = WN_INF, lo1 = WN_INF, lo2 = WN_INF, hi0 = -WN_INF, hi1 = -WN_INF, hi2 = -WN_INF;
    for (int n = tid; n < V; n += WN_THREADS) {
        const float x = wn_lds[3 * n], y = wn_lds[3 * n + 1], z = wn_lds[3 * n + 2];
        lo0 = fminf(lo0, x); lo1 = fminf(lo1, y); lo2 = fminf(lo2, z);
        hi0 = fmaxf(hi0, x); hi1 = fmaxf(hi1, y); hi2 = fmaxf(hi2, z);
    }
    lo0 = wn_wave_min(lo0); lo1 = wn_wave_min(lo1); lo2 = wn_wave_min(lo2);
    hi0 = wn_wave_max(hi0); hi1 = wn_wave_max(hi1); hi2 = wn_wave_max(hi2);
    if (lane == 0) {
        red[0][wave] = lo0; red[1][wave] = lo1; red[2][wave] = lo2;
        red[3][wave] = hi0; red[4][wave] = hi1; red[5][wave] = hi2;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WN_WAVES; ++w) {
        lo0 = fminf(lo0, red[0][w]); lo1 = fminf(lo1, red[1][w]); lo2 = fminf(lo2, red[2][w]);
        hi0 = fmaxf(hi0, red[3][w]); hi1 = fmaxf(hi1, red[4][w]); hi2 = fmaxf(hi2, red[5][w]);
    }

    const float* sp = scene + (size_t)sc * P * 3;
    const int nblk = (P + WN_THREADS - 1) / WN_THREADS;
    const int b0 = (int)((long)sl * nblk / NS), b1 = (int)((long)(sl + 1) * nblk / NS);
    int qn = 0, inside = 0;                                              // qn: queued points (the same in every thread), < WN_THREADS
    for (int blk = b0; blk <= b1; ++blk) {
        if (blk < b1) {                                                  // queue the survivors of this step
            const int p = blk * WN_THREADS + tid;
            float x = 0.f, y = 0.f, z = 0.f;
            bool in = false;
            if (p < P) {
                x = sp[(size_t)p * 3]; y = sp[(size_t)p * 3 + 1]; z = sp[(size_t)p * 3 + 2];
                in = x >= lo0 && x <= hi0 && y >= lo1 && y <= hi1 && z >= lo2 && z <= hi2;
            }
            const unsigned long long m = __ballot(in);
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int off = qn, tot = 0;
#pragma unroll
            for (int w = 0; w < WN_WAVES; ++w) {
                const int c = wcnt[w];
                off += w < wave ? c : 0;
                tot += c;
            }
            if (in) {
                float* q = queue + 3 * (off + __popcll(m & ((1ull << lane) - 1ull)));      // < 3 WN_QUEUE: qn < 512, tot <= 512
                q[0] = x; q[1] = y; q[2] = z;
            }
            qn += tot;
            __syncthreads();
            if (qn < WN_THREADS) continue;
        } else if (qn == 0) {
            break;
        }
        // one round: the first min(qn, 512) queued points, one per lane
        const int n = qn < WN_THREADS ? qn : WN_THREADS;
        if (wave * 64 < n) {                                             // wave-uniform
            const int q = tid < n ? tid : n - 1;                         // idle lanes repeat a point and count nothing
            const float w = wn_point(wn_lds, faces, NF, V, queue[3 * q], queue[3 * q + 1], queue[3 * q + 2]);
            inside += (tid < n && fabsf(w) >= 0.5f) ? 1 : 0;
        }
        qn -= n;
        float x = 0.f, y = 0.f, z = 0.f;                                 // the rest of the queue moves to its front
        if (tid < qn) { x = queue[3 * (n + tid)]; y = queue[3 * (n + tid) + 1]; z = queue[3 * (n + tid) + 2]; }
        __syncthreads();
        if (tid < qn) { queue[3 * tid] = x; queue[3 * tid + 1] = y; queue[3 * tid + 2] = z; }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) inside += __shfl_xor(inside, o, 64);
    __syncthreads();                                                     // wcnt is free again
    if (lane == 0) wcnt[wave] = inside;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < WN_WAVES; ++w) s += wcnt[w];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void k_inside_finish(const int32_t* __restrict__ partial, int F, int NS, int32_t* __restrict__ out) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    int s = 0;
    for (int i = 0; i < NS; ++i) s += partial[(size_t)f * NS + i];
    out[f] = s;
}

// ----------------------------------------------------------------------------------------------------------------- C-ABI
static int wn_check(const char* who, const void* verts, const void* faces, int NF, const void* pts, const void* map, int F, int V,
                    int S, int P, const void* out) {
    char msg[160];
    const char* bad = nullptr;
    if (F < 1) bad = "F must be >= 1";
    else if (V < 1 || V > WN_VMAX) bad = "V must be in 1..10112";
    else if (NF < 1) bad = "NF must be >= 1";
    else if (S < 1) bad = "S must be >= 1";
    else if (P < 1) bad = "P must be >= 1";
    else if (!verts || !faces || !pts || !map || !out) bad = "null pointer";
    else if ((long)F * wn_slices(F, P) > 0x7fffffffL) bad = "too many frames for one launch";
    if (!bad) return 0;
    snprintf(msg, sizeof msg, "%s: %s", who, bad);
    return seeme_fail(msg);
}

extern "C" size_t seeme_scene_inside_count_workspace_bytes(int F, int V, int S, int P) {
    if (F < 1 || V < 1 || V > WN_VMAX || S < 1 || P < 1) return 0;
    return (size_t)F * wn_slices(F, P) * sizeof(int32_t);
}

extern "C" int seeme_scene_inside_count(const float* verts, const int32_t* faces, int NF, const float* scene,
                                        const int32_t* scene_of_frame, int F, int V, int S, int P, int32_t* out_count, void* ws,
                                        size_t ws_bytes, void* stream) {
    if (int rc = wn_check("scene_inside_count", verts, faces, NF, scene, scene_of_frame, F, V, S, P, out_count)) return rc;
    if (!ws) return seeme_fail("scene_inside_count: null pointer");
    if ((uintptr_t)ws & 15) return seeme_fail("scene_inside_count: workspace must be 16-byte aligned");
    if (ws_bytes < seeme_scene_inside_count_workspace_bytes(F, V, S, P)) return seeme_fail("scene_inside_count: workspace too small");
    const int NS = wn_slices(F, P);
    const size_t lds = ((size_t)3 * V + 3 * WN_QUEUE) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    SEEME_HIP(hipFuncSetAttribute((const void*)k_inside_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_inside_count, dim3(F * NS), dim3(WN_THREADS), lds, st, verts, faces, NF, scene, scene_of_frame, V, S, P, NS,
                       (int32_t*)ws);
    if (int rc = seeme_check_launch("k_inside_count")) return rc;
    hipLaunchKernelGGL(k_inside_finish, dim3((F + 63) / 64), dim3(64), 0, st, (const int32_t*)ws, F, NS, out_count);
    return seeme_check_launch("k_inside_finish");
}

extern "C" int seeme_mesh_winding(const float* verts, const int32_t* faces, int NF, const float* points,
                                  const int32_t* points_of_frame, int F, int V, int S, int P, float* out_w, void* stream) {
    if (int rc = wn_check("mesh_winding", verts, faces, NF, points, points_of_frame, F, V, S, P, out_w)) return rc;
    const int NS = wn_slices(F, P);
    const size_t lds = (size_t)3 * V * sizeof(float);
    SEEME_HIP(hipFuncSetAttribute((const void*)k_mesh_winding, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_mesh_winding, dim3(F * NS), dim3(WN_THREADS), lds, (hipStream_t)stream, verts, faces, NF, points,
                       points_of_frame, V, S, P, NS, out_w);
    return seeme_check_launch("k_mesh_winding");
}
