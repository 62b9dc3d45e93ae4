// scene_views.hip -- the view-dependent selection of a scene mesh's vertices for W camera poses in one call (seeme_scene_views):
// into the view's frame, keep z > 0, every k-th survivor in vertex order, the first P.  Definition: include/seeme_hip.h; the plain-torch
// twin is seeme_amd/recording.py scene_views_torch.  fp32, no atomics: every output row has ONE owner, found from ranks alone.
//
// Plan.  A workgroup (256 lanes) owns a tile of SV_TILE consecutive vertices and a chunk of SV_WPP views: the tile is read once
// (coalesced dword loads into LDS, then 4 vertices per lane in registers) and the views are walked over it, rows 0..2 of their
// matrices in LDS as well: no global load inside the walk.  So the vertices are read ceil(W / SV_WPP) times per pass.
//   k_scene_views_count  pass 1: the survivors of every (view, tile) -> workspace [W][NT]
//   k_scene_views_scan   one workgroup per view: exclusive prefix of its tile counts in place, count[w]; a view without survivors
//                        gets its zero rows and index -1 here
//   k_scene_views_write  pass 2: the predicate again (the same fmaf chain, so the same bits), a survivor's rank = tile offset + the
//                        survivors of the earlier (slot, wave) groups of the tile (ballot counts through LDS) + the survivors on lower
//                        lanes of its own ballot; the survivor writes the rows it owns.
// A lane's vertex q (0..3) is tile*SV_TILE + (q*4 + wave)*64 + lane: vertex order is (q, wave, lane) order.
#include "api_util.hpp"
#include <stdint.h>

#define SV_THREADS 256
#define SV_TILE SEEME_SCENE_VIEW_TILE
#define SV_WPP SEEME_SCENE_VIEW_WINDOWS_PER_PASS
#define SV_WAVES (SV_THREADS / 64)
#define SV_VPT (SV_TILE / SV_THREADS)          // vertices per lane (4)
#define SV_GROUPS (SV_VPT * SV_WAVES)          // 64-vertex groups of a tile (16)
#define SV_NMAX (1 << 24)
#define SV_WMAX 4096
#define SV_PMAX (1 << 20)

static_assert(SV_TILE % SV_THREADS == 0 && SV_THREADS % 64 == 0 && SV_WPP <= SV_THREADS, "scene_views tiling");

struct SvVerts {
    float x[SV_VPT], y[SV_VPT], z[SV_VPT];
    bool ok[SV_VPT];
};

// one row of a view's matrix applied to a vertex: THE expression of the definition (classification and written coordinate)
__device__ __forceinline__ float sv_coord(const float* __restrict__ m, float x, float y, float z) {
    return fmaf(m[2], z, fmaf(m[1], y, fmaf(m[0], x, m[3])));
}

// the tile's floats and rows 0..2 of the chunk's nw matrices into LDS (nothing past 3*N is read), then this lane's vertices into
// registers; a vertex past N is not ok.  The walk over the views then waits for no global load.
__device__ __forceinline__ void sv_load_tile(const float* __restrict__ verts, int N, int tile, float* lds, SvVerts& v,
                                             const float* __restrict__ M, int nw, float (*mat)[12]) {
    const int tid = threadIdx.x;
    const int first = tile * SV_TILE, nv = min(SV_TILE, N - first);
    const float* src = verts + (size_t)first * 3;
    for (int i = tid; i < 3 * nv; i += SV_THREADS) lds[i] = src[i];
    if (tid < nw * 12) mat[tid / 12][tid % 12] = M[(size_t)(tid / 12) * 16 + tid % 12];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SV_VPT; ++q) {
        const int l = q * SV_THREADS + tid;
        v.ok[q] = l < nv;
        v.x[q] = v.ok[q] ? lds[3 * l] : 0.f;
        v.y[q] = v.ok[q] ? lds[3 * l + 1] : 0.f;
        v.z[q] = v.ok[q] ? lds[3 * l + 2] : 0.f;
    }
}

__global__ __launch_bounds__(SV_THREADS) void k_scene_views_count(const float* __restrict__ verts, const float* __restrict__ M, int N,
                                                                  int W, int NT, int32_t* __restrict__ tile_cnt) {
    __shared__ float lds[3 * SV_TILE];
    __shared__ int cnt[SV_WPP][SV_WAVES];
    __shared__ float mat[SV_WPP][12];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
    const int w0 = blockIdx.y * SV_WPP, nw = min(SV_WPP, W - w0);
    SvVerts v;
    sv_load_tile(verts, N, tile, lds, v, M + (size_t)w0 * 16, nw, mat);
    for (int wi = 0; wi < nw; ++wi) {
        const float* m = mat[wi] + 8;                                 // row 2: the view's depth
        int c = 0;
#pragma unroll
        for (int q = 0; q < SV_VPT; ++q) c += __popcll(__ballot(v.ok[q] && sv_coord(m, v.x[q], v.y[q], v.z[q]) > 0.f));
        if (lane == 0) cnt[wi][wave] = c;
    }
    __syncthreads();
    if (tid < nw) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < SV_WAVES; ++i) c += cnt[tid][i];
        tile_cnt[(size_t)(w0 + tid) * NT + tile] = c;
    }
}

// one workgroup per view: lane t sums a run of consecutive tiles, lane 0 scans the 256 run sums, every lane rewrites its run
__global__ __launch_bounds__(SV_THREADS) void k_scene_views_scan(int32_t* __restrict__ tile_cnt, int NT, int P, float* __restrict__ cloud,
                                                                 int32_t* __restrict__ index, int32_t* __restrict__ count) {
    __shared__ int part[SV_THREADS + 1];
    const int tid = threadIdx.x, w = blockIdx.x;
    int32_t* c = tile_cnt + (size_t)w * NT;
    const int per = (NT + SV_THREADS - 1) / SV_THREADS;
    const int lo = min(tid * per, NT), hi = min(lo + per, NT);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += c[i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < SV_THREADS; ++i) {
            const int t = part[i];
            part[i] = run;
            run += t;
        }
        part[SV_THREADS] = run;
        count[w] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int i = lo; i < hi; ++i) {
        const int t = c[i];
        c[i] = run;
        run += t;
    }
    if (part[SV_THREADS] == 0) {                                      // no survivor: no lane of pass 2 owns a row of this view
        const size_t row0 = (size_t)w * P;
        for (int j = tid; j < P; j += SV_THREADS) {
            float* o = cloud + (row0 + j) * 3;
            o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
            index[row0 + j] = -1;
        }
    }
}

__global__ __launch_bounds__(SV_THREADS) void k_scene_views_write(const float* __restrict__ verts, const float* __restrict__ M, int N,
                                                                  int W, int P, int NT, const int32_t* __restrict__ tile_off,
                                                                  const int32_t* __restrict__ count, float* __restrict__ cloud,
                                                                  int32_t* __restrict__ index) {
    __shared__ float lds[3 * SV_TILE];
    __shared__ int cnt[SV_WPP][SV_GROUPS];
    __shared__ float mat[SV_WPP][12];
    __shared__ int meta[SV_WPP][2];                                   // a view's survivors, and those of the tiles before this one
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
    const int w0 = blockIdx.y * SV_WPP, nw = min(SV_WPP, W - w0);
    if (tid < nw) {
        meta[tid][0] = count[w0 + tid];
        meta[tid][1] = tile_off[(size_t)(w0 + tid) * NT + tile];
    }
    SvVerts v;
    sv_load_tile(verts, N, tile, lds, v, M + (size_t)w0 * 16, nw, mat);
    for (int wi = 0; wi < nw; ++wi) {                                 // the survivors of every 64-vertex group, per view
        const float* m = mat[wi] + 8;
#pragma unroll
        for (int q = 0; q < SV_VPT; ++q) {
            const int c = __popcll(__ballot(v.ok[q] && sv_coord(m, v.x[q], v.y[q], v.z[q]) > 0.f));
            if (lane == 0) cnt[wi][q * SV_WAVES + wave] = c;
        }
    }
    __syncthreads();
    for (int wi = 0; wi < nw; ++wi) {
        const int w = w0 + wi;
        const int total = meta[wi][0];
        if (total == 0) continue;                                     // (uniform; k_scene_views_scan wrote the view)
        const float* m = mat[wi];
        const int k = total >= P ? total / P : 0;                     // 0: fewer survivors than rows, cyclic fill
        const float inv_k = 1.f / (float)max(k, 1);
        const size_t row0 = (size_t)w * P;
        int run = meta[wi][1];
        int base[SV_VPT];                                             // rank of the first survivor of this wave's group q
#pragma unroll
        for (int q = 0; q < SV_VPT; ++q) {
            base[q] = 0;
#pragma unroll
            for (int i = 0; i < SV_WAVES; ++i) {
                if (i == wave) base[q] = run;
                run += cnt[wi][q * SV_WAVES + i];
            }
        }
#pragma unroll
        for (int q = 0; q < SV_VPT; ++q) {
            const float zc = sv_coord(m + 8, v.x[q], v.y[q], v.z[q]);
            const bool s = v.ok[q] && zc > 0.f;
            const unsigned long long b = __ballot(s);
            if (s) {
                const int rank = base[q] + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
                const float xc = sv_coord(m, v.x[q], v.y[q], v.z[q]), yc = sv_coord(m + 4, v.x[q], v.y[q], v.z[q]);
                const int src = tile * SV_TILE + q * SV_THREADS + tid;
                if (k) {                                              // row j holds rank j*k, j < P
                    // rank, k < 2^24 + 1 are exact in fp32 and rank * inv_k is within 2^-22 relative of rank / k: when rank is
                    // j*k with j < P <= 2^20 the product is within 0.25 of j and rounds to it; any other j fails the exact test
                    const int j = (int)rintf((float)rank * inv_k);
                    if (j * k == rank && j < P) {
                        float* o = cloud + (row0 + j) * 3;
                        o[0] = xc; o[1] = yc; o[2] = zc;
                        index[row0 + j] = src;
                    }
                } else {                                              // row j holds rank j mod total
                    for (int j = rank; j < P; j += total) {
                        float* o = cloud + (row0 + j) * 3;
                        o[0] = xc; o[1] = yc; o[2] = zc;
                        index[row0 + j] = src;
                    }
                }
            }
        }
    }
}

extern "C" size_t seeme_scene_views_workspace_bytes(int N, int W, int P) {
    if (N < 1 || N > SV_NMAX || W < 1 || W > SV_WMAX || P < 1 || P > SV_PMAX) return 0;
    return (size_t)W * ((N + SV_TILE - 1) / SV_TILE) * sizeof(int32_t);
}

extern "C" int seeme_scene_views(const float* verts, const float* M, int N, int W, int P, float* cloud, int32_t* index, int32_t* count,
                                 void* ws, size_t ws_bytes, void* stream) {
    if (N < 1 || N > SV_NMAX) return seeme_fail("scene_views: N must be in 1..2^24");
    if (W < 1 || W > SV_WMAX) return seeme_fail("scene_views: W must be in 1..4096");
    if (P < 1 || P > SV_PMAX) return seeme_fail("scene_views: P must be in 1..2^20");
    if (!verts || !M || !cloud || !index || !count || !ws) return seeme_fail("scene_views: null pointer");
    if (((uintptr_t)verts | (uintptr_t)M | (uintptr_t)cloud | (uintptr_t)index | (uintptr_t)count | (uintptr_t)ws) & 3)
        return seeme_fail("scene_views: pointers must be 4-byte aligned");
    if (ws_bytes < seeme_scene_views_workspace_bytes(N, W, P)) return seeme_fail("scene_views: workspace too small");
    const int NT = (N + SV_TILE - 1) / SV_TILE, chunks = (W + SV_WPP - 1) / SV_WPP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_scene_views_count, dim3(NT, chunks), dim3(SV_THREADS), 0, st, verts, M, N, W, NT, (int32_t*)ws);
    if (int rc = seeme_check_launch("k_scene_views_count")) return rc;
    hipLaunchKernelGGL(k_scene_views_scan, dim3(W), dim3(SV_THREADS), 0, st, (int32_t*)ws, NT, P, cloud, index, count);
    if (int rc = seeme_check_launch("k_scene_views_scan")) return rc;
    hipLaunchKernelGGL(k_scene_views_write, dim3(NT, chunks), dim3(SV_THREADS), 0, st, verts, M, N, W, P, NT, (const int32_t*)ws,
                       (const int32_t*)count, cloud, index);
    return seeme_check_launch("k_scene_views_write");
}
