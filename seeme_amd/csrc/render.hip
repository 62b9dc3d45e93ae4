// render.hip -- mesh and point-cloud rasteriser: per pixel the id and the inverse depth of the nearest primitive (seeme_render), and a
// flat-shaded RGB image from the ids (seeme_render_shade).  Definition: include/seeme_hip.h (an integer one after the vertex stage:
// 1/16-pixel snapped corners, int64 edge functions with a tie rule, a 22-bit inverse depth); the plain-torch twin is
// seeme_amd/render.py render_torch / shade_torch and the two agree bit for bit on ids, inv_depth and dropped.
//
// Plan.  A pixel's result is the MAXIMUM of a 64-bit key over everything that covers it, so the order of arrival does
// not matter and a vector atomic max on a key image gives the same bits as any other plan.
//   k_render_project   one lane per (frame, vertex): the vertex stage in double -> X, Y, Q, valid (16 bytes) in the workspace
//   k_render_faces     one lane per (frame, face): the face's box clamped to the image; a box of at most RD_WAVE_BOX pixels is walked
//                      by its lane, a larger one by the whole wave (ballot, then the corners broadcast lane by lane), so that one
//                      screen-filling triangle does not serialise the frame on one lane.  Covered pixel: atomicMax on the key.
//   k_render_points    one lane per (frame, point): the vertex stage again and the point's square
//   k_render_resolve   one lane per pixel: key -> id, inverse depth
//   k_render_shade     one lane per pixel: id -> colour; a face pixel recomputes its three camera-space corners in fp32
// blockIdx.y is the frame (F <= 65535).  The key image and dropped are cleared with hipMemsetAsync on the same stream.
#include "api_util.hpp"
#include <float.h>
#include <stdint.h>

#define RD_THREADS 256
#define RD_WAVE_BOX 256                        // box pixels above which the wave walks the box together
#define RD_FMAX 65535
#define RD_NVMAX (1 << 24)
#define RD_PRIM_MAX 2147483646LL               // NF + P <= 2^31 - 2

struct __attribute__((aligned(16))) RdVert {
    int X, Y, Q, ok;
};

struct RdCam {
    float fx, fy, cx, cy, znear;
};

// THE vertex stage of the definition: double, every operation rounded on its own, rows left to right
__device__ __forceinline__ RdVert rd_project(const float* __restrict__ m, float x, float y, float z, const RdCam k) {
#pragma clang fp contract(off)
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    const double xc = (((double)m[0] * xd + (double)m[1] * yd) + (double)m[2] * zd) + (double)m[3];
    const double yc = (((double)m[4] * xd + (double)m[5] * yd) + (double)m[6] * zd) + (double)m[7];
    const double zc = (((double)m[8] * xd + (double)m[9] * yd) + (double)m[10] * zd) + (double)m[11];
    RdVert v = {0, 0, 0, 0};
    if (!(zc >= (double)k.znear) || !(zc <= DBL_MAX)) return v;       // (a NaN fails the first comparison, +inf the second)
    const double X = rint((((double)k.fx * xc) / zc + (double)k.cx) * 16.0);
    const double Y = rint((((double)k.fy * yc) / zc + (double)k.cy) * 16.0);
    const double lim = (double)SEEME_RENDER_COORD_MAX;
    if (!(fabs(X) <= lim) || !(fabs(Y) <= lim)) return v;             // (NaN and inf fail)
    v.X = (int)X;
    v.Y = (int)Y;
    v.Q = (int)rint(((double)k.znear / zc) * (double)SEEME_RENDER_Q);
    v.ok = 1;
    return v;
}

__global__ __launch_bounds__(RD_THREADS) void k_render_project(const float* __restrict__ verts, const float* __restrict__ cams, int FC,
                                                               int NV, RdCam k, RdVert* __restrict__ pv) {
    const int v = blockIdx.x * RD_THREADS + threadIdx.x, f = blockIdx.y;
    if (v >= NV) return;
    const float* m = cams + (size_t)(FC == 1 ? 0 : f) * 16;
    const float* p = verts + ((size_t)f * (size_t)NV + (size_t)v) * 3;
    pv[(size_t)f * (size_t)NV + (size_t)v] = rd_project(m, p[0], p[1], p[2], k);
}

// a face ready to be walked: corners after the swap that makes area2 positive
struct RdFace {
    int ax, ay, aq, bx, by, bq, cx, cy, cq;
};

// w >= 0 counts as inside on the edges the tie rule gives to this triangle
__device__ __forceinline__ bool rd_inside(long long w, int dx, int dy) {
    return w > 0 || (w == 0 && (dy > 0 || (dy == 0 && dx < 0)));
}

// one pixel (row i, col j) of one face: the three edge functions, the tie rule, the inverse depth, the key
__device__ __forceinline__ void rd_pixel(unsigned long long* __restrict__ keys, int W, int i, int j, const RdFace t, long long area2,
                                         uint32_t id) {
    const long long px = 16LL * j, py = 16LL * i;
    const int d0x = t.cx - t.bx, d0y = t.cy - t.by;                   // edge B -> C
    const int d1x = t.ax - t.cx, d1y = t.ay - t.cy;                   // edge C -> A
    const int d2x = t.bx - t.ax, d2y = t.by - t.ay;                   // edge A -> B
    const long long w0 = (long long)d0x * (py - t.by) - (long long)d0y * (px - t.bx);
    const long long w1 = (long long)d1x * (py - t.cy) - (long long)d1y * (px - t.cx);
    const long long w2 = (long long)d2x * (py - t.ay) - (long long)d2y * (px - t.ax);
    if (!(rd_inside(w0, d0x, d0y) && rd_inside(w1, d1x, d1y) && rd_inside(w2, d2x, d2y))) return;
    const long long num = w0 * t.aq + w1 * t.bq + w2 * t.cq;          // 0 <= num <= 2^22 area2 <= 2^61 (header)
    const unsigned long long q = (unsigned long long)num / (unsigned long long)area2;
    atomicMax(keys + (size_t)i * (size_t)W + (size_t)j, (q << 32) | (unsigned long long)(0xFFFFFFFFu - id));
}

__global__ __launch_bounds__(RD_THREADS) void k_render_faces(const int32_t* __restrict__ faces, int NF, int NV,
                                                             const RdVert* __restrict__ pv, int H, int W,
                                                             unsigned long long* __restrict__ keys, int32_t* __restrict__ dropped) {
    const int face = blockIdx.x * RD_THREADS + threadIdx.x, f = blockIdx.y, lane = threadIdx.x & 63;
    unsigned long long* kf = keys + (size_t)f * (size_t)H * (size_t)W;
    bool have = face < NF;                                            // no early return: every lane reaches the ballot below
    RdFace t = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int j0 = 0, i0 = 0, bw = 0, npx = 0;
    if (have) {
        const int ia = faces[(size_t)face * 3], ib = faces[(size_t)face * 3 + 1], ic = faces[(size_t)face * 3 + 2];
        have = ia >= 0 && ia < NV && ib >= 0 && ib < NV && ic >= 0 && ic < NV;
        if (have) {
            const RdVert* fv = pv + (size_t)f * (size_t)NV;
            const RdVert A = fv[ia], B = fv[ib], C = fv[ic];
            if (!(A.ok && B.ok && C.ok)) {
                atomicAdd(dropped + f, 1);
                have = false;
            } else {
                const long long area2 = (long long)(B.X - A.X) * (C.Y - A.Y) - (long long)(B.Y - A.Y) * (C.X - A.X);
                const bool sw = area2 < 0;
                t.ax = A.X; t.ay = A.Y; t.aq = A.Q;
                t.bx = sw ? C.X : B.X; t.by = sw ? C.Y : B.Y; t.bq = sw ? C.Q : B.Q;
                t.cx = sw ? B.X : C.X; t.cy = sw ? B.Y : C.Y; t.cq = sw ? B.Q : C.Q;
                const int xmin = min(A.X, min(B.X, C.X)), xmax = max(A.X, max(B.X, C.X));
                const int ymin = min(A.Y, min(B.Y, C.Y)), ymax = max(A.Y, max(B.Y, C.Y));
                j0 = max(0, (xmin + 15) >> 4);                        // the first and last sample inside the box, clamped
                i0 = max(0, (ymin + 15) >> 4);
                const int j1 = min(W - 1, xmax >> 4), i1 = min(H - 1, ymax >> 4);
                have = area2 != 0 && j0 <= j1 && i0 <= i1;
                if (have) {
                    bw = j1 - j0 + 1;
                    npx = bw * (i1 - i0 + 1);                         // <= 2^24
                }
            }
        }
    }
    const bool big = have && npx > RD_WAVE_BOX;
    if (have && !big) {
        const long long area2 = (long long)(t.bx - t.ax) * (t.cy - t.ay) - (long long)(t.by - t.ay) * (t.cx - t.ax);
        for (int idx = 0; idx < npx; ++idx) rd_pixel(kf, W, i0 + idx / bw, j0 + idx % bw, t, area2, (uint32_t)face);
    }
    unsigned long long todo = __ballot(big);
    while (todo) {                                                    // (wave-uniform)
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        RdFace s;
        s.ax = __shfl(t.ax, src); s.ay = __shfl(t.ay, src); s.aq = __shfl(t.aq, src);
        s.bx = __shfl(t.bx, src); s.by = __shfl(t.by, src); s.bq = __shfl(t.bq, src);
        s.cx = __shfl(t.cx, src); s.cy = __shfl(t.cy, src); s.cq = __shfl(t.cq, src);
        const int sj0 = __shfl(j0, src), si0 = __shfl(i0, src), sbw = __shfl(bw, src), snpx = __shfl(npx, src);
        const int sface = __shfl(face, src);
        const long long area2 = (long long)(s.bx - s.ax) * (s.cy - s.ay) - (long long)(s.by - s.ay) * (s.cx - s.ax);
        for (int idx = lane; idx < snpx; idx += 64) rd_pixel(kf, W, si0 + idx / sbw, sj0 + idx % sbw, s, area2, (uint32_t)sface);
    }
}

__global__ __launch_bounds__(RD_THREADS) void k_render_points(const float* __restrict__ points, int P, int NF,
                                                              const float* __restrict__ cams, int FC, RdCam k, int H, int W,
                                                              int point_size, unsigned long long* __restrict__ keys) {
    const int p = blockIdx.x * RD_THREADS + threadIdx.x, f = blockIdx.y;
    if (p >= P) return;
    const float* m = cams + (size_t)(FC == 1 ? 0 : f) * 16;
    const RdVert v = rd_project(m, points[(size_t)p * 3], points[(size_t)p * 3 + 1], points[(size_t)p * 3 + 2], k);
    if (!v.ok) return;
    const int j = (v.X + 8) >> 4, i = (v.Y + 8) >> 4;
    const int lo = -((point_size - 1) / 2), hi = point_size / 2;
    const int ja = max(0, j + lo), jb = min(W - 1, j + hi), ia = max(0, i + lo), ib = min(H - 1, i + hi);
    const unsigned long long key = ((unsigned long long)v.Q << 32) | (unsigned long long)(0xFFFFFFFFu - ((uint32_t)NF + (uint32_t)p));
    unsigned long long* kf = keys + (size_t)f * (size_t)H * (size_t)W;
    for (int r = ia; r <= ib; ++r)
        for (int c = ja; c <= jb; ++c) atomicMax(kf + (size_t)r * (size_t)W + (size_t)c, key);
}

__global__ __launch_bounds__(RD_THREADS) void k_render_resolve(const unsigned long long* __restrict__ keys, int HW,
                                                               int32_t* __restrict__ ids, int32_t* __restrict__ inv_depth) {
    const int px = blockIdx.x * RD_THREADS + threadIdx.x;
    if (px >= HW) return;
    const size_t at = (size_t)blockIdx.y * (size_t)HW + (size_t)px;
    const unsigned long long key = keys[at];
    ids[at] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
    inv_depth[at] = (int32_t)(key >> 32);
}

__global__ __launch_bounds__(RD_THREADS) void k_render_shade(const float* __restrict__ verts, const int32_t* __restrict__ faces, int NV,
                                                             int NF, int P, const float* __restrict__ cams, int FC,
                                                             const int32_t* __restrict__ ids, const int32_t* __restrict__ mesh_of_face,
                                                             const uint8_t* __restrict__ palette, int n_mesh,
                                                             const uint8_t* __restrict__ point_rgb, uint32_t bg, int HW,
                                                             uint8_t* __restrict__ rgb) {
    const int px = blockIdx.x * RD_THREADS + threadIdx.x, f = blockIdx.y;
    if (px >= HW) return;
    const size_t at = (size_t)f * (size_t)HW + (size_t)px;
    const int id = ids[at];
    uint8_t r = (uint8_t)(bg & 255u), g = (uint8_t)((bg >> 8) & 255u), b = (uint8_t)((bg >> 16) & 255u);
    if (id >= NF) {
        const long long p = (long long)id - NF;
        if (p < P) {
            r = point_rgb[(size_t)p * 3]; g = point_rgb[(size_t)p * 3 + 1]; b = point_rgb[(size_t)p * 3 + 2];
        }
    } else if (id >= 0) {
        const int ia = faces[(size_t)id * 3], ib = faces[(size_t)id * 3 + 1], ic = faces[(size_t)id * 3 + 2];
        const int mesh = mesh_of_face[id];
        if (ia >= 0 && ia < NV && ib >= 0 && ib < NV && ic >= 0 && ic < NV && mesh >= 0 && mesh < n_mesh) {
            const float* m = cams + (size_t)(FC == 1 ? 0 : f) * 16;
            const float* fv = verts + (size_t)f * (size_t)NV * 3;
            float c[3][3];
            const int idx[3] = {ia, ib, ic};
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float x = fv[(size_t)idx[q] * 3], y = fv[(size_t)idx[q] * 3 + 1], z = fv[(size_t)idx[q] * 3 + 2];
#pragma unroll
                for (int d = 0; d < 3; ++d) c[q][d] = ((m[4 * d] * x + m[4 * d + 1] * y) + m[4 * d + 2] * z) + m[4 * d + 3];
            }
            const float ux = c[1][0] - c[0][0], uy = c[1][1] - c[0][1], uz = c[1][2] - c[0][2];
            const float vx = c[2][0] - c[0][0], vy = c[2][1] - c[0][1], vz = c[2][2] - c[0][2];
            const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const float len = sqrtf(nx * nx + ny * ny + nz * nz);
            const float level = 0.3f + 0.7f * (len > 0.f ? fabsf(nz) / len : 0.f);
            r = (uint8_t)fminf(255.f, floorf((float)palette[mesh * 3] * level + 0.5f));
            g = (uint8_t)fminf(255.f, floorf((float)palette[mesh * 3 + 1] * level + 0.5f));
            b = (uint8_t)fminf(255.f, floorf((float)palette[mesh * 3 + 2] * level + 0.5f));
        }
    }
    uint8_t* o = rgb + at * 3;
    o[0] = r; o[1] = g; o[2] = b;
}

static size_t rd_key_bytes(int F, int H, int W) {
    return ((size_t)F * (size_t)H * (size_t)W * sizeof(unsigned long long) + 15) & ~(size_t)15;
}

extern "C" size_t seeme_render_workspace_bytes(int F, int NV, int H, int W) {
    if (F < 1 || F > RD_FMAX || NV < 0 || NV > RD_NVMAX || H < 1 || H > SEEME_RENDER_SIZE_MAX || W < 1 || W > SEEME_RENDER_SIZE_MAX)
        return 0;
    return rd_key_bytes(F, H, W) + (size_t)F * (size_t)NV * sizeof(RdVert);
}

// the checks both entry points share; NULL when the scene is usable
static const char* rd_scene_error(const SeemeRenderScene* s) {
    if (!s) return "render: scene is a null pointer";
    if (s->F < 1 || s->F > RD_FMAX) return "render: F must be in 1..65535";
    if (s->FC != 1 && s->FC != s->F) return "render: FC must be 1 or F";
    if (s->H < 1 || s->H > SEEME_RENDER_SIZE_MAX || s->W < 1 || s->W > SEEME_RENDER_SIZE_MAX) return "render: H and W must be in 1..4096";
    if (s->NV < 0 || s->NV > RD_NVMAX) return "render: NV must be in 0..2^24";
    if (s->NF < 0 || s->P < 0 || (long long)s->NF + (long long)s->P > RD_PRIM_MAX) return "render: NF, P must be >= 0 with NF + P <= 2^31 - 2";
    if (s->NF > 0 && s->NV < 1) return "render: NV must be >= 1 when there are faces";
    if (s->point_size < 1 || s->point_size > SEEME_RENDER_POINT_MAX) return "render: point_size must be in 1..8";
    if (!(fabsf(s->fx) <= FLT_MAX && fabsf(s->fy) <= FLT_MAX && fabsf(s->cx) <= FLT_MAX && fabsf(s->cy) <= FLT_MAX))
        return "render: fx, fy, cx, cy must be finite";
    if (!(s->znear > 0.f && s->znear <= FLT_MAX)) return "render: znear must be finite and > 0";
    if (!s->cams || (s->NF > 0 && (!s->verts || !s->faces)) || (s->P > 0 && !s->points)) return "render: null pointer (verts, faces, points or cams)";
    if (((uintptr_t)s->verts | (uintptr_t)s->faces | (uintptr_t)s->points | (uintptr_t)s->cams) & 3)
        return "render: verts, faces, points and cams must be 4-byte aligned";
    return NULL;
}

static RdCam rd_cam(const SeemeRenderScene* s) {
    RdCam k = {s->fx, s->fy, s->cx, s->cy, s->znear};
    return k;
}

extern "C" int seeme_render(const SeemeRenderScene* s, int32_t* ids, int32_t* inv_depth, int32_t* dropped, void* ws, size_t ws_bytes,
                            void* stream) {
    if (const char* e = rd_scene_error(s)) return seeme_fail(e);
    if (!ids || !inv_depth || !dropped || !ws) return seeme_fail("render: null pointer (ids, inv_depth, dropped or ws)");
    if (((uintptr_t)ids | (uintptr_t)inv_depth | (uintptr_t)dropped) & 3) return seeme_fail("render: ids, inv_depth and dropped must be 4-byte aligned");
    if ((uintptr_t)ws & 15) return seeme_fail("render: workspace must be 16-byte aligned");
    if (ws_bytes < seeme_render_workspace_bytes(s->F, s->NV, s->H, s->W)) return seeme_fail("render: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int F = s->F, HW = s->H * s->W;
    unsigned long long* keys = (unsigned long long*)ws;
    RdVert* pv = (RdVert*)((char*)ws + rd_key_bytes(F, s->H, s->W));
    const RdCam k = rd_cam(s);
    SEEME_HIP(hipMemsetAsync(keys, 0, (size_t)F * (size_t)HW * sizeof(unsigned long long), st));
    SEEME_HIP(hipMemsetAsync(dropped, 0, (size_t)F * sizeof(int32_t), st));
    if (s->NF > 0) {
        hipLaunchKernelGGL(k_render_project, dim3((s->NV + RD_THREADS - 1) / RD_THREADS, F), dim3(RD_THREADS), 0, st, s->verts, s->cams,
                           s->FC, s->NV, k, pv);
        if (int rc = seeme_check_launch("k_render_project")) return rc;
        hipLaunchKernelGGL(k_render_faces, dim3((s->NF + RD_THREADS - 1) / RD_THREADS, F), dim3(RD_THREADS), 0, st, s->faces, s->NF, s->NV,
                           (const RdVert*)pv, s->H, s->W, keys, dropped);
        if (int rc = seeme_check_launch("k_render_faces")) return rc;
    }
    if (s->P > 0) {
        hipLaunchKernelGGL(k_render_points, dim3((s->P + RD_THREADS - 1) / RD_THREADS, F), dim3(RD_THREADS), 0, st, s->points, s->P, s->NF,
                           s->cams, s->FC, k, s->H, s->W, s->point_size, keys);
        if (int rc = seeme_check_launch("k_render_points")) return rc;
    }
    hipLaunchKernelGGL(k_render_resolve, dim3((HW + RD_THREADS - 1) / RD_THREADS, F), dim3(RD_THREADS), 0, st,
                       (const unsigned long long*)keys, HW, ids, inv_depth);
    return seeme_check_launch("k_render_resolve");
}

extern "C" int seeme_render_shade(const SeemeRenderScene* s, const int32_t* ids, const int32_t* mesh_of_face, const uint8_t* palette,
                                  int n_mesh, const uint8_t* point_rgb, uint32_t bg, uint8_t* rgb, void* stream) {
    if (const char* e = rd_scene_error(s)) return seeme_fail(e);
    if (!ids || !rgb) return seeme_fail("render_shade: null pointer (ids or rgb)");
    if (s->NF > 0 && (!mesh_of_face || !palette)) return seeme_fail("render_shade: mesh_of_face and palette are needed when there are faces");
    if (s->NF > 0 && n_mesh < 1) return seeme_fail("render_shade: n_mesh must be >= 1 when there are faces");
    if (s->P > 0 && !point_rgb) return seeme_fail("render_shade: point_rgb is needed when there are points");
    if (((uintptr_t)ids | (uintptr_t)mesh_of_face) & 3) return seeme_fail("render_shade: ids and mesh_of_face must be 4-byte aligned");
    if (bg >> 24) return seeme_fail("render_shade: bg must be r | g << 8 | b << 16");
    const int HW = s->H * s->W;
    hipLaunchKernelGGL(k_render_shade, dim3((HW + RD_THREADS - 1) / RD_THREADS, s->F), dim3(RD_THREADS), 0, (hipStream_t)stream, s->verts,
                       s->faces, s->NV, s->NF, s->P, s->cams, s->FC, ids, mesh_of_face, palette, n_mesh, point_rgb, bg, HW, rgb);
    return seeme_check_launch("k_render_shade");
}
