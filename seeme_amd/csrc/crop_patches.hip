// crop_patches.hip -- the S x S patch around the interactee, cut from raw uint8 RGB frames (seeme_crop_patches): all n patches of a
// call in one launch.  Definition: include/seeme_hip.h (an integer one: 1/1024-pixel coordinates cut to 1/32, 15-bit bilinear weights,
// constant zero border); the plain-torch twin is seeme_amd/crops.py crop_patches_torch and the two agree bit for bit.
//
// Plan.  Memory-bound gather work: no LDS, no matrix core.  A lane owns 4 consecutive patch pixels of one row (12 output bytes: three
// dword stores when the group is whole and its address 4-byte aligned, byte stores otherwise -- the tail of a row with S % 4 != 0 and
// the rows such an S leaves unaligned).  X (4 per lane) and Y (1 per lane) are computed in double per lane: 2 * S distinct values per
// patch are not worth a table.  Taps are byte loads; neighbouring lanes read neighbouring bytes of a frame row and L2 serves them.
// blockIdx.x walks the groups of one patch, blockIdx.y the patches, with a stride: n is not capped by the grid.
#include "api_util.hpp"
#include <stdint.h>

#define CP_THREADS 256
#define CP_MAX_BLOCKS 2048                     // workgroups of a launch: 8 per CU; more patches than grid rows are walked in a loop
#define CP_PX 4                                // patch pixels per lane

// the box of patch p is usable: finite, |cx|, |cy| <= 2^20, 0 < b <= 2^20 (NaN fails every comparison)
__device__ __forceinline__ bool cp_box_ok(float cx, float cy, float b) {
    const float lim = (float)SEEME_CROP_COORD_MAX;
    return fabsf(cx) <= lim && fabsf(cy) <= lim && b > 0.f && b <= lim;
}

// one tap: 0 outside the frame, and then never read
__device__ __forceinline__ void cp_tap(const uint8_t* __restrict__ frame, int H, int W, long long sy, long long sx, int wgt, int* acc) {
    if (wgt == 0 || sy < 0 || sy >= H || sx < 0 || sx >= W) return;
    const uint8_t* p = frame + ((size_t)sy * (size_t)W + (size_t)sx) * 3;
    acc[0] += wgt * (int)p[0];
    acc[1] += wgt * (int)p[1];
    acc[2] += wgt * (int)p[2];
}

__global__ __launch_bounds__(CP_THREADS) void k_crop_patches(const uint8_t* __restrict__ frames, int n_frames, int H, int W,
                                                             const int32_t* __restrict__ frame_of_patch,
                                                             const float* __restrict__ boxes, int n, int S, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)                 // every product and sum of the definition is rounded on its own, as in the twin
    const int G = (S + CP_PX - 1) / CP_PX;                            // groups per row
    const int item = blockIdx.x * CP_THREADS + threadIdx.x;           // < S * G <= 2^18
    if (item >= S * G) return;
    const int v = item / G, u0 = (item - v * G) * CP_PX;
    const int nu = min(CP_PX, S - u0);
    const size_t frame_bytes = (size_t)H * (size_t)W * 3;
    for (int p = blockIdx.y; p < n; p += gridDim.y) {
        const float cx = boxes[(size_t)p * 3], cy = boxes[(size_t)p * 3 + 1], b = boxes[(size_t)p * 3 + 2];
        const int f = frame_of_patch[p];
        const bool ok = cp_box_ok(cx, cy, b) && f >= 0 && f < n_frames;
        uint8_t px[CP_PX * 3];
#pragma unroll
        for (int i = 0; i < CP_PX * 3; ++i) px[i] = 0;
        if (ok) {
            const uint8_t* frame = frames + (size_t)f * frame_bytes;
            const double m = (double)b / (double)S;
            const double hs = 0.5 * (double)S * m;
            const double ox = (double)cx - hs, oy = (double)cy - hs;
            const long long X0 = (long long)rint(ox * 1024.0) + 16;
            const long long Y = ((long long)rint((m * (double)v + oy) * 1024.0) + 16) >> 5;
            const long long sy = Y >> 5;
            const int ay = (int)(Y & 31);
#pragma unroll
            for (int i = 0; i < CP_PX; ++i) {
                if (i < nu) {
                    const long long X = (X0 + (long long)rint(m * (double)(u0 + i) * 1024.0)) >> 5;
                    const long long sx = X >> 5;
                    const int ax = (int)(X & 31);
                    int acc[3] = {512, 512, 512};
                    cp_tap(frame, H, W, sy, sx, (32 - ay) * (32 - ax), acc);
                    cp_tap(frame, H, W, sy, sx + 1, (32 - ay) * ax, acc);
                    cp_tap(frame, H, W, sy + 1, sx, ay * (32 - ax), acc);
                    cp_tap(frame, H, W, sy + 1, sx + 1, ay * ax, acc);
                    px[3 * i] = (uint8_t)(acc[0] >> 10);
                    px[3 * i + 1] = (uint8_t)(acc[1] >> 10);
                    px[3 * i + 2] = (uint8_t)(acc[2] >> 10);
                }
            }
        }
        uint8_t* o = out + (((size_t)p * (size_t)S + (size_t)v) * (size_t)S + (size_t)u0) * 3;
        if (nu == CP_PX && ((uintptr_t)o & 3) == 0) {
            uint32_t* o4 = (uint32_t*)o;
#pragma unroll
            for (int d = 0; d < 3; ++d)
                o4[d] = (uint32_t)px[4 * d] | ((uint32_t)px[4 * d + 1] << 8) | ((uint32_t)px[4 * d + 2] << 16) | ((uint32_t)px[4 * d + 3] << 24);
        } else {
            for (int i = 0; i < nu * 3; ++i) o[i] = px[i];
        }
    }
}

extern "C" int seeme_crop_patches(const uint8_t* frames, int n_frames, int H, int W, const int32_t* frame_of_patch, const float* boxes,
                                  int n, int S, uint8_t* out, void* stream) {
    if (n_frames < 1) return seeme_fail("crop_patches: n_frames must be >= 1");
    if (H < 1 || H > SEEME_CROP_FRAME_MAX || W < 1 || W > SEEME_CROP_FRAME_MAX) return seeme_fail("crop_patches: H and W must be in 1..16384");
    if (S < 1 || S > SEEME_CROP_PATCH_MAX) return seeme_fail("crop_patches: S must be in 1..1024");
    if (n < 1) return seeme_fail("crop_patches: n must be >= 1");
    if (!frames || !frame_of_patch || !boxes || !out) return seeme_fail("crop_patches: null pointer");
    if (((uintptr_t)frame_of_patch | (uintptr_t)boxes) & 3) return seeme_fail("crop_patches: frame_of_patch and boxes must be 4-byte aligned");
    const int G = (S + CP_PX - 1) / CP_PX;
    const int gx = (S * G + CP_THREADS - 1) / CP_THREADS;             // <= 1024
    const int rows = CP_MAX_BLOCKS / gx;                              // >= 2
    const int gy = n < rows ? n : rows;
    hipLaunchKernelGGL(k_crop_patches, dim3(gx, gy), dim3(CP_THREADS), 0, (hipStream_t)stream, frames, n_frames, H, W, frame_of_patch,
                       boxes, n, S, out);
    return seeme_check_launch("k_crop_patches");
}
