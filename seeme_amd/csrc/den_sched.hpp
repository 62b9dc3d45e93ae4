// den_sched.hpp -- scheduler.step (mld.py:495-497) as the sampling kernels close a denoising step with it: ONE definition for
// k_den_sample (den_kernels.hip), k_den_cluster in both of its bodies (den_cluster.inc.hip) and k_den_cluster_ms (den_cluster_ms.inc.hip).
// The kernels differ in where the coefficients and the noise row come from (table row or LDS), never in the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/seeme_hip.h"

// the eight scalars of one step (one row of SeemeSampleArgs.coef, prepared by seeme_amd/schedulers.py)
struct SchedCoef { float c0, c1, c2, c3, c4, c5, clip, ptype; };

// One element of the step.  These operations, in this order and with these roundings, DEFINE the latents of every sampling kernel: the
// suite asserts equal bits between the kernels, so the sums are spelled out with fmaf under contract(off) and nothing is left to
// what a compiler would fuse.  Elements 0 .. 2 of a lane are one chain of fused multiply-adds; element 3 (e3) is paired differently --
// fma(c2, x0, c3 ep), an unfused c5 x added, then fma(c4, n, .).  Both divisions are divisions.
__device__ __forceinline__ float sched_elem(bool e3, float x, float e, float n, const SchedCoef& k) {
#pragma clang fp contract(off)
    float x0, ep;
    if (k.ptype == 0.f) { ep = e; x0 = fmaf(-k.c1, ep, x) / k.c0; }
    else                { x0 = e; ep = fmaf(-k.c0, x0, x) / k.c1; }
    if (k.clip != 0.f) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    if (e3) return fmaf(k.c4, n, k.c5 * x + fmaf(k.c2, x0, k.c3 * ep));
    return fmaf(k.c4, n, fmaf(k.c5, x, fmaf(k.c3, ep, k.c2 * x0)));
}
// a lane's four elements: latent x, model output e, noise row n (zeros without step noise) -> the next latent
__device__ __forceinline__ float4 sched_step(float4 x, float4 e, float4 n, const SchedCoef& k) {
    const float xs[4] = {x.x, x.y, x.z, x.w}, es[4] = {e.x, e.y, e.z, e.w}, ns[4] = {n.x, n.y, n.z, n.w};
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = sched_elem(i == 3, xs[i], es[i], ns[i], k);
    return make_float4(o[0], o[1], o[2], o[3]);
}

// the step's row of the coefficient table through the constant address space: scalar loads, which do not queue behind (and whose
// waits do not drain) the vector-memory weight ring
__device__ __forceinline__ SchedCoef sched_coef_row(const float* coef, int step) {
    typedef const __attribute__((address_space(4))) float* CF32;
    const CF32 c = (CF32)(uintptr_t)coef + (size_t)step * 8;
    return SchedCoef{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]};
}
// the same eight floats from an LDS block (k_den_cluster with two wave groups, ClRowG): uniform values back into scalar registers
__device__ __forceinline__ SchedCoef sched_coef_lds(const float* blk) {
    const float4 k0 = *reinterpret_cast<const float4*>(blk), k1 = *reinterpret_cast<const float4*>(blk + 4);
    const auto sc = [](float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); };
    return SchedCoef{sc(k0.x), sc(k0.y), sc(k0.z), sc(k0.w), sc(k1.x), sc(k1.y), sc(k1.z), sc(k1.w)};
}

// a lane's four floats of sample b's row of step noise (SeemeSampleArgs.noise [steps, B, 256]; the caller checks the pointer).  It takes
// the two members, not the struct: by reference the two-wave-group kernel came out re-scheduled throughout and measurably slower
__device__ __forceinline__ const float* sched_noise_row(const float* noise, int B, int step, int b, int lane) {
    return noise + ((size_t)step * B + b) * 256 + 4 * lane;
}
