// flow_head.hip -- the ProHMR-scene pose head (SMPLFlow): the inverse of a four-layer conditional Glow over the 144 rot6d values,
// the betas / camera MLP, Gram-Schmidt and the log-probability.  The definition is in include/seeme_hip.h (SeemeFlowHead); the
// host-side folds are seeme_amd/prohmr_head.py fold().  Everything is fp32 on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain).
//
// Three launches per call:
//   k_flow_ctx    C[L,5120] = ctx[L,2566] x ctx_w^T + ctx_b: the context columns of the four initial layers and fc_head.layers.0
//                 in ONE GEMM (the context is read once per frame); ReLU on the fc_head part.
//   k_flow_chain  one workgroup per FH_T rows of (frame, sample): the whole inverse, layers 3 -> 0.  Per layer
//                     gather identity (72) -> initial layer (K 80) + C[frame] -> 2 x [BN ReLU Linear BN ReLU Linear +] ->
//                     final layer (1024 -> 72) -> subtract from the transform features -> inv(LU) (144 x 144) -> ActNorm^-1
//                 the residual stream h lives in registers (each wave owns 256 of the 1024 columns), the MFMA A operand in two
//                 LDS tiles that alternate, the 144-wide state in LDS.  No [R,1024] intermediate goes to global memory.
//   k_flow_fc     per frame: fc_head.layers.2 (1024 -> 13) on C[:, 4096:], + init_betas / init_cam.
//
// LDS map of k_flow_chain (FH_T = 16 rows), floats:  A0 [16][1032] | A1 [16][1032] | X [16][152] | I [16][88]  = 147 456 bytes.
// A row's arithmetic never looks at another row (an MFMA row is its own fmaf chain over k in a fixed order), so a row computed
// alone and the same row inside a full tile are bitwise equal; rows past R are computed on a copy of row R-1 and not stored.
#include "common.hpp"
#include "api_util.hpp"

#define FH_T 16
#define FH_LDA 1032
#define FH_LDX 152
#define FH_LDI 88
#define FH_H SEEME_FLOW_HIDDEN
#define FH_D SEEME_FLOW_DIM
#define FH_CTXP SEEME_FLOW_CTX_PAD
#define FH_CW SEEME_FLOW_CTX_COLS
#define FH_CHAIN_LDS ((2 * FH_T * FH_LDA + FH_T * FH_LDX + FH_T * FH_LDI) * 4)

// ------------------------------------------------------------------------------------------------ context pass
#define FC_ROWS 32
#define FC_KC 256
#define FC_LDA (FC_KC + LDS_PAD)
__global__ __launch_bounds__(256) void k_flow_ctx(SeemeFlowHead w, const float* __restrict__ ctx, int L, float* __restrict__ Cw) {
    __shared__ __attribute__((aligned(16))) float As[FC_ROWS * FC_LDA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    const int g0 = blockIdx.y * FC_ROWS;
    const int n0 = blockIdx.x * CH_N + wave * 64;
    f32x4 acc[2][4];
    acc_zero(acc);
    for (int kc = 0; kc < FH_CTXP; kc += FC_KC) {
        const int kw = FH_CTXP - kc < FC_KC ? FH_CTXP - kc : FC_KC;      // 256, and 16 for the tail (2566 = 10 x 256 + 6, padded to 16)
        __syncthreads();
        for (int i = tid; i < FC_ROWS * kw; i += 256) {
            const int row = i / kw, c = i - row * kw;
            const int g = g0 + row, k = kc + c;
            As[row * FC_LDA + c] = (g < L && k < SEEME_FLOW_CTX) ? ctx[(size_t)g * SEEME_FLOW_CTX + k] : 0.f;
        }
        __syncthreads();
        tile_gemm_f32<2, 4>(As, FC_LDA, w.ctx_w + kc, FH_CTXP, n0, FH_CW, kw / 16, acc);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int col = n0 + nt * 16 + r;
            const float b = w.ctx_b[col];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int g = g0 + mt * 16 + 4 * kq + e;
                float v = acc[mt][nt][e] + b;
                if (col >= 4 * FH_H) v = fmaxf(v, 0.f);
                if (g < L) Cw[(size_t)g * FH_CW + col] = v;
            }
        }
}

// ------------------------------------------------------------------------------------------------ the chain
// One 1024-column GEMM pass of this wave: its 256 columns as 4 passes of 4 n-tiles; f(t, acc) receives n-tile t = 0..15.
template <class F>
__device__ __forceinline__ void fh_gemm1024(const float* As, int lda, const float* W, int ldw, int K16, int wave, F&& f) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f32x4 acc[1][4];
        acc_zero(acc);
        tile_gemm_f32<1, 4>(As, lda, W, ldw, wave * 256 + p * 64, FH_H, K16, acc);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) f(p * 4 + nt, acc[0][nt]);
    }
}

__global__ __launch_bounds__(256) void k_flow_chain(SeemeFlowHead w, const float* __restrict__ Cw, const float* __restrict__ z, int R,
                                                    int S, float* __restrict__ pose6d, float* __restrict__ rotmat,
                                                    float* __restrict__ log_prob) {
    extern __shared__ __attribute__((aligned(16))) float fh_lds[];
    float* A0 = fh_lds;
    float* A1 = A0 + FH_T * FH_LDA;
    float* Xs = A1 + FH_T * FH_LDA;
    float* Is = Xs + FH_T * FH_LDX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    const int g0 = blockIdx.x * FH_T;

    for (int i = tid; i < FH_T * FH_LDX; i += 256) {
        const int row = i / FH_LDX, c = i - row * FH_LDX;
        const int g = g0 + row < R ? g0 + row : R - 1;
        Xs[i] = c < FH_D ? z[(size_t)g * FH_D + c] : 0.f;
    }
    for (int i = tid; i < FH_T * FH_LDI; i += 256) Is[i] = 0.f;         // columns 72..79 stay zero: K of the initial layer is padded
    __syncthreads();
    if (tid < FH_T && g0 + tid < R) {                                    // log N(z; 0, I) + the constant log|det|: one fixed-order row sum
        float ss = 0.f;
        for (int c = 0; c < FH_D; ++c) ss = fmaf(Xs[tid * FH_LDX + c], Xs[tid * FH_LDX + c], ss);
        log_prob[g0 + tid] = fmaf(-0.5f, ss, w.log_const);
    }
    size_t crow[4];                                                      // this lane's 4 rows -> their frames' rows of C
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int g = g0 + 4 * kq + e < R ? g0 + 4 * kq + e : R - 1;
        crow[e] = (size_t)(g / S) * FH_CW;
    }

    for (int l = SEEME_FLOW_LAYERS - 1; l >= 0; --l) {
        const int par = (w.id_parity >> l) & 1;
        __syncthreads();
        for (int i = tid; i < FH_T * 72; i += 256) {
            const int row = i / 72, j = i - row * 72;
            Is[row * FH_LDI + j] = Xs[row * FH_LDX + 2 * j + par];
        }
        __syncthreads();
        // initial layer: W[:, :72] identity + (W[:, 72:] ctx + b), the second term from the context pass
        f32x4 h[16];
        fh_gemm1024(Is, FH_LDI, w.id_w + (size_t)l * FH_H * 80, 80, 5, wave, [&](int t, const f32x4& a) { h[t] = a; });
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int col = l * FH_H + wave * 256 + t * 16 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[t][e] += Cw[crow[e] + col];
        }
        for (int b = 0; b < 2; ++b) {
            const int m0 = l * 4 + 2 * b;
            const float* s0 = w.bn_s + (size_t)m0 * FH_H;
            const float* o0 = w.bn_o + (size_t)m0 * FH_H;
            const float* s1 = s0 + FH_H;
            const float* o1 = o0 + FH_H;
            const float* rb = w.res_b + (size_t)(l * 2 + b) * FH_H;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int col = wave * 256 + t * 16 + r;
                const float sv = s0[col], ov = o0[col];
#pragma unroll
                for (int e = 0; e < 4; ++e) A0[(4 * kq + e) * FH_LDA + col] = fmaxf(fmaf(h[t][e], sv, ov), 0.f);
            }
            __syncthreads();
            fh_gemm1024(A0, FH_LDA, w.lin_w + (size_t)m0 * FH_H * FH_H, FH_H, FH_H / 16, wave, [&](int t, const f32x4& a) {
                const int col = wave * 256 + t * 16 + r;
                const float sv = s1[col], ov = o1[col];                  // the first Linear's bias is folded into ov
#pragma unroll
                for (int e = 0; e < 4; ++e) A1[(4 * kq + e) * FH_LDA + col] = fmaxf(fmaf(a[e], sv, ov), 0.f);
            });
            __syncthreads();
            fh_gemm1024(A1, FH_LDA, w.lin_w + (size_t)(m0 + 1) * FH_H * FH_H, FH_H, FH_H / 16, wave, [&](int t, const f32x4& a) {
                const float bv = rb[wave * 256 + t * 16 + r];
#pragma unroll
                for (int e = 0; e < 4; ++e) h[t][e] += a[e] + bv;
            });
        }
        // final layer: the shift of the 72 transform features; the coupling is additive, its inverse subtracts
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int col = wave * 256 + t * 16 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) A0[(4 * kq + e) * FH_LDA + col] = h[t][e];
        }
        __syncthreads();
        if (wave < 3) {
            f32x4 acc[1][2];
            acc_zero(acc);
            tile_gemm_f32<1, 2>(A0, FH_LDA, w.fin_w + (size_t)l * 72 * FH_H, FH_H, wave * 32, 72, FH_H / 16, acc);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int j = wave * 32 + nt * 16 + r;
                if (j < 72) {
                    const float bv = w.fin_b[l * 72 + j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) Xs[(4 * kq + e) * FH_LDX + 2 * j + 1 - par] -= acc[0][nt][e] + bv;
                }
            }
        }
        __syncthreads();
        // inv(L U) as one dense matrix, then the ActNorm inverse (and the LU bias) as scale / offset
        f32x4 lu[1][3];
        acc_zero(lu);
        if (wave < 3) tile_gemm_f32<1, 3>(Xs, FH_LDX, w.lu_w + (size_t)l * FH_D * FH_D, FH_D, wave * 48, FH_D, FH_D / 16, lu);
        __syncthreads();
        if (wave < 3) {
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) {
                const int c = wave * 48 + nt * 16 + r;
                const float sv = w.act_s[l * FH_D + c], ov = w.act_o[l * FH_D + c];
#pragma unroll
                for (int e = 0; e < 4; ++e) Xs[(4 * kq + e) * FH_LDX + c] = fmaf(lu[0][nt][e], sv, ov);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < FH_T * FH_D; i += 256) {
        const int row = i / FH_D, c = i - row * FH_D;
        if (g0 + row < R) pose6d[(size_t)(g0 + row) * FH_D + c] = Xs[row * FH_LDX + c];
    }
    // Gram-Schmidt in the 'prohmr' order: a1 = x[0:3], a2 = x[3:6] are the first two COLUMNS; R = [b1 b2 b1 x b2]
    for (int i = tid; i < FH_T * 24; i += 256) {
        const int row = i / 24, j = i - row * 24;
        if (g0 + row >= R) continue;
        const float* x = Xs + row * FH_LDX + 6 * j;
        const float a1x = x[0], a1y = x[1], a1z = x[2], a2x = x[3], a2y = x[4], a2z = x[5];
        const float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);
        const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
        const float d = b1x * a2x + b1y * a2y + b1z * a2z;
        const float cx = a2x - d * b1x, cy = a2y - d * b1y, cz = a2z - d * b1z;
        const float n2 = fmaxf(sqrtf(cx * cx + cy * cy + cz * cz), 1e-12f);
        const float b2x = cx / n2, b2y = cy / n2, b2z = cz / n2;
        float* o = rotmat + ((size_t)(g0 + row) * 24 + j) * 9;
        o[0] = b1x; o[1] = b2x; o[2] = b1y * b2z - b1z * b2y;
        o[3] = b1y; o[4] = b2y; o[5] = b1z * b2x - b1x * b2z;
        o[6] = b1z; o[7] = b2z; o[8] = b1x * b2y - b1y * b2x;
    }
}

// ------------------------------------------------------------------------------------------------ betas and camera
__global__ __launch_bounds__(64) void k_flow_fc(SeemeFlowHead w, const float* __restrict__ Cw, int L, float* __restrict__ betas,
                                                float* __restrict__ cam) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const float* hid = Cw + (size_t)f * FH_CW + 4 * FH_H;
    for (int o = 0; o < 13; ++o) {
        float s = 0.f;
        for (int k = lane; k < FH_H; k += 64) s = fmaf(hid[k], w.fc_w[o * FH_H + k], s);
        s = wave_sum(s);
        if (lane == 0) {
            const float v = s + w.fc_b[o];
            if (o < 10) betas[(size_t)f * 10 + o] = v;
            else cam[(size_t)f * 3 + (o - 10)] = v;
        }
    }
}

static bool fh_sizes_ok(int L, int S) {
    return L >= 1 && S >= 1 && S <= SEEME_FLOW_S_MAX && (long long)L * S <= SEEME_FLOW_ROWS_MAX;
}

extern "C" size_t seeme_flow_head_workspace_bytes(int L, int S) {
    if (!fh_sizes_ok(L, S)) return 0;
    return (size_t)L * FH_CW * sizeof(float);
}

extern "C" int seeme_flow_head(const SeemeFlowHead* w, const float* ctx, const float* z, int L, int S, float* pose6d, float* rotmat,
                               float* betas, float* cam, float* log_prob, void* ws, size_t ws_bytes, void* stream) {
    if (!fh_sizes_ok(L, S)) return seeme_fail("flow_head: L >= 1, 1 <= S <= 32 and L * S <= 2^20");
    if (!w || !ctx || !z || !pose6d || !rotmat || !betas || !cam || !log_prob || !ws) return seeme_fail("flow_head: null pointer");
    const void* wp[] = {w->ctx_w, w->ctx_b, w->id_w, w->lin_w, w->bn_s, w->bn_o, w->res_b, w->fin_w, w->fin_b, w->lu_w, w->act_s,
                        w->act_o, w->fc_w, w->fc_b};
    for (const void* p : wp) {
        if (!p) return seeme_fail("flow_head: null weight pointer");
        if ((uintptr_t)p & 15) return seeme_fail("flow_head: weight pointers must be 16-byte aligned");
    }
    if (((uintptr_t)ctx | (uintptr_t)z) & 3) return seeme_fail("flow_head: ctx and z must be 4-byte aligned");
    if ((uintptr_t)ws & 15) return seeme_fail("flow_head: workspace must be 16-byte aligned");
    if (ws_bytes < seeme_flow_head_workspace_bytes(L, S)) return seeme_fail("flow_head: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* Cw = (float*)ws;
    const int R = L * S;
    hipLaunchKernelGGL(k_flow_ctx, dim3(FH_CW / CH_N, (L + FC_ROWS - 1) / FC_ROWS), dim3(256), 0, st, *w, ctx, L, Cw);
    if (int rc = seeme_check_launch("k_flow_ctx")) return rc;
    SEEME_HIP(hipFuncSetAttribute((const void*)k_flow_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FH_CHAIN_LDS));
    hipLaunchKernelGGL(k_flow_chain, dim3((R + FH_T - 1) / FH_T), dim3(256), FH_CHAIN_LDS, st, *w, Cw, z, R, S, pose6d, rotmat, log_prob);
    if (int rc = seeme_check_launch("k_flow_chain")) return rc;
    hipLaunchKernelGGL(k_flow_fc, dim3(L), dim3(64), 0, st, *w, Cw, L, betas, cam);
    return seeme_check_launch("k_flow_fc");
}
