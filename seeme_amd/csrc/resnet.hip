// resnet.hip -- frozen, eval-mode ResNet-50 backbone (EgoHMR/models/resnet.py: ResNet(Bottleneck, [3,4,6,3]) without fc),
// the image encoder behind proscene.encode_image (prohmr_scene.py:99-100).  BatchNorm is folded into weight + bias on the host.
//
// Activations are NHWC.  Every convolution is ONE implicit GEMM  Y[m][n] = sum_k X[row(m, tap(k))][cin(k)] * W[n][k]  with
// m = (image, ho, wo), n = cout, k = (kh, kw, cin): k_conv gathers the shifted input rows straight into LDS (zero outside the
// image), no im2col buffer.  One kernel body serves both precisions -- a K-step is 128 bytes of k per row, i.e. 64 bf16 or 32 fp32:
//   bf16: v_mfma_f32_16x16x32_bf16, one per 16-byte chunk quad;   fp32: 4 x v_mfma_f32_16x16x4_f32 on the same chunks.
// The weights are the MFMA's A operand (rows = cout) and the pixels its B operand, so a lane ends up with 4 consecutive output
// channels of one pixel per fragment; the host interleaves the rows of each 64-channel group (row(t, q) below) so that the 4
// fragments of a lane are 16 CONSECUTIVE channels: the epilogue (+bias, +residual, ReLU) loads and stores 32 / 64 contiguous bytes.
// The stem (K = 147) reads an image repacked to 16 bytes per pixel (k_stem_pack: layout change + uint8 normalisation), so a
// 16-byte chunk is one tap and K = 49 chunks padded to 56.  No atomics anywhere: two launches are bitwise equal.
#include "api_util.hpp"
#include <stdint.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned f2bf(float f) {      // round to nearest even (finite inputs)
    unsigned u = __float_as_uint(f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf2f(unsigned h) { return __uint_as_float(h << 16); }

struct ConvArgs {
    const unsigned char* x;      // [B, H, W, cin] activations, 16 << ccl2 bytes per pixel
    const unsigned char* w;      // packed fragments [cout/16][kgroups][64 lanes][16 B]
    const float* bias;           // [cout]
    const unsigned char* res;    // [M, cout] or null
    unsigned char* y;            // [M, cout]
    int H, W, Ho, Wo, ccl2, cout, stride, M, ksteps, relu;
};

// 128 pixels x BN channels per workgroup of 4 waves; BN = 128: 2 x 2 waves of 64 x 64, BN = 64: 4 x 1 waves of 32 x 64.
template <bool BF16, int KS, int BN>
__global__ __launch_bounds__(256) void k_conv(ConvArgs a) {
    constexpr int WN = BN / 64, WM = 4 / WN, MI = 8 / WM, NBL = BN / 32;
    __shared__ __attribute__((aligned(16))) unsigned char lds[16384 + BN * 128];
    unsigned char* As = lds;                  // [128 rows][8 chunks of 16 B], chunk c of row r at c ^ ((r >> 1) & 7)
    unsigned char* Bs = lds + 16384;          // [BN/16 tiles][2 k-groups][64 lanes][16 B], as packed
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.y * 128, n0 = blockIdx.x * BN;
    const int c = t & 7;
    int pix[4], hi0[4], wi0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + (t >> 3) + 32 * i;
        const int wo = m % a.Wo, q = m / a.Wo, ho = q % a.Ho, b = q / a.Ho;
        pix[i] = b * a.H * a.W;
        hi0[i] = m < a.M ? ho * a.stride - KS / 2 : -(1 << 20);      // rows past M read as outside the image
        wi0[i] = wo * a.stride - KS / 2;
    }
    const int kgroups = a.ksteps * 2;
    const unsigned char* wb = a.w + (size_t)(n0 >> 4) * kgroups * 1024;
    u32x4 ra[4], rb[NBL];
    auto fetch = [&](int ks) {
        const int q = ks * 8 + c, tap = q >> a.ccl2, coff = (q & ((1 << a.ccl2) - 1)) << 4;
        const int kh = tap / KS, kw = tap - kh * KS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int hi = hi0[i] + kh, wi = wi0[i] + kw;
            const bool ok = tap < KS * KS && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *(const u32x4*)(a.x + ((size_t)(pix[i] + hi * a.W + wi) << (a.ccl2 + 4)) + coff);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < NBL; ++i) {
            const int j = t + 256 * i;
            rb[i] = *(const u32x4*)(wb + ((size_t)(j >> 7) * kgroups + ks * 2) * 1024 + (j & 127) * 16);
        }
    };
    f32x4 acc[MI][4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    for (int ks = 0; ks < a.ksteps; ++ks) {
        __syncthreads();                       // the previous step's fragment reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (t >> 3) + 32 * i;
            *(u32x4*)(As + r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < NBL; ++i) *(u32x4*)(Bs + (t + 256 * i) * 16) = rb[i];
        __syncthreads();
        if (ks + 1 < a.ksteps) fetch(ks + 1);  // in flight behind this step's MFMAs
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            u32x4 xf[MI], wf[4];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int r = (wm * MI + mi) * 16 + (lane & 15), ch = g * 4 + (lane >> 4);
                xf[mi] = *(const u32x4*)(As + r * 128 + ((ch ^ ((r >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) wf[ni] = *(const u32x4*)(Bs + ((wn * 4 + ni) * 2 + g) * 1024 + lane * 16);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    if constexpr (BF16) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[ni]),
                                                                              __builtin_bit_cast(bf16x8, xf[mi]), acc[mi][ni], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(wf[ni][e]), __uint_as_float(xf[mi][e]),
                                                                               acc[mi][ni], 0, 0, 0);
                    }
                }
        }
    }
    // epilogue: lane = pixel (lane & 15) x 16 consecutive channels (fragment ni holds channels 4 ni .. 4 ni + 3 of them)
    const int n = n0 + wn * 64 + (lane >> 4) * 16;
    float bz[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 b4 = *(const float4*)(a.bias + n + 4 * i);
        bz[4 * i] = b4.x, bz[4 * i + 1] = b4.y, bz[4 * i + 2] = b4.z, bz[4 * i + 3] = b4.w;
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int m = m0 + (wm * MI + mi) * 16 + (lane & 15);
        if (m >= a.M) continue;
        float v[16];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * ni + j] = acc[mi][ni][j] + bz[4 * ni + j];
        const size_t off = (size_t)m * a.cout + n;
        if constexpr (BF16) {
            if (a.res) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const u32x4 r4 = *(const u32x4*)(a.res + off * 2 + 16 * h);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[8 * h + 2 * i] += bf2f(r4[i] & 0xffffu), v[8 * h + 2 * i + 1] += bf2f(r4[i] >> 16);
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                u32x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float lo = v[8 * h + 2 * i], hi = v[8 * h + 2 * i + 1];
                    if (a.relu) lo = fmaxf(lo, 0.f), hi = fmaxf(hi, 0.f);
                    o[i] = f2bf(lo) | (f2bf(hi) << 16);
                }
                *(u32x4*)(a.y + off * 2 + 16 * h) = o;
            }
        } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                float4 o = {v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
                if (a.res) {
                    const float4 r4 = *(const float4*)(a.res + off * 4 + 16 * h);
                    o.x += r4.x, o.y += r4.y, o.z += r4.z, o.w += r4.w;
                }
                if (a.relu) o.x = fmaxf(o.x, 0.f), o.y = fmaxf(o.y, 0.f), o.z = fmaxf(o.z, 0.f), o.w = fmaxf(o.w, 0.f);
                *(float4*)(a.y + off * 4 + 16 * h) = o;
            }
        }
    }
}

// The stem's loader: images -> [B, H, W] pixels of 16 bytes (r, g, b, 0 ...): 8 bf16 or 4 fp32.  fmt 0: float NCHW, already
// normalised; fmt 1: uint8 NHWC RGB, normalised here as (x - 255 mean_c) / (255 std_c) (dataset.py:1693-1705).
template <bool BF16>
__global__ __launch_bounds__(256) void k_stem_pack(const void* __restrict__ img, int fmt, long npix, int HW, unsigned char* __restrict__ y) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    float v[3];
    if (fmt == 0) {
        const long b = p / HW, s = p - b * HW;
        const float* f = (const float*)img + b * 3 * HW + s;
        v[0] = f[0], v[1] = f[HW], v[2] = f[2 * (long)HW];
    } else {
        const unsigned char* u = (const unsigned char*)img + p * 3;
        // the reference forms 255 * mean_c in float64 (numpy): round that product, not a float product
        const float mean[3] = {(float)(255.0 * 0.485), (float)(255.0 * 0.456), (float)(255.0 * 0.406)};
        const float sd[3] = {(float)(255.0 * 0.229), (float)(255.0 * 0.224), (float)(255.0 * 0.225)};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = ((float)u[ch] - mean[ch]) / sd[ch];
    }
    u32x4 o;
    if constexpr (BF16) o = u32x4{f2bf(v[0]) | (f2bf(v[1]) << 16), f2bf(v[2]), 0u, 0u};
    else o = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), 0u};
    *(u32x4*)(y + p * 16) = o;
}

// MaxPool2d(3, stride 2, pad 1) over NHWC, 16 bytes of channels per thread.
template <bool BF16>
__global__ __launch_bounds__(256) void k_maxpool(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int B, int H, int W,
                                                 int Ho, int Wo, int cchunks) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long)B * Ho * Wo * cchunks) return;
    const int cc = id % cchunks;
    long q = id / cchunks;
    const int wo = q % Wo; q /= Wo;
    const int ho = q % Ho, b = q / Ho;
    constexpr int E = BF16 ? 8 : 4;
    float mx[E];
#pragma unroll
    for (int e = 0; e < E; ++e) mx[e] = -INFINITY;
    for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) {
            const int hi = 2 * ho - 1 + kh, wi = 2 * wo - 1 + kw;
            if ((unsigned)hi >= (unsigned)H || (unsigned)wi >= (unsigned)W) continue;
            const u32x4 v = *(const u32x4*)(x + (((size_t)(b * H + hi) * W + wi) * cchunks + cc) * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (BF16) mx[2 * i] = fmaxf(mx[2 * i], bf2f(v[i] & 0xffffu)), mx[2 * i + 1] = fmaxf(mx[2 * i + 1], bf2f(v[i] >> 16));
                else mx[i] = fmaxf(mx[i], __uint_as_float(v[i]));
            }
        }
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (BF16) o[i] = f2bf(mx[2 * i]) | (f2bf(mx[2 * i + 1]) << 16);
        else o[i] = __float_as_uint(mx[i]);
    }
    *(u32x4*)(y + id * 16) = o;
}

// mean over the HW positions of [B, HW, C] -> fp32 [B, C]; one thread per (image, channel), positions summed in order.
template <bool BF16>
__global__ __launch_bounds__(256) void k_avgpool(const unsigned char* __restrict__ x, float* __restrict__ out, int B, int HW, int C) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= B * C) return;
    const int b = id / C, ch = id - b * C;
    float s = 0.f;
    for (int p = 0; p < HW; ++p) {
        const size_t e = ((size_t)b * HW + p) * C + ch;
        s += BF16 ? bf2f(((const unsigned short*)x)[e]) : ((const float*)x)[e];
    }
    out[id] = s / (float)HW;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline size_t esize(int precision) { return precision == SEEME_RESNET_BF16 ? 2 : 4; }

// cin as the kernel sees it: the stem reads 16-byte pixels (3 channels zero padded to 8 bf16 / 4 fp32)
inline int cin_padded(const SeemeConv& c, int precision) { return c.cin == 3 ? (int)(16 / esize(precision)) : c.cin; }

const char* conv_shape_error(const SeemeConv& c, int precision) {
    if (c.k != 1 && c.k != 3 && c.k != 7) return "convolution kernel size must be 1, 3 or 7";
    if (c.stride != 1 && c.stride != 2) return "convolution stride must be 1 or 2";
    if (c.cout <= 0 || c.cout % 64) return "convolution cout must be a positive multiple of 64";
    const int cb = cin_padded(c, precision) * (int)esize(precision);
    if (c.cin <= 0 || cb % 16 || (1 << ilog2(cb / 16)) != cb / 16) return "convolution cin must be 3 or a power of two of at least 16 bytes";
    return nullptr;
}

template <bool BF16, int KS>
int launch_conv_bn(const ConvArgs& a, long mtiles, hipStream_t st) {
    // 64-channel tiles where 128 would leave the chip short of workgroups
    if (a.cout % 128 == 0 && mtiles * (a.cout / 128) >= 512) {
        hipLaunchKernelGGL((k_conv<BF16, KS, 128>), dim3(a.cout / 128, (unsigned)mtiles), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_conv<BF16, KS, 64>), dim3(a.cout / 64, (unsigned)mtiles), dim3(256), 0, st, a);
    }
    return seeme_check_launch("k_conv");
}

// x [B,H,W,cin] -> y [B,Ho,Wo,cout] (pad k/2); all pointers checked by the callers
int run_conv(const SeemeConv& c, int precision, const void* x, int B, int H, int W, const void* res, int relu, void* y, hipStream_t st) {
    const bool bf = precision == SEEME_RESNET_BF16;
    ConvArgs a;
    a.x = (const unsigned char*)x, a.w = (const unsigned char*)(bf ? (const void*)c.weight_bf16 : (const void*)c.weight);
    a.bias = c.bias, a.res = (const unsigned char*)res, a.y = (unsigned char*)y;
    a.H = H, a.W = W, a.Ho = (H + 2 * (c.k / 2) - c.k) / c.stride + 1, a.Wo = (W + 2 * (c.k / 2) - c.k) / c.stride + 1;
    const int cb = cin_padded(c, precision) * (int)esize(precision);
    a.ccl2 = ilog2(cb / 16), a.cout = c.cout, a.stride = c.stride, a.relu = relu;
    const long M = (long)B * a.Ho * a.Wo;
    a.M = (int)M;
    a.ksteps = (c.k * c.k * (cb / 16) + 7) / 8;
    const long mtiles = (M + 127) / 128;
    if (mtiles > 65535) return seeme_fail("convolution: too many output pixels for one launch");
    if (bf) return c.k == 1 ? launch_conv_bn<true, 1>(a, mtiles, st) : c.k == 3 ? launch_conv_bn<true, 3>(a, mtiles, st) : launch_conv_bn<true, 7>(a, mtiles, st);
    return c.k == 1 ? launch_conv_bn<false, 1>(a, mtiles, st) : c.k == 3 ? launch_conv_bn<false, 3>(a, mtiles, st) : launch_conv_bn<false, 7>(a, mtiles, st);
}

int run_maxpool(int precision, const void* x, int B, int H, int W, int C, void* y, hipStream_t st) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, cch = C * (int)esize(precision) / 16;
    const long n = (long)B * Ho * Wo * cch;
    if (precision == SEEME_RESNET_BF16)
        hipLaunchKernelGGL(k_maxpool<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const unsigned char*)x, (unsigned char*)y, B, H, W, Ho, Wo, cch);
    else
        hipLaunchKernelGGL(k_maxpool<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const unsigned char*)x, (unsigned char*)y, B, H, W, Ho, Wo, cch);
    return seeme_check_launch("k_maxpool");
}

int run_stem_pack(const void* images, int fmt, int B, int H, int W, int precision, void* y, hipStream_t st) {
    const long npix = (long)B * H * W;
    if (precision == SEEME_RESNET_BF16)
        hipLaunchKernelGGL(k_stem_pack<true>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, images, fmt, npix, H * W, (unsigned char*)y);
    else
        hipLaunchKernelGGL(k_stem_pack<false>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, images, fmt, npix, H * W, (unsigned char*)y);
    return seeme_check_launch("k_stem_pack");
}

// ---- the network: conv table order = stem, then per bottleneck conv1, conv2, conv3 and, in a layer's first one, downsample
constexpr int kBlocks[4] = {3, 4, 6, 3};
constexpr size_t kS = 112 * 112 * 64;        // elements of the largest activation per image (= 56 * 56 * 256)
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
struct WsLayout { size_t stem, x, y, ds, t1, t2, total; };
WsLayout ws_layout(int B, int precision) {
    const size_t e = esize(precision);
    WsLayout l;
    size_t o = 0;
    l.stem = o, o += up256((size_t)B * 224 * 224 * 16);
    l.x = o, o += up256(B * kS * e);
    l.y = o, o += up256(B * kS * e);
    l.ds = o, o += up256(B * kS * e);
    l.t1 = o, o += up256(B * kS / 2 * e);
    l.t2 = o, o += up256(B * kS / 4 * e);
    l.total = o;
    return l;
}

const char* table_error(const SeemeResnet50* w) {
    int i = 0, inpl = 64;
    auto same = [&](const SeemeConv& c, int cin, int cout, int k, int s) { return c.cin == cin && c.cout == cout && c.k == k && c.stride == s; };
    if (!same(w->conv[i++], 3, 64, 7, 2)) return "conv table: entry 0 is not the 7x7 stride-2 stem";
    for (int L = 0; L < 4; ++L)
        for (int b = 0; b < kBlocks[L]; ++b) {
            const int pl = 64 << L, s = (b == 0 && L > 0) ? 2 : 1;
            if (!same(w->conv[i], inpl, pl, 1, 1) || !same(w->conv[i + 1], pl, pl, 3, s) || !same(w->conv[i + 2], pl, 4 * pl, 1, 1))
                return "conv table: a bottleneck entry has the wrong {cin, cout, k, stride}";
            i += 3;
            if (b == 0) {
                if (!same(w->conv[i], inpl, 4 * pl, 1, s)) return "conv table: a downsample entry has the wrong {cin, cout, k, stride}";
                ++i;
            }
            inpl = 4 * pl;
        }
    for (i = 0; i < SEEME_RESNET50_NCONV; ++i) {
        const SeemeConv& c = w->conv[i];
        const void* wt = w->precision == SEEME_RESNET_BF16 ? (const void*)c.weight_bf16 : (const void*)c.weight;
        if (!wt || !c.bias) return "conv table: null weight or bias (is the table packed for this precision?)";
        if (!aligned16(wt) || !aligned16(c.bias)) return "conv table: weight and bias must be 16-byte aligned";
    }
    return nullptr;
}

}  // namespace

extern "C" size_t seeme_resnet50_workspace_bytes(int B, int precision) {
    if (B <= 0 || B > 1024 || (precision != SEEME_RESNET_FP32 && precision != SEEME_RESNET_BF16)) return 0;
    return ws_layout(B, precision).total;
}

extern "C" int seeme_resnet50_encode(const SeemeResnet50* w, const void* images, int image_format, int B, float* out, void* ws,
                                     size_t ws_bytes, void* stream) {
    if (!w || !images || !out || !ws) return seeme_fail("seeme_resnet50_encode: null pointer");
    if (w->precision != SEEME_RESNET_FP32 && w->precision != SEEME_RESNET_BF16) return seeme_fail("seeme_resnet50_encode: precision must be fp32 (0) or bf16 (1)");
    if (image_format != SEEME_IMG_F32_NCHW && image_format != SEEME_IMG_U8_NHWC) return seeme_fail("seeme_resnet50_encode: image_format must be float NCHW (0) or uint8 NHWC (1)");
    if (B <= 0 || B > 1024) return seeme_fail("seeme_resnet50_encode: B must be in 1..1024");
    if ((image_format == SEEME_IMG_F32_NCHW && ((uintptr_t)images & 3)) || ((uintptr_t)out & 3) || ((uintptr_t)ws & 255))
        return seeme_fail("seeme_resnet50_encode: unaligned pointer (images 4, out 4, workspace 256 bytes)");
    const WsLayout l = ws_layout(B, w->precision);
    if (ws_bytes < l.total) return seeme_fail("seeme_resnet50_encode: workspace too small (seeme_resnet50_workspace_bytes)");
    if (const char* e = table_error(w)) return seeme_fail(e);
    hipStream_t st = (hipStream_t)stream;
    const int P = w->precision;
    const size_t es = esize(P);
    unsigned char* base = (unsigned char*)ws;
    unsigned char *X = base + l.x, *Y = base + l.y, *DS = base + l.ds, *T1 = base + l.t1, *T2 = base + l.t2;
    int rc;
    if ((rc = run_stem_pack(images, image_format, B, 224, 224, P, base + l.stem, st))) return rc;
    if ((rc = run_conv(w->conv[0], P, base + l.stem, B, 224, 224, nullptr, 1, Y, st))) return rc;
    if ((rc = run_maxpool(P, Y, B, 112, 112, 64, X, st))) return rc;
    int H = 56, C = 64, i = 1;
    if (w->tap[0]) SEEME_HIP(hipMemcpyAsync(w->tap[0], X, (size_t)B * H * H * C * es, hipMemcpyDeviceToDevice, st));
    for (int L = 0; L < 4; ++L) {
        for (int b = 0; b < kBlocks[L]; ++b) {
            const int s = w->conv[i + 1].stride, Ho = H / s;
            if ((rc = run_conv(w->conv[i], P, X, B, H, H, nullptr, 1, T1, st))) return rc;
            if ((rc = run_conv(w->conv[i + 1], P, T1, B, H, H, nullptr, 1, T2, st))) return rc;
            const unsigned char* res = X;
            if (b == 0) {
                if ((rc = run_conv(w->conv[i + 3], P, X, B, H, H, nullptr, 0, DS, st))) return rc;
                res = DS;
            }
            if ((rc = run_conv(w->conv[i + 2], P, T2, B, Ho, Ho, res, 1, Y, st))) return rc;
            i += b == 0 ? 4 : 3;
            unsigned char* tmp = X; X = Y; Y = tmp;
            H = Ho, C = 256 << L;
        }
        if (w->tap[L + 1]) SEEME_HIP(hipMemcpyAsync(w->tap[L + 1], X, (size_t)B * H * H * C * es, hipMemcpyDeviceToDevice, st));
    }
    if (P == SEEME_RESNET_BF16) hipLaunchKernelGGL(k_avgpool<true>, dim3((B * 2048 + 255) / 256), dim3(256), 0, st, X, out, B, 49, 2048);
    else hipLaunchKernelGGL(k_avgpool<false>, dim3((B * 2048 + 255) / 256), dim3(256), 0, st, X, out, B, 49, 2048);
    return seeme_check_launch("k_avgpool");
}

extern "C" int seeme_resnet_conv(const SeemeConv* c, int precision, const void* x, int B, int H, int W, const void* residual, int relu,
                                 void* y, void* stream) {
    if (!c || !x || !y) return seeme_fail("seeme_resnet_conv: null pointer");
    if (precision != SEEME_RESNET_FP32 && precision != SEEME_RESNET_BF16) return seeme_fail("seeme_resnet_conv: precision must be fp32 (0) or bf16 (1)");
    if (const char* e = conv_shape_error(*c, precision)) return seeme_fail(e);
    const void* wt = precision == SEEME_RESNET_BF16 ? (const void*)c->weight_bf16 : (const void*)c->weight;
    if (!wt || !c->bias) return seeme_fail("seeme_resnet_conv: null weight or bias");
    if (!aligned16(wt) || !aligned16(c->bias) || !aligned16(x) || !aligned16(y) || !aligned16(residual))
        return seeme_fail("seeme_resnet_conv: unaligned pointer (16 bytes)");
    if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W > (1L << 26)) return seeme_fail("seeme_resnet_conv: bad B / H / W");
    return run_conv(*c, precision, x, B, H, W, residual, relu, y, (hipStream_t)stream);
}

extern "C" int seeme_resnet_stem_pack(const void* images, int image_format, int B, int H, int W, int precision, void* y, void* stream) {
    if (!images || !y) return seeme_fail("seeme_resnet_stem_pack: null pointer");
    if (precision != SEEME_RESNET_FP32 && precision != SEEME_RESNET_BF16) return seeme_fail("seeme_resnet_stem_pack: precision must be fp32 (0) or bf16 (1)");
    if (image_format != SEEME_IMG_F32_NCHW && image_format != SEEME_IMG_U8_NHWC) return seeme_fail("seeme_resnet_stem_pack: image_format must be 0 or 1");
    if (!aligned16(y) || (image_format == SEEME_IMG_F32_NCHW && ((uintptr_t)images & 3))) return seeme_fail("seeme_resnet_stem_pack: unaligned pointer");
    if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W > (1L << 26)) return seeme_fail("seeme_resnet_stem_pack: bad B / H / W");
    return run_stem_pack(images, image_format, B, H, W, precision, y, (hipStream_t)stream);
}

extern "C" int seeme_resnet_maxpool(int precision, const void* x, int B, int H, int W, int C, void* y, void* stream) {
    if (!x || !y) return seeme_fail("seeme_resnet_maxpool: null pointer");
    if (precision != SEEME_RESNET_FP32 && precision != SEEME_RESNET_BF16) return seeme_fail("seeme_resnet_maxpool: precision must be fp32 (0) or bf16 (1)");
    if (!aligned16(x) || !aligned16(y)) return seeme_fail("seeme_resnet_maxpool: unaligned pointer (16 bytes)");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C * (int)esize(precision)) % 16 || (long)B * H * W > (1L << 26)) return seeme_fail("seeme_resnet_maxpool: bad B / H / W / C");
    return run_maxpool(precision, x, B, H, W, C, y, (hipStream_t)stream);
}
