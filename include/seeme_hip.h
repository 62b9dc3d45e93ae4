/* seeme_hip.h -- C-ABI of libseeme_hip.so: MI355X (gfx950) kernels for the SEE-ME
 * motion-latent-diffusion hot path.
 *
 * The reference (L-Scofano/SEEME) is pure Python/PyTorch and has no FFI boundary of its own
 * (SURVEY.md F1); its plug-in boundary is instantiate_from_config(cfg) in mld/config.py:25-32.
 * This header is therefore the *build-side* boundary proposed in SURVEY.md section 8(b): plain
 * pointers and sizes, no torch types.  Each entry point names the reference code it replaces.
 * The Python classes in seeme_amd/ (same constructor kwargs / methods / state_dict keys as the
 * reference classes) are the only callers; see INTEGRATION.md for the ctypes binding.
 *
 * Conventions
 *   - all tensor arguments are DEVICE pointers to contiguous fp32 (unless stated), row-major;
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*) and returns
 *     without synchronising; no allocation, no host sync inside (hipGraph-capturable);
 *   - return value 0 = ok, non-zero = error; seeme_last_error() gives a thread-local message;
 *   - workspaces are caller-allocated device buffers; *_workspace_bytes() gives the size.
 */
#ifndef SEEME_HIP_H
#define SEEME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEEME_D 256        /* latent_dim[-1]; every config of the reference uses 256 */
#define SEEME_NLAYERS 5    /* VAE: hard-coded mld_vae.py:51; denoiser: configs/modules/denoiser.yaml:6 */

enum { SEEME_ACT_NONE = 0, SEEME_ACT_RELU = 1, SEEME_ACT_GELU = 2, SEEME_ACT_SILU = 3 };
enum { SEEME_SCHED_NONE = 0, SEEME_SCHED_DDIM = 1, SEEME_SCHED_DDPM = 2 };

int seeme_version(void);
const char* seeme_last_error(void);

/* ------------------------------------------------------------------ generic fused linear
 * Y[M,N] = LN?( act( pre(A)[M,K] @ W[N,K]^T + bias ) + res )
 * Replaces torch.nn.functional.linear (+ fused neighbours) wherever the path uses it, e.g.
 * skel_embedding mld_vae.py:147, final_layer :251, skip Linear(2D,D) cross_attention.py:58-60
 * (A | A2 concatenation without materialising it), ResnetBlockFC respointnet.py:88-97.
 * K may be any size up to SEEME_LINEAR_MAX_K (a 32-row tile of A, padded to roundup16(K), shares a workgroup's 163,840 B
 * of LDS with the output tile; a larger K is refused): W rows must be readable for roundup16(K) floats (zero padded)
 * -- ldw says so -- and ldw must be a multiple of 4 with W 16-byte aligned.  A, A2, res and Y may have any 4-byte
 * alignment and any row stride >= their width; 16-byte aligned rows take the vector paths. */
#define SEEME_LINEAR_MAX_K 1008
typedef struct {
    const float* A;  int lda;         /* [M, K1] */
    const float* A2; int lda2;        /* optional [M, K-K1] (concat along K); NULL if unused */
    int K1;
    const float* W;  int ldw;         /* [N, >=roundup16(K)] */
    const float* bias;                /* [N] or NULL */
    const float* res; int ldr;        /* optional residual [M,N] added after act */
    const float* ln_w; const float* ln_b;          /* optional LayerNorm over N (needs N == 256) */
    const float* pre_ln_w; const float* pre_ln_b;  /* optional LayerNorm over K applied to A rows first */
    float* Y; int ldy;
    int M, N, K;
    int pre_act;                      /* activation applied to A (after pre-LN), SEEME_ACT_* */
    int act;                          /* activation applied to the product */
    float eps;
} SeemeLinearArgs;
int seeme_linear(const SeemeLinearArgs* args, void* stream);

/* ------------------------------------------------------------------ Transformer VAE
 * Weights of mld.models.architectures.mld_vae.MldVae (state_dict names in comments,
 * SURVEY.md App. A).  All fp32 device pointers in PyTorch layout ([out,in]). */
typedef struct {
    const float *in_w, *in_b;       /* self_attn.in_proj_weight [768,256], in_proj_bias */
    const float *out_w, *out_b;     /* self_attn.out_proj.{weight,bias} */
    const float *l1_w, *l1_b;       /* linear1 [ff,256] */
    const float *l2_w, *l2_b;       /* linear2 [256,ff] */
    const float *n1_w, *n1_b, *n2_w, *n2_b;
    /* decoder layers only (TransformerDecoderLayer, cross_attention.py:319-367); NULL in encoder */
    const float *ca_in_w, *ca_in_b; /* multihead_attn.in_proj_* */
    const float *ca_out_w, *ca_out_b;
    const float *n3_w, *n3_b;
} SeemeXfLayer;

typedef struct {
    SeemeXfLayer layer[SEEME_NLAYERS];   /* input_blocks.0, .1, middle_block, output_blocks.0, .1 */
    const float *skip_w[2], *skip_b[2];  /* linear_blocks.{0,1} [256,512] */
    const float *norm_w, *norm_b;        /* stack-final LayerNorm */
} SeemeSkipStack;

/* fp16 copies of the VAE matrices packed in MFMA fragment order (N padded to 16, K padded to 32),
 * Wp[(t * (K/32) + k/32) * 64 + lane][8] = W[16*t + (lane&15)][32*(k/32) + 8*(lane>>4) .. +7] for n-tile t:
 * the throughput mode of the VAE (fp16 MFMA operands, fp32 accumulation / residual stream). */
typedef struct { const uint16_t *in_w, *out_w, *l1_w, *l2_w; } SeemeXfLayerH;
typedef struct {
    SeemeXfLayerH enc[SEEME_NLAYERS], dec[SEEME_NLAYERS];
    const uint16_t *enc_skip[2], *dec_skip[2];
    const uint16_t *emb_w, *fin_w, *ca_fold_w;
    /* the decoder's sample-independent prologue (seeme_vae_dec_prologue_h16), built for dec_pro_T frames; NULL: none.  Decode reads
     * it only when dec_pro_T equals its own T, and never writes it. */
    const void* dec_pro; int dec_pro_T;
} SeemeVaeWeightsH;

typedef struct {
    int nfeats;                 /* F */
    int ff;                     /* 128 (hard-coded mld_vae.py:53) */
    const float* token;         /* global_motion_token [2,256] */
    const float* pe_enc;        /* query_pos_encoder.pe [500,1,256] */
    const float* pe_dec;        /* query_pos_decoder.pe */
    const float* emb_w; int emb_ldw; /* skel_embedding.weight [256, roundup16(F)] zero-padded copy */
    const float* emb_b;
    const float* fin_w;         /* final_layer.weight [F,256] */
    const float* fin_b;
    SeemeSkipStack enc, dec;
    /* decoder cross-attention to the single latent token, folded on the host:
     * c_l = ca_fold_w[l*256:(l+1)*256] z + ca_fold_b[...],  ca_fold_w = out_proj_l . W_v_l,  ca_fold_b = out_proj_l b_v_l + b_o_l */
    const float* ca_fold_w;     /* [5*256, 256] */
    const float* ca_fold_b;     /* [5*256] */
    const SeemeVaeWeightsH* h16; /* NULL: fp32-exact MFMA path (parity); else fp16-operand MFMA path */
} SeemeVaeWeights;

size_t seeme_vae_workspace_bytes(int B, int T);

/* MldVae.encode (mld_vae.py:128-193) up to the posterior parameters:
 * features [B,T,F], lengths [B] (int32, device) -> mu [B,256], logvar [B,256]
 * (the caller forms std = exp(logvar)^0.5 and the Normal; rsample is RNG, host side). */
int seeme_vae_encode(const SeemeVaeWeights* w, const float* features, const int32_t* lengths,
                     int B, int T, float* mu, float* logvar, void* workspace, size_t ws_bytes, void* stream);

/* MldVae.decode, arch encoder_decoder (mld_vae.py:195-256): z [B,256], lengths -> feats [B,T,F]
 * (padded frames not zeroed, as in the reference :253). */
int seeme_vae_decode(const SeemeVaeWeights* w, const float* z, const int32_t* lengths,
                     int B, int T, float* feats, void* workspace, size_t ws_bytes, void* stream);

/* The fp16 decoder's first-layer inputs for T frames.  The queries are zeros + learned positional rows, so the rows and their
 * q | K | V^T depend on the weights and on T only: built once into buf (16-byte aligned, seeme_vae_dec_prologue_bytes(T) bytes; x rows
 * [T][256] fp32, q [T][256] fp16, K and V^T fragment-packed for ONE sequence) and handed to decode through SeemeVaeWeightsH.dec_pro.
 * Rebuild it whenever the weights change. */
size_t seeme_vae_dec_prologue_bytes(int T);
int seeme_vae_dec_prologue_h16(const SeemeVaeWeights* w, int T, void* buf, size_t bytes, void* stream);

/* ------------------------------------------------------------------ denoiser + sampling loop
 * mld.models.architectures.mld_denoiser.MldDenoiser (arch trans_enc, MD_TRANS layers
 * mdiff_transformer.py:257-304) and MLD._diffusion_reverse (mld/models/modeltype/mld.py:432-511).
 *
 * Weight image: the host packs the state_dict once into
 *   wg : the matrices in stream order, element type fp32, bf16 or fp16 (wdtype 0 / 1 / 2); a [N,K] PyTorch
 *        matrix is stored as [K/4][N][4] (fp32, vector-ALU path) or as the per-wave matrix-core operand stream
 *        [wave 8][K/32][N/128][lane 64][8] (16-bit), so that every wave-load is 1 KiB contiguous;
 *   vp : fp32 vectors (biases, LayerNorm params, pe row 0);
 * in the order documented in seeme_amd/csrc/den_layout.h; seeme_den_layout() exports the offsets.
 * sa_fold = 1 (one attention head): the image's in_proj V rows / bias and kv_cat_w / kv_cat_b V rows hold
 * W_o W_v and W_o b_v + b_o instead of W_v, b_v, and the out_proj slot is unused (seeme_amd/mld_denoiser.py).
 */
typedef struct {
    const void*  wg;   int wdtype;       /* 0 = fp32, 1 = bf16, 2 = fp16 */
    const float* vp;
    const int64_t* layout;               /* device copy of the seeme_den_layout() table (155 int64) */
    int nhead;                           /* 1, 2 or 4 */
    int ff_sa;                           /* 1024 (hard-coded mdiff_transformer.py:279) */
    int ff;                              /* 128 */
    /* PyTorch-layout fp32 tensors used by the per-call table builders */
    const float* kv_cat_w; const float* kv_cat_b;       /* [5*512,256]: sa in_proj K|V rows per layer */
    const float* style_cat_w; const float* style_cat_b; /* [5*1024,256]: ca emb_layers.1 | ffn emb_layers.1 */
    const float* time_w1; const float* time_b1; const float* time_w2; const float* time_b2;
    const float* ca_kv_w[SEEME_NLAYERS]; const float* ca_kv_b[SEEME_NLAYERS];   /* [512,256] key|value per layer */
    const float* ca_tn_w[SEEME_NLAYERS]; const float* ca_tn_b[SEEME_NLAYERS];   /* ca_block.text_norm */
    /* key|value of all layers with the text_norm affine folded in: [5*512,256] = W_l diag(tn_w_l),
     * bias W_l tn_b_l + b_l; applied to the affine-free LayerNorm of the condition (ln_ones / ln_zeros) */
    const float* ca_fold_w; const float* ca_fold_b;
    const float* ln_ones; const float* ln_zeros;                                /* [256] each */
    int sa_fold;                                                                /* 1: out_proj folded into V (nhead == 1) */
    /* ca_block.proj_out of each layer (StylizationBlock, mdiff_transformer.py:152-163), for seeme_denoiser_ca_tables */
    const float* ca_pn_w; const float* ca_pn_b;   /* proj_out.norm of the 5 layers, [5,256] each */
    const float* ca_po_w; const float* ca_po_b;   /* proj_out.out_layers.2 of the 5 layers, [5,256,256] and [5,256] */
} SeemeDenoiserWeights;

/* per-row time tables: floats per row = 5*512 (sa K|V of the time token) + 5*1024 (AdaLN scale|shift, ca|ffn) */
#define SEEME_TROW 7680
/* per-sample condition tables: floats per (sample, token) = 5 layers * (sa K|V 512 + ca key|value 512) */
#define SEEME_CROW 5120

size_t seeme_denoiser_workspace_bytes(int n_rows, int B, int N);

/* Build the time tables for `n_rows` timestep feature rows tfeat [n_rows,256] (sinusoidal features,
 * tools/embeddings.py:245-285, computed by the host) -> ttab [n_rows, SEEME_TROW].
 * Batch-invariant in sampling. */
int seeme_denoiser_time_tables(const SeemeDenoiserWeights* w, const float* tfeat, int n_rows,
                               float* ttab, void* workspace, size_t ws_bytes, void* stream);

/* Build the per-sample condition tables for cond [Bc,N,256] (batch-first) -> ctab [Bc,N,SEEME_CROW]
 * (step-invariant K/V of the condition tokens). */
int seeme_denoiser_cond_tables(const SeemeDenoiserWeights* w, const float* cond, int Bc, int N,
                               float* ctab, void* workspace, size_t ws_bytes, void* stream);

/* ONE condition token (N == 1): the ca_block's contribution does not depend on the latent (the key softmax over
 * a single token is 1, mdiff_transformer.py:231-237), so it is tabulated per (sample, table row, layer):
 *   catab[bc][r][l] = proj_out.out_layers( SiLU( LN(value_l(cond_bc)) * (1 + scale_{row,l}) + shift_{row,l} ) )
 * with row = trow[r] (trow_per_sample 0, R = n_rows rows per sample) or trow[bc % n_b] (trow_per_sample 1, R = 1,
 * n_b = number of trow entries).  ctab [Bc,1,SEEME_CROW]; catab [Bc,R,5,256].
 * workspace >= 5*Bc*R*256 floats. */
int seeme_denoiser_ca_tables(const SeemeDenoiserWeights* w, const float* ctab, const float* ttab, const int32_t* trow,
                             int trow_per_sample, int n_trow, int Bc, float* catab,
                             void* workspace, size_t ws_bytes, void* stream);

/* ONE condition token: seeme_denoiser_cond_tables + seeme_denoiser_ca_tables as ONE launch, for cond [Bc,1,256].  Each
 * workgroup of a catab tile forms the value columns of its samples itself, so ctab and catab come out of one grid with the
 * bits of the two calls (same MFMAs, operands and k order per element) and no workspace.  `zero` (optional, 16-byte aligned):
 * zero_bytes bytes that the same launch sets to zero -- the exchange buffer of a cluster launch that follows on `stream`
 * (SeemeDenCluster.xchg_zeroed). */
int seeme_denoiser_tables1(const SeemeDenoiserWeights* w, const float* cond, const float* ttab, const int32_t* trow,
                           int trow_per_sample, int n_trow, int Bc, float* ctab, float* catab,
                           void* zero, size_t zero_bytes, void* stream);

typedef struct {
    int B;                 /* samples (latents rows) */
    int N;                 /* condition tokens per sample */
    int steps;             /* loop iterations (1 for a plain forward) */
    int sched;             /* SEEME_SCHED_* ; NONE: out = eps of the single step */
    int cfg;               /* 1: ctab holds 2B samples (uncond first, mld.py:489) and guidance is applied */
    float guidance_scale;
    const float* latents;  /* [B,256] initial */
    const float* ctab;     /* [B or 2B, N, SEEME_CROW] */
    const float* ttab;     /* [rows, SEEME_TROW] */
    const int32_t* trow;   /* sampling: [steps] row of ttab per step; forward: [B] row per sample */
    int trow_per_sample;   /* 0: trow[step], 1: trow[b] */
    const float* coef;     /* [steps,8] scheduler scalars per step (see seeme_amd/schedulers.py); required unless sched == SEEME_SCHED_NONE */
    const float* noise;    /* optional [steps,B,256] step noise (eta>0 / DDPM), NULL otherwise */
    float* out;            /* [B,256] */
    const float* catab;    /* N == 1: [B or 2B, R, 5, 256] from seeme_denoiser_ca_tables (R = steps, or 1 with trow_per_sample) */
    float* save;           /* training forward only (steps == 1, no CFG, unfolded fp32 image, query GEMV kept): [B, SEEME_DEN_SAVE_FLOATS]
                            * intermediates for seeme_denoiser_backward (seeme_amd/csrc/den_train.h); NULL otherwise */
    int force_query;       /* 1: keep the ca_block query / proj_out GEMVs even for one condition token (differentiable path) */
    const unsigned char* drop;   /* training forward only (with save): dropout keep-masks [B, SEEME_DEN_DROP_BYTES] of the MD layers'
                                  * nn.Dropout sites in training mode (layout csrc/den_train.h DM_*), or NULL (eval arithmetic) */
    float drop_scale;      /* 1 / (1 - p) */
    int xcds;              /* seeme_denoiser_sample only: 0 or 8 = workgroups dealt to all XCDs; k in 1..7 = the working workgroups sit on
                            * k XCDs (blockIdx % 8 < k; assumes the round-robin dispatch of SPX mode -- any other placement only changes which
                            * L2s are shared, never results).  Fewer L2s re-fetching the 9 MB image each step: B = 32 on 2 XCDs pulls 962 MB per
                            * 50-step launch from the Infinity Cache instead of 3.72 GB.  A choice of the CALLER (it knows whether the launch has
                            * the chip to itself); the library keeps no state about streams. */
} SeemeSampleArgs;
#define SEEME_DEN_DROP_BYTES 10960

int seeme_denoiser_sample(const SeemeDenoiserWeights* w, const SeemeSampleArgs* a, void* stream);

/* ---- the same loop with ONE SAMPLE SPLIT OVER C WORKGROUPS (csrc/den_cluster.inc.hip; MLD._diffusion_reverse, mld.py:467-497, at
 * batch sizes that leave most of the chip idle: B x C <= 256).  One attention head, one or two condition tokens, no CFG.
 *   wgc : the cluster weight image [layer 5][CU C][unit][wave 8][load][lane 64][16 B], packed by the host
 *         (seeme_amd/mld_denoiser.py, geometry from seeme_den_cluster_layout); the skip linears of layers 3, 4 are folded
 *         into that layer's in_proj;
 *   vpc : the vector array of seeme_den_layout() order with in_b of layers 3, 4 = W_in' b_skip + b_in';
 *   xchg: exchange workspace (>= seeme_den_cluster_xchg_bytes(B, C), 16-byte aligned), zeroed by the call on `stream` (unless xchg_zeroed).  Word 0
 *         of it is non-zero after the launch if a cluster gave up waiting for a peer (results invalid), word 1 counts the
 *         clusters that ran with L2-local granule stores.
 *   placement 0: the workgroups of a cluster have equal blockIdx % 8 (one XCD under round-robin dispatch), 1: consecutive
 *   blockIdx.  flags bit 0: granule stores always write-through.  Placement and flags change speed, never results. */
typedef struct {
    const void*  wgc;  int wdtype;       /* 0 = fp32, 1 = bf16, 2 = fp16 */
    const float* vpc;
    int C;                               /* workgroups (CUs) per sample: 2, 4 or 8 */
    int placement;
    int flags;
    void* xchg; size_t xchg_bytes;
    int query;                           /* 0: image packed for ONE condition token (ca term from seeme_denoiser_ca_tables); 1: for two
                                          * (units of ca_block.query / proj_out included, one more exchange per layer) */
    int samples;                         /* 0 / 1: one sample per cluster (k_den_cluster).  2..8: the large-batch form (k_den_cluster_ms,
                                          * csrc/den_cluster_ms.inc.hip): a cluster owns up to `samples` chains that share its weight stream
                                          * (two or four MFMA A rows per sample, wave s = epilogue wave of sample s): fp16 image (C = 4 or 8) or bf16
                                          * image (C = 4, at most 4 samples), one or two condition tokens, one table row per step; ceil(B / samples) rounded up to 8 clusters x C <= CUs;
                                          * xchg >= seeme_den_cluster_ms_xchg_bytes(B, C, samples) */
    int xchg_zeroed;                     /* 1: the caller zeroed the first seeme_den_cluster[_ms]_xchg_bytes(...) bytes of xchg on `stream`
                                          * after the previous cluster launch (seeme_denoiser_tables1 does): the call skips its own
                                          * memset.  0: the call zeroes them */
} SeemeDenCluster;
size_t seeme_den_cluster_xchg_bytes(int B, int C);
size_t seeme_den_cluster_ms_xchg_bytes(int B, int C, int samples);
/* out[0] units per (layer, CU) incl. padding, [1] bytes per unit, [2] image bytes, [3] wave-loads per unit, [4] k per wave-load,
 * [5..11] first unit of stage A (x half), A (skip half), B, C, D, E, F, [12] of G (ca query), [13] of H (ca proj_out) (-1 when query = 0) */
int seeme_den_cluster_layout(int C, int wdtype, int query, int64_t* out, int cap);
int seeme_denoiser_sample_cluster(const SeemeDenoiserWeights* w, const SeemeDenCluster* cl, const SeemeSampleArgs* a, void* stream);

/* ---- stage-2 training (MLD._diffusion_process, mld.py:582-631, and the backward of MldDenoiser.forward) ----
 * Forward = seeme_denoiser_sample with steps 1, SCHED_NONE, per-sample rows, force_query 1 and `save` set, on the
 * unfolded fp32 image.  seeme_den_train_pack refreshes that image, its transposed twin and the vector array from the
 * parameter tensors (mats: [5][10] device pointers in den_layout.h order, NULL where a layer has no skip linear).
 * seeme_denoiser_backward walks the chain in reverse (one workgroup per sample) and writes, per sample, x and dy of
 * every linear + LayerNorm parameter terms + d(first layer input) into gout [B, DB_TOTAL] (seeme_amd/csrc/den_train.h),
 * and the gradients of the tables into dctab [B,N,SEEME_CROW] / dttab [B,SEEME_TROW].  The batch reductions
 * (dW = sum_b dy_b x_b^T) are left to the host.  seeme_den_train_layout: [5][10] offsets of the transposed image,
 * its size, floats of `save` per sample, floats of `gout` per sample, floats per layer block of `gout`. */
int seeme_den_train_layout(int64_t* out, int cap);
int seeme_den_train_pack(const float* const* mats, float* img_f, float* img_b, const float* const* vec_src,
                         const int* vec_n, const int64_t* vec_dst, int n_vec, float* vp, void* stream);
int seeme_denoiser_backward(const SeemeDenoiserWeights* w, const void* img_bwd, int B, int N, const float* save,
                            const float* ctab, const float* ttab, const int32_t* trow, const float* dout,
                            float* gout, float* dctab, float* dttab, void* stream);
/* The same with the dropout keep-masks the forward was given (SeemeSampleArgs.drop / drop_scale) and the caller's XCD packing
 * (SeemeSampleArgs.xcds; seeme_denoiser_backward runs unpacked). */
int seeme_denoiser_backward_drop(const SeemeDenoiserWeights* w, const void* img_bwd, int B, int N, const float* save,
                                 const float* ctab, const float* ttab, const int32_t* trow, const float* dout,
                                 float* gout, float* dctab, float* dttab, const unsigned char* drop, float drop_scale, int xcds, void* stream);

/* Offsets of the packed weight image (30 per layer x 5, then pe0, fnw, fnb, wg_total, vp_total). */
int seeme_den_layout(int ff_sa, int ff, int64_t* out, int cap);

/* ------------------------------------------------------------------ SMPL linear blend skinning
 * smplx.SMPL.forward (call sites mld/models/modeltype/mld.py:764-770 ...). */
typedef struct {
    int V;                        /* 6890 */
    const float* v_template;      /* [V,3] (flat [V*3] = bias of the blend GEMM) */
    const float* blend_w;         /* [V*3, 224]: cols 0..9 shapedirs, 10..216 posedirs^T, 217..223 zero */
    const float* lbs_weights;     /* [V,24] */
    const float* J_template;      /* [24,3]  = J_regressor @ v_template      (precomputed) */
    const float* J_shapedirs;     /* [24,3,10] = J_regressor @ shapedirs */
    const int32_t* parents;       /* [24] kinematic tree, parents[0] = -1 */
    /* compact copy of the model restricted to the 21 extra-joint vertices (smplx VertexJointSelector) */
    const float* ex_template;     /* [21,3] */
    const float* ex_shapedirs;    /* [21*3,10] */
    const float* ex_posedirs;     /* [207, 63] */
    const float* ex_weights;      /* [21,24] */
} SeemeSmplModel;

size_t seeme_smpl_workspace_bytes(int M);

/* pose: axis-angle [M,72] (pose2rot=True) or rotation matrices [M,24,9]; betas [M,10]; transl [M,3] or NULL.
 * joints [M,45,3] (24 posed joints + 21 vertex-picked joints); vertices [M,V,3] or NULL (joints-only
 * fast path: no mesh is formed). */
int seeme_smpl_lbs(const SeemeSmplModel* m, const float* betas, const float* pose, int pose_is_rotmat,
                   const float* transl, int M, float* joints, float* vertices,
                   void* workspace, size_t ws_bytes, void* stream);

/* Gradient of the 24 posed joints (the first 24 of seeme_smpl_lbs's joints, axis-angle pose) w.r.t. pose [M,72] and transl
 * [M,3] (dtransl may be NULL): djoints [M, dj_stride >= 24, 3].  Replaces autograd through smplx's lbs for the joints loss of
 * train_vae_forward (mld.py:764-773,871-878). */
int seeme_smpl_joints_backward(const SeemeSmplModel* m, const float* betas, const float* pose, const float* djoints, int dj_stride,
                               float* dpose, float* dtransl, int M, void* stream);

/* DATA_TYPE 'rot6d' (mld.py:703-742): the 24 posed joints [M,24,3] straight from the renormed features r6 [M,24,6] -- Gram-Schmidt
 * per joint (order: SEEME_GEO_ROT6D_PROHMR or SEEME_GEO_ROT6D_DIFFUSION, as seeme_geometry), rest joints, kinematic chain -- in one
 * launch; the same joints as seeme_geometry followed by seeme_smpl_lbs(pose_is_rotmat = 1).  betas [M,10] or NULL (zeros: the
 * reference's create_beta=False call); transl [M,3] or NULL. */
int seeme_smpl_joints_rot6d(const SeemeSmplModel* m, const float* betas, const float* r6, int order, const float* transl, int M,
                            float* joints, void* stream);
/* ... and their gradient w.r.t. r6 (dr6 [M,24,6]) and transl (dtransl [M,3], may be NULL): djoints [M, dj_stride >= 24, 3]. */
int seeme_smpl_joints_rot6d_backward(const SeemeSmplModel* m, const float* betas, const float* r6, int order, const float* djoints,
                                     int dj_stride, float* dr6, float* dtransl, int M, void* stream);

/* ------------------------------------------------------------------ rotation helpers / renorm
 * mld/utils/geometry2.py: aa_to_quat :33-54, aa_to_rotmat :56-72, quat_to_rotmat :74-95,
 * rot6d_to_rotmat :98-117 ('prohmr' / 'diffusion' column order).  in [M,3|4|6] -> out [M,4] or [M,3,3]. */
enum { SEEME_GEO_AA_TO_QUAT = 0, SEEME_GEO_AA_TO_ROTMAT = 1, SEEME_GEO_QUAT_TO_ROTMAT = 2,
       SEEME_GEO_ROT6D_PROHMR = 3, SEEME_GEO_ROT6D_DIFFUSION = 4 };
int seeme_geometry(int op, const float* in, float* out, int M, void* stream);
/* EgoBodyDataModule.renorm (mld/data/EgoBody.py:151-157): y = x * std[:F] + mean[:F], x [rows,F]. */
int seeme_renorm(const float* x, const float* mean, const float* stdv, float* y, long rows, int F, void* stream);

/* ------------------------------------------------------------------ PointNet scene encoder
 * EgoHMR.models.respointnet.ResnetPointnet(out_dim, hidden 256) (respointnet.py:6-59); PyTorch-layout
 * fp32 weights, fc_pos_0.weight zero padded to [512,16]. */
typedef struct {
    int out_dim;                          /* 512 */
    const float* pos_w; const float* pos_b;          /* fc_pos_0 [512,16 padded], [512] */
    const float* fc0_w[4]; const float* fc0_b[4];    /* block_i.fc_0 [256,512] */
    const float* fc1_w[4]; const float* fc1_b[4];    /* block_i.fc_1 [256,256] */
    const float* sc_w[4];                            /* block_i.shortcut [256,512], no bias */
    const float* fcc_w; const float* fcc_b;          /* fc_c [out_dim,256] */
} SeemePointnetWeights;
size_t seeme_pointnet_workspace_bytes(int B, int P);
/* points [B,P,3] -> out [B,out_dim] */
int seeme_pointnet_encode(const SeemePointnetWeights* w, const float* points, int B, int P, float* out,
                          void* workspace, size_t ws_bytes, void* stream);

/* bf16-MFMA variant (fp32 accumulation): the same weights as bf16 copies packed in MFMA fragment order.
 * One fused persistent kernel per ResnetBlockFC on 256-point tiles, max-pool folded into the epilogue.  Results
 * differ from the fp32 path by bf16 rounding of weights and activations (tolerance stated in the tests).
 * Every member is required: a NULL one is an error. */
typedef struct {
    const uint16_t* posf;       /* fc_pos_0 (weight [512,3], bias) as split-bf16 operands of v_mfma_f32_16x16x16_bf16,
                                 * w = hi + lo: [32 n-tiles][64 lanes][4], lane = 16*kq + q for column 16*t + q:
                                 * kq 0: whx why whz whx | kq 1: why whz wlx wly | kq 2: wlz bh bl 0 | kq 3: 0 */
    /* Block kernels (csrc/pointnet_bf16.hip): per block ONE weight stream of
     * 24 slots x 16 fragments x 64 lanes x 8 bf16, in the order a 256-point tile consumes it.  Fragment (feature tile nt,
     * k-block kb): lane 16*kq + m, element j = W[16 nt + m][32 kb + 16 (j/4) + 4 kq + j%4] -- the k order in which an
     * accumulator tile pair is the next B operand; the activations between blocks are stored in that order too.
     *   block_0:   slots 0..15 fc_0 k-block = slot, fragment nt; slot 16 + 4 g + p: fc_1 tiles 8 g + n, k-blocks 2 p + kbi
     *              at fragment 8 kbi + n.
     *   block_1-3: slots 0..7 fc_0[:, :256] k-block = slot, fragment nt; slot 8 + 8 g + kb: fragments 0..7 shortcut[:, :256]
     *              tiles 8 g + n, fragments 8..15 fc_1 tiles 8 g + n, both k-block kb. */
    const uint16_t* stream[4];
    const uint16_t* sc3f;       /* block_0.shortcut folded through fc_pos_0 (both linear, no bias: respointnet.py:35,84,93) to
                                 * [256][4] = ( Ws Wp | Ws bp ), as split-bf16 fragments like posf: [16 n-tiles][64 lanes][4] */
} SeemePointnetBf16;
size_t seeme_pointnet_bf16_workspace_bytes(int B, int P);
int seeme_pointnet_encode_bf16(const SeemePointnetWeights* w, const SeemePointnetBf16* wb, const float* points,
                               int B, int P, float* out, void* workspace, size_t ws_bytes, void* stream);

/* Weight gradients of the denoiser chain in one launch: for every tile {int x_col, y_col, ldo, nn, kk, pad; int64 out_off}
 * out[out_off + n*ldo + k] = sum_b gout[b*ldg + y_col + n] * gout[b*ldg + x_col + k], n < nn <= 32, k < kk <= 256, where
 * gout is the per-sample buffer of seeme_denoiser_backward (x and dy of every linear, csrc/den_train.h).  Replaces the
 * autograd weight-gradient accumulation of loss.backward() through MldDenoiser.forward (mld.py:582-631). */
/* (out is stored, not accumulated; elements of out outside the tiles -- the ldo - kk gap of a row included -- are not written; the sum
 * over b runs in order in one thread: two launches give the same bits.) */
int seeme_den_wgrad(const float* gout, int ldg, int B, const void* tiles, int n_tiles, float* out, void* stream);
/* The chain's vector gradients (biases, LayerNorm weights / biases) in one launch: out[q] = sum_b gout[b*ldg + idx[q]], q < n,
 * and dpe_row0[c] = sum_b gout[b*ldg + dx0_col + c], c < 256 (query_pos.pe row 0; NULL to skip the write -- the 256 columns from
 * dx0_col are read either way and must lie inside a row).  idx may repeat.  Same reference as above. */
int seeme_den_vecgrad(const float* gout, int ldg, int B, const int64_t* idx, int n, float* out, int dx0_col, float* dpe_row0,
                      void* stream);

/* AdamW step of a list of fp32 tensors in one launch, torch.optim.AdamW arithmetic (amsgrad off): replaces the
 * optimiser step Lightning runs after training_step (reference: mld/models/modeltype/base.py configure_optimizers,
 * train.py:127-149).  chunks: device array of {int tensor, int count, int64 offset}; params / grads / exp_avg /
 * exp_avg_sq: device arrays of per-tensor base pointers; step = the 1-based step count (bias corrections and the
 * other scalar factors are formed in double, as PyTorch forms them). */
int seeme_adamw_step(const void* chunks, int n_chunks, void* const* params, const void* const* grads, void* const* exp_avg,
                     void* const* exp_avg_sq, double lr, double beta1, double beta2, double eps, double weight_decay,
                     double step, void* stream);

/* The same update with the step count and the learning rate read from device memory (step_lr = {step, lr}, the caller
 * increments step_lr[0] on the stream before the launch): nothing in the launch depends on host state, so a captured
 * hipGraph of the whole training step (MLD.capture_training_step) advances correctly from replay to replay.  Replaces the
 * same optimiser step as seeme_adamw_step. */
int seeme_adamw_step_dev(const void* chunks, int n_chunks, void* const* params, const void* const* grads, void* const* exp_avg,
                         void* const* exp_avg_sq, const float* step_lr, double beta1, double beta2, double eps,
                         double weight_decay, void* stream);

/* The same update with the training loop's two options in the same pass (seeme_amd/optim.py: FusedAdamWStep with ema_decay /
 * grad_clip_norm; the reference has neither, Lightning's gradient_clip_val and an EMA callback are what a user would add).
 * Per element, in fp32: g' = g * grad_scale[0] (skipped when grad_scale is NULL; g is read and never written); the four AdamW
 * lines of seeme_adamw_step on g'; e += (p_new - e) * (1 - d_t) (skipped when ema is NULL), with
 * d_t = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay, t = the 1-based count of this update, formed in double: on
 * the host from `step` when step_lr is NULL, in the kernel from step_lr[0] otherwise.  With ema == NULL and grad_scale == NULL
 * the results are the bits of seeme_adamw_step / seeme_adamw_step_dev. */
typedef struct {
    const void* chunks;               /* device array of {int tensor, int count, int64 offset} */
    int n_chunks;
    void* const* params;              /* device arrays of per-tensor base pointers */
    const void* const* grads;
    void* const* exp_avg;
    void* const* exp_avg_sq;
    void* const* ema;                 /* NULL: no EMA shadow */
    const float* step_lr;             /* device {step, lr}; NULL: the host fields lr and step */
    double lr, step;
    double beta1, beta2, eps, weight_decay;
    double ema_decay;                 /* d, 0 <= d < 1 */
    int ema_warmup;                   /* 0 or 1 */
    const float* grad_scale;          /* device float (seeme_grad_norm's out + 1); NULL: 1 */
} SeemeAdamWEx;
int seeme_adamw_step_ex(const SeemeAdamWEx* a, void* stream);
int seeme_adamw_ex_bytes(void);

/* Global L2 norm of the gradients behind the same chunk table and pointer table, and the clipping scale of
 * torch.nn.utils.clip_grad_norm_: out[0] = sqrt(sum g^2), out[1] = min(1, max_norm / (out[0] + 1e-6)); a non-finite norm
 * propagates as it does there.  Two launches: one workgroup per chunk sums the squares in double (per lane, then the lane sums
 * in a fixed order) into ws[chunk]; one workgroup adds the partials in chunk order.  No atomics and no host read: equal inputs
 * give equal bits, and both launches can sit in a captured step.  ws: 8-byte aligned, seeme_grad_norm_workspace_bytes(n_chunks). */
size_t seeme_grad_norm_workspace_bytes(int n_chunks);
int seeme_grad_norm(const void* chunks, int n_chunks, const void* const* grads, double max_norm, float* out /* {norm, scale} */,
                    void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ stage-2 training step: the work around the chain
 * Replaces, for MLD.train_diffusion_forward / _diffusion_process (mld/models/modeltype/mld.py:582-631,887-1017), the
 * PyTorch ops (and their autograd backward) that build the chain's inputs: posterior rsample (mld_vae.py:186-193),
 * scheduler.add_noise (:604-606), the sinusoidal timestep features + TimestepEmbedding MLP (tools/embeddings.py:207-285),
 * output_scene (mld.py:257-261) and MldDenoiser.forward's per-layer condition / time tables (mld_denoiser.py:150-256:
 * self-attention K|V of the condition and time tokens, text_norm + linear-attention key|value, AdaLN scale|shift rows). */
typedef struct {
    int B, N;                 /* samples, condition tokens per sample */
    const float* dist;        /* [2, dist_rows, 256]: row 0 mu, row 1 logvar (seeme_vae_encode_dist), z = mu + eps * exp(logvar / 2); rows [0,B) = target,
                                 rows [B,2B) = condition motion when eps_c is set */
    int dist_rows;
    const float* eps_z;       /* [B,256] rsample noise of the target */
    const float* eps_c;       /* [B,256] rsample noise of the condition latent, or NULL (no 'interactee' condition) */
    int slot_c;               /* token slot of the condition latent in cond */
    float* cond;              /* [B,N,256] condition tokens (slot_c written here) */
    const float* noise;       /* [B,256] */
    const int64_t* timesteps; /* [B] */
    const float* acp;         /* alphas_cumprod [num_train_timesteps] */
    const float* freq;        /* [128] exp(-ln(max_period) * j / (128 - freq_shift)) */
    int flip_sin_to_cos;
    float* latents;           /* [B,256] z */
    float* noisy;             /* [B,256] x_t */
    float* tfeat;             /* [B,256]: [sin | cos](float(t) * freq[j]), the product in fp32; cos first when flip_sin_to_cos */
} SeemeGlueRows;                 /* noisy = sqrt(acp[t]) z + sqrt(1 - acp[t]) noise.  1 <= N <= 4; with eps_c, dist_rows >= 2B. */
int seeme_glue_rows(const SeemeGlueRows* a, void* stream);
/* F.layer_norm(x, (256,)) without affine: xhat [M,256], rstd [M]. */
int seeme_glue_ln(const float* x, float* xhat, float* rstd, int M, void* stream);

/* One problem of seeme_grouped_gemm:  C[i,j] (+)= sum_s sum_{k < seg_len[s]} A_s[i,k] * B_s[k,j]  (+ bias[j]) (* epilogue)
 * with A_s[i,k] = pro_a(a[s][i*a_rs + k*a_ks[s]]) and B_s[k,j] = pro_b(b[s][k*b_ks[s] + j*b_cs]); prologue modes: 0 none, 1 SiLU,
 * 2 ReLU, 3 affine v*p0[idx] + p1[idx] (idx = k for A, j for B; k counts WITHIN the segment, every segment reads p0 / p1 from
 * element 0, so they hold max seg_len entries).  epi 1: multiply by SiLU'(e0[i*e_ld + j]); epi 2: by alpha.  The order is
 * C = ((A B + bias) * epilogue) + addend, and then the accumulate mode is applied to that value.  1 <= nseg <= 10 and every
 * seg_len >= 1.
 * colsum (needs a_rs == 1 and a_pro == 0): colsum[i] (+)= sum_s sum_k a[s][i,k], the raw operand -- the bias gradient that comes
 * free with a weight gradient; it is stored / added / atomically added as `accumulate` says for C.  tile0 / tiles_n: position
 * of the problem's 64x64 tiles in the launch (tile0 ascending over the table; a problem has nbatch * ceil(M/64) * tiles_n tiles). */
typedef struct {
    const float* a[10];
    const float* b[10];
    int seg_len[10];
    long a_ks[10];
    long b_ks[10];
    int nseg;
    long a_rs, b_cs;
    float* c;
    long ldc;
    int M, N;
    int a_pro;
    const float* a_p0;
    const float* a_p1;
    int b_pro;
    const float* b_p0;
    const float* b_p1;
    const float* bias;
    int epi;
    const float* e0;
    long e_ld;
    int accumulate;
    float* colsum;
    int tile0, tiles_n;
    int nbatch;               /* > 1: nbatch independent problems of this shape; a[s] / b[s] / c advance by the strides below */
    long a_bstride, b_bstride, c_bstride;
    float alpha;              /* epi 2: C = alpha * (A B + bias) */
    const float* addend;      /* optional [M,N] (row stride add_ld) added after the epilogue */
    long add_ld;
} SeemeGemmProblem;              /* accumulate: 0 store, 1 C += (one writer), 2 atomicAdd (nbatch members share C: split reduction).
                                  * Batch members may share C (c_bstride == 0) ONLY with accumulate == 2: with 0 or 1 they would race. */
int seeme_grouped_gemm(const SeemeGemmProblem* probs_dev, int n_probs, int n_tiles, void* stream);
int seeme_gemm_problem_bytes(void);
/* Plain large fp32 GEMM on the matrix cores (the projections of the stage-1 training step): C[M,N] = A[M,K] B + bias[N] + addend,
 * B = W[N,K] (b_is_nt: y = x W^T, F.linear) or W[K,N] (data gradient dx = dy W).  M, N multiples of 128, K of 32, operands 16-byte
 * aligned with strides in multiples of 4 floats; anything else goes through seeme_grouped_gemm. */
/* Large weight gradient: G[Nout,Kin] += dY[M,Nout]^T X[M,Kin], gbias[Nout] += column sums of dY (NULL to skip); Nout, Kin
 * multiples of 128; split over row chunks with atomic accumulation (G must hold the value to add to). */
int seeme_wgrad128(const float* dY, long ldy, const float* X, long ldx, int M, int Nout, int Kin, float* G, long ldg, float* gbias,
                   void* stream);
int seeme_gemm128(const float* A, long lda, const float* B, long ldb, int b_is_nt, float* C, long ldc, int M, int N, int K,
                  const float* bias, const float* addend, long add_ld, void* stream);

/* Element-wise middle of the backward: d cond = sum_l dcs[l] + LayerNorm-backward(sum_l dxl[l] * tn_w[l]); text_norm
 * affine gradients g_tn_w[l] += sum_m dxl[l]*xhat, g_tn_b[l] += sum_m dxl[l]; d emb = sum_5 dea + SiLU'(emb) * sum_10 deb. */
typedef struct {
    int M, B;
    const float* dxl;         /* [5,M,256] */
    const float* dcs;         /* [5,M,256] */
    const float* xhat;        /* [M,256] */
    const float* rstd;        /* [M] */
    const float* tn_w[5];
    float* g_tn_w[5];
    float* g_tn_b[5];
    float* dcond;             /* [M,256] */
    const float* dea;         /* [5,B,256] */
    const float* deb;         /* [10,B,256] */
    const float* emb;         /* [B,256] */
    float* demb;              /* [B,256] */
} SeemeGlueMid;
int seeme_glue_mid(const SeemeGlueMid* a, void* stream);

/* ------------------------------------------------------------------ stage-1 (VAE) training: row kernels
 * The hand-written forward-with-saves / backward of MldVae.encode / decode for train_vae_forward (mld.py:633-885; layers
 * cross_attention.py:41-147,281-367).  GEMMs run on seeme_grouped_gemm; call order in seeme_amd/vae_train.py. */
typedef struct {
    const float* sub;         /* [M,256] sublayer output, or one row per sequence when sub_seq_rows > 0 */
    const float* res;         /* [M,256] residual or NULL */
    const float* gamma; const float* beta;
    float* y; float* xhat; float* rstd;
    long M; int sub_seq_rows; float eps;
} SeemeVtLn;
/* y = LN(sub + res) * gamma + beta over the 256 features (biased variance); keeps xhat = (v - mean) * rstd and
 * rstd = 1 / sqrt(var + eps) for the backward.  sub_seq_rows > 0: row m reads sub[m / sub_seq_rows]. */
int seeme_vt_add_ln(const SeemeVtLn* a, void* stream);
typedef struct {
    const float* dy; const float* xhat; const float* rstd; const float* gamma;
    float* dpre;              /* [M,256] gradient w.r.t. (sub + res) */
    float* dgamma; float* dbeta;   /* accumulated (atomics) */
    long M; int accumulate;   /* 1: dpre += */
    const float* dy2;         /* optional second gradient of the same output (skip connection): dy + dy2 */
} SeemeVtLnBwd;
/* With d = dy (+ dy2) and g = d * gamma: dpre (+)= rstd * (g - mean(g) - xhat * mean(g * xhat)); dgamma += sum_m d * xhat and
 * dbeta += sum_m d ALWAYS accumulate (the caller zeroes them), whatever `accumulate` says for dpre. */
int seeme_vt_ln_bwd(const SeemeVtLnBwd* a, void* stream);
/* scores [B,S,S] = q k^T (unscaled) -> softmax(scale * s) over the keys [0, n_b), n_b = min(S, n_prefix + lengths[b]), exact zeros
 * elsewhere whatever the masked inputs hold (NaN included).  1 <= S <= 512; n_b >= 1 is the caller's contract (a sequence without
 * a valid key has no softmax: its rows would be 0/0). */
int seeme_vt_softmax_fwd(float* scores, const int32_t* lengths, int B, int S, int n_prefix, float scale, void* stream);
/* dp [rows,S] (gradient w.r.t. the probabilities) -> gradient w.r.t. the unscaled scores, in place. */
int seeme_vt_softmax_bwd(float* dp, const float* p, long rows, int S, float scale, void* stream);
/* exact GELU: dh == NULL: out = gelu(pre); else out = dh * gelu'(pre). */
int seeme_vt_gelu(const float* pre, const float* dh, float* out, long n, void* stream);
/* out[b,:] (+)= sum_s w[b,s] d[b,s,:]  (d [B,S,256]); w = wmask[b,s] ? scale : 0, or 1 when wmask is NULL. */
int seeme_vt_seq_sum(const float* d, float* out, int B, int S, int accumulate, const unsigned char* wmask, float scale, void* stream);
/* Inverted dropout with a given keep-mask (nn.Dropout / the attention-weight dropout of nn.MultiheadAttention in training,
 * cross_attention.py:264-273,324-337): out = x * scale (one float32 rounding) where the mask byte is non-zero, +0 elsewhere; scale =
 * 1 / (1 - p); in place allowed; x / out 16-byte aligned, mask 4-byte aligned. */
int seeme_vt_dropout(const float* x, const unsigned char* mask, float scale, float* out, long n, void* stream);
/* Decoder cross-attention to the single latent token under dropout (cross_attention.py:357-362):
 * out[b,s,:] = ((wmask[b,s] ? scale : 0) * cvn[b,:] + bo) * (m2[b,s,:] ? scale : 0). */
int seeme_vt_cross_rows(const float* cvn, const float* bo, const unsigned char* wmask, const unsigned char* m2, float scale,
                        int B, int S, float* out, void* stream);

/* ------------------------------------------------------------------ K hypotheses per sequence: errors and diversity
 * jts_pred [B*K,T,24,3] (row b*K + k = hypothesis k of sequence b), jts_ref [B,T,24,3], fp32 metres, 16-byte aligned; lengths [B].
 * per_hyp [3,B,K] = MPJPE, ROOT_ERROR, ACCL of EgoMetrics.per_sequence for hypothesis k against the reference of b (mm);
 * per_seq [2,B] = APD_JOINTS (EgoHMR form, test_egohmr.py:519-520: half the mean distance over unordered pairs) and STD_JOINTS
 * (unbiased standard deviation over K of every joint coordinate, :496), means over the valid frames (mm); both 0 for K = 1.
 * K <= 32; every length must be in 1..T (as per_sequence, the sums run over min(len, T) frames and are divided by len, so a length
 * outside that range gives a meaningless or non-finite row; it is never read out of bounds).  No atomics: bitwise reproducible.  The workspace holds the per-chunk partial sums. */
size_t seeme_hyp_metrics_workspace_bytes(int B, int K, int T);
int seeme_hyp_metrics(const float* jts_pred, const float* jts_ref, const int32_t* lengths, int B, int K, int T,
                      float* per_hyp, float* per_seq, void* ws, size_t ws_bytes, void* stream);

/* Pairwise distances of the K hypotheses of a sequence and their medoid (the label-free choice among the K draws).
 * jts_pred [B,K,T,24,3] as above, 16-byte aligned; lengths [B], nvalid = clamp(len, 0, T).  With a_k the prediction of hypothesis k
 * after the alignment of seeme_hyp_metrics (minus its own first-frame joint 15, then minus each frame's own joint 0):
 * dist[b,i,j] = 1000 x the mean over the nvalid frames and the 24 joints of |a_i - a_j| (mm).  The diagonal is exactly 0 and the
 * matrix exactly symmetric (every unordered pair is computed once and mirrored); sum_{i,j} dist[b] / (K (K-1)) / 2 is APD_JOINTS[b].
 * medoid[b] = argmin over i of sum_j dist[b,i,j], the sum taken in j order in fp32; the LOWEST index wins a tie (so K = 2 gives 0).
 * nvalid = 0 gives a zero matrix and medoid 0; K = 1 gives [[0]] and medoid 0.  K <= 32.  Frames past nvalid are never read.  No
 * atomics: bitwise reproducible.  The workspace (16-byte aligned) holds the per-chunk partial sums of the pairs. */
size_t seeme_hyp_pairdist_workspace_bytes(int B, int K, int T);   /* 0 for bad sizes */
int seeme_hyp_pairdist(const float* jts_pred, const int32_t* lengths, int B, int K, int T, float* dist, int32_t* medoid,
                       void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ interpersonal distance and mutual gaze (csrc/social_metrics.hip)
 * How the wearer stands to the interactee, for the reference body (what an evaluation is binned by) and for each of K hypotheses
 * (whether a hypothesis reproduces the interaction).  All inputs fp32, 16-byte aligned, in ONE coordinate frame per sequence: there is
 * no alignment of any kind, the relative placement of the two people is the thing measured.
 *   jts_pred [B,K,T,24,3] joints of the K hypotheses      quat_pred [B,K,T,4] their global orientation, (w,x,y,z)
 *   jts_ref  [B,T,24,3]   the wearer's reference joints   quat_ref  [B,T,4]   the reference's global orientation
 *   jts_int  [B,T,24,3]   the interactee's joints         quat_int  [B,T,4]   the interactee's global orientation
 *   lengths  [B] int32; n = clamp(len, 0, T) valid frames; every mean below runs over the frames t < n; n = 0 gives zeros.
 * Per frame, for a body x with orientation q:
 *   d(x) = |x[0] - int[0]|                                          pelvis-to-pelvis distance
 *   c(x) = min over the 24 x 24 joint pairs of |x[i] - int[j]|      closest approach
 *   g(q) = third column of the rotation matrix of q, q normalised as EgoMetrics.quat_to_rotmat does (q sqrt(2 / |q|^2)); a degenerate
 *          quaternion (|q|^2 < 1e-15) is the identity, g = (0,0,1)
 *   a(q) = min(atan2(|g(q) x g(q_int)|, g(q) . g(q_int)) 180/pi, 180), degrees in [0, 180].  This is the reference's arccos of the
 *          normalised dot product (mld/models/metrics/compute.py:31) in the form that stays accurate at 0 and 180 degrees, where the
 *          arccos loses half its digits.  The products of the cross product are rounded one by one, so parallel directions give
 *          exactly 0 and antiparallel ones exactly 180.
 * per_seq [3,B], from the reference body alone (they do not depend on any prediction):
 *   PERSON_DIST = 1000 mean d(ref) (mm), CLOSEST_DIST_REF = 1000 mean c(ref) (mm), GAZE_ANGLE_REF = mean a(q_ref) (degrees)
 * per_hyp [5,B,K]:
 *   PERSON_DIST_ERROR = 1000 mean |d(pred_k) - d(ref)|, CLOSEST_DIST = 1000 mean c(pred_k),
 *   CLOSEST_DIST_ERROR = 1000 mean |c(pred_k) - c(ref)|, GAZE_ANGLE = mean a(q_pred_k), GAZE_ANGLE_ERROR = mean |a(q_pred_k) - a(q_ref)|
 * (a hypothesis whose quaternions equal the reference's bit for bit has a GAZE_ANGLE_ERROR of exactly 0).
 * 1 <= K <= 32, 1 <= B <= 65535, T >= 1.  One workgroup per (sequence, chunk of SEEME_SOCIAL_FRAME_CHUNK frames) writes partial sums
 * to the workspace (4-byte aligned), a second launch adds them in chunk order.  Frames past n are never read.  No atomics, no
 * allocation, no synchronisation: bitwise reproducible, and a sequence's values do not depend on B or on the other sequences. */
#define SEEME_SOCIAL_FRAME_CHUNK 8
size_t seeme_social_metrics_workspace_bytes(int B, int K, int T);   /* 0 for bad sizes */
int seeme_social_metrics(const float* jts_pred, const float* jts_ref, const float* jts_int, const float* quat_pred,
                         const float* quat_ref, const float* quat_int, const int32_t* lengths, int B, int K, int T,
                         float* per_hyp, float* per_seq, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ a whole recording from overlapping windows (csrc/recording.hip)
 * A recording of n_frames frames is cut into W windows of T frames that start S = T - O frames apart, 0 <= O and 2*O <= T (no frame
 * lies in more than two windows): W = 1 for n_frames <= T, else ceil((n_frames - T) / S) + 1; window w starts at w*S and has
 * min(T, n_frames - w*S) valid frames; windows w and w+1 share the last O frames of w and the first O of w+1.  All windows are in ONE
 * coordinate frame.  K hypotheses per window, K <= 32.  fp32, no atomics: bitwise reproducible.
 *
 * Disagreement of neighbouring windows on their shared frames.  jts [W,K,T,24,3] (metres, 16-byte aligned):
 * cost[w,i,j] = 1000 x the mean over r = 0..O-1 and the 24 joints of |a - b| (mm), a = hypothesis i of window w at frame T-O+r,
 * b = hypothesis j of window w+1 at frame r.  No alignment of any kind: the global position is part of what must agree.  cost is
 * [W-1,K,K]; W = 1 or O = 0 writes nothing and returns success.  Frames outside the overlaps are never read.  The workspace (16-byte
 * aligned) holds the per-chunk partial sums. */
size_t seeme_overlap_cost_workspace_bytes(int W, int K, int T, int O);   /* 0 for bad sizes */
int seeme_overlap_cost(const float* jts, int W, int K, int T, int O, float* cost, void* ws, size_t ws_bytes, void* stream);

/* The path p_0 .. p_{W-1} that minimises sum_w unary[w,p_w] + sum_w cost[w,p_w,p_{w+1}], by dynamic programming.  cost [W-1,K,K],
 * unary [W,K] or NULL (no unary term).  With d_0[j] = unary[0,j] (0 without unary), d_{w+1}[j] = min_i (d_w[i] + cost[w,i,j]) +
 * unary[w+1,j], every sum in fp32 in this order; the LOWEST i wins a tie and is the back-pointer, and the lowest j of the smallest
 * d_{W-1} ends the path.  path [W] int32; seam[w] = cost[w,p_w,p_{w+1}] ([W-1]); total[0] = d_{W-1}[p_{W-1}], the path's sum.  W = 1
 * gives the argmin of unary (0 without it).  A set of candidates that holds a NaN has no minimum: index 0 and a NaN sum.  The
 * workspace (4-byte aligned) holds the back-pointers. */
size_t seeme_path_select_workspace_bytes(int W, int K);                  /* 0 for bad sizes */
int seeme_path_select(const float* cost, const float* unary, int W, int K, int32_t* path, float* seam, float* total,
                      void* ws, size_t ws_bytes, void* stream);

/* One motion out of the chosen hypothesis of every window.  feats [W,T,F] renormed features, out [n_frames,F]; W must be the window
 * plan of (n_frames, T, O).  Frame n lies in window w = min(n / S, W-1) at local frame t = n - w*S; for w >= 1 and t < O it is also
 * frame t + S of window w-1 and the two are blended with weight u = (t+1)/(O+1) for the LATER window, otherwise it is copied.
 * layout: SEEME_STITCH_ANGLE F = J x 3 axis-angle values; SEEME_STITCH_ANGLE_TRANSL the same with 3 translation values last
 * (TRAIN.ABLATION.PREDICT_TRANSL); SEEME_STITCH_ROT6D F = 24 x 6, read as seeme_geometry's SEEME_GEO_ROT6D_PROHMR reads it (a1 = x[0:3],
 * a2 = x[3:6], Gram-Schmidt) and written back as the first two columns of the blended rotation.  Each joint rotation: unit
 * quaternion (axis-angle v: (cos(|v|/2), sin(|v|/2) v/|v|); rot6d: of its rotation matrix) -> the later one negated when the dot
 * product of the two is negative -> slerp, or, when the dot product exceeds SEEME_STITCH_NLERP_DOT, the lerp (1-u) p + u q -> normalised
 * -> back to the feature's own parameterisation (axis-angle with an angle in [0, pi]).  Translation: a + u (b - a).  Frames past a
 * window's valid length are never read. */
enum { SEEME_STITCH_ANGLE = 0, SEEME_STITCH_ANGLE_TRANSL = 1, SEEME_STITCH_ROT6D = 2 };
#define SEEME_STITCH_NLERP_DOT 0.9995f
int seeme_stitch_windows(const float* feats, int W, int T, int O, int n_frames, int F, int layout, float* out, void* stream);

/* ------------------------------------------------------------------ one coherent track through sparse key frames (csrc/track.hip)
 * Lf key frames (the stored frames of a recording of L frames, idx [Lf] int32 on the device, strictly increasing inside 0..L-1: the
 * caller's contract) carry S candidate bodies each.  ONE candidate per key frame is chosen by seeme_path_select (W = Lf, K = S) with the
 * transition costs below, and the chosen bodies are filled to all L frames and filtered.  fp32, no atomics: bitwise reproducible.
 *
 * Transition costs of a random walk of every joint whose variance grows linearly over a gap.  jts [Lf,S,24,3] fp32 metres (16-byte
 * aligned): cost[l,i,j] = weight * (sum over the 24 joints, in joint order, of |jts[l,i,k] - jts[l+1,j,k]|^2) / (idx[l+1] - idx[l]),
 * cost [Lf-1,S,S].  weight = 1e6 / (2 step_mm^2) makes it the negative log-density (nats, without the constant) of a walk with a
 * standard deviation of step_mm per frame.  1 <= S <= 32, 1 <= Lf <= 65536; Lf = 1 writes nothing and succeeds.  One workgroup per l,
 * fixed summation order. */
int seeme_track_cost(const float* jts, const int32_t* idx, int Lf, int S, float weight, float* cost, void* stream);

/* Fill between the keys and a symmetric FIR.  pose [Lf,J,3] axis-angle at the key frames idx [Lf] (device), transl [Lf,3] or NULL;
 * taps_host [R+1] on the HOST, 0 <= R <= 32, taps[0] > 0, every tap finite and >= 0 (validated; they reach the kernel by value).
 * pose_out [L,J,3], transl_out [L,3] or NULL (with transl: both or neither).  1 <= J <= 32, 1 <= Lf <= L <= 2^20.
 * A unit is one joint rotation or the translation.  The quaternion of a key is the one seeme_stitch_windows forms from an axis-angle
 * vector v: (cos(|v|/2), sin(|v|/2) v/|v|).
 * fill(m) for a recording frame m: the first key for m <= idx[0]; the last key for m >= idx[Lf-1]; key a itself when m == idx[a];
 *   otherwise, with idx[a] < m < idx[a+1] and u = (m - idx[a]) / (idx[a+1] - idx[a]), exactly seeme_stitch_windows' blend of keys a
 *   and a+1 at u (the later key negated on a negative dot product, then the slerp, or the lerp above SEEME_STITCH_NLERP_DOT,
 *   normalised).  The translation: a + u (b - a).
 * out(n): over the window m = max(0, n-R) .. min(L-1, n+R), acc = sum_m taps[|m-n|] * s_m * fill(m) with s_m = -1 when
 *   dot(fill(m), fill(n)) < 0 and +1 otherwise, summed in increasing m; the rotation is acc / |acc| (acc . fill(n) >= taps[0] > 0: it
 *   never vanishes), written as axis-angle with an angle in [0, pi] as the stitch kernel writes it.  The translation is
 *   sum_m taps[|m-n|] * fill_t(m) / sum_m taps[|m-n|] over the same truncated window.
 * With R == 0 a frame that is a key is copied from the input bit for bit (no round trip through the quaternion); with R > 0 nothing is
 * copied.  One launch: a workgroup owns SEEME_TRACK_TILE output frames, finds the key interval of each of its TILE + 2R frames by
 * binary search, holds their fill in LDS and applies the taps from there.  The result depends neither on the tiling nor on what the
 * outputs held before. */
#define SEEME_TRACK_TILE 64
int seeme_track_filter(const float* pose, const float* transl, const int32_t* idx, int Lf, int L, int J,
                       const float* taps_host, int R, float* pose_out, float* transl_out, void* stream);

/* ------------------------------------------------------------------ the headset's own path (csrc/headset.hip)
 * A recording from a head-worn device carries the device's position in every frame: the only label-free evidence about where the
 * wearer went.  The head is SMPL joint SEEME_HEAD_JOINT.  fp32, no atomics, fixed summation order: bitwise reproducible.
 *
 * How far a hypothesis' head strays from the SHAPE of the device's path over its window.  jts [W,K,T,24,3] (metres, in the frame the
 * path is in), path [W,T,3] (row w: the device's positions at window w's frames, then anything), lengths [W] int32 on the device.
 * With n = min(max(lengths[w], 0), T), h_t = jts[w,k,t,15], r_t = h_t - path[w,t] and o = (1/n) sum_{t<n} r_t:
 *     cost[w,k] = 1000 x (1/n) sum_{t<n} |r_t - o|   (mm; 0 for n <= 1)
 * The mean offset o is removed per hypothesis, so a constant offset between head and device costs nothing.  Two passes in this order
 * (the mean, then the deviations from it); one wave per (w, k), a lane adds its frames t = lane, lane + 64, ... in increasing t and
 * the 64 partial sums are added by a butterfly (distances 32, 16, .. 1).  Frames t >= n and joints other than 15 are never read.
 * cost [W,K], usable as the unary term of seeme_path_select.  1 <= W <= 65536, 1 <= K <= 32, 1 <= T <= 2^20. */
#define SEEME_HEAD_JOINT 15
int seeme_head_path_cost(const float* jts, const float* path, const int32_t* lengths, int W, int K, int T, float* cost, void* stream);

/* The shift that puts the head of ONE motion onto the device's path, smoothed.  joints [L,24,3], path [L,3]; taps_host [R+1] on the
 * HOST, 0 <= R <= SEEME_HEAD_ANCHOR_RMAX, taps[0] > 0, every tap finite and >= 0 (validated; they reach the kernel by value:
 * seeme_amd/track.py gaussian_taps).  With r[n] = path[n] - joints[n,15]:
 *     shift[n]    = (sum_d taps[|d|] r[n+d]) / (sum_d taps[|d|])   over -R <= d <= R with 0 <= n+d < L, both sums in increasing d
 *     residual[n] = 1000 x |r[n] - shift[n]|                        (mm)
 * so the filter renormalises at the recording's two ends.  taps = {1} (R = 0) gives shift = r and residual = 0 exactly.  shift [L,3],
 * residual [L]; 1 <= L <= 2^20.  One workgroup per 256 output frames holds r of its 256 + 2R frames in LDS; the result depends
 * neither on the tiling nor on what the outputs held before. */
#define SEEME_HEAD_ANCHOR_RMAX 30
int seeme_head_anchor(const float* joints, const float* path, int L, const float* taps_host, int R, float* shift, float* residual,
                      void* stream);

/* How far a hypothesis' head TURNS against the device over its window, up to a constant mount rotation.  A head-worn device also
 * reports its orientation in every frame, and it is rigid with the head: seen from the head, its orientation does not change.
 * feats [W,K,T,F] renormed features in one of seeme_stitch_windows' layouts: SEEME_STITCH_ANGLE (F = J x 3) and
 * SEEME_STITCH_ANGLE_TRANSL (F = J x 3 + 3) with J >= 16 (EgoBody 72 / 75, GIMO 66 / 69), SEEME_STITCH_ROT6D (F = 144); another
 * layout / F pair is refused by name.  dev_quat [W,T,4]: unit quaternions (w,x,y,z), the device's orientation (device -> the frame
 * the features are in) at window w's frames, then anything; lengths [W] int32 on the device.  Per (w,k), with
 * n = min(max(lengths[w], 0), T):
 *     h_t  = the global rotation of joint SEEME_HEAD_JOINT: the quaternion product along the chain 0 -> 3 -> 6 -> 9 -> 12 -> 15, in
 *            that order; a joint's quaternion is formed exactly as seeme_stitch_windows forms it (axis-angle v: (cos(|v|/2),
 *            sin(|v|/2) v/|v|); rot6d: Gram-Schmidt, then of the rotation matrix, the largest of w, x, y, z first)
 *     d_t  = conj(h_t) (x) dev_quat[w,t]           the device seen from the head: constant in t for a correct hypothesis, whatever
 *                                                  the camera's axis convention
 *     s_t  = -1 when d_t . d_0 < 0, otherwise +1
 *     m    = sum_{t<n} s_t d_t, normalised         (m . d_0 >= 1: it never vanishes)
 *     a_t  = 2 atan2(|vec(conj(m) (x) d_t)|, |scalar(conj(m) (x) d_t)|) x 180/pi
 *     cost[w,k] = (1/n) sum_{t<n} a_t              (degrees; 0 for n <= 1)
 * angle [W,K,T] (or NULL: not written) holds a_t, degrees per frame, and 0 for t >= n (all of it for n <= 1).  The constant m is
 * removed per hypothesis, so a constant rotation between head and device (how the device is mounted, which way its axes point)
 * costs nothing -- and cannot be observed.  Two passes in this order (m, then the angles against it); one wave per (w, k), a lane
 * adds its frames t = lane, lane + 64, ... in increasing t, the 64 partial sums are added by the butterfly of seeme_head_path_cost
 * and d_0 is broadcast from lane 0.  Only the six chain joints of the frames t < n are read; in the angle layouts the translation
 * columns never.  cost [W,K], usable as a unary term of seeme_path_select.  1 <= W <= 65536, 1 <= K <= 32, 1 <= T <= 2^20.
 * Against a float64 evaluation of this definition on the same fp32 inputs (chain rotations of about 0.4 rad per joint, 10 degrees
 * of noise, T up to 196; 26 324 frames) the kernel on the MI355X is within 2.9e-6 relative per frame at angles >= 5 degrees and
 * within 1.8e-5 degrees below that, and cost is within 1.5e-6 relative. */
int seeme_head_rot_cost(const float* feats, int layout, int F, const float* dev_quat, const int32_t* lengths, int W, int K, int T,
                        float* cost, float* angle /* or NULL */, void* stream);

/* ------------------------------------------------------------------ the body against the scene, per candidate frame (csrc/scene_depth.hip)
 * How deep a hypothesis reaches into the scene's points, from the joints alone: the body is NB capsules (one per bone), the scene one
 * cloud shared by every window.  jts [W,K,T,J,3] (metres), lengths [W] int32 on the device, points [N,3] in the frame jts is in;
 * segs_host [NB,2] int32 (joint indices in 0..J-1; equal ends: a sphere) and radius_host [NB] (finite, >= 0) on the HOST, validated
 * there, by value in the kernel arguments; 1 <= NB <= SEEME_SCENE_DEPTH_NBMAX.  With n = min(max(lengths[w], 0), T), for a frame
 * f = (w,k,t), t < n, a point p and a segment b:
 *     a = jts[f,segs[b,0]], c = jts[f,segs[b,1]], e = c - a, q = p - a, ee = e.e
 *     s = ee > 0 ? clamp((q.e) / ee, 0, 1) : 0,  v = q - s e,  dist = sqrt(v.v)
 *     depth[w,k,t] = 1000 x max(0, max over p < N, b < NB of (radius[b] - dist))   (mm; 0 for t >= n)
 *     cost[w,k]    = (1/n) sum_{t<n} depth[w,k,t]                                  (mm; 0 for n = 0)
 *     hits[w,k]    = the number of frames t < n with depth > 0                     (int32)
 * A pair whose value is NaN contributes nothing.  Frames t >= n and joints that no segment names are never read.  The kernel
 * multiplies by 1/ee where the definition divides.  max is exact and free of order and ONE expression evaluates a (frame, point,
 * segment) triple, so depth is bit for bit independent of the order of the points, of N under appended points out of reach, of W, K
 * and T as a layout of the same frames, and of the culling, which skips only triples whose computed value is <= 0.  cost adds depth
 * in fp32, one wave per (w,k): a lane adds t = lane, lane + 64, ... in increasing t, the 64 partial sums by a butterfly (distances
 * 32 .. 1), as seeme_head_path_cost does.  cost is usable as a unary term of seeme_path_select.
 * 1 <= W <= 65536, 1 <= K <= 32, 1 <= T <= 2^20, 1 <= N <= 2^24, 1 <= J <= 32, and W x K x ceil(T / SEEME_SCENE_DEPTH_CHUNK) < 2^24
 * (the launch's workgroups).  depth [W,K,T], cost [W,K], hits [W,K] int32.  No workspace, no allocation, no synchronisation. */
#define SEEME_SCENE_DEPTH_NBMAX 32
#define SEEME_SCENE_DEPTH_CHUNK 32
int seeme_scene_depth(const float* jts, const int32_t* lengths, const float* points, int W, int K, int T, int J, int N,
                      const int32_t* segs_host, const float* radius_host, int NB, float* depth, float* cost, int32_t* hits,
                      void* stream);

/* ------------------------------------------------------------------ scene views of a moving camera (csrc/scene_views.hip)
 * The view-dependent selection of a scene mesh's vertices that the EgoBody scene tables are made with (EgoHMR
 * preprocess_scene_s1.py:91-114: into the camera frame, keep z > 0, every k-th survivor, the first P), for W views in one call.
 * verts [N,3] fp32; M [W,4,4] fp32 row-major, world -> view, rows 0..2 are read; cloud [W,P,3] fp32 in the view's frame; index
 * [W,P] int32, the source vertex of every output row; count [W] int32, the number of survivors.
 * For vertex i = (x, y, z) and view w, coordinate c of the moved vertex is
 *     p'_c = fmaf(M[c][2], z, fmaf(M[c][1], y, fmaf(M[c][0], x, M[c][3])))
 * and the vertex survives iff p'_z > 0 (a NaN compares false); the classification and the written coordinate are this one
 * expression.  Survivors keep vertex order; r is a survivor's rank among its view's survivors.
 *   count >= P:      k = count / P (integer division, >= 1); output row j < P holds the survivor of rank j*k.
 *   0 < count < P:   row j holds the survivor of rank j mod count (the table is filled cyclically; count tells the caller).
 *   count = 0:       the rows are zero and index is -1; no error.
 * 1 <= N <= 2^24, 1 <= W <= 4096, 1 <= P <= 2^20.  A workgroup owns a tile of SEEME_SCENE_VIEW_TILE consecutive vertices and walks
 * SEEME_SCENE_VIEW_WINDOWS_PER_PASS views over it.  No atomics; a row's owner is found from ranks alone, so the output is bitwise
 * reproducible and does not depend on W, on the tiling or on what the workspace held.  The workspace (4-byte aligned) holds the
 * survivor count of every (view, tile), then its exclusive prefix. */
#define SEEME_SCENE_VIEW_TILE 1024
#define SEEME_SCENE_VIEW_WINDOWS_PER_PASS 16
size_t seeme_scene_views_workspace_bytes(int N, int W, int P);           /* 0 for bad sizes */
int seeme_scene_views(const float* verts, const float* M, int N, int W, int P, float* cloud, int32_t* index, int32_t* count,
                      void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ interactee patches from raw frames (csrc/crop_patches.hip)
 * The S x S patch that the reference's dataset cuts around the interactee with OpenCV (dataset.py:1664-1690: warpAffine,
 * INTER_LINEAR, constant zero border, no flip, no rotation, no rescaling), for n patches in one launch.  frames [n_frames,H,W,3]
 * uint8 RGB; frame_of_patch [n] int32 (several patches may name one frame, in any order); boxes [n,3] fp32 = cx, cy, b: the centre
 * the reference hands to its warp and the side of the box in frame pixels (seeme_amd/crops.py patch_box); out [n,S,S,3] uint8.
 * An integer definition, so the kernel and its plain-torch twin (crops.py crop_patches_torch) agree bit for bit.  In double, every
 * product and sum rounded on its own: m = b / S, ox = cx - (S/2) m, oy = cy - (S/2) m; rne = round half to even; 64-bit integers,
 * >> the arithmetic (flooring) shift:
 *   X = (rne(ox 1024) + 16 + rne(m u 1024)) >> 5          (the two axes are NOT symmetric)
 *   Y = (rne((m v + oy) 1024) + 16) >> 5
 *   sx = X >> 5, ax = X & 31, sy = Y >> 5, ay = Y & 31
 *   out[v,u,c] = ((32-ay)(32-ax) I[sy,sx,c] + (32-ay) ax I[sy,sx+1,c] + ay (32-ax) I[sy+1,sx,c] + ay ax I[sy+1,sx+1,c] + 512) >> 10
 * A tap outside 0 <= row < H, 0 <= col < W contributes 0 and is never read.  1 <= H, W <= SEEME_CROP_FRAME_MAX, 1 <= S <=
 * SEEME_CROP_PATCH_MAX, n >= 1 (not capped by the grid), n_frames >= 1; a frame's byte offset is computed in size_t.  The caller
 * checks |cx|, |cy| <= SEEME_CROP_COORD_MAX, 0 < b <= SEEME_CROP_COORD_MAX, all finite, and 0 <= frame_of_patch < n_frames (the
 * entry point cannot look into device memory without a synchronisation); inside these nothing overflows 64 bits.  The kernel
 * guards itself as well: a patch whose box or frame index is outside them is all zeros, never an out-of-range read.  No
 * allocation, no synchronisation, no atomics, no workspace; frame_of_patch and boxes 4-byte aligned, out any alignment. */
#define SEEME_CROP_FRAME_MAX 16384
#define SEEME_CROP_PATCH_MAX 1024
#define SEEME_CROP_COORD_MAX 1048576            /* 2^20 */
int seeme_crop_patches(const uint8_t* frames, int n_frames, int H, int W, const int32_t* frame_of_patch, const float* boxes,
                       int n, int S, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ per-frame mesh metrics (csrc/mesh_metrics.hip)
 * Frame-level primitives of the EgoHMR tables (test_egohmr.py:463-492, 540-549): one float per frame, fp32 metres in and out, a
 * frame whose map entry is negative is skipped and gets 0; the caller averages over the valid frames of a sequence and chunks the
 * frames.  Map entries must be below the number of reference frames / scenes the caller holds (scene entries >= S are skipped).
 * No atomics, fixed-order sums: bitwise reproducible, and a frame's value does not depend on the other frames of the launch.
 *
 * seeme_pa_mpjpe_frames: out[f] = mean over the 24 joints of |s R x + t - y|, x = j_pred[f], y = j_ref[ref_of_frame[f]], (s, R, t)
 * the similarity transform of EgoHMR utils/pose_utils.py:11-59 (R a proper rotation: the reflection correction included).
 * seeme_mesh_v2v_frames: out[f] = mean over the V vertices of |(v - pel_pred[f]) - (v_ref - pel_ref[r])|, r = ref_of_frame[f]
 * (test_egohmr.py:485); v_pred / v_ref 16-byte aligned.
 * seeme_scene_min_dist2: out_d2[f] = min over the V x P pairs of the SQUARED distance between verts[f] and scene[scene_of_frame[f]]:
 * an fp32 MFMA pass in the expansion form picks the scene points that can hold the minimum (error bound in the source), those are
 * re-evaluated in direct form; the result is the minimum over all pairs of the direct-form value.  V <= 10112 (the frame's
 * operands live in LDS); workspace 16-byte aligned. */
int seeme_pa_mpjpe_frames(const float* j_pred, const float* j_ref, const int32_t* ref_of_frame, int F, float* out, void* stream);
int seeme_mesh_v2v_frames(const float* v_pred, const float* pel_pred, const float* v_ref, const float* pel_ref,
                          const int32_t* ref_of_frame, int F, int V, float* out, void* stream);
size_t seeme_scene_min_dist2_workspace_bytes(int F, int V, int S, int P);   /* 0 for bad sizes */
int seeme_scene_min_dist2(const float* verts, const float* scene, const int32_t* scene_of_frame, int F, int V, int S, int P,
                          float* out_d2, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ point-in-mesh test (csrc/collision.hip)
 * The collision ratio of the EgoHMR tables (egohmr.py:511-538) without the learned occupancy network: a point is inside the closed,
 * consistently oriented mesh (verts [F,V,3] of frame f, faces [NF,3] shared by all frames) iff |w| >= 0.5, w the winding number:
 * w(p) = sum over the faces of 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 4 pi, a, b, c the corners minus p.
 * A face with two equal indices or an index outside 0..V-1 contributes 0 and is never read (the caller validates the table once:
 * the entry points cannot look into device memory without a synchronisation); a corner vector of length 0 makes the face
 * contribute 0, never NaN.  V <= 10112 (the frame's vertices live in LDS).  A frame whose map entry is negative (or >= S) is skipped.
 * One lane sums a point's faces in table order: w and the count do not depend on F, on the other frames or on any chunking, bit
 * for bit.  No allocation, no synchronisation, no atomics.
 *
 * seeme_mesh_winding: out_w[f,p] = w of points[points_of_frame[f]][p] around frame f, every point, no prefilter; zeros for a skipped
 * frame.
 * seeme_scene_inside_count: out_count[f] = number of the P points of scene[scene_of_frame[f]] that are inside frame f; 0 for a
 * skipped frame.  Points outside the closed bounding box of the frame's vertices (w = 0) are dropped on the device first and only
 * the survivors are evaluated; all P may survive, there is no candidate cap.  Workspace 16-byte aligned: the per-slice counts. */
size_t seeme_scene_inside_count_workspace_bytes(int F, int V, int S, int P);   /* 0 for bad sizes */
int seeme_scene_inside_count(const float* verts, const int32_t* faces, int NF, const float* scene, const int32_t* scene_of_frame,
                             int F, int V, int S, int P, int32_t* out_count, void* ws, size_t ws_bytes, void* stream);
int seeme_mesh_winding(const float* verts, const int32_t* faces, int NF, const float* points, const int32_t* points_of_frame,
                       int F, int V, int S, int P, float* out_w, void* stream);

/* ------------------------------------------------------------------ ResNet-50 image backbone (csrc/resnet.hip)
 * EgoHMR.models.resnet.ResNet(Bottleneck, [3,4,6,3]) without fc, frozen and in eval mode: proscene.encode_image
 * (prohmr_scene.py:99-100).  Every BatchNorm is folded on the host (float64) into its convolution:
 * w' = w * g / sqrt(var + 1e-5), bias = b - mean * g / sqrt(var + 1e-5).  Activations are NHWC; a convolution is an implicit GEMM
 * (M = B Ho Wo, N = cout, K = k k cin), epilogue + bias, + residual, ReLU, store.
 * Packed weight of one convolution, element size s (4: fp32, 2: bf16), E = 16 / s elements per 16-byte chunk:
 *   Wk[cout][K]: K = (kh, kw, cin) with cin fastest; the stem's cin 3 is zero padded to E (one chunk per tap) and its K to 56 chunks;
 *   Wp[cout/16][K/(4E)][lane 64][E], lane = 16 kq + r:  Wp[t][g][16 kq + r][e] = Wk[row(t, r)][(4 g + kq) E + e],
 *   row(t, r) = 64 (t/4) + 16 (r/4) + 4 (t%4) + r%4   (a lane of the kernel then owns 16 consecutive output channels). */
enum { SEEME_RESNET_FP32 = 0, SEEME_RESNET_BF16 = 1 };
enum { SEEME_IMG_F32_NCHW = 0,      /* float32 [B,3,224,224], already normalised (the reference's batch slot) */
       SEEME_IMG_U8_NHWC = 1 };     /* uint8 [B,224,224,3] RGB; normalised in the stem's loader: (x - 255 mean_c) / (255 std_c) */
#define SEEME_RESNET50_NCONV 53
typedef struct {
    const float* weight;            /* packed fp32 fragments (NULL in a bf16 table) */
    const uint16_t* weight_bf16;    /* packed bf16 fragments (NULL in an fp32 table) */
    const float* bias;              /* [cout] fp32, the folded BatchNorm shift */
    int cin, cout, k, stride;       /* padding is k/2 */
} SeemeConv;
typedef struct {
    int precision;                  /* SEEME_RESNET_FP32: every tensor fp32, v_mfma_f32_16x16x4_f32 (parity path);
                                     * SEEME_RESNET_BF16: bf16 weights and activations, fp32 accumulation and epilogue */
    SeemeConv conv[SEEME_RESNET50_NCONV];   /* conv1; then per bottleneck conv1, conv2, conv3 and, in a layer's first one, downsample.0 */
    void* tap[5];                   /* bring-up, normally NULL: device copies of the NHWC activations after the max-pool and after
                                     * layer1..4 ([B,56,56,64], [B,56,56,256], [B,28,28,512], [B,14,14,1024], [B,7,7,2048]) */
} SeemeResnet50;
size_t seeme_resnet50_workspace_bytes(int B, int precision);      /* 0 for a bad B (1..1024) or precision */
/* images (image_format above) -> out [B,2048] fp32 = mean over the 7x7 map of layer4.  No allocation, no synchronisation, no
 * atomics; everything is enqueued on `stream` (capturable); workspace 256-byte aligned. */
int seeme_resnet50_encode(const SeemeResnet50* w, const void* images, int image_format, int B, float* out, void* ws,
                          size_t ws_bytes, void* stream);
/* The pieces of the network one by one (tests, bring-up); x / residual / y NHWC in the precision's element type, 16-byte aligned.
 * seeme_resnet_conv: cin 3 (the stem: x is the output of seeme_resnet_stem_pack) or a power of two >= 16 bytes, cout % 64 == 0. */
int seeme_resnet_conv(const SeemeConv* c, int precision, const void* x, int B, int H, int W, const void* residual, int relu,
                      void* y, void* stream);
int seeme_resnet_stem_pack(const void* images, int image_format, int B, int H, int W, int precision, void* y, void* stream);
int seeme_resnet_maxpool(int precision, const void* x, int B, int H, int W, int C, void* y, void* stream);

/* ------------------------------------------------------------------ mesh and point-cloud rasteriser (csrc/render.hip)
 * F frames of NF triangles over per-frame vertices, and P points shared by the frames, seen through a pinhole camera: per pixel the
 * id of the nearest primitive and its inverse depth, then a flat-shaded RGB image.  Everything after the vertex stage is integer
 * arithmetic, so the kernels, the plain-torch twin (seeme_amd/render.py render_torch) and tests/render_reference.py agree bit for
 * bit on ids, inv_depth and dropped.
 *
 * Vertex stage, per frame f and vertex (x, y, z), fp32 inputs widened to double, every product, sum and quotient rounded on its own
 * (no contraction).  M = cams[FC == 1 ? 0 : f], row-major world -> camera, rows 0..2 are read, left to right:
 *     xc = ((M00 x + M01 y) + M02 z) + M03        yc, zc likewise from rows 1 and 2
 *     X = rint(((fx xc) / zc + cx) 16)            Y = rint(((fy yc) / zc + cy) 16)          (rint: round half to even)
 *     Qv = rint((znear / zc) 2^22)                the inverse depth: affine in screen space, so interpolating it is perspective-correct
 * The vertex is valid iff zc is finite, zc >= znear, and X, Y are finite with |X|, |Y| <= SEEME_RENDER_COORD_MAX; then 0 <= Qv <=
 * SEEME_RENDER_Q.  X, Y are in 1/SEEME_RENDER_SUB pixel; pixel (row i, col j) is sampled at (16 j, 16 i): pixel centres sit at
 * integer coordinates (the OpenCV convention).
 *
 * Faces.  A face with an invalid corner is dropped whole and counted in dropped[f] (no near-plane clipping).  For the snapped
 * corners A, B, C: area2 = (Bx-Ax)(Cy-Ay) - (By-Ay)(Cx-Ax); 0 draws nothing; negative: B and C (and their Q) are swapped, so both
 * windings draw the same.  With e(U,V,P) = (Vx-Ux)(Py-Uy) - (Vy-Uy)(Px-Ux): w0 = e(B,C,P), w1 = e(C,A,P), w2 = e(A,B,P).  The pixel
 * is covered iff for every k: w_k > 0, or w_k == 0 and the edge's (dx, dy) = V - U has dy > 0 or (dy == 0 and dx < 0) -- an edge
 * shared by two triangles gives its pixels to exactly one of them.  The inverse depth at the pixel, in int64:
 *     q = floor((w0 Q_A + w1 Q_B + w2 Q_C) / area2)
 * Why 64 bits hold: |X|, |Y| <= 2^18 and a pixel's coordinates lie in 0..16 * 4095 < 2^16, so the difference of two corners is at
 * most 2^19 in magnitude and that of a pixel and a corner below 2^19; a product of two such is at most 2^38, so |area2|, |w_k| <=
 * 2^39.  q is evaluated on covered pixels only; there w_k >= 0 and w0 + w1 + w2 = area2, so 0 <= w_k <= area2, every product
 * w_k Q_k <= 2^39 2^22 = 2^61, and the numerator, a convex combination of the Q times area2, as well: |products| <= 2^61 < 2^63,
 * no partial sum exceeds the total, and 0 <= q <= 2^22.
 *
 * Points use the same vertex stage; the pixel is j = (X + 8) >> 4, i = (Y + 8) >> 4 (arithmetic shifts), a point_size square spans
 * the offsets -((s-1)/2) .. s/2 on both axes, clipped to the image; q = Qv, id = NF + p.  An invalid point draws nothing and is not
 * counted.
 *
 * Visibility.  key = (q << 32) | (0xFFFFFFFF - id), unsigned 64-bit; a pixel holds the MAXIMUM key over everything that covers it:
 * nearer wins, then the lower id (a face beats a point at equal depth).  Key 0 is the empty pixel (id <= 2^31 - 2 keeps a real key
 * above it).  A maximum does not depend on the order of arrival: the result is bitwise reproducible.
 * Outputs: ids [F,H,W] int32 (-1 empty), inv_depth [F,H,W] int32 (0 empty; depth in metres = znear 2^22 / q), dropped [F] int32.
 *
 * Shading (a separate entry point) writes rgb [F,H,W,3] uint8 from ids: an empty pixel gets bg, a point pixel point_rgb[id - NF], a
 * face pixel floor(base (0.3 + 0.7 |n_z| / |n|) + 0.5) per channel, n = (B-A) x (C-A) from the un-snapped camera-space corners
 * (|n| = 0: the ratio counts as 0), base = palette[mesh_of_face[id]].  The twin evaluates this in float64, the kernel in fp32: a
 * channel can differ by one where the value sits on a rounding boundary.
 *
 * 1 <= F <= 65535, FC = 1 or F, 1 <= H, W <= SEEME_RENDER_SIZE_MAX, 0 <= NV <= 2^24, NF, P >= 0 with NF + P <= 2^31 - 2 (NF > 0 needs
 * NV > 0), 1 <= point_size <= SEEME_RENDER_POINT_MAX, fx, fy, cx, cy finite, znear finite and > 0.  The caller validates the face table
 * (indices in 0..NV-1) and mesh_of_face (0..n_mesh-1) once: the entry points cannot look into device memory without a synchronisation.
 * The kernels guard themselves as well: a face with an index outside 0..NV-1 draws nothing, is not counted and is never read; a
 * mesh_of_face entry outside 0..n_mesh-1 shades as bg.  Plan: project every (frame, vertex) once into the workspace,
 * one lane per (frame, face) walks the face's clamped bounding box and issues a 64-bit vector atomic max into the workspace's key
 * image (a box above 256 pixels is walked by the whole wave), points likewise, and a resolve pass unpacks the keys.  No allocation,
 * no synchronisation; workspace 16-byte aligned: keys [F,H,W] uint64, then the projected vertices [F,NV] int32 x 4. */
#define SEEME_RENDER_SUB 16
#define SEEME_RENDER_COORD_MAX 262144           /* 2^18 sub-pixel units */
#define SEEME_RENDER_Q 4194304                  /* 2^22 */
#define SEEME_RENDER_SIZE_MAX 4096
#define SEEME_RENDER_POINT_MAX 8
typedef struct {
    const float* verts;             /* [F,NV,3] fp32, world frame */
    const int32_t* faces;           /* [NF,3] vertex indices, shared by the frames */
    const float* points;            /* [P,3] fp32, world frame, shared by the frames (NULL with P = 0) */
    const float* cams;              /* [FC,4,4] fp32 row-major world -> camera */
    int F, NV, NF, P, FC, H, W, point_size;
    float fx, fy, cx, cy, znear;
} SeemeRenderScene;
size_t seeme_render_workspace_bytes(int F, int NV, int H, int W);     /* 0 for bad sizes */
int seeme_render(const SeemeRenderScene* s, int32_t* ids, int32_t* inv_depth, int32_t* dropped, void* ws, size_t ws_bytes,
                 void* stream);
/* bg = r | g << 8 | b << 16; palette [n_mesh,3] and point_rgb [P,3] uint8 (point_rgb NULL with P = 0; mesh_of_face and palette NULL
 * with NF = 0); ids as written by the render entry point for the same scene. */
int seeme_render_shade(const SeemeRenderScene* s, const int32_t* ids, const int32_t* mesh_of_face, const uint8_t* palette,
                       int n_mesh, const uint8_t* point_rgb, uint32_t bg, uint8_t* rgb, void* stream);

/* ------------------------------------------------------------------ ProHMR-scene pose head (csrc/flow_head.hip)
 * The sampling direction of SMPLFlow (EgoHMR/models/prohmr/smpl_flow.py): nflows ConditionalGlow(144, 1024, 4, 2, context 2566) =
 * four layers of ActNorm -> LULinear -> AdditiveCoupling, inverted (layers 3 down to 0; inside a layer coupling^-1, LU^-1,
 * ActNorm^-1), plus FCHead for betas and the weak-perspective camera, eval mode, fp32 throughout.
 *
 * Inputs: ctx [L,2566] = [cam_cx/f, cam_cy/f, box_cx/f, box_cy/f, box_size/f, f/1500, image 2048, scene 512] per frame, z [L,S,144]
 * the base-distribution draws (z = 0 is the mode).  Row (l, s) uses ctx[l].  With x = z[l, s], per layer k = 3..0 whose identity
 * features are the indices 2j + p_k (p_k = bit k of id_parity; j = 0..71) and whose transform features are the others:
 *     h  = id_w[k] x[identity] + (ctx_w[k] ctx[l] + ctx_b[k])                               initial_layer, split by columns
 *     for the two blocks b:  h += lin_w[k][2b+1] relu(bn(lin_w[k][2b] relu(bn(h)))) + res_b[k][b]
 *                            bn(v) = v * bn_s + bn_o, the eval-mode BatchNorm; the first Linear's bias is folded into the second
 *                            BatchNorm's offset
 *     x[transform] -= fin_w[k] h + fin_b[k]                                                 additive coupling, inverted
 *     x = (lu_w[k] x) * act_s[k] + act_o[k]                                                 lu_w = inv(L U), a dense 144 x 144 matrix;
 *                                                                                           act_s = exp(-log_scale),
 *                                                                                           act_o = -(lu_w bias + shift) act_s
 * Outputs: pose6d [L,S,144] = x; rotmat [L,S,24,3,3]: per joint a1 = x[6j..6j+2], a2 = x[6j+3..6j+5], b1 = a1 / max(|a1|, 1e-12),
 * b2 likewise from a2 - (b1.a2) b1, columns (b1, b2, b1 x b2) (rot6d_to_rotmat, 'prohmr' order); log_prob [L,S] =
 * -|z|^2 / 2 + log_const, log_const = sum over layers of (sum log_scale + sum log diag U) - 72 log 2 pi (the coupling is additive, so
 * log|det| depends on neither z nor ctx); betas [L,10], cam [L,3] = fc_w relu(ctx_w[4] ctx[l] + ctx_b[4]) + fc_b with init_betas /
 * init_cam folded into fc_b.
 *
 * Every matrix is row-major [out, in] fp32, 16-byte aligned.  ctx_w stacks the context columns of the four initial layers and
 * fc_head.layers.0: [5 * 1024, SEEME_FLOW_CTX_PAD], columns 2566.. zero; id_w [4][1024][80], columns 72.. zero.
 * 1 <= S <= SEEME_FLOW_S_MAX, L >= 1, L * S <= SEEME_FLOW_ROWS_MAX.  A row's result does not depend on the rows it shares a
 * workgroup with.  Three launches on `stream`, no allocation, no synchronisation; workspace 16-byte aligned, [L, 5120] fp32. */
#define SEEME_FLOW_DIM 144
#define SEEME_FLOW_HIDDEN 1024
#define SEEME_FLOW_LAYERS 4
#define SEEME_FLOW_CTX 2566
#define SEEME_FLOW_CTX_PAD 2576
#define SEEME_FLOW_CTX_COLS 5120
#define SEEME_FLOW_S_MAX 32
#define SEEME_FLOW_ROWS_MAX 1048576
typedef struct {
    const float* ctx_w;             /* [5120, 2576] */
    const float* ctx_b;             /* [5120] */
    const float* id_w;              /* [4][1024][80] */
    const float* lin_w;             /* [4][4][1024][1024]: block 0 Linear 0, 1, block 1 Linear 0, 1 */
    const float* bn_s;              /* [4][4][1024] the BatchNorm in front of each of them, as scale ... */
    const float* bn_o;              /* [4][4][1024] ... and offset */
    const float* res_b;             /* [4][2][1024] bias of each block's second Linear */
    const float* fin_w;             /* [4][72][1024] */
    const float* fin_b;             /* [4][72] */
    const float* lu_w;              /* [4][144][144] */
    const float* act_s;             /* [4][144] */
    const float* act_o;             /* [4][144] */
    const float* fc_w;              /* [13][1024] */
    const float* fc_b;              /* [13] */
    int id_parity;                  /* bit k: layer k's identity features are the odd indices */
    float log_const;
} SeemeFlowHead;
size_t seeme_flow_head_workspace_bytes(int L, int S);                  /* 0 for bad sizes */
int seeme_flow_head(const SeemeFlowHead* w, const float* ctx, const float* z, int L, int S, float* pose6d, float* rotmat, float* betas,
                    float* cam, float* log_prob, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEEME_HIP_H */
