"""Plain numpy twins of the training-step entry points of include/seeme_hip.h, one per entry point, written from the header's
contract (not from the kernels), and the error bounds the direct kernel tests hold the HIP kernels to.

Every twin computes in ``dtype`` (float64 by default).  Run with ``dtype=np.float32`` the same lines are "the same formula in
float32 numpy": tests/test_gpu_train_kernels.py measures that against the float64 result to size a row kernel's tolerance, so
the measured formula and the reference cannot drift apart.  tests/test_train_kernels_cpu.py pins the twins against torch
float64 autograd / functional ops.

Where fp32 input formation is part of an operation's definition the twin forms that input in float32 whatever ``dtype`` is:
glue_rows multiplies float32(t) by float32(freq[j]) in float32 before sin / cos, and reads alphas_cumprod as the float32 it is.

Error model (u = 2^-24; a sum of L fp32 terms in any order has |err| <= (L + c) u sum|terms|):
  * sums (GEMMs, column sums, gather-reduces): per element |got - ref| <= (L + 16) u mag + 4 u |ref|, ``mag`` the sum of the
    absolute values of the terms (for a GEMM (|A'| |B'|)_ij with A', B' the float64 prologue outputs), L the reduced length
    (+ 1 for an accumulating output).  The 16 covers the few-ulp expf / division error of SiLU, SiLU' and the epilogue terms.
    Nothing in it depends on the order of the additions, so atomically accumulated outputs use it unchanged.
  * row kernels: per element |got - ref| <= 4 E + 4 u |ref|, E the largest float32-numpy-vs-float64 error among the elements
    of the same row of the same output (of the whole output where it has no rows: rstd vectors, the element-wise GELU).  The
    group maximum and not the element's own error, because a single element's float32 error is zero by luck often enough;
    4x for a different reduction order and FMA contraction.
"""
import math

import numpy as np

U = 2.0 ** -24
_erf = np.vectorize(math.erf, otypes=[np.float64])


def _a(x, dtype=np.float64):
    return np.asarray(x, dtype=dtype)


# ----------------------------------------------------------------------------- bounds
def sum_bound(L, mag, ref):
    return (L + 16) * U * np.asarray(mag, np.float64) + 4 * U * np.abs(np.asarray(ref, np.float64))


def row_bound(f32, ref, axis=-1):
    """4 E + 4 u |ref| with E the row maximum (axis=None: the whole tensor) of |float32 formula - float64 twin|."""
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(f32, np.float64) - ref)
    E = err.max() if axis is None or ref.ndim == 0 else err.max(axis=axis, keepdims=True)
    return 4 * E + 4 * U * np.abs(ref)


# ----------------------------------------------------------------------------- scalar functions
def erf(x, dtype=np.float64):
    if dtype == np.float32:          # numpy has no erf: torch's float32 erff
        import torch
        return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()
    return _erf(np.asarray(x, np.float64))


def silu(x, dtype=np.float64):
    x = _a(x, dtype)
    return x / (dtype(1) + np.exp(-x))


def dsilu(x, dtype=np.float64):
    x = _a(x, dtype)
    s = dtype(1) / (dtype(1) + np.exp(-x))
    return s * (dtype(1) + x * (dtype(1) - s))


def gelu(x, dtype=np.float64):
    """exact GELU 0.5 x (1 + erf(x / sqrt 2))"""
    x = _a(x, dtype)
    return dtype(0.5) * x * (dtype(1) + erf(x * dtype(math.sqrt(0.5)), dtype))


def dgelu(x, dtype=np.float64):
    """gelu'(x) = Phi(x) + x phi(x)"""
    x = _a(x, dtype)
    cdf = dtype(0.5) * (dtype(1) + erf(x * dtype(math.sqrt(0.5)), dtype))
    pdf = dtype(1.0 / math.sqrt(2.0 * math.pi)) * np.exp(dtype(-0.5) * x * x)
    return cdf + x * pdf


def vt_gelu(pre, dh=None, dtype=np.float64):
    """seeme_vt_gelu: dh None: gelu(pre); else dh * gelu'(pre)."""
    return gelu(pre, dtype) if dh is None else _a(dh, dtype) * dgelu(pre, dtype)


# ----------------------------------------------------------------------------- grouped GEMM
def gg_prologue(v, mode, p0=None, p1=None):
    """0 none, 1 SiLU, 2 ReLU, 3 affine v * p0 + p1 (p0 / p1 already broadcast to v's index)."""
    v = _a(v)
    if mode == 0:
        return v
    if mode == 1:
        return silu(v)
    if mode == 2:
        return np.maximum(v, 0.0)
    if mode == 3:
        return v * _a(p0) + _a(p1)
    raise ValueError(mode)


def grouped_gemm(A_segs, B_segs, *, a_pro=0, a_p=(None, None), b_pro=0, b_p=(None, None), bias=None, epi=0, e0=None, alpha=1.0,
                 addend=None):
    """One member of one seeme_grouped_gemm problem on its logical operands A_segs[s] [M, len_s], B_segs[s] [len_s, N]:
         val = ((sum_s pro_a(A_s) pro_b(B_s) + bias[j]) * epilogue) + addend
    epilogue: epi 1 SiLU'(e0[i,j]), epi 2 alpha.  The affine prologue of A is indexed by k WITHIN the segment (p0[k], k <
    len_s, the same vectors for every segment), that of B by the output column j.  Returns val, mag = sum_s |A'_s| |B'_s|,
    colsum[i] = sum_s sum_k A_s[i,k] (the raw operand) and its magnitude sum |A_s[i,k]|.  What the accumulate mode does with
    val is `accumulate` below."""
    M, N = np.shape(A_segs[0])[0], np.shape(B_segs[0])[1]
    acc, mag = np.zeros((M, N)), np.zeros((M, N))
    cs, csmag = np.zeros(M), np.zeros(M)
    for A, B in zip(A_segs, B_segs):
        A, B = _a(A), _a(B)
        n = A.shape[1]
        assert B.shape[0] == n and n >= 1
        Ap = gg_prologue(A, a_pro, None if a_p[0] is None else _a(a_p[0])[None, :n], None if a_p[1] is None else _a(a_p[1])[None, :n])
        Bp = gg_prologue(B, b_pro, None if b_p[0] is None else _a(b_p[0])[None, :N], None if b_p[1] is None else _a(b_p[1])[None, :N])
        acc += Ap @ Bp
        mag += np.abs(Ap) @ np.abs(Bp)
        cs += A.sum(1)
        csmag += np.abs(A).sum(1)
    val = acc
    if bias is not None:
        val = val + _a(bias)[None, :N]
    if epi == 1:
        val = val * dsilu(_a(e0)[:M, :N])
    elif epi == 2:
        val = val * float(alpha)
    if addend is not None:
        val = val + _a(addend)[:M, :N]
    return val, mag, cs, csmag


def accumulate(c0, vals, mode):
    """0: C = val; 1: C = C0 + val (one writer); 2: C = C0 + sum over the batch members that share C."""
    if mode == 0:
        assert len(vals) == 1
        return vals[0]
    if mode == 1:
        assert len(vals) == 1
        return _a(c0) + vals[0]
    return _a(c0) + sum(vals)


def gemm128(A, B, b_is_nt, bias=None, addend=None):
    """seeme_gemm128: C = A B + bias[N] + addend, B = W[N,K] used transposed (b_is_nt) or W[K,N].  Returns val, mag."""
    A, B = _a(A), _a(B)
    Bm = B.T if b_is_nt else B
    val = A @ Bm
    if bias is not None:
        val = val + _a(bias)[None, :]
    if addend is not None:
        val = val + _a(addend)
    return val, np.abs(A) @ np.abs(Bm)


def wgrad128(dY, X, G0, gbias0=None):
    """seeme_wgrad128: G = G0 + dY^T X, gbias = gbias0 + column sums of dY.  Returns G, mag, gbias, gbias mag."""
    dY, X = _a(dY), _a(X)
    G = _a(G0) + dY.T @ X
    gb = None if gbias0 is None else _a(gbias0) + dY.sum(0)
    return G, np.abs(dY).T @ np.abs(X), gb, np.abs(dY).sum(0)


# ----------------------------------------------------------------------------- stage-1 row kernels
def layer_norm_stats(v, eps, dtype=np.float64):
    """xhat = (v - mean) * rstd, rstd = 1 / sqrt(biased variance + eps), over the last axis."""
    v = _a(v, dtype)
    n = dtype(v.shape[-1])
    mean = v.sum(-1, keepdims=True, dtype=dtype) / n
    c = v - mean
    var = (c * c).sum(-1, keepdims=True, dtype=dtype) / n
    rstd = dtype(1) / np.sqrt(var + dtype(eps))
    return c * rstd, rstd[..., 0]


def vt_add_ln(sub, res, gamma, beta, M, sub_seq_rows=0, eps=1e-5, dtype=np.float64):
    """seeme_vt_add_ln: y = LN(sub + res) * gamma + beta over 256 features; sub_seq_rows > 0: row m takes sub[m // sub_seq_rows].
    Returns y, xhat, rstd."""
    sub = _a(sub, dtype)
    v = sub[np.arange(M) // sub_seq_rows] if sub_seq_rows > 0 else sub[:M]
    if res is not None:
        v = v + _a(res, dtype)[:M]
    xhat, rstd = layer_norm_stats(v, eps, dtype)
    return xhat * _a(gamma, dtype) + _a(beta, dtype), xhat, rstd


def ln_backward(g, xhat, rstd, dtype=np.float64):
    """Gradient through xhat = (v - mean) rstd of a gradient g w.r.t. xhat: rstd (g - mean(g) - xhat mean(g xhat))."""
    g, xhat = _a(g, dtype), _a(xhat, dtype)
    n = dtype(g.shape[-1])
    m1 = g.sum(-1, keepdims=True, dtype=dtype) / n
    m2 = (g * xhat).sum(-1, keepdims=True, dtype=dtype) / n
    return _a(rstd, dtype)[..., None] * (g - m1 - xhat * m2)


def vt_ln_bwd(dy, xhat, rstd, gamma, dy2=None, accumulate=0, dpre0=None, dgamma0=None, dbeta0=None, dtype=np.float64):
    """seeme_vt_ln_bwd: with d = dy (+ dy2): dpre (+)= LN-backward(d * gamma); dgamma += sum_m d * xhat; dbeta += sum_m d.
    Returns dpre, dgamma, dbeta and the magnitudes sum_m |d xhat|, sum_m |d| of the two column sums."""
    d = _a(dy, dtype)
    if dy2 is not None:
        d = d + _a(dy2, dtype)
    xhat = _a(xhat, dtype)
    dpre = ln_backward(d * _a(gamma, dtype), xhat, rstd, dtype)
    if accumulate:
        dpre = dpre + _a(dpre0, dtype)
    dgamma = _a(dgamma0, dtype) + (d * xhat).sum(0, dtype=dtype)
    dbeta = _a(dbeta0, dtype) + d.sum(0, dtype=dtype)
    return dpre, dgamma, dbeta, np.abs(d * xhat).sum(0), np.abs(d).sum(0)


def softmax_valid(lengths, S, n_prefix):
    """keys [0, n_b) take part, n_b = min(S, n_prefix + lengths[b]); n_b >= 1 is the caller's contract."""
    return [min(S, n_prefix + int(l)) for l in lengths]


def vt_softmax_fwd(scores, lengths, n_prefix, scale, dtype=np.float64):
    """seeme_vt_softmax_fwd: scores [B,S,S] -> softmax(scale * s) over the valid keys, exact zeros elsewhere (whatever the masked
    inputs hold)."""
    s = np.asarray(scores)
    B, S = s.shape[0], s.shape[-1]
    out = np.zeros(s.shape, dtype)
    for b, n in enumerate(softmax_valid(lengths, S, n_prefix)):
        assert n >= 1
        v = _a(s[b, :, :n], dtype) * dtype(scale)
        e = np.exp(v - v.max(-1, keepdims=True))
        out[b, :, :n] = e / e.sum(-1, keepdims=True, dtype=dtype)
    return out


def vt_softmax_bwd(dp, p, scale, dtype=np.float64):
    """seeme_vt_softmax_bwd: rows of dL/dP -> dL/d(unscaled scores) = scale * P * (dP - sum_k dP_k P_k)."""
    dp, p = _a(dp, dtype), _a(p, dtype)
    dot = (dp * p).sum(-1, keepdims=True, dtype=dtype)
    return dtype(scale) * p * (dp - dot)


def vt_seq_sum(d, out0, accumulate, wmask, scale):
    """seeme_vt_seq_sum: out[b,:] (+)= sum_s w[b,s] d[b,s,:], w = wmask ? scale : 0 (1 when wmask is None).  Returns out, mag."""
    d = _a(d)
    B, S = d.shape[:2]
    w = np.ones((B, S)) if wmask is None else np.where(np.asarray(wmask).reshape(B, S) != 0, float(np.float32(scale)), 0.0)
    out = (w[:, :, None] * d).sum(1)
    mag = np.abs(w[:, :, None] * d).sum(1)
    if accumulate:
        out = out + _a(out0)
    return out, mag


def vt_dropout(x, mask, scale):
    """seeme_vt_dropout: a single float32 rounding, float32(x) * float32(scale) where the mask byte is non-zero, +0 elsewhere."""
    x = np.asarray(x, np.float32)
    return np.where(np.asarray(mask) != 0, x * np.float32(scale), np.float32(0)).astype(np.float32)


def vt_cross_rows(cvn, bo, wmask, m2, scale, dtype=np.float64):
    """seeme_vt_cross_rows: out[b,s,:] = ((wmask[b,s] ? scale : 0) * cvn[b,:] + bo) * (m2[b,s,:] ? scale : 0)."""
    sc = dtype(np.float32(scale))
    w = np.where(np.asarray(wmask) != 0, sc, dtype(0))[:, :, None]
    k = np.where(np.asarray(m2) != 0, sc, dtype(0))
    return (w * _a(cvn, dtype)[:, None, :] + _a(bo, dtype)) * k


# ----------------------------------------------------------------------------- stage-2 glue
def glue_rows(B, N, dist, eps_z, eps_c, slot_c, cond0, noise, timesteps, acp, freq, flip_sin_to_cos, dtype=np.float64):
    """seeme_glue_rows.  dist [2, dist_rows, 256] (mu, logvar); latents z = mu + eps_z * exp(logvar / 2) on rows [0,B); with eps_c
    the same rsample of rows [B,2B) goes to cond[:, slot_c] (the other slots keep cond0); noisy = sqrt(acp[t]) z + sqrt(1 - acp[t])
    noise; tfeat = [sin | cos](t * freq) (cos first when flip_sin_to_cos), the argument formed in float32.
    Returns latents, noisy, tfeat, cond."""
    dist = _a(dist, dtype)
    mu, lv = dist[0], dist[1]
    half = dtype(0.5)
    z = mu[:B] + _a(eps_z, dtype) * np.exp(half * lv[:B])
    cond = None if cond0 is None else np.array(cond0, dtype=dtype).reshape(B, N, 256)
    if eps_c is not None:
        cond[:, slot_c] = mu[B:2 * B] + _a(eps_c, dtype) * np.exp(half * lv[B:2 * B])
    t = np.asarray(timesteps, np.int64)
    a = _a(np.asarray(acp, np.float32)[t], dtype)[:, None]
    noisy = np.sqrt(a) * z + np.sqrt(dtype(1) - a) * _a(noise, dtype)
    arg = _a(t.astype(np.float32)[:, None] * np.asarray(freq, np.float32)[None, :], dtype)     # [B,128], float32 product
    s, c = np.sin(arg), np.cos(arg)
    tfeat = np.concatenate([c, s] if flip_sin_to_cos else [s, c], axis=1)
    return z, noisy, tfeat, cond


def glue_ln(x, dtype=np.float64):
    """seeme_glue_ln: F.layer_norm(x, (256,)) without affine, eps 1e-5.  Returns xhat, rstd."""
    return layer_norm_stats(x, 1e-5, dtype)


def glue_mid(dxl, dcs, xhat, rstd, tn_w, g_tn_w0, g_tn_b0, dea, deb, emb, dtype=np.float64):
    """seeme_glue_mid: dcond = sum_l dcs[l] + LN-backward(sum_l dxl[l] * tn_w[l]); g_tn_w[l] = g_tn_w0[l] + sum_m dxl[l] * xhat;
    g_tn_b[l] = g_tn_b0[l] + sum_m dxl[l]; demb = sum_5 dea + SiLU'(emb) * sum_10 deb.
    Returns dcond, g_tn_w, g_tn_b, demb and the magnitudes of the two column sums."""
    dxl, dcs, xhat, tn_w = _a(dxl, dtype), _a(dcs, dtype), _a(xhat, dtype), _a(tn_w, dtype)
    g = (dxl * tn_w[:, None, :]).sum(0, dtype=dtype)
    dcond = dcs.sum(0, dtype=dtype) + ln_backward(g, xhat, rstd, dtype)
    g_w = _a(g_tn_w0, dtype) + (dxl * xhat[None]).sum(1, dtype=dtype)
    g_b = _a(g_tn_b0, dtype) + dxl.sum(1, dtype=dtype)
    demb = _a(dea, dtype).sum(0, dtype=dtype) + dsilu(emb, dtype) * _a(deb, dtype).sum(0, dtype=dtype)
    return dcond, g_w, g_b, demb, np.abs(dxl * xhat[None]).sum(1), np.abs(dxl).sum(1)


# ----------------------------------------------------------------------------- denoiser chain gradients
def den_wgrad(gout, tiles, out0):
    """seeme_den_wgrad: for every tile (x_col, y_col, ldo, nn, kk, out_off): out[out_off + n*ldo + k] = sum_b gout[b, y_col + n] *
    gout[b, x_col + k].  Returns out (a float64 copy of out0 with the tiles written) and mag (0 outside the tiles)."""
    g = _a(gout)
    out = np.array(out0, dtype=np.float64)
    mag = np.zeros_like(out)
    for x_col, y_col, ldo, nn, kk, out_off in tiles:
        dy, x = g[:, y_col:y_col + nn], g[:, x_col:x_col + kk]
        idx = out_off + np.arange(nn)[:, None] * ldo + np.arange(kk)[None, :]
        out[idx] = dy.T @ x
        mag[idx] = np.abs(dy).T @ np.abs(x)
    return out, mag


def den_vecgrad(gout, idx, dx0_col):
    """seeme_den_vecgrad: out[q] = sum_b gout[b, idx[q]]; dpe_row0[c] = sum_b gout[b, dx0_col + c], c < 256.
    Returns out, its magnitude, dpe_row0, its magnitude."""
    g = _a(gout)
    idx = np.asarray(idx, np.int64)
    cols = dx0_col + np.arange(256)
    return g[:, idx].sum(0), np.abs(g[:, idx]).sum(0), g[:, cols].sum(0), np.abs(g[:, cols]).sum(0)
