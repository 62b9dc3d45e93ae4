"""The float64 twins of tests/train_kernel_reference.py against torch float64 autograd / functional ops: a wrong twin must not be
able to bless a wrong kernel.  No GPU; everything is float64 on both sides, so the bound is a few float64 roundings (1e-11 of the
tensor's largest entry, far below anything a float32 kernel test could resolve)."""
import numpy as np
import pytest
import torch

import train_kernel_reference as R

TOL = 1e-11


def _close(got, want, what=""):
    got, want = np.asarray(got, np.float64), want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= TOL * max(1.0, float(np.abs(want).max())), (what, err)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _t(x, grad=False):
    return torch.tensor(np.asarray(x, np.float64), dtype=torch.float64, requires_grad=grad)


# ----------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("M,sub_seq_rows,with_res", [(1, 0, False), (5, 0, True), (21, 7, True), (21, 7, False)])
def test_add_ln_forward_matches_layer_norm(M, sub_seq_rows, with_res):
    rng = _rng(1)
    sub = rng.standard_normal((M // sub_seq_rows if sub_seq_rows else M, 256)) * 2 + 0.5
    res = rng.standard_normal((M, 256)) if with_res else None
    gamma, beta = rng.standard_normal(256), rng.standard_normal(256)
    y, xhat, rstd = R.vt_add_ln(sub, res, gamma, beta, M, sub_seq_rows, 1e-5)
    v = _t(sub).repeat_interleave(sub_seq_rows, 0) if sub_seq_rows else _t(sub)
    if with_res:
        v = v + _t(res)
    _close(y, torch.nn.functional.layer_norm(v, (256,), _t(gamma), _t(beta), 1e-5), "y")
    _close(xhat, torch.nn.functional.layer_norm(v, (256,), None, None, 1e-5), "xhat")
    _close(rstd, 1.0 / torch.sqrt(v.var(-1, unbiased=False) + 1e-5), "rstd")
    xh2, rs2 = R.glue_ln(v.numpy())
    _close(xh2, xhat, "glue_ln xhat")
    _close(rs2, rstd, "glue_ln rstd")


def test_add_ln_constant_row_is_exactly_zero_with_rstd_of_eps():
    sub = np.full((2, 256), 3.25)
    y, xhat, rstd = R.vt_add_ln(sub, None, np.ones(256), np.zeros(256), 2, 0, 1e-5)
    assert (xhat == 0).all() and (y == 0).all()
    _close(rstd, np.full(2, 1.0 / np.sqrt(1e-5)))


@pytest.mark.parametrize("M,with_dy2,acc", [(1, False, 0), (33, True, 0), (33, True, 1), (7, False, 1)])
def test_ln_bwd_matches_autograd(M, with_dy2, acc):
    rng = _rng(2)
    v = _t(rng.standard_normal((M, 256)) * 1.5 + 0.3, grad=True)
    gamma, beta = _t(rng.standard_normal(256), grad=True), _t(rng.standard_normal(256), grad=True)
    dy = rng.standard_normal((M, 256))
    dy2 = rng.standard_normal((M, 256)) if with_dy2 else None
    dpre0, dg0, db0 = rng.standard_normal((M, 256)), rng.standard_normal(256), rng.standard_normal(256)
    y = torch.nn.functional.layer_norm(v, (256,), gamma, beta, 1e-5)
    y.backward(_t(dy) + (_t(dy2) if with_dy2 else 0))
    _, xhat, rstd = R.vt_add_ln(v.detach().numpy(), None, gamma.detach().numpy(), beta.detach().numpy(), M, 0, 1e-5)
    dpre, dgamma, dbeta, mg, mb = R.vt_ln_bwd(dy, xhat, rstd, gamma.detach().numpy(), dy2, acc, dpre0, dg0, db0)
    _close(dpre, v.grad + (_t(dpre0) if acc else 0), "dpre")
    _close(dgamma, gamma.grad + _t(dg0), "dgamma")         # the affine gradients always accumulate
    _close(dbeta, beta.grad + _t(db0), "dbeta")
    d = dy + (dy2 if with_dy2 else 0)
    _close(mg, np.abs(d * xhat).sum(0))
    _close(mb, np.abs(d).sum(0))


# ----------------------------------------------------------------------------- masked softmax
@pytest.mark.parametrize("S,n_prefix", [(1, 0), (7, 2), (65, 0), (65, 2)])
def test_masked_softmax_forward_and_backward(S, n_prefix):
    rng = _rng(3)
    B, scale = 3, 0.37
    lengths = [max(1 - n_prefix, 1), max(S // 2, 1), S + 3][:B]          # n = 1 (or n_prefix + 1), a mid n, and a clamped one
    ns = R.softmax_valid(lengths, S, n_prefix)
    assert ns[-1] == S and all(1 <= n <= S for n in ns)
    s = rng.standard_normal((B, S, S)) * 3
    s_nan = s.copy()
    for b, n in enumerate(ns):
        s_nan[b, :, n:] = np.nan
    p = R.vt_softmax_fwd(s_nan, lengths, n_prefix, scale)
    st = _t(s, grad=True)
    mask = torch.zeros(B, 1, S, dtype=torch.bool)
    for b, n in enumerate(ns):
        mask[b, :, n:] = True
    pt = torch.softmax((st * scale).masked_fill(mask, float("-inf")), -1)
    _close(p, pt, "p")
    for b, n in enumerate(ns):
        assert (p[b, :, n:] == 0).all()
    dp = rng.standard_normal((B, S, S))
    pt.backward(_t(dp))
    _close(R.vt_softmax_bwd(dp.reshape(B * S, S), p.reshape(B * S, S), scale).reshape(B, S, S), st.grad, "ds")


# ----------------------------------------------------------------------------- activations
def test_gelu_silu_and_derivatives():
    x = np.concatenate([np.linspace(-10, 10, 401), [0.0, 1e-3, -1e-3]])
    xt = _t(x, grad=True)
    g = torch.nn.functional.gelu(xt)
    _close(R.gelu(x), g, "gelu")
    _close(R.vt_gelu(x), g, "vt_gelu fwd")
    g.sum().backward()
    _close(R.dgelu(x), xt.grad, "gelu'")
    dh = _rng(4).standard_normal(x.shape)
    _close(R.vt_gelu(x, dh), _t(dh) * xt.grad, "vt_gelu bwd")
    xs = _t(x, grad=True)
    s = torch.nn.functional.silu(xs)
    _close(R.silu(x), s, "silu")
    s.sum().backward()
    _close(R.dsilu(x), xs.grad, "silu'")


# ----------------------------------------------------------------------------- grouped GEMM
@pytest.mark.parametrize("a_pro,b_pro,epi", [(0, 0, 0), (1, 2, 1), (2, 3, 2), (3, 1, 1), (3, 3, 2)])
def test_grouped_gemm_twin_matches_composed_matmul(a_pro, b_pro, epi):
    rng = _rng(5)
    M, N, seg_len = 5, 6, (4, 1, 7)
    A = [rng.standard_normal((M, n)) for n in seg_len]
    Bm = [rng.standard_normal((n, N)) for n in seg_len]
    ap0, ap1, bp0, bp1 = rng.standard_normal(8), rng.standard_normal(8), rng.standard_normal(N), rng.standard_normal(N)
    bias, e0, addend, c0, alpha = rng.standard_normal(N), rng.standard_normal((M, N)), rng.standard_normal((M, N)), rng.standard_normal((M, N)), -0.37
    val, mag, cs, csmag = R.grouped_gemm(A, Bm, a_pro=a_pro, a_p=(ap0, ap1), b_pro=b_pro, b_p=(bp0, bp1), bias=bias, epi=epi, e0=e0,
                                         alpha=alpha, addend=addend)

    def pro(v, mode, p0, p1):
        return [v, torch.nn.functional.silu(v), torch.relu(v), v * p0 + p1][mode]

    acc, tmag = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, N, dtype=torch.float64)
    for a, b in zip(A, Bm):
        n = a.shape[1]
        at = pro(_t(a), a_pro, _t(ap0)[None, :n], _t(ap1)[None, :n])          # k within the segment
        bt = pro(_t(b), b_pro, _t(bp0)[None, :], _t(bp1)[None, :])             # the output column
        acc = acc + torch.matmul(at, bt)
        tmag = tmag + torch.matmul(at.abs(), bt.abs())
    want = acc + _t(bias)
    if epi == 1:
        e = _t(e0, grad=True)
        torch.nn.functional.silu(e).sum().backward()
        want = want * e.grad
    elif epi == 2:
        want = want * alpha
    want = want + _t(addend)                                                   # ((A B + bias) * epi) + addend
    _close(val, want, "val")
    _close(mag, tmag, "mag")
    _close(cs, sum(a.sum(1) for a in A), "colsum")
    _close(csmag, sum(np.abs(a).sum(1) for a in A), "colsum mag")
    _close(R.accumulate(c0, [val], 0), want)
    _close(R.accumulate(c0, [val], 1), _t(c0) + want)
    _close(R.accumulate(c0, [val, 2 * val, 3 * val], 2), _t(c0) + 6 * want)


def test_gemm128_and_wgrad128_twins():
    rng = _rng(6)
    A, W, bias, add = rng.standard_normal((4, 3)), rng.standard_normal((5, 3)), rng.standard_normal(5), rng.standard_normal((4, 5))
    val, mag = R.gemm128(A, W, 1, bias, add)
    _close(val, torch.nn.functional.linear(_t(A), _t(W), _t(bias)) + _t(add))
    _close(mag, np.abs(A) @ np.abs(W).T)
    val, mag = R.gemm128(A, W.T.copy(), 0, None, None)
    _close(val, _t(A) @ _t(W).T)
    x, w, b = _t(rng.standard_normal((7, 3))), _t(W, grad=True), _t(bias, grad=True)
    dy = rng.standard_normal((7, 5))
    torch.nn.functional.linear(x, w, b).backward(_t(dy))
    G0, g0 = rng.standard_normal((5, 3)), rng.standard_normal(5)
    G, gmag, gb, gbmag = R.wgrad128(dy, x.numpy(), G0, g0)
    _close(G, w.grad + _t(G0))
    _close(gb, b.grad + _t(g0))
    _close(gmag, np.abs(dy).T @ np.abs(x.numpy()))
    _close(gbmag, np.abs(dy).sum(0))


# ----------------------------------------------------------------------------- glue_mid
@pytest.mark.parametrize("M,B", [(1, 1), (6, 3)])
def test_glue_mid_matches_autograd(M, B):
    rng = _rng(7)
    x = _t(rng.standard_normal((M, 256)) * 1.3 + 0.2, grad=True)
    w = [_t(rng.standard_normal(256), grad=True) for _ in range(5)]
    bb = [_t(rng.standard_normal(256), grad=True) for _ in range(5)]
    dxl, dcs = rng.standard_normal((5, M, 256)), rng.standard_normal((5, M, 256))
    xh_t = torch.nn.functional.layer_norm(x, (256,), None, None, 1e-5)
    loss = sum(((xh_t * w[l] + bb[l]) * _t(dxl[l])).sum() + (x * _t(dcs[l])).sum() for l in range(5))      # cond feeds LN and K|V directly
    emb = _t(rng.standard_normal((B, 256)), grad=True)
    dea, deb = rng.standard_normal((5, B, 256)), rng.standard_normal((10, B, 256))
    loss = loss + sum((emb * _t(dea[l])).sum() for l in range(5)) + sum((torch.nn.functional.silu(emb) * _t(deb[l])).sum() for l in range(10))
    loss.backward()
    xhat, rstd = R.glue_ln(x.detach().numpy())
    gw0, gb0 = rng.standard_normal((5, 256)), rng.standard_normal((5, 256))
    dcond, g_w, g_b, demb, mw, mb = R.glue_mid(dxl, dcs, xhat, rstd, np.stack([t.detach().numpy() for t in w]), gw0, gb0, dea, deb,
                                               emb.detach().numpy())
    _close(dcond, x.grad, "dcond")
    _close(g_w, torch.stack([t.grad for t in w]) + _t(gw0), "g_tn_w")
    _close(g_b, torch.stack([t.grad for t in bb]) + _t(gb0), "g_tn_b")
    _close(demb, emb.grad, "demb")
    _close(mw, np.abs(dxl * xhat[None]).sum(1))
    _close(mb, np.abs(dxl).sum(1))


# ----------------------------------------------------------------------------- one-liners
def test_seq_sum_cross_rows_dropout():
    rng = _rng(8)
    B, S, scale = 3, 5, float(np.float32(1.0 / 0.9))
    d, out0 = rng.standard_normal((B, S, 256)), rng.standard_normal((B, 256))
    wmask = rng.integers(0, 2, (B, S)).astype(np.uint8)
    wmask[1] = 0
    out, mag = R.vt_seq_sum(d, out0, 1, wmask, scale)
    w = _t((wmask != 0) * scale)
    _close(out, _t(out0) + (w[:, :, None] * _t(d)).sum(1), "seq_sum masked")
    _close(mag, (w[:, :, None] * _t(d)).abs().sum(1))
    assert (R.vt_seq_sum(d, out0, 0, wmask, scale)[0][1] == 0).all()
    _close(R.vt_seq_sum(d, out0, 0, None, scale)[0], _t(d).sum(1), "seq_sum unmasked")
    cvn, bo = rng.standard_normal((B, 256)), rng.standard_normal(256)
    m2 = rng.integers(0, 2, (B, S, 256)).astype(np.uint8)
    want = (w[:, :, None] * _t(cvn)[:, None, :] + _t(bo)) * _t((m2 != 0) * scale)
    _close(R.vt_cross_rows(cvn, bo, wmask, m2, scale), want, "cross_rows")
    x = rng.standard_normal(37).astype(np.float32)
    mask = rng.choice(np.array([0, 1, 255], np.uint8), 37)
    got = R.vt_dropout(x, mask, scale)
    want = (torch.from_numpy(x) * torch.tensor(scale, dtype=torch.float32)) * torch.from_numpy((mask != 0).astype(np.float32))
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())          # equal values (a dropped -x is +0 in the twin, -0 here)
    assert not np.signbit(got[mask == 0]).any()


def test_glue_rows_twin():
    rng = _rng(9)
    B, N, R_ = 3, 2, 9
    dist = rng.standard_normal((2, R_, 256))
    eps_z, eps_c, noise = rng.standard_normal((B, 256)), rng.standard_normal((B, 256)), rng.standard_normal((B, 256))
    cond0 = rng.standard_normal((B, N, 256))
    t = np.array([0, 999, 417])
    acp = np.cumprod(1 - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2).astype(np.float32)
    freq = np.exp(-np.log(10000.0) * np.arange(128, dtype=np.float32) / 128).astype(np.float32)
    for flip in (0, 1):
        z, noisy, tfeat, cond = R.glue_rows(B, N, dist, eps_z, eps_c, 1, cond0, noise, t, acp, freq, flip)
        d = _t(dist)
        zt = d[0, :B] + _t(eps_z) * torch.exp(0.5 * d[1, :B])
        _close(z, zt, "latents")
        a = _t(acp.astype(np.float64)[t])[:, None]
        _close(noisy, a.sqrt() * zt + (1 - a).sqrt() * _t(noise), "noisy")
        arg = _t((t.astype(np.float32)[:, None] * freq[None, :]).astype(np.float64))
        want = torch.cat([arg.cos(), arg.sin()] if flip else [arg.sin(), arg.cos()], 1)
        _close(tfeat, want, "tfeat")
        _close(cond[:, 1], d[0, B:2 * B] + _t(eps_c) * torch.exp(0.5 * d[1, B:2 * B]), "cond slot")
        assert np.array_equal(cond[:, 0], cond0[:, 0])
    assert R.glue_rows(B, N, dist, eps_z, None, 0, None, noise, t, acp, freq, 0)[3] is None


def test_den_gradient_twins():
    rng = _rng(10)
    B, ldg = 9, 400
    g = rng.standard_normal((B, ldg))
    tiles = [(3, 40, 7, 1, 1, 0), (100, 50, 300, 17, 100, 64)]
    out0 = rng.standard_normal(64 + 17 * 300)
    out, mag = R.den_wgrad(g, tiles, out0)
    gt = _t(g)
    _close(out[0], (gt[:, 40] * gt[:, 3]).sum())
    want = torch.einsum("bn,bk->nk", gt[:, 50:67], gt[:, 100:200])
    got = np.stack([out[64 + n * 300: 64 + n * 300 + 100] for n in range(17)])
    _close(got, want, "den_wgrad")
    untouched = np.ones(out.shape, bool)
    untouched[0] = False
    for n in range(17):
        untouched[64 + n * 300: 64 + n * 300 + 100] = False
    assert np.array_equal(out[untouched], out0[untouched]) and (mag[untouched] == 0).all() and (mag[~untouched] > 0).all()
    idx = np.array([5, 5, 399, 0, 17])
    o, om, pe, pm = R.den_vecgrad(g, idx, 100)
    _close(o, gt[:, idx].sum(0))
    _close(om, gt[:, idx].abs().sum(0))
    _close(pe, gt[:, 100:356].sum(0))
    _close(pm, gt[:, 100:356].abs().sum(0))


def test_float32_runs_of_the_twins_stay_float32():
    """the tolerance of a row-kernel test is measured by running these same lines in float32: they must not silently promote"""
    rng = _rng(11)
    f = np.float32
    x = rng.standard_normal((3, 256)).astype(f)
    for out in R.vt_add_ln(x, x[::-1], x[0], x[1], 3, 0, 1e-5, f) + R.glue_ln(x, f):
        assert out.dtype == f
    _, xhat, rstd = R.vt_add_ln(x, None, x[0], x[1], 3, 0, 1e-5, f)
    for out in R.vt_ln_bwd(x, xhat, rstd, x[0], x, 1, x, x[0], x[1], f)[:3]:
        assert out.dtype == f
    s = rng.standard_normal((2, 5, 5)).astype(f)
    p = R.vt_softmax_fwd(s, [2, 9], 1, 0.3, f)
    assert p.dtype == f and R.vt_softmax_bwd(s.reshape(10, 5), p.reshape(10, 5), 0.3, f).dtype == f
    assert R.vt_gelu(x, None, f).dtype == f and R.vt_gelu(x, x, f).dtype == f and R.dsilu(x, f).dtype == f
    m = np.ones((1, 3), np.uint8)
    assert R.vt_cross_rows(x[:1], x[0], m, np.ones((1, 3, 256), np.uint8), 1.1, f).dtype == f
    acp = np.linspace(0.999, 0.005, 1000).astype(f)
    for out in R.glue_rows(1, 1, np.stack([x, x]), x[:1], x[:1], 0, x[:1], x[:1], [7], acp, np.linspace(1, 1e-4, 128).astype(f), 0, f):
        assert out.dtype == f
    outs = R.glue_mid(np.stack([x] * 5), np.stack([x] * 5), xhat, rstd, np.stack([x[0]] * 5), np.stack([x[0]] * 5), np.stack([x[1]] * 5),
                      np.stack([x] * 5), np.stack([x] * 10), x, f)
    for out in outs[:4]:
        assert out.dtype == f
