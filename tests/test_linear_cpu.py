"""The float64 twin of tests/linear_reference.py against torch float64 (F.linear, F.layer_norm, F.gelu, F.silu, torch.cat): a wrong
twin must not be able to bless a wrong kernel.  No GPU; float64 on both sides, so the bound is a few float64 roundings (1e-11 of
the tensor's largest entry).  The epilogue combinations and the sum-bound cases are read from the case table of
tests/test_gpu_linear_edges.py, so the two files cannot drift apart."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linear_reference as LR
import test_gpu_linear_edges as G

TOL = 1e-11
EPS = float(np.float32(1e-5))


def _close(got, want, what=""):
    got, want = np.asarray(got, np.float64), want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= TOL * max(1.0, float(np.abs(want).max())), (what, err)


def _t(x):
    return torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)


def _torch_act(x, act):
    return {LR.ACT_NONE: lambda v: v, LR.ACT_RELU: F.relu, LR.ACT_GELU: F.gelu, LR.ACT_SILU: F.silu}[act](x)


def _combo(c):
    return (c.concat, c.bias, c.res, c.ln, c.pre_ln, c.pre_act, c.act)


COMBOS = sorted({_combo(c) for c in G.CASES + [G.WIDE_CASE]})


@pytest.mark.parametrize("combo", COMBOS, ids=[str(tuple(int(v) for v in c)) for c in COMBOS])
def test_twin_matches_torch_float64(combo):
    """Every (concat, bias, res, fused LN, pre-LN, pre_act, act) combination the GPU file uses, at M = 3, K = 7 (K1 = 3), N = 5 (256
    with the fused LN, as the kernel requires); W carries columns past K that must not take part."""
    concat, bias, res, ln, pre_ln, pre_act, act = combo
    rng = np.random.Generator(np.random.PCG64(41))
    M, K, K1, N = 3, 7, 3, 256 if ln else 5
    X, W = rng.standard_normal((M, K)), rng.standard_normal((N, K + 9))
    b, r = rng.standard_normal(N), rng.standard_normal((M, N))
    lw, lb, pw, pb = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal(K), rng.standard_normal(K)
    out = LR.linear(X[:, :K1] if concat else X, W, K, A2=X[:, K1:] if concat else None, bias=b if bias else None, res=r if res else None,
                    ln=(lw, lb) if ln else None, pre_ln=(pw, pb) if pre_ln else None, pre_act=pre_act, act=act, eps=EPS)
    x = torch.cat([_t(X[:, :K1]), _t(X[:, K1:])], dim=1) if concat else _t(X)
    if pre_ln:
        x = F.layer_norm(x, (K,), _t(pw), _t(pb), EPS)
    x = _torch_act(x, pre_act)
    s = F.linear(x, _t(W[:, :K]), _t(b) if bias else None)
    a = _torch_act(s, act)
    y = a + _t(r) if res else a
    if ln:
        y = F.layer_norm(y, (N,), _t(lw), _t(lb), EPS)
    _close(out.pre, s, "pre")
    _close(out.act, a, "act")
    _close(out.y, y, "y")
    mag = x.abs() @ _t(W[:, :K]).abs().T + (_t(b).abs() if bias else 0.0)
    _close(out.mag, mag, "mag")
    _close(out.res_abs, _t(r).abs() if res else torch.zeros(M, N, dtype=torch.float64), "res_abs")


def test_float32_twin_runs_in_float32_and_keeps_a_float64_magnitude():
    rng = np.random.Generator(np.random.PCG64(42))
    A, W, b = rng.standard_normal((4, 9)).astype(np.float32), rng.standard_normal((6, 16)).astype(np.float32), rng.standard_normal(6).astype(np.float32)
    o32 = LR.linear(A, W, 9, bias=b, pre_act=LR.ACT_SILU, act=LR.ACT_GELU, res=b[None, :] * A[:, :1], dtype=np.float32)
    o64 = LR.linear(A, W, 9, bias=b, pre_act=LR.ACT_SILU, act=LR.ACT_GELU, res=b[None, :] * A[:, :1])
    assert o32.y.dtype == np.float32 and o32.pre.dtype == np.float32 and o32.act.dtype == np.float32
    assert o32.mag.dtype == np.float64 and np.array_equal(o32.mag, o64.mag)
    assert 0 < np.abs(o32.y - o64.y).max() < 1e-5


def test_constant_row_into_the_fused_layer_norm_is_exactly_the_bias():
    case = next(c for c in G.CASES if c.zero_row is not None)
    p = G.Problem(case)
    for dtype in (np.float64, np.float32):
        assert np.array_equal(p.twin(dtype).y[case.zero_row], p.lnb[:case.N].astype(dtype))


SUM_CASES = [c for c in G.CASES + [G.WIDE_CASE] if c.sum_bound]


@pytest.mark.parametrize("case", SUM_CASES, ids=[c.id for c in SUM_CASES])
def test_float32_twin_lies_inside_every_sum_bound(case):
    """The one condition the case list must satisfy: the sum bound is the worst case of ANY order of the additions, so the same
    formula in float32 numpy must lie inside it on the very inputs of the GPU case."""
    p = G.Problem(case)
    ref = p.twin()
    bound, _ = p.bound(ref)
    err = np.abs(np.asarray(p.twin(np.float32).y, np.float64) - ref.y)
    assert (err <= bound).all(), (case.id, float((err / bound).max()))


def test_the_case_table_names_what_it_runs():
    """narrow cases are narrow by the launcher's rule (asserted when a Case is built); the LayerNorm cases take the row rule."""
    assert all(c.sum_bound != (c.ln or c.pre_ln) for c in G.CASES)
    assert sum(c.narrow for c in G.CASES) == 15 and all(c.N >= 512 and c.M == 32 for c in G.CASES if c.narrow)
    assert {c.K for c in G.CASES if c.group == "K pipeline"} >= {16 * k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63)} | {1008}
