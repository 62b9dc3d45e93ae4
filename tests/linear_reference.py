"""Plain numpy twin of the SeemeLinearArgs contract of include/seeme_hip.h (seeme_linear), written from the header and not from
the kernel, and the error bounds tests/test_gpu_linear_edges.py holds k_linear to.

    Y = LN?( act( pre_act( preLN?( [A | A2] ) ) @ W[:, :K].T + bias ) + res )

The twin computes in ``dtype`` (float64 by default); with ``dtype=np.float32`` the same lines are "the same formula in float32
numpy", as in tests/train_kernel_reference.py, whose scalar functions, LayerNorm and bounds are used here unchanged.
tests/test_linear_cpu.py pins the twin against torch float64.

Bounds (u = 2^-24, the error model of train_kernel_reference.py, no new constants):
  * without a LayerNorm on either side the output is a sum followed by element-wise steps, `sum_path_bound`:
      s  (the value the activation is applied to, a sum of L = K (+ 1 with a bias) terms):  b = (L + 16) u mag + 4 u |s|,
         mag = |A'| |W|^T + |bias| with A' the float64 prologue output;
      act(s): GELU and SiLU have slope at most 1.13 (ReLU and none: 1), so f b + 4 u |act(s)| with f = 1.13 or 1;
      + res: one more rounded addition, u (|act(s)| + |res|).
    Nothing in it depends on the order of the additions, so the float32 twin lies inside it by construction
    (tests/test_linear_cpu.py asserts that for every case of the GPU file that uses it).
  * with a pre-LayerNorm over K or the fused LayerNorm over N: the row rule `R.row_bound(float32 twin, float64 twin)`,
    4 E + 4 u |ref| with E the largest float32-twin error of the same output row.
"""
import types

import numpy as np

import train_kernel_reference as R

ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3


def activation(x, act, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    if act == ACT_NONE:
        return x
    if act == ACT_RELU:
        return np.maximum(x, dtype(0))
    if act == ACT_GELU:
        return R.gelu(x, dtype)
    if act == ACT_SILU:
        return R.silu(x, dtype)
    raise ValueError(act)


def _prologue(A, A2, K, pre_ln, pre_act, eps, dtype):
    X = np.asarray(A, dtype=dtype)
    if A2 is not None:
        X = np.concatenate([X, np.asarray(A2, dtype=dtype)], axis=1)
    assert X.shape[1] == K, (X.shape, K)
    if pre_ln is not None:
        xhat, _ = R.layer_norm_stats(X, eps, dtype)
        X = xhat * np.asarray(pre_ln[0], dtype=dtype)[:K] + np.asarray(pre_ln[1], dtype=dtype)[:K]
    return activation(X, pre_act, dtype)


def linear(A, W, K, *, A2=None, bias=None, res=None, ln=None, pre_ln=None, pre_act=ACT_NONE, act=ACT_NONE, eps=1e-5,
           dtype=np.float64):
    """A [M, K1], A2 [M, K - K1] or None, W [N, >= K] (only W[:, :K] takes part), bias [N], res [M, N], ln / pre_ln = (weight,
    bias) over N / over K.  Returns a namespace: y, the output; pre, the sum the activation is applied to; act, the activated
    value (before the residual); mag = |A'| |W[:, :K]|^T + |bias| with A' the FLOAT64 prologue output whatever `dtype`; res_abs,
    |res| (0 without one)."""
    Wk = np.asarray(W, dtype=dtype)[:, :K]
    N = Wk.shape[0]
    Ap = _prologue(A, A2, K, pre_ln, pre_act, eps, dtype)
    pre = Ap @ Wk.T
    if bias is not None:
        pre = pre + np.asarray(bias, dtype=dtype)[None, :N]
    a = activation(pre, act, dtype)
    y = a
    if res is not None:
        y = y + np.asarray(res, dtype=dtype)
    if ln is not None:
        xhat, _ = R.layer_norm_stats(y, eps, dtype)
        y = xhat * np.asarray(ln[0], dtype=dtype)[:N] + np.asarray(ln[1], dtype=dtype)[:N]
    A64 = Ap if dtype == np.float64 else _prologue(A, A2, K, pre_ln, pre_act, eps, np.float64)
    mag = np.abs(A64) @ np.abs(np.asarray(W, np.float64)[:, :K]).T
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, np.float64))[None, :N]
    res_abs = np.abs(np.asarray(res, np.float64)) if res is not None else np.zeros_like(mag)
    return types.SimpleNamespace(y=y, pre=pre, act=a, mag=mag, res_abs=res_abs)


def sum_path_bound(ref, K, with_bias, act, with_res):
    """The bound on y of a `linear` without pre-LN and without fused LN; `ref` is the float64 twin's namespace."""
    b = R.sum_bound(K + (1 if with_bias else 0), ref.mag, ref.pre)
    f = 1.13 if act in (ACT_GELU, ACT_SILU) else 1.0
    a = np.abs(np.asarray(ref.act, np.float64))
    bound = f * b + 4 * R.U * a
    if with_res:
        bound = bound + R.U * (a + ref.res_abs)
    return bound
