"""The exact-16-bit denoiser of tests/exact16_reference.py, checked with the float64 oracle alone (no GPU): the premises that
tests/test_gpu_exact16.py rests on when it holds the 16-bit kernels to fp32 tolerance."""
import functools

import numpy as np
import pytest

import exact16_reference as X
from conftest import rel_err
from oracle import mld_oracle as O
from seeme_amd import shapes
from seeme_amd.weights_recipe import recipe_state_dict


@functools.lru_cache(maxsize=None)
def _params(dtype, num_heads=1):
    return X.oracle_params(X.structured_denoiser(dtype, num_heads=num_heads))


def _plain():
    return {k: v.astype(np.float64) for k, v in recipe_state_dict(shapes.denoiser_shapes()).items()}


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_structured_model_is_exact(dtype):
    P = _params(dtype)
    assert set(P) == set(_plain())                                     # the oracle's names
    assert X.matrices_are_exact(P, dtype) and X.folds_are_exact(P, dtype)
    assert len(X.folded_products(P)) == 7                              # W_o W_v of five layers, W_in' W_s of two
    # several heads: out_proj dense and merely rounded, no W_o W_v fold
    assert X.matrices_are_exact(_params(dtype, 2), dtype)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_exactness_check_can_fail(dtype):
    plain = _plain()
    assert not X.folds_are_exact(plain, dtype) and not X.matrices_are_exact(plain, dtype)
    # rounding the matrices alone does not make the products representable ...
    rounded = {k: (X.round_through(v, dtype).astype(np.float64) if X.is_matrix_weight(k, v) else v) for k, v in plain.items()}
    assert X.matrices_are_exact(rounded, dtype) and not X.folds_are_exact(rounded, dtype)
    # ... and neither does one structured factor without the other
    P = _params(dtype)
    for part in ("self_attn.out_proj.weight", ".linear_blocks."):
        Q = {k: (rounded[k] if part in k else v) for k, v in P.items()}
        assert not X.folds_are_exact(Q, dtype), part
    # a per-row scale of 1/2 loses bits of small fp16 entries (subnormal range); bf16 has the exponent range of fp32
    Q = dict(P)
    for k in P:
        if k.endswith("self_attn.out_proj.weight"):
            Q[k] = P[k] * 0.5
    assert X.folds_are_exact(Q, dtype) == (dtype == "bf16")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("num_heads", [1, 2])
def test_structured_model_output_is_ordinary(dtype, num_heads):
    """One forward has unit scale (std within 0.5 .. 2); the 6-step DDIM latent is finite and of the size the recipe model gives
    (std about 8, absmax about 30): nothing saturates or collapses under the permutation structure."""
    P = _params(dtype, num_heads)
    lat, cond = X.sensitivity_inputs()
    y = O.denoiser_forward(P, lat, 501, np.transpose(cond, (1, 0, 2)), nhead=num_heads)
    z = O.diffusion_reverse(P, cond, lat, 6, nhead=num_heads)
    assert y.dtype == np.float64 and z.dtype == np.float64
    assert np.isfinite(y).all() and np.isfinite(z).all()
    assert 0.5 < y.std() < 2.0
    z_plain = O.diffusion_reverse(_plain(), cond, lat, 6, nhead=num_heads)
    assert 0.5 < z.std() / z_plain.std() < 2.0                         # the loop scales unit noise by about 8 on either model
    assert np.abs(z).max() < 100.0


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_float32_arithmetic_floor(dtype):
    """The oracle evaluated in float32 on the structured model sits some 1e-6 from the float64 result after 6 steps: the room that
    fp32-level kernel arithmetic needs, two orders below the 5e-4 loop bound."""
    P = _params(dtype)
    lat, cond = X.sensitivity_inputs()
    z = O.diffusion_reverse(P, cond, lat, 6)
    z32 = O.diffusion_reverse(O.cast_params(P, np.float32), cond.astype(np.float32), lat.astype(np.float32), 6)
    assert z32.dtype == np.float32
    assert rel_err(z32, z) < 1e-5


def test_sensitivity_perturbation_lies_between_the_bounds():
    """Zeroing one element of input_blocks.0.sa_block.linear2.bias moves the 6-step latent by at least 3 x the new loop bound and at most
    half the old one: a defect the old 16-bit bound admitted and the new one rejects (the GPU test asserts 5e-4 < err < 6e-3)."""
    P = _params("fp16")
    lat, cond = X.sensitivity_inputs()
    z = O.diffusion_reverse(P, cond, lat, 6)
    Q = dict(P)
    b = P[X.PERTURB_KEY].copy()
    assert b[X.PERTURB_INDEX] != 0.0
    b[X.PERTURB_INDEX] = 0.0
    Q[X.PERTURB_KEY] = b
    e = rel_err(O.diffusion_reverse(Q, cond, lat, 6), z)
    print(f"zeroed {X.PERTURB_KEY}[{X.PERTURB_INDEX}]: 6-step rel err {e:.3e}")
    assert 3 * X.LOOP_BOUND <= e <= X.OLD_LOOP_BOUND / 2
