"""The VAE kernels at their key, row and batch edges: csrc/vae_h16.hip (precision="fp16": k_vae_pro_h, k_layer_h<8,4> / <4,8>, and
below 16 tokens k_qkv_h / k_attn_block_h / k_ffn_block_h / k_linear_h) and the fp32 path of csrc/vae_kernels.hip, through MldVae
with recipe weights.  Three kinds of test, none of which needs a rounding model of the fp16 path:

  * bit-exact properties (c, d, f, g): pad frames and workspace contents are never seen, a sequence does not depend on its batch;
  * loud edge inputs (a, e): the cases of tests/vae_edges_reference.py, on which the float64 oracle itself moves by at least 5e-2
    when a length is one off, so `5 * err <= sensitivity` separates a one-key mistake from fp16 rounding;
  * negative controls (b, e): the HIP path run with the length one off must FAIL that inequality.

All errors are per sequence, max|a - b| / max|b| over that sequence's rows.  Needs a real MI355X: run with `pytest -m gpu`.

Measured on an MI355X against the float64 oracle, fp16 path, err of sequence 0 and of sequence 1 (the fp32 path: at most 1.3e-6 in
every case).  Worst encoder case 2.13e-3 (F = 132, L = 2, sequence 0): TOL_EDGE = 3 x that = 6.4e-3; the smallest sensitivity / err
over the encoder cases is 70.  Worst decoder case 9.99e-4 (F = 132, L = 256, sequence 1): TOL_DEC = 3 x that = 3.0e-3.  The runs are
deterministic; the factor 3 is room for a later re-seed.  In the negative controls err / sensitivity was never below 0.996.

  Encoder (loud cases):    L   F = 75: seq 0   seq 1    F = 132: seq 0   seq 1
                            1           7.1e-04  7.7e-04           8.0e-04  5.7e-04
                            2           8.3e-04  5.1e-04           2.1e-03  6.6e-04
                            3           7.7e-04  8.6e-04           6.3e-04  7.0e-04
                            4           1.2e-03  6.0e-04           8.0e-04  6.9e-04
                           13           5.4e-04  6.1e-04           9.7e-04  7.0e-04
                           14           6.4e-04  5.7e-04           6.4e-04  6.1e-04
                           15           8.1e-04  6.2e-04           5.2e-04  5.8e-04
                           29           5.7e-04  6.0e-04           6.6e-04  4.3e-04
                           30           7.3e-04  5.6e-04           8.2e-04  6.8e-04
                           31           6.9e-04  4.7e-04           4.3e-04  6.2e-04
                           61           6.0e-04  4.6e-04           8.1e-04  4.5e-04
                           62           5.0e-04  5.2e-04           5.6e-04  6.0e-04
                           63           6.7e-04  4.8e-04           7.3e-04  4.9e-04
                          253           4.4e-04  6.4e-04           5.3e-04  5.9e-04
                          254           5.5e-04  5.1e-04           4.9e-04  5.7e-04
                          255           5.3e-04  5.1e-04           5.1e-04  5.0e-04
                          256           5.9e-04  4.6e-04           2.1e-03  6.1e-04
                          257           1.7e-03  5.2e-04           7.0e-04  5.5e-04
                          300           4.9e-04  5.2e-04           5.8e-04  5.1e-04
                          496           8.2e-04  6.2e-04           4.3e-04  4.9e-04
  Decoder:    L   F = 75: seq 0   seq 1    F = 132: seq 0   seq 1
               1           8.8e-04  5.9e-04           9.3e-04  6.0e-04
               2           8.7e-04  8.4e-04           7.4e-04  8.2e-04
               3           6.0e-04  7.8e-04           7.0e-04  9.1e-04
               4           6.4e-04  7.5e-04           6.4e-04  6.5e-04
              14           7.3e-04  6.1e-04           6.5e-04  5.8e-04
              15           7.0e-04  7.1e-04           6.9e-04  7.3e-04
              16           9.8e-04  7.6e-04           7.3e-04  7.4e-04
              17           8.0e-04  8.7e-04           7.4e-04  6.4e-04
              31           7.9e-04  8.4e-04           6.9e-04  8.5e-04
              32           7.4e-04  7.1e-04           8.1e-04  7.5e-04
              33           7.0e-04  7.9e-04           8.3e-04  7.5e-04
              63           6.3e-04  5.8e-04           5.0e-04  5.6e-04
              64           6.9e-04  9.1e-04           7.6e-04  8.6e-04
              65           7.4e-04  5.6e-04           7.2e-04  7.9e-04
             255           7.3e-04  8.3e-04           6.4e-04  9.2e-04
             256           7.6e-04  9.6e-04           7.8e-04  1.0e-03
             257           5.8e-04  7.1e-04           6.6e-04  8.4e-04
             300           8.8e-04  6.9e-04           7.7e-04  7.4e-04
             496           5.7e-04  8.1e-04           7.1e-04  6.4e-04
  F = 144, L = 17: 6.5e-04  7.4e-04
"""
import numpy as np
import pytest
import torch

import vae_edges_reference as R
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-4        # the project's parity gate
TOL_EDGE = 6.4e-3     # fp16 encoder on the loud cases: 3 x the worst measured case (2.13e-3)
TOL_DEC = 3.0e-3      # fp16 decoder: 3 x the worst measured case (9.99e-4)
FACTOR = 5            # discrimination: 5 * err <= the oracle's own change for a length one off

ENC_CASES = sorted(R.ENC_TABLE)
# one L per edge family: unfused sequence, 16-key tile (n_valid = 16), 32-key block, 64-column chunk, Sp 256 -> 512, 500 tokens
CONTROL_LENGTHS = (2, 14, 30, 62, 254, 496)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


_VAES = {}


def _vae(dev, F, precision):
    """One module per (F, precision), shared between tests."""
    if (F, precision) not in _VAES:
        import types
        from seeme_amd.mld_vae import MldVae
        abl = types.SimpleNamespace(MLP_DIST=False, PE_TYPE="mld", SKIP_CONNECT=True, VAE_TYPE="actor", DIFF_PE_TYPE="mld", MD_TRANS=True)
        _VAES[(F, precision)] = load_recipe_(MldVae(abl, nfeats=F, latent_dim=[1, 256], arch="encoder_decoder",
                                                    precision=precision)).to(dev).eval()
    return _VAES[(F, precision)]


def _encode(dev, F, precision, x, lengths):
    return _vae(dev, F, precision).encode_dist(torch.from_numpy(np.ascontiguousarray(x)).to(dev), list(lengths)).cpu().numpy()


def _decode(dev, F, precision, z, lengths):
    return _vae(dev, F, precision).decode(torch.from_numpy(np.ascontiguousarray(z)).to(dev), list(lengths)).cpu().numpy()


def _fill_workspace(dev, F, precision, B, T, byte):
    vae = _vae(dev, F, precision)
    vae._workspace(B, T, dev)
    vae._ws.fill_(byte)           # the whole cached allocation, which may be larger than this shape needs


def _valid(dec, lengths):
    return [dec[b, :n] for b, n in enumerate(lengths)]


# ----------------------------------------------------------------------------- a: encoder edges against the oracle
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("F,L", ENC_CASES)
def test_encoder_edges_vs_oracle(dev, F, L, precision):
    """Sequence 0 ends at a loud frame and is followed by a loud pad frame; sequence 1 is two tokens longer, so the pair straddles
    the edge.  fp32 path: the 1e-4 gate.  fp16 path: within TOL_EDGE, and five times closer to the oracle than the oracle at a
    length one off is."""
    x, lengths = R.enc_case(F, L)
    ref, sens = R.enc_reference(F, L), R.enc_sens(F, L)
    got = _encode(dev, F, precision, x, lengths)
    assert np.isfinite(got).all()
    e0, e1 = R.seq_err(got[:, 0], ref[:, 0]), R.seq_err(got[:, 1], ref[:, 1])
    print(f"EDGE enc {precision} F={F} L={L}: err seq0 {e0:.3e} seq1 {e1:.3e} sens {sens:.3e}")
    if precision == "fp32":
        assert e0 < TOL_F32 and e1 < TOL_F32
    else:
        assert FACTOR * e0 <= sens
        assert e0 < TOL_EDGE and e1 < TOL_EDGE


# ----------------------------------------------------------------------------- b: negative control
@pytest.mark.parametrize("F", R.ENC_FEATS)
@pytest.mark.parametrize("L", CONTROL_LENGTHS)
def test_encoder_edges_negative_control(dev, F, L):
    """The fp16 path, called with sequence 0's length one short and one long, fails the inequality of (a) against the oracle at L:
    with the kernel's real numerics, a one-key mistake cannot pass."""
    x, lengths = R.enc_case(F, L)
    ref, sens = R.enc_reference(F, L), R.enc_sens(F, L)
    for l0 in (L - 1, L + 1):
        got = _encode(dev, F, "fp16", x, [l0, lengths[1]])
        e0 = R.seq_err(got[:, 0], ref[:, 0])
        print(f"EDGE enc control F={F} L={L} run at {l0}: err seq0 {e0:.3e} sens {sens:.3e}")
        assert not FACTOR * e0 <= sens


# ----------------------------------------------------------------------------- c: pad frames are never seen
@pytest.mark.parametrize("F,L", ENC_CASES)
def test_pad_frames_are_never_seen(dev, F, L):
    """encode_dist is bit-identical with zeros and with N(0,1) garbage in the frames past each length (unit scale: values that
    overflow fp16 would give 0 x inf in the reference formula too)."""
    x, lengths = R.enc_case(F, L, quiet=True)
    zeros, garbage = x.copy(), x.copy()
    junk = np.random.default_rng(5000 + L).standard_normal(x.shape).astype(np.float32)
    for b, n in enumerate(lengths):
        zeros[b, n:] = 0
        garbage[b, n:] = junk[b, n:]
    assert not np.array_equal(zeros, garbage)
    for precision in ("fp32", "fp16"):
        a, g = _encode(dev, F, precision, zeros, lengths), _encode(dev, F, precision, garbage, lengths)
        assert np.isfinite(a).all() and np.array_equal(a, g), (precision, float(np.abs(a - g).max()))


# ----------------------------------------------------------------------------- d: workspace contents are never seen
# S = L + 4 tokens: 6 (below 16: unfused), 17 and 65 (S % 16 != 0 and S % 32 != 0), 258 (Sp = 512)
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("F,L", [(75, 2), (132, 13), (75, 61), (132, 254)])
def test_encoder_ignores_workspace_contents(dev, F, L, precision):
    """The workspace is torch.empty and reused across calls: bytes 0xFF (NaN as fp16 and as fp32) in all of it change nothing."""
    x, lengths = R.enc_case(F, L, quiet=True)
    _fill_workspace(dev, F, precision, 2, lengths[1], 0)
    clean = _encode(dev, F, precision, x, lengths)
    _fill_workspace(dev, F, precision, 2, lengths[1], 0xFF)
    dirty = _encode(dev, F, precision, x, lengths)
    assert np.isfinite(dirty).all() and np.array_equal(clean, dirty)


# T = L + 2 tokens: 3 and 6 (unfused, V^T in the packed-key region and behind q | k), 17 and 65, 257 (Sp = 512)
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("F,L", [(132, 1), (75, 4), (75, 15), (132, 63), (75, 255)])
def test_decoder_ignores_workspace_contents(dev, F, L, precision):
    z, lengths = R.dec_case(F, L)
    _fill_workspace(dev, F, precision, 2, lengths[1], 0)
    clean = _decode(dev, F, precision, z, lengths)
    _fill_workspace(dev, F, precision, 2, lengths[1], 0xFF)
    dirty = _decode(dev, F, precision, z, lengths)
    for c, d in zip(_valid(clean, lengths), _valid(dirty, lengths)):
        assert np.isfinite(d).all() and np.array_equal(c, d)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_decoder_after_larger_encoder_call(dev, precision):
    """A decoder call directly after an encoder call of a larger shape finds that call's rows beyond its own S in the workspace."""
    F = 75
    z, lengths = R.dec_case(F, 31)                                     # T = 33
    x, xl = R.enc_case(F, 300, quiet=True)                             # S = 304
    _fill_workspace(dev, F, precision, 2, xl[1], 0)
    clean = _decode(dev, F, precision, z, lengths)
    _encode(dev, F, precision, x, xl)
    stale = _decode(dev, F, precision, z, lengths)
    for c, d in zip(_valid(clean, lengths), _valid(stale, lengths)):
        assert np.isfinite(d).all() and np.array_equal(c, d)


# ----------------------------------------------------------------------------- e: decoder edges against the oracle
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("F,L", R.DEC_CASES)
def test_decoder_edges_vs_oracle(dev, F, L, precision):
    """Every frame < len of both sequences: fp32 path below 1e-4, fp16 path below TOL_DEC.  The decoder has no input that makes a
    key loud: the oracle's own change for a length one off (dec_sens, tests/test_vae_edges_cpu.py) falls from 0.2 at L = 1 to below
    1e-3 at L = 496.  Where it is at least 5 * TOL_DEC (the short lengths) the fp16 path is also held to the discrimination
    inequality, with its negative control (the call with L - 1 and L + 1 must fail it on the frames all three runs share).  Above
    that length the decoder's key edges are held only by the bit-exact tests (c, d, f) and by the encoder cases, which run the same
    k_layer_h mask code with n_prefix = 2.  Frames >= len are unspecified and not compared."""
    z, lengths = R.dec_case(F, L)
    ref, sens = R.dec_reference(F, L), R.dec_sens(F, L)
    got = _decode(dev, F, precision, z, lengths)
    assert got.shape == ref.shape
    e0, e1 = (R.seq_err(g, r) for g, r in zip(_valid(got, lengths), _valid(ref, lengths)))
    print(f"EDGE dec {precision} F={F} L={L}: err seq0 {e0:.3e} seq1 {e1:.3e} dec_sens {sens:.3e}")
    assert np.isfinite(e0) and np.isfinite(e1)
    if precision == "fp32":
        assert e0 < TOL_F32 and e1 < TOL_F32
        return
    assert e0 < TOL_DEC and e1 < TOL_DEC
    if sens >= FACTOR * TOL_DEC:
        assert FACTOR * e0 <= sens
        n = R.dec_common(L)
        for l0 in ([L - 1] if L > 1 else []) + [L + 1]:
            wrong = _decode(dev, F, "fp16", z, [l0, L + 2])
            ew = R.seq_err(wrong[0, :n], ref[0, :n])
            print(f"EDGE dec control F={F} L={L} run at {l0}: err seq0 {ew:.3e} dec_sens {sens:.3e}")
            assert not FACTOR * ew <= sens


# ----------------------------------------------------------------------------- f: partition independence, ragged lengths
def test_fp16_ragged_batch_partition_independence(dev):
    """B = 40, T = 300 is 400 workgroups (k_layer_h<4,8>) at Sp = 512; rows 0, 17 and 39 alone are 30 workgroups (k_layer_h<8,4>).
    With ragged lengths the same sequences come out bit-identical either way, encode and decode."""
    F, T, B = 75, 300, 40
    pat = [300, 256, 64, 257, 17, 1]
    lengths = [pat[i % 6] for i in range(B)]
    idx = [0, 17, 39]
    sub = [lengths[i] for i in idx]
    assert sub == [300, 1, 257] and set(lengths) == set(pat)
    rng = np.random.default_rng(41)
    x = torch.from_numpy(rng.standard_normal((B, T, F)).astype(np.float32)).to(dev)
    z = torch.from_numpy(rng.standard_normal((1, B, 256)).astype(np.float32)).to(dev)
    vae = _vae(dev, F, "fp16")
    big = vae.encode_dist(x, lengths)
    small = vae.encode_dist(x[idx].contiguous(), sub)
    assert bool(torch.isfinite(big).all()) and torch.equal(big[:, idx], small)
    dbig = vae.decode(z, lengths)
    dsmall = vae.decode(z[:, idx].contiguous(), sub)
    for j, (i, n) in enumerate(zip(idx, sub)):
        assert bool(torch.isfinite(dbig[i, :n]).all()) and torch.equal(dbig[i, :n], dsmall[j, :n]), i


# ----------------------------------------------------------------------------- g: in_shared
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("T", [24, 300])
def test_decoder_first_layer_shared_inputs(dev, T, precision):
    """The decoder's first layer reads one sequence's q / K / V for every batch member (in_shared): three different z with equal
    lengths decode bit-identically to each z alone."""
    F = 132
    z = torch.from_numpy(np.random.default_rng(43).standard_normal((1, 3, 256)).astype(np.float32)).to(dev)
    vae = _vae(dev, F, precision)
    batch = vae.decode(z, [T] * 3)
    assert bool(torch.isfinite(batch).all())
    for b in range(3):
        alone = vae.decode(z[:, b:b + 1].contiguous(), [T])
        assert torch.equal(batch[b], alone[0]), b
    assert not torch.equal(batch[0], batch[1])
