"""fp16 decode without its per-pass glue launches: the decoder prologue cached per (weights, T), and each decoder layer's
cross-attention vector formed inside k_layer_h<8,4> instead of by a k_linear_h launch.

Both are exact re-arrangements.  The cached prologue is the output of the same k_vae_pro_h launch, read from a buffer of its own; the
in-layer vector is the same MFMA on the same fragments in the same k order with one accumulator per output tile and the bias added
in fp32.  So every comparison here is torch.equal, and the only tolerance is TOL_DEC of tests/test_gpu_vae_edges.py, against the
float64 oracle of tests/vae_edges_reference.py.

Which form of a layer runs is a matter of the launch size alone (at most 256 workgroups of 32 rows: 8 waves, the vector formed in
the layer; more: 4 waves, the vector from its own launch), so both are reached through real shapes.
"""
import types

import numpy as np
import pytest
import torch

import vae_edges_reference as R
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu

TOL_DEC = 3.0e-3      # the bound tests/test_gpu_vae_edges.py holds the fp16 decoder to


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _new_vae(dev, F):
    from seeme_amd.mld_vae import MldVae
    abl = types.SimpleNamespace(MLP_DIST=False, PE_TYPE="mld", SKIP_CONNECT=True, VAE_TYPE="actor", DIFF_PE_TYPE="mld", MD_TRANS=True)
    return load_recipe_(MldVae(abl, nfeats=F, latent_dim=[1, 256], arch="encoder_decoder", precision="fp16")).to(dev).eval()


_VAES = {}


def _vae(dev, F):
    """One module per F, shared between the tests that leave its parameters alone; its cache starts empty in every test."""
    if F not in _VAES:
        _VAES[F] = _new_vae(dev, F)
    m = _VAES[F]
    m.dec_prologue_cache = True
    m._dec_pro.clear()
    return m


def _z(dev, B, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((1, B, 256)).astype(np.float32)).to(dev)


def _uncached(m, z, lengths):
    m.dec_prologue_cache = False
    try:
        out = m.decode(z, lengths)
        assert m._wcache[3].dec_pro in (None, 0)
        return out
    finally:
        m.dec_prologue_cache = True


def _valid_finite(a, lengths):
    return all(bool(torch.isfinite(a[i, :n]).all()) for i, n in enumerate(lengths))


def _valid_equal(a, b, lengths):
    return all(torch.equal(a[i, :n], b[i, :n]) for i, n in enumerate(lengths))


# ----------------------------------------------------------------------------- cached against uncached prologue
@pytest.mark.parametrize("lengths,F", [([16], 132), ([33, 17, 1], 132), ([257, 40], 75), ([5, 3], 132)])
def test_cached_prologue_equals_uncached(dev, lengths, F):
    """Smallest T on the one-kernel-per-layer path; ragged masks over the shared inputs; Sp = 512; and T = 5, which runs the
    three-kernels-per-layer sequence and must ignore the buffer it is handed."""
    T = max(lengths)
    m = _vae(dev, F)
    z = _z(dev, len(lengths), 100 + T)
    cached = m.decode(z, lengths)
    assert T in m._dec_pro and m._wcache[3].dec_pro_T == T
    again = m.decode(z, lengths)           # the first call built the entry, this one only reads it
    plain = _uncached(m, z, lengths)
    assert _valid_finite(cached, lengths)
    assert torch.equal(cached, plain) and torch.equal(again, plain)


# ----------------------------------------------------------------------------- keying by T
def test_cache_is_keyed_by_T(dev):
    m = _vae(dev, 132)
    z = _z(dev, 2, 7)
    plain = {T: _uncached(m, z, [T, T - 1]) for T in (33, 16)}
    for T in (33, 16, 33):
        assert torch.equal(m.decode(z, [T, T - 1]), plain[T]), T
    assert sorted(m._dec_pro) == [16, 33]


def test_cache_is_bounded(dev):
    m = _vae(dev, 132)
    z = _z(dev, 1, 8)
    for T in range(16, 25):                # nine distinct T
        out = m.decode(z, [T])
        assert len(m._dec_pro) <= 8 and T in m._dec_pro
        assert torch.equal(out, _uncached(m, z, [T])), T


# ----------------------------------------------------------------------------- invalidation
@pytest.mark.parametrize("which", ["pe", "in_proj"])
def test_cache_follows_the_weights(dev, which):
    m = _new_vae(dev, 132)
    z, lengths = _z(dev, 2, 9), [33, 20]
    before = m.decode(z, lengths)
    assert 33 in m._dec_pro
    p = m.query_pos_decoder.pe if which == "pe" else m.decoder.input_blocks[0].self_attn.in_proj_weight
    with torch.no_grad():
        p.add_(0.01)
    after = m.decode(z, lengths)
    assert torch.equal(after, _uncached(m, z, lengths))
    assert not _valid_equal(after, before, lengths)


def test_cache_survives_a_precision_round_trip(dev):
    m = _new_vae(dev, 132)
    z, lengths = _z(dev, 2, 10), [33, 20]
    first = m.decode(z, lengths)
    m.precision = "fp32"
    f32 = m.decode(z, lengths)
    assert _valid_finite(f32, lengths)
    assert not m._dec_pro                  # the fp32 path has no such buffer, and the fp16 image's entries went with it
    m.precision = "fp16"
    second = m.decode(z, lengths)
    assert torch.equal(first, second) and torch.equal(second, _uncached(m, z, lengths))


# ----------------------------------------------------------------------------- in-layer against launched cvec
def test_in_layer_vector_equals_launched_vector(dev):
    """T = 196: B = 40 is 280 workgroups (4 waves, the vector from the k_linear_h launch); 20 + 20 is 140 each (8 waves, the
    vector formed in the layer)."""
    T, B = 196, 40
    m = _vae(dev, 132)
    z = _z(dev, B, 11)
    lengths = [T - 9 * (i % 20) for i in range(B)]    # ragged, and each half holds a full-length sequence
    big = m.decode(z, lengths)
    assert _valid_finite(big, lengths)
    for lo in (0, 20):
        small = m.decode(z[:, lo:lo + 20].contiguous(), lengths[lo:lo + 20])
        for j, n in enumerate(lengths[lo:lo + 20]):
            assert torch.equal(big[lo + j, :n], small[j, :n]), lo + j


def test_single_sequence_equals_its_row_in_a_batch(dev):
    m = _vae(dev, 132)
    z = _z(dev, 3, 12)
    batch = m.decode(z, [16, 16, 16])
    for b in range(3):
        assert torch.equal(batch[b], m.decode(z[:, b:b + 1].contiguous(), [16])[0]), b


def test_vector_of_zero_and_of_large_latents(dev):
    """z = 0: the vector is the bias alone.  A row scaled by 50 next to a row of N(0,1): no row sees its neighbour."""
    m = _vae(dev, 132)
    z = _z(dev, 3, 13)
    z[0, 0] = 0.0
    z[0, 1] *= 50.0
    batch = m.decode(z, [16, 16, 16])
    assert bool(torch.isfinite(batch).all())
    for b in range(3):
        assert torch.equal(batch[b], m.decode(z[:, b:b + 1].contiguous(), [16])[0]), b
    assert not torch.equal(batch[0], batch[2])


# ----------------------------------------------------------------------------- the oracle, both parts on
@pytest.mark.parametrize("F,L", [(132, 33), (75, 257)])
def test_decode_vs_oracle(dev, F, L):
    z, lengths = R.dec_case(F, L)
    ref = R.dec_reference(F, L)
    m = _vae(dev, F)
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    m.decode(zt, list(lengths))                       # builds the entry
    got = m.decode(zt, list(lengths)).cpu().numpy()   # reads it
    assert (L + 2) in m._dec_pro and got.shape == ref.shape
    errs = [R.seq_err(got[b, :n], ref[b, :n]) for b, n in enumerate(lengths)]
    print(f"GLUE dec F={F} L={L}: err seq0 {errs[0]:.3e} seq1 {errs[1]:.3e}")
    assert all(np.isfinite(e) and e < TOL_DEC for e in errs)


# ----------------------------------------------------------------------------- graph capture
def test_capture_neither_builds_nor_misses_the_cache(dev):
    T, lengths = 24, [24, 11]
    m = _vae(dev, 132)
    z = _z(dev, 2, 14)
    eager = _uncached(m, z, lengths).clone()          # also warms the lengths tensor, the workspace and the weight image
    torch.cuda.synchronize()
    assert T not in m._dec_pro
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.decode(z, lengths)
    assert T not in m._dec_pro
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(m.decode(z, lengths), eager) and T in m._dec_pro
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        out2 = m.decode(z, lengths)
    assert m._wcache[3].dec_pro == m._dec_pro[T].data_ptr()
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out2, eager)
