"""The premises of tests/test_gpu_vae_edges.py, checked with the float64 oracle alone (no GPU): every loud encoder case of
tests/vae_edges_reference.py moves by at least 5e-2 when sequence 0's length is one off, the same shapes with quiet N(0,1) inputs
move by less than the 2e-2 the fp16 VAE tests used to allow, and the decoder's own sensitivity per length.

Decoder sensitivity (min over L - 1 and L + 1 of the change of sequence 0's frames < L - 1), as test_decoder_sensitivity_recorded
prints it.  Only the lengths up to 33 can carry a discrimination check in the GPU file:

      L      1       2       3       4       14      15      16      17      31      32      33      63      64      65      255     256     257     300     496
  F = 75   2.0e-1  1.7e-1  6.6e-2  7.4e-2  2.5e-2  2.3e-2  2.6e-2  2.0e-2  1.0e-2  1.6e-2  1.2e-2  5.1e-3  4.2e-3  5.5e-3  1.1e-3  1.4e-3  1.3e-3  2.0e-3  4.6e-4
  F = 132  2.0e-1  1.7e-1  1.0e-1  8.2e-2  2.3e-2  2.5e-2  2.3e-2  1.8e-2  1.3e-2  1.6e-2  1.2e-2  3.8e-3  4.2e-3  5.5e-3  9.8e-4  1.7e-3  1.3e-3  2.0e-3  4.7e-4
  F = 144, L = 17: 1.8e-2
"""
import numpy as np
import pytest

import vae_edges_reference as R

OLD_FP16_BOUND = 2e-2      # what every fp16 VAE assertion of tests/test_gpu_parity.py allowed before the edge tests


def test_case_tables_cover_the_listed_lengths():
    assert set(R.ENC_TABLE) == {(F, L) for F in R.ENC_FEATS for L in R.ENC_LENGTHS}
    assert all(4 <= scale <= 10 for _, scale in R.ENC_TABLE.values())
    assert max(R.ENC_LENGTHS) + 4 == 500 and max(R.DEC_LENGTHS) + 2 <= 500      # the learned position table has 500 rows
    assert {F for F, _ in R.DEC_CASES} == {75, 132, 144}


@pytest.mark.parametrize("F,L", sorted(R.ENC_TABLE))
def test_loud_edge_moves_the_oracle(F, L):
    """Dropping the last valid key or admitting the first pad key moves sequence 0's [mu, logvar] by at least 5e-2 in float64."""
    seed, scale = R.ENC_TABLE[(F, L)]
    x, lengths = R.enc_case(F, L)
    assert x.shape == (2, L + 2, F) and lengths == [L, L + 2] and x.dtype == np.float32
    quiet, _ = R.enc_case(F, L, quiet=True)
    loud = np.zeros(x.shape[:2], bool)
    loud[0, L - 1:L + 1] = True                                       # the last valid frame and the first pad frame, nothing else
    assert np.array_equal(x[~loud], quiet[~loud]) and np.array_equal(x[loud], quiet[loud] * np.float32(scale))
    ref = R.enc_reference(F, L)
    assert ref.shape == (2, 2, 256) and ref.dtype == np.float64 and np.isfinite(ref).all()
    d, a = R.sens_drop(F, L, seed, scale), R.sens_admit(F, L, seed, scale)
    print(f"encoder F={F} L={L} seed={seed} scale={scale}: sens_drop {d} sens_admit {a}")
    assert (d is None) == (L == 1)
    assert R.enc_sens(F, L) == (a if d is None else min(d, a)) >= R.SENS_MIN


@pytest.mark.parametrize("F", R.ENC_FEATS)
@pytest.mark.parametrize("L", [254, 300])
def test_quiet_inputs_hide_a_one_key_mistake(F, L):
    """The gap: on N(0,1) inputs of the same shape both sensitivities are below 2e-2, so no bound of that size could see the mistake."""
    seed, _ = R.ENC_TABLE[(F, L)]
    d, a = R.sens_drop(F, L, seed, 1.0), R.sens_admit(F, L, seed, 1.0)
    print(f"quiet encoder F={F} L={L}: sens_drop {d:.3e} sens_admit {a:.3e}")
    assert 0 < d < OLD_FP16_BOUND and 0 < a < OLD_FP16_BOUND


def test_neighbour_does_not_move():
    """Sequence 1 (full length) is the same whatever sequence 0's length is: the per-sequence errors are not diluted and not shared."""
    F, L = 75, 14
    x, lengths = R.enc_case(F, L)
    ref = R.enc_reference(F, L)
    for l0 in (L - 1, L + 1):
        assert R.seq_err(R.enc_oracle(F, x, [l0, lengths[1]])[:, 1], ref[:, 1]) < 1e-12


@pytest.mark.parametrize("F,L", R.DEC_CASES)
def test_decoder_sensitivity_recorded(F, L):
    """The decoder has no input that makes a key loud: its sensitivity falls with the length.  Recorded; asserted only up to L = 33."""
    z, lengths = R.dec_case(F, L)
    ref = R.dec_reference(F, L)
    assert z.shape == (1, 2, 256) and lengths == [L, L + 2] and ref.shape == (2, L + 2, F) and np.isfinite(ref).all()
    s = R.dec_sens(F, L)
    print(f"decoder F={F} L={L}: dec_sens {s:.3e}")
    if L <= 33:
        assert s >= 1e-2
