"""Edge cases for the VAE kernels (csrc/vae_h16.hip, csrc/vae_kernels.hip), built with the float64 oracle alone.  No GPU.

The fp16 path's index edges (key mask c < n_valid, K32 = ceil(n_valid / 32), NT16 = ceil(S / 16), the 4- or 8-column softmax, the
unfused sequence below 16 tokens) move a quiet N(0,1) sequence's output by a few 1e-3 when they are one key off: inside any bound
an fp16 path can be given.  The encoder cases here make the two frames at the mask's edge LOUD (the last valid frame and the first
pad frame of sequence 0, times `scale`), so that the oracle itself moves by more than 5e-2 when the length is one off: then a plain
comparison with the float64 oracle tells a one-key mistake from fp16 rounding.

All errors are per sequence: max|a - b| / max|b| over that sequence's rows only, so that the neighbour cannot dilute them.
tests/test_vae_edges_cpu.py holds the premises, tests/test_gpu_vae_edges.py uses the cases."""
import functools

import numpy as np

from oracle import mld_oracle as O
from seeme_amd import shapes
from seeme_amd.weights_recipe import recipe_state_dict

SENS_MIN = 5e-2        # every encoder case: the oracle moves by at least this much when sequence 0's length is one off

# Sequence 0 has n_valid = L + 2 keys and sequence 1 has S = L + 4 tokens (two prefix tokens): together they straddle the unfused /
# fused switch at 16 tokens, 16-key tiles, 32-key / 32-row blocks, the 64-column wave chunk, Sp 256 -> 512 and the 500-token limit.
# L = 3 and 4 (S = 7 and 8) straddle the size below which the unfused sequence keeps V^T in the packed-key region of the workspace.
ENC_LENGTHS = (1, 2, 3, 4, 13, 14, 15, 29, 30, 31, 61, 62, 63, 253, 254, 255, 256, 257, 300, 496)
ENC_FEATS = (75, 132)

# (F, L) -> (seed, scale); features come from default_rng(1000 * seed + L).  Found by enc_search() (scale 10 first, seed 0 first),
# except (132, 496): seed 0 meets the condition with 5.03e-2, seed 1 gives 0.63 and leaves room.  The smallest of the table is
# 7.1e-2 (F = 75, L = 13); test_vae_edges_cpu.py asserts the 5e-2 condition for every row.
ENC_TABLE = {
    (75, 1): (0, 10), (75, 2): (0, 10), (75, 3): (0, 10), (75, 4): (0, 10), (75, 13): (0, 10), (75, 14): (0, 10),
    (75, 15): (0, 10), (75, 29): (0, 10), (75, 30): (0, 10), (75, 31): (0, 10), (75, 61): (1, 10), (75, 62): (0, 10),
    (75, 63): (0, 10), (75, 253): (0, 10), (75, 254): (1, 10), (75, 255): (0, 10), (75, 256): (0, 10), (75, 257): (1, 10),
    (75, 300): (1, 10), (75, 496): (4, 10),
    (132, 1): (0, 10), (132, 2): (0, 10), (132, 3): (0, 10), (132, 4): (0, 10), (132, 13): (0, 10), (132, 14): (0, 10),
    (132, 15): (0, 10), (132, 29): (0, 10), (132, 30): (0, 10), (132, 31): (0, 10), (132, 61): (0, 10), (132, 62): (0, 10),
    (132, 63): (0, 10), (132, 253): (0, 10), (132, 254): (0, 10), (132, 255): (0, 10), (132, 256): (0, 10), (132, 257): (0, 10),
    (132, 300): (0, 10), (132, 496): (1, 10),
}

# the decoder has no prefix tokens: S = T = L + 2, the unfused sequence runs for T <= 15 (V^T in the packed-key region for T <= 5)
DEC_LENGTHS = (1, 2, 3, 4, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 496)
DEC_CASES = tuple((F, L) for F in (75, 132) for L in DEC_LENGTHS) + ((144, 17),)   # F = 144 (rot6d): N is a multiple of 16 in final_layer


@functools.lru_cache(maxsize=None)
def params(F):
    """float64 oracle parameters of the recipe model, built once and left unchanged."""
    return O.cast_params(recipe_state_dict(shapes.vae_shapes(F)), np.float64)


def seq_err(a, b):
    """max|a - b| / max|b| of ONE sequence's rows."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ----------------------------------------------------------------------------- encoder
def enc_features(F, L, seed, scale):
    """[2, L + 2, F] float32, lengths [L, L + 2]: N(0,1), frames L-1 and L of sequence 0 (last valid, first pad) times `scale`."""
    T = L + 2
    x = np.random.default_rng(1000 * seed + L).standard_normal((2, T, F)).astype(np.float32)
    x[0, L - 1:L + 1] *= np.float32(scale)
    return x, [L, T]


def enc_case(F, L, quiet=False):
    seed, scale = ENC_TABLE[(F, L)]
    return enc_features(F, L, seed, 1.0 if quiet else scale)


def enc_oracle(F, x, lengths):
    """[2, B, 256] float64: row 0 = mu, row 1 = logvar, as MldVae.encode_dist lays them out."""
    mu, std = O.vae_encode(params(F), np.asarray(x, np.float64), list(lengths))
    assert mu.dtype == np.float64
    return np.concatenate([mu, 2.0 * np.log(std)], axis=0)


@functools.lru_cache(maxsize=None)
def _enc_runs(F, L, seed, scale):
    x, lengths = enc_features(F, L, seed, scale)
    T = lengths[1]
    ref = enc_oracle(F, x, lengths)
    drop = seq_err(enc_oracle(F, x, [L - 1, T])[:, 0], ref[:, 0]) if L > 1 else None
    admit = seq_err(enc_oracle(F, x, [L + 1, T])[:, 0], ref[:, 0])
    ref.setflags(write=False)
    return ref, drop, admit


def enc_reference(F, L, quiet=False):
    """The oracle's [mu, logvar] of the case at its true lengths (shared, read-only)."""
    seed, scale = ENC_TABLE[(F, L)]
    return _enc_runs(F, L, seed, 1.0 if quiet else float(scale))[0]


def sens_drop(F, L, seed, scale):
    """rel_err of sequence 0's [mu, logvar] between oracle runs with lengths [L-1, T] and [L, T]; None at L = 1."""
    return _enc_runs(F, L, seed, float(scale))[1]


def sens_admit(F, L, seed, scale):
    """The same with [L+1, T]: the first pad key admitted."""
    return _enc_runs(F, L, seed, float(scale))[2]


def enc_sens(F, L, quiet=False):
    """min(sens_drop, sens_admit) of the table's case (sens_admit alone at L = 1)."""
    seed, scale = ENC_TABLE[(F, L)]
    scale = 1.0 if quiet else float(scale)
    d, a = sens_drop(F, L, seed, scale), sens_admit(F, L, seed, scale)
    return a if d is None else min(d, a)


def enc_search(F, L, seeds=range(8), scales=(10, 8, 6, 4)):
    """First (seed, scale) that meets SENS_MIN; how ENC_TABLE was made."""
    for scale in scales:
        for seed in seeds:
            d, a = sens_drop(F, L, seed, scale), sens_admit(F, L, seed, scale)
            if min(a, a if d is None else d) >= SENS_MIN:
                return seed, scale
    raise LookupError((F, L))


# ----------------------------------------------------------------------------- decoder
def dec_case(F, L):
    """z [1, 2, 256] float32 N(0,1), lengths [L, L + 2]."""
    z = np.random.default_rng(7000 + L).standard_normal((1, 2, 256)).astype(np.float32)
    return z, [L, L + 2]


def dec_common(L):
    """Frames of sequence 0 that are valid at lengths L - 1, L and L + 1 (frame 0 alone at L = 1, where only L + 1 is legal)."""
    return max(L - 1, 1)


@functools.lru_cache(maxsize=None)
def _dec_runs(F, L):
    z, lengths = dec_case(F, L)
    P, z64, n = params(F), z.astype(np.float64), dec_common(L)
    ref = O.vae_decode(P, z64, lengths)
    assert ref.dtype == np.float64
    drop = seq_err(O.vae_decode(P, z64, [L - 1, L + 2])[0, :n], ref[0, :n]) if L > 1 else None
    admit = seq_err(O.vae_decode(P, z64, [L + 1, L + 2])[0, :n], ref[0, :n])
    ref.setflags(write=False)
    return ref, drop, admit


def dec_reference(F, L):
    """The oracle's [2, L + 2, F] at lengths [L, L + 2] (shared, read-only); frames >= len are unspecified."""
    return _dec_runs(F, L)[0]


def dec_sens(F, L):
    """The oracle's change of frames < L - 1 of sequence 0 when its length is L - 1 or L + 1: the smaller of the two."""
    _, d, a = _dec_runs(F, L)
    return a if d is None else min(d, a)
