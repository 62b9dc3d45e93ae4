"""The headset's own path on the CPU: the plain-torch twins of seeme_head_path_cost / seeme_head_anchor in float64 against the explicit
loops of tests/headset_reference.py, the host-side helpers (camera centres, the path cut into windows), the head_path key of a
recording and the C-ABI of the two entry points."""
import os

import numpy as np
import pytest
import torch

import headset_reference as HREF
from seeme_amd import recording as R
from seeme_amd.track import gaussian_taps

TWIN_TOL = 1e-12             # float64 twin against float64 loops, relative to the largest reference value
COST_CASES = [(1, 1, 1), (2, 3, 2), (3, 32, 5), (2, 5, 63), (2, 5, 65), (4, 33, 9)]
ANCHOR_CASES = [(L_, s) for L_ in (1, 2, 7, 64, 65, 300) for s in (0, 0.5, 2, 10)]


def _close(got, want):
    got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64
    return float(np.abs(got - want).max()) <= TWIN_TOL * max(float(np.abs(want).max()), 1e-300)


# ----------------------------------------------------------------------------- the twins against the loops
@pytest.mark.parametrize("shape", COST_CASES, ids=str)
def test_head_path_cost_twin_vs_float64_loops(shape):
    W, K, T = shape
    jts, path = (torch.from_numpy(a).double() for a in HREF.cost_inputs(W, K, T))
    for lengths in HREF.cost_lengths(W, T):
        want = HREF.head_path_cost(jts.numpy(), path.numpy(), lengths)
        got = R.head_path_cost_torch(jts, path, lengths)
        assert _close(got, want), (lengths, got, want)
        for w, n in enumerate(lengths):
            if n <= 1:
                assert float(got[w].abs().max()) == 0.0                # n = 0 and n = 1: exactly 0
            elif K > 1:
                assert float(got[w].min()) > 10.0                      # 0.1 m of noise: deviations far above rounding
        # frames past the length and joints other than the head take no part; a tensor of lengths is read like a list
        poisoned = jts.clone()
        keep = torch.zeros(W, K, T, 24, dtype=torch.bool)
        for w, n in enumerate(lengths):
            keep[w, :, :n, HREF.HEAD] = True
        poisoned[~keep] = float("nan")
        assert torch.equal(R.head_path_cost_torch(poisoned, path, torch.tensor(lengths)), got)
    assert torch.equal(R.head_path_cost_torch(jts, path, [T + 5] * W), R.head_path_cost_torch(jts, path, [T] * W))   # a length above T is T


def test_head_path_cost_is_blind_to_a_constant_offset_and_sees_the_shape():
    W, K, T = 2, 4, 12
    jts, path = (torch.from_numpy(a).double() for a in HREF.cost_inputs(W, K, T))
    lengths = [T, T - 3]
    for k in range(K):                                                 # hypothesis k: the path plus a constant of its own
        jts[:, k, :, HREF.HEAD] = path + torch.tensor([0.1 * k, -0.3, 0.05 * k], dtype=torch.float64)
    assert float(R.head_path_cost_torch(jts, path, lengths).abs().max()) <= 1e-9
    jts[1, 2, 4, HREF.HEAD, 0] += 0.5                                  # one frame half a metre off: (2 (n-1) / n^2) x 500 mm
    got = R.head_path_cost_torch(jts, path, lengths)
    n = lengths[1]
    assert abs(float(got[1, 2]) - 1000.0 * 0.5 * 2 * (n - 1) / n ** 2) <= 1e-9 and float(got[0].abs().max()) <= 1e-9


@pytest.mark.parametrize("case", ANCHOR_CASES, ids=str)
def test_head_anchor_twin_vs_float64_loops(case):
    L_, sigma = case
    joints, path = (torch.from_numpy(a).double() for a in HREF.anchor_inputs(L_))
    taps = gaussian_taps(sigma)
    want_s, want_r = HREF.head_anchor(joints.numpy(), path.numpy(), taps)
    shift, residual = R.head_anchor_torch(joints, path, taps)
    assert _close(shift, want_s) and (sigma == 0 or L_ == 1 or _close(residual, want_r))
    if sigma == 0 or L_ == 1:                                          # taps [1], or nothing but the frame itself inside the window
        assert torch.equal(shift, path - joints[:, HREF.HEAD]) and float(residual.abs().max()) == 0.0


def test_head_anchor_renormalises_at_the_two_ends():
    L_ = 40
    joints, _ = (torch.from_numpy(a).double() for a in HREF.anchor_inputs(L_))
    const = torch.tensor([0.25, -1.5, 0.75], dtype=torch.float64)
    path = joints[:, HREF.HEAD] + const
    for sigma in (0.5, 2, 10):                                         # R = 30 reaches past both ends of 40 frames
        shift, residual = R.head_anchor_torch(joints, path, gaussian_taps(sigma))
        assert float((shift - const).abs().max()) <= 1e-12 and float(residual.max()) <= 1e-9
    with pytest.raises(ValueError, match="tap"):
        R.head_anchor_torch(joints, path, [0.0, 1.0])
    with pytest.raises(ValueError, match="expected"):
        R.head_anchor_torch(joints, path[:-1], [1.0])
    long = np.exp(-np.arange(41.0) ** 2 / 200.0)                       # the twin serves any R
    assert float((R.head_anchor_torch(joints, path, long)[0] - const).abs().max()) <= 1e-12


# ----------------------------------------------------------------------------- host-side helpers
def _rigid(g):
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = q, 3.0 * g.standard_normal(3)
    return M


def test_camera_centres_are_the_translations_of_the_inverse_maps():
    g = np.random.default_rng(3)
    M = np.stack([_rigid(g) for _ in range(9)])
    c = R.camera_centres(M)
    assert c.shape == (9, 3) and c.dtype == np.float64
    assert float(np.abs(c - np.linalg.inv(M)[:, :3, 3]).max()) <= 1e-12
    assert float(np.abs(np.einsum("nij,nj->ni", M[:, :3, :3], c) + M[:, :3, 3]).max()) <= 1e-12     # the centre maps to the origin
    with pytest.raises(ValueError, match="world2cam"):
        R.camera_centres(M[0])


def test_head_path_windows_are_the_slices_of_the_window_plan():
    n, T, O = 37, 16, 4
    path = torch.from_numpy(np.random.default_rng(4).standard_normal((n, 3)))
    starts, lengths = R.window_plan(n, T, O)
    assert lengths[-1] == 13                                           # a short last window
    pw = R.head_path_windows(path, starts, lengths, T)
    assert pw.shape == (len(starts), T, 3) and pw.dtype == torch.float64
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        assert torch.equal(pw[w, :ln], path[lo:lo + ln]) and float(pw[w, ln:].abs().max() if ln < T else 0.0) == 0.0
    again = R.head_path_windows(path.float().numpy(), starts, lengths, T)                           # an array is read like a tensor
    assert again.dtype == torch.float32 and torch.equal(again, pw.float())
    one = R.head_path_windows(path[:5], [0], [5], 5)                   # a lone window shorter than T comes back cut to its length
    assert torch.equal(one[0], path[:5])
    with pytest.raises(ValueError, match="does not fit"):
        R.head_path_windows(path[:30], starts, lengths, T)
    with pytest.raises(ValueError, match="expected"):
        R.head_path_windows(path.reshape(-1), starts, lengths, T)


# ----------------------------------------------------------------------------- the recording file
def _recording(n, g):
    return {"global_orient": g.standard_normal((n, 3)).astype(np.float32), "body_pose": g.standard_normal((n, 69)).astype(np.float32),
            "transl": g.standard_normal((n, 3)).astype(np.float32), "betas": g.standard_normal(10).astype(np.float32)}


def test_load_recording_accepts_or_refuses_head_path(tmp_path):
    g = np.random.default_rng(5)
    n = 9
    rec = _recording(n, g)
    hp = g.standard_normal((n, 3))

    def save(name, extra):
        p = os.path.join(tmp_path, name)
        np.savez(p, **rec, **extra)
        return p

    assert "head_path" not in R.load_recording(save("none.npz", {}))
    for arr in (hp, hp.astype(np.float32)):                            # a recording in one fixed frame: no world2cam needed
        got = R.load_recording(save("good.npz", {"head_path": arr}))
        assert got["head_path"].dtype == np.float64 and np.array_equal(got["head_path"], arr.astype(np.float64))
    w2c = np.stack([_rigid(g) for _ in range(n)])
    both = R.load_recording(save("both.npz", {"head_path": hp, "world2cam": w2c}))                  # head_path stands beside world2cam
    assert np.array_equal(both["head_path"], hp) and np.array_equal(both["world2cam"], w2c)
    nan = hp.copy()
    nan[4, 1] = np.nan
    for name, bad in (("short", hp[:-1]), ("wide", np.zeros((n, 4))), ("nan", nan), ("inf", np.where(nan != nan, np.inf, nan)),
                      ("int", np.zeros((n, 3), np.int64)), ("bool", np.zeros((n, 3), bool))):
        with pytest.raises(ValueError, match="head_path"):
            R.load_recording(save(name + ".npz", {"head_path": bad}))


# ----------------------------------------------------------------------------- the C-ABI
def test_headset_entry_points_are_declared_bound_and_exported():
    import ctypes
    from conftest import REPO
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("seeme_head_path_cost", "seeme_head_anchor"):
        assert f"{name}(" in hdr and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert f"SEEME_HEAD_JOINT {R.HEAD_JOINT}\n" in hdr and f"SEEME_HEAD_ANCHOR_RMAX {R.HEAD_ANCHOR_RMAX}\n" in hdr
    assert gaussian_taps(10.0).shape[0] - 1 == R.HEAD_ANCHOR_RMAX     # the widest filter check_sigma admits
    assert "headset.hip" in open(os.path.join(REPO, "seeme_amd", "csrc", "build.sh")).read()
    # the argument checks run on the host, before anything is launched
    L = _lib.lib()
    one = (ctypes.c_float * 1)(1.0)
    assert L.seeme_head_path_cost(None, None, None, 1, 1, 1, None, None) != 0 and b"null" in L.seeme_last_error()
    assert L.seeme_head_path_cost(64, 64, 64, 1, 33, 1, 64, None) != 0 and b"K must be" in L.seeme_last_error()
    assert L.seeme_head_path_cost(64, 64, 64, 0, 1, 1, 64, None) != 0 and b"W must be" in L.seeme_last_error()
    assert L.seeme_head_anchor(None, None, 1, one, 0, None, None, None) != 0 and b"null" in L.seeme_last_error()
    assert L.seeme_head_anchor(64, 64, 0, one, 0, 64, 64, None) != 0 and b"L must be" in L.seeme_last_error()
    assert L.seeme_head_anchor(64, 64, 1, one, 31, 64, 64, None) != 0 and b"R must be" in L.seeme_last_error()
