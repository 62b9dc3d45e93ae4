"""The interactee track on the CPU: the plain-torch twins of seeme_amd/track.py in float64 against the explicit loops of
tests/track_reference.py, the properties of the fill-and-filter definition (constant motion, -q keys, bitwise copy, holds, jitter),
the path of ``track_interactee`` against exhaustive enumeration, sparse recordings and the validation of keys and arguments."""
import os

import numpy as np
import pytest
import torch

import recording_reference as REF
import track_reference as TR
from conftest import REPO


def _t(x):
    return None if x is None else torch.from_numpy(np.asarray(x, np.float64))


def _filter64(pose, transl, idx, L, taps):
    from seeme_amd.track import track_filter_torch
    out, tout = track_filter_torch(_t(pose), _t(transl), np.asarray(idx), L, taps)
    assert out.dtype == torch.float64 and out.shape == (L, pose.shape[1], 3)
    return out.numpy(), None if tout is None else tout.numpy()


# ----------------------------------------------------------------------------- 1. the twins against the loops
@pytest.mark.parametrize("LfS", [(2, 1), (3, 2), (4, 5)], ids=str)
def test_track_cost_twin_equals_the_loops(LfS):
    from seeme_amd.track import track_cost_torch
    Lf, S = LfS
    g = np.random.default_rng(Lf * 10 + S)
    jts = g.standard_normal((Lf, S, 24, 3))
    idx = np.cumsum(g.choice([1, 2, 7], Lf))
    want = TR.track_cost_loops(jts, idx, 1250.0)
    got = track_cost_torch(_t(jts), idx, 1250.0)
    assert got.shape == (Lf - 1, S, S) and np.abs(got.numpy() - want).max() <= 1e-12 * want.max()
    assert track_cost_torch(_t(jts[:1]), idx[:1], 1.0).shape == (0, S, S)


FILTER_CASES = [("apart", [0, 2, 3, 6, 8], 9, [1.0]), ("apart", [0, 2, 3, 6, 8], 9, [1.0, 0.6, 0.1]), ("apart", [3, 4, 9], 14, [0.7, 0.7]),
                ("smooth", [0, 5, 6, 11], 12, [1.0, 0.5]), ("apart", [0], 1, [1.0, 0.5]), ("smooth", [2, 4], 9, [2.0] + [0.25] * 32)]


@pytest.mark.parametrize("case", FILTER_CASES, ids=lambda c: f"{c[0]}-{c[2]}-R{len(c[3]) - 1}")
def test_track_filter_twin_equals_the_loops(case):
    kind, idx, L, taps = case
    J = 4
    pose, tr = TR.keys_apart(len(idx), J, seed=L) if kind == "apart" else TR.smooth_keys(idx, L, J, seed=L)
    Mw, Tw, Aw = TR.track_filter_loops(pose, tr, idx, L, taps)
    out, tout = _filter64(pose, tr, idx, L, taps)
    assert np.abs(TR.matrices(out) - Mw).max() <= 1e-12 and np.abs(tout - Tw).max() <= 1e-12
    assert np.abs(out - Aw).max() <= 1e-12                             # (angles well below pi: the axis-angle itself agrees too)
    out2, none = _filter64(pose, None, idx, L, taps)
    assert none is None and np.array_equal(out2, out)


# ----------------------------------------------------------------------------- 2. properties of the definition
def test_constant_motion_comes_out_unchanged():
    g = np.random.default_rng(0)
    one = 0.8 * g.standard_normal((1, 6, 3))
    idx = [1, 4, 5, 11]
    pose = np.repeat(one, len(idx), axis=0)
    tr = np.repeat(g.standard_normal((1, 3)), len(idx), axis=0)
    for taps in ([1.0], [1.0, 0.5, 0.25]):
        out, tout = _filter64(pose, tr, idx, 14, taps)
        assert np.abs(TR.matrices(out) - TR.matrices(one)).max() <= 1e-12 and np.abs(tout - tr[:1]).max() <= 1e-12


def test_minus_q_keys_give_the_same_rotations():
    idx, L = [0, 2, 3, 6, 8], 9
    pose, tr = TR.keys_apart(len(idx), 5, seed=4)
    flipped = TR.flip_alternate(pose)
    assert np.abs(TR.matrices(flipped) - TR.matrices(pose)).max() <= 1e-12 and np.abs(flipped - pose).max() > 1.0
    for taps in ([1.0], [1.0, 0.6, 0.2]):
        a, _ = _filter64(pose, tr, idx, L, taps)
        b, _ = _filter64(flipped, tr, idx, L, taps)
        assert np.abs(TR.matrices(a) - TR.matrices(b)).max() <= 1e-12


def test_without_a_filter_keys_are_copied_bit_for_bit_and_the_ends_hold():
    from seeme_amd.track import track_filter_torch
    idx, L = [3, 4, 9, 10], 14                                          # first key at 3, last key at L - 4
    pose, tr = TR.keys_apart(len(idx), 5, seed=6)
    p32, t32 = torch.from_numpy(pose).float(), torch.from_numpy(tr).float()
    out, tout = track_filter_torch(p32, t32, idx, L, [1.0])
    assert out.dtype == torch.float32 and torch.equal(out[idx], p32) and torch.equal(tout[idx], t32)
    out2, tout2 = track_filter_torch(p32, t32, idx, L, [0.37])          # any single tap
    assert torch.equal(out2[idx], p32) and torch.equal(tout2[idx], t32)
    o64, t64 = _filter64(pose, tr, idx, L, [1.0])
    assert np.abs(TR.matrices(o64[:3]) - TR.matrices(pose[:1])).max() <= 1e-12 and np.abs(t64[:3] - tr[:1]).max() <= 1e-12
    assert np.abs(TR.matrices(o64[10:]) - TR.matrices(pose[-1:])).max() <= 1e-12 and np.abs(t64[10:] - tr[-1:]).max() <= 1e-12
    # with a filter nothing is copied: a key between two different neighbours moves
    o3, _ = _filter64(pose, tr, idx, L, [1.0, 0.5])
    assert np.abs(TR.matrices(o3[4]) - TR.matrices(pose[1])).max() > 1e-3
    # taps [1, 0, 0] are no filter, in matrices
    oz, tz = _filter64(pose, tr, idx, L, [1.0, 0.0, 0.0])
    assert np.abs(TR.matrices(oz) - TR.matrices(o64)).max() <= 1e-12 and np.abs(tz - t64).max() <= 1e-12


@pytest.mark.parametrize("sigma", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("L", [24, 48])
def test_filter_removes_jitter(L, sigma):
    """Mean absolute second difference of the rotation matrices: the output's is at most 0.5 of the input's (a float64 prototype of
    the definition gave 0.08-0.21 on these inputs; the Gaussian's noise gain alone is 0.53 at sigma 1 before differencing, so 0.5
    leaves room without letting an identity filter pass)."""
    from seeme_amd.track import gaussian_taps
    _smooth, noisy = TR.jitter_motion(L, seed=L)
    out, _ = _filter64(noisy, None, np.arange(L), L, gaussian_taps(sigma))
    ratio = TR.second_difference(TR.matrices(out)) / TR.second_difference(TR.matrices(noisy))
    print(f"jitter L {L} sigma {sigma}: second-difference ratio {ratio:.3f}")
    assert ratio <= 0.5, ratio


def test_gaussian_taps():
    from seeme_amd.track import gaussian_taps
    assert gaussian_taps(0).tolist() == [1.0] and gaussian_taps(0).dtype == np.float32
    t = gaussian_taps(2.0)
    assert t.shape == (7,) and t.dtype == np.float32 and t[0] == 1.0
    assert np.array_equal(t, np.exp(-np.arange(7.0) ** 2 / 8.0).astype(np.float32))
    assert gaussian_taps(10.0).shape == (31,) and gaussian_taps(0.5).shape == (3,)
    for bad in (-1.0, 10.5, float("nan"), "2", None, True):
        with pytest.raises(ValueError, match="sigma"):
            gaussian_taps(bad)


# ----------------------------------------------------------------------------- 3. the track
@pytest.fixture(scope="module")
def smpl():
    from seeme_amd.smpl import SMPL
    return SMPL.synthetic(1234, V=64).double()


@pytest.mark.parametrize("prior_weight", [0.0, 1.0])
def test_track_path_equals_enumeration(smpl, prior_weight):
    from seeme_amd.track import track_interactee
    from seeme_amd.vae_autograd import smpl_joints_torch
    Lf, S, L = 4, 3, 9
    idx = np.array([0, 2, 3, 8])
    go, bp, tr, lp = (_t(x) for x in TR.candidates(Lf, S, seed=11))
    betas = _t(0.3 * np.random.default_rng(1).standard_normal(10))
    out = track_interactee(go, bp, tr, lp, idx, L, smpl, betas, step_mm=20.0, prior_weight=prior_weight, sigma=1.0)
    assert out["global_orient"].shape == (L, 3) and out["body_pose"].shape == (L, 69) and out["transl"].shape == (L, 3)
    assert out["path"].shape == (Lf,) and out["path"].dtype == torch.int64 and out["step_cost"].shape == (Lf - 1,)
    # the costs are those of the joints of every candidate; the unary term is the flow's density relative to the mode
    pose = torch.cat([go, bp], dim=-1).reshape(Lf * S, 72)
    jts = smpl_joints_torch(smpl, betas[None].expand(Lf * S, 10), pose, tr[:, None].expand(Lf, S, 3).reshape(-1, 3)).reshape(Lf, S, 24, 3)
    cost = TR.track_cost_loops(jts.numpy(), idx, 1e6 / (2 * 20.0 ** 2))
    assert np.abs(out["cost"].numpy() - cost).max() <= 1e-12 * cost.max()
    unary = prior_weight * (lp[:, :1] - lp).numpy()
    assert (unary >= 0).all() and np.abs(out["unary"].numpy() - unary).max() <= 1e-12
    low, arg = REF.best_path_enumerate(cost, unary, Lf, S)
    assert out["path"].tolist() == arg and abs(float(out["path_cost"]) - low) <= 1e-12 * low
    assert np.abs(out["step_cost"].numpy() - np.array([cost[l, arg[l], arg[l + 1]] for l in range(Lf - 1)])).max() <= 1e-12 * cost.max()
    # ... and the motion is the filter of the chosen rows
    from seeme_amd.track import gaussian_taps
    keys = np.concatenate([go.numpy(), bp.numpy()], axis=-1)[np.arange(Lf), arg].reshape(Lf, 24, 3)
    Mw, Tw, _ = TR.track_filter_loops(keys, tr.numpy(), idx, L, gaussian_taps(1.0))
    got = torch.cat([out["global_orient"], out["body_pose"]], dim=-1).reshape(L, 24, 3).numpy()
    assert np.abs(TR.matrices(got) - Mw).max() <= 1e-12 and np.abs(out["transl"].numpy() - Tw).max() <= 1e-12


# ----------------------------------------------------------------------------- 4. sparse recordings
def _estimate_input(n=9, H=12, W=16):
    g = np.random.default_rng(2)
    return {"video": g.integers(0, 256, (n, H, W, 3), dtype=np.uint8), "center": g.uniform(4, 10, (n, 2)).astype(np.float32),
            "scale": g.uniform(0.02, 0.04, n).astype(np.float32), "cam_intrinsics": np.array([20.0, 8.0, 6.0], np.float32),
            "world2cam": np.tile(np.eye(4), (n, 1, 1)), "scene_vertices": g.normal(size=(50, 3)).astype(np.float32)}


def test_load_recording_allow_sparse(tmp_path):
    from seeme_amd import recording as R
    path = str(tmp_path / "rec.npz")
    d = _estimate_input()
    stored = np.array([0, 2, 3, 6, 8])
    np.savez(path, **dict(d, video=d["video"][stored], video_index=stored))
    rec = R.load_recording(path, require_interactee=False, allow_sparse=True)
    assert rec["n_frames"] == 9 and np.array_equal(rec["video_index"], stored) and rec["video"].shape[0] == 5
    assert rec["center"].shape == (9, 2) and rec["scale"].shape == (9,) and rec["cam_intrinsics"].shape == (9, 3)
    assert rec["world2cam"].shape == (9, 4, 4)
    with pytest.raises(ValueError, match="frame 1 has no stored image.*filling between sparse estimates is not built"):
        R.load_recording(path, require_interactee=False)               # the default keeps its error
    np.savez(path, **dict(d, video=d["video"][stored], video_index=stored[::-1].copy()))
    with pytest.raises(ValueError, match="strictly increasing"):
        R.load_recording(path, require_interactee=False, allow_sparse=True)
    np.savez(path, **d)                                                 # a dense recording loads either way
    assert R.load_recording(path, require_interactee=False, allow_sparse=True)["n_frames"] == 9


# ----------------------------------------------------------------------------- 5. validation
def test_track_config_keys_are_validated():
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    path = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    smpl = SMPL.synthetic(1, V=64)
    m = MLD(parse_config(path), SyntheticEgoDataModule(), smpl_model=smpl)
    assert (m.track_step_mm, m.track_prior_weight, m.track_sigma) == (20.0, 1.0, 2.0)
    bad = {"TRACK_STEP_MM": (0, -1.0, float("inf"), "20", None, True), "TRACK_PRIOR_WEIGHT": (-0.5, float("nan"), "1", None, False),
           "TRACK_SIGMA": (-1, 10.5, float("nan"), "2", None, True)}
    for key, values in bad.items():
        for v in values:
            cfg = parse_config(path)
            cfg.TEST[key] = v
            with pytest.raises(ValueError, match=f"TEST.{key}"):
                MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    cfg = parse_config(path)
    cfg.TEST.TRACK_STEP_MM, cfg.TEST.TRACK_PRIOR_WEIGHT, cfg.TEST.TRACK_SIGMA = 35, 0, 0
    m = MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    assert (m.track_step_mm, m.track_prior_weight, m.track_sigma) == (35.0, 0.0, 0.0)


def test_bad_idx_and_taps_name_themselves():
    from seeme_amd.track import check_idx, track_cost_torch, track_filter_torch
    pose = torch.zeros(3, 2, 3, dtype=torch.float64)
    for idx in ([0, 2, 2], [2, 1, 3], [-1, 0, 1], [0, 1, 9], [0.0, 1.0, 2.0], [[0, 1, 2]], [0, 1]):
        with pytest.raises(ValueError, match="idx"):
            track_filter_torch(pose, None, np.asarray(idx), 9, [1.0])
    with pytest.raises(ValueError, match="idx"):
        track_cost_torch(torch.zeros(3, 2, 24, 3), np.array([0, 3, 3]), 1.0)
    with pytest.raises(ValueError, match="idx"):
        check_idx(np.zeros(0, np.int64), 4)
    assert check_idx(torch.tensor([0, 3, 8]), 9).tolist() == [0, 3, 8]
    for taps in ([0.0, 1.0], [1.0, -0.1], [1.0, float("nan")], [], [1.0] * 34):
        with pytest.raises(ValueError, match="tap"):
            track_filter_torch(pose, None, np.array([0, 1, 2]), 9, taps)

