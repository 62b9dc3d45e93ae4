"""A whole recording on the CPU: the window plan, the plain-torch twins of seeme_amd/recording.py in float64 against the independent
restatements of tests/recording_reference.py (loops, exhaustive enumeration, rotation matrices), and the recording files."""
import os

import numpy as np
import pytest
import torch

import recording_reference as REF
from seeme_amd import recording as R

T8 = 8


# ----------------------------------------------------------------------------- window plan
@pytest.mark.parametrize("O", [0, 1, 3, 4])
def test_window_plan_covers_every_frame_with_exact_overlaps(O):
    for n in range(1, 3 * T8 + 1):
        starts, lengths = R.window_plan(n, T8, O)
        W = len(starts)
        assert W == len(lengths) and (starts, lengths) == REF.plan(n, T8, O)
        count = np.zeros(n, int)
        for lo, ln in zip(starts, lengths):
            assert 1 <= ln <= T8 and lo + ln <= n
            count[lo:lo + ln] += 1
        assert count.min() >= 1 and count.max() <= 2, (n, O)          # the union covers every frame; none lies in more than two
        assert all(ln == T8 for ln in lengths[:-1])                    # every window but the last is full
        if W > 1:
            assert lengths[-1] >= O + 1
        for w in range(W - 1):                                         # w and w+1 share the last O frames of w and the first O of w+1
            a = set(range(starts[w], starts[w] + lengths[w]))
            b = set(range(starts[w + 1], starts[w + 1] + lengths[w + 1]))
            assert a & b == set(range(starts[w + 1], starts[w + 1] + O)) == set(range(starts[w] + T8 - O, starts[w] + T8))
        assert int((count == 2).sum()) == (W - 1) * O


def test_window_plan_bad_arguments_raise():
    for args in ((10, 8, 5), (10, 8, -1), (0, 8, 2), (10, 0, 0), (10.0, 8, 2), (10, 8, True)):
        with pytest.raises(ValueError):
            R.window_plan(*args)
    assert R.window_plan(10, 8, 4) == ([0, 4], [8, 6])                  # 2*O = T is allowed


# ----------------------------------------------------------------------------- path
def _costs(W, K, seed, with_unary):
    g = torch.Generator().manual_seed(seed)
    cost = 50.0 * torch.rand(max(W - 1, 0), K, K, generator=g, dtype=torch.float64)
    unary = 30.0 * torch.rand(W, K, generator=g, dtype=torch.float64) if with_unary else None
    return cost, unary


@pytest.mark.parametrize("with_unary", [False, True])
@pytest.mark.parametrize("WK", [(4, 3), (5, 2), (1, 4), (3, 1)], ids=str)
def test_path_select_twin_finds_the_enumerated_minimum(WK, with_unary):
    W, K = WK
    cost, unary = _costs(W, K, 3 + W * 10 + K, with_unary)
    got = R.path_select_torch(cost, unary)
    path = got["path"].tolist()
    assert got["path"].dtype == torch.int64 and len(path) == W and got["seam_cost"].shape == (W - 1,)
    low, arg = REF.best_path_enumerate(cost.numpy(), None if unary is None else unary.numpy(), W, K)
    mine = REF.path_total(cost.numpy(), None if unary is None else unary.numpy(), path)
    assert abs(mine - low) <= 1e-12 * max(abs(low), 1e-300), (mine, low, path, arg)
    assert abs(float(got["path_cost"]) - mine) <= 1e-12 * max(abs(mine), 1.0)
    for w in range(W - 1):
        assert float(got["seam_cost"][w]) == float(cost[w, path[w], path[w + 1]])


@pytest.mark.parametrize("with_unary", [False, True])
def test_path_select_twin_ties_go_to_the_lowest_index(with_unary):
    W, K = 5, 4
    cost = torch.full((W - 1, K, K), 2.5, dtype=torch.float64)
    unary = torch.full((W, K), 1.25, dtype=torch.float64) if with_unary else None
    assert R.path_select_torch(cost, unary)["path"].tolist() == [0] * W
    # and a tie between two complete paths: the lowest final index, then the lowest predecessor
    cost = torch.ones(1, 3, 3, dtype=torch.float64)
    cost[0, 2, 1] = cost[0, 1, 1] = cost[0, 1, 2] = 0.0
    assert R.path_select_torch(cost)["path"].tolist() == [1, 1]
    # a NaN column has no minimum: index 0
    cost = torch.ones(1, 3, 3, dtype=torch.float64)
    cost[0, 1, :] = float("nan")
    got = R.path_select_torch(cost)
    assert got["path"].tolist() == [0, 0] and torch.isnan(got["path_cost"])


# ----------------------------------------------------------------------------- stitch
def _rot_err(feats, R_want, t_want, layout):
    Rg, tg = REF.feats_to_matrices(feats, layout)
    e_t = 0.0 if t_want is None else float(np.abs(tg - t_want).max())
    return float(np.abs(Rg - R_want).max()), e_t


@pytest.mark.parametrize("name", ["angle", "angle_transl", "rot6d"])
@pytest.mark.parametrize("nTO", [(19, 8, 3), (8, 5, 2), (24, 8, 4), (7, 8, 3)], ids=str)
def test_stitch_twin_gives_back_the_motion_its_windows_were_cut_from(name, nTO):
    n, T, O = nTO
    layout, F = REF.LAYOUTS[name]
    motion = REF.random_motion(n, name, seed=5)
    wins = REF.cut_windows(motion, T, O, fill=np.nan)                   # frames past a window's length are never read
    got = R.stitch_windows_torch(torch.from_numpy(wins), O, n, layout)
    assert got.shape == (n, F) and got.dtype == torch.float64 and torch.isfinite(got).all()
    R_want, t_want = REF.feats_to_matrices(motion, layout)
    e_r, e_t = _rot_err(got.numpy(), R_want, t_want, layout)
    assert e_r <= 1e-10 and e_t <= 1e-12, (e_r, e_t)
    # one side of every overlap written as the -q-equivalent rotation: the same result
    starts, lengths = REF.plan(n, T, O)
    mask = np.zeros(wins.shape[:2], bool)
    mask[1:, :O] = True
    mask &= np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    flipped = REF.flip_representation(wins, layout, mask)
    if layout != REF.ROT6D and len(starts) > 1:
        assert np.abs(np.nan_to_num(flipped - wins)).max() > 1.0
    got2 = R.stitch_windows_torch(torch.from_numpy(flipped), O, n, layout)
    e_r, e_t = _rot_err(got2.numpy(), R_want, t_want, layout)
    assert e_r <= 1e-10 and e_t <= 1e-12, (e_r, e_t)


@pytest.mark.parametrize("name", ["angle", "angle_transl", "rot6d"])
def test_stitch_twin_blends_disagreeing_windows_along_the_geodesic(name):
    """Windows that disagree by 0.3..1.0 rad per joint (always the slerp branch): the twin against the matrix form."""
    layout, F = REF.LAYOUTS[name]
    n, T, O = 19, 8, 3
    wins = REF.perturbed_windows(n, T, O, name, seed=9, fill=np.nan)
    got = R.stitch_windows_torch(torch.from_numpy(wins), O, n, layout)
    R_want, t_want = REF.stitch_matrices(wins, O, n, layout)
    e_r, e_t = _rot_err(got.numpy(), R_want, t_want, layout)
    assert e_r <= 1e-10 and e_t <= 1e-12, (e_r, e_t)
    # frames covered by one window are copied bit for bit
    starts, lengths = REF.plan(n, T, O)
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        first = O if w > 0 else 0
        last = T - O if w + 1 < len(starts) else ln
        assert np.array_equal(got.numpy()[lo + first:lo + last], wins[w, first:last])


def test_stitch_twin_without_overlap_is_concatenation():
    n, T = 19, 8
    motion = REF.random_motion(n, "angle_transl", seed=2)
    wins = REF.cut_windows(motion, T, 0, fill=np.nan)
    got = R.stitch_windows_torch(torch.from_numpy(wins), 0, n, REF.ANGLE_TRANSL)
    assert np.array_equal(got.numpy(), motion)
    with pytest.raises(ValueError):
        R.stitch_windows_torch(torch.from_numpy(wins), 0, n + 8, REF.ANGLE_TRANSL)      # not the plan of n + 8 frames
    with pytest.raises(ValueError):
        R.stitch_windows_torch(torch.from_numpy(wins), 5, n, REF.ANGLE_TRANSL)          # 2*O > T


# ----------------------------------------------------------------------------- overlap cost
def test_overlap_cost_twin_against_the_loop_form():
    W, K, T, O = 3, 3, 8, 3
    g = torch.Generator().manual_seed(17)
    jts = torch.randn(W, K, T, 24, 3, generator=g, dtype=torch.float64)
    want = REF.overlap_cost_loops(jts.numpy(), O)
    got = R.overlap_cost_torch(jts, O)
    assert got.shape == (W - 1, K, K) and got.dtype == torch.float64
    assert np.abs(got.numpy() - want).max() <= 1e-12 * want.max()
    # frames outside the overlaps are never read
    masked = jts.clone()
    masked[:, :, O:T - O] = float("nan")
    masked[0, :, :O] = float("nan")
    masked[-1, :, T - O:] = float("nan")
    assert torch.equal(R.overlap_cost_torch(masked, O), got)
    assert R.overlap_cost_torch(jts, 0).abs().max() == 0 and R.overlap_cost_torch(jts[:1], O).shape == (0, K, K)
    with pytest.raises(ValueError):
        R.overlap_cost_torch(jts, 5)


# ----------------------------------------------------------------------------- recording files
def _recording(n, seed=0, pose=69, scene=True, image=True):
    g = np.random.default_rng(seed)
    rec = {"global_orient": g.standard_normal((n, 3)), "body_pose": 0.3 * g.standard_normal((n, pose)),
           "transl": g.standard_normal((n, 3)), "betas": g.standard_normal(10), "wearer_betas": g.standard_normal(10)}
    if scene:
        rec["scene"] = g.standard_normal((50, 3))
    if image:
        rec["image_feats"] = g.random((n, 2048))
    return {k: v.astype(np.float32) for k, v in rec.items()}


def test_load_recording_round_trip_and_windows_batch(tmp_path):
    n, T, O = 19, 8, 3
    rec = _recording(n)
    path = os.path.join(tmp_path, "rec.npz")
    np.savez(path, **rec)
    got = R.load_recording(path)
    assert got["n_frames"] == n
    for k, v in rec.items():
        assert got[k].dtype == np.float32 and np.array_equal(got[k], v), k
    g = np.random.default_rng(1)
    mean, std = g.standard_normal((1, 75)).astype(np.float32), (0.5 + g.random((1, 75))).astype(np.float32)
    batch, starts, lengths = R.windows_batch(got, (mean, std), T, O, ("text", "interactee", "scene", "image"), dataset="egobody")
    assert (starts, lengths) == REF.plan(n, T, O) == ([0, 5, 10, 15], [8, 8, 8, 4])
    W = len(starts)
    motion, transl, beta, utils_, scene, images, length = batch
    assert motion.shape == (W, T, 2, 72) and transl.shape == (W, 2, T, 3) and beta.shape == (W, 2, T, 10) and utils_.shape == (W, T, 6)
    assert scene.shape == (W, 50, 3) and images.shape == (W, 2048) and length.reshape(-1).tolist() == lengths
    # the wearer's slot is all zeros
    assert float(motion[:, :, 0].abs().max()) == 0 and float(transl[:, 0].abs().max()) == 0 and float(beta[:, 0].abs().max()) == 0
    # the interactee: (x - mean) / std of the raw values, renormed back by x * std + mean
    m, s = torch.from_numpy(mean[0]), torch.from_numpy(std[0])
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        raw = torch.from_numpy(np.concatenate([rec["global_orient"][lo:lo + ln], rec["body_pose"][lo:lo + ln]], axis=1))
        assert torch.allclose(motion[w, :ln, 1] * s[:72] + m[:72], raw, atol=1e-5)
        assert torch.allclose(transl[w, 1, :ln] * s[72:75] + m[72:75], torch.from_numpy(rec["transl"][lo:lo + ln]), atol=1e-5)
        assert torch.equal(beta[w, 1, :ln], torch.from_numpy(rec["betas"]).expand(ln, 10))
        # padding past the window's length is the zero frame (zero padding comes before the normalisation, as at load time)
        if ln < T:
            assert torch.equal(motion[w, ln:, 1], (-m[:72] / s[:72]).expand(T - ln, 72)) and float(beta[w, 1, ln:].abs().max()) == 0
            assert torch.allclose(motion[w, ln:, 1] * s[:72] + m[:72], torch.zeros(T - ln, 72), atol=1e-6)
        assert torch.equal(images[w], torch.from_numpy(rec["image_feats"][lo + ln // 2]))
        assert torch.equal(scene[w], torch.from_numpy(rec["scene"]))
    # conditions the recording cannot serve, and a GIMO body pose for an EgoBody model
    with pytest.raises(ValueError, match="scene"):
        R.windows_batch({k: v for k, v in got.items() if k != "scene"}, (mean, std), T, O, ("interactee", "scene"), dataset="egobody")
    with pytest.raises(ValueError, match="body_pose"):
        R.windows_batch(got, (mean, std), T, O, ("interactee",), dataset="gimo")
    # without scene / image conditions the tuple is (motion, transl, beta, utils, length)
    assert len(R.windows_batch(got, (mean, std), T, O, ("text", "interactee"), dataset="egobody")[0]) == 5


def test_windows_batch_is_the_data_modules_load_time_rule(tmp_path):
    """The same person through ``data.normalise_person`` (what EgoSequenceSplit applies) and through windows_batch: equal bits; and
    GIMO's translation statistics are the LAST three."""
    from seeme_amd.data import load_time_stats, normalise_person
    n, T = 6, 8
    rec = _recording(n, seed=3, pose=63, scene=False, image=False)
    rec["n_frames"] = n
    g = np.random.default_rng(4)
    mean, std = g.standard_normal((1, 80)).astype(np.float32), (0.5 + g.random((1, 80))).astype(np.float32)
    batch, starts, lengths = R.windows_batch(rec, (mean, std), T, 2, ("interactee",), dataset="gimo")
    assert (starts, lengths) == ([0], [n])
    pad = lambda x: np.concatenate([x, np.zeros((T - n, x.shape[1]), np.float32)])
    m, s = load_time_stats(mean, std, False)
    mo, tr = normalise_person(pad(rec["global_orient"]), pad(rec["body_pose"]), pad(rec["transl"]), m, s, "gimo", True)
    assert np.array_equal(batch[0][0, :, 1].numpy(), mo) and np.array_equal(batch[1][0, 1].numpy(), tr)
    assert np.allclose(tr[:n] * std[0, -3:] + mean[0, -3:], rec["transl"], atol=1e-5)


def test_load_recording_refuses_pickled_arrays_and_bad_shapes(tmp_path):
    rec = _recording(5, scene=False, image=False)
    bad = os.path.join(tmp_path, "pickled.npz")
    np.savez(bad, **{**rec, "betas": np.array([{"a": 1}] * 10, dtype=object)})
    with pytest.raises(ValueError, match="[Oo]bject|pickle"):
        R.load_recording(bad)
    short = os.path.join(tmp_path, "short.npz")
    np.savez(short, **{**rec, "transl": rec["transl"][:4]})
    with pytest.raises(ValueError, match="transl"):
        R.load_recording(short)
    missing = os.path.join(tmp_path, "missing.npz")
    np.savez(missing, **{k: v for k, v in rec.items() if k != "body_pose"})
    with pytest.raises(ValueError, match="body_pose"):
        R.load_recording(missing)


# ----------------------------------------------------------------------------- the C-ABI
def test_recording_entry_points_are_declared_bound_and_exported():
    import ctypes
    from conftest import REPO
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("seeme_overlap_cost", "seeme_overlap_cost_workspace_bytes", "seeme_path_select", "seeme_path_select_workspace_bytes",
                 "seeme_stitch_windows"):
        assert f"{name}(" in hdr and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert f"SEEME_STITCH_NLERP_DOT {R.NLERP_DOT}f" in hdr
    # the size functions run on the host: 0 for bad sizes
    L = _lib.lib()
    assert L.seeme_overlap_cost_workspace_bytes(3, 33, 8, 3) == 0 and L.seeme_overlap_cost_workspace_bytes(3, 3, 8, 5) == 0
    assert L.seeme_overlap_cost_workspace_bytes(3, 3, 8, 3) == 2 * 1 * 9 * 4
    assert L.seeme_path_select_workspace_bytes(4, 33) == 0 and L.seeme_path_select_workspace_bytes(4, 3) == 3 * 3 * 4
