"""A whole recording on the device: the three kernels of csrc/recording.hip against the float64 references of
tests/recording_reference.py at the project's fp32 bound, then MLD.predict (never reads the wearer's slot; equals ego_eval's
hypotheses), MLD.predict_recording (the composition of the three twins) and cli.predict_main."""
import os

import numpy as np
import pytest
import torch

import recording_reference as REF
from test_gpu_hyp_select import TOL_F32, _draws, _elem_rel, _mld

pytestmark = pytest.mark.gpu

# REC_FC of csrc/recording.hip: shared frames per workgroup of k_overlap_partial.  O = 33 = 8 * REC_FC + 1 makes the last workgroup
# of a seam hold a single frame (and T = 67 > 2 * 33 leaves one frame outside both overlaps).
REC_FC = 4
OVERLAP_CASES = [(3, 3, 8, 3), (2, 32, 5, 2), (4, 1, 8, 4), (2, 5, 67, 8 * REC_FC + 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _joints(W, K, T, seed):
    g = torch.Generator().manual_seed(seed)
    # hypotheses of one window 0.1 m apart around a common walk, windows displaced from each other: costs of 100 mm and more
    return (torch.randn(W, 1, T, 24, 3, generator=g, dtype=torch.float64) + 0.1 * torch.randn(W, K, T, 24, 3, generator=g, dtype=torch.float64))


# ----------------------------------------------------------------------------- 1. overlap cost
@pytest.mark.parametrize("shape", OVERLAP_CASES, ids=str)
def test_overlap_cost_kernel_vs_float64_loops(dev, shape):
    from seeme_amd.recording import overlap_cost_hip, overlap_cost_torch
    W, K, T, O = shape
    j64 = _joints(W, K, T, seed=sum(shape))
    want = overlap_cost_torch(j64, O)
    if W * K * K * O <= 3000:                                          # the explicit loops where they are quick; the twin was held to them on the CPU
        assert np.abs(REF.overlap_cost_loops(j64.numpy(), O) - want.numpy()).max() <= 1e-12 * float(want.max())
    j32 = j64.float().to(dev)
    got = overlap_cost_hip(j32, O)
    torch.cuda.synchronize()
    assert got.shape == (W - 1, K, K) and got.dtype == torch.float32
    e = _elem_rel(got, overlap_cost_torch(j32.double().cpu(), O))      # float64 on the inputs the kernel saw
    print(f"overlap_cost {shape}: max element-wise relative error {e:.3e}")
    assert e <= TOL_F32, e
    # bitwise reproducible
    assert torch.equal(overlap_cost_hip(j32, O), got)
    # frames outside the overlaps are never read
    masked = j32.clone()
    masked[:, :, O:T - O] = float("nan")
    masked[0, :, :O] = float("nan")
    masked[-1, :, T - O:] = float("nan")
    assert torch.equal(overlap_cost_hip(masked, O), got)


def test_overlap_cost_without_a_seam_or_a_shared_frame(dev):
    from seeme_amd.recording import overlap_cost_hip
    j32 = _joints(3, 4, 8, seed=1).float().to(dev)
    assert overlap_cost_hip(j32[:1], 3).shape == (0, 4, 4)
    z = overlap_cost_hip(j32, 0)
    assert z.shape == (2, 4, 4) and float(z.abs().max()) == 0.0


# ----------------------------------------------------------------------------- 2. path
def _costs(W, K, seed, with_unary):
    g = torch.Generator().manual_seed(seed)
    cost = (50.0 * torch.rand(max(W - 1, 0), K, K, generator=g, dtype=torch.float64)).float()
    unary = (30.0 * torch.rand(W, K, generator=g, dtype=torch.float64)).float() if with_unary else None
    return cost, unary


def _check_path(got, cost, unary, W, K, low):
    """The float64 total of the returned path is within TOL_F32 (relative) of the minimum `low` (the form of _assert_near_minimum: no
    index equality where two paths lie closer than that); seam and total are the float64 sums along the returned path."""
    path = got["path"].cpu().tolist()
    assert got["path"].dtype == torch.int64 and len(path) == W and all(0 <= p < K for p in path)
    c64, u64 = cost.double().numpy(), None if unary is None else unary.double().numpy()
    mine = REF.path_total(c64, u64, path)
    assert mine - low <= TOL_F32 * abs(low), (mine, low, path)
    assert abs(float(got["path_cost"]) - mine) <= TOL_F32 * max(abs(mine), 1e-30), (float(got["path_cost"]), mine)
    seam = got["seam_cost"].cpu()
    assert seam.shape == (W - 1,)
    for w in range(W - 1):
        assert float(seam[w]) == float(cost[w, path[w], path[w + 1]])
    return mine


@pytest.mark.parametrize("with_unary", [False, True])
@pytest.mark.parametrize("WK", [(4, 3), (5, 2), (1, 4)], ids=str)
def test_path_select_kernel_finds_the_enumerated_minimum(dev, WK, with_unary):
    from seeme_amd.recording import path_select_hip
    W, K = WK
    cost, unary = _costs(W, K, 3 + W * 10 + K, with_unary)
    got = path_select_hip(cost.to(dev), None if unary is None else unary.to(dev))
    low, arg = REF.best_path_enumerate(cost.double().numpy(), None if unary is None else unary.double().numpy(), W, K)
    mine = _check_path(got, cost, unary, W, K, low)
    print(f"path_select {WK} unary {with_unary}: path {got['path'].tolist()} total {mine:.6f}, enumerated {arg} {low:.6f}")


@pytest.mark.parametrize("with_unary", [False, True])
def test_path_select_kernel_long_chain_vs_float64_twin(dev, with_unary):
    from seeme_amd.recording import path_select_hip, path_select_torch
    W, K = 40, 32
    cost, unary = _costs(W, K, 77, with_unary)
    want = path_select_torch(cost.double(), None if unary is None else unary.double())
    got = path_select_hip(cost.to(dev), None if unary is None else unary.to(dev))
    _check_path(got, cost, unary, W, K, float(want["path_cost"]))
    again = path_select_hip(cost.to(dev), None if unary is None else unary.to(dev))
    assert torch.equal(again["path"], got["path"]) and torch.equal(again["seam_cost"], got["seam_cost"])
    assert torch.equal(again["path_cost"], got["path_cost"])


def test_path_select_kernel_ties_and_nan(dev):
    from seeme_amd.recording import path_select_hip, path_select_torch
    W, K = 6, 5
    cost = torch.full((W - 1, K, K), 2.5, device=dev)
    assert path_select_hip(cost)["path"].tolist() == [0] * W
    assert path_select_hip(cost, torch.full((W, K), 1.25, device=dev))["path"].tolist() == [0] * W
    tie = torch.ones(1, 3, 3)
    tie[0, 2, 1] = tie[0, 1, 1] = tie[0, 1, 2] = 0.0
    assert path_select_hip(tie.to(dev))["path"].tolist() == path_select_torch(tie)["path"].tolist() == [1, 1]
    bad = torch.ones(1, 3, 3)
    bad[0, 1, :] = float("nan")
    got = path_select_hip(bad.to(dev))
    assert got["path"].tolist() == [0, 0] and torch.isnan(got["path_cost"])
    # W = 1: the argmin of unary, 0 without it
    u = torch.tensor([[3.0, 1.0, 2.0, 1.0]], device=dev)
    got = path_select_hip(torch.zeros(0, 4, 4, device=dev), u)
    assert got["path"].tolist() == [1] and float(got["path_cost"]) == 1.0 and got["seam_cost"].shape == (0,)
    assert path_select_hip(torch.zeros(0, 4, 4, device=dev))["path"].tolist() == [0]


# ----------------------------------------------------------------------------- 3. stitch
def _rot_err(feats, R_want, t_want, layout):
    Rg, tg = REF.feats_to_matrices(feats.double().cpu().numpy(), layout)
    e_t = 0.0 if t_want is None else float(np.abs(tg - t_want).max())
    return float(np.abs(Rg - R_want).max()), e_t


@pytest.mark.parametrize("name", ["angle", "angle_transl", "rot6d"])
@pytest.mark.parametrize("WTO", [(3, 8, 3), (2, 5, 2)], ids=str)
def test_stitch_kernel_vs_float64_matrices(dev, name, WTO):
    """Last windows of length O + 1.  Two inputs: windows that disagree by 0.3..1.0 rad per joint (the slerp branch) and windows
    cut from one motion (dot product 1: the normalised-lerp branch, which between IDENTICAL rotations is exact; between rotations
    a quaternion angle t < acos(0.9995) = 0.0316 apart it leaves the geodesic by less than t^3 / 10 = 3e-6, far inside the bound)."""
    from seeme_amd.recording import stitch_windows_hip
    W, T, O = WTO
    n = (W - 1) * (T - O) + O + 1
    layout, F = REF.LAYOUTS[name]
    assert REF.plan(n, T, O)[1] == [T] * (W - 1) + [O + 1]
    for kind in ("disagree", "one_motion"):
        if kind == "disagree":
            wins = REF.perturbed_windows(n, T, O, name, seed=9 + W)
        else:
            wins = REF.cut_windows(REF.random_motion(n, name, seed=5), T, O)
        w32 = torch.from_numpy(wins).float()
        R_want, t_want = REF.stitch_matrices(w32.double().numpy(), O, n, layout)      # float64 on the inputs the kernel saw
        got = stitch_windows_hip(w32.to(dev), O, n, layout)
        torch.cuda.synchronize()
        assert got.shape == (n, F) and got.dtype == torch.float32 and torch.isfinite(got).all()
        e_r, e_t = _rot_err(got, R_want, t_want, layout)
        print(f"stitch {name} {WTO} {kind}: rotation matrices {e_r:.3e}, translation {e_t:.3e}")
        assert e_r <= TOL_F32 and e_t <= TOL_F32, (e_r, e_t)
        # frames covered by one window are copied bit for bit
        starts, lengths = REF.plan(n, T, O)
        for w, (lo, ln) in enumerate(zip(starts, lengths)):
            first, last = (O if w > 0 else 0), (T - O if w + 1 < W else ln)
            assert torch.equal(got[lo + first:lo + last].cpu(), w32[w, first:last])
        # the later side of every overlap written as the -q-equivalent rotation: the same rotations
        mask = np.zeros((W, T), bool)
        mask[1:, :O] = True
        flipped = torch.from_numpy(REF.flip_representation(w32.double().numpy(), layout, mask)).float()
        e_r, e_t = _rot_err(stitch_windows_hip(flipped.to(dev), O, n, layout), R_want, t_want, layout)
        print(f"  sign-flipped: {e_r:.3e}, {e_t:.3e}")
        assert e_r <= TOL_F32 and e_t <= TOL_F32, (e_r, e_t)
        # NaN past the last window's length leaves the result unchanged, bit for bit
        holes = w32.clone()
        holes[-1, O + 1:] = float("nan")
        assert torch.equal(stitch_windows_hip(holes.to(dev), O, n, layout), got)


def test_stitch_kernel_without_overlap_and_single_window(dev):
    from seeme_amd.recording import stitch_windows_hip
    motion = torch.from_numpy(REF.random_motion(19, "angle_transl", seed=2)).float()
    wins = torch.from_numpy(REF.cut_windows(motion.double().numpy(), 8, 0, fill=np.nan)).float()
    assert torch.equal(stitch_windows_hip(wins.to(dev), 0, 19, REF.ANGLE_TRANSL).cpu(), motion)
    one = torch.from_numpy(REF.cut_windows(motion[:6].double().numpy(), 8, 3, fill=np.nan)).float()
    assert torch.equal(stitch_windows_hip(one.to(dev), 3, 6, REF.ANGLE_TRANSL).cpu(), motion[:6])


# ----------------------------------------------------------------------------- 4. bad arguments
def test_recording_kernels_bad_arguments_raise(dev):
    from seeme_amd import _lib as L
    from seeme_amd import recording as R
    W, T, O = 3, 8, 3
    with pytest.raises(L.SeemeError, match="K must be"):
        R.overlap_cost_hip(torch.zeros(W, 33, T, 24, 3, device=dev), O)
    with pytest.raises(L.SeemeError, match="overlap"):
        R.overlap_cost_hip(torch.zeros(W, 4, T, 24, 3, device=dev), 5)
    jts = torch.zeros(W, 4, T, 24, 3, device=dev)
    need = int(L.lib().seeme_overlap_cost_workspace_bytes(W, 4, T, O))
    assert need == (W - 1) * 1 * 16 * 4
    with pytest.raises(L.SeemeError, match="workspace"):
        R._launch_overlap(jts, W, 4, T, O, ws_bytes=need - 1)
    assert float(R._launch_overlap(jts, W, 4, T, O, ws_bytes=need).abs().max()) == 0.0        # the exact size is enough
    with pytest.raises(L.SeemeError):
        R.overlap_cost_hip(jts.cpu(), O)
    with pytest.raises(L.SeemeError, match="K must be"):
        R.path_select_hip(torch.zeros(2, 33, 33, device=dev))
    cost = torch.zeros(W - 1, 4, 4, device=dev)
    need = int(L.lib().seeme_path_select_workspace_bytes(W, 4))
    assert need == (W - 1) * 4 * 4
    with pytest.raises(L.SeemeError, match="workspace"):
        R._launch_path(cost, None, W, 4, ws_bytes=need - 1)
    assert R._launch_path(cost, None, W, 4, ws_bytes=need)["path"].tolist() == [0] * W
    with pytest.raises(L.SeemeError, match="cost is"):
        R.path_select_hip(cost, torch.zeros(W + 1, 4, device=dev))
    feats = torch.zeros(W, T, 75, device=dev)
    n = 2 * (T - O) + O + 1
    with pytest.raises(L.SeemeError, match="overlap"):
        R.stitch_windows_hip(feats, 5, n, R.STITCH_ANGLE_TRANSL)
    for bad_n in (n + T, T, 0):                                        # n_frames does not match the plan
        with pytest.raises(L.SeemeError, match="window plan|n_frames"):
            R.stitch_windows_hip(feats, O, bad_n, R.STITCH_ANGLE_TRANSL)
    with pytest.raises(L.SeemeError, match="144"):
        R.stitch_windows_hip(feats, O, n, R.STITCH_ROT6D)
    with pytest.raises(L.SeemeError, match="layout"):
        R.stitch_windows_hip(feats, O, n, 7)
    with pytest.raises(L.SeemeError, match="wide"):
        R.stitch_windows_hip(torch.zeros(W, T, 74, device=dev), O, n, R.STITCH_ANGLE)
    assert R.stitch_windows_hip(feats, O, n, R.STITCH_ANGLE_TRANSL).shape == (n, 75)


# ----------------------------------------------------------------------------- 5. MLD.predict
def _mut(cfg):
    cfg.model.scheduler.num_inference_timesteps = 10


@pytest.fixture(scope="module")
def scene_model(dev):
    return _mld(dev, "config_mld_scene.yaml", mutate=_mut)


def _nan_wearer(batch):
    motion, transl, beta = (t.clone() for t in batch[:3])
    motion[:, :, 0], transl[:, 0], beta[:, 0] = float("nan"), float("nan"), float("nan")
    return (motion, transl, beta) + tuple(batch[3:])


def test_predict_never_reads_the_wearer_slot_and_equals_ego_eval(dev, scene_model):
    model, dm, cfg = scene_model
    B, K, T = 3, 3, 16
    batch = dm.batch(B, idx=4, with_scene=True, lengths=[16, 11, 16])
    lat, cn = _draws(B, K, model.do_classifier_free_guidance, dev)
    betas = batch[2][:, 0, 0].contiguous()                              # the batch's wearer betas [B,10]
    a = model.predict(batch, num_hypotheses=K, betas=betas, latents=lat, cond_noise=cn)
    b = model.predict(_nan_wearer(batch), num_hypotheses=K, betas=betas, latents=lat, cond_noise=cn)
    assert set(a) == {"m_rst_all", "joints_rst_all", "lat_t_all", "lengths", "hyp_metrics"}
    assert set(a["hyp_metrics"]) == {"PAIR_DIST", "medoid_index"}
    F = model.vae.nfeats
    assert a["m_rst_all"].shape == (B, K, T, F) and a["joints_rst_all"].shape == (B, K, T, 24, 3) and a["lengths"] == [16, 11, 16]
    pairs = [(a[k], b[k]) for k in ("m_rst_all", "joints_rst_all", "lat_t_all")] + [(a["hyp_metrics"][k], b["hyp_metrics"][k])
                                                                                    for k in ("PAIR_DIST", "medoid_index")]
    for x, y in pairs:                                                  # finite, and bitwise equal with a NaN wearer: never read
        assert torch.isfinite(x.float()).all() and torch.equal(x, y)
    assert b["lengths"] == a["lengths"]
    rs = model.ego_eval(batch, latents=lat, cond_noise=cn, num_hypotheses=K)
    assert torch.equal(a["m_rst_all"], rs["m_rst_all"]) and torch.equal(a["joints_rst_all"], rs["joints_rst_all"])
    assert torch.equal(a["lat_t_all"], rs["lat_t_all"])
    # betas default to zeros: another body, the same features
    z = model.predict(batch, num_hypotheses=K, latents=lat, cond_noise=cn)
    assert torch.equal(z["m_rst_all"], a["m_rst_all"]) and not torch.equal(z["joints_rst_all"], a["joints_rst_all"])
    with pytest.raises(ValueError, match="betas"):
        model.predict(batch, num_hypotheses=K, betas=betas[:2])
    with pytest.raises(ValueError, match="num_hypotheses"):
        model.predict(batch, num_hypotheses=33)


def test_predict_refuses_stage_vae(dev, scene_model):
    model, dm, cfg = scene_model
    stage, model.stage = model.stage, "vae"                             # stage 'vae' reconstructs its target: it needs labels
    try:
        with pytest.raises(ValueError, match="stage"):
            model.predict(dm.batch(2, idx=1, with_scene=True), num_hypotheses=2)
    finally:
        model.stage = stage


# ----------------------------------------------------------------------------- 6. MLD.predict_recording
def _synthetic_recording(n, seed=0, scene_points=384):
    g = np.random.default_rng(seed)
    walk = lambda w, s: np.cumsum(s * g.standard_normal((n, w)), axis=0)
    rec = {"global_orient": 0.5 * g.standard_normal((1, 3)) + walk(3, 0.03), "body_pose": 0.3 * g.standard_normal((1, 69)) + walk(69, 0.02),
           "transl": g.standard_normal((1, 3)) + walk(3, 0.02), "betas": 0.5 * g.standard_normal(10),
           "wearer_betas": 0.5 * g.standard_normal(10), "scene": g.random((scene_points, 3)) * 6 - 3}
    return {k: v.astype(np.float32) for k, v in rec.items()}


def test_predict_recording_is_the_composition_of_the_twins(dev, scene_model):
    from seeme_amd import recording as R
    model, dm, cfg = scene_model
    n, T, O, K = 37, 16, 4, 3
    rec = _synthetic_recording(n)
    rec["n_frames"] = n
    batch, starts, lengths = R.windows_batch(rec, dm, T, O, tuple(cfg.model.condition), dataset="egobody", device=dev)
    assert starts == [0, 12, 24] and lengths == [16, 16, 13] and float(batch[0][:, :, 0].abs().max()) == 0
    W = len(starts)
    lat, cn = _draws(W, K, model.do_classifier_free_guidance, dev, seed=5)
    betas = torch.from_numpy(rec["wearer_betas"]).to(dev)
    out = model.predict_recording(batch, n, overlap=O, betas=betas, num_hypotheses=K, latents=lat, cond_noise=cn)
    assert set(out) == {"motion", "joints", "path", "seam_cost", "path_cost", "window_starts", "window_lengths", "predict"}
    F = model.vae.nfeats
    assert out["motion"].shape == (n, F) and out["joints"].shape == (n, 24, 3) and out["path"].shape == (W,) and out["seam_cost"].shape == (W - 1,)
    assert out["window_starts"] == starts and out["window_lengths"] == lengths
    assert torch.isfinite(out["motion"]).all() and torch.isfinite(out["joints"]).all()
    pr = out["predict"]
    # the three twins in float64 on the predict result
    j64, m64 = pr["joints_rst_all"].double().cpu(), pr["m_rst_all"].double().cpu()
    cost = R.overlap_cost_torch(j64, O)
    unary = pr["hyp_metrics"]["PAIR_DIST"].double().cpu().sum(dim=2) / max(K - 1, 1)
    want = R.path_select_torch(cost, unary)
    path = out["path"].cpu().tolist()
    low = float(want["path_cost"])
    mine = REF.path_total(cost.numpy(), unary.numpy(), path)
    print(f"predict_recording: path {path} (float64 twin {want['path'].tolist()}), total {mine:.4f} vs {low:.4f}, seams {out['seam_cost'].tolist()}")
    assert mine - low <= TOL_F32 * low                                  # (index equality only where no two paths lie closer than that)
    assert abs(float(out["path_cost"]) - mine) <= TOL_F32 * mine
    assert _elem_rel(out["seam_cost"], cost[torch.arange(W - 1), torch.tensor(path[:-1]), torch.tensor(path[1:])]) <= TOL_F32
    layout = R.stitch_layout(model.data_type, model.transl_in_feats)
    assert layout == R.STITCH_ANGLE_TRANSL
    chosen = m64[torch.arange(W), torch.tensor(path)]
    stitched = R.stitch_windows_torch(chosen, O, n, layout)
    R_want, t_want = REF.feats_to_matrices(stitched.numpy(), layout)
    e_r, e_t = _rot_err(out["motion"], R_want, t_want, layout)
    print(f"  stitched motion vs the float64 twin: rotation matrices {e_r:.3e}, translation {e_t:.3e}")
    assert e_r <= TOL_F32 and e_t <= TOL_F32
    # frames covered by one window are the chosen hypothesis's frames, exactly
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        first, last = (O if w > 0 else 0), (T - O if w + 1 < W else ln)
        assert torch.equal(out["motion"][lo + first:lo + last], pr["m_rst_all"][w, path[w], first:last])
    # the joints are the SMPL joints of the stitched motion
    jj = model._feats_to_joints(out["motion"][None], betas[None, None].expand(1, n, 10))[0]
    assert torch.equal(jj, out["joints"])
    # a batch that is not the plan of n_frames
    with pytest.raises(ValueError, match="plan"):
        model.predict_recording(batch, n + 1, overlap=O, num_hypotheses=K)


def test_predict_recording_single_window(dev, scene_model):
    from seeme_amd import recording as R
    model, dm, cfg = scene_model
    n, T, O, K = 13, 16, 4, 4
    rec = _synthetic_recording(n, seed=2)
    rec["n_frames"] = n
    batch, starts, lengths = R.windows_batch(rec, dm, T, O, tuple(cfg.model.condition), dataset="egobody", device=dev)
    assert lengths == [13]
    lat, cn = _draws(1, K, model.do_classifier_free_guidance, dev, seed=6)
    a = model.predict_recording(batch, n, overlap=O, medoid_weight=0, num_hypotheses=K, latents=lat, cond_noise=cn)
    assert a["path"].tolist() == [0] and a["seam_cost"].shape == (0,) and float(a["path_cost"]) == 0.0
    assert torch.equal(a["motion"], a["predict"]["m_rst_all"][0, 0, :n])
    b = model.predict_recording(batch, n, overlap=O, medoid_weight=1.0, num_hypotheses=K, latents=lat, cond_noise=cn)
    rows = b["predict"]["hyp_metrics"]["PAIR_DIST"][0].double().cpu().sum(dim=1)
    k = int(b["path"][0])
    assert float(rows[k]) - float(rows.min()) <= TOL_F32 * float(rows.min()), (k, rows)
    assert torch.equal(b["motion"], b["predict"]["m_rst_all"][0, k, :n])
    with pytest.raises(ValueError, match="medoid_weight"):
        model.predict_recording(batch, n, overlap=O, medoid_weight=-1.0, num_hypotheses=K)
    # a recording shorter than twice the overlap is still one window
    rec5 = {k: (v[:5] if v.shape[:1] == (n,) else v) for k, v in rec.items() if k != "n_frames"}
    rec5["n_frames"] = 5
    b5, _, l5 = R.windows_batch(rec5, dm, T, O, tuple(cfg.model.condition), dataset="egobody", device=dev)
    c = model.predict_recording(b5, 5, overlap=O, num_hypotheses=K)
    assert l5 == [5] and c["motion"].shape == (5, model.vae.nfeats) and c["joints"].shape == (5, 24, 3) and torch.isfinite(c["motion"]).all()
    assert torch.equal(c["motion"], c["predict"]["m_rst_all"][0, int(c["path"][0]), :5])


def test_window_config_keys_are_validated(dev):
    def bad_overlap(cfg):
        cfg.TEST.WINDOW_OVERLAP = -2
    with pytest.raises(ValueError, match="WINDOW_OVERLAP"):
        _mld(dev, "config_mld_egobody.yaml", mutate=bad_overlap)

    def bad_weight(cfg):
        cfg.TEST.PATH_MEDOID_WEIGHT = "much"
    with pytest.raises(ValueError, match="PATH_MEDOID_WEIGHT"):
        _mld(dev, "config_mld_egobody.yaml", mutate=bad_weight)


# ----------------------------------------------------------------------------- 7. cli.predict_main
def test_cli_predict_main_writes_the_stitched_motion(dev, tmp_path, scene_model):
    from conftest import REPO
    from seeme_amd import cli
    model, dm, cfg = scene_model
    ckpt = os.path.join(tmp_path, "model.ckpt")
    cli.save_checkpoint(ckpt, model, 0, 0)
    n = 37
    rec_path, out_path = os.path.join(tmp_path, "rec.npz"), os.path.join(tmp_path, "out", "motion.npz")
    np.savez(rec_path, **_synthetic_recording(n, seed=3))
    argv = ["--cfg", os.path.join(REPO, "configs", "config_mld_scene.yaml"), "--checkpoint", ckpt, "--folder", str(tmp_path), "--frames", "16",
            "--scene_points", "384", "--input", rec_path, "--output", out_path, "--num_hypotheses", "3", "--overlap", "4", "--seed", "11"]
    r = cli.predict_main(argv + ["--save_hypotheses"])
    assert r["file"] == out_path and r["n_frames"] == n and r["windows"] == 3
    with np.load(out_path, allow_pickle=False) as z:
        first = {k: z[k] for k in z.files}
    assert set(first) == {"global_orient", "body_pose", "transl", "joints", "window_starts", "path", "seam_cost", "m_rst_all"}
    assert first["global_orient"].shape == (n, 3) and first["body_pose"].shape == (n, 69) and first["transl"].shape == (n, 3)
    assert first["joints"].shape == (n, 24, 3) and first["window_starts"].tolist() == [0, 12, 24] and first["path"].shape == (3,)
    assert first["seam_cost"].shape == (2,) and first["m_rst_all"].shape == (3, 3, 16, 75)
    assert all(np.isfinite(v).all() for v in first.values())
    r2 = cli.predict_main(argv)                                          # --seed makes two runs equal
    with np.load(out_path, allow_pickle=False) as z:
        second = {k: z[k] for k in z.files}
    assert set(second) == set(first) - {"m_rst_all"} and r2["path"] == r["path"]
    for k, v in second.items():
        assert np.array_equal(v, first[k]), k
