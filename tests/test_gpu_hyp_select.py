"""Choosing one of K hypotheses without ground truth on the device: the seeme_hyp_pairdist kernel pair against its float64 torch twin,
and the medoid selection through ego_eval, allsplit_step and cli.test_main (TEST.HYP_SELECT).

Inputs and the gap assertion are those of tests/test_hyp_select_cpu.py (one hypothesis per sequence made central; every sequence with
K >= 3 has a float64 gap >= 1e-2 between its two smallest row sums, asserted before anything is compared).  (64,3,64) is the smallest
case on the far side of the chunk-length switch (B * ceil(T/8) >= 512: chunks of 8 frames instead of 4)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO
import test_hyp_select_cpu as C
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu
TOL_F32 = 1e-4               # the project's fp32 bound (tests/test_gpu_flows.py)
KERNEL_CASES = ["recipe", (1, 1, 3), (3, 2, 16), (3, 3, 9), (4, 7, 17), (3, 20, 9), (2, 31, 4), (2, 32, 5), (1, 4, 1), (64, 3, 64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _elem_rel(got, want):
    """max over elements of |got - want| / |want| (every element against its own reference value; exact zeros must be zeros)."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = want.detach().double().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    zero = want == 0
    assert (got[zero] == 0).all()
    return float((np.abs(got - want)[~zero] / np.abs(want)[~zero]).max()) if (~zero).any() else 0.0


def _rows64(D):
    """float64 row sums in j order."""
    rows = torch.zeros_like(D[:, :, 0])
    for j in range(D.shape[1]):
        rows = rows + D[:, :, j]
    return rows


def _assert_near_minimum(D64, index):
    """Independent of any gap: the float64 row sum at the returned index is within TOL_F32 (relative) of the float64 minimum."""
    rows = _rows64(D64)
    at = rows.gather(1, index.cpu().long()[:, None])[:, 0]
    low = rows.min(dim=1).values
    assert (at - low <= TOL_F32 * low).all(), (at, low)


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("shape", KERNEL_CASES, ids=str)
def test_hyp_pairdist_kernel_vs_float64_twin(dev, shape):
    from seeme_amd.hyp_metrics import hyp_metrics_hip, hyp_pairdist_hip, hyp_pairdist_torch
    pred, ref, lengths, centers = C.inputs(shape)
    B, K, T = pred.shape[:3]
    p64 = torch.from_numpy(pred)
    want = hyp_pairdist_torch(p64, lengths)                     # float64 on the unrounded inputs
    D64 = want["PAIR_DIST"]
    gap = C.assert_gap(_rows64(D64).numpy())
    p32 = p64.float().to(dev)
    got = hyp_pairdist_hip(p32, lengths)
    torch.cuda.synchronize()
    D = got["PAIR_DIST"]
    assert D.shape == (B, K, K) and D.dtype == torch.float32
    assert got["medoid_index"].shape == (B,) and got["medoid_index"].dtype == torch.int64
    e = _elem_rel(D, D64)
    print(f"hyp_pairdist {shape}: max element-wise relative error {e:.3e}, smallest gap {gap}, medoid {got['medoid_index'].tolist()}")
    assert e <= TOL_F32, e
    assert torch.equal(D, D.transpose(1, 2)) and float(torch.diagonal(D, dim1=1, dim2=2).abs().max()) == 0.0
    assert got["medoid_index"].cpu().tolist() == want["medoid_index"].tolist()
    assert want["medoid_index"].tolist() == (centers if K >= 3 else [0] * B)
    _assert_near_minimum(D64, got["medoid_index"])
    # the matrix adds up to the APD of seeme_hyp_metrics
    apd = hyp_metrics_hip(p32, torch.from_numpy(ref).float().to(dev), lengths)["APD_JOINTS"]
    mine = D.double().sum(dim=(1, 2)) / max(K * (K - 1), 1) / 2
    ea = _elem_rel(mine, apd)
    print(f"  APD identity: {ea:.3e}")
    assert ea <= TOL_F32, ea
    # bitwise reproducible
    again = hyp_pairdist_hip(p32, lengths)
    assert torch.equal(again["PAIR_DIST"], D) and torch.equal(again["medoid_index"], got["medoid_index"])
    # a length above T is T
    over = [l + 5 if l == T else l for l in lengths]
    assert max(over) == T + 5
    clamped = hyp_pairdist_hip(p32, over)
    assert torch.equal(clamped["PAIR_DIST"], D) and torch.equal(clamped["medoid_index"], got["medoid_index"])


def test_hyp_pairdist_no_valid_frame_is_a_zero_matrix(dev):
    from seeme_amd.hyp_metrics import hyp_pairdist_hip, hyp_pairdist_torch
    pred, ref, lengths, centers = C.inputs((4, 7, 17))
    hand = [40, 0, -3, 5]
    want = hyp_pairdist_torch(torch.from_numpy(pred), hand)
    got = hyp_pairdist_hip(torch.from_numpy(pred).float().to(dev), hand)
    assert _elem_rel(got["PAIR_DIST"], want["PAIR_DIST"]) <= TOL_F32
    for b in (1, 2):
        assert float(got["PAIR_DIST"][b].abs().max()) == 0.0 and int(got["medoid_index"][b]) == 0
    _assert_near_minimum(want["PAIR_DIST"], got["medoid_index"])


# ----------------------------------------------------------------------------- 2. bad arguments
def test_hyp_pairdist_bad_arguments_raise(dev):
    from seeme_amd import _lib as L
    from seeme_amd import hyp_metrics as H
    B, T = 2, 8
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    with pytest.raises(L.SeemeError, match="K must be"):
        H._launch_pairdist(torch.zeros(0, device=dev), lens, B, 0, T)
    with pytest.raises(L.SeemeError, match="K must be"):
        H.hyp_pairdist_hip(torch.zeros(B, 33, T, 24, 3, device=dev), [T] * B)
    pred = torch.zeros(B, 4, T, 24, 3, device=dev)
    need = int(L.lib().seeme_hyp_pairdist_workspace_bytes(B, 4, T))
    assert need == B * 2 * 6 * 4
    with pytest.raises(L.SeemeError, match="workspace"):
        H._launch_pairdist(pred, lens, B, 4, T, ws_bytes=need - 1)
    with pytest.raises(L.SeemeError):
        H.hyp_pairdist_hip(pred.cpu(), [T] * B)
    out = H._launch_pairdist(pred, lens, B, 4, T, ws_bytes=need)          # the exact size is enough
    assert float(out["PAIR_DIST"].abs().max()) == 0.0 and out["medoid_index"].tolist() == [0, 0]


# ----------------------------------------------------------------------------- ego_eval with the selection
def _mld(dev, cfg_name, T=16, n_points=384, mutate=None):
    """The parity configuration of tests/test_gpu_flows.py::_mld: recipe weights, fp32 weight image, fp32 VAE."""
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(os.path.join(REPO, "configs", cfg_name))
    if mutate:
        mutate(cfg)
    dm = SyntheticEgoDataModule(nfeats=cfg.model.nfeats, T=T, n_points=n_points, device=dev,
                                pose_dim=cfg.model.nfeats - (3 if cfg.TRAIN.ABLATION.PREDICT_TRANSL else 0))
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser)
    if hasattr(model, "proscene"):
        load_recipe_(model.proscene.scene_enc)
    model = model.to(dev).eval()
    assert model.denoiser.weight_dtype == "fp32" and model.vae.precision == "fp32"
    return model, dm, cfg


def _draws(B, K, guidance, dev, seed=11):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    lat = rn(B * K, 1, 256)
    e_c = rn(1, B * K, 256)
    return lat, ((e_c, rn(1, B * K, 256)) if guidance else e_c)


_RS_TODAY = {"m_ref", "m_rst", "joints_ref", "joints_rst", "orientation_quat_rst", "orientation_quat_ref", "root_interactee",
             "joints_interactee", "orientation_quat_int", "joints_interactee_gt", "lengths", "list_names", "lat_t",
             "joints_rst_all", "m_rst_all", "lat_t_all", "hyp_metrics"}
_HM_TODAY = {"MPJPE", "ROOT_ERROR", "ACCL", "APD_JOINTS", "STD_JOINTS", "HEAD_ORIENTATION_ERROR", "have_quat", "best_index"}
_HM_NEW = {"PAIR_DIST", "medoid_index", "selected_index"}


def _assert_selection(rs, B, K):
    """The keys of a K = 1 result are the _all tensors gathered at the selected index, bit for bit; the matrix is the twin's."""
    from seeme_amd.hyp_metrics import hyp_pairdist_torch
    hm = rs["hyp_metrics"]
    sel = hm["selected_index"]
    assert sel.dtype == torch.int64 and sel.shape == (B,) and torch.equal(sel, hm["medoid_index"])
    rows = torch.arange(B, device=sel.device)
    T = rs["joints_rst_all"].shape[2]
    assert torch.equal(rs["joints_rst"], rs["joints_rst_all"][rows, sel])
    assert torch.equal(rs["m_rst"], rs["m_rst_all"][rows, sel])
    assert rs["lat_t"].shape == (1, B, 256) and torch.equal(rs["lat_t"][0], rs["lat_t_all"].reshape(B, K, 256)[rows, sel])
    from seeme_amd import geometry as G
    q_all = G.aa_to_quat(rs["m_rst_all"][..., :3].reshape(-1, 3).contiguous()).reshape(B, K, T, 4)
    assert rs["orientation_quat_rst"].shape == (B * T, 4) and torch.equal(rs["orientation_quat_rst"], q_all[rows, sel].reshape(-1, 4))
    want = hyp_pairdist_torch(rs["joints_rst_all"].double().cpu(), rs["lengths"])
    e = _elem_rel(hm["PAIR_DIST"], want["PAIR_DIST"])
    print(f"  PAIR_DIST {e:.3e}, selected {sel.tolist()}, float64 medoid {want['medoid_index'].tolist()}")
    assert e <= TOL_F32
    _assert_near_minimum(want["PAIR_DIST"], hm["medoid_index"])       # random weights: no gap is assumed


def test_ego_eval_medoid_selection_fills_the_single_prediction_keys(dev):
    def mut(cfg):
        cfg.model.scheduler.num_inference_timesteps = 10
    model, dm, cfg = _mld(dev, "config_mld_egobody.yaml", mutate=mut)
    B, K, T = 3, 4, 16
    batch = dm.batch(B, idx=4, lengths=[16, 11, 16])
    lat, cn = _draws(B, K, False, dev)
    rs = model.ego_eval(batch, latents=lat, cond_noise=cn, num_hypotheses=K, hyp_select="medoid")
    assert set(rs) == _RS_TODAY and set(rs["hyp_metrics"]) == _HM_TODAY | _HM_NEW
    assert rs["hyp_metrics"]["PAIR_DIST"].shape == (B, K, K)
    _assert_selection(rs, B, K)
    # 'first', or nothing: today's keys and hypothesis 0; the _all tensors do not depend on the selection
    for kw in ({"hyp_select": "first"}, {}):
        r0 = model.ego_eval(batch, latents=lat, cond_noise=cn, num_hypotheses=K, **kw)
        assert set(r0) == _RS_TODAY and set(r0["hyp_metrics"]) == _HM_TODAY
        assert torch.equal(r0["joints_rst"], r0["joints_rst_all"][:, 0]) and torch.equal(r0["m_rst"], r0["m_rst_all"][:, 0])
        assert torch.equal(r0["lat_t"][0], r0["lat_t_all"].reshape(B, K, 256)[:, 0])
        for key in ("joints_rst_all", "m_rst_all", "lat_t_all"):
            assert torch.equal(r0[key], rs[key]), key
    # K = 1 has nothing to select
    l1, c1 = lat.unflatten(0, (B, K))[:, 0].contiguous(), cn.unflatten(1, (B, K))[:, :, 0].contiguous()
    r1 = model.ego_eval(batch, latents=l1, cond_noise=c1, num_hypotheses=1, hyp_select="medoid")
    assert "hyp_metrics" not in r1
    with pytest.raises(ValueError, match="hyp_select"):
        model.ego_eval(batch, num_hypotheses=K, hyp_select="mean")


def test_ego_eval_medoid_with_scene_and_mesh_metrics(dev):
    """TEST.HYP_SELECT and TEST.MESH_METRICS from the config, a scene of 384 points: the mesh numbers of the selection are the
    [B,K] entries gathered at the index, and want_vertices poses the selected hypothesis."""
    from seeme_amd.hyp_metrics import best_index, keep_mask

    def mut(cfg):
        cfg.model.scheduler.num_inference_timesteps = 10
        cfg.TEST.MESH_METRICS = True
        cfg.TEST.HYP_SELECT = "medoid"
        cfg.TEST.NUM_HYPOTHESES = 4
    model, dm, cfg = _mld(dev, "config_mld_scene.yaml", mutate=mut)
    B, K, T = 3, 4, 16
    batch = dm.batch(B, idx=4, with_scene=True, lengths=[16, 11, 16])
    lat, cn = _draws(B, K, model.do_classifier_free_guidance, dev)
    rs = model.ego_eval(batch, latents=lat, cond_noise=cn, want_vertices=True)
    assert set(rs) == _RS_TODAY | {"mesh_metrics", "vertices_ref", "vertices_rst"}
    _assert_selection(rs, B, K)
    hm, mm = rs["hyp_metrics"], rs["mesh_metrics"]
    sel = hm["selected_index"]
    # the mesh of the selection: its pelvis-free joints are those of joints_rst
    from seeme_amd.mld import split_batch
    beta = split_batch(model.condition, batch)[2].float()
    posed = model._feats_to_joints(rs["m_rst"], beta[:, 0 if model.estimate == "wearer" else 1, :T], True)
    assert rs["vertices_rst"].shape == (B, T, 6890, 3) and torch.equal(rs["vertices_rst"], posed[1])
    hm["best_index"] = best_index(hm["MPJPE"], keep_mask(hm, "val", hm["have_quat"]))         # as allsplit_step('val')
    model.SelMetric.reset()
    model.SelMetric.update(hm, "val", mm)
    got = model.SelMetric.compute()
    assert got["count_seq_medoid"] == B
    for name in ("PA_MPJPE", "V2V"):
        want = float(mm[name].double().gather(1, sel[:, None]).mean())
        assert abs(got[f"{name}_medoid"] - want) <= 1e-12 * want, name
    assert 0 < got["PA_MPJPE_medoid"] < got["MPJPE_medoid"]           # Procrustes alignment can only lower the joint error


# ----------------------------------------------------------------------------- 4. allsplit_step
def test_allsplit_step_val_follows_the_selection(dev):
    def mut(cfg):
        cfg.model.scheduler.num_inference_timesteps = 5
        cfg.TEST.NUM_HYPOTHESES = 4
        cfg.TEST.HYP_SELECT = "medoid"
    model, dm, cfg = _mld(dev, "config_mld_egobody.yaml", mutate=mut)
    model.EgoMetric.reset(), model.HypMetric.reset(), model.SelMetric.reset()
    for it in range(2):
        model.allsplit_step("val", dm.batch(3, idx=20 + it))
    got, hyp, ego = model.SelMetric.compute(), model.HypMetric.compute(), model.EgoMetric.compute()
    print(got, hyp, ego)
    assert set(got) == {"MPJPE_medoid", "ROOT_ERROR_medoid", "ACCL_medoid", "count_seq_medoid", "medoid_is_best_ratio"}
    assert got["count_seq_medoid"] == 6 == ego["count_seq"]
    assert 0 < hyp["MPJPE_best_of_k"] <= got["MPJPE_medoid"]
    assert abs(ego["MPJPE"] - got["MPJPE_medoid"]) <= TOL_F32 * got["MPJPE_medoid"]            # EgoMetric now sees the selection
    assert abs(ego["ROOT_ERROR"] - got["ROOT_ERROR_medoid"]) <= TOL_F32 * got["ROOT_ERROR_medoid"]
    assert 0 <= got["medoid_is_best_ratio"] <= 1 and got["ACCL_medoid"] > 0
    out = model.test_step(dm.batch(3, idx=30))
    assert out.shape == (3, 16, 24, 3)
    # with the mesh metrics on, the selection's PA-MPJPE and V2V are reported beside its joint error
    model.mesh_metrics = True
    model.SelMetric.reset()
    model.allsplit_step("val", dm.batch(3, idx=20))
    mesh = model.SelMetric.compute()
    assert set(mesh) == set(got) | {"PA_MPJPE_medoid", "V2V_medoid"} and mesh["count_seq_medoid"] == 3
    assert 0 < mesh["PA_MPJPE_medoid"] < mesh["MPJPE_medoid"] and mesh["V2V_medoid"] > 0


# ----------------------------------------------------------------------------- 5. cli.test_main
_TODAY_METRICS = ("MPJPE", "ROOT_ERROR", "ACCL", "HEAD_ORIENTATION_ERROR", "mpjpe_interactee", "count_seq", "seqs_per_s")
_K_METRICS = ("MPJPE_best_of_k", "MPJPE_mean_of_k", "APD_JOINTS", "STD_JOINTS", "count_seq_k", "num_hypotheses", "samples_per_s")
_SEL_METRICS = ("MPJPE_medoid", "ROOT_ERROR_medoid", "ACCL_medoid", "count_seq_medoid", "medoid_is_best_ratio")


def _json_keys(names):
    return {f"Metrics/{n}{s}" for n in names for s in ("", "/mean", "/min", "/max", "/conf_interval")}


def test_cli_test_main_reports_the_selection_metrics(dev, tmp_path):
    from seeme_amd import cli
    cfgp = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    r = cli.train_main(["--cfg", cfgp, "--batch_size", "4", "--nodebug", "--folder", str(tmp_path), "--frames", "24",
                        "--iters_per_epoch", "1", "--epochs", "1"])
    ckpt = os.path.join(r["checkpoints"], "epoch=0.ckpt")
    common = ["--cfg", cfgp, "--batch_size", "4", "--folder", str(tmp_path), "--frames", "24", "--test_batches", "2", "--checkpoint", ckpt,
              "--num_hypotheses", "4"]
    out = cli.test_main(common + ["--hyp_select", "medoid"])
    assert set(json.load(open(out["file"]))) == _json_keys(_TODAY_METRICS + _K_METRICS + _SEL_METRICS)
    for n in _SEL_METRICS:
        assert np.isfinite(out[f"Metrics/{n}/mean"]), n
    assert 0 <= out["Metrics/count_seq_medoid/mean"] <= 8 and 0 <= out["Metrics/medoid_is_best_ratio/mean"] <= 1
    out0 = cli.test_main(common + ["--hyp_select", "first"])
    assert set(json.load(open(out0["file"]))) == _json_keys(_TODAY_METRICS + _K_METRICS)
