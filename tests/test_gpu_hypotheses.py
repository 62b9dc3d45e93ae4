"""K hypotheses per sequence on the device: the seeme_hyp_metrics kernel against its float64 torch twin, and ego_eval with K > 1
(one encode of the condition per sequence, K draws) against K = 1 runs fed the same draws."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO
import hyp_reference as R
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu
TOL_F32 = 1e-4               # the project's fp32 bound (tests/test_gpu_flows.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _elem_rel(got, want):
    """max over elements of |got - want| / |want| (every element against its own reference value; exact zeros must be zeros)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    zero = want == 0
    assert (got[zero] == 0).all()
    return float((np.abs(got - want)[~zero] / np.abs(want)[~zero]).max()) if (~zero).any() else 0.0


def _max_rel(a, b):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ----------------------------------------------------------------------------- 5. the kernel
@pytest.mark.parametrize("shape", ["recipe", (1, 1, 3), (3, 2, 16), (32, 20, 196), (5, 32, 196)])
def test_hyp_metrics_kernel_vs_float64_twin(dev, shape):
    from seeme_amd.hyp_metrics import best_index, hyp_metrics_hip, hyp_metrics_torch, keep_mask
    from seeme_amd.mld import EgoMetrics
    if shape == "recipe":
        pred, ref, qp, q, lengths = R.recipe()
    else:
        B, K, T = shape
        pred, ref, qp, q, lengths = R.recipe(B, K, T, lengths=R.ragged_lengths(B, T), seed=3, special=B > 1 and K > 2)
        assert T in lengths and (B < 4 or {1, 2, 3} <= set(lengths))
    B, K, T = pred.shape[:3]
    if shape == "recipe":        # the facts of the recipe, on the REFERENCE values, before anything is compared: at least half of the
        # (b,k) kept on 'test', at least one dropped by each of the three conditions (a filter that drops everything cannot pass)
        kept, _ = R.oracle_per_hyp(pred, ref, qp, q, lengths, "test")
        ph, head = R.np_per_hyp(pred, ref, lengths), R.np_head(qp, q, lengths)
        moving = ph["ACCL"] > 0
        assert kept.sum() == 18 and kept.sum() * 2 >= kept.size
        assert (~moving).any() and (moving & ~(ph["ROOT_ERROR"] < 300)).any() and (moving & ~(head < 0.9)).any()
        assert np.array_equal(kept, moving & (head < 0.9) & (ph["ROOT_ERROR"] < 300))
    p64, r64 = torch.from_numpy(pred), torch.from_numpy(ref)
    want = hyp_metrics_torch(p64, r64, lengths)                 # float64 on the unrounded inputs
    p32, r32 = p64.float().to(dev), r64.float().to(dev)
    got = hyp_metrics_hip(p32, r32, lengths)
    torch.cuda.synchronize()
    for n in ("MPJPE", "ROOT_ERROR", "ACCL", "APD_JOINTS", "STD_JOINTS"):
        e = _elem_rel(got[n].cpu().numpy(), want[n].numpy())
        print(f"hyp_metrics {shape} {n}: max element-wise relative error {e:.3e}")
        assert got[n].shape == ((B, K) if n in ("MPJPE", "ROOT_ERROR", "ACCL") else (B,))
        assert e <= TOL_F32, (n, e)
    if shape == "recipe":        # the 'test' inclusion rule with the recipe's quaternions: the oracle's decision and the float64 argmin
        lens = torch.tensor(lengths, device=dev)
        mask = (torch.arange(T, device=dev)[None] < lens[:, None]).float().repeat_interleave(K, dim=0)
        q_ref = torch.from_numpy(q).float().to(dev).repeat_interleave(K, dim=0).reshape(-1, 4)
        got_t = dict(got)
        got_t["HEAD_ORIENTATION_ERROR"] = EgoMetrics.head_orientation_error(torch.from_numpy(qp).float().to(dev).reshape(-1, 4), q_ref, mask,
                                                                            lens.repeat_interleave(K)).reshape(B, K)
        keep_t = keep_mask(got_t, "test", True)
        assert np.array_equal(keep_t.cpu().numpy(), kept)
        want_best = [int(np.argmin(np.where(kept[b], ph["MPJPE"][b], np.inf))) if kept[b].any() else -1 for b in range(B)]
        assert best_index(got["MPJPE"], keep_t).cpu().tolist() == want_best and want_best.count(-1) == 2
    assert (want["MPJPE"] > 0).all() and (K == 1 or (want["APD_JOINTS"] > 0).all())
    # bitwise reproducible
    again = hyp_metrics_hip(p32, r32, lengths)
    for n in got:
        assert torch.equal(got[n], again[n]), n
    # best_index equals the float64 argmin (inclusion: the 'val' rule, ACCL > 0)
    keep64 = keep_mask(want, "val", False)
    assert torch.equal(keep_mask(got, "val", False).cpu(), keep64)
    assert best_index(got["MPJPE"], keep_mask(got, "val", False)).cpu().tolist() == best_index(want["MPJPE"], keep64).tolist()
    # hypothesis 0 alone (K = 1): per_sequence's numbers, and no diversity at all
    one = hyp_metrics_hip(p32[:, :1].contiguous(), r32, lengths)
    per = EgoMetrics.per_sequence(p32[:, 0], r32, lengths)
    for n in ("MPJPE", "ROOT_ERROR", "ACCL"):
        assert _elem_rel(one[n][:, 0].cpu().numpy(), per[n].cpu().numpy()) <= TOL_F32, n
        assert _elem_rel(one[n][:, 0].cpu().numpy(), want[n][:, 0].numpy()) <= TOL_F32, n
    assert float(one["APD_JOINTS"].abs().max()) == 0.0 and float(one["STD_JOINTS"].abs().max()) == 0.0


# ----------------------------------------------------------------------------- 6. bad arguments
def test_hyp_metrics_bad_arguments_raise(dev):
    from seeme_amd import _lib as L
    from seeme_amd import hyp_metrics as H
    B, T = 2, 8
    ref = torch.zeros(B, T, 24, 3, device=dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    with pytest.raises(L.SeemeError, match="K must be"):
        H._launch(torch.zeros(0, device=dev), ref, lens, B, 0, T)
    with pytest.raises(L.SeemeError, match="K must be"):
        H.hyp_metrics_hip(torch.zeros(B, 33, T, 24, 3, device=dev), ref, [T] * B)
    pred = torch.zeros(B, 4, T, 24, 3, device=dev)
    need = int(L.lib().seeme_hyp_metrics_workspace_bytes(B, 4, T))
    assert need > 0
    with pytest.raises(L.SeemeError, match="workspace"):
        H._launch(pred, ref, lens, B, 4, T, ws_bytes=need - 1)
    with pytest.raises(L.SeemeError):
        H.hyp_metrics_hip(pred.cpu(), ref, [T] * B)
    out = H._launch(pred, ref, lens, B, 4, T, ws_bytes=need)          # the exact size is enough
    assert float(out["MPJPE"].abs().max()) == 0.0


# ----------------------------------------------------------------------------- ego_eval with K > 1
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


def _slice_k(lat, cn, B, K, k):
    sl = lambda t, dim: t.unflatten(dim, (B, K)).select(dim + 1, k).contiguous()
    return sl(lat, 0), (tuple(sl(e, 1) for e in cn) if isinstance(cn, tuple) else sl(cn, 1))


_EXISTING = ("m_ref", "m_rst", "joints_ref", "joints_rst", "orientation_quat_rst", "orientation_quat_ref", "root_interactee",
             "joints_interactee", "orientation_quat_int", "lat_t")
_NEW = ("joints_rst_all", "m_rst_all", "lat_t_all", "hyp_metrics")


def _configs():
    def guided(cfg):
        cfg.model.guidance_scale = 2.5
        cfg.model.scheduler.num_inference_timesteps = 10

    def plain(cfg):
        cfg.model.scheduler.num_inference_timesteps = 10
    return [("config_mld_egobody.yaml", plain, False), ("config_mld_scene.yaml", guided, True)]


@pytest.mark.parametrize("cfg_name,mutate,guidance", _configs(), ids=["egobody", "scene_guided"])
def test_ego_eval_k4_equals_k1_runs_and_shares_the_encoders(dev, cfg_name, mutate, guidance):
    """7, 8, 10: each hypothesis of a K = 4 ego_eval equals the K = 1 ego_eval (the path that existed before the key) fed the k-th slice of the same
    draws; the scene encoder and the VAE encoder run once per call (twice under guidance) on B rows; the keys of a K = 1 result
    hold hypothesis 0 and a K = 1 result has none of the new keys."""
    model, dm, cfg = _mld(dev, cfg_name, mutate=mutate)
    B, K, T = 3, 4, 16
    with_scene = "scene" in cfg.model.condition
    batch = dm.batch(B, idx=4, with_scene=with_scene, lengths=[16, 11, 16])
    lat, cn = _draws(B, K, guidance, dev)
    calls = {"scene": [], "vae": []}
    enc_dist = model.vae.encode_dist
    model.vae.encode_dist = lambda f, l=None: (calls["vae"].append(f.shape[0]), enc_dist(f, l))[1]
    if with_scene:
        enc_scene = model.proscene.encode_scene
        model.proscene.encode_scene = lambda s: (calls["scene"].append(s.shape[0]), enc_scene(s))[1]
    rs = model.ego_eval(batch, latents=lat, cond_noise=cn, num_hypotheses=K)
    n = 2 if guidance else 1
    assert calls["vae"] == [B] * n and calls["scene"] == ([B] * n if with_scene else [])
    model.vae.encode_dist = enc_dist
    if with_scene:
        model.proscene.encode_scene = enc_scene
    assert rs["joints_rst_all"].shape == (B, K, T, 24, 3) and rs["m_rst_all"].shape == (B, K, T, 75) and rs["lat_t_all"].shape == (1, B * K, 256)
    assert rs["joints_rst"].shape == (B, T, 24, 3) and rs["lat_t"].shape == (1, B, 256)
    lat_all = rs["lat_t_all"].reshape(B, K, 256)
    for k in range(K):
        l1, c1 = _slice_k(lat, cn, B, K, k)
        r1 = model.ego_eval(batch, latents=l1, cond_noise=c1)
        assert not any(key in r1 for key in _NEW)
        errs = {"lat_t": _max_rel(lat_all[:, k], r1["lat_t"][0]), "m_rst": _max_rel(rs["m_rst_all"][:, k], r1["m_rst"]),
                "joints_rst": _max_rel(rs["joints_rst_all"][:, k], r1["joints_rst"])}
        print(f"{cfg_name} k={k}: {errs}")
        assert max(errs.values()) <= TOL_F32, (k, errs)
        if k == 0:                                # 10: the existing keys are hypothesis 0
            assert set(r1) | set(_NEW) == set(rs)
            for key in _EXISTING:
                assert rs[key].shape == r1[key].shape, key
                assert _max_rel(rs[key], r1[key]) <= TOL_F32, key
            assert rs["lengths"] == r1["lengths"] and rs["joints_interactee_gt"] is None and r1["joints_interactee_gt"] is None
    # the hypotheses differ from each other, and the device metrics are those of the twin on the same joints
    from seeme_amd.hyp_metrics import hyp_metrics_torch
    hm = rs["hyp_metrics"]
    assert float((rs["joints_rst_all"][:, 0] - rs["joints_rst_all"][:, 1]).abs().max()) > 1e-3
    want = hyp_metrics_torch(rs["joints_rst_all"].double().cpu(), rs["joints_ref"].double().cpu(), rs["lengths"])
    for name in ("MPJPE", "ROOT_ERROR", "ACCL", "APD_JOINTS", "STD_JOINTS"):
        assert _elem_rel(hm[name].cpu().numpy(), want[name].numpy()) <= TOL_F32, name
    assert hm["HEAD_ORIENTATION_ERROR"].shape == (B, K) and hm["best_index"].shape == (B,) and hm["have_quat"] is True
    assert (hm["APD_JOINTS"] > 0).all() and (hm["STD_JOINTS"] > 0).all()


def test_ego_eval_640_rows_is_chunked(dev):
    """9: B = 20, K = 32 is 640 rows: two sampling launches of 320; the cluster kernel reports no give-up, everything is finite, and
    the first and last hypothesis of the first and last sequence equal their K = 1 runs."""
    def mut(cfg):
        cfg.model.scheduler.num_inference_timesteps = 10
    model, dm, cfg = _mld(dev, "config_mld_egobody.yaml", mutate=mut)
    B, K, T = 20, 32, 16
    assert [hi - lo for lo, hi in model._row_chunks(B * K)] == [320, 320] and model._row_chunks(512) == [(0, 512)]
    batch = dm.batch(B, idx=6)
    lat, cn = _draws(B, K, False, dev, seed=5)
    rs = model.ego_eval(batch, latents=lat, cond_noise=cn, num_hypotheses=K)
    torch.cuda.synchronize()
    assert model.denoiser.cluster_status()[0] == 0
    for key in ("joints_rst_all", "m_rst_all", "lat_t_all"):
        assert torch.isfinite(rs[key]).all(), key
    for name in ("MPJPE", "ROOT_ERROR", "ACCL", "APD_JOINTS", "STD_JOINTS"):
        assert torch.isfinite(rs["hyp_metrics"][name]).all(), name
    for k in (0, 31):
        l1, c1 = _slice_k(lat, cn, B, K, k)
        r1 = model.ego_eval(batch, latents=l1, cond_noise=c1)
        for b in (0, 19):
            errs = {"lat_t": _max_rel(rs["lat_t_all"].reshape(B, K, 256)[b, k], r1["lat_t"][0, b]),
                    "m_rst": _max_rel(rs["m_rst_all"][b, k], r1["m_rst"][b]),
                    "joints_rst": _max_rel(rs["joints_rst_all"][b, k], r1["joints_rst"][b])}
            print(f"640 rows b={b} k={k}: {errs}")
            assert max(errs.values()) <= TOL_F32, (b, k, errs)


_TODAY_METRICS = ("MPJPE", "ROOT_ERROR", "ACCL", "HEAD_ORIENTATION_ERROR", "mpjpe_interactee", "count_seq", "seqs_per_s")
_K_METRICS = ("MPJPE_best_of_k", "MPJPE_mean_of_k", "APD_JOINTS", "STD_JOINTS", "count_seq_k", "num_hypotheses", "samples_per_s")


def _json_keys(names):
    return {f"Metrics/{n}{s}" for n in names for s in ("", "/mean", "/min", "/max", "/conf_interval")}


def test_cli_test_main_reports_the_hypothesis_metrics(dev, tmp_path):
    """11: test_main on the synthetic data module with TEST.NUM_HYPOTHESES = 4 writes the new keys; with 1 the JSON has today's keys."""
    from seeme_amd import cli
    cfgp = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    r = cli.train_main(["--cfg", cfgp, "--batch_size", "4", "--nodebug", "--folder", str(tmp_path), "--frames", "24",
                        "--iters_per_epoch", "1", "--epochs", "1"])
    ckpt = os.path.join(r["checkpoints"], "epoch=0.ckpt")
    common = ["--cfg", cfgp, "--batch_size", "4", "--folder", str(tmp_path), "--frames", "24", "--test_batches", "2", "--checkpoint", ckpt]
    out = cli.test_main(common + ["--num_hypotheses", "4"])
    saved = json.load(open(out["file"]))
    assert set(saved) == _json_keys(_TODAY_METRICS + _K_METRICS)
    assert out["Metrics/num_hypotheses/mean"] == 4
    for n in ("APD_JOINTS", "STD_JOINTS"):
        assert np.isfinite(out[f"Metrics/{n}/mean"]) and out[f"Metrics/{n}/mean"] > 0
    assert np.isfinite(out["Metrics/MPJPE_best_of_k/mean"]) and out["Metrics/count_seq_k/mean"] >= 0
    assert abs(out["Metrics/samples_per_s/mean"] - 4 * out["Metrics/seqs_per_s/mean"]) <= 1e-9 * out["Metrics/samples_per_s/mean"]
    out1 = cli.test_main(common)
    assert set(json.load(open(out1["file"]))) == _json_keys(_TODAY_METRICS)


def test_allsplit_step_val_orders_best_and_mean_of_k(dev):
    """11: random weights leave no hypothesis inside the 'test' bounds, so the ordering best <= mean is asserted on 'val'."""
    def mut(cfg):
        cfg.model.scheduler.num_inference_timesteps = 5
        cfg.TEST.NUM_HYPOTHESES = 4
    model, dm, cfg = _mld(dev, "config_mld_egobody.yaml", mutate=mut)
    model.EgoMetric.reset(), model.HypMetric.reset()
    for it in range(2):
        model.allsplit_step("val", dm.batch(3, idx=20 + it))
    got = model.HypMetric.compute()
    assert got["count_seq_k"] == 6 and got["num_hypotheses"] == 4
    assert 0 < got["MPJPE_best_of_k"] < got["MPJPE_mean_of_k"] and got["APD_JOINTS"] > 0 and got["STD_JOINTS"] > 0
    ego = model.EgoMetric.compute()
    assert ego["count_seq"] == 6 and got["MPJPE_best_of_k"] <= ego["MPJPE"]            # EgoMetric sees hypothesis 0
    out = model.test_step(dm.batch(3, idx=30))
    assert out.shape == (3, 16, 24, 3)


def _variant_vae(cfg):
    pass


def _variant_future_pose(cfg):
    cfg.TEST.SEE_FUTURE = True
    cfg.TEST.POSE_ESTIMATION_TASK = True
    cfg.TEST.GLOBAL_ORIENT_PRED = False
    cfg.model.scheduler.num_inference_timesteps = 5


def _variant_rot6d(cfg):
    cfg.DATA_TYPE = "rot6d"
    cfg.model.nfeats = 144
    cfg.model.motion_vae.params.nfeats = cfg.model.denoiser.params.nfeats = 144
    cfg.TRAIN.ABLATION.PREDICT_TRANSL = False
    cfg.model.scheduler.num_inference_timesteps = 5


@pytest.mark.parametrize("cfg_name,mutate", [("config_vae_egobody.yaml", _variant_vae), ("config_mld_egobody.yaml", _variant_future_pose),
                                             ("config_mld_egobody.yaml", _variant_rot6d)], ids=["stage_vae", "see_future_pose_task", "rot6d"])
def test_ego_eval_variants_keep_working_with_hypotheses(dev, cfg_name, mutate):
    """Stage 'vae' (K posterior draws of the target), SEE_FUTURE + POSE_ESTIMATION_TASK + the reference orientation, rot6d: every
    hypothesis equals the K = 1 run fed its slice of the draws."""
    model, dm, cfg = _mld(dev, cfg_name, mutate=mutate)
    B, K = 3, 3
    pose = bool(cfg.TEST.get("POSE_ESTIMATION_TASK", False))
    batch = dm.batch(B, idx=8, lengths=[16, 12, 16], pose_estimation=pose)
    lat, cn = _draws(B, K, False, dev, seed=2)
    rs = model.ego_eval(batch, latents=lat, cond_noise=cn, num_hypotheses=K)
    T = rs["joints_ref"].shape[1]
    assert T == (8 if model.see_future else 16) and rs["joints_rst_all"].shape == (B, K, T, 24, 3)
    assert (rs["joints_interactee_gt"] is not None) == pose
    assert rs["hyp_metrics"]["have_quat"] == (cfg.DATA_TYPE == "angle")
    for k in range(K):
        l1, c1 = _slice_k(lat, cn, B, K, k)
        r1 = model.ego_eval(batch, latents=l1, cond_noise=c1)
        assert r1["joints_rst"].shape == (B, T, 24, 3)
        assert _max_rel(rs["m_rst_all"][:, k], r1["m_rst"]) <= TOL_F32 and _max_rel(rs["joints_rst_all"][:, k], r1["joints_rst"]) <= TOL_F32
        if k == 0:
            for key in _EXISTING + (("joints_interactee_gt",) if pose else ()):
                if r1[key] is None:
                    assert rs[key] is None, key
                else:
                    assert _max_rel(rs[key], r1[key]) <= TOL_F32, key
    assert float((rs["joints_rst_all"][:, 0] - rs["joints_rst_all"][:, 1]).abs().max()) > 1e-4


def _ddpm(cfg):
    cfg.model.scheduler.target = "seeme_amd.schedulers.DDPMScheduler"
    cfg.model.scheduler.num_inference_timesteps = 50
    cfg.model.scheduler.params = {"num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "scaled_linear",
                                  "variance_type": "fixed_small", "clip_sample": False}


def test_ego_eval_ddpm_step_noise_has_bk_rows(dev):
    """The DDPM injection point: step_noise [steps, B*K, 256], row b*K + k.  Each hypothesis equals the K = 1 run fed the k-th slices of
    the latents, the condition noise and the step noise; without injection the draws are made and the result is finite."""
    model, dm, cfg = _mld(dev, "config_mld_egobody.yaml", mutate=_ddpm)
    B, K, T, steps = 3, 4, 16, 50
    batch = dm.batch(B, idx=12, lengths=[16, 16, 9])
    lat, cn = _draws(B, K, False, dev, seed=21)
    g = torch.Generator().manual_seed(22)
    noise = torch.randn(steps, B * K, 256, generator=g).to(dev)
    rs = model.ego_eval(batch, latents=lat, cond_noise=cn, step_noise=noise, num_hypotheses=K)
    assert model.scheduler.needs_noise(0.0) and len(model.scheduler.timesteps) == steps
    lat_all = rs["lat_t_all"].reshape(B, K, 256)
    for k in range(K):
        l1, c1 = _slice_k(lat, cn, B, K, k)
        n1 = noise.reshape(steps, B, K, 256)[:, :, k].contiguous()
        r1 = model.ego_eval(batch, latents=l1, cond_noise=c1, step_noise=n1)
        errs = {"lat_t": _max_rel(lat_all[:, k], r1["lat_t"][0]), "m_rst": _max_rel(rs["m_rst_all"][:, k], r1["m_rst"]),
                "joints_rst": _max_rel(rs["joints_rst_all"][:, k], r1["joints_rst"])}
        print(f"ddpm k={k}: {errs}")
        assert max(errs.values()) <= TOL_F32, (k, errs)
    # the step noise matters: another slice of it gives another sample
    l1, c1 = _slice_k(lat, cn, B, K, 0)
    other = model.ego_eval(batch, latents=l1, cond_noise=c1, step_noise=noise.reshape(steps, B, K, 256)[:, :, 1].contiguous())
    assert _max_rel(other["lat_t"][0], lat_all[:, 0]) > 1e-3
    torch.manual_seed(5)
    free = model.ego_eval(batch, num_hypotheses=K)
    assert torch.isfinite(free["joints_rst_all"]).all() and float((free["lat_t_all"] - rs["lat_t_all"]).abs().max()) > 1e-3


@pytest.mark.parametrize("condition", [["text", "image", "scene"], ["text", "interactee", "scene", "image"]], ids=["scene_image", "int_scene_image"])
def test_ego_eval_image_token_with_hypotheses(dev, condition):
    """The image token (and the scene token beside it) is computed once per sequence and repeated K times."""
    def mut(cfg):
        cfg.model.condition = list(condition)
        cfg.model.guidance_scale = 1.0
        cfg.model.scheduler.num_inference_timesteps = 10
    model, dm, cfg = _mld(dev, "config_mld_image_scene.yaml", mutate=mut)
    B, K, T = 3, 3, 16
    batch = dm.batch(B, idx=14, with_scene=True, with_image=True, lengths=[16, 13, 16])
    lat, cn = _draws(B, K, False, dev, seed=31)
    calls = []
    proj = model.output_images.forward
    model.output_images.forward = lambda x: (calls.append(x.shape[0]), proj(x))[1]
    rs = model.ego_eval(batch, latents=lat, cond_noise=cn, num_hypotheses=K)
    assert calls == [B]
    model.output_images.forward = proj
    for k in range(K):
        l1, c1 = _slice_k(lat, cn, B, K, k)
        r1 = model.ego_eval(batch, latents=l1, cond_noise=c1)
        errs = {"lat_t": _max_rel(rs["lat_t_all"].reshape(B, K, 256)[:, k], r1["lat_t"][0]), "m_rst": _max_rel(rs["m_rst_all"][:, k], r1["m_rst"]),
                "joints_rst": _max_rel(rs["joints_rst_all"][:, k], r1["joints_rst"])}
        print(f"{condition} k={k}: {errs}")
        assert max(errs.values()) <= TOL_F32, (k, errs)
    assert float((rs["joints_rst_all"][:, 0] - rs["joints_rst_all"][:, 1]).abs().max()) > 1e-4


# ----------------------------------------------------------------------------- the draws of a pass that is handed none
def _steps10(cfg):
    cfg.model.scheduler.num_inference_timesteps = 10


def _guided10(cfg):
    cfg.model.guidance_scale = 2.5
    cfg.model.scheduler.num_inference_timesteps = 10


@pytest.mark.parametrize("cfg_name,mutate,entry,B,K", [("config_mld_egobody.yaml", _steps10, "ego_eval", 3, 1),
                                                      ("config_mld_egobody.yaml", _steps10, "ego_eval", 3, 4),
                                                      ("config_mld_scene.yaml", _guided10, "ego_eval", 3, 3),
                                                      ("config_mld_scene.yaml", _guided10, "predict", 3, 3),
                                                      ("config_mld_egobody.yaml", _ddpm, "ego_eval", 2, 2)],
                         ids=["egobody_k1", "egobody_k4", "scene_guided_k3", "scene_guided_predict_k3", "ddpm_k2"])
def test_uninjected_pass_draws_in_the_documented_order(dev, cfg_name, mutate, entry, B, K):
    """A pass that is handed no draws makes them on the device in this order and with these shapes: the condition's posterior noise
    [1,B*K,256] (then the unconditional condition's under guidance), the initial latents [B*K,1,256], the DDPM step noise
    [steps,B*K,256].  So the same draws, made by the same calls after the same seed and injected, give the same bits."""
    model, dm, cfg = _mld(dev, cfg_name, mutate=mutate)
    guidance = model.do_classifier_free_guidance
    batch = dm.batch(B, idx=4, with_scene="scene" in cfg.model.condition, lengths=[16, 11, 16][:B])
    run = lambda **kw: (model.predict if entry == "predict" else model.ego_eval)(batch, num_hypotheses=K, **kw)
    seed = 1234
    torch.manual_seed(seed)
    eps_c = torch.empty(1, B * K, 256, device=dev).normal_()
    cn = (eps_c, torch.empty(1, B * K, 256, device=dev).normal_()) if guidance else eps_c
    lat = torch.randn(B * K, 1, 256, device=dev)
    ddpm = mutate is _ddpm
    noise = torch.randn(cfg.model.scheduler.num_inference_timesteps, B * K, 256, device=dev) if ddpm else None
    fed = run(latents=lat, cond_noise=cn, step_noise=noise)
    assert model.scheduler.needs_noise(0.0) == ddpm
    torch.manual_seed(seed)
    free = run()
    keys = ("lat_t", "m_rst", "joints_rst") if K == 1 else ("lat_t_all", "m_rst_all", "joints_rst_all")
    if entry == "ego_eval" and K > 1:
        keys += ("lat_t", "m_rst", "joints_rst")
    for key in keys:
        assert torch.isfinite(fed[key]).all() and torch.equal(fed[key], free[key]), key
    torch.manual_seed(seed + 1)                                       # (and the free pass does draw: another seed, another sample)
    assert not torch.equal(run()[keys[0]], free[keys[0]])
