"""Interpersonal distance and mutual gaze on the device: the seeme_social_metrics kernel against its float64 torch twin on the unrounded
inputs, its reproducibility and argument checks, and TEST.SOCIAL_METRICS through ego_eval, allsplit_step and test_main."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO
import social_reference as R
from seeme_amd.social_metrics import FRAME_CHUNK as FC
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu
TOL_F32 = 1e-4               # the project's fp32 bound (tests/test_gpu_hypotheses.py)
NAMES = R.PER_SEQ + R.PER_HYP


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


def _edge_lengths(T):
    """Lengths that end before, on and after the first chunk edge, the full length, and 0 (or the second edge when T reaches it)."""
    return [T, min(T, FC - 1), min(T, FC), min(T, FC + 1), 2 * FC if T >= 2 * FC else 0]


def _shapes():
    out = [((1, 1, 1), [1]), ((3, 2, 16), [1, 2, 16]), ((2, 32, 9), [9, 5])]
    return out + [((5, 3, T), _edge_lengths(T)) for T in (FC - 1, FC, FC + 1, 2 * FC + 1)]


def _f32(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).float().to(dev) for a in arrays]


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shape,lengths", _shapes(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_social_kernel_vs_float64_twin(dev, shape, lengths):
    """Every figure is printed before it is asserted.  Measured on an MI355X: the largest element-wise relative error over these
    shapes is 3.0e-6 (GAZE_ANGLE_ERROR at (3,2,16)); the distance numbers stay below 1e-6.  The bound is the project's 1e-4."""
    from seeme_amd.social_metrics import social_metrics_hip, social_metrics_torch
    B, K, T = shape
    a = R.recipe(B, K, T, lengths=lengths, seed=5 + T)
    want = {n: v.numpy() for n, v in social_metrics_torch(*[torch.from_numpy(x) for x in a[:-1]], lengths).items()}     # unrounded inputs
    R.assert_recipe_margins(want, lengths)                                       # the facts of the recipe, before anything is compared
    got = social_metrics_hip(*_f32(a[:-1], dev), lengths)
    torch.cuda.synchronize()
    for n in NAMES:
        assert got[n].shape == ((B, K) if n in R.PER_HYP else (B,)) and got[n].dtype == torch.float32
        e = _elem_rel(got[n].cpu().numpy(), want[n])
        print(f"social_metrics {shape} {n}: max element-wise relative error {e:.3e}")
        assert e <= TOL_F32, (n, e)
    for b, n_valid in enumerate(lengths):
        if n_valid == 0:
            assert all(float(got[n][b].abs().max()) == 0.0 for n in NAMES)
    again = social_metrics_hip(*_f32(a[:-1], dev), lengths)                      # bitwise reproducible
    assert all(torch.equal(got[n], again[n]) for n in NAMES)


def test_social_kernel_special_frames(dev):
    """Parallel gaze exactly 0, antiparallel exactly 180, a degenerate quaternion the identity, coincident joints c = 0; lengths below 0
    and above T are clamped."""
    from seeme_amd.social_metrics import social_metrics_hip, social_metrics_torch
    B, K, T = 5, 2, FC + 2
    pred, ref, intr, qp, qr, qi, _ = R.recipe(B, K, T, seed=8)
    lengths = [0, 1, T, T + 3, -2]
    qr[1] = 2.0 * qi[1]                                                          # the same rotation: 0 degrees
    qp[1, 1] = 0.0                                                               # degenerate: the identity
    qi[3] = np.array([2.0, 0.0, 0.0, 0.0])                                       # looks along +z ...
    qp[3, 0] = np.array([0.0, 3.0, 0.0, 0.0])                                    # ... and a half turn about x of that: 180 degrees
    ref[2, :, 7] = intr[2, :, 3]                                                 # coincident joints
    pred[2, 1, :, 5] = intr[2, :, 0]
    args = (pred, ref, intr, qp, qr, qi)
    want = {n: v.numpy() for n, v in social_metrics_torch(*[torch.from_numpy(x) for x in args], lengths).items()}
    got = {n: v.cpu().numpy() for n, v in social_metrics_hip(*_f32(args, dev), lengths).items()}
    for n in NAMES:
        e = _elem_rel(got[n], want[n])                                           # (exact zeros of the twin must be zeros here)
        print(f"social_metrics special {n}: {e:.3e}")
        assert e <= TOL_F32, (n, e)
        assert (got[n][[0, 4]] == 0).all(), n
    assert want["GAZE_ANGLE_REF"][1] == 0.0 and want["GAZE_ANGLE"][3, 0] == 180.0 and got["GAZE_ANGLE"][3, 0] == 180.0
    assert want["CLOSEST_DIST_REF"][2] == 0.0 and want["CLOSEST_DIST"][2, 1] == 0.0 and want["CLOSEST_DIST"][2, 0] > 0
    assert (got["GAZE_ANGLE"] <= 180.0).all() and (got["GAZE_ANGLE"] >= 0.0).all()


def test_social_kernel_rows_do_not_depend_on_the_batch(dev):
    """Rows of a B = 5 call equal the B = 1 calls on each sequence, bit for bit, whatever the workspace held."""
    from seeme_amd import social_metrics as S
    B, K, T = 5, 3, 2 * FC + 1
    lengths = _edge_lengths(T)
    a = _f32(R.recipe(B, K, T, lengths=lengths, seed=2)[:-1], dev)
    got = S.social_metrics_hip(*a, lengths)
    S._WS.fill_(0xFF)
    for b in range(B):
        one = S.social_metrics_hip(*[x[b:b + 1].contiguous() for x in a], lengths[b:b + 1])
        for n in NAMES:
            assert torch.equal(one[n][0], got[n][b]), (b, n)
    # flat quaternions, as ego_eval holds them, are the same call
    flat = S.social_metrics_hip(a[0], a[1], a[2], a[3].reshape(-1, 4), a[4].reshape(-1, 4), a[5].reshape(-1, 4), lengths)
    assert all(torch.equal(flat[n], got[n]) for n in NAMES)


def test_social_kernel_bad_arguments_raise(dev):
    from seeme_amd import _lib as L
    from seeme_amd import social_metrics as S
    B, K, T = 2, 4, 9
    z = lambda *s: torch.zeros(*s, device=dev)
    ref, intr, qr, qi = z(B, T, 24, 3), z(B, T, 24, 3), z(B, T, 4), z(B, T, 4)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    with pytest.raises(L.SeemeError, match="K must"):
        S._launch(z(16), ref, intr, z(16), qr, qi, lens, B, 0, T)
    with pytest.raises(L.SeemeError, match="K must"):
        S.social_metrics_hip(z(B, 33, T, 24, 3), ref, intr, z(B, 33, T, 4), qr, qi, [T] * B)
    pred, qp = z(B, K, T, 24, 3), z(B, K, T, 4)
    need = int(L.lib().seeme_social_metrics_workspace_bytes(B, K, T))
    assert need == B * 2 * (5 * K + 3) * 4
    with pytest.raises(L.SeemeError, match="workspace"):
        S._launch(pred, ref, intr, qp, qr, qi, lens, B, K, T, ws_bytes=need - 1)
    with pytest.raises(L.SeemeError, match="jts_ref"):
        S.social_metrics_hip(pred, ref.cpu(), intr, qp, qr, qi, [T] * B)
    with pytest.raises(L.SeemeError, match="quaternions"):
        S.social_metrics_hip(pred, ref, intr, qp[:, :2], qr, qi, [T] * B)
    with pytest.raises(L.SeemeError, match="float32"):
        S.social_metrics_hip(pred, ref, intr.double(), qp, qr, qi, [T] * B)
    out = S._launch(pred, ref, intr, qp, qr, qi, lens, B, K, T, ws_bytes=need)   # the exact size is enough; all-zero input: all zeros
    assert float(out["PERSON_DIST"].abs().max()) == 0.0 and float(out["GAZE_ANGLE"].abs().max()) == 0.0      # (identity vs identity)


# ----------------------------------------------------------------------------- ego_eval, allsplit_step, test_main
_MODELS = {}


def _mld(dev, mutate=None, T=16):
    """The parity configuration of tests/test_gpu_hypotheses.py::_mld: recipe weights, fp32 weight image, fp32 VAE.  One model per
    configuration for the whole module (they are only evaluated)."""
    if mutate in _MODELS:
        return _MODELS[mutate]
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_egobody.yaml"))
    cfg.model.scheduler.num_inference_timesteps = 5
    if mutate:
        mutate(cfg)
    dm = SyntheticEgoDataModule(nfeats=cfg.model.nfeats, T=T, n_points=384, device=dev, pose_dim=cfg.model.nfeats - 3)
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser)
    model = model.to(dev).eval()
    assert model.denoiser.weight_dtype == "fp32" and model.vae.precision == "fp32"
    _MODELS[mutate] = (model, dm)
    return model, dm


def _twin_of_result(model, rs, K):
    """social_metrics_torch in float64 on rs's own joints and quaternions."""
    from seeme_amd.social_metrics import social_metrics_torch
    d = lambda t: t.detach().double().cpu()
    B, T = rs["joints_ref"].shape[:2]
    if K == 1:
        jp, qp = rs["joints_rst"][:, None], rs["orientation_quat_rst"].reshape(B, 1, T, 4)
    else:
        jp = rs["joints_rst_all"]
        o = None if model.pred_global_orient else rs["m_ref"][:, :, :3].repeat_interleave(K, dim=0)
        qp = model._orientation_quat(rs["m_rst_all"].reshape(B * K, T, -1), o).reshape(B, K, T, 4)
    return social_metrics_torch(d(jp), d(rs["joints_ref"]), d(rs["joints_interactee"]), d(qp), d(rs["orientation_quat_ref"]).reshape(B, T, 4),
                                d(rs["orientation_quat_int"]).reshape(B, T, 4), rs["lengths"])


def _on(cfg):
    cfg.TEST.SOCIAL_METRICS = True


def _on_future(cfg):
    cfg.TEST.SOCIAL_METRICS, cfg.TEST.SEE_FUTURE = True, True


@pytest.mark.parametrize("K,mutate", [(1, _on), (4, _on), (4, _on_future)], ids=["k1", "k4", "k4_see_future"])
def test_ego_eval_social_metrics_equal_the_twin(dev, K, mutate):
    model, dm = _mld(dev, mutate)
    B, T = 3, 16
    lengths = [16, 11, 5]
    rs = model.ego_eval(dm.batch(B, idx=4, lengths=lengths), num_hypotheses=K)
    assert rs["lengths"] == ([8, 5, 2] if model.see_future else lengths)         # the lengths ego_eval uses: halved under SEE_FUTURE
    sm, want = rs["social_metrics"], _twin_of_result(model, rs, K)
    assert set(sm) == set(NAMES)
    for n in NAMES:
        assert sm[n].shape == ((B, K) if n in R.PER_HYP else (B,))
        e = _elem_rel(sm[n].cpu().numpy(), want[n].numpy())
        print(f"ego_eval K={K} see_future={model.see_future} {n}: {e:.3e}")
        assert e <= TOL_F32, (n, e)
    assert (want["PERSON_DIST"] > 0).all() and (want["GAZE_ANGLE_ERROR"] > 0).all()


def _off(cfg):
    cfg.TEST.SOCIAL_METRICS = False


def _on_ref_orient(cfg):
    cfg.TEST.SOCIAL_METRICS, cfg.TEST.GLOBAL_ORIENT_PRED = True, False


@pytest.mark.parametrize("K", [1, 4])
def test_option_off_leaves_the_result_keys_alone_and_reference_orientation_gives_zero(dev, K):
    batch_of = lambda dm: dm.batch(2, idx=9, lengths=[16, 9])
    keys, hm_keys = [], []
    for mutate in (None, _off, _on):
        model, dm = _mld(dev, mutate)
        rs = model.ego_eval(batch_of(dm), num_hypotheses=K)
        keys.append(set(rs))
        hm_keys.append(set(rs.get("hyp_metrics", {})))
    assert keys[0] == keys[1] and "social_metrics" not in keys[0] and keys[2] == keys[0] | {"social_metrics"}
    assert hm_keys[0] == hm_keys[1] == hm_keys[2]
    model, dm = _mld(dev, _on_ref_orient)
    sm = model.ego_eval(batch_of(dm), num_hypotheses=K)["social_metrics"]
    assert float(sm["GAZE_ANGLE_ERROR"].abs().max()) == 0.0                       # posed with the reference orientation: exactly 0
    assert torch.equal(sm["GAZE_ANGLE"], sm["GAZE_ANGLE_REF"][:, None].expand(2, K)) and (sm["PERSON_DIST_ERROR"] > 0).all()


@pytest.mark.parametrize("K", [1, 4])
def test_allsplit_step_accumulates_what_numpy_accumulates(dev, K, monkeypatch):
    """Two batches through allsplit_step('test'), then two through 'val' (random weights leave no sequence inside the 'test' bounds, so
    the binned errors are checked on 'val'): compute() equals the numpy accumulation over the results ego_eval returned."""
    from seeme_amd.hyp_metrics import keep_mask
    from seeme_amd.mld import EgoMetrics

    model, dm = _mld(dev, _on)
    seen, ego_eval = [], model.ego_eval
    monkeypatch.setattr(model, "num_hypotheses", K)                              # TEST.NUM_HYPOTHESES, as MLD.__init__ reads it
    monkeypatch.setattr(model, "ego_eval", lambda batch, **kw: (seen.append(ego_eval(batch, **kw)), seen[-1])[1])
    for split in ("test", "val"):
        seen.clear()
        model.SocialMetric.reset(), model.EgoMetric.reset(), model.HypMetric.reset()
        for it in range(2):
            model.allsplit_step(split, dm.batch(3, idx=40 + it, lengths=[16, 12, 7]))
        got = model.SocialMetric.compute()
        social = {n: np.concatenate([rs["social_metrics"][n].double().cpu().numpy() for rs in seen]) for n in NAMES}
        cols = {"MPJPE": [], "ROOT_ERROR": [], "keep": []}
        for rs in seen:
            if K == 1:
                m = {k: v[:, None] for k, v in EgoMetrics.per_sequence(rs["joints_rst"], rs["joints_ref"], rs["lengths"],
                                                                       rs["orientation_quat_rst"], rs["orientation_quat_ref"]).items()}
                keep = keep_mask(m, split, True)
            else:
                m = rs["hyp_metrics"]
                keep = keep_mask(m, split, m["have_quat"])
            cols["MPJPE"].append(m["MPJPE"].double().cpu().numpy()), cols["ROOT_ERROR"].append(m["ROOT_ERROR"].double().cpu().numpy())
            cols["keep"].append(keep.cpu().numpy())
        mp, root, keep = (np.concatenate(cols[n]) for n in ("MPJPE", "ROOT_ERROR", "keep"))
        want = R.np_accumulate(social, mp, root, keep)
        assert set(got) == set(want), split
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-12 * max(abs(want[k]), 1e-300), (split, k, got[k], want[k])
        assert got["count_seq_social"] == 6.0 and sum(got[f"count_seq_gaze_{b}"] for b in ("lt150", "ge150")) == 6.0
        if split == "val":
            assert got["count_pairs_social"] > 0 and any(k.startswith("MPJPE") for k in got)
            ego = model.EgoMetric.compute()                                      # the bins of either axis add up to the unbinned number
            first = "MPJPE" if K == 1 else "MPJPE_best_of_k"
            total = (model.EgoMetric.sums()[0] if K == 1 else model.HypMetric.sums()[0]).item()
            for axis, labels in (("dist", R.np_labels(R.DIST_EDGES)), ("gaze", R.np_labels(R.GAZE_EDGES))):
                s = sum(got.get(f"{first}_{axis}_{b}", 0.0) * got[f"count_kept_{axis}_{b}"] for b in labels)
                assert abs(s - total) <= 1e-5 * total and ego["count_seq"] > 0, (axis, s, total)      # (EgoMetrics adds in fp32)


def test_cli_test_main_reports_the_social_keys_only_when_asked(dev, tmp_path):
    from seeme_amd import cli
    from seeme_amd.social_metrics import SocialMetrics
    cfgp = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    r = cli.train_main(["--cfg", cfgp, "--batch_size", "4", "--nodebug", "--folder", str(tmp_path), "--frames", "24",
                        "--iters_per_epoch", "1", "--epochs", "1"])
    common = ["--cfg", cfgp, "--batch_size", "4", "--folder", str(tmp_path), "--frames", "24", "--test_batches", "2",
              "--checkpoint", os.path.join(r["checkpoints"], "epoch=0.ckpt")]
    today = ("MPJPE", "ROOT_ERROR", "ACCL", "HEAD_ORIENTATION_ERROR", "mpjpe_interactee", "count_seq", "seqs_per_s")
    json_keys = lambda names: {f"Metrics/{n}{s}" for n in names for s in ("", "/mean", "/min", "/max", "/conf_interval")}
    off = json.load(open(cli.test_main(common)["file"]))
    assert set(off) == json_keys(today)                                          # the default file keeps its keys
    out = cli.test_main(common + ["--social_metrics"])
    on = json.load(open(out["file"]))
    new = {k.split("/")[1] for k in set(on) - set(off)}
    assert set(off) <= set(on) and {"PERSON_DIST", "CLOSEST_DIST_REF", "GAZE_ANGLE_REF", "count_seq_social", "count_pairs_social"} <= new
    assert new <= set(SocialMetrics().compute()) | set(SocialMetrics.UNBINNED_SEQ + SocialMetrics.UNBINNED_HYP) | {
        f"{m}_{axis}_{b}" for m in ("MPJPE", "ROOT_ERROR") for axis, edges in (("dist", R.DIST_EDGES), ("gaze", R.GAZE_EDGES))
        for b in R.np_labels(edges)}
    assert out["Metrics/count_seq_social/mean"] == 8.0 and out["Metrics/PERSON_DIST/mean"] > 0
    assert sum(out[f"Metrics/count_seq_dist_{b}/mean"] for b in R.np_labels(R.DIST_EDGES)) == 8.0
