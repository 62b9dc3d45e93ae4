"""The image condition on the HIP path (mld.py:251-255, 887-1017, 1076-1306): stage-2 forward against an oracle restatement with
injected draws, the hand-written glue against the autograd tables, ego_eval's 50-step DDIM loop on the cluster kernel (two tokens)
and on k_den_sample (three), training through the CLI, the captured step and the file data module.  The image token of the
oracle is relu(f) W^T + b in numpy; everything else comes from the pinned oracle pieces."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from oracle import mld_flows as F
from oracle import mld_oracle as O
from seeme_amd import shapes
from seeme_amd.weights_recipe import recipe_state_dict
from test_gpu_flows import TOL_F32, _gen, _mld, _np

pytestmark = pytest.mark.gpu
CFG = "config_mld_image_scene.yaml"
LAYOUTS = {"scene_image": ["text", "image", "scene"], "image": ["text", "image"], "int_scene_image": ["text", "interactee", "scene", "image"]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _model(dev, layout, guidance=1.0, T=16, **kw):
    def mut(cfg):
        cfg.model.condition = list(LAYOUTS[layout])
        cfg.model.guidance_scale = guidance
        for k, v in kw.items():
            node = cfg
            *path, last = k.split(".")
            for p in path:
                node = node[p]
            node[last] = v
    return _mld(dev, CFG, T=T, mutate=mut)


def _batch(dm, model, B, idx, lengths=None):
    return dm.batch(B, idx=idx, with_scene="scene" in model.condition, with_image=True, lengths=lengths)


def _oracle_tokens(model, batch, eps_c=None):
    """[interactee sample, scene token, image token] in the reference's order (:991-1013, :1297-1306), seq-first [N,B,256]."""
    from seeme_amd.mld import split_batch
    motion, transl, _beta, _u, scene, images, length, _ = split_batch(model.condition, batch)
    motion, transl = _np(motion), _np(transl)
    lengths = [int(v) for v in _np(length).reshape(-1)]
    Pv = recipe_state_dict(shapes.vae_shapes(75))
    toks = []
    if "interactee" in model.condition:
        mu, sd = O.vae_encode(Pv, F.person_features(motion, transl, 1, True), lengths)
        toks.append(mu + _np(eps_c) * sd)
    if scene is not None:
        Pos = {k: _np(v) for k, v in model.output_scene.state_dict().items()}
        toks.append(F.scene_token(recipe_state_dict(shapes.pointnet_shapes()), Pos, _np(scene)))     # no input mask with an image
    W, b = _np(model.output_images[1].weight), _np(model.output_images[1].bias)
    toks.append((np.maximum(_np(images), 0.0) @ W.T + b)[None].astype(np.float32))
    return np.concatenate(toks, axis=0), Pv, lengths


# ----------------------------------------------------------------------------- 1: stage-2 forward, injected draws
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("guidance", [1.0, 7.5])
def test_train_diffusion_forward_with_image_vs_oracle(dev, layout, guidance):
    """Batch unpack by layout, [z_cond, scene, image] assembly, add_noise and the denoiser against the oracle; with guidance the
    interactee keeps its input mask and the scene does NOT get one (the image branches of mld.py:889-909)."""
    model, dm, cfg = _model(dev, layout, guidance)
    model.eval()
    B, T = 3, 16
    batch = _batch(dm, model, B, idx=5)
    rn, rm = _gen(21, dev)
    eps_z, eps_c, noise = rn(1, B, 256), rn(1, B, 256), rn(B, 1, 256)
    ts = torch.tensor([999, 0, 417], device=dev)
    m_scene, m_int = rm(0.5, B, dm.n_points, 3), rm(0.1, B, T, 75)
    with torch.no_grad():
        rs = model.train_diffusion_forward(batch, noise=noise, timesteps=ts, eps=(eps_z, eps_c), masks=(m_scene, m_int))
    from seeme_amd.mld import split_batch
    motion, transl = (_np(t) for t in split_batch(model.condition, batch)[:2])
    masked = batch
    if guidance > 1.0 and "interactee" in model.condition:
        f = np.where(_np(m_int), np.float32(0.0), F.person_features(motion, transl, 1, True))
        mm = motion.copy()
        mm[:, :, 1], tt = f[..., :72], transl.copy()
        tt[:, 1] = f[..., 72:]
        masked = tuple(torch.from_numpy(x) for x in (mm, tt)) + tuple(batch[2:])
    cond_emb, Pv, lengths = _oracle_tokens(model, masked, eps_c)
    assert cond_emb.shape[0] == len(LAYOUTS[layout]) - 1
    mu, sd = O.vae_encode(Pv, F.person_features(motion, transl, 1, True), lengths)     # ESTIMATE interactee
    latents = np.transpose(mu + _np(eps_z) * sd, (1, 0, 2))
    noisy = O.ddpm_add_noise(O.alphas_cumprod(O.make_betas()), latents, _np(noise), _np(ts))
    want = O.denoiser_forward(recipe_state_dict(shapes.denoiser_shapes()), noisy, _np(ts), cond_emb)
    assert rel_err(_np(rs["noise_pred"]), want) < 2 * TOL_F32
    if "scene" in model.condition:           # the scene mask is ignored: with it applied the prediction would change
        with torch.no_grad():
            rs2 = model.train_diffusion_forward(batch, noise=noise, timesteps=ts, eps=(eps_z, eps_c), masks=(torch.zeros_like(m_scene), m_int))
        assert rel_err(_np(rs2["noise_pred"]), _np(rs["noise_pred"])) < 1e-6


# ----------------------------------------------------------------------------- 2: glue vs autograd tables
@pytest.mark.parametrize("layout,B,guidance,train", [("scene_image", 5, 1.0, True), ("scene_image", 70, 1.0, True), ("image", 5, 1.0, True),
                                                     ("int_scene_image", 5, 7.5, True), ("int_scene_image", 70, 1.0, False)])
def test_stage2_glue_with_image_matches_autograd_path(dev, layout, B, guidance, train):
    """stage2_glue with the image token (one more k_gg problem forward with the ReLU prologue, K = 2048, and one more weight
    gradient) against TRAIN.HIP_GLUE false: loss, noise prediction and every parameter gradient, output_images included.
    Three tokens at B = 70 run with dropout off: the two paths' tables differ by ~1e-6 (GEMM order), and one of the dropout draws
    of this seed puts a unit of output_blocks.0's FFN ReLU within that of its kink -- its linear1 gradient row then differs by
    5e-3 of the tensor's largest entry while the losses agree to the last bit (both paths run the same chain kernels)."""
    got = []
    for glue in (True, False):
        model, dm, cfg = _model(dev, layout, guidance, **{"TRAIN.HIP_GLUE": glue})
        model.train(train)
        tb = _batch(dm, model, B, idx=3)
        g = torch.Generator().manual_seed(5)
        noise, ts = torch.randn(B, 1, 256, generator=g).to(dev), torch.randint(0, 1000, (B,), generator=g).to(dev)
        eps = (torch.randn(1, B, 256, generator=g).to(dev), torch.randn(1, B, 256, generator=g).to(dev))
        masks = None
        if model.do_classifier_free_guidance:
            masks = ((torch.rand(B, dm.n_points, 3, generator=g) < 0.1).to(dev), (torch.rand(B, 16, 75, generator=g) < 0.1).to(dev))
        out = []
        for it in range(2):
            for p in model.parameters():
                p.grad = None
            rs = model.train_diffusion_forward(tb, noise=noise, timesteps=ts, eps=eps, masks=masks)
            loss = model.losses["train"].update(rs)
            loss.backward()
            out.append((float(loss.detach()), rs["noise_pred"].detach().clone(),
                        {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}))
        assert (getattr(model, "_glue", None) is not None) == glue
        if glue:
            assert any(k[3] for k in model._glue.plans)                  # the plan with the image slot ran
        got.append(out)
    for it in range(2):
        (l1, n1, g1), (l0, n0, g0) = got[0][it], got[1][it]
        assert abs(l1 - l0) < 1e-5 * abs(l0), (it, l1, l0)
        assert rel_err(_np(n1), _np(n0)) < 1e-5
        assert set(g1) == set(g0), set(g1) ^ set(g0)
        assert {"output_images.1.weight", "output_images.1.bias"} <= set(g0)
        assert float(g0["output_images.1.weight"].abs().max()) > 0
        scale = max(float(v.abs().max()) for v in g0.values())
        errs = sorted(((float((g1[k] - g0[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-4 * scale), k) for k in g0), reverse=True)
        assert errs[0][0] < 5e-5, (it, errs[:6])


# ----------------------------------------------------------------------------- 3: ego_eval, 50-step DDIM
class _KernelLog:
    """Records which sampling entry point ran (and the cluster shape) by wrapping the library's two symbols."""

    def __init__(self, monkeypatch):
        from seeme_amd import _lib as L
        lib = L.lib()
        self.calls = []
        cl_fn, one_fn = lib.seeme_denoiser_sample_cluster, lib.seeme_denoiser_sample

        def cluster(w, cl, a, st):
            c = cl._obj
            self.calls.append(("cluster_ms" if c.samples > 1 else "cluster", int(c.C), int(c.samples)))
            return cl_fn(w, cl, a, st)

        def one(w, a, st):
            self.calls.append(("k_den_sample", 0, 1))
            return one_fn(w, a, st)

        monkeypatch.setattr(lib, "seeme_denoiser_sample_cluster", cluster)
        monkeypatch.setattr(lib, "seeme_denoiser_sample", one)


def _oracle_eval(model, dm, batch, lat, eps_c):
    cond_emb, Pv, lengths = _oracle_tokens(model, batch, eps_c)
    z = O.diffusion_reverse(recipe_state_dict(shapes.denoiser_shapes()), np.transpose(cond_emb, (1, 0, 2)), _np(lat), 50)
    feats_rst = O.vae_decode(Pv, z, lengths)
    m_rst = O.renorm(feats_rst, _np(dm.mean), _np(dm.std))
    joints = F.feats_to_joints(O.make_synthetic_smpl(1234), m_rst, _np(batch[2])[:, 1], "egobody", True)   # ESTIMATE interactee
    return z, joints


def test_ego_eval_scene_image_on_the_cluster_kernel_vs_oracle(dev, monkeypatch):
    """[scene, image] is N = 2: the Q variant of k_den_cluster.  fp32 image (the parity mode) against the restated 50-step DDIM loop
    at 1e-3 on joints; the one-CU kernel agrees; a 16-bit image at B = 72 runs k_den_cluster_ms (the default above B = 64)."""
    model, dm, cfg = _model(dev, "scene_image")
    model.eval()
    assert cfg.model.scheduler.num_inference_timesteps == 50 and model.denoiser.weight_dtype == "fp32"
    B, lengths = 3, [16, 16, 11]
    batch = _batch(dm, model, B, idx=6, lengths=lengths)
    rn, _ = _gen(2, dev)
    lat = rn(B, 1, 256)
    log = _KernelLog(monkeypatch)
    rs = model.ego_eval(batch, latents=lat)
    assert log.calls == [("cluster", 8, 1)] and model.denoiser.cluster_status()[0] == 0
    z, joints = _oracle_eval(model, dm, batch, lat, None)
    assert rel_err(_np(rs["lat_t"]), z) < 5 * TOL_F32
    assert rel_err(_np(rs["joints_rst"]), joints) < 1e-3
    model.denoiser.cluster = 0
    rs1 = model.ego_eval(batch, latents=lat)
    assert log.calls[-1] == ("k_den_sample", 0, 1)
    assert rel_err(_np(rs1["lat_t"]), _np(rs["lat_t"])) < 1e-5
    # default large-batch form: 16-bit image, several samples per cluster
    model.denoiser.cluster, model.denoiser.weight_dtype = "auto", "fp16"
    B = 72
    batch = _batch(dm, model, B, idx=7)
    lat = rn(B, 1, 256)
    rs = model.ego_eval(batch, latents=lat)
    assert log.calls[-1][0] == "cluster_ms" and model.denoiser.cluster_status()[0] == 0
    model.denoiser.weight_dtype = "fp32"
    model.denoiser.cluster = 0
    ref = model.ego_eval(batch, latents=lat)
    assert rel_err(_np(rs["lat_t"]), _np(ref["lat_t"])) < 2e-2


def test_ego_eval_interactee_scene_image_on_k_den_sample_vs_oracle(dev, monkeypatch):
    """[interactee, scene, image] is N = 3: past the cluster kernels' two tokens, so k_den_sample runs it."""
    model, dm, cfg = _model(dev, "int_scene_image")
    model.eval()
    B = 3
    batch = _batch(dm, model, B, idx=8)
    rn, _ = _gen(4, dev)
    lat, e_c = rn(B, 1, 256), rn(1, B, 256)
    log = _KernelLog(monkeypatch)
    rs = model.ego_eval(batch, latents=lat, cond_noise=e_c)
    assert log.calls == [("k_den_sample", 0, 1)]
    z, joints = _oracle_eval(model, dm, batch, lat, e_c)
    assert rel_err(_np(rs["lat_t"]), z) < 5 * TOL_F32
    assert rel_err(_np(rs["joints_rst"]), joints) < 1e-3
    model.EgoMetric.reset()
    model.validation_step(batch)
    assert np.isfinite(model.EgoMetric.compute()["MPJPE"])


def test_ego_eval_image_with_guidance_raises(dev):
    for layout in ("scene_image", "image"):
        model, dm, cfg = _model(dev, layout, guidance=2.5)
        model.eval()
        with pytest.raises(NotImplementedError, match="guidance"):
            model.ego_eval(_batch(dm, model, 2, idx=1))


# ----------------------------------------------------------------------------- 4: the CLI
def test_cli_train_and_test_with_image_config(dev, tmp_path):
    """train_main on synthetic image batches with the new YAML: finite loss, output_images trained; the checkpoint reloads
    strictly through test_main."""
    from seeme_amd import cli
    cfgp = os.path.join(REPO, "configs", CFG)
    common = ["--cfg", cfgp, "--batch_size", "4", "--nodebug", "--folder", str(tmp_path), "--frames", "24", "--scene_points", "512"]
    r = cli.train_main(common + ["--epochs", "2", "--iters_per_epoch", "2"])
    assert r["step"] == 4 and np.isfinite(r["total"])
    sd0 = cli.read_checkpoint(os.path.join(r["checkpoints"], "epoch=0.ckpt"))["state_dict"]
    sd1 = cli.read_checkpoint(os.path.join(r["checkpoints"], "epoch=1.ckpt"))["state_dict"]
    assert sd1["output_images.1.weight"].shape == (256, 2048)
    assert not torch.equal(sd0["output_images.1.weight"], sd1["output_images.1.weight"])
    assert not torch.equal(sd0["output_images.1.bias"], sd1["output_images.1.bias"])
    assert torch.equal(sd0["vae.global_motion_token"], sd1["vae.global_motion_token"])                        # frozen
    out = cli.test_main(["--cfg", cfgp, "--batch_size", "4", "--folder", str(tmp_path), "--frames", "24", "--scene_points", "512",
                         "--test_batches", "2", "--checkpoint", os.path.join(r["checkpoints"], "epoch=1.ckpt")])
    assert np.isfinite(out["Metrics/MPJPE/mean"]) and os.path.exists(out["file"])


# ----------------------------------------------------------------------------- 5: captured step
def test_capture_training_step_with_image_replay_equals_eager(dev):
    """capture_training_step with the image features in the static batch: every replay applies exactly the AdamW update of the
    gradients it left in the flat bucket (output_images' among them), and a new batch copied in changes the loss."""
    model, dm, cfg = _model(dev, "scene_image")
    model.train()
    tb = _batch(dm, model, 4, idx=3)
    model.configure_optimizers()
    model.optimizer_step(model.training_step(tb))
    model.optimizer_step(model.training_step(tb))
    replay = model.capture_training_step(tb, warmup=1)
    torch.cuda.synchronize()
    bucket = model.grad_bucket()
    opt = model.optimizer
    w_img = model.output_images[1].weight
    assert any(p is w_img for p in bucket.params)
    losses = []
    for it in range(3):
        p0 = {id(p): p.detach().clone() for p in bucket.params}
        m0 = {id(p): opt.state[p]["exp_avg"].clone() for p in bucket.params}
        v0 = {id(p): opt.state[p]["exp_avg_sq"].clone() for p in bucket.params}
        t = float(opt.state[bucket.params[0]]["step"]) + 1.0
        loss = replay(_batch(dm, model, 4, idx=10) if it == 2 else None)
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        losses.append(float(loss))
        lr, (b1, b2), eps_, wd = (opt.param_groups[0][k] for k in ("lr", "betas", "eps", "weight_decay"))
        worst = 0.0
        for p in bucket.params:
            gth = bucket.views[id(p)].double()
            m = m0[id(p)].double() * b1 + (1 - b1) * gth
            v = v0[id(p)].double() * b2 + (1 - b2) * gth * gth
            want = p0[id(p)].double() * (1 - lr * wd) - lr / (1 - b1 ** t) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps_)
            worst = max(worst, float((p.detach().double() - want).abs().max() / want.abs().max().clamp_min(1e-12)))
        assert worst < 1e-5, (it, worst)
        assert float(bucket.views[id(w_img)].abs().max()) > 0
    assert losses[2] != losses[1]


# ----------------------------------------------------------------------------- 6: file data module
def test_data_module_image_features_feed_training_and_eval(dev, tmp_path):
    """EgoDataModule with image_feats_<split>.npz: the table lives on the device, frames are drawn there per access, and the
    batches drive a training step and an evaluation step."""
    from test_data_module import write_dataset
    from test_image_condition_cpu import write_image_feats
    from seeme_amd import data as D
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD
    from seeme_amd.smpl import SMPL
    from seeme_amd.weights_recipe import load_recipe_
    root = str(tmp_path / "egobody")
    items, _ = write_dataset(root, "egobody", n=9, T=12, P=64, full_every=4)
    write_image_feats(root, items)
    dm = D.EgoDataModule(root, "egobody", condition=("text", "image", "scene"), motion_length=12, device=dev, scene_root=root)
    assert dm.splits["train"].image_table.is_cuda and dm.splits["train"].image_table.dtype == torch.float16
    cfg = parse_config(os.path.join(REPO, "configs", CFG))
    cfg.model.scheduler.num_inference_timesteps = 5
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser), load_recipe_(model.proscene.scene_enc)
    model = model.to(dev).train()
    for it in range(3):
        batch = dm.batch(4, idx=it, split="train")
        assert len(batch) == 7 and batch[5].shape == (4, 2048) and batch[5].is_cuda and batch[5].dtype == torch.float32
        loss = model.training_step(batch)
        model.optimizer_step(loss)
        assert np.isfinite(float(loss))
    assert getattr(model, "_glue", None) is not None
    model.eval()
    model.EgoMetric.reset()
    for b in dm.iterate("test", 4):
        out = model.validation_step(b)
        assert out is None or torch.isfinite(out)
    got = model.EgoMetric.compute()
    assert np.isfinite(got["MPJPE"]) and got["count_seq"] > 0
    for b in dm.iterate("test", 4):
        assert model.test_step(b).shape[1:] == (12, 24, 3)
