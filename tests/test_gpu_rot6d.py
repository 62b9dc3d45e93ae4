"""DATA_TYPE rot6d on the GPU: the fused joints kernels (seeme_smpl_joints_rot6d / _backward) against the two-launch route and the
float64 autograd twin, the stage-1 step with the hand-written backward against the autograd twins, the stage-2 step, evaluation,
the graph-captured step and the CLI on synthetic rot6d batches.  Every Gram-Schmidt input comes from test_rot6d_cpu.make_rot6d
(rotations + 0.1 noise, conditioning asserted on the CPU, no joint dropped)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from test_rot6d_cpu import make_rot6d

pytestmark = pytest.mark.gpu
TOL_F32 = 1e-4
M9 = 9            # three workgroups of four frames, the last with one live wave


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def smpl(dev):
    from seeme_amd.smpl import SMPL
    return SMPL.synthetic(1234).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(M, order, dev, seed=21):
    r6, _ = make_rot6d(M, seed, order)
    g = torch.Generator().manual_seed(seed + 1)
    betas = 0.5 * torch.randn(M, 10, generator=g, dtype=torch.float64)
    tr = torch.randn(M, 3, generator=g, dtype=torch.float64)
    wgt = torch.randn(M, 24, 3, generator=g, dtype=torch.float64)
    return r6.to(dev), betas.to(dev), tr.to(dev), wgt.to(dev)


def _grads(fn, r6, tr, wgt):
    """(joints, d r6, d transl) of sum(joints * wgt) through fn(r6, tr)."""
    a = r6.clone().requires_grad_(True)
    t = None if tr is None else tr.clone().requires_grad_(True)
    j = fn(a, t)
    (j * wgt.to(j.dtype)).sum().backward()
    return j.detach(), a.grad.detach(), None if t is None else t.grad.detach()


# ----------------------------------------------------------------------------- 6: forward
@pytest.mark.parametrize("order", ["prohmr", "diffusion"])
def test_forward_equals_two_launch_route_and_float64_twin(dev, smpl, order):
    from seeme_amd import geometry as G
    from seeme_amd.smpl import smpl_joints_rot6d_hip
    from seeme_amd.vae_autograd import smpl_joints_rot6d_torch
    r6, betas, tr, _ = _inputs(M9, order, dev)
    for with_bt in (True, False):
        b64, t64 = (betas, tr) if with_bt else (None, None)
        b32, t32 = (betas.float(), tr.float()) if with_bt else (None, None)
        got = smpl_joints_rot6d_hip(smpl, b32, r6.float(), t32, order)
        assert got.shape == (M9, 24, 3) and got.dtype == torch.float32
        R = G.rot6d_to_rotmat(r6.float().reshape(-1, 6), order).reshape(M9, 24, 3, 3)
        two = smpl(betas=b32 if with_bt else torch.zeros(M9, 10, device=dev), body_pose=R[:, 1:], global_orient=R[:, 0:1], pose2rot=False,
                   return_verts=False, transl=t32).joints[:, :24]
        want = smpl_joints_rot6d_torch(smpl, b64, r6, t64, order)
        e2, e64 = rel_err(_np(got), _np(two)), rel_err(_np(got), _np(want))
        print(f"forward {order} betas/transl={with_bt}: vs two launches {e2:.3e}, vs float64 twin {e64:.3e}")
        # fp32 rounding only: the deepest SMPL joint sits 9 hops from the root, a hop of the chain is a 3-term product sum plus the
        # translation (4 roundings), Gram-Schmidt adds about 8 more: 44 roundings of 2^-24 against float64, twice that between two
        # fp32 routes that round differently (worst case; the typical figure is several times smaller)
        assert e64 < 44 * 2.0 ** -24 and e2 < 88 * 2.0 ** -24
    # r6 as [M,144]: the same joints, and a gradient in the input's own shape
    flat = r6.float().reshape(M9, 144).clone().requires_grad_(True)
    j = smpl_joints_rot6d_hip(smpl, None, flat, None, order)
    assert torch.equal(j.detach(), smpl_joints_rot6d_hip(smpl, None, r6.float(), None, order))
    j.sum().backward()
    a = r6.float().clone().requires_grad_(True)
    smpl_joints_rot6d_hip(smpl, None, a, None, order).sum().backward()
    assert flat.grad.shape == (M9, 144) and torch.equal(flat.grad, a.grad.reshape(M9, 144))
    # transl = None means none: the module's own `transl` parameter (smplx picks it up in forward()) is not added
    old = smpl.transl.data.clone()
    try:
        smpl.transl.data.fill_(5.0)
        assert torch.equal(smpl_joints_rot6d_hip(smpl, None, r6.float(), None, order), j.detach())
    finally:
        smpl.transl.data.copy_(old)
    with pytest.raises(ValueError):
        smpl_joints_rot6d_hip(smpl, None, r6.float(), None, "bogus")


# ----------------------------------------------------------------------------- 7: backward
def _backward_errors(dev, smpl, M, order, with_bt=True, seed=21):
    """Errors of the gradients w.r.t. r6 and transl against autograd through the FLOAT64 twin: of the HIP kernel, and of autograd
    through the fp32 twin on the same input (= fp32 rounding of this very computation; the kernel is allowed 4x that)."""
    from seeme_amd.smpl import smpl_joints_rot6d_hip
    from seeme_amd.vae_autograd import smpl_joints_rot6d_torch
    r6, betas, tr, wgt = _inputs(M, order, dev, seed)
    if not with_bt:
        betas, tr = None, None
    f32 = lambda x: None if x is None else x.float()
    ref = _grads(lambda a, t: smpl_joints_rot6d_torch(smpl, betas, a, t, order), r6, tr, wgt)
    tw32 = _grads(lambda a, t: smpl_joints_rot6d_torch(smpl, f32(betas), a, t, order), r6.float(), f32(tr), wgt)
    hip = _grads(lambda a, t: smpl_joints_rot6d_hip(smpl, f32(betas), a, t, order), r6.float(), f32(tr), wgt)
    assert hip[1].shape == (M, 24, 6) and torch.isfinite(hip[1]).all()
    out = {"r6": (rel_err(_np(hip[1]), _np(ref[1])), rel_err(_np(tw32[1]), _np(ref[1])))}
    if with_bt:
        out["transl"] = (rel_err(_np(hip[2]), _np(ref[2])), rel_err(_np(tw32[2]), _np(ref[2])))
    return out, hip, ref


@pytest.mark.parametrize("M,order,with_bt", [(M9, "prohmr", True), (M9, "diffusion", True), (M9, "prohmr", False), (1, "prohmr", True)])
def test_backward_matches_float64_autograd(dev, smpl, M, order, with_bt):
    """Gradients w.r.t. r6 and transl against autograd through the float64 twin.  The bound is 4x the error of autograd through the
    fp32 twin on the same input (fp32 rounding of this very computation; neither side sums in the other's order), under the 1e-4
    ceiling of the axis-angle kernel's test.  Both figures are printed per case."""
    errs, _, _ = _backward_errors(dev, smpl, M, order, with_bt)
    for k, (e_hip, e_tw) in errs.items():
        print(f"backward M={M} {order} betas/transl={with_bt} d{k}: kernel {e_hip:.3e}, fp32 twin {e_tw:.3e}, ratio {e_hip / max(e_tw, 1e-30):.2f}")
    for k, (e_hip, e_tw) in errs.items():
        assert e_hip < 1e-4, (k, e_hip)                      # the sanity ceiling of the axis-angle kernel's test
        assert e_hip <= 4 * e_tw, (k, e_hip, e_tw)


def test_backward_takes_the_45_joint_gradient_layout(dev, smpl):
    """dj_stride = 45: the joints gradient handed over as [M,45,3] (rows 24.. are not read) gives the gradients of dj_stride = 24."""
    from seeme_amd import _lib as L
    r6, betas, tr, wgt = _inputs(M9, "prohmr", dev)
    r6, betas, wgt = r6.float().contiguous(), betas.float().contiguous(), wgt.float().contiguous()
    model = smpl._model()
    dj45 = torch.full((M9, 45, 3), float("nan"), device=dev)
    dj45[:, :24] = wgt
    out = []
    for dj, stride in ((wgt, 24), (dj45, 45)):
        dr6, dtr = torch.zeros(M9, 24, 6, device=dev), torch.zeros(M9, 3, device=dev)
        L.check(L.lib().seeme_smpl_joints_rot6d_backward(C.byref(model), betas.data_ptr(), r6.data_ptr(), L.GEO_ROT6D_PROHMR, dj.data_ptr(),
                                                         stride, dr6.data_ptr(), dtr.data_ptr(), M9, L.current_stream()))
        out.append((dr6, dtr))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.isfinite(out[1][0]).all()


def test_frames_past_M_are_not_written(dev, smpl):
    """M = 5 of a buffer of 8 frames: the three dead waves of the second workgroup leave joints, dr6 and dtransl untouched."""
    from seeme_amd import _lib as L
    r6, _, tr, wgt = _inputs(8, "prohmr", dev)
    r6, tr, wgt = r6.float().contiguous(), tr.float().contiguous(), wgt.float().contiguous()
    model = smpl._model()
    joints, dr6, dtr = (torch.full(s, 7.0, device=dev) for s in ((8, 24, 3), (8, 24, 6), (8, 3)))
    L.check(L.lib().seeme_smpl_joints_rot6d(C.byref(model), 0, r6.data_ptr(), L.GEO_ROT6D_PROHMR, tr.data_ptr(), 5, joints.data_ptr(),
                                            L.current_stream()))
    L.check(L.lib().seeme_smpl_joints_rot6d_backward(C.byref(model), 0, r6.data_ptr(), L.GEO_ROT6D_PROHMR, wgt.data_ptr(), 24, dr6.data_ptr(),
                                                     dtr.data_ptr(), 5, L.current_stream()))
    for t in (joints, dr6, dtr):
        assert bool((t[5:] == 7.0).all()) and not bool((t[:5] == 7.0).any())


# ----------------------------------------------------------------------------- 8: degenerate joint
def test_degenerate_joint_is_finite_and_the_others_match(dev, smpl):
    """One frame with a1 = 0 at joint 7 (F.normalize: b1 = 0, the clamped norm carries no gradient): the output and all gradients are
    finite, the joints equal the twin's, and the gradients of the other 23 joints match the float64 twin at the bound of the backward
    test (4x the fp32 twin's own error, measured over the same 23 joints)."""
    from seeme_amd.smpl import smpl_joints_rot6d_hip
    from seeme_amd.vae_autograd import smpl_joints_rot6d_torch
    r6, _, tr, wgt = _inputs(1, "prohmr", dev, seed=33)
    r6[0, 7, :3] = 0.0
    ref = _grads(lambda a, t: smpl_joints_rot6d_torch(smpl, None, a, t), r6, tr, wgt)
    tw32 = _grads(lambda a, t: smpl_joints_rot6d_torch(smpl, None, a, t), r6.float(), tr.float(), wgt)
    hip = _grads(lambda a, t: smpl_joints_rot6d_hip(smpl, None, a, t), r6.float(), tr.float(), wgt)
    assert all(torch.isfinite(x).all() for x in hip) and all(torch.isfinite(x).all() for x in ref)
    assert rel_err(_np(hip[0]), _np(ref[0])) < 1e-6
    others = [j for j in range(24) if j != 7]
    e_hip, e_tw = rel_err(_np(hip[1][:, others]), _np(ref[1][:, others])), rel_err(_np(tw32[1][:, others]), _np(ref[1][:, others]))
    e7 = rel_err(_np(hip[1][:, 7]), _np(ref[1][:, 7]))
    print(f"degenerate joint: other 23 joints kernel {e_hip:.3e}, fp32 twin {e_tw:.3e}; joint 7 (gradients ~1e12, the 1 / 1e-12 of the clamp) {e7:.3e}")
    assert e_hip < 1e-4 and e_hip <= 4 * e_tw
    assert rel_err(_np(hip[2]), _np(ref[2])) < 1e-5


# ----------------------------------------------------------------------------- 11: the axis-angle kernel is left alone
def test_axis_angle_backward_unchanged_around_a_rot6d_call(dev, smpl):
    """seeme_smpl_joints_backward before and after a call of the new kernels on the same buffers: bit-equal (nothing shared is
    clobbered; the factored tree walk itself is pinned by test_gpu_parity.test_smpl_joints_backward_matches_autograd)."""
    from seeme_amd import _lib as L
    g = torch.Generator().manual_seed(8)
    M = M9
    betas = (torch.randn(M, 10, generator=g) * 0.5).to(dev)
    pose = (torch.randn(M, 72, generator=g) * 0.5).to(dev)
    wgt = torch.randn(M, 24, 3, generator=g).to(dev)
    r6 = make_rot6d(M, 21)[0].float().to(dev).contiguous()
    model = smpl._model()
    lib, st = L.lib(), L.current_stream()

    def aa_bwd():
        dpose, dtr = torch.zeros(M, 72, device=dev), torch.zeros(M, 3, device=dev)
        L.check(lib.seeme_smpl_joints_backward(C.byref(model), betas.data_ptr(), pose.data_ptr(), wgt.data_ptr(), 24, dpose.data_ptr(),
                                               dtr.data_ptr(), M, st))
        return dpose, dtr

    before = aa_bwd()
    joints, dr6, dtr = torch.empty(M, 24, 3, device=dev), torch.empty(M, 24, 6, device=dev), torch.empty(M, 3, device=dev)
    L.check(lib.seeme_smpl_joints_rot6d(C.byref(model), betas.data_ptr(), r6.data_ptr(), L.GEO_ROT6D_PROHMR, 0, M, joints.data_ptr(), st))
    L.check(lib.seeme_smpl_joints_rot6d_backward(C.byref(model), betas.data_ptr(), r6.data_ptr(), L.GEO_ROT6D_PROHMR, wgt.data_ptr(), 24,
                                                 dr6.data_ptr(), dtr.data_ptr(), M, st))
    after = aa_bwd()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and float(before[0].abs().max()) > 0


# ----------------------------------------------------------------------------- 9 / 10: the stages
def _mld(dev, cfg_name, T=8, mutate=None):
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    from seeme_amd.weights_recipe import load_recipe_
    cfg = parse_config(os.path.join(REPO, "configs", cfg_name))
    if mutate:
        mutate(cfg)
    dm = SyntheticEgoDataModule(nfeats=144, T=T, device=dev, data_type="rot6d")
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser)
    return model.to(dev), dm, cfg


def test_stage1_step_hip_backward_matches_autograd_twins(dev):
    """config_vae_egobody_rot6d, B = 3, T = 8, injected eps: loss, m_rst and EVERY VAE parameter gradient with TRAIN.HIP_VAE_BACKWARD
    true (vae_train.py + smpl._JointsRot6d) against false (the autograd twins), at the bounds of the 'angle' comparison
    (tests/test_gpu_flows.py:515-520: loss 1e-5, m_rst 2e-5, gradients 1e-4 of max(own largest entry, 1e-4 of the model's largest))."""
    B, T = 3, 8
    got = []
    for hip in (True, False):
        def mut(cfg):
            cfg.TRAIN.HIP_VAE_BACKWARD = hip
        model, dm, cfg = _mld(dev, "config_vae_egobody_rot6d.yaml", T=T, mutate=mut)
        model.train()
        model.vae.eval()                                     # dropout off on both sides (the twin's arithmetic)
        tb = dm.batch(B, idx=4)
        assert tb[0].shape == (B, T, 2, 144)
        eps = torch.randn(1, B, 256, generator=torch.Generator().manual_seed(11)).to(dev)
        out = []
        for it in range(2):                                  # twice: the second step runs on vae_train's recorded launch lists
            for p in model.parameters():
                p.grad = None
            rs = model.train_vae_forward(tb, eps=eps)
            assert rs["m_ref"].shape == (B, T, 144) and rs["m_rst"].shape == (B, T, 144)
            assert rs["joints_ref"].shape == (B, T, 24, 3) and rs["joints_rst"].shape == (B, T, 24, 3)
            loss = model.losses["train"].update(rs)
            loss.backward()
            out.append((float(loss.detach()), rs["m_rst"].detach().clone(), rs["joints_rst"].detach().clone(),
                        {k: v.grad.detach().clone() for k, v in model.vae.named_parameters() if v.grad is not None}))
        assert (getattr(model, "_vae_tr", None) is not None) == hip
        got.append(out)
    for it in range(2):
        (l1, m1, j1, g1), (l0, m0, j0, g0) = got[0][it], got[1][it]
        scale = max(float(v.abs().max()) for v in g0.values())
        errs = sorted(((float((g1[k] - g0[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-4 * scale), k) for k in g0), reverse=True)
        print(f"stage-1 rot6d step {it}: loss {l1:.6f} / {l0:.6f}, m_rst {rel_err(_np(m1), _np(m0)):.3e}, joints {rel_err(_np(j1), _np(j0)):.3e}, "
              f"worst gradient {errs[0][0]:.3e} ({errs[0][1]})")
        assert abs(l1 - l0) < 1e-5 * abs(l0), (it, l1, l0)
        assert rel_err(_np(m1), _np(m0)) < 2e-5
        assert set(g0) <= set(g1), set(g0) - set(g1)
        assert errs[0][0] < 1e-4, (it, errs[:6])


def test_data_module_encodes_on_the_device(dev, tmp_path):
    """EgoDataModule(data_type='rot6d') bound for the device converts with seeme_amd.geometry's kernel: the split equals the one a
    CPU data module builds with plain torch, to fp32 rounding of the conversion (both are fp32; sin / cos of the half angle, one
    normalisation and two products per entry: 1e-6 on entries of size <= 1, divided by std >= 0.5), and feeds a stage-1 forward."""
    from seeme_amd import data as D
    from test_rot6d_cpu import _write_egobody
    root = str(tmp_path / "egobody")
    T = 5
    _write_egobody(root, 3, T)
    kw = dict(condition=("text", "interactee"), motion_length=T, splits=("train",), data_type="rot6d", pose_estimation_task=True)
    on_dev, on_cpu = D.EgoDataModule(root, "egobody", device=dev, **kw), D.EgoDataModule(root, "egobody", device="cpu", **kw)
    sd, sc = on_dev.splits["train"], on_cpu.splits["train"]
    assert sd.motion.is_cuda and sd.encode_device.type == "cuda" and sc.encode_device.type == "cpu" and not sc.motion.is_cuda
    assert sd.motion.shape == (3, T, 2, 144)
    for a, b in ((sd.motion, sc.motion), (sd.pe_motion, sc.pe_motion)):
        e = float((a.cpu() - b).abs().max())
        print(f"device encoder vs torch encoder: {e:.3e}")
        assert e < 2e-6
    assert torch.equal(sd.transl.cpu(), sc.transl)
    x = on_dev.renorm(sd.motion[:, :, 0].contiguous())
    assert x.shape == (3, T, 144) and float((x - (sc.motion[:, :, 0] * on_cpu.std[0, :144] + on_cpu.mean[0, :144]).to(dev)).abs().max()) < 2e-6


def test_stage2_step_eval_and_captured_step(dev):
    """config_mld_egobody_rot6d, B = 3, T = 8, 5 DDIM steps: train_diffusion_forward gives a finite loss and finite gradients (144-wide
    encodes, no translation column); ego_eval runs and its joints are _feats_to_joints of the decoded features; the graph-captured
    training step replays bit-identically in two models of the same seed."""
    def mut(cfg):
        cfg.model.scheduler.num_inference_timesteps = 5
    B, T = 3, 8
    model, dm, cfg = _mld(dev, "config_mld_egobody_rot6d.yaml", T=T, mutate=mut)
    model.train()
    tb = dm.batch(B, idx=2)
    f = model._wearer_features(tb[0].float(), tb[1].float(), 1)
    assert f.shape == (B, T, 144)
    for p in model.parameters():
        p.grad = None
    loss = model.losses["train"].update(model.train_diffusion_forward(tb))
    loss.backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in model.denoiser.parameters() if p.grad is not None]
    assert torch.isfinite(loss) and grads and all(torch.isfinite(x).all() for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
    assert all(p.grad is None for p in model.vae.parameters())              # frozen in stage 2
    model.eval()
    g = torch.Generator().manual_seed(3)
    lat, e_c = torch.randn(B, 1, 256, generator=g).to(dev), torch.randn(1, B, 256, generator=g).to(dev)
    rs = model.ego_eval(tb, latents=lat, cond_noise=e_c)
    assert rs["m_rst"].shape == (B, T, 144) and rs["joints_rst"].shape == (B, T, 24, 3) and rs["orientation_quat_rst"] is None
    assert torch.isfinite(rs["joints_rst"]).all()
    assert torch.equal(rs["joints_rst"], model._feats_to_joints(rs["m_rst"], tb[2][:, 0].float()))
    assert torch.equal(rs["joints_ref"], model._feats_to_joints(rs["m_ref"], tb[2][:, 0].float()))
    del model
    runs = []
    for _ in range(2):
        model, dm, cfg = _mld(dev, "config_mld_egobody_rot6d.yaml", T=T, mutate=mut)
        model.eval()                                             # no dropout draws: the two models see the same numbers
        tb = dm.batch(B, idx=2)
        model.configure_optimizers()
        torch.manual_seed(11)
        model.optimizer_step(model.training_step(tb))
        replay = model.capture_training_step(tb, warmup=1)
        torch.cuda.synchronize()
        losses = [float(replay().detach()), float(replay().detach())]
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in losses)
        runs.append((losses, torch.cat([p.detach().flatten() for p in model.denoiser.parameters()]).clone()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def test_cli_trains_both_stages_and_tests_on_rot6d(dev, tmp_path):
    """train.py --cfg config_vae_egobody_rot6d.yaml, then config_mld_egobody_rot6d.yaml with that VAE as TRAIN.PRETRAINED_VAE, then
    test.py on the result: what the three command lines do, through cli.train_main / cli.test_main on synthetic batches."""
    from seeme_amd import cli
    small = ["--batch_size", "4", "--folder", str(tmp_path), "--frames", "8"]
    vae_cfg, mld_cfg = (os.path.join(REPO, "configs", n) for n in ("config_vae_egobody_rot6d.yaml", "config_mld_egobody_rot6d.yaml"))
    r1 = cli.train_main(["--cfg", vae_cfg, "--nodebug", "--epochs", "1", "--iters_per_epoch", "2"] + small)
    assert r1["step"] == 2 and np.isfinite(r1["total"])
    ck1 = os.path.join(r1["checkpoints"], "epoch=0.ckpt")
    sd1 = cli.read_checkpoint(ck1)["state_dict"]
    assert sd1["vae.skel_embedding.weight"].shape[1] == 144 and sd1["vae.final_layer.weight"].shape[0] == 144
    assets = tmp_path / "assets.yaml"
    assets.write_text(f"TRAIN:\n  PRETRAINED_VAE: {ck1}\n")
    r2 = cli.train_main(["--cfg", mld_cfg, "--cfg_assets", str(assets), "--nodebug", "--epochs", "1", "--iters_per_epoch", "2"] + small)
    assert r2["step"] == 2 and np.isfinite(r2["total"])
    ck2 = os.path.join(r2["checkpoints"], "epoch=0.ckpt")
    sd2 = cli.read_checkpoint(ck2)["state_dict"]
    assert torch.equal(sd2["vae.final_layer.weight"], sd1["vae.final_layer.weight"])              # the frozen stage-1 VAE
    out = cli.test_main(["--cfg", mld_cfg, "--test_batches", "2", "--checkpoint", ck2] + small)
    assert np.isfinite(out["Metrics/MPJPE/mean"])
