"""DATA_TYPE rot6d, host side: the float64 autograd twin of the fused joints kernels (finite differences, and the axis-angle twin it must
agree with), the rot6d data module on files written in the reference's on-disk layout, the synthetic rot6d batches, and the C-ABI
surface of the two new entry points."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO


def make_rot6d(M, seed, order="prohmr", dtype=torch.float64):
    """Test inputs of every Gram-Schmidt check: the encoding of random rotations plus noise of scale 0.1 per element, with the
    conditioning asserted on the CPU: every joint has ||a1|| > 0.3 and ||a2 - (b1 . a2) b1|| > 0.3 (orthonormal columns perturbed by
    0.1: a wide margin; no joint is dropped).  Returns (r6 [M,24,6], the axis-angle poses [M,72] the rotations came from)."""
    from seeme_amd import geometry as G
    g = torch.Generator().manual_seed(seed)
    aa = 0.7 * torch.randn(M, 72, generator=g, dtype=torch.float64)
    R = G.aa_to_rotmat_torch(aa.reshape(-1, 3))
    r6 = G.rotmat_to_rot6d(R, order) + 0.1 * torch.randn(M * 24, 6, generator=g, dtype=torch.float64)
    x = r6.reshape(-1, 2, 3).permute(0, 2, 1) if order == "prohmr" else r6.reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = a1 / a1.norm(dim=1, keepdim=True)
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    assert float(a1.norm(dim=1).min()) > 0.3 and float(u.norm(dim=1).min()) > 0.3, (seed, float(a1.norm(dim=1).min()), float(u.norm(dim=1).min()))
    return r6.reshape(M, 24, 6).to(dtype), aa


# ----------------------------------------------------------------------------- the oracle itself
def test_twin_float64_gradcheck():
    """torch.autograd.gradcheck of smpl_joints_rot6d_torch in float64 (M = 3, the synthetic SMPL model): both element orders, with
    betas + translation and with neither."""
    from seeme_amd.smpl import SMPL
    from seeme_amd.vae_autograd import smpl_joints_rot6d_torch
    smpl = SMPL.synthetic(1234)
    g = torch.Generator().manual_seed(5)
    betas = 0.5 * torch.randn(3, 10, generator=g, dtype=torch.float64)
    for order in ("prohmr", "diffusion"):
        r6, _ = make_rot6d(3, 11, order)
        r6.requires_grad_(True)
        tr = torch.randn(3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
        assert smpl_joints_rot6d_torch(smpl, betas, r6, tr, order).dtype == torch.float64
        assert torch.autograd.gradcheck(lambda a, b: smpl_joints_rot6d_torch(smpl, betas, a, b, order), (r6, tr))
        assert torch.autograd.gradcheck(lambda a: smpl_joints_rot6d_torch(smpl, None, a, None, order), (r6,))


def test_twin_forward_equals_the_axis_angle_twin():
    """Axis-angle -> rotation matrices -> the model-side element order -> joints equal smpl_joints_torch on the axis-angle pose, to
    1e-6 relative in float64 (the two conversions regularise the angle differently: ||aa + 1e-8||, a 1e-8 effect)."""
    from seeme_amd import geometry as G
    from seeme_amd.smpl import SMPL
    from seeme_amd.vae_autograd import smpl_joints_rot6d_torch, smpl_joints_torch
    smpl = SMPL.synthetic(1234).double()
    g = torch.Generator().manual_seed(2)
    M = 6
    aa = 0.7 * torch.randn(M, 72, generator=g, dtype=torch.float64)
    betas = 0.5 * torch.randn(M, 10, generator=g, dtype=torch.float64)
    tr = torch.randn(M, 3, generator=g, dtype=torch.float64)
    want = smpl_joints_torch(smpl, betas, aa, tr)
    R = G.aa_to_rotmat_torch(aa.reshape(-1, 3))
    for order in ("prohmr", "diffusion"):
        got = smpl_joints_rot6d_torch(smpl, betas, G.rotmat_to_rot6d(R, order).reshape(M, 24, 6), tr, order)
        err = float((got - want).abs().max() / want.abs().max())
        print(f"rot6d twin vs axis-angle twin ({order}): {err:.3e}")
        assert err < 1e-6
    # zero betas = no betas
    a = smpl_joints_rot6d_torch(smpl, None, G.rotmat_to_rot6d(R, "prohmr").reshape(M, 24, 6))
    b = smpl_joints_rot6d_torch(smpl, torch.zeros(M, 10, dtype=torch.float64), G.rotmat_to_rot6d(R, "prohmr").reshape(M, 24, 6))
    assert torch.equal(a, b)


def test_degenerate_joint_follows_the_normalize_convention_in_the_twin():
    """a1 = 0 at one joint: F.normalize divides by max(||.||, 1e-12), so b1 = 0, b2 = normalize(a2), b3 = 0 and every gradient is
    finite (the clamped norm carries none)."""
    from seeme_amd.vae_autograd import rot6d_to_rotmat_torch
    x = torch.tensor([[0.0, 0.0, 0.0, 0.3, -0.4, 1.2]], dtype=torch.float64, requires_grad=True)
    R = rot6d_to_rotmat_torch(x)
    assert torch.equal(R[0, :, 0], torch.zeros(3, dtype=torch.float64)) and torch.equal(R[0, :, 2], torch.zeros(3, dtype=torch.float64))
    assert torch.allclose(R[0, :, 1], x.detach()[0, 3:] / x.detach()[0, 3:].norm())
    R.sum().backward()
    assert torch.isfinite(x.grad).all()


def test_rotmat_to_rot6d_orders_invert_rot6d_to_rotmat():
    from seeme_amd import geometry as G
    from seeme_amd.vae_autograd import rot6d_to_rotmat_torch
    g = torch.Generator().manual_seed(4)
    R = G.aa_to_rotmat_torch(torch.randn(8, 3, generator=g, dtype=torch.float64))
    d = G.rotmat_to_rot6d(R)                                   # the dataset's default: 'diffusion'
    assert torch.equal(d, torch.stack([R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 0], R[:, 2, 1]], dim=1))
    p = G.rotmat_to_rot6d(R, "prohmr")
    assert torch.equal(p, torch.cat([R[:, :, 0], R[:, :, 1]], dim=1))
    for mode, x in (("diffusion", d), ("prohmr", p)):
        assert float((rot6d_to_rotmat_torch(x, mode) - R).abs().max()) < 1e-12
    with pytest.raises(ValueError):
        G.rotmat_to_rot6d(R, "bogus")


# ----------------------------------------------------------------------------- data
def _write_egobody(root, n=3, T=5, seed=0, rot6d_stats=True):
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    np.save(os.path.join(root, "mean.npy"), rng.standard_normal((1, 75)).astype(np.float32) * 0.1)
    np.save(os.path.join(root, "std.npy"), (0.5 + rng.random((1, 75))).astype(np.float32))
    if rot6d_stats:
        np.save(os.path.join(root, "mean_rot6d.npy"), rng.standard_normal((1, 144)).astype(np.float32) * 0.1)
        np.save(os.path.join(root, "std_rot6d.npy"), (0.5 + rng.random((1, 144))).astype(np.float32))
    items = []
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    for i in range(n):
        L = T if i == 0 else T - i                              # one full-length item, two padded ones
        person = lambda: {"global_orient": rng.standard_normal((L, 1, 3)), "transl": rng.standard_normal((L, 1, 3)),
                          "body_pose": rng.standard_normal((L, 1, 69)) * 0.3, "betas": np.repeat(rng.standard_normal((1, 1, 10)), L, 0)}
        it = {"video": [f"frame_{k}" for k in range(L)],
              "recording_utils": {"original_imgname": [f"egocentric_color/rec_{i}/d/PV/{1000 + k}_frame_{k:05d}.jpg" for k in range(L)],
                                  "fx": list(rng.random(L)), "cx": list(rng.random(L)), "cy": list(rng.random(L)),
                                  "center": rng.random((L, 2)), "scale": list(rng.random(L))},
              "wearer": person(), "interactee": person()}
        np.save(os.path.join(root, "train", f"seq_{i:03d}.npy"), it, allow_pickle=True)
        items.append(it)
    return items


def test_data_module_rot6d(tmp_path):
    from seeme_amd import data as D
    from seeme_amd import geometry as G
    root = str(tmp_path / "egobody")
    T = 5
    items = _write_egobody(root, 3, T)
    dm = D.EgoDataModule(root, "egobody", condition=("text", "interactee"), motion_length=T, device="cpu", splits=("train",),
                         data_type="rot6d", pose_estimation_task=True)
    assert dm.nfeats == 144 and dm.numdims == 144
    s = dm.splits["train"]
    assert tuple(s.motion.shape) == (3, T, 2, 144) and (s.numdims, s.go_dims) == (144, 6)
    mean, std = np.load(os.path.join(root, "mean_rot6d.npy")), np.load(os.path.join(root, "std_rot6d.npy"))
    assert np.array_equal(dm.mean.numpy(), mean) and np.array_equal(dm.std.numpy(), std)
    # the renorm width follows numdims; the data module renorms on the device, so the same formula is applied here on the CPU
    renormed = s.motion.double() * torch.from_numpy(std[0, :144]).double() + torch.from_numpy(mean[0, :144]).double()
    for i, it in enumerate(items):
        L = len(it["video"])
        assert int(s.length[i]) == L
        for p, who in enumerate(("wearer", "interactee")):
            aa = np.concatenate([np.asarray(it[who]["global_orient"]).reshape(L, 3), np.asarray(it[who]["body_pose"]).reshape(L, 69)], 1)
            R = G.aa_to_rotmat_torch(torch.from_numpy(aa).double().reshape(-1, 3)).reshape(L, 24, 3, 3)
            got = renormed[i, :L, p].reshape(L, 24, 3, 2)                      # [go 6 | body 138], 'diffusion' order: rows x 2 columns
            assert float((got - R[..., :2]).abs().max()) < 1e-6
            # frames past the length: zeros in rot6d space before the normalisation, i.e. renorm gives 0
            if L < T:
                assert float(renormed[i, L:, p].abs().max()) < 1e-6 and float(s.transl[i, p, L:].abs().max()) == 0.0
            # translation raw, betas as stored
            assert np.allclose(s.transl[i, p, :L].numpy(), np.asarray(it[who]["transl"], np.float32).reshape(L, 3), rtol=0, atol=0)
        # POSE_ESTIMATION ground truth: the interactee's own pose, re-encoded the same way
        assert tuple(s.pe_motion.shape) == (3, T, 1, 144) and torch.equal(s.pe_motion[i, :, 0], s.motion[i, :, 1])
    batch = dm.collate("train", torch.tensor([2, 0]))
    assert tuple(batch[0].shape) == (2, T, 2, 144) and tuple(batch[1].shape) == (2, 2, T, 3) and tuple(batch[-3].shape) == (2, T, 1, 144)
    # GIMO + rot6d keeps raising, and says why
    with pytest.raises(NotImplementedError, match="22 x 6"):
        D.EgoSequenceSplit(root, "train", dataset="gimo", data_type="rot6d")
    with pytest.raises(ValueError):
        D.EgoSequenceSplit(root, "train", data_type="quat")
    # the 'angle' statistics alone are not enough
    root2 = str(tmp_path / "nostats")
    _write_egobody(root2, 3, T, rot6d_stats=False)
    with pytest.raises(FileNotFoundError, match="mean_rot6d.npy"):
        D.EgoSequenceSplit(root2, "train", motion_length=T, data_type="rot6d")
    assert D.EgoSequenceSplit(root2, "train", motion_length=T).motion.shape[-1] == 72            # 'angle' unchanged


def test_data_module_rot6d_interactee_estimates(tmp_path):
    """TEST.INTERACTEE_PRED: the estimates replace the interactee's pose as the condition and are re-encoded the same way; the
    POSE_ESTIMATION ground truth stays the file's own interactee."""
    import pickle
    from seeme_amd import data as D
    from seeme_amd import geometry as G
    root = str(tmp_path / "egobody")
    T = 5
    items = _write_egobody(root, 3, T)
    rng = np.random.default_rng(9)
    pred = {}
    for it in items:
        for im in it["recording_utils"]["original_imgname"]:
            pred[im] = {"smpl_parameters": {"global_orient": rng.standard_normal(3), "body_pose": rng.standard_normal(69) * 0.3,
                                            "betas": rng.standard_normal(10)}}
    path = os.path.join(root, "interactee_pred_train.pkl")
    with open(path, "wb") as f:
        pickle.dump(pred, f)
    s = D.EgoSequenceSplit(root, "train", motion_length=T, data_type="rot6d", pose_estimation_task=True, interactee_pred=path)
    mean, std = np.load(os.path.join(root, "mean_rot6d.npy")), np.load(os.path.join(root, "std_rot6d.npy"))
    ren = lambda x: x.double() * torch.from_numpy(std[0, :144]).double() + torch.from_numpy(mean[0, :144]).double()
    it = items[0]
    aa = np.stack([np.concatenate([pred[im]["smpl_parameters"]["global_orient"], pred[im]["smpl_parameters"]["body_pose"]])
                   for im in it["recording_utils"]["original_imgname"]])
    R = G.aa_to_rotmat_torch(torch.from_numpy(aa).double().reshape(-1, 3)).reshape(T, 24, 3, 3)
    assert float((ren(s.motion[0, :, 1]).reshape(T, 24, 3, 2) - R[..., :2]).abs().max()) < 1e-6
    aa_gt = np.concatenate([np.asarray(it["interactee"]["global_orient"]).reshape(T, 3), np.asarray(it["interactee"]["body_pose"]).reshape(T, 69)], 1)
    Rg = G.aa_to_rotmat_torch(torch.from_numpy(aa_gt).double().reshape(-1, 3)).reshape(T, 24, 3, 3)
    assert float((ren(s.pe_motion[0, :, 0]).reshape(T, 24, 3, 2) - Rg[..., :2]).abs().max()) < 1e-6


def test_synthetic_rot6d_batches_decode_to_rotations():
    """SyntheticEgoDataModule(data_type='rot6d'): 144-wide motion whose renormed values are the model-side encoding of rotations
    (orthonormal first two columns), raw translation, the tuple layouts of the 'angle' module; 'angle' batches are unchanged."""
    from seeme_amd.mld import SyntheticEgoDataModule
    from seeme_amd.vae_autograd import rot6d_to_rotmat_torch
    dm = SyntheticEgoDataModule(nfeats=144, T=6, data_type="rot6d")
    b = dm.batch(3, idx=1, pose_estimation=True)
    assert tuple(b[0].shape) == (3, 6, 2, 144) and tuple(b[1].shape) == (3, 2, 6, 3) and tuple(b[-3].shape) == (3, 6, 1, 144)
    for feats in (b[0], b[-3]):
        x = feats.double() * dm.std[0, :144].double() + dm.mean[0, :144].double()
        R = rot6d_to_rotmat_torch(x.reshape(-1, 6))
        eye = torch.eye(3, dtype=torch.float64).expand_as(R)
        assert float((R.transpose(1, 2) @ R - eye).abs().max()) < 1e-5
        a = x.reshape(-1, 2, 3)                                 # the two columns themselves are orthonormal (fp32 storage)
        assert float((a.norm(dim=2) - 1).abs().max()) < 1e-5 and float((a[:, 0] * a[:, 1]).sum(1).abs().max()) < 1e-5
    with pytest.raises(ValueError):
        SyntheticEgoDataModule(nfeats=75, data_type="rot6d")
    a0, a1 = SyntheticEgoDataModule(nfeats=75, T=6).batch(2, idx=3), SyntheticEgoDataModule(nfeats=75, T=6, data_type="angle").batch(2, idx=3)
    assert all(torch.equal(x, y) for x, y in zip(a0, a1))


def test_mld_rot6d_keeps_translation_out_of_the_features():
    """config_vae_egobody_rot6d: 144 features whatever PREDICT_TRANSL says; GIMO + rot6d raises where the joints are formed."""
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(os.path.join(REPO, "configs", "config_vae_egobody_rot6d.yaml"))
    assert cfg.DATA_TYPE == "rot6d" and cfg.model.nfeats == 144 and cfg.TRAIN.ABLATION.PREDICT_TRANSL is True
    dm = SyntheticEgoDataModule(nfeats=144, T=4, data_type="rot6d")
    smpl = SMPL.synthetic(1, V=64)
    m = MLD(cfg, dm, smpl_model=smpl)
    assert m.nfeats == 144 and m.vae.nfeats == 144 and m.transl_in_feats is False
    b = dm.batch(2)
    assert tuple(m._wearer_features(b[0], b[1], 0).shape) == (2, 4, 144)
    # the autograd twin of the joints runs on the CPU: [B,T,24,3], differentiable
    f = (b[0][:, :, 0] * dm.std[0, :144] + dm.mean[0, :144]).clone().requires_grad_(True)
    m.hip_vae_backward = False
    j = m._feats_to_joints_torch(f, None)
    assert tuple(j.shape) == (2, 4, 24, 3)
    j.sum().backward()
    assert torch.isfinite(f.grad).all() and float(f.grad.abs().max()) > 0
    from seeme_amd import cli
    cfg2 = parse_config(os.path.join(REPO, "configs", "config_mld_egobody_rot6d.yaml"))
    assert cfg2.DATA_TYPE == "rot6d" and cfg2.model.denoiser.params.nfeats == 144 and cfg2.TRAIN.STAGE == "diffusion"
    # an [M,144] input that requires grad gets its gradient in its own shape
    from seeme_amd.vae_autograd import smpl_joints_rot6d_torch
    flat = f.detach().reshape(-1, 144).clone().requires_grad_(True)
    smpl_joints_rot6d_torch(smpl, None, flat).sum().backward()
    assert flat.grad.shape == flat.shape
    # GIMO + rot6d: refused where the model is built, by the one rule every layer shares
    from seeme_amd.shapes import motion_layout
    assert motion_layout("egobody", "rot6d", True) == (144, False) and motion_layout("egobody", "angle", True) == (75, True)
    assert motion_layout("gimo", "angle", False) == (66, False) and motion_layout("other", "angle", True, 132) == (132, True)
    with pytest.raises(ValueError):
        motion_layout("egobody", "quat", True)
    cfg3 = parse_config(os.path.join(REPO, "configs", "config_vae_gimo.yaml"))
    cfg3.DATA_TYPE = "rot6d"
    with pytest.raises(NotImplementedError, match="22 x 6"):
        MLD(cfg3, dm, smpl_model=smpl)
    with pytest.raises(NotImplementedError, match="22 x 6"):
        cli.build(cfg3, "cpu", None)
    from seeme_amd import cli
    args = cli.build_parser("train").parse_args(["--cfg", os.path.join(REPO, "configs", "config_vae_egobody_rot6d.yaml"), "--nodebug"])
    assert cli.load_cfg(args, "train").DATA_TYPE == "rot6d"


# ----------------------------------------------------------------------------- the C-ABI surface
def test_header_ctypes_and_library_agree_on_the_rot6d_entry_points():
    from seeme_amd import _lib
    names = ("seeme_smpl_joints_rot6d", "seeme_smpl_joints_rot6d_backward")
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    declared = set(re.findall(r"\b(seeme_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    dynamic = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in names:
        assert name in declared and name in _lib.exported_symbols() and name in dynamic and hasattr(lib, name)
    # the argument counts of the ctypes table are those of the header's prototypes
    for name in names:
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name
    # every seeme_* symbol the library defines is declared, and the reverse (two more than before this path existed)
    assert {s for s in dynamic if s.startswith("seeme_")} >= declared - {"seeme_make_den_layout"}
    err = lambda: lib.seeme_last_error()
    # argument checks come before any device work: they hold without a GPU
    P, D = _lib.GEO_ROT6D_PROHMR, _lib.GEO_ROT6D_DIFFUSION
    model = _lib.SmplModel()
    import ctypes as C
    mp = C.byref(model)
    assert lib.seeme_smpl_joints_rot6d(mp, 0, 16, P, 0, 0, 16, 0) != 0 and b"M must" in err()
    assert lib.seeme_smpl_joints_rot6d(mp, 0, 0, P, 0, 3, 16, 0) != 0 and b"null" in err()
    assert lib.seeme_smpl_joints_rot6d(mp, 0, 16, 7, 0, 3, 16, 0) != 0 and b"order" in err()
    assert lib.seeme_smpl_joints_rot6d_backward(mp, 0, 16, D, 16, 24, 16, 0, 0, 0) != 0 and b"M must" in err()
    assert lib.seeme_smpl_joints_rot6d_backward(mp, 0, 16, D, 16, 23, 16, 0, 3, 0) != 0 and b"dj_stride" in err()
    assert lib.seeme_smpl_joints_rot6d_backward(mp, 0, 16, D, 0, 24, 16, 0, 3, 0) != 0 and b"null" in err()
    assert lib.seeme_smpl_joints_rot6d_backward(mp, 0, 16, 0, 16, 24, 16, 0, 3, 0) != 0 and b"order" in err()
