#!/usr/bin/env python3
"""Generate flow_head.npz from the REFERENCE's own SMPLFlow (EgoHMR/models/prohmr/smpl_flow.py over its nflows copy).

Runs only where the reference tree exists (SEEME_REFERENCE, default /root/reference); nothing of it is copied.  Three modules the
reference imports but never calls on this path are replaced by empty stubs: ``yacs`` / ``yacs.config`` (CfgNode = dict) and ``UMNN``
(NeuralIntegral = ParallelNeuralIntegral = object).  FCHead reads cfg.SMPL.MEAN_PARAMS with np.load: a temporary npz with
cam = [0.9, 0, 0] and shape = ten small values stands in for smpl_mean_params.npz (both buffers are then overwritten by the recipe,
being entries of the state dict).  Weights: seeme_amd.weights_recipe.load_flow_head_recipe_.  No weights are stored.

With noise given, Flow.sample_and_log_prob takes one sample per frame only (distributions/base.py:37), so the S = 4 fixture is made
by calling the reference once per sample column.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_flow_head.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SEEME_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "nflows"))

for name, attrs in (("yacs", {}), ("yacs.config", {"CfgNode": dict}),
                    ("UMNN", {"NeuralIntegral": object, "ParallelNeuralIntegral": object})):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
sys.modules["yacs"].config = sys.modules["yacs.config"]

from seeme_amd import prohmr_head as PH  # noqa: E402
from seeme_amd.weights_recipe import load_flow_head_recipe_  # noqa: E402

torch.set_grad_enabled(False)
NS = types.SimpleNamespace
L, S = 3, 4


def reference_head():
    from EgoHMR.models.prohmr.smpl_flow import SMPLFlow
    with tempfile.TemporaryDirectory() as tmp:
        mean = os.path.join(tmp, "mean.npz")
        np.savez(mean, cam=np.array([0.9, 0, 0], np.float32), shape=0.01 * np.arange(10, dtype=np.float32), pose=np.zeros(144, np.float32))
        cfg = NS(MODEL=NS(FLOW=NS(DIM=144, LAYER_HIDDEN_FEATURES=1024, NUM_LAYERS=4, LAYER_DEPTH=2, CONTEXT_FEATURES=2048),
                          FC_HEAD=NS(NUM_FEATURES=1024)), SMPL=NS(MEAN_PARAMS=mean))
        net = SMPLFlow(cfg, contect_feats_dim=PH.CTX_DIM)
    return load_flow_head_recipe_(net).eval()


def run(net, ctx, z):
    """The reference once per sample column -> pose6d [L,S,144], log_prob [L,S], betas [L,10], cam [L,3], rotmat [L,S,24,3,3]."""
    from EgoHMR.utils.geometry import rot6d_to_rotmat
    pose, lp = [], []
    for s in range(z.shape[1]):
        params, cam, log_prob, _z, pose6d = net(ctx, z=z[:, s:s + 1])
        pose.append(pose6d)
        lp.append(log_prob)
    pose, lp = torch.cat(pose, dim=1), torch.cat(lp, dim=1)
    rot = rot6d_to_rotmat(pose.reshape(-1, 144)).reshape(z.shape[0], z.shape[1], 24, 3, 3)
    return pose, lp, params["betas"][:, 0], cam[:, 0], rot


def inputs():
    rng = np.random.Generator(np.random.PCG64(20))
    f = np.array([1075.0, 1080.5, 1069.25], np.float32)                  # HoloLens-like: 1920 x 1080, f ~ 1075 px
    cx = np.array([960.0, 955.5, 948.0], np.float32)
    cy = np.array([540.0, 536.25, 545.5], np.float32)
    center = np.array([[900.0, 520.0], [1210.5, 640.25], [433.0, 388.5]], np.float32)
    scale = np.array([1.4, 2.25, 0.8], np.float32)
    image = np.abs(rng.standard_normal((L, PH.IMAGE_DIM))).astype(np.float32) * 0.5          # pooled ReLU features: non-negative
    scene = (0.5 * rng.standard_normal((L, PH.SCENE_DIM))).astype(np.float32)
    z = rng.standard_normal((L, S, PH.DIM)).astype(np.float32)
    z[:, 0] = 0
    return {k: torch.from_numpy(v) for k, v in dict(f=f, cx=cx, cy=cy, center=center, scale=scale, image=image, scene=scene, z=z).items()}


def main():
    from EgoHMR.utils.geometry import convert_pare_to_full_img_cam
    net = reference_head()
    d = inputs()
    ctx = PH.context_rows(d["image"], d["scene"], d["center"], d["scale"], d["f"], d["cx"], d["cy"])
    z = d["z"]
    pose, lp, betas, cam, rot = run(net, ctx, z)
    nrm = float(pose.abs().max())

    # the conditions the fixture has to meet (they are what makes a skipped or mis-ordered stage visible)
    couplings = [net.flow._transform._transforms[3 * k + 2] for k in range(4)]
    for k, cp in enumerate(couplings):
        fl = cp.transform_net.final_layer
        w, b = fl.weight.clone(), fl.bias.clone()
        fl.weight.zero_(), fl.bias.zero_()
        diff = float((run(net, ctx, z)[0] - pose).abs().max()) / nrm
        fl.weight.copy_(w), fl.bias.copy_(b)
        print(f"dropping the coupling shift of layer {k}: {diff:.3f} of the max norm")
        assert diff > 0.1, (k, diff)
    for cp in couplings:
        i, t = cp.identity_features.clone(), cp.transform_features.clone()
        cp.identity_features.copy_(t), cp.transform_features.copy_(i)
    diff = float((run(net, ctx, z)[0] - pose).abs().max()) / nrm
    for cp in couplings:
        i, t = cp.identity_features.clone(), cp.transform_features.clone()
        cp.identity_features.copy_(t), cp.transform_features.copy_(i)
    print(f"swapping the odd and even feature sets: {diff:.3f} of the max norm")
    assert diff > 0.1, diff
    assert torch.equal(run(net, ctx, z)[0], pose), "the reference was not restored"
    print("cam[:, 0]:", cam[:, 0].tolist())
    assert bool(((cam[:, 0] >= 0.3) & (cam[:, 0] <= 2)).all())
    p = pose.reshape(-1, 2, 3).double()
    a1, a2 = p[:, 0] / p[:, 0].norm(dim=1, keepdim=True), p[:, 1] / p[:, 1].norm(dim=1, keepdim=True)
    sine = torch.cross(a1, a2, dim=1).norm(dim=1)
    print("rot6d pairs, smallest sine of the angle between them:", float(sine.min()))
    assert float(sine.min()) > 0.1
    # float64: SMPLFlow.forward casts its features to fp32 (smpl_flow.py:87), so its two parts are called directly
    net.double()
    c64, z64 = ctx.double(), z.double()
    cols = [net.flow.sample_and_log_prob(1, context=c64, noise=z64[:, s:s + 1]) for s in range(S)]
    pose64, lp64 = torch.cat([c[0] for c in cols], dim=1), torch.cat([c[1] for c in cols], dim=1)
    off = net.fc_head.layers(c64)
    betas64, cam64 = off[:, :10] + net.fc_head.init_betas[0], off[:, 10:] + net.fc_head.init_cam[0]
    net.float()
    e64 = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in ((pose, pose64), (lp, lp64), (betas, betas64), (cam, cam64)))
    print(f"reference fp32 vs float64: {e64:.2e}")
    assert e64 < 1e-5, e64

    cam_t_full = convert_pare_to_full_img_cam(cam, 200.0 * d["scale"], d["center"], 2 * d["cx"], 2 * d["cy"], d["f"], crop_res=224)
    sd = net.state_dict()
    out = {"keys": np.array(sorted(sd)), "shapes": np.array([",".join(str(v) for v in sd[k].shape) for k in sorted(sd)]),
           "ctx": ctx.numpy(), "z": z.numpy(), "pose6d": pose.numpy(), "log_prob": lp.numpy(), "betas": betas.numpy(), "cam": cam.numpy(),
           "rotmat": rot.numpy(), "cam_t_full": cam_t_full.numpy(),
           **{k: d[k].numpy() for k in ("f", "cx", "cy", "center", "scale")}}
    path = os.path.join(HERE, "flow_head.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
