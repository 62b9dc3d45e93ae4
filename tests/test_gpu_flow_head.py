"""seeme_flow_head on the device: against the float64 twin on recipe weights and against the reference's fixture, at the row-tile
edges of the chain kernel, bit for bit across tiles, launches and workspace contents; then MLD.estimate_interactee and
cli.estimate_main end to end."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, elem_err, load_golden, rel_err
from seeme_amd import prohmr_head as PH
from seeme_amd.weights_recipe import load_flow_head_recipe_, load_recipe_

pytestmark = pytest.mark.gpu
GATE = 1e-4
T = PH.TILE_ROWS
BIG = (2 * T + 5, 3)                       # more than two workgroups with a remainder, S not dividing the tile
SHAPES = [(1, 1), (1, 4), (T - 1, 1), (T, 1), (T + 1, 1), (3, 32), BIG]
NAMES = ("pose6d", "rotmat", "betas", "cam", "log_prob")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_golden("flow_head.npz")


@pytest.fixture(scope="module")
def head(dev):
    return load_flow_head_recipe_(PH.SMPLFlowHead()).to(dev)


def well_conditioned(pose6d, amplification=20.0):
    """[..., 144] -> bool [...]: every joint's Gram-Schmidt is well conditioned.  b1 = a1 / |a1| and b2 = a2' / |a2'| (a2' = a2 minus
    its part along b1) turn an absolute error d of the rot6d values into errors of about d / |a1| and d / |a2'| of the matrix
    entries.  A row of fp32 rot6d values carries about 1e-6 of the row's largest entry m (the reference differs from itself in
    float64 by 7.9e-7 of the largest), so with |a1|, |a2'| >= m / 20 the matrix entries, which are O(1), inherit at most a few 1e-5:
    inside the 1e-4 gate for any correct fp32 chain, while a wrong Gram-Schmidt is off by O(1).  About two draws in three pass."""
    p = pose6d.reshape(*pose6d.shape[:-1], 24, 2, 3)
    a1, a2 = p[..., 0, :], p[..., 1, :]
    n1 = a1.norm(dim=-1)
    b1 = a1 / n1[..., None]
    perp = (a2 - (b1 * a2).sum(-1, keepdim=True) * b1).norm(dim=-1)
    return torch.minimum(n1, perp).amin(dim=-1) * amplification >= pose6d.abs().amax(dim=-1)


@pytest.fixture(scope="module")
def pool():
    """Inputs for every shape (slices of one draw) and their float64 twin, computed once on the CPU: rows are independent, so a
    slice of the twin's result is the twin's result of the slice.  Only the (frame, sample) slots some shape reads are filled:
    32 samples of the first three frames, three of the others.  Each slot takes the first of twelve candidate draws whose float64
    rot6d values are `well_conditioned`, so that the rotation matrices can be held to the same gate as everything else."""
    g = torch.Generator().manual_seed(11)
    n, s, K = BIG[0], 32, 12
    f = 1075.0 + 10 * torch.randn(n, generator=g)
    cx, cy = 960.0 + 8 * torch.randn(n, generator=g), 540.0 + 8 * torch.randn(n, generator=g)
    center = torch.stack([200 + 1500 * torch.rand(n, generator=g), 150 + 800 * torch.rand(n, generator=g)], dim=1)
    scale = 0.6 + 2 * torch.rand(n, generator=g)
    image = 0.5 * torch.randn(n, PH.IMAGE_DIM, generator=g).abs()
    scene = 0.5 * torch.randn(n, PH.SCENE_DIM, generator=g)
    ctx = PH.context_rows(image, scene, center, scale, f, cx, cy)
    slots = [(l, j) for l in range(n) for j in range(s if l < 3 else BIG[1])]
    frame = torch.tensor([l for l, _ in slots])
    cand = torch.randn(len(slots), K, PH.DIM, generator=g)
    cpu_head = load_flow_head_recipe_(PH.SMPLFlowHead())
    pose, rot, betas_r, cam_r, lp = PH.flow_head_torch(cpu_head, ctx[frame].double(), cand.double())
    ok = well_conditioned(pose)
    assert bool(ok.any(dim=1).all()), "a slot without a well-conditioned candidate: raise K"
    pick = ok.double().argmax(dim=1)                                    # the first that is
    rows = torch.arange(len(slots))
    z = torch.zeros(n, s, PH.DIM)
    want_pose, want_rot = torch.zeros(n, s, PH.DIM, dtype=torch.float64), torch.zeros(n, s, 24, 3, 3, dtype=torch.float64)
    want_lp = torch.zeros(n, s, dtype=torch.float64)
    col = torch.tensor([j for _, j in slots])
    z[frame, col] = cand[rows, pick]
    want_pose[frame, col], want_rot[frame, col], want_lp[frame, col] = pose[rows, pick], rot[rows, pick], lp[rows, pick]
    first = torch.tensor([slots.index((l, 0)) for l in range(n)])
    return ctx, z, (want_pose, want_rot, betas_r[first], cam_r[first], want_lp)


def _slice(want, L_, S):
    pose, rot, betas, cam, lp = want
    return pose[:L_, :S], rot[:L_, :S], betas[:L_], cam[:L_], lp[:L_, :S]


def _check(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(w.shape), name
        g, w = g.cpu().numpy(), w.cpu().numpy()
        r, e = rel_err(g, w), elem_err(g, w)
        print(f"{name}: rel_err {r:.3e} elem_err {e:.3e}")
        assert np.isfinite(g).all() and r <= GATE and (e <= GATE or name == "log_prob"), (name, r, e)


# ----------------------------------------------------------------------------- 1. kernel against the float64 twin and the reference
@pytest.mark.parametrize("shape", SHAPES, ids=[f"L{a}_S{b}" for a, b in SHAPES])
def test_kernel_equals_the_float64_twin(dev, head, pool, shape):
    ctx, z, want = pool
    L_, S = shape
    got = PH.flow_head_hip(head, ctx[:L_].to(dev), z[:L_, :S].contiguous().to(dev))
    torch.cuda.synchronize()
    _check(got, _slice(want, L_, S))


def test_rotmat_on_unfiltered_draws_within_the_gate_times_each_joints_amplification(dev, head, pool):
    """`pool` holds the rotation matrices to the gate on draws chosen to be well conditioned.  Here nothing is chosen: 32 plain
    normal draws for each of three frames.  A joint whose Gram-Schmidt amplifies by a = (row's largest |rot6d|) / min(|a1|, |a2'|)
    turns the fp32 chain's error budget of gate / 20 of the row's largest value (see `well_conditioned`) into a / 20 of the gate, so
    every joint's matrix is held to gate * max(1, a / 20) by its own a from the float64 twin; the rot6d values themselves to the gate."""
    ctx = pool[0][:3]
    z = torch.randn(3, 32, PH.DIM, generator=torch.Generator().manual_seed(23))
    pose, rot, _b, _c, _lp = PH.flow_head_torch(load_flow_head_recipe_(PH.SMPLFlowHead()), ctx.double(), z.double())
    got = PH.flow_head_hip(head, ctx.to(dev), z.to(dev))
    p = pose.reshape(3, 32, 24, 2, 3)
    a1, a2 = p[..., 0, :], p[..., 1, :]
    n1 = a1.norm(dim=-1)
    perp = (a2 - ((a1 / n1[..., None]) * a2).sum(-1, keepdim=True) * (a1 / n1[..., None])).norm(dim=-1)
    amp = pose.abs().amax(dim=-1, keepdim=True) / torch.minimum(n1, perp)                     # [3,32,24]
    err = (got[1].cpu().double() - rot).abs().amax(dim=(-1, -2))                                # [3,32,24]; the entries are O(1)
    bound = GATE * torch.clamp(amp / 20.0, min=1.0)
    print(f"amplification: median {float(amp.median()):.1f} max {float(amp.max()):.1f}; joints above 20: {int((amp > 20).sum())} of {amp.numel()}; "
          f"largest error / bound {float((err / bound).max()):.3f}; largest error {float(err.max()):.3e}")
    assert bool((amp > 20).any()), "no ill-conditioned joint among the draws: the test would say nothing beyond pool's"
    assert bool((err <= bound).all())
    assert rel_err(got[0].cpu().numpy(), pose.numpy()) <= GATE


def test_kernel_equals_the_reference_fixture(dev, head, fx):
    got = PH.flow_head_hip(head, torch.from_numpy(fx["ctx"]).to(dev), torch.from_numpy(fx["z"]).to(dev))
    _check(got, [torch.from_numpy(fx[k]) for k in NAMES])


# ----------------------------------------------------------------------------- 2. bit for bit
def test_rows_do_not_depend_on_their_tile_the_launch_or_the_workspace(dev, head, pool):
    ctx, z, _ = pool
    L_, S = BIG
    c, zz = ctx[:L_].to(dev), z[:L_, :S].contiguous().to(dev)
    first = PH.flow_head_hip(head, c, zz)
    again = PH.flow_head_hip(head, c, zz)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    head._ws.fill_(0xFF)                                                # NaN bytes in the workspace
    poisoned = PH.flow_head_hip(head, c, zz)
    assert all(torch.equal(a, b) for a, b in zip(first, poisoned))
    # every frame's sample 0 from a call of another shape: row l there, row 3 l here, so all but row 0 sit at another tile row
    col0 = PH.flow_head_hip(head, c, zz[:, :1].contiguous())
    assert torch.equal(col0[0][:, 0], first[0][:, 0]) and torch.equal(col0[1][:, 0], first[1][:, 0]) and torch.equal(col0[4][:, 0], first[4][:, 0])
    assert torch.equal(col0[2], first[2]) and torch.equal(col0[3], first[3])
    # row 16 = (5, 1) opens the second tile; row 34 = (11, 1) is mid-way in the partial last tile; the last row ends it
    for l, s in ((0, 0), (5, 1), (T, 2), (11, 1), (L_ - 1, S - 1)):
        alone = PH.flow_head_hip(head, c[l:l + 1].contiguous(), zz[l:l + 1, s:s + 1].contiguous())
        assert torch.equal(alone[0][0, 0], first[0][l, s]) and torch.equal(alone[1][0, 0], first[1][l, s]), (l, s)
        assert torch.equal(alone[2][0], first[2][l]) and torch.equal(alone[3][0], first[3][l]) and torch.equal(alone[4][0, 0], first[4][l, s])


def test_sizes_the_entry_does_not_take(dev, head):
    from seeme_amd import _lib as L
    lib = L.lib()
    assert lib.seeme_flow_head_workspace_bytes(1, 33) == 0 and lib.seeme_flow_head_workspace_bytes(0, 1) == 0
    assert lib.seeme_flow_head_workspace_bytes(1 << 16, 32) == 0 and lib.seeme_flow_head_workspace_bytes(4, 2) == 4 * 5120 * 4
    with pytest.raises(ValueError):
        PH.flow_head_hip(head, torch.zeros(2, 2566, device=dev), torch.zeros(2, 33, 144, device=dev))
    with pytest.raises(L.SeemeError, match="float32"):
        PH.flow_head_hip(head, torch.zeros(2, 2566, device=dev, dtype=torch.float64), torch.zeros(2, 1, 144, device=dev))


# ----------------------------------------------------------------------------- 3. through MLD
CFG = "config_mld_interactee_head.yaml"


def _mld(dev, **kw):
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(os.path.join(REPO, "configs", CFG))
    assert cfg.model.interactee_head is True
    cfg.model.scheduler.num_inference_timesteps = 5
    for k, v in kw.items():
        node = cfg
        *path, last = k.split(".")
        for p in path:
            node = node[p]
        node[last] = v
    dm = SyntheticEgoDataModule(nfeats=cfg.model.nfeats, T=4, n_points=256, device=dev, pose_dim=cfg.model.nfeats - 3)
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser), load_recipe_(model.proscene)      # flow.* entries: the flow-head recipe
    return model.to(dev).eval(), dm, cfg


@pytest.fixture(scope="module")
def model(dev):
    return _mld(dev)


def _frames(n, H=48, W=64, N=3000, seed=0):
    """A synthetic headset recording without the interactee: smooth frames, a box inside them, EgoBody-style world2cam (the camera
    looks along -z of its own frame, so D = diag(1,-1,-1) makes it OpenCV) inside a cloud of scene vertices: the head's view keeps
    what lies in front of D world2cam, predict's own window views (INTEGRATION K) keep z > 0 of world2cam as it is, and both find rows."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    video = np.stack([np.stack([(xx * 3 + 5 * t) % 256, (yy * 4 + 7 * t) % 256, (xx + yy + 11 * t) % 256], axis=-1) for t in range(n)])
    w2c = np.tile(np.eye(4), (n, 1, 1))
    w2c[:, :3, 3] = np.stack([0.02 * np.arange(n), np.zeros(n), -0.01 * np.arange(n)], axis=1)
    verts = g.normal(size=(N, 3)) * np.array([1.5, 1.0, 2.5])
    return {"video": video.astype(np.uint8), "center": np.stack([30 + g.uniform(-3, 3, n), 24 + g.uniform(-3, 3, n)], axis=1).astype(np.float32),
            "scale": g.uniform(0.1, 0.15, n).astype(np.float32), "cam_intrinsics": np.array([60.0, 32.0, 24.0], np.float32),
            "world2cam": w2c, "scene_vertices": verts.astype(np.float32), "wearer_betas": (0.3 * g.normal(size=10)).astype(np.float32)}


def test_estimate_interactee_is_the_head_on_the_encoders_features(dev, model, tmp_path):
    from seeme_amd import cli, crops as CR, recording as R
    m, _dm, _cfg = model
    fr = _frames(5)
    patches = CR.crop_patches_hip(torch.from_numpy(fr["video"]).to(dev), np.arange(5), PH.head_box(fr["center"], fr["scale"]))
    view = torch.from_numpy(R.opencv_views(fr["world2cam"], m.interactee_camera_axes)).float().to(dev)
    sv = R.scene_views_hip(torch.from_numpy(fr["scene_vertices"]).to(dev), view, 256)
    assert int(sv["count"].min()) > 0
    z = PH.draw_z(5, 3, torch.Generator().manual_seed(2), dev)
    out = m.estimate_interactee(patches, sv["cloud"], fr["center"], fr["scale"], fr["cam_intrinsics"], z=z)
    img, sc = m.proscene.encode_image(patches), m.proscene.encode_scene(sv["cloud"])
    f, cx, cy = (float(v) for v in fr["cam_intrinsics"])
    ctx = PH.context_rows(img, sc, torch.from_numpy(fr["center"]).to(dev), torch.from_numpy(fr["scale"]).to(dev), f, cx, cy)
    want = PH.flow_head_hip(m.proscene.flow, ctx, z)
    assert torch.equal(out["ctx"], ctx) and all(torch.equal(out[k], w) for k, w in zip(NAMES, want))
    assert torch.isfinite(out["pose6d"]).all() and torch.isfinite(out["transl"]).all() and bool((out["cam"][:, 0] > 0).all())
    feats = m.estimate_interactee(img, sc, fr["center"], fr["scale"], np.tile(fr["cam_intrinsics"], (5, 1)), z=z)      # features, [L,3] intrinsics
    assert all(torch.equal(feats[k], out[k]) for k in out)
    mode = m.estimate_interactee(img, sc, fr["center"], fr["scale"], fr["cam_intrinsics"], num_samples=2, generator=torch.Generator().manual_seed(1))
    assert torch.equal(mode["pose6d"][:, 0], out["pose6d"][:, 0]) and mode["pose6d"].shape == (5, 2, 144)
    # a strict reload of a saved checkpoint reproduces it
    ckpt = os.path.join(tmp_path, "model.ckpt")
    cli.save_checkpoint(ckpt, m, 0, 0)
    other, _, _ = _mld(dev)
    with torch.no_grad():
        for p in other.proscene.flow.parameters():
            p.add_(0.01)
    other.load_state_dict(cli.read_checkpoint(ckpt)["state_dict"], strict=True)
    again = other.to(dev).eval().estimate_interactee(patches, sv["cloud"], fr["center"], fr["scale"], fr["cam_intrinsics"], z=z)
    assert all(torch.equal(again[k], out[k]) for k in out)


# ----------------------------------------------------------------------------- 4. estimate.py end to end, then predict.py on its output
def test_cli_estimate_main_then_predict_main(dev, model, tmp_path):
    from seeme_amd import cli, recording as R
    m, _dm, _cfg = model
    ckpt = os.path.join(tmp_path, "model.ckpt")
    cli.save_checkpoint(ckpt, m, 0, 0)
    n, S = 5, 3
    fr = _frames(n, seed=4)
    rec_path, out_path, out2 = (os.path.join(tmp_path, f) for f in ("rec.npz", "with_interactee.npz", "again.npz"))
    np.savez(rec_path, **fr)
    base = ["--cfg", os.path.join(REPO, "configs", CFG), "--checkpoint", ckpt, "--folder", str(tmp_path), "--scene_points", "256"]
    argv = base + ["--input", rec_path, "--num_samples", str(S), "--seed", "3", "--save_samples", "--chunk_frames", "2"]
    r = cli.estimate_main(argv + ["--output", out_path])
    assert r["file"] == out_path and r["n_frames"] == n and r["num_samples"] == S
    with np.load(out_path, allow_pickle=False) as z:
        got = {k: z[k] for k in z.files}
    assert all(np.array_equal(got[k], fr[k]) for k in fr)               # the input's keys are copied through
    shapes = {"global_orient": (n, 3), "body_pose": (n, 69), "transl": (n, 3), "betas": (10,), "interactee_betas_frames": (n, 10),
              "interactee_cam": (n, 3), "interactee_log_prob": (n, S), "scene_view_count": (n,),
              "interactee_samples_global_orient": (n, S, 3), "interactee_samples_body_pose": (n, S, 69), "interactee_samples_transl": (n, S, 3)}
    for k, shp in shapes.items():
        assert got[k].shape == shp and np.isfinite(got[k]).all(), k
    assert np.array_equal(got["interactee_samples_transl"][:, 0], got["transl"]) and (got["scene_view_count"] > 0).all()
    assert np.allclose(got["betas"], got["interactee_betas_frames"].mean(axis=0), atol=1e-6)
    # the mode is the most probable of a frame's samples, and the samples differ from it
    assert (got["interactee_log_prob"][:, :1] >= got["interactee_log_prob"]).all()
    assert not np.array_equal(got["interactee_samples_body_pose"][:, 1], got["body_pose"])
    rec = R.load_recording(out_path)
    assert rec["n_frames"] == n and rec["cam_intrinsics"].shape == (n, 3)
    # the same seed gives the same bytes, whatever the chunking
    cli.estimate_main([a if a != "2" else "64" for a in argv] + ["--output", out2])
    with open(out_path, "rb") as a, open(out2, "rb") as b:
        assert a.read() == b.read()
    # predict.py runs on it unchanged
    motion = os.path.join(tmp_path, "motion.npz")
    p = cli.predict_main(base + ["--input", out_path, "--output", motion, "--frames", "4", "--num_hypotheses", "2", "--seed", "5"])
    assert p["n_frames"] == n
    with np.load(motion, allow_pickle=False) as z:
        assert z["global_orient"].shape == (n, 3) and all(np.isfinite(z[k]).all() for k in z.files)
