"""The point-in-mesh test on the device: the two kernels of csrc/collision.hip against the float64 torch twin ON THE SAME fp32 VALUES,
their bitwise behaviour, their argument checks, and ego_eval / cli.test_main with TEST.COLLISION_METRICS.

Every case is F = 3 bodies at metre offsets (frame 1 skipped) and S = 2 clouds; frame 0 reads cloud 1 and frame 2 reads cloud 0.
"Points in the box" are drawn uniformly in the bounding box of the frame that reads them and rounded to fp32."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu
AXES = (0.25, 0.6, 0.15)                       # semi-axes of the test body, metres
OFFSETS = ((1.5, 0.9, -2.0), (0.0, 1.0, 0.0), (-2.2, 1.1, 1.4))
SOF = [1, -1, 0]
TETRA_V = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
TETRA_F = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _bodies(shape):
    """verts [3,V,3] fp32 (one body at the three offsets) and faces [NF,3]."""
    from seeme_amd.mesh_metrics import uv_sphere
    if shape == "tetra":
        v, f = torch.tensor(TETRA_V, dtype=torch.float64) * 0.7, torch.tensor(TETRA_F)
    else:
        v, f = uv_sphere(*{"small": (5, 7), "full": (84, 82)}[shape])
        v = v * torch.tensor(AXES, dtype=torch.float64)
    return torch.stack([v + torch.tensor(o, dtype=torch.float64) for o in OFFSETS]).float(), f


def _box_points(verts, n, seed):
    lo, hi = verts.double().min(dim=0).values, verts.double().max(dim=0).values
    u = torch.from_numpy(np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)))
    return (lo + u * (hi - lo)).float()


@functools.lru_cache(maxsize=None)
def _case(shape, P):
    """(verts, faces, clouds [2,P,3], w64 [3,P]) on the device; the float64 twin's w is computed once and shared."""
    from seeme_amd.mesh_metrics import winding_number_torch
    dev = torch.device("cuda:0")
    verts, faces = _bodies(shape)
    if shape == "tetra":               # the issue's two points: (0.2, 0.2, 0.2) is inside, (1, 1, 1) outside; frame 2 gets the inner one
        inner = (torch.tensor([0.2, 0.2, 0.2], dtype=torch.float64) * 0.7 + torch.tensor(OFFSETS[2], dtype=torch.float64)).float()
        outer = (torch.tensor([1.0, 1.0, 1.0], dtype=torch.float64) * 0.7 + torch.tensor(OFFSETS[0], dtype=torch.float64)).float()
        clouds = torch.stack([inner[None], outer[None]])
    else:
        clouds = torch.stack([_box_points(verts[2], P, 5), _box_points(verts[0], P, 6)])
    verts, faces, clouds = verts.to(dev), faces.to(dev), clouds.to(dev).contiguous()
    w64 = winding_number_torch(verts.double(), faces, clouds.double(), SOF)
    return verts, faces, clouds, w64


SHAPES = [("tetra", 1), ("small", 250), ("full", 2048)]


# ----------------------------------------------------------------------------- 1. accuracy of the winding kernel
@pytest.mark.parametrize("shape,P", SHAPES)
def test_winding_kernel_against_the_float64_twin(dev, shape, P):
    """Measured on the MI355X (kernel error / e32, the error of the twin run in float32 on the same inputs): see DESIGN 5.6a."""
    from seeme_amd.mesh_metrics import winding_number_hip, winding_number_torch
    verts, faces, clouds, w64 = _case(shape, P)
    live = [0, 2]
    # the condition on the inputs first: no point so near the surface that float64 itself is unsure
    assert float((w64 - w64.round()).abs().max()) <= 1e-6
    w32 = winding_number_torch(verts, faces, clouds, SOF)
    e32 = float((w32.double() - w64)[live].abs().max())
    got = winding_number_hip(verts, faces, clouds, SOF)
    assert got.shape == (3, P) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    err = float((got.double() - w64)[live].abs().max())
    n_in = int((w64[live].abs() >= 0.5).sum())
    print(f"winding {shape} P={P}: kernel vs float64 twin {err:.3e}, fp32 twin vs float64 twin (e32) {e32:.3e}, inside {n_in} of {2 * P}")
    assert torch.equal(got.abs() >= 0.5, w64.abs() >= 0.5)
    assert bool((got[1] == 0).all())
    if shape != "tetra":
        assert 0 < n_in < 2 * P
    assert err <= 16 * e32
    assert torch.equal(winding_number_hip(verts, faces, clouds, SOF), got)
    for f in live:                                                                 # F = 1 gives the row of F = 3
        assert torch.equal(winding_number_hip(verts[f:f + 1].clone(), faces, clouds, SOF[f:f + 1])[0], got[f]), f


# ----------------------------------------------------------------------------- 2. counts
@functools.lru_cache(maxsize=None)
def _room_case():
    """V = 6890, P = 20 000: 18 000 room-wide points, none of them in a live frame's box, and 2000 points in the box, shuffled."""
    dev = torch.device("cuda:0")
    verts, faces = _bodies("full")
    g = torch.Generator().manual_seed(20000)
    clouds = []
    for s, f in ((0, 2), (1, 0)):
        room = torch.rand(18000, 3, generator=g) * torch.tensor([8.0, 3.0, 8.0]) - torch.tensor([4.0, 0.0, 4.0])
        for b in (0, 2):
            lo, hi = verts[b].min(dim=0).values, verts[b].max(dim=0).values
            room[((room >= lo) & (room <= hi)).all(dim=1), 1] += 10.0
        pts = torch.cat([room, _box_points(verts[f], 2000, 7 + s)])
        clouds.append(pts[torch.randperm(20000, generator=g)])
    return verts.to(dev), faces.to(dev), torch.stack(clouds).to(dev).contiguous()


def _count_inputs(shape, P):
    return _room_case() if shape == "room" else _case(shape, P)[:3]


@functools.lru_cache(maxsize=None)
def _count_want(shape, P):
    from seeme_amd.mesh_metrics import scene_inside_count_torch
    verts, faces, clouds = _count_inputs(shape, P)
    return scene_inside_count_torch(verts.double(), faces, clouds.double(), SOF)


@pytest.mark.parametrize("shape,P", SHAPES + [("room", 20000)])
def test_inside_count_equals_the_float64_twin_and_is_bitwise_stable(dev, shape, P):
    from seeme_amd.mesh_metrics import scene_inside_count_hip, scene_inside_count_torch
    verts, faces, clouds = _count_inputs(shape, P)
    want = _count_want(shape, P)
    got = scene_inside_count_hip(verts, faces, clouds, SOF)
    print(f"count {shape} P={P}: {got.tolist()} (twin {want.tolist()})")
    assert got.dtype == torch.int32 and torch.equal(got, want) and int(got[1]) == 0
    if shape != "tetra":
        assert 0 < int(got[0]) < P and 0 < int(got[2]) < P
    else:
        assert got.tolist() == [0, 0, 1]
    assert torch.equal(scene_inside_count_hip(verts, faces, clouds, SOF), got)     # twice the same
    for f in (0, 2):                                                               # F = 1 launches give the rows of F = 3
        assert torch.equal(scene_inside_count_hip(verts[f:f + 1].clone(), faces, clouds, SOF[f:f + 1])[0], got[f]), f
    many = scene_inside_count_hip(verts[[0, 2] * 256].contiguous(), faces, clouds, [SOF[0], SOF[2]] * 256)       # one slice per frame
    assert torch.equal(many, got[[0, 2] * 256])
    two = scene_inside_count_hip(verts[:2].contiguous(), faces, clouds)            # without a map frame f uses scene f
    assert torch.equal(two, scene_inside_count_torch(verts[:2].double(), faces, clouds.double()))
    assert torch.equal(scene_inside_count_hip(verts, faces.flip(1).contiguous(), clouds, SOF), got)             # a flipped table
    junk = torch.cat([faces, torch.zeros(10, 3, dtype=faces.dtype, device=dev)])                                 # 10 all-zero faces
    assert torch.equal(scene_inside_count_hip(verts, junk, clouds, SOF), got)


def test_inside_count_edge_shapes(dev):
    from seeme_amd.mesh_metrics import scene_inside_count_hip, scene_inside_count_torch
    verts, faces, clouds, _ = _case("small", 250)
    # P = 65: one point more than a wave
    c65 = clouds[:, :65].contiguous()
    got = scene_inside_count_hip(verts, faces, c65, SOF)
    assert torch.equal(got, scene_inside_count_torch(verts.double(), faces, c65.double(), SOF)) and int(got[0]) > 0
    # P = 1
    c1 = clouds[:, 3:4].contiguous()
    assert torch.equal(scene_inside_count_hip(verts, faces, c1, SOF), scene_inside_count_torch(verts.double(), faces, c1.double(), SOF))
    # no point inside the box: 0 (the other frame's cloud is metres away), and a cloud 100 m up
    assert scene_inside_count_hip(verts, faces, clouds, [0, -1, 1]).tolist() == [0, 0, 0]
    assert scene_inside_count_hip(verts, faces, clouds + torch.tensor([0.0, 100.0, 0.0], device=dev), SOF).tolist() == [0, 0, 0]
    # all points inside the box AND inside the body: every one is counted, through full rounds of the queue
    inner = (torch.tensor(OFFSETS[0], device=dev) + 0.3 * torch.tensor(AXES, device=dev) * (2 * torch.rand(1, 1500, 3, device=dev) - 1)).contiguous()
    assert scene_inside_count_hip(verts[0:1], faces, inner).tolist() == [1500]
    # two overlapping copies in one mesh: a point of the overlap (w = 2) counts once
    from seeme_amd.mesh_metrics import winding_number_torch
    v2 = torch.cat([verts, verts + torch.tensor([0.2, 0.0, 0.0], device=dev)], dim=1).contiguous()
    f2 = torch.cat([faces, faces + verts.shape[1]])
    pts = torch.stack([_box_points(v2[2].cpu(), 400, 2), _box_points(v2[0].cpu(), 400, 3)]).to(dev)
    w = winding_number_torch(v2.double(), f2, pts.double(), SOF)
    assert float((w - w.round()).abs().max()) <= 1e-6 and set(w[[0, 2]].round().long().flatten().tolist()) == {0, 1, 2}
    got = scene_inside_count_hip(v2, f2, pts, SOF)
    assert torch.equal(got.long(), (w.round() >= 1).sum(dim=1)) and torch.equal(got, scene_inside_count_torch(v2.double(), f2, pts.double(), SOF))


# ----------------------------------------------------------------------------- 3. bad arguments
def test_collision_kernels_bad_arguments_raise(dev):
    from seeme_amd import _lib as L
    from seeme_amd import mesh_metrics as M
    z = lambda *s: torch.zeros(*s, device=dev)
    faces = torch.tensor(TETRA_F, device=dev)
    for fn in (M.scene_inside_count_hip, M.winding_number_hip):
        with pytest.raises(L.SeemeError, match="V must"):
            fn(z(1, 10113, 3), faces, z(1, 4, 3))
        with pytest.raises(L.SeemeError, match="face index"):
            fn(z(1, 4, 3), torch.tensor([[0, 1, 4]], device=dev), z(1, 4, 3))
        with pytest.raises(L.SeemeError, match="face index"):
            fn(z(1, 4, 3), torch.tensor([[0, -1, 2]], device=dev), z(1, 4, 3))
        with pytest.raises(L.SeemeError, match="map entry"):
            fn(z(2, 4, 3), faces, z(1, 4, 3), [0, 1])
        with pytest.raises(L.SeemeError):
            fn(z(1, 4, 3).cpu(), faces, z(1, 4, 3))
        with pytest.raises(L.SeemeError):
            fn(z(1, 4, 3), faces, z(1, 4, 3).cpu())
        with pytest.raises(L.SeemeError, match="expected"):
            fn(z(1, 4, 3), faces, z(4, 3))
        with pytest.raises(L.SeemeError, match="faces must"):
            fn(z(1, 4, 3), faces.float(), z(1, 4, 3))
    with pytest.raises(L.SeemeError, match="workspace too small"):
        M.scene_inside_count_hip(z(2, 4, 3), faces, z(1, 4, 3), [0, 0], ws_bytes=4)


# ----------------------------------------------------------------------------- 4. ego_eval with TEST.COLLISION_METRICS
def _sphere_smpl():
    from seeme_amd.mesh_metrics import uv_sphere
    from seeme_amd.smpl import SMPL, synthetic_model_arrays
    v, f = uv_sphere(84, 82)
    arrays = synthetic_model_arrays(1234)
    arrays["v_template"] = (v * torch.tensor(AXES, dtype=torch.float64)).float().numpy()
    arrays["faces"] = f.numpy()
    return SMPL(model_arrays=arrays)


def _mld(dev, mutate=None, T=8, n_points=384):
    """The parity configuration of tests/test_gpu_mesh_metrics.py::_mld on config_mld_scene, with the ellipsoid as the body."""
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_scene.yaml"))
    cfg.model.scheduler.num_inference_timesteps = 5
    if mutate:
        mutate(cfg)
    dm = SyntheticEgoDataModule(nfeats=cfg.model.nfeats, T=T, n_points=n_points, device=dev,
                                pose_dim=cfg.model.nfeats - (3 if cfg.TRAIN.ABLATION.PREDICT_TRANSL else 0))
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=_sphere_smpl())
    load_recipe_(model.vae), load_recipe_(model.denoiser)
    load_recipe_(model.proscene.scene_enc)
    return model.to(dev).eval(), dm, cfg


def _coll_on(cfg):
    cfg.TEST.COLLISION_METRICS = True


def test_collision_ratio_is_exact_on_a_constructed_scene(dev):
    """Rigidly moved ellipsoids (zero body pose, a random global orientation per frame) eight metres apart per frame and row.  The cloud
    of a sequence has, for every body, n_in in 0..5 points at half the semi-axes along random directions (inside) and four points at
    0.9 x the semi-axes along box diagonals (x^2/a^2 + y^2/b^2 + z^2/c^2 = 2.43: near the body, outside it), mapped through the
    frame's rigid transform; the float64 twin counts n_in in every frame, and the driver's four numbers are the twin's."""
    from seeme_amd.mesh_metrics import collision_from_meshes_torch
    model, dm, cfg = _mld(dev, mutate=_coll_on)
    assert model.predict_transl and model.data_type == "angle" and model.collision_metrics and not model.mesh_metrics
    B, K, T = 2, 3, 8
    lengths = [8, 5]
    g = torch.Generator().manual_seed(12)
    feats = torch.zeros(B, K + 1, T, model.nfeats)                                   # row K of a sequence is its reference
    feats[..., :3] = 1.5 * torch.randn(B, K + 1, T, 3, generator=g)                  # global orientation (axis-angle)
    feats[..., -3] = 8.0 * torch.arange(T, dtype=torch.float32)[None, None, :]       # translation: 8 m per frame along x ...
    feats[..., -1] = 8.0 * torch.arange(K + 1, dtype=torch.float32)[None, :, None]   # ... and 8 m per row along z
    feats = feats.to(dev)
    betas = torch.zeros(B, T, 10, device=dev)
    vt = torch.stack([model._feats_to_joints(feats[:, r].contiguous(), betas, True)[1] for r in range(K + 1)], dim=1)     # [B,K+1,T,V,3]
    tmpl = model.smpl_model.v_template.double().cpu()
    X = torch.cat([tmpl, torch.ones(tmpl.shape[0], 1, dtype=torch.float64)], dim=1)
    axes = torch.tensor(AXES, dtype=torch.float64)
    diag = torch.tensor([[1.0, 1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, -1.0], [-1.0, -1.0, 1.0]], dtype=torch.float64)
    per = 9
    P = (K + 1) * T * per
    scene = torch.zeros(B, P, 3, dtype=torch.float64) + torch.tensor([0.0, 100.0, 0.0], dtype=torch.float64)
    n_in = torch.randint(0, 6, (B, K + 1, T), generator=g)
    n_in[:, :, 0], n_in[:, :, 1] = 3, 0                                              # both kinds in every row
    vc = vt.double().cpu()
    for b in range(B):
        for r in range(K + 1):
            for t in range(T):
                A = torch.linalg.lstsq(X, vc[b, r, t]).solution                     # the frame's rigid transform, template -> posed
                assert float((X @ A - vc[b, r, t]).abs().max()) < 1e-4            # rigid up to fp32 rounding at 56 m
                u = torch.randn(int(n_in[b, r, t]), 3, generator=g, dtype=torch.float64)
                q = torch.cat([0.5 * axes * u / u.norm(dim=1, keepdim=True), 0.9 * axes * diag])
                s0 = (r * T + t) * per
                scene[b, s0:s0 + q.shape[0]] = torch.cat([q, torch.ones(q.shape[0], 1, dtype=torch.float64)], dim=1) @ A
    scene = scene.float().to(dev)
    faces = model.smpl_model.faces_tensor
    want = collision_from_meshes_torch(vt[:, :K].double(), vt[:, K].double(), faces, lengths, scene.double())
    valid = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None])
    assert torch.equal(want["_count"].cpu().long() * valid[:, None, :], n_in[:, :K] * valid[:, None, :])
    assert torch.equal(want["_count_ref"].cpu().long() * valid, n_in[:, K] * valid)
    f_rst = feats[:, :K].reshape(B * K, T, model.nfeats).contiguous()
    f_ref = feats[:, K].contiguous()
    cm = model._collision_metrics(f_rst, f_ref, betas, None, lengths, K, scene)
    names = ("COLLISION_RATIO", "COLLISION_FRAMES", "COLLISION_RATIO_REF", "COLLISION_FRAMES_REF")
    assert set(cm) == set(names)
    for n in names:
        print(n, cm[n].tolist())
        assert cm[n].dtype == torch.float32 and cm[n].shape == ((B,) if n.endswith("_REF") else (B, K))
        assert torch.equal(cm[n], want[n]), n
        assert 0 < float(cm[n].min()) and float(cm[n].max()) < 1
    # several chunks (one frame of K + 1 meshes is 0.32 MiB) give the bits of one chunk
    model.mesh_chunk_mb = 1.0
    cm_c = model._collision_metrics(f_rst, f_ref, betas, None, lengths, K, scene)
    for n in names:
        assert torch.equal(cm_c[n], cm[n]), n
    model.mesh_chunk_mb = 256
    # both groups from one pass: the collision keys as above, the mesh keys as without them
    both = model._mesh_metrics(f_rst, f_ref, betas, None, lengths, K, scene, mesh=True, collision=True)
    plain = model._mesh_metrics(f_rst, f_ref, betas, None, lengths, K, scene)
    assert set(both) == set(plain) | set(names) and set(plain) == {"PA_MPJPE", "V2V", "SCENE_DIST", "CONTACT_RATIO", "SCENE_DIST_REF",
                                                                   "CONTACT_RATIO_REF"}
    for n in both:
        assert torch.equal(both[n], plain[n] if n in plain else cm[n]), n


def test_ego_eval_collision_switch_is_independent_of_the_mesh_switch(dev):
    model, dm, cfg = _mld(dev, mutate=_coll_on)
    B, K = 2, 3
    batch = dm.batch(B, idx=3, with_scene=True, lengths=[8, 5])
    g = torch.Generator().manual_seed(4)
    lat, cn = torch.randn(B * K, 1, 256, generator=g).to(dev), torch.randn(1, B * K, 256, generator=g).to(dev)
    if model.do_classifier_free_guidance:
        cn = (cn, torch.randn(1, B * K, 256, generator=g).to(dev))
    sl = lambda t, dim: t.unflatten(dim, (B, K)).select(dim + 1, 0).contiguous()
    lat1, cn1 = sl(lat, 0), (tuple(sl(e, 1) for e in cn) if isinstance(cn, tuple) else sl(cn, 1))
    run_k = lambda: model.ego_eval(batch, latents=lat, cond_noise=cn, num_hypotheses=K)
    run_1 = lambda: model.ego_eval(batch, latents=lat1, cond_noise=cn1)
    names = {"COLLISION_RATIO", "COLLISION_FRAMES", "COLLISION_RATIO_REF", "COLLISION_FRAMES_REF"}
    coll_k, coll_1 = run_k(), run_1()                                                # the new switch alone
    for rs, k in ((coll_k, K), (coll_1, 1)):
        assert "mesh_metrics" not in rs and set(rs["collision_metrics"]) == names
        for n, v in rs["collision_metrics"].items():
            assert v.shape == ((B,) if n.endswith("_REF") else (B, k)) and bool(((v >= 0) & (v <= 1)).all()), n
    model.mesh_metrics = True                                                        # both
    both_k, both_1 = run_k(), run_1()
    model.collision_metrics = False                                                  # TEST.MESH_METRICS alone: today's result
    mesh_k, mesh_1 = run_k(), run_1()
    model.mesh_metrics = False                                                       # both off
    off_k, off_1 = run_k(), run_1()
    for both, mesh, coll, off in ((both_k, mesh_k, coll_k, off_k), (both_1, mesh_1, coll_1, off_1)):
        assert set(mesh) == set(off) | {"mesh_metrics"} and set(coll) == set(off) | {"collision_metrics"}
        assert set(both) == set(off) | {"mesh_metrics", "collision_metrics"}
        assert set(both["mesh_metrics"]) == set(mesh["mesh_metrics"]) == {"PA_MPJPE", "V2V", "SCENE_DIST", "CONTACT_RATIO", "SCENE_DIST_REF",
                                                                         "CONTACT_RATIO_REF"}
        for n, v in mesh["mesh_metrics"].items():
            assert torch.equal(both["mesh_metrics"][n], v), n
        for n, v in coll["collision_metrics"].items():
            assert torch.equal(both["collision_metrics"][n], v), n
    # allsplit_step feeds the accumulator
    model.collision_metrics = True
    model.num_hypotheses = K
    model.CollMetric.reset()
    model.allsplit_step("test", batch)
    got = model.CollMetric.compute()
    assert set(got) == names and float(model.CollMetric.sums()[2]) == B * K and float(model.CollMetric.sums()[5]) == B


# ----------------------------------------------------------------------------- 5. cli.test_main
_TODAY = ("MPJPE", "ROOT_ERROR", "ACCL", "HEAD_ORIENTATION_ERROR", "mpjpe_interactee", "count_seq", "seqs_per_s")
_K = ("MPJPE_best_of_k", "MPJPE_mean_of_k", "APD_JOINTS", "STD_JOINTS", "count_seq_k", "num_hypotheses", "samples_per_s")
_COLL = ("COLLISION_RATIO", "COLLISION_FRAMES", "COLLISION_RATIO_REF", "COLLISION_FRAMES_REF")


def _json_keys(names):
    return {f"Metrics/{n}{s}" for n in names for s in ("", "/mean", "/min", "/max", "/conf_interval")}


def test_cli_test_main_reports_the_collision_metrics(dev, tmp_path):
    from seeme_amd import cli
    cfgp = os.path.join(REPO, "configs", "config_mld_scene.yaml")
    size = ["--batch_size", "2", "--folder", str(tmp_path), "--frames", "16", "--scene_points", "1000"]
    r = cli.train_main(["--cfg", cfgp, "--nodebug", "--iters_per_epoch", "1", "--epochs", "1"] + size, smpl_model=_sphere_smpl())
    common = ["--cfg", cfgp, "--test_batches", "1", "--checkpoint", os.path.join(r["checkpoints"], "epoch=0.ckpt")] + size
    out = cli.test_main(common + ["--num_hypotheses", "2", "--collision_metrics"], smpl_model=_sphere_smpl())
    assert set(json.load(open(out["file"]))) == _json_keys(_TODAY + _K + _COLL)
    for n in _COLL:
        assert math.isfinite(out[f"Metrics/{n}/mean"]) and 0 <= out[f"Metrics/{n}/mean"] <= 1, n
    out1 = cli.test_main(common + ["--collision_metrics"], smpl_model=_sphere_smpl())            # K = 1
    assert set(json.load(open(out1["file"]))) == _json_keys(_TODAY + _COLL)
    off = cli.test_main(common, smpl_model=_sphere_smpl())
    assert set(json.load(open(off["file"]))) == _json_keys(_TODAY)
