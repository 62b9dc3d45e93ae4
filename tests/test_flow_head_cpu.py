"""The ProHMR-scene pose head on the CPU: the module carries the reference's state-dict entries, the plain-torch twin reproduces the
fixture made from the reference's SMPLFlow (tests/golden/make_golden_flow_head.py), the host folds equal the unfolded twin in
float64, the context order and the independence of a frame's samples are pinned, and everything that has to be refused is."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, elem_err, load_golden, rel_err
from seeme_amd import prohmr_head as PH
from seeme_amd.weights_recipe import load_flow_head_recipe_

GATE = 1e-4                                # the project's fp32 gate; the reference differs from itself in float64 by 7.9e-7


@pytest.fixture(scope="module")
def fx():
    return load_golden("flow_head.npz")


@pytest.fixture(scope="module")
def head():
    return load_flow_head_recipe_(PH.SMPLFlowHead())


@pytest.fixture(scope="module")
def twin32(fx, head):
    return PH.flow_head_torch(head, torch.from_numpy(fx["ctx"]), torch.from_numpy(fx["z"]))


def _close(got, want, gate=GATE):
    r, e = rel_err(got, want), elem_err(got, want)
    print(f"rel_err {r:.3e} elem_err {e:.3e}")
    assert r <= gate and e <= gate, (r, e)


def _cfg(**kw):
    from seeme_amd.config import parse_config
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_image_scene_backbone.yaml"))
    for k, v in kw.items():
        node = cfg
        *path, last = k.split(".")
        for p in path:
            node = node[p]
        node[last] = v
    return cfg


def _mld(**kw):
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    return MLD(_cfg(**kw), SyntheticEgoDataModule(T=8, n_points=16), smpl_model=SMPL.synthetic(1, V=64))


# ----------------------------------------------------------------------------- the module and its state dict
def test_state_dict_names_and_shapes_equal_the_reference(fx):
    sd = PH.SMPLFlowHead().state_dict()
    assert sorted(sd) == [str(k) for k in fx["keys"]]
    for k, shp in zip(fx["keys"], fx["shapes"]):
        assert ",".join(str(d) for d in sd[str(k)].shape) == str(shp), k
    assert "flow._transform._transforms.2.identity_features" in sd and "flow._transform._transforms.0.initialized" in sd
    assert "flow._transform._transforms.2.transform_net.blocks.1.batch_norm_layers.0.num_batches_tracked" in sd
    assert {k: tuple(v.shape) for k, v in sd.items()} == PH.state_shapes()


def test_recipe_loads_strictly_and_the_head_stays_frozen_in_eval_mode(head):
    m = PH.SMPLFlowHead()
    load_flow_head_recipe_(m)                                           # load_state_dict(strict=True) inside
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), head.state_dict().values()))
    m.train()
    assert not m.training and not any(x.training for x in m.modules())
    assert not any(p.requires_grad for p in m.parameters())
    var = m.state_dict()["flow._transform._transforms.2.transform_net.blocks.0.batch_norm_layers.0.running_var"]
    assert float(var.min()) >= 1.0 and float(var.max()) <= 1.3


def test_mld_grows_exactly_the_flow_entries():
    plain, grown = _mld(), _mld(**{"model.interactee_head": True})
    a, b = set(plain.state_dict()), set(grown.state_dict())
    assert a < b and b - a == {"proscene.flow." + k for k in PH.state_shapes()}
    assert not plain.interactee_head and not any(k.startswith("proscene.flow.") for k in a)
    assert not any(p.requires_grad for p in grown.proscene.flow.parameters())
    grown.train()
    assert not grown.proscene.flow.training


# ----------------------------------------------------------------------------- the twin against the reference's fixture
@pytest.mark.parametrize("name,idx", [("pose6d", 0), ("rotmat", 1), ("betas", 2), ("cam", 3), ("log_prob", 4)])
def test_twin_fp32_equals_the_reference(fx, twin32, name, idx):
    assert twin32[idx].dtype == torch.float32 and tuple(twin32[idx].shape) == fx[name].shape
    _close(twin32[idx].numpy(), fx[name])


def test_cam_to_transl_equals_the_reference(fx):
    t = lambda k: torch.from_numpy(fx[k])
    got = PH.cam_to_transl(t("cam"), t("center"), t("scale"), t("f"), t("cx"), t("cy"))
    _close(got.numpy(), fx["cam_t_full"])


def test_fixture_context_is_context_rows(fx):
    t = lambda k: torch.from_numpy(fx[k])
    ctx = t("ctx")
    again = PH.context_rows(ctx[:, 6:6 + 2048], ctx[:, 6 + 2048:], t("center"), t("scale"), t("f"), t("cx"), t("cy"))
    assert torch.equal(again, ctx) and bool((ctx[:, 6:6 + 2048] >= 0).all())


# ----------------------------------------------------------------------------- the folds
def folded_chain(f, ctx, z):
    """seeme_flow_head's definition (include/seeme_hip.h) from fold()'s tensors, float64."""
    L_, S, _ = z.shape
    x = z.reshape(L_ * S, 144).clone()
    C = ctx @ f["ctx_w"].t() + f["ctx_b"]                                # [L, 5120]
    Cr = C.repeat_interleave(S, dim=0)
    for k in range(3, -1, -1):
        par = (f["id_parity"] >> k) & 1
        idf, tf = torch.arange(par, 144, 2), torch.arange(1 - par, 144, 2)
        h = x[:, idf] @ f["id_w"][k].t() + Cr[:, 1024 * k:1024 * (k + 1)]
        for b in range(2):
            u = torch.relu(h * f["bn_s"][k, 2 * b] + f["bn_o"][k, 2 * b]) @ f["lin_w"][k, 2 * b].t()
            u = torch.relu(u * f["bn_s"][k, 2 * b + 1] + f["bn_o"][k, 2 * b + 1]) @ f["lin_w"][k, 2 * b + 1].t()
            h = h + u + f["res_b"][k, b]
        x[:, tf] -= h @ f["fin_w"][k].t() + f["fin_b"][k]
        x = (x @ f["lu_w"][k].t()) * f["act_s"][k] + f["act_o"][k]
    off = torch.relu(C[:, 4096:]) @ f["fc_w"].t() + f["fc_b"]
    log_prob = -0.5 * (z * z).sum(-1) + f["log_const"]
    return x.reshape(L_, S, 144), off[:, :10], off[:, 10:], log_prob


def test_fold_equals_the_unfolded_twin_in_float64(fx, head):
    ctx, z = torch.from_numpy(fx["ctx"]).double(), torch.from_numpy(fx["z"]).double()
    pose, _rot, betas, cam, lp = PH.flow_head_torch(head, ctx, z)
    f = PH.fold(head)
    assert f["ctx_w"].shape == (5 * 1024, 2566) and f["ctx_w"].dtype == torch.float64 and f["lu_w"].shape == (4, 144, 144)
    assert f["id_parity"] == 0b1010                                     # identity = even indices in layers 0 and 2, odd in 1 and 3
    got = folded_chain(f, ctx, z)
    for g, w in zip(got, (pose, betas, cam, lp)):
        r = rel_err(g.numpy(), w.numpy())
        print(f"{r:.3e}")
        assert r <= 1e-10
    assert PH.fold(head) is f                                           # cached under the fingerprint ...
    sd = head.state_dict()
    head.load_state_dict(sd)
    assert PH.fold(head) is not f                                       # ... and stale after a load


def test_log_det_constant_is_the_reference_log_prob_of_the_mode(fx, head):
    f = PH.fold(head)
    assert abs(f["log_const"] - float(fx["log_prob"][0, 0])) <= 1e-4 * abs(float(fx["log_prob"][0, 0]))
    assert np.all(fx["z"][:, 0] == 0)


# ----------------------------------------------------------------------------- properties
def test_every_scalar_slot_of_the_context_is_read_in_its_place(fx, head):
    ctx, z = torch.from_numpy(fx["ctx"][:1]).double(), torch.from_numpy(fx["z"][:1, :2]).double()
    base = PH.flow_head_torch(head, ctx, z)
    for i in range(6):
        for j in range(i + 1, 6):
            c = ctx.clone()
            c[:, [i, j]] = c[:, [j, i]]
            out = PH.flow_head_torch(head, c, z)
            assert rel_err(out[0].numpy(), base[0].numpy()) > 1e-6 and rel_err(out[3].numpy(), base[3].numpy()) > 1e-6, (i, j)


def test_samples_of_a_frame_are_independent(fx, head):
    """z = 0 in sample 0 gives the mode whatever the other samples hold, and a sample computed alone is the sample computed among
    others.  float64: independence is exact algebra, so only rounding that depends on the batch's shape (the host GEMM's blocking)
    may differ, 1e-12 of the largest value at the most."""
    ctx, z = torch.from_numpy(fx["ctx"]).double(), torch.from_numpy(fx["z"]).double()
    base = PH.flow_head_torch(head, ctx, z)
    z2 = z.clone()
    z2[:, 1:] = torch.randn(z[:, 1:].shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    other = PH.flow_head_torch(head, ctx, z2)
    assert rel_err(other[0][:, 0].numpy(), base[0][:, 0].numpy()) <= 1e-12 and torch.equal(other[4][:, 0], base[4][:, 0])      # the mode
    assert rel_err(other[0][:, 1].numpy(), base[0][:, 1].numpy()) > 1e-2
    alone = PH.flow_head_torch(head, ctx, z2[:, 2:3])
    assert rel_err(alone[0][:, 0].numpy(), other[0][:, 2].numpy()) <= 1e-12 and rel_err(alone[4][:, 0].numpy(), other[4][:, 2].numpy()) <= 1e-12
    zz = PH.draw_z(3, 4, torch.Generator().manual_seed(5))
    assert not zz[:, 0].any() and zz[:, 1:].std() > 0.5 and torch.equal(zz, PH.draw_z(3, 4, torch.Generator().manual_seed(5)))


def test_head_box_is_centred_on_the_stored_centre():
    from seeme_amd import crops as CR
    c, s = np.array([[100.0, 50.0], [7.5, 9.0]], np.float32), np.array([1.5, 0.25], np.float32)
    hb, pb = PH.head_box(c, s), CR.boxes_of(c, s)
    assert np.array_equal(hb[:, :2], c) and np.array_equal(hb[:, 2], s * 200) and hb.dtype == np.float32
    assert np.array_equal(pb[:, 2], hb[:, 2]) and np.array_equal(pb[:, :2], c + hb[:, 2:3])      # SEE-ME's box is shifted by b


# ----------------------------------------------------------------------------- refusals
def test_bad_shapes_are_refused(head):
    ctx, z = torch.zeros(2, 2566), torch.zeros(2, 1, 144)
    for bad_ctx, bad_z in ((ctx[:, :-1], z), (ctx, z[:1]), (ctx, z[:, :, :-1]), (ctx, torch.zeros(2, 33, 144)), (ctx, torch.zeros(2, 0, 144))):
        with pytest.raises(ValueError):
            PH.flow_head_torch(head, bad_ctx, bad_z)
        with pytest.raises(ValueError):
            PH.flow_head_hip(head, bad_ctx, bad_z)
    from seeme_amd._lib import SeemeError
    with pytest.raises(SeemeError, match="no CPU fallback"):
        PH.flow_head_hip(head, ctx, z)                                  # a CPU tensor: there is no fallback


def test_cam_scale_not_positive_is_refused_by_frame():
    cam = torch.tensor([[0.9, 0.0, 0.0], [0.0, 0.1, 0.1], [-1.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="frame 1"):
        PH.cam_to_transl(cam, torch.zeros(3, 2), torch.ones(3), 1000.0, 500.0, 300.0)
    cam[1, 0] = float("nan")
    with pytest.raises(ValueError, match="frame 1"):
        PH.cam_to_transl(cam, torch.zeros(3, 2), torch.ones(3), 1000.0, 500.0, 300.0)


def test_bad_interactee_head_value_is_refused():
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="model.interactee_head"):
            _mld(**{"model.interactee_head": bad})
    with pytest.raises(NotImplementedError, match="model.interactee_head"):
        _mld().estimate_interactee(torch.zeros(1, 2048), torch.zeros(1, 512), torch.zeros(1, 2), torch.ones(1), [1000.0, 500.0, 300.0])


def test_checkpoint_without_flow_entries_names_the_first_missing_key(head):
    sd = head.state_dict()
    first = next(iter(PH.state_shapes()))
    with pytest.raises(KeyError, match="proscene.flow." + first.replace(".", r"\.")):
        PH.flow_state_from_checkpoint({"vae.x": torch.zeros(1)})
    see_me = {"proscene.flow." + k: v for k, v in sd.items()}
    see_me["proscene.scene_enc.fc_c.weight"] = torch.zeros(1)
    assert list(PH.flow_state_from_checkpoint(see_me)) == list(sd)
    prohmr = {"flow." + k: v for k, v in sd.items()}
    prohmr.update({"smpl.shapedirs": torch.zeros(1), "discriminator.D_conv1.weight": torch.zeros(1), "backbone.conv1.weight": torch.zeros(1)})
    got = PH.flow_state_from_checkpoint(prohmr)
    PH.SMPLFlowHead().load_state_dict(got, strict=True)
    gone = dict(prohmr)
    del gone["flow.fc_head.init_cam"]
    with pytest.raises(KeyError, match=r"flow\.fc_head\.init_cam"):
        PH.flow_state_from_checkpoint(gone)


# ----------------------------------------------------------------------------- the recording side
def _estimate_input(n=4, H=12, W=16):
    g = np.random.default_rng(2)
    w2c = np.tile(np.eye(4), (n, 1, 1))
    return {"video": g.integers(0, 256, (n, H, W, 3), dtype=np.uint8), "center": g.uniform(4, 10, (n, 2)).astype(np.float32),
            "scale": g.uniform(0.02, 0.04, n).astype(np.float32), "cam_intrinsics": np.array([20.0, 8.0, 6.0], np.float32),
            "world2cam": w2c, "scene_vertices": g.normal(size=(50, 3)).astype(np.float32)}


def _interactee(n):
    g = np.random.default_rng(3)
    return {"global_orient": g.normal(size=(n, 3)).astype(np.float32), "body_pose": g.normal(size=(n, 69)).astype(np.float32),
            "transl": g.normal(size=(n, 3)).astype(np.float32), "betas": g.normal(size=10).astype(np.float32)}


def test_load_recording_without_the_interactee(tmp_path):
    from seeme_amd import recording as R
    path = str(tmp_path / "rec.npz")
    d = _estimate_input()
    np.savez(path, **d)
    rec = R.load_recording(path, require_interactee=False)
    assert rec["n_frames"] == 4 and rec["cam_intrinsics"].shape == (4, 3) and rec["cam_intrinsics"].dtype == np.float32
    assert np.array_equal(rec["video_index"], np.arange(4)) and "global_orient" not in rec
    with pytest.raises(ValueError, match="missing"):                    # the default still asks for the interactee
        R.load_recording(path)
    # interactee keys and require_interactee=False: the file is an input of predict, not of estimate
    np.savez(path, **d, **_interactee(4))
    with pytest.raises(ValueError, match="already"):
        R.load_recording(path, require_interactee=False)
    full = R.load_recording(path)                                       # ... and as such it loads, cam_intrinsics validated, extras ignored
    assert full["n_frames"] == 4 and full["cam_intrinsics"].shape == (4, 3)
    np.savez(path, **d, **_interactee(4), interactee_log_prob=np.zeros((4, 2), np.float32), scene_view_count=np.ones(4, np.int32))
    assert R.load_recording(path)["n_frames"] == 4
    # a video_index that skips a frame names the first frame without an image
    sparse = dict(d, video=d["video"][[0, 1, 3]], video_index=np.array([0, 1, 3]))
    np.savez(path, **sparse)
    with pytest.raises(ValueError, match="frame 2 has no stored image"):
        R.load_recording(path, require_interactee=False)
    np.savez(path, **dict(d, video=d["video"][:3], video_index=np.array([0, 1, 2])))
    with pytest.raises(ValueError, match="frame 3 has no stored image"):
        R.load_recording(path, require_interactee=False)
    for gone in ("cam_intrinsics", "world2cam", "scene_vertices", "scale"):
        np.savez(path, **{k: v for k, v in d.items() if k != gone})
        with pytest.raises(ValueError, match=gone):
            R.load_recording(path, require_interactee=False)


def test_bad_intrinsics_name_the_frame(tmp_path):
    from seeme_amd import recording as R
    K = np.tile(np.array([20.0, 8.0, 6.0]), (4, 1))
    for f, (col, val) in ((2, (0, 0.0)), (1, (0, -3.0)), (3, (1, np.nan)), (0, (2, np.inf))):
        bad = K.copy()
        bad[f, col] = val
        with pytest.raises(ValueError, match=f"frame {f}"):
            R.check_intrinsics(bad, 4)
    with pytest.raises(ValueError, match="expected"):
        R.check_intrinsics(np.zeros((3, 3)), 4)
    path = str(tmp_path / "rec.npz")
    np.savez(path, **dict(_estimate_input(), cam_intrinsics=np.array([0.0, 8.0, 6.0])))
    with pytest.raises(ValueError, match="frame 0"):
        R.load_recording(path, require_interactee=False)


def test_camera_axes_are_a_rotation():
    from seeme_amd import recording as R
    assert R.check_camera_axes([1, -1, -1]) == (1, -1, -1) and R.check_camera_axes([1, 1, 1]) == (1, 1, 1)
    for bad in ([1, 1, -1], [-1, -1, -1], [1, -1], [1, -1, -2], [1.5, 1, 1], "xyz", None, [True, 1, 1]):
        with pytest.raises(ValueError, match="INTERACTEE_CAMERA_AXES"):
            R.check_camera_axes(bad)
    with pytest.raises(ValueError, match="INTERACTEE_CAMERA_AXES"):
        _mld(**{"TEST.INTERACTEE_CAMERA_AXES": [1, 1, -1]})
    assert _mld().interactee_camera_axes == (1, -1, -1)
    M = np.tile(np.eye(4), (2, 1, 1))
    assert np.array_equal(R.opencv_views(M, [1, -1, -1])[1], np.diag([1.0, -1.0, -1.0, 1.0]))


@pytest.mark.parametrize("axes", [(1, -1, -1), (1, 1, 1)])
def test_a_camera_frame_body_moved_to_the_world_is_the_rigidly_moved_body(axes):
    """ProHMR's body in the camera frame is SMPL posed without a translation plus cam_t; its world joints must be those joints
    moved by inv(D world2cam).  Synthetic SMPL, float64."""
    from seeme_amd import recording as R
    from seeme_amd.smpl import SMPL
    from test_scene_views_cpu import _exact_joints, _params, _rigid_maps
    smpl = SMPL.synthetic(1234, V=431)
    n = 5
    aa, cam_t, _ = _params(n, 9)
    betas = 0.5 * torch.randn(10, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    bn = betas[None].expand(n, 10)
    w2c = _rigid_maps(n, 10).numpy()
    J0 = R.rest_pelvis(smpl, betas[None])[0]
    in_camera = _exact_joints(smpl, bn, aa, None) + cam_t[:, None]
    go, tr = R.camera_body_to_world(aa[:, :3], cam_t, J0, w2c, axes)
    in_world = _exact_joints(smpl, bn, torch.cat([go, aa[:, 3:]], dim=1), tr)
    inv = np.linalg.inv(np.diag([*axes, 1.0])[None] @ w2c)
    want = torch.einsum("nij,nkj->nki", torch.from_numpy(inv[:, :3, :3]), in_camera) + torch.from_numpy(inv[:, None, :3, 3])
    assert float((in_world - want).abs().max()) <= 1e-9
    # with samples: [L,S,3] in, the same numbers out
    go2, tr2 = R.camera_body_to_world(aa[:, None, :3].expand(n, 2, 3), cam_t[:, None].expand(n, 2, 3), J0, w2c, axes)
    assert torch.equal(go2[:, 1], go) and torch.equal(tr2[:, 0], tr)
    # a J0 that is not the pelvis of the betas moves the body: the handling is pinned
    _, off = R.camera_body_to_world(aa[:, :3], cam_t, J0 + 0.1, w2c, axes)
    assert float((off - tr).abs().max()) > 1e-3
