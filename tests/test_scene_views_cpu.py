"""Recordings from a moving camera on the CPU: the scene-view twin in float64 against the per-view loop of
tests/scene_views_reference.py, the rigid re-framing of SMPL parameters and joints on the synthetic SMPL model, ``windows_batch`` with
world2cam against a float64 host restatement, the validation of the new recording keys and the C-ABI of seeme_scene_views."""
import os

import numpy as np
import pytest
import torch

import scene_views_reference as SV
from seeme_amd import recording as R

TOL_F32 = 1e-4               # the project's fp32 bound


# ----------------------------------------------------------------------------- 1. the twin against the restatement
@pytest.mark.parametrize("NP", [(150, 8), (150, 1), (150, 64), (1, 8), (40, 64)], ids=str)
def test_scene_views_twin_vs_restatement_with_controlled_counts(NP):
    N, P = NP
    verts, M, counts = SV.controlled_case(N, P, seed=N + P)
    assert SV.margin(verts, M) >= SV.MARGIN                            # on the inputs: no vertex within 1e-3 of any view's plane
    cloud, index, count = SV.restate(verts, M, P)
    assert count[:len(counts)].tolist() == counts                      # all of {0, 1, P-1, P, P+1, 2P-1, 2P, 2P+1, N} that fit, in ONE call
    got = R.scene_views_torch(torch.from_numpy(verts), torch.from_numpy(M), P)
    assert got["cloud"].dtype == torch.float64 and got["index"].dtype == torch.int32 and got["count"].dtype == torch.int32
    assert got["cloud"].shape == (len(M), P, 3) and got["index"].shape == (len(M), P) and got["count"].shape == (len(M),)
    assert np.array_equal(got["count"].numpy(), count) and np.array_equal(got["index"].numpy(), index)
    assert np.abs(got["cloud"].numpy() - cloud).max() <= 1e-12
    # the rows of a view are its source vertices moved by the view, and survivors only
    for w in range(len(M)):
        if count[w] == 0:
            assert (got["index"][w] == -1).all() and float(got["cloud"][w].abs().max()) == 0.0
        else:
            assert float(got["cloud"][w, :, 2].min()) > 0
            assert (np.diff(index[w][:min(P, count[w])]) > 0).all()    # vertex order is kept
    # a view's result does not depend on the other views of the call
    alone = R.scene_views_torch(torch.from_numpy(verts), torch.from_numpy(M[-1:]), P)
    assert torch.equal(alone["cloud"][0], got["cloud"][-1]) and torch.equal(alone["index"][0], got["index"][-1])


def test_scene_views_twin_fp32_agrees_where_the_margin_holds_and_refuses_bad_shapes():
    N, P = 300, 16
    verts, M, _ = SV.controlled_case(N, P, seed=3)
    assert SV.margin(verts, M) >= SV.MARGIN
    v32, M32 = torch.from_numpy(verts).float(), torch.from_numpy(M).float()
    assert SV.margin(v32.double().numpy(), M32.double().numpy()) >= 0.5 * SV.MARGIN        # ... also after the rounding to fp32
    want = R.scene_views_torch(v32.double(), M32.double(), P)
    got = R.scene_views_torch(v32, M32, P)
    assert torch.equal(got["index"], want["index"]) and torch.equal(got["count"], want["count"])
    assert float((got["cloud"].double() - want["cloud"]).abs().max()) <= TOL_F32
    # a NaN vertex compares false: it never survives
    v_nan = v32.clone()
    v_nan[5] = float("nan")
    assert not bool((R.scene_views_torch(v_nan, M32, P)["index"] == 5).any())
    with pytest.raises(ValueError):
        R.scene_views_torch(v32[:, :2], M32, P)
    with pytest.raises(ValueError):
        R.scene_views_torch(v32, M32[:, :3], P)
    with pytest.raises(ValueError):
        R.scene_views_torch(v32, M32, 0)


# ----------------------------------------------------------------------------- 2. re-framing of SMPL parameters and joints
@pytest.fixture(scope="module")
def smpl():
    from seeme_amd.smpl import SMPL
    return SMPL.synthetic(1234, V=431)


def _rigid_maps(n, seed):
    g = np.random.default_rng(seed)
    M = np.stack([SV.rigid(g.normal(size=3), g.uniform(-3, 3, 3)) for _ in range(n)])
    return torch.from_numpy(M)


def _exact_joints(smpl, betas, aa, transl):
    """SMPL joints with Rodrigues' formula at the EXACT angle |aa|.  (The project's ``smpl_joints_torch`` follows smplx and takes
    the angle of aa + 1e-8: a rotation that is off by about 1e-8 rad, more than the float64 bound of this test; the fp32 case
    below uses it.)"""
    from seeme_amd.vae_autograd import _smpl_joints_from_rotmat
    Rm = torch.from_numpy(SV.rodrigues(aa.numpy().reshape(-1, 24, 3)))
    return _smpl_joints_from_rotmat(smpl, betas, Rm, transl)


def _params(n, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    aa = 0.4 * rn(n, 72)
    aa[:, :3] = 0.8 * rn(n, 3)                                          # global orientation: angles well inside (0, pi)
    return aa, rn(n, 3), 0.5 * rn(n, 10)


@pytest.mark.parametrize("has_transl", [True, False], ids=["angle_transl", "angle"])
def test_reframe_smpl_joints_of_the_reframed_parameters_are_the_reframed_joints(smpl, has_transl):
    n = 6
    aa, tr, betas = _params(n, 5)
    M = _rigid_maps(n, 6)
    A, a = R.rigid_parts(M)
    J0 = R.rest_pelvis(smpl, betas)
    zero = torch.zeros(n, 72, dtype=torch.float64)
    assert float((J0 - _exact_joints(smpl, betas, zero, None)[:, 0]).abs().max()) <= 1e-12      # the rest pelvis IS joint 0 at zero pose
    before = _exact_joints(smpl, betas, aa, tr if has_transl else None)
    go2, tr2 = R.reframe_smpl(aa[:, :3], tr, J0, A, a)
    aa2 = torch.cat([go2, aa[:, 3:]], dim=1)
    after = _exact_joints(smpl, betas, aa2, tr2 if has_transl else None)
    want = R.reframe_joints(before, J0, A, a, has_transl)
    assert float((after - want).abs().max()) <= 1e-9
    # the independent form of both rules
    Rg = torch.from_numpy(SV.rodrigues(aa[:, :3].numpy()))
    assert float((torch.from_numpy(SV.rodrigues(go2.numpy())) - A @ Rg).abs().max()) <= 1e-12
    moved = torch.einsum("nij,nkj->nki", A, before) + a[:, None]
    if has_transl:
        assert float((want - moved).abs().max()) <= 1e-12
    else:                                                              # without a translation the pelvis stays where it was
        assert float((want[:, 0] - before[:, 0]).abs().max()) <= 1e-12
    # a map followed by its inverse
    Ai, ai = R.rigid_parts(R.rigid_inverse(M))
    go3, tr3 = R.reframe_smpl(go2, tr2, J0, Ai, ai)
    assert float((go3 - aa[:, :3]).abs().max()) <= 1e-9 and float((tr3 - tr).abs().max()) <= 1e-9
    assert float((R.reframe_joints(want, J0, Ai, ai, has_transl) - before).abs().max()) <= 1e-9
    # fp32, with the project's own joints function, at the project's bound
    from seeme_amd.vae_autograd import smpl_joints_torch
    f = lambda t: t.float()
    b32 = smpl_joints_torch(smpl, f(betas), f(aa), f(tr) if has_transl else None)
    go32, tr32 = R.reframe_smpl(f(aa[:, :3]), f(tr), f(J0), f(A), f(a))
    a32 = smpl_joints_torch(smpl, f(betas), torch.cat([go32, f(aa[:, 3:])], dim=1), tr32 if has_transl else None)
    assert go32.dtype == torch.float32 and float((a32 - R.reframe_joints(b32, f(J0), f(A), f(a), has_transl)).abs().max()) <= TOL_F32
    go33, tr33 = R.reframe_smpl(go32, tr32, f(J0), f(Ai), f(ai))
    assert float((go33 - f(aa[:, :3])).abs().max()) <= TOL_F32 and float((tr33 - f(tr)).abs().max()) <= TOL_F32


def test_reframe_rot6d_joints_of_the_reframed_features_are_the_reframed_joints(smpl):
    from seeme_amd.vae_autograd import smpl_joints_rot6d_torch
    n = 6
    aa, _, _ = _params(n, 8)
    Rm = torch.from_numpy(SV.rodrigues(aa.numpy().reshape(n, 24, 3)))
    r6 = torch.cat([Rm[..., :, 0], Rm[..., :, 1]], dim=-1)              # model-side order: the two columns one after the other
    M = _rigid_maps(n, 9)
    A, a = R.rigid_parts(M)
    J0 = R.rest_pelvis(smpl, torch.zeros(n, 10, dtype=torch.float64))   # rot6d is posed with zero betas and no translation
    before = smpl_joints_rot6d_torch(smpl, None, r6)
    r6b = r6.clone()
    r6b[:, 0] = R.reframe_rot6d(r6[:, 0], A)
    after = smpl_joints_rot6d_torch(smpl, None, r6b)
    want = R.reframe_joints(before, J0, A, a, False)
    assert float((after - want).abs().max()) <= 1e-9
    assert float((want[:, 0] - before[:, 0]).abs().max()) <= 1e-12
    Ai, ai = R.rigid_parts(R.rigid_inverse(M))
    assert float((R.reframe_rot6d(r6b[:, 0], Ai) - r6[:, 0]).abs().max()) <= 1e-9
    assert float((R.reframe_joints(want, J0, Ai, ai, False) - before).abs().max()) <= 1e-9
    f = lambda t: t.float()
    r32 = f(r6).clone()
    r32[:, 0] = R.reframe_rot6d(f(r6[:, 0]), f(A))
    e = (smpl_joints_rot6d_torch(smpl, None, r32) - R.reframe_joints(smpl_joints_rot6d_torch(smpl, None, f(r6)), f(J0), f(A), f(a), False)).abs().max()
    assert float(e) <= TOL_F32
    assert float((R.reframe_rot6d(r32[:, 0], f(Ai)) - f(r6[:, 0])).abs().max()) <= TOL_F32


# ----------------------------------------------------------------------------- 3. windows_batch with world2cam
def _recording(n, seed=0, pose=69):
    g = np.random.default_rng(seed)
    rec = {"global_orient": 0.6 * g.standard_normal((n, 3)), "body_pose": 0.3 * g.standard_normal((n, pose)),
           "transl": g.standard_normal((n, 3)), "betas": g.standard_normal(10), "wearer_betas": g.standard_normal(10),
           "scene": g.uniform(-3, 3, (50, 3))}
    return {k: v.astype(np.float32) for k, v in rec.items()}


def _camera_path(n, seed=0):
    """A camera that yaws and drifts from frame to frame: world2cam [n,4,4] float64."""
    g = np.random.default_rng(seed)
    rot0, t0 = g.normal(size=3) * 0.5, g.uniform(-2, 2, 3)
    return np.stack([SV.rigid(rot0 + np.array([0.0, 0.03 * f, 0.0]), t0 + 0.02 * f) for f in range(n)])


def test_windows_batch_with_world2cam_vs_float64_host_restatement(smpl):
    n, T, O = 19, 8, 3
    rec = _recording(n)
    rec["n_frames"] = n
    w2c = _camera_path(n)
    stats = (np.zeros((1, 75), np.float32), np.ones((1, 75), np.float32))          # raw values: (x - 0) / 1
    cond = ("text", "interactee", "scene")
    pelvis = R.rest_pelvis(smpl, torch.from_numpy(rec["betas"]).double()[None])[0]
    with pytest.raises(ValueError, match="pelvis"):
        R.windows_batch(rec, stats, T, O, cond, dataset="egobody", world2cam=w2c)
    batch, starts, lengths, frames = R.windows_batch(rec, stats, T, O, cond, dataset="egobody", world2cam=w2c, pelvis=pelvis)
    assert starts == [0, 5, 10, 15] and lengths == [8, 8, 8, 4] and frames["scene_view_count"] is None
    assert np.array_equal(frames["world2cam"].numpy(), w2c[starts])
    motion, transl, beta, _u, scene, length = batch
    J0 = pelvis.numpy()
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        A, a = w2c[lo, :3, :3], w2c[lo, :3, 3]
        Rw = A @ SV.rodrigues(rec["global_orient"][lo:lo + ln].astype(np.float64))
        angle = np.arccos(np.clip((np.trace(Rw, axis1=1, axis2=2) - 1) / 2, -1, 1))
        assert 0.05 < angle.min() and angle.max() < 3.0                # (the trace form of the log is good there)
        assert np.abs(motion[w, :ln, 1, :3].numpy() - SV.log_rotation(Rw)).max() <= 1e-5
        tw = (J0 + rec["transl"][lo:lo + ln].astype(np.float64)) @ A.T + a - J0
        assert np.abs(transl[w, 1, :ln].numpy() - tw).max() <= 1e-5
        assert np.array_equal(motion[w, :ln, 1, 3:].numpy(), rec["body_pose"][lo:lo + ln])           # the body pose is untouched
        assert float(motion[w, ln:, 1].abs().max() if ln < T else 0.0) == 0.0                          # padding stays the zero frame
        assert np.abs(scene[w].numpy() - (rec["scene"].astype(np.float64) @ A.T + a)).max() <= 1e-5   # the fixed cloud, moved
    assert float(motion[:, :, 0].abs().max()) == 0 and float(transl[:, 0].abs().max()) == 0
    # the recording's own key does the same as the argument
    again = R.windows_batch({**rec, "world2cam": w2c}, stats, T, O, cond, dataset="egobody", pelvis=pelvis)
    assert all(torch.equal(x, y) for x, y in zip(again[0], batch))
    # scene_vertices are selected per view by the kernel: no device, no views
    rv = {k: v for k, v in rec.items() if k != "scene"}
    rv["scene_vertices"] = rec["scene"]
    with pytest.raises(ValueError, match="device"):
        R.windows_batch(rv, stats, T, O, cond, dataset="egobody", world2cam=w2c, pelvis=pelvis)
    with pytest.raises(ValueError, match="world2cam"):
        R.windows_batch(rv, stats, T, O, cond, dataset="egobody")


def test_windows_batch_without_world2cam_is_bit_identical_to_the_load_time_rule():
    from seeme_amd.data import load_time_stats, normalise_person
    n, T, O = 19, 8, 3
    rec = _recording(n, seed=2)
    rec["n_frames"] = n
    g = np.random.default_rng(1)
    mean, std = g.standard_normal((1, 75)).astype(np.float32), (0.5 + g.random((1, 75))).astype(np.float32)
    made = R.windows_batch(rec, (mean, std), T, O, ("text", "interactee", "scene"), dataset="egobody")
    assert len(made) == 3
    batch, starts, lengths = made
    m, s = load_time_stats(mean, std, False)
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        pad = lambda x: np.concatenate([x[lo:lo + ln], np.zeros((T - ln, x.shape[1]), np.float32)])
        mo, tr = normalise_person(pad(rec["global_orient"]), pad(rec["body_pose"]), pad(rec["transl"]), m, s, "egobody", True)
        assert np.array_equal(batch[0][w, :, 1].numpy(), mo) and np.array_equal(batch[1][w, 1].numpy(), tr)
        assert np.array_equal(batch[4][w].numpy(), rec["scene"])


# ----------------------------------------------------------------------------- 4. validation of the new keys
def test_load_recording_validates_world2cam_and_scene_vertices(tmp_path):
    n = 6
    rec = _recording(n)
    w2c = _camera_path(n)
    verts = np.random.default_rng(0).uniform(-3, 3, (40, 3)).astype(np.float32)
    save = lambda name, d: (np.savez(os.path.join(tmp_path, name), **d), os.path.join(tmp_path, name))[1]
    no_scene = {k: v for k, v in rec.items() if k != "scene"}
    good = R.load_recording(save("good.npz", {**no_scene, "world2cam": w2c, "scene_vertices": verts}))
    assert good["world2cam"].dtype == np.float64 and np.array_equal(good["world2cam"], w2c)
    assert good["scene_vertices"].dtype == np.float32 and np.array_equal(good["scene_vertices"], verts)
    mirrored, sheared, last_row, wrong_shape = w2c.copy(), w2c.copy(), w2c.copy(), w2c[:5]
    mirrored[2, :3, 0] *= -1.0                                          # orthonormal, determinant -1
    sheared[4, 0, 1] += 0.01
    last_row[3, 3, 0] = 0.5
    for name, bad, frame in (("mirrored", mirrored, "frame 2"), ("sheared", sheared, "frame 4"), ("last_row", last_row, "frame 3"),
                             ("shape", wrong_shape, r"\[6,4,4\]")):
        with pytest.raises(ValueError, match=frame):
            R.load_recording(save(name + ".npz", {**no_scene, "world2cam": bad}))
    with pytest.raises(ValueError, match="world2cam"):
        R.load_recording(save("verts_only.npz", {**no_scene, "scene_vertices": verts}))
    with pytest.raises(ValueError, match="both"):
        R.load_recording(save("both.npz", {**rec, "world2cam": w2c, "scene_vertices": verts}))
    with pytest.raises(ValueError, match="scene_vertices"):
        R.load_recording(save("flat.npz", {**no_scene, "world2cam": w2c, "scene_vertices": verts.reshape(-1)}))


# ----------------------------------------------------------------------------- 5. the C-ABI
def test_scene_views_entry_points_are_declared_bound_and_exported():
    import ctypes
    from conftest import REPO
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("seeme_scene_views", "seeme_scene_views_workspace_bytes"):
        assert f"{name}(" in hdr and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert f"#define SEEME_SCENE_VIEW_TILE {R.SCENE_VIEW_TILE}\n" in hdr
    assert f"#define SEEME_SCENE_VIEW_WINDOWS_PER_PASS {R.SCENE_VIEW_WINDOWS_PER_PASS}\n" in hdr
    L = _lib.lib()
    ws = L.seeme_scene_views_workspace_bytes
    assert ws(0, 4, 8) == 0 and ws(100, 4097, 8) == 0 and ws(100, 4, 0) == 0
    assert ws((1 << 24) + 1, 4, 8) == 0 and ws(100, 0, 8) == 0 and ws(100, 4, (1 << 20) + 1) == 0
    tiles = lambda N: -(-N // R.SCENE_VIEW_TILE)
    for N, W in ((1, 1), (R.SCENE_VIEW_TILE, 3), (R.SCENE_VIEW_TILE + 1, 17), (1 << 24, 4096)):
        assert ws(N, W, 8) == W * tiles(N) * 4
