"""The headset's orientation on the device: seeme_head_rot_cost against its float64 twin on the fp32 inputs the kernel saw, the planted
choice through seeme_path_select, bad arguments, and the new options of MLD.predict_recording and cli.predict_main (head_rot,
head_rot_weight, head_rot_report, head_offset).

Bounds: TOL_F32 and _elem_rel of tests/test_gpu_hyp_select.py.  cost is held element-wise to TOL_F32.  angle is held element-wise to
TOL_F32 where it is at least 5 degrees and to the absolute bound of a 5 degree angle (TOL_F32 x 5 degrees) below that, so no frame
goes unchecked.  A CPU fp32 emulation of the definition on the inputs of head_rot_reference.rot_inputs (200 trials, the window
lengths T of COST_CASES) gave a worst absolute error of 2.7e-5 degrees, a worst relative error of 4.2e-6 at angles >= 5 degrees and
3 % of the frames below 5 degrees: the quaternion products cost about 1e-7 absolute in |vec|, 1e-5 degrees in the angle."""
import os

import numpy as np
import pytest
import torch

import head_rot_reference as HR
import recording_reference as REF
from headset_reference import cost_lengths
from test_gpu_headset import PARENT_KEYS, _camera, _flat, moving_case, scene_model  # noqa: F401 (the fixtures of the moving camera)
from test_gpu_hyp_select import TOL_F32, _draws, _elem_rel, _mld
from test_gpu_recording import _mut, _synthetic_recording

pytestmark = pytest.mark.gpu

COST_CASES = [(1, 1, 1), (2, 3, 2), (3, 32, 5), (2, 5, 63), (2, 5, 64), (2, 5, 65), (3, 4, 196)]
WIDTHS = (72, 75, 69, 144)
ANGLE_FLOOR_DEG = 5.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _angle_errors(got, want, lengths):
    """(frames t < n, those of them >= the floor, the worst relative error there, the worst absolute error below it); frames t >= n
    must be exact zeros."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    live = torch.zeros_like(want, dtype=torch.bool)
    for w, n in enumerate(lengths):
        if n > 1:
            live[w, :, :min(n, want.shape[2])] = True
    assert float(got[~live].abs().sum()) == 0.0 and float(want[~live].abs().sum()) == 0.0
    err = (got - want).abs()
    big = live & (want >= ANGLE_FLOOR_DEG)
    small = live & ~big
    rel = float((err[big] / want[big]).max()) if big.any() else 0.0
    return int(live.sum()), int(big.sum()), rel, float(err[small].max()) if small.any() else 0.0


def _hold_angle(got, want, lengths, what):
    n_live, n_big, rel, small = _angle_errors(got, want, lengths)
    print(f"{what}: {n_big} of {n_live} frames >= {ANGLE_FLOOR_DEG:g} degrees, element-wise relative error {rel:.3e}; below it absolute error "
          f"{small:.3e} degrees")
    assert rel <= TOL_F32 and small <= TOL_F32 * ANGLE_FLOOR_DEG
    return n_live, n_big


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("shape", COST_CASES, ids=str)
def test_head_rot_cost_kernel_vs_float64_twin(dev, shape, F):
    from seeme_amd.recording import head_rot_cost_hip, head_rot_cost_torch
    W, K, T = shape
    layout = HR.LAYOUT_OF_F[F]
    f32, q32 = (torch.from_numpy(a) for a in HR.rot_inputs(W, K, T, F))
    fd, qd = f32.to(dev), q32.to(dev)
    cols = torch.from_numpy(HR.chain_columns(F, layout))
    live = big = 0
    for lengths in cost_lengths(W, T):
        want = head_rot_cost_torch(f32.double(), layout, q32.double(), lengths)   # float64 on the fp32 inputs the kernel sees
        got = head_rot_cost_hip(fd, layout, qd, lengths)
        torch.cuda.synchronize()
        assert set(got) == {"cost", "angle"} and got["cost"].shape == (W, K) and got["angle"].shape == (W, K, T)
        assert got["cost"].dtype == got["angle"].dtype == torch.float32
        e = _elem_rel(got["cost"], want["cost"])
        print(f"head_rot_cost {shape} F {F} lengths {lengths}: cost max element-wise relative error {e:.3e}, values "
              f"{float(want['cost'].min()):.2f} .. {float(want['cost'].max()):.2f} degrees")
        assert e <= TOL_F32, e
        a, b = _hold_angle(got["angle"], want["angle"], lengths, "  angle")
        live, big = live + a, big + b
        for w, n in enumerate(lengths):
            if n <= 1:
                assert float(got["cost"][w].abs().max()) == 0.0 and float(got["angle"][w].abs().max()) == 0.0
        again = head_rot_cost_hip(fd, layout, qd, lengths)                        # bitwise reproducible
        assert torch.equal(again["cost"], got["cost"]) and torch.equal(again["angle"], got["angle"])
        # frames t >= n, joints off the chain and the translation columns are never read
        poisoned, pq = torch.full_like(f32, float("nan")), torch.full_like(q32, float("nan"))
        for w, n in enumerate(lengths):
            poisoned[w, :, :n, cols] = f32[w, :, :n, cols]
            pq[w, :n] = q32[w, :n]
        nan = head_rot_cost_hip(poisoned.to(dev), layout, pq.to(dev), lengths)
        assert torch.equal(nan["cost"], got["cost"]) and torch.equal(nan["angle"], got["angle"])
    if T >= 5:                                                         # (two frames lie half their distance from their mean: often < 5)
        assert big * 2 > live, (big, live)                             # the element-wise form is what most frames are held to
    over, full = head_rot_cost_hip(fd, layout, qd, [T + 5] * W), head_rot_cost_hip(fd, layout, qd, [T] * W)
    assert torch.equal(over["cost"], full["cost"]) and torch.equal(over["angle"], full["angle"])           # a length above T is T


@pytest.mark.parametrize("F", (75, 144))
def test_head_rot_cost_finds_the_planted_hypothesis(dev, F):
    from seeme_amd.recording import head_rot_cost_hip, path_select_hip
    W, K, T = 6, 8, 32
    star = [(3 * w + 1) % K for w in range(W)]
    feats, dq = HR.planted_inputs(W, K, T, F, star)
    cost = head_rot_cost_hip(torch.from_numpy(feats).to(dev), HR.LAYOUT_OF_F[F], torch.from_numpy(dq).to(dev), [T] * W)["cost"]
    print(f"planted F {F}: cost of the planted hypotheses {cost[torch.arange(W), torch.tensor(star)].tolist()} degrees, smallest other "
          f"{float(cost.scatter(1, torch.tensor(star, device=dev)[:, None], float('inf')).min()):.1f} degrees")
    assert cost.argmin(dim=1).cpu().tolist() == star and float(cost[torch.arange(W), torch.tensor(star)].max()) < 2.0
    sel = path_select_hip(torch.zeros(W - 1, K, K, device=dev), unary=cost)
    assert sel["path"].cpu().tolist() == star


# ----------------------------------------------------------------------------- 2. bad arguments
def test_head_rot_cost_bad_arguments_raise(dev):
    from seeme_amd import _lib as L
    from seeme_amd import recording as R
    W, K, T, F = 2, 3, 8, 72
    feats, dq = torch.zeros(W, K, T, F, device=dev), torch.zeros(W, T, 4, device=dev)
    dq[..., 0] = 1.0
    len32 = torch.full((W,), T, dtype=torch.int32, device=dev)
    slot = lambda: {"cost": torch.zeros(W, K, device=dev), "angle": torch.zeros(W, K, T, device=dev)}
    with pytest.raises(L.SeemeError, match="K must be"):
        R.head_rot_cost_hip(torch.zeros(W, 33, T, F, device=dev), R.STITCH_ANGLE, dq, [T] * W)
    for a, b, c in ((None, dq, len32), (feats, None, len32), (feats, dq, None)):
        with pytest.raises(L.SeemeError, match="null"):
            R._launch_head_rot_cost(a, R.STITCH_ANGLE, F, b, c, W, K, T, out=slot())
    with pytest.raises(L.SeemeError, match="null"):
        R._launch_head_rot_cost(feats, R.STITCH_ANGLE, F, dq, len32, W, K, T, out={"cost": None, "angle": None})
    only = R._launch_head_rot_cost(feats, R.STITCH_ANGLE, F, dq, len32, W, K, T, out={"cost": torch.ones(W, K, device=dev), "angle": None})
    assert float(only["cost"].abs().max()) == 0.0                     # angle is optional: a null pointer there is "not wanted"
    for bad_w in (0, -1):
        with pytest.raises(L.SeemeError, match="W must be"):
            R._launch_head_rot_cost(feats, R.STITCH_ANGLE, F, dq, len32, bad_w, K, T, out=slot())
    for layout, width in ((R.STITCH_ROT6D, 72), (R.STITCH_ANGLE, 45), (R.STITCH_ANGLE_TRANSL, 48), (7, 72)):
        with pytest.raises(L.SeemeError, match=f"layout {layout} with F = {width}"):
            R._launch_head_rot_cost(feats, layout, width, dq, len32, W, K, T, out=slot())
        with pytest.raises(ValueError, match="layout"):
            R.head_rot_cost_hip(feats[..., :width], layout, dq, [T] * W)
    with pytest.raises(L.SeemeError):
        R.head_rot_cost_hip(feats.cpu(), R.STITCH_ANGLE, dq.cpu(), [T] * W)
    for args in ((feats[0], R.STITCH_ANGLE, dq, [T] * W), (feats, R.STITCH_ANGLE, dq[:, :-1], [T] * W), (feats, R.STITCH_ANGLE, dq[..., :3], [T] * W),
                 (feats, R.STITCH_ANGLE, dq, [T]), (feats, R.STITCH_ANGLE, dq, [T, 2.5]), (feats.double(), R.STITCH_ANGLE, dq.double(), [T] * W),
                 (feats, R.STITCH_ANGLE, dq.double(), [T] * W), (feats.long(), R.STITCH_ANGLE, dq, [T] * W)):
        with pytest.raises(ValueError):
            R.head_rot_cost_hip(*args)


# ----------------------------------------------------------------------------- 3. MLD.predict_recording
def _case_rotations(c):
    """The moving camera of test_gpu_headset.moving_case again: (world2cam [n,4,4], its rotations camera -> world [n,3,3])."""
    from seeme_amd.recording import camera_rotations
    w2c = _camera(c["n"], c["T"] - c["O"])
    return w2c, camera_rotations(w2c)


def test_predict_recording_with_the_rotation_terms_off_is_bit_identical(dev, scene_model, moving_case):
    model = scene_model[0]
    c = moving_case
    _, rot = _case_rotations(c)
    for kw in (dict(head_rot=rot), dict(head_rot=rot, head_rot_weight=0.0, head_rot_report=False, head_offset=[0.0, 0.0, 0.0]),
               dict(head_rot=torch.from_numpy(rot), head_path=c["head_path"], head_offset=np.zeros(3))):
        out = model.predict_recording(c["batch"], c["n"], **kw, **c["kw"])
        a, b = dict(_flat(c["plain"])), dict(_flat(out))
        assert set(a) == set(b) and not any(k.startswith("head_") for k in b)
        for k, v in a.items():
            assert torch.equal(v, b[k]) if isinstance(v, torch.Tensor) else v == b[k], k
    for kw, name in ((dict(head_rot_weight=1.0), "head_rot.*world2cam"), (dict(head_rot_report=True), "head_rot.*world2cam"),
                     (dict(head_offset=[0.0, 0.1, 0.0], head_path=c["head_path"], head_weight=1.0), "head_rot.*world2cam"),
                     (dict(head_rot_weight=-1.0, head_rot=rot), "head_rot_weight"), (dict(head_rot_weight=True, head_rot=rot), "head_rot_weight"),
                     (dict(head_rot_report=1, head_rot=rot), "head_rot_report"), (dict(head_offset=[0.0, 0.1], head_rot=rot), "head_offset"),
                     (dict(head_offset=[0.0, float("nan"), 0.0], head_rot=rot), "head_offset"),
                     (dict(head_rot_weight=1.0, head_rot=rot[:-1]), "head_rot"), (dict(head_rot_report=True, head_rot=1.01 * rot), "head_rot of frame 0"),
                     (dict(head_rot_weight=1.0, head_rot=np.zeros((c["n"], 3, 3), np.int64)), "head_rot")):
        with pytest.raises(ValueError, match=name):
            model.predict_recording(c["batch"], c["n"], **kw, **c["kw"])


def test_predict_recording_head_rot_weight_adds_the_rotation_term(dev, scene_model, moving_case):
    from seeme_amd import recording as R
    from test_gpu_scene_views import _to_world
    model = scene_model[0]
    c = moving_case
    _, rot = _case_rotations(c)
    W, K, O, hrw = c["W"], c["K"], c["O"], 3.0
    out = model.predict_recording(c["batch"], c["n"], head_rot=rot, head_rot_weight=hrw, **c["kw"])
    assert set(out) == set(c["plain"]) | {"head_rot_cost", "head_rot_cost_path"}
    pr, path = out["predict"], out["path"].cpu().tolist()
    assert torch.equal(pr["m_rst_all"], c["plain"]["predict"]["m_rst_all"])                                # the same hypotheses
    layout = R.stitch_layout(model.data_type, model.transl_in_feats)
    dq = R.head_rot_windows(rot, out["window_starts"], out["window_lengths"], c["T"], window_frames=c["kw"]["window_frames"])
    want = R.head_rot_cost_torch(pr["m_rst_all"].double().cpu(), layout, dq.double(), out["window_lengths"])["cost"]
    assert out["head_rot_cost"].shape == (W, K) and out["head_rot_cost"].dtype == torch.float32
    e = _elem_rel(out["head_rot_cost"], want)
    print(f"predict_recording: head_rot_cost {out['head_rot_cost'].tolist()} degrees, max element-wise relative error {e:.3e}")
    assert e <= TOL_F32
    assert torch.equal(out["head_rot_cost_path"], out["head_rot_cost"][torch.arange(W), out["path"]])
    world = torch.from_numpy(_to_world(pr["joints_rst_all"], c["Mw"]))                                      # float64, on the host
    cost = R.overlap_cost_torch(world, O)
    unary = model.path_medoid_weight * pr["hyp_metrics"]["PAIR_DIST"].double().cpu().sum(dim=2) / max(K - 1, 1) + hrw * want
    low = float(R.path_select_torch(cost, unary)["path_cost"])
    mine = REF.path_total(cost.numpy(), unary.numpy(), path)
    print(f"  path {path} (without the term {c['plain']['path'].tolist()}), float64 total {mine:.4f} vs the minimum {low:.4f}")
    assert mine - low <= TOL_F32 * low
    assert abs(float(out["path_cost"]) - mine) <= TOL_F32 * mine
    # the rotation term alone (no medoid term): the unary is the rotation term
    alone = model.predict_recording(c["batch"], c["n"], head_rot=rot, head_rot_weight=hrw, medoid_weight=0, **c["kw"])
    mine = REF.path_total(cost.numpy(), (hrw * want).numpy(), alone["path"].cpu().tolist())
    low = float(R.path_select_torch(cost, hrw * want)["path_cost"])
    assert mine - low <= TOL_F32 * low and torch.equal(alone["head_rot_cost"], out["head_rot_cost"])


def test_predict_recording_head_rot_report_is_the_twin_on_the_stitched_motion(dev, scene_model, moving_case):
    from seeme_amd import recording as R
    model = scene_model[0]
    c = moving_case
    n = c["n"]
    _, rot = _case_rotations(c)
    out = model.predict_recording(c["batch"], n, head_rot=rot, head_rot_report=True, **c["kw"])
    assert set(out) == set(c["plain"]) | {"head_rot_residual", "head_rot_mean"}
    assert torch.equal(out["motion"], c["plain"]["motion"]) and torch.equal(out["path"], c["plain"]["path"])
    assert out["head_rot_residual"].shape == (n,) and out["head_rot_mean"].shape == () and out["head_rot_residual"].dtype == torch.float32
    layout = R.stitch_layout(model.data_type, model.transl_in_feats)
    want = R.head_rot_cost_torch(out["motion"].double().cpu()[None, None], layout, R.head_rot_windows(rot, [0], [n], n).double(), [n])
    assert _elem_rel(out["head_rot_mean"], want["cost"][0, 0]) <= TOL_F32
    _hold_angle(out["head_rot_residual"][None, None], want["angle"], [n], f"head_rot_report (mean {float(out['head_rot_mean']):.2f} degrees)")
    # both at once, with the anchoring (which moves positions, not rotations): the same residual
    both = model.predict_recording(c["batch"], n, head_rot=rot, head_rot_report=True, head_rot_weight=0.5, head_path=c["head_path"],
                                   head_anchor=True, **c["kw"])
    assert set(both) == set(c["plain"]) | {"head_rot_residual", "head_rot_mean", "head_rot_cost", "head_rot_cost_path", "head_shift",
                                           "head_residual", "transl"}
    if torch.equal(both["path"], out["path"]):
        assert torch.equal(both["head_rot_residual"], out["head_rot_residual"])


def test_predict_recording_head_offset_moves_the_path_to_joint_15(dev, scene_model, moving_case):
    from seeme_amd import recording as R
    model = scene_model[0]
    c = moving_case
    _, rot = _case_rotations(c)
    offset = [0.08, 0.11, -0.02]
    moved = R.head_joint_path(c["head_path"], rot, offset)
    assert float(np.abs(np.linalg.norm(moved - c["head_path"], axis=1) - np.linalg.norm(offset)).max()) <= 1e-12
    got = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], head_rot=rot, head_offset=offset, head_weight=2.0,
                                  head_anchor=True, **c["kw"])
    want = model.predict_recording(c["batch"], c["n"], head_path=moved, head_weight=2.0, head_anchor=True, **c["kw"])
    near = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], head_weight=2.0, head_anchor=True, **c["kw"])
    assert set(got) == set(want)
    for k in ("head_cost", "head_cost_path", "head_shift", "head_residual", "joints", "motion", "transl", "path"):
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["head_shift"], near["head_shift"]) and not torch.equal(got["head_cost"], near["head_cost"])


def test_predict_recording_head_rot_weight_serves_features_without_a_translation(dev):
    from seeme_amd import recording as R
    from test_gpu_rot6d import _mld as _mld_rot6d
    n, T, O, K = 37, 16, 4, 3
    model, dm, cfg = _mld_rot6d(dev, "config_mld_egobody_rot6d.yaml", T=T, mutate=_mut)
    model.eval()
    assert not model.transl_in_feats and model.data_type == "rot6d" and model.path_head_rot_weight == 0.0 and model.head_rot_report is False
    assert not model.head_device_offset.any()
    starts, lengths = R.window_plan(n, T, O)
    batch = dm.batch(len(starts), idx=2, lengths=lengths)
    lat, cn = _draws(len(starts), K, model.do_classifier_free_guidance, dev, seed=3)
    kw = dict(overlap=O, num_hypotheses=K, latents=lat, cond_noise=cn)
    g = np.random.default_rng(2)
    rot = np.stack([HR.aa_matrix(v) for v in np.cumsum(0.05 * g.standard_normal((n, 3)), axis=0) + np.array([0.4, -1.0, 2.0])])
    with pytest.raises(ValueError, match="PATH_HEAD_WEIGHT"):         # the position term still has nothing to compare
        model.predict_recording(batch, n, head_path=np.zeros((n, 3)), head_weight=1.0, **kw)
    plain = model.predict_recording(batch, n, **kw)
    out = model.predict_recording(batch, n, head_rot=rot, head_rot_weight=1.0, head_rot_report=True, **kw)
    assert set(out) == set(plain) | {"head_rot_cost", "head_rot_cost_path", "head_rot_residual", "head_rot_mean"}
    m_all = out["predict"]["m_rst_all"]
    assert m_all.shape[-1] == 144
    want = R.head_rot_cost_torch(m_all.double().cpu(), R.STITCH_ROT6D, R.head_rot_windows(rot, starts, lengths, T).double(), lengths)["cost"]
    e = _elem_rel(out["head_rot_cost"], want)
    print(f"rot6d: head_rot_cost {out['head_rot_cost'].tolist()} degrees, max element-wise relative error {e:.3e}")
    assert e <= TOL_F32
    rep = R.head_rot_cost_torch(out["motion"].double().cpu()[None, None], R.STITCH_ROT6D, R.head_rot_windows(rot, [0], [n], n).double(), [n])
    assert _elem_rel(out["head_rot_mean"], rep["cost"][0, 0]) <= TOL_F32
    _hold_angle(out["head_rot_residual"][None, None], rep["angle"], [n], "rot6d head_rot_report")


def test_head_rot_config_keys_are_validated(dev):
    for key, bad in (("PATH_HEAD_ROT_WEIGHT", -1.0), ("PATH_HEAD_ROT_WEIGHT", "much"), ("PATH_HEAD_ROT_WEIGHT", True),
                     ("PATH_HEAD_ROT_WEIGHT", float("inf")), ("HEAD_ROT_REPORT", 1), ("HEAD_ROT_REPORT", "yes"), ("HEAD_DEVICE_OFFSET", 0.1),
                     ("HEAD_DEVICE_OFFSET", [0.0, 0.1]), ("HEAD_DEVICE_OFFSET", [0.0, "x", 0.0]), ("HEAD_DEVICE_OFFSET", [0.0, float("nan"), 0.0]),
                     ("HEAD_DEVICE_OFFSET", [True, 0.0, 0.0])):
        def mutate(cfg, key=key, bad=bad):
            cfg.TEST[key] = bad
        with pytest.raises(ValueError, match=key):
            _mld(dev, "config_mld_egobody.yaml", mutate=mutate)

    def good(cfg):
        cfg.TEST.PATH_HEAD_ROT_WEIGHT, cfg.TEST.HEAD_ROT_REPORT, cfg.TEST.HEAD_DEVICE_OFFSET = 2, True, [0.08, 0.11, -0.02]
    model = _mld(dev, "config_mld_egobody.yaml", mutate=good)[0]
    assert model.path_head_rot_weight == 2 and model.head_rot_report is True and model.head_device_offset.tolist() == [0.08, 0.11, -0.02]


# ----------------------------------------------------------------------------- 4. cli.predict_main
def test_cli_predict_main_follows_the_headsets_orientation(dev, tmp_path, scene_model):
    from conftest import REPO, load_golden
    from seeme_amd import cli
    from seeme_amd import recording as R
    model, dm, cfg = scene_model
    ckpt = os.path.join(tmp_path, "model.ckpt")
    cli.save_checkpoint(ckpt, model, 0, 0)
    n = 37
    rec = _synthetic_recording(n, seed=3)
    w2c = _camera(n, 12)
    rec_path, out_path = os.path.join(tmp_path, "rec.npz"), os.path.join(tmp_path, "out", "motion.npz")
    np.savez(rec_path, **rec, world2cam=w2c)
    argv = ["--cfg", os.path.join(REPO, "configs", "config_mld_scene.yaml"), "--checkpoint", ckpt, "--folder", str(tmp_path), "--frames", "16",
            "--scene_points", "384", "--input", rec_path, "--output", out_path, "--num_hypotheses", "3", "--overlap", "4", "--seed", "11"]

    def run(extra):
        r = cli.predict_main(argv + extra)
        with np.load(out_path, allow_pickle=False) as z:
            return r, {k: z[k] for k in z.files}

    def residual_of(res, rot):
        """The twin on the written motion (the chain's rotations are global_orient and body_pose) against the rotations `rot`."""
        feats = torch.from_numpy(np.concatenate([res["global_orient"], res["body_pose"]], axis=1)).double()[None, None]
        return R.head_rot_cost_torch(feats, R.STITCH_ANGLE, R.head_rot_windows(rot, [0], [n], n).double(), [n])

    # without the options: the keys and the bytes of the commit before the headset options (tests/golden/headset_cli_parent.npz)
    _, plain = run([])
    parent = load_golden("headset_cli_parent.npz")
    assert set(plain) == set(parent) == PARENT_KEYS
    for k, v in parent.items():
        assert plain[k].dtype == v.dtype and plain[k].shape == v.shape and plain[k].tobytes() == v.tobytes(), k
    _, zero = run(["--head_rot_weight", "0", "--head_offset", "0", "0", "0"])                  # a weight of 0 and no lever arm: the same bytes
    assert set(zero) == PARENT_KEYS and all(np.array_equal(zero[k], plain[k]) and zero[k].dtype == plain[k].dtype for k in plain)
    r, res = run(["--head_rot_weight", "1", "--head_rot_report"])
    assert set(res) == PARENT_KEYS | {"head_rot_cost", "head_rot_residual", "head_rot_mean"} and r["windows"] == 3
    assert res["head_rot_cost"].shape == (3, 3) and res["head_rot_residual"].shape == (n,) and res["head_rot_mean"].shape == ()
    assert all(np.isfinite(v).all() for v in res.values())
    want = residual_of(res, R.camera_rotations(w2c))
    _hold_angle(torch.from_numpy(res["head_rot_residual"])[None, None], want["angle"], [n], "cli head_rot_residual")
    assert _elem_rel(res["head_rot_mean"], want["cost"][0, 0].numpy()) <= TOL_F32
    # the recording's own head_rot goes before the rotations of world2cam
    g = np.random.default_rng(12)
    own = R.camera_rotations(w2c) @ np.stack([HR.aa_matrix(v) for v in np.cumsum(0.1 * g.standard_normal((n, 3)), axis=0)])
    np.savez(rec_path, **rec, world2cam=w2c, head_rot=own)
    _, up = run(["--head_rot_report"])
    assert set(up) == PARENT_KEYS | {"head_rot_residual", "head_rot_mean"}
    assert all(np.array_equal(up[k], plain[k]) for k in PARENT_KEYS)                            # a report chooses nothing
    _hold_angle(torch.from_numpy(up["head_rot_residual"])[None, None], residual_of(up, own)["angle"], [n], "cli, the recording's own head_rot")
    assert float(np.abs(up["head_rot_residual"] - residual_of(up, R.camera_rotations(w2c))["angle"][0, 0].numpy()).max()) > 1.0
    # the lever arm: head_path moves by the offset turned with the device before the anchoring
    _, arm = run(["--anchor_headset", "--anchor_sigma", "0", "--head_offset", "0.08", "0.11", "-0.02"])
    assert set(arm) == PARENT_KEYS | {"head_shift", "head_residual"}
    joint = R.head_joint_path(R.camera_centres(w2c), own, [0.08, 0.11, -0.02])
    assert float(np.abs(arm["joints"][:, 15].astype(np.float64) - joint).max()) <= 1e-5
    # neither key: the error says which would provide the orientation
    np.savez(rec_path, **rec)
    for extra in (["--head_rot_weight", "1"], ["--head_rot_report"], ["--head_offset", "0", "0.1", "0"]):
        with pytest.raises(ValueError, match="head_rot.*world2cam"):
            run(extra)
