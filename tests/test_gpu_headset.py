"""The headset's own path on the device: seeme_head_path_cost and seeme_head_anchor against their float64 twins on the fp32 inputs the
kernels saw, the planted choice through seeme_path_select, bad arguments, and the new options of MLD.predict_recording and
cli.predict_main (head_path, head_weight, head_anchor, anchor_sigma).

Bounds: TOL_F32 and _elem_rel of tests/test_gpu_hyp_select.py.  The cost inputs (headset_reference.cost_inputs) keep the deviations
|r_t - o| at the order of 100 mm against coordinates of metres: the cancellation in r_t - o costs about 1e-7 m absolute, 1e-6 of the
value.  The anchor inputs make r a random walk with 30 mm steps; a residual is held element-wise to TOL_F32 where it is at least
10 mm, and to the absolute bound of a 10 mm residual (TOL_F32 x 10 mm) where the walk leaves it smaller (sigma = 0.5 weighs the
neighbours by 0.135: most of its residuals are a few mm), so no element goes unchecked."""
import os

import numpy as np
import pytest
import torch

import headset_reference as HREF
import recording_reference as REF
import scene_views_reference as SV
from test_gpu_hyp_select import TOL_F32, _draws, _elem_rel, _mld
from test_gpu_recording import _mut, _synthetic_recording

pytestmark = pytest.mark.gpu

COST_CASES = [(1, 1, 1), (2, 3, 2), (3, 32, 5), (2, 5, 63), (2, 5, 64), (2, 5, 65), (3, 4, 196)]
ANCHOR_LENGTHS = (1, 2, 7, 64, 65, 300)
ANCHOR_SIGMAS = (0, 0.5, 2, 10)
RESIDUAL_FLOOR_MM = 10.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- 1. the cost kernel
@pytest.mark.parametrize("shape", COST_CASES, ids=str)
def test_head_path_cost_kernel_vs_float64_twin(dev, shape):
    from seeme_amd.recording import head_path_cost_hip, head_path_cost_torch
    W, K, T = shape
    j32, p32 = (torch.from_numpy(a) for a in HREF.cost_inputs(W, K, T))
    jd, pd = j32.to(dev), p32.to(dev)
    for lengths in HREF.cost_lengths(W, T):
        want = head_path_cost_torch(j32.double(), p32.double(), lengths)         # float64 on the fp32 inputs the kernel sees
        got = head_path_cost_hip(jd, pd, lengths)
        torch.cuda.synchronize()
        assert got.shape == (W, K) and got.dtype == torch.float32
        e = _elem_rel(got, want)
        print(f"head_path_cost {shape} lengths {lengths}: max element-wise relative error {e:.3e}, values {float(want.min()):.1f} .. "
              f"{float(want.max()):.1f} mm")
        assert e <= TOL_F32, e
        for w, n in enumerate(lengths):
            if n <= 1:
                assert float(got[w].abs().max()) == 0.0
        assert torch.equal(head_path_cost_hip(jd, pd, lengths), got)             # bitwise reproducible
        # frames t >= n and joints other than 15 are never read
        poisoned = j32.clone()
        keep = torch.zeros(W, K, T, 24, dtype=torch.bool)
        pp = torch.full_like(p32, float("nan"))
        for w, n in enumerate(lengths):
            keep[w, :, :n, HREF.HEAD] = True
            pp[w, :n] = p32[w, :n]
        poisoned[~keep] = float("nan")
        assert torch.equal(head_path_cost_hip(poisoned.to(dev), pp.to(dev), lengths), got)
    assert torch.equal(head_path_cost_hip(jd, pd, [T + 5] * W), head_path_cost_hip(jd, pd, [T] * W))       # a length above T is T


def test_head_path_cost_finds_the_planted_hypothesis(dev):
    from seeme_amd.recording import head_path_cost_hip, path_select_hip
    W, K, T = 6, 8, 32
    jts, path = HREF.cost_inputs(W, K, T, seed=1)
    g = np.random.default_rng(8)
    star = [(3 * w + 1) % K for w in range(W)]
    for w, k in enumerate(star):                                       # the path plus a constant, plus 1 mm of noise
        jts[w, k, :, HREF.HEAD] = path[w] + g.uniform(-0.3, 0.3, 3).astype(np.float32) + (0.001 * g.standard_normal((T, 3))).astype(np.float32)
    cost = head_path_cost_hip(torch.from_numpy(jts).to(dev), torch.from_numpy(path).to(dev), [T] * W)
    print(f"planted: cost of the planted hypotheses {cost[torch.arange(W), torch.tensor(star)].tolist()} mm, smallest other "
          f"{float(cost.scatter(1, torch.tensor(star, device=dev)[:, None], float('inf')).min()):.1f} mm")
    assert cost.argmin(dim=1).cpu().tolist() == star
    sel = path_select_hip(torch.zeros(W - 1, K, K, device=dev), unary=cost)
    assert sel["path"].cpu().tolist() == star


# ----------------------------------------------------------------------------- 2. the anchor kernel
@pytest.mark.parametrize("L_", ANCHOR_LENGTHS)
def test_head_anchor_kernel_vs_float64_twin(dev, L_):
    from seeme_amd.recording import head_anchor_hip, head_anchor_torch
    from seeme_amd.track import gaussian_taps
    j32, p32 = (torch.from_numpy(a) for a in HREF.anchor_inputs(L_))
    jd, pd = j32.to(dev), p32.to(dev)
    for sigma in ANCHOR_SIGMAS:
        taps = gaussian_taps(sigma)
        assert taps.shape[0] - 1 == int(np.ceil(3 * sigma))           # sigma 10: R = 30, longer than the recording at L = 7
        want_s, want_r = head_anchor_torch(j32.double(), p32.double(), taps)     # float64 on the fp32 inputs the kernel sees
        shift, residual = head_anchor_hip(jd, pd, taps)
        torch.cuda.synchronize()
        assert shift.shape == (L_, 3) and residual.shape == (L_,) and shift.dtype == residual.dtype == torch.float32
        assert torch.isfinite(shift).all() and torch.isfinite(residual).all()
        es = float((shift.double().cpu() - want_s).abs().max())
        bound = TOL_F32 * float(want_s.abs().max())
        er = (residual.double().cpu() - want_r).abs()
        big = want_r >= RESIDUAL_FLOOR_MM
        rel = float((er[big] / want_r[big]).max()) if big.any() else 0.0
        small = float(er[~big].max()) if (~big).any() else 0.0
        print(f"head_anchor L {L_} sigma {sigma}: shift max-norm error {es:.3e} (bound {bound:.3e}); residual: {int(big.sum())} of {L_} "
              f">= {RESIDUAL_FLOOR_MM:g} mm, element-wise relative error {rel:.3e}; below it absolute error {small:.3e} mm")
        assert es <= bound
        assert rel <= TOL_F32 and small <= TOL_F32 * RESIDUAL_FLOOR_MM
        if sigma == 0 or L_ == 1:
            assert torch.equal(shift, pd - jd[:, HREF.HEAD]) and float(residual.abs().max()) == 0.0
        elif sigma >= 2 and L_ >= 64:
            assert int(big.sum()) * 2 > L_                             # the element-wise form is what most frames are held to
        again = head_anchor_hip(jd, pd, taps)                          # bitwise reproducible
        assert torch.equal(again[0], shift) and torch.equal(again[1], residual)
        # joints other than 15 are never read
        poisoned = torch.full_like(j32, float("nan"))
        poisoned[:, HREF.HEAD] = j32[:, HREF.HEAD]
        nan = head_anchor_hip(poisoned.to(dev), pd, taps)
        assert torch.equal(nan[0], shift) and torch.equal(nan[1], residual)


# ----------------------------------------------------------------------------- 3. bad arguments
def test_headset_kernels_bad_arguments_raise(dev):
    from seeme_amd import _lib as L
    from seeme_amd import recording as R
    from seeme_amd.track import gaussian_taps
    W, K, T = 2, 3, 8
    jts, path = torch.zeros(W, K, T, 24, 3, device=dev), torch.zeros(W, T, 3, device=dev)
    len32 = torch.full((W,), T, dtype=torch.int32, device=dev)
    with pytest.raises(L.SeemeError, match="K must be"):
        R.head_path_cost_hip(torch.zeros(W, 33, T, 24, 3, device=dev), path, [T] * W)
    for a, b, c in ((None, path, len32), (jts, None, len32), (jts, path, None)):
        with pytest.raises(L.SeemeError, match="null"):
            R._launch_head_cost(a, b, c, W, K, T, out=torch.zeros(W, K, device=dev))
    for bad_w in (0, -1):
        with pytest.raises(L.SeemeError, match="W must be"):
            R._launch_head_cost(jts, path, len32, bad_w, K, T, out=torch.zeros(W, K, device=dev))
    with pytest.raises(L.SeemeError):
        R.head_path_cost_hip(jts.cpu(), path.cpu(), [T] * W)
    for args in ((jts[..., :2], path, [T] * W), (jts, path[:, :-1], [T] * W), (jts, path, [T]), (jts, path, [T, 2.5]),
                 (jts.double(), path.double(), [T] * W), (jts, path.double(), [T] * W), (jts.long(), path, [T] * W)):
        with pytest.raises(ValueError):
            R.head_path_cost_hip(*args)
    n = 12
    joints, hp = torch.zeros(n, 24, 3, device=dev), torch.zeros(n, 3, device=dev)
    one = np.ones(1, np.float32)
    with pytest.raises(L.SeemeError, match="R must be"):
        R.head_anchor_hip(joints, hp, np.ones(32, np.float32))       # R = 31
    assert R.head_anchor_hip(joints, hp, np.ones(31, np.float32))[0].shape == (n, 3)                       # R = 30 is served
    for a, b, t in ((None, hp, one), (joints, None, one), (joints, hp, None)):
        with pytest.raises(L.SeemeError, match="null"):
            R._launch_head_anchor(a, b, n, t, 0)
    for bad_n in (0, -3):
        with pytest.raises(L.SeemeError, match="L must be"):
            R._launch_head_anchor(joints, hp, bad_n, one, 0, out=(torch.zeros(n, 3, device=dev), torch.zeros(n, device=dev)))
    for taps in ([0.0, 1.0], [1.0, -0.5], [1.0, float("nan")]):
        with pytest.raises(L.SeemeError, match="tap"):
            R.head_anchor_hip(joints, hp, taps)
    with pytest.raises(L.SeemeError):
        R.head_anchor_hip(joints.cpu(), hp.cpu(), one)
    for args in ((joints[:, :23], hp, one), (joints, hp[:-1], one), (joints.double(), hp.double(), one), (joints, hp.double(), one),
                 (joints, hp, np.ones((2, 2), np.float32)), (joints, hp, np.zeros(0, np.float32))):
        with pytest.raises(ValueError):
            R.head_anchor_hip(*args)
    assert gaussian_taps(10.0).shape[0] == R.HEAD_ANCHOR_RMAX + 1


# ----------------------------------------------------------------------------- 4. MLD.predict_recording
@pytest.fixture(scope="module")
def scene_model(dev):
    return _mld(dev, "config_mld_scene.yaml", mutate=_mut)


def _camera(n, S):
    """A camera that yaws 30 degrees and moves half a metre from one window to the next: world2cam [n,4,4] float64."""
    return np.stack([SV.rigid([0.1, np.radians(30.0) * f / S, -0.2], [0.5 * f / S, -0.3, 1.0 + 0.2 * f / S]) for f in range(n)])


@pytest.fixture(scope="module")
def moving_case(dev, scene_model):
    """A moving-camera batch with 3 windows, K = 4 and fixed latents; the call without head_path, made once."""
    from seeme_amd import recording as R
    model, dm, cfg = scene_model
    n, T, O, K = 37, 16, 4, 4
    rec = _synthetic_recording(n, seed=1)
    rec["n_frames"] = n
    w2c = _camera(n, T - O)
    pelvis = R.rest_pelvis(model.smpl_model, torch.from_numpy(rec["betas"]).to(dev)[None])[0]
    batch, starts, lengths, frames = R.windows_batch(rec, dm, T, O, tuple(cfg.model.condition), dataset="egobody", device=dev,
                                                     world2cam=w2c, pelvis=pelvis)
    assert lengths == [16, 16, 13]
    lat, cn = _draws(len(starts), K, model.do_classifier_free_guidance, dev, seed=6)
    kw = dict(overlap=O, betas=torch.from_numpy(rec["wearer_betas"]).to(dev), num_hypotheses=K, latents=lat, cond_noise=cn,
              window_frames=frames["world2cam"].float())
    assert model.transl_in_feats
    return {"n": n, "T": T, "O": O, "K": K, "W": len(starts), "batch": batch, "kw": kw, "Mw": frames["world2cam"].numpy(),
            "head_path": R.camera_centres(w2c), "plain": model.predict_recording(batch, n, **kw)}


def _flat(out, prefix=""):
    for k, v in out.items():
        if isinstance(v, dict):
            yield from _flat(v, prefix + k + ".")
        else:
            yield prefix + k, v


def test_predict_recording_with_the_head_terms_off_is_bit_identical(dev, scene_model, moving_case):
    model = scene_model[0]
    c = moving_case
    out = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], **c["kw"])
    a, b = dict(_flat(c["plain"])), dict(_flat(out))
    assert set(a) == set(b) and "head_cost" not in b and "head_shift" not in b and "transl" not in b
    for k, v in a.items():
        assert torch.equal(v, b[k]) if isinstance(v, torch.Tensor) else v == b[k], k
    off = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], head_weight=0.0, head_anchor=False, **c["kw"])
    assert set(off) == set(c["plain"]) and torch.equal(off["motion"], c["plain"]["motion"])
    for kw, name in ((dict(head_weight=1.0), "head_path"), (dict(head_anchor=True), "head_path"),
                     (dict(head_weight=-1.0, head_path=c["head_path"]), "head_weight"),
                     (dict(head_anchor=1, head_path=c["head_path"]), "head_anchor"),
                     (dict(head_anchor=True, anchor_sigma=11.0, head_path=c["head_path"]), "anchor_sigma"),
                     (dict(head_weight=1.0, head_path=c["head_path"][:-1]), "head_path"),
                     (dict(head_weight=1.0, head_path=np.zeros((c["n"], 3), np.int64)), "head_path")):
        with pytest.raises(ValueError, match=name):
            model.predict_recording(c["batch"], c["n"], **kw, **c["kw"])


def test_predict_recording_head_weight_adds_the_head_path_term(dev, scene_model, moving_case):
    from seeme_amd import recording as R
    from test_gpu_scene_views import _to_world
    model = scene_model[0]
    c = moving_case
    W, K, O, hw = c["W"], c["K"], c["O"], 2.0
    out = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], head_weight=hw, **c["kw"])
    assert set(out) == set(c["plain"]) | {"head_cost", "head_cost_path"}
    pr, path = out["predict"], out["path"].cpu().tolist()
    assert torch.equal(pr["joints_rst_all"], c["plain"]["predict"]["joints_rst_all"])                      # the same hypotheses
    world = torch.from_numpy(_to_world(pr["joints_rst_all"], c["Mw"]))                                      # float64, on the host
    hp32 = torch.from_numpy(c["head_path"]).float().double()                                               # the path the kernel saw
    want = R.head_path_cost_torch(world, R.head_path_windows(hp32, out["window_starts"], out["window_lengths"], c["T"]),
                                  out["window_lengths"])
    assert out["head_cost"].shape == (W, K) and out["head_cost"].dtype == torch.float32
    e = _elem_rel(out["head_cost"], want)
    print(f"predict_recording: head_cost {out['head_cost'].tolist()} mm, max element-wise relative error {e:.3e}")
    assert e <= TOL_F32
    assert torch.equal(out["head_cost_path"], out["head_cost"][torch.arange(W), out["path"]])
    cost = R.overlap_cost_torch(world, O)
    unary = model.path_medoid_weight * pr["hyp_metrics"]["PAIR_DIST"].double().cpu().sum(dim=2) / max(K - 1, 1) + hw * want
    low = float(R.path_select_torch(cost, unary)["path_cost"])
    mine = REF.path_total(cost.numpy(), unary.numpy(), path)
    print(f"  path {path} (without the term {c['plain']['path'].tolist()}), float64 total {mine:.4f} vs the minimum {low:.4f}")
    assert mine - low <= TOL_F32 * low
    assert abs(float(out["path_cost"]) - mine) <= TOL_F32 * mine
    # the head term alone (no medoid term): the unary is the head term
    alone = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], head_weight=hw, medoid_weight=0, **c["kw"])
    mine = REF.path_total(cost.numpy(), (hw * want).numpy(), alone["path"].cpu().tolist())
    low = float(R.path_select_torch(cost, hw * want)["path_cost"])
    assert mine - low <= TOL_F32 * low and torch.equal(alone["head_cost"], out["head_cost"])


def test_predict_recording_head_weight_on_a_single_short_window(dev, scene_model):
    """A lone window shorter than T comes back from predict cut to its length: the path is cut the same way, and with the head term
    alone the chosen hypothesis is the one whose head follows the path best."""
    from seeme_amd import recording as R
    model, dm, cfg = scene_model
    n, T, O, K = 13, 16, 4, 4
    rec = _synthetic_recording(n, seed=2)
    rec["n_frames"] = n
    batch, starts, lengths = R.windows_batch(rec, dm, T, O, tuple(cfg.model.condition), dataset="egobody", device=dev)
    assert lengths == [13]
    lat, cn = _draws(1, K, model.do_classifier_free_guidance, dev, seed=6)
    head_path = np.cumsum(0.02 * np.random.default_rng(9).standard_normal((n, 3)), axis=0)
    out = model.predict_recording(batch, n, overlap=O, medoid_weight=0, num_hypotheses=K, latents=lat, cond_noise=cn,
                                  head_path=head_path, head_weight=1.0)
    jts = out["predict"]["joints_rst_all"]
    assert jts.shape[:3] == (1, K, n)
    want = R.head_path_cost_torch(jts.double().cpu(), torch.from_numpy(head_path).float().double()[None], [n])
    assert _elem_rel(out["head_cost"], want) <= TOL_F32
    k = int(out["path"][0])
    assert float(want[0, k]) - float(want.min()) <= TOL_F32 * float(want.min()), (k, want)
    assert abs(float(out["path_cost"]) - float(want[0, k])) <= TOL_F32 * float(want[0, k])
    assert torch.equal(out["motion"], out["predict"]["m_rst_all"][0, k, :n])


def test_predict_recording_head_anchor_moves_joints_and_translation(dev, scene_model, moving_case):
    model = scene_model[0]
    c = moving_case
    plain = c["plain"]
    hp = torch.from_numpy(c["head_path"]).float().to(dev)
    new = {"head_shift", "head_residual", "transl"}
    exact = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], head_anchor=True, anchor_sigma=0, **c["kw"])
    assert set(exact) == set(plain) | new and torch.equal(exact["path"], plain["path"])
    e = float((exact["joints"][:, 15] - hp).abs().max())
    print(f"head_anchor sigma 0: the head is {e:.3e} m from the path; residual max {float(exact['head_residual'].max()):.3e} mm")
    assert e <= 1e-5 and float(exact["head_residual"].abs().max()) == 0.0
    out = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], head_anchor=True, anchor_sigma=2, **c["kw"])
    assert set(out) == set(plain) | new
    shift = out["head_shift"]
    assert shift.shape == (c["n"], 3) and out["head_residual"].shape == (c["n"],) and float(out["head_residual"].min()) >= 0.0
    assert torch.equal(out["joints"], plain["joints"] + shift[:, None])
    assert torch.equal(out["motion"][:, :-3], plain["motion"][:, :-3])                                      # a translation model:
    assert torch.equal(out["motion"][:, -3:], plain["motion"][:, -3:] + shift)                              # the last three columns
    assert torch.equal(out["transl"], out["motion"][:, -3:])
    left = (hp - out["joints"][:, 15]).norm(dim=1) * 1000.0           # what the smoothing leaves between the path and the moved head
    assert float((left - out["head_residual"]).abs().max()) <= 1e-2   # (1e-5 m)
    # TEST.HEAD_ANCHOR_SIGMA is the default of anchor_sigma
    assert model.head_anchor_sigma == 2.0
    dflt = model.predict_recording(c["batch"], c["n"], head_path=c["head_path"], head_anchor=True, **c["kw"])
    assert torch.equal(dflt["head_shift"], shift) and torch.equal(dflt["joints"], out["joints"])


def test_predict_recording_on_features_without_a_translation(dev):
    from seeme_amd import recording as R
    from test_gpu_rot6d import _mld as _mld_rot6d
    n, T, O, K = 37, 16, 4, 3
    model, dm, cfg = _mld_rot6d(dev, "config_mld_egobody_rot6d.yaml", T=T, mutate=_mut)
    model.eval()
    assert not model.transl_in_feats and model.path_head_weight == 0.0 and model.head_anchor is False
    starts, lengths = R.window_plan(n, T, O)
    batch = dm.batch(len(starts), idx=2, lengths=lengths)
    lat, cn = _draws(len(starts), K, model.do_classifier_free_guidance, dev, seed=3)
    kw = dict(overlap=O, num_hypotheses=K, latents=lat, cond_noise=cn)
    g = np.random.default_rng(2)
    head_path = np.cumsum(0.02 * g.standard_normal((n, 3)), axis=0) + np.array([1.0, -2.0, 0.5])
    with pytest.raises(ValueError, match="PATH_HEAD_WEIGHT"):
        model.predict_recording(batch, n, head_path=head_path, head_weight=1.0, **kw)
    plain = model.predict_recording(batch, n, **kw)
    out = model.predict_recording(batch, n, head_path=head_path, head_anchor=True, **kw)
    assert set(out) == set(plain) | {"head_shift", "head_residual", "transl"}
    assert torch.equal(out["transl"], out["head_shift"]) and torch.equal(out["motion"], plain["motion"])
    assert torch.equal(out["joints"], plain["joints"] + out["head_shift"][:, None])
    hp = torch.from_numpy(head_path).float().to(dev)
    assert float(((hp - out["joints"][:, 15]).norm(dim=1) * 1000.0 - out["head_residual"]).abs().max()) <= 1e-2


def test_headset_config_keys_are_validated(dev):
    for key, bad in (("PATH_HEAD_WEIGHT", -1.0), ("PATH_HEAD_WEIGHT", "much"), ("PATH_HEAD_WEIGHT", True), ("HEAD_ANCHOR", 1),
                     ("HEAD_ANCHOR", "yes"), ("HEAD_ANCHOR_SIGMA", 10.5), ("HEAD_ANCHOR_SIGMA", -1), ("HEAD_ANCHOR_SIGMA", "wide")):
        def mutate(cfg, key=key, bad=bad):
            cfg.TEST[key] = bad
        with pytest.raises(ValueError, match=key):
            _mld(dev, "config_mld_egobody.yaml", mutate=mutate)


# ----------------------------------------------------------------------------- 5. cli.predict_main
PARENT_KEYS = {"global_orient", "body_pose", "transl", "joints", "window_starts", "path", "seam_cost", "world2cam_windows"}


def test_cli_predict_main_follows_the_headset(dev, tmp_path, scene_model):
    from conftest import REPO, load_golden
    from seeme_amd import cli
    from seeme_amd.recording import camera_centres
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

    # without the options: the keys and the bytes of the commit before the headset options (tests/golden/headset_cli_parent.npz is
    # what that commit's predict.py wrote for this command on the MI355X)
    _, plain = run([])
    parent = load_golden("headset_cli_parent.npz")
    assert set(plain) == set(parent) == PARENT_KEYS
    for k, v in parent.items():
        assert plain[k].dtype == v.dtype and plain[k].shape == v.shape and plain[k].tobytes() == v.tobytes(), k
    _, zero = run(["--head_weight", "0", "--anchor_sigma", "3"])       # a weight of 0 and an unused width: the same bytes
    assert set(zero) == PARENT_KEYS and all(np.array_equal(zero[k], plain[k]) and zero[k].dtype == plain[k].dtype for k in plain)
    r, res = run(["--head_weight", "1", "--anchor_headset"])
    assert set(res) == PARENT_KEYS | {"head_cost", "head_shift", "head_residual"} and r["windows"] == 3
    assert res["head_cost"].shape == (3, 3) and res["head_shift"].shape == (n, 3) and res["head_residual"].shape == (n,)
    assert all(np.isfinite(v).all() for v in res.values())
    head = res["transl"] + (res["joints"][:, 15] - res["transl"])
    left = np.linalg.norm(head.astype(np.float64) - camera_centres(w2c), axis=1)
    print(f"cli: head to camera centre {left.max():.4f} m at most, head_residual {res['head_residual'].max():.2f} mm at most")
    assert float(np.abs(left - res["head_residual"] / 1000.0).max()) <= 1e-4
    # the recording's own head_path goes before the centres of world2cam
    own = camera_centres(w2c) + np.array([0.0, 0.0, 1.0])
    np.savez(rec_path, **rec, world2cam=w2c, head_path=own)
    _, up = run(["--anchor_headset", "--anchor_sigma", "1"])
    assert set(up) == PARENT_KEYS | {"head_shift", "head_residual"}
    left = np.linalg.norm(up["joints"][:, 15].astype(np.float64) - own, axis=1)
    assert float(np.abs(left - up["head_residual"] / 1000.0).max()) <= 1e-4      # (against the centres it would be off by the metre)
    # neither key: the error says which would provide the path
    np.savez(rec_path, **rec)
    with pytest.raises(ValueError, match="head_path.*world2cam"):
        run(["--anchor_headset"])
