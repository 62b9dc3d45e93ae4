"""The body-scene term on the device: seeme_scene_depth against the float64 loops of tests/scene_depth_reference.py on the fp32 inputs
the kernel saw, its bitwise independence of the points' order, of appended points out of reach, of K and of the layout of the
frames, bad arguments, and the new options of MLD.predict_recording and cli.predict_main (scene_cloud, scene_weight, scene_report,
capsules).

Bound of the kernel: depth and cost within 5e-3 mm absolute of the reference.  A pair takes about a dozen fp32 operations on
differences below 1 m, about 1e-6 m = 1e-3 mm; the bound is five times that.  Measured worst over KERNEL_CASES on one MI355X:
depth 4.8e-5 mm, cost 8.3e-6 mm.
hits must be equal: a condition on the inputs, asserted on the reference (no frame's max(radius - dist) within +-0.02 mm of 0).

End to end the joints the kernel sees are the hypotheses' joints re-framed on the device in fp32, and the reference re-frames them in
float64 on the host: up to 1e-5 m = 1e-2 mm of difference in a joint at these coordinates (a few ulp of 4 m per coordinate), to
which depth is 1-Lipschitz.  E2E_TOL_MM is the kernel's bound plus that."""
import os

import numpy as np
import pytest
import torch

import recording_reference as REF
import scene_depth_reference as SREF
from test_gpu_headset import PARENT_KEYS, _camera, _flat
from test_gpu_hyp_select import TOL_F32, _draws, _mld
from test_gpu_recording import _mut, _synthetic_recording

pytestmark = pytest.mark.gpu

TOL_MM = 5e-3
E2E_TOL_MM = TOL_MM + 1e-2
CHUNK = 32                   # SEEME_SCENE_DEPTH_CHUNK
# (W, K, T, J, N, NB, kind): N in {1, 63, 64, 65, 257, 5000}; T in {1, 2, 60, 196}, CHUNK - 1, CHUNK, CHUNK + 1, and 1000 with
# W = K = 1; K in {1, 3, 32}; W in {1, 2, 5} (a short last window from W = 2, a length of 0 from W = 3); NB in {1, 21, 32}
KERNEL_CASES = [(1, 1, 1, 24, 1, 1, "mixed"), (2, 3, 2, 24, 63, 21, "mixed"), (1, 2, 9, 5, 64, 3, "mixed"),
                (1, 3, CHUNK - 1, 24, 64, 21, "mixed"), (2, 1, CHUNK, 24, 65, 32, "mixed"), (1, 3, CHUNK + 1, 24, 257, 21, "mixed"),
                (5, 1, 60, 24, 5000, 21, "mixed"), (2, 32, 5, 24, 257, 1, "mixed"), (1, 1, 196, 24, 5000, 21, "mixed"),
                (1, 1, 1000, 24, 257, 21, "mixed"), (1, 2, 40, 24, 5000, 21, "dense"), (2, 3, CHUNK + 1, 24, 257, 21, "far")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a))


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("depth", "cost", "hits"))


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_scene_depth_kernel_vs_float64_reference(dev, case):
    from seeme_amd.recording import SCENE_DEPTH_CHUNK, scene_depth_hip
    assert SCENE_DEPTH_CHUNK == CHUNK
    W, K, T, J, N, NB, kind = case
    jts, lengths, points, segs, radius = SREF.inputs(*case)
    want = SREF.reference(*case)
    assert SREF.near_zero(want["raw"]) == 0                            # hits are decided far from rounding
    jd, pd = _t(jts).to(dev), _t(points).to(dev)
    got = scene_depth_hip(jd, list(lengths), pd, segs, radius)
    torch.cuda.synchronize()
    assert got["depth"].shape == (W, K, T) and got["cost"].shape == got["hits"].shape == (W, K)
    assert got["depth"].dtype == got["cost"].dtype == torch.float32 and got["hits"].dtype == torch.int32
    ed = float(np.abs(got["depth"].double().cpu().numpy() - want["depth"]).max())
    ec = float(np.abs(got["cost"].double().cpu().numpy() - want["cost"]).max())
    print(f"scene_depth {case}: depth error {ed:.3e} mm, cost error {ec:.3e} mm (bound {TOL_MM:g}); depth up to "
          f"{want['depth'].max():.2f} mm, {int(want['hits'].sum())} of {int(sum(lengths)) * K} frames penetrate")
    assert ed <= TOL_MM and ec <= TOL_MM
    assert np.array_equal(got["hits"].cpu().numpy(), want["hits"])
    for w, n in enumerate(lengths):
        assert float(got["depth"][w, :, n:].abs().max() if n < T else 0.0) == 0.0
    if kind == "far":
        assert float(got["depth"].abs().max()) == 0.0 and float(got["cost"].abs().max()) == 0.0 and int(got["hits"].abs().max()) == 0
    elif N >= 63:
        assert want["hits"].sum() > 0
    if kind == "dense":                                                # every point inside the box of every frame's joints: none is
        named = np.unique(segs)                                        # culled, and the queue of 512 wraps several times
        lo, hi = jts[:, :, :, named].min(axis=3).max(axis=(0, 1, 2)), jts[:, :, :, named].max(axis=3).min(axis=(0, 1, 2))
        assert (points >= lo).all() and (points <= hi).all() and N >= 8 * 512
    assert _same(scene_depth_hip(jd, list(lengths), pd, segs, radius), got)                       # a second launch: the same bits
    assert _same(scene_depth_hip(jd, torch.tensor(lengths, dtype=torch.int32, device=dev), pd, _t(segs), _t(radius)), got)
    # what must not be read (NaN so far) now holds points of the cloud: read, it would penetrate by a whole radius
    bait = jts.copy()
    fill = points[np.isfinite(points).all(axis=1)][:1]
    bait[np.isnan(bait).any(axis=-1)] = fill[0] if len(fill) else 0.0
    assert _same(scene_depth_hip(_t(bait).to(dev), list(lengths), pd, segs, radius), got)


def _full_case():
    """A case whose windows are all full: the frames past the short window repeat its first ones."""
    case = (2, 3, CHUNK + 1, 24, 257, 21, "mixed")
    jts, lengths, points, segs, radius = SREF.inputs(*case)
    jts = jts.copy()
    n = lengths[1]
    jts[1, :, n:] = jts[1, :, :case[2] - n]
    assert np.isfinite(jts[:, :, :, np.unique(segs)]).all()
    return case, jts, points, segs, radius


def test_scene_depth_is_bitwise_independent_of_order_reach_and_layout(dev):
    from seeme_amd.recording import scene_depth_hip
    (W, K, T, J, N, NB, _), jts, points, segs, radius = _full_case()
    jd, pd = _t(jts).to(dev), _t(points).to(dev)
    full = [T] * W
    got = scene_depth_hip(jd, full, pd, segs, radius)
    assert int(got["hits"].sum()) > 0
    g = np.random.default_rng(4)
    perm = g.permutation(N)
    assert _same(scene_depth_hip(jd, full, _t(points[perm]).to(dev), segs, radius), got)          # the order of the points
    far = g.uniform(7.9, 8.0, (300, 3)).astype(np.float32)             # out of reach: the bodies stay within 7.1 m, radii <= 0.1 m
    more = np.concatenate([points[:100], far[:150], points[100:], far[150:]])
    assert _same(scene_depth_hip(jd, full, _t(more).to(dev), segs, radius), got)                  # N, under appended far points
    K2 = 8                                                             # a hypothesis replicated to a larger K
    wide = scene_depth_hip(_t(jts[:, np.arange(K2) % K]).to(dev), full, pd, segs, radius)
    assert torch.equal(wide["depth"], got["depth"][:, torch.arange(K2) % K]) and torch.equal(wide["cost"], got["cost"][:, torch.arange(K2) % K])
    flat = scene_depth_hip(jd.reshape(1, 1, W * K * T, J, 3), [W * K * T], pd, segs, radius)      # the same frames as one row: other
    assert torch.equal(flat["depth"].reshape(W, K, T), got["depth"])                              # chunks, other boxes, the same bits
    one = scene_depth_hip(jd[1:, 2:], [T], pd, segs, radius)           # W and K: a hypothesis on its own
    assert torch.equal(one["depth"][0, 0], got["depth"][1, 2]) and torch.equal(one["cost"][0, 0], got["cost"][1, 2])


# ----------------------------------------------------------------------------- 2. bad arguments
def test_scene_depth_bad_arguments_raise(dev):
    from seeme_amd import _lib as L
    from seeme_amd import recording as R
    W, K, T, J, N = 2, 3, 8, 24, 50
    jts, pts = torch.zeros(W, K, T, J, 3, device=dev), torch.zeros(N, 3, device=dev)
    len32 = torch.full((W,), T, dtype=torch.int32, device=dev)
    segs, radius = np.array([[0, 1], [2, 2]], np.int32), np.array([0.05, 0.02], np.float32)
    slot = lambda: {"depth": torch.zeros(W, K, T, device=dev), "cost": torch.zeros(W, K, device=dev),
                    "hits": torch.zeros(W, K, dtype=torch.int32, device=dev)}
    assert R.scene_depth_hip(jts, [T] * W, pts, segs, radius)["depth"].shape == (W, K, T)
    with pytest.raises(L.SeemeError, match="NB must"):
        R.scene_depth_hip(jts, [T] * W, pts, np.zeros((33, 2), np.int32), np.zeros(33, np.float32))
    assert R.scene_depth_hip(jts, [T] * W, pts, np.zeros((32, 2), np.int32), np.zeros(32, np.float32))["cost"].shape == (W, K)
    with pytest.raises(L.SeemeError, match="K must"):
        R.scene_depth_hip(torch.zeros(W, 33, T, J, 3, device=dev), [T] * W, pts, segs, radius)
    with pytest.raises(L.SeemeError, match="J must"):
        R.scene_depth_hip(torch.zeros(W, K, T, 33, 3, device=dev), [T] * W, pts, segs, radius)
    for bad in ([[0, 24], [2, 2]], [[0, 1], [-1, 2]]):
        with pytest.raises(L.SeemeError, match="segment index"):
            R.scene_depth_hip(jts, [T] * W, pts, np.array(bad, np.int32), radius)
    for bad in (-0.01, float("nan"), float("inf")):
        with pytest.raises(L.SeemeError, match="radius"):
            R.scene_depth_hip(jts, [T] * W, pts, segs, np.array([0.05, bad], np.float32))
    for kw, msg in ((dict(W=0), "W must"), (dict(W=-1), "W must"), (dict(T=0), "T must"), (dict(N=0), "N must"), (dict(K=0), "K must")):
        a = dict(W=W, K=K, T=T, J=J, N=N)
        a.update(kw)
        with pytest.raises(L.SeemeError, match=msg):
            R._launch_scene_depth(jts, len32, pts, a["W"], a["K"], a["T"], a["J"], a["N"], segs, radius, 2, out=slot())
    for a, b, c, s, r in ((None, len32, pts, segs, radius), (jts, None, pts, segs, radius), (jts, len32, None, segs, radius),
                          (jts, len32, pts, None, radius), (jts, len32, pts, segs, None)):
        with pytest.raises(L.SeemeError, match="null"):
            R._launch_scene_depth(a, b, c, W, K, T, J, N, s, r, 2, out=slot())
    with pytest.raises(L.SeemeError):                                  # host tensors
        R.scene_depth_hip(jts.cpu(), [T] * W, pts.cpu(), segs, radius)
    for args in ((jts[..., :2], [T] * W, pts), (jts, [T] * W, pts[:, :2]), (jts, [T], pts), (jts, [T, 2.5], pts),
                 (jts.double(), [T] * W, pts.double()), (jts, [T] * W, pts.double()), (jts, [T] * W, pts.cpu()), (jts[0], [T], pts)):
        with pytest.raises(ValueError, match="scene_depth"):
            R.scene_depth_hip(*args, segs, radius)
    for s, r in ((segs[:, :1], radius), (segs.astype(np.float32), radius), (segs, radius[:1])):
        with pytest.raises(ValueError, match="scene_depth"):
            R.scene_depth_hip(jts, [T] * W, pts, s, r)


# ----------------------------------------------------------------------------- 3. MLD.predict_recording
@pytest.fixture(scope="module")
def scene_model(dev):
    return _mld(dev, "config_mld_scene.yaml", mutate=_mut)


@pytest.fixture(scope="module")
def moving_case(dev, scene_model):
    """The moving-camera batch of tests/test_gpu_headset.py (3 windows, K = 4, fixed latents), the call without a cloud made once,
    and a cloud in the world frame: joints of the hypotheses, moved by 3 cm of noise, so that bodies do reach into it."""
    from seeme_amd import recording as R
    from test_gpu_scene_views import _to_world
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
    betas = torch.from_numpy(rec["wearer_betas"]).to(dev)
    kw = dict(overlap=O, betas=betas, num_hypotheses=K, latents=lat, cond_noise=cn, window_frames=frames["world2cam"].float())
    assert model.transl_in_feats
    plain = model.predict_recording(batch, n, **kw)
    Mw = frames["world2cam"].numpy()
    world = _to_world(plain["predict"]["joints_rst_all"], Mw)                                       # [W,K,T,24,3] float64
    g = np.random.default_rng(12)
    pick = np.stack([g.integers(0, s, 1500) for s in world.shape[:4]])
    pick[2] = np.minimum(pick[2], np.array(lengths)[pick[0]] - 1)
    cloud = (world[tuple(pick)] + 0.03 * g.standard_normal((1500, 3))).astype(np.float32)
    return {"n": n, "T": T, "O": O, "K": K, "W": len(starts), "batch": batch, "kw": kw, "Mw": Mw, "plain": plain, "cloud": cloud,
            "betas": betas, "head_path": R.camera_centres(w2c)}


def test_predict_recording_with_the_scene_terms_off_is_bit_identical(dev, scene_model, moving_case):
    model = scene_model[0]
    c = moving_case
    for extra in (dict(), dict(scene_weight=0.0, scene_report=False), dict(capsules=([[0, 1]], [0.1]))):
        out = model.predict_recording(c["batch"], c["n"], scene_cloud=c["cloud"], **extra, **c["kw"])
        a, b = dict(_flat(c["plain"])), dict(_flat(out))
        assert set(a) == set(b) and not any(k.startswith("scene_") for k in b)
        for k, v in a.items():
            assert torch.equal(v, b[k]) if isinstance(v, torch.Tensor) else v == b[k], k
    for kw, name in ((dict(scene_weight=1.0), "scene_cloud"), (dict(scene_report=True), "scene_cloud"),
                     (dict(scene_weight=-1.0, scene_cloud=c["cloud"]), "scene_weight"),
                     (dict(scene_weight=True, scene_cloud=c["cloud"]), "scene_weight"),
                     (dict(scene_report=1, scene_cloud=c["cloud"]), "scene_report"),
                     (dict(scene_weight=1.0, scene_cloud=c["cloud"][:, :2]), "scene_cloud"),
                     (dict(scene_report=True, scene_cloud=np.zeros((5, 3), np.int64)), "scene_cloud"),
                     (dict(scene_weight=1.0, scene_cloud=c["cloud"], capsules=[[0, 1]]), "capsules")):
        with pytest.raises(ValueError, match=name):
            model.predict_recording(c["batch"], c["n"], **kw, **c["kw"])


def test_predict_recording_scene_weight_adds_the_body_scene_term(dev, scene_model, moving_case):
    from seeme_amd import recording as R
    from test_gpu_scene_views import _to_world
    model = scene_model[0]
    c = moving_case
    W, K, O, sw, hw = c["W"], c["K"], c["O"], 3.0, 2.0
    out = model.predict_recording(c["batch"], c["n"], scene_cloud=c["cloud"], scene_weight=sw, head_path=c["head_path"], head_weight=hw,
                                  **c["kw"])
    assert set(out) == set(c["plain"]) | {"scene_cost", "scene_hits", "scene_cost_path", "head_cost", "head_cost_path"}
    pr, path = out["predict"], out["path"].cpu().tolist()
    assert torch.equal(pr["joints_rst_all"], c["plain"]["predict"]["joints_rst_all"])             # the same hypotheses
    world = torch.from_numpy(_to_world(pr["joints_rst_all"], c["Mw"]))                             # float64, on the host
    segs, radius = R.body_capsules(model.smpl_model, c["betas"], 0.5)
    assert segs.shape == (21, 2) and model.scene_capsule_quantile == 0.5
    want = R.scene_depth_torch(world, out["window_lengths"], torch.from_numpy(c["cloud"]).double(), segs, radius)
    assert out["scene_cost"].shape == (W, K) and out["scene_cost"].dtype == torch.float32 and out["scene_hits"].dtype == torch.int32
    e = float((out["scene_cost"].double().cpu() - want["cost"]).abs().max())
    print(f"predict_recording: scene_cost {out['scene_cost'].tolist()} mm, hits {out['scene_hits'].tolist()}, error {e:.3e} mm "
          f"(bound {E2E_TOL_MM:g})")
    assert e <= E2E_TOL_MM and float(want["cost"].max()) > 1.0 and int(out["scene_hits"].sum()) > 0
    assert torch.equal(out["scene_cost_path"], out["scene_cost"][torch.arange(W), out["path"]])
    # the path is the minimum of the seams and the unary rebuilt from the returned pieces: medoid + head + scene
    cost = R.overlap_cost_torch(world, O)
    unary = model.path_medoid_weight * pr["hyp_metrics"]["PAIR_DIST"].double().cpu().sum(dim=2) / max(K - 1, 1) \
        + hw * out["head_cost"].double().cpu() + sw * out["scene_cost"].double().cpu()
    ref = R.path_select_torch(cost, unary)
    low, mine = float(ref["path_cost"]), REF.path_total(cost.numpy(), unary.numpy(), path)
    print(f"  path {path} (without the terms {c['plain']['path'].tolist()}), float64 total {mine:.4f} vs the minimum {low:.4f}")
    assert mine - low <= TOL_F32 * low and abs(float(out["path_cost"]) - mine) <= TOL_F32 * mine
    # the scene term alone, with capsules of the caller's
    caps = ([[j, j] for j in range(24)], [0.05] * 24)
    alone = model.predict_recording(c["batch"], c["n"], scene_cloud=c["cloud"], scene_weight=sw, medoid_weight=0, capsules=caps, **c["kw"])
    want = R.scene_depth_torch(world, out["window_lengths"], torch.from_numpy(c["cloud"]).double(), *caps)
    assert float((alone["scene_cost"].double().cpu() - want["cost"]).abs().max()) <= E2E_TOL_MM
    unary = sw * alone["scene_cost"].double().cpu()
    mine = REF.path_total(cost.numpy(), unary.numpy(), alone["path"].cpu().tolist())
    low = float(R.path_select_torch(cost, unary)["path_cost"])
    assert mine - low <= TOL_F32 * low


def test_predict_recording_scene_term_finds_the_planted_hypothesis(dev, scene_model):
    """One window, no medoid term, 1 mm spheres at the joints, and a cloud made of the frame-0 joints of every hypothesis but one:
    the others touch the cloud in frame 0, the spared one does not, and it is chosen."""
    from seeme_amd import recording as R
    model, dm, cfg = scene_model
    n, T, O, K, spared = 13, 16, 4, 4, 2
    rec = _synthetic_recording(n, seed=2)
    rec["n_frames"] = n
    batch, starts, lengths = R.windows_batch(rec, dm, T, O, tuple(cfg.model.condition), dataset="egobody", device=dev)
    assert lengths == [13]
    lat, cn = _draws(1, K, model.do_classifier_free_guidance, dev, seed=6)
    kw = dict(overlap=O, medoid_weight=0, num_hypotheses=K, latents=lat, cond_noise=cn)
    jts = model.predict_recording(batch, n, **kw)["predict"]["joints_rst_all"]                    # [1,K,13,24,3], the frame of the seams
    assert jts.shape[:3] == (1, K, n)
    cloud = torch.cat([jts[0, k, 0] for k in range(K) if k != spared]).cpu()
    caps = (np.array([[j, j] for j in range(24)], np.int32), np.full(24, 1e-3, np.float32))
    ref = SREF.scene_depth(jts.cpu().numpy(), [n], cloud.numpy(), *caps)
    print(f"planted: reference cost {ref['cost'].tolist()} mm")
    assert ref["cost"][0, spared] == 0.0 and all(ref["cost"][0, k] > 0.0 for k in range(K) if k != spared)
    out = model.predict_recording(batch, n, scene_cloud=cloud, scene_weight=1.0, capsules=caps, **kw)
    assert out["path"].cpu().tolist() == [spared]
    assert float(out["scene_cost"][0, spared]) == 0.0 and int(out["scene_hits"][0, spared]) == 0
    assert float(np.abs(out["scene_cost"].double().cpu().numpy() - ref["cost"]).max()) <= TOL_MM and float(out["path_cost"]) == 0.0


def test_predict_recording_scene_report_is_the_depth_of_the_final_joints(dev, scene_model, moving_case):
    from seeme_amd import recording as R
    model = scene_model[0]
    c = moving_case
    segs, radius = R.body_capsules(model.smpl_model, c["betas"], 0.5)
    cloud64 = torch.from_numpy(c["cloud"]).double()
    out = model.predict_recording(c["batch"], c["n"], scene_cloud=c["cloud"], scene_report=True, **c["kw"])
    assert set(out) == set(c["plain"]) | {"scene_depth"} and torch.equal(out["joints"], c["plain"]["joints"])
    assert out["scene_depth"].shape == (c["n"],) and out["scene_depth"].dtype == torch.float32
    want = R.scene_depth_torch(out["joints"].double().cpu()[None, None], [c["n"]], cloud64, segs, radius)["depth"][0, 0]
    e = float((out["scene_depth"].double().cpu() - want).abs().max())
    print(f"scene_report: depth up to {float(want.max()):.2f} mm over {c['n']} frames, error {e:.3e} mm")
    assert e <= TOL_MM and float(want.max()) > 0.0
    # with the anchoring: the depth of the joints AFTER the shift
    moved = model.predict_recording(c["batch"], c["n"], scene_cloud=c["cloud"], scene_report=True, head_path=c["head_path"],
                                    head_anchor=True, **c["kw"])
    assert set(moved) == set(c["plain"]) | {"scene_depth", "head_shift", "head_residual", "transl"}
    assert not torch.equal(moved["joints"], out["joints"])
    want = R.scene_depth_torch(moved["joints"].double().cpu()[None, None], [c["n"]], cloud64, segs, radius)["depth"][0, 0]
    assert float((moved["scene_depth"].double().cpu() - want).abs().max()) <= TOL_MM
    # with the weight as well: both sets of keys
    both = model.predict_recording(c["batch"], c["n"], scene_cloud=c["cloud"], scene_report=True, scene_weight=1.0, **c["kw"])
    assert set(both) == set(c["plain"]) | {"scene_depth", "scene_cost", "scene_hits", "scene_cost_path"}


def test_predict_recording_scene_weight_needs_a_translation(dev):
    from seeme_amd import recording as R
    from test_gpu_rot6d import _mld as _mld_rot6d
    n, T, O, K = 37, 16, 4, 3
    model, dm, cfg = _mld_rot6d(dev, "config_mld_egobody_rot6d.yaml", T=T, mutate=_mut)
    model.eval()
    assert not model.transl_in_feats and model.path_scene_weight == 0.0 and model.scene_report is False
    starts, lengths = R.window_plan(n, T, O)
    batch = dm.batch(len(starts), idx=2, lengths=lengths)
    lat, cn = _draws(len(starts), K, model.do_classifier_free_guidance, dev, seed=3)
    kw = dict(overlap=O, num_hypotheses=K, latents=lat, cond_noise=cn)
    cloud = np.random.default_rng(2).uniform(-1.0, 1.0, (200, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="PATH_SCENE_WEIGHT"):
        model.predict_recording(batch, n, scene_cloud=cloud, scene_weight=1.0, **kw)
    out = model.predict_recording(batch, n, scene_cloud=cloud, scene_report=True, **kw)            # the report needs none
    segs, radius = R.body_capsules(model.smpl_model, None, 0.5)
    want = R.scene_depth_torch(out["joints"].double().cpu()[None, None], [n], torch.from_numpy(cloud).double(), segs, radius)
    assert float((out["scene_depth"].double().cpu() - want["depth"][0, 0]).abs().max()) <= TOL_MM


# ----------------------------------------------------------------------------- 4. cli.predict_main
def test_cli_predict_main_writes_the_scene_arrays(dev, tmp_path, scene_model):
    from conftest import REPO
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

    _, plain = run([])
    assert set(plain) == PARENT_KEYS
    _, zero = run(["--scene_weight", "0", "--scene_quantile", "0.9"])  # a weight of 0 and an unused quantile: the same arrays
    assert set(zero) == PARENT_KEYS and all(np.array_equal(zero[k], plain[k]) and zero[k].dtype == plain[k].dtype for k in plain)
    r, res = run(["--scene_weight", "1", "--scene_report", "--scene_quantile", "1.0"])
    assert set(res) == PARENT_KEYS | {"scene_cost", "scene_hits", "scene_depth"} and r["windows"] == 3
    assert res["scene_cost"].shape == (3, 3) and res["scene_cost"].dtype == np.float32 and res["scene_hits"].shape == (3, 3)
    assert res["scene_hits"].dtype == np.int32 and res["scene_depth"].shape == (n,) and res["scene_depth"].dtype == np.float32
    assert all(np.isfinite(v).all() for v in res.values()) and (res["scene_cost"] >= 0).all()
    # the report is the depth of the written joints against the recording's scene (the fixed cloud, in the common frame), with the
    # capsules of the recording's wearer at the quantile asked for
    segs, radius = R.body_capsules(model.smpl_model, rec["wearer_betas"], 1.0)
    want = R.scene_depth_torch(torch.from_numpy(res["joints"]).double()[None, None], [n], torch.from_numpy(rec["scene"]).double(), segs,
                               radius)["depth"][0, 0]
    e = float((torch.from_numpy(res["scene_depth"]).double() - want).abs().max())
    print(f"cli: scene_depth up to {float(want.max()):.2f} mm, error {e:.3e} mm; scene_cost {res['scene_cost'].tolist()}")
    assert e <= TOL_MM
    _, rep = run(["--scene_report"])
    assert set(rep) == PARENT_KEYS | {"scene_depth"} and np.array_equal(rep["joints"], plain["joints"])
    # neither key: the error names both
    np.savez(rec_path, **{k: v for k, v in rec.items() if k != "scene"}, world2cam=w2c)
    with pytest.raises(ValueError, match="scene_vertices.*scene"):
        run(["--scene_report"])
