"""The interactee track on the device: the two kernels of csrc/track.hip against the float64 twins of seeme_amd/track.py on the fp32
inputs the kernels saw, at the project's fp32 bound (applied as the stitch tests apply it: rotation-matrix entries and the
translation), then ``track_interactee`` (the composition of the twins) and ``cli.estimate_main --track`` on a sparse recording."""
import os

import numpy as np
import pytest
import torch

import recording_reference as REF
import track_reference as TR
from conftest import REPO
from test_gpu_flow_head import CFG, _frames, _mld
from test_gpu_hyp_select import TOL_F32, _elem_rel

pytestmark = pytest.mark.gpu

TILE = TR.TILE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- 1. transition costs
COST_CASES = [(2, 1), (3, 2), (5, 31), (4, 32), (70, 3)]


def _cost_input(Lf, S, seed):
    g = np.random.default_rng(seed)
    walk = np.cumsum(0.05 * g.standard_normal((Lf, 1, 24, 3)), axis=0) + g.standard_normal((1, 1, 24, 3))
    jts = torch.from_numpy(walk + 0.1 * g.standard_normal((Lf, S, 24, 3))).float()
    idx = np.cumsum(np.resize(np.array([1, 2, 7, 2, 1, 7]), Lf)) - 1     # gaps among {1, 2, 7}
    return jts, idx


@pytest.mark.parametrize("shape", COST_CASES, ids=str)
def test_track_cost_kernel_vs_float64_twin(dev, shape):
    from seeme_amd import track as TK
    Lf, S = shape
    jts, idx = _cost_input(Lf, S, seed=Lf + S)
    assert set(np.diff(idx).tolist()) <= {1, 2, 7}
    weight = 1e6 / (2 * 20.0 ** 2)
    want = TK.track_cost_torch(jts.double(), idx, weight)              # float64 on the inputs the kernel saw
    j32 = jts.to(dev)
    got = TK.track_cost_hip(j32, idx, weight)
    torch.cuda.synchronize()
    assert got.shape == (Lf - 1, S, S) and got.dtype == torch.float32
    e = _elem_rel(got, want)
    print(f"track_cost {shape}: max element-wise relative error {e:.3e}")
    assert e <= TOL_F32, e
    assert torch.equal(TK.track_cost_hip(j32, idx, weight), got)        # two runs are bit-equal
    idx32 = torch.from_numpy(idx.astype(np.int32)).to(dev)
    filled = TK._launch_cost(j32, idx32, Lf, S, weight, out=torch.full((Lf - 1, S, S), float("nan"), device=dev))
    assert torch.equal(filled, got)                                     # ... whatever the output held before


def test_track_cost_single_key_frame_writes_nothing(dev):
    from seeme_amd import track as TK
    jts, idx = _cost_input(1, 4, seed=1)
    assert TK.track_cost_hip(jts.to(dev), idx, 1.0).shape == (0, 4, 4)
    out = torch.full((1, 4, 4), -7.0, device=dev)
    TK._launch_cost(jts.to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev), 1, 4, 1.0, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ----------------------------------------------------------------------------- 2. fill and filter
def _every(L, seed, gaps=(1, 2, 7, 4)):
    g = np.random.default_rng(seed)
    idx = np.cumsum(g.choice(gaps, L)) - 1
    return idx[idx < L]


FILTER_CASES = {                                                        # name: (idx, L, R)
    "one_frame": ([0], 1, 2),
    "dense_no_filter": (list(range(5)), 5, 0),
    "both_ends_truncated": ([0, 2, 3, 6, 8], 9, 32),
    "halo_crosses_a_tile_edge": (_every(TILE + 3, 1).tolist(), TILE + 3, 3),
    "interval_spans_a_tile": ([0, 1, TILE + 40, 2 * TILE], 2 * TILE + 1, 6),
    "holds": ([3, 5, 10, 16], 20, 2),
    "sparse_no_filter": ([1, 4, 5, 9], 12, 0),
}
# seeds for which the generator meets the tests' condition on their inputs (asserted below): every pair of quaternions that meets
# inside a window, or as neighbouring keys, has |dot| >= 0.1
SEEDS = {"one_frame": 1, "dense_no_filter": 2, "both_ends_truncated": 3, "halo_crosses_a_tile_edge": 4, "interval_spans_a_tile": 5,
         "holds": 6, "sparse_no_filter": 7}


def _taps(R):
    return (np.exp(-np.arange(R + 1.0) ** 2 / (2 * max(R / 3.0, 0.5) ** 2)) if R else np.ones(1)).astype(np.float32)


def _filter_err(out, tout, Mw, Tw):
    e_r = float(np.abs(TR.matrices(out.double().cpu().numpy()) - Mw).max())
    e_t = 0.0 if Tw is None else float(np.abs(tout.double().cpu().numpy() - Tw).max())
    return e_r, e_t


@pytest.mark.parametrize("body", [(24, True), (22, False)], ids=["J24_transl", "J22"])
@pytest.mark.parametrize("name", list(FILTER_CASES))
def test_track_filter_kernel_vs_float64_twin(dev, name, body):
    from seeme_amd import track as TK
    idx, L, R = FILTER_CASES[name]
    idx = np.asarray(idx)
    J, with_transl = body
    taps = _taps(R)
    for kind in ("apart", "smooth"):
        if kind == "apart":                                             # neighbouring keys 0.3..1.0 rad apart: the slerp branch
            pose, tr = TR.keys_apart(len(idx), J, SEEDS[name], with_transl)
        else:                                                           # cut from one smooth motion: the lerp branch
            pose, tr = TR.smooth_keys(idx, L, J, SEEDS[name], with_transl)
        p32 = torch.from_numpy(pose).float()
        t32 = None if tr is None else torch.from_numpy(tr).float()
        low = TR.min_abs_dot(p32.double().numpy(), idx, L, R)           # the condition on the inputs, in float64 (not a kernel property)
        assert low >= 0.1, (name, kind, low)
        want, twant = TK.track_filter_torch(p32.double(), None if t32 is None else t32.double(), idx, L, taps)
        Mw, Tw = TR.matrices(want.numpy()), None if twant is None else twant.numpy()
        got, tgot = TK.track_filter_hip(p32.to(dev), None if t32 is None else t32.to(dev), idx, L, taps)
        torch.cuda.synchronize()
        assert got.shape == (L, J, 3) and got.dtype == torch.float32 and torch.isfinite(got).all()
        assert (tgot is None) == (not with_transl) and (tgot is None or (tgot.shape == (L, 3) and torch.isfinite(tgot).all()))
        e_r, e_t = _filter_err(got, tgot, Mw, Tw)
        print(f"track_filter {name} J {J} {kind}: rotation matrices {e_r:.3e}, translation {e_t:.3e} (min |dot| {low:.3f})")
        assert e_r <= TOL_F32 and e_t <= TOL_F32, (e_r, e_t)
        assert float(torch.linalg.vector_norm(got, dim=-1).max()) <= np.pi + 1e-5        # angles in [0, pi]
        if R == 0:                                                      # a key without a filter: bit for bit
            assert torch.equal(got[idx].cpu(), p32) and (tgot is None or torch.equal(tgot[idx].cpu(), t32))
        elif len(idx) > 1 and kind == "apart":                          # with a filter nothing is copied
            assert not torch.equal(got[idx].cpu(), p32)
        # alternate keys rewritten as the -q axis-angle: the same rotations
        f32 = torch.from_numpy(TR.flip_alternate(p32.double().numpy())).float()
        fgot, ftgot = TK.track_filter_hip(f32.to(dev), None if t32 is None else t32.to(dev), idx, L, taps)
        e_r, e_t = _filter_err(fgot, ftgot, Mw, Tw)
        print(f"  -q keys: {e_r:.3e}, {e_t:.3e}")
        assert e_r <= TOL_F32 and e_t <= TOL_F32, (e_r, e_t)
        # NaN in the outputs before the launch changes no bit; neither does a second run
        idx32 = torch.from_numpy(idx.astype(np.int32)).to(dev)
        slot = (torch.full((L, J, 3), float("nan"), device=dev), None if t32 is None else torch.full((L, 3), float("nan"), device=dev))
        again = TK._launch_filter(p32.to(dev), None if t32 is None else t32.to(dev), idx32, len(idx), L, J, taps, R, out=slot)
        assert torch.equal(again[0], got) and (tgot is None or torch.equal(again[1], tgot))


def test_track_filter_holds_and_single_tap_equivalence(dev):
    from seeme_amd import track as TK
    idx, L = np.array([3, 5, 10, 16]), 20                               # first key at 3, last key at L - 4
    pose, tr = TR.keys_apart(4, 24, seed=6)
    p, t = torch.from_numpy(pose).float().to(dev), torch.from_numpy(tr).float().to(dev)
    out, tout = TK.track_filter_hip(p, t, idx, L, [1.0])
    Mk = TR.matrices(p.double().cpu().numpy())
    Mo = TR.matrices(out.double().cpu().numpy())
    assert np.abs(Mo[:3] - Mk[:1]).max() <= TOL_F32 and np.abs(Mo[17:] - Mk[-1:]).max() <= TOL_F32
    assert torch.equal(tout[:3], t[:1].expand(3, 3)) and torch.equal(tout[17:], t[-1:].expand(3, 3))
    oz, tz = TK.track_filter_hip(p, t, idx, L, [1.0, 0.0, 0.0])        # taps [1, 0, 0] are no filter, in matrices
    assert np.abs(TR.matrices(oz.double().cpu().numpy()) - Mo).max() <= TOL_F32 and float((tz - tout).abs().max()) <= TOL_F32


# ----------------------------------------------------------------------------- 3. bad arguments
def test_track_kernels_bad_arguments_raise_and_launch_nothing(dev):
    from seeme_amd import _lib as L
    from seeme_amd import track as TK
    import ctypes as C
    st = L.current_stream()
    jts, idx = _cost_input(3, 4, seed=2)
    j32, i32 = jts.to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev)
    cost = torch.full((2, 4, 4), -7.0, device=dev)
    for args in ((0, i32.data_ptr(), 3, 4, 1.0, cost.data_ptr(), st), (j32.data_ptr(), 0, 3, 4, 1.0, cost.data_ptr(), st),
                 (j32.data_ptr(), i32.data_ptr(), 3, 4, 1.0, 0, st)):
        with pytest.raises(L.SeemeError, match="null pointer"):
            L.call("seeme_track_cost", *args)
    with pytest.raises(L.SeemeError, match="S must be"):
        TK.track_cost_hip(torch.zeros(2, 33, 24, 3, device=dev), [0, 1], 1.0)
    with pytest.raises(L.SeemeError, match="S must be"):
        L.call("seeme_track_cost", j32.data_ptr(), i32.data_ptr(), 3, 0, 1.0, cost.data_ptr(), st)
    with pytest.raises(L.SeemeError, match="Lf must be"):
        L.call("seeme_track_cost", j32.data_ptr(), i32.data_ptr(), 65537, 4, 1.0, cost.data_ptr(), st)
    with pytest.raises(L.SeemeError):
        TK.track_cost_hip(jts, idx, 1.0)                                # not on the device
    with pytest.raises(ValueError, match="idx"):
        TK.track_cost_hip(j32, [0, 2, 2], 1.0)                          # validated on the host, before any upload
    torch.cuda.synchronize()
    assert bool((cost == -7.0).all())

    pose, tr = TR.keys_apart(3, 24, seed=1)
    p, t = torch.from_numpy(pose).float().to(dev), torch.from_numpy(tr).float().to(dev)
    fidx = np.array([0, 2, 5])
    f32 = torch.from_numpy(fidx.astype(np.int32)).to(dev)
    out, tout = torch.full((6, 24, 3), -7.0, device=dev), torch.full((6, 3), -7.0, device=dev)
    one = (C.c_float * 1)(1.0)

    def raw(pose_=p.data_ptr(), transl_=t.data_ptr(), idx_=f32.data_ptr(), taps_=one, out_=out.data_ptr(), tout_=tout.data_ptr()):
        L.call("seeme_track_filter", pose_, transl_, idx_, 3, 6, 24, taps_, 0, out_, tout_, st)

    for kw in ({"pose_": 0}, {"idx_": 0}, {"taps_": None}, {"out_": 0}, {"transl_": 0}, {"tout_": 0}):
        with pytest.raises(L.SeemeError, match="null pointer"):
            raw(**kw)
    slot = (out, tout)
    with pytest.raises(L.SeemeError, match="R must be"):
        TK._launch_filter(p, t, f32, 3, 6, 24, np.ones(34, np.float32), 33, out=slot)
    with pytest.raises(L.SeemeError, match=r"taps\[0\]"):
        TK._launch_filter(p, t, f32, 3, 6, 24, np.array([0.0, 1.0], np.float32), 1, out=slot)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(L.SeemeError, match="tap"):
            TK._launch_filter(p, t, f32, 3, 6, 24, np.array([1.0, bad], np.float32), 1, out=slot)
    with pytest.raises(L.SeemeError, match="J must be"):
        TK._launch_filter(p, t, f32, 3, 6, 0, np.ones(1, np.float32), 0, out=slot)
    with pytest.raises(L.SeemeError, match="J must be"):
        TK._launch_filter(p, t, f32, 3, 6, 33, np.ones(1, np.float32), 0, out=slot)
    with pytest.raises(L.SeemeError, match="Lf must be"):
        TK._launch_filter(p, t, f32, 3, 2, 24, np.ones(1, np.float32), 0, out=slot)
    with pytest.raises(L.SeemeError, match="L must be"):
        TK._launch_filter(p, t, f32, 3, (1 << 20) + 1, 24, np.ones(1, np.float32), 0, out=slot)
    for bad_idx in ([0, 2, 2], [0, 2, 6], [-1, 2, 5], [0.0, 2.0, 5.0]):  # validated on the host, before any upload
        with pytest.raises(ValueError, match="idx"):
            TK.track_filter_hip(p, t, bad_idx, 6, [1.0])
    with pytest.raises(L.SeemeError):
        TK.track_filter_hip(p.cpu(), t.cpu(), fidx, 6, [1.0])
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((tout == -7.0).all())
    good, tgood = TK._launch_filter(p, t, f32, 3, 6, 24, np.ones(1, np.float32), 0, out=slot)      # the same slots, good arguments
    assert torch.isfinite(good).all() and torch.equal(good[fidx], p) and torch.equal(tgood[fidx], t)


# ----------------------------------------------------------------------------- 4. the track
@pytest.mark.parametrize("shape", [(4, 3, 9), (12, 8, 60)], ids=str)
def test_track_interactee_is_the_composition_of_the_twins(dev, shape):
    from seeme_amd import track as TK
    from seeme_amd.smpl import SMPL
    Lf, S, L = shape
    idx = np.array([0, 2, 3, 8]) if Lf == 4 else _every(L, 3)[:Lf]
    assert len(idx) == Lf
    go, bp, tr, lp = (torch.from_numpy(x).float() for x in TR.candidates(Lf, S, seed=11 + Lf))
    betas = torch.from_numpy(0.3 * np.random.default_rng(1).standard_normal(10)).float()
    smpl32, smpl64 = SMPL.synthetic(1234, V=256).to(dev), SMPL.synthetic(1234, V=256).double()
    kw = dict(step_mm=20.0, prior_weight=1.0, sigma=1.5)
    out = TK.track_interactee(go, bp, tr, lp, idx, L, smpl32, betas, device=dev, **kw)
    torch.cuda.synchronize()
    want = TK.track_interactee(go.double(), bp.double(), tr.double(), lp.double(), idx, L, smpl64, betas.double(), **kw)
    assert out["global_orient"].shape == (L, 3) and out["body_pose"].shape == (L, 69) and out["transl"].shape == (L, 3)
    assert out["path"].shape == (Lf,) and out["path"].dtype == torch.int64 and out["step_cost"].shape == (Lf - 1,)
    # the cost kernel on the joints the device posed
    assert _elem_rel(out["cost"], TK.track_cost_torch(out["joints"].double().cpu(), idx, 1e6 / 800.0)) <= TOL_F32
    # the path: its float64 total under the twins' costs is within TOL_F32 (relative) of the minimum (no index equality where two
    # paths lie closer than that)
    c64, u64 = want["cost"].numpy(), want["unary"].numpy()
    path = out["path"].cpu().tolist()
    mine = REF.path_total(c64, u64, path)
    low = REF.best_path_enumerate(c64, u64, Lf, S)[0] if S ** Lf <= 100 else float(want["path_cost"])
    print(f"track_interactee {shape}: path {path}, total {mine:.6f}, minimum {low:.6f}")
    assert mine - low <= TOL_F32 * low, (mine, low)
    assert abs(float(out["path_cost"]) - mine) <= TOL_F32 * mine
    assert _elem_rel(out["step_cost"], torch.from_numpy(np.array([c64[l, path[l], path[l + 1]] for l in range(Lf - 1)]))) <= TOL_F32
    # the motion: the float64 filter of the rows the device chose
    keys = torch.cat([go, bp], dim=-1)[torch.arange(Lf), torch.tensor(path)].reshape(Lf, 24, 3)
    assert TR.min_abs_dot(keys.double().numpy(), idx, L, 5) >= 0.1
    fw, tw = TK.track_filter_torch(keys.double(), tr.double(), idx, L, TK.gaussian_taps(1.5))
    got = torch.cat([out["global_orient"], out["body_pose"]], dim=-1).reshape(L, 24, 3)
    e_r, e_t = _filter_err(got, out["transl"], TR.matrices(fw.numpy()), tw.numpy())
    print(f"  rotation matrices {e_r:.3e}, translation {e_t:.3e}")
    assert e_r <= TOL_F32 and e_t <= TOL_F32


# ----------------------------------------------------------------------------- 5. estimate.py --track on a sparse recording
@pytest.fixture(scope="module")
def model(dev):
    return _mld(dev)


def test_cli_estimate_main_track_then_predict_main(dev, model, tmp_path):
    from seeme_amd import cli, recording as R
    m, _dm, _cfg = model
    ckpt = os.path.join(tmp_path, "model.ckpt")
    cli.save_checkpoint(ckpt, m, 0, 0)
    n, S = 9, 4
    stored = np.array([0, 2, 3, 6, 8])
    nf = len(stored)
    fr = _frames(n, seed=4)
    fr = dict(fr, video=fr["video"][stored], video_index=stored)
    rec_path, out_path, out2 = (os.path.join(tmp_path, f) for f in ("rec.npz", "with_interactee.npz", "again.npz"))
    np.savez(rec_path, **fr)
    base = ["--cfg", os.path.join(REPO, "configs", CFG), "--checkpoint", ckpt, "--folder", str(tmp_path), "--scene_points", "256"]
    argv = base + ["--input", rec_path, "--num_samples", str(S), "--seed", "3", "--track", "--chunk_frames", "2"]
    r = cli.estimate_main(argv + ["--output", out_path])
    assert r["file"] == out_path and r["n_frames"] == n and r["num_samples"] == S and r["stored_frames"] == nf and len(r["path"]) == nf
    with np.load(out_path, allow_pickle=False) as z:
        got = {k: z[k] for k in z.files}
    assert all(np.array_equal(got[k], fr[k]) for k in fr)               # the input's keys are copied through
    shapes = {"global_orient": (n, 3), "body_pose": (n, 69), "transl": (n, 3), "betas": (10,), "interactee_betas_frames": (nf, 10),
              "interactee_cam": (nf, 3), "interactee_log_prob": (nf, S), "scene_view_count": (nf,), "interactee_frames": (nf,),
              "interactee_path": (nf,), "interactee_step_cost": (nf - 1,), "interactee_raw_global_orient": (nf, 3),
              "interactee_raw_body_pose": (nf, 69), "interactee_raw_transl": (nf, 3)}
    for k, shp in shapes.items():
        assert got[k].shape == shp and np.isfinite(got[k]).all(), k
    assert np.array_equal(got["interactee_frames"], stored) and got["interactee_path"].tolist() == r["path"]
    assert ((0 <= got["interactee_path"]) & (got["interactee_path"] < S)).all() and (got["interactee_step_cost"] >= 0).all()
    rec = R.load_recording(out_path)
    assert rec["n_frames"] == n and np.array_equal(rec["video_index"], stored)
    # the same seed gives the same bytes, whatever the chunking
    cli.estimate_main([a if a != "2" else "64" for a in argv] + ["--output", out2])
    with open(out_path, "rb") as a, open(out2, "rb") as b:
        assert a.read() == b.read()
    # the options reach the track: no filter and no prior leave the path's own rows at the stored frames
    out3 = os.path.join(tmp_path, "unfiltered.npz")
    cli.estimate_main(argv + ["--output", out3, "--track_sigma", "0", "--track_prior_weight", "1e9"])
    with np.load(out3, allow_pickle=False) as z:
        assert z["interactee_path"].tolist() == [0] * nf               # a density that outweighs every transition keeps the mode
        assert np.array_equal(z["global_orient"][stored], z["interactee_raw_global_orient"])
        assert np.array_equal(z["body_pose"][stored], z["interactee_raw_body_pose"])
        assert np.array_equal(z["transl"][stored], z["interactee_raw_transl"])
    with pytest.raises(ValueError, match="TEST.TRACK_SIGMA"):
        cli.estimate_main(argv + ["--output", out3, "--track_sigma", "11"])
    # predict.py runs on it unchanged
    motion = os.path.join(tmp_path, "motion.npz")
    p = cli.predict_main(base + ["--input", out_path, "--output", motion, "--frames", "4", "--num_hypotheses", "2", "--seed", "5"])
    assert p["n_frames"] == n
    with np.load(motion, allow_pickle=False) as z:
        assert z["global_orient"].shape == (n, 3) and all(np.isfinite(z[k]).all() for k in z.files)
