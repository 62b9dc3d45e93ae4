"""Per-hypothesis mesh metrics, host side: the plain-torch twins against the reference's Procrustes error (golden fixture) and explicit
numpy loops, the MeshMetrics accumulator and its reduction, the config key and the C-ABI surface."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "pa_mpjpe.npz")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.abs(b)).max())


# ----------------------------------------------------------------------------- the twins
def test_pa_mpjpe_torch_float64_matches_the_reference_fixture():
    from seeme_amd.mesh_metrics import pa_mpjpe_torch
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    pred, ref, want, same = g["pred"], g["ref"], g["err"], int(g["same"])
    assert pred.shape == (64, 24, 3) and pred.dtype == np.float32 and want.dtype == np.float64 and len(g["mirrored"]) == 8
    assert np.allclose(g["per_joint"].mean(axis=-1), want, rtol=1e-15, atol=0) and np.array_equal(pred[same], ref[same])
    got = pa_mpjpe_torch(torch.from_numpy(pred).double(), torch.from_numpy(ref).double()).numpy()
    live = np.arange(64) != same
    e = _rel(got[live], want[live])
    print(f"pa_mpjpe_torch float64 vs reconstruction_error: {e:.3e}; pred == ref row {got[same]:.3e} m")
    assert e <= 1e-9 and abs(got[same]) <= 1e-9 and want[same] <= 1e-9
    # the mirrored rows are no better aligned than a rotation allows: a reflection would bring them to the noise level (~0.05 m)
    plain = np.setdiff1d(np.arange(64), np.append(g["mirrored"], same))
    print(f"mirrored rows {want[g['mirrored']].min():.4f}..{want[g['mirrored']].max():.4f} m, the others up to {want[plain].max():.4f} m")
    assert want[g["mirrored"]].min() > 2 * want[plain].max()
    # a map with repeats and a skipped frame
    m = [5, 5, -1, 0]
    sub = pa_mpjpe_torch(torch.from_numpy(pred[[5, 9, 3, 0]]).double(), torch.from_numpy(ref).double(), m).numpy()
    assert abs(sub[0] - want[5]) <= 1e-9 * want[5] and sub[2] == 0.0 and abs(sub[3] - want[0]) <= 1e-9 * want[0]
    assert abs(sub[1] - want[9]) > 1e-3           # prediction 9 against reference 5 is another number
    # float32 inputs stay float32 and stay close
    g32 = pa_mpjpe_torch(torch.from_numpy(pred), torch.from_numpy(ref))
    assert g32.dtype == torch.float32 and _rel(g32.numpy()[live], want[live]) <= 1e-4


def test_v2v_torch_against_numpy_loops():
    from seeme_amd.mesh_metrics import v2v_torch
    rng = np.random.Generator(np.random.PCG64(3))
    F, Fr, V = 5, 3, 7
    vp, pp = rng.standard_normal((F, V, 3)), rng.standard_normal((F, 3))
    vr, pr = rng.standard_normal((Fr, V, 3)), rng.standard_normal((Fr, 3))
    m = [2, 0, -1, 2, 1]
    want = np.zeros(F)
    for f in range(F):
        if m[f] < 0:
            continue
        s = 0.0
        for v in range(V):
            d = (vp[f, v] - pp[f]) - (vr[m[f], v] - pr[m[f]])
            s += float(np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2))
        want[f] = s / V
    t = torch.from_numpy
    got = v2v_torch(t(vp), t(pp), t(vr), t(pr), m).numpy()
    assert got[2] == 0.0 and np.abs(got - want).max() <= 1e-14
    same = v2v_torch(t(vp[:3]), t(pp[:3]), t(vr), t(pr)).numpy()                 # no map: frame f against reference f
    assert abs(same[1] - np.linalg.norm((vp[1] - pp[1]) - (vr[1] - pr[1]), axis=-1).mean()) <= 1e-14
    assert v2v_torch(t(vp).float(), t(pp).float(), t(vr).float(), t(pr).float(), m).dtype == torch.float32


def test_scene_min_dist2_torch_against_numpy_loops():
    from seeme_amd.mesh_metrics import scene_min_dist2_torch
    rng = np.random.Generator(np.random.PCG64(4))
    F, V, S, P = 4, 6, 2, 11
    verts, scene = rng.standard_normal((F, V, 3)), rng.standard_normal((S, P, 3)) * 2
    m = [1, -1, 0, 1]
    want = np.zeros(F)
    for f in range(F):
        if m[f] < 0:
            continue
        best = np.inf
        for v in range(V):
            for p in range(P):
                d = verts[f, v] - scene[m[f], p]
                best = min(best, float(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        want[f] = best
    for chunk in (1, 4, 11, 512):                # the chunking over P does not change the result
        got = scene_min_dist2_torch(torch.from_numpy(verts), torch.from_numpy(scene), m, chunk=chunk).numpy()
        assert got[1] == 0.0 and np.abs(got - want).max() <= 1e-15, chunk
    assert scene_min_dist2_torch(torch.from_numpy(verts[:2]).float(), torch.from_numpy(scene).float()).dtype == torch.float32


def test_mesh_metrics_from_meshes_torch_masks_and_units():
    from seeme_amd.mesh_metrics import CONTACT_D2_THRESH, mesh_metrics_from_meshes_torch, pa_mpjpe_torch
    assert CONTACT_D2_THRESH == 0.02             # squared metres (test_egohmr.py:548), not 2 cm
    rng = np.random.Generator(np.random.PCG64(5))
    B, K, T, V, P = 2, 3, 4, 5, 6
    t = torch.from_numpy
    jp, vp = t(rng.standard_normal((B, K, T, 24, 3))), t(rng.standard_normal((B, K, T, V, 3)) * 0.2)
    jr, vr = t(rng.standard_normal((B, T, 24, 3))), t(rng.standard_normal((B, T, V, 3)) * 0.2)
    scene = t(rng.standard_normal((B, P, 3)) * 0.2)
    lengths = [4, 2]
    out = mesh_metrics_from_meshes_torch(jp, vp, jr, vr, lengths, scene)
    assert out["PA_MPJPE"].shape == (B, K) and out["SCENE_DIST_REF"].shape == (B,)
    want = pa_mpjpe_torch(jp[1, 2, :2], jr[1, :2]).mean() * 1000.0                # sequence 1 has two valid frames
    assert abs(float(out["PA_MPJPE"][1, 2]) - float(want)) <= 1e-12 * float(want)
    d2 = out["_d2"][1, 0, :2].numpy()
    assert abs(float(out["SCENE_DIST"][1, 0]) - np.sqrt(d2).mean() * 1000.0) <= 1e-9
    assert abs(float(out["CONTACT_RATIO"][1, 0]) - (d2 < 0.02).mean()) <= 1e-15
    assert set(mesh_metrics_from_meshes_torch(jp, vp, jr, vr, lengths)) == {"PA_MPJPE", "V2V"}


def test_frame_chunks_cover_the_valid_frames_once():
    from seeme_amd.mesh_metrics import frame_chunks
    for lengths, T, n in (([8, 5, 8], 8, 3), ([1], 4, 10), ([9, 0, 2], 6, 4), ([3, 3], 3, 6), ([3, 3], 3, 1)):
        chunks = frame_chunks(lengths, T, n)
        seen = [(b, t) for c in chunks for b, t0, t1 in c for t in range(t0, t1)]
        assert seen == [(b, t) for b, l in enumerate(lengths) for t in range(min(l, T))]
        assert all(0 < sum(t1 - t0 for _, t0, t1 in c) <= n for c in chunks)
        assert all(sum(t1 - t0 for _, t0, t1 in c) == n for c in chunks[:-1])


# ----------------------------------------------------------------------------- the accumulator
def test_mesh_metrics_accumulator_and_rank_reduction():
    from seeme_amd.mesh_metrics import MeshMetrics
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    mm = {"PA_MPJPE": f([[10., 20., 30.], [5., 7., 9.], [1., 2., 3.], [40., 50., 60.]]),
          "V2V": f([[3., 2., 1.], [8., 6., 4.], [9., 9., 9.], [2., 4., 6.]]),
          "CONTACT_RATIO": f([[1., 0., .5], [0., 0., 0.], [1., 1., 1.], [.25, .25, .5]]),
          "SCENE_DIST": f([[10., 30., 20.], [100., 100., 100.], [0., 0., 0.], [40., 40., 40.]]),
          "CONTACT_RATIO_REF": f([1., 0., 1., .5]), "SCENE_DIST_REF": f([10., 90., 0., 20.])}
    keep = torch.tensor([[True, True, False], [False, True, True], [False, False, False], [True, True, True]])
    acc = MeshMetrics()
    acc.update(mm, keep)
    got = acc.compute()
    assert set(got) == {"PA_MPJPE_best_of_k", "PA_MPJPE_mean_of_k", "V2V_best_of_k", "V2V_mean_of_k", "count_seq_mesh",
                        "CONTACT_RATIO", "SCENE_DIST", "CONTACT_RATIO_REF", "SCENE_DIST_REF"}
    assert got["count_seq_mesh"] == 3                                             # sequence 2 has no kept hypothesis
    assert got["PA_MPJPE_best_of_k"] == pytest.approx((10 + 7 + 40) / 3, rel=1e-12)
    assert got["PA_MPJPE_mean_of_k"] == pytest.approx((15 + 8 + 50) / 3, rel=1e-12)
    assert got["V2V_best_of_k"] == pytest.approx((2 + 4 + 2) / 3, rel=1e-12)      # its own best, not that of the PA winner
    assert got["V2V_mean_of_k"] == pytest.approx((2.5 + 5 + 4) / 3, rel=1e-12)
    assert got["CONTACT_RATIO"] == pytest.approx(5.5 / 12, rel=1e-12)             # all hypotheses, all sequences
    assert got["SCENE_DIST"] == pytest.approx(480 / 12, rel=1e-12)
    assert got["CONTACT_RATIO_REF"] == pytest.approx(2.5 / 4, rel=1e-12) and got["SCENE_DIST_REF"] == pytest.approx(30.0, rel=1e-12)
    # two ranks: sums() are added (seeme_amd.distributed.reduce_sums is a sum), the result is that of one update
    a, b = MeshMetrics(), MeshMetrics()
    a.update({k: v[:1] for k, v in mm.items()}, keep[:1])
    b.update({k: v[1:] for k, v in mm.items()}, keep[1:])
    assert a.sums().dtype == torch.float64 and a.sums().shape == (11,)
    two = a.compute(a.sums() + b.sums())
    for k, v in got.items():
        assert two[k] == pytest.approx(v, rel=1e-12), k
    from seeme_amd import distributed as D
    assert torch.equal(D.reduce_sums(a.sums().clone()), a.sums())                 # one rank: unchanged
    # no scene: no scene numbers; K = 1 takes [B,1]
    acc = MeshMetrics()
    acc.update({"PA_MPJPE": f([[4.], [6.]]), "V2V": f([[1.], [3.]])}, torch.tensor([[True], [True]]))
    got = acc.compute()
    assert set(got) == {"PA_MPJPE_best_of_k", "PA_MPJPE_mean_of_k", "V2V_best_of_k", "V2V_mean_of_k", "count_seq_mesh"}
    assert got["PA_MPJPE_best_of_k"] == 5.0 == got["PA_MPJPE_mean_of_k"] and got["V2V_best_of_k"] == 2.0
    assert MeshMetrics().compute()["count_seq_mesh"] == 0 and MeshMetrics().sums().shape == (11,)
    acc.reset()
    assert acc.compute()["PA_MPJPE_best_of_k"] == 0.0


# ----------------------------------------------------------------------------- the config key
def test_mesh_metrics_config_key_and_validation():
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    base = parse_config(os.path.join(REPO, "configs", "base.yaml"))
    assert base.TEST.MESH_METRICS is False and base.TEST.MESH_CHUNK_MB == 256
    path = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    smpl = SMPL.synthetic(1, V=64)
    m = MLD(parse_config(path), SyntheticEgoDataModule(), smpl_model=smpl)
    assert m.mesh_metrics is False and m.mesh_chunk_mb == 256 and m.MeshMetric.compute()["count_seq_mesh"] == 0
    for bad in (1, 0, "yes", None):
        cfg = parse_config(path)
        cfg.TEST.MESH_METRICS = bad
        with pytest.raises(ValueError, match="MESH_METRICS"):
            MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    for bad in (0, -1, "big", True):
        cfg = parse_config(path)
        cfg.TEST.MESH_CHUNK_MB = bad
        with pytest.raises(ValueError, match="MESH_CHUNK_MB"):
            MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    cfg = parse_config(path)
    cfg.TEST.MESH_METRICS = True
    assert MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl).mesh_metrics is True
    from seeme_amd import cli
    args = cli.build_parser("test").parse_args(["--cfg", path, "--mesh_metrics"])
    assert cli.load_cfg(args, "test").TEST.MESH_METRICS is True
    args = cli.build_parser("test").parse_args(["--cfg", path])
    assert cli.load_cfg(args, "test").TEST.MESH_METRICS is False


# ----------------------------------------------------------------------------- the C-ABI surface
def test_header_declares_and_library_exports_mesh_metrics():
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    declared = set(re.findall(r"\b(seeme_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in ("seeme_pa_mpjpe_frames", "seeme_mesh_v2v_frames", "seeme_scene_min_dist2", "seeme_scene_min_dist2_workspace_bytes"):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name)
    err = lambda: lib.seeme_last_error()
    # argument checks come before any device work: they hold without a GPU
    assert lib.seeme_pa_mpjpe_frames(16, 16, 16, 0, 16, 0) != 0 and b"F must" in err()
    assert lib.seeme_pa_mpjpe_frames(0, 16, 16, 4, 16, 0) != 0 and b"null" in err()
    assert lib.seeme_mesh_v2v_frames(16, 16, 16, 16, 16, 0, 5, 16, 0) != 0 and b"F must" in err()
    assert lib.seeme_mesh_v2v_frames(16, 16, 16, 16, 16, 2, 0, 16, 0) != 0 and b"V must" in err()
    assert lib.seeme_mesh_v2v_frames(16, 16, 16, 0, 16, 2, 5, 16, 0) != 0 and b"null" in err()
    assert lib.seeme_mesh_v2v_frames(20, 16, 16, 16, 16, 2, 5, 16, 0) != 0 and b"aligned" in err()
    assert lib.seeme_mesh_v2v_frames(16, 16, 24, 16, 16, 2, 5, 16, 0) != 0 and b"aligned" in err()
    need = lib.seeme_scene_min_dist2_workspace_bytes(3, 6890, 2, 20000)
    assert need >= 3 * 20000 * 4 and lib.seeme_scene_min_dist2_workspace_bytes(40320, 6890, 32, 20000) >= 40320 * 20000 * 4
    for bad in ((0, 6890, 2, 20000), (3, 0, 2, 20000), (3, 6890, 0, 20000), (3, 6890, 2, 0), (3, 20000, 2, 20000)):
        assert lib.seeme_scene_min_dist2_workspace_bytes(*bad) == 0, bad
    assert lib.seeme_scene_min_dist2(16, 16, 16, 0, 37, 2, 9, 16, 16, 1 << 20, 0) != 0 and b"F must" in err()
    assert lib.seeme_scene_min_dist2(16, 16, 16, 3, 0, 2, 9, 16, 16, 1 << 20, 0) != 0 and b"V must" in err()
    assert lib.seeme_scene_min_dist2(16, 16, 16, 3, 37, 0, 9, 16, 16, 1 << 20, 0) != 0 and b"S must" in err()
    assert lib.seeme_scene_min_dist2(16, 16, 16, 3, 37, 2, 0, 16, 16, 1 << 20, 0) != 0 and b"P must" in err()
    assert lib.seeme_scene_min_dist2(16, 0, 16, 3, 37, 2, 9, 16, 16, 1 << 20, 0) != 0 and b"null" in err()
    assert lib.seeme_scene_min_dist2(16, 16, 16, 3, 37, 2, 9, 16, 0, 1 << 20, 0) != 0 and b"null" in err()
    assert lib.seeme_scene_min_dist2(16, 16, 16, 3, 37, 2, 9, 16, 20, 1 << 20, 0) != 0 and b"aligned" in err()
    small = lib.seeme_scene_min_dist2_workspace_bytes(3, 37, 2, 9)
    assert small > 0
    assert lib.seeme_scene_min_dist2(16, 16, 16, 3, 37, 2, 9, 16, 16, small - 1, 0) != 0 and b"workspace too small" in err()


# ----------------------------------------------------------------------------- the driver's bookkeeping (primitives replaced by the twins)
def test_driver_bookkeeping_with_the_twins_in_place_of_the_kernels(monkeypatch):
    """Which frame goes where: the driver on the CPU with the three primitives replaced by their twins and a linear 'pose' function
    gives what the twins give on resident meshes, whatever the chunk size, with ragged lengths, with and without a scene."""
    from seeme_amd import mesh_metrics as M
    monkeypatch.setattr(M, "pa_mpjpe_hip", M.pa_mpjpe_torch)
    monkeypatch.setattr(M, "v2v_hip", M.v2v_torch)
    monkeypatch.setattr(M, "scene_min_dist2_hip", M.scene_min_dist2_torch)
    g = torch.Generator().manual_seed(8)
    B, K, T, F, V, P = 3, 2, 5, 6, 9, 7
    Wj, Wv = torch.randn(F + 10 + 3, 24 * 3, generator=g), torch.randn(F + 10 + 3, V * 3, generator=g)
    calls = []

    def pose(feats, betas, orient):
        calls.append(feats.shape[1])
        x = torch.cat([feats, betas, torch.zeros_like(feats[..., :3]) if orient is None else orient], dim=-1)
        return (x @ Wj).reshape(1, -1, 24, 3), (x @ Wv).reshape(1, -1, V, 3)

    f_rst, f_ref = torch.randn(B * K, T, F, generator=g), torch.randn(B, T, F, generator=g)
    betas, orient, scene = torch.randn(B, T, 10, generator=g), torch.randn(B, T, 3, generator=g), torch.randn(B, P, 3, generator=g)
    lengths = [5, 2, 4]
    for o in (None, orient):
        rep = lambda t: t.repeat_interleave(K, dim=0)
        jp, vp = pose(f_rst.reshape(1, -1, F), rep(betas).reshape(1, -1, 10), None if o is None else rep(o).reshape(1, -1, 3))
        jr, vr = pose(f_ref.reshape(1, -1, F), betas.reshape(1, -1, 10), None if o is None else o.reshape(1, -1, 3))
        for sc in (None, scene):
            want = M.mesh_metrics_from_meshes_torch(jp.reshape(B, K, T, 24, 3), vp.reshape(B, K, T, V, 3), jr.reshape(B, T, 24, 3),
                                                    vr.reshape(B, T, V, 3), lengths, sc)
            first = None
            for mb in (1e-3, 3 * (K + 1) * V * 12 / (1 << 20), 256):          # one frame per chunk, three, everything
                del calls[:]
                got = M.mesh_metrics_eval(pose, f_rst, f_ref, betas, o, lengths, K, scene=sc, chunk_mb=mb, num_vertices=V)
                assert sum(calls) == (K + 1) * sum(lengths) and max(calls) <= (K + 1) * max(1, int(mb * (1 << 20)) // ((K + 1) * V * 12))
                assert set(got) == {k for k in want if not k.startswith("_")}
                for k, v in got.items():
                    assert v.shape == want[k].shape and torch.allclose(v, want[k].float(), rtol=1e-5, atol=1e-6), (k, mb)
                    assert first is None or torch.equal(v, first[k]), (k, mb)
                first = first or got
