"""The point-in-mesh test without a GPU: uv_sphere and check_closed_faces, the winding-number twin in float64 on shapes whose answer is
known, the counting twin, the driver's bookkeeping and the accumulator through the twins, the config switch and the C-ABI surface."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

AXES = torch.tensor([0.25, 0.6, 0.15], dtype=torch.float64)          # semi-axes of the test body, metres
TETRA_V = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
TETRA_F = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def _ellipsoid(rings, segments, offset):
    from seeme_amd.mesh_metrics import uv_sphere
    v, f = uv_sphere(rings, segments)
    return (v * AXES + torch.tensor(offset, dtype=torch.float64)).float().double(), f          # values rounded to fp32


def _box_points(verts, n, seed):
    """n points uniform in the bounding box of verts [V,3], rounded to fp32."""
    lo, hi = verts.min(dim=0).values, verts.max(dim=0).values
    u = torch.from_numpy(np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)))
    return (lo + u * (hi - lo)).float().double()


# ----------------------------------------------------------------------------- uv_sphere, check_closed_faces
@pytest.mark.parametrize("rings,segments,V,NF", [(84, 82, 6890, 13776), (5, 7, 37, 70)])
def test_uv_sphere_counts_and_closedness(rings, segments, V, NF):
    from seeme_amd.mesh_metrics import check_closed_faces, uv_sphere
    v, f = uv_sphere(rings, segments)
    assert v.shape == (V, 3) and f.shape == (NF, 3) and f.dtype == torch.long
    assert torch.allclose(v.norm(dim=1), torch.ones(V, dtype=v.dtype))
    assert int(f.min()) == 0 and int(f.max()) == V - 1 and len(set(f.flatten().tolist())) == V
    check_closed_faces(f, V)
    with pytest.raises(ValueError, match="not closed"):
        check_closed_faces(torch.cat([f[:3], f[4:]]), V)
    with pytest.raises(ValueError, match="consistently oriented"):
        check_closed_faces(torch.cat([f[:3], f[3:4].flip(1), f[4:]]), V)
    with pytest.raises(ValueError, match="indices run"):
        check_closed_faces(f, V - 1)


def test_check_closed_faces_names_the_all_zero_table():
    from seeme_amd.mesh_metrics import check_closed_faces
    from seeme_amd.smpl import SMPL
    with pytest.raises(ValueError, match="all zeros"):
        check_closed_faces(SMPL.synthetic(1, V=64).faces_tensor, 64)
    check_closed_faces(TETRA_F, 4)


# ----------------------------------------------------------------------------- winding_number_torch in float64
def test_winding_tetrahedron_ellipsoid_overlap_and_flip():
    from seeme_amd.mesh_metrics import winding_number_torch
    pts = torch.tensor([[[0.2, 0.2, 0.2], [1.0, 1.0, 1.0]]], dtype=torch.float64)
    w = winding_number_torch(TETRA_V[None], TETRA_F, pts)
    assert w.shape == (1, 2) and abs(float(w[0, 0]) - 1.0) <= 1e-12 and abs(float(w[0, 1])) <= 1e-12
    # the (5, 7) ellipsoid at metre coordinates: w is an integer for every point of its box
    v, f = _ellipsoid(5, 7, (1.5, 0.9, -2.0))
    p = _box_points(v, 250, 1)
    w = winding_number_torch(v[None], f, p[None])[0]
    assert float((w - w.round()).abs().max()) <= 1e-9 and set(w.round().long().tolist()) == {0, 1}
    n_in = int((w.abs() >= 0.5).sum())
    assert 80 <= n_in <= 140                      # the inscribed polyhedron fills a little less of the box than pi / 6
    # chunking over the points changes nothing
    assert torch.equal(winding_number_torch(v[None], f, p[None], chunk=7)[0].round(), w.round())
    assert float((winding_number_torch(v[None], f, p[None], chunk=7)[0] - w).abs().max()) <= 1e-12
    # two overlapping copies in ONE mesh: w in {0, 1, 2}, all three present
    v2 = torch.cat([v, v + torch.tensor([0.2, 0.0, 0.0], dtype=torch.float64)])
    f2 = torch.cat([f, f + v.shape[0]])
    p2 = _box_points(v2, 400, 2)
    w2 = winding_number_torch(v2[None], f2, p2[None])[0]
    assert float((w2 - w2.round()).abs().max()) <= 1e-9 and set(w2.round().long().tolist()) == {0, 1, 2}
    # a flipped table flips the sign
    wf = winding_number_torch(v[None], f.flip(1), p[None])[0]
    assert float((wf + w).abs().max()) <= 1e-12 and set(wf.round().long().tolist()) == {0, -1}
    # faces with two equal indices or an index out of range contribute nothing
    junk = torch.tensor([[0, 0, 0], [3, 3, 5], [1, 2, 99], [-1, 2, 3]])
    assert torch.equal(winding_number_torch(v[None], torch.cat([f, junk]), p[None])[0], w)


def test_winding_is_finite_on_a_vertex_and_maps_frames_to_clouds():
    from seeme_amd.mesh_metrics import winding_number_torch
    v, f = _ellipsoid(5, 7, (0.0, 1.0, 0.0))
    for dt in (torch.float64, torch.float32):
        on_vertex = torch.stack([v[0], v[11], 0.5 * (v[1] + v[2])])[None].to(dt)
        assert torch.isfinite(winding_number_torch(v[None].to(dt), f, on_vertex)).all()
    # F = 3, frame 1 skipped, two clouds
    verts = torch.stack([v, v + 5.0, v + torch.tensor([-2.0, 0.0, 1.0], dtype=torch.float64)])
    clouds = torch.stack([_box_points(verts[2], 40, 3), _box_points(verts[0], 40, 4)])
    w = winding_number_torch(verts, f, clouds, [1, -1, 0])
    assert w.shape == (3, 40) and bool((w[1] == 0).all())
    assert torch.equal(w[0], winding_number_torch(verts[0:1], f, clouds[1:2])[0])
    assert torch.equal(w[2], winding_number_torch(verts[2:3], f, clouds[0:1])[0])
    assert 0 < int((w[0].abs() >= 0.5).sum()) < 40
    # without a map frame f uses cloud f
    assert torch.equal(winding_number_torch(verts[:2], f, clouds)[0], winding_number_torch(verts[0:1], f, clouds[0:1])[0])


# ----------------------------------------------------------------------------- scene_inside_count_torch
def test_inside_count_equals_the_unfiltered_classification():
    from seeme_amd.mesh_metrics import scene_inside_count_torch, winding_number_torch
    v, f = _ellipsoid(5, 7, (1.5, 0.9, -2.0))
    verts = torch.stack([v, v + 3.0, v + torch.tensor([-3.7, 0.2, 3.4], dtype=torch.float64)])
    g = torch.Generator().manual_seed(5)
    room = lambda n: (torch.rand(n, 3, generator=g, dtype=torch.float64) * torch.tensor([8.0, 3.0, 8.0]) - torch.tensor([4.0, 0.0, 4.0])).float().double()
    clouds = torch.stack([torch.cat([room(150), _box_points(verts[2], 60, 6)]), torch.cat([room(150), _box_points(verts[0], 60, 7)])])
    sof = [1, -1, 0]
    cnt = scene_inside_count_torch(verts, f, clouds, sof)
    assert cnt.dtype == torch.int32 and cnt.shape == (3,)
    w = winding_number_torch(verts, f, clouds, sof)                           # every point, no prefilter
    assert torch.equal(cnt.long(), (w.abs() >= 0.5).sum(dim=1))
    assert int(cnt[1]) == 0 and 10 <= int(cnt[0]) <= 50 and 10 <= int(cnt[2]) <= 50
    # frames map to their scenes: the other cloud's box points are nowhere near
    assert int(scene_inside_count_torch(verts[0:1], f, clouds, [0])[0]) <= 2
    assert torch.equal(scene_inside_count_torch(verts[:2], f, clouds)[0], scene_inside_count_torch(verts[0:1], f, clouds[0:1])[0])
    # fp32 classifies these points like float64, and a flipped table counts the same
    assert torch.equal(scene_inside_count_torch(verts.float(), f, clouds.float(), sof), cnt)
    assert torch.equal(scene_inside_count_torch(verts, f.flip(1), clouds, sof), cnt)


# ----------------------------------------------------------------------------- the driver and the accumulator through the twins
def test_driver_adds_the_collision_keys_and_leaves_the_others_alone(monkeypatch):
    from seeme_amd import mesh_metrics as M
    monkeypatch.setattr(M, "pa_mpjpe_hip", M.pa_mpjpe_torch)
    monkeypatch.setattr(M, "v2v_hip", M.v2v_torch)
    monkeypatch.setattr(M, "scene_min_dist2_hip", M.scene_min_dist2_torch)
    monkeypatch.setattr(M, "scene_inside_count_hip", M.scene_inside_count_torch)
    sv, sf = M.uv_sphere(3, 5)
    V = sv.shape[0]
    g = torch.Generator().manual_seed(8)
    B, K, T, F, P = 3, 2, 5, 6, 40
    Wj = torch.randn(F + 10, 24 * 3, generator=g)
    calls = []

    def pose(feats, betas, orient):
        """A rigidly moved, scaled sphere: centre and radius are linear in the features."""
        calls.append(feats.shape[1])
        x = torch.cat([feats, betas], dim=-1)
        c, r = feats[0, :, :3], 0.3 + 0.05 * feats[0, :, 3:4].abs()
        return (x @ Wj).reshape(1, -1, 24, 3), (c[:, None, :] + r[:, None, :] * sv.float()[None])[None]

    f_rst, f_ref = torch.randn(B * K, T, F, generator=g), torch.randn(B, T, F, generator=g)
    betas = torch.randn(B, T, 10, generator=g)
    scene = 1.2 * torch.randn(B, P, 3, generator=g)
    lengths = [5, 2, 4]
    rep = lambda t: t.repeat_interleave(K, dim=0)
    _, vp = pose(f_rst.reshape(1, -1, F), rep(betas).reshape(1, -1, 10), None)
    _, vr = pose(f_ref.reshape(1, -1, F), betas.reshape(1, -1, 10), None)
    want = M.collision_from_meshes_torch(vp.reshape(B, K, T, V, 3), vr.reshape(B, T, V, 3), sf, lengths, scene)
    assert int(want["_count"].sum()) > 0 and int((want["_count"] == 0).sum()) > 0
    plain = M.mesh_metrics_eval(pose, f_rst, f_ref, betas, None, lengths, K, scene=scene, num_vertices=V)
    assert set(plain) == {"PA_MPJPE", "V2V", "SCENE_DIST", "CONTACT_RATIO", "SCENE_DIST_REF", "CONTACT_RATIO_REF"}
    names = set(M.COLLISION_HYP + M.COLLISION_REF)
    for mb in (1e-3, 3 * (K + 1) * V * 12 / (1 << 20), 256):
        del calls[:]
        both = M.mesh_metrics_eval(pose, f_rst, f_ref, betas, None, lengths, K, scene=scene, chunk_mb=mb, num_vertices=V, faces=sf)
        assert sum(calls) == (K + 1) * sum(lengths)                               # every frame posed once
        assert set(both) == set(plain) | names
        for k in plain:
            assert torch.equal(both[k], plain[k]), k
        only = M.mesh_metrics_eval(pose, f_rst, f_ref, betas, None, lengths, K, scene=scene, chunk_mb=mb, num_vertices=V, faces=sf,
                                   mesh=False)
        assert set(only) == names
        for k in names:
            assert both[k].dtype == torch.float32 and both[k].shape == ((B,) if k.endswith("_REF") else (B, K))
            assert torch.equal(both[k], want[k]) and torch.equal(only[k], want[k]), (k, mb)
    # no scene, or no faces: no collision keys
    assert set(M.mesh_metrics_eval(pose, f_rst, f_ref, betas, None, lengths, K, num_vertices=V, faces=sf)) == {"PA_MPJPE", "V2V"}
    # the numbers by hand for one sequence
    b, k = 2, 1
    c = want["_count"][b, k, :lengths[b]].double()
    assert float(want["COLLISION_RATIO"][b, k]) == pytest.approx(float((c / P).mean()), rel=1e-6)
    assert float(want["COLLISION_FRAMES"][b, k]) == pytest.approx(float((c > 0).double().mean()), rel=1e-6)
    assert int(want["_count"][1, :, 2:].sum()) == 0                                # frames past a length are not counted


def test_collision_accumulator_sums_and_compute():
    from seeme_amd.mesh_metrics import CollisionMetrics
    acc = CollisionMetrics()
    assert acc.compute() == {} and acc.sums().shape == (6,) and acc.sums().dtype == torch.float64
    a = {"COLLISION_RATIO": torch.tensor([[0.1, 0.3], [0.0, 0.2]]), "COLLISION_FRAMES": torch.tensor([[1.0, 0.5], [0.0, 0.5]]),
         "COLLISION_RATIO_REF": torch.tensor([0.05, 0.15]), "COLLISION_FRAMES_REF": torch.tensor([0.25, 0.75])}
    b = {"COLLISION_RATIO": torch.tensor([[0.4, 0.0]]), "COLLISION_FRAMES": torch.tensor([[1.0, 0.0]]),
         "COLLISION_RATIO_REF": torch.tensor([0.1]), "COLLISION_FRAMES_REF": torch.tensor([1.0])}
    acc.update(a)
    acc.update(b)
    s = acc.sums()
    assert s.dtype == torch.float64
    np.testing.assert_allclose(s.numpy(), [1.0, 3.0, 6.0, 0.3, 2.0, 3.0], rtol=1e-6)
    got = acc.compute()
    assert set(got) == set(CollisionMetrics.NAMES)
    assert got["COLLISION_RATIO"] == pytest.approx(1.0 / 6) and got["COLLISION_FRAMES"] == pytest.approx(0.5)
    assert got["COLLISION_RATIO_REF"] == pytest.approx(0.1) and got["COLLISION_FRAMES_REF"] == pytest.approx(2.0 / 3)
    # two ranks' sums added give the numbers of the union
    other = CollisionMetrics()
    other.update(b)
    assert acc.compute(acc.sums() + other.sums())["COLLISION_RATIO"] == pytest.approx(1.4 / 8)
    acc.reset()
    assert acc.compute() == {}


# ----------------------------------------------------------------------------- the config switch
def _sphere_smpl(rings=5, segments=7):
    from seeme_amd.mesh_metrics import uv_sphere
    from seeme_amd.smpl import SMPL, synthetic_model_arrays
    v, f = uv_sphere(rings, segments)
    arrays = synthetic_model_arrays(1, V=v.shape[0])
    arrays["v_template"] = (v * AXES).float().numpy()
    arrays["faces"] = f.numpy()
    return SMPL(model_arrays=arrays)


def test_collision_switch_validation_in_mld_and_cli():
    from seeme_amd import cli
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    base = parse_config(os.path.join(REPO, "configs", "base.yaml"))
    assert base.TEST.COLLISION_METRICS is False
    scene_cfg = os.path.join(REPO, "configs", "config_mld_scene.yaml")
    plain_cfg = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    smpl = _sphere_smpl()
    m = MLD(parse_config(scene_cfg), SyntheticEgoDataModule(), smpl_model=SMPL.synthetic(1, V=64))
    assert m.collision_metrics is False and m.CollMetric.compute() == {}             # off: an open table is nobody's business
    for bad in (1, 0, "yes", None):
        cfg = parse_config(scene_cfg)
        cfg.TEST.COLLISION_METRICS = bad
        with pytest.raises(ValueError, match="COLLISION_METRICS"):
            MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    cfg = parse_config(plain_cfg)                                                    # no 'scene' in the condition
    assert "scene" not in cfg.model.condition
    cfg.TEST.COLLISION_METRICS = True
    with pytest.raises(ValueError, match="no 'scene'"):
        MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    cfg = parse_config(scene_cfg)                                                    # an open (all-zero) face table
    cfg.TEST.COLLISION_METRICS = True
    with pytest.raises(ValueError, match="all zeros"):
        MLD(cfg, SyntheticEgoDataModule(), smpl_model=SMPL.synthetic(1, V=64))
    on = MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    assert on.collision_metrics is True and on.mesh_metrics is False                 # independent switches
    cfg.TEST.MESH_METRICS = True
    both = MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    assert both.collision_metrics is True and both.mesh_metrics is True
    args = cli.build_parser("test").parse_args(["--cfg", scene_cfg, "--collision_metrics"])
    c = cli.load_cfg(args, "test")
    assert c.TEST.COLLISION_METRICS is True and c.TEST.MESH_METRICS is False
    args = cli.build_parser("test").parse_args(["--cfg", scene_cfg, "--mesh_metrics"])
    assert cli.load_cfg(args, "test").TEST.COLLISION_METRICS is False


# ----------------------------------------------------------------------------- the C-ABI surface
def test_header_ctypes_table_and_library_agree_on_the_collision_entry_points():
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    declared = set(re.findall(r"\b(seeme_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in ("seeme_scene_inside_count", "seeme_scene_inside_count_workspace_bytes", "seeme_mesh_winding"):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name)
        proto = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name
    err = lambda: lib.seeme_last_error()
    ws = lib.seeme_scene_inside_count_workspace_bytes
    assert ws(3, 6890, 2, 20000) >= 3 * 4 and ws(40320, 6890, 32, 20000) >= 40320 * 4
    for bad in ((0, 6890, 2, 20000), (3, 0, 2, 20000), (3, 6890, 0, 20000), (3, 6890, 2, 0), (3, 10113, 2, 20000)):
        assert ws(*bad) == 0, bad
    assert ws(3, 10112, 2, 20000) > 0
    # argument checks come before any device work: they hold without a GPU
    cnt = lambda **k: lib.seeme_scene_inside_count(*[{**dict(verts=16, faces=16, NF=4, scene=16, sof=16, F=3, V=37, S=2, P=9, out=16, ws=16,
                                                              wsb=1 << 20, st=0), **k}[n]
                                                     for n in ("verts", "faces", "NF", "scene", "sof", "F", "V", "S", "P", "out", "ws", "wsb", "st")])
    for kw, msg in ((dict(F=0), b"F must"), (dict(V=0), b"V must"), (dict(V=10113), b"V must"), (dict(NF=0), b"NF must"),
                    (dict(S=0), b"S must"), (dict(P=0), b"P must"), (dict(faces=0), b"null"), (dict(ws=0), b"null"),
                    (dict(ws=20), b"aligned"), (dict(wsb=ws(3, 37, 2, 9) - 1), b"workspace too small")):
        assert cnt(**kw) != 0 and msg in err() and b"scene_inside_count" in err(), kw
    assert lib.seeme_mesh_winding(16, 16, 4, 16, 16, 0, 37, 2, 9, 16, 0) != 0 and b"F must" in err()
    assert lib.seeme_mesh_winding(16, 16, 4, 16, 16, 3, 10113, 2, 9, 16, 0) != 0 and b"V must" in err()
    assert lib.seeme_mesh_winding(16, 16, 4, 16, 16, 3, 37, 2, 9, 0, 0) != 0 and b"null" in err() and b"mesh_winding" in err()
