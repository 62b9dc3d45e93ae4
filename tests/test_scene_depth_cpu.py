"""The body-scene term on the CPU: the plain-torch twin of seeme_scene_depth in float64 against the explicit loops of
tests/scene_depth_reference.py, hand cases, the capsule table of recording.body_capsules against an independent restatement and on
hand-made templates, the validation of arguments and configuration keys, and the C-ABI of the entry point."""
import os
import types

import numpy as np
import pytest
import torch

import scene_depth_reference as SREF
from seeme_amd import recording as R

TWIN_TOL = 1e-12             # float64 twin against float64 loops, relative to the largest reference value
CASES = [(1, 1, 1, 24, 1, 1), (2, 3, 2, 24, 63, 21), (1, 2, 9, 5, 64, 3), (3, 2, 7, 24, 65, 32), (2, 2, 5, 32, 257, 33)]


def _t(a):
    return torch.from_numpy(np.array(a))


# ----------------------------------------------------------------------------- the twin against the loops
@pytest.mark.parametrize("case", CASES, ids=str)
def test_scene_depth_twin_vs_float64_loops(case):
    jts, lengths, points, segs, radius = SREF.inputs(*case)
    want = SREF.reference(*case)
    got = R.scene_depth_torch(_t(jts).double(), list(lengths), _t(points).double(), segs, radius)
    assert got["depth"].dtype == got["cost"].dtype == torch.float64 and got["hits"].dtype == torch.int32
    for k in ("depth", "cost"):
        assert got[k].shape == want[k].shape
        assert float(np.abs(got[k].numpy() - want[k]).max()) <= TWIN_TOL * max(float(np.abs(want[k]).max()), 1e-300), k
    assert SREF.near_zero(want["raw"]) == 0 and np.array_equal(got["hits"].numpy(), want["hits"])
    W, K, T = case[:3]
    if case[4] >= 63:
        assert want["hits"].sum() > 0                                  # the inputs do penetrate
    for w, n in enumerate(lengths):
        assert float(got["depth"][w, :, n:].abs().max() if n < T else 0.0) == 0.0
        if n == 0:
            assert float(got["cost"][w].abs().max()) == 0.0 and int(got["hits"][w].abs().max()) == 0
    # chunking over the points changes nothing, a tensor of lengths is read like a list, float32 is served
    small = R.scene_depth_torch(_t(jts).double(), torch.tensor(lengths), _t(points).double(), _t(segs), _t(radius), max_elems=1)
    assert all(torch.equal(small[k], got[k]) for k in got)
    f32 = R.scene_depth_torch(_t(jts), list(lengths), _t(points), segs, radius)
    assert f32["depth"].dtype == torch.float32 and float((f32["depth"].double() - got["depth"]).abs().max()) <= 5e-3
    full = np.nan_to_num(jts)                                          # a length above T is T
    assert torch.equal(R.scene_depth_torch(_t(full), [T + 5] * W, _t(points), segs, radius)["depth"],
                       R.scene_depth_torch(_t(full), [T] * W, _t(points), segs, radius)["depth"])


def test_scene_depth_hand_cases():
    f8 = torch.float64
    jts = torch.zeros(1, 1, 2, 3, 3, dtype=f8)
    jts[0, 0, :, 1] = torch.tensor([1.0, 0.0, 0.0], dtype=f8)          # joint 1 one metre along x; joint 2 = joint 0 (coincident)
    segs, radius = [[0, 1], [2, 2], [0, 2]], [0.05, 0.02, 0.01]
    on = torch.tensor([[0.25, 0.0, 0.0]], dtype=f8)                    # a point on the segment: depth = 1000 x radius
    out = R.scene_depth_torch(jts, [2], on, segs, radius)
    assert torch.equal(out["depth"], torch.full((1, 1, 2), 50.0, dtype=f8)) and float(out["cost"]) == 50.0 and int(out["hits"]) == 2
    assert np.array_equal(SREF.scene_depth(jts.numpy(), [2], on.numpy(), segs, radius)["depth"], out["depth"].numpy())
    off = torch.tensor([[0.25, 0.03, 0.0], [2.0, 0.0, 0.04], [-0.03, 0.0, 0.0]], dtype=f8)
    out = R.scene_depth_torch(jts, [1], off[:1], segs, radius)         # beside the segment: radius minus the distance
    assert abs(float(out["depth"][0, 0, 0]) - 20.0) <= 1e-12 and float(out["depth"][0, 0, 1]) == 0.0 and int(out["hits"]) == 1
    assert abs(float(out["cost"]) - 20.0) <= 1e-12                     # the mean over the window's ONE frame
    assert float(R.scene_depth_torch(jts, [2], off[1:2], segs, radius)["depth"].abs().max()) == 0.0   # past the end c: out of reach
    out = R.scene_depth_torch(jts, [2], off[2:], segs, radius)         # before a: the end's sphere, 50 - 30 mm
    assert abs(float(out["depth"][0, 0, 0]) - 20.0) <= 1e-12
    # a sphere segment is a sphere, and coincident joints give no NaN
    sph = R.scene_depth_torch(jts, [2], torch.tensor([[0.0, 0.012, 0.0], [0.0, 0.0, 0.5]], dtype=f8), [[2, 2], [0, 2]], [0.02, 0.01])
    assert torch.isfinite(sph["depth"]).all() and abs(float(sph["depth"][0, 0, 0]) - 8.0) <= 1e-12
    ref = SREF.scene_depth(jts.numpy(), [2], np.array([[0.0, 0.012, 0.0], [0.0, 0.0, 0.5]]), [[2, 2], [0, 2]], [0.02, 0.01])
    assert abs(ref["depth"][0, 0, 0] - 8.0) <= 1e-12 and np.isfinite(ref["depth"]).all()
    # n = 0: zeros, whatever the frames hold
    nan = torch.full_like(jts, float("nan"))
    z = R.scene_depth_torch(nan, [0], on, segs, radius)
    assert float(z["depth"].abs().max()) == 0.0 and float(z["cost"]) == 0.0 and int(z["hits"]) == 0
    # NaN points are ignored; a cloud of nothing but NaN gives zeros
    mixed = torch.cat([torch.full((2, 3), float("nan"), dtype=f8), on, torch.tensor([[float("nan"), 0.0, 0.0]], dtype=f8)])
    assert torch.equal(R.scene_depth_torch(jts, [2], mixed, segs, radius)["depth"], torch.full((1, 1, 2), 50.0, dtype=f8))
    assert float(R.scene_depth_torch(jts, [2], mixed[:2], segs, radius)["depth"].abs().max()) == 0.0
    assert float(SREF.scene_depth(jts.numpy(), [2], mixed[:2].numpy(), segs, radius)["depth"].max()) == 0.0
    # a radius of 0 never penetrates, not even with the point on the segment
    assert float(R.scene_depth_torch(jts, [2], on, [[0, 1]], [0.0])["depth"].abs().max()) == 0.0


def test_scene_depth_argument_validation():
    jts, lengths, points, segs, radius = SREF.inputs(2, 2, 3, 24, 7, 3)
    j, p = _t(jts).double(), _t(points).double()
    good = (j, list(lengths), p, segs, radius)
    R.scene_depth_torch(*good)
    for i, bad in ((0, j[..., :2]), (0, j[0]), (0, j.long()), (0, jts), (2, p.float()), (2, p[:, :2]), (2, p[:0]), (2, points),
                   (1, [3]), (1, [3, 2.5]), (1, [3, True]),
                   (3, segs[:, :1]), (3, segs.astype(np.float32)), (3, segs[:0]), (3, np.array([[0, 24], [1, 2], [3, 4]])),
                   (3, np.array([[0, -1], [1, 2], [3, 4]])),
                   (4, radius[:2]), (4, np.array([0.1, -0.1, 0.1])), (4, np.array([0.1, np.nan, 0.1])), (4, np.array([0.1, np.inf, 0.1])),
                   (4, ["a", "b", "c"])):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError, match="scene_depth"):
            R.scene_depth_torch(*args)
    with pytest.raises(ValueError, match="float32"):                   # the kernel's wrapper: fp32 only, then the device
        R.scene_depth_hip(*good)
    from seeme_amd import _lib
    with pytest.raises(_lib.SeemeError):
        R.scene_depth_hip(_t(jts), list(lengths), _t(points), segs, radius)


# ----------------------------------------------------------------------------- the capsule table
def _capsules_restated(v, jt, segs, quantile):
    """Vertex by vertex, the three cases, a strict < so that the lowest b keeps a tie, numpy's own lower quantile."""
    own, dist = [], []
    for p in v:
        best, which = np.inf, -1
        for b, (i0, i1) in enumerate(segs):
            a, c = jt[i0], jt[i1]
            e = c - a
            u, ee = float((p - a) @ e), float(e @ e)
            d = np.linalg.norm(p - a) if u <= 0 else np.linalg.norm(p - c) if u >= ee else np.linalg.norm(p - (a + (u / ee) * e))
            if d < best:
                best, which = d, b
        own.append(which)
        dist.append(best)
    own, dist = np.array(own), np.array(dist)
    return np.array([np.quantile(dist[own == b], quantile, method="lower") if (own == b).any() else 0.0 for b in range(len(segs))])


def test_body_capsules_vs_restatement_on_the_test_model():
    from seeme_amd.smpl import SMPL, SMPL_PARENTS
    smpl = SMPL.synthetic(1234, V=500)
    betas = np.linspace(-1.0, 1.0, 10)
    want_segs = [(SMPL_PARENTS[j], j) for j in range(1, 24) if j not in (10, 11)]
    for b, q in ((None, 0.5), (betas, 0.5), (torch.from_numpy(betas).float(), 0.9), (None, 0.0), (None, 1.0)):
        segs, radius = R.body_capsules(smpl, b, q)
        assert segs.dtype == np.int32 and radius.dtype == np.float32 and segs.shape == (21, 2) and radius.shape == (21,)
        assert segs.tolist() == [list(s) for s in want_segs] and not ({10, 11} & set(segs[:, 1].tolist()))
        v = smpl.v_template.double().numpy()
        if b is not None:
            v = v + smpl.shapedirs.double().numpy() @ np.asarray(torch.as_tensor(b).double().numpy())
        want = _capsules_restated(v, smpl.J_regressor.double().numpy() @ v, want_segs, q)
        assert float(np.abs(radius.astype(np.float64) - want).max()) <= 1e-7 * max(float(want.max()), 1e-30), (q, radius, want)
    custom = [(0, 1), (4, 4), (7, 2)]
    segs, radius = R.body_capsules(smpl, None, 0.25, segs=custom)
    v = smpl.v_template.double().numpy()
    want = _capsules_restated(v, smpl.J_regressor.double().numpy() @ v, custom, 0.25)
    assert segs.tolist() == [list(s) for s in custom] and float(np.abs(radius - want).max()) <= 1e-7 * float(want.max())
    for kw in (dict(quantile=1.5), dict(quantile=-0.1), dict(quantile="half"), dict(quantile=True), dict(segs=[(0, 24)]),
               dict(segs=[(0, 1, 2)]), dict(segs=[]), dict(segs=[(0.5, 1.0)]), dict(betas=np.zeros(9))):
        with pytest.raises(ValueError, match="body_capsules"):
            R.body_capsules(smpl, **kw)


def _ring_template(rho, heights=(0.0, 0.25, 0.5, 0.75, 1.0)):
    """Rings of four vertices at distance rho round the y axis; joint 0 is the centre of the first ring, joint 1 that of the last
    (sums of +-rho: exact), joint 2 the centre of the middle one."""
    v = np.array([[sx * rho, y, sz * rho] for y in heights for sx, sz in ((1, 0), (-1, 0), (0, 1), (0, -1))], np.float64)
    Jr = np.zeros((3, v.shape[0]))
    Jr[0, :4], Jr[1, -4:], Jr[2, 8:12] = 0.25, 0.25, 0.25
    return types.SimpleNamespace(v_template=torch.from_numpy(v), shapedirs=torch.zeros(v.shape[0], 3, 10, dtype=torch.float64),
                                 J_regressor=torch.from_numpy(Jr), parents=torch.tensor([-1, 0, 0]))


def test_body_capsules_on_hand_made_templates():
    rho = 0.125
    tpl = _ring_template(rho)
    for q in (0.0, 0.5, 1.0):                                          # every vertex lies on the cylinder of radius rho round 0 -> 1
        segs, radius = R.body_capsules(tpl, None, q, segs=[(0, 1)])
        assert radius.tolist() == [rho]
    # the tie rule and the empty segment: the first ring is rho from the segment 0 -> 1 AND from the sphere at joint 0; the lowest b
    # takes it.  Behind the segment the sphere gets nothing: radius 0.  In front of it the sphere takes the first ring.
    _, radius = R.body_capsules(tpl, None, 0.5, segs=[(0, 1), (0, 0)])
    assert radius.tolist() == [rho, 0.0]
    _, radius = R.body_capsules(tpl, None, 0.5, segs=[(0, 0), (0, 1)])
    assert radius.tolist() == [rho, rho]
    # the lower quantile is a sample: rings of 1, 2, 3, 4, 5 x rho round one segment, four vertices each (20 distances)
    v = np.concatenate([_ring_template(k * rho, heights=(0.1 * k,)).v_template.numpy() for k in range(1, 6)])
    axis = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    Jr = np.linalg.lstsq(v.T, axis.T, rcond=None)[0].T                 # any regressor that puts the two joints on the axis
    assert float(np.abs(Jr @ v - axis).max()) <= 1e-12
    tpl = types.SimpleNamespace(v_template=torch.from_numpy(v), shapedirs=torch.zeros(20, 3, 10, dtype=torch.float64),
                                J_regressor=torch.from_numpy(Jr), parents=torch.tensor([-1, 0]))
    for q, k in ((0.0, 1), (0.2, 1), (0.25, 2), (0.5, 3), (0.99, 5), (1.0, 5)):     # sorted[floor(q x 19)]
        _, radius = R.body_capsules(tpl, None, q, segs=[(0, 1)])
        assert abs(float(radius[0]) - k * rho) <= 1e-7, (q, radius)


# ----------------------------------------------------------------------------- configuration keys
def test_scene_config_keys_are_validated():
    from conftest import REPO
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    path = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    smpl = SMPL.synthetic(1, V=64)
    m = MLD(parse_config(path), SyntheticEgoDataModule(), smpl_model=smpl)
    assert m.path_scene_weight == 0.0 and m.scene_report is False and m.scene_capsule_quantile == 0.5
    cfg = parse_config(path)
    cfg.TEST.PATH_SCENE_WEIGHT, cfg.TEST.SCENE_REPORT, cfg.TEST.SCENE_CAPSULE_QUANTILE = 2, True, 0.75
    m = MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    assert m.path_scene_weight == 2 and m.scene_report is True and m.scene_capsule_quantile == 0.75
    for key, bad in (("PATH_SCENE_WEIGHT", -1.0), ("PATH_SCENE_WEIGHT", "much"), ("PATH_SCENE_WEIGHT", True),
                     ("PATH_SCENE_WEIGHT", float("inf")), ("SCENE_REPORT", 1), ("SCENE_REPORT", "yes"),
                     ("SCENE_CAPSULE_QUANTILE", 1.5), ("SCENE_CAPSULE_QUANTILE", -0.1), ("SCENE_CAPSULE_QUANTILE", "half"),
                     ("SCENE_CAPSULE_QUANTILE", False)):
        cfg = parse_config(path)
        cfg.TEST[key] = bad
        with pytest.raises(ValueError, match=key):
            MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)


# ----------------------------------------------------------------------------- the C-ABI
def test_scene_depth_entry_point_is_declared_bound_and_exported():
    import ctypes
    from conftest import REPO
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "seeme_scene_depth(" in hdr and "seeme_scene_depth" in _lib.exported_symbols() and hasattr(lib, "seeme_scene_depth")
    assert f"SEEME_SCENE_DEPTH_NBMAX {R.SCENE_DEPTH_NBMAX}\n" in hdr and f"SEEME_SCENE_DEPTH_CHUNK {R.SCENE_DEPTH_CHUNK}\n" in hdr
    assert "scene_depth.hip" in open(os.path.join(REPO, "seeme_amd", "csrc", "build.sh")).read()
    assert _lib.lib().seeme_version() >= 102
    # the argument checks run on the host, before anything is launched
    L = _lib.lib()
    segs = (ctypes.c_int32 * 66)(*([0, 1] * 33))
    rad = (ctypes.c_float * 33)(*([0.05] * 33))
    call = lambda W=1, K=1, T=1, J=2, N=1, NB=1, p=64, s=segs, r=rad: L.seeme_scene_depth(p, p, p, W, K, T, J, N, s, r, NB, p, p, p, None)
    for kw, msg in ((dict(W=0), b"W must"), (dict(W=65537), b"W must"), (dict(K=0), b"K must"), (dict(K=33), b"K must"),
                    (dict(T=0), b"T must"), (dict(T=(1 << 20) + 1), b"T must"), (dict(J=0), b"J must"), (dict(J=33), b"J must"),
                    (dict(N=0), b"N must"), (dict(N=(1 << 24) + 1), b"N must"), (dict(NB=0), b"NB must"), (dict(NB=33), b"NB must"),
                    (dict(p=None), b"null"), (dict(s=None), b"null"), (dict(r=None), b"null"), (dict(p=66), b"aligned"),
                    (dict(J=1), b"segment index"), (dict(W=65536, K=32, T=1 << 20), b"2^24")):
        assert call(**kw) != 0 and msg in L.seeme_last_error(), kw
    for bad in (-0.01, float("nan"), float("inf")):
        assert call(r=(ctypes.c_float * 1)(bad)) != 0 and b"radius" in L.seeme_last_error()
    assert call(s=(ctypes.c_int32 * 2)(0, -1)) != 0 and b"segment index" in L.seeme_last_error()
