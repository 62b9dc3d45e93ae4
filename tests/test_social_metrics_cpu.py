"""Interpersonal distance and mutual gaze without a GPU: the plain-torch twin against the float64 numpy restatement (recipe and special
frames), bin_index, the SocialMetrics accumulator against EgoMetrics / HypothesisMetrics and against a numpy accumulation, the config
keys and the C-ABI surface."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import social_reference as R

TOL64 = 1e-12


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _t(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


@pytest.fixture(scope="module")
def recipe8():
    """(inputs, restatement) of the B = 8 recipe: computed once, read by the accumulator tests."""
    a = R.recipe(8, 3, 12)
    return a, R.np_social(*a)


# ----------------------------------------------------------------------------- 1. twin against restatement
def test_twin_equals_the_restatement_on_the_recipe(recipe8):
    from seeme_amd.social_metrics import PER_HYP, PER_SEQ, social_metrics_torch
    a, want = recipe8
    assert PER_HYP == R.PER_HYP and PER_SEQ == R.PER_SEQ
    R.assert_recipe_margins(want, a[-1])
    assert 300.0 <= want["PERSON_DIST"].min() < 320.0 and 3900.0 < want["PERSON_DIST"].max() <= 4000.0      # 0.3 .. 4 m apart
    got = social_metrics_torch(*_t(a[:-1]), a[-1])
    for n in want:
        assert got[n].dtype == torch.float64 and _rel(got[n].numpy(), want[n]) <= TOL64, n
    # the frame chunking of the pair tensor changes nothing, bit for bit
    for fc in (1, 5, 64):
        again = social_metrics_torch(*_t(a[:-1]), a[-1], frame_chunk=fc)
        assert all(torch.equal(again[n], got[n]) for n in got), fc
    # float32 inputs give float32 results near the float64 ones
    got32 = social_metrics_torch(*[x.float() for x in _t(a[:-1])], a[-1])
    for n in want:
        assert got32[n].dtype == torch.float32 and _rel(got32[n].numpy(), want[n]) <= 1e-4, n


def test_twin_on_special_frames():
    """Parallel gaze is exactly 0 degrees, antiparallel exactly 180, a degenerate quaternion is the identity, coincident joints give
    c = 0, and lengths 0, 1 and T (and beyond) are clamped."""
    from seeme_amd.social_metrics import social_metrics_torch
    B, K, T = 5, 2, 4
    pred, ref, intr, qp, qr, qi, _ = R.recipe(B, K, T, seed=8)
    lengths = [0, 1, T, T + 3, -2]
    # b = 1: the reference's quaternion is twice the interactee's (the same rotation: 0 degrees), hypothesis 1 has an all-zero
    # quaternion = identity; b = 3: the interactee looks along +z, hypothesis 0 is a half turn about x of that (180 degrees)
    qr[1] = 2.0 * qi[1]
    qp[1, 1] = 0.0
    qi[3] = np.array([2.0, 0.0, 0.0, 0.0])
    qp[3, 0] = np.array([0.0, 3.0, 0.0, 0.0])
    # b = 2: joint 7 of the reference sits on joint 3 of the interactee, and joint 5 of hypothesis 1 on joint 0
    ref[2, :, 7] = intr[2, :, 3]
    pred[2, 1, :, 5] = intr[2, :, 0]
    args = (pred, ref, intr, qp, qr, qi)
    want = R.np_social(*args, lengths)
    got = {n: v.numpy() for n, v in social_metrics_torch(*_t(args), lengths).items()}
    for n in want:
        assert _rel(got[n], want[n]) <= TOL64, n
        assert (got[n][[0, 4]] == 0).all(), n                                   # n = 0 gives zeros
    assert got["GAZE_ANGLE_REF"][1] == 0.0 and want["GAZE_ANGLE_REF"][1] == 0.0
    assert got["GAZE_ANGLE"][3, 0] == 180.0 and want["GAZE_ANGLE"][3, 0] == 180.0
    ident = R.angle(np.array([0.0, 0.0, 1.0]), R.gaze(qi[1, 0]))
    assert want["GAZE_ANGLE"][1, 1] == ident and abs(got["GAZE_ANGLE"][1, 1] - ident) <= TOL64 * ident
    assert got["CLOSEST_DIST_REF"][2] == 0.0 and got["CLOSEST_DIST"][2, 1] == 0.0 and got["CLOSEST_DIST"][2, 0] > 0
    assert got["CLOSEST_DIST_ERROR"][2, 1] == 0.0                              # |0 - 0|
    # lengths past T are clamped: b = 3 equals a run with length T
    same = social_metrics_torch(*_t(args), [0, 1, T, T, 0])
    assert all(np.array_equal(same[n].numpy(), got[n]) for n in got)


def test_arccos_form_agrees_between_5_and_175_degrees():
    """The restatement's own tie to compute.py:31: angle() asserts it on every frame it sees; here on a sweep, and the two forms part
    company only where the arccos loses its digits."""
    g = np.array([0.0, 0.0, 1.0])
    for deg in (5.0, 30.0, 90.0, 150.0, 175.0):
        h = np.array([np.sin(np.deg2rad(deg)), 0.0, np.cos(np.deg2rad(deg))])
        assert abs(R.angle(g, h) - deg) <= 1e-12 * 180
    tiny = 1e-7
    h = np.array([np.sin(np.deg2rad(tiny)), 0.0, np.cos(np.deg2rad(tiny))])
    assert abs(R.angle(g, h) - tiny) <= 1e-12 * tiny                            # atan2 keeps 1e-7 degrees
    assert abs(np.degrees(np.arccos(np.dot(g, h))) - tiny) > 0.01 * tiny         # ... the arccos form does not


# ----------------------------------------------------------------------------- 2. bins
def test_bin_index_at_below_and_above_every_edge():
    from seeme_amd.social_metrics import bin_index, bin_labels
    for edges in (R.DIST_EDGES, R.GAZE_EDGES, (0.5, 0.75, 22.5)):
        vals, want = [], []
        for i, e in enumerate(edges):
            vals += [np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)]
            want += [i, i + 1, i + 1]
        vals += [-1e30, 1e30]
        want += [0, len(edges)]
        got = bin_index(torch.tensor(vals, dtype=torch.float64), edges)
        assert got.dtype == torch.int64 and got.tolist() == want == [R.np_bin(v, edges) for v in vals]
        assert bin_labels(edges) == R.np_labels(edges) and len(bin_labels(edges)) == len(edges) + 1
    assert bin_labels(R.DIST_EDGES) == ["lt1000", "1000_2000", "2000_3000", "ge3000"] and bin_labels(R.GAZE_EDGES) == ["lt150", "ge150"]
    # fp32 values (what the kernel hands over) are compared as they are
    assert bin_index(torch.tensor([999.99994, 1000.0], dtype=torch.float32), R.DIST_EDGES).tolist() == [0, 1]


# ----------------------------------------------------------------------------- 3. the accumulator
def _errors(a, split):
    """EgoMetrics.per_sequence per hypothesis on the recipe (hypothesis (0,1) gets a random head orientation, so that the 'test' rule
    drops it): (mpjpe, root, keep [B,K], hm-like dict)."""
    from seeme_amd.hyp_metrics import hyp_metrics_torch, keep_mask
    from seeme_amd.mld import EgoMetrics
    pred, ref, intr, qp, qr, qi, lengths = a
    B, K, T = pred.shape[:3]
    hm = hyp_metrics_torch(torch.from_numpy(pred), torch.from_numpy(ref), lengths)
    lens = torch.tensor(lengths)
    mask = (torch.arange(T)[None] < lens[:, None]).double().repeat_interleave(K, dim=0)
    q_ref_k = torch.from_numpy(qr).repeat_interleave(K, dim=0).reshape(-1, 4)
    hm["HEAD_ORIENTATION_ERROR"] = EgoMetrics.head_orientation_error(torch.from_numpy(qp).reshape(-1, 4), q_ref_k, mask,
                                                                     lens.repeat_interleave(K)).reshape(B, K)
    hm["have_quat"] = True
    return hm["MPJPE"], hm["ROOT_ERROR"], keep_mask(hm, split, True), hm


def _with_outlier(a):
    pred, ref, intr, qp, qr, qi, lengths = a
    qp = qp.copy()
    qp[0, 1] = np.random.default_rng(3).standard_normal(qp[0, 1].shape)
    return pred, ref, intr, qp, qr, qi, lengths


def test_recipe_populates_the_bins(recipe8):
    """On the REFERENCE values, before anything is accumulated: kept sequences in at least three distance bins and in both gaze bins,
    and the inclusion rule drops something (a filter that keeps everything, or nothing, cannot pass)."""
    a, want = recipe8
    a = _with_outlier(a)
    _, _, keep, _ = _errors(a, "test")
    keep = keep.numpy()
    assert not keep[0, 1] and not keep[1].any() and not keep[2].any() and keep.sum() >= keep.size // 2
    kept = [b for b in range(8) if keep[b].any()]
    assert len({R.np_bin(want["PERSON_DIST"][b], R.DIST_EDGES) for b in kept}) >= 3
    assert {R.np_bin(want["GAZE_ANGLE_REF"][b], R.GAZE_EDGES) for b in kept} == {0, 1}


@pytest.mark.parametrize("split", ["test", "val"])
def test_social_metrics_k1_sums_to_ego_metrics(recipe8, split):
    from seeme_amd.mld import EgoMetrics
    from seeme_amd.social_metrics import SocialMetrics
    a, _ = recipe8
    pred, ref, intr, qp, qr, qi, lengths = _with_outlier(a)
    pred, qp = pred[:, 1:2], qp[:, 1:2]                                         # K = 1: hypothesis 1 (the outlier at b = 0)
    a1 = (pred, ref, intr, qp, qr, qi, lengths)
    want = R.np_social(*a1)
    mp, root, keep, _ = _errors(a1, split)
    sm = {n: torch.from_numpy(v) for n, v in want.items()}
    acc = SocialMetrics(R.DIST_EDGES, R.GAZE_EDGES)
    acc.update(sm, mp, root, keep)
    ego = EgoMetrics()
    ego.update(torch.from_numpy(pred[:, 0]), torch.from_numpy(ref), lengths, torch.from_numpy(qp).reshape(-1, 4),
               torch.from_numpy(qr).reshape(-1, 4), split=split)
    es = ego.sums().numpy()
    s = acc.sums().numpy()
    assert s.shape == (len(acc),) and len(acc) == 9 + 4 * (4 + 2)
    dist, gaze = s[9:9 + 16].reshape(4, 4), s[25:].reshape(2, 4)
    assert es[5] > 0 and es[5] < 8                                              # MPJPE's count: some kept, some dropped
    for bins in (dist, gaze):
        assert abs(bins[:, 0].sum() - es[0]) <= TOL64 * es[0]                   # sum of MPJPE
        assert abs(bins[:, 1].sum() - es[1]) <= TOL64 * es[1]                   # sum of ROOT_ERROR
        assert bins[:, 2].sum() == es[5] == es[6] and bins[:, 3].sum() == 8
    got = acc.compute()
    ref_out = R.np_accumulate(want, mp.numpy(), root.numpy(), keep.numpy())
    assert set(got) == set(ref_out)
    for k in ref_out:
        assert abs(got[k] - ref_out[k]) <= TOL64 * max(abs(ref_out[k]), 1e-300), k
    assert "MPJPE_dist_lt1000" in got and "ROOT_ERROR_gaze_ge150" in got and got["count_seq_dist_1000_2000"] == 2.0
    assert got["count_kept_dist_2000_3000"] + got["count_kept_dist_1000_2000"] == 2.0       # b = 1, 2 (one and two frames) never move


@pytest.mark.parametrize("split", ["test", "val"])
def test_social_metrics_k_sums_to_hypothesis_metrics(recipe8, split):
    from seeme_amd.hyp_metrics import HypothesisMetrics
    from seeme_amd.social_metrics import SocialMetrics
    a, _ = recipe8
    a = _with_outlier(a)
    want = R.np_social(*a)
    mp, root, keep, hm = _errors(a, split)
    sm = {n: torch.from_numpy(v) for n, v in want.items()}
    acc = SocialMetrics()
    acc.update(sm, mp, root, keep)
    hyp = HypothesisMetrics()
    hyp.update(hm, split)
    hs, s = hyp.sums().numpy(), acc.sums().numpy()
    for bins in (s[9:25].reshape(4, 4), s[25:].reshape(2, 4)):
        assert abs(bins[:, 0].sum() - hs[0]) <= TOL64 * hs[0] and abs(bins[:, 1].sum() - hs[1]) <= TOL64 * hs[1]
        assert bins[:, 2].sum() == hs[4] and 0 < hs[4] < 8 and bins[:, 3].sum() == hs[5] == 8
    got, ref_out = acc.compute(), R.np_accumulate(want, mp.numpy(), root.numpy(), keep.numpy())
    assert set(got) == set(ref_out) and "MPJPE_best_of_k_dist_ge3000" in got and "MPJPE_mean_of_k_gaze_lt150" in got
    for k in ref_out:
        assert abs(got[k] - ref_out[k]) <= TOL64 * max(abs(ref_out[k]), 1e-300), k
    # two updates equal one update on the concatenated batch
    two = SocialMetrics()
    for rows in (slice(0, 3), slice(3, 8)):
        two.update({n: v[rows] for n, v in sm.items()}, mp[rows], root[rows], keep[rows])
    assert _rel(two.sums().numpy(), s) <= TOL64
    # the sums travel (a reduction over ranks hands them back): compute(sums, K) reads them, reset() forgets them
    assert acc.compute(acc.sums().clone(), 3) == got
    acc.reset()
    assert float(acc.sums().abs().sum()) == 0.0 and acc.num_hypotheses == 0
    with pytest.raises(ValueError, match="hypotheses"):
        two.update({n: v[:, :1] if v.dim() == 2 else v for n, v in sm.items()}, mp[:, :1], root[:, :1], keep[:, :1])


def test_an_empty_bin_reports_its_count_and_no_mean(recipe8):
    from seeme_amd.social_metrics import SocialMetrics
    a, want = recipe8
    mp, root, keep, _ = _errors(a, "val")
    acc = SocialMetrics((100.0, 5000.0), (10.0, 179.5))                          # nobody is nearer than 0.1 m or further than 5 m
    acc.update({n: torch.from_numpy(v) for n, v in want.items()}, mp, root, keep)
    got = acc.compute()
    assert got["count_seq_dist_lt100"] == 0.0 and got["count_kept_dist_ge5000"] == 0.0 and got["count_seq_dist_100_5000"] == 8.0
    assert "MPJPE_best_of_k_dist_lt100" not in got and "MPJPE_best_of_k_dist_100_5000" in got
    assert "MPJPE_mean_of_k_gaze_lt10" not in got and "MPJPE_mean_of_k_gaze_ge179.5" not in got
    empty = SocialMetrics().compute()
    assert empty["count_seq_social"] == 0.0 and not any(k.startswith(("MPJPE", "PERSON", "GAZE")) for k in empty)
    with pytest.raises(ValueError, match="sums"):
        SocialMetrics().compute(torch.zeros(5, dtype=torch.float64))


# ----------------------------------------------------------------------------- 4. configuration and plumbing
def test_social_config_validation_in_mld_and_cli():
    from seeme_amd import cli
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    plain = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    smpl = SMPL.synthetic(1, V=64)
    mk = lambda cfg: MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    cfg = parse_config(plain)
    assert "SOCIAL_METRICS" not in cfg.TEST                                      # no YAML names the keys
    off = mk(cfg)
    assert off.social_metrics is False and off.social_dist_edges == (1000.0, 2000.0, 3000.0) and off.social_gaze_edges == (150.0,)
    cfg.TEST.SOCIAL_METRICS = True
    on = mk(cfg)
    assert on.social_metrics is True and len(on.SocialMetric) == 9 + 4 * 6
    for bad in (1, 0, "yes", None):
        cfg = parse_config(plain)
        cfg.TEST.SOCIAL_METRICS = bad
        with pytest.raises(ValueError, match="TEST.SOCIAL_METRICS"):
            mk(cfg)
    for key, bads in (("SOCIAL_DIST_EDGES", ([], [2000, 1000], [1000, 1000], [float("nan")], [float("inf")], list(range(1, 10)), 1000,
                                             ["a"], [True])),
                      ("SOCIAL_GAZE_EDGES", ([], [0], [180], [-5], [150, 30], [181.0], list(range(1, 10)), "150"))):
        for bad in bads:
            cfg = parse_config(plain)
            setattr(cfg.TEST, key, bad)                                          # checked whether or not the option is on
            with pytest.raises(ValueError, match="TEST." + key):
                mk(cfg)
    cfg = parse_config(plain)
    cfg.TEST.SOCIAL_METRICS, cfg.TEST.SOCIAL_DIST_EDGES, cfg.TEST.SOCIAL_GAZE_EDGES = True, [500, 1500.5], [30, 90, 150]
    m = mk(cfg)
    assert m.SocialMetric.edges == {"dist": (500.0, 1500.5), "gaze": (30.0, 90.0, 150.0)} and len(m.SocialMetric) == 9 + 4 * 7
    # the three things the option needs
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_egobody_rot6d.yaml"))
    cfg.TEST.SOCIAL_METRICS = True
    with pytest.raises(ValueError, match="DATA_TYPE"):
        MLD(cfg, SyntheticEgoDataModule(nfeats=144, data_type="rot6d"), smpl_model=smpl)
    cfg = parse_config(plain)
    cfg.TEST.SOCIAL_METRICS, cfg.TRAIN.ABLATION.PREDICT_TRANSL = True, False
    with pytest.raises(ValueError, match="PREDICT_TRANSL"):
        mk(cfg)
    cfg = parse_config(plain)
    cfg.TEST.SOCIAL_METRICS, cfg.ESTIMATE = True, "interactee"
    with pytest.raises(ValueError, match="ESTIMATE"):
        mk(cfg)
    # the command line
    args = cli.build_parser("test").parse_args(["--cfg", plain, "--social_metrics"])
    c = cli.load_cfg(args, "test")
    assert c.TEST.SOCIAL_METRICS is True and c.TEST.MESH_METRICS is False
    assert "SOCIAL_METRICS" not in cli.load_cfg(cli.build_parser("test").parse_args(["--cfg", plain]), "test").TEST


def test_allsplit_step_feeds_the_accumulator_only_when_the_key_is_there(recipe8, monkeypatch):
    """allsplit_step on a prepared ego_eval result (K = 1, CPU tensors): without rs['social_metrics'] the accumulator stays empty and
    EgoMetrics' sums are what they are with it; with it, the bins add up to EgoMetrics' MPJPE sum and count."""
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    a, _ = recipe8
    pred, ref, intr, qp, qr, qi, lengths = a
    want = R.np_social(pred[:, :1], ref, intr, qp[:, :1], qr, qi, lengths)
    rs = {"joints_rst": torch.from_numpy(pred[:, 0]), "joints_ref": torch.from_numpy(ref), "lengths": lengths,
          "orientation_quat_rst": torch.from_numpy(qp[:, 0]).reshape(-1, 4), "orientation_quat_ref": torch.from_numpy(qr).reshape(-1, 4),
          "joints_interactee": torch.from_numpy(intr), "joints_interactee_gt": None}
    model = MLD(parse_config(os.path.join(REPO, "configs", "config_mld_egobody.yaml")), SyntheticEgoDataModule(),
                smpl_model=SMPL.synthetic(1, V=64))
    sums = {}
    for with_key in (False, True):
        out = dict(rs, social_metrics={n: torch.from_numpy(v) for n, v in want.items()}) if with_key else dict(rs)
        monkeypatch.setattr(model, "ego_eval", lambda batch, out=out: out)
        model.EgoMetric.reset()
        model.SocialMetric.reset()
        model.allsplit_step("test", None)
        sums[with_key] = (model.EgoMetric.sums().clone(), model.SocialMetric.sums().clone())
    assert torch.equal(sums[False][0], sums[True][0]) and float(sums[False][1].abs().sum()) == 0.0
    es, s = sums[True][0].numpy(), sums[True][1].numpy()
    assert es[5] > 0 and abs(s[9:25].reshape(4, 4)[:, 0].sum() - es[0]) <= TOL64 * es[0] and s[25:].reshape(2, 4)[:, 2].sum() == es[5]


# ----------------------------------------------------------------------------- 5. the C-ABI surface
def test_header_ctypes_table_build_script_and_library_agree():
    from seeme_amd import _lib
    from seeme_amd import social_metrics as S
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    assert f"#define SEEME_SOCIAL_FRAME_CHUNK {S.FRAME_CHUNK}\n" in hdr
    assert "social_metrics.hip" in open(os.path.join(REPO, "seeme_amd", "csrc", "build.sh")).read()
    lib = _lib.lib()
    for name in ("seeme_social_metrics", "seeme_social_metrics_workspace_bytes"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        proto = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name
    for word in ("atan2", "compute.py:31", "quat_to_rotmat"):
        assert word in hdr and word in S.__doc__, word                           # the definitions are stated in both places
    ws = lib.seeme_social_metrics_workspace_bytes
    chunks = lambda T: -(-T // S.FRAME_CHUNK)
    for B, K, T in ((1, 1, 1), (3, 2, 16), (5, 3, S.FRAME_CHUNK + 1), (64, 20, 60), (32, 32, 196)):
        assert ws(B, K, T) == B * chunks(T) * (5 * K + 3) * 4, (B, K, T)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 33, 1), (1, 1, 0)):
        assert ws(*bad) == 0, bad
    # argument checks come before any device work: they hold without a GPU
    err = lambda: lib.seeme_last_error()
    base = dict(jp=16, jr=32, ji=48, qp=64, qr=80, qi=96, lens=4, B=2, K=3, T=9, ph=8, ps=12, ws=16, wsb=1 << 20, st=0)
    order = ("jp", "jr", "ji", "qp", "qr", "qi", "lens", "B", "K", "T", "ph", "ps", "ws", "wsb", "st")
    call = lambda **k: lib.seeme_social_metrics(*[{**base, **k}[n] for n in order])
    for kw, msg in ((dict(K=0), b"K must"), (dict(K=33), b"K must"), (dict(B=0), b"B must"), (dict(B=65536), b"B must"),
                    (dict(T=0), b"T must"), (dict(jp=0), b"null"), (dict(qi=0), b"null"), (dict(ws=0), b"null"),
                    (dict(jr=36), b"16-byte"), (dict(qp=72), b"16-byte"), (dict(ws=18), b"4-byte"), (dict(lens=6), b"4-byte"),
                    (dict(wsb=ws(2, 3, 9) - 1), b"workspace too small")):
        assert call(**kw) != 0 and msg in err() and b"social_metrics" in err(), kw
