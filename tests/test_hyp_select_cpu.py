"""Choosing one of K hypotheses without ground truth, host side: the plain-torch twin of the pair-distance kernel against a numpy loop
restatement, the medoid and its tie rule, ``select_index``, the SelectionMetrics accumulator, the config key, the CLI option and
the C-ABI surface.

Inputs (shared with tests/test_gpu_hyp_select.py): ``hyp_reference.recipe`` with one hypothesis per sequence made central,
c_b = (3b+1) % K, pred[b,c_b] = ref[b] + 0.25 (pred[b,c_b] - ref[b]).  Without that the K row sums of a sequence differ by 9e-5
relative, the size of fp32 rounding; with it the float64 gap between the smallest and the second smallest row sum is >= 8.8e-2
(1.35e-2 for (64,3,64)), and ``assert_gap`` holds every sequence with K >= 3 to >= 1e-2 = 100 x TOL_F32 before anything is compared."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
import hyp_reference as R

TOL = 1e-12
GAP_MIN = 1e-2               # 100 x the project's fp32 bound TOL_F32 = 1e-4
GAP_CASES = ["recipe", (3, 3, 9), (4, 7, 17), (3, 20, 9), (2, 31, 4), (2, 32, 5), (1, 4, 1)]
SMALL_CASES = [(1, 1, 3), (3, 2, 16)]


def inputs(shape):
    """float64 pred [B,K,T,24,3], ref [B,T,24,3], lengths, and the central hypothesis c_b of every sequence."""
    if shape == "recipe":
        pred, ref, _, _, lengths = R.recipe()
    else:
        B, K, T = shape
        pred, ref, _, _, lengths = R.recipe(B, K, T, lengths=R.ragged_lengths(B, T), seed=3, special=B > 1 and K > 2)
    B, K = pred.shape[:2]
    centers = [(3 * b + 1) % K for b in range(B)]
    pred = pred.copy()
    for b, c in enumerate(centers):
        pred[b, c] = ref[b] + 0.25 * (pred[b, c] - ref[b])
    return pred, ref, lengths, centers


def np_pairdist(pred, lengths):
    """The definition as plain loops: dist [B,K,K] in mm, the row sums taken in j order, and the first index of the smallest."""
    B, K, T = pred.shape[:3]
    dist, rows, medoid = np.zeros((B, K, K)), np.zeros((B, K)), np.zeros(B, np.int64)
    for b in range(B):
        n = min(max(int(lengths[b]), 0), T)
        a = R.align(pred[b])                                        # [K,T,24,3]
        for i in range(K):
            for j in range(i + 1, K):
                if n > 0:
                    s = 0.0
                    for t in range(n):
                        s += np.linalg.norm(a[i, t] - a[j, t], axis=-1).sum()
                    dist[b, i, j] = dist[b, j, i] = s / 24 / n * 1000
        for i in range(K):
            for j in range(K):
                rows[b, i] += dist[b, i, j]
        medoid[b] = int(np.argmin(rows[b]))                         # the first of the smallest
    return dist, rows, medoid


def assert_gap(rows):
    """Every sequence (none left out) with K >= 3: the two smallest float64 row sums are >= GAP_MIN apart, relatively."""
    if rows.shape[1] < 3:
        return None
    s = np.sort(rows, axis=1)
    assert (s[:, 0] > 0).all()
    gap = (s[:, 1] - s[:, 0]) / s[:, 0]
    assert (gap >= GAP_MIN).all(), gap
    return float(gap.min())


def _close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return bool(np.all(np.abs(a - b) <= tol * np.abs(b)))


# ----------------------------------------------------------------------------- the torch twin
@pytest.mark.parametrize("shape", GAP_CASES + SMALL_CASES, ids=str)
def test_hyp_pairdist_torch_float64_vs_numpy_loops(shape):
    from seeme_amd.hyp_metrics import hyp_metrics_torch, hyp_pairdist_torch
    pred, ref, lengths, centers = inputs(shape)
    B, K, T = pred.shape[:3]
    want, rows, medoid = np_pairdist(pred, lengths)
    gap = assert_gap(rows)
    print(f"{shape}: smallest relative gap of the row sums {gap}")
    got = hyp_pairdist_torch(torch.from_numpy(pred), lengths)
    D = got["PAIR_DIST"]
    assert D.dtype == torch.float64 and D.shape == (B, K, K)
    assert got["medoid_index"].dtype == torch.int64 and got["medoid_index"].shape == (B,)
    assert _close(D.numpy(), want)
    assert float(torch.diagonal(D, dim1=1, dim2=2).abs().max()) == 0.0 and torch.equal(D, D.transpose(1, 2))
    assert K == 1 or (D[:, ~np.eye(K, dtype=bool)] > 0).all()
    assert got["medoid_index"].tolist() == medoid.tolist()
    if K >= 3:
        assert medoid.tolist() == centers
    else:                       # K = 2: both row sums are the same number, the lowest index wins; K = 1: the only one
        assert medoid.tolist() == [0] * B
    # the matrix adds up to the existing APD
    apd = hyp_metrics_torch(torch.from_numpy(pred), torch.from_numpy(ref), lengths)["APD_JOINTS"].numpy()
    mine = D.sum(dim=(1, 2)).numpy() / max(K * (K - 1), 1) / 2
    assert _close(mine, apd) and (K > 1) == bool((apd > 0).all())
    if K == 1:
        assert float(D.abs().max()) == 0.0


def test_hyp_pairdist_torch_clamps_lengths_and_breaks_ties_low():
    from seeme_amd.hyp_metrics import _medoid, hyp_pairdist_torch
    pred, ref, lengths, centers = inputs((4, 7, 17))
    p = torch.from_numpy(pred)
    hand = [40, 0, -3, 5]                                           # above T, zero, negative, inside
    got = hyp_pairdist_torch(p, hand)
    want, rows, medoid = np_pairdist(pred, hand)
    assert _close(got["PAIR_DIST"].numpy(), want) and got["medoid_index"].tolist() == medoid.tolist()
    full = hyp_pairdist_torch(p, [17, 17, 17, 17])
    assert torch.equal(got["PAIR_DIST"][0], full["PAIR_DIST"][0]) and got["medoid_index"][0] == full["medoid_index"][0]
    for b in (1, 2):                                                # no valid frame: a zero matrix, medoid 0
        assert float(got["PAIR_DIST"][b].abs().max()) == 0.0 and int(got["medoid_index"][b]) == 0
    assert float(got["PAIR_DIST"][3].max()) > 0
    # the tie rule itself
    tie = torch.tensor([[[0.0, 2.0, 1.0], [2.0, 0.0, 1.0], [1.0, 1.0, 0.0]],        # rows 3, 3, 2 -> 2
                        [[0.0, 1.0, 2.0], [1.0, 0.0, 2.0], [2.0, 2.0, 0.0]],        # rows 3, 3, 4 -> 0 (not 1)
                        [[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]]])       # all equal -> 0
    assert _medoid(tie).tolist() == [2, 0, 0]
    # any float dtype, any K: 40 hypotheses in float32
    rng = np.random.default_rng(0)
    big = torch.from_numpy(rng.standard_normal((1, 40, 3, 24, 3))).float()
    out = hyp_pairdist_torch(big, [3])
    assert out["PAIR_DIST"].shape == (1, 40, 40) and out["PAIR_DIST"].dtype == torch.float32
    w, _, m = np_pairdist(big.double().numpy(), [3])
    assert _close(out["PAIR_DIST"].numpy(), w, 1e-5)


def test_select_index():
    from seeme_amd.hyp_metrics import select_index
    hm = {"MPJPE": torch.zeros(4, 5), "medoid_index": torch.tensor([3, 0, 4, 1], dtype=torch.int32)}
    first, med = select_index(hm, "first"), select_index(hm, "medoid")
    assert first.dtype == torch.int64 and first.tolist() == [0, 0, 0, 0]
    assert med.dtype == torch.int64 and med.tolist() == [3, 0, 4, 1]
    with pytest.raises(ValueError, match="mode"):
        select_index(hm, "mean")


# ----------------------------------------------------------------------------- the accumulator
def _reference_hm():
    """The per-hypothesis numbers of the unmodified recipe (tests/test_hypotheses_cpu.py asserts their facts against the oracle) with a
    selection that meets every case of the inclusion rule."""
    pred, ref, qp, q, lengths = R.recipe()
    ph, head = R.np_per_hyp(pred, ref, lengths), R.np_head(qp, q, lengths)
    sel = np.array([1, 3, 2, 0, 3, 1])                              # sequence 1: the best hypothesis under both rules
    moving = ph["ACCL"] > 0
    kept = moving & (head < 0.9) & (ph["ROOT_ERROR"] < 300)
    rows = np.arange(6)
    # sequence 0: the selection moves but drifts at the root -> dropped by the 'test' rule only; 3 and 4: too short to have an ACCL
    assert moving[0, 1] and not kept[0, 1] and not moving[3].any() and not moving[4].any()
    assert kept[rows, sel].tolist() == [False, True, True, False, False, True]
    assert moving[rows, sel].tolist() == [True, True, True, False, False, True]
    rng = np.random.default_rng(5)
    mesh = {"PA_MPJPE": 10 + rng.random((6, 5)), "V2V": 20 + rng.random((6, 5))}
    return ph, head, sel, kept, moving, mesh


def _hm(ph, head, sel, keep, rows):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows]))
    best = [int(np.argmin(np.where(keep[b], ph["MPJPE"][b], np.inf))) if keep[b].any() else -1 for b in range(6)]
    return {"MPJPE": t(ph["MPJPE"]), "ROOT_ERROR": t(ph["ROOT_ERROR"]), "ACCL": t(ph["ACCL"]), "HEAD_ORIENTATION_ERROR": t(head),
            "have_quat": True, "selected_index": t(sel), "medoid_index": t(sel), "best_index": t(np.array(best))}, best


@pytest.mark.parametrize("split", ["test", "val"])
def test_selection_metrics_accumulator(split):
    from seeme_amd.hyp_metrics import SelectionMetrics
    ph, head, sel, kept, moving, mesh = _reference_hm()
    keep = kept if split == "test" else moving
    _, best = _hm(ph, head, sel, keep, slice(None))
    counted = [b for b in range(6) if keep[b, sel[b]]]
    assert len(counted) == (3 if split == "test" else 4) and (0 in counted) == (split == "val")
    want = {f"{n}_medoid": float(np.sum([ph[n][b, sel[b]] for b in counted])) / len(counted) for n in ("MPJPE", "ROOT_ERROR", "ACCL")}
    want["count_seq_medoid"] = float(len(counted))
    want["medoid_is_best_ratio"] = sum(best[b] == sel[b] for b in counted) / len(counted)
    want_mesh = {"PA_MPJPE_medoid": float(np.sum([mesh["PA_MPJPE"][b, sel[b]] for b in counted])) / len(counted),
                 "V2V_medoid": float(np.sum([mesh["V2V"][b, sel[b]] for b in counted])) / len(counted)}
    tm = lambda rows: {k: torch.from_numpy(np.ascontiguousarray(v[rows])) for k, v in mesh.items()}
    # two updates add
    acc = SelectionMetrics()
    assert acc.sums().shape == (8,) and acc.compute()["count_seq_medoid"] == 0
    for rows in (slice(0, 2), slice(2, 6)):
        acc.update(_hm(ph, head, sel, keep, rows)[0], split)
    got = acc.compute()
    assert set(got) == set(want) and acc.sums().dtype == torch.float64
    for k, v in want.items():
        assert _close(got[k], v), (k, got[k], v)
    # ... with the mesh metrics of the same batches: two more names
    a, b = SelectionMetrics(), SelectionMetrics()
    a.update(_hm(ph, head, sel, keep, slice(0, 2))[0], split, tm(slice(0, 2)))
    b.update(_hm(ph, head, sel, keep, slice(2, 6))[0], split, tm(slice(2, 6)))
    two = a.compute(sums=a.sums() + b.sums())                       # what the reduction over ranks hands over
    assert set(two) == set(want) | set(want_mesh)
    for k, v in {**want, **want_mesh}.items():
        assert _close(two[k], v), (k, two[k], v)
    one = SelectionMetrics()
    one.update(_hm(ph, head, sel, keep, slice(None))[0], split, tm(slice(None)))
    for k, v in two.items():
        assert _close(one.compute()[k], v), k
    # the medoid is the best hypothesis somewhere and not everywhere
    assert want["medoid_is_best_ratio"] == (1 / 3 if split == "test" else 1 / 4)
    one.reset()
    assert one.compute()["count_seq_medoid"] == 0 and set(one.compute()) == set(want)


# ----------------------------------------------------------------------------- config and CLI
def test_hyp_select_config_key_and_validation():
    from seeme_amd.config import parse_config
    from seeme_amd.hyp_metrics import SelectionMetrics
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    assert parse_config(os.path.join(REPO, "configs", "base.yaml")).TEST.HYP_SELECT == "first"
    path = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    cfg = parse_config(path)
    assert cfg.TEST.HYP_SELECT == "first"
    smpl = SMPL.synthetic(1, V=64)
    m = MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    assert m.hyp_select == "first" and isinstance(m.SelMetric, SelectionMetrics) and m.SelMetric.compute()["count_seq_medoid"] == 0
    cfg = parse_config(path)
    cfg.TEST.HYP_SELECT = "medoid"
    m = MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    assert m.hyp_select == "medoid"
    for bad in ("mean", "", 1, None, True):
        cfg = parse_config(path)
        cfg.TEST.HYP_SELECT = bad
        with pytest.raises(ValueError, match="HYP_SELECT"):
            MLD(cfg, SyntheticEgoDataModule(), smpl_model=smpl)
    with pytest.raises(ValueError, match="hyp_select"):
        m.ego_eval((), num_hypotheses=4, hyp_select="mean")


def test_cli_hyp_select_option():
    from seeme_amd import cli
    cfgp = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
    p = cli.build_parser("test")
    assert p.parse_args(["--cfg", cfgp]).hyp_select is None
    assert cli.load_cfg(p.parse_args(["--cfg", cfgp]), "test").TEST.HYP_SELECT == "first"
    for word in ("first", "medoid"):
        args = p.parse_args(["--cfg", cfgp, "--hyp_select", word])
        assert args.hyp_select == word and cli.load_cfg(args, "test").TEST.HYP_SELECT == word
    with pytest.raises(SystemExit):
        p.parse_args(["--cfg", cfgp, "--hyp_select", "mean"])


# ----------------------------------------------------------------------------- the C-ABI surface
def test_header_ctypes_and_library_agree_on_the_pairdist_entry_points():
    from seeme_amd import _lib
    names = ("seeme_hyp_pairdist", "seeme_hyp_pairdist_workspace_bytes")
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    declared = set(re.findall(r"\b(seeme_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    dynamic = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in names:
        assert name in declared and name in _lib.exported_symbols() and name in dynamic and hasattr(lib, name)
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name
    ws = lib.seeme_hyp_pairdist_workspace_bytes
    assert ws(32, 20, 196) == 32 * 25 * 190 * 4              # chunks of 8 frames at this size, 190 pairs
    assert ws(2, 32, 5) == 2 * 2 * 496 * 4 and ws(1, 1, 3) > 0
    assert ws(32, 33, 196) == 0 and ws(32, 0, 196) == 0 and ws(0, 4, 8) == 0 and ws(4, 4, 0) == 0
    # argument checks come before any device work: they hold without a GPU
    err = lambda: lib.seeme_last_error()
    for k in (0, 33):
        assert lib.seeme_hyp_pairdist(16, 16, 1, k, 3, 16, 16, 16, 1 << 20, 0) != 0 and b"K must be" in err()
    assert lib.seeme_hyp_pairdist(16, 16, 0, 4, 3, 16, 16, 16, 1 << 20, 0) != 0 and b"B must be" in err()
    assert lib.seeme_hyp_pairdist(16, 16, 1, 4, 0, 16, 16, 16, 1 << 20, 0) != 0 and b"T must be" in err()
    assert lib.seeme_hyp_pairdist(0, 16, 1, 4, 3, 16, 16, 16, 1 << 20, 0) != 0 and b"null" in err()
    assert lib.seeme_hyp_pairdist(16, 16, 1, 4, 3, 16, 0, 16, 1 << 20, 0) != 0 and b"null" in err()
    assert lib.seeme_hyp_pairdist(8, 16, 1, 4, 3, 16, 16, 16, 1 << 20, 0) != 0 and b"aligned" in err()
    assert lib.seeme_hyp_pairdist(16, 16, 1, 4, 3, 16, 16, 16, ws(1, 4, 3) - 1, 0) != 0 and b"workspace" in err()
