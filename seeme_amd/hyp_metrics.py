"""K hypotheses per sequence: per-hypothesis errors and the diversity of the K draws.

``hyp_metrics_hip``   one pass of ``seeme_hyp_metrics`` (csrc/hyp_metrics.hip) over the joints: K <= 32, fp32, on the device.
``hyp_metrics_torch`` the plain-torch twin (any float dtype, any device, any K): the test reference, and what callers of this
                      module use for K > 32.  ``MLD.ego_eval`` uses the kernel.

Row order is sequence-major: ``jts_pred_all[b, k]`` is hypothesis k of sequence b.  Results are in mm:

  MPJPE, ROOT_ERROR, ACCL [B,K]  ``EgoMetrics.per_sequence`` of hypothesis k against the reference of its sequence
  APD_JOINTS [B]                 per valid frame, on the K aligned predictions a [K,24,3]:
                                 sum_{i,j} sum_joints |a_i - a_j| / 24 / K / (K-1) / 2 (the EgoHMR form, test_egohmr.py:519-520 --
                                 HALF the mean distance over unordered pairs), then the mean over the valid frames
  STD_JOINTS [B]                 per valid frame the unbiased standard deviation over K of every joint coordinate, mean over
                                 the 72 coordinates (test_egohmr.py:496), then the mean over the valid frames
Both diversity numbers are 0 for K = 1.

Choosing ONE of the K hypotheses without ground truth (TEST.HYP_SELECT medoid):

``hyp_pairdist_hip``   ``seeme_hyp_pairdist``: PAIR_DIST [B,K,K] (mm), the mean over the valid frames (clamp(len, 0, T)) and the 24
                       joints of |a_i - a_j| on the aligned predictions, and medoid_index [B] int64, the argmin over i of
                       sum_j PAIR_DIST[b,i,j] (lowest index on a tie).  sum PAIR_DIST[b] / (K (K-1)) / 2 is APD_JOINTS[b].
``hyp_pairdist_torch`` its plain-torch twin (any float dtype, any device, any K).
``SelectionMetrics``   running sums of the selected hypothesis' errors.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib as L

K_MAX = 32
PER_HYP = ("MPJPE", "ROOT_ERROR", "ACCL")
PER_SEQ = ("APD_JOINTS", "STD_JOINTS")


def _align(j):
    """First frame's joint 15, then each frame's own joint 0 (EgoMetrics.per_sequence); j [..., T, 24, 3]."""
    j = j - j[..., 0:1, 15:16, :]
    return j - j[..., :, 0:1, :]


def hyp_metrics_torch(jts_pred_all, jts_ref, lengths) -> Dict[str, torch.Tensor]:
    from .mld import EgoMetrics
    B, K, T = jts_pred_all.shape[:3]
    dev, dt = jts_ref.device, jts_ref.dtype
    lens = torch.as_tensor(lengths, device=dev).reshape(B)
    cols = [EgoMetrics.per_sequence(jts_pred_all[:, k].to(dt), jts_ref, lens) for k in range(K)]
    out = {n: torch.stack([c[n] for c in cols], dim=1) for n in PER_HYP}
    if K == 1:
        out["APD_JOINTS"] = torch.zeros(B, device=dev, dtype=dt)
        out["STD_JOINTS"] = torch.zeros(B, device=dev, dtype=dt)
        return out
    mask = (torch.arange(T, device=dev)[None, :] < lens[:, None]).to(dt)
    apd = torch.zeros(B, T, device=dev, dtype=dt)
    for b in range(B):                       # per sequence: the pair tensor is [T,K,K,24,3]
        a = _align(jts_pred_all[b].to(dt)).transpose(0, 1)                            # [T,K,24,3]
        d = (a[:, :, None] - a[:, None, :]).norm(dim=-1)                               # [T,K,K,24]
        apd[b] = d.sum(dim=(1, 2, 3)) / 24 / K / (K - 1) / 2                           # test_egohmr.py:519-520
    a = _align(jts_pred_all.to(dt))                                                    # [B,K,T,24,3]
    std = a.std(dim=1, unbiased=True).flatten(2).mean(dim=-1)                           # [B,T]; test_egohmr.py:496
    out["APD_JOINTS"] = (apd * mask).sum(1) / lens * 1000.0
    out["STD_JOINTS"] = (std * mask).sum(1) / lens * 1000.0
    return out


_WS = L.Workspace(per_stream=True)    # shared by _launch and _launch_pairdist: launches of one stream run in order


def hyp_metrics_hip(jts_pred_all, jts_ref, lengths) -> Dict[str, torch.Tensor]:
    """jts_pred_all [B,K,T,24,3] (or [B*K,T,24,3] with K inferred from jts_ref), jts_ref [B,T,24,3], fp32 on the device."""
    L.require_cuda(jts_pred_all, "jts_pred_all")
    L.require_cuda(jts_ref, "jts_ref")
    B, T = int(jts_ref.shape[0]), int(jts_ref.shape[1])
    if jts_pred_all.dim() == 4:
        jts_pred_all = jts_pred_all.reshape(B, -1, T, 24, 3)
    K = int(jts_pred_all.shape[1])
    if tuple(jts_pred_all.shape) != (B, K, T, 24, 3) or tuple(jts_ref.shape) != (B, T, 24, 3):
        raise L.SeemeError(f"hyp_metrics: joints are {tuple(jts_pred_all.shape)} / {tuple(jts_ref.shape)}: expected [B,K,T,24,3] / [B,T,24,3]")
    dev = jts_ref.device
    pred, ref = jts_pred_all.contiguous(), jts_ref.contiguous()
    lens = torch.as_tensor(lengths).reshape(B).to(device=dev, dtype=torch.int32)
    return _launch(pred, ref, lens, B, K, T)


def _launch(pred, ref, lens, B, K, T, ws_bytes=None) -> Dict[str, torch.Tensor]:
    dev = ref.device
    lib = L.lib()
    need = int(lib.seeme_hyp_metrics_workspace_bytes(B, K, T))
    ws = _WS.get(need, dev)
    per_hyp = torch.empty(3, B, max(K, 0), device=dev, dtype=torch.float32)
    per_seq = torch.empty(2, B, device=dev, dtype=torch.float32)
    L.call("seeme_hyp_metrics", pred.data_ptr(), ref.data_ptr(), lens.data_ptr(), B, K, T, per_hyp.data_ptr(), per_seq.data_ptr(),
           ws.data_ptr(), need if ws_bytes is None else ws_bytes, L.current_stream())
    out = {n: per_hyp[i] for i, n in enumerate(PER_HYP)}
    out.update({n: per_seq[i] for i, n in enumerate(PER_SEQ)})
    return out


def _medoid(dist):
    """argmin over i of the row sums (taken in j order), lowest index on a tie; dist [B,K,K] -> [B] int64."""
    K = dist.shape[1]
    rows = torch.zeros_like(dist[:, :, 0])
    for j in range(K):
        rows = rows + dist[:, :, j]
    ks = torch.arange(K, device=dist.device).expand_as(rows)
    idx = torch.where(rows == rows.min(dim=1, keepdim=True).values, ks, torch.full_like(ks, K)).min(dim=1).values
    return torch.where(idx < K, idx, torch.zeros_like(idx))          # (a row of NaNs has no minimum: 0, as the kernel)


def hyp_pairdist_torch(jts_pred_all, lengths) -> Dict[str, torch.Tensor]:
    """jts_pred_all [B,K,T,24,3], any float dtype, any device, any K; lengths are clamped to 0..T."""
    B, K, T = jts_pred_all.shape[:3]
    dev, dt = jts_pred_all.device, jts_pred_all.dtype
    lens = torch.as_tensor(lengths, device=dev).reshape(B).clamp(0, T)
    dist = torch.zeros(B, K, K, device=dev, dtype=dt)
    iu = torch.triu_indices(K, K, offset=1, device=dev)
    for b in range(B):                       # per sequence: the pair tensor is [L,K,K,24,3]
        n = int(lens[b])
        if n == 0 or K == 1:
            continue
        a = _align(jts_pred_all[b])[:, :n].transpose(0, 1)                            # [L,K,24,3]
        d = (a[:, :, None] - a[:, None, :]).norm(dim=-1).sum(dim=(0, 3)) / 24 / n * 1000.0      # [K,K]
        dist[b, iu[0], iu[1]] = d[iu[0], iu[1]]                                       # every unordered pair once, mirrored
        dist[b, iu[1], iu[0]] = d[iu[0], iu[1]]
    return {"PAIR_DIST": dist, "medoid_index": _medoid(dist)}


def hyp_pairdist_hip(jts_pred_all, lengths) -> Dict[str, torch.Tensor]:
    """jts_pred_all [B,K,T,24,3] fp32 on the device, K <= 32 (``hyp_pairdist_torch`` serves K > 32)."""
    L.require_cuda(jts_pred_all, "jts_pred_all")
    if jts_pred_all.dim() != 5 or tuple(jts_pred_all.shape[3:]) != (24, 3):
        raise L.SeemeError(f"hyp_pairdist: joints are {tuple(jts_pred_all.shape)}: expected [B,K,T,24,3]")
    B, K, T = (int(n) for n in jts_pred_all.shape[:3])
    lens = torch.as_tensor(lengths).reshape(B).to(device=jts_pred_all.device, dtype=torch.int32)
    return _launch_pairdist(jts_pred_all.contiguous(), lens, B, K, T)


def _launch_pairdist(pred, lens, B, K, T, ws_bytes=None) -> Dict[str, torch.Tensor]:
    dev = lens.device
    lib = L.lib()
    need = int(lib.seeme_hyp_pairdist_workspace_bytes(B, K, T))
    ws = _WS.get(need, dev)
    dist = torch.empty(B, max(K, 0), max(K, 0), device=dev, dtype=torch.float32)
    medoid = torch.empty(B, device=dev, dtype=torch.int32)
    L.call("seeme_hyp_pairdist", pred.data_ptr(), lens.data_ptr(), B, K, T, dist.data_ptr(), medoid.data_ptr(), ws.data_ptr(),
           need if ws_bytes is None else ws_bytes, L.current_stream())
    return {"PAIR_DIST": dist, "medoid_index": medoid.long()}


SELECT_MODES = ("first", "medoid")


def check_select(mode, what: str) -> str:
    if mode not in SELECT_MODES:
        raise ValueError(f"{what} must be one of {SELECT_MODES}, got {mode!r}")
    return mode


def select_index(hm: Dict[str, torch.Tensor], mode: str) -> torch.Tensor:
    """The hypothesis that stands for its sequence, [B] int64: 'first' hypothesis 0, 'medoid' ``hm['medoid_index']``."""
    check_select(mode, "mode")
    if mode == "medoid":
        return hm["medoid_index"].long()
    return torch.zeros(hm["MPJPE"].shape[0], dtype=torch.int64, device=hm["MPJPE"].device)


def keep_mask(m: Dict[str, torch.Tensor], split: str, have_quat: bool) -> torch.Tensor:
    """Inclusion per (b,k) as ``EgoMetrics.update`` decides it per sequence (compute.py:488-517,567-576): on 'test' with quaternions
    ACCL > 0, head error < 0.9 and root error < 300 mm; otherwise ACCL > 0."""
    keep = m["ACCL"] > 0
    if split == "test" and have_quat:
        keep = keep & (m["HEAD_ORIENTATION_ERROR"] < 0.9) & (m["ROOT_ERROR"] < 300.0)
    return keep


def best_index(mpjpe: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """argmin of MPJPE over the kept hypotheses, lowest k on a tie, -1 when none is kept.  [B] int64."""
    K = mpjpe.shape[1]
    v = torch.where(keep, mpjpe, torch.full_like(mpjpe, float("inf")))
    best = v.min(dim=1, keepdim=True).values
    ks = torch.arange(K, device=mpjpe.device).expand_as(v)
    idx = torch.where((v == best) & keep, ks, torch.full_like(ks, K)).min(dim=1).values
    return torch.where(idx < K, idx, torch.full_like(idx, -1))


class HypothesisMetrics:
    """Running sums of the K-hypothesis statistics, one float64 device vector of six entries (reduced over ranks like EgoMetrics'
    sums): [sum best-of-K MPJPE, sum mean-of-K MPJPE, sum APD, sum STD, sequences with a kept hypothesis, sequences].  K is not
    part of the vector: ``compute(sums, num_hypotheses=)`` takes it from the caller (the model's setting) or, by default, from the
    last update of this object."""

    NAMES = ("MPJPE_best_of_k", "MPJPE_mean_of_k", "APD_JOINTS", "STD_JOINTS")

    def __init__(self):
        self.reset()

    def reset(self):
        self._sums = None
        self.num_hypotheses = 0

    def update(self, hm: Dict[str, torch.Tensor], split: str = "test"):
        """hm: ``rs['hyp_metrics']`` of ``MLD.ego_eval`` (MPJPE, ROOT_ERROR, ACCL, HEAD_ORIENTATION_ERROR [B,K], APD_JOINTS,
        STD_JOINTS [B]; ``have_quat`` False when the data type has no orientation quaternions)."""
        mp = hm["MPJPE"]
        K = int(mp.shape[1])
        if self.num_hypotheses not in (0, K):
            raise ValueError(f"HypothesisMetrics: {K} hypotheses after {self.num_hypotheses}; reset() between settings")
        self.num_hypotheses = K
        keep = keep_mask(hm, split, bool(hm.get("have_quat", True)) and "HEAD_ORIENTATION_ERROR" in hm)
        n = keep.sum(dim=1)
        any_ = n > 0
        mpd = mp.double()
        zero = torch.zeros_like(mpd[:, 0])
        best = torch.where(any_, torch.where(keep, mpd, torch.full_like(mpd, float("inf"))).min(dim=1).values, zero)
        mean = torch.where(any_, (mpd * keep).sum(dim=1) / n.clamp_min(1), zero)
        vals = torch.stack([best.sum(), mean.sum(), hm["APD_JOINTS"].double().sum(), hm["STD_JOINTS"].double().sum(),
                            any_.sum().double(), torch.tensor(float(mp.shape[0]), dtype=torch.float64, device=mp.device)])
        self._sums = vals if self._sums is None else self._sums + vals

    def sums(self):
        return torch.zeros(6, dtype=torch.float64) if self._sums is None else self._sums

    def compute(self, sums=None, num_hypotheses=None):
        s = (self.sums() if sums is None else sums).detach().double().cpu()
        K = self.num_hypotheses if num_hypotheses is None else num_hypotheses
        nk, nb = max(float(s[4]), 1.0), max(float(s[5]), 1.0)
        return {"MPJPE_best_of_k": float(s[0]) / nk, "MPJPE_mean_of_k": float(s[1]) / nk, "APD_JOINTS": float(s[2]) / nb,
                "STD_JOINTS": float(s[3]) / nb, "count_seq_k": float(s[4]), "num_hypotheses": float(K)}


class SelectionMetrics:
    """Running sums of the errors of the SELECTED hypothesis (``hm['selected_index']``, TEST.HYP_SELECT), one float64 device vector
    of eight entries (reduced over ranks like HypothesisMetrics' sums): [sum MPJPE, sum ROOT_ERROR, sum ACCL, counted sequences,
    counted sequences whose selection is also best_index, sum PA-MPJPE, sum V2V, counted sequences with mesh metrics].  A sequence is
    counted when its selected hypothesis passes ``keep_mask`` for the split -- the rule EgoMetrics applies to a single prediction."""

    NAMES = ("MPJPE_medoid", "ROOT_ERROR_medoid", "ACCL_medoid")
    MESH_NAMES = ("PA_MPJPE_medoid", "V2V_medoid")

    def __init__(self):
        self.reset()

    def reset(self):
        self._sums = None

    def update(self, hm: Dict[str, torch.Tensor], split: str = "test", mesh: Dict[str, torch.Tensor] = None):
        """hm: ``rs['hyp_metrics']`` with ``selected_index`` and ``best_index`` (of the same split); mesh: ``rs['mesh_metrics']``."""
        sel = hm["selected_index"].long()[:, None]
        keep = keep_mask(hm, split, bool(hm.get("have_quat", True)) and "HEAD_ORIENTATION_ERROR" in hm).gather(1, sel)[:, 0]
        at = lambda x: (x.double().gather(1, sel)[:, 0] * keep).sum()
        n = keep.sum().double()
        vals = [at(hm["MPJPE"]), at(hm["ROOT_ERROR"]), at(hm["ACCL"]), n, ((hm["best_index"] == sel[:, 0]) & keep).sum().double()]
        if mesh is not None:
            vals += [at(mesh["PA_MPJPE"]), at(mesh["V2V"]), n]
        else:
            z = torch.zeros((), dtype=torch.float64, device=sel.device)
            vals += [z, z, z]
        vals = torch.stack(vals)
        self._sums = vals if self._sums is None else self._sums + vals

    def sums(self):
        return torch.zeros(8, dtype=torch.float64) if self._sums is None else self._sums

    def compute(self, sums=None):
        s = (self.sums() if sums is None else sums).detach().double().cpu()
        n = max(float(s[3]), 1.0)
        out = {name: float(s[i]) / n for i, name in enumerate(self.NAMES)}
        out["count_seq_medoid"] = float(s[3])
        out["medoid_is_best_ratio"] = float(s[4]) / n
        if float(s[7]) > 0:           # the mesh numbers exist only when an update had mesh metrics
            out["PA_MPJPE_medoid"], out["V2V_medoid"] = float(s[5]) / float(s[7]), float(s[6]) / float(s[7])
        return out
