"""Interpersonal distance and mutual gaze: how the wearer stands to the interactee, and the evaluation broken down by it.

``social_metrics_hip``   one pass of ``seeme_social_metrics`` (csrc/social_metrics.hip): K <= 32, fp32, on the device.
``social_metrics_torch`` the plain-torch twin (any float dtype, any device, any K), in chunks of frames so that the [.,24,24,3] pair
                         tensor stays small: the test reference, and what serves K > 32.  ``MLD.ego_eval`` uses the kernel.
``bin_index``            the bin of a value among edges e_1 < ... < e_m.
``SocialMetrics``        running sums of the binned evaluation (TEST.SOCIAL_METRICS).

Definitions (include/seeme_hip.h states them once; this repeats them).  Inputs, in the coordinates ``MLD.ego_eval`` already has -- there
is NO alignment of any kind, the two people share the batch's frame and their relative placement is the thing measured:

  jts_pred [B,K,T,24,3] joints of the K hypotheses        quat_pred [B,K,T,4] their global orientation, (w,x,y,z)
  jts_ref  [B,T,24,3]   the wearer's reference joints     quat_ref  [B,T,4]   the reference's global orientation
  jts_int  [B,T,24,3]   the interactee's joints           quat_int  [B,T,4]   the interactee's global orientation
  lengths  [B]          n = clamp(len, 0, T) valid frames; every mean runs over the frames t < n; n = 0 gives zeros

Per frame, for a body x with orientation q:

  d(x) = |x[0] - int[0]|                                        pelvis-to-pelvis distance
  c(x) = min over the 24 x 24 joint pairs of |x[i] - int[j]|    closest approach
  g(q) = third column of the rotation matrix of q, normalised as ``EgoMetrics.quat_to_rotmat`` does; a degenerate quaternion is the
         identity by that function's rule
  a(q) = min(atan2(|g(q) x g(q_int)|, g(q) . g(q_int)) * 180/pi, 180)   degrees in [0, 180]: the reference's arccos of the normalised
         dot product (mld/models/metrics/compute.py:31) in the form that stays accurate at 0 and 180 degrees

Per sequence [B], from the reference body (what the bins are made of; they do not depend on any prediction):

  PERSON_DIST = 1000 mean d(ref) (mm)    CLOSEST_DIST_REF = 1000 mean c(ref) (mm)    GAZE_ANGLE_REF = mean a(q_ref) (degrees)

Per hypothesis [B,K]:

  PERSON_DIST_ERROR = 1000 mean |d(pred_k) - d(ref)|    CLOSEST_DIST = 1000 mean c(pred_k)    CLOSEST_DIST_ERROR = 1000 mean |c(pred_k) - c(ref)|
  GAZE_ANGLE = mean a(q_pred_k)                         GAZE_ANGLE_ERROR = mean |a(q_pred_k) - a(q_ref)|

The reference's ``person_dist`` (compute.py:458) subtracts the wearer's first-frame head from the wearer's pelvis only, so it mixes two
frames; PERSON_DIST does not follow it.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence

import torch

from . import _lib as L

K_MAX = 32
FRAME_CHUNK = 8                      # SEEME_SOCIAL_FRAME_CHUNK: frames of one workgroup of seeme_social_metrics
PER_HYP = ("PERSON_DIST_ERROR", "CLOSEST_DIST", "CLOSEST_DIST_ERROR", "GAZE_ANGLE", "GAZE_ANGLE_ERROR")
PER_SEQ = ("PERSON_DIST", "CLOSEST_DIST_REF", "GAZE_ANGLE_REF")
MAX_EDGES = 8
DEFAULT_DIST_EDGES = (1000.0, 2000.0, 3000.0)     # mm; compute.py:555 filters at 2000 and 3000
DEFAULT_GAZE_EDGES = (150.0,)                     # degrees; within 30 degrees of opposite gaze directions (the reference's threshold)


# ----------------------------------------------------------------------------- the plain-torch twin
def _gaze(q):
    """[...,4] -> [...,3]: the third column of the rotation matrix."""
    from .mld import EgoMetrics
    return EgoMetrics.quat_to_rotmat(q.reshape(-1, 4))[:, :, 2].reshape(*q.shape[:-1], 3)


def _angle(g, h):
    # every product of the cross product is rounded on its own (separate tensor operations, never a fused multiply-add): parallel
    # and antiparallel directions give exactly 0 and exactly 180
    g0, g1, g2 = g.unbind(-1)
    h0, h1, h2 = h.unbind(-1)
    cross = torch.stack([g1 * h2 - g2 * h1, g2 * h0 - g0 * h2, g0 * h1 - g1 * h0], dim=-1)
    a = torch.atan2(cross.norm(dim=-1), (g * h).sum(-1)) * (180.0 / math.pi)
    return a.clamp_max(180.0)


def social_metrics_torch(jts_pred, jts_ref, jts_int, quat_pred, quat_ref, quat_int, lengths, frame_chunk: int = 16) -> Dict[str, torch.Tensor]:
    """Any float dtype (that of jts_ref), any device, any K."""
    B, K, T = (int(n) for n in jts_pred.shape[:3])
    dev, dt = jts_ref.device, jts_ref.dtype
    n = torch.as_tensor(lengths, device=dev).reshape(B).clamp(0, T)
    mask = (torch.arange(T, device=dev)[None, :] < n[:, None]).to(dt)                  # [B,T]
    bodies = torch.cat([jts_pred.to(dt), jts_ref[:, None]], dim=1)                      # [B,K+1,T,24,3], row K the reference
    jts_int = jts_int.to(dt)
    d = (bodies[:, :, :, 0] - jts_int[:, None, :, 0]).norm(dim=-1)                      # [B,K+1,T]
    c = torch.empty_like(d)
    for t0 in range(0, T, frame_chunk):
        x, y = bodies[:, :, t0:t0 + frame_chunk], jts_int[:, None, t0:t0 + frame_chunk]
        c[:, :, t0:t0 + frame_chunk] = (x[..., :, None, :] - y[..., None, :, :]).norm(dim=-1).flatten(-2).min(dim=-1).values
    q = torch.cat([quat_pred.to(dt).reshape(B, K, T, 4), quat_ref.to(dt).reshape(B, 1, T, 4)], dim=1)
    a = _angle(_gaze(q), _gaze(quat_int.to(dt).reshape(B, 1, T, 4)))                     # [B,K+1,T]
    nf = n.to(dt)
    mean = lambda v: torch.where(nf > 0, (v * mask).sum(-1) / nf.clamp_min(1), torch.zeros_like(nf))        # [B,T] -> [B]
    meank = lambda v: torch.where(nf[:, None] > 0, (v * mask[:, None]).sum(-1) / nf[:, None].clamp_min(1),
                                  torch.zeros_like(nf)[:, None].expand(B, K))            # [B,K,T] -> [B,K]
    return {"PERSON_DIST": 1000.0 * mean(d[:, K]), "CLOSEST_DIST_REF": 1000.0 * mean(c[:, K]), "GAZE_ANGLE_REF": mean(a[:, K]),
            "PERSON_DIST_ERROR": 1000.0 * meank((d[:, :K] - d[:, K:]).abs()), "CLOSEST_DIST": 1000.0 * meank(c[:, :K]),
            "CLOSEST_DIST_ERROR": 1000.0 * meank((c[:, :K] - c[:, K:]).abs()), "GAZE_ANGLE": meank(a[:, :K]),
            "GAZE_ANGLE_ERROR": meank((a[:, :K] - a[:, K:]).abs())}


# ----------------------------------------------------------------------------- the kernel
_WS = L.Workspace(per_stream=True)


def social_metrics_hip(jts_pred, jts_ref, jts_int, quat_pred, quat_ref, quat_int, lengths) -> Dict[str, torch.Tensor]:
    """fp32 on the device, K <= 32.  The quaternions may come flat ([B*K*T,4], [B*T,4]), as ``MLD.ego_eval`` holds them."""
    names = ("jts_pred", "jts_ref", "jts_int", "quat_pred", "quat_ref", "quat_int")
    for t, name in zip((jts_pred, jts_ref, jts_int, quat_pred, quat_ref, quat_int), names):
        L.require_cuda(t, name)
    if jts_pred.dim() != 5 or tuple(jts_pred.shape[3:]) != (24, 3):
        raise L.SeemeError(f"social_metrics: jts_pred is {tuple(jts_pred.shape)}: expected [B,K,T,24,3]")
    B, K, T = (int(n) for n in jts_pred.shape[:3])
    if tuple(jts_ref.shape) != (B, T, 24, 3) or tuple(jts_int.shape) != (B, T, 24, 3):
        raise L.SeemeError(f"social_metrics: jts_ref / jts_int are {tuple(jts_ref.shape)} / {tuple(jts_int.shape)}: expected {(B, T, 24, 3)}")
    if quat_pred.numel() != B * K * T * 4 or quat_ref.numel() != B * T * 4 or quat_int.numel() != B * T * 4:
        raise L.SeemeError(f"social_metrics: quaternions have {quat_pred.numel()} / {quat_ref.numel()} / {quat_int.numel()} values: "
                           f"expected [B,K,T,4] / [B,T,4] / [B,T,4] for B, K, T = {B}, {K}, {T}")
    lens = torch.as_tensor(lengths).reshape(B).to(device=jts_ref.device, dtype=torch.int32)
    return _launch(jts_pred.contiguous(), jts_ref.contiguous(), jts_int.contiguous(), quat_pred.contiguous(), quat_ref.contiguous(),
                   quat_int.contiguous(), lens, B, K, T)


def _launch(pred, ref, intr, qp, qr, qi, lens, B, K, T, ws_bytes=None) -> Dict[str, torch.Tensor]:
    dev = ref.device
    need = int(L.lib().seeme_social_metrics_workspace_bytes(B, K, T))
    ws = _WS.get(need, dev)
    per_hyp = torch.empty(len(PER_HYP), B, max(K, 0), device=dev, dtype=torch.float32)
    per_seq = torch.empty(len(PER_SEQ), B, device=dev, dtype=torch.float32)
    L.call("seeme_social_metrics", pred.data_ptr(), ref.data_ptr(), intr.data_ptr(), qp.data_ptr(), qr.data_ptr(), qi.data_ptr(),
           lens.data_ptr(), B, K, T, per_hyp.data_ptr(), per_seq.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes,
           L.current_stream())
    out = {n: per_seq[i] for i, n in enumerate(PER_SEQ)}
    out.update({n: per_hyp[i] for i, n in enumerate(PER_HYP)})
    return out


# ----------------------------------------------------------------------------- bins
def check_edges(edges, what: str, lo: float = None, hi: float = None) -> tuple:
    """A list of at most MAX_EDGES finite, strictly increasing numbers (inside the open interval (lo, hi) when given) -> tuple of
    floats; anything else is a ValueError that names `what`."""
    if not isinstance(edges, (list, tuple)) or not 1 <= len(edges) <= MAX_EDGES:
        raise ValueError(f"{what} must be a list of 1..{MAX_EDGES} numbers, got {edges!r}")
    for e in edges:
        if isinstance(e, bool) or not isinstance(e, (int, float)) or not math.isfinite(e):
            raise ValueError(f"{what} must hold finite numbers, got {edges!r}")
        if (lo is not None and not e > lo) or (hi is not None and not e < hi):
            raise ValueError(f"{what} must lie inside ({lo}, {hi}), got {edges!r}")
    if any(not a < b for a, b in zip(edges[:-1], edges[1:])):
        raise ValueError(f"{what} must be strictly increasing, got {edges!r}")
    return tuple(float(e) for e in edges)


def bin_index(values, edges: Sequence[float]) -> torch.Tensor:
    """The number of edges <= value, int64: edges e_1 < ... < e_m give m+1 bins [e_i, e_{i+1}), the first and the last open."""
    values = torch.as_tensor(values)
    e = torch.as_tensor([float(x) for x in edges], dtype=torch.float64, device=values.device)
    return torch.bucketize(values.double(), e, right=True)


def bin_labels(edges: Sequence[float]) -> list:
    """lt<e_1>, <e_1>_<e_2>, ..., ge<e_m>."""
    s = [f"{float(e):g}" for e in edges]
    return [f"lt{s[0]}"] + [f"{a}_{b}" for a, b in zip(s[:-1], s[1:])] + [f"ge{s[-1]}"]


class SocialMetrics:
    """Running sums of the evaluation by interpersonal distance and mutual gaze, one float64 device vector (reduced over ranks like the
    other accumulators):

      [0:3]  sums of PERSON_DIST, CLOSEST_DIST_REF, GAZE_ANGLE_REF over all sequences       [3]  sequences
      [4:8]  sums of PERSON_DIST_ERROR, CLOSEST_DIST, CLOSEST_DIST_ERROR, GAZE_ANGLE_ERROR over the kept (b,k) pairs     [8]  kept pairs
      then four entries per bin, the bins of PERSON_DIST first and those of GAZE_ANGLE_REF after them:
        K = 1: [sum MPJPE, sum ROOT_ERROR, counted sequences, all sequences of the bin]
        K > 1: [sum best-of-K MPJPE, sum mean-of-K MPJPE, sequences with a kept hypothesis, all sequences of the bin]

    `keep` [B,K] is the inclusion mask of the split (``hyp_metrics.keep_mask``): for K = 1 the sequences ``EgoMetrics.update`` counts
    for MPJPE, for K > 1 the rule of ``HypothesisMetrics.update``.  Summed over the bins of either axis the first three entries are
    therefore EgoMetrics' MPJPE sum, ROOT_ERROR sum and count (K = 1) or HypothesisMetrics' entries 0, 1 and 4 (K > 1).  K is not part
    of the vector: ``compute(sums, num_hypotheses=)`` takes it from the caller or, by default, from the last update."""

    UNBINNED_SEQ = PER_SEQ
    UNBINNED_HYP = ("PERSON_DIST_ERROR", "CLOSEST_DIST", "CLOSEST_DIST_ERROR", "GAZE_ANGLE_ERROR")
    AXES = (("dist", "PERSON_DIST"), ("gaze", "GAZE_ANGLE_REF"))

    def __init__(self, dist_edges=DEFAULT_DIST_EDGES, gaze_edges=DEFAULT_GAZE_EDGES):
        self.edges = {"dist": check_edges(list(dist_edges), "dist_edges"), "gaze": check_edges(list(gaze_edges), "gaze_edges", 0.0, 180.0)}
        self.reset()

    def reset(self):
        self._sums = None
        self.num_hypotheses = 0

    def __len__(self):
        return 9 + 4 * sum(len(e) + 1 for e in self.edges.values())

    def update(self, sm: Dict[str, torch.Tensor], mpjpe: torch.Tensor, root_error: torch.Tensor, keep: torch.Tensor):
        """sm: ``rs['social_metrics']`` of ``MLD.ego_eval``; mpjpe, root_error, keep [B,K] (root_error is read for K = 1 only)."""
        K = int(mpjpe.shape[1])
        if self.num_hypotheses not in (0, K):
            raise ValueError(f"SocialMetrics: {K} hypotheses after {self.num_hypotheses}; reset() between settings")
        self.num_hypotheses = K
        dev = mpjpe.device
        keep = keep.to(dev)
        kd = keep.double()
        n = keep.sum(dim=1)
        any_ = n > 0
        mpd = mpjpe.double()
        zero = torch.zeros_like(mpd[:, 0])
        if K == 1:
            first, second = mpd[:, 0] * kd[:, 0], root_error.double()[:, 0] * kd[:, 0]
        else:                                                               # HypothesisMetrics.update, term for term
            first = torch.where(any_, torch.where(keep, mpd, torch.full_like(mpd, float("inf"))).min(dim=1).values, zero)
            second = torch.where(any_, (mpd * keep).sum(dim=1) / n.clamp_min(1), zero)
        cols = torch.stack([first, second, any_.double(), torch.ones_like(zero)], dim=1)                    # [B,4]
        count = lambda x: torch.tensor(float(x), dtype=torch.float64, device=dev)
        vals = [sm[name].double().sum() for name in self.UNBINNED_SEQ] + [count(mpjpe.shape[0])]
        vals += [(sm[name].double() * kd).sum() for name in self.UNBINNED_HYP] + [kd.sum()]
        vals = [torch.stack(vals)]
        for axis, name in self.AXES:
            idx = bin_index(sm[name], self.edges[axis])
            onehot = (idx[:, None] == torch.arange(len(self.edges[axis]) + 1, device=dev)[None, :]).double()       # [B,bins]
            vals.append((onehot[:, :, None] * cols[:, None, :]).sum(dim=0).reshape(-1))                            # fixed order: no atomics
        vals = torch.cat(vals)
        self._sums = vals if self._sums is None else self._sums + vals

    def sums(self):
        return torch.zeros(len(self), dtype=torch.float64) if self._sums is None else self._sums

    def compute(self, sums=None, num_hypotheses=None) -> Dict[str, float]:
        s = (self.sums() if sums is None else sums).detach().double().cpu()
        if s.numel() != len(self):
            raise ValueError(f"SocialMetrics.compute: {s.numel()} sums, this object's edges need {len(self)}")
        K = self.num_hypotheses if num_hypotheses is None else num_hypotheses
        names = ("MPJPE", "ROOT_ERROR") if K <= 1 else ("MPJPE_best_of_k", "MPJPE_mean_of_k")
        out = {}
        if float(s[3]) > 0:
            out.update({n: float(s[i]) / float(s[3]) for i, n in enumerate(self.UNBINNED_SEQ)})
        if float(s[8]) > 0:
            out.update({n: float(s[4 + i]) / float(s[8]) for i, n in enumerate(self.UNBINNED_HYP)})
        out["count_seq_social"], out["count_pairs_social"] = float(s[3]), float(s[8])
        at = 9
        for axis, _ in self.AXES:
            for label in bin_labels(self.edges[axis]):
                a, b, kept, every = (float(x) for x in s[at:at + 4])
                at += 4
                out[f"count_seq_{axis}_{label}"] = every
                out[f"count_kept_{axis}_{label}"] = kept
                if kept > 0:
                    out[f"{names[0]}_{axis}_{label}"], out[f"{names[1]}_{axis}_{label}"] = a / kept, b / kept
        return out
