"""One coherent interactee track from the flow head's samples at the STORED frames of a recording (``estimate.py --track``).

The flow head (``prohmr_head``) gives S candidate bodies with their log-density at each of the Lf stored frames idx [Lf] of a
recording of L frames.  The track is the most probable state sequence of an HMM: the emission term is the flow's log-density, the
transition a Gaussian random walk of every joint with a standard deviation of ``step_mm`` per frame whose variance grows linearly
over a gap; both in nats.  The chosen bodies are then filled to all L frames and smoothed:

``track_cost_hip``     ``seeme_track_cost``: cost [Lf-1,S,S] = weight * sum over the 24 joints of |a - b|^2 / (idx[l+1] - idx[l]).
``track_filter_hip``   ``seeme_track_filter``: keys [Lf,J,3] (+ translation) -> [L,J,3]: between two keys the sign-aligned slerp of
                       ``seeme_stitch_windows``, before the first / after the last key that key, then a symmetric FIR over the
                       sign-aligned quaternions (the translation: a plain weighted mean), truncated at the recording's ends.
``*_torch``            their plain-torch twins (any float dtype, any device): in float64 the test references.
``track_interactee``   joints (``seeme_smpl_lbs``, joints only) -> costs -> ``recording.path_select_hip`` -> gather -> filter.

The definitions are stated once, in include/seeme_hip.h.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import geometry as G
from . import recording as R

TRACK_TILE = 64              # SEEME_TRACK_TILE: output frames of one workgroup of seeme_track_filter
S_MAX, R_MAX, J_MAX = 32, 32, 32
SIGMA_MAX = 10.0
# Not tuned on data (there is no dataset of headset video with a tracked interactee here): 20 mm per frame is about 0.6 m/s at 30 fps.
DEFAULT_STEP_MM, DEFAULT_PRIOR_WEIGHT, DEFAULT_SIGMA = 20.0, 1.0, 2.0


# ----------------------------------------------------------------------------- host-side checks
def _number(v, name: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def check_step_mm(v, name: str = "TEST.TRACK_STEP_MM") -> float:
    if not _number(v, name) > 0:
        raise ValueError(f"{name} must be a finite number > 0 (mm per frame), got {v!r}")
    return float(v)


def check_prior_weight(v, name: str = "TEST.TRACK_PRIOR_WEIGHT") -> float:
    if not _number(v, name) >= 0:
        raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    return float(v)


def check_sigma(v, name: str = "TEST.TRACK_SIGMA") -> float:
    if not 0 <= _number(v, name) <= SIGMA_MAX:
        raise ValueError(f"{name} must be a number in 0..{SIGMA_MAX:g} (frames), got {v!r}")
    return float(v)


def gaussian_taps(sigma) -> np.ndarray:
    """float32 [R+1]: exp(-d^2 / (2 sigma^2)) for d = 0 .. R = ceil(3 sigma), computed in float64; sigma == 0 gives [1.].  The filter
    divides by the taps' sum over its (truncated) window, so they are not normalised here."""
    sigma = check_sigma(sigma, "gaussian_taps: sigma")
    if sigma == 0:
        return np.ones(1, np.float32)
    d = np.arange(int(math.ceil(3.0 * sigma)) + 1, dtype=np.float64)
    return np.exp(-d * d / (2.0 * sigma * sigma)).astype(np.float32)


def check_idx(idx, L_: Optional[int], what: str = "track") -> np.ndarray:
    """idx -> int64 numpy [Lf]: integers, strictly increasing, inside 0..L-1 (when L is given); a ValueError names idx otherwise."""
    a = idx.detach().cpu().numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
    if a.ndim != 1 or a.shape[0] < 1 or a.dtype.kind not in "iu":
        raise ValueError(f"{what}: idx is {a.shape} {a.dtype}: expected integers [Lf], Lf >= 1")
    a = a.astype(np.int64)
    if (np.diff(a) <= 0).any():
        raise ValueError(f"{what}: idx must be strictly increasing, got {a[:8].tolist()}{' ...' if a.shape[0] > 8 else ''}")
    if a[0] < 0 or (L_ is not None and a[-1] >= L_):
        raise ValueError(f"{what}: idx must lie inside 0..{'L-1' if L_ is None else L_ - 1}, got {int(a[0])} .. {int(a[-1])}")
    return a


def _check_taps(taps, what: str) -> np.ndarray:
    t = np.asarray(taps.detach().cpu().numpy() if isinstance(taps, torch.Tensor) else taps, np.float64).reshape(-1)
    if not 1 <= t.shape[0] <= R_MAX + 1:
        raise ValueError(f"{what}: {t.shape[0]} taps: expected R + 1 of them, R in 0..{R_MAX}")
    if not np.isfinite(t).all() or (t < 0).any() or not t[0] > 0:
        raise ValueError(f"{what}: every tap must be finite and >= 0 and taps[0] > 0, got {t.tolist()}")
    return t


# ----------------------------------------------------------------------------- torch twins
def track_cost_torch(jts, idx, weight: float) -> torch.Tensor:
    """jts [Lf,S,24,3] (metres), idx [Lf], any float dtype, any device, any S -> cost [Lf-1,S,S]."""
    if jts.dim() != 4 or tuple(jts.shape[2:]) != (24, 3):
        raise ValueError(f"track_cost: joints are {tuple(jts.shape)}: expected [Lf,S,24,3]")
    Lf, S = int(jts.shape[0]), int(jts.shape[1])
    at = torch.from_numpy(check_idx(idx, None, "track_cost")).to(jts.device)
    if at.shape[0] != Lf:
        raise ValueError(f"track_cost: idx has {at.shape[0]} entries for {Lf} key frames")
    cost = torch.zeros(max(Lf - 1, 0), S, S, device=jts.device, dtype=jts.dtype)
    gap = (at[1:] - at[:-1]).to(jts.dtype)
    step = max(1, (1 << 24) // (S * S * 72))              # pairs of key frames per pass: the pair tensor is [step,S,S,24,3]
    for lo in range(0, Lf - 1, step):
        hi = min(lo + step, Lf - 1)
        d = jts[lo:hi, :, None] - jts[lo + 1:hi + 1, None, :]
        cost[lo:hi] = weight * (d * d).sum(dim=-1).sum(dim=-1) / gap[lo:hi, None, None]
    return cost


def _fill_torch(pose, transl, at, L_: int):
    """fill(m) of include/seeme_hip.h for m = 0..L-1: quaternions [L,J,4], translation [L,3] or None, and key [L] bool."""
    Lf = at.shape[0]
    m = torch.arange(L_, device=pose.device)
    a = (torch.searchsorted(at, m, right=True) - 1).clamp(0, Lf - 1)            # the last key at or before m (0 before the first)
    b = (a + 1).clamp(max=Lf - 1)
    inside = (m > at[a]) & (b > a)                                               # strictly between keys a and a + 1
    gap = (at[b] - at[a]).clamp(min=1).to(pose.dtype)
    u = torch.where(inside, (m - at[a]).to(pose.dtype) / gap, torch.zeros_like(gap))
    qa, qb = R._aa_to_quat(pose[a]), R._aa_to_quat(pose[b])
    q = torch.where(inside[:, None, None], R._blend(qa, qb, u[:, None, None]), qa)
    t = None
    if transl is not None:
        t = torch.where(inside[:, None], transl[a] + u[:, None] * (transl[b] - transl[a]), transl[a])
    return q, t, m == at[a]


def track_filter_torch(pose, transl, idx, L_: int, taps):
    """pose [Lf,J,3] axis-angle keys, transl [Lf,3] or None, idx [Lf], taps [R+1] -> (pose_out [L,J,3], transl_out [L,3] or None):
    the definition of ``seeme_track_filter``.  Any float dtype, any device, any J."""
    if pose.dim() != 3 or pose.shape[2] != 3 or pose.shape[1] < 1:
        raise ValueError(f"track_filter: pose is {tuple(pose.shape)}: expected [Lf,J,3]")
    L_ = int(L_)
    at_np = check_idx(idx, L_, "track_filter")
    Lf = int(pose.shape[0])
    if at_np.shape[0] != Lf or (transl is not None and tuple(transl.shape) != (Lf, 3)):
        raise ValueError(f"track_filter: {Lf} keys, idx has {at_np.shape[0]} entries"
                         + ("" if transl is None else f", transl is {tuple(transl.shape)}") + ": expected [Lf] and [Lf,3]")
    tp = _check_taps(taps, "track_filter")
    Rr = tp.shape[0] - 1
    tp = torch.from_numpy(tp).to(device=pose.device, dtype=pose.dtype)
    at = torch.from_numpy(at_np).to(pose.device)
    q, t, key = _fill_torch(pose, transl, at, L_)
    n = torch.arange(L_, device=pose.device)
    acc = torch.zeros_like(q)
    tacc = None if t is None else torch.zeros_like(t)
    wsum = torch.zeros(L_, device=pose.device, dtype=pose.dtype)
    for d in range(-Rr, Rr + 1):                                                 # increasing frame order
        m = n + d
        ok = ((m >= 0) & (m < L_)).to(pose.dtype)
        mc = m.clamp(0, L_ - 1)
        k = tp[abs(d)] * ok
        qm = q[mc]
        s = torch.where((qm * q).sum(-1, keepdim=True) < 0, -torch.ones_like(qm[..., :1]), torch.ones_like(qm[..., :1]))
        acc = acc + k[:, None, None] * s * qm
        wsum = wsum + k
        if t is not None:
            tacc = tacc + k[:, None] * t[mc]
    out = G.quat_to_aa_torch(R._normalize(acc))
    tout = None if t is None else tacc / wsum[:, None]
    if Rr == 0:                                                                  # a key without a filter: bit for bit
        out = torch.where(key[:, None, None], pose[(torch.searchsorted(at, n, right=True) - 1).clamp(0, Lf - 1)], out)
        if t is not None:
            tout = torch.where(key[:, None], transl[(torch.searchsorted(at, n, right=True) - 1).clamp(0, Lf - 1)], tout)
    return out, tout


# ----------------------------------------------------------------------------- kernels
def track_cost_hip(jts, idx, weight: float) -> torch.Tensor:
    """jts [Lf,S,24,3] fp32 on the device, S <= 32, idx [Lf] (validated on the host) -> cost [Lf-1,S,S]."""
    L.require_cuda(jts, "jts")
    if jts.dim() != 4 or tuple(jts.shape[2:]) != (24, 3):
        raise L.SeemeError(f"track_cost: joints are {tuple(jts.shape)}: expected [Lf,S,24,3]")
    Lf, S = int(jts.shape[0]), int(jts.shape[1])
    at = check_idx(idx, None, "track_cost")
    if at.shape[0] != Lf or at[-1] >= 1 << 31:
        raise ValueError(f"track_cost: idx has {at.shape[0]} entries up to {int(at[-1])} for {Lf} key frames")
    return _launch_cost(jts.contiguous(), torch.from_numpy(at.astype(np.int32)).to(jts.device), Lf, S, float(weight))


def _launch_cost(jts, idx32, Lf, S, weight, out=None) -> torch.Tensor:
    cost = out if out is not None else torch.empty(max(Lf - 1, 0), max(S, 0), max(S, 0), device=jts.device, dtype=torch.float32)
    L.call("seeme_track_cost", L.ptr(jts), L.ptr(idx32), Lf, S, weight, L.ptr(cost), L.current_stream())
    return cost


def track_filter_hip(pose, transl, idx, L_: int, taps):
    """pose [Lf,J,3] fp32 on the device, transl [Lf,3] or None, idx [Lf] (validated on the host: integers, strictly increasing,
    inside 0..L-1), taps [R+1] on the host -> (pose_out [L,J,3], transl_out [L,3] or None).  Launches on the current stream."""
    L.require_cuda(pose, "pose")
    if transl is not None:
        L.require_cuda(transl, "transl")
    if pose.dim() != 3 or pose.shape[2] != 3:
        raise L.SeemeError(f"track_filter: pose is {tuple(pose.shape)}: expected [Lf,J,3]")
    Lf, J = int(pose.shape[0]), int(pose.shape[1])
    L_ = int(L_)
    at = check_idx(idx, L_, "track_filter")
    if at.shape[0] != Lf or (transl is not None and tuple(transl.shape) != (Lf, 3)):
        raise ValueError(f"track_filter: {Lf} keys, idx has {at.shape[0]} entries"
                         + ("" if transl is None else f", transl is {tuple(transl.shape)}") + ": expected [Lf] and [Lf,3]")
    tp = np.asarray(taps.detach().cpu().numpy() if isinstance(taps, torch.Tensor) else taps, np.float32).reshape(-1)
    idx32 = torch.from_numpy(at.astype(np.int32)).to(pose.device)
    return _launch_filter(pose.contiguous(), None if transl is None else transl.contiguous(), idx32, Lf, L_, J, tp, tp.shape[0] - 1)


def _launch_filter(pose, transl, idx32, Lf, L_, J, taps, Rr, out=None):
    """taps: float32 numpy on the host (the library validates them); out: (pose_out, transl_out) to write into (the tests' slots)."""
    dev = pose.device
    if out is None:
        out = (torch.empty(max(L_, 0), max(J, 0), 3, device=dev, dtype=torch.float32),
               None if transl is None else torch.empty(max(L_, 0), 3, device=dev, dtype=torch.float32))
    taps = np.ascontiguousarray(taps, np.float32)
    L.call("seeme_track_filter", L.ptr(pose), L.ptr(transl), L.ptr(idx32), Lf, L_, J,
           taps.ctypes.data_as(C.POINTER(C.c_float)) if taps.size else None, Rr, L.ptr(out[0]), L.ptr(out[1]), L.current_stream())
    return out


# ----------------------------------------------------------------------------- the track
def track_interactee(global_orient, body_pose, transl, log_prob, idx, L_: int, smpl_model, betas, step_mm: float = DEFAULT_STEP_MM,
                     prior_weight: float = DEFAULT_PRIOR_WEIGHT, sigma: float = DEFAULT_SIGMA, device=None) -> Dict[str, torch.Tensor]:
    """global_orient [Lf,S,3], body_pose [Lf,S,69] axis-angle and transl [Lf,3] of the S candidates at the stored frames idx [Lf] of a
    recording of L frames, in ONE coordinate frame (the recording's world frame); log_prob [Lf,S] their log-density (nats); betas
    [10] the body they are posed with.  -> global_orient [L,3], body_pose [L,69], transl [L,3] of the track, path [Lf] int64 (the
    candidate chosen per stored frame), path_cost [] and step_cost [Lf-1] (the transition costs along the path, nats); and what the
    path was chosen from: joints [Lf,S,24,3], cost [Lf-1,S,S], unary [Lf,S].

    The path minimises sum_l unary[l,p_l] + sum_l cost[l,p_l,p_{l+1}] with unary[l,s] = prior_weight * (log_prob[l,0] -
    log_prob[l,s]) and cost = ``track_cost`` of the candidates' SMPL joints at weight 1e6 / (2 step_mm^2): joints in metres, so the
    cost is |a - b|^2 / (2 sigma_gap^2) summed over the joints, with sigma_gap^2 = step_mm^2 x the gap in frames.  The chosen rows
    are filled and filtered by ``track_filter`` with ``gaussian_taps(sigma)``.

    `device`: the ROCm device -> fp32 through the kernels (seeme_smpl_lbs joints, seeme_track_cost, seeme_path_select,
    seeme_track_filter).  None -> the composition of the plain-torch twins in the inputs' dtype, on their device."""
    step_mm, prior_weight = check_step_mm(step_mm, "track_interactee: step_mm"), check_prior_weight(prior_weight, "track_interactee: prior_weight")
    taps = gaussian_taps(sigma)
    L_ = int(L_)
    at = check_idx(idx, L_, "track_interactee")
    Lf, S = int(global_orient.shape[0]), int(global_orient.shape[1])
    want = {"global_orient": (Lf, S, 3), "body_pose": (Lf, S, 69), "transl": (Lf, 3), "log_prob": (Lf, S)}
    for k, v in (("global_orient", global_orient), ("body_pose", body_pose), ("transl", transl), ("log_prob", log_prob)):
        if tuple(v.shape) != want[k]:
            raise ValueError(f"track_interactee: {k} is {tuple(v.shape)}: expected {list(want[k])} (Lf = {Lf}, S = {S})")
    if at.shape[0] != Lf:
        raise ValueError(f"track_interactee: idx has {at.shape[0]} entries for {Lf} stored frames")
    weight = 1e6 / (2.0 * step_mm * step_mm)
    hip = device is not None
    if hip:
        if S > S_MAX:
            raise L.SeemeError(f"track_interactee: {S} candidates per frame: the kernels take 1..{S_MAX}")
        global_orient, body_pose, transl, log_prob = (t.to(device=device, dtype=torch.float32)
                                                      for t in (global_orient, body_pose, transl, log_prob))
    pose = torch.cat([global_orient, body_pose], dim=-1).reshape(Lf * S, 72)
    tr = transl[:, None].expand(Lf, S, 3).reshape(Lf * S, 3)
    b = betas.to(pose).reshape(1, 10).expand(Lf * S, 10)
    if hip:
        from .smpl import smpl_joints_hip
        with torch.no_grad():
            jts = smpl_joints_hip(smpl_model, b.contiguous(), pose.contiguous(), tr.contiguous()).reshape(Lf, S, 24, 3)
        cost = track_cost_hip(jts, at, weight)
    else:
        from .vae_autograd import smpl_joints_torch
        with torch.no_grad():
            jts = smpl_joints_torch(smpl_model, b, pose, tr).reshape(Lf, S, 24, 3)
        cost = track_cost_torch(jts, at, weight)
    unary = (prior_weight * (log_prob[:, :1] - log_prob)).contiguous()
    sel = (R.path_select_hip if hip else R.path_select_torch)(cost, unary)
    path = sel["path"]
    rows = torch.arange(Lf, device=path.device)
    keys = torch.cat([global_orient[rows, path], body_pose[rows, path]], dim=-1).reshape(Lf, 24, 3)
    out, tout = (track_filter_hip if hip else track_filter_torch)(keys, transl.contiguous(), at, L_, taps)
    return {"global_orient": out[:, 0], "body_pose": out[:, 1:].reshape(L_, 69), "transl": tout, "path": path,
            "path_cost": sel["path_cost"], "step_cost": sel["seam_cost"], "cost": cost, "unary": unary, "joints": jts}
