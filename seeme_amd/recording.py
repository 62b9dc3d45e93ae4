"""A whole unlabelled recording: windows, one coherent path through their hypotheses, one stitched motion.

The model sees clips of T frames; a recording is cut into W overlapping windows (``window_plan``), every window gets K hypotheses
(``MLD.predict``), and ONE hypothesis per window is chosen so that neighbouring windows agree on the frames they share:

``overlap_cost_hip``   ``seeme_overlap_cost``: cost [W-1,K,K] (mm), the mean over the O shared frames and the 24 joints of |a - b|,
                       a = hypothesis i of window w at frame T-O+r, b = hypothesis j of window w+1 at frame r.  No alignment: the
                       windows are in ONE coordinate frame and the global position is part of what must agree.
``path_select_hip``    ``seeme_path_select``: the path that minimises sum_w unary[w,p_w] + sum_w cost[w,p_w,p_{w+1}] (dynamic
                       programming, fp32 sums in window order, the lowest index on a tie), its seam costs and its total.
``stitch_windows_hip`` ``seeme_stitch_windows``: the chosen windows' renormed features -> one motion [n_frames,F]; on an overlap frame
                       r takes weight (r+1)/(O+1) for the later window, rotations through unit quaternions (sign-aligned slerp, a
                       normalised lerp above a dot product of ``NLERP_DOT``), the translation by a plain lerp.
``*_torch``            their plain-torch twins (any float dtype, any device, any K): the test references, and what serves K > 32.

``scene_views_hip``    ``seeme_scene_views``: the view-dependent selection of a scene mesh's vertices (into the view's frame, z > 0, every
                       k-th survivor, the first P) for W camera poses in one call; ``scene_views_torch`` is its twin.
``reframe_smpl`` / ``reframe_rot6d`` / ``reframe_joints``: a rigid map p -> A p + a applied to SMPL parameters and to joints, plain torch.

``head_path_cost_hip`` ``seeme_head_path_cost``: cost [W,K] (mm), how far a hypothesis' head (joint 15) strays from the shape of the
                       headset's own path over its window, the mean offset removed: a unary term of ``path_select``.
``head_anchor_hip``    ``seeme_head_anchor``: the smoothed shift [L,3] that puts the stitched motion's head onto the headset's path,
                       and what is left per frame (mm).  ``camera_centres`` / ``head_path_windows`` prepare the path on the host.
``head_rot_cost_hip``  ``seeme_head_rot_cost``: cost [W,K] (degrees), how far a hypothesis' head (the chain 0-3-6-9-12-15) turns against
                       the headset's orientation over its window, a constant mount rotation removed: a unary term as well, and the
                       angle per frame.  ``camera_rotations`` / ``head_rot_windows`` prepare the quaternions on the host;
                       ``head_joint_path`` / ``fit_device_offset`` are the lever arm between joint 15 and the device.
``scene_depth_hip``    ``seeme_scene_depth``: depth [W,K,T] (mm), how deep the capsules round a hypothesis' bones (``body_capsules``)
                       reach into the scene's points, its mean cost [W,K] (a unary term of ``path_select``) and the count of
                       penetrating frames hits [W,K]; ``scene_depth_torch`` is its twin.

``load_recording`` / ``windows_batch`` read a recording ``.npz`` and cut it into a batch with the data module's tuple
layout whose wearer slot is zero; a recording may carry its image condition as raw video frames, whose patches around the interactee
are then cut by ``crops.crop_patches_hip`` (``choose_frames``: which stored frame serves a window).  The definitions are stated once,
in include/seeme_hip.h.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import geometry as G

STITCH_ANGLE, STITCH_ANGLE_TRANSL, STITCH_ROT6D = 0, 1, 2
NLERP_DOT = 0.9995           # SEEME_STITCH_NLERP_DOT
SCENE_VIEW_TILE = 1024               # SEEME_SCENE_VIEW_TILE: vertices of one workgroup of seeme_scene_views
SCENE_VIEW_WINDOWS_PER_PASS = 16     # SEEME_SCENE_VIEW_WINDOWS_PER_PASS: views a workgroup walks over its tile
SCENE_VIEW_POINTS = 20000            # rows of an EgoBody scene table (TEST.SCENE_VIEW_POINTS)
HEAD_JOINT = 15                      # SEEME_HEAD_JOINT: the SMPL head, as EgoMetrics uses it
HEAD_ANCHOR_RMAX = 30                # SEEME_HEAD_ANCHOR_RMAX: ceil(3 x track.SIGMA_MAX)
SCENE_DEPTH_NBMAX = 32               # SEEME_SCENE_DEPTH_NBMAX: capsules of one table
SCENE_DEPTH_CHUNK = 32               # SEEME_SCENE_DEPTH_CHUNK: frames of one workgroup of seeme_scene_depth
CAPSULE_SKIP = (10, 11)              # the feet: standing on the floor is contact, the shin capsule ends at the ankle


# ----------------------------------------------------------------------------- window plan (host)
def window_plan(n_frames: int, T: int, overlap: int) -> Tuple[List[int], List[int]]:
    """(starts, lengths) of the windows of a recording: stride S = T - overlap, W = 1 for n_frames <= T, else
    ceil((n_frames - T) / S) + 1; starts[w] = w*S, lengths[w] = min(T, n_frames - w*S).  2*overlap <= T, so no frame lies in more
    than two windows; every window but the last is full, the last has at least overlap + 1 frames, and windows w, w+1 share exactly
    the last `overlap` frames of w and the first `overlap` of w+1."""
    for name, v in (("n_frames", n_frames), ("T", T), ("overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"window_plan: {name} must be an integer, got {v!r}")
    n_frames, T, O = int(n_frames), int(T), int(overlap)
    if n_frames < 1 or T < 1:
        raise ValueError(f"window_plan: n_frames and T must be >= 1, got {n_frames}, {T}")
    if O < 0 or 2 * O > T:
        raise ValueError(f"window_plan: the overlap must satisfy 0 <= overlap and 2*overlap <= T, got overlap {O}, T {T}")
    S = T - O
    W = 1 if n_frames <= T else -(-(n_frames - T) // S) + 1
    return [w * S for w in range(W)], [min(T, n_frames - w * S) for w in range(W)]


def stitch_layout(data_type: str, transl_in_feats: bool) -> int:
    """The layout argument of ``stitch_windows`` for what ``shapes.motion_layout`` decided."""
    if data_type == "rot6d":
        return STITCH_ROT6D
    return STITCH_ANGLE_TRANSL if transl_in_feats else STITCH_ANGLE


# ----------------------------------------------------------------------------- torch twins
def overlap_cost_torch(jts, overlap: int) -> torch.Tensor:
    """jts [W,K,T,24,3], any float dtype, any device, any K -> cost [W-1,K,K] (mm); zeros for overlap 0."""
    W, K, T = jts.shape[:3]
    O = int(overlap)
    if O < 0 or 2 * O > T:
        raise ValueError(f"overlap_cost: the overlap must satisfy 0 <= overlap and 2*overlap <= T, got overlap {O}, T {T}")
    cost = torch.zeros(max(W - 1, 0), K, K, device=jts.device, dtype=jts.dtype)
    if W < 2 or O == 0:
        return cost
    step = max(1, (1 << 24) // (K * K * O * 72))          # seams per pass: the pair tensor is [step,K,K,O,24,3]
    for lo in range(0, W - 1, step):
        hi = min(lo + step, W - 1)
        a = jts[lo:hi, :, T - O:]                                              # [s,K,O,24,3]
        b = jts[lo + 1:hi + 1, :, :O]
        cost[lo:hi] = (a[:, :, None] - b[:, None, :]).norm(dim=-1).sum(dim=(-1, -2)) / 24 / O * 1000.0
    return cost


def _argmin_low(x: torch.Tensor):
    """min over dim 0 and the LOWEST index that attains it; a NaN among the candidates: (NaN, 0), as the kernel."""
    n = x.shape[0]
    best = x.min(dim=0).values                                                 # (torch propagates NaN)
    ks = torch.arange(n, device=x.device).reshape(n, *([1] * (x.dim() - 1))).expand_as(x)
    idx = torch.where(x == best, ks, torch.full_like(ks, n)).min(dim=0).values
    return best, torch.where(idx < n, idx, torch.zeros_like(idx))


def path_select_torch(cost, unary=None) -> Dict[str, torch.Tensor]:
    """cost [W-1,K,K], unary [W,K] or None, any float dtype, any device, any K -> path [W] int64, seam_cost [W-1], path_cost [].
    d_0 = unary[0] (0 without unary); d_{w+1}[j] = min_i (d_w[i] + cost[w,i,j]) + unary[w+1,j], the lowest i on a tie, the lowest
    j of the smallest d_{W-1} at the end."""
    K = int(cost.shape[-1]) if unary is None else int(unary.shape[1])
    W = int(cost.shape[0]) + 1 if unary is None else int(unary.shape[0])
    if cost.shape[0] != W - 1 or (W > 1 and tuple(cost.shape[1:]) != (K, K)):
        raise ValueError(f"path_select: cost is {tuple(cost.shape)} for W = {W}, K = {K}: expected [W-1,K,K]")
    dev = cost.device
    d = unary[0].clone() if unary is not None else torch.zeros(K, device=dev, dtype=cost.dtype)
    back = torch.zeros(max(W - 1, 0), K, dtype=torch.int64, device=dev)
    for w in range(W - 1):
        d, back[w] = _argmin_low(d[:, None] + cost[w])
        if unary is not None:
            d = d + unary[w + 1]
    total, last = _argmin_low(d)
    path = torch.zeros(W, dtype=torch.int64, device=dev)
    path[W - 1] = last
    for w in range(W - 2, -1, -1):
        path[w] = back[w, path[w + 1]]
    seam = cost[torch.arange(W - 1, device=dev), path[:-1], path[1:]] if W > 1 else cost.new_zeros(0)
    return {"path": path, "seam_cost": seam, "path_cost": total}


def _normalize(q):
    return q / q.norm(dim=-1, keepdim=True)


def _aa_to_quat(a):
    th = a.norm(dim=-1, keepdim=True)
    safe = torch.where(th > 1e-6, th, torch.ones_like(th))
    k = torch.where(th > 1e-6, torch.sin(0.5 * th) / safe, 0.5 - th * th / 48.0)
    return torch.cat([torch.cos(0.5 * th), k * a], dim=-1)


def _rot6d_to_quat(x):
    """Model-side rot6d (``geometry.rot6d_to_rotmat`` 'prohmr': a1 = x[0:3], a2 = x[3:6], Gram-Schmidt) -> unit quaternion."""
    a1, a2 = x[..., :3], x[..., 3:6]
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u / u.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return G.rotmat_to_quat_torch(torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], dim=-1))     # columns b1, b2, b1 x b2


def _quat_to_rot6d(q):
    w, a, b, c = q.unbind(-1)
    return torch.stack([1.0 - 2.0 * (b * b + c * c), 2.0 * (a * b + w * c), 2.0 * (a * c - w * b),
                        2.0 * (a * b - w * c), 1.0 - 2.0 * (a * a + c * c), 2.0 * (b * c + w * a)], dim=-1)


def _blend(p, q, u):
    """p, q [...,4] unit quaternions, u [...,1]: q onto p's hemisphere, slerp (normalised lerp above NLERP_DOT), normalised."""
    dt = (p * q).sum(-1, keepdim=True)
    q = torch.where(dt < 0, -q, q)
    dt = dt.abs()
    near = dt > NLERP_DOT
    th = torch.acos(torch.where(near, torch.zeros_like(dt), dt))
    s = torch.sin(th)
    kp = torch.where(near, 1.0 - u, torch.sin((1.0 - u) * th) / s)
    kq = torch.where(near, u, torch.sin(u * th) / s)
    return _normalize(kp * p + kq * q)


def _check_stitch(W, T, O, n_frames, F, layout):
    starts, _ = window_plan(n_frames, T, O)
    if len(starts) != W:
        raise ValueError(f"stitch_windows: {W} windows, but the plan of n_frames {n_frames}, T {T}, overlap {O} has {len(starts)}")
    if layout == STITCH_ROT6D:
        ok = F == 144
    elif layout in (STITCH_ANGLE, STITCH_ANGLE_TRANSL):
        ok = F >= 3 and F % 3 == 0 and (layout == STITCH_ANGLE or F >= 6)
    else:
        raise ValueError(f"stitch_windows: unknown layout {layout!r}")
    if not ok:
        raise ValueError(f"stitch_windows: features are {F} wide: expected J x 3 (+ 3 translation values) or 24 x 6 for rot6d")


def stitch_windows_torch(feats, overlap: int, n_frames: int, layout: int) -> torch.Tensor:
    """feats [W,T,F] renormed features of the chosen hypotheses, any float dtype, any device -> [n_frames,F]."""
    W, T, F = feats.shape
    O = int(overlap)
    _check_stitch(W, T, O, n_frames, F, layout)
    dev = feats.device
    S = T - O
    n = torch.arange(n_frames, device=dev)
    w = (n // S).clamp(max=W - 1)
    t = n - w * S
    out = feats[w, t].clone()
    ov = ((w >= 1) & (t < O)).nonzero()[:, 0]
    if ov.numel() == 0:
        return out
    wo, to = w[ov], t[ov]
    a, b = feats[wo - 1, to + S], feats[wo, to]                                # earlier, later: [n_ov,F]
    u = ((to + 1).to(feats.dtype) / (O + 1))[:, None, None]
    if layout == STITCH_ROT6D:
        y = _quat_to_rot6d(_blend(_rot6d_to_quat(a.reshape(-1, 24, 6)), _rot6d_to_quat(b.reshape(-1, 24, 6)), u)).reshape(-1, F)
    else:
        nr = F - 3 if layout == STITCH_ANGLE_TRANSL else F
        y = G.quat_to_aa_torch(_blend(_aa_to_quat(a[:, :nr].reshape(len(ov), -1, 3)), _aa_to_quat(b[:, :nr].reshape(len(ov), -1, 3)), u))
        y = y.reshape(len(ov), nr)
        if layout == STITCH_ANGLE_TRANSL:
            y = torch.cat([y, a[:, nr:] + u[:, 0] * (b[:, nr:] - a[:, nr:])], dim=1)
    out[ov] = y
    return out


# ----------------------------------------------------------------------------- the headset's own path: host side and twins
def camera_centres(world2cam) -> np.ndarray:
    """world2cam [L,4,4], the rigid maps p -> A_n p + a_n -> float64 [L,3]: c[n] = -A_n^T a_n, the device's position in the world frame.
    Only the centre is used, so no convention about the camera's axes enters."""
    M = np.asarray(world2cam, np.float64)
    if M.ndim != 3 or M.shape[1:] != (4, 4):
        raise ValueError(f"camera_centres: world2cam is {M.shape}: expected [L,4,4]")
    return -np.einsum("nji,nj->ni", M[:, :3, :3], M[:, :3, 3])


def check_head_path(path, n_frames: int, what: str = "head_path") -> np.ndarray:
    """head_path -> float64 [L,3]: floats, finite, one row per recording frame, or a ValueError that names the key."""
    a = path.detach().cpu().numpy() if isinstance(path, torch.Tensor) else np.asarray(path)
    if a.dtype.kind != "f" or a.shape != (n_frames, 3):
        raise ValueError(f"{what}: head_path is {a.shape} {a.dtype}: expected floats [{n_frames},3] (L = {n_frames}), the device's "
                         "position in the recording's world frame")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: head_path of frame {int(np.argmax(~np.isfinite(a).all(axis=1)))} is not finite")
    return np.ascontiguousarray(a, np.float64)


def head_path_windows(path, starts, lengths, T: int) -> torch.Tensor:
    """path [L,3] (tensor or array) -> [W,T,3] in its dtype (on its device): row w holds path[starts[w] : starts[w] + lengths[w]], then
    zeros: the path operand of ``head_path_cost`` for the windows of ``window_plan``."""
    p = path if isinstance(path, torch.Tensor) else torch.from_numpy(np.asarray(path))
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"head_path_windows: the path is {tuple(p.shape)}: expected [L,3]")
    T = int(T)
    out = torch.zeros(len(starts), T, 3, dtype=p.dtype, device=p.device)
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        lo, ln = int(lo), int(ln)
        if lo < 0 or ln < 0 or ln > T or lo + ln > p.shape[0]:
            raise ValueError(f"head_path_windows: window {w} (frames {lo}..{lo + ln - 1}) does not fit T = {T} and a path of {p.shape[0]} frames")
        out[w, :ln] = p[lo:lo + ln]
    return out


def _check_head_cost(jts, path, lengths):
    if not isinstance(jts, torch.Tensor) or not isinstance(path, torch.Tensor) or not jts.dtype.is_floating_point or path.dtype != jts.dtype:
        raise ValueError(f"head_path_cost: joints and path must be float tensors of one dtype, got {getattr(jts, 'dtype', type(jts))} and "
                         f"{getattr(path, 'dtype', type(path))}")
    if jts.dim() != 5 or tuple(jts.shape[3:]) != (24, 3) or tuple(path.shape) != (jts.shape[0], jts.shape[2], 3):
        raise ValueError(f"head_path_cost: joints are {tuple(jts.shape)}, the path is {tuple(path.shape)}: expected [W,K,T,24,3] and [W,T,3]")
    n = lengths.detach().cpu().reshape(-1).tolist() if isinstance(lengths, torch.Tensor) else [v for v in lengths]
    if len(n) != jts.shape[0] or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in n):
        raise ValueError(f"head_path_cost: lengths are {n!r}: expected {jts.shape[0]} integers, one per window")
    return [int(v) for v in n]


def head_path_cost_torch(jts, path, lengths) -> torch.Tensor:
    """jts [W,K,T,24,3], path [W,T,3], lengths [W] (integers), any float dtype, any device, any K -> cost [W,K] (mm): the definition of
    ``seeme_head_path_cost``.  Frames past a window's length take no part (a NaN there is not seen)."""
    n = _check_head_cost(jts, path, lengths)
    W, K, T = (int(v) for v in jts.shape[:3])
    nn = torch.tensor(n, device=jts.device).clamp(0, T)
    keep = (torch.arange(T, device=jts.device)[None] < nn[:, None])[:, None, :, None]                 # [W,1,T,1]
    div = nn.clamp(min=1).to(jts.dtype)[:, None]
    r = torch.where(keep, jts[:, :, :, HEAD_JOINT] - path[:, None], torch.zeros((), dtype=jts.dtype, device=jts.device))
    o = r.sum(dim=2) / div[..., None]                                                                  # [W,K,3]
    dev = torch.where(keep[..., 0], (r - o[:, :, None]).norm(dim=-1), torch.zeros((), dtype=jts.dtype, device=jts.device))
    cost = 1000.0 * (dev.sum(dim=2) / div)
    return torch.where((nn > 1)[:, None], cost, torch.zeros_like(cost))


def _host_taps(taps, what: str) -> np.ndarray:
    t = np.asarray(taps.detach().cpu().numpy() if isinstance(taps, torch.Tensor) else taps)
    if t.ndim != 1 or t.shape[0] < 1 or t.dtype.kind not in "fiu":
        raise ValueError(f"{what}: taps are {t.shape} {t.dtype}: expected numbers [R+1]")
    return t


def _check_head_anchor(joints, path):
    if not isinstance(joints, torch.Tensor) or not isinstance(path, torch.Tensor) or not joints.dtype.is_floating_point \
            or path.dtype != joints.dtype:
        raise ValueError(f"head_anchor: joints and path must be float tensors of one dtype, got {getattr(joints, 'dtype', type(joints))} "
                         f"and {getattr(path, 'dtype', type(path))}")
    if joints.dim() != 3 or tuple(joints.shape[1:]) != (24, 3) or joints.shape[0] < 1 or tuple(path.shape) != (joints.shape[0], 3):
        raise ValueError(f"head_anchor: joints are {tuple(joints.shape)}, the path is {tuple(path.shape)}: expected [L,24,3] and [L,3], "
                         "L >= 1")


def head_anchor_torch(joints, path, taps) -> Tuple[torch.Tensor, torch.Tensor]:
    """joints [L,24,3], path [L,3], any float dtype, any device; taps [R+1] (``track.gaussian_taps``), any R -> (shift [L,3], residual
    [L] in mm): the definition of ``seeme_head_anchor``."""
    _check_head_anchor(joints, path)
    tp = _host_taps(taps, "head_anchor").astype(np.float64)
    if not np.isfinite(tp).all() or (tp < 0).any() or not tp[0] > 0:
        raise ValueError(f"head_anchor: every tap must be finite and >= 0 and taps[0] > 0, got {tp.tolist()}")
    Rr, n_fr = tp.shape[0] - 1, int(joints.shape[0])
    tp = torch.from_numpy(tp).to(device=joints.device, dtype=joints.dtype)
    r = path - joints[:, HEAD_JOINT]
    n = torch.arange(n_fr, device=joints.device)
    acc, wsum = torch.zeros_like(r), torch.zeros(n_fr, device=joints.device, dtype=joints.dtype)
    for d in range(-Rr, Rr + 1):                                                 # increasing frame order
        m = n + d
        k = tp[abs(d)] * ((m >= 0) & (m < n_fr)).to(joints.dtype)
        acc = acc + k[:, None] * r[m.clamp(0, n_fr - 1)]
        wsum = wsum + k
    shift = acc / wsum[:, None]
    return shift, 1000.0 * (r - shift).norm(dim=-1)


# ----------------------------------------------------------------------------- the headset's orientation: host side and the twin
def camera_rotations(world2cam) -> np.ndarray:
    """world2cam [L,4,4], the rigid maps p -> A_n p + a_n -> float64 [L,3,3]: A_n^T, the rotation camera -> world of every frame, the
    device's orientation in the world frame.  Which way the camera's axes point does not matter to ``head_rot_cost``: a constant
    rotation on the device's side costs nothing."""
    M = np.asarray(world2cam, np.float64)
    if M.ndim != 3 or M.shape[1:] != (4, 4):
        raise ValueError(f"camera_rotations: world2cam is {M.shape}: expected [L,4,4]")
    return np.ascontiguousarray(M[:, :3, :3].transpose(0, 2, 1))


def check_head_rot(rot, n_frames: int, what: str = "head_rot") -> np.ndarray:
    """head_rot -> float64 [L,3,3], the rotations device -> world: floats, finite, orthonormal to 1e-3 with a positive determinant (as
    ``check_world2cam`` asks of its 3x3 block), one per recording frame, or a ValueError that names the key and the frame."""
    a = rot.detach().cpu().numpy() if isinstance(rot, torch.Tensor) else np.asarray(rot)
    if a.dtype.kind != "f" or a.shape != (n_frames, 3, 3):
        raise ValueError(f"{what}: head_rot is {a.shape} {a.dtype}: expected floats [{n_frames},3,3] (L = {n_frames}), the rotation "
                         "device -> world of every frame")
    a = np.ascontiguousarray(a, np.float64)
    bad = ~np.isfinite(a).all(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        bad |= ~(np.abs(a.transpose(0, 2, 1) @ a - np.eye(3)).max(axis=(1, 2)) <= 1e-3) | ~(np.linalg.det(np.nan_to_num(a)) > 0)
    if bad.any():
        f = int(np.argmax(bad))
        raise ValueError(f"{what}: head_rot of frame {f} is not a rotation (finite, orthonormal to 1e-3, a positive determinant):\n{a[f]}")
    return a


def _rot3(rot, name: str) -> np.ndarray:
    a = np.asarray(rot.detach().cpu().numpy() if isinstance(rot, torch.Tensor) else rot, np.float64)
    if a.ndim != 3 or a.shape[1:] != (3, 3):
        raise ValueError(f"{name}: the rotations are {a.shape}: expected [L,3,3]")
    return a


def head_rot_windows(rot, starts, lengths, T: int, window_frames=None) -> torch.Tensor:
    """rot [L,3,3] (device -> world) -> float32 [W,T,4] on the host: row w holds the unit quaternions (w,x,y,z) of
    rot[starts[w] : starts[w] + lengths[w]], then identities: the dev_quat operand of ``head_rot_cost`` for the windows of
    ``window_plan``.  window_frames [W,4,4] (M_w, world -> window w's frame): the rotations are moved into every window's own frame
    first, A_w C_n with A_w the rotation block of M_w -- the frame ``predict``'s m_rst_all is in.  Computed in float64."""
    C = _rot3(rot, "head_rot_windows")
    T = int(T)
    A = None
    if window_frames is not None:
        A = np.asarray(window_frames.detach().cpu().numpy() if isinstance(window_frames, torch.Tensor) else window_frames, np.float64)
        if A.shape != (len(starts), 4, 4):
            raise ValueError(f"head_rot_windows: window_frames are {A.shape}: expected [W,4,4] = [{len(starts)},4,4]")
    out = torch.zeros(len(starts), T, 4, dtype=torch.float64)
    out[..., 0] = 1.0
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        lo, ln = int(lo), int(ln)
        if lo < 0 or ln < 0 or ln > T or lo + ln > C.shape[0]:
            raise ValueError(f"head_rot_windows: window {w} (frames {lo}..{lo + ln - 1}) does not fit T = {T} and {C.shape[0]} rotations")
        if ln:
            Cw = C[lo:lo + ln] if A is None else A[w, :3, :3][None] @ C[lo:lo + ln]
            out[w, :ln] = G.rotmat_to_quat_torch(torch.from_numpy(np.ascontiguousarray(Cw)))
    return out.float()


def check_head_offset(offset, what: str = "head_offset") -> np.ndarray:
    """The vector from joint 15 to the device in the device's frame, metres -> float64 [3]: three finite numbers, or a ValueError that
    names `what`."""
    vals = offset.detach().cpu().reshape(-1).tolist() if isinstance(offset, torch.Tensor) else offset
    try:
        vals = list(vals)
    except TypeError:
        vals = None
    if vals is None or len(vals) != 3 or any(isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating))
                                             or not np.isfinite(v) for v in vals):
        raise ValueError(f"{what} must be three finite numbers (x, y, z in metres, in the device's frame), got {offset!r}")
    return np.array([float(v) for v in vals], np.float64)


def head_joint_path(path, rot, offset) -> np.ndarray:
    """The lever arm: path [L,3] (the device's positions), rot [L,3,3] (device -> the frame the path is in), offset [3] (the vector
    from joint 15 to the device, metres, in the device's frame) -> float64 [L,3], path[n] - C_n offset: the path of joint 15 itself,
    which both head terms take in place of the device's."""
    C = _rot3(rot, "head_joint_path")
    p = np.asarray(path.detach().cpu().numpy() if isinstance(path, torch.Tensor) else path, np.float64)
    o = np.asarray(offset.detach().cpu().numpy() if isinstance(offset, torch.Tensor) else offset, np.float64)
    if p.shape != (C.shape[0], 3) or o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"head_joint_path: the path is {p.shape}, the offset {o.shape}: expected [{C.shape[0]},3] and 3 finite numbers")
    return p - np.einsum("nij,j->ni", C, o)


def fit_device_offset(head, path, rot) -> Tuple[np.ndarray, float]:
    """head [L,3] (joint 15 of a KNOWN wearer), path [L,3] (the device), rot [L,3,3] (device -> their frame) -> (offset [3] float64 in
    the device's frame, rms_mm): the least-squares offset mean_n C_n^T (path_n - head_n) and the RMS of what it leaves, mm."""
    C = _rot3(rot, "fit_device_offset")
    h, p = (np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float64) for a in (head, path))
    if h.shape != (C.shape[0], 3) or p.shape != h.shape or C.shape[0] < 1:
        raise ValueError(f"fit_device_offset: head is {h.shape}, the path {p.shape}, the rotations {C.shape}: expected [L,3], [L,3] and "
                         "[L,3,3], L >= 1")
    offset = np.einsum("nji,nj->ni", C, p - h).mean(axis=0)
    left = p - h - np.einsum("nij,j->ni", C, offset)
    return offset, 1000.0 * float(np.sqrt((left * left).sum(axis=1).mean()))


def _quat_mul(p, q):
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                        pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], dim=-1)


def _quat_conj(q):
    return torch.cat([q[..., :1], -q[..., 1:]], dim=-1)


def _check_head_rot_cost(feats, layout, dev_quat, lengths):
    if not isinstance(feats, torch.Tensor) or not isinstance(dev_quat, torch.Tensor) or not feats.dtype.is_floating_point \
            or dev_quat.dtype != feats.dtype:
        raise ValueError(f"head_rot_cost: features and dev_quat must be float tensors of one dtype, got {getattr(feats, 'dtype', type(feats))} "
                         f"and {getattr(dev_quat, 'dtype', type(dev_quat))}")
    if feats.dim() != 4 or tuple(dev_quat.shape) != (feats.shape[0], feats.shape[2], 4):
        raise ValueError(f"head_rot_cost: features are {tuple(feats.shape)}, dev_quat is {tuple(dev_quat.shape)}: expected [W,K,T,F] and "
                         "[W,T,4]")
    F = int(feats.shape[3])
    if isinstance(layout, bool) or not isinstance(layout, (int, np.integer)) or layout not in (STITCH_ANGLE, STITCH_ANGLE_TRANSL, STITCH_ROT6D) \
            or not (F == 144 if layout == STITCH_ROT6D else F % 3 == 0 and F // 3 - (layout == STITCH_ANGLE_TRANSL) >= HEAD_JOINT + 1):
        raise ValueError(f"head_rot_cost: layout {layout!r} with features {F} wide: expected STITCH_ANGLE with J x 3, STITCH_ANGLE_TRANSL "
                         "with J x 3 + 3 (J >= 16) or STITCH_ROT6D with 144")
    n = lengths.detach().cpu().reshape(-1).tolist() if isinstance(lengths, torch.Tensor) else [v for v in lengths]
    if len(n) != feats.shape[0] or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in n):
        raise ValueError(f"head_rot_cost: lengths are {n!r}: expected {feats.shape[0]} integers, one per window")
    return [int(v) for v in n]


def head_rot_cost_torch(feats, layout: int, dev_quat, lengths) -> Dict[str, torch.Tensor]:
    """feats [W,K,T,F] renormed features, dev_quat [W,T,4], lengths [W] (integers), any float dtype, any device, any K ->
    {"cost" [W,K], "angle" [W,K,T]} (degrees): the definition of ``seeme_head_rot_cost``.  Frames past a window's length, joints off
    the chain 0-3-6-9-12-15 and the translation columns take no part (a NaN there is not seen)."""
    n = _check_head_rot_cost(feats, layout, dev_quat, lengths)
    W, K, T = (int(v) for v in feats.shape[:3])
    dev, dt = feats.device, feats.dtype
    nn = torch.tensor(n, device=dev).clamp(0, T)
    keep = (torch.arange(T, device=dev)[None] < nn[:, None])[:, None, :]                               # [W,1,T]
    uw = 6 if layout == STITCH_ROT6D else 3
    unit = torch.tensor([1.0, 0, 0, 0, 1.0, 0] if uw == 6 else [0.0, 0, 0], device=dev, dtype=dt)      # the identity, where not kept
    to_quat = _rot6d_to_quat if uw == 6 else _aa_to_quat
    h = None
    for j in range(0, HEAD_JOINT + 1, 3):                                                              # the chain 0, 3, 6, 9, 12, 15
        q = to_quat(torch.where(keep[..., None], feats[..., uw * j:uw * j + uw], unit))
        h = q if h is None else _quat_mul(h, q)
    one = torch.tensor([1.0, 0, 0, 0], device=dev, dtype=dt)
    d = _quat_mul(_quat_conj(h), torch.where(keep[..., None], dev_quat[:, None], one))                 # [W,K,T,4]
    s = torch.where((d * d[:, :, :1]).sum(-1, keepdim=True) < 0, -1.0, 1.0).to(dt) * keep[..., None].to(dt)
    m = (s * d).sum(dim=2)
    live = (nn > 1)[:, None]                                                                           # [W,1]
    m = _normalize(torch.where(live[..., None], m, one))
    r = _quat_mul(_quat_conj(m)[:, :, None], d)
    a = 2.0 * torch.atan2(r[..., 1:].norm(dim=-1), r[..., 0].abs()) * (180.0 / np.pi)
    a = torch.where(keep & live[..., None], a, torch.zeros((), device=dev, dtype=dt))
    return {"cost": a.sum(dim=2) / nn.clamp(min=1).to(dt)[:, None], "angle": a}


# ----------------------------------------------------------------------------- the body against the scene: capsules and the twin
def _segment_distance(p: np.ndarray, a: np.ndarray, c: np.ndarray) -> np.ndarray:
    """Distance of the points p [V,3] from the segments a[b] .. c[b] ([NB,3] each) -> [V,NB], float64 on the host.  Where the closest
    point is an end, the distance is taken from that joint itself: two bones that share the joint then tie exactly."""
    e, q = c - a, p[:, None] - a[None]
    ee = (e * e).sum(-1)
    s = (np.clip((q * e[None]).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0) * (ee > 0))[..., None]
    x = np.where(s <= 0, a[None], np.where(s >= 1, c[None], a[None] + s * e[None]))
    return np.linalg.norm(p[:, None] - x, axis=-1)


def body_capsules(smpl_model, betas=None, quantile: float = 0.5, segs=None) -> Tuple[np.ndarray, np.ndarray]:
    """The capsule table of ``scene_depth``: (segs [NB,2] int32, radius [NB] float32), built on the host in float64.  segs defaults to
    (parent[j], j) for j = 1..23 without the feet j = 10, 11: 21 bones.  The template is posed at rest with betas [10] (zeros if
    None), every vertex goes to its nearest segment (the lowest b on a tie), and radius[b] is the `quantile` of the distances of b's
    vertices, the lower one (a sample, never an interpolation); 0 for a segment without vertices, which never penetrates.  The
    median keeps the capsule inside the body: the term under-reports rather than penalising contact."""
    if isinstance(quantile, bool) or not isinstance(quantile, (int, float)) or not 0 <= quantile <= 1:
        raise ValueError(f"body_capsules: quantile must be a number in 0..1, got {quantile!r}")
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)        # noqa: E731
    v = f64(smpl_model.v_template)
    if betas is not None:
        b = np.asarray(betas.detach().cpu().numpy() if isinstance(betas, torch.Tensor) else betas, np.float64).reshape(-1)
        if b.shape != (10,) or not np.isfinite(b).all():
            raise ValueError(f"body_capsules: betas are {b.shape}: expected 10 finite numbers")
        v = v + f64(smpl_model.shapedirs)[:, :, :10] @ b
    jt = f64(smpl_model.J_regressor) @ v                               # [J,3]: at rest the joints are the regressed ones
    if segs is None:
        par = smpl_model.parents.detach().cpu().numpy()
        segs = [(int(par[j]), j) for j in range(1, 24) if j not in CAPSULE_SKIP]
    sg = np.asarray(segs)
    if sg.ndim != 2 or sg.shape[1] != 2 or sg.shape[0] < 1 or sg.dtype.kind not in "iu" or sg.min() < 0 or sg.max() >= jt.shape[0]:
        raise ValueError(f"body_capsules: segs must be joint indices [NB,2] in 0..{jt.shape[0] - 1}, got {sg.tolist()!r}")
    d = _segment_distance(v, jt[sg[:, 0]], jt[sg[:, 1]])               # [V,NB]
    own = d.argmin(axis=1)                                             # (the first of equal minima: the lowest b)
    radius = np.zeros(sg.shape[0], np.float64)
    for b in range(sg.shape[0]):
        mine = np.sort(d[own == b, b])
        if mine.size:
            radius[b] = mine[int(np.floor(quantile * (mine.size - 1)))]
    return sg.astype(np.int32), radius.astype(np.float32)


def _check_scene_depth(jts, lengths, points, segs, radius):
    """Shapes and dtypes of the operands of ``scene_depth``; -> (lengths as a list, or the int32 device tensor itself; segs [NB,2]
    int32; radius [NB] float64), the two tables on the host."""
    if not isinstance(jts, torch.Tensor) or not isinstance(points, torch.Tensor) or not jts.dtype.is_floating_point \
            or points.dtype != jts.dtype:
        raise ValueError(f"scene_depth: joints and points must be float tensors of one dtype, got {getattr(jts, 'dtype', type(jts))} "
                         f"and {getattr(points, 'dtype', type(points))}")
    if jts.dim() != 5 or jts.shape[4] != 3 or min(jts.shape) < 1 or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"scene_depth: joints are {tuple(jts.shape)}, the points {tuple(points.shape)}: expected [W,K,T,J,3] and [N,3], "
                         "nothing empty")
    if points.device != jts.device:
        raise ValueError(f"scene_depth: joints are on {jts.device}, the points on {points.device}")
    sg = np.asarray(segs.detach().cpu().numpy() if isinstance(segs, torch.Tensor) else segs)
    rd = np.asarray(radius.detach().cpu().numpy() if isinstance(radius, torch.Tensor) else radius)
    if sg.ndim != 2 or sg.shape[1] != 2 or sg.shape[0] < 1 or sg.dtype.kind not in "iu" or rd.shape != (sg.shape[0],) \
            or rd.dtype.kind not in "fiu":
        raise ValueError(f"scene_depth: segs are {sg.shape} {sg.dtype}, radius is {rd.shape} {rd.dtype}: expected integers [NB,2] and "
                         "numbers [NB], NB >= 1")
    W = int(jts.shape[0])
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda and lengths.dtype == torch.int32 and tuple(lengths.shape) == (W,):
        return lengths, sg.astype(np.int32), rd.astype(np.float64)     # on the device already: nothing is copied back
    n = lengths.detach().cpu().reshape(-1).tolist() if isinstance(lengths, torch.Tensor) else [v for v in lengths]
    if len(n) != W or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in n):
        raise ValueError(f"scene_depth: lengths are {n!r}: expected {W} integers, one per window")
    return [int(v) for v in n], sg.astype(np.int32), rd.astype(np.float64)


def scene_depth_torch(jts, lengths, points, segs, radius, max_elems: int = 1 << 24) -> Dict[str, torch.Tensor]:
    """jts [W,K,T,J,3], points [N,3] (any float dtype, any device), lengths [W] integers, segs [NB,2] joint indices and radius [NB]
    (finite, >= 0; any NB) -> {"depth" [W,K,T] (mm), "cost" [W,K] (mm), "hits" [W,K] int32}: the definition of ``seeme_scene_depth``.
    The points go through in chunks, so that no intermediate holds more than about `max_elems` (frame, segment, point) triples.
    Frames past a window's length, joints that no segment names and pairs whose value is a NaN take no part."""
    n, sg, rd = _check_scene_depth(jts, lengths, points, segs, radius)
    W, K, T, J = (int(v) for v in jts.shape[:4])
    if sg.min() < 0 or sg.max() >= J:
        raise ValueError(f"scene_depth: every segment index must be in 0..J-1 = 0..{J - 1}, got {sg.tolist()}")
    if not np.isfinite(rd).all() or (rd < 0).any():
        raise ValueError(f"scene_depth: every radius must be finite and >= 0, got {rd.tolist()}")
    dev, dt = jts.device, jts.dtype
    nn = (n.to(torch.int64) if isinstance(n, torch.Tensor) else torch.tensor(n, device=dev)).clamp(0, T)
    keep = (torch.arange(T, device=dev)[None] < nn[:, None])[:, None]                                # [W,1,T]
    sgt = torch.from_numpy(sg.astype(np.int64)).to(dev)
    r = torch.from_numpy(rd).to(device=dev, dtype=dt)
    a = jts[:, :, :, sgt[:, 0]][..., None, :]                                                        # [W,K,T,NB,1,3]
    e = jts[:, :, :, sgt[:, 1]][..., None, :] - a
    ee = (e * e).sum(-1)                                                                             # [W,K,T,NB,1]
    pos = ee > 0
    one, zero, ninf = torch.ones((), dtype=dt, device=dev), torch.zeros((), dtype=dt, device=dev), \
        torch.full((), float("-inf"), dtype=dt, device=dev)
    best = torch.full((W, K, T), float("-inf"), dtype=dt, device=dev)
    step = max(1, int(max_elems) // (W * K * T * sg.shape[0]))
    for lo in range(0, int(points.shape[0]), step):
        q = points[lo:lo + step] - a                                                                 # [W,K,T,NB,P,3]
        s = torch.where(pos, ((q * e).sum(-1) / torch.where(pos, ee, one)).clamp(0, 1), zero)
        val = r[:, None] - (q - s[..., None] * e).norm(dim=-1)                                       # [W,K,T,NB,P]
        best = torch.maximum(best, torch.where(val != val, ninf, val).amax(dim=(-1, -2)))
    depth = torch.where(keep, 1000.0 * best.clamp(min=0), zero)
    cost = torch.where((nn > 0)[:, None], depth.sum(dim=2) / nn.clamp(min=1).to(dt)[:, None], zero)
    return {"depth": depth, "cost": cost, "hits": (depth > 0).sum(dim=2).to(torch.int32)}


# ----------------------------------------------------------------------------- scene views: the twin
def _view_coord(M, c: int, x, y, z):
    """Coordinate c of the moved vertices, in the order of the kernel's fmaf chain (torch has no fused multiply-add: two roundings
    per step where the kernel has one).  M [w,4,4]; x, y, z [N] or [w,P] -> [w,N] or [w,P]."""
    return M[:, c, 2, None] * z + (M[:, c, 1, None] * y + (M[:, c, 0, None] * x + M[:, c, 3, None]))


def scene_views_torch(verts, world2view, P: int) -> Dict[str, torch.Tensor]:
    """verts [N,3], world2view [W,4,4] (rows 0..2 are read), any float dtype, any device -> cloud [W,P,3] in the view's frame, index
    [W,P] int32 (the source vertex of every row), count [W] int32: the definition of ``seeme_scene_views`` (include/seeme_hip.h).  No
    host synchronisation: the row of rank r is found by a search in the running survivor count.  In fp32 its ``z > 0`` may differ
    from the kernel's for vertices within rounding of the view's plane (the kernel fuses every multiply-add); in float64 on inputs
    that keep a margin from the plane it is the kernel's reference."""
    if verts.dim() != 2 or verts.shape[1] != 3 or world2view.dim() != 3 or tuple(world2view.shape[1:]) != (4, 4):
        raise ValueError(f"scene_views: verts are {tuple(verts.shape)}, world2view is {tuple(world2view.shape)}: expected [N,3] and [W,4,4]")
    N, W, P = int(verts.shape[0]), int(world2view.shape[0]), int(P)
    if N < 1 or W < 1 or P < 1:
        raise ValueError(f"scene_views: N, W and P must be >= 1, got {N}, {W}, {P}")
    dev = verts.device
    M = world2view.to(verts.dtype)
    x, y, z = verts.unbind(-1)
    j = torch.arange(P, device=dev)
    cloud = torch.zeros(W, P, 3, device=dev, dtype=verts.dtype)
    index = torch.full((W, P), -1, device=dev, dtype=torch.int32)
    count = torch.zeros(W, device=dev, dtype=torch.int32)
    step = max(1, (1 << 24) // N)                                              # views per pass: the temporaries are [step,N]
    for lo in range(0, W, step):
        Mc = M[lo:lo + step]
        running = (_view_coord(Mc, 2, x, y, z) > 0).cumsum(dim=1)              # [w,N] survivors up to and including vertex i
        n = running[:, -1]
        k = torch.div(n, P, rounding_mode="floor").clamp(min=1)
        rank = torch.where((n >= P)[:, None], j[None] * k[:, None], j[None] % n.clamp(min=1)[:, None])
        at = torch.searchsorted(running, rank + 1).clamp(max=N - 1)            # the first vertex whose running count reaches rank + 1
        px, py, pz = verts[at].unbind(-1)                                      # [w,P]
        rows = torch.stack([_view_coord(Mc, c, px, py, pz) for c in range(3)], dim=-1)
        some = (n > 0)[:, None]
        cloud[lo:lo + step] = torch.where(some[..., None], rows, torch.zeros_like(rows))
        index[lo:lo + step] = torch.where(some, at, torch.full_like(at, -1)).to(torch.int32)
        count[lo:lo + step] = n.to(torch.int32)
    return {"cloud": cloud, "index": index, "count": count}


# ----------------------------------------------------------------------------- rigid re-framing of SMPL parameters and joints
def _apply(A, v):
    """A [...,3,3] on v [...,3] (leading dimensions broadcast)."""
    return (A @ v[..., None])[..., 0]


def _quat_mul(p, q):
    pw, px, py, pz = p.unbind(-1)
    qw, qx, qy, qz = q.unbind(-1)
    return torch.stack([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                        pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], dim=-1)


def rigid_parts(M):
    """[...,4,4] -> (A [...,3,3], a [...,3]) of p -> A p + a."""
    return M[..., :3, :3], M[..., :3, 3]


def rigid_inverse(M):
    """[...,4,4] rigid maps -> their inverses (A^T, -A^T a)."""
    A, a = rigid_parts(M)
    At = A.transpose(-1, -2)
    out = torch.zeros_like(M)
    out[..., :3, :3], out[..., :3, 3], out[..., 3, 3] = At, -_apply(At, a), 1.0
    return out


def rest_pelvis(smpl_model, betas):
    """J0 [n,3]: joint 0 of the SMPL layer at zero pose and zero translation for betas [n,10] (in their dtype, on their device).  The
    regressor is folded into the template and the shape directions in the model's own dtype, as the SMPL kernels and their twins
    fold it, so J0 is the pelvis they rotate about."""
    b = betas.reshape(-1, 10)
    J_t = (smpl_model.J_regressor @ smpl_model.v_template)[0].to(b)                                   # [3]
    J_s = torch.einsum("jv,vkl->jkl", smpl_model.J_regressor, smpl_model.shapedirs)[0].to(b)          # [3,10]
    return J_t[None] + b @ J_s.T


def reframe_smpl(global_orient, transl, J0, A, a):
    """SMPL parameters of the same body seen through p -> A p + a: go' = log(A exp(go)), t' = A (J0 + t) + a - J0 (SMPL rotates about
    the rest pelvis J0: joints = R_g (X - J0) + J0 + t).  global_orient, transl [...,3]; J0, a [...,3] and A [...,3,3] broadcast
    over the leading dimensions.  Plain torch, any float dtype, any device; go' has an angle in [0, pi]."""
    q = _quat_mul(G.rotmat_to_quat_torch(A.to(global_orient)), _aa_to_quat(global_orient))
    J0, a = J0.to(transl), a.to(transl)
    return G.quat_to_aa_torch(_normalize(q)), _apply(A.to(transl), J0 + transl) + a - J0


def reframe_rot6d(x6, A):
    """The 6-D variant for model-side rot6d features (``geometry.rot6d_to_rotmat`` 'prohmr': x[0:3], x[3:6] -> columns b1, b2):
    x6 [...,6] -> the first two columns of A R.  fp32 on the device goes through the kernel, anything else through its torch twin."""
    if x6.is_cuda and x6.dtype == torch.float32:
        R = G.rot6d_to_rotmat(x6.reshape(-1, 6).contiguous())
    else:
        from .vae_autograd import rot6d_to_rotmat_torch
        R = rot6d_to_rotmat_torch(x6.reshape(-1, 6))
    R = A.to(x6) @ R.reshape(*x6.shape[:-1], 3, 3)
    return torch.cat([R[..., :, 0], R[..., :, 1]], dim=-1)


def reframe_joints(joints, J0, A, a, has_transl: bool):
    """joints [...,J,3] of a body through p -> A p + a: A j + a when the parameters carry a translation; A (j - J0) + J0 when they
    do not (``predict_transl`` false, and rot6d, which is posed with zero betas and no translation): only the orientation can be
    re-framed then, and this is what the SMPL joints of the re-framed parameters are.  J0, a [...,3], A [...,3,3] broadcast over the
    leading dimensions of joints (the joint axis excluded)."""
    A = A.to(joints)[..., None, :, :]
    if has_transl:
        return _apply(A, joints) + a.to(joints)[..., None, :]
    J0 = J0.to(joints)[..., None, :]
    return _apply(A, joints - J0) + J0


# ----------------------------------------------------------------------------- kernels
_WS = L.Workspace(per_stream=True)    # shared by the launches below: launches of one stream run in order


def overlap_cost_hip(jts, overlap: int) -> torch.Tensor:
    """jts [W,K,T,24,3] fp32 on the device, K <= 32 (``overlap_cost_torch`` serves K > 32) -> cost [W-1,K,K] (mm)."""
    L.require_cuda(jts, "jts")
    if jts.dim() != 5 or tuple(jts.shape[3:]) != (24, 3):
        raise L.SeemeError(f"overlap_cost: joints are {tuple(jts.shape)}: expected [W,K,T,24,3]")
    W, K, T = (int(n) for n in jts.shape[:3])
    return _launch_overlap(jts.contiguous(), W, K, T, int(overlap))


def _launch_overlap(jts, W, K, T, O, ws_bytes=None) -> torch.Tensor:
    lib = L.lib()
    need = int(lib.seeme_overlap_cost_workspace_bytes(W, K, T, O))
    ws = _WS.get(need, jts.device)
    # (the kernel writes nothing for O = 0: the cost of sharing no frame is 0)
    cost = (torch.zeros if O == 0 else torch.empty)(max(W - 1, 0), max(K, 0), max(K, 0), device=jts.device, dtype=torch.float32)
    L.call("seeme_overlap_cost", jts.data_ptr(), W, K, T, O, cost.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes,
           L.current_stream())
    return cost


def path_select_hip(cost, unary=None) -> Dict[str, torch.Tensor]:
    """cost [W-1,K,K], unary [W,K] or None, fp32 on the device, K <= 32 -> path [W] int64, seam_cost [W-1], path_cost []."""
    L.require_cuda(cost, "cost")
    if unary is not None:
        L.require_cuda(unary, "unary")
    K = int(cost.shape[-1]) if unary is None else int(unary.shape[1])
    W = int(cost.shape[0]) + 1 if unary is None else int(unary.shape[0])
    if cost.dim() != 3 or cost.shape[0] != W - 1 or (W > 1 and tuple(cost.shape[1:]) != (K, K)):
        raise L.SeemeError(f"path_select: cost is {tuple(cost.shape)} for W = {W}, K = {K}: expected [W-1,K,K]")
    return _launch_path(cost.contiguous(), None if unary is None else unary.contiguous(), W, K)


def _launch_path(cost, unary, W, K, ws_bytes=None) -> Dict[str, torch.Tensor]:
    dev = cost.device
    lib = L.lib()
    need = int(lib.seeme_path_select_workspace_bytes(W, K))
    ws = _WS.get(need, dev)
    path = torch.empty(max(W, 0), device=dev, dtype=torch.int32)
    seam = torch.empty(max(W - 1, 0), device=dev, dtype=torch.float32)
    total = torch.empty(1, device=dev, dtype=torch.float32)
    L.call("seeme_path_select", cost.data_ptr(), L.ptr(unary), W, K, path.data_ptr(), seam.data_ptr(), total.data_ptr(), ws.data_ptr(),
           need if ws_bytes is None else ws_bytes, L.current_stream())
    return {"path": path.long(), "seam_cost": seam, "path_cost": total[0]}


def stitch_windows_hip(feats, overlap: int, n_frames: int, layout: int) -> torch.Tensor:
    """feats [W,T,F] renormed features of the chosen hypotheses, fp32 on the device -> [n_frames,F]."""
    L.require_cuda(feats, "feats")
    if feats.dim() != 3:
        raise L.SeemeError(f"stitch_windows: features are {tuple(feats.shape)}: expected [W,T,F]")
    W, T, F = (int(n) for n in feats.shape)
    out = torch.empty(max(int(n_frames), 0), F, device=feats.device, dtype=torch.float32)
    L.call("seeme_stitch_windows", feats.contiguous().data_ptr(), W, T, int(overlap), int(n_frames), F, int(layout), out.data_ptr(),
           L.current_stream())
    return out


def head_path_cost_hip(jts, path, lengths) -> torch.Tensor:
    """jts [W,K,T,24,3], path [W,T,3] fp32 on the device, K <= 32 (``head_path_cost_torch`` serves K > 32), lengths [W] integers ->
    cost [W,K] (mm) (``seeme_head_path_cost``).  Launches on the current stream."""
    n = _check_head_cost(jts, path, lengths)
    if jts.dtype != torch.float32:
        raise ValueError(f"head_path_cost: joints and path must be float32, got {jts.dtype}")
    L.require_cuda(jts, "jts")
    L.require_cuda(path, "path")
    W, K, T = (int(v) for v in jts.shape[:3])
    len32 = torch.tensor(n, dtype=torch.int64).clamp(-1, T).to(device=jts.device, dtype=torch.int32)
    return _launch_head_cost(jts.contiguous(), path.contiguous(), len32, W, K, T)


def _launch_head_cost(jts, path, len32, W, K, T, out=None) -> torch.Tensor:
    """out: the cost tensor to write into (the tests' slot); None operands travel as null pointers."""
    cost = out if out is not None else torch.empty(max(W, 0), max(K, 0), device=jts.device, dtype=torch.float32)
    L.call("seeme_head_path_cost", L.ptr(jts), L.ptr(path), L.ptr(len32), W, K, T, L.ptr(cost), L.current_stream())
    return cost


def head_anchor_hip(joints, path, taps) -> Tuple[torch.Tensor, torch.Tensor]:
    """joints [L,24,3], path [L,3] fp32 on the device, taps [R+1] on the host, R <= 30 (the library validates them) -> (shift [L,3],
    residual [L] in mm) (``seeme_head_anchor``).  Launches on the current stream."""
    _check_head_anchor(joints, path)
    if joints.dtype != torch.float32:
        raise ValueError(f"head_anchor: joints and path must be float32, got {joints.dtype}")
    L.require_cuda(joints, "joints")
    L.require_cuda(path, "path")
    tp = _host_taps(taps, "head_anchor").astype(np.float32)
    return _launch_head_anchor(joints.contiguous(), path.contiguous(), int(joints.shape[0]), tp, tp.shape[0] - 1)


def _launch_head_anchor(joints, path, n_frames, taps, Rr, out=None):
    """taps: float32 numpy on the host or None; out: (shift, residual) to write into (the tests' slots)."""
    import ctypes as C
    dev = (joints if joints is not None else path).device
    if out is None:
        out = (torch.empty(max(n_frames, 0), 3, device=dev, dtype=torch.float32), torch.empty(max(n_frames, 0), device=dev, dtype=torch.float32))
    if taps is not None:
        taps = np.ascontiguousarray(taps, np.float32)
    L.call("seeme_head_anchor", L.ptr(joints), L.ptr(path), n_frames, None if taps is None else taps.ctypes.data_as(C.POINTER(C.c_float)),
           Rr, L.ptr(out[0]), L.ptr(out[1]), L.current_stream())
    return out


def head_rot_cost_hip(feats, layout: int, dev_quat, lengths) -> Dict[str, torch.Tensor]:
    """feats [W,K,T,F] renormed features, dev_quat [W,T,4] fp32 on the device, K <= 32 (``head_rot_cost_torch`` serves K > 32), lengths
    [W] integers -> {"cost" [W,K], "angle" [W,K,T]} (degrees) (``seeme_head_rot_cost``).  Launches on the current stream."""
    n = _check_head_rot_cost(feats, layout, dev_quat, lengths)
    if feats.dtype != torch.float32:
        raise ValueError(f"head_rot_cost: features and dev_quat must be float32, got {feats.dtype}")
    L.require_cuda(feats, "feats")
    L.require_cuda(dev_quat, "dev_quat")
    W, K, T, F = (int(v) for v in feats.shape)
    len32 = torch.tensor(n, dtype=torch.int64).clamp(-1, T).to(device=feats.device, dtype=torch.int32)
    return _launch_head_rot_cost(feats.contiguous(), int(layout), F, dev_quat.contiguous(), len32, W, K, T)


def _launch_head_rot_cost(feats, layout, F, dev_quat, len32, W, K, T, out=None) -> Dict[str, torch.Tensor]:
    """out: {"cost", "angle"} to write into (the tests' slots; "angle" None: not written); None operands travel as null pointers."""
    if out is None:
        dev = next(t for t in (feats, dev_quat, len32) if t is not None).device
        out = {"cost": torch.empty(max(W, 0), max(K, 0), device=dev, dtype=torch.float32),
               "angle": torch.empty(max(W, 0), max(K, 0), max(T, 0), device=dev, dtype=torch.float32)}
    L.call("seeme_head_rot_cost", L.ptr(feats), layout, F, L.ptr(dev_quat), L.ptr(len32), W, K, T, L.ptr(out["cost"]),
           L.ptr(out.get("angle")), L.current_stream())
    return out


def scene_depth_hip(jts, lengths, points, segs, radius) -> Dict[str, torch.Tensor]:
    """jts [W,K,T,J,3], points [N,3] fp32 on the device, lengths [W] integers (an int32 tensor on the device is taken as it is),
    segs [NB,2] and radius [NB] on the host (NB <= 32, indices below J, radii finite and >= 0: the library validates them) ->
    {"depth" [W,K,T] (mm), "cost" [W,K] (mm), "hits" [W,K] int32} (``seeme_scene_depth``).  Launches on the current stream and does
    not synchronise; no workspace."""
    n, sg, rd = _check_scene_depth(jts, lengths, points, segs, radius)
    if jts.dtype != torch.float32:
        raise ValueError(f"scene_depth: joints and points must be float32, got {jts.dtype}")
    L.require_cuda(jts, "jts")
    L.require_cuda(points, "points")
    W, K, T, J = (int(v) for v in jts.shape[:4])
    len32 = n if isinstance(n, torch.Tensor) else torch.tensor(n, dtype=torch.int64).clamp(-1, T).to(device=jts.device, dtype=torch.int32)
    return _launch_scene_depth(jts.contiguous(), len32, points.contiguous(), W, K, T, J, int(points.shape[0]), sg, rd.astype(np.float32),
                               sg.shape[0])


def _launch_scene_depth(jts, len32, points, W, K, T, J, N, segs, radius, NB, out=None) -> Dict[str, torch.Tensor]:
    """segs int32 [NB,2] / radius float32 [NB] numpy on the host, or None; out: {"depth", "cost", "hits"} to write into (the tests'
    slots); None operands travel as null pointers."""
    import ctypes as C
    dev = next(t for t in (jts, points, len32) if t is not None).device
    if out is None:
        out = {"depth": torch.empty(max(W, 0), max(K, 0), max(T, 0), device=dev, dtype=torch.float32),
               "cost": torch.empty(max(W, 0), max(K, 0), device=dev, dtype=torch.float32),
               "hits": torch.empty(max(W, 0), max(K, 0), device=dev, dtype=torch.int32)}
    if segs is not None:
        segs = np.ascontiguousarray(segs, np.int32)
    if radius is not None:
        radius = np.ascontiguousarray(radius, np.float32)
    L.call("seeme_scene_depth", L.ptr(jts), L.ptr(len32), L.ptr(points), W, K, T, J, N,
           None if segs is None else segs.ctypes.data_as(C.POINTER(C.c_int32)),
           None if radius is None else radius.ctypes.data_as(C.POINTER(C.c_float)), NB, L.ptr(out["depth"]), L.ptr(out["cost"]),
           L.ptr(out["hits"]), L.current_stream())
    return out


def scene_views_hip(verts, world2view, P: int) -> Dict[str, torch.Tensor]:
    """verts [N,3], world2view [W,4,4] fp32 on the device -> cloud [W,P,3], index [W,P] int32, count [W] int32
    (``seeme_scene_views``).  Launches on the current stream and does not synchronise."""
    L.require_cuda(verts, "verts")
    L.require_cuda(world2view, "world2view")
    if verts.dim() != 2 or verts.shape[1] != 3 or world2view.dim() != 3 or tuple(world2view.shape[1:]) != (4, 4):
        raise L.SeemeError(f"scene_views: verts are {tuple(verts.shape)}, world2view is {tuple(world2view.shape)}: expected [N,3] and [W,4,4]")
    return _launch_scene_views(verts.contiguous(), world2view.contiguous(), int(P))


def _launch_scene_views(verts, M, P, ws=None, ws_bytes=None, out=None) -> Dict[str, torch.Tensor]:
    """ws / ws_bytes: another workspace and the size to state for it; out: (cloud, index, count) to write into (the tests' slots)."""
    dev = verts.device
    N, W = int(verts.shape[0]), int(M.shape[0])
    lib = L.lib()
    need = int(lib.seeme_scene_views_workspace_bytes(N, W, P))
    if ws is None:
        ws = _WS.get(need, dev)
    if out is None:
        out = (torch.empty(W, max(P, 0), 3, device=dev, dtype=torch.float32), torch.empty(W, max(P, 0), device=dev, dtype=torch.int32),
               torch.empty(W, device=dev, dtype=torch.int32))
    cloud, index, count = out
    L.call("seeme_scene_views", verts.data_ptr(), M.data_ptr(), N, W, P, cloud.data_ptr(), index.data_ptr(), count.data_ptr(),
           ws.data_ptr(), need if ws_bytes is None else ws_bytes, L.current_stream())
    return {"cloud": cloud, "index": index, "count": count}


# ----------------------------------------------------------------------------- recording files
_REC_KEYS = ("global_orient", "body_pose", "transl", "betas")
_FRAME_KEYS = ("video", "video_index", "center", "scale", "image_crops")      # read in the file's own dtype
_IMAGE_SOURCES = ("image_feats", "video", "image_crops")


def _check_frames(rec, n: int, path: str) -> None:
    """The frame keys of a recording with L = n frames: ONE image source, uint8 frames, a box per recording frame with video, and a
    strictly increasing video_index inside 0..L-1 (made the identity when the file has none)."""
    have = [k for k in _IMAGE_SOURCES if k in rec]
    if len(have) > 1:
        raise ValueError(f"{path}: holds {have}; a recording has ONE image source: image_feats, video or image_crops")
    src = have[0] if have and have[0] != "image_feats" else None
    if "video_index" in rec and src is None:
        raise ValueError(f"{path}: video_index names the frames of video or image_crops, and the recording holds neither")
    if src is None:
        for k in ("center", "scale"):                                          # nothing reads them: float32 like every optional key
            if k in rec:
                rec[k] = np.asarray(rec[k], np.float32)
        return
    fr = rec[src]
    tail = "[Lf,H,W,3]" if src == "video" else "[Lf,224,224,3]"
    if fr.dtype != np.uint8 or fr.ndim != 4 or fr.shape[3] != 3 or fr.shape[0] < 1 or (src == "image_crops" and fr.shape[1:3] != (224, 224)):
        raise ValueError(f"{path}: {src} is {fr.shape} {fr.dtype}: expected uint8 {tail} (RGB)")
    if src == "video":
        if min(fr.shape[1:3]) < 1 or max(fr.shape[1:3]) > 16384:
            raise ValueError(f"{path}: video frames are {fr.shape[1]} x {fr.shape[2]}: H and W must be in 1..16384")
        for k, shape in (("center", (n, 2)), ("scale", (n,))):
            if k not in rec:
                raise ValueError(f"{path}: video needs center [L,2] and scale [L], the interactee's box per frame; {k} is missing")
            if rec[k].dtype.kind != "f" or rec[k].shape != shape:
                raise ValueError(f"{path}: {k} is {rec[k].shape} {rec[k].dtype}: expected floats {list(shape)} (L = {n})")
            rec[k] = np.asarray(rec[k], np.float32)
    Lf = fr.shape[0]
    if "video_index" not in rec:
        if Lf != n:
            raise ValueError(f"{path}: {src} holds {Lf} frames and the recording {n}: video_index [Lf] must say which they are")
        rec["video_index"] = np.arange(n, dtype=np.int64)
        return
    vi = rec["video_index"]
    if vi.dtype.kind not in "iu" or vi.shape != (Lf,):
        raise ValueError(f"{path}: video_index is {vi.shape} {vi.dtype}: expected integers [{Lf}], one per frame of {src}")
    vi = rec["video_index"] = vi.astype(np.int64)
    if vi[0] < 0 or vi[-1] >= n or (np.diff(vi) <= 0).any():
        raise ValueError(f"{path}: video_index must be strictly increasing inside 0..{n - 1} (L = {n}), got {vi[:8].tolist()}"
                         f"{' ...' if Lf > 8 else ''} .. {int(vi[-1])}")


def choose_frames(video_index, starts, lengths) -> List[int]:
    """For every window [lo, lo + ln) the POSITION (row of video / image_crops) of the stored frame nearest to its centre frame
    lo + ln // 2 among the stored frames inside the window; a tie goes to the earlier frame.  A window without a stored frame is
    a ValueError that names it."""
    vi = np.asarray(video_index, np.int64)
    rows = []
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        a, b = int(np.searchsorted(vi, lo, "left")), int(np.searchsorted(vi, lo + ln, "left"))      # rows a..b-1 lie in the window
        if a == b:
            raise ValueError(f"windows_batch: window {w} (frames {lo}..{lo + ln - 1}) holds no stored video frame: video_index has "
                             "none inside it")
        d = np.abs(vi[a:b] - (lo + ln // 2))
        rows.append(a + int(np.argmin(d)))                                     # (argmin: the first, so the earlier, of a tie)
    return rows


def check_intrinsics(K, n_frames: int, what: str = "cam_intrinsics") -> np.ndarray:
    """cam_intrinsics, [3] or [L,3] = (f, cx, cy) in pixels -> float32 [L,3]; every value finite and f > 0, or a ValueError that names
    the first frame where not."""
    K = np.asarray(K)
    if K.dtype.kind not in "fiu" or K.shape not in ((3,), (n_frames, 3)):
        raise ValueError(f"{what}: cam_intrinsics is {K.shape} {K.dtype}: expected numbers [3] or [{n_frames},3] = (f, cx, cy) in pixels")
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3), (n_frames, 3))
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(K).all(axis=1) | ~(K[:, 0] > 0)
    if bad.any():
        f = int(np.argmax(bad))
        raise ValueError(f"{what}: cam_intrinsics of frame {f} is {K[f].tolist()}: (f, cx, cy) must be finite with f > 0")
    return np.ascontiguousarray(K, np.float32)


def check_camera_axes(axes, what: str = "TEST.INTERACTEE_CAMERA_AXES") -> Tuple[int, int, int]:
    """Three entries of +-1 with product +1: D = diag(axes) takes the recording's camera frame to the image's OpenCV frame (x right,
    y down, z forward).  [1,-1,-1] is EgoBody's (ADD_TRANS of seeme_amd/data.py), [1,1,1] says world2cam is OpenCV already."""
    try:
        a = [v for v in axes]
    except TypeError:
        a = None
    if a is None or len(a) != 3 or any(isinstance(v, bool) or v not in (1, -1) for v in a) or a[0] * a[1] * a[2] != 1:
        raise ValueError(f"{what} must be three entries of +1 or -1 with product +1 (a rotation), got {axes!r}")
    return tuple(int(v) for v in a)


def opencv_views(world2cam, axes) -> np.ndarray:
    """[L,4,4] float64: D world2cam[l] with D = diag(axes, 1), the map from the recording's world frame to frame l's OpenCV camera frame."""
    D = np.diag(np.array(list(check_camera_axes(axes)) + [1], np.float64))
    return D[None] @ np.asarray(world2cam, np.float64)


def camera_body_to_world(global_orient, cam_t, J0, world2cam, axes):
    """A body estimated in the image's OpenCV camera frame -> the recording's world frame, by the rigid parts of
    inv(D world2cam[l]).  global_orient, cam_t [L,3] or [L,S,3] (axis-angle; ProHMR adds cam_t to the body posed WITHOUT a
    translation, prohmr_scene.py:177-212, and SMPL turns about its rest pelvis, so cam_t is SMPL's transl in that frame); J0 [3] the
    rest pelvis of the betas the body is posed with; world2cam [L,4,4].  -> (global_orient, transl) of the same shapes."""
    inv = rigid_inverse(torch.from_numpy(opencv_views(world2cam, axes)))
    A, a = (t.to(global_orient.device) for t in rigid_parts(inv))
    for _ in range(global_orient.dim() - 2):
        A, a = A[:, None], a[:, None]
    return reframe_smpl(global_orient, cam_t, J0, A, a)


_ESTIMATE_KEYS = ("center", "scale", "cam_intrinsics", "world2cam", "scene_vertices")


def _check_estimate_input(rec, n: int, path: str, allow_sparse: bool = False) -> None:
    """What ``estimate`` reads of a recording without interactee keys: the box, the intrinsics, the camera path, the scene's vertices
    and an image for EVERY recording frame (allow_sparse: for the stored frames of video_index only; ``estimate.py --track`` fills the
    frames between them)."""
    missing = [k for k in _ESTIMATE_KEYS if k not in rec]
    if missing:
        raise ValueError(f"{path}: missing {missing}; estimating the interactee needs {list(_ESTIMATE_KEYS)} and video or image_crops")
    src = "video" if "video" in rec else "image_crops" if "image_crops" in rec else None
    if src is None:
        raise ValueError(f"{path}: holds neither video nor image_crops: the interactee is estimated from the frames' images")
    for k, shape in (("center", (n, 2)), ("scale", (n,))):
        if rec[k].dtype.kind != "f" or rec[k].shape != shape:
            raise ValueError(f"{path}: {k} is {rec[k].shape} {rec[k].dtype}: expected floats {list(shape)} (L = {n})")
        rec[k] = np.asarray(rec[k], np.float32)
    vi = rec["video_index"]
    if vi.shape[0] != n and not allow_sparse:              # strictly increasing inside 0..L-1: fewer than L entries skip a frame
        f = int(np.argmax(vi != np.arange(vi.shape[0]))) if (vi != np.arange(vi.shape[0])).any() else int(vi.shape[0])
        raise ValueError(f"{path}: frame {f} has no stored image (video_index skips it): every recording frame needs one; filling "
                         "between sparse estimates is not built")


def load_recording(path: str, video: Optional[str] = None, require_interactee: bool = True,
                   allow_sparse: bool = False) -> Dict[str, np.ndarray]:
    """A recording ``.npz`` (read with allow_pickle=False: an object array is refused): the INTERACTEE's global_orient [L,3],
    body_pose [L,69|63], transl [L,3], betas [10]; optionally scene [P,3], image_feats [L,2048], wearer_betas [10].  float32.
    A moving camera adds world2cam [L,4,4], the rigid map from the recording's world frame to every frame's camera frame (float64:
    it is composed and inverted), and, in place of scene, scene_vertices [N,3]: the scene's vertices in the world frame, from which
    every window's view is selected (``scene_views_hip``).  head_path [L,3] (floats, finite; returned float64) is the device's position
    in the world frame; when present it is used instead of the centres of world2cam (``camera_centres``), and it also serves
    recordings in one fixed frame that have no world2cam.  head_rot [L,3,3] (floats, rotations to 1e-3; returned float64) is the device's
    orientation, device -> world, in the same way: used instead of the rotations of world2cam (``camera_rotations``) when present.

    The image condition has ONE source: image_feats, or video [Lf,H,W,3] uint8 RGB (decoded frames; needs center [L,2] and scale
    [L], the interactee's box per recording frame, ``crops.patch_box``), or image_crops [Lf,224,224,3] uint8 (patches already cut).
    video_index [Lf] integers names the recording frame of every stored frame, strictly increasing in 0..L-1; without it Lf = L and
    it is the identity.  video and image_crops stay uint8.  `video`: a ``.npy`` of the frames, opened memory-mapped, in place of the
    video key.

    cam_intrinsics, [3] or [L,3] = (f, cx, cy) in pixels, is validated when present (``check_intrinsics``) and returned as [L,3].
    require_interactee=False reads the INPUT of ``estimate``: a recording WITHOUT the four interactee keys, whose
    length L is that of center [L,2]; it needs center, scale, cam_intrinsics, world2cam, scene_vertices and an image per frame.  A
    file that holds interactee keys is refused there: it is an input of predict already.  allow_sparse=True (with
    require_interactee=False) accepts a video_index that skips frames: center / scale / cam_intrinsics / world2cam stay [L,...] and are
    read at the stored frames (``estimate.py --track``, seeme_amd/track.py)."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in _REC_KEYS if k not in z.files]
        if require_interactee and missing:
            raise ValueError(f"{path}: missing {missing}; a recording holds {list(_REC_KEYS)} of the interactee")
        if not require_interactee and len(missing) < len(_REC_KEYS):
            raise ValueError(f"{path}: holds {[k for k in _REC_KEYS if k in z.files]} of the interactee already; require_interactee=False "
                             "reads a recording WITHOUT them (the input of estimate), this one is an input of predict")
        if not require_interactee and "center" not in z.files:
            raise ValueError(f"{path}: missing ['center']; a recording without interactee keys takes its length from center [L,2]")
        intrinsics = z["cam_intrinsics"] if "cam_intrinsics" in z.files else None
        rec = {k: np.asarray(z[k], np.float32) for k in _REC_KEYS + ("scene", "image_feats", "wearer_betas", "scene_vertices")
               if k in z.files}
        if "world2cam" in z.files:
            rec["world2cam"] = np.asarray(z["world2cam"], np.float64)
        head_path = z["head_path"] if "head_path" in z.files else None
        head_rot = z["head_rot"] if "head_rot" in z.files else None
        rec.update({k: z[k] for k in _FRAME_KEYS if k in z.files})
    if video is not None:
        if "video" in rec:
            raise ValueError(f"{path}: holds a video key and {video} was given as well; a recording has ONE image source")
        rec["video"] = np.load(video, mmap_mode="r", allow_pickle=False)
    n = rec["global_orient"].shape[0] if require_interactee else int(np.asarray(rec["center"]).shape[0])
    _check_frames(rec, n, path)
    if intrinsics is not None:
        rec["cam_intrinsics"] = check_intrinsics(intrinsics, n, path)
    want = {"global_orient": [(n, 3)], "body_pose": [(n, 69), (n, 63)], "transl": [(n, 3)], "betas": [(10,)], "wearer_betas": [(10,)],
            "image_feats": [(n, 2048)]}
    if n < 1:
        raise ValueError(f"{path}: the recording has no frame")
    for k, shapes in want.items():
        if k in rec and rec[k].shape not in shapes:
            raise ValueError(f"{path}: {k} is {rec[k].shape}: expected {' or '.join(str(list(s)) for s in shapes)} (L = {n})")
    if "scene" in rec and (rec["scene"].ndim != 2 or rec["scene"].shape[1] != 3 or rec["scene"].shape[0] < 1):
        raise ValueError(f"{path}: scene is {rec['scene'].shape}: expected [P,3]")
    if "scene_vertices" in rec and (rec["scene_vertices"].ndim != 2 or rec["scene_vertices"].shape[1] != 3 or rec["scene_vertices"].shape[0] < 1):
        raise ValueError(f"{path}: scene_vertices is {rec['scene_vertices'].shape}: expected [N,3]")
    if "scene_vertices" in rec and "scene" in rec:
        raise ValueError(f"{path}: holds both scene and scene_vertices; a recording has ONE scene: a fixed cloud, or the vertices "
                         "every window's view is selected from")
    if "scene_vertices" in rec and "world2cam" not in rec:
        raise ValueError(f"{path}: scene_vertices need world2cam: a view is selected per camera pose")
    if "world2cam" in rec:
        check_world2cam(rec["world2cam"], n, path)
    if head_path is not None:
        rec["head_path"] = check_head_path(head_path, n, path)
    if head_rot is not None:
        rec["head_rot"] = check_head_rot(head_rot, n, path)
    if not require_interactee:
        _check_estimate_input(rec, n, path, bool(allow_sparse))
    rec["n_frames"] = n
    return rec


def check_world2cam(M, n_frames: int, what: str = "world2cam") -> None:
    """[L,4,4] rigid maps: last row 0 0 0 1, the 3x3 block orthonormal to 1e-3 with a positive determinant; a ValueError names the
    first frame that is not."""
    M = np.asarray(M, np.float64)
    if M.shape != (n_frames, 4, 4):
        raise ValueError(f"{what}: world2cam is {M.shape}: expected [{n_frames},4,4] (L = {n_frames})")
    A = M[:, :3, :3]
    bad = (np.abs(M[:, 3] - np.array([0.0, 0.0, 0.0, 1.0])).max(axis=1) > 1e-6) | ~np.isfinite(M).all(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        bad |= ~(np.abs(A.transpose(0, 2, 1) @ A - np.eye(3)).max(axis=(1, 2)) <= 1e-3) | ~(np.linalg.det(np.nan_to_num(A)) > 0)
    if bad.any():
        f = int(np.argmax(bad))
        raise ValueError(f"{what}: world2cam of frame {f} is not a rigid map (last row 0 0 0 1, a rotation to 1e-3 with a positive "
                         f"determinant):\n{M[f]}")


def _stats_of(dm_or_stats):
    """(mean [1,D], std [1,D]) as numpy, and the data module's own dataset name / data type when it states them."""
    if isinstance(dm_or_stats, (tuple, list)):
        mean, std = dm_or_stats
        return np.asarray(mean, np.float32).reshape(1, -1), np.asarray(std, np.float32).reshape(1, -1), None, None
    dm = dm_or_stats
    mean, std = (torch.as_tensor(x).detach().float().cpu().numpy().reshape(1, -1) for x in (dm.mean, dm.std))
    if not hasattr(dm, "splits"):            # the synthetic module renorms with the first nfeats statistics
        mean, std = mean[:, :dm.nfeats], std[:, :dm.nfeats]
    return mean, std, getattr(dm, "name", None), getattr(dm, "data_type", None)


def windows_batch(rec, datamodule_or_stats, T: int, overlap: int, condition, dataset: Optional[str] = None,
                  data_type: Optional[str] = None, predict_transl: bool = True, device=None, world2cam=None,
                  scene_points: Optional[int] = None, pelvis=None):
    """The W windows of a recording as ONE batch with the data module's tuple layout (``mld.split_batch``): motion [W,T,2,D], transl
    [W,2,T,3], beta [W,2,T,10], utils [W,T,6], [scene [W,P,3]], [images [W,2048]], length [W,1].  The interactee (slot 1) is
    normalised by the rule the data module applies at load time (``data.normalise_person`` / ``data.normalise_rot6d``: zero padding to
    T first); the wearer's slot (0) is all zeros.  A window's image features are those of its centre frame.  Returns (batch, starts,
    lengths).  datamodule_or_stats: a data module (``mean`` / ``std``) or the pair (mean, std).

    A recording with video or image_crops instead of image_feats: the image slot is uint8 [W,224,224,3], for a model with
    ``model.image_backbone``.  A window takes the stored frame nearest to its centre frame inside the window (``choose_frames``);
    with video only those frames go to `device` and ONE ``crops.crop_patches_hip`` launch cuts their patches around
    ``crops.patch_box`` of the frame's center / scale (without a ROCm `device`: ``crops.crop_patches_torch``, the same bytes).

    A moving camera: world2cam [L,4,4] (default: the recording's own key; without either nothing changes).  Window w is then put
    into the camera frame of its first frame, M_w = world2cam[starts[w]], as the data module does for training: the interactee's
    global_orient / transl are re-framed by M_w (``reframe_smpl``, float64, about `pelvis` [3] = ``rest_pelvis`` of the interactee's
    betas) before the normalisation, and the scene slot holds each window's own view: ``scene_views_hip`` of the recording's
    scene_vertices with `scene_points` rows (default 20000; needs `device`), or the fixed scene cloud moved by M_w.  Returns
    (batch, starts, lengths, frames) with frames = {"world2cam": M [W,4,4] float64, "scene_view_count": count [W] int32 or None}."""
    from .data import load_time_stats, normalise_person, normalise_rot6d
    mean, std, dm_name, dm_type = _stats_of(datamodule_or_stats)
    n = int(rec["n_frames"])
    P = rec["body_pose"].shape[1]
    dataset = dataset or dm_name or ("egobody" if P == 69 else "gimo")
    data_type = data_type or dm_type or "angle"
    if P != (69 if dataset == "egobody" else 63):
        raise ValueError(f"windows_batch: body_pose is {P} wide, dataset '{dataset}' poses {69 if dataset == 'egobody' else 63} values")
    rot6d = data_type == "rot6d"
    starts, lengths = window_plan(n, T, overlap)
    W = len(starts)
    m, s = load_time_stats(mean, std, rot6d)
    w2c = world2cam if world2cam is not None else rec.get("world2cam")
    if w2c is not None:
        check_world2cam(w2c, n, "windows_batch")
        if pelvis is None:
            raise ValueError("windows_batch: world2cam needs pelvis [3], the interactee's rest pelvis (recording.rest_pelvis): SMPL "
                             "rotates about it, so the translation cannot be re-framed without it")
        Mw = torch.from_numpy(np.asarray(w2c, np.float64)[starts])                                  # [W,4,4]
        J0 = torch.as_tensor(pelvis).detach().double().cpu().reshape(3)
    elif "scene_vertices" in rec:
        raise ValueError("windows_batch: scene_vertices need world2cam: a view is selected per camera pose")
    motion = np.zeros((W, T, 2, 3 + P), np.float32)
    transl = np.zeros((W, 2, T, 3), np.float32)
    beta = np.zeros((W, 2, T, 10), np.float32)
    for w, (lo, ln) in enumerate(zip(starts, lengths)):
        go, bp, tr = np.zeros((T, 3), np.float32), np.zeros((T, P), np.float32), np.zeros((T, 3), np.float32)
        go[:ln], bp[:ln], tr[:ln] = rec["global_orient"][lo:lo + ln], rec["body_pose"][lo:lo + ln], rec["transl"][lo:lo + ln]
        if w2c is not None:
            A, a = rigid_parts(Mw[w])
            go_w, tr_w = reframe_smpl(torch.from_numpy(go[:ln]).double(), torch.from_numpy(tr[:ln]).double(), J0, A, a)
            go[:ln], tr[:ln] = go_w.float().numpy(), tr_w.float().numpy()
        motion[w, :, 1], transl[w, 1] = normalise_person(go, bp, tr, m, s, dataset, bool(predict_transl) and not rot6d)
        beta[w, 1, :ln] = rec["betas"]
    length = torch.tensor(lengths, dtype=torch.long).reshape(W, 1)
    motion_t = torch.from_numpy(motion)
    if rot6d:
        motion_t = normalise_rot6d(motion_t, length, mean, std)
        motion_t[:, :, 0] = 0.0                                                # the wearer's slot stays zero
    out = [motion_t, torch.from_numpy(transl), torch.from_numpy(beta), torch.zeros(W, T, 6)]
    view_count = None
    if "scene" in condition:
        if "scene_vertices" in rec:
            if device is None or torch.device(device).type != "cuda":
                raise ValueError("windows_batch: the views of scene_vertices are selected by seeme_scene_views: pass the ROCm device")
            npts = SCENE_VIEW_POINTS if scene_points is None else int(scene_points)
            views = scene_views_hip(torch.from_numpy(rec["scene_vertices"]).to(device), Mw.float().to(device), npts)
            out.append(views["cloud"])
            view_count = views["count"]
        elif "scene" not in rec:
            raise ValueError("windows_batch: the model has a 'scene' condition and the recording holds no scene cloud")
        elif w2c is not None:                                                  # the fixed cloud, moved into each window's frame
            A, a = rigid_parts(Mw)
            out.append((torch.from_numpy(rec["scene"]).double()[None] @ A.transpose(1, 2) + a[:, None]).float().contiguous())
        else:
            out.append(torch.from_numpy(rec["scene"])[None].expand(W, -1, -1).contiguous())
    if "image" in condition:
        if "video" in rec or "image_crops" in rec:                            # uint8 crops [W,224,224,3] for the model's backbone
            from . import crops as CR
            vi = rec["video_index"] if "video_index" in rec else np.arange(n)
            rows = choose_frames(vi, starts, lengths)
            if "video" in rec:                                                 # only the chosen frames go to the device: ONE launch
                uniq, fop = np.unique(np.asarray(rows), return_inverse=True)
                at = np.asarray(vi)[rows]                                      # their recording frames: the boxes' rows
                frames = torch.from_numpy(np.ascontiguousarray(rec["video"][uniq]))
                out.append(CR.crop_patches(frames, fop.reshape(-1), CR.boxes_of(rec["center"][at], rec["scale"][at]), CR.PATCH, device))
            else:
                out.append(torch.from_numpy(np.ascontiguousarray(rec["image_crops"][rows])))
        elif "image_feats" not in rec:
            raise ValueError("windows_batch: the model has an 'image' condition and the recording holds no image_feats")
        else:
            centre = [lo + ln // 2 for lo, ln in zip(starts, lengths)]
            out.append(torch.from_numpy(rec["image_feats"][centre]).contiguous())
    out.append(length)
    if device is not None:
        out = [t.to(device) for t in out]
    if w2c is not None:
        return tuple(out), starts, lengths, {"world2cam": Mw, "scene_view_count": view_count}
    return tuple(out), starts, lengths
