"""Per-hypothesis mesh metrics: PA-MPJPE, V2V and the body-scene contact of the EgoHMR tables (test_egohmr.py:463-492, 540-549).

Frame-level primitives, one float per frame, metres; a frame whose map entry is negative is skipped and gets 0:

``pa_mpjpe_hip`` / ``pa_mpjpe_torch``                mean over the 24 joints of |s R x + t - y| after the similarity transform of
                                                     EgoHMR utils/pose_utils.py:11-59 (reflection correction included)
``v2v_hip`` / ``v2v_torch``                          mean over the vertices of |(v - pelvis) - (v_ref - pelvis_ref)| (test_egohmr.py:485)
``scene_min_dist2_hip`` / ``scene_min_dist2_torch``  min over all vertex x scene-point pairs of the SQUARED distance

The ``_hip`` functions run csrc/mesh_metrics.hip (fp32, on the device, no fallback); the ``_torch`` twins are plain torch, take any
float dtype and any device, and are the test reference.  ``mesh_metrics_eval`` is the driver ``MLD.ego_eval`` calls under
``TEST.MESH_METRICS``; ``MeshMetrics`` keeps the running sums.

Results of the driver are in mm unless a ratio:

  PA_MPJPE, V2V [B,K]        mean over the valid frames of the per-frame value
  SCENE_DIST [B,K]           mean over the valid frames of sqrt(min d^2)
  CONTACT_RATIO [B,K]        share of the valid frames with min d^2 < CONTACT_D2_THRESH
  SCENE_DIST_REF, CONTACT_RATIO_REF [B]   the same for the reference body

``CONTACT_D2_THRESH`` = 0.02 applies to the SQUARED distance in m^2 (a gap of 14.1 cm): the reference compares pytorch3d k-NN
``dists``, which are squared, against 0.02 (test_egohmr.py:548), and the numbers are meant to compare with that table.

The body and the cloud are taken in the coordinates the batch hands over: the data module puts the cloud into the first frame's camera
frame (dataset.py:1270-1284), and the body is there only when the features carry the translation (TRAIN.ABLATION.PREDICT_TRANSL), so
the scene terms mean something only then.  They are absent from the result when the batch has no scene.

Collision (``TEST.COLLISION_METRICS``; EgoHMR models/egohmr/egohmr.py:511-538, eval_coll): the share of the scene cloud that lies inside
the body.  The reference asks a learned occupancy network (COAP) whether a point is inside the posed surface; here that question is
answered exactly, by the winding number of the closed mesh.  A point p against vertices v [V,3] and faces f [NF,3] (closed,
consistently oriented), a, b, c the corners of a face minus p:

  solid angle of a face   Omega = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)      (Van Oosterom-Strackee)
  winding number          w(p) = sum over the faces of Omega / 4 pi
  inside                  |w(p)| >= 0.5: the sign convention of the face table does not matter, and a point in the overlap of two
                          interpenetrating limbs (w = 2) counts once
  degenerate face         a face with two equal indices contributes 0
  zero corner vector      a face with a corner vector of length 0 contributes 0, never NaN (a point ON a vertex or an edge has no
                          defined side; its w is finite)
  bounding-box prefilter  a point outside the closed axis-aligned bounding box of the frame's vertices is not inside (its w is 0, so
                          the filter is exact; egohmr.py:527-531)
  count[f]                the number of points of the frame's cloud that are inside, an integer

``winding_number_hip`` / ``winding_number_torch``          w for every point [F,P], no prefilter
``scene_inside_count_hip`` / ``scene_inside_count_torch``  count [F] int32, with the prefilter
(csrc/collision.hip; the twins as above).  With ``faces`` and a scene the driver adds

  COLLISION_RATIO [B,K]      mean over the valid frames of count / P, P ALL points of the cloud (egohmr.py:534)
  COLLISION_FRAMES [B,K]     share of the valid frames with count > 0
  COLLISION_RATIO_REF, COLLISION_FRAMES_REF [B]   the same for the reference body

and ``CollisionMetrics`` keeps their running sums.  ``check_closed_faces`` says whether a face table is one the test is defined for;
``uv_sphere`` is a closed body with SMPL's counts for tests, benchmarks and a synthetic SMPL (whose own table is all zeros).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import _lib as L

CONTACT_D2_THRESH = 0.02       # m^2: a threshold on the SQUARED distance (test_egohmr.py:548), i.e. 14.1 cm
PER_HYP = ("PA_MPJPE", "V2V")
SCENE_HYP = ("SCENE_DIST", "CONTACT_RATIO")
SCENE_REF = ("SCENE_DIST_REF", "CONTACT_RATIO_REF")
COLLISION_HYP = ("COLLISION_RATIO", "COLLISION_FRAMES")
COLLISION_REF = ("COLLISION_RATIO_REF", "COLLISION_FRAMES_REF")


def _map(ref_of_frame, F: int, device) -> torch.Tensor:
    if ref_of_frame is None:
        return torch.arange(F, device=device, dtype=torch.long)
    return torch.as_tensor(ref_of_frame, device=device).reshape(F).long()


# ----------------------------------------------------------------------------- plain-torch twins
def pa_mpjpe_torch(j_pred, j_ref, ref_of_frame=None) -> torch.Tensor:
    """j_pred [F,J,3], j_ref [Fr,J,3] -> [F].  pose_utils.compute_similarity_transform step by step (S1 = prediction, S2 = reference)."""
    F = j_pred.shape[0]
    m = _map(ref_of_frame, F, j_pred.device)
    on = m >= 0
    S1, S2 = j_pred.transpose(1, 2), j_ref.to(j_pred.dtype)[m.clamp_min(0)].transpose(1, 2)        # [F,3,J]
    mu1, mu2 = S1.mean(dim=2, keepdim=True), S2.mean(dim=2, keepdim=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = (X1 ** 2).sum(dim=(1, 2))
    Km = X1 @ X2.transpose(1, 2)
    U, _, Vh = torch.linalg.svd(Km)
    Vm = Vh.transpose(1, 2)
    Z = torch.eye(3, dtype=j_pred.dtype, device=j_pred.device).repeat(F, 1, 1)
    Z[:, 2, 2] = torch.sign(torch.linalg.det(U @ Vm.transpose(1, 2)))
    R = Vm @ (Z @ U.transpose(1, 2))
    scale = (R @ Km).diagonal(dim1=1, dim2=2).sum(dim=1) / var1
    t = mu2 - scale[:, None, None] * (R @ mu1)
    S1_hat = scale[:, None, None] * (R @ S1) + t
    err = (S1_hat - S2).norm(dim=1).mean(dim=1)
    return torch.where(on, err, torch.zeros_like(err))


def v2v_torch(v_pred, pel_pred, v_ref, pel_ref, ref_of_frame=None) -> torch.Tensor:
    """v_pred [F,V,3], pel_pred [F,3], v_ref [Fr,V,3], pel_ref [Fr,3] -> [F]."""
    F = v_pred.shape[0]
    m = _map(ref_of_frame, F, v_pred.device)
    on = m >= 0
    mi = m.clamp_min(0)
    dt = v_pred.dtype
    d = (v_pred - pel_pred[:, None]) - (v_ref.to(dt)[mi] - pel_ref.to(dt)[mi][:, None])
    err = d.norm(dim=-1).mean(dim=-1)
    return torch.where(on, err, torch.zeros_like(err))


def scene_min_dist2_torch(verts, scene, scene_of_frame=None, chunk: int = 512) -> torch.Tensor:
    """verts [F,V,3], scene [S,P,3] -> [F]: min over the V x P pairs of dx^2 + dy^2 + dz^2, `chunk` scene points at a time (float64 at
    V = 6890, P = 20 000 then needs 85 MB, not 3.3 GB)."""
    F = verts.shape[0]
    m = _map(scene_of_frame, F, verts.device)
    out = torch.zeros(F, dtype=verts.dtype, device=verts.device)
    P = scene.shape[1]
    for f in range(F):
        if int(m[f]) < 0:
            continue
        s = scene[int(m[f])].to(verts.dtype)
        best = None
        for p0 in range(0, P, chunk):
            d = verts[f][:, None, :] - s[None, p0:p0 + chunk, :]
            v = (d * d).sum(dim=-1).min()
            best = v if best is None else torch.minimum(best, v)
        out[f] = best
    return out


# ----------------------------------------------------------------------------- closed meshes and the winding number
def uv_sphere(rings: int, segments: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Closed unit sphere: north pole, `rings` latitude rings of `segments` vertices, south pole -> (verts [2 + rings*segments, 3]
    float64, faces [2*rings*segments, 3] int64), wound counter-clockwise seen from outside, so that w = +1 inside.
    uv_sphere(84, 82) has SMPL's 6890 vertices and 13 776 faces."""
    if rings < 1 or segments < 3:
        raise ValueError(f"uv_sphere: rings must be >= 1 and segments >= 3, got {rings}, {segments}")
    th = torch.arange(1, rings + 1, dtype=torch.float64) * (math.pi / (rings + 1))          # polar angle of ring r
    ph = torch.arange(segments, dtype=torch.float64) * (2 * math.pi / segments)
    ring = torch.stack([th.sin()[:, None] * ph.cos()[None, :], th.cos()[:, None].expand(rings, segments),
                        th.sin()[:, None] * ph.sin()[None, :]], dim=-1).reshape(-1, 3)
    verts = torch.cat([torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float64), ring, torch.tensor([[0.0, -1.0, 0.0]], dtype=torch.float64)])
    idx = lambda r, s: 1 + r * segments + s % segments
    south = 1 + rings * segments
    faces = []
    for s_ in range(segments):
        faces.append((0, idx(0, s_ + 1), idx(0, s_)))
        for r in range(rings - 1):
            a, b, c, d = idx(r, s_), idx(r, s_ + 1), idx(r + 1, s_), idx(r + 1, s_ + 1)
            faces += [(a, b, d), (a, d, c)]
        faces.append((south, idx(rings - 1, s_), idx(rings - 1, s_ + 1)))
    return verts, torch.tensor(faces, dtype=torch.long)


def check_closed_faces(faces, V: int) -> None:
    """ValueError unless `faces` [NF,3] is the table of a closed, consistently oriented mesh on V vertices: every index in 0..V-1,
    every directed edge exactly once and its reverse present."""
    f = torch.as_tensor(faces).detach().cpu().long()
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] < 4:
        raise ValueError(f"face table is {tuple(f.shape)}: expected [NF,3] with NF >= 4")
    if not bool(f.any()):
        raise ValueError("the face table is all zeros (as in SMPL.synthetic(), which carries no mesh): the point-in-mesh test needs "
                         "a closed face table, e.g. the SMPL model file's or uv_sphere's")
    if int(f.min()) < 0 or int(f.max()) >= V:
        raise ValueError(f"face indices run from {int(f.min())} to {int(f.max())} with {V} vertices")
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if bool((e[:, 0] == e[:, 1]).any()):
        raise ValueError("the face table has a face with two equal indices")
    code, rev = e[:, 0] * V + e[:, 1], e[:, 1] * V + e[:, 0]
    uniq, cnt = torch.unique(code, return_counts=True)
    if bool((cnt != 1).any()):
        raise ValueError(f"the face table is not consistently oriented: {int((cnt != 1).sum())} directed edges occur more than once")
    missing = ~torch.isin(rev, uniq)
    if bool(missing.any()):
        raise ValueError(f"the face table is not closed: {int(missing.sum())} edges have no opposite face")


def _live_faces(faces, V: int, device) -> torch.Tensor:
    """The faces that count: every index in range and all three different."""
    f = torch.as_tensor(faces).to(device).long().reshape(-1, 3)
    ok = ((f >= 0) & (f < V)).all(dim=1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return f[ok]


def _winding(tri: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """tri [NF,3,3], p [n,3] -> w [n], straight from the formula."""
    a, b, c = (tri[None, :, i] - p[:, None] for i in range(3))                   # [n,NF,3]
    la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
    num = (a * torch.linalg.cross(b, c, dim=-1)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    h = torch.atan2(num, den)
    h = torch.where((la == 0) | (lb == 0) | (lc == 0), torch.zeros_like(h), h)
    return 2.0 * h.sum(dim=-1) / (4.0 * math.pi)


def winding_number_torch(verts, faces, points, points_of_frame=None, chunk: Optional[int] = None) -> torch.Tensor:
    """verts [F,V,3], faces [NF,3], points [S,P,3] -> w [F,P] in verts' dtype, `chunk` points at a time (default: 2^20 (point, face)
    pairs per step).  No prefilter; a skipped frame gets zeros."""
    F, V = int(verts.shape[0]), int(verts.shape[1])
    m = _map(points_of_frame, F, verts.device)
    fa = _live_faces(faces, V, verts.device)
    P = int(points.shape[1])
    chunk = chunk or max(1, (1 << 20) // max(int(fa.shape[0]), 1))
    out = torch.zeros(F, P, dtype=verts.dtype, device=verts.device)
    for f in range(F):
        if int(m[f]) < 0:
            continue
        tri, pts = verts[f][fa], points[int(m[f])].to(verts.dtype)
        for p0 in range(0, P, chunk):
            out[f, p0:p0 + chunk] = _winding(tri, pts[p0:p0 + chunk])
    return out


def scene_inside_count_torch(verts, faces, scene, scene_of_frame=None, chunk: Optional[int] = None) -> torch.Tensor:
    """verts [F,V,3], faces [NF,3], scene [S,P,3] -> int32 [F]: the points of the frame's cloud with |w| >= 0.5 among those inside the
    closed bounding box of the frame's vertices."""
    F, V = int(verts.shape[0]), int(verts.shape[1])
    m = _map(scene_of_frame, F, verts.device)
    fa = _live_faces(faces, V, verts.device)
    chunk = chunk or max(1, (1 << 20) // max(int(fa.shape[0]), 1))
    out = torch.zeros(F, dtype=torch.int32, device=verts.device)
    for f in range(F):
        if int(m[f]) < 0:
            continue
        pts = scene[int(m[f])].to(verts.dtype)
        lo, hi = verts[f].min(dim=0).values, verts[f].max(dim=0).values
        pts = pts[((pts >= lo) & (pts <= hi)).all(dim=1)]
        tri, n = verts[f][fa], 0
        for p0 in range(0, int(pts.shape[0]), chunk):
            n += int((_winding(tri, pts[p0:p0 + chunk]).abs() >= 0.5).sum())
        out[f] = n
    return out


# ----------------------------------------------------------------------------- the kernels
def _i32(ref_of_frame, F: int, device) -> torch.Tensor:
    if ref_of_frame is None:
        return torch.arange(F, device=device, dtype=torch.int32)
    return torch.as_tensor(ref_of_frame).reshape(F).to(device=device, dtype=torch.int32).contiguous()


def _check_map(m: torch.Tensor, n: int, what: str):
    if m.numel() and int(m.max()) >= n:
        raise L.SeemeError(f"{what}: a map entry is {int(m.max())} with only {n} rows to point at")


def pa_mpjpe_hip(j_pred, j_ref, ref_of_frame=None) -> torch.Tensor:
    """j_pred [F,24,3], j_ref [Fr,24,3], fp32 on the device -> [F]."""
    L.require_cuda(j_pred, "j_pred")
    L.require_cuda(j_ref, "j_ref")
    F = int(j_pred.shape[0])
    if tuple(j_pred.shape[1:]) != (24, 3) or tuple(j_ref.shape[1:]) != (24, 3):
        raise L.SeemeError(f"pa_mpjpe: joints are {tuple(j_pred.shape)} / {tuple(j_ref.shape)}: expected [F,24,3] / [Fr,24,3]")
    m = _i32(ref_of_frame, F, j_pred.device)
    _check_map(m, int(j_ref.shape[0]), "pa_mpjpe")
    jp, jr = j_pred.contiguous(), j_ref.contiguous()
    out = torch.empty(max(F, 0), device=j_pred.device, dtype=torch.float32)
    L.call("seeme_pa_mpjpe_frames", jp.data_ptr(), jr.data_ptr(), m.data_ptr(), F, out.data_ptr(), L.current_stream())
    return out


def v2v_hip(v_pred, pel_pred, v_ref, pel_ref, ref_of_frame=None) -> torch.Tensor:
    """v_pred [F,V,3], pel_pred [F,3], v_ref [Fr,V,3], pel_ref [Fr,3], fp32 on the device -> [F]."""
    for t, n in ((v_pred, "v_pred"), (pel_pred, "pel_pred"), (v_ref, "v_ref"), (pel_ref, "pel_ref")):
        L.require_cuda(t, n)
    F, V = int(v_pred.shape[0]), int(v_pred.shape[1]) if v_pred.dim() == 3 else 0
    if v_pred.dim() != 3 or v_ref.dim() != 3 or v_pred.shape[2] != 3 or tuple(v_ref.shape[1:]) != (V, 3) \
            or tuple(pel_pred.shape) != (F, 3) or tuple(pel_ref.shape) != (int(v_ref.shape[0]), 3):
        raise L.SeemeError(f"v2v: shapes {tuple(v_pred.shape)} {tuple(pel_pred.shape)} {tuple(v_ref.shape)} {tuple(pel_ref.shape)}: "
                           "expected [F,V,3] [F,3] [Fr,V,3] [Fr,3]")
    m = _i32(ref_of_frame, F, v_pred.device)
    _check_map(m, int(v_ref.shape[0]), "v2v")
    # the kernel's 16-byte loads need aligned bases: a slice of a larger buffer (frames of 6890 vertices are 8 bytes off) is copied
    al = lambda t: t.contiguous() if t.contiguous().data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)
    vp, pp, vr, pr = al(v_pred), pel_pred.contiguous(), al(v_ref), pel_ref.contiguous()
    out = torch.empty(max(F, 0), device=v_pred.device, dtype=torch.float32)
    L.call("seeme_mesh_v2v_frames", vp.data_ptr(), pp.data_ptr(), vr.data_ptr(), pr.data_ptr(), m.data_ptr(), F, V, out.data_ptr(),
           L.current_stream())
    return out


_WS = L.Workspace(per_stream=True)    # shared by scene_min_dist2 and scene_inside_count: launches of one stream run in order


def scene_min_dist2_hip(verts, scene, scene_of_frame=None, ws_bytes=None) -> torch.Tensor:
    """verts [F,V,3], scene [S,P,3], fp32 on the device -> [F] squared metres.  Without a map frame f uses scene f."""
    L.require_cuda(verts, "verts")
    L.require_cuda(scene, "scene")
    if verts.dim() != 3 or scene.dim() != 3 or verts.shape[2] != 3 or scene.shape[2] != 3:
        raise L.SeemeError(f"scene_min_dist2: shapes {tuple(verts.shape)} / {tuple(scene.shape)}: expected [F,V,3] / [S,P,3]")
    F, V, S, P = int(verts.shape[0]), int(verts.shape[1]), int(scene.shape[0]), int(scene.shape[1])
    dev = verts.device
    m = _i32(scene_of_frame, F, dev)
    _check_map(m, S, "scene_min_dist2")
    lib = L.lib()
    need = int(lib.seeme_scene_min_dist2_workspace_bytes(F, V, S, P))
    ws = _WS.get(need, dev)
    vs, sc = verts.contiguous(), scene.contiguous()
    out = torch.empty(max(F, 0), device=dev, dtype=torch.float32)
    L.call("seeme_scene_min_dist2", vs.data_ptr(), sc.data_ptr(), m.data_ptr(), F, V, S, P, out.data_ptr(), ws.data_ptr(),
           need if ws_bytes is None else ws_bytes, L.current_stream())
    return out


_FACES: List = []              # [source tensor, its version, V, device, int32 copy on the device]: the table checked last


def _faces_i32(faces, V: int, device) -> torch.Tensor:
    """The face table as contiguous int32 on the device, every index checked once against 0..V-1 (the check reads the table back, so
    its result is kept for as long as the same tensor comes again)."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.dtype not in (
            torch.int32, torch.int64):
        raise L.SeemeError("faces must be an int32 or int64 tensor [NF,3] with NF >= 1")
    c = _FACES
    if c and c[0] is faces and c[1] == faces._version and c[2] == V and c[3] == device:
        return c[4]
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= V:
        raise L.SeemeError(f"a face index is {lo if lo < 0 else hi} with {V} vertices: indices must be in 0..V-1")
    f32 = faces.to(device=device, dtype=torch.int32).contiguous()
    c[:] = [faces, faces._version, V, device, f32]
    return f32


def _mesh_args(verts, faces, points, what: str):
    L.require_cuda(verts, "verts")
    L.require_cuda(points, what)
    if verts.dim() != 3 or points.dim() != 3 or verts.shape[2] != 3 or points.shape[2] != 3:
        raise L.SeemeError(f"shapes {tuple(verts.shape)} / {tuple(points.shape)}: expected verts [F,V,3] and {what} [S,P,3]")
    F, V, S, P = int(verts.shape[0]), int(verts.shape[1]), int(points.shape[0]), int(points.shape[1])
    return F, V, S, P, _faces_i32(faces, V, verts.device)


def winding_number_hip(verts, faces, points, points_of_frame=None) -> torch.Tensor:
    """verts [F,V,3], points [S,P,3] fp32 on the device, faces [NF,3] int -> w [F,P], every point, no prefilter.  Without a map frame f
    uses cloud f."""
    F, V, S, P, fa = _mesh_args(verts, faces, points, "points")
    dev = verts.device
    m = _i32(points_of_frame, F, dev)
    _check_map(m, S, "winding_number")
    vs, pt = verts.contiguous(), points.contiguous()
    out = torch.empty(max(F, 0), max(P, 0), device=dev, dtype=torch.float32)
    L.call("seeme_mesh_winding", vs.data_ptr(), fa.data_ptr(), int(fa.shape[0]), pt.data_ptr(), m.data_ptr(), F, V, S, P,
           out.data_ptr(), L.current_stream())
    return out


def scene_inside_count_hip(verts, faces, scene, scene_of_frame=None, ws_bytes=None) -> torch.Tensor:
    """verts [F,V,3], scene [S,P,3] fp32 on the device, faces [NF,3] int -> int32 [F]: the points of the frame's cloud inside the mesh.
    Without a map frame f uses scene f."""
    F, V, S, P, fa = _mesh_args(verts, faces, scene, "scene")
    dev = verts.device
    m = _i32(scene_of_frame, F, dev)
    _check_map(m, S, "scene_inside_count")
    lib = L.lib()
    need = int(lib.seeme_scene_inside_count_workspace_bytes(F, V, S, P))
    ws = _WS.get(need, dev)
    vs, sc = verts.contiguous(), scene.contiguous()
    out = torch.empty(max(F, 0), device=dev, dtype=torch.int32)
    L.call("seeme_scene_inside_count", vs.data_ptr(), fa.data_ptr(), int(fa.shape[0]), sc.data_ptr(), m.data_ptr(), F, V, S, P,
           out.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, L.current_stream())
    return out


# ----------------------------------------------------------------------------- the driver of ego_eval
PoseFn = Callable[[torch.Tensor, torch.Tensor, Optional[torch.Tensor]], Tuple[torch.Tensor, torch.Tensor]]


def frame_chunks(lengths: List[int], T: int, frames_per_chunk: int) -> List[List[Tuple[int, int, int]]]:
    """The valid frames of the batch as chunks of pieces (b, t0, t1), at most `frames_per_chunk` reference frames per chunk."""
    chunks, cur, room = [], [], frames_per_chunk
    for b, n in enumerate(lengths):
        t0, n = 0, max(0, min(int(n), T))
        while t0 < n:
            t1 = min(n, t0 + room)
            cur.append((b, t0, t1))
            room -= t1 - t0
            t0 = t1
            if room == 0:
                chunks.append(cur)
                cur, room = [], frames_per_chunk
    if cur:
        chunks.append(cur)
    return chunks


def mesh_metrics_eval(pose: PoseFn, f_rst, f_ref, betas, orient, lengths, K: int, scene=None, chunk_mb: float = 256,
                      num_vertices: int = 6890, faces=None, mesh: bool = True) -> Dict[str, torch.Tensor]:
    """f_rst [B*K,T,F] renormed features of the hypotheses (row b*K + k), f_ref [B,T,F] of the reference, betas [B,T,10], orient
    [B,T,3] or None (the orientation every body of sequence b is posed with instead of its own), scene [B,P,3] or None.
    pose(feats [1,N,F], betas [1,N,10], orient [1,N,3] | None) -> (joints [1,N,24,3], vertices [1,N,V,3]).

    The valid frames are walked in chunks of n reference frames and their n*K hypothesis frames, n such that the (K+1)*n meshes of a
    chunk stay under `chunk_mb` MiB; per chunk the bodies are posed, the three kernels run, and only the per-frame floats are kept:
    B*K*T meshes are never resident at once.  A frame's value does not depend on the chunking.

    faces [NF,3] (with a scene): the collision keys are added, from the SAME posed chunks (a chunk is posed once whatever is asked
    for).  mesh False leaves the keys of TEST.MESH_METRICS out, and their kernels."""
    B, T = int(f_ref.shape[0]), int(f_ref.shape[1])
    dev = f_ref.device
    if int(f_rst.shape[0]) != B * K or int(f_rst.shape[1]) != T:
        raise ValueError(f"mesh_metrics_eval: f_rst is {tuple(f_rst.shape)} for B = {B}, K = {K}, T = {T}")
    lengths = [int(l) for l in lengths]
    per_mesh = num_vertices * 3 * 4
    n_max = max(1, int(chunk_mb * (1 << 20)) // ((K + 1) * per_mesh))
    pa = torch.zeros(B, K, T, device=dev, dtype=torch.float32)
    vv = torch.zeros_like(pa)
    d2 = torch.zeros_like(pa) if scene is not None else None
    d2r = torch.zeros(B, T, device=dev, dtype=torch.float32) if scene is not None else None
    coll = faces is not None and scene is not None
    cnt = torch.zeros(B, K, T, device=dev, dtype=torch.int32) if coll else None
    cntr = torch.zeros(B, T, device=dev, dtype=torch.int32) if coll else None
    if scene is not None:
        scene = scene.float().contiguous()
    ks = torch.arange(K, device=dev)
    for pieces in frame_chunks(lengths, T, n_max):
        bs = torch.cat([torch.full((t1 - t0,), b, dtype=torch.long) for b, t0, t1 in pieces]).to(dev)
        ts = torch.cat([torch.arange(t0, t1, dtype=torch.long) for _, t0, t1 in pieces]).to(dev)
        n = int(bs.numel())
        # hypothesis frames first, frame-major (i*K + k), then the n reference frames
        rows = (bs[:, None] * K + ks[None, :]).reshape(-1)
        tt = ts[:, None].expand(n, K).reshape(-1)
        feats = torch.cat([f_rst[rows, tt], f_ref[bs, ts]], dim=0)[None]
        b_all = torch.cat([bs[:, None].expand(n, K).reshape(-1), bs])
        t_all = torch.cat([tt, ts])
        joints, verts = pose(feats.contiguous(), betas[b_all, t_all][None].contiguous(),
                             None if orient is None else orient[b_all, t_all][None].contiguous())
        joints, verts = joints[0].contiguous(), verts[0].contiguous()
        rof = torch.arange(n, device=dev, dtype=torch.int32)[:, None].expand(n, K).reshape(-1).contiguous()
        jp, jr, vp = joints[:n * K], joints[n * K:], verts[:n * K]
        bk = bs[:, None].expand(n, K).reshape(-1)
        kk = ks[None, :].expand(n, K).reshape(-1)
        if mesh:
            pa[bk, kk, tt] = pa_mpjpe_hip(jp, jr, rof)
            # the references are rows n*K .. of the same buffers: the map points there, no slice (whose base may be off 16 bytes), no copy
            vv[bk, kk, tt] = v2v_hip(vp, jp[:, 0].contiguous(), verts, joints[:, 0].contiguous(), rof + n * K)
        if mesh and scene is not None:
            dd = scene_min_dist2_hip(verts, scene, b_all.to(torch.int32))
            d2[bk, kk, tt] = dd[:n * K]
            d2r[bs, ts] = dd[n * K:]
        if coll:
            cc = scene_inside_count_hip(verts, faces, scene, b_all.to(torch.int32))
            cnt[bk, kk, tt] = cc[:n * K]
            cntr[bs, ts] = cc[n * K:]
        del joints, verts, jp, jr, vp
    lens = torch.as_tensor(lengths, device=dev).reshape(B)
    mask = (torch.arange(T, device=dev)[None, :] < lens[:, None]).to(torch.float32)            # [B,T]
    flen = lens.to(torch.float32)
    mean_bk = lambda x: (x * mask[:, None, :]).sum(dim=-1) / flen[:, None]
    out = {"PA_MPJPE": mean_bk(pa) * 1000.0, "V2V": mean_bk(vv) * 1000.0} if mesh else {}
    if mesh and scene is not None:
        out["SCENE_DIST"] = mean_bk(d2.sqrt()) * 1000.0
        out["CONTACT_RATIO"] = mean_bk((d2 < CONTACT_D2_THRESH).to(torch.float32))
        out["SCENE_DIST_REF"] = (d2r.sqrt() * mask).sum(dim=-1) / flen * 1000.0
        out["CONTACT_RATIO_REF"] = ((d2r < CONTACT_D2_THRESH).to(torch.float32) * mask).sum(dim=-1) / flen
    if coll:
        out.update(collision_from_counts(cnt, cntr, lengths, int(scene.shape[1])))
    return out


def collision_from_counts(cnt, cnt_ref, lengths, P: int) -> Dict[str, torch.Tensor]:
    """cnt [B,K,T], cnt_ref [B,T] integer counts of inside points per frame, P points per cloud -> the four collision keys, fp32; the
    means over the valid frames are taken in float64 and rounded once."""
    B, K, T = cnt.shape
    dev = cnt.device
    lens = torch.as_tensor([int(l) for l in lengths], device=dev).reshape(B)
    mask = (torch.arange(T, device=dev)[None, :] < lens[:, None]).double()
    flen = lens.double()
    mean_bk = lambda x: ((x * mask[:, None, :]).sum(dim=-1) / flen[:, None]).float()
    mean_b = lambda x: ((x * mask).sum(dim=-1) / flen).float()
    return {"COLLISION_RATIO": mean_bk(cnt.double() / P), "COLLISION_FRAMES": mean_bk((cnt > 0).double()),
            "COLLISION_RATIO_REF": mean_b(cnt_ref.double() / P), "COLLISION_FRAMES_REF": mean_b((cnt_ref > 0).double())}


def collision_from_meshes_torch(v_pred, v_ref, faces, lengths, scene) -> Dict[str, torch.Tensor]:
    """The driver's collision keys from resident meshes through the twin: v_pred [B,K,T,V,3], v_ref [B,T,V,3], scene [B,P,3]; any
    float dtype, any device.  `_count` [B,K,T] and `_count_ref` [B,T] come along (0 at frames past a length)."""
    B, K, T, V = v_pred.shape[:4]
    dev = v_pred.device
    lens = torch.as_tensor([int(l) for l in lengths], device=dev).reshape(B)
    sof = torch.arange(B, device=dev)[:, None].expand(B, T)
    sof = torch.where(torch.arange(T, device=dev)[None, :] < lens[:, None], sof, torch.full_like(sof, -1))
    sc = scene.to(v_pred.dtype)
    cnt = scene_inside_count_torch(v_pred.reshape(-1, V, 3), faces, sc, sof[:, None, :].expand(B, K, T).reshape(-1)).reshape(B, K, T)
    cntr = scene_inside_count_torch(v_ref.reshape(-1, V, 3), faces, sc, sof.reshape(-1)).reshape(B, T)
    out = collision_from_counts(cnt, cntr, lengths, int(scene.shape[1]))
    out["_count"], out["_count_ref"] = cnt, cntr
    return out


def mesh_metrics_from_meshes_torch(j_pred, v_pred, j_ref, v_ref, lengths, scene=None) -> Dict[str, torch.Tensor]:
    """The driver's result from resident meshes through the twins: j_pred [B,K,T,24,3], v_pred [B,K,T,V,3], j_ref [B,T,24,3], v_ref
    [B,T,V,3], scene [B,P,3] or None; any float dtype, any device.  (Small inputs: this is the reference of the tests.)"""
    B, K, T = j_pred.shape[:3]
    V = v_pred.shape[3]
    dev, dt = j_pred.device, j_pred.dtype
    lens = torch.as_tensor([int(l) for l in lengths], device=dev).reshape(B)
    mask = (torch.arange(T, device=dev)[None, :] < lens[:, None]).to(dt)
    flen = lens.to(dt)
    rof = (torch.arange(B * T, device=dev).reshape(B, 1, T).expand(B, K, T)).reshape(-1)
    pa = pa_mpjpe_torch(j_pred.reshape(-1, 24, 3), j_ref.reshape(-1, 24, 3), rof).reshape(B, K, T)
    vv = v2v_torch(v_pred.reshape(-1, V, 3), j_pred[..., 0, :].reshape(-1, 3), v_ref.reshape(-1, V, 3), j_ref[..., 0, :].reshape(-1, 3),
                   rof).reshape(B, K, T)
    mean_bk = lambda x: (x * mask[:, None, :]).sum(dim=-1) / flen[:, None]
    out = {"PA_MPJPE": mean_bk(pa) * 1000.0, "V2V": mean_bk(vv) * 1000.0}
    if scene is not None:
        valid = mask > 0
        sof = torch.arange(B, device=dev)[:, None].expand(B, T)
        sof = torch.where(valid, sof, torch.full_like(sof, -1))
        d2 = scene_min_dist2_torch(v_pred.reshape(-1, V, 3), scene.to(dt), sof[:, None, :].expand(B, K, T).reshape(-1)).reshape(B, K, T)
        d2r = scene_min_dist2_torch(v_ref.reshape(-1, V, 3), scene.to(dt), sof.reshape(-1)).reshape(B, T)
        out["SCENE_DIST"] = mean_bk(d2.sqrt()) * 1000.0
        out["CONTACT_RATIO"] = mean_bk((d2 < CONTACT_D2_THRESH).to(dt) * mask[:, None, :])
        out["SCENE_DIST_REF"] = (d2r.sqrt() * mask).sum(dim=-1) / flen * 1000.0
        out["CONTACT_RATIO_REF"] = ((d2r < CONTACT_D2_THRESH).to(dt) * mask).sum(dim=-1) / flen
        out["_d2"], out["_d2_ref"] = d2, d2r
    return out


class MeshMetrics:
    """Running sums of the mesh metrics, one float64 device vector of eleven entries (reduced over ranks like HypothesisMetrics'
    sums): [sum best-of-K PA-MPJPE, sum mean-of-K PA-MPJPE, sum best-of-K V2V, sum mean-of-K V2V, sequences with a kept hypothesis,
    sum CONTACT_RATIO, sum SCENE_DIST, (b,k) pairs with a scene, sum CONTACT_RATIO_REF, sum SCENE_DIST_REF, sequences with a scene].
    best / mean run over the hypotheses ``keep`` marks (the inclusion mask of HypothesisMetrics; for K = 1 the same rule on that
    batch's per-sequence errors); the scene numbers run over all hypotheses and all sequences."""

    NAMES = ("PA_MPJPE_best_of_k", "PA_MPJPE_mean_of_k", "V2V_best_of_k", "V2V_mean_of_k")
    SCENE_NAMES = ("CONTACT_RATIO", "SCENE_DIST", "CONTACT_RATIO_REF", "SCENE_DIST_REF")

    def __init__(self):
        self.reset()

    def reset(self):
        self._sums = None

    def update(self, mm: Dict[str, torch.Tensor], keep: torch.Tensor):
        """mm: ``rs['mesh_metrics']`` of ``MLD.ego_eval``; keep [B,K] bool."""
        pa = mm["PA_MPJPE"].double()
        dev = pa.device
        keep = keep.to(dev)
        n = keep.sum(dim=1)
        any_ = n > 0
        zero = torch.zeros_like(pa[:, 0])
        vals = []
        for name in ("PA_MPJPE", "V2V"):
            x = mm[name].double()
            best = torch.where(any_, torch.where(keep, x, torch.full_like(x, float("inf"))).min(dim=1).values, zero)
            mean = torch.where(any_, (x * keep).sum(dim=1) / n.clamp_min(1), zero)
            vals += [best.sum(), mean.sum()]
        vals.append(any_.sum().double())
        z = torch.zeros((), dtype=torch.float64, device=dev)
        if "CONTACT_RATIO" in mm:
            cnt = lambda t: torch.tensor(float(t.numel()), dtype=torch.float64, device=dev)
            vals += [mm["CONTACT_RATIO"].double().sum(), mm["SCENE_DIST"].double().sum(), cnt(mm["CONTACT_RATIO"]),
                     mm["CONTACT_RATIO_REF"].double().sum(), mm["SCENE_DIST_REF"].double().sum(), cnt(mm["CONTACT_RATIO_REF"])]
        else:
            vals += [z, z, z, z, z, z]
        vals = torch.stack(vals)
        self._sums = vals if self._sums is None else self._sums + vals

    def sums(self):
        return torch.zeros(11, dtype=torch.float64) if self._sums is None else self._sums

    def compute(self, sums=None):
        s = (self.sums() if sums is None else sums).detach().double().cpu()
        nk = max(float(s[4]), 1.0)
        out = {n: float(s[i]) / nk for i, n in enumerate(self.NAMES)}
        out["count_seq_mesh"] = float(s[4])
        if float(s[7]) > 0:           # the scene numbers exist only when a batch had a scene
            out["CONTACT_RATIO"], out["SCENE_DIST"] = float(s[5]) / float(s[7]), float(s[6]) / float(s[7])
            nb = max(float(s[10]), 1.0)
            out["CONTACT_RATIO_REF"], out["SCENE_DIST_REF"] = float(s[8]) / nb, float(s[9]) / nb
        return out


class CollisionMetrics:
    """Running sums of the collision keys, one float64 device vector of six entries (reduced over ranks like the other accumulators):
    [sum COLLISION_RATIO, sum COLLISION_FRAMES, (b,k) pairs, sum COLLISION_RATIO_REF, sum COLLISION_FRAMES_REF, sequences].  The numbers
    run over all hypotheses and all sequences, as CONTACT_RATIO does."""

    NAMES = ("COLLISION_RATIO", "COLLISION_FRAMES", "COLLISION_RATIO_REF", "COLLISION_FRAMES_REF")

    def __init__(self):
        self.reset()

    def reset(self):
        self._sums = None

    def update(self, cm: Dict[str, torch.Tensor]):
        """cm: ``rs['collision_metrics']`` of ``MLD.ego_eval``."""
        dev = cm["COLLISION_RATIO"].device
        cnt = lambda t: torch.tensor(float(t.numel()), dtype=torch.float64, device=dev)
        vals = torch.stack([cm["COLLISION_RATIO"].double().sum(), cm["COLLISION_FRAMES"].double().sum(), cnt(cm["COLLISION_RATIO"]),
                            cm["COLLISION_RATIO_REF"].double().sum(), cm["COLLISION_FRAMES_REF"].double().sum(),
                            cnt(cm["COLLISION_RATIO_REF"])])
        self._sums = vals if self._sums is None else self._sums + vals

    def sums(self):
        return torch.zeros(6, dtype=torch.float64) if self._sums is None else self._sums

    def compute(self, sums=None):
        s = (self.sums() if sums is None else sums).detach().double().cpu()
        if float(s[2]) <= 0:
            return {}
        nb = max(float(s[5]), 1.0)
        return {"COLLISION_RATIO": float(s[0]) / float(s[2]), "COLLISION_FRAMES": float(s[1]) / float(s[2]),
                "COLLISION_RATIO_REF": float(s[3]) / nb, "COLLISION_FRAMES_REF": float(s[4]) / nb}
