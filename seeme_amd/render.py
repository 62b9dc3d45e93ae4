"""Meshes and point clouds to pixels: the step from a predicted recording to something one can look at.

``render_hip`` / ``shade_hip``      ``seeme_render`` / ``seeme_render_shade`` (csrc/render.hip): per pixel the id and the inverse depth of
                                   the nearest primitive, then a flat-shaded RGB image.  fp32 on the ROCm device, no fallback.
``render_torch`` / ``shade_torch``  the plain-torch twins, any device.  After the vertex stage the definition (include/seeme_hip.h,
                                   DESIGN 5.9) is integer arithmetic, so ids, inv_depth and dropped agree bit for bit with the kernels;
                                   the twin shades in float64, the kernel in fp32 (a channel can differ by one on a rounding boundary).
``look_at`` / ``orbit_camera`` / ``intrinsics``   world -> camera maps in the OpenCV convention (x right, y down, z forward).
``write_png``                      8-bit RGB PNG with zlib and struct alone.
``uv_sphere``                      a closed test mesh; ``uv_sphere(84, 82)`` has SMPL's 6890 vertices and 13 776 faces.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import zlib
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

SUB = 16                     # SEEME_RENDER_SUB
COORD_MAX = 1 << 18          # SEEME_RENDER_COORD_MAX
Q_ONE = 1 << 22              # SEEME_RENDER_Q
SIZE_MAX = 4096              # SEEME_RENDER_SIZE_MAX
POINT_MAX = 8                # SEEME_RENDER_POINT_MAX
FRAMES_MAX = 65535           # frames of one launch (the grid's y)
NV_MAX = 1 << 24
PRIM_MAX = (1 << 31) - 2
_ID_MASK = 0xFFFFFFFF
_TWIN_BUDGET = 1 << 20       # box pixels of one pass of the twin: its temporaries are a few int64 arrays of this size


# ----------------------------------------------------------------------------- preconditions
def _check_scene(who: str, verts, faces, cams, intrinsics, size, points, near, point_size):
    """The preconditions of the definition, on the host before any launch -> (F, NV, NF, P, FC, H, W, (fx, fy, cx, cy, near) as
    float32-exact Python floats, point_size).  Tensors are not moved or converted here."""
    for name, t, tail in (("verts", verts, "[F,NV,3]"), ("cams", cams, "[FC,4,4]")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3:
            what = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{who}: {name} is {what}: expected a float32 tensor {tail}")
    if verts.shape[2] != 3:
        raise ValueError(f"{who}: verts are {tuple(verts.shape)}: expected [F,NV,3]")
    F, NV = int(verts.shape[0]), int(verts.shape[1])
    if not 1 <= F <= FRAMES_MAX:
        raise ValueError(f"{who}: verts hold F = {F} frames: F must be in 1..{FRAMES_MAX} per call")
    if NV > NV_MAX:
        raise ValueError(f"{who}: verts hold NV = {NV} vertices per frame: at most 2^24")
    if tuple(cams.shape[1:]) != (4, 4) or cams.shape[0] not in (1, F):
        raise ValueError(f"{who}: cams are {tuple(cams.shape)}: expected [1,4,4] or [{F},4,4] (F = {F})")
    if not isinstance(faces, torch.Tensor) or faces.dtype not in (torch.int32, torch.int64) or faces.dim() != 2 or faces.shape[1] != 3:
        what = f"{tuple(faces.shape)} {faces.dtype}" if isinstance(faces, torch.Tensor) else type(faces).__name__
        raise ValueError(f"{who}: faces are {what}: expected an int32 or int64 tensor [NF,3]")
    NF = int(faces.shape[0])
    if NF and NV < 1:
        raise ValueError(f"{who}: faces without vertices (NV = 0)")
    if NF:
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= NV:
            raise ValueError(f"{who}: faces hold the index {lo if lo < 0 else hi}: outside 0..{NV - 1} (NV = {NV})")
    P = 0
    if points is not None:
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
            what = f"{tuple(points.shape)} {points.dtype}" if isinstance(points, torch.Tensor) else type(points).__name__
            raise ValueError(f"{who}: points are {what}: expected a float32 tensor [P,3]")
        P = int(points.shape[0])
    if NF + P > PRIM_MAX:
        raise ValueError(f"{who}: NF + P is {NF + P}: at most 2^31 - 2")
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: size is {size!r}: expected (H, W)") from None
    if not (1 <= H <= SIZE_MAX and 1 <= W <= SIZE_MAX):
        raise ValueError(f"{who}: size is {H} x {W}: H and W must be in 1..{SIZE_MAX}")
    try:
        k = [float(np.float32(v)) for v in intrinsics]
    except (TypeError, ValueError):
        k = []
    if len(k) != 4 or not all(math.isfinite(v) for v in k):
        raise ValueError(f"{who}: intrinsics are {intrinsics!r}: expected four finite numbers fx, fy, cx, cy")
    near32 = float(np.float32(near))
    if not (math.isfinite(near32) and near32 > 0.0):
        raise ValueError(f"{who}: near is {near!r}: the near plane must be finite and > 0")
    if isinstance(point_size, bool) or not isinstance(point_size, (int, np.integer)) or not 1 <= int(point_size) <= POINT_MAX:
        raise ValueError(f"{who}: point_size is {point_size!r}: expected an integer in 1..{POINT_MAX}")
    return F, NV, NF, P, int(cams.shape[0]), H, W, tuple(k) + (near32,), int(point_size)


def _check_shade(who: str, ids, F, H, W, NF, P, mesh_of_face, palette, point_rgb, bg):
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or tuple(ids.shape) != (F, H, W):
        what = f"{tuple(ids.shape)} {ids.dtype}" if isinstance(ids, torch.Tensor) else type(ids).__name__
        raise ValueError(f"{who}: ids are {what}: expected an int32 tensor [{F},{H},{W}]")
    n_mesh = 0
    if NF:
        if not isinstance(palette, torch.Tensor) or palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or palette.shape[0] < 1:
            what = f"{tuple(palette.shape)} {palette.dtype}" if isinstance(palette, torch.Tensor) else type(palette).__name__
            raise ValueError(f"{who}: palette is {what}: expected a uint8 tensor [n_mesh,3], n_mesh >= 1")
        n_mesh = int(palette.shape[0])
        if not isinstance(mesh_of_face, torch.Tensor) or mesh_of_face.dtype not in (torch.int32, torch.int64) or tuple(mesh_of_face.shape) != (NF,):
            what = f"{tuple(mesh_of_face.shape)} {mesh_of_face.dtype}" if isinstance(mesh_of_face, torch.Tensor) else type(mesh_of_face).__name__
            raise ValueError(f"{who}: mesh_of_face is {what}: expected an integer tensor [{NF}]")
        lo, hi = int(mesh_of_face.min()), int(mesh_of_face.max())
        if lo < 0 or hi >= n_mesh:
            raise ValueError(f"{who}: mesh_of_face holds {lo if lo < 0 else hi}: outside 0..{n_mesh - 1}, the rows of palette")
    if P:
        if not isinstance(point_rgb, torch.Tensor) or point_rgb.dtype != torch.uint8 or tuple(point_rgb.shape) != (P, 3):
            what = f"{tuple(point_rgb.shape)} {point_rgb.dtype}" if isinstance(point_rgb, torch.Tensor) else type(point_rgb).__name__
            raise ValueError(f"{who}: point_rgb is {what}: expected a uint8 tensor [{P},3], one colour per point")
    try:
        bg = tuple(int(v) for v in bg)
    except (TypeError, ValueError):
        bg = ()
    if len(bg) != 3 or not all(0 <= v <= 255 for v in bg):
        raise ValueError(f"{who}: bg is {bg!r}: expected three integers in 0..255")
    return n_mesh, bg


# ----------------------------------------------------------------------------- the twin
def _vertex_stage(p, M, k):
    """p [F or 1,N,3] float32, M [FC,4,4] float32, k = (fx, fy, cx, cy, near) -> X, Y, Q int64 and ok bool, [max(F, FC) or 1, N]:
    the vertex stage of the definition in float64, one torch op per product, sum and quotient (nothing is contracted)."""
    fx, fy, cx, cy, near = k
    p, M = p.double(), M.double()
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    row = lambda r: ((M[:, r, 0, None] * x + M[:, r, 1, None] * y) + M[:, r, 2, None] * z) + M[:, r, 3, None]
    xc, yc, zc = row(0), row(1), row(2)
    ok = torch.isfinite(zc) & (zc >= near)
    X = torch.round(((fx * xc) / zc + cx) * 16.0)
    Y = torch.round(((fy * yc) / zc + cy) * 16.0)
    ok = ok & (X.abs() <= COORD_MAX) & (Y.abs() <= COORD_MAX)               # (NaN and inf fail the comparison)
    Q = torch.round((near / zc) * float(Q_ONE))
    zero = torch.zeros_like(X)
    as_int = lambda v: torch.where(ok, v, zero).long()
    return as_int(X), as_int(Y), as_int(Q), ok


def _edge(ux, uy, vx, vy, px, py):
    return (vx - ux) * (py - uy) - (vy - uy) * (px - ux)


def _owned(w, dx, dy):
    return (w > 0) | ((w == 0) & ((dy > 0) | ((dy == 0) & (dx < 0))))


def _raster_frame(keys, H: int, W: int, X, Y, Q, ok, faces) -> int:
    """The faces of one frame into keys [H*W] int64 (a key is below 2^55, so the signed maximum is the unsigned one) -> dropped."""
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    good = ok[a] & ok[b] & ok[c]
    dropped = int((~good).sum())
    ax, ay, aq = X[a], Y[a], Q[a]
    bx, by, bq = X[b], Y[b], Q[b]
    cx, cy, cq = X[c], Y[c], Q[c]
    area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    sw = area2 < 0
    bx, cx = torch.where(sw, cx, bx), torch.where(sw, bx, cx)
    by, cy = torch.where(sw, cy, by), torch.where(sw, by, cy)
    bq, cq = torch.where(sw, cq, bq), torch.where(sw, bq, cq)
    area2 = area2.abs()
    j0 = ((torch.minimum(ax, torch.minimum(bx, cx)) + 15) >> 4).clamp(min=0)
    i0 = ((torch.minimum(ay, torch.minimum(by, cy)) + 15) >> 4).clamp(min=0)
    j1 = (torch.maximum(ax, torch.maximum(bx, cx)) >> 4).clamp(max=W - 1)
    i1 = (torch.maximum(ay, torch.maximum(by, cy)) >> 4).clamp(max=H - 1)
    keep = torch.nonzero(good & (area2 != 0) & (j0 <= j1) & (i0 <= i1)).flatten()
    if keep.numel() == 0:
        return dropped
    side = torch.maximum(j1 - j0, i1 - i0)[keep] + 1
    side, order = torch.sort(side, stable=True)
    keep = keep[order]
    side_l = side.tolist()
    n, lo = len(side_l), 0
    while lo < n:                                                          # faces of similar box size share one pass
        a, b = lo + 1, n                                                   # the largest hi with (hi - lo) side[hi-1]^2 in the budget:
        while a < b:                                                       # sides ascend, so the cost ascends with hi
            mid = (a + b + 1) // 2
            if (mid - lo) * side_l[mid - 1] ** 2 <= _TWIN_BUDGET:
                a = mid
            else:
                b = mid - 1
        hi = a
        sel = keep[lo:hi]
        m = side_l[hi - 1]
        d = torch.arange(m, device=keys.device)
        g = lambda v: v[sel][:, None, None]
        jj, ii = g(j0) + d[None, None, :], g(i0) + d[None, :, None]
        px, py = 16 * jj, 16 * ii
        Ax, Ay, Bx, By, Cx, Cy = g(ax), g(ay), g(bx), g(by), g(cx), g(cy)
        w0, w1, w2 = _edge(Bx, By, Cx, Cy, px, py), _edge(Cx, Cy, Ax, Ay, px, py), _edge(Ax, Ay, Bx, By, px, py)
        cover = (jj <= g(j1)) & (ii <= g(i1)) & _owned(w0, Cx - Bx, Cy - By) & _owned(w1, Ax - Cx, Ay - Cy) & _owned(w2, Bx - Ax, By - Ay)
        q = torch.div(w0 * g(aq) + w1 * g(bq) + w2 * g(cq), g(area2), rounding_mode="floor")
        key = (q << 32) | (_ID_MASK - sel)[:, None, None]
        at = (ii * W + jj).expand_as(cover)[cover]
        keys.scatter_reduce_(0, at, key.expand_as(cover)[cover], "amax", include_self=True)
        lo = hi
    return dropped


def _splat_frame(keys, H: int, W: int, X, Y, Q, ok, NF: int, s: int) -> None:
    j, i = (X + 8) >> 4, (Y + 8) >> 4
    key = (Q << 32) | (_ID_MASK - (NF + torch.arange(X.shape[0], device=keys.device)))
    for dy in range(-((s - 1) // 2), s // 2 + 1):
        for dx in range(-((s - 1) // 2), s // 2 + 1):
            r, c = i + dy, j + dx
            m = ok & (r >= 0) & (r < H) & (c >= 0) & (c < W)
            keys.scatter_reduce_(0, (r * W + c)[m], key[m], "amax", include_self=True)


def render_torch(verts, faces, cams, intrinsics, size, points=None, near: float = 0.05, point_size: int = 1) -> Dict[str, torch.Tensor]:
    """verts [F,NV,3] float32 (any device), faces [NF,3] integers, cams [1 or F,4,4] float32 world -> camera, intrinsics = (fx, fy, cx,
    cy), size = (H, W), points [P,3] float32 or None -> ids [F,H,W] int32 (-1 empty; a point is NF + p), inv_depth [F,H,W] int32
    (depth in metres = near * 2^22 / q) and dropped [F] int32: the definition of ``seeme_render`` in integer torch ops, frame by
    frame, the faces of a frame in passes of similar box size."""
    F, NV, NF, P, FC, H, W, k, s = _check_scene("render_torch", verts, faces, cams, intrinsics, size, points, near, point_size)
    dev = verts.device
    faces = faces.to(dev).long()
    cams = cams.to(dev)
    ids = torch.empty(F, H, W, dtype=torch.int32, device=dev)
    inv = torch.empty(F, H, W, dtype=torch.int32, device=dev)
    dropped = torch.zeros(F, dtype=torch.int32, device=dev)
    for f in range(F):
        M = cams[f if FC > 1 else 0][None]
        keys = torch.zeros(H * W, dtype=torch.int64, device=dev)
        if NF:
            X, Y, Q, ok = (t[0] for t in _vertex_stage(verts[f][None], M, k))
            dropped[f] = _raster_frame(keys, H, W, X, Y, Q, ok, faces)
        if P:
            X, Y, Q, ok = (t[0] for t in _vertex_stage(points.to(dev)[None], M, k))
            _splat_frame(keys, H, W, X, Y, Q, ok, NF, s)
        ids[f] = torch.where(keys == 0, torch.full_like(keys, -1), _ID_MASK - (keys & _ID_MASK)).view(H, W).to(torch.int32)
        inv[f] = (keys >> 32).view(H, W).to(torch.int32)
    return {"ids": ids, "inv_depth": inv, "dropped": dropped}


def shade_torch(verts, faces, cams, ids, mesh_of_face=None, palette=None, points=None, point_rgb=None, bg=(0, 0, 0)) -> torch.Tensor:
    """ids [F,H,W] of ``render_torch`` / ``render_hip`` for the same scene -> rgb [F,H,W,3] uint8, in float64: an empty pixel is bg, a
    point pixel point_rgb[p], a face pixel floor(palette[mesh_of_face[id]] * (0.3 + 0.7 |n_z| / |n|) + 0.5), n the normal of the
    un-snapped camera-space corners."""
    H, W = (int(v) for v in ids.shape[1:]) if isinstance(ids, torch.Tensor) and ids.dim() == 3 else (1, 1)
    F, NV, NF, P, FC, H, W, _, _ = _check_scene("shade_torch", verts, faces, cams, (1.0, 1.0, 0.0, 0.0), (H, W), points, 1.0, 1)
    n_mesh, bg = _check_shade("shade_torch", ids, F, H, W, NF, P, mesh_of_face, palette, point_rgb, bg)
    dev = verts.device
    rgb = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    rgb[:] = torch.tensor(bg, dtype=torch.uint8, device=dev)
    idl = ids.to(dev).long()
    if P:
        at = (idl >= NF) & (idl < NF + P)
        rgb[at] = point_rgb.to(dev)[idl[at] - NF]
    if NF:
        faces = faces.to(dev).long()
        for f in range(F):
            at = (idl[f] >= 0) & (idl[f] < NF)
            fid = idl[f][at]
            M = cams.to(dev)[f if FC > 1 else 0].double()
            v = verts[f].double()
            x, y, z = v[:, 0], v[:, 1], v[:, 2]
            cam = torch.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], dim=1)      # [NV,3]
            A, B, Cc = (cam[faces[fid, q]] for q in range(3))
            n = torch.linalg.cross(B - A, Cc - A)
            ln = n.norm(dim=1)
            ratio = torch.where(ln > 0, n[:, 2].abs() / ln.clamp(min=1e-300), torch.zeros_like(ln))
            base = palette.to(dev)[mesh_of_face.to(dev).long()[fid]].double()
            rgb[f][at] = torch.floor(base * (0.3 + 0.7 * ratio)[:, None] + 0.5).clamp(max=255).to(torch.uint8)
    return rgb


# ----------------------------------------------------------------------------- the kernels
_WS = L.Workspace(per_stream=True)


def _scene_struct(verts, faces, points, cams, F, NV, NF, P, FC, H, W, k, s) -> L.RenderScene:
    sc = L.RenderScene()
    sc.verts, sc.faces, sc.points, sc.cams = L.ptr(verts if NF else None), L.ptr(faces if NF else None), L.ptr(points if P else None), cams.data_ptr()
    sc.F, sc.NV, sc.NF, sc.P, sc.FC, sc.H, sc.W, sc.point_size = F, NV, NF, P, FC, H, W, s
    sc.fx, sc.fy, sc.cx, sc.cy, sc.znear = k
    return sc


def _on_device(who: str, **tensors):
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise L.SeemeError(f"{who}: {name} must be a tensor on the ROCm device (cuda:N); this path has no CPU fallback "
                               f"({who.replace('_hip', '_torch')} is the twin for any device)")
        if dev is not None and t.device != dev:
            raise L.SeemeError(f"{who}: {name} is on {t.device}, the tensors before it on {dev}")
        dev = t.device
    return dev


def render_hip(verts, faces, cams, intrinsics, size, points=None, near: float = 0.05, point_size: int = 1,
               chunk_mb: float = 256.0) -> Dict[str, torch.Tensor]:
    """``render_torch`` on the ROCm device through ``seeme_render``: the same arguments (all tensors on the device) and the same three
    results.  The frames go in chunks whose workspace (8 bytes per pixel and 16 per vertex, per frame) stays under `chunk_mb` MiB; the
    result does not depend on the chunking.  Launches on the current stream; only the face table's range check synchronises."""
    dev = _on_device("render_hip", verts=verts, faces=faces, cams=cams, points=points)
    F, NV, NF, P, FC, H, W, k, s = _check_scene("render_hip", verts, faces, cams, intrinsics, size, points, near, point_size)
    if not (isinstance(chunk_mb, (int, float)) and not isinstance(chunk_mb, bool) and chunk_mb > 0):
        raise ValueError(f"render_hip: chunk_mb is {chunk_mb!r}: expected a positive number of MiB")
    verts, cams = verts.contiguous(), cams.contiguous()
    faces = faces.to(torch.int32).contiguous()
    points = points.contiguous() if P else None
    ids = torch.empty(F, H, W, dtype=torch.int32, device=dev)
    inv = torch.empty(F, H, W, dtype=torch.int32, device=dev)
    dropped = torch.empty(F, dtype=torch.int32, device=dev)
    per_frame = H * W * 8 + NV * 16
    step = max(1, min(F, int(chunk_mb * (1 << 20)) // per_frame))
    with torch.cuda.device(dev):
        for lo in range(0, F, step):
            n = min(step, F - lo)
            _launch_render(verts[lo:lo + n], faces, points, cams[lo:lo + n] if FC > 1 else cams, n, NV, NF, P, FC if FC == 1 else n,
                           H, W, k, s, ids[lo:lo + n], inv[lo:lo + n], dropped[lo:lo + n])
    return {"ids": ids, "inv_depth": inv, "dropped": dropped}


def _launch_render(verts, faces, points, cams, F, NV, NF, P, FC, H, W, k, s, ids, inv, dropped, ws=None, ws_bytes=None) -> None:
    """The C entry as it is.  ws / ws_bytes: another workspace and the size to state for it (the tests' refusals)."""
    need = int(L.lib().seeme_render_workspace_bytes(F, NV, H, W))
    if ws is None:
        ws = _WS.get(need, verts.device)
    sc = _scene_struct(verts, faces, points, cams, F, NV, NF, P, FC, H, W, k, s)
    L.call("seeme_render", C.byref(sc), ids.data_ptr(), inv.data_ptr(), dropped.data_ptr(), ws.data_ptr(),
           need if ws_bytes is None else ws_bytes, L.current_stream())


def shade_hip(verts, faces, cams, ids, mesh_of_face=None, palette=None, points=None, point_rgb=None, bg=(0, 0, 0)) -> torch.Tensor:
    """``shade_torch`` on the ROCm device through ``seeme_render_shade`` (fp32): one launch on the current stream."""
    dev = _on_device("shade_hip", verts=verts, faces=faces, cams=cams, ids=ids, mesh_of_face=mesh_of_face, palette=palette,
                     points=points, point_rgb=point_rgb)
    H, W = (int(v) for v in ids.shape[1:]) if ids.dim() == 3 else (1, 1)
    F, NV, NF, P, FC, H, W, k, s = _check_scene("shade_hip", verts, faces, cams, (1.0, 1.0, 0.0, 0.0), (H, W), points, 1.0, 1)
    n_mesh, bg = _check_shade("shade_hip", ids, F, H, W, NF, P, mesh_of_face, palette, point_rgb, bg)
    verts, cams, ids = verts.contiguous(), cams.contiguous(), ids.contiguous()
    faces = faces.to(torch.int32).contiguous()
    mof = mesh_of_face.to(torch.int32).contiguous() if NF else None
    pal = palette.contiguous() if NF else None
    prgb = point_rgb.contiguous() if P else None
    rgb = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    sc = _scene_struct(verts, faces, points.contiguous() if P else None, cams, F, NV, NF, P, FC, H, W, k, s)
    with torch.cuda.device(dev):
        L.call("seeme_render_shade", C.byref(sc), ids.data_ptr(), L.ptr(mof), L.ptr(pal), n_mesh, L.ptr(prgb),
               bg[0] | bg[1] << 8 | bg[2] << 16, rgb.data_ptr(), L.current_stream())
    return rgb


# ----------------------------------------------------------------------------- cameras
def _unit(v, what: str) -> np.ndarray:
    v = np.asarray(v, np.float64).reshape(-1)
    n = float(np.linalg.norm(v)) if v.shape == (3,) and np.isfinite(v).all() else 0.0
    if n < 1e-12:
        raise ValueError(f"{what} is {v.tolist()}: expected a finite, non-zero 3-vector")
    return v / n


def look_at(eye, target, up) -> np.ndarray:
    """The rigid world -> camera map [4,4] float64 of a camera at `eye` whose optical axis (+z) passes through `target`, image x to the
    right and image y DOWN (the OpenCV convention), `up` pointing up in the image."""
    eye, target = np.asarray(eye, np.float64).reshape(-1), np.asarray(target, np.float64).reshape(-1)
    if eye.shape != (3,) or target.shape != (3,) or not (np.isfinite(eye).all() and np.isfinite(target).all()):
        raise ValueError(f"look_at: eye is {eye.tolist()}, target is {target.tolist()}: expected two finite 3-vectors")
    z = _unit(target - eye, "look_at: target - eye")
    x = np.cross(z, _unit(up, "look_at: up"))
    if np.linalg.norm(x) < 1e-9:
        raise ValueError("look_at: up is parallel to the viewing direction")
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[:3, :3] = np.stack([x, y, z])
    M[:3, 3] = -M[:3, :3] @ eye
    return M


def intrinsics(fov: float, size) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) of a pinhole camera with square pixels whose WIDTH spans `fov` degrees; the principal point is the middle of
    the image in the pixel-centre convention, ((W-1)/2, (H-1)/2)."""
    H, W = (int(v) for v in size)
    if not 0.0 < float(fov) < 180.0:
        raise ValueError(f"intrinsics: fov is {fov!r}: expected degrees in (0, 180)")
    f = 0.5 * W / math.tan(math.radians(float(fov)) / 2)
    return f, f, 0.5 * (W - 1), 0.5 * (H - 1)


def orbit_camera(points, azimuth: float = 30.0, elevation: float = 20.0, fov: float = 60.0, up=(0.0, 0.0, 1.0), aspect: float = 4 / 3,
                 margin: float = 1.1) -> np.ndarray:
    """One fixed world -> camera map [4,4] that looks at the middle of `points` [...,3] from `azimuth` degrees around `up` and
    `elevation` degrees above the plane across it (|elevation| < 90), far enough for the sphere around all points to fit a view whose
    width spans `fov` degrees at the aspect ratio W / H (``intrinsics``), with `margin` to spare."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if p.shape[0] < 1:
        raise ValueError("orbit_camera: no finite point to look at")
    if not abs(float(elevation)) < 90.0:
        raise ValueError(f"orbit_camera: elevation is {elevation!r}: expected degrees in (-90, 90)")
    if not 0.0 < float(fov) < 180.0:
        raise ValueError(f"orbit_camera: fov is {fov!r}: expected degrees in (0, 180)")
    if not (aspect > 0 and margin >= 1.0):
        raise ValueError(f"orbit_camera: aspect is {aspect!r}, margin is {margin!r}: expected aspect > 0 and margin >= 1")
    u = _unit(up, "orbit_camera: up")
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    radius = max(float(np.linalg.norm(p - centre, axis=1).max()), 1e-6)
    axis = np.eye(3)[int(np.argmin(np.abs(u)))]                              # the frame around up: e1, e2 = up x e1
    e1 = axis - (axis @ u) * u
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    az, el = math.radians(float(azimuth)), math.radians(float(elevation))
    d = math.cos(el) * (math.cos(az) * e1 + math.sin(az) * e2) + math.sin(el) * u
    half_w = math.radians(float(fov)) / 2
    half = min(half_w, math.atan(math.tan(half_w) / float(aspect)))          # the narrower of the two half angles
    return look_at(centre + (float(margin) * radius / math.sin(half)) * d, centre, u)


# ----------------------------------------------------------------------------- files and test meshes
def write_png(path: str, rgb) -> None:
    """rgb uint8 [H,W,3] -> an 8-bit truecolour PNG (filter 0 on every row, one IDAT chunk)."""
    a = np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: rgb is {a.shape} {a.dtype}: expected uint8 [H,W,3]")
    H, W = a.shape[:2]
    rows = np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(a).reshape(H, W * 3)], axis=1).tobytes()
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows, 6)) + chunk(b"IEND", b""))


def uv_sphere(n_seg: int, n_ring: int, radius: float = 1.0, centre: Sequence[float] = (0.0, 0.0, 0.0)):
    """A closed sphere of n_ring latitude rings of n_seg vertices between two poles -> (verts float32 [n_seg n_ring + 2, 3], faces
    int64 [2 n_seg n_ring, 3]), consistently wound, the normals outward.  uv_sphere(84, 82): 6890 vertices, 13 776 faces."""
    if n_seg < 3 or n_ring < 1:
        raise ValueError(f"uv_sphere: n_seg is {n_seg}, n_ring is {n_ring}: expected n_seg >= 3 and n_ring >= 1")
    th = np.pi * np.arange(1, n_ring + 1) / (n_ring + 1)
    ph = 2 * np.pi * np.arange(n_seg) / n_seg
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None],
                     np.broadcast_to(np.cos(th)[:, None], (n_ring, n_seg))], axis=-1).reshape(-1, 3)
    verts = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]) * radius + np.asarray(centre, np.float64)
    at = lambda r, s: 1 + r * n_seg + s % n_seg
    south = 1 + n_ring * n_seg
    faces = []
    for s in range(n_seg):
        faces.append((0, at(0, s), at(0, s + 1)))
        for r in range(n_ring - 1):
            faces.append((at(r, s), at(r + 1, s), at(r + 1, s + 1)))
            faces.append((at(r, s), at(r + 1, s + 1), at(r, s + 1)))
        faces.append((south, at(n_ring - 1, s + 1), at(n_ring - 1, s)))
    return verts.astype(np.float32), np.asarray(faces, np.int64)


# ----------------------------------------------------------------------------- a predicted motion file
def load_motion(path: str, n_frames: int) -> Dict[str, np.ndarray]:
    """The ``.npz`` that ``predict.py`` writes, for a recording of `n_frames` frames: global_orient [L,3], body_pose [L,69|63] and
    transl [L,3] of the wearer in the recording's world frame, float32.  A missing key or another shape is a ValueError that names
    the key."""
    want = {"global_orient": [(n_frames, 3)], "body_pose": [(n_frames, 69), (n_frames, 63)], "transl": [(n_frames, 3)]}
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in want if k not in z.files]
        if missing:
            raise ValueError(f"{path}: missing {missing}; a motion file holds {list(want)} of the wearer (predict.py writes them)")
        mot = {k: np.asarray(z[k], np.float32) for k in want}
    for k, shapes in want.items():
        if mot[k].shape not in shapes:
            raise ValueError(f"{path}: {k} is {mot[k].shape}: expected {' or '.join(str(list(s)) for s in shapes)} "
                             f"(the recording has L = {n_frames} frames)")
        if not np.isfinite(mot[k]).all():
            raise ValueError(f"{path}: {k} holds a value that is not finite")
    return mot


def height_colours(points: np.ndarray, up, low=(70, 80, 120), high=(225, 215, 175)) -> np.ndarray:
    """points [P,3] -> uint8 [P,3]: a linear blend from `low` to `high` by the height along `up` between the cloud's lowest and
    highest point."""
    h = np.asarray(points, np.float64) @ _unit(up, "height_colours: up")
    span = float(h.max() - h.min()) if h.size else 0.0
    t = (h - h.min()) / span if span > 0 else np.zeros_like(h)
    lo, hi = np.asarray(low, np.float64), np.asarray(high, np.float64)
    return np.floor(lo + t[:, None] * (hi - lo) + 0.5).clip(0, 255).astype(np.uint8)
