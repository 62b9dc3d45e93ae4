"""Rotation-representation helpers with the signatures of ``mld/utils/geometry2.py`` (:33-117) and the
dataset ``renorm`` (mld/data/EgoBody.py:151-157), running in libseeme_hip.so."""
from __future__ import annotations

import torch

from . import _lib as L


def _run(op: int, x: torch.Tensor, in_w: int, out_shape):
    L.require_cuda(x, "input")
    x2 = x.reshape(-1, in_w).contiguous()
    M = x2.shape[0]
    out = torch.empty((M,) + out_shape, device=x.device, dtype=torch.float32)
    L.call("seeme_geometry", op, x2.data_ptr(), out.data_ptr(), M, L.current_stream())
    return out


def aa_to_quat(theta: torch.Tensor) -> torch.Tensor:
    """[M,3] axis-angle -> [M,4] quaternion (w,x,y,z)."""
    return _run(L.GEO_AA_TO_QUAT, theta, 3, (4,))


def aa_to_rotmat(theta: torch.Tensor) -> torch.Tensor:
    return _run(L.GEO_AA_TO_ROTMAT, theta, 3, (3, 3))


def quat_to_rotmat(quat: torch.Tensor) -> torch.Tensor:
    return _run(L.GEO_QUAT_TO_ROTMAT, quat, 4, (3, 3))


def rot6d_to_rotmat(x: torch.Tensor, rot6d_mode: str = "prohmr") -> torch.Tensor:
    if rot6d_mode not in ("prohmr", "diffusion"):
        raise ValueError(rot6d_mode)
    return _run(L.GEO_ROT6D_PROHMR if rot6d_mode == "prohmr" else L.GEO_ROT6D_DIFFUSION, x, 6, (3, 3))


def _renorm_launch(f2: torch.Tensor, m: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(f2)
    L.call("seeme_renorm", f2.data_ptr(), m.data_ptr(), s.data_ptr(), out.data_ptr(), f2.shape[0], f2.shape[1], L.current_stream())
    return out


class _Renorm(torch.autograd.Function):
    """y = x * std + mean through k_renorm; dL/dx = dL/dy * std is the same kernel with a zero mean (stage-1 training
    differentiates through the renormed reconstruction, mld.py:757-778)."""

    @staticmethod
    def forward(ctx, f2, m, s):
        ctx.save_for_backward(s)
        return _renorm_launch(f2, m, s)

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return _renorm_launch(g.contiguous().float(), torch.zeros_like(s), s), None, None


def renorm(features: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """features [..., F] * std[..., :F] + mean[..., :F]."""
    L.require_cuda(features, "features")
    F = features.shape[-1]
    f2 = features.reshape(-1, F).contiguous()
    m = mean.reshape(-1)[:F].to(features.device, torch.float32).contiguous()
    s = std.reshape(-1)[:F].to(features.device, torch.float32).contiguous()
    out = _Renorm.apply(f2, m, s) if (f2.requires_grad and torch.is_grad_enabled()) else _renorm_launch(f2, m, s)
    return out.reshape(features.shape)


def rotmat_to_rot6d(R: torch.Tensor, mode: str = "diffusion") -> torch.Tensor:
    """[..., 3, 3] rotation matrices -> [M, 6]: the first two columns (utils_egobody/geometry.py:256-262).  'diffusion' (the
    dataset's default): ``R[:, :, :2].reshape(-1, 6)`` = [r00, r01, r10, r11, r20, r21]; 'prohmr': the two columns one after the
    other, [r00, r10, r20, r01, r11, r21] -- the order ``rot6d_to_rotmat`` reads under the same name.  Pure indexing, any device."""
    if mode not in ("prohmr", "diffusion"):
        raise ValueError(mode)
    R = R.reshape(-1, 3, 3)
    if mode == "diffusion":
        return R[:, :, :2].reshape(-1, 6)
    return R[:, :, :2].permute(0, 2, 1).reshape(-1, 6)


def aa_to_rotmat_torch(theta: torch.Tensor) -> torch.Tensor:
    """``aa_to_rotmat`` in plain torch (any device and dtype; the data module's conversion on the CPU): axis-angle [M,3] ->
    quaternion with the half angle of ||theta + 1e-8|| -> [M,3,3], the formulas of the kernel (geometry2.py:33-95)."""
    theta = theta.reshape(-1, 3)
    ang = torch.norm(theta + 1e-8, dim=1, keepdim=True)
    q = torch.cat([torch.cos(0.5 * ang), torch.sin(0.5 * ang) * (theta / ang)], dim=1)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                        2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], dim=1).view(-1, 3, 3)


def rotmat_to_quat_torch(R: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] rotation matrices -> [..., 4] unit quaternions (w,x,y,z), plain torch (any device and dtype): the largest of
    w, x, y, z is taken first (Shepperd), so no branch divides by a small number.  The sign is whatever that branch gives."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = R.reshape(*R.shape[:-2], 9).unbind(-1)
    root = lambda v: torch.sqrt(v.clamp_min(1e-30)) * 2.0                      # (only the selected branch's value is used)
    tr = m00 + m11 + m22
    s0, s1, s2, s3 = root(tr + 1.0), root(1.0 + m00 - m11 - m22), root(1.0 + m11 - m00 - m22), root(1.0 + m22 - m00 - m11)
    q0 = torch.stack([0.25 * s0, (m21 - m12) / s0, (m02 - m20) / s0, (m10 - m01) / s0], dim=-1)
    q1 = torch.stack([(m21 - m12) / s1, 0.25 * s1, (m01 + m10) / s1, (m02 + m20) / s1], dim=-1)
    q2 = torch.stack([(m02 - m20) / s2, (m01 + m10) / s2, 0.25 * s2, (m12 + m21) / s2], dim=-1)
    q3 = torch.stack([(m10 - m01) / s3, (m02 + m20) / s3, (m12 + m21) / s3, 0.25 * s3], dim=-1)
    c0, c1, c2 = (tr > 0)[..., None], ((m00 > m11) & (m00 > m22))[..., None], (m11 > m22)[..., None]
    q = torch.where(c0, q0, torch.where(c1, q1, torch.where(c2, q2, q3)))
    return q / q.norm(dim=-1, keepdim=True)


def quat_to_aa_torch(q: torch.Tensor) -> torch.Tensor:
    """[..., 4] unit quaternions -> [..., 3] axis-angle with an angle in [0, pi] (q and -q give the same result)."""
    q = torch.where(q[..., :1] < 0, -q, q)
    v = q[..., 1:]
    vn = v.norm(dim=-1, keepdim=True)
    k = torch.where(vn > 1e-12, 2.0 * torch.atan2(vn, q[..., :1]) / vn.clamp_min(1e-12), torch.full_like(vn, 2.0))
    return k * v


def rotmat_to_aa_torch(R: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] rotation matrices -> [M, 3] axis-angle with an angle in [0, pi], plain torch (any device and dtype)."""
    return quat_to_aa_torch(rotmat_to_quat_torch(R.reshape(-1, 3, 3)))
