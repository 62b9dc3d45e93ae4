"""SMPLFlowHead -- drop-in for ``EgoHMR.models.prohmr.smpl_flow.SMPLFlow``, the pose head of ProHMR-scene: a conditional Glow over the
144 rot6d pose values (``nflows.flows.ConditionalGlow(144, 1024, 4, 2, context_features=2566)``, nflows/flows/glow.py:15-64) and
``FCHead`` (fc_head.py:19-52) for betas and the weak-perspective camera.  Same state-dict entries
(``flow._transform._transforms.{0..11}.*``, ``fc_head.layers.{0,2}.*``, ``fc_head.init_cam``, ``fc_head.init_betas``), so the
``proscene.flow.*`` entries of a SEE-ME checkpoint and the ``flow.*`` entries of a ProHMR-scene ``best_model.pt`` load strictly.

Only the sampling direction is built (``ProHMRScene.forward_step`` without its losses, prohmr_scene.py:108-233):

``flow_head_torch``   the plain-torch twin in the reference's unfolded order (BatchNorm applied, triangular solves, concatenated
                      context), any float dtype, any device: the oracle of everything folded.
``fold``              the host-side float64 preparation: BatchNorm as scale / offset, inv(L U) as one dense matrix, the ActNorm
                      inverse as scale / offset, the context columns of the five consumers stacked, the log|det| constant.
``flow_head_hip``     ``seeme_flow_head`` (csrc/flow_head.hip) on the folded weights, fp32, three launches on the current stream.

Always eval mode: BatchNorm uses its running statistics and dropout is off."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L

DIM = 144                  # MODEL.FLOW.DIM (EgoHMR/configs/prohmr.yaml:45-52)
HIDDEN = 1024              # MODEL.FLOW.LAYER_HIDDEN_FEATURES
LAYERS = 4                 # MODEL.FLOW.NUM_LAYERS
DEPTH = 2                  # MODEL.FLOW.LAYER_DEPTH: residual blocks per coupling net
HALF = DIM // 2
CTX_SCALARS = 6
IMAGE_DIM = 2048
SCENE_DIM = 512
CTX_DIM = CTX_SCALARS + IMAGE_DIM + SCENE_DIM          # 2566
CTX_PAD = 2576                                         # SEEME_FLOW_CTX_PAD: K of the context GEMM, a multiple of 16
ID_PAD = 80                                            # K of the initial layer's identity part
FC_FEATURES = 1024         # MODEL.FC_HEAD.NUM_FEATURES
FX_NORM_COEFF = 1500.0     # CAM.FX_NORM_COEFF (prohmr.yaml:56)
IMAGE_SIZE = 224           # MODEL.IMAGE_SIZE
LU_EPS = 1e-3              # LULinear(eps) (nflows/transforms/lu.py:13)
BN_EPS = 1e-5
S_MAX = 32                 # SEEME_FLOW_S_MAX
ROWS_MAX = 1 << 20         # SEEME_FLOW_ROWS_MAX
TILE_ROWS = 16             # rows of (frame, sample) per workgroup of k_flow_chain


# ----------------------------------------------------------------------------- the parameter holder
class _Transform(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("dummy_buffer", torch.tensor(1.0))        # nflows/transforms/base.py:27: every Transform carries one


class _ActNorm(_Transform):
    def __init__(self):
        super().__init__()
        self.register_buffer("initialized", torch.tensor(True, dtype=torch.bool))
        self.log_scale = nn.Parameter(torch.zeros(DIM))
        self.shift = nn.Parameter(torch.zeros(DIM))


class _LULinear(_Transform):
    def __init__(self):
        super().__init__()
        n = (DIM - 1) * DIM // 2
        self.bias = nn.Parameter(torch.zeros(DIM))
        self.lower_entries = nn.Parameter(torch.zeros(n))
        self.upper_entries = nn.Parameter(torch.zeros(n))
        self.unconstrained_upper_diag = nn.Parameter(torch.full((DIM,), math.log(math.exp(1 - LU_EPS) - 1)))


class _ResidualBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.batch_norm_layers = nn.ModuleList([nn.BatchNorm1d(HIDDEN) for _ in range(2)])
        self.linear_layers = nn.ModuleList([nn.Linear(HIDDEN, HIDDEN) for _ in range(2)])


class _ResidualNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.initial_layer = nn.Linear(HALF + CTX_DIM, HIDDEN)
        self.blocks = nn.ModuleList([_ResidualBlock() for _ in range(DEPTH)])
        self.final_layer = nn.Linear(HIDDEN, HALF)


class _Coupling(_Transform):
    def __init__(self, identity_odd: bool):
        super().__init__()
        idx = torch.arange(DIM)
        self.register_buffer("identity_features", idx[1::2].clone() if identity_odd else idx[0::2].clone())
        self.register_buffer("transform_features", idx[0::2].clone() if identity_odd else idx[1::2].clone())
        self.transform_net = _ResidualNet()


class _Composite(_Transform):
    def __init__(self):
        super().__init__()
        layers = []
        for k in range(LAYERS):                     # glow.py:36-59: mask[::2] = -1, flipped after every layer
            layers += [_ActNorm(), _LULinear(), _Coupling(identity_odd=k % 2 == 1)]
        self._transforms = nn.ModuleList(layers)


class _Flow(nn.Module):
    def __init__(self):
        super().__init__()
        self._transform = _Composite()
        self._distribution = nn.Module()            # StandardNormal: its only buffer (_log_z) is not persistent


class _FCHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(CTX_DIM, FC_FEATURES), nn.ReLU(), nn.Linear(FC_FEATURES, 13))
        self.register_buffer("init_cam", torch.tensor([[[0.9, 0.0, 0.0]]]))
        self.register_buffer("init_betas", torch.zeros(1, 1, 10))


def _fingerprint(module: nn.Module):
    return tuple((t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers()))


class SMPLFlowHead(nn.Module):
    """Parameter holder with the reference's names.  Frozen, always eval: ``train()`` does not reach the BatchNorms."""

    def __init__(self):
        super().__init__()
        self.flow = _Flow()
        self.fc_head = _FCHead()
        for p in self.parameters():
            p.requires_grad = False
        super().train(False)
        self._fold = None
        self._wcache = None
        self._ws = L.Workspace(per_stream=False)

    def train(self, mode: bool = True):
        return super().train(False)

    def layer(self, k: int):
        """(ActNorm, LULinear, coupling) of flow layer k."""
        t = self.flow._transform._transforms
        return t[3 * k], t[3 * k + 1], t[3 * k + 2]

    def forward(self, ctx: torch.Tensor, z: torch.Tensor):
        return flow_head_hip(self, ctx, z)


_STATE_SHAPES = None


def state_shapes() -> Dict[str, Tuple[int, ...]]:
    """{name: shape} of the reference SMPLFlow's state dict; built once, on the meta device (no storage is allocated)."""
    global _STATE_SHAPES
    if _STATE_SHAPES is None:
        with torch.device("meta"):
            _STATE_SHAPES = {k: tuple(v.shape) for k, v in SMPLFlowHead().state_dict().items()}
    return dict(_STATE_SHAPES)


# ----------------------------------------------------------------------------- small pieces shared by twin and tests
def lu_matrices(lu: _LULinear, dtype=torch.float64):
    """(lower, upper) of an LULinear (nflows/transforms/lu.py:44-54): unit lower triangle, softplus(diag) + eps on the upper."""
    dev = lu.bias.device
    lower = torch.eye(DIM, dtype=dtype, device=dev)
    upper = torch.zeros(DIM, DIM, dtype=dtype, device=dev)
    il, iu = np.tril_indices(DIM, k=-1), np.triu_indices(DIM, k=1)
    lower[il[0], il[1]] = lu.lower_entries.detach().to(dtype)
    upper[iu[0], iu[1]] = lu.upper_entries.detach().to(dtype)
    d = np.arange(DIM)
    upper[d, d] = F.softplus(lu.unconstrained_upper_diag.detach().to(dtype)) + LU_EPS
    return lower, upper


def rot6d_to_rotmat_torch(x: torch.Tensor) -> torch.Tensor:
    """[..., 6] -> [M,3,3], the 'prohmr' order of EgoHMR/utils/geometry.py:47-66 in plain torch (any device and dtype)."""
    x = x.reshape(-1, 2, 3).permute(0, 2, 1)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = F.normalize(a1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=1)), dim=-1)


def log_det_constant(head: SMPLFlowHead) -> float:
    """sum over layers of (sum log_scale + sum log diag U): log|det| of the forward transform, input-independent since the
    coupling is additive (flows/base.py:62-94 subtracts the inverse's log|det|, which is minus this)."""
    total = 0.0
    for k in range(LAYERS):
        act, lu, _ = head.layer(k)
        total += float(act.log_scale.detach().double().sum())
        total += float(torch.log(F.softplus(lu.unconstrained_upper_diag.detach().double()) + LU_EPS).sum())
    return total


LOG_Z = 0.5 * DIM * math.log(2 * math.pi)     # distributions/normal.py:18-21


def _check_inputs(ctx, z):
    if not torch.is_tensor(ctx) or ctx.dim() != 2 or ctx.shape[1] != CTX_DIM:
        raise ValueError(f"ctx is {tuple(ctx.shape) if torch.is_tensor(ctx) else type(ctx).__name__}: expected [L,{CTX_DIM}]")
    if not torch.is_tensor(z) or z.dim() != 3 or z.shape[0] != ctx.shape[0] or z.shape[2] != DIM:
        raise ValueError(f"z is {tuple(z.shape) if torch.is_tensor(z) else type(z).__name__}: expected [L={ctx.shape[0]},S,{DIM}]")
    L_, S = int(z.shape[0]), int(z.shape[1])
    if L_ < 1 or not 1 <= S <= S_MAX or L_ * S > ROWS_MAX:
        raise ValueError(f"flow head: L = {L_}, S = {S}: needs L >= 1, 1 <= S <= {S_MAX} and L * S <= {ROWS_MAX}")
    return L_, S


# ----------------------------------------------------------------------------- the twin
@torch.no_grad()
def flow_head_torch(head: SMPLFlowHead, ctx: torch.Tensor, z: torch.Tensor):
    """``SMPLFlow.forward(feats=ctx, z=z)`` (smpl_flow.py:65-120) for S >= 1 in plain torch, in the dtype and on the device of ``ctx``
    and in the reference's own order of operations -> pose6d [L,S,144], rotmat [L,S,24,3,3], betas [L,10], cam [L,3], log_prob [L,S]."""
    L_, S = _check_inputs(ctx, z)
    dt, dev = ctx.dtype, ctx.device
    p = lambda t: t.detach().to(device=dev, dtype=dt)
    x = z.to(device=dev, dtype=dt).reshape(L_ * S, DIM)
    c = ctx.repeat_interleave(S, dim=0)                                  # torchutils.repeat_rows
    log_prob = -0.5 * (x * x).sum(1) - LOG_Z
    logabsdet = torch.zeros((), dtype=dt, device=dev)
    for k in range(LAYERS - 1, -1, -1):                                  # CompositeTransform.inverse: last transform first
        act, lu, cp = head.layer(k)
        idf, tf = cp.identity_features.to(dev), cp.transform_features.to(dev)
        net = cp.transform_net
        t = F.linear(torch.cat((x[:, idf], c), dim=1), p(net.initial_layer.weight), p(net.initial_layer.bias))
        for blk in net.blocks:                                           # nn/nets/resnet.py:40-53, eval mode
            u = t
            for j in range(2):
                bn = blk.batch_norm_layers[j]
                u = F.batch_norm(u, p(bn.running_mean), p(bn.running_var), p(bn.weight), p(bn.bias), False, 0.0, bn.eps)
                u = F.linear(F.relu(u), p(blk.linear_layers[j].weight), p(blk.linear_layers[j].bias))
            t = t + u
        shift = F.linear(t, p(net.final_layer.weight), p(net.final_layer.bias))
        y = torch.empty_like(x)
        y[:, idf] = x[:, idf]
        y[:, tf] = x[:, tf] - shift                                      # AdditiveCouplingTransform inverse, scale 1
        lower, upper = lu_matrices(lu, dt)
        lower, upper = lower.to(dev), upper.to(dev)
        v = (y - p(lu.bias)).t()                                         # lu.py:70-91
        v = torch.linalg.solve_triangular(lower, v, upper=False, unitriangular=True)
        v = torch.linalg.solve_triangular(upper, v, upper=True)
        logabsdet = logabsdet - torch.log(torch.diagonal(upper)).sum()
        x = (v.t() - p(act.shift)) / torch.exp(p(act.log_scale))         # normalization.py:192-206
        logabsdet = logabsdet - p(act.log_scale).sum()
    log_prob = (log_prob - logabsdet).reshape(L_, S)
    pose6d = x.reshape(L_, S, DIM)
    rotmat = rot6d_to_rotmat_torch(x).reshape(L_, S, 24, 3, 3)
    fc = head.fc_head
    off = F.linear(F.relu(F.linear(ctx, p(fc.layers[0].weight), p(fc.layers[0].bias))), p(fc.layers[2].weight), p(fc.layers[2].bias))
    betas = off[:, :10] + p(fc.init_betas).reshape(1, 10)
    cam = off[:, 10:] + p(fc.init_cam).reshape(1, 3)
    return pose6d, rotmat, betas, cam, log_prob


# ----------------------------------------------------------------------------- the folds
@torch.no_grad()
def fold(head: SMPLFlowHead) -> Dict[str, object]:
    """The host-side float64 preparation of ``seeme_flow_head`` (the tensors of SeemeFlowHead, include/seeme_hip.h), cached under a
    fingerprint of the parameters and buffers:

    ctx_w [5120,2566], ctx_b [5120]   context columns and bias of the four initial layers, then fc_head.layers.0
    id_w [4,1024,72]                  identity columns of the initial layers
    lin_w [4,4,1024,1024]             block 0 Linear 0, 1, block 1 Linear 0, 1
    bn_s, bn_o [4,4,1024]             the BatchNorm in front of each as v * s + o; a block's first Linear bias is inside the second's o
    res_b [4,2,1024]                  bias of each block's second Linear
    fin_w [4,72,1024], fin_b [4,72]
    lu_w [4,144,144]                  inv(L U)
    act_s, act_o [4,144]              x = (lu_w y) * act_s + act_o: exp(-log_scale), -(lu_w bias + shift) exp(-log_scale)
    fc_w [13,1024], fc_b [13]         fc_head.layers.2 with init_betas / init_cam added to the bias
    id_parity                         bit k: layer k's identity features are the odd indices
    log_det, log_const                sum of the layers' log|det|; log_det - 72 log 2 pi"""
    key = _fingerprint(head)
    if head._fold is not None and head._fold[0] == key:
        return head._fold[1]
    d = lambda t: t.detach().double().cpu()
    ctx_w, ctx_b, id_w, lin_w, bn_s, bn_o, res_b, fin_w, fin_b, lu_w, act_s, act_o = ([] for _ in range(12))
    parity = 0
    even, odd = torch.arange(0, DIM, 2), torch.arange(1, DIM, 2)
    for k in range(LAYERS):
        act, lu, cp = head.layer(k)
        idf, tf = cp.identity_features.cpu(), cp.transform_features.cpu()
        if torch.equal(idf, odd) and torch.equal(tf, even):
            parity |= 1 << k
        elif not (torch.equal(idf, even) and torch.equal(tf, odd)):
            raise ValueError(f"flow layer {k}: identity_features / transform_features are not the even / odd split of ConditionalGlow "
                             "(glow.py:36-37); this kernel takes no other mask")
        net = cp.transform_net
        w0 = d(net.initial_layer.weight)
        id_w.append(w0[:, :HALF])
        ctx_w.append(w0[:, HALF:])
        ctx_b.append(d(net.initial_layer.bias))
        ws, ss, os_, rb = [], [], [], []
        for blk in net.blocks:
            prev_bias = None
            for j in range(2):
                bn = blk.batch_norm_layers[j]
                s = d(bn.weight) / torch.sqrt(d(bn.running_var) + bn.eps)
                o = d(bn.bias) - d(bn.running_mean) * s
                if prev_bias is not None:
                    o = o + prev_bias * s
                ss.append(s)
                os_.append(o)
                ws.append(d(blk.linear_layers[j].weight))
                prev_bias = d(blk.linear_layers[j].bias)
            rb.append(prev_bias)
        lin_w.append(torch.stack(ws))
        bn_s.append(torch.stack(ss))
        bn_o.append(torch.stack(os_))
        res_b.append(torch.stack(rb))
        fin_w.append(d(net.final_layer.weight))
        fin_b.append(d(net.final_layer.bias))
        lower, upper = lu_matrices(lu, torch.float64)
        minv = torch.linalg.inv(lower.cpu() @ upper.cpu())
        inv_scale = torch.exp(-d(act.log_scale))
        lu_w.append(minv)
        act_s.append(inv_scale)
        act_o.append(-(minv @ d(lu.bias) + d(act.shift)) * inv_scale)
    fc = head.fc_head
    ctx_w.append(d(fc.layers[0].weight))
    ctx_b.append(d(fc.layers[0].bias))
    log_det = log_det_constant(head)
    out = {
        "ctx_w": torch.cat(ctx_w), "ctx_b": torch.cat(ctx_b), "id_w": torch.stack(id_w), "lin_w": torch.stack(lin_w),
        "bn_s": torch.stack(bn_s), "bn_o": torch.stack(bn_o), "res_b": torch.stack(res_b), "fin_w": torch.stack(fin_w),
        "fin_b": torch.stack(fin_b), "lu_w": torch.stack(lu_w), "act_s": torch.stack(act_s), "act_o": torch.stack(act_o),
        "fc_w": d(fc.layers[2].weight),
        "fc_b": d(fc.layers[2].bias) + torch.cat([d(fc.init_betas).reshape(10), d(fc.init_cam).reshape(3)]),
        "id_parity": parity, "log_det": log_det, "log_const": log_det - LOG_Z,
    }
    head._fold = (key, out)
    return out


# ----------------------------------------------------------------------------- the kernel
def _weights(head: SMPLFlowHead, device) -> L.FlowHead:
    key = (torch.device(device), _fingerprint(head))
    if head._wcache is not None and head._wcache[0] == key:
        return head._wcache[1]
    f = fold(head)
    dev32 = lambda t: t.float().contiguous().to(device)
    pad = lambda t, k: F.pad(t, (0, k - t.shape[-1]))
    keep = {n: dev32(f[n]) for n in ("ctx_b", "lin_w", "bn_s", "bn_o", "res_b", "fin_w", "fin_b", "lu_w", "act_s", "act_o", "fc_w", "fc_b")}
    keep["ctx_w"] = dev32(pad(f["ctx_w"], CTX_PAD))
    keep["id_w"] = dev32(pad(f["id_w"], ID_PAD))
    w = L.FlowHead()
    for n, t in keep.items():
        setattr(w, n, t.data_ptr())
    w.id_parity = int(f["id_parity"])
    w.log_const = float(f["log_const"])
    head._wcache = (key, w, keep)
    return w


@torch.no_grad()
def flow_head_hip(head: SMPLFlowHead, ctx: torch.Tensor, z: torch.Tensor):
    """ctx [L,2566], z [L,S,144], fp32 on the ROCm device -> pose6d [L,S,144], rotmat [L,S,24,3,3], betas [L,10], cam [L,3],
    log_prob [L,S]: ``seeme_flow_head`` on the current stream.  There is no fallback: a shape it does not take is a ValueError."""
    L_, S = _check_inputs(ctx, z)
    L.require_cuda(ctx, "ctx")
    L.require_cuda(z, "z")
    if z.device != ctx.device:
        raise L.SeemeError(f"ctx is on {ctx.device} and z on {z.device}")
    dev = ctx.device
    ctx, z = ctx.contiguous(), z.contiguous()
    need = L.lib().seeme_flow_head_workspace_bytes(L_, S)
    if need == 0:
        raise L.SeemeError(f"seeme_flow_head takes no L = {L_}, S = {S}")
    with torch.cuda.device(dev):
        w = _weights(head, dev)
        ws = head._ws.get(need, dev)
        pose6d = torch.empty(L_, S, DIM, device=dev)
        rotmat = torch.empty(L_, S, 24, 3, 3, device=dev)
        betas = torch.empty(L_, 10, device=dev)
        cam = torch.empty(L_, 3, device=dev)
        log_prob = torch.empty(L_, S, device=dev)
        L.call("seeme_flow_head", C.byref(w), ctx.data_ptr(), z.data_ptr(), L_, S, pose6d.data_ptr(), rotmat.data_ptr(), betas.data_ptr(),
               cam.data_ptr(), log_prob.data_ptr(), ws.data_ptr(), ws.numel(), L.current_stream())
    return pose6d, rotmat, betas, cam, log_prob


# ----------------------------------------------------------------------------- around the head
def _per_frame(v, n: int, like: torch.Tensor, name: str) -> torch.Tensor:
    t = torch.as_tensor(v, dtype=like.dtype, device=like.device)
    if t.dim() == 0:
        t = t.expand(n)
    if tuple(t.shape) != (n,):
        raise ValueError(f"{name} is {tuple(t.shape)}: expected a scalar or [{n}]")
    return t


def context_rows(image_feats, scene_feats, center, scale, f, cx, cy) -> torch.Tensor:
    """[cam_cx/f, cam_cy/f, box_cx/f, box_cy/f, box_size/f, f/1500, image 2048, scene 512] per frame: the torch.cat order of prohmr_scene.py:119-138."""
    n = image_feats.shape[0]
    if tuple(image_feats.shape) != (n, IMAGE_DIM) or tuple(scene_feats.shape) != (n, SCENE_DIM):
        raise ValueError(f"image features are {tuple(image_feats.shape)} and scene features {tuple(scene_feats.shape)}: expected "
                         f"[L,{IMAGE_DIM}] and [L,{SCENE_DIM}]")
    center = torch.as_tensor(center, dtype=image_feats.dtype, device=image_feats.device)
    if tuple(center.shape) != (n, 2):
        raise ValueError(f"center is {tuple(center.shape)}: expected [{n},2]")
    size = 200.0 * _per_frame(scale, n, image_feats, "scale")            # egobody_dataset.py:269-272, 422-423
    f, cx, cy = (_per_frame(v, n, image_feats, name) for v, name in ((f, "f"), (cx, "cx"), (cy, "cy")))
    head6 = torch.stack([cx / f, cy / f, center[:, 0] / f, center[:, 1] / f, size / f, f / FX_NORM_COEFF], dim=1)
    return torch.cat([head6, image_feats, scene_feats.to(image_feats.dtype)], dim=1)


def cam_to_transl(cam, center, scale, f, cx, cy) -> torch.Tensor:
    """Weak-perspective crop camera -> the body's translation in the full image's camera: convert_pare_to_full_img_cam (EgoHMR/utils/geometry.py:126-130) with img_w = 2 cx, img_h = 2 cy."""
    n = cam.shape[0]
    if cam.dim() != 2 or cam.shape[1] != 3:
        raise ValueError(f"cam is {tuple(cam.shape)}: expected [L,3]")
    bad = torch.nonzero(~(cam[:, 0] > 0)).reshape(-1)
    if bad.numel():
        i = int(bad[0])
        raise ValueError(f"frame {i}: the predicted camera scale cam[0] is {float(cam[i, 0])}, not > 0: the depth 2 f / (b s) has no meaning")
    center = torch.as_tensor(center, dtype=cam.dtype, device=cam.device)
    size = 200.0 * _per_frame(scale, n, cam, "scale")
    f, cx, cy = (_per_frame(v, n, cam, name) for v, name in ((f, "f"), (cx, "cx"), (cy, "cy")))
    s, tx, ty = cam[:, 0], cam[:, 1], cam[:, 2]
    r = size / IMAGE_SIZE
    tz = 2 * f / (r * IMAGE_SIZE * s)
    ox = 2 * (center[:, 0] - (2 * cx) / 2.0) / (s * size)
    oy = 2 * (center[:, 1] - (2 * cy) / 2.0) / (s * size)
    return torch.stack([tx + ox, ty + oy, tz], dim=-1)


def head_box(center, scale) -> np.ndarray:
    """center [L,2], scale [L] -> the [L,3] float32 table (cx, cy, b) of the HEAD's crop: b = 200 scale, centred on ``center`` (egobody_dataset.py:269-272).

    Unlike ``crops.patch_box``, which restates SEE-ME's own box for SEE-ME's image token (it adds b to the stored centre,
    dataset.py:1670-1672), ProHMR-scene was trained on crops centred on the stored centre.  This is the one place where the two
    crops differ; ``seeme_crop_patches`` takes arbitrary boxes, so both are cut by the same kernel."""
    c, s = np.asarray(center, np.float32), np.asarray(scale, np.float32)
    if c.ndim != 2 or c.shape[1] != 2 or s.shape != c.shape[:1]:
        raise ValueError(f"head_box: center is {c.shape}, scale is {s.shape}: expected [L,2] and [L]")
    return np.stack([c[:, 0], c[:, 1], s * np.float32(200.0)], axis=-1).astype(np.float32)


def draw_z(L_: int, S: int, generator=None, device="cpu") -> torch.Tensor:
    """z [L,S,144]: sample 0 is the mode (z = 0), samples 1.. are standard normal draws of `generator` (prohmr_scene.py:152-158 puts the mode first)."""
    z = torch.zeros(L_, S, DIM)
    if S > 1:
        z[:, 1:] = torch.randn(L_, S - 1, DIM, generator=generator)
    return z.to(device)


# ----------------------------------------------------------------------------- checkpoints
_SKIP_PREFIXES = ("smpl", "discriminator.")          # mld/models/modeltype/mld.py:197-203


def flow_state_from_checkpoint(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The head's entries out of a SEE-ME state dict (``proscene.flow.*``) or a ProHMR-scene one (``flow.*``, no prefix; its
    ``smpl*``, ``discriminator.*`` and loss entries are skipped as mld.py:197-203 does), renamed to this module's names.  A file
    without them is a KeyError naming the first missing key."""
    want = state_shapes()
    for prefix in ("proscene.flow.", "flow."):
        got = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix) and not k.startswith(_SKIP_PREFIXES)}
        if got:
            break
    else:
        prefix, got = "proscene.flow.", {}
    for k in want:
        if k not in got:
            raise KeyError(f"the checkpoint has no '{prefix}{k}': it does not hold the ProHMR-scene pose head (flow.* / proscene.flow.*)")
    return {k: got[k] for k in want}
