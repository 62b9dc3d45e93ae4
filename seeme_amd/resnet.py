"""ResNet50 -- drop-in for ``EgoHMR.models.resnet.resnet50`` (resnet.py:99-150: ``ResNet(Bottleneck, [3, 4, 6, 3])`` without
``fc``, output = mean over the 7x7 map of layer4), the frozen image backbone MLD consumes through ``ProHMRScene.encode_image``
(prohmr_scene.py:33-34, 99-100; mld/models/modeltype/mld.py:893-896).  Same 318 state-dict entries (``conv1.weight``, ``bn1.*``,
``layer{1..4}.{i}.conv{1,2,3}.weight``, ``...bn{1,2,3}.*``, ``...downsample.{0,1}.*``) so the ``proscene.backbone.*`` entries of a
checkpoint load; forward runs in libseeme_hip.so (csrc/resnet.hip).

Always eval mode: BatchNorm uses its running statistics and is folded on the host into each convolution (the
reference leaves these BatchNorms in training mode during ``fit``)."""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import torch
import torch.nn as nn

from . import _lib as L

BLOCKS = (3, 4, 6, 3)
OUT_DIM = 2048
BN_EPS = 1e-5
IMAGENET_MEAN = (0.485, 0.456, 0.406)        # dataset.py:1693-1705
IMAGENET_STD = (0.229, 0.224, 0.225)


def conv_table() -> List[Tuple[str, str, int, int, int, int]]:
    """(conv name, bn name, cin, cout, k, stride) of the 53 convolutions in the order SeemeResnet50.conv holds them: conv1, then
    per bottleneck conv1, conv2 (carries the stride), conv3 and, in a layer's first block, downsample."""
    t = [("conv1", "bn1", 3, 64, 7, 2)]
    inpl = 64
    for li, nb in enumerate(BLOCKS):
        pl = 64 << li
        for b in range(nb):
            s = 2 if (b == 0 and li > 0) else 1
            p = f"layer{li + 1}.{b}."
            t += [(p + "conv1", p + "bn1", inpl, pl, 1, 1), (p + "conv2", p + "bn2", pl, pl, 3, s), (p + "conv3", p + "bn3", pl, 4 * pl, 1, 1)]
            if b == 0:
                t.append((p + "downsample.0", p + "downsample.1", inpl, 4 * pl, 1, s))
            inpl = 4 * pl
    return t


def state_shapes() -> dict:
    """{name: shape} of the reference module's state dict (318 entries)."""
    out = {}
    for conv, bn, cin, cout, k, _s in conv_table():
        out[conv + ".weight"] = (cout, cin, k, k)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            out[f"{bn}.{leaf}"] = (cout,)
        out[bn + ".num_batches_tracked"] = ()
    return out


def fold_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv weight [cout,cin,k,k] + eval-mode BatchNorm -> (weight, bias) in float64: w g / sqrt(var + eps), b - mean g / sqrt(var + eps)."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s[:, None, None, None], beta.double() - mean.double() * s


def normalise_uint8(crops: torch.Tensor) -> torch.Tensor:
    """uint8 NHWC RGB [B,H,W,3] -> float32 NCHW, (x - 255 mean_c) / (255 std_c): what the stem's loader computes for uint8 input."""
    mean = torch.tensor([255.0 * m for m in IMAGENET_MEAN], dtype=torch.float64).float().to(crops.device)    # float64 product, rounded once
    std = torch.tensor([255.0 * s for s in IMAGENET_STD], dtype=torch.float64).float().to(crops.device)
    return ((crops.float() - mean) / std).permute(0, 3, 1, 2).contiguous()


def pack_conv(w64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Folded weight [cout,cin,k,k] (float64) -> MFMA fragments in the order k_conv consumes them (include/seeme_hip.h):
    K = (kh, kw, cin) with cin fastest (the stem's cin 3 zero padded to one 16-byte chunk per tap, its K to a whole K-step),
    rows of every 64-channel group interleaved so that a lane owns 16 consecutive channels, then [cout/16][K/(4E)][kq 4][r 16][E]."""
    E = 16 // torch.empty(0, dtype=dtype).element_size()
    cout, cin, k, _ = w64.shape
    w = w64.permute(0, 2, 3, 1)                                     # [cout, kh, kw, cin]
    if cin < E:
        w = torch.cat([w, w.new_zeros(cout, k, k, E - cin)], dim=-1)
    w = w.reshape(cout, -1)
    kstep = 8 * E                                                   # 128 bytes of k
    if w.shape[1] % kstep:
        w = torch.cat([w, w.new_zeros(cout, kstep - w.shape[1] % kstep)], dim=1)
    t, r = torch.meshgrid(torch.arange(cout // 16), torch.arange(16), indexing="ij")
    rows = (64 * (t // 4) + 16 * (r // 4) + 4 * (t % 4) + r % 4).reshape(-1).to(w.device)
    w = w[rows].to(dtype)
    return w.view(cout // 16, 16, w.shape[1] // (4 * E), 4, E).permute(0, 2, 3, 1, 4).contiguous()


class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * planes)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False), nn.BatchNorm2d(4 * planes))


def _fingerprint(module: nn.Module):
    # parameters AND buffers: the running statistics are part of the folded weights
    return tuple((t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers()))


class ResNet50(nn.Module):
    """Parameter holder with the reference's names; ``forward`` = ``encode``.  Frozen: no parameter requires a gradient and
    ``train()`` does not reach the BatchNorms (they always use the running statistics)."""

    def __init__(self, precision: str = "fp32"):
        super().__init__()
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' (fp32 MFMA, parity path) or 'bf16' (bf16 weights and activations)")
        self.precision = precision
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inpl = 64
        for li, nb in enumerate(BLOCKS):
            pl = 64 << li
            blocks = []
            for b in range(nb):
                blocks.append(_Bottleneck(inpl, pl, 2 if (b == 0 and li > 0) else 1, downsample=b == 0))
                inpl = 4 * pl
            setattr(self, f"layer{li + 1}", nn.Sequential(*blocks))
        for p in self.parameters():
            p.requires_grad = False
        self._wcache = None
        self._ws = L.Workspace(per_stream=False)

    def train(self, mode: bool = True):
        return super().train(False)

    def stale(self) -> bool:
        """True when the packed weight image no longer matches the tensors (load_state_dict, .to(), in-place edits)."""
        return self._wcache is None or self._wcache[0] != (self.precision, _fingerprint(self))

    def folded(self, i: int):
        """(weight [cout,cin,k,k], bias [cout]) of convolution i of conv_table() with its BatchNorm folded in, float64."""
        conv, bn = conv_table()[i][:2]
        c, b = self.get_submodule(conv), self.get_submodule(bn)
        return fold_bn(c.weight, b.weight, b.bias, b.running_mean, b.running_var, BN_EPS)

    def _weights(self) -> L.Resnet50:
        if self.precision not in ("fp32", "bf16"):
            raise ValueError(f"ResNet50.precision is {self.precision!r}: 'fp32' or 'bf16' (TRAIN.IMAGE_PRECISION)")
        if not self.stale():
            return self._wcache[1]
        for p in self.parameters():
            L.require_cuda(p, "ResNet50 parameter")
        key = (self.precision, _fingerprint(self))
        bf = self.precision == "bf16"
        w = L.Resnet50()
        w.precision = L.RESNET_BF16 if bf else L.RESNET_FP32
        keep = []
        with torch.no_grad():
            for i, (_c, _b, cin, cout, k, s) in enumerate(conv_table()):
                w64, b64 = self.folded(i)
                pk = pack_conv(w64, torch.bfloat16 if bf else torch.float32)
                bias = b64.float().contiguous()
                keep += [pk, bias]
                e = w.conv[i]
                e.weight, e.weight_bf16 = (0, pk.data_ptr()) if bf else (pk.data_ptr(), 0)
                e.bias, e.cin, e.cout, e.k, e.stride = bias.data_ptr(), cin, cout, k, s
        self._wcache = (key, w, keep)
        return w

    @staticmethod
    def image_format(images: torch.Tensor) -> int:
        """The two accepted forms: float32 NCHW [B,3,224,224] (normalised) or uint8 NHWC [B,224,224,3] (RGB)."""
        if not torch.is_tensor(images) or images.dim() != 4:
            raise L.SeemeError("images must be a 4-D tensor: float32 [B,3,224,224] or uint8 [B,224,224,3]")
        if images.dtype == torch.uint8 and tuple(images.shape[1:]) == (224, 224, 3):
            return L.IMG_U8_NHWC
        if images.dtype == torch.float32 and tuple(images.shape[1:]) == (3, 224, 224):
            return L.IMG_F32_NCHW
        raise L.SeemeError(f"images are {tuple(images.shape)} {images.dtype}: expected float32 [B,3,224,224] (normalised) or "
                           "uint8 [B,224,224,3] (RGB)")

    def encode(self, images: torch.Tensor, taps=None) -> torch.Tensor:
        """images -> [B,2048] float32.  taps (bring-up): a list that receives the NHWC activations after the max-pool and after
        layer1..4 in the precision's element type."""
        fmt = self.image_format(images)
        if not images.is_cuda:
            raise L.SeemeError("images must be on the ROCm device (cuda:N); this path has no CPU fallback")
        B = images.shape[0]
        images = images.contiguous()
        dev = images.device
        out = torch.empty(B, OUT_DIM, device=dev, dtype=torch.float32)
        prec = L.RESNET_BF16 if self.precision == "bf16" else L.RESNET_FP32
        need = L.lib().seeme_resnet50_workspace_bytes(B, prec)
        if need == 0:
            raise L.SeemeError(f"ResNet50: batch size {B} is outside 1..1024")
        ws = self._ws.get(need, dev)
        w = self._weights()
        if taps is not None:
            dt = torch.bfloat16 if self.precision == "bf16" else torch.float32
            bufs = [torch.empty(B, s, s, c, device=dev, dtype=dt) for s, c in ((56, 64), (56, 256), (28, 512), (14, 1024), (7, 2048))]
            w = L.Resnet50.from_buffer_copy(w)
            for i, t in enumerate(bufs):
                w.tap[i] = t.data_ptr()
            taps.extend(bufs)
        L.call("seeme_resnet50_encode", C.byref(w), images.data_ptr(), fmt, B, out.data_ptr(), ws.data_ptr(), ws.numel(),
               L.current_stream())
        return out

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        return self.encode(images)


# ----------------------------------------------------------------------------- the pieces one by one (tests, bring-up)
def _prec(precision: str):
    if precision not in ("fp32", "bf16"):
        raise ValueError("precision must be 'fp32' or 'bf16'")
    return (L.RESNET_BF16, torch.bfloat16) if precision == "bf16" else (L.RESNET_FP32, torch.float32)


def conv2d_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, stride: int = 1, residual=None, relu: bool = False,
                precision: str = "fp32") -> torch.Tensor:
    """One k_conv launch: x [B,H,W,cin] NHWC in the precision's dtype (for cin 3: the output of stem_pack), weight [cout,cin,k,k]
    and bias [cout] as folded -> [B,Ho,Wo,cout], padding k/2, epilogue + bias, + residual, ReLU."""
    code, dt = _prec(precision)
    if not x.is_cuda or x.dtype != dt:
        raise L.SeemeError(f"conv2d_nhwc: x must be a {dt} tensor on the ROCm device")
    cout, cin, k, _ = weight.shape
    B, H, W, _c = x.shape
    E = 16 // torch.empty(0, dtype=dt).element_size()
    if cout % 64:
        raise L.SeemeError(f"conv2d_nhwc: cout {cout} is no multiple of 64")
    if cin != 3 and (cin % E or (cin // E) & (cin // E - 1)):
        raise L.SeemeError(f"conv2d_nhwc: cin {cin} must be 3 or a power-of-two number of 16-byte chunks")
    pk = pack_conv(weight.double(), dt).to(x.device)
    b = bias.float().contiguous().to(x.device)
    c = L.Conv()
    c.weight, c.weight_bf16 = (0, pk.data_ptr()) if precision == "bf16" else (pk.data_ptr(), 0)
    c.bias, c.cin, c.cout, c.k, c.stride = b.data_ptr(), cin, cout, k, stride
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    y = torch.empty(B, Ho, Wo, cout, device=x.device, dtype=dt)
    x = x.contiguous()
    if residual is not None:
        residual = residual.contiguous()
        if residual.shape != y.shape or residual.dtype != dt:
            raise L.SeemeError("conv2d_nhwc: the residual must have the output's shape and dtype")
    L.call("seeme_resnet_conv", C.byref(c), code, x.data_ptr(), B, H, W, L.ptr(residual), int(relu), y.data_ptr(), L.current_stream())
    return y


def stem_pack(images: torch.Tensor, precision: str = "fp32") -> torch.Tensor:
    """The stem's loader on its own: float32 NCHW [B,3,H,W] or uint8 NHWC [B,H,W,3] -> [B,H,W,16 bytes] (r, g, b, 0 ...)."""
    code, dt = _prec(precision)
    if not images.is_cuda or images.dim() != 4:
        raise L.SeemeError("stem_pack: a 4-D tensor on the ROCm device")
    if images.dtype == torch.uint8 and images.shape[3] == 3:
        fmt, (B, H, W) = L.IMG_U8_NHWC, (images.shape[0], images.shape[1], images.shape[2])
    elif images.dtype == torch.float32 and images.shape[1] == 3:
        fmt, (B, H, W) = L.IMG_F32_NCHW, (images.shape[0], images.shape[2], images.shape[3])
    else:
        raise L.SeemeError("stem_pack: float32 [B,3,H,W] or uint8 [B,H,W,3]")
    y = torch.empty(B, H, W, 16 // torch.empty(0, dtype=dt).element_size(), device=images.device, dtype=dt)
    L.call("seeme_resnet_stem_pack", images.contiguous().data_ptr(), fmt, B, H, W, code, y.data_ptr(), L.current_stream())
    return y


def maxpool_nhwc(x: torch.Tensor, precision: str = "fp32") -> torch.Tensor:
    """MaxPool2d(3, stride 2, padding 1) over NHWC."""
    code, dt = _prec(precision)
    if not x.is_cuda or x.dtype != dt:
        raise L.SeemeError(f"maxpool_nhwc: x must be a {dt} tensor on the ROCm device")
    B, H, W, Cc = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, device=x.device, dtype=dt)
    L.call("seeme_resnet_maxpool", code, x.contiguous().data_ptr(), B, H, W, Cc, y.data_ptr(), L.current_stream())
    return y
