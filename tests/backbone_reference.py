"""The ResNet-50 backbone restated in plain torch (F.conv2d, BatchNorm written out with the running statistics): the oracle of the
GPU tests, pinned on the CPU to tests/golden/resnet50_B2.npz (made from the reference module by make_golden_backbone.py).
Works on a state dict with the reference's names, in any floating dtype, on any device."""
import numpy as np
import torch
import torch.nn.functional as F

BLOCKS = (3, 4, 6, 3)
EPS = 1e-5
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def recipe_state(dtype=torch.float32, device="cpu", seed=1234):
    """The backbone recipe as a state dict with the reference's 318 names."""
    from seeme_amd.resnet import state_shapes
    from seeme_amd.weights_recipe import backbone_recipe_tensor
    sd = {}
    for k, shp in state_shapes().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long, device=device)
        else:
            sd[k] = torch.from_numpy(backbone_recipe_tensor(k, shp, seed)).to(device=device, dtype=dtype)
    return sd


def normalise(crops_u8):
    """uint8 [B,H,W,3] RGB -> float32 [B,3,H,W], the reference formula (dataset.py:1693-1705): (x - 255 mean_c) / (255 std_c)."""
    x = torch.as_tensor(crops_u8).float().permute(0, 3, 1, 2)
    mean = torch.tensor([255.0 * m for m in MEAN], dtype=torch.float64).float().to(x.device)[None, :, None, None]
    std = torch.tensor([255.0 * s for s in STD], dtype=torch.float64).float().to(x.device)[None, :, None, None]
    return ((x - mean) / std).contiguous()


def bn(sd, name, x):
    w, b, m, v = (sd[f"{name}.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + EPS) * w[None, :, None, None] + b[None, :, None, None]


def conv_bn(sd, conv, bnname, x, stride=1, relu=False, residual=None):
    w = sd[conv + ".weight"]
    y = bn(sd, bnname, F.conv2d(x, w, stride=stride, padding=w.shape[-1] // 2))
    if residual is not None:
        y = y + residual
    return F.relu(y) if relu else y


def bottleneck(sd, p, x, stride, down):
    o = conv_bn(sd, p + "conv1", p + "bn1", x, relu=True)
    o = conv_bn(sd, p + "conv2", p + "bn2", o, stride=stride, relu=True)
    res = conv_bn(sd, p + "downsample.0", p + "downsample.1", x, stride=stride) if down else x
    return conv_bn(sd, p + "conv3", p + "bn3", o, relu=True, residual=res)


def stem(sd, x):
    return conv_bn(sd, "conv1", "bn1", x, stride=2, relu=True)


def forward(sd, x, stages=None):
    """x [B,3,H,W] normalised -> [B,2048]; stages (a list) receives the NCHW activations after the max-pool and layer1..4."""
    x = F.max_pool2d(stem(sd, x), 3, 2, 1)
    if stages is not None:
        stages.append(x)
    for li, nb in enumerate(BLOCKS):
        for b in range(nb):
            x = bottleneck(sd, f"layer{li + 1}.{b}.", x, 2 if (b == 0 and li > 0) else 1, b == 0)
        if stages is not None:
            stages.append(x)
    return x.mean(dim=(2, 3))


def smooth_crops(B, seed=0, size=224):
    """uint8 [B,size,size,3]: bilinear upsampling of 7x7 uniform noise -- smooth, so the fixture compresses."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, 7, 7, generator=g)
    up = F.interpolate(low, size=(size, size), mode="bilinear", align_corners=False)
    return (up * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def load_fixture(path):
    d = np.load(path, allow_pickle=False)
    return {k: d[k] for k in d.files}
