"""Deterministic weight recipe ("weights by recipe, I/O by fixture").

No checkpoint, dataset or SMPL file exists offline, so every
parity fixture and every benchmark uses weights generated here from a seed.
The recipe only looks at parameter *names and shapes*, which are identical in
the reference modules and in this package, so the same
state-dict can be loaded into the reference module (fixture generation, in the
build container only) and into ours (everywhere).

The values are chosen so that every branch of the path is numerically alive
(non-zero biases, non-unit LayerNorm gains, non-zero ``zero_module`` layers;
the reference re-initialises those with xavier anyway, see
mld/models/operator/cross_attention.py:36-39).
"""
from __future__ import annotations

import zlib
from typing import Dict, Iterable, Mapping, Tuple

import numpy as np


def _key_seed(seed: int, key: str) -> int:
    # Stable per-key stream: independent of dict order and of other keys.
    return (int(seed) * 1000003 + zlib.crc32(key.encode("utf-8"))) & 0x7FFFFFFF


def recipe_tensor(key: str, shape: Tuple[int, ...], seed: int = 1234) -> np.ndarray:
    """float32 array for one parameter, determined by (seed, key, shape)."""
    rng = np.random.Generator(np.random.PCG64(_key_seed(seed, key)))
    shape = tuple(int(s) for s in shape)
    leaf = key.rsplit(".", 1)[-1]
    if leaf == "pe":  # PositionEmbeddingLearned1D: uniform(0,1) (position_encoding.py:150-151)
        out = rng.random(shape)
    elif key.endswith("global_motion_token"):
        out = rng.standard_normal(shape)
    elif len(shape) >= 2:
        fan_out, fan_in = shape[0], int(np.prod(shape[1:]))
        # xavier-uniform-like scale (cross_attention.py:36-39), gaussian draw
        std = np.sqrt(2.0 / (fan_in + fan_out))
        out = rng.standard_normal(shape) * std
    elif "norm" in key and leaf == "weight":
        out = 1.0 + 0.1 * rng.standard_normal(shape)
    else:  # biases and LayerNorm biases
        out = 0.05 * rng.standard_normal(shape)
    return np.ascontiguousarray(out, dtype=np.float32)


def is_backbone_key(key: str) -> bool:
    """Entries of the ResNet-50 image backbone inside a larger model (``proscene.backbone.*``)."""
    return key.startswith("backbone.") or ".backbone." in key


def backbone_recipe_tensor(key: str, shape: Tuple[int, ...], seed: int = 1234) -> np.ndarray:
    """Recipe of the ResNet-50 backbone, keyed by the entry's name inside the backbone (``layer1.0.bn3.weight``; a
    ``...backbone.`` prefix is dropped, so the module alone and the module inside MLD receive the same values).  The generic
    recipe gives BatchNorm gains of ~0.05 and negative running variances; here convolutions are N(0, sqrt(2 / fan_in)),
    BatchNorm weight 1 + 0.1 N (times 0.35 for every bn3 and downsample.1, which keeps the residual stream O(1) over 16 blocks),
    bias 0.05 N, running_mean 0.1 N, running_var U(0.5, 1.5)."""
    tail = key.split("backbone.", 1)[1] if is_backbone_key(key) else key
    rng = np.random.Generator(np.random.PCG64(_key_seed(seed, "backbone." + tail)))
    shape = tuple(int(s) for s in shape)
    parts = tail.split(".")
    leaf = parts[-1]
    block_end = parts[-2:-1] == ["bn3"] or parts[-3:-1] == ["downsample", "1"]
    if len(shape) == 4:
        out = rng.standard_normal(shape) * np.sqrt(2.0 / float(np.prod(shape[1:])))
    elif leaf == "weight":
        out = (1.0 + 0.1 * rng.standard_normal(shape)) * (0.35 if block_end else 1.0)
    elif leaf == "bias":
        out = 0.05 * rng.standard_normal(shape)
    elif leaf == "running_mean":
        out = 0.1 * rng.standard_normal(shape)
    elif leaf == "running_var":
        out = 0.5 + rng.random(shape)
    else:
        raise KeyError(f"no backbone recipe for {key}")
    return np.ascontiguousarray(out, dtype=np.float32)


def load_backbone_recipe_(module, seed: int = 1234):
    """In-place: the backbone recipe for every floating-point entry of a ResNet-50 module on its own."""
    import torch

    sd = module.state_dict()
    new = {k: (torch.from_numpy(backbone_recipe_tensor(k, tuple(v.shape), seed)).to(dtype=v.dtype) if torch.is_floating_point(v) else v)
           for k, v in sd.items()}
    module.load_state_dict(new, strict=True)
    return module


def _flow_head_tail(key: str):
    for mark in ("flow._transform.", "fc_head."):
        i = key.find(mark)
        if i >= 0:
            return key[i:]
    return None


def is_flow_head_key(key: str) -> bool:
    """Entries of the ProHMR-scene pose head inside a larger model (``proscene.flow.flow._transform...``, ``proscene.flow.fc_head...``)."""
    return _flow_head_tail(key) is not None


def flow_head_recipe_tensor(key: str, shape: Tuple[int, ...], seed: int = 1234) -> np.ndarray:
    """Recipe of the pose head (SMPLFlow), keyed by the entry's name inside the head (``flow._transform._transforms.2...``,
    ``fc_head...``; whatever stands in front is dropped, so the module alone and the module inside MLD receive the same values).  The values keep every stage alive and well conditioned: linear weights N(0, 0.03)
    (``fc_head.layers.2.weight`` N(0, 0.003), so that the camera scale stays near init_cam), biases 0.05 N, BatchNorm weight
    1 + 0.1 N, bias 0.05 N, running_mean 0.1 N, running_var U(1, 1.3); ActNorm log_scale and shift 0.1 N; LU lower / upper
    entries 0.02 N, unconstrained_upper_diag 0.1 N, bias 0.05 N; init_cam (0.9, 0, 0) + 0.02 N on the offsets, init_betas 0.1 N."""
    tail = _flow_head_tail(key)
    if tail is None:
        raise KeyError(f"no flow-head recipe for {key}")
    rng = np.random.Generator(np.random.PCG64(_key_seed(seed, "flow_head." + tail)))
    shape = tuple(int(s) for s in shape)
    leaf = tail.rsplit(".", 1)[-1]
    n = lambda std: std * rng.standard_normal(shape)
    if leaf == "running_var":
        out = 1.0 + 0.3 * rng.random(shape)
    elif leaf == "dummy_buffer":                  # nflows' per-transform device marker: its value is never read
        out = np.ones(shape)
    elif leaf == "running_mean":
        out = n(0.1)
    elif "batch_norm_layers" in tail and leaf == "weight":
        out = 1.0 + n(0.1)
    elif leaf in ("log_scale", "shift", "unconstrained_upper_diag", "init_betas"):
        out = n(0.1)
    elif leaf in ("lower_entries", "upper_entries"):
        out = n(0.02)
    elif leaf == "init_cam":
        out = n(0.02)
        out.reshape(-1)[0] = 0.9
    elif leaf == "weight" and len(shape) == 2:
        out = n(0.003 if tail == "fc_head.layers.2.weight" else 0.03)
    elif leaf == "bias":
        out = n(0.05)
    else:
        raise KeyError(f"no flow-head recipe for {key}")
    return np.ascontiguousarray(out, dtype=np.float32)


def load_flow_head_recipe_(module, seed: int = 1234):
    """In-place: the flow-head recipe for every floating-point entry of an SMPLFlow-shaped module on its own; the ActNorm
    ``initialized`` flags become true, the integer buffers stay."""
    import torch

    sd = module.state_dict()
    new = {}
    for k, v in sd.items():
        if torch.is_floating_point(v):
            new[k] = torch.from_numpy(flow_head_recipe_tensor(k, tuple(v.shape), seed)).to(dtype=v.dtype)
        elif v.dtype == torch.bool:
            new[k] = torch.ones_like(v)
        else:
            new[k] = v
    module.load_state_dict(new, strict=True)
    return module


def recipe_state_dict(shapes: Mapping[str, Iterable[int]], seed: int = 1234) -> Dict[str, np.ndarray]:
    """Fill every entry of ``{name: shape}`` by the recipe."""
    return {k: recipe_tensor(k, tuple(v), seed) for k, v in sorted(shapes.items())}


def load_recipe_(module, seed: int = 1234):
    """In-place: overwrite every entry of ``module.state_dict()`` (torch) by the recipe."""
    import torch

    sd = module.state_dict()
    new = {}
    for k, v in sd.items():
        if not torch.is_floating_point(v):
            new[k] = v
            continue
        make = flow_head_recipe_tensor if is_flow_head_key(k) else backbone_recipe_tensor if is_backbone_key(k) else recipe_tensor
        new[k] = torch.from_numpy(make(k, tuple(v.shape), seed)).to(dtype=v.dtype)
    module.load_state_dict(new, strict=True)
    return module
