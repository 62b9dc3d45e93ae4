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
        make = backbone_recipe_tensor if is_backbone_key(k) else recipe_tensor
        new[k] = torch.from_numpy(make(k, tuple(v.shape), seed)).to(dtype=v.dtype)
    module.load_state_dict(new, strict=True)
    return module
