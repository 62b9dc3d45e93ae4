#!/usr/bin/env python3
"""Generate resnet50_B2.npz from the REFERENCE's own ResNet-50 (EgoHMR/models/resnet.py, imported by path).

Runs only where the reference tree exists (SEEME_REFERENCE, default /root/reference); nothing of it is copied.  Weights: the
backbone recipe of seeme_amd.weights_recipe; inputs: two smooth uint8 crops (bilinear upsampling of 7x7 uniform noise, seeded),
normalised with the dataset's formula (dataset.py:1693-1705); outputs: what the reference module computes on the CPU, fp32, eval.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_backbone.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SEEME_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from seeme_amd.weights_recipe import load_backbone_recipe_  # noqa: E402
import backbone_reference as R  # noqa: E402

torch.set_grad_enabled(False)
PIXELS = ((0, 0, 0), (0, 55, 55), (0, 17, 40), (1, 30, 2), (1, 9, 9))      # (image, h, w): corners, borders, interior


def main():
    spec = importlib.util.spec_from_file_location("ref_resnet", os.path.join(REF, "EgoHMR", "models", "resnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = load_backbone_recipe_(mod.resnet50(pretrained=False)).eval()
    crops = R.smooth_crops(2, seed=0)
    x = R.normalise(crops)
    stages = []
    h = net.maxpool(net.relu(net.bn1(net.conv1(x))))
    stages.append(h)
    for name in ("layer1", "layer2", "layer3", "layer4"):
        h = getattr(net, name)(h)
        stages.append(h)
    feats = net(x)
    assert torch.equal(feats, stages[-1].mean(dim=(2, 3)))
    f64 = net.double()(x.double())
    print("fp32 vs float64:", float((feats.double() - f64).abs().max() / f64.abs().max()))
    print("stage maxima:", [round(float(s.max()), 3) for s in stages], "feats mean/max:", float(feats.mean()), float(feats.max()),
          "zeros:", float((feats == 0).float().mean()), "image difference:", float((feats[0] - feats[1]).abs().max() / feats.abs().max()))
    sd = net.float().state_dict()
    out = {"crops": crops.numpy(), "feats": feats.numpy(),
           "keys": np.array(sorted(sd)), "shapes": np.array([",".join(str(d) for d in sd[k].shape) for k in sorted(sd)]),
           "pixels": np.array(PIXELS, np.int64)}
    for name, s in zip(("pool", "layer1", "layer2", "layer3", "layer4"), stages):
        out["mean_" + name] = s.mean(dim=(2, 3)).numpy()
    # full-depth pixels [n, C]; layer3 is 14x14, so its coordinates are those of PIXELS divided by 4
    out["pix_layer1"] = np.stack([stages[1][b, :, i, j].numpy() for b, i, j in PIXELS])
    out["pix_layer3"] = np.stack([stages[3][b, :, i // 4, j // 4].numpy() for b, i, j in PIXELS])
    path = os.path.join(HERE, "resnet50_B2.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
