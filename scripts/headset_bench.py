#!/usr/bin/env python
"""Cost of the two headset kernels beside their plain-torch twins.  Writes profiles/headset.json (``--out``).

Shapes: (W,K,T) = (32,20,196) for the head-path cost, a recording of L = 5000 frames with sigma = track.DEFAULT_SIGMA (R = 6) and
with sigma = 10 (R = 30) for the anchoring.  Same input for a kernel and its twin, fp32 on the device:
  (a) head_path_cost_hip_ms / head_path_cost_torch_ms   ``seeme_head_path_cost`` (the launch alone: lengths on the device already) /
                                                        ``head_path_cost_torch``
  (b) head_anchor_hip_ms / head_anchor_torch_ms         ``seeme_head_anchor`` / ``head_anchor_torch`` (2R+1 steps of torch ops)
  (c) head_anchor_r30_hip_ms / head_anchor_r30_torch_ms the same with the widest filter

Every leg is warmed up first; times are device events around work that ends in a synchronise; the legs alternate, ``--repeats``
(5) times each; min / median / max in ms."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from hyp_select_bench import alternate                # noqa: E402

SHAPE = (32, 20, 196)
FRAMES = 5000


def legs(dev, repeats):
    import numpy as np
    from seeme_amd import recording as R
    from seeme_amd.track import DEFAULT_SIGMA, gaussian_taps
    W, K, T = SHAPE
    g = torch.Generator().manual_seed(3)
    walk = torch.cumsum(0.02 * torch.randn(W, T, 1, 3, generator=g), dim=1) + 0.3 * torch.randn(1, 1, 24, 3, generator=g)
    jts = (walk[:, None] + 0.1 * torch.randn(W, K, T, 24, 3, generator=g)).to(dev)
    path = (walk[:, :, R.HEAD_JOINT] + torch.tensor([0.05, -0.08, 0.1])).contiguous().to(dev)
    lengths = [T] * (W - 1) + [T // 2]
    len32 = torch.tensor(lengths, dtype=torch.int32, device=dev)
    joints = (torch.cumsum(0.01 * torch.randn(FRAMES, 1, 3, generator=g), dim=0) + 0.3 * torch.randn(1, 24, 3, generator=g)).to(dev)
    hp = (joints[:, R.HEAD_JOINT] + torch.cumsum(0.03 * torch.randn(FRAMES, 3, generator=g), dim=0).to(dev)).contiguous()
    taps, wide = (np.ascontiguousarray(gaussian_taps(s), np.float32) for s in (DEFAULT_SIGMA, 10.0))
    r = alternate({"head_path_cost_hip_ms": lambda: R._launch_head_cost(jts, path, len32, W, K, T),
                   "head_path_cost_torch_ms": lambda: R.head_path_cost_torch(jts, path, len32),
                   "head_anchor_hip_ms": lambda: R._launch_head_anchor(joints, hp, FRAMES, taps, taps.shape[0] - 1),
                   "head_anchor_torch_ms": lambda: R.head_anchor_torch(joints, hp, taps),
                   "head_anchor_r30_hip_ms": lambda: R._launch_head_anchor(joints, hp, FRAMES, wide, wide.shape[0] - 1),
                   "head_anchor_r30_torch_ms": lambda: R.head_anchor_torch(joints, hp, wide)}, repeats)
    a, b = R.head_path_cost_hip(jts, path, lengths), R.head_path_cost_torch(jts, path, lengths)
    r["head_path_cost_max_rel_diff_hip_vs_torch_fp32"] = float(((a - b).abs() / b).max())
    (s, e), (st, et) = R.head_anchor_hip(joints, hp, taps), R.head_anchor_torch(joints, hp, taps)
    r["head_shift_max_abs_diff_hip_vs_torch_fp32"] = float((s - st).abs().max())
    r["head_residual_max_abs_diff_hip_vs_torch_fp32_mm"] = float((e - et).abs().max())
    for name in ("head_path_cost", "head_anchor", "head_anchor_r30"):
        r[f"{name}_torch_over_hip"] = round(r[f"{name}_torch_ms"]["median"] / max(r[f"{name}_hip_ms"]["median"], 1e-6), 1)
    r["shape"], r["n_frames"], r["taps"] = list(SHAPE), FRAMES, [int(taps.shape[0]), int(wide.shape[0])]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "headset.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"bench": "headset", "device": torch.cuda.get_device_name(0), "kernels": legs(dev, args.repeats)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
