#!/usr/bin/env python
"""Cost of the head-rotation kernel per layout, beside its plain-torch twin and beside the head-path kernel at the same size.  Writes
profiles/head_rot.json (``--out``).

Shape: (W,K,T) = (32,20,196), a recording of about 4700 frames at an overlap of 49, with 20 hypotheses per window; the last window
is half full.  Same input for the kernel and its twin, fp32 on the device:
  (a) head_rot_cost_<F>_hip_ms / head_rot_cost_<F>_torch_ms   ``seeme_head_rot_cost`` with cost and angle (the launch alone: lengths on
                                                              the device already) / ``head_rot_cost_torch``, for F = 72
                                                              (STITCH_ANGLE), 75 (STITCH_ANGLE_TRANSL) and 144 (STITCH_ROT6D)
  (b) head_path_cost_hip_ms                                   ``seeme_head_path_cost`` at the same W, K, T, for scale
No time is gated.

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
WIDTHS = (72, 75, 144)


def _inputs(F, dev, g):
    """Chain joints that turn by about 0.4 rad each, hypotheses 0.03 rad of noise apart; the device follows the base's head up to a
    mount rotation and 10 degrees of noise (the inputs of tests/head_rot_reference.py, drawn with torch)."""
    from seeme_amd import recording as R
    W, K, T = SHAPE
    nj = 24 if F == 144 else F // 3
    base = (0.4 / 3 ** 0.5) * torch.randn(W, 1, T, nj, 3, generator=g)
    aa = base + 0.03 * torch.randn(W, K, T, nj, 3, generator=g)
    h = None
    for j in range(0, R.HEAD_JOINT + 1, 3):
        q = R._aa_to_quat(base[:, 0, :, j])
        h = q if h is None else R._quat_mul(h, q)
    mount = R._aa_to_quat(torch.tensor([1.1, -0.7, 2.0]))
    dq = R._quat_mul(R._quat_mul(h, mount.expand_as(h)), R._aa_to_quat(0.1745 * torch.randn(W, T, 3, generator=g)))
    feats = R._quat_to_rot6d(R._aa_to_quat(aa)).reshape(W, K, T, 144) if F == 144 else aa.reshape(W, K, T, F)
    return feats.contiguous().to(dev), dq.contiguous().to(dev)


def legs(dev, repeats):
    from seeme_amd import recording as R
    W, K, T = SHAPE
    g = torch.Generator().manual_seed(5)
    lengths = [T] * (W - 1) + [T // 2]
    len32 = torch.tensor(lengths, dtype=torch.int32, device=dev)
    layouts = {72: R.STITCH_ANGLE, 75: R.STITCH_ANGLE_TRANSL, 144: R.STITCH_ROT6D}
    data = {F: _inputs(F, dev, g) for F in WIDTHS}
    jts = torch.randn(W, K, T, 24, 3, generator=g).to(dev)
    path = torch.randn(W, T, 3, generator=g).to(dev)
    todo = {"head_path_cost_hip_ms": lambda: R._launch_head_cost(jts, path, len32, W, K, T)}
    for F in WIDTHS:
        feats, dq = data[F]
        todo[f"head_rot_cost_{F}_hip_ms"] = lambda feats=feats, dq=dq, F=F: R._launch_head_rot_cost(feats, layouts[F], F, dq, len32, W, K, T)
        todo[f"head_rot_cost_{F}_torch_ms"] = lambda feats=feats, dq=dq, F=F: R.head_rot_cost_torch(feats, layouts[F], dq, len32)
    r = alternate(todo, repeats)
    for F in WIDTHS:
        feats, dq = data[F]
        a, b = R.head_rot_cost_hip(feats, layouts[F], dq, lengths), R.head_rot_cost_torch(feats.double(), layouts[F], dq.double(), lengths)
        r[f"head_rot_cost_{F}_max_rel_diff_hip_vs_float64"] = float(((a["cost"] - b["cost"]).abs() / b["cost"]).max())
        r[f"head_rot_angle_{F}_max_abs_diff_hip_vs_float64_deg"] = float((a["angle"] - b["angle"]).abs().max())
        r[f"head_rot_cost_{F}_torch_over_hip"] = round(r[f"head_rot_cost_{F}_torch_ms"]["median"] / max(r[f"head_rot_cost_{F}_hip_ms"]["median"], 1e-6), 1)
    r["shape"], r["lengths"] = list(SHAPE), [T, T // 2]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "head_rot.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"bench": "head_rot", "device": torch.cuda.get_device_name(0), "kernels": legs(dev, args.repeats)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
