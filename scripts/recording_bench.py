#!/usr/bin/env python
"""Cost of turning W windows x K hypotheses into one motion (MLD.predict_recording).  Writes profiles/recording.json (``--out``).

Shape (W,K,T,O) = (64,20,60,15): a recording of 2895 frames in the shipped window length.  Same input for a kernel and its twin,
fp32 on the device:
  (a) overlap_cost_hip_ms / overlap_cost_torch_ms     ``seeme_overlap_cost`` (both launches) / ``overlap_cost_torch``
  (b) path_select_hip_ms / path_select_torch_ms       ``seeme_path_select`` / ``path_select_torch`` (W-1 steps of torch ops)
  (c) stitch_hip_ms / stitch_torch_ms                 ``seeme_stitch_windows`` / ``stitch_windows_torch``
and (d) on config_mld_egobody (fp16 weight image and fp16 VAE, the setting of scripts/hypotheses_bench.py): predict_ms, the sampling
pass the three kernels follow (``MLD.predict`` of the W windows: encode, reverse diffusion of W*K rows, decode, SMPL joints,
seeme_hyp_pairdist), and predict_recording_ms, the whole pass; ``share_of_pass`` is the sum of the three kernel medians over the
whole pass's median.

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
from hypotheses_bench import build                    # noqa: E402

SHAPE = (64, 20, 60, 15)


def kernel_legs(dev, repeats):
    from seeme_amd import recording as R
    W, K, T, O = SHAPE
    n = (W - 1) * (T - O) + T
    g = torch.Generator().manual_seed(3)
    walk = torch.cumsum(0.02 * torch.randn(n, 24, 3, generator=g), dim=0) + 0.3 * torch.randn(1, 24, 3, generator=g)
    starts, _ = R.window_plan(n, T, O)
    jts = (torch.stack([walk[s:s + T] for s in starts])[:, None] + 0.01 * torch.randn(W, K, T, 24, 3, generator=g)).to(dev)
    feats = (0.3 * torch.randn(W, 1, 75, generator=g) + torch.cumsum(0.02 * torch.randn(W, T, 75, generator=g), dim=1)).to(dev)
    cost = R.overlap_cost_hip(jts, O)
    unary = (30.0 * torch.rand(W, K, generator=g)).to(dev)
    r = alternate({"overlap_cost_hip_ms": lambda: R.overlap_cost_hip(jts, O), "overlap_cost_torch_ms": lambda: R.overlap_cost_torch(jts, O),
                   "path_select_hip_ms": lambda: R.path_select_hip(cost, unary), "path_select_torch_ms": lambda: R.path_select_torch(cost, unary),
                   "stitch_hip_ms": lambda: R.stitch_windows_hip(feats, O, n, R.STITCH_ANGLE_TRANSL),
                   "stitch_torch_ms": lambda: R.stitch_windows_torch(feats, O, n, R.STITCH_ANGLE_TRANSL)}, repeats)
    twin = R.overlap_cost_torch(jts, O)
    r["overlap_cost_max_rel_diff_hip_vs_torch_fp32"] = float(((cost - twin).abs() / twin).max())
    a, b = R.path_select_hip(cost, unary), R.path_select_torch(cost, unary)
    r["path_equal_hip_vs_torch_fp32"] = bool(torch.equal(a["path"], b["path"]))
    r["stitch_max_abs_diff_hip_vs_torch_fp32"] = float((R.stitch_windows_hip(feats, O, n, R.STITCH_ANGLE_TRANSL)
                                                        - R.stitch_windows_torch(feats, O, n, R.STITCH_ANGLE_TRANSL)).abs().max())
    for name in ("overlap_cost", "path_select", "stitch"):
        r[f"{name}_torch_over_hip"] = round(r[f"{name}_torch_ms"]["median"] / max(r[f"{name}_hip_ms"]["median"], 1e-6), 1)
    r["shape"], r["n_frames"] = list(SHAPE), n
    return r


def pass_legs(dev, repeats, kernels):
    W, K, T, O = SHAPE
    n = (W - 1) * (T - O) + T
    model, dm, cfg = build("config_mld_egobody.yaml", dev, T, 20000)
    batch = dm.batch(W, idx=1)
    with torch.no_grad():
        torch.manual_seed(1)
        r = alternate({"predict_ms": lambda: model.predict(batch, num_hypotheses=K),
                       "predict_recording_ms": lambda: model.predict_recording(batch, n, overlap=O, num_hypotheses=K)}, repeats)
    three = sum(kernels[f"{k}_hip_ms"]["median"] for k in ("overlap_cost", "path_select", "stitch"))
    r["three_kernels_median_ms"] = round(three, 3)
    r["share_of_pass"] = round(three / r["predict_recording_ms"]["median"], 5)
    r["after_predict_median_ms"] = round(r["predict_recording_ms"]["median"] - r["predict_ms"]["median"], 3)
    r["config"], r["shape"] = "config_mld_egobody.yaml", list(SHAPE)
    r["cluster_status"] = list(model.denoiser.cluster_status())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "recording.json"))
    ap.add_argument("--skip_pass", action="store_true", help="kernel legs only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"bench": "recording", "device": torch.cuda.get_device_name(0), "kernels": kernel_legs(dev, args.repeats)}
    if not args.skip_pass:
        res["pass"] = pass_legs(dev, args.repeats, res["kernels"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
