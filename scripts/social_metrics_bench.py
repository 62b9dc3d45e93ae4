#!/usr/bin/env python
"""Cost of the evaluation by interpersonal distance and mutual gaze (TEST.SOCIAL_METRICS).  Writes profiles/social_metrics.json (``--out``).

Per shape (B,K,T) = (64,20,60) and (32,32,196), same input for all legs, fp32 on the device:
  (a) social_hip_ms       ``seeme_social_metrics``, both launches, through ``social_metrics_hip``
  (b) social_torch_ms     ``social_metrics_torch`` -- what a user would otherwise write
  (c) hyp_metrics_hip_ms  ``seeme_hyp_metrics`` on the same joints, for scale
and (d) the evaluation batch on config_mld_egobody at the same (B,K,T) (fp16 weight image and fp16 VAE): one
``ego_eval(batch, num_hypotheses=K)`` plus the metric updates ``allsplit_step`` makes, with the option off -- the code of the commit
before the option existed -- and on.

Every shape is warmed up first; times are device events around work that ends in a synchronise; the legs alternate, ``--repeats``
(5) times each; min / median / max in ms."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from hyp_select_bench import alternate               # noqa: E402
from hypotheses_bench import build                   # noqa: E402

SHAPES = [(64, 20, 60), (32, 32, 196)]


def kernel_legs(shape, dev, repeats):
    from seeme_amd.hyp_metrics import hyp_metrics_hip
    from seeme_amd.social_metrics import PER_HYP, PER_SEQ, social_metrics_hip, social_metrics_torch
    B, K, T = shape
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g)
    ref = torch.cumsum(0.02 * rn(B, T, 24, 3), dim=1) + 0.3 * rn(B, 1, 24, 3)
    pred = (ref[:, None] + 0.2 * rn(B, K, 1, 1, 3) + 0.01 * rn(B, K, T, 24, 3)).to(dev)
    intr = (ref + 1.5 * rn(B, 1, 1, 3) + 0.3 * rn(B, 1, 24, 3)).to(dev)
    ref = ref.to(dev)
    qr, qi = rn(B, T, 4).to(dev), rn(B, T, 4).to(dev)
    qp = (qr[:, None] + 0.1 * rn(B, K, T, 4).to(dev)).contiguous()
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    args = (pred, ref, intr, qp, qr, qi, lens)
    r = alternate({"social_hip_ms": lambda: social_metrics_hip(*args), "social_torch_ms": lambda: social_metrics_torch(*args),
                   "hyp_metrics_hip_ms": lambda: hyp_metrics_hip(pred, ref, lens)}, repeats)
    a, b = social_metrics_hip(*args), social_metrics_torch(*args)
    r["max_rel_diff_hip_vs_torch_fp32"] = max(float(((a[n] - b[n]).abs() / b[n].abs().clamp_min(1e-30)).max()) for n in PER_SEQ + PER_HYP)
    r["hip_below_hyp_metrics"] = r["social_hip_ms"]["max"] < r["hyp_metrics_hip_ms"]["min"]
    r["shape"] = list(shape)
    return r


def eval_legs(shape, dev, repeats):
    from seeme_amd.hyp_metrics import keep_mask
    B, K, T = shape
    model, dm, cfg = build("config_mld_egobody.yaml", dev, T, 20000)
    batch = dm.batch(B, idx=1)

    def leg(on):
        def run():
            model.social_metrics = on
            rs = model.ego_eval(batch, num_hypotheses=K)
            hm = rs["hyp_metrics"]
            model.HypMetric.update(hm, "test")
            if on:
                model.SocialMetric.update(rs["social_metrics"], hm["MPJPE"], hm["ROOT_ERROR"], keep_mask(hm, "test", hm["have_quat"]))
        return run

    def reset():
        model.EgoMetric.reset(), model.HypMetric.reset(), model.SocialMetric.reset()

    with torch.no_grad():
        torch.manual_seed(1)
        r = alternate({"t_off_ms": leg(False), "t_on_ms": leg(True)}, repeats, reset)
    r["added_median_ms"] = round(r["t_on_ms"]["median"] - r["t_off_ms"]["median"], 3)
    r["off_spread_ms"] = round(r["t_off_ms"]["max"] - r["t_off_ms"]["min"], 3)
    r["config"], r["shape"] = "config_mld_egobody.yaml", [B, K, T]
    r["cluster_status"] = list(model.denoiser.cluster_status())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "social_metrics.json"))
    ap.add_argument("--skip_eval", action="store_true", help="kernel legs only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"bench": "social_metrics", "device": torch.cuda.get_device_name(0),
           "kernels": [kernel_legs(s, dev, args.repeats) for s in SHAPES]}
    if not args.skip_eval:
        res["ego_eval"] = [eval_legs(s, dev, args.repeats) for s in SHAPES]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
