#!/usr/bin/env python
"""K hypotheses per sequence in one evaluation pass against K passes of today's evaluation.  One JSON line.

  t_K    one ``ego_eval(batch, num_hypotheses=K)`` plus the HypothesisMetrics update (condition encoded once);
  t_1xK  K consecutive ``ego_eval(batch)`` calls, each with the EgoMetric update -- what TEST.REPLICATION_TIMES costs per batch.
         This leg uses only what exists without the feature: run this same file from a checkout of the parent commit
         (``--legs 1xk``) for the baseline.

config_mld_egobody (B = 32, T = 196) and config_mld_scene (B = 32, 20 000 points), fp16 weight image and fp16 VAE, K = 20, seeded
synthetic batches, recipe weights.  Every shape is warmed up first; times are device events around work that ends in a
synchronise; the legs alternate, ``--repeats`` times each; min / median / max in ms.

``--kernel`` times the metric kernel alone at (B, K, T) beside its torch twin on the device in fp32 (same input), with the kernel's
algorithmic bytes (B*K + B) * T * 288 over its time."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "n": len(v)}


def build(cfg_name, dev, T, points):
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    from seeme_amd.weights_recipe import load_recipe_
    cfg = parse_config(os.path.join(REPO, "configs", cfg_name))
    dm = SyntheticEgoDataModule(nfeats=75, T=T, n_points=points, device=dev)
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser)
    if hasattr(model, "proscene"):
        load_recipe_(model.proscene.scene_enc)
    model = model.to(dev).eval()
    model.denoiser.weight_dtype, model.vae.precision = "fp16", "fp16"
    return model, dm, cfg


def eval_legs(args, dev):
    out = {}
    for cfg_name in args.configs:
        model, dm, cfg = build(cfg_name, dev, args.frames, args.points)
        batch = dm.batch(args.batch, idx=1, with_scene="scene" in cfg.model.condition)
        K = args.hypotheses
        have_k = hasattr(model, "HypMetric")

        def leg_k():
            rs = model.ego_eval(batch, num_hypotheses=K)
            model.HypMetric.update(rs["hyp_metrics"], "test")

        def leg_1xk():
            for _ in range(K):
                rs = model.ego_eval(batch)
                model.EgoMetric.update(rs["joints_rst"], rs["joints_ref"], rs["lengths"], rs.get("orientation_quat_rst"),
                                       rs.get("orientation_quat_ref"), split="test")

        legs = {}
        if "k" in args.legs and have_k:
            legs["t_K_ms"] = leg_k
        if "1xk" in args.legs:
            legs["t_1xK_ms"] = leg_1xk
        times = {n: [] for n in legs}
        with torch.no_grad():
            torch.manual_seed(1)
            for fn in legs.values():                 # warm-up of every shape: weight images, tables, workspaces, cluster plan
                fn(), fn()
            for _ in range(args.repeats):            # alternating
                for n, fn in legs.items():
                    model.EgoMetric.reset()
                    if have_k:
                        model.HypMetric.reset()
                    times[n].append(timed(fn))
        r = {n: stats(v) for n, v in times.items()}
        if have_k and "k" in args.legs:              # what one such pass reports (recipe weights: nothing is inside the 'test' bounds)
            model.HypMetric.reset()
            with torch.no_grad():
                leg_k()
            r["hyp"] = {k: round(v, 4) for k, v in model.HypMetric.compute().items()}
        r["cluster_status"] = list(model.denoiser.cluster_status())
        out[cfg_name] = r
    return out


def kernel_leg(args, dev):
    from seeme_amd.hyp_metrics import hyp_metrics_hip, hyp_metrics_torch
    B, K, T = args.batch, args.hypotheses, args.frames
    g = torch.Generator().manual_seed(3)
    ref = (torch.cumsum(0.02 * torch.randn(B, T, 24, 3, generator=g), dim=1) + 0.3 * torch.randn(B, 1, 24, 3, generator=g)).to(dev)
    pred = (ref[:, None].cpu() + 0.01 * torch.randn(B, K, T, 24, 3, generator=g)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    hip = lambda: hyp_metrics_hip(pred, ref, lens)
    twin = lambda: hyp_metrics_torch(pred, ref, lens)
    hip(), twin()
    n_hip = 1 if args.once else 20
    t_hip = [timed(hip) for _ in range(n_hip)]
    t_twin = [timed(twin) for _ in range(1 if args.once else 5)]
    a, b = hip(), twin()
    err = max(float(((a[n] - b[n]).abs() / b[n].abs().clamp_min(1e-30)).max()) for n in a)
    nbytes = (B * K + B) * T * 288
    return {"shape": [B, K, T], "hip_call_ms": stats(t_hip), "torch_twin_fp32_ms": stats(t_twin), "algorithmic_bytes": nbytes,
            "GBps_at_min_call": round(nbytes / (min(t_hip) * 1e-3) / 1e9, 1), "max_rel_diff_hip_vs_twin_fp32": err,
            "note": "hip_call_ms is both launches plus the host call, by device events; the kernel's own time comes from a kernel trace"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["config_mld_egobody.yaml", "config_mld_scene.yaml"])
    ap.add_argument("--legs", nargs="+", default=["k", "1xk"], choices=["k", "1xk"])
    ap.add_argument("--hypotheses", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=196)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel", action="store_true", help="time the metric kernel and its torch twin instead of the evaluation legs")
    ap.add_argument("--once", action="store_true", help="--kernel: one timed call each (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"bench": "hypotheses", "K": args.hypotheses, "B": args.batch, "T": args.frames, "points": args.points}
    res["results"] = kernel_leg(args, dev) if args.kernel else eval_legs(args, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
