#!/usr/bin/env python
"""Cost of the label-free choice among K hypotheses (TEST.HYP_SELECT medoid).  Writes profiles/hyp_select.json (``--out``).

Per shape (B,K,T) = (32,20,196) and (32,32,196), same input for all three, fp32 on the device:
  (a) pairdist_hip_ms     ``seeme_hyp_pairdist``, both launches, through ``hyp_pairdist_hip``
  (b) pairdist_torch_ms   ``hyp_pairdist_torch`` -- what a user would otherwise write
  (c) hyp_metrics_hip_ms  ``seeme_hyp_metrics`` for scale: the same pair work plus the error work
and (d) the ``t_K`` leg of scripts/hypotheses_bench.py on config_mld_egobody (B = 32, T = 196, K = 20, fp16 weight image and fp16 VAE):
one ``ego_eval(batch, num_hypotheses=K)`` plus the metric updates, with ``hyp_select`` 'medoid' and 'first'.  'first' runs the code
of the commit before the selection existed; the same leg from a checkout of that commit is
``scripts/hypotheses_bench.py --legs k --configs config_mld_egobody.yaml``.

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

from hypotheses_bench import build, stats, timed      # noqa: E402

SHAPES = [(32, 20, 196), (32, 32, 196)]


def alternate(legs, repeats, before=None):
    for fn in legs.values():
        fn(), fn()
    times = {n: [] for n in legs}
    for _ in range(repeats):
        for n, fn in legs.items():
            if before:
                before()
            times[n].append(timed(fn))
    return {n: stats(v) for n, v in times.items()}


def kernel_legs(shape, dev, repeats):
    from seeme_amd.hyp_metrics import hyp_metrics_hip, hyp_pairdist_hip, hyp_pairdist_torch
    B, K, T = shape
    g = torch.Generator().manual_seed(3)
    ref = torch.cumsum(0.02 * torch.randn(B, T, 24, 3, generator=g), dim=1) + 0.3 * torch.randn(B, 1, 24, 3, generator=g)
    pred = (ref[:, None] + 0.01 * torch.randn(B, K, T, 24, 3, generator=g)).to(dev)
    ref = ref.to(dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    r = alternate({"pairdist_hip_ms": lambda: hyp_pairdist_hip(pred, lens), "pairdist_torch_ms": lambda: hyp_pairdist_torch(pred, lens),
                   "hyp_metrics_hip_ms": lambda: hyp_metrics_hip(pred, ref, lens)}, repeats)
    a, b = hyp_pairdist_hip(pred, lens), hyp_pairdist_torch(pred, lens)
    off = ~torch.eye(K, dtype=torch.bool, device=dev)
    r["max_rel_diff_hip_vs_torch_fp32"] = float(((a["PAIR_DIST"] - b["PAIR_DIST"]).abs()[:, off] / b["PAIR_DIST"][:, off]).max())
    r["hip_below_torch"] = r["pairdist_hip_ms"]["max"] < r["pairdist_torch_ms"]["min"]
    r["shape"] = list(shape)
    return r


def eval_legs(dev, repeats, B=32, K=20, T=196):
    model, dm, cfg = build("config_mld_egobody.yaml", dev, T, 20000)
    batch = dm.batch(B, idx=1)

    def leg(select):
        def run():
            rs = model.ego_eval(batch, num_hypotheses=K, hyp_select=select)
            model.HypMetric.update(rs["hyp_metrics"], "test")
            if select == "medoid":
                model.SelMetric.update(rs["hyp_metrics"], "test")
        return run

    def reset():
        model.EgoMetric.reset(), model.HypMetric.reset(), model.SelMetric.reset()

    with torch.no_grad():
        torch.manual_seed(1)
        r = alternate({"t_K_first_ms": leg("first"), "t_K_medoid_ms": leg("medoid")}, repeats, reset)
    r["added_median_ms"] = round(r["t_K_medoid_ms"]["median"] - r["t_K_first_ms"]["median"], 3)
    r["first_spread_ms"] = round(r["t_K_first_ms"]["max"] - r["t_K_first_ms"]["min"], 3)
    r["config"], r["shape"] = "config_mld_egobody.yaml", [B, K, T]
    r["cluster_status"] = list(model.denoiser.cluster_status())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "hyp_select.json"))
    ap.add_argument("--skip_eval", action="store_true", help="kernel legs only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"bench": "hyp_select", "device": torch.cuda.get_device_name(0), "kernels": [kernel_legs(s, dev, args.repeats) for s in SHAPES]}
    if not args.skip_eval:
        res["ego_eval"] = eval_legs(dev, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
