#!/usr/bin/env python3
"""Timing of the HIP ResNet-50 backbone (csrc/resnet.hip) on one GPU, written to profiles/backbone_resnet50.json.

  * encode time at B = 32 and 64, fp32 and bf16, against the torch restatement of the same network (tests/backbone_reference.py)
    under PyTorch in fp32 NCHW -- the reference's numerics -- and, for information, in bf16 channels-last;
  * algorithmic FLOPs counted from the shapes, the share of the bf16 matrix peak, and per layer class whether the matrix peak or
    the activation traffic bounds it;
  * the captured stage-2 step of [scene, image] at B = 64 with crops in the batch against the step with pre-extracted features
    (the step as it was before the backbone existed), in the same process.

All arms run in this process, alternating, `--repeats` times after a warm-up; device events; min / median / max reported.
THE GATE: the HIP bf16 path at B = 64 is not slower than the fp32 PyTorch run (median against median).  Exit status 1 if it is.

    python scripts/backbone_bench.py [--repeats 7] [--kernel-stats <rocprofv3 kernel_stats.csv>] [--no-step]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/backbone_bench.py --encode-only
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

PEAK_BF16 = 2.5e15      # dense bf16 matrix peak, FLOP/s
PEAK_F32 = PEAK_BF16 / 16
HBM = 8.0e12            # bytes/s


def shapes_and_flops(B):
    """Per convolution: class, M, N, K, FLOPs (2 M N K) and the bytes it must move (input + output + residual + weight) in bf16."""
    from seeme_amd.resnet import BLOCKS
    rows = []

    def add(conv, cls, hin, cin, cout, k, s, res=False):
        ho = hin // s
        M, K = B * ho * ho, k * k * cin
        byts = 2 * (B * hin * hin * cin + M * cout * (2 if res else 1) + cout * K)
        rows.append({"conv": conv, "class": cls, "M": M, "N": cout, "K": K, "flops": 2.0 * M * cout * K, "bytes_bf16": byts})

    add("conv1", "stem", 224, 3, 64, 7, 2)
    H, inpl = 56, 64                                        # after the max-pool
    for li, nb in enumerate(BLOCKS):
        pl = 64 << li
        for b in range(nb):
            s = 2 if (b == 0 and li > 0) else 1
            p = f"layer{li + 1}.{b}."
            add(p + "conv1", "1x1_s1", H, inpl, pl, 1, 1)
            add(p + "conv2", f"3x3_s{s}", H, pl, pl, 3, s)
            if b == 0:
                add(p + "downsample.0", f"1x1_s{s}", H, inpl, 4 * pl, 1, s)
            H //= s
            add(p + "conv3", "1x1_s1", H, pl, 4 * pl, 1, 1, res=True)
            inpl = 4 * pl
    return rows


def timed(fn, start, end):
    start.record()
    fn()
    end.record()


def bench_arms(arms, repeats, warmup=3):
    """arms: {name: fn}.  Alternating order, every arm once per repeat; returns {name: [ms, ...]}."""
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in arms}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            timed(fn, *ev[k])
        torch.cuda.synchronize()
        for k in arms:
            out[k].append(ev[k][0].elapsed_time(ev[k][1]))
    return out


def summary(ms):
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "n": len(ms)}


def encode_section(dev, B, repeats):
    import backbone_reference as R
    from seeme_amd.resnet import ResNet50
    from seeme_amd.weights_recipe import load_backbone_recipe_
    crops = R.smooth_crops(B, seed=1).to(dev)
    x32 = R.normalise(crops)
    nets = {p: load_backbone_recipe_(ResNet50(precision=p)).to(dev) for p in ("fp32", "bf16")}
    sd32 = R.recipe_state(device=dev)
    arms = {"hip_fp32": lambda: nets["fp32"](crops), "hip_bf16": lambda: nets["bf16"](crops)}
    note = None
    try:
        with torch.no_grad():
            R.forward(sd32, x32[:2])
        arms["torch_fp32"] = lambda: R.forward(sd32, x32)
        sd16 = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sd32.items()}
        sd16 = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd16.items()}
        x16 = x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        R.forward(sd16, x16[:2])
        arms["torch_bf16_channels_last"] = lambda: R.forward(sd16, x16)
    except RuntimeError as e:          # no convolution backend for this device
        note = f"PyTorch convolutions cannot run here ({str(e).splitlines()[0][:200]}): times are ungated"
    with torch.no_grad():
        ms = bench_arms(arms, repeats)
    flops = sum(r["flops"] for r in shapes_and_flops(B))
    res = {"B": B, "algorithmic_flops": flops, "arms": {}}
    for k, v in ms.items():
        s = summary(v)
        s["tflops"] = flops / (s["median_ms"] * 1e-3) / 1e12
        if k == "hip_bf16":
            s["share_of_bf16_peak"] = s["tflops"] * 1e12 / PEAK_BF16
        if k == "hip_fp32":
            s["share_of_f32_mfma_peak"] = s["tflops"] * 1e12 / PEAK_F32
        res["arms"][k] = s
    if note:
        res["note"] = note
    return res


def class_table(B, kernel_stats):
    """FLOPs and roofline bound per convolution class; kernel times per class from a rocprofv3 --kernel-trace --stats CSV of a
    run of its own, when given (the kernel names carry <bf16, kernel size, tile>)."""
    classes = {}
    for r in shapes_and_flops(B):
        c = classes.setdefault(r["class"], {"convs": 0, "flops": 0.0, "bytes_bf16": 0.0})
        c["convs"] += 1
        c["flops"] += r["flops"]
        c["bytes_bf16"] += r["bytes_bf16"]
    for c in classes.values():
        t_mfma, t_hbm = c["flops"] / PEAK_BF16, c["bytes_bf16"] / HBM
        c["roofline_ms_bf16"] = 1e3 * max(t_mfma, t_hbm)
        c["bound"] = "activation traffic (HBM)" if t_hbm > t_mfma else "bf16 matrix peak"
    out = {"classes": classes}
    if kernel_stats and os.path.exists(kernel_stats):
        rows = []
        with open(kernel_stats) as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                if any(k in name for k in ("k_conv", "k_maxpool", "k_avgpool", "k_stem_pack")):
                    rows.append({"kernel": name, "calls": int(r.get("Calls", 0) or 0), "total_ns": float(r.get("TotalDurationNs", 0) or 0),
                                 "average_ns": float(r.get("AverageNs", 0) or 0), "percentage": float(r.get("Percentage", 0) or 0)})
        out["kernels"] = rows
    return out


def step_section(dev, repeats):
    """Captured stage-2 step, [scene, image], B = 64: crops in the static batch (backbone inside the graph) against features."""
    import backbone_reference as R  # noqa: F401
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    from seeme_amd.weights_recipe import load_recipe_
    B = 64
    replays = {}
    for name, prec, crops in (("features", "fp32", False), ("crops_fp32", "fp32", True), ("crops_bf16", "bf16", True)):
        cfg = parse_config(os.path.join(REPO, "configs", "config_mld_image_scene_backbone.yaml"))
        cfg.TRAIN.IMAGE_PRECISION = prec
        dm = SyntheticEgoDataModule(nfeats=cfg.model.nfeats, T=60, n_points=20000, device=dev, pose_dim=cfg.model.nfeats - 3)
        torch.manual_seed(7)
        model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
        load_recipe_(model.vae), load_recipe_(model.denoiser), load_recipe_(model.proscene)
        model = model.to(dev).train()
        batch = list(dm.batch(B, idx=1, with_scene=True, with_image="crops"))
        if not crops:
            batch[5] = model.proscene.backbone(batch[5])
        model.configure_optimizers()
        replays[name] = model.capture_training_step(tuple(batch), warmup=2)
    ms = bench_arms({k: (lambda r=r: r()) for k, r in replays.items()}, repeats)
    out = {"B": B, "arms": {k: summary(v) for k, v in ms.items()}}
    base = out["arms"]["features"]["median_ms"]
    for k in ("crops_fp32", "crops_bf16"):
        out["arms"][k]["over_features_ms"] = out["arms"][k]["median_ms"] - base
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--encode-only", action="store_true", help="5 encodes per precision at B = 64 and nothing else: the program to put under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "backbone_resnet50.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and torch.cuda.is_available()
    dev = torch.device("cuda:0")
    if a.encode_only:
        import backbone_reference as R
        from seeme_amd.resnet import ResNet50
        from seeme_amd.weights_recipe import load_backbone_recipe_
        crops = R.smooth_crops(64, seed=1).to(dev)
        for p in ("bf16", "fp32"):
            net = load_backbone_recipe_(ResNet50(precision=p)).to(dev)
            for _ in range(5):
                net(crops)
            torch.cuda.synchronize()
        return 0
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "peaks": {"bf16_flops": PEAK_BF16, "f32_mfma_flops": PEAK_F32, "hbm_bytes_per_s": HBM},
           "encode": [encode_section(dev, B, a.repeats) for B in (32, 64)], "per_class_B64": class_table(64, a.kernel_stats)}
    if not a.no_step:
        res["stage2_step_B64"] = step_section(dev, a.repeats)
    arms = res["encode"][1]["arms"]
    if "torch_fp32" in arms:
        res["gate"] = {"rule": "HIP bf16 at B = 64 not slower than the fp32 PyTorch restatement (medians)",
                       "hip_bf16_ms": arms["hip_bf16"]["median_ms"], "torch_fp32_ms": arms["torch_fp32"]["median_ms"],
                       "pass": arms["hip_bf16"]["median_ms"] <= arms["torch_fp32"]["median_ms"]}
    else:
        res["gate"] = {"rule": "ungated: the PyTorch convolutions could not run", "pass": None}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"encode_B64": {k: round(v["median_ms"], 3) for k, v in arms.items()}, "gate": res["gate"],
                      "step": {k: round(v["median_ms"], 3) for k, v in res.get("stage2_step_B64", {}).get("arms", {}).items()}}))
    return 0 if res["gate"]["pass"] in (True, None) else 1


if __name__ == "__main__":
    sys.exit(main())
