#!/usr/bin/env python3
"""Timing of the ProHMR-scene pose head (csrc/flow_head.hip) on one GPU, written to profiles/flow_head.json.  Nothing is gated.

  * seeme_flow_head at L in {64, 600} x S in {1, 4}: ms per call and per launch (three launches), and the share of the fp32 matrix
    peak from the EXECUTED FLOPs (padded rows and columns included);
  * the same folded chain through PyTorch-ROCm on the same card, for information;
  * one estimate.py-shaped pass at L = 600, P = 20 000 in chunks of 64 frames, split into crop, ResNet-50, scene views, PointNet,
    head and host: where a user's wait goes.

Device events around every arm, a warm-up, then `--repeats` (>= 5) passes with the arms alternating; min / median / max reported.

    python scripts/flow_head_bench.py [--repeats 7] [--no-pass]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_F32 = 157.3e12     # fp32-input MFMA peak, FLOP/s
LAUNCHES = 3


def executed_flops(L, S):
    """What the three kernels issue: the context GEMM on 32-row tiles and K padded to 2576; the chain on 16-row tiles with the
    initial layer's K padded to 80, the final layer on 96 columns, the 144 x 144 LU; the 13 x 1024 camera / betas rows."""
    from seeme_amd import prohmr_head as PH
    ctx_rows = -(-L // 32) * 32
    rows = -(-(L * S) // PH.TILE_ROWS) * PH.TILE_ROWS
    per_row_layer = 80 * 1024 + 4 * 1024 * 1024 + 1024 * 96 + 144 * 144
    return 2.0 * (ctx_rows * PH.CTX_PAD * 5120 + rows * 4 * per_row_layer + L * 13 * 1024)


def folded_chain_torch(f, ctx, z):
    """The definition of seeme_flow_head (include/seeme_hip.h) on fold()'s tensors, in their dtype on their device."""
    L, S, _ = z.shape
    x = z.reshape(L * S, 144).clone()
    C = torch.addmm(f["ctx_b"], ctx, f["ctx_w"].t())
    Cr = C.repeat_interleave(S, dim=0)
    for k in range(3, -1, -1):
        par = (f["id_parity"] >> k) & 1
        h = x[:, par::2] @ f["id_w"][k].t() + Cr[:, 1024 * k:1024 * (k + 1)]
        for b in range(2):
            u = torch.relu(h * f["bn_s"][k, 2 * b] + f["bn_o"][k, 2 * b]) @ f["lin_w"][k, 2 * b].t()
            u = torch.relu(u * f["bn_s"][k, 2 * b + 1] + f["bn_o"][k, 2 * b + 1]) @ f["lin_w"][k, 2 * b + 1].t()
            h = h + u + f["res_b"][k, b]
        x[:, 1 - par::2] -= h @ f["fin_w"][k].t() + f["fin_b"][k]
        x = (x @ f["lu_w"][k].t()) * f["act_s"][k] + f["act_o"][k]
    off = torch.relu(C[:, 4096:]) @ f["fc_w"].t() + f["fc_b"]
    return x.reshape(L, S, 144), off, -0.5 * (z * z).sum(-1) + f["log_const"]


def bench_arms(arms, repeats, warmup=3):
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in arms}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            ev[k][0].record()
            fn()
            ev[k][1].record()
        torch.cuda.synchronize()
        for k in arms:
            out[k].append(ev[k][0].elapsed_time(ev[k][1]))
    return out


def summary(ms):
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "n": len(ms)}


def head_section(dev, repeats):
    from seeme_amd import prohmr_head as PH
    from seeme_amd.weights_recipe import load_flow_head_recipe_
    head = load_flow_head_recipe_(PH.SMPLFlowHead()).to(dev)
    f32 = {k: (v.float().to(dev) if torch.is_tensor(v) else v) for k, v in PH.fold(head).items()}
    g = torch.Generator().manual_seed(0)
    out = []
    for L in (64, 600):
        for S in (1, 4):
            ctx = torch.cat([torch.rand(L, 6, generator=g), 0.5 * torch.randn(L, 2048, generator=g).abs(), 0.5 * torch.randn(L, 512, generator=g)], dim=1).to(dev)
            z = PH.draw_z(L, S, g, dev)
            got, ref = PH.flow_head_hip(head, ctx, z), folded_chain_torch(f32, ctx, z)
            err = float((got[0] - ref[0]).abs().max() / ref[0].abs().max())
            with torch.no_grad():
                ms = bench_arms({"hip": lambda: PH.flow_head_hip(head, ctx, z), "torch_folded_fp32": lambda: folded_chain_torch(f32, ctx, z)}, repeats)
            fl = executed_flops(L, S)
            row = {"L": L, "S": S, "rows": L * S, "executed_flops": fl, "hip_vs_torch_pose6d_rel": err, "arms": {k: summary(v) for k, v in ms.items()}}
            hip = row["arms"]["hip"]
            hip["ms_per_launch"] = hip["median_ms"] / LAUNCHES
            hip["tflops_executed"] = fl / (hip["median_ms"] * 1e-3) / 1e12
            hip["share_of_f32_mfma_peak"] = hip["tflops_executed"] * 1e12 / PEAK_F32
            out.append(row)
    return out


def pass_section(dev, repeats, L=600, P=20000, chunk=64, H=480, W=640):
    """The loop of cli.estimate_main on synthetic input, every stage between its own pair of events."""
    from seeme_amd import crops as CR, geometry as G, prohmr_head as PH, recording as R
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    from seeme_amd.weights_recipe import load_recipe_
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_interactee_head.yaml"))
    dm = SyntheticEgoDataModule(nfeats=cfg.model.nfeats, T=16, n_points=256, device=dev, pose_dim=cfg.model.nfeats - 3)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.proscene)
    model = model.to(dev).eval()
    g = np.random.default_rng(0)
    video = torch.randint(0, 256, (chunk, H, W, 3), dtype=torch.uint8, device=dev)                # one chunk of frames, reused
    center = np.stack([g.uniform(200, 440, L), g.uniform(150, 330, L)], axis=1).astype(np.float32)
    scale = g.uniform(0.8, 1.6, L).astype(np.float32)
    intr = np.tile(np.array([500.0, 320.0, 240.0], np.float32), (L, 1))
    verts = torch.from_numpy((g.normal(size=(200000, 3)) * [3.0, 1.5, 3.0]).astype(np.float32)).to(dev)
    w2c = np.tile(np.eye(4), (L, 1, 1))
    view = R.opencv_views(w2c, model.interactee_camera_axes)
    z = PH.draw_z(L, 1, None, dev)
    stages = ("crop", "resnet50", "scene_views", "pointnet", "head", "host")

    def one_pass():
        marks = []
        mark = lambda: marks.append(torch.cuda.Event(enable_timing=True)) or marks[-1].record()
        rot, cam = [], []
        for lo in range(0, L, chunk):
            hi = min(L, lo + chunk)
            n = hi - lo
            mark()
            patches = CR.crop_patches_hip(video[:n], np.arange(n), PH.head_box(center[lo:hi], scale[lo:hi]))
            mark()
            img = model.proscene.encode_image(patches)
            mark()
            sv = R.scene_views_hip(verts, torch.from_numpy(view[lo:hi]).float().to(dev), P)
            mark()
            sc = model.proscene.encode_scene(sv["cloud"])
            mark()
            out = model.estimate_interactee(img, sc, center[lo:hi], scale[lo:hi], intr[lo:hi], z=z[lo:hi])
            mark()
            rot.append(out["rotmat"]), cam.append(out["transl"])
        mark()
        aa = G.rotmat_to_aa_torch(torch.cat(rot).double()).reshape(L, 1, 72)
        J0 = torch.zeros(3, dtype=torch.float64, device=dev)
        R.camera_body_to_world(aa[:, :, :3], torch.cat(cam).double()[:, None], J0, w2c, model.interactee_camera_axes)
        mark()
        torch.cuda.synchronize()
        t = dict.fromkeys(stages, 0.0)
        per = 6                                                          # marks per chunk; the host stage is the last pair
        nchunks = (len(marks) - 2) // per
        for c in range(nchunks):
            for i, name in enumerate(stages[:5]):
                t[name] += marks[c * per + i].elapsed_time(marks[c * per + i + 1])
        t["host"] = marks[-2].elapsed_time(marks[-1])
        t["total"] = marks[0].elapsed_time(marks[-1])
        return t

    with torch.no_grad():
        for _ in range(2):
            one_pass()
        runs = [one_pass() for _ in range(repeats)]
    return {"L": L, "P": P, "chunk_frames": chunk, "frame": [H, W], "scene_vertices": int(verts.shape[0]),
            "scene_precision": model.proscene.scene_enc.precision, "image_precision": model.proscene.backbone.precision,
            "stages_ms": {k: summary([r[k] for r in runs]) for k in stages + ("total",)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-pass", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flow_head.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and torch.cuda.is_available()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "f32_mfma_peak_flops": PEAK_F32, "launches_per_call": LAUNCHES,
           "head": head_section(dev, a.repeats)}
    if not a.no_pass:
        res["estimate_pass"] = pass_section(dev, a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"head": [{"L": r["L"], "S": r["S"], **{k: round(v["median_ms"], 3) for k, v in r["arms"].items()},
                                "peak_share": round(r["arms"]["hip"]["share_of_f32_mfma_peak"], 3)} for r in res["head"]],
                      "pass_ms": {k: round(v["median_ms"], 2) for k, v in res.get("estimate_pass", {}).get("stages_ms", {}).items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
