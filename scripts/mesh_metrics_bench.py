#!/usr/bin/env python
"""Times the mesh-metric driver (PA-MPJPE, V2V, body-scene distance per hypothesis) and its hot kernel.  One JSON line.

  driver_ms      ``MLD._mesh_metrics`` at B = 32, K = 20, T = 60, P = 20 000 on random poses (config_mld_scene, synthetic SMPL with
                 6890 vertices): posing in chunks of TEST.MESH_CHUNK_MB, the three kernels, the per-frame floats.
  scene_ms       ``seeme_scene_min_dist2`` alone on ``--scene_frames`` resident frames (both launches, by device events), its
                 pairs/s = frames * V * P / time, and the ratio to the MFMA issue bound: v_mfma_f32_16x16x4_f32 covers 256 pairs and
                 issues every 32 cycles per SIMD = 8 pairs per clock per SIMD; 1024 SIMDs at 2.4 GHz give 1.97e13 pairs/s.
  twin_ms        the plain-torch twin in fp32 on the same device on ``--twin_frames`` of those frames -- what a user could do today
                 without copying the meshes to the host -- and the per-frame ratio to the kernel.

Every shape is warmed up first; times are device events around work that ends in a synchronise; min / median / max in ms."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MFMA_BOUND_PAIRS_PER_S = 8 * 1024 * 2.4e9


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hypotheses", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scene_frames", type=int, default=2048)
    ap.add_argument("--twin_frames", type=int, default=8)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    from seeme_amd.config import parse_config
    from seeme_amd.mesh_metrics import scene_min_dist2_hip, scene_min_dist2_torch
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_scene.yaml"))
    cfg.TEST.MESH_METRICS = True
    B, K, T, P = args.batch, args.hypotheses, args.frames, args.points
    dm = SyntheticEgoDataModule(nfeats=75, T=T, n_points=P, device=dev)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234)).to(dev).eval()
    V = int(model.smpl_model.v_template.shape[0])
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    f_rst, f_ref, betas = 0.3 * rn(B * K, T, model.nfeats), 0.3 * rn(B, T, model.nfeats), 0.5 * rn(B, 1, 10).expand(B, T, 10).contiguous()
    scene = (torch.rand(B, P, 3, generator=g) * 6 - 3).to(dev)
    lengths = [T] * B
    res = {"bench": "mesh_metrics", "B": B, "K": K, "T": T, "P": P, "V": V, "chunk_mb": model.mesh_chunk_mb}
    with torch.no_grad():
        run = lambda: model._mesh_metrics(f_rst, f_ref, betas, None, lengths, K, scene)
        out = run()
        t = [timed(run) for _ in range(args.repeats)]
        pairs = float(B * K * T + B * T) * V * P
        res["driver_ms"] = stats(t)
        res["driver_pairs_per_s"] = pairs / (min(t) * 1e-3)
        res["driver_ratio_to_mfma_bound"] = round(res["driver_pairs_per_s"] / MFMA_BOUND_PAIRS_PER_S, 4)
        res["driver_result_means"] = {n: round(float(v.mean()), 4) for n, v in out.items()}
        # the hot kernel alone on resident meshes
        n = args.scene_frames
        feats = 0.3 * rn(1, n, model.nfeats)
        _, verts = model._feats_to_joints(feats, 0.5 * rn(1, n, 10), True)
        verts = verts[0].contiguous()
        sof = (torch.arange(n) % B).to(torch.int32).to(dev)
        hip = lambda: scene_min_dist2_hip(verts, scene, sof)
        d_hip = hip()
        t = [timed(hip) for _ in range(args.repeats)]
        res["scene_frames"] = n
        res["scene_ms"] = stats(t)
        res["scene_pairs_per_s"] = float(n) * V * P / (min(t) * 1e-3)
        res["scene_ratio_to_mfma_bound"] = round(res["scene_pairs_per_s"] / MFMA_BOUND_PAIRS_PER_S, 4)
        m = args.twin_frames
        twin = lambda: scene_min_dist2_torch(verts[:m], scene, sof[:m])
        d_twin = twin()
        t2 = [timed(twin) for _ in range(args.repeats)]
        res["twin_frames"] = m
        res["twin_ms"] = stats(t2)
        res["kernel_speedup_over_twin_per_frame"] = round((min(t2) / m) / (min(t) / n), 2)
        res["max_rel_diff_hip_vs_twin_fp32"] = float(((d_hip[:m] - d_twin).abs() / d_twin).max())
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
