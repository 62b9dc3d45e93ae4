#!/usr/bin/env python
"""Times the collision ratio (share of the scene cloud inside the body, per hypothesis) and its kernel.  One JSON line.

The body is a synthetic SMPL whose v_template is uv_sphere(84, 82) scaled to (0.25, 0.6, 0.15) m, with the sphere's face table (SMPL's
6890 vertices and 13 776 faces); poses are random.  A tenth of every cloud lies within (0.5, 0.9, 0.5) m of the origin, where the
bodies are; the rest is room-wide.

  driver_on_ms / driver_off_ms   ``MLD._mesh_metrics`` at B = 32, K = 20, T = 60, P = 20 000 with TEST.MESH_METRICS on, with and
                                 without TEST.COLLISION_METRICS: the same posed chunks, so the difference is the feature's cost.
  driver_alone_ms                TEST.COLLISION_METRICS alone.
  count_ms                       ``seeme_scene_inside_count`` alone on ``--count_frames`` resident frames (both launches, by device
                                 events), the candidates per frame (points inside the frame's bounding box) and the (point, face)
                                 pairs per second = candidates * faces / time.
  twin_ms                        ``scene_inside_count_torch`` in fp32 on the same device on ``--twin_frames`` of those frames, and the
                                 per-frame ratio to the kernel.

Every shape is warmed up first; times are device events around work that ends in a synchronise; min / median / max in ms."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hypotheses", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--count_frames", type=int, default=2048)
    ap.add_argument("--twin_frames", type=int, default=8)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "collision_metrics.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    from seeme_amd.config import parse_config
    from seeme_amd.mesh_metrics import scene_inside_count_hip, scene_inside_count_torch, uv_sphere
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL, synthetic_model_arrays
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_scene.yaml"))
    cfg.TEST.MESH_METRICS = True
    cfg.TEST.COLLISION_METRICS = True
    B, K, T, P = args.batch, args.hypotheses, args.frames, args.points
    sv, sf = uv_sphere(84, 82)
    arrays = synthetic_model_arrays(1234)
    arrays["v_template"] = (sv * torch.tensor([0.25, 0.6, 0.15], dtype=torch.float64)).float().numpy()
    arrays["faces"] = sf.numpy()
    dm = SyntheticEgoDataModule(nfeats=75, T=T, n_points=P, device=dev)
    model = MLD(cfg, dm, smpl_model=SMPL(model_arrays=arrays)).to(dev).eval()
    V, NF = int(model.smpl_model.v_template.shape[0]), int(model.smpl_model.faces_tensor.shape[0])
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    f_rst, f_ref, betas = 0.3 * rn(B * K, T, model.nfeats), 0.3 * rn(B, T, model.nfeats), 0.5 * rn(B, 1, 10).expand(B, T, 10).contiguous()
    near = (torch.rand(B, P // 10, 3, generator=g) * 2 - 1) * torch.tensor([0.5, 0.9, 0.5])
    scene = torch.cat([torch.rand(B, P - P // 10, 3, generator=g) * 6 - 3, near], dim=1)
    scene = scene[:, torch.randperm(P, generator=g)].contiguous().to(dev)
    lengths = [T] * B
    res = {"bench": "collision_metrics", "B": B, "K": K, "T": T, "P": P, "V": V, "NF": NF, "chunk_mb": model.mesh_chunk_mb}
    with torch.no_grad():
        runs = {"driver_off_ms": lambda: model._mesh_metrics(f_rst, f_ref, betas, None, lengths, K, scene),
                "driver_on_ms": lambda: model._mesh_metrics(f_rst, f_ref, betas, None, lengths, K, scene, mesh=True, collision=True),
                "driver_alone_ms": lambda: model._collision_metrics(f_rst, f_ref, betas, None, lengths, K, scene)}
        for name, run in runs.items():
            out = run()
            res[name] = stats([timed(run) for _ in range(args.repeats)])
        res["driver_feature_cost_ms"] = round(res["driver_on_ms"]["min"] - res["driver_off_ms"]["min"], 3)
        res["driver_result_means"] = {n: round(float(v.mean()), 6) for n, v in out.items()}
        # the counting kernel alone on resident meshes
        n = args.count_frames
        _, verts = model._feats_to_joints(0.3 * rn(1, n, model.nfeats), 0.5 * rn(1, n, 10), True)
        verts = verts[0].contiguous()
        sof = (torch.arange(n) % B).to(torch.int32).to(dev)
        faces = model.smpl_model.faces_tensor
        lo, hi = verts.min(dim=1).values, verts.max(dim=1).values
        cand = torch.stack([((scene[int(sof[i])] >= lo[i]) & (scene[int(sof[i])] <= hi[i])).all(dim=1).sum() for i in range(n)])
        hip = lambda: scene_inside_count_hip(verts, faces, scene, sof)
        c_hip = hip()
        t = [timed(hip) for _ in range(args.repeats)]
        res["count_frames"] = n
        res["count_ms"] = stats(t)
        res["candidates_per_frame"] = {"mean": round(float(cand.float().mean()), 1), "min": int(cand.min()), "max": int(cand.max())}
        res["inside_per_frame_mean"] = round(float(c_hip.float().mean()), 1)
        res["pairs_per_s"] = float(cand.sum()) * NF / (min(t) * 1e-3)
        m = args.twin_frames
        twin = lambda: scene_inside_count_torch(verts[:m], faces, scene, sof[:m])
        c_twin = twin()
        t2 = [timed(twin) for _ in range(args.repeats)]
        res["twin_frames"] = m
        res["twin_ms"] = stats(t2)
        res["kernel_speedup_over_twin_per_frame"] = round((min(t2) / m) / (min(t) / n), 2)
        res["counts_differing_from_twin_fp32"] = int((c_hip[:m] != c_twin).sum())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
