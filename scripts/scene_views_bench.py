#!/usr/bin/env python
"""Cost of selecting every window's scene view from the scene's vertices (recording.scene_views_hip).  Writes
profiles/scene_views.json (``--out``).

Shape (W,N,P) = (64, 1 000 000, 20 000): the windows of scripts/recording_bench.py over a scene mesh of a million vertices, EgoBody's
table size.  The camera walks through a 10 x 10 x 3 m room and turns once around; the same fp32 input for every leg:
  (a) scene_views_hip_ms      ``seeme_scene_views`` (three launches) through ``scene_views_hip``
  (b) scene_views_torch_ms    ``scene_views_torch`` in fp32 on the same device
  (c) scene_views_numpy_ms    the per-window host loop a user would otherwise write (mask, [::k], [:P]), float32
``floor_ms`` is the kernel's traffic, 2 x ceil(W / windows-per-pass) x 12 N bytes read + 16 W P bytes written, over the measured
HBM rate of 6.29 TB/s (MI355X_MICROARCH: float4 copy).  (d) on config_mld_scene (fp16 weight image and fp16 VAE, K = 20, T = 60,
O = 15: the pass of scripts/recording_bench.py with a scene condition fed by the views): predict_recording_ms with window_frames, and
``share_of_pass`` = the kernel's median over (the kernel's median + the pass's median).

Every leg is warmed up first; times are device events around work that ends in a synchronise; the legs alternate, ``--repeats``
(5) times each; min / median / max in ms."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from hyp_select_bench import alternate                # noqa: E402
from hypotheses_bench import build                    # noqa: E402

SHAPE = (64, 1_000_000, 20_000)
HBM_BYTES_PER_S = 6.29e12


def inputs(W, N):
    g = np.random.default_rng(3)
    verts = (g.random((N, 3)) * np.array([10.0, 10.0, 3.0]) - np.array([5.0, 5.0, 0.0])).astype(np.float32)
    M = np.zeros((W, 4, 4))
    for w in range(W):
        yaw, pos = 2.0 * math.pi * w / W, np.array([3.0 * math.cos(0.1 * w), 3.0 * math.sin(0.1 * w), 1.6])
        c, s = math.cos(yaw), math.sin(yaw)
        cam2world = np.array([[c, 0.0, s], [s, 0.0, -c], [0.0, 1.0, 0.0]])           # the camera looks along its +z, level with the floor
        M[w, :3, :3], M[w, :3, 3], M[w, 3, 3] = cam2world.T, -cam2world.T @ pos, 1.0
    return verts, M.astype(np.float32)


def views_numpy(verts, M, P):
    W = M.shape[0]
    cloud, index, count = np.zeros((W, P, 3), np.float32), np.full((W, P), -1, np.int32), np.zeros(W, np.int32)
    for w in range(W):
        p = verts @ M[w, :3, :3].T + M[w, :3, 3]
        idx = np.flatnonzero(p[:, 2] > 0)
        n = count[w] = len(idx)
        if n == 0:
            continue
        sel = idx[::n // P][:P] if n >= P else idx[np.arange(P) % n]
        cloud[w], index[w] = p[sel], sel
    return cloud, index, count


def kernel_legs(dev, repeats):
    from seeme_amd import recording as R
    W, N, P = SHAPE
    verts, M = inputs(W, N)
    v, m = torch.from_numpy(verts).to(dev), torch.from_numpy(M).to(dev)
    r = alternate({"scene_views_hip_ms": lambda: R.scene_views_hip(v, m, P), "scene_views_torch_ms": lambda: R.scene_views_torch(v, m, P),
                   "scene_views_numpy_ms": lambda: views_numpy(verts, M, P)}, repeats)
    a, b = R.scene_views_hip(v, m, P), R.scene_views_torch(v, m, P)
    same = a["index"] == b["index"]
    r["count_min_max"] = [int(a["count"].min()), int(a["count"].max())]
    r["rows_with_equal_index_hip_vs_torch_fp32"] = float(same.float().mean())      # (they may differ within rounding of a view's plane)
    r["max_abs_diff_on_equal_rows_hip_vs_torch_fp32"] = float((a["cloud"] - b["cloud"]).abs()[same].max())
    passes = -(-W // R.SCENE_VIEW_WINDOWS_PER_PASS)
    r["traffic_bytes"] = 2 * passes * 12 * N + 16 * W * P
    r["floor_ms"] = round(r["traffic_bytes"] / HBM_BYTES_PER_S * 1e3, 4)
    r["hip_over_floor"] = round(r["scene_views_hip_ms"]["median"] / r["floor_ms"], 1)
    for name in ("torch", "numpy"):
        r[f"{name}_over_hip"] = round(r[f"scene_views_{name}_ms"]["median"] / max(r["scene_views_hip_ms"]["median"], 1e-6), 1)
    r["hip_below_torch"] = r["scene_views_hip_ms"]["max"] < r["scene_views_torch_ms"]["min"]
    r["shape"] = list(SHAPE)
    return r, a["cloud"], m


def pass_legs(dev, repeats, kernels, cloud, m):
    from seeme_amd import recording as R
    W, N, P = SHAPE
    K, T, O = 20, 60, 15
    n = (W - 1) * (T - O) + T
    model, dm, cfg = build("config_mld_scene.yaml", dev, T, P)
    batch = list(dm.batch(W, idx=1, with_scene=True))
    batch[4] = cloud                                                     # the scene slot: every window's own view
    with torch.no_grad():
        torch.manual_seed(1)
        r = alternate({"predict_recording_ms": lambda: model.predict_recording(tuple(batch), n, overlap=O, num_hypotheses=K, window_frames=m)},
                      repeats)
    hip = kernels["scene_views_hip_ms"]["median"]
    r["share_of_pass"] = round(hip / (hip + r["predict_recording_ms"]["median"]), 5)
    r["config"], r["shape"] = "config_mld_scene.yaml", [W, K, T, O]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "scene_views.json"))
    ap.add_argument("--skip_pass", action="store_true", help="kernel legs only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    kernels, cloud, m = kernel_legs(dev, args.repeats)
    res = {"bench": "scene_views", "device": torch.cuda.get_device_name(0), "kernels": kernels}
    if not args.skip_pass:
        res["pass"] = pass_legs(dev, args.repeats, kernels, cloud, m)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
