#!/usr/bin/env python
"""Cost of the body-scene term beside its plain-torch twin and beside a whole ``predict_recording`` pass.  Writes
profiles/scene_cost.json (``--out``).

Synthetic input: a room of 6 x 5 x 2.7 m (floor, four walls, a table top and a shelf, sampled uniformly per area) as a cloud of
N = 20 000 and N = 500 000 points, and (W,K,T) = (64,20,60) standing bodies in it: a 24-joint skeleton of SMPL's proportions, one
spot per window, 0.2 m of scatter per hypothesis, a slow walk over the frames; 21 capsules of 4 to 9 cm.  fp32 on the device:
  (a) scene_depth_hip_ms_N / scene_depth_torch_ms_N   ``seeme_scene_depth`` (both launches: lengths on the device already) /
                                                      ``scene_depth_torch`` in chunks of 2^27 triples.  The twin at N = 500 000
                                                      takes most of a minute per call and is timed ``--twin_large_repeats`` (1) times
  (b) cull_N                                          what the boxes let through: the share of the N points inside a chunk's box
                                                      (mean and largest over the chunks), restated in torch
  (c) predict_recording_ms / ..._scene_N              one ``MLD.predict_recording`` pass of config_mld_scene (fp16 weight image and
                                                      VAE) over the same windows without a cloud -- the pass of the commit before the
                                                      term existed -- and with scene_weight 1, scene_report and the same clouds

Every leg is warmed up first; times are device events around work that ends in a synchronise; the legs alternate, ``--repeats``
(5) times each; min / median / max in ms."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from hyp_select_bench import alternate                # noqa: E402
from hypotheses_bench import build, stats, timed      # noqa: E402

SHAPE = (64, 20, 60)
SIZES = (20000, 500000)
ROOM = (6.0, 2.7, 5.0)                                 # x, y (up), z
# a standing body: SMPL's joint order, metres, y up, the floor at y = 0
SKELETON = [(0, .92, 0), (.07, .83, 0), (-.07, .83, 0), (0, 1.03, 0), (.1, .45, 0), (-.1, .45, 0), (0, 1.17, 0), (.09, .06, 0),
            (-.09, .06, 0), (0, 1.22, 0), (.1, 0, .12), (-.1, 0, .12), (0, 1.43, 0), (.08, 1.34, 0), (-.08, 1.34, 0), (0, 1.52, .03),
            (.17, 1.38, 0), (-.17, 1.38, 0), (.42, 1.37, 0), (-.42, 1.37, 0), (.67, 1.37, 0), (-.67, 1.37, 0), (.75, 1.37, 0),
            (-.75, 1.37, 0)]


def room_cloud(n, g):
    """n points on the room's surfaces, uniform per area: the floor, the four walls, a table top (0.75 m up) and a shelf."""
    X, Y, Z = ROOM
    quads = [((-X / 2, 0, -Z / 2), (X, 0, 0), (0, 0, Z)), ((-X / 2, 0, -Z / 2), (X, 0, 0), (0, Y, 0)), ((-X / 2, 0, Z / 2), (X, 0, 0), (0, Y, 0)),
             ((-X / 2, 0, -Z / 2), (0, 0, Z), (0, Y, 0)), ((X / 2, 0, -Z / 2), (0, 0, Z), (0, Y, 0)),
             ((-0.8, 0.75, -0.5), (1.6, 0, 0), (0, 0, 1.0)), ((1.5, 1.2, -2.4), (1.2, 0, 0), (0, 0, 0.4))]
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in quads])
    which = g.choice(len(quads), n, p=area / area.sum())
    o, u, v = (np.array([q[i] for q in quads], np.float64)[which] for i in range(3))
    return (o + g.random((n, 1)) * u + g.random((n, 1)) * v).astype(np.float32)


def bodies(g):
    W, K, T = SHAPE
    X, _, Z = ROOM
    spot = np.stack([g.uniform(-X / 2 + 0.5, X / 2 - 0.5, W), np.zeros(W), g.uniform(-Z / 2 + 0.5, Z / 2 - 0.5, W)], axis=1)
    root = spot[:, None, None] + 0.2 * g.standard_normal((W, K, 1, 3)) * [1, 0, 1] + np.cumsum(0.01 * g.standard_normal((W, K, T, 3)), axis=2) * [1, 0, 1]
    return (root[:, :, :, None] + np.array(SKELETON) + 0.01 * g.standard_normal((W, K, T, 24, 3))).astype(np.float32)


def capsules():
    from seeme_amd.recording import CAPSULE_SKIP
    from seeme_amd.smpl import SMPL_PARENTS
    segs = np.array([(SMPL_PARENTS[j], j) for j in range(1, 24) if j not in CAPSULE_SKIP], np.int32)
    return segs, np.linspace(0.04, 0.09, len(segs)).astype(np.float32)


def cull_share(jts, points, rmax, chunk):
    """Share of the points inside a chunk's box (the joints' box grown by rmax and the kernel's margin): mean and max over chunks."""
    W, K, T = jts.shape[:3]
    shares = []
    for t0 in range(0, T, chunk):
        j = jts[:, :, t0:t0 + chunk].reshape(W * K, -1, 3)
        lo, hi = j.min(dim=1).values, j.max(dim=1).values
        pad = rmax + 1e-3 + 1e-5 * (torch.maximum(lo.abs(), hi.abs()).max(dim=1, keepdim=True).values + rmax)
        lo, hi = lo - pad, hi + pad
        for c in range(0, W * K, 64):
            inside = ((points[None] >= lo[c:c + 64, None]) & (points[None] <= hi[c:c + 64, None])).all(dim=-1)
            shares.append(inside.float().mean(dim=1))
    s = torch.cat(shares)
    return {"mean": round(float(s.mean()), 5), "max": round(float(s.max()), 5), "chunks": int(s.numel())}


def kernel_legs(dev, repeats, twin_large_repeats):
    from seeme_amd import recording as R
    W, K, T = SHAPE
    g = np.random.default_rng(5)
    jts = torch.from_numpy(bodies(g)).to(dev)
    len32 = torch.full((W,), T, dtype=torch.int32, device=dev)
    segs, radius = capsules()
    clouds = {n: torch.from_numpy(room_cloud(n, g)).to(dev) for n in SIZES}
    hip = lambda n: R._launch_scene_depth(jts, len32, clouds[n], W, K, T, 24, n, segs, radius, len(segs))
    twin = lambda n: R.scene_depth_torch(jts, len32.cpu().tolist(), clouds[n], segs, radius, max_elems=1 << 27)
    small, large = SIZES
    r = alternate({f"scene_depth_hip_ms_{small}": lambda: hip(small), f"scene_depth_hip_ms_{large}": lambda: hip(large),
                   f"scene_depth_torch_ms_{small}": lambda: twin(small)}, repeats)
    r[f"scene_depth_torch_ms_{large}"] = stats([timed(lambda: twin(large)) for _ in range(twin_large_repeats)])
    for n in SIZES:
        r[f"cull_{n}"] = cull_share(jts, clouds[n], float(radius.max()), R.SCENE_DEPTH_CHUNK)
        a = hip(n)
        r[f"frames_penetrating_{n}"] = int(a["hits"].sum())
        r[f"depth_max_mm_{n}"] = round(float(a["depth"].max()), 3)
    a, b = hip(small), twin(small)
    r["depth_max_abs_diff_hip_vs_torch_fp32_mm"] = float((a["depth"] - b["depth"]).abs().max())
    r["hits_equal_hip_vs_torch_fp32"] = bool(torch.equal(a["hits"], b["hits"]))
    r["shape"], r["capsules"] = list(SHAPE), int(len(segs))
    return r


def predict_legs(dev, repeats):
    from seeme_amd import recording as R
    W, K, T = SHAPE
    O = T // 4
    n_frames = T + (W - 1) * (T - O)
    model, dm, cfg = build("config_mld_scene.yaml", dev, T, 20000)
    starts, lens = R.window_plan(n_frames, T, O)
    assert len(starts) == W and lens == [T] * W
    batch = dm.batch(W, idx=1, with_scene=True, lengths=lens)
    g = np.random.default_rng(6)
    caps = capsules()
    plain = model.predict_recording(batch, n_frames, overlap=O, num_hypotheses=K)
    j = plain["predict"]["joints_rst_all"]
    centre = j.reshape(-1, 3).mean(dim=0).cpu().numpy() * [1, 0, 1] + [0, float(j[..., 1].min()), 0]     # the room round the estimates
    clouds = {n: torch.from_numpy(room_cloud(n, g) + centre.astype(np.float32)).to(dev) for n in SIZES}
    legs = {"predict_recording_ms": lambda: model.predict_recording(batch, n_frames, overlap=O, num_hypotheses=K)}
    for n in SIZES:
        legs[f"predict_recording_scene_ms_{n}"] = lambda n=n: model.predict_recording(
            batch, n_frames, overlap=O, num_hypotheses=K, scene_cloud=clouds[n], scene_weight=1.0, scene_report=True, capsules=caps)
    r = alternate(legs, repeats)
    len32 = torch.tensor(lens, dtype=torch.int32, device=dev)
    jc = j.contiguous()
    for n in SIZES:                                                    # the term's own launches on these hypotheses
        r[f"scene_term_ms_{n}"] = stats([timed(lambda: R._launch_scene_depth(jc, len32, clouds[n], W, K, T, 24, n, caps[0], caps[1], len(caps[0])))
                                         for _ in range(repeats + 1)][1:])
        r[f"cull_{n}"] = cull_share(jc, clouds[n], float(caps[1].max()), R.SCENE_DEPTH_CHUNK)
        r[f"scene_share_of_pass_{n}"] = round(r[f"scene_term_ms_{n}"]["median"] / r[f"predict_recording_scene_ms_{n}"]["median"], 4)
    r["n_frames"], r["windows"], r["hypotheses"] = n_frames, W, K
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--twin_large_repeats", type=int, default=1)
    ap.add_argument("--skip_predict", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "scene_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"bench": "scene_cost", "device": torch.cuda.get_device_name(0), "kernels": kernel_legs(dev, args.repeats, args.twin_large_repeats)}
    if not args.skip_predict:
        res["predict"] = predict_legs(dev, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
