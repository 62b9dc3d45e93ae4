#!/usr/bin/env python
"""Launch times of the interactee track (seeme_amd/track.py) at Lf = 2000 stored frames, S = 32 samples, L = 6000 recording frames
(every third frame stored), fp32 on the device.  Writes profiles/track.json (``--out``).

  track_cost_ms     ``seeme_track_cost``: 1999 x 32 x 32 transition costs
  path_select_ms    ``seeme_path_select`` with W = 2000, K = 32 (one wave: the chain of 1999 dependent steps)
  track_filter_ms   ``seeme_track_filter``: 24 joints and the translation, Gaussian taps of sigma 2 (R = 6)
  track_filter_r32_ms  the same with R = 32 (sigma 10 has R = 30)

Every leg is warmed up; a timed window is ``--launches`` (20) back-to-back launches between device events, ended by a synchronise;
``--repeats`` (5) windows per leg, the legs alternating; min / median / max of the time per launch in ms."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from hypotheses_bench import stats, timed      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "track.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from seeme_amd import recording as R
    from seeme_amd import track as TK
    dev = torch.device("cuda:0")
    Lf, S, L_ = 2000, 32, 6000
    g = torch.Generator().manual_seed(5)
    idx = np.arange(Lf, dtype=np.int64) * 3
    idx32 = torch.from_numpy(idx.astype(np.int32)).to(dev)
    walk = torch.cumsum(0.02 * torch.randn(Lf, 1, 24, 3, generator=g), dim=0)
    jts = (walk + 0.05 * torch.randn(Lf, S, 24, 3, generator=g)).to(dev)
    unary = torch.rand(Lf, S, generator=g).to(dev)
    pose = (0.5 * torch.randn(1, 24, 3, generator=g) + torch.cumsum(0.02 * torch.randn(Lf, 24, 3, generator=g), dim=0)).to(dev)
    tr = torch.cumsum(0.02 * torch.randn(Lf, 3, generator=g), dim=0).to(dev)
    cost = TK._launch_cost(jts, idx32, Lf, S, 1250.0)
    slot = (torch.empty(L_, 24, 3, device=dev), torch.empty(L_, 3, device=dev))
    taps, taps32 = TK.gaussian_taps(2.0), np.ones(33, np.float32)
    n = args.launches
    legs = {"track_cost_ms": lambda: [TK._launch_cost(jts, idx32, Lf, S, 1250.0, out=cost) for _ in range(n)],
            "path_select_ms": lambda: [R._launch_path(cost, unary, Lf, S) for _ in range(n)],
            "track_filter_ms": lambda: [TK._launch_filter(pose, tr, idx32, Lf, L_, 24, taps, len(taps) - 1, out=slot) for _ in range(n)],
            "track_filter_r32_ms": lambda: [TK._launch_filter(pose, tr, idx32, Lf, L_, 24, taps32, 32, out=slot) for _ in range(n)]}
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            times[k].append(timed(fn) / n)
    res = {"bench": "track", "device": torch.cuda.get_device_name(0), "shape": {"Lf": Lf, "S": S, "L": L_, "J": 24, "transl": True},
           "launches_per_window": n}
    res.update({k: stats(v) for k, v in times.items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
