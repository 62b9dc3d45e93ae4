"""One launch of seeme_crop_patches under HIP events: 32 patches of 224 from 1080 x 1920 frames, after warm-up, the median of 20.
Information, not a target: the call is bounded by the upload of the frames, which is timed next to it.
    python scripts/crop_patches_bench.py [--out profiles/crop_patches.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seeme_amd import crops as CR  # noqa: E402


def _events(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"min_ms": min(ms), "median_ms": float(np.median(ms)), "max_ms": max(ms), "n": repeats}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--patches", type=int, default=32)
    p.add_argument("--repeats", type=int, default=20)
    args = p.parse_args()
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    dev = torch.device("cuda:0")
    n, H, W, S = args.patches, 1080, 1920, CR.PATCH
    g = np.random.default_rng(0)
    host = torch.from_numpy(g.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).pin_memory()
    frames = host.to(dev)
    # boxes of 300..900 pixels around the interactee, some over the border
    boxes = np.stack([g.uniform(200, 1800, n), g.uniform(100, 1000, n), g.uniform(300, 900, n)], axis=1).astype(np.float32)
    fop_d, box_d = torch.arange(n, dtype=torch.int32, device=dev), torch.from_numpy(boxes).to(dev)
    out = torch.empty(n, S, S, 3, dtype=torch.uint8, device=dev)
    launch = _events(lambda: CR._launch(frames, fop_d, box_d, S, out), 5, args.repeats)
    assert torch.equal(out.cpu(), CR.crop_patches_torch(host, np.arange(n), boxes)), "kernel and twin disagree"
    upload = _events(lambda: frames.copy_(host, non_blocking=True), 2, args.repeats)
    m = boxes[:, 2].astype(np.float64) / S
    res = {"device": torch.cuda.get_device_name(0), "what": "information, not a target",
           "shape": {"patches": n, "S": S, "H": H, "W": W, "box_side_px": [float(boxes[:, 2].min()), float(boxes[:, 2].max())]},
           "launch": launch, "upload_of_the_frames_pinned": dict(upload, bytes=int(host.numel())),
           "bytes_written": n * S * S * 3,
           "bytes_of_the_taps_upper_bound": int(sum(min(H, (S * k + 2)) * min(W, (S * k + 2)) * 3 for k in m))}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
