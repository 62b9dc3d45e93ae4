#!/usr/bin/env python
"""Times the optimiser phase and the whole stage-2 training step with the training loop's options, against the same work done
with PyTorch operations after the plain one-launch AdamW.  Writes profiles/train_opt.json.

config_mld_egobody and config_mld_scene at the benchmark's training size (B = 64, T = 196, 20 000-point scenes, bf16 PointNet and
fp16 frozen VAE operands, as ``bench.py --mode train`` sets them).  One model per config; the legs share its optimiser state and
take turns in ONE process (leg 1..6, then again, ``--repeats`` times), one untimed step after every switch:

  parent    the plain step as it was before the options existed: the same calls, without the version-counter bump
  off       options off                                       -- must match `parent` within the spread measured here
  ema       EMA in the AdamW launch (seeme_adamw_step_ex)
  ema_torch the plain step, then torch._foreach_lerp_ over the shadows
  clip      seeme_grad_norm + the scale read by seeme_adamw_step_ex from device memory
  clip_torch torch.nn.utils.clip_grad_norm_, then the plain step

`adamw_ms` is the span between the events MLD.optimizer_step records around its optimiser phase, `step_ms` the span of the whole
step (training_step + optimizer_step); device events, per step; min / median / max over all timed steps of a leg, and the
median of every repeat, whose range over the repeats is the run-to-run spread a comparison has to beat.  One GPU: the
all-reduce is a no-op, and nothing here says anything about several ranks."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4), "n": len(v)}


class _Leg:
    """A stepper in the place of MLD._fused_adamw: `before` / `after` run around the plain one-launch step."""

    def __init__(self, plain, before=None, after=None, bump=True):
        self.plain, self.before, self.after, self.bump = plain, before, after, bump
        self.last_grad_norm = None

    def step(self, device_step=False):
        if self.before:
            self.before()
        if self.bump:
            self.plain.step()
        else:
            keep = torch.autograd.graph.increment_version
            torch.autograd.graph.increment_version = lambda ts: None
            try:
                self.plain.step()
            finally:
                torch.autograd.graph.increment_version = keep
        if self.after:
            self.after()


def run_config(name, args, dev):
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.optim import FusedAdamWStep, ema_decay_at
    from seeme_amd.smpl import SMPL
    from seeme_amd.weights_recipe import load_recipe_
    cfg = parse_config(os.path.join(REPO, "configs", name + ".yaml"))
    cfg.TRAIN.FROZEN_VAE_PRECISION = "fp16"
    cfg.TRAIN.SCENE_PRECISION = "bf16"
    with_scene = "scene" in cfg.model.condition
    dm = SyntheticEgoDataModule(nfeats=75, T=196, n_points=args.points, seed=1234, device=dev)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser)
    if with_scene:
        load_recipe_(model.proscene.scene_enc)
    model = model.to(dev).train()
    model.configure_optimizers()
    batches = [dm.batch(args.batch, idx=i, with_scene=with_scene) for i in range(2)]
    plain = model._fused_adamw
    for i in range(4):                                     # parameter discovery, gradient bucket, optimiser state
        model.optimizer_step(model.training_step(batches[i % 2], i))
    opt = model.optimizer
    params = list(model.grad_bucket().params)
    shadows = [p.detach().clone() for p in params]
    d, c = args.ema_decay, args.clip
    w = lambda: 1.0 - ema_decay_at(d, True, float(opt.state[params[0]]["step"]))
    legs = {
        "parent": _Leg(plain, bump=False),
        "off": plain,
        "ema": FusedAdamWStep(opt, ema_decay=d),
        "ema_torch": _Leg(plain, after=lambda: torch._foreach_lerp_(shadows, [p.detach() for p in params], w())),
        "clip": FusedAdamWStep(opt, grad_clip_norm=c),
        "clip_torch": _Leg(plain, before=lambda: torch.nn.utils.clip_grad_norm_(params, c)),
    }
    ev = lambda: torch.cuda.Event(enable_timing=True)
    adamw = {k: [] for k in legs}
    whole = {k: [] for k in legs}
    rep_adamw = {k: [] for k in legs}
    rep_whole = {k: [] for k in legs}
    it = 0
    for rep in range(args.repeats):
        for k, leg in legs.items():
            model._fused_adamw = leg
            model.optimizer_step(model.training_step(batches[it % 2], it))         # untimed: tables, adopted step count
            it += 1
            evs = [[ev() for _ in range(6)] for _ in range(args.steps)]
            torch.cuda.synchronize()
            for e in evs:
                e[4].record()
                model.optimizer_step(model.training_step(batches[it % 2], it), events=e[:4])
                e[5].record()
                it += 1
            torch.cuda.synchronize()
            a, s = [e[2].elapsed_time(e[3]) for e in evs], [e[4].elapsed_time(e[5]) for e in evs]
            adamw[k] += a
            whole[k] += s
            rep_adamw[k].append(round(statistics.median(a), 4))
            rep_whole[k].append(round(statistics.median(s), 4))
    model._fused_adamw = plain
    spread = lambda r: round(max(max(v) - min(v) for v in r.values()), 4)
    out = {"trainable_elements": sum(p.numel() for p in params), "tensors": len(params),
           "legs": {k: {"adamw_ms": stats(adamw[k]), "step_ms": stats(whole[k]), "adamw_ms_median_per_repeat": rep_adamw[k],
                        "step_ms_median_per_repeat": rep_whole[k]} for k in legs},
           "spread_ms": {"adamw": spread(rep_adamw), "step": spread(rep_whole)}}
    med = lambda k, t=adamw: statistics.median(t[k])
    out["adamw_ms_median_difference"] = {"off - parent": round(med("off") - med("parent"), 4), "ema - ema_torch": round(med("ema") - med("ema_torch"), 4),
                                         "clip - clip_torch": round(med("clip") - med("clip_torch"), 4)}
    out["step_ms_median_difference"] = {"off - parent": round(med("off", whole) - med("parent", whole), 4),
                                        "ema - ema_torch": round(med("ema", whole) - med("ema_torch", whole), 4),
                                        "clip - clip_torch": round(med("clip", whole) - med("clip_torch", whole), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per leg and repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ema_decay", type=float, default=0.999)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "train_opt.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    res = {"what": "optimiser phase and whole stage-2 training step per leg, ms, device events; see scripts/train_opt_bench.py",
           "batch": args.batch, "frames": 196, "points": args.points, "steps_per_leg_and_repeat": args.steps, "repeats": args.repeats,
           "ema_decay": args.ema_decay, "grad_clip_norm": args.clip, "gpus": 1,
           "configs": {name: run_config(name, args, dev) for name in ("config_mld_egobody", "config_mld_scene")}}
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {leg: v["adamw_ms"]["median"] for leg, v in c["legs"].items()} for k, c in res["configs"].items()}))


if __name__ == "__main__":
    main()
