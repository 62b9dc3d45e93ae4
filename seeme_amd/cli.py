"""Lightning-free equivalents of the reference's ``train.py`` / ``test.py`` for the accelerated path.

What the reference delegates to ``pl.Trainer`` (train.py:127-149, test.py:86-134) is done here directly:
one process per GPU (``torch.distributed`` / RCCL, launched by ``torchrun``), parameter broadcast, one
flat-bucket gradient all-reduce per step, checkpoints in Lightning's ``{"state_dict": ...}`` layout under
``<FOLDER>/<model_type>/<NAME>/checkpoints/epoch=<n>.ckpt`` (train.py:114-123), resume from the newest
``epoch=*.ckpt`` of ``TRAIN.RESUME`` (train.py:26-53), strict load of the ``vae.*`` sub-dict for stage 2
(train.py:155-167), strict full load for testing (test.py:111-113), metrics summed over ranks and written
to ``metrics_<time>.json`` (test.py:136-152), a validation pass every ``LOGGER.VAL_EVERY_STEPS`` epochs (train.py:142-148) with
``checkpoints/best.ckpt``, and the EMA weights / gradient clipping of ``seeme_amd.optim``.

The argument surface is the reference's (mld/config.py:35-65: --cfg --cfg_assets --batch_size --device
--nodebug --dir) plus loop bounds for the synthetic data module: the EgoBody / GIMO datasets are
licence-gated: ``--data_root`` points ``seeme_amd.data.EgoDataModule`` at a directory in the reference's on-disk layout
(split resident in HBM); without it batches come from ``SyntheticEgoDataModule``.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import logging
import os
import re
import time
from typing import Dict, List, Optional

import torch

from . import distributed as D
from .config import parse_config

CKPT_RE = re.compile(r"^epoch=(\d+)\.ckpt$")


# ----------------------------------------------------------------------------- arguments / folders
def build_parser(phase: str) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog=f"seeme_amd {phase}")
    g = p.add_argument_group("reference options (mld/config.py:35-65)")
    g.add_argument("--cfg", type=str, default="./configs/config_mld_egobody.yaml", help="config file")
    g.add_argument("--cfg_assets", type=str, default=None, help="config file for asset paths")
    g.add_argument("--batch_size", type=int, help="batch size per GPU")
    g.add_argument("--device", type=int, nargs="+", help="accepted for compatibility; ranks come from torchrun")
    g.add_argument("--nodebug", action="store_true", help="debug or not")
    g.add_argument("--dir", type=str, help="evaluate existing npys (not supported on this path)")
    s = p.add_argument_group("loop bounds of the synthetic data module")
    s.add_argument("--epochs", type=int, default=None, help="override TRAIN.END_EPOCH")
    s.add_argument("--iters_per_epoch", type=int, default=8, help="batches per epoch and rank")
    s.add_argument("--test_batches", type=int, default=4, help="batches per replication and rank")
    s.add_argument("--data_root", type=str, default=None,
                   help="directory in the reference's EgoBody / GIMO on-disk layout (seeme_amd/data.py); default: synthetic batches")
    s.add_argument("--scene_root", type=str, default=None, help="scene tables of --data_root (default: the same directory)")
    s.add_argument("--storage", type=str, default="device", choices=["device", "pinned"], help="where --data_root's splits live")
    s.add_argument("--scene_points", type=int, default=20000)
    s.add_argument("--frames", type=int, default=196)
    s.add_argument("--folder", type=str, default=None, help="override FOLDER (experiment root)")
    s.add_argument("--checkpoint", type=str, default=None, help="override TEST.CHECKPOINTS")
    s.add_argument("--num_hypotheses", type=int, default=None, help="override TEST.NUM_HYPOTHESES (draws per sequence, 1..32)")
    s.add_argument("--hyp_select", type=str, default=None, choices=["first", "medoid"],
                   help="override TEST.HYP_SELECT: the draw that stands for its sequence when --num_hypotheses > 1 (medoid: label-free)")
    s.add_argument("--mesh_metrics", action="store_true",
                   help="set TEST.MESH_METRICS: PA-MPJPE, V2V and body-scene contact per hypothesis (seeme_amd/mesh_metrics.py)")
    s.add_argument("--collision_metrics", action="store_true",
                   help="set TEST.COLLISION_METRICS: share of the scene cloud inside the body per hypothesis (needs a 'scene' condition)")
    s.add_argument("--social_metrics", action="store_true",
                   help="set TEST.SOCIAL_METRICS: the errors by interpersonal distance and mutual gaze (seeme_amd/social_metrics.py)")
    t = p.add_argument_group("training loop (seeme_amd/optim.py, INTEGRATION.md J)")
    t.add_argument("--ema_decay", type=float, default=None, help="override TRAIN.EMA_DECAY (0 = no EMA of the weights)")
    t.add_argument("--grad_clip", type=float, default=None, help="override TRAIN.GRAD_CLIP_NORM (0 = no gradient-norm clipping)")
    t.add_argument("--val_every", type=int, default=None, help="override LOGGER.VAL_EVERY_STEPS: validate every N epochs (0 = never)")
    t.add_argument("--val_batches", type=int, default=4, help="synthetic data: validation batches per pass and rank")
    t.add_argument("--use_ema", action="store_true", help="set TEST.USE_EMA: evaluate the checkpoint's ema_state_dict")
    return p


def load_cfg(args, phase: str):
    cfg = parse_config(args.cfg, cfg_assets=args.cfg_assets, batch_size=args.batch_size, phase=phase)
    if phase == "train":
        cfg.DEBUG = (not args.nodebug) if args.nodebug else cfg.get("DEBUG", False)
        if cfg.DEBUG:
            cfg.NAME = "debug--" + str(cfg.get("NAME", "exp"))       # mld/config.py:190-193
    if getattr(args, "num_hypotheses", None) is not None:
        cfg.TEST.NUM_HYPOTHESES = args.num_hypotheses
    if getattr(args, "hyp_select", None) is not None:
        cfg.TEST.HYP_SELECT = args.hyp_select
    if getattr(args, "mesh_metrics", False):
        cfg.TEST.MESH_METRICS = True
    if getattr(args, "collision_metrics", False):
        cfg.TEST.COLLISION_METRICS = True
    if getattr(args, "social_metrics", False):
        cfg.TEST.SOCIAL_METRICS = True
    if getattr(args, "ema_decay", None) is not None:
        cfg.TRAIN.EMA_DECAY = args.ema_decay
    if getattr(args, "grad_clip", None) is not None:
        cfg.TRAIN.GRAD_CLIP_NORM = args.grad_clip
    if getattr(args, "val_every", None) is not None:
        if args.val_every < 0:
            raise ValueError("--val_every must be >= 0 (0 = never)")
        cfg.LOGGER.VAL_EVERY_STEPS = args.val_every
    if getattr(args, "use_ema", False):
        cfg.TEST.USE_EMA = True
    if args.folder:
        cfg.FOLDER = args.folder
    cfg.setdefault("FOLDER", "./experiments")
    cfg.setdefault("NAME", "exp")
    cfg.setdefault("TIME", time.strftime("%Y-%m-%d-%H-%M-%S"))
    cfg.FOLDER_EXP = os.path.join(cfg.FOLDER, str(cfg.model.get("model_type", "mld")), str(cfg.NAME))
    if args.dir:
        raise NotImplementedError("--dir (evaluate stored npys) is outside the accelerated path")
    return cfg


def make_logger(cfg, phase: str, rank: int) -> logging.Logger:
    log = logging.getLogger(f"seeme_amd.{phase}")
    log.setLevel(logging.INFO if rank == 0 else logging.WARNING)
    log.handlers.clear()
    fmt = logging.Formatter("%(asctime)s %(message)s")
    h = logging.StreamHandler()
    h.setFormatter(fmt)
    log.addHandler(h)
    if rank == 0:
        os.makedirs(cfg.FOLDER_EXP, exist_ok=True)
        fh = logging.FileHandler(os.path.join(cfg.FOLDER_EXP, f"log_{phase}_{cfg.TIME}.log"))
        fh.setFormatter(fmt)
        log.addHandler(fh)
    return log


# ----------------------------------------------------------------------------- checkpoints (Lightning layout)
BEST_CKPT = "best.ckpt"            # the checkpoint of the best validation MPJPE so far; not an epoch=<n>.ckpt, so resume ignores it


def save_checkpoint(path: str, model, epoch: int, global_step: int, monitor: Optional[Dict] = None) -> None:
    """"state_dict" is always the RAW weights (reference tooling loads the file unchanged); with TRAIN.EMA_DECAY on the EMA
    weights of the trainable tensors travel beside them as "ema_state_dict", under the same names."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    obj = {"epoch": epoch, "global_step": global_step, "pytorch-lightning_version": "seeme-amd",
           "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
           "optimizer_states": [model.optimizer.state_dict()] if model.optimizer is not None else []}
    if getattr(model, "ema_decay", 0.0) > 0.0 and model.optimizer is not None:
        obj["ema_state_dict"] = {k: v.detach().cpu() for k, v in model.ema_state_dict().items()}
    if monitor is not None:
        obj["monitor"] = dict(monitor)
    # where this process's random streams stand: a resumed single-process run then draws what the uninterrupted run would have drawn
    obj["rng_state"] = {"cpu": torch.get_rng_state()}
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        obj["rng_state"]["cuda"] = torch.cuda.get_rng_state()
    tmp = path + ".tmp"
    torch.save(obj, tmp)
    os.replace(tmp, path)


def read_checkpoint(path: str) -> Dict:
    """Tensor-only load: nothing in the file is executed."""
    return torch.load(path, map_location="cpu", weights_only=True)


def newest_checkpoint(resume_dir: str) -> Optional[str]:
    d = os.path.join(resume_dir, "checkpoints")
    if not os.path.isdir(d):
        raise ValueError("Resume path is not right.")                  # train.py:56
    best = None
    for fn in os.listdir(d):
        m = CKPT_RE.match(fn)
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), os.path.join(d, fn))
    return best[1] if best else None


def load_pretrained_vae(model, path: str) -> int:
    """Stage 2 starts from a stage-1 checkpoint: the ``vae.*`` entries, strictly (train.py:155-167)."""
    sd = read_checkpoint(path)["state_dict"]
    sub = {k[len("vae."):]: v for k, v in sd.items() if k.split(".")[0] == "vae"}
    model.vae.load_state_dict(sub, strict=True)
    return len(sub)


# ----------------------------------------------------------------------------- model / data
def build(cfg, dev, args, datamodule=None, smpl_model=None):
    from .mld import MLD, SyntheticEgoDataModule
    from .smpl import SMPL
    from .shapes import motion_layout
    data_type = str(cfg.DATA_TYPE)
    nfeats = 75 if cfg.DATASET_NAME == "egobody" else (69 if cfg.DATASET_NAME == "gimo" else cfg.model.nfeats)
    if data_type != "angle":                                          # rot6d: 144 on EgoBody; raises for GIMO
        nfeats = motion_layout(cfg.DATASET_NAME, data_type, True, cfg.model.nfeats)[0]
    if datamodule is None and getattr(args, "data_root", None):
        from .data import EgoDataModule
        datamodule = EgoDataModule(args.data_root, cfg.DATASET_NAME, tuple(cfg.model.condition), motion_length=int(cfg.MOTION_LENGTH),
                                   predict_transl=bool(cfg.TRAIN.ABLATION.PREDICT_TRANSL), device=dev, storage=args.storage,
                                   scene_root=args.scene_root, pose_estimation_task=bool(cfg.TEST.get("POSE_ESTIMATION_TASK", False)),
                                   interactee_pred=bool(cfg.TEST.get("INTERACTEE_PRED", False)),      # get_data.py:196
                                   seed=int(cfg.SEED_VALUE), image_backbone=bool(cfg.model.get("image_backbone", False)),
                                   data_type=data_type)
    dm = datamodule or SyntheticEgoDataModule(nfeats=nfeats, T=args.frames, n_points=args.scene_points,
                                               seed=int(cfg.SEED_VALUE), device=dev, data_type=data_type)
    if smpl_model is None and not os.path.exists(str(cfg.model.smpl_path)):
        smpl_model = SMPL.synthetic(int(cfg.SEED_VALUE))              # SMPL_NEUTRAL.pkl is licence-gated
    model = MLD(cfg, dm, smpl_model=smpl_model)
    return model, dm


def _with_scene(cfg) -> bool:
    return "scene" in cfg.model.condition


def _with_image(cfg):
    """False, True (pooled features) or "crops" (model.image_backbone: uint8 crops for the HIP ResNet-50)."""
    if "image" not in cfg.model.condition:
        return False
    return "crops" if bool(cfg.model.get("image_backbone", False)) else True


def overlay_ema(model, ck: Dict, path: str) -> int:
    """TEST.USE_EMA: the checkpoint's EMA weights over the (strictly loaded) raw ones."""
    ema = ck.get("ema_state_dict")
    if not ema:
        raise ValueError(f"--use_ema / TEST.USE_EMA: {path} has no ema_state_dict (it was trained with TRAIN.EMA_DECAY 0)")
    missing, unexpected = model.load_state_dict(ema, strict=False)
    if unexpected:
        raise ValueError(f"--use_ema: {path}: ema_state_dict has entries the model does not: {unexpected}")
    return len(ema)


def validate(model, dm, cfg, args, dev, rank: int, ws: int) -> Optional[Dict]:
    """One validation pass (what Lightning runs every check_val_every_n_epoch, train.py:142-148): model.validation_step over the
    'val' split -- files: dm.iterate("val", EVAL.BATCH_SIZE); synthetic: --val_batches batches from an index range of their own --
    on the EMA weights when TRAIN.EMA_DECAY is on, metrics and losses summed over the ranks.  The pass runs on a forked random
    stream seeded from SEED_VALUE: it draws the same noise every time and leaves the training stream where it was.  None when
    the data has no 'val' split."""
    if hasattr(dm, "iterate") and "val" not in getattr(dm, "splits", {"val": None}):
        return None
    B = int(cfg.EVAL.BATCH_SIZE if args.batch_size is None else args.batch_size)
    was_training = model.training
    model.eval()
    model.EgoMetric.reset()
    model.losses["val"].reset()
    scope = model.ema_scope() if model.ema_decay > 0.0 else contextlib.nullcontext()
    try:
        with torch.random.fork_rng(devices=[dev]), torch.no_grad(), scope:
            torch.manual_seed(int(cfg.SEED_VALUE) * 7919 + 104729 + rank)
            if hasattr(dm, "iterate"):
                batches = dm.iterate("val", B, rank=rank, world=ws)
            else:
                batches = (dm.batch(B, idx=20_000_000 + it * ws + rank, with_scene=_with_scene(cfg), split="val",
                                    with_image=_with_image(cfg)) for it in range(args.val_batches))
            for it, batch in enumerate(batches):
                model.validation_step(batch, it)
            sums = D.reduce_sums(model.EgoMetric.sums().to(dev)).cpu()
            metrics = model.EgoMetric.compute(sums)
            lsum = model.losses["val"]
            names = sorted(lsum.sums)
            vec = D.reduce_sums(torch.stack([torch.as_tensor(lsum.sums[k], dtype=torch.float32, device=dev) for k in names] +
                                            [torch.as_tensor(float(lsum.count), dtype=torch.float32, device=dev)])).cpu()
            n = max(float(vec[-1]), 1.0)
            metrics.update({f"loss_{k}": float(vec[i]) / n for i, k in enumerate(names)})
    finally:
        model.train(was_training)
    return {k: float(v) for k, v in metrics.items()}


# ----------------------------------------------------------------------------- train
def train_main(argv: Optional[List[str]] = None, datamodule=None, smpl_model=None) -> Dict:
    args = build_parser("train").parse_args(argv)
    rank, ws, local = D.init_from_env()
    cfg = load_cfg(args, "train")
    log = make_logger(cfg, "train", rank)
    if not torch.cuda.is_available():
        raise SystemExit("training runs on the HIP path: an MI355X is required (no CPU fallback)")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    torch.manual_seed(int(cfg.SEED_VALUE) + rank)

    model, dm = build(cfg, dev, args, datamodule, smpl_model)
    start_epoch, global_step = 0, 0
    if cfg.TRAIN.get("PRETRAINED_VAE"):
        n = load_pretrained_vae(model, cfg.TRAIN.PRETRAINED_VAE)
        log.info("Loading pretrain vae from %s (%d tensors, strict)", cfg.TRAIN.PRETRAINED_VAE, n)
    resume_ckpt = newest_checkpoint(cfg.TRAIN.RESUME) if cfg.TRAIN.get("RESUME") else None
    pre = resume_ckpt or cfg.TRAIN.get("PRETRAINED")
    ck = None
    if pre:
        ck = read_checkpoint(pre)
        sd = {k: v for k, v in ck["state_dict"].items() if k != "denoiser.sequence_pos_encoding.pe"}   # train.py:177-180
        missing, unexpected = model.load_state_dict(sd, strict=False)
        log.info("Loading pretrain model from %s (missing %d, unexpected %d)", pre, len(missing), len(unexpected))
    model = model.to(dev).train()
    D.broadcast_parameters(model)
    model.configure_optimizers()
    if resume_ckpt and ck is not None:
        start_epoch, global_step = int(ck.get("epoch", -1)) + 1, int(ck.get("global_step", 0))
        if ck.get("optimizer_states"):
            model.optimizer.load_state_dict(ck["optimizer_states"][0])
        log.info("Resuming after epoch %d (step %d)", start_epoch - 1, global_step)
        rng = ck.get("rng_state")
        if rng and ws == 1:            # (several ranks: only rank 0's streams are in the file; every rank restarts from its seed)
            torch.set_rng_state(rng["cpu"])
            if "cuda" in rng:
                torch.cuda.set_rng_state(rng["cuda"], dev)
        if model.ema_decay > 0.0:
            if ck.get("ema_state_dict"):
                model.load_ema_state_dict(ck["ema_state_dict"], strict=True)
            else:                      # (the shadows are copies of the loaded weights: configure_optimizers made them)
                log.info("%s has no ema_state_dict: the EMA starts from the loaded weights", resume_ckpt)

    B = int(cfg.TRAIN.BATCH_SIZE)
    end_epoch = int(args.epochs if args.epochs is not None else cfg.TRAIN.END_EPOCH)
    save_every = max(1, int((cfg.get("LOGGER") or {}).get("SACE_CHECKPOINT_EPOCH", 1)))
    ckpt_dir = os.path.join(cfg.FOLDER_EXP, "checkpoints")
    val_every = int((cfg.get("LOGGER") or {}).get("VAL_EVERY_STEPS", 0) or 0)
    best, last_val, val_skipped = None, {}, False
    best_path = os.path.join(ckpt_dir, BEST_CKPT)
    if resume_ckpt and os.path.exists(os.path.join(cfg.TRAIN.RESUME, "checkpoints", BEST_CKPT)):
        mon = read_checkpoint(os.path.join(cfg.TRAIN.RESUME, "checkpoints", BEST_CKPT)).get("monitor")
        if mon:
            best = {"epoch": int(mon["epoch"]), "MPJPE": float(mon["MPJPE"])}
            log.info("best so far: %s", json.dumps(best))
    log.info("stage %s, conditions %s, batch %d per GPU x %d GPU(s), epochs %d..%d", cfg.TRAIN.STAGE,
             list(cfg.model.condition), B, ws, start_epoch, end_epoch - 1)
    last = {}
    for epoch in range(start_epoch, end_epoch):
        model.losses["train"].reset()
        t0 = time.perf_counter()
        if hasattr(dm, "iterate"):      # files: one pass over the train split per epoch, a new permutation each, ranks take disjoint
            # strided shares (what the reference's DataLoader + DistributedSampler do, train.py:127-149); drop_last keeps the ranks in step
            batches = dm.iterate("train", B, shuffle=True, seed=int(cfg.SEED_VALUE), epoch=epoch, rank=rank, world=ws, drop_last=True)
        else:                           # synthetic stream: `iters_per_epoch` fresh batches
            batches = (dm.batch(B, idx=(epoch * args.iters_per_epoch + it) * ws + rank, with_scene=_with_scene(cfg),
                                with_image=_with_image(cfg)) for it in range(args.iters_per_epoch))
        n_it = 0
        for it, batch in enumerate(batches):
            loss = model.training_step(batch, it)
            model.optimizer_step(loss)
            global_step += 1
            n_it += 1
        if getattr(model, "sch", None) is not None:
            model.sch.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        sums = model.losses["train"].compute()
        last = {"epoch": epoch, "step": global_step, "seqs_per_s": round(ws * B * n_it / dt, 1),
                **{k: round(v, 6) for k, v in sums.items()}}
        if model.grad_clip_norm > 0.0 and model.last_grad_norm is not None:
            last["grad_norm"] = round(float(model.last_grad_norm[0]), 6)        # of the epoch's last step; the device is idle here
        if val_every > 0 and (epoch + 1) % val_every == 0 and not val_skipped:
            val = validate(model, dm, cfg, args, dev, rank, ws)
            if val is None:
                val_skipped = True
                log.info("the data has no 'val' split: validation is skipped")
            else:
                last_val = {f"val_{k}": round(v, 6) for k, v in val.items()}
                log.info("val epoch %d: %s", epoch, json.dumps(last_val))
                if val["MPJPE"] == val["MPJPE"] and (best is None or val["MPJPE"] < best["MPJPE"]):
                    best = {"epoch": epoch, "MPJPE": float(val["MPJPE"])}
                    if rank == 0:
                        save_checkpoint(best_path, model, epoch, global_step, monitor=best)
                        log.info("checkpoint %s (validation MPJPE %.6f)", best_path, best["MPJPE"])
        last.update(last_val)
        if best is not None:
            last["best"] = dict(best)
        log.info("epoch %d: %s", epoch, json.dumps(last))
        if rank == 0 and ((epoch + 1) % save_every == 0 or epoch + 1 == end_epoch):
            path = os.path.join(ckpt_dir, f"epoch={epoch}.ckpt")
            save_checkpoint(path, model, epoch, global_step)
            log.info("checkpoint %s", path)
    if D.is_dist():
        torch.distributed.barrier()
    log.info("The checkpoints are stored in %s", ckpt_dir)
    log.info("Training ends!")
    return {"folder": cfg.FOLDER_EXP, "checkpoints": ckpt_dir, **last}


# ----------------------------------------------------------------------------- test
def test_main(argv: Optional[List[str]] = None, datamodule=None, smpl_model=None) -> Dict:
    args = build_parser("test").parse_args(argv)
    rank, ws, local = D.init_from_env()
    cfg = load_cfg(args, "test")
    log = make_logger(cfg, "test", rank)
    if not torch.cuda.is_available():
        raise SystemExit("testing runs on the HIP path: an MI355X is required (no CPU fallback)")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    torch.manual_seed(int(cfg.SEED_VALUE) + rank)
    model, dm = build(cfg, dev, args, datamodule, smpl_model)
    ckpt = args.checkpoint or cfg.TEST.get("CHECKPOINTS")
    if not ckpt:
        raise ValueError("TEST.CHECKPOINTS (or --checkpoint) is required")
    log.info("Loading checkpoints from %s", ckpt)
    ck = read_checkpoint(ckpt)
    model.load_state_dict(ck["state_dict"])                           # strict, test.py:111-113
    use_ema = cfg.TEST.get("USE_EMA", False)
    if not isinstance(use_ema, bool):
        raise ValueError(f"TEST.USE_EMA must be true or false, got {use_ema!r}")
    if use_ema:
        log.info("EMA weights over %d tensors", overlay_ema(model, ck, ckpt))
    model = model.to(dev).eval()
    B = int(cfg.TEST.BATCH_SIZE if args.batch_size is None else args.batch_size)
    all_metrics: Dict[str, List[float]] = {}
    for rep in range(int(cfg.TEST.REPLICATION_TIMES)):
        model.EgoMetric.reset()
        model.HypMetric.reset()
        model.MeshMetric.reset()
        model.CollMetric.reset()
        model.SelMetric.reset()
        model.SocialMetric.reset()
        t0 = time.perf_counter()
        with torch.no_grad():
            if hasattr(dm, "iterate"):  # files: ONE pass over the test split, every sequence exactly once over the ranks (test.py:115-133)
                batches = dm.iterate("test", B, rank=rank, world=ws)
            else:
                batches = (dm.batch(B, idx=10_000_000 + it * ws + rank, with_scene=_with_scene(cfg), split="test",
                                    with_image=_with_image(cfg)) for it in range(args.test_batches))
            n_seq = 0
            for it, batch in enumerate(batches):
                model.test_step(batch, it)
                n_seq += int(batch[0].shape[0])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        sums = D.reduce_sums(model.EgoMetric.sums().to(dev)).cpu()
        metrics = model.EgoMetric.compute(sums)
        metrics["seqs_per_s"] = ws * n_seq / dt
        if model.num_hypotheses > 1:    # K draws per sequence in this pass: best-of-K / mean-of-K error and the diversity of the draws
            metrics.update(model.HypMetric.compute(D.reduce_sums(model.HypMetric.sums().to(dev)).cpu(), model.num_hypotheses))
            metrics["samples_per_s"] = model.num_hypotheses * metrics["seqs_per_s"]
        if model.mesh_metrics:          # PA-MPJPE / V2V (best and mean over the kept hypotheses) and, with a scene, distance and contact
            metrics.update(model.MeshMetric.compute(D.reduce_sums(model.MeshMetric.sums().to(dev)).cpu()))
        if model.collision_metrics:     # share of the scene cloud inside the body, over all hypotheses, and for the reference body
            metrics.update(model.CollMetric.compute(D.reduce_sums(model.CollMetric.sums().to(dev)).cpu()))
        if model.hyp_select == "medoid" and model.num_hypotheses > 1:    # the errors of the label-free choice among the K draws
            metrics.update(model.SelMetric.compute(D.reduce_sums(model.SelMetric.sums().to(dev)).cpu()))
        if model.social_metrics:        # MPJPE by interpersonal distance and by mutual gaze, and how well the interaction is reproduced
            metrics.update(model.SocialMetric.compute(D.reduce_sums(model.SocialMetric.sums().to(dev)).cpu(), model.num_hypotheses))
        log.info("Replication %d: %s", rep, json.dumps({k: round(v, 4) for k, v in metrics.items()}))
        for k, v in metrics.items():
            all_metrics.setdefault(k, []).append(float(v))
    out = {}
    for k, v in all_metrics.items():
        t = torch.tensor(v, dtype=torch.float64)
        out[f"Metrics/{k}/mean"] = float(t.mean())
        out[f"Metrics/{k}/min"], out[f"Metrics/{k}/max"] = float(t.min()), float(t.max())
        out[f"Metrics/{k}/conf_interval"] = float(1.96 * t.std(unbiased=False) / max(len(v), 1) ** 0.5)
        out[f"Metrics/{k}"] = v
    if rank == 0:
        os.makedirs(cfg.FOLDER_EXP, exist_ok=True)
        metric_file = os.path.join(cfg.FOLDER_EXP, f"metrics_{cfg.TIME}.json")
        with open(metric_file, "w", encoding="utf-8") as f:
            json.dump(out, f, indent=4)
        log.info("Testing done, the metrics are saved to %s", metric_file)
        out["file"] = metric_file
    return out


# ----------------------------------------------------------------------------- a recording without labels -> one stitched motion
def motion_to_smpl(motion: torch.Tensor, data_type: str, transl_in_feats: bool, nb: int) -> Dict[str, torch.Tensor]:
    """Renormed features [N,F] -> global_orient [N,3], body_pose [N,nb] and transl [N,3] (zeros when the features carry none), axis-
    angle: 'angle' features are split, 'rot6d' ones (24 x 6, the translation outside them) go through ``geometry.rot6d_to_rotmat`` and
    ``geometry.rotmat_to_aa_torch``."""
    from . import geometry as G
    N = motion.shape[0]
    if data_type == "rot6d":
        aa = G.rotmat_to_aa_torch(G.rot6d_to_rotmat(motion[:, :144].reshape(-1, 6).contiguous())).reshape(N, 72)
        return {"global_orient": aa[:, :3], "body_pose": aa[:, 3:], "transl": torch.zeros(N, 3, device=motion.device)}
    tr = motion[:, -3:] if transl_in_feats else torch.zeros(N, 3, device=motion.device)
    return {"global_orient": motion[:, :3], "body_pose": motion[:, 3:3 + nb], "transl": tr}


def predict_main(argv: Optional[List[str]] = None, datamodule=None, smpl_model=None) -> Dict:
    """predict.py: a recording .npz (``recording.load_recording``: the interactee's motion, optionally a scene cloud, image features
    -- or, for an image_backbone model, video frames with the interactee's box, whose patches are cut on the device -- and the
    wearer's betas -- no wearer labels) -> the stitched SMPL motion of the wearer as an .npz."""
    import numpy as np
    from . import recording as R
    p = build_parser("predict")
    g = p.add_argument_group("recording")
    g.add_argument("--input", type=str, required=True, help="recording .npz (INTEGRATION.md K)")
    g.add_argument("--output", type=str, required=True, help="where the stitched motion goes (.npz)")
    g.add_argument("--overlap", type=int, default=None, help="override TEST.WINDOW_OVERLAP (frames shared by neighbouring windows)")
    g.add_argument("--seed", type=int, default=None, help="seed of the draws (default: SEED_VALUE)")
    g.add_argument("--save_hypotheses", action="store_true", help="also store m_rst_all [W,K,T,F], every window's K hypotheses")
    g.add_argument("--video", type=str, default=None, help="decoded frames, uint8 RGB [Lf,H,W,3] as a .npy (opened memory-mapped), in "
                   "place of the recording's video key; the recording holds center, scale and, for Lf < L, video_index")
    h = p.add_argument_group("the headset's own path (head_path, or the centres of world2cam; INTEGRATION.md K)")
    h.add_argument("--head_weight", type=float, default=None, help="override TEST.PATH_HEAD_WEIGHT: weight of the head-path term (mm) "
                   "when one hypothesis per window is chosen (0 = off)")
    h.add_argument("--anchor_headset", action="store_true", help="set TEST.HEAD_ANCHOR: shift the stitched motion's head onto the path")
    h.add_argument("--anchor_sigma", type=float, default=None, help="override TEST.HEAD_ANCHOR_SIGMA: Gaussian width of the shift's "
                   "filter, frames (0..10)")
    h.add_argument("--head_rot_weight", type=float, default=None, help="override TEST.PATH_HEAD_ROT_WEIGHT: weight of the head-rotation "
                   "term (mm per degree the head turns against the device: head_rot, or the rotations of world2cam; 0 = off)")
    h.add_argument("--head_rot_report", action="store_true", help="set TEST.HEAD_ROT_REPORT: also write head_rot_residual [L] and "
                   "head_rot_mean, the stitched motion's head against the device's orientation (degrees)")
    h.add_argument("--head_offset", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="override "
                   "TEST.HEAD_DEVICE_OFFSET: the vector from joint 15 to the device in the device's frame, metres")
    s = p.add_argument_group("the body against the scene (scene_vertices, or scene; INTEGRATION.md K)")
    s.add_argument("--scene_weight", type=float, default=None, help="override TEST.PATH_SCENE_WEIGHT: weight of the body-scene term "
                   "(mm of penetration) when one hypothesis per window is chosen (0 = off)")
    s.add_argument("--scene_report", action="store_true", help="set TEST.SCENE_REPORT: also write scene_depth [L], the stitched "
                   "motion's penetration per frame (mm)")
    s.add_argument("--scene_quantile", type=float, default=None, help="override TEST.SCENE_CAPSULE_QUANTILE: quantile of the "
                   "template's distances that gives a capsule's radius (0..1)")
    p.set_defaults(frames=None)                                         # the window length: MOTION_LENGTH unless --frames says otherwise
    p.set_defaults(scene_points=None)                                   # rows of a scene view: TEST.SCENE_VIEW_POINTS unless given
    args = p.parse_args(argv)
    cfg = load_cfg(args, "test")
    if args.head_weight is not None:
        cfg.TEST.PATH_HEAD_WEIGHT = args.head_weight
    if args.anchor_headset:
        cfg.TEST.HEAD_ANCHOR = True
    if args.anchor_sigma is not None:
        cfg.TEST.HEAD_ANCHOR_SIGMA = args.anchor_sigma
    if args.head_rot_weight is not None:
        cfg.TEST.PATH_HEAD_ROT_WEIGHT = args.head_rot_weight
    if args.head_rot_report:
        cfg.TEST.HEAD_ROT_REPORT = True
    if args.head_offset is not None:
        cfg.TEST.HEAD_DEVICE_OFFSET = list(args.head_offset)
    if args.scene_weight is not None:
        cfg.TEST.PATH_SCENE_WEIGHT = args.scene_weight
    if args.scene_report:
        cfg.TEST.SCENE_REPORT = True
    if args.scene_quantile is not None:
        cfg.TEST.SCENE_CAPSULE_QUANTILE = args.scene_quantile
    if args.scene_points is not None:
        cfg.TEST.SCENE_VIEW_POINTS = args.scene_points
    args.scene_points = int(cfg.TEST.get("SCENE_VIEW_POINTS", 20000))
    args.frames = T = int(args.frames or cfg.MOTION_LENGTH)
    log = make_logger(cfg, "predict", 0)
    if not torch.cuda.is_available():
        raise SystemExit("prediction runs on the HIP path: an MI355X is required (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.overlap is not None:
        cfg.TEST.WINDOW_OVERLAP = args.overlap
    model, dm = build(cfg, dev, args, datamodule, smpl_model)
    ckpt = args.checkpoint or cfg.TEST.get("CHECKPOINTS")
    if not ckpt:
        raise ValueError("TEST.CHECKPOINTS (or --checkpoint) is required")
    log.info("Loading checkpoints from %s", ckpt)
    ck = read_checkpoint(ckpt)
    model.load_state_dict(ck["state_dict"])
    if cfg.TEST.get("USE_EMA", False):
        log.info("EMA weights over %d tensors", overlay_ema(model, ck, ckpt))
    model = model.to(dev).eval()
    rec = R.load_recording(args.input, video=args.video)
    scene_cloud = None
    if model.path_scene_weight > 0 or model.scene_report:               # the scene's points, in the recording's common frame
        scene_cloud = rec.get("scene_vertices", rec.get("scene"))
        if scene_cloud is None:
            raise ValueError(f"{args.input}: --scene_weight / --scene_report need the scene's points: the recording holds neither "
                             "scene_vertices [N,3] nor scene [P,3]")
    O = model.window_overlap if model.window_overlap is not None else T // 4
    moving = "world2cam" in rec                                         # every window in the camera frame of its first frame
    pelvis = R.rest_pelvis(model.smpl_model, torch.from_numpy(rec["betas"]).to(dev)[None])[0] if moving else None
    made = R.windows_batch(rec, dm, T, O, tuple(cfg.model.condition), dataset=str(cfg.DATASET_NAME), data_type=str(cfg.DATA_TYPE),
                           predict_transl=bool(cfg.TRAIN.ABLATION.PREDICT_TRANSL), device=dev, scene_points=model.scene_view_points,
                           pelvis=pelvis)
    batch, starts, lengths = made[:3]
    frames = made[3] if moving else None
    torch.manual_seed(int(cfg.SEED_VALUE) if args.seed is None else args.seed)
    betas = torch.from_numpy(rec["wearer_betas"]).to(dev) if "wearer_betas" in rec else None
    head_path = None
    if model.path_head_weight > 0 or model.head_anchor:                 # the device's position per frame, in the world frame
        if "head_path" in rec:
            head_path = rec["head_path"]
        elif moving:
            head_path = R.camera_centres(rec["world2cam"])
        else:
            raise ValueError(f"{args.input}: --head_weight / --anchor_headset need the headset's path: the recording holds neither "
                             "head_path [L,3] nor world2cam [L,4,4] (whose camera centres are the path)")
    head_rot = None
    if model.path_head_rot_weight > 0 or model.head_rot_report or (model.head_device_offset != 0).any():
        if "head_rot" in rec:                                           # the device's orientation per frame, device -> world
            head_rot = rec["head_rot"]
        elif moving:
            head_rot = R.camera_rotations(rec["world2cam"])
        else:
            raise ValueError(f"{args.input}: --head_rot_weight / --head_rot_report / --head_offset need the headset's orientation: the "
                             "recording holds neither head_rot [L,3,3] nor world2cam [L,4,4] (whose rotations, transposed, are it)")
    out = model.predict_recording(batch, rec["n_frames"], overlap=O, betas=betas,
                                  window_frames=frames["world2cam"].float() if moving else None, head_path=head_path,
                                  scene_cloud=scene_cloud, head_rot=head_rot)
    nb = 69 if model.name_dataset == "egobody" else 63
    res = {k: v.float().cpu().numpy() for k, v in motion_to_smpl(out["motion"], model.data_type, model.transl_in_feats, nb).items()}
    if "transl" in out:                                                 # anchored: for features without a translation the shift alone
        res["transl"] = out["transl"].float().cpu().numpy()
    res.update({k: out[k].cpu().numpy() for k in ("head_cost", "head_shift", "head_residual", "scene_cost", "scene_hits", "scene_depth",
                                                  "head_rot_cost", "head_rot_residual", "head_rot_mean") if k in out})
    res.update(joints=out["joints"].cpu().numpy(), window_starts=np.asarray(starts, np.int64), path=out["path"].cpu().numpy(),
               seam_cost=out["seam_cost"].cpu().numpy())
    if moving:                                                          # everything above is in the recording's world frame
        res["world2cam_windows"] = frames["world2cam"].numpy()
        if frames["scene_view_count"] is not None:
            res["scene_view_count"] = frames["scene_view_count"].cpu().numpy()
            empty = np.flatnonzero(res["scene_view_count"] == 0)
            if empty.size:
                raise ValueError(f"{args.input}: window {int(empty[0])} (frames {starts[empty[0]]}..{starts[empty[0]] + lengths[empty[0]] - 1}) "
                                 "sees no scene vertex (scene_view_count 0): its camera pose looks away from scene_vertices")
    if args.save_hypotheses:
        res["m_rst_all"] = out["predict"]["m_rst_all"].cpu().numpy()
    d = os.path.dirname(os.path.abspath(args.output))
    os.makedirs(d, exist_ok=True)
    with open(args.output, "wb") as f:                                  # (np.savez would append .npz to a bare name)
        np.savez(f, **res)
    scene_note = f"; mean scene cost of the path {float(out['scene_cost_path'].mean()):.2f} mm" if "scene_cost_path" in out else ""
    if "head_rot_cost_path" in out:
        scene_note += f"; mean rotation cost of the path {float(out['head_rot_cost_path'].mean()):.2f} degrees"
    log.info("%d frames in %d windows of %d (overlap %d), %d hypotheses each; mean seam cost %.1f mm%s; written to %s", rec["n_frames"],
             len(starts), T, O, int(out["predict"]["m_rst_all"].shape[1]),
             float(out["seam_cost"].mean()) if len(starts) > 1 else 0.0, scene_note, args.output)
    return {"file": args.output, "n_frames": rec["n_frames"], "windows": len(starts), "path": out["path"].tolist(),
            "path_cost": float(out["path_cost"])}


# ----------------------------------------------------------------------------- a recording without the interactee -> one with
def load_proscene(model, state: Dict, path: str) -> str:
    """The ProHMR-scene modules of `model` (scene_enc, backbone, flow, as far as it has them) from a SEE-ME state dict (prefix
    ``proscene.``) or from a ProHMR-scene one (no prefix; its smpl*, discriminator.* and loss entries are not read, mld.py:197-203),
    each strictly.  A file without the flow entries is a KeyError naming the first missing key."""
    from .prohmr_head import flow_state_from_checkpoint
    prefix = "proscene." if any(k.startswith("proscene.") for k in state) else ""
    kind = "SEE-ME" if prefix else "ProHMR-scene"
    model.proscene.flow.load_state_dict(flow_state_from_checkpoint(state), strict=True)
    for name in ("scene_enc", "backbone"):
        if hasattr(model.proscene, name):
            sub = {k[len(prefix + name) + 1:]: v for k, v in state.items() if k.startswith(prefix + name + ".")}
            if not sub:
                raise KeyError(f"{path}: a {kind} checkpoint without '{prefix}{name}.*': the model's {name} cannot be loaded from it")
            getattr(model.proscene, name).load_state_dict(sub, strict=True)
    return kind


def estimate_main(argv: Optional[List[str]] = None, datamodule=None, smpl_model=None) -> Dict:
    """estimate.py: a recording .npz WITHOUT the interactee (video or image_crops, center, scale, cam_intrinsics, world2cam,
    scene_vertices) -> the same recording with the interactee's global_orient, body_pose, transl and betas as the
    ProHMR-scene head estimates them, in the recording's world frame: a file predict.py accepts.  --track: the head runs at the
    stored frames only (video_index may skip frames) and the output's motion is ONE track through its samples, filled to every
    recording frame and smoothed (seeme_amd/track.py)."""
    import numpy as np
    from . import crops as CR
    from . import geometry as G
    from . import prohmr_head as PH
    from . import recording as R
    p = build_parser("estimate")
    g = p.add_argument_group("recording")
    g.add_argument("--input", type=str, required=True, help="recording .npz without interactee keys (INTEGRATION.md N)")
    g.add_argument("--output", type=str, required=True, help="where the recording with the interactee goes (.npz)")
    g.add_argument("--video", type=str, default=None, help="decoded frames, uint8 RGB [L,H,W,3] as a .npy (opened memory-mapped), in "
                   "place of the recording's video key")
    g.add_argument("--num_samples", type=int, default=1, help="samples per frame, 1..32: sample 0 is the mode (z = 0)")
    g.add_argument("--seed", type=int, default=None, help="seed of the draws (default: SEED_VALUE)")
    g.add_argument("--save_samples", action="store_true", help="also store interactee_samples_{global_orient,body_pose,transl} [L,S,...]")
    g.add_argument("--chunk_frames", type=int, default=64, help="frames per pass: bounds the scene clouds (scene_points x 12 bytes each)")
    t = p.add_argument_group("one coherent track (seeme_amd/track.py, INTEGRATION.md N)")
    t.add_argument("--track", action="store_true", help="estimate at the STORED frames only (video_index may skip frames), choose one "
                   "sample per stored frame by the min-sum path, fill every recording frame between them and smooth the result")
    t.add_argument("--track_sigma", type=float, default=None, help="override TEST.TRACK_SIGMA: Gaussian width of the filter, frames (0..10)")
    t.add_argument("--track_step_mm", type=float, default=None, help="override TEST.TRACK_STEP_MM: the random walk's step, mm per frame")
    t.add_argument("--track_prior_weight", type=float, default=None,
                   help="override TEST.TRACK_PRIOR_WEIGHT: weight of the flow's log-density against the transitions")
    p.set_defaults(scene_points=None, frames=16)
    args = p.parse_args(argv)
    cfg = load_cfg(args, "test")
    cfg.model.interactee_head = True
    for key, v in (("TRACK_SIGMA", args.track_sigma), ("TRACK_STEP_MM", args.track_step_mm), ("TRACK_PRIOR_WEIGHT", args.track_prior_weight)):
        if v is not None:
            cfg.TEST[key] = v
    if args.scene_points is not None:
        cfg.TEST.SCENE_VIEW_POINTS = args.scene_points
    args.scene_points = P = int(cfg.TEST.get("SCENE_VIEW_POINTS", 20000))
    S = args.num_samples
    if not 1 <= S <= PH.S_MAX:
        raise ValueError(f"--num_samples is {S}: expected 1..{PH.S_MAX}")
    if args.chunk_frames < 1:
        raise ValueError(f"--chunk_frames is {args.chunk_frames}: expected >= 1")
    log = make_logger(cfg, "estimate", 0)
    if not torch.cuda.is_available():
        raise SystemExit("the estimate runs on the HIP path: an MI355X is required (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    model, _dm = build(cfg, dev, args, datamodule, smpl_model)
    if "scene" not in cfg.model.condition or not model.image_backbone:
        raise ValueError("estimate needs the scene encoder and the image backbone: model.condition with 'scene' and 'image', and "
                         "model.image_backbone: true")
    ckpt = args.checkpoint or cfg.TEST.get("CHECKPOINTS")
    if not ckpt:
        raise ValueError("TEST.CHECKPOINTS (or --checkpoint) is required")
    ck = read_checkpoint(ckpt)
    log.info("Loading the %s modules of %s", load_proscene(model, ck.get("state_dict", ck), ckpt), ckpt)
    model = model.to(dev).eval()
    rec = R.load_recording(args.input, video=args.video, require_interactee=False, allow_sparse=args.track)
    n = int(rec["n_frames"])
    vi = np.asarray(rec["video_index"], np.int64)                       # the recording frame of every stored frame: 0..L-1 without --track
    nf = int(vi.shape[0])
    view = R.opencv_views(rec["world2cam"], model.interactee_camera_axes)               # [L,4,4] float64: world -> OpenCV camera
    verts = torch.from_numpy(np.ascontiguousarray(rec["scene_vertices"], np.float32)).to(dev)
    gen = torch.Generator().manual_seed(int(cfg.SEED_VALUE) if args.seed is None else args.seed)
    z = PH.draw_z(nf, S, gen)                                           # drawn for the whole recording: chunking changes nothing
    got = {k: [] for k in ("rotmat", "betas", "cam", "log_prob", "transl", "count")}
    with torch.no_grad():
        for lo in range(0, nf, args.chunk_frames):                      # rows lo..hi-1 of the stored frames
            hi = min(nf, lo + args.chunk_frames)
            fr = vi[lo:hi]
            c, s_ = rec["center"][fr], rec["scale"][fr]
            if "video" in rec:
                frames = torch.from_numpy(np.ascontiguousarray(rec["video"][lo:hi])).to(dev)
                patches = CR.crop_patches_hip(frames, np.arange(hi - lo), PH.head_box(c, s_))
            else:
                patches = torch.from_numpy(np.ascontiguousarray(rec["image_crops"][lo:hi])).to(dev)
            sv = R.scene_views_hip(verts, torch.from_numpy(view[fr]).float().to(dev), P)
            count = sv["count"].cpu()
            if bool((count == 0).any()):
                f = int(fr[int(torch.nonzero(count == 0)[0])])
                raise ValueError(f"{args.input}: frame {f} sees no scene vertex (scene_view_count 0): its camera pose looks away from "
                                 "scene_vertices (is TEST.INTERACTEE_CAMERA_AXES right for this world2cam?)")
            out = model.estimate_interactee(patches, sv["cloud"], c, s_, rec["cam_intrinsics"][fr], z=z[lo:hi])
            for k in ("rotmat", "betas", "cam", "log_prob", "transl"):
                got[k].append(out[k])
            got["count"].append(count)
    cat = {k: torch.cat(v) for k, v in got.items()}
    aa = G.rotmat_to_aa_torch(cat["rotmat"].double()).reshape(nf, S, 72)                # camera frame, every sample
    betas = cat["betas"].double().mean(dim=0)
    # to the world; SMPL turns about the rest pelvis of the betas the body is posed with: the file's betas, the mean
    J0 = R.rest_pelvis(model.smpl_model, betas[None].to(dev))[0].double()
    go, tr = R.camera_body_to_world(aa[:, :, :3], cat["transl"].double()[:, None].expand(nf, S, 3), J0, rec["world2cam"][vi],
                                    model.interactee_camera_axes)
    f32 = lambda t: t.float().cpu().numpy()
    with np.load(args.input, allow_pickle=False) as zf:
        res = {k: zf[k] for k in zf.files}
    res.update(global_orient=f32(go[:, 0]), body_pose=f32(aa[:, 0, 3:]), transl=f32(tr[:, 0]), betas=f32(betas),
               interactee_betas_frames=f32(cat["betas"]), interactee_cam=f32(cat["cam"]), interactee_log_prob=f32(cat["log_prob"]),
               scene_view_count=cat["count"].numpy())
    if args.save_samples:
        res.update(interactee_samples_global_orient=f32(go), interactee_samples_body_pose=f32(aa[:, :, 3:]),
                   interactee_samples_transl=f32(tr))
    trk = None
    if args.track:                                                      # one sample per stored frame, every recording frame filled
        from . import track as TK
        trk = TK.track_interactee(go, aa[:, :, 3:], tr[:, 0], cat["log_prob"], vi, n, model.smpl_model, betas.to(dev),
                                  step_mm=model.track_step_mm, prior_weight=model.track_prior_weight, sigma=model.track_sigma, device=dev)
        res.update(interactee_raw_global_orient=res["global_orient"], interactee_raw_body_pose=res["body_pose"],
                   interactee_raw_transl=res["transl"], interactee_frames=vi, interactee_path=trk["path"].cpu().numpy(),
                   interactee_step_cost=f32(trk["step_cost"]))
        res.update(global_orient=f32(trk["global_orient"]), body_pose=f32(trk["body_pose"]), transl=f32(trk["transl"]))
    d = os.path.dirname(os.path.abspath(args.output))
    os.makedirs(d, exist_ok=True)
    with open(args.output, "wb") as f:
        np.savez(f, **res)
    log.info("%d frames, %d samples each; mean log-probability of the mode %.2f; written to %s", n, S,
             float(cat["log_prob"][:, 0].mean()), args.output)
    if trk is not None:
        log.info("track through %d stored frames: path cost %.2f nats, mean step cost %.2f", nf, float(trk["path_cost"]),
                 float(trk["step_cost"].mean()) if nf > 1 else 0.0)
        return {"file": args.output, "n_frames": n, "num_samples": S, "stored_frames": nf, "path": trk["path"].tolist(),
                "path_cost": float(trk["path_cost"])}
    return {"file": args.output, "n_frames": n, "num_samples": S}


# ----------------------------------------------------------------------------- a predicted recording -> frames to look at
RENDER_UP = {"egobody": (0.0, 1.0, 0.0), "gimo": (0.0, 1.0, 0.0)}     # the datasets' vertical axis
RENDER_PALETTE = ((96, 152, 232), (236, 146, 84))                     # the wearer, the interactee
RENDER_BG = (24, 24, 28)


def _parse_size(text: str):
    m = re.match(r"^(\d+)x(\d+)$", str(text))
    if not m or not (1 <= int(m.group(1)) <= 4096 and 1 <= int(m.group(2)) <= 4096):
        raise ValueError(f"--size is {text!r}: expected HxW with H and W in 1..4096, e.g. 480x640")
    return int(m.group(1)), int(m.group(2))


def render_main(argv: Optional[List[str]] = None, smpl_model=None) -> Dict:
    """render.py: a recording .npz and the motion .npz that predict.py wrote for it -> uint8 frames [L,H,W,3] as a .npy (and PNGs):
    the wearer's and the interactee's SMPL bodies, flat-shaded in two colours, and the scene cloud as points coloured by height, seen
    from one fixed orbit camera or through the recording's own headset path.  No checkpoint is read."""
    import numpy as np
    from . import recording as R
    from . import render as RD
    from .smpl import SMPL
    p = build_parser("render")
    g = p.add_argument_group("rendering")
    g.add_argument("--input", type=str, required=True, help="recording .npz (INTEGRATION.md K): the interactee, the scene, world2cam")
    g.add_argument("--motion", type=str, required=True, help="the wearer's motion .npz, as predict.py writes it")
    g.add_argument("--output", type=str, required=True, help="where the frames go: uint8 [L,H,W,3] as a .npy")
    g.add_argument("--png_dir", type=str, default=None, help="also write one PNG per frame into this directory")
    g.add_argument("--view", type=str, default="orbit", choices=["orbit", "ego"],
                   help="orbit: one fixed camera for the whole recording; ego: the recording's world2cam [L,4,4]")
    g.add_argument("--azimuth", type=float, default=30.0, help="orbit: degrees around --up")
    g.add_argument("--elevation", type=float, default=20.0, help="orbit: degrees above the plane across --up")
    g.add_argument("--fov", type=float, default=60.0, help="degrees spanned by the image width")
    g.add_argument("--up", type=float, nargs=3, default=None, help="the world's vertical axis (default: the dataset's)")
    g.add_argument("--camera", type=str, default=None, help="a .npy world2cam [4,4] or [L,4,4] in place of --view")
    g.add_argument("--size", type=str, default="480x640", help="HxW")
    g.add_argument("--point_size", type=int, default=2, help="side of a scene point's square in pixels, 1..8")
    g.add_argument("--near", type=float, default=0.05, help="near plane in metres; a face with a corner nearer than it is dropped")
    g.add_argument("--chunk_mb", type=float, default=256.0, help="bound on the device memory of one chunk of frames")
    p.set_defaults(scene_points=20000)                                 # the scene cloud is thinned to at most this many points
    args = p.parse_args(argv)
    cfg = load_cfg(args, "test")
    log = make_logger(cfg, "render", 0)
    H, W = _parse_size(args.size)
    if args.scene_points < 0:
        raise ValueError(f"--scene_points is {args.scene_points}: expected >= 0 (0 draws no scene)")
    if not 1 <= args.point_size <= RD.POINT_MAX:
        raise ValueError(f"--point_size is {args.point_size}: expected 1..{RD.POINT_MAX}")
    if not args.chunk_mb > 0:
        raise ValueError(f"--chunk_mb is {args.chunk_mb}: expected a positive number of MiB")
    name = str(cfg.DATASET_NAME)
    up = tuple(args.up) if args.up is not None else RENDER_UP.get(name)
    if up is None:
        raise ValueError(f"DATASET_NAME is {name!r}: no default vertical axis is known for it, give --up x y z")
    rec = R.load_recording(args.input)
    n = int(rec["n_frames"])
    mot = RD.load_motion(args.motion, n)
    if args.camera is not None:
        cam = np.asarray(np.load(args.camera, allow_pickle=False), np.float64)
        if cam.shape == (4, 4):
            cam = cam[None]
        if cam.shape not in ((1, 4, 4), (n, 4, 4)):
            raise ValueError(f"--camera {args.camera}: world2cam is {cam.shape}: expected [4,4] or [{n},4,4] (L = {n})")
        R.check_world2cam(cam, cam.shape[0], f"--camera {args.camera}")
    elif args.view == "ego":
        if "world2cam" not in rec:
            raise ValueError(f"{args.input}: --view ego needs the recording's world2cam [L,4,4] (the headset path), and the file holds none; "
                             "use --view orbit or --camera")
        cam = rec["world2cam"]
    else:
        cam = None                                                      # fitted below, once the bodies are known
    if smpl_model is None:
        path = str(cfg.model.smpl_path)
        smpl_model = SMPL(model_path=path, gender="neutral") if os.path.exists(path) else SMPL.synthetic(int(cfg.SEED_VALUE))
    faces1 = smpl_model.faces_tensor.detach().cpu().long()
    V = int(smpl_model.v_template.shape[0])
    solid = (faces1[:, 0] != faces1[:, 1]) & (faces1[:, 1] != faces1[:, 2]) & (faces1[:, 0] != faces1[:, 2])
    if faces1.numel() == 0 or not bool(solid.any()) or int(faces1.min()) < 0 or int(faces1.max()) >= V:
        raise ValueError("the SMPL model's face table holds no non-degenerate face inside its vertices (the synthetic stand-in has "
                         "none): set model.smpl_path to a real SMPL model file to render bodies")
    if not torch.cuda.is_available():
        raise SystemExit("rendering runs on the HIP path: an MI355X is required (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    smpl_model = smpl_model.to(dev)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)

    def pose69(bp):                                                     # GIMO's 21 body joints, padded as mld.py:807-813 does
        return np.concatenate([bp, np.zeros((bp.shape[0], 69 - bp.shape[1]), np.float32)], axis=1) if bp.shape[1] < 69 else bp

    people = []                                                         # the wearer first: palette row 0
    for src, betas in ((mot, rec.get("wearer_betas", np.zeros(10, np.float32))), (rec, rec["betas"])):
        people.append({"global_orient": to(src["global_orient"]), "body_pose": to(pose69(src["body_pose"])), "transl": to(src["transl"]),
                       "betas": to(betas)[None]})

    def bodies(lo, hi, verts=True):
        out = [smpl_model(betas=q["betas"], body_pose=q["body_pose"][lo:hi], global_orient=q["global_orient"][lo:hi],
                          transl=q["transl"][lo:hi], return_verts=verts) for q in people]
        return torch.cat([o.vertices if verts else o.joints[:, :24] for o in out], dim=1)

    faces = torch.cat([faces1, faces1 + V]).to(torch.int32).to(dev)
    mesh_of_face = torch.cat([torch.zeros(faces1.shape[0]), torch.ones(faces1.shape[0])]).to(torch.int32).to(dev)
    palette = torch.tensor(RENDER_PALETTE, dtype=torch.uint8, device=dev)
    cloud = rec.get("scene", rec.get("scene_vertices"))
    points = point_rgb = None
    if cloud is not None and args.scene_points > 0:
        cloud = cloud[np.isfinite(cloud).all(axis=1)]
        cloud = cloud[::max(1, -(-cloud.shape[0] // args.scene_points))]   # every k-th point, down to at most --scene_points
        if cloud.shape[0]:
            points, point_rgb = to(cloud), torch.from_numpy(RD.height_colours(cloud, up)).to(dev)
    with torch.no_grad():
        if cam is None:
            cam = RD.orbit_camera(bodies(0, n, verts=False).cpu().numpy(), args.azimuth, args.elevation, args.fov, up, aspect=W / H,
                                  margin=1.25)[None]                    # the joints of both bodies, with room for the flesh around them
        cams = to(cam)
        K = RD.intrinsics(args.fov, (H, W))
        d = os.path.dirname(os.path.abspath(args.output))
        os.makedirs(d, exist_ok=True)
        if args.png_dir:
            os.makedirs(args.png_dir, exist_ok=True)
        frames = np.lib.format.open_memmap(args.output, "w+", np.uint8, (n, H, W, 3))
        per_frame = H * W * (8 + 4 + 4 + 3) + 2 * V * (12 + 16)          # keys, ids, inverse depth, rgb; vertices and their projections
        step = max(1, min(n, int(args.chunk_mb * (1 << 20)) // per_frame))
        dropped = 0
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            verts = bodies(lo, hi)
            c = cams[lo:hi] if cams.shape[0] > 1 else cams
            r = RD.render_hip(verts, faces, c, K, (H, W), points=points, near=args.near, point_size=args.point_size,
                              chunk_mb=args.chunk_mb)
            rgb = RD.shade_hip(verts, faces, c, r["ids"], mesh_of_face, palette, points, point_rgb, RENDER_BG).cpu().numpy()
            dropped += int(r["dropped"].sum())
            frames[lo:hi] = rgb
            if args.png_dir:
                for f in range(lo, hi):
                    RD.write_png(os.path.join(args.png_dir, f"frame_{f:06d}.png"), rgb[f - lo])
        frames.flush()
        del frames
    log.info("%d frames of %d x %d (%s), %d scene points; %d faces dropped for a corner outside the view volume (near %.3f m); written to %s",
             n, H, W, "camera file" if args.camera else args.view, 0 if points is None else int(points.shape[0]), dropped, args.near,
             args.output)
    return {"file": args.output, "n_frames": n, "size": (H, W), "dropped": dropped, "scene_points": 0 if points is None else int(points.shape[0])}
