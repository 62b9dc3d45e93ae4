"""Training-loop options without a GPU: the library surface of seeme_adamw_step_ex / seeme_grad_norm and their argument checks
(none of which launches), the EMA decay schedule, the PyTorch fallback (TorchAdamWStep) against torch's own operations and the
float64 reference, config keys and CLI options, the checkpoint layout with EMA weights, and the name rules of best.ckpt."""
import ctypes as C
import os

import pytest
import torch

from conftest import REPO, rel_err
from seeme_amd import _lib as L
from seeme_amd import cli
from seeme_amd.optim import TorchAdamWStep, ema_decay_at, reference_step_f64

CFG = os.path.join(REPO, "configs", "config_mld_egobody.yaml")


# ----------------------------------------------------------------------------- library surface, bad arguments
def test_library_surface():
    header = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    lib = L.lib()
    for name in ("seeme_adamw_step_ex", "seeme_adamw_ex_bytes", "seeme_grad_norm", "seeme_grad_norm_workspace_bytes"):
        assert name + "(" in header, name
        assert name in L.exported_symbols() and hasattr(lib, name), name
    assert C.sizeof(L.AdamWEx) == lib.seeme_adamw_ex_bytes()


def _ex(**kw):
    a = L.AdamWEx()
    a.chunks = a.params = a.grads = a.exp_avg = a.exp_avg_sq = 64       # never dereferenced: every case returns before a launch
    a.n_chunks, a.lr, a.step, a.beta1, a.beta2, a.eps, a.weight_decay = 1, 1e-3, 1.0, 0.9, 0.999, 1e-8, 1e-2
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_bad_arguments_return_before_any_launch():
    lib = L.lib()
    assert lib.seeme_adamw_step_ex(None, None) != 0
    assert b"NULL" in lib.seeme_last_error()
    assert lib.seeme_adamw_step_ex(C.byref(_ex(n_chunks=0)), None) == 0
    assert lib.seeme_adamw_step_ex(C.byref(_ex(params=0)), None) != 0
    for d in (-0.1, 1.0):
        assert lib.seeme_adamw_step_ex(C.byref(_ex(ema_decay=d)), None) != 0
        assert b"ema_decay" in lib.seeme_last_error()
    assert lib.seeme_grad_norm_workspace_bytes(0) == 0 and lib.seeme_grad_norm_workspace_bytes(-3) == 0
    assert lib.seeme_grad_norm_workspace_bytes(5) == 40
    assert lib.seeme_grad_norm(64, 0, 64, 1.0, 64, 64, 0, None) == 0
    assert lib.seeme_grad_norm(64, 2, 64, 0.0, 64, 64, 16, None) != 0
    assert b"max_norm" in lib.seeme_last_error()
    assert lib.seeme_grad_norm(0, 2, 64, 1.0, 64, 64, 16, None) != 0            # NULL table
    assert lib.seeme_grad_norm(64, 2, 64, 1.0, 64, 64, 8, None) != 0            # short workspace
    assert lib.seeme_grad_norm(64, 2, 64, 1.0, 64, 68, 16, None) != 0           # misaligned workspace
    assert b"aligned" in lib.seeme_last_error()


# ----------------------------------------------------------------------------- decay schedule
def test_decay_schedule():
    d = 0.9
    assert ema_decay_at(d, True, 1) == 2.0 / 11.0
    first = next(t for t in range(1, 1000) if (1.0 + t) / (10.0 + t) >= d)
    assert first == 80
    for t in range(1, 200):
        got = ema_decay_at(d, True, t)
        assert (got == d) if t >= first else (got == (1.0 + t) / (10.0 + t) < d), t
        assert ema_decay_at(d, False, t) == d


# ----------------------------------------------------------------------------- the PyTorch fallback on CPU tensors
SIZES = [(1,), (3, 5, 7), (20001,)]


def _params(seed=0):
    return [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(seed + i))) for i, s in enumerate(SIZES)]


@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("warmup", [True, False])
def test_fallback_matches_torch_bitwise_and_float64_reference(clip, warmup):
    d = 0.9
    pa, pb = _params(), _params()
    oa, ob = torch.optim.AdamW(pa, lr=1e-3), torch.optim.AdamW(pb, lr=1e-3)
    st = TorchAdamWStep(ob, ema_decay=d, ema_warmup=warmup, grad_clip_norm=clip)
    ea = [p.detach().clone() for p in pa]
    p64, e64 = [p.detach().double() for p in pa], [p.detach().double() for p in pa]
    m64, v64 = [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64]
    g = torch.Generator().manual_seed(5)
    lr = 1e-3
    for it in range(3):
        if it == 2:
            lr = 3e-4
            for o in (oa, ob):
                o.param_groups[0]["lr"] = lr
        grads = [torch.randn(p.shape, generator=g) for p in pa]
        for x, y, gr in zip(pa, pb, grads):
            x.grad, y.grad = gr.clone(), gr.clone()
        # torch's own operations
        if clip:
            torch.nn.utils.clip_grad_norm_(pa, clip)
        oa.step()
        with torch.no_grad():
            for e, p in zip(ea, pa):
                e.lerp_(p, 1.0 - ema_decay_at(d, warmup, it + 1))
        st.step()
        # float64
        n64 = torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads))
        scale = min(1.0, clip / (float(n64) + 1e-6)) if clip else None
        reference_step_f64(p64, [gr.double() for gr in grads], m64, v64, e64, it + 1, lr, ema_decay=d, ema_warmup=warmup, grad_scale=scale)
        for i, (x, y) in enumerate(zip(pa, pb)):
            assert torch.equal(x.detach(), y.detach()) and torch.equal(ea[i], st.shadow[y])
            assert torch.equal(y.grad, grads[i])                                     # the fallback leaves p.grad unscaled
            assert rel_err(y.detach().numpy(), p64[i].numpy()) < 2e-6
            assert rel_err(st.shadow[y].numpy(), e64[i].numpy()) < 2e-6
            assert rel_err(ob.state[y]["exp_avg"].numpy(), m64[i].numpy()) < 2e-6
            assert rel_err(ob.state[y]["exp_avg_sq"].numpy(), v64[i].numpy()) < 2e-6
        if clip:
            assert abs(float(st.last_grad_norm[0]) - float(n64)) < 1e-6 * float(n64)
            assert abs(float(st.last_grad_norm[1]) - scale) < 1e-6


# ----------------------------------------------------------------------------- config keys, CLI options
def _cpu_model(**train):
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(CFG)
    for k, v in train.items():
        cfg.TRAIN[k] = v
    return MLD(cfg, SyntheticEgoDataModule(), smpl_model=SMPL.synthetic(1, V=64)), cfg


def test_config_defaults_and_range_checks():
    m, cfg = _cpu_model()
    assert cfg.TRAIN.EMA_DECAY == 0.0 and cfg.TRAIN.EMA_WARMUP is True and cfg.TRAIN.GRAD_CLIP_NORM == 0.0 and cfg.TEST.USE_EMA is False
    assert m.ema_decay == 0.0 and m.grad_clip_norm == 0.0 and m.ema_warmup is True
    for key, bad in (("EMA_DECAY", 1.0), ("EMA_DECAY", -0.1), ("EMA_DECAY", "x"), ("GRAD_CLIP_NORM", -1.0), ("GRAD_CLIP_NORM", float("inf")),
                     ("EMA_WARMUP", 1)):
        with pytest.raises(ValueError, match="TRAIN." + key):
            _cpu_model(**{key: bad})
    with pytest.raises(RuntimeError):
        with m.ema_scope():
            pass


def test_cli_options_override_the_keys(tmp_path):
    args = cli.build_parser("train").parse_args(["--cfg", CFG, "--folder", str(tmp_path), "--ema_decay", "0.99", "--grad_clip", "0.5",
                                                 "--val_every", "3", "--val_batches", "2"])
    cfg = cli.load_cfg(args, "train")
    assert cfg.TRAIN.EMA_DECAY == 0.99 and cfg.TRAIN.GRAD_CLIP_NORM == 0.5 and cfg.LOGGER.VAL_EVERY_STEPS == 3 and args.val_batches == 2
    d = cli.load_cfg(cli.build_parser("train").parse_args(["--cfg", CFG, "--folder", str(tmp_path)]), "train")
    assert d.LOGGER.VAL_EVERY_STEPS == 10 and d.TRAIN.EMA_DECAY == 0.0
    t = cli.load_cfg(cli.build_parser("test").parse_args(["--cfg", CFG, "--folder", str(tmp_path), "--use_ema"]), "test")
    assert t.TEST.USE_EMA is True
    assert cli.load_cfg(cli.build_parser("test").parse_args(["--cfg", CFG, "--folder", str(tmp_path)]), "test").TEST.USE_EMA is False


# ----------------------------------------------------------------------------- checkpoints
def test_checkpoint_round_trip_with_ema(tmp_path):
    m, _ = _cpu_model(EMA_DECAY=0.9)
    m.configure_optimizers()
    names = {n for n, p in m.named_parameters() if p.requires_grad}
    assert set(m.ema_state_dict()) == names and names < set(m.state_dict())
    with torch.no_grad():
        for i, e in enumerate(m.ema_state_dict().values()):
            e.add_(0.001 * (i + 1))
    path = str(tmp_path / "checkpoints" / "epoch=0.ckpt")
    cli.save_checkpoint(path, m, 0, 2)
    ck = cli.read_checkpoint(path)
    assert set(ck["ema_state_dict"]) == names and set(ck["state_dict"]) == set(m.state_dict())
    m2, _ = _cpu_model(EMA_DECAY=0.9)
    m2.configure_optimizers()
    m2.load_ema_state_dict(ck["ema_state_dict"])
    for k, v in m.ema_state_dict().items():
        assert torch.equal(m2.ema_state_dict()[k], v)
    with pytest.raises(RuntimeError):
        m2.load_ema_state_dict({k: v for k, v in list(ck["ema_state_dict"].items())[1:]})
    # the scope swaps in place and restores the raw weights, also on an exception; no step and no second scope inside
    raw = {k: v.detach().clone() for k, v in m2.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in m2.state_dict().items()}
    with pytest.raises(KeyError):
        with m2.ema_scope():
            assert all(torch.equal(m2.state_dict()[k], v) for k, v in ck["ema_state_dict"].items())
            with pytest.raises(RuntimeError):
                with m2.ema_scope():
                    pass
            with pytest.raises(RuntimeError):
                m2.optimizer_update()
            raise KeyError("x")
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in raw.items())
    assert {k: v.data_ptr() for k, v in m2.state_dict().items()} == ptrs
    # a checkpoint without EMA weights: no key, and --use_ema names the file
    m3, _ = _cpu_model()
    m3.configure_optimizers()
    plain = str(tmp_path / "checkpoints" / "epoch=1.ckpt")
    cli.save_checkpoint(plain, m3, 1, 4)
    ck3 = cli.read_checkpoint(plain)
    assert "ema_state_dict" not in ck3
    with pytest.raises(ValueError, match="epoch=1.ckpt"):
        cli.overlay_ema(m3, ck3, plain)
    assert cli.overlay_ema(m3, ck, path) == len(names)
    assert all(torch.equal(m3.state_dict()[k], v) for k, v in ck["ema_state_dict"].items())


def test_best_ckpt_name_rules(tmp_path):
    assert cli.BEST_CKPT == "best.ckpt" and cli.CKPT_RE.match(cli.BEST_CKPT) is None
    m = torch.nn.Linear(2, 2)
    m.optimizer = None
    d = tmp_path / "exp" / "checkpoints"
    cli.save_checkpoint(str(d / "epoch=3.ckpt"), m, 3, 8)
    cli.save_checkpoint(str(d / cli.BEST_CKPT), m, 7, 16, monitor={"epoch": 7, "MPJPE": 0.25})
    assert cli.newest_checkpoint(str(tmp_path / "exp")).endswith("epoch=3.ckpt")
    assert cli.read_checkpoint(str(d / cli.BEST_CKPT))["monitor"] == {"epoch": 7, "MPJPE": 0.25}
