"""The training loop's options on the GPU: seeme_adamw_step_ex (gradient scale and EMA shadow in the AdamW pass) and seeme_grad_norm
against float64, their equivalence to the plain step, MLD with EMA and clipping (eager and captured), the weight images after a
training step and inside ema_scope(), and train_main / test_main with validation, best.ckpt, --use_ema and resume."""
import itertools
import math
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from seeme_amd import _lib as L
from seeme_amd.optim import FusedAdamWStep, TorchAdamWStep, ema_decay_at, reference_step_f64
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu
CFG = os.path.join(REPO, "configs", "config_mld_egobody.yaml")
# chunk edges (16384 elements per workgroup), the 16-byte vector body and its tail, and one tensor that starts one element into
# its storage: no 16-byte alignment, the scalar path
NUMELS = [1, 3, 4, 5, 16383, 16384, 16385, 40000]
VIEW = 1000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _tensors(dev, seed=0):
    ts = [torch.randn(n, generator=torch.Generator().manual_seed(seed + i)).to(dev) for i, n in enumerate(NUMELS)]
    base = torch.randn(VIEW + 1, generator=torch.Generator().manual_seed(seed + 99)).to(dev)
    ts.append(base[1:])
    assert ts[-1].data_ptr() % 16 == 4 and ts[-1].is_contiguous()
    return ts


def _params(dev):
    return [torch.nn.Parameter(t) for t in _tensors(dev)]


def _grads(dev, it, scale=1.0):
    return [scale * g for g in _tensors(dev, seed=1000 * (it + 1))]


def _norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


# ----------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("ema,clip,device_step", list(itertools.product([None, (0.9, True), (0.9, False)], [0.0, 0.5], [False, True])))
def test_step_ex_vs_float64_reference(dev, ema, clip, device_step):
    """Three steps (the third after an LR change) through FusedAdamWStep; p, m, v and e within 2e-6 relative of the float64
    definition, whose scale comes from the float64 norm."""
    d, warm = ema if ema else (0.0, True)
    ps = _params(dev)
    opt = torch.optim.AdamW(ps, lr=1e-3)
    f = FusedAdamWStep(opt, ema_decay=d, ema_warmup=warm, grad_clip_norm=clip)
    f._force_ex = True                                       # also with both options off: NULL ema, NULL grad_scale
    p64 = [p.detach().double() for p in ps]
    e64 = [p.detach().double() for p in ps] if ema else None
    m64, v64 = [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64]
    lr = 1e-3
    for it in range(3):
        if it == 2:
            lr = 3e-4
            opt.param_groups[0]["lr"] = lr
        grads = _grads(dev, it)
        versions = [p._version for p in ps]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        f.step(device_step=device_step)
        n64 = _norm64(grads)
        scale = min(1.0, clip / (n64 + 1e-6)) if clip else None
        reference_step_f64(p64, [g.double() for g in grads], m64, v64, e64, it + 1, lr, ema_decay=d, ema_warmup=warm, grad_scale=scale)
        worst = 0.0
        for i, p in enumerate(ps):
            assert torch.equal(p.grad, grads[i])                                    # g is read, never written
            assert p._version > versions[i]
            worst = max(worst, rel_err(_np(p), _np(p64[i])), rel_err(_np(opt.state[p]["exp_avg"]), _np(m64[i])),
                        rel_err(_np(opt.state[p]["exp_avg_sq"]), _np(v64[i])))
            if ema:
                worst = max(worst, rel_err(_np(f.shadow[p]), _np(e64[i])))
        print(f"step {it}: worst relative error {worst:.3e}")
        assert worst < 2e-6, (it, worst)
        if clip:
            got = f.last_grad_norm.cpu()
            assert abs(float(got[0]) - n64) < 1e-6 * n64 and abs(float(got[1]) - scale) < 1e-6
    assert float(opt.state[ps[0]]["step"]) == 3.0


@pytest.mark.parametrize("device_step", [False, True])
def test_step_ex_without_options_is_the_old_step_bitwise(dev, device_step):
    pa, pb = _params(dev), _params(dev)
    oa, ob = torch.optim.AdamW(pa, lr=1e-3), torch.optim.AdamW(pb, lr=1e-3)
    fa, fb = FusedAdamWStep(oa), FusedAdamWStep(ob)
    fb._force_ex = True
    for it in range(3):
        if it == 2:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 3e-4
        for x, y, g in zip(pa, pb, _grads(dev, it)):
            x.grad, y.grad = g.clone(), g.clone()
        fa.step(device_step=device_step)
        fb.step(device_step=device_step)
        for x, y in zip(pa, pb):
            assert torch.equal(x.detach(), y.detach())
            assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"]) and torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])


# ----------------------------------------------------------------------------- seeme_grad_norm alone
def _tables(tensors, dev):
    chunks = [[t, min(16384, x.numel() - off), off, 0] for t, x in enumerate(tensors) for off in range(0, x.numel(), 16384)]
    return (torch.tensor(chunks, dtype=torch.int32).to(dev), len(chunks),
            torch.tensor([x.data_ptr() for x in tensors], dtype=torch.int64).to(dev))


def _grad_norm(grads, max_norm, dev):
    ch, n, gp = _tables(grads, dev)
    out = torch.full((2,), -1.0, dtype=torch.float32, device=dev)
    ws = torch.empty(L.lib().seeme_grad_norm_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    L.check(L.lib().seeme_grad_norm(ch.data_ptr(), n, gp.data_ptr(), float(max_norm), out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                    L.current_stream()), "seeme_grad_norm")
    torch.cuda.synchronize()
    return out.cpu()


def test_grad_norm_value_bits_and_scale(dev):
    grads = _grads(dev, 0)
    n64 = _norm64(grads)
    a, b = _grad_norm(grads, 0.5, dev), _grad_norm(grads, 0.5, dev)
    assert torch.equal(a, b)                                                       # no atomics: equal bits
    assert abs(float(a[0]) - n64) < 1e-6 * n64
    hs = [torch.nn.Parameter(torch.empty_like(g)) for g in grads]
    for h, g in zip(hs, grads):
        h.grad = g.clone()
    tn = torch.nn.utils.clip_grad_norm_(hs, 0.5)
    want = float(torch.clamp(0.5 / (tn + 1e-6), max=1.0))
    assert 0 < want < 1 and abs(float(a[1]) - want) < 1e-6
    below = _grad_norm(grads, 10.0 * n64, dev)
    assert float(below[1]) == 1.0 and float(below[0]) == float(a[0])
    bad = [g.clone() for g in grads]
    bad[5][777] = float("inf")
    got = _grad_norm(bad, 0.5, dev)
    assert math.isinf(float(got[0])) and float(got[1]) == 0.0


def test_clip_above_the_norm_is_the_unclipped_step_bitwise(dev):
    pa, pb = _params(dev), _params(dev)
    oa, ob = torch.optim.AdamW(pa, lr=1e-3), torch.optim.AdamW(pb, lr=1e-3)
    fa, fb = FusedAdamWStep(oa), FusedAdamWStep(ob, grad_clip_norm=1e6)
    for it in range(2):
        for x, y, g in zip(pa, pb, _grads(dev, it)):
            x.grad, y.grad = g.clone(), g.clone()
        fa.step()
        fb.step()
        assert float(fb.last_grad_norm[1]) == 1.0
        for x, y in zip(pa, pb):
            assert torch.equal(x.detach(), y.detach())


def test_hip_step_agrees_with_the_torch_fallback(dev):
    """The twin: clip_grad_norm_ + torch.optim.AdamW + _foreach_lerp_ on the same device tensors (other association of the fp32
    operations, and torch's norm is fp32: 2e-6, the bound of the existing AdamW test)."""
    pa, pb = _params(dev), _params(dev)
    oa, ob = torch.optim.AdamW(pa, lr=1e-3), torch.optim.AdamW(pb, lr=1e-3)
    fa, fb = TorchAdamWStep(oa, ema_decay=0.9, grad_clip_norm=0.5), FusedAdamWStep(ob, ema_decay=0.9, grad_clip_norm=0.5)
    for it in range(3):
        for x, y, g in zip(pa, pb, _grads(dev, it)):
            x.grad, y.grad = g.clone(), g.clone()
        fa.step()
        fb.step()
        for x, y in zip(pa, pb):
            assert rel_err(_np(y), _np(x)) < 2e-6 and rel_err(_np(fb.shadow[y]), _np(fa.shadow[x])) < 2e-6


# ----------------------------------------------------------------------------- MLD
def _mld(dev, T=24, **train):
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(CFG)
    for k, v in train.items():
        cfg.TRAIN[k] = v
    dm = SyntheticEgoDataModule(nfeats=cfg.model.nfeats, T=T, n_points=384, device=dev, pose_dim=cfg.model.nfeats - 3)
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser)
    return model.to(dev), dm


def _eval(model, batch, dev):
    g = torch.Generator().manual_seed(11)
    B = batch[0].shape[0]
    lat, cn = torch.randn(B, 1, 256, generator=g).to(dev), torch.randn(1, B, 256, generator=g).to(dev)
    was = model.training
    model.eval()
    with torch.no_grad():
        torch.manual_seed(3)
        rs = model.ego_eval(batch, latents=lat, cond_noise=cn)
    model.train(was)
    return rs["m_rst"].clone(), rs["joints_rst"].clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def trained(dev):
    """MLD with EMA 0.9 and clipping at 0.5 after three optimizer_steps (B = 4, T = 24), with what the tests below compare:
    parameter snapshots after each step, the sample drawn BEFORE training (which builds the weight images), the addresses."""
    model, dm = _mld(dev, EMA_DECAY=0.9, GRAD_CLIP_NORM=0.5)
    model.train()
    tb, eb = dm.batch(4, idx=3), dm.batch(4, idx=5, split="test")
    model.configure_optimizers()
    ptrs = {n: p.data_ptr() for n, p in model.named_parameters()}
    before = _eval(model, eb, dev)
    snaps = [{n: p.detach().double().clone() for n, p in model.named_parameters() if p.requires_grad}]
    for _ in range(3):
        model.optimizer_step(model.training_step(tb))
        snaps.append({n: p.detach().double().clone() for n, p in model.named_parameters() if p.requires_grad})
    torch.cuda.synchronize()
    return dict(model=model, dm=dm, eb=eb, ptrs=ptrs, before=before, snaps=snaps)


def test_mld_shadows_follow_the_recurrence_and_norm_of_the_bucket(dev, trained):
    model, snaps = trained["model"], trained["snaps"]
    e = {n: v.clone() for n, v in snaps[0].items()}
    for t in (1, 2, 3):
        for n in e:
            e[n] += (snaps[t][n] - e[n]) * (1.0 - ema_decay_at(0.9, True, t))
    got = model.ema_state_dict()
    assert set(got) == set(e)
    worst = max(rel_err(_np(got[n]), _np(e[n])) for n in e)
    print(f"shadows vs float64 recurrence: {worst:.3e}")
    assert worst < 2e-6, worst
    moved = [n for n in e if not torch.equal(snaps[0][n], snaps[3][n])]
    still = [n for n in e if n not in moved]
    assert moved and all(torch.equal(got[n].double(), snaps[0][n]) for n in still)     # off the path: the shadow equals the tensor
    n64 = float(model.grad_bucket().flat.double().norm())
    ln = model.last_grad_norm.cpu()
    assert abs(float(ln[0]) - n64) < 1e-6 * n64 and abs(float(ln[1]) - min(1.0, 0.5 / (n64 + 1e-6))) < 1e-6


def test_weight_images_follow_training_and_ema_scope(dev, trained):
    """The hazard: the AdamW kernels write through raw pointers, and the sampling-side images are cached on (data_ptr, _version)."""
    model, eb = trained["model"], trained["eb"]
    raw = _eval(model, eb, dev)
    assert _same(raw, _eval(model, eb, dev))                                            # the sampling path repeats its bits
    assert not _same(raw, trained["before"])
    fresh, _ = _mld(dev)
    fresh.load_state_dict(model.state_dict())
    assert _same(raw, _eval(fresh, eb, dev))
    fresh.load_state_dict({k: v.clone() for k, v in model.ema_state_dict().items()}, strict=False)
    want_ema = _eval(fresh, eb, dev)
    with model.ema_scope():
        inside = _eval(model, eb, dev)
        with pytest.raises(RuntimeError):
            model.optimizer_step(None)
        with pytest.raises(RuntimeError):
            with model.ema_scope():
                pass
    assert _same(inside, want_ema) and not _same(inside, raw)
    assert _same(raw, _eval(model, eb, dev))
    assert {n: p.data_ptr() for n, p in model.named_parameters()} == trained["ptrs"]
    off, _ = _mld(dev)
    off.configure_optimizers()
    with pytest.raises(RuntimeError):
        with off.ema_scope():
            pass


def test_captured_step_with_ema_and_clip_equals_eager(dev):
    """Three replays of the captured step against three eager steps of a twin optimiser that starts from the same parameters,
    moments, step count and shadows and is fed the gradients each replay left in the bucket: 1e-5, the bound of
    test_capture_training_step_replay_equals_eager."""
    model, dm = _mld(dev, EMA_DECAY=0.9, GRAD_CLIP_NORM=0.5)
    model.train()
    tb = dm.batch(4, idx=3)
    replay = model.capture_training_step(tb, warmup=1)
    torch.cuda.synchronize()
    bucket, opt, fused = model.grad_bucket(), model.optimizer, model._fused_adamw
    twin = [torch.nn.Parameter(p.detach().clone()) for p in bucket.params]
    ot = torch.optim.AdamW(twin, lr=opt.param_groups[0]["lr"])
    ft = FusedAdamWStep(ot, ema_decay=0.9, grad_clip_norm=0.5)
    t0 = float(opt.state[bucket.params[0]]["step"])
    for p, q in zip(bucket.params, twin):
        ot.state[q] = {"step": torch.tensor(t0), "exp_avg": opt.state[p]["exp_avg"].clone(), "exp_avg_sq": opt.state[p]["exp_avg_sq"].clone()}
        ft.shadow[q].copy_(fused.shadow[p])
    for it in range(3):
        if it == 2:
            opt.param_groups[0]["lr"] = ot.param_groups[0]["lr"] = 0.5 * opt.param_groups[0]["lr"]
        versions = [p._version for p in bucket.params]
        loss = replay()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and float(opt.state[bucket.params[0]]["step"]) == t0 + it + 1
        assert all(p._version > v for p, v in zip(bucket.params, versions))
        for p, q in zip(bucket.params, twin):
            q.grad = bucket.views[id(p)].clone()
        ft.step()
        # (the twin's chunk order may differ from the bucket's: the double sums agree to 1e-15, the fp32 results to one ulp)
        assert rel_err(_np(ft.last_grad_norm), _np(fused.last_grad_norm)) < 2.4e-7 and 0 < float(fused.last_grad_norm[1]) <= 1
        worst = max(max(rel_err(_np(p), _np(q)), rel_err(_np(fused.shadow[p]), _np(ft.shadow[q]))) for p, q in zip(bucket.params, twin))
        print(f"replay {it}: graph vs eager {worst:.3e}")
        assert worst < 1e-5, (it, worst)


# ----------------------------------------------------------------------------- train_main / test_main
def _common(folder):
    return ["--cfg", CFG, "--batch_size", "4", "--nodebug", "--folder", str(folder), "--frames", "24", "--iters_per_epoch", "2"]


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    from seeme_amd import cli
    d = tmp_path_factory.mktemp("val")
    r = cli.train_main(_common(d) + ["--epochs", "2", "--val_every", "1", "--val_batches", "1", "--ema_decay", "0.9"])
    return r


def test_train_main_validates_and_keeps_the_training_stream(dev, run, tmp_path):
    from seeme_amd import cli
    assert run["step"] == 4 and np.isfinite(run["total"])
    assert np.isfinite(run["val_MPJPE"]) and np.isfinite(run["val_loss_total"]) and run["best"]["epoch"] in (0, 1)
    assert run["best"]["MPJPE"] <= run["val_MPJPE"] + 1e-6 and "grad_norm" not in run      # (the logged value is rounded to 6 digits)
    assert sorted(os.listdir(run["checkpoints"])) == ["best.ckpt", "epoch=0.ckpt", "epoch=1.ckpt"]
    best = cli.read_checkpoint(os.path.join(run["checkpoints"], "best.ckpt"))
    assert best["monitor"] == run["best"] and "ema_state_dict" in best
    ck = cli.read_checkpoint(os.path.join(run["checkpoints"], "epoch=1.ckpt"))
    assert set(ck["ema_state_dict"]) < set(ck["state_dict"]) and "monitor" not in ck
    assert any(not torch.equal(v, ck["state_dict"][k]) for k, v in ck["ema_state_dict"].items())
    assert cli.newest_checkpoint(run["folder"]).endswith("epoch=1.ckpt")
    # RNG isolation: without validation the training draws, and so the weights, are the same bits
    r0 = cli.train_main(_common(tmp_path) + ["--epochs", "2", "--val_every", "0", "--ema_decay", "0.9"])
    assert "val_MPJPE" not in r0 and "best" not in r0 and not os.path.exists(os.path.join(r0["checkpoints"], "best.ckpt"))
    ck0 = cli.read_checkpoint(os.path.join(r0["checkpoints"], "epoch=1.ckpt"))
    assert all(torch.equal(ck0["state_dict"][k], v) for k, v in ck["state_dict"].items())
    assert all(torch.equal(ck0["ema_state_dict"][k], v) for k, v in ck["ema_state_dict"].items())


def _test_main(monkeypatch, argv):
    """cli.test_main and the joints every test_step returned: on two epochs of training the test split's rule (root error below
    300 mm) keeps no sequence, so the metrics are all zero and say nothing about the weights."""
    from seeme_amd import cli, mld
    seen, orig = [], mld.MLD.test_step

    def spy(self, batch, batch_idx=0):
        out = orig(self, batch, batch_idx)
        seen.append(out.detach().clone())
        return out

    with monkeypatch.context() as m:
        m.setattr(mld.MLD, "test_step", spy)
        res = cli.test_main(argv)
    assert len(seen) == 1
    return res, seen[0]


def test_test_main_use_ema(dev, run, tmp_path, monkeypatch):
    from seeme_amd import cli
    ckpt = os.path.join(run["checkpoints"], "epoch=1.ckpt")
    common = ["--cfg", CFG, "--batch_size", "4", "--folder", str(tmp_path), "--frames", "24", "--test_batches", "1"]
    raw, j_raw = _test_main(monkeypatch, common + ["--checkpoint", ckpt])
    again, j_again = _test_main(monkeypatch, common + ["--checkpoint", ckpt])
    ema, j_ema = _test_main(monkeypatch, common + ["--checkpoint", ckpt, "--use_ema"])
    assert torch.equal(j_raw, j_again) and not torch.equal(j_raw, j_ema)
    ck = cli.read_checkpoint(ckpt)
    ck["state_dict"].update(ck.pop("ema_state_dict"))
    by_hand = str(tmp_path / "by_hand.ckpt")
    torch.save(ck, by_hand)
    hand, j_hand = _test_main(monkeypatch, common + ["--checkpoint", by_hand])
    assert torch.equal(j_hand, j_ema)
    for k in ema:
        if k.startswith("Metrics/") and "seqs_per_s" not in k:
            assert hand[k] == ema[k], k
    with pytest.raises(ValueError, match="by_hand.ckpt"):
        cli.test_main(common + ["--checkpoint", by_hand, "--use_ema"])


def test_resume_reproduces_the_shadows(dev, run, tmp_path):
    """Epoch 0's checkpoint alone in a folder, resumed for one more epoch: the shadows of the two-epoch run, bit for bit."""
    from seeme_amd import cli
    src = tmp_path / "src" / "checkpoints"
    os.makedirs(src)
    shutil.copy(os.path.join(run["checkpoints"], "epoch=0.ckpt"), src / "epoch=0.ckpt")
    assets = tmp_path / "assets.yaml"
    assets.write_text(f"TRAIN:\n  RESUME: {tmp_path / 'src'}\n")
    r = cli.train_main(_common(tmp_path / "out") + ["--cfg_assets", str(assets), "--epochs", "2", "--val_every", "0", "--ema_decay", "0.9"])
    assert r["epoch"] == 1 and r["step"] == 4
    want = cli.read_checkpoint(os.path.join(run["checkpoints"], "epoch=1.ckpt"))
    got = cli.read_checkpoint(os.path.join(r["checkpoints"], "epoch=1.ckpt"))
    assert all(torch.equal(got["ema_state_dict"][k], v) for k, v in want["ema_state_dict"].items())
    assert all(torch.equal(got["state_dict"][k], v) for k, v in want["state_dict"].items())
