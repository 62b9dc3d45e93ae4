"""The HIP ResNet-50 backbone (csrc/resnet.hip) on the device: the fp32 path against the fixture made from the reference module, one
convolution of each class against the torch restatement (tests/backbone_reference.py, float64 on the CPU), the bf16 path against
the fp32 fixture, both input forms, determinism, and MLD with crops in the image slot against the same model given the backbone's
output as features."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backbone_reference as R
from conftest import REPO, load_golden, rel_err
from seeme_amd.weights_recipe import load_backbone_recipe_, load_recipe_

pytestmark = pytest.mark.gpu
TOL_F32 = 1e-4          # the project's parity gate, relative to the largest entry
# bf16 path against the fp32 fixture, relative max-norm error; measured on the MI355X and gated at 3x the measurement
BF16_FEATS_MEASURED, BF16_TOKEN_MEASURED = 2.945e-3, 2.958e-3
CFG = "config_mld_image_scene_backbone.yaml"
LAYOUTS = {"scene_image": ["text", "image", "scene"], "image": ["text", "image"]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_golden("resnet50_B2.npz")


@pytest.fixture(scope="module")
def nets(dev):
    from seeme_amd.resnet import ResNet50
    return {p: load_backbone_recipe_(ResNet50(precision=p)).to(dev) for p in ("fp32", "bf16")}


@pytest.fixture(scope="module")
def fp32_run(dev, fx, nets):
    """The fp32 path on the fixture's crops, once: features and the five stage activations (NHWC)."""
    taps = []
    feats = nets["fp32"].encode(torch.from_numpy(fx["crops"]).to(dev), taps=taps)
    torch.cuda.synchronize()
    return feats, taps


def _np(t):
    return t.detach().float().cpu().numpy()


# ----------------------------------------------------------------------------- 1: fp32 path against the fixture
def test_fp32_features_match_the_fixture(fx, fp32_run):
    feats, _ = fp32_run
    got = _np(feats)
    assert got.shape == (2, 2048)
    errs = [rel_err(got, fx["feats"])] + [rel_err(got[i], fx["feats"][i]) for i in range(2)]
    print("fp32 feats rel err (all, image 0, image 1):", errs)
    assert max(errs) < TOL_F32, errs
    # (a per-image mix-up would show: the fixture's two rows differ by percent of the maximum)
    assert rel_err(got[::-1], fx["feats"]) > 100 * TOL_F32


def test_fp32_stage_means_and_pixels_match_the_fixture(fx, fp32_run):
    _, taps = fp32_run
    for name, t in zip(("pool", "layer1", "layer2", "layer3", "layer4"), taps):
        e = rel_err(_np(t.mean(dim=(1, 2))), fx["mean_" + name])
        print("stage mean", name, e)
        assert e < TOL_F32, (name, e)
    pix = fx["pixels"]
    e1 = rel_err(np.stack([_np(taps[1][b, i, j]) for b, i, j in pix]), fx["pix_layer1"])
    e3 = rel_err(np.stack([_np(taps[3][b, i // 4, j // 4]) for b, i, j in pix]), fx["pix_layer3"])
    print("pixels layer1, layer3:", e1, e3)
    assert e1 < TOL_F32 and e3 < TOL_F32


# ----------------------------------------------------------------------------- 2: one convolution of each class
def _conv_case(dev, seed, B, H, W, cin, cout, k, stride, residual, relu, precision="fp32", integer=False):
    from seeme_amd.resnet import conv2d_nhwc
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    if integer:       # asymmetric exact-integer data: every product and sum is exact in fp32 (and the inputs in bf16)
        x = torch.randint(-2, 3, (B, cin, H, W), generator=g).double() + (torch.arange(W) % 3 == 0).double()
        w = torch.randint(-2, 3, (cout, cin, k, k), generator=g).double()
        w[:, :, 0, -1] += 1.0
        b = torch.randint(-3, 4, (cout,), generator=g).double()
        res = torch.randint(-4, 5, (B, cout, Ho, Wo), generator=g).double() if residual else None
    else:
        x = torch.randn(B, cin, H, W, generator=g).double()
        w = torch.randn(cout, cin, k, k, generator=g).double() / (cin * k * k) ** 0.5
        b = torch.randn(cout, generator=g).double()
        res = torch.randn(B, cout, Ho, Wo, generator=g).double() if residual else None
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    # the kernel's operands ARE fp32 / bf16: the reference takes the rounded values, so the bound below is about the arithmetic alone
    x, w = x.to(dt).double(), w.to(dt).double()
    res = res.to(dt).double() if res is not None else None
    b = b.float().double()
    want = F.conv2d(x, w, b, stride=stride, padding=k // 2)
    mag = F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=k // 2)        # sum |a b| of every output
    if res is not None:
        want, mag = want + res, mag + res.abs()
    if relu:
        want = want.relu()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev, dt)
    got = conv2d_nhwc(nhwc(x), w, b, stride=stride, residual=nhwc(res) if res is not None else None, relu=relu, precision=precision)
    torch.cuda.synchronize()
    return got.double().cpu().permute(0, 3, 1, 2), want, mag


# fp32 MFMA = a k-ordered chain of fmaf (one rounding per product): |error| <= (K + 2) u sum|a b| in the worst case, ~sqrt(K) u
# typically; 8 u sum|a b| (u = 2^-24) per ELEMENT holds the chain to a few roundings and is far below any indexing mistake
_U = 2.0 ** -24
CASES = {  # name: (cin, cout, k, stride, residual, relu, H, W)
    "1x1_s1": (64, 128, 1, 1, False, True, 7, 5),
    "1x1_s2": (128, 256, 1, 2, False, False, 9, 7),
    "3x3_s1": (64, 64, 3, 1, False, True, 7, 9),
    "3x3_s2": (128, 128, 3, 2, False, True, 9, 7),
    "1x1_residual": (64, 256, 1, 1, True, True, 5, 7),
}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_convolution_classes_fp32_vs_restatement(dev, name, B):
    cin, cout, k, stride, residual, relu, H, W = CASES[name]
    got, want, mag = _conv_case(dev, 11, B, H, W, cin, cout, k, stride, residual, relu)
    assert got.shape == want.shape
    worst = float(((got - want).abs() / mag).max())
    print(name, B, "worst |err| / sum|ab| =", worst, "in u:", worst / _U)
    assert worst < 8 * _U


@pytest.mark.parametrize("name,B,H,W,cin,cout,k", [("1x1_tile128", 3, 105, 105, 16, 256, 1), ("3x3_tile128", 3, 149, 149, 16, 128, 3)])
def test_convolution_wide_tile_variant_and_many_blocks(dev, name, B, H, W, cin, cout, k):
    """Enough output pixels that the launcher takes the 128-channel tile (the small cases above all run the 64-channel one); the row
    count is no multiple of 128, so the last block is partial."""
    assert ((B * H * W + 127) // 128) * (cout // 128) >= 512 and (B * H * W) % 128
    got, want, mag = _conv_case(dev, 13, B, H, W, cin, cout, k, 1, False, True)
    worst = float(((got - want).abs() / mag).max())
    print(name, "worst |err| / sum|ab| in u:", worst / _U)
    assert worst < 8 * _U


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_convolution_layout_with_exact_integers(dev, precision):
    """Asymmetric integer data: any swap of rows / columns / taps / channels in the packing or the fragment maps changes the result,
    and the right result is exact -- in fp32 bit for bit, in bf16 after the one rounding of the store."""
    for name in ("3x3_s2", "1x1_residual", "3x3_s1"):
        cin, cout, k, stride, residual, relu, H, W = CASES[name]
        got, want, _ = _conv_case(dev, 17, 3, H, W, cin, cout, k, stride, residual, relu, precision=precision, integer=True)
        if precision == "bf16":
            want = want.to(torch.bfloat16).double()
        assert torch.equal(got, want), (name, float((got - want).abs().max()))


@pytest.mark.parametrize("B,H,W", [(1, 21, 17), (3, 15, 19)])
def test_stem_and_maxpool_vs_restatement(dev, B, H, W):
    """conv1 (7x7 stride 2, K = 147 padded in the packed image) from both input forms, then the 3x3 stride-2 max-pool, odd sizes."""
    from seeme_amd.resnet import conv2d_nhwc, maxpool_nhwc, stem_pack
    g = torch.Generator().manual_seed(23)
    crops = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    x = R.normalise(crops)                                                       # float32 NCHW, the reference formula
    w = torch.randn(64, 3, 7, 7, generator=g).double() / 147 ** 0.5
    b = torch.randn(64, generator=g).double()
    want = F.conv2d(x.double(), w, b, stride=2, padding=3).relu()
    mag = F.conv2d(x.double().abs(), w.abs(), b.abs(), stride=2, padding=3)
    outs = []
    for images in (x.to(dev), crops.to(dev)):
        y = conv2d_nhwc(stem_pack(images), w, b, stride=2, relu=True)
        outs.append(y)
        got = y.double().cpu().permute(0, 3, 1, 2)
        worst = float(((got - want).abs() / mag).max())
        print("stem", B, images.dtype, "worst in u:", worst / _U)
        assert worst < 8 * _U                   # (the loader's normalisation is the same two fp32 operations as the formula)
    p = maxpool_nhwc(outs[0])
    assert torch.equal(p.cpu().permute(0, 3, 1, 2), F.max_pool2d(outs[0].cpu().permute(0, 3, 1, 2), 3, 2, 1))     # a max is exact
    pb = maxpool_nhwc(outs[0].to(torch.bfloat16), precision="bf16")
    assert torch.equal(pb.float().cpu().permute(0, 3, 1, 2), F.max_pool2d(outs[0].to(torch.bfloat16).float().cpu().permute(0, 3, 1, 2), 3, 2, 1))


def test_bad_arguments_are_refused_before_any_launch(dev, nets):
    from seeme_amd._lib import SeemeError
    from seeme_amd.resnet import conv2d_nhwc
    net = nets["fp32"]
    with pytest.raises(SeemeError):
        net(torch.zeros(2, 3, 224, 200, device=dev))
    with pytest.raises(SeemeError):
        net(torch.zeros(2, 224, 224, 3, device=dev))                 # float NHWC is neither form
    with pytest.raises(SeemeError, match="cout"):
        conv2d_nhwc(torch.zeros(1, 5, 5, 64, device=dev), torch.zeros(96, 64, 1, 1), torch.zeros(96))
    with pytest.raises(SeemeError, match="cin"):
        conv2d_nhwc(torch.zeros(1, 5, 5, 24, device=dev), torch.zeros(64, 24, 1, 1), torch.zeros(64))


# ----------------------------------------------------------------------------- 3: bf16 path against the fp32 fixture
def test_bf16_path_against_the_fp32_fixture(dev, fx, nets):
    """The throughput path's error is a measurement, gated at 3x (the rule for throughput-mode bounds): features, and the token
    after output_images (ReLU + Linear(2048, 256), recipe weights, float64) -- both against the fp32 FIXTURE."""
    from seeme_amd.weights_recipe import recipe_tensor
    got = _np(nets["bf16"](torch.from_numpy(fx["crops"]).to(dev)))
    W = recipe_tensor("output_images.1.weight", (256, 2048)).astype(np.float64)
    b = recipe_tensor("output_images.1.bias", (256,)).astype(np.float64)
    tok = lambda f: np.maximum(f.astype(np.float64), 0.0) @ W.T + b
    e_f, e_t = rel_err(got, fx["feats"]), rel_err(tok(got), tok(fx["feats"]))
    print(f"bf16 vs fp32 fixture: feats {e_f:.3e}, token {e_t:.3e}")
    assert e_f < 3 * BF16_FEATS_MEASURED and e_t < 3 * BF16_TOKEN_MEASURED, (e_f, e_t)
    assert rel_err(got[::-1], fx["feats"]) > 3 * BF16_FEATS_MEASURED          # the bound still tells the two images apart


# ----------------------------------------------------------------------------- 4: input forms, determinism
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_uint8_input_equals_float_input(dev, fx, nets, precision):
    crops = torch.from_numpy(fx["crops"]).to(dev)
    a = nets[precision](crops)
    b = nets[precision](R.normalise(crops))                         # the same crops, normalised with the reference formula
    e = rel_err(_np(a), _np(b))
    print(precision, "uint8 vs float NCHW:", e)
    # fp32 rounding of the normalisation (a division against torch's: <= 1 ulp of the input) through 53 layers; bf16 mostly
    # rounds the difference away, a flipped bf16 rounding of an input costs up to the path's own error
    assert e < (1e-5 if precision == "fp32" else 3 * BF16_FEATS_MEASURED)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_launches_are_bitwise_equal_and_rows_do_not_depend_on_the_batch(dev, fx, nets, precision):
    net = nets[precision]
    two = torch.from_numpy(fx["crops"]).to(dev)
    a, b = net(two), net(two)
    assert torch.equal(a, b)
    big = torch.cat([two, R.smooth_crops(62, seed=9).to(dev)])
    assert big.shape[0] == 64
    c, d = net(big), net(big)
    torch.cuda.synchronize()
    assert torch.equal(c, d) and bool(torch.isfinite(c).all())
    assert torch.equal(c[:2], a)                                    # other tile shapes at B = 64, the same sums in the same order
    assert float(c[2:].abs().max()) > 0 and not torch.equal(c[2], c[3])


def test_repack_when_the_tensors_change(dev, fx, nets):
    from seeme_amd.resnet import ResNet50
    net = load_backbone_recipe_(ResNet50()).to(dev)
    x = torch.from_numpy(fx["crops"]).to(dev)
    a = net(x)
    assert not net.stale()
    with torch.no_grad():
        net.layer4[2].bn3.running_var.mul_(4.0)                     # a buffer: part of the folded weights
    assert net.stale()
    b = net(x)
    assert not torch.equal(a, b)
    load_backbone_recipe_(net)
    assert net.stale() and torch.equal(net(x), a)
    net.precision = "bf16"
    assert net.stale() and rel_err(_np(net(x)), _np(a)) < 3 * BF16_FEATS_MEASURED


# ----------------------------------------------------------------------------- 5: MLD with crops against MLD with features
def _mld(dev, layout, T=16, n_points=384, **kw):
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(os.path.join(REPO, "configs", CFG))
    cfg.model.condition = list(LAYOUTS[layout])
    for k, v in kw.items():
        node = cfg
        *path, last = k.split(".")
        for p in path:
            node = node[p]
        node[last] = v
    dm = SyntheticEgoDataModule(nfeats=cfg.model.nfeats, T=T, n_points=n_points, device=dev, pose_dim=cfg.model.nfeats - 3)
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser), load_recipe_(model.proscene)      # backbone.* entries: the backbone recipe
    return model.to(dev), dm, cfg


def _forms(batch, slot, model, form):
    """(batch with crops in `form`, the same batch with the backbone's output as 2-D features)."""
    crops = batch[slot]
    assert crops.dtype == torch.uint8 and tuple(crops.shape[1:]) == (224, 224, 3)
    images = crops if form == "u8" else R.normalise(crops)
    feats = model.proscene.backbone(images)
    a, b = list(batch), list(batch)
    a[slot], b[slot] = images, feats
    return tuple(a), tuple(b)


@pytest.mark.parametrize("layout,form", [("scene_image", "u8"), ("image", "f32")])
def test_mld_with_crops_equals_mld_with_backbone_features(dev, layout, form):
    """train_diffusion_forward (the stage-2 glue), ego_eval and the K = 4 hypotheses pass with crops in the image slot against the
    same model given ResNet50(crops) as features: loss, gradients and joints bit for bit; the backbone runs once per sequence."""
    model, dm, cfg = _mld(dev, layout)
    assert model.image_backbone and sum(k.startswith("proscene.backbone.") for k in model.state_dict()) == 318
    slot = 5 if layout == "scene_image" else 4
    B = 3
    raw = dm.batch(B, idx=3, with_scene=layout == "scene_image", with_image="crops")
    with_crops, with_feats = _forms(raw, slot, model, form)
    g = torch.Generator().manual_seed(5)
    noise, ts = torch.randn(B, 1, 256, generator=g).to(dev), torch.randint(0, 1000, (B,), generator=g).to(dev)
    eps = (torch.randn(1, B, 256, generator=g).to(dev), torch.randn(1, B, 256, generator=g).to(dev))
    model.eval()
    calls = []
    enc = model.proscene.backbone.encode
    model.proscene.backbone.encode = lambda images, taps=None: (calls.append(images.shape[0]), enc(images, taps))[1]
    out = []
    for tb in (with_crops, with_feats):
        for p in model.parameters():
            p.grad = None
        rs = model.train_diffusion_forward(tb, noise=noise, timesteps=ts, eps=eps)
        loss = model.losses["train"].update(rs)
        loss.backward()
        out.append((loss.detach().clone(), {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}))
    assert calls == [B]                                              # once per sequence, and not at all for features
    (l1, g1), (l0, g0) = out
    assert torch.equal(l1, l0) and set(g1) == set(g0) and "output_images.1.weight" in g0
    assert all(torch.equal(g1[k], g0[k]) for k in g0)
    assert not any(k.startswith("proscene.") for k in g0)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    lat = rn(B, 1, 256)
    r1, r0 = model.ego_eval(with_crops, latents=lat), model.ego_eval(with_feats, latents=lat)
    assert torch.equal(r1["joints_rst"], r0["joints_rst"]) and torch.equal(r1["lat_t"], r0["lat_t"])
    assert calls == [B, B]
    K = 4
    latk = rn(B * K, 1, 256)
    k1 = model.ego_eval(with_crops, latents=latk, num_hypotheses=K)
    k0 = model.ego_eval(with_feats, latents=latk, num_hypotheses=K)
    assert k1["joints_rst_all"].shape[:2] == (B, K) and torch.equal(k1["joints_rst_all"], k0["joints_rst_all"])
    assert torch.equal(k1["lat_t_all"], k0["lat_t_all"]) and not torch.equal(k1["joints_rst_all"][:, 0], k1["joints_rst_all"][:, 1])
    assert calls == [B, B, B]                                        # K hypotheses: still one backbone pass over B crops
    # another crop changes the result (the slot is really read)
    other = list(with_crops)
    other[slot] = torch.flip(with_crops[slot], dims=[0])
    assert not torch.equal(model.ego_eval(tuple(other), latents=lat)["joints_rst"], r1["joints_rst"])


def test_captured_training_step_with_crops_replays(dev):
    """capture_training_step with the crops in the static batch and the backbone's launches inside the capture, against a second
    model of the same seed captured on the backbone's output as features: the losses of two replays and of a third on a new batch,
    and the trained projection afterwards, bit for bit.  The backbone stays out of the optimiser and its tensors do not move."""
    runs = []
    for use_crops in (True, False):
        model, dm, cfg = _mld(dev, "scene_image")
        model.eval()                                                 # no dropout draws: the two models see the same numbers
        batches = []
        for idx in (3, 10):
            raw = dm.batch(4, idx=idx, with_scene=True, with_image="crops")
            batches.append(_forms(raw, 5, model, "u8")[0 if use_crops else 1])
        model.configure_optimizers()
        held = {id(p) for gp in model.optimizer.param_groups for p in gp["params"]}
        assert not any(id(p) in held for p in model.proscene.parameters())
        sd0 = {k: v.clone() for k, v in model.proscene.backbone.state_dict().items()}
        torch.manual_seed(11)
        model.optimizer_step(model.training_step(batches[0]))
        replay = model.capture_training_step(batches[0], warmup=1)
        torch.cuda.synchronize()
        assert not any(any(p is q for q in model.grad_bucket().params) for p in model.proscene.parameters())
        losses = [float(replay().detach()), float(replay().detach()), float(replay(batches[1]).detach())]
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in losses) and losses[2] != losses[1]
        assert all(torch.equal(v, sd0[k]) for k, v in model.proscene.backbone.state_dict().items())      # frozen: running stats too
        runs.append((losses, model.output_images[1].weight.detach().clone()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


# ----------------------------------------------------------------------------- 6: the CLI and the file data module
def test_cli_trains_and_tests_from_crops(dev, tmp_path):
    """train_main / test_main on synthetic crops with the backbone YAML: finite loss, output_images trained, the backbone's entries
    in the checkpoint unchanged, and the checkpoint reloads strictly."""
    from seeme_amd import cli
    cfgp = os.path.join(REPO, "configs", CFG)
    common = ["--cfg", cfgp, "--batch_size", "4", "--nodebug", "--folder", str(tmp_path), "--frames", "24", "--scene_points", "512"]
    r = cli.train_main(common + ["--epochs", "2", "--iters_per_epoch", "2"])
    assert r["step"] == 4 and np.isfinite(r["total"])
    sd0 = cli.read_checkpoint(os.path.join(r["checkpoints"], "epoch=0.ckpt"))["state_dict"]
    sd1 = cli.read_checkpoint(os.path.join(r["checkpoints"], "epoch=1.ckpt"))["state_dict"]
    assert sum(k.startswith("proscene.backbone.") for k in sd1) == 318
    assert not torch.equal(sd0["output_images.1.weight"], sd1["output_images.1.weight"])
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd1 if k.startswith("proscene.backbone."))
    out = cli.test_main(["--cfg", cfgp, "--batch_size", "4", "--folder", str(tmp_path), "--frames", "24", "--scene_points", "512",
                         "--test_batches", "2", "--checkpoint", os.path.join(r["checkpoints"], "epoch=1.ckpt")])
    assert np.isfinite(out["Metrics/MPJPE/mean"])


def test_data_module_crops_feed_training_and_eval(dev, tmp_path):
    """EgoDataModule with image_crops_<split>.npy: the uint8 table lives on the device, frames are drawn there per access, and the
    batches drive a training step and an evaluation step through the backbone."""
    from seeme_amd import data as D
    from test_backbone_cpu import write_image_crops
    from test_data_module import write_dataset
    root = str(tmp_path / "egobody")
    items, _ = write_dataset(root, "egobody", n=4, T=12, P=32, full_every=2)
    write_image_crops(root, items)
    dm = D.EgoDataModule(root, "egobody", condition=("text", "image", "scene"), motion_length=12, device=dev, scene_root=root,
                         image_backbone=True)
    sp = dm.splits["train"]
    assert sp.image_table.is_cuda and sp.image_table.dtype == torch.uint8
    b = dm.batch(3, idx=0)
    assert b[5].is_cuda and b[5].dtype == torch.uint8 and b[5].shape == (3, 224, 224, 3)
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD
    from seeme_amd.smpl import SMPL
    cfg = parse_config(os.path.join(REPO, "configs", CFG))
    cfg.model.scheduler.num_inference_timesteps = 5
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser), load_recipe_(model.proscene)
    model = model.to(dev).train()
    loss = model.training_step(b)
    model.optimizer_step(loss)
    assert np.isfinite(float(loss.detach()))
    model.eval()
    for tb in dm.iterate("test", 4):
        assert tb[5].dtype == torch.uint8 and model.test_step(tb).shape[1:] == (12, 24, 3)
