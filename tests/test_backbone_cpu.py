"""The ResNet-50 image backbone on the CPU: the state dict has the reference's 318 entries, the recipe round-trips, the torch
restatement reproduces the fixture made from the reference module, the host BatchNorm fold and the uint8 normalisation are what the
kernels assume, MLD grows ``proscene.backbone`` only with ``model.image_backbone``, and the crop files load and draw one frame per
access."""
import os

import numpy as np
import pytest
import torch

import backbone_reference as R
from conftest import REPO, load_golden, rel_err
from seeme_amd import data as D
from test_data_module import write_dataset


@pytest.fixture(scope="module")
def fx():
    return load_golden("resnet50_B2.npz")


def _cfg(condition, backbone=True, **kw):
    from seeme_amd.config import parse_config
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_image_scene_backbone.yaml"))
    cfg.model.condition = list(condition)
    cfg.model.image_backbone = backbone
    for k, v in kw.items():
        node = cfg
        *path, last = k.split(".")
        for p in path:
            node = node[p]
        node[last] = v
    return cfg


def _model(condition, backbone=True, **kw):
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    return MLD(_cfg(condition, backbone, **kw), SyntheticEgoDataModule(T=8, n_points=16), smpl_model=SMPL.synthetic(1, V=64))


def write_image_crops(root, items, drop=(), seed=5):
    """image_crops_<split>.npy + image_crop_names_<split>.npy for the frames of `items` (write_dataset's result)."""
    out = {}
    for split in sorted({sp for sp, _ in items}):
        names = [im for (sp, _n), it in sorted(items.items()) if sp == split for im in it["recording_utils"]["original_imgname"]]
        names = [n for n in dict.fromkeys(names) if n not in drop]
        rng = np.random.default_rng(seed)
        # every crop is constant but for its first bytes, which spell its row: cheap to write, unique per frame
        crops = np.zeros((len(names), 224, 224, 3), np.uint8)
        crops[:, :, :, :] = rng.integers(0, 256, (len(names), 1, 1, 3), dtype=np.uint8)
        crops[:, 0, 0, 0] = np.arange(len(names)) % 256
        crops[:, 0, 0, 1] = np.arange(len(names)) // 256
        np.save(os.path.join(root, f"image_crops_{split}.npy"), crops)
        np.save(os.path.join(root, f"image_crop_names_{split}.npy"), np.array(names))
        out[split] = {"names": names, "crops": crops}
    return out


# ----------------------------------------------------------------------------- the module and its state dict
def test_state_dict_keys_and_shapes_equal_the_reference(fx):
    from seeme_amd.resnet import ResNet50, conv_table, state_shapes
    sd = ResNet50().state_dict()
    assert len(sd) == 318 and len(conv_table()) == 53
    assert sorted(sd) == [str(k) for k in fx["keys"]]
    for k, shp in zip(fx["keys"], fx["shapes"]):
        assert ",".join(str(d) for d in sd[str(k)].shape) == str(shp), k
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in state_shapes().items()}


def test_backbone_is_frozen_and_stays_in_eval_mode():
    from seeme_amd.resnet import ResNet50
    m = ResNet50()
    assert not any(p.requires_grad for p in m.parameters())
    m.train()
    assert not m.training and not any(mod.training for mod in m.modules())
    with pytest.raises(ValueError):
        ResNet50(precision="fp16")


def test_recipe_round_trips_strictly():
    from seeme_amd.resnet import ResNet50
    from seeme_amd.weights_recipe import backbone_recipe_tensor, load_backbone_recipe_, recipe_tensor
    m = load_backbone_recipe_(ResNet50())
    sd = m.state_dict()
    want = R.recipe_state()
    for k, v in want.items():
        assert torch.equal(sd[k], v), k
    m2 = ResNet50()
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), sd.values()))
    assert float(sd["layer3.2.bn2.running_var"].min()) >= 0.5 and float(sd["layer3.2.bn2.running_var"].max()) <= 1.5
    assert abs(float(sd["layer2.1.bn3.weight"].mean()) - 0.35) < 0.02 and abs(float(sd["layer2.1.bn2.weight"].mean()) - 1.0) < 0.05
    assert abs(float(sd["layer2.0.downsample.1.weight"].mean()) - 0.35) < 0.02
    # keyed by name: a prefix in front of `backbone.` changes nothing, and no other key's recipe moved
    a = backbone_recipe_tensor("proscene.backbone.layer1.0.conv1.weight", (64, 64, 1, 1))
    assert np.array_equal(a, backbone_recipe_tensor("layer1.0.conv1.weight", (64, 64, 1, 1)))
    assert not np.array_equal(a, recipe_tensor("layer1.0.conv1.weight", (64, 64, 1, 1)))


def test_restatement_reproduces_the_reference_fixture(fx):
    """tests/backbone_reference.py is the oracle on the GPU machine: pinned here to the reference module's outputs at 1e-6."""
    sd = R.recipe_state()
    crops = torch.from_numpy(fx["crops"])
    assert torch.equal(crops, R.smooth_crops(2, seed=0))
    stages = []
    with torch.no_grad():
        feats = R.forward(sd, R.normalise(crops), stages)
    assert rel_err(feats.numpy(), fx["feats"]) < 1e-6
    for name, s in zip(("pool", "layer1", "layer2", "layer3", "layer4"), stages):
        assert rel_err(s.mean(dim=(2, 3)).numpy(), fx["mean_" + name]) < 1e-6, name
    pix = fx["pixels"]
    assert rel_err(np.stack([stages[1][b, :, i, j].numpy() for b, i, j in pix]), fx["pix_layer1"]) < 1e-6
    assert rel_err(np.stack([stages[3][b, :, i // 4, j // 4].numpy() for b, i, j in pix]), fx["pix_layer3"]) < 1e-6
    # the fixture tells the two images apart by far more than any tolerance of the GPU tests
    assert np.abs(fx["feats"][0] - fx["feats"][1]).max() > 0.02 * np.abs(fx["feats"]).max()


@pytest.mark.parametrize("conv", ["conv1", "layer1.0.conv1", "layer2.0.conv2", "layer1.1.conv2", "layer3.0.downsample.0", "layer4.2.conv3"])
def test_host_bn_fold_equals_conv_plus_bn(conv):
    """One convolution of each kind (stem, 1x1, 3x3 stride 2, 3x3 stride 1, 1x1 stride 2 downsample, last 1x1): folded weight + bias
    against conv followed by the written-out BatchNorm of the restatement."""
    import torch.nn.functional as F
    from seeme_amd.resnet import ResNet50, conv_table
    from seeme_amd.weights_recipe import load_backbone_recipe_
    m = load_backbone_recipe_(ResNet50())
    i = [c[0] for c in conv_table()].index(conv)
    _c, bnname, cin, cout, k, stride = conv_table()[i]
    w64, b64 = m.folded(i)
    assert w64.dtype == torch.float64 and b64.dtype == torch.float64
    sd = {kk: v.double() for kk, v in m.state_dict().items() if v.is_floating_point()}
    x = torch.randn(2, cin, 9, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    want = R.conv_bn(sd, conv, bnname, x, stride=stride)
    got = F.conv2d(x.float(), w64.float(), b64.float(), stride=stride, padding=k // 2)        # the cast the kernels see
    assert rel_err(got.numpy(), want.numpy()) < 1e-6


def test_packed_weights_hold_every_folded_value_once():
    from seeme_amd.resnet import pack_conv
    g = torch.Generator().manual_seed(0)
    for cout, cin, k, dt, E in ((64, 64, 3, torch.float32, 4), (128, 64, 1, torch.bfloat16, 8), (64, 3, 7, torch.float32, 4), (64, 3, 7, torch.bfloat16, 8)):
        w = torch.randint(1, 100, (cout, cin, k, k), generator=g).double()
        p = pack_conv(w, dt)
        cinp = max(cin, E)
        K = -(-(k * k * cinp) // (8 * E)) * 8 * E
        assert tuple(p.shape) == (cout // 16, K // (4 * E), 4, 16, E) and p.dtype == dt
        assert float(p.double().sum()) == float(w.sum()) and int((p != 0).sum()) == w.numel()
        # fragment (tile 1, k-group 0, kq 2, row 5): channel 16 (5 // 4) + 4 (1 % 4) + 5 % 4 = 21, k = 2 E .. 3 E - 1 of tap (0, 0)
        if cin >= 3 * E:
            assert torch.equal(p[1, 0, 2, 5].double(), w[21, 2 * E:3 * E, 0, 0])


def test_uint8_normalisation_is_the_reference_formula(fx):
    from seeme_amd.resnet import IMAGENET_MEAN, IMAGENET_STD, normalise_uint8
    crops = fx["crops"]
    # dataset.py:1693-1705, in numpy as the reference writes it: (x - 255 mean_c) / (255 std_c) per channel of the CHW patch
    patch = np.transpose(crops.astype(np.float32), (0, 3, 1, 2)).copy()
    mean_col, std_col = 255.0 * np.array([0.485, 0.456, 0.406]), 255.0 * np.array([0.229, 0.224, 0.225])
    for c in range(3):
        patch[:, c] = (patch[:, c] - mean_col[c]) / std_col[c]
    got = normalise_uint8(torch.from_numpy(crops)).numpy()
    assert got.shape == (2, 3, 224, 224) and got.dtype == np.float32
    assert np.abs(got - patch).max() < 1e-6 * np.abs(patch).max()
    assert np.abs(R.normalise(crops).numpy() - patch).max() < 1e-6 * np.abs(patch).max()
    assert IMAGENET_MEAN == R.MEAN and IMAGENET_STD == R.STD


def test_cpu_tensors_raise():
    from seeme_amd._lib import SeemeError
    from seeme_amd.resnet import ResNet50
    m = ResNet50()
    with pytest.raises(SeemeError):
        m(torch.zeros(1, 3, 224, 224))
    with pytest.raises(SeemeError):
        m(torch.zeros(1, 224, 224, 3, dtype=torch.uint8))
    with pytest.raises(SeemeError):
        m(torch.zeros(1, 3, 200, 224))


# ----------------------------------------------------------------------------- the C-ABI surface
def test_header_declares_and_library_exports_the_backbone():
    import ctypes as C
    import re
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    declared = set(re.findall(r"\b(seeme_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in ("seeme_resnet50_workspace_bytes", "seeme_resnet50_encode", "seeme_resnet_conv", "seeme_resnet_stem_pack", "seeme_resnet_maxpool"):
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name)
    assert int(re.search(r"#define SEEME_RESNET50_NCONV (\d+)", hdr).group(1)) == _lib.RESNET50_NCONV == 53
    f32, b16 = lib.seeme_resnet50_workspace_bytes(2, 0), lib.seeme_resnet50_workspace_bytes(2, 1)
    assert f32 > b16 >= 2 * (224 * 224 * 16 + 3 * 112 * 112 * 64 * 2) and f32 % 256 == 0
    assert lib.seeme_resnet50_workspace_bytes(0, 0) == 0 and lib.seeme_resnet50_workspace_bytes(2, 7) == 0
    # argument checks come before any device work: they hold without a GPU
    w = _lib.Resnet50()
    assert lib.seeme_resnet50_encode(C.byref(w), 0, 0, 2, 0, 0, 0, 0) != 0 and b"null" in lib.seeme_last_error()
    assert lib.seeme_resnet50_encode(C.byref(w), 256, 0, 2, 256, 256, 1 << 40, 0) != 0 and b"conv table" in lib.seeme_last_error()
    assert lib.seeme_resnet50_encode(C.byref(w), 256, 0, 2, 256, 256, 16, 0) != 0 and b"workspace" in lib.seeme_last_error()
    assert lib.seeme_resnet50_encode(C.byref(w), 256, 3, 2, 256, 256, 1 << 40, 0) != 0 and b"image_format" in lib.seeme_last_error()
    assert lib.seeme_resnet50_encode(C.byref(w), 258, 0, 2, 256, 256, 1 << 40, 0) != 0 and b"unaligned" in lib.seeme_last_error()
    assert lib.seeme_resnet50_encode(C.byref(w), 256, 0, 0, 256, 256, 1 << 40, 0) != 0 and b"B must" in lib.seeme_last_error()
    c = _lib.Conv()
    c.cin, c.cout, c.k, c.stride = 64, 96, 3, 1
    assert lib.seeme_resnet_conv(C.byref(c), 0, 256, 1, 5, 5, 0, 1, 256, 0) != 0 and b"cout" in lib.seeme_last_error()
    c.cout, c.k = 64, 5
    assert lib.seeme_resnet_conv(C.byref(c), 0, 256, 1, 5, 5, 0, 1, 256, 0) != 0 and b"kernel size" in lib.seeme_last_error()


# ----------------------------------------------------------------------------- MLD
def test_model_with_the_key_holds_and_loads_the_backbone():
    m = _model(["text", "image", "scene"])
    sd = m.state_dict()
    bb = [k for k in sd if k.startswith("proscene.backbone.")]
    assert len(bb) == 318 and "proscene.backbone.layer4.2.bn3.running_var" in sd and "proscene.scene_enc.fc_c.weight" in sd
    assert not any(p.requires_grad for n, p in m.named_parameters() if n.startswith("proscene."))
    # a state dict that carries them (a reference checkpoint's proscene.backbone.* entries) loads strictly
    other = {k: (torch.randn_like(v) if v.is_floating_point() else v) for k, v in sd.items()}
    m2 = _model(["text", "image", "scene"])
    m2.load_state_dict(other, strict=True)
    assert torch.equal(m2.state_dict()["proscene.backbone.layer1.0.conv1.weight"], other["proscene.backbone.layer1.0.conv1.weight"])
    # ... and stays out of the optimiser
    m.configure_optimizers()
    held = {id(p) for g in m.optimizer.param_groups for p in g["params"]}
    assert held and not any(id(p) in held for p in m.proscene.parameters())
    assert all(id(p) in held for p in m.output_images.parameters())
    assert not any(n.startswith("proscene.") for n, p in m.named_parameters() if p.requires_grad)
    m.train()
    assert not m.proscene.backbone.training and not m.proscene.backbone.bn1.training


def test_image_only_model_has_the_holder_and_precision_follows_the_config():
    m = _model(["text", "image"], **{"TRAIN.IMAGE_PRECISION": "bf16"})
    sd = m.state_dict()
    assert sum(k.startswith("proscene.backbone.") for k in sd) == 318 and not any(k.startswith("proscene.scene_enc") for k in sd)
    assert m.proscene.backbone.precision == "bf16"
    assert _model(["text", "image", "scene"]).proscene.backbone.precision == "fp32"


def test_models_without_the_key_keep_their_key_sets():
    with_key = set(_model(["text", "scene", "interactee"], backbone=True).state_dict())      # no image: the key changes nothing
    without = set(_model(["text", "scene", "interactee"], backbone=False).state_dict())
    assert with_key == without and not any("backbone" in k for k in without)
    img = set(_model(["text", "image", "scene"], backbone=False).state_dict())
    assert not any("backbone" in k for k in img) and "output_images.1.weight" in img
    assert not hasattr(_model(["text", "image"], backbone=False), "proscene")


def test_raw_images_raise_without_the_key():
    from seeme_amd.mld import SyntheticEgoDataModule
    m = _model(["text", "image", "scene"], backbone=False)
    dm = SyntheticEgoDataModule(T=8, n_points=16)
    b = list(dm.batch(2, with_scene=True, with_image=True))
    b[5] = torch.rand(2, 3, 224, 224)
    with pytest.raises(NotImplementedError, match="backbone"):
        m.train_diffusion_forward(tuple(b))
    b[5] = torch.zeros(2, 224, 224, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="backbone"):
        m.ego_eval(tuple(b))


def test_new_config_file_parses_with_the_key_on():
    from seeme_amd.config import parse_config
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_image_scene_backbone.yaml"))
    assert cfg.model.image_backbone is True and list(cfg.model.condition) == ["text", "image", "scene"]
    assert cfg.TRAIN.IMAGE_PRECISION == "fp32" and cfg.TRAIN.BATCH_SIZE == 64
    old = parse_config(os.path.join(REPO, "configs", "config_mld_image_scene.yaml"))
    assert not old.model.get("image_backbone", False)


def test_synthetic_crops():
    from seeme_amd.mld import SyntheticEgoDataModule
    dm = SyntheticEgoDataModule(T=8, n_points=16)
    b = dm.batch(3, idx=4, with_scene=True, with_image="crops")
    feats = dm.batch(3, idx=4, with_scene=True, with_image=True)
    assert len(b) == 7 and b[5].shape == (3, 224, 224, 3) and b[5].dtype == torch.uint8 and b[6].shape == (3, 1)
    assert all(torch.equal(x, y) for x, y in zip(b[:5], feats[:5])) and feats[5].shape == (3, 2048)      # with_image=True unchanged
    assert torch.equal(dm.batch(3, idx=4, with_image="crops")[4], b[5]) and not torch.equal(dm.batch(3, idx=5, with_image="crops")[4], b[5])
    c = b[5].float()
    assert float(c.max()) > 200 and float(c.min()) < 55 and not torch.equal(b[5][0], b[5][1])
    assert float((c[:, 1:] - c[:, :-1]).abs().max()) <= 10                                                # smooth
    with pytest.raises(ValueError):
        dm.batch(3, with_image="jpeg")


# ----------------------------------------------------------------------------- the crop files
def test_crop_files_load_and_frames_are_drawn_per_access(tmp_path):
    root = str(tmp_path / "egobody")
    items, _ = write_dataset(root, "egobody", n=6, T=12, P=32, full_every=2)
    files = write_image_crops(root, items)
    dm = D.EgoDataModule(root, "egobody", condition=("text", "image", "scene"), motion_length=12, device="cpu", scene_root=root,
                         image_backbone=True)
    assert dm.with_image and dm.with_scene
    for split, sp in dm.splits.items():
        names, table = files[split]["names"], files[split]["crops"]
        frames = [[table[names.index(im)] for im in ims] for ims in sp.images]
        ix = torch.arange(len(sp))
        seen = [set() for _ in range(len(sp))]
        for _ in range(25):
            b = dm.collate(split, ix)
            assert len(b) == 7 and b[5].shape == (len(sp), 224, 224, 3) and b[5].dtype == torch.uint8 and b[6].shape == (len(sp), 1)
            got = b[5].numpy()
            for i in range(len(sp)):
                hit = [k for k, f in enumerate(frames[i]) if np.array_equal(f, got[i])]
                assert hit, (split, i)                               # a frame of THIS sequence
                seen[i].add(hit[0])
        assert any(len(s) > 1 for s in seen)                         # a new draw on every access
        u = torch.tensor([0.0, 0.999999, 0.5, 0.25, 0.75, 0.1])[: len(sp)]
        got = dm.collate(split, ix, image_draws=u)[5].numpy()
        for i in range(len(sp)):
            k = min(int(float(u[i]) * len(frames[i])), len(frames[i]) - 1)
            assert np.array_equal(got[i], frames[i][k])
        one = sp.item(2)
        assert len(one) == 7 and one[5].shape == (224, 224, 3) and one[5].dtype == torch.uint8
    # without the key the same directory still asks for the feature file
    with pytest.raises(FileNotFoundError, match="image_feats_"):
        D.EgoDataModule(root, "egobody", condition=("text", "image"), motion_length=12, device="cpu")


def test_missing_crop_names_and_bad_files_are_reported(tmp_path):
    root = str(tmp_path / "egobody")
    items, _ = write_dataset(root, "egobody", n=4, T=10, P=16, full_every=2)
    gone = [items[("train", "seq_001.npy")]["recording_utils"]["original_imgname"][k] for k in (0, 1)]
    write_image_crops(root, items, drop=gone)
    mk = lambda: D.EgoDataModule(root, "egobody", condition=("text", "image"), motion_length=10, device="cpu", splits=("train",),
                                 image_backbone=True)
    with pytest.raises(KeyError, match="2 frame") as e:
        mk()
    assert gone[0] in str(e.value)
    files = write_image_crops(root, items)
    mk()
    np.save(os.path.join(root, "image_crops_train.npy"), files["train"]["crops"].astype(np.float32)[:, :8, :8])
    with pytest.raises(ValueError, match="uint8"):
        mk()
    np.save(os.path.join(root, "image_crop_names_train.npy"), np.array(files["train"]["names"], dtype=object), allow_pickle=True)
    with pytest.raises(ValueError):                                   # an object array needs pickle: refused
        mk()
    os.remove(os.path.join(root, "image_crop_names_train.npy"))
    with pytest.raises(FileNotFoundError, match="image_crop_names_train.npy"):
        mk()
