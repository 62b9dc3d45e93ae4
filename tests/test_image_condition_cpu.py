"""The image condition (mld.py:251-255, 887-1017, 1076-1306; dataset.py:1657-1706, 1788-1792) on the CPU: the model builds with
``output_images`` for every layout that carries an image token, its state dict round-trips strictly, the image slot refuses raw
images (the ResNet-50 backbone is outside this path), the per-split feature files load and every access draws one frame of the
sequence, and the synthetic batches have the dataset's layouts."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from seeme_amd import data as D
from test_data_module import write_dataset


def write_image_feats(root, items, dtype=np.float16, drop=(), seed=3):
    """image_feats_<split>.npz for the frames of `items` (write_dataset's result): names [F] as in original_imgname, feats [F,2048]
    non-negative (pooled after a ReLU).  `drop`: names left out.  Returns {split: {name: row}}."""
    rng = np.random.default_rng(seed)
    out = {}
    for split in sorted({sp for sp, _ in items}):
        names = [im for (sp, _n), it in sorted(items.items()) if sp == split for im in it["recording_utils"]["original_imgname"]]
        names = [n for n in dict.fromkeys(names) if n not in drop]
        feats = rng.random((len(names), 2048)).astype(dtype)
        np.savez(os.path.join(root, f"image_feats_{split}.npz"), names=np.array(names), feats=feats)
        out[split] = {"names": names, "feats": feats}
    return out


def _cfg(condition, **kw):
    from seeme_amd.config import parse_config
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_image_scene.yaml"))
    cfg.model.condition = list(condition)
    for k, v in kw.items():
        node = cfg
        *path, last = k.split(".")
        for p in path:
            node = node[p]
        node[last] = v
    return cfg


def _model(condition, **kw):
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    return MLD(_cfg(condition, **kw), SyntheticEgoDataModule(T=8, n_points=16), smpl_model=SMPL.synthetic(1, V=64))


def test_image_config_file():
    cfg = _cfg(["text", "image", "scene"])
    from seeme_amd.config import parse_config
    ref = parse_config(os.path.join(REPO, "configs", "config_mld_image_scene.yaml"))
    assert list(ref.model.condition) == ["text", "image", "scene"] and ref.ESTIMATE == "interactee"
    assert ref.TRAIN.BATCH_SIZE == 64 and ref.model.nfeats == 75 and ref.TRAIN.STAGE == "diffusion"
    assert cfg.model.guidance_scale == 1.0


@pytest.mark.parametrize("condition", [["text", "image", "scene"], ["text", "image"], ["text", "interactee", "scene", "image"]])
def test_mld_builds_with_output_images(condition):
    m = _model(condition)
    sd = m.state_dict()
    assert sd["output_images.1.weight"].shape == (256, 2048) and sd["output_images.1.bias"].shape == (256,)
    assert m.output_images[1].weight.requires_grad and m.output_images[1].bias.requires_grad       # trainable in stage 2
    assert ("proscene.scene_enc.fc_c.weight" in sd) == ("scene" in condition)
    assert not any(p.requires_grad for n, p in m.named_parameters() if n.startswith(("vae.", "proscene.")))
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert "output_images.1.weight" in names and "output_images.1.bias" in names
    # a strict load into a fresh model restores output_images
    m2 = _model(condition)
    assert not torch.equal(m2.output_images[1].weight, m.output_images[1].weight)
    m2.load_state_dict(sd, strict=True)
    assert torch.equal(m2.output_images[1].weight, m.output_images[1].weight)
    assert torch.equal(m2.output_images[1].bias, m.output_images[1].bias)


def test_configs_without_image_build_no_image_projection():
    m = _model(["text", "scene", "interactee"])
    assert not hasattr(m, "output_images") and not any(k.startswith("output_images") for k in m.state_dict())


def test_state_dict_round_trips_through_a_checkpoint(tmp_path):
    from seeme_amd import cli
    m = _model(["text", "image", "scene"])
    cli.save_checkpoint(str(tmp_path / "checkpoints" / "epoch=0.ckpt"), m, 0, 1)
    sd = cli.read_checkpoint(str(tmp_path / "checkpoints" / "epoch=0.ckpt"))["state_dict"]
    m2 = _model(["text", "image", "scene"])
    m2.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k


def test_raw_images_and_bad_features_raise():
    from seeme_amd.mld import SyntheticEgoDataModule
    m = _model(["text", "image", "scene"])
    dm = SyntheticEgoDataModule(T=8, n_points=16)
    b = list(dm.batch(2, with_scene=True, with_image=True))
    b[5] = torch.rand(2, 3, 224, 224)                                       # what the reference's dataset hands over
    with pytest.raises(NotImplementedError, match="backbone"):
        m.train_diffusion_forward(tuple(b))
    with pytest.raises(NotImplementedError, match="backbone"):
        m.ego_eval(tuple(b))
    b[5] = torch.rand(2, 512)
    with pytest.raises(ValueError):
        m.train_diffusion_forward(tuple(b))


def test_image_with_pose_estimation_task_raises():
    with pytest.raises(NotImplementedError, match="POSE_ESTIMATION_TASK"):
        _model(["text", "image", "scene"], **{"TEST.POSE_ESTIMATION_TASK": True})


def test_synthetic_batch_layouts():
    from seeme_amd.mld import SyntheticEgoDataModule, split_batch
    dm = SyntheticEgoDataModule(T=8, n_points=16)
    base = dm.batch(3, idx=4)
    b = dm.batch(3, idx=4, with_scene=True, with_image=True)            # (motion, transl, beta, utils, scene, images, length)
    assert len(b) == 7 and b[4].shape == (3, 16, 3) and b[5].shape == (3, 2048) and b[6].shape == (3, 1)
    assert b[5].dtype == torch.float32 and float(b[5].min()) >= 0.0
    b2 = dm.batch(3, idx=4, with_image=True)                            # (motion, transl, beta, utils, images, length)
    assert len(b2) == 6 and b2[4].shape == (3, 2048) and b2[5].shape == (3, 1)
    for t in (b, b2):
        assert all(torch.equal(x, y) for x, y in zip(t[:4], base[:4]))
    assert torch.equal(b[5], b2[4]) and torch.equal(dm.batch(3, idx=4, with_image=True)[4], b2[4])
    assert not torch.equal(dm.batch(3, idx=5, with_image=True)[4], b2[4])
    scene_only = dm.batch(3, idx=4, with_scene=True)
    assert len(scene_only) == 7 and scene_only[6] == []                 # unchanged: (..., scene, length, names)
    m, tr, be, ut, sc, im, ln, rest = split_batch(("text", "image", "scene"), b)
    assert sc is b[4] and im is b[5] and ln is b[6] and rest == ()
    m, tr, be, ut, sc, im, ln, rest = split_batch(("text", "image"), b2)
    assert sc is None and im is b2[4] and ln is b2[5]
    m, tr, be, ut, sc, im, ln, rest = split_batch(("text", "scene", "interactee"), scene_only)
    assert sc is scene_only[4] and im is None and ln is scene_only[5] and rest == ([],)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_feature_files_load_and_frames_are_drawn_per_access(tmp_path, dtype):
    root = str(tmp_path / "egobody")
    items, _ = write_dataset(root, "egobody", n=6, T=12, P=32, full_every=2)
    feats = write_image_feats(root, items, dtype=dtype)
    dm = D.EgoDataModule(root, "egobody", condition=("text", "image", "scene"), motion_length=12, device="cpu", scene_root=root)
    assert dm.with_image and dm.with_scene
    for split, sp in dm.splits.items():
        names = feats[split]["names"]
        table = feats[split]["feats"].astype(np.float32)
        frames = [[table[names.index(im)] for im in ims] for ims in sp.images]
        ix = torch.arange(len(sp))
        seen = [set() for _ in range(len(sp))]
        for _ in range(40):
            b = dm.collate(split, ix)
            assert len(b) == 7 and b[5].shape == (len(sp), 2048) and b[5].dtype == torch.float32 and b[6].shape == (len(sp), 1)
            got = b[5].numpy()
            for i in range(len(sp)):
                hit = [k for k, f in enumerate(frames[i]) if np.array_equal(f, got[i])]
                assert hit, (split, i)                               # a frame of THIS sequence
                seen[i].add(hit[0])
        assert any(len(s) > 1 for s in seen)                         # a new draw on every access
        # injected draws pick the frame floor(u * n)
        u = torch.tensor([0.0, 0.999999, 0.5, 0.25, 0.75, 0.1])[: len(sp)]
        got = dm.collate(split, ix, image_draws=u)[5].numpy()
        for i in range(len(sp)):
            k = min(int(float(u[i]) * len(frames[i])), len(frames[i]) - 1)
            assert np.array_equal(got[i], frames[i][k])
        one = sp.item(2)
        assert len(one) == 7 and one[5].shape == (2048,) and one[6].shape == (1,)
    # the same seed repeats the same draws; another seed does not
    run = lambda seed: [D.EgoDataModule(root, "egobody", condition=("text", "image"), motion_length=12, device="cpu", seed=seed)
                        .batch(4, idx=k) for k in range(3)]
    r1, r2, r3 = run(7), run(7), run(8)
    assert all(len(b) == 6 and b[4].shape == (4, 2048) for b in r1)
    assert all(torch.equal(a[4], b[4]) for a, b in zip(r1, r2))
    assert not all(torch.equal(a[4], b[4]) for a, b in zip(r1, r3))


def test_missing_feature_names_are_listed(tmp_path):
    root = str(tmp_path / "egobody")
    items, _ = write_dataset(root, "egobody", n=4, T=10, P=16, full_every=2)
    gone = [items[("train", "seq_001.npy")]["recording_utils"]["original_imgname"][k] for k in (0, 1)]
    write_image_feats(root, items, drop=gone)
    with pytest.raises(KeyError, match="2 frame") as e:
        D.EgoDataModule(root, "egobody", condition=("text", "image"), motion_length=10, device="cpu", splits=("train",))
    assert gone[0] in str(e.value)
    os.remove(os.path.join(root, "image_feats_train.npz"))
    with pytest.raises(FileNotFoundError, match="image_feats_train.npz"):
        D.EgoDataModule(root, "egobody", condition=("text", "image"), motion_length=10, device="cpu", splits=("train",))
