"""seeme_crop_patches on the device: the kernel against its plain-torch twin with torch.equal (the patch is an integer definition: no
tolerance anywhere) over the case list of tests/crop_reference.py, past 32-bit byte offsets, with bad arguments; then a recording
with video frames end to end (windows_batch, MLD.predict_recording, cli.predict_main) and the crop files for training."""
import os
import zlib

import numpy as np
import pytest
import torch

import crop_reference as REF
from conftest import REPO
from seeme_amd import crops as CR
from test_gpu_backbone import CFG, _mld
from test_gpu_hyp_select import _draws

pytestmark = pytest.mark.gpu
CASES = REF.cases() + REF.many_patch_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- 1. kernel against twin
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_twin(dev, case):
    name, frames, fop, boxes, S = case
    want = CR.crop_patches_torch(torch.from_numpy(frames), fop, boxes, S)
    fr = torch.from_numpy(frames).to(dev)
    got = CR.crop_patches_hip(fr, fop, boxes, S)
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got.cpu(), want)
    assert torch.equal(CR.crop_patches_hip(fr, fop, boxes, S), got)                  # a second launch, bit for bit
    # the bytes around `out` are untouched; head 4: the dword stores, head 1: an unaligned `out`, every group by bytes
    n = len(fop)
    for head in (4, 1):
        buf = torch.full((head + n * S * S * 3 + 64,), 0xA5, dtype=torch.uint8, device=dev)
        out = buf[head:head + n * S * S * 3].view(n, S, S, 3)
        CR._launch(fr, torch.from_numpy(fop.astype(np.int32)).to(dev), torch.from_numpy(boxes).to(dev), S, out)
        assert torch.equal(out.cpu(), want), head
        assert bool((buf[:head] == 0xA5).all()) and bool((buf[head + n * S * S * 3:] == 0xA5).all()), head


# ----------------------------------------------------------------------------- 2. past 32-bit byte offsets
def test_frames_past_two_and_four_gibibytes(dev):
    """1367 frames of 1024 x 1024 x 3 bytes are 4.3 GB: frame 683 starts past 2^31 bytes, frame 1366 past 2^32.  Only the three
    frames that are read are filled."""
    nf, H, W = 1367, 1024, 1024
    used = [0, 683, 1366]
    assert 683 * H * W * 3 > 2 ** 31 and 1366 * H * W * 3 > 2 ** 32
    g = torch.Generator().manual_seed(3)
    three = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8)
    frames = torch.empty((nf, H, W, 3), dtype=torch.uint8, device=dev)
    for i, f in enumerate(used):
        frames[f] = three[i].to(dev)
    boxes = np.array([[500.0, 400.0, 300.0], [20.5, 1000.25, 150.0], [900.0, 512.0, 700.5]], np.float32)
    order = [2, 0, 1]                                                  # descending and ascending frame indices
    got = CR.crop_patches_hip(frames, [used[i] for i in order], boxes)
    del frames
    want = CR.crop_patches_torch(three, order, boxes)
    assert got.shape == (3, 224, 224, 3) and torch.equal(got.cpu(), want)
    assert all(bool(want[i].any()) for i in range(3)) and not torch.equal(want[0], want[1])
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 3. bad arguments
def test_bad_arguments_raise_before_any_launch(dev):
    from seeme_amd import _lib as L
    fr = torch.randint(1, 256, (2, 9, 11, 3), dtype=torch.uint8).to(dev)
    ok = np.array([[5.0, 4.0, 6.0]], np.float32)
    with pytest.raises(L.SeemeError, match="ROCm device"):
        CR.crop_patches_hip(fr.cpu(), [0], ok)
    for fop, boxes, S, msg in (([2], ok, 8, r"frame_of_patch\[0\] is 2"), ([-1], ok, 8, r"frame_of_patch\[0\] is -1"),
                               ([0], np.array([[np.nan, 4, 6]], np.float32), 8, "centre"), ([0], np.array([[5, 4, 0]], np.float32), 8, "b = 0"),
                               ([0], np.array([[5, 4, 2.0 ** 21]], np.float32), 8, "b = 2097152"), ([0], ok, 0, "S is 0"),
                               ([0], ok, 1025, "S is 1025"), ([0, 1], ok, 8, "boxes are")):
        with pytest.raises(ValueError, match=msg):
            CR.crop_patches_hip(fr, fop, boxes, S)
    with pytest.raises(ValueError, match="frames are"):
        CR.crop_patches_hip(fr.float(), [0], ok)
    # the C entry's own status codes
    lib = L.lib()
    fop_d, box_d = torch.zeros(1, dtype=torch.int32, device=dev), torch.from_numpy(ok).to(dev)
    out = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev)
    st = L.current_stream()
    good = dict(frames=fr.data_ptr(), n_frames=2, H=9, W=11, fop=fop_d.data_ptr(), boxes=box_d.data_ptr(), n=1, S=8, out=out.data_ptr())
    for change, msg in ((dict(frames=0), "null"), (dict(fop=0), "null"), (dict(boxes=0), "null"), (dict(out=0), "null"),
                        (dict(n_frames=0), "n_frames"), (dict(H=0), "H and W"), (dict(W=16385), "H and W"), (dict(S=0), "S must"),
                        (dict(S=1025), "S must"), (dict(n=0), "n must"), (dict(boxes=box_d.data_ptr() + 1), "aligned")):
        a = dict(good, **change)
        rc = lib.seeme_crop_patches(a["frames"], a["n_frames"], a["H"], a["W"], a["fop"], a["boxes"], a["n"], a["S"], a["out"], st)
        assert rc != 0 and msg in lib.seeme_last_error().decode(), (change, lib.seeme_last_error())
    torch.cuda.synchronize()
    assert not out.any()                                               # nothing was launched


def test_kernel_guards_itself_outside_the_preconditions(dev):
    """Boxes and frame indices the wrapper would refuse, handed to the C entry directly: status 0, an all-zero patch each, never an
    out-of-range read; the valid patches of the same launch are the twin's."""
    fr = torch.randint(1, 256, (2, 9, 11, 3), dtype=torch.uint8)
    inf, nan = float("inf"), float("nan")
    boxes = np.array([[5, 4, 6], [nan, 4, 6], [5, nan, 6], [5, 4, nan], [inf, 4, 6], [5, -inf, 6], [5, 4, inf], [5, 4, 0], [5, 4, -3],
                      [2.0 ** 21, 4, 6], [5, -2.0 ** 21, 6], [5, 4, 2.0 ** 21], [5, 4, 6], [5, 4, 6], [5, 4, 6], [3, 6, 9]], np.float32)
    fop = np.array([1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 2, 2 ** 31 - 1, 0], np.int32)
    S = 8
    out = torch.full((len(fop), S, S, 3), 0xA5, dtype=torch.uint8, device=dev)
    CR._launch(fr.to(dev), torch.from_numpy(fop).to(dev), torch.from_numpy(boxes).to(dev), S, out)       # (L.check: status 0)
    torch.cuda.synchronize()
    out = out.cpu()
    assert not out[1:15].any()
    want = CR.crop_patches_torch(fr, [1, 0], boxes[[0, 15]], S)
    assert torch.equal(out[[0, 15]], want) and want[0].any() and want[1].any()


# ----------------------------------------------------------------------------- 4. a recording with video frames, end to end
def _recording(n, seed=0, H=96, W=128, scene_points=384):
    g = np.random.default_rng(seed)
    walk = lambda w, s: np.cumsum(s * g.standard_normal((n, w)), axis=0)
    rec = {"global_orient": 0.5 * g.standard_normal((1, 3)) + walk(3, 0.03), "body_pose": 0.3 * g.standard_normal((1, 69)) + walk(69, 0.02),
           "transl": g.standard_normal((1, 3)) + walk(3, 0.02), "betas": 0.5 * g.standard_normal(10),
           "wearer_betas": 0.5 * g.standard_normal(10), "scene": g.random((scene_points, 3)) * 6 - 3}
    rec = {k: v.astype(np.float32) for k, v in rec.items()}
    # smooth frames that differ from each other, the box wandering over the left half: (center + b) stays inside the frame
    yy, xx = np.mgrid[0:H, 0:W]
    video = np.stack([np.stack([(xx * 2 + 3 * t) % 256, (yy * 2 + 5 * t) % 256, (xx + yy + 7 * t) % 256], axis=-1) for t in range(n)])
    frames = {"video": video.astype(np.uint8), "center": np.stack([20 + walk(1, 1.0)[:, 0], 10 + walk(1, 1.0)[:, 0]], axis=1).astype(np.float32),
              "scale": g.uniform(0.15, 0.25, n).astype(np.float32)}
    return rec, frames


@pytest.fixture(scope="module")
def backbone_model(dev):
    model, dm, cfg = _mld(dev, "scene_image", **{"model.scheduler.num_inference_timesteps": 10})
    assert model.image_backbone
    return model.eval(), dm, cfg


def test_recording_with_video_equals_recording_with_cut_crops(dev, backbone_model, tmp_path):
    from seeme_amd import recording as R
    model, dm, cfg = backbone_model
    n, T, O, K = 37, 16, 4, 3
    rec, fr = _recording(n)
    index = np.array([0, 3, 8, 9, 17, 20, 26, 30, 33])                 # a sparse video: 9 of the 37 frames
    path = os.path.join(tmp_path, "video.npz")
    np.savez(path, **rec, **dict(fr, video=fr["video"][index], video_index=index))
    with_video = R.load_recording(path)
    cond = tuple(cfg.model.condition)
    batch, starts, lengths = R.windows_batch(with_video, dm, T, O, cond, dataset="egobody", device=dev)
    assert starts == [0, 12, 24] and lengths == [16, 16, 13]          # centres 8, 20, 30: all three are stored
    at = [8, 20, 30]
    boxes = CR.boxes_of(fr["center"][at], fr["scale"][at])
    want = CR.crop_patches_torch(torch.from_numpy(fr["video"]), at, boxes)
    assert batch[5].is_cuda and batch[5].dtype == torch.uint8 and torch.equal(batch[5].cpu(), want)
    assert all(bool(want[i].any()) for i in range(3)) and not torch.equal(want[0], want[1])
    # the same recording with image_crops cut by the twin: the same batch, and with the same seeds the same motion and path
    cut = CR.crop_patches_torch(torch.from_numpy(fr["video"]), list(index), CR.boxes_of(fr["center"][index], fr["scale"][index]))
    path2 = os.path.join(tmp_path, "crops.npz")
    np.savez(path2, **rec, image_crops=cut.numpy(), video_index=index)
    batch2 = R.windows_batch(R.load_recording(path2), dm, T, O, cond, dataset="egobody", device=dev)[0]
    assert all(torch.equal(a, b) for a, b in zip(batch, batch2))
    W = len(starts)
    lat, cn = _draws(W, K, model.do_classifier_free_guidance, dev, seed=5)
    betas = torch.from_numpy(rec["wearer_betas"]).to(dev)
    outs = [model.predict_recording(b, n, overlap=O, betas=betas, num_hypotheses=K, latents=lat, cond_noise=cn) for b in (batch, batch2)]
    assert outs[0]["motion"].shape == (n, model.vae.nfeats) and torch.isfinite(outs[0]["motion"]).all()
    assert torch.equal(outs[0]["motion"], outs[1]["motion"]) and torch.equal(outs[0]["path"], outs[1]["path"])
    # the crops are really read: other frames, another motion
    other = list(batch)
    other[5] = torch.flip(batch[5], dims=[0])
    moved = model.predict_recording(tuple(other), n, overlap=O, betas=betas, num_hypotheses=K, latents=lat, cond_noise=cn)
    assert not torch.equal(moved["predict"]["m_rst_all"], outs[0]["predict"]["m_rst_all"])


def test_cli_predict_main_with_video(dev, backbone_model, tmp_path):
    from seeme_amd import cli
    model, dm, cfg = backbone_model
    ckpt = os.path.join(tmp_path, "model.ckpt")
    cli.save_checkpoint(ckpt, model, 0, 0)
    n = 37
    rec, fr = _recording(n, seed=3)
    rec_path, npy, out_path = os.path.join(tmp_path, "rec.npz"), os.path.join(tmp_path, "frames.npy"), os.path.join(tmp_path, "motion.npz")
    np.savez(rec_path, **rec, center=fr["center"], scale=fr["scale"])
    np.save(npy, fr["video"])
    argv = ["--cfg", os.path.join(REPO, "configs", CFG), "--checkpoint", ckpt, "--folder", str(tmp_path), "--frames", "16", "--scene_points", "384",
            "--input", rec_path, "--output", out_path, "--num_hypotheses", "2", "--overlap", "4", "--seed", "11"]
    r = cli.predict_main(argv + ["--video", npy])
    assert r["file"] == out_path and r["n_frames"] == n and r["windows"] == 3
    with np.load(out_path, allow_pickle=False) as z:
        first = {k: z[k] for k in z.files}
    assert first["global_orient"].shape == (n, 3) and first["joints"].shape == (n, 24, 3) and all(np.isfinite(v).all() for v in first.values())
    # the video key in the file is the same recording: the same motion under the same seed
    both = os.path.join(tmp_path, "both.npz")
    np.savez(both, **rec, **fr)
    cli.predict_main([a if a != rec_path else both for a in argv])
    with np.load(out_path, allow_pickle=False) as z:
        assert all(np.array_equal(z[k], first[k]) for k in first)


# ----------------------------------------------------------------------------- 5. crop files for training
def test_crop_files_feed_the_data_modules_crop_route(dev, tmp_path):
    from seeme_amd import data as D
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD
    from seeme_amd.smpl import SMPL
    from seeme_amd.weights_recipe import load_recipe_
    from test_data_module import write_dataset
    root = str(tmp_path / "egobody")
    items, _ = write_dataset(root, "egobody", n=4, T=12, P=32, full_every=2)

    def read_frame(name):                                             # seeded by the name; two frame sizes
        # (write_dataset draws center in 0..1 and scale in 0..1: the box spans b/2 .. 3b/2 with b <= 200, so it meets these frames)
        g = np.random.default_rng(zlib.crc32(name.encode()))
        return g.integers(1, 256, (240, 320, 3) if name.endswith(("0.jpg", "5.jpg")) else (200, 300, 3), dtype=np.uint8)

    frames = {}
    for split in ("train", "test"):
        entries = [(nm, c, s) for (sp, _n), it in sorted(items.items()) if sp == split
                   for nm, c, s in zip(it["recording_utils"]["original_imgname"], it["recording_utils"]["center"], it["recording_utils"]["scale"])]
        frames.update({nm: read_frame(nm) for nm, _c, _s in entries})
        res = CR.write_crop_files(entries, frames.__getitem__, root, split, device=dev, batch=8)
        names, crops = np.load(res["names"], allow_pickle=False), np.load(res["crops"], mmap_mode="r", allow_pickle=False)
        assert names.tolist() == sorted({e[0] for e in entries}) and crops.shape == (len(names), 224, 224, 3)
        box = {nm: CR.boxes_of(c, s) for nm, c, s in entries}
        for i in range(0, len(names), 5):                             # every fifth row against the twin
            nm = str(names[i])
            assert np.array_equal(crops[i], CR.crop_patches_torch(torch.from_numpy(frames[nm])[None], [0], box[nm])[0].numpy()), nm
            assert crops[i].any(), nm
        assert res["launches"] < len(names)
    dm = D.EgoDataModule(root, "egobody", condition=("text", "image", "scene"), motion_length=12, device=dev, scene_root=root,
                         image_backbone=True)
    cfg = parse_config(os.path.join(REPO, "configs", CFG))
    cfg.model.scheduler.num_inference_timesteps = 5
    torch.manual_seed(7)
    model = MLD(cfg, dm, smpl_model=SMPL.synthetic(1234))
    load_recipe_(model.vae), load_recipe_(model.denoiser), load_recipe_(model.proscene)
    model = model.to(dev).eval()
    tb = next(iter(dm.iterate("test", 4)))
    assert tb[5].dtype == torch.uint8 and tb[5].shape[1:] == (224, 224, 3) and bool(tb[5].any())
    assert model.test_step(tb).shape[1:] == (12, 24, 3)
