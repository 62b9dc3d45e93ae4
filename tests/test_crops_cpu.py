"""The interactee patch on the CPU: the plain-torch twin of seeme_crop_patches against the Python loops of tests/crop_reference.py (bit
for bit) and against plain float64 bilinear interpolation (a derived bound), patch_box on literal numbers, the recording keys that
carry frames (load_recording's refusals, the frame choice of windows_batch, its image slot) and the crop files for training."""
import os
import re

import numpy as np
import pytest
import torch

import crop_reference as REF
from conftest import REPO
from seeme_amd import crops as CR
from seeme_amd import recording as R

CASES = REF.cases()


@pytest.fixture(scope="module")
def twin_results():
    """The twin on every case, computed once."""
    return {c[0]: CR.crop_patches_torch(torch.from_numpy(c[1]), c[2], c[3], c[4]).numpy() for c in CASES}


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_twin_equals_the_loops(case, twin_results):
    name, frames, fop, boxes, S = case
    got = twin_results[name]
    assert got.dtype == np.uint8 and got.shape == (len(fop), S, S, 3)
    assert np.array_equal(got, REF.patches_loops(frames, fop, boxes, S))


def test_case_list_reaches_what_it_names(twin_results):
    """The cases really hold negative coordinates (the flooring shift and the mask), sx = -1 and sx = W - 1, the rne tie, an
    all-zero patch and the rounding half of the final shift."""
    by = {c[0]: c for c in CASES}
    _, frames, fop, boxes, S = by["37x53_S7"]
    W = frames.shape[2]
    names = [b[0] for b in REF._boxes_for(37, 53)]
    X = {n: REF.coords(*boxes[i], S)[0] for i, n in enumerate(names)}
    Y = {n: REF.coords(*boxes[i], S)[1] for i, n in enumerate(names)}
    assert X["sx_minus_one"][0] >> 5 == -1 and X["sx_minus_one"][0] & 31 == 16        # the mask of a negative X
    assert X["sx_last"][0] >> 5 == W - 1
    assert min(X["over_left"]) < 0 and max(X["over_right"]) >> 5 >= W and min(Y["over_top"]) < 0 and max(Y["over_bottom"]) >> 5 >= 37
    assert len(set(X["subpixel"])) > 1 and max(X["subpixel"]) - min(X["subpixel"]) < 32
    out = twin_results["37x53_S7"]
    assert not out[names.index("outside")].any() and out[names.index("inside")].any()
    assert out[names.index("sx_minus_one")][:, 0].any() and out[names.index("sx_last")][:, 0].any()      # one tap in, one out
    # m 1024 = 512.5 exactly: rne(512.5) = 512 at u = 1 and rne(1537.5) = 1538 at u = 3
    b = float(by["rne_tie_S224"][3][0, 2])
    assert (b / 224) * 1024 == 512.5 and round((b / 224) * 1 * 1024) == 512 and round((b / 224) * 3 * 1024) == 1538
    assert twin_results["half_of_the_final_shift"].tolist() == [[[[1, 1, 1]]]]
    assert sorted({len(c[2]) for c in CASES if c[0].startswith("n")}) == [1, 3, 65]


def test_patch_box_on_literal_numbers():
    cx, cy, b = CR.patch_box(np.array([[100.0, 50.0], [10.5, -3.25]]), np.array([0.5, 1.12109375]))
    assert cx.dtype == cy.dtype == b.dtype == np.float32
    assert b.tolist() == [100.0, 224.21875]                           # scale * 200
    assert cx.tolist() == [200.0, 234.71875] and cy.tolist() == [150.0, 220.96875]      # center + b, as dataset.py:1670-1672
    # float32 throughout: 0.1f * 200 is not the double product
    s = np.float32(0.3)
    assert float(CR.patch_box([0.0, 0.0], s)[2]) == float(np.float32(s * np.float32(200))) != 0.3 * 200
    assert CR.boxes_of([[1.0, 2.0]], [0.01]).tolist() == [[3.0, 4.0, 2.0]]
    with pytest.raises(ValueError, match="center"):
        CR.patch_box(np.zeros((3, 2)), np.zeros(4))
    assert "dataset.py:1670-1672" in CR.patch_box.__doc__


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_twin_against_float64_bilinear(case, twin_results):
    """The coordinate of a tap is off by at most 1/64 + 1/1024 pixel per axis (two roundings to 1/1024, one to 1/32), a bilinear
    surface moves by at most G per pixel along an axis, and the final shift rounds to nearest: |twin - exact| <= 0.5 + 2 (1/64 +
    1/1024) G, G the largest neighbour difference of the zero-padded frame.  Derived, not measured."""
    name, frames, fop, boxes, S = case
    got = twin_results[name].astype(np.float64)
    for i, (f, bx) in enumerate(zip(fop, boxes)):
        G = REF.neighbour_step(frames[f])
        err = np.abs(got[i] - REF.bilinear_exact(frames[f], bx[0], bx[1], bx[2], S)).max()
        assert err <= 0.5 + 2 * (1 / 64 + 1 / 1024) * G + 1e-9, (name, i, err, G)


def test_twin_refuses_what_the_definition_excludes():
    fr = torch.zeros(2, 5, 6, 3, dtype=torch.uint8)
    ok = np.array([[3.0, 2.0, 4.0]], np.float32)
    with pytest.raises(ValueError, match="frames are"):
        CR.crop_patches_torch(fr.float(), [0], ok)
    with pytest.raises(ValueError, match="frames are"):
        CR.crop_patches_torch(fr[..., :2], [0], ok)
    with pytest.raises(ValueError, match=r"frame_of_patch\[0\] is 2"):
        CR.crop_patches_torch(fr, [2], ok)
    with pytest.raises(ValueError, match=r"frame_of_patch\[1\] is -1"):
        CR.crop_patches_torch(fr, [0, -1], np.repeat(ok, 2, 0))
    with pytest.raises(ValueError, match="frame_of_patch is"):
        CR.crop_patches_torch(fr, [], np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match="boxes are"):
        CR.crop_patches_torch(fr, [0, 1], ok)
    for S in (0, 1025, 2.0, True):
        with pytest.raises(ValueError, match="S is"):
            CR.crop_patches_torch(fr, [0], ok, S)
    for bad, what in (([np.nan, 2, 4], "centre"), ([3, np.inf, 4], "centre"), ([2.0 ** 20 + 1, 2, 4], "centre"), ([3, -2.0 ** 21, 4], "centre"),
                      ([3, 2, 0], "b = 0"), ([3, 2, -1], "b = -1"), ([3, 2, np.nan], "b = nan"), ([3, 2, 2.0 ** 20 + 1], "b = 1048577")):
        with pytest.raises(ValueError, match=re.escape(what)):
            CR.crop_patches_torch(fr, [0, 1], np.array([ok[0], bad], np.float32))
    # the limits themselves are inside
    edge = np.array([[2.0 ** 20, -2.0 ** 20, 2.0 ** 20]], np.float32)
    assert not CR.crop_patches_torch(fr, [1], edge, 4).any()
    big = torch.zeros(1, 1, 16385, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="16385"):
        CR.crop_patches_torch(big, [0], ok)


def test_c_abi_declares_and_exports_the_entry():
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    m = re.search(r"int seeme_crop_patches\(([^;]*)\);", hdr)
    assert m and "seeme_crop_patches" in _lib.exported_symbols() and hasattr(_lib.lib(), "seeme_crop_patches")
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["seeme_crop_patches"][1]) == 10
    for name, v in (("SEEME_CROP_FRAME_MAX", CR.FRAME_MAX), ("SEEME_CROP_PATCH_MAX", CR.PATCH_MAX), ("SEEME_CROP_COORD_MAX", CR.COORD_MAX)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == v
    assert "crop_patches.hip" in open(os.path.join(REPO, "seeme_amd", "csrc", "build.sh")).read()


# ----------------------------------------------------------------------------- recordings
def _recording(n, seed=0):
    g = np.random.default_rng(seed)
    rec = {"global_orient": g.standard_normal((n, 3)), "body_pose": 0.3 * g.standard_normal((n, 69)),
           "transl": g.standard_normal((n, 3)), "betas": g.standard_normal(10)}
    return {k: v.astype(np.float32) for k, v in rec.items()}


def _frames(n, H=24, W=32, seed=1):
    g = np.random.default_rng(seed)
    return {"video": g.integers(0, 256, (n, H, W, 3), dtype=np.uint8),
            "center": np.stack([g.uniform(-4, 8, n), g.uniform(-6, 4, n)], axis=1).astype(np.float32),
            "scale": g.uniform(0.04, 0.1, n).astype(np.float32)}


def _save(tmp_path, name, **keys):
    path = os.path.join(tmp_path, name)
    np.savez(path, **keys)
    return path


def test_load_recording_keeps_frames_uint8_and_refuses_the_rest(tmp_path):
    n = 9
    rec, fr = _recording(n), _frames(n)
    got = R.load_recording(_save(tmp_path, "ok.npz", **rec, **fr))
    assert got["video"].dtype == np.uint8 and np.array_equal(got["video"], fr["video"])
    assert got["center"].dtype == got["scale"].dtype == np.float32 and got["video_index"].tolist() == list(range(n))
    crops = np.zeros((3, 224, 224, 3), np.uint8)
    got = R.load_recording(_save(tmp_path, "crops.npz", **rec, image_crops=crops, video_index=np.array([0, 4, 8], np.int32)))
    assert got["image_crops"].dtype == np.uint8 and got["video_index"].dtype == np.int64 and got["video_index"].tolist() == [0, 4, 8]
    feats = np.zeros((n, 2048), np.float32)
    refusals = {
        "'image_feats', 'video'": dict(**fr, image_feats=feats),
        "ONE image source": dict(**fr, image_crops=crops, video_index=np.array([0, 4, 8])),
        "image_feats', 'image_crops": dict(image_feats=feats, image_crops=crops, video_index=np.array([0, 4, 8])),
        "video is": dict(fr, video=fr["video"].astype(np.float32)),
        "video is .*expected uint8": dict(fr, video=fr["video"][..., :2]),
        "image_crops is": dict(image_crops=np.zeros((n, 224, 200, 3), np.uint8)),
        "center is missing": {k: v for k, v in fr.items() if k != "center"},
        "scale is missing": {k: v for k, v in fr.items() if k != "scale"},
        "center is": dict(fr, center=fr["center"][:4]),
        "scale is": dict(fr, scale=fr["scale"].astype(np.int32)),
        "video holds 3 frames and the recording 9": dict(fr, video=fr["video"][:3]),
        "video_index is": dict(fr, video_index=np.arange(n, dtype=np.float32)),
        "video_index is .*expected integers": dict(fr, video_index=np.arange(n - 1)),
        "strictly increasing": dict(fr, video=fr["video"][:3], video_index=np.array([0, 4, 4])),
        "strictly increasing inside 0..8": dict(fr, video=fr["video"][:3], video_index=np.array([0, 4, 9])),
        "increasing": dict(fr, video=fr["video"][:3], video_index=np.array([-1, 4, 8])),
        "holds neither": dict(video_index=np.arange(n)),
    }
    for i, (msg, keys) in enumerate(refusals.items()):
        with pytest.raises(ValueError, match=msg):
            R.load_recording(_save(tmp_path, f"bad{i}.npz", **rec, **keys))
    # --video: the frames from a .npy, memory-mapped, in place of the key; both is an error
    npy = os.path.join(tmp_path, "frames.npy")
    np.save(npy, fr["video"])
    no_video = _save(tmp_path, "novideo.npz", **rec, center=fr["center"], scale=fr["scale"])
    got = R.load_recording(no_video, video=npy)
    assert isinstance(got["video"], np.memmap) and got["video"].dtype == np.uint8 and np.array_equal(got["video"], fr["video"])
    with pytest.raises(ValueError, match="ONE image source"):
        R.load_recording(os.path.join(tmp_path, "ok.npz"), video=npy)
    obj = os.path.join(tmp_path, "obj.npy")
    np.save(obj, np.array([{"a": 1}], dtype=object), allow_pickle=True)
    with pytest.raises(ValueError, match="[Oo]bject|pickle"):
        R.load_recording(no_video, video=obj)


def test_frame_choice_of_a_window():
    starts, lengths = R.window_plan(19, 8, 3)                         # [0, 5, 10, 15], [8, 8, 8, 4]: centres 4, 9, 14, 17
    assert R.choose_frames(np.arange(19), starts, lengths) == [4, 9, 14, 17]                  # identity: the centre frame itself
    assert R.choose_frames(np.array([2, 9, 13, 18]), starts, lengths) == [0, 1, 2, 3]         # sparse: rows, not frames
    assert R.choose_frames(np.array([1, 6, 11, 18]), starts, lengths) == [1, 2, 2, 3]         # one stored frame may serve two windows
    # the tie: frames 3 and 5 are both one away from the centre 4 of window 0 -> the earlier; window 1 (5..12, centre 9): 8 and 10
    assert R.choose_frames(np.array([3, 5, 8, 10, 14, 16]), starts, lengths) == [0, 2, 4, 5]
    # the nearest frame INSIDE the window: 13 is nearer to the centre 9 of window 1 than 5, and outside 5..12
    assert R.choose_frames(np.array([2, 5, 13, 15]), starts, lengths) == [1, 1, 2, 3]
    with pytest.raises(ValueError, match=r"window 2 \(frames 10\.\.17\)"):
        R.choose_frames(np.array([0, 7, 18]), starts, lengths)


def test_windows_batch_image_slot_is_the_twin_on_the_chosen_frames(tmp_path):
    n, T, O = 19, 8, 3
    rec, fr = _recording(n), _frames(n)
    g = np.random.default_rng(1)
    stats = (g.standard_normal((1, 75)).astype(np.float32), (0.5 + g.random((1, 75))).astype(np.float32))
    cond = ("text", "interactee", "image")
    for index in (None, np.array([3, 5, 8, 10, 14, 16])):
        keys = dict(fr) if index is None else dict(fr, video=fr["video"][index], video_index=index)
        got = R.load_recording(_save(tmp_path, "rec.npz", **rec, **keys))
        batch, starts, lengths = R.windows_batch(got, stats, T, O, cond, dataset="egobody")
        at = [4, 9, 14, 17] if index is None else [3, 8, 14, 16]       # the recording frames of the chosen stored frames
        want = CR.crop_patches_torch(torch.from_numpy(fr["video"]), at, CR.boxes_of(fr["center"][at], fr["scale"][at]))
        assert len(batch) == 6 and batch[4].dtype == torch.uint8 and batch[4].shape == (4, 224, 224, 3)
        assert torch.equal(batch[4], want) and want.any()
        # the same recording with the patches already cut
        stored = at if index is None else list(index)
        cut = CR.crop_patches_torch(torch.from_numpy(fr["video"]), stored, CR.boxes_of(fr["center"][stored], fr["scale"][stored])).numpy()
        pre = R.load_recording(_save(tmp_path, "pre.npz", **rec, image_crops=cut, video_index=np.asarray(stored)))
        assert torch.equal(R.windows_batch(pre, stats, T, O, cond, dataset="egobody")[0][4], want)
    with pytest.raises(ValueError, match=r"window 3 \(frames 15\.\.18\)"):
        sparse = R.load_recording(_save(tmp_path, "sparse.npz", **rec, **dict(fr, video=fr["video"][:2], video_index=np.array([4, 12]))))
        R.windows_batch(sparse, stats, T, O, cond, dataset="egobody")
    # no image source at all: the message of before, word for word; features: as before
    with pytest.raises(ValueError, match="^windows_batch: the model has an 'image' condition and the recording holds no image_feats$"):
        R.windows_batch(dict(rec, n_frames=n), stats, T, O, cond, dataset="egobody")
    feats = g.standard_normal((n, 2048)).astype(np.float32)
    b = R.windows_batch(dict(rec, n_frames=n, image_feats=feats), stats, T, O, cond, dataset="egobody")[0]
    assert torch.equal(b[4], torch.from_numpy(feats[[4, 9, 14, 17]]))
    # a recording without an image condition ignores its frames
    assert len(R.windows_batch(got, stats, T, O, ("text", "interactee"), dataset="egobody")[0]) == 5


# ----------------------------------------------------------------------------- crop files
def test_write_crop_files_with_a_synthetic_reader(tmp_path):
    g = np.random.default_rng(3)
    sizes = {"b/2.jpg": (20, 30), "a/1.jpg": (20, 30), "c/3.jpg": (16, 16), "a/0.jpg": (20, 30), "d/4.jpg": (20, 30)}
    frames = {k: g.integers(0, 256, (h, w, 3), dtype=np.uint8) for k, (h, w) in sizes.items()}
    box = {k: (g.uniform(0, 6, 2).astype(np.float32), np.float32(g.uniform(0.03, 0.08))) for k in sizes}
    entries = [(k, *box[k]) for k in sizes] + [("a/1.jpg", *box["a/1.jpg"])]                   # a repeated name
    read = []
    res = CR.write_crop_files(entries, lambda name: (read.append(name), frames[name])[1], str(tmp_path), "val", batch=2)
    names = np.load(res["names"], allow_pickle=False)
    crops = np.load(res["crops"], allow_pickle=False)
    assert os.path.basename(res["crops"]) == "image_crops_val.npy" and os.path.basename(res["names"]) == "image_crop_names_val.npy"
    assert names.dtype.kind == "U" and names.tolist() == sorted(sizes) == read and res["count"] == 5
    assert crops.dtype == np.uint8 and crops.shape == (5, 224, 224, 3)
    for i, k in enumerate(names.tolist()):
        want = CR.crop_patches_torch(torch.from_numpy(frames[k])[None], [0], CR.boxes_of(*box[k]))[0].numpy()
        assert np.array_equal(crops[i], want) and want.any(), k
    # a/0, a/1 | b/2 | c/3 (another size) | d/4: equal sizes are batched, `batch` at a time
    assert res["launches"] == 4
    with pytest.raises(ValueError, match="two boxes"):
        CR.write_crop_files(entries + [("b/2.jpg", box["b/2.jpg"][0] + 1, box["b/2.jpg"][1])], frames.__getitem__, str(tmp_path), "val")
    with pytest.raises(ValueError, match="read_frame"):
        CR.write_crop_files(entries, lambda name: frames[name].astype(np.float32), str(tmp_path), "val")
    with pytest.raises(ValueError, match="no entry"):
        CR.write_crop_files([], frames.__getitem__, str(tmp_path), "val")
