"""seeme_render / seeme_render_shade on the device: the kernels against their plain-torch twins with torch.equal on ids, inv_depth and
dropped (an integer definition: no tolerance), the fp32 shading within one grey level of the float64 twin on face pixels and equal
elsewhere, launch-to-launch and chunking invariance, the entry points' refusals, and cli.render_main end to end on a synthetic
recording with a predict_main output."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import render_cases as RC
from conftest import REPO
from seeme_amd import _lib as L
from seeme_amd import render as RD
from test_render_cpu import _decode_png, as_torch

pytestmark = pytest.mark.gpu
KEYS = ("ids", "inv_depth", "dropped")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def on(s, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in as_torch(s).items()}


def assert_same(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype == torch.int32 and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k].cpu(), want[k].cpu()), (what, k)


# ----------------------------------------------------------------------------- 1. kernel against twin
def test_hand_scenes_batched(dev):
    """(a) every hand scene of tests/render_cases.py, the scenes of one size and point set as the frames of ONE call."""
    for names, s in RC.batches():
        got = RD.render_hip(**on(s, dev))
        assert_same(got, RD.render_torch(**as_torch(s)), names)
        assert_same(RD.render_hip(**on(s, dev)), got, names)               # a second launch, bit for bit


def test_random_triangles(dev):
    """(b) 64 random triangles at 37 x 29: one fills the screen (its box is walked by the whole wave), slivers, corners off the screen,
    behind near and behind the camera."""
    s = RC.scene(RC.random_triangles())
    want = RD.render_torch(**as_torch(s))
    assert int(want["dropped"][0]) == 6 and len(torch.unique(want["ids"])) > 20
    assert_same(RD.render_hip(**on(s, dev)), want)


@pytest.fixture(scope="module")
def bodies():
    """(c) two interpenetrating uv_sphere(84, 82) bodies (SMPL's size each) that move over 3 frames, 2000 points around them, a
    camera per frame, 160 x 120; and the twin's result, computed once."""
    g = np.random.default_rng(17)
    v, f = RD.uv_sphere(84, 82, radius=0.45)
    verts = np.stack([np.concatenate([v * (1.0, 1.0, 1.8) + (0.25 * t, 0.0, 0.0), v * (1.0, 1.8, 1.0) + (0.5 - 0.1 * t, 0.1, 0.2)])
                      for t in range(3)]).astype(np.float32)
    faces = np.concatenate([f, f + v.shape[0]])
    points = (g.random((2000, 3)) * 4 - 2).astype(np.float32)
    cams = np.stack([RD.orbit_camera(verts[0], 20 + 25 * t, 15, 60, (0, 0, 1), aspect=160 / 120, margin=1.0 + 0.2 * t) for t in range(3)])
    s = {"verts": verts, "faces": faces, "cams": cams.astype(np.float32), "intrinsics": RD.intrinsics(60, (120, 160)), "size": (120, 160),
         "points": points, "near": 0.05, "point_size": 1}
    return s, RD.render_torch(**as_torch(s))


def test_two_bodies_and_a_cloud(dev, bodies):
    s, want = bodies
    ids = want["ids"]
    NF = s["faces"].shape[0]
    assert NF == 27552 and ((ids >= 0) & (ids < NF // 2)).any() and ((ids >= NF // 2) & (ids < NF)).any() and (ids >= NF).any() and (ids == -1).any()
    got = RD.render_hip(**on(s, dev))
    assert_same(got, want)
    assert_same(RD.render_hip(**on(s, dev)), got)                           # two launches are equal
    for mb in (0.75, 0.4, 1e-6):                                            # 2 + 1 frames, then a frame per chunk (one needs 0.36 MiB)
        assert_same(RD.render_hip(**on(s, dev), chunk_mb=mb), got, mb)
    one = RD.render_hip(**on(dict(s, verts=s["verts"][1:2], cams=s["cams"][1:2]), dev))
    assert all(torch.equal(one[k][0], got[k][1]) for k in KEYS)             # a frame alone is its slice


def test_one_camera_and_wide_points(dev, bodies):
    """(d) the same with one camera for all frames and point_size 3."""
    s, _ = bodies
    s = dict(s, cams=s["cams"][:1], point_size=3)
    want = RD.render_torch(**as_torch(s))
    got = RD.render_hip(**on(s, dev))
    assert_same(got, want)
    rep = RD.render_hip(**on(dict(s, cams=np.repeat(s["cams"], 3, axis=0)), dev))
    assert_same(rep, got)


def test_workspace_contents_do_not_matter(dev, bodies):
    s, want = bodies
    RD._WS.fill_(0xFF)
    assert_same(RD.render_hip(**on(s, dev)), want)


# ----------------------------------------------------------------------------- 2. shading
def test_shade_kernel_within_one_level_of_the_twin(dev, bodies):
    """A float32 level is far more accurate than half a grey step: only a value that sits on a rounding boundary can move, by one."""
    s, want = bodies
    t = as_torch(s)
    NF, P = s["faces"].shape[0], s["points"].shape[0]
    mof = torch.cat([torch.zeros(NF // 2), torch.ones(NF // 2)]).to(torch.int32)
    pal = torch.tensor([[96, 152, 232], [236, 146, 84]], dtype=torch.uint8)
    prgb = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (P, 3), dtype=np.uint8))
    ref = RD.shade_torch(t["verts"], t["faces"], t["cams"], want["ids"], mof, pal, t["points"], prgb, bg=(24, 24, 28))
    d = on(s, dev)
    got = RD.shade_hip(d["verts"], d["faces"], d["cams"], want["ids"].to(dev), mof.to(dev), pal.to(dev), d["points"], prgb.to(dev),
                       bg=(24, 24, 28))
    assert got.dtype == torch.uint8 and got.shape == (3, 120, 160, 3)
    got = got.cpu()
    face = (want["ids"] >= 0) & (want["ids"] < NF)
    assert face.any() and torch.equal(got[~face], ref[~face])               # points and background: equal
    diff = (got[face].int() - ref[face].int()).abs()
    assert int(diff.max()) <= 1
    assert float((diff > 0).float().mean()) < 0.01                          # ... and a boundary is rare
    again = RD.shade_hip(d["verts"], d["faces"], d["cams"], want["ids"].to(dev), mof.to(dev), pal.to(dev), d["points"], prgb.to(dev),
                         bg=(24, 24, 28))
    assert torch.equal(again.cpu(), got)


# ----------------------------------------------------------------------------- 3. refusals of the entry points
def test_entry_points_refuse_bad_arguments(dev):
    s = on(RC.HAND["points_1"], dev)
    F, NV, NF, P, FC, H, W, k, ps = RD._check_scene("t", s["verts"], s["faces"], s["cams"], s["intrinsics"], s["size"], s["points"], s["near"], 1)
    faces = s["faces"].to(torch.int32)
    ids, inv = (torch.empty(F, H, W, dtype=torch.int32, device=dev) for _ in range(2))
    dropped = torch.empty(F, dtype=torch.int32, device=dev)
    need = L.lib().seeme_render_workspace_bytes(F, NV, H, W)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    stream = L.current_stream()

    def scene(**change):
        sc = RD._scene_struct(s["verts"], faces, s["points"], s["cams"], F, NV, NF, P, FC, H, W, k, ps)
        for name, value in change.items():
            setattr(sc, name, value)
        return sc

    def refused(word, sc, ws_ptr=None, ws_bytes=need, ids_ptr=None):
        with pytest.raises(L.SeemeError, match=word):
            L.call("seeme_render", C.byref(sc), ids.data_ptr() if ids_ptr is None else ids_ptr, inv.data_ptr(), dropped.data_ptr(),
                   ws.data_ptr() if ws_ptr is None else ws_ptr, ws_bytes, stream)

    for word, change in (("F must", dict(F=0)), ("F must", dict(F=65536)), ("FC must", dict(FC=2)), ("H and W", dict(H=0)),
                         ("H and W", dict(W=4097)), ("NV must", dict(NV=-1)), ("NF, P", dict(NF=-1)), ("NF, P", dict(NF=2 ** 31 - 2, P=1)),
                         ("point_size", dict(point_size=0)), ("point_size", dict(point_size=9)), ("fx, fy, cx, cy", dict(cx=float("inf"))),
                         ("znear", dict(znear=0.0)), ("znear", dict(znear=float("nan"))), ("null pointer", dict(cams=0)),
                         ("null pointer", dict(verts=0)), ("null pointer", dict(points=0)), ("4-byte aligned", dict(points=s["points"].data_ptr() + 2))):
        refused(word, scene(**change))
    refused("workspace too small", scene(), ws_bytes=need - 1)
    refused("16-byte aligned", scene(), ws_ptr=ws.data_ptr() + 8)
    refused("null pointer", scene(), ws_ptr=0)
    refused("null pointer", scene(), ids_ptr=0)
    refused("ids, inv_depth and dropped", scene(), ids_ptr=ids.data_ptr() + 1)
    rgb = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    mof, pal, prgb = torch.zeros(NF, dtype=torch.int32, device=dev), torch.zeros(1, 3, dtype=torch.uint8, device=dev), torch.zeros(P, 3, dtype=torch.uint8, device=dev)
    for word, a in (("ids or rgb", (0, mof.data_ptr(), pal.data_ptr(), 1, prgb.data_ptr(), 0, rgb.data_ptr())),
                    ("ids or rgb", (ids.data_ptr(), mof.data_ptr(), pal.data_ptr(), 1, prgb.data_ptr(), 0, 0)),
                    ("mesh_of_face and palette", (ids.data_ptr(), 0, pal.data_ptr(), 1, prgb.data_ptr(), 0, rgb.data_ptr())),
                    ("n_mesh", (ids.data_ptr(), mof.data_ptr(), pal.data_ptr(), 0, prgb.data_ptr(), 0, rgb.data_ptr())),
                    ("point_rgb", (ids.data_ptr(), mof.data_ptr(), pal.data_ptr(), 1, 0, 0, rgb.data_ptr())),
                    ("bg must", (ids.data_ptr(), mof.data_ptr(), pal.data_ptr(), 1, prgb.data_ptr(), 1 << 24, rgb.data_ptr()))):
        with pytest.raises(L.SeemeError, match=word):
            L.call("seeme_render_shade", C.byref(scene()), *a, stream)
    with pytest.raises(ValueError, match="chunk_mb"):
        RD.render_hip(**s, chunk_mb=0)
    with pytest.raises(L.SeemeError, match="points must be a tensor on the ROCm device"):
        RD.render_hip(**dict(s, points=s["points"].cpu()))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 4. cli.render_main
def test_cli_render_main_writes_frames_and_pngs(dev, tmp_path):
    from seeme_amd import cli
    from seeme_amd.smpl import SMPL
    from test_gpu_hyp_select import _mld
    from test_gpu_recording import _mut, _synthetic_recording
    model, dm, cfg = _mld(dev, "config_mld_scene.yaml", mutate=_mut)
    ckpt = os.path.join(tmp_path, "model.ckpt")
    cli.save_checkpoint(ckpt, model, 0, 0)
    n, (H, W) = 21, (48, 64)
    cfg_path = os.path.join(REPO, "configs", "config_mld_scene.yaml")
    rec_path, mot_path = os.path.join(tmp_path, "rec.npz"), os.path.join(tmp_path, "motion.npz")
    np.savez(rec_path, **_synthetic_recording(n, seed=3))
    cli.predict_main(["--cfg", cfg_path, "--checkpoint", ckpt, "--folder", str(tmp_path), "--frames", "16", "--scene_points", "384",
                      "--input", rec_path, "--output", mot_path, "--num_hypotheses", "2", "--overlap", "4", "--seed", "11"])
    sm = SMPL.synthetic(1234)
    sm.faces_tensor = torch.from_numpy(RD.uv_sphere(84, 82)[1])             # the stand-in's own table is all zeros
    out = [os.path.join(tmp_path, f"frames{i}.npy") for i in range(2)]
    png = os.path.join(tmp_path, "png")
    argv = ["--cfg", cfg_path, "--folder", str(tmp_path), "--input", rec_path, "--motion", mot_path, "--size", f"{H}x{W}", "--scene_points", "200"]
    r = cli.render_main(argv + ["--output", out[0], "--png_dir", png], smpl_model=sm)
    assert r["file"] == out[0] and r["n_frames"] == n and r["size"] == (H, W) and 0 < r["scene_points"] <= 200
    a = np.load(out[0])
    assert a.dtype == np.uint8 and a.shape == (n, H, W, 3)
    flat = a.reshape(-1, 3)
    assert (flat == cli.RENDER_BG).all(axis=1).any()                        # the background ...
    for base in cli.RENDER_PALETTE:                                         # ... and both bodies: a shade of its palette row, 0.3 .. 1
        lvl = flat.astype(np.float64) / np.asarray(base, np.float64)
        assert ((np.ptp(lvl, axis=1) < 0.02) & (lvl.min(axis=1) >= 0.29) & (lvl.max(axis=1) <= 1.01)).any(), base
    cli.render_main(argv + ["--output", out[1], "--chunk_mb", "0.1"], smpl_model=sm)      # a frame per chunk: byte-equal
    assert open(out[0], "rb").read() == open(out[1], "rb").read()
    names = sorted(os.listdir(png))
    assert names == [f"frame_{f:06d}.png" for f in range(n)]
    for f in (0, n // 2, n - 1):
        assert np.array_equal(_decode_png(open(os.path.join(png, names[f]), "rb").read()), a[f])
