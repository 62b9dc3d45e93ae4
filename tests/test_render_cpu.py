"""The rasteriser on the CPU: the plain-torch twin of seeme_render against the Python integers of tests/render_reference.py (bit for
bit on ids, inv_depth and dropped) on hand-made scenes at the edges of the definition (tests/render_cases.py), literal expectations
for those scenes, the shading twin on hand-computed normals, the cameras, the PNG writer, the binding, and the refusals of
render_hip, load_motion and cli.render_main that need no device."""
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import render_cases as RC
import render_reference as REF
from conftest import REPO
from seeme_amd import render as RD

CFG = os.path.join(REPO, "configs", "config_mld_scene.yaml")


def as_torch(s):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    return dict(s, verts=t(s["verts"]), faces=t(s["faces"]), cams=t(s["cams"]), points=t(s["points"]))


def twin(s):
    return {k: v.numpy() for k, v in RD.render_torch(**as_torch(s)).items()}


@pytest.fixture(scope="module")
def hand():
    """name -> (reference, twin) of every hand scene, computed once."""
    return {name: (REF.render(**s), twin(s)) for name, s in RC.HAND.items()}


def same(a, b):
    return all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in ("ids", "inv_depth", "dropped"))


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", sorted(RC.HAND))
def test_twin_equals_the_integers(name, hand):
    ref, got = hand[name]
    H, W = RC.HAND[name]["size"]
    assert got["ids"].shape == got["inv_depth"].shape == (1, H, W) and got["dropped"].shape == (1,)
    assert got["ids"].dtype == got["inv_depth"].dtype == got["dropped"].dtype == np.int32
    assert same(ref, got)
    assert ((got["ids"] == -1) == (got["inv_depth"] == 0)).all()           # (every depth here is finite: q > 0 on a drawn pixel)


def test_triangle_through_pixel_centres(hand):
    """Corners (2,2), (10,2), (2,10), positive area2: the tie rule (dy > 0, or dy = 0 and dx < 0) gives the triangle its diagonal
    B -> C (dy > 0) and neither the top edge A -> B (dy = 0, dx > 0) nor the left edge C -> A (dy < 0)."""
    ref, got = hand["triangle"]
    want = np.zeros(RC.SIZE, bool)
    for i in range(3, 10):
        for j in range(3, 10):
            want[i, j] = j + i <= 12
    assert np.array_equal(got["ids"][0] == 0, want)
    assert (got["inv_depth"][0][want] == RD.Q_ONE // 2).all()              # z = 1, near = 0.5


def test_quad_and_fan_have_one_owner_per_pixel(hand):
    ref, got = hand["quad"]
    inside = np.zeros(RC.SIZE, bool)
    inside[4:12, 4:12] = True                                               # the bottom and right edges are in, the top and left out
    assert np.array_equal(ref["cover"][0], inside.astype(np.int64))
    assert np.array_equal(got["ids"][0] >= 0, inside)
    assert (np.diag(got["ids"][0])[4:12] == got["ids"][0][4, 4]).all()      # the shared diagonal went to ONE of the two
    ref, got = hand["fan"]
    inside[:] = False
    inside[5:13, 5:13] = True
    assert np.array_equal(ref["cover"][0], inside.astype(np.int64)) and ref["cover"][0, 8, 8] == 1
    assert np.array_equal(got["ids"][0] >= 0, inside)


def test_zero_area_draws_nothing(hand):
    ref, got = hand["nothing"]
    assert (got["ids"] == -1).all() and (got["inv_depth"] == 0).all() and got["dropped"][0] == 0 and ref["cover"].sum() == 0


def test_both_windings_draw_the_same(hand):
    assert same(hand["triangle"][1], hand["triangle_cw"][1])


def test_borders(hand):
    ref, got = hand["borders"]
    ids = got["ids"][0]
    assert set(np.unique(ids).tolist()) == {-1, 0, 1, 2, 3, 4, 9}           # the partly visible ones and the one around pixel (0,0)
    assert ids[0, 0] == 9 and (ids == 9).sum() == 1 and (ids[0, :] >= 0).any() and (ids[-1, :] >= 0).any() and (ids[:, 0] >= 0).any() and (ids[:, -1] >= 0).any()
    assert got["dropped"][0] == 0
    assert hand["borders_1x1"][1]["ids"].tolist() == [[[9]]]                # pixel (0,0) of the 37 x 29 image
    assert np.array_equal(hand["borders_1x16"][1]["ids"][0], ids[:1, :16])


def test_bad_corner_drops_its_face_and_only_it(hand):
    ref, got = hand["bad_corners"]
    assert got["dropped"][0] == 3 and set(np.unique(got["ids"]).tolist()) == {-1, 0, 4}
    alone = twin(RC.scene(RC.BAD_CORNERS[[0, 4]]))
    assert np.array_equal(alone["ids"] == 0, got["ids"] == 0) and np.array_equal(alone["ids"] == 1, got["ids"] == 4)
    assert np.array_equal(alone["inv_depth"], got["inv_depth"]) and alone["dropped"][0] == 0


def test_equal_depth_goes_to_the_lower_id_and_nearer_wins(hand):
    ref, got = hand["twins"]
    assert ref["cover"].max() == 2 and set(np.unique(got["ids"]).tolist()) == {-1, 0}
    ref, got = hand["crossing"]
    ids = got["ids"][0]
    assert (ids == 0).any() and (ids == 1).any()
    both = ref["cover"][0] == 2
    one = twin(RC.scene(RC.CROSSING[:1]))["inv_depth"][0]
    two = twin(RC.scene(RC.CROSSING[1:]))["inv_depth"][0]
    assert both.sum() > 50
    assert np.array_equal(got["inv_depth"][0], np.maximum(one, two))       # per pixel the nearer one (the larger inverse depth)
    assert np.array_equal(ids[both] == 0, (one >= two)[both])              # ... and the lower id where they tie


def test_extreme_corners_stay_inside_int64(hand):
    """Corners at +-COORD_MAX with Q = 2^22: the reference asserts the header's 2^61 bound on Python's big integers, and the twin's
    int64 arithmetic gives the same bits."""
    ref, got = hand["extreme"]
    assert (ref["cover"] == 1).all() and set(np.unique(got["ids"]).tolist()) == {0, 1} and (got["inv_depth"] == RD.Q_ONE).all()
    assert hand["extreme_1x1"][1]["inv_depth"].tolist() == [[[RD.Q_ONE]]]
    A, B, C = [(int(v[0] / v[2] * 16), int(v[1] / v[2] * 16), RD.Q_ONE) for v in RC.EXTREME[0]]
    assert {abs(c) for v in (A, B, C) for c in v[:2]} == {RD.COORD_MAX}
    w = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
    assert w == 1 << 38 and w * RD.Q_ONE == 1 << 60


def test_points(hand):
    NF = 2
    ids1 = hand["points_1"][1]["ids"][0]
    assert ids1[4, 3] == NF + 0                                             # X = 40, Y = 56: (40 + 8) >> 4 = 3, (56 + 8) >> 4 = 4
    assert ids1[0, 0] in (NF + 1, NF + 3) and ids1[0, 0] == NF + 1          # X = -8 rounds up to 0; equal depth: the lower id
    assert not (ids1 == NF + 2).any()                                       # X = -9 is column -1
    assert ids1[36, 28] == NF + 4 and ids1[0, 28] == NF + 5 and ids1[36, 0] == NF + 6
    assert ids1[10, 10] == 0 or ids1[10, 10] == 1                           # a point at the face's exact depth loses
    assert ids1[10, 12] == NF + 8 and ids1[10, 14] in (0, 1)                # nearer wins, farther loses
    assert not (ids1 >= NF + 10).any()                                      # behind near, NaN
    ids2, ids3 = hand["points_2"][1]["ids"][0], hand["points_3"][1]["ids"][0]
    assert (ids2[36, 28] == NF + 4) and (ids2 == NF + 4).sum() == 1         # even size spans 0 .. +1: clipped to one pixel at the far corner
    assert (ids2[0:2, 0:2] >= NF).all()                                     # ... and whole at the near one
    assert (ids3 == NF + 4).sum() == 4 and (ids3[35:37, 27:29] == NF + 4).all()      # odd size spans -1 .. +1
    assert (ids3 == NF + 8).sum() == 9 and (ids3[9:12, 11:14] == NF + 8).all()
    only = hand["points_only"][1]
    assert (only["ids"][0][3:7, 2:6] == 0).all() and only["dropped"][0] == 0       # -1 .. +2 around (4, 3); NF = 0, so point 0 is id 0


def test_frames_are_independent_and_one_camera_is_every_camera():
    for names, s in RC.batches():
        got = twin(s)
        F = len(names)
        for f, name in enumerate(names):
            alone = twin(dict(s, verts=s["verts"][f:f + 1]))
            assert all(np.array_equal(alone[k][0], got[k][f]) for k in got), name
            if RC.HAND[name]["verts"].shape[1] == s["verts"].shape[1]:      # not padded: the hand scene itself
                assert same(alone, twin(RC.HAND[name]))
        rep = twin(dict(s, cams=np.repeat(s["cams"], F, axis=0)))
        assert same(rep, got)


def test_moving_camera_frames_equal_their_own_render():
    t = RC.random_triangles()
    s = RC.scene(t)
    cams = np.stack([RD.look_at((0.3 * f, -0.2 * f, -0.5 * f), (14.0, 18.0, 1.0), (0, -1, 0)) @ np.eye(4) for f in range(3)]).astype(np.float32)
    s3 = dict(s, verts=np.repeat(s["verts"], 3, axis=0), cams=cams, intrinsics=(20.0, 20.0, 14.0, 18.0), near=0.25)
    got = twin(s3)
    assert same(got, REF.render(**s3))
    for f in range(3):
        alone = twin(dict(s3, verts=s3["verts"][f:f + 1], cams=cams[f:f + 1]))
        assert all(np.array_equal(alone[k][0], got[k][f]) for k in got)
    assert not np.array_equal(got["ids"][0], got["ids"][2])


def test_random_triangles_equal_the_integers():
    s = RC.scene(RC.random_triangles())
    ref, got = REF.render(**s), twin(s)
    assert same(ref, got) and got["dropped"][0] == 6 and (got["ids"] >= 0).all()      # (triangle 0 fills the screen)
    assert len(np.unique(got["ids"])) > 20


def test_closed_sphere_is_covered_an_even_number_of_times():
    """uv_sphere(84, 82) has SMPL's size; fully in view every pixel it touches is covered by one front and one back face (the tie rule
    gives every shared edge and vertex to exactly one triangle on each side)."""
    v, f = RD.uv_sphere(84, 82, radius=0.5, centre=(0.1, -0.05, 2.0))
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    s = {"verts": v[None], "faces": f, "cams": RC.CAM, "intrinsics": (60.0, 60.0, 23.5, 17.5), "size": (36, 48), "points": None, "near": 0.1,
         "point_size": 1}
    ref, got = REF.render(**s), twin(s)
    assert same(ref, got) and got["dropped"][0] == 0
    assert (ref["cover"] % 2 == 0).all() and set(np.unique(ref["cover"]).tolist()) == {0, 2}
    disc = ref["cover"][0] == 2
    assert 500 < disc.sum() < 900 and not disc[0].any() and not disc[-1].any() and not disc[:, 0].any() and not disc[:, -1].any()


# ----------------------------------------------------------------------------- shading
def test_shade_twin_on_hand_computed_normals():
    # world coordinates, fx = fy = 64, so at z = 64 a unit is a pixel.  Three faces: facing the camera (n along z), tilted 45 degrees
    # about x (|n_z| / |n| = 1 / sqrt 2) and tilted 60 degrees (1/2)
    t = np.array([[(0, 0, 64), (8, 0, 64), (0, 8, 64)],
                  [(10, 0, 64), (18, 0, 64), (10, 8, 72)],                  # (8,0,0) x (0,8,8) = (0,-64,64)
                  [(0, 10, 64), (6, 10, 64), (0, 16, 64)]], np.float32)
    t[2, 2] = (0, 16, 64 + 6 * np.sqrt(3))                                  # (6,0,0) x (0,6,6 sqrt 3) = (0,-36 sqrt 3,36)
    s = RC.scene(t, points=[(20.0, 20.0, 64.0)], size=(24, 24), point_size=2)
    s = dict(s, intrinsics=(64.0, 64.0, 0.0, 0.0))
    r = RD.render_torch(**as_torch(s))
    pal = torch.tensor([[200, 100, 50], [10, 20, 255]], dtype=torch.uint8)
    rgb = RD.shade_torch(torch.from_numpy(s["verts"]), torch.from_numpy(s["faces"]), torch.from_numpy(s["cams"]), r["ids"],
                         torch.tensor([0, 1, 0]), pal, torch.from_numpy(s["points"]), torch.tensor([[1, 2, 3]], dtype=torch.uint8),
                         bg=(9, 8, 7)).numpy()[0]
    ids = r["ids"][0].numpy()
    assert rgb.shape == (24, 24, 3) and rgb.dtype == np.uint8
    assert (rgb[ids == -1] == (9, 8, 7)).all() and (ids == -1).any()
    assert (rgb[ids == 3] == (1, 2, 3)).all() and (ids == 3).sum() == 4
    assert (rgb[ids == 0] == (200, 100, 50)).all() and (ids == 0).any()     # level 1
    lvl = 0.3 + 0.7 / np.sqrt(2.0)
    assert (rgb[ids == 1] == tuple(int(np.floor(c * lvl + 0.5)) for c in (10, 20, 255))).all() and (ids == 1).any()
    lvl = 0.3 + 0.7 * 0.5
    got = rgb[ids == 2]
    want = np.array([int(np.floor(c * lvl + 0.5)) for c in (200, 100, 50)])
    assert (ids == 2).any() and (np.abs(got.astype(int) - want) <= 1).all()  # (sqrt 3 is not exact in float32: 130 and 65 sit on .0)
    with pytest.raises(ValueError, match="mesh_of_face"):
        RD.shade_torch(torch.from_numpy(s["verts"]), torch.from_numpy(s["faces"]), torch.from_numpy(s["cams"]), r["ids"],
                       torch.tensor([0, 2, 0]), pal, torch.from_numpy(s["points"]), torch.tensor([[1, 2, 3]], dtype=torch.uint8))


# ----------------------------------------------------------------------------- cameras
def test_look_at_and_orbit_camera():
    M = RD.look_at((1.0, 2.0, 3.0), (4.0, -1.0, 0.5), (0.0, 0.0, 1.0))
    A = M[:3, :3]
    assert np.allclose(A @ A.T, np.eye(3), atol=1e-12) and np.linalg.det(A) > 0 and np.array_equal(M[3], (0, 0, 0, 1))
    assert np.allclose(M @ (1.0, 2.0, 3.0, 1.0), (0, 0, 0, 1), atol=1e-12)             # the eye is the origin
    c = M @ (4.0, -1.0, 0.5, 1.0)
    assert np.allclose(c[:2], 0, atol=1e-12) and c[2] > 0                              # the target is on the optical axis, in front
    assert (A @ (0.0, 0.0, 1.0))[1] < 0                                                # up points up in the image (y is down)
    with pytest.raises(ValueError, match="up"):
        RD.look_at((0, 0, 0), (0, 0, 1), (0, 0, 2))
    g = np.random.default_rng(3)
    pts = g.normal(size=(500, 3)) * (2.0, 0.5, 1.0) + (5.0, -3.0, 1.0)
    from seeme_amd.recording import check_world2cam
    for az, el, fov, up, (H, W) in ((30, 20, 60, (0, 0, 1), (120, 160)), (200, -35, 40, (0, 1, 0), (160, 120)), (0, 80, 90, (1, 0, 0), (64, 64))):
        M = RD.orbit_camera(pts, az, el, fov, up, aspect=W / H)
        check_world2cam(M[None], 1)
        fx, fy, cx, cy = RD.intrinsics(fov, (H, W))
        p = pts @ M[:3, :3].T + M[:3, 3]
        u, v = fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy
        assert (p[:, 2] > 0).all() and u.min() >= 0 and u.max() <= W - 1 and v.min() >= 0 and v.max() <= H - 1
        mid = M @ np.append(0.5 * (pts.min(0) + pts.max(0)), 1.0)
        assert np.allclose(mid[:2], 0, atol=1e-9)
        assert max(u.max() - u.min(), (v.max() - v.min()) * W / H) > 0.3 * W           # ... and the view is not mostly empty
    with pytest.raises(ValueError, match="elevation"):
        RD.orbit_camera(pts, 0, 90, 60)
    with pytest.raises(ValueError, match="fov"):
        RD.intrinsics(180, (4, 4))


# ----------------------------------------------------------------------------- files
def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3)


def test_write_png_round_trip(tmp_path):
    g = np.random.default_rng(1)
    for shape in ((1, 1, 3), (7, 5, 3), (29, 37, 3)):
        img = g.integers(0, 256, shape, dtype=np.uint8)
        path = os.path.join(tmp_path, "a.png")
        RD.write_png(path, img)
        assert np.array_equal(_decode_png(open(path, "rb").read()), img)
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img)
    with pytest.raises(ValueError, match="rgb"):
        RD.write_png(os.path.join(tmp_path, "b.png"), np.zeros((4, 4), np.uint8))


# ----------------------------------------------------------------------------- the binding
def test_entry_points_are_declared_bound_and_exported():
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    for name in ("seeme_render_workspace_bytes", "seeme_render", "seeme_render_shade"):
        proto = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, code)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib._SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert "render.hip" in open(os.path.join(REPO, "seeme_amd", "csrc", "build.sh")).read()
    m = re.search(r"typedef struct \{([^}]*)\} SeemeRenderScene;", code)
    fields = re.findall(r"(\w+)\s*[;,]", m.group(1))
    assert fields == [n for n, _ in _lib.RenderScene._fields_]
    for macro, value in (("SUB", RD.SUB), ("COORD_MAX", RD.COORD_MAX), ("Q", RD.Q_ONE), ("SIZE_MAX", RD.SIZE_MAX), ("POINT_MAX", RD.POINT_MAX)):
        assert int(re.search(r"#define SEEME_RENDER_%s (\d+)" % macro, hdr).group(1)) == value, macro


def test_workspace_bytes_is_zero_for_every_bad_size():
    from seeme_amd import _lib
    ws = _lib.lib().seeme_render_workspace_bytes
    assert ws(3, 100, 29, 37) == (3 * 29 * 37 * 8 + 15) // 16 * 16 + 3 * 100 * 16
    assert ws(1, 0, 1, 1) == 16 and ws(65535, 1 << 24, 1, 1) > 0 and ws(1, 0, 4096, 4096) == 4096 * 4096 * 8
    for bad in ((0, 1, 1, 1), (65536, 1, 1, 1), (-1, 1, 1, 1), (1, -1, 1, 1), (1, (1 << 24) + 1, 1, 1), (1, 1, 0, 1), (1, 1, 4097, 1),
                (1, 1, 1, 0), (1, 1, 1, 4097), (1, 1, -5, 8)):
        assert ws(*bad) == 0, bad


# ----------------------------------------------------------------------------- refusals
def test_refusals_name_their_argument(tmp_path):
    from seeme_amd import _lib
    s = as_torch(RC.HAND["points_1"])
    with pytest.raises(_lib.SeemeError, match="verts must be a tensor on the ROCm device"):
        RD.render_hip(**s)
    with pytest.raises(_lib.SeemeError, match="ids must be a tensor on the ROCm device"):
        RD._on_device("shade_hip", verts=None, ids=torch.zeros(1, 2, 2, dtype=torch.int32))
    with pytest.raises(_lib.SeemeError, match="verts must be a tensor on the ROCm device"):
        RD.shade_hip(s["verts"], s["faces"], s["cams"], torch.zeros(1, 37, 29, dtype=torch.int32), torch.zeros(2, dtype=torch.int64),
                     torch.zeros(1, 3, dtype=torch.uint8), s["points"], torch.zeros(12, 3, dtype=torch.uint8))
    bad = [("verts", dict(verts=s["verts"].double())), ("verts", dict(verts=s["verts"][0])), ("cams", dict(cams=s["cams"].repeat(2, 1, 1))),
           ("faces", dict(faces=s["faces"].float())), ("faces", dict(faces=s["faces"] + 1)), ("faces", dict(faces=s["faces"] - 1)),
           ("points", dict(points=s["points"][:, :2])), ("size", dict(size=(0, 5))), ("size", dict(size=(5, 4097))), ("size", dict(size=7)),
           ("intrinsics", dict(intrinsics=(1.0, 1.0, float("nan"), 0.0))), ("intrinsics", dict(intrinsics=(1.0, 1.0, 0.0))),
           ("near", dict(near=0.0)), ("near", dict(near=float("inf"))), ("point_size", dict(point_size=0)),
           ("point_size", dict(point_size=9)), ("point_size", dict(point_size=2.0))]
    for word, change in bad:
        with pytest.raises(ValueError, match=word):
            RD.render_torch(**dict(s, **change))
    path = os.path.join(tmp_path, "m.npz")
    good = {"global_orient": np.zeros((5, 3), np.float32), "body_pose": np.zeros((5, 69), np.float32), "transl": np.zeros((5, 3), np.float32)}
    np.savez(path, **good)
    assert set(RD.load_motion(path, 5)) == set(good)
    with pytest.raises(ValueError, match="global_orient"):
        RD.load_motion(path, 6)
    for key, value in (("body_pose", np.zeros((5, 60), np.float32)), ("transl", np.full((5, 3), np.nan, np.float32))):
        np.savez(path, **dict(good, **{key: value}))
        with pytest.raises(ValueError, match=key):
            RD.load_motion(path, 5)
    np.savez(path, **{k: v for k, v in good.items() if k != "transl"})
    with pytest.raises(ValueError, match="transl"):
        RD.load_motion(path, 5)


def _recording(n, seed=0, **extra):
    g = np.random.default_rng(seed)
    rec = {"global_orient": 0.1 * g.standard_normal((n, 3)), "body_pose": 0.1 * g.standard_normal((n, 69)),
           "transl": g.standard_normal((n, 3)), "betas": 0.5 * g.standard_normal(10), "wearer_betas": 0.5 * g.standard_normal(10),
           "scene": g.random((64, 3)) * 6 - 3}
    rec = {k: v.astype(np.float32) for k, v in rec.items()}
    rec.update(extra)
    return rec


def test_render_main_refusals_need_no_device(tmp_path):
    from seeme_amd import cli
    from seeme_amd.smpl import SMPL
    n = 4
    rec_path, mot_path, out = (os.path.join(tmp_path, f) for f in ("rec.npz", "motion.npz", "frames.npy"))
    rec = _recording(n)
    np.savez(rec_path, **rec)
    np.savez(mot_path, **{k: rec[k] for k in ("global_orient", "body_pose", "transl")})
    argv = ["--cfg", CFG, "--folder", str(tmp_path), "--input", rec_path, "--motion", mot_path, "--output", out, "--size", "12x16"]
    with pytest.raises(ValueError, match="world2cam"):
        cli.render_main(argv + ["--view", "ego"])
    assert not SMPL.synthetic(1).faces_tensor.any()                         # the stand-in's table is all zeros
    with pytest.raises(ValueError, match="smpl_path"):
        cli.render_main(argv, smpl_model=SMPL.synthetic(1))
    with pytest.raises(ValueError, match="--size"):
        cli.render_main(argv[:-1] + ["640"])
    cam = os.path.join(tmp_path, "cam.npy")
    np.save(cam, np.zeros((3, 4, 4)))
    with pytest.raises(ValueError, match="--camera"):
        cli.render_main(argv + ["--camera", cam])
    np.save(cam, 2 * np.eye(4))
    with pytest.raises(ValueError, match="rigid"):
        cli.render_main(argv + ["--camera", cam])
    assert not os.path.exists(out)
