"""The headset's orientation on the CPU: the plain-torch twin of seeme_head_rot_cost in float64 against the explicit rotation-matrix loops
of tests/head_rot_reference.py, its invariances and a closed form, the host-side helpers (camera rotations, the quaternions cut into
windows, the lever arm and its fit), the head_rot key of a recording and the C-ABI of the entry point."""
import os

import numpy as np
import pytest
import torch

import head_rot_reference as HR
from headset_reference import cost_lengths
from seeme_amd import recording as R

TWIN_TOL = 1e-12             # float64 twin against float64 loops, relative to the largest reference value
INVARIANT_DEG = 1e-9         # float64: what a rotation that must not matter may change, degrees
COST_CASES = [(1, 1, 1), (2, 3, 2), (3, 32, 5), (2, 5, 63), (2, 5, 65), (4, 33, 9)]
WIDTHS = (72, 75, 144)       # STITCH_ANGLE, STITCH_ANGLE_TRANSL, STITCH_ROT6D


def _close(got, want):
    got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64
    return float(np.abs(got - want).max()) <= TWIN_TOL * max(float(np.abs(want).max()), 1e-300)


def _inputs(W, K, T, F, **kw):
    """The shared inputs in float64; the device's quaternions, unit to float32 as stored, are made unit to float64 (the definition
    takes unit quaternions and does not normalise them; the loops go through a rotation matrix and have to)."""
    feats, dq = (torch.from_numpy(a).double() for a in HR.rot_inputs(W, K, T, F, **kw))
    return feats, dq / dq.norm(dim=-1, keepdim=True)


# ----------------------------------------------------------------------------- the twin against the loops
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("shape", COST_CASES, ids=str)
def test_head_rot_cost_twin_vs_float64_loops(shape, F):
    W, K, T = shape
    layout = HR.LAYOUT_OF_F[F]
    feats, dq = _inputs(W, K, T, F)
    for lengths in cost_lengths(W, T):
        want_c, want_a = HR.head_rot_cost(feats.numpy(), layout, dq.numpy(), lengths)
        got = R.head_rot_cost_torch(feats, layout, dq, lengths)
        assert set(got) == {"cost", "angle"}
        assert _close(got["cost"], want_c) and _close(got["angle"], want_a), (lengths, got["cost"], want_c)
        for w, n in enumerate(lengths):
            if n <= 1:                                                 # n = 0 and n = 1: exactly 0
                assert float(got["cost"][w].abs().max()) == 0.0 and float(got["angle"][w].abs().max()) == 0.0
            else:
                assert float(got["cost"][w].min()) > 1.0 and float(got["angle"][w, :, n:].abs().sum()) == 0.0
        # frames past the length, joints off the chain and the translation columns take no part; a tensor of lengths is read like a list
        poisoned = torch.full_like(feats, float("nan"))
        pq = torch.full_like(dq, float("nan"))
        cols = torch.from_numpy(HR.chain_columns(F, layout))
        for w, n in enumerate(lengths):
            poisoned[w, :, :n, cols] = feats[w, :, :n, cols]
            pq[w, :n] = dq[w, :n]
        assert int(torch.isnan(poisoned[0, 0, 0]).sum()) == (F - len(cols) if lengths[0] > 0 else F)
        nan = R.head_rot_cost_torch(poisoned, layout, pq, torch.tensor(lengths))
        assert torch.equal(nan["cost"], got["cost"]) and torch.equal(nan["angle"], got["angle"])
    over, full = R.head_rot_cost_torch(feats, layout, dq, [T + 5] * W), R.head_rot_cost_torch(feats, layout, dq, [T] * W)
    assert torch.equal(over["cost"], full["cost"]) and torch.equal(over["angle"], full["angle"])          # a length above T is T


def test_head_rot_cost_twin_takes_the_gimo_widths_and_refuses_others():
    W, K, T = 2, 3, 7
    for F in (66, 69):
        layout = HR.LAYOUT_OF_F[F]
        feats, dq = _inputs(W, K, T, F)
        want_c, want_a = HR.head_rot_cost(feats.numpy(), layout, dq.numpy(), [T, T - 2])
        got = R.head_rot_cost_torch(feats, layout, dq, [T, T - 2])
        assert _close(got["cost"], want_c) and _close(got["angle"], want_a)
    feats, dq = _inputs(W, K, T, 72)
    for layout, width in ((R.STITCH_ROT6D, 72), (R.STITCH_ANGLE, 45), (R.STITCH_ANGLE_TRANSL, 48), (R.STITCH_ANGLE, 50), (3, 72), (True, 72)):
        with pytest.raises(ValueError, match="layout"):
            R.head_rot_cost_torch(feats[..., :width], layout, dq, [T] * W)
    for args in ((feats[0], R.STITCH_ANGLE, dq, [T] * W), (feats, R.STITCH_ANGLE, dq[:, :-1], [T] * W), (feats, R.STITCH_ANGLE, dq, [T]),
                 (feats, R.STITCH_ANGLE, dq, [T, 2.5]), (feats, R.STITCH_ANGLE, dq.float(), [T] * W),
                 (feats.long(), R.STITCH_ANGLE, dq.long(), [T] * W)):
        with pytest.raises(ValueError):
            R.head_rot_cost_torch(*args)
    assert R.head_rot_cost_torch(feats.float(), R.STITCH_ANGLE, dq.float(), [T] * W)["cost"].dtype == torch.float32


# ----------------------------------------------------------------------------- what must not matter, and a closed form
def _turn_world(feats, layout, dq, g):
    """One world rotation g (a quaternion) applied to the global orientation of every frame and to the device."""
    out = feats.clone()
    if layout == HR.ROT6D:
        Gm = torch.from_numpy(HR.quat_matrix(g.numpy()))
        out[..., 0:3], out[..., 3:6] = feats[..., 0:3] @ Gm.T, feats[..., 3:6] @ Gm.T
    else:
        from seeme_amd import geometry as G
        out[..., 0:3] = G.quat_to_aa_torch(R._quat_mul(g.expand_as(feats[..., :4]), R._aa_to_quat(feats[..., 0:3])))
    return out, R._quat_mul(g.expand_as(dq), dq)


@pytest.mark.parametrize("F", WIDTHS)
def test_head_rot_cost_is_blind_to_the_mount_and_to_the_world_frame(F):
    W, K, T = 2, 3, 11
    layout = HR.LAYOUT_OF_F[F]
    feats, dq = _inputs(W, K, T, F)
    lengths = [T, T - 4]
    got = R.head_rot_cost_torch(feats, layout, dq, lengths)
    mount = torch.from_numpy(HR.matrix_quat(HR.aa_matrix([0.3, -2.2, 0.9])))             # a constant rotation on the device's side
    turned = R.head_rot_cost_torch(feats, layout, R._quat_mul(dq, mount.expand_as(dq)), lengths)
    f_w, dq_w = _turn_world(feats, layout, dq, torch.from_numpy(HR.matrix_quat(HR.aa_matrix([-1.4, 0.5, 1.8]))))
    world = R.head_rot_cost_torch(f_w, layout, dq_w, lengths)
    for other, what in ((turned, "mount"), (world, "world")):
        ec, ea = float((other["cost"] - got["cost"]).abs().max()), float((other["angle"] - got["angle"]).abs().max())
        print(f"F {F} {what}: cost moves by {ec:.3e}, angle by {ea:.3e} degrees")
        assert ec <= INVARIANT_DEG and ea <= INVARIANT_DEG
    # a rotation on the HEAD's side that is not constant is seen
    assert float((R.head_rot_cost_torch(feats, layout, R._quat_mul(mount.expand_as(dq), dq), lengths)["cost"] - got["cost"]).abs().max()) > 1.0


@pytest.mark.parametrize("F", WIDTHS)
def test_head_rot_cost_of_one_turned_frame_is_the_closed_form(F):
    """dev_t = h_t (x) c exactly but for frame t0, turned by phi: m = c (x) normalised((n-1) + r(phi)) lies beta = 2 atan2(sin(phi/2),
    n - 1 + cos(phi/2)) from the n-1 frames and phi - beta from frame t0."""
    W, K, T, t0 = 2, 2, 12, 4
    layout = HR.LAYOUT_OF_F[F]
    feats, _ = _inputs(W, K, T, F, hyp_rad=0.0)                        # (every hypothesis is the base)
    to_quat, u = (R._rot6d_to_quat, 6) if layout == HR.ROT6D else (R._aa_to_quat, 3)
    h = None
    for j in HR.CHAIN:
        q = to_quat(feats[:, 0, :, u * j:u * j + u])
        h = q if h is None else R._quat_mul(h, q)
    c = torch.from_numpy(HR.matrix_quat(HR.aa_matrix([0.8, 0.1, -1.3])))
    dq = R._quat_mul(h, c.expand_as(h))
    lengths = [T, T - 3]
    assert float(R.head_rot_cost_torch(feats, layout, dq, lengths)["cost"].abs().max()) <= INVARIANT_DEG
    phi = np.radians(40.0)
    axis = np.array([2.0, -1.0, 2.0]) / 3.0
    turn = torch.tensor([np.cos(phi / 2), *(np.sin(phi / 2) * axis)], dtype=torch.float64)
    dq[1, t0] = R._quat_mul(dq[1, t0], turn)
    got = R.head_rot_cost_torch(feats, layout, dq, lengths)
    n = lengths[1]
    beta = np.degrees(2.0 * np.arctan2(np.sin(phi / 2), n - 1 + np.cos(phi / 2)))
    want = np.full(T, beta)
    want[t0], want[n:] = 40.0 - beta, 0.0
    assert float((got["angle"][1] - torch.from_numpy(want)).abs().max()) <= INVARIANT_DEG
    assert float((got["cost"][1] - ((n - 1) * beta + 40.0 - beta) / n).abs().max()) <= INVARIANT_DEG
    assert float(got["cost"][0].abs().max()) <= INVARIANT_DEG


# ----------------------------------------------------------------------------- host-side helpers
def _rotation(g):
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _rigid(g):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = _rotation(g), 3.0 * g.standard_normal(3)
    return M


def test_camera_rotations_are_the_rotations_of_the_inverse_maps():
    g = np.random.default_rng(3)
    M = np.stack([_rigid(g) for _ in range(9)])
    C = R.camera_rotations(M)
    assert C.shape == (9, 3, 3) and C.dtype == np.float64 and C.flags["C_CONTIGUOUS"]
    assert float(np.abs(C - np.linalg.inv(M)[:, :3, :3]).max()) <= 1e-12
    assert float(np.abs(C @ M[:, :3, :3] - np.eye(3)).max()) <= 1e-12
    R.check_head_rot(C, 9)
    with pytest.raises(ValueError, match="world2cam"):
        R.camera_rotations(M[0])


def test_head_rot_windows_are_the_slices_of_the_window_plan_reframed_by_hand():
    g = np.random.default_rng(4)
    n, T, O = 37, 16, 4
    C = np.stack([_rotation(g) for _ in range(n)])
    starts, lengths = R.window_plan(n, T, O)
    assert lengths[-1] == 13                                           # a short last window
    Mw = np.stack([_rigid(g) for _ in starts])
    for frames in (None, Mw, torch.from_numpy(Mw)):
        q = R.head_rot_windows(C, starts, lengths, T, window_frames=frames)
        assert q.shape == (len(starts), T, 4) and q.dtype == torch.float32 and not q.is_cuda
        assert float((q.double().norm(dim=-1) - 1.0).abs().max()) <= 1e-6
        for w, (lo, ln) in enumerate(zip(starts, lengths)):
            for t in range(ln):
                want = C[lo + t] if frames is None else Mw[w, :3, :3] @ C[lo + t]
                assert float(np.abs(HR.quat_matrix(q[w, t].numpy()) - want).max()) <= 1e-6, (w, t)           # (the float32 of the result)
            assert torch.equal(q[w, ln:], torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(T - ln, 4))
    again = R.head_rot_windows(torch.from_numpy(C).float(), starts, lengths, T)                              # a tensor is read like an array
    assert float((again - R.head_rot_windows(C, starts, lengths, T)).abs().max()) <= 1e-6
    one = R.head_rot_windows(C[:5], [0], [5], 5)                       # a lone window shorter than T, cut to its length
    assert one.shape == (1, 5, 4)
    with pytest.raises(ValueError, match="does not fit"):
        R.head_rot_windows(C[:30], starts, lengths, T)
    with pytest.raises(ValueError, match="expected"):
        R.head_rot_windows(C.reshape(-1, 9), starts, lengths, T)
    with pytest.raises(ValueError, match="window_frames"):
        R.head_rot_windows(C, starts, lengths, T, window_frames=Mw[:-1])


def test_check_head_rot_names_the_key_and_the_frame():
    g = np.random.default_rng(6)
    n = 7
    C = np.stack([_rotation(g) for _ in range(n)])
    out = R.check_head_rot(C.astype(np.float32), n)
    assert out.dtype == np.float64 and out.shape == (n, 3, 3) and float(np.abs(out - C).max()) <= 1e-6
    assert np.array_equal(R.check_head_rot(torch.from_numpy(C), n), C)
    scaled, mirror, nan = C.copy(), C.copy(), C.copy()
    scaled[3] *= 1.01
    mirror[5, :, 0] = -mirror[5, :, 0]
    nan[2, 1, 1] = np.nan
    for bad, frame in ((scaled, 3), (mirror, 5), (nan, 2)):
        with pytest.raises(ValueError, match=f"head_rot of frame {frame}"):
            R.check_head_rot(bad, n, "rec.npz")
    for bad in (C[:-1], C.reshape(n, 9), np.zeros((n, 4, 4)), np.stack([np.eye(3, dtype=np.int64)] * n), np.stack([np.eye(3, dtype=bool)] * n)):
        with pytest.raises(ValueError, match="rec.npz: head_rot"):
            R.check_head_rot(bad, n, "rec.npz")


def test_fit_device_offset_recovers_a_planted_offset_and_head_joint_path_undoes_it():
    g = np.random.default_rng(7)
    n = 50
    C = np.stack([_rotation(g) for _ in range(n)])
    head = np.cumsum(0.02 * g.standard_normal((n, 3)), axis=0) + np.array([0.3, 1.6, -2.0])
    planted = np.array([0.08, 0.11, -0.02])                            # the device 8 cm, 11 cm and -2 cm from joint 15, in its own frame
    path = head + np.einsum("nij,j->ni", C, planted)
    offset, rms = R.fit_device_offset(head, path, C)
    assert offset.dtype == np.float64 and offset.shape == (3,)
    assert float(np.abs(offset - planted).max()) <= 1e-12 and rms <= 1e-9
    back = R.head_joint_path(path, C, offset)
    assert back.dtype == np.float64 and float(np.abs(back - head).max()) <= 1e-12
    assert np.array_equal(R.head_joint_path(path, C, np.zeros(3)), path)
    t_off, t_rms = R.fit_device_offset(torch.from_numpy(head), torch.from_numpy(path), torch.from_numpy(C))  # tensors are read like arrays
    assert np.array_equal(t_off, offset) and t_rms == rms
    noisy = path + 0.005 * g.standard_normal((n, 3))                   # 5 mm per coordinate: an RMS of about 5 sqrt(3) mm is left
    o2, rms2 = R.fit_device_offset(head, noisy, C)
    assert float(np.abs(o2 - planted).max()) <= 0.005 and 5.0 < rms2 < 12.0
    for args in ((head[:-1], path, C), (head, path[:, :2], C), (head, path, C[:, :2])):
        with pytest.raises(ValueError, match="fit_device_offset"):
            R.fit_device_offset(*args)
    for args in ((path[:-1], C, planted), (path, C, planted[:2]), (path, C, [0.0, np.nan, 0.0])):
        with pytest.raises(ValueError, match="head_joint_path"):
            R.head_joint_path(*args)


# ----------------------------------------------------------------------------- the recording file
def test_load_recording_accepts_or_refuses_head_rot(tmp_path):
    g = np.random.default_rng(5)
    n = 9
    rec = {"global_orient": g.standard_normal((n, 3)).astype(np.float32), "body_pose": g.standard_normal((n, 69)).astype(np.float32),
           "transl": g.standard_normal((n, 3)).astype(np.float32), "betas": g.standard_normal(10).astype(np.float32)}
    C = np.stack([_rotation(g) for _ in range(n)])

    def save(name, extra):
        p = os.path.join(tmp_path, name)
        np.savez(p, **rec, **extra)
        return p

    assert "head_rot" not in R.load_recording(save("none.npz", {}))
    for arr in (C, C.astype(np.float32)):                              # a recording in one fixed frame: no world2cam needed
        got = R.load_recording(save("good.npz", {"head_rot": arr}))
        assert got["head_rot"].dtype == np.float64 and np.array_equal(got["head_rot"], arr.astype(np.float64))
    w2c = np.stack([_rigid(g) for _ in range(n)])
    both = R.load_recording(save("both.npz", {"head_rot": C, "world2cam": w2c, "head_path": g.standard_normal((n, 3))}))
    assert np.array_equal(both["head_rot"], C) and np.array_equal(both["world2cam"], w2c) and "head_path" in both
    for name, bad in (("short", C[:-1]), ("flat", C.reshape(n, 9)), ("scaled", 1.01 * C), ("mirror", -C), ("int", np.zeros((n, 3, 3), np.int64))):
        with pytest.raises(ValueError, match="head_rot"):
            R.load_recording(save(name + ".npz", {"head_rot": bad}))


# ----------------------------------------------------------------------------- the C-ABI
def test_head_rot_entry_point_is_declared_bound_and_exported():
    import ctypes
    from conftest import REPO
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = "seeme_head_rot_cost"
    assert f"{name}(" in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
    assert "0 -> 3 -> 6 -> 9 -> 12 -> 15" in hdr and tuple(range(0, R.HEAD_JOINT + 1, 3)) == HR.CHAIN
    assert (R.STITCH_ANGLE, R.STITCH_ANGLE_TRANSL, R.STITCH_ROT6D) == (HR.ANGLE, HR.ANGLE_TRANSL, HR.ROT6D)
    src = open(os.path.join(REPO, "seeme_amd", "csrc", "headset.hip")).read()
    assert f'extern "C" int {name}(' in src and '#include "rec_quat.hpp"' in src and "rec_rot6d_to_quat" in src
    # the argument checks run on the host, before anything is launched
    L = _lib.lib()
    assert L.seeme_head_rot_cost(None, 0, 72, None, None, 1, 1, 1, None, None, None) != 0 and b"null" in L.seeme_last_error()
    assert L.seeme_head_rot_cost(64, 0, 72, 64, 64, 1, 33, 1, 64, None, None) != 0 and b"K must be" in L.seeme_last_error()
    assert L.seeme_head_rot_cost(64, 0, 72, 64, 64, 0, 1, 1, 64, None, None) != 0 and b"W must be" in L.seeme_last_error()
    assert L.seeme_head_rot_cost(64, 0, 72, 64, 64, 1, 1, (1 << 20) + 1, 64, None, None) != 0 and b"T must be" in L.seeme_last_error()
    assert L.seeme_head_rot_cost(64, 0, 72, 64, 64, 1, 1, 1, 64, 66, None) != 0 and b"aligned" in L.seeme_last_error()
    for layout, F in ((2, 72), (0, 45), (1, 48), (0, 50), (3, 72), (-1, 144)):
        assert L.seeme_head_rot_cost(64, layout, F, 64, 64, 1, 1, 1, 64, None, None) != 0
        assert f"layout {layout} with F = {F}".encode() in L.seeme_last_error(), (layout, F)
