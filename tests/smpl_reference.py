"""Plain references of the axis-angle SMPL kernels (csrc/smpl_kernels.hip: k_smpl_joints, k_smpl_skin, k_smpl_joints_bwd), in
numpy, in the dtype of their inputs: in float64 they are the yardstick, in float32 they give the rounding error a float32 evaluation
of the same operation has, which sets the bound of tests/test_gpu_smpl.py.  Nothing here imports oracle/: lbs64 is a second,
independent restatement of smplx's lbs (tests/test_smpl_cpu.py holds it against O.smpl_lbs), written joint by joint with 3x3
rotations and 3-vectors where the oracle batches 4x4 matrices.

Every input maker draws in float64 and rounds to float32 first, so a float32 and a float64 run see the same numbers."""
import numpy as np

from seeme_amd.smpl import SMPL_EXTRA_VERTEX_IDS, SMPL_PARENTS

SMALL_MAGS = (1e-6, 1e-5, 1e-4, 2.4e-4, 1e-3, 1e-2)
WIDE_MAGS = (np.pi - 1e-3, np.pi, 3.5, 4.0)   # not past 4: near 2 pi the float32 input itself conditions the gradient to ~1e-4


# ----------------------------------------------------------------------------- forward
def rodrigues(r):
    """smplx batch_rodrigues, r [N,3] -> [N,3,3]: angle = ||r + 1e-8||, axis = r / angle, R = I + sin K + (1 - cos) K^2."""
    f = r.dtype.type
    e = r + f(1e-8)
    ang = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
    d = r / ang[:, None]
    s, c1 = np.sin(ang), f(1) - np.cos(ang)
    K = np.zeros((r.shape[0], 3, 3), r.dtype)
    K[:, 0, 1], K[:, 0, 2] = -d[:, 2], d[:, 1]
    K[:, 1, 0], K[:, 1, 2] = d[:, 2], -d[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -d[:, 1], d[:, 0]
    return np.eye(3, dtype=r.dtype)[None] + s[:, None, None] * K + c1[:, None, None] * (K @ K)


def lbs64(model, betas, pose, transl, pose_is_rotmat):
    """Linear blend skinning in the dtype of `betas` (the model arrays and the other inputs are cast to it).
    model: the arrays of seeme_amd.smpl.synthetic_model_arrays (any V); betas [M,10]; pose [M,72] axis-angle, or [M,24,3,3]
    rotation matrices with pose_is_rotmat; transl [M,3] or None.
    Returns a dict: joints [M,24,3], extra [M,21,3] (vertices SMPL_EXTRA_VERTEX_IDS[i] % V), vertices [M,V,3], A [M,24,12] (the
    skinning transforms, rows of [R|t]) and feat [M,224] (betas | R_1..23 - I | 7 zeros)."""
    dt = betas.dtype
    M = betas.shape[0]
    vt, sd, pd = (np.asarray(model[k], dt) for k in ("v_template", "shapedirs", "posedirs"))
    Jr, W = np.asarray(model["J_regressor"], dt), np.asarray(model["lbs_weights"], dt)
    V = vt.shape[0]
    if pose_is_rotmat:
        R = np.asarray(pose, dt).reshape(M, 24, 3, 3)
    else:
        R = rodrigues(np.asarray(pose, dt).reshape(M * 24, 3)).reshape(M, 24, 3, 3)
    eye = np.eye(3, dtype=dt)
    feat = np.zeros((M, 224), dt)
    feat[:, :10] = betas
    feat[:, 10:217] = (R[:, 1:] - eye).reshape(M, 207)
    v_shaped = vt[None] + (sd.reshape(V * 3, 10) @ betas.T).T.reshape(M, V, 3)
    v_posed = v_shaped + (feat[:, 10:217] @ pd).reshape(M, V, 3)
    J = np.stack([Jr @ v_shaped[m] for m in range(M)])                      # rest joints [M,24,3]
    Gr, Gt = np.zeros((M, 24, 3, 3), dt), np.zeros((M, 24, 3), dt)          # world rotation and position of every joint
    Gr[:, 0], Gt[:, 0] = R[:, 0], J[:, 0]
    for j in range(1, 24):
        p = SMPL_PARENTS[j]
        Gr[:, j] = Gr[:, p] @ R[:, j]
        Gt[:, j] = Gt[:, p] + (Gr[:, p] @ (J[:, j] - J[:, p])[:, :, None])[:, :, 0]
    A = np.zeros((M, 24, 3, 4), dt)
    A[..., :3] = Gr
    A[..., 3] = Gt - (Gr @ J[..., None])[..., 0]
    T = (W @ A.reshape(M, 24, 12)).reshape(M, V, 3, 4)                      # per-vertex blended transform
    verts = (T[..., :3] @ v_posed[..., None])[..., 0] + T[..., 3]
    joints = Gt.copy()
    if transl is not None:
        tr = np.asarray(transl, dt)[:, None, :]
        verts, joints = verts + tr, joints + tr
    ids = [i % V for i in SMPL_EXTRA_VERTEX_IDS]
    return dict(joints=joints, extra=verts[:, ids], vertices=verts, A=A.reshape(M, 24, 12), feat=feat)


# ----------------------------------------------------------------------------- d Rodrigues / d axis-angle
def drodrigues(aa, gR, dtype, c1_form="one_minus_cos"):
    """The closed form of k_smpl_joints_bwd, term by term, in `dtype`: aa [N,3], gR = dL/dR [N,3,3] -> dL/d aa [N,3].
    c1_form: how the factor (1 - cos theta) of the K^2 term's derivative is formed, "one_minus_cos" (1 - cos(theta), which cancels
    at small angles) or "half_angle" (2 sin^2(theta / 2), the same function without the cancellation)."""
    if c1_form not in ("one_minus_cos", "half_angle"):
        raise ValueError(c1_form)
    f = np.dtype(dtype).type
    aa, g = np.asarray(aa, dtype), np.asarray(gR, dtype).reshape(-1, 9)
    e = aa + f(1e-8)
    th = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
    d = aa / th[:, None]
    sn, c = np.sin(th), np.cos(th)
    if c1_form == "one_minus_cos":
        c1 = f(1) - c
    else:
        h = np.sin(f(0.5) * th)
        c1 = f(2) * h * h
    dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    tr = g[:, 0] + g[:, 4] + g[:, 8]
    w = np.stack([g[:, 7] - g[:, 5], g[:, 2] - g[:, 6], g[:, 3] - g[:, 1]], axis=1)            # sum(gR o K(v)) = v . w
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
    Gd = np.stack([g[:, a * 3 + 0] * d[:, 0] + g[:, a * 3 + 1] * d[:, 1] + g[:, a * 3 + 2] * d[:, 2] for a in range(3)], axis=1)
    Gtd = np.stack([g[:, 0 * 3 + a] * d[:, 0] + g[:, 1 * 3 + a] * d[:, 1] + g[:, 2 * 3 + a] * d[:, 2] for a in range(3)], axis=1)
    dGd, dw = dot(d, Gd), dot(d, w)
    out = np.zeros_like(aa)
    for k in range(3):
        thk = e[:, k] / th
        pd = np.stack([((f(1) if j == k else f(0)) - d[:, j] * thk) / th for j in range(3)], axis=1)
        pdw, pdGd, Gtdpd, dpd = dot(pd, w), dot(pd, Gd), dot(Gtd, pd), dot(d, pd)
        out[:, k] = c * thk * dw + sn * pdw + sn * thk * (dGd - dd * tr) + c1 * (pdGd + Gtdpd - f(2) * dpd * tr)
    assert out.dtype == np.dtype(dtype)
    return out


def joints_backward(model, betas, pose, dj, dtype, c1_form="one_minus_cos"):
    """Chain rule of the 24 posed joints w.r.t. the axis-angle pose [M,72] and the translation, in `dtype`: the tree walk of
    smpl_bwd_tree (g_p[parent] += g_p[j]; g_W[parent] += g_p[j] rel_j^T + g_W[j] R_j^T; g_R[j] = W_parent^T g_W[j]) followed by
    drodrigues.  dj [M,24,3] = dL/d joints.  Returns (dpose [M,72], dtransl [M,3])."""
    dt = np.dtype(dtype)
    betas, pose = np.asarray(betas, dt), np.asarray(pose, dt)
    M = pose.shape[0]
    gp = np.array(dj, dt).reshape(M, 24, 3)
    Jr, vt, sd = (np.asarray(model[k], dt) for k in ("J_regressor", "v_template", "shapedirs"))
    V = vt.shape[0]
    v_shaped = vt[None] + (sd.reshape(V * 3, 10) @ betas.T).T.reshape(M, V, 3)
    J = np.stack([Jr @ v_shaped[m] for m in range(M)])
    R = rodrigues(pose.reshape(M * 24, 3)).reshape(M, 24, 3, 3)
    Wr = np.zeros_like(R)
    Wr[:, 0] = R[:, 0]
    for j in range(1, 24):
        Wr[:, j] = Wr[:, SMPL_PARENTS[j]] @ R[:, j]
    dtransl = gp.sum(axis=1)
    gW, gR = np.zeros((M, 24, 3, 3), dt), np.zeros((M, 24, 3, 3), dt)
    for j in range(23, 0, -1):
        p = SMPL_PARENTS[j]
        rel = J[:, j] - J[:, p]
        gp[:, p] += gp[:, j]
        gR[:, j] = np.swapaxes(Wr[:, p], 1, 2) @ gW[:, j]
        gW[:, p] += gp[:, j][:, :, None] * rel[:, None, :] + gW[:, j] @ np.swapaxes(R[:, j], 1, 2)
    gR[:, 0] = gW[:, 0]
    dpose = drodrigues(pose.reshape(M * 24, 3), gR.reshape(M * 24, 3, 3), dt, c1_form).reshape(M, 72)
    return dpose, dtransl


def twin_grads(smpl, betas, pose, transl, wgt):
    """(joints, d pose, d transl) of sum(joints * wgt) by autograd through vae_autograd.smpl_joints_torch, in the dtype and on the
    device of the module `smpl` (SMPL.synthetic(...).double() for the float64 yardstick: its regressor fold is float64 too); numpy in,
    numpy out (transl None: d transl is None)."""
    import torch
    from seeme_amd.vae_autograd import smpl_joints_torch
    dev, dtype = smpl.v_template.device, smpl.v_template.dtype
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dev, dtype)
    p = t(pose).requires_grad_(True)
    tr = None if transl is None else t(transl).requires_grad_(True)
    j = smpl_joints_torch(smpl, t(betas), p, tr)
    assert j.dtype == dtype
    (j * t(wgt)).sum().backward()
    n = lambda x: None if x is None else x.detach().cpu().numpy()
    return n(j), n(p.grad), None if tr is None else n(tr.grad)


# ----------------------------------------------------------------------------- inputs
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _axes(n, rng):
    a = rng.standard_normal((n, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def ordinary(M, seed):
    """[M,72] float32 poses drawn N(0, 0.5)."""
    return _f32(0.5 * np.random.default_rng(seed).standard_normal((M, 72)))


def small_angle(mags=SMALL_MAGS, seed=0):
    """One frame per magnitude: 24 random axes, each scaled to exactly that angle.  [len(mags),72] float32."""
    rng = np.random.default_rng(seed)
    return _f32(np.stack([(_axes(24, rng) * m).reshape(72) for m in mags]))


def wide_angle(seed=0):
    """One frame each with all 24 angles at pi - 1e-3, pi, 3.5 and 4.0.  [4,72] float32."""
    return small_angle(WIDE_MAGS, seed + 1000)


def zero_frame():
    return np.zeros((1, 72), np.float32)


def padded_frame(seed=0):
    """An ordinary frame whose entries 66..71 (the two hand joints, which GIMO's 21 body joints leave out) are zero."""
    p = ordinary(1, seed + 2000)
    p[:, 66:] = 0.0
    return p


N_ORDINARY_IN_EDGE_BATCH = 3


def edge_batch(kind, seed=0):
    """An angle-edge batch of the GPU tests: three ordinary frames (they set the yardstick of the backward bound), the zero frame,
    the padded frame, then the six small-angle frames (kind "small", M = 11) or the four wide-angle frames (kind "wide", M = 9).
    Zero, padded, small and wide frames with three ordinary ones would be 15 frames; the tests keep M <= 12, hence two batches.
    Returns (pose [M,72] float32, names: one label per frame)."""
    if kind == "small":
        edge, tags = small_angle(seed=seed), [f"small {m:g}" for m in SMALL_MAGS]
    elif kind == "wide":
        edge, tags = wide_angle(seed), [f"wide {m:.4f}" for m in WIDE_MAGS]
    else:
        raise ValueError(kind)
    pose = np.concatenate([ordinary(N_ORDINARY_IN_EDGE_BATCH, seed + 3000), zero_frame(), padded_frame(seed), edge])
    return pose, ["ordinary"] * N_ORDINARY_IN_EDGE_BATCH + ["zero", "padded"] + tags


def betas_transl_weights(M, seed, transl_scale=1.0):
    """float32 betas [M,10] (N(0, 0.5)), translation [M,3] and joint-loss weights [M,24,3] (unit normal)."""
    rng = np.random.default_rng(seed + 77)
    return _f32(0.5 * rng.standard_normal((M, 10))), _f32(transl_scale * rng.standard_normal((M, 3))), _f32(rng.standard_normal((M, 24, 3)))


# ----------------------------------------------------------------------------- error measure
def frame_err(got, ref):
    """Per frame (first axis): max |got - ref| / max |ref| over that frame's entries.  A vector of length M."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    M = ref.shape[0]
    num = np.abs(got - ref).reshape(M, -1).max(axis=1)
    den = np.abs(ref).reshape(M, -1).max(axis=1)
    return num / np.maximum(den, 1e-300)


def item_err(got, ref):
    """frame_err under the name the rotation-helper tests use: one figure per item (row)."""
    return frame_err(got, ref)
