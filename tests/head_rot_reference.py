"""An independent float64 restatement of seeme_head_rot_cost (include/seeme_hip.h) as explicit numpy loops over ROTATION MATRICES,
written from the formulas and not from the torch twin of seeme_amd/recording.py: the chain 0 -> 3 -> 6 -> 9 -> 12 -> 15 is a product
of matrices, the device is brought into the head's frame as a matrix, and a quaternion is taken only of that one matrix d_t.  And the
inputs the CPU and GPU tests share."""
import numpy as np

HEAD = 15
CHAIN = (0, 3, 6, 9, 12, 15)
ANGLE, ANGLE_TRANSL, ROT6D = 0, 1, 2
LAYOUT_OF_F = {72: ANGLE, 66: ANGLE, 75: ANGLE_TRANSL, 69: ANGLE_TRANSL, 144: ROT6D}


# ----------------------------------------------------------------------------- rotations, one at a time
def aa_matrix(v):
    """Rodrigues: the rotation by |v| about v / |v|."""
    v = np.asarray(v, np.float64)
    th = float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    Kx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + Kx + 0.5 * Kx @ Kx
    return np.eye(3) + (np.sin(th) / th) * Kx + ((1.0 - np.cos(th)) / (th * th)) * Kx @ Kx


def rot6d_matrix(x):
    """Model-side rot6d: a1 = x[0:3], a2 = x[3:6], Gram-Schmidt, columns b1, b2, b1 x b2."""
    x = np.asarray(x, np.float64)
    b1 = x[:3] / max(float(np.linalg.norm(x[:3])), 1e-12)
    u = x[3:6] - float(b1 @ x[3:6]) * b1
    b2 = u / max(float(np.linalg.norm(u)), 1e-12)
    return np.stack([b1, b2, np.cross(b1, b2)], axis=1)


def quat_matrix(q):
    """The rotation of a unit quaternion (w,x,y,z), normalised first."""
    w, x, y, z = np.asarray(q, np.float64) / float(np.linalg.norm(np.asarray(q, np.float64)))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def matrix_quat(R):
    """A unit quaternion (w,x,y,z) of a rotation matrix: the component of largest magnitude first, then the others from it."""
    d = [1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1.0 + R[0, 0] - R[1, 1] - R[2, 2], 1.0 - R[0, 0] + R[1, 1] - R[2, 2],
         1.0 - R[0, 0] - R[1, 1] + R[2, 2]]
    i = int(np.argmax(d))
    r = 0.5 * float(np.sqrt(d[i]))
    if i == 0:
        q = [r, (R[2, 1] - R[1, 2]) / (4 * r), (R[0, 2] - R[2, 0]) / (4 * r), (R[1, 0] - R[0, 1]) / (4 * r)]
    elif i == 1:
        q = [(R[2, 1] - R[1, 2]) / (4 * r), r, (R[0, 1] + R[1, 0]) / (4 * r), (R[0, 2] + R[2, 0]) / (4 * r)]
    elif i == 2:
        q = [(R[0, 2] - R[2, 0]) / (4 * r), (R[0, 1] + R[1, 0]) / (4 * r), r, (R[1, 2] + R[2, 1]) / (4 * r)]
    else:
        q = [(R[1, 0] - R[0, 1]) / (4 * r), (R[0, 2] + R[2, 0]) / (4 * r), (R[1, 2] + R[2, 1]) / (4 * r), r]
    q = np.array(q, np.float64)
    return q / float(np.linalg.norm(q))


def quat_product(p, q):
    return np.array([p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                     p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]])


def head_matrix(row, layout):
    """The global rotation of joint 15 from one frame's feature row."""
    H = np.eye(3)
    for j in CHAIN:
        H = H @ (rot6d_matrix(row[6 * j:6 * j + 6]) if layout == ROT6D else aa_matrix(row[3 * j:3 * j + 3]))
    return H


# ----------------------------------------------------------------------------- the definition
def head_rot_cost(feats, layout, dev_quat, lengths):
    """feats [W,K,T,F], dev_quat [W,T,4], lengths [W] -> (cost [W,K], angle [W,K,T]) float64, degrees."""
    feats, dev_quat = np.asarray(feats, np.float64), np.asarray(dev_quat, np.float64)
    W, K, T = feats.shape[:3]
    cost, angle = np.zeros((W, K)), np.zeros((W, K, T))
    for w in range(W):
        n = min(max(int(lengths[w]), 0), T)
        if n <= 1:
            continue
        C = [quat_matrix(dev_quat[w, t]) for t in range(n)]
        for k in range(K):
            d = [matrix_quat(head_matrix(feats[w, k, t], layout).T @ C[t]) for t in range(n)]
            m = np.zeros(4)
            for t in range(n):
                m = m + (-1.0 if float(d[t] @ d[0]) < 0 else 1.0) * d[t]
            m = m / float(np.linalg.norm(m))
            mc = np.array([m[0], -m[1], -m[2], -m[3]])
            s = 0.0
            for t in range(n):
                r = quat_product(mc, d[t])
                a = 2.0 * float(np.arctan2(np.sqrt(r[1] * r[1] + r[2] * r[2] + r[3] * r[3]), abs(r[0]))) * 180.0 / np.pi
                angle[w, k, t] = a
                s += a
            cost[w, k] = s / n
    return cost, angle


# ----------------------------------------------------------------------------- shared inputs
def chain_columns(F, layout):
    """The columns of a feature row that the definition reads."""
    u = 6 if layout == ROT6D else 3
    return np.concatenate([np.arange(u * j, u * j + u) for j in CHAIN])


def _aa_quat(v):
    th = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.concatenate([np.cos(0.5 * th), np.sin(0.5 * th) * v / np.maximum(th, 1e-300)], axis=-1)


def _qmul(p, q):
    return np.stack([p[..., 0] * q[..., 0] - p[..., 1] * q[..., 1] - p[..., 2] * q[..., 2] - p[..., 3] * q[..., 3],
                     p[..., 0] * q[..., 1] + p[..., 1] * q[..., 0] + p[..., 2] * q[..., 3] - p[..., 3] * q[..., 2],
                     p[..., 0] * q[..., 2] - p[..., 1] * q[..., 3] + p[..., 2] * q[..., 0] + p[..., 3] * q[..., 1],
                     p[..., 0] * q[..., 3] + p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1] + p[..., 3] * q[..., 0]], axis=-1)


def rot_inputs(W, K, T, F, seed=0, noise_deg=10.0, hyp_rad=0.03):
    """float32 (feats [W,K,T,F], dev_quat [W,T,4]) for the layout LAYOUT_OF_F[F].  A base motion turns every joint by about 0.4 rad
    (an axis-angle vector with 0.4 / sqrt(3) rad per component); hypothesis k is the base plus hyp_rad of noise per component.  The
    device is h_t of the base (x) one constant mount rotation (x) noise, the noise an axis-angle vector with noise_deg degrees per
    component, and every other quaternion is stored negated (q and -q are one rotation): the deviations a_t are then of the order of
    10 degrees, every d_t . d_0 is far from 0 and both signs of it occur."""
    layout = LAYOUT_OF_F[F]
    g = np.random.default_rng(100000 * F + 1000 * W + 10 * K + T + seed)
    nj = 24 if layout == ROT6D else F // 3                                 # (with a translation: its columns are drawn like a joint's)
    base = (0.4 / np.sqrt(3.0)) * g.standard_normal((W, 1, T, nj, 3))
    aa = base + hyp_rad * g.standard_normal((W, K, T, nj, 3))
    h = None
    for j in CHAIN:
        q = _aa_quat(base[:, 0, :, j])
        h = q if h is None else _qmul(h, q)                                # [W,T,4]
    mount = _aa_quat(np.array([1.1, -0.7, 2.0]))
    dev = _qmul(_qmul(h, mount), _aa_quat(np.radians(noise_deg) * g.standard_normal((W, T, 3))))
    dev = dev * np.where(g.integers(0, 2, (W, T, 1)) == 1, -1.0, 1.0)
    if layout == ROT6D:
        Rm = np.stack([aa_matrix(v) for v in aa.reshape(-1, 3)]).reshape(W, K, T, nj, 3, 3)
        a1 = 1.3 * Rm[..., :, 0]                                           # not unit, not orthogonal: Gram-Schmidt has work to do
        a2 = 0.8 * Rm[..., :, 1] + 0.2 * Rm[..., :, 0]
        feats = np.concatenate([a1, a2], axis=-1).reshape(W, K, T, 144)
    else:
        feats = aa.reshape(W, K, T, F)
    return feats.astype(np.float32), dev.astype(np.float32)


def planted_inputs(W, K, T, F, star, seed=0):
    """rot_inputs whose hypotheses are drawn independently (0.4 rad per joint each) but for star[w] in window w, whose head follows the
    device up to the constant mount rotation with 0.5 degrees of noise."""
    layout = LAYOUT_OF_F[F]
    g = np.random.default_rng(31 * F + W + K + T + seed)
    nj = 24 if layout == ROT6D else F // 3
    aa = (0.4 / np.sqrt(3.0)) * g.standard_normal((W, K, T, nj, 3))
    dev = np.zeros((W, T, 4))
    for w, k in enumerate(star):
        h = None
        for j in CHAIN:
            q = _aa_quat(aa[w, k, :, j])
            h = q if h is None else _qmul(h, q)
        dev[w] = _qmul(_qmul(h, _aa_quat(np.array([-0.4, 1.9, 0.6]))), _aa_quat(np.radians(0.5) * g.standard_normal((T, 3))))
    if layout == ROT6D:
        Rm = np.stack([aa_matrix(v) for v in aa.reshape(-1, 3)]).reshape(W, K, T, nj, 3, 3)
        feats = np.concatenate([Rm[..., :, 0], Rm[..., :, 1]], axis=-1).reshape(W, K, T, 144)
    else:
        feats = aa.reshape(W, K, T, F)
    return feats.astype(np.float32), dev.astype(np.float32)
