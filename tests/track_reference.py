"""float64 restatements of the track definitions (include/seeme_hip.h: seeme_track_cost, seeme_track_filter), written independently of
seeme_amd/track.py as explicit numpy loops, and the input generators.  Shared by tests/test_track_cpu.py and tests/test_gpu_track.py."""
import numpy as np

import recording_reference as REF

NLERP_DOT = 0.9995
TILE = 64                    # SEEME_TRACK_TILE


# ----------------------------------------------------------------------------- transition costs
def track_cost_loops(jts, idx, weight):
    jts = np.asarray(jts, np.float64)
    Lf, S = jts.shape[:2]
    cost = np.zeros((max(Lf - 1, 0), S, S))
    for l in range(Lf - 1):
        for i in range(S):
            for j in range(S):
                acc = 0.0
                for k in range(24):
                    d = jts[l, i, k] - jts[l + 1, j, k]
                    acc += d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                cost[l, i, j] = weight * acc / float(idx[l + 1] - idx[l])
    return cost


# ----------------------------------------------------------------------------- quaternions, one at a time
def aa_to_quat(v):
    th = float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    k = np.sin(0.5 * th) / th if th > 1e-6 else 0.5 - th * th / 48.0
    return np.array([np.cos(0.5 * th), k * v[0], k * v[1], k * v[2]])


def quat_to_aa(q):
    if q[0] < 0:
        q = -q
    vn = float(np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
    k = 2.0 * np.arctan2(vn, q[0]) / vn if vn > 1e-12 else 2.0
    return k * q[1:]


def quat_to_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def blend(p, q, u):
    dt = float(p @ q)
    if dt < 0:
        dt, q = -dt, -q
    kp, kq = 1.0 - u, u
    if not dt > NLERP_DOT:
        th = np.arccos(dt)
        kp, kq = np.sin((1.0 - u) * th) / np.sin(th), np.sin(u * th) / np.sin(th)
    r = kp * p + kq * q
    return r / np.sqrt(r @ r)


def fill_loops(pose, transl, idx, L):
    """fill(m), m = 0..L-1: quaternions [L,J,4] and the translation [L,3] (None without one)."""
    pose = np.asarray(pose, np.float64)
    Lf, J = pose.shape[:2]
    Q = np.zeros((L, J, 4))
    T = None if transl is None else np.zeros((L, 3))
    for m in range(L):
        if m <= idx[0]:
            a, u = 0, None
        elif m >= idx[Lf - 1]:
            a, u = Lf - 1, None
        else:
            a = max(k for k in range(Lf) if idx[k] <= m)
            u = None if idx[a] == m else (m - idx[a]) / float(idx[a + 1] - idx[a])
        for j in range(J):
            p = aa_to_quat(pose[a, j])
            Q[m, j] = p if u is None else blend(p, aa_to_quat(pose[a + 1, j]), u)
        if T is not None:
            ta = np.asarray(transl[a], np.float64)
            T[m] = ta if u is None else ta + u * (np.asarray(transl[a + 1], np.float64) - ta)
    return Q, T


def track_filter_loops(pose, transl, idx, L, taps):
    """-> (rotation matrices [L,J,3,3], translation [L,3] or None, axis-angle [L,J,3]) of out(n), n = 0..L-1."""
    taps = np.asarray(taps, np.float64)
    R = taps.shape[0] - 1
    Q, T = fill_loops(pose, transl, idx, L)
    J = Q.shape[1]
    M, A = np.zeros((L, J, 3, 3)), np.zeros((L, J, 3))
    To = None if T is None else np.zeros((L, 3))
    for n in range(L):
        lo, hi = max(0, n - R), min(L - 1, n + R)
        for j in range(J):
            acc = np.zeros(4)
            for m in range(lo, hi + 1):
                s = -1.0 if float(Q[m, j] @ Q[n, j]) < 0 else 1.0
                acc = acc + taps[abs(m - n)] * s * Q[m, j]
            q = acc / np.sqrt(acc @ acc)
            M[n, j], A[n, j] = quat_to_matrix(q), quat_to_aa(q)
        if To is not None:
            acc, ws = np.zeros(3), 0.0
            for m in range(lo, hi + 1):
                acc, ws = acc + taps[abs(m - n)] * T[m], ws + taps[abs(m - n)]
            To[n] = acc / ws
    return M, To, A


def min_abs_dot(pose, idx, L, R):
    """The smallest |dot| of two quaternions that MEET: fill(m) and fill(n) inside one window (|m - n| <= R), or neighbouring keys.
    The tests' condition on their inputs: at 0.1 and more a sign decision is the same in fp32 and in float64."""
    pose = np.asarray(pose, np.float64)
    Q, _ = fill_loops(pose, None, idx, L)
    low = 1.0
    for d in range(1, min(R, L - 1) + 1):
        low = min(low, float(np.abs((Q[d:] * Q[:-d]).sum(-1)).min()))
    for a in range(pose.shape[0] - 1):
        for j in range(pose.shape[1]):
            low = min(low, abs(float(aa_to_quat(pose[a, j]) @ aa_to_quat(pose[a + 1, j]))))
    return low


def matrices(aa):
    return REF.aa_to_matrix(np.asarray(aa, np.float64))


# ----------------------------------------------------------------------------- inputs
def keys_apart(Lf, J, seed, with_transl=True):
    """Keys whose neighbours are 0.3..1.0 rad apart in every joint (quaternion dot product cos(0.15) at most: the slerp branch), each
    key a further rotation of the one before it about a random axis; the translation a walk of 0.1 m steps."""
    g = np.random.default_rng(seed)
    Rm = REF.aa_to_matrix(0.5 * g.standard_normal((J, 3)))
    out = []
    for _ in range(Lf):
        out.append(REF.matrix_log(Rm))
        ax = g.standard_normal((J, 3))
        Rm = Rm @ REF.aa_to_matrix(ax / np.linalg.norm(ax, axis=-1, keepdims=True) * g.uniform(0.3, 1.0, (J, 1)))
    tr = np.cumsum(0.1 * g.standard_normal((Lf, 3)), axis=0) + g.standard_normal((1, 3))
    return np.stack(out), (tr if with_transl else None)


def smooth_keys(idx, L, J, seed, with_transl=True):
    """Keys cut from ONE smooth motion of L frames (a walk of 0.002 rad per component and frame: neighbouring keys stay above
    NLERP_DOT, the lerp branch)."""
    m = REF.random_motion(L, "angle_transl", seed, step=0.002)
    idx = np.asarray(idx)
    return m[idx, :72].reshape(len(idx), 24, 3)[:, :J], (m[idx, 72:] if with_transl else None)


def flip_alternate(pose):
    """Every second key written as the -q axis-angle (theta - 2 pi about the same axis): the same rotations."""
    mask = np.zeros((1, pose.shape[0]), bool)
    mask[0, 1::2] = True
    return REF.flip_representation(np.asarray(pose, np.float64).reshape(1, pose.shape[0], -1), REF.ANGLE, mask)[0].reshape(pose.shape)


def jitter_motion(L, seed, J=24):
    """(smooth, noisy) axis-angle [L,J,3]: a sinusoid of period 40 frames and amplitude 0.6 rad per component (random phases) plus iid
    N(0, 0.05 rad) noise."""
    g = np.random.default_rng(seed)
    t = np.arange(L)[:, None, None]
    smooth = 0.6 * np.sin(2 * np.pi * t / 40.0 + g.uniform(0, 2 * np.pi, (1, J, 3)))
    return smooth, smooth + 0.05 * g.standard_normal((L, J, 3))


def second_difference(Rm):
    """Mean absolute second difference over time of rotation matrices [L,...]."""
    return float(np.abs(Rm[2:] - 2 * Rm[1:-1] + Rm[:-2]).mean())


def candidates(Lf, S, seed, spread=0.15):
    """S candidate bodies per stored frame around one smooth motion: global_orient [Lf,S,3], body_pose [Lf,S,69], transl [Lf,3],
    log_prob [Lf,S] with candidate 0 the most probable."""
    g = np.random.default_rng(seed)
    base = REF.random_motion(Lf, "angle_transl", seed + 1, step=0.03)
    aa = base[:, None, :72] + spread * g.standard_normal((Lf, S, 72))
    lp = -np.sort(g.uniform(0.0, 4.0, (Lf, S)), axis=1)
    return aa[:, :, :3], aa[:, :, 3:], base[:, 72:], lp
