"""float64 numpy restatement of the social-interaction definitions (include/seeme_hip.h, seeme_social_metrics), written with plain loops
straight from the formulas and independently of seeme_amd/social_metrics.py, and a recipe of inputs: two people 0.3 - 4 m apart with
ragged lengths (tests/test_social_metrics_cpu.py, tests/test_gpu_social_metrics.py)."""
import math

import numpy as np

PER_HYP = ("PERSON_DIST_ERROR", "CLOSEST_DIST", "CLOSEST_DIST_ERROR", "GAZE_ANGLE", "GAZE_ANGLE_ERROR")
PER_SEQ = ("PERSON_DIST", "CLOSEST_DIST_REF", "GAZE_ANGLE_REF")
DIST_EDGES = (1000.0, 2000.0, 3000.0)
GAZE_EDGES = (150.0,)
# pelvis distance (m) and gaze angle (degrees) of the recipe's sequences, cycled over b: every distance bin and both gaze bins
RECIPE_DIST = (0.5, 1.5, 2.5, 3.5, 0.3, 4.0, 1.2, 2.2)
RECIPE_GAZE = (170.0, 60.0, 160.0, 120.0, 175.0, 20.0, 155.0, 90.0)


# ----------------------------------------------------------------------------- the definitions
def gaze(q):
    """Third column of the rotation matrix of q = (w,x,y,z), q scaled by sqrt(2 / |q|^2); |q|^2 < 1e-15 is the identity."""
    n = sum(float(v) * float(v) for v in q)
    if n < 1e-15:
        return np.array([0.0, 0.0, 1.0])
    w, x, y, z = (float(v) * math.sqrt(2.0 / n) for v in q)
    return np.array([x * z + y * w, y * z - x * w, 1.0 - x * x - y * y])


def angle(g, h):
    """atan2(|g x h|, g . h) in degrees, at most 180; between 5 and 175 degrees also the reference's arccos of the normalised dot
    product (compute.py:31), which must agree."""
    cx = g[1] * h[2] - g[2] * h[1]
    cy = g[2] * h[0] - g[0] * h[2]
    cz = g[0] * h[1] - g[1] * h[0]
    a = min(math.atan2(math.sqrt(cx * cx + cy * cy + cz * cz), g[0] * h[0] + g[1] * h[1] + g[2] * h[2]) * (180.0 / math.pi), 180.0)
    if 5.0 <= a <= 175.0:
        ref = np.arccos(np.dot(g, h) / (np.linalg.norm(g) * np.linalg.norm(h))) * 180.0 / np.pi
        assert abs(ref - a) <= 1e-9, (ref, a)
    return a


def closest(x, y):
    """min over the 24 x 24 joint pairs of |x[i] - y[j]|."""
    best = math.inf
    for i in range(24):
        for j in range(24):
            best = min(best, math.sqrt(sum((float(x[i, c]) - float(y[j, c])) ** 2 for c in range(3))))
    return best


def np_social(pred, ref, intr, qp, qr, qi, lengths):
    """{name: [B] or [B,K]} of the eight numbers; n = clamp(len, 0, T), n = 0 gives zeros."""
    B, K, T = pred.shape[:3]
    out = {n: np.zeros(B) for n in PER_SEQ}
    out.update({n: np.zeros((B, K)) for n in PER_HYP})
    for b in range(B):
        n = min(max(int(lengths[b]), 0), T)
        for t in range(n):
            h = gaze(qi[b, t])
            d_ref = float(np.linalg.norm(ref[b, t, 0] - intr[b, t, 0]))
            c_ref = closest(ref[b, t], intr[b, t])
            a_ref = angle(gaze(qr[b, t]), h)
            out["PERSON_DIST"][b] += 1000.0 * d_ref / n
            out["CLOSEST_DIST_REF"][b] += 1000.0 * c_ref / n
            out["GAZE_ANGLE_REF"][b] += a_ref / n
            for k in range(K):
                d = float(np.linalg.norm(pred[b, k, t, 0] - intr[b, t, 0]))
                c = closest(pred[b, k, t], intr[b, t])
                a = angle(gaze(qp[b, k, t]), h)
                out["PERSON_DIST_ERROR"][b, k] += 1000.0 * abs(d - d_ref) / n
                out["CLOSEST_DIST"][b, k] += 1000.0 * c / n
                out["CLOSEST_DIST_ERROR"][b, k] += 1000.0 * abs(c - c_ref) / n
                out["GAZE_ANGLE"][b, k] += a / n
                out["GAZE_ANGLE_ERROR"][b, k] += abs(a - a_ref) / n
    return out


def np_bin(value, edges):
    """The number of edges <= value."""
    return sum(1 for e in edges if e <= value)


def np_labels(edges):
    s = [f"{float(e):g}" for e in edges]
    return [f"lt{s[0]}"] + [f"{a}_{b}" for a, b in zip(s[:-1], s[1:])] + [f"ge{s[-1]}"]


def np_accumulate(social, mpjpe, root, keep, dist_edges=DIST_EDGES, gaze_edges=GAZE_EDGES):
    """What SocialMetrics.compute reports for one set of sequences: social {name: array}, mpjpe / root / keep [B,K]."""
    B, K = mpjpe.shape
    names = ("MPJPE", "ROOT_ERROR") if K == 1 else ("MPJPE_best_of_k", "MPJPE_mean_of_k")
    out = {n: float(np.mean(social[n])) for n in PER_SEQ}
    pairs = [(b, k) for b in range(B) for k in range(K) if keep[b, k]]
    if pairs:
        for n in ("PERSON_DIST_ERROR", "CLOSEST_DIST", "CLOSEST_DIST_ERROR", "GAZE_ANGLE_ERROR"):
            out[n] = float(np.mean([social[n][b, k] for b, k in pairs]))
    out["count_seq_social"], out["count_pairs_social"] = float(B), float(len(pairs))
    for axis, key, edges in (("dist", "PERSON_DIST", dist_edges), ("gaze", "GAZE_ANGLE_REF", gaze_edges)):
        for i, label in enumerate(np_labels(edges)):
            members = [b for b in range(B) if np_bin(social[key][b], edges) == i]
            kept = [b for b in members if keep[b].any()]
            out[f"count_seq_{axis}_{label}"], out[f"count_kept_{axis}_{label}"] = float(len(members)), float(len(kept))
            if kept:
                if K == 1:
                    first, second = [mpjpe[b, 0] for b in kept], [root[b, 0] for b in kept]
                else:
                    first, second = [mpjpe[b][keep[b]].min() for b in kept], [mpjpe[b][keep[b]].mean() for b in kept]
                out[f"{names[0]}_{axis}_{label}"], out[f"{names[1]}_{axis}_{label}"] = float(np.mean(first)), float(np.mean(second))
    return out


# ----------------------------------------------------------------------------- inputs
def _qmul(a, b):
    """Hamilton product of (w,x,y,z) quaternions, [...,4]."""
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def _about(axis, deg):
    """Rotation by deg [...] degrees about the unit axis [...,3], as a quaternion."""
    half = np.deg2rad(deg)[..., None] / 2
    return np.concatenate([np.cos(half), np.sin(half) * axis], axis=-1)


def ragged_lengths(B, T):
    """T, 1, 2 first, then lengths spread over 3..T."""
    return [T, 1, 2][:B] + [min(T, 3 + (b * 5) % max(T - 2, 1)) for b in range(3, B)]


def recipe(B=6, K=3, T=12, lengths=None, seed=5):
    """Two people RECIPE_DIST[b] apart (pelvis to pelvis, in a random horizontal direction), both on a slow random walk, their gaze
    directions RECIPE_GAZE[b] +- 3 degrees apart.  Hypothesis k stands 0.15 + 0.1 (k mod 4) metres further from the interactee than
    the reference (nearer, beyond 2 m) and is turned by 3 + 2 (k mod 5) degrees towards 90 degrees, plus 5 mm / 0.2 degree noise; the quaternions
    are not normalised (lengths 0.5 .. 2).  float64: pred [B,K,T,24,3], ref, intr [B,T,24,3], qp [B,K,T,4], qr, qi [B,T,4], lengths."""
    rng = np.random.default_rng(seed)
    body = np.concatenate([rng.uniform(-0.12, 0.12, (B, 2, 24, 2)), rng.uniform(-0.9, 0.7, (B, 2, 24, 1))], axis=-1)
    body[:, :, 0] = 0.0                                                              # joint 0 is the pelvis itself
    walk = np.cumsum(0.01 * rng.standard_normal((B, 2, T, 1, 3)), axis=2)
    phi = rng.uniform(0, 2 * np.pi, B)
    u = np.stack([np.cos(phi), np.sin(phi), np.zeros(B)], axis=-1)                    # wearer -> interactee, unit
    dist = np.array([RECIPE_DIST[b % len(RECIPE_DIST)] for b in range(B)])
    wiggle = 0.003 * rng.standard_normal((B, 2, T, 24, 3))                            # the joints move: a non-zero acceleration error
    ref = body[:, 0, None] + walk[:, 0] + wiggle[:, 0]
    intr = body[:, 1, None] + walk[:, 1] + wiggle[:, 1] + (dist[:, None] * u)[:, None, None, :]
    sign = np.where(dist > 2.0, 1.0, -1.0)                                            # towards the interactee beyond 2 m, away below
    ks = np.arange(K)
    shift = sign[:, None] * (0.15 + 0.1 * (ks % 4) + 0.002 * ks)[None, :]             # [B,K] metres along u
    pred = ref[:, None] + (shift[:, :, None] * u[:, None, :])[:, :, None, None, :] + 0.005 * rng.standard_normal((B, K, T, 24, 3))
    # orientations: a random one for the interactee; the wearer's is the interactee's turned about an axis normal to its gaze
    qi = rng.standard_normal((B, T, 4))
    qi /= np.linalg.norm(qi, axis=-1, keepdims=True)
    g = np.stack([[gaze(qi[b, t]) for t in range(T)] for b in range(B)])              # [B,T,3]
    other = np.where(np.abs(g[..., 2:3]) < 0.9, np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    axis = np.cross(g, other)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    theta = np.array([RECIPE_GAZE[b % len(RECIPE_GAZE)] for b in range(B)])[:, None] + 3.0 * np.sin(np.arange(T) * 0.7)[None, :]
    qr = _qmul(_about(axis, theta), qi)
    turn = np.where(theta > 90.0, -1.0, 1.0)[:, None, :] * (3.0 + 2.0 * (ks % 5) + 0.05 * ks)[None, :, None] \
        + 0.2 * rng.standard_normal((B, K, T))                                        # [B,K,T] degrees
    qp = _qmul(_about(np.broadcast_to(axis[:, None], (B, K, T, 3)), theta[:, None, :] + turn), qi[:, None])
    qr = qr * rng.uniform(0.5, 2.0, (B, T, 1))
    qp = qp * rng.uniform(0.5, 2.0, (B, K, T, 1))
    qi = qi * rng.uniform(0.5, 2.0, (B, T, 1))
    lengths = list(ragged_lengths(B, T) if lengths is None else lengths)
    assert len(lengths) == B
    return pred, ref, intr, qp, qr, qi, lengths


def assert_recipe_margins(want, lengths):
    """The error terms are differences: on the float64 values every distance error of a sequence with a valid frame is at least
    50 mm and every gaze-angle error at least 1 degree, so that fp32 rounding of 4 m and 180 degrees stays far below the bound."""
    rows = np.array([int(n) > 0 for n in lengths])
    assert rows.any()
    for name, least in (("PERSON_DIST_ERROR", 50.0), ("CLOSEST_DIST_ERROR", 50.0), ("GAZE_ANGLE_ERROR", 1.0)):
        v = np.asarray(want[name], np.float64)[rows]
        assert (v >= least).all(), (name, float(v.min()))
