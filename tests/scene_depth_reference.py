"""Independent float64 restatement of seeme_scene_depth (include/seeme_hip.h): explicit loops over frames and segments, the closest
point of a segment found by the three cases (before a, past c, the perpendicular foot) and not by the clamp formula of the twin in
seeme_amd/recording.py; and the inputs the CPU and GPU tests share."""
import functools

import numpy as np

NEAR_ZERO_M = 2e-5           # hits are compared only on inputs where no frame's max(radius - dist) lies within +-0.02 mm of 0


def scene_depth(jts, lengths, points, segs, radius):
    """jts [W,K,T,J,3], lengths [W], points [N,3], segs [NB,2], radius [NB] -> {"depth" [W,K,T] mm, "cost" [W,K] mm, "hits" [W,K],
    "raw" [W,K,T]: max over points and segments of radius - dist in metres, -inf where nothing counts}, float64."""
    jts, P = np.asarray(jts, np.float64), np.asarray(points, np.float64)
    segs, radius = np.asarray(segs), np.asarray(radius, np.float64)
    W, K, T = jts.shape[:3]
    raw = np.full((W, K, T), -np.inf)
    depth, cost, hits = np.zeros((W, K, T)), np.zeros((W, K)), np.zeros((W, K), np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for w in range(W):
            n = min(max(int(lengths[w]), 0), T)
            for k in range(K):
                for t in range(n):
                    best = -np.inf
                    for b in range(segs.shape[0]):
                        a, c = jts[w, k, t, segs[b, 0]], jts[w, k, t, segs[b, 1]]
                        e = c - a
                        ee = float(e @ e)
                        u = (P - a) @ e                                # where along a -> c the foot falls, times ee
                        d_a = np.sqrt(((P - a) ** 2).sum(-1))
                        d_c = np.sqrt(((P - c) ** 2).sum(-1))
                        foot = a + (u / ee)[:, None] * e if ee > 0 else P * np.nan
                        d_f = np.sqrt(((P - foot) ** 2).sum(-1))
                        dist = np.where(u <= 0, d_a, np.where(u >= ee, d_c, d_f))
                        val = radius[b] - dist
                        val = val[~np.isnan(val)]
                        if val.size:
                            best = max(best, float(val.max()))
                    raw[w, k, t] = best
                    depth[w, k, t] = 1000.0 * max(0.0, best)
                if n > 0:
                    s = 0.0
                    for t in range(n):
                        s += depth[w, k, t]
                    cost[w, k] = s / n
                    hits[w, k] = sum(1 for t in range(n) if depth[w, k, t] > 0)
    return {"depth": depth, "cost": cost, "hits": hits, "raw": raw}


def near_zero(raw):
    """How many frames have their max(radius - dist) within +-NEAR_ZERO_M of 0."""
    return int((np.abs(raw[np.isfinite(raw)]) <= NEAR_ZERO_M).sum())


def case_lengths(W, T):
    """Full windows, for W >= 2 a short last one, for W >= 3 one of 0 frames."""
    n = [T] * W
    if W >= 2:
        n[-1] = max(1, (3 * T) // 4)
    if W >= 3:
        n[W // 2] = 0
    return n


def make_segs(J, NB, g):
    """[NB,2] int32: random pairs of joints; row 1 (where there is one) is a sphere, both ends equal."""
    sg = g.integers(0, J, (NB, 2))
    if NB >= 2:
        sg[1, 1] = sg[1, 0]
    return sg.astype(np.int32)


@functools.lru_cache(maxsize=None)
def inputs(W, K, T, J, N, NB, kind="mixed", seed=0):
    """float32 jts [W,K,T,J,3], int lengths [W], float32 points [N,3], int32 segs [NB,2], float32 radius [NB]; |coordinate| <= 8 m.
    Frames t >= n and joints that no segment names are NaN.  kind: 'mixed' (half the points near joints of random frames, half
    anywhere in the room), 'dense' (one standing body, every point inside the box of the joints of every frame, so none is culled),
    'far' (every point out of reach)."""
    g = np.random.default_rng([W, K, T, J, N, NB, seed])
    lengths = case_lengths(W, T)
    segs = make_segs(J, NB, g)
    radius = g.uniform(0.02, 0.1, NB).astype(np.float32)
    if kind == "dense":
        root = np.zeros((W, K, T, 1, 3)) + g.uniform(-3.0, 3.0, 3)
        spread = 0.3
    else:
        lim = 2.0 if kind == "far" else 6.0
        root = lim * np.tanh(g.uniform(-1.5, 1.5, (W, K, 1, 1, 3)) + np.cumsum(0.02 * g.standard_normal((W, K, T, 1, 3)), axis=2))
        spread = 0.3
    shape = np.clip(spread * g.standard_normal((1, 1, 1, J, 3)), -1.0, 1.0)
    jts = (root + shape + 0.01 * g.standard_normal((W, K, T, J, 3))).astype(np.float32)
    if kind == "dense":
        points = (root[0, 0, 0, 0] + g.uniform(-0.05, 0.05, (N, 3))).astype(np.float32)
    elif kind == "far":
        points = g.uniform(7.0, 8.0, (N, 3)).astype(np.float32)
    else:
        wi, ki, ji = g.integers(0, W, N), g.integers(0, K, N), segs[g.integers(0, NB, N), g.integers(0, 2, N)]
        ti = np.array([g.integers(0, max(lengths[w], 1)) for w in wi])
        near = jts[wi, ki, ti, ji].astype(np.float64) + 0.06 * g.standard_normal((N, 3))
        room = g.uniform(-8.0, 8.0, (N, 3))
        points = np.clip(np.where((g.random(N) < 0.5)[:, None], near, room), -8.0, 8.0).astype(np.float32)
    named = np.zeros(J, bool)
    named[segs.reshape(-1)] = True
    jts[:, :, :, ~named] = np.nan
    for w, n in enumerate(lengths):
        jts[w, :, n:] = np.nan
    for a in (jts, points, segs, radius):
        a.setflags(write=False)
    return jts, tuple(lengths), points, segs, radius


@functools.lru_cache(maxsize=None)
def reference(W, K, T, J, N, NB, kind="mixed", seed=0):
    """The float64 reference on ``inputs`` of the same arguments: computed once, shared, and not to be written to."""
    out = scene_depth(*inputs(W, K, T, J, N, NB, kind, seed))
    for a in out.values():
        a.setflags(write=False)
    return out
