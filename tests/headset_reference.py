"""Independent float64 restatements of the two headset definitions of include/seeme_hip.h, as explicit numpy loops written from the
formulas and not from the torch twins of seeme_amd/recording.py, and the inputs the CPU and GPU tests share."""
import numpy as np

HEAD = 15


def head_path_cost(jts, path, lengths):
    """jts [W,K,T,24,3], path [W,T,3], lengths [W] -> cost [W,K] float64 (mm)."""
    jts, path = np.asarray(jts, np.float64), np.asarray(path, np.float64)
    W, K, T = jts.shape[:3]
    cost = np.zeros((W, K))
    for w in range(W):
        n = min(max(int(lengths[w]), 0), T)
        if n <= 1:
            continue
        for k in range(K):
            r = [jts[w, k, t, HEAD] - path[w, t] for t in range(n)]
            o = np.zeros(3)
            for t in range(n):
                o = o + r[t]
            o = o / n
            s = 0.0
            for t in range(n):
                e = r[t] - o
                s += float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
            cost[w, k] = 1000.0 * s / n
    return cost


def head_anchor(joints, path, taps):
    """joints [L,24,3], path [L,3], taps [R+1] -> (shift [L,3], residual [L]) float64."""
    joints, path, taps = np.asarray(joints, np.float64), np.asarray(path, np.float64), np.asarray(taps, np.float64)
    L, R = joints.shape[0], taps.shape[0] - 1
    r = np.stack([path[n] - joints[n, HEAD] for n in range(L)])
    shift, residual = np.zeros((L, 3)), np.zeros(L)
    for n in range(L):
        acc, ws = np.zeros(3), 0.0
        for d in range(-R, R + 1):
            if 0 <= n + d < L:
                acc = acc + taps[abs(d)] * r[n + d]
                ws += taps[abs(d)]
        shift[n] = acc / ws
        e = r[n] - shift[n]
        residual[n] = 1000.0 * float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
    return shift, residual


def cost_lengths(W, T):
    """Two sets of lengths [W] that between them hold a full window, T-1, 1 and 0 for every W (W = 1: the full window, then 0)."""
    return [[T, T - 1, 1, 0][w % 4] for w in range(W)], [[0, T, T - 1, 1][w % 4] for w in range(W)]


def cost_inputs(W, K, T, seed=0):
    """float32 (jts [W,K,T,24,3], path [W,T,3]): the joints are a common walk within +-2 m plus 0.1 m of noise per hypothesis, the path is
    the walk's head plus a constant offset.  The deviations |r_t - o| are then of the order of 100 mm against coordinates of metres."""
    g = np.random.default_rng(1000 * W + 10 * K + T + seed)
    walk = np.cumsum(0.05 * g.standard_normal((W, T, 1, 3)), axis=1) + g.uniform(-1.0, 1.0, (W, 1, 1, 3))
    walk = 2.0 * np.tanh(walk / 2.0)                                   # within +-2 m
    body = walk + 0.3 * g.standard_normal((1, 1, 24, 3))               # [W,T,24,3]
    jts = body[:, None] + 0.1 * g.standard_normal((W, K, T, 24, 3))
    path = body[:, :, HEAD] + np.array([0.05, -0.08, 0.1])
    return jts.astype(np.float32), path.astype(np.float32)


def anchor_inputs(L, seed=0):
    """float32 (joints [L,24,3], path [L,3]) with r = path - head a random walk with 30 mm steps per coordinate."""
    g = np.random.default_rng(7 * L + seed)
    joints = np.cumsum(0.01 * g.standard_normal((L, 1, 3)), axis=0) + 0.3 * g.standard_normal((1, 24, 3))
    r = np.cumsum(0.03 * g.standard_normal((L, 3)), axis=0)
    return joints.astype(np.float32), (joints[:, HEAD] + r).astype(np.float32)
