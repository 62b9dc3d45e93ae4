"""Inputs and a numpy restatement for the K-hypothesis metric tests (tests/test_hypotheses_cpu.py, tests/test_gpu_hypotheses.py).

The per-hypothesis errors and the inclusion decision are ``oracle.mld_oracle.ego_metrics`` on a one-sequence batch wherever that
function reports them (it reports nothing for a sequence it drops); ``np_per_hyp`` restates them for every (b,k) and is itself
checked against the oracle on the kept ones.  The two diversity numbers restate the EgoHMR forms (test_egohmr.py:494-497 joint
standard deviation, :515-520 APD of the joints)."""
import warnings

import numpy as np

from oracle import mld_oracle as O

RECIPE_LENGTHS = [24, 17, 3, 2, 1, 24]


def recipe(B=6, K=5, T=24, lengths=None, seed=9, special=True):
    """ref = random walk over the frames + a per-joint offset; pred[b,k] = ref[b] + 1 cm noise; hypothesis (0,1) drifts 1 m at the
    root, hypothesis (B-1,2) has a random head orientation.  Returns float64 arrays: pred [B,K,T,24,3], ref [B,T,24,3],
    qp [B,K,T,4], q [B,T,4], lengths."""
    rng = np.random.default_rng(seed)
    ref = np.cumsum(0.02 * rng.standard_normal((B, T, 24, 3)), axis=1) + 0.3 * rng.standard_normal((B, 1, 24, 3))
    pred = ref[:, None] + 0.01 * rng.standard_normal((B, K, T, 24, 3))
    q = rng.standard_normal((B, T, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    qp = q[:, None] + 0.01 * rng.standard_normal((B, K, T, 4))
    if special:
        pred[0, 1, :, :, 0] += np.linspace(0.0, 1.0, T)[:, None]
        qp[B - 1, 2] = rng.standard_normal((T, 4))
    lengths = list(RECIPE_LENGTHS if lengths is None else lengths)
    assert len(lengths) == B and max(lengths) <= T
    return pred, ref, qp, q, lengths


def ragged_lengths(B, T):
    """1, 2, 3 and T first, then lengths spread over 1..T."""
    base = [T, 1, 2, 3]
    return [min(T, base[b]) if b < 4 else 1 + (b * 37) % T for b in range(B)]


def align(j):
    j = j - j[..., 0:1, 15:16, :]
    return j - j[..., :, 0:1, :]


def np_per_hyp(pred, ref, lengths):
    """MPJPE, ROOT_ERROR, ACCL [B,K] in mm for every (b,k) (compute.py:364-399,470-474,243-271; ACCL = 0 below three frames)."""
    B, K = pred.shape[:2]
    out = {n: np.zeros((B, K)) for n in ("MPJPE", "ROOT_ERROR", "ACCL")}
    for b in range(B):
        L = int(lengths[b])
        g0 = ref[b] - ref[b, 0:1, 15:16]
        g = (g0 - g0[:, 0:1])[:L]
        for k in range(K):
            p0 = pred[b, k] - pred[b, k, 0:1, 15:16]
            p = (p0 - p0[:, 0:1])[:L]
            out["MPJPE"][b, k] = np.linalg.norm(p - g, axis=-1).mean() * 1000
            out["ROOT_ERROR"][b, k] = np.linalg.norm(p0[:L, 0] - g0[:L, 0], axis=-1).mean() * 1000
            if L >= 3:
                ag, ap = g[:-2] - 2 * g[1:-1] + g[2:], p[:-2] - 2 * p[1:-1] + p[2:]
                out["ACCL"][b, k] = np.linalg.norm(ap - ag, axis=-1).mean() * 1000
    return out


def np_head(qp, q, lengths):
    """Head-orientation error [B,K] (compute.py:338-346,469)."""
    B, K = qp.shape[:2]
    out = np.zeros((B, K))
    for b in range(B):
        for k in range(K):
            L = int(lengths[b])
            out[b, k] = np.mean([np.linalg.norm(np.identity(3) - O._quat_matrix(q[b, t]) @ np.linalg.inv(O._quat_matrix(qp[b, k, t])), "fro")
                                 for t in range(L)])
    return out


def oracle_per_hyp(pred, ref, qp, q, lengths, split):
    """ego_metrics on the one-sequence batch of every (b,k): (kept [B,K] bool, values {name: [B,K]} valid where kept)."""
    B, K, T = pred.shape[:3]
    kept = np.zeros((B, K), bool)
    vals = {n: np.zeros((B, K)) for n in ("MPJPE", "ROOT_ERROR", "ACCL", "HEAD_ORIENTATION_ERROR")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # the oracle takes the mean of an empty acceleration array below three frames
        for b in range(B):
            for k in range(K):
                m = O.ego_metrics(pred[b:b + 1, k], ref[b:b + 1], qp[b, k].reshape(T, 4), q[b].reshape(T, 4), [lengths[b]], split)
                kept[b, k] = m["count_seq"] > 0
                for n in vals:
                    vals[n][b, k] = m[n]
    return kept, vals


def np_diversity(pred, lengths):
    """APD_JOINTS, STD_JOINTS [B] in mm, and the mean distance over unordered pairs [B] (= 2 x APD)."""
    B, K = pred.shape[:2]
    apd, std, pair = np.zeros(B), np.zeros(B), np.zeros(B)
    if K == 1:
        return apd, std, pair
    for b in range(B):
        L = int(lengths[b])
        a = align(pred[b])[:, :L]                                   # [K,L,24,3]
        for t in range(L):
            x = a[:, t]                                             # [K,24,3]
            d = np.linalg.norm(x[:, None] - x[None, :], axis=-1)    # [K,K,24]
            apd[b] += d.sum() / 24 / K / (K - 1) / 2                # test_egohmr.py:519-520
            std[b] += x.std(axis=0, ddof=1).mean()                  # test_egohmr.py:496
            pair[b] += np.mean([np.linalg.norm(x[i] - x[j], axis=-1).mean() for i in range(K) for j in range(i + 1, K)])
        apd[b], std[b], pair[b] = apd[b] / L * 1000, std[b] / L * 1000, pair[b] / L * 1000
    return apd, std, pair


def np_accumulate(mp, keep, apd, std):
    """What HypothesisMetrics.compute reports for one set of sequences."""
    any_ = keep.any(axis=1)
    best = [mp[b][keep[b]].min() for b in range(len(mp)) if any_[b]]
    mean = [mp[b][keep[b]].mean() for b in range(len(mp)) if any_[b]]
    n = max(int(any_.sum()), 1)
    return {"MPJPE_best_of_k": float(np.sum(best)) / n, "MPJPE_mean_of_k": float(np.sum(mean)) / n, "APD_JOINTS": float(apd.mean()),
            "STD_JOINTS": float(std.mean()), "count_seq_k": float(any_.sum())}
