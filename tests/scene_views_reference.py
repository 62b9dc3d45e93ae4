"""Independent restatements for the scene-view tests: the selection written from its definition as a per-view loop (mask, [::k],
[:P], cyclic fill), clouds and views with controlled survivor counts, the margin condition on the inputs, Rodrigues' formula and
its inverse.  numpy float64 throughout; nothing here calls the code under test."""
import numpy as np

MARGIN = 1e-3           # no vertex within this distance of a view's plane: the fp32 classification is then unambiguous


def restate(verts, M, P):
    """verts [N,3], M [W,4,4] float64 -> cloud [W,P,3], index [W,P], count [W]."""
    W = M.shape[0]
    cloud, index, count = np.zeros((W, P, 3)), np.full((W, P), -1, np.int64), np.zeros(W, np.int64)
    for w in range(W):
        p = verts @ M[w, :3, :3].T + M[w, :3, 3]
        idx = np.flatnonzero(p[:, 2] > 0)
        n = count[w] = len(idx)
        if n >= P:
            k = int(n / P)
            sel = idx[::k][:P]
        elif n > 0:
            sel = idx[np.arange(P) % n]
        else:
            continue
        cloud[w], index[w] = p[sel], sel
    return cloud, index, count


def margin(verts, M):
    """The smallest distance of a vertex to a view's plane z' = 0, float64."""
    z = np.einsum("wc,nc->wn", M[:, 2, :3], verts) + M[:, 2, 3:4]
    return float(np.abs(z).min())


def cloud(N, seed=0):
    """Vertices at z_i = 0.01 i + 0.005 with random x, y in [-3, 3]."""
    g = np.random.default_rng(seed)
    v = g.uniform(-3.0, 3.0, (N, 3))
    v[:, 2] = 0.01 * np.arange(N) + 0.005
    return v


def view_with_count(N, c, flip=False):
    """A view that translates along z so that exactly c of ``cloud(N)`` survive: the LAST c vertices, or with flip (z -> -z) the
    FIRST c.  Every vertex is at least 0.005 from the plane."""
    M = np.eye(4)
    if flip:
        M[2, 2], M[2, 3] = -1.0, 0.01 * c
    else:
        M[2, 3] = -0.01 * (N - c)
    return M


def rodrigues(aa):
    """Axis-angle [...,3] -> rotation matrices [...,3,3]: I + sin(t) K + (1 - cos(t)) K^2, t = |aa| exactly (no offset)."""
    aa = np.asarray(aa, np.float64)
    t = np.linalg.norm(aa, axis=-1)[..., None, None]
    k = aa / np.maximum(np.linalg.norm(aa, axis=-1, keepdims=True), 1e-300)
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def log_rotation(R):
    """Rotation matrices [...,3,3] with an angle away from 0 and pi -> axis-angle [...,3] (trace and antisymmetric part)."""
    t = np.arccos(np.clip((np.trace(R, axis1=-2, axis2=-1) - 1.0) / 2.0, -1.0, 1.0))
    v = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    return v * (t / (2.0 * np.sin(t)))[..., None]


def rigid(rotvec, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = rodrigues(np.asarray(rotvec, np.float64)), t
    return M


def rotated_view(verts, rotvec, keep, t_xy=(0.0, 0.0)):
    """A view rotated by rotvec whose depth offset is put in the middle of a gap of the vertices' depths wider than 4 MARGIN, so
    that about `keep` (0..1) of them survive (a single vertex: it survives, half a metre in front of the plane)."""
    M = rigid(rotvec, [t_xy[0], t_xy[1], 0.0])
    z = np.sort(verts @ M[2, :3])
    if len(z) < 2:
        M[2, 3] = 0.5 - z[0]
        return M
    m = int(round((1.0 - keep) * (len(z) - 1)))
    for step in range(len(z)):
        for i in (m + step, m - step):
            if 1 <= i < len(z) and z[i] - z[i - 1] > 4 * MARGIN:
                M[2, 3] = -0.5 * (z[i] + z[i - 1])
                return M
    raise AssertionError("no gap wider than the margin")


def controlled_case(N, P, seed=0, min_views=0):
    """(verts [N,3], M [W,4,4], counts): translated views with count in {0, 1, P-1, P, P+1, 2P-1, 2P, 2P+1, N} (those that fit
    into 0..N, in this order), two flipped ones, then rotated ones: three, or as many as make `min_views` views."""
    v = cloud(N, seed)
    counts = [c for c in (0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, N) if 0 <= c <= N]
    views = [view_with_count(N, c) for c in counts]
    views += [view_with_count(N, min(N, P + 1), flip=True), view_with_count(N, N // 2, flip=True)]
    g = np.random.default_rng(seed + 1)
    for i in range(max(3, min_views - len(views))):
        views.append(rotated_view(v, g.normal(size=3) * 0.8, keep=g.uniform(0.1, 0.9), t_xy=g.uniform(-1, 1, 2)))
    return v, np.stack(views), counts
