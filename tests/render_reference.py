"""An independent, slow restatement of the rasteriser's definition (include/seeme_hip.h, seeme_render): the vertex stage in numpy
float64 scalars, everything after it in Python integers (which cannot overflow), one pixel at a time.  It does not import
seeme_amd.render: it is the yardstick for the plain-torch twin, which in turn is the yardstick for the kernels."""
import math

import numpy as np

SUB, COORD_MAX, Q_ONE = 16, 1 << 18, 1 << 22


def project(M, p, k):
    """M [4,4] float32, p [3] float32, k = (fx, fy, cx, cy, near) float32 -> (X, Y, Q) Python integers, or None for an invalid vertex."""
    d = np.float64
    M, (x, y, z) = np.asarray(M, np.float32), (d(v) for v in np.asarray(p, np.float32))
    fx, fy, cx, cy, near = (d(np.float32(v)) for v in k)
    with np.errstate(all="ignore"):
        xc, yc, zc = (((d(M[r, 0]) * x + d(M[r, 1]) * y) + d(M[r, 2]) * z) + d(M[r, 3]) for r in range(3))
        if not (math.isfinite(zc) and zc >= near):
            return None
        X, Y = np.rint(((fx * xc) / zc + cx) * d(16.0)), np.rint(((fy * yc) / zc + cy) * d(16.0))
        if not (math.isfinite(X) and math.isfinite(Y) and abs(X) <= COORD_MAX and abs(Y) <= COORD_MAX):
            return None
        return int(X), int(Y), int(np.rint((near / zc) * d(Q_ONE)))


def _owned(w, dx, dy):
    return w > 0 or (w == 0 and (dy > 0 or (dy == 0 and dx < 0)))


def face_pixels(A, B, C, H, W):
    """Snapped corners (X, Y, Q) -> [(i, j, q)] of the covered pixels; the int64 claim of the header is checked on the way."""
    area2 = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
    if area2 == 0:
        return []
    if area2 < 0:
        B, C, area2 = C, B, -area2
    e = lambda U, V, px, py: (V[0] - U[0]) * (py - U[1]) - (V[1] - U[1]) * (px - U[0])
    out = []
    j_lo, j_hi = max(0, -(-min(A[0], B[0], C[0]) // 16)), min(W - 1, max(A[0], B[0], C[0]) // 16)
    i_lo, i_hi = max(0, -(-min(A[1], B[1], C[1]) // 16)), min(H - 1, max(A[1], B[1], C[1]) // 16)
    for i in range(i_lo, i_hi + 1):
        for j in range(j_lo, j_hi + 1):
            px, py = 16 * j, 16 * i
            w = (e(B, C, px, py), e(C, A, px, py), e(A, B, px, py))
            edges = ((B, C), (C, A), (A, B))
            if all(_owned(w[k], edges[k][1][0] - edges[k][0][0], edges[k][1][1] - edges[k][0][1]) for k in range(3)):
                terms = (w[0] * A[2], w[1] * B[2], w[2] * C[2])
                assert all(abs(t) <= 1 << 61 for t in terms) and abs(sum(terms)) <= 1 << 61, "the header's 2^61 bound"
                out.append((i, j, sum(terms) // area2))
    return out


def render(verts, faces, cams, intrinsics, size, points=None, near=0.05, point_size=1):
    """The arguments of seeme_amd.render.render_torch as numpy arrays -> ids, inv_depth [F,H,W] int32, dropped [F] int32 and cover
    [F,H,W] int64, the number of FACES that cover each pixel (the definition has no such output; the tests count with it)."""
    verts, faces, cams = np.asarray(verts, np.float32), np.asarray(faces, np.int64), np.asarray(cams, np.float32)
    F, (H, W), NF = verts.shape[0], size, faces.shape[0]
    k = tuple(intrinsics) + (near,)
    keys = [[[0] * W for _ in range(H)] for _ in range(F)]
    cover = np.zeros((F, H, W), np.int64)
    dropped = np.zeros(F, np.int32)
    for f in range(F):
        M = cams[f if cams.shape[0] > 1 else 0]
        pv = [project(M, v, k) for v in verts[f]]
        for fi, (a, b, c) in enumerate(faces.tolist()):
            if pv[a] is None or pv[b] is None or pv[c] is None:
                dropped[f] += 1
                continue
            for i, j, q in face_pixels(pv[a], pv[b], pv[c], H, W):
                assert 0 <= q <= Q_ONE
                cover[f, i, j] += 1
                keys[f][i][j] = max(keys[f][i][j], (q << 32) | (0xFFFFFFFF - fi))
        for pi, p in enumerate(() if points is None else np.asarray(points, np.float32)):
            v = project(M, p, k)
            if v is None:
                continue
            j, i = (v[0] + 8) >> 4, (v[1] + 8) >> 4
            for r in range(i - (point_size - 1) // 2, i + point_size // 2 + 1):
                for c in range(j - (point_size - 1) // 2, j + point_size // 2 + 1):
                    if 0 <= r < H and 0 <= c < W:
                        keys[f][r][c] = max(keys[f][r][c], (v[2] << 32) | (0xFFFFFFFF - (NF + pi)))
    ids = np.array([[[-1 if key == 0 else 0xFFFFFFFF - (key & 0xFFFFFFFF) for key in row] for row in fr] for fr in keys], np.int64)
    inv = np.array([[[key >> 32 for key in row] for row in fr] for fr in keys], np.int64)
    return {"ids": ids.astype(np.int32).reshape(F, H, W), "inv_depth": inv.astype(np.int32).reshape(F, H, W), "dropped": dropped,
            "cover": cover}
