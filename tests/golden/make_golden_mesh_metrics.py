#!/usr/bin/env python3
"""Generate pa_mpjpe.npz from the REFERENCE's own Procrustes error (EgoHMR/utils/pose_utils.py, imported by path):
``reconstruction_error(pred, ref, avg_joint=False)`` in float64 on 64 joint pairs.

Runs only where the reference tree exists (SEEME_REFERENCE, default /root/reference); nothing of it is copied.  Each prediction is
a rotated, scaled, translated and noised copy of its reference (24 joints of a body-sized anisotropic cloud); pairs 8..15 are
mirrored as well, so the reflection branch of compute_similarity_transform runs; pair 63 has pred == ref.

The generator asserts that an fp32 restatement of the same steps agrees with the float64 result to 1e-5 relative: the cases are
well conditioned, so an fp32 kernel can be held to the project's fp32 bound on them.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_mesh_metrics.py
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SEEME_REFERENCE", "/root/reference")
N, NJ, MIRRORED, SAME = 64, 24, range(8, 16), 63


def cases(seed=20):
    rng = np.random.Generator(np.random.PCG64(seed))
    ref = rng.standard_normal((N, NJ, 3)) * np.array([0.25, 0.6, 0.15]) + rng.uniform(-2.0, 2.0, (N, 1, 3))
    pred = np.empty_like(ref)
    for i in range(N):
        q = rng.standard_normal(4)
        w, x, y, z = q / np.linalg.norm(q)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        body = ref[i] - ref[i].mean(axis=0)
        if i in MIRRORED:
            body = body * np.array([-1.0, 1.0, 1.0])
        pred[i] = rng.uniform(0.7, 1.4) * body @ R.T + rng.uniform(-2.0, 2.0, 3) + rng.standard_normal((NJ, 3)) * 0.03
    pred[SAME] = ref[SAME]
    return pred, ref


def restated(S1, S2, dt):
    """The steps of compute_similarity_transform in dtype dt; per-joint error [J]."""
    S1, S2 = S1.astype(dt).T, S2.astype(dt).T
    mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    K = X1 @ X2.T
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(3, dtype=dt)
    Z[2, 2] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.T @ Z @ U.T
    s = np.trace(R @ K) / (X1 ** 2).sum()
    hat = s * (R @ S1) + (mu2 - s * (R @ mu1))
    return np.sqrt(((hat - S2) ** 2).sum(axis=0))


def main():
    spec = importlib.util.spec_from_file_location("ref_pose_utils", os.path.join(REF, "EgoHMR", "utils", "pose_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pred, ref = cases()
    # the fixture stores fp32-representable inputs, so that a device test feeds the kernel exactly what the reference saw
    pred, ref = pred.astype(np.float32).astype(np.float64), ref.astype(np.float32).astype(np.float64)
    per_joint = mod.reconstruction_error(pred, ref, avg_joint=False)              # [N, J] float64
    assert per_joint.shape == (N, NJ) and per_joint.dtype == np.float64
    err = per_joint.mean(axis=-1)
    live = np.arange(N) != SAME
    e32 = np.stack([restated(pred[i], ref[i], np.float32) for i in range(N)]).mean(axis=-1)
    e64 = np.stack([restated(pred[i], ref[i], np.float64) for i in range(N)]).mean(axis=-1)
    rel32 = float((np.abs(e32 - err)[live] / err[live]).max())
    rel64 = float((np.abs(e64 - err)[live] / err[live]).max())
    print(f"fp32 restatement vs reference: {rel32:.3e}; float64 restatement: {rel64:.3e}; pred == ref row: {err[SAME]:.3e} m")
    assert rel32 <= 1e-5 and rel64 <= 1e-12 and err[SAME] <= 1e-9
    # mirrored rows really take the reflection branch: det(U V^T) < 0 for them and only for them
    for i in range(N):
        X1, X2 = (pred[i] - pred[i].mean(0)).T, (ref[i] - ref[i].mean(0)).T
        U, _, Vh = np.linalg.svd(X1 @ X2.T)
        if i != SAME:
            assert (np.linalg.det(U @ Vh) < 0) == (i in MIRRORED), i
    print("error range (m):", float(err[live].min()), float(err[live].max()))
    path = os.path.join(HERE, "pa_mpjpe.npz")
    np.savez_compressed(path, pred=pred.astype(np.float32), ref=ref.astype(np.float32), per_joint=per_joint, err=err,
                        mirrored=np.array(list(MIRRORED), np.int64), same=np.int64(SAME))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
