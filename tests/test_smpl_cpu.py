"""The yardsticks of tests/test_gpu_smpl.py, checked on the host: lbs64 against the oracle's lbs (two independent restatements, in
float64), the autograd twin against lbs64, the float64 chain rule through drodrigues against float64 autograd on every frame of
every input maker, the conditioning of those inputs, the float32 cancellation of 1 - cos(theta) in d Rodrigues / d axis-angle (and
its absence with 2 sin^2(theta / 2)), and that no float32-reference error the GPU bounds are built from is zero."""
import numpy as np
import pytest
import torch

import smpl_reference as SR
from oracle import mld_oracle as O
from seeme_amd.smpl import SMPL, synthetic_model_arrays


@pytest.fixture(scope="module")
def arrays():
    return synthetic_model_arrays(1234)


@pytest.fixture(scope="module")
def smpl64():
    return SMPL.synthetic(1234).double()


@pytest.fixture(scope="module")
def smpl32():
    return SMPL.synthetic(1234)


def _makers():
    """Every frame of every maker, labelled."""
    pose = np.concatenate([SR.ordinary(5, 5), SR.small_angle(), SR.wide_angle(), SR.zero_frame(), SR.padded_frame()])
    names = ["ordinary"] * 5 + [f"small {m:g}" for m in SR.SMALL_MAGS] + [f"wide {m:.4f}" for m in SR.WIDE_MAGS] + ["zero", "padded"]
    return pose, names


def test_lbs64_equals_the_oracle_in_float64(arrays):
    """V = 6890, M = 3, axis-angle and rotation-matrix input: joints, extra joints and vertices within 1e-12 per frame."""
    M = 3
    pose = SR.ordinary(M, 3).astype(np.float64)
    betas, tr, _ = (x.astype(np.float64) for x in SR.betas_transl_weights(M, 3))
    oracle_model = O.make_synthetic_smpl(1234)
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"):
        assert np.array_equal(oracle_model[k], arrays[k]), k
    for rotmat in (False, True):
        if rotmat:
            R = SR.rodrigues(pose.reshape(-1, 3)).reshape(M, 24, 3, 3)
            jo, vo = O.smpl_lbs(oracle_model, betas, R[:, :1], R[:, 1:], tr, pose2rot=False)
            got = SR.lbs64(arrays, betas, R, tr, True)
        else:
            jo, vo = O.smpl_lbs(oracle_model, betas, pose[:, :3], pose[:, 3:], tr)
            got = SR.lbs64(arrays, betas, pose, tr, False)
        assert jo.dtype == np.float64 and got["vertices"].dtype == np.float64
        for name, a, b in (("joints", got["joints"], jo[:, :24]), ("extra", got["extra"], jo[:, 24:]), ("vertices", got["vertices"], vo)):
            e = SR.frame_err(a, b)
            print(f"lbs64 vs oracle, rotmat={rotmat}, {name}: per frame {np.array2string(e, precision=2)}")
            assert e.shape == (M,) and (e < 1e-12).all(), (name, e)
    assert np.array_equal(got["feat"][:, 217:], np.zeros((M, 7))) and got["A"].shape == (M, 24, 12)


def test_lbs64_takes_any_vertex_count():
    """V = 64: the extra joints are the vertices SMPL_EXTRA_VERTEX_IDS[i] % V, as seeme_amd.smpl.SMPL picks them."""
    from seeme_amd.smpl import SMPL_EXTRA_VERTEX_IDS
    arr = synthetic_model_arrays(1234, 64)
    betas, tr, _ = SR.betas_transl_weights(2, 1)
    out = SR.lbs64(arr, betas.astype(np.float64), SR.ordinary(2, 1).astype(np.float64), tr.astype(np.float64), False)
    assert out["vertices"].shape == (2, 64, 3) and out["extra"].shape == (2, 21, 3)
    assert np.array_equal(out["extra"], out["vertices"][:, [i % 64 for i in SMPL_EXTRA_VERTEX_IDS]])
    assert SMPL.synthetic(1234, 64).vertex_joint_selector.extra_joints_idxs.tolist() == [i % 64 for i in SMPL_EXTRA_VERTEX_IDS]


def test_twin_joints_equal_lbs64_in_float64(arrays, smpl64):
    pose, _ = _makers()
    M = pose.shape[0]
    betas, tr, wgt = SR.betas_transl_weights(M, 9)
    j, _, _ = SR.twin_grads(smpl64, betas, pose, tr, wgt)
    ref = SR.lbs64(arrays, betas.astype(np.float64), pose.astype(np.float64), tr.astype(np.float64), False)["joints"]
    e = SR.frame_err(j, ref)
    print(f"float64 twin joints vs lbs64: worst frame {e.max():.3e}")
    assert j.dtype == np.float64 and (e < 1e-12).all(), e


@pytest.mark.parametrize("c1_form", ["one_minus_cos", "half_angle"])
def test_float64_chain_rule_equals_float64_autograd_on_every_frame(arrays, smpl64, c1_form):
    """d pose and d transl of sum(joints * w): autograd through the float64 twin against the tree walk + drodrigues in float64, per
    frame within 1e-8, with either form of 1 - cos (in float64 the cancellation costs 1e-16 / theta <= 1e-10 at theta = 1e-6)."""
    pose, names = _makers()
    M = pose.shape[0]
    betas, tr, wgt = SR.betas_transl_weights(M, 9)
    _, dp_ref, dt_ref = SR.twin_grads(smpl64, betas, pose, tr, wgt)
    dp, dtr = SR.joints_backward(arrays, betas, pose, wgt, np.float64, c1_form)
    ep, et = SR.frame_err(dp, dp_ref), SR.frame_err(dtr, dt_ref)
    for n, a, b in zip(names, ep, et):
        print(f"float64 chain rule ({c1_form}) vs autograd, {n}: d pose {a:.3e}, d transl {b:.3e}")
    assert (ep < 1e-8).all() and (et < 1e-8).all(), (ep, et)


def test_inputs_are_what_they_claim():
    """small_angle: every joint's float32 angle within 1 % of its nominal magnitude (wide_angle too); ordinary: no joint below 1e-2 or
    above 4, for every (M, seed) the GPU tests draw; the zero and padded frames have their zeros; float32 throughout."""
    ang = lambda p: np.linalg.norm(p.astype(np.float64).reshape(-1, 24, 3), axis=2)
    for maker, mags in ((SR.small_angle(), SR.SMALL_MAGS), (SR.wide_angle(), SR.WIDE_MAGS)):
        assert maker.dtype == np.float32 and maker.shape == (len(mags), 72)
        a = ang(maker)
        for row, m in zip(a, mags):
            assert (np.abs(row / m - 1) < 0.01).all(), (m, row)
    cases = [(M, M) for M in (1, 3, 4, 5, 8, 9)] + [(SR.N_ORDINARY_IN_EDGE_BATCH, 3000), (5, 5)]
    for M, seed in cases:
        p = SR.ordinary(M, seed)
        assert p.dtype == np.float32 and p.shape == (M, 72)
        a = ang(p)
        assert a.min() >= 1e-2 and a.max() <= 4, (M, seed, a.min(), a.max())
    z, pad = SR.zero_frame(), SR.padded_frame()
    assert z.shape == (1, 72) and not z.any()
    assert not pad[:, 66:].any() and 1e-2 <= ang(pad)[:, :22].min() and ang(pad)[:, :22].max() <= 4
    for kind, M in (("small", 11), ("wide", 9)):
        pose, names = SR.edge_batch(kind)
        assert pose.shape == (M, 72) and len(names) == M and M <= 12 and names[:3] == ["ordinary"] * 3


TABLE_ANGLES = (0.0, 1e-6, 1e-5, 1e-4, 2.4e-4, 1e-3, 1e-2, 0.5, 3.1, 4.0)


def _joint_errors(angle, form, n=2048, seed=0):
    """Per-joint relative error (max over the three outputs / their largest) of the float32 drodrigues against float64, n random axes
    at one angle (angle None: ordinary N(0, 0.5) vectors), unit-normal dL/dR."""
    rng = np.random.default_rng(seed)
    aa = SR._f32(SR._axes(n, rng) * angle) if angle is not None else SR._f32(0.5 * rng.standard_normal((n, 3)))
    g = SR._f32(rng.standard_normal((n, 3, 3)))
    ref = SR.drodrigues(aa, g, np.float64, "half_angle")
    return SR.frame_err(SR.drodrigues(aa, g, np.float32, form), ref)


def test_cancellation_of_one_minus_cos_in_float32():
    """The closed form in float32 against itself in float64, per joint: with 1 - cos(theta) the error passes 1e-4 inside the band
    1e-6..1e-2; with 2 sin^2(theta / 2) every angle of the band stays within 4x the form's own largest error on ordinary joints.
    In float64 the two forms are the same function."""
    worst = {}
    print("angle        1 - cos        2 sin^2(th/2)")
    for a in TABLE_ANGLES:
        worst[a] = tuple(float(_joint_errors(a, form).max()) for form in ("one_minus_cos", "half_angle"))
        print(f"{a:<10g}   {worst[a][0]:.3e}      {worst[a][1]:.3e}")
    ordinary = tuple(float(_joint_errors(None, form).max()) for form in ("one_minus_cos", "half_angle"))
    print(f"ordinary     {ordinary[0]:.3e}      {ordinary[1]:.3e}")
    band = [a for a in TABLE_ANGLES if 1e-6 <= a <= 1e-2]
    assert max(worst[a][0] for a in band) > 1e-4
    assert all(worst[a][1] <= 4 * ordinary[1] for a in band), (worst, ordinary)
    rng = np.random.default_rng(1)
    aa, g = SR.small_angle().reshape(-1, 3), rng.standard_normal((144, 3, 3))
    same = SR.frame_err(SR.drodrigues(aa, g, np.float64, "one_minus_cos"), SR.drodrigues(aa, g, np.float64, "half_angle"))
    assert (same < 1e-9).all(), same


@pytest.mark.parametrize("kind", ["small", "wide"])
def test_the_gpu_edge_bound_separates_the_two_forms_on_the_host(arrays, smpl32, smpl64, kind):
    """The bound of test_gpu_smpl's angle-edge backward case, applied to the float32 restatement of the kernel: every frame at most
    4x the float32 twin's largest error on the batch's ordinary frames.  The half-angle form passes on every frame of both batches;
    the 1 - cos form fails on a small-angle frame (and passes the wide batch, which has none)."""
    pose, names = SR.edge_batch(kind)
    betas, tr, wgt = SR.betas_transl_weights(pose.shape[0], 0)
    _, ref, _ = SR.twin_grads(smpl64, betas, pose, tr, wgt)
    _, tw, _ = SR.twin_grads(smpl32, betas, pose, tr, wgt)
    bound = 4 * SR.frame_err(tw, ref)[:SR.N_ORDINARY_IN_EDGE_BATCH].max()
    errs = {form: SR.frame_err(SR.joints_backward(arrays, betas, pose, wgt, np.float32, form)[0], ref) for form in ("one_minus_cos", "half_angle")}
    for i, n in enumerate(names):
        print(f"{kind} batch, {n}: 1 - cos {errs['one_minus_cos'][i]:.3e}, half angle {errs['half_angle'][i]:.3e}, bound {bound:.3e}")
    assert (errs["half_angle"] <= bound).all()
    assert (errs["one_minus_cos"] > bound).any() == (kind == "small")


def test_float32_reference_errors_are_not_zero(arrays, smpl32, smpl64):
    """Every figure a GPU bound multiplies by 4 is > 0: the largest per-frame error of the float32 run of lbs64 in each forward group,
    and of autograd through the float32 twin in d pose and d transl (M = 1 and the ordinary frames of both edge batches)."""
    for V in (64, 257):
        arr = synthetic_model_arrays(1234, V)
        pose = SR.ordinary(5, 5)
        betas, tr, _ = SR.betas_transl_weights(5, 5)
        ref = SR.lbs64(arr, betas.astype(np.float64), pose.astype(np.float64), None, False)
        f32 = SR.lbs64(arr, betas, pose, None, False)
        for k in ("joints", "extra", "vertices", "A", "feat"):
            e = SR.frame_err(f32[k], ref[k])
            print(f"V={V} float32 lbs64 {k}: largest per-frame error {e.max():.3e}")
            assert f32[k].dtype == np.float32 and e.max() > 0, k
    cases = [("M=1", SR.ordinary(1, 1))] + [(kind, SR.edge_batch(kind)[0][:SR.N_ORDINARY_IN_EDGE_BATCH]) for kind in ("small", "wide")]
    for name, pose in cases:
        betas, tr, wgt = SR.betas_transl_weights(pose.shape[0], 1)
        _, dp64, dt64 = SR.twin_grads(smpl64, betas, pose, tr, wgt)
        _, dp32, dt32 = SR.twin_grads(smpl32, betas, pose, tr, wgt)
        ep, et = SR.frame_err(dp32, dp64), SR.frame_err(dt32, dt64)
        print(f"{name} float32 twin: d pose {ep.max():.3e}, d transl {et.max():.3e}")
        assert dp32.dtype == np.float32 and ep.max() > 0 and et.max() > 0


def test_float32_twin_shares_the_cancellation(smpl32, smpl64):
    """Why the small-angle frames are not held to the twin's error on themselves: autograd through the float32 twin (smplx's 1 - cos)
    is an order of magnitude or more worse on a frame whose angles are all 1e-4 than on ordinary frames."""
    pose, names = SR.edge_batch("small")
    betas, tr, wgt = SR.betas_transl_weights(pose.shape[0], 0)
    _, dp64, _ = SR.twin_grads(smpl64, betas, pose, tr, wgt)
    _, dp32, _ = SR.twin_grads(smpl32, betas, pose, tr, wgt)
    e = SR.frame_err(dp32, dp64)
    for n, v in zip(names, e):
        print(f"float32 twin d pose, {n}: {v:.3e}")
    assert e[names.index("small 0.0001")] > 10 * e[:SR.N_ORDINARY_IN_EDGE_BATCH].max()
