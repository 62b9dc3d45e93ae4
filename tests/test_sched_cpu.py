"""What can be said about the scheduler step without a GPU: coef_table() and the torch step() of both scheduler classes against the
float64 twin of tests/sched_reference.py on every branch (prediction type, clip, eta, the prev_t < 0 rows, DDPM's t == 0 row, 4 / 50 /
1000 inference steps), and the conditions the cases of tests/test_gpu_sched_step.py rest on: the clamp bites on part of the elements
and neither on none nor on all, and each planted mistake moves the twin by at least ten times the tolerance of the case."""
import numpy as np
import pytest
import torch

import exact16_reference as X
import sched_reference as R
from conftest import rel_err

U = R.U32
KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _configs():
    out = []
    for n_infer in (4, 50, 1000):
        for ptype in ("epsilon", "sample"):
            for clip in (False, True):
                for eta in (0.0, 0.5):
                    for one, off in ((False, 1), (True, 0)):
                        out.append(("ddim", ptype, clip, eta, one, off, n_infer))
                out.append(("ddpm", ptype, clip, 0.0, False, 0, n_infer))
    return out


CONFIGS = _configs()
# steps_offset 1 at 1000 inference steps asks for alphas_cumprod[1000]: no such entry, and the table refuses (test below)
VALID = [c for c in CONFIGS if not (c[0] == "ddim" and c[5] == 1 and c[6] == 1000)]


def _scheduler(kind, ptype, clip, one, off, n_infer):
    from seeme_amd.schedulers import DDIMScheduler, DDPMScheduler
    if kind == "ddim":
        sch = DDIMScheduler(clip_sample=clip, prediction_type=ptype, set_alpha_to_one=one, steps_offset=off, **KW)
    else:
        sch = DDPMScheduler(clip_sample=clip, prediction_type=ptype, variance_type="fixed_small", **KW)
    sch.set_timesteps(n_infer)
    return sch


def _twin_rows(sch, kind, ptype, clip, eta, one, off, n_infer, ts):
    return R.coef_rows(kind, sch.alphas_cumprod.numpy(), ts, n_infer, eta, clip, 0 if ptype == "epsilon" else 1, one, with_cancel=True)


def _id(c):
    return "-".join(str(v) for v in c)


def test_schedule_is_the_projects():
    """The twin's timesteps are those of the scheduler classes.  alphas_cumprod is defined twice in the project, by torch in
    seeme_amd/schedulers.py and by numpy in oracle/mld_oracle.py; linspace and cumprod round differently in the two, so the 1000 values
    agree to a few ulps and not to the bit.  Each is a product of at most 1000 factors that differ by at most one ulp (2 u relative)
    and takes one rounding (u) per multiplication in either library: 1000 x 4 u = 2.4e-4 relative bounds the difference, 1.3e-6 is
    measured.  The table and step() tests below therefore hand the scheduler's OWN fp32 values to the twin, which holds the formulas to
    a few u; the GPU cases, at 250-step spacing where nothing cancels, use the oracle's values and see that difference as ~1e-6."""
    for kind, off in (("ddim", 1), ("ddim", 0), ("ddpm", 0)):
        for n in (4, 50, 1000):
            sch = _scheduler(kind, "epsilon", False, False, off, n)
            assert sch.timesteps.tolist() == R.timesteps_of(kind, n, off).tolist()
    a, b = _scheduler("ddim", "epsilon", False, False, 1, 4).alphas_cumprod.double().numpy(), R.acp32().astype(np.float64)
    worst = float((np.abs(a - b) / b).max())
    print(f"alphas_cumprod, torch against numpy: worst relative difference {worst:.3e}")
    assert worst <= 1000 * 4 * U


# which of c0 .. c5 contain 1 - a_t / a_prev
_DEP = {"ddim": np.array([0, 0, 0, 1, 1, 0.0]), "ddpm": np.array([0, 0, 1, 0, 1, 0.0])}
K_TABLE = 8.0


def _table_ratio(c):
    kind, ptype, clip, eta, one, off, n_infer = c
    sch = _scheduler(kind, ptype, clip, one, off, n_infer)
    tab = sch.coef_table(eta)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (n_infer, 8)
    tab = tab.double().numpy()
    ref, cancel = _twin_rows(sch, kind, ptype, clip, eta, one, off, n_infer, sch.timesteps.tolist())
    # the flags, and every entry whose value is a constant 0 in the twin, are equal
    assert np.array_equal(tab[:, 6:], ref[:, 6:])
    const = ref[:, :6] == 0.0
    assert np.array_equal(tab[:, :6][const], ref[:, :6][const])
    bound = (K_TABLE * U + _DEP[kind][None] * (U / cancel)[:, None]) * np.abs(ref[:, :6])
    ratio = np.where(const, 0.0, np.abs(tab[:, :6] - ref[:, :6]) / np.where(const, 1.0, bound))
    return float(ratio.max()), const


@pytest.mark.parametrize("c", VALID, ids=_id)
def test_coef_table_vs_twin(c):
    """coef_table() forms 1 - a_t / a_prev in fp32: a_t / a_prev carries one rounding, u = 2^-24 relative, and the difference from 1
    keeps that absolute error, so the entries that contain it (DDIM c3 with eta > 0 and c4; DDPM c2 and c4) are off by up to
    u / (1 - a_t / a_prev) relative -- 1200 u at 1000-step spacing, where the difference is beta_t >= 0.00085.  On top of that every entry
    gets K_TABLE = 8 u: the longest chain (DDPM c2: a pow at 2 u, 1 - a_t, 1 - a_t / a_prev, a product, a quotient) is six roundings.
    Measured on the CPU, worst |table - twin| / bound over all rows and configurations: DDIM 0.13 at 4 inference steps, 0.23 at 50, 0.25
    at 1000; DDPM 0.15, 0.41, 0.49.
    Constant entries (0, 1, the flags; c4 at eta 0 and at DDPM's t == 0; c3 of the set_alpha_to_one row) must be equal."""
    ratio, const = _table_ratio(c)
    kind, _, _, eta, one, _, n_infer = c
    print(f"coef_table {_id(c)}: worst error / bound {ratio:.3f}")
    assert const[:, 5 if kind == "ddim" else 3].all()
    if kind == "ddim" and eta == 0.0:
        assert const[:, 4].all()
    if kind == "ddpm":
        assert const[-1, 4] and not const[:-1, 4].any()              # t == 0: no noise; every other row has some
    if kind == "ddim" and one:
        assert const[-1, 3]                                          # a_prev = 1: nothing left of eps
    assert ratio <= 1.0


def test_offset_past_the_schedule_is_refused():
    """DDIM with steps_offset 1 at 1000 inference steps starts at t = 1000, one past alphas_cumprod: the table raises and wraps nothing."""
    sch = _scheduler("ddim", "epsilon", False, False, 1, 1000)
    assert int(sch.timesteps[0]) == 1000
    with pytest.raises(IndexError):
        sch.coef_table(0.0)


K_STEP = 16.0


@pytest.mark.parametrize("c", VALID, ids=_id)
def test_torch_step_vs_twin(c):
    """step() of the scheduler class in fp32 against step(coef_rows(...)) at the first, middle and last timestep, with a noise tensor
    passed wherever the class takes one (DDPM's t == 0 included: it must be ignored).  Per element the bound is
    (K_STEP u + u / (1 - a_t / a_prev)) S with S the sum of the magnitudes that enter the result -- |c2| (|x| + |c1 out|) / |c0| +
    |c3 out| + |c5 x| + |c4 noise| for epsilon prediction and its mirror image for sample prediction; the clamp is 1-Lipschitz and only
    shrinks them.  K_STEP = 16: the eight roundings of the table's entries and as many in the four-term sum.
    Measured on the CPU, worst error / bound: DDIM 0.20 at 4 inference steps, 0.16 at 50, 0.08 at 1000; DDPM 0.28, 0.20, 0.20."""
    kind, ptype, clip, eta, one, off, n_infer = c
    sch = _scheduler(kind, ptype, clip, one, off, n_infer)
    ts = sch.timesteps.tolist()
    rows, cancel = _twin_rows(sch, kind, ptype, clip, eta, one, off, n_infer, ts)
    rng = np.random.default_rng(n_infer + 7)
    x, m, nz = (rng.standard_normal((3, 1, 256)).astype(np.float32) for _ in range(3))
    worst = 0.0
    for i in (0, len(ts) // 2, len(ts) - 1):
        xt, mt, nt = torch.from_numpy(x), torch.from_numpy(m), torch.from_numpy(nz)
        if kind == "ddim":
            got = sch.step(mt, ts[i], xt, eta=eta, variance_noise=nt if eta > 0 else None).prev_sample
        else:
            got = sch.step(mt, ts[i], xt, variance_noise=nt).prev_sample
        assert got.dtype == torch.float32
        has_noise = (kind == "ddpm") or eta > 0
        ref = R.step(rows[i], x, m, nz if has_noise else None)
        c0, c1, c2, c3, c4, c5 = np.abs(rows[i, :6])
        ax, am = np.abs(x.astype(np.float64)), np.abs(m.astype(np.float64))
        if ptype == "epsilon":
            S = c2 * (ax + c1 * am) / c0 + c3 * am + c5 * ax
        else:
            S = c2 * am + c3 * (ax + c0 * am) / c1 + c5 * ax
        if has_noise:
            S = S + c4 * np.abs(nz.astype(np.float64))
        bound = (K_STEP * U + U / cancel[i]) * S
        worst = max(worst, float((np.abs(got.double().numpy() - ref) / bound).max()))
        if kind == "ddpm" and ts[i] == 0:
            assert np.array_equal(ref, R.step(rows[i], x, m, None))            # the twin's own t == 0 row ignores the noise
    print(f"step() {_id(c)}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_coef_key_separates_what_coef_table_reads():
    """MldDenoiser.sample_loop caches the device copy of coef_table() under coef_key(): two schedulers whose tables differ must not
    share a key, and two that are configured alike must."""
    def key(kind="ddim", ptype="epsilon", clip=False, one=False, n=4, **kw):
        from seeme_amd.schedulers import DDIMScheduler, DDPMScheduler
        k = dict(KW, **kw)
        sch = (DDIMScheduler(clip_sample=clip, prediction_type=ptype, set_alpha_to_one=one, steps_offset=0, **k) if kind == "ddim"
               else DDPMScheduler(clip_sample=clip, prediction_type=ptype, **k))
        sch.set_timesteps(n)
        return sch.coef_key(), sch.coef_table(0.0)
    base = key()
    assert key()[0] == base[0] and torch.equal(key()[1], base[1])
    for other in (key(clip=True), key(ptype="sample"), key(one=True), key(kind="ddpm"), key(beta_schedule="linear"), key(beta_end=0.02),
                  key(beta_start=0.0001), key(num_train_timesteps=500)):
        assert other[0] != base[0]
        assert other[1].shape != base[1].shape or not torch.equal(other[1], base[1])
    # same timesteps, another spacing: the existing suite truncates a 1000-step schedule
    from seeme_amd.schedulers import DDPMScheduler
    a, b = DDPMScheduler(**KW), DDPMScheduler(**KW)
    a.set_timesteps(1000)
    b.set_timesteps(4)
    assert a.coef_key() != b.coef_key()


# ----------------------------------------------------------------------------- the conditions the GPU cases rest on
_P = {}


def _params(dtype):
    if dtype not in _P:
        _P[dtype] = X.oracle_params(X.structured_denoiser(dtype))
    return _P[dtype]


def _representatives():
    seen = {}
    for name in R.BODIES:
        seen.setdefault(R.input_key(name), name)
    return list(seen.values())


def test_tolerances_are_the_projects():
    import test_gpu_exact16 as E
    assert (R.TOL_F32, R.TOL_LOOP) == (E.TOL_F32, E.TOL_LOOP) == (1e-4, 5e-4)
    for row in R.probe_rows([(0, 0), (0, 1), (0, 0)]):
        assert len(set(np.abs(row[:6]))) == 6 and (row[:6] != 0).all() and R.gain(row) <= 2.0
    assert all(len(set(R.PROBE_ROWS[:, j])) == 3 for j in range(6))            # every slot changes from step to step
    for body in R.BODIES:
        for case in R.one_step_cases(body):
            assert case["tol"] == R.TOL_F32 * max(1.0, R.gain(case["rows"][0])) and case["tol"] <= 2 * R.TOL_F32


@pytest.mark.parametrize("body", _representatives())
def test_gpu_case_conditions(body):
    """For the exact inputs of every case of test_gpu_sched_step.py (one body per distinct (model, B, N, guidance): the others share
    its inputs), on the float64 twin alone:
    - at every step whose row clamps, between 10 % and 90 % of the elements have an unclamped x0 outside [-1, 1];
    - a twin with one planted mistake ends at least 10 tolerances from the true one, for every mistake that applies to the case;
    - the 1e30 in the noise row of DDPM's t == 0 leaves no trace.
    Measured for the committed inputs: clamped shares between 0.18 and 0.74, the smallest margin 609 tolerances (c3 and c5 exchanged
    in the DDPM chain, where c3 is 0 and c5 small at the first steps)."""
    P = _params(R.BODIES[body]["dtype"])
    for case in R.one_step_cases(body) + R.chain_cases(body):
        true, x0s = R.twin_final(P, body, case, with_x0=True)
        assert true.dtype == np.float64 and np.isfinite(true).all()
        shares = [float((np.abs(x0) > 1.0).mean()) for x0, row in zip(x0s, case["rows"]) if row[6] != 0]
        margins = {m: rel_err(R.twin_final(P, body, case, mistake=m), true) / case["tol"] for m in R.mistakes_of(body, case)}
        print(f"{body} | {case['name']}: clamped share {[round(s, 3) for s in shares]}, margins / tol "
              + ", ".join(f"{m} {v:.3g}" for m, v in margins.items()))
        assert all(0.1 <= s <= 0.9 for s in shares), (case["name"], shares)
        assert all(v >= 10.0 for v in margins.values()), (case["name"], margins)
        if "rows_noise_at_t0" in case:
            assert case["noise"][3].min() == np.float32(1e30) and "noise_at_t0" in margins
            zeroed = dict(case, noise=np.concatenate([case["noise"][:3], np.zeros_like(case["noise"][:1])]))
            assert np.array_equal(R.twin_final(P, body, zeroed), true)
