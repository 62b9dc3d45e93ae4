"""The scheduler step that closes every step of the sampling kernels -- k_den_sample (den_kernels.hip), k_den_cluster in its
two-wave-group and its eight-wave spelling (den_cluster.inc.hip), k_den_cluster_ms (den_cluster_ms.inc.hip) -- against the float64 twin
of tests/sched_reference.py on EVERY branch of the coefficient row: sample prediction (c7), the clamp (c6), DDPM's weight on the
current sample (c5) away from 1000-step spacing, step noise (c4) with and without a noise pointer, the DDIM prev_t < 0 row and DDPM's
t == 0 row with 1e30 in the noise it must not use.  The rest of the GPU suite runs epsilon prediction without the clamp only.

The model is the exact-16-bit one of tests/exact16_reference.py, so the project's fp32 bounds apply to every weight image: TOL_F32 for
one step, times the gain of the row where that exceeds 1, and TOL_LOOP for a chain (both from test_gpu_exact16.py).  tests/test_sched_cpu.py
checks on the twin alone that the clamp bites on 10 to 90 % of the elements in every clamped step of these inputs and that a planted
mistake (clamp skipped or on eps, prediction type ignored, c3 and c5 exchanged, a neighbour's noise row, noise at t == 0) moves the
result by at least ten tolerances.  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import sched_reference as R
from conftest import elem_err, rel_err
from test_gpu_exact16 import TOL_F32, TOL_LOOP, _cus, _den, _model

pytestmark = pytest.mark.gpu

assert (TOL_F32, TOL_LOOP) == (R.TOL_F32, R.TOL_LOOP)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


_TWIN = {}


def _twin(body, case):
    """The twin's final latent of a case, computed once per (inputs, case) and shared by the bodies with the same inputs."""
    key = (R.input_key(body), case["name"])
    if key not in _TWIN:
        ref = R.twin_final(_model(R.BODIES[body]["dtype"])[1], body, case)
        assert ref.dtype == np.float64
        ref.setflags(write=False)
        _TWIN[key] = ref
    return _TWIN[key]


def _select(body, dev, monkeypatch, wd=None):
    """The module of a body under its launch switches; the plan it resolves to is the body's."""
    b = R.BODIES[body]
    monkeypatch.delenv("SEEME_DEN_CLUSTER", raising=False)
    monkeypatch.delenv("SEEME_DEN_CLUSTER_MS_PLAN", raising=False)
    if b["plan"]:
        monkeypatch.setenv("SEEME_DEN_CLUSTER_MS_PLAN", b["plan"])
    wd = wd or b["wd"]
    den = _den(dev, b["dtype"], wd, cluster=b["cluster"], ms=True)
    if wd == b["wd"]:
        assert den._cluster_plan(b["B"], b["N"], b["gs"] > 1.0, False, _cus(dev)) == b["expect"], "the switches did not select the body"
    return den


def _launch(den, body, case, dev):
    """sample_loop of a case on the inputs of its body: [B, 256]."""
    b = R.BODIES[body]
    lat, cond, _ = R.inputs(body)
    noise = None if case["noise"] is None else torch.from_numpy(case["noise"]).to(dev)
    out = den.sample_loop(torch.from_numpy(lat).to(dev), torch.from_numpy(cond).to(dev), R.make_scheduler(case), eta=case["eta"],
                          guidance_scale=b["gs"], step_noise=noise)
    if b["expect"][0]:
        assert den.cluster_status()[0] == 0, "a cluster gave up waiting for a peer"
    assert tuple(out.shape) == (1, b["B"], 256)
    return out[0].cpu().numpy()


def _check(body, cases, dev, monkeypatch):
    den = _select(body, dev, monkeypatch)
    sel = R.twin_rows(body)
    for case in cases:
        out = _launch(den, body, case, dev)
        ref = _twin(body, case)
        err, el = rel_err(out[sel], ref), elem_err(out[sel], ref)
        print(f"sched {body} | {case['name']}: rel err {err:.3e} (elem {el:.3e}), bound {case['tol']:.3g}")
        assert np.isfinite(out).all()
        assert err < case["tol"], (body, case["name"], err)


BODY_IDS = [b for b in R.BODIES if b != "sample_pairs"]


@pytest.mark.parametrize("body", BODY_IDS)
def test_one_step_every_branch(dev, monkeypatch, body):
    """Probe rows, one step: prediction type x clamp x (noise pointer set | null), each at TOL_F32 max(1, gain(row)).  The bodies:
    k_den_sample with the fp32, fp16 and bf16 image (B = 3) and as a guidance pair (7.5, B = 2, condition 2 B: sample prediction and
    the clamp under guidance); k_den_cluster C = 8 on the fp16 image -- two wave groups, coefficients and noise row through LDS -- at
    B = 2 with one and two condition tokens and at B = 9 (ragged); C = 4 and C = 2, the eight-wave body with scalar-loaded
    coefficients; k_den_cluster_ms under the forced plans "8,2" and "4,2" at B = 3 (an odd sample in the last cluster), "4,2" also on the
    bf16 image.  As everywhere in the suite, placement and launch form change speed and never results: every body is held to the one
    twin of its inputs.  Measured on an MI355X: the worst case of any body is 1.3e-5 against a bound of 1.4e-4 (k_den_cluster_ms, sample
    prediction with the clamp)."""
    _check(body, R.one_step_cases(body), dev, monkeypatch)


@pytest.mark.parametrize("body", BODY_IDS)
def test_chains_every_branch(dev, monkeypatch, body):
    """At TOL_LOOP, the final latent (which every intermediate one implies) of: probe rows over 3 steps with other values and other
    flags at every step and given step noise [3, B, 256]; DDIM with sample prediction, the clamp and eta 0.5 over the 4-step schedule
    (t = 751 .. 1, the last row with prev_t < 0); DDIM with epsilon prediction and the clamp over four steps of the 50-step schedule;
    DDPM at set_timesteps(4) (t = 750, 500, 250, 0: c5 away from 1000-step spacing) with sample prediction, the clamp and 1e30 in the
    noise row of t == 0.  Measured on an MI355X: at most 5.5e-5 (the guidance pair on the DDPM chain), 1.5e-5 without guidance."""
    _check(body, R.chain_cases(body), dev, monkeypatch)


def test_sample_pairs_every_branch(dev, monkeypatch):
    """k_den_sample with two independent samples per workgroup: B = SEEME_DEN_PAIR_ABOVE + 1 = 257, odd, so the last workgroup holds one
    sample.  Samples 0, 1, 255 and 256 (first pair, last pair's neighbour, the lone one) against the twin, every other sample against the
    fp32-image run of the same call at 2 TOL: both runs are held to TOL of the truth, so that is what the triangle inequality leaves."""
    body = "sample_pairs"
    den16, sel = _select(body, dev, monkeypatch), R.twin_rows(body)
    assert R.BODIES[body]["B"] == 257 and list(sel) == [0, 1, 255, 256]
    for case in R.one_step_cases(body) + R.chain_cases(body):
        out = _launch(den16, body, case, dev)
        o32 = _launch(_select(body, dev, monkeypatch, wd="fp32"), body, case, dev)
        ref = _twin(body, case)
        err, e32 = rel_err(out[sel], ref), rel_err(o32[sel], ref)
        rest = max(rel_err(out[i], o32[i]) for i in range(257))
        print(f"sched {body} | {case['name']}: rel err {err:.3e}, fp32 image {e32:.3e}, worst sample fp16 against fp32 image {rest:.3e}, "
              f"bound {case['tol']:.3g}")
        assert np.isfinite(out).all()
        assert err < case["tol"] and e32 < case["tol"] and rest < 2 * case["tol"], (case["name"], err, e32, rest)


def test_wave_group_body_against_eight_wave_body(dev, monkeypatch):
    """test_gpu_cluster_groups.py asserts that the two-wave-group body of k_den_cluster (C = 8, fp16 image: coefficients and noise row
    from LDS) gives the bits of the eight-wave body (k_den_cluster_ms forced to "8,2": scalar-loaded coefficients) -- on the epsilon /
    no-clamp branch.  Here the same pair runs every case at B = 2: sample prediction, the clamp, c5 != 0 and the noise term included.
    Both bodies close the step with the one sched_step of csrc/den_sched.hpp, whose sums are spelled out and not left to the compiler,
    and what they feed it is bit-identical by test_gpu_cluster_groups.py: so the bits must agree in all twelve cases, next to the
    float64 bound for each of the two."""
    body = "cluster8_B2"
    b = R.BODIES[body]
    for case in R.one_step_cases(body) + R.chain_cases(body):
        grp = _launch(_select(body, dev, monkeypatch), body, case, dev)
        monkeypatch.setenv("SEEME_DEN_CLUSTER_MS_PLAN", "8,2")
        den = _den(dev, b["dtype"], b["wd"], cluster="auto", ms=True)
        assert den._cluster_plan(b["B"], 1, False, False, _cus(dev)) == (8, 2)
        ms = _launch(den, body, case, dev)
        monkeypatch.delenv("SEEME_DEN_CLUSTER_MS_PLAN")
        ref = _twin(body, case)
        eg, em = rel_err(grp, ref), rel_err(ms, ref)
        print(f"sched pair | {case['name']}: bits agree {np.array_equal(grp, ms)}, max |grp - ms| {float(np.abs(grp - ms).max()):.3e}, "
              f"rel err two wave groups {eg:.3e}, eight waves {em:.3e}, bound {case['tol']:.3g}")
        assert eg < case["tol"] and em < case["tol"], (case["name"], eg, em)
        assert np.array_equal(grp, ms), case["name"]


@pytest.mark.parametrize("body", ["sample_fp32", "cluster8_B2", "cluster4_B2"])
def test_one_denoiser_three_schedulers(dev, monkeypatch, body):
    """ONE denoiser object, three sample_loop calls whose scheduler class, timesteps and eta are the same: clamp off, clamp on, sample
    prediction.  The module caches the device copy of the coefficient table; keyed on (timesteps, eta, class name) alone, as it was, the
    second and third call ran with the first call's coefficients.  Each result must match its own twin.  Measured on an MI355X: with
    the old key the second call is off by 17 to 19 times the largest latent; with coef_key() in the key the three calls are at 1.6e-6,
    4.3e-5 and 2.2e-6 (k_den_sample, fp32 image)."""
    den = _select(body, dev, monkeypatch)
    ts, acp = R.timesteps_of("ddim", 4, 1), R.acp32()
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False, steps_offset=1)
    for name, clip, ptype in (("clip off", False, "epsilon"), ("clip on", True, "epsilon"), ("sample prediction", True, "sample")):
        case = R._case(f"cache: DDIM 4 steps, {name}", "ddim", R.coef_rows("ddim", acp, ts, 4, 0.0, clip, int(ptype == "sample")), ts, 0.0, None,
                       TOL_LOOP, sched_kw=dict(kw, clip_sample=clip, prediction_type=ptype), n_infer=4)
        out = _launch(den, body, case, dev)
        err = rel_err(out, _twin(body, case))
        print(f"sched {body} | {case['name']}: rel err {err:.3e}, bound {TOL_LOOP:g}")
        assert err < TOL_LOOP, (name, err)


def test_mld_sample_prediction_end_to_end(dev):
    """An MLD from config_mld_egobody.yaml with TRAIN.ABLATION.PREDICT_EPSILON false, B = 2, 4 inference steps: the scheduler it builds
    predicts the sample, its reverse pass is denoiser.sample_loop with that scheduler bit for bit, and both equal the float64 chain on
    the module's own parameters (fp32 weight image, recipe weights) at TOL_LOOP.  Measured on an MI355X: 8.4e-7."""
    import exact16_reference as X
    from test_gpu_flows import _mld

    def mut(cfg):
        cfg.TRAIN.ABLATION.PREDICT_EPSILON = False
        cfg.model.scheduler.num_inference_timesteps = 4
    model, dm, cfg = _mld(dev, "config_mld_egobody.yaml", mutate=mut)
    model.eval()
    sch = model.scheduler
    assert sch.config.prediction_type == "sample" and model.noise_scheduler.config.prediction_type == "sample"
    assert type(sch).__name__ == "DDIMScheduler" and not model.do_classifier_free_guidance
    rng = np.random.default_rng(77)
    lat, cond = (rng.standard_normal((2, 1, 256)).astype(np.float32) for _ in range(2))
    lt, ct = torch.from_numpy(lat).to(dev), torch.from_numpy(cond).to(dev)
    z = model._diffusion_reverse(ct, latents=lt)
    ts = sch.timesteps.tolist()
    assert ts == R.timesteps_of("ddim", 4, sch.config.steps_offset).tolist()
    z2 = model.denoiser.sample_loop(lt * sch.init_noise_sigma, ct, sch, eta=cfg.model.scheduler.eta)
    assert torch.equal(z, z2)
    rows = R.coef_rows("ddim", R.acp32(), ts, 4, cfg.model.scheduler.eta, bool(sch.config.clip_sample), 1, bool(sch.config.set_alpha_to_one))
    assert (rows[:, 7] == 1).all()
    ref = R.chain(X.oracle_params(model.denoiser), cond, lat, rows, ts)[-1][:, 0]
    assert ref.dtype == np.float64
    err = rel_err(z[0].cpu().numpy(), ref)
    print(f"sched MLD sample prediction, 4 DDIM steps: rel err {err:.3e}, bound {TOL_LOOP:g}")
    assert err < TOL_LOOP, err
