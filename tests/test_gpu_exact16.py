"""The 16-bit denoiser kernels (k_den_sample, k_den_cluster, k_den_cluster_ms with an fp16 / bf16 weight image) against the float64
oracle at the project's fp32 tolerance.  The model is the exact-16-bit one of tests/exact16_reference.py: every matrix the packers
round is representable in the 16-bit type, so the weight image is exact and what is left is fp32-level arithmetic (operand split of
22 to 24 bits, fp32 accumulation).  Every case also runs a weight_dtype="fp32" module on the same parameters and prints both errors.
Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import exact16_reference as X
from conftest import elem_err, rel_err
from oracle import mld_oracle as O

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-4       # one forward: the fp32 parity gate (tests/test_gpu_parity.py)
TOL_LOOP = 5e-4      # chained steps: the fp32 row of test_sampling_kernel_variants


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


_MODELS, _DENS = {}, {}


def _model(dtype, H=1):
    """(state_dict on the CPU, float64 oracle parameters) of the structured model, built once and left unchanged."""
    if (dtype, H) not in _MODELS:
        den = X.structured_denoiser(dtype, num_heads=H)
        _MODELS[(dtype, H)] = ({k: v.clone() for k, v in den.state_dict().items()}, X.oracle_params(den))
    return _MODELS[(dtype, H)]


def _fresh_den(dev, dtype, wd, H=1, edit=None):
    from seeme_amd.mld_denoiser import MldDenoiser
    sd = dict(_model(dtype, H)[0])
    if edit is not None:
        edit(sd)
    den = MldDenoiser(X.ablation(), nfeats=75, condition=["text", "scene", "interactee"], latent_dim=[1, 256], ff_size=128,
                      num_layers=5, num_heads=H, weight_dtype=wd)
    den.load_state_dict(sd, strict=True)
    return den.to(dev).eval()


def _den(dev, dtype, wd, H=1, cluster=0, place=1, ms=True):
    """The module with weight image `wd` on the parameters made exact for `dtype` (shared between tests: only the launch policy changes)."""
    if (dtype, wd, H) not in _DENS:
        _DENS[(dtype, wd, H)] = _fresh_den(dev, dtype, wd, H)
    den = _DENS[(dtype, wd, H)]
    den.cluster, den.cluster_placement, den.cluster_flags, den.cluster_ms = cluster, place, 0, ms
    return den


def _sched(kind="ddim"):
    from seeme_amd.schedulers import DDIMScheduler, DDPMScheduler
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
    if kind == "ddim":
        return DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **kw)
    return DDPMScheduler(variance_type="fixed_small", **kw)


def _cus(dev):
    from seeme_amd.mld_denoiser import _device_cus
    return _device_cus(dev)


def _inputs(seed, B, N, cfg=False):
    rng = np.random.default_rng(seed)
    lat = rng.standard_normal((B, 1, 256)).astype(np.float32)
    cond = rng.standard_normal(((2 * B if cfg else B), N, 256)).astype(np.float32)
    return lat, cond


def _ddim(den, dev, lat, cond, steps, gs=1.0):
    sch = _sched()
    sch.set_timesteps(steps)
    out = den.sample_loop(torch.from_numpy(lat).to(dev), torch.from_numpy(cond).to(dev), sch, guidance_scale=gs)
    return out.cpu().numpy()


def _ddim_ref(dtype, H, lat, cond, steps, gs=1.0):
    ref = O.diffusion_reverse(_model(dtype, H)[1], cond.astype(np.float64), lat.astype(np.float64), steps, guidance_scale=gs, nhead=H)
    assert ref.dtype == np.float64
    return ref


def _report(what, e16, e32):
    print(f"exact16 {what}: 16-bit image rel err {e16:.3e}, fp32 image {e32:.3e}")


# ----------------------------------------------------------------------------- a, b: k_den_sample
@pytest.mark.parametrize("wd", ["fp16", "bf16"])
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("cfg", [False, True])
def test_one_cu_kernel_loop_vs_oracle(dev, wd, H, N, cfg):
    """k_den_sample (cluster = 0) in every compiled 16-bit variant -- folded / unfolded out_proj, one / many condition tokens, CFG pair --
    6 DDIM steps, B = 3.  With H = 1, N = 1 and no CFG this is the shipped one-head, one-token form, which cluster='auto' never runs at
    this batch size."""
    B, steps, gs = 3, 6, (2.5 if cfg else 1.0)
    lat, cond = _inputs(100 * H + 10 * N + int(cfg), B, N, cfg)
    ref = _ddim_ref(wd, H, lat, cond, steps, gs)
    errs = []
    for w in (wd, "fp32"):
        den = _den(dev, wd, w, H, cluster=0)
        assert den._cluster_plan(B, N, cfg, False, _cus(dev)) == (0, 1)
        errs.append(rel_err(_ddim(den, dev, lat, cond, steps, gs), ref))
    _report(f"k_den_sample {wd} H={H} N={N} cfg={cfg} 6 steps", *errs)
    assert errs[0] < TOL_LOOP and errs[1] < TOL_LOOP, errs


def test_one_cu_kernel_sample_pairs_vs_oracle(dev):
    """Batches above 256: two samples per workgroup on one weight stream; B = 259, so the last workgroup holds one sample."""
    B, steps = 259, 3
    lat, cond = _inputs(259, B, 1)
    ref = _ddim_ref("fp16", 1, lat, cond, steps)
    errs = []
    for w in ("fp16", "fp32"):
        den = _den(dev, "fp16", w, cluster=0)
        assert den._cluster_plan(B, 1, False, False, _cus(dev)) == (0, 1)
        out = _ddim(den, dev, lat, cond, steps)
        errs.append(rel_err(out, ref))
        assert rel_err(out[:, -1], ref[:, -1]) < TOL_LOOP and rel_err(out[:, -3:-1], ref[:, -3:-1]) < TOL_LOOP
    _report("k_den_sample fp16 B=259 (pairs) 3 steps", *errs)
    assert errs[0] < TOL_LOOP and errs[1] < TOL_LOOP, errs


# ----------------------------------------------------------------------------- c: k_den_cluster
@pytest.mark.parametrize("Cc,place", [(8, 1), (8, 0), (4, 1), (2, 1)])
@pytest.mark.parametrize("wd", ["fp16", "bf16"])
@pytest.mark.parametrize("N", [1, 2])
def test_cluster_kernel_loop_vs_oracle(dev, Cc, place, wd, N):
    """k_den_cluster: one sample split over Cc CUs, whose image also carries [W_in' W_s ; W_s] for layers 3 and 4.  B = 3, so the clusters
    beyond B exit; N = 2 adds the query / proj_out stages and the third exchange.  Cc = 8 on C XCDs (the default placement) and on one."""
    B, steps = 3, 6
    lat, cond = _inputs(1000 + 10 * Cc + N, B, N)
    ref = _ddim_ref(wd, 1, lat, cond, steps)
    errs = []
    for w in (wd, "fp32"):
        den = _den(dev, wd, w, cluster=Cc, place=place)
        assert den._cluster_plan(B, N, False, False, _cus(dev)) == (Cc, 1)
        errs.append(rel_err(_ddim(den, dev, lat, cond, steps), ref))
        assert den.cluster_status()[0] == 0
    _report(f"k_den_cluster C={Cc} placement={place} {wd} N={N} 6 steps", *errs)
    assert errs[0] < TOL_LOOP and errs[1] < TOL_LOOP, errs


# ----------------------------------------------------------------------------- d: k_den_cluster_ms
@pytest.mark.parametrize("wd,N,B,spc", [("fp16", 1, 65, 2), ("fp16", 2, 65, 2), ("bf16", 1, 65, 2), ("fp16", 1, 449, 8)])
def test_cluster_ms_kernel_loop_vs_oracle(dev, wd, N, B, spc):
    """k_den_cluster_ms: clusters of 4 CUs that own several samples.  B = 65: two samples per cluster, the last cluster ragged; B = 449: the
    full eight.  (The fp32 image has no such kernel: its module runs whatever the policy gives it and is printed for comparison.)"""
    steps = 4
    lat, cond = _inputs(B + N, B, N)
    ref = _ddim_ref(wd, 1, lat, cond, steps)
    den = _den(dev, wd, wd, cluster="auto", ms=True)
    assert den._cluster_plan(B, N, False, False, _cus(dev)) == (4, spc)
    out = _ddim(den, dev, lat, cond, steps)
    assert den.cluster_status()[0] == 0
    e16 = rel_err(out, ref)
    worst = max(rel_err(out[:, i], ref[:, i]) for i in range(B))           # every sample against its own largest entry
    e32 = rel_err(_ddim(_den(dev, wd, "fp32", cluster="auto", ms=True), dev, lat, cond, steps), ref)
    _report(f"k_den_cluster_ms {wd} N={N} B={B} 4 steps (worst sample {worst:.3e})", e16, e32)
    assert e16 < TOL_LOOP and worst < TOL_LOOP and e32 < TOL_LOOP


# ----------------------------------------------------------------------------- e: one forward
@pytest.mark.parametrize("Cc", [0, 8])
@pytest.mark.parametrize("wd", ["fp16", "bf16"])
def test_one_forward_vs_oracle(dev, Cc, wd):
    """MldDenoiser.forward on k_den_sample / k_den_cluster: scalar timesteps at both ends of the schedule, a per-sample timestep vector, and
    latents scaled by 64 -- layer 0's in_proj sees x + pe un-normalised, so the hi / lo operand split meets magnitudes near 200."""
    B = 3
    lat, cond = _inputs(7 + Cc, B, 1)
    cs = np.ascontiguousarray(np.transpose(cond, (1, 0, 2)))                  # seq-first, as the reference takes it
    P = _model(wd)[1]
    cases = [("t=981", lat, 981), ("t=1", lat, 1), ("tvec", lat, np.array([3, 999, 250])), ("x64 t=501", 64 * lat, 501)]
    for name, x, t in cases:
        ref = O.denoiser_forward(P, x.astype(np.float64), t, cs.astype(np.float64))
        errs = []
        for w in (wd, "fp32"):
            den = _den(dev, wd, w, cluster=Cc)
            assert den._cluster_plan(B, 1, False, True, _cus(dev)) == (Cc, 1)
            y = den(sample=torch.from_numpy(x).to(dev), timestep=torch.as_tensor(t).to(dev),
                    encoder_hidden_states=torch.from_numpy(cs).to(dev))[0].cpu().numpy()
            if Cc:
                assert den.cluster_status()[0] == 0
            errs.append((rel_err(y, ref), elem_err(y, ref)))
        print(f"exact16 forward C={Cc} {wd} {name}: 16-bit image rel {errs[0][0]:.3e} elem {errs[0][1]:.3e}, "
              f"fp32 image rel {errs[1][0]:.3e} elem {errs[1][1]:.3e}")
        assert max(errs[0]) < TOL_F32 and max(errs[1]) < TOL_F32, (name, errs)


# ----------------------------------------------------------------------------- f: DDPM with injected step noise
@pytest.mark.parametrize("Cc", [0, 8])
def test_ddpm_steps_vs_oracle(dev, Cc):
    """The first 5 of the 1000 ancestral steps with the noise injected (as test_ddpm_loop_vs_oracle does for the fp32 image)."""
    B, k = 2, 5
    rng = np.random.default_rng(3)
    lat = rng.standard_normal((B, 1, 256)).astype(np.float32)
    cond = rng.standard_normal((B, 1, 256)).astype(np.float32)
    noise = rng.standard_normal((k, B, 1, 256)).astype(np.float32)
    P = _model("fp16")[1]
    acp = O.alphas_cumprod(O.make_betas())
    x = lat.astype(np.float64)
    cs = np.transpose(cond, (1, 0, 2)).astype(np.float64)
    for i, t in enumerate(range(999, 999 - k, -1)):
        x = O.ddpm_step(acp, O.denoiser_forward(P, x, t, cs), t, x, noise[i].astype(np.float64))
    ref = np.transpose(x, (1, 0, 2))
    errs = []
    for w in ("fp16", "fp32"):
        den = _den(dev, "fp16", w, cluster=Cc)
        assert den._cluster_plan(B, 1, False, False, _cus(dev)) == (Cc, 1)
        sch = _sched("ddpm")
        sch.set_timesteps(1000)
        sch.timesteps = sch.timesteps[:k]
        out = den.sample_loop(torch.from_numpy(lat).to(dev), torch.from_numpy(cond).to(dev), sch, step_noise=torch.from_numpy(noise).to(dev))
        if Cc:
            assert den.cluster_status()[0] == 0
        errs.append(rel_err(out.cpu().numpy(), ref))
    _report(f"DDPM 5 steps C={Cc} fp16", *errs)
    assert errs[0] < TOL_LOOP and errs[1] < TOL_LOOP, errs


# ----------------------------------------------------------------------------- the gap, pinned
@pytest.mark.parametrize("Cc", [0, 8])
def test_dropped_bias_lane_is_caught(dev, Cc):
    """A defect of the size the old 16-bit bounds admitted: the kernel's module loses one element of input_blocks.0.sa_block.linear2.bias,
    the oracle keeps it.  The 6-step error lies above the new loop bound and below the old one (tests/test_exact16_cpu.py measures
    1.7e-3 with the oracle alone)."""
    def drop(sd):
        b = sd[X.PERTURB_KEY].clone()
        b[X.PERTURB_INDEX] = 0.0
        sd[X.PERTURB_KEY] = b
    lat, cond = (a.astype(np.float32) for a in X.sensitivity_inputs())
    ref = _ddim_ref("fp16", 1, lat, cond, 6)
    den = _fresh_den(dev, "fp16", "fp16", edit=drop)
    den.cluster = Cc
    assert den._cluster_plan(3, 1, False, False, _cus(dev)) == (Cc, 1)
    err = rel_err(_ddim(den, dev, lat, cond, 6), ref)
    if Cc:
        assert den.cluster_status()[0] == 0
    print(f"exact16 dropped bias lane C={Cc}: rel err {err:.3e}")
    assert X.LOOP_BOUND < err < X.OLD_LOOP_BOUND
