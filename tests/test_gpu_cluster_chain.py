"""The two-wave-group body of k_den_cluster (csrc/den_cluster.inc.hip, ClGrp) reads the MFMA A-operand fragments and the epilogue
operands of a phase ahead of its MFMA chain, and finds the scheduler coefficients, the step noise and the next step's table row in
LDS / in a register, requested in the X1 windows of the step (ClRowG) -- no sum changes, so the result stays BIT-identical to the
eight-wave body of k_den_cluster_ms on the same C = 8 image (SEEME_DEN_CLUSTER_MS_PLAN = "8,2", the reference of
test_gpu_cluster_groups.py), which still reads its fragments per k-block and its coefficients with scalar loads.

Shapes: the smallest at which the staging of the scheduler operands can go wrong -- 1 step (the clamp of the next step at the last
one is the only step), 2 and 4 steps (the rows written by the five windows of one step are read by that step's scheduler and
replaced in the next), B = 1 (one cluster, seven padded) and B = 9 (two rounds of clusters, ragged); step noise with DDIM eta = 0.5 and
with the DDPM scheduler of `bench.py --scheduler ddpm` cut to 4 steps; and MldDenoiser.forward (no scheduler: the coefficient lanes
re-read a table row instead, per-sample timestep rows).  Five layers always include both skip layers.  Needs a real MI355X: `pytest -m gpu`."""
import pytest
import torch

from conftest import rel_err
from test_gpu_parity import _sched, _with_cluster, make_den

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def den16(dev):
    return make_den(dev, weight_dtype="fp16")


def _ddim(steps):
    sch = _sched()
    sch.set_timesteps(steps)
    return sch


def _ddpm(steps):
    sch = _sched("ddpm")            # the scheduler of `bench.py --scheduler ddpm`
    sch.set_timesteps(1000)
    sch.timesteps = sch.timesteps[:steps]
    return sch


def _inputs(dev, B, seed):
    torch.manual_seed(seed)
    return torch.randn(B, 1, 256, device=dev), torch.randn(B, 1, 256, device=dev)


def _run_pair(den, monkeypatch, B, call):
    """call(den) under the forced ms plan (eight-wave body, the reference) and under the default plan (two wave groups), the latter twice;
    no cluster gives up in any launch."""
    _with_cluster(den, "auto")
    monkeypatch.delenv("SEEME_DEN_CLUSTER", raising=False)
    monkeypatch.setenv("SEEME_DEN_CLUSTER_MS_PLAN", "8,2")
    assert den._cluster_plan(B, 1, False, False) == (8, 2), "the forced plan did not select k_den_cluster_ms"
    ref = call(den)
    assert den.cluster_status()[0] == 0, "a cluster of the reference kernel gave up waiting for a peer"
    monkeypatch.delenv("SEEME_DEN_CLUSTER_MS_PLAN")
    assert den._cluster_plan(B, 1, False, False) == (8, 1)
    z = call(den)
    assert den.cluster_status()[0] == 0, "a cluster gave up waiting for a peer"
    z2 = call(den)
    assert den.cluster_status()[0] == 0, "a cluster gave up waiting for a peer (second run)"
    return z, z2, ref


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("steps", [1, 2, 4])
def test_chain_ddim_bit_identical(dev, den16, monkeypatch, steps, B):
    lat, cond = _inputs(dev, B, 100 + 10 * steps + B)
    z, z2, ref = _run_pair(den16, monkeypatch, B, lambda d: d.sample_loop(lat, cond, _ddim(steps)))
    print(f"ddim steps={steps} B={B}: max |z - ref| = {float((z - ref).abs().max()):.3e}, repeat equal {torch.equal(z, z2)}")
    assert torch.equal(z, ref), float((z - ref).abs().max())
    assert torch.equal(z, z2)


@pytest.mark.parametrize("steps", [2, 4])
def test_chain_step_noise_bit_identical(dev, den16, monkeypatch, steps):
    """DDIM with eta = 0.5 and given step noise, B = 2: the noise row travels through LDS; it must reach the result."""
    lat, cond = _inputs(dev, 2, 200 + steps)
    noise = torch.randn(steps, 2, 256, device=dev)
    z, z2, ref = _run_pair(den16, monkeypatch, 2, lambda d: d.sample_loop(lat, cond, _ddim(steps), eta=0.5, step_noise=noise))
    plain = den16.sample_loop(lat, cond, _ddim(steps))
    assert den16.cluster_status()[0] == 0
    print(f"eta=0.5 steps={steps}: max |z - ref| = {float((z - ref).abs().max()):.3e}, max |z - plain| = {float((z - plain).abs().max()):.3e}")
    assert torch.equal(z, ref), float((z - ref).abs().max())
    assert torch.equal(z, z2)
    assert not torch.equal(z, plain), "the step noise did not reach the kernel"


def test_chain_ddpm_bit_identical(dev, den16, monkeypatch):
    """The DDPM scheduler of `bench.py --scheduler ddpm` (1000 ancestral steps), cut to its first 4, B = 2, given step noise."""
    lat, cond = _inputs(dev, 2, 301)
    noise = torch.randn(4, 2, 256, device=dev)
    z, z2, ref = _run_pair(den16, monkeypatch, 2, lambda d: d.sample_loop(lat, cond, _ddpm(4), step_noise=noise))
    other = den16.sample_loop(lat, cond, _ddpm(4), step_noise=noise.flip(0))
    assert den16.cluster_status()[0] == 0
    print(f"ddpm 4 steps: max |z - ref| = {float((z - ref).abs().max()):.3e}")
    assert torch.equal(z, ref), float((z - ref).abs().max())
    assert torch.equal(z, z2)
    assert not torch.equal(z, other), "the step noise did not reach the kernel"


def test_chain_forward_per_sample_timesteps(dev, den16):
    """MldDenoiser.forward (no scheduler, steps = 1), B = 3, per-sample timesteps: k_den_cluster_ms does not take per-sample rows, so the
    reference is the one-CU-per-sample kernel at the tolerance of test_gpu_parity.test_cluster_sampler_equals_one_cu_kernel (fp16 5e-4);
    twice the same bits."""
    lat, cond = _inputs(dev, 3, 401)
    t = torch.tensor([981, 501, 1], device=dev)
    call = lambda d: d(sample=lat, timestep=t, encoder_hidden_states=cond.permute(1, 0, 2))[0]
    _with_cluster(den16, "auto")
    assert den16._cluster_plan(3, 1, False, True) == (8, 1)
    y = call(den16)
    assert den16.cluster_status()[0] == 0
    y2 = call(den16)
    assert den16.cluster_status()[0] == 0
    y0 = call(_with_cluster(den16, 0))
    _with_cluster(den16, "auto")
    err = rel_err(y.cpu().numpy(), y0.cpu().numpy())
    print(f"forward: rel err vs one-CU kernel {err:.3e} (bound 5e-4)")
    assert torch.equal(y, y2)
    assert err < 5e-4, err
