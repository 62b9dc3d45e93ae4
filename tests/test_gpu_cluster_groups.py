"""k_den_cluster at 8 CUs per sample on a 16-bit image runs its six GEMV phases on two wave groups in turn (csrc/den_cluster.inc.hip,
ClGrp): waves 0 .. 3 take A, C, E, waves 4 .. 7 take B, D, F, and each wave plays two stored waves of the unchanged weight image.  Per
output tile the k-blocks and their order are the same, so the result must be BIT-identical to an independent kernel body that still
consumes every unit with all eight waves on the same C = 8 image: k_den_cluster_ms forced to 8-CU clusters of two samples
(SEEME_DEN_CLUSTER_MS_PLAN = "8,2"; the same exchanges and order of every addition, test_gpu_parity.test_cluster_ms_equals_one_sample_cluster).

Where that kernel cannot run -- it takes neither the bf16 image at C = 8 nor per-sample timestep rows, which is all MldDenoiser.forward
launches -- the reference is the one-CU-per-sample kernel (cluster = 0) at the tolerance test_gpu_parity.test_cluster_sampler_equals_one_cu_kernel
holds that pair to (fp16 5e-4, bf16 5e-3: the contraction order differs).  Needs a real MI355X: `pytest -m gpu`."""
import pytest
import torch

from conftest import rel_err
from test_gpu_parity import _sched, _with_cluster, make_den

pytestmark = pytest.mark.gpu

STEPS = 3      # crosses every layer seam, both skip layers, the step seam and the ring wrap


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def den16(dev):
    return make_den(dev, weight_dtype="fp16")


def _ddim():
    sch = _sched()
    sch.set_timesteps(STEPS)
    return sch


def _inputs(dev, B, seed):
    torch.manual_seed(seed)
    return torch.randn(B, 1, 256, device=dev), torch.randn(B, 1, 256, device=dev)


def _run_pair(den, monkeypatch, B, call):
    """call(den) under the default plan (k_den_cluster, one sample per 8-CU cluster) and under the forced ms plan; no give-up in either."""
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
    return z, ref


@pytest.mark.parametrize("B", [2, 9])
def test_groups_bit_identical_to_eight_wave_body(dev, den16, monkeypatch, B):
    """B = 2: one cluster of the reference; B = 9: ragged, clusters padded to 8.  3 DDIM steps, fp16 image; and twice the same bits."""
    lat, cond = _inputs(dev, B, 20 + B)
    z, ref = _run_pair(den16, monkeypatch, B, lambda d: d.sample_loop(lat, cond, _ddim()))
    z2 = den16.sample_loop(lat, cond, _ddim())
    assert den16.cluster_status()[0] == 0
    print(f"B={B}: max |z - ref| = {float((z - ref).abs().max()):.3e}, repeat equal {torch.equal(z, z2)}")
    assert torch.equal(z, ref), float((z - ref).abs().max())
    assert torch.equal(z, z2)


def test_groups_bit_identical_with_step_noise(dev, den16, monkeypatch):
    """DDIM with eta = 0.5 and given step noise, B = 2, 3 steps."""
    lat, cond = _inputs(dev, 2, 31)
    noise = torch.randn(STEPS, 2, 256, device=dev)
    z, ref = _run_pair(den16, monkeypatch, 2, lambda d: d.sample_loop(lat, cond, _ddim(), eta=0.5, step_noise=noise))
    plain = den16.sample_loop(lat, cond, _ddim())
    print(f"eta=0.5: max |z - ref| = {float((z - ref).abs().max()):.3e}")
    assert torch.equal(z, ref), float((z - ref).abs().max())
    assert not torch.equal(z, plain), "the step noise did not reach the kernel"


@pytest.mark.parametrize("wd,tol", [("fp16", 5e-4), ("bf16", 5e-3)])
def test_groups_forward_per_sample_timesteps(dev, wd, tol):
    """MldDenoiser.forward (SCHED_NONE, steps = 1), B = 3, per-sample timesteps: against the one-CU-per-sample kernel; twice the same bits."""
    den = make_den(dev, weight_dtype=wd)
    lat, cond = _inputs(dev, 3, 41)
    t = torch.tensor([981, 501, 1], device=dev)
    call = lambda d: d(sample=lat, timestep=t, encoder_hidden_states=cond.permute(1, 0, 2))[0]
    _with_cluster(den, "auto")
    assert den._cluster_plan(3, 1, False, True) == (8, 1)
    y, y2 = call(den), call(den)
    assert den.cluster_status()[0] == 0
    y0 = call(_with_cluster(den, 0))
    err = rel_err(y.cpu().numpy(), y0.cpu().numpy())
    print(f"{wd} forward: rel err vs one-CU kernel {err:.3e} (bound {tol:g})")
    assert torch.equal(y, y2)
    assert err < tol, err


def test_groups_bf16_image(dev):
    """The bf16 image (k_den_cluster_ms does not take it at C = 8): B = 9, 3 DDIM steps against the one-CU-per-sample kernel; twice the same bits."""
    den = _with_cluster(make_den(dev, weight_dtype="bf16"), "auto")
    lat, cond = _inputs(dev, 9, 51)
    assert den._cluster_plan(9, 1, False, False) == (8, 1)
    z, z2 = den.sample_loop(lat, cond, _ddim()), den.sample_loop(lat, cond, _ddim())
    assert den.cluster_status()[0] == 0
    base = _with_cluster(den, 0).sample_loop(lat, cond, _ddim())
    err = rel_err(z.cpu().numpy(), base.cpu().numpy())
    print(f"bf16 B=9: rel err vs one-CU kernel {err:.3e} (bound 5e-3)")
    assert torch.equal(z, z2)
    assert err < 5e-3, err
