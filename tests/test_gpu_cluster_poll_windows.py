"""k_den_cluster on two wave groups (16-bit image, 8 CUs per sample; csrc/den_cluster.inc.hip, ClGrp) requests HALF of unit E behind the FIRST
poll of the X1 exchange (the other half where the whole unit used to be requested, in phase B): the epilogue wave issues the poll's loads, then
its own share of the half unit, sets an LDS word ("first poll issued", FPI) to the exchange's epoch and only then waits for the poll; waves
1 .. 3 spin on that word and request their shares.
Only WHEN a weight load is requested changes -- no operand, no sum, no order -- so every result must be BIT-identical to the independent body
that consumes every unit with all eight waves (k_den_cluster_ms forced to the plan "8,2", as tests/test_gpu_cluster_groups.py does), and a wave
that waits for the new word must always see it arrive: no launch may end with a give-up code.  Where that body cannot run (bf16 image at C = 8,
per-sample timestep rows) the reference is the one-CU-per-sample kernel at the tolerance test_gpu_cluster_groups.py holds that pair to.
Needs a real MI355X: `pytest -m gpu`."""
import pytest
import torch

from conftest import rel_err
from test_gpu_parity import _sched, _with_cluster, make_den

pytestmark = pytest.mark.gpu

STEPS = 3      # crosses every layer seam, both skip layers, the step seam


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def den16(dev):
    return make_den(dev, weight_dtype="fp16")


def _sch(kind="ddim"):
    sch = _sched(kind)
    sch.set_timesteps(1000 if kind == "ddpm" else STEPS)
    sch.timesteps = sch.timesteps[:STEPS]
    return sch


def _inputs(dev, B, seed):
    torch.manual_seed(seed)
    return torch.randn(B, 1, 256, device=dev), torch.randn(B, 1, 256, device=dev)


def _launch(den, call):
    out = call(den)
    assert den.cluster_status()[0] == 0, "a cluster gave up waiting for a peer"
    return out


def _run_pair(den, monkeypatch, B, call):
    """call(den) under the forced ms plan (the eight-wave body) and under the default plan (k_den_cluster, two wave groups)."""
    _with_cluster(den, "auto")
    monkeypatch.delenv("SEEME_DEN_CLUSTER", raising=False)
    monkeypatch.setenv("SEEME_DEN_CLUSTER_MS_PLAN", "8,2")
    assert den._cluster_plan(B, 1, False, False) == (8, 2), "the forced plan did not select k_den_cluster_ms"
    ref = _launch(den, call)
    monkeypatch.delenv("SEEME_DEN_CLUSTER_MS_PLAN")
    assert den._cluster_plan(B, 1, False, False) == (8, 1)
    return _launch(den, call), ref


@pytest.mark.parametrize("B", [2, 9])
def test_poll_windows_ddim_bit_identical(dev, den16, monkeypatch, B):
    """fp16 image, 3 DDIM steps; B = 2: one cluster of the reference, B = 9: a ragged second row of clusters.  Twice the same bits."""
    lat, cond = _inputs(dev, B, 60 + B)
    call = lambda d: d.sample_loop(lat, cond, _sch())
    z, ref = _run_pair(den16, monkeypatch, B, call)
    z2 = _launch(den16, call)
    print(f"B={B}: max |z - ref| = {float((z - ref).abs().max()):.3e}, repeat equal {torch.equal(z, z2)}")
    assert torch.equal(z, ref), float((z - ref).abs().max())
    assert torch.equal(z, z2)


def test_poll_windows_ddpm_step_noise_bit_identical(dev, den16, monkeypatch):
    """DDPM ancestral steps with injected step noise, B = 9, 3 steps."""
    B = 9
    lat, cond = _inputs(dev, B, 71)
    noise = torch.randn(STEPS, B, 256, device=dev)
    call = lambda d: d.sample_loop(lat, cond, _sch("ddpm"), step_noise=noise)
    z, ref = _run_pair(den16, monkeypatch, B, call)
    z2 = _launch(den16, call)
    quiet = _launch(den16, lambda d: d.sample_loop(lat, cond, _sch("ddpm"), step_noise=torch.zeros_like(noise)))
    print(f"ddpm B={B}: max |z - ref| = {float((z - ref).abs().max()):.3e}, repeat equal {torch.equal(z, z2)}")
    assert torch.equal(z, ref), float((z - ref).abs().max())
    assert torch.equal(z, z2)
    assert not torch.equal(z, quiet), "the step noise did not reach the kernel"


def test_poll_windows_bf16_image(dev):
    """bf16 image, B = 9, 3 DDIM steps: against the one-CU-per-sample kernel within 5e-3; twice the same bits."""
    den = _with_cluster(make_den(dev, weight_dtype="bf16"), "auto")
    lat, cond = _inputs(dev, 9, 81)
    assert den._cluster_plan(9, 1, False, False) == (8, 1)
    call = lambda d: d.sample_loop(lat, cond, _sch())
    z, z2 = _launch(den, call), _launch(den, call)
    base = _with_cluster(den, 0).sample_loop(lat, cond, _sch())
    err = rel_err(z.cpu().numpy(), base.cpu().numpy())
    print(f"bf16 B=9: rel err vs one-CU kernel {err:.3e} (bound 5e-3)")
    assert torch.equal(z, z2)
    assert err < 5e-3, err


def test_poll_windows_placements_and_store_flavours(dev, den16, monkeypatch):
    """Placement 0 (one XCD) / 1 (eight XCDs) x flags 0 / 1 (flags 1: write-through granule stores) at B = 9: four times the same bits."""
    monkeypatch.delenv("SEEME_DEN_CLUSTER", raising=False)
    monkeypatch.delenv("SEEME_DEN_CLUSTER_PLACE", raising=False)
    monkeypatch.delenv("SEEME_DEN_CLUSTER_FLAGS", raising=False)
    monkeypatch.delenv("SEEME_DEN_CLUSTER_MS_PLAN", raising=False)
    lat, cond = _inputs(dev, 9, 91)
    outs = {}
    for place in (0, 1):
        for flags in (0, 1):
            _with_cluster(den16, "auto", place, flags)
            assert den16._cluster_plan(9, 1, False, False) == (8, 1)
            outs[(place, flags)] = _launch(den16, lambda d: d.sample_loop(lat, cond, _sch()))
            if place == 1 or flags == 1:
                assert den16.cluster_status()[1] == 0, "write-through stores were asked for, or the cluster spans XCDs"
    _with_cluster(den16, "auto")
    for k, z in outs.items():
        assert torch.equal(z, outs[(0, 0)]), k


def test_poll_windows_one_forward_launch(dev, den16, monkeypatch):
    """MldDenoiser.forward (SCHED_NONE, steps = 1, per-sample timesteps) at B = 2: the shortest launch, the release happens exactly five times.
    Against the one-CU-per-sample kernel at that pair's fp16 tolerance (5e-4); twice the same bits."""
    monkeypatch.delenv("SEEME_DEN_CLUSTER", raising=False)
    lat, cond = _inputs(dev, 2, 101)
    t = torch.tensor([981, 1], device=dev)
    call = lambda d: d(sample=lat, timestep=t, encoder_hidden_states=cond.permute(1, 0, 2))[0]
    _with_cluster(den16, "auto")
    assert den16._cluster_plan(2, 1, False, True) == (8, 1)
    y, y2 = _launch(den16, call), _launch(den16, call)
    y0 = call(_with_cluster(den16, 0))
    _with_cluster(den16, "auto")
    err = rel_err(y.cpu().numpy(), y0.cpu().numpy())
    print(f"forward B=2: rel err vs one-CU kernel {err:.3e} (bound 5e-4)")
    assert torch.equal(y, y2)
    assert err < 5e-4, err


def test_poll_windows_four_launches_on_one_model(dev, den16, monkeypatch):
    """Four launches in a row on one model -- another B or scheduler each time; the LDS word and the granule tags of one launch must
    not leak into the next -- each bit-identical to the same launch on a freshly built model."""
    monkeypatch.delenv("SEEME_DEN_CLUSTER", raising=False)
    monkeypatch.delenv("SEEME_DEN_CLUSTER_MS_PLAN", raising=False)
    _with_cluster(den16, "auto")
    torch.manual_seed(109)
    noise = {B: torch.randn(STEPS, B, 256, device=dev) for B in (2, 3)}
    plan = [(9, "ddim"), (2, "ddpm"), (3, "ddpm"), (5, "ddim")]

    def run(den, B, kind, seed):
        lat, cond = _inputs(dev, B, seed)
        kw = dict(step_noise=noise[B]) if kind == "ddpm" else {}
        return _launch(den, lambda d: d.sample_loop(lat, cond, _sch(kind), **kw))

    kept = [run(den16, B, kind, 110 + i) for i, (B, kind) in enumerate(plan)]
    for i, (B, kind) in enumerate(plan):
        fresh = run(_with_cluster(make_den(dev, weight_dtype="fp16"), "auto"), B, kind, 110 + i)
        assert torch.equal(kept[i], fresh), (i, B, kind)
