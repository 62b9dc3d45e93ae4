"""k_den_cluster keeps the launch-constant small operands of all five layers resident in LDS for the length of a launch
(csrc/den_cluster.inc.hip, ClRes) and streams only the rows that change with step and layer.  What that could break and no stored
array is needed for: operands of one launch seen by the next (another condition, another batch size, another scheduler, per-sample
timestep rows), for every cluster size and both resident layouts of the weight dtype.  Needs a real MI355X: `pytest -m gpu`."""
import pytest
import torch

from conftest import rel_err
from test_gpu_parity import _sched, _with_cluster, make_den

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


# tolerances against the one-CU kernel: those of test_gpu_parity.test_cluster_sampler_equals_one_cu_kernel
@pytest.mark.parametrize("wd,tol", [("fp16", 5e-4), ("fp32", 1e-5)])
@pytest.mark.parametrize("Cc", [8, 4, 2])
def test_resident_operands_do_not_leak_between_launches(dev, wd, tol, Cc):
    """ONE model runs four different launches in a row; each result is bit-identical to the same call on a freshly built model,
    agrees with the one-CU-per-sample kernel, and no cluster gives up."""
    torch.manual_seed(11)
    lat, cond_x, cond_y = (torch.randn(32, 1, 256, device=dev) for _ in range(3))
    noise = torch.randn(40, 32, 256, device=dev)
    t = torch.randint(0, 1000, (32,), device=dev)

    def ddim50(d):
        sch = _sched()
        sch.set_timesteps(50)
        return d.sample_loop(lat, cond_x, sch)

    def ddim20_ragged(d):
        sch = _sched()
        sch.set_timesteps(20)
        return d.sample_loop(lat[:5].contiguous(), cond_y[:5].contiguous(), sch)

    def ddpm40(d):
        sch = _sched("ddpm")
        sch.set_timesteps(1000)
        sch.timesteps = sch.timesteps[:40]
        return d.sample_loop(lat, cond_x, sch, step_noise=noise)

    def forward_tvec(d):
        return d(sample=lat, timestep=t, encoder_hidden_states=cond_y.permute(1, 0, 2))[0]

    den = _with_cluster(make_den(dev, weight_dtype=wd), Cc)
    for call in (ddim50, ddim20_ragged, ddpm40, forward_tvec):
        z = call(den)
        assert den.cluster_status()[0] == 0, (call.__name__, "a cluster gave up waiting for a peer")
        fresh = _with_cluster(make_den(dev, weight_dtype=wd), Cc)
        zf = call(fresh)
        assert fresh.cluster_status()[0] == 0, call.__name__
        z1 = call(_with_cluster(fresh, 0))
        err = rel_err(z.cpu().numpy(), z1.cpu().numpy())
        print(f"{wd} C={Cc} {call.__name__}: equal to a fresh model {torch.equal(z, zf)}, rel err vs one-CU kernel {err:.3e} (bound {tol:g})")
        assert torch.equal(z, zf), call.__name__
        assert err < tol, (call.__name__, err)
