"""The float64 reference of the denoiser chain (tests/den_backward_reference.py) pinned on the CPU, before the device test
(tests/test_gpu_den_backward.py) holds k_den_bwd to it: its forward equals the autograd twin and the seeme_amd-independent oracle
stack in float64, its per-sample gradients summed over the batch and pushed through the table builders equal autograd through the
twin, and the conditions its inputs are chosen by (ReLU margin, share of mathematically zero gradients) hold for the reference alone."""
import pytest
import torch

import den_backward_reference as R

NS = [1, 2, 3, 4]
B = 4
# seeds of the vetted-sample fixture that are not 7000 + 10 N + masks: at that seed the 18 samples of (N = 1, all units kept) cost 13
# rejections, 42 % (the all-kept rejection rate is about 37 %; the cap is a condition on the inputs, so the inputs change)
VET_SEEDS = {(1, False): 7110}


def _relmax(a, b, floor=0.0):
    return float((a - b).abs().max()) / max(float(b.abs().max()), floor, 1e-300)


@pytest.fixture(scope="module")
def den64():
    return R.recipe_den64()


def _inputs(N, seed, masks):
    g = torch.Generator().manual_seed(seed)
    noisy = torch.randn(B, 256, generator=g, dtype=torch.float64)
    cond = torch.randn(B, N, 256, generator=g, dtype=torch.float64)
    dout = torch.randn(B, 256, generator=g, dtype=torch.float64)
    t = torch.tensor([0, 999, 250, 250])
    m = (torch.rand(B, R.DM_TOTAL, generator=g) < 0.7).to(torch.uint8) if masks else None
    return noisy, cond, dout, t, m


def _p(den):
    return float(den.encoder.blocks()[0].sa_block.self_attn.dropout)


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("N", NS)
def test_forward_equals_the_float64_twin(den64, N, masks):
    from seeme_amd.denoiser_autograd import denoiser_forward_torch
    noisy, cond, _, t, m = _inputs(N, 100 + N, masks)
    with torch.no_grad():
        ctab, ttab = R.tables(den64, cond, t)
        assert ctab.shape == (B, N, R.CROW) and ttab.shape == (B, R.TROW) and ctab.dtype == torch.float64
        got = R.chain_from_tables(R.chain_params(den64, torch.float64), noisy, ctab, ttab, list(range(B)), m, _p(den64))
        want = denoiser_forward_torch(den64, noisy[:, None], t, cond.permute(1, 0, 2), masks=m)[:, 0]
        if masks:                                                      # ... and the masks do change the forward
            assert _relmax(denoiser_forward_torch(den64, noisy[:, None], t, cond.permute(1, 0, 2))[:, 0], want) > 1e-2
    e = _relmax(got, want)
    print(f"N={N} masks={masks}: reference forward vs float64 twin {e:.2e}")
    assert e <= 1e-12


@pytest.mark.parametrize("N", NS)
def test_eval_forward_equals_the_oracle_stack(den64, N):
    """oracle.mld_oracle_torch's md_layer / _skip_stack: full sequence attention, nothing shared with seeme_amd.  Both sides get
    the same time embedding (oracle.denoiser_forward computes fp32 timestep features of its own and lands 2.5e-6 away)."""
    from oracle import mld_oracle_torch as OT
    noisy, cond, _, t, _ = _inputs(N, 200 + N, False)
    P = {k: v.detach() for k, v in den64.state_dict().items()}
    with torch.no_grad():
        emb = R.time_emb(den64, t)
        ctab, ttab = R.tables(den64, cond, t)
        got = R.chain_from_tables(R.chain_params(den64, torch.float64), noisy, ctab, ttab, list(range(B)), None, 0.0)
        x = noisy[:, None] + P["query_pos.pe"][:1, 0][None]
        want = OT._skip_stack(x, P, "encoder.", 5, lambda h, pre: OT.md_layer(P, pre, h, cond, emb, 1))[:, 0]
    e = _relmax(got, want)
    print(f"N={N}: reference forward vs oracle stack {e:.2e}")
    assert e <= 1e-12


def test_shared_time_rows_and_taps(den64):
    """trow picks each sample's row of ttab, and relu_margin is what its definition says (dropped units do not count)."""
    noisy, cond, _, t, m = _inputs(2, 300, True)
    P = R.chain_params(den64, torch.float64)
    with torch.no_grad():
        ctab, ttab = R.tables(den64, cond, t)
        a = R.chain_from_tables(P, noisy, ctab, ttab, [0, 1, 2, 3], m, 0.5)
        b = R.chain_from_tables(P, noisy, ctab, ttab[:3], [0, 1, 2, 2], m, 0.5)          # t[2] == t[3]
        assert torch.equal(a, b)
        taps = []
        R.chain_from_tables(P, noisy, ctab, ttab, [0, 1, 2, 3], m, 0.5, taps)
    assert len(taps) == 5 and taps[0].shape == (B, 1024)
    want = []
    for s in range(B):
        per = []
        for l in range(5):
            keep = m[s, l * R.DM_LAYER + 264:l * R.DM_LAYER + 264 + 1024].bool()
            per.append(float(taps[l][s].abs()[keep].min() / taps[l][s].abs().max()))
        want.append(min(per))
    got = R.relu_margin(P, noisy, ctab, ttab, [0, 1, 2, 3], m, 0.5)
    assert torch.allclose(got, torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0)
    m2 = m.clone()                                              # a dropped unit exactly on the kink does not count, a kept one does
    z0 = float(taps[0][0].abs().max())
    unit = int(torch.nonzero(m[0, 264:264 + 1024] == 0)[0])
    P2 = dict(P)
    b1 = P["encoder.input_blocks.0.sa_block.linear1.bias"].clone()
    b1[unit] -= taps[0][0, unit]
    P2["encoder.input_blocks.0.sa_block.linear1.bias"] = b1
    assert float(R.relu_margin(P2, noisy, ctab, ttab, [0, 1, 2, 3], m, 0.5)[0]) == float(got[0]) and z0 > 0
    m2[0, 264 + unit] = 1
    assert float(R.relu_margin(P2, noisy, ctab, ttab, [0, 1, 2, 3], m2, 0.5)[0]) < 1e-12


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("N", NS)
def test_per_sample_gradients_sum_to_autograd_through_the_twin(den64, N, masks):
    """sum_b of the per-sample chain gradients, plus the table gradients carried through denoiser_train._tables and the timestep
    MLP, plus d noisy into query_pos.pe[0], against loss.backward() through the float64 twin: every named parameter."""
    from seeme_amd.denoiser_autograd import denoiser_forward_torch
    noisy, cond, dout, t, m = _inputs(N, 400 + N, masks)
    named = dict(den64.named_parameters())
    for p in named.values():
        p.grad = None
    out = denoiser_forward_torch(den64, noisy[:, None], t, cond.permute(1, 0, 2), masks=m)[:, 0]
    (out * dout).sum().backward()
    want = {k: (None if p.grad is None else p.grad.clone()) for k, p in named.items()}
    for p in named.values():
        p.grad = None

    ctab, ttab = R.tables(den64, cond, t)                                        # with their graph
    P = R.chain_params(den64, torch.float64)
    per = R.per_sample_grads(P, noisy, ctab.detach(), ttab.detach(), list(range(B)), m, _p(den64), dout)
    assert len(per) == B
    for b, (o, g) in enumerate(per):
        assert _relmax(o, out[b].detach()) <= 1e-12
        assert g["ctab"].shape == (N, R.CROW) and g["ttab"].shape == (R.TROW,) and g["noisy"].shape == (256,)
    total = {k: sum(g[k] for _, g in per) for k in R.chain_keys()}
    dctab = torch.stack([g["ctab"] for _, g in per])
    dttab = torch.stack([g["ttab"] for _, g in per])
    plist = list(named.items())
    tg = torch.autograd.grad([ctab, ttab], [p for _, p in plist], [dctab, dttab], allow_unused=True)
    got = {k: g for (k, _), g in zip(plist, tg)}
    for k, g in total.items():
        got[k] = g if got[k] is None else got[k] + g
    dpe = torch.zeros_like(named["query_pos.pe"])
    dpe[0, 0] = sum(g["noisy"] for _, g in per)
    got["query_pos.pe"] = dpe
    gmax = max(float(v.abs().max()) for v in want.values() if v is not None)
    worst = ("", 0.0)
    for k, w in want.items():
        if w is None:
            assert got[k] is None, k
            continue
        assert got[k] is not None, k
        e = _relmax(got[k], w, 1e-4 * gmax)
        if e > worst[1]:
            worst = (k, e)
    print(f"N={N} masks={masks}: summed per-sample gradients vs twin autograd, worst {worst[1]:.2e} at {worst[0]}")
    assert worst[1] <= 1e-10, worst


# ----------------------------------------------------------------------------- the conditions of the device test, for the reference alone
@pytest.fixture(scope="module")
def vetted():
    return {(N, wm): R.vetted_samples(N, 18, VET_SEEDS.get((N, wm), 7000 + 10 * N + int(wm)), wm) for N in NS for wm in (False, True)}


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("N", NS)
def test_vetting_rejects_within_its_cap(vetted, N, with_masks):
    v = vetted[(N, with_masks)]
    share = v["rejected"] / v["drawn"]
    print(f"N={N} masks={with_masks}: relu margin >= {R.RELU_MARGIN:g} rejects {v['rejected']} of {v['drawn']} candidates ({100 * share:.0f} %)")
    assert share <= 0.4 and float(v["margin"].min()) >= R.RELU_MARGIN
    assert v["noisy"].shape == (18, 256) and v["cond"].shape == (18, N, 256) and v["t"].shape == (18,)
    assert (v["masks"] is None) == (not with_masks)
    if with_masks:
        assert v["masks"].shape == (18, R.DM_TOTAL) and abs(float(v["masks"].float().mean()) - 0.5) < 0.01


def test_vetting_pins_timesteps_and_attention_bytes():
    ts = [0, 999, None, 250, 250]
    rows = [None, [1, 0, 1, 0, 1, 0, 1, 1], None, None, [0] * 8]
    v = R.vetted_samples(4, 5, 31, True, timesteps=ts, p_rows=rows)
    assert v["t"][[0, 1, 3, 4]].tolist() == [0, 999, 250, 250]
    for l in range(5):
        assert v["masks"][1, l * R.DM_LAYER:l * R.DM_LAYER + 8].tolist() == rows[1]
        assert v["masks"][4, l * R.DM_LAYER:l * R.DM_LAYER + 8].tolist() == rows[4]
    w = R.vetted_samples(4, 5, 31, True, timesteps=ts, p_rows=rows)
    assert all(torch.equal(v[k], w[k]) for k in ("noisy", "cond", "t", "masks"))


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("N", NS)
def test_floor_share_and_float32_yardstick(den64, vetted, N, with_masks):
    """Of the (sample, tensor) pairs of vetted samples, at most 20 % (N = 1: a softmax over one token has zero gradient, so the
    query path of the linear attention has none) / 5 % (N >= 2) have a float64 gradient below the floor.  And the same code in
    float32 -- the yardstick of the device test's 4x rule -- is itself inside the device test's ceilings on these samples."""
    v = vetted[(N, with_masks)]
    n = 6
    noisy, cond, t = v["noisy"][:n], v["cond"][:n], v["t"][:n]
    m = None if v["masks"] is None else v["masks"][:n]
    dout = torch.randn(n, 256, generator=torch.Generator().manual_seed(5 + N), dtype=torch.float64)
    with torch.no_grad():
        ctab, ttab = R.tables(den64, cond.double(), t)
    ref = R.iter_per_sample_grads(R.chain_params(den64, torch.float64), noisy.double(), ctab, ttab, list(range(n)), m, 0.5, dout)
    tw = R.iter_per_sample_grads(R.chain_params(den64, torch.float32), noisy, ctab.float(), ttab.float(), list(range(n)), m, 0.5, dout.float())
    low = pairs = 0
    worst = {}
    for (o64, g64), (o32, g32) in zip(ref, tw):
        errs, lows = R.pair_errors(g32, g64, N)
        pairs += len(errs) + len(lows)
        low += len(lows)
        assert all(x <= R.FLOOR_ABS for x in lows.values()), lows
        for (kind, _), e in errs.items():
            worst[kind] = max(worst.get(kind, 0.0), e)
        assert _relmax(o32.double(), o64) <= 1e-4
    share = low / pairs
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print(f"N={N} masks={with_masks}: {low} of {pairs} pairs below the floor ({100 * share:.1f} %); float32 reference worst kinds {top}")
    assert share <= (0.20 if N == 1 else 0.05)
    for kind, e in worst.items():
        assert e <= (2e-4 if kind.startswith("ctab") or kind == "dx0" else 5e-4), (kind, e)
