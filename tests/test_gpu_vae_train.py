"""seeme_amd/vae_train.py -- the recorded launch lists of the stage-1 VAE forward / backward (grouped-GEMM descriptor tables with
hand-written offsets and batch strides, the choice between seeme_gemm128 / seeme_wgrad128 and the grouped GEMM, split atomic
weight-gradient reductions, the plan cache) -- against the float64 twin of tests/vae_train_reference.py (pinned on the CPU by
tests/test_vae_train_cpu.py): PER SAMPLE and per part, at the shapes of vae_train_reference.CASES, in eval mode and with the plans'
own keep-masks in training mode, and through the plan life cycle.

Sample b's gradient is read by a step whose upstream gradient (fixed random ddist / dfeats) is zero outside sample b, from zeroed
``.grad``: B small steps per case.  Padded feature frames hold values 1e3 times the valid ones; dfeats is non-zero on padded frames
in `m128_dec` and masked elsewhere.  Measures, all against float64: max|got - ref64| / max|ref64| for mu, logvar, the valid rows of
feats, the padded rows of feats, dz[b] and every non-zero part; the key-bias parts max|got - ref64| <= 1e-5 S_b; parts that are
exactly 0 in the reference stay bit-equal to what ``.grad`` held on entry.

Bound (DESIGN 5.7's rule; vae_train_reference.bounds): per case and kind the HIP path's worst error over samples and layers is at most
4 x the worst error of the float32 CPU run of the same reference on the same inputs (same computation, other summation order, here
with atomics on top), and every (sample, part) pair is under 3 x the worst e_tw of its case; forward outputs 1e-4 and 4 x the float32
reference's own error on that sample.  Nothing is measured against the code under test.

Measured on an MI355X (gfx950) by the first run of this file, 19 tests in 11 s; the float32 column is that machine's CPU.  No kind
needed a factor above 4 (FACTORS is empty).  Largest ratio of every run: eval tiny 3.07, one_frame 2.11, s64 2.21, s65 2.38, dec64
2.73, m128_enc 2.65 (the same on the grouped GEMM alone), m128_dec 2.24, short_max 3.30; training mode tiny 1.67, s65 1.65, m128_enc
2.20; the life-cycle runs 1.89 - 3.07.  The worst (sample, part) pair of a run sits at 0.23 - 0.97 of its ceiling (0.97: short_max, 0.96:
tiny -- the q bias of a self-attention, a near-cancelling column sum, on both sides); key-bias parts are within 6e-8 S_b of the reference
(allowed 1e-5).  Forward outputs: 6e-7 .. 1e-6, at most 2.8 x the float32 reference's.  Per kind for short_max in eval mode, the case
with the largest ratio (e = worst over samples and layers of max|got - ref64| / max|ref64 part|; ceiling 1.54e-5):

    kind                                               e_hip      e_tw  ratio
    encoder.layer.self_attn.in_proj_bias.q          5.43e-06  1.64e-06   3.30
    decoder.layer.self_attn.in_proj_bias.q          1.49e-05  5.12e-06   2.91
    decoder.layer.self_attn.in_proj_weight.q        1.22e-05  4.60e-06   2.65
    decoder.layer.self_attn.in_proj_weight.k        7.59e-06  2.96e-06   2.57
    encoder.layer.self_attn.in_proj_weight.q        3.45e-06  1.67e-06   2.07
    global_motion_token                             1.15e-06  6.49e-07   1.77
    query_pos_encoder.pe                            1.15e-06  6.49e-07   1.77
    encoder.layer.linear2.bias                      1.10e-06  6.39e-07   1.72
    encoder.layer.self_attn.in_proj_weight.k        3.01e-06  1.79e-06   1.68
    encoder.layer.self_attn.out_proj.bias           1.23e-06  7.53e-07   1.63
    encoder.layer.self_attn.out_proj.weight         1.27e-06  7.84e-07   1.62
    skel_embedding.bias                             1.27e-06  8.11e-07   1.57
    encoder.layer.norm1.weight                      1.65e-06  1.12e-06   1.48
    encoder.layer.linear1.weight                    1.20e-06  8.10e-07   1.48
    encoder.layer.self_attn.in_proj_bias.v          1.12e-06  7.76e-07   1.44
    encoder.layer.norm1.bias                        1.36e-06  9.59e-07   1.42
    encoder.layer.linear2.weight                    1.19e-06  8.43e-07   1.41
    encoder.layer.norm2.bias                        8.55e-07  6.14e-07   1.39
    encoder.norm.weight                             8.85e-07  6.46e-07   1.37
    decoder.norm.weight                             7.70e-07  5.64e-07   1.37
    final_layer.weight                              5.48e-07  4.14e-07   1.32
    decoder.layer.norm2.bias                        9.99e-07  7.60e-07   1.31
    encoder.linear_blocks.weight                    7.83e-07  5.98e-07   1.31
    skel_embedding.weight                           1.07e-06  8.37e-07   1.27
    decoder.layer.multihead_attn.out_proj.weight    1.07e-06  8.80e-07   1.22
    decoder.layer.multihead_attn.in_proj_weight.v   1.09e-06  9.11e-07   1.20
    encoder.layer.self_attn.in_proj_weight.v        1.16e-06  9.73e-07   1.19
    decoder.layer.multihead_attn.in_proj_bias.v     1.08e-06  9.13e-07   1.19
    decoder.linear_blocks.weight                    9.22e-07  7.85e-07   1.18
    decoder.layer.self_attn.out_proj.bias           9.98e-07  8.52e-07   1.17
    decoder.layer.norm3.weight                      1.08e-06  9.25e-07   1.16
    decoder.linear_blocks.bias                      6.98e-07  6.11e-07   1.14
    decoder.layer.norm3.bias                        8.76e-07  7.85e-07   1.12
    decoder.layer.multihead_attn.out_proj.bias      9.44e-07  8.74e-07   1.08
    decoder.layer.norm1.bias                        9.44e-07  8.74e-07   1.08
    encoder.linear_blocks.bias                      5.98e-07  5.56e-07   1.08
    decoder.layer.linear2.weight                    8.80e-07  8.20e-07   1.07
    decoder.layer.norm2.weight                      8.70e-07  8.17e-07   1.06
    encoder.layer.linear1.bias                      1.07e-06  1.01e-06   1.06
    decoder.layer.linear2.bias                      8.25e-07  7.87e-07   1.05
    decoder.dz                                      6.96e-07  6.72e-07   1.04
    decoder.layer.self_attn.out_proj.weight         9.03e-07  8.77e-07   1.03
    encoder.norm.bias                               5.69e-08  5.69e-08   1.00
    final_layer.bias                                8.76e-08  8.76e-08   1.00
    decoder.layer.self_attn.in_proj_bias.v          8.43e-07  8.63e-07   0.98
    query_pos_decoder.pe                            6.86e-07  7.06e-07   0.97
    decoder.layer.linear1.weight                    1.41e-06  1.49e-06   0.95
    decoder.layer.linear1.bias                      1.33e-06  1.45e-06   0.92
    encoder.layer.norm2.weight                      8.81e-07  9.63e-07   0.92
    decoder.layer.self_attn.in_proj_weight.v        8.73e-07  9.79e-07   0.89
    decoder.layer.norm1.weight                      8.24e-07  1.05e-06   0.79
    decoder.norm.bias                               2.72e-07  3.48e-07   0.78
    forward sample 0: mu 8.6e-07 / 6.2e-07  logvar 6.7e-07 / 5.6e-07  feats 7.2e-07 / 5.2e-07
    forward sample 1: mu 7.3e-07 / 5.0e-07  logvar 7.7e-07 / 5.7e-07  feats 8.2e-07 / 6.6e-07  feats_pad 6.0e-07 / 3.8e-07
"""
import contextlib

import pytest
import torch

import vae_train_reference as R

pytestmark = pytest.mark.gpu
P = R.P_DROP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


class Rig:
    def __init__(self, dev):
        self.dev, self._vae, self._params, self._cases = dev, {}, {}, {}

    def vae(self, F, fresh=False):
        """The recipe VAE with F features on the device (one per F; `fresh`: one of its own)."""
        if fresh or F not in self._vae:
            vae, sd = R.recipe_state(F)
            self._params[F] = (R.params_of(sd, torch.float64), R.params_of(sd, torch.float32))
            vae = vae.to(self.dev).eval()
            if fresh:
                return vae
            self._vae[F] = vae
        return self._vae[F]

    def params(self, F):
        self.vae(F)
        return self._params[F]


@pytest.fixture(scope="module")
def rig(dev):
    return Rig(dev)


# ----------------------------------------------------------------------------- the driver
@contextlib.contextmanager
def spy_calls():
    """Record the entry names that go through seeme_amd._lib.call."""
    from seeme_amd import _lib as L
    names, orig = [], L.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    L.call = call
    try:
        yield names
    finally:
        L.call = orig


def to_dev(inp, dev):
    return {k: inp[k].to(dev) for k in ("features", "z", "ddist", "dfeats")}


def set_grads(vae, fill=None):
    """Zero every existing .grad in place, or (fill: {name: tensor}) copy a fixed tensor into it, creating it where there is none."""
    for k, p in vae.named_parameters():
        if fill is not None:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            p.grad.copy_(fill[k])
        elif p.grad is not None:
            p.grad.zero_()


def forward(tr, d, lengths, names=None):
    z = d["z"][None].clone().requires_grad_(True)
    n0 = 0 if names is None else len(names)
    mu, logvar = tr.encode(d["features"], lengths)
    n1 = 0 if names is None else len(names)
    feats = tr.decode(z, lengths)
    split = None if names is None else (names[n0:n1], names[n1:])
    return dict(z=z, mu=mu, logvar=logvar, feats=feats, calls=split)


def backward(d, fw, sel):
    """Backward with the upstream gradient zero outside the samples `sel`."""
    dd, df = torch.zeros_like(d["ddist"]), torch.zeros_like(d["dfeats"])
    dd[:, sel], df[sel] = d["ddist"][:, sel], d["dfeats"][sel]
    ((fw["mu"][0] * dd[0]).sum() + (fw["logvar"][0] * dd[1]).sum() + (fw["feats"] * df).sum()).backward()
    torch.cuda.synchronize()


def plan_masks(tr, dec, B, T):
    """The keep-masks the plan drew in its last forward, batched: {"<layer>.<site>": uint8 on the CPU}."""
    plan = tr.plans[(dec, B, T, P)]
    return {f"{l}.{k}": sv[k].clone().cpu() for l, sv in enumerate(plan.sv) for k in (R.DEC_SITES if dec else R.ENC_SITES)}


def read_grads(vae):
    return {k: p.grad.detach().cpu().clone() for k, p in vae.named_parameters()}


def result_of(fw, grads, b, entry=None, scale=1.0):
    """Sample b of a step in the layout of vae_train_reference.sample_result; the parameter gradients are grads minus `entry` (what
    .grad held before), times scale; dz is that of the step `fw`."""
    g = {k: (v.double() - (0 if entry is None else entry[k].cpu().double())) * scale for k, v in grads.items()}
    res = dict(mu=fw["mu"][0, b].detach().cpu(), logvar=fw["logvar"][0, b].detach().cpu(), feats=fw["feats"][b].detach().cpu())
    for key, dec in (("enc", False), ("dec", True)):
        res[key] = dict(pt for k in R.stack_keys(g, dec) for pt in R.split_parts(k, g[k]))
    res["dec"]["decoder.dz"] = fw["z"].grad[0, b].detach().cpu().double()
    return res


def steps_per_sample(tr, vae, inp, d, train=False, fill=None, names=None):
    """One step per sample b (upstream gradient on b alone).  -> (results, masks_e, masks_d, raw grads, forwards)."""
    B, T, Td, lengths = inp["B"], inp["T"], inp["Td"], inp["lengths"]
    vae.train(train)
    got, me, md, raw, fws = [], ([] if train else None), ([] if train else None), [], []
    try:
        for b in range(B):
            set_grads(vae, fill)
            fw = forward(tr, d, lengths, names)
            if train:
                e, dm = plan_masks(tr, False, B, T), plan_masks(tr, True, B, Td)
                keep = float(torch.cat([m.float().flatten() for m in list(e.values()) + list(dm.values())]).mean())
                assert abs(keep - (1 - P)) < 0.01, keep
                me.append(R.slice_masks(e, b, B))
                md.append(R.slice_masks(dm, b, B))
            backward(d, fw, [b])
            raw.append(read_grads(vae))
            got.append(result_of(fw, raw[-1], b, fill))
            fws.append(fw)
    finally:
        vae.eval()
    return got, me, md, raw, fws


def twin(rig, inp, me=None, md=None, fill=None):
    """(float64 reference per sample, float32 reference compared with it).  `fill`: the float32 run accumulates its gradients into
    these float32 tensors too and is read back as the difference, as the device's .grad is."""
    P64, P32 = rig.params(inp["F"])
    r64, r32 = R.per_sample(P64, inp, me, md), R.per_sample(P32, inp, me, md)
    if fill is not None:
        parts = {}
        for k, v in fill.items():
            parts.update(R.split_parts(k, v.cpu()))
        for r in r32:
            for key in ("enc", "dec"):
                for part, g in r[key].items():
                    if part in parts:
                        r[key][part] = (parts[part] + g).double() - parts[part].double()
    return r64, R.compare(r32, r64, inp["lengths"], md)


def check(name, rig, inp, got, raw, me=None, md=None, fill=None):
    """The per-sample assertions of one run: bounds from the float32 reference, zero parts bit-equal to the entry value."""
    r64, tw = twin(rig, inp, me, md, fill)
    hip = R.compare(got, r64, inp["lengths"], md)
    print("\n" + R.format_table(name, tw, hip))
    lows = [e for _, _, e in hip["low"]]
    print(f"{name}: key-bias parts, worst |got - ref64| / S_b = {max(lows):.2e}; exactly-zero parts per sample {[len(x) for x in hip['exact']]}")
    for b, parts in enumerate(hip["exact"]):
        entry = {}
        for k in raw[b]:
            entry.update(R.split_parts(k, torch.zeros_like(raw[b][k]) if fill is None else fill[k].cpu()))
        have = {}
        for k, v in raw[b].items():
            have.update(R.split_parts(k, v))
        for part in parts:
            assert torch.equal(have[part].contiguous().view(torch.int32), entry[part].contiguous().view(torch.int32)), (b, part)
    bad = R.violations(hip, R.bounds(tw))
    assert not bad, bad
    return hip, tw


def run_case(rig, name, train):
    key = (name, train)
    if key not in rig._cases:
        from seeme_amd.vae_train import VaeTrainer
        inp = R.case_inputs(name)
        vae = rig.vae(inp["F"])
        torch.manual_seed(1000 + R.CASES[name]["seed"])
        with spy_calls() as names:
            got, me, md, raw, fws = steps_per_sample(VaeTrainer(vae), vae, inp, to_dev(inp, rig.dev), train, names=names)
        rig._cases[key] = dict(inp=inp, got=got, me=me, md=md, raw=raw, names=list(names), calls=fws[0]["calls"])
    return rig._cases[key]


# ----------------------------------------------------------------------------- accuracy per sample, every case and mode
@pytest.mark.parametrize("name,train", [(n, False) for n in R.CASES] + [(n, True) for n in R.DROPOUT_CASES])
def test_per_sample_against_float64(rig, name, train):
    c = run_case(rig, name, train)
    inp = c["inp"]
    # the case reached the kernels it was chosen for
    enc_calls, dec_calls = c["calls"]
    assert "seeme_grouped_gemm" in c["names"] and "seeme_wgrad128" in c["names"]
    if name == "tiny":
        assert "seeme_gemm128" not in c["names"]
    if name == "m128_enc":
        assert inp["B"] * (inp["T"] + 2) == 128 and "seeme_gemm128" in enc_calls and "seeme_gemm128" not in dec_calls
    if name == "m128_dec":
        assert inp["B"] * inp["Td"] == 128 and "seeme_gemm128" in dec_calls and "seeme_gemm128" not in enc_calls
    if train:
        assert "seeme_vt_dropout" in c["names"] and "seeme_vt_cross_rows" in c["names"]
    check(f"{name} {'train' if train else 'eval'}", rig, inp, c["got"], c["raw"], c["me"], c["md"])


def test_both_gemm_paths_agree_with_the_reference(rig, monkeypatch):
    """SEEME_GEMM128=0 puts every projection of m128_enc on the grouped GEMM: the same bounds hold (the path assertion of the case
    itself is the primary check)."""
    from seeme_amd.vae_train import VaeTrainer
    monkeypatch.setenv("SEEME_GEMM128", "0")
    inp = R.case_inputs("m128_enc")
    vae = rig.vae(inp["F"])
    with spy_calls() as names:
        got, _, _, raw, _ = steps_per_sample(VaeTrainer(vae), vae, inp, to_dev(inp, rig.dev))
    assert "seeme_gemm128" not in names and "seeme_wgrad128" not in names and "seeme_grouped_gemm" in names
    check("m128_enc on the grouped GEMM alone", rig, inp, got, raw)


# ----------------------------------------------------------------------------- the plan life cycle, on `tiny`
def _fill(vae, seed, scale=1e-2):
    g = torch.Generator().manual_seed(seed)
    return {k: (scale * torch.randn(p.shape, generator=g)).to(p.device) for k, p in vae.named_parameters()}


def test_accumulation_into_prefilled_grads(rig):
    """.grad pre-filled with a fixed non-zero g0: .grad - g0 is the gradient (the float32 reference accumulates into g0 the same way, so
    the one more rounding is on both sides of the 4x rule); slices the backward never writes equal g0 bitwise (check's zero parts)."""
    from seeme_amd.vae_train import VaeTrainer
    inp = R.case_inputs("tiny")
    vae = rig.vae(inp["F"])
    g0 = _fill(vae, 31)
    got, _, _, raw, _ = steps_per_sample(VaeTrainer(vae), vae, inp, to_dev(inp, rig.dev), fill=g0)
    check("tiny, .grad = g0 on entry", rig, inp, got, raw, fill=g0)


def test_two_backward_passes_sum(rig):
    from seeme_amd.vae_train import VaeTrainer
    inp = R.case_inputs("tiny")
    vae, d = rig.vae(inp["F"]), to_dev(inp, rig.dev)
    tr = VaeTrainer(vae)
    got, raw = [], []
    for b in range(inp["B"]):
        set_grads(vae)
        for _ in range(2):
            fw = forward(tr, d, inp["lengths"])
            backward(d, fw, [b])
        raw.append(read_grads(vae))
        got.append(result_of(fw, raw[-1], b, scale=0.5))
    assert len(tr.plans) == 2
    check("tiny, two steps without zeroing, halved", rig, inp, got, raw)


def test_second_forward_before_the_first_backward(rig):
    """The busy branch: two forwards on different inputs, then each backward matches its own inputs; a third forward reuses a plan."""
    from seeme_amd.vae_train import VaeTrainer
    inp_a = R.case_inputs("tiny")
    inp_b = R.make_inputs(**dict(R.CASES["tiny"], seed=131))
    vae = rig.vae(inp_a["F"])
    da, db = to_dev(inp_a, rig.dev), to_dev(inp_b, rig.dev)
    tr = VaeTrainer(vae)
    B, T, lengths = inp_a["B"], inp_a["T"], inp_a["lengths"]
    ga, gb, ra, rb = [], [], [], []
    for b in range(B):
        fa = forward(tr, da, lengths)
        plan_a = tr.plans[(False, B, T, 0.0)]
        fb = forward(tr, db, lengths)
        plan_b = tr.plans[(False, B, T, 0.0)]
        assert plan_a is not plan_b and plan_a.busy and plan_b.busy and len(tr.plans) == 2
        set_grads(vae)
        backward(da, fa, [b])
        ra.append(read_grads(vae))
        ga.append(result_of(fa, ra[-1], b))
        set_grads(vae)
        backward(db, fb, [b])
        rb.append(read_grads(vae))
        gb.append(result_of(fb, rb[-1], b))
        assert not plan_a.busy and not plan_b.busy
        forward(tr, da, lengths)                             # a third forward: the plan in the cache, no new one
        assert tr.plans[(False, B, T, 0.0)] is plan_b and len(tr.plans) == 2
        for p in tr.plans.values():                          # (its backward is not run: free the plans for the next round)
            p.busy = False
    check("tiny, first of two forwards in flight", rig, inp_a, ga, ra)
    check("tiny, second of two forwards in flight", rig, inp_b, gb, rb)


def test_rerecord_after_grads_were_replaced(rig):
    from seeme_amd.vae_train import VaeTrainer
    inp = R.case_inputs("tiny")
    vae, d = rig.vae(inp["F"]), to_dev(inp, rig.dev)
    tr = VaeTrainer(vae)
    got, raw = [], []
    for b in range(inp["B"]):
        set_grads(vae)
        fw = forward(tr, d, inp["lengths"])
        backward(d, fw, [b])
        old = {k: p.grad for k, p in vae.named_parameters()}
        before = {k: v.clone() for k, v in old.items()}
        key = tr.plans[(True, inp["B"], inp["Td"], 0.0)]._bwd_key
        for p in vae.parameters():
            p.grad = None
        fw = forward(tr, d, inp["lengths"])
        backward(d, fw, [b])
        assert tr.plans[(True, inp["B"], inp["Td"], 0.0)]._bwd_key != key and len(tr.plans) == 2
        for k, p in vae.named_parameters():
            assert p.grad is not old[k] and p.grad.data_ptr() != old[k].data_ptr(), k
            assert torch.equal(old[k].view(torch.int32), before[k].view(torch.int32)), k
        raw.append(read_grads(vae))
        got.append(result_of(fw, raw[-1], b))
    check("tiny, re-recorded backward", rig, inp, got, raw)


def test_recorded_plan_with_other_lengths(rig):
    from seeme_amd.vae_train import VaeTrainer
    inp_a = R.case_inputs("tiny")
    inp_b = R.make_inputs(**dict(R.CASES["tiny"], lengths=[2, 5, 4], seed=141))
    vae = rig.vae(inp_a["F"])
    tr = VaeTrainer(vae)
    for tag, inp in (("5, 1, 3", inp_a), ("2, 5, 4", inp_b), ("5, 1, 3 again", inp_a)):
        got, _, _, raw, _ = steps_per_sample(tr, vae, inp, to_dev(inp, rig.dev))
        assert len(tr.plans) == 2
        check("tiny, one trainer, lengths " + tag, rig, inp, got, raw)


def test_eviction_beyond_eight_plans(rig):
    """Nine distinct T at B = 1 (two plans each), then the first again: at most 8 plans are kept and every result is right."""
    from seeme_amd.vae_train import VaeTrainer
    vae = rig.vae(75)
    tr = VaeTrainer(vae)
    for i, T in enumerate(list(range(1, 10)) + [1]):
        inp = R.make_inputs(F=75, B=1, T=T, lengths=[T], pad_dfeats=False, seed=150 + T)
        got, _, _, raw, _ = steps_per_sample(tr, vae, inp, to_dev(inp, rig.dev))
        assert len(tr.plans) == min(2 * (i + 1), 8) and (True, 1, T, 0.0) in tr.plans
        check(f"B = 1, T = {T}, plan {i}", rig, inp, got, raw)
    assert (False, 1, 2, 0.0) not in tr.plans


def test_stale_trainer_is_rebuilt(rig):
    from seeme_amd.vae_train import VaeTrainer
    from test_gpu_flows import _mld
    vae = rig.vae(75, fresh=True)
    tr = VaeTrainer(vae)
    assert not tr.stale()
    vae.final_layer.bias = torch.nn.Parameter(vae.final_layer.bias.detach().clone())
    assert tr.stale()
    model = _mld(rig.dev, "config_vae_egobody.yaml")[0]
    t1 = model._vae_trainer(16)
    assert t1 is not None and model._vae_trainer(16) is t1
    lin = model.vae.encoder.linear_blocks[0]
    lin.weight = torch.nn.Parameter(lin.weight.detach().clone())
    assert t1.stale()
    t2 = model._vae_trainer(16)
    assert t2 is not t1 and not t2.stale() and model._vae_trainer(16) is t2
