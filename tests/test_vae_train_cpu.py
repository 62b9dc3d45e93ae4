"""The float64 twin of the stage-1 VAE forward / backward (tests/vae_train_reference.py) pinned on the CPU, before the device test
(tests/test_gpu_vae_train.py) holds seeme_amd/vae_train.py to it: its forward equals the numpy oracle and the autograd twin in
float64, its per-sample gradients summed over the batch equal float64 autograd through vae_autograd.py for every named parameter
(injected keep-masks included) and a directional finite difference, the three mistakes the device test is there to catch (a length one
off, an upstream gradient attributed to the neighbouring sample, a keep-mask shifted by one element) each move the reference's own
result by at least 10 times what the device test allows, and the float32-versus-float64 errors e_tw that set the device test's
bounds are computed and printed per kind and case."""
import copy

import pytest
import torch

import vae_train_reference as R

LOUD = 10.0
MASK_SEEDS = {"tiny": (7, 8), "s65": (17, 18), "m128_enc": (27, 28)}     # (encoder, decoder) keep-mask seeds of the dropout cases
MODES = [(n, False) for n in R.CASES] + [(n, True) for n in R.DROPOUT_CASES]


class Ctx:
    def __init__(self):
        self._f, self._case = {}, {}

    def model(self, F):
        """(float64 MldVae module, float64 params, float32 params, numpy float64 params) of the recipe VAE with F features."""
        if F not in self._f:
            vae, sd = R.recipe_state(F)
            self._f[F] = (copy.deepcopy(vae).double().eval(), R.params_of(sd, torch.float64), R.params_of(sd, torch.float32),
                          {k: v.double().numpy() for k, v in sd.items() if torch.is_floating_point(v)})
        return self._f[F]

    def masks(self, name, inp):
        se, sd = MASK_SEEDS[name]
        return R.make_masks(False, inp["B"], inp["T"] + 2, se), R.make_masks(True, inp["B"], inp["Td"], sd)

    def case(self, name, masked):
        """inputs, masks, the float64 and float32 per-sample results, the float32 errors and the bounds they set."""
        if (name, masked) not in self._case:
            inp = R.case_inputs(name)
            _, P64, P32, _ = self.model(inp["F"])
            me, md = self.masks(name, inp) if masked else (None, None)
            r64, r32 = R.per_sample(P64, inp, me, md), R.per_sample(P32, inp, me, md)
            tw = R.compare(r32, r64, inp["lengths"], md)
            self._case[(name, masked)] = dict(inp=inp, me=me, md=md, r64=r64, tw=tw, bnd=R.bounds(tw))
        return self._case[(name, masked)]


@pytest.fixture(scope="module")
def ctx():
    torch.manual_seed(0)
    return Ctx()


def _trunc(inp):
    """The case with the encoder's frames cut to max(lengths): what the oracle and the autograd twin take (they build their key mask
    from max(lengths)); the reference gives the same with the padded frames in place (test_padded_frames_do_not_matter)."""
    return dict(inp, T=inp["Td"], features=inp["features"][:, :inp["Td"]].contiguous())


def _forward64(P64, inp, me=None, md=None):
    mu, lv, feats = [], [], []
    with torch.no_grad():
        for b, n in enumerate(inp["lengths"]):
            o = R.encode_sample(P64, inp["features"][b].double(), n, None if me is None else me[b])
            mu.append(o[0]), lv.append(o[1])
            feats.append(R.decode_sample(P64, inp["z"][b].double(), inp["Td"], n, None if md is None else md[b]))
    return torch.stack(mu), torch.stack(lv), torch.stack(feats)


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_equals_the_oracle_and_the_autograd_twin(ctx, name):
    from oracle import mld_oracle as O
    from seeme_amd.vae_autograd import vae_decode_torch, vae_encode_torch
    inp = _trunc(R.case_inputs(name))
    vae64, P64, _, Pnp = ctx.model(inp["F"])
    mu, lv, feats = _forward64(P64, inp)
    omu, ostd = O.vae_encode(Pnp, inp["features"].double().numpy(), inp["lengths"])
    ofeats = O.vae_decode(Pnp, inp["z"][None].double().numpy(), inp["lengths"])
    with torch.no_grad():
        tmu, tstd = vae_encode_torch(vae64, inp["features"].double(), inp["lengths"])
        tfeats = vae_decode_torch(vae64, inp["z"][None].double(), inp["lengths"])
    errs = {"mu/oracle": R.relmax(mu, torch.from_numpy(omu[0])), "logvar/oracle": R.relmax(lv, 2 * torch.from_numpy(ostd[0]).log()),
            "feats/oracle": R.relmax(feats, torch.from_numpy(ofeats)), "mu/twin": R.relmax(mu, tmu[0]),
            "logvar/twin": R.relmax(lv, 2 * tstd[0].log()), "feats/twin": R.relmax(feats, tfeats)}
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("name", R.DROPOUT_CASES)
def test_forward_with_masks_equals_the_autograd_twin(ctx, name):
    from seeme_amd.vae_autograd import vae_decode_torch, vae_encode_torch
    inp = _trunc(R.case_inputs(name))
    vae64, P64, _, _ = ctx.model(inp["F"])
    assert float(vae64.encoder.input_blocks[0].self_attn.dropout) == R.P_DROP
    me, md = ctx.masks(name, inp)
    mu, lv, feats = _forward64(P64, inp, me, md)
    with torch.no_grad():
        tmu, tstd = vae_encode_torch(vae64, inp["features"].double(), inp["lengths"], masks=R.batch_masks(me))
        tfeats = vae_decode_torch(vae64, inp["z"][None].double(), inp["lengths"], masks=R.batch_masks(md))
        plain = _forward64(P64, inp)
    errs = [R.relmax(mu, tmu[0]), R.relmax(lv, 2 * tstd[0].log()), R.relmax(feats, tfeats)]
    assert max(errs) <= 1e-12, errs
    assert R.relmax(mu, plain[0]) > 1e-2 and R.relmax(feats, plain[2]) > 1e-2          # ... and the masks do change the forward


@pytest.mark.parametrize("name", ["tiny", "s65", "short_max"])
def test_padded_frames_do_not_matter(ctx, name):
    """Frames behind a sample's length are no keys: their values (1e3 times the valid ones), or cutting them off, change nothing
    of mu, logvar and the gradients -- in float64 up to the summation order of the matrix products."""
    inp = R.case_inputs(name)
    _, P64, _, _ = ctx.model(inp["F"])
    other = dict(inp, features=inp["features"].clone())
    for b, n in enumerate(inp["lengths"]):
        other["features"][b, n:] = 0.0
    for b, n in enumerate(inp["lengths"]):
        a, c, t = R.sample_result(P64, inp, b), R.sample_result(P64, other, b), R.sample_result(P64, _trunc(inp), b)
        pe = "query_pos_encoder.pe"                                    # (longer by the cut rows, which are zero)
        assert not bool(a["enc"][pe][inp["Td"] + 2:].any())
        for r in (c, t):
            assert R.relmax(r["mu"], a["mu"]) <= 1e-12 and R.relmax(r["logvar"], a["logvar"]) <= 1e-12
            for part, g in a["enc"].items():
                if float(g.abs().max()) > 0:
                    assert R.relmax(r["enc"][part], g) <= 1e-10, (b, part)


# ----------------------------------------------------------------------------- gradients
def test_zero_part_counts():
    P = R.params_of(R.recipe_state(75)[1], torch.float64)
    ne = sum(len(R.split_parts(k, P[k])) for k in R.stack_keys(P, False))
    nd = sum(len(R.split_parts(k, P[k])) for k in R.stack_keys(P, True)) + 1          # + dz
    assert (ne, nd) == (90, 140)
    for dec, n, want in ((False, 1, 5), (False, 9, 5), (True, 9, 25), (True, 1, 40)):
        keyb, exact = R.zero_parts(dec, n)
        assert len(keyb) == 5 and len(keyb | exact) == want and not keyb & exact
    assert R.kind_of("decoder.output_blocks.1.self_attn.in_proj_bias.k") == "decoder.layer.self_attn.in_proj_bias.k"
    assert R.kind_of("encoder.middle_block.norm2.weight") == R.kind_of("encoder.input_blocks.0.norm2.weight") == "encoder.layer.norm2.weight"
    assert R.kind_of("encoder.linear_blocks.1.weight") == "encoder.linear_blocks.weight" and R.kind_of("final_layer.bias") == "final_layer.bias"
    assert all(4 < f <= 16 for f in R.FACTORS.values())


@pytest.mark.parametrize("name,masked", MODES)
def test_per_sample_gradients_sum_to_autograd_and_a_finite_difference(ctx, name, masked):
    from seeme_amd.vae_autograd import vae_decode_torch, vae_encode_torch
    inp = _trunc(R.case_inputs(name))
    vae64, P64, _, _ = ctx.model(inp["F"])
    me, md = ctx.masks(name, inp) if masked else (None, None)
    named = dict(vae64.named_parameters())
    for p in named.values():
        p.grad = None
    z = inp["z"][None].double().clone().requires_grad_(True)
    dd, df = inp["ddist"].double(), inp["dfeats"].double()
    mu, std = vae_encode_torch(vae64, inp["features"].double(), inp["lengths"], masks=None if me is None else R.batch_masks(me))
    feats = vae_decode_torch(vae64, z, inp["lengths"], masks=None if md is None else R.batch_masks(md))
    ((mu[0] * dd[0]).sum() + (2 * std[0].log() * dd[1]).sum() + (feats * df).sum()).backward()
    want = {k: p.grad.clone() for k, p in named.items()}
    for p in named.values():
        p.grad = None
    per = R.per_sample(P64, inp, me, md)
    got = {}
    for k in want:
        key = "dec" if k in R.stack_keys(P64, True) else "enc"
        if k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            got[k] = sum(torch.cat([r[key][k + ".q"], r[key][k + ".k"], r[key][k + ".v"]]) for r in per)
        else:
            got[k] = sum(r[key][k] for r in per)
    gmax = max(float(v.abs().max()) for v in want.values())
    errs = sorted(((float((got[k] - w).abs().max()) / max(float(w.abs().max()), 1e-4 * gmax), k) for k, w in want.items()), reverse=True)
    edz = R.relmax(torch.stack([r["dec"]["decoder.dz"] for r in per]), z.grad[0])
    print(f"{name} masks={masked}: summed per-sample gradients vs autograd through the twin, worst {errs[0][0]:.1e} at {errs[0][1]}; dz {edz:.1e}")
    assert set(want) == set(R.stack_keys(P64, False)) | set(R.stack_keys(P64, True))
    assert errs[0][0] <= 1e-10 and edz <= 1e-10, (errs[:4], edz)

    # one directional finite difference of the batch loss through the reference itself
    g = torch.Generator().manual_seed(R.CASES[name]["seed"])
    dirs = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) * float(v.abs().max()) for k, v in P64.items() if k in want}
    dz = torch.randn(inp["B"], 256, generator=g, dtype=torch.float64)

    def loss(h):
        Ph = dict(P64)
        Ph.update({k: P64[k] + h * d for k, d in dirs.items()})
        ih = dict(inp, z=inp["z"].double() + h * dz)
        m, lv, f = _forward64(Ph, ih, me, md)
        return float((m * dd[0]).sum() + (lv * dd[1]).sum() + (f * df).sum())
    h = 1e-6
    fd = (loss(h) - loss(-h)) / (2 * h)
    an = float(sum((got[k] * d).sum() for k, d in dirs.items()) + sum((r["dec"]["decoder.dz"] * dz[b]).sum() for b, r in enumerate(per)))
    print(f"{name} masks={masked}: directional derivative {an:.6e}, central difference {fd:.6e}")
    assert abs(fd - an) <= 1e-6 * abs(an), (fd, an)


# ----------------------------------------------------------------------------- calibration: the float32 reference's own error
@pytest.mark.parametrize("name,masked", MODES)
def test_float32_yardstick_table(ctx, name, masked):
    """e_tw per kind, the table the device test's bounds are taken from (vae_train_reference.bounds): 4 x per kind, every pair under 3 x
    the worst kind of the case.  compare() asserts on the way that the zero parts are the listed ones and no others."""
    c = ctx.case(name, masked)
    print("\n" + R.format_table(f"{name} {'with keep-masks' if masked else 'eval'}", c["tw"]))
    worst = max(e for e, _ in c["tw"]["kind"].values())
    # 23 encoder + 29 decoder kinds (dz among them) have a non-zero part; three fewer where every decoder sample has one frame
    assert len(c["tw"]["kind"]) == (49 if max(c["inp"]["lengths"]) == 1 else 52) and 1e-7 < worst < 1e-3, worst
    assert all(e <= R.TOL_F32 for f in c["tw"]["fwd"] for e in f.values())
    assert all(e <= R.FLOOR_ABS for _, _, e in c["tw"]["low"])
    assert not R.violations(c["tw"], c["bnd"])                             # (the yardstick is inside its own bounds)


# ----------------------------------------------------------------------------- sensitivity: what the device test would not let pass
def _is_dec(kind):
    return kind.startswith(("decoder.", "final_layer.", "query_pos_decoder."))


def _loud(res, bnd, fwd=True):
    """(encoder side, decoder side): the largest error in units of what the device test allows for it."""
    e = [x / max(bnd["kind"][k], 1e-300) for k, (x, _) in res["kind"].items() if not _is_dec(k)]
    d = [x / max(bnd["kind"][k], 1e-300) for k, (x, _) in res["kind"].items() if _is_dec(k)]
    if fwd:
        for f, fb in zip(res["fwd"], bnd["fwd"]):
            e += [f[k] / fb[k] for k in ("mu", "logvar")]
            d += [f[k] / fb[k] for k in f if k.startswith("feats")]
    return max(e), max(d)


def _swap(r64, b, new):
    out = list(r64)
    out[b] = dict(r64[b], **new)
    return out


@pytest.mark.parametrize("name,masked", MODES)
def test_a_length_one_off_is_loud(ctx, name, masked):
    c = ctx.case(name, masked)
    inp, r64 = c["inp"], c["r64"]
    _, P64, _, _ = ctx.model(inp["F"])
    for b, n in enumerate(inp["lengths"]):
        n2 = n + 1 if n < inp["Td"] else n - 1
        me, md = (None, None) if c["me"] is None else (c["me"][b], c["md"][b])
        # a decoder sample of no frame does not exist (no key at all): at T = 1 only the encoder's length can be one off
        stacks = ("enc", "dec") if n2 > 0 else ("enc",)
        new = R.sample_result(P64, inp, b, me, md, length=n2, stacks=stacks)
        le, ld = _loud(R.compare(_swap(r64, b, new), r64, inp["lengths"], c["md"]), c["bnd"])
        print(f"{name} masks={masked}: sample {b} with {n2} for {n} frames: {le:.1e} (encoder) and {ld:.1e} (decoder) times the allowed error")
        assert le >= LOUD and (ld >= LOUD or "dec" not in stacks), (b, le, ld)


@pytest.mark.parametrize("name,masked", MODES)
def test_a_neighbours_upstream_gradient_is_loud(ctx, name, masked):
    c = ctx.case(name, masked)
    inp, r64 = c["inp"], c["r64"]
    _, P64, _, _ = ctx.model(inp["F"])
    for b in range(inp["B"]):
        a = (b - 1) % inp["B"]                                        # sample a's upstream gradient given to sample a + 1 = b
        me, md = (None, None) if c["me"] is None else (c["me"][b], c["md"][b])
        new = R.sample_result(P64, inp, b, me, md, ddist=inp["ddist"][:, a], dfeats=inp["dfeats"][a])
        le, ld = _loud(R.compare(_swap(r64, b, new), r64, inp["lengths"], c["md"]), c["bnd"], fwd=False)
        print(f"{name} masks={masked}: sample {b} with the upstream gradient of {a}: {le:.1e} (encoder) and {ld:.1e} (decoder) times the allowed error")
        assert le >= LOUD and ld >= LOUD, (b, le, ld)


@pytest.mark.parametrize("name", R.DROPOUT_CASES)
def test_a_keep_mask_shifted_by_one_element_is_loud(ctx, name):
    """Every site's batched mask of the middle layer, moved by one element (what a wrong slice offset does)."""
    c = ctx.case(name, True)
    inp, r64 = c["inp"], c["r64"]
    _, P64, _, _ = ctx.model(inp["F"])
    B = inp["B"]
    for dec, sites, per in ((False, R.ENC_SITES, c["me"]), (True, R.DEC_SITES, c["md"])):
        batched = R.batch_masks(per)
        for site in sites:
            k = f"2.{site}"
            moved = dict(batched)
            moved[k] = torch.roll(batched[k].reshape(-1), 1).reshape(batched[k].shape)
            assert not torch.equal(moved[k], batched[k])
            pert = []
            for b in range(B):
                m = R.slice_masks(moved, b, B)
                pert.append(dict(r64[b], **R.sample_result(P64, inp, b, m if not dec else c["me"][b], m if dec else c["md"][b],
                                                           stacks=("dec",) if dec else ("enc",))))
            le, ld = _loud(R.compare(pert, r64, inp["lengths"], c["md"]), c["bnd"])
            print(f"{name}: {'decoder' if dec else 'encoder'} {k} moved by one element: {ld if dec else le:.1e} times the allowed error")
            assert (ld if dec else le) >= LOUD, (dec, site, le, ld)
