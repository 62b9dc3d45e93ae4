"""Plain torch restatement of the denoiser's token-0 chain FROM ITS TABLES, for the tests of k_den_bwd (csrc/den_train.inc.hip).

One code path, run in float64 (the reference) and in float32 (the rounding yardstick of the 4x rule).  The arithmetic is
that of seeme_amd/denoiser_autograd._layer -- token-0 pruning, the ``sum_n (q.k_n) v_n`` form of the linear attention, dropout by
injected keep-masks at the DM_* offsets of csrc/den_train.h scaled by 1 / (1 - p) -- but the K|V rows of the condition and time
tokens, the linear attention's key|value rows and the AdaLN scale|shift rows are READ from ctab / ttab (include/seeme_hip.h,
denoiser_train._tables) instead of being computed, as the kernel reads them.  So the chain is checked apart from the table builders,
and the gradients of the tables are leaves' gradients.

Nothing here touches the device or the library; the model classes are imported only inside the helpers that build recipe inputs.
"""
import functools
import math

import torch
import torch.nn.functional as F

CROW, TROW = 5120, 7680                  # SEEME_CROW / SEEME_TROW
DM_LAYER, DM_TOTAL = 2192, 10960         # csrc/den_train.h
# dropout sites: byte offset inside a layer's mask block (DM_P, DM_1, DM_H, DM_2, DM_C, DM_F, DM_O)
SITES = {"P": 0, "1": 8, "H": 264, "2": 1288, "C": 1544, "F": 1800, "O": 1928}
LAYERS = ("encoder.input_blocks.0.", "encoder.input_blocks.1.", "encoder.middle_block.", "encoder.output_blocks.0.",
          "encoder.output_blocks.1.")
# the chain's linears, named as in denoiser_train._LIN: (weight key, bias key) below a layer's prefix
LINEARS = {"inp": ("sa_block.self_attn.in_proj_weight", "sa_block.self_attn.in_proj_bias"),
           "outp": ("sa_block.self_attn.out_proj.weight", "sa_block.self_attn.out_proj.bias"),
           "l1": ("sa_block.linear1.weight", "sa_block.linear1.bias"), "l2": ("sa_block.linear2.weight", "sa_block.linear2.bias"),
           "caq": ("ca_block.query.weight", "ca_block.query.bias"),
           "cao": ("ca_block.proj_out.out_layers.2.weight", "ca_block.proj_out.out_layers.2.bias"),
           "f1": ("ffn.linear1.weight", "ffn.linear1.bias"), "f2": ("ffn.linear2.weight", "ffn.linear2.bias"),
           "fo": ("ffn.proj_out.out_layers.2.weight", "ffn.proj_out.out_layers.2.bias")}
NORMS = ("sa_block.norm1", "sa_block.norm2", "ca_block.norm", "ca_block.proj_out.norm", "ffn.proj_out.norm")   # DB_LN order
RELU_MARGIN = 3e-5
FLOOR, FLOOR_ABS = 1e-4, 1e-5            # of S_b, the sample's largest gradient entry


def skip_keys(l):
    return f"encoder.linear_blocks.{l - 3}.weight", f"encoder.linear_blocks.{l - 3}.bias"


def chain_keys():
    """State-dict keys of every parameter the chain reads (query_pos.pe is reached through d noisy)."""
    keys = []
    for l, pre in enumerate(LAYERS):
        if l >= 3:
            keys += list(skip_keys(l))
        for wk, bk in LINEARS.values():
            keys += [pre + wk, pre + bk]
        for n in NORMS:
            keys += [pre + n + ".weight", pre + n + ".bias"]
    return keys + ["encoder.norm.weight", "encoder.norm.bias"]


def chain_params(den, dtype):
    """Detached copies of the chain's parameters (and query_pos.pe) of an MldDenoiser, on the CPU in `dtype`."""
    sd = den.state_dict()
    return {k: sd[k].detach().to("cpu", dtype).clone() for k in chain_keys() + ["query_pos.pe"]}


def _ln(x, P, pre):
    return F.layer_norm(x, (x.shape[-1],), P[pre + ".weight"], P[pre + ".bias"], 1e-5)


class _Drop:
    def __init__(self, masks, p):
        self.masks, self.scale, self.layer = masks, 1.0 / (1.0 - float(p)), 0

    def __call__(self, x, site):
        if self.masks is None:
            return x
        o = self.layer * DM_LAYER + SITES[site]
        return x * self.masks[:, o:o + x.shape[-1]].to(x.dtype) * self.scale


def _stylization(P, pre, h, scale, shift, drop, site):
    h = _ln(h, P, pre + "norm") * (1 + scale) + shift
    return F.linear(drop(F.silu(h), site), P[pre + "out_layers.2.weight"], P[pre + "out_layers.2.bias"])


def _layer(P, l, x, ctab, tt, drop, taps):
    """x [B,256]; ctab [B,N,5120]; tt [B,7680] (each sample's time row)."""
    pre, D = LAYERS[l], 256
    drop.layer = l
    sa, ca, ffn = pre + "sa_block.", pre + "ca_block.", pre + "ffn."
    w, b = P[sa + "self_attn.in_proj_weight"], P[sa + "self_attn.in_proj_bias"]
    q = F.linear(x, w[:D], b[:D])
    k0 = F.linear(x, w[D:2 * D], b[D:2 * D])
    v0 = F.linear(x, w[2 * D:], b[2 * D:])
    o = l * 512
    k = torch.cat([k0[:, None], ctab[:, :, o:o + D], tt[:, None, o:o + D]], dim=1)                  # [B,2+N,256]: self, conditions, time
    v = torch.cat([v0[:, None], ctab[:, :, o + D:o + 2 * D], tt[:, None, o + D:o + 2 * D]], dim=1)
    pw = torch.softmax((q[:, None] @ k.transpose(1, 2))[:, 0] / math.sqrt(D), dim=-1)              # token 0's row, one head
    att = (drop(pw, "P")[:, None] @ v)[:, 0]
    x = _ln(x + drop(F.linear(att, P[sa + "self_attn.out_proj.weight"], P[sa + "self_attn.out_proj.bias"]), "1"), P, sa + "norm1")
    z = F.linear(x, P[sa + "linear1.weight"], P[sa + "linear1.bias"])
    if taps is not None:
        taps.append(z.detach())
    x = _ln(x + drop(F.linear(drop(F.relu(z), "H"), P[sa + "linear2.weight"], P[sa + "linear2.bias"]), "2"), P, sa + "norm2")
    # linear cross-attention: keys | values of the condition tokens from the table
    qc = torch.softmax(F.linear(_ln(x, P, ca + "norm"), P[ca + "query.weight"], P[ca + "query.bias"]), dim=-1)
    o = 2560 + l * 512
    kc = torch.softmax(ctab[:, :, o:o + D], dim=1)
    vc = ctab[:, :, o + D:o + 2 * D]
    y = ((qc[:, None] * kc).sum(-1, keepdim=True) * vc).sum(1)                                     # sum_n (q.k_n) v_n
    o = 2560 + l * 1024
    x = x + _stylization(P, ca + "proj_out.", y, tt[:, o:o + D], tt[:, o + D:o + 2 * D], drop, "C")
    y = F.linear(drop(F.gelu(F.linear(x, P[ffn + "linear1.weight"], P[ffn + "linear1.bias"])), "F"),
                 P[ffn + "linear2.weight"], P[ffn + "linear2.bias"])
    return x + _stylization(P, ffn + "proj_out.", y, tt[:, o + 2 * D:o + 3 * D], tt[:, o + 3 * D:o + 4 * D], drop, "O")


def chain_from_tables(params, noisy, ctab, ttab, trow, masks, p_drop, taps=None):
    """noisy [B,256], ctab [B,N,5120], ttab [R,7680], trow [B] (row of ttab per sample), masks uint8 [B,10960] or None -> [B,256].
    `taps` (a list) collects the five sa_block.linear1 pre-activations."""
    tt = ttab.index_select(0, torch.as_tensor(trow, dtype=torch.long))
    drop = _Drop(masks, p_drop)
    x = noisy + params["query_pos.pe"][0, 0]
    xs = []
    for l in range(2):
        x = _layer(params, l, x, ctab, tt, drop, taps)
        xs.append(x)
    x = _layer(params, 2, x, ctab, tt, drop, taps)
    for l in (3, 4):
        wk, bk = skip_keys(l)
        x = F.linear(torch.cat([x, xs.pop()], dim=-1), params[wk], params[bk])
        x = _layer(params, l, x, ctab, tt, drop, taps)
    return _ln(x, params, "encoder.norm")


def iter_per_sample_grads(params, noisy, ctab, ttab, trow, masks, p_drop, dout):
    """For b = 0..B-1: (out[b], {chain parameter key: its gradient, "noisy": d noisy[b], "ctab": dctab[b] [N,5120], "ttab": the dttab
    row of sample b}) of sum(out[b] * dout[b]).  One forward and one backward per sample: the samples are independent."""
    keys = chain_keys()
    for b in range(noisy.shape[0]):
        leaves = {k: params[k].detach().clone().requires_grad_(True) for k in keys}
        leaves["query_pos.pe"] = params["query_pos.pe"]
        x = noisy[b:b + 1].detach().clone().requires_grad_(True)
        c = ctab[b:b + 1].detach().clone().requires_grad_(True)
        t = ttab.detach().clone().requires_grad_(True)
        out = chain_from_tables(leaves, x, c, t, [int(trow[b])], None if masks is None else masks[b:b + 1], p_drop)
        gs = torch.autograd.grad((out * dout[b:b + 1]).sum(), [leaves[k] for k in keys] + [x, c, t])
        g = dict(zip(keys, gs[:len(keys)]))
        g["noisy"], g["ctab"], g["ttab"] = gs[-3][0], gs[-2][0], gs[-1][int(trow[b])]
        yield out.detach()[0], g


def per_sample_grads(*args):
    return list(iter_per_sample_grads(*args))


def relu_margin(params, noisy, ctab, ttab, trow, masks, p_drop):
    """Per sample: the smallest |pre-activation| of sa_block.linear1 over the units its dropout keeps, over all five layers, each
    divided by that layer's largest |pre-activation|."""
    taps = []
    with torch.no_grad():
        chain_from_tables(params, noisy, ctab, ttab, trow, masks, p_drop, taps)
    m = torch.full((noisy.shape[0],), float("inf"), dtype=taps[0].dtype)
    for l, z in enumerate(taps):
        a = z.abs()
        big = a.max(dim=1).values
        if masks is not None:
            o = l * DM_LAYER + SITES["H"]
            a = torch.where(masks[:, o:o + 1024] != 0, a, torch.full_like(a, float("inf")))
        m = torch.minimum(m, a.min(dim=1).values / big)
    return m


# ----------------------------------------------------------------------------- recipe inputs
@functools.lru_cache(maxsize=None)
def recipe_den64():
    """The recipe denoiser of the parity tests on the CPU, in float64."""
    import types
    from seeme_amd.mld_denoiser import MldDenoiser
    from seeme_amd.weights_recipe import load_recipe_
    abl = types.SimpleNamespace(MLP_DIST=False, PE_TYPE="mld", SKIP_CONNECT=True, VAE_TYPE="actor", DIFF_PE_TYPE="mld", MD_TRANS=True)
    den = load_recipe_(MldDenoiser(abl, nfeats=75, condition=["text", "scene", "interactee"], latent_dim=[1, 256], ff_size=128,
                                   num_layers=5, num_heads=1))
    return den.double().eval()


def time_emb(den, t):
    """The twin's timestep embedding (denoiser_autograd.denoiser_forward_torch): fp32 features cast to the module's dtype."""
    from seeme_amd.mld_denoiser import timestep_features
    te = den.time_embedding
    feat = timestep_features(torch.as_tensor(t), den.text_encoded_dim, den.flip_sin_to_cos, den.freq_shift).to(te.linear_1.weight)
    return F.linear(F.silu(F.linear(feat, te.linear_1.weight, te.linear_1.bias)), te.linear_2.weight, te.linear_2.bias)


def tables(den, cond_bf, t):
    """ctab [B,N,5120], ttab [B,7680] of condition tokens cond_bf [B,N,256] (batch-first) and timesteps t, by the module's own builders."""
    from seeme_amd.denoiser_train import _tables
    return _tables(den, cond_bf.permute(1, 0, 2), time_emb(den, t))


def vetted_samples(N, count, seed, with_masks, timesteps=None, p_rows=None):
    """`count` samples for an N-token chain whose float64 relu_margin is >= RELU_MARGIN: candidates are drawn one at a time from a
    generator seeded with `seed` (latent, N condition tokens, timestep, mask row at keep-rate 0.5) and the first `count` that pass
    are kept.  ReLU is the chain's only kink: a unit within fp32 rounding of it (about 1e-6 of the layer's largest pre-activation)
    falls on either side and moves every upstream gradient by about 1 / 500, which no rounding bound covers.  The margin is a
    condition on the inputs, not a measurement of the kernel: at most 40 % of the candidates may fail it.
    `timesteps[i]` (not None) fixes the timestep and `p_rows[i]` (8 bytes, not None) the DM_P bytes, in every layer, of the sample
    that ends up at position i, before it is vetted.  Returns a dict: noisy [count,256], cond [count,N,256], t [count] (int64),
    masks uint8 [count,10960] or None, margin [count] (float64), rejected, drawn."""
    den = recipe_den64()
    P = chain_params(den, torch.float64)
    g = torch.Generator().manual_seed(seed)
    keep = {"noisy": [], "cond": [], "t": [], "masks": [], "margin": []}
    drawn = 0
    while len(keep["t"]) < count:
        i = len(keep["t"])
        drawn += 1
        noisy = torch.randn(1, 256, generator=g)
        cond = torch.randn(1, N, 256, generator=g)
        t = torch.randint(0, 1000, (1,), generator=g)
        m = (torch.rand(1, DM_TOTAL, generator=g) < 0.5).to(torch.uint8)
        if timesteps is not None and timesteps[i] is not None:
            t = torch.tensor([int(timesteps[i])])
        if p_rows is not None and p_rows[i] is not None:
            for l in range(5):
                m[0, l * DM_LAYER:l * DM_LAYER + 8] = torch.as_tensor(p_rows[i], dtype=torch.uint8)
        if not with_masks:
            m = None
        with torch.no_grad():
            ctab, ttab = tables(den, cond.double(), t)
        margin = float(relu_margin(P, noisy.double(), ctab, ttab, [0], m, 0.5)[0])
        if margin >= RELU_MARGIN:
            for k, v in (("noisy", noisy), ("cond", cond), ("t", t), ("masks", m)):
                keep[k].append(v)
            keep["margin"].append(margin)
        assert drawn <= 4 * count + 8, f"relu margin rejects {drawn - len(keep['t'])} of {drawn} candidates"
    rejected = drawn - count
    assert rejected <= 0.4 * drawn, f"relu margin rejected {rejected} of {drawn} candidates"
    out = {k: torch.cat(keep[k]) for k in ("noisy", "cond", "t")}
    out["masks"] = torch.cat(keep["masks"]) if with_masks else None
    out.update(margin=torch.tensor(keep["margin"], dtype=torch.float64), rejected=rejected, drawn=drawn)
    return out


# ----------------------------------------------------------------------------- error measure
def split_tensors(g, N):
    """A sample's gradients (keys of iter_per_sample_grads) -> {(kind, label): tensor}: the kinds group tensors over layers -- each
    linear's weight and bias, each of the five LayerNorms, encoder.norm, dx0, dctab as SA-K / SA-V / CA-key / CA-value, dttab as
    K / V and the four AdaLN rows."""
    out = {}
    for l, pre in enumerate(LAYERS):
        if l >= 3:
            wk, bk = skip_keys(l)
            out[("skip.weight", l)], out[("skip.bias", l)] = g[wk], g[bk]
        for name, (wk, bk) in LINEARS.items():
            out[(name + ".weight", l)], out[(name + ".bias", l)] = g[pre + wk], g[pre + bk]
        for n in NORMS:
            out[(n, (l, "w"))], out[(n, (l, "b"))] = g[pre + n + ".weight"], g[pre + n + ".bias"]
        c, t = g["ctab"], g["ttab"]
        for i, kind in enumerate(("ctab.sa_k", "ctab.sa_v")):
            out[(kind, l)] = c[:, l * 512 + 256 * i:l * 512 + 256 * (i + 1)]
        for i, kind in enumerate(("ctab.ca_key", "ctab.ca_value")):
            out[(kind, l)] = c[:, 2560 + l * 512 + 256 * i:2560 + l * 512 + 256 * (i + 1)]
        for i, kind in enumerate(("ttab.k", "ttab.v")):
            out[(kind, l)] = t[l * 512 + 256 * i:l * 512 + 256 * (i + 1)]
        for i, kind in enumerate(("ttab.ca_scale", "ttab.ca_shift", "ttab.ffn_scale", "ttab.ffn_shift")):
            out[(kind, l)] = t[2560 + l * 1024 + 256 * i:2560 + l * 1024 + 256 * (i + 1)]
    out[("encoder.norm", "w")], out[("encoder.norm", "b")] = g["encoder.norm.weight"], g["encoder.norm.bias"]
    out[("dx0", 0)] = g["noisy"]
    return out


def pair_errors(got, ref, N):
    """One sample: per (kind, label) the error max|got - ref| / max|ref| of the pairs whose reference reaches FLOOR * S_b (S_b: the
    sample's largest gradient entry over all tensors), and the pairs below it with max|got - ref| / S_b, to be held to FLOOR_ABS.
    Most of those are mathematically zero (one condition token: the softmax over the tokens is constant), where this is max|got| / S_b;
    a few are small and real -- the K row of a time token that gets almost no attention sits at 1e-5 .. 1e-4 of S_b -- and a bound on
    |got| alone would refuse the exact answer there."""
    R, G = split_tensors(ref, N), split_tensors(got, N)
    S = max(float(v.abs().max()) for v in R.values())
    errs, low = {}, {}
    for key, r in R.items():
        rm = float(r.abs().max())
        if rm < FLOOR * S:
            low[key] = float((G[key].double() - r.double()).abs().max()) / S
        else:
            errs[key] = float((G[key].double() - r.double()).abs().max()) / rm
    return errs, low
