"""k_den_bwd (csrc/den_train.inc.hip), the hand-derived backward of the five-layer denoiser chain, against a float64 restatement of the
chain from its tables (tests/den_backward_reference.py, pinned on the CPU by tests/test_den_backward_cpu.py): per sample, per
tensor, at 1-4 condition tokens.

The driver below does what denoiser_train._Chain does with everything explicit -- the caller's trow, masks, drop_scale and xcds, gout
zero-filled (the contract), dctab / dttab pre-filled with NaN, a sentinel tail behind every output -- and the reference takes the
DEVICE's fp32 tables cast to float64 as its leaves, so the chain is tested apart from the table builders.  Per-sample parameter
gradients are formed from gout on the CPU in float64 with the maps of denoiser_train._LIN / _DB (dW_b = dY_b (x) X_b, db_b = dY_b).

Error of sample b and tensor T: max|got - ref64| / max|ref64_T|; pairs whose float64 gradient is below 1e-4 of the sample's largest
gradient entry S_b (mathematically zero, e.g. the query path of the linear attention at one token, or next to it) only need
max|got - ref64| <= 1e-5 S_b, and their share is capped (20 % at N = 1, 5 % above).  Every other pair is under the ceiling of the end-to-end test
(test_gpu_parity.py::test_hip_backward_matches_autograd: 5e-4, 2e-4 for dctab and dx0), and per kind of tensor the kernel's worst
error is at most 4x the worst error of the SAME reference code run in float32 on the same inputs, both against float64 (DESIGN 5.7:
same computation, other summation order).  The forward's output is held, per sample, to 1e-4 and to 4x the float32 reference's own
error on that sample.  Inputs come from den_backward_reference.vetted_samples (no ReLU unit within fp32 rounding of its kink)."""
import ctypes as C

import pytest
import torch

import den_backward_reference as R

pytestmark = pytest.mark.gpu
TOL_F32 = 1e-4
CEILING, CEILING_TIGHT = 5e-4, 2e-4              # every pair; dctab and dx0
FACTOR = 4.0                                     # e_hip <= FACTOR * e_tw per kind
FACTORS = {}                                     # kind -> larger factor (at most 16), each with its reason
TAIL, SENT = 4096, -7777.25                      # sentinel floats behind every output buffer
# name -> (N, B, masks, seed of vetted_samples); the timesteps start 0, 999 and a duplicate pair
CASES = {"N1_B5_m": (1, 5, True, 11), "N2_B5": (2, 5, False, 12), "N3_B17_m": (3, 17, True, 13), "N4_B5_m": (4, 5, True, 14),
         "N4_B5": (4, 5, False, 15), "N3_B33_m": (3, 33, True, 16), "attn_rows": (4, 8, True, 17), "shared_t": (2, 5, True, 18)}
ACCURACY = ["N1_B5_m", "N2_B5", "N3_B17_m", "N4_B5_m", "N4_B5", "N3_B33_m"]
# (b) DM_P bytes of the eight samples, every layer: sample i drops attention weight i, 6 keeps only the time token, 7 drops all six
ATTN_ROWS = [[int(j != i) for j in range(6)] + [0, 0] for i in range(6)] + [[0, 0, 0, 0, 0, 1, 0, 0], [0] * 8]
SHARED_TROW, SHARED_T = [0, 0, 1, 2, 1], [0, 999, 500]


def case_inputs(name):
    """The vetted CPU inputs of a case (den_backward_reference.vetted_samples), deterministic."""
    N, B, wm, seed = CASES[name]
    ts = [0, 999, 250, 250] + [None] * (B - 4)
    rows = None
    if name == "attn_rows":
        rows = ATTN_ROWS
    if name == "shared_t":
        ts = [SHARED_T[r] for r in SHARED_TROW]
    return R.vetted_samples(N, B, seed, wm, timesteps=ts, p_rows=rows)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


class Rig:
    def __init__(self, dev):
        import types
        from seeme_amd.denoiser_train import TrainPack
        from seeme_amd.mld_denoiser import MldDenoiser
        from seeme_amd.weights_recipe import load_recipe_
        abl = types.SimpleNamespace(MLP_DIST=False, PE_TYPE="mld", SKIP_CONNECT=True, VAE_TYPE="actor", DIFF_PE_TYPE="mld", MD_TRANS=True)
        self.dev = dev
        self.den = load_recipe_(MldDenoiser(abl, nfeats=75, condition=["text", "scene", "interactee"], latent_dim=[1, 256], ff_size=128,
                                            num_layers=5, num_heads=1)).to(dev).eval()
        self.pack = TrainPack(self.den)
        self.pack.refresh()
        self.lay = self.pack.lay
        self.P64, self.P32 = R.chain_params(self.den, torch.float64), R.chain_params(self.den, torch.float32)
        self._inputs, self._runs, self._evals = {}, {}, {}

    def inputs(self, name):
        """Device inputs of a case: the vetted samples, the fp32 tables of denoiser_train._tables on the device, dout."""
        if name not in self._inputs:
            v = case_inputs(name)
            N, B, wm, seed = CASES[name]
            with torch.no_grad():
                ctab, ttab = R.tables(self.den, v["cond"].to(self.dev), v["t"].to(self.dev))
            assert ctab.dtype == torch.float32 and ctab.shape == (B, N, R.CROW) and ttab.shape == (B, R.TROW)
            dout = torch.randn(B, 256, generator=torch.Generator().manual_seed(1000 + seed))
            inp = dict(noisy=v["noisy"].to(self.dev), ctab=ctab.contiguous(), ttab=ttab.contiguous(),
                       trow=torch.arange(B, dtype=torch.int32, device=self.dev), masks=None if v["masks"] is None else v["masks"].to(self.dev),
                       scale=2.0 if wm else 1.0, p=0.5, dout=dout.to(self.dev), N=N, B=B)
            # the vetting holds for the tables the device built too (they move a pre-activation by about 1e-7 of the largest)
            m = R.relu_margin(self.P64, v["noisy"].double(), ctab.cpu().double(), ttab.cpu().double(), list(range(B)), v["masks"], 0.5)
            assert float(m.min()) >= 0.9 * R.RELU_MARGIN, (name, float(m.min()))
            self._inputs[name] = inp
        return self._inputs[name]

    def run(self, name, xcds=None):
        from seeme_amd import _lib as L
        inp = self.inputs(name)
        xcds = L.default_xcds(inp["B"]) if xcds is None else xcds
        if (name, xcds) not in self._runs:
            self._runs[(name, xcds)] = chain_run(self, inp, xcds)
        return self._runs[(name, xcds)]


@pytest.fixture(scope="module")
def rig(dev):
    return Rig(dev)


# ----------------------------------------------------------------------------- the driver
def _buf(n, fill, dev, dtype=torch.float32):
    b = torch.full((n + TAIL,), SENT, device=dev, dtype=dtype)
    b[:n] = fill
    return b


class Run:
    """The five output buffers of one forward + backward, on the CPU, heads and sentinel tails."""
    NAMES = ("out", "save", "gout", "dctab", "dttab")

    def __init__(self, B, N, lay):
        self.B, self.N = B, N
        self.shape = {"out": (B, 256), "save": (B, lay["DT_TOTAL"]), "gout": (B, lay["DB_TOTAL"]), "dctab": (B, N, R.CROW), "dttab": (B, R.TROW)}
        self.fill = {"out": float("nan"), "save": float("nan"), "gout": 0.0, "dctab": float("nan"), "dttab": float("nan")}
        self.full = {}

    def numel(self, k):
        n = 1
        for d in self.shape[k]:
            n *= d
        return n

    def alloc(self, k, dev):
        self.full[k] = _buf(self.numel(k), self.fill[k], dev)
        return self.full[k].data_ptr()

    def to_cpu(self):
        self.full = {k: v.cpu() for k, v in self.full.items()}
        return self

    def head(self, k):
        return self.full[k][:self.numel(k)].view(*self.shape[k])

    def bits(self, k, rows=None):
        h = self.head(k) if rows is None else self.head(k)[rows]
        return h.contiguous().view(torch.int32)

    def tails_intact(self):
        return all(bool((self.full[k][self.numel(k):] == SENT).all()) and self.full[k].numel() == self.numel(k) + TAIL for k in self.full)

    def untouched(self, k):
        want = torch.full((self.numel(k) + TAIL,), SENT)
        want[:self.numel(k)] = self.fill[k]
        return torch.equal(self.full[k].view(torch.int32), want.view(torch.int32))


def chain_forward(rig, inp, xcds, run, B=None, N=None):
    from seeme_amd import _lib as L
    a = L.SampleArgs()
    a.B, a.N = (inp["B"] if B is None else B), (inp["N"] if N is None else N)
    a.steps, a.sched, a.cfg, a.guidance_scale = 1, L.SCHED_NONE, 0, 1.0
    a.latents, a.ctab, a.ttab, a.trow, a.trow_per_sample = inp["noisy"].data_ptr(), inp["ctab"].data_ptr(), inp["ttab"].data_ptr(), inp["trow"].data_ptr(), 1
    a.coef, a.noise, a.catab = 0, 0, 0
    a.out, a.save, a.force_query = run.alloc("out", rig.dev), run.alloc("save", rig.dev), 1
    a.drop, a.drop_scale, a.xcds = L.ptr(inp["masks"]), inp["scale"], xcds
    try:
        L.call("seeme_denoiser_sample", C.byref(rig.pack.w), C.byref(a), L.current_stream())
    finally:
        torch.cuda.synchronize()


def chain_backward(rig, inp, xcds, run, B=None, N=None):
    from seeme_amd import _lib as L
    gout, dctab, dttab = run.alloc("gout", rig.dev), run.alloc("dctab", rig.dev), run.alloc("dttab", rig.dev)
    try:
        L.call("seeme_denoiser_backward_drop", C.byref(rig.pack.w), rig.pack.img_b.data_ptr(), inp["B"] if B is None else B,
               inp["N"] if N is None else N, run.full["save"].data_ptr(), inp["ctab"].data_ptr(), inp["ttab"].data_ptr(), inp["trow"].data_ptr(),
               inp["dout"].data_ptr(), gout, dctab, dttab, L.ptr(inp["masks"]), inp["scale"], xcds, L.current_stream())
    finally:
        torch.cuda.synchronize()


def chain_run(rig, inp, xcds):
    for k in ("noisy", "ctab", "ttab", "dout"):
        assert inp[k].is_contiguous() and inp[k].dtype == torch.float32
    assert inp["trow"].dtype == torch.int32 and int(inp["trow"].max()) < inp["ttab"].shape[0] and inp["trow"].numel() == inp["B"]
    assert inp["masks"] is None or (inp["masks"].dtype == torch.uint8 and inp["masks"].shape == (inp["B"], R.DM_TOTAL) and inp["masks"].is_contiguous())
    run = Run(inp["B"], inp["N"], rig.lay)
    chain_forward(rig, inp, xcds, run)
    chain_backward(rig, inp, xcds, run)
    return run.to_cpu()


def rows_of(inp, idx):
    """The samples `idx` of a case as a batch of their own (each with its own time row)."""
    i = torch.as_tensor(idx, device=inp["noisy"].device)
    sub = dict(inp, noisy=inp["noisy"][i].contiguous(), ctab=inp["ctab"][i].contiguous(), ttab=inp["ttab"][inp["trow"][i].long()].contiguous(),
               trow=torch.arange(len(idx), dtype=torch.int32, device=i.device), dout=inp["dout"][i].contiguous(), B=len(idx))
    sub["masks"] = None if inp["masks"] is None else inp["masks"][i].contiguous()
    return sub


# ----------------------------------------------------------------------------- gradients of one sample from the kernel's buffers
def hip_sample_grads(lay, gout_b, dctab_b, dttab_b):
    from seeme_amd.denoiser_train import _DB, _LIN
    DBL = lay["DB_LAYER"]
    gout_b = gout_b.double()
    g = {}
    for l, pre in enumerate(R.LAYERS):
        G = gout_b[l * DBL:(l + 1) * DBL]
        for name, (xo, K, yo, Nn) in _LIN.items():
            if name == "skip":
                if l < 3:
                    continue
                wk, bk = R.skip_keys(l)
            else:
                wk, bk = pre + R.LINEARS[name][0], pre + R.LINEARS[name][1]
            X, Y = G[_DB[xo]:_DB[xo] + K], G[_DB[yo]:_DB[yo] + Nn]
            g[wk], g[bk] = torch.outer(Y, X), Y
        for i, n in enumerate(R.NORMS):
            o = _DB["LN"] + i * 512
            g[pre + n + ".weight"], g[pre + n + ".bias"] = G[o:o + 256], G[o + 256:o + 512]
    fin = 5 * DBL
    g["encoder.norm.weight"], g["encoder.norm.bias"], g["noisy"] = gout_b[fin:fin + 256], gout_b[fin + 256:fin + 512], gout_b[fin + 512:fin + 768]
    g["ctab"], g["ttab"] = dctab_b.double(), dttab_b.double()
    return g


def evaluate(rig, name):
    """Per kind the worst error of the kernel and of the float32 reference against the float64 reference, the pairs below the floor,
    and the forward errors per sample."""
    if name in rig._evals:
        return rig._evals[name]
    inp, run = rig.inputs(name), rig.run(name)
    N, B = inp["N"], inp["B"]
    cpu = {k: (None if inp[k] is None else inp[k].cpu()) for k in ("noisy", "ctab", "ttab", "masks", "dout")}
    trow = inp["trow"].cpu().tolist()
    ref = R.iter_per_sample_grads(rig.P64, cpu["noisy"].double(), cpu["ctab"].double(), cpu["ttab"].double(), trow, cpu["masks"], inp["p"], cpu["dout"].double())
    tw = R.iter_per_sample_grads(rig.P32, cpu["noisy"], cpu["ctab"], cpu["ttab"], trow, cpu["masks"], inp["p"], cpu["dout"])
    res = dict(hip={}, tw={}, low=0, pairs=0, low_bad=[], worst_pair={}, fwd_hip=[], fwd_tw=[])
    out, gout, dctab, dttab = run.head("out"), run.head("gout"), run.head("dctab"), run.head("dttab")
    for b, ((o64, g64), (o32, g32)) in enumerate(zip(ref, tw)):
        om = float(o64.abs().max())
        res["fwd_hip"].append(float((out[b].double() - o64).abs().max()) / om)
        res["fwd_tw"].append(float((o32.double() - o64).abs().max()) / om)
        eh, lh = R.pair_errors(hip_sample_grads(rig.lay, gout[b], dctab[b], dttab[b]), g64, N)
        et, _ = R.pair_errors(g32, g64, N)
        res["pairs"] += len(eh) + len(lh)
        res["low"] += len(lh)
        res["low_bad"] += [(b, k, x) for k, x in lh.items() if not x <= R.FLOOR_ABS]
        for (kind, label), e in eh.items():
            if not e <= res["hip"].get(kind, -1.0):
                res["hip"][kind], res["worst_pair"][kind] = e, (b, label)
            res["tw"][kind] = max(res["tw"].get(kind, 0.0), et[(kind, label)])
    rig._evals[name] = res
    return res


def check_accuracy(name, res, N):
    print(f"\n{name}: forward per sample, kernel vs float64 " + " ".join(f"{e:.1e}" for e in res["fwd_hip"]) +
          f"; float32 reference worst {max(res['fwd_tw']):.2e}")
    print(f"{name}: {res['low']} of {res['pairs']} (sample, tensor) pairs below the floor")
    print(f"{'kind':<16}{'e_hip':>11}{'e_tw':>11}{'ratio':>8}   worst at (sample, label)")
    for kind in sorted(res["hip"], key=lambda k: -res["hip"][k] / max(res["tw"][k], 1e-30)):
        print(f"{kind:<16}{res['hip'][kind]:>11.3e}{res['tw'][kind]:>11.3e}{res['hip'][kind] / max(res['tw'][kind], 1e-30):>8.2f}   {res['worst_pair'][kind]}")
    print(f"{name}: forward per sample, float32 reference vs float64 " + " ".join(f"{e:.1e}" for e in res["fwd_tw"]))
    assert all(h <= TOL_F32 and h <= 4 * t for h, t in zip(res["fwd_hip"], res["fwd_tw"])), (res["fwd_hip"], res["fwd_tw"])
    assert not res["low_bad"], res["low_bad"][:5]
    assert res["low"] <= (0.20 if N == 1 else 0.05) * res["pairs"], (res["low"], res["pairs"])
    bad = []
    for kind, e in res["hip"].items():
        ceil = CEILING_TIGHT if kind.startswith("ctab") or kind == "dx0" else CEILING
        if not (e <= ceil and e <= FACTORS.get(kind, FACTOR) * res["tw"][kind]):
            bad.append((kind, e, res["tw"][kind], res["worst_pair"][kind]))
    assert not bad, bad


def memory_ok(run):
    """(f) no NaN pre-fill survives in dctab / dttab, every sentinel tail is intact, the skip slots of layers 0-2 are still zero."""
    from seeme_amd.denoiser_train import _DB
    assert bool(torch.isfinite(run.head("dctab")).all()) and bool(torch.isfinite(run.head("dttab")).all())
    assert bool(torch.isfinite(run.head("out")).all()) and bool(torch.isfinite(run.head("gout")).all())
    assert run.tails_intact()
    G = run.head("gout")[:, :5 * 9728].view(run.B, 5, 9728)
    assert not bool(G[:, :3, _DB["X_SKIP"]:_DB["X_SKIP"] + 512].any()) and not bool(G[:, :3, _DB["Y_SKIP"]:_DB["Y_SKIP"] + 256].any())
    assert bool(G[:, 3:, _DB["X_SKIP"]:_DB["X_SKIP"] + 512].any()) and bool(G[:, 3:, _DB["Y_SKIP"]:_DB["Y_SKIP"] + 256].any())


def same_bits(a, b, rows_a=None, rows_b=None):
    return [k for k in Run.NAMES if not torch.equal(a.bits(k, rows_a), b.bits(k, rows_b))]


# ----------------------------------------------------------------------------- a: accuracy per sample and per tensor
@pytest.mark.parametrize("name", ACCURACY)
def test_backward_per_sample_against_float64(rig, name):
    assert rig.lay["DB_LAYER"] == 9728
    inp = rig.inputs(name)
    t = case_inputs(name)["t"].tolist()
    assert 0 in t and 999 in t and len(set(t)) < len(t)
    memory_ok(rig.run(name))
    check_accuracy(name, evaluate(rig, name), inp["N"])


# ----------------------------------------------------------------------------- b: dropout of the attention row
def test_attention_row_dropout(rig):
    """N = 4, B = 8: sample i drops attention weight i of token 0's row (self, four conditions, time) in every layer, sample 6 keeps
    only the time token, sample 7 drops all six.  The bounds of the accuracy cases apply; bytes 6 and 7 of DM_P belong to no token
    and must not matter."""
    inp = rig.inputs("attn_rows")
    m = inp["masks"].cpu()
    for l in range(5):
        assert m[:, l * R.DM_LAYER:l * R.DM_LAYER + 8].tolist() == ATTN_ROWS
    base = rig.run("attn_rows")
    memory_ok(base)
    check_accuracy("attn_rows", evaluate(rig, "attn_rows"), 4)
    m2 = inp["masks"].clone()
    for l in range(5):
        m2[:, l * R.DM_LAYER + 6:l * R.DM_LAYER + 8] = 1
    other = chain_run(rig, dict(inp, masks=m2), 1)
    assert same_bits(base, other) == []


# ----------------------------------------------------------------------------- c: placement
@pytest.mark.parametrize("name", ["N4_B5_m", "N3_B17_m"])
def test_placement_does_not_change_a_bit(rig, name):
    """xcds 0 and 8: the dense grid; 1, 2, 7: the packed grids (7 > 5 leaves idle slots, 2 at B = 17 a half-filled last group).  One
    workgroup per sample, fixed-order sums, no atomics: every output is the same bits wherever the sample's workgroup sits."""
    base = rig.run(name, 0)
    memory_ok(base)
    for xcds in (1, 2, 7, 8):
        run = rig.run(name, xcds)
        memory_ok(run)
        assert same_bits(base, run) == [], xcds


# ----------------------------------------------------------------------------- d: shared time rows
def test_shared_time_rows(rig):
    """ttab with 3 rows and trow = [0, 0, 1, 2, 1] against the same samples with 5 expanded rows and trow = arange: same bits, and
    row b of dttab is sample b's."""
    inp = rig.inputs("shared_t")
    assert case_inputs("shared_t")["t"].tolist() == [SHARED_T[r] for r in SHARED_TROW]
    expanded = rig.run("shared_t", 1)
    for a, b in ((0, 1), (2, 4)):
        assert torch.equal(inp["ttab"][a], inp["ttab"][b])
    # (the three rows sit at the head of a five-row block, so that a row index taken from the wrong table stays inside it)
    block = torch.zeros(5, R.TROW, device=rig.dev)
    block[:3] = inp["ttab"][[0, 2, 3]]
    shared = dict(inp, ttab=block[:3], trow=torch.tensor(SHARED_TROW, dtype=torch.int32, device=rig.dev))
    run = chain_run(rig, shared, 1)
    memory_ok(run)
    assert same_bits(expanded, run) == []
    d = run.head("dttab")
    assert not torch.equal(d[0], d[1]) and not torch.equal(d[2], d[4])


# ----------------------------------------------------------------------------- e: batch independence
def test_rows_equal_the_samples_run_alone(rig):
    inp, big = rig.inputs("N3_B17_m"), rig.run("N3_B17_m")
    for b in (0, 7, 16):
        alone = chain_run(rig, rows_of(inp, [b]), 1)
        memory_ok(alone)
        assert same_bits(big, alone, rows_a=slice(b, b + 1)) == [], b


# ----------------------------------------------------------------------------- f: memory
def test_memory_of_every_case(rig):
    for name in CASES:
        memory_ok(rig.run(name))


# ----------------------------------------------------------------------------- g: refusals
@pytest.mark.parametrize("B,N", [(None, 0), (None, 5), (0, None)])
def test_refusals_leave_the_outputs_alone(rig, B, N):
    from seeme_amd._lib import SeemeError
    inp = rig.inputs("N4_B5")
    good = rig.run("N4_B5")
    run = Run(inp["B"], inp["N"], rig.lay)
    with pytest.raises(SeemeError):
        chain_forward(rig, inp, 1, run, B=B, N=N)
    run.full["save"].copy_(good.full["save"])                      # a valid forward's save: the backward refuses on its own
    with pytest.raises(SeemeError):
        chain_backward(rig, inp, 1, run, B=B, N=N)
    run.to_cpu()
    assert all(run.untouched(k) for k in ("out", "gout", "dctab", "dttab")) and torch.equal(run.bits("save"), good.bits("save"))
    assert run.tails_intact()
