"""k_linear (csrc/vae_kernels.hip) called directly through seeme_linear against the float64 twin of tests/linear_reference.py, at the
smallest shapes that reach every residue of the K pipeline, both A staging paths and their second load batch, the wide and the
narrow column mode, every epilogue path and the refusals of the launcher; and the three denoiser table builders against the
same GEMMs issued one by one through seeme_linear (the batched launch: nz, zs_*, pre_ln_zmin, a strided Y at a column offset).

Every input lives in a larger noise-filled buffer (A rows out to lda, columns past K, res out to ldr, W beyond roundup16(K);
W is zero from K to roundup16(K) as the header requires), every output in a sentinel-filled one: `_Out.read` asserts that nothing
outside Y[m, :N], m < M, changed a bit.  Inputs are N(0,1), W is scaled by 1/sqrt(K).  Unless a case says otherwise M = 33 (one
full and one 1-row tile), N = 80 (wave 0 full, wave 1 partial, waves 2 and 3 idle), K = 64, with a bias.

Bounds (linear_reference.py): without a LayerNorm `sum_path_bound`, the worst case of any summation order; with the pre-LN or
the fused LN the row rule 4 E + 4 u |ref|, E the float32-numpy error of the same formula (printed by every run).  CASES is
shared with tests/test_linear_cpu.py, which asserts that the float32 twin lies inside every sum bound.

Measured on an MI355X (printed again by every run), largest err / bound of each case group:
  K pipeline 0.066 (K = 3; 0.003 at K = 1008), A staging 0.036, M 0.050, wide N 0.053, narrow N 0.050, residual 0.054, output 0.044,
  activations 0.046, narrow vs wide 0.100 (and the same bits), table builders against the twin 0.013 (and the same bits);
  fused LN 0.480 with float32-twin E between 8.6e-7 and 1.9e-6; pre-LN 0.447 with E between 4.3e-7 (K = 3) and 3.0e-6 (K = 272).
K = 1008 launches with all 163,840 B of a workgroup's LDS; K = 1009 and K = 1024 are refused by the launcher's own guard.
The whole file runs in about 3 s.

What the cases catch (scratch builds, each a one-line change of the kernel, the whole file run once per change): the last
peeled k-block skipped: all 105 cases of CASES; the bias guard `g < n_valid - 1`: every case with a bias; the pre-LN statistics divided
by roundup16(K): the pre-LN cases with K = 3 and K = 75; the residual vector zeroed one vector early: the float4-residual cases
(res vec / ldr=N+4 at N = 256 and 132, narrow N=512 with ldr % 4 == 0, and every fused-LN case with a residual).
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import linear_reference as LR
import train_kernel_reference as R
from seeme_amd import _lib as L

pytestmark = pytest.mark.gpu
SENT = np.float32(-7.0e7)
F32 = np.float32
MAX_K = 1008        # SEEME_LINEAR_MAX_K of include/seeme_hip.h: 32 (Kp + 8) + 32 * 264 floats are 163,840 B at Kp = 1008
NONE, RELU, GELU, SILU = LR.ACT_NONE, LR.ACT_RELU, LR.ACT_GELU, LR.ACT_SILU
ACT_NAME = {NONE: "none", RELU: "relu", GELU: "gelu", SILU: "silu"}


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _up4(n):
    return (n + 3) // 4 * 4


def _up16(n):
    return (n + 15) // 16 * 16


def launcher_is_narrow(M, N, ln=False, nz=1):
    """seeme_launch_linear's rule: one 16-column tile per wave when N >= 512, no fused LN and at most 64 wide (32 x 256) tiles."""
    wide = ((M + 31) // 32) * ((N + 255) // 256) * nz
    return (not ln) and N >= 512 and wide <= 64


# ============================================================================= the cases
class Case:
    """One seeme_linear call.  None strides mean: lda = K1 (the float4 path when K % 4 == 0), lda2 = K - K1, ldr = N,
    ldy = roundup4(N) + 4 (vector stores when N % 4 == 0, a sentinel gap after every row).  *_off: floats between the (16-byte
    aligned) buffer and the pointer passed.  K1: columns taken from A, the rest from A2.  zero_row: that row of A is zero and its
    residual row constant, so that the value entering the fused LN is constant."""

    def __init__(self, id, group, M=33, N=80, K=64, K1=None, lda=None, lda2=None, a_off=0, bias=True, res=False, ldr=None, r_off=0,
                 ldy=None, y_off=0, act=NONE, pre_act=NONE, ln=False, pre_ln=False, zero_row=None, narrow=False):
        self.id, self.group, self.M, self.N, self.K = id, group, M, N, K
        self.K1 = K if K1 is None else K1
        self.concat = K1 is not None
        self.lda = self.K1 if lda is None else lda
        self.lda2 = (K - self.K1 if lda2 is None else lda2) if self.concat else 0
        self.a_off, self.bias, self.res, self.r_off = a_off, bias, res, r_off
        self.ldr = N if ldr is None else ldr
        self.ldy = _up4(N) + 4 if ldy is None else ldy
        self.y_off, self.act, self.pre_act, self.ln, self.pre_ln, self.zero_row, self.narrow = y_off, act, pre_act, ln, pre_ln, zero_row, narrow
        assert self.lda >= self.K1 and self.ldr >= N and self.ldy >= N and (not self.concat or self.lda2 >= K - self.K1)
        assert launcher_is_narrow(M, N, ln) == narrow, id

    @property
    def sum_bound(self):
        return not (self.ln or self.pre_ln)


def _cases():
    c = []
    # ---- K pipeline of tile_gemm_f32: every residue of K16 mod 4 below, at and above one ring, the unrolled K16 == 16, a long one
    for k16 in (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63):
        c.append(Case(f"K16={k16}", "K pipeline", K=16 * k16))
    for K in (3, 17, 75, 100, 270):       # K % 16 != 0: the zero-padded tail; K = 100: float4 staging with zero-filled vectors
        c.append(Case(f"K={K}", "K pipeline", K=K))
    c.append(Case(f"K={MAX_K}", "K pipeline", K=MAX_K))      # the largest K that fits: all of a workgroup's LDS
    # ---- A staging: float4 path and its second, partly filled batch (Kp >= 272), every way onto the scalar path, concat
    for K in (64, 272):
        c.append(Case(f"A vec K={K}", "A staging", K=K))
        c.append(Case(f"A lda=K+1 K={K}", "A staging", K=K, lda=K + 1))
        c.append(Case(f"A lda=K+4 K={K}", "A staging", K=K, lda=K + 4))
        c.append(Case(f"A+1 K={K}", "A staging", K=K, a_off=1))
    for K, K1 in ((64, 1), (64, 7), (64, 16), (64, 63), (272, 130)):
        c.append(Case(f"concat K={K} K1={K1}", "A staging", K=K, K1=K1, lda=K1 + 1, lda2=K - K1 + 3))
    # ---- rows
    for M in (1, 31, 32, 33, 65):
        c.append(Case(f"M={M}", "M", M=M))
    # ---- wide columns: N < 4, a partial 16-column tile, idle waves, a full tile, a one-column second tile
    for N in (1, 3, 75, 132, 255, 256, 257, 320):
        c.append(Case(f"N={N}", "wide N", N=N))
    # ---- narrow columns (M = 32: 2 or 3 wide tiles): whole, a one-column last workgroup, N % 4 != 0, partial last 16-column tiles
    for N in (512, 513, 530, 575, 577):
        c.append(Case(f"narrow N={N}", "narrow N", M=32, N=N, narrow=True))
        c.append(Case(f"narrow N={N} res ldr%4=0", "narrow N", M=32, N=N, res=True, ldr=_up4(N), narrow=True))
        c.append(Case(f"narrow N={N} res ldr=N+1", "narrow N", M=32, N=N, res=True, ldr=N + 1, narrow=True))
    # ---- residual: float4 rows (with the tail guard at N = 132: lanes 33.. hold no column), and every way onto the scalar path
    for N in (256, 132):
        c.append(Case(f"res vec N={N}", "residual", N=N, res=True, ldy=N))
        c.append(Case(f"res ldr=N+4 N={N}", "residual", N=N, res=True, ldr=N + 4))
        c.append(Case(f"res ldr=N+1 N={N}", "residual", N=N, res=True, ldr=N + 1))
        c.append(Case(f"res+1 N={N}", "residual", N=N, res=True, r_off=1))
    for N in (75, 257):
        c.append(Case(f"res N={N}", "residual", N=N, res=True))
    # ---- output rows
    for N in (132, 75):
        c.append(Case(f"ldy=N+4 N={N}", "output", N=N, ldy=N + 4))
        c.append(Case(f"ldy=N+1 N={N}", "output", N=N, ldy=N + 1))
    c.append(Case("Y at column 300 of 700", "output", N=256, ldy=700, y_off=300))     # as the table builders write
    c.append(Case("Y+1 ldy%4=0 N%4=0", "output", N=80, ldy=84, y_off=1))               # strides allow float4 stores, the pointer does not
    # ---- activations: (pre_act, act)
    for pre, act in ((NONE, NONE), (NONE, RELU), (NONE, GELU), (NONE, SILU), (RELU, NONE), (GELU, NONE), (SILU, NONE), (RELU, RELU)):
        for bias in (True, False):
            c.append(Case(f"pre={ACT_NAME[pre]} act={ACT_NAME[act]} bias={int(bias)}", "activations", pre_act=pre, act=act, bias=bias))
    # ---- fused LayerNorm over N = 256
    c.append(Case("ln", "fused LN", N=256, ln=True))
    c.append(Case("ln res", "fused LN", N=256, ln=True, res=True))
    c.append(Case("ln gelu res", "fused LN", N=256, ln=True, res=True, act=GELU))
    c.append(Case("ln M=1", "fused LN", M=1, N=256, ln=True, res=True))
    c.append(Case("ln constant row", "fused LN", N=256, ln=True, res=True, bias=False, zero_row=2))
    # ---- LayerNorm over K first: the lane loop strides by 64
    for K in (3, 75, 256, 272):
        c.append(Case(f"pre_ln K={K}", "pre-LN", K=K, pre_ln=True))
    c.append(Case("pre_ln silu K=75", "pre-LN", K=75, pre_ln=True, pre_act=SILU))
    c.append(Case("pre_ln concat K=75 K1=30", "pre-LN", K=75, K1=30, lda=31, lda2=48, pre_ln=True))
    c.append(Case("pre_ln M=1", "pre-LN", M=1, K=75, pre_ln=True))
    c.append(Case("pre_ln + ln", "pre-LN", N=256, K=75, pre_ln=True, ln=True, res=True))
    assert len({x.id for x in c}) == len(c)
    return c


CASES = _cases()
WIDE_CASE = Case("wide M=2080 N=512 K=16", "narrow vs wide", M=2080, N=512, K=16)


class Problem:
    """The host side of a case: flat noise buffers with the operands written into them, the twin and the bound."""

    def __init__(self, case):
        cs = self.case = case
        rng = np.random.Generator(np.random.PCG64(zlib.crc32(cs.id.encode())))
        M, N, K, K1 = cs.M, cs.N, cs.K, cs.K1
        Kp = _up16(K)
        noise = lambda n: rng.standard_normal(n).astype(F32)
        mm = np.arange(M)[:, None]
        self.a = noise(cs.a_off + M * cs.lda + 8)
        self.ia = cs.a_off + mm * cs.lda + np.arange(K1)[None, :]
        self.a2 = self.ia2 = None
        if cs.concat:
            self.a2 = noise(M * cs.lda2 + 8)
            self.ia2 = mm * cs.lda2 + np.arange(K - K1)[None, :]
        self.ldw = Kp + 4
        self.w = noise(N * self.ldw + 8)
        iw = np.arange(N)[:, None] * self.ldw + np.arange(Kp)[None, :]
        wv = np.zeros((N, Kp), F32)
        wv[:, :K] = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(F32)
        self.w[iw] = wv                                     # zero from K to roundup16(K), noise beyond
        self.iw = iw[:, :K]
        self.b = noise(N + 3)
        self.r = noise(cs.r_off + M * cs.ldr + 8)
        self.ir = cs.r_off + mm * cs.ldr + np.arange(N)[None, :]
        self.lnw, self.lnb = noise(max(N, 256) + 4), noise(max(N, 256) + 4)
        self.plw, self.plb = noise(Kp + 4), noise(Kp + 4)
        if cs.zero_row is not None:
            self.a[self.ia[cs.zero_row]] = 0.0
            self.r[self.ir[cs.zero_row]] = 1.25
        self.iy = cs.y_off + mm * cs.ldy + np.arange(N)[None, :]
        self.ny = cs.y_off + (M + 1) * cs.ldy + 7

    def twin(self, dtype=np.float64):
        cs = self.case
        return LR.linear(self.a[self.ia], self.w[self.iw], cs.K, A2=self.a2[self.ia2] if cs.concat else None,
                         bias=self.b[:cs.N] if cs.bias else None, res=self.r[self.ir] if cs.res else None,
                         ln=(self.lnw[:cs.N], self.lnb[:cs.N]) if cs.ln else None,
                         pre_ln=(self.plw[:cs.K], self.plb[:cs.K]) if cs.pre_ln else None, pre_act=cs.pre_act, act=cs.act,
                         eps=float(F32(1e-5)), dtype=dtype)

    def bound(self, ref):
        """-> bound, E (the largest float32-twin error, row cases only)"""
        cs = self.case
        if cs.sum_bound:
            return LR.sum_path_bound(ref, cs.K, cs.bias, cs.act, cs.res), None
        f32 = self.twin(F32).y
        return R.row_bound(f32, ref.y), float(np.abs(np.asarray(f32, np.float64) - ref.y).max())


# ============================================================================= device side
def _dev(dev, h):
    import torch
    return torch.from_numpy(np.ascontiguousarray(h)).to(dev)


class _Out:
    """A flat float32 device buffer of n elements, sentinel everywhere; `idx` (flat indices, any shape) is the window the kernel may
    write."""

    def __init__(self, dev, n, idx):
        self.idx = np.asarray(idx, np.int64)
        assert self.idx.min() >= 0 and self.idx.max() < n
        self.before = np.full(n, SENT, F32)
        self.t = _dev(dev, self.before)

    def ptr(self, off=0):
        return self.t.data_ptr() + 4 * off

    def raw(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def read(self):
        """the window after the kernel, having asserted that nothing outside it changed a bit"""
        after = self.raw()
        outside = np.ones(after.shape, bool)
        outside[self.idx.ravel()] = False
        assert np.array_equal(after.view(np.int32)[outside], self.before.view(np.int32)[outside]), "written outside the window"
        return after[self.idx]

    def untouched(self):
        return np.array_equal(self.raw().view(np.int32), self.before.view(np.int32))


def _within(got, ref, bound, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bound = np.broadcast_to(bound, err.shape)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max |err| {float(err.max()):.3e}, largest err / bound {worst:.3f}")
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(err[bad].max()), worst)


class _Launch:
    """The device buffers of a Problem and its SeemeLinearArgs; M: only the first M rows of the problem."""

    def __init__(self, dev, p, M=None):
        cs = p.case
        M = cs.M if M is None else M
        self.keep = {k: _dev(dev, getattr(p, k)) for k in ("a", "w", "b", "r", "lnw", "lnb", "plw", "plb")}
        if cs.concat:
            self.keep["a2"] = _dev(dev, p.a2)
        self.Y = _Out(dev, p.ny, p.iy[:M])
        t = lambda k, off=0: self.keep[k].data_ptr() + 4 * off
        a = self.args = L.LinearArgs()
        a.A, a.lda, a.K1 = t("a", cs.a_off), cs.lda, cs.K1
        a.A2, a.lda2 = (t("a2"), cs.lda2) if cs.concat else (0, 0)
        a.W, a.ldw, a.bias = t("w"), p.ldw, t("b") if cs.bias else 0
        a.res, a.ldr = (t("r", cs.r_off), cs.ldr) if cs.res else (0, 0)
        a.ln_w, a.ln_b = (t("lnw"), t("lnb")) if cs.ln else (0, 0)
        a.pre_ln_w, a.pre_ln_b = (t("plw"), t("plb")) if cs.pre_ln else (0, 0)
        a.Y, a.ldy, a.M, a.N, a.K = self.Y.ptr(cs.y_off), cs.ldy, M, cs.N, cs.K
        a.pre_act, a.act, a.eps = cs.pre_act, cs.act, 1e-5

    def run(self):
        L.check(L.lib().seeme_linear(C.byref(self.args), L.current_stream()), "seeme_linear")
        return self.Y.read()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_linear_case(dev, case):
    """One entry of CASES: the output window within the case's bound of the float64 twin, everything around it untouched."""
    p = Problem(case)
    got = _Launch(dev, p).run()
    ref = p.twin()
    bound, E = p.bound(ref)
    _within(got, ref.y, bound, f"[{case.group}] {case.id}" + ("" if E is None else f" (float32 twin E {E:.2e})"))
    if case.zero_row is not None:      # a constant row into the fused LN: centred values are exact zeros, the output is ln_b
        assert (ref.y[case.zero_row] == p.lnb[:case.N].astype(np.float64)).all()
        assert np.array_equal(got[case.zero_row], p.lnb[:case.N])


def test_narrow_and_wide_tiles_give_the_same_bits(dev):
    """M = 2080, N = 512, K = 16 is 65 x 2 = 130 wide tiles, above the launcher's 64: the wide path.  The same first 32 rows as an
    M = 32 call are 2 wide tiles: the narrow path.  Which wave owns a column changes, the order of its sum does not."""
    pb = Problem(WIDE_CASE)
    assert launcher_is_narrow(32, WIDE_CASE.N) and not launcher_is_narrow(WIDE_CASE.M, WIDE_CASE.N)
    gb, gs = _Launch(dev, pb).run(), _Launch(dev, pb, M=32).run()
    ref = pb.twin()
    _within(gb, ref.y, pb.bound(ref)[0], "[narrow vs wide] wide, M=2080")
    assert np.array_equal(gb[:32].view(np.int32), gs.view(np.int32)), "narrow and wide tiles differ"


REFUSALS = ["M=0", "N=0", "K=0", "ldw<roundup16(K)", "ldw%4!=0", "ln N=255", "K=1009", "K=1024"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_a_message_and_the_output_untouched(dev, what):
    """K = 1009 and K = 1024 pass every other guard and need 165,888 B of LDS: the launcher itself must refuse them, naming the
    largest K it supports (not the runtime, with a message about a function attribute)."""
    kw = {"ln N=255": dict(N=255, ln=True), "K=1009": dict(K=1009), "K=1024": dict(K=1024)}.get(what, {})
    p = Problem(Case(what, "refusals", **kw))
    l = _Launch(dev, p)
    a = l.args
    if what in ("M=0", "N=0", "K=0"):
        setattr(a, what[0], 0)
        if what == "K=0":
            a.K1 = 0
    elif what == "ldw<roundup16(K)":
        a.ldw = 48
    elif what == "ldw%4!=0":
        a.ldw = 66
    rc = L.lib().seeme_linear(C.byref(a), L.current_stream())
    msg = L.lib().seeme_last_error().decode("utf-8", "replace")
    print(f"{what}: rc {rc}, message {msg!r}")
    assert rc != 0 and msg.startswith("seeme_linear:"), (rc, msg)
    if what.startswith("K=10"):
        assert f"K > {MAX_K}" in msg, msg
    assert l.Y.untouched()


# ============================================================================= table builders
def _pub(**kw):
    """one public seeme_linear call from keyword fields (pointers as integers)"""
    a = L.LinearArgs()
    a.K1, a.eps = kw["K"], 1e-5
    for k, v in kw.items():
        setattr(a, k, v)
    L.check(L.lib().seeme_linear(C.byref(a), L.current_stream()), "seeme_linear")


def _same_bits(x, y, what):
    assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)), what


def _rows(n, ld, width=None):
    return np.arange(n)[:, None] * ld + np.arange(ld if width is None else width)[None, :]


@pytest.fixture(scope="module")
def den(dev):
    import types
    from seeme_amd.mld_denoiser import MldDenoiser
    from seeme_amd.weights_recipe import load_recipe_
    abl = types.SimpleNamespace(MLP_DIST=False, PE_TYPE="mld", SKIP_CONNECT=True, VAE_TYPE="actor", DIFF_PE_TYPE="mld", MD_TRANS=True)
    return load_recipe_(MldDenoiser(abl, nfeats=75, condition=["text", "interactee"], latent_dim=[1, 256], ff_size=128, num_layers=5,
                                    num_heads=1, weight_dtype="fp32")).to(dev).eval()


def _noise_dev(dev, seed, n):
    h = np.random.Generator(np.random.PCG64(seed)).standard_normal(n).astype(F32)
    return h, _dev(dev, h)


@pytest.mark.parametrize("n_rows", [1, 5, 33])
def test_time_tables_equal_their_four_public_calls(dev, den, n_rows):
    """seeme_denoiser_time_tables issues four plain launches: linear_1 + SiLU, linear_2, the 2560-column K|V table and the
    5120-column SiLU-prologue style table into SEEME_TROW-strided rows at column 0 and 2560 (both narrow here).  Bit for bit the
    same four calls through seeme_linear.  At n_rows = 5 every one of the four is also held to the float64 twin on the input the
    GPU gave it (t1 and temb are read back from the workspace), with the sum bound at K = 256."""
    import torch
    w = den._weights()
    fh, ft = _noise_dev(dev, [31, n_rows], n_rows * 256)
    ws = torch.zeros(L.lib().seeme_denoiser_workspace_bytes(n_rows, 0, 0) // 4, dtype=torch.float32, device=dev)
    ttab = _Out(dev, (n_rows + 1) * L.TROW, _rows(n_rows, L.TROW))
    L.check(L.lib().seeme_denoiser_time_tables(C.byref(w), ft.data_ptr(), n_rows, ttab.ptr(), ws.data_ptr(), ws.numel() * 4,
                                               L.current_stream()), "seeme_denoiser_time_tables")
    got = ttab.read()
    t1, temb = _Out(dev, (n_rows + 1) * 256, _rows(n_rows, 256)), _Out(dev, (n_rows + 1) * 256, _rows(n_rows, 256))
    tt2 = _Out(dev, (n_rows + 1) * L.TROW, _rows(n_rows, L.TROW))
    sh = dict(lda=256, ldw=256, M=n_rows, K=256)
    _pub(A=ft.data_ptr(), W=w.time_w1, bias=w.time_b1, Y=t1.ptr(), ldy=256, N=256, act=SILU, **sh)
    _pub(A=t1.ptr(), W=w.time_w2, bias=w.time_b2, Y=temb.ptr(), ldy=256, N=256, **sh)
    _pub(A=temb.ptr(), W=w.kv_cat_w, bias=w.kv_cat_b, Y=tt2.ptr(), ldy=L.TROW, N=2560, **sh)
    _pub(A=temb.ptr(), W=w.style_cat_w, bias=w.style_cat_b, Y=tt2.ptr(2560), ldy=L.TROW, N=5120, pre_act=SILU, **sh)
    g1, g2 = t1.read(), temb.read()
    _same_bits(got, tt2.read(), "ttab")
    wsh = ws.cpu().numpy()
    _same_bits(wsh[:n_rows * 256].reshape(n_rows, 256), g1, "t1 in the workspace")
    _same_bits(wsh[n_rows * 256:2 * n_rows * 256].reshape(n_rows, 256), g2, "temb in the workspace")
    if n_rows == 5:
        te, wc = den.time_embedding, den._wcache[2]
        host = lambda t: t.detach().cpu().numpy()
        steps = [("t1", fh.reshape(n_rows, 256), te.linear_1.weight, te.linear_1.bias, NONE, SILU, g1),
                 ("temb", g1, te.linear_2.weight, te.linear_2.bias, NONE, NONE, g2),
                 ("ttab K|V", g2, wc[2], wc[3], NONE, NONE, got[:, :2560]),
                 ("ttab style", g2, wc[4], wc[5], SILU, NONE, got[:, 2560:])]
        for name, x, W, b, pre, act, out in steps:
            ref = LR.linear(x, host(W), 256, bias=host(b), pre_act=pre, act=act)
            _within(out, ref.y, LR.sum_path_bound(ref, 256, True, act, False), f"[tables] time_tables {name}")


@pytest.mark.parametrize("Bc,N", [(1, 1), (5, 1), (33, 1), (1, 2), (3, 2), (17, 2)])
def test_cond_tables_equal_their_two_public_calls(dev, den, Bc, N):
    """One batched launch (nz = 2, zs_a = 0, zs_w / zs_b the distance between two weight tensors, zs_y = 2560, pre_ln_zmin = 1: only
    z = 1 normalises its rows) against the two GEMMs through seeme_linear: bit for bit.  Bc N = 1, 5, 33 rows with one token per
    sample; with two tokens the row count is even: 2, 6 and 34 (below a tile, and one full tile plus two rows)."""
    w = den._weights()
    M = Bc * N
    _, ct = _noise_dev(dev, [32, Bc, N], M * 256)
    ctab, ctab2 = (_Out(dev, (M + 1) * L.CROW, _rows(M, L.CROW)) for _ in range(2))
    L.check(L.lib().seeme_denoiser_cond_tables(C.byref(w), ct.data_ptr(), Bc, N, ctab.ptr(), 0, 0, L.current_stream()),
            "seeme_denoiser_cond_tables")
    sh = dict(A=ct.data_ptr(), lda=256, ldw=256, ldy=L.CROW, M=M, N=2560, K=256)
    _pub(W=w.kv_cat_w, bias=w.kv_cat_b, Y=ctab2.ptr(), **sh)
    _pub(W=w.ca_fold_w, bias=w.ca_fold_b, Y=ctab2.ptr(2560), pre_ln_w=w.ln_ones, pre_ln_b=w.ln_zeros, **sh)
    _same_bits(ctab.read(), ctab2.read(), "ctab")


@pytest.mark.parametrize("Bc,n_trow,per_sample", [(1, 1, 1), (5, 2, 1), (11, 3, 0)])
def test_ca_tables_equal_their_five_public_calls(dev, den, Bc, n_trow, per_sample):
    """rows = Bc R = 1, 5, 33.  The builder leaves its H rows [5][rows][256] in the caller's workspace and multiplies them by the five
    proj_out matrices in one batched launch (nz = 5, every zs_* non-zero, Y at column 256 l of 1280-float rows); the same H rows
    through five seeme_linear calls give the same bits."""
    import torch
    w = den._weights()
    R_ = 1 if per_sample else n_trow
    rows = Bc * R_
    _, ct = _noise_dev(dev, [33, Bc], Bc * 256)
    _, ft = _noise_dev(dev, [34, Bc], 3 * 256)
    ctab, ttab = den.cond_tables(ct.reshape(Bc, 1, 256)), den.time_tables(ft.reshape(3, 256))
    trow = torch.tensor([2, 0, 1][:n_trow], dtype=torch.int32, device=dev)
    ws = torch.zeros(5 * rows * 256, dtype=torch.float32, device=dev)
    catab, catab2 = (_Out(dev, (rows + 1) * 1280, _rows(rows, 1280)) for _ in range(2))
    L.check(L.lib().seeme_denoiser_ca_tables(C.byref(w), ctab.data_ptr(), ttab.data_ptr(), trow.data_ptr(), per_sample, n_trow, Bc,
                                             catab.ptr(), ws.data_ptr(), ws.numel() * 4, L.current_stream()), "seeme_denoiser_ca_tables")
    got = catab.read()
    assert np.isfinite(got).all()
    for l in range(5):
        _pub(A=ws.data_ptr() + 4 * l * rows * 256, lda=256, W=w.ca_po_w + 4 * l * 65536, ldw=256, bias=w.ca_po_b + 4 * l * 256,
             Y=catab2.ptr(256 * l), ldy=1280, M=rows, N=256, K=256)
    _same_bits(got, catab2.read(), "catab")
