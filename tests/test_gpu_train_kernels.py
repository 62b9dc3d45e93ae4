"""The training-step HIP entry points called directly, one by one, against the float64 twins of train_kernel_reference.py at the
smallest shapes that reach each tile edge, path switch and tail.

Every output buffer is larger than the window the kernel may write and is pre-filled with a sentinel; `_Out.read` asserts that
everything outside the window is bit-identical afterwards.  Every accumulating output starts from random non-zero contents.
Bounds (train_kernel_reference.py): sums `(L + 16) u mag + 4 u |ref|`; row kernels `4 E + 4 u |ref|` with E the float32-numpy
error of the same formula, measured on the CPU (figures in the docstrings, printed again by every run); sentinels, masked
softmax zeros, dropout and the den_wgrad repeat launch are bit-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_kernel_reference as R
from seeme_amd import _lib as L
from seeme_amd.stage2_glue import _Group, _prob

pytestmark = pytest.mark.gpu
SENT = np.float32(-7.0e7)
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


class _In:
    """A flat float32 device buffer holding `vals` at the flat indices `idx` (random elsewhere, so a wrong stride reads noise)."""

    def __init__(self, dev, rng, n, idx=None, vals=None):
        self.h = rng.standard_normal(n).astype(F32)
        if idx is not None:
            self.h[idx] = vals
        self.t = torch.from_numpy(self.h).to(dev)

    def ptr(self, off=0):
        return self.t.data_ptr() + 4 * off


def _in(dev, arr, dtype=None):
    a = np.ascontiguousarray(arr, dtype=dtype)
    return torch.from_numpy(a).to(dev)


class _Out:
    """A flat float32 device buffer of n elements, sentinel everywhere except the window `idx` (flat indices, any shape), which
    holds `init` when the kernel accumulates into it."""

    def __init__(self, dev, n, idx, init=None):
        self.idx = np.asarray(idx, np.int64)
        assert self.idx.min() >= 0 and self.idx.max() < n
        h = np.full(n, SENT, F32)
        if init is not None:
            h[self.idx] = np.asarray(init, F32)
        self.before = h.copy()
        self.t = torch.from_numpy(h).to(dev)

    def ptr(self, off=0):
        return self.t.data_ptr() + 4 * off

    def init(self):
        return self.before[self.idx]

    def raw(self):
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


def _st():
    return L.current_stream()


# ============================================================================= grouped GEMM
class _GG:
    """One seeme_grouped_gemm problem on freshly drawn N(0,1) operands, built with the production descriptor builder.
    a_contig 'k': A[i,k] at i*lda + k (a_rs = lda, a_ks = 1); 'i': at k*lda[s] + i (a_rs = 1, a_ks[s] = lda[s]).
    b_contig 'k': B[k,j] at j*ldb + k (b_cs = ldb, b_ks = 1); 'j': at k*ldb[s] + j (b_cs = 1, b_ks[s] = ldb[s]).
    Every segment has its own buffer (base); batch members are a_bs / b_bs / c_bs floats apart (0: shared)."""

    def __init__(self, rng, dev, M, N, seg_len, *, a_contig="k", b_contig="k", lda=None, ldb=None, a_off=0, b_off=0, ldc=None,
                 a_pro=0, b_pro=0, bias=False, epi=0, e_ld=None, alpha=1.0, addend=False, add_ld=None, accumulate=0, colsum=False,
                 nbatch=1, share_b=False, share_c=False, name=""):
        self.name, self.M, self.N, self.seg_len, self.nbatch, self.acc, self.share_c = name, M, N, list(seg_len), nbatch, accumulate, share_c
        nseg = len(seg_len)
        assert nbatch == 1 or nseg == 1
        assert not share_c or accumulate == 2            # a shared C is legal only as a split reduction
        ii, jj = np.arange(M)[:, None], np.arange(N)[None, :]
        as_list = lambda v, d: [d] * nseg if v is None else ([v] * nseg if np.isscalar(v) else list(v))
        if a_contig == "k":
            lda = as_list(lda, max(seg_len))
            assert len(set(lda)) == 1
            a_rs, a_ks, a_size = lda[0], [1] * nseg, [M * lda[0]] * nseg
        else:
            lda = as_list(lda, M)
            a_rs, a_ks, a_size = 1, lda, [n * l for n, l in zip(seg_len, lda)]
        if b_contig == "k":
            ldb = as_list(ldb, max(seg_len))
            assert len(set(ldb)) == 1
            b_cs, b_ks, b_size = ldb[0], [1] * nseg, [N * ldb[0]] * nseg
        else:
            ldb = as_list(ldb, N)
            b_cs, b_ks, b_size = 1, ldb, [n * l for n, l in zip(seg_len, ldb)]
        a_bs = a_size[0] + 4 if nbatch > 1 else 0
        b_bs = 0 if (share_b or nbatch == 1) else b_size[0] + 4
        self.A = [[None] * nseg for _ in range(nbatch)]
        self.B = [[None] * nseg for _ in range(nbatch)]
        self.keep, a_ptr, b_ptr = [], [], []
        for s, n in enumerate(seg_len):
            kk = np.arange(n)
            ab = _In(dev, rng, a_off + a_size[s] + (nbatch - 1) * a_bs + 8)
            bb = _In(dev, rng, b_off + b_size[s] + (nbatch - 1) * b_bs + 8)
            for z in range(nbatch):
                self.A[z][s] = ab.h[a_off + z * a_bs + ii * a_rs + kk[None, :] * a_ks[s]]
                self.B[z][s] = bb.h[b_off + z * b_bs + kk[:, None] * b_ks[s] + jj * b_cs]
            self.keep += [ab, bb]
            a_ptr.append(ab.ptr(a_off))
            b_ptr.append(bb.ptr(b_off))
        kw = {}
        self.tw = dict(a_pro=a_pro, b_pro=b_pro, epi=epi, alpha=alpha)
        if a_pro == 3:
            p0, p1 = _In(dev, rng, max(seg_len)), _In(dev, rng, max(seg_len))
            self.keep += [p0, p1]
            kw["a_p"], self.tw["a_p"] = (p0.ptr(), p1.ptr()), (p0.h, p1.h)
        if b_pro == 3:
            p0, p1 = _In(dev, rng, N), _In(dev, rng, N)
            self.keep += [p0, p1]
            kw["b_p"], self.tw["b_p"] = (p0.ptr(), p1.ptr()), (p0.h, p1.h)
        if bias:
            bv = _In(dev, rng, N)
            self.keep.append(bv)
            kw["bias"], self.tw["bias"] = bv.ptr(), bv.h
        if epi == 1:
            e_ld = e_ld or N
            ev = _In(dev, rng, M * e_ld)
            self.keep.append(ev)
            kw.update(e0=ev.ptr(), e_ld=e_ld)
            self.tw["e0"] = ev.h[ii * e_ld + jj]
        if addend:
            add_ld = add_ld or N
            av = _In(dev, rng, M * add_ld)
            self.keep.append(av)
            kw.update(addend=av.ptr(), add_ld=add_ld)
            self.tw["addend"] = av.h[ii * add_ld + jj]
        ldc = ldc or N + 3
        c_bs = 0 if (share_c or nbatch == 1) else (M + 2) * ldc + 5
        nc = 1 if share_c else nbatch
        cidx = 3 + np.arange(nc)[:, None, None] * c_bs + ii[None] * ldc + jj[None]
        self.C = _Out(dev, 3 + (M + 2) * ldc + (nc - 1) * c_bs + 7, cidx, rng.standard_normal(cidx.shape) if accumulate else None)
        self.cs = None
        if colsum:
            assert nbatch == 1 or accumulate == 2
            self.cs = _Out(dev, M + 5, 2 + np.arange(M), rng.standard_normal(M) if accumulate else None)
        self.prob = _prob(a_ptr, b_ptr, list(seg_len), a_ks, b_ks, a_rs, b_cs, self.C.ptr(3), ldc, M, N, a_pro=a_pro, b_pro=b_pro,
                          epi=epi, accumulate=accumulate, colsum=self.cs.ptr(2) if colsum else 0, nbatch=nbatch,
                          bstrides=(a_bs, b_bs, c_bs), alpha=alpha, **kw)

    def check(self):
        got, c0 = self.C.read(), self.C.init()
        parts = [R.grouped_gemm(self.A[z], self.B[z], **self.tw) for z in range(self.nbatch)]
        K = sum(self.seg_len)
        if self.share_c:
            ref = R.accumulate(c0[0], [p[0] for p in parts], 2)[None]
            mag = sum(p[1] for p in parts)[None]
            L_ = K * self.nbatch + 1
        else:
            ref = np.stack([R.accumulate(c0[z], [parts[z][0]], self.acc) for z in range(self.nbatch)])
            mag = np.stack([p[1] for p in parts])
            L_ = K + (1 if self.acc else 0)
        _within(got, ref, R.sum_bound(L_, mag, ref), f"k_gg {self.name} C")
        if self.cs is not None:
            got, cs0 = self.cs.read(), self.cs.init()
            ref = sum(p[2] for p in parts) + (cs0.astype(np.float64) if self.acc else 0.0)
            _within(got, ref, R.sum_bound(K * self.nbatch + 1, sum(p[3] for p in parts), ref), f"k_gg {self.name} colsum")


def _launch(dev, cases):
    g = _Group([c.prob for c in cases], dev)
    tiles = [c.prob.tile0 for c in cases]
    assert tiles == sorted(tiles)
    g.launch()
    torch.cuda.synchronize()
    for c in cases:
        c.check()
    return g


def test_gg_minimal_single_problem(dev):
    """n_probs = 1, one tile, M = N = K = 1: the tile0 search with lo == hi, every guard of the slow path at once."""
    g = _launch(dev, [_GG(_rng(1), dev, 1, 1, [1], name="1x1x1")])
    assert (g.n, g.tiles) == (1, 1)


def test_gg_fast_and_slow_paths_of_the_fwd_form(dev):
    """k-contiguous A and B at M=65, N=130, K=129: interior tiles take dwordx4 loads (ld 132, aligned bases), edge tiles and the
    last k-step the guarded scalar ones; ld 131 and bases offset by one float push every tile onto the scalar path.  The same
    bound holds for all three; a 1x1x1 problem in between gives the tile0 search unequal tile counts (6, 1, 6, 6)."""
    rng = _rng(2)
    kw = dict(bias=True)
    cases = [_GG(rng, dev, 65, 130, [129], lda=132, ldb=132, ldc=132, name="ld132", **kw),
             _GG(rng, dev, 1, 1, [1], name="1x1x1 among others"),
             _GG(rng, dev, 65, 130, [129], lda=131, ldb=131, ldc=131, name="ld131", **kw),
             _GG(rng, dev, 65, 130, [129], lda=132, ldb=132, a_off=1, b_off=1, name="ld132 bases+1", **kw)]
    g = _launch(dev, cases)
    assert g.tiles == 19


def test_gg_wgrad_form_with_colsum(dev):
    """i-contiguous A, j-contiguous B (dY^T X over 100 rows) at M=70, N=66 with the fused column sum and accumulate=1, on the
    dwordx4 path (ld 72 / 68) and on the scalar one (ld 71 / 67, and aligned strides on bases offset by one float)."""
    rng = _rng(3)
    kw = dict(a_contig="i", b_contig="j", accumulate=1, colsum=True)
    _launch(dev, [_GG(rng, dev, 70, 66, [100], lda=72, ldb=68, name="wgrad ld72/68", **kw),
                  _GG(rng, dev, 70, 66, [100], lda=71, ldb=67, name="wgrad ld71/67", **kw),
                  _GG(rng, dev, 70, 66, [100], lda=72, ldb=68, a_off=1, b_off=1, name="wgrad bases+1", **kw),
                  _GG(rng, dev, 70, 66, [100], lda=72, ldb=68, a_contig="i", b_contig="j", colsum=True, name="wgrad store")])


def test_gg_segments(dev):
    """nseg=3 with lengths (64, 1, 70): a segment that ends exactly on a k-step, a one-element one, and one with a ragged second
    step; nseg=10 of length 5, every segment with its own base and its own a_ks / b_ks; both operand orientations."""
    rng = _rng(4)
    _launch(dev, [_GG(rng, dev, 65, 66, [64, 1, 70], a_contig="k", b_contig="j", lda=72, ldb=[68, 67, 72], name="3 seg dgrad form"),
                  _GG(rng, dev, 65, 66, [64, 1, 70], a_contig="k", b_contig="k", lda=72, ldb=72, bias=True, name="3 seg fwd form"),
                  _GG(rng, dev, 70, 66, [5] * 10, a_contig="i", b_contig="j", lda=[72 + s for s in range(10)],
                      ldb=[68 + 2 * s for s in range(10)], accumulate=1, colsum=True, name="10 seg wgrad form"),
                  _GG(rng, dev, 3, 2, [5] * 10, a_contig="k", b_contig="j", lda=8, ldb=[2 + s for s in range(10)], name="10 seg small")])


def test_gg_prologues(dev):
    """a_pro x b_pro in {SiLU, ReLU, affine}^2 at M=65, N=66, K=65 (a ragged tile in every dimension), distinct p0 / p1 vectors per
    operand; and the affine A prologue over two segments (40 + 25), where its index restarts with the segment."""
    rng = _rng(5)
    cases = [_GG(rng, dev, 65, 66, [65], lda=68, ldb=68, a_pro=a, b_pro=b, name=f"pro a{a} b{b}") for a in (1, 2, 3) for b in (1, 2, 3)]
    cases.append(_GG(rng, dev, 65, 66, [40, 25], lda=44, ldb=44, a_pro=3, name="affine A over 2 segments"))
    cases.append(_GG(rng, dev, 65, 66, [65], a_contig="i", b_contig="j", lda=68, ldb=68, a_pro=3, b_pro=3, name="affine, wgrad form"))
    _launch(dev, cases)


def test_gg_epilogues(dev):
    """bias; epi=1 with e_ld != N; epi=2 with alpha=-0.37; addend with add_ld != ldc; and all of them with accumulate=1: the order
    ((A B + bias) * epi) + addend, then the accumulate."""
    rng = _rng(6)
    sh = dict(lda=68, ldb=68)
    _launch(dev, [_GG(rng, dev, 65, 66, [65], bias=True, name="bias", **sh),
                  _GG(rng, dev, 65, 66, [65], epi=1, e_ld=71, name="epi1", **sh),
                  _GG(rng, dev, 65, 66, [65], epi=2, alpha=-0.37, name="epi2", **sh),
                  _GG(rng, dev, 65, 66, [65], addend=True, add_ld=75, ldc=70, name="addend", **sh),
                  _GG(rng, dev, 65, 66, [65], bias=True, epi=1, e_ld=71, addend=True, add_ld=75, ldc=70, accumulate=1, name="all, epi1", **sh),
                  _GG(rng, dev, 65, 66, [65], bias=True, epi=2, alpha=-0.37, addend=True, add_ld=75, ldc=70, accumulate=1, name="all, epi2", **sh)])


def test_gg_batched(dev):
    """nbatch=3 with distinct outputs (accumulate=0) and a shared B (b_bstride=0); nbatch=3 as a split reduction into one C
    (c_bstride=0, accumulate=2) with the column sum; a plain problem after them, so tile0 follows the batch members' tiles."""
    rng = _rng(7)
    g = _launch(dev, [_GG(rng, dev, 65, 66, [70], lda=72, ldb=72, nbatch=3, share_b=True, bias=True, name="batched, own C"),
                      _GG(rng, dev, 70, 66, [33], a_contig="i", b_contig="j", lda=72, ldb=68, nbatch=3, share_c=True, accumulate=2,
                          colsum=True, name="batched, split reduction"),
                      _GG(rng, dev, 5, 3, [2], name="after the batches")])
    assert g.tiles == 12 + 12 + 1


# ============================================================================= gemm128 / wgrad128
def _gemm128_bufs(dev, rng, M, N, K, nt, lda, ldb, ldc, a_off=0):
    A = _In(dev, rng, a_off + M * lda + 8)
    Bw = _In(dev, rng, (N if nt else K) * ldb + 8)
    ii, jj = np.arange(M)[:, None], np.arange(N)[None, :]
    Cb = _Out(dev, (M + 1) * ldc + 4, ii * ldc + jj)
    Ah = A.h[a_off + ii * lda + np.arange(K)[None, :]]
    Bh = Bw.h[np.arange(N)[:, None] * ldb + np.arange(K)[None, :]] if nt else Bw.h[np.arange(K)[:, None] * ldb + jj]
    return A, Bw, Cb, Ah, Bh


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("shape", [(128, 128, 32), (256, 128, 96), (128, 256, 64)])
@pytest.mark.parametrize("bias,addend", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm128(dev, nt, shape, bias, addend):
    """one, three and two k-steps (the double buffer's first, odd and even hand-over); lda / ldb / ldc padded by 4; bias and an
    addend of its own row stride on and off; NT (y = x W^T) and NN (dx = dy W)."""
    M, N, K = shape
    rng = _rng(8, M, N, K, nt, bias, addend)
    lda, ldb, ldc, add_ld = K + 4, (K if nt else N) + 4, N + 4, N + 8
    A, Bw, Cb, Ah, Bh = _gemm128_bufs(dev, rng, M, N, K, nt, lda, ldb, ldc)
    bv = _In(dev, rng, N) if bias else None
    av = _In(dev, rng, M * add_ld) if addend else None
    L.check(L.lib().seeme_gemm128(A.ptr(), lda, Bw.ptr(), ldb, nt, Cb.ptr(), ldc, M, N, K, bv.ptr() if bias else 0,
                                  av.ptr() if addend else 0, add_ld if addend else 0, _st()), "seeme_gemm128")
    ref, mag = R.gemm128(Ah, Bh, nt, bv.h if bias else None,
                         av.h[np.arange(M)[:, None] * add_ld + np.arange(N)[None, :]] if addend else None)
    _within(Cb.read(), ref, R.sum_bound(K, mag, ref), f"gemm128 nt={nt} {shape} bias={bias} addend={addend}")


@pytest.mark.parametrize("what", ["M=127", "K=48", "lda=130", "A+1"])
def test_gemm128_refusals_leave_the_output_untouched(dev, what):
    rng = _rng(9)
    M, N, K, lda, a_off = 128, 128, 64, 132, 0
    A, Bw, Cb, _, _ = _gemm128_bufs(dev, rng, M, N, K, 1, lda, 68, 132, a_off=4)
    if what == "M=127":
        M = 127
    elif what == "K=48":
        K = 48
    elif what == "lda=130":
        lda = 130
    else:
        a_off = 1
    with pytest.raises(L.SeemeError):
        L.check(L.lib().seeme_gemm128(A.ptr(a_off), lda, Bw.ptr(), 68, 1, Cb.ptr(), 132, M, N, K, 0, 0, 0, _st()), "seeme_gemm128")
    assert Cb.untouched()


@pytest.mark.parametrize("shape", [(128, 128), (256, 128), (128, 256)])
@pytest.mark.parametrize("M", [1, 31, 64, 65, 97, 200])
@pytest.mark.parametrize("with_gbias", [0, 1])
def test_wgrad128(dev, shape, M, with_gbias):
    """fewer rows than one 32-row k-step, exactly one 64-row chunk, one row into the second chunk, a ragged k-step inside a chunk,
    and four chunks with a ragged last one; G and gbias start from random contents; ldy / ldx / ldg padded."""
    Nout, Kin = shape
    rng = _rng(10, Nout, Kin, M, with_gbias)
    ldy, ldx, ldg = Nout + 4, Kin + 4, Kin + 3
    dY, X = _In(dev, rng, M * ldy + 8), _In(dev, rng, M * ldx + 8)
    mm = np.arange(M)[:, None]
    gi = 5 + np.arange(Nout)[:, None] * ldg + np.arange(Kin)[None, :]
    G = _Out(dev, 5 + (Nout + 1) * ldg, gi, rng.standard_normal(gi.shape))
    gb = _Out(dev, Nout + 6, 3 + np.arange(Nout), rng.standard_normal(Nout))
    L.check(L.lib().seeme_wgrad128(dY.ptr(), ldy, X.ptr(), ldx, M, Nout, Kin, G.ptr(5), ldg, gb.ptr(3) if with_gbias else 0, _st()),
            "seeme_wgrad128")
    ref, mag, rb, bmag = R.wgrad128(dY.h[mm * ldy + np.arange(Nout)[None, :]], X.h[mm * ldx + np.arange(Kin)[None, :]], G.init(), gb.init())
    _within(G.read(), ref, R.sum_bound(M + 1, mag, ref), f"wgrad128 {shape} M={M} G")
    if with_gbias:
        _within(gb.read(), rb, R.sum_bound(M + 1, bmag, rb), f"wgrad128 {shape} M={M} gbias")
    else:
        assert gb.untouched()


# ============================================================================= stage-1 row kernels
EPS32 = float(np.float32(1e-5))


def _group_bound(f32, ref, labels):
    """row_bound for an output without rows (rstd): E is the largest float32 error among the entries with the same label (rows drawn
    alike: ordinary, large-mean, constant)."""
    f32, ref, labels = np.asarray(f32, np.float64), np.asarray(ref, np.float64), np.asarray(labels)
    E = np.zeros(ref.shape)
    for l in np.unique(labels):
        E[labels == l] = np.abs(f32 - ref)[labels == l].max()
    return 4 * E + 4 * R.U * np.abs(ref)


def _add_ln_case(M, with_res, ssr):
    rng = _rng(11, M, with_res, ssr)
    sub = (rng.standard_normal((M // ssr if ssr else M, 256)) * 1.5 + 0.25).astype(F32)
    res = rng.standard_normal((M, 256)).astype(F32) if with_res else None
    labels = np.zeros(M, int)
    if M >= 4 and not ssr:
        # mean 1e3, spread ~0.3, every entry a multiple of 1/16: the 256-term sum is exact in float32 in ANY order (partial sums are
        # multiples of 1/16 below 2^18), so the row's statistics do not depend on the reduction tree and the row rule applies as to
        # any other row -- while a one-pass E[x^2] - mean^2 variance (1e6 against 0.03) would be lost entirely
        sub[2] = (1000.0 + rng.integers(-8, 9, 256) / 16.0).astype(F32)
        sub[3] = 2.0                                                              # a constant row (3.25 with the residual)
        if with_res:
            res[2] = (rng.integers(-4, 5, 256) / 16.0).astype(F32)
            res[3] = 1.25
        labels[2], labels[3] = 1, 2
    gamma, beta = rng.standard_normal(256).astype(F32), rng.standard_normal(256).astype(F32)
    ref = R.vt_add_ln(sub, res, gamma, beta, M, ssr, EPS32)
    f32 = R.vt_add_ln(sub, res, gamma, beta, M, ssr, EPS32, F32)
    return sub, res, gamma, beta, labels, ref, f32


ADD_LN_CASES = [(M, r, 0) for M in (1, 4, 5, 33) for r in (0, 1)] + [(21, 0, 7), (21, 1, 7)]


@pytest.mark.parametrize("M,with_res,ssr", ADD_LN_CASES)
def test_vt_add_ln(dev, M, with_res, ssr):
    """Fewer rows than a block, a whole block, one row into the second, several blocks; the broadcast of one sub row per 7-row sequence.
    Row 2 has mean 1e3 and spread 0.3, row 3 is constant: xhat exactly 0, y exactly beta, rstd = 1/sqrt(eps).
    float32 numpy vs float64 (CPU, these inputs), largest over the cases: ordinary rows y 1.4e-6, xhat 5.0e-7, rstd 6.6e-8; the
    mean-1e3 row y 7.4e-7, xhat 4.0e-7, rstd 4.3e-7; the constant row 0, 0, rstd 1.3e-5 (one ulp of 316.2)."""
    sub, res, gamma, beta, labels, ref, f32 = _add_ln_case(M, with_res, ssr)
    rows = np.arange(M)[:, None] * 256 + np.arange(256)[None, :]
    y, xh, rs = _Out(dev, (M + 1) * 256, rows), _Out(dev, (M + 1) * 256, rows), _Out(dev, M + 3, np.arange(M))
    ts, tr, tg, tb = _in(dev, sub), (_in(dev, res) if with_res else None), _in(dev, gamma), _in(dev, beta)
    a = L.VtLn()
    a.sub, a.res, a.gamma, a.beta, a.y, a.xhat, a.rstd = ts.data_ptr(), L.ptr(tr), tg.data_ptr(), tb.data_ptr(), y.ptr(), xh.ptr(), rs.ptr()
    a.M, a.sub_seq_rows, a.eps = M, ssr, 1e-5
    L.check(L.lib().seeme_vt_add_ln(C.byref(a), _st()), "seeme_vt_add_ln")
    gy, gx, gr = y.read(), xh.read(), rs.read()
    what = f"vt_add_ln M={M} res={with_res} ssr={ssr}"
    _within(gy, ref[0], R.row_bound(f32[0], ref[0]), what + " y")
    _within(gx, ref[1], R.row_bound(f32[1], ref[1]), what + " xhat")
    _within(gr, ref[2], _group_bound(f32[2], ref[2], labels), what + " rstd")
    if (labels == 2).any():
        assert (ref[1][3] == 0).all() and (gx[3] == 0).all() and np.array_equal(gy[3], beta)


def _ln_bwd_case(M, acc, with_dy2):
    rng = _rng(12, M, acc, with_dy2)
    v = rng.standard_normal((M, 256)) * 1.5 + 0.25
    gamma = rng.standard_normal(256).astype(F32)
    _, xhat, rstd = R.vt_add_ln(v, None, gamma, gamma, M, 0, EPS32)
    xhat, rstd = xhat.astype(F32), rstd.astype(F32)
    dy = rng.standard_normal((M, 256)).astype(F32)
    dy2 = rng.standard_normal((M, 256)).astype(F32) if with_dy2 else None
    dpre0, dg0, db0 = (rng.standard_normal(s).astype(F32) for s in ((M, 256), 256, 256))
    ref = R.vt_ln_bwd(dy, xhat, rstd, gamma, dy2, acc, dpre0, dg0, db0)
    f32 = R.vt_ln_bwd(dy, xhat, rstd, gamma, dy2, acc, dpre0, dg0, db0, F32)
    return dy, dy2, xhat, rstd, gamma, dpre0, dg0, db0, ref, f32


@pytest.mark.parametrize("M", [1, 31, 32, 33, 70])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("with_dy2", [0, 1])
def test_vt_ln_bwd(dev, M, acc, with_dy2):
    """One row, one short of a 32-row block, exactly one, one more, and three blocks with a wave that has no rows; dpre stored and
    accumulated; the second gradient dy2 NULL and set (it enters dpre AND both affine gradients).  dgamma / dbeta always accumulate:
    they start from random contents and take the sum bound with L = M + 1.
    float32 numpy vs float64 of dpre (CPU, these inputs): at most 5.5e-7 in any row without dy2, 1.0e-6 with."""
    dy, dy2, xhat, rstd, gamma, dpre0, dg0, db0, ref, f32 = _ln_bwd_case(M, acc, with_dy2)
    rows = np.arange(M)[:, None] * 256 + np.arange(256)[None, :]
    dpre = _Out(dev, (M + 1) * 256, rows, dpre0 if acc else None)
    dg, db = _Out(dev, 260, np.arange(256), dg0), _Out(dev, 260, np.arange(256), db0)
    t = [_in(dev, x) for x in (dy, xhat, rstd, gamma)] + ([_in(dev, dy2)] if with_dy2 else [])
    a = L.VtLnBwd()
    a.dy, a.xhat, a.rstd, a.gamma, a.dpre, a.dgamma, a.dbeta = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), dpre.ptr(), dg.ptr(), db.ptr()
    a.M, a.accumulate, a.dy2 = M, acc, t[4].data_ptr() if with_dy2 else 0
    L.check(L.lib().seeme_vt_ln_bwd(C.byref(a), _st()), "seeme_vt_ln_bwd")
    what = f"vt_ln_bwd M={M} acc={acc} dy2={with_dy2}"
    _within(dpre.read(), ref[0], R.row_bound(f32[0], ref[0]), what + " dpre")
    _within(dg.read(), ref[1], R.sum_bound(M + 1, ref[3], ref[1]), what + " dgamma")
    _within(db.read(), ref[2], R.sum_bound(M + 1, ref[4], ref[2]), what + " dbeta")


SOFTMAX_S = [1, 2, 63, 64, 65, 130, 512]
SM_SCALE = 1.0 / 16.0


def _softmax_case(S, n_prefix):
    """B = 3 with n = min(S, n_prefix + 1) (n = 1 without a prefix), a mid n, and n_prefix + length > S, which clamps to n = S.
    Masked inputs hold NaN.  Row 0 of the last sequence has scores of +-1e3 before scaling."""
    rng = _rng(13, S, n_prefix)
    lengths = np.array([1, max(S // 2 - n_prefix, 1), S + 3], np.int32)
    ns = R.softmax_valid(lengths, S, n_prefix)
    assert ns[2] == S and ns[0] == min(S, n_prefix + 1)
    s = (rng.standard_normal((3, S, S)) * 8).astype(F32)
    s[2, 0] = np.where(rng.integers(0, 2, S) == 1, 1e3, -1e3).astype(F32)
    if S > 1:
        s[2, 0, :2] = (1e3, -1e3)
    valid = np.zeros((3, S, S), bool)
    for b, n in enumerate(ns):
        valid[b, :, :n] = True
    s[~valid] = np.nan
    ref = R.vt_softmax_fwd(s, lengths, n_prefix, SM_SCALE)
    f32 = R.vt_softmax_fwd(s, lengths, n_prefix, SM_SCALE, F32)
    return s, lengths, valid, ref, f32


@pytest.mark.parametrize("S", SOFTMAX_S)
@pytest.mark.parametrize("n_prefix", [0, 2])
def test_vt_softmax_fwd(dev, S, n_prefix):
    """S below, at and above one 64-lane column step, two steps and a bit, and all eight; masked positions hold NaN on input and must
    come out as exact zeros.  float32 numpy vs float64 (CPU, these inputs): at most 6.6e-8 in any row (probabilities <= 1)."""
    s, lengths, valid, ref, f32 = _softmax_case(S, n_prefix)
    buf = _Out(dev, 3 * S * S + 9, np.arange(3 * S * S).reshape(3, S, S), s)
    tl = _in(dev, lengths)
    L.check(L.lib().seeme_vt_softmax_fwd(buf.ptr(), tl.data_ptr(), 3, S, n_prefix, SM_SCALE, _st()), "seeme_vt_softmax_fwd")
    got = buf.read()
    assert (got.view(np.int32)[~valid] == 0).all(), "masked positions must be exact zeros"
    _within(got, ref, R.row_bound(f32, ref), f"vt_softmax_fwd S={S} n_prefix={n_prefix}")


def test_vt_softmax_refuses_S_513(dev):
    S = 513
    buf = _Out(dev, 4 * S + 8, np.arange(S), np.zeros(S))
    tl = _in(dev, np.array([S], np.int32))
    p = _in(dev, np.zeros(4 * S, F32))
    with pytest.raises(L.SeemeError):
        L.check(L.lib().seeme_vt_softmax_fwd(buf.ptr(), tl.data_ptr(), 1, S, 0, SM_SCALE, _st()), "seeme_vt_softmax_fwd")
    with pytest.raises(L.SeemeError):
        L.check(L.lib().seeme_vt_softmax_bwd(buf.ptr(), p.data_ptr(), 1, S, SM_SCALE, _st()), "seeme_vt_softmax_bwd")
    assert buf.untouched()


def _softmax_bwd_case(S):
    rng = _rng(14, S)
    _, _, _, p64, _ = _softmax_case(S, 0)
    rows = 3 * S - 1 if (3 * S - 1) % 4 else 3 * S - 2
    p = p64.reshape(3 * S, S)[:rows].astype(F32)                     # the forward's probabilities: masked zeros are present
    dp = rng.standard_normal((rows, S)).astype(F32)
    return rows, p, dp, R.vt_softmax_bwd(dp, p, SM_SCALE), R.vt_softmax_bwd(dp, p, SM_SCALE, F32)


@pytest.mark.parametrize("S", SOFTMAX_S)
def test_vt_softmax_bwd(dev, S):
    """The same S; rows not a multiple of the 4 rows of a block; p from the forward, masked zeros included (their gradient is an exact
    zero).  float32 numpy vs float64 (CPU, these inputs): at most 9.1e-10 in any row (|dS| is scale * p * O(1) ~ 1e-2)."""
    rows, p, dp, ref, f32 = _softmax_bwd_case(S)
    assert rows % 4 and rows >= 1
    buf = _Out(dev, (rows + 2) * S + 3, np.arange(rows * S).reshape(rows, S), dp)
    tp = _in(dev, p)
    L.check(L.lib().seeme_vt_softmax_bwd(buf.ptr(), tp.data_ptr(), rows, S, SM_SCALE, _st()), "seeme_vt_softmax_bwd")
    got = buf.read()
    assert (got[p == 0] == 0).all()
    _within(got, ref, R.row_bound(f32, ref), f"vt_softmax_bwd S={S} rows={rows}")


def _gelu_case(n):
    rng = _rng(15, n)
    x = np.linspace(-10, 10, n).astype(F32) if n > 1 else np.zeros(1, F32)
    x[n // 2] = 0.0
    dh = rng.standard_normal(n).astype(F32)
    return x, dh, (R.vt_gelu(x), R.vt_gelu(x, dh)), (R.vt_gelu(x, None, F32), R.vt_gelu(x, dh, F32))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_vt_gelu_forward_and_backward(dev, n):
    """One short of a block, a block, one more; x over [-10, 10] and an exact 0.  An element-wise kernel has no rows: E is the largest
    float32 error of the tensor.  float32 numpy (torch erff) vs float64 (CPU, these inputs): forward 4.1e-7, backward 2.7e-7 (n >= 255);
    0 at n = 1, where gelu(0) = 0 and gelu'(0) = 1/2 are exact."""
    x, dh, ref, f32 = _gelu_case(n)
    tx, td = _in(dev, x), _in(dev, dh)
    for k, name in ((0, "forward"), (1, "backward")):
        out = _Out(dev, n + 7, np.arange(n))
        L.check(L.lib().seeme_vt_gelu(tx.data_ptr(), td.data_ptr() if k else 0, out.ptr(), n, _st()), "seeme_vt_gelu")
        _within(out.read(), ref[k], R.row_bound(f32[k], ref[k], axis=None), f"vt_gelu {name} n={n}")


@pytest.mark.parametrize("S", [1, 7, 70])
@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("acc", [0, 1])
def test_vt_seq_sum(dev, S, masked, acc):
    """B = 3; wmask NULL (weights 1) or mixed, with sequence 1 masked entirely (its sum is an exact zero, or its old contents when
    accumulating); store and accumulate.  Sum bound with L = S + 1."""
    rng = _rng(16, S, masked, acc)
    B, scale = 3, float(np.float32(1.0 / 0.9))
    d = rng.standard_normal((B, S, 256)).astype(F32)
    out0 = rng.standard_normal((B, 256)).astype(F32)
    wm = rng.choice(np.array([0, 1, 255], np.uint8), (B, S))
    wm[1] = 0
    wm[2, 0] = 1
    out = _Out(dev, (B + 1) * 256, np.arange(B * 256).reshape(B, 256), out0 if acc else None)
    td, tw = _in(dev, d), _in(dev, wm)
    L.check(L.lib().seeme_vt_seq_sum(td.data_ptr(), out.ptr(), B, S, acc, tw.data_ptr() if masked else 0, scale, _st()), "seeme_vt_seq_sum")
    ref, mag = R.vt_seq_sum(d, out0, acc, wm if masked else None, scale)
    got = out.read()
    _within(got, ref, R.sum_bound(S + 1, mag, ref), f"vt_seq_sum S={S} masked={masked} acc={acc}")
    if masked:
        assert np.array_equal(got[1], out0[1] if acc else np.zeros(256, F32))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1027])
@pytest.mark.parametrize("in_place", [0, 1])
def test_vt_dropout_is_one_rounding(dev, n, in_place):
    """The float4 body and the scalar tail (n = 4q + 0..3, below and across one 1024-element block); mask bytes from {0, 1, 255}; out
    of place and in place.  Bit-exact against float32(x) * float32(scale): the operation is a single rounding."""
    rng = _rng(17, n, in_place)
    scale = float(np.float32(1.0 / 0.9))
    x = rng.standard_normal(n).astype(F32)
    m = rng.choice(np.array([0, 1, 255], np.uint8), n)
    m[0] = 255
    out = _Out(dev, n + 9, np.arange(n), x if in_place else None)
    tx, tm = _in(dev, x), _in(dev, np.concatenate([m, np.full(8, 1, np.uint8)]))
    L.check(L.lib().seeme_vt_dropout(out.ptr() if in_place else tx.data_ptr(), tm.data_ptr(), scale, out.ptr(), n, _st()), "seeme_vt_dropout")
    got, want = out.read(), R.vt_dropout(x, m, scale)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_vt_cross_rows(dev):
    """B = 3, S = 5.  float32 numpy vs float64 (CPU, these inputs): at most 4.4e-7 in any row; a row whose m2 is all zero is exactly 0."""
    rng = _rng(18)
    B, S, scale = 3, 5, float(np.float32(1.0 / 0.9))
    cvn, bo = rng.standard_normal((B, 256)).astype(F32), rng.standard_normal(256).astype(F32)
    wm = rng.choice(np.array([0, 1, 255], np.uint8), (B, S))
    wm[0, :2] = (0, 1)
    m2 = rng.choice(np.array([0, 1, 255], np.uint8), (B, S, 256))
    m2[1, 1] = 0
    out = _Out(dev, (B * S + 1) * 256, np.arange(B * S * 256).reshape(B, S, 256))
    t = [_in(dev, x) for x in (cvn, bo, wm, m2)]
    L.check(L.lib().seeme_vt_cross_rows(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), scale, B, S, out.ptr(), _st()),
            "seeme_vt_cross_rows")
    ref, f32 = R.vt_cross_rows(cvn, bo, wm, m2, scale), R.vt_cross_rows(cvn, bo, wm, m2, scale, F32)
    got = out.read()
    assert (got[1, 1] == 0).all() and (got[m2 == 0] == 0).all()
    _within(got, ref, R.row_bound(f32, ref), "vt_cross_rows")


# ============================================================================= stage-2 glue
def _acp():
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas).astype(F32)


def _glue_rows_case(B, N, mode, flip):
    rng = _rng(19, B, N, ["none", "first", "last"].index(mode), flip)
    rows = 2 * B + 3
    dist = rng.standard_normal((2, rows, 256)).astype(F32)
    eps_z, eps_c, noise = (rng.standard_normal((B, 256)).astype(F32) for _ in range(3))
    slot = {"none": 0, "first": 0, "last": N - 1}[mode]
    cond0 = np.full((B, N, 256), SENT, F32)
    t = np.array([0, 999, 1, 500, 37][:B] if B > 1 else [999 if flip else 0], np.int64)
    freq = np.exp(-np.log(10000.0) * np.arange(128, dtype=np.float64) / 128).astype(F32)
    args = (B, N, dist, eps_z, None if mode == "none" else eps_c, slot, cond0, noise, t, _acp(), freq, flip)
    return args, rows, R.glue_rows(*args), R.glue_rows(*args, dtype=F32)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["none", "first", "last"])
def test_glue_rows(dev, B, N, mode):
    """eps_c NULL (cond untouched), and set with the condition latent in the first / last of N token slots (the other slots keep their
    bits); dist_rows = 2B + 3; both feature orders; timesteps 0 and 999 included.
    float32 numpy vs float64 (CPU, these inputs), largest row: latents 1.2e-6, noisy 1.5e-6, tfeat 5.4e-8, cond 1.2e-6."""
    for flip in (0, 1):
        (B_, N_, dist, eps_z, eps_c, slot, cond0, noise, t, acp, freq, _), rows, ref, f32 = _glue_rows_case(B, N, mode, flip)
        r256 = np.arange(B)[:, None] * 256 + np.arange(256)[None, :]
        lat, noisy, tf = (_Out(dev, (B + 1) * 256, r256) for _ in range(3))
        cidx = (np.arange(B)[:, None] * N + slot) * 256 + np.arange(256)[None, :]
        cond = _Out(dev, (B * N + 1) * 256, cidx)
        ti = [_in(dev, x) for x in (dist, eps_z, noise, t, acp, freq)] + ([_in(dev, eps_c)] if eps_c is not None else [])
        a = L.GlueRows()
        a.B, a.N, a.dist, a.dist_rows, a.eps_z = B, N, ti[0].data_ptr(), rows, ti[1].data_ptr()
        a.eps_c, a.slot_c, a.cond = (ti[6].data_ptr() if eps_c is not None else 0), slot, cond.ptr()
        a.noise, a.timesteps, a.acp, a.freq, a.flip_sin_to_cos = ti[2].data_ptr(), ti[3].data_ptr(), ti[4].data_ptr(), ti[5].data_ptr(), flip
        a.latents, a.noisy, a.tfeat = lat.ptr(), noisy.ptr(), tf.ptr()
        L.check(L.lib().seeme_glue_rows(C.byref(a), _st()), "seeme_glue_rows")
        what = f"glue_rows B={B} N={N} {mode} flip={flip}"
        for k, (o, name) in enumerate(((lat, "latents"), (noisy, "noisy"), (tf, "tfeat"))):
            _within(o.read(), ref[k], R.row_bound(f32[k], ref[k]), f"{what} {name}")
        if eps_c is None:
            assert cond.untouched()
        else:
            _within(cond.read(), ref[3][:, slot], R.row_bound(f32[3][:, slot], ref[3][:, slot]), what + " cond slot")


@pytest.mark.parametrize("what", ["N=5", "dist_rows<2B"])
def test_glue_rows_refusals(dev, what):
    B, N = 2, 4
    (_, _, dist, eps_z, eps_c, slot, _, noise, t, acp, freq, _), rows, _, _ = _glue_rows_case(B, N, "first", 0)
    outs = [_Out(dev, (B * 5 + 1) * 256, np.arange(1)) for _ in range(4)]
    ti = [_in(dev, x) for x in (dist, eps_z, noise, t, acp, freq, eps_c)]
    a = L.GlueRows()
    a.B, a.N, a.dist, a.dist_rows, a.eps_z = B, (5 if what == "N=5" else N), ti[0].data_ptr(), (rows if what == "N=5" else 2 * B - 1), ti[1].data_ptr()
    a.eps_c, a.slot_c, a.cond = ti[6].data_ptr(), slot, outs[3].ptr()
    a.noise, a.timesteps, a.acp, a.freq, a.flip_sin_to_cos = ti[2].data_ptr(), ti[3].data_ptr(), ti[4].data_ptr(), ti[5].data_ptr(), 0
    a.latents, a.noisy, a.tfeat = outs[0].ptr(), outs[1].ptr(), outs[2].ptr()
    with pytest.raises(L.SeemeError):
        L.check(L.lib().seeme_glue_rows(C.byref(a), _st()), "seeme_glue_rows")
    assert all(o.untouched() for o in outs)


def _glue_ln_case(M):
    x = (_rng(20, M).standard_normal((M, 256)) * 1.5 + 0.25).astype(F32)
    return x, R.glue_ln(x), R.glue_ln(x, F32)


@pytest.mark.parametrize("M", [1, 6])
def test_glue_ln(dev, M):
    """float32 numpy vs float64 (CPU, these inputs): xhat at most 4.5e-7 in any row, rstd 3.7e-8."""
    x, ref, f32 = _glue_ln_case(M)
    xh, rs = _Out(dev, (M + 1) * 256, np.arange(M * 256).reshape(M, 256)), _Out(dev, M + 3, np.arange(M))
    tx = _in(dev, x)
    L.check(L.lib().seeme_glue_ln(tx.data_ptr(), xh.ptr(), rs.ptr(), M, _st()), "seeme_glue_ln")
    _within(xh.read(), ref[0], R.row_bound(f32[0], ref[0]), f"glue_ln M={M} xhat")
    _within(rs.read(), ref[1], R.row_bound(f32[1], ref[1], axis=None), f"glue_ln M={M} rstd")


def _glue_mid_case(M, B):
    rng = _rng(21, M, B)
    g = lambda *s: rng.standard_normal(s).astype(F32)
    xhat, rstd = R.glue_ln(g(M, 256) * 1.5)
    ins = dict(dxl=g(5, M, 256), dcs=g(5, M, 256), xhat=xhat.astype(F32), rstd=rstd.astype(F32), tn_w=g(5, 256), g_tn_w0=g(5, 256),
               g_tn_b0=g(5, 256), dea=g(5, B, 256), deb=g(10, B, 256), emb=g(B, 256))
    return ins, R.glue_mid(**ins), R.glue_mid(**ins, dtype=F32)


@pytest.mark.parametrize("M,B", [(1, 1), (6, 3)])
def test_glue_mid(dev, M, B):
    """dcond and demb by the row rule; the text_norm affine gradients accumulate onto random contents and take the sum bound (L = M + 1).
    float32 numpy vs float64 (CPU, these inputs), largest row: dcond 7.9e-7, demb 9.8e-7."""
    ins, ref, f32 = _glue_mid_case(M, B)
    t = {k: _in(dev, v) for k, v in ins.items()}
    i256 = np.arange(256)
    gw = [_Out(dev, 260, i256, ins["g_tn_w0"][l]) for l in range(5)]
    gb = [_Out(dev, 260, i256, ins["g_tn_b0"][l]) for l in range(5)]
    dcond = _Out(dev, (M + 1) * 256, np.arange(M * 256).reshape(M, 256))
    demb = _Out(dev, (B + 1) * 256, np.arange(B * 256).reshape(B, 256))
    a = L.GlueMid()
    a.M, a.B = M, B
    a.dxl, a.dcs, a.xhat, a.rstd = (t[k].data_ptr() for k in ("dxl", "dcs", "xhat", "rstd"))
    for l in range(5):
        a.tn_w[l], a.g_tn_w[l], a.g_tn_b[l] = t["tn_w"].data_ptr() + 4 * 256 * l, gw[l].ptr(), gb[l].ptr()
    a.dcond, a.dea, a.deb, a.emb, a.demb = dcond.ptr(), t["dea"].data_ptr(), t["deb"].data_ptr(), t["emb"].data_ptr(), demb.ptr()
    L.check(L.lib().seeme_glue_mid(C.byref(a), _st()), "seeme_glue_mid")
    what = f"glue_mid M={M} B={B}"
    _within(dcond.read(), ref[0], R.row_bound(f32[0], ref[0]), what + " dcond")
    _within(demb.read(), ref[3], R.row_bound(f32[3], ref[3]), what + " demb")
    _within(np.stack([o.read() for o in gw]), ref[1], R.sum_bound(M + 1, ref[4], ref[1]), what + " g_tn_w")
    _within(np.stack([o.read() for o in gb]), ref[2], R.sum_bound(M + 1, ref[5], ref[2]), what + " g_tn_b")


# ============================================================================= denoiser chain gradients
LDG = 700
WGRAD_TILES = [(5, 300, 3, 1, 1, 2), (10, 400, 260, 32, 256, 16), (290, 450, 103, 17, 100, 16 + 32 * 260 + 8)]
WGRAD_OUT = 16 + 32 * 260 + 8 + 17 * 103 + 11


def _tile_table(dev, tiles):
    dt = np.dtype([("x_col", "<i4"), ("y_col", "<i4"), ("ldo", "<i4"), ("nn", "<i4"), ("kk", "<i4"), ("pad", "<i4"), ("out_off", "<i8")])
    assert dt.itemsize == 32
    arr = np.zeros(len(tiles), dt)
    for i, (x, y, ldo, nn, kk, off) in enumerate(tiles):
        assert nn <= 32 and kk <= 256 and ldo >= kk and x + kk <= LDG and y + nn <= LDG and off + (nn - 1) * ldo + kk <= WGRAD_OUT
        arr[i] = (x, y, ldo, nn, kk, 0, off)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(dev)


@pytest.mark.parametrize("B", [1, 8, 9, 64, 65, 130])
def test_den_wgrad(dev, B):
    """A tile table mixing (nn, kk) = (1,1), (32,256), (17,100), ldo > kk, over B below / at / above the 8-sample inner step and the
    64-sample LDS block.  `out` outside the tiles (the ldo - kk gap of every row included) keeps its bits; two launches give the same
    bits (fixed summation order)."""
    rng = _rng(22, B)
    g = _In(dev, rng, B * LDG)
    tt = _tile_table(dev, WGRAD_TILES)
    idx = np.concatenate([(off + np.arange(nn)[:, None] * ldo + np.arange(kk)[None, :]).ravel() for _, _, ldo, nn, kk, off in WGRAD_TILES])
    outs = [_Out(dev, WGRAD_OUT, idx) for _ in range(2)]
    for o in outs:
        L.check(L.lib().seeme_den_wgrad(g.ptr(), LDG, B, tt.data_ptr(), len(WGRAD_TILES), o.ptr(), _st()), "seeme_den_wgrad")
    ref, mag = R.den_wgrad(g.h.reshape(B, LDG), WGRAD_TILES, outs[0].before)
    got = outs[0].read()
    _within(got, ref[idx], R.sum_bound(B, mag[idx], ref[idx]), f"den_wgrad B={B}")
    assert np.array_equal(got.view(np.int32), outs[1].read().view(np.int32)), "two launches differ"


@pytest.mark.parametrize("n", [1, 255, 256, 300])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("with_dpe", [0, 1])
def test_den_vecgrad(dev, n, B, with_dpe):
    """Gather-reduce with repeated indices, n around one 256-thread block; the query_pos.pe row NULL (nothing written) and set."""
    rng = _rng(23, n, B, with_dpe)
    g = _In(dev, rng, B * LDG)
    idx = rng.integers(0, LDG, n).astype(np.int64)
    idx[n // 2] = idx[0]
    if n > 2:
        idx[-1], idx[1] = LDG - 1, 0
    out, dpe = _Out(dev, n + 5, np.arange(n)), _Out(dev, 256 + 5, np.arange(256))
    ti = _in(dev, idx)
    L.check(L.lib().seeme_den_vecgrad(g.ptr(), LDG, B, ti.data_ptr(), n, out.ptr(), 17, dpe.ptr() if with_dpe else 0, _st()), "seeme_den_vecgrad")
    ro, mo, rp, mp = R.den_vecgrad(g.h.reshape(B, LDG), idx, 17)
    _within(out.read(), ro, R.sum_bound(B, mo, ro), f"den_vecgrad n={n} B={B} out")
    if with_dpe:
        _within(dpe.read(), rp, R.sum_bound(B, mp, rp), f"den_vecgrad n={n} B={B} dpe_row0")
    else:
        assert dpe.untouched()
