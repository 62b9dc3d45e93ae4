"""seeme_denoiser_tables1 (csrc/den_kernels.hip, k_den_tables1): the condition tables of ONE condition token from one launch, against
the launches it replaces (seeme_denoiser_cond_tables, then seeme_denoiser_ca_tables = k_ca_rows + the batched proj_out), bit for
bit; its zero region; and MldDenoiser.sample_loop with the fused call on and off.

Shapes are the smallest at which the tiling of the new kernel can go wrong: a catab tile is 32 rows of rows = Bc R, its value GEMM
runs one m-tile up to 16 samples per tile and two above, a sample boundary may fall before, on or after a tile edge, and the last
tile may be partial.  Outputs live in sentinel-filled buffers with guard cells on both sides.  trow is never the identity: reversed,
one entry repeated, into a ttab with more rows than are used.

The sample_loop tests are the stale-tag check of the exchange buffer: with the fused call the table launch zeroes the buffer and
the cluster call skips its memset, so every later call on the same model (another batch size, a graph replay) has to find it zero.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from seeme_amd import _lib as L
from seeme_amd.mld_denoiser import MldDenoiser
from seeme_amd.schedulers import DDIMScheduler
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu
SENT = np.float32(-7.0e7)
LEAD = 8          # guard floats in front of an output (keeps the 16-byte alignment of the pointer handed to the kernel)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _no_env_switch(monkeypatch):
    monkeypatch.delenv("SEEME_DEN_TABLES", raising=False)
    monkeypatch.delenv("SEEME_DEN_CLUSTER", raising=False)


def _model(dev, **kw):
    abl = types.SimpleNamespace(MLP_DIST=False, PE_TYPE="mld", SKIP_CONNECT=True, VAE_TYPE="actor", DIFF_PE_TYPE="mld", MD_TRANS=True)
    return load_recipe_(MldDenoiser(abl, nfeats=75, condition=["text", "interactee"], latent_dim=[1, 256], ff_size=128, num_layers=5,
                                    num_heads=1, **kw)).to(dev).eval()


@pytest.fixture(scope="module")
def den(dev):
    return _model(dev)


def _noise(dev, seed, *shape):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32)).to(dev)


def _scheduler(steps=4):
    sch = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                        clip_sample=False, set_alpha_to_one=False, steps_offset=1)
    sch.set_timesteps(steps)
    return sch


class _Out:
    """n floats between LEAD guard floats in front and `tail` behind, sentinel everywhere (the pattern of tests/test_gpu_linear_edges.py)."""

    def __init__(self, dev, n, tail):
        self.n = n
        self.before = np.full(LEAD + n + tail, SENT, np.float32)
        self.t = torch.from_numpy(self.before.copy()).to(dev)

    def ptr(self):
        return self.t.data_ptr() + 4 * LEAD

    def read(self):
        torch.cuda.synchronize()
        after = self.t.cpu().numpy()
        assert np.array_equal(after[:LEAD].view(np.int32), self.before[:LEAD].view(np.int32)), "written in front of the output"
        assert np.array_equal(after[LEAD + self.n:].view(np.int32), self.before[LEAD + self.n:].view(np.int32)), "written behind the output"
        return after[LEAD:LEAD + self.n]


def _trow(dev, n_trow, n_rows):
    """reversed, entry 1 repeats entry 0, shifted into the upper rows of a ttab of n_rows > n_trow rows"""
    t = np.arange(n_trow)[::-1].copy() + (n_rows - n_trow)
    if n_trow > 1:
        t[1] = t[0]
    assert n_trow == 1 or not np.array_equal(t, np.arange(n_trow))
    return torch.from_numpy(t.astype(np.int32)).to(dev)


def _same_bits(x, y, what):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)), what


# (Bc, n_trow, trow_per_sample)
TABLE_CASES = [(1, 1, 0), (1, 1, 1),            # a single row, both index modes at R = 1
               (33, 1, 0), (33, 1, 1),          # tile 0 spans 32 samples (two m-tiles in the value GEMM), tile 1 has one row
               (17, 1, 0), (17, 1, 1),          # 17 samples: just over one m-tile
               (33, 5, 1),                      # R = 1 with row trow[bc % 5]
               (2, 31, 0), (2, 32, 0), (2, 33, 0),   # the sample boundary before, on and after a tile edge
               (3, 50, 0)]                      # the workload's R: a tile straddling two samples, partial last tile


@pytest.mark.parametrize("Bc,n_trow,per_sample", TABLE_CASES)
def test_tables1_equals_cond_tables_then_ca_tables(dev, den, Bc, n_trow, per_sample):
    w = den._weights()
    n_rows = n_trow + 3
    cond = _noise(dev, [41, Bc, n_trow], Bc, 1, 256)
    ttab = den.time_tables(_noise(dev, [42, n_trow], n_rows, 256))
    trow = _trow(dev, n_trow, n_rows)
    ctab_ref = den.cond_tables(cond)
    catab_ref = den.ca_tables(ctab_ref, ttab, trow, bool(per_sample))
    R_ = 1 if per_sample else n_trow
    ctab, catab = _Out(dev, Bc * L.CROW, L.CROW), _Out(dev, Bc * R_ * 1280, 1280)
    L.check(L.lib().seeme_denoiser_tables1(C.byref(w), cond.data_ptr(), ttab.data_ptr(), trow.data_ptr(), per_sample, n_trow, Bc,
                                           ctab.ptr(), catab.ptr(), 0, 0, L.current_stream()), "seeme_denoiser_tables1")
    got_c, got_ca = ctab.read(), catab.read()
    assert np.isfinite(got_ca).all()
    _same_bits(got_c, ctab_ref.cpu().numpy().reshape(-1), "ctab")
    _same_bits(got_ca, catab_ref.cpu().numpy().reshape(-1), "catab")


@pytest.mark.parametrize("nbytes", [7, 16, 4100, 700007])
def test_tables1_zero_region(dev, den, nbytes):
    """The zero region: exactly nbytes bytes, whatever the length (a tail that is no multiple of 16, more than the zero workgroups
    cover in one sweep); the tables of the same launch are what they are without it."""
    w = den._weights()
    cond, ttab, trow = _noise(dev, 43, 2, 1, 256), den.time_tables(_noise(dev, 44, 3, 256)), _trow(dev, 2, 3)
    ctab0, catab0 = den.tables1(cond, ttab, trow, False)
    buf = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device=dev)
    ctab1, catab1 = den.tables1(cond, ttab, trow, False, buf, nbytes)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert not h[:nbytes].any() and (h[nbytes:] == 0xAB).all()
    _same_bits(ctab1.cpu().numpy(), ctab0.cpu().numpy(), "ctab")
    _same_bits(catab1.cpu().numpy(), catab0.cpu().numpy(), "catab")
    with pytest.raises(L.SeemeError):       # a region that is not 16-byte aligned is refused
        den.tables1(cond, ttab, trow, False, buf[4:], 16)


def _sample(den, lat, cond, steps=4, guidance=1.0):
    out = den.sample_loop(lat, cond, _scheduler(steps), guidance_scale=guidance)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("cluster,guidance", [(8, 1.0), (0, 1.0), (0, 7.5)])
def test_sample_loop_fused_on_and_off(dev, cluster, guidance):
    """B = 3, 4 DDIM steps: the 8-CU cluster kernel, the one-CU kernel, and the one-CU kernel with a CFG pair (Bc = 2 B)."""
    den = _model(dev, cluster=cluster, weight_dtype="fp16")
    B = 3
    lat, cond = _noise(dev, 51, B, 1, 256), _noise(dev, 52, 2 * B if guidance > 1 else B, 1, 256)
    den.fused_tables = False
    off = _sample(den, lat, cond, guidance=guidance)
    assert den.cluster_status()[0] == 0
    den.fused_tables = True
    on = _sample(den, lat, cond, guidance=guidance)
    assert den.cluster_status()[0] == 0
    assert np.isfinite(on).all()
    _same_bits(on, off, "latents")


def test_sample_loop_calls_in_a_row_equal_fresh_models(dev):
    """Four calls on one model with different conditions and batch sizes: each finds the exchange buffer as a fresh model does."""
    den = _model(dev, weight_dtype="fp16")
    for i, B in enumerate((3, 1, 3, 2)):
        lat, cond = _noise(dev, [61, i], B, 1, 256), _noise(dev, [62, i], B, 1, 256)
        got = _sample(den, lat, cond)
        assert den.cluster_status()[0] == 0
        fresh = _model(dev, weight_dtype="fp16")
        ref = _sample(fresh, lat, cond)
        assert fresh.cluster_status()[0] == 0
        _same_bits(got, ref, f"call {i} (B = {B})")


def test_sample_loop_graph_replays(dev):
    """One capture of a B = 2, 4-step sample_loop, replayed twice with the condition buffer's contents changed in between: each
    replay zeroes the exchange buffer again (the table launch is part of the graph) and equals the eager result."""
    den = _model(dev, weight_dtype="fp16")
    B = 2
    lat, cond = _noise(dev, 71, B, 1, 256), _noise(dev, 72, B, 1, 256)
    sch = _scheduler(4)
    conds = [_noise(dev, 73, B, 1, 256), _noise(dev, 74, B, 1, 256)]
    eager = [_sample(den, lat, c) for c in conds]             # (also the warm-up: weight images, time tables, exchange buffer)
    side = torch.cuda.Stream()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        out = den.sample_loop(lat, cond, sch)
    torch.cuda.synchronize()
    for c, ref in zip(conds, eager):
        cond.copy_(c)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        _same_bits(out.cpu().numpy(), ref, "replay")
        assert den.cluster_status()[0] == 0
