"""ResnetPointnet -- drop-in for ``EgoHMR.models.respointnet.ResnetPointnet`` (respointnet.py:6-97), the
frozen scene encoder MLD consumes through ``ProHMRScene.encode_scene`` (prohmr_scene.py:102-104;
mld/models/modeltype/mld.py:911-922).  Same parameter names (``fc_pos_0``, ``block_{0..3}.{fc_0,fc_1,shortcut}``,
``fc_c``) so the ``proscene.scene_enc.*`` entries of a checkpoint load; forward runs in libseeme_hip.so."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch
import torch.nn as nn

from . import _lib as L
from .mld_vae import _param_fingerprint


# what _weights() builds for one parameter fingerprint: the two ABI structs and the tensors their pointers refer to
_PackedWeights = namedtuple("_PackedWeights", "fingerprint w wb tensors")


class _ResnetBlockFCParams(nn.Module):
    def __init__(self, size_in, size_out, size_h):
        super().__init__()
        self.fc_0 = nn.Linear(size_in, size_h)
        self.fc_1 = nn.Linear(size_h, size_out)
        self.shortcut = nn.Linear(size_in, size_out, bias=False)
        nn.init.zeros_(self.fc_1.weight)            # respointnet.py:86


class ResnetPointnet(nn.Module):
    def __init__(self, out_dim: int = 512, hidden_dim: int = 256, precision: str = "fp32"):
        super().__init__()
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' (fp32 MFMA, parity path) or 'bf16' (fused bf16-MFMA blocks)")
        self.precision = precision
        if hidden_dim != 256:
            raise NotImplementedError("accelerated path: hidden_dim 256 (ProHMRScene builds ResnetPointnet(512, 256))")
        self.out_dim = out_dim
        self.fc_pos_0 = nn.Linear(3, 2 * hidden_dim)
        for i in range(4):
            setattr(self, f"block_{i}", _ResnetBlockFCParams(2 * hidden_dim, hidden_dim, hidden_dim))
        self.fc_c = nn.Linear(hidden_dim, out_dim)
        self._wcache = None
        self._ws = L.Workspace(per_stream=False)

    def _weights(self):
        fpnt = _param_fingerprint(self)
        if self._wcache is not None and self._wcache.fingerprint == fpnt:
            return self._wcache.w
        for p in self.parameters():
            L.require_cuda(p, "ResnetPointnet parameter")
        with torch.no_grad():
            posw = torch.zeros(512, 16, device=self.fc_pos_0.weight.device, dtype=torch.float32)
            posw[:, :3] = self.fc_pos_0.weight
        w = L.PointnetWeights()
        w.out_dim = self.out_dim
        w.pos_w, w.pos_b = posw.data_ptr(), L.ptr(self.fc_pos_0.bias)
        for i in range(4):
            blk = getattr(self, f"block_{i}")
            w.fc0_w[i], w.fc0_b[i] = L.ptr(blk.fc_0.weight), L.ptr(blk.fc_0.bias)
            w.fc1_w[i], w.fc1_b[i] = L.ptr(blk.fc_1.weight), L.ptr(blk.fc_1.bias)
            w.sc_w[i] = L.ptr(blk.shortcut.weight)
        w.fcc_w, w.fcc_b = L.ptr(self.fc_c.weight), L.ptr(self.fc_c.bias)
        with torch.no_grad():
            bf = [getattr(self, f"block_{i}") for i in range(4)]
            # block_0's shortcut acts on fc_pos_0(p): two linear maps, folded in fp64 to a 3 -> 256 map
            ws0 = bf[0].shortcut.weight.double()
            sc3 = torch.cat([ws0 @ self.fc_pos_0.weight.double(), (ws0 @ self.fc_pos_0.bias.double())[:, None]], dim=1).float().contiguous()
            posf = self._split_frags(self.fc_pos_0.weight.float(), self.fc_pos_0.bias.float())
            streams, sc3f = self._pack_streams(bf, sc3)
        wb = L.PointnetBf16()
        for i in range(4):
            wb.stream[i] = streams[i].data_ptr()
        wb.posf, wb.sc3f = posf.data_ptr(), sc3f.data_ptr()
        # the structs hold raw pointers: the tensors they point into stay alive with them
        self._wcache = _PackedWeights(fpnt, w, wb, (posw, posf, streams, sc3f))
        return w

    @staticmethod
    def _split_frags(W3, bias):
        """A 3 -> N map (W3 [N, 3], bias [N]) as split-bf16 matrix-core operands, v = hi + lo (include/seeme_hip.h:
        SeemePointnetBf16.posf): [N/16 n-tiles][kq][q][4], k slots per kq 0: whx why whz whx | 1: why whz wlx wly |
        2: wlz bh bl 0 | 3: zeros."""
        wh, bh = W3.to(torch.bfloat16), bias.to(torch.bfloat16)
        wl, bl = (W3 - wh.float()).to(torch.bfloat16), (bias - bh.float()).to(torch.bfloat16)
        zz = torch.zeros_like(bh)
        frag = torch.stack([torch.stack([wh[:, 0], wh[:, 1], wh[:, 2], wh[:, 0]], -1),
                            torch.stack([wh[:, 1], wh[:, 2], wl[:, 0], wl[:, 1]], -1),
                            torch.stack([wl[:, 2], bh, bl, zz], -1),
                            torch.stack([zz, zz, zz, zz], -1)], dim=1)                 # [N, kq, 4]
        return frag.view(-1, 16, 4, 4).permute(0, 2, 1, 3).contiguous()

    @staticmethod
    def _pack_streams(bf, sc3):
        """Weight streams of the block kernel k_pn_block2 (include/seeme_hip.h: SeemePointnetBf16.stream): per block
        24 slots x 16 fragments x 64 lanes x 8 bf16 in the order a 256-point tile consumes them, and the folded block_0
        shortcut as split-bf16 fragments (sc3f)."""
        dev = sc3.device
        kq, m, j = torch.meshgrid(torch.arange(4), torch.arange(16), torch.arange(8), indexing="ij")     # lane = 16 kq + m
        # every B operand of these kernels is built from an accumulator tile pair (generated input, hidden tile, stored
        # activations): element j of lane (kq, .) of k-block kb is feature 32 kb + 16 (j/4) + 4 kq + j%4
        k_perm = (16 * (j // 4) + 4 * kq + j % 4).reshape(64, 8).to(dev)
        m_l = m.reshape(64, 8).to(dev)
        rows_nat = lambda nt: 16 * nt + m_l

        def frag(W, nt, kb):                # feature tile nt (rows 16 nt + m), k-block kb in the permuted k order
            return W[rows_nat(nt), 32 * kb + k_perm].to(torch.bfloat16)     # [64, 8]

        streams = []
        for i, b in enumerate(bf):
            W0, W1, Ws = b.fc_0.weight.float(), b.fc_1.weight.float(), b.shortcut.weight.float()
            if i == 0:      # slots 0..15: fc_0 k-block = slot; slot 16 + 4 g + p: fc_1 half g, fragment 8 kbi + n = tile 8 g + n, k-block 2 p + kbi
                slots = [torch.stack([frag(W0, nt, kb) for nt in range(16)]) for kb in range(16)]
                slots += [torch.stack([frag(W1, 8 * g + n, 2 * p + kbi) for kbi in range(2) for n in range(8)])
                          for g in range(2) for p in range(4)]
            else:           # slots 0..7: fc_0[:, :256]; slot 8 + 8 g + kb: shortcut[:, :256] tiles 8 g + n (fragments 0..7) | fc_1 (8..15)
                slots = [torch.stack([frag(W0, nt, kb) for nt in range(16)]) for kb in range(8)]
                for g in range(2):
                    slots += [torch.stack([frag(Ws, 8 * g + n, kb) for n in range(8)] + [frag(W1, 8 * g + n, kb) for n in range(8)])
                              for kb in range(8)]
            assert len(slots) == 24
            streams.append(torch.stack(slots).contiguous())             # [24, 16, 64, 8] bf16
        return streams, ResnetPointnet._split_frags(sc3[:, :3], sc3[:, 3])     # sc3 [256, 4] = (Ws Wp | Ws bp)

    def forward(self, p: torch.Tensor) -> torch.Tensor:
        """p [B, n_pts, 3] -> [B, out_dim]."""
        L.require_cuda(p, "points")
        B, P, three = p.shape
        assert three == 3
        p = p.contiguous()
        out = torch.empty(B, self.out_dim, device=p.device, dtype=torch.float32)
        bf16 = self.precision == "bf16"
        need = (L.lib().seeme_pointnet_bf16_workspace_bytes if bf16 else L.lib().seeme_pointnet_workspace_bytes)(B, P)
        ws = self._ws.get(need, p.device)
        w = self._weights()
        ev = getattr(self, "timing_events", None)       # (start, end) torch.cuda.Event pair: bench.py brackets the encode
        if ev is not None:
            ev[0].record()
        if bf16:
            L.call("seeme_pointnet_encode_bf16", C.byref(w), C.byref(self._wcache.wb), p.data_ptr(), B, P, out.data_ptr(),
                   ws.data_ptr(), ws.numel(), L.current_stream())
        else:
            L.call("seeme_pointnet_encode", C.byref(w), p.data_ptr(), B, P, out.data_ptr(), ws.data_ptr(), ws.numel(),
                   L.current_stream())
        if ev is not None:
            ev[1].record()
        return out
