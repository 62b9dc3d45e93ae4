"""One-launch AdamW step for the trainable tensors of ``MLD`` (``seeme_adamw_step``, csrc/misc_kernels.hip).

The reference trains with ``torch.optim.AdamW`` built in ``BaseModel.configure_optimizers`` (mld/models/modeltype/base.py)
and stepped by Lightning after ``training_step`` (train.py:127-149).  The ``torch.optim.AdamW`` object is kept -- it owns
the hyper-parameters the LR scheduler edits and the ``state_dict`` layout that goes into the checkpoints -- and only its
``step()`` is replaced: same arithmetic (decoupled weight decay, bias corrections, ``amsgrad`` off) on the same state
tensors (``exp_avg``, ``exp_avg_sq``, ``step``), in one kernel over all tensors instead of 27 multi-tensor launches.

Two options of the training loop ride on the same pass (``seeme_grad_norm`` + ``seeme_adamw_step_ex``): clipping of the global
gradient norm, whose scale goes from the reduction to the update through device memory, and an exponential moving average
(EMA) of the weights as a fifth stream of the update.  ``TorchAdamWStep`` is the same three steps in PyTorch operations (CPU
parameters, ``TRAIN.FUSED_ADAMW: false``) and ``reference_step_f64`` their float64 definition.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional

import torch

from . import _lib as L

_CHUNK = 16384      # elements per workgroup


def ema_decay_at(decay: float, warmup: bool, t: float) -> float:
    """d_t of update t (1-based): with warm-up min(d, (1 + t) / (10 + t)), so that a young average follows the weights closely."""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def check_options(ema_decay, grad_clip_norm, names=("ema_decay", "grad_clip_norm")):
    for v, name, ok in ((ema_decay, names[0], lambda x: 0.0 <= x < 1.0), (grad_clip_norm, names[1], lambda x: 0.0 <= x < math.inf)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(float(v)):
            raise ValueError(f"{name} must be a number in {'[0, 1)' if name == names[0] else '[0, inf)'} (0 = off), got {v!r}")
    return float(ema_decay), float(grad_clip_norm)


def clip_scale_torch(params: List[torch.nn.Parameter], max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ on COPIES of the gradients, which become ``p.grad`` (the caller puts the originals back
    after the step, so that they stay unscaled as on the HIP path).  Returns {norm, scale}."""
    for p in params:
        p.grad = p.grad.detach().clone()
    norm = torch.nn.utils.clip_grad_norm_(params, float(max_norm))
    return torch.stack([norm, torch.clamp(float(max_norm) / (norm + 1e-6), max=1.0)]).to(torch.float32)


def ema_update_torch(shadows: List[torch.Tensor], params: List[torch.Tensor], decay_t: float) -> None:
    """e.lerp_(p, 1 - d_t) over the list."""
    if shadows:
        torch._foreach_lerp_(shadows, [p.detach() for p in params], 1.0 - decay_t)


def reference_step_f64(p, g, m, v, e, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, ema_decay=0.0, ema_warmup=True,
                       grad_scale=None):
    """One update in float64 on lists of float64 tensors, in place: g' = g * scale, torch.optim.AdamW (amsgrad off) on g',
    e += (p_new - e) (1 - d_t).  `e` may be None (no EMA), `grad_scale` None (no clipping); t = the 1-based step count."""
    b1, b2 = betas
    d_t = ema_decay_at(ema_decay, ema_warmup, t)
    for i in range(len(p)):
        gi = g[i] if grad_scale is None else g[i] * grad_scale
        p[i].mul_(1.0 - lr * weight_decay)
        m[i].mul_(b1).add_(gi, alpha=1.0 - b1)
        v[i].mul_(b2).addcmul_(gi, gi, value=1.0 - b2)
        p[i].sub_(lr / (1.0 - b1 ** t) * m[i] / (v[i].sqrt() / math.sqrt(1.0 - b2 ** t) + eps))
        if e is not None:
            e[i].add_((p[i] - e[i]) * (1.0 - d_t))


class _EmaClipOptions:
    """What FusedAdamWStep and TorchAdamWStep share: the options, one fp32 shadow per parameter of the optimiser (whether or not
    it ever receives a gradient: one off the training path keeps a shadow equal to itself), the last {norm, scale}."""

    def _init_options(self, optimizer, ema_decay, ema_warmup, grad_clip_norm):
        self.ema_decay, self.grad_clip_norm = check_options(ema_decay, grad_clip_norm)
        self.ema_warmup = bool(ema_warmup)
        self.opt = optimizer
        self.shadow: Dict[torch.nn.Parameter, torch.Tensor] = {}
        self.last_grad_norm: Optional[torch.Tensor] = None     # {norm, scale} of the last step; reading it synchronises
        self._ensure_shadows()

    def _ensure_shadows(self):
        if self.ema_decay > 0.0:
            for group in self.opt.param_groups:
                for p in group["params"]:
                    if p not in self.shadow:
                        self.shadow[p] = p.detach().clone(memory_format=torch.contiguous_format)


class TorchAdamWStep(_EmaClipOptions):
    """clip_grad_norm_-style scaling, ``optimizer.step()`` and ``torch._foreach_lerp_``: the path for CPU parameters and
    ``TRAIN.FUSED_ADAMW: false``, and the twin of the HIP path.  Like it, ``p.grad`` is left unscaled after a clipped step: the
    scaled gradients are temporaries."""

    def __init__(self, optimizer, ema_decay: float = 0.0, ema_warmup: bool = True, grad_clip_norm: float = 0.0):
        self._init_options(optimizer, ema_decay, ema_warmup, grad_clip_norm)

    def note_replay(self):
        raise NotImplementedError("TorchAdamWStep cannot sit in a captured step")

    @torch.no_grad()
    def step(self, device_step: bool = False):
        self._ensure_shadows()
        params = [p for g in self.opt.param_groups for p in g["params"] if p.grad is not None]
        kept = None
        if self.grad_clip_norm > 0.0 and params:
            kept = [p.grad for p in params]
            self.last_grad_norm = clip_scale_torch(params, self.grad_clip_norm)
        self.opt.step()
        if kept is not None:
            for p, g in zip(params, kept):
                p.grad = g
        if self.ema_decay > 0.0 and params:
            t = float(self.opt.state[params[0]]["step"])
            ema_update_torch([self.shadow[p] for p in params], params, ema_decay_at(self.ema_decay, self.ema_warmup, t))


class FusedAdamWStep(_EmaClipOptions):
    def __init__(self, optimizer: torch.optim.AdamW, ema_decay: float = 0.0, ema_warmup: bool = True, grad_clip_norm: float = 0.0):
        """ema_decay d in [0, 1) (0 = off): a shadow e of every parameter follows e += (p_new - e) (1 - d_t), d_t = d or, with
        ema_warmup, min(d, (1 + t) / (10 + t)).  grad_clip_norm c (0 = off): the update sees g * min(1, c / (|g| + 1e-6)) with |g|
        the L2 norm over all gradients; ``p.grad`` itself is read and never written, so it stays UNSCALED after a clipped step
        (torch.nn.utils.clip_grad_norm_ scales it in place).  With both off, step() makes the calls it made before the options
        existed."""
        for g in optimizer.param_groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable"):
                raise NotImplementedError("FusedAdamWStep: amsgrad / maximize / capturable / differentiable AdamW")
        self._init_options(optimizer, ema_decay, ema_warmup, grad_clip_norm)
        if (self.ema_decay > 0.0 or self.grad_clip_norm > 0.0) and len(optimizer.param_groups) != 1:
            raise NotImplementedError("FusedAdamWStep: EMA / gradient clipping with more than one parameter group")
        self._key = None
        self._shared = {}
        self._dev_scalars, self._dev_lr = {}, {}
        self._updated: List[torch.nn.Parameter] = []
        self._force_ex = False         # True: seeme_adamw_step_ex also with both options off (equivalence tests, benchmarks)

    def _tables(self, params: List[torch.nn.Parameter]):
        """Static device tables (chunks, parameter / moment pointers); rebuilt when the tensors behind them change."""
        ema = self.ema_decay > 0.0
        key = tuple((p.data_ptr(), self.opt.state[p]["exp_avg"].data_ptr(), self.opt.state[p]["exp_avg_sq"].data_ptr()) +
                    ((self.shadow[p].data_ptr(),) if ema else ()) for p in params)
        if key == self._key:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamWStep: parameter or state addresses changed inside a graph capture (run warm-up steps first)")
        dev = params[0].device
        chunks = []
        for t, p in enumerate(params):
            n = p.numel()
            for off in range(0, n, _CHUNK):
                chunks.append((t, min(_CHUNK, n - off), off))
        assert all(off < 2 ** 31 for _, _, off in chunks)
        # {int tensor, int count, int64 offset}, little-endian: the offset's high word stays zero
        ch = torch.tensor([[t, cnt, off, 0] for t, cnt, off in chunks], dtype=torch.int32)
        self._chunks = ch.to(dev)
        self._n_chunks = len(chunks)
        ptr = lambda xs: torch.tensor(xs, dtype=torch.int64).to(dev)
        self._p = ptr([k[0] for k in key])
        self._m = ptr([k[1] for k in key])
        self._v = ptr([k[2] for k in key])
        self._e = ptr([k[3] for k in key]) if ema else None
        if self.grad_clip_norm > 0.0:                     # the norm's partials and its {norm, scale}: addresses a captured step keeps
            if getattr(self, "_gn_ws", None) is None or self._gn_ws.numel() < self._n_chunks:
                self._gn_ws = torch.empty(self._n_chunks, dtype=torch.float64, device=dev)
            if self.last_grad_norm is None:
                self.last_grad_norm = torch.zeros(2, dtype=torch.float32, device=dev)
        self._key = key

    def _grad_pointers(self, grads, dev):
        """Table of gradient base pointers.  With the gradients in a GradBucket the addresses never change and the table
        is uploaded once; otherwise autograd re-allocates most of them every step: pinned host buffers, two in rotation,
        copied asynchronously -- a pageable copy would stall the host on the whole backward."""
        n = len(grads)
        key = tuple(g.data_ptr() for g in grads)
        if getattr(self, "_gp_key", None) == key:
            return self._gp_dev
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamWStep: gradient addresses changed inside a graph capture (run warm-up steps first)")
        if getattr(self, "_gp_host", None) is None or self._gp_host[0].numel() != n:
            self._gp_host = [torch.empty(n, dtype=torch.int64).pin_memory() for _ in range(2)]
            self._gp_ev = [None, None]
            self._gp_dev = torch.empty(n, dtype=torch.int64, device=dev)
            self._gp_i = 0
        i = self._gp_i
        self._gp_i ^= 1
        if self._gp_ev[i] is not None:
            self._gp_ev[i].synchronize()                  # the copy that last read this host buffer has run
        self._gp_host[i].copy_(torch.tensor(key, dtype=torch.int64))
        self._gp_dev.copy_(self._gp_host[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._gp_ev[i] = ev
        self._gp_key = key
        return self._gp_dev

    def _device_scalars(self, group, shared, dev):
        """{step, lr} on the device for the graph-capturable launch; the host copies stay authoritative for checkpoints."""
        sc = self._dev_scalars.get(id(group))
        if sc is None:
            sc = torch.tensor([float(shared), float(group["lr"])], dtype=torch.float32, device=dev)
            self._dev_scalars[id(group)] = sc
            self._dev_lr[id(group)] = float(group["lr"])
        elif self._dev_lr[id(group)] != float(group["lr"]) and not torch.cuda.is_current_stream_capturing():
            sc[1].fill_(float(group["lr"]))               # the LR scheduler edited the group
            self._dev_lr[id(group)] = float(group["lr"])
        return sc

    def _refresh_device_step(self, group, shared):
        """The device-side {step, lr} tensor is never dropped once it exists: a hipGraph captured by MLD.capture_training_step has
        its ADDRESS baked in, and a freed tensor's memory may be handed to someone else while replays still add to it.  After a
        host-side step (or load_state_dict) the count is rewritten in place instead."""
        sc = self._dev_scalars.get(id(group))
        if sc is not None and not torch.cuda.is_current_stream_capturing():
            sc[0].fill_(float(shared))

    def sync_lr(self):
        """Push a learning rate the LR scheduler edited to the device-side scalars (before replaying a captured step)."""
        for group in self.opt.param_groups:
            k = id(group)
            if k in self._dev_scalars and self._dev_lr[k] != float(group["lr"]):
                self._dev_scalars[k][1].fill_(float(group["lr"]))
                self._dev_lr[k] = float(group["lr"])

    def note_replay(self):
        """A captured step was replayed: advance the host-side step counts (the device-side count advanced in the graph)."""
        for group in self.opt.param_groups:
            shared = self._shared.get(id(group))
            if shared is not None:
                shared.add_(1.0)
        torch.autograd.graph.increment_version(self._updated)

    def _step_ex(self, group, shared, gp, device_step, capturing):
        """seeme_grad_norm (after the caller's all-reduce: every rank forms the same scale) and seeme_adamw_step_ex."""
        a = L.AdamWEx()
        a.chunks, a.n_chunks = self._chunks.data_ptr(), self._n_chunks
        a.params, a.grads, a.exp_avg, a.exp_avg_sq = self._p.data_ptr(), gp.data_ptr(), self._m.data_ptr(), self._v.data_ptr()
        a.ema = L.ptr(self._e)
        a.beta1, a.beta2 = (float(b) for b in group["betas"])
        a.eps, a.weight_decay = float(group["eps"]), float(group["weight_decay"])
        a.ema_decay, a.ema_warmup = self.ema_decay, int(self.ema_warmup)
        if self.grad_clip_norm > 0.0:
            out, ws = self.last_grad_norm, self._gn_ws
            L.call("seeme_grad_norm", a.chunks, a.n_chunks, a.grads, self.grad_clip_norm, out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                   L.current_stream())
            a.grad_scale = out.data_ptr() + 4
        if device_step:
            sc = self._device_scalars(group, shared, self._chunks.device)
            sc[0:1].add_(1.0)
            if not capturing:
                shared.add_(1.0)
            a.step_lr = sc.data_ptr()
        else:
            step = float(shared) + 1.0
            shared.fill_(step)
            self._refresh_device_step(group, shared)
            a.lr, a.step = float(group["lr"]), step
        L.call("seeme_adamw_step_ex", C.byref(a), L.current_stream())

    @torch.no_grad()
    def step(self, device_step: bool = False):
        """device_step: step count and learning rate are read from device memory (seeme_adamw_step_dev), which makes the
        launch capturable in a hipGraph; inside a capture the host-side step count is left to note_replay().

        The kernels write the parameters through raw pointers, so the version counter of every updated parameter is bumped here
        (and in note_replay): the sampling-side weight images are cached on (data_ptr, _version) and must rebuild."""
        capturing = torch.cuda.is_current_stream_capturing()
        extras = self.ema_decay > 0.0 or self.grad_clip_norm > 0.0 or self._force_ex
        if not capturing:
            self._ensure_shadows()
        updated = []
        for group in self.opt.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            for p in params:
                L.require_cuda(p, "AdamW parameter")
                if p.dtype != torch.float32 or not p.is_contiguous() or p.grad.dtype != torch.float32:
                    raise NotImplementedError("FusedAdamWStep: contiguous fp32 parameters and gradients")
                st = self.opt.state[p]
                if len(st) == 0:                          # same lazy state as torch.optim.AdamW._init_group
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            # one shared step tensor per group: 204 scalar increments per step cost more host time than the kernel
            # (a tensor of this object's own: state handed over by load_state_dict may alias another optimiser's)
            shared = self._shared.get(id(group))
            if shared is None or any(self.opt.state[p]["step"] is not shared for p in params):
                steps = {float(self.opt.state[p]["step"]) for p in params}
                if len(steps) != 1:
                    raise NotImplementedError("FusedAdamWStep: parameters of a group must share their step count")
                shared = torch.tensor(steps.pop(), dtype=torch.float32)
                self._shared[id(group)] = shared
                for p in params:
                    self.opt.state[p]["step"] = shared
                self._refresh_device_step(group, shared)
            self._tables(params)
            grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in params]
            gp = self._grad_pointers(grads, params[0].device)
            b1, b2 = group["betas"]
            updated += params
            if extras:
                self._step_ex(group, shared, gp, device_step, capturing)
            elif device_step:
                sc = self._device_scalars(group, shared, params[0].device)
                sc[0:1].add_(1.0)
                if not capturing:
                    shared.add_(1.0)
                L.call("seeme_adamw_step_dev", self._chunks.data_ptr(), self._n_chunks, self._p.data_ptr(), gp.data_ptr(),
                       self._m.data_ptr(), self._v.data_ptr(), sc.data_ptr(), float(b1), float(b2), float(group["eps"]),
                       float(group["weight_decay"]), L.current_stream())
            else:
                step = float(shared) + 1.0
                shared.fill_(step)
                self._refresh_device_step(group, shared)  # the device-side count (if any) follows the host's
                L.call("seeme_adamw_step", self._chunks.data_ptr(), self._n_chunks, self._p.data_ptr(), gp.data_ptr(),
                       self._m.data_ptr(), self._v.data_ptr(), float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                       float(group["weight_decay"]), float(step), L.current_stream())
            self._keep = (grads, gp)                      # alive until the next step (the launch is asynchronous)
        self._updated = updated
        torch.autograd.graph.increment_version(updated)
        self.opt._opt_called = True                       # what the LR scheduler's wrapper of optimizer.step() records
