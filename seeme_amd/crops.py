"""The 224 x 224 patch around the interactee, cut from raw video frames: the step before the ResNet-50 backbone.

``patch_box``            the stored ``recording_utils.center`` / ``.scale`` of a frame -> the box (cx, cy, b) the reference warps.
``crop_patches_hip``     ``seeme_crop_patches`` (csrc/crop_patches.hip): all patches of a call in ONE launch.
``crop_patches_torch``   its plain-torch twin: integer torch ops, any device.  The patch is an integer definition (include/seeme_hip.h,
                         DESIGN 5.4b), so the two agree bit for bit and no test needs a tolerance.
``write_crop_files``     ``image_crops_<split>.npy`` / ``image_crop_names_<split>.npy`` for the data module's crop route
                          from a frame reader; scripts/make_image_crops.py wraps it.

Decoding a video or a JPEG stays outside the package: frames come in as uint8 RGB arrays.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, List, Tuple

import numpy as np
import torch

from . import _lib as L

PATCH = 224                  # the model's patch side (dataset.py:1668)
FRAME_MAX = 16384            # SEEME_CROP_FRAME_MAX
PATCH_MAX = 1024             # SEEME_CROP_PATCH_MAX
COORD_MAX = 1 << 20          # SEEME_CROP_COORD_MAX


def patch_box(center, scale) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """center [...,2], scale [...] -> (cx, cy, b), float32 [...]: b = float32(scale * 200), cx = float32(center[...,0] + b),
    cy = float32(center[...,1] + b).

    This restates the reference as it is, dataset.py:1670-1672 included: it ADDS the box size to the stored centre before it
    warps (``center_x = center[0] + bbox_size``), so the patch is not centred on ``center``.  Its checkpoints were trained on
    exactly these patches, so the conditioning image has to be cut the same way; this function is the one place that says so."""
    c, s = np.asarray(center, np.float32), np.asarray(scale, np.float32)
    if c.shape[-1:] != (2,) or c.shape[:-1] != s.shape:
        raise ValueError(f"patch_box: center is {c.shape}, scale is {s.shape}: expected [...,2] and [...]")
    b = s * np.float32(200.0)
    return c[..., 0] + b, c[..., 1] + b, b


def boxes_of(center, scale) -> np.ndarray:
    """``patch_box`` as the [n,3] float32 table (cx, cy, b) the cutters take."""
    return np.stack(patch_box(center, scale), axis=-1).reshape(-1, 3).astype(np.float32)


def _check(who: str, frames, frame_of_patch, boxes, S):
    """The preconditions of the definition, checked on the host before any launch -> (frame_of_patch int64 [n], boxes float32 [n,3], S)."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        what = f"{tuple(frames.shape)} {frames.dtype}" if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"{who}: frames are {what}: expected a uint8 tensor [n_frames,H,W,3]")
    nf, H, W = (int(v) for v in frames.shape[:3])
    if nf < 1:
        raise ValueError(f"{who}: n_frames is {nf}: at least one frame is needed")
    if not (1 <= H <= FRAME_MAX and 1 <= W <= FRAME_MAX):
        raise ValueError(f"{who}: frames are {H} x {W}: H and W must be in 1..{FRAME_MAX}")
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= int(S) <= PATCH_MAX:
        raise ValueError(f"{who}: S is {S!r}: the patch side must be an integer in 1..{PATCH_MAX}")
    as_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    fop, bx = as_np(frame_of_patch), as_np(boxes)
    if fop.ndim != 1 or fop.shape[0] < 1 or fop.dtype.kind not in "iu":
        raise ValueError(f"{who}: frame_of_patch is {fop.shape} {fop.dtype}: expected integers [n], n >= 1")
    fop = fop.astype(np.int64)
    n = fop.shape[0]
    if bx.shape != (n, 3) or bx.dtype.kind != "f":
        raise ValueError(f"{who}: boxes are {bx.shape} {bx.dtype}: expected floats [{n},3] = cx, cy, b (n = {n})")
    bx = np.ascontiguousarray(bx, np.float32)
    bad = np.flatnonzero((fop < 0) | (fop >= nf))
    if bad.size:
        raise ValueError(f"{who}: frame_of_patch[{int(bad[0])}] is {int(fop[bad[0]])}: outside 0..{nf - 1}")
    with np.errstate(invalid="ignore"):
        bad_c = ~(np.abs(bx[:, :2]) <= COORD_MAX).all(axis=1)           # (NaN and inf fail the comparison)
        bad_b = ~((bx[:, 2] > 0) & (bx[:, 2] <= COORD_MAX))
    if bad_c.any():
        i = int(np.argmax(bad_c))
        raise ValueError(f"{who}: box {i} has its centre at ({bx[i, 0]}, {bx[i, 1]}): cx and cy must be finite with |cx|, |cy| <= 2^20")
    if bad_b.any():
        i = int(np.argmax(bad_b))
        raise ValueError(f"{who}: box {i} has the side b = {bx[i, 2]}: b must be finite with 0 < b <= 2^20")
    return fop, bx, int(S)


# ----------------------------------------------------------------------------- the twin
def crop_patches_torch(frames, frame_of_patch, boxes, S: int = PATCH) -> torch.Tensor:
    """frames uint8 [n_frames,H,W,3] (any device), frame_of_patch [n] integers, boxes [n,3] = cx, cy, b -> uint8 [n,S,S,3] on the
    frames' device: the definition of ``seeme_crop_patches`` (include/seeme_hip.h) in integer torch ops.  The coordinates are
    float64 with every product and sum rounded on its own, ``torch.round`` is round-half-to-even, ``>>`` on int64 floors."""
    fop, bx, S = _check("crop_patches_torch", frames, frame_of_patch, boxes, S)
    dev = frames.device
    H, W = int(frames.shape[1]), int(frames.shape[2])
    n = fop.shape[0]
    f = torch.from_numpy(fop).to(dev)
    cx, cy, b = torch.from_numpy(bx).to(dev).double().unbind(1)
    m = b / S
    hs = (0.5 * S) * m
    ox, oy = cx - hs, cy - hs
    t = torch.arange(S, device=dev, dtype=torch.float64)
    X = (torch.round(ox * 1024.0).long()[:, None] + 16 + torch.round(m[:, None] * t * 1024.0).long()) >> 5        # [n,S] over u
    Y = (torch.round((m[:, None] * t + oy[:, None]) * 1024.0).long() + 16) >> 5                                  # [n,S] over v
    sx, ax, sy, ay = X >> 5, X & 31, Y >> 5, Y & 31
    flat = frames.reshape(-1, 3)
    out = torch.empty(n, S, S, 3, dtype=torch.uint8, device=dev)
    step = max(1, (1 << 21) // (S * S))                                        # patches per pass: the temporaries are [step,S,S,3]
    for lo in range(0, n, step):
        sl = slice(lo, lo + step)
        acc = torch.full((f[sl].shape[0], S, S, 3), 512, dtype=torch.int32, device=dev)
        for dy, wy in ((0, 32 - ay[sl]), (1, ay[sl])):
            for dx, wx in ((0, 32 - ax[sl]), (1, ax[sl])):
                r, c = (sy[sl] + dy)[:, :, None], (sx[sl] + dx)[:, None, :]
                inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)                # a tap outside contributes 0
                at = (f[sl, None, None] * H + r.clamp(0, H - 1)) * W + c.clamp(0, W - 1)
                w = (wy[:, :, None] * wx[:, None, :] * inside).to(torch.int32)
                acc += w[..., None] * flat[at].to(torch.int32)
        out[sl] = (acc >> 10).to(torch.uint8)
    return out


# ----------------------------------------------------------------------------- the kernel
def crop_patches_hip(frames, frame_of_patch, boxes, S: int = PATCH) -> torch.Tensor:
    """frames uint8 [n_frames,H,W,3] on the ROCm device, frame_of_patch [n] integers and boxes [n,3] = cx, cy, b (host arrays; a
    device tensor is copied back: the preconditions are checked on the host, before any launch) -> uint8 [n,S,S,3] on the device,
    ONE launch of ``seeme_crop_patches`` on the current stream."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise L.SeemeError("crop_patches: frames must be a tensor on the ROCm device (cuda:N); crop_patches_torch is the twin for any device")
    fop, bx, S = _check("crop_patches_hip", frames, frame_of_patch, boxes, S)
    dev = frames.device
    out = torch.empty(fop.shape[0], S, S, 3, dtype=torch.uint8, device=dev)
    _launch(frames.contiguous(), torch.from_numpy(fop.astype(np.int32)).to(dev), torch.from_numpy(bx).to(dev), S, out)
    return out


def _launch(frames, fop_dev, boxes_dev, S: int, out) -> None:
    """The C entry as it is (no host checks: the tests hand it boxes outside the preconditions)."""
    with torch.cuda.device(frames.device):
        L.call("seeme_crop_patches", frames.data_ptr(), int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2]),
               fop_dev.data_ptr(), boxes_dev.data_ptr(), int(fop_dev.shape[0]), int(S), out.data_ptr(), L.current_stream())


def crop_patches(frames, frame_of_patch, boxes, S: int = PATCH, device=None) -> torch.Tensor:
    """The kernel when `device` is a ROCm device (the frames are moved there), the twin otherwise (on the frames' own device)."""
    if device is not None and torch.device(device).type == "cuda":
        return crop_patches_hip(frames.to(device), frame_of_patch, boxes, S)
    return crop_patches_torch(frames, frame_of_patch, boxes, S)


# ----------------------------------------------------------------------------- crop files for training
def write_crop_files(entries: Iterable, read_frame: Callable[[str], np.ndarray], out_dir: str, split: str, device=None,
                     batch: int = 64) -> Dict:
    """``<out_dir>/image_crops_<split>.npy`` (uint8 [F,224,224,3] RGB) and ``<out_dir>/image_crop_names_<split>.npy`` (unicode [F]), as
    INTEGRATION.md F specifies them: what ``EgoDataModule`` reads with ``image_backbone``.

    entries: an iterable of (image name, center [2], scale), e.g. a split's ``recording_utils`` rows; names are de-duplicated (a
    name that comes again with another box is an error) and sorted.  read_frame(name) -> uint8 RGB [H,W,3].  Consecutive frames of
    equal size are cut `batch` at a time, one launch per batch on a ROCm `device`, the twin without one.  The crops file is
    written through a memory map, so only one batch of frames is held at a time."""
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"write_crop_files: batch is {batch!r}: expected an integer >= 1")
    box: Dict[str, np.ndarray] = {}
    for name, center, scale in entries:
        name, bx = str(name), boxes_of(np.asarray(center, np.float32).reshape(2), np.asarray(scale, np.float32).reshape(()))[0]
        if name in box and not np.array_equal(box[name], bx):
            raise ValueError(f"write_crop_files: '{name}' comes with two boxes, {box[name].tolist()} and {bx.tolist()}")
        box[name] = bx
    names = sorted(box)
    if not names:
        raise ValueError("write_crop_files: no entry")
    os.makedirs(out_dir, exist_ok=True)
    crops_path = os.path.join(out_dir, f"image_crops_{split}.npy")
    names_path = os.path.join(out_dir, f"image_crop_names_{split}.npy")
    crops = np.lib.format.open_memmap(crops_path, "w+", np.uint8, (len(names), PATCH, PATCH, 3))
    launches = 0
    held: List[np.ndarray] = []

    def flush(first: int):
        nonlocal launches
        if held:
            k = len(held)
            cut = crop_patches(torch.from_numpy(np.stack(held)), np.arange(k), np.stack([box[n] for n in names[first:first + k]]),
                               PATCH, device)
            crops[first:first + k] = cut.cpu().numpy()
            launches += 1
            held.clear()

    first = 0
    for i, name in enumerate(names):
        fr = np.asarray(read_frame(name))
        if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
            raise ValueError(f"write_crop_files: read_frame('{name}') gave {fr.shape} {fr.dtype}: expected uint8 RGB [H,W,3]")
        if held and (fr.shape != held[0].shape or len(held) == batch):
            flush(first)
        if not held:
            first = i
        held.append(fr)
    flush(first)
    crops.flush()
    del crops
    np.save(names_path, np.array(names))
    return {"crops": crops_path, "names": names_path, "count": len(names), "launches": launches}
