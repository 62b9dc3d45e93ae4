"""seeme_render + seeme_render_shade under HIP events: 600 frames of 640 x 480 with two SMPL-size bodies (uv_sphere(84, 82) stretched to
a person's proportions: 6890 vertices, 13 776 faces each) and 20 000 scene points, one orbit camera, in chunks of --chunk frames.
After warm-up, the median of --repeats passes over all frames; the twin's CPU time on the first --twin_frames frames of the same
inputs, which also checks the kernels' ids, inv_depth and dropped bit for bit there.  Information, not a target.
    python scripts/render_bench.py [--out profiles/render.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seeme_amd import _lib as L  # noqa: E402
from seeme_amd import render as RD  # noqa: E402


def scene(frames, n_points, seed=0):
    g = np.random.default_rng(seed)
    v, f = RD.uv_sphere(84, 82)
    body = v * (0.22, 0.15, 0.85)                                            # a 1.7 m ellipsoid, z up
    t = np.linspace(0.0, 1.0, frames)[:, None, None]
    a = body[None] + np.concatenate([0.8 * np.cos(2 * np.pi * t), 0.8 * np.sin(2 * np.pi * t), 0.85 + 0 * t], axis=2)
    b = body[None] + np.concatenate([0.3 * t, -0.2 + 0 * t, 0.85 + 0.1 * np.sin(6 * np.pi * t)], axis=2)
    verts = np.concatenate([a, b], axis=1).astype(np.float32)
    faces = np.concatenate([f, f + v.shape[0]]).astype(np.int32)
    room = g.random((n_points, 3)) * (6.0, 6.0, 2.5) - (3.0, 3.0, 0.0)
    room[: n_points // 2, 2] = 0.0                                          # half of the cloud is the floor
    return verts, faces, room.astype(np.float32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--frames", type=int, default=600)
    p.add_argument("--size", default="480x640")
    p.add_argument("--points", type=int, default=20000)
    p.add_argument("--point_size", type=int, default=2)
    p.add_argument("--chunk", type=int, default=100)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--twin_frames", type=int, default=2)
    args = p.parse_args()
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    dev = torch.device("cuda:0")
    H, W = (int(v) for v in args.size.split("x"))
    F, step = args.frames, min(args.chunk, args.frames)
    verts_h, faces_h, points_h = scene(F, args.points)
    cam = RD.orbit_camera(verts_h[::50], 30, 20, 60, (0, 0, 1), aspect=W / H)[None].astype(np.float32)
    K = RD.intrinsics(60, (H, W))
    verts, faces, points, cams = (torch.from_numpy(a).to(dev) for a in (verts_h, faces_h, points_h, cam))
    NV, NF, P = verts.shape[1], faces.shape[0], points.shape[0]
    k = tuple(float(np.float32(v)) for v in K) + (float(np.float32(0.05)),)
    mof = torch.cat([torch.zeros(NF // 2), torch.ones(NF // 2)]).to(torch.int32).to(dev)
    pal = torch.tensor([[96, 152, 232], [236, 146, 84]], dtype=torch.uint8, device=dev)
    prgb = torch.from_numpy(RD.height_colours(points_h, (0, 0, 1))).to(dev)
    ids, inv = (torch.empty(step, H, W, dtype=torch.int32, device=dev) for _ in range(2))
    dropped = torch.empty(step, dtype=torch.int32, device=dev)
    rgb = torch.empty(step, H, W, 3, dtype=torch.uint8, device=dev)
    ws_bytes = int(L.lib().seeme_render_workspace_bytes(step, NV, H, W))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = L.current_stream()

    def chunk_scene(lo):
        n = min(step, F - lo)
        return n, RD._scene_struct(verts[lo:lo + n], faces, points, cams, n, NV, NF, P, 1, H, W, k, args.point_size)

    def render(lo):
        n, sc = chunk_scene(lo)
        L.call("seeme_render", C.byref(sc), ids.data_ptr(), inv.data_ptr(), dropped.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    def shade(lo):
        n, sc = chunk_scene(lo)
        L.call("seeme_render_shade", C.byref(sc), ids.data_ptr(), mof.data_ptr(), pal.data_ptr(), 2, prgb.data_ptr(),
               24 | 24 << 8 | 28 << 16, rgb.data_ptr(), stream)

    def one_pass():
        """All frames once -> (ms in seeme_render, ms in seeme_render_shade), an event pair around every call."""
        ev = []
        for lo in range(0, F, step):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            render(lo)
            e[1].record()
            shade(lo)
            e[2].record()
            ev.append(e)
        torch.cuda.synchronize()
        return sum(e[0].elapsed_time(e[1]) for e in ev), sum(e[1].elapsed_time(e[2]) for e in ev)

    one_pass()                                                              # warm-up: code objects, every chunk shape
    passes = [one_pass() for _ in range(args.repeats)]
    stat = lambda xs: {"min_ms": min(xs), "median_ms": float(np.median(xs)), "max_ms": max(xs), "n": len(xs)}
    r_ms, s_ms = stat([a for a, _ in passes]), stat([b for _, b in passes])
    both = stat([a + b for a, b in passes])
    # the kernels against the twin on the first frames, and what the twin costs on the CPU
    nt = min(args.twin_frames, step)
    render(0)
    shade(0)
    torch.cuda.synchronize()
    got = {"ids": ids[:nt].cpu(), "inv_depth": inv[:nt].cpu(), "dropped": dropped[:nt].cpu()}
    got_rgb = rgb[:nt].cpu()
    covered = float((ids >= 0).float().mean())
    body_px = float(((ids >= 0) & (ids < NF)).float().mean())
    t0 = time.perf_counter()
    want = RD.render_torch(torch.from_numpy(verts_h[:nt]), torch.from_numpy(faces_h), torch.from_numpy(cam), K, (H, W),
                           points=torch.from_numpy(points_h), near=0.05, point_size=args.point_size)
    t1 = time.perf_counter()
    want_rgb = RD.shade_torch(torch.from_numpy(verts_h[:nt]), torch.from_numpy(faces_h), torch.from_numpy(cam), want["ids"], mof.cpu(),
                              pal.cpu(), torch.from_numpy(points_h), prgb.cpu(), bg=(24, 24, 28))
    t2 = time.perf_counter()
    assert all(torch.equal(got[key], want[key]) for key in want), "kernel and twin disagree"
    assert int((got_rgb.int() - want_rgb.int()).abs().max()) <= 1, "shading differs from the twin by more than one level"
    res = {"device": torch.cuda.get_device_name(0), "what": "information, not a target",
           "plan": "project, per-face box walk with 64-bit global atomic max (wave-shared above 256 box pixels), points, resolve; shade",
           "shape": {"frames": F, "H": H, "W": W, "bodies": 2, "vertices": NV, "faces": NF, "points": P, "point_size": args.point_size,
                     "frames_per_call": step, "pixels_covered": covered, "pixels_covered_by_a_body": body_px},
           "launches_per_call": {"seeme_render": "2 memsets + k_render_project, k_render_faces, k_render_points, k_render_resolve",
                                 "seeme_render_shade": "k_render_shade"},
           "calls_per_pass": -(-F // step),
           "workspace_bytes_per_call": ws_bytes,
           "seeme_render_all_frames": r_ms, "seeme_render_shade_all_frames": s_ms, "both_all_frames": both,
           "per_frame_ms": {"seeme_render": r_ms["median_ms"] / F, "seeme_render_shade": s_ms["median_ms"] / F, "both": both["median_ms"] / F},
           "bytes_written_per_frame": H * W * 11,
           "twin_cpu": {"frames": nt, "render_torch_s_per_frame": (t1 - t0) / nt, "shade_torch_s_per_frame": (t2 - t1) / nt,
                        "threads": torch.get_num_threads(), "equal_to_the_kernels": True}}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
