"""An independent, slow restatement of the patch definition (include/seeme_hip.h, seeme_crop_patches): Python loops over pixels, Python
integers (unbounded, ``>>`` floors, ``round`` of a float is round-half-to-even), plus plain float64 bilinear interpolation and the case
list the CPU and the GPU tests share.  Nothing here imports the package."""
import numpy as np

SIDES = (1, 4, 7, 224)
FRAME_SIZES = ((1, 1), (2, 3), (37, 53))


def coords(cx, cy, b, S):
    """(X [S] over u, Y [S] over v): the 1/32-pixel coordinates of the definition, Python integers."""
    cx, cy, b = float(np.float32(cx)), float(np.float32(cy)), float(np.float32(b))
    m = b / S
    ox, oy = cx - (S / 2) * m, cy - (S / 2) * m
    X = [(round(ox * 1024) + 16 + round(m * u * 1024)) >> 5 for u in range(S)]
    Y = [(round((m * v + oy) * 1024) + 16) >> 5 for v in range(S)]
    return X, Y


def patch_loops(frame, cx, cy, b, S):
    """frame uint8 [H,W,3] -> uint8 [S,S,3], pixel by pixel."""
    H, W = frame.shape[:2]
    I = frame.tolist()
    X, Y = coords(cx, cy, b, S)
    out = np.zeros((S, S, 3), np.uint8)
    for v in range(S):
        sy, ay = Y[v] >> 5, Y[v] & 31
        for u in range(S):
            sx, ax = X[u] >> 5, X[u] & 31
            acc = [512, 512, 512]
            for r, c, w in ((sy, sx, (32 - ay) * (32 - ax)), (sy, sx + 1, (32 - ay) * ax), (sy + 1, sx, ay * (32 - ax)),
                            (sy + 1, sx + 1, ay * ax)):
                if 0 <= r < H and 0 <= c < W:                         # a tap outside contributes 0
                    for ch in range(3):
                        acc[ch] += w * I[r][c][ch]
            out[v, u] = [a >> 10 for a in acc]
    return out


def patches_loops(frames, frame_of_patch, boxes, S):
    return np.stack([patch_loops(frames[int(f)], bx[0], bx[1], bx[2], S) for f, bx in zip(frame_of_patch, boxes)])


def bilinear_exact(frame, cx, cy, b, S):
    """Plain float64 bilinear interpolation of the zero-padded frame at (m u + ox, m v + oy) -> float64 [S,S,3]."""
    H, W = frame.shape[:2]
    cx, cy, b = float(np.float32(cx)), float(np.float32(cy)), float(np.float32(b))
    m = b / S
    t = np.arange(S, dtype=np.float64)
    x, y = m * t + (cx - (S / 2) * m), m * t + (cy - (S / 2) * m)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[None, :, None], (y - y0)[:, None, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(r, c):
        ok = ((r >= 0) & (r < H))[:, None] & ((c >= 0) & (c < W))[None, :]
        return np.where(ok[..., None], frame[np.clip(r, 0, H - 1)[:, None], np.clip(c, 0, W - 1)[None, :]].astype(np.float64), 0.0)

    return ((1 - fy) * ((1 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)) + fy * ((1 - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1)))


def neighbour_step(frame):
    """G: the largest difference between horizontal or vertical neighbours of the zero-padded frame."""
    p = np.pad(frame.astype(np.int64), ((1, 1), (1, 1), (0, 0)))
    return int(max(np.abs(np.diff(p, axis=0)).max(), np.abs(np.diff(p, axis=1)).max()))


def _boxes_for(H, W):
    """(name, cx, cy, b) for an H x W frame: inside, over each side, one tap in / one out at both ends of a row, outside, larger than
    the frame, smaller than a pixel."""
    b = 0.6 * min(H, W) + 0.25
    return [("inside", W / 2 + 0.3, H / 2 - 0.2, b),
            ("over_left", 0.5, H / 2, b + 3), ("over_right", W - 0.75, H / 2, b + 3),
            ("over_top", W / 2, 0.25, b + 3), ("over_bottom", W / 2, H - 0.5, b + 3),
            ("sx_minus_one", 3.5, H / 2, 8.0),                        # ox = -0.5: the first column of the patch has sx = -1
            ("sx_last", W + 3.5, H / 2, 8.0),                         # ox = W - 0.5: the first column has sx = W - 1
            ("outside", -100.0, -80.0, b + 3),
            ("larger", W / 2, H / 2, 4.0 * max(H, W) + 1.5),
            ("subpixel", W / 2 + 0.1, H / 2 + 0.1, 0.4)]


def cases():
    """[(id, frames uint8 [nf,H,W,3], frame_of_patch int64 [n], boxes float32 [n,3], S)]: the smallest shapes at which the cutter can
    still go wrong.  Seeded; the frames are noise (every neighbour differs) with a bright last frame."""
    out = []
    for H, W in FRAME_SIZES:
        rng = np.random.default_rng(100 * H + W)
        frames = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        frames[2] |= 0xC0
        named = _boxes_for(H, W)
        boxes = np.array([bx[1:] for bx in named], np.float32)
        fop = np.array([(len(named) - 1 - i) % 3 for i in range(len(named))], np.int64)            # repeated, mostly descending
        for S in SIDES:
            if S == 224 and (H, W) != (37, 53):                       # the model's side once: the loops are slow
                continue
            keep = slice(None) if S != 224 else [0, 1, 3, 5, 9]
            out.append((f"{H}x{W}_S{S}", frames, fop[keep], boxes[keep], S))
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    # b = 112.109375 at S = 224: m 1024 = 512.5, the round-half-even tie of rne(m u 1024) at u = 1 (and every odd u)
    out.append(("rne_tie_S224", frames, np.array([1], np.int64), np.array([[30.0, 20.0, 112.109375]], np.float32), 224))
    # two columns 0 | 1, X = 16 (sx = 0, ax = 16), ay = 0: (32 * 16 * 1 + 512) >> 10 = 1, the rounding half of the final shift
    two = np.zeros((1, 1, 2, 3), np.uint8)
    two[0, 0, 1] = 1
    out.append(("half_of_the_final_shift", two, np.array([0], np.int64), np.array([[1.0, 0.5, 1.0]], np.float32), 1))
    # n = 1, 3, 65 with repeated and descending frame indices
    for n in (1, 3, 65):
        out.append((f"n{n}_S7",) + _many(rng, frames, n) + (7,))
    return out


def _many(rng, frames, n):
    fop = np.array([(n - 1 - i) % 3 for i in range(n)], np.int64)
    boxes = np.stack([rng.uniform(-5, 58, n), rng.uniform(-5, 42, n), rng.uniform(0.5, 70, n)], axis=1).astype(np.float32)
    return frames, fop, boxes


def many_patch_cases():
    """More patches than a launch has grid rows, so that a workgroup walks several (too slow for the loops: the twin is the
    reference): 65 patches of 224 (41 rows), 3000 of 1 (2048 rows)."""
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    return [("n65_S224",) + _many(rng, frames, 65) + (224,), ("n3000_S1",) + _many(rng, frames, 3000) + (1,)]
