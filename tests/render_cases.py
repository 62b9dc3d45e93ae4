"""Hand-made scenes for the rasteriser's tests, shared by tests/test_render_cpu.py and tests/test_gpu_render.py.

Every scene is seen through the identity camera with fx = fy = 1, cx = cy = 0 and near = 0.5, so a corner given as (x, y, z) in
PIXELS and metres is the world point (x z, y z, z) and snaps to X = 16 x, Y = 16 y exactly when x, y are multiples of 1/16 and z is
a power of two: the tests place corners and edges on pixel centres on purpose.  Q = 2^21 / z."""
import numpy as np

K = (1.0, 1.0, 0.0, 0.0)
NEAR = 0.5
CAM = np.eye(4, dtype=np.float32)[None]
SIZE = (37, 29)                 # H x W: odd, no multiple of anything
PX_MAX = 16384.0                # SEEME_RENDER_COORD_MAX / 16


def P(x, y, z=1.0):
    return (x * z, y * z, z)


def tris(*corners):
    """Corners in threes, each (x, y) or (x, y, z) in pixels / metres -> float32 [n,3,3] world."""
    a = np.array([P(*c) for c in corners], np.float32)
    assert a.shape[0] % 3 == 0
    return a.reshape(-1, 3, 3)


def scene(t, points=None, size=SIZE, point_size=1):
    """Triangles [n,3,3] with their own three vertices each -> the keyword arguments of render_* for ONE frame, as numpy."""
    t = np.asarray(t, np.float32).reshape(-1, 3, 3)
    n = t.shape[0]
    return {"verts": t.reshape(1, 3 * n, 3), "faces": np.arange(3 * n, dtype=np.int64).reshape(n, 3), "cams": CAM, "intrinsics": K,
            "size": size, "points": None if points is None else np.asarray(points, np.float32).reshape(-1, 3), "near": NEAR,
            "point_size": point_size}


TRIANGLE = tris((2, 2), (10, 2), (2, 10))                                   # corners, two axis-parallel edges and the diagonal on centres
QUAD = tris((3, 3), (11, 3), (11, 11), (3, 3), (11, 11), (3, 11))           # the shared diagonal passes through (4,4) .. (10,10)
_RIM = [(12, 8), (12, 12), (8, 12), (4, 12), (4, 8), (4, 4), (8, 4), (12, 4)]
FAN = tris(*[c for k in range(8) for c in ((8, 8), _RIM[k], _RIM[(k + 1) % 8])])
NOTHING = tris((1, 1), (5, 5), (9, 9),                                      # collinear
               (4, 4), (4, 4), (4, 4),                                      # one point
               (1, 1), (5, 5), (3, 3.01),                                   # collinear after snapping: 3.01 * 16 = 48.16 -> 48
               (2, 7), (9, 7), (5, 7))                                      # collinear on a pixel row
BORDERS = tris((-5, 5), (6, 3), (4, 12),                                    # partly off the left
               (25, 5), (40, 9), (26, 14),                                  # ... the right
               (10, -6), (18, 4), (8, 5),                                   # ... the top
               (10, 30), (18, 45), (6, 41),                                 # ... the bottom
               (-8, -9), (60, -3), (-4, 70),                                # over every border at once
               (-20, 3), (-3, 5), (-9, 20),                                 # wholly off the left
               (31, 3), (50, 5), (40, 20),                                  # ... the right
               (3, -20), (9, -2), (20, -11),                                # ... the top
               (3, 38), (9, 60), (20, 41),                                  # ... the bottom
               (-0.5, -0.5, 0.5), (0.5, -0.25, 0.5), (-0.25, 0.75, 0.5))    # around pixel (0, 0) alone, in front of the others
# the middle three faces each have ONE bad corner: behind near, beyond COORD_MAX, NaN; their neighbours must not notice
_BAD = tris((2, 2), (9, 3), (3, 9),
            (12, 2), (20, 3), (14, 9),
            (12, 12), (20, 13), (14, 19),
            (2, 22), (9, 23), (3, 29),
            (15, 25), (25, 26), (17, 33)).copy()
_BAD[1, 1] = (5.0, 1.0, 0.25)
_BAD[2, 2] = P(PX_MAX + 1.0, 3.0)
_BAD[3, 0, 1] = np.nan
BAD_CORNERS = _BAD
TWINS = tris((2, 2), (20, 5), (6, 25), (2, 2), (20, 5), (6, 25))           # two identical triangles
CROSSING = tris((2, 4, 1.0), (26, 4, 4.0), (14, 30, 2.0),                   # depth rises to the right / falls to the right
                (2, 6, 4.0), (26, 6, 1.0), (14, 32, 2.0))
EXTREME = tris((-PX_MAX, -PX_MAX, NEAR), (PX_MAX, -PX_MAX, NEAR), (PX_MAX, PX_MAX, NEAR),       # corners at +-COORD_MAX, Q = 2^22:
               (-PX_MAX, -PX_MAX, NEAR), (PX_MAX, PX_MAX, NEAR), (-PX_MAX, PX_MAX, NEAR))      # the largest quad there is
FLOOR = tris((1, 1), (27, 1), (27, 35), (1, 1), (27, 35), (1, 35))         # z = 1 under the points below
POINTS = np.array([P(2.5, 3.5, 0.75),          # X = 40, Y = 56: both 8 (mod 16), round up to pixel (row 4, col 3)
                   P(-0.5, -0.5, 0.75),        # X = Y = -8: pixel (0, 0)
                   P(-0.5625, 5, 0.75),        # X = -9: column -1, off the image
                   P(0, 0, 0.75), P(28, 36, 0.75), P(28, 0, 0.75), P(0, 36, 0.75),      # the four corner pixels
                   P(10, 10, 1.0),             # exactly the floor's depth: the face wins
                   P(12, 10, 0.96875),         # a little nearer: the point wins
                   P(14, 10, 2.0),             # behind the floor
                   P(16, 10, 0.25),            # behind near: invalid
                   (np.nan, 0.0, 1.0)], np.float32)

HAND = {                                                                    # name -> one-frame scene
    "triangle": scene(TRIANGLE), "quad": scene(QUAD), "fan": scene(FAN), "nothing": scene(NOTHING), "borders": scene(BORDERS),
    "triangle_cw": scene(TRIANGLE[:, [0, 2, 1]]), "bad_corners": scene(BAD_CORNERS), "twins": scene(TWINS), "crossing": scene(CROSSING),
    "extreme": scene(EXTREME), "borders_1x1": scene(BORDERS, size=(1, 1)), "borders_1x16": scene(BORDERS, size=(1, 16)),
    "extreme_1x1": scene(EXTREME, size=(1, 1)),
    "points_1": scene(FLOOR, POINTS, point_size=1), "points_2": scene(FLOOR, POINTS, point_size=2),
    "points_3": scene(FLOOR, POINTS, point_size=3), "points_8": scene(FLOOR, POINTS, point_size=8),
    "points_only": scene(np.zeros((0, 3, 3)), POINTS, point_size=4), "points_1x16": scene(FLOOR, POINTS, size=(1, 16), point_size=3),
}


def batches():
    """The hand scenes grouped into multi-frame calls: scenes of one size, point size and point set become the frames of one call,
    the shorter face lists padded with a valid zero-area triangle (it draws nothing and is not dropped)."""
    groups = {}
    for name, s in HAND.items():
        key = (s["size"], s["point_size"], None if s["points"] is None else s["points"].tobytes())
        groups.setdefault(key, []).append(name)
    out = []
    for names in groups.values():
        n = max(HAND[m]["verts"].shape[1] for m in names)
        pad = np.array(P(1, 1), np.float32)
        verts = np.stack([np.concatenate([HAND[m]["verts"][0], np.broadcast_to(pad, (n - HAND[m]["verts"].shape[1], 3))]) for m in names])
        s = dict(HAND[names[0]], verts=verts.astype(np.float32), faces=np.arange(n, dtype=np.int64).reshape(-1, 3))
        out.append((names, s))
    return out


def random_triangles(seed=5, n=64):
    """n random triangles at SIZE: a screen-filling one, slivers, corners off the screen and behind the camera, mixed depths."""
    g = np.random.default_rng(seed)
    H, W = SIZE
    xy = g.uniform((-6, -6), (W + 6, H + 6), (n, 3, 2))
    xy = np.round(xy * 16) / 16                                              # on the snapping grid: the cases above cover the rest
    z = 2.0 ** g.integers(0, 3, (n, 3))
    t = np.concatenate([xy * z[..., None], z[..., None]], axis=-1)
    t[0] = tris((-40, -30, 8.0), (90, -20, 8.0), (10, 120, 8.0))[0]          # fills the screen behind the others (the wave-shared walk)
    t[1:9, 2, :2] = t[1:9, 1, :2] + g.uniform(-0.2, 0.2, (8, 2))             # slivers
    t[9:13, 0, 2] = 0.25                                                     # a corner behind near
    t[13:15, 1, 2] = -1.0                                                    # ... behind the camera
    return t.astype(np.float32)
