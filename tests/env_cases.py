"""The scenes, maps and configurations of tests/test_env_cpu.py and tests/test_gpu_env.py.  TEST INFRASTRUCTURE ONLY.

Scenes, both in front of the fixed camera ((0, 100, 0) looking along +x):
  open     scenes.mirror_hall: floor, one side wall, two mirrors and the blob under an open sky -- most bounce rays leave the scene
  closed   a box around the camera and the blob: no ray ever misses, so the map is never seen and only the environment rays' any-hit
           launch tells the frame from the plain one (every one of them is blocked)
Maps (texel (i, j) at [j, i]; the upper hemisphere is the inner diamond |u| + |v| < 1):
  constant(n, c)   every texel c
  sun(n)           a dim sky with ONE bright texel in the upper hemisphere -- what sample = 1 is for
  hdr(n)           random radiance over six decades, some texels black: weights that quantise to 1 and to 65535
  negzero(n)       hdr(n) with -0.0 components, whole texels of -0.0 among them: not negative, so the map is legal, and a weight of -0.0
                   must not win the maximum
The frames are 37 x 19 and 40 x 24."""
import numpy as np

import adaptive_cases as ac
import path_frame_cases as fc
import scenes

W, H = 40, 24
ODD_W, ODD_H, ODD_ROWS = 37, 19, (3, 17)
SIZES = (4, 16, 256)
SCALE = 1.5
SKY = (0.05, 0.07, 0.1)
SUN = (900.0, 800.0, 600.0)
DN, TP, VP = fc.DN, fc.TP, fc.VP
CHILD_BATCH = fc.CHILD_BATCH
COUNT_VALUES = (0, 1, 3, 4, 9, ac.U32_MAX)
# name -> (scene, map, frame, spp, bounces, shadow, seed, sample, camera); frame "odd" = 37 x 19 rows 3..17, "even" = 40 x 24
FRAMES = {
    "open_s0": ("open", "hdr", "even", 3, 3, 1, 3, 0, "fixed"),
    "open_s1": ("open", "hdr", "even", 3, 3, 1, 3, 1, "fixed"),
    "open_s1_sun_pinhole": ("open", "sun", "even", 4, 3, 0, 5, 1, "pinhole"),
    "open_s0_window": ("open", "sun", "odd", 4, 1, 1, 7, 0, "pinhole"),
    "open_s1_window": ("open", "hdr", "odd", 1, 3, 0, 7, 1, "fixed"),
    "open_s1_flat": ("open", "hdr", "odd", 3, 0, 1, 1, 1, "fixed"),
    "open_s1_one": ("open", "hdr", "even", 1, 1, 1, 2, 1, "pinhole"),
    "closed_s0": ("closed", "hdr", "even", 3, 3, 1, 3, 0, "fixed"),
    "closed_s1": ("closed", "sun", "even", 3, 3, 0, 3, 1, "fixed"),
}
ROULETTE = dict(first=1, q_min=0.3)
EYE, TARGET = (30.0, 140.0, -160.0), (200.0, 60.0, 40.0)


def open_scene(vrt):
    return scenes.mirror_hall(vrt)


def closed_scene(vrt):
    blob = vrt.scene.procedural("blob", 2, 0, 3)
    bt = np.frombuffer(bytes(blob.buffers["tri"]), np.float32).reshape(-1, 3).copy()
    c = bt.mean(0)
    r = np.abs(bt - c).max()
    bt = ((bt - c) * np.float32(40.0 / r) + np.array([180.0, 90.0, 30.0], np.float32)).reshape(-1, 9).astype(np.float32)
    # (bounds that no pixel's primary ray meets in an edge: a vertex on an edge lies in the neighbouring wall's plane and its rays may
    #  start outside; and every wall overlaps its neighbours, so that no ray leaves through an edge)
    x0, x1, y0, y1, z0, z1 = -51.9, 603.7, -0.73, 261.3, -301.37, 297.91
    a0, a1, b0, b1, c0, c1 = x0 - 20, x1 + 20, y0 - 20, y1 + 20, z0 - 20, z1 + 20
    q = scenes._quad
    box = np.array(q((a0, y0, c0), (a1, y0, c0), (a1, y0, c1), (a0, y0, c1)) + q((a0, y1, c0), (a1, y1, c0), (a1, y1, c1), (a0, y1, c1)) +
                   q((a0, b0, z0), (a1, b0, z0), (a1, b1, z0), (a0, b1, z0)) + q((a0, b0, z1), (a1, b0, z1), (a1, b1, z1), (a0, b1, z1)) +
                   q((x0, b0, c0), (x0, b0, c1), (x0, b1, c1), (x0, b1, c0)) + q((x1, b0, c0), (x1, b0, c1), (x1, b1, c1), (x1, b1, c0)), np.float32)
    sc = vrt.scene.from_triangles([box, bt])
    return {k: np.frombuffer(bytes(v), np.uint8).copy() for k, v in sc.buffers.items()}


SCENES = {"open": open_scene, "closed": closed_scene}


def constant(n, c=(0.4, 0.35, 0.25)):
    return np.tile(np.asarray(c, np.float32), (n, n, 1))


def sun(n, at=None):
    """the dim sky with one texel of the upper hemisphere lit: (i, j) = at, by default a texel next to the centre (the pole)"""
    t = np.tile(np.asarray(SKY, np.float32), (n, n, 1))
    i, j = at or (n // 2 + n // 8, n // 2 - n // 8)
    t[j, i] = SUN
    return t


def hdr(n, seed=11):
    rng = np.random.default_rng(seed + n)
    t = (10.0 ** rng.uniform(-3.0, 3.0, (n, n, 1)) * rng.uniform(0.2, 1.0, (n, n, 3))).astype(np.float32)
    t[rng.uniform(size=(n, n)) < 0.1] = 0.0
    t[0, 0] = (0.0, 0.0, 0.0)
    t[n - 1, n - 1] = (2000.0, 0.0, 1.0)
    return t


def negzero(n):
    t = hdr(n)
    nz = np.float32(-0.0)
    t[0, 0] = (nz, nz, nz)
    t[1, 2] = (nz, 0.0, 0.0)
    t[2, 1] = (nz, 5.0, nz)
    t[n - 1, 0] = (0.0, nz, nz)
    assert np.signbit(t).sum() == 8
    return t


def one_texel(n):
    """a single positive texel: every other weight is 0 and quantises to 1"""
    t = np.zeros((n, n, 3), np.float32)
    t[n - 1, 1] = (0.0, 3.0, 0.0)
    return t


MAPS = {"sun": lambda: sun(16), "hdr": lambda: hdr(16)}


def camera(vrt, name, w, h):
    """None (the fixed camera) or the pinhole camera's 14 floats"""
    if name == "fixed":
        return None
    return np.array(vrt.rtapi.look_at(EYE, TARGET, (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32)


def window(frame):
    return (ODD_W, ODD_H, ODD_ROWS) if frame == "odd" else (W, H, (0, H))


def counts_of(w=W, h=H, salt=0):
    return ac.hashed(w, h, COUNT_VALUES, salt)


def lookup_dirs():
    """directions of vxrt_envmap_lookup's test: the axes, +-0 components, the fold (y == 0), the poles, the diagonals, denormal and huge
    lengths, a NaN in each place, infinities and the zero vector, then random ones"""
    z, nz, nan, inf = 0.0, -0.0, np.nan, np.inf
    d = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
         (1, z, nz), (1, nz, z), (nz, 1, z), (z, 1, nz), (nz, -1, nz), (z, -1, z), (nz, nz, 1), (z, nz, -1),
         (1, z, 1), (1, nz, 1), (-1, z, 1), (1, nz, -1), (-1, nz, -1), (0.3, z, -0.7), (0.3, nz, -0.7), (1, 1e-30, 1), (1, -1e-30, 1),
         (1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1), (1, -1, -1), (1e-40, 1e-40, 1e-40), (1e-40, -1e-40, 0), (3e38, 3e38, 3e38),
         (1e20, -1e20, 1e20), (nan, 0, 0), (0, nan, 0), (0, 0, nan), (nan, nan, nan), (1, nan, 1), (inf, 0, 0), (0, -inf, 0), (inf, inf, inf),
         (1, -inf, 1), (z, z, z), (nz, nz, nz), (z, nz, z)]
    rng = np.random.default_rng(5)
    r = rng.normal(size=(2000, 3))
    r[:300, 1] = 0.0                                       # (on the fold)
    r[300:400, 1] = -np.abs(r[300:400, 1]) * 1e-6          # (just under it)
    return np.concatenate([np.array(d, np.float64), r]).astype(np.float32)


def ray_points(n, m, seed=3):
    """(points (k, 6), seeds (k,)) of vxrt_env_rays' test on a map `m` (env_ref.make_map): random vertices whose normals face every way
    -- half of them downwards, away from most of the sky -- and hash outputs among which those that give t = 0 and t = Q - 1, the first
    and the last texel of a row, and 0, 1 and 0xFFFFFFFF"""
    import emissive_ref as er
    rng = np.random.default_rng(seed)
    k = 3000
    pts = np.zeros((k, 6), np.float32)
    pts[:, 0:3] = rng.uniform(-100, 100, (k, 3))
    nr = rng.normal(size=(k, 3))
    nr[: k // 2, 1] = -np.abs(nr[: k // 2, 1]) - 2.0
    pts[:, 3:6] = nr / np.linalg.norm(nr, axis=1)[:, None]
    pts[0, 3:6] = (0, -1, 0)
    pts[1, 3:6] = (0, 1, 0)
    s = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    s[:3] = (0, 1, 0xFFFFFFFF)
    # t = (r0 * Q) >> 32 of the first xorshift output r0: r0 = 1 gives t = 0, r0 = 0xFFFFFFFF gives t = Q - 1 (Q < 2^32), and the
    # step is a bijection, so the seeds are its inverses; the row ends come from a fixed stream of candidates
    s[3:5] = [unxorshift(1), unxorshift(0xFFFFFFFF)]
    assert (er.xorshift(s[3:5]) == (1, 0xFFFFFFFF)).all()
    cand = np.arange(1, 1 << 16, dtype=np.uint32)
    t = ((er.xorshift(cand).astype(np.uint64) * np.uint64(m["Q"])) >> np.uint64(32)).astype(np.uint32)
    e = np.searchsorted(m["cum"], t, side="right")
    s[5:13] = cand[np.nonzero(e % n == 0)[0][:8]]
    s[13:21] = cand[np.nonzero(e % n == n - 1)[0][:8]]
    return pts, s


def unxorshift(y):
    """the state x with xorshift(x) = y (x ^= x << 13; x ^= x >> 17; x ^= x << 5, each undone by repeating it until the shift runs out)"""
    M = 0xFFFFFFFF
    x = y
    for k in range(5, 32, 5):
        x = y ^ ((x << 5) & M)
    y = x
    x = y ^ (y >> 17)
    y = x
    for k in range(13, 32, 13):
        x = y ^ ((x << 13) & M)
    return x
