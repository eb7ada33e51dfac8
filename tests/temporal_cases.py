"""The cases of tests/test_gpu_temporal.py, which tests/test_temporal_cpu.py shows to be non-vacuous.  TEST INFRASTRUCTURE ONLY.  All seeded.

Synthetic sequences are pinhole views (camera_ref.rays) of an analytic scene, intersected here in float64, so that reprojection lands
somewhere sensible: a floor (y = 0), a back wall with a step in it (z = 30 left of x = 5, z = 24 right of it: two surfaces with the same
normal, 6 units apart, for the plane test), a sphere in front of the wall (normals that turn, and a silhouette), and the sky where none of
them is hit.  The signal is a smooth function of the WORLD point, so a surface keeps its value from frame to frame, plus independent noise
per frame.

Per frame of at least 8 x 8 the guides are made hostile where denoise_cases makes them so, at fixed places of the screen: a disc of miss
pixels that carry a sentinel signal (1e6: a leak would be seen), a hit pixel with a zero normal, one pixel at an infinite and one at a NaN
position, hit flags 2.5 and NaN, one NaN signal pixel and a patch of -0.0 signals.  The frames thinner than that carry what fits.

A sequence is a list of cameras; frame k is accumulated onto the history of frame k - 1, so cameras[k - 1] is the PREVIOUS camera of frame k."""
import math

import numpy as np

import camera_ref as cr

f32 = np.float32
INF = float("inf")

FRAMES = ((1, 1), (7, 1), (1, 5), (45, 37), (64, 64), (130, 70))   # as denoise_cases.FRAMES: thin ones, odd, whole tiles, several tiles
BIG = ((45, 37), (64, 64), (130, 70))
SENTINEL = 1e6
NOISE = 0.15
# (alpha_min, max_len, sigma_z, normal_min)
DEFAULT = (0.1, 32, 0.5, 0.9)
CAP = (0.05, 3, 0.5, 0.9)            # the third frame of a static sequence reaches max_len
ALPHA_ONE = (1.0, 8, INF, -2.0)      # no accumulation: out = Eh + 1 * (E - Eh); both guide tests switched off
EYE, TARGET = (0.0, 5.0, -4.0), (1.0, 3.0, 15.0)


def _norm(v):
    return v / math.sqrt(float(np.dot(v, v)))


def look_at(eye, target, w, h, vfov=0.9):
    """14 floats: forward = normalize(target - eye), right = normalize(forward x up), up = right x forward, viewplane = 2 tan(vfov / 2) * (w / h, 1)"""
    e, t = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = _norm(t - e)
    r = _norm(np.cross(f, (0.0, 1.0, 0.0)))
    u = np.cross(r, f)
    vh = 2.0 * math.tan(0.5 * vfov)
    return np.array(list(e) + list(f) + list(r) + list(u) + [vh * w / h, vh], np.float32)


def yaw(cam, pixels, w):
    """the camera turned about its up axis by `pixels` pixels of the frame's centre"""
    c = np.array(cam, np.float64)
    a = math.atan(pixels * c[12] / w)
    f, r = c[3:6].copy(), c[6:9].copy()
    c[3:6], c[6:9] = f * math.cos(a) + r * math.sin(a), r * math.cos(a) - f * math.sin(a)
    return c.astype(np.float32)


def dolly(cam, units):
    c = np.array(cam, np.float64)
    c[0:3] += units * c[3:6]
    return c.astype(np.float32)


def turned(cam):
    """looks the other way: every point the camera saw is behind it"""
    c = np.array(cam, np.float32)
    c[3:6], c[6:9] = -c[3:6], -c[6:9]
    return c


def non_orthonormal(cam):
    c = np.array(cam, np.float64)
    f, r, u = c[3:6].copy(), c[6:9].copy(), c[9:12].copy()
    c[6:9], c[9:12] = r + 0.3 * f, 1.5 * u + 0.2 * r
    return c.astype(np.float32)


def singular(cam):
    """up = right: the basis spans a plane, its reciprocal is infinities and NaNs"""
    c = np.array(cam, np.float32)
    c[9:12] = c[6:9]
    return c


def zero_viewplane(cam):
    c = np.array(cam, np.float32)
    c[12:14] = 0.0
    return c


def view(cam14, w, h, y0, y1):
    """the analytic scene seen through rows [y0, y1): P (rows, w, 4) = (I, 1) | 0, N (rows, w, 4) = (n, 0) | 0, base (rows, w, 3)"""
    r = cr.rays(cam14, w, h, y0, y1).astype(np.float64)
    o, d = r[:, 0:3], r[:, 3:6]
    n = len(r)
    t = np.full(n, np.inf)
    nr = np.zeros((n, 3))

    def closer(tt, ok, normal):
        ok = ok & (tt > 1e-3) & (tt < t)
        t[ok] = tt[ok]
        nr[ok] = normal[ok] if isinstance(normal, np.ndarray) else normal

    with np.errstate(all="ignore"):
        tf = -o[:, 1] / d[:, 1]                                             # the floor
        pf = o + tf[:, None] * d
        closer(tf, (np.abs(pf[:, 0]) < 40) & (np.abs(pf[:, 2]) < 40), (0.0, 1.0, 0.0))
        for z, xlo, xhi in ((30.0, -25.0, 5.0), (24.0, 5.0, 25.0)):         # the wall and its step
            tw = (z - o[:, 2]) / d[:, 2]
            pw = o + tw[:, None] * d
            closer(tw, (pw[:, 0] >= xlo) & (pw[:, 0] < xhi) & (pw[:, 1] > 0) & (pw[:, 1] < 14), (0.0, 0.0, -1.0))
        cen, rad = np.array((0.0, 3.0, 15.0)), 3.0                          # the sphere
        oc = o - cen
        bq = (oc * d).sum(1)
        disc = bq * bq - ((oc * oc).sum(1) - rad * rad)
        ts = -bq - np.sqrt(disc)
        ps = o + ts[:, None] * d
        closer(ts, disc > 0, (ps - cen) / rad)
        hit = np.isfinite(t)
        I = o + np.where(hit, t, 0.0)[:, None] * d
        base = np.stack([0.5 + 0.25 * np.sin(0.9 * I[:, 0] + 0.4 * I[:, 2]), 0.4 + 0.2 * np.cos(0.7 * I[:, 1] + 0.5 * I[:, 0]),
                         0.3 + 0.2 * np.sin(0.3 * I[:, 2])], 1)
    P = np.zeros((n, 4), np.float32)
    N = np.zeros((n, 4), np.float32)
    P[hit, 0:3], P[hit, 3] = I[hit], 1.0
    N[hit, 0:3] = nr[hit]
    base = np.where(hit[:, None], base, 0.0).astype(np.float32)
    return P.reshape(y1 - y0, w, 4), N.reshape(y1 - y0, w, 4), base.reshape(y1 - y0, w, 3)


def frame(cam14, w, h, y0, y1, seed, hostile=True, noise=NOISE):
    """E (rows, w, 3), P, N (rows, w, 4), the noise-free base and `clean`, the mask of ordinary hit pixels"""
    rows = y1 - y0
    rng = np.random.RandomState(seed * 1000003 + w * 131 + h)
    P, N, base = view(cam14, w, h, y0, y1)
    E = (base + rng.normal(0.0, noise, (rows, w, 3))).astype(np.float32)
    miss = P[..., 3] == 0
    E[miss] = SENTINEL
    clean = ~miss
    if not hostile:
        return E, P, N, base, clean
    ys, xs = np.mgrid[0:rows, 0:w].astype(np.float32)
    if w >= 8 and rows >= 8:
        disc = (xs - 0.3 * w) ** 2 + (ys - 0.4 * rows) ** 2 <= (min(w, rows) / 6.0) ** 2
        P[disc] = (7.0, -3.0, 1e9, 0.0)
        N[disc] = (0.3, 0.3, 0.3, 9.0)
        E[disc] = SENTINEL
        clean &= ~disc
        spots = {"zero_normal": (rows // 4 + 1, (3 * w) // 4), "inf_pos": (rows // 2, w // 8), "nan_pos": (rows // 2 + 2, w // 8 + 1),
                 "nan_sig": ((2 * rows) // 3, (2 * w) // 3), "flag_25": (rows - 2, w - 2), "flag_nan": (rows - 2, w - 3)}
        N[spots["zero_normal"]][0:3] = 0.0
        P[spots["inf_pos"]][0] = INF
        P[spots["nan_pos"]][1] = np.nan
        E[spots["nan_sig"]][1] = np.nan
        P[spots["flag_25"]][3] = 2.5
        P[spots["flag_nan"]][3] = np.nan
        for k in ("flag_25", "flag_nan"):       # (hits by their flag, whatever the scene has there: not the sentinel of a miss)
            E[spots[k]] = (0.25, 0.5, 0.75)
        E[rows - 3:rows - 1, 2:5] = -0.0
        for y, x in spots.values():
            clean[y, x] = False
        clean[rows - 3:rows - 1, 2:5] = False
    elif w * rows >= 5:
        P.reshape(-1, 4)[1] = 0.0
        E.reshape(-1, 3)[1] = SENTINEL
        N.reshape(-1, 4)[3, 0:3] = 0.0
        E.reshape(-1, 3)[2] = -0.0
        clean.reshape(-1)[1:4] = False
    return E, P, N, base, clean


def sequences(w, h):
    """name -> (cameras, (y0, y1), prm) of a frame size"""
    c0 = look_at(EYE, TARGET, w, h)
    seq = {
        "static": ([c0] * 4, (0, h), CAP),
        "pan": ([c0, yaw(c0, 0.3, w), yaw(c0, 7.7, w), yaw(c0, 7.4, w)], (0, h), DEFAULT),     # a fraction of a pixel, many pixels
    }
    if (w, h) in BIG:
        win = (h // 5, h - h // 4)                                                            # a row window with y0 > 0
        seq["dolly_window"] = ([dolly(c0, 1.5 * k) for k in range(4)], win, DEFAULT)
        seq["pan_alpha_one"] = ([yaw(c0, 2.5 * k, w) for k in range(3)], win, ALPHA_ONE)
        seq["hostile_previous"] = ([c0, turned(c0), c0, non_orthonormal(c0), c0, singular(c0), c0, zero_viewplane(c0), c0], (0, h), DEFAULT)
    return seq


def frames(w, h, name, hostile=True):
    """the frames of a sequence: a list of (cam14, E, P, N, base, clean), with its window and prm"""
    cams, win, prm = sequences(w, h)[name]
    return [(c,) + frame(c, w, h, win[0], win[1], 7 + k, hostile) for k, c in enumerate(cams)], win, prm


def all_sequences():
    return [(w, h, name) for w, h in FRAMES for name in sequences(w, h)]


# ---- the path frame with temporal accumulation: scenes.mirror_hall at 96 x 64 (denoise_cases.W, H, PATH_CONFIGS, PATH_WINDOW, PATH_DN) ----
# an orbit step, a dolly and one cut (rtapi.look_at(eye, centre, up, 1.0, W, H)); the hall is about 500 units across
PATH_CENTRE = (180.0, 90.0, 0.0)
PATH_EYES = ((363.8, 140.0, 183.8), (347.1, 140.0, 199.2), (328.2, 134.3, 176.6), (-3.8, 140.0, -183.8))
PATH_TP = (0.2, 3, 2.0, 0.9)   # sigma_z as denoise_cases.PATH_DN's; max_len 3: the fourth frame of a static pixel would be capped
