"""The cases of tests/test_gpu_denoise.py, which tests/test_denoise_cpu.py shows to be non-vacuous.  TEST INFRASTRUCTURE ONLY.  All seeded.

Synthetic inputs of the filter alone, per frame size: a plane with a crease (two normals whose dot is 0.8), a depth step of 5 units in
the lower rows, a disc of miss pixels that carry a sentinel signal (1e6: a leak would be seen), a hit pixel with a zero normal (every
weight 0: the sw == 0 pass-through), a band of normals that are not unit vectors, one pixel at an infinite position, one NaN signal
pixel, a patch of -0.0 signals, and hit flags other than 1 (2.5 and NaN: `hit != 0`).  The frames thinner than the stencil (1x1, 7x1,
1x5) are too small for those shapes and carry what fits: random signals, one miss pixel, one zero normal."""
import numpy as np

import camera_secondary_ref as csr

f32 = np.float32
INF = float("inf")

# 1x1, 7x1, 1x5: thinner than the stencil; 45x37: odd, two tiles wide; 64x64: whole 32 x 8 tiles; 130x70: several tiles, and from step 8
# on a halo (2 * step) larger than a tile
FRAMES = ((1, 1), (7, 1), (1, 5), (45, 37), (64, 64), (130, 70))
BIG = ((45, 37), (64, 64), (130, 70))
ITERATIONS = (1, 2, 3, 4, 5, 6)   # steps up to 32: beyond the small frames
# (normal_power, sigma_z, sigma_l); the last one is the unguided filter
VARIANTS = ((2, 1.0, 0.3), (0, INF, 0.3), (7, 1.0, INF), (0, INF, INF))
GUIDED, UNGUIDED = VARIANTS[0], VARIANTS[3]
SENTINEL = 1e6
NOISE = 0.15


def synthetic(w, h, seed=1):
    """S (h, w, 3), P (h, w, 4), N (h, w, 4) float32 and the noise-free base (h, w, 3) with `clean`, the mask of ordinary hit pixels"""
    rng = np.random.RandomState(seed * 1000003 + w * 131 + h)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    right = xs >= w / 2.0
    low = ys >= 0.7 * h
    z = np.where(right, 10.0 + 0.75 * (xs - w / 2.0), 10.0) + np.where(low, 5.0, 0.0)   # the tilted half's plane: normal (-0.6, 0, 0.8)
    P = np.stack([xs, ys, z, np.ones_like(xs)], 2).astype(np.float32)
    N = np.zeros((h, w, 4), np.float32)
    N[..., 2] = 1.0
    N[right] = (-0.6, 0.0, 0.8, 0.0)
    base = np.zeros((h, w, 3), np.float32)
    base[...] = (0.2, 0.25, 0.3)
    base[right] = (0.8, 0.7, 0.6)
    base[low] = base[low] * f32(0.5)
    S = (base + rng.normal(0.0, NOISE, (h, w, 3))).astype(np.float32)
    clean = np.ones((h, w), bool)
    if w >= 8 and h >= 8:
        disc = (xs - 0.3 * w) ** 2 + (ys - 0.4 * h) ** 2 <= (min(w, h) / 6.0) ** 2
        P[disc] = (7.0, -3.0, 1e9, 0.0)
        N[disc] = (0.3, 0.3, 0.3, 9.0)
        S[disc] = SENTINEL
        band = ys < h / 5.0
        N[band, 0:3] *= rng.uniform(0.5, 2.0, (int(band.sum()), 1)).astype(np.float32)
        zy, zx = h // 4 + 1, (3 * w) // 4
        N[zy, zx, 0:3] = 0.0
        iy, ix = h // 2, w // 8
        P[iy, ix, 0] = INF
        ny, nx = (2 * h) // 3, (2 * w) // 3
        S[ny, nx, 1] = np.nan
        S[h - 3:h - 1, 2:5] = -0.0
        P[h - 2, w - 2, 3] = 2.5
        P[h - 2, w - 3, 3] = np.nan
        clean &= ~disc
        for y, x in ((zy, zx), (iy, ix), (ny, nx)):
            clean[y, x] = False
        clean[h - 3:h - 1, 2:5] = False
    else:
        if w * h >= 5:
            P.reshape(-1, 4)[1, 3] = 0.0
            S.reshape(-1, 3)[1] = SENTINEL
            N.reshape(-1, 4)[3, 0:3] = 0.0
            S.reshape(-1, 3)[2] = -0.0
    return S, P, N, base, clean


def cases(w, h):
    """(iterations, normal_power, sigma_z, sigma_l) of every synthetic case of a frame"""
    return [(it,) + v for it in ITERATIONS for v in VARIANTS]


# ---- the denoised path frame: scenes.mirror_hall at 96 x 64 ----
W, H = csr.W, csr.H
PATH_CONFIGS = ((2, 3, 1, 3), (5, 2, 0, 0))   # (spp, bounces, shadow, seed), as path_ref.CONFIGS
PATH_CAMERAS = ("framing", "inside_blob", "non_orthonormal", None)   # None: the fixed camera
PATH_WINDOW = (8, 40)
# The hall is about 500 units across (cameras orbit it at a radius of 260).  sigma_z = 1/250 of that: across a wall seen at a grazing
# angle neighbouring pixels stay in the tangent plane (weight 1), while the blob and the steps between the walls and the floor are tens
# of units off it (weight far below 0.5).  sigma_l is a quarter of the light's 1.0: the 2-spp noise of E exceeds it between some
# neighbours, not between most.  normal_power 5 (dot^32) halves the weight at 12 degrees.
HALL_EXTENT = 500.0
PATH_DN = (3, 5, HALL_EXTENT / 250.0, 0.25)   # (iterations, normal_power, sigma_z, sigma_l)
