"""The cases of tests/test_gpu_variance.py, which tests/test_variance_cpu.py shows to be non-vacuous.  TEST INFRASTRUCTURE ONLY.  All seeded.

Sizes are denoise_cases.FRAMES (1x1, 7x1 and 1x5 are thinner than every stencil here, 45x37 is odd, 64x64 is whole tiles, at 130x70 steps
8 and above reach past a tile); sequences are temporal_cases' with their hostile guides (static, panned 0.3 and 7 pixels, dolly, turned
away, singular).  Added to them: the parameters of the initial variance (min_len 1: never spatial; 4; 64: above every max_len of the
sequences, always spatial; radius 1 and 3), epsilon 1e-6 and 1.0, and, for the filter alone, a variance field with single pixels that are
0, NaN, negative and +inf."""
import numpy as np

import camera_ref as cr
import denoise_cases as dc
import temporal_cases as tc

f32 = np.float32
INF = float("inf")

FRAMES, BIG = dc.FRAMES, dc.BIG
# (epsilon, min_len, radius)
VPS = ((1e-6, 1, 1), (1e-6, 4, 3), (1.0, 64, 1), (1.0, 4, 1))
NEVER_SPATIAL, DEFAULT, ALWAYS_SPATIAL = VPS[0], VPS[1], VPS[2]
# (normal_power, sigma_z) of the initial variance's weights: guided, and both guides switched off
V0_GUIDES = ((2, 1.0), (0, INF))
# the filter alone: (normal_power, sigma_z, sigma_l, epsilon).  sigma_l multiplies a standard deviation here, so it is of order 1.
FILTER_VARIANTS = ((2, 1.0, 4.0, 1e-6), (2, 1.0, 4.0, 1.0), (0, INF, 1.0, 1e-6), (7, 1.0, INF, 1.0), (0, INF, INF, 1e-6))
ITERATIONS = dc.ITERATIONS
V_SCALE = 0.05


def filter_cases():
    """(iterations, normal_power, sigma_z, sigma_l, epsilon) of every case of a frame"""
    return [(it,) + v for it in ITERATIONS for v in FILTER_VARIANTS]


def variance(w, h, seed=3):
    """V (h, w) float32 for denoise_cases.synthetic(w, h): positive noise, and single pixels 0, NaN, negative, +inf (what fits)"""
    rng = np.random.RandomState(seed * 7919 + w * 131 + h)
    V = rng.uniform(0.0, V_SCALE, (h, w)).astype(np.float32)
    if w >= 8 and h >= 8:
        spots = {"zero": (h // 2 + 1, w // 2 + 2), "nan": (h // 3, (2 * w) // 3 + 1), "negative": ((3 * h) // 5, w // 5), "inf": (h // 5 + 2, w // 2)}
        V[spots["zero"]] = 0.0
        V[spots["nan"]] = np.nan
        V[spots["negative"]] = -40.0       # (drags the prefiltered variance of its neighbours below zero: a NaN scale)
        V[spots["inf"]] = INF
    elif w * h >= 5:
        V.reshape(-1)[0] = 0.0
        V.reshape(-1)[2] = -1.0
        V.reshape(-1)[4] = np.nan
    return V


def all_sequences():
    return tc.all_sequences()


# ---- a flat all-hit plane seen from temporal_cases' camera: what the statistical checks of tests/test_variance_cpu.py accumulate on ----
PLANE_DEPTH = 10.0
PLANE_TP = (0.01, 32, INF, -2.0)    # al = 1 / L for the first 32 frames; every tap kept


def plane(w, h):
    """(cam14, P, N) of the plane dot(I - eye, forward) = PLANE_DEPTH: every pixel a hit, reprojection lands on the pixel itself"""
    cam = tc.look_at(tc.EYE, tc.TARGET, w, h)
    r = cr.rays(cam, w, h, 0, h).astype(np.float64)
    f = cam[3:6].astype(np.float64)
    t = PLANE_DEPTH / (r[:, 3:6] @ f)
    I = r[:, 0:3] + t[:, None] * r[:, 3:6]
    P = np.concatenate([I, np.ones((len(I), 1))], 1).astype(np.float32).reshape(h, w, 4)
    N = np.zeros((h, w, 4), np.float32)
    N[..., 0:3] = -cam[3:6]
    return cam, P, N


def grey(base, sigma, rng):
    """base (h, w) luminance plus Gaussian noise of standard deviation sigma (a number or (h, w)), the same on the three channels: the
    weights of lum() sum to 1, so the luminance has that noise"""
    n = rng.normal(0.0, 1.0, base.shape) * sigma
    return np.repeat((base + n)[..., None], 3, 2).astype(np.float32)


# ---- the frame: scenes.mirror_hall at 96 x 64, as temporal_cases / motion_cases; 4 frames of temporal_cases.PATH_EYES ----
PATH_VP = (1e-3, 3, 2)              # min_len 3 = PATH_TP's max_len: frames 0 and 1 are spatial everywhere, later ones where history was lost
N_PATH_FRAMES = 4
