"""The cases tests/test_gpu_adaptive.py runs and tests/test_adaptive_cpu.py shows to be non-vacuous: count maps, the configurations
they go with, the batch size of the child process and the hostile table of vxrt_sample_counts."""
import numpy as np

import camera_secondary_ref as csr

W, H = csr.W, csr.H
f32 = np.float32
U32_MAX = 0xFFFFFFFF


def hashed(w, h, values, salt=0):
    """(h, w) uint32: values[hash of the pixel index % len(values)] -- neighbouring pixels get unrelated counts"""
    i = np.arange(w * h, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B9)
    k = ((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)
    return np.asarray(values, np.uint32)[(k % np.uint64(len(values))).astype(np.int64)].reshape(h, w)


# the mosaic identity: every pixel against the uniform frame of its count (GPU against GPU)
MOSAIC = {"values": (1, 2, 5), "cap": 5, "bounces": 3, "shadow": 1, "seed": 3}
# against the restatement: raw 0 (= 1), raw 0xFFFFFFFF and raw cap + 2 (= cap), four distinct clamped values
RESTATED = {"values": (0, 2, U32_MAX, 6, 3), "cap": 4, "bounces": 2, "shadow": 1, "seed": 3}
# the scan levels: bounces 1, counts of 1 and 2
SCAN = {"values": (1, 2), "cap": 2, "bounces": 1, "shadow": 0, "seed": 5}
# VXRT_PATH_BATCH of the child process: a prime, so that batch boundaries fall inside pixels' samples and the last batch is short
CHILD_BATCH = 997
# the two maps of the frames in flight
IN_FLIGHT = ({"values": (1, 3, 4), "cap": 4, "bounces": 2, "shadow": 1, "seed": 3, "salt": 1},
             {"values": (2, 0, 9), "cap": 3, "bounces": 3, "shadow": 0, "seed": 11, "salt": 2})
# the variance frame with counts that are not uniform (cap 3: clamped values 1, 2, 3)
VARIANCE = {"values": (1, 3, 0, 2, 7), "cap": 3, "bounces": 2, "shadow": 1, "seed": 3}
# the closed loop: (gain, min_spp, max_spp) of vxrt_sample_counts; the first frame's counts are all 2
LOOP = {"prm": (128.0, 1, 4), "cap": 4, "bounces": 2, "shadow": 1, "seed": 7, "first": 2, "frames": 3}


def counts_of(case, w=W, h=H):
    return hashed(w, h, case["values"], case.get("salt", 0))


def _ulp(x, k):
    return (np.array([x], np.float32).view(np.int32) + np.int32(k)).view(np.float32)[0]


def hostile_variances(prm):
    """variances for vxrt_sample_counts with parameters prm = (gain, min_spp, max_spp), gain a power of two: NaN, +-inf, negatives, +-0,
    denormals, 3e38, products that land exactly on an integer, and values one ulp either side of min_spp and max_spp"""
    gain, lo, hi = f32(prm[0]), prm[1], prm[2]
    v = [np.nan, np.inf, -np.inf, -1.0, -1e-30, 0.0, -0.0, 1e-45, -1e-45, 1e-39, 3e38, -3e38]
    for k in (1, 2, 3, lo, lo + 1, hi - 1, hi, hi + 1, 4096, 4097):
        exact = f32(k) / gain                   # (a power of two: the product is k again)
        v += [exact, _ulp(exact, -1), _ulp(exact, 1)]
    v += [0.3, 0.5, 1.0, 7.25, 100.0, 1e4, 1e9]
    return np.array(v, np.float32)


SAMPLE_PRMS = ((0.5, 2, 16), (4.0, 1, 4096), (1.0, 3, 3), (0.125, 1, 7))   # (gain, min_spp, max_spp): gains are powers of two
SAMPLE_SIZES = (1, 255, 256, 257, 6144)


def sample_inputs(n, prm, seed):
    """(variance, prev_counts) of n entries: the hostile table first (as much of it as fits), then a spread of magnitudes; prev_counts
    with 0, 1, 4096, 4097 and 0xFFFFFFFF among them"""
    rng = np.random.RandomState(seed)
    v = np.exp(rng.uniform(-8.0, 10.0, n)).astype(np.float32)
    t = hostile_variances(prm)[:n]
    v[:len(t)] = t
    prev = rng.randint(0, 12, n).astype(np.uint32)
    prev[rng.permutation(n)[: max(1, n // 7)]] = np.array([0, 4096, 4097, U32_MAX, 5000, 1], np.uint32)[rng.randint(0, 6, max(1, n // 7))]
    return v, prev
