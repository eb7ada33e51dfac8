"""The scenes and configurations of tests/test_roulette_cpu.py and tests/test_gpu_roulette.py.  TEST INFRASTRUCTURE ONLY.

All of it is path_frame_cases.hall -- the mirror hall with the ceiling light and the leaning lamp -- with the diffuse colours of its
seven untextured materials set, which is what Alb reads:
  dark    every material (0.6, 0.5, 0.4), the blob black.  thr falls below 1 at the first bounce hit, so every vertex draws; a path
          that meets the blob has thr = 0 exactly, m = 0 < q_min, and survives with q_min.
  white   every material (1.0, 0.6, 0.3): max(Alb) = 1 exactly everywhere, so max(thr) = 1 at every vertex and nothing ever draws.
The emissive colours, and with them the emitter table, are the hall's.

The cases (the table of the issue; `first`, `q_min` = the roulette part, the rest as path_frame_cases.CONFIG names it):
  a   dark, first 1, q_min 0.05, 6 bounces x 3 spp, 21 x 14 with rows 3..12: 567 paths at most, 6 alive at the last depth
  b   a with q_min = 2^-30, from a's camera and from csr.hall_cameras' "inside_blob": a path that met the blob dies for certain (xi <
      2^-30 takes one of four hash outputs), so from inside the blob every path of every batch is dead after the first draw and the
      launches of depths 1 .. 5 fall through on a live count of 0
  c   white: the frame without roulette, bit for bit
  d   first >= bounces (equal, and 16 > bounces): no vertex is in first .. bounces - 1
  e   q_min = 1: q >= 1 always
  f   dark, each emitter form, shadow = 1
  g   counts mixed 1 .. cap and beyond, without an emitter form and with MIS
  h   the variance chain, two frames of a moving camera on one history, with emitter sampling"""
import numpy as np

import adaptive_cases as ac
import path_frame_cases as fc

SCALE = fc.SCALE
W, H = 16, 12
ODD_W, ODD_H, ODD_ROWS = 21, 14, (3, 12)
BLOB_MATERIAL = 3
DARK, WHITE = (0.6, 0.5, 0.4), (1.0, 0.6, 0.3)
Q_TINY = 2.0 ** -30
A = dict(first=1, q_min=0.05, spp=3, bounces=6, shadow=1, seed=3)
B = dict(A, q_min=Q_TINY)
C = dict(first=1, q_min=0.05, spp=2, bounces=3, shadow=1, seed=5)
D = (dict(C, first=3), dict(C, first=16))
E = dict(C, q_min=1.0)
F = dict(first=1, q_min=0.05, spp=2, bounces=4, shadow=1, seed=7)
FORMS = ("nee0", "nee1", "mis")
G = dict(first=2, q_min=0.05, spp=4, bounces=4, shadow=1, seed=3, values=(0, 1, 3, 4, 9, ac.U32_MAX))
G_FORMS = (None, "mis")
HH = dict(first=1, q_min=0.05, spp=2, bounces=3, shadow=1, seed=3, form="nee1")
CHILD_BATCH = fc.CHILD_BATCH
# the frames of the unbiasedness test, 16 x 12: the frame without roulette from seed 1, the frames with it from seed 2
UNBIASED = dict(first=1, q_min=0.05, spp=128, bounces=4, shadow=1, seeds=(1, 2), forms=(None, "mis"))


def _recolour(b, diffuse, blob=None):
    m = b["mat"].view(np.float32).reshape(-1, 22)
    assert len(m) == 7
    m[:, 3:6] = diffuse
    if blob is not None:
        m[BLOB_MATERIAL, 3:6] = blob
    return b


def dark(vrt):
    """(scene buffers, pairs)"""
    b, pairs = fc.hall(vrt)
    return _recolour(b, DARK, (0.0, 0.0, 0.0)), pairs


def white(vrt):
    b, pairs = fc.hall(vrt)
    return _recolour(b, WHITE), pairs


def cameras(vrt, n=1, w=W, h=H):
    return fc.cameras(vrt, n, w, h)


def counts_of(w=W, h=H, salt=0):
    return ac.hashed(w, h, G["values"], salt)


def hostile(q_min, n=4096, seed=9):
    """(thr (n, 3) f32, seeds (n,) u32) of the step alone: random throughputs over [0, 1.5) with hostile components mixed in -- NaN,
    +-inf, 0, -0, negatives, denormals, exactly q_min, exactly 1, the largest float below 1 -- in every channel and in whole rows, and
    hash outputs with 0, 1 and 0xFFFFFFFF among them"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 1.5, (n, 3)).astype(np.float32)
    t[n // 2:] *= np.float32(0.2)                         # (rows that draw)
    edge = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -0.5, -3.0, 1e-40, -1e-40, 1.4e-45, q_min, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)),
                     np.nextafter(np.float32(q_min), np.float32(0.0)), np.nextafter(np.float32(q_min), np.float32(1.0)), 3e38], np.float32)
    k = 0
    for e in edge:
        for ch in range(3):
            t[k, ch] = e                                  # one channel hostile, the others random
            k += 1
        t[k] = e                                          # the whole row
        k += 1
        t[k] = (e, np.float32(0.5) * np.float32(q_min), np.float32(0.3))
        k += 1
    t[k:k + 6] = [(np.nan, 0.5, 0.2), (0.5, np.nan, 0.2), (0.2, 0.5, np.nan), (1e-40, 2e-40, 3e-40), (0.0, -0.0, 0.0), (-1.0, -2.0, -np.inf)]
    s = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    s[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
    s[k:k + 2] = (0, 1)
    return t, s
