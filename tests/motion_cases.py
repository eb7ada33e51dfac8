"""The moving scene of tests/test_motion_cpu.py and tests/test_gpu_motion.py.  TEST INFRASTRUCTURE ONLY.

scenes.mirror_hall at 64 x 48, seen from inside the hall, 153 units from the centre of the blob (instance 3, about 80 units across: some
30 pixels).  A pixel at the centre's distance is 153 * 2 tan(0.45) / 48 = 3.08 units and one on the blob's near side about 2.6, so the
blob's step of 3.9 units along x per frame is 1.5 pixels of the surface that is seen (tests/test_motion_cpu.py measures it).  Frame k
sees the blob at k steps; the snapshot it is rendered with is the scene of frame k - 1 (of frame 0 for frame 0: nothing has moved yet)."""
import numpy as np

import motion_ref as mr
import scenes
import temporal_cases as tc

W, H = 64, 48
N_FRAMES = 6
BLOB = 3
EYE, TARGET = (180.0, 120.0, -120.0), (180.0, 90.0, 30.0)
STEP = (3.9, 0.0, 0.0)
YAW = 0.4                       # pixels per frame, for the sequences whose camera turns
TP = (0.2, 32, 2.0, 0.9)        # sigma_z as denoise_cases.PATH_DN's; max_len beyond the six frames


def translation(k):
    m = np.eye(4, dtype=np.float32)
    m[0:3, 3] = np.float32(k) * np.asarray(STEP, np.float32)
    return m


def cameras(yaw=True):
    c0 = tc.look_at(EYE, TARGET, W, H)
    return [tc.yaw(c0, YAW * k, W) if yaw else c0 for k in range(N_FRAMES)]


def hall(vrt):
    b = scenes.mirror_hall(vrt)
    rec = b["blas"].view(np.float32).reshape(-1, 40)
    assert (rec[BLOB, 17:33] == np.eye(4, dtype=np.float32).reshape(-1)).all()      # (the blob starts where its vertices are)
    return b


def sequence(b):
    """[(scene of frame k, the snapshot frame k is rendered with)]"""
    out, prev = [], b
    for k in range(N_FRAMES):
        cur = b if k == 0 else mr.moved(b, BLOB, translation(k)[None])
        out.append((cur, mr.snapshot(prev)))
        prev = cur
    return out
