"""The scene, cameras and configurations of tests/test_path_frame_cpu.py and tests/test_gpu_path_frame.py.  TEST INFRASTRUCTURE ONLY.

The scene is emissive_mis_cases.hall("full"): scenes.mirror_hall with the ceiling light and the leaning lamp, the pair list shuffled.
The cameras stand in front of the blob and look past it at the lamp, so that some primary hits emit (D != Lit_0), the blob and the
ceiling panel block some emitter rays, and the surfaces that face away from both lights skip theirs.  They move by a few units per frame:
a temporal sequence that reprojects most pixels and loses some."""
import numpy as np

import adaptive_cases as ac
import camera_secondary_ref as csr
import denoise_cases as dc
import emissive_cases as ec
import emissive_mis_cases as mc
import emissive_mis_ref as mir
import emissive_ref as er
import temporal_cases as tc
import variance_cases as vc

W, H = csr.W, csr.H
SCALE = mc.SCALE
FORMS = ("nee0", "nee1", "mis")
EYES = ((150.0, 110.0, -200.0), (156.0, 112.0, -196.0), (163.0, 113.0, -190.0))
TARGET = (210.0, 125.0, 140.0)
CONFIG = (2, 2, 1, 3)                       # (spp, bounces, shadow, seed) of the frames against the restatement
DN, TP, VP = dc.PATH_DN, tc.PATH_TP, vc.PATH_VP
# counts below 1, 1, between, the cap and above the cap (the mosaic identity and the restated counts frames)
COUNTS = {"values": (0, 1, 3, 4, 9, ac.U32_MAX), "cap": 4, "bounces": 2, "shadow": 1, "seed": 3}
VARIANCE_COUNTS = {"values": (1, 3, 0, 2, 7), "cap": 3, "bounces": 2, "shadow": 1, "seed": 3}
# paths per batch of the child process of the small-batch test: a capacity under 256 paths -- one workgroup of the emitter-ray kernel,
# its last wavefront partly live -- and no multiple of 64
CHILD_BATCH = 193
LAMP_STEP = (-6.0, 3.0, -9.0)               # the lamp's move of the motion test, world units


def hall(vrt):
    """(scene buffers, pairs)"""
    return mc.hall(vrt, "full")


def cameras(vrt, n=3, w=W, h=H):
    return [np.array(vrt.rtapi.look_at(e, TARGET, (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32) for e in EYES][:n]


def emitter(form, b, pairs, scale=SCALE):
    """the emitter form as tests/path_frame_ref.py takes it"""
    if form is None:
        return None
    if form == "nee0":
        return ("nee0", scale)
    tab = er.table(b, pairs)
    return ("nee1", scale, tab) if form == "nee1" else ("mis", scale, tab, mir.index(pairs))


def counts_of(case, w=W, h=H, salt=0):
    return ac.hashed(w, h, case["values"], salt)


def moved_lamp():
    m = ec.lamp_transform().copy()
    m[0:3, 3] += np.asarray(LAMP_STEP, np.float32)
    return m
