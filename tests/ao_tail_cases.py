"""The frames tests/test_gpu_ao_tail.py renders and tests/test_ao_tail_cpu.py shows to be non-vacuous.  TEST INFRASTRUCTURE ONLY.

The tail of an ambient-occlusion frame (render_ao_tail, csrc/rt_secondary.hip) traces spp samples per pixel in batches of
ns = clamp(rays per batch / pixels of the window, 1, spp) samples: 32 Mi rays per batch by default, VXRT_AO_BATCH otherwise.  The
cases are chosen for what that code does with them, not for what they look like:

  name        window               spp   what it is for
  spp7        40 x 24, whole         7   a pixel's samples straddle wavefronts (64 is no multiple of 7); 2880 rays per batch: 3, 3, 1
  spp16       40 x 24, whole        16   four pixels per wavefront; one ray per batch: sixteen batches of one sample
  spp63/64/65 40 x 24, whole  63,64,65   a pixel just short of, exactly and just over one wavefront
  spp130      40 x 24, whole       130   a pixel spans three wavefronts
  spp4096     13 x 7, whole       4096   the header's maximum: a pixel is 64 wavefronts, 16 workgroups
  small65     13 x 7, whole         65   2880 rays per batch: 31, 31, 3 -- segments that straddle wavefronts, and a short last batch
  rows        45 x 27, rows 3..22    5   a row window with y0 > 0; 2880 rays per batch: 3, 2
  one_row     40 x 24, row 11      130   the smallest window; 2880 rays per batch: 72, 58
  cells143    208 x 176, rows 3..176 3   143 cells of 16 x 16 pixels, 1,144 bins: the sort's scan takes 2 counters per thread
  cells272    272 x 256, whole       2   272 cells, 2,176 bins: 3 counters per thread
  all_miss    40 x 24, whole         7   a camera that looks away from the hall: no pixel is listed, every launch of the tail runs on
                                         zero live rays

Scene: scenes.mirror_hall.  Camera form: hall_cameras(w, h)["orbit_1"] with occlusion radius 300 against
camera_secondary_ref.ao_frame, everything equal.  Fixed-camera form: the light, the seed and a radius of
test_ambient_occlusion_pass_matches_oracle (tests/test_gpu_parity.py) against pyoracle.render_ao, held to what that test asserts.
The definition of the frame does not mention batches or an order of the rays, so the same references serve every knob.

`open_or_closed` is the third of the conditions of tests/test_ao_tail_cpu.py -- among the pixels with a hit, one whose samples are
all open or all blocked.  With 65 samples and more no pixel of these frames is either (every hit point of the hall has something
within 300 units in some direction and open sky in another), so those cases ask for partly occluded pixels and misses only; the
counts measured on the CPU are next to each case.  The fixed-camera frames are held to the first two conditions."""
import collections
import functools

import camera_ref as cr
import camera_secondary_ref as csr
import scenes

Case = collections.namedtuple("Case", "name w h y0 y1 spp camera open_or_closed")

CAMERA, AWAY = "orbit_1", "far_cancel"   # (far_cancel: one of the hostile cameras, 2^40 away and looking past the hall)
RADIUS, SEED = 300.0, 7                  # camera form
FIXED_LIGHT, FIXED_RADIUS = (150.0, 220.0, -60.0), 60.0   # fixed-camera form (test_ambient_occlusion_pass_matches_oracle's)

#                                                              hit pixels: open / partly / closed (camera form, measured on the CPU)
CASES = [
    Case("spp7", 40, 24, 0, 24, 7, CAMERA, True),            # 635 of 960: 83 / 547 / 5
    Case("spp16", 40, 24, 0, 24, 16, CAMERA, True),          # 635: 23 / 611 / 1
    Case("spp63", 40, 24, 0, 24, 63, CAMERA, True),          # 635: 2 / 633 / 0
    Case("spp64", 40, 24, 0, 24, 64, CAMERA, True),          # 635: 4 / 631 / 0
    Case("spp65", 40, 24, 0, 24, 65, CAMERA, False),         # 635: 0 / 635 / 0
    Case("spp130", 40, 24, 0, 24, 130, CAMERA, False),       # 635: 0 / 635 / 0
    Case("spp4096", 13, 7, 0, 7, 4096, CAMERA, False),       # 61 of 91: 0 / 61 / 0
    Case("small65", 13, 7, 0, 7, 65, CAMERA, False),         # 61 of 91: 0 / 61 / 0
    Case("rows", 45, 27, 3, 22, 5, CAMERA, True),            # 607 of 855: 138 / 458 / 11
    Case("one_row", 40, 24, 11, 12, 130, CAMERA, False),     # 21 of 40: 0 / 21 / 0
    Case("cells143", 208, 176, 3, 176, 3, CAMERA, True),     # 23,700 of 35,984: 9,594 / 12,976 / 1,130
    Case("cells272", 272, 256, 0, 256, 2, CAMERA, True),     # 46,324 of 69,632: 24,740 / 16,852 / 4,732
    Case("all_miss", 40, 24, 0, 24, 7, AWAY, False),         # 0 of 960
]
BY_NAME = {c.name: c for c in CASES}

SAMPLE_COUNTS = ["spp7", "spp16", "spp63", "spp64", "spp65", "spp130", "spp4096", "small65"]
ROW_WINDOWS = ["rows", "one_row"]
LARGE_WINDOWS = ["cells143", "cells272"]   # the sort's scan: per = ceil(8 * cells / 1024) = 2, 3 (every other case: 1)


def n_cells(case):
    """16 x 16-pixel cells of the window, as render_ao_tail counts them"""
    return ((case.w + 15) // 16) * ((case.y1 - case.y0 + 15) // 16)


def batches(case, rays_per_batch):
    """the samples per batch render_ao_tail takes for `case` with `rays_per_batch` (VXRT_AO_BATCH)"""
    ns = min(case.spp, max(1, rays_per_batch // (case.w * (case.y1 - case.y0))))
    return [min(ns, case.spp - s0) for s0 in range(0, case.spp, ns)]


@functools.lru_cache(maxsize=None)
def hall(vrt):
    return scenes.mirror_hall(vrt)


def camera(vrt, case):
    return csr.hall_cameras(vrt, case.w, case.h)[case.camera]


_REF = {}


def camera_reference(vrt, po, case):
    """csr.ao_frame of the case -- pixels, colours, unoccluded counts (rows of the window), rays traced -- and the indices of its
    pixels with a hit; computed once per process, read-only"""
    if case.name not in _REF:
        b, cam, pp = hall(vrt), camera(vrt, case), po.shade_params()
        prim = csr.primary(b, cr.rays(cam, case.w, case.h, case.y0, case.y1), pp)
        ref = csr.ao_frame(b, cam, case.w, case.h, pp, case.spp, RADIUS, SEED, case.y0, case.y1, prim)
        for a in ref[:3]:
            a.setflags(write=False)
        _REF[case.name] = (ref, prim["fi"])
    return _REF[case.name]


_FIXED = {}


def fixed_reference(vrt, po, case):
    """pyoracle.render_ao of the case from the fixed camera: pixels, colours, unoccluded counts (whole frames; rows outside the window
    are zero), rays traced"""
    if case.name not in _FIXED:
        ref = po.render_ao(hall(vrt), case.w, case.h, po.shade_params(light_pos=FIXED_LIGHT), case.spp, FIXED_RADIUS, SEED, case.y0, case.y1)
        for a in ref[:3]:
            a.setflags(write=False)
        _FIXED[case.name] = ref
    return _FIXED[case.name]


def census(vrt, po, case):
    """pixels of the window, pixels with a hit, and of those the fully open, partly occluded and fully blocked ones (camera form)"""
    (_, _, opn, _), fi = camera_reference(vrt, po, case)
    o = opn.reshape(-1)[fi]
    return opn.size, len(fi), int((o == case.spp).sum()), int(((o > 0) & (o < case.spp)).sum()), int((o == 0).sum())
