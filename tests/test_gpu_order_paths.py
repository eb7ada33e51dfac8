"""GPU: the ordered node step without the sorting network (RT_ORDER_PATHS: csrc/rt_order.h, rt_traverse_loop.inc) against the oracle on
the same inputs -- hit records (dist, bx, by, bz, blasIdx, triIdx, the occlusion bit) and packed pixels bit for bit, the status word zero
-- on the shipped library and, in child processes, through the general kernels, the 8-wavefront kernels and the variant library, whose
check mode (-DRT_ORDER_CHECK=1) evaluates the network beside every step that skips it and reports a difference in the status word.

A run of the ordered arm (all node lanes of a wavefront taking one node step) asks how many valid children its lanes hold at most: none
or one -> path A (the valid child is taken, nothing is pushed, no network); two, three or four -> the network.  The switch between the
two is per run, so what can go wrong is a run of the wrong class, a lane of a mixed run, or the state a skipped step leaves for the
steps with the network behind it (the stack height, the register top, the path maximum, the overflow status).  The trees here are made
by hand (test_gpu_stack_push._tree_scene: nested lists, a leaf is one triangle) so that a step's class is known: a child that must not
be valid is a triangle BEHIND the fixed camera ((0,100,0) looking along +x), whose box no camera ray enters; children that must be valid
face the camera in planes x = const.  The counting build classes the runs (vxrt_debug_child_counts: at most 0, 1, 2, 3 or more valid
children), and the tests assert that the classes they are built for are the ones that ran.

The shortcut is built into the identity-root shadow frame kernels: the shadow frames of the hand-made trees and the atrium take it for
their primary rays (and for occlusion rays in wavefronts that still hold primary rays); their plain frames, the translated scenes and
VXRT_IDENT_ROOT=0 run the same trees through kernels that keep the network, which must agree with the same oracle.

Frames of 16 x 16 (four tiles), 64 x 64 and a ragged 13 x 7 (tiles with lanes outside the frame)."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import _bits, _occlusion_oracle, gpu_render
from test_gpu_stack_push import _chain, _translated, _tree_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((16, 16), (64, 64), (13, 7))
LIGHT = (-50.0, 180.0, 40.0)                             # beside the camera: occlusion rays run back towards it
STATUS_STACK_OVERFLOW = 1


def _params(vrt, light=LIGHT):
    p = vrt.rtapi.default_shade_params()
    p.light_pos[:] = light
    return p


def _frames_equal_oracle(vrt, po, sc, ds, sizes=SIZES, light=LIGHT, occlusion=True):
    """plain and shadow frames of every size: hit records, occlusion bits, pixels and ray counts against the oracle (gpu_render asserts a
    zero status word) -> the oracle's 64 x 64 hit records (the last 64 x 64 frame compared).  The shadow frame is the one whose primary rays
    take the kernels with the shortcut; the plain frame runs the same tree through the kernels that keep the network."""
    pp = po.shade_params(light_pos=light)
    keep = None
    for w, h in sizes:
        for shadow in (0, 1):
            rpx, rhits, _, rn = po.render_ex(sc, w, h, pp, shadow)
            px, hn, _, n = gpu_render(vrt, ds, w, h, shadow=shadow, params=_params(vrt, light))
            assert np.array_equal(_bits(hn), _bits(rhits)), (sc.name, w, h, shadow)
            if shadow and not occlusion:
                continue                                 # (hit records and status only: see _deep_chain)
            if shadow:
                occ_ref, _ = _occlusion_oracle(po, sc, w, h, pp, rhits)
                np.testing.assert_array_equal(gpu_render.occluded, occ_ref)
            assert np.array_equal(px, rpx), (sc.name, w, h, shadow)
            assert n == rn
            if (w, h) == (64, 64):
                keep = rhits
    return keep


def _child_counts(vrt, ds, w, h, shadow):
    """the counting build's classes of node-body runs for one frame: [0..3] ordered arm with at most 0, 1, 2, >= 3 valid children,
    [4..7] occlusion arm"""
    import torch
    L = vrt.rtapi._lib()
    fn = L.vxrt_debug_child_counts
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.c_int, C.c_void_p]
    L.vxrt_render_wave_log.restype = C.c_int
    L.vxrt_render_wave_log.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vrt.rtapi.ShadeParams), C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    dev = ds.device
    px = torch.zeros((h, w), dtype=torch.int32, device=dev)
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    log = torch.zeros((4 * 8 * 256, 16), dtype=torch.int64, device=dev)
    out = (C.c_ulonglong * 8)()
    p = _params(vrt)
    assert fn(None, 1, None) == 0
    assert L.vxrt_render_wave_log(ds.accel, w, h, 0, h, C.byref(p), shadow, px.data_ptr(), cnt.data_ptr(), log.data_ptr(), None) == 0
    assert fn(out, 1, None) == 0
    assert vrt.rtapi.status(None) == 0
    assert sum(out) == int(log[:, 4].sum().item())       # every node-body run of the log is classed once
    return [int(v) for v in out]


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def _half(x, y0, y1, z0, z1, upper=False):
    """one triangle in the plane x = const over half of the rectangle (y0..y1) x (z0..z1): its box is the whole rectangle"""
    if upper:
        return [x, y0, z0, x, y1, z1, x, y0, z1]
    return [x, y0, z0, x, y1, z0, x, y1, z1]


def _behind(tris):
    """a triangle behind the camera: a child no camera ray finds valid"""
    k = len(tris)
    tris.append([-100.0, 90.0 + k, -10.0, -100.0, 110.0 + k, -10.0, -100.0, 110.0 + k, 10.0])
    return k


def _add(tris, t):
    tris.append(t)
    return len(tris) - 1


def one_child_scene(vrt):
    """Every node holds children whose boxes are disjoint rectangles of the plane x = 400, so a camera ray enters at most one of them at
    every node step; an occlusion ray starts in front of that plane and enters none.  Three levels in one quadrant, two in the others."""
    tris = []

    def grid(y0, y1, z0, z1, depth):
        if depth == 0:
            return _add(tris, _half(400.0, y0, y1, z0, z1, upper=len(tris) % 2 == 1))
        ym, zm, gy, gz = (y0 + y1) / 2, (z0 + z1) / 2, (y1 - y0) * 0.04, (z1 - z0) * 0.04
        return [grid(y0, ym - gy, z0, zm - gz, depth - 1), grid(y0, ym - gy, zm + gz, z1, depth - 1),
                grid(ym + gy, y1, z0, zm - gz, depth - 1), grid(ym + gy, y1, zm + gz, z1, depth - 1)]

    root = [grid(-350.0, 90.0, -420.0, -10.0, 2), grid(-350.0, 90.0, 10.0, 420.0, 1),
            grid(110.0, 550.0, -420.0, -10.0, 1), grid(110.0, 550.0, 10.0, 420.0, 1)]
    return _tree_scene(vrt, root, tris, "one_child")


PAIRS = [(i, j) for i in range(4) for j in range(i + 1, 4)]
KINDS = ("lower_slot_nearer", "higher_slot_nearer", "equal_distance")


def pair_scene(vrt, i, j, kind):
    """One node of four leaves: slots i < j face the camera with overlapping boxes, the two others lie behind it.  equal_distance: the
    two triangles are the SAME triangle, so their quantised boxes and their hit distances are identical -- the first one visited keeps the
    hit (strict '<'), and the reference visits the higher slot first."""
    tris, kids = [], [None] * 4
    for k in range(4):
        if k not in (i, j):
            kids[k] = _behind(tris)
    if kind == "equal_distance":
        kids[i] = _add(tris, _half(400.0, -200.0, 400.0, -300.0, 300.0))
        kids[j] = _add(tris, _half(400.0, -200.0, 400.0, -300.0, 300.0))
    else:
        x_lo, x_hi = (380.0, 400.0) if kind == "lower_slot_nearer" else (400.0, 380.0)
        kids[i] = _add(tris, _half(x_lo, -200.0, 400.0, -300.0, 300.0, upper=x_lo > x_hi))
        kids[j] = _add(tris, _half(x_hi, -250.0, 350.0, -250.0, 350.0, upper=x_hi > x_lo))
    return _tree_scene(vrt, kids, tris, "pair_%d%d_%s" % (i, j, kind)), kids


def three_forms_scene(vrt):
    """A chain a tile descends in step: the root has one valid child (path A), the next node two (the network with one entry pushed), the
    next one two valid children for every pixel and a third and a fourth whose boxes cover only part of a tile (the network, for lanes
    with two, three and four valid children in the same run)."""
    tris = []
    n2 = [_add(tris, _half(380.0, -400.0, 600.0, -500.0, 500.0)), _add(tris, _half(390.0, -400.0, 600.0, -500.0, 500.0, upper=True)),
          _add(tris, _half(385.0, -400.0, 600.0, -150.0, 500.0)), _add(tris, _half(395.0, -50.0, 600.0, -500.0, 500.0, upper=True))]
    n1 = [_behind(tris), n2, _behind(tris), _add(tris, _half(430.0, -400.0, 600.0, -500.0, 500.0))]
    root = [n1, _behind(tris), _behind(tris), _behind(tris)]
    return _tree_scene(vrt, root, tris, "three_forms")


def shrinking_scene(vrt):
    """Two-child nodes whose far children wait on the stack while the hit distance shrinks and one-child steps run: root [X, Y], X = [x1 at 300, x2 at 400],
    Y = [y1 at 350, y2 at 450], the boxes of X (300..400) and Y (350..450) overlap in depth.  A ray that hits x1 drops x2 and Y when they
    are popped (their maxima 400 and 350 are not below 300); one that misses x1 and hits x2 still enters Y (350 < 400), finds y1 its only
    valid child and may shrink to 350; one that misses both takes Y with both children."""
    tris = []
    x = [_add(tris, _half(300.0, -200.0, 400.0, -300.0, 300.0)), _add(tris, _half(400.0, -200.0, 400.0, -300.0, 100.0, upper=True))]
    y = [_add(tris, _half(350.0, -100.0, 400.0, -100.0, 300.0)), _add(tris, _half(450.0, -300.0, 500.0, -400.0, 400.0, upper=True))]
    return _tree_scene(vrt, [x, y], tris, "shrinking"), x + y


def _scenes_for_every_form(vrt):
    yield one_child_scene(vrt)
    for (i, j), kind in (((0, 1), KINDS[0]), ((1, 3), KINDS[1]), ((0, 3), KINDS[2]), ((2, 3), KINDS[2])):
        yield pair_scene(vrt, i, j, kind)[0]
    yield three_forms_scene(vrt)
    yield shrinking_scene(vrt)[0]
    tris = []
    yield _tree_scene(vrt, _chain((3, 3, 1, 0, 1), tris), tris, "chain_33101")
    yield vrt.scene.procedural("atrium", 5, 0, 3)        # (a built tree: leaves of two triangles, the abandon rule inside a leaf)


def _deep_scenes(vrt):
    """the stack filled to the last height at which a step passes, then a one-child and a two-child step"""
    P = _stack_cap() - 3
    yield _deep_chain(vrt, _levels(P), True, "full_one")
    yield _deep_chain(vrt, _levels(P) + (1,), False, "full_two")


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_tree_of_one_child_steps_takes_path_a_alone(vrt, po, gpu_device):
    sc = one_child_scene(vrt)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    rhits = _frames_equal_oracle(vrt, po, sc, ds)
    hit = rhits["dist"].reshape(-1) < 1e29
    assert hit.sum() >= 256 and (~hit).sum() >= 256       # half of every rectangle is triangle
    assert len(np.unique(rhits["triIdx"].reshape(-1)[hit])) >= 16
    for shadow in (0, 1):
        cc = _child_counts(vrt, ds, 64, 64, shadow)
        assert cc[1] > 0 and cc[2] == 0 and cc[3] == 0 and cc[6] == 0 and cc[7] == 0, cc
    ds.close()


@pytest.mark.parametrize("kind", KINDS)
def test_two_valid_children_in_each_of_the_six_slot_pairs(vrt, po, gpu_device, kind):
    for i, j in PAIRS:
        sc, kids = pair_scene(vrt, i, j, kind)
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        rhits = _frames_equal_oracle(vrt, po, sc, ds)
        hit = rhits["dist"].reshape(-1) < 1e29
        got = set(np.unique(rhits["triIdx"].reshape(-1)[hit]).tolist())
        if kind == "equal_distance":
            assert got == {kids[j]}, (i, j, got)         # the higher slot is visited first and keeps the hit
        else:
            assert got == {kids[i], kids[j]}, (i, j, got)   # the nearer triangle where it covers the pixel, the farther one beside it
        cc = _child_counts(vrt, ds, 64, 64, 0)
        assert cc[2] > 0 and cc[3] == 0, cc
        ds.close()


def test_one_wavefront_takes_all_three_forms_within_one_frame(vrt, po, gpu_device):
    sc = three_forms_scene(vrt)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    rhits = _frames_equal_oracle(vrt, po, sc, ds)
    hit = rhits["dist"].reshape(-1) < 1e29
    assert len(np.unique(rhits["triIdx"].reshape(-1)[hit])) >= 3   # the two nearest halves and the third child in front of one of them
    for w, h in ((16, 16), (64, 64)):
        cc = _child_counts(vrt, ds, w, h, 0)
        assert cc[1] > 0 and cc[2] > 0 and cc[3] > 0, cc
    ds.close()


def test_pushed_entries_wait_while_one_child_steps_run_and_the_hit_distance_shrinks(vrt, po, gpu_device):
    sc, (x1, x2, y1, y2) = shrinking_scene(vrt)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    rhits = _frames_equal_oracle(vrt, po, sc, ds)
    tri, hit = rhits["triIdx"].reshape(-1), rhits["dist"].reshape(-1) < 1e29
    for t in (x1, x2, y1, y2):                           # every outcome occurs: dropped entries, a shrinking hit, both children of Y
        assert (tri[hit] == t).sum() >= 16, (t, np.unique(tri[hit], return_counts=True))
    cc = _child_counts(vrt, ds, 64, 64, 0)
    assert cc[1] > 0 and cc[2] > 0 and cc[3] == 0, cc
    ds.close()


# The full-size stacks hold STACK_CAP = LSTK + 96 entries (LSTK levels in LDS: 6 in the 7-wavefront frame kernels, 5 in the 8-wavefront
# ones, one less each in the variant library, whose flags are build.py's TEST_VARIANT_FLAGS); with P entries pending a lane's sp is
# P - 1, and a step that holds a valid child reports the overflow when sp + 4 > STACK_CAP, whether it pushes or not.  Levels of three
# siblings are four-child steps (the network); P = STACK_CAP - 3 pending entries are the last height at which a step passes.
def _stack_cap():
    lstk = (5 if os.environ.get("VXRT_PACKED") == "1" else 6) - (1 if os.environ.get("VXRT_LIB_DIR") else 0)
    return lstk + 96


def _levels(P):
    return (3,) * (P // 3) + ((P % 3,) if P % 3 else ())


def _deep_chain(vrt, sib, one_child_tail, name):
    """test_gpu_stack_push's chain; one_child_tail: the deepest leaf becomes a node of that leaf and a triangle behind the camera, whose
    step holds one valid child for every ray.  These chains are deeper than the 32 levels the reference's trail holds, so its any-hit
    traversal, which decides the occlusion bits of a shadow frame, is no yardstick for them (the parent commit's library gives this
    library's bits): their shadow frames are compared in the hit records, which the primary rays decide, and the status word."""
    tris = []
    root = _chain(sib, tris)
    if one_child_tail:
        node = root
        while not isinstance(node[0], int):
            node = node[0]
        node[0] = [node[0], _behind(tris)]
    return _tree_scene(vrt, root, tris, name)


@pytest.mark.parametrize("one", [True, False])
def test_a_stack_filled_to_the_last_slot_then_a_one_or_two_child_step(vrt, po, gpu_device, one):
    """... then a step with one valid child (path A) or two (the network, one entry pushed): a correct frame, no overflow."""
    P = _stack_cap() - 3
    sc = _deep_chain(vrt, _levels(P) + (() if one else (1,)), one, "full_%d_%d" % (P, one))
    _, st = po.trace_canonical(sc, po.camera_rays(64, 64))
    assert st["max_stack"] == P + (0 if one else 1)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    if os.environ.get("VXRT_SHALLOW") != "0":
        assert vrt.rtapi.accel_info(ds.accel, 1) == 0    # full-size stacks
    _frames_equal_oracle(vrt, po, sc, ds, sizes=((64, 64),), occlusion=False)
    ds.close()


@pytest.mark.parametrize("one", [True, False])
def test_the_overflow_is_reported_by_a_step_that_pushes_little_or_nothing(vrt, po, gpu_device, one):
    """One entry more: P = STACK_CAP - 2 pending, sp = STACK_CAP - 3.  The next step holds one valid child and pushes nothing (path A),
    or two: sp + 4 > STACK_CAP, so it sets STATUS_STACK_OVERFLOW as the step with the network does, and nothing else.  The chains one
    entry shorter are the cases of the test above."""
    import torch
    P = _stack_cap() - 2
    sc = _deep_chain(vrt, _levels(P) + (() if one else (1,)), one, "over_%d_%d" % (P, one))
    _, st = po.trace_canonical(sc, po.camera_rays(64, 64))
    assert st["max_stack"] == P + (0 if one else 1)      # (the stack itself would hold it: the test in front of the step is what reports)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    s = torch.cuda.current_stream().cuda_stream
    for shadow in (0, 1):
        px = torch.zeros((64, 64), dtype=torch.int32, device=gpu_device)
        vrt.rtapi.render(ds.accel, 64, 64, 0, 64, _params(vrt), px.data_ptr(), shadow, None, None, None, s)
        assert vrt.rtapi.status(s) == STATUS_STACK_OVERFLOW, (P, one, shadow)
        assert vrt.rtapi.status(s) == 0                  # read-and-clear
    ds.close()
    tris = []
    ok = _tree_scene(vrt, _chain((3, 1, 0), tris), tris, "short")   # the next scene on the device is unaffected
    d2 = vrt.tracer.DeviceScene(ok, gpu_device)
    _frames_equal_oracle(vrt, po, ok, d2, sizes=((13, 7),))
    d2.close()


def test_every_scene_under_a_translated_root_instance(vrt, po, gpu_device):
    """The same trees under an instance whose record is a translation: the general kernels (TLAS level and instance step inside the loop)."""
    for sc in _scenes_for_every_form(vrt):
        s2 = _translated(vrt, sc)
        ds = vrt.tracer.DeviceScene(s2, gpu_device)
        assert vrt.rtapi.accel_info(ds.accel, 5) == 0    # no identity-root kernels
        _frames_equal_oracle(vrt, po, s2, ds)
        ds.close()
    for sc in _deep_scenes(vrt):
        s2 = _translated(vrt, sc)
        ds = vrt.tracer.DeviceScene(s2, gpu_device)
        _frames_equal_oracle(vrt, po, s2, ds, sizes=((64, 64),), occlusion=False)
        ds.close()


def test_every_scene_through_the_callers_camera(vrt, po, gpu_device):
    import torch
    import camera_ref as cr
    from test_gpu_camera import _check, _host_frame, _render_camera
    eyes = ((0.0, 100.0, 0.0), (20.0, 120.0, 15.0))
    for sc in _scenes_for_every_form(vrt):
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        for w, h in ((16, 16), (64, 64)):
            for eye in eyes:
                cam = np.array(eye + (1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0), np.float32)
                for shadow in (0, 1):
                    got = _host_frame(*_render_camera(vrt, ds, cam, w, h, _params(vrt), shadow), w, h, 0, h)
                    assert vrt.rtapi.status(torch.cuda.current_stream().cuda_stream) == 0
                    _check(got, cr.frame(sc, cam, w, h, po.shade_params(light_pos=LIGHT), shadow), "%s eye %r shadow=%d" % (sc.name, eye, shadow))
        ds.close()
    w, h = 64, 64
    cam = np.array(eyes[0] + (1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0), np.float32)
    for sc in _deep_scenes(vrt):                         # (shadow frames in their hit records and the status word: see _deep_chain)
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        _, hits, _, _ = _host_frame(*_render_camera(vrt, ds, cam, w, h, _params(vrt), 1), w, h, 0, h)
        assert vrt.rtapi.status(torch.cuda.current_stream().cuda_stream) == 0
        _, rhits, _, _ = cr.frame(sc, cam, w, h, po.shade_params(light_pos=LIGHT), 0)
        for k in ("dist", "bx", "by", "bz", "triIdx"):
            np.testing.assert_array_equal(hits[k].view(np.uint32), rhits[k].view(np.uint32), err_msg="%s: hits.%s" % (sc.name, k))
        np.testing.assert_array_equal(hits["blasIdx"] & 0x7FFFFFFF, rhits["blasIdx"] & 0x7FFFFFFF)
        assert (rhits["dist"] < 1e29).any()
        ds.close()


def test_a_set_of_two_frames_with_different_lights_equals_the_frames_one_by_one(vrt, po, gpu_device):
    import torch
    w, h = 64, 64
    lights = (LIGHT, (30.0, 160.0, -60.0))
    plist = [_params(vrt, lp) for lp in lights]
    s = torch.cuda.current_stream().cuda_stream
    for sc in (three_forms_scene(vrt), shrinking_scene(vrt)[0]):
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        buf = torch.zeros((2, h, w), dtype=torch.int32, device=gpu_device)
        vrt.rtapi.render_batch(ds.accel, w, h, plist, buf.data_ptr(), w * h, 1, None, s)
        assert vrt.rtapi.status(s) == 0
        got = buf.cpu().numpy().view(np.uint32)
        for i, lp in enumerate(lights):
            one, _, _, _ = gpu_render(vrt, ds, w, h, shadow=1, params=plist[i])
            rpx, _, _, _ = po.render_ex(sc, w, h, po.shade_params(light_pos=lp), 1)
            assert np.array_equal(one, rpx), (sc.name, i)
            assert np.array_equal(got[i], one), (sc.name, i)
        ds.close()


def _rerun(extra_env):
    env = dict(os.environ, **extra_env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "not child_process"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (extra_env, r.stdout[-3000:] + r.stderr[-2000:])
    assert " passed" in r.stdout


def test_child_process_the_eight_wavefront_kernels(vrt, gpu_device):
    """VXRT_PACKED=1 (read once per process) forces the 8-wavefront instantiations, which the benchmark's sets of frames run."""
    if os.environ.get("VXRT_PACKED") != "1":
        _rerun({"VXRT_PACKED": "1"})


def test_child_process_the_general_kernels(vrt, gpu_device):
    """VXRT_IDENT_ROOT=0: identity scenes take the general kernels too, with 7 and with 8 wavefronts."""
    if os.environ.get("VXRT_IDENT_ROOT") != "0":
        _rerun({"VXRT_IDENT_ROOT": "0"})
        _rerun({"VXRT_IDENT_ROOT": "0", "VXRT_PACKED": "1"})


def test_child_process_the_variant_library_checks_every_skipped_step_against_the_network(vrt, gpu_device):
    """The variant library (build.py: TEST_VARIANT_FLAGS, -DRT_ORDER_CHECK=1) evaluates the network beside every step that path A takes
    and sets STATUS_ITER_LIMIT on a difference; every comparison above asserts a zero status word."""
    if os.environ.get("VXRT_LIB_DIR"):
        return
    bld = importlib.import_module("vortex-raytracing_amd.build")
    d = bld.build_test_variant()                         # (built by __graft_entry__.build(); rebuilt here only if a source is newer)
    _rerun({"VXRT_LIB_DIR": d})
    _rerun({"VXRT_LIB_DIR": d, "VXRT_PACKED": "1"})
