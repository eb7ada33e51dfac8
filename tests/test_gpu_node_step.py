"""GPU: the node step of the frame kernels -- the box tests' validity masks handed to the occlusion arm (csrc/rt_kernels.hip:
RT_OCC_OK_MASKS) and the pushes that follow -- against the oracle on the same inputs: hit records bit-equal and packed RGB8 equal, with
and without shadow rays.

  * the occlusion arm takes the validity of the children from the box tests and pushes raw slab distances: nodes with empty slots in
    every position, children an occlusion ray misses, children beyond the light and children behind the ray's origin;
  * the pushing step at every stack height from 0 to LSTK + 1 with 1, 2 and 3 entries, with an empty and an occupied register top,
    and one tree whose ray pushes low in the stack, pops back to an empty stack and pushes three entries through the same slots
    (written for a push without store predicates low in the LDS part, which lost its A/B -- DESIGN.md s5 -- and kept: they hold
    whatever form the push takes);
  * stacks filled to the last entry of their depth class stay silent and equal the oracle, deeper ones report the overflow bit and
    nothing else.

Every case runs in the 7-wavefront kernels (6 LDS levels) here and, through a child process that forces them for small frames, in the
8-wavefront ones (5 LDS levels) -- one frame at a time and as batches on two streams with a light per frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import _bits, gpu_render
from test_gpu_stack_push import SIZES, _frame_equals_oracle, _params, _tree_scene, chain_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTKS = (6, 5)
# levels that leave P entries pending in front of the last level's step: the top is occupied and sp = P - 1 (P >= 1), or nothing is
# pending at all (P = 0: sp = 0 and the register top empty -- the only height at which it can be)
PREFIX = {0: (), 1: (1,), 2: (2,), 3: (3,), 4: (3, 1), 5: (3, 2), 6: (3, 3), 7: (3, 3, 1), 8: (3, 3, 2)}
HEIGHT_CASES = [(P, s) for P in sorted(PREFIX) for s in (1, 2, 3)]


def test_the_height_cases_cover_every_sp_up_to_the_scratch_part():
    """(no GPU work: the case table itself)  sp = 0 .. LSTK + 1 for both kernels with 1, 2 and 3 entries pushed, sp = 0 with an empty and
    with an occupied top, and heights on both sides of `sp + 2 < LSTK` (a push that cannot leave LDS whatever it pushes)."""
    for lstk in LSTKS:
        for sp in range(0, lstk + 2):
            for s in (1, 2, 3):
                assert (sp + 1, s) in HEIGHT_CASES
        low = {max(P - 1, 0) + 2 < lstk for P, _ in HEIGHT_CASES}
        assert low == {True, False}
    assert all((0, s) in HEIGHT_CASES and (1, s) in HEIGHT_CASES for s in (1, 2, 3))


@pytest.mark.parametrize("P,s", HEIGHT_CASES)
def test_a_push_of_s_entries_at_every_height(vrt, po, gpu_device, P, s):
    sc = chain_tree(vrt, PREFIX[P] + (s,))
    _, st = po.trace_canonical(sc, po.camera_rays(64, 64))
    assert st["max_stack"] == P + s
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    hit = False
    for w, h in ((17, 9), (64, 64)):
        for shadow in (0, 1):
            hit |= bool((_frame_equals_oracle(vrt, po, sc, ds, w, h, shadow)["dist"] < 1e29).any())
    assert hit
    ds.close()


def _tri(tris, x, s, zc=0.0, flip=False):
    """a triangle facing the fixed camera ((0, 100, 0), looking along +x) at depth x: it covers the low-z side of its box, or the high-z
    side when flipped"""
    z0, z1 = (zc + s, zc - s) if flip else (zc - s, zc + s)
    tris.append([x, 100.0 - s, z0, x, 100.0 + s, z0, x, 100.0 + 0.4 * s, z1])
    return len(tris) - 1


def test_slots_that_held_garbage_receive_real_entries_and_are_popped(vrt, po, gpu_device):
    """Under one root, a near subtree A and a far subtree B of the same outline.  A ray enters A first with B pending (sp = 0, top
    occupied): A's step pushes ONE entry (a push without store predicates also writes slots 1 and 2 there), A's next level one more.  A's
    triangles cover the low-z side of the outline, B's the other: a ray on the high-z side misses everything in A, pops back to an
    empty stack, and B's two levels then push three entries each through slots 0 .. 4, which are popped one by one."""
    tris = []
    a = [[_tri(tris, 300.0, 100.0), _tri(tris, 303.0, 99.0)], _tri(tris, 306.0, 98.0)]
    b2 = [_tri(tris, 380.0, 100.0, flip=True)] + [_tri(tris, 383.0 + 3.0 * j, 99.0 - j, flip=True) for j in range(3)]
    b = [b2] + [_tri(tris, 395.0 + 3.0 * j, 95.0 - j, flip=True) for j in range(3)]
    n_a = 3
    sc = _tree_scene(vrt, [a, b], tris, "garbage_slots")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    for w, h in SIZES:
        for shadow in (0, 1):
            rh = _frame_equals_oracle(vrt, po, sc, ds, w, h, shadow)
    found = rh["dist"] < 1e29                                    # (64 x 64)
    assert (found & (rh["triIdx"] < n_a)).sum() >= 16 and (found & (rh["triIdx"] >= n_a)).sum() >= 16
    _, st = po.trace_canonical(sc, po.camera_rays(64, 64))
    assert st["max_stack"] == 6
    ds.close()


@pytest.mark.parametrize("last", [1, 2, 3])
def test_stacks_filled_to_the_last_entry_of_each_depth_class_stay_silent(vrt, po, gpu_device, last):
    """48 entries in the 16-level class and 96 in the full-size one (the reference's own limit, the deepest the oracle walks), the last
    step pushing 1, 2 or 3 of them from the scratch part: frames equal the oracle's, status 0 (gpu_render asserts it)."""
    for levels, shallow in ((16, 1), (32, 0)):
        sib = (3,) * (levels - 1) + (last,)
        sc = chain_tree(vrt, sib)
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        if os.environ.get("VXRT_SHALLOW") != "0":
            assert vrt.rtapi.accel_info(ds.accel, 1) == shallow
        _, st = po.trace_canonical(sc, po.camera_rays(64, 64))
        assert st["max_stack"] == 3 * (levels - 1) + last
        for shadow in (0, 1):
            _frame_equals_oracle(vrt, po, sc, ds, 64, 64, shadow)
        ds.close()


def test_the_first_step_that_does_not_fit_reports_the_overflow_and_nothing_else(vrt, po, gpu_device):
    """The full-size stacks hold LSTK + 96 entries below the register top and a step is refused when sp + 4 exceeds that -- always with
    sp in the scratch part: a push that ends in LDS, or straddles the boundary, starts below LSTK, and LSTK + 4 <= capacity.  35 levels
    of three siblings reach sp = 101 in front of the last step, past both kernels' bound."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    for lstk in LSTKS:
        assert 3 * 34 - 1 + 4 > lstk + 96 >= lstk + 4
    sc = chain_tree(vrt, (3,) * 35)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    assert vrt.rtapi.accel_info(ds.accel, 1) == 0
    for shadow in (0, 1):
        px = torch.zeros((64, 64), dtype=torch.int32, device=gpu_device)
        vrt.rtapi.render(ds.accel, 64, 64, 0, 64, _params(vrt), px.data_ptr(), shadow, None, None, None, s)
        assert vrt.rtapi.status(s) == 1, shadow     # STATUS_STACK_OVERFLOW alone
        assert vrt.rtapi.status(s) == 0             # read-and-clear
    ds.close()
    ok = chain_tree(vrt, (3, 3, 2))                 # the next scene on the device is unaffected
    d2 = vrt.tracer.DeviceScene(ok, gpu_device)
    _frame_equals_oracle(vrt, po, ok, d2, 17, 9, 1)
    d2.close()


def _layers(vrt, keep, name):
    """Root with four children, each a node over two leaves, at four depths (nearest in slot 3); the root's slots not in `keep` are
    emptied (meta byte 0: the slot keeps its planes, so its box test still passes -- only the descriptor says there is no child).  The
    layers sit side by side in z with an overlap, alternate between the two triangle orientations and shrink with depth."""
    tris, kids = [], []
    for k in range(4):
        x, zc = 400.0 - 30.0 * k, -90.0 + 60.0 * k
        kids.append([_tri(tris, x, 80.0 - 5.0 * k, zc, flip=bool(k & 1)), _tri(tris, x + 4.0, 70.0 - 5.0 * k, zc + 10.0, flip=not (k & 1))])
    sc = _tree_scene(vrt, kids, tris, name)
    bufs = {kk: np.frombuffer(bytes(v), np.uint8).copy() for kk, v in sc.buffers.items()}
    for k in range(4):
        if k not in keep:
            bufs["bvh"][24 + 7 * k] = 0
    return vrt.scene.Scene(bufs, name=name)


# the light in front of every layer (occlusion rays run back through the nearer layers: boxes they cross and miss, boxes behind
# their origin), between the layers (children beyond the light: past tmax) and behind them all
LIGHTS = ((-50.0, 180.0, 40.0), (355.0, 110.0, 10.0), (600.0, 60.0, -80.0))
KEEPS = [tuple(k for k in range(4) if k != e) for e in range(4)] + [(k,) for k in range(4)] + [(0, 1, 2, 3), (0, 3), (1, 2)]


@pytest.mark.parametrize("keep", KEEPS, ids=lambda k: "".join(map(str, k)))
def test_empty_slots_in_every_position_under_three_lights(vrt, po, gpu_device, keep):
    sc = _layers(vrt, keep, "layers_" + "".join(map(str, keep)))
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    lit = shaded = 0
    for light in LIGHTS:
        p = vrt.rtapi.default_shade_params()
        p.light_pos[:] = light
        for w, h in ((17, 9), (64, 64)):
            for shadow in (0, 1):
                rpx, rhits, _, _ = po.render_ex(sc, w, h, po.shade_params(light_pos=light), shadow)
                px, hn, _, _ = gpu_render(vrt, ds, w, h, shadow=shadow, params=p)
                assert np.array_equal(_bits(hn), _bits(rhits)), (keep, light, w, h, shadow)
                assert np.array_equal(px, rpx), (keep, light, w, h, shadow)
        found = rhits["dist"] < 1e29                             # (64 x 64 with shadow rays)
        assert found.any() and not found.all()                   # hits and misses share the tiles
        shaded += int((gpu_render.occluded & found).sum())
        lit += int((~gpu_render.occluded & found).sum())
    assert lit > 0 and (shaded > 0 or len(keep) == 1)            # occlusion rays that end blocked and ones that reach the light
    ds.close()


def test_batches_on_two_streams_with_a_light_per_frame(vrt, po, gpu_device):
    """Two sets of three frames, one per stream (two frame contexts), each frame under its own light: every frame equals the oracle's."""
    import torch
    sc = _layers(vrt, (0, 1, 2, 3), "layers_batch")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    w, h = 64, 64
    lights = LIGHTS + ((30.0, 160.0, -60.0), (-10.0, 220.0, 90.0), (340.0, 100.0, 0.0))
    plist = []
    for lp in lights:
        p = vrt.rtapi.default_shade_params()
        p.light_pos[:] = lp
        plist.append(p)
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    streams = [torch.cuda.Stream(device=gpu_device) for _ in range(2)]
    bufs = [torch.zeros((3, h, w), dtype=torch.int32, device=gpu_device) for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        vrt.rtapi.render_batch(ds.accel, w, h, plist[3 * i: 3 * i + 3], bufs[i].data_ptr(), w * h, 1, None, streams[i].cuda_stream)
    torch.cuda.synchronize()
    for st in streams:
        assert vrt.rtapi.status(st.cuda_stream) == 0
    for i, lp in enumerate(lights):
        rpx, _, _, _ = po.render_ex(sc, w, h, po.shade_params(light_pos=lp), 1)
        assert np.array_equal(bufs[i // 3][i % 3].cpu().numpy().view(np.uint32), rpx), i
    vrt.rtapi.accel_frames_in_flight(ds.accel, 1)
    ds.close()


def test_the_eight_wavefront_kernels_pass_the_same_cases(vrt, gpu_device):
    """The 8-wavefront instantiations (5 LDS levels) are what frames in overlapping sets run; small frames take them only when forced
    (VXRT_PACKED=1), which is read once per process: a child process runs this file's other tests with it."""
    if os.environ.get("VXRT_PACKED") == "1":
        return
    env = dict(os.environ, VXRT_PACKED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "not eight_wavefront"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
