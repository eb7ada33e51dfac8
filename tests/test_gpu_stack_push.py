"""GPU: the traversal stack of the frame kernels -- pending children pushed in one operation per node step, the register top refilled
once per pop, the identity-root instantiations -- against the oracle on the same inputs (hit records bit-exact, packed RGB8 equal).

The stack keeps LSTK levels per lane in LDS (6 in the 7-wavefront frame kernels, 5 in the 8-wavefront ones) and the rest in scratch.  A
lane holds its newest pending entry in registers (the register top) and the others in memory slots 0 .. sp - 1, so with P entries pending
(what the oracle counts: its max_stack is the largest P of a ray) the kernel's sp is P - 1 and the top is occupied; the top is empty only
while nothing is pending (sp = 0: start_ray, and pop_next refills it whenever sp > 0), so "top empty" exists at sp = 0 alone.  A step
that pushes s entries at height sp writes slots sp .. sp + s - 1 (the old top, then all pushed entries but the last) and ends at sp + s:
all in LDS if sp + s <= LSTK, all in scratch if sp >= LSTK, entry by entry otherwise.

chain_tree builds the trees by hand: level i has one chain child and sib[i] single-triangle leaves, DEEPER = NEARER (as
scenes.chain_bvh4), so a ray through the middle of the frame descends the chain first at every level and leaves sib[i] entries pending:
before the last level's step sum(sib[:-1]) entries are pending, and that step pushes sib[-1]."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import _bits, gpu_render

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHT = (-50.0, 180.0, 40.0)
SIZES = ((8, 8), (17, 9), (64, 64))


def torch_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _params(vrt):
    p = vrt.rtapi.default_shade_params()
    p.light_pos[:] = LIGHT
    return p


def _frame_equals_oracle(vrt, po, sc, ds, w, h, shadow):
    rpx, rhits, _, _ = po.render_ex(sc, w, h, po.shade_params(light_pos=LIGHT), shadow)
    px, hn, _, _ = gpu_render(vrt, ds, w, h, shadow=shadow, params=_params(vrt))
    assert np.array_equal(_bits(hn), _bits(rhits)), (w, h, shadow)
    assert np.array_equal(px, rpx), (w, h, shadow)
    return rhits


def _tree_scene(vrt, root, tris, name):
    """A BVH4 in the RTU test's formats under the identity instance of the cornell scene.  root: nested lists, a child is a list (an
    internal node, at most four children) or an int (a leaf holding that one triangle).  A node's children lie next to each other behind
    their parent; quantisation as in scenes.chain_bvh4 (origin + ldexp(q, e), floor / ceil: conservative)."""
    base = vrt.scene.procedural("cornell")
    tris = np.asarray(tris, np.float32)
    lo_t, hi_t = tris.reshape(-1, 3, 3).min(1), tris.reshape(-1, 3, 3).max(1)

    def box(c):
        if isinstance(c, int):
            return lo_t[c], hi_t[c]
        bs = [box(x) for x in c]
        return np.min([b[0] for b in bs], 0), np.max([b[1] for b in bs], 0)

    def count(c):
        return 1 if isinstance(c, int) else 1 + sum(count(x) for x in c)

    nodes = np.zeros((count(root), 52), np.uint8)
    todo, free = [(0, root)], 1
    while todo:
        idx, kids = todo.pop(0)
        assert 1 <= len(kids) <= 4
        first, free = free, free + len(kids)
        boxes = [box(c) for c in kids]
        lo = np.min([b[0] for b in boxes], 0).astype(np.float32)
        hi = np.max([b[1] for b in boxes], 0).astype(np.float32)
        e = np.ceil(np.log2(np.maximum(hi.astype(np.float64) - lo, 1e-6) / 255.0)).astype(np.int64)
        n = nodes[idx]
        n[0:12] = lo.view(np.uint8)
        n[12:15] = e.astype(np.int8).view(np.uint8)
        n[16:20] = np.array([first], np.uint32).view(np.uint8)
        for c, (blo, bhi) in enumerate(boxes):
            n[24 + 7 * c] = 1
            n[25 + 7 * c: 28 + 7 * c] = np.clip(np.floor((blo.astype(np.float64) - lo) / np.exp2(e)), 0, 255).astype(np.uint8)
            n[28 + 7 * c: 31 + 7 * c] = np.clip(np.ceil((bhi.astype(np.float64) - lo) / np.exp2(e)), 0, 255).astype(np.uint8)
            if isinstance(kids[c], int):
                leaf = nodes[first + c]
                leaf[0:12] = lo_t[kids[c]].view(np.uint8)
                leaf[16:20] = np.array([kids[c]], np.uint32).view(np.uint8)
                leaf[20:24] = np.array([1], np.uint32).view(np.uint8)
            else:
                todo.append((first + c, kids[c]))
    ex = np.zeros((len(tris), 16), np.float32)
    ex[:, 0] = ex[:, 3] = ex[:, 6] = -1.0                # normals facing the camera; texId 0
    b = {kk: np.frombuffer(bytes(v), np.uint8).copy() for kk, v in base.buffers.items()}
    b["bvh"] = nodes.reshape(-1)
    b["tri"] = tris.view(np.uint8).reshape(-1)
    b["triEx"] = ex.view(np.uint8).reshape(-1)
    if "triIdx" in b:
        b["triIdx"] = np.arange(len(tris), dtype=np.uint32).view(np.uint8)
    assert b["blas"].size == 160 and b["blas"].view(np.uint32)[0] == 0 and b["tlas"].size == 52
    return vrt.scene.Scene(b, name=name)


def _chain(sib, tris, size=300.0, zc=0.0):
    """the nested lists of a chain with sib[i] sibling leaves at level i; its triangles are appended to tris (facing the fixed camera at
    (0,100,0) looking along +x, centred at z = zc, deeper = nearer and smaller)"""
    def tri(level, j):
        x = 420.0 - 5.0 * level - 1.25 * j
        s = size - 5.0 * level - 1.25 * j
        tris.append([x, 100.0 - s, zc - s, x, 100.0 + s, zc - s, x, 100.0 + 0.4 * s, zc + s])
        return len(tris) - 1
    node = tri(len(sib), 0)                              # the chain child of the last level: a leaf
    for level in range(len(sib) - 1, -1, -1):
        node = [node] + [tri(level, j) for j in range(sib[level])]
    return node


def chain_tree(vrt, sib):
    tris = []
    return _tree_scene(vrt, _chain(sib, tris), tris, "chain_tree_" + "".join(map(str, sib)))


LSTKS = (6, 5)                                           # 7-wavefront frame kernels, 8-wavefront (PACKED) ones
PREFIX = {0: (), 4: (3, 1), 5: (3, 2), 6: (3, 3), 7: (3, 3, 1), 8: (3, 3, 2)}   # levels that leave P entries pending
# P = 0: the register top empty (sp = 0).  P = 4 .. 8: the top occupied and sp = P - 1 = 3 .. 7, which is LSTK - 2 .. LSTK + 1 of both
# kernels (5: 3 .. 6, 6: 4 .. 7).  Each followed by a step that pushes 1, 2 and 3 entries.
BOUNDARY_CASES = [(P, s) for P in sorted(PREFIX) for s in (1, 2, 3)]


def _arm(lstk, P, s):
    sp = max(P - 1, 0)
    stored = s if P else s - 1                           # (no old top to store when nothing was pending)
    return "none" if stored == 0 else "lds" if sp + stored <= lstk else "scratch" if sp >= lstk else "straddle"


def test_the_boundary_cases_reach_every_arm_of_the_push_in_both_kernels():
    """(no GPU work: the case table itself)  For each LSTK: sp = LSTK - 2 .. LSTK + 1 with 1, 2 and 3 entries pushed, and every arm."""
    for lstk in LSTKS:
        for sp in range(lstk - 2, lstk + 2):
            for s in (1, 2, 3):
                assert (sp + 1, s) in BOUNDARY_CASES
        arms = {_arm(lstk, P, s) for P, s in BOUNDARY_CASES}
        assert arms == {"none", "lds", "scratch", "straddle"}, (lstk, arms)
    assert _arm(5, 5, 3) == "straddle" and _arm(6, 5, 3) == "straddle" and _arm(6, 6, 2) == "straddle" and _arm(5, 6, 1) == "scratch"


@pytest.mark.parametrize("P,s", BOUNDARY_CASES)
def test_a_step_that_pushes_s_entries_with_P_pending(vrt, po, gpu_device, P, s):
    """The last level's step finds P entries pending (sp = P - 1 and the top occupied, or nothing at all) and pushes s: the oracle's
    deepest stack is exactly P + s, reached by the rays through the middle of the frame, and the frames equal the oracle's.  Run for
    LSTK = 6 here and for LSTK = 5 by test_the_eight_wavefront_kernels_pass_the_same_cases."""
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


# scenes.chain_bvh4: k levels of three siblings, the deepest stack is 3 k entries -- all in LDS (k = 1), up to the boundary (k = 2),
# across it (k = 3), far in scratch (k = 4, 7)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("shadow", [0, 1])
def test_chains_that_cross_the_lds_boundary_match_the_oracle(vrt, po, gpu_device, k, shadow):
    from scenes import chain_bvh4
    sc = chain_bvh4(vrt, k)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    _, st = po.trace_canonical(sc, po.camera_rays(64, 64))
    assert st["max_stack"] == 3 * k
    hit = False
    for w, h in SIZES:
        hit |= bool((_frame_equals_oracle(vrt, po, sc, ds, w, h, shadow)["dist"] < 1e29).any())
    assert hit
    ds.close()


@pytest.mark.parametrize("k,entries,shallow", [(16, 48, 1), (32, 96, 0)])
def test_depth_class_boundaries_fill_the_stack_exactly(vrt, po, gpu_device, k, entries, shallow):
    """16 levels need exactly the 48 entries of the shallow stacks, 32 levels the reference's 96: both frames equal the oracle's and no
    overflow is reported (gpu_render asserts a zero status)."""
    from scenes import chain_bvh4
    sc = chain_bvh4(vrt, k)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    if os.environ.get("VXRT_SHALLOW") != "0":
        assert vrt.rtapi.accel_info(ds.accel, 1) == shallow
    _, st = po.trace_canonical(sc, po.camera_rays(64, 64))
    assert st["max_stack"] == entries
    for shadow in (0, 1):
        _frame_equals_oracle(vrt, po, sc, ds, 64, 64, shadow)
    ds.close()


def test_thirty_six_levels_set_the_overflow_status_and_nothing_else(vrt, po, gpu_device):
    import torch
    from scenes import chain_bvh4
    sc = chain_bvh4(vrt, 36)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    s = torch.cuda.current_stream().cuda_stream
    for shadow in (0, 1):
        px = torch.zeros((64, 64), dtype=torch.int32, device=gpu_device)
        vrt.rtapi.render(ds.accel, 64, 64, 0, 64, _params(vrt), px.data_ptr(), shadow, None, None, None, s)
        assert vrt.rtapi.status(s) == 1, shadow     # STATUS_STACK_OVERFLOW alone
        assert vrt.rtapi.status(s) == 0             # read-and-clear
    ds.close()
    ok = chain_bvh4(vrt, 3)                          # the next scene on the device is unaffected
    d2 = vrt.tracer.DeviceScene(ok, gpu_device)
    _frame_equals_oracle(vrt, po, ok, d2, 17, 9, 1)
    d2.close()


def test_lanes_of_one_wavefront_on_both_sides_of_the_boundary(vrt, po, gpu_device):
    """An 8x8 frame is one tile, traced by one wavefront.  Under one root, a deep chain (three siblings per level) covers the tile's left
    half and a shallow one of as many levels (one sibling per level) its right half: lanes of the same wavefront take their node steps
    level by level together, the left ones with up to 9 entries pending (slots up to 7 = LSTK + 1 of the 7-wavefront kernel, scratch in
    both kernels), the right ones with at most 3 (LDS in both)."""
    tris = []
    deep, shallow = _chain((3, 3, 3), tris, 140.0, -150.0), _chain((1, 1, 1), tris, 140.0, 150.0)
    sc = _tree_scene(vrt, [deep, shallow], tris, "deep_and_shallow")
    rays = po.camera_rays(8, 8)
    depth = np.array([po.trace_canonical(sc, rays[i:i + 1])[1]["max_stack"] for i in range(len(rays))])
    slots = depth - 1                                    # memory slots in use at a ray's deepest point
    for lstk in LSTKS:
        assert (slots >= lstk + 1).sum() >= 4 and ((depth >= 1) & (slots < lstk)).sum() >= 4, depth
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    for w, h in ((8, 8), (17, 9)):
        for shadow in (0, 1):
            _frame_equals_oracle(vrt, po, sc, ds, w, h, shadow)
    ds.close()


def _translated(vrt, sc):
    bufs = dict(sc.buffers)
    blas = sc["blas"].copy().view(np.float32)
    blas[1 + 3] -= 7.0        # invTransform[0][3]
    blas[17 + 3] += 7.0       # transform[0][3]
    bufs["blas"] = blas.view(np.uint8)
    return vrt.scene.Scene(bufs)


def test_identity_root_kernels_are_taken_by_identity_scenes_only(vrt, po, golden, gpu_device):
    """One identity instance: the frame kernels without the TLAS level (vxrt_accel_info 5) -- unless a knob or the build switches them off,
    which this test follows.  The same triangles under a translated instance and the six-instance fixture keep the general kernels.
    All three render the oracle's frames; the identity scene's own rays outside the fast domain (the frame's middle row and column: a zero
    direction component) are handed to the EXACT launch and are part of the comparison."""
    sc = vrt.scene.procedural("cornell")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    assert vrt.rtapi.accel_info(ds.accel, 2) == (0 if os.environ.get("VXRT_IDENT_ROOT") == "0" else 1)
    want = vrt.rtapi.accel_info(ds.accel, 2) and vrt.rtapi.accel_info(ds.accel, 1) and not vrt.rtapi.accel_info(ds.accel, 3)
    taken = vrt.rtapi.accel_info(ds.accel, 5)
    if os.environ.get("VXRT_LIB_DIR"):
        assert taken in (0, int(bool(want)))         # (a variant library may be built without them)
    else:
        assert taken == int(bool(want))
    for w, h in SIZES:
        for shadow in (0, 1):
            _frame_equals_oracle(vrt, po, sc, ds, w, h, shadow)
    ds.close()
    s2 = _translated(vrt, sc)
    d2 = vrt.tracer.DeviceScene(s2, gpu_device)
    assert vrt.rtapi.accel_info(d2.accel, 2) == 0 and vrt.rtapi.accel_info(d2.accel, 5) == 0
    for shadow in (0, 1):
        _frame_equals_oracle(vrt, po, s2, d2, 64, 64, shadow)
    d2.close()
    g = golden("sphere_x6")
    d3 = vrt.tracer.DeviceScene(g, gpu_device)
    assert vrt.rtapi.accel_info(d3.accel, 2) == 0 and vrt.rtapi.accel_info(d3.accel, 5) == 0
    for w, h in ((17, 9), (64, 64)):
        for shadow in (0, 1):
            _frame_equals_oracle(vrt, po, g, d3, w, h, shadow)
    d3.close()


def test_the_shipped_library_has_the_identity_root_kernels(vrt, gpu_device):
    if os.environ.get("VXRT_LIB_DIR") or os.environ.get("VXRT_IDENT_ROOT") == "0" or os.environ.get("VXRT_SHALLOW") == "0":
        pytest.skip("a variant library or a measurement knob is set: nothing to say about the shipped default")
    sc = vrt.scene.procedural("cornell")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    assert vrt.rtapi.accel_info(ds.accel, 5) == 1
    ds.close()


def test_signed_zero_camera_positions_in_the_identity_root_kernels(vrt, po, gpu_device):
    """Camera frames (vxrt_render_camera) of the identity scene take the identity-root kernels, and every primary ray starts at the
    camera position.  With a -0 component there, start_ray enters the instance through the general step -- the one place an
    identity-root kernel runs it, and its second fast-domain check may hand the ray to the EXACT launch -- and the lane then lives in a
    loop without an instance step.  Frames against tests/camera_ref.py (the oracle's traversal), bit for bit; +0 as the control."""
    import camera_ref as cr
    from test_gpu_camera import _check, _host_frame, _render_camera
    sc = vrt.scene.procedural("cornell")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    if not (os.environ.get("VXRT_LIB_DIR") or os.environ.get("VXRT_IDENT_ROOT") == "0" or os.environ.get("VXRT_SHALLOW") == "0"):
        assert vrt.rtapi.accel_info(ds.accel, 5) == 1
    w, h = 64, 40
    p, pp = vrt.rtapi.default_shade_params(), po.shade_params()
    for eye in ((0.0, 100.0, 0.0), (-0.0, 100.0, -0.0), (-0.0, 100.0, 0.0), (0.0, 100.0, -0.0), (-0.0, 100.0, 30.0), (120.0, 60.0, -0.0)):
        cam = np.array(eye + (1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0), np.float32)
        assert [np.signbit(c) for c in cam[:3]] == [np.signbit(np.float32(c)) for c in eye]
        for shadow in (0, 1):
            got = _host_frame(*_render_camera(vrt, ds, cam, w, h, p, shadow), w, h, 0, h)
            assert vrt.rtapi.status(torch_stream()) == 0
            _check(got, cr.frame(sc, cam, w, h, pp, shadow), "eye %r shadow=%d" % (eye, shadow))
    ds.close()


def test_a_batch_of_three_frames_equals_the_frames_one_by_one(vrt, po, gpu_device):
    import torch
    from scenes import chain_bvh4
    sc = chain_bvh4(vrt, 4)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    w, h = 64, 64
    s = torch.cuda.current_stream().cuda_stream
    lights = ((-50.0, 180.0, 40.0), (30.0, 160.0, -60.0), (-10.0, 220.0, 90.0))
    plist = []
    for lp in lights:
        p = vrt.rtapi.default_shade_params()
        p.light_pos[:] = lp
        plist.append(p)
    buf = torch.zeros((3, h, w), dtype=torch.int32, device=gpu_device)
    vrt.rtapi.render_batch(ds.accel, w, h, plist, buf.data_ptr(), w * h, 1, None, s)
    assert vrt.rtapi.status(s) == 0
    got = buf.cpu().numpy().view(np.uint32)
    for i, lp in enumerate(lights):
        one, _, _, _ = gpu_render(vrt, ds, w, h, shadow=1, params=plist[i])
        assert np.array_equal(got[i], one), i
        rpx, _, _, _ = po.render_ex(sc, w, h, po.shade_params(light_pos=lp), 1)
        assert np.array_equal(one, rpx), i
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
