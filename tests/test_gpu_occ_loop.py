"""GPU: the occlusion-only form of the shadow frame kernels' traversal loop (RT_OCC_LOOP) against the oracle on the same inputs -- hit
records bit-exact, the occlusion bit (bit 31 of blasIdx in the kernel's record) equal to what the faithful restatement decides in any-hit
mode, packed RGB8 equal.

A wavefront takes that form each time it enters the traversal loop with an any-hit ray in every lane that holds work: the second half of
a tile all of whose primary rays hit (lanes outside the frame hold nothing).  A tile with a miss hands the missed lanes the next tile's
primary rays, and the wavefront keeps the general loop.  In the occlusion-only form a stack entry is the 4-byte descriptor, so the LDS rows
hold 2 * LSTK entries per lane (LSTK = 6 in the 7-wavefront kernels, 5 in the 8-wavefront ones) before scratch; heights, visiting order
(slot order) and the capacity are those of the general loop's occlusion arm.  The identity-root kernels hold that form (scenes of one
identity instance: every hand-made tree here, the atrium); the general kernels keep the one loop.

The chain trees are test_gpu_stack_push's: level i has one chain child and sib[i] single-triangle leaves, deeper = nearer to the camera.
With the light BEHIND the stack of triangles (further along +x), the occlusion ray of a pixel in the middle of the frame starts on the
deepest triangle and runs back through every sibling of every level: at each level it enters the chain child (slot 0, which holds its
origin) and leaves sib[i] entries pending, exactly as the primary ray did.  occlusion_steps() below restates that in slot order."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import _bits, _occlusion_oracle, gpu_render
from test_gpu_stack_push import _chain, _translated, _tree_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((17, 9), (64, 64))
BEHIND = (2000.0, 100.0, 0.0)                            # light behind the chain trees' triangles (x = 420 - ...)
LSTKS = (6, 5)


def _params(vrt, light):
    p = vrt.rtapi.default_shade_params()
    p.light_pos[:] = light
    return p


def _shadow_frame_equals_oracle(vrt, po, sc, ds, w, h, light):
    """-> (oracle's hit records, occluded mask, hit mask) of the frame, after the comparison"""
    pp = po.shade_params(light_pos=light)
    rpx, rhits, _, rn = po.render_ex(sc, w, h, pp, 1)
    px, hn, _, n = gpu_render(vrt, ds, w, h, shadow=1, params=_params(vrt, light))
    occ_gpu = gpu_render.occluded
    assert np.array_equal(_bits(hn), _bits(rhits)), (w, h)
    occ_ref, hit_mask = _occlusion_oracle(po, sc, w, h, pp, rhits)
    np.testing.assert_array_equal(occ_gpu, occ_ref)      # bit 31 of blasIdx
    assert np.array_equal(px, rpx), (w, h)
    assert n == rn
    return rhits, occ_ref, hit_mask


def _tiles_with_hits_and_misses(hit_mask):
    """per 8x8 tile of the frame (lanes outside the frame hold nothing): does it hold a hit, does it hold a miss"""
    h, w = hit_mask.shape
    out = []
    for ty in range(0, h, 8):
        for tx in range(0, w, 8):
            t = hit_mask[ty:ty + 8, tx:tx + 8]
            out.append((bool(t.any()), bool((~t).any())))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# flat scenes: quads facing the fixed camera ((0,100,0), looking along +x) in the plane x = X, a blocker behind the camera
# ---------------------------------------------------------------------------------------------------------------------------------
X_WALL = 400.0
LIGHT_BACK = (-300.0, 100.0, 0.0)                        # behind the camera: occlusion rays run back past it


def _balanced(ids):
    """nested lists (at most four children per node) over the triangle indices"""
    ids = list(ids)
    if len(ids) <= 4:
        return ids
    step = -(-len(ids) // 4)
    return [(_balanced(ids[i:i + step]) if len(ids[i:i + step]) > 1 else ids[i]) for i in range(0, len(ids), step)]


def _quad_x(x, y0, y1, z0, z1):
    return [[x, y0, z0, x, y1, z0, x, y1, z1], [x, y0, z0, x, y1, z1, x, y0, z1]]


def _column_edges(po, w, h):
    """z at which the boundaries between the pixel columns of a w x h frame meet the plane x = X_WALL, and the y extent of the rows"""
    rays = po.camera_rays(w, h).reshape(h, w, 6).astype(np.float64)
    z = rays[h // 2, :, 2] + rays[h // 2, :, 5] / rays[h // 2, :, 3] * (X_WALL - rays[h // 2, :, 0])
    y = rays[:, w // 2, 1] + rays[:, w // 2, 4] / rays[:, w // 2, 3] * (X_WALL - rays[:, w // 2, 0])
    edges = np.concatenate([[z[0] - (z[1] - z[0]) / 2], (z[1:] + z[:-1]) / 2, [z[-1] + (z[-1] - z[-2]) / 2]])
    yedges = np.concatenate([[y[0] - (y[1] - y[0]) / 2], (y[1:] + y[:-1]) / 2, [y[-1] + (y[-1] - y[-2]) / 2]])
    return edges, yedges


def flat_scene(vrt, po, kind):
    """kind "wall": one quad over the whole 64 x 64 frame (every pixel hits).  "strips": quads over pixel columns 8k .. 8k+3 of the 64 x 64
    frame, all rows (every tile holds hits and background).  "half": the wall over the rows above the middle, the strips below it (only
    some tiles are mixed).  Behind the camera a blocker hides the light from the part of the plane with z > 0."""
    edges, yedges = _column_edges(po, 64, 64)
    ylo, yhi = float(min(yedges[0], yedges[-1])) - 1500.0, float(max(yedges[0], yedges[-1])) + 1500.0   # (beyond any frame's view)
    ymid = float(yedges[32])
    up = yedges[0] > yedges[-1]                          # row 0 is the top of the frame if y falls with the row index
    tris = []

    def strips(y0, y1):
        for k in range(8):
            a, b = sorted((float(edges[8 * k]), float(edges[8 * k + 4])))
            tris.extend(_quad_x(X_WALL, y0, y1, a, b))

    zlo, zhi = float(min(edges[0], edges[-1])) - 1500.0, float(max(edges[0], edges[-1])) + 1500.0
    if kind == "wall":
        tris.extend(_quad_x(X_WALL, ylo, yhi, zlo, zhi))
    elif kind == "strips":
        strips(ylo, yhi)
    else:
        top, bottom = ((ymid, yhi), (ylo, ymid)) if up else ((ylo, ymid), (ymid, yhi))
        tris.extend(_quad_x(X_WALL, top[0], top[1], zlo, zhi))
        strips(*bottom)
    tris.extend(_quad_x(-100.0, -1000.0, 1200.0, 0.0, 1000.0))   # the blocker (behind the camera: no primary ray meets it)
    return _tree_scene(vrt, _balanced(range(len(tris))), tris, "flat_" + kind)


def test_pure_wavefronts_every_pixel_hits_and_the_light_is_inside(vrt, po, gpu_device):
    """Every tile's lanes all turn to their occlusion rays together: each wavefront enters the loop in its occlusion-only form for the
    second half of every tile.  The atrium is the headline's closed scene at a small tessellation level; the wall is the same situation
    on a hand-made tree."""
    for sc, light in ((vrt.scene.procedural("atrium", 5, 0, 3), (300.0, 480.0, 60.0)), (flat_scene(vrt, po, "wall"), LIGHT_BACK)):
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        for w, h in SIZES:
            rhits, occ, hit_mask = _shadow_frame_equals_oracle(vrt, po, sc, ds, w, h, light)
            assert hit_mask.all(), (sc.name, w, h)
            if (w, h) == (64, 64):
                assert occ.sum() >= 16 and (~occ).sum() >= 16, (sc.name, int(occ.sum()))
        ds.close()


def test_mixed_wavefronts_every_tile_has_hits_and_background(vrt, po, gpu_device):
    """Geometry over 4 of every 8 pixel columns: the lanes that missed take the next tile's primary rays beside this tile's occlusion
    rays, so every wavefront keeps the general loop for them."""
    sc = flat_scene(vrt, po, "strips")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    for w, h in SIZES:
        rhits, occ, hit_mask = _shadow_frame_equals_oracle(vrt, po, sc, ds, w, h, LIGHT_BACK)
        if (w, h) == (64, 64):
            assert all(a and b for a, b in _tiles_with_hits_and_misses(hit_mask))
            assert occ.sum() >= 16 and (hit_mask & ~occ).sum() >= 16
    ds.close()


def test_only_some_tiles_are_mixed(vrt, po, gpu_device):
    sc = flat_scene(vrt, po, "half")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    for w, h in SIZES:
        rhits, occ, hit_mask = _shadow_frame_equals_oracle(vrt, po, sc, ds, w, h, LIGHT_BACK)
        if (w, h) == (64, 64):
            t = _tiles_with_hits_and_misses(hit_mask)
            assert sum(1 for a, b in t if a and not b) >= 16 and sum(1 for a, b in t if a and b) >= 16, t
            assert occ.sum() >= 16 and (hit_mask & ~occ).sum() >= 16
    ds.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# stack heights
# ---------------------------------------------------------------------------------------------------------------------------------
def tilted_chain(sib, tris):
    """test_gpu_stack_push's _chain with the deepest triangle tilted out of its plane x = const (by +-1: it stays the nearest).  An
    occlusion ray starts 0.001 off the triangle it comes from; a triangle in a plane x = const has a box without thickness, which that
    ray never enters, so the last level would leave one entry less pending for the occlusion ray than for the primary ray.  The tilted
    triangle's box holds the ray's origin: the last level's step visits it (slot 0) and pushes every sibling."""
    root = _chain(sib, tris)
    deepest = root
    while not isinstance(deepest, int):
        deepest = deepest[0]
    t = tris[deepest]
    t[0] -= 1.0; t[3] -= 1.0; t[6] += 1.0
    return root


def _levels(P):
    """levels of three siblings (and one of P % 3) that leave P entries pending"""
    return (3,) * (P // 3) + ((P % 3,) if P % 3 else ())


# P entries pending in front of the last level's step: the register top is occupied and sp = P - 1 memory slots are in use (P = 0: nothing
# at all, sp = 0).  sp = 0 .. 14 = 2 * LSTK + 2 of the 7-wavefront kernels (2 * LSTK + 4 of the 8-wavefront ones); 1, 2, 3 entries pushed.
HEIGHT_CASES = [(P, s) for P in range(0, 16) for s in (1, 2, 3)]


def occlusion_steps(root, tris, org, dirn, tmax):
    """Slot-order any-hit traversal of the nested lists `root` (a child is a list = internal node, or an int = a leaf with that one
    triangle) by the ray org + t dirn, 0 < t < tmax, on the triangles' own boxes (the quantised boxes are supersets: the same decisions
    for a ray through the middle).  The first child whose box the ray enters before tmax is visited, the others are pushed as they come,
    the newest pending entry is taken next; the first triangle met before tmax ends the ray.
    -> [(pending entries in front of the step, entries it pushed)] of the node steps, and whether the ray was blocked."""
    t3 = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    org, dirn = np.asarray(org, np.float64), np.asarray(dirn, np.float64)

    def box(c):
        if isinstance(c, int):
            return t3[c].min(0), t3[c].max(0)
        bs = [box(x) for x in c]
        return np.min([b[0] for b in bs], 0), np.max([b[1] for b in bs], 0)

    def enters(c):
        lo, hi = box(c)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (lo - org) / dirn, (hi - org) / dirn
        tmin, tmx = np.minimum(t1, t2).max(), np.maximum(t1, t2).min()
        return not (tmx < tmin or tmx <= 0) and tmin < tmax

    def tri_hit(i):
        v0, e1, e2 = t3[i][0], t3[i][1] - t3[i][0], t3[i][2] - t3[i][0]
        hv = np.cross(dirn, e2)
        a = e1 @ hv
        if abs(a) < 1e-12:
            return False
        s = org - v0
        u = (s @ hv) / a
        q = np.cross(s, e1)
        v = (dirn @ q) / a
        t = (e2 @ q) / a
        return 0 <= u <= 1 and v >= 0 and u + v <= 1 and 1e-6 < t < tmax

    steps, pending, cur = [], [], root
    while True:
        if isinstance(cur, int):
            if tri_hit(cur):
                return steps, True
            if not pending:
                return steps, False
            cur = pending.pop()
            continue
        valid = [c for c in cur if enters(c)]
        if valid:
            steps.append((len(pending), len(valid) - 1))
            pending.extend(valid[1:])
            cur = valid[0]
        elif pending:
            cur = pending.pop()
        else:
            return steps, False


def _middle_occlusion_ray(po, sc, light):
    """the occlusion ray of the pixel in the middle of the 64 x 64 frame, as shadow_ray builds it"""
    rays = po.camera_rays(64, 64)
    i = 32 * 64 + 33
    hits, _ = po.trace_canonical(sc, rays[i:i + 1])
    assert hits["dist"][0] < 1e29
    I = rays[i, :3].astype(np.float64) + rays[i, 3:].astype(np.float64) * float(hits["dist"][0])
    L = np.asarray(light, np.float64) - I
    dist = float(np.linalg.norm(L))
    return I + L / dist * 0.001, L / dist, dist


def test_the_height_cases_cover_both_lds_boundaries_of_both_kernels():
    """(no GPU work: the case table itself)  sp = 0 .. 2 * LSTK + 2 with 1, 2 and 3 entries pushed, for both LSTK: the steps that stay in
    the 4-byte rows, those that cross their end (2 * LSTK) and those in scratch -- and the general form's boundary (LSTK) on the way."""
    for lstk in LSTKS:
        for sp in range(0, 2 * lstk + 3):
            for s in (1, 2, 3):
                assert (sp + 1, s) in HEIGHT_CASES
        assert (0, 1) in HEIGHT_CASES                    # (sp = 0 with the register top empty)


@pytest.mark.parametrize("P,s", HEIGHT_CASES)
def test_an_occlusion_step_that_pushes_s_entries_with_P_pending(vrt, po, gpu_device, P, s):
    sib = _levels(P) + (s,)
    tris = []
    root = tilted_chain(sib, tris)
    sc = _tree_scene(vrt, root, tris, "occ_chain_%d_%d" % (P, s))
    org, dirn, dist = _middle_occlusion_ray(po, sc, BEHIND)
    steps, blocked = occlusion_steps(root, tris, org, dirn, dist)
    assert (P, s) in steps and max(a + b for a, b in steps) == P + s and blocked, steps
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    for w, h in SIZES:
        rhits, occ, hit_mask = _shadow_frame_equals_oracle(vrt, po, sc, ds, w, h, BEHIND)
        if (w, h) == (64, 64):
            # the whole tile of the pixel hits, so its wavefront takes the occlusion-only loop (and the 4-byte stack) for these rays
            assert hit_mask[32:40, 32:40].all() and occ[32, 33]
    ds.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# stack limits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,entries,shallow", [(16, 48, 1), (32, 96, 0)])
def test_occlusion_rays_fill_each_depth_class_exactly(vrt, po, gpu_device, k, entries, shallow):
    """16 levels of three siblings fill the 48 entries of the shallow stacks, 32 levels the full-size 96, for the occlusion ray as for
    the primary ray: the frames equal the oracle's and no overflow is reported (gpu_render asserts a zero status)."""
    tris = []
    root = tilted_chain((3,) * k, tris)
    sc = _tree_scene(vrt, root, tris, "occ_chain_%d_levels" % k)
    _, st = po.trace_canonical(sc, po.camera_rays(64, 64))
    assert st["max_stack"] == entries                    # (the primary rays fill it too, in the general loop)
    org, dirn, dist = _middle_occlusion_ray(po, sc, BEHIND)
    steps, blocked = occlusion_steps(root, tris, org, dirn, dist)
    assert max(a + b for a, b in steps) == entries and blocked
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    if os.environ.get("VXRT_SHALLOW") != "0":
        assert vrt.rtapi.accel_info(ds.accel, 1) == shallow
    _shadow_frame_equals_oracle(vrt, po, sc, ds, 64, 64, BEHIND)
    ds.close()


def test_thirty_five_levels_report_the_overflow_bit_and_nothing_else(vrt, po, gpu_device):
    import torch
    from scenes import chain_bvh4
    sc = chain_bvh4(vrt, 35)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    s = torch.cuda.current_stream().cuda_stream
    px = torch.zeros((64, 64), dtype=torch.int32, device=gpu_device)
    vrt.rtapi.render(ds.accel, 64, 64, 0, 64, _params(vrt, BEHIND), px.data_ptr(), 1, None, None, None, s)
    assert vrt.rtapi.status(s) == 1                      # STATUS_STACK_OVERFLOW alone
    assert vrt.rtapi.status(s) == 0                      # read-and-clear
    ds.close()
    ok = chain_bvh4(vrt, 3)                              # the next scene on the device is unaffected
    d2 = vrt.tracer.DeviceScene(ok, gpu_device)
    _shadow_frame_equals_oracle(vrt, po, ok, d2, 17, 9, BEHIND)
    d2.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# general kernels (TLAS level inside the loop), camera frames
# ---------------------------------------------------------------------------------------------------------------------------------
SIDE = (-200.0, 100.0, 600.0)                            # behind the camera and to its side


def two_instance_scene(vrt):
    """A wall over the whole frame (instance 0) and, in front of its lower part, a smaller panel (instance 1) whose instance record is a
    translation: occlusion rays start at TLAS level, pass the instance step of one or both instances and come back to the TLAS level."""
    wall = np.array(_quad_x(X_WALL, -2000.0, 2200.0, -2000.0, 2000.0), np.float32)
    panel = np.array(_quad_x(250.0, -300.0, 100.0, -150.0, 150.0), np.float32)
    sc = vrt.scene.from_triangles([wall, panel])
    bufs = {k: np.frombuffer(bytes(v), np.uint8).copy() for k, v in sc.buffers.items()}
    rec = bufs["blas"].view(np.float32).reshape(-1, 40)
    assert len(rec) == 2
    rec[1, 1 + 3] -= 7.0                                 # invTransform[0][3]
    rec[1, 17 + 3] += 7.0                                # transform[0][3]
    return vrt.scene.Scene(bufs, name="two_instances")


def test_general_kernels_trace_occlusion_rays_through_instances(vrt, po, gpu_device):
    """Scenes that are not one identity instance take the general kernels, which keep the one loop (the second loop cost their register
    allocation too much: DESIGN s5, rejected): their occlusion rays pass the instance step and come back to the TLAS level in the
    general loop's occlusion arm."""
    light = SIDE                                         # the panel's shadow falls on the wall beside it; every pixel hits
    for sc in (_translated(vrt, vrt.scene.procedural("cornell")), two_instance_scene(vrt)):
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        assert vrt.rtapi.accel_info(ds.accel, 5) == 0    # no identity-root kernels
        for w, h in SIZES:
            rhits, occ, hit_mask = _shadow_frame_equals_oracle(vrt, po, sc, ds, w, h, light)
            if (w, h) == (64, 64) and sc.name == "two_instances":
                assert hit_mask.all() and len(np.unique(rhits["blasIdx"])) == 2
                assert occ.sum() >= 16 and (~occ).sum() >= 16, int(occ.sum())
        ds.close()


def test_caller_camera_shadow_frames(vrt, po, gpu_device):
    import torch
    import camera_ref as cr
    from test_gpu_camera import _check, _host_frame, _render_camera
    w, h = 64, 64
    for sc, light in ((vrt.scene.procedural("atrium", 5, 0, 3), (300.0, 480.0, 60.0)), (two_instance_scene(vrt), SIDE)):
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        for eye in ((0.0, 100.0, 0.0), (20.0, 120.0, 15.0)):
            cam = np.array(eye + (1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0), np.float32)
            got = _host_frame(*_render_camera(vrt, ds, cam, w, h, _params(vrt, light), 1), w, h, 0, h)
            assert vrt.rtapi.status(torch.cuda.current_stream().cuda_stream) == 0
            _check(got, cr.frame(sc, cam, w, h, po.shade_params(light_pos=light), 1), "%s eye %r" % (sc.name, eye))
        ds.close()


def test_a_batch_of_three_frames_on_two_streams_equals_the_frames_one_by_one(vrt, po, gpu_device):
    import torch
    sc = flat_scene(vrt, po, "half")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    w, h = 64, 64
    lights = (LIGHT_BACK, (-300.0, 100.0, 120.0), (-250.0, 300.0, -90.0))
    plist = [_params(vrt, lp) for lp in lights]
    streams = [torch.cuda.Stream(device=gpu_device) for _ in range(2)]
    bufs = [torch.zeros((3, h, w), dtype=torch.int32, device=gpu_device) for _ in streams]
    torch.cuda.synchronize()
    for st, buf in zip(streams, bufs):
        vrt.rtapi.render_batch(ds.accel, w, h, plist, buf.data_ptr(), w * h, 1, None, st.cuda_stream)
    for st in streams:
        st.synchronize()
        assert vrt.rtapi.status(st.cuda_stream) == 0
    for i, lp in enumerate(lights):
        one, _, _, _ = gpu_render(vrt, ds, w, h, shadow=1, params=plist[i])
        rpx, _, _, _ = po.render_ex(sc, w, h, po.shade_params(light_pos=lp), 1)
        assert np.array_equal(one, rpx), i
        for buf in bufs:
            assert np.array_equal(buf.cpu().numpy().view(np.uint32)[i], one), i
    ds.close()


def test_the_eight_wavefront_kernels_pass_the_same_cases(vrt, gpu_device):
    """The 8-wavefront instantiations (5 LDS levels: ten 4-byte rows) are what frames in overlapping sets run; small frames take them
    only when forced (VXRT_PACKED=1), which is read once per process: a child process runs this file's other tests with it."""
    if os.environ.get("VXRT_PACKED") == "1":
        return
    env = dict(os.environ, VXRT_PACKED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "not eight_wavefront"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
