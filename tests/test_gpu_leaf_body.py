"""GPU: the leaf body of the frame kernels -- the straight-line triangle test (ray_tri_flat) inside the triangle loop, with lanes of
one wavefront in leaves of different sizes -- against the oracle on the same inputs (hit records bit-exact, packed RGB8 equal; the
helpers of tests/test_gpu_parity.py).  The cases hold for any form of the loop, per-lane or walked in step.

One hand-built tree (leaf_scene) holds every case, and an 8x8 frame -- one tile, one wavefront -- meets all of them.  The fixed camera
sits at (0, 100, 0) and looks along +x; pixel (px, py) of the 8x8 frame looks at (400, 100 (py - 3), 100 (px - 4)) of the plane x = 400,
called the cell (px, py) below.  Column 4 and row 4 have a zero direction component and belong to the EXACT launch; the cells used are
the other ones.

  row 1   leaves of 1, 2, 3, 7, 15 inline triangles and one of 17 (kept by reference: the triCount == 0 path), side by side under
          two sibling nodes, so the lanes of the tile reach them in the same iteration and walk leaves of different sizes in one run of
          the leaf body; their triangles lie behind each other, far to near in index order (a nearer triangle later in the leaf: every
          one of them is accepted), in the leaf of 7 near to far (only the first is)
  row 2   boundary rays.  v = -0.5 there, so dy = -dx / 2 exactly: the ray of the row runs through the edge y = -100 of the plane
          x = 400 with products that cancel exactly (w1 == 0 for the two triangles that share the edge, cells 1-3), through the
          vertex four triangles share (cell 6: w1 == w2 == 0) and through the second vertex of a triangle (cell 5: w1 near 1)
  row 3   ties: two bit-identical triangles in one leaf, in front of a third (cell 0) and behind a farther first one (cell 1): the
          lower index wins; the abandon test (cell 2): a leaf whose box lies BEHIND three of its four triangles, so the second
          triangle's hit shrinks hit.dist below the path's entry distance and the two nearer triangles after it are never tested
  row 0   degenerate triangles in front of an ordinary one: zero area (a point, a segment), vertices that are NaN, +inf, -inf
          (cell 0); triangles edge-on to the ray of cell 1 with |a| on both sides of RT_EPSILON (cell 1)
  near    two triangles in the plane x = 5e-7 and x = 2e-6 in front of the camera: tf on both sides of RT_EPSILON; the second
          covers the quadrant px > 4, py > 4 and is those pixels' hit
  above   (outside the view, on the way to the light at (10, 900, 0)) three leaves of three triangles whose first, middle and last
          triangle blocks the occlusion ray of the hit in cells 0, 1, 3 of row 3; the other two triangles of each are missed

What the inputs contain is asserted on the oracle's own output (no GPU): test_the_oracle_alone_meets_every_case."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import _bits, gpu_render

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHT = (10.0, 900.0, 0.0)                              # (x > 0: behind the two planes in front of the camera every ray would be blocked)
LIGHTS = (LIGHT, (50.0, 180.0, 40.0), (300.0, 800.0, -200.0))
SIZES = ((8, 8), (17, 9), (64, 64))
BLOCKED = (0, 1, 3)                                      # cells of row 3 whose occlusion ray meets a blocker leaf
EPS = np.float32(1e-6)                                   # RT_EPSILON
f32 = np.float32


def _cell(px, py):
    """(y, z) of cell (px, py) in the plane x = 400"""
    return 100.0 * (py - 3), 100.0 * (px - 4)


def _at(x, y400, z400):
    """the point of the plane x = const on the camera ray through (400, y400, z400)"""
    return [x, 100.0 + (y400 - 100.0) * x / 400.0, z400 * x / 400.0]


def _facing(x, px, py, r=20.0):
    """a triangle in the plane x = const around the ray of cell (px, py)"""
    y, z = _cell(px, py)
    return _at(x, y - r, z - r) + _at(x, y + 2 * r, z - r) + _at(x, y - r, z + 2 * r)


def _ray8(px, py):
    """the camera ray of pixel (px, py) of the 8x8 frame, as orc_generate_ray computes it"""
    d = np.array([1.0, (py * 2.0 - 8) / 8, (px * 2.0 - 8) / 8], np.float32)
    n = np.sqrt((d[0] * d[0] + d[1] * d[1]).astype(f32) + (d[2] * d[2]).astype(f32)).astype(f32)
    return np.array([0, 100, 0], np.float32), (d / n).astype(f32)


def tri_terms(o, d, t):
    """a, w1, w2, tf of ray_tri (rt_kernels.hip) in float32, operation by operation; t = the nine floats v0, v1, v2"""
    t = np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        v0, e1, e2 = t[0:3], (t[3:6] - t[0:3]).astype(f32), (t[6:9] - t[0:3]).astype(f32)
        m = lambda x, y: f32(f32(x) * f32(y))
        cross = lambda p, q: (f32(m(p[1], q[2]) - m(p[2], q[1])), f32(m(p[2], q[0]) - m(p[0], q[2])), f32(m(p[0], q[1]) - m(p[1], q[0])))
        dot = lambda p, q: f32(f32(m(p[0], q[0]) + m(p[1], q[1])) + m(p[2], q[2]))
        h = cross(d, e2)
        a = dot(e1, h)
        f = f32(1) / a
        s = (o - v0).astype(f32)
        w1 = m(f, dot(s, h))
        q = cross(s, e1)
        w2 = m(f, dot(d, q))
        tf = m(f, dot(e2, q))
    return a, w1, w2, tf


def _edge_on(px, py, want_below):
    """a triangle edge-on to the ray of cell (px, py) of the 8x8 frame whose determinant |a| lies just below / just above RT_EPSILON:
    a short edge across the ray, the other along it; the far vertex is moved across the ray's plane one float at a time and tri_terms
    (the kernel's arithmetic) picks the position nearest to the threshold on the wanted side"""
    o, d = _ray8(px, py)
    v0 = (o + d * f32(380.0)).astype(f32)
    v1 = (v0 + np.array([0, 0, 2.0 ** -8], np.float32)).astype(f32)
    v2 = (v0 + d).astype(f32)
    best = None
    y = v2[1]
    for _ in range(300):
        y = np.nextafter(y, f32(-1e9))
    for _ in range(600):
        y = np.nextafter(y, f32(1e9))
        t = np.concatenate([v0, v1, [v2[0], y, v2[2]]]).astype(f32)
        a = abs(tri_terms(o, d, t)[0])
        ok = (f32(0.5e-6) < a < EPS) if want_below else (EPS < a < f32(2e-6))
        if ok and (best is None or abs(a - EPS) < best[0]):
            best = (abs(a - EPS), t)
    assert best is not None
    return list(best[1])


class Leaf:
    def __init__(self, name, tris, box=None):
        self.name, self.tris, self.box = name, [list(map(float, t)) for t in tris], box


def _leaves():
    L = []
    # row 1: the sizes
    for px, n in ((0, 1), (1, 2), (2, 3), (3, 7), (5, 15), (6, 17)):
        xs = [440.0 - 2.0 * j for j in range(n)]
        if n == 7:
            xs = xs[::-1]
        L.append(Leaf("size%d" % n, [_facing(x, px, 1) for x in xs]))
    # row 2: the shared edge y = -100, z = -350 .. -50 of the plane x = 400, the shared vertex (400, -100, 200), a second vertex at (400, -100, 100)
    L.append(Leaf("edge", [[400, -100, -350, 400, -160, -200, 400, -100, -50], [400, -100, -350, 400, -40, -200, 400, -100, -50]]))
    L.append(Leaf("vertex", [[400, -100, 200, 400, -100 + sy * 60, 200, 400, -100, 200 + sz * 60] for sy in (-1, 1) for sz in (-1, 1)]))
    L.append(Leaf("vertex1", [[400, -160, 100, 400, -100, 100, 400, -160, 160]]))
    # row 3: ties and the abandon test
    a, b = _facing(410.0, 0, 3), _facing(430.0, 0, 3)
    L.append(Leaf("tie_first", [a, a, b]))
    a, b = _facing(410.0, 1, 3), _facing(430.0, 1, 3)
    L.append(Leaf("tie_last", [b, a, a]))
    y, z = _cell(2, 3)
    L.append(Leaf("abandon", [_facing(455.0, 2, 3), _facing(420.0, 2, 3), _facing(418.0, 2, 3), _facing(416.0, 2, 3)],
                  box=([450.0, y - 60, z - 60], [460.0, y + 60, z + 60])))
    # row 0: degenerate triangles in front of an ordinary one
    p = _at(400.0, *_cell(0, 0))
    q = [p[0], p[1] + 10, p[2] + 10]
    nan, inf = float("nan"), float("inf")
    good = _facing(430.0, 0, 0)
    junk = [p + p + p, p + q + [p[0], p[1] + 5, p[2] + 5], [nan] + good[1:], good[:4] + [inf] + good[5:], good[:8] + [-inf], [nan] * 9, good]
    L.append(Leaf("junk", junk, box=([395.0, p[1] - 60, p[2] - 60], [435.0, p[1] + 60, p[2] + 60])))
    L.append(Leaf("edge_on", [_edge_on(1, 0, True), _edge_on(1, 0, False), _facing(430.0, 1, 0)]))
    # in front of the camera: tf below RT_EPSILON (the whole view), above it (the quadrant y > 100, z > 0)
    B = 500.0
    L.append(Leaf("near", [[5e-7, 100 - B, -B, 5e-7, 100 + 3 * B, -B, 5e-7, 100 - B, 3 * B], [2e-6, 100, 0, 2e-6, 100 + B, 0, 2e-6, 100, B]]))
    L.append(Leaf("plain", [_facing(410.0, 3, 3)]))
    # above the view: the blockers of the occlusion rays of tie_first, tie_last and plain (row 3, hit at x = 410; light at (10, 900, 0):
    # nothing else of the tree lies on their way)
    for k, px in enumerate(BLOCKED):
        hit = np.array(_at(410.0, *_cell(px, 3)))
        m = hit + (np.array(LIGHT) - hit) * 0.5                                 # the occlusion ray's midpoint
        blocker = [m[0], m[1] - 20, m[2] - 20, m[0], m[1] + 40, m[2] - 20, m[0], m[1] - 20, m[2] + 40]
        miss = lambda dy: [m[0], m[1] + dy, m[2] + 30, m[0], m[1] + dy + 2, m[2] + 30, m[0], m[1] + dy, m[2] + 32]
        tris = [miss(30.0), miss(34.0)]
        tris.insert(k, blocker)
        L.append(Leaf("blocker%d" % k, tris, box=([m[0] - 1, m[1] - 25, m[2] - 25], [m[0] + 1, m[1] + 45, m[2] + 45])))
    return L


def _box(c):
    if isinstance(c, Leaf):
        if c.box is not None:
            return np.array(c.box[0], np.float32), np.array(c.box[1], np.float32)
        t = np.array(c.tris, np.float32).reshape(-1, 3)
        return t.min(0), t.max(0)
    bs = [_box(x) for x in c]
    return np.min([b[0] for b in bs], 0), np.max([b[1] for b in bs], 0)


def leaf_scene(vrt):
    """(scene, {leaf name: (first triangle, count)}).  A BVH4 in the RTU test's formats under the identity instance of the cornell
    scene, built as tests/test_gpu_stack_push.py::_tree_scene builds its trees (children next to each other behind their parent,
    origin + ldexp(q, e) with floor / ceil), with leaves of any size and, where a case needs it, a leaf box that is not its triangles'."""
    leaves = _leaves()
    tris, where = [], {}
    for lf in leaves:
        where[lf.name] = lf.first, lf.count = len(tris), len(lf.tris)
        tris += lf.tris
    # sizes 1, 2, 3, 7 under one node and 15, 17 under its sibling; the others in fours
    groups = [leaves[0:4], leaves[4:8], leaves[8:12], leaves[12:16], leaves[16:]]
    root = [[groups[0], groups[1], groups[2], groups[3]], [g for g in groups[4:] if g]]
    base = vrt.scene.procedural("cornell")
    tris = np.asarray(tris, np.float32)

    def count(c):
        return 1 if isinstance(c, Leaf) else 1 + sum(count(x) for x in c)

    nodes = np.zeros((count(root), 52), np.uint8)
    todo, free = [(0, root)], 1
    while todo:
        idx, kids = todo.pop(0)
        assert 1 <= len(kids) <= 4
        first, free = free, free + len(kids)
        boxes = [_box(c) for c in kids]
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
            if isinstance(kids[c], Leaf):
                leaf = nodes[first + c]
                leaf[0:12] = blo.astype(np.float32).view(np.uint8)
                leaf[16:20] = np.array([kids[c].first], np.uint32).view(np.uint8)
                leaf[20:24] = np.array([kids[c].count], np.uint32).view(np.uint8)
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
    return vrt.scene.Scene(b, name="leaf_body"), where


_shared = {}


def _scene(vrt):
    if "scene" not in _shared:
        _shared["scene"] = leaf_scene(vrt)
    return _shared["scene"]


def _oracle_frame(vrt, po, w, h, shadow, light=LIGHT):
    """the oracle's frame, computed once per (size, shadow, light) and shared"""
    key = (w, h, shadow, light)
    if key not in _shared:
        _shared[key] = po.render_ex(_scene(vrt)[0], w, h, po.shade_params(light_pos=light), shadow)
    return _shared[key]


def _params(vrt, light=LIGHT):
    p = vrt.rtapi.default_shade_params()
    p.light_pos[:] = light
    return p


def _tris(sc):
    return np.frombuffer(bytes(sc["tri"]), np.float32).reshape(-1, 9)


def test_the_oracle_alone_meets_every_case(vrt, po):
    """(no GPU work)  The 8x8 frame of the oracle contains the cases the file is about."""
    sc, where = _scene(vrt)
    tris = _tris(sc)
    _, hits, _, _ = _oracle_frame(vrt, po, 8, 8, 1)
    hit = hits["dist"] < 1e29
    tri_of = lambda px, py: int(hits["triIdx"][py, px]) if hit[py, px] else -1
    last = lambda name: where[name][0] + where[name][1] - 1
    # leaf sizes: the ray of each cell of row 1 ends on its leaf's nearest triangle -- the last one, in the leaf of 7 the first one
    assert [where["size%d" % n][1] for n in (1, 2, 3, 7, 15, 17)] == [1, 2, 3, 7, 15, 17]
    for px, n in ((0, 1), (1, 2), (2, 3), (5, 15), (6, 17)):
        assert tri_of(px, 1) == last("size%d" % n), (px, n)
    assert tri_of(3, 1) == where["size7"][0]
    # a barycentric that is exactly zero: the shared edge (the lower index of the two wins), the shared vertex
    on_edge = [(px, 2) for px in (1, 2, 3) if tri_of(px, 2) == where["edge"][0] and hits["bx"][2, px] == 0.0]
    assert len(on_edge) == 3, on_edge
    assert tri_of(6, 2) == where["vertex"][0] and hits["bx"][2, 6] == 0.0 and hits["by"][2, 6] == 0.0
    assert tri_of(5, 2) == where["vertex1"][0] or not hit[2, 5]      # (w1 within rounding of 1: either side is a case)
    # equal distance: bit-identical triangles, the lower index is the hit; a tie behind a farther first triangle
    for name, px, k in (("tie_first", 0, 0), ("tie_last", 1, 1)):
        i = where[name][0] + k
        assert np.array_equal(_bits(tris[i]), _bits(tris[i + 1])) and tri_of(px, 3) == i, name
    o, d = _ray8(0, 3)
    assert tri_terms(o, d, tris[where["tie_first"][0]])[3] == tri_terms(o, d, tris[where["tie_first"][0] + 1])[3] == hits["dist"][3, 0]
    # the abandon test: the hit is the leaf's second triangle although two nearer ones follow it, and the oracle counts abandons
    assert tri_of(2, 3) == where["abandon"][0] + 1
    o, d = _ray8(2, 3)
    assert all(0 < tri_terms(o, d, tris[where["abandon"][0] + k])[3] < hits["dist"][3, 2] for k in (2, 3))
    _, st = po.trace_canonical(sc, po.camera_rays(8, 8))
    assert st["abandon"] >= 1
    # degenerate triangles are passed over: the ordinary triangle behind them is the hit
    assert tri_of(0, 0) == last("junk") and tri_of(1, 0) == last("edge_on")
    assert not np.isfinite(tris[where["junk"][0]:last("junk")]).all() and np.isnan(tris[where["junk"][0] + 5]).all()
    o, d = _ray8(1, 0)
    a_lo, a_hi = (abs(tri_terms(o, d, tris[where["edge_on"][0] + k])[0]) for k in (0, 1))
    assert f32(0.5e-6) < a_lo < EPS < a_hi < f32(2e-6), (a_lo, a_hi)
    # tf on both sides of RT_EPSILON: the nearer plane is rejected for every pixel, the farther one is the hit of its quadrant
    n0 = where["near"][0]
    for px, py in ((5, 5), (7, 7), (6, 5)):
        o, d = _ray8(px, py)
        assert tri_terms(o, d, tris[n0])[3] <= EPS < tri_terms(o, d, tris[n0 + 1])[3] and tri_of(px, py) == n0 + 1
    assert not (hits["triIdx"][hit] == n0).any()
    # occlusion rays: blocked by the first, a middle and the last triangle of a leaf, and not blocked
    pp = po.shade_params(light_pos=LIGHT)
    from test_gpu_parity import _occlusion_oracle
    occ, hm = _occlusion_oracle(po, sc, 8, 8, pp, hits)
    assert all(occ[3, px] for px in BLOCKED), occ[3]
    assert (hm & ~occ).any()
    for k, px in enumerate(BLOCKED):
        i = where["blocker%d" % k][0]
        hp = (np.array([0, 100, 0], np.float64) + _ray8(px, 3)[1].astype(np.float64) * float(hits["dist"][3, px]))
        L = np.array(LIGHT) - hp
        so, sd = (hp + 0.001 * L / np.linalg.norm(L)).astype(f32), (L / np.linalg.norm(L)).astype(f32)
        blocks = []
        for j in range(3):
            a, w1, w2, tf = tri_terms(so, sd, tris[i + j])
            blocks.append(bool(abs(a) >= EPS and 0 <= w1 <= 1 and w2 >= 0 and w1 + w2 <= 1 and tf > EPS))
        assert blocks == [j == k for j in range(3)], (k, blocks)


def _frame_equals_oracle(vrt, po, ds, w, h, shadow, light=LIGHT):
    rpx, rhits, _, _ = _oracle_frame(vrt, po, w, h, shadow, light)
    px, hn, _, _ = gpu_render(vrt, ds, w, h, shadow=shadow, params=_params(vrt, light))
    assert np.array_equal(_bits(hn), _bits(rhits)), (w, h, shadow)
    assert np.array_equal(px, rpx), (w, h, shadow)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("shadow", [0, 1])
def test_frames_equal_the_oracle(vrt, po, gpu_device, w, h, shadow):
    sc, _ = _scene(vrt)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    _frame_equals_oracle(vrt, po, ds, w, h, shadow)
    if shadow:
        from test_gpu_parity import _occlusion_oracle
        _, rhits, _, _ = _oracle_frame(vrt, po, w, h, 1)
        occ, _ = _occlusion_oracle(po, sc, w, h, po.shade_params(light_pos=LIGHT), rhits)
        gpu_render(vrt, ds, w, h, shadow=1, params=_params(vrt))
        np.testing.assert_array_equal(gpu_render.occluded, occ)
    ds.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_triangle_counts_equal_the_oracle_counts(vrt, po, gpu_device, w, h):
    """The counting build tests exactly the triangles the oracle tests: none after a lane's leaf is abandoned, none for a lane that
    waits for its neighbours' longer leaves."""
    import torch
    sc, _ = _scene(vrt)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    px = torch.zeros((h, w), dtype=torch.int32, device=gpu_device)
    c = vrt.rtapi.render_stats(ds.accel, w, h, 0, h, _params(vrt), px.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    hits, st = po.trace_canonical(sc, po.camera_rays(w, h))
    assert st["abandon"] >= 1
    assert c["tri_fetches"] == st["tri_reads"]
    assert c["node_fetches"] == st["node_reads"]
    assert c["shaded_hits"] == int((hits["dist"] < 1e29).sum())
    rpx, _, _, _ = _oracle_frame(vrt, po, w, h, 0)
    assert np.array_equal(px.cpu().numpy().view(np.uint32), rpx)
    ds.close()


def test_a_batch_of_three_lights_equals_the_frames_one_by_one(vrt, po, gpu_device):
    import torch
    sc, _ = _scene(vrt)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    s = torch.cuda.current_stream().cuda_stream
    for w, h in ((8, 8), (64, 64)):
        plist = [_params(vrt, lp) for lp in LIGHTS]
        buf = torch.zeros((3, h, w), dtype=torch.int32, device=gpu_device)
        vrt.rtapi.render_batch(ds.accel, w, h, plist, buf.data_ptr(), w * h, 1, None, s)
        assert vrt.rtapi.status(s) == 0
        got = buf.cpu().numpy().view(np.uint32)
        for i, lp in enumerate(LIGHTS):
            one, _, _, _ = gpu_render(vrt, ds, w, h, shadow=1, params=plist[i])
            assert np.array_equal(got[i], one), (w, h, i)
            assert np.array_equal(one, _oracle_frame(vrt, po, w, h, 1, lp)[0]), (w, h, i)
    ds.close()


def test_the_eight_wavefront_kernels_pass_the_same_cases(vrt, gpu_device):
    """The 8-wavefront instantiations are what frames in overlapping sets run; small frames take them only when forced (VXRT_PACKED=1),
    which is read once per process: a child process runs this file's other tests with it."""
    if os.environ.get("VXRT_PACKED") == "1":
        return
    env = dict(os.environ, VXRT_PACKED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "not eight_wavefront"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
