"""GPU: both device builders (csrc/bvh_builder.hip: vxrt_bvh_build, vxrt_tlas_build) on hostile geometry, on the sizes that sit on
their hand-offs, with a scratch arena left dirty by other builds, and inside guarded buffers.  The families and sizes are those of
tests/builder_cases.py; tests/test_builder_cases_cpu.py holds the CPU builder to the same families and measures the hit counts the
caps below rely on.  "Right" is: the format's invariants, counts and bounds that match a walk over the emitted nodes and the input,
node bytes equal to the numpy restatement of the quantiser computed from the triangles up (tests/refit_ref.py), and the HIP traversal
bit-equal to the oracle on that tree.  No brute force here.

Non-finite input (section b).  vxrt_bvh_build / vxrt_tlas_build refuse a NaN or infinite coordinate with -1, by a flag that
bb_bounds_kernel raises; the kernels after it still run on the bad values before the host reads the flag.  Read on paper before these
cases first ran, a NaN and an inf through every stage (the note above build_common in csrc/bvh_builder.hip has the stage-by-stage
result): bounds drop a NaN in fminf / fmaxf and guard the empty case; the axis sequence always picks an axis with bits left; the Morton
quantiser clamps t (a NaN through !(t >= 0)) before the integer conversion and keys index nothing; the sort handles integers; in the
clustering a partner is always an existing position of the window (NaN orders after +inf), and a round that merges nothing is followed
by a forced round that pairs half the array, so the tail's loop ends; compaction and node ids come from ballots and prefix sums; the reinsertion's walks are bounded
by BB_RI_LISTS / BB_RI_STEPS / BB_RI_STACK and a NaN gain never asks for a move; the refit counts arrivals; the collapse's plan bits are
comparisons and its ranges integer counts; the quantiser maps NaN to 0 before converting and its loops are bounded by 255 and 126.
No index, loop bound or shared-memory address depends on a coordinate.  The reading found one value-dependent defect of another kind: a
node whose area overflows compared INFINITY <= INFINITY and became a leaf of any size (fixed in bb_merge: a leaf needs count <= leaf_max)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import builder_cases as bc
import refit_ref as rr
from test_gpu_parity import gpu_trace, _bits
from test_scene_builder import NODE, check_tree_fast

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INTERNAL = 0xFFFFFFFF


def _walk_counts(nodes):
    """(reachable nodes, leaves, largest leaf) of a BLAS by a walk from node 0."""
    idx = np.array([0], np.int64)
    n_nodes = n_leaves = max_leaf = 0
    while len(idx):
        n = nodes[idx]
        n_nodes += len(idx)
        leaf = n["ld"] != 0
        n_leaves += int(leaf.sum())
        if leaf.any():
            max_leaf = max(max_leaf, int(n["ld"][leaf].max()))
        nn = n[~leaf]
        valid = nn["ch"][:, :, 0] != 0
        idx = (nn["lf"].astype(np.int64)[:, None] + np.arange(4)[None, :])[valid]
    return n_nodes, n_leaves, max_leaf


def _tagged_ex(n):
    """Shading records that carry their triangle's input index (uv0.x, exact below 2^24): the records must move with the triangles."""
    ex = np.zeros((n, 16), F32)
    ex[:, 2] = ex[:, 5] = ex[:, 8] = 1.0
    ex[:, 9] = np.arange(n)
    return ex


def built(vrt, po, dev, tri, kind, leaf_max, min_hits=0):
    """Build `tri` on the GPU, read the scene back and hold it to everything that together is "the builder is right".  Returns the
    host scene (and the builder's info as sc.bvh_info)."""
    n = len(tri)
    ds = vrt.tracer.DeviceScene.build_on_gpu(tri, _tagged_ex(n), device=dev, leaf_max=leaf_max)
    try:
        sc, info = ds.to_host(), ds.bvh_info
        depth = check_tree_fast(sc)
        print("%s n %d leaf_max %d: depth %d, %d nodes, %d leaves, largest %d" % (kind, n, leaf_max, depth, info.n_nodes, info.n_leaves, info.max_leaf))
        assert depth == info.max_depth and depth < 32 and info.n_nodes == sc.n_bvh_nodes
        nodes = sc["bvh"].view(NODE)
        assert (info.n_nodes, info.n_leaves, info.max_leaf) == _walk_counts(nodes)
        assert 1 <= info.max_leaf <= min(leaf_max if leaf_max else 2, 15)
        v = tri.reshape(-1, 3)
        want_bounds = np.concatenate([v.min(0), v.max(0)]).astype(F32)
        assert np.array_equal(_bits(np.array(list(info.bounds), F32) + F32(0)), _bits(want_bounds + F32(0)))     # (+ 0: -0 and +0 are the same plane)
        out = sc["tri"].view(F32).reshape(-1, 9)
        src = sc["triEx"].view(F32).reshape(-1, 16)[:, 9].astype(np.int64)
        assert np.array_equal(np.sort(src), np.arange(n)) and np.array_equal(_bits(out), _bits(tri[src]))      # a permutation, records alongside
        # origin, exponents and every quantised plane: the restatement, from the triangles up
        _, want = rr.refit({k: sc[k] for k in ("tlas", "blas", "bvh", "tri")}, geometry=True)
        assert np.array_equal(want, sc["bvh"])
        rays = bc.rays_at(tri, kind)
        got = gpu_trace(vrt, ds, rays)
        ref, _ = po.trace_canonical(sc, rays)
        assert np.array_equal(_bits(got), _bits(ref))
        hits = int((got["dist"] < 1e29).sum())
        print("    %d of %d aimed rays hit" % (hits, len(rays)))
        assert hits >= min_hits
        sc.bvh_info = info
        return sc
    finally:
        ds.close()


def _cap(kind, n):
    return 10 if kind in bc.HITTING and n >= 300 else 0


# ---- a. hostile families, and the sizes on the hand-offs ----
@pytest.mark.parametrize("leaf_max", [1, 4])
@pytest.mark.parametrize("n", [300, 1025])
@pytest.mark.parametrize("kind", bc.FINITE)
def test_hostile_families(vrt, po, gpu_device, kind, n, leaf_max):
    """Every finite family builds (no -1, no -2) and is right.  For huge / tiny / subnormal / point / line / dups every surface-area
    comparison ties, so the tree comes from the tie rule alone.  With "the lower position wins" a round merged positions 0 and 1 only,
    the forced round after it halved the array, and below 32 clusters (where one merge is no longer "fewer than a sixteenth") the rest
    went one per round: 25 levels at n = 300, 27 at 1025, and -2 for 5,000 instance boxes (test_tlas_over_hostile_boxes).  Now a
    position whose whole window ties takes its buddy g ^ 1 and every such round pairs the whole array: log2(n) binary levels, which is
    also the depth of the wide tree where all costs tie (nothing widens a node).  The bound asserted is that reasoning plus slack for the
    ragged end, not a measurement."""
    sc = built(vrt, po, gpu_device, bc.family(kind, n), kind, leaf_max, _cap(kind, n))
    if kind in ("huge", "tiny", "subnormal", "point", "line", "dups"):
        assert sc.bvh_info.max_depth <= int(np.ceil(np.log2(n))) + 3


@pytest.mark.parametrize("n", bc.SIZES_SMALL + bc.SIZES_EDGE)
@pytest.mark.parametrize("kind", ["plain", "dups"])
def test_sizes_on_the_hand_offs(vrt, po, gpu_device, kind, n):
    """Around BB_TAIL = 1024 (global rounds / the single-workgroup tail), one item in a last BB_TILE = 256 tile, two read-backs of the
    cluster count (4097); 16 / 17: the smallest meshes the reinsertion runs on."""
    built(vrt, po, gpu_device, bc.family(kind, n), kind, 4, _cap(kind, n))


# ---- b. non-finite input is refused ----
def _raw_build(vrt, dev, tri, leaf_max=4):
    """vxrt_bvh_build on plain buffers: (info, node bytes, tri bytes)."""
    import torch
    n = len(tri)
    t = torch.from_numpy(np.ascontiguousarray(tri, F32)).to(dev)
    nodes = torch.zeros((2 * n - 1) * 52, dtype=torch.uint8, device=dev)
    info = vrt.rtapi.bvh_build(t.data_ptr(), None, n, nodes.data_ptr(), 2 * n - 1, 0, leaf_max, torch.cuda.current_stream().cuda_stream)
    return info, nodes.cpu().numpy()[: info.n_nodes * 52].copy(), t.cpu().numpy().view(np.uint8).reshape(-1).copy()


@pytest.mark.parametrize("n", [300, 1025])
@pytest.mark.parametrize("kind", bc.NON_FINITE)
def test_non_finite_and_overflowing_meshes_are_refused(vrt, gpu_device, kind, n):
    """-1 (not -2, not a tree) for a NaN vertex, a NaN triangle, an infinite coordinate -- the rule of vxrt_accel_refit -- and for finite
    vertices whose extent overflows (no exponent quantises the root); the ordinary build that follows gives its usual bytes."""
    plain = bc.family("plain", n)
    _, want_nodes, want_tri = _raw_build(vrt, gpu_device, plain)
    with pytest.raises(vrt.runtime.VxError, match="returned -1"):
        _raw_build(vrt, gpu_device, bc.family(kind, n))
    _, nodes, tri = _raw_build(vrt, gpu_device, plain)
    assert np.array_equal(nodes, want_nodes) and np.array_equal(tri, want_tri)


def _raw_tlas(vrt, dev, boxes):
    import torch
    n = len(boxes)
    b = torch.from_numpy(np.ascontiguousarray(boxes, F32)).to(dev)
    cap = max(1, 2 * n - 1)
    nodes = torch.zeros(cap * 52, dtype=torch.uint8, device=dev)
    info = vrt.rtapi.tlas_build(b.data_ptr(), n, nodes.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    return info, nodes.cpu().numpy()[: info.n_nodes * 52].copy()


@pytest.mark.parametrize("n", [3, 300, 1025])
def test_a_non_finite_instance_box_is_refused(vrt, gpu_device, n):
    grid = bc.boxes("grid", n)
    _, want = _raw_tlas(vrt, gpu_device, grid)
    with pytest.raises(vrt.runtime.VxError, match="returned -1"):
        _raw_tlas(vrt, gpu_device, bc.boxes("nan_box", n))
    inf = grid.copy()
    inf[n // 3, 3] = np.inf
    with pytest.raises(vrt.runtime.VxError, match="returned -1"):
        _raw_tlas(vrt, gpu_device, inf)
    assert np.array_equal(_raw_tlas(vrt, gpu_device, grid)[1], want)


# ---- c. the scratch arena ----
def scratch_sequence(vrt, dev):
    """release; A; B (60000: the arena grows, every array moves and is left full); A; C (ties everywhere); A; C; release; A.
    Returns {"A": [sha of nodes + tri, ...], "C": [...]}."""
    import hashlib
    sha = lambda r: hashlib.sha256(r[1].tobytes() + r[2].tobytes()).hexdigest()
    a, b, c = bc.family("plain", 1025), bc.family("plain", 60000), bc.family("dups", 4097)
    out = {"A": [], "C": []}
    vrt.rtapi.release_scratch()
    out["A"].append(sha(_raw_build(vrt, dev, a)))
    _raw_build(vrt, dev, b)
    out["A"].append(sha(_raw_build(vrt, dev, a)))
    out["C"].append(sha(_raw_build(vrt, dev, c)))
    out["A"].append(sha(_raw_build(vrt, dev, a)))
    out["C"].append(sha(_raw_build(vrt, dev, c)))
    vrt.rtapi.release_scratch()
    out["A"].append(sha(_raw_build(vrt, dev, a)))
    return out


def _with_triex(vrt, dev, tri):
    """The same through build_on_gpu (shading records reordered alongside): bytes of bvh, tri and triEx."""
    ds = vrt.tracer.DeviceScene.build_on_gpu(tri, _tagged_ex(len(tri)), device=dev, leaf_max=4)
    sc = ds.to_host()
    ds.close()
    return sc["bvh"].tobytes(), sc["tri"].tobytes(), sc["triEx"].tobytes()


def test_a_builds_bytes_do_not_depend_on_what_the_arena_held(vrt, gpu_device):
    """The grow-only arena is never cleared (dec, tile_counts, ri_*, q0 / q1, order): whatever the previous build left there, and whether
    the arena was just allocated, a build gives the same bytes; where every comparison ties (C) nothing may depend on the order in
    which atomics land."""
    out = scratch_sequence(vrt, gpu_device)
    assert len(set(out["A"])) == 1 and len(set(out["C"])) == 1, out
    a, c = bc.family("plain", 1025), bc.family("dups", 4097)
    first = _with_triex(vrt, gpu_device, a)
    c1 = _with_triex(vrt, gpu_device, c)
    vrt.rtapi.release_scratch()
    assert _with_triex(vrt, gpu_device, c) == c1 and _with_triex(vrt, gpu_device, a) == first


def test_the_same_without_reinsertion(vrt, gpu_device):
    """VXRT_BVH_REINSERT is read once per process: the sequence again in a child, on the PLOC tree as it is."""
    code = ("import importlib, json, sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "vrt = importlib.import_module('vortex-raytracing_amd')\nimport test_gpu_bvh_hostile as t\n"
            "print(json.dumps(t.scratch_sequence(vrt, 'cuda:0')))\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, VXRT_BVH_REINSERT="0"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert len(set(out["A"])) == 1 and len(set(out["C"])) == 1, out
    import hashlib
    here = _raw_build(vrt, gpu_device, bc.family("plain", 1025))
    assert out["A"][0] != hashlib.sha256(here[1].tobytes() + here[2].tobytes()).hexdigest()          # (the child really built another tree)


# ---- d. nothing written outside the caller's buffers ----
@pytest.mark.parametrize("tri_offset", [7, 0x0ff00000])
@pytest.mark.parametrize("n", [17, 1025])
def test_nothing_is_written_outside_the_callers_buffers(vrt, gpu_device, n, tri_offset):
    """nodes, tri and triEx are slices in the middle of larger buffers filled with 0xA5, node_capacity is exactly 2 n - 1: after the build
    every guard byte is intact -- around tri / triEx, in front of the nodes, behind node_capacity and in nodes [n_nodes, capacity) -- and
    the leaves carry start + tri_offset."""
    import torch
    tri = bc.family("plain", n)
    ex = _tagged_ex(n)
    g, cap = 64, 2 * n - 1       # guard: 64 records either side
    def guarded(payload, rec):
        buf = np.full((2 * g + len(payload)) * rec, 0xA5, np.uint8)
        buf[g * rec: (g + len(payload)) * rec] = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        return torch.from_numpy(buf).to(gpu_device)
    t_tri, t_ex = guarded(tri, 36), guarded(ex, 64)
    t_nodes = torch.full(((2 * g + cap) * 52,), 0xA5, dtype=torch.uint8, device=gpu_device)
    info = vrt.rtapi.bvh_build(t_tri.data_ptr() + g * 36, t_ex.data_ptr() + g * 64, n, t_nodes.data_ptr() + g * 52, cap, tri_offset, 4,
                               torch.cuda.current_stream().cuda_stream)
    h_tri, h_ex, h_nodes = t_tri.cpu().numpy(), t_ex.cpu().numpy(), t_nodes.cpu().numpy()
    for buf, rec, m in ((h_tri, 36, n), (h_ex, 64, n), (h_nodes, 52, info.n_nodes)):
        assert (buf[: g * rec] == 0xA5).all() and (buf[(g + m) * rec:] == 0xA5).all()
    assert info.n_nodes <= cap
    nodes = h_nodes[g * 52: (g + info.n_nodes) * 52].view(NODE)
    leaf = nodes["ld"] != 0
    first = nodes["lf"][leaf].astype(np.int64) - tri_offset
    cover = np.zeros(n, np.int32)
    for f, c in zip(first, nodes["ld"][leaf]):
        assert 0 <= f and f + c <= n
        cover[f: f + c] += 1
    assert (cover == 1).all()
    out = h_tri[g * 36: (g + n) * 36].view(F32).reshape(n, 9)
    src = h_ex[g * 64: (g + n) * 64].view(F32).reshape(n, 16)[:, 9].astype(np.int64)
    assert np.array_equal(np.sort(src), np.arange(n)) and np.array_equal(_bits(out), _bits(tri[src]))
    # the same tree as at offset 0 in plain buffers, but for the leaves' first triangle
    _, plain_nodes, plain_tri = _raw_build(vrt, gpu_device, tri)
    want = plain_nodes.view(NODE).copy()
    want["lf"][want["ld"] != 0] += np.uint32(tri_offset)
    assert np.array_equal(want.view(np.uint8), nodes.view(np.uint8)) and np.array_equal(plain_tri, h_tri[g * 36: (g + n) * 36])


# ---- e. leaf_max ----
@pytest.mark.parametrize("kind,n", [("plain", 1025), ("dups", 300)])
@pytest.mark.parametrize("leaf_max", [15, 200])
def test_large_leaves(vrt, po, gpu_device, kind, n, leaf_max):
    """leaf_max = 15 is the format's largest leaf, anything above is clamped to it."""
    sc = built(vrt, po, gpu_device, bc.family(kind, n), kind, leaf_max, _cap(kind, n))
    assert sc.bvh_info.max_leaf <= 15
    if leaf_max > 15:
        info, nodes, _ = _raw_build(vrt, gpu_device, bc.family(kind, n), leaf_max)
        assert info.max_leaf <= 15 and np.array_equal(nodes, _raw_build(vrt, gpu_device, bc.family(kind, n), 15)[1])


# ---- f. the TLAS builder ----
def check_tlas(nodes, boxes, info):
    """The format's invariants of a TLAS over `boxes` (check_tree_fast for vxrt_tlas_build): every instance in exactly one leaf with
    ld == i, imask == 1, internal nodes carry UINT32_MAX and >= 2 children in their first slots, stored after their parent, every
    instance box inside the decoded boxes of all its ancestors, depth == info.max_depth < 32, info.bounds exact."""
    n = len(boxes)
    assert len(nodes) == info.n_nodes and (nodes["imask"] == 1).all()
    seen = np.zeros(n, np.int32)
    idx = np.array([0], np.int64)
    lo = np.full((1, 3), -np.inf, F32)
    hi = np.full((1, 3), np.inf, F32)
    depth = n_leaves = 0
    while len(idx):
        nd = nodes[idx]
        leaf = nd["ld"] != INTERNAL
        if leaf.any():
            i = nd["ld"][leaf].astype(np.int64)
            assert (i < n).all() and (nd["lf"][leaf] == 0).all()
            np.add.at(seen, i, 1)
            n_leaves += len(i)
            assert (boxes[i, :3] >= lo[leaf]).all() and (boxes[i, 3:] <= hi[leaf]).all(), "an instance box outside a decoded box of its ancestors"
        inner = ~leaf
        if not inner.any():
            break
        ni, nn = idx[inner], nd[inner]
        valid = nn["ch"][:, :, 0] != 0
        cnt = valid.sum(1)
        assert (cnt >= 2).all() and (valid == (np.arange(4)[None, :] < cnt[:, None])).all(), "children not in the first slots"
        s = np.ldexp(F32(1), nn["e"].astype(np.int32)).astype(F32)
        q = nn["ch"][:, :, 1:].astype(F32)
        clo = nn["o"][:, None, :] + q[:, :, :3] * s[:, None, :]
        chi = nn["o"][:, None, :] + q[:, :, 3:] * s[:, None, :]
        assert (chi >= clo)[valid].all()
        clo = np.maximum(clo, lo[inner][:, None, :])
        chi = np.minimum(chi, hi[inner][:, None, :])
        child = nn["lf"].astype(np.int64)[:, None] + np.arange(4)[None, :]
        assert (child[valid] > np.repeat(ni, cnt)).all() and (child[valid] < len(nodes)).all(), "children must come after their parent"
        idx, lo, hi = child[valid], clo[valid], chi[valid]
        depth += 1
    assert (seen == 1).all() and n_leaves == info.n_leaves == n and info.max_leaf == 1
    assert depth == info.max_depth and depth < 32
    want = np.concatenate([boxes[:, :3].min(0), boxes[:, 3:].max(0)]).astype(F32)
    assert np.array_equal(_bits(np.array(list(info.bounds), F32) + F32(0)), _bits(want + F32(0)))
    return depth


@pytest.mark.parametrize("n", [1, 2, 3, 300, 1025, 5000])
@pytest.mark.parametrize("kind", bc.BOX_KINDS)
def test_tlas_over_hostile_boxes(vrt, gpu_device, kind, n):
    """vxrt_tlas_build itself (build_on_gpu makes its instance boxes on the host in fp64; here the boxes are the input): invariants, and
    node bytes equal to the restatement's for the emitted topology; twice the same bytes."""
    boxes = bc.boxes(kind, n)
    info, raw = _raw_tlas(vrt, gpu_device, boxes)
    nodes = raw.view(NODE)
    depth = check_tlas(nodes, boxes, info)
    print("%s n %d: depth %d, %d nodes" % (kind, n, depth, info.n_nodes))
    assert np.array_equal(rr.refit_tlas_from_boxes(raw, boxes[:, :3], boxes[:, 3:]), raw)
    assert np.array_equal(_raw_tlas(vrt, gpu_device, boxes)[1], raw)


def test_scene_of_coincident_and_nested_instances(vrt, po, gpu_device):
    """300 instances of one 64-triangle mesh all in one place (300 equal boxes; every hit there ties between all of them, and the
    traversal must break the tie as the oracle does) and 300 more each inside the one before, end to end: BLASes, TLAS, accel build and
    the HIP traversal against the oracle on that scene."""
    rng = np.random.default_rng(3)
    base = rng.uniform(-1, 1, size=(64, 9)).astype(F32)
    xf = []
    for i in range(600):
        m = np.eye(4, dtype=F32)
        m[:3, 3] = (220, 100, -60) if i < 300 else (220, 100, 60)
        m[:3, :3] *= F32(40.0) if i < 300 else F32(40.0 - 0.125 * (i - 300))
        xf.append(m)
    ds = vrt.tracer.DeviceScene.build_on_gpu([base] * 600, transforms=xf, device=gpu_device)
    try:
        sc = ds.to_host()
        nodes = sc["tlas"].view(NODE)
        leaves = nodes[nodes["ld"] != INTERNAL]
        assert sorted(leaves["ld"].tolist()) == list(range(600)) and ds.tlas_info.max_depth < 32
        r = np.random.default_rng(3)
        rays = np.concatenate([bc.aimed_rays(r, [180, 60, -100], [260, 140, -20], 128), bc.aimed_rays(r, [180, 60, 20], [260, 140, 100], 128)])
        got = gpu_trace(vrt, ds, rays)
        want, _ = po.trace_canonical(sc, rays)
        assert np.array_equal(_bits(got), _bits(want))
        hit = got["dist"] < 1e29
        who = set(int(b) for b in got["blasIdx"][hit])
        print("%d of %d rays hit, %d distinct instances (%d of the coincident ones)" % (int(hit.sum()), len(rays), len(who), sum(b < 300 for b in who)))
        assert hit.sum() > 20 and len(who) >= 4 and any(b < 300 for b in who) and any(b >= 300 for b in who)
    finally:
        ds.close()
