"""GPU: the refit under hostile motion and unusual topology.  Geometry refits that move boxes across many exponents (a mesh flown far
away, collapsed to a point or a plane, permuted vertices, a mirror, the whole scene scaled by 1e-30 or 2e35 or 1e7 away, an overflowing vertex
pair), on trees from both builders and a fixture; a BLAS shared by several instances; leaf-root BLASes; thousands of instances; a
long seeded chain of refits with failures in it; what == 0; an internal node without a child.  After every refit the buffers hold
the bytes of the numpy restatement (tests/refit_ref.py), and the accel traces as a fresh build, the oracle and (small scenes) a
brute-force loop over every triangle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import refit_ref as rr
from builder_cases import aimed_rays as _aimed_rays
from test_gpu_refit import KEYS, W, H, _agrees_with_fresh_and_oracle, _blob, _host, _put_tri, _render, _stream, _trace
from test_refit_cpu import _blas_ranges, _check_blases
from test_scene_builder import NODE, brute_force

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _lib(vrt):
    L = vrt.rtapi._lib()
    L.vxrt_accel_refit.restype = C.c_int
    L.vxrt_accel_refit.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.vxrt_render.restype = C.c_int
    return L


def _render_rc(vrt, ds):
    """vxrt_render's return code and the framebuffer it left (filled with a marker first)."""
    import torch
    px = torch.full((H, W), 0x5A5A5A, dtype=torch.int32, device=ds.t["tri"].device)
    rc = _lib(vrt).vxrt_render(ds.accel, W, H, 0, H, C.byref(vrt.rtapi.default_shade_params()), 1, px.data_ptr(), None, None, None,
                                _stream())
    assert vrt.rtapi.status(_stream()) == 0
    return rc, px.cpu().numpy()


def _tri_ranges(b):
    """Triangle range [t0, t1) of every distinct BLAS."""
    nodes = b["bvh"].view(NODE)
    out = []
    for lo, hi in _blas_ranges(b):
        sub = nodes[lo:hi]
        leaf = sub["ld"] != 0
        out.append((int(sub["lf"][leaf].min()), int((sub["lf"][leaf].astype(np.int64) + sub["ld"][leaf]).max())))
    return out


# -------------------------------------------------------------------------------------------------------------------------------
# scenes
# -------------------------------------------------------------------------------------------------------------------------------
def _small_meshes(vrt):
    tiny = np.array([[0, 0, 0, 6, 0, 1, 0, 7, 2], [6, 0, 1, 6, 7, 3, 0, 7, 2]], F32) + F32(300)
    return [_blob(vrt, 40, (260, 100, -60), 2), _blob(vrt, 25, (240, 110, 55), 1), tiny]


def _scene(vrt, golden, dev, how):
    """(DeviceScene, brute-forceable: identity transforms and few triangles)."""
    if how == "teapot_x3":
        g = golden("teapot_x3")
        return vrt.tracer.DeviceScene({k: g[k] for k in KEYS}, dev), False
    meshes = _small_meshes(vrt)
    if how == "cpu":
        return vrt.tracer.DeviceScene(vrt.scene.from_triangles(meshes, [np.eye(4, dtype=F32)] * len(meshes)), dev), True
    return vrt.tracer.DeviceScene.build_on_gpu(meshes, device=dev, leaf_max=1 if how == "gpu1" else 4), True


def _move(case, b, rng):
    """New vertices in b["tri"] for one hostile case; returns the world box (lo, hi) the rays aim at."""
    v = b["tri"].view(F32).reshape(-1, 3, 3)
    t0, t1 = _tri_ranges(b)[0]
    allv = v.reshape(-1, 3)
    ext = float(np.ptp(allv, 0).max())
    m = v[t0:t1]
    if case == "fly":
        m += F32(100 * ext)
    elif case == "point":
        m[...] = m.reshape(-1, 3).mean(0).astype(F32)
    elif case == "plane":
        m[..., 2] = F32(m[..., 2].mean())
    elif case == "permute":
        flat = v.reshape(-1, 3)
        flat[...] = flat[rng.permutation(len(flat))]
    elif case == "mirror":
        c = F32((allv[:, 0].min() + allv[:, 0].max()) / 2)
        v[..., 0] = (F32(2) * c - v[..., 0]).astype(F32)
    elif case == "tiny":
        v *= F32(1e-30)
    elif case == "huge":
        v[...] = ((v - allv.mean(0)) * F32(2e35)).astype(F32)           # (about its centre: extents ~1e37 to 1e38, still finite)
    elif case == "offset":
        v += F32(1e7)
    return None


CASES = ["fly", "point", "plane", "permute", "mirror", "tiny", "huge", "offset"]


def _refit_and_check(vrt, po, ds, b, rng, brute, geometry=True):
    """Put b's vertices, refit, compare with the restatement; then fresh accel + oracle on rays at every instance, brute force."""
    _put_tri(ds, b["tri"])
    try:
        want_tlas, want_bvh = rr.refit(b, geometry=geometry)
    except rr.RefitError:                                               # (refused alike: the caller restores)
        with pytest.raises(Exception):
            ds.refit(geometry=geometry)
        return None
    ds.refit(geometry=geometry)
    got = _host(ds)
    assert np.array_equal(got["bvh"], want_bvh)
    assert np.array_equal(got["tlas"], want_tlas)
    _check_blases(got)
    wl, wh = rr.instance_boxes(got)
    rays = np.concatenate([_aimed_rays(rng, wl[j], wh[j], 24) for j in range(min(len(wl), 4))] + [_aimed_rays(rng, wl.min(0), wh.max(0), 24)])
    _agrees_with_fresh_and_oracle(vrt, po, ds, rays)
    if brute:
        d = _trace(vrt, ds.accel, ds.t["tri"].device, rays)["dist"]
        bf = brute_force(ds.to_host(), rays, po)
        # equal, but where coplanar overlapping triangles (a collapsed mesh) put two hits within an ulp or two of each other: the
        # reference's traversal may skip the box of the nearer one by its slab distance (the oracle agrees with the GPU above)
        assert np.array_equal(d < 1e29, bf < 1e29)
        assert (np.abs(d - bf) <= 2 * np.spacing(bf)).all() and (d == bf).mean() >= 0.95
    return got


@pytest.mark.parametrize("how", ["gpu1", "gpu4", "cpu", "teapot_x3"])
@pytest.mark.parametrize("case", CASES)
def test_hostile_geometry(vrt, po, golden, gpu_device, how, case):
    ds, brute = _scene(vrt, golden, gpu_device, how)
    rng = np.random.default_rng(17 * CASES.index(case) + len(how))
    b0 = _host(ds)
    rest_tlas, rest_bvh = rr.refit(b0, geometry=True)
    if how.startswith("gpu"):
        assert np.array_equal(rest_bvh, b0["bvh"])                     # the builder's bytes are the refit's
    b = {k: v.copy() for k, v in b0.items()}
    _move(case, b, rng)
    _refit_and_check(vrt, po, ds, b, rng, brute)
    # back to the rest pose: the rest bytes again
    b = {k: v.copy() for k, v in b0.items()}
    got = _refit_and_check(vrt, po, ds, b, rng, brute)
    assert np.array_equal(got["bvh"], rest_bvh) and np.array_equal(got["tlas"], rest_tlas)
    ds.close()


@pytest.mark.parametrize("how", ["gpu1", "cpu", "teapot_x3"])
def test_overflowing_extent_fails_stale_and_recovers(vrt, po, golden, gpu_device, how):
    ds, brute = _scene(vrt, golden, gpu_device, how)
    b0 = _host(ds)
    rest_tlas, rest_bvh = rr.refit(b0, geometry=True)
    bad = b0["tri"].copy()
    v = bad.view(F32).reshape(-1, 3, 3)
    v[5, 0, 0], v[6, 1, 0] = F32(-3e38), F32(3e38)                    # one vertex pair: the extent overflows fp32
    with pytest.raises(rr.RefitError):
        rr.refit(dict(b0, tri=bad), geometry=True)
    _put_tri(ds, bad)
    with pytest.raises(Exception):
        ds.refit(geometry=True)
    rc, px = _render_rc(vrt, ds)
    assert rc == -1 and (px == 0x5A5A5A).all()                         # stale: refused, the pixels untouched
    with pytest.raises(Exception):                                      # (a stale accel redoes the BLAS boxes: still the bad vertices)
        ds.set_transforms([b0["blas"].view(F32).reshape(-1, rr.BLAS_WORDS)[0, 17:33].reshape(4, 4)])
    _put_tri(ds, b0["tri"])
    ds.refit(geometry=True)
    got = _host(ds)
    assert np.array_equal(got["bvh"], rest_bvh) and np.array_equal(got["tlas"], rest_tlas)
    if how == "gpu1":
        assert np.array_equal(got["bvh"], b0["bvh"])
    assert _render_rc(vrt, ds)[0] == 0
    _agrees_with_fresh_and_oracle(vrt, po, ds)
    ds.close()


def test_quantiser_edges_on_the_gpu(vrt, po, gpu_device):
    """Boxes that need the two corner cases of the quantiser: node extents of exactly 255 * 2^k (bb_pick_exp's power-of-two branch)
    and a child whose lo plane only stays conservative through the --lo correction (c - o rounds up onto 128 * 2^e)."""
    rng = np.random.default_rng(3)
    grid = _blob(vrt, 1, (0, 0, 0), 2).reshape(-1, 3, 3).astype(np.float64)
    grid = np.round((grid - grid.min((0, 1))) / np.ptp(grid, (0, 1)) * 255).astype(F32)              # integers spanning [0, 255]
    grid[..., 1] *= F32(2)
    o = np.nextafter(F32(-128), F32(0))                                 # 2^-17 above -128
    c = F32(0.75) * F32(2.0 ** -17)
    cancel = np.array([[o, 0, 0, 72, 0, 1, 72, 1, 0], [c, 0, 0, c + 1, 0, 1, c + 1, 1, 0]], F32)
    ds = vrt.tracer.DeviceScene.build_on_gpu([grid.reshape(-1, 9), cancel], device=gpu_device, leaf_max=1)
    b0 = _host(ds)
    nodes = b0["bvh"].view(NODE)
    assert (nodes["e"][0] == [0, 1, 0]).all()                          # root of the grid mesh: extents 255, 510, 255
    r1 = _blas_ranges(b0)[1][0]
    assert sorted(nodes["ch"][r1, :2, 1].tolist()) == [0, 127]          # the cancelling child: 128 corrected to 127
    want_tlas, want_bvh = rr.refit(b0, geometry=True)
    assert np.array_equal(want_bvh, b0["bvh"])
    for step in range(3):
        b = {k: v.copy() for k, v in b0.items()}
        v = b["tri"].view(F32).reshape(-1, 3, 3)
        v[:len(grid)] = np.round(v[:len(grid)] * F32(2 ** step) + F32(rng.integers(-4, 4) * 255)).astype(F32)
        _refit_and_check(vrt, po, ds, b, rng, True)
    ds.close()


# -------------------------------------------------------------------------------------------------------------------------------
# topology
# -------------------------------------------------------------------------------------------------------------------------------
def test_shared_blas(vrt, po, golden, gpu_device):
    """Three instances of one BLAS (teapot_x3's first tree, every record at offset 0, their own transforms)."""
    g = golden("teapot_x3")
    b = {k: np.array(g[k]).copy() for k in KEYS}
    rec = b["blas"].view(F32).reshape(-1, rr.BLAS_WORDS)
    offs = rec[:, 0].view(np.uint32)
    end = int(sorted(offs)[1])
    b["bvh"] = b["bvh"][: end * 52].copy()
    offs[:] = 0
    b["tlas"], _ = rr.refit(b, geometry=False)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    _agrees_with_fresh_and_oracle(vrt, po, ds, g["rays"])
    rng = np.random.default_rng(5)
    t1 = _tri_ranges(b)[0][1]
    for step in range(3):
        h = _host(ds)
        v = h["tri"].view(F32).reshape(-1, 3, 3)
        v[:t1] += rng.normal(scale=0.05, size=v[:t1].shape).astype(F32)
        v[: t1 // 3] += F32(3 * step)                                   # one subtree's triangles fly off
        _refit_and_check(vrt, po, ds, h, rng, False)
        mats = [rec[i, 17:33].reshape(4, 4).copy() for i in range(3)]
        for m in mats:
            m[:3, 3] += rng.uniform(-2, 2, 3).astype(F32)
        h = _host(ds)
        want_blas = rr.set_transforms(h["blas"], 0, mats)
        want_tlas, _ = rr.refit(dict(h, blas=want_blas), geometry=False)
        ds.set_transforms(mats)
        got = _host(ds)
        assert np.array_equal(got["blas"], want_blas) and np.array_equal(got["tlas"], want_tlas)
        _agrees_with_fresh_and_oracle(vrt, po, ds, g["rays"])
    ds.close()


def _leaf_root_scene(vrt, dev):
    rng = np.random.default_rng(9)
    meshes = []
    for i in range(6):
        k = i % 4 + 1
        t = (rng.normal(size=(k, 9)) * 4 + np.tile([230 + 20 * i, 60, -40 + 15 * i], 3)).astype(F32)
        meshes.append(t)
    meshes += [_blob(vrt, 30, (260, 90, 0), 2), _blob(vrt, 20, (300, 40, 60), 1)]
    return vrt.tracer.DeviceScene.build_on_gpu(meshes, device=dev, leaf_max=4)


def test_leaf_root_blases(vrt, po, gpu_device):
    ds = _leaf_root_scene(vrt, gpu_device)
    b = _host(ds)
    nodes = b["bvh"].view(NODE)
    roots = b["blas"].view(F32).reshape(-1, rr.BLAS_WORDS)[:, 0].view(np.uint32)
    assert (nodes["ld"][roots] != 0).sum() >= 4                        # leaf roots, under an internal-root BLAS or two
    rng = np.random.default_rng(13)
    for step in range(4):
        mats = []
        for j in range(len(roots)):
            m = np.eye(4, dtype=F32)
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            m[:3, :3] = q * rng.uniform(0.5, 1.5)
            m[:3, 3] = rng.uniform(-10, 10, 3) + (np.eye(3) - m[:3, :3]) @ np.array([260, 80, 0])
            mats.append(m)
        h = _host(ds)
        want_blas = rr.set_transforms(h["blas"], 0, mats)
        want_tlas, _ = rr.refit(dict(h, blas=want_blas), geometry=False)
        ds.set_transforms(mats)
        got = _host(ds)
        assert np.array_equal(got["blas"], want_blas) and np.array_equal(got["tlas"], want_tlas)
        wl, wh = rr.instance_boxes(got)
        rays = np.concatenate([_aimed_rays(rng, wl[j], wh[j], 16) for j in range(6)])
        _agrees_with_fresh_and_oracle(vrt, po, ds, rays)
        h = _host(ds)
        v = h["tri"].view(F32).reshape(-1, 3, 3)
        v += rng.normal(scale=0.5, size=v.shape).astype(F32)
        _refit_and_check(vrt, po, ds, h, rng, False)
    ds.close()


def test_many_instances(vrt, po, gpu_device):
    """2,400 instances: the TLAS leaves and its lowest levels span several 256-thread blocks."""
    n = 2400
    base = _blob(vrt, 1, (0, 0, 0), 0)
    rng = np.random.default_rng(21)
    xf = []
    for i in range(n):
        m = np.eye(4, dtype=F32)
        m[:3, 3] = (230 + 1.5 * (i % 40), 20 + 1.5 * (i // 40 % 60), -40 + rng.uniform(0, 80))
        xf.append(m)
    ds = vrt.tracer.DeviceScene.build_on_gpu([base] * n, device=gpu_device, transforms=xf)
    b = _host(ds)
    tl = b["tlas"].view(NODE)
    _, levels = rr._walk(tl, [0], [0], tlas=True)
    assert max(len(ii) for ii, _ in levels) > 256
    for step in range(4):
        first = int(rng.integers(1, n // 2))
        count = int(rng.integers(300, n - first))
        mats = []
        for i in range(first, first + count):
            m = xf[i].copy()
            m[:3, 3] += rng.uniform(-3, 3, 3).astype(F32)
            m[:3, :3] *= F32(rng.uniform(0.7, 1.3))
            mats.append(m)
        want_blas = rr.set_transforms(b["blas"], first, mats)
        want_tlas, _ = rr.refit(dict(b, blas=want_blas), geometry=False)
        ds.set_transforms(mats, first=first)
        got = _host(ds)
        assert np.array_equal(got["blas"], want_blas) and np.array_equal(got["tlas"], want_tlas), step
        b = got
    _agrees_with_fresh_and_oracle(vrt, po, ds)
    h = _host(ds)
    h["tri"].view(F32)[:] += rng.normal(scale=0.01, size=h["tri"].size // 4).astype(F32)
    _refit_and_check(vrt, po, ds, h, rng, False)
    ds.close()


def test_refit_chain(vrt, po, gpu_device):
    """40 seeded steps: set_transforms on random subsets, geometry refits, INSTANCES | GEOMETRY, refused matrices, a NaN vertex that
    leaves the accel stale until it is restored.  The bytes follow the restatement chained from the previous expected state."""
    ds = _leaf_root_scene(vrt, gpu_device)
    L = _lib(vrt)
    rest = _host(ds)
    b = {k: v.copy() for k, v in rest.items()}
    nb = len(b["blas"]) // 160
    rng = np.random.default_rng(40)
    for step in range(40):
        op = int(rng.integers(0, 5))
        if op == 0:
            first = int(rng.integers(0, nb))
            count = int(rng.integers(1, nb - first + 1))
            mats = []
            for _ in range(count):
                m = np.eye(4, dtype=F32)
                q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
                m[:3, :3] = q * rng.uniform(0.3, 3)
                m[:3, 3] = rng.uniform(-30, 30, 3)
                mats.append(m)
            b["blas"] = rr.set_transforms(b["blas"], first, mats)
            b["tlas"], _ = rr.refit(b, geometry=False)
            ds.set_transforms(mats, first=first)
        elif op in (1, 2):
            v = b["tri"].view(F32).reshape(-1, 3, 3)
            v += rng.normal(scale=float(rng.choice([0.01, 1, 20])), size=v.shape).astype(F32)
            _put_tri(ds, b["tri"])
            b["tlas"], b["bvh"] = rr.refit(b, geometry=True)
            if op == 1:
                ds.refit(geometry=True)
            else:
                vrt.rtapi.accel_refit(ds.accel, vrt.rtapi.REFIT_INSTANCES | vrt.rtapi.REFIT_GEOMETRY, _stream())
        elif op == 3:
            sing = np.eye(4, dtype=F32)
            sing[int(rng.integers(0, 3)), :3] = 0
            j = int(rng.integers(0, nb))
            with pytest.raises(Exception):
                ds.set_transforms([np.eye(4, dtype=F32)] * int(rng.integers(0, nb - j)) + [sing], first=j)
            b["tlas"], _ = rr.refit(b, geometry=False)                  # the records as they were, the instance pass redone
        else:
            bad = b["tri"].copy()
            bad.view(F32)[int(rng.integers(0, bad.size // 4))] = np.nan
            _put_tri(ds, bad)
            with pytest.raises(Exception):
                ds.refit(geometry=True)
            assert _render_rc(vrt, ds)[0] == -1
            assert L.vxrt_accel_refit(ds.accel, 0, _stream()) == -1      # what == 0 on a stale accel
            _put_tri(ds, b["tri"])
            b["tlas"], b["bvh"] = rr.refit(b, geometry=True)
            ds.refit(geometry=False)                                     # (stale: the BLAS boxes are redone as well)
        got = _host(ds)
        for k in ("tlas", "bvh", "blas"):
            assert np.array_equal(got[k], b[k]), (step, op, k)
        if step % 8 == 7:
            wl, wh = rr.instance_boxes(got)
            _agrees_with_fresh_and_oracle(vrt, po, ds, _aimed_rays(rng, wl.min(0), wh.max(0), 48))
    _put_tri(ds, rest["tri"])
    ds.refit(geometry=True)
    assert np.array_equal(_host(ds)["bvh"], rest["bvh"])
    ds.close()


def test_what_zero_moves_nothing(vrt, po, gpu_device):
    ds = _leaf_root_scene(vrt, gpu_device)
    L = _lib(vrt)
    b = _host(ds)
    moved = b["tri"].copy()
    moved.view(F32)[:] += F32(5)
    _put_tri(ds, moved)
    rec = b["blas"].view(F32).reshape(-1, rr.BLAS_WORDS).copy()
    rec[:, 20] += F32(7)                                                # a translation written into the records behind the API's back
    import torch
    ds.t["blas"].copy_(torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(gpu_device))
    assert L.vxrt_accel_refit(ds.accel, 0, _stream()) == 0
    got = _host(ds)
    assert np.array_equal(got["tlas"], b["tlas"]) and np.array_equal(got["bvh"], b["bvh"])
    ds.close()


def test_internal_node_without_a_child_is_refused(vrt, po, golden, gpu_device):
    """A hand-built BLAS with one internal node whose four child slots are empty: the refit refuses the tree before writing (-1, the
    accel not stale), as the restatement does."""
    meshes = _small_meshes(vrt)
    sc = vrt.scene.from_triangles(meshes, [np.eye(4, dtype=F32)] * len(meshes))
    b = {k: np.frombuffer(bytes(sc.buffers[k]), np.uint8).copy() for k in KEYS}
    nodes = b["bvh"].view(NODE)
    root = int(b["blas"].view(F32).reshape(-1, rr.BLAS_WORDS)[0, 0].view(np.uint32))
    kid = root + int(nodes["lf"][root])
    inner = [kid + k for k in range(4) if nodes["ch"][root, k, 0] and nodes["ld"][kid + k] == 0]
    assert inner
    nodes["ch"][inner[0]] = 0                                           # no child at all
    for geometry in (True, False):
        with pytest.raises(rr.RefitError):
            rr.refit(b, geometry=geometry)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    L = _lib(vrt)
    before = _host(ds)
    for what in (vrt.rtapi.REFIT_GEOMETRY, vrt.rtapi.REFIT_INSTANCES, 3, 0):
        assert L.vxrt_accel_refit(ds.accel, what, _stream()) == -1
    with pytest.raises(Exception):
        ds.set_transforms([np.eye(4, dtype=F32)])
    after = _host(ds)
    for k in KEYS:
        assert np.array_equal(after[k], before[k]), k
    assert _render_rc(vrt, ds)[0] == 0                                  # not stale
    _agrees_with_fresh_and_oracle(vrt, po, ds)
    ds.close()


def test_refit_stress_on_the_lds_staging_variant(vrt, gpu_device):
    """The cases above on the library that stages the top of the tree in LDS (the image is re-staged after every refit)."""
    import importlib
    bld = importlib.import_module("vortex-raytracing_amd.build")
    d = bld.build_test_variant()
    env = dict(os.environ, VXRT_LIB_DIR=d, VXRT_DEBUG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k",
                        "not lds_staging and (gpu4 or teapot_x3 or shared or leaf_root or many or chain or edges)"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1500:])
    assert " passed" in r.stdout and "top-of-tree nodes staged" in (r.stdout + r.stderr)
