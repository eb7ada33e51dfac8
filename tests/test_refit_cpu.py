"""CPU: the refit entry points (vxrt_accel_refit / vxrt_accel_set_transforms) exist and refuse a null accel without a device, and the
numpy restatement of the refit (tests/refit_ref.py) turns CPU-built scenes with moved vertices and moved instances into valid trees:
every vertex inside the decoded boxes of its ancestors, every instance's transformed BLAS box inside the decoded TLAS boxes above it."""
import ctypes as C

import numpy as np
import pytest

import refit_ref as rr
from test_scene_builder import NODE, check_tree_fast


def _lib(vrt):
    return C.CDLL(vrt.lib_path("libvortex-hip.so"))


def test_refit_symbols_exported_and_null_accel_refused(vrt):
    L = _lib(vrt)
    L.vxrt_accel_refit.restype = C.c_int
    L.vxrt_accel_refit.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.vxrt_accel_set_transforms.restype = C.c_int
    L.vxrt_accel_set_transforms.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    for what in (0, 1, 2, 3, 4):
        assert L.vxrt_accel_refit(None, what, None) == -1
    assert L.vxrt_accel_set_transforms(None, 0, 1, None, None) == -1
    assert L.vxrt_accel_set_transforms(None, 0, 0, None, None) == -1
    assert vrt.rtapi.REFIT_INSTANCES == 1 and vrt.rtapi.REFIT_GEOMETRY == 2


def _rand_xf(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3] = q @ np.diag(rng.uniform(0.5, 2.0, 3))
    m[:3, 3] = rng.uniform(-50, 50, 3)
    return m.astype(np.float32)


def _blas_ranges(sc):
    rec = np.asarray(sc["blas"], np.uint8).view(np.float32).reshape(-1, rr.BLAS_WORDS)
    bases = np.unique(rec[:, 0].view(np.uint32).astype(np.int64))
    n = len(np.asarray(sc["bvh"]).view(NODE))
    return [(int(b), int(e)) for b, e in zip(bases, list(bases[1:]) + [n])]


def _check_blases(sc):
    """check_tree_fast on every BLAS of a multi-mesh scene: its node range on its own, leaves re-based to its triangles."""
    nodes = np.asarray(sc["bvh"], np.uint8).view(NODE)
    tri = np.asarray(sc["tri"], np.uint8).view(np.float32).reshape(-1, 9)
    for b, e in _blas_ranges(sc):
        sub = nodes[b:e].copy()
        leaf = sub["ld"] != 0
        t0 = int(sub["lf"][leaf].min())
        t1 = int((sub["lf"][leaf].astype(np.int64) + sub["ld"][leaf]).max())
        sub["lf"][leaf] -= t0
        check_tree_fast({"bvh": sub.view(np.uint8).reshape(-1), "tri": np.ascontiguousarray(tri[t0:t1]).view(np.uint8).reshape(-1)})


def _check_tlas_holds(sc, want_lo, want_hi):
    """Every instance's box (want_lo / want_hi [n_blas, 3]) lies inside the decoded boxes of all its TLAS ancestors."""
    tl = np.asarray(sc["tlas"], np.uint8).view(NODE)
    seen = np.zeros(len(want_lo), int)
    stack = [(0, np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32))]
    while stack:
        i, lo, hi = stack.pop()
        n = tl[i]
        assert n["imask"] == 1
        if n["ld"] != rr.TLAS_INTERNAL:
            j = int(n["ld"])
            seen[j] += 1
            assert (want_lo[j] >= lo).all() and (want_hi[j] <= hi).all(), "instance %d outside a TLAS box above it" % j
            continue
        dlo, dhi, pres = rr.decode_children(tl[i:i + 1])
        for k in range(4):
            if pres[0, k]:
                stack.append((int(n["lf"]) + k, np.maximum(lo, dlo[0, k]), np.minimum(hi, dhi[0, k])))
    assert (seen == 1).all()


def _bufs(sc):
    return {k: np.frombuffer(bytes(sc.buffers[k]), np.uint8).copy() for k in ("tlas", "blas", "bvh", "tri")}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restated_refit_of_cpu_built_scenes_holds_the_moved_geometry(vrt, seed):
    rng = np.random.default_rng(seed)
    blob = np.frombuffer(bytes(vrt.scene.procedural("blob", 2, 0, seed).buffers["tri"]), np.float32).reshape(-1, 9)
    meshes = [blob * np.float32(20), (blob[: len(blob) // 2] * np.float32(35)).astype(np.float32), (blob * np.float32(8) + 3).astype(np.float32)]
    sc = vrt.scene.from_triangles(meshes, [np.eye(4, dtype=np.float32)] * len(meshes))
    b = _bufs(sc)
    # vertex jitter + a smooth warp, then the GEOMETRY refit
    tri = b["tri"].view(np.float32).reshape(-1, 3, 3)
    tri += rng.normal(scale=0.3, size=tri.shape).astype(np.float32)
    tri[..., 1] += np.sin(tri[..., 0] * np.float32(0.05)).astype(np.float32) * np.float32(4)
    b["tlas"], b["bvh"] = rr.refit(b, geometry=True)
    _check_blases(b)
    # random instance transforms through the set_transforms restatement, then the INSTANCES refit
    mats = [_rand_xf(rng) for _ in meshes]
    b["blas"] = rr.set_transforms(b["blas"], 0, mats)
    rec = b["blas"].view(np.float32).reshape(-1, rr.BLAS_WORDS)
    assert np.allclose(rec[:, 1:17].reshape(-1, 4, 4) @ np.stack(mats), np.eye(4), atol=1e-4)
    b["tlas"], b["bvh"] = rr.refit(b, geometry=False)
    lo, hi = rr.instance_boxes(b)
    _check_tlas_holds(b, lo, hi)
    # and every transformed vertex (fp64) lies inside its instance's box up to fp32 rounding
    tri_all = b["tri"].view(np.float32).reshape(-1, 3)
    for j, (t0, m) in enumerate(zip(np.cumsum([0] + [len(x) for x in meshes[:-1]]), mats)):
        v = tri_all[3 * t0: 3 * (t0 + len(meshes[j]))].astype(np.float64)
        w = v @ m[:3, :3].T.astype(np.float64) + m[:3, 3]
        tol = 1e-5 * (np.abs(w).max() + 1)
        assert (w >= lo[j] - tol).all() and (w <= hi[j] + tol).all()
    # a refit of what a refit wrote changes nothing (one quantiser, exact min / max)
    t2, b2 = rr.refit(b, geometry=True)
    b["tlas"], b["bvh"] = rr.refit(b, geometry=True)
    assert np.array_equal(t2, b["tlas"]) and np.array_equal(b2, b["bvh"])
    t3, b3 = rr.refit(b, geometry=True)
    assert np.array_equal(t3, b["tlas"]) and np.array_equal(b3, b["bvh"])


def test_restated_refit_refuses_what_the_call_refuses(vrt):
    sc = vrt.scene.from_triangles([np.frombuffer(bytes(vrt.scene.procedural("blob", 1).buffers["tri"]), np.float32).reshape(-1, 9)])
    b = _bufs(sc)
    sing = np.eye(4, dtype=np.float32)
    sing[2, 2] = 0
    with pytest.raises(rr.RefitError):
        rr.set_transforms(b["blas"], 0, [sing])
    nanm = np.eye(4, dtype=np.float32)
    nanm[0, 3] = np.nan
    with pytest.raises(rr.RefitError):
        rr.set_transforms(b["blas"], 0, [nanm])
    b["tri"].view(np.float32)[4] = np.nan
    with pytest.raises(rr.RefitError):
        rr.refit(b, geometry=True)


def test_quantiser_and_inverse_restatement():
    # the exponent rule: smallest e with extent / 255 <= 2^e
    ext = np.array([255.0, 256.0, 1.0, 0.0, -1.0, 1e-30, 3e38, 510.0], np.float32)
    e = rr.pick_exp(ext)
    assert list(e[[0, 1, 3, 4, 7]]) == [0, 1, 0, 0, 1]
    ok = (ext > 0) & (ext < 3e38)
    assert (ext[ok] / 255 <= np.ldexp(1.0, e[ok])).all() and (ext[ok] / 255 > np.ldexp(1.0, e[ok] - 1)).all()
    # quantised boxes are conservative after the decode's rounding
    rng = np.random.default_rng(5)
    org = rng.uniform(-100, 100, 500).astype(np.float32)
    a = (org + rng.uniform(0, 50, 500)).astype(np.float32)
    bb = (a + rng.uniform(0, 50, 500)).astype(np.float32)
    e0 = rr.pick_exp((bb - org).astype(np.float32))
    pres = np.zeros((500, 4), bool)
    pres[:, 0] = True
    cmin = np.zeros((500, 4), np.float32)
    cmax = np.zeros((500, 4), np.float32)
    cmin[:, 0], cmax[:, 0] = a, bb
    e1, ql, qh, good = rr.quant_children(org, e0, cmin, cmax, pres)
    assert good.all()
    s = np.ldexp(np.float32(1), e1).astype(np.float32)
    assert ((org + ql[:, 0].astype(np.float32) * s) <= a).all() and ((org + qh[:, 0].astype(np.float32) * s) >= bb).all()
    # MESA inverse
    m = np.stack([_rand_xf(np.random.default_rng(i)) for i in range(20)])
    inv, det = rr.inverted(m.reshape(-1, 16))
    assert (det != 0).all()
    assert np.allclose(inv.reshape(-1, 4, 4), np.linalg.inv(m.astype(np.float64)), atol=1e-4)
