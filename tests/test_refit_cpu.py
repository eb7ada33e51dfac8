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


# ------------------------------------------------------------------------------------------------------------------------------
# The quantiser under hostile boxes, against an exact reference on fractions.Fraction
# ------------------------------------------------------------------------------------------------------------------------------
from fractions import Fraction

F32 = np.float32


def _exact_exp(x):
    """Smallest integer e with x <= 2^e, for a Fraction x > 0."""
    e = x.numerator.bit_length() - x.denominator.bit_length()
    while x > Fraction(2) ** e:
        e += 1
    while x <= Fraction(2) ** (e - 1):
        e -= 1
    return e


def _hostile_nodes(rng, n):
    """n single-axis nodes: origin = the min of the present children's lo (as the refit takes it), child boxes cmin / cmax [n, 4],
    present [n, 4].  Each node is drawn from one family of hostile boxes."""
    fam = rng.integers(0, 9, n)
    k = rng.integers(-149 + 8, 120, n)                                  # 255 * 2^k is an fp32 for k >= -141
    base = np.zeros(n, np.float64)
    ext = np.zeros(n, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        # 0: extents 255 * 2^k exactly (extent / 255 a power of two), origin +-0;  1: the same +-1 ulp
        p2 = np.ldexp(255.0, k).astype(F32)
        ext = np.where(fam == 0, p2, ext)
        ext = np.where(fam == 1, np.where(rng.random(n) < 0.5, np.nextafter(p2, F32(np.inf)), np.nextafter(p2, F32(0))), ext)
        base = np.where(fam <= 1, np.where(rng.random(n) < 0.5, 0.0, -0.0), base)
        # 2: large origins, tiny extents (1e7 with 1e-3: the decode cancels)
        base = np.where(fam == 2, rng.choice([-1, 1], n) * 10 ** rng.uniform(6, 8, n), base)
        ext = np.where(fam == 2, 10 ** rng.uniform(-4, 0.5, n), ext)
        # 3: subnormal origins and extents;  4: extents at the -126 clamp (normal origin near the smallest normal)
        base = np.where(fam == 3, rng.uniform(-1, 1, n) * 2.0 ** -130, base)
        ext = np.where(fam == 3, rng.uniform(0, 1, n) * 2.0 ** rng.integers(-149, -126, n), ext)
        base = np.where(fam == 4, rng.uniform(-4, 4, n) * 2.0 ** -126, base)
        ext = np.where(fam == 4, 255 * rng.uniform(0.25, 2, n) * 2.0 ** -126, ext)
        # 5: extents above 3e38 (bb_pick_exp starts at 0, the bump loop climbs to ~120);  6: extents that overflow fp32
        base = np.where(fam == 5, -1.7e38, base)
        ext = np.where(fam == 5, rng.uniform(3.05e38, 3.4e38, n), ext)
        base = np.where(fam == 6, -rng.uniform(2.5e38, 3.4e38, n), base)
        ext = np.where(fam == 6, rng.uniform(5.5e38, 6.8e38, n), ext)
        # 7: every magnitude;  8: the node box itself of width 0 (a point)
        base = np.where(fam == 7, rng.normal(size=n) * 10.0 ** rng.uniform(-30, 30, n), base)
        ext = np.where(fam == 7, 10.0 ** rng.uniform(-35, 35, n), ext)
        base = np.where(fam == 8, rng.normal(size=n) * 100, base)
        u0 = rng.random((n, 4))
        u1 = rng.random((n, 4))
        lo = base[:, None] + u0 * ext[:, None]
        hi = lo + u1 * (base[:, None] + ext[:, None] - lo)
        lo, hi = np.minimum(lo, 3.4e38).astype(F32), np.minimum(hi, 3.4e38).astype(F32)
        kind = rng.integers(0, 5, (n, 4))
        hi = np.where(kind == 0, lo, hi)                                     # point children
        whole = kind == 1                                                    # children equal to the node box
        lo = np.where(whole, F32(base[:, None]), lo)
        hi = np.where(whole, np.minimum(base + ext, 3.4e38).astype(F32)[:, None], hi)
        lo[:, 0] = F32(base)                                                 # one child on the node's lo plane (+-0 kept)
        hi[:, 0] = np.where(fam <= 1, np.minimum(base + ext, 3.4e38).astype(F32), hi[:, 0])
        hi = np.where(fam[:, None] == 8, lo, hi)
        lo = np.where(fam[:, None] == 8, F32(base[:, None]), lo)
        hi = np.where(fam[:, None] == 8, lo, hi)
    # 9: cancellation: origin o = the fp32 just above -2^(e+7), a child's lo plane c = 0.75 ulp(o) above 0, so c - o rounds up onto
    # 128 * 2^e and the decode o + 128 * 2^e = ulp(o) > c: only the quantiser's lo correction keeps that child conservative
    fam = np.where(rng.random(n) < 0.1, 9, fam)
    c9 = fam == 9
    e9 = rng.integers(-100, 100, n)
    o9 = np.nextafter(-np.ldexp(F32(1), e9 + 7).astype(F32), F32(0))
    d9 = (np.ldexp(F32(1), e9 + 7).astype(F32) + o9).astype(F32)             # ulp(o), exact
    lo = np.where(c9[:, None], (F32(0.75) * d9)[:, None], lo)
    hi = np.where(c9[:, None], (lo + np.ldexp(F32(1), e9)[:, None] * rng.uniform(0, 40, (n, 4))).astype(F32), hi)
    lo[c9, 0], hi[c9, 0] = o9[c9], (o9 + np.ldexp(F32(200), e9).astype(F32))[c9]
    present = rng.random((n, 4)) < 0.7
    present[:, 0] = True
    present[c9, 1] = True
    hi = np.maximum(hi, lo)
    origin = np.where(present, lo, F32(np.inf)).min(1).astype(F32)
    top = np.where(present, hi, F32(-np.inf)).max(1).astype(F32)
    return fam, origin, top, lo.astype(F32), hi.astype(F32), present


def test_pick_exp_against_exact_powers_of_two():
    rng = np.random.default_rng(17)
    k = np.arange(-141, 121)
    p2 = np.ldexp(255.0, k).astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        ext = np.concatenate([p2, np.nextafter(p2, F32(np.inf)), np.nextafter(p2, F32(0)),
                              (10.0 ** rng.uniform(-45, 38.5, 20000)).astype(F32), np.array([1e-45, 3e-45, 1e-43, 2e-43, 3.5e-43], F32)])
    ext = ext[(ext > 0) & (ext <= F32(3e38))]
    got = rr.pick_exp(ext)
    for x, g in zip(ext.tolist(), got.tolist()):
        # exact, the fp32 quotient notwithstanding: no fp32 lies in (255 * 2^k, 255 * 2^k * (1 + 2^-24)], so a rounded quotient never
        # lands on a power of two from above; a quotient that underflows (to a subnormal or to 0) is at the clamp either way
        assert g == max(-126, min(126, _exact_exp(Fraction(x) / 255))), x
    # the power-of-two branch itself: 255 * 2^k -> k, one ulp above -> k + 1, one below -> k
    kk = (k >= -126) & (k <= 119)                                          # (255 * 2^120 > 3e38: no exponent picked)
    with np.errstate(under="ignore"):
        assert (rr.pick_exp(p2[kk]) == k[kk]).all() and (rr.pick_exp(np.nextafter(p2[kk], F32(np.inf))) == k[kk] + 1).all()
        assert (rr.pick_exp(np.nextafter(p2[kk], F32(0))) == k[kk]).all()
    assert rr.pick_exp(np.array([1e-45, 0.0, -0.0, -1.0, np.inf, np.nan, 3.1e38], F32)).tolist() == [-126, 0, 0, 0, 0, 0, 0]


def test_quantiser_against_an_exact_reference():
    """rr.quant_children on 25,000 hostile nodes (10^5 child boxes): conservative fp32 decodes; where every decode is exact, q within
    one of the exact floor / ceil and e the smallest exponent that fits or one more; ok false exactly when no exponent fits."""
    rng = np.random.default_rng(2024)
    n = 25000
    fam, origin, top, cmin, cmax, present = _hostile_nodes(rng, n)
    with np.errstate(over="ignore", invalid="ignore"):
        e0 = rr.pick_exp((top - origin).astype(F32))
    e, ql, qh, ok = rr.quant_children(origin, e0, np.where(present, cmin, 0), np.where(present, cmax, 0), present)
    assert ((e >= -126) & (e <= 126)).all() and (e >= e0).all()
    # no exponent fits where some child's distance from the origin overflows fp32 (the quantiser's arithmetic is fp32): with a finite
    # distance D, 2^126 * 255 > D always fits
    with np.errstate(over="ignore", invalid="ignore"):
        reach = np.isfinite(np.where(present, (cmax - origin[:, None]).astype(F32), 0)).all(1)
    assert np.array_equal(ok, reach)
    assert (~ok).sum() > 1000 and ok[fam == 6].sum() > 0          # (family 6 overflows unless its far children are absent)
    # conservative after the decode's own rounding (origin + q * 2^e in fp32)
    s = np.ldexp(F32(1), e).astype(F32)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        dlo = (origin[:, None] + (ql.astype(F32) * s).astype(F32)).astype(F32)
        dhi = (origin[:, None] + (qh.astype(F32) * s).astype(F32)).astype(F32)
    m = present & ok[:, None]
    assert (dlo <= cmin)[m].all() and (dhi >= cmax)[m].all()
    assert ((ql >= 0) & (ql <= qh) & (qh <= 255))[m].all()
    assert (ql[~present] == 0).all() and (qh[~present] == 0).all()
    # the exact reference
    checked = bumped = 0
    for i in np.flatnonzero(ok).tolist():
        o = Fraction(float(origin[i]))
        sc = Fraction(2) ** int(e[i])
        kids = np.flatnonzero(present[i]).tolist()
        exact = np.isfinite(dhi[i, kids]).all() and all(Fraction(float(dlo[i, c])) == o + int(ql[i, c]) * sc and Fraction(float(dhi[i, c])) == o + int(qh[i, c]) * sc for c in kids)
        if not exact:
            continue
        checked += 1
        far = max(Fraction(float(cmax[i, c])) - o for c in kids)
        if far == 0:
            assert e[i] == 0                                                 # a flat node: e = 0, as both builders write it
        else:
            estar = max(-126, _exact_exp(far / 255))                        # smallest e with every ceil((cmax - o) / 2^e) <= 255
            assert int(e[i]) in (estar, estar + 1), (i, int(fam[i]), int(e[i]), estar)
        bumped += int(e[i]) > int(e0[i])
        for c in kids:
            fl = (Fraction(float(cmin[i, c])) - o) / sc
            fh = (Fraction(float(cmax[i, c])) - o) / sc
            fl_i, fh_i = fl.numerator // fl.denominator, -((-fh.numerator) // fh.denominator)
            assert fl_i - 1 <= int(ql[i, c]) <= fl_i and fh_i <= int(qh[i, c]) <= fh_i + 1, (i, c, int(fam[i]))
    assert checked > n // 2 and bumped > 0
    # every family reached: exact power-of-two extents, the -126 clamp, the bump loop, ok == False
    assert (e == -126).any() and ((e > e0) & ok).any() and (fam == 0).sum() > 1000
    fl9 = np.floor(((cmin - origin[:, None]).astype(F32) * np.ldexp(F32(1), -e)[:, None]).astype(F32))
    assert ((ql < fl9) & present & (fam == 9)[:, None]).sum() > 1000      # the lo correction ran
