"""numpy restatement of emissive geometry (include/vortex_hip.h, "Emissive geometry"): the emitter table, the emitter ray and the path
frame with emission at bounce hits (nee = 0) or emitter sampling (nee = 1).  TEST INFRASTRUCTURE ONLY.

The frame is tests/path_ref.py's, piece for piece (primary, lit, bounce_rays, albedo, the accumulation), with the additions of the
definition; tests/test_emissive_cpu.py holds it bit-equal to path_ref.frame on a scene without emissive materials.  The table, the RNG
and the selection are restated in numpy uint32 / uint64, everything else in numpy float32: one operation per symbol of the header."""
import numpy as np

import camera_ref as cr
import camera_secondary_ref as csr
import path_ref as pr
from camera_ref import po

f32 = np.float32
u32 = np.uint32
LARGE = cr.LARGE
PI = f32(3.14159265)


# ---- RNG (common.h:129-147) ----
def wang_hash(s):
    s = np.asarray(s, np.uint32).copy()
    with np.errstate(over="ignore"):
        s = (s ^ u32(61)) ^ (s >> u32(16))
        s = s * u32(9)
        s = s ^ (s >> u32(4))
        s = s * u32(0x27d4eb2d)
        s = s ^ (s >> u32(15))
    return s


def xorshift(s):
    s = np.asarray(s, np.uint32)
    s = s ^ (s << u32(13))
    s = s ^ (s >> u32(17))
    s = s ^ (s << u32(5))
    return s


def to_float(s):
    return s.astype(np.float32) * f32(2.3283064365387e-10)


def path_seeds(xs, ys, w, spp, smp, user_seed):
    """the bounce ray's hash input with user seed `user_seed` (uint32 arithmetic)"""
    with np.errstate(over="ignore"):
        x, y, s = np.asarray(xs, np.uint32), np.asarray(ys, np.uint32), np.asarray(smp, np.uint32)
        return wang_hash((x + y * u32(w)) * u32(spp) + s + u32(1) + u32(user_seed & 0xFFFFFFFF) * u32(0x9E3779B9))


# ---- the table ----
def _materials(scene):
    return np.frombuffer(np.ascontiguousarray(scene["mat"], np.uint8).tobytes(), np.float32).reshape(-1, 22)


def _tex_ids(scene):
    return np.frombuffer(np.ascontiguousarray(scene["triEx"], np.uint8).tobytes(), np.uint32).reshape(-1, 16)[:, 15]


def table(scene, pairs):
    """tri12 (n, 12) f32 = V0, E1, E2, Le; q (n,) u32; cum (n,) u32; Q"""
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    blas = np.frombuffer(np.ascontiguousarray(scene["blas"], np.uint8).tobytes(), np.float32).reshape(-1, 40)
    tri = np.frombuffer(np.ascontiguousarray(scene["tri"], np.uint8).tobytes(), np.float32).reshape(-1, 3, 3)
    m = blas[pairs[:, 0], 17:29].reshape(-1, 3, 4)
    v = tri[pairs[:, 1]]
    Le = _materials(scene)[_tex_ids(scene)[pairs[:, 1]], 9:12]
    with np.errstate(all="ignore"):
        V = np.zeros((len(pairs), 3, 3), np.float32)
        for k in range(3):
            for a in range(3):
                V[:, k, a] = ((m[:, a, 0] * v[:, k, 0] + m[:, a, 1] * v[:, k, 1]) + m[:, a, 2] * v[:, k, 2]) + m[:, a, 3]
        E1, E2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
        c = _cross(E1, E2)
        area = f32(0.5) * np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        w = area * np.maximum(np.maximum(Le[:, 0], Le[:, 1]), Le[:, 2])
        x = (w / w.max()) * f32(65535.0)
    q = np.maximum(x.astype(np.uint32), u32(1))
    cum = np.cumsum(q.astype(np.uint64)).astype(np.uint32)
    return np.concatenate([V[:, 0], E1, E2, Le], 1).astype(np.float32), q, cum, int(cum[-1])


def _cross(a, b):
    return [a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]]


def select(cum, Q, r0):
    """t = (r0 * Q) >> 32 in uint64; the smallest e with cum[e] > t"""
    t = (np.asarray(r0, np.uint64) * np.uint64(Q)) >> np.uint64(32)
    return np.searchsorted(np.asarray(cum, np.uint64), t, side="right").astype(np.uint32)


# ---- the emitter ray ----
def emitter_rays(tab, scale, seeds, I, N, info=None):
    """rays (n, 6), tmax (n,), G (n, 3), e (n,), real (n,) of hash outputs `seeds` at points I with facing normals N"""
    tri12, q, cum, Q = tab
    seeds = np.asarray(seeds, np.uint32).copy()
    seeds[seeds == 0] = 1
    I, N = np.asarray(I, np.float32).reshape(-1, 3), np.asarray(N, np.float32).reshape(-1, 3)
    n = len(seeds)
    s = xorshift(seeds)
    r0 = s
    s = xorshift(s)
    a = to_float(s)
    s = xorshift(s)
    b = to_float(s)
    e = select(cum, Q, r0)
    T = tri12[e]
    with np.errstate(all="ignore"):
        fold = a + b > f32(1.0)
        a = np.where(fold, f32(1.0) - a, a).astype(np.float32)
        b = np.where(fold, f32(1.0) - b, b).astype(np.float32)
        P = [(T[:, k] + a * T[:, 3 + k]) + b * T[:, 6 + k] for k in range(3)]
        o = [I[:, k] + N[:, k] * f32(0.001) for k in range(3)]
        v = [P[k] - o[k] for k in range(3)]
        d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        d = np.sqrt(d2)
        w = [v[k] / d for k in range(3)]
        dot = (N[:, 0] * w[0] + N[:, 1] * w[1]) + N[:, 2] * w[2]
        cosx = np.where(f32(0.0) < dot, dot, f32(0.0)).astype(np.float32)     # std::max(0.0f, dot)
        c = _cross(T[:, 3:6], T[:, 6:9])
        an = f32(0.5) * np.abs((c[0] * w[0] + c[1] * w[1]) + c[2] * w[2])
        den = (PI * d2) * (q[e].astype(np.float32) / f32(Q))
        G = np.stack([(((T[:, 9 + k] * f32(scale)) * cosx) * an) / den for k in range(3)], 1).astype(np.float32)
        real = ~((cosx == 0) | (d2 == 0) | ~np.isfinite(G).all(1))
        rays = np.stack(o + w, 1).astype(np.float32)
        tmax = (d - f32(0.001)).astype(np.float32)
    rays[~real] = (0, 0, 0, 1, 1, 1)
    tmax[~real] = -1.0
    G[~real] = 0.0
    if info is not None:
        info["folds"] = info.get("folds", 0) + int(fold.sum())
        info["skipped_cos"] = info.get("skipped_cos", 0) + int(((cosx == 0) & (d2 != 0)).sum())
        info.setdefault("selected", set()).update(int(x) for x in np.unique(e))
    assert n == len(rays)
    return rays, tmax, G, e, real


def emission(scene, hits, scale):
    """(mask of the hits whose material emits, Emi = emissive * scale of all of them)"""
    Le = _materials(scene)[_tex_ids(scene)[hits["triIdx"]], 9:12]
    with np.errstate(all="ignore"):
        return (Le > 0).any(1), (Le * f32(scale)).astype(np.float32)


# ---- the frame ----
def frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, nee, scale, tab=None, prim=None, info=None, samples=False):
    """path_ref.frame_from_rays with emissive geometry: pixels (n,) u32, colours (n, 3), rays traced.  info (optional dict) collects what
    happened; samples = True returns (fi, Lc (m, spp, 3)) in place of the pixels."""
    info = {} if info is None else info
    params = pr._params(params)
    prim = prim or pr.primary(scene, rays)
    rays, hits0 = prim["rays"], prim["hits"]
    n = len(rays)
    bg = np.asarray(params.background, np.float32)
    col = np.tile(bg, (n, 1)).astype(np.float32)
    fi = np.nonzero(hits0["dist"] != LARGE)[0]
    traced = n
    for key in ("primary_emissive", "bounce_emissive", "unblocked", "blocked", "skipped"):
        info.setdefault(key, 0)
    if len(fi) == 0:
        return (fi, np.zeros((0, spp, 3), np.float32), traced) if samples else (cr.pack_rgb8(col), col, traced)
    lit0, _, nocc = pr.lit(scene, rays[fi], hits0[fi], params, shadow)
    traced += nocc
    with np.errstate(all="ignore"):
        em0, E0 = emission(scene, hits0[fi], scale)
        lit0 = lit0.copy()
        lit0[em0] = lit0[em0] + E0[em0]
        info["primary_emissive"] += int(em0.sum())
        alb0 = csr.albedo(scene, hits0[fi])
        m = len(fi)
        Lc = np.repeat(lit0, spp, 0).astype(np.float32)
        thr = np.repeat(alb0, spp, 0).astype(np.float32)
        pxs, pys = np.repeat(np.asarray(xs)[fi], spp), np.repeat(np.asarray(ys)[fi], spp)
        smp = np.tile(np.arange(spp, dtype=np.uint32), m)
        alive = np.arange(m * spp)
        r, h = np.repeat(rays[fi], spp, 0), np.repeat(hits0[fi], spp, 0)
        for k in range(bounces):
            if len(alive) == 0:
                continue
            I, N, _ = cr._normal_and_point(scene, r, h)
            I, N = np.stack(I, 1).astype(np.float32), np.stack(N, 1).astype(np.float32)
            sec = pr.bounce_rays(pxs[alive], pys[alive], w, spp, smp[alive], seed + k, I, N, r[:, 3:6])
            if nee:
                d = r[:, 3:6]
                flip = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2] > f32(0.0)
                Nf = np.where(flip[:, None], -N, N).astype(np.float32)
                seeds = path_seeds(pxs[alive], pys[alive], w, spp, smp[alive], ((seed + k) & 0xFFFFFFFF) ^ 0x80000000)
                er, et, G, _, real = emitter_rays(tab, scale, seeds, I, Nf, info)
                open_ = np.zeros(len(alive), bool)
                if real.any():
                    open_[real] = cr._trace(scene, er[real], tmax=et[real], any_hit=True)["dist"] == LARGE
                traced += int(real.sum())
                info["unblocked"] += int(open_.sum())
                info["blocked"] += int((real & ~open_).sum())
                info["skipped"] += int((~real).sum())
                oi = alive[open_]
                Lc[oi] = Lc[oi] + thr[oi] * G[open_]
            bh = cr._trace(scene, sec)
            traced += len(alive)
            hit = bh["dist"] != LARGE
            miss_i, hit_i = alive[~hit], alive[hit]
            Lc[miss_i] = Lc[miss_i] + thr[miss_i] * bg
            lk, _, nocc = pr.lit(scene, sec[hit], bh[hit], params, shadow)
            traced += nocc
            Lc[hit_i] = Lc[hit_i] + thr[hit_i] * lk
            if hit.any():
                if not nee:
                    emk, Ek = emission(scene, bh[hit], scale)
                    ei = hit_i[emk]
                    Lc[ei] = Lc[ei] + thr[ei] * Ek[emk]
                    info["bounce_emissive"] += int(emk.sum())
                thr[hit_i] = thr[hit_i] * csr.albedo(scene, bh[hit])
            r, h, alive = sec[hit], bh[hit], hit_i
        Lc = Lc.reshape(m, spp, 3)
        if samples:
            return fi, Lc, traced
        acc = Lc[:, 0].copy()
        for s in range(1, spp):
            acc = acc + Lc[:, s]
        col[fi] = acc / f32(spp)
    return cr.pack_rgb8(col), col, traced


def frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, nee, scale, tab=None, y0=0, y1=None, prim=None, info=None):
    """the frame of rows [y0, y1) seen from cam14 (None: the fixed camera): pixels (rows, w), colours (rows, w, 3), rays traced"""
    y1 = h if y1 is None else y1
    xs, ys = csr.pixel_grid(w, y0, y1)
    if prim is None:
        prim = pr.primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))
    px, col, n = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, nee, scale, tab, prim, info)
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), n


def sample_means(scene, cam14, w, h, params, spp, bounces, seed, shadow, nee, scale, tab=None):
    """frame-mean colour (3,) of the frame before the pack, and its standard error from the per-pixel sample variances, in float64: the
    frame mean is the mean over pixels of per-pixel means of spp independent samples (a pixel that misses is the background, exactly)"""
    xs, ys = csr.pixel_grid(w, 0, h)
    prim = pr.primary(scene, cr.rays(cam14, w, h, 0, h))
    fi, Lc, _ = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, nee, scale, tab, prim, samples=True)
    n = w * h
    L = Lc.astype(np.float64)
    bg = np.asarray(pr._params(params).background, np.float64)
    mean = (L.mean(1).sum(0) + (n - len(fi)) * bg) / n
    var = (L.var(1, ddof=1) / spp).sum(0) / (n * n)
    return mean, np.sqrt(var)
