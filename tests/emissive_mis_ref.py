"""numpy restatement of multiple importance sampling of area lights (include/vortex_hip.h, "Multiple importance sampling"): the two
balance-heuristic weights, the emitter index and its lookup, and the frame.  TEST INFRASTRUCTURE ONLY.

A layer over tests/emissive_ref.py: the table, the RNG, the selection, the emitter ray and every piece of the frame are that module's;
what is restated here is what the definition adds, one numpy float32 operation per symbol of the header."""
import numpy as np

import camera_ref as cr
import camera_secondary_ref as csr
import emissive_ref as er
import path_ref as pr
from camera_ref import po

f32 = np.float32
u32 = np.uint32
LARGE = cr.LARGE
PI = er.PI
NOT_LISTED = 0xFFFFFFFF


# ---- the emitter-ray side ----
def _ray_terms(tab, seeds, I, N):
    """e, d2, cosx, an of emissive_ref.emitter_rays, which does not return them: the same operations on the same inputs"""
    tri12, q, cum, Q = tab
    seeds = np.asarray(seeds, np.uint32).copy()
    seeds[seeds == 0] = 1
    I, N = np.asarray(I, np.float32).reshape(-1, 3), np.asarray(N, np.float32).reshape(-1, 3)
    s = er.xorshift(seeds)
    r0 = s
    s = er.xorshift(s)
    a = er.to_float(s)
    s = er.xorshift(s)
    b = er.to_float(s)
    e = er.select(cum, Q, r0)
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
        cosx = np.where(f32(0.0) < dot, dot, f32(0.0)).astype(np.float32)
        c = er._cross(T[:, 3:6], T[:, 6:9])
        an = f32(0.5) * np.abs((c[0] * w[0] + c[1] * w[1]) + c[2] * w[2])
    return e, d2.astype(np.float32), cosx, an.astype(np.float32)


def emitter_rays(tab, scale, seeds, I, N, info=None):
    """rays (n, 6), tmax (n,), Gm (n, 3), e (n,), real (n,), wE (n,): emissive_ref.emitter_rays with G weighted by wE; a ray whose Gm is
    not finite is skipped too, and a skipped ray has wE = 0"""
    tri12, q, cum, Q = tab
    rays, tmax, G, e, real = er.emitter_rays(tab, scale, seeds, I, N, info)
    e2, d2, cosx, an = _ray_terms(tab, seeds, I, N)
    assert (e2 == e).all()
    with np.errstate(all="ignore"):
        qf = q[e].astype(np.float32) / f32(Q)
        pe = d2 * qf
        pb = (cosx / PI) * an
        wE = (pe / (pe + pb)).astype(np.float32)
        Gm = (G * wE[:, None]).astype(np.float32)
        real = real & np.isfinite(Gm).all(1)
    rays, tmax = rays.copy(), tmax.copy()
    rays[~real] = (0, 0, 0, 1, 1, 1)
    tmax[~real] = -1.0
    Gm[~real] = 0.0
    wE[~real] = 0.0
    return rays, tmax, Gm, e, real, wE


# ---- the emitter index ----
def index(pairs):
    """(n, 3) u32: (blasIdx, triIdx, e) sorted by (blasIdx, triIdx, e)"""
    p = np.asarray(pairs, np.uint32).reshape(-1, 2)
    e = np.arange(len(p), dtype=np.uint32)
    order = np.lexsort((e, p[:, 1], p[:, 0]))
    return np.stack([p[order, 0], p[order, 1], e[order]], 1).astype(np.uint32)


def _keys(blas, tri):
    return (np.asarray(blas, np.uint64) << np.uint64(32)) | np.asarray(tri, np.uint64)


def lookup(idx, blas, tri):
    """e (u32) of every (blas, tri): at the smallest position whose key is not below the wanted key, if the key there is equal;
    NOT_LISTED otherwise"""
    want = _keys(blas, tri)
    if len(idx) == 0:
        return np.full(len(want), NOT_LISTED, np.uint32)
    keys = _keys(idx[:, 0], idx[:, 1])
    pos = np.minimum(np.searchsorted(keys, want, side="left"), len(idx) - 1)
    return np.where(keys[pos] == want, idx[pos, 2], u32(NOT_LISTED)).astype(np.uint32)


# ---- the bounce-ray side ----
def hit_weights(tab, idx, rays, hits, normals):
    """(e (n,) u32, wB (n,) f32) of bounce rays (n, 6) with hit records `hits` that left vertices with facing normals `normals` (n, 3);
    a pair that is not listed has wB = 1"""
    tri12, q, cum, Q = tab
    rays, N = np.asarray(rays, np.float32).reshape(-1, 6), np.asarray(normals, np.float32).reshape(-1, 3)
    e = lookup(idx, hits["blasIdx"] & u32(0x7fffffff), hits["triIdx"])
    wB = np.ones(len(e), np.float32)
    m = e != u32(NOT_LISTED)
    if m.any():
        T = tri12[e[m]]
        w, n, t = rays[m, 3:6], N[m], hits["dist"][m].astype(np.float32)
        with np.errstate(all="ignore"):
            qf = q[e[m]].astype(np.float32) / f32(Q)
            dot = (n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]
            cosx = np.where(f32(0.0) < dot, dot, f32(0.0)).astype(np.float32)
            c = er._cross(T[:, 3:6], T[:, 6:9])
            an = f32(0.5) * np.abs((c[0] * w[:, 0] + c[1] * w[:, 1]) + c[2] * w[:, 2])
            pe = (t * t) * qf
            pb = (cosx / PI) * an
            den = pe + pb
            wB[m] = np.where(den > f32(0.0), pb / den, f32(1.0)).astype(np.float32)
    return e, wB


def _facing(N, d):
    flip = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2] > f32(0.0)
    return np.where(flip[:, None], -N, N).astype(np.float32)


# ---- the frame ----
def frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, scale, tab, idx, prim=None, info=None, samples=False, keep=None):
    """emissive_ref.frame_from_rays with nee = 1 and the two weights: pixels (n,) u32, colours (n, 3), rays traced.  info (optional dict)
    collects what happened; samples = True returns (fi, Lc (m, spp, 3), traced) in place of the pixels; keep (optional list) receives, per
    depth, what the weights were computed from: dicts of the emitter rays (er, et, real, open, wE, e, I, Nf) and of the bounce rays that hit
    (rays, hits, normals, emits, e, wB)."""
    info = {} if info is None else info
    params = pr._params(params)
    prim = prim or pr.primary(scene, rays)
    rays, hits0 = prim["rays"], prim["hits"]
    n = len(rays)
    bg = np.asarray(params.background, np.float32)
    col = np.tile(bg, (n, 1)).astype(np.float32)
    fi = np.nonzero(hits0["dist"] != LARGE)[0]
    traced = n
    for key in ("primary_emissive", "bounce_emissive", "unblocked", "blocked", "skipped", "wB_between", "wB_one_unlisted", "wE_below_one"):
        info.setdefault(key, 0)
    info.setdefault("largest", 0.0)
    if len(fi) == 0:
        return (fi, np.zeros((0, spp, 3), np.float32), traced) if samples else (cr.pack_rgb8(col), col, traced)
    lit0, _, nocc = pr.lit(scene, rays[fi], hits0[fi], params, shadow)
    traced += nocc
    with np.errstate(all="ignore"):
        em0, E0 = er.emission(scene, hits0[fi], scale)
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
            Nf = _facing(N, r[:, 3:6])
            seeds = er.path_seeds(pxs[alive], pys[alive], w, spp, smp[alive], ((seed + k) & 0xFFFFFFFF) ^ 0x80000000)
            erays, et, Gm, e_ray, real, wE = emitter_rays(tab, scale, seeds, I, Nf, info)
            open_ = np.zeros(len(alive), bool)
            if real.any():
                open_[real] = cr._trace(scene, erays[real], tmax=et[real], any_hit=True)["dist"] == LARGE
            traced += int(real.sum())
            info["unblocked"] += int(open_.sum())
            info["blocked"] += int((real & ~open_).sum())
            info["skipped"] += int((~real).sum())
            info["wE_below_one"] += int((real & (wE < f32(1.0))).sum())
            oi = alive[open_]
            add = thr[oi] * Gm[open_]
            Lc[oi] = Lc[oi] + add
            if len(add):
                info["largest"] = max(info["largest"], float(Gm[open_].max()))
            bh = cr._trace(scene, sec)
            traced += len(alive)
            hit = bh["dist"] != LARGE
            miss_i, hit_i = alive[~hit], alive[hit]
            Lc[miss_i] = Lc[miss_i] + thr[miss_i] * bg
            lk, _, nocc = pr.lit(scene, sec[hit], bh[hit], params, shadow)
            traced += nocc
            Lc[hit_i] = Lc[hit_i] + thr[hit_i] * lk
            if hit.any():
                emk, Ek = er.emission(scene, bh[hit], scale)
                e_hit, wB = hit_weights(tab, idx, sec[hit], bh[hit], Nf[hit])
                ei = hit_i[emk]
                Ew = (Ek[emk] * wB[emk][:, None]).astype(np.float32)
                Lc[ei] = Lc[ei] + thr[ei] * Ew
                info["bounce_emissive"] += int(emk.sum())
                info["wB_between"] += int((emk & (wB > 0) & (wB < 1)).sum())
                info["wB_one_unlisted"] += int((emk & (e_hit == u32(NOT_LISTED))).sum())
                if len(Ew):
                    info["largest"] = max(info["largest"], float(Ew.max()))
                if keep is not None:
                    keep.append(dict(er=erays, et=et, real=real, open=open_, wE=wE, e_ray=e_ray, I=I, Nf=Nf, rays=sec[hit], hits=bh[hit], normals=Nf[hit],
                                     emits=emk, e=e_hit, wB=wB))
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


def frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, scale, tab, idx, y0=0, y1=None, prim=None, info=None, keep=None):
    """the frame of rows [y0, y1) seen from cam14 (None: the fixed camera): pixels (rows, w), colours (rows, w, 3), rays traced"""
    y1 = h if y1 is None else y1
    xs, ys = csr.pixel_grid(w, y0, y1)
    if prim is None:
        prim = pr.primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))
    px, col, n = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, scale, tab, idx, prim, info, keep=keep)
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), n


def sample_means(scene, cam14, w, h, params, spp, bounces, seed, shadow, scale, tab, idx, info=None):
    """emissive_ref.sample_means of the weighted frame: frame-mean colour (3,) and its standard error, in float64"""
    xs, ys = csr.pixel_grid(w, 0, h)
    prim = pr.primary(scene, cr.rays(cam14, w, h, 0, h))
    fi, Lc, _ = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, scale, tab, idx, prim, info, samples=True)
    n = w * h
    L = Lc.astype(np.float64)
    bg = np.asarray(pr._params(params).background, np.float64)
    mean = (L.mean(1).sum(0) + (n - len(fi)) * bg) / n
    var = (L.var(1, ddof=1) / spp).sum(0) / (n * n)
    return mean, np.sqrt(var)
