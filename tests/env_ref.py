"""numpy restatement of the environment light (include/vortex_hip.h, "Environment light"; vxrt_envmap_*, vxrt_envmap_lookup,
vxrt_env_rays, vxrt_render_path_frame_env).  TEST INFRASTRUCTURE ONLY.

The frame is tests/roulette_ref.py's without an emitter form, piece for piece, with the two rules of the definition -- what a ray that
misses sees, and the environment ray of sample = 1 -- composed of pieces that are pinned elsewhere:
  closest hit, I, N, Lit, Alb       camera_ref, path_ref.lit, camera_secondary_ref.albedo
  the bounce ray, N'                path_ref.bounce_rays, emissive_mis_ref._facing
  seeds, xorshift, random_float     emissive_ref.path_seeds / xorshift / to_float, with the user seed's bit 28 flipped
  the roulette draw                 roulette_ref.step / survival
  counts                            adaptive_ref.clamp, one uniform frame per distinct clamped count, as path_frame_ref.colour
  the filter chain                  path_frame_ref.frame, which takes this module's colours and guides as its `pre`
Everything is numpy float32, one operation per symbol in the order the header writes; np.float32 division and sqrt are the correctly
rounded ones.  tests/test_env_cpu.py holds the restatement to the geometry it claims (density, round trip, estimators).

A map is make_map(texels): a dict with n, texels (n * n, 3), q, cum, Q.  An env part is (map, scale, sample)."""
import numpy as np

import adaptive_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import emissive_mis_ref as mir
import emissive_ref as er
import path_frame_ref as pfr
import path_ref as pr
import roulette_ref as rr
from camera_ref import po

f32 = np.float32
u32 = np.uint32
LARGE = cr.LARGE
PI = f32(3.14159265)
ENV_BIT = 0x10000000


def _sign(t):
    return np.where(t >= 0, f32(1.0), f32(-1.0)).astype(np.float32)


def unfold(u, v):
    """P (3 arrays) and r2 of (u, v) of the texel square"""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        c = (f32(1.0) - np.abs(u)) - np.abs(v)
        fold = c < 0
        uf = np.where(fold, (f32(1.0) - np.abs(v)) * _sign(u), u).astype(np.float32)
        vf = np.where(fold, (f32(1.0) - np.abs(u)) * _sign(v), v).astype(np.float32)
        r2 = (uf * uf + c * c) + vf * vf
    return (uf, c, vf), r2


def _centre_weights(n, texels):
    e = np.arange(n * n)
    i, j = (e % n).astype(np.float32), (e // n).astype(np.float32)
    with np.errstate(all="ignore"):
        u = ((i + f32(0.5)) / f32(n)) * f32(2.0) - f32(1.0)
        v = ((j + f32(0.5)) / f32(n)) * f32(2.0) - f32(1.0)
        _, r2 = unfold(u, v)
        r = np.sqrt(r2)
        m = np.maximum(np.maximum(texels[:, 0], texels[:, 1]), texels[:, 2])
        return (m / (r2 * r)).astype(np.float32)


def make_map(texels):
    """THE TABLE of host texels (n, n, 3), texel (i, j) at [j, i]; None for what vxrt_envmap_create refuses"""
    t = np.asarray(texels, np.float32)
    if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3:
        return None
    n = t.shape[0]
    if n < 4 or n > 256 or n & (n - 1):
        return None
    t = np.ascontiguousarray(t.reshape(n * n, 3))
    if not np.isfinite(t).all() or (t < 0).any() or not (t > 0).any():
        return None
    w = _centre_weights(n, t)
    if not np.isfinite(w).all():
        return None
    with np.errstate(all="ignore"):
        x = (w / w.max()) * f32(65535.0)
    q = np.maximum(x.astype(np.uint32), u32(1))
    cum = np.cumsum(q.astype(np.uint64)).astype(np.uint32)
    return {"n": n, "texels": t, "q": q, "cum": cum, "Q": int(cum[-1])}


def _axis(t, n):
    with np.errstate(all="ignore"):
        fu = (t * f32(0.5) + f32(0.5)) * f32(n)
        ok = fu >= 0                                      # (false for a NaN)
        return np.where(ok, np.minimum(np.where(ok, fu, f32(0.0)).astype(np.uint32), u32(n - 1)), u32(0)).astype(np.uint32)


def texel_of(n, dirs):
    """TEXEL OF A DIRECTION: e (m,) u32 and r2 * r (m,) f32"""
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        s = (np.abs(x) + np.abs(y)) + np.abs(z)
        px, py, pz = x / s, y / s, z / s
        fold = py < 0
        u = np.where(fold, (f32(1.0) - np.abs(pz)) * _sign(px), px).astype(np.float32)
        v = np.where(fold, (f32(1.0) - np.abs(px)) * _sign(pz), pz).astype(np.float32)
        i, j = _axis(u, n), _axis(v, n)
        r2 = (px * px + py * py) + pz * pz
        r = np.sqrt(r2)
        return (i + j * u32(n)).astype(np.uint32), (r2 * r).astype(np.float32)


def density(m, e, r3):
    with np.errstate(all="ignore"):
        qf = m["q"][e].astype(np.float32) / f32(m["Q"])
        nn4 = f32(m["n"] * m["n"]) * f32(0.25)
        return ((qf * nn4) * r3).astype(np.float32)


def lookup(m, scale, dirs):
    """vxrt_envmap_lookup: Env(w) (k, 3), e (k,), pe(w) (k,)"""
    e, r3 = texel_of(m["n"], dirs)
    with np.errstate(all="ignore"):
        L = (m["texels"][e] * f32(scale)).astype(np.float32)
    return L, e, density(m, e, r3)


def miss_weight(pe, Nf, w):
    """wB of bounce rays w that missed, from vertices with facing normals Nf"""
    Nf, w = np.asarray(Nf, np.float32).reshape(-1, 3), np.asarray(w, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        dot = (Nf[:, 0] * w[:, 0] + Nf[:, 1] * w[:, 1]) + Nf[:, 2] * w[:, 2]
        cosx = np.where(f32(0.0) < dot, dot, f32(0.0)).astype(np.float32)       # std::max(0, dot): a NaN gives 0
        pb = cosx / PI
        den = pe + pb
        return np.where(den > 0, pb / den, f32(1.0)).astype(np.float32)


def select(m, r0):
    """(t, e): t = (r0 * Q) >> 32 and the smallest e with cum[e] > t"""
    t = ((np.asarray(r0, np.uint64) * np.uint64(m["Q"])) >> np.uint64(32)).astype(np.uint32)
    return t, np.searchsorted(m["cum"], t, side="right").astype(np.uint32)


def env_rays(m, scale, seeds, I, N, info=None):
    """vxrt_env_rays: rays (k, 6), tmax (k,), Gm (k, 3), e (k,), wE (k,), real (k,) of hash outputs `seeds` at points I with facing normals N"""
    n = m["n"]
    seeds = np.asarray(seeds, np.uint32).copy()
    seeds[seeds == 0] = 1
    I, N = np.asarray(I, np.float32).reshape(-1, 3), np.asarray(N, np.float32).reshape(-1, 3)
    s = er.xorshift(seeds)
    r0 = s
    s = er.xorshift(s)
    a = er.to_float(s)
    s = er.xorshift(s)
    b = er.to_float(s)
    t, e = select(m, r0)
    if info is not None:
        info.setdefault("t", []).append(t)
    i, j = (e % u32(n)).astype(np.float32), (e // u32(n)).astype(np.float32)
    with np.errstate(all="ignore"):
        u = ((i + a) / f32(n)) * f32(2.0) - f32(1.0)
        v = ((j + b) / f32(n)) * f32(2.0) - f32(1.0)
        P, r2 = unfold(u, v)
        r = np.sqrt(r2)
        w = [P[k] / r for k in range(3)]
        o = [I[:, k] + N[:, k] * f32(0.001) for k in range(3)]
        dot = (N[:, 0] * w[0] + N[:, 1] * w[1]) + N[:, 2] * w[2]
        cosx = np.where(f32(0.0) < dot, dot, f32(0.0)).astype(np.float32)
        pE = density(m, e, r2 * r)
        pb = cosx / PI
        Ls = (m["texels"][e] * f32(scale)).astype(np.float32)
        den = PI * pE
        wE = pE / (pE + pb)
        G = (((Ls * cosx[:, None]) / den[:, None]) * wE[:, None]).astype(np.float32)
        skip = (cosx == 0) | (Ls == 0).all(1) | ~np.isfinite(G).all(1)
    rays = np.stack(o + w, 1).astype(np.float32)
    tmax = np.full(len(seeds), f32(1e30), np.float32)
    rays[skip] = (0, 0, 0, 1, 1, 1)
    tmax[skip] = -1.0
    G[skip] = 0.0
    wE = np.where(skip, f32(0.0), wE).astype(np.float32)
    return rays, tmax, G, e, wE, ~skip


def frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, env, roulette=None, prim=None, info=None, samples=False):
    """the frame over `rays` (ray i belongs to pixel (xs[i], ys[i]) of a frame `w` wide): pixels (n,) u32, colours (n, 3), rays traced.
    info (optional dict): "live"[k], "missed"[k] = the bounce rays of depth k and those that missed, "sent"[k] / "open"[k] = the
    environment rays traced / unblocked, "killed"[k] = the hits the roulette ended.  samples = True returns (fi, Lc (m, spp, 3), traced,
    the colours of the misses)."""
    m, scale, sample = env
    info = {} if info is None else info
    for key in ("live", "missed", "sent", "open", "killed"):
        info.setdefault(key, [0] * bounces)
    params = pr._params(params)
    prim = prim or pr.primary(scene, rays)
    rays, hits0 = prim["rays"], prim["hits"]
    n = len(rays)
    col = np.zeros((n, 3), np.float32)
    fi = np.nonzero(hits0["dist"] != LARGE)[0]
    mi = np.nonzero(hits0["dist"] == LARGE)[0]
    col[mi] = lookup(m, scale, rays[mi, 3:6])[0]
    traced = n
    if len(fi) == 0:
        return (fi, np.zeros((0, spp, 3), np.float32), traced, col) if samples else (cr.pack_rgb8(col), col, traced)
    lit0, _, nocc = pr.lit(scene, rays[fi], hits0[fi], params, shadow)
    traced += nocc
    with np.errstate(all="ignore"):
        alb0 = csr.albedo(scene, hits0[fi])
        k0 = len(fi)
        Lc = np.repeat(lit0, spp, 0).astype(np.float32)
        thr = np.repeat(alb0, spp, 0).astype(np.float32)
        pxs, pys = np.repeat(np.asarray(xs)[fi], spp), np.repeat(np.asarray(ys)[fi], spp)
        smp = np.tile(np.arange(spp, dtype=np.uint32), k0)
        alive = np.arange(k0 * spp)
        r, h = np.repeat(rays[fi], spp, 0), np.repeat(hits0[fi], spp, 0)
        for k in range(bounces):
            if len(alive) == 0:
                continue
            info["live"][k] += len(alive)
            user = (seed + k) & 0xFFFFFFFF
            I, N, _ = cr._normal_and_point(scene, r, h)
            I, N = np.stack(I, 1).astype(np.float32), np.stack(N, 1).astype(np.float32)
            ax, ay, asmp = pxs[alive], pys[alive], smp[alive]
            sec = pr.bounce_rays(ax, ay, w, spp, asmp, seed + k, I, N, r[:, 3:6])
            Nf = mir._facing(N, r[:, 3:6])
            if sample:
                seeds = er.path_seeds(ax, ay, w, spp, asmp, user ^ ENV_BIT)
                erays, et, G, _, _, real = env_rays(m, scale, seeds, I, Nf)
                open_ = np.zeros(len(alive), bool)
                if real.any():
                    open_[real] = cr._trace(scene, erays[real], tmax=et[real], any_hit=True)["dist"] == LARGE
                traced += int(real.sum())
                info["sent"][k] += int(real.sum())
                info["open"][k] += int(open_.sum())
                oi = alive[open_]
                Lc[oi] = Lc[oi] + thr[oi] * G[open_]
            bh = cr._trace(scene, sec)
            traced += len(alive)
            hit = bh["dist"] != LARGE
            miss_i, hit_i = alive[~hit], alive[hit]
            info["missed"][k] += len(miss_i)
            if len(miss_i):
                E, _, pe = lookup(m, scale, sec[~hit, 3:6])
                if sample:
                    E = (E * miss_weight(pe, Nf[~hit], sec[~hit, 3:6])[:, None]).astype(np.float32)
                Lc[miss_i] = Lc[miss_i] + thr[miss_i] * E
            rh, hh = sec[hit], bh[hit]
            lk, _, nocc = pr.lit(scene, rh, hh, params, shadow)
            traced += nocc
            Lc[hit_i] = Lc[hit_i] + thr[hit_i] * lk
            keep = np.ones(len(hit_i), bool)
            if hit.any():
                thr[hit_i] = thr[hit_i] * csr.albedo(scene, hh)
                j = k + 1
                if roulette is not None and roulette[0] <= j < bounces:
                    first, q_min = roulette
                    seeds = er.path_seeds(pxs[hit_i], pys[hit_i], w, spp, smp[hit_i], user ^ rr.ROULETTE_BIT)
                    t, a, _ = rr.step(thr[hit_i], seeds, q_min)
                    keep = a != 0
                    thr[hit_i[keep]] = t[keep]
                    info["killed"][k] += int((~keep).sum())
            r, h, alive = rh[keep], hh[keep], hit_i[keep]
        Lc = Lc.reshape(k0, spp, 3)
        if samples:
            return fi, Lc, traced, col
        acc = Lc[:, 0].copy()
        for s in range(1, spp):
            acc = acc + Lc[:, s]
        col[fi] = acc / f32(spp)
    return cr.pack_rgb8(col), col, traced


def _prim(scene, cam14, w, h, y0, y1):
    return pr.primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))


def colour(scene, cam14, w, h, params, spp, bounces, seed, shadow, env, counts=None, roulette=None, y0=0, y1=None, prim=None, info=None):
    """pixels (rows, w), colours (rows, w, 3), rays traced of rows [y0, y1).  counts: None, or the full frame's raw counts (h, w) -- spp
    is then the cap and every hash input takes the pixel's own n_p"""
    y1 = h if y1 is None else y1
    xs, ys = csr.pixel_grid(w, y0, y1)
    prim = prim or _prim(scene, cam14, w, h, y0, y1)
    n = len(prim["rays"])
    if counts is None:
        px, col, traced = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, env, roulette, prim, info)
    else:
        n_p = ar.clamp(np.asarray(counts).reshape(h, w)[y0:y1].reshape(-1), spp)
        px, col, traced = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), 0
        for v in np.unique(n_p):
            sel = np.nonzero(n_p == v)[0]
            sub = {"rays": prim["rays"][sel], "hits": prim["hits"][sel]}
            p, c, t = frame_from_rays(scene, sub["rays"], xs[sel], ys[sel], w, params, int(v), bounces, seed, shadow, env, roulette, sub, info)
            px[sel], col[sel] = p, c
            traced += t
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), traced


def guides(scene, cam14, w, h, params, shadow, env, y0=0, y1=None, prim=None):
    """denoise_ref.path_guides with D = Env(dir(r_0)) at a primary miss"""
    D, A, P, N, prim = pfr.guides(scene, cam14, w, h, params, shadow, None, y0, y1, prim)
    miss = prim["hits"]["dist"] == LARGE
    flat = D.reshape(-1, 3).copy()
    flat[miss] = lookup(env[0], env[1], prim["rays"][miss, 3:6])[0]
    return flat.reshape(D.shape), A, P, N, prim


def frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, env, counts=None, roulette=None, dn=None, tp=None, hist=None, motion=0, snap=None, vp=None,
          y0=0, y1=None, info=None):
    """vxrt_render_path_frame_env over rows [y0, y1): path_frame_ref.frame's dict, made from this module's colours and guides -- the
    filter chain is path_frame_ref's, untouched"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim = guides(scene, cam14, w, h, params, shadow, env, y0, y1)
    px, c, traced = colour(scene, cam14, w, h, params, spp, bounces, seed, shadow, env, counts, roulette, y0, y1, prim, info)
    return pfr.frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, None, counts, dn, tp, hist, motion, snap, vp, y0, y1,
                     pre=(D, A, P, N, prim, px, c, traced))


def sample_stats(scene, cam14, w, h, params, spp, bounces, seed, shadow, env, info=None):
    """in float64: the frame-mean colour (3,) before the pack, its standard error from the per-sample spread, and the mean over the
    pixels with a hit of the per-pixel sample variance (3,)"""
    xs, ys = csr.pixel_grid(w, 0, h)
    prim = _prim(scene, cam14, w, h, 0, h)
    fi, Lc, _, col = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, env, None, prim, info, samples=True)
    n = w * h
    L = Lc.astype(np.float64)
    miss = np.ones(n, bool)
    miss[fi] = False
    mean = (L.mean(1).sum(0) + col[miss].astype(np.float64).sum(0)) / n
    var = L.var(1, ddof=1)
    return mean, np.sqrt((var / spp).sum(0)) / n, var.mean(0)
