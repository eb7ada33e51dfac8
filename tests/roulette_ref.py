"""numpy restatement of Russian roulette in path frames (include/vortex_hip.h, "Russian roulette"; vxrt_render_path_frame_ex and
vxrt_roulette).  TEST INFRASTRUCTURE ONLY.

The frame is tests/path_ref.py's, piece for piece, with the emitter forms of emissive_ref / emissive_mis_ref and the draw of the
definition, composed of pieces that are pinned elsewhere:
  closest hit, I, N                 camera_ref._trace, camera_ref._normal_and_point
  Lit, Alb                          path_ref.lit, camera_secondary_ref.albedo
  the bounce ray                    path_ref.bounce_rays
  the draw's seed, xi               emissive_ref.path_seeds / xorshift / to_float with the user seed's bit 29 flipped
  emitter rays, Emi, weights        emissive_ref / emissive_mis_ref (tables, emitter_rays, emission, hit_weights)
  counts                            adaptive_ref.clamp, one uniform frame per distinct clamped count, as path_frame_ref.colour
  the filter chain                  path_frame_ref.frame, which takes this module's colours as its `pre`
Everything is numpy float32; np.float32 division is the correctly rounded one.  tests/test_roulette_cpu.py holds the frame without
roulette bit-equal to path_frame_ref's and shows that the GPU cases (tests/roulette_cases.py) are not vacuous.

roulette is None or (first, q_min).  An emitter form is None, ("nee0", scale), ("nee1", scale, tab) or ("mis", scale, tab, idx), as
tests/path_frame_ref.py takes it."""
import numpy as np

import adaptive_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import emissive_mis_ref as mir
import emissive_ref as er
import path_frame_ref as pfr
import path_ref as pr
from camera_ref import po

f32 = np.float32
u32 = np.uint32
LARGE = cr.LARGE
ROULETTE_BIT = 0x20000000
EMITTER_BIT = 0x80000000


def survival(thr, q_min):
    """q (n,) f32 of throughputs thr (n, 3): m = x; if (y > m) m = y; if (z > m) m = z; q = m; if (!(q >= q_min)) q = q_min"""
    t = np.asarray(thr, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        m = t[:, 0]
        m = np.where(t[:, 1] > m, t[:, 1], m)
        m = np.where(t[:, 2] > m, t[:, 2], m)
        return np.where(m >= f32(q_min), m, f32(q_min)).astype(np.float32)


def step(thr, seeds, q_min, divide=True):
    """vxrt_roulette: (thr_out (n, 3), alive (n,) u32, drew (n,) bool) of throughputs thr and hash outputs seeds (0 becomes 1).  q >= 1:
    no draw, thr untouched; else alive iff xi < q and thr_out = thr / q; a dead entry has three zeros.  divide = False is the
    deliberately wrong variant of tests/test_roulette_cpu.py: survivors keep thr."""
    t = np.asarray(thr, np.float32).reshape(-1, 3)
    q = survival(t, q_min)
    s = np.asarray(seeds, np.uint32).copy()
    s[s == 0] = 1
    xi = er.to_float(er.xorshift(s))
    with np.errstate(all="ignore"):
        drew = ~(q >= f32(1.0))
        alive = ~drew | (xi < q)
        out = t.copy()
        sv = drew & alive
        if divide:
            out[sv] = (t[sv] / q[sv][:, None]).astype(np.float32)
    out[~alive] = 0.0
    return out, alive.astype(np.uint32), drew


def frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, emitter=None, roulette=None, prim=None, info=None, samples=False,
                    divide=True):
    """the frame over `rays` (ray i belongs to pixel (xs[i], ys[i]) of a frame `w` wide): pixels (n,) u32, colours (n, 3), rays traced.
    info (optional dict): "live"[k] = the paths that trace a bounce ray at depth k, "drew"[k] / "killed"[k] = the hits of depth k that
    took a draw / that it ended, "floored" = the draws whose q was q_min.  samples = True returns (fi, Lc (m, spp, 3), traced)."""
    info = {} if info is None else info
    for key in ("live", "drew", "killed"):
        info.setdefault(key, [0] * bounces)
    info.setdefault("floored", 0)
    params = pr._params(params)
    prim = prim or pr.primary(scene, rays)
    rays, hits0 = prim["rays"], prim["hits"]
    form = None if emitter is None else emitter[0]
    scale = None if emitter is None else emitter[1]
    tab = emitter[2] if form in ("nee1", "mis") else None
    n = len(rays)
    bg = np.asarray(params.background, np.float32)
    col = np.tile(bg, (n, 1)).astype(np.float32)
    fi = np.nonzero(hits0["dist"] != LARGE)[0]
    traced = n
    if len(fi) == 0:
        return (fi, np.zeros((0, spp, 3), np.float32), traced) if samples else (cr.pack_rgb8(col), col, traced)
    lit0, _, nocc = pr.lit(scene, rays[fi], hits0[fi], params, shadow)
    traced += nocc
    with np.errstate(all="ignore"):
        lit0 = lit0.copy()
        if form is not None:
            em0, E0 = er.emission(scene, hits0[fi], scale)
            lit0[em0] = lit0[em0] + E0[em0]
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
            info["live"][k] += len(alive)
            user = (seed + k) & 0xFFFFFFFF
            I, N, _ = cr._normal_and_point(scene, r, h)
            I, N = np.stack(I, 1).astype(np.float32), np.stack(N, 1).astype(np.float32)
            ax, ay, asmp = pxs[alive], pys[alive], smp[alive]
            sec = pr.bounce_rays(ax, ay, w, spp, asmp, seed + k, I, N, r[:, 3:6])
            Nf = mir._facing(N, r[:, 3:6])
            if tab is not None:
                seeds = er.path_seeds(ax, ay, w, spp, asmp, user ^ EMITTER_BIT)
                sample = mir.emitter_rays if form == "mis" else er.emitter_rays
                erays, et, G, _, real = sample(tab, scale, seeds, I, Nf)[:5]
                open_ = np.zeros(len(alive), bool)
                if real.any():
                    open_[real] = cr._trace(scene, erays[real], tmax=et[real], any_hit=True)["dist"] == LARGE
                traced += int(real.sum())
                oi = alive[open_]
                Lc[oi] = Lc[oi] + thr[oi] * G[open_]
            bh = cr._trace(scene, sec)
            traced += len(alive)
            hit = bh["dist"] != LARGE
            miss_i, hit_i = alive[~hit], alive[hit]
            Lc[miss_i] = Lc[miss_i] + thr[miss_i] * bg
            rh, hh = sec[hit], bh[hit]
            lk, _, nocc = pr.lit(scene, rh, hh, params, shadow)
            traced += nocc
            Lc[hit_i] = Lc[hit_i] + thr[hit_i] * lk
            keep = np.ones(len(hit_i), bool)
            if hit.any():
                if form in ("nee0", "mis"):
                    emk, Ek = er.emission(scene, hh, scale)
                    if form == "mis":
                        _, wB = mir.hit_weights(tab, emitter[3], rh, hh, Nf[hit])
                        Ek = (Ek * wB[:, None]).astype(np.float32)
                    ei = hit_i[emk]
                    Lc[ei] = Lc[ei] + thr[ei] * Ek[emk]
                thr[hit_i] = thr[hit_i] * csr.albedo(scene, hh)
                j = k + 1                                            # the hits of depth k are vertex j
                if roulette is not None and roulette[0] <= j < bounces:
                    first, q_min = roulette
                    seeds = er.path_seeds(pxs[hit_i], pys[hit_i], w, spp, smp[hit_i], user ^ ROULETTE_BIT)
                    info["floored"] += int((survival(thr[hit_i], q_min) == f32(q_min)).sum())
                    t, a, drew = step(thr[hit_i], seeds, q_min, divide)
                    keep = a != 0
                    thr[hit_i[keep]] = t[keep]
                    info["drew"][k] += int(drew.sum())
                    info["killed"][k] += int((~keep).sum())
            r, h, alive = rh[keep], hh[keep], hit_i[keep]
        Lc = Lc.reshape(m, spp, 3)
        if samples:
            return fi, Lc, traced
        acc = Lc[:, 0].copy()
        for s in range(1, spp):
            acc = acc + Lc[:, s]
        col[fi] = acc / f32(spp)
    return cr.pack_rgb8(col), col, traced


def colour(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter=None, counts=None, roulette=None, y0=0, y1=None, prim=None, info=None):
    """path_frame_ref.colour with roulette: pixels (rows, w), colours (rows, w, 3), rays traced.  counts: None, or the full frame's raw
    counts (h, w) -- spp is then the cap and the draw's hash input takes the pixel's own n_p"""
    y1 = h if y1 is None else y1
    xs, ys = csr.pixel_grid(w, y0, y1)
    if prim is None:
        prim = pr.primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))
    n = len(prim["rays"])
    if counts is None:
        px, col, traced = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, emitter, roulette, prim, info)
    else:
        n_p = ar.clamp(np.asarray(counts).reshape(h, w)[y0:y1].reshape(-1), spp)
        px, col, traced = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), 0
        for v in np.unique(n_p):
            sel = np.nonzero(n_p == v)[0]
            sub = {"rays": prim["rays"][sel], "hits": prim["hits"][sel]}
            p, c, t = frame_from_rays(scene, sub["rays"], xs[sel], ys[sel], w, params, int(v), bounces, seed, shadow, emitter, roulette, sub, info)
            px[sel], col[sel] = p, c
            traced += t
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), traced


def frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter=None, counts=None, roulette=None, dn=None, tp=None, hist=None, motion=0, snap=None,
          vp=None, y0=0, y1=None, info=None):
    """vxrt_render_path_frame_ex over rows [y0, y1): path_frame_ref.frame's dict, made from this module's colours -- the guides and the
    filter chain are path_frame_ref's, untouched, as the definition has it"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim = pfr.guides(scene, cam14, w, h, params, shadow, emitter, y0, y1)
    px, c, traced = colour(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter, counts, roulette, y0, y1, prim, info)
    return pfr.frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter, counts, dn, tp, hist, motion, snap, vp, y0, y1,
                     pre=(D, A, P, N, prim, px, c, traced))


def sample_means(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter=None, roulette=None, divide=True, info=None):
    """frame-mean colour (3,) of the frame before the pack and its standard error, in float64, as emissive_ref.sample_means"""
    xs, ys = csr.pixel_grid(w, 0, h)
    prim = pr.primary(scene, cr.rays(cam14, w, h, 0, h))
    fi, Lc, _ = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, emitter, roulette, prim, info, samples=True, divide=divide)
    n = w * h
    L = Lc.astype(np.float64)
    bg = np.asarray(pr._params(params).background, np.float64)
    mean = (L.mean(1).sum(0) + (n - len(fi)) * bg) / n
    var = (L.var(1, ddof=1) / spp).sum(0) / (n * n)
    return mean, np.sqrt(var)
