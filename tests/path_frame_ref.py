"""numpy restatement of path frames by descriptor (include/vortex_hip.h, "Path frames by descriptor"; vxrt_render_path_frame).  TEST
INFRASTRUCTURE ONLY.

A thin layer that composes the unchanged restatements of the sections the frame is made of:
  colour       c and the rays traced come from path_ref / emissive_ref / emissive_mis_ref, whichever the emitter form names; with counts,
               once per distinct clamped count v over the rays whose pixel has n_p = v, with spp = v, as adaptive_ref.frame_from_rays does
               (EMITTER FORM x COUNTS: the pixel is the emissive frame's pixel with spp := n_p)
  guides       D = denoise_ref.path_guides' Lit_0, plus emissive_ref.emission at the primary hits whose material emits -- nothing is added
               elsewhere (EMITTER FORM x FILTER); A, P, N are path_guides'
  the chain    demodulation as every *_ref.path_frame writes it, then denoise_ref.atrous | temporal_ref.step / motion_ref.step |
               variance_ref.step, initial_variance, atrous_v, none of them changed
tests/test_path_frame_cpu.py holds the layer bit-equal to each of those path_frame functions where no emitter form is named.

An emitter form is None, ("nee0", scale), ("nee1", scale, tab) or ("mis", scale, tab, idx): tab = emissive_ref.table, idx =
emissive_mis_ref.index."""
import numpy as np

import adaptive_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import denoise_ref as dr
import emissive_mis_ref as mir
import emissive_ref as er
import motion_ref as mr
import path_ref as pr
import temporal_ref as tr
import variance_ref as vr
from camera_ref import po

f32 = np.float32


def _uniform(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, emitter, prim, info=None):
    """(pixels, colours, rays traced) of the uniform frame of the emitter form over `rays`"""
    if emitter is None:
        return pr.frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, prim)[:3]
    if emitter[0] == "mis":
        return mir.frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, emitter[1], emitter[2], emitter[3], prim, info)
    nee = {"nee0": 0, "nee1": 1}[emitter[0]]
    return er.frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, nee, emitter[1], emitter[2] if nee else None, prim, info)


def colour(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter=None, counts=None, y0=0, y1=None, prim=None, info=None):
    """the path frame the filter chain starts from, rows [y0, y1): pixels (rows, w), colours (rows, w, 3), rays traced.  counts: None, or
    the full frame's raw counts (h, w) -- spp is then the cap"""
    y1 = h if y1 is None else y1
    xs, ys = csr.pixel_grid(w, y0, y1)
    if prim is None:
        prim = pr.primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))
    n = len(prim["rays"])
    if counts is None:
        px, col, traced = _uniform(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, emitter, prim, info)
    else:
        n_p = ar.clamp(np.asarray(counts).reshape(h, w)[y0:y1].reshape(-1), spp)
        px, col, traced = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), 0
        for v in np.unique(n_p):
            sel = np.nonzero(n_p == v)[0]
            sub = {"rays": prim["rays"][sel], "hits": prim["hits"][sel]}
            p, c, t = _uniform(scene, sub["rays"], xs[sel], ys[sel], w, params, int(v), bounces, seed, shadow, emitter, sub, info)
            px[sel], col[sel] = p, c
            traced += t
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), traced


def guides(scene, cam14, w, h, params, shadow, emitter=None, y0=0, y1=None, prim=None):
    """denoise_ref.path_guides with D = Lit_0 + Emi(h_0) where the primary hit's material emits"""
    D, A, P, N, prim = dr.path_guides(scene, cam14, w, h, params, shadow, y0, y1, prim)
    if emitter is not None:
        hits0 = prim["hits"]
        fi = np.nonzero(hits0["dist"] != pr.LARGE)[0]
        if len(fi):
            with np.errstate(all="ignore"):
                em0, E0 = er.emission(scene, hits0[fi], emitter[1])
                flat = D.reshape(-1, 3).copy()
                flat[fi[em0]] = flat[fi[em0]] + E0[em0]
            D = flat.reshape(D.shape)
    return D, A, P, N, prim


def inputs(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter=None, counts=None, y0=0, y1=None, info=None):
    """(D, A, P, N, prim, px, c, rays traced): what a frame is made from whatever its filter, history and motion -- the expensive part"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim = guides(scene, cam14, w, h, params, shadow, emitter, y0, y1)
    px, c, traced = colour(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter, counts, y0, y1, prim, info)
    return D, A, P, N, prim, px, c, traced


def frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter=None, counts=None, dn=None, tp=None, hist=None, motion=0, snap=None, vp=None,
          y0=0, y1=None, pre=None, stats=None, info=None):
    """vxrt_render_path_frame over rows [y0, y1).  dn = (iterations, normal_power, sigma_z, sigma_l) or None; tp = the step's prm with
    hist, a temporal_ref / variance_ref History (moments iff vp); motion = 1 takes snapshot `snap` (motion_ref.snapshot); vp = (epsilon,
    min_len, radius); pre = inputs() of the same arguments.  A dict: px, col, rays, and with dn the guide outputs noisy, direct, albedo,
    position, normal and what the chain made on the way (E, T, M, variance, F, VF, prev_position, prev_normal)"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim, px, c, traced = pre or inputs(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter, counts, y0, y1, info)
    out = {"px": px, "col": c, "rays": traced}
    if dn is None:
        return out
    out.update({"noisy": c, "direct": D, "albedo": A, "position": P, "normal": N})
    iterations, normal_power, sigma_z, sigma_l = dn
    if tp is None and iterations == 0:   # the path frame's own end, no demodulation round trip
        return out
    Q = Nq = None
    if motion:
        Q, Nq = (a.reshape(y1 - y0, w, 4) for a in mr.previous_positions(scene, snap, prim["hits"]))
        out["prev_position"], out["prev_normal"] = Q, Nq
    hit = P[..., 3] != 0
    with np.errstate(all="ignore"):
        E = np.where(A > 0, (c - D) / A, f32(0.0)).astype(np.float32)
        E[~hit] = 0.0
        out["E"] = E
        if vp is not None:
            epsilon, min_len, radius = vp
            T, M = vr.step(E, P, N, hist, cam14, w, h, y0, y1, tp, Q, Nq, stats)
            V0 = vr.initial_variance(hist, normal_power, sigma_z, min_len, radius, stats)
            F, VF = vr.atrous_v(T[..., :3], V0, P, N, iterations, normal_power, sigma_z, sigma_l, epsilon, stats)
            out["T"], out["M"], out["variance"], out["VF"] = T, M, V0, VF
        elif tp is not None:
            T = mr.step(E, P, N, Q, Nq, hist, cam14, w, h, y0, y1, tp, stats) if motion else tr.step(E, P, N, hist, cam14, w, h, y0, y1, tp, stats)
            F = dr.atrous(T[..., :3], P, N, *dn)
            out["T"] = T
        else:
            F = dr.atrous(E, P, N, iterations, normal_power, sigma_z, sigma_l, stats)
        col = np.where(hit[..., None], D + A * F, D).astype(np.float32)
    out["F"] = F
    out["px"], out["col"] = cr.pack_rgb8(col.reshape(-1, 3)).reshape(y1 - y0, w), col
    return out
