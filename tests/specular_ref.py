"""numpy restatement of specular vertices in path frames (include/vortex_hip.h, "Specular vertices"; vxrt_render_path_frame_specular and
vxrt_specular_pick).  TEST INFRASTRUCTURE ONLY.

The frame is tests/path_ref.py's, piece for piece, with the additions of the definition, composed of pieces that are pinned elsewhere:
  closest hit, I, N, reflectivity   camera_ref._trace, camera_ref._normal_and_point
  Lit and `term`                    path_ref.lit -- `term` is Lit with background = 0, as camera_ref._radiance takes it for its mirror arm
  the mirror ray                    the arithmetic of camera_ref._radiance, operation for operation
  the diffuse bounce ray            path_ref.bounce_rays
  the pick's seed, xi               emissive_ref.path_seeds / xorshift / to_float with the user seed's bit 30 flipped
  emitter rays, Emi, weights        emissive_ref / emissive_mis_ref (tables, emitter_rays, emission, hit_weights)
  counts                            adaptive_ref.clamp, one uniform frame per distinct clamped count, as path_frame_ref.colour
tests/test_specular_cpu.py holds it to the three identities of the definition and shows that the GPU cases are not vacuous.

An emitter form is None, ("nee0", scale), ("nee1", scale, tab) or ("mis", scale, tab, idx), as tests/path_frame_ref.py takes it."""
import numpy as np

import adaptive_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import emissive_mis_ref as mir
import emissive_ref as er
import path_ref as pr
from camera_ref import po

f32 = np.float32
u32 = np.uint32
LARGE = cr.LARGE
PICK_BIT = 0x40000000
EMITTER_BIT = 0x80000000
INFO_KEYS = ("mirror", "diffuse_at_specular", "specular_emitter", "skipped_by_mirror")


def is_specular(rho):
    """rho > 0 and finite: NaN, +-inf and rho <= 0 are not"""
    rho = np.asarray(rho, np.float32)
    with np.errstate(all="ignore"):
        return (rho > f32(0.0)) & np.isfinite(rho)


def pick(rho, seeds):
    """(mirror (n,) bool, xi (n,) f32) of hash outputs `seeds` (0 becomes 1) at vertices of reflectivity rho: one xorshift step"""
    rho = np.asarray(rho, np.float32)
    s = np.asarray(seeds, np.uint32).copy()
    s[s == 0] = 1
    xi = er.to_float(er.xorshift(s))
    with np.errstate(all="ignore"):
        return is_specular(rho) & ((rho >= f32(1.0)) | (xi < rho)), xi


def mirror_rays(I, N, d):
    """closest.cpp:96-99 as camera_ref._radiance restates it: R = normalize(d - (2 N) (N . d)), origin I + R * 0.001; N is not turned"""
    I, N, d = (np.asarray(v, np.float32).reshape(-1, 3) for v in (I, N, d))
    with np.errstate(all="ignore"):
        dn = N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1] + N[:, 2] * d[:, 2]
        v = [d[:, k] - (f32(2.0) * N[:, k]) * dn for k in range(3)]
        inv = f32(1.0) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        R = [v[k] * inv for k in range(3)]
        return np.stack([I[:, 0] + R[0] * f32(0.001), I[:, 1] + R[1] * f32(0.001), I[:, 2] + R[2] * f32(0.001), R[0], R[1], R[2]], 1).astype(np.float32)


def pick_step(vertices, seeds):
    """vxrt_specular_pick: vertices (n, 10) = I, N, dir, rho -> (rays (n, 6), lobe (n,) u32); a diffuse pick has six zeros"""
    v = np.asarray(vertices, np.float32).reshape(-1, 10)
    m, _ = pick(v[:, 9], seeds)
    rays = np.zeros((len(v), 6), np.float32)
    if m.any():
        rays[m] = mirror_rays(v[m, 0:3], v[m, 3:6], v[m, 6:9])
    return rays, m.astype(np.uint32)


def _lit_split(scene, r, h, params, p_term, shadow, term_sel):
    """Lit of the hits, `term` alone (background = 0) where term_sel: colours, occlusion rays traced"""
    col, nocc = np.zeros((len(r), 3), np.float32), 0
    for sel, p in ((term_sel, p_term), (~term_sel, params)):
        if sel.any():
            c, _, k = pr.lit(scene, r[sel], h[sel], p, shadow)
            col[sel] = c
            nocc += k
    return col, nocc


def frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed, shadow, emitter=None, prim=None, info=None, samples=False, force0=None):
    """the frame with specular vertices over `rays`: pixels (n,) u32, colours (n, 3), rays traced.  info (optional dict) counts per depth
    the mirror picks, the diffuse picks at specular vertices, the specular segments that found an emitter and the emitter rays a mirror
    pick skipped, and in "specular_vertices" every specular vertex any path met.  samples = True returns (fi, Lc (m, spp, 3), traced,
    rho_0 (m,)) in place of the pixels.  force0 = "mirror" / "diffuse": no draw at depth 0 -- every specular vertex there takes that lobe
    (the deterministic split of tests/test_specular_cpu.py)."""
    info = {} if info is None else info
    for key in INFO_KEYS:
        info.setdefault(key, [0] * bounces)
    info.setdefault("specular_vertices", 0)
    params = pr._params(params)
    p_term = cr._with(params, background=(0.0, 0.0, 0.0))
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
        return (fi, np.zeros((0, spp, 3), np.float32), traced, np.zeros(0, np.float32)) if samples else (cr.pack_rgb8(col), col, traced)
    r0, h0 = rays[fi], hits0[fi]
    with np.errstate(all="ignore"):
        _, _, rho0 = cr._normal_and_point(scene, r0, h0)
        spec0 = is_specular(rho0)
        info["specular_vertices"] += int(spec0.sum())
        lit0, nocc = _lit_split(scene, r0, h0, params, p_term, shadow, spec0 & (bounces > 0))
        traced += nocc
        if form is not None:
            em0, E0 = er.emission(scene, h0, scale)
            lit0[em0] = lit0[em0] + E0[em0]
        m = len(fi)
        Lc = np.repeat(lit0, spp, 0).astype(np.float32)
        thr = np.ones((m * spp, 3), np.float32)
        pxs, pys = np.repeat(np.asarray(xs)[fi], spp), np.repeat(np.asarray(ys)[fi], spp)
        smp = np.tile(np.arange(spp, dtype=np.uint32), m)
        alive = np.arange(m * spp)
        r, h = np.repeat(r0, spp, 0), np.repeat(h0, spp, 0)
        for k in range(bounces):
            if len(alive) == 0:
                continue
            I, N, rho = cr._normal_and_point(scene, r, h)
            I, N = np.stack(I, 1).astype(np.float32), np.stack(N, 1).astype(np.float32)
            d = r[:, 3:6]
            ax, ay, asmp = pxs[alive], pys[alive], smp[alive]
            user = (seed + k) & 0xFFFFFFFF
            spec = is_specular(rho)
            mirror, _ = pick(rho, er.path_seeds(ax, ay, w, spp, asmp, user ^ PICK_BIT))
            if k == 0 and force0 is not None:
                mirror = spec.copy() if force0 == "mirror" else np.zeros(len(alive), bool)
            dif = ~mirror
            info["mirror"][k] += int(mirror.sum())
            info["diffuse_at_specular"][k] += int((spec & dif).sum())
            di = alive[dif]
            thr[di] = thr[di] * csr.albedo(scene, h[dif])
            sec = np.zeros((len(alive), 6), np.float32)
            if dif.any():
                sec[dif] = pr.bounce_rays(ax[dif], ay[dif], w, spp, asmp[dif], seed + k, I[dif], N[dif], d[dif])
            if mirror.any():
                sec[mirror] = mirror_rays(I[mirror], N[mirror], d[mirror])
            Nf = mir._facing(N, d)
            if tab is not None:
                info["skipped_by_mirror"][k] += int(mirror.sum())
                if dif.any():
                    seeds = er.path_seeds(ax[dif], ay[dif], w, spp, asmp[dif], user ^ EMITTER_BIT)
                    sample = mir.emitter_rays if form == "mis" else er.emitter_rays
                    erays, et, G, _, real = sample(tab, scale, seeds, I[dif], Nf[dif])[:5]
                    open_ = np.zeros(len(di), bool)
                    if real.any():
                        open_[real] = cr._trace(scene, erays[real], tmax=et[real], any_hit=True)["dist"] == LARGE
                    traced += int(real.sum())
                    oi = di[open_]
                    Lc[oi] = Lc[oi] + thr[oi] * G[open_]
            bh = cr._trace(scene, sec)
            traced += len(alive)
            hit = bh["dist"] != LARGE
            miss_i, hit_i = alive[~hit], alive[hit]
            Lc[miss_i] = Lc[miss_i] + thr[miss_i] * bg
            rh, hh = sec[hit], bh[hit]
            if hit.any():
                _, _, rho_h = cr._normal_and_point(scene, rh, hh)
                spec_h = is_specular(rho_h)
                info["specular_vertices"] += int(spec_h.sum())
                lk, nocc = _lit_split(scene, rh, hh, params, p_term, shadow, spec_h & (k + 1 < bounces))
                traced += nocc
                Lc[hit_i] = Lc[hit_i] + thr[hit_i] * lk
                if form is not None:
                    emk, Ek = er.emission(scene, hh, scale)
                    seg = mirror[hit]
                    info["specular_emitter"][k] += int((emk & seg).sum())
                    full = emk if form == "nee0" else emk & seg          # (after a specular segment: in full in all three forms)
                    ei = hit_i[full]
                    Lc[ei] = Lc[ei] + thr[ei] * Ek[full]
                    weighted = emk & ~seg
                    if form == "mis" and weighted.any():
                        _, wB = mir.hit_weights(tab, emitter[3], rh[weighted], hh[weighted], Nf[hit][weighted])
                        wi = hit_i[weighted]
                        Lc[wi] = Lc[wi] + thr[wi] * (Ek[weighted] * wB[:, None]).astype(np.float32)
            r, h, alive = rh, hh, hit_i
        Lc = Lc.reshape(m, spp, 3)
        if samples:
            return fi, Lc, traced, rho0
        acc = Lc[:, 0].copy()
        for s in range(1, spp):
            acc = acc + Lc[:, s]
        col[fi] = acc / f32(spp)
    return cr.pack_rgb8(col), col, traced


def frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter=None, counts=None, y0=0, y1=None, prim=None, info=None):
    """vxrt_render_path_frame_specular with enable = 1 over rows [y0, y1) seen from cam14 (None: the fixed camera): a dict of px (rows,
    w), col (rows, w, 3), rays.  counts: None, or the full frame's raw counts (h, w) -- spp is then the cap, and pixel p is the uniform
    frame's pixel with spp := n_p"""
    y1 = h if y1 is None else y1
    xs, ys = csr.pixel_grid(w, y0, y1)
    if prim is None:
        prim = pr.primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))
    n = len(prim["rays"])
    if counts is None:
        px, col, traced = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, emitter, prim, info)
    else:
        n_p = ar.clamp(np.asarray(counts).reshape(h, w)[y0:y1].reshape(-1), spp)
        px, col, traced = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), 0
        for v in np.unique(n_p):
            sel = np.nonzero(n_p == v)[0]
            sub = {"rays": prim["rays"][sel], "hits": prim["hits"][sel]}
            p, c, t = frame_from_rays(scene, sub["rays"], xs[sel], ys[sel], w, params, int(v), bounces, seed, shadow, emitter, sub, info)
            px[sel], col[sel] = p, c
            traced += t
    return {"px": px.reshape(y1 - y0, w), "col": col.reshape(y1 - y0, w, 3), "rays": traced}


def _mean_and_error(L, n, n_hit, bg):
    """emissive_ref.sample_means' estimate from per-pixel samples L (m, spp, 3), float64"""
    spp = L.shape[1]
    mean = (L.mean(1).sum(0) + (n - n_hit) * bg) / n
    var = (L.var(1, ddof=1) / spp).sum(0) / (n * n)
    return mean, np.sqrt(var)


def sample_means(scene, cam14, w, h, params, spp, bounces, seed, shadow, emitter=None, split=False, info=None):
    """frame-mean colour (3,) of the frame before the pack and its standard error, in float64, as emissive_ref.sample_means.  split =
    True: the deterministic split at depth 0 in place of the pick -- per sample rho_0 * (forced mirror) + (1 - rho_0) * (forced diffuse)
    at a specular primary vertex, both from the same seed"""
    xs, ys = csr.pixel_grid(w, 0, h)
    prim = pr.primary(scene, cr.rays(cam14, w, h, 0, h))
    args = (scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, emitter, prim)
    if split:
        fi, Lm, _, rho0 = frame_from_rays(*args, samples=True, force0="mirror")
        _, Ld, _, _ = frame_from_rays(*args, samples=True, force0="diffuse")
        p = np.where(is_specular(rho0), np.minimum(rho0.astype(np.float64), 1.0), 0.0)[:, None, None]
        L = p * Lm.astype(np.float64) + (1.0 - p) * Ld.astype(np.float64)
    else:
        fi, Lc, _, _ = frame_from_rays(*args, info=info, samples=True)
        L = Lc.astype(np.float64)
    return _mean_and_error(L, w * h, len(fi), np.asarray(pr._params(params).background, np.float64))
