"""numpy restatement of variance guidance: the step with moments T_v (vxrt_temporal_accumulate_moments), the initial variance V0
(vxrt_history_variance), the variance-guided filter atrous_v (vxrt_denoise_variance) and the frame (vxrt_render_path_variance).  TEST
INFRASTRUCTURE ONLY.

The definition is the header's "Variance guidance", one numpy float32 operation per + - * / sqrt, in the order written there.
  T_v      step(): the header defines T_v as T (or T_m) with additions, so `out` IS temporal_ref.step (motion_ref.step) on the plain part
           of the history.  The moments are the same step once more: s1, s2, M1, M2, m1, m2 are, symbol for symbol, what T computes for
           the first two channels of a signal (lE, lE * lE, .) on a history whose HE is (HM.x, HM.y, ., len) -- the taps kept, their
           weights, sw, sl, L1 and al depend on the guides and on len alone, and `else out = E` is `else m1 = lE, m2 = lE * lE`.  What the
           substitution does not carry is the pixel that is not a hit, whose moments are 0.
  V0       initial_variance(): every tap of the window side by side, in the definition's order
  atrous_v atrous_v(): denoise_ref.atrous's loop with the prefiltered variance, the per-pixel scale and the variance sum
  frame    path_frame(): temporal_ref.path_frame / motion_ref.path_frame with T_v, V0 and atrous_v
`stats` (optional dict) counts what tests/test_variance_cpu.py needs to show that a case is not vacuous."""
import numpy as np

import camera_ref as cr
import denoise_ref as dr
import motion_ref as mr
import path_ref as pr
import temporal_ref as tr

f32 = np.float32
KK = np.array([0.25, 0.5, 0.25], np.float32)


def _count(stats, key, n):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(n)


def _max0(a):
    """max(a, 0) = a < 0 ? 0 : a"""
    return np.where(a < 0, f32(0.0), a).astype(np.float32)


class History:
    """a vxrt_history_t with moments: the plain history `h` (temporal_ref.History) and HM (rows, W, 2) of the last frame"""

    def __init__(self):
        self.h = tr.History()
        self.HM = None

    def reset(self):
        self.h.reset()
        self.HM = None

    def copy(self):
        c = History()
        c.h, c.HM = self.h.copy(), None if self.HM is None else self.HM.copy()
        return c


def step(E, P, N, hist, cam14, W, H, y0, y1, prm, Q=None, Nq=None, stats=None):
    """(out, HM) = T_v(E, P, N[, Q, N']; hist, hist.h.cam, prm): out (rows, W, 4) as temporal_ref.step / motion_ref.step, HM (rows, W, 2).
    Makes them, P, N, cam14 the history."""
    E, P, N = (np.array(a, np.float32) for a in (E, P, N))
    hit = P[..., 3] != 0
    have = (not hist.h.empty) and hist.h.geom == (W, H, y0, y1)
    hm = hist.h.copy()
    with np.errstate(all="ignore"):
        lE = dr.lum(E)
        Em = np.stack([lE, lE * lE, np.zeros_like(lE)], -1).astype(np.float32)
    if have:
        hm.HE = np.concatenate([hist.HM, np.zeros_like(hist.HM[..., :1]), hist.h.HE[..., 3:4]], -1).astype(np.float32)
    if Q is None:
        out = tr.step(E, P, N, hist.h, cam14, W, H, y0, y1, prm, stats)
        om = tr.step(Em, P, N, hm, cam14, W, H, y0, y1, prm)
    else:
        out = mr.step(E, P, N, Q, Nq, hist.h, cam14, W, H, y0, y1, prm, stats)
        om = mr.step(Em, P, N, Q, Nq, hm, cam14, W, H, y0, y1, prm)
    assert (om[..., 3].view(np.uint32) == out[..., 3].view(np.uint32)).all()     # (the same taps, the same al)
    hist.HM = np.where(hit[..., None], om[..., :2], f32(0.0)).astype(np.float32)
    return out, hist.HM.copy()


def temporal_variance(HM):
    """vt = max(m2 - m1 * m1, 0)"""
    with np.errstate(all="ignore"):
        return _max0(HM[..., 1] - HM[..., 0] * HM[..., 0])


def initial_variance(hist, normal_power, sigma_z, min_len, radius, stats=None):
    """V0 (rows, W) of the history's current set"""
    A, P, N = hist.h.HE, hist.h.HP, hist.h.HN
    rows, w = A.shape[:2]
    hit = P[..., 3] != 0
    fmin = f32(min_len)
    with np.errstate(all="ignore"):
        vt = temporal_variance(hist.HM)
        long = hit & (A[..., 3] >= fmin)
        need = hit & ~long
        LA = dr.lum(A)
        sw = np.zeros((rows, w), np.float32)
        s1 = np.zeros((rows, w), np.float32)
        s2 = np.zeros((rows, w), np.float32)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                ylo, yhi, xlo, xhi = max(0, -dy), min(rows, rows - dy), max(0, -dx), min(w, w - dx)
                if ylo >= yhi or xlo >= xhi:
                    continue
                ps = (slice(ylo, yhi), slice(xlo, xhi))
                qs = (slice(ylo + dy, yhi + dy), slice(xlo + dx, xhi + dx))
                ok = hit[ps] & hit[qs]
                d = dr.dot(N[ps], N[qs])
                dn = np.where(d > 0, d, f32(0.0)).astype(np.float32)
                for _ in range(normal_power):
                    dn = dn * dn
                t = np.abs(dr.dot(N[ps], P[qs][..., :3] - P[ps][..., :3])) / f32(sigma_z)
                wz = f32(1.0) / (f32(1.0) + t * t)
                wgt = dn * wz
                take = ok & (wgt > 0)
                l = LA[qs]
                sw[ps] = np.where(take, sw[ps] + wgt, sw[ps])
                s1[ps] = np.where(take, s1[ps] + wgt * l, s1[ps])
                s2[ps] = np.where(take, s2[ps] + wgt * (l * l), s2[ps])
        a1 = s1 / sw
        vs = _max0(s2 / sw - a1 * a1)
        spatial = vs * (fmin / A[..., 3])
        V0 = np.where(need & (sw > 0), spatial, vt)
        V0 = np.where(hit, V0, f32(0.0)).astype(np.float32)
    _count(stats, "v0_miss", (~hit).sum())
    _count(stats, "v0_temporal", long.sum())
    _count(stats, "v0_spatial", (need & (sw > 0)).sum())
    _count(stats, "v0_spatial_sw0", (need & ~(sw > 0)).sum())
    return V0


def atrous_v(S, V, P, N, iterations, normal_power, sigma_z, sigma_l, epsilon, stats=None):
    """(F, VF) = atrous_v(S, V, P, N, dn, vp): S (rows, w, 3), V (rows, w), P and N (rows, w, 4)"""
    cur, var = np.array(S, np.float32), np.array(V, np.float32)
    P, N = np.asarray(P, np.float32), np.asarray(N, np.float32)
    rows, w = cur.shape[:2]
    hit = P[..., 3] != 0
    sz, sl, eps = f32(sigma_z), f32(sigma_l), f32(epsilon)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            step_ = 1 << i
            gw = np.zeros((rows, w), np.float32)
            gs = np.zeros((rows, w), np.float32)
            ntap = np.zeros((rows, w), np.int64)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    ylo, yhi, xlo, xhi = max(0, -dy), min(rows, rows - dy), max(0, -dx), min(w, w - dx)
                    if ylo >= yhi or xlo >= xhi:
                        continue
                    ps = (slice(ylo, yhi), slice(xlo, xhi))
                    qs = (slice(ylo + dy, yhi + dy), slice(xlo + dx, xhi + dx))
                    ok = hit[ps] & hit[qs]
                    c = KK[dy + 1] * KK[dx + 1]
                    gw[ps] = np.where(ok, gw[ps] + c, gw[ps])
                    gs[ps] = np.where(ok, gs[ps] + c * var[qs], gs[ps])
                    ntap[ps] += ok
            g = gs / gw
            den = sl * np.sqrt(g) + eps
            _count(stats, "prefilter_short", (hit & (ntap < 9)).sum())
            _count(stats, "nan_scale", (hit & np.isnan(den)).sum())
            L = dr.lum(cur)
            sw = np.zeros((rows, w), np.float32)
            sc = np.zeros((rows, w, 3), np.float32)
            sv = np.zeros((rows, w), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = step_ * dy, step_ * dx
                    ylo, yhi, xlo, xhi = max(0, -oy), min(rows, rows - oy), max(0, -ox), min(w, w - ox)
                    if ylo >= yhi or xlo >= xhi:
                        continue
                    ps = (slice(ylo, yhi), slice(xlo, xhi))
                    qs = (slice(ylo + oy, yhi + oy), slice(xlo + ox, xhi + ox))
                    ok = hit[ps] & hit[qs]
                    h = dr.K[dy + 2] * dr.K[dx + 2]
                    d = dr.dot(N[ps], N[qs])
                    dn = np.where(d > 0, d, f32(0.0)).astype(np.float32)
                    for _ in range(normal_power):
                        dn = dn * dn
                    t = np.abs(dr.dot(N[ps], P[qs][..., :3] - P[ps][..., :3])) / sz
                    wz = f32(1.0) / (f32(1.0) + t * t)
                    u = np.abs(L[ps] - L[qs]) / den[ps]
                    wc = f32(1.0) / (f32(1.0) + u * u)
                    wgt = ((h * dn) * wz) * wc
                    take = ok & (wgt > 0)
                    sw[ps] = np.where(take, sw[ps] + wgt, sw[ps])
                    sc[ps] = np.where(take[..., None], sc[ps] + wgt[..., None] * cur[qs], sc[ps])
                    sv[ps] = np.where(take, sv[ps] + (wgt * wgt) * var[qs], sv[ps])
            good = hit & (sw > 0)
            _count(stats, "all_dropped", (hit & ~(sw > 0)).sum())
            _count(stats, "all_dropped_nan", (hit & ~(sw > 0) & np.isnan(den)).sum())
            _count(stats, "variance_pass_miss", (~hit).sum())
            cur = np.where(good[..., None], sc / sw[..., None], cur).astype(np.float32)
            var = np.where(good, sv / (sw * sw), var).astype(np.float32)
    return cur, var


def path_inputs(scene, cam14, w, h, params, spp, bounces, seed, shadow, y0=0, y1=None):
    """what a frame is made from, whatever its history and motion: (D, A, P, N, prim) of denoise_ref.path_guides and (c, rays traced) of
    path_ref.frame -- the expensive part, which the frames of one scene, camera and seed share"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim = dr.path_guides(scene, cam14, w, h, params, shadow, y0, y1)
    _, c, traced, _ = pr.frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, y0, y1, prim)
    return D, A, P, N, prim, c, traced


def path_frame(scene, snap, cam14, w, h, params, spp, bounces, seed, shadow, dn, tp, vp, hist, motion=0, y0=0, y1=None, pre=None, stats=None):
    """vxrt_render_path_variance over rows [y0, y1); dn = (iterations, normal_power, sigma_z, sigma_l), tp = the step's prm, vp =
    (epsilon, min_len, radius); motion = 1 takes snapshot `snap` (motion_ref.snapshot); pre = path_inputs() of the same arguments.
    temporal_ref.path_frame's dict with M (the moments), variance (V0; computed whatever iterations is: the optional output) and VF"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim, c, traced = pre or path_inputs(scene, cam14, w, h, params, spp, bounces, seed, shadow, y0, y1)
    out = {"noisy": c, "direct": D, "albedo": A, "position": P, "normal": N, "rays": traced}
    Q = Nq = None
    if motion:
        Q, Nq = (a.reshape(y1 - y0, w, 4) for a in mr.previous_positions(scene, snap, prim["hits"]))
        out["prev_position"], out["prev_normal"] = Q, Nq
    hit = P[..., 3] != 0
    iterations, normal_power, sigma_z, sigma_l = dn
    epsilon, min_len, radius = vp
    with np.errstate(all="ignore"):
        E = np.where(A > 0, (c - D) / A, f32(0.0)).astype(np.float32)
        E[~hit] = 0.0
        T, M = step(E, P, N, hist, cam14, w, h, y0, y1, tp, Q, Nq, stats)
        V0 = initial_variance(hist, normal_power, sigma_z, min_len, radius, stats)
        F, VF = atrous_v(T[..., :3], V0, P, N, iterations, normal_power, sigma_z, sigma_l, epsilon, stats)
        col = np.where(hit[..., None], D + A * F, D).astype(np.float32)
    out["E"], out["T"], out["M"], out["variance"], out["F"], out["VF"] = E, T, M, V0, F, VF
    out["px"], out["col"] = cr.pack_rgb8(col.reshape(-1, 3)).reshape(y1 - y0, w), col
    return out
