"""numpy restatement of temporal accumulation (vxrt_temporal_accumulate) and of the path frame that uses it (vxrt_render_path_temporal).
TEST INFRASTRUCTURE ONLY.

The definition in include/vortex_hip.h, one numpy float32 operation per + - * /, in the order written there; the reciprocal basis of the
previous camera in float64, by the header's rule.  Every pixel of the window is carried side by side; the four taps are visited in the
definition's order.  The path frame composes pieces that are pinned elsewhere: denoise_ref.path_guides (D, A, P, N), path_ref.frame (c),
denoise_ref.atrous (the filter) and camera_ref.pack_rgb8.
`stats` (optional dict) counts every outcome of the step, so that tests/test_temporal_cpu.py can show that a case is not vacuous:
  miss, empty_history, behind, outside          pixels that never reach the taps
  skip_window, skip_invalid, skip_normal, skip_plane     taps, by the first reason that drops them
  taps_0, taps_some, taps_4                     pixels inside the previous window, by the number of taps they accumulate
  blended, capped                               pixels that take history; those whose length max_len cuts"""
import numpy as np

import camera_ref as cr
import denoise_ref as dr
import path_ref as pr

f32 = np.float32
MAX_LEN = 1024


class History:
    """vxrt_history_t: HE, HP, HN of the last frame with its camera and geometry"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.empty = True
        self.HE = self.HP = self.HN = self.cam = self.geom = None

    def copy(self):
        h = History()
        h.empty, h.geom = self.empty, self.geom
        h.HE, h.HP, h.HN, h.cam = (None if a is None else a.copy() for a in (self.HE, self.HP, self.HN, self.cam))
        return h


def reciprocal_basis(cam14):
    """Rr, Ur, Fr of the camera, float32 (3,) each: float64 arithmetic, one rounding at the end"""
    c = np.asarray(cam14, np.float32).astype(np.float64)
    F, R, U = c[3:6], c[6:9], c[9:12]

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float64)

    UF, FR, RU = cross(U, F), cross(F, R), cross(R, U)
    det = (R[0] * UF[0] + R[1] * UF[1]) + R[2] * UF[2]
    with np.errstate(all="ignore"):
        return tuple((v / det).astype(np.float32) for v in (UF, FR, RU))


def _count(stats, key, n):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(n)


def step(E, P, N, hist, cam14, W, H, y0, y1, prm, stats=None):
    """out = T(E, P, N; hist, hist.cam, prm) over rows [y0, y1) of a W x H frame seen from cam14: E (rows, W, 3), P and N (rows, W, 4),
    prm = (alpha_min, max_len, sigma_z, normal_min).  Returns out (rows, W, 4) and makes it, P, N, cam14 the history."""
    alpha_min, max_len, sigma_z, normal_min = prm
    E, P, N = (np.array(a, np.float32) for a in (E, P, N))
    rows, w = y1 - y0, W
    assert E.shape == (rows, w, 3) and P.shape == (rows, w, 4) and N.shape == (rows, w, 4)
    hit = P[..., 3] != 0
    out = np.empty((rows, w, 4), np.float32)
    out[..., :3] = E
    out[..., 3] = np.where(hit, f32(1.0), f32(0.0))
    have = (not hist.empty) and hist.geom == (W, H, y0, y1)
    _count(stats, "miss", (~hit).sum())
    if not have:
        _count(stats, "empty_history", hit.sum())
    else:
        with np.errstate(all="ignore"):
            cp = np.asarray(hist.cam, np.float32)
            Rr, Ur, Fr = reciprocal_basis(cp)
            I = P[..., :3]
            d = I - cp[0:3]
            a, b, c = dr.dot(d, Rr), dr.dot(d, Ur), dr.dot(d, Fr)
            front = hit & (c > 0)
            fx = (((a / c) / cp[12]) + f32(0.5)) * f32(W) - f32(0.5)
            fy = ((((b / c) / cp[13]) + f32(0.5)) * f32(H) - f32(0.5)) - f32(y0)
            inside = front & (fx > -1) & (fx < f32(W)) & (fy > -1) & (fy < f32(rows))
            _count(stats, "behind", (hit & ~front).sum())
            _count(stats, "outside", (front & ~inside).sum())
            flx, fly = np.floor(fx), np.floor(fy)
            tx, ty = fx - flx, fy - fly
            x0 = np.where(inside, flx, f32(0.0)).astype(np.int64)
            yy = np.where(inside, fly, f32(0.0)).astype(np.int64)
            sw = np.zeros((rows, w), np.float32)
            se = np.zeros((rows, w, 3), np.float32)
            sl = np.zeros((rows, w), np.float32)
            taken = np.zeros((rows, w), np.int64)
            for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
                qx, qy = x0 + i, yy + j
                inwin = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < rows)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, rows - 1)
                he, hp, hn = hist.HE[cy, cx], hist.HP[cy, cx], hist.HN[cy, cx]
                valid = (hp[..., 3] != 0) & (he[..., 3] > 0)
                nok = dr.dot(N, hn) >= f32(normal_min)
                pok = (np.abs(dr.dot(N, hp[..., :3] - I)) / f32(sigma_z)) <= 1
                k1 = inwin
                k2 = k1 & valid
                k3 = k2 & nok
                k4 = k3 & pok
                _count(stats, "skip_window", (inside & ~k1).sum())
                _count(stats, "skip_invalid", (k1 & ~k2).sum())
                _count(stats, "skip_normal", (k2 & ~k3).sum())
                _count(stats, "skip_plane", (k3 & ~k4).sum())
                wgt = (tx if i else f32(1.0) - tx) * (ty if j else f32(1.0) - ty)
                take = k4 & (wgt > 0)
                sw = np.where(take, sw + wgt, sw)
                se = np.where(take[..., None], se + wgt[..., None] * he[..., :3], se)
                sl = np.where(take, sl + wgt * he[..., 3], sl)
                taken += take
            good = inside & (sw > 0)
            Eh = se / sw[..., None]
            L = sl / sw
            Lp = L + f32(1.0)
            L1 = np.where(f32(max_len) < Lp, f32(max_len), Lp)          # min(a, b) = b < a ? b : a
            r1 = f32(1.0) / L1
            al = np.where(r1 < f32(alpha_min), f32(alpha_min), r1)     # max(a, b) = a < b ? b : a
            blended = Eh + al[..., None] * (E - Eh)
            out[..., :3] = np.where(good[..., None], blended, E)
            out[..., 3] = np.where(good, L1, out[..., 3])
            _count(stats, "taps_0", (inside & (taken == 0)).sum())
            _count(stats, "taps_some", (inside & (taken > 0) & (taken < 4)).sum())
            _count(stats, "taps_4", (inside & (taken == 4)).sum())
            _count(stats, "blended", good.sum())
            _count(stats, "capped", (good & (f32(max_len) < Lp)).sum())
    hist.empty = False
    hist.HE, hist.HP, hist.HN = out.copy(), P.copy(), N.copy()
    hist.cam, hist.geom = np.array(cam14, np.float32), (W, H, y0, y1)
    return out


def path_frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, dn, tp, hist, y0=0, y1=None, prim=None, stats=None):
    """vxrt_render_path_temporal over rows [y0, y1); dn = (iterations, normal_power, sigma_z, sigma_l), tp = the step's prm.  A dict as
    denoise_ref.path_frame's, with E (demodulated), T (the step's out, which is the history's HE) and F (filtered)"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim = dr.path_guides(scene, cam14, w, h, params, shadow, y0, y1, prim)
    px, c, traced, _ = pr.frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, y0, y1, prim)
    out = {"noisy": c, "direct": D, "albedo": A, "position": P, "normal": N, "rays": traced}
    hit = P[..., 3] != 0
    with np.errstate(all="ignore"):
        E = np.where(A > 0, (c - D) / A, f32(0.0)).astype(np.float32)
        E[~hit] = 0.0
        T = step(E, P, N, hist, cam14, w, h, y0, y1, tp, stats)
        F = dr.atrous(T[..., :3], P, N, *dn)
        col = np.where(hit[..., None], D + A * F, D).astype(np.float32)
    out["E"], out["T"], out["F"] = E, T, F
    out["px"], out["col"] = cr.pack_rgb8(col.reshape(-1, 3)).reshape(y1 - y0, w), col
    return out
