"""numpy restatement of the guided a-trous filter (vxrt_denoise) and of the denoised path frame (vxrt_render_path_denoised).  TEST
INFRASTRUCTURE ONLY.

The definition in include/vortex_hip.h, one numpy float32 operation per + - * /, in the order written there.  The 25 taps are visited
in the definition's order (dy outer, dx inner); every pixel of the window is carried side by side per tap.  The path frame composes
pieces that are pinned elsewhere:
  c  (the path frame's colour)   path_ref.frame_from_rays
  D  = Lit(r_0, h_0)             path_ref.lit
  A  = Alb(h_0)                  camera_secondary_ref.albedo
  I, N of the primary hit        camera_ref._normal_and_point
  RGB8 pack                      camera_ref.pack_rgb8
`stats` (optional dict) counts what tests/test_denoise_cpu.py needs to show that a case is not vacuous."""
import numpy as np

import camera_ref as cr
import camera_secondary_ref as csr
import path_ref as pr
from camera_ref import po

f32 = np.float32
K = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16], np.float32)
MAX_ITERATIONS = 6


def lum(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _count(stats, key, n):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(n)


def atrous(S, P, N, iterations, normal_power, sigma_z, sigma_l, stats=None):
    """F = atrous(S, P, N, prm): S (rows, w, 3), P and N (rows, w, 4), all float32"""
    cur = np.array(S, np.float32)
    P, N = np.asarray(P, np.float32), np.asarray(N, np.float32)
    rows, w = cur.shape[:2]
    hit = P[..., 3] != 0
    sz = f32(sigma_z)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            step = 1 << i
            sl = f32(sigma_l) * f32(2.0 ** -i)
            L = lum(cur)
            sw = np.zeros((rows, w), np.float32)
            sc = np.zeros((rows, w, 3), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = step * dy, step * dx
                    ylo, yhi, xlo, xhi = max(0, -oy), min(rows, rows - oy), max(0, -ox), min(w, w - ox)
                    if ylo >= yhi or xlo >= xhi:
                        _count(stats, "skip_window", hit.sum())
                        continue
                    ps = (slice(ylo, yhi), slice(xlo, xhi))
                    qs = (slice(ylo + oy, yhi + oy), slice(xlo + ox, xhi + ox))
                    _count(stats, "skip_window", hit.sum() - hit[ps].sum())
                    ok = hit[ps] & hit[qs]
                    _count(stats, "skip_miss", (hit[ps] & ~hit[qs]).sum())
                    h = K[dy + 2] * K[dx + 2]
                    d = dot(N[ps], N[qs])
                    dn = np.where(d > 0, d, f32(0.0)).astype(np.float32)
                    for _ in range(normal_power):
                        dn = dn * dn
                    t = np.abs(dot(N[ps], P[qs][..., :3] - P[ps][..., :3])) / sz
                    wz = f32(1.0) / (f32(1.0) + t * t)
                    u = np.abs(L[ps] - L[qs]) / sl
                    wc = f32(1.0) / (f32(1.0) + u * u)
                    wgt = ((h * dn) * wz) * wc
                    take = ok & (wgt > 0)
                    _count(stats, "skip_weight", (ok & ~(wgt > 0)).sum())
                    _count(stats, "low_dn", (ok & (dn < 0.5)).sum())
                    _count(stats, "low_wz", (ok & (wz < 0.5)).sum())
                    _count(stats, "low_wc", (ok & (wc < 0.5)).sum())
                    _count(stats, "taps", take.sum())
                    sw[ps] = np.where(take, sw[ps] + wgt, sw[ps])
                    sc[ps] = np.where(take[..., None], sc[ps] + wgt[..., None] * cur[qs], sc[ps])
            good = hit & (sw > 0)
            _count(stats, "pass_through", (hit & ~(sw > 0)).sum())
            cur = np.where(good[..., None], sc / sw[..., None], cur).astype(np.float32)
    return cur


def path_guides(scene, cam14, w, h, params, shadow, y0=0, y1=None, prim=None):
    """the primary hit's buffers over rows [y0, y1): D (rows, w, 3) = Lit_0 | background, A (rows, w, 3) = Alb_0 | 0, P (rows, w, 4) =
    (I, 1) | 0, N (rows, w, 4) = (N, 0) | 0, and the primary pass (path_ref.primary) they came from"""
    y1 = h if y1 is None else y1
    rows = y1 - y0
    if prim is None:
        prim = pr.primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))
    rays, hits0 = prim["rays"], prim["hits"]
    n = len(rays)
    p1 = pr._params(params)
    D = np.tile(np.asarray(p1.background, np.float32), (n, 1)).astype(np.float32)
    A = np.zeros((n, 3), np.float32)
    P = np.zeros((n, 4), np.float32)
    N = np.zeros((n, 4), np.float32)
    fi = np.nonzero(hits0["dist"] != pr.LARGE)[0]
    if len(fi):
        D[fi] = pr.lit(scene, rays[fi], hits0[fi], p1, shadow)[0]
        A[fi] = csr.albedo(scene, hits0[fi])
        with np.errstate(all="ignore"):
            I, Nn, _ = cr._normal_and_point(scene, rays[fi], hits0[fi])
        P[fi, 0:3] = np.stack(I, 1)
        P[fi, 3] = 1.0
        N[fi, 0:3] = np.stack(Nn, 1)
    return D.reshape(rows, w, 3), A.reshape(rows, w, 3), P.reshape(rows, w, 4), N.reshape(rows, w, 4), prim


def path_frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, dn, y0=0, y1=None, prim=None, stats=None):
    """the denoised path frame of rows [y0, y1); dn = (iterations, normal_power, sigma_z, sigma_l).  A dict: px (rows, w) u32, col
    (rows, w, 3), rays (traced), and the five guide outputs noisy, direct, albedo (rows, w, 3), position, normal (rows, w, 4)"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim = path_guides(scene, cam14, w, h, params, shadow, y0, y1, prim)
    px, c, traced, _ = pr.frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, y0, y1, prim)
    out = {"noisy": c, "direct": D, "albedo": A, "position": P, "normal": N, "rays": traced}
    iterations, normal_power, sigma_z, sigma_l = dn
    if iterations == 0:   # vxrt_render_path, no demodulation round trip
        out["px"], out["col"] = px, c
        return out
    hit = P[..., 3] != 0
    with np.errstate(all="ignore"):
        E = np.where(A > 0, (c - D) / A, f32(0.0)).astype(np.float32)
        E[~hit] = 0.0
        F = atrous(E, P, N, iterations, normal_power, sigma_z, sigma_l, stats)
        col = np.where(hit[..., None], D + A * F, D).astype(np.float32)
    out["E"], out["F"] = E, F
    out["px"], out["col"] = cr.pack_rgb8(col.reshape(-1, 3)).reshape(y1 - y0, w), col
    return out
