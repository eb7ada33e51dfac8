"""numpy fp32 restatement of a camera frame (vxrt_render_camera / vxrt_pinhole_rays).  TEST INFRASTRUCTURE ONLY.

rays():  the pinhole GenerateRay of include/vortex_hip.h (vxrt_camera_t), operation for operation.  The library is built with
         -ffp-contract=off and numpy float32 arithmetic rounds every operation, so the bits agree.
frame(): what the frame path does with those rays -- closest hit (pyoracle.trace_canonical), the optional occlusion ray of
         oracle/rt_oracle.c:occluded_toward_light, shading (pyoracle.shade) and the mirror bounce of radiance_of, restated from
         the oracle's static helpers:
           orc_shade with light_color = 0 is the occluded colour, orc_shade with background = 0 the shading term alone;
           the reflected ray needs the hit point I and the shading normal N of shade_terms (rt_oracle.c:490-507)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pyoracle as po   # noqa: E402

f32 = np.float32
LARGE = f32(1e30)
BLAS_STRIDE = 160       # orc_blas_t: bvh_offset, invTransform[16] @4, transform[16], mat_offset, tex w / h, reflectivity @152
TRIEX_STRIDE = 64       # orc_triex_t: N0, N1, N2 @0, 12, 24


def ndc(i, n):
    """(float)((double)(((float)i + 0.5f) / (float)n) - 0.5)"""
    q = (np.asarray(i, np.float32) + f32(0.5)) / f32(n)
    return (q.astype(np.float64) - 0.5).astype(np.float32)


def rays(cam14, w, h, y0=0, y1=None):
    """(n, 6) f32: the ray of pixel (x, y) at x + (y - y0) * w"""
    y1 = h if y1 is None else y1
    c = np.asarray(cam14, np.float32)
    pos, fwd, right, up, vp = c[0:3], c[3:6], c[6:9], c[9:12], c[12:14]
    xs = np.tile(np.arange(w, dtype=np.uint32), y1 - y0)
    ys = np.repeat(np.arange(y0, y1, dtype=np.uint32), w)
    with np.errstate(all="ignore"):
        xvp = ndc(xs, w) * vp[0]
        yvp = ndc(ys, h) * vp[1]
        d = []
        for k in range(3):
            cam = (xvp * right[k] + yvp * up[k]) + fwd[k]
            d.append((cam + pos[k]) - pos[k])
        inv = f32(1.0) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        out = np.empty((len(xs), 6), np.float32)
        out[:, 0:3] = pos
        for k in range(3):
            out[:, 3 + k] = d[k] * inv
    return out


def _trace(scene, r, tmax=None, any_hit=False):
    if len(r) == 0:
        return np.zeros(0, po.HIT_DTYPE)
    return po.trace_mt(po.trace_canonical, scene, r, tmax=tmax, any_hit=any_hit)


def _shade(scene, r, hits, params):
    if len(r) == 0:
        return np.zeros((0, 3), np.float32)
    return po.shade(scene, r, hits, params)[0]


def _with(params, **kw):
    q = po.shade_params(tuple(params.ambient), tuple(params.light_color), tuple(params.light_pos), tuple(params.background), params.max_depth)
    for k, v in kw.items():
        getattr(q, k)[:] = v
    return q


def _normal_and_point(scene, r, hits):
    """shade_terms' I = o + d * dist and N = normalize(M^T-ish transform of the interpolated normal)"""
    blas = np.frombuffer(np.ascontiguousarray(scene["blas"], np.uint8).tobytes(), np.uint8)
    triex = np.frombuffer(np.ascontiguousarray(scene["triEx"], np.uint8).tobytes(), np.uint8)
    bi = hits["blasIdx"].astype(np.int64) & 0x7fffffff
    ti = hits["triIdx"].astype(np.int64)
    m = np.stack([blas[(bi * BLAS_STRIDE + 4 + 4 * k)[:, None] + np.arange(4)].copy().view(np.float32)[:, 0] for k in range(16)], 1)
    nrm = np.stack([triex[(ti * TRIEX_STRIDE + 4 * k)[:, None] + np.arange(4)].copy().view(np.float32)[:, 0] for k in range(9)], 1)
    refl = blas[(bi * BLAS_STRIDE + 152)[:, None] + np.arange(4)].copy().view(np.float32)[:, 0]
    bx, by, bz = hits["bx"], hits["by"], hits["bz"]
    N = [(nrm[:, 3 + k] * bx + nrm[:, 6 + k] * by) + nrm[:, k] * bz for k in range(3)]
    Nt = [((m[:, k] * N[0] + m[:, 4 + k] * N[1]) + m[:, 8 + k] * N[2]) + f32(0.0) * f32(0.0) for k in range(3)]
    inv = f32(1.0) / np.sqrt(Nt[0] * Nt[0] + Nt[1] * Nt[1] + Nt[2] * Nt[2])
    N = [Nt[k] * inv for k in range(3)]
    I = [r[:, k] + r[:, 3 + k] * hits["dist"] for k in range(3)]
    return I, N, refl


def _radiance(scene, r, params, shadow, bounce, counter):
    """colours (n, 3) and hit records (bit 31 of blasIdx = occluded) of rays r at bounce level `bounce`"""
    n = len(r)
    hits = _trace(scene, r)
    counter[0] += n
    found = hits["dist"] != LARGE
    occ = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        if shadow and found.any():
            fi = np.nonzero(found)[0]
            lp = np.asarray(params.light_pos, np.float32)
            I = [r[fi, k] + r[fi, 3 + k] * hits["dist"][fi] for k in range(3)]
            L = [lp[k] - I[k] for k in range(3)]
            dist = np.sqrt(L[0] * L[0] + L[1] * L[1] + L[2] * L[2])
            inv = f32(1.0) / dist
            L = [L[k] * inv for k in range(3)]
            sr = np.stack([I[0] + L[0] * f32(0.001), I[1] + L[1] * f32(0.001), I[2] + L[2] * f32(0.001), L[0], L[1], L[2]], 1).astype(np.float32)
            sh = _trace(scene, sr, tmax=dist.astype(np.float32), any_hit=True)
            counter[0] += len(fi)
            occ[fi] = sh["dist"] != LARGE
        col = np.zeros((n, 3), np.float32)
        col[~found] = np.asarray(params.background, np.float32)
        refl = np.zeros(n, np.float32)
        if found.any():
            _, _, refl_f = _normal_and_point(scene, r[found], hits[found])
            refl[found] = refl_f
        bnc = found & (refl > f32(0.0)) & (bounce + 1 < params.max_depth)
        fin = found & ~bnc
        dark = _with(params, light_color=(0.0, 0.0, 0.0))
        for sel, p in ((fin & ~occ, params), (fin & occ, dark)):
            if sel.any():
                col[sel] = _shade(scene, r[sel], hits[sel], p)
        if bnc.any():
            bi = np.nonzero(bnc)[0]
            term = np.zeros((len(bi), 3), np.float32)
            for sel, p in ((~occ[bi], _with(params, background=(0.0, 0.0, 0.0))), (occ[bi], _with(dark, background=(0.0, 0.0, 0.0)))):
                if sel.any():
                    term[sel] = _shade(scene, r[bi[sel]], hits[bi[sel]], p)
            I, N, rf = _normal_and_point(scene, r[bi], hits[bi])
            d = [r[bi, 3 + k] for k in range(3)]
            dn = N[0] * d[0] + N[1] * d[1] + N[2] * d[2]
            v = [d[k] - (f32(2.0) * N[k]) * dn for k in range(3)]
            inv = f32(1.0) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            R = [v[k] * inv for k in range(3)]
            sec = np.stack([I[0] + R[0] * f32(0.001), I[1] + R[1] * f32(0.001), I[2] + R[2] * f32(0.001), R[0], R[1], R[2]], 1).astype(np.float32)
            sc, _ = _radiance(scene, sec, params, shadow, bounce + 1, counter)
            col[bi] = term + sc * rf[:, None]
    hits = hits.copy()
    hits["blasIdx"] |= np.where(occ, np.uint32(0x80000000), np.uint32(0))
    return col, hits


def pack_rgb8(col):
    """common.h:149-154: (int)(min(c, 1) * 255) per channel"""
    with np.errstate(all="ignore"):
        q = (np.minimum(col, f32(1.0)) * f32(255)).astype(np.float32)
        i = np.trunc(q).astype(np.int64)
    return (((i[:, 0] << 16) + (i[:, 1] << 8) + i[:, 2]) & 0xFFFFFFFF).astype(np.uint32)


def frame_from_rays(scene, r, params=None, shadow=0):
    """pixels (n,) u32, hit records (n,) (bit 31 of blasIdx: the occlusion ray was blocked), colours (n, 3), rays traced"""
    params = params or po.shade_params()
    counter = [0]
    col, hits = _radiance(scene, np.ascontiguousarray(r, np.float32), params, shadow, 0, counter)
    return pack_rgb8(col), hits, col, counter[0]


def frame(scene, cam14, w, h, params=None, shadow=0, y0=0, y1=None):
    """the camera frame of rows [y0, y1): pixels (rows, w), hits (rows, w), colours (rows, w, 3), rays traced"""
    y1 = h if y1 is None else y1
    px, hits, col, n = frame_from_rays(scene, rays(cam14, w, h, y0, y1), params, shadow)
    return px.reshape(y1 - y0, w), hits.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), n


def hostile_cameras(w, h):
    """the cameras the issue's GPU checks list, as cam14 arrays (name -> cam14)"""
    c = {}
    c["axis_aligned"] = [0, 100, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0]   # exact zero components at the centre row / column
    c["far_cancel"] = [2.0 ** 40, 2.0 ** 40, -2.0 ** 40, -1, 0, 0, 0, 0, 1, 0, 1, 0, 1e-3, 1e-3]   # pt_w - pos cancels to 0
    c["subnormal_basis"] = [0, 100, 0, 1, 1e-40, -1e-41, 1e-39, 0, 1, 0, 1, 3e-40, 2.0, 1.5]
    c["neg_zero_pos"] = [-0.0, 100, -0.0, 1, 0.01, 0.02, 0.03, 0, 1, 0, 1, 0, 2.0, 1.5]
    c["beyond_2_60"] = [2.0 ** 61, 100, 0, -1, 0.1, 0.05, 0.05, 0, 1, 0, 1, 0.1, 2.0, 1.5]
    c["zero_viewplane"] = [0, 100, 0, 1, 0.1, 0.2, 0, 0, 1, 0, 1, 0, 0.0, 0.0]
    c["non_orthonormal"] = [5, 95, -3, 2.0, -0.3, 0.1, 0.5, 0.7, 1.5, 0.2, 3.0, -0.4, 2.5, 1.7]
    return {k: np.array(v, np.float32) for k, v in c.items()}
