"""numpy / ctypes restatement of the path-traced frame (vxrt_render_path) "from rays".  TEST INFRASTRUCTURE ONLY.

The definition in include/vortex_hip.h, composed only of pieces that are pinned elsewhere:
  closest hit, occlusion ray        camera_ref._trace (pyoracle.trace_canonical)
  Lit (orc_shade, both forms)       camera_ref._shade with the parameters of camera_ref._with: light_color = 0 is the occluded colour
  hit point I, shading normal N     camera_ref._normal_and_point
  Alb = texColor                    camera_secondary_ref.albedo
  bounce ray                        orc_ao_ray through pyoracle.orc(), one call per ray, user seed = (seed + depth) mod 2^32
  RGB8 pack                         camera_ref.pack_rgb8
All paths of a frame are carried side by side (path = pixel with a primary hit x sample); every + and * is one numpy float32 operation.
tests/test_path_cpu.py holds the two identities of the definition and shows that the GPU cases are not vacuous."""
import ctypes as C

import numpy as np

import camera_ref as cr
import camera_secondary_ref as csr
from camera_ref import po

f32 = np.float32
LARGE = cr.LARGE


def _params(params):
    """the shade parameters with max_depth = 1 (the path frame ignores it)"""
    return po.shade_params(tuple(params.ambient), tuple(params.light_color), tuple(params.light_pos), tuple(params.background), 1)


def primary(scene, rays):
    """what every frame from the same rays shares: the closest hits of the primary rays"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    return {"rays": rays, "hits": cr._trace(scene, rays)}


def lit(scene, r, hits, params, shadow):
    """Lit of rays r that hit (hits): colours, number of blocked occlusion rays, occlusion rays traced"""
    n = len(r)
    if n == 0:
        return np.zeros((0, 3), np.float32), 0, 0
    occ = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        if shadow:   # camera_ref._radiance's restatement of occluded_toward_light
            lp = np.asarray(params.light_pos, np.float32)
            I = [r[:, k] + r[:, 3 + k] * hits["dist"] for k in range(3)]
            L = [lp[k] - I[k] for k in range(3)]
            dist = np.sqrt(L[0] * L[0] + L[1] * L[1] + L[2] * L[2])
            inv = f32(1.0) / dist
            L = [L[k] * inv for k in range(3)]
            sr = np.stack([I[0] + L[0] * f32(0.001), I[1] + L[1] * f32(0.001), I[2] + L[2] * f32(0.001), L[0], L[1], L[2]], 1).astype(np.float32)
            occ = cr._trace(scene, sr, tmax=dist.astype(np.float32), any_hit=True)["dist"] != LARGE
        col = np.zeros((n, 3), np.float32)
        for sel, p in ((~occ, params), (occ, cr._with(params, light_color=(0.0, 0.0, 0.0)))):
            if sel.any():
                col[sel] = cr._shade(scene, r[sel], hits[sel], p)
    return col, int(occ.sum()), n if shadow else 0


def bounce_rays(xs, ys, w, spp, smp, seed, I, N, d):
    """orc_ao_ray per path: pixel (xs[i], ys[i]), sample smp[i], leaving I[i] about N[i] turned against d[i]"""
    L = po.orc()
    u32 = C.c_uint32
    L.orc_ao_ray.restype = None
    L.orc_ao_ray.argtypes = [u32] * 6 + [C.c_void_p] * 4
    I, N, d = (np.ascontiguousarray(v, np.float32) for v in (I, N, d))
    out = np.zeros((len(I), 6), np.float32)
    pI, pN, pd, po_ = I.ctypes.data, N.ctypes.data, d.ctypes.data, out.ctypes.data
    px, py, ps = [int(v) for v in xs], [int(v) for v in ys], [int(v) for v in smp]
    fn = L.orc_ao_ray
    for i in range(len(I)):
        fn(px[i], py[i], w, spp, ps[i], seed & 0xFFFFFFFF, pI + 12 * i, pN + 12 * i, pd + 12 * i, po_ + 24 * i)
    return out


def frame_from_rays(scene, rays, xs, ys, w, params, spp, bounces, seed=0, shadow=0, prim=None):
    """the path frame over `rays` (ray i belongs to pixel (xs[i], ys[i]) of a frame `w` wide): pixels (n,) u32, colours (n, 3), rays
    traced, and per depth 0 .. bounces-1 the tuple (live paths, bounce rays that hit, blocked occlusion rays)"""
    params = _params(params)
    prim = prim or primary(scene, rays)
    rays, hits0 = prim["rays"], prim["hits"]
    n = len(rays)
    bg = np.asarray(params.background, np.float32)
    col = np.tile(bg, (n, 1)).astype(np.float32)
    fi = np.nonzero(hits0["dist"] != LARGE)[0]
    traced, depths = n, []
    if len(fi) == 0:
        return cr.pack_rgb8(col), col, traced, [(0, 0, 0)] * bounces
    lit0, _, nocc = lit(scene, rays[fi], hits0[fi], params, shadow)
    traced += nocc
    alb0 = csr.albedo(scene, hits0[fi])
    m = len(fi)
    with np.errstate(all="ignore"):
        # path j * spp + s = sample s of pixel fi[j]
        Lc = np.repeat(lit0, spp, 0).astype(np.float32)
        thr = np.repeat(alb0, spp, 0).astype(np.float32)
        pxs, pys = np.repeat(np.asarray(xs)[fi], spp), np.repeat(np.asarray(ys)[fi], spp)
        smp = np.tile(np.arange(spp, dtype=np.uint32), m)
        alive = np.arange(m * spp)
        r, h = np.repeat(rays[fi], spp, 0), np.repeat(hits0[fi], spp, 0)
        for k in range(bounces):
            if len(alive) == 0:
                depths.append((0, 0, 0))
                continue
            I, N, _ = cr._normal_and_point(scene, r, h)
            sec = bounce_rays(pxs[alive], pys[alive], w, spp, smp[alive], seed + k, np.stack(I, 1), np.stack(N, 1), r[:, 3:6])
            bh = cr._trace(scene, sec)
            traced += len(alive)
            hit = bh["dist"] != LARGE
            miss_i, hit_i = alive[~hit], alive[hit]
            Lc[miss_i] = Lc[miss_i] + thr[miss_i] * bg
            lk, blocked, nocc = lit(scene, sec[hit], bh[hit], params, shadow)
            traced += nocc
            Lc[hit_i] = Lc[hit_i] + thr[hit_i] * lk
            if hit.any():
                thr[hit_i] = thr[hit_i] * csr.albedo(scene, bh[hit])
            depths.append((len(alive), int(hit.sum()), blocked))
            r, h, alive = sec[hit], bh[hit], hit_i
        Lc = Lc.reshape(m, spp, 3)
        acc = Lc[:, 0].copy()
        for s in range(1, spp):
            acc = acc + Lc[:, s]
        col[fi] = acc / f32(spp)
    return cr.pack_rgb8(col), col, traced, depths


def frame(scene, cam14, w, h, params, spp, bounces, seed=0, shadow=0, y0=0, y1=None, prim=None):
    """the path frame of rows [y0, y1) seen from cam14 (None: the fixed camera): pixels (rows, w), colours (rows, w, 3), rays traced,
    per-depth counts"""
    y1 = h if y1 is None else y1
    xs, ys = csr.pixel_grid(w, y0, y1)
    if prim is None:
        prim = primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))
    px, col, n, depths = frame_from_rays(scene, prim["rays"], xs, ys, w, params, spp, bounces, seed, shadow, prim)
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), n, depths


# ---- the cases tests/test_gpu_path.py runs and tests/test_path_cpu.py shows to be non-vacuous ----
W, H = csr.W, csr.H
CONFIGS = ((2, 3, 1, 3), (5, 2, 0, 0))   # (spp, bounces, shadow, seed)
