"""numpy / ctypes restatement of the ambient-occlusion and diffuse-bounce frames over an arbitrary set of primary rays
(vxrt_render_ao_camera / vxrt_render_diffuse_bounce_camera).  TEST INFRASTRUCTURE ONLY.

oracle/rt_oracle.c:orc_render_ao / orc_render_gi with the primary ray handed in instead of orc_generate_ray, composed only of pieces
that are pinned elsewhere:
  closest hit                      pyoracle.trace_mt(pyoracle.trace_canonical, ...)
  Lambert colour (orc_shade)       pyoracle.shade
  hit point I, shading normal N    camera_ref._normal_and_point (shade_terms' I and N)
  secondary ray                    orc_ao_ray through pyoracle.orc(), one call per ray: seed WangHash((x + y * W) * spp + s + 1 +
                                   user_seed * 0x9E3779B9), view_dir = the primary ray's direction
  occlusion                        trace_canonical(any_hit=True, tmax=radius)
  albedo = texColor                closest.cpp:72-77, restated as tests/shading_ref.py does it
  RGB8 pack                        camera_ref.pack_rgb8
tests/test_camera_secondary_cpu.py holds both functions bit-equal to pyoracle.render_ao / render_gi on the fixed camera's rays."""
import ctypes as C
import math

import numpy as np

import camera_ref as cr
import shading_ref as sr
from camera_ref import po

f32 = np.float32
LARGE = cr.LARGE


def primary(scene, rays, params):
    """what both frames share, computed once per set of rays: closest hits, Lambert colours, and I / N of the rays that hit"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    hits = cr._trace(scene, rays)
    col = cr._shade(scene, rays, hits, params).astype(np.float32)
    fi = np.nonzero(hits["dist"] != LARGE)[0]
    I = N = np.zeros((0, 3), np.float32)
    if len(fi):
        with np.errstate(all="ignore"):
            Il, Nl, _ = cr._normal_and_point(scene, rays[fi], hits[fi])
        I, N = np.ascontiguousarray(np.stack(Il, 1), np.float32), np.ascontiguousarray(np.stack(Nl, 1), np.float32)
    return {"rays": rays, "hits": hits, "col": col, "fi": fi, "I": I, "N": N}


def secondary_rays(prim, xs, ys, w, spp, seed):
    """(len(fi) * spp, 6): orc_ao_ray for every sample of every pixel with a hit, the samples of a pixel next to each other"""
    L = po.orc()
    u32 = C.c_uint32
    L.orc_ao_ray.restype = None
    L.orc_ao_ray.argtypes = [u32] * 6 + [C.c_void_p] * 4
    fi, I, N = prim["fi"], prim["I"], prim["N"]
    d = np.ascontiguousarray(prim["rays"][fi, 3:6], np.float32)
    out = np.zeros((len(fi) * spp, 6), np.float32)
    pI, pN, pd, po_ = I.ctypes.data, N.ctypes.data, d.ctypes.data, out.ctypes.data
    px, py = [int(v) for v in np.asarray(xs)[fi]], [int(v) for v in np.asarray(ys)[fi]]
    fn = L.orc_ao_ray
    for k in range(len(fi)):
        for s in range(spp):
            fn(px[k], py[k], w, spp, s, seed & 0xFFFFFFFF, pI + 12 * k, pN + 12 * k, pd + 12 * k, po_ + 24 * (k * spp + s))
    return out


def albedo(scene, hits):
    """texColor of closest.cpp:72-77 for hit records that hit: texSample + RGB8toRGB32F for a textured material, else its diffuse colour"""
    ti = hits["triIdx"]
    bx, by, bz = hits["bx"], hits["by"], hits["bz"]
    ex = [sr._col(scene["triEx"], 64, 4 * k, ti, np.float32) for k in range(9, 15)]     # uv0, uv1, uv2
    tex_id = sr._col(scene["triEx"], 64, 60, ti, np.uint32)
    mat = np.frombuffer(np.ascontiguousarray(scene["mat"], np.uint8).tobytes(), sr.MAT_DT)[tex_id]
    tex = np.frombuffer(np.ascontiguousarray(scene["tex"], np.uint8).tobytes(), np.uint8)
    with np.errstate(all="ignore"):
        uv = []
        for k in range(2):
            a = ex[2 + k] * bx
            b = ex[4 + k] * by
            c = ex[k] * bz
            s = a + b
            uv.append(s + c)
        textured = mat["tex_id"] >= 0
        tw = np.where(textured, mat["tw"], 1).astype(np.uint32)
        th = np.where(textured, mat["th"], 1).astype(np.uint32)
        iu = sr.f2u_x86(uv[0] * tw.astype(np.float32)) % tw
        iv = sr.f2u_x86(uv[1] * th.astype(np.float32)) % th
        texel_index = iu.astype(np.int64) + iv.astype(np.int64) * tw.astype(np.int64)
        byte = np.where(textured, mat["off"].astype(np.int64) + 4 * texel_index, 0)
        texel = tex[byte[:, None] + np.arange(4)].copy().view(np.uint32)[:, 0] if len(tex) >= 4 else np.zeros(len(ti), np.uint32)
        scale = f32(1.0) / f32(256.0)
        tc = []
        for k, shift in enumerate((16, 8, 0)):
            ch = ((texel >> np.uint32(shift)) & np.uint32(255)).astype(np.int32).astype(np.float32) * scale
            tc.append(np.where(textured, ch, mat["f"][:, 3 + k]).astype(np.float32))
    return np.stack(tc, 1)


def ao_frame_from_rays(scene, rays, xs, ys, w, params, spp, radius, seed, prim=None):
    """orc_render_ao over `rays` (ray i belongs to pixel (xs[i], ys[i]) of a frame `w` wide): pixels (n,) u32, colours (n, 3),
    unoccluded counts (n,) u32, rays traced"""
    prim = prim or primary(scene, rays, params)
    n, fi = len(prim["rays"]), prim["fi"]
    col = prim["col"].copy()
    opn = np.zeros(n, np.uint32)
    if len(fi):
        sec = secondary_rays(prim, xs, ys, w, spp, seed)
        oh = cr._trace(scene, sec, tmax=np.full(len(sec), radius, np.float32), any_hit=True)
        opn[fi] = (oh["dist"] == LARGE).reshape(len(fi), spp).sum(1).astype(np.uint32)
        with np.errstate(all="ignore"):
            f = opn[fi].astype(np.float32) / f32(spp)
            col[fi] = col[fi] * f[:, None]
    return cr.pack_rgb8(col), col, opn, n + len(fi) * spp


def gi_frame_from_rays(scene, rays, xs, ys, w, params, seed, prim=None, info=None):
    """orc_render_gi over `rays`: pixels (n,) u32, colours (n, 3), rays traced.  info (optional dict): gets `bounce_found`, per pixel
    with a primary hit whether its bounce ray hit something"""
    prim = prim or primary(scene, rays, params)
    n, fi = len(prim["rays"]), prim["fi"]
    col = prim["col"].copy()
    if len(fi):
        sec = secondary_rays(prim, xs, ys, w, 1, seed)
        bh = cr._trace(scene, sec)
        c1 = cr._shade(scene, sec, bh, params)
        alb = albedo(scene, prim["hits"][fi])
        with np.errstate(all="ignore"):
            col[fi] = col[fi] + alb * c1
        if info is not None:
            info["bounce_found"] = bh["dist"] != LARGE
    elif info is not None:
        info["bounce_found"] = np.zeros(0, bool)
    return cr.pack_rgb8(col), col, n + len(fi)


def pixel_grid(w, y0, y1):
    """(xs, ys) of the rays camera_ref.rays / pyoracle.camera_rays return for rows [y0, y1)"""
    return np.tile(np.arange(w, dtype=np.uint32), y1 - y0), np.repeat(np.arange(y0, y1, dtype=np.uint32), w)


def ao_frame(scene, cam14, w, h, params, spp, radius, seed=0, y0=0, y1=None, prim=None):
    """the camera's ambient-occlusion frame of rows [y0, y1): pixels (rows, w), colours (rows, w, 3), unoccluded (rows, w), rays traced"""
    y1 = h if y1 is None else y1
    xs, ys = pixel_grid(w, y0, y1)
    px, col, opn, n = ao_frame_from_rays(scene, cr.rays(cam14, w, h, y0, y1) if prim is None else prim["rays"], xs, ys, w, params, spp, radius, seed, prim)
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), opn.reshape(y1 - y0, w), n


def gi_frame(scene, cam14, w, h, params, seed=0, y0=0, y1=None, prim=None, info=None):
    """the camera's diffuse-bounce frame of rows [y0, y1): pixels (rows, w), colours (rows, w, 3), rays traced"""
    y1 = h if y1 is None else y1
    xs, ys = pixel_grid(w, y0, y1)
    px, col, n = gi_frame_from_rays(scene, cr.rays(cam14, w, h, y0, y1) if prim is None else prim["rays"], xs, ys, w, params, seed, prim, info)
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), n


def in_fast_domain(rays):
    """the fast traversal's domain test on world-space rays (DESIGN s2): every component of 1/d finite, non-zero and at most 2^64,
    every origin component at most 2^60.  A primary ray outside it is deferred to the EXACT launch."""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        inv = f32(1.0) / r[:, 3:6]
        ok = (np.abs(inv) <= f32(2.0 ** 64)).all(1) & (inv != 0).all(1) & (np.abs(r[:, 0:3]) <= f32(2.0 ** 60)).all(1)
    return ok


# ---- the cases tests/test_gpu_camera_secondary.py runs and tests/test_camera_secondary_cpu.py shows to be non-vacuous ----
W, H = 96, 64
KEYS = ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")
GOLDEN_CENTRE, GOLDEN_ORBIT = (0.0, 0.0, 0.0), 6.0    # (the golden scenes: three instances within 2.8 units of the origin)


def framing(w, h):
    return np.array([0, 100, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0], np.float32)


def orbit(vrt, k, n=8, w=W, h=H, centre=(180.0, 90.0, 0.0), radius=260.0, height=140.0):
    a = 2.0 * math.pi * k / n
    eye = (centre[0] + radius * math.cos(a), height, centre[2] + radius * math.sin(a))
    return np.array(vrt.rtapi.look_at(eye, centre, (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32)


HALL_CAMERA_NAMES = ["framing", "inside_blob"] + ["orbit_%d" % k for k in range(8)] + sorted(cr.hostile_cameras(W, H))


def hall_cameras(vrt, w=W, h=H):
    """the cameras of tests/test_gpu_camera.py on scenes.mirror_hall: framing, inside_blob, orbit_0..7 and the hostile ones"""
    c = {"framing": framing(w, h), "inside_blob": np.array([180, 90, 30, 0.3, -0.2, 1, 1, 0, 0, 0, 1, 0, 2.0, 1.4], np.float32)}
    for k in range(8):
        c["orbit_%d" % k] = orbit(vrt, k, 8, w, h)
    c.update(cr.hostile_cameras(w, h))
    return c


def golden_cameras(vrt, w=W, h=H):
    """two cameras that orbit the golden scenes (teapot_x3, tex_mix: a few units across, in front of the fixed camera)"""
    return {"g_orbit_1": orbit(vrt, 1, 8, w, h, GOLDEN_CENTRE, GOLDEN_ORBIT, GOLDEN_CENTRE[1] + 0.4 * GOLDEN_ORBIT),
            "g_orbit_5": orbit(vrt, 5, 8, w, h, GOLDEN_CENTRE, GOLDEN_ORBIT, GOLDEN_CENTRE[1] + 0.4 * GOLDEN_ORBIT)}


def chain_camera(vrt, w=W, h=H):
    """looks down scenes.chain_bvh4's stack of triangles (x = 320 .. 420, facing -x) from the side of the fixed camera"""
    return np.array(vrt.rtapi.look_at((100.0, 100.0, 200.0), (400.0, 100.0, 0.0), (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32)


# Radii of the occlusion rays, chosen on the CPU (tests/test_camera_secondary_cpu.py) so that every frame has partly occluded pixels
# as well as fully open ones.  They are inputs, not tolerances.  orbit_0 and orbit_4 stand behind a mirror and see its flat back: the
# nearest other surface is the floor, a few hundred units away.  inside_blob sits in a closed surface 40 units across.
RADIUS = {"mirror_hall": 40.0, "tex_mix": 0.5, "teapot_x3": 0.5, "chain20": 20.0}
HALL_RADIUS = {"orbit_0": 300.0, "orbit_4": 300.0, "inside_blob": 20.0}


def hall_radius(camera_name):
    return HALL_RADIUS.get(camera_name, RADIUS["mirror_hall"])
