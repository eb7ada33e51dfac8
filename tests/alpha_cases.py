"""The cases of the alpha test (vxrt_accel_set_alpha_test): scenes with cutout textures, their thresholds, cameras and ray buffers.
TEST INFRASTRUCTURE ONLY.  tests/test_alpha_cpu.py pins the restatement on them and shows that they are not vacuous;
tests/test_gpu_alpha.py compares the kernels with the restatement on them, bit for bit.

Every case is a dict: scene (buffers), thresholds (one byte per material), cams (name -> cam14, None = the RTU test's fixed camera),
params (oracle shade parameters), and is built once per process (case())."""
import functools
import os

import numpy as np

import alpha_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import scenes
import shading_cases
import shading_ref as sr
from camera_ref import po

f32 = np.float32
KEYS = csr.KEYS
W, H = csr.W, csr.H
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAME_CASES = ("tex_mix", "chain20", "mirror_hall")
N_RANDOM = 2048


def _checker(w, h, block):
    """top bytes of a w x h texture: a block checkerboard of 255 / 0"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x // block) + (y // block)) % 2 == 0, 255, 0).astype(np.uint32)


def _set_top_bytes(tex, off, alpha):
    t = tex[off:off + 4 * alpha.size].view(np.uint32)
    t[:] = (t & np.uint32(0x00FFFFFF)) | (alpha.reshape(-1).astype(np.uint32) << np.uint32(24))


def tri_instances(b):
    """instance index of every triangle (the leaves under each instance's BLAS root; a triangle no instance reaches: -1)"""
    bvh = np.ascontiguousarray(b["bvh"], np.uint8).view(ar.NODE)
    blas = np.ascontiguousarray(b["blas"], np.uint8).view(np.uint32).reshape(-1, 40)
    out = np.full(b["tri"].size // 36, -1, np.int64)
    for j in range(len(blas)):
        base = int(blas[j, 0])
        todo = [0]
        while todo:
            n = bvh[base + todo.pop()]
            if n["ld"] != 0:
                out[int(n["lf"]):int(n["lf"]) + int(n["ld"])] = j
            else:
                todo += [int(n["lf"]) + k for k in range(4) if n["ch"][k, 0] != 0]
    return out


def has_multi_triangle_leaves(b):
    return bool((np.ascontiguousarray(b["bvh"], np.uint8).view(ar.NODE)["ld"] > 1).any())


def _tex_mix(vrt):
    with np.load(os.path.join(GOLDEN, "tex_mix.npz")) as z:
        b = {k: z[k].copy() for k in KEYS}
        z_rays = z["rays"].astype(np.float32).copy()
    mat = b["mat"].view(sr.MAT_DT)
    thr = np.zeros(len(mat), np.uint8)
    for m, t in zip(np.nonzero(mat["tex_id"] >= 0)[0], (128, 1)):
        w, h = int(mat["tw"][m]), int(mat["th"][m])
        _set_top_bytes(b["tex"], int(mat["off"][m]), _checker(w, h, max(1, w // 24)))
        thr[m] = t
    cams = dict(csr.golden_cameras(vrt, W, H))
    cams["fixed"] = None
    # (the fixture's own rays: the fixed camera's, at the size the fixture was recorded with -- they go into the ray buffer)
    return {"scene": b, "thresholds": thr, "cams": cams, "params": po.shade_params(), "extra_rays": z_rays}


def _one_texture(b, w, h, alpha, rgb=0x808080):
    """append one textured material (w x h texels, top bytes `alpha`) to the scene's materials; returns its index"""
    mat = np.frombuffer(b["mat"].tobytes(), sr.MAT_DT).copy()
    tex = b["tex"].copy() if b["tex"].size >= 4 and (mat["tex_id"] >= 0).any() else np.zeros(0, np.uint8)
    new = np.zeros(1, sr.MAT_DT)
    new["f"][0, 3:6] = 0.8
    new["tex_id"], new["tw"], new["th"], new["off"] = int((mat["tex_id"] >= 0).sum()), w, h, tex.size
    texels = (np.uint32(rgb) + (np.arange(w * h, dtype=np.uint32) * np.uint32(0x010203) & np.uint32(0x3F3F3F))) | (alpha.reshape(-1).astype(np.uint32) << np.uint32(24))
    b["mat"] = np.concatenate([mat, new]).view(np.uint8).reshape(-1).copy()
    b["tex"] = np.concatenate([tex, texels.view(np.uint8)]).copy()
    return len(mat)


def _chain20(vrt):
    sc = scenes.chain_bvh4(vrt, 20)
    b = {k: np.frombuffer(bytes(sc.buffers[k]), np.uint8).copy() for k in KEYS}
    n = b["tri"].size // 36
    # one texel per stacked triangle (constant uv over the triangle); roughly every third layer is solid
    alpha = np.where(np.arange(n) % 3 == 2, 255, 0).astype(np.uint32)
    m = _one_texture(b, n, 1, alpha)
    ex = b["triEx"].view(np.float32).reshape(-1, 16)
    for k in (9, 11, 13):
        ex[:, k] = ((np.arange(n) + 0.5) / n).astype(np.float32)
        ex[:, k + 1] = 0.5
    b["triEx"].view(np.uint32).reshape(-1, 16)[:, 15] = m
    thr = np.zeros(m + 1, np.uint8)
    thr[m] = 128
    # a light in front of the stack, off its axis: the floor of holes lets it through to the solid layers behind
    return {"scene": b, "thresholds": thr, "cams": {"chain": csr.chain_camera(vrt, W, H), "fixed": None},
            "params": po.shade_params(light_pos=(150.0, 160.0, 40.0))}


def _mirror_hall(vrt):
    b = scenes.mirror_hall(vrt)
    b = {k: b[k].copy() for k in KEYS}
    inst = tri_instances(b)
    tri = b["tri"].view(np.float32).reshape(-1, 3, 3)
    ex = b["triEx"].view(np.float32).reshape(-1, 16)
    tid = b["triEx"].view(np.uint32).reshape(-1, 16)
    m_blob = _one_texture(b, 23, 17, _checker(23, 17, 2), 0x905030)
    m_mirror = _one_texture(b, 16, 16, _checker(16, 16, 2), 0x305090)
    rng = np.random.default_rng(4711)
    blob = np.nonzero(inst == 3)[0]
    ex[blob, 9:15] = rng.uniform(-1.5, 2.5, (len(blob), 6)).astype(np.float32)     # (uv outside [0, 1] too)
    tid[blob, 15] = m_blob
    for t in np.nonzero(inst == 1)[0]:       # the mirror facing the camera: uv from the quad's z and y
        for c, k in enumerate((9, 11, 13)):
            ex[t, k] = (tri[t, c, 2] + 200.0) / 400.0
            ex[t, k + 1] = (tri[t, c, 1] - 10.0) / 220.0
        tid[t, 15] = m_mirror
    thr = np.zeros(m_mirror + 1, np.uint8)
    thr[m_blob], thr[m_mirror] = 128, 255
    cams = {"fixed": None, "orbit_1": csr.orbit(vrt, 1, 8, W, H), "inside_blob": csr.hall_cameras(vrt, W, H)["inside_blob"]}
    return {"scene": b, "thresholds": thr, "cams": cams, "params": po.shade_params(max_depth=3)}


@functools.lru_cache(maxsize=None)
def _case(name):
    import importlib
    vrt = importlib.import_module("vortex-raytracing_amd")
    return {"tex_mix": _tex_mix, "chain20": _chain20, "mirror_hall": _mirror_hall}[name](vrt)


def case(name):
    return _case(name)


def cam_rays(cam, w=W, h=H, y0=0, y1=None):
    return po.camera_rays(w, h, y0, h if y1 is None else y1) if cam is None else cr.rays(cam, w, h, y0, y1)


@functools.lru_cache(maxsize=None)
def ray_buffer(name):
    """(rays, tmax) for vxrt_trace on a frame case: the rays of its first camera, N_RANDOM random rays aimed at the scene,
    axis-parallel rays (a zero direction component: the EXACT launch) and a per-ray tmax (some above 1e30, some that cut the hit off)"""
    c = case(name)
    b = c["scene"]
    rng = np.random.default_rng(900 + FRAME_CASES.index(name))
    frame = cam_rays(next(iter(c["cams"].values())))
    hits = cr._trace(b, frame)
    fi = np.nonzero(hits["dist"] != cr.LARGE)[0]
    assert len(fi) > 20
    pts = frame[fi, 0:3] + frame[fi, 3:6] * hits["dist"][fi, None]
    lo, hi = pts.min(0), pts.max(0)
    tgt = rng.uniform(lo, hi, (N_RANDOM, 3))
    org = tgt + rng.normal(size=(N_RANDOM, 3)) * (np.linalg.norm(hi - lo) + 1.0)
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rnd = np.concatenate([org, d], 1).astype(np.float32)
    # axis-parallel: through hit points, along each axis (the other two direction components are zero)
    k = rng.choice(len(pts), 96)
    axis = np.zeros((96, 6), np.float32)
    for i, j in enumerate(k):
        a = i % 3
        sign = 1.0 if (i // 3) % 2 else -1.0
        axis[i, 0:3] = pts[j]
        axis[i, a] -= sign * 500.0
        axis[i, 3 + a] = sign
    rays = np.ascontiguousarray(np.concatenate([frame, rnd, axis] + ([c["extra_rays"]] if "extra_rays" in c else [])), np.float32)
    opaque = cr._trace(b, rays)
    dist = np.where(opaque["dist"] != cr.LARGE, opaque["dist"], f32(100.0))
    tmax = (dist * rng.choice([0.5, 0.999, 1.0, 1.5, 4.0, 1e35], len(rays))).astype(np.float32)
    return rays, tmax


@functools.lru_cache(maxsize=None)
def hostile(seed, family):
    """a shading_cases scene (random textures of odd sizes; negative / huge / NaN uv) with random top bytes and thresholds 1, 128, 255
    dealt over its textured materials; the rays of its ragged frame"""
    import importlib
    vrt = importlib.import_module("vortex-raytracing_amd")
    b, _, _ = shading_cases.case(vrt, po, seed, family)
    b = {k: np.ascontiguousarray(b[k], np.uint8).copy() for k in KEYS}
    rng = np.random.default_rng(7700 + seed)
    mat = b["mat"].view(sr.MAT_DT)
    thr = np.zeros(len(mat), np.uint8)
    for i, m in enumerate(np.nonzero(mat["tex_id"] >= 0)[0]):
        n = int(mat["tw"][m]) * int(mat["th"][m])
        _set_top_bytes(b["tex"], int(mat["off"][m]), rng.integers(0, 256, n).astype(np.uint32))
        thr[m] = (1, 128, 255)[(i + seed) % 3]
    return {"scene": b, "thresholds": thr, "rays": po.camera_rays(*shading_cases.FRAME_SIZES[1])}


HOSTILE = ((2, "hostile"), (3, "hostile"), (4, "outside_c"))     # (the seeds with two or three textured materials)


# ---- reference results, computed once per process and shared ----
@functools.lru_cache(maxsize=None)
def tracer(name, alpha=True):
    c = case(name)
    return ar.tracer(c["scene"], c["thresholds"] if alpha else None)


@functools.lru_cache(maxsize=None)
def ref_frame(name, cam_name, shadow, alpha=True):
    """(pixels, hits, colours, rays traced, lit_by_hole) of the case's frame from camera cam_name"""
    c = case(name)
    rays = cam_rays(c["cams"][cam_name])
    lit = np.zeros(len(rays), bool) if (shadow and alpha) else None
    px, hits, col, n = ar.frame_from_rays(c["scene"], tracer(name, alpha), rays, c["params"], shadow, lit)
    return px, hits, col, n, lit


@functools.lru_cache(maxsize=None)
def ref_trace(name, any_hit, with_tmax, alpha=True, with_info=False):
    rays, tmax = ray_buffer(name)
    info = np.zeros(len(rays), ar.INFO_DT) if with_info else None
    hits = tracer(name, alpha)(rays, tmax if with_tmax else None, any_hit, info)
    return hits, info
