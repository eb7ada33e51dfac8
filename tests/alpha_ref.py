"""Restatement of the alpha-tested traversal (vxrt_accel_set_alpha_test) and of the frames traced through it.  TEST INFRASTRUCTURE ONLY.

trace(): a per-ray Python loop with the control flow of oracle/rt_oracle.c:orc_trace_canonical -- the stack of (node, m) entries, the
`m < hit.dist` filter on popped entries, children sorted far to near by a stable insertion sort, triangles of a leaf in index order
with a strict '<', the abandon after an accept, any-hit stop -- whose ARITHMETIC is the exported, already pinned pieces of
librt_oracle.so called through ctypes: orc_child_box, orc_ray_box, orc_ray_transform, orc_ray_tri.  The one addition is the accept
predicate: a candidate (a triangle test that returned d < hit.dist) for which it returns False is treated as if the test had returned
1e30.  With no predicate the loop is orc_trace_canonical (tests/test_alpha_cpu.py holds it bit-equal).

alpha_predicate(): the rule of include/vortex_hip.h -- material m = triEx[t].texId, threshold T[m] > 0, and the top byte of the texel the
closest-hit shader would sample (uv from the candidate's barycentrics without contraction, shading_ref.f2u_x86, exactly as
camera_secondary_ref.albedo indexes it) below T[m].

frame_from_rays(): camera_ref._radiance with the tracer handed in: alpha closest hit, pyoracle.shade, the shadow ray of orc_render_ex
(occluded_toward_light) and the mirror ray (radiance_of), each traced through the alpha traversal."""
import ctypes as C

import numpy as np

import camera_ref as cr
import shading_ref as sr
from camera_ref import po

f32 = np.float32
LARGE = cr.LARGE
NODE = np.dtype([("o", "<f4", 3), ("e", "i1", 3), ("imask", "u1"), ("lf", "<u4"), ("ld", "<u4"), ("ch", "u1", (4, 7))])
assert NODE.itemsize == 52
INFO_DT = np.dtype([("rejected", "<u4"), ("rejected_before_accept", "<u4"), ("accepted", "<u4"), ("first_rejected", "?"),
                    ("same_leaf", "?"), ("other_instance", "?")])


def _lib():
    L = po.orc()
    vp, fl = C.c_void_p, C.c_float
    L.orc_ray_box.restype = fl
    L.orc_ray_box.argtypes = [vp] + [fl] * 6
    L.orc_child_box.restype = None
    L.orc_child_box.argtypes = [vp, C.c_int, vp]
    L.orc_ray_transform.restype = None
    L.orc_ray_transform.argtypes = [vp, vp, vp]
    L.orc_ray_tri.restype = fl
    L.orc_ray_tri.argtypes = [vp, vp, vp, vp, vp]
    return L


class Walker:
    """the scene's buffers parsed once, and the decoded child boxes of the nodes visited so far (orc_child_box depends on the node alone)"""

    def __init__(self, scene):
        self.L = _lib()
        self.b = {k: np.ascontiguousarray(scene[k], np.uint8).copy() for k in ("tlas", "blas", "bvh", "tri")}
        self.tlas, self.bvh = self.b["tlas"].view(NODE), self.b["bvh"].view(NODE)
        self.blas_u32 = self.b["blas"].view(np.uint32).reshape(-1, 40)
        self.p = {k: v.ctypes.data for k, v in self.b.items()}
        self.boxes = {}

    def children(self, top, idx):
        """[(k, box6)] of the present children of TLAS node idx (top) / bvh node idx (absolute index in the bvh buffer)"""
        key = (top, idx)
        got = self.boxes.get(key)
        if got is None:
            nodes, base = (self.tlas, self.p["tlas"]) if top else (self.bvh, self.p["bvh"])
            box = (C.c_float * 6)()
            got = []
            for k in range(4):
                if nodes["ch"][idx, k, 0] == 0:
                    continue
                self.L.orc_child_box(base + 52 * idx, k, box)
                got.append((k, tuple(box)))
            self.boxes[key] = got
        return got


def trace(scene, rays, tmax=None, any_hit=False, accept=None, info=None, walker=None):
    """hit records (pyoracle.HIT_DTYPE) of orc_trace_canonical's loop with the accept predicate accept(triIdx, bx, by, bz) -> bool
    (None: every candidate is accepted).  info: optional array of INFO_DT, one entry per ray, filled with what the ray met."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = len(rays)
    out = np.zeros(n, po.HIT_DTYPE)
    w = walker or Walker(scene)
    L = w.L
    ray_box, ray_tri, ray_xf = L.orc_ray_box, L.orc_ray_tri, L.orc_ray_transform
    tm = po._tmax(tmax)
    tlas, bvh, blas_u32 = w.tlas, w.bvh, w.blas_u32
    t_imask, t_ld, t_lf = tlas["imask"].tolist(), tlas["ld"].tolist(), tlas["lf"].tolist()
    b_ld, b_lf = bvh["ld"].tolist(), bvh["lf"].tolist()
    p_blas, p_tri = w.p["blas"], w.p["tri"]
    cur_ray = (C.c_float * 6)()
    p_cur = C.addressof(cur_ray)
    bx, by, bz = C.c_float(), C.c_float(), C.c_float()
    pbx, pby, pbz = C.byref(bx), C.byref(by), C.byref(bz)
    neg_inf, large = float("-inf"), float(LARGE)
    for r in range(n):
        p_ray = rays[r].ctypes.data
        hit_dist = float(tm[r]) if tm is not None else large
        rec = (0.0, 0.0, 0.0, 0, 0)
        found = False
        C.memmove(p_cur, p_ray, 24)
        blas_idx, bbase = 0, 0
        stack = []
        cur_top, cur = True, 0
        path_m = neg_inf
        have = True
        n_rej = n_rej_before = n_acc = 0
        first_rej = same_leaf = other_inst = False
        rej_inst = set()
        while have:
            descend = False
            if cur_top:
                leaf = t_ld[cur] != 0xFFFFFFFF if t_imask[cur] == 1 else t_ld[cur] != 0
            else:
                leaf = b_ld[bbase + cur] != 0
            if not leaf:
                isect = []
                pr = p_ray if cur_top else p_cur
                for k, box in w.children(cur_top, cur if cur_top else bbase + cur):
                    d = ray_box(pr, *box)
                    if d < hit_dist:
                        isect.append((d, k))
                for i in range(1, len(isect)):       # sort_far_to_near: stable insertion sort, farthest first
                    v = isect[i]
                    j = i
                    while j > 0 and v[0] > isect[j - 1][0]:
                        isect[j] = isect[j - 1]
                        j -= 1
                    isect[j] = v
                if isect:
                    lf = t_lf[cur] if cur_top else b_lf[bbase + cur]
                    for d, k in isect[:-1]:
                        stack.append((cur_top, lf + k, d if path_m < d else path_m))     # std_max(path_m, d) = (path_m < d) ? d : path_m
                    d, k = isect[-1]
                    cur = lf + k
                    path_m = d if path_m < d else path_m
                    descend = True
            elif cur_top:
                blas_idx = t_ld[cur]
                ray_xf(p_ray, p_blas + 160 * blas_idx + 4, p_cur)
                bbase = int(blas_u32[blas_idx, 0])
                cur_top, cur = False, 0
                descend = True
            else:
                node = bbase + cur
                leaf_rej = leaf_acc = False
                stop = False
                for tri_idx in range(b_lf[node], b_lf[node] + b_ld[node]):
                    d = ray_tri(p_cur, p_tri + 36 * tri_idx, pbx, pby, pbz)
                    if d < hit_dist:
                        if accept is not None and not accept(tri_idx, bx.value, by.value, bz.value):
                            n_rej += 1
                            if n_acc == 0:
                                n_rej_before += 1
                                if n_rej == 1:
                                    first_rej = True
                            leaf_rej = True
                            rej_inst.add(blas_idx)
                            continue
                        hit_dist = d
                        rec = (bx.value, by.value, bz.value, blas_idx, tri_idx)
                        found = True
                        n_acc += 1
                        leaf_acc = True
                        if any_hit:
                            stack = []
                            stop = True
                            break
                        if not (path_m < hit_dist):
                            break
                same_leaf = same_leaf or (leaf_rej and leaf_acc)
                if stop:
                    break
            if not descend:
                have = False
                while stack:
                    e_top, e_node, e_m = stack.pop()
                    if e_m < hit_dist:
                        cur_top, cur, path_m, have = e_top, e_node, e_m, True
                        break
        if found:
            out[r] = (hit_dist, rec[0], rec[1], rec[2], rec[3], rec[4])
            other_inst = any(i != rec[3] for i in rej_inst)
        else:
            out[r]["dist"] = LARGE
        if info is not None:
            info[r] = (n_rej, n_rej_before, n_acc, first_rej, same_leaf, other_inst)
    return out


def alpha_predicate(scene, thresholds):
    """accept(triIdx, bx, by, bz) for the per-material thresholds (None or all zero: None, every candidate is accepted)"""
    if thresholds is None or not any(int(t) for t in thresholds):
        return None
    thr = [int(t) for t in thresholds]
    ex = np.ascontiguousarray(scene["triEx"], np.uint8).view(np.float32).reshape(-1, 16)
    tex_id = np.ascontiguousarray(scene["triEx"], np.uint8).view(np.uint32).reshape(-1, 16)[:, 15].tolist()
    mat = np.frombuffer(np.ascontiguousarray(scene["mat"], np.uint8).tobytes(), sr.MAT_DT)
    tex = np.frombuffer(np.ascontiguousarray(scene["tex"], np.uint8).tobytes(), np.uint8)
    assert len(thr) == len(mat)

    def accept(tri_idx, bx, by, bz):
        m = tex_id[tri_idx]
        T = thr[m]
        if T == 0:
            return True
        assert mat["tex_id"][m] >= 0
        e = ex[tri_idx]
        bx, by, bz = f32(bx), f32(by), f32(bz)
        tw, th = np.uint32(mat["tw"][m]), np.uint32(mat["th"][m])
        with np.errstate(all="ignore"):
            u = (e[11] * bx + e[13] * by) + e[9] * bz          # uv1 * bx + uv2 * by + uv0 * bz
            v = (e[12] * bx + e[14] * by) + e[10] * bz
            iu = int(sr.f2u_x86(u * f32(tw))) % int(tw)
            iv = int(sr.f2u_x86(v * f32(th))) % int(th)
        byte = int(mat["off"][m]) + 4 * (iu + iv * int(tw))
        return int(tex[byte + 3]) >= T                          # top byte of the little-endian 0xAARRGGBB texel

    return accept


def tracer(scene, thresholds):
    """trace_fn(rays, tmax=None, any_hit=False) through the alpha traversal of `scene` (one Walker, one predicate)"""
    w = Walker(scene)
    accept = alpha_predicate(scene, thresholds)

    def fn(rays, tmax=None, any_hit=False, info=None):
        if len(rays) == 0:
            return np.zeros(0, po.HIT_DTYPE)
        return trace(scene, rays, tmax, any_hit, accept, info, w)

    return fn


def _radiance(scene, trace_fn, r, params, shadow, bounce, counter, lit_by_hole=None):
    """camera_ref._radiance with the tracer handed in.  lit_by_hole (level 0 only): optional bool array, set where the pixel's
    occlusion ray reached the light although the opaque traversal says it is blocked."""
    n = len(r)
    hits = trace_fn(r)
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
            srays = np.stack([I[0] + L[0] * f32(0.001), I[1] + L[1] * f32(0.001), I[2] + L[2] * f32(0.001), L[0], L[1], L[2]], 1).astype(np.float32)
            sh = trace_fn(srays, tmax=dist.astype(np.float32), any_hit=True)
            counter[0] += len(fi)
            occ[fi] = sh["dist"] != LARGE
            if lit_by_hole is not None and bounce == 0:
                opaque = cr._trace(scene, srays, tmax=dist.astype(np.float32), any_hit=True)
                lit_by_hole[fi] = (opaque["dist"] != LARGE) & ~occ[fi]
        col = np.zeros((n, 3), np.float32)
        col[~found] = np.asarray(params.background, np.float32)
        refl = np.zeros(n, np.float32)
        if found.any():
            _, _, refl_f = cr._normal_and_point(scene, r[found], hits[found])
            refl[found] = refl_f
        bnc = found & (refl > f32(0.0)) & (bounce + 1 < params.max_depth)
        fin = found & ~bnc
        dark = cr._with(params, light_color=(0.0, 0.0, 0.0))
        for sel, p in ((fin & ~occ, params), (fin & occ, dark)):
            if sel.any():
                col[sel] = cr._shade(scene, r[sel], hits[sel], p)
        if bnc.any():
            bi = np.nonzero(bnc)[0]
            term = np.zeros((len(bi), 3), np.float32)
            for sel, p in ((~occ[bi], cr._with(params, background=(0.0, 0.0, 0.0))), (occ[bi], cr._with(dark, background=(0.0, 0.0, 0.0)))):
                if sel.any():
                    term[sel] = cr._shade(scene, r[bi[sel]], hits[bi[sel]], p)
            I, N, rf = cr._normal_and_point(scene, r[bi], hits[bi])
            d = [r[bi, 3 + k] for k in range(3)]
            dn = N[0] * d[0] + N[1] * d[1] + N[2] * d[2]
            v = [d[k] - (f32(2.0) * N[k]) * dn for k in range(3)]
            inv = f32(1.0) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            R = [v[k] * inv for k in range(3)]
            sec = np.stack([I[0] + R[0] * f32(0.001), I[1] + R[1] * f32(0.001), I[2] + R[2] * f32(0.001), R[0], R[1], R[2]], 1).astype(np.float32)
            sc, _ = _radiance(scene, trace_fn, sec, params, shadow, bounce + 1, counter)
            col[bi] = term + sc * rf[:, None]
    hits = hits.copy()
    hits["blasIdx"] |= np.where(occ, np.uint32(0x80000000), np.uint32(0))
    return col, hits


def frame_from_rays(scene, trace_fn, rays, params=None, shadow=0, lit_by_hole=None):
    """pixels (n,) u32, hit records (n,) (bit 31 of blasIdx: the occlusion ray was blocked), colours (n, 3), rays traced"""
    params = params or po.shade_params()
    counter = [0]
    col, hits = _radiance(scene, trace_fn, np.ascontiguousarray(rays, np.float32).reshape(-1, 6), params, shadow, 0, counter, lit_by_hole)
    return cr.pack_rgb8(col), hits, col, counter[0]
