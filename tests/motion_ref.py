"""numpy restatement of motion-aware temporal accumulation: the previous-position guide (vxrt_previous_positions), the step with motion
(vxrt_temporal_accumulate_motion) and the path frame that uses both (vxrt_render_path_temporal_motion).  TEST INFRASTRUCTURE ONLY.

The definition is the header's "Motion", one numpy float32 operation per + - * /, in the order written there.
  guide   previous_positions(): Q4 and N'4 of hit records from a SNAPSHOT -- {"blas": the instance records as they were, "tri": the
          vertices as they were, or None for the scene's current ones} -- and the scene's current triEx
  T_m     step(): the header defines T_m as T with three substitutions, so it is computed AS temporal_ref.step on substituted guides --
          position (Q.xyz, 1 where P.w != 0 and Q.w != 0, else 0) and normal N' -- and then corrected for the two things the
          substitution does not carry: a hit pixel without a previous position takes len 1, not 0, and the history keeps the CURRENT
          frame's P and N
  frame   path_frame(): temporal_ref.path_frame with T_m, the guide taken from the primary hits
moved() is the host side of DeviceScene.set_transforms: refit_ref's records and TLAS."""
import numpy as np

import camera_ref as cr
import denoise_ref as dr
import path_ref as pr
import refit_ref as rr
import temporal_ref as tr

f32 = np.float32
BLAS_WORDS = rr.BLAS_WORDS
INSTANCES, GEOMETRY = 1, 2


def _u8(a):
    return np.frombuffer(np.ascontiguousarray(a, np.uint8).tobytes(), np.uint8)


def snapshot(scene, what=INSTANCES):
    """vxrt_accel_motion_snapshot of a host scene: copies, so that the scene may move on"""
    assert what in (INSTANCES, INSTANCES | GEOMETRY)
    return {"blas": _u8(scene["blas"]).copy(), "tri": _u8(scene["tri"]).copy() if what & GEOMETRY else None}


def moved(scene, first, mats):
    """the scene after vxrt_accel_set_transforms(first, mats): new records and the refitted TLAS (a dict; `scene` is left alone)"""
    b = {k: scene[k] for k in ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")}
    b["blas"] = rr.set_transforms(_u8(scene["blas"]), first, mats)
    b["tlas"], b["bvh"] = rr.refit(b, geometry=False)
    return b


def previous_positions(scene, snap, hits):
    """Q4 (n, 4) and N'4 (n, 4) of hit records (pyoracle.HIT_DTYPE) on `scene` as it is now, seen from snapshot `snap`"""
    n = len(hits)
    Q4 = np.zeros((n, 4), np.float32)
    N4 = np.zeros((n, 4), np.float32)
    rec = _u8(snap["blas"]).view(np.float32).reshape(-1, BLAS_WORDS)
    tri = _u8(scene["tri"] if snap["tri"] is None else snap["tri"]).view(np.float32).reshape(-1, 3, 3)
    tex = _u8(scene["triEx"]).view(np.float32).reshape(-1, 16)
    bi = hits["blasIdx"].astype(np.int64) & 0x7fffffff
    ti = hits["triIdx"].astype(np.int64)
    ok = np.nonzero((hits["dist"] != cr.LARGE) & (bi < len(rec)) & (ti < len(tri)))[0]
    if not len(ok):
        return Q4, N4
    h = hits[ok]
    bx, by, bz = h["bx"], h["by"], h["bz"]
    v, r, e = tri[ti[ok]], rec[bi[ok]], tex[ti[ok]]
    minv, m = r[:, 1:17], r[:, 17:33]
    with np.errstate(all="ignore"):
        o = [(v[:, 1, c] * bx + v[:, 2, c] * by) + v[:, 0, c] * bz for c in range(3)]
        for c in range(3):
            Q4[ok, c] = ((m[:, 4 * c] * o[0] + m[:, 4 * c + 1] * o[1]) + m[:, 4 * c + 2] * o[2]) + m[:, 4 * c + 3]
        Q4[ok, 3] = 1.0
        nn = [(e[:, 3 + c] * bx + e[:, 6 + c] * by) + e[:, c] * bz for c in range(3)]
        t = [((minv[:, c] * nn[0] + minv[:, 4 + c] * nn[1]) + minv[:, 8 + c] * nn[2]) + f32(0.0) * f32(0.0) for c in range(3)]
        inv = f32(1.0) / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        for c in range(3):
            N4[ok, c] = t[c] * inv
    return Q4, N4


def step(E, P, N, Q, Nq, hist, cam14, W, H, y0, y1, prm, stats=None):
    """out = T_m(E, P, N, Q, N'; hist, hist.cam, prm): as temporal_ref.step, with Q and Nq (rows, W, 4).  Returns out (rows, W, 4) and
    makes it, P, N, cam14 the history."""
    E, P, N, Q, Nq = (np.array(a, np.float32) for a in (E, P, N, Q, Nq))
    hit = P[..., 3] != 0
    prev = hit & (Q[..., 3] != 0)
    Ps = Q.copy()
    Ps[..., 3] = np.where(prev, f32(1.0), f32(0.0))
    out = tr.step(E, Ps, Nq, hist, cam14, W, H, y0, y1, prm, stats)
    out[..., 3] = np.where(hit & ~prev, f32(1.0), out[..., 3])      # no previous position: (E, 1)
    hist.HE, hist.HP, hist.HN = out.copy(), P.copy(), N.copy()
    return out


def path_frame(scene, snap, cam14, w, h, params, spp, bounces, seed, shadow, dn, tp, hist, y0=0, y1=None, prim=None, stats=None):
    """vxrt_render_path_temporal_motion over rows [y0, y1) of `scene` as it is now, with snapshot `snap`: temporal_ref.path_frame's dict
    with T from T_m, and prev_position / prev_normal (rows, w, 4), the guide of the primary hits"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim = dr.path_guides(scene, cam14, w, h, params, shadow, y0, y1, prim)
    px, c, traced, _ = pr.frame(scene, cam14, w, h, params, spp, bounces, seed, shadow, y0, y1, prim)
    Q, Nq = (a.reshape(y1 - y0, w, 4) for a in previous_positions(scene, snap, prim["hits"]))
    out = {"noisy": c, "direct": D, "albedo": A, "position": P, "normal": N, "rays": traced, "prev_position": Q, "prev_normal": Nq}
    hit = P[..., 3] != 0
    with np.errstate(all="ignore"):
        E = np.where(A > 0, (c - D) / A, f32(0.0)).astype(np.float32)
        E[~hit] = 0.0
        T = step(E, P, N, Q, Nq, hist, cam14, w, h, y0, y1, tp, stats)
        F = dr.atrous(T[..., :3], P, N, *dn)
        col = np.where(hit[..., None], D + A * F, D).astype(np.float32)
    out["E"], out["T"], out["F"] = E, T, F
    out["px"], out["col"] = cr.pack_rgb8(col.reshape(-1, 3)).reshape(y1 - y0, w), col
    return out
