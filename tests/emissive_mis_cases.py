"""The scenes, tables, cameras and configurations of tests/test_emissive_mis_cpu.py and tests/test_gpu_emissive_mis.py.  TEST
INFRASTRUCTURE ONLY.

All of it is emissive_cases.hall, whose dark ceiling panel lies 5 units above its 200 x 200 ceiling light: the place where the
emitter ray's G grows as 1 / d^2.  Three tables of it:
  full      every emissive triangle, the pair list in a seeded shuffled order, so that the table index e is not the sorted rank;
  partial   the same without one lamp triangle: it keeps emitting through bounce rays at full weight (wB = 1);
  twice     the lamp mesh placed under two instance records -- the same triIdx under two blasIdx.  vrt.scene.from_triangles gives every
            instance a mesh of its own, so the second placement is made as the shared-BLAS scenes of tests/test_gpu_refit_stress.py are:
            record 2 (the side mirror) is pointed at the lamp's BVH with a transform of its own and the TLAS is refitted on the host."""
import numpy as np

import emissive_cases as ec
import refit_ref as rr

SCALE = ec.SCALE
# (spp, bounces, shadow, seed)
CONFIGS = ((2, 3, 1, 3), (5, 2, 0, 0), (1, 1, 0, 7))
CAMERA_NAMES = ("framing", "orbit_1", "gap", None)   # None: the fixed camera
TABLE_NAMES = ("full", "partial", "twice")
SECOND_LAMP = 2                                      # the instance record that places the lamp mesh a second time


def gap_camera(vrt, w, h):
    """between the ceiling panel (y = 260) and the ceiling light (y = 255), looking along them"""
    return np.array(vrt.rtapi.look_at((60.0, 257.5, 0.0), (180.0, 257.5, 0.0), (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32)


def cameras(vrt, w, h):
    import camera_secondary_ref as csr
    c = csr.hall_cameras(vrt, w, h)
    return {"framing": c["framing"], "orbit_1": c["orbit_1"], "gap": gap_camera(vrt, w, h), None: None}


def shuffled(pairs, seed=11):
    p = np.asarray(pairs, np.uint32).reshape(-1, 2)
    return p[np.random.default_rng(seed).permutation(len(p))].copy()


def second_lamp_transform():
    cy, sy, cx, sx = np.cos(0.8), np.sin(0.8), np.cos(0.6), np.sin(0.6)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ np.diag([45.0, 30.0, 20.0])
    m[:3, 3] = (120.0, 60.0, -140.0)
    return m.astype(np.float32)


def lookup_keys(pairs):
    """(m, 2) u32 keys to look up in the index of `pairs`: every listed key, each key's two neighbours in triIdx and in blasIdx, keys below
    the smallest and above the largest, and listed keys with the top bit of blasIdx set (raw: no such key is listed)"""
    k = [int(b) * 2 ** 32 + int(t) for b, t in np.asarray(pairs, np.uint32).reshape(-1, 2)]
    lo, hi = min(k), max(k)
    cand = k + [v - 1 for v in k] + [v + 1 for v in k] + [v - 2 ** 32 for v in k] + [v + 2 ** 32 for v in k] + [v + 2 ** 63 for v in k[:8]]
    cand += [lo - 1, lo - 2, 0, hi + 1, hi + 2, 2 ** 63 - 1, 2 ** 64 - 1]
    ks = np.array([v for v in cand if 0 <= v < 2 ** 64], np.uint64)
    return np.stack([(ks >> np.uint64(32)), ks & np.uint64(0xFFFFFFFF)], 1).astype(np.uint32)


def unxorshift(r):
    """the state whose xorshift is r (each of the three steps undone)"""
    r &= 0xFFFFFFFF
    x = r
    for _ in range(7):
        x = r ^ ((x << 5) & 0xFFFFFFFF)
    r = x
    for _ in range(2):
        x = r ^ (x >> 17)
    r = x
    for _ in range(3):
        x = r ^ ((x << 13) & 0xFFFFFFFF)
    return x


def near_field(tab, per=10, seed=3):
    """(seeds (m,) u32, I (m, 3), N' (m, 3)): for every entry e of the table, ray origins at `per` distances 1e-3 .. 10 from the point the
    seed samples on e, along e's normal on both sides, with N' towards the emitter and at a grazing angle to it -- where the emitter
    ray's G grows as 1 / d^2"""
    import emissive_ref as er
    tri12, q, cum, Q = tab
    rng = np.random.default_rng(seed)
    seeds, I, N = [], [], []
    for e in range(len(q)):
        T = tri12[e].astype(np.float64)
        n = np.cross(T[3:6], T[6:9])
        n /= np.linalg.norm(n)
        t1 = T[3:6] / np.linalg.norm(T[3:6])
        lo, hi = (0 if e == 0 else int(cum[e - 1])), int(cum[e])
        for d in np.geomspace(1e-3, 10.0, per):
            for side in (1.0, -1.0):
                for graze in (False, True):
                    t = int(rng.integers(lo, hi))
                    r0 = max(-((-t << 32) // Q), 1)                   # the smallest r0 with (r0 * Q) >> 32 == t
                    s = unxorshift(r0)
                    st = er.xorshift(np.array([r0], np.uint32))
                    a = float(er.to_float(st)[0])
                    b = float(er.to_float(er.xorshift(st))[0])
                    if np.float32(a) + np.float32(b) > np.float32(1.0):
                        a, b = 1.0 - a, 1.0 - b
                    P = T[0:3] + a * T[3:6] + b * T[6:9]
                    nn = -side * n
                    if graze:
                        nn = 0.02 * nn + t1
                        nn /= np.linalg.norm(nn)
                    seeds.append(s); I.append(P + side * n * d - nn * 0.001); N.append(nn)
    return np.array(seeds, np.uint32), np.array(I, np.float32), np.array(N, np.float32)


def hall(vrt, which):
    """(scene buffers, pairs (n, 2) u32 in the order the table takes them) of TABLE_NAMES[...] = which"""
    b, ranges = ec.hall(vrt)
    pairs = vrt.rtapi.emitter_pairs(b, ranges)
    if which == "partial":
        lamp = np.nonzero(pairs[:, 0] == ec.LAMP)[0]
        pairs = np.delete(pairs, lamp[-1], 0)
    elif which == "twice":
        rec = b["blas"].view(np.float32).reshape(-1, rr.BLAS_WORDS)
        rec[SECOND_LAMP] = rec[ec.LAMP]                               # (the lamp's BVH offset and everything else of its record)
        rec[SECOND_LAMP, 38] = 0.0
        b["blas"] = rr.set_transforms(b["blas"], SECOND_LAMP, [second_lamp_transform()])
        b["tlas"], _ = rr.refit(b, geometry=False)
        again = pairs[pairs[:, 0] == ec.LAMP].copy()
        again[:, 0] = SECOND_LAMP
        pairs = np.concatenate([pairs, again])
    else:
        assert which == "full"
    return b, shuffled(pairs)
