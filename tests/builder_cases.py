"""Hostile inputs for both BVH builders (csrc/scene_builder.cpp on the CPU, csrc/bvh_builder.hip on the GPU): triangle soups where
surface areas overflow, underflow or tie everywhere, non-finite vertices, instance boxes for the TLAS, the mesh sizes that sit on the GPU
builder's hand-offs, and rays aimed at a box.  numpy only (no GPU, no torch).  Not a test module: tests/test_builder_cases_cpu.py,
tests/test_gpu_bvh_hostile.py and tests/test_gpu_refit_stress.py import it."""
import numpy as np

F32 = np.float32

# every family is a random soup -- centres uniform in +-80 around (200, 100, 0), vertices +-12 around each centre -- then:
FINITE = ("plain",         # nothing
          "huge",          # (v - mean) * 2e35: every product of two extents overflows
          "tiny",          # v * 1e-30: every product of two extents underflows to 0 (all surface areas tie)
          "subnormal",     # v * 1e-42: the coordinates themselves are subnormal (a few distinct values per axis)
          "offset",        # v * 0.01 + 1e7: one ulp is 1, most coordinates coincide
          "point",         # every vertex = the mean
          "plane",         # z = 3
          "line",          # y = 100, z = 0: every box has zero area
          "range",         # triangle 0 moved by +1e30: the others share one cell of any grid over the bounds
          "dups",          # every triangle = triangle 0
          "same_centre")   # segments symmetric about one point, different lengths: every box centre and centroid coincide
NON_FINITE = ("nan_vertex",   # one vertex of every 20th triangle NaN
              "nan_tri",      # three whole triangles NaN
              "inf_vertex",   # one coordinate +inf
              "overflow")     # scaled to +-3e38 about the origin: finite vertices, an axis extent of inf (a box that cannot be quantised)
# who may keep more than four triangles in a leaf: nothing tells their triangles apart but the position in the array
INDISTINGUISHABLE = ("dups", "point", "same_centre")
# where the reference's triangle test finds hits on aimed rays (elsewhere its products over- or underflow, or there is no area to hit)
HITTING = ("plain", "offset", "plane", "range", "dups")

# the GPU builder's hand-offs: around BB_TAIL = 1024 (global rounds -> the single-workgroup tail), one item in a last BB_TILE = 256 tile
# (1025, 1281, 2049, 4097), two read-backs of the cluster count (4097)
SIZES_EDGE = [1023, 1024, 1025, 1281, 2047, 2049, 4097]
SIZES_SMALL = [2, 3, 16, 17, 300]

CENTRE = np.array([200.0, 100.0, 0.0])


def soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-80, 80, size=(n, 1, 3))
    return (c + rng.uniform(-12, 12, size=(n, 3, 3)) + CENTRE).astype(F32)


def family(kind, n, seed=1):
    """float32 [n, 9]: n triangles of the family `kind` (FINITE + NON_FINITE)."""
    v = soup(n, seed)
    rng = np.random.default_rng(seed + 7)
    mean = v.reshape(-1, 3).mean(0)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if kind == "plain":
            pass
        elif kind == "huge":
            v = ((v - mean) * F32(2e35)).astype(F32)
        elif kind == "tiny":
            v = (v * F32(1e-30)).astype(F32)
        elif kind == "subnormal":
            v = (v * F32(1e-42)).astype(F32)
        elif kind == "offset":
            v = (v * F32(0.01) + F32(1e7)).astype(F32)
        elif kind == "point":
            v[...] = mean.astype(F32)
        elif kind == "plane":
            v[..., 2] = F32(3.0)
        elif kind == "line":
            v[..., 1] = F32(100)
            v[..., 2] = F32(0)
        elif kind == "range":
            v[0] = (v[0] + F32(1e30)).astype(F32)
        elif kind == "dups":
            v[...] = v[0]
        elif kind == "same_centre":
            r = rng.uniform(1, 60, size=(n, 1))
            u = rng.normal(size=(n, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            v = (np.stack([u * r, -u * r, np.zeros((n, 3))], 1) + CENTRE).astype(F32)
        elif kind == "nan_vertex":
            v[::20, 1, :] = np.nan
        elif kind == "nan_tri":
            v[rng.choice(n, size=min(3, n), replace=False)] = np.nan
        elif kind == "inf_vertex":
            v[n // 2, 2, 0] = np.inf
        elif kind == "overflow":      # the soup scaled to +-3e38 about the origin: every vertex finite, hi - lo = inf
            u = v.astype(np.float64) - mean
            v = (u / np.abs(u).max() * 3e38).astype(F32)
        else:
            raise ValueError(kind)
    return np.ascontiguousarray(v.reshape(n, 9), F32)


def aim_box(tri, kind=None):
    """lo, hi of the finite part of a mesh the rays are aimed at (for `range`: without the outlier)."""
    v = np.asarray(tri, F32).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    if kind == "range":
        v = v[np.abs(v).max(1) < 1e20]
    return v.min(0), v.max(0)


def aimed_rays(rng, lo, hi, n=64):
    """Rays from around the box lo / hi at points inside it (unit directions, no zero component)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = (lo + hi) / 2
    size = float((hi - lo).max())
    if not size > 0:
        size = max(float(np.abs(c).max()) * 1e-3, 1e-30)
    d = rng.normal(size=(n, 3))
    org = c + 3 * size * d / np.linalg.norm(d, axis=1, keepdims=True)
    tgt = lo + rng.random((n, 3)) * (hi - lo)
    dirn = tgt - org
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    rays = np.concatenate([org, dirn], 1).astype(F32)
    return rays[(rays[:, 3:] != 0).all(1) & np.isfinite(rays).all(1)]


def rays_at(tri, kind=None, n=96, seed=3):
    """The aimed rays every builder test traces: n rays (seed 3) at the finite part of the mesh."""
    with np.errstate(all="ignore"):
        lo, hi = aim_box(tri, kind)
        return aimed_rays(np.random.default_rng(seed), lo, hi, n)


BOX_KINDS = ("grid", "coincident", "nested", "flat", "tiny", "huge", "offset")


def boxes(kind, n, seed=1):
    """float32 [n, 6] (lo, hi): n instance boxes of the family `kind` (BOX_KINDS + "nan_box")."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1.0 / 3.0)))
    i = np.arange(n)
    g = np.stack([i % k, (i // k) % k, i // (k * k)], 1).astype(np.float64)
    lo = CENTRE + 30.0 * g + rng.uniform(-3, 3, size=(n, 3))
    hi = lo + rng.uniform(5, 25, size=(n, 3))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if kind == "grid":
            pass
        elif kind == "coincident":
            lo[...] = lo[0]
            hi[...] = hi[0]
        elif kind == "nested":       # box i strictly inside box i-1 (in fp32: the steps are 1/8)
            lo = CENTRE - 1000.0 + 0.125 * i[:, None]
            hi = CENTRE + 1000.0 - 0.125 * i[:, None]
        elif kind == "flat":         # lo == hi on one axis; every third box on all three
            hi[:, 1] = lo[:, 1]
            hi[::3] = lo[::3]
        elif kind == "tiny":
            lo, hi = lo * 1e-30, hi * 1e-30
        elif kind == "huge":
            m = lo.mean(0)
            lo, hi = (lo - m) * 2e35 / k, (hi - m) * 2e35 / k
        elif kind == "offset":
            lo, hi = lo * 0.01 + 1e7, hi * 0.01 + 1e7
        elif kind == "nan_box":
            lo[n // 2, 1] = np.nan
        else:
            raise ValueError(kind)
        out = np.concatenate([lo, hi], 1).astype(F32)
    if kind != "nan_box":
        assert np.isfinite(out).all() and (out[:, 3:] >= out[:, :3]).all()
    return np.ascontiguousarray(out)
