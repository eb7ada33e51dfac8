"""Randomised SHADING inputs for the closest-hit / miss shader (shade_terms, shade_eval of csrc/rt_shading.h, pack_rgb8 of csrc/rt_internal.h and their
restatement in oracle/rt_oracle.c), shared by tests/test_shading_cpu.py and tests/test_gpu_shading_fuzz.py.  TEST INFRASTRUCTURE ONLY.

geometry(seed)   the triangle soups and transforms of tests/test_gpu_fuzz.py (1-4 instances, rotations x non-uniform scales)
decorate(...)    overwrites triEx, mat, tex and blas[..].reflectivity of the BUILT scene in place of the builder's defaults -- after
                 the build, so that the builder's triangle order cannot matter -- and returns the shade-parameter sets of the case
case(...)        geometry -> scene.from_triangles -> decorate

Three families (FAMILIES).  Every range and seed below is a module constant.
  benign    unit normals that differ per corner, uv in [0, 1), 2-6 materials of which half are textured, textures of TEX_SIZES
            with pairwise different texels, ambient / light colour / background in [0, 1]
  hostile   every value inside what C defines: unnormalised and cancelling normals, negative / huge / boundary / -0.0 uv, lights on
            and next to surfaces, channels above 1 and below 0, reflectivities outside [0, 1], garbage in an untextured material
  outside_c values whose float -> integer conversion C leaves undefined: uv * w >= 2^63, +-inf and NaN uv, channels with
            c * 255 beyond +-2^31, NaN and inf shade parameters.  The rule for them is written in include/vortex_hip.h
            (vxrt_shade_rays) and pinned in tests/test_shading_cpu.py"""
import numpy as np

f32 = np.float32

FAMILIES = ("benign", "hostile", "outside_c")
SEEDS = tuple(range(6))                     # the committed seeds (VXRT_FUZZ_SEEDS=n runs n of them on the GPU)
SEED_BASE = {"benign": 31000, "hostile": 32000, "outside_c": 33000}
N_INSTANCES = (1, 4)                        # inclusive
TRIS_PER_MESH = (80, 400)
SCALE_RANGE = (15.0, 50.0)                  # per axis: non-uniform
TRANSLATE = ((180.0, 350.0), (60.0, 140.0), (-100.0, 100.0))   # in front of the fixed camera ((0, 100, 0) looking along +x)
N_MATERIALS = (2, 6)                        # inclusive; n // 2 of them textured
TEX_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (23, 37), (64, 64), (255, 3))     # (width, height)
HOSTILE_NORMAL_LENGTHS = (-20.0, 18.0)      # decimal exponents of the unnormalised normals' lengths
HOSTILE_UV_HUGE_BITS = (8, 31)              # |uv * w| up to 2^31
HOSTILE_REFLECTIVITY = (0.0, 0.3, 1.0, 1.5, -0.5)
BENIGN_REFLECTIVITY = (0.0, 0.25, 0.5)
HOSTILE_LIGHT_COLORS = (50.0, -50.0)
LIGHT_BOX = ((50.0, 300.0), (150.0, 400.0), (-200.0, 200.0))
OUTSIDE_UV = (2.0 ** 63, 2.0 ** 64, 3.0e38, -1.0e19, -3.0e38, float("inf"), float("-inf"), float("nan"))
OUTSIDE_LIGHT_COLOR = -1.0e12               # channels with c * 255 below -2^31
FRAME_SIZES = ((104, 72), (67, 45))         # ragged: neither a multiple of the 8 x 8 tiles

MAT_DT = np.dtype([("f", "<f4", 16), ("tex_id", "<i4"), ("illum", "<i4"), ("tw", "<u4"), ("th", "<u4"), ("off", "<u8")])
assert MAT_DT.itemsize == 88
KEYS = ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _soup(rng, n):
    c = rng.uniform(-1, 1, size=(n, 1, 3))
    size = rng.choice([0.1, 0.4, 1.0], size=(n, 1, 1))
    return (c + rng.uniform(-1, 1, size=(n, 3, 3)) * size).astype(np.float32).reshape(n, 9)


def geometry(seed, family):
    """(meshes, transforms) of the case: lists of (n, 9) f32 triangle soups and 4 x 4 f32 object-to-world matrices"""
    rng = np.random.default_rng(SEED_BASE[family] + seed)
    meshes, xf = [], []
    for _ in range(int(rng.integers(N_INSTANCES[0], N_INSTANCES[1] + 1))):
        meshes.append(_soup(rng, int(rng.integers(TRIS_PER_MESH[0], TRIS_PER_MESH[1] + 1))))
        m = np.eye(4)
        m[:3, :3] = _rot(rng) @ np.diag(rng.uniform(SCALE_RANGE[0], SCALE_RANGE[1], 3))
        m[:3, 3] = [rng.uniform(lo, hi) for lo, hi in TRANSLATE]
        xf.append(m.astype(np.float32))
    return meshes, xf


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _materials(rng, family):
    """(mat bytes, tex bytes, list of (w, h) per material or None)"""
    n = int(rng.integers(N_MATERIALS[0], N_MATERIALS[1] + 1))
    n_tex = n // 2
    sizes = [TEX_SIZES[i] for i in rng.choice(len(TEX_SIZES), n_tex, replace=False)]
    if family != "benign" and (1, 1) not in sizes:
        sizes[0] = (1, 1)                                    # (the hostile families always sample a 1 x 1 texture)
    if family == "outside_c":
        sizes[-1] = (23, 37) if n_tex > 1 else sizes[-1]
    textured = np.zeros(n, bool)
    textured[rng.choice(n, n_tex, replace=False)] = True
    mat = np.zeros(n, MAT_DT)
    mat["f"] = rng.uniform(0, 1, (n, 16)).astype(np.float32)       # ambient, DIFFUSE (f[3:6]), specular, ... : only diffuse is read
    mat["tex_id"] = -1
    texels, dims, off, k = [], [None] * n, 0, 0
    salt = np.uint64(rng.integers(0, 1 << 24))
    for i in np.nonzero(textured)[0]:
        w, h = sizes[k]
        k += 1
        mat["tex_id"][i], mat["tw"][i], mat["th"][i], mat["off"][i] = k - 1, w, h, off
        dims[i] = (w, h)
        # pairwise different texels over the whole buffer (an odd multiplier is a bijection mod 2^24), so that a wrong
        # index, stride or texture shows in the colour
        idx = np.arange(off // 4, off // 4 + w * h, dtype=np.uint64)
        texels.append(((idx * np.uint64(2654435761) + salt) & np.uint64(0xFFFFFF)).astype(np.uint32))
        off += 4 * w * h                                       # (4-byte aligned offsets)
    if family != "benign":
        # an untextured material whose texture fields are garbage: diffuse_tex_id = -1 means they are never read
        j = int(np.nonzero(~textured)[0][0])
        mat["tw"][j], mat["th"][j], mat["off"][j] = 0xFFFFFFFF, 0, 0xDEADBEEFDEADBEEF
    tex = np.concatenate(texels).view(np.uint8) if texels else np.zeros(4, np.uint8)
    return mat.view(np.uint8).reshape(-1).copy(), tex.copy(), dims


def _benign_triex(rng, n, dims):
    ex = np.zeros((n, 16), np.float32)
    for c in range(3):
        ex[:, 3 * c:3 * c + 3] = _unit(rng, n)                  # a different unit normal per corner
    ex[:, 9:15] = rng.uniform(0, 1, (n, 6)).astype(np.float32) * f32(0.99999)
    ex.view(np.uint32)[:, 15] = rng.permutation(n) % len(dims)      # materials dealt round robin: every one is used
    return ex


def _hostile_triex(rng, n, dims, tri_obj):
    ex = _benign_triex(rng, n, dims)
    tex_id = ex.view(np.uint32)[:, 15].astype(np.int64)
    w = np.array([dims[t][0] if dims[t] else 1 for t in tex_id], np.float64)
    h = np.array([dims[t][1] if dims[t] else 1 for t in tex_id], np.float64)
    ncls = rng.integers(0, 5, n)
    d = _unit(rng, n)
    # 0: unnormalised, lengths 1e-20 .. 1e18 (one direction and one decade per triangle, a different length within it per corner)
    s = ncls == 0
    decade = rng.uniform(HOSTILE_NORMAL_LENGTHS[0], HOSTILE_NORMAL_LENGTHS[1] - 1.0, n)
    for c in range(3):
        ln = 10.0 ** (decade + rng.uniform(0, 1, n))
        ex[s, 3 * c:3 * c + 3] = (d[s] * ln[s, None]).astype(np.float32)
    # 1: corner normals that cancel: N1 = N2 = d, N0 = -d -> N1 * bx + N2 * by + N0 * bz is exactly 0 at bx = by = 1/4, bz = 1/2
    s = ncls == 1
    ex[s, 3:6] = ex[s, 6:9] = d[s]
    ex[s, 0:3] = -d[s]
    # 2: a zero normal at every corner
    ex[ncls == 2, 0:9] = 0.0
    # 3: the geometric normal of the triangle, either sign (half of them face away from the ray, half oppose it)
    s = ncls == 3
    v = tri_obj.reshape(-1, 3, 3).astype(np.float64)
    g = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    g = g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-30) * rng.choice([-1.0, 1.0], (n, 1))
    for c in range(3):
        ex[s, 3 * c:3 * c + 3] = g[s].astype(np.float32)
    # 4: stays benign
    ucls = rng.integers(0, 5, n)
    uv = ex[:, 9:15].astype(np.float64).reshape(n, 3, 2)
    wh = np.stack([w, h], 1)[:, None, :]
    # 0: negative
    s = ucls == 0
    uv[s] = -rng.uniform(0, 8, (int(s.sum()), 3, 2))
    # 1: |uv * w| up to 2^31, either sign, the three corners close to each other
    s = ucls == 1
    base = rng.choice([-1.0, 1.0], (n, 1, 2)) * 2.0 ** rng.uniform(HOSTILE_UV_HUGE_BITS[0], HOSTILE_UV_HUGE_BITS[1], (n, 1, 2)) / wh
    uv[s] = (base * (1.0 - rng.uniform(0, 1e-3, (n, 3, 2))))[s]
    # 2: on a texel boundary (j / w) or on a multiple of the texture's size (k), the same value at the three corners
    s = ucls == 2
    j = rng.integers(-3 * wh.astype(np.int64), 3 * wh.astype(np.int64) + 1).astype(np.float64)
    onb = np.where(rng.integers(0, 2, (n, 1, 2)) == 0, j / wh, np.round(j / wh))
    uv[s] = np.broadcast_to(onb, (n, 3, 2))[s]
    # 3: -0.0
    uv[ucls == 3] = -0.0
    ex[:, 9:15] = uv.reshape(n, 6).astype(np.float32)
    return ex, ncls


def _outside_triex(rng, n, dims):
    ex = _benign_triex(rng, n, dims)
    ucls = rng.integers(0, 3, n)                                   # 0: benign, 1: one value of OUTSIDE_UV at every corner, 2: mixed corners
    uv = ex[:, 9:15].reshape(n, 3, 2).copy()
    tab = np.array(OUTSIDE_UV, np.float32)
    pick = tab[rng.integers(0, len(tab), (n, 1, 2))]
    s = ucls == 1
    uv[s] = np.broadcast_to(pick, (n, 3, 2))[s]
    s = ucls == 2
    uv[s] = tab[rng.integers(0, len(tab), (n, 3, 2))][s]
    ex[:, 9:15] = uv.reshape(n, 6)
    return ex


def _params(po, ambient, light_color, light_pos, background, max_depth=1):
    return po.shade_params(tuple(float(v) for v in ambient), tuple(float(v) for v in light_color), tuple(float(v) for v in light_pos),
                           tuple(float(v) for v in background), int(max_depth))


def params_tuple(p):
    """(ambient, light_color, light_pos, background, max_depth) of a parameter set, as plain Python values"""
    return tuple(p.ambient), tuple(p.light_color), tuple(p.light_pos), tuple(p.background), int(p.max_depth)


def decorate(b, seed, family, po, xf, mesh_sizes):
    """b: the built scene's buffers (dict of uint8 arrays; triEx, mat, tex and the reflectivities are replaced in a copy); xf,
    mesh_sizes: the transforms and triangle counts of geometry()'s meshes (instance i owns the i-th range of triangles).
    Returns (b, [parameter sets], extra) -- extra["pairs"]: (rays, hit records) with hand-set barycentrics for the per-ray entry."""
    rng = np.random.default_rng(SEED_BASE[family] + 500 + seed)
    n = b["tri"].size // 36
    n_blas = b["blas"].size // 160
    mat, tex, dims = _materials(rng, family)
    tri_obj = np.frombuffer(b["tri"].tobytes(), np.float32).reshape(n, 9)
    ncls = None
    if family == "benign":
        ex = _benign_triex(rng, n, dims)
    elif family == "hostile":
        ex, ncls = _hostile_triex(rng, n, dims, tri_obj)
    else:
        ex = _outside_triex(rng, n, dims)
    b = dict(b)
    b["triEx"] = ex.view(np.uint8).reshape(-1).copy()
    b["mat"], b["tex"] = mat, tex
    blas = b["blas"].copy()
    rec = blas.view(np.float32).reshape(-1, 40)
    choices = HOSTILE_REFLECTIVITY if family == "hostile" else BENIGN_REFLECTIVITY
    refl = rng.choice(choices, n_blas)
    refl[int(rng.integers(0, n_blas))] = choices[1]              # at least one instance with 0 < reflectivity < 1
    rec[:, 38] = refl.astype(np.float32)
    b["blas"] = blas
    rnd_light = [rng.uniform(lo, hi) for lo, hi in LIGHT_BOX]
    u = lambda: rng.uniform(0, 1, 3)                               # noqa: E731
    extra = {"pairs": None}
    if family == "benign":
        plist = [_params(po, u(), u(), [rng.uniform(lo, hi) for lo, hi in LIGHT_BOX], u(), d) for d in (1, 2, 3)]
        return b, plist, extra
    # a first oracle trace of the frame's rays: hit points for the lights that sit on and next to surfaces
    rays = po.camera_rays(*FRAME_SIZES[0])
    hits, _ = po.trace_canonical(b, rays)
    found = np.nonzero(hits["dist"] != f32(1e30))[0]
    assert len(found) > 50, "the case's geometry must be visible"
    k0, k1 = (int(v) for v in rng.choice(found, 2, replace=False))
    I = lambda k: np.array([rays[k, c] + rays[k, 3 + c] * hits["dist"][k] for c in range(3)], np.float32)   # noqa: E731  (orig + dir * dist, rounded per operation)
    if family == "hostile":
        one_ulp_below = np.nextafter(f32(1.0), f32(0.0))
        inside = np.asarray(xf[int(rng.integers(0, len(xf)))], np.float32)[:3, 3]      # the centre of an instance's soup
        plist = [
            _params(po, u(), [HOSTILE_LIGHT_COLORS[0]] * 3, I(k0), [1.0, one_ulp_below, rng.uniform(0, 1)], 1),      # the light ON a hit point
            _params(po, [0, 0, 0], [HOSTILE_LIGHT_COLORS[1]] * 3, inside, [one_ulp_below, 1.0, 1.0], int(rng.integers(2, 5))),
            _params(po, u(), [HOSTILE_LIGHT_COLORS[0], HOSTILE_LIGHT_COLORS[1], 1.0], I(k1).astype(np.float64) + _unit(rng, 1)[0] * 1e6, u(), 2),
            _params(po, [0, 0, 0], u(), I(k1).astype(np.float64) + _unit(rng, 1)[0] * 1e-6, u(), int(rng.integers(1, 5))),
            _params(po, u(), u(), rnd_light, u(), 4),
        ]
        # per-ray pairs with the barycentrics at which the cancelling normals vanish, one per such triangle
        cancel = np.nonzero(ncls == 1)[0]
        blas_of = np.repeat(np.arange(n_blas, dtype=np.uint32), mesh_sizes)
        pr = np.zeros((len(cancel), 6), np.float32)
        pr[:, 0:3] = (0.0, 100.0, 0.0)
        pr[:, 3] = 1.0
        ph = np.zeros(len(cancel), po.HIT_DTYPE)
        ph["dist"], ph["bx"], ph["by"], ph["bz"] = 200.0, 0.25, 0.25, 0.5
        ph["blasIdx"], ph["triIdx"] = blas_of[cancel], cancel
        extra["pairs"] = (pr, ph)
        return b, plist, extra
    nan, inf = float("nan"), float("inf")
    plist = [
        _params(po, [1, 1, 1], [0, 0, 0], rnd_light, [0.25, 0.5, 0.75], 1),              # colour = texel / 256: shows which texel was read
        _params(po, u(), [OUTSIDE_LIGHT_COLOR] * 3, rnd_light, u(), 1),                  # c * 255 < -2^31
        _params(po, [3e38] * 3, [3e38] * 3, rnd_light, [-3e38, 3e38, 2.0], 1),           # finite parameters, inf and NaN colours
        _params(po, [nan, 0.5, 0.5], [inf, -inf, 1.0], rnd_light, [nan, inf, -inf], 1),
        _params(po, u(), u(), [nan, rnd_light[1], inf], u(), 1),
    ]
    return b, plist, extra


def case(vrt, po, seed, family):
    """(buffers, [parameter sets], extra) on the tree the CPU builder makes"""
    meshes, xf = geometry(seed, family)
    sc = vrt.scene.from_triangles(meshes, xf)
    b = {k: np.frombuffer(bytes(sc.buffers[k]), np.uint8).copy() for k in KEYS}
    return decorate(b, seed, family, po, xf, [len(m) for m in meshes])


def per_ray_inputs(po, b, seed, family, extra):
    """(rays, hit records) for the per-ray entry: the frame's camera rays and random rays with the oracle's hit records, plus the
    hand-set pairs of the case"""
    rng = np.random.default_rng(SEED_BASE[family] + 900 + seed)
    cam = po.camera_rays(*FRAME_SIZES[0])             # (the rays decorate() took its hit points from)
    n = 1200
    o = np.stack([rng.uniform(-50, 500, n), rng.uniform(-50, 300, n), rng.uniform(-250, 250, n)], 1)
    tgt = np.stack([rng.uniform(lo - 30, hi + 30, n) for lo, hi in TRANSLATE], 1)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([cam, np.concatenate([o, d], 1)]).astype(np.float32)
    hits, _ = po.trace_canonical(b, rays)
    if extra.get("pairs") is not None:
        rays = np.concatenate([rays, extra["pairs"][0]])
        hits = np.concatenate([hits, extra["pairs"][1]])
    return rays, hits
