"""Hand-built scenes in the software twin's formats (include/vortex_hip.h vxrc_scene_t; raycast/common.h) that reach the parts of
csrc/rc_kernels.hip the fixtures and the package builder never do: by-reference leaves, every wide-node shape, distance ties, boxes that
switch the build to the two-wide walk or the libstdc++ slab form, rays outside the fast domain next to rays inside it, TLAS shapes,
mirror chains and the conversions C leaves undefined.  numpy only.  Every index of every scene is well formed.

A case is a dict: scene (the seven buffers + tlas_root), cam (14 floats), light (12 floats), spp, depth, w, h, info (what vxrc_accel_info(0)
must report), elements (what the case exists for: label -> (blasIdx or None, set of global triangle indices or None); a primary ray counts
for an element when its closest hit names them), and flags read by tests/test_rc_hostile_cpu.py.  CASES maps a name to a builder; case(name)
builds and caches."""
import numpy as np

F = np.float32
W, H = 97, 61                      # neither a multiple of 8; both odd: with an axis-aligned camera the centre column / row has a zero direction component
LIGHT = (0.0, 150.0, -50.0, 8.0, 8.0, 8.0, 0.3, 0.3, 0.3, 0.4, 0.35, 0.25)


def cam_axis(w, h, pos=(0.0, 100.0, 0.0)):
    """eye looking along +x, right = +z, up = +y, 90 degrees vertical field of view"""
    return np.array([pos[0], pos[1], pos[2], 1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0], F)


def cam_tilted(w, h, pos=(0.0, 100.0, 0.0), yaw=0.03, pitch=-0.02):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    fwd = np.array([cy * cp, sp, sy * cp])
    right = np.array([-sy, 0.0, cy])
    up = np.cross(right, fwd)
    return np.concatenate([pos, fwd, right, up, [2.0 * w / h, 2.0]]).astype(F)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
def grid_mesh(ny, nz, y=(40.0, 160.0), z=(-80.0, 80.0), x=62.0, bump=0.0, seed=0, tilt=(0.0, 0.0)):
    """ny x nz quads (two triangles each) on the plane x = const (+ a random bump per vertex), facing -x.  Returns tris [n, 9] and
    triEx [n, 15] (N0 N1 N2 uv0 uv1 uv2): normals near (-1, tilt) with a little noise per vertex, uv = position in the grid."""
    rng = np.random.default_rng(seed)
    ys, zs = np.linspace(y[0], y[1], ny + 1), np.linspace(z[0], z[1], nz + 1)
    X = x + bump * rng.uniform(-1, 1, (ny + 1, nz + 1))
    Nn = np.stack([-np.ones((ny + 1, nz + 1)), tilt[0] + 0.15 * rng.uniform(-1, 1, (ny + 1, nz + 1)),
                   tilt[1] + 0.15 * rng.uniform(-1, 1, (ny + 1, nz + 1))], -1)
    Nn /= np.linalg.norm(Nn, axis=-1, keepdims=True)
    tris, ex = [], []
    for i in range(ny):
        for j in range(nz):
            q = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            for c in ((0, 1, 2), (0, 2, 3)):
                v = [q[k] for k in c]
                tris.append(np.concatenate([[X[a, b], ys[a], zs[b]] for a, b in v]))
                ex.append(np.concatenate([Nn[a, b] for a, b in v] + [[a / ny, b / nz] for a, b in v]))
    return np.array(tris, F), np.array(ex, F)


def median_tree(tris, ids, leaf):
    """median split on the axis of the largest centroid extent; a leaf is a list of triangle ids, an internal node a pair"""
    ids = list(ids)
    if len(ids) <= leaf:
        return ids
    c = tris[ids].reshape(len(ids), 3, 3).mean(1)
    ax = int(np.argmax(c.max(0) - c.min(0)))
    order = [ids[k] for k in np.argsort(c[:, ax], kind="stable")]
    m = len(order) // 2
    return (median_tree(tris, order[:m], leaf), median_tree(tris, order[m:], leaf))


def shuffled(tris, ex, seed):
    """the triangles in a random order, so that triIdx (leaf order) is a real permutation"""
    p = np.random.default_rng(seed).permutation(len(tris))
    return tris[p], ex[p]


def emit(tree, tris, pad=0.0):
    """BVH2 in the reference's layout: root in slot 0, slot 1 empty, children as adjacent pairs stored after their parent; a leaf's box is
    the exact bounds of its vertices (+ pad), an internal node's the exact float32 union of its children's.  Returns the node dicts by slot."""
    nodes = [None, None]

    def rec(t, at, parent):
        if isinstance(t, tuple):
            l = len(nodes)
            nodes.extend([None, None])
            a, b = rec(t[0], l, at), rec(t[1], l + 1, at)
            n = {"lo": np.minimum(a["lo"], b["lo"]), "hi": np.maximum(a["hi"], b["hi"]), "left": l, "ids": a["ids"] + b["ids"], "leaf": False}
        else:
            v = tris[list(t)].reshape(-1, 3)
            n = {"lo": v.min(0) - F(pad), "hi": v.max(0) + F(pad), "ids": list(t), "leaf": True}
        n["at"], n["parent"] = at, parent
        nodes[at] = n
        return n

    rec(tree, 0, None)
    return nodes


def mesh(tris, ex, tree=None, leaf=4, pad=0.0):
    tree = median_tree(tris, range(len(tris)), leaf) if tree is None else tree
    return {"tris": tris, "ex": ex, "nodes": emit(tree, tris, pad)}


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def xform(A=np.eye(3), t=(0, 0, 0)):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = A, t
    return M


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def texture(w, h, seed):
    rng = np.random.default_rng(1000 + seed)
    c = rng.integers(64, 256, (h * w, 3)).astype(np.uint32)
    return (c[:, 0] << 16 | c[:, 1] << 8 | c[:, 2]).astype(np.uint32).reshape(h, w)


def tlas_tree(n, shape):
    """leaf = instance number, internal = pair"""
    if shape == "chain":                       # n - 1 internal levels, the leaf alternately left and right
        t = (n - 2, n - 1)
        for k in range(n - 3, -1, -1):
            t = (k, t) if k % 2 == 0 else (t, k)
        return t

    def bal(lo, hi):
        if hi - lo == 1:
            return lo
        m = (lo + hi + 1) // 2
        return (bal(lo, m), bal(m, hi))
    return bal(0, n)


def assemble(meshes, insts, textures, tlas="balanced"):
    """insts: dicts with mesh, xf (4x4 world from object; float64), tex, refl and optionally inv (4x4 used as given) and box (lo, hi: the
    instance's TLAS box, else the transformed corners of the mesh's root box, padded)."""
    tri = np.concatenate([m["tris"] for m in meshes])
    ex = np.concatenate([m["ex"] for m in meshes])
    tri_base = np.cumsum([0] + [len(m["tris"]) for m in meshes])
    node_base = np.cumsum([0] + [len(m["nodes"]) for m in meshes])
    bvh = np.zeros((node_base[-1], 8), np.uint32)
    fb = bvh.view(F)
    tri_idx = []
    for k, m in enumerate(meshes):
        m["tri_base"], m["node_base"] = int(tri_base[k]), int(node_base[k])
        for n in m["nodes"]:
            if n is None:
                continue
            r = node_base[k] + n["at"]
            fb[r, 0:3], fb[r, 4:7] = n["lo"], n["hi"]
            if n["leaf"]:
                bvh[r, 3], bvh[r, 7] = len(tri_idx), len(n["ids"])
                tri_idx += [int(tri_base[k]) + i for i in n["ids"]]
            else:
                bvh[r, 3], bvh[r, 7] = n["left"], 0                 # relative to the instance's bvh_offset (render.h:103)
    assert sorted(tri_idx) == list(range(len(tri))) and tri_idx != list(range(len(tri)))
    tex_off, words = [], [np.full(4, 0x00FF00FF, np.uint32)]       # 16 bytes in front: no texture at offset 0
    for t in textures:
        tex_off.append(4 * sum(len(x) for x in words))
        words.append(np.ascontiguousarray(t, np.uint32).reshape(-1))
    blas = np.zeros((len(insts), 40), np.uint32)
    bf = blas.view(F)
    boxes = []
    for j, it in enumerate(insts):
        M = np.asarray(it["xf"], np.float64)
        inv = np.asarray(it["inv"], np.float64) if "inv" in it else np.linalg.inv(M)
        bf[j, 0:16], bf[j, 16:32] = M.reshape(-1), inv.reshape(-1)
        m = meshes[it["mesh"]]
        th, tw = textures[it["tex"]].shape
        blas[j, 32], blas[j, 34], blas[j, 36], blas[j, 37] = m["node_base"], tex_off[it["tex"]], tw, th
        bf[j, 38] = it.get("refl", 0.0)
        if "box" in it:
            lo, hi = np.array(it["box"][0], F), np.array(it["box"][1], F)
        else:
            r = m["nodes"][0]
            c = np.array([[(r["lo"], r["hi"])[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
            wc = c @ M[:3, :3].T + M[:3, 3]
            e = 1e-3 * (wc.max(0) - wc.min(0)) + 1e-3
            lo, hi = (wc.min(0) - e).astype(F), (wc.max(0) + e).astype(F)
        boxes.append((lo, hi))
    n = len(insts)
    tl = []

    def rec(t):
        if isinstance(t, tuple):
            at = len(tl)
            tl.append(None)
            a, b = rec(t[0]), rec(t[1])
            tl[at] = (np.minimum(tl[a][0], tl[b][0]), np.maximum(tl[a][1], tl[b][1]), a | (b << 16), 0)
            assert tl[at][2] != 0 and max(a, b) < 65536
            return at
        tl.append((boxes[t][0], boxes[t][1], 0, t))
        return len(tl) - 1

    tl.append((np.zeros(3, F), np.zeros(3, F), 0, 0))               # slot 0: an unreferenced leaf record, so that the root is not node 0
    root = rec(tlas_tree(n, tlas) if n > 1 else 0)
    tlas_b = np.zeros((len(tl), 8), np.uint32)
    for i, (lo, hi, lr, b) in enumerate(tl):
        tlas_b.view(F)[i, 0:3], tlas_b.view(F)[i, 4:7] = lo, hi
        tlas_b[i, 3], tlas_b[i, 7] = lr, b
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
    return {"tlas": u8(tlas_b), "blas": u8(blas), "bvh": u8(bvh), "tri": u8(tri), "triEx": u8(ex), "triIdx": u8(np.array(tri_idx, np.uint32)),
            "tex": u8(np.concatenate(words)), "tlas_root": root}


def _case(scene, cam, elements, w=W, h=H, light=LIGHT, spp=1, depth=1, info=1, **flags):
    d = {"scene": scene, "cam": np.asarray(cam, F), "light": tuple(float(v) for v in light), "spp": spp, "depth": depth, "w": w, "h": h,
         "info": info, "elements": elements}
    d.update(flags)
    return d


def _gids(m, ids):
    return {m["tri_base"] + i for i in ids}


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def _ties_mesh(swap):
    """a flat axis-aligned grid, every triangle three times, bit-identical, each copy with its own normals and uv.  All boxes share the
    planes x = 62, and with an axis-aligned camera every box a ray goes through is entered at the same distance: every `dLeft < dRight` on
    the way is a tie, and the copy visited first keeps the hit (strict `<`).  The grid is cut into three strips along z; in each the copies
    are subtrees of their own (leaf sizes 2, 3 and 1: different shapes) arranged differently -- ((0, 1), 2), (1, (2, 0)), ((2, 0), 1) -- so
    that each copy wins one strip, the order inside a side of a wide node decides the first and the third, the order of the sides all three."""
    copies = [grid_mesh(6, 9, y=(50, 150), z=(-72, 72), tilt=t, seed=s) for t, s in (((0.0, 0.0), 1), ((0.6, 0.0), 2), ((0.0, -0.6), 3))]
    n = len(copies[0][0])
    tris = np.concatenate([copies[0][0]] * 3)
    exs = [c[1].copy() for c in copies]
    for k in range(3):
        exs[k][:, 9:15] = np.clip(copies[k][1][:, 9:15] * (0.3 + 0.3 * k) + 0.2 * k, 0, 0.999)
    if swap:
        nrm = [e[:, 0:9].copy() for e in exs]
        for k in range(3):
            exs[k][:, 0:9] = nrm[(k + 1) % 3]
    ex = np.concatenate(exs)
    p = np.random.default_rng(7).permutation(3 * n)
    inv = np.argsort(p)
    tris, ex = tris[p], ex[p]
    cz = copies[0][0].reshape(n, 3, 3).mean(1)[:, 2]
    strip = np.digitize(cz, [-24.0, 24.0])
    sub = [[median_tree(tris, [int(inv[k * n + i]) for i in range(n) if strip[i] == r], leaf) for k, leaf in enumerate((2, 3, 1))] for r in range(3)]
    tree = (((sub[0][0], sub[0][1]), sub[0][2]), ((sub[1][1], (sub[1][2], sub[1][0])), ((sub[2][2], sub[2][0]), sub[2][1])))
    m = mesh(tris, ex, tree=tree)
    m["copies"] = [[int(inv[k * n + i]) for i in range(n)] for k in range(3)]
    return m


def ties(swap=False):
    m = _ties_mesh(swap)
    sc = assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}], [texture(9, 7, 0)])
    return _case(sc, cam_axis(W, H), {"copy_%d_wins" % k: (0, _gids(m, ids)) for k, ids in enumerate(m["copies"])}, swappable=True)


def ties_instances(swap=False):
    """the same mesh instanced twice with the identical transform: equal TLAS distances (render.h:176) and equal hits; the instance that
    wins shows through its texture"""
    m = _ties_mesh(swap)
    sc = assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}, {"mesh": 0, "xf": xform(), "tex": 1, "refl": 0.25}], [texture(9, 7, 0), texture(5, 3, 1)])
    el = {"copy_%d_wins" % k: (0, _gids(m, ids)) for k, ids in enumerate(m["copies"])}      # (and the first instance every time)
    return _case(sc, cam_axis(W, H), el, depth=2, swappable=True)


# ---- leaf sizes -----------------------------------------------------------------------------------------------------------------
LEAF_SIZES = (1, 2, 31, 32, 33, 40)


def leaf_sizes():
    """leaves of 1, 2, 31, 32 (inline descriptors), 33 and 40 triangles (by reference) under internal nodes of all four shapes:
    root = (I1, I2) both internal; I1 = (leaf, internal); I2 = (internal, leaf); the two lowest both leaves"""
    tris, ex = shuffled(*grid_mesh(10, 7, y=(45, 155), z=(-75, 75), bump=6.0, seed=4), seed=5)
    c = tris.reshape(-1, 3, 3).mean(1)
    order = list(np.lexsort((c[:, 1], np.round(c[:, 2] / 21.5))))      # strips along z
    g, at = {}, 0
    for s in (40, 33, 1, 2, 31, 32):                                    # the small leaves in the middle of the frame
        g[s] = [int(i) for i in order[at:at + s]]
        at += s
    keep = sorted(int(i) for i in order[:at])                           # (the grid has one triangle more than the leaves hold)
    new = {old: k for k, old in enumerate(keep)}
    g = {s: [new[i] for i in ids] for s, ids in g.items()}
    tree = ((g[1], (g[2], g[31])), ((g[33], g[40]), g[32]))
    m = mesh(tris[keep], ex[keep], tree=tree)
    sc = assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}], [texture(6, 6, 2)])
    return _case(sc, cam_axis(W, H), {"leaf_%d" % s: (0, _gids(m, g[s])) for s in LEAF_SIZES})


def leaf_single():
    """two instances whose BVH is a single leaf node (the root descriptor is the leaf): 6 triangles inline, 36 by reference"""
    a = mesh(*shuffled(*grid_mesh(1, 3, y=(60, 140), z=(-75, -15), bump=3.0, seed=6), seed=1), tree=[4, 1, 5, 0, 3, 2])
    b = mesh(*shuffled(*grid_mesh(6, 3, y=(60, 140), z=(15, 75), bump=3.0, seed=7), seed=2), tree=list(range(35, -1, -1)))
    sc = assemble([a, b], [{"mesh": 0, "xf": xform(), "tex": 0}, {"mesh": 1, "xf": xform(), "tex": 1}], [texture(4, 4, 3), texture(5, 2, 4)])
    return _case(sc, cam_axis(W, H), {"inline": (0, None), "by_reference": (1, None)})


# ---- boxes ----------------------------------------------------------------------------------------------------------------------
def _boxes(kind):
    m = mesh(*shuffled(*grid_mesh(8, 10, y=(45, 155), z=(-78, 78), bump=8.0, seed=8), seed=3), leaf=3, pad=0.5 if kind == "padded" else 0.0)
    # an internal node below the root with a fair share of the mesh: a child whose box the wide layout recomputes from ITS children
    t = next(n for n in m["nodes"] if n is not None and not n["leaf"] and n["parent"] is not None and n["parent"] != 0 and len(n["ids"]) >= 16)
    lo, hi = t["lo"].copy(), t["hi"].copy()
    if kind == "ulp":
        hi[0] = np.nextafter(hi[0], F(np.inf))
    elif kind == "ten_percent":
        e = hi - lo
        lo, hi = lo - F(0.05) * e, hi + F(0.05) * e
    elif kind == "inverted":
        lo[1], hi[1] = hi[1], lo[1]
    elif kind == "inf":
        hi[0] = np.inf
    elif kind == "huge":
        hi[0] = F(2.0 ** 61)
    elif kind == "nan":
        hi[0] = np.nan                     # the far plane of a ray going +x: the slab chain falls back on the near plane (libstdc++ min / max)
    t["lo"], t["hi"] = lo, hi
    sc = assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}], [texture(8, 8, 5)])
    return _case(sc, cam_axis(W, H), {"subtree": (0, _gids(m, t["ids"]))}, info=1 if kind in ("exact", "padded") else 0)


# ---- slow rays ------------------------------------------------------------------------------------------------------------------
def _slow_mesh(seed=9, **kw):
    g = dict(y=(40, 160), z=(-80, 80), bump=5.0, seed=seed)
    g.update(kw)
    return mesh(*shuffled(*grid_mesh(8, 8, **g), seed=seed), leaf=2)


def slow_axis():
    """axis-aligned camera, odd width and height: the centre column has dz = 0 exactly, the centre row dy = 0 -- lanes outside the fast
    domain in the same 8x8 tiles as lanes inside it"""
    m = _slow_mesh()
    return _case(assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}], [texture(8, 8, 6)]), cam_axis(W, H), {"mesh": (0, None)}, slow=True)


def slow_on_plane():
    """as slow_axis with a flat grid whose vertices lie on y = 100 and z = 0, the camera's own coordinates: the slabs of the zero components
    are 0 * inf = NaN on those planes"""
    m = mesh(*shuffled(*grid_mesh(8, 8, y=(40, 160), z=(-80, 80), seed=10), seed=10), leaf=2)
    return _case(assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}], [texture(8, 8, 7)]), cam_axis(W, H), {"mesh": (0, None)}, slow=True)


def slow_instances():
    """three instances side by side: an ordinary one; one whose inverse transform has a zero row (object-space dy = 0 for every ray, all
    rays in the plane y = 100); one scaled by 2^-70 (1/d beyond 2^64: every lane that walks it is outside the fast domain, walks the tree
    like an ordinary ray and hits nothing, its determinants fall below the reference's epsilon) in front of an ordinary one"""
    m = _slow_mesh(seed=11, z=(-25, 25))
    flat = np.eye(4)
    flat[1, :] = (0, 0, 0, 100.0)
    flat[2, 3] = 60.0                                              # world z -> object z + 60
    tiny = np.diag([2.0 ** -70] * 3 + [1.0])
    tiny[:3, 3] = (0, 100.0, 0)
    insts = [{"mesh": 0, "xf": xform(t=(0, 0, 0)), "tex": 0},
             {"mesh": 0, "xf": xform(t=(0, 0, -60)), "inv": flat, "tex": 1, "box": ((52, 45, -85), (72, 155, -35))},
             {"mesh": 0, "xf": xform(t=(0, 0, 60)), "inv": tiny, "tex": 0, "box": ((40, 40, 35), (45, 160, 85))},
             {"mesh": 0, "xf": xform(t=(0, 0, 60)), "tex": 2, "refl": 0.3}]
    sc = assemble([m], insts, [texture(8, 8, 8), texture(3, 5, 9), texture(7, 2, 10)])
    return _case(sc, cam_axis(W, H), {"ordinary": (0, None), "zero_row": (1, None), "behind_tiny": (3, None)}, depth=2, slow=True, entered={"tiny": 2})


def slow_inside():
    """camera inside the root box and several boxes below it (negative entry distances)"""
    m = _slow_mesh(seed=12, bump=25.0, y=(88, 110), z=(-22, 12))
    return _case(assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}], [texture(8, 8, 11)]), cam_axis(W, H, pos=(50.0, 100.0, 0.0)),
                 {"mesh": (0, None)}, slow=True)


def slow_zero_viewplane():
    """viewplane 0 x 0: every ray is the forward ray (1, 0, 0), two zero components in every lane"""
    m = _slow_mesh(seed=13)
    cam = cam_axis(W, H)
    cam[12:14] = 0
    return _case(assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}], [texture(8, 8, 12)]), cam, {}, uniform="hit")


def slow_nan_camera():
    """forward = right = up = 0: the direction normalises to NaN in every lane; nothing can be hit"""
    m = _slow_mesh(seed=14)
    cam = cam_axis(W, H)
    cam[3:12] = 0
    return _case(assemble([m], [{"mesh": 0, "xf": xform(), "tex": 0}], [texture(8, 8, 13)]), cam, {}, uniform="miss")


# ---- TLAS shapes ----------------------------------------------------------------------------------------------------------------
_KINDS = [lambda k: rot(0, 0.4 + 0.3 * k), lambda k: np.diag([1.0, 1.3, 0.7]), lambda k: np.array([[1, 0, 0], [0, 1, 0.4], [0, 0, 1.0]]),
          lambda k: np.diag([1.0, 1.0, -1.0]), lambda k: rot(1, 0.35) @ np.diag([1.0, 0.8, 1.2]), lambda k: rot(2, -0.3) @ rot(0, 0.1 * k)]
_TEX = [(1, 1), (3, 5), (7, 2), (4, 4)]


def _tlas_case(n, shape="balanced", w=W, h=H):
    a = mesh(*shuffled(*grid_mesh(3, 3, y=(-8, 8), z=(-8, 8), x=0.0, bump=1.5, seed=20), seed=20), leaf=3)
    b = mesh(*shuffled(*grid_mesh(2, 4, y=(-7, 7), z=(-9, 9), x=0.0, bump=1.0, seed=21), seed=21), leaf=1)
    texs = [texture(tw, th, 30 + i) for i, (tw, th) in enumerate(_TEX)]
    cols = 7
    rows = (n + cols - 1) // cols
    insts = []
    for k in range(n):
        if n == 1:
            A, t = 4.0 * _KINDS[0](1), (60.0, 100.0, 0.0)
        else:
            r, c = divmod(k, cols)
            A, t = _KINDS[k % len(_KINDS)](k), (60.0 + (k % 3), 100.0 + 19.0 * (r - (rows - 1) / 2), 24.0 * (c - (cols - 1) / 2) + (12.0 if n == 2 else 0.0))
            A = 2.5 * A if n == 2 else A
        insts.append({"mesh": k % 2, "xf": xform(A, t), "tex": k % len(texs), "refl": (0.0, 0.3, 0.0, 0.6)[k % 4]})
    sc = assemble([a, b], insts, texs, tlas=shape)
    return _case(sc, cam_tilted(w, h), {"instance_%d" % k: (k, None) for k in range(n)}, w=w, h=h, depth=2)


# ---- mirrors --------------------------------------------------------------------------------------------------------------------
def _mirrors(depth, spp, light_on_hit=False):
    """two reflective walls facing each other along z (one a rotation, one a reflection of the same grid; reflectivity 1 and 0.6), a floor
    patch between them; one triangle of the first wall has zero normals: its shading normal, and the ray bounced off it, are NaN"""
    tris, ex = shuffled(*grid_mesh(6, 8, y=(40, 160), z=(-80, 80), x=250.0, bump=2.0, seed=40), seed=40)
    c = tris.reshape(-1, 3, 3).mean(1)
    zero = int(np.argmin(np.abs(c[:, 1] - 100) + np.abs(c[:, 2] + 65)))     # (object z -> world x: near the camera)
    ex[zero, 0:9] = 0
    m = mesh(tris, ex, leaf=2)
    A1, A2 = np.array([[0, 0, 1.0], [0, 1, 0], [1, 0, 0]]), np.array([[0, 0, 1.0], [0, 1, 0], [-1, 0, 0]])
    insts = [{"mesh": 0, "xf": xform(A1, (140, 0, -190)), "tex": 0, "refl": 1.0},        # wall z = +60 (reflection, det -1)
             {"mesh": 0, "xf": xform(A2, (140, 0, 190)), "tex": 1, "refl": 0.6},         # wall z = -60 (rotation)
             {"mesh": 0, "xf": xform(np.diag([1.0, 0.5, 0.4]), (20, 50, 0)), "tex": 2}]  # back wall x = 270
    sc = assemble([m], insts, [texture(8, 8, 41), texture(3, 5, 42), texture(7, 2, 43)])
    return _case(sc, cam_tilted(W, H, yaw=0.05, pitch=0.01), {"wall_a": (0, None), "wall_b": (1, None), "back": (2, None), "zero_normals": (0, {zero})},
                 depth=depth, spp=spp, light_on_hit=(70, 30) if light_on_hit else None)


# ---- conversions ----------------------------------------------------------------------------------------------------------------
CONV_W, CONV_H = 7, 4              # 0xFFFFFFFF % 7 = 3 and % 4 = 3: a saturating conversion shows in the texel column / row
# class -> (value of u * tex_width at the triangle's three corners); `v_` classes put the value on v * tex_height instead
_E = 1e-4
CONV_CLASSES = [("plain", (2.5, 2.6, 2.7)), ("negative", (-3.2, -1.4, -5.9)),
                ("at_2^31", (2.0 ** 31 * (1 - 2 * _E), 2.0 ** 31 * (1 + _E), 2.0 ** 31 * (1 + _E))),
                ("at_2^32", (2.0 ** 32 * (1 - 2 * _E), 2.0 ** 32 * (1 + _E), 2.0 ** 32 * (1 + _E))),
                ("at_2^63", (2.0 ** 63 * (1 - 2 * _E), 2.0 ** 63 * (1 + _E), 2.0 ** 63 * (1 + _E))),
                ("at_-2^63", (-2.0 ** 63 * (1 - 2 * _E), -2.0 ** 63 * (1 + _E), -2.0 ** 63 * (1 + _E))),
                ("huge", (3.0e38, 2.9e38, 2.8e38)), ("plus_inf", (np.inf,) * 3), ("minus_inf", (-np.inf,) * 3), ("nan", (np.nan,) * 3),
                ("v_negative", (-3.2, -1.4, -2.9)), ("v_at_2^63", (2.0 ** 63 * (1 - 2 * _E), 2.0 ** 63 * (1 + _E), 2.0 ** 63 * (1 + _E))),
                ("v_plus_inf", (np.inf,) * 3), ("v_nan", (np.nan,) * 3), ("v_at_2^32", (2.0 ** 32 * (1 - 2 * _E), 2.0 ** 32 * (1 + _E), 2.0 ** 32 * (1 + _E)))]
CONV_LIGHTS = {
    "plain": (0.0, 150.0, -50.0, 0, 0, 0, 1, 1, 1, 0.4, 0.35, 0.25),                              # colour = texel / 256: the pixel names the texel
    "signs": (0.0, 150.0, -50.0, 2.5, -1.0, 0.5, 0.3, 1.5, -0.2, -0.5, 2.0, 0.25),
    "below_int": (0.0, 150.0, -50.0, 1, 1, 1, -1.0e8, 0.2, -8421507.0, 0.1, -3.0e9, 0.5),          # * 255 below -2^31
    "inf": (0.0, 150.0, -50.0, np.inf, 1, -np.inf, 0.3, 0.3, 0.3, np.inf, -np.inf, 0.5),
    "nan": (0.0, 150.0, -50.0, 1, 1, 1, np.nan, 0.3, 0.3, 0.2, np.nan, 0.2),
    "nan_blue": (0.0, 150.0, -50.0, 1, 1, np.nan, 0.3, 0.3, 0.3, 0.2, 0.2, np.nan),                # the channel whose INT_MIN survives the pack
}


def conversions(light="plain"):
    """one triangle per conversion class in a 5 x 3 arrangement, each in its own screen region, all with one 7 x 4 texture of distinct
    texels; three more quads (instances 1-3) with reflectivity above 1, negative and NaN"""
    tris, ex, ids = [], [], {}
    cols = 5
    for k, (name, val) in enumerate(CONV_CLASSES):
        r, c = divmod(k, cols)
        y0, z0 = 48.0 + 24.0 * r, -80.0 + 32.0 * c
        tris.append([62, y0, z0 + 1, 62, y0 + 22, z0 + 1, 62, y0 + 2, z0 + 30])
        e = np.zeros(15)
        e[[0, 3, 6]] = -1.0
        on_v = name.startswith("v_")
        for j in range(3):
            u, v = (0.3 + 0.1 * j, val[j] / CONV_H) if on_v else (val[j] / CONV_W, 0.3 + 0.1 * j)
            e[9 + 2 * j], e[10 + 2 * j] = u, v
        ex.append(e)
        ids[name] = k
    with np.errstate(over="ignore"):
        m = mesh(np.array(tris, F), np.array(ex, F), tree=median_tree(np.array(tris, F), [3, 1, 4, 0, 5, 9, 2, 6, 8, 7, 10, 14, 12, 11, 13], 2))
    q = mesh(*shuffled(*grid_mesh(1, 2, y=(-9, 9), z=(-14, 14), x=0.0, seed=50), seed=50), leaf=2)
    tex = (np.arange(1, CONV_W * CONV_H + 1, dtype=np.uint32) * np.uint32(0x080905)) & np.uint32(0xFFFFFF)
    insts = [{"mesh": 0, "xf": xform(), "tex": 0}]
    for k, r in enumerate((1.5, -0.5, np.nan)):
        insts.append({"mesh": 1, "xf": xform(t=(62.0, 134.0, -55.0 + 55.0 * k)), "tex": 1, "refl": r})
    sc = assemble([m, q], insts, [tex.reshape(CONV_H, CONV_W), texture(3, 5, 51)])
    el = {name: (0, {m["tri_base"] + k}) for name, k in ids.items()}
    el.update({"refl_above_1": (1, None), "refl_negative": (2, None), "refl_nan": (3, None)})
    return _case(sc, cam_axis(W, H), el, light=CONV_LIGHTS[light], depth=2, conv_ids={n: m["tri_base"] + k for n, k in ids.items()})


CASES = {
    "ties": ties, "ties_instances": ties_instances,
    "leaf_sizes": leaf_sizes, "leaf_single": leaf_single,
    "boxes_exact": lambda: _boxes("exact"), "boxes_padded": lambda: _boxes("padded"), "boxes_ulp": lambda: _boxes("ulp"),
    "boxes_ten_percent": lambda: _boxes("ten_percent"), "boxes_inverted": lambda: _boxes("inverted"), "boxes_inf": lambda: _boxes("inf"),
    "boxes_huge": lambda: _boxes("huge"), "boxes_nan": lambda: _boxes("nan"),
    "slow_axis": slow_axis, "slow_on_plane": slow_on_plane, "slow_instances": slow_instances, "slow_inside": slow_inside,
    "slow_zero_viewplane": slow_zero_viewplane, "slow_nan_camera": slow_nan_camera,
    "tlas_1": lambda: _tlas_case(1), "tlas_2": lambda: _tlas_case(2), "tlas_9": lambda: _tlas_case(9), "tlas_33": lambda: _tlas_case(33),
    "tlas_chain_41": lambda: _tlas_case(41, "chain", 101, 69),
    "mirrors_d1_s1": lambda: _mirrors(1, 1), "mirrors_d2_s2": lambda: _mirrors(2, 2), "mirrors_d3_s3": lambda: _mirrors(3, 3),
    "mirrors_d4_s1": lambda: _mirrors(4, 1, light_on_hit=True), "mirrors_d5_s2": lambda: _mirrors(5, 2), "mirrors_d6_s3": lambda: _mirrors(6, 3),
    "conv_plain": lambda: conversions("plain"), "conv_signs": lambda: conversions("signs"), "conv_below_int": lambda: conversions("below_int"),
    "conv_inf": lambda: conversions("inf"), "conv_nan": lambda: conversions("nan"), "conv_nan_blue": lambda: conversions("nan_blue"),
}
NAMES = list(CASES)
_cache = {}


def case(name, po=None):
    """the built case; with the oracle module `po`, a case that wants its light on a hit point gets it there: the point the restatement
    computes (render.h:239, orig + dir * dist in float32) for the primary ray of the pixel the case names"""
    if name not in _cache:
        _cache[name] = CASES[name]()
    c = _cache[name]
    if c.get("light_on_hit") and po is not None and not c.get("light_placed"):
        x, y = c["light_on_hit"]
        a = args(po, c)
        ray = po.rc_camera_rays(a)[y * c["w"] + x]
        hit = po.rc_trace(a, ray[None])[0]
        assert hit["dist"] < 1e29
        c["light"] = tuple(float(v) for v in (ray[0:3] + ray[3:6] * F(hit["dist"]))) + c["light"][3:]
        c["light_placed"] = True
    return c


def args(po, c, w=None, h=None, **over):
    return po.rc_args(c["scene"], w or c["w"], h or c["h"], over.get("cam", c["cam"]), over.get("light", c["light"]), over.get("spp", c["spp"]),
                      over.get("depth", c["depth"]))
