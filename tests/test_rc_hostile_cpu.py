"""The hand-built twin scenes of tests/rc_cases.py are what they claim to be -- every element a case exists for is on screen, the frames are
neither empty nor flat -- and the restatement oracle/rc_oracle.c renders them as the reference's own object code does (where
oracle/_ref/libvxref_rc.so is built).  That comparison decides the two conversions C leaves undefined; the rule is pinned below."""
import numpy as np
import pytest

import rc_cases as rcc

F = np.float32


@pytest.fixture(scope="module")
def frames(po):
    """name -> (case, pixels, colours, primary rays, their hits): rendered once, shared, left unchanged"""
    memo = {}

    def get(name):
        if name not in memo:
            c = rcc.case(name, po)
            a = rcc.args(po, c)
            px, col = po.rc_render(a)
            rays = po.rc_camera_rays(a)
            memo[name] = (c, px, col, rays, po.rc_trace(a, rays))
        return memo[name]
    return get


def _ray_box(rays, lo, hi):
    """geometry.h:1442-1465 over many rays (the libstdc++ min / max chains, in float32)"""
    with np.errstate(all="ignore"):
        o, inv = rays[:, 0:3], F(1) / rays[:, 3:6]
        smin = lambda a, b: np.where(b < a, b, a)
        smax = lambda a, b: np.where(a < b, b, a)
        t1, t2 = (lo - o) * inv, (hi - o) * inv
        tmin, tmax = smin(t1[:, 0], t2[:, 0]), smax(t1[:, 0], t2[:, 0])
        for k in (1, 2):
            tmin, tmax = smax(tmin, smin(t1[:, k], t2[:, k])), smin(tmax, smax(t1[:, k], t2[:, k]))
        return ~((tmax < tmin) | (tmax <= 0))


@pytest.mark.parametrize("name", rcc.NAMES)
def test_case_is_what_it_claims(po, frames, name):
    c, px, col, rays, hits = frames(name)
    hit = hits["dist"] < 1e29
    if c.get("uniform"):
        # every ray of these two cases is the same ray by construction (zero viewplane; a camera basis that normalises to NaN): the frame
        # is one value, and the shares below cannot apply -- the ray must be the hostile one and do what the case says
        assert len(np.unique(px)) == 1 and (rays.view(np.uint32) == rays.view(np.uint32)[0]).all()
        with np.errstate(all="ignore"):
            assert (~np.isfinite(F(1) / rays[0, 3:6])).sum() >= 2
        assert hit.all() if c["uniform"] == "hit" else not hit.any()
        return
    for label, (blas, ids) in c["elements"].items():
        m = hit.copy()
        if blas is not None:
            m &= hits["blasIdx"] == blas
        if ids is not None:
            m &= np.isin(hits["triIdx"], sorted(ids))
        assert m.sum() >= 20, (label, int(m.sum()))
    for label, blas in c.get("entered", {}).items():
        # an instance no ray can hit (its triangle tests fall below the reference's epsilon): what counts is the rays that walk its tree
        tl = c["scene"]["tlas"].view(np.uint32).reshape(-1, 8)
        leaf = int(np.nonzero((tl[:, 3] == 0) & (tl[:, 7] == blas))[0][-1])
        n = int(_ray_box(rays, tl.view(F)[leaf, 0:3], tl.view(F)[leaf, 4:7]).sum())
        assert n >= 20, (label, n)
    assert 0.02 <= hit.mean() <= 0.98, hit.mean()
    assert len(np.unique(px)) >= 4
    if c.get("slow"):
        with np.errstate(all="ignore"):
            inv = F(1) / rays[:, 3:6]
        n = int(((inv == 0) | ~np.isfinite(inv)).any(1).sum())
        assert 0 < n < len(rays) / 2, n


@pytest.mark.parametrize("name", [n for n in rcc.NAMES if n.startswith("ties")])
def test_ties_show_which_copy_won(po, frames, name):
    """with the copies' normal sets exchanged the same triangles are hit at the same distances, and the pixels change: the copy that wins
    a tie is visible"""
    c, px, _, rays, hits = frames(name)
    s = rcc.CASES[name](swap=True)
    a = rcc.args(po, s)
    px2, _ = po.rc_render(a)
    h2 = po.rc_trace(a, rays)
    assert np.array_equal(hits.view(np.uint8), h2.view(np.uint8))
    assert (px2 != px).mean() > 0.2
    # ... and the ties are real: the winner's two bit-identical copies are in the mesh
    tri = c["scene"]["tri"].view(np.uint32).reshape(-1, 9)
    w = hits["triIdx"][hits["dist"] < 1e29][::37]
    assert all((tri == tri[t]).all(1).sum() == 3 for t in w)


def test_leaf_sizes_and_node_shapes_are_in_the_tree(po):
    c = rcc.case("leaf_sizes", po)
    bvh = c["scene"]["bvh"].view(np.uint32).reshape(-1, 8)
    assert sorted(bvh[bvh[:, 7] != 0, 7].tolist()) == list(rcc.LEAF_SIZES)
    shapes = set()
    for i in np.nonzero((bvh[:, 7] == 0) & (np.arange(len(bvh)) != 1))[0]:
        l = int(bvh[i, 3])
        shapes.add((bool(bvh[l, 7] == 0), bool(bvh[l + 1, 7] == 0)))
    assert shapes == {(True, True), (True, False), (False, True), (False, False)}
    s = rcc.case("leaf_single", po)["scene"]
    bv, bl = s["bvh"].view(np.uint32).reshape(-1, 8), s["blas"].view(np.uint32).reshape(-1, 40)
    assert [int(bv[int(bl[j, 32]), 7]) for j in range(2)] == [6, 36]


def test_tlas_chain_is_forty_levels_deep(po):
    s = rcc.case("tlas_chain_41", po)["scene"]
    tl = s["tlas"].view(np.uint32).reshape(-1, 8)

    def depth(i):
        lr = int(tl[i, 3])
        return 0 if lr == 0 else 1 + max(depth(lr & 0xFFFF), depth(lr >> 16))
    assert depth(s["tlas_root"]) == 40


@pytest.mark.parametrize("name", rcc.NAMES)
def test_restatement_equals_reference_object_code_on_hostile_scenes(po, frames, name):
    """every case through the reference's own render loop, compiled where it lies: equal pixels.  No case is left out: none makes the
    reference's walk read outside its buffers."""
    if not po.have_ref_rc():
        pytest.skip("oracle/_ref/libvxref_rc.so is not built here")
    c, px, _, _, _ = frames(name)
    live, _ = po.ref_rc_render_buffers(c["scene"], c["w"], c["h"], 0, c["h"], c["cam"], c["light"], spp=c["spp"], max_depth=c["depth"])
    bad = np.argwhere(live != px)
    assert len(bad) == 0, "%d pixels differ, first (y, x) = %s: reference %08x, restatement %08x" % (
        len(bad), tuple(bad[0]), live[tuple(bad[0])], px[tuple(bad[0])])


# ---- the conversions C leaves undefined: decided by the reference's x86-64 object code (the test above), then pinned -----------------
# The rule is the RTU path's (include/vortex_hip.h, vxrt_shade_rays) -- the live reference agrees with it for every class:
#   uint32_t(f) -> the truncated value mod 2^32 for -2^63 <= f < 2^63, 0 otherwise (NaN included)
#   int(f)      -> the truncated value for -2^31 <= f < 2^31, INT_MIN otherwise (NaN included)
nan, inf = float("nan"), float("inf")
# value of u * 7 (v * 4) -> texel column of the 7-texel row (row of the 4 rows)
RC_F2U_PINS = [(2.5, 2, 2), (-1.0, 0xFFFFFFFF % 7, 3), (-3.7, 0xFFFFFFFD % 7, 1), (-0.75, 0, 0), (2.0 ** 31 - 128.0, (2 ** 31 - 128) % 7, 0),
               (2.0 ** 31, 2 ** 31 % 7, 0), (2.0 ** 32 - 256.0, (2 ** 32 - 256) % 7, 0), (2.0 ** 32, 0, 0), (2.0 ** 32 + 512.0, 512 % 7, 0),
               (2.0 ** 63 - 2.0 ** 39, (2 ** 32 - 2 ** 39 % 2 ** 32) % 2 ** 32 % 7, 0), (2.0 ** 63, 0, 0), (-2.0 ** 63, 0, 0), (-2.0 ** 63 - 2.0 ** 40, 0, 0),
               (3.0e38, 0, 0), (inf, 0, 0), (-inf, 0, 0), (nan, 0, 0)]
# summed colour -> packed pixel (kernel.cpp:27 / common.h:104-112)
RC_PACK_PINS = [((nan, nan, nan), 0x80000000), ((0.5, nan, 0.5), 0x007F007F), ((0.5, 0.5, nan), 0x807F7F00), ((-inf, 0.25, 2.0), 0x00003FFF),
                ((inf, inf, inf), 0x00FFFFFF), ((0.0, 0.0, -8421504.0), 0x80000080), ((0.0, 0.0, -8421507.0), 0x80000000),
                ((0.0, 0.0, -1.0e10), 0x80000000), ((0.0, 0.0, -1.0), 0xFFFFFF01), ((-1.0, -1.0, -1.0), 0xFF000001), ((1.0, 1.0 - 2.0 ** -24, 0.0), 0x00FFFE00)]


def _probe(po, uw, vh, light):
    """one pixel looking at one triangle whose uv give u * 7 = uw and v * 4 = vh at the hit; ambient 1, no light: colour = texel / 256"""
    tris = np.array([[250, 0, -200, 250, 300, 0, 250, 0, 200]], F)
    ex = np.zeros((1, 15), F)
    ex[0, [0, 3, 6]] = -1
    with np.errstate(all="ignore"):
        ex[0, 9::2], ex[0, 10::2] = F(uw) / F(7), F(vh) / F(4)
    pad = np.array([[251, 0, 0, 251, 1, 0, 251, 0, 1]], F)                       # (a second triangle: triIdx is no identity)
    m = rcc.mesh(np.concatenate([pad, tris]), np.concatenate([ex, ex]), tree=[1, 0])
    tex = (np.arange(1, 29, dtype=np.uint32) * np.uint32(0x080905)).reshape(4, 7)
    sc = rcc.assemble([m], [{"mesh": 0, "xf": rcc.xform(), "tex": 0}], [tex])
    cam = rcc.cam_axis(1, 1)
    px, col = po.rc_render(po.rc_args(sc, 1, 1, cam, light, 1, 1))
    return sc, cam, int(px[0, 0]), col[0, 0]


def test_twin_conversion_rule_is_pinned(po):
    plain = (0.0, 150.0, -50.0, 0, 0, 0, 1, 1, 1, 0.4, 0.35, 0.25)
    texel = lambda col, row: (1 + col + 7 * row) * 0x080905
    pack = lambda t: ((t >> 16 & 255) * 255 // 256 << 16) + ((t >> 8 & 255) * 255 // 256 << 8) + ((t & 255) * 255 // 256)
    for value, col_want, row_want in RC_F2U_PINS:
        # uv = value / size is exact for the powers of two and their neighbours only through the product: find the column from the product
        sc, cam, got, _ = _probe(po, value, 1.5, plain)
        with np.errstate(all="ignore"):
            prod = F(F(value) / F(7)) * F(7)
        if prod == F(value) or value != value:
            assert got == pack(texel(col_want, 1)), (value, hex(got))
        sc, cam, got, _ = _probe(po, 2.5, value, plain)
        assert got == pack(texel(2, row_want)), (value, hex(got))                 # (v = value / 4 and v * 4 are exact)
        if po.have_ref_rc():
            live, _ = po.ref_rc_render_buffers(sc, 1, 1, 0, 1, cam, plain)
            assert int(live[0, 0]) == got, (value, hex(int(live[0, 0])), hex(got))
    # the pack: background = the colour, the ray looks away from the triangle
    for colour, want in RC_PACK_PINS:
        light = (0.0, 150.0, -50.0, 0, 0, 0, 1, 1, 1) + tuple(colour)
        sc, cam, _, _ = _probe(po, 2.5, 1.5, plain)
        cam[3] = -1.0
        px, col = po.rc_render(po.rc_args(sc, 1, 1, cam, light, 1, 1))
        assert int(px[0, 0]) == want, (colour, hex(int(px[0, 0])), hex(want))
        if po.have_ref_rc():
            live, _ = po.ref_rc_render_buffers(sc, 1, 1, 0, 1, cam, light)
            assert int(live[0, 0]) == want, (colour, hex(int(live[0, 0])), hex(want))


def test_conversion_classes_are_on_screen(po, frames):
    """the triangles of conv_* carry what their names say: u * w (v * h) as the restatement computes it from the hit's barycentrics
    (render.h:247) falls into the class, on both sides of a threshold where the class straddles one"""
    c, _, _, _, hits = frames("conv_plain")
    exs = c["scene"]["triEx"].view(F).reshape(-1, 15)
    with np.errstate(all="ignore"):
        for name, tid in c["conv_ids"].items():
            h = hits[(hits["dist"] < 1e29) & (hits["triIdx"] == tid) & (hits["blasIdx"] == 0)]
            k = 10 if name.startswith("v_") else 9
            e = exs[tid]
            x = (e[k + 2] * h["bx"] + e[k + 4] * h["by"] + e[k] * h["bz"]) * F(rcc.CONV_H if k == 10 else rcc.CONV_W)
            key = name[2:] if name.startswith("v_") else name
            if key.startswith("at_"):
                t = float(eval(key[3:].replace("^", "**")))
                lo_, hi_ = (np.abs(x) < abs(t)).sum(), (np.abs(x) >= abs(t)).sum()
                assert lo_ >= 20 and hi_ >= 20 and (np.abs(x / F(t) - 1) < 1e-3).all() and (np.sign(x) == np.sign(t)).all(), (name, lo_, hi_)
            else:
                ok = {"plain": (x > 0) & (x < 7), "negative": x < -1, "huge": (x > 2.0 ** 64) & np.isfinite(x), "plus_inf": x == np.inf,
                      "minus_inf": x == -np.inf, "nan": x != x}[key]
                assert ok.sum() >= 20, (name, int(ok.sum()))
