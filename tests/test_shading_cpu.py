"""CPU: the shading fuzz's inputs (tests/shading_cases.py) through the oracle alone -- that every family reaches the branches it
was written for, that the oracle equals the reference's own helpers on them, that an independent numpy restatement equals the
oracle bit for bit, and what the conversions C leaves undefined return (the rule of include/vortex_hip.h, vxrt_shade_rays)."""
import zlib

import numpy as np
import pytest

import shading_cases as sc
import shading_ref

COLOR_RTOL = 1e-5        # the project's colour tolerance (tests/test_gpu_parity.py)
f32 = np.float32


def _all_param_sets(vrt, po, seed, family):
    b, plist, extra = sc.case(vrt, po, seed, family)
    rays, hits = sc.per_ray_inputs(po, b, seed, family, extra)
    return b, plist, rays, hits


def _same_colours(a, b):
    """bit-equal where neither is NaN, NaN in the same places"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_benign_family_reaches_its_branches(vrt, po, seed):
    b, plist, rays, hits = _all_param_sets(vrt, po, seed, "benign")
    col, px, info = shading_ref.shade(b, rays, hits, plist[0])
    n_mats = len(b["mat"]) // 88
    mats = np.frombuffer(b["mat"].tobytes(), sc.MAT_DT)
    n_textured, n_plain = int(info["textured"].sum()), int((~info["textured"]).sum())
    assert n_textured >= 20 and n_plain >= 20, (n_textured, n_plain)
    per_mat = np.bincount(info["material"], minlength=n_mats)
    assert (per_mat > 0).all(), per_mat                                          # every material, so every texture, sampled
    assert int((mats["tex_id"] >= 0).sum()) == n_mats // 2 and n_mats >= 2
    n_clamped, n_lit = int((info["ndl_raw"] <= 0).sum()), int((info["ndl_raw"] > 0).sum())
    assert n_clamped >= 20 and n_lit >= 20, (n_clamped, n_lit)
    assert 0 <= info["u"].min() and info["u"].max() < 1 and 0 <= info["v"].min() and info["v"].max() < 1
    # texels that differ: at least half as many distinct texels read as textured hits of the larger textures allow
    big = info["textured"] & (info["tw"].astype(np.int64) * info["th"] >= 256)
    if big.any():
        assert len(np.unique(info["texel_index"][big])) >= min(int(big.sum()), 256) // 4
    refl = np.frombuffer(b["blas"].tobytes(), np.float32).reshape(-1, 40)[:, 38]
    assert ((refl > 0) & (refl < 1)).any()
    # rotations x non-uniform scales: the inverse's 3 x 3 block is neither symmetric nor diagonal
    m = np.frombuffer(b["blas"].tobytes(), np.float32).reshape(-1, 40)[:, 1:17].reshape(-1, 4, 4)[:, :3, :3]
    assert (np.abs(m - m.transpose(0, 2, 1)).max((1, 2)) > 1e-4).all()


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_hostile_family_reaches_its_branches(vrt, po, seed):
    b, plist, rays, hits = _all_param_sets(vrt, po, seed, "hostile")
    n_mats = len(b["mat"]) // 88
    infos, cols = [], []
    for p in plist:
        col, px, info = shading_ref.shade(b, rays, hits, p)
        infos.append(info)
        cols.append(col[info["found"]])
    i0 = infos[0]
    n_textured, n_plain = int(i0["textured"].sum()), int((~i0["textured"]).sum())
    assert n_textured >= 20 and n_plain >= 20, (n_textured, n_plain)
    assert (np.bincount(i0["material"], minlength=n_mats) > 0).all()             # every texture sampled
    t = i0["textured"]
    n_neg = int((t & ((i0["u"] < 0) | (i0["v"] < 0))).sum())
    n_above = int((t & ((i0["uw"] > 2 * i0["tw"].astype(np.float32)) | (i0["vh"] > 2 * i0["th"].astype(np.float32)))).sum())
    n_huge = int((t & ((np.abs(i0["uw"]) > 2.0 ** 24) | (np.abs(i0["vh"]) > 2.0 ** 24))).sum())
    n_1x1 = int((t & (i0["tw"] == 1) & (i0["th"] == 1)).sum())
    n_boundary = int((t & ((i0["uw"] == np.trunc(i0["uw"])) | (i0["vh"] == np.trunc(i0["vh"])))).sum())
    assert n_neg >= 5 and n_above >= 5 and n_huge >= 1 and n_1x1 >= 1 and n_boundary >= 5, (n_neg, n_above, n_huge, n_1x1, n_boundary)
    assert max(np.abs(i0["uw"][t]).max(), np.abs(i0["vh"][t]).max()) < 2.0 ** 32      # inside what C defines
    n_clamped, n_lit = int((i0["ndl_raw"] <= 0).sum()), int((i0["ndl_raw"] > 0).sum())
    assert n_clamped >= 20 and n_lit >= 20, (n_clamped, n_lit)
    n_zero_normal = int((i0["tlen"] == 0).sum())
    assert n_zero_normal >= 1, n_zero_normal                                     # the cancelling pairs and the zero normals
    n_tiny, n_long = int(((i0["tlen"] > 0) & (i0["tlen"] < 1e-15)).sum()), int((i0["tlen"] > 1e10).sum())
    assert n_tiny >= 1 and n_long >= 1, (n_tiny, n_long)
    n_on_light = int((infos[0]["light_dist"] == 0).sum())
    assert n_on_light >= 1, n_on_light                                            # the light ON a hit point
    assert int((infos[2]["light_dist"] > 9e5).sum()) == len(infos[2]["light_dist"])
    assert float(infos[3]["light_dist"].min()) < 1e-3
    allc = np.concatenate(cols)
    n_above_1, n_below_0 = int((allc > 1).sum()), int((allc < 0).sum())
    assert n_above_1 >= 20 and n_below_0 >= 20, (n_above_1, n_below_0)
    assert np.isfinite(allc).all()                                                # finite inputs, finite colours
    mats = np.frombuffer(b["mat"].tobytes(), sc.MAT_DT)
    garbage = (mats["tex_id"] < 0) & (mats["tw"] == 0xFFFFFFFF)
    assert garbage.sum() == 1 and int((i0["material"] == np.nonzero(garbage)[0][0]).sum()) >= 1
    depths = {p.max_depth for p in plist}
    assert min(depths) == 1 and max(depths) == 4


@pytest.mark.parametrize("family", ["benign", "hostile"])
@pytest.mark.parametrize("seed", sc.SEEDS)
def test_restatement_equals_the_oracle_bit_for_bit(vrt, po, seed, family):
    b, plist, rays, hits = _all_param_sets(vrt, po, seed, family)
    for k, p in enumerate(plist):
        col, px, _ = shading_ref.shade(b, rays, hits, p)
        ocol, opx = po.shade(b, rays, hits, p)
        assert _same_colours(col, ocol), "colours, parameter set %d" % k
        assert np.array_equal(px, opx), "rgb8, parameter set %d" % k


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("seed", sc.SEEDS)
def test_oracle_equals_the_reference_helpers(vrt, po, seed, family):
    """every hit and every miss of the case, through the reference's texSample / diffuseLighting / RGB32FtoRGB8 as compiled from
    where they lie: RGB8 equal, colours within COLOR_RTOL, NaN in the same places.  None excluded (for the outside_c family
    this is the x86-64 lowering itself, which the written rule restates)."""
    if not po.have_ref():
        pytest.skip("oracle/_ref/libvxref.so is not built (it needs the reference tree)")
    b, plist, rays, hits = _all_param_sets(vrt, po, seed, family)
    for k, p in enumerate(plist):
        ocol, opx = po.shade(b, rays, hits, p)
        rcol, rpx = po.ref_shade(b, rays, hits, p)
        assert np.array_equal(np.isnan(ocol), np.isnan(rcol)), "NaN positions, parameter set %d" % k
        np.testing.assert_allclose(ocol, rcol, rtol=COLOR_RTOL, atol=0, err_msg="parameter set %d" % k)
        np.testing.assert_array_equal(opx, rpx, err_msg="parameter set %d" % k)


# ---- outside C: decided, then pinned -----------------------------------------------------------------------------------------
# The rule (include/vortex_hip.h, vxrt_shade_rays): what x86-64 g++ makes of the reference's casts.
#   uint32_t(f) -> the truncated value mod 2^32 for -2^63 <= f < 2^63, 0 otherwise (NaN included)
#   int(f)      -> the truncated value for -2^31 <= f < 2^31, INT_MIN otherwise (NaN included)
nan, inf = float("nan"), float("inf")
PACK_PINS = [
    ((nan, nan, nan), 0x80000000),                 # (INT_MIN << 16) + (INT_MIN << 8) + INT_MIN in 32-bit registers
    ((0.5, nan, 0.5), 0x007F007F),                 # INT_MIN << 8 = 0
    ((0.5, 0.5, nan), 0x807F7F00),
    ((-inf, 0.25, 2.0), 0x00003FFF),
    ((0.0, 0.0, -inf), 0x80000000),
    ((inf, inf, inf), 0x00FFFFFF),                 # min(inf, 1) = 1
    ((0.0, 0.0, -8421504.0), 0x80000080),          # -8421504 * 255 = -2^31 + 128: in range
    ((0.0, 0.0, -8421505.0), 0x80000000),          # -2147483775 rounds to -2^31: in range, INT_MIN by value
    ((0.0, 0.0, -8421507.0), 0x80000000),          # rounds to -2^31 - 512: out of range, INT_MIN by the rule
    ((0.0, 0.0, -1.0e10), 0x80000000),
    ((0.0, 0.0, -1.0), 0xFFFFFF01),                # in range: -255
    ((-1.0, -1.0, -1.0), 0xFF000001),
    ((1.0, 1.0 - 2.0 ** -24, 0.0), 0x00FFFE00),    # 1 - 1ulp packs to 254
]
# value of u * w -> texel column of a 32-texel row (f2u_x86(x) % 32; a power of two so that u = x / 32 and u * 32 = x are exact)
F2U_PINS = [(2.0 ** 63, 0), (2.0 ** 64, 0), (3.0e38, 0), (inf, 0), (-inf, 0), (nan, 0), (-3.0e38, 0), (-1.0e19, 0),
            (-2.0 ** 63, 0),                        # in range: the low half of 0x8000000000000000
            (2.0 ** 62, 0), (2.0 ** 24 + 6.0, 6), (2.0 ** 31 + 256.0 * 3 + 0.0, 0), (-1.0, 31), (-3.0, 29), (-(2.0 ** 25 + 4.0), 28),
            (-0.0, 0), (31.999998, 31), (32.0, 0), (37.5, 5), (-0.75, 0), (7.0, 7), (19.99, 19)]
# crc32 of the oracle's RGB8 over (per-ray inputs x parameter sets) of every outside_c seed: what x86 returned when this was written
OUTSIDE_C_CRC = {0: 0xA6C764D2, 1: 0xC992EB5A, 2: 0xD5CE13FA, 3: 0x862A38E6, 4: 0x9237E0B4, 5: 0xF3A661F9}


def test_pack_conversion_rule_is_pinned(po):
    for colour, want in PACK_PINS:
        c = np.array(colour, np.float32)
        got = int(po.orc().orc_pack_rgb8(c.ctypes.data))
        assert got == want, (colour, hex(got), hex(want))
        assert int(shading_ref.pack_rgb8(c[None])[0]) == want, colour


def _probe_scene(vrt, po):
    """one triangle per F2U_PINS entry in front of the camera, all with one 32 x 3 texture of distinct texels; u = value / 32 at
    every corner, v = 0"""
    n = len(F2U_PINS)
    tris = np.zeros((n, 9), np.float32)
    for i in range(n):
        y = 60.0 + 5.0 * i
        tris[i] = [300.0, y, -20.0, 300.0, y + 4.0, -20.0, 300.0, y, 20.0]
    s = vrt.scene.from_triangles([tris])
    b = {k: np.frombuffer(bytes(s.buffers[k]), np.uint8).copy() for k in sc.KEYS}
    order = np.frombuffer(b["tri"].tobytes(), np.float32).reshape(n, 9)[:, 1]          # the builder may reorder: find each by its y
    which = np.round((order - 60.0) / 5.0).astype(int)
    ex = np.zeros((n, 16), np.float32)
    ex[:, 0] = ex[:, 3] = ex[:, 6] = -1.0
    mat = np.zeros(1, sc.MAT_DT)
    mat["tex_id"], mat["tw"], mat["th"], mat["off"] = 0, 32, 3, 0
    b["mat"] = mat.view(np.uint8).reshape(-1).copy()
    b["tex"] = (np.arange(32 * 3, dtype=np.uint32) * np.uint32(0x010305) & np.uint32(0xFFFFFF)).view(np.uint8).copy()
    rays = np.zeros((n, 6), np.float32)
    hits = np.zeros(n, po.HIT_DTYPE)
    for slot, i in enumerate(which):
        ex[slot, 9] = ex[slot, 11] = ex[slot, 13] = f32(F2U_PINS[i][0]) / f32(32.0)
        rays[i] = [0, 100, 0, 1, 0, 0]
        hits[i] = (300.0, 0.25, 0.25, 0.5, 0, slot)
    b["triEx"] = ex.view(np.uint8).reshape(-1).copy()
    return b, rays, hits


def probe_case(vrt, po):
    """(buffers, rays, hit records, parameters, expected rgb8) of the pinned uv conversions: ambient 1, no light, so that the colour
    is the texel's"""
    b, rays, hits = _probe_scene(vrt, po)
    p = po.shade_params(ambient=(1, 1, 1), light_color=(0, 0, 0), light_pos=(0, 500, 0), background=(0, 0, 0))
    tex = np.frombuffer(b["tex"].tobytes(), np.uint32)
    want = np.zeros(len(F2U_PINS), np.uint32)
    for i, (x, column) in enumerate(F2U_PINS):
        t = int(tex[column])
        ch = [int(f32(f32((t >> s) & 255) * f32(1 / 256.0)) * f32(255)) for s in (16, 8, 0)]
        want[i] = (ch[0] << 16) + (ch[1] << 8) + ch[2]
    return b, rays, hits, p, want


def test_uv_conversion_rule_is_pinned(vrt, po):
    b, rays, hits, p, want = probe_case(vrt, po)
    _, info_px, info = shading_ref.shade(b, rays, hits, p)
    xs = np.array([x for x, _ in F2U_PINS], np.float32)
    ok = ~np.isnan(xs)
    assert np.array_equal(info["uw"][ok], xs[ok]) and np.isnan(info["uw"][~ok]).all()   # the probe really presents the pinned values
    assert [int(v) for v in info["texel_index"]] == [c for _, c in F2U_PINS]
    _, px = po.shade(b, rays, hits, p)
    np.testing.assert_array_equal(px, want)
    np.testing.assert_array_equal(info_px, want)
    assert len(np.unique(want)) >= 6                                                     # the columns are told apart
    if po.have_ref():
        _, rpx = po.ref_shade(b, rays, hits, p)
        np.testing.assert_array_equal(rpx, want)


def outside_c_crc(po, b, plist, rays, hits):
    crc = 0
    for p in plist:
        _, px = po.shade(b, rays, hits, p)
        crc = zlib.crc32(np.ascontiguousarray(px).tobytes(), crc)
    return crc


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_outside_c_family_is_pinned(vrt, po, seed):
    """the family reaches the conversions the rule is about, the restatement (written from the rule) equals the oracle on every
    ray, and the oracle's RGB8 is the recorded x86 result"""
    b, plist, rays, hits = _all_param_sets(vrt, po, seed, "outside_c")
    n_big = n_nan_uv = n_nan_col = n_below = 0
    for k, p in enumerate(plist):
        col, px, info = shading_ref.shade(b, rays, hits, p)
        ocol, opx = po.shade(b, rays, hits, p)
        assert _same_colours(col, ocol), "colours, parameter set %d" % k
        assert np.array_equal(px, opx), "rgb8, parameter set %d" % k
        t = info["textured"]
        with np.errstate(all="ignore"):
            n_big += int((t & ((np.abs(info["uw"]) >= 2.0 ** 63) | (np.abs(info["vh"]) >= 2.0 ** 63))).sum())
            n_nan_uv += int((t & (np.isnan(info["uw"]) | np.isnan(info["vh"]))).sum())
            n_nan_col += int(np.isnan(col).sum())
            n_below += int((col * f32(255) < -2.0 ** 31).sum())
    assert n_big >= 20 and n_nan_uv >= 20 and n_nan_col >= 20 and n_below >= 20, (n_big, n_nan_uv, n_nan_col, n_below)
    assert outside_c_crc(po, b, plist, rays, hits) == OUTSIDE_C_CRC[seed]
