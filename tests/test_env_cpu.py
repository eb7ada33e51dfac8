"""CPU: the restatement of the environment light (tests/env_ref.py) alone -- that its density integrates to one over the sphere, that a
sampled direction looks up the texel it was sampled from, that the two estimators of the frame agree and that sampling the map lowers
the variance it is for -- and that the cases of tests/test_gpu_env.py (tests/env_cases.py) are not vacuous."""
import numpy as np
import pytest

import env_cases as vc
import env_ref as ev
import path_ref as pr

f32 = np.float32


def _uv_grid(n, k):
    """midpoints of a (n k) x (n k) grid over the texel square, k x k per texel, in double: no cell is crossed by a texel border or by
    the fold.  u, v, the texel each point lies in, the unit direction it unfolds to and its solid angle du dv / r^3"""
    m = n * k
    c = (np.arange(m) + 0.5) * 2.0 / m - 1.0
    v, u = (a.reshape(-1) for a in np.meshgrid(c, c, indexing="ij"))
    y = 1.0 - np.abs(u) - np.abs(v)
    fold = y < 0
    x = np.where(fold, (1.0 - np.abs(v)) * np.where(u >= 0, 1.0, -1.0), u)
    z = np.where(fold, (1.0 - np.abs(u)) * np.where(v >= 0, 1.0, -1.0), v)
    r = np.sqrt(x * x + y * y + z * z)
    i, j = np.arange(m) // k, np.arange(m) // k
    e = (np.tile(i, m) + np.repeat(j, m) * n).astype(np.uint32)
    return e, np.stack([x, y, z], 1) / r[:, None], (2.0 / m) ** 2 / r ** 3


def test_density_integrates_to_one():
    """The sum of pe(w) dw over the sphere is 1 -- pe integrates to 4 pi x 1 / (4 pi) -- for a constant, an HDR and a one-texel-sun
    map, n = 16, on a grid of 16 x 16 midpoints per texel of the unfolding (65,536 directions), dw = du dv / r^3 in double.

    The grid.  No cell is crossed by a texel border or by the fold, so inside every cell pe(w) dw is smooth -- by the definition it is
    constant, qf_e * nn4 * du dv -- and the sum has no border error at all.  That dw is the solid angle of a cell is checked apart: the
    sum of du dv / r^3 over 4 pi is 1 up to the midpoint error of the grid, measured here 3.0e-11 at 256 x 256 and 1.9e-12 at 512 x 512
    (a factor 16: the integrand is smooth inside every cell); it must at least halve from one grid to the next and stay below the
    tolerance's format part, or the sums below would measure the grid.

    Tolerance.  As the issue has it, the grid's own error on the CONSTANT map, measured in the test (here 9.5e-9: what is left is fp32
    rounding of the lookup), plus the precision of the format: pe(w) is eleven fp32 operations from the direction (three divisions, the
    sums of s and r2, sqrtf, r2 * r, qf, two multiplications), each within 2^-24 relative, and a sum of terms each within 16 x 2^-24 is
    within 16 x 2^-24 = 9.5e-7.  The constant map's own error is held to that format part ABSOLUTELY -- on this grid it has no other
    source, and without that bound an error common to all maps (a wrong nn4, a factor on the density) would only widen the tolerance
    it broke -- and then |sum - 1| <= err_const + 16 x 2^-24 for every other map, at most 2 x 9.5e-7.  A lookup that takes a direction
    to a neighbouring texel fails the texel assertion; a density or an r^3 off by 2e-6 everywhere fails the sums (the last lines of
    the test apply such factors to the restatement's density and see the assertion's condition fail)."""
    areas = {}
    for k in (16, 32):
        _, _, dw = _uv_grid(16, k)
        areas[k] = abs(float(dw.sum()) / (4.0 * np.pi) - 1.0)
    print("solid angle of the square / 4 pi - 1: %.3g at 256 x 256, %.3g at 512 x 512" % (areas[16], areas[32]))
    fmt = 16.0 * 2.0 ** -24
    assert areas[16] < fmt and areas[32] <= 0.5 * areas[16]
    e, d, dw = _uv_grid(16, 16)

    def total(texels):
        m = ev.make_map(texels)
        _, got, pe = ev.lookup(m, 1.0, d)
        np.testing.assert_array_equal(got, e)                                         # (every midpoint looks up the texel it lies in)
        return float((pe.astype(np.float64) * dw).sum())
    err_const = abs(total(vc.constant(16)) - 1.0)
    print("constant map: error %.3g; format part %.3g" % (err_const, fmt))
    assert err_const <= fmt, err_const
    for name, texels in (("hdr", vc.hdr(16)), ("sun", vc.sun(16)), ("negzero", vc.negzero(16))):
        s = total(texels)
        print("%s: sum %.9f, error %.3g" % (name, s, abs(s - 1.0)))
        assert abs(s - 1.0) <= err_const + fmt, (name, s, err_const)
    # the bound bites: the same sums with the restatement's density off by a factor, common to all maps, miss it
    honest = ev.density
    try:
        for factor in (2.0, 1.01, 1.0 + 2e-6, 1.0 - 2e-6):
            ev.density = lambda m, e, r3, f=factor: (honest(m, e, r3).astype(np.float64) * f).astype(np.float32)
            assert abs(total(vc.constant(16)) - 1.0) > fmt, factor
    finally:
        ev.density = honest


@pytest.mark.parametrize("n", vc.SIZES)
def test_round_trip_every_texel(n):
    """the lookup of a direction sampled from texel e with jitters in [1/8, 7/8] returns e, for EVERY texel: the direction -> uv map of
    TEXEL OF A DIRECTION inverts the unfolding of THE ENVIRONMENT RAY (to 2e-16 in double; fp32 moves uv by far less than 1 / (8 n))"""
    e = np.arange(n * n, dtype=np.uint32)
    i, j = (e % n).astype(np.float32), (e // n).astype(np.float32)
    for a in (0.125, 0.5, 0.875):
        for b in (0.125, 0.5, 0.875):
            u = ((i + f32(a)) / f32(n)) * f32(2.0) - f32(1.0)
            v = ((j + f32(b)) / f32(n)) * f32(2.0) - f32(1.0)
            P, r2 = ev.unfold(u, v)
            r = np.sqrt(r2)
            w = np.stack([P[k] / r for k in range(3)], 1)
            got, r3 = ev.texel_of(n, w)
            np.testing.assert_array_equal(got, e, err_msg="n %d, jitter (%g, %g)" % (n, a, b))
            assert np.abs(np.linalg.norm(w.astype(np.float64), axis=1) - 1.0).max() < 1e-6
            # r2 * r of the lookup is that of the sample up to rounding: the two densities of one direction agree
            np.testing.assert_allclose(r3, r2 * r, rtol=2e-6)


def test_round_trip_in_double():
    rng = np.random.default_rng(1)
    u, v = rng.uniform(-1, 1, 100000), rng.uniform(-1, 1, 100000)
    c = 1 - np.abs(u) - np.abs(v)
    fold = c < 0
    uf = np.where(fold, (1 - np.abs(v)) * np.where(u >= 0, 1.0, -1.0), u)
    vf = np.where(fold, (1 - np.abs(u)) * np.where(v >= 0, 1.0, -1.0), v)
    w = np.stack([uf, c, vf], 1)
    w /= np.linalg.norm(w, axis=1)[:, None]
    p = w / np.abs(w).sum(1)[:, None]
    down = p[:, 1] < 0
    u2 = np.where(down, (1 - np.abs(p[:, 2])) * np.where(p[:, 0] >= 0, 1.0, -1.0), p[:, 0])
    v2 = np.where(down, (1 - np.abs(p[:, 0])) * np.where(p[:, 2] >= 0, 1.0, -1.0), p[:, 2])
    assert max(np.abs(u2 - u).max(), np.abs(v2 - v).max()) < 1e-14


def test_the_table_and_its_refusals():
    for n in vc.SIZES:
        for texels in (vc.constant(n), vc.one_texel(n), vc.hdr(n), vc.negzero(n)):
            m = ev.make_map(texels)
            assert m["q"].min() >= 1 and m["q"].max() == 65535 and m["Q"] == int(m["q"].astype(np.uint64).sum()) < 2 ** 32
            assert (np.diff(m["cum"].astype(np.int64)) >= 1).all()
        assert (ev.make_map(vc.one_texel(n))["q"] == 1).sum() == n * n - 1
        # -0.0 is not negative: the map is legal, its -0 texels weigh -0 and quantise to 1, and the table is hdr's but for the texel made brighter
        nz, plain = ev.make_map(vc.negzero(n)), ev.make_map(vc.hdr(n))
        assert nz["q"][0] == 1 and nz["q"][2 + n] == 1 and nz["q"][(n - 1) * n] == 1 and nz["q"].max() == 65535
        same = np.ones(n * n, bool)
        same[[0, 2 + n, 1 + 2 * n, (n - 1) * n]] = False
        np.testing.assert_array_equal(nz["q"][same], plain["q"][same])
    bad = vc.hdr(16)
    bad[3, 4, 1] = -1.0
    assert ev.make_map(bad) is None
    bad[3, 4, 1] = np.inf
    assert ev.make_map(bad) is None
    bad[3, 4, 1] = np.nan
    assert ev.make_map(bad) is None
    assert ev.make_map(np.zeros((16, 16, 3), np.float32)) is None
    for n in (2, 3, 12, 512):
        assert ev.make_map(vc.constant(n)) is None
    huge = vc.constant(16)
    huge[8, 8] = 3e38                                                                # (the weight at the pole's texels: 3e38 / r^3 with r < 1 overflows)
    assert ev.make_map(huge) is None


@pytest.fixture(scope="module")
def open_scene(vrt):
    return vc.open_scene(vrt)


def test_estimators_agree_and_sampling_lowers_the_variance(vrt, po, open_scene):
    """a one-texel sun on a dim sky over the open scene, 16 x 12, 2 bounces: the frame means of sample = 1 and sample = 0 (different
    seeds) agree within 4 standard errors of their difference, estimated from the restatement's own per-sample spread; and the mean
    per-pixel sample variance of sample = 1 is below that of sample = 0"""
    m = ev.make_map(vc.sun(16))
    w, h, spp = 16, 12, 96
    i0, i1 = {}, {}
    mean0, se0, var0 = ev.sample_stats(open_scene, None, w, h, po.shade_params(), spp, 2, 1, 1, (m, vc.SCALE, 0), i0)
    mean1, se1, var1 = ev.sample_stats(open_scene, None, w, h, po.shade_params(), spp, 2, 2, 1, (m, vc.SCALE, 1), i1)
    print("sample 0: mean %s se %s var %s" % (mean0, se0, var0))
    print("sample 1: mean %s se %s var %s" % (mean1, se1, var1))
    assert sum(i0["missed"]) > 0.5 * sum(i0["live"]) and sum(i1["open"]) > 0            # most bounce rays miss; environment rays get through
    se = np.sqrt(se0 ** 2 + se1 ** 2)
    assert (np.abs(mean1 - mean0) <= 4.0 * se).all(), (mean0, mean1, se)
    assert (var1 < var0).all(), (var0, var1)


def test_the_constant_map_is_the_plain_frame(vrt, po, open_scene):
    """CONSTANT on the CPU: every texel c, scale = 1, sample = 0, background = c is path_ref's frame bit for bit"""
    c = (0.4, 0.35, 0.25)
    w, h = 16, 12
    px, col, traced = ev.colour(open_scene, None, w, h, po.shade_params(background=c), 2, 3, 3, 1, (ev.make_map(vc.constant(16, c)), 1.0, 0))
    wpx, wcol, wtraced, _ = pr.frame(open_scene, None, w, h, po.shade_params(background=c), 2, 3, 3, 1)
    np.testing.assert_array_equal(px, wpx)
    np.testing.assert_array_equal(col.view(np.uint32), wcol.view(np.uint32))
    assert traced == wtraced


def test_the_gpu_cases_are_not_vacuous(vrt, po):
    """the closed scene has no miss at all and blocks every environment ray; the open one loses most bounce rays; the seeds of the
    ray test reach t = 0, t = Q - 1 and both ends of a row; the skipped rays are there"""
    p = po.shade_params()
    closed, opened = vc.closed_scene(vrt), vc.open_scene(vrt)
    m = ev.make_map(vc.sun(16))
    info = {}
    ev.colour(closed, None, vc.W, vc.H, p, 2, 3, 3, 0, (m, vc.SCALE, 1), info=info)
    assert sum(info["missed"]) == 0 and sum(info["open"]) == 0 and sum(info["sent"]) > 0 and (pr.primary(closed, po.camera_rays(vc.W, vc.H))["hits"]["dist"] != pr.LARGE).all()
    info = {}
    ev.colour(opened, None, vc.W, vc.H, p, 2, 3, 3, 0, (m, vc.SCALE, 1), roulette=(vc.ROULETTE["first"], vc.ROULETTE["q_min"]), info=info)
    assert sum(info["missed"]) > 0.5 * sum(info["live"]) and sum(info["open"]) > 0 and sum(info["killed"]) > 0
    hm = ev.make_map(vc.hdr(16))
    pts, seeds = vc.ray_points(16, hm)
    info = {}
    _, tmax, G, e, wE, real = ev.env_rays(hm, vc.SCALE, seeds, pts[:, 0:3], pts[:, 3:6], info)
    t = info["t"][0]
    assert (t == 0).any() and (t == hm["Q"] - 1).any() and (e % 16 == 0).any() and (e % 16 == 15).any()
    assert (~real).sum() > 100 and real.sum() > 100 and (tmax[~real] == -1).all() and (G[~real] == 0).all()
    assert ((hm["texels"][e] == 0).all(1) & ~real).any()                             # (a black texel skips its ray)
