"""CPU: tests/specular_ref.py (the restatement the specular GPU tests compare against) is held to what pins it -- the three identities of
the header's "Specular vertices", the estimator's expectation, the agreement of the three emitter forms, the pick at its edges -- and the
cases of tests/test_gpu_specular.py are shown to exercise what they are meant to."""
import numpy as np
import pytest

import adaptive_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import emissive_mis_ref as mir
import emissive_ref as er
import path_frame_cases as fc
import path_frame_ref as fr
import path_ref as pr
import specular_cases as sc
import specular_ref as sr

W, H = sc.W, sc.H
f32 = np.float32


def _emitter(form, b, pairs):
    return fc.emitter(form, b, pairs, sc.SCALE)


@pytest.fixture(scope="module")
def hall(vrt):
    return sc.hall(vrt)


@pytest.fixture(scope="module")
def hidden(vrt):
    return sc.hidden_mirror_hall(vrt)


@pytest.fixture(scope="module")
def ones(vrt):
    return sc.hall(vrt, (1.0, 1.0))


def _same(got, want_px, want_col, want_rays, what):
    np.testing.assert_array_equal(got["col"].view(np.uint32), np.ascontiguousarray(want_col, np.float32).view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got["px"], want_px, err_msg=what + ": pixels")
    assert got["rays"] == want_rays, "%s: rays traced %d, %d" % (what, got["rays"], want_rays)


@pytest.mark.parametrize("form", sc.FORMS)
def test_identity_a_no_specular_vertex_is_the_frame_of_today(po, vrt, hidden, form):
    """the hidden-mirror hall: against path_ref / emissive_ref / emissive_mis_ref through path_frame_ref, and with counts adaptive_ref"""
    b, pairs = hidden
    pp, em = po.shade_params(), _emitter(form, b, pairs)
    spp, bounces, seed = sc.CONFIG
    for name, shadow in (("framing", 1), (None, 0)):
        cam = None if name is None else csr.framing(W, H)
        info = {}
        got = sr.frame(b, cam, W, H, pp, spp, bounces, seed, shadow, em, info=info)
        assert info["specular_vertices"] == 0 and sum(info["mirror"]) == 0, info
        _same(got, *fr.colour(b, cam, W, H, pp, spp, bounces, seed, shadow, em), "%r %r" % (form, name))
    if form is None:
        px, col, n, _ = pr.frame(b, csr.framing(W, H), W, H, pp, spp, bounces, seed, 1)
        _same(sr.frame(b, csr.framing(W, H), W, H, pp, spp, bounces, seed, 1), px, col, n, "path_ref")
        counts = sc.counts_of()
        got = sr.frame(b, csr.framing(W, H), W, H, pp, sc.COUNTS["cap"], bounces, seed, 1, counts=counts)
        _same(got, *ar.frame(b, csr.framing(W, H), W, H, pp, counts, sc.COUNTS["cap"], bounces, seed, 1), "adaptive_ref")


@pytest.mark.parametrize("form", sc.FORMS)
def test_identity_b_without_bounces_every_vertex_is_last(po, hall, form):
    b, pairs = hall
    pp, em, cam = po.shade_params(), _emitter(form, b, pairs), csr.framing(W, H)
    info = {}
    got = sr.frame(b, cam, W, H, pp, 4, 0, 3, 1, em, info=info)
    assert info["specular_vertices"] > 0
    _same(got, *fr.colour(b, cam, W, H, pp, 4, 0, 3, 1, em), repr(form))


@pytest.mark.parametrize("shadow", [0, 1])
def test_identity_c_a_perfect_mirror_is_the_camera_frame_of_depth_two(po, vrt, ones, shadow):
    """bounces = 1, spp a power of two: a pixel whose primary hit has rho = 1 exactly is vxrt_render_camera's with max_depth = 2"""
    b, _ = ones
    rec = b["blas"].view(np.float32).reshape(-1, 40)
    p1 = po.shade_params()
    pp2 = po.shade_params(tuple(p1.ambient), tuple(p1.light_color), tuple(p1.light_pos), tuple(p1.background), 2)
    seen = 0
    for cam in (csr.framing(W, H), fc.cameras(vrt, 1, W, H)[0]):
        want_px, hits, want_col, _ = cr.frame(b, cam, W, H, pp2, shadow)
        got = sr.frame(b, cam, W, H, po.shade_params(), 4, 1, 9, shadow)
        found = hits["dist"] != cr.LARGE
        m = found & (rec[hits["blasIdx"] & 0x7fffffff, 38] == f32(1.0))
        assert m.sum() >= 10 and len(np.unique(want_px[m])) >= 3, (m.sum(), np.unique(want_px[m]))
        np.testing.assert_array_equal(got["col"][m].view(np.uint32), want_col[m].view(np.uint32))
        np.testing.assert_array_equal(got["px"][m], want_px[m])
        seen += int(m.sum())
    print("identity C: %d mirror pixels" % seen)


def test_the_pick_is_unbiased(po, vrt, hall):
    """16 x 12, csr.framing, one bounce, 256 spp: the frame mean with stochastic picks (seed 1) against the deterministic split at depth 0,
    rho_0 * (forced mirror) + (1 - rho_0) * (forced diffuse) per sample (seed 2), within 4 combined standard errors -- the rule of
    tests/test_emissive_cpu.py; and the frame without specular vertices is more than 10 of them away, so a dropped weight cannot hide."""
    b, _ = hall
    cam, pp = csr.framing(W, H), po.shade_params()
    m1, s1 = sr.sample_means(b, cam, W, H, pp, 256, 1, 1, 0)
    m2, s2 = sr.sample_means(b, cam, W, H, pp, 256, 1, 2, 0, split=True)
    se = np.sqrt(s1 * s1 + s2 * s2)
    z = np.abs(m1 - m2) / se
    m0, s0 = er.sample_means(b, cam, W, H, pp, 256, 1, 1, 0, 0, 0.0)      # (nee = 0 with scale 0 adds zeros: the plain path frame's mean)
    z0 = np.abs(m0 - m2) / np.sqrt(s0 * s0 + s2 * s2)
    print("unbiasedness: picks %r se %r, split %r se %r, z %r; not specular %r, z %r" % (m1, s1, m2, s2, z, m0, z0))
    assert (s1 > 0).all() and (s2 > 0).all()
    assert (z <= 4.0).all(), z
    assert (z0 > 10.0).all(), z0


def test_the_three_emitter_forms_agree(po, vrt, hall):
    """the hall at 2 bounces, 16 x 12, 256 spp, shadow = 0: the frame means of nee = 0, nee = 1 and MIS with specular vertices agree
    pairwise within 4 combined standard errors"""
    b, pairs = hall
    cam, pp = csr.framing(W, H), po.shade_params()
    res = {}
    for seed, form in enumerate(("nee0", "nee1", "mis"), 1):
        info = {}
        res[form] = sr.sample_means(b, cam, W, H, pp, 256, 2, seed, 0, _emitter(form, b, pairs), info=info)
        assert sum(info["mirror"]) > 0 and sum(info["specular_emitter"]) > 0, (form, info)
    for a, c in (("nee0", "nee1"), ("nee0", "mis"), ("nee1", "mis")):
        z = np.abs(res[a][0] - res[c][0]) / np.sqrt(res[a][1] ** 2 + res[c][1] ** 2)
        print("emitter forms with specular vertices: %s %r se %r, %s %r se %r, z %r" % (a, res[a][0], res[a][1], c, res[c][0], res[c][1], z))
        assert (z <= 4.0).all(), (a, c, z)


def test_the_gpu_cases_are_not_vacuous(po, vrt, hall):
    b, pairs = hall
    cam, pp = csr.framing(W, H), po.shade_params()
    spp, bounces, seed = sc.CONFIG
    info = {}
    got = sr.frame(b, cam, W, H, pp, spp, bounces, seed, 1, _emitter("nee0", b, pairs), info=info)
    print("non-vacuity: %r" % info)
    for key in ("mirror", "diffuse_at_specular", "specular_emitter"):
        assert len(info[key]) == bounces and min(info[key]) >= 1, (key, info)
    px, _, _ = fr.colour(b, cam, W, H, pp, spp, bounces, seed, 1, _emitter("nee0", b, pairs))
    differ = int((px != got["px"]).sum())
    print("non-vacuity: %d of %d pixels differ from the frame without specular vertices" % (differ, W * H))
    assert differ * 4 >= W * H
    # emitter sampling: mirror picks skip emitter rays at every depth, in both forms and with counts
    for form in ("nee1", "mis"):
        info = {}
        sr.frame(b, cam, W, H, pp, sc.COUNTS["cap"], bounces, seed, 1, _emitter(form, b, pairs), counts=sc.counts_of(), info=info)
        assert min(info["skipped_by_mirror"]) >= 1 and min(info["specular_emitter"][:2]) >= 1, (form, info)
    # the deep case keeps paths alive to the last depth, and the fixed camera sees a mirror
    s1, b16, seed16 = sc.DEEP
    info = {}
    sr.frame(b, cam, W, H, pp, s1, b16, seed16, 0, info=info)
    assert info["mirror"][-1] + info["diffuse_at_specular"][-1] >= 1, info
    info = {}
    sr.frame(b, None, W, H, pp, spp, bounces, seed, 0, info=info)
    assert info["mirror"][0] >= 1, info


def test_the_pick_at_its_edges():
    n = 4096
    seeds = np.random.default_rng(1).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seeds[:3] = (0, 1, 0xFFFFFFFF)
    always, _ = sr.pick(np.full(n, 1.0, np.float32), seeds)
    assert always.all()                                       # rho = 1 mirrors whatever xi
    for rho in sc.EDGE_RHO[1:]:
        never, _ = sr.pick(np.full(n, rho, np.float32), seeds)
        assert not never.any(), rho                           # 0, -0.3, NaN, +inf: not specular
    half, xi = sr.pick(np.full(n, 0.5, np.float32), seeds)
    assert ((xi < f32(0.5)) == half).all() and 0.45 < half.mean() < 0.55
    assert (xi >= 0).all() and (xi <= f32(1.0)).all()
    # seed 0 becomes 1
    a, xa = sr.pick(np.array([0.5], np.float32), np.array([0], np.uint32))
    c, xc = sr.pick(np.array([0.5], np.float32), np.array([1], np.uint32))
    assert xa[0] == xc[0] and a[0] == c[0]
    v, s = sc.pick_vertices()
    rays, lobe = sr.pick_step(v, s)
    assert 0 < lobe.sum() < len(lobe) and (rays[lobe == 0] == 0).all()
    d = rays[lobe == 1, 3:6].astype(np.float64)
    assert np.allclose((d * d).sum(1), 1.0, atol=1e-5)
