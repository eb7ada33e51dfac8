"""CPU: tests/emissive_ref.py (the restatement the emissive GPU tests compare against) is held to what pins it -- without emissive
materials it is tests/path_ref.py bit for bit, its selection is the definition's, and its two estimators agree -- and the cases of
tests/test_gpu_emissive.py are shown to exercise what they are meant to.

Estimator agreement (measured, seeds as below, 16 x 12, one bounce, 256 spp; z = |mean(nee = 1) - mean(nee = 0)| over the combined standard
error, per channel): see test_the_two_estimators_agree's docstring."""
import numpy as np
import pytest

import camera_ref as cr
import camera_secondary_ref as csr
import emissive_cases as ec
import emissive_ref as er
import path_ref as pr
import scenes

W, H = pr.W, pr.H


@pytest.fixture(scope="module")
def lit_hall(vrt):
    b, ranges = ec.hall(vrt)
    pairs = vrt.rtapi.emitter_pairs(b, ranges)
    return b, pairs, er.table(b, pairs)


def _same(got, want, what):
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": pixels")
    assert got[2] == want[2], "%s: rays traced %d, %d" % (what, got[2], want[2])


@pytest.mark.parametrize("name", ["framing", "orbit_1", None])
def test_without_emissive_materials_it_is_the_path_frame(po, vrt, name):
    b, pp = scenes.mirror_hall(vrt), po.shade_params()
    cam = None if name is None else csr.hall_cameras(vrt)[name]
    prim = pr.primary(b, po.camera_rays(W, H, 0, H) if cam is None else cr.rays(cam, W, H))
    for spp, bounces, shadow, seed in pr.CONFIGS:
        want = pr.frame(b, cam, W, H, pp, spp, bounces, seed, shadow, prim=prim)
        _same(er.frame(b, cam, W, H, pp, spp, bounces, seed, shadow, 0, 2.5, prim=prim), want, "%s %r" % (name, (spp, bounces, shadow, seed)))


def test_the_dark_variant_of_the_lit_hall_is_a_path_frame_too(po, vrt):
    """the geometry of emissive_cases.hall with both emissive colours zero: nothing is added anywhere"""
    b, _ = ec.hall(vrt, emissive=False)
    cam, pp = csr.hall_cameras(vrt)["framing"], po.shade_params()
    _same(er.frame(b, cam, W, H, pp, 2, 2, 1, 0, 0, 1.0), pr.frame(b, cam, W, H, pp, 2, 2, 1, 0), "dark hall")


def test_emitter_pairs_keeps_the_emissive_triangles(vrt, lit_hall):
    b, pairs, tab = lit_hall
    assert pairs.shape == (4, 2) and sorted(set(pairs[:, 0])) == [ec.CEILING, ec.LAMP]
    tri12, q, cum, Q = tab
    assert (tri12[:2, 9:12] == np.array(ec.LE_CEILING, np.float32)).all() and (tri12[2:, 9:12] == np.array(ec.LE_LAMP, np.float32)).all()
    # the lamp's world-space edges are those of no axis and not of the mesh's unit length: rotated, scaled by (60, 25, 40)
    e1 = tri12[2:, 3:6]
    assert (np.abs(e1) > 1.0).sum(1).min() >= 2
    assert q.max() == 65535 and (q >= 1).all() and Q == int(q.astype(np.uint64).sum())


def test_the_cases_are_not_vacuous(po, vrt, lit_hall):
    b, pairs, tab = lit_hall
    pp = po.shade_params()
    total = {}
    for name in ("framing", "orbit_1"):
        cam = csr.hall_cameras(vrt)[name]
        prim = pr.primary(b, cr.rays(cam, W, H))
        for spp, bounces, shadow, seed, nee in ec.CONFIGS:
            info = {}
            er.frame(b, cam, W, H, pp, spp, bounces, seed, shadow, nee, ec.SCALE, tab, prim=prim, info=info)
            for k, v in info.items():
                total[k] = (total.get(k, set()) | v) if isinstance(v, set) else total.get(k, 0) + v
            if nee == 0:
                assert info["bounce_emissive"] > 0, name              # a bounce ray hit an emitter
            else:
                assert info["unblocked"] > 0 and info["blocked"] > 0 and info["skipped_cos"] > 0 and info["folds"] > 0, (name, info)
            assert info["primary_emissive"] > 0 or name != "framing"  # emission visible at a primary hit
    assert total["primary_emissive"] > 0
    assert total["selected"] == set(range(len(pairs)))               # every entry, so both emitters


def _definition(cum, Q, r0):
    t = (int(r0) * int(Q)) >> 32
    return next(e for e in range(len(cum)) if int(cum[e]) > t)


def _bounded_search(cum, Q, r0):
    """the device's loop: at most 17 steps over [0, n - 1]"""
    t = (int(r0) * int(Q)) >> 32
    lo, hi = 0, len(cum) - 1
    for _ in range(17):
        if lo >= hi:
            break
        mid = lo + ((hi - lo) >> 1)
        if int(cum[mid]) > t:
            hi = mid
        else:
            lo = mid + 1
    assert lo >= hi
    return lo


@pytest.mark.parametrize("n", [1, 2, 257])
def test_selection_on_the_extremes_and_on_every_boundary(n):
    rng = np.random.default_rng(n)
    q = rng.integers(1, 65536, n).astype(np.uint32)
    q[rng.integers(0, n)] = 65535
    if n > 2:
        q[:5] = 1                                                     # (entries of the smallest weight next to each other)
    cum = np.cumsum(q.astype(np.uint64)).astype(np.uint32)
    Q = int(cum[-1])
    r0s = [0, 1, 2 ** 31, 2 ** 32 - 1]
    for c in [int(v) for v in cum[:-1]]:
        for t in (c - 1, c):                                          # the last t of entry e and the first of entry e + 1
            r0 = -((-t << 32) // Q)                                   # the smallest r0 with (r0 * Q) >> 32 == t
            assert (r0 * Q) >> 32 == t and r0 < 2 ** 32
            r0s += [r0, max(r0 - 1, 0)]
    got = er.select(cum, Q, np.array(r0s, np.uint32))
    for r0, e in zip(r0s, got):
        want = _definition(cum, Q, r0)
        assert int(e) == want and _bounded_search(cum, Q, r0) == want, (n, r0)
    assert int(got[0]) == 0 and int(got[3]) == n - 1


def test_a_65536_entry_table_is_searched_in_17_steps():
    cum = np.arange(1, 65537, dtype=np.uint32)
    for r0 in (0, 1, 2 ** 31, 2 ** 32 - 1, 12345678):
        assert _bounded_search(cum, 65536, r0) == (r0 * 65536) >> 32     # (cum[e] = e + 1 > t first at e = t)


def test_the_two_estimators_agree(po, vrt, lit_hall):
    """16 x 12, one bounce, 256 spp, framing camera, shadow = 0: the frame mean of nee = 1 (seed 2) against nee = 0 (seed 1) within 4
    combined standard errors, each run's from its own per-sample variances.  A missing cosine, pi or pdf factor moves the mean of one
    of them by a factor, i.e. by tens of standard errors.  Measured z per channel: 0.011, 0.088, 0.498 (means 1.25005 / 1.25000 in r; standard errors 0.0044 against 0.0009)."""
    b, pairs, tab = lit_hall
    w, h = 16, 12
    cam, pp = csr.framing(w, h), po.shade_params()
    m0, s0 = er.sample_means(b, cam, w, h, pp, 256, 1, 1, 0, 0, ec.SCALE, tab)
    m1, s1 = er.sample_means(b, cam, w, h, pp, 256, 1, 2, 0, 1, ec.SCALE, tab)
    z = np.abs(m1 - m0) / np.sqrt(s0 * s0 + s1 * s1)
    print("estimator agreement: mean nee=0 %r se %r, mean nee=1 %r se %r, z %r" % (m0, s0, m1, s1, z))
    assert (s0 > 0).all() and (s1 > 0).all() and (s1 < s0).all()     # (and emitter sampling is the quieter of the two)
    assert (z <= 4.0).all(), z
    # the direct light of the emitters is a visible part of the mean, so a wrong factor cannot hide in it
    d0, _ = er.sample_means(ec.hall(vrt, emissive=False)[0], cam, w, h, pp, 4, 1, 1, 0, 0, ec.SCALE)
    assert ((m0 - d0) > 10 * np.sqrt(s0 * s0 + s1 * s1)).all()
