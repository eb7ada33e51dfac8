"""CPU: tests/emissive_mis_ref.py (the restatement the GPU tests of multiple importance sampling compare against) is held to what pins
it -- its frame mean agrees with both estimators of tests/emissive_ref.py, it is the quieter one where each of them fails, its samples
are bounded by the emitter's radiance, its two weights sum to one, its lookup is the definition's -- and the cases of
tests/test_gpu_emissive_mis.py are shown to exercise what they are meant to."""
import numpy as np
import pytest

import camera_ref as cr
import camera_secondary_ref as csr
import emissive_cases as ec
import emissive_mis_cases as mc
import emissive_mis_ref as mr
import emissive_ref as er
import path_ref as pr

W, H = pr.W, pr.H
f32 = np.float32


@pytest.fixture(scope="module")
def lit_hall(vrt):
    """emissive_cases.hall with the pair list reversed: scene, pairs, table, index"""
    b, ranges = ec.hall(vrt)
    pairs = vrt.rtapi.emitter_pairs(b, ranges)[::-1].copy()
    return b, pairs, er.table(b, pairs), mr.index(pairs)


@pytest.fixture(scope="module")
def estimates(po, vrt, lit_hall):
    """(camera, bounces) -> ((mean, se) of nee = 0 with seed 1, of nee = 1 with seed 2, of MIS with seed 3, MIS's info): 16 x 12, 256 spp,
    shadow = 0.  Computed once for the tests below."""
    b, pairs, tab, idx = lit_hall
    w, h = 16, 12
    pp = po.shade_params()
    out = {}
    for name, cam in (("framing", csr.framing(w, h)), ("gap", mc.gap_camera(vrt, w, h))):
        for bounces in (1, 2):
            info = {}
            out[name, bounces] = (er.sample_means(b, cam, w, h, pp, 256, bounces, 1, 0, 0, mc.SCALE, tab),
                                  er.sample_means(b, cam, w, h, pp, 256, bounces, 2, 0, 1, mc.SCALE, tab),
                                  mr.sample_means(b, cam, w, h, pp, 256, bounces, 3, 0, mc.SCALE, tab, idx, info), info)
    return out


@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("name", ["framing", "gap"])
def test_the_frame_mean_agrees_with_both_estimators(estimates, name, bounces):
    """The frame mean of MIS (seed 3) against nee = 0 (seed 1) and against nee = 1 (seed 2) within 4 combined standard errors, each run's
    from its own per-sample variances: tests/test_emissive_cpu.py's rule.  A weight that does not partition moves the mean by a visible
    part of the emitters' light.  Measured, largest z over the channels against nee = 0 / nee = 1:
      framing, 1 bounce  0.22 / 1.24     framing, 2 bounces  0.88 / 1.05     gap, 1 bounce  1.82 / 1.21     gap, 2 bounces  1.15 / 2.30"""
    (m0, s0), (m1, s1), (mm, sm), _ = estimates[name, bounces]
    z0 = np.abs(mm - m0) / np.sqrt(sm * sm + s0 * s0)
    z1 = np.abs(mm - m1) / np.sqrt(sm * sm + s1 * s1)
    print("agreement %s %d: mean nee=0 %r nee=1 %r mis %r; z against nee=0 %r, against nee=1 %r" % (name, bounces, m0, m1, mm, z0, z1))
    assert (sm > 0).all() and (s0 > 0).all() and (s1 > 0).all()
    assert (z0 <= 4.0).all() and (z1 <= 4.0).all(), (z0, z1)


@pytest.mark.parametrize("bounces", [1, 2])
def test_quieter_than_both_in_the_gap(estimates, bounces):
    """Between the ceiling panel and the ceiling light 5 units below it, the standard error of MIS is below that of both other estimators
    in every channel.  A condition, not a tolerance.  Measured se(r) nee = 0 / nee = 1 / MIS: 1 bounce 0.00327 / 0.0319 / 0.00148, 2 bounces
    0.00383 / 0.0358 / 0.00167 -- below half the error of the better one and a twentieth of nee = 1's.  The largest weighted term MIS
    adds to a sample (Gm, or Emi * wB) is 5.9888: below the ceiling light's radiance of 6."""
    (m0, s0), (m1, s1), (mm, sm), info = estimates["gap", bounces]
    print("gap %d: se nee=0 %r nee=1 %r mis %r; largest weighted term %r" % (bounces, s0, s1, sm, info["largest"]))
    assert (sm < s0).all() and (sm < s1).all(), (s0, s1, sm)


@pytest.mark.parametrize("bounces", [1, 2])
def test_elsewhere_the_errors_are_recorded(estimates, bounces):
    """csr.framing, where nee = 1 is the good estimator: recorded, not gated.  Measured se(r) nee = 0 / nee = 1 / MIS: 1 bounce 0.00438 /
    0.00091 / 0.00094, 2 bounces 0.00507 / 0.00222 / 0.00130 -- on a par with the better one."""
    (m0, s0), (m1, s1), (mm, sm), info = estimates["framing", bounces]
    print("framing %d: se nee=0 %r nee=1 %r mis %r; largest weighted term %r" % (bounces, s0, s1, sm, info["largest"]))
    assert np.isfinite(sm).all()


def test_every_sample_is_bounded_by_the_radiance(lit_hall):
    """Ray origins 1e-3 .. 10 units from each emitter along its normal, N' towards it and at a grazing angle: every channel of Gm is at
    most Le * scale * (1 + 2^-20) -- mathematically Le * scale * pb / (pe + pb) <= Le * scale, and the margin is 16 roundings of 2^-24
    -- while G of nee = 1 exceeds 100 Le in the same set."""
    b, pairs, tab, idx = lit_hall
    seeds, I, N = mc.near_field(tab)
    for scale in (1.0, 0.37):
        _, _, G, e, real = er.emitter_rays(tab, scale, seeds, I, N)
        _, _, Gm, e2, real_m, wE = mr.emitter_rays(tab, scale, seeds, I, N)
        Le = tab[0][e, 9:12]
        bound = (Le * f32(scale)) * f32(1 + 2.0 ** -20)
        print("bound: scale %g, %d rays, %d real; largest G / (Le scale) %g, largest Gm / (Le scale) %.9g" %
              (scale, len(seeds), int(real_m.sum()), float((G / (Le * f32(scale))).max()), float((Gm / (Le * f32(scale))).max())))
        assert real_m.sum() > len(seeds) // 2 and (real_m <= real).all()
        assert (Gm <= bound).all(), float((Gm / bound).max())
        assert (G > 100 * Le * f32(scale)).any()                       # (not vacuous: the unweighted sample is unbounded here)
        assert set(e.tolist()) == set(range(len(pairs)))


def test_the_two_weights_partition(po, vrt, lit_hall):
    """The unblocked emitter rays of a frame, traced again for their closest hit without a tmax: where they hit the emitter they chose,
    |wE + wB - 1| <= 64 * 2^-24 = 3.8e-6 -- two weights of about ten roundings each, and t against d a few ulps apart.  Measured maximum
    over the 34,397 such rays of the gap and the framing camera: 4.47e-7, an eighth of the bound."""
    b, pairs, tab, idx = lit_hall
    worst, n = 0.0, 0
    for cam in (mc.gap_camera(vrt, W, H), csr.framing(W, H)):
        keep = []
        mr.frame(b, cam, W, H, po.shade_params(), 2, 2, 3, 0, mc.SCALE, tab, idx, keep=keep)
        for k in keep:
            o = k["open"]
            hits = cr._trace(b, k["er"][o])
            e_hit, wB = mr.hit_weights(tab, idx, k["er"][o], hits, k["Nf"][o])
            same = (hits["dist"] != cr.LARGE) & (e_hit == k["e_ray"][o])
            err = np.abs((k["wE"][o][same].astype(np.float64) + wB[same].astype(np.float64)) - 1.0)
            worst, n = max(worst, float(err.max()) if len(err) else 0.0), n + int(same.sum())
    print("partition: %d rays, largest |wE + wB - 1| = %.3g (bound %.3g)" % (n, worst, 64 * 2.0 ** -24))
    assert n > 1000
    assert worst <= 64 * 2.0 ** -24, worst


# ---- the lookup ----
def _linear_scan(pairs, keys):
    """the definition: the first entry of the pair list that names the key, 0xFFFFFFFF if none does"""
    first = {}
    for e, (bb, t) in enumerate(np.asarray(pairs, np.uint32).tolist()):
        first.setdefault((bb, t), e)
    return np.array([first.get((bb, t), mr.NOT_LISTED) for bb, t in keys.tolist()], np.uint32)


def _bounded_search(idx, keys):
    """the device's loop over all keys at once: at most 17 steps over [0, n - 1], the smallest position whose key is not below the wanted"""
    ik = (idx[:, 0].astype(np.uint64) << np.uint64(32)) | idx[:, 1].astype(np.uint64)
    want = (keys[:, 0].astype(np.uint64) << np.uint64(32)) | keys[:, 1].astype(np.uint64)
    lo, hi = np.zeros(len(want), np.int64), np.full(len(want), len(idx) - 1, np.int64)
    for _ in range(17):
        go = lo < hi
        mid = lo + ((hi - lo) >> 1)
        below = ik[mid] < want
        lo = np.where(go & below, mid + 1, lo)
        hi = np.where(go & ~below, mid, hi)
    assert (lo >= hi).all()                                           # 17 steps were enough
    return np.where(ik[lo] == want, idx[lo, 2], np.uint32(mr.NOT_LISTED)).astype(np.uint32)


@pytest.mark.parametrize("n", [1, 2, 257, 65536])
def test_lookup_against_a_linear_scan_and_the_17_step_loop(n):
    """Shuffled tables (from n = 257 on with pairs listed twice and three times): every listed key, each key's neighbours in triIdx and
    in blasIdx, keys below the smallest and above the largest, and a blasIdx with the top bit set."""
    rng = np.random.default_rng(n)
    k = rng.choice(6 * 2 ** 17, size=n, replace=False)
    pairs = np.stack([k >> 17, (k & (2 ** 17 - 1)) * 3 + 1], 1).astype(np.uint32)     # (triIdx = 1 mod 3: neighbours are not listed)
    if n > 2:
        pairs[-40:-20] = pairs[:20]                                                   # listed twice
        pairs[-20:-10] = pairs[:10]                                                   # ... and a third time
    pairs = mc.shuffled(pairs, seed=n + 1)
    idx = mr.index(pairs)
    ik = (idx[:, 0].astype(np.uint64) << np.uint64(32)) | idx[:, 1].astype(np.uint64)
    assert (np.diff(ik.astype(np.float64)) >= 0).all() and sorted(idx[:, 2].tolist()) == list(range(n))
    dup = np.nonzero(ik[1:] == ik[:-1])[0]
    assert (idx[dup + 1, 2] > idx[dup, 2]).all() and (n <= 2 or len(dup) >= 30)          # pairs listed more than once are sorted by e
    keys = mc.lookup_keys(pairs)
    got = mr.lookup(idx, keys[:, 0], keys[:, 1])
    np.testing.assert_array_equal(got, _linear_scan(pairs, keys))
    np.testing.assert_array_equal(got, _bounded_search(idx, keys))
    assert (got[:n] != mr.NOT_LISTED).all() and (got[n:] == mr.NOT_LISTED).sum() >= min(n, 8) + 4
    top = keys[keys[:, 0] >= 2 ** 31]
    assert len(top) and (mr.lookup(idx, top[:, 0], top[:, 1]) == mr.NOT_LISTED).all()


def test_the_index_of_a_shuffled_table_is_not_the_identity(vrt):
    for which in mc.TABLE_NAMES:
        _, pairs = mc.hall(vrt, which)
        idx = mr.index(pairs)
        assert (idx[:, 2] != np.arange(len(idx))).any(), which


# ---- the cases of the GPU tests ----
def test_the_cases_are_not_vacuous(po, vrt):
    pp = po.shade_params()
    for which in mc.TABLE_NAMES:
        b, pairs = mc.hall(vrt, which)
        tab, idx = er.table(b, pairs), mr.index(pairs)
        total, blas_hit, seen = {}, set(), {}
        for name, cam in mc.cameras(vrt, W, H).items():
            prim = pr.primary(b, po.camera_rays(W, H, 0, H) if cam is None else cr.rays(cam, W, H))
            for spp, bounces, shadow, seed in mc.CONFIGS:
                info, keep = {}, []
                mr.frame(b, cam, W, H, pp, spp, bounces, seed, shadow, mc.SCALE, tab, idx, prim=prim, info=info, keep=keep)
                for k, v in info.items():
                    if not isinstance(v, (set, float)):
                        total[k] = total.get(k, 0) + v
                for k in keep:
                    listed = k["emits"] & (k["e"] != mr.NOT_LISTED)
                    blas_hit |= set(int(v) for v in np.unique(k["hits"]["blasIdx"][listed] & np.uint32(0x7fffffff)))
            # per camera: bounce hits with 0 < wB < 1, emitter rays with wE < 1, and skipped, blocked and unblocked emitter rays
            assert all(total[k] > seen.get(k, 0) for k in ("wB_between", "wE_below_one", "skipped", "blocked", "unblocked")), (which, name, total)
            seen = dict(total)
        assert total["primary_emissive"] > 0
        assert (total["wB_one_unlisted"] > 0) == (which == "partial"), (which, total)
        # bounce rays found emitters under every instance record that places one: the twice-placed lamp under both of its records
        assert blas_hit == set(int(v) for v in np.unique(pairs[:, 0])), (which, blas_hit)
