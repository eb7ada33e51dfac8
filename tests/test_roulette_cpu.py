"""CPU: tests/roulette_ref.py (the restatement the roulette GPU tests compare against) is held to what pins it -- the stand-alone rule on
hostile throughputs, the frame without roulette, the identities of the header's "Russian roulette", the estimator's expectation -- and
the cases of tests/test_gpu_roulette.py (tests/roulette_cases.py) are shown to exercise what they are meant to."""
import ctypes as C

import numpy as np
import pytest

import camera_secondary_ref as csr
import emissive_ref as er
import path_frame_cases as fc
import path_frame_ref as fr
import roulette_cases as rc
import roulette_ref as rr

W, H = rc.W, rc.H
f32 = np.float32


@pytest.fixture(scope="module")
def dark(vrt):
    return rc.dark(vrt)


@pytest.fixture(scope="module")
def white(vrt):
    return rc.white(vrt)


def _same(got, want, what):
    np.testing.assert_array_equal(got["col"].view(np.uint32), want["col"].view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got["px"], want["px"], err_msg=what + ": pixels")
    assert got["rays"] == want["rays"], "%s: rays traced %d, %d" % (what, got["rays"], want["rays"])


def _rr(case):
    return (case["first"], case["q_min"])


def test_the_python_interface(vrt):
    """the names the issue gives: RouletteParams with its defaults, the roulette argument, the stand-alone call, the prototypes"""
    R = vrt.rtapi
    p = R.RouletteParams()
    assert (p.enable, p.first, p.reserved) == (1, 2, 0) and p.q_min == f32(0.05) and C.sizeof(p) == 16
    p = R.RouletteParams(0, 5, 0.25)
    assert (p.enable, p.first, p.q_min) == (0, 5, 0.25)
    assert "roulette" in R.render_path_frame.__code__.co_varnames and callable(R.roulette)
    L = R._lib()
    assert L.vxrt_render_path_frame_ex.argtypes[3] == C.POINTER(R.RouletteParams) and L.vxrt_roulette.argtypes[3] == C.c_float


def test_the_rule_on_hostile_throughputs():
    """the stand-alone rule, line by line in Python floats of one entry at a time, against the vectorised restatement"""
    for q_min in (0.05, 1.0, rc.Q_TINY, 0.5):
        thr, seeds = rc.hostile(q_min)
        out, alive, drew = rr.step(thr, seeds, q_min)
        s = seeds.copy()
        s[s == 0] = 1
        xi = er.to_float(er.xorshift(s))
        qm = f32(q_min)
        seen = {"nan": 0, "floor": 0, "no_draw": 0, "dead": 0, "survivor": 0}
        with np.errstate(all="ignore"):
            for i in range(len(thr)):
                x, y, z = thr[i]
                m = x
                if y > m:
                    m = y
                if z > m:
                    m = z
                q = m
                if not (q >= qm):
                    q = qm
                    seen["floor"] += 1
                    seen["nan"] += int(np.isnan(m))
                if q >= f32(1.0):
                    want, lives = thr[i], 1
                    seen["no_draw"] += 1
                elif xi[i] < q:
                    want, lives = np.array([x / q, y / q, z / q], np.float32), 1
                    seen["survivor"] += 1
                else:
                    want, lives = np.zeros(3, np.float32), 0
                    seen["dead"] += 1
                assert alive[i] == lives and bool(drew[i]) == (not q >= f32(1.0)), (i, thr[i], q)
                nan = np.isnan(want)
                assert (np.isnan(out[i]) == nan).all() and (out[i][~nan].view(np.uint32) == want[~nan].view(np.uint32)).all(), (i, thr[i], out[i], want)
        print("q_min %r: %r" % (q_min, seen))
        assert seen["nan"] >= 3 and seen["floor"] > seen["nan"] and seen["no_draw"] > 0
        if q_min < 1.0:
            assert seen["survivor"] > 0 and seen["dead"] > 0
        else:
            assert seen["survivor"] == 0 and seen["dead"] == 0 and alive.all()
    # exactly q_min is not floored and exactly 1 takes no draw; the largest float below 1 draws and is divided
    below = np.nextafter(f32(1.0), f32(0.0))
    t = np.array([[0.05, 0.01, 0.0], [1.0, 0.2, 0.2], [below, 0.5, 0.25]], np.float32)
    out, alive, drew = rr.step(t, np.array([1, 1, 1], np.uint32), 0.05)
    assert list(drew) == [True, False, True] and alive[1] == 1 and (out[1] == t[1]).all()
    assert alive[2] == 1 and out[2, 0] == f32(1.0) and out[2, 1] == f32(0.5) / below


def test_a_seed_of_zero_becomes_one():
    t = np.full((2, 3), 0.5, np.float32)
    out, alive, _ = rr.step(t, np.array([0, 1], np.uint32), 0.05)
    assert alive[0] == alive[1] and (out[0] == out[1]).all()
    xi = er.to_float(er.xorshift(np.array([1], np.uint32)))[0]
    assert alive[0] == int(xi < f32(0.5))


def test_without_roulette_the_frame_is_the_descriptors(po, vrt, dark):
    """roulette = None: path_frame_ref's frame, every emitter form, counts, and the filter chain's outputs"""
    b, pairs = dark
    pp, cam = po.shade_params(), rc.cameras(vrt)[0]
    for form in (None,) + rc.FORMS:
        em = fc.emitter(form, b, pairs)
        _same(rr.frame(b, cam, W, H, pp, 2, 3, 5, 1, em), fr.frame(b, cam, W, H, pp, 2, 3, 5, 1, em), repr(form))
    raw = rc.counts_of()
    em = fc.emitter("mis", b, pairs)
    _same(rr.frame(b, cam, W, H, pp, 4, 2, 3, 1, em, raw), fr.frame(b, cam, W, H, pp, 4, 2, 3, 1, em, raw), "counts")
    got, want = rr.frame(b, cam, W, H, pp, 2, 2, 3, 1, em, dn=fc.DN), fr.frame(b, cam, W, H, pp, 2, 2, 3, 1, em, dn=fc.DN)
    _same(got, want, "denoised")
    for k in ("direct", "albedo", "F"):
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32))


def test_the_identities(po, vrt, dark, white):
    """(c) the white hall, (d) first >= bounces, (e) q_min = 1: the frame without roulette, bit for bit, and no draw was taken"""
    pp, cam = po.shade_params(), rc.cameras(vrt)[0]
    b, pairs = white
    c, info = rc.C, {}
    plain = fr.frame(b, cam, W, H, pp, c["spp"], c["bounces"], c["seed"], c["shadow"])
    _same(rr.frame(b, cam, W, H, pp, c["spp"], c["bounces"], c["seed"], c["shadow"], roulette=_rr(c), info=info), plain, "white")
    assert sum(info["drew"]) == 0 and min(info["live"]) > 0, info
    b, pairs = dark
    plain = fr.frame(b, cam, W, H, pp, c["spp"], c["bounces"], c["seed"], c["shadow"])
    for case in rc.D + (rc.E,):
        info = {}
        _same(rr.frame(b, cam, W, H, pp, case["spp"], case["bounces"], case["seed"], case["shadow"], roulette=_rr(case), info=info), plain, repr(case))
        assert sum(info["drew"]) == 0, info
    info = {}
    got = rr.frame(b, cam, W, H, pp, c["spp"], c["bounces"], c["seed"], c["shadow"], roulette=_rr(c), info=info)
    assert sum(info["killed"]) > 0 and (got["px"] != plain["px"]).any() and got["rays"] < plain["rays"]     # (the identities are not vacuous on the dark hall)


def test_the_dark_scene_kills_paths(po, vrt, dark):
    """case (a): the live count falls at every depth, to less than half by the last; the floor is reached; fewer rays than the plain
    frame.  Case (b) from inside the blob: every path is dead after the first draw"""
    b, pairs = dark
    pp, a = po.shade_params(), rc.A
    w, h, (y0, y1) = rc.ODD_W, rc.ODD_H, rc.ODD_ROWS
    cam = rc.cameras(vrt, 1, w, h)[0]
    info = {}
    got = rr.frame(b, cam, w, h, pp, a["spp"], a["bounces"], a["seed"], a["shadow"], roulette=_rr(a), y0=y0, y1=y1, info=info)
    plain = fr.frame(b, cam, w, h, pp, a["spp"], a["bounces"], a["seed"], a["shadow"], y0=y0, y1=y1)
    print("case a: %r; rays %d, plain %d" % (info, got["rays"], plain["rays"]))
    live = info["live"]
    assert len(live) == a["bounces"] and all(live[k + 1] < live[k] for k in range(len(live) - 1)) and 0 < 2 * live[-1] < live[0], live
    assert info["floored"] > 0 and min(info["killed"][:-1]) > 0 and info["drew"][-1] == 0, info      # (the last vertex takes no draw)
    assert got["rays"] < plain["rays"] and (got["px"] != plain["px"]).sum() * 4 > (y1 - y0) * w
    bb, info_b = rc.B, {}
    other = rr.frame(b, cam, w, h, pp, bb["spp"], bb["bounces"], bb["seed"], bb["shadow"], roulette=_rr(bb), y0=y0, y1=y1, info=info_b)
    # (the floor matters from a's camera too: other paths die -- those with thr = 0, which add nothing either way -- and other rays are traced)
    assert info_b["killed"] != info["killed"] and other["rays"] != got["rays"]
    inside, info_i = csr.hall_cameras(vrt, w, h)["inside_blob"], {}
    rr.frame(b, inside, w, h, pp, bb["spp"], bb["bounces"], bb["seed"], bb["shadow"], roulette=_rr(bb), y0=y0, y1=y1, info=info_i)
    assert info_i["live"][0] == (y1 - y0) * w * bb["spp"] and info_i["killed"][0] == info_i["live"][0] and sum(info_i["live"][1:]) == 0, info_i


def test_the_cases_with_emitter_forms_and_counts_draw(po, vrt, dark):
    """(f), (g), (h): paths are killed at vertices that would have sent an emitter ray, with counts every distinct count is met"""
    b, pairs = dark
    pp, cam = po.shade_params(), rc.cameras(vrt)[0]
    f = rc.F
    for form in rc.FORMS:
        em, info = fc.emitter(form, b, pairs), {}
        got = rr.frame(b, cam, W, H, pp, f["spp"], f["bounces"], f["seed"], f["shadow"], em, roulette=_rr(f), info=info)
        plain = fr.frame(b, cam, W, H, pp, f["spp"], f["bounces"], f["seed"], f["shadow"], em)
        assert min(info["killed"][:-1]) > 0 and got["rays"] < plain["rays"] and (got["px"] != plain["px"]).any(), (form, info)
    g, raw = rc.G, rc.counts_of()
    assert len(np.unique(np.clip(raw, 1, g["spp"]))) >= 3 and raw.min() == 0 and raw.max() > g["spp"]
    for form in rc.G_FORMS:
        info = {}
        rr.frame(b, cam, W, H, pp, g["spp"], g["bounces"], g["seed"], g["shadow"], fc.emitter(form, b, pairs), raw, _rr(g), info=info)
        assert info["drew"][0] == 0 and min(info["killed"][1:-1]) > 0, (form, info)                    # (first = 2: vertex 1 takes no draw)


@pytest.mark.parametrize("form", rc.UNBIASED["forms"])
def test_roulette_is_unbiased(po, vrt, dark, form):
    """16 x 12, the dark hall, 4 bounces, 128 spp: the frame mean with roulette (seed 2) against the frame without it (seed 1), per channel
    z of the image mean as tests/test_specular_cpu.py forms it, |z| <= 3; and the deliberately wrong variant -- survivors not divided by
    q -- from the same seed is more than 10 standard errors away, so a dropped division cannot hide"""
    b, pairs = dark
    u, pp, cam = rc.UNBIASED, po.shade_params(), rc.cameras(vrt)[0]
    em = fc.emitter(form, b, pairs)
    args = (b, cam, W, H, pp, u["spp"], u["bounces"])
    m0, s0 = rr.sample_means(*args, u["seeds"][0], u["shadow"], em)
    info = {}
    m1, s1 = rr.sample_means(*args, u["seeds"][1], u["shadow"], em, _rr(u), info=info)
    m2, s2 = rr.sample_means(*args, u["seeds"][1], u["shadow"], em, _rr(u), divide=False)
    z = np.abs(m1 - m0) / np.sqrt(s0 * s0 + s1 * s1)
    zw = np.abs(m2 - m0) / np.sqrt(s0 * s0 + s2 * s2)
    print("unbiasedness %r: plain %r se %r, roulette %r se %r, z %r; not divided %r, z %r; %r" % (form, m0, s0, m1, s1, z, m2, zw, info))
    assert (s0 > 0).all() and (s1 > 0).all() and sum(info["killed"]) * 2 > info["live"][0]
    assert (z <= 3.0).all(), z
    assert (zw > 10.0).all(), zw
