"""CPU: the cases tests/test_gpu_denoise.py holds the a-trous kernels to (tests/denoise_cases.py, restated by tests/denoise_ref.py) are
shown to exercise what they are meant to, and the restatement is held to the identities of the definition.

Which conditions a case can meet is a matter of its shape and its parameters:
  - a frame thinner than the stencil (1x1, 7x1, 1x5) has room for a window skip and, from 5 pixels on, a miss and a zero normal, but not
    for a crease and a depth step: the six tap conditions are asserted on every frame of at least 45x37 and on every path configuration;
  - a term whose sigma is +inf has weight 1 and normal_power 0 leaves the crease's dot of 0.8 above 0.5, so "down-weighted below 0.5
    by wz / wc" is asserted where that sigma is finite, and "by dn" everywhere (the zero normal gives dn = 0 with any power)."""
import numpy as np
import pytest

import camera_secondary_ref as csr
import denoise_cases as dc
import denoise_ref as dr
import scenes

INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h", dc.BIG)
def test_every_big_synthetic_case_meets_every_tap_condition(w, h):
    S, P, N, _, _ = dc.synthetic(w, h)
    unguided = {it: dr.atrous(S, P, N, it, *dc.UNGUIDED) for it in dc.ITERATIONS}
    for it, npow, sz, sl in dc.cases(w, h):
        st = {}
        F = dr.atrous(S, P, N, it, npow, sz, sl, st)
        what = "%dx%d %r: %r" % (w, h, (it, npow, sz, sl), st)
        assert st["skip_window"] > 0 and st["skip_miss"] > 0 and st["skip_weight"] > 0, what
        assert st["low_dn"] > 0, what
        assert st["low_wz"] > 0 or sz == INF, what
        assert st["low_wc"] > 0 or sl == INF, what
        assert st["pass_through"] >= it, what   # (the zero normal, every iteration)
        if (npow, sz, sl) != dc.UNGUIDED:
            assert (_bits(F) != _bits(unguided[it])).any(), what
        disc = P[..., 3] == 0
        np.testing.assert_array_equal(_bits(F[disc]), _bits(S[disc]))   # (a miss keeps its sentinel)
        assert not (np.abs(F[~disc]) > 1e3).any(), what                 # (and leaks it nowhere)


@pytest.mark.parametrize("w,h", [f for f in dc.FRAMES if f not in dc.BIG])
def test_the_thin_frames_skip_what_fits(w, h):
    S, P, N, _, _ = dc.synthetic(w, h)
    for it, npow, sz, sl in dc.cases(w, h):
        st = {}
        dr.atrous(S, P, N, it, npow, sz, sl, st)
        assert st["skip_window"] > 0
        if w * h >= 5:
            assert st["skip_miss"] > 0 and st["skip_weight"] > 0 and st["pass_through"] > 0, (w, h, st)


def test_the_synthetic_set_passes_pixels_through():
    n = 0
    for w, h in dc.FRAMES:
        st = {}
        dr.atrous(*dc.synthetic(w, h)[:3], 1, *dc.GUIDED, st)
        n += st["pass_through"]
    assert n > 0


def test_rmse_against_the_noise_free_base_falls():
    S, P, N, base, clean = dc.synthetic(45, 37)
    F = dr.atrous(S, P, N, 5, *dc.GUIDED)
    before = float(np.sqrt(np.mean((S[clean] - base[clean]) ** 2)))
    after = float(np.sqrt(np.mean((F[clean] - base[clean]) ** 2)))
    assert np.isfinite(after) and after < 0.25 * before, (before, after)   # (0.151 -> 0.016)
    assert 0.8 * dc.NOISE < before < 1.2 * dc.NOISE


@pytest.mark.parametrize("w,h", dc.FRAMES)
def test_no_iterations_return_the_input(w, h):
    S, P, N, _, _ = dc.synthetic(w, h)
    np.testing.assert_array_equal(_bits(dr.atrous(S, P, N, 0, *dc.GUIDED)), _bits(S))


def test_the_infinite_position_and_the_nan_signal_stay_where_they_are():
    """with a finite sigma_l a NaN signal poisons only its own pixel (the tap's weight is NaN, `w > 0` is false); with sigma_l = +inf the
    weight is finite and the NaN spreads, as the definition says it must"""
    S, P, N, _, _ = dc.synthetic(45, 37)
    assert np.isnan(dr.atrous(S, P, N, 5, *dc.GUIDED)).any(2).sum() == 1
    assert np.isnan(dr.atrous(S, P, N, 5, 7, 1.0, INF)).any(2).sum() > 1


# ---- the denoised path frame ----
@pytest.fixture(scope="module")
def hall(vrt):
    return scenes.mirror_hall(vrt)


def _camera(vrt, name):
    return None if name is None else csr.hall_cameras(vrt)[name]


@pytest.fixture(scope="module")
def path_runs(po, vrt, hall):
    cache = {}

    def get(name, cfg, window=(0, dc.H)):
        key = (name, cfg, window)
        if key not in cache:
            spp, bounces, shadow, seed = cfg
            st = {}
            out = dr.path_frame(hall, _camera(vrt, name), dc.W, dc.H, po.shade_params(), spp, bounces, seed, shadow, dc.PATH_DN, window[0], window[1],
                                stats=st)
            cache[key] = (out, st)
        return cache[key]
    return get


@pytest.mark.parametrize("cfg", dc.PATH_CONFIGS)
@pytest.mark.parametrize("name", dc.PATH_CAMERAS)
def test_path_configurations_meet_every_tap_condition(po, vrt, hall, path_runs, name, cfg):
    """every configuration from every camera of the GPU test that looks at the hall from outside.  From inside the blob -- a closed
    surface -- every primary ray hits, no path ever sees the background and E is all but constant (its luminance varies by about 1 %), so
    a miss tap, a zero weight and a luminance weight below 0.5 cannot occur there with any sigma_l that means something elsewhere: that
    camera is in the GPU test for its normals and depths (dn and wz), which are asserted."""
    out, st = path_runs(name, cfg)
    keys = ("skip_window", "low_dn", "low_wz") if name == "inside_blob" else ("skip_window", "skip_miss", "skip_weight", "low_dn", "low_wz", "low_wc")
    for key in keys:
        assert st[key] > 0, (name, cfg, key, st)
    assert np.isfinite(out["col"]).all()
    it, npow, sz, sl = dc.PATH_DN
    hit = out["position"][..., 3] != 0
    unguided = dr.atrous(out["E"], out["position"], out["normal"], it, *dc.UNGUIDED)
    assert (_bits(out["F"][hit]) != _bits(unguided[hit])).any()
    assert (_bits(out["col"]) != _bits(out["noisy"])).any()


def test_a_row_window_is_its_own_image(path_runs):
    out, st = path_runs("framing", dc.PATH_CONFIGS[0], dc.PATH_WINDOW)
    whole = path_runs("framing", dc.PATH_CONFIGS[0])[0]
    y0, y1 = dc.PATH_WINDOW
    assert st["taps"] > 0
    np.testing.assert_array_equal(_bits(out["noisy"]), _bits(whole["noisy"][y0:y1]))
    assert (_bits(out["col"][:4]) != _bits(whole["col"][y0:y0 + 4])).any()   # (the rows next to the window's edge lose taps)


def test_no_iterations_are_the_path_frame(po, vrt, hall):
    import path_ref as pr
    cam = _camera(vrt, "framing")
    out = dr.path_frame(hall, cam, dc.W, dc.H, po.shade_params(), 2, 3, 3, 1, (0,) + dc.PATH_DN[1:])
    px, col, n, _ = pr.frame(hall, cam, dc.W, dc.H, po.shade_params(), 2, 3, 3, 1)
    np.testing.assert_array_equal(_bits(out["col"]), _bits(col))
    np.testing.assert_array_equal(out["px"], px)
    assert out["rays"] == n


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("shadow", [0, 1])
def test_without_bounces_the_frame_is_the_direct_term(po, vrt, hall, spp, shadow):
    """bounces = 0, spp a power of two: c = D, E = +0, F = +0, colour = D + A * 0 = D wherever D is not -0 (-0 + 0 is +0)"""
    out = dr.path_frame(hall, _camera(vrt, "framing"), dc.W, dc.H, po.shade_params(), spp, 0, 5, shadow, dc.PATH_DN)
    D, col = out["direct"], out["col"]
    keep = _bits(D) != 0x80000000
    np.testing.assert_array_equal(_bits(col)[keep], _bits(D)[keep])
    assert (out["position"][..., 3] != 0).any() and not (_bits(out["E"]) != 0).any()
