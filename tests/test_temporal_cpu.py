"""CPU: the cases tests/test_gpu_temporal.py holds the temporal accumulation kernel to (tests/temporal_cases.py, restated by
tests/temporal_ref.py) are shown to exercise what they are meant to, and the restatement is held to the identities of the definition."""
import numpy as np
import pytest

import temporal_cases as tc
import temporal_ref as tr

OUTCOMES = ("miss", "empty_history", "behind", "outside", "skip_window", "skip_invalid", "skip_normal", "skip_plane", "taps_0", "taps_some", "taps_4",
            "blended", "capped")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(w, h, name, hostile=True, stats=None):
    """the outs of a sequence, with its frames"""
    fr, win, prm = tc.frames(w, h, name, hostile)
    hist = tr.History()
    outs = [tr.step(E, P, N, hist, cam, w, h, win[0], win[1], prm, stats) for cam, E, P, N, _, _ in fr]
    return outs, fr, prm


@pytest.fixture(scope="module")
def big_runs():
    runs = {}
    for w, h in tc.BIG:
        for name in tc.sequences(w, h):
            st = {}
            runs[(w, h, name)] = _run(w, h, name, True, st) + (st,)
    return runs


@pytest.mark.parametrize("w,h", tc.BIG)
def test_every_outcome_occurs_in_every_big_frame_size(big_runs, w, h):
    total = {}
    for (ww, hh, name), (_, _, _, st) in big_runs.items():
        if (ww, hh) == (w, h):
            for k, v in st.items():
                total[k] = total.get(k, 0) + v
    for key in OUTCOMES:
        assert total.get(key, 0) > 0, (w, h, key, total)


def test_the_sequences_meet_what_they_are_named_for(big_runs):
    for (w, h, name), (_, _, _, st) in big_runs.items():
        what = "%dx%d %s: %r" % (w, h, name, st)
        assert st["miss"] > 0 and st["empty_history"] > 0 and st["blended"] > 0, what
        if name == "static":
            assert st["capped"] > 0 and st["taps_4"] > 0, what
        if name == "pan":
            assert st["outside"] > 0 and st["skip_window"] > 0 and st["skip_plane"] > 0 and st["skip_normal"] > 0 and st["skip_invalid"] > 0, what
        if name == "hostile_previous":
            assert st["behind"] > 0 and st["outside"] > 0, what


def test_hostile_previous_cameras_reject_every_pixel(big_runs):
    """the frames whose PREVIOUS camera is turned away (2; and 1, which is turned away from its predecessor), has a singular basis (6) or a
    zero viewplane (8) find nothing to take: out = (E, 1 | 0); the frames around the camera that is only not orthonormal do blend"""
    for w, h in tc.BIG:
        outs, fr, _ = big_runs[(w, h, "hostile_previous")][:3]
        for k in (1, 2, 6, 8):
            E, P = fr[k][1], fr[k][2]
            np.testing.assert_array_equal(_bits(outs[k][..., :3]), _bits(E))
            np.testing.assert_array_equal(outs[k][..., 3], (P[..., 3] != 0).astype(np.float32))
        for k in (3, 4):
            assert (outs[k][..., 3] > 1).any(), (w, h, k)


def test_the_sentinel_never_leaks(big_runs):
    for key, (outs, fr, _, _) in big_runs.items():
        for out, (_, E, P, _, _, _) in zip(outs, fr):
            hit = P[..., 3] != 0
            np.testing.assert_array_equal(_bits(out[~hit][:, :3]), _bits(E[~hit]))
            assert (out[~hit][:, 3] == 0).all()
            assert not (np.abs(out[hit][:, :3]) > 1e3).any(), key
            assert (out[hit][:, 3] >= 1).all(), key


@pytest.mark.parametrize("w,h,name", tc.all_sequences())
def test_a_reset_history_gives_the_input(w, h, name):
    fr, win, prm = tc.frames(w, h, name)
    hist = tr.History()
    for k, (cam, E, P, N, _, _) in enumerate(fr[:2]):
        if k == 1:
            hist.reset()
        out = tr.step(E, P, N, hist, cam, w, h, win[0], win[1], prm)
        np.testing.assert_array_equal(_bits(out[..., :3]), _bits(E))
        np.testing.assert_array_equal(out[..., 3], (P[..., 3] != 0).astype(np.float32))


def test_another_window_is_a_reset():
    w, h = 45, 37
    fr, win, prm = tc.frames(w, h, "dolly_window")
    cam, E, P, N = fr[0][:4]
    hist = tr.History()
    tr.step(E, P, N, hist, cam, w, h, win[0], win[1], prm)
    E2, P2, N2 = tc.frame(cam, w, h, win[0] + 1, win[1] + 1, 3)[:3]
    st = {}
    out = tr.step(E2, P2, N2, hist, cam, w, h, win[0] + 1, win[1] + 1, prm, st)
    assert st["empty_history"] > 0 and "blended" not in st
    np.testing.assert_array_equal(_bits(out[..., :3]), _bits(E2))
    assert hist.geom == (w, h, win[0] + 1, win[1] + 1)


def test_alpha_one_keeps_no_history_and_the_length_still_grows(big_runs):
    outs, fr, prm, _ = big_runs[(64, 64, "pan_alpha_one")]
    assert prm == tc.ALPHA_ONE
    out, E = outs[2], fr[2][1]
    took = out[..., 3] > 1
    assert took.any() and (out[..., 3] == 3).any()
    with np.errstate(all="ignore"):
        assert np.nanmax(np.abs(out[took][:, :3] - E[took])) < 1e-5   # (Eh + 1 * (E - Eh): E up to a rounding)


def test_the_length_is_capped(big_runs):
    for w, h in tc.BIG:
        outs, _, prm, _ = big_runs[(w, h, "static")]
        assert prm[1] == 3 and outs[3][..., 3].max() == 3 and outs[2][..., 3].max() == 3 and outs[1][..., 3].max() == 2


def _rmse(a, b, m):
    return float(np.sqrt(np.mean((a[m].astype(np.float64) - b[m]) ** 2)))


@pytest.mark.parametrize("kind,prm", [("pan", (0.125, 8, 0.5, 0.9)), ("static", (0.1, 32, 0.5, 0.9))])
def test_rmse_against_the_noise_free_base_halves_in_eight_frames(kind, prm):
    """independent noise per frame, max_len >= 8 and alpha_min <= 1/8: averaging 8 samples gives 1 / sqrt(8) = 0.354 of one frame's error;
    the bound is 0.5.  Pixels that are ordinary hits in the eighth frame, on frames without the hostile guides."""
    w, h = 45, 37
    c0 = tc.look_at(tc.EYE, tc.TARGET, w, h)
    cams = [tc.yaw(c0, 0.6 * k, w) if kind == "pan" else c0 for k in range(8)]
    hist = tr.History()
    for k, cam in enumerate(cams):
        E, P, N, base, clean = tc.frame(cam, w, h, 0, h, 100 + k, hostile=False)
        out = tr.step(E, P, N, hist, cam, w, h, 0, h, prm)
    one = _rmse(E, base, clean)
    acc = _rmse(out[..., :3], base, clean)
    print("%s: rmse of one frame %.4f, accumulated %.4f, ratio %.3f" % (kind, one, acc, acc / one))
    assert 0.8 * tc.NOISE < one < 1.2 * tc.NOISE
    assert acc < 0.5 * one, (kind, one, acc)


def test_the_reciprocal_basis_inverts_an_orthonormal_camera():
    c = tc.look_at(tc.EYE, tc.TARGET, 64, 64)
    Rr, Ur, Fr = tr.reciprocal_basis(c)
    for got, want in ((Rr, c[6:9]), (Ur, c[9:12]), (Fr, c[3:6])):
        np.testing.assert_allclose(got, want, atol=1e-6)
    with np.errstate(all="ignore"):
        assert not np.isfinite(np.concatenate(tr.reciprocal_basis(tc.singular(c)))).any()


def test_a_static_pixel_reprojects_onto_itself():
    """an identical previous camera: fx, fy land within a hundredth of a pixel of the pixel's own centre"""
    w, h = 64, 64
    fr, win, prm = tc.frames(w, h, "static", hostile=False)
    cam, E, P, N = fr[0][:4]
    hist = tr.History()
    tr.step(E, P, N, hist, cam, w, h, 0, h, prm)
    Rr, Ur, Fr = tr.reciprocal_basis(cam)
    d = P[..., :3] - cam[0:3]
    hit = P[..., 3] != 0
    with np.errstate(all="ignore"):
        fx = ((d @ Rr) / (d @ Fr) / cam[12] + 0.5) * w - 0.5
        fy = ((d @ Ur) / (d @ Fr) / cam[13] + 0.5) * h - 0.5
    ys, xs = np.mgrid[0:h, 0:w]
    assert np.abs(fx - xs)[hit].max() < 0.01 and np.abs(fy - ys)[hit].max() < 0.01


# ---- the path frame with temporal accumulation ----
def test_the_path_sequence_takes_and_rejects_history(po, vrt):
    """scenes.mirror_hall over the orbit step, the dolly and the cut of tests/test_gpu_temporal.py: every frame after the first blends, every
    tap condition occurs, the cut puts most of the hall outside or behind the previous camera, and the length reaches its cap"""
    import denoise_cases as dc
    import scenes
    hall = scenes.mirror_hall(vrt)
    cams = [np.array(vrt.rtapi.look_at(e, tc.PATH_CENTRE, (0.0, 1.0, 0.0), 1.0, dc.W, dc.H).cam14(), np.float32) for e in tc.PATH_EYES]
    spp, bounces, shadow, seed = dc.PATH_CONFIGS[0]
    hist = tr.History()
    total = {}
    for k, cam in enumerate(cams):
        st = {}
        out = tr.path_frame(hall, cam, dc.W, dc.H, po.shade_params(), spp, bounces, seed + k, shadow, dc.PATH_DN, tc.PATH_TP, hist, stats=st)
        assert np.isfinite(out["col"]).all()
        if k == 0:
            assert st["empty_history"] > 0 and "blended" not in st
            plain = __import__("denoise_ref").path_frame(hall, cam, dc.W, dc.H, po.shade_params(), spp, bounces, seed, shadow, dc.PATH_DN)
            np.testing.assert_array_equal(_bits(out["col"]), _bits(plain["col"]))     # (the first frame is the denoised frame)
            np.testing.assert_array_equal(out["px"], plain["px"])
        else:
            assert st["blended"] > 0 and (_bits(out["T"][..., :3]) != _bits(out["E"])).any(), (k, st)
        if k == 3:
            assert st["behind"] > 0 and st["outside"] > st["blended"] and st["capped"] > 0, st
        for key, v in st.items():
            total[key] = total.get(key, 0) + v
    for key in OUTCOMES:
        assert total.get(key, 0) > 0, (key, total)
