"""CPU: the restatement of path frames by descriptor (tests/path_frame_ref.py) is, where no emitter form is named, each of the
restatements it composes, bit for bit; with an emitter form on a scene that does not emit it is the frame without one; and the cases
of tests/test_gpu_path_frame.py (tests/path_frame_cases.py) are not vacuous.  No GPU."""
import numpy as np
import pytest

import adaptive_ref as ar
import camera_ref as cr
import denoise_ref as dr
import emissive_cases as ec
import motion_cases as moc
import motion_ref as mr
import path_frame_cases as fc
import path_frame_ref as fr
import path_ref as pr
import temporal_ref as tr
import variance_ref as vr

W, H = fc.W, fc.H
SPP, BOUNCES, SHADOW, SEED = fc.CONFIG


@pytest.fixture(scope="module")
def hall(vrt):
    return fc.hall(vrt)


def _same(got, want, what):
    """every entry of the dict `want` is in `got`, bit for bit"""
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(v)
            assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s" % (what, k)
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg="%s: %s" % (what, k))
        else:
            assert got[k] == v, "%s: %s" % (what, k)


def _moving(b):
    """[(scene of frame k, the snapshot it is rendered with)] of three frames: the blob moves as in tests/motion_cases.py"""
    out, prev = [], b
    for k in range(3):
        cur = b if k == 0 else mr.moved(b, moc.BLOB, moc.translation(k)[None])
        out.append((cur, mr.snapshot(prev)))
        prev = cur
    return out


# ---- without an emitter form the layer is the restatement of each existing entry point ----
def test_is_the_path_and_the_denoised_frame(vrt, po, hall):
    b, _ = hall
    cam = fc.cameras(vrt)[0]
    p = po.shade_params()
    px, col, n, _ = pr.frame(b, cam, W, H, p, SPP, BOUNCES, SEED, SHADOW)
    _same(fr.frame(b, cam, W, H, p, SPP, BOUNCES, SEED, SHADOW), {"px": px, "col": col, "rays": n}, "path")
    for dn in (fc.DN, (0,) + tuple(fc.DN[1:])):
        _same(fr.frame(b, cam, W, H, p, SPP, BOUNCES, SEED, SHADOW, dn=dn, y0=8, y1=40), dr.path_frame(b, cam, W, H, p, SPP, BOUNCES, SEED, SHADOW, dn, 8, 40),
              "denoised %r" % (dn,))


def test_is_the_adaptive_frame(vrt, po, hall):
    b, _ = hall
    cam = fc.cameras(vrt)[0]
    case = fc.COUNTS
    raw = fc.counts_of(case)
    px, col, n = ar.frame(b, cam, W, H, po.shade_params(), raw, case["cap"], case["bounces"], case["seed"], case["shadow"])
    _same(fr.frame(b, cam, W, H, po.shade_params(), case["cap"], case["bounces"], case["seed"], case["shadow"], counts=raw), {"px": px, "col": col, "rays": n},
          "adaptive")


def test_is_the_temporal_and_the_motion_frames(vrt, po, hall):
    b, _ = hall
    p = po.shade_params()
    ha, hb, hc, hd = tr.History(), tr.History(), tr.History(), tr.History()
    for k, ((cur, snap), cam) in enumerate(zip(_moving(b), fc.cameras(vrt))):
        _same(fr.frame(cur, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, dn=fc.DN, tp=fc.TP, hist=ha),
              tr.path_frame(cur, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, fc.DN, fc.TP, hb), "temporal frame %d" % k)
        _same(fr.frame(cur, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, dn=fc.DN, tp=fc.TP, hist=hc, motion=1, snap=snap),
              mr.path_frame(cur, snap, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, fc.DN, fc.TP, hd), "motion frame %d" % k)
    _same({"HE": ha.HE, "HP": ha.HP}, {"HE": hb.HE, "HP": hb.HP}, "the history")
    assert (ha.HE[..., 3] > 1).any()


@pytest.mark.parametrize("motion", (0, 1))
def test_is_the_variance_and_the_variance_adaptive_frames(vrt, po, hall, motion):
    b, _ = hall
    p = po.shade_params()
    case = fc.VARIANCE_COUNTS
    ha, hb, hc, hd = vr.History(), vr.History(), vr.History(), vr.History()
    for k, ((cur, snap), cam) in enumerate(zip(_moving(b), fc.cameras(vrt))):
        _same(fr.frame(cur, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, dn=fc.DN, tp=fc.TP, hist=ha, motion=motion, snap=snap, vp=fc.VP),
              vr.path_frame(cur, snap, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, fc.DN, fc.TP, fc.VP, hb, motion), "variance frame %d" % k)
        raw = fc.counts_of(case, salt=20 + k)
        _same(fr.frame(cur, cam, W, H, p, case["cap"], case["bounces"], case["seed"] + k, case["shadow"], counts=raw, dn=fc.DN, tp=fc.TP, hist=hc, motion=motion,
                       snap=snap, vp=fc.VP),
              ar.variance_frame(cur, snap, cam, W, H, p, raw, case["cap"], case["bounces"], case["seed"] + k, case["shadow"], fc.DN, fc.TP, fc.VP, hd, motion),
              "variance-adaptive frame %d" % k)
    assert (ha.h.HE[..., 3] > 1).any()


# ---- an emitter form on a scene without emissive materials adds nothing ----
def test_brute_force_form_on_a_dark_scene_is_the_frame_without_it(vrt, po):
    b, _ = ec.hall(vrt, emissive=False)
    p = po.shade_params()
    ha, hb, hc = vr.History(), vr.History(), vr.History()
    for k, cam in enumerate(fc.cameras(vrt, 2)):
        got = fr.frame(b, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, emitter=("nee0", fc.SCALE), dn=fc.DN, tp=fc.TP, hist=ha, vp=fc.VP)
        _same(got, fr.frame(b, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, dn=fc.DN, tp=fc.TP, hist=hb, vp=fc.VP), "dark hall frame %d" % k)
        _same(got, vr.path_frame(b, None, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, fc.DN, fc.TP, fc.VP, hc), "vxrt_render_path_variance, frame %d" % k)


# ---- the GPU cases are not vacuous ----
@pytest.mark.parametrize("form", fc.FORMS)
def test_cases_are_not_vacuous(vrt, po, hall, form):
    b, pairs = hall
    p = po.shade_params()
    em = fc.emitter(form, b, pairs)
    for k, cam in enumerate(fc.cameras(vrt)):
        # pixels whose primary hit emits: D != Lit_0 there, and nowhere else
        D, A, P, N, prim = fr.guides(b, cam, W, H, p, SHADOW, em)
        D0 = dr.path_guides(b, cam, W, H, p, SHADOW, prim=prim)[0]
        emits = np.zeros(W * H, bool)
        fi = np.nonzero(prim["hits"]["dist"] != cr.LARGE)[0]
        emits[fi] = fr.er.emission(b, prim["hits"][fi], fc.SCALE)[0]
        differs = (D.view(np.uint32) != D0.view(np.uint32)).any(-1).reshape(-1)
        assert emits.sum() > 100 and (differs == emits).all(), "frame %d: primary hits that emit" % k
        # depth 0 alone (bounces = 1): an unblocked, a blocked and a skipped emitter ray; MIS bounce hits with 0 < wB < 1
        info = {}
        fr.colour(b, cam, W, H, p, SPP, 1, SEED + k, SHADOW, em, prim=prim, info=info)
        if form == "nee0":
            assert info["bounce_emissive"] > 100
        else:
            assert min(info["unblocked"], info["blocked"], info["skipped"]) > 100, info
        if form == "mis":
            assert info["wB_between"] > 100 and info["wE_below_one"] > 100
        # the a-trous passes of the frame reject taps and accept taps
        stats = {}
        out = fr.frame(b, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, em, dn=fc.DN, stats=stats)
        rejected = stats["skip_weight"] + stats["low_dn"] + stats["low_wz"] + stats["low_wc"]
        assert stats["taps"] > 10000 and rejected > 10000 and stats["skip_miss"] > 1000, stats
        assert (out["col"].view(np.uint32) != out["noisy"].view(np.uint32)).any()
        # the filter sees the emitter rays of h_0: E differs from the frame's without the form
        plain = fr.frame(b, cam, W, H, p, SPP, BOUNCES, SEED + k, SHADOW, None, dn=fc.DN)
        assert (out["E"].view(np.uint32) != plain["E"].view(np.uint32)).any()


@pytest.mark.parametrize("case", [fc.COUNTS], ids=["counts"])
def test_samples_straddle_the_child_batches(vrt, hall, case):
    """under VXRT_PATH_BATCH = CHILD_BATCH: pixels whose samples are in two batches, a short last batch whose live count is no multiple of
    64, and batches past the end (the host issues them for cap * pixels paths)"""
    b, _ = hall
    hit = pr.primary(b, cr.rays(fc.cameras(vrt)[0], W, H))["hits"]["dist"] != cr.LARGE
    n_p = ar.clamp(fc.counts_of(case), case["cap"])
    assert set(np.unique(fc.counts_of(case)[hit.reshape(H, W)])) >= {0, 1, case["cap"], case["cap"] + 5}   # below 1, 1, the cap, above it
    cnt, off, total = ar.offsets(n_p, hit)
    assert 0 < hit.sum() < W * H and fc.CHILD_BATCH < 256 and fc.CHILD_BATCH % 64 != 0
    issued = -(-(W * H * case["cap"]) // fc.CHILD_BATCH)
    used = -(-total // fc.CHILD_BATCH)
    assert len(ar.straddlers(cnt, off, fc.CHILD_BATCH)) > 10
    assert used > 5 and total % fc.CHILD_BATCH != 0 and (total % fc.CHILD_BATCH) % 64 != 0 and issued > used
