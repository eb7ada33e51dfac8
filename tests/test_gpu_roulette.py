"""GPU: Russian roulette in path frames (vxrt_render_path_frame_ex, vxrt_roulette), bit for bit: every case of tests/roulette_cases.py
against the restatement tests/roulette_ref.py -- pixels, colours, rays traced, the guide outputs, the history -- the identities of the
definition against the GPU's own vxrt_render_path_frame, the step alone on hostile throughputs, every refusal with everything
pre-marked, small batches in a child process and two frames in flight.  No masks, no tolerances (a NaN of the restatement asks for a
NaN); guard words behind every output.  tests/test_roulette_cpu.py pins the restatement and shows that the cases are not vacuous."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_secondary_ref as csr
import emissive_cases as ec
import path_frame_cases as fc
import path_frame_ref as fr
import roulette_cases as rc
import roulette_ref as rr
import variance_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = rc.W, rc.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
FMARK = -12345.5
GUARD = 64
CHILD = os.environ.get("VXRT_ROULETTE_TEST_CHILD") == "1"
AOV = (("noisy", 3), ("direct", 3), ("albedo", 3), ("position", 4), ("normal", 4))
FLOATS = (("col", 3),) + AOV + (("var", 1), ("hist", 4), ("mom", 2))
f32 = np.float32


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _u32(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(dev)


def _outputs(dev, w=W, h=H):
    """every output a frame can have, each with GUARD marked words behind it"""
    import torch
    o = {"px": torch.full((h * w + GUARD,), MARK, dtype=torch.int32, device=dev), "cnt": torch.full((1 + GUARD,), MARK, dtype=torch.int64, device=dev)}
    o["cnt"][0] = 0
    for k, c in FLOATS:
        o[k] = torch.full((h * w * c + GUARD,), FMARK, dtype=torch.float32, device=dev)
    return o


def _host(o, w=W, h=H):
    """the outputs on the host, frame-shaped (hist, mom: flat, window-addressed); the guard words must be untouched"""
    import torch
    torch.cuda.synchronize()
    px, cnt = o["px"].cpu().numpy(), o["cnt"].cpu().numpy()
    assert (px[h * w:] == MARK).all() and (cnt[1:] == MARK).all(), "a guard word was written"
    out = {"px": px[:h * w].view(np.uint32).reshape(h, w), "cnt": int(cnt[0])}
    for k, c in FLOATS:
        a = o[k].cpu().numpy()
        assert (a[h * w * c:] == f32(FMARK)).all(), "a guard word of %s was written" % k
        out[k] = a[:h * w * c] if k in ("hist", "mom") else a[:h * w * c].reshape((h, w, c) if c > 1 else (h, w))
    return out


def _form(R, form, scale=rc.SCALE):
    if form == "mis":
        return None, R.EmissiveMisParams(float(scale), (C.c_uint32 * 3)(0, 0, 0))
    if form in ("nee0", "nee1"):
        return R.EmissiveParams(int(form == "nee1"), float(scale), (C.c_uint32 * 2)(0, 0)), None
    assert form is None
    return None, None


def _descriptor(vrt, o, cam, w, h, case, form=None, counts=None, dn=None, tp=None, hist=None, vp=None, y0=0, y1=None):
    R = vrt.rtapi
    em, mis = _form(R, form)
    return R.PathFrame(w, h, y0, h if y1 is None else y1, R.default_shade_params(), R.PathParams(case["spp"], case["bounces"], case["seed"], case["shadow"]),
                       o["px"].data_ptr(), cam=cam, emissive=em, emissive_mis=mis, counts=None if counts is None else counts.data_ptr(),
                       denoise=None if dn is None else R.DenoiseParams(*dn), aov=R.PathAov(*[o[n].data_ptr() for n, _ in AOV]) if dn is not None else None,
                       temporal=None if tp is None else R.TemporalParams(*tp), history=hist, variance=None if vp is None else R.VarianceParams(*vp, 0),
                       colors=o["col"].data_ptr(), variance_out=o["var"].data_ptr() if vp is not None else None, rays_traced=o["cnt"].data_ptr())


def _roulette(vrt, case, enable=1):
    return vrt.rtapi.RouletteParams(enable, case["first"], case["q_min"])


def _render(vrt, ds, cam, case, w=W, h=H, roulette="case", out=None, stream=None, **parts):
    """vxrt_render_path_frame_ex with the case's roulette part (roulette = None: vxrt_render_path_frame) into fresh outputs (or `out`); a
    history is read behind the frame on the same stream"""
    o = out or _outputs(ds.device, w, h)
    s = _stream() if stream is None else stream
    vrt.rtapi.render_path_frame(ds.accel, _descriptor(vrt, o, cam, w, h, case, **parts), s, roulette=_roulette(vrt, case) if roulette == "case" else roulette)
    hist = parts.get("hist")
    if hist is not None:
        hist.read(o["hist"].data_ptr(), s)
        if hist.moments:
            hist.read_moments(o["mom"].data_ptr(), s)
    return o


def _same_floats(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what + ": a NaN of the restatement is not a NaN"
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=what)


def _identical(a, b, what):
    assert a["cnt"] == b["cnt"], "%s: rays traced %d and %d" % (what, a["cnt"], b["cnt"])
    for k in a:
        if k != "cnt":
            np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32), err_msg="%s: %s" % (what, k))


def _check(got, want, what, w=W, h=H, y0=0, y1=None):
    """the outputs against the restatement's dict: what it holds is compared over rows [y0, y1), what it lacks must be untouched"""
    y1 = h if y1 is None else y1
    rows = slice(y0, y1)
    _same_floats(got["col"][rows], want["col"], what + ": colours")
    np.testing.assert_array_equal(got["px"][rows], want["px"], err_msg=what + ": pixels")
    assert (got["px"][:y0] == MARK).all() and (got["px"][y1:] == MARK).all(), what + ": a row outside the window was written"
    assert got["cnt"] == want["rays"], "%s: rays traced %d, restatement %d" % (what, got["cnt"], want["rays"])
    for k, key in [(n, n) for n, _ in AOV] + [("var", "variance")]:
        if key in want:
            _same_floats(got[k][rows], want[key], what + ": " + key)
        else:
            assert (got[k] == f32(FMARK)).all(), what + ": %s was written" % key
    n = (y1 - y0) * w
    for k, key, c in (("hist", "T", 4), ("mom", "M", 2)):
        if key in want:
            _same_floats(got[k][:n * c].reshape(y1 - y0, w, c), want[key], what + ": the history's " + key)
            assert (got[k][n * c:] == f32(FMARK)).all()


def _untouched(o, w=W, h=H):
    got = _host(o, w, h)
    return (got["px"] == MARK).all() and got["cnt"] == 0 and all((got[k] == f32(FMARK)).all() for k, _ in FLOATS)


@pytest.fixture(autouse=True)
def _status_is_clean(vrt):
    yield
    assert vrt.rtapi.status(_stream()) == 0


def _scene(vrt, gpu_device, make):
    b, pairs = make(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    ds.set_emitters(pairs)
    return b, ds, pairs


@pytest.fixture(scope="module")
def dark(vrt, gpu_device):
    """(scene buffers, DeviceScene with the emitter table set, pairs) of the dark hall"""
    b, ds, pairs = _scene(vrt, gpu_device, rc.dark)
    yield b, ds, pairs
    ds.close()


@pytest.fixture(scope="module")
def white(vrt, gpu_device):
    b, ds, pairs = _scene(vrt, gpu_device, rc.white)
    yield b, ds, pairs
    ds.close()


# ---- 1: the cases against the restatement.  name -> (scene, case, emitter form, counts?, camera, odd window?) ----
CASES = {
    "case_a": ("dark", rc.A, None, False, "hall", True),
    "case_b_cam": ("dark", rc.B, None, False, "hall", True),
    "case_b_inside": ("dark", rc.B, None, False, "inside_blob", True),
    "case_c": ("white", rc.C, None, False, "hall", False),
    "case_d_equal": ("dark", rc.D[0], None, False, "hall", False),
    "case_d_16": ("dark", rc.D[1], None, False, "hall", False),
    "case_e": ("dark", rc.E, None, False, "hall", False),
    "case_f_nee0": ("dark", rc.F, "nee0", False, "hall", False),
    "case_f_nee1": ("dark", rc.F, "nee1", False, "hall", False),
    "case_f_mis": ("dark", rc.F, "mis", False, "hall", False),
    "case_g_none": ("dark", rc.G, None, True, "hall", False),
    "case_g_mis": ("dark", rc.G, "mis", True, "hall", False),
}


def _camera(vrt, name, w, h):
    return rc.cameras(vrt, 1, w, h)[0] if name == "hall" else csr.hall_cameras(vrt, w, h)[name]


def _run_case(vrt, po, scenes, name, roulette="case"):
    """(the GPU's outputs, the restatement's dict, the window) of a case; roulette = None: the same frame without roulette, both sides"""
    which, case, form, with_counts, cam_name, odd = CASES[name]
    b, ds, pairs = scenes[which]
    w, h, (y0, y1) = (rc.ODD_W, rc.ODD_H, rc.ODD_ROWS) if odd else (W, H, (0, H))
    cam = _camera(vrt, cam_name, w, h)
    raw = rc.counts_of(w, h) if with_counts else None
    got = _host(_render(vrt, ds, cam, case, w, h, roulette, form=form, counts=None if raw is None else _u32(ds.device, raw), y0=y0, y1=y1), w, h)
    want = rr.frame(b, cam, w, h, po.shade_params(), case["spp"], case["bounces"], case["seed"], case["shadow"], fc.emitter(form, b, pairs), raw,
                    None if roulette is None else (case["first"], case["q_min"]), y0=y0, y1=y1)
    return got, want, (w, h, y0, y1)


@pytest.mark.parametrize("name", list(CASES))
def test_frame_against_the_restatement(vrt, po, dark, white, name):
    """pixels, colours and rays traced of every case; the child process of test_small_batches runs (a), (b) and (g) again"""
    got, want, (w, h, y0, y1) = _run_case(vrt, po, {"dark": dark, "white": white}, name)
    _check(got, want, name, w, h, y0, y1)
    assert got["cnt"] > (y1 - y0) * w


def test_case_h_the_variance_chain_on_one_history(vrt, po, dark):
    """two frames of a moving camera with emitter sampling and roulette on ONE history with moments: the guide outputs, the variance
    and the history's contents besides"""
    b, ds, pairs = dark
    case, ref = rc.HH, vr.History()
    em = fc.emitter(case["form"], b, pairs)
    with vrt.rtapi.History(W, H, moments=True) as hist:
        for k, cam in enumerate(rc.cameras(vrt, 2)):
            c = dict(case, seed=case["seed"] + k)
            got = _host(_render(vrt, ds, cam, c, form=case["form"], dn=fc.DN, tp=fc.TP, vp=fc.VP, hist=hist))
            want = rr.frame(b, cam, W, H, po.shade_params(), c["spp"], c["bounces"], c["seed"], c["shadow"], em, None, (c["first"], c["q_min"]), fc.DN, fc.TP, ref,
                            vp=fc.VP)
            _check(got, want, "variance chain frame %d" % k)
        assert (want["T"][..., 3] > 1).any() and (want["variance"] > 0).any()


# ---- 2: the identities, each against vxrt_render_path_frame on the GPU ----
def test_enable_zero_and_a_null_part_are_the_descriptors_frame(vrt, dark):
    b, ds, pairs = dark
    R, L = vrt.rtapi, vrt.rtapi._lib()
    cam, case = rc.cameras(vrt)[0], rc.F
    for form, with_counts in ((None, False), ("mis", True)):
        counts = _u32(ds.device, rc.counts_of()) if with_counts else None
        plain = _host(_render(vrt, ds, cam, case, roulette=None, form=form, counts=counts, dn=fc.DN))
        off = _host(_render(vrt, ds, cam, case, roulette=_roulette(vrt, case, 0), form=form, counts=counts, dn=fc.DN))
        _identical(off, plain, "enable = 0, %r" % form)
        junk = R.RouletteParams(0, 99, float("nan"))          # (enable = 0: the rest of the part is not read)
        _identical(_host(_render(vrt, ds, cam, case, roulette=junk, form=form, counts=counts, dn=fc.DN)), plain, "enable = 0 with junk, %r" % form)
        o = _outputs(ds.device)
        d = _descriptor(vrt, o, cam, W, H, case, form=form, counts=counts, dn=fc.DN)
        assert L.vxrt_render_path_frame_ex(ds.accel, C.byref(d), None, None, _stream()) == 0
        _identical(_host(o), plain, "a null roulette part, %r" % form)
        o = _outputs(ds.device)
        d = _descriptor(vrt, o, cam, W, H, case, form=form, counts=counts, dn=fc.DN)
        assert L.vxrt_render_path_frame_ex(ds.accel, C.byref(d), C.byref(R.SpecularParams(0)), None, _stream()) == 0
        _identical(_host(o), plain, "a null roulette part beside specular enable = 0, %r" % form)
        assert plain["cnt"] > W * H
    # enable = 1 beside a specular part with enable = 0 is the roulette frame
    on = _host(_render(vrt, ds, cam, case))
    o = _outputs(ds.device)
    R.render_path_frame(ds.accel, _descriptor(vrt, o, cam, W, H, case), _stream(), specular=R.SpecularParams(0), roulette=_roulette(vrt, case))
    _identical(_host(o), on, "roulette beside specular enable = 0")
    assert on["cnt"] < _host(_render(vrt, ds, cam, case, roulette=None))["cnt"]


@pytest.mark.parametrize("name", ("case_c", "case_d_equal", "case_d_16", "case_e"))
def test_identity_cases_are_the_descriptors_frame(vrt, dark, white, name):
    """(c) max(Alb) >= 1 everywhere, (d) first >= bounces, (e) q_min = 1: vxrt_render_path_frame bit for bit, with every emitter form"""
    which, case, _, _, cam_name, _ = CASES[name]
    b, ds, pairs = {"dark": dark, "white": white}[which]
    cam = _camera(vrt, cam_name, W, H)
    for form in (None,) + rc.FORMS:
        plain = _host(_render(vrt, ds, cam, case, roulette=None, form=form))
        _identical(_host(_render(vrt, ds, cam, case, form=form)), plain, "%s %r" % (name, form))
        assert plain["cnt"] > W * H


def test_fewer_rays_than_the_plain_frame(vrt, dark):
    """case (a): rays_traced is strictly below the plain frame's"""
    b, ds, pairs = dark
    w, h, (y0, y1) = rc.ODD_W, rc.ODD_H, rc.ODD_ROWS
    cam = _camera(vrt, "hall", w, h)
    with_rr = _host(_render(vrt, ds, cam, rc.A, w, h, y0=y0, y1=y1), w, h)
    plain = _host(_render(vrt, ds, cam, rc.A, w, h, roulette=None, y0=y0, y1=y1), w, h)
    print("case a: %d rays with roulette, %d without" % (with_rr["cnt"], plain["cnt"]))
    assert (y1 - y0) * w < with_rr["cnt"] < plain["cnt"]


# ---- 3: the step alone ----
@pytest.mark.parametrize("q_min", (0.05, 1.0, rc.Q_TINY, 0.5))
def test_the_step_alone_on_hostile_throughputs(vrt, gpu_device, q_min):
    import torch
    thr, seeds = rc.hostile(q_min)
    n = len(thr)
    want_t, want_a, _ = rr.step(thr, seeds, q_min)
    dt = torch.from_numpy(thr.copy()).to(gpu_device)
    dsd = _u32(gpu_device, seeds)
    out = torch.full((3 * n + GUARD,), FMARK, dtype=torch.float32, device=gpu_device)
    alive = torch.full((n + GUARD,), MARK, dtype=torch.int32, device=gpu_device)
    vrt.rtapi.roulette(n, dt.data_ptr(), dsd.data_ptr(), q_min, out.data_ptr(), alive.data_ptr(), _stream())
    torch.cuda.synchronize()
    o, a = out.cpu().numpy(), alive.cpu().numpy()
    assert (o[3 * n:] == f32(FMARK)).all() and (a[n:] == MARK).all()
    np.testing.assert_array_equal(a[:n].view(np.uint32), want_a)
    _same_floats(o[:3 * n].reshape(n, 3), want_t, "thr_out, q_min %r" % q_min)
    assert (dt.cpu().numpy().view(np.uint32) == thr.view(np.uint32)).all()                  # (the input is not written)
    # n that is no multiple of the workgroup, and n = 0
    out[:] = FMARK
    alive[:] = MARK
    vrt.rtapi.roulette(257, dt.data_ptr(), dsd.data_ptr(), q_min, out.data_ptr(), alive.data_ptr(), _stream())
    vrt.rtapi.roulette(0, dt.data_ptr(), dsd.data_ptr(), q_min, out.data_ptr() + 12 * 300, alive.data_ptr() + 4 * 300, _stream())
    torch.cuda.synchronize()
    o, a = out.cpu().numpy(), alive.cpu().numpy()
    assert (o[3 * 257:] == f32(FMARK)).all() and (a[257:] == MARK).all()
    np.testing.assert_array_equal(a[:257].view(np.uint32), want_a[:257])


# ---- 4: refusals ----
def test_refusals_leave_everything_untouched(vrt, gpu_device):
    import torch
    R = vrt.rtapi
    L = R._lib()
    b, ds, pairs = _scene(vrt, gpu_device, rc.dark)
    try:
        cam, case = rc.cameras(vrt)[0], rc.HH
        chain = dict(dn=fc.DN, tp=fc.TP, vp=fc.VP)
        with R.History(W, H, moments=True) as hist, R.History(W, H) as plain_hist:
            # one frame fills the history; its contents are the mark the refusals must leave
            filled = _host(_render(vrt, ds, cam, case, form="nee1", hist=hist, **chain))
            o = _outputs(gpu_device)

            def call(rp, specular=None, accel="own", frame="built", edit=None, **parts):
                d = _descriptor(vrt, o, parts.pop("cam", cam), W, H, parts.pop("case", case), **parts)
                if edit:
                    edit(d)
                return L.vxrt_render_path_frame_ex(ds.accel if accel == "own" else accel, None if frame is None else C.byref(d),
                                                   None if specular is None else C.byref(specular), None if rp is None else C.byref(rp), _stream())

            def setter(**kw):
                def edit(d):
                    for k, v in kw.items():
                        setattr(d, k, v)
                return edit

            def part(enable=1, first=2, q_min=0.05, reserved=0):
                p = R.RouletteParams(enable, first, q_min)
                p.reserved = reserved
                return p
            ok = part()
            full = dict(form="nee1", hist=hist, **chain)
            # the part itself, on a plain frame and on the frame with everything
            for bad in (part(enable=2), part(enable=0xFFFFFFFF), part(first=0), part(first=R.PATH_MAX_BOUNCES + 1), part(first=0xFFFFFFFF), part(q_min=0.0),
                        part(q_min=-0.0), part(q_min=-0.5), part(q_min=float(np.nextafter(f32(1.0), f32(2.0)))), part(q_min=2.0), part(q_min=float("nan")),
                        part(q_min=float("inf")), part(q_min=float("-inf")), part(reserved=1), part(reserved=0x80000000)):
                assert call(bad) == -1 and call(bad, **full) == -1, (bad.enable, bad.first, bad.q_min, bad.reserved)
                assert call(bad, edit=setter(y0=5, y1=5)) == -1                                      # (ahead of the empty window)
            # roulette with specular vertices: on purpose
            assert call(ok, R.SpecularParams(1)) == -1 and call(ok, R.SpecularParams(1), form="mis") == -1
            assert call(ok, R.SpecularParams(1), edit=setter(y0=5, y1=5)) == -1
            assert call(ok, R.SpecularParams(2)) == -1
            bad_spec = R.SpecularParams(0)
            bad_spec.reserved[1] = 1
            assert call(ok, bad_spec) == -1
            # everything vxrt_render_path_frame refuses
            assert call(ok, frame=None) == -1 and call(ok, accel=None) == -1
            assert call(ok, edit=setter(size=C.sizeof(R.PathFrame) - 8)) == -1
            rsv = (C.c_uint32 * 4)(0, 0, 1, 0)
            assert call(ok, edit=setter(reserved=rsv)) == -1
            assert call(ok, edit=setter(path=None)) == -1 and call(ok, edit=setter(params=None)) == -1 and call(ok, edit=setter(dst=None)) == -1
            assert call(ok, edit=setter(y0=5, y1=3)) == -1 and call(ok, edit=setter(y1=H + 1)) == -1 and call(ok, edit=setter(width=0)) == -1
            for bad in (dict(case, spp=0), dict(case, spp=4097), dict(case, bounces=R.PATH_MAX_BOUNCES + 1), dict(case, shadow=2)):
                assert call(ok, case=bad) == -1
            both = _form(R, "mis")[1]
            assert call(ok, form="nee1", edit=setter(emissive_mis=C.pointer(both))) == -1               # both emitter forms
            assert call(ok, form="nee1", edit=setter(emissive=C.pointer(R.EmissiveParams(2, 1.0, (C.c_uint32 * 2)(0, 0))))) == -1
            assert call(ok, dn=fc.DN, tp=fc.TP) == -1 and call(ok, tp=fc.TP, hist=plain_hist) == -1     # the chain's own rules
            assert call(ok, dn=fc.DN, tp=fc.TP, hist=hist) == -1 and call(ok, hist=plain_hist, **chain) == -1   # the kind of history
            assert call(ok, hist=hist, **dict(chain, vp=(0.0,) + tuple(fc.VP[1:]))) == -1
            assert call(ok, cam=None, hist=hist, **chain) == -1                                          # a history needs a camera
            assert call(ok, edit=setter(variance_out=o["var"].data_ptr()), dn=fc.DN) == -1              # variance_out without variance
            assert call(ok, edit=setter(motion=1), hist=hist, **chain) == -1                            # no motion snapshot
            ds.set_transforms([ec.lamp_transform()], first=ec.LAMP)                                      # a stale emitter table
            assert call(ok, **full) == -1 and call(ok, form="mis") == -1
            ds.set_emitters(pairs)
            assert call(ok, edit=setter(y0=7, y1=7), **full) == 0                                        # the empty window
            assert _untouched(o)
            hist.read(o["hist"].data_ptr(), _stream())
            hist.read_moments(o["mom"].data_ptr(), _stream())
            after = _host(o)
            np.testing.assert_array_equal(after["hist"].view(np.uint32), filled["hist"].view(np.uint32), err_msg="a refused frame changed the history")
            np.testing.assert_array_equal(after["mom"].view(np.uint32), filled["mom"].view(np.uint32), err_msg="a refused frame changed the moments")
            assert L.vxrt_history_read(plain_hist.handle, o["hist"].data_ptr(), _stream()) == -1         # still empty
            assert R.status(_stream()) == 0
            assert call(ok, **full) == 0                                                                 # and the frame that is allowed renders
            torch.cuda.synchronize()
            assert (_host(o)["px"] != MARK).all()
        # the step alone
        t = torch.zeros(30, dtype=torch.float32, device=gpu_device)
        s = torch.zeros(10, dtype=torch.int32, device=gpu_device)
        out = torch.full((30,), FMARK, dtype=torch.float32, device=gpu_device)
        al = torch.full((10,), MARK, dtype=torch.int32, device=gpu_device)
        args = [10, t.data_ptr(), s.data_ptr(), 0.05, out.data_ptr(), al.data_ptr(), _stream()]
        for k in (1, 2, 4, 5):
            bad = list(args)
            bad[k] = None
            assert L.vxrt_roulette(*bad) == -1
        for q in (0.0, -1.0, 1.5, float("nan"), float("inf")):
            assert L.vxrt_roulette(*(args[:3] + [q] + args[4:])) == -1
        assert L.vxrt_roulette(*([2 ** 31] + args[1:])) == -1 and L.vxrt_roulette(*([2 ** 40] + args[1:])) == -1
        assert L.vxrt_roulette(*([0] + args[1:])) == 0
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == f32(FMARK)).all() and (al.cpu().numpy() == MARK).all() and R.status(_stream()) == 0
    finally:
        ds.close()


# ---- 5: small batches, two frames in flight ----
def test_small_batches(vrt):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs cases (a), (b) and (g) with rc.CHILD_BATCH paths per batch -- batches
    of one sample each for the uniform tail, for the counts tail pixels that straddle batches and a short last batch -- and batches
    whose paths all die, whose later launches fall through on a live count of 0.  The knob line the library prints under VXRT_DEBUG
    shows that the child took it."""
    assert not CHILD
    env = dict(os.environ, VXRT_PATH_BATCH=str(rc.CHILD_BATCH), VXRT_ROULETTE_TEST_CHILD="1", VXRT_DEBUG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "case_a or case_b or case_g"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "5 passed" in r.stdout and ("path_batch=%d " % rc.CHILD_BATCH) in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_two_frames_in_flight(vrt, po, dark):
    """one frame with roulette (MIS, counts) and one without (emitter sampling, denoised) on two streams, twice: the second round finds
    the contexts' buffers grown"""
    import torch
    b, ds, pairs = dark
    dev, p = ds.device, po.shade_params()
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cams = rc.cameras(vrt, 2)
        raw = rc.counts_of(salt=1)
        cfg = [dict(roulette="case", form="mis", counts=_u32(dev, raw)), dict(roulette=None, form="nee1", dn=fc.DN)]
        cases = (rc.G, rc.F)
        outs = [_outputs(dev) for _ in range(2)]
        torch.cuda.synchronize()
        for rnd in range(2):
            for i in range(2):
                _render(vrt, ds, cams[i], cases[i], out=outs[i], stream=streams[i].cuda_stream, **cfg[i])
            torch.cuda.synchronize()
            if rnd == 0:
                outs = [_outputs(dev) for _ in range(2)]
                torch.cuda.synchronize()
        g, f = cases
        _check(_host(outs[0]), rr.frame(b, cams[0], W, H, p, g["spp"], g["bounces"], g["seed"], g["shadow"], fc.emitter("mis", b, pairs), raw, (g["first"], g["q_min"])),
               "in flight, with roulette")
        _check(_host(outs[1]), fr.frame(b, cams[1], W, H, p, f["spp"], f["bounces"], f["seed"], f["shadow"], fc.emitter("nee1", b, pairs), dn=fc.DN),
               "in flight, without")
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)
