"""GPU: path frames by descriptor (vxrt_render_path_frame), bit for bit: against the GPU's own entry points, each of which is the frame
with that entry point's parts; against the emissive frames through the identities of the definition (uniform, mosaic, a filter without
passes, a scene that does not emit); and against the restatement tests/path_frame_ref.py for what no entry point could name before --
an emitter form with the filter, a history, motion, variance guidance and counts.  No masks, no tolerances (a NaN of the restatement
asks for a NaN, as tests/test_gpu_variance.py); guard words behind every output.  tests/test_path_frame_cpu.py pins the restatement and
shows that the cases (tests/path_frame_cases.py) are not vacuous."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as ar
import camera_secondary_ref as csr
import emissive_cases as ec
import motion_cases as moc
import motion_ref as mr
import path_frame_cases as fc
import path_frame_ref as fr
import temporal_ref as tr
import variance_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = fc.W, fc.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
FMARK = -12345.5
GUARD = 64
CHILD = os.environ.get("VXRT_PATH_FRAME_TEST_CHILD") == "1"
SPP, BOUNCES, SHADOW, SEED = fc.CONFIG
AOV = (("noisy", 3), ("direct", 3), ("albedo", 3), ("position", 4), ("normal", 4))
FLOATS = (("col", 3),) + AOV + (("prev", 4), ("var", 1), ("hist", 4), ("mom", 2))
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


def _form(R, form, scale=fc.SCALE):
    """(emissive, emissive_mis) of an emitter form's name"""
    if form == "mis":
        return None, R.EmissiveMisParams(float(scale), (C.c_uint32 * 3)(0, 0, 0))
    if form in ("nee0", "nee1"):
        return R.EmissiveParams(int(form == "nee1"), float(scale), (C.c_uint32 * 2)(0, 0)), None
    assert form is None
    return None, None


def _descriptor(vrt, o, cam, w, h, spp, bounces, seed, shadow, form=None, counts=None, dn=None, aov=True, tp=None, hist=None, motion=0, vp=None, y0=0, y1=None):
    R = vrt.rtapi
    em, mis = _form(R, form)
    return R.PathFrame(w, h, y0, h if y1 is None else y1, R.default_shade_params(), R.PathParams(spp, bounces, seed & 0xFFFFFFFF, shadow), o["px"].data_ptr(),
                       cam=cam, emissive=em, emissive_mis=mis, counts=None if counts is None else counts.data_ptr(),
                       denoise=None if dn is None else R.DenoiseParams(*dn), aov=R.PathAov(*[o[n].data_ptr() for n, _ in AOV]) if dn is not None and aov else None,
                       temporal=None if tp is None else R.TemporalParams(*tp), history=hist, motion=motion,
                       variance=None if vp is None else R.VarianceParams(*vp, 0), colors=o["col"].data_ptr(),
                       prev_position=o["prev"].data_ptr() if motion else None, variance_out=o["var"].data_ptr() if vp is not None else None,
                       rays_traced=o["cnt"].data_ptr())


def _render(vrt, ds, cam, spp, bounces, seed, shadow, w=W, h=H, out=None, stream=None, **parts):
    """vxrt_render_path_frame into fresh outputs (or `out`); a history is read behind the frame on the same stream"""
    o = out or _outputs(ds.device, w, h)
    s = _stream() if stream is None else stream
    vrt.rtapi.render_path_frame(ds.accel, _descriptor(vrt, o, cam, w, h, spp, bounces, seed, shadow, **parts), s)
    hist = parts.get("hist")
    if hist is not None:
        hist.read(o["hist"].data_ptr(), s)
        if hist.moments:
            hist.read_moments(o["mom"].data_ptr(), s)
    return o


def _same_floats(got, want, what):
    """bit for bit, except that a NaN of the restatement asks for a NaN of any payload"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what + ": a NaN of the restatement is not a NaN"
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=what)


def _identical(a, b, what):
    """two sets of outputs of the GPU, every word of every buffer"""
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
    for k, key in [(n, n) for n, _ in AOV] + [("prev", "prev_position"), ("var", "variance")]:
        if key in want:
            _same_floats(got[k][rows], want[key], what + ": " + key)
        else:
            assert (got[k] == f32(FMARK)).all(), what + ": %s was written" % key
    n = (y1 - y0) * w
    for k, key, c in (("hist", "T", 4), ("mom", "M", 2)):
        if key in want:
            _same_floats(got[k][:n * c].reshape(y1 - y0, w, c), want[key], what + ": the history's " + key)
            assert (got[k][n * c:] == f32(FMARK)).all()


@pytest.fixture(autouse=True)
def _status_is_clean(vrt):
    yield
    assert vrt.rtapi.status(_stream()) == 0


@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    """(scene buffers, DeviceScene with the emitter table set, pairs)"""
    b, pairs = fc.hall(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    ds.set_emitters(pairs)
    yield b, ds, pairs
    ds.close()


@pytest.fixture()
def fresh(vrt, gpu_device):
    """a scene of its own for the tests that move it"""
    b, pairs = fc.hall(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    ds.set_emitters(pairs)
    yield b, ds, pairs
    ds.close()


# ---- 1: every existing entry point is the descriptor with its parts ----
def _entry_point(vrt, ds, name, o, cam, seed, counts, hist, motion):
    """the existing entry point `name` into the outputs o"""
    R = vrt.rtapi
    p, s = R.default_shade_params(), _stream()
    px, col, cnt = o["px"].data_ptr(), o["col"].data_ptr(), o["cnt"].data_ptr()
    dn, tp, vp = R.DenoiseParams(*fc.DN), R.TemporalParams(*fc.TP), R.VarianceParams(*fc.VP, 0)
    aov = R.PathAov(*[o[n].data_ptr() for n, _ in AOV])
    head = (ds.accel, cam, W, H, 0, H, p, SPP, BOUNCES)
    prev, var = o["prev"].data_ptr() if motion else None, o["var"].data_ptr()
    if name == "path":
        R.render_path(*head, px, seed, SHADOW, col, cnt, s)
    elif name == "denoised":
        R.render_path_denoised(*head, dn, px, seed, SHADOW, col, aov, cnt, s)
    elif name == "temporal":
        R.render_path_temporal(*head, dn, tp, hist, px, seed, SHADOW, col, aov, cnt, s)
    elif name == "temporal_motion":
        R.render_path_temporal_motion(*head, dn, tp, hist, px, seed, SHADOW, col, aov, prev, cnt, s)
    elif name == "variance":
        R.render_path_variance(*head, dn, tp, vp, hist, px, motion, seed, SHADOW, col, aov, prev, var, cnt, s)
    elif name == "adaptive":
        R.render_path_adaptive(*head, counts.data_ptr(), px, seed, SHADOW, col, cnt, s)
    elif name == "variance_adaptive":
        R.render_path_variance_adaptive(*head, counts.data_ptr(), dn, tp, vp, hist, px, motion, seed, SHADOW, col, aov, prev, var, cnt, s)
    elif name in ("emissive_nee0", "emissive_nee1"):
        R.render_path_emissive(*head, _form(R, name[9:])[0], px, seed, SHADOW, col, cnt, s)
    else:
        assert name == "emissive_mis"
        R.render_path_emissive_mis(*head, _form(R, "mis")[1], px, seed, SHADOW, col, cnt, s)
    if hist is not None:
        hist.read(o["hist"].data_ptr(), s)
        if hist.moments:
            hist.read_moments(o["mom"].data_ptr(), s)
    return o


# name -> (the descriptor's parts, moments of its history or None, motion values)
ENTRY_POINTS = {
    "path": ({}, None, (0,)),
    "denoised": ({"dn": fc.DN}, None, (0,)),
    "temporal": ({"dn": fc.DN, "tp": fc.TP}, False, (0,)),
    "temporal_motion": ({"dn": fc.DN, "tp": fc.TP}, False, (1,)),
    "variance": ({"dn": fc.DN, "tp": fc.TP, "vp": fc.VP}, True, (0, 1)),
    "adaptive": ({"counts": True}, None, (0,)),
    "variance_adaptive": ({"counts": True, "dn": fc.DN, "tp": fc.TP, "vp": fc.VP}, True, (0, 1)),
    "emissive_nee0": ({"form": "nee0"}, None, (0,)),
    "emissive_nee1": ({"form": "nee1"}, None, (0,)),
    "emissive_mis": ({"form": "mis"}, None, (0,)),
}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_descriptor_is_the_entry_point(vrt, fresh, name):
    """two frames of a moving camera and a moving blob through the entry point and through the descriptor, each on a history of its own:
    pixels, colours, rays traced, the guide outputs, prev_position, variance and the history's contents, where the form has them"""
    b, ds, pairs = fresh
    parts, moments, motions = ENTRY_POINTS[name]
    parts = dict(parts)
    counts = _u32(ds.device, fc.counts_of(fc.VARIANCE_COUNTS)) if parts.pop("counts", False) else None
    for motion in motions:
        ha = hb = None
        if moments is not None:
            ha, hb = vrt.rtapi.History(W, H, moments=moments), vrt.rtapi.History(W, H, moments=moments)
        try:
            for k, cam in enumerate(fc.cameras(vrt, 2)):
                if motion:
                    ds.snapshot_motion(mr.INSTANCES)
                    if k:
                        ds.set_transforms([moc.translation(k)], moc.BLOB)
                        ds.set_emitters(pairs)
                old = _host(_entry_point(vrt, ds, name, _outputs(ds.device), cam, SEED + k, counts, ha, motion))
                new = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED + k, SHADOW, counts=counts, hist=hb, motion=motion, **parts))
                _identical(new, old, "%s motion %d frame %d" % (name, motion, k))
                assert old["cnt"] > W * H and (old["px"] != MARK).all()
            if ha is not None:
                assert (old["hist"].reshape(H, W, 4)[..., 3] > 1).any()
        finally:
            if motion:
                ds.set_transforms([moc.translation(0)], moc.BLOB)
                ds.set_emitters(pairs)
            for hh in (ha, hb):
                if hh is not None:
                    hh.close()


def test_descriptor_is_the_entry_point_with_the_fixed_camera(vrt, hall):
    b, ds, _ = hall
    counts = _u32(ds.device, fc.counts_of(fc.COUNTS))
    for name in ("path", "denoised", "adaptive", "emissive_nee1", "emissive_mis"):
        parts = dict(ENTRY_POINTS[name][0])
        cts = counts if parts.pop("counts", False) else None
        old = _host(_entry_point(vrt, ds, name, _outputs(ds.device), None, SEED, cts, None, 0))
        _identical(_host(_render(vrt, ds, None, SPP, BOUNCES, SEED, SHADOW, counts=cts, **parts)), old, name + ", fixed camera")


# ---- 2: the identities of the definition, against the GPU's own emissive frames ----
def _emissive(vrt, ds, form, cam, spp, bounces, seed, shadow, w=W, h=H):
    """the uniform emissive frame of the existing entry point of `form`"""
    return _host(_entry_point_sized(vrt, ds, form, cam, spp, bounces, seed, shadow, w, h), w, h)


def _entry_point_sized(vrt, ds, form, cam, spp, bounces, seed, shadow, w, h):
    R = vrt.rtapi
    o = _outputs(ds.device, w, h)
    em, mis = _form(R, form)
    head = (ds.accel, cam, w, h, 0, h, R.default_shade_params(), spp, bounces)
    tail = (o["px"].data_ptr(), seed, shadow, o["col"].data_ptr(), o["cnt"].data_ptr(), _stream())
    if form == "mis":
        R.render_path_emissive_mis(*head, mis, *tail)
    else:
        R.render_path_emissive(*head, em, *tail)
    return o


@pytest.mark.parametrize("form", fc.FORMS)
def test_uniform_counts_are_the_emissive_frame(vrt, hall, form):
    b, ds, _ = hall
    cam = fc.cameras(vrt)[0]
    for spp, bounces, shadow in ((1, 1, 0), (3, 2, 1), (4, 0, 1)):
        counts = _u32(ds.device, np.full((H, W), spp, np.uint32))
        want = _emissive(vrt, ds, form, cam, spp, bounces, SEED, shadow)
        _identical(_host(_render(vrt, ds, cam, spp, bounces, SEED, shadow, form=form, counts=counts)), want, "%s spp %d bounces %d" % (form, spp, bounces))
        assert bounces == 0 or want["cnt"] > W * H


def test_filter_without_passes_and_history_is_the_emissive_frame(vrt, hall):
    b, ds, _ = hall
    cam = fc.cameras(vrt)[1]
    for form in fc.FORMS:
        want = _emissive(vrt, ds, form, cam, SPP, BOUNCES, SEED, SHADOW)
        got = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, SHADOW, form=form, dn=(0,) + tuple(fc.DN[1:])))
        assert got["cnt"] == want["cnt"]
        for k in ("px", "col"):
            np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg="%s: %s" % (form, k))
        np.testing.assert_array_equal(got["noisy"].view(np.uint32), want["col"].view(np.uint32))
        assert (got["direct"] != f32(FMARK)).all()


def test_dark_hall_with_the_brute_force_form_is_the_variance_frame(vrt, gpu_device):
    """no material emits: nee = 0 adds nothing anywhere, through the whole chain, history and moments included"""
    b, _ = ec.hall(vrt, emissive=False)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    try:
        with vrt.rtapi.History(W, H, moments=True) as ha, vrt.rtapi.History(W, H, moments=True) as hb:
            for k, cam in enumerate(fc.cameras(vrt, 2)):
                old = _host(_entry_point(vrt, ds, "variance", _outputs(ds.device), cam, SEED + k, None, ha, 0))
                new = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED + k, SHADOW, form="nee0", dn=fc.DN, tp=fc.TP, vp=fc.VP, hist=hb))
                _identical(new, old, "dark hall frame %d" % k)
    finally:
        ds.close()


# ---- 3: the counts tail with an emitter form; the child process of test_small_batches runs every test named counts_tail ----
def _mosaic(vrt, ds, form, cam, case, w=W, h=H):
    raw = fc.counts_of(case, w, h)
    got = _host(_render(vrt, ds, cam, case["cap"], case["bounces"], case["seed"], case["shadow"], w, h, form=form, counts=_u32(ds.device, raw)), w, h)
    n_p = ar.clamp(raw, case["cap"])
    want_px, want_col = np.zeros_like(got["px"]), np.zeros_like(got["col"])
    for v in np.unique(n_p):
        u = _emissive(vrt, ds, form, cam, int(v), case["bounces"], case["seed"], case["shadow"], w, h)
        want_px[n_p == v], want_col[n_p == v] = u["px"][n_p == v], u["col"][n_p == v]
    np.testing.assert_array_equal(got["col"].view(np.uint32), want_col.view(np.uint32), err_msg="%s mosaic: colours" % form)
    np.testing.assert_array_equal(got["px"], want_px, err_msg="%s mosaic: pixels" % form)
    return got, raw


@pytest.mark.parametrize("form", ("nee1", "mis"))
def test_counts_tail_mosaic_and_restatement(vrt, po, hall, form):
    """counts below 1, 1, between, the cap and above it: every pixel is the GPU's own uniform emissive frame of its count, and the frame
    is the restatement's, rays traced included"""
    b, ds, pairs = hall
    cam, case = fc.cameras(vrt)[0], fc.COUNTS
    got, raw = _mosaic(vrt, ds, form, cam, case)
    want = fr.frame(b, cam, W, H, po.shade_params(), case["cap"], case["bounces"], case["seed"], case["shadow"], fc.emitter(form, b, pairs), raw)
    _check(got, want, form + " counts")


def test_counts_tail_brute_force_form(vrt, po, hall):
    b, ds, pairs = hall
    cam, case = fc.cameras(vrt)[2], fc.COUNTS
    got, raw = _mosaic(vrt, ds, "nee0", cam, case)
    _check(got, fr.frame(b, cam, W, H, po.shade_params(), case["cap"], case["bounces"], case["seed"], case["shadow"], ("nee0", fc.SCALE), raw), "nee0 counts")


@pytest.mark.parametrize("form", ("nee1", "mis"))
def test_counts_tail_edges(vrt, po, hall, form):
    b, ds, pairs = hall
    em = fc.emitter(form, b, pairs)
    p = po.shade_params()
    case = fc.COUNTS
    # one pixel
    cam = csr.orbit(vrt, 1, 8, 1, 1)
    raw = np.full((1, 1), 3, np.uint32)
    got = _host(_render(vrt, ds, cam, case["cap"], 2, 5, 1, 1, 1, form=form, counts=_u32(ds.device, raw)), 1, 1)
    _check(got, fr.frame(b, cam, 1, 1, p, case["cap"], 2, 5, 1, em, raw), form + " 1x1", 1, 1)
    assert got["cnt"] > 1
    # every primary ray misses: the background, only the primary rays are counted
    w, h = 40, 24
    away = csr.hall_cameras(vrt, w, h)["far_cancel"]
    got = _host(_render(vrt, ds, away, case["cap"], 2, 5, 1, w, h, form=form, counts=_u32(ds.device, fc.counts_of(case, w, h))), w, h)
    assert got["cnt"] == w * h and (got["px"] == got["px"][0, 0]).all()
    _check(got, fr.frame(b, away, w, h, p, case["cap"], 2, 5, 1, em, fc.counts_of(case, w, h)), form + " all miss", w, h)
    # 16 bounces from inside the blob: whole batches die on the way
    w, h = 24, 16
    cam = csr.hall_cameras(vrt, w, h)["inside_blob"]
    raw = fc.counts_of({"values": (1, 2, 5)}, w, h)
    got = _host(_render(vrt, ds, cam, 2, 16, 0, 1, w, h, form=form, counts=_u32(ds.device, raw)), w, h)
    _check(got, fr.frame(b, cam, w, h, p, 2, 16, 0, 1, em, raw), form + " 16 bounces", w, h)


def test_small_batches(vrt):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs the counts-tail tests above with CHILD_BATCH paths per batch -- a
    capacity under one workgroup of the emitter-ray kernel, pixels whose samples straddle two batches, a short last batch whose live
    count is no multiple of 64 and empty trailing ones (tests/test_path_frame_cpu.py computes that from the offsets).  The knob line the
    library prints under VXRT_DEBUG shows that the child took it."""
    assert not CHILD
    env = dict(os.environ, VXRT_PATH_BATCH=str(fc.CHILD_BATCH), VXRT_PATH_FRAME_TEST_CHILD="1", VXRT_DEBUG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "counts_tail"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "5 passed" in r.stdout and ("path_batch=%d " % fc.CHILD_BATCH) in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 4: an emitter form with the filter chain, against the restatement ----
@pytest.mark.parametrize("form", fc.FORMS)
def test_denoised_frame(vrt, po, hall, form):
    b, ds, pairs = hall
    cam = fc.cameras(vrt)[0]
    got = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, SHADOW, form=form, dn=fc.DN))
    want = fr.frame(b, cam, W, H, po.shade_params(), SPP, BOUNCES, SEED, SHADOW, fc.emitter(form, b, pairs), dn=fc.DN)
    _check(got, want, form + " denoised")
    assert (want["direct"] != fr.frame(b, cam, W, H, po.shade_params(), 1, 0, 0, SHADOW, None, dn=fc.DN)["direct"]).any()


@pytest.mark.parametrize("form", fc.FORMS)
def test_temporal_frames(vrt, po, hall, form):
    b, ds, pairs = hall
    em, ref = fc.emitter(form, b, pairs), tr.History()
    with vrt.rtapi.History(W, H) as hist:
        for k, cam in enumerate(fc.cameras(vrt)):
            got = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED + k, SHADOW, form=form, dn=fc.DN, tp=fc.TP, hist=hist))
            want = fr.frame(b, cam, W, H, po.shade_params(), SPP, BOUNCES, SEED + k, SHADOW, em, dn=fc.DN, tp=fc.TP, hist=ref)
            _check(got, want, "%s temporal frame %d" % (form, k))
        assert (want["T"][..., 3] > 1).any()


@pytest.mark.parametrize("motion", (0, 1))
@pytest.mark.parametrize("form", fc.FORMS)
def test_variance_and_variance_adaptive_frames(vrt, po, fresh, form, motion):
    """three frames on ONE history with moments: two variance frames, then the variance frame with counts; the blob moves under them
    (motion = 1 reprojects through the snapshot; the blob emits nothing, so the table stays what it was, but it is set again as
    the definition asks)"""
    b, ds, pairs = fresh
    case, ref = fc.VARIANCE_COUNTS, vr.History()
    with vrt.rtapi.History(W, H, moments=True) as hist:
        prev = b
        for k, cam in enumerate(fc.cameras(vrt)):
            cur = b if k == 0 else mr.moved(b, moc.BLOB, moc.translation(k)[None])
            snap = mr.snapshot(prev)
            ds.snapshot_motion(mr.INSTANCES)
            if k:
                ds.set_transforms([moc.translation(k)], moc.BLOB)
                ds.set_emitters(pairs)
            raw = fc.counts_of(case, salt=20 + k) if k == 2 else None
            spp, bounces, seed, shadow = (case["cap"], case["bounces"], case["seed"] + k, case["shadow"]) if k == 2 else (SPP, BOUNCES, SEED + k, SHADOW)
            got = _host(_render(vrt, ds, cam, spp, bounces, seed, shadow, form=form, counts=None if raw is None else _u32(ds.device, raw), dn=fc.DN, tp=fc.TP,
                                vp=fc.VP, hist=hist, motion=motion))
            want = fr.frame(cur, cam, W, H, po.shade_params(), spp, bounces, seed, shadow, fc.emitter(form, cur, pairs), raw, fc.DN, fc.TP, ref, motion, snap, fc.VP)
            _check(got, want, "%s motion %d frame %d" % (form, motion, k))
            prev = cur
        assert (want["T"][..., 3] > 1).any() and (want["variance"] > 0).any()


@pytest.mark.parametrize("form", fc.FORMS)
def test_odd_size_and_row_window(vrt, po, hall, form):
    b, ds, pairs = hall
    em, p = fc.emitter(form, b, pairs), po.shade_params()
    w, h = 13, 7
    cam = fc.cameras(vrt, 1, w, h)[0]
    raw = fc.counts_of(fc.COUNTS, w, h)
    got = _host(_render(vrt, ds, cam, 4, BOUNCES, SEED, SHADOW, w, h, form=form, counts=_u32(ds.device, raw), dn=fc.DN), w, h)
    _check(got, fr.frame(b, cam, w, h, p, 4, BOUNCES, SEED, SHADOW, em, raw, fc.DN), form + " 13x7", w, h)
    cam, ref = fc.cameras(vrt)[1], vr.History()
    with vrt.rtapi.History(W, 30, moments=True) as hist:
        got = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, SHADOW, form=form, dn=fc.DN, tp=fc.TP, vp=fc.VP, hist=hist, y0=13, y1=43))
        want = fr.frame(b, cam, W, H, p, SPP, BOUNCES, SEED, SHADOW, em, None, fc.DN, fc.TP, ref, vp=fc.VP, y0=13, y1=43)
        _check(got, want, form + " rows 13..43", y0=13, y1=43)


# ---- 5: motion with emission ----
@pytest.mark.parametrize("form", ("nee1", "mis"))
def test_moved_lamp_needs_its_table_again(vrt, po, fresh, form):
    """frame 0, snapshot, the lamp's instance moves (set_transforms refits), the frame is refused while the table is stale, the
    emitters are set again, and frame 1 is the restatement's on the moved scene with the new table, motion = 1"""
    import torch
    b, ds, pairs = fresh
    cams, ref, p = fc.cameras(vrt, 2), tr.History(), po.shade_params()
    with vrt.rtapi.History(W, H) as hist:
        got = _host(_render(vrt, ds, cams[0], SPP, BOUNCES, SEED, SHADOW, form=form, dn=fc.DN, tp=fc.TP, hist=hist))
        _check(got, fr.frame(b, cams[0], W, H, p, SPP, BOUNCES, SEED, SHADOW, fc.emitter(form, b, pairs), dn=fc.DN, tp=fc.TP, hist=ref), form + " frame 0")
        ds.snapshot_motion(mr.INSTANCES)
        ds.set_transforms([fc.moved_lamp()], ec.LAMP)
        assert vrt.rtapi.accel_info(ds.accel, 7) == 0
        o = _outputs(ds.device)
        d = _descriptor(vrt, o, cams[1], W, H, SPP, BOUNCES, SEED + 1, SHADOW, form=form, dn=fc.DN, tp=fc.TP, hist=hist, motion=1)
        assert vrt.rtapi._lib().vxrt_render_path_frame(ds.accel, C.byref(d), _stream()) == -1
        before = _host(o)
        assert (before["px"] == MARK).all() and before["cnt"] == 0 and all((before[k] == f32(FMARK)).all() for k, _ in FLOATS)
        hist.read(o["hist"].data_ptr(), _stream())
        np.testing.assert_array_equal(_host(o)["hist"].view(np.uint32), got["hist"].view(np.uint32), err_msg="the refused frame changed the history")
        ds.set_emitters(pairs)
        cur = mr.moved(b, ec.LAMP, fc.moved_lamp()[None])
        got = _host(_render(vrt, ds, cams[1], SPP, BOUNCES, SEED + 1, SHADOW, form=form, dn=fc.DN, tp=fc.TP, hist=hist, motion=1))
        want = fr.frame(cur, cams[1], W, H, p, SPP, BOUNCES, SEED + 1, SHADOW, fc.emitter(form, cur, pairs), None, fc.DN, fc.TP, ref, 1, mr.snapshot(b))
        _check(got, want, form + " frame 1, lamp moved")
        seen = want["prev_position"][..., 3] != 0      # (the lamp's pixels: their surface point was LAMP_STEP away)
        assert ((np.abs(want["prev_position"][..., :3] - want["position"][..., :3]).max(-1) > 2.0) & seen).sum() > 10


# ---- 6: two frames in flight with different emitter forms ----
def test_two_frames_in_flight(vrt, po, hall):
    import torch
    b, ds, pairs = hall
    dev, p = ds.device, po.shade_params()
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cams = fc.cameras(vrt, 2)
        raws = [fc.counts_of(fc.COUNTS, salt=1), None]
        cts = [_u32(dev, raws[0]), None]
        cfg = [dict(form="mis", counts=cts[0]), dict(form="nee1", dn=fc.DN)]
        spps = (fc.COUNTS["cap"], SPP)
        outs = [_outputs(dev) for _ in range(2)]
        torch.cuda.synchronize()
        for rnd in range(2):      # (the second round finds the contexts' buffers grown: no synchronisation at all)
            for i in range(2):
                _render(vrt, ds, cams[i], spps[i], BOUNCES, SEED + i, SHADOW, out=outs[i], stream=streams[i].cuda_stream, **cfg[i])
            torch.cuda.synchronize()
            if rnd == 0:
                outs = [_outputs(dev) for _ in range(2)]
                torch.cuda.synchronize()
        _check(_host(outs[0]), fr.frame(b, cams[0], W, H, p, spps[0], BOUNCES, SEED, SHADOW, fc.emitter("mis", b, pairs), raws[0]), "in flight 0")
        _check(_host(outs[1]), fr.frame(b, cams[1], W, H, p, spps[1], BOUNCES, SEED + 1, SHADOW, fc.emitter("nee1", b, pairs), dn=fc.DN), "in flight 1")
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)


# ---- 7: refusals ----
def test_refusals_leave_everything_untouched(vrt, gpu_device):
    import torch
    R = vrt.rtapi
    L = R._lib()
    b, pairs = fc.hall(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    try:
        o = _outputs(gpu_device)
        cam = fc.cameras(vrt)[0]
        counts = _u32(gpu_device, np.full((H, W), 2, np.uint32))
        with R.History(W, H, moments=True) as hm, R.History(W, H) as hp, R.History(W, H // 2, moments=True) as small:
            def call(accel="own", frame="built", edit=None, **parts):
                d = _descriptor(vrt, o, parts.pop("cam", cam), W, H, SPP, BOUNCES, SEED, SHADOW, **parts)
                if edit:
                    edit(d)
                return L.vxrt_render_path_frame(ds.accel if accel == "own" else accel, None if frame is None else C.byref(d), _stream())

            def setter(**kw):
                def edit(d):
                    for k, v in kw.items():
                        setattr(d, k, v)
                return edit
            chain = dict(dn=fc.DN, tp=fc.TP, vp=fc.VP, hist=hm)
            # the descriptor itself
            assert call(frame=None) == -1
            assert call(edit=setter(size=C.sizeof(R.PathFrame) - 8)) == -1 and call(edit=setter(size=0)) == -1 and call(edit=setter(size=C.sizeof(R.PathFrame) + 8)) == -1
            for k in range(4):
                rsv = (C.c_uint32 * 4)(0, 0, 0, 0)
                rsv[k] = 1
                assert call(edit=setter(reserved=rsv)) == -1
            assert call(form="nee1") == -1 and call(form="mis") == -1                                     # no table yet
            assert call(form="nee0") == 0
            ds.set_emitters(pairs)
            both = _form(R, "mis")[1]
            assert call(form="nee1", edit=setter(emissive_mis=C.pointer(both))) == -1                     # both emitter forms
            assert call(edit=setter(motion=2), **chain) == -1 and call(motion=1, **chain) == -1            # motion > 1; no snapshot
            assert call(edit=setter(prev_position=o["prev"].data_ptr()), **chain) == -1                   # prev_position without motion
            assert call(dn=fc.DN, tp=fc.TP, hist=hp, edit=setter(variance_out=o["var"].data_ptr())) == -1  # variance_out without variance
            # what the entry points of the combination refuse
            assert call(edit=setter(path=None)) == -1 and call(edit=setter(params=None)) == -1 and call(edit=setter(dst=None)) == -1 and call(accel=None) == -1
            assert call(edit=setter(y0=5, y1=3)) == -1 and call(edit=setter(y1=H + 1)) == -1 and call(edit=setter(width=0)) == -1
            bad_cam = cam.copy()
            bad_cam[3] = float("nan")
            assert call(cam=bad_cam) == -1 and call(cam=None, **chain) == -1                              # a bad camera; a history needs one
            PP = R.PathParams
            for bad in (PP(0, 2, 0, 1), PP(4097, 2, 0, 1), PP(2, R.PATH_MAX_BOUNCES + 1, 0, 1), PP(2, 2, 0, 2)):
                assert call(edit=setter(path=C.pointer(bad))) == -1
            assert call(dn=fc.DN, tp=fc.TP) == -1 and call(dn=fc.DN, hist=hp) == -1                       # temporal and history: both or neither
            assert call(dn=fc.DN, tp=fc.TP, hist=hm) == -1 and call(dn=fc.DN, tp=fc.TP, vp=fc.VP, hist=hp) == -1   # the kind of history
            assert call(dn=fc.DN, tp=fc.TP, vp=fc.VP, hist=small) == -1                                   # ... and its size
            assert call(tp=fc.TP, hist=hp) == -1 and call(dn=fc.DN, edit=setter(denoise=None)) == -1      # the chain, and aov, without denoise
            assert call(dn=fc.DN, vp=fc.VP) == -1 and call(dn=fc.DN, edit=setter(motion=1)) == -1         # variance, motion without temporal
            assert call(dn=(7,) + tuple(fc.DN[1:])) == -1 and call(dn=fc.DN, tp=(0.0,) + tuple(fc.TP[1:]), hist=hp) == -1
            assert call(dn=fc.DN, tp=fc.TP, vp=(0.0,) + tuple(fc.VP[1:]), hist=hm) == -1
            for form, em in (("nee1", R.EmissiveParams(2, 1.0, (C.c_uint32 * 2)(0, 0))), ("nee1", R.EmissiveParams(1, -1.0, (C.c_uint32 * 2)(0, 0))),
                             ("nee1", R.EmissiveParams(1, 1.0, (C.c_uint32 * 2)(0, 1))), ("nee0", R.EmissiveParams(0, float("nan"), (C.c_uint32 * 2)(0, 0)))):
                assert call(form=form, edit=setter(emissive=C.pointer(em)), counts=counts, **chain) == -1
            for em in (R.EmissiveMisParams(float("inf"), (C.c_uint32 * 3)(0, 0, 0)), R.EmissiveMisParams(1.0, (C.c_uint32 * 3)(0, 0, 5))):
                assert call(form="mis", edit=setter(emissive_mis=C.pointer(em)), **chain) == -1
            # a stale table: a move, a refit
            ds.set_transforms([ec.lamp_transform()], first=ec.LAMP)
            assert call(form="nee1", counts=counts, **chain) == -1 and call(form="mis", dn=fc.DN) == -1 and call(form="nee0", dn=fc.DN) == 0
            o = _outputs(gpu_device)                                                                       # (the frames that were allowed wrote theirs)
            ds.set_emitters(pairs)
            ds.refit(geometry=True)
            assert call(form="mis", counts=counts) == -1
            ds.set_emitters(pairs)
            assert call(edit=setter(y0=7, y1=7), form="mis", **chain) == 0                                 # the empty window
            got = _host(o)
            assert (got["px"] == MARK).all() and got["cnt"] == 0 and all((got[k] == f32(FMARK)).all() for k, _ in FLOATS)
            assert L.vxrt_history_read(hm.handle, o["hist"].data_ptr(), _stream()) == -1                   # the histories are still empty
            assert L.vxrt_history_read(hp.handle, o["hist"].data_ptr(), _stream()) == -1
            assert R.status(_stream()) == 0
            assert call(form="mis", counts=counts, **chain) == 0
            torch.cuda.synchronize()
            assert (_host(o)["px"] != MARK).all()
    finally:
        ds.close()


def test_alpha_table_and_stale_accel_are_refused(vrt, golden, gpu_device):
    import torch
    import scenes
    import shading_ref as sr
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in KEYS}, gpu_device)
    try:
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        o = _outputs(gpu_device)
        cam = csr.golden_cameras(vrt)["g_orbit_1"]
        d = _descriptor(vrt, o, cam, W, H, SPP, BOUNCES, SEED, SHADOW, form="nee0", dn=fc.DN)
        call = lambda accel: vrt.rtapi._lib().vxrt_render_path_frame(accel, C.byref(d), _stream())
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1 and call(ds.accel) == -1
        assert (_host(o)["px"] == MARK).all()
        ds.set_alpha_test(None)
        assert call(ds.accel) == 0
        torch.cuda.synchronize()
    finally:
        ds.close()
    ds = vrt.tracer.DeviceScene(scenes.mirror_hall(vrt), gpu_device)
    try:
        v = ds.t["tri"].view(torch.float32).view(-1, 3, 3)
        v[0, 0, 0], v[1, 1, 0] = -3e38, 3e38   # the extent overflows fp32: the refit fails and leaves the accel stale
        with pytest.raises(Exception):
            ds.refit(geometry=True)
        o = _outputs(gpu_device)
        d = _descriptor(vrt, o, csr.framing(W, H), W, H, SPP, BOUNCES, SEED, SHADOW, form="nee0", dn=fc.DN)
        assert vrt.rtapi._lib().vxrt_render_path_frame(ds.accel, C.byref(d), _stream()) == -1
        assert (_host(o)["px"] == MARK).all()
    finally:
        ds.close()
