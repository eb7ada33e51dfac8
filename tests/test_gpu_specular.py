"""GPU: path frames with specular vertices (vxrt_render_path_frame_specular) and the lobe pick alone (vxrt_specular_pick), bit for bit
against the restatement tests/specular_ref.py -- pixels, colours, rays traced -- and through the three identities of the header's
"Specular vertices" against the GPU's own vxrt_render_path_frame and vxrt_render_camera.  No masks, no tolerances; guard words behind
every output.  tests/test_specular_cpu.py pins the restatement and shows that the cases (tests/specular_cases.py) are not vacuous."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import path_frame_cases as fc
import path_frame_ref as fr
import path_ref as pr
import specular_cases as sc
import specular_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = sc.W, sc.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
FMARK = -12345.5
GUARD = 64
CHILD = os.environ.get("VXRT_SPECULAR_TEST_CHILD") == "1"
SPP, BOUNCES, SEED = sc.CONFIG
f32 = np.float32


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _u32(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(dev)


def _outputs(dev, w=W, h=H):
    import torch
    o = {"px": torch.full((h * w + GUARD,), MARK, dtype=torch.int32, device=dev), "cnt": torch.full((1 + GUARD,), MARK, dtype=torch.int64, device=dev),
         "col": torch.full((h * w * 3 + GUARD,), FMARK, dtype=torch.float32, device=dev)}
    o["cnt"][0] = 0
    return o


def _host(o, w=W, h=H):
    import torch
    torch.cuda.synchronize()
    px, cnt, col = o["px"].cpu().numpy(), o["cnt"].cpu().numpy(), o["col"].cpu().numpy()
    assert (px[h * w:] == MARK).all() and (cnt[1:] == MARK).all() and (col[h * w * 3:] == f32(FMARK)).all(), "a guard word was written"
    return {"px": px[:h * w].view(np.uint32).reshape(h, w), "cnt": int(cnt[0]), "col": col[:h * w * 3].reshape(h, w, 3)}


def _form(R, form, scale=sc.SCALE):
    if form == "mis":
        return None, R.EmissiveMisParams(float(scale), (C.c_uint32 * 3)(0, 0, 0))
    if form in ("nee0", "nee1"):
        return R.EmissiveParams(int(form == "nee1"), float(scale), (C.c_uint32 * 2)(0, 0)), None
    assert form is None
    return None, None


def _descriptor(vrt, o, cam, w, h, spp, bounces, seed, shadow, form=None, counts=None, y0=0, y1=None):
    R = vrt.rtapi
    em, mis = _form(R, form)
    return R.PathFrame(w, h, y0, h if y1 is None else y1, R.default_shade_params(), R.PathParams(spp, bounces, seed & 0xFFFFFFFF, shadow), o["px"].data_ptr(),
                       cam=cam, emissive=em, emissive_mis=mis, counts=None if counts is None else counts.data_ptr(), colors=o["col"].data_ptr(),
                       rays_traced=o["cnt"].data_ptr())


def _render(vrt, ds, cam, spp, bounces, seed, shadow, w=W, h=H, out=None, stream=None, specular=1, **parts):
    """vxrt_render_path_frame_specular (specular = None: vxrt_render_path_frame) into fresh outputs (or `out`)"""
    o = out or _outputs(ds.device, w, h)
    sp = None if specular is None else vrt.rtapi.SpecularParams(specular)
    vrt.rtapi.render_path_frame(ds.accel, _descriptor(vrt, o, cam, w, h, spp, bounces, seed, shadow, **parts), _stream() if stream is None else stream, specular=sp)
    return o


def _check(got, want, what, h=H, y0=0, y1=None):
    """the outputs against the restatement's dict over rows [y0, y1): bit for bit, a NaN of the restatement asks for a NaN"""
    y1 = h if y1 is None else y1
    g, wc = np.ascontiguousarray(got["col"][y0:y1], np.float32), np.ascontiguousarray(want["col"], np.float32)
    nan = np.isnan(wc)
    assert np.isnan(g[nan]).all(), what
    np.testing.assert_array_equal(g.view(np.uint32)[~nan], wc.view(np.uint32)[~nan], err_msg=what + ": colours")
    np.testing.assert_array_equal(got["px"][y0:y1], want["px"], err_msg=what + ": pixels")
    assert (got["px"][:y0] == MARK).all() and (got["px"][y1:] == MARK).all(), what + ": a row outside the window was written"
    assert got["cnt"] == want["rays"], "%s: rays traced %d, restatement %d" % (what, got["cnt"], want["rays"])


def _identical(a, b, what):
    assert a["cnt"] == b["cnt"], "%s: rays traced %d and %d" % (what, a["cnt"], b["cnt"])
    for k in ("px", "col"):
        np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32), err_msg="%s: %s" % (what, k))


@pytest.fixture(autouse=True)
def _status_is_clean(vrt):
    yield
    assert vrt.rtapi.status(_stream()) == 0


def _scene(vrt, gpu_device, b, pairs):
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    ds.set_emitters(pairs)
    return ds


@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    b, pairs = sc.hall(vrt)
    ds = _scene(vrt, gpu_device, b, pairs)
    yield b, ds, pairs
    ds.close()


# ---- 1: the frame against the restatement ----
@pytest.mark.parametrize("shadow", [0, 1])
@pytest.mark.parametrize("form", sc.FORMS)
def test_frame_is_the_restatement(vrt, po, hall, form, shadow):
    b, ds, pairs = hall
    em = fc.emitter(form, b, pairs, sc.SCALE)
    for name, cam in (("framing", csr.framing(W, H)), ("fixed", None)):
        got = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, shadow, form=form))
        _check(got, sr.frame(b, cam, W, H, po.shade_params(), SPP, BOUNCES, SEED, shadow, em), "%r shadow %d %s" % (form, shadow, name))


def test_odd_size_and_row_window(vrt, po, hall):
    b, ds, pairs = hall
    w, h, (y0, y1) = sc.ODD_W, sc.ODD_H, sc.ODD_ROWS
    cam = csr.framing(w, h)
    got = _host(_render(vrt, ds, cam, 3, 2, 11, 1, w, h, form="mis", y0=y0, y1=y1), w, h)
    _check(got, sr.frame(b, cam, w, h, po.shade_params(), 3, 2, 11, 1, fc.emitter("mis", b, pairs, sc.SCALE), y0=y0, y1=y1), "13 x 7 rows", h, y0, y1)


def test_sixteen_bounces(vrt, po, hall):
    b, ds, pairs = hall
    spp, bounces, seed = sc.DEEP
    cam = csr.framing(W, H)
    got = _host(_render(vrt, ds, cam, spp, bounces, seed, 0, form="nee1"))
    _check(got, sr.frame(b, cam, W, H, po.shade_params(), spp, bounces, seed, 0, fc.emitter("nee1", b, pairs, sc.SCALE)), "16 bounces")


# ---- 2: counts, and the batches of both tails (these run again in the child process of test_small_batches) ----
def test_batches_counts_tail_mosaic_and_restatement(vrt, po, hall):
    """counts of 1, between, the cap and above it, with MIS: every pixel is the GPU's own uniform specular frame of its count, and the
    frame is the restatement's, rays traced included"""
    b, ds, pairs = hall
    cam, case = csr.framing(W, H), sc.COUNTS
    raw = sc.counts_of()
    got = _host(_render(vrt, ds, cam, case["cap"], case["bounces"], case["seed"], case["shadow"], form="mis", counts=_u32(ds.device, raw)))
    n_p = ar.clamp(raw, case["cap"])
    assert set(np.unique(n_p)) == {1, 3, 4}
    want_px, want_col = np.zeros_like(got["px"]), np.zeros_like(got["col"])
    for v in np.unique(n_p):
        u = _host(_render(vrt, ds, cam, int(v), case["bounces"], case["seed"], case["shadow"], form="mis"))
        want_px[n_p == v], want_col[n_p == v] = u["px"][n_p == v], u["col"][n_p == v]
    np.testing.assert_array_equal(got["col"].view(np.uint32), want_col.view(np.uint32), err_msg="mosaic: colours")
    np.testing.assert_array_equal(got["px"], want_px, err_msg="mosaic: pixels")
    _check(got, sr.frame(b, cam, W, H, po.shade_params(), case["cap"], case["bounces"], case["seed"], case["shadow"], fc.emitter("mis", b, pairs, sc.SCALE), raw),
           "counts")


@pytest.mark.parametrize("form", [None, "nee1"])
def test_batches_uniform_tail_five_samples(vrt, po, hall, form):
    b, ds, pairs = hall
    cam = csr.framing(W, H)
    got = _host(_render(vrt, ds, cam, sc.CHILD_SPP, 2, 3, 1, form=form))
    _check(got, sr.frame(b, cam, W, H, po.shade_params(), sc.CHILD_SPP, 2, 3, 1, fc.emitter(form, b, pairs, sc.SCALE)), "5 spp %r" % form)


def test_small_batches(vrt):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs the tests above with CHILD_BATCH paths per batch -- spp = 5 of 192
    pixels in whole samples of 2, 2, 1 for the uniform tail, and for the counts tail batches of 400 consecutive paths whose boundaries
    fall inside pixels.  The knob line the library prints under VXRT_DEBUG shows that the child took it."""
    assert not CHILD
    env = dict(os.environ, VXRT_PATH_BATCH=str(sc.CHILD_BATCH), VXRT_SPECULAR_TEST_CHILD="1", VXRT_DEBUG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "test_batches"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "3 passed" in r.stdout and ("path_batch=%d " % sc.CHILD_BATCH) in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 3: the identities, through the C ABI ----
@pytest.mark.parametrize("form", sc.FORMS)
def test_identity_a_hidden_mirror(vrt, gpu_device, form):
    b, pairs = sc.hidden_mirror_hall(vrt)
    ds = _scene(vrt, gpu_device, b, pairs)
    try:
        for cam, shadow in ((csr.framing(W, H), 1), (None, 0)):
            got = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, shadow, form=form))
            _identical(got, _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, shadow, form=form, specular=None)), "A %r" % form)
        if form == "mis":
            cts = _u32(ds.device, sc.counts_of())
            got = _host(_render(vrt, ds, csr.framing(W, H), sc.COUNTS["cap"], BOUNCES, SEED, 1, form=form, counts=cts))
            _identical(got, _host(_render(vrt, ds, csr.framing(W, H), sc.COUNTS["cap"], BOUNCES, SEED, 1, form=form, counts=cts, specular=None)), "A counts")
    finally:
        ds.close()


@pytest.mark.parametrize("form", sc.FORMS)
def test_identity_b_no_bounces(vrt, hall, form):
    b, ds, pairs = hall
    cam = csr.framing(W, H)
    _identical(_host(_render(vrt, ds, cam, 4, 0, 3, 1, form=form)), _host(_render(vrt, ds, cam, 4, 0, 3, 1, form=form, specular=None)), "B %r" % form)
    cts = _u32(ds.device, sc.counts_of())
    _identical(_host(_render(vrt, ds, cam, 4, 0, 3, 1, form=form, counts=cts)), _host(_render(vrt, ds, cam, 4, 0, 3, 1, form=form, counts=cts, specular=None)), "B counts")


@pytest.mark.parametrize("shadow", [0, 1])
def test_identity_c_perfect_mirrors(vrt, gpu_device, shadow):
    import torch
    R = vrt.rtapi
    b, pairs = sc.hall(vrt, (1.0, 1.0))
    ds = _scene(vrt, gpu_device, b, pairs)
    try:
        rec = b["blas"].view(np.float32).reshape(-1, 40)
        p = R.default_shade_params()
        p.max_depth = 2
        seen = 0
        for cam in (csr.framing(W, H), fc.cameras(vrt, 1, W, H)[0]):
            got = _host(_render(vrt, ds, cam, 4, 1, 9, shadow))
            px = torch.zeros(H * W, dtype=torch.int32, device=gpu_device)
            col = torch.zeros(H * W * 3, dtype=torch.float32, device=gpu_device)
            R.render_camera(ds.accel, cam, W, H, 0, H, p, px.data_ptr(), shadow=shadow, colors_ptr=col.data_ptr(), stream=_stream())
            torch.cuda.synchronize()
            h0 = pr.primary(b, cr.rays(cam, W, H))["hits"].reshape(H, W)
            m = (h0["dist"] != cr.LARGE) & (rec[h0["blasIdx"] & 0x7fffffff, 38] == f32(1.0))
            assert m.sum() >= 10
            np.testing.assert_array_equal(got["col"][m].view(np.uint32), col.cpu().numpy().reshape(H, W, 3)[m].view(np.uint32))
            np.testing.assert_array_equal(got["px"][m], px.cpu().numpy().view(np.uint32).reshape(H, W)[m])
            seen += int(m.sum())
        assert seen >= 20
    finally:
        ds.close()


# ---- 4: the pick alone ----
def test_specular_pick(vrt, gpu_device):
    import torch
    v, seeds = sc.pick_vertices()
    n = len(v)
    dv, dseeds = torch.from_numpy(v.reshape(-1)).to(gpu_device), _u32(gpu_device, seeds)
    rays = torch.full((n * 6 + GUARD,), FMARK, dtype=torch.float32, device=gpu_device)
    lobe = torch.full((n + GUARD,), MARK, dtype=torch.int32, device=gpu_device)
    vrt.rtapi.specular_pick(n, dv.data_ptr(), dseeds.data_ptr(), rays.data_ptr(), lobe.data_ptr(), _stream())
    torch.cuda.synchronize()
    gr, gl = rays.cpu().numpy(), lobe.cpu().numpy()
    assert (gr[n * 6:] == f32(FMARK)).all() and (gl[n:] == MARK).all()
    wr, wl = sr.pick_step(v, seeds)
    np.testing.assert_array_equal(gl[:n].view(np.uint32), wl)
    np.testing.assert_array_equal(gr[:n * 6].view(np.uint32), wr.reshape(-1).view(np.uint32))
    L = vrt.rtapi._lib()
    assert L.vxrt_specular_pick(n, None, dseeds.data_ptr(), rays.data_ptr(), lobe.data_ptr(), _stream()) == -1
    assert L.vxrt_specular_pick(2 ** 31, dv.data_ptr(), dseeds.data_ptr(), rays.data_ptr(), lobe.data_ptr(), _stream()) == -1
    assert L.vxrt_specular_pick(0, dv.data_ptr(), dseeds.data_ptr(), rays.data_ptr(), lobe.data_ptr(), _stream()) == 0


# ---- 5: two frames in flight, one specular and one not ----
def test_two_frames_in_flight(vrt, po, hall):
    import torch
    b, ds, pairs = hall
    dev, p = ds.device, po.shade_params()
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cams = [csr.framing(W, H), fc.cameras(vrt, 1, W, H)[0]]
        cfg = [dict(form="mis", specular=1), dict(form="nee1", specular=None)]
        outs = [_outputs(dev) for _ in range(2)]
        torch.cuda.synchronize()
        for rnd in range(2):      # (the second round finds the contexts' buffers grown: no synchronisation at all)
            for i in range(2):
                _render(vrt, ds, cams[i], SPP, BOUNCES, SEED + i, 1, out=outs[i], stream=streams[i].cuda_stream, **cfg[i])
            torch.cuda.synchronize()
            if rnd == 0:
                outs = [_outputs(dev) for _ in range(2)]
                torch.cuda.synchronize()
        _check(_host(outs[0]), sr.frame(b, cams[0], W, H, p, SPP, BOUNCES, SEED, 1, fc.emitter("mis", b, pairs, sc.SCALE)), "in flight, specular")
        _check(_host(outs[1]), fr.frame(b, cams[1], W, H, p, SPP, BOUNCES, SEED + 1, 1, fc.emitter("nee1", b, pairs, sc.SCALE)), "in flight, not specular")
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)


# ---- 6: refusals, and what enable = 0 is ----
def test_refusals_leave_everything_untouched(vrt, gpu_device):
    import torch
    R = vrt.rtapi
    L = R._lib()
    b, pairs = sc.hall(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    try:
        o = _outputs(gpu_device)
        cam = csr.framing(W, H)
        aux = torch.zeros(W * H * 4, dtype=torch.float32, device=gpu_device)

        def call(sp, edit=None, **parts):
            d = _descriptor(vrt, o, cam, W, H, SPP, BOUNCES, SEED, 1, **parts)
            if edit:
                edit(d)
            return L.vxrt_render_path_frame_specular(ds.accel, C.byref(d), None if sp is None else C.byref(sp), _stream())

        def setter(**kw):
            def edit(d):
                d._more = list(kw.values())
                for k, v in kw.items():
                    setattr(d, k, v)
            return edit
        assert call(R.SpecularParams(2)) == -1 and call(R.SpecularParams(0xFFFFFFFF)) == -1
        for k in range(3):
            for enable in (0, 1):
                sp = R.SpecularParams(enable)
                sp.reserved[k] = 1
                assert call(sp) == -1
        on = R.SpecularParams(1)
        dn, tp, vp = R.DenoiseParams(*fc.DN), R.TemporalParams(*fc.TP), R.VarianceParams(*fc.VP, 0)
        aov = R.PathAov(aux.data_ptr(), None, None, None, None)
        with R.History(W, H) as hp, R.History(W, H, moments=True) as hm:
            chain = dict(denoise=C.pointer(dn), temporal=C.pointer(tp), history=hp.handle)
            assert call(on, setter(denoise=C.pointer(dn))) == -1
            assert call(on, setter(denoise=C.pointer(dn), aov=C.pointer(aov))) == -1 and call(on, setter(aov=C.pointer(aov))) == -1
            assert call(on, setter(**chain)) == -1
            assert call(on, setter(temporal=C.pointer(tp))) == -1 and call(on, setter(history=hp.handle)) == -1
            assert call(on, setter(motion=1)) == -1 and call(on, setter(motion=1, **chain)) == -1
            assert call(on, setter(denoise=C.pointer(dn), temporal=C.pointer(tp), history=hm.handle, variance=C.pointer(vp))) == -1
            assert call(on, setter(variance=C.pointer(vp))) == -1
            assert L.vxrt_history_read(hp.handle, aux.data_ptr(), _stream()) == -1 and L.vxrt_history_read(hm.handle, aux.data_ptr(), _stream()) == -1
        # everything vxrt_render_path_frame refuses
        assert call(on, setter(size=0)) == -1 and call(on, setter(path=None)) == -1 and call(on, setter(dst=None)) == -1 and call(on, setter(y1=H + 1)) == -1
        rsv = (C.c_uint32 * 4)(0, 0, 1, 0)
        assert call(on, setter(reserved=rsv)) == -1
        assert call(on, form="nee1") == -1 and call(on, form="mis") == -1                     # no table yet
        assert L.vxrt_render_path_frame_specular(None, None, C.byref(on), _stream()) == -1
        ds.set_emitters(pairs)
        both = _form(R, "mis")[1]
        assert call(on, setter(emissive_mis=C.pointer(both)), form="nee1") == -1
        bad = R.PathParams(2, R.PATH_MAX_BOUNCES + 1, 0, 1)
        assert call(on, setter(path=C.pointer(bad))) == -1
        got = _host(o)
        assert (got["px"] == MARK).all() and got["cnt"] == 0 and (got["col"] == f32(FMARK)).all()
        assert R.status(_stream()) == 0
        assert call(on, setter(y0=5, y1=5), form="mis") == 0                                  # the empty window
        assert (_host(o)["px"] == MARK).all()
        assert call(on, form="mis") == 0
        assert (_host(o)["px"] != MARK).all()
    finally:
        ds.close()


def test_alpha_table_and_stale_accel_are_refused(vrt, golden, gpu_device):
    import torch
    import scenes
    import shading_ref
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in KEYS}, gpu_device)
    on = vrt.rtapi.SpecularParams(1)
    L = vrt.rtapi._lib()
    try:
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), shading_ref.MAT_DT)
        o = _outputs(gpu_device)
        d = _descriptor(vrt, o, csr.golden_cameras(vrt, W, H)["g_orbit_1"], W, H, SPP, BOUNCES, SEED, 1)
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert L.vxrt_render_path_frame_specular(ds.accel, C.byref(d), C.byref(on), _stream()) == -1
        assert (_host(o)["px"] == MARK).all()
        ds.set_alpha_test(None)
        assert L.vxrt_render_path_frame_specular(ds.accel, C.byref(d), C.byref(on), _stream()) == 0
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
        d = _descriptor(vrt, o, csr.framing(W, H), W, H, SPP, BOUNCES, SEED, 1)
        assert L.vxrt_render_path_frame_specular(ds.accel, C.byref(d), C.byref(on), _stream()) == -1
        assert (_host(o)["px"] == MARK).all()
    finally:
        ds.close()


@pytest.mark.parametrize("form", [None, "mis"])
def test_disabled_is_the_frame_of_today_and_leaves_it_alone(vrt, po, hall, form):
    """enable = 0 and a null part are vxrt_render_path_frame; and that call on the same descriptor is what it was after a specular frame
    on the same context, whose per-path buffers the two share"""
    b, ds, pairs = hall
    cam = csr.framing(W, H)
    before = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, 1, form=form, specular=None))
    _check(before, fr.frame(b, cam, W, H, po.shade_params(), SPP, BOUNCES, SEED, 1, fc.emitter(form, b, pairs, sc.SCALE)), "today's frame")
    _identical(_host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, 1, form=form, specular=0)), before, "enable = 0")
    o = _outputs(ds.device)
    d = _descriptor(vrt, o, cam, W, H, SPP, BOUNCES, SEED, 1, form=form)
    assert vrt.rtapi._lib().vxrt_render_path_frame_specular(ds.accel, C.byref(d), None, _stream()) == 0
    _identical(_host(o), before, "a null part")
    spec = _host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, 1, form=form))
    assert (spec["px"] != before["px"]).sum() * 4 >= W * H
    _identical(_host(_render(vrt, ds, cam, SPP, BOUNCES, SEED, 1, form=form, specular=None)), before, "after a specular frame")
