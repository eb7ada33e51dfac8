"""GPU: temporal accumulation (vxrt_temporal_accumulate, vxrt_history_*) and the path frame that uses it (vxrt_render_path_temporal)
against the restatement tests/temporal_ref.py, bit for bit: f32 as u32, pixels, rays traced, the guide outputs, the history after every
frame.  No masks, no tolerances, with one exception: where the restatement gives a NaN the kernel must give a NaN of any payload (x86 and
gfx950 generate different default NaNs).  tests/test_temporal_cpu.py shows that the cases (tests/temporal_cases.py) are not vacuous."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import scenes
import temporal_cases as tc
import temporal_ref as tr

pytestmark = pytest.mark.gpu
W, H = dc.W, dc.H
MARK = 0x5A5A5A
FMARK = -12345.5   # marker of float outputs
GUARD = 64         # floats past the end of out4
AOV = (("noisy", 3), ("direct", 3), ("albedo", 3), ("position", 4), ("normal", 4))
N_FRAMES = len(tc.PATH_EYES)
WINDOWS = ((0, H), dc.PATH_WINDOW)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_floats(got, want, what):
    """bit for bit, except that a NaN of the restatement asks for a NaN of any payload"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what + ": a NaN of the restatement is not a NaN"
    np.testing.assert_array_equal(_bits(got)[~nan], _bits(want)[~nan], err_msg=what)


@pytest.fixture(autouse=True)
def _status_is_clean(vrt):
    yield
    assert vrt.rtapi.status(_stream()) == 0


# ---- the step alone ----
def _device(dev, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in arrays]


def _out4(dev, n):
    import torch
    return torch.full((n * 4 + GUARD,), FMARK, dtype=torch.float32, device=dev)


def _accumulate(vrt, dev, hist, cam, w, h, win, E, P, N, prm):
    """vxrt_temporal_accumulate on device copies; returns out (rows, w, 4), the guard floats behind it and the history read back"""
    import torch
    rows = win[1] - win[0]
    t = _device(dev, E, P, N)
    out, rd = _out4(dev, rows * w), _out4(dev, rows * w)
    vrt.rtapi.temporal_accumulate(hist, cam, w, h, win[0], win[1], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), vrt.rtapi.TemporalParams(*prm),
                                  out.data_ptr(), _stream())
    hist.read(rd.data_ptr(), _stream())
    torch.cuda.synchronize()
    o, r = out.cpu().numpy(), rd.cpu().numpy()
    n4 = rows * w * 4
    assert (o[n4:] == np.float32(FMARK)).all() and (r[n4:] == np.float32(FMARK)).all(), "written past the end of out4"
    return o[:n4].reshape(rows, w, 4), r[:n4].reshape(rows, w, 4)


@pytest.mark.parametrize("w,h,name", tc.all_sequences())
def test_step_against_the_restatement(vrt, gpu_device, w, h, name):
    fr, win, prm = tc.frames(w, h, name)
    ref = tr.History()
    with vrt.rtapi.History(w, win[1] - win[0]) as hist:
        for k, (cam, E, P, N, _, _) in enumerate(fr):
            want = tr.step(E, P, N, ref, cam, w, h, win[0], win[1], prm)
            got, read = _accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm)
            what = "%dx%d %s frame %d" % (w, h, name, k)
            _same_floats(got, want, what)
            _same_floats(read, want, what + ": vxrt_history_read")


def test_reset_and_another_window_start_again(vrt, gpu_device):
    w, h = 45, 37
    fr, win, prm = tc.frames(w, h, "dolly_window")
    ref = tr.History()
    with vrt.rtapi.History(w, h) as hist:       # (room for every window of the frame)
        for k in range(2):
            cam, E, P, N = fr[k][:4]
            _same_floats(_accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm)[0], tr.step(E, P, N, ref, cam, w, h, win[0], win[1], prm), "frame %d" % k)
        hist.reset()
        ref.reset()
        cam, E, P, N = fr[2][:4]
        got = _accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm)[0]
        _same_floats(got, tr.step(E, P, N, ref, cam, w, h, win[0], win[1], prm), "after the reset")
        np.testing.assert_array_equal(_bits(got[..., :3]), _bits(E))
        win2 = (win[0] + 1, win[1] + 1)
        E2, P2, N2 = tc.frame(cam, w, h, win2[0], win2[1], 3)[:3]
        got = _accumulate(vrt, gpu_device, hist, cam, w, h, win2, E2, P2, N2, prm)[0]
        _same_floats(got, tr.step(E2, P2, N2, ref, cam, w, h, win2[0], win2[1], prm), "another window")
        np.testing.assert_array_equal(_bits(got[..., :3]), _bits(E2))
        cam = fr[3][0]
        E, P, N = tc.frame(cam, w, h, win2[0], win2[1], 4)[:3]
        got = _accumulate(vrt, gpu_device, hist, cam, w, h, win2, E, P, N, prm)[0]
        _same_floats(got, tr.step(E, P, N, ref, cam, w, h, win2[0], win2[1], prm), "the window's second frame")
        assert (got[..., 3] > 1).any()


def test_step_refusals(vrt, gpu_device):
    import torch
    L = vrt.rtapi._temporal_lib()
    TP = vrt.rtapi.TemporalParams
    w, h = 45, 37
    fr, win, prm = tc.frames(w, h, "pan")
    rows = h
    ref = tr.History()
    nan, inf = float("nan"), float("inf")
    with vrt.rtapi.History(w, rows) as hist:
        cam, E, P, N = fr[0][:4]
        _same_floats(_accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm)[0], tr.step(E, P, N, ref, cam, w, h, 0, h, prm), "frame 0")
        cam, E, P, N = fr[1][:4]
        t = _device(gpu_device, E, P, N)
        out = _out4(gpu_device, rows * w)
        good_cam, good = vrt.rtapi.Camera.from_cam14(cam), TP(*prm)

        def call(hh=hist.handle, c=good_cam, ww=w, fh=h, y0=0, y1=h, sig=0, pos=0, nrm=0, p=good, o=0, null=()):
            a = {"sig": t[0].data_ptr() + sig, "pos": t[1].data_ptr() + pos, "nrm": t[2].data_ptr() + nrm, "out": out.data_ptr() + o}
            for k in null:
                a[k] = None
            return L.vxrt_temporal_accumulate(hh, None if c is None else C.byref(c), ww, fh, y0, y1, a["sig"], a["pos"], a["nrm"],
                                              None if p is None else C.byref(p), a["out"], _stream())
        assert call(hh=None) == -1 and call(c=None) == -1 and call(p=None) == -1
        for k in ("sig", "pos", "nrm", "out"):
            assert call(null=(k,)) == -1
        for i in range(14):
            for v in (nan, inf, -inf):
                c = np.array(cam, np.float32)
                c[i] = v
                assert call(c=vrt.rtapi.Camera.from_cam14(c)) == -1
        assert call(pos=4) == -1 and call(nrm=8) == -1                                  # not 16-byte aligned
        assert call(ww=65536, fh=32768, y1=32768) == -1                                 # 2^31 pixels
        assert call(fh=h + 1, y1=h + 1) == -1                                           # more than the history holds
        assert call(ww=0) == -1 and call(fh=0, y1=0) == -1 and call(y0=5, y1=3) == -1 and call(y1=h + 1) == -1
        for bad in (TP(0.0, 32, 0.5, 0.9), TP(-0.1, 32, 0.5, 0.9), TP(1.5, 32, 0.5, 0.9), TP(nan, 32, 0.5, 0.9), TP(0.1, 0, 0.5, 0.9),
                    TP(0.1, vrt.rtapi.TEMPORAL_MAX_LEN + 1, 0.5, 0.9), TP(0.1, 32, 0.0, 0.9), TP(0.1, 32, -1.0, 0.9), TP(0.1, 32, nan, 0.9),
                    TP(0.1, 32, 0.5, nan), TP(0.1, 32, 0.5, inf), TP(0.1, 32, 0.5, -inf)):
            assert call(p=bad) == -1
        assert call(y0=7, y1=7) == 0                                                    # the empty window
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == np.float32(FMARK)).all()
        # the history is as frame 0 left it
        _same_floats(_accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm)[0], tr.step(E, P, N, ref, cam, w, h, 0, h, prm), "frame 1")
        assert call(p=TP(1.0, vrt.rtapi.TEMPORAL_MAX_LEN, inf, -3.0e38)) == 0
    e = vrt.rtapi.History(4, 4)
    rd = _out4(gpu_device, 16)
    assert L.vxrt_history_read(e.handle, rd.data_ptr(), _stream()) == -1 and L.vxrt_history_read(None, rd.data_ptr(), _stream()) == -1   # empty
    assert L.vxrt_history_reset(None) == -1 and L.vxrt_history_destroy(None) == -1
    h0 = C.c_void_p()
    assert L.vxrt_history_create(0, 4, C.byref(h0)) == -1 and L.vxrt_history_create(4, 0, C.byref(h0)) == -1 and L.vxrt_history_create(4, 4, None) == -1
    assert L.vxrt_history_create(65536, 32768, C.byref(h0)) == -1
    e.close()


# ---- the path frame ----
@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    yield b, ds
    ds.close()


def _cameras(vrt):
    return [np.array(vrt.rtapi.look_at(e, tc.PATH_CENTRE, (0.0, 1.0, 0.0), 1.0, W, H).cam14(), np.float32) for e in tc.PATH_EYES]


@pytest.fixture(scope="module")
def reference(vrt, po, hall):
    """the restatement's frames of a (configuration, window, dn) sequence, computed once: frame k has seed + k"""
    cache = {}

    def get(cfg, win=(0, H), dn=dc.PATH_DN, n=N_FRAMES):
        key = (cfg, win, dn)
        if key not in cache or len(cache[key]) < n:
            spp, bounces, shadow, seed = cfg
            hist = tr.History()
            cache[key] = [tr.path_frame(hall[0], cam, W, H, po.shade_params(), spp, bounces, seed + k, shadow, dn, tc.PATH_TP, hist, win[0], win[1])
                          for k, cam in enumerate(_cameras(vrt)[:n])]
        return cache[key]
    return get


def _outputs(dev):
    import torch
    o = {"px": torch.full((H, W), MARK, dtype=torch.int32, device=dev), "col": torch.full((H, W, 3), FMARK, dtype=torch.float32, device=dev),
         "cnt": torch.zeros(1, dtype=torch.int64, device=dev), "hist": torch.full((H * W * 4,), FMARK, dtype=torch.float32, device=dev)}
    for k, c in AOV:
        o[k] = torch.full((H, W, c), FMARK, dtype=torch.float32, device=dev)
    return o


def _temporal(vrt, ds, hist, cam, cfg, k, win=(0, H), dn=dc.PATH_DN, stream=None, out=None):
    """frame k of a sequence: seed + k.  Returns the device outputs, the history read behind the frame on the same stream"""
    spp, bounces, shadow, seed = cfg
    o = out or _outputs(ds.t["tri"].device)
    s = _stream() if stream is None else stream
    vrt.rtapi.render_path_temporal(ds.accel, cam, W, H, win[0], win[1], vrt.rtapi.default_shade_params(), spp, bounces, vrt.rtapi.DenoiseParams(*dn),
                                   vrt.rtapi.TemporalParams(*tc.PATH_TP), hist, o["px"].data_ptr(), seed + k, shadow, o["col"].data_ptr(),
                                   vrt.rtapi.PathAov(*[o[n].data_ptr() for n, _ in AOV]), o["cnt"].data_ptr(), s)
    hist.read(o["hist"].data_ptr(), s)
    return o


def _host(o):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "px" else int(v.item()) if k == "cnt" else v.cpu().numpy()) for k, v in o.items()}


def _check(got, want, what, win=(0, H)):
    y0, y1 = win
    _same_floats(got["col"][y0:y1], want["col"], what + ": colours")
    np.testing.assert_array_equal(got["px"][y0:y1], want["px"], err_msg=what + ": pixels")
    assert got["cnt"] == want["rays"], "%s: rays traced %d, restatement %d" % (what, got["cnt"], want["rays"])
    outside = np.ones(H, bool)
    outside[y0:y1] = False
    assert (got["px"][outside] == MARK).all() and (got["col"][outside] == np.float32(FMARK)).all(), what + ": rows outside the window"
    for k, _ in AOV:
        _same_floats(got[k][y0:y1], want[k], what + ": " + k)
        assert (got[k][outside] == np.float32(FMARK)).all(), what + ": " + k + " outside the window"
    n4 = (y1 - y0) * W * 4
    _same_floats(got["hist"][:n4].reshape(y1 - y0, W, 4), want["T"], what + ": the history")
    assert (got["hist"][n4:] == np.float32(FMARK)).all(), what + ": vxrt_history_read past the window"


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("cfg", dc.PATH_CONFIGS)
def test_frames_against_the_restatement(vrt, hall, reference, cfg, win):
    b, ds = hall
    want = reference(cfg, win)
    assert all((w["T"][..., 3] > 1).any() for w in want[1:3])     # (the orbit step and the dolly take history)
    with vrt.rtapi.History(W, win[1] - win[0]) as hist:
        for k, cam in enumerate(_cameras(vrt)):
            got = _host(_temporal(vrt, ds, hist, cam, cfg, k, win))
            _check(got, want[k], "%r rows %r frame %d" % (cfg, win, k), win)


def test_no_iterations_remodulate_the_accumulated_signal(vrt, hall, reference):
    b, ds = hall
    cfg, dn = dc.PATH_CONFIGS[0], (0,) + dc.PATH_DN[1:]
    want = reference(cfg, (0, H), dn, 2)
    with vrt.rtapi.History(W, H) as hist:
        for k, cam in enumerate(_cameras(vrt)[:2]):
            _check(_host(_temporal(vrt, ds, hist, cam, cfg, k, dn=dn)), want[k], "no iterations, frame %d" % k)


def _denoised(vrt, ds, cam, cfg, k, win=(0, H)):
    spp, bounces, shadow, seed = cfg
    o = _outputs(ds.t["tri"].device)
    vrt.rtapi.render_path_denoised(ds.accel, cam, W, H, win[0], win[1], vrt.rtapi.default_shade_params(), spp, bounces, vrt.rtapi.DenoiseParams(*dc.PATH_DN),
                                   o["px"].data_ptr(), seed + k, shadow, o["col"].data_ptr(), vrt.rtapi.PathAov(*[o[n].data_ptr() for n, _ in AOV]),
                                   o["cnt"].data_ptr(), _stream())
    return o


def _same_frame(got, want, what):
    for k in ("px", "col") + tuple(n for n, _ in AOV):
        np.testing.assert_array_equal(np.asarray(got[k]).view(np.uint32), np.asarray(want[k]).view(np.uint32), err_msg=what + ": " + k)
    assert got["cnt"] == want["cnt"], what


def test_first_frames_are_the_denoised_frame(vrt, hall):
    """on an empty history, after a reset and in another window the frame is vxrt_render_path_denoised bit for bit; the frame in between is not"""
    b, ds = hall
    cams = _cameras(vrt)
    cfg = dc.PATH_CONFIGS[0]
    with vrt.rtapi.History(W, H) as hist:
        _same_frame(_host(_temporal(vrt, ds, hist, cams[0], cfg, 0)), _host(_denoised(vrt, ds, cams[0], cfg, 0)), "an empty history")
        second, plain = _host(_temporal(vrt, ds, hist, cams[1], cfg, 1)), _host(_denoised(vrt, ds, cams[1], cfg, 1))
        assert (second["px"] != plain["px"]).any() and (second["hist"].reshape(H, W, 4)[..., 3] > 1).any()
        hist.reset()
        _same_frame(_host(_temporal(vrt, ds, hist, cams[2], cfg, 2)), _host(_denoised(vrt, ds, cams[2], cfg, 2)), "after a reset")
        win = dc.PATH_WINDOW
        _same_frame(_host(_temporal(vrt, ds, hist, cams[2], cfg, 3, win)), _host(_denoised(vrt, ds, cams[2], cfg, 3, win)), "another window")


def test_frame_refusals(vrt, hall, reference):
    import torch
    b, ds = hall
    L = vrt.rtapi._temporal_lib()
    cfg = dc.PATH_CONFIGS[0]
    want = reference(cfg)
    cams = _cameras(vrt)
    PP, DP, TP = vrt.rtapi.PathParams, vrt.rtapi.DenoiseParams, vrt.rtapi.TemporalParams
    nan, inf = float("nan"), float("inf")
    px = torch.full((H, W), MARK, dtype=torch.int32, device=ds.t["tri"].device)
    with vrt.rtapi.History(W, H) as hist, vrt.rtapi.History(W, H // 2) as small:
        _check(_host(_temporal(vrt, ds, hist, cams[0], cfg, 0)), want[0], "frame 0")
        p, q, d, t = vrt.rtapi.default_shade_params(), PP(cfg[0], cfg[1], cfg[3] + 1, cfg[2]), DP(*dc.PATH_DN), TP(*tc.PATH_TP)
        good = vrt.rtapi.Camera.from_cam14(cams[1])

        def call(accel=ds.accel, cam=good, y0=0, y1=H, params=p, path=q, dn=d, tp=t, hh=hist.handle, dst=px.data_ptr()):
            ref = [None if v is None else C.byref(v) for v in (cam, params, path, dn, tp)]
            return L.vxrt_render_path_temporal(accel, ref[0], W, H, y0, y1, ref[1], ref[2], ref[3], ref[4], hh, dst, None, None, None, _stream())
        assert call(cam=None) == -1                       # the fixed camera has no vxrt_camera_t
        for kw in ({"accel": None}, {"params": None}, {"path": None}, {"dn": None}, {"tp": None}, {"hh": None}, {"dst": None}):
            assert call(**kw) == -1, kw
        for i in range(14):
            for v in (nan, inf, -inf):
                c = cams[1].copy()
                c[i] = v
                assert call(cam=vrt.rtapi.Camera.from_cam14(c)) == -1
        for bad in (TP(0.0, 3, 2.0, 0.9), TP(1.5, 3, 2.0, 0.9), TP(nan, 3, 2.0, 0.9), TP(0.2, 0, 2.0, 0.9), TP(0.2, vrt.rtapi.TEMPORAL_MAX_LEN + 1, 2.0, 0.9),
                    TP(0.2, 3, 0.0, 0.9), TP(0.2, 3, nan, 0.9), TP(0.2, 3, 2.0, nan), TP(0.2, 3, 2.0, inf)):
            assert call(tp=bad) == -1
        # whatever the denoised entry point refuses
        for bad in (DP(7, 5, 2.0, 0.25), DP(3, 8, 2.0, 0.25), DP(3, 5, 0.0, 0.25), DP(3, 5, 2.0, nan)):
            assert call(dn=bad) == -1
        for bad in (PP(0, 3, 0, 1), PP(4097, 3, 0, 1), PP(2, vrt.rtapi.PATH_MAX_BOUNCES + 1, 0, 1), PP(2, 3, 0, 2)):
            assert call(path=bad) == -1
        assert call(y0=5, y1=3) == -1 and call(y1=H + 1) == -1
        assert call(hh=small.handle) == -1                # a window larger than the capacity
        assert call(y0=7, y1=7) == 0                      # the empty window
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
        assert L.vxrt_history_read(small.handle, px.data_ptr(), _stream()) == -1      # still empty
        _check(_host(_temporal(vrt, ds, hist, cams[1], cfg, 1)), want[1], "frame 1 after the refusals")


def test_alpha_table_is_refused(vrt, golden, gpu_device):
    import torch
    import camera_secondary_ref as csr
    import shading_ref as sr
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in csr.KEYS}, gpu_device)
    try:
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        cam = csr.golden_cameras(vrt)["g_orbit_1"]
        with vrt.rtapi.History(W, H) as hist:
            def call():
                vrt.rtapi.render_path_temporal(ds.accel, cam, W, H, 0, H, vrt.rtapi.default_shade_params(), 2, 3, vrt.rtapi.DenoiseParams(*dc.PATH_DN),
                                               vrt.rtapi.TemporalParams(*tc.PATH_TP), hist, px.data_ptr(), 0, 0, None, None, None, _stream())
            with pytest.raises(RuntimeError):
                call()
            torch.cuda.synchronize()
            assert (px.cpu().numpy() == MARK).all()
            with pytest.raises(RuntimeError):
                hist.read(px.data_ptr(), _stream())       # (the refused frame left the history empty)
            ds.set_alpha_test(None)
            call()
            torch.cuda.synchronize()
            assert (px.cpu().numpy() != MARK).all()
    finally:
        ds.close()


def test_two_histories_on_two_streams(vrt, hall, reference):
    """two sequences interleaved on two streams, two frames in flight, a history each: every frame is the one its sequence gives alone"""
    import torch
    b, ds = hall
    dev = ds.t["tri"].device
    cams = _cameras(vrt)
    want = [reference(cfg) for cfg in dc.PATH_CONFIGS]
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        with vrt.rtapi.History(W, H) as h0, vrt.rtapi.History(W, H) as h1:
            outs = [[_outputs(dev) for _ in range(N_FRAMES)] for _ in range(2)]
            torch.cuda.synchronize()
            for k in range(N_FRAMES):
                for i, hist in enumerate((h0, h1)):
                    _temporal(vrt, ds, hist, cams[k], dc.PATH_CONFIGS[i], k, stream=streams[i].cuda_stream, out=outs[i][k])
            torch.cuda.synchronize()
            for i in range(2):
                for k in range(N_FRAMES):
                    _check(_host(outs[i][k]), want[i][k], "stream %d frame %d" % (i, k))
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)
