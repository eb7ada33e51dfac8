"""GPU: the guided a-trous filter (vxrt_denoise) and the denoised path frame (vxrt_render_path_denoised) against the restatement
tests/denoise_ref.py, bit for bit: f32 as u32, pixels, rays traced, the five guide outputs.  No masks, no tolerances, with one exception:
where the restatement gives a NaN the kernel must give a NaN of any payload (x86 and gfx950 generate different default NaNs).
tests/test_denoise_cpu.py shows that the cases (tests/denoise_cases.py) are not vacuous."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_secondary_ref as csr
import denoise_cases as dc
import denoise_ref as dr
import scenes

pytestmark = pytest.mark.gpu
W, H = dc.W, dc.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
FMARK = -12345.5   # marker of float outputs
GUARD = 64         # floats past the end of vxrt_denoise's out
AOV = (("noisy", 3), ("direct", 3), ("albedo", 3), ("position", 4), ("normal", 4))
BATCH_CHILD = os.environ.get("VXRT_DENOISE_TEST_CHILD") == "1"


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


# ---- the filter alone ----
def _denoise(vrt, dev, S, P, N, prm):
    """vxrt_denoise on device copies; returns out (rows, w, 3) and the guard floats behind it"""
    import torch
    rows, w = S.shape[:2]
    t = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (S, P, N)]
    out = torch.full((rows * w * 3 + GUARD,), FMARK, dtype=torch.float32, device=dev)
    nbytes = vrt.rtapi.denoise_scratch_bytes(w, rows)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    vrt.rtapi.denoise(w, rows, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), vrt.rtapi.DenoiseParams(*prm), out.data_ptr(), scratch.data_ptr(), nbytes,
                      _stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:rows * w * 3].reshape(rows, w, 3), o[rows * w * 3:]


@pytest.mark.parametrize("w,h", dc.FRAMES)
def test_filter_against_the_restatement(vrt, gpu_device, w, h):
    S, P, N, _, _ = dc.synthetic(w, h)
    for prm in dc.cases(w, h):
        got, guard = _denoise(vrt, gpu_device, S, P, N, prm)
        assert vrt.rtapi.status(_stream()) == 0
        _same_floats(got, dr.atrous(S, P, N, *prm), "%dx%d %r" % (w, h, prm))
        assert (guard == np.float32(FMARK)).all(), "%dx%d %r: written past the end of out" % (w, h, prm)


def test_filter_without_iterations_copies_the_signal(vrt, gpu_device):
    S, P, N, _, _ = dc.synthetic(45, 37)
    got, guard = _denoise(vrt, gpu_device, S, P, N, (0,) + dc.GUIDED)
    np.testing.assert_array_equal(_bits(got), _bits(S))
    assert (guard == np.float32(FMARK)).all()


def test_filter_refusals(vrt, gpu_device):
    import torch
    L = vrt.rtapi._denoise_lib()
    DP = vrt.rtapi.DenoiseParams
    w, h = 45, 37
    S, P, N, _, _ = dc.synthetic(w, h)
    t = [torch.from_numpy(a).to(gpu_device) for a in (S, P, N)]
    out = torch.full((h * w * 3,), FMARK, dtype=torch.float32, device=gpu_device)
    nbytes = vrt.rtapi.denoise_scratch_bytes(w, h)
    assert nbytes == 32 * w * h
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)

    def call(dn, scratch_bytes=nbytes, ww=w, hh=h, sig=0, pos=0, nrm=0, scr=0, alias=False):
        return L.vxrt_denoise(ww, hh, t[0].data_ptr() + sig, t[1].data_ptr() + pos, t[2].data_ptr() + nrm, None if dn is None else C.byref(dn),
                              t[0].data_ptr() if alias else out.data_ptr(), scratch.data_ptr() + scr, scratch_bytes, _stream())
    nan, inf = float("nan"), float("inf")
    assert call(None) == -1
    for bad in (DP(7, 2, 1.0, 0.3), DP(3, 8, 1.0, 0.3), DP(3, 2, 0.0, 0.3), DP(3, 2, -1.0, 0.3), DP(3, 2, nan, 0.3), DP(3, 2, -inf, 0.3),
                DP(3, 2, 1.0, 0.0), DP(3, 2, 1.0, -0.5), DP(3, 2, 1.0, nan)):
        assert call(bad) == -1
    assert call(DP(3, 2, 1.0, 0.3), scratch_bytes=nbytes - 1) == -1
    assert call(DP(3, 2, 1.0, 0.3), pos=4) == -1 and call(DP(3, 2, 1.0, 0.3), nrm=8) == -1 and call(DP(3, 2, 1.0, 0.3), scr=4) == -1   # not 16-byte aligned
    assert call(DP(3, 2, 1.0, 0.3), alias=True) == -1                                                                            # out aliases signal
    assert call(DP(3, 2, 1.0, 0.3), ww=0) == 0 and call(DP(3, 2, 1.0, 0.3), hh=0) == 0   # the empty window
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(FMARK)).all()
    assert call(DP(3, 2, inf, inf)) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != np.float32(FMARK)).any()
    assert vrt.rtapi.status(_stream()) == 0


# ---- the denoised path frame ----
@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    yield b, ds
    ds.close()


def _camera(vrt, name):
    return None if name is None else csr.hall_cameras(vrt)[name]


def _outputs(dev, w, h, aov=True):
    import torch
    o = {"px": torch.full((h, w), MARK, dtype=torch.int32, device=dev), "col": torch.full((h, w, 3), FMARK, dtype=torch.float32, device=dev),
         "cnt": torch.zeros(1, dtype=torch.int64, device=dev)}
    if aov:
        for k, c in AOV:
            o[k] = torch.full((h, w, c), FMARK, dtype=torch.float32, device=dev)
    return o


def _denoised(vrt, ds, cam, w, h, cfg, dn, y0=0, y1=None, stream=None, out=None, aov=True):
    spp, bounces, shadow, seed = cfg
    o = out or _outputs(ds.t["tri"].device, w, h, aov)
    a = vrt.rtapi.PathAov(*[o[k].data_ptr() for k, _ in AOV]) if aov else None
    vrt.rtapi.render_path_denoised(ds.accel, cam, w, h, y0, h if y1 is None else y1, vrt.rtapi.default_shade_params(), spp, bounces, vrt.rtapi.DenoiseParams(*dn),
                                   o["px"].data_ptr(), seed, shadow, o["col"].data_ptr(), a, o["cnt"].data_ptr(), _stream() if stream is None else stream)
    return o


def _host(o):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "px" else int(v.item()) if k == "cnt" else v.cpu().numpy()) for k, v in o.items()}


def _check(got, want, what, y0=0, y1=H, aov=True):
    """got: _host() of a full frame; want: denoise_ref.path_frame of rows [y0, y1).  Rows outside keep their markers."""
    _same_floats(got["col"][y0:y1], want["col"], what + ": colours")
    np.testing.assert_array_equal(got["px"][y0:y1], want["px"], err_msg=what + ": pixels")
    assert got["cnt"] == want["rays"], "%s: rays traced %d, restatement %d" % (what, got["cnt"], want["rays"])
    outside = np.ones(got["px"].shape[0], bool)
    outside[y0:y1] = False
    assert (got["px"][outside] == MARK).all() and (got["col"][outside] == np.float32(FMARK)).all(), what + ": rows outside the window"
    for k, _ in (AOV if aov else ()):
        _same_floats(got[k][y0:y1], want[k], what + ": " + k)
        assert (got[k][outside] == np.float32(FMARK)).all(), what + ": " + k + " outside the window"


def _against_ref(vrt, po, b, ds, name, cfg, dn=dc.PATH_DN, y0=0, y1=H):
    cam = _camera(vrt, name)
    got = _host(_denoised(vrt, ds, cam, W, H, cfg, dn, y0, y1))
    assert vrt.rtapi.status(_stream()) == 0
    spp, bounces, shadow, seed = cfg
    want = dr.path_frame(b, cam, W, H, po.shade_params(), spp, bounces, seed, shadow, dn, y0, y1)
    _check(got, want, "%s %r %r rows %d..%d" % (name, cfg, dn, y0, y1), y0, y1)
    return got


@pytest.mark.parametrize("cfg", dc.PATH_CONFIGS)
@pytest.mark.parametrize("name", dc.PATH_CAMERAS)
def test_frames_against_the_restatement(vrt, po, hall, name, cfg):
    b, ds = hall
    _against_ref(vrt, po, b, ds, name, cfg)


@pytest.mark.parametrize("cfg", dc.PATH_CONFIGS)
def test_row_window(vrt, po, hall, cfg):
    b, ds = hall
    got = _against_ref(vrt, po, b, ds, "framing", cfg, y0=dc.PATH_WINDOW[0], y1=dc.PATH_WINDOW[1])
    assert (got["px"][dc.PATH_WINDOW[0]:dc.PATH_WINDOW[1]] != MARK).any()


def test_six_iterations(vrt, po, hall):
    """step 32: a third of the frame's width"""
    b, ds = hall
    _against_ref(vrt, po, b, ds, "framing", dc.PATH_CONFIGS[0], (6,) + dc.PATH_DN[1:])


@pytest.mark.parametrize("name", ["framing", None])
def test_no_iterations_are_the_path_frame(vrt, hall, name):
    """iterations = 0 against the GPU's own vxrt_render_path: colours, pixels, rays; the guide outputs are still written"""
    import torch
    b, ds = hall
    cam = _camera(vrt, name)
    dev = ds.t["tri"].device
    for spp, bounces, shadow, seed in dc.PATH_CONFIGS + ((4, 0, 1, 5),):
        px = torch.full((H, W), MARK, dtype=torch.int32, device=dev)
        col = torch.zeros(H * W * 3, dtype=torch.float32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        vrt.rtapi.render_path(ds.accel, cam, W, H, 0, H, vrt.rtapi.default_shade_params(), spp, bounces, px.data_ptr(), seed, shadow, col.data_ptr(),
                              cnt.data_ptr(), _stream())
        got = _host(_denoised(vrt, ds, cam, W, H, (spp, bounces, shadow, seed), (0,) + dc.PATH_DN[1:]))
        assert vrt.rtapi.status(_stream()) == 0
        np.testing.assert_array_equal(_bits(got["col"]).reshape(-1), _bits(col.cpu().numpy()))
        np.testing.assert_array_equal(got["px"], px.cpu().numpy().view(np.uint32))
        assert got["cnt"] == int(cnt.item())
        np.testing.assert_array_equal(_bits(got["noisy"]), _bits(got["col"]))
        assert (got["position"][..., 3] == 1.0).any() and (got["albedo"] != np.float32(FMARK)).all()


def _prototype(vrt):
    return vrt.rtapi._denoise_lib()


def _call(vrt, L, accel, px, cam, y0=0, y1=H, params="default", path="default", dn="default"):
    p = vrt.rtapi.default_shade_params()
    pref = C.byref(p) if params == "default" else params
    q = vrt.rtapi.PathParams(2, 3, 0, 1)
    qref = C.byref(q) if path == "default" else (C.byref(path) if path is not None else None)
    d = vrt.rtapi.DenoiseParams(*dc.PATH_DN)
    dref = C.byref(d) if dn == "default" else (C.byref(dn) if dn is not None else None)
    cref = C.byref(cam) if cam is not None else None
    return L.vxrt_render_path_denoised(accel, cref, W, H, y0, y1, pref, qref, dref, px.data_ptr(), None, None, None, _stream())


def test_refusals(vrt, hall):
    import torch
    b, ds = hall
    L = _prototype(vrt)
    px = torch.full((H, W), MARK, dtype=torch.int32, device=ds.t["tri"].device)
    base = csr.framing(W, H)
    good = vrt.rtapi.Camera.from_cam14(base)
    PP, DP = vrt.rtapi.PathParams, vrt.rtapi.DenoiseParams
    nan, inf = float("nan"), float("inf")
    for cam in (good, None):
        assert _call(vrt, L, ds.accel, px, cam, dn=None) == -1
        for bad in (DP(7, 5, 2.0, 0.25), DP(3, 8, 2.0, 0.25), DP(3, 5, 0.0, 0.25), DP(3, 5, -2.0, 0.25), DP(3, 5, nan, 0.25), DP(3, 5, 2.0, 0.0),
                    DP(3, 5, 2.0, -inf), DP(3, 5, 2.0, nan), DP(0, 8, 2.0, 0.25)):
            assert _call(vrt, L, ds.accel, px, cam, dn=bad) == -1
        # everything vxrt_render_path refuses
        assert _call(vrt, L, ds.accel, px, cam, path=None) == -1
        for bad in (PP(0, 3, 0, 1), PP(4097, 3, 0, 1), PP(2, vrt.rtapi.PATH_MAX_BOUNCES + 1, 0, 1), PP(2, 3, 0, 2)):
            assert _call(vrt, L, ds.accel, px, cam, path=bad) == -1
        assert _call(vrt, L, ds.accel, px, cam, y0=5, y1=3) == -1
        assert _call(vrt, L, ds.accel, px, cam, y0=0, y1=H + 1) == -1
        assert _call(vrt, L, ds.accel, px, cam, params=None) == -1
        assert _call(vrt, L, None, px, cam) == -1
        assert _call(vrt, L, ds.accel, px, cam, y0=7, y1=7) == 0         # the empty window
    for i in range(14):
        for v in (nan, inf, -inf):
            c = base.copy()
            c[i] = v
            assert _call(vrt, L, ds.accel, px, vrt.rtapi.Camera.from_cam14(c)) == -1
    torch.cuda.synchronize()
    assert (px.cpu().numpy() == MARK).all()
    assert vrt.rtapi.status(_stream()) == 0
    assert _call(vrt, L, ds.accel, px, good, dn=DP(6, 7, inf, inf)) == 0
    torch.cuda.synchronize()
    assert (px.cpu().numpy() != MARK).all()


def test_alpha_table_is_refused(vrt, golden, gpu_device):
    import torch
    import shading_ref as sr
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in KEYS}, gpu_device)
    try:
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        assert (mat["tex_id"] >= 0).any()
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        L = _prototype(vrt)
        cam = vrt.rtapi.Camera.from_cam14(csr.golden_cameras(vrt)["g_orbit_1"])
        assert _call(vrt, L, ds.accel, px, cam) == -1
        assert _call(vrt, L, ds.accel, px, None) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
        ds.set_alpha_test(None)
        assert _call(vrt, L, ds.accel, px, cam) == 0
        torch.cuda.synchronize()
        assert (px.cpu().numpy() != MARK).all()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()


def test_two_frames_in_flight(vrt, po, hall):
    """two frames on two streams with different cameras (and so different signals in the contexts' buffers) equal their serial results"""
    import torch
    b, ds = hall
    dev = ds.t["tri"].device
    cams = [csr.orbit(vrt, 1), csr.orbit(vrt, 6)]
    cfgs = [(2, 3, 1, 3), (2, 3, 1, 11)]
    serial = [_host(_denoised(vrt, ds, cams[i], W, H, cfgs[i], dc.PATH_DN)) for i in range(2)]
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        outs = [_outputs(dev, W, H) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(2):
            _denoised(vrt, ds, cams[i], W, H, cfgs[i], dc.PATH_DN, stream=streams[i].cuda_stream, out=outs[i])
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
        for i in range(2):
            got = _host(outs[i])
            for k in got:
                np.testing.assert_array_equal(np.asarray(got[k]).view(np.uint32) if k != "cnt" else got[k],
                                              np.asarray(serial[i][k]).view(np.uint32) if k != "cnt" else serial[i][k], err_msg="in flight %d: %s" % (i, k))
        spp, bounces, shadow, seed = cfgs[0]
        _check(serial[0], dr.path_frame(b, cams[0], W, H, po.shade_params(), spp, bounces, seed, shadow, dc.PATH_DN), "serial 0")
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)


def test_small_path_batches(vrt, po, hall):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs this test's body with 2 * W * H paths per batch, so that spp = 5 takes
    batches of 2, 2 and 1 samples before the filter"""
    if not BATCH_CHILD:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, VXRT_PATH_BATCH=str(2 * W * H), VXRT_DENOISE_TEST_CHILD="1")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "small_path_batches"],
                           env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
        return
    b, ds = hall
    assert os.environ["VXRT_PATH_BATCH"] == str(2 * W * H)
    _against_ref(vrt, po, b, ds, "framing", (5, 2, 1, 0))
