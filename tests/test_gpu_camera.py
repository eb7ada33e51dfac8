"""GPU: frames from a caller-supplied pinhole camera (vxrt_render_camera, vxrt_render_batch_camera, vxrt_pinhole_rays) against the
numpy restatement tests/camera_ref.py, bit for bit: rays, pixels, hit records (occlusion bit included), colours and rays traced."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_ref as cr
import scenes

pytestmark = pytest.mark.gpu
W, H = 96, 64
KEYS = ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")
LDS_VARIANT = os.environ.get("VXRT_CAMERA_TEST_VARIANT") == "1"


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _host(ds):
    return {k: ds.t[k].cpu().numpy().copy() for k in KEYS}


def _framing(w, h):
    return np.array([0, 100, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0], np.float32)


def _orbit(vrt, k, n=8, w=W, h=H):
    a = 2.0 * math.pi * k / n
    eye = (180.0 + 260.0 * math.cos(a), 140.0, 260.0 * math.sin(a))
    return np.array(vrt.rtapi.look_at(eye, (180.0, 90.0, 0.0), (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32)


def _cameras(vrt, w=W, h=H):
    c = {"framing": _framing(w, h), "inside_blob": np.array([180, 90, 30, 0.3, -0.2, 1, 1, 0, 0, 0, 1, 0, 2.0, 1.4], np.float32)}
    for k in range(8):
        c["orbit_%d" % k] = _orbit(vrt, k, 8, w, h)
    c.update(cr.hostile_cameras(w, h))
    return c


def _outputs(dev, w, h):
    """pixels (marker-filled), hit records, colours, ray counter of a w x h frame"""
    import torch
    return (torch.full((h, w), 0x5A5A5A, dtype=torch.int32, device=dev), torch.zeros(h * w * 24, dtype=torch.uint8, device=dev),
            torch.zeros(h * w * 3, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def _issue(vrt, ds, cam, w, h, params, shadow, out, y0=0, y1=None, stream=None):
    px, hits, col, cnt = out
    y1 = h if y1 is None else y1
    vrt.rtapi.render_camera(ds.accel, cam, w, h, y0, y1, params, px.data_ptr(), shadow, hits.data_ptr(), col.data_ptr(), cnt.data_ptr(),
                            _stream() if stream is None else stream)
    return out


def _render_camera(vrt, ds, cam, w, h, params, shadow, y0=0, y1=None):
    """one camera frame on the current stream (the outputs are filled on it too)"""
    return _issue(vrt, ds, cam, w, h, params, shadow, _outputs(ds.t["tri"].device, w, h), y0, y1)


def _host_frame(px, hits, col, cnt, w, h, y0, y1):
    import torch
    from oracle.pyoracle import HIT_DTYPE
    torch.cuda.synchronize()
    return (px.cpu().numpy().view(np.uint32)[y0:y1], hits.cpu().numpy().view(HIT_DTYPE).reshape(h, w)[y0:y1],
            col.cpu().numpy().reshape(h, w, 3)[y0:y1], int(cnt.item()))


def _check(got, want, what):
    px, hits, col, n = got
    rpx, rhits, rcol, rn = want
    bad = np.nonzero(px.reshape(-1) != rpx.reshape(-1))[0]
    assert len(bad) == 0, "%s: %d pixels differ, first at %s" % (what, len(bad), bad[:5])
    for k in ("dist", "bx", "by", "bz", "blasIdx", "triIdx"):
        np.testing.assert_array_equal(hits[k].view(np.uint32), rhits[k].view(np.uint32), err_msg="%s: hits.%s" % (what, k))
    np.testing.assert_array_equal(col.view(np.uint32), rcol.view(np.uint32), err_msg=what + ": colours")
    assert n == rn, "%s: rays traced %d, restatement %d" % (what, n, rn)


@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    yield b, ds
    ds.close()


@pytest.mark.parametrize("w,h,y0,y1", [(1, 1, 0, 1), (13, 7, 0, 7), (96, 64, 0, 64), (96, 64, 5, 29), (13, 7, 3, 3)])
def test_pinhole_rays(vrt, gpu_device, w, h, y0, y1):
    import torch
    for name, cam in _cameras(vrt, w, h).items():
        n = w * (y1 - y0)
        out = torch.full((max(n, 1) * 6,), float("nan"), dtype=torch.float32, device=gpu_device)
        vrt.rtapi.pinhole_rays(cam, w, h, y0, y1, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        got = out.cpu().numpy()[:n * 6].reshape(-1, 6)
        np.testing.assert_array_equal(got.view(np.uint32), cr.rays(cam, w, h, y0, y1).view(np.uint32), err_msg=name)


@pytest.mark.parametrize("shadow", [0, 1])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_render_camera_mirror_hall(vrt, po, hall, shadow, depth):
    b, ds = hall
    p = vrt.rtapi.default_shade_params()
    p.max_depth = depth
    pp = po.shade_params(max_depth=depth)
    cams = _cameras(vrt)
    if depth > 1:   # (the bounce paths: a representative subset, every hostile camera at depth 1)
        cams = {k: v for k, v in cams.items() if k in ("framing", "orbit_0", "orbit_3", "orbit_6", "inside_blob", "axis_aligned", "non_orthonormal")}
    for name, cam in cams.items():
        got = _host_frame(*_render_camera(vrt, ds, cam, W, H, p, shadow), W, H, 0, H)
        assert vrt.rtapi.status(_stream()) == 0
        _check(got, cr.frame(b, cam, W, H, pp, shadow), "%s shadow=%d depth=%d" % (name, shadow, depth))


def test_render_camera_row_window(vrt, po, hall):
    b, ds = hall
    p = vrt.rtapi.default_shade_params()
    cam = _orbit(vrt, 2)
    got = _host_frame(*_render_camera(vrt, ds, cam, W, H, p, 1, 11, 37), W, H, 11, 37)
    _check(got, cr.frame(b, cam, W, H, po.shade_params(), 1, 11, 37), "window")


@pytest.mark.parametrize("n_frames", [1, 5, 32])
def test_render_batch_camera(vrt, po, golden, gpu_device, n_frames):
    import torch
    g = golden("teapot_x3")
    b = {k: g[k] for k in KEYS}
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        w, h = 48, 32
        cams = [_orbit(vrt, f, 32, w, h) if f % 3 else _framing(w, h) for f in range(n_frames)]
        plist = []
        for f in range(n_frames):
            p = vrt.rtapi.default_shade_params()
            p.light_pos[:] = (10.0 * math.cos(f), 50.0, -10.0 + f)
            plist.append(p)
        buf = torch.full((n_frames, h, w), 0x5A5A5A, dtype=torch.int32, device=gpu_device)
        cnt = torch.zeros(1, dtype=torch.int64, device=gpu_device)
        vrt.rtapi.render_batch_camera(ds.accel, w, h, cams, plist, buf.data_ptr(), h * w, 1, cnt.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
        frames = buf.cpu().numpy().view(np.uint32)
        total = 0
        for f in range(0, n_frames, max(1, n_frames // 6)):
            pp = po.shade_params(light_pos=tuple(plist[f].light_pos))
            rpx, _, _, rn = cr.frame(b, cams[f], w, h, pp, 1)
            np.testing.assert_array_equal(frames[f], rpx, err_msg="frame %d" % f)
            single = _host_frame(*_render_camera(vrt, ds, cams[f], w, h, plist[f], 1), w, h, 0, h)
            np.testing.assert_array_equal(single[0], frames[f])
        for f in range(n_frames):
            pp = po.shade_params(light_pos=tuple(plist[f].light_pos))
            total += cr.frame_from_rays(b, cr.rays(cams[f], w, h), pp, 1)[3] if n_frames <= 5 else 0
        if n_frames <= 5:
            assert int(cnt.item()) == total
    finally:
        ds.close()


def test_frames_in_flight_and_fixed_frame_untouched(vrt, po, hall):
    import torch
    b, ds = hall
    dev = ds.t["tri"].device
    p = vrt.rtapi.default_shade_params()
    fixed0 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    vrt.rtapi.render(ds.accel, W, H, 0, H, p, fixed0.data_ptr(), 1, None, None, None, _stream())
    torch.cuda.synchronize()
    fixed0 = fixed0.cpu().numpy().copy()
    vrt.rtapi.accel_frames_in_flight(ds.accel, 4)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(4)]
        sizes = [(96, 64), (40, 24), (96, 64), (72, 40)]
        # every job's outputs first, one synchronisation, then all renders back to back with no host wait: up to four camera
        # frames (different cameras, different sizes) in flight on four streams and four frame contexts at once, and a fixed-camera
        # frame among them
        jobs = []
        for i in range(8):
            w, h = sizes[i % 4]
            cam = _orbit(vrt, i, 8, w, h) if i % 2 else _framing(w, h) * np.float32(1.0 + 0.01 * i)
            jobs.append((cam, w, h, _outputs(dev, w, h)))
        fixed_mid = torch.zeros((H, W), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for i, (cam, w, h, out) in enumerate(jobs):
            _issue(vrt, ds, cam, w, h, p, 1, out, stream=streams[i % 4].cuda_stream)
            if i == 4:
                vrt.rtapi.render(ds.accel, W, H, 0, H, p, fixed_mid.data_ptr(), 1, None, None, None, streams[1].cuda_stream)
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
        for i, (cam, w, h, out) in enumerate(jobs):
            _check(_host_frame(*out, w, h, 0, h), cr.frame(b, cam, w, h, po.shade_params(), 1), "in flight %d" % i)
        np.testing.assert_array_equal(fixed_mid.cpu().numpy(), fixed0)
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)
    fixed1 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    vrt.rtapi.render(ds.accel, W, H, 0, H, p, fixed1.data_ptr(), 1, None, None, None, _stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(fixed1.cpu().numpy(), fixed0)
    np.testing.assert_array_equal(fixed0.view(np.uint32), po.render_ex(b, W, H, po.shade_params(), 1)[0])


def test_camera_frame_after_set_transforms_and_refit(vrt, po, gpu_device):
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        m = np.eye(4, dtype=np.float32)
        m[0, 3], m[1, 3], m[2, 3] = -30.0, 12.0, 25.0
        ds.set_transforms([m], first=3)
        cam = _orbit(vrt, 1)
        p = vrt.rtapi.default_shade_params()
        got = _host_frame(*_render_camera(vrt, ds, cam, W, H, p, 1), W, H, 0, H)
        _check(got, cr.frame(_host(ds), cam, W, H, po.shade_params(), 1), "after set_transforms")
        import torch
        ds.t["tri"].view(torch.float32).mul_(1.01)
        ds.refit(geometry=True)
        got = _host_frame(*_render_camera(vrt, ds, cam, W, H, p, 1), W, H, 0, H)
        _check(got, cr.frame(_host(ds), cam, W, H, po.shade_params(), 1), "after refit")
    finally:
        ds.close()


def test_camera_errors(vrt, hall):
    import torch
    b, ds = hall
    L = vrt.rtapi._lib()
    p = vrt.rtapi.default_shade_params()
    dev = ds.t["tri"].device
    px = torch.full((H, W), 0x5A5A5A, dtype=torch.int32, device=dev)
    rays = torch.full((W * H * 6,), 7.0, dtype=torch.float32, device=dev)
    base = _framing(W, H)
    L.vxrt_render_camera.restype = C.c_int
    L.vxrt_render_camera.argtypes = [C.c_void_p, C.POINTER(vrt.rtapi.Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.POINTER(vrt.rtapi.ShadeParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vxrt_pinhole_rays.restype = C.c_int
    L.vxrt_pinhole_rays.argtypes = [C.POINTER(vrt.rtapi.Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.vxrt_render_batch_camera.restype = C.c_int
    L.vxrt_render_batch_camera.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vrt.rtapi.Camera), C.POINTER(vrt.rtapi.ShadeParams),
                                           C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    assert L.vxrt_render_camera(ds.accel, None, W, H, 0, H, C.byref(p), 1, px.data_ptr(), None, None, None, _stream()) == -1
    for i in range(14):
        for bad in (float("nan"), float("inf"), -float("inf")):
            c = base.copy()
            c[i] = bad
            cam = vrt.rtapi.Camera.from_cam14(c)
            assert L.vxrt_render_camera(ds.accel, C.byref(cam), W, H, 0, H, C.byref(p), 1, px.data_ptr(), None, None, None, _stream()) == -1
            assert L.vxrt_pinhole_rays(C.byref(cam), W, H, 0, H, rays.data_ptr(), _stream()) == -1
            arr = (vrt.rtapi.Camera * 2)(vrt.rtapi.Camera.from_cam14(base), cam)
            parr = (vrt.rtapi.ShadeParams * 2)(p, p)
            assert L.vxrt_render_batch_camera(ds.accel, W, H, 2, arr, parr, 1, px.data_ptr(), 0, None, _stream()) == -1
    cam = vrt.rtapi.Camera.from_cam14(base)
    # what vxrt_render refuses
    assert L.vxrt_render_camera(ds.accel, C.byref(cam), W, H, 5, 3, C.byref(p), 1, px.data_ptr(), None, None, None, _stream()) == -1
    assert L.vxrt_render_camera(ds.accel, C.byref(cam), W, H, 0, H, None, 1, px.data_ptr(), None, None, None, _stream()) == -1
    torch.cuda.synchronize()
    assert (px.cpu().numpy() == 0x5A5A5A).all()
    assert (rays.cpu().numpy() == 7.0).all()
    assert vrt.rtapi.status(_stream()) == 0


def test_stale_accel_is_refused(vrt, gpu_device):
    import torch
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        v = ds.t["tri"].view(torch.float32).view(-1, 3, 3)
        v[0, 0, 0], v[1, 1, 0] = -3e38, 3e38   # one vertex pair: the extent overflows fp32, the refit fails and leaves the accel stale
        with pytest.raises(Exception):
            ds.refit(geometry=True)
        px = torch.full((H, W), 0x5A5A5A, dtype=torch.int32, device=gpu_device)
        L = vrt.rtapi._lib()
        L.vxrt_render_camera.restype = C.c_int
        cam = vrt.rtapi.Camera.from_cam14(_framing(W, H))
        L.vxrt_render_camera.argtypes = [C.c_void_p, C.POINTER(vrt.rtapi.Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(vrt.rtapi.ShadeParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.vxrt_render_camera(ds.accel, C.byref(cam), W, H, 0, H, C.byref(vrt.rtapi.default_shade_params()), 1, px.data_ptr(),
                                  None, None, None, _stream())
        L.vxrt_render_batch_camera.restype = C.c_int
        L.vxrt_render_batch_camera.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vrt.rtapi.Camera),
                                               C.POINTER(vrt.rtapi.ShadeParams), C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        rcb = [L.vxrt_render_batch_camera(ds.accel, W, hh, 1, C.byref(cam), C.byref(vrt.rtapi.default_shade_params()), 1, px.data_ptr(), 0,
                                          None, _stream()) for hh in (H, 0)]   # (a stale accel is refused even for an empty frame)
        torch.cuda.synchronize()
        assert rc == -1 and rcb == [-1, -1]
        assert (px.cpu().numpy() == 0x5A5A5A).all()
    finally:
        ds.close()


def test_1080p_atrium_framing_camera(vrt, po, gpu_device):
    if LDS_VARIANT:
        return   # (the variant run repeats the small scenes only)
    sc = vrt.scene.procedural("atrium", 8, 0, 3)
    assert sc.n_tris == 1048576
    b = {k: np.frombuffer(bytes(v), np.uint8).copy() for k, v in sc.buffers.items()}
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    try:
        w, h = 1920, 1080
        cam = np.array(vrt.scene.rc_camera_like_rtu(w, h), np.float32)
        p = vrt.rtapi.default_shade_params()
        px, hits, col, cnt = _render_camera(vrt, ds, cam, w, h, p, 1)
        px, hits, _, n = _host_frame(px, hits, col, cnt, w, h, 0, h)
        r = cr.rays(cam, w, h)
        want = po.trace_mt(po.trace_canonical, b, r)
        for k in ("dist", "bx", "by", "bz", "triIdx"):
            np.testing.assert_array_equal(hits.reshape(-1)[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
        np.testing.assert_array_equal(hits.reshape(-1)["blasIdx"] & 0x7fffffff, want["blasIdx"])
        # pixels: the full restatement (shadow rays and shading) on every pixel
        rpx, rhits, _, rn = cr.frame_from_rays(b, r, po.shade_params(), 1)
        np.testing.assert_array_equal(px.reshape(-1), rpx)
        np.testing.assert_array_equal(hits.reshape(-1)["blasIdx"], rhits["blasIdx"])
        assert n == rn
    finally:
        ds.close()


def test_camera_on_the_lds_staging_variant(vrt, gpu_device):
    """The same checks on the library with both LDS-staging variants on (built by build(); tests/test_gpu_variants.py's library)."""
    if LDS_VARIANT:
        return
    import importlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = importlib.import_module("vortex-raytracing_amd.build").build_test_variant()   # (rebuilt when a source or header is newer)
    env = dict(os.environ, VXRT_LIB_DIR=lib, VXRT_CAMERA_TEST_VARIANT="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                        "not lds_staging and not 1080p"], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def _tracer_frame(vrt, sc, w, h, camera, spp=1, row_window=None, shadow=True, quirks=False, stride=0):
    tr = vrt.tracer.Tracer(w, h, samples_per_pixel=spp)
    tr.init(sc)
    try:
        tr.setup(row_window=row_window, shadow=shadow, camera=camera)
        if quirks:
            tr.dev.dcr_write(vrt.runtime.VX_DCR_HIP_REFERENCE_QUIRKS, 1)
        if stride:
            tr.dev.dcr_write(vrt.runtime.VX_DCR_HIP_ROW_STRIDE, stride)
        return tr.run()
    finally:
        if quirks:
            tr.dev.dcr_write(vrt.runtime.VX_DCR_HIP_REFERENCE_QUIRKS, 0)
        tr.close()


def test_vx_boundary_camera(vrt, po, gpu_device):
    """Tracer.setup(camera=...) through vx_start (DCR 0x7F5) gives vxrt_render_camera's frame; without a camera, today's frame."""
    if LDS_VARIANT:
        return
    import torch
    sc = vrt.scene.procedural("cornell")
    w, h = 64, 48
    cam = np.array(vrt.rtapi.look_at((-2.0, 3.0, -12.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 0.9, w, h).cam14(), np.float32)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    try:
        p = vrt.rtapi.default_shade_params()
        p.light_pos[:] = vrt.tracer.DEFAULT_LIGHT_POS
        p.light_color[:] = vrt.tracer.DEFAULT_LIGHT_COLOR
        p.ambient[:] = vrt.tracer.DEFAULT_AMBIENT
        p.background[:] = vrt.tracer.DEFAULT_BACKGROUND
        want = _host_frame(*_render_camera(vrt, ds, cam, w, h, p, 1), w, h, 0, h)[0]
        fixed = torch.zeros((h, w), dtype=torch.int32, device=gpu_device)
        vrt.rtapi.render(ds.accel, w, h, 0, h, p, fixed.data_ptr(), 1, None, None, None, _stream())
        torch.cuda.synchronize()
        fixed = fixed.cpu().numpy().view(np.uint32)
    finally:
        ds.close()
    assert (want != fixed).any()   # (the camera sees another view)
    np.testing.assert_array_equal(_tracer_frame(vrt, sc, w, h, cam), want)
    np.testing.assert_array_equal(_tracer_frame(vrt, sc, w, h, cam, spp=3), want)               # samples: one set of launches
    np.testing.assert_array_equal(_tracer_frame(vrt, sc, w, h, cam, row_window=(9, 30))[9:30], want[9:30])
    np.testing.assert_array_equal(_tracer_frame(vrt, sc, w, h, cam, spp=2, row_window=(16, 40))[16:40], want[16:40])
    np.testing.assert_array_equal(_tracer_frame(vrt, sc, w, h, None), fixed)                      # DCR 0x7F5 = 0: today's frame
    np.testing.assert_array_equal(_tracer_frame(vrt, sc, w, h, None, shadow=False), po.render(sc, w, h)[0])
    with pytest.raises(Exception):
        _tracer_frame(vrt, sc, w, h, cam, shadow=False, quirks=True)    # no camera form of the reference-quirks mode
    with pytest.raises(Exception):
        _tracer_frame(vrt, sc, w, h, cam, row_window=(8, h), stride=2)  # no interleaved camera form
    bad = cam.copy()
    bad[4] = np.inf
    with pytest.raises(Exception):
        _tracer_frame(vrt, sc, w, h, bad)
