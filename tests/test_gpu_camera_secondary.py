"""GPU: ambient-occlusion and diffuse-bounce frames from a caller-supplied pinhole camera (vxrt_render_ao_camera,
vxrt_render_diffuse_bounce_camera) against the restatement tests/camera_secondary_ref.py, bit for bit: pixels, f32 colours as u32,
unoccluded counts and rays traced.  No masks, no tolerances.  tests/test_camera_secondary_cpu.py pins the restatement to the oracle
and shows that the cases below are not vacuous (the radii are chosen there).

What the deferral check can see: the diffuse-bounce frame leaves its control block as its launches left it, so word 0 is the number of
pixels its main launch deferred to the EXACT launch.  The ambient-occlusion frame's primary launch is the JOB_RENDER | JOB_CAM launch of
vxrt_render_camera, and the first kernel of its tail (unchanged by this feature) zeroes the control block for the occlusion-ray launch
that follows: the count of deferred PRIMARY rays is gone when the call returns.  For that pass the test asserts what remains
observable: the primary rays of those cameras are outside the fast domain (restated on the CPU) and their pixels are bit-equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_ref as cr
import camera_secondary_ref as csr
import scenes

pytestmark = pytest.mark.gpu
W, H = csr.W, csr.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
LDS_VARIANT = os.environ.get("VXRT_CAMERA_SECONDARY_TEST_VARIANT") == "1"


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _host(ds):
    return {k: ds.t[k].cpu().numpy().copy() for k in KEYS}


def _outputs(dev, w, h):
    """pixels (marker-filled), colours, unoccluded counts, ray counter of a w x h frame"""
    import torch
    return (torch.full((h, w), MARK, dtype=torch.int32, device=dev), torch.zeros(h * w * 3, dtype=torch.float32, device=dev),
            torch.full((h, w), 0x7777, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def _ao(vrt, ds, cam, w, h, p, spp, radius, seed=0, y0=0, y1=None, stream=None, out=None):
    px, col, opn, cnt = out = out or _outputs(ds.t["tri"].device, w, h)
    vrt.rtapi.render_ao_camera(ds.accel, cam, w, h, y0, h if y1 is None else y1, p, spp, radius, px.data_ptr(), seed, col.data_ptr(), opn.data_ptr(),
                               cnt.data_ptr(), _stream() if stream is None else stream)
    return out


def _gi(vrt, ds, cam, w, h, p, seed=0, y0=0, y1=None, stream=None, out=None):
    px, col, _, cnt = out = out or _outputs(ds.t["tri"].device, w, h)
    vrt.rtapi.render_diffuse_bounce_camera(ds.accel, cam, w, h, y0, h if y1 is None else y1, p, px.data_ptr(), seed, col.data_ptr(), cnt.data_ptr(),
                                           _stream() if stream is None else stream)
    return out


def _frame(out, w, h, y0=0, y1=None):
    import torch
    y1 = h if y1 is None else y1
    torch.cuda.synchronize()
    px, col, opn, cnt = out
    return (px.cpu().numpy().view(np.uint32)[y0:y1], col.cpu().numpy().reshape(h, w, 3)[y0:y1], opn.cpu().numpy().view(np.uint32)[y0:y1],
            int(cnt.item()))


def _check_ao(got, want, what):
    px, col, opn, n = got
    rpx, rcol, ropn, rn = want
    np.testing.assert_array_equal(opn, ropn, err_msg=what + ": unoccluded")
    np.testing.assert_array_equal(col.view(np.uint32), rcol.view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(px, rpx, err_msg=what + ": pixels")
    assert n == rn, "%s: rays traced %d, restatement %d" % (what, n, rn)


def _check_gi(got, want, what):
    px, col, _, n = got
    rpx, rcol, rn = want
    np.testing.assert_array_equal(col.view(np.uint32), rcol.view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(px, rpx, err_msg=what + ": pixels")
    assert n == rn, "%s: rays traced %d, restatement %d" % (what, n, rn)


def _both(vrt, po, b, ds, cam, radius, what, w=W, h=H, y0=0, y1=None, spps=(5,), seeds=(0,)):
    """both passes from `cam` against the restatement; returns the deferral counts of the bounce frames' main launches"""
    p, pp = vrt.rtapi.default_shade_params(), po.shade_params()
    y1 = h if y1 is None else y1
    prim = csr.primary(b, cr.rays(cam, w, h, y0, y1), pp)
    deferred = []
    for spp in spps:
        got = _frame(_ao(vrt, ds, cam, w, h, p, spp, radius, 0, y0, y1), w, h, y0, y1)
        assert vrt.rtapi.status(_stream()) == 0
        _check_ao(got, csr.ao_frame(b, cam, w, h, pp, spp, radius, 0, y0, y1, prim), "%s ao spp=%d" % (what, spp))
    for seed in seeds:
        got = _frame(_gi(vrt, ds, cam, w, h, p, seed, y0, y1), w, h, y0, y1)
        assert vrt.rtapi.status(_stream()) == 0
        deferred.append(int(vrt.rtapi.debug_read_control(ds.accel, 0, 32, _stream())[0]))
        _check_gi(got, csr.gi_frame(b, cam, w, h, pp, seed, y0, y1, prim), "%s bounce seed=%d" % (what, seed))
    return deferred


@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    yield b, ds
    ds.close()


@pytest.mark.parametrize("name", csr.HALL_CAMERA_NAMES)
def test_hall_cameras(vrt, po, hall, name):
    b, ds = hall
    cam = csr.hall_cameras(vrt)[name]
    deferred = _both(vrt, po, b, ds, cam, csr.hall_radius(name), name, spps=(5, 16), seeds=(0, 7))
    outside = int((~csr.in_fast_domain(cr.rays(cam, W, H))).sum())
    if name == "beyond_2_60":
        # every primary ray starts beyond 2^60: the main launch of the bounce frame defers every pixel (and the ambient-occlusion
        # frame's primary launch, which the control block no longer shows, gets the same rays: see the module's docstring)
        assert outside == W * H and deferred == [W * H, W * H]
    else:
        assert all(d >= outside for d in deferred)   # (a pixel whose BOUNCE ray leaves the fast domain is deferred too)


def test_axis_aligned_odd_size_defers_its_centre_lines(vrt, po, hall):
    """13 x 7: the centre column and row of the axis-aligned camera have a zero direction component, and most of them hit the hall"""
    b, ds = hall
    cam = csr.hall_cameras(vrt, 13, 7)["axis_aligned"]
    outside = ~csr.in_fast_domain(cr.rays(cam, 13, 7))
    assert outside.sum() == 13 + 7 - 1
    prim = csr.primary(b, cr.rays(cam, 13, 7), po.shade_params())
    assert outside[prim["fi"]].any()   # deferred primary rays that hit: their secondary rays come from the EXACT launch's hit
    deferred = _both(vrt, po, b, ds, cam, csr.RADIUS["mirror_hall"], "13x7 axis_aligned", 13, 7, spps=(5, 16), seeds=(0, 7))
    assert all(d >= 19 for d in deferred)


@pytest.mark.parametrize("name", ["tex_mix", "teapot_x3"])
def test_textured_scenes(vrt, po, golden, gpu_device, name):
    g = golden(name)
    b = {k: g[k] for k in KEYS}
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        for cname, cam in csr.golden_cameras(vrt).items():
            _both(vrt, po, b, ds, cam, csr.RADIUS[name], name + " " + cname, spps=(5,), seeds=(3,))
    finally:
        ds.close()


@pytest.mark.parametrize("w,h,y0,y1", [(1, 1, 0, 1), (13, 7, 0, 7), (96, 64, 11, 37), (96, 64, 3, 3)])
def test_smallest_shapes(vrt, po, hall, w, h, y0, y1):
    b, ds = hall
    cam = csr.orbit(vrt, 2, 8, w, h)
    if y0 == y1:   # the empty window: returns 0 and writes nothing
        p = vrt.rtapi.default_shade_params()
        for out in (_ao(vrt, ds, cam, w, h, p, 5, 40.0, 0, y0, y1), _gi(vrt, ds, cam, w, h, p, 0, y0, y1)):
            px, col, opn, n = _frame(out, w, h)
            assert (px == MARK).all() and (col == 0).all() and (opn == 0x7777).all() and n == 0
        return
    _both(vrt, po, b, ds, cam, csr.RADIUS["mirror_hall"], "%dx%d rows %d..%d" % (w, h, y0, y1), w, h, y0, y1)
    px = _frame(_ao(vrt, ds, cam, w, h, vrt.rtapi.default_shade_params(), 5, 40.0, 0, y0, y1), w, h)[0]
    assert (px[:y0] == MARK).all() and (px[y1:] == MARK).all()   # rows outside the window stay untouched


def test_optional_outputs(vrt, po, hall):
    import torch
    b, ds = hall
    cam = csr.orbit(vrt, 5)
    p = vrt.rtapi.default_shade_params()
    full = _frame(_ao(vrt, ds, cam, W, H, p, 5, 40.0, 9), W, H)
    px = torch.full((H, W), MARK, dtype=torch.int32, device=ds.t["tri"].device)
    vrt.rtapi.render_ao_camera(ds.accel, cam, W, H, 0, H, p, 5, 40.0, px.data_ptr(), 9, None, None, None, _stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(px.cpu().numpy().view(np.uint32), full[0])
    _check_ao(full, csr.ao_frame(b, cam, W, H, po.shade_params(), 5, 40.0, 9), "seed 9")
    px.fill_(MARK)
    vrt.rtapi.render_diffuse_bounce_camera(ds.accel, cam, W, H, 0, H, p, px.data_ptr(), 9, None, None, _stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(px.cpu().numpy().view(np.uint32), csr.gi_frame(b, cam, W, H, po.shade_params(), 9)[0])


def test_frames_in_flight_and_fixed_frames_untouched(vrt, po, hall):
    import torch
    b, ds = hall
    dev = ds.t["tri"].device
    p, pp = vrt.rtapi.default_shade_params(), po.shade_params()

    def fixed(stream):
        """the three fixed-camera / plain camera frames issued among the camera frames: AO, bounce, vxrt_render_camera"""
        o = [torch.zeros((H, W), dtype=torch.int32, device=dev) for _ in range(3)]
        vrt.rtapi.render_ao(ds.accel, W, H, 0, H, p, 5, 40.0, o[0].data_ptr(), 0, None, None, None, stream)
        vrt.rtapi.render_diffuse_bounce(ds.accel, W, H, 0, H, p, o[1].data_ptr(), 0, None, None, stream)
        vrt.rtapi.render_camera(ds.accel, csr.orbit(vrt, 3), W, H, 0, H, p, o[2].data_ptr(), 1, None, None, None, stream)
        return o

    before = fixed(_stream())
    torch.cuda.synchronize()
    before = [t.cpu().numpy().copy() for t in before]
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cams = [csr.orbit(vrt, 1), csr.orbit(vrt, 6)]
        outs = [_outputs(dev, W, H) for _ in range(4)]
        torch.cuda.synchronize()
        _gi(vrt, ds, cams[0], W, H, p, 0, stream=streams[0].cuda_stream, out=outs[0])
        _gi(vrt, ds, cams[1], W, H, p, 0, stream=streams[1].cuda_stream, out=outs[1])
        mid = fixed(streams[1].cuda_stream)
        _ao(vrt, ds, cams[0], W, H, p, 5, 40.0, stream=streams[0].cuda_stream, out=outs[2])
        _ao(vrt, ds, cams[1], W, H, p, 5, 40.0, stream=streams[1].cuda_stream, out=outs[3])
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
        for i in range(2):
            _check_gi(_frame(outs[i], W, H), csr.gi_frame(b, cams[i], W, H, pp, 0), "bounce in flight %d" % i)
            _check_ao(_frame(outs[2 + i], W, H), csr.ao_frame(b, cams[i], W, H, pp, 5, 40.0), "ao in flight %d" % i)
        for t, want in zip(mid, before):
            np.testing.assert_array_equal(t.cpu().numpy(), want)
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)
    after = fixed(_stream())
    torch.cuda.synchronize()
    for t, want in zip(after, before):
        np.testing.assert_array_equal(t.cpu().numpy(), want)
    np.testing.assert_array_equal(before[0].view(np.uint32), po.render_ao(b, W, H, pp, 5, 40.0, 0)[0])
    np.testing.assert_array_equal(before[1].view(np.uint32), po.render_gi(b, W, H, pp, 0)[0])


def test_after_set_transforms_and_refit(vrt, po, gpu_device):
    import torch
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        m = np.eye(4, dtype=np.float32)
        m[0, 3], m[1, 3], m[2, 3] = -30.0, 12.0, 25.0
        ds.set_transforms([m], first=3)
        cam = csr.orbit(vrt, 1)
        _both(vrt, po, _host(ds), ds, cam, csr.RADIUS["mirror_hall"], "after set_transforms")
        ds.t["tri"].view(torch.float32).mul_(1.01)
        ds.refit(geometry=True)
        _both(vrt, po, _host(ds), ds, cam, csr.RADIUS["mirror_hall"], "after refit")
    finally:
        ds.close()


def test_ldexp_decode_scene(vrt, po, golden, gpu_device):
    """inverted child boxes make the accel build select the ldexp decode / generic slab form (vxrt_accel_info 3)"""
    g = golden("teapot_x3")
    node = np.dtype([("o", "<f4", 3), ("e", "i1", 3), ("imask", "u1"), ("lf", "<u4"), ("ld", "<u4"), ("ch", "u1", (4, 7))])
    b = {k: g[k].copy() for k in KEYS}
    n = b["bvh"].view(node)
    swapped = 0
    for i in np.nonzero(n["ld"] == 0)[0][1::3]:
        ch = n["ch"][i]
        valid = np.nonzero(ch[:, 0] != 0)[0]
        if len(valid) and ch[int(valid[-1]), 1] != ch[int(valid[-1]), 4]:
            k = int(valid[-1])
            ch[k, 1], ch[k, 4] = ch[k, 4], ch[k, 1]
            swapped += 1
    assert swapped > 10
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        assert vrt.rtapi.accel_info(ds.accel, 3) == 1
        _both(vrt, po, b, ds, csr.golden_cameras(vrt)["g_orbit_1"], csr.RADIUS["teapot_x3"], "ldexp", seeds=(3,))
    finally:
        ds.close()


def test_deep_chain_is_not_shallow(vrt, po, gpu_device):
    """scenes.chain_bvh4(20): deeper than 16 levels, so the full-size stack form of the bounce kernel, from a camera looking down the chain"""
    sc = scenes.chain_bvh4(vrt, 20)
    b = {k: np.frombuffer(bytes(sc.buffers[k]), np.uint8).copy() for k in KEYS}
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    try:
        assert vrt.rtapi.accel_info(ds.accel, 1) == 0
        _both(vrt, po, b, ds, csr.chain_camera(vrt), csr.RADIUS["chain20"], "chain20", seeds=(1,))
        _both(vrt, po, b, ds, csr.framing(W, H), csr.RADIUS["chain20"], "chain20 head-on", seeds=(1,))
    finally:
        ds.close()


def _prototypes(vrt):
    L = vrt.rtapi._lib()
    cam_p, sp_p, ao_p = C.POINTER(vrt.rtapi.Camera), C.POINTER(vrt.rtapi.ShadeParams), C.POINTER(vrt.rtapi.AoParams)
    L.vxrt_render_ao_camera.restype = C.c_int
    L.vxrt_render_ao_camera.argtypes = [C.c_void_p, cam_p] + [C.c_uint32] * 4 + [sp_p, ao_p] + [C.c_void_p] * 5
    L.vxrt_render_diffuse_bounce_camera.restype = C.c_int
    L.vxrt_render_diffuse_bounce_camera.argtypes = [C.c_void_p, cam_p] + [C.c_uint32] * 4 + [sp_p, C.c_uint32] + [C.c_void_p] * 4
    return L


def _refused(vrt, L, accel, px, cam, y0=0, y1=H, params="default", ao="default", only_ao=False):
    """both entry points (the bounce one unless the case is about `ao`) return -1"""
    p = vrt.rtapi.default_shade_params()
    pref = C.byref(p) if params == "default" else params
    a = vrt.rtapi.AoParams(5, 40.0, 0, 0)
    aref = C.byref(a) if ao == "default" else (C.byref(ao) if ao is not None else None)
    cref = C.byref(cam) if cam is not None else None
    assert L.vxrt_render_ao_camera(accel, cref, W, H, y0, y1, pref, aref, px.data_ptr(), None, None, None, _stream()) == -1
    if not only_ao:
        assert L.vxrt_render_diffuse_bounce_camera(accel, cref, W, H, y0, y1, pref, 0, px.data_ptr(), None, None, _stream()) == -1


def test_refusals(vrt, hall):
    import torch
    b, ds = hall
    L = _prototypes(vrt)
    px = torch.full((H, W), MARK, dtype=torch.int32, device=ds.t["tri"].device)
    base = csr.framing(W, H)
    good = vrt.rtapi.Camera.from_cam14(base)
    _refused(vrt, L, ds.accel, px, None)
    for i in range(14):
        for bad in (float("nan"), float("inf"), -float("inf")):
            c = base.copy()
            c[i] = bad
            _refused(vrt, L, ds.accel, px, vrt.rtapi.Camera.from_cam14(c))
    _refused(vrt, L, ds.accel, px, good, y0=5, y1=3)
    _refused(vrt, L, ds.accel, px, good, params=None)
    _refused(vrt, L, ds.accel, px, good, ao=None, only_ao=True)
    for spp, radius in ((0, 40.0), (4097, 40.0), (5, 0.0), (5, -1.0), (5, float("nan"))):
        _refused(vrt, L, ds.accel, px, good, ao=vrt.rtapi.AoParams(spp, radius, 0, 0), only_ao=True)
    torch.cuda.synchronize()
    assert (px.cpu().numpy() == MARK).all()
    assert vrt.rtapi.status(_stream()) == 0


def test_stale_accel_is_refused(vrt, gpu_device):
    import torch
    ds = vrt.tracer.DeviceScene(scenes.mirror_hall(vrt), gpu_device)
    try:
        v = ds.t["tri"].view(torch.float32).view(-1, 3, 3)
        v[0, 0, 0], v[1, 1, 0] = -3e38, 3e38   # the extent overflows fp32: the refit fails and leaves the accel stale
        with pytest.raises(Exception):
            ds.refit(geometry=True)
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        _refused(vrt, _prototypes(vrt), ds.accel, px, vrt.rtapi.Camera.from_cam14(csr.framing(W, H)))
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
    finally:
        ds.close()


def test_on_the_lds_staging_variant(vrt, gpu_device):
    """The same checks on the library with both LDS-staging variants on (built by build(); tests/test_gpu_variants.py's library)."""
    if LDS_VARIANT:
        return
    import importlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = importlib.import_module("vortex-raytracing_amd.build").build_test_variant()   # (rebuilt when a source or header is newer)
    env = dict(os.environ, VXRT_LIB_DIR=lib, VXRT_CAMERA_SECONDARY_TEST_VARIANT="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "not lds_staging"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
