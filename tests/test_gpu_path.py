"""GPU: path-traced frames (vxrt_render_path) against the restatement tests/path_ref.py, bit for bit: pixels, f32 colours as u32 and rays
traced.  No masks, no tolerances.  tests/test_path_cpu.py pins the restatement to the two identities of the definition and shows that
the cases below are not vacuous."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_ref as cr
import camera_secondary_ref as csr
import path_ref as pr
import scenes

pytestmark = pytest.mark.gpu
W, H = pr.W, pr.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
BATCH_CHILD = os.environ.get("VXRT_PATH_TEST_CHILD") == "1"


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _outputs(dev, w, h):
    """pixels (marker-filled), colours, ray counter of a w x h frame"""
    import torch
    return (torch.full((h, w), MARK, dtype=torch.int32, device=dev), torch.zeros(h * w * 3, dtype=torch.float32, device=dev),
            torch.zeros(1, dtype=torch.int64, device=dev))


def _path(vrt, ds, cam, w, h, spp, bounces, seed=0, shadow=0, y0=0, y1=None, stream=None, out=None):
    px, col, cnt = out = out or _outputs(ds.t["tri"].device, w, h)
    vrt.rtapi.render_path(ds.accel, cam, w, h, y0, h if y1 is None else y1, vrt.rtapi.default_shade_params(), spp, bounces, px.data_ptr(), seed, shadow,
                          col.data_ptr(), cnt.data_ptr(), _stream() if stream is None else stream)
    return out


def _frame(out, w, h, y0=0, y1=None):
    import torch
    y1 = h if y1 is None else y1
    torch.cuda.synchronize()
    px, col, cnt = out
    return px.cpu().numpy().view(np.uint32)[y0:y1], col.cpu().numpy().reshape(h, w, 3)[y0:y1], int(cnt.item())


def _check(got, want, what):
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": pixels")
    assert got[2] == want[2], "%s: rays traced %d, restatement %d" % (what, got[2], want[2])


def _against_ref(vrt, po, b, ds, cam, what, w=W, h=H, y0=0, y1=None, configs=pr.CONFIGS, seeds=None):
    """the configurations (spp, bounces, shadow, seed) from `cam` against the restatement, the primary hits traced once on the CPU"""
    y1 = h if y1 is None else y1
    prim = pr.primary(b, po.camera_rays(w, h, y0, y1) if cam is None else cr.rays(cam, w, h, y0, y1))
    for spp, bounces, shadow, seed0 in configs:
        for seed in (seeds or (seed0,)):
            got = _frame(_path(vrt, ds, cam, w, h, spp, bounces, seed, shadow, y0, y1), w, h, y0, y1)
            assert vrt.rtapi.status(_stream()) == 0
            _check(got, pr.frame(b, cam, w, h, po.shade_params(), spp, bounces, seed, shadow, y0, y1, prim),
                   "%s spp=%d bounces=%d shadow=%d seed=%d" % (what, spp, bounces, shadow, seed))


@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    yield b, ds
    ds.close()


@pytest.mark.parametrize("name", csr.HALL_CAMERA_NAMES)
def test_hall_cameras(vrt, po, hall, name):
    b, ds = hall
    _against_ref(vrt, po, b, ds, csr.hall_cameras(vrt)[name], name, seeds=(3, 0))


@pytest.mark.parametrize("name", ["framing", "orbit_1", "inside_blob", None])
def test_one_bounce_is_the_diffuse_bounce_frame(vrt, hall, name):
    """bounces = 1, spp = 1, shadow = 0 against the GPU's own vxrt_render_diffuse_bounce[_camera]: colours, pixels, rays traced"""
    b, ds = hall
    cam = None if name is None else csr.hall_cameras(vrt)[name]
    p = vrt.rtapi.default_shade_params()
    for seed in (0, 7):
        px, col, cnt = _outputs(ds.t["tri"].device, W, H)
        if cam is None:
            vrt.rtapi.render_diffuse_bounce(ds.accel, W, H, 0, H, p, px.data_ptr(), seed, col.data_ptr(), cnt.data_ptr(), _stream())
        else:
            vrt.rtapi.render_diffuse_bounce_camera(ds.accel, cam, W, H, 0, H, p, px.data_ptr(), seed, col.data_ptr(), cnt.data_ptr(), _stream())
        want = _frame((px, col, cnt), W, H)
        got = _frame(_path(vrt, ds, cam, W, H, 1, 1, seed, 0), W, H)
        assert vrt.rtapi.status(_stream()) == 0
        _check(got, want, "%s seed %d" % (name, seed))
        assert got[2] > W * H or name is None


@pytest.mark.parametrize("name", ["framing", "orbit_1", "inside_blob", None])
@pytest.mark.parametrize("shadow", [0, 1])
def test_no_bounce_is_the_direct_frame(vrt, hall, name, shadow):
    """bounces = 0 against the GPU's own vxrt_render[_camera] with max_depth = 1, for the spp whose sum and division are exact"""
    b, ds = hall
    cam = None if name is None else csr.hall_cameras(vrt)[name]
    p = vrt.rtapi.default_shade_params()
    px, col, cnt = _outputs(ds.t["tri"].device, W, H)
    if cam is None:
        vrt.rtapi.render(ds.accel, W, H, 0, H, p, px.data_ptr(), shadow, None, col.data_ptr(), cnt.data_ptr(), _stream())
    else:
        vrt.rtapi.render_camera(ds.accel, cam, W, H, 0, H, p, px.data_ptr(), shadow, None, col.data_ptr(), cnt.data_ptr(), _stream())
    want = _frame((px, col, cnt), W, H)
    for spp in (1, 2, 4):
        got = _frame(_path(vrt, ds, cam, W, H, spp, 0, 5, shadow), W, H)
        assert vrt.rtapi.status(_stream()) == 0
        _check(got, want, "%s shadow %d spp %d" % (name, shadow, spp))


def test_fixed_camera(vrt, po, hall):
    b, ds = hall
    _against_ref(vrt, po, b, ds, None, "fixed camera")


def test_axis_aligned_odd_size(vrt, po, hall):
    """13 x 7: the centre column and row of the axis-aligned camera have a zero direction component (deferred to the EXACT launch)"""
    b, ds = hall
    _against_ref(vrt, po, b, ds, csr.hall_cameras(vrt, 13, 7)["axis_aligned"], "13x7 axis_aligned", 13, 7)


def test_row_window_leaves_the_other_rows(vrt, po, hall):
    b, ds = hall
    cam = csr.orbit(vrt, 2)
    _against_ref(vrt, po, b, ds, cam, "rows 13..43", y0=13, y1=43)
    px = _frame(_path(vrt, ds, cam, W, H, 2, 3, 3, 1, 13, 43), W, H)[0]
    assert (px[:13] == MARK).all() and (px[43:] == MARK).all() and (px[13:43] != MARK).any()


@pytest.mark.parametrize("name", ["tex_mix", "teapot_x3"])
def test_textured_scenes(vrt, po, golden, gpu_device, name):
    g = golden(name)
    b = {k: g[k] for k in KEYS}
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        for cname, cam in csr.golden_cameras(vrt).items():
            _against_ref(vrt, po, b, ds, cam, name + " " + cname)
    finally:
        ds.close()


def test_deep_chain(vrt, po, gpu_device):
    """scenes.chain_bvh4(20): deeper than 16 levels, the deep-stack class of the ray-buffer launch"""
    sc = scenes.chain_bvh4(vrt, 20)
    b = {k: np.frombuffer(bytes(sc.buffers[k]), np.uint8).copy() for k in KEYS}
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    try:
        assert vrt.rtapi.accel_info(ds.accel, 1) == 0
        _against_ref(vrt, po, b, ds, csr.chain_camera(vrt), "chain20")
    finally:
        ds.close()


def test_sixteen_bounces(vrt, po, hall):
    b, ds = hall
    _against_ref(vrt, po, b, ds, csr.hall_cameras(vrt)["inside_blob"], "16 bounces", configs=((1, 16, 1, 0),))


def test_one_bounce_against_the_restatement(vrt, po, hall):
    """bounces = 1: the batch's first depth is its last, so the only scatter launch compacts nothing; with and without light sampling"""
    b, ds = hall
    _against_ref(vrt, po, b, ds, csr.hall_cameras(vrt)["orbit_1"], "one bounce", configs=((2, 1, 1, 3), (2, 1, 0, 0)))


def test_batches_of_two_two_and_one_samples(vrt, po, hall, gpu_device):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs this test's body with 2 * W * H paths per batch, so that spp = 5
    takes batches of 2, 2 and 1 samples"""
    if not BATCH_CHILD:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, VXRT_PATH_BATCH=str(2 * W * H), VXRT_PATH_TEST_CHILD="1")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "batches_of_two"],
                           env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
        return
    b, ds = hall
    assert os.environ["VXRT_PATH_BATCH"] == str(2 * W * H)
    _against_ref(vrt, po, b, ds, csr.hall_cameras(vrt)["orbit_1"], "batched", configs=((5, 2, 1, 0), (5, 2, 0, 3)))


def test_two_frames_in_flight(vrt, po, hall):
    import torch
    b, ds = hall
    dev = ds.t["tri"].device
    pp = po.shade_params()
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cams = [csr.orbit(vrt, 1), csr.orbit(vrt, 6)]
        seeds = (3, 11)
        outs = [_outputs(dev, W, H) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(2):
            _path(vrt, ds, cams[i], W, H, 2, 3, seeds[i], 1, stream=streams[i].cuda_stream, out=outs[i])
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
        for i in range(2):
            _check(_frame(outs[i], W, H), pr.frame(b, cams[i], W, H, pp, 2, 3, seeds[i], 1), "in flight %d" % i)
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)


def _prototype(vrt):
    L = vrt.rtapi._lib()
    L.vxrt_render_path.restype = C.c_int
    L.vxrt_render_path.argtypes = [C.c_void_p, C.POINTER(vrt.rtapi.Camera)] + [C.c_uint32] * 4 + [C.POINTER(vrt.rtapi.ShadeParams),
                                   C.POINTER(vrt.rtapi.PathParams)] + [C.c_void_p] * 4
    return L


def _call(vrt, L, accel, px, cam, y0=0, y1=H, params="default", path="default"):
    p = vrt.rtapi.default_shade_params()
    pref = C.byref(p) if params == "default" else params
    q = vrt.rtapi.PathParams(2, 3, 0, 1)
    qref = C.byref(q) if path == "default" else (C.byref(path) if path is not None else None)
    cref = C.byref(cam) if cam is not None else None
    return L.vxrt_render_path(accel, cref, W, H, y0, y1, pref, qref, px.data_ptr(), None, None, _stream())


def test_refusals(vrt, hall):
    import torch
    b, ds = hall
    L = _prototype(vrt)
    px = torch.full((H, W), MARK, dtype=torch.int32, device=ds.t["tri"].device)
    base = csr.framing(W, H)
    good = vrt.rtapi.Camera.from_cam14(base)
    PP = vrt.rtapi.PathParams
    assert _call(vrt, L, ds.accel, px, good, path=None) == -1
    for bad in (PP(0, 3, 0, 1), PP(4097, 3, 0, 1), PP(2, vrt.rtapi.PATH_MAX_BOUNCES + 1, 0, 1), PP(2, 3, 0, 2)):
        for cam in (good, None):
            assert _call(vrt, L, ds.accel, px, cam, path=bad) == -1
    for i in range(14):
        for v in (float("nan"), float("inf"), -float("inf")):
            c = base.copy()
            c[i] = v
            assert _call(vrt, L, ds.accel, px, vrt.rtapi.Camera.from_cam14(c)) == -1
    for cam in (good, None):
        assert _call(vrt, L, ds.accel, px, cam, y0=5, y1=3) == -1        # what vxrt_render refuses for the window
        assert _call(vrt, L, ds.accel, px, cam, y0=0, y1=H + 1) == -1
        assert _call(vrt, L, ds.accel, px, cam, params=None) == -1
        assert _call(vrt, L, None, px, cam) == -1
        assert _call(vrt, L, ds.accel, px, cam, y0=7, y1=7) == 0         # the empty window
    torch.cuda.synchronize()
    assert (px.cpu().numpy() == MARK).all()
    assert vrt.rtapi.status(_stream()) == 0


def test_alpha_table_is_refused(vrt, golden, gpu_device):
    import torch
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in KEYS}, gpu_device)
    try:
        n_mats = len(bytes(g["mat"])) // 88
        import shading_ref as sr
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        assert len(mat) == n_mats and (mat["tex_id"] >= 0).any()
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        L = _prototype(vrt)
        cam = vrt.rtapi.Camera.from_cam14(csr.golden_cameras(vrt)["g_orbit_1"])
        assert _call(vrt, L, ds.accel, px, cam) == -1
        assert _call(vrt, L, ds.accel, px, None) == -1
        ds.set_alpha_test(None)
        assert _call(vrt, L, ds.accel, px, cam) == 0
        torch.cuda.synchronize()
        assert (px.cpu().numpy() != MARK).all()
    finally:
        ds.close()


def test_stale_accel_is_refused(vrt, gpu_device):
    import torch
    ds = vrt.tracer.DeviceScene(scenes.mirror_hall(vrt), gpu_device)
    try:
        v = ds.t["tri"].view(torch.float32).view(-1, 3, 3)
        v[0, 0, 0], v[1, 1, 0] = -3e38, 3e38   # the extent overflows fp32: the refit fails and leaves the accel stale
        with pytest.raises(Exception):
            ds.refit(geometry=True)
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        L = _prototype(vrt)
        assert _call(vrt, L, ds.accel, px, vrt.rtapi.Camera.from_cam14(csr.framing(W, H))) == -1
        assert _call(vrt, L, ds.accel, px, None) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
    finally:
        ds.close()
