"""GPU: the alpha test (vxrt_accel_set_alpha_test) against the restatement tests/alpha_ref.py on the cases of tests/alpha_cases.py,
bit for bit: hit records of vxrt_trace (closest and any-hit, with and without tmax, the EXACT launch's axis-parallel rays included),
and hits (with bit 31), colours, pixels and rays traced of vxrt_render / vxrt_render_camera with shadow 0 and 1.  No tolerance
anywhere.  tests/test_alpha_cpu.py pins the restatement and shows that the cases are not vacuous."""
import ctypes as C

import numpy as np
import pytest

import alpha_cases as ac
import alpha_ref as ar
import camera_ref as cr
import refit_ref
from camera_ref import po

pytestmark = pytest.mark.gpu
W, H = ac.W, ac.H
MARK = 0x5A5A5A


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _params(vrt, p):
    q = vrt.rtapi.default_shade_params()
    q.ambient[:], q.light_color[:], q.light_pos[:], q.background[:] = tuple(p.ambient), tuple(p.light_color), tuple(p.light_pos), tuple(p.background)
    q.max_depth = p.max_depth
    return q


def _trace(vrt, ds, rays, tmax=None, any_hit=False, stream=None):
    import torch
    dev = ds.t["tri"].device
    r = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(dev)
    t = torch.from_numpy(np.ascontiguousarray(tmax, np.float32)).to(dev) if tmax is not None else None
    out = torch.full((len(rays), 6), 0x7B, dtype=torch.int32, device=dev)
    vrt.rtapi.trace(ds.accel, r.data_ptr(), len(rays), out.data_ptr(), vrt.rtapi.MODE_ANY if any_hit else vrt.rtapi.MODE_CLOSEST,
                    t.data_ptr() if t is not None else None, _stream() if stream is None else stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(po.HIT_DTYPE).reshape(-1)


def _outputs(dev):
    import torch
    return (torch.full((H, W), MARK, dtype=torch.int32, device=dev), torch.zeros((H * W, 6), dtype=torch.int32, device=dev),
            torch.zeros(H * W * 3, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def _render(vrt, ds, cam, p, shadow, stream=None, out=None):
    px, hits, col, cnt = out = out or _outputs(ds.t["tri"].device)
    s = _stream() if stream is None else stream
    if cam is None:
        vrt.rtapi.render(ds.accel, W, H, 0, H, p, px.data_ptr(), shadow, hits.data_ptr(), col.data_ptr(), cnt.data_ptr(), s)
    else:
        vrt.rtapi.render_camera(ds.accel, cam, W, H, 0, H, p, px.data_ptr(), shadow, hits.data_ptr(), col.data_ptr(), cnt.data_ptr(), s)
    return out


def _frame(out):
    import torch
    torch.cuda.synchronize()
    px, hits, col, cnt = out
    return (px.cpu().numpy().view(np.uint32).reshape(-1), hits.cpu().numpy().view(po.HIT_DTYPE).reshape(-1), col.cpu().numpy().reshape(-1, 3),
            int(cnt.item()))


def _check_frame(got, want, what):
    px, hits, col, n = got
    rpx, rhits, rcol, rn = want[:4]
    assert hits.tobytes() == rhits.tobytes(), "%s: hit records differ at %s" % (what, np.nonzero(hits != rhits)[0][:8])
    np.testing.assert_array_equal(col.view(np.uint32), rcol.view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(px, rpx, err_msg=what + ": pixels")
    assert n == rn, "%s: rays traced %d, restatement %d" % (what, n, rn)


@pytest.fixture(scope="module")
def dev_scene(vrt, gpu_device):
    """the frame cases' device scenes, built on first use, with their tables set"""
    made = {}

    def get(name):
        if name not in made:
            ds = vrt.tracer.DeviceScene(ac.case(name)["scene"], gpu_device)
            ds.set_alpha_test(ac.case(name)["thresholds"])
            made[name] = ds
        return made[name]
    yield get
    for ds in made.values():
        ds.close()


@pytest.mark.parametrize("name", ac.FRAME_CASES)
@pytest.mark.parametrize("any_hit", [False, True])
def test_trace(vrt, dev_scene, name, any_hit):
    ds = dev_scene(name)
    assert vrt.rtapi.accel_info(ds.accel, 4) == 1
    rays, tmax = ac.ray_buffer(name)
    for with_tmax in (False, True):
        got = _trace(vrt, ds, rays, tmax if with_tmax else None, any_hit)
        want = ac.ref_trace(name, any_hit, with_tmax)[0]
        assert got.tobytes() == want.tobytes(), "%s any=%s tmax=%s: rays %s" % (name, any_hit, with_tmax, np.nonzero(got != want)[0][:8])
    assert vrt.rtapi.status(_stream()) == 0


@pytest.mark.parametrize("seed,family", ac.HOSTILE)
def test_trace_hostile_textures(vrt, gpu_device, seed, family):
    c = ac.hostile(seed, family)
    ds = vrt.tracer.DeviceScene(c["scene"], gpu_device)
    try:
        ds.set_alpha_test(c["thresholds"])
        tr = ar.tracer(c["scene"], c["thresholds"])
        for any_hit in (False, True):
            assert _trace(vrt, ds, c["rays"], None, any_hit).tobytes() == tr(c["rays"], None, any_hit).tobytes()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()


@pytest.mark.parametrize("name", ac.FRAME_CASES)
@pytest.mark.parametrize("shadow", [0, 1])
def test_frames(vrt, dev_scene, name, shadow):
    """vxrt_render (the fixed camera) and vxrt_render_camera (the case's other cameras)"""
    ds = dev_scene(name)
    c = ac.case(name)
    p = _params(vrt, c["params"])
    for cam_name, cam in c["cams"].items():
        got = _frame(_render(vrt, ds, cam, p, shadow))
        assert vrt.rtapi.status(_stream()) == 0
        _check_frame(got, ac.ref_frame(name, cam_name, shadow), "%s %s shadow=%d" % (name, cam_name, shadow))


@pytest.mark.parametrize("name", ac.FRAME_CASES)
def test_switching_the_table_off_restores_the_opaque_outputs(vrt, gpu_device, name):
    c = ac.case(name)
    ds = vrt.tracer.DeviceScene(c["scene"], gpu_device)
    try:
        p = _params(vrt, c["params"])
        rays, tmax = ac.ray_buffer(name)
        cam_name = next(iter(c["cams"]))

        def outputs():
            return [_trace(vrt, ds, rays, tmax, any_hit).tobytes() for any_hit in (False, True)] + \
                   [tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in _frame(_render(vrt, ds, cam, p, 1))) for cam in (None, c["cams"][cam_name])]

        before = outputs()
        assert vrt.rtapi.accel_info(ds.accel, 4) == 0
        ds.set_alpha_test(c["thresholds"])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        assert outputs() != before
        ds.set_alpha_test(None)
        assert vrt.rtapi.accel_info(ds.accel, 4) == 0
        assert outputs() == before
        ds.set_alpha_test(c["thresholds"])
        ds.set_alpha_test(np.zeros(len(c["thresholds"]), np.uint8))
        assert vrt.rtapi.accel_info(ds.accel, 4) == 0
        assert outputs() == before
        # and the opaque outputs are the oracle's
        assert before[0] == po.trace_mt(po.trace_canonical, c["scene"], rays, tmax=tmax).tobytes()
    finally:
        ds.close()


def test_table_survives_set_transforms_and_refit(vrt, gpu_device):
    import torch
    c = ac.case("mirror_hall")
    ds = vrt.tracer.DeviceScene(c["scene"], gpu_device)
    try:
        ds.set_alpha_test(c["thresholds"])
        p = _params(vrt, c["params"])
        cam = c["cams"]["orbit_1"]
        m = np.eye(4, dtype=np.float32)
        m[0, 3], m[1, 3], m[2, 3] = -30.0, 12.0, 25.0
        ds.set_transforms([m], first=3)
        host = {k: ds.t[k].cpu().numpy().copy() for k in ac.KEYS}
        # (the moved scene as the refit restatement makes it: the device's buffers are the same bytes)
        want = {k: c["scene"][k].copy() for k in ac.KEYS}
        want["blas"] = refit_ref.set_transforms(want["blas"], 3, [m])
        want["tlas"], want["bvh"] = (x.view(np.uint8).reshape(-1) for x in refit_ref.refit(want, geometry=False))
        for k in ("tlas", "blas"):
            assert host[k].tobytes() == want[k].tobytes()
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        tr = ar.tracer(host, c["thresholds"])
        _check_frame(_frame(_render(vrt, ds, cam, p, 1)), ar.frame_from_rays(host, tr, cr.rays(cam, W, H), c["params"], 1), "after set_transforms")
        ds.t["tri"].view(torch.float32).mul_(1.01)
        ds.refit(geometry=True)
        host = {k: ds.t[k].cpu().numpy().copy() for k in ac.KEYS}
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        tr = ar.tracer(host, c["thresholds"])
        _check_frame(_frame(_render(vrt, ds, cam, p, 1)), ar.frame_from_rays(host, tr, cr.rays(cam, W, H), c["params"], 1), "after refit")
        rays, tmax = ac.ray_buffer("mirror_hall")
        assert _trace(vrt, ds, rays[:1500], tmax[:1500]).tobytes() == tr(rays[:1500], tmax[:1500]).tobytes()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()


def _lib(vrt):
    L = vrt.rtapi._lib()
    L.vxrt_accel_set_alpha_test.restype = C.c_int
    L.vxrt_accel_set_alpha_test.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def test_set_alpha_test_refusals(vrt, gpu_device):
    import torch
    c = ac.case("mirror_hall")
    ds = vrt.tracer.DeviceScene(c["scene"], gpu_device)
    try:
        L = _lib(vrt)
        thr = (C.c_uint8 * len(c["thresholds"]))(*[int(t) for t in c["thresholds"]])
        n = len(c["thresholds"])
        assert L.vxrt_accel_set_alpha_test(None, thr, n, _stream()) == -1
        assert L.vxrt_accel_set_alpha_test(ds.accel, thr, n - 1, _stream()) == -1
        assert L.vxrt_accel_set_alpha_test(ds.accel, thr, n + 1, _stream()) == -1
        bad = (C.c_uint8 * n)(*([7] + [0] * (n - 1)))          # material 0 has no texture
        assert L.vxrt_accel_set_alpha_test(ds.accel, bad, n, _stream()) == -1
        assert vrt.rtapi.accel_info(ds.accel, 4) == 0
        # a refusal while a table is set leaves that table in force
        ds.set_alpha_test(c["thresholds"])
        assert L.vxrt_accel_set_alpha_test(ds.accel, bad, n, _stream()) == -1
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        p = _params(vrt, c["params"])
        _check_frame(_frame(_render(vrt, ds, None, p, 0)), ac.ref_frame("mirror_hall", "fixed", 0), "table kept")
        # a stale accel
        v = ds.t["tri"].view(torch.float32).view(-1, 3, 3)
        v[0, 0, 0], v[1, 1, 0] = -3e38, 3e38
        with pytest.raises(Exception):
            ds.refit(geometry=True)
        assert L.vxrt_accel_set_alpha_test(ds.accel, thr, n, _stream()) == -1
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()


def test_entry_points_that_refuse_while_a_table_is_set(vrt, dev_scene):
    """every tracing entry point other than vxrt_trace / vxrt_render / vxrt_render_camera: -1, dst untouched, status 0"""
    import torch
    ds = dev_scene("mirror_hall")
    dev = ds.t["tri"].device
    L = vrt.rtapi._lib()
    R = vrt.rtapi
    p = R.default_shade_params()
    pp = C.byref(p)
    parr = (R.ShadeParams * 2)(p, p)
    cam = R.Camera.from_cam14(ac.case("mirror_hall")["cams"]["orbit_1"])
    cams = (R.Camera * 2)(cam, cam)
    ao = R.AoParams(4, 40.0, 0, 0)
    px = torch.full((2, H, W), MARK, dtype=torch.int32, device=dev)
    cnt = torch.zeros(16, dtype=torch.int64, device=dev)
    log = torch.zeros(16 * 8192, dtype=torch.int64, device=dev)
    rays = torch.from_numpy(ac.ray_buffer("mirror_hall")[0][:256].copy()).to(dev)
    hits = torch.full((256, 6), MARK, dtype=torch.int32, device=dev)
    u32, vp, i32, u64 = C.c_uint32, C.c_void_p, C.c_int, C.c_uint64
    s, d, n = _stream(), px.data_ptr(), cnt.data_ptr()
    SP, CP, AP = C.POINTER(R.ShadeParams), C.POINTER(R.Camera), C.POINTER(R.AoParams)
    calls = [
        ("vxrt_render_interleaved", [vp, u32, u32, u32, u32, SP, i32, vp, vp, vp, vp, vp], (ds.accel, W, H, 0, 1, pp, 0, d, None, None, None, s)),
        ("vxrt_render_interleaved", None, (ds.accel, W, H, 1, 2, pp, 1, d, None, None, None, s)),
        ("vxrt_render_interleaved_batch", [vp, u32, u32, u32, u32, u32, SP, i32, vp, u64, vp, vp], (ds.accel, W, H, 0, 1, 2, parr, 0, d, W * H, None, s)),
        ("vxrt_render_rows_batch", [vp, u32, u32, u32, u32, u32, SP, i32, vp, u64, vp, vp], (ds.accel, W, H, 0, H, 2, parr, 0, d, W * H, None, s)),
        ("vxrt_render_rows_batch", None, (ds.accel, W, H, 0, H, 1, parr, 0, d, W * H, None, s)),
        ("vxrt_render_batch", [vp, u32, u32, u32, SP, i32, vp, u64, vp, vp], (ds.accel, W, H, 2, parr, 1, d, W * H, None, s)),
        ("vxrt_render_batch_camera", [vp, u32, u32, u32, CP, SP, i32, vp, u64, vp, vp], (ds.accel, W, H, 2, cams, parr, 0, d, W * H, None, s)),
        ("vxrt_render_stats", [vp, u32, u32, u32, u32, SP, i32, vp, vp, vp], (ds.accel, W, H, 0, H, pp, 0, d, n, s)),
        ("vxrt_render_stats_timed", [vp, u32, u32, u32, u32, SP, i32, vp, vp, vp], (ds.accel, W, H, 0, H, pp, 1, d, n, s)),
        ("vxrt_render_wave_log", [vp, u32, u32, u32, u32, SP, i32, vp, vp, vp, vp], (ds.accel, W, H, 0, H, pp, 0, d, n, log.data_ptr(), s)),
        ("vxrt_render_interleaved_batch_wave_log", [vp, u32, u32, u32, u32, u32, SP, i32, vp, u64, vp, vp, vp],
         (ds.accel, W, H, 0, 1, 2, parr, 0, d, W * H, n, log.data_ptr(), s)),
        ("vxrt_render_ao", [vp, u32, u32, u32, u32, SP, AP, vp, vp, vp, vp, vp], (ds.accel, W, H, 0, H, pp, C.byref(ao), d, None, None, None, s)),
        ("vxrt_render_ao_camera", [vp, CP, u32, u32, u32, u32, SP, AP, vp, vp, vp, vp, vp], (ds.accel, C.byref(cam), W, H, 0, H, pp, C.byref(ao), d, None, None, None, s)),
        ("vxrt_render_diffuse_bounce", [vp, u32, u32, u32, u32, SP, u32, vp, vp, vp, vp], (ds.accel, W, H, 0, H, pp, 0, d, None, None, s)),
        ("vxrt_render_diffuse_bounce_camera", [vp, CP, u32, u32, u32, u32, SP, u32, vp, vp, vp, vp], (ds.accel, C.byref(cam), W, H, 0, H, pp, 0, d, None, None, s)),
        ("vxrt_trace_stats", [vp, vp, u64, vp, vp, i32, vp, vp], (ds.accel, rays.data_ptr(), 256, None, hits.data_ptr(), 0, n, s)),
    ]
    for name, argtypes, args in calls:
        fn = getattr(L, name)
        if argtypes is not None:
            fn.restype, fn.argtypes = C.c_int, argtypes
        assert fn(*args) == -1, name
    torch.cuda.synchronize()
    assert (px.cpu().numpy() == MARK).all() and (hits.cpu().numpy() == MARK).all() and (cnt.cpu().numpy() == 0).all()
    assert vrt.rtapi.status(_stream()) == 0
    # ... and the three that honour the table still run
    _check_frame(_frame(_render(vrt, ds, None, _params(vrt, ac.case("mirror_hall")["params"]), 1)), ac.ref_frame("mirror_hall", "fixed", 1), "after the refusals")


def test_two_frames_in_flight(vrt, dev_scene):
    import torch
    ds = dev_scene("mirror_hall")
    c = ac.case("mirror_hall")
    dev = ds.t["tri"].device
    p = _params(vrt, c["params"])
    names = ["orbit_1", "inside_blob"]
    serial = [_frame(_render(vrt, ds, c["cams"][k], p, 1)) for k in names]
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        outs = [_outputs(dev) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(2):
            _render(vrt, ds, c["cams"][names[i]], p, 1, streams[i].cuda_stream, outs[i])
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
        for i in range(2):
            _check_frame(_frame(outs[i]), serial[i], "in flight %d" % i)
            _check_frame(serial[i], ac.ref_frame("mirror_hall", names[i], 1), "serial %d" % i)
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)
