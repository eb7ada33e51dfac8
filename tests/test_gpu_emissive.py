"""GPU: emissive geometry (vxrt_accel_set_emitters, vxrt_emitter_rays, vxrt_render_path_emissive) against the restatement
tests/emissive_ref.py, bit for bit: the emitter table, the emitter rays, and of the frames pixels, f32 colours as u32 and rays traced.
No masks, no tolerances.  tests/test_emissive_cpu.py pins the restatement and shows that the cases below are not vacuous.

The identity "a scene without emissive materials renders as vxrt_render_path" is held for nee = 0 on scenes.mirror_hall.  For nee = 1
it cannot be posed: a table needs a pair whose material emits, so on such a scene none can be set and the frame is refused -- which is
what test_a_scene_without_emissive_materials asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_ref as cr
import camera_secondary_ref as csr
import emissive_cases as ec
import emissive_ref as er
import path_ref as pr
import scenes

pytestmark = pytest.mark.gpu
W, H = pr.W, pr.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
BATCH_CHILD = os.environ.get("VXRT_EMISSIVE_TEST_CHILD") == "1"


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _outputs(dev, w, h):
    import torch
    return (torch.full((h, w), MARK, dtype=torch.int32, device=dev), torch.zeros(h * w * 3, dtype=torch.float32, device=dev),
            torch.zeros(1, dtype=torch.int64, device=dev))


def _em(vrt, nee, scale=ec.SCALE):
    return vrt.rtapi.EmissiveParams(int(nee), float(scale), (C.c_uint32 * 2)(0, 0))


def _render(vrt, ds, cam, w, h, spp, bounces, seed, shadow, nee, y0=0, y1=None, stream=None, out=None, scale=ec.SCALE):
    px, col, cnt = out = out or _outputs(ds.t["tri"].device, w, h)
    vrt.rtapi.render_path_emissive(ds.accel, cam, w, h, y0, h if y1 is None else y1, vrt.rtapi.default_shade_params(), spp, bounces, _em(vrt, nee, scale),
                                   px.data_ptr(), seed, shadow, col.data_ptr(), cnt.data_ptr(), _stream() if stream is None else stream)
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


@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    b, ranges = ec.hall(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    pairs = vrt.rtapi.emitter_pairs(b, ranges)
    ds.set_emitters(pairs)
    assert vrt.rtapi.accel_info(ds.accel, 7) == len(pairs) == 4
    yield b, ds, er.table(b, pairs), pairs
    ds.close()


def _against_ref(vrt, po, hall, cam, what, w=W, h=H, y0=0, y1=None, configs=ec.CONFIGS):
    b, ds, tab, _ = hall
    y1 = h if y1 is None else y1
    prim = pr.primary(b, po.camera_rays(w, h, y0, y1) if cam is None else cr.rays(cam, w, h, y0, y1))
    for spp, bounces, shadow, seed, nee in configs:
        got = _frame(_render(vrt, ds, cam, w, h, spp, bounces, seed, shadow, nee, y0, y1), w, h, y0, y1)
        assert vrt.rtapi.status(_stream()) == 0
        _check(got, er.frame(b, cam, w, h, po.shade_params(), spp, bounces, seed, shadow, nee, ec.SCALE, tab, y0, y1, prim),
               "%s spp=%d bounces=%d shadow=%d seed=%d nee=%d" % (what, spp, bounces, shadow, seed, nee))


@pytest.mark.parametrize("name", csr.HALL_CAMERA_NAMES)
def test_hall_cameras(vrt, po, hall, name):
    _against_ref(vrt, po, hall, csr.hall_cameras(vrt)[name], name)


def test_fixed_camera(vrt, po, hall):
    _against_ref(vrt, po, hall, None, "fixed camera")


def test_axis_aligned_odd_size(vrt, po, hall):
    _against_ref(vrt, po, hall, csr.hall_cameras(vrt, 13, 7)["axis_aligned"], "13x7 axis_aligned", 13, 7)


def test_row_window_leaves_the_other_rows(vrt, po, hall):
    cam = csr.orbit(vrt, 2)
    _against_ref(vrt, po, hall, cam, "rows 13..43", y0=13, y1=43)
    px = _frame(_render(vrt, hall[1], cam, W, H, 2, 3, 3, 1, 1, 13, 43), W, H)[0]
    assert (px[:13] == MARK).all() and (px[43:] == MARK).all() and (px[13:43] != MARK).any()


def test_sixteen_bounces(vrt, po, hall):
    _against_ref(vrt, po, hall, csr.hall_cameras(vrt)["inside_blob"], "16 bounces", configs=((1, 16, 1, 0, 1), (1, 16, 0, 0, 0)))


def test_one_bounce_and_emission_under_light_sampling(vrt, po, hall):
    """bounces = 1 (the batch's first depth is its last) for nee = 1 and nee = 0, each with and without light sampling; and nee = 0 with
    light sampling over two depths, which ec.CONFIGS leaves out"""
    _against_ref(vrt, po, hall, csr.hall_cameras(vrt)["orbit_1"], "one bounce",
                 configs=((2, 1, 1, 3, 1), (2, 1, 0, 0, 1), (2, 1, 1, 1, 0), (2, 1, 0, 5, 0), (2, 2, 1, 1, 0)))


def test_no_bounce_is_the_flat_sum_with_emission(vrt, po, hall):
    _against_ref(vrt, po, hall, csr.hall_cameras(vrt)["framing"], "bounces 0", configs=((3, 0, 1, 0, 1), (2, 0, 0, 0, 0)))


def test_batches_of_two_two_and_one_samples(vrt, po, hall):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs this test's body with 2 * W * H paths per batch, so that spp = 5
    takes batches of 2, 2 and 1 samples"""
    if not BATCH_CHILD:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, VXRT_PATH_BATCH=str(2 * W * H), VXRT_EMISSIVE_TEST_CHILD="1")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "batches_of_two"],
                           env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
        return
    assert os.environ["VXRT_PATH_BATCH"] == str(2 * W * H)
    _against_ref(vrt, po, hall, csr.hall_cameras(vrt)["orbit_1"], "batched", configs=((5, 2, 1, 0, 1), (5, 2, 0, 3, 0)))


def test_two_frames_in_flight(vrt, po, hall):
    import torch
    b, ds, tab, _ = hall
    dev = ds.t["tri"].device
    pp = po.shade_params()
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cams = [csr.orbit(vrt, 1), csr.orbit(vrt, 6)]
        cfg = ((2, 3, 1, 3, 1), (2, 2, 0, 11, 0))
        outs = [_outputs(dev, W, H) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(2):
            spp, bounces, shadow, seed, nee = cfg[i]
            _render(vrt, ds, cams[i], W, H, spp, bounces, seed, shadow, nee, stream=streams[i].cuda_stream, out=outs[i])
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
        for i in range(2):
            spp, bounces, shadow, seed, nee = cfg[i]
            _check(_frame(outs[i], W, H), er.frame(b, cams[i], W, H, pp, spp, bounces, seed, shadow, nee, ec.SCALE, tab), "in flight %d" % i)
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)


def test_a_scene_without_emissive_materials(vrt, gpu_device):
    """nee = 0 is vxrt_render_path bit for bit; no table can be set, so nee = 1 is refused and dst stays"""
    import torch
    ds = vrt.tracer.DeviceScene(scenes.mirror_hall(vrt), gpu_device)
    try:
        cam = csr.hall_cameras(vrt)["orbit_1"]
        for spp, bounces, shadow, seed in pr.CONFIGS:
            px, col, cnt = _outputs(gpu_device, W, H)
            vrt.rtapi.render_path(ds.accel, cam, W, H, 0, H, vrt.rtapi.default_shade_params(), spp, bounces, px.data_ptr(), seed, shadow, col.data_ptr(),
                                  cnt.data_ptr(), _stream())
            want = _frame((px, col, cnt), W, H)
            _check(_frame(_render(vrt, ds, cam, W, H, spp, bounces, seed, shadow, 0, scale=3.0), W, H), want, "plain hall %r" % ((spp, bounces, shadow, seed),))
        with pytest.raises(Exception):
            ds.set_emitters(np.array([[0, 0]], np.uint32))
        assert vrt.rtapi.accel_info(ds.accel, 7) == 0
        out = _outputs(gpu_device, W, H)
        with pytest.raises(Exception):
            _render(vrt, ds, cam, W, H, 2, 2, 0, 0, 1, out=out)
        torch.cuda.synchronize()
        assert (out[0].cpu().numpy() == MARK).all()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()


# ---- the table ----
@pytest.fixture(scope="module")
def strips(vrt, gpu_device):
    """the ceiling light cut into 4,096 triangles of growing width, and the lamp: 4,098 emissive triangles to take tables from"""
    b, ranges = ec.hall(vrt, light_tris=4096)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    pairs = vrt.rtapi.emitter_pairs(b, ranges)
    assert len(pairs) == 4098
    yield b, ds, pairs
    ds.close()


@pytest.mark.parametrize("n", ec.TABLE_SIZES)
def test_table_parity(vrt, strips, n):
    b, ds, pairs = strips
    sub = pairs[:n] if n <= 4096 and n % 2 == 0 else np.concatenate([pairs[:n - 1], pairs[4096:4097]])   # (an odd table ends with a lamp triangle)
    base = vrt.rtapi._lib().vxrt_accel_bytes(ds.accel) - 56 * vrt.rtapi.accel_info(ds.accel, 7)
    ds.set_emitters(sub)
    assert vrt.rtapi.accel_info(ds.accel, 7) == n
    assert vrt.rtapi._lib().vxrt_accel_bytes(ds.accel) == base + 56 * n
    tri, q, cum = vrt.rtapi.accel_read_emitters(ds.accel, _stream())
    wtri, wq, wcum, Q = er.table(b, sub)
    np.testing.assert_array_equal(tri.view(np.uint32), wtri.view(np.uint32))
    np.testing.assert_array_equal(q, wq)
    np.testing.assert_array_equal(cum, wcum)
    assert int(cum[-1]) == Q and (n < 3 or len(set(q.tolist())) > 1)
    assert vrt.rtapi.status(_stream()) == 0


# ---- the emitter ray alone ----
def _unxorshift(r):
    """the state whose xorshift is r (each of the three steps undone)"""
    r &= 0xFFFFFFFF
    x = r
    for _ in range(7):
        x = r ^ ((x << 5) & 0xFFFFFFFF)
    r = x
    for _ in range(2):
        x = r ^ (x >> 17)
    r = x
    for _ in range(3):
        x = r ^ ((x << 13) & 0xFFFFFFFF)
    return x


def test_emitter_rays_on_hostile_seeds_and_points(vrt, hall):
    import torch
    b, ds, tab, pairs = hall
    tri12, q, cum, Q = tab
    r0s = [1, 2 ** 31, 2 ** 32 - 1]
    for c in [int(v) for v in cum[:-1]]:
        for t in (c - 1, c):
            r0 = -((-t << 32) // Q)
            r0s += [r0, r0 - 1]
    seeds = [0] + [_unxorshift(r) for r in r0s if 0 < r < 2 ** 32]
    assert all(int(er.xorshift(np.array([s], np.uint32))[0]) == r for s, r in zip(seeds[1:], [r for r in r0s if 0 < r < 2 ** 32]))
    rng = np.random.default_rng(5)
    seeds += [int(v) for v in rng.integers(1, 2 ** 32, 200)]
    n0 = len(seeds)
    I = np.stack([rng.uniform(0, 350, n0), rng.uniform(5, 250, n0), rng.uniform(-250, 250, n0)], 1).astype(np.float32)
    N = rng.normal(size=(n0, 3))
    N = (N / np.linalg.norm(N, axis=1)[:, None]).astype(np.float32)
    # a point in the ceiling light's own plane (o = I + N' * 1e-3 keeps y = 255: the projected area is 0, G = 0, the ray is real)
    seeds.append(seeds[0]); I = np.vstack([I, [[0.0, 255.0, 0.0]]]).astype(np.float32); N = np.vstack([N, [[1.0, 0.0, 0.0]]]).astype(np.float32)
    # a normal that faces away from every emitter it can draw (below the floor, looking down)
    seeds.append(12345); I = np.vstack([I, [[100.0, -5.0, 0.0]]]).astype(np.float32); N = np.vstack([N, [[0.0, -1.0, 0.0]]]).astype(np.float32)
    # points AT their own sample position: d2 = 0 (a zero normal keeps o = I)
    for s in (7, 99, 2 ** 31):
        P = er.emitter_rays(tab, 1.0, [s], [[0, 0, 0]], [[0, 1, 0]])
        e = int(P[3][0])
        st = er.xorshift(er.xorshift(np.array([s], np.uint32)))
        a = er.to_float(st)[0]
        bb = er.to_float(er.xorshift(st))[0]
        if a + bb > np.float32(1.0):
            a, bb = np.float32(1.0) - a, np.float32(1.0) - bb
        T = tri12[e]
        pt = [(T[k] + a * T[3 + k]) + bb * T[6 + k] for k in range(3)]
        seeds.append(s); I = np.vstack([I, [pt]]).astype(np.float32); N = np.vstack([N, [[0.0, 0.0, 0.0]]]).astype(np.float32)
    seeds = np.array(seeds, np.uint32)
    n = len(seeds)
    want = er.emitter_rays(tab, 0.75, seeds, I, N)
    assert (~want[4][-3:]).all() and not want[4][-4] and want[4][-5] and (want[2][-5] == 0).all()   # d2 = 0 x 3, facing away, in plane
    assert want[4][:n0].any() and (~want[4][:n0]).any() and set(want[3].tolist()) == set(range(len(pairs)))
    dev = ds.t["tri"].device
    pts = torch.from_numpy(np.concatenate([I, N], 1).astype(np.float32)).to(dev)
    sd = torch.from_numpy(seeds.view(np.int32)).to(dev)
    rays = torch.zeros(n * 6, dtype=torch.float32, device=dev)
    tmax = torch.zeros(n, dtype=torch.float32, device=dev)
    G = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    e = torch.zeros(n, dtype=torch.int32, device=dev)
    vrt.rtapi.emitter_rays(ds.accel, n, pts.data_ptr(), sd.data_ptr(), 0.75, rays.data_ptr(), tmax.data_ptr(), G.data_ptr(), e.data_ptr(), _stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(e.cpu().numpy().view(np.uint32), want[3])
    np.testing.assert_array_equal(rays.cpu().numpy().reshape(n, 6).view(np.uint32), want[0].view(np.uint32))
    np.testing.assert_array_equal(tmax.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(G.cpu().numpy().reshape(n, 3).view(np.uint32), want[2].view(np.uint32))
    assert vrt.rtapi.status(_stream()) == 0


# ---- refusals ----
def _raw(vrt, accel, px, cam14, em, path=None):
    L = vrt.rtapi._lib()
    p = vrt.rtapi.default_shade_params()
    q = path or vrt.rtapi.PathParams(2, 2, 0, 1)
    cam = vrt.rtapi.Camera.from_cam14(cam14)
    return L.vxrt_render_path_emissive(accel, C.byref(cam), W, H, 0, H, C.byref(p), C.byref(q), None if em is None else C.byref(em), px.data_ptr(), None, None,
                                       _stream())


def test_refusals_leave_dst_untouched(vrt, gpu_device):
    import torch
    b, ranges = ec.hall(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    try:
        EP = vrt.rtapi.EmissiveParams
        two = C.c_uint32 * 2
        pairs = vrt.rtapi.emitter_pairs(b, ranges)
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        cam = csr.framing(W, H)
        info = lambda: vrt.rtapi.accel_info(ds.accel, 7)
        assert _raw(vrt, ds.accel, px, cam, EP(1, 1.0, two(0, 0))) == -1                      # nee = 1 without a table
        ds.set_emitters(pairs)
        assert info() == 4
        for bad in (None, EP(2, 1.0, two(0, 0)), EP(0, 1.0, two(1, 0)), EP(1, 1.0, two(0, 7)), EP(0, -1.0, two(0, 0)), EP(1, float("nan"), two(0, 0)),
                    EP(0, float("inf"), two(0, 0))):
            assert _raw(vrt, ds.accel, px, cam, bad) == -1
        assert _raw(vrt, ds.accel, px, cam, EP(1, 1.0, two(0, 0)), vrt.rtapi.PathParams(0, 2, 0, 1)) == -1   # what vxrt_render_path refuses
        assert _raw(vrt, None, px, cam, EP(0, 1.0, two(0, 0))) == -1
        # the table is kept by every refused call
        for bad in ([[0, 0]], [[ec.CEILING, 10 ** 6]], [[99, int(pairs[0, 1])]], np.zeros((vrt.rtapi.MAX_EMITTERS + 1, 2), np.uint32) + pairs[0]):
            with pytest.raises(Exception):
                ds.set_emitters(np.asarray(bad, np.uint32))
            assert info() == 4
        # what moves the scene makes the table stale; setting it again makes it valid
        ds.set_transforms([ec.lamp_transform()], first=ec.LAMP)
        assert info() == 0 and _raw(vrt, ds.accel, px, cam, EP(1, 1.0, two(0, 0))) == -1
        with pytest.raises(Exception):
            vrt.rtapi.accel_read_emitters(ds.accel, _stream())
        ds.set_emitters(pairs)
        assert info() == 4
        ds.refit(geometry=False)
        assert info() == 0 and _raw(vrt, ds.accel, px, cam, EP(1, 1.0, two(0, 0))) == -1
        ds.set_emitters(pairs)
        ds.refit(geometry=True)
        assert info() == 0 and _raw(vrt, ds.accel, px, cam, EP(1, 1.0, two(0, 0))) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
        assert _raw(vrt, ds.accel, px, cam, EP(0, 1.0, two(0, 0))) == 0                       # nee = 0 needs no table
        ds.set_emitters(pairs)
        assert _raw(vrt, ds.accel, px, cam, EP(1, 1.0, two(0, 0))) == 0
        ds.set_emitters(None)
        assert info() == 0
        torch.cuda.synchronize()
        assert (px.cpu().numpy() != MARK).all()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()


def test_alpha_table_is_refused(vrt, golden, gpu_device):
    import torch
    import shading_ref as sr
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in KEYS}, gpu_device)
    try:
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        cam = csr.golden_cameras(vrt)["g_orbit_1"]
        em = vrt.rtapi.EmissiveParams(0, 1.0, (C.c_uint32 * 2)(0, 0))
        assert _raw(vrt, ds.accel, px, cam, em) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
        ds.set_alpha_test(None)
        assert _raw(vrt, ds.accel, px, cam, em) == 0
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()
