"""GPU: multiple importance sampling of area lights (vxrt_render_path_emissive_mis, vxrt_emitter_rays_mis, vxrt_emitter_hit_weights,
the emitter index) against the restatement tests/emissive_mis_ref.py, bit for bit: of the frames pixels, f32 colours as u32 and rays
traced; of the two steps every output.  No masks, no tolerances; guard words behind every output.  tests/test_emissive_mis_cpu.py pins
the restatement and shows that the cases below are not vacuous."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_ref as cr
import camera_secondary_ref as csr
import emissive_cases as ec
import emissive_mis_cases as mc
import emissive_mis_ref as mr
import emissive_ref as er
import path_ref as pr
from camera_ref import po as _po

pytestmark = pytest.mark.gpu
W, H = pr.W, pr.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
FMARK = -12345.5
GUARD = 64
BATCH_CHILD = os.environ.get("VXRT_EMISSIVE_MIS_TEST_CHILD") == "1"


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _outputs(dev, w, h):
    """pixels, colours and the ray count, each with GUARD marked words behind it"""
    import torch
    cnt = torch.full((1 + GUARD,), MARK, dtype=torch.int64, device=dev)
    cnt[0] = 0
    return (torch.full((h * w + GUARD,), MARK, dtype=torch.int32, device=dev), torch.full((h * w * 3 + GUARD,), FMARK, dtype=torch.float32, device=dev), cnt)


def _em(vrt, scale=mc.SCALE, reserved=(0, 0, 0)):
    return vrt.rtapi.EmissiveMisParams(float(scale), (C.c_uint32 * 3)(*reserved))


def _render(vrt, ds, cam, w, h, spp, bounces, seed, shadow, y0=0, y1=None, stream=None, out=None, scale=mc.SCALE):
    px, col, cnt = out = out or _outputs(ds.t["tri"].device, w, h)
    vrt.rtapi.render_path_emissive_mis(ds.accel, cam, w, h, y0, h if y1 is None else y1, vrt.rtapi.default_shade_params(), spp, bounces, _em(vrt, scale),
                                       px.data_ptr(), seed, shadow, col.data_ptr(), cnt.data_ptr(), _stream() if stream is None else stream)
    return out


def _frame(out, w, h, y0=0, y1=None):
    """(pixels, colours, rays traced) of rows [y0, y1); the guard words must be untouched"""
    import torch
    y1 = h if y1 is None else y1
    torch.cuda.synchronize()
    px, col, cnt = (t.cpu().numpy() for t in out)
    assert (px[h * w:] == MARK).all() and (col[h * w * 3:] == np.float32(FMARK)).all() and (cnt[1:] == MARK).all(), "a guard word was written"
    return px[:h * w].view(np.uint32).reshape(h, w)[y0:y1], col[:h * w * 3].reshape(h, w, 3)[y0:y1], int(cnt[0])


def _check(got, want, what):
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": pixels")
    assert got[2] == want[2], "%s: rays traced %d, restatement %d" % (what, got[2], want[2])


_SCENES = {}


@pytest.fixture(scope="module")
def halls(vrt, gpu_device):
    """which -> (scene buffers, DeviceScene with the table set, table, index, pairs); built on first use, closed with the module"""
    def get(which):
        if which not in _SCENES:
            b, pairs = mc.hall(vrt, which)
            ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
            ds.set_emitters(pairs)
            assert vrt.rtapi.accel_info(ds.accel, 7) == len(pairs)
            _SCENES[which] = (b, ds, er.table(b, pairs), mr.index(pairs), pairs)
        return _SCENES[which]
    yield get
    for v in _SCENES.values():
        v[1].close()
    _SCENES.clear()


def _against_ref(vrt, po, hall, cam, what, w=W, h=H, y0=0, y1=None, configs=mc.CONFIGS):
    b, ds, tab, idx, _ = hall
    y1 = h if y1 is None else y1
    prim = pr.primary(b, po.camera_rays(w, h, y0, y1) if cam is None else cr.rays(cam, w, h, y0, y1))
    for spp, bounces, shadow, seed in configs:
        got = _frame(_render(vrt, ds, cam, w, h, spp, bounces, seed, shadow, y0, y1), w, h, y0, y1)
        assert vrt.rtapi.status(_stream()) == 0
        _check(got, mr.frame(b, cam, w, h, po.shade_params(), spp, bounces, seed, shadow, mc.SCALE, tab, idx, y0, y1, prim),
               "%s spp=%d bounces=%d shadow=%d seed=%d" % (what, spp, bounces, shadow, seed))


@pytest.mark.parametrize("which", mc.TABLE_NAMES)
@pytest.mark.parametrize("name", mc.CAMERA_NAMES)
def test_configurations(vrt, po, halls, name, which):
    _against_ref(vrt, po, halls(which), mc.cameras(vrt, W, H)[name], "%s %s" % (which, name))


def test_odd_size(vrt, po, halls):
    _against_ref(vrt, po, halls("full"), mc.gap_camera(vrt, 13, 7), "13x7 gap", 13, 7)


def test_row_window_leaves_the_other_rows(vrt, po, halls):
    cam = csr.orbit(vrt, 2)
    _against_ref(vrt, po, halls("full"), cam, "rows 13..43", y0=13, y1=43)
    px = _frame(_render(vrt, halls("full")[1], cam, W, H, 2, 3, 3, 1, 13, 43), W, H)[0]
    assert (px[:13] == MARK).all() and (px[43:] == MARK).all() and (px[13:43] != MARK).any()


def test_sixteen_bounces(vrt, po, halls):
    _against_ref(vrt, po, halls("twice"), csr.hall_cameras(vrt)["inside_blob"], "16 bounces", configs=((1, 16, 1, 0),))


def test_batches_of_two_two_and_one_samples(vrt, po, halls):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs this test's body with 2 * W * H paths per batch, so that spp = 5
    takes batches of 2, 2 and 1 samples"""
    if not BATCH_CHILD:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, VXRT_PATH_BATCH=str(2 * W * H), VXRT_EMISSIVE_MIS_TEST_CHILD="1")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "batches_of_two"],
                           env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
        return
    assert os.environ["VXRT_PATH_BATCH"] == str(2 * W * H)
    _against_ref(vrt, po, halls("full"), mc.gap_camera(vrt, W, H), "batched", configs=((5, 2, 1, 0),))


def test_two_frames_in_flight(vrt, po, halls):
    import torch
    b, ds, tab, idx, _ = halls("full")
    dev = ds.t["tri"].device
    pp = po.shade_params()
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cams = [csr.orbit(vrt, 1), mc.gap_camera(vrt, W, H)]
        cfg = ((2, 3, 1, 3), (2, 2, 0, 11))
        outs = [_outputs(dev, W, H) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(2):
            spp, bounces, shadow, seed = cfg[i]
            _render(vrt, ds, cams[i], W, H, spp, bounces, seed, shadow, stream=streams[i].cuda_stream, out=outs[i])
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
        for i in range(2):
            spp, bounces, shadow, seed = cfg[i]
            _check(_frame(outs[i], W, H), mr.frame(b, cams[i], W, H, pp, spp, bounces, seed, shadow, mc.SCALE, tab, idx), "in flight %d" % i)
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)


def test_no_bounce_is_the_frame_of_emitter_sampling(vrt, halls):
    """bounces = 0: vxrt_render_path_emissive with nee = 1 and bounces = 0, bit for bit, against the GPU's own frame"""
    b, ds, _, _, _ = halls("full")
    dev = ds.t["tri"].device
    for name in ("framing", "gap"):
        cam = mc.cameras(vrt, W, H)[name]
        for spp, shadow in ((3, 1), (2, 0)):
            out = _outputs(dev, W, H)
            vrt.rtapi.render_path_emissive(ds.accel, cam, W, H, 0, H, vrt.rtapi.default_shade_params(), spp, 0,
                                           vrt.rtapi.EmissiveParams(1, float(mc.SCALE), (C.c_uint32 * 2)(0, 0)), out[0].data_ptr(), 0, shadow, out[1].data_ptr(),
                                           out[2].data_ptr(), _stream())
            want = _frame(out, W, H)
            _check(_frame(_render(vrt, ds, cam, W, H, spp, 0, 0, shadow), W, H), want, "bounces 0 %s spp=%d shadow=%d" % (name, spp, shadow))
    assert vrt.rtapi.status(_stream()) == 0


# ---- the emitter ray alone ----
def _rays_mis(vrt, ds, seeds, I, N, scale):
    """(rays, tmax, Gm, e, wE) of vxrt_emitter_rays_mis, guard words checked"""
    import torch
    dev = ds.t["tri"].device
    n = len(seeds)
    pts = torch.from_numpy(np.concatenate([I, N], 1).astype(np.float32)).to(dev)
    sd = torch.from_numpy(np.asarray(seeds, np.uint32).view(np.int32)).to(dev)
    rays = torch.full((n * 6 + GUARD,), FMARK, dtype=torch.float32, device=dev)
    tmax = torch.full((n + GUARD,), FMARK, dtype=torch.float32, device=dev)
    G = torch.full((n * 3 + GUARD,), FMARK, dtype=torch.float32, device=dev)
    e = torch.full((n + GUARD,), MARK, dtype=torch.int32, device=dev)
    wE = torch.full((n + GUARD,), FMARK, dtype=torch.float32, device=dev)
    vrt.rtapi.emitter_rays_mis(ds.accel, n, pts.data_ptr(), sd.data_ptr(), scale, rays.data_ptr(), tmax.data_ptr(), G.data_ptr(), e.data_ptr(), wE.data_ptr(), _stream())
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (rays, tmax, G, e, wE)]
    for a, k in zip(out, (6, 1, 3, 1, 1)):
        assert (a[n * k:] == (MARK if a.dtype == np.int32 else np.float32(FMARK))).all(), "a guard word was written"
    return out[0][:n * 6].reshape(n, 6), out[1][:n], out[2][:n * 3].reshape(n, 3), out[3][:n].view(np.uint32), out[4][:n]


def _check_rays(got, want):
    np.testing.assert_array_equal(got[3], want[3], err_msg="e")
    np.testing.assert_array_equal(got[0].view(np.uint32), want[0].view(np.uint32), err_msg="rays")
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg="tmax")
    np.testing.assert_array_equal(got[2].view(np.uint32), want[2].view(np.uint32), err_msg="Gm")
    np.testing.assert_array_equal(got[4].view(np.uint32), want[5].view(np.uint32), err_msg="wE")


def test_emitter_rays_mis_on_hostile_seeds_and_points(vrt, halls):
    b, ds, tab, _, pairs = halls("full")
    tri12, q, cum, Q = tab
    r0s = [1, 2 ** 31, 2 ** 32 - 1]
    for c in [int(v) for v in cum[:-1]]:                              # the selection extremes and both sides of every boundary
        for t in (c - 1, c):
            r0 = -((-t << 32) // Q)
            r0s += [r0, r0 - 1]
    seeds = [0] + [mc.unxorshift(r) for r in r0s if 0 < r < 2 ** 32]
    rng = np.random.default_rng(5)
    seeds += [int(v) for v in rng.integers(1, 2 ** 32, 200)]
    n0 = len(seeds)
    I = np.stack([rng.uniform(0, 350, n0), rng.uniform(5, 250, n0), rng.uniform(-250, 250, n0)], 1).astype(np.float32)
    N = rng.normal(size=(n0, 3))
    N = (N / np.linalg.norm(N, axis=1)[:, None]).astype(np.float32)
    # a point in the plane of the emitter its seed draws (o = I + N' * 1e-3 stays in it: an = 0, so wE = 1, Gm = 0, and the ray is real)
    s_plane = next(s for s in range(1, 1000) if pairs[int(er.select(cum, Q, er.xorshift(np.array([s], np.uint32)))[0]), 0] == ec.CEILING)
    seeds.append(s_plane); I = np.vstack([I, [[0.0, 255.0, 0.0]]]).astype(np.float32); N = np.vstack([N, [[1.0, 0.0, 0.0]]]).astype(np.float32)
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
    want = mr.emitter_rays(tab, 0.75, seeds, I, N)
    assert (~want[4][-3:]).all() and (want[5][-3:] == 0).all()                                   # d2 = 0 x 3: skipped, wE = 0
    assert not want[4][-4]                                                                       # facing away
    assert want[4][-5] and (want[2][-5] == 0).all() and want[5][-5] == 1.0                       # in plane: real, Gm = 0, wE = 1
    assert want[4][:n0].any() and (~want[4][:n0]).any() and set(want[3].tolist()) == set(range(len(pairs)))
    assert ((want[5] > 0) & (want[5] < 1)).any()
    _check_rays(_rays_mis(vrt, ds, seeds, I, N, 0.75), want)
    assert vrt.rtapi.status(_stream()) == 0


def test_emitter_rays_mis_in_the_near_field(vrt, halls):
    """the points of the bound test (tests/test_emissive_mis_cpu.py): Gm stays below the emitter's radiance where G does not"""
    b, ds, tab, _, _ = halls("full")
    seeds, I, N = mc.near_field(tab)
    want = mr.emitter_rays(tab, mc.SCALE, seeds, I, N)
    got = _rays_mis(vrt, ds, seeds, I, N, mc.SCALE)
    _check_rays(got, want)
    Le = tab[0][got[3], 9:12]
    assert (got[2] <= Le * np.float32(mc.SCALE) * np.float32(1 + 2.0 ** -20)).all() and want[4].any()
    assert vrt.rtapi.status(_stream()) == 0


# ---- the lookup and the bounce ray's weight alone ----
def _hit_weights(vrt, ds, rays, hits, normals):
    import torch
    dev = ds.t["tri"].device
    n = len(hits)
    r = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(dev)
    hh = torch.from_numpy(np.ascontiguousarray(hits).view(np.int32).reshape(n, 6).copy()).to(dev)
    nn = torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(dev)
    e = torch.full((n + GUARD,), MARK, dtype=torch.int32, device=dev)
    w = torch.full((n + GUARD,), FMARK, dtype=torch.float32, device=dev)
    vrt.rtapi.emitter_hit_weights(ds.accel, n, r.data_ptr(), hh.data_ptr(), nn.data_ptr(), e.data_ptr(), w.data_ptr(), _stream())
    torch.cuda.synchronize()
    e, w = e.cpu().numpy(), w.cpu().numpy()
    assert (e[n:] == MARK).all() and (w[n:] == np.float32(FMARK)).all(), "a guard word was written"
    return e[:n].view(np.uint32), w[:n]


@pytest.fixture(scope="module")
def strips(vrt, gpu_device):
    """emissive_cases' 4,098-pair strip hall: the ceiling light cut into 4,096 triangles, and the lamp"""
    b, ranges = ec.hall(vrt, light_tris=4096)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    pairs = vrt.rtapi.emitter_pairs(b, ranges)
    assert len(pairs) == 4098
    yield b, ds, pairs
    ds.close()


@pytest.mark.parametrize("n", [1, 2, 64, 65, 4097])
def test_hit_weights_on_synthetic_records(vrt, strips, n):
    b, ds, pairs = strips
    sub = mc.shuffled(pairs, seed=n)[:n]
    ds.set_emitters(sub)
    tab, idx = er.table(b, sub), mr.index(sub)
    keys = mc.lookup_keys(sub)
    m = len(keys)
    rng = np.random.default_rng(n)
    hits = np.zeros(m, _po.HIT_DTYPE)
    hits["blasIdx"], hits["triIdx"] = keys[:, 0], keys[:, 1]
    hits["dist"] = rng.uniform(0.0, 400.0, m).astype(np.float32)
    hits["dist"][::7] = 0.0                                           # t = 0: pe = 0
    hits["dist"][3::11] = cr.LARGE                                    # (every record is looked up, whatever its dist)
    d = rng.normal(size=(m, 3))
    rays = np.concatenate([rng.uniform(-100, 400, (m, 3)), d / np.linalg.norm(d, axis=1)[:, None]], 1).astype(np.float32)
    nr = rng.normal(size=(m, 3))
    nr = (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(np.float32)
    nr[::14] = -rays[::14, 3:6]                                       # t = 0 and cosx = 0: den = 0, the weight's other arm
    we, ww = mr.hit_weights(tab, idx, rays, hits, nr)
    assert (we[:n] != mr.NOT_LISTED).all() and (we == mr.NOT_LISTED).any() and ((ww > 0) & (ww < 1)).any()
    ge, gw = _hit_weights(vrt, ds, rays, hits, nr)
    assert vrt.rtapi.accel_info(ds.accel, 8) == n
    np.testing.assert_array_equal(ge, we)
    np.testing.assert_array_equal(gw.view(np.uint32), ww.view(np.uint32))
    assert vrt.rtapi.status(_stream()) == 0


def test_hit_weights_on_the_bounce_rays_of_a_frame(vrt, po, halls):
    """the bounce rays of a frame of the restatement, traced by vxrt_trace: the device's records, its lookup and its weights"""
    import torch
    for which in ("partial", "twice"):
        b, ds, tab, idx, _ = halls(which)
        keep = []
        mr.frame(b, mc.gap_camera(vrt, W, H), W, H, po.shade_params(), 1, 2, 5, 0, mc.SCALE, tab, idx, keep=keep)
        rays = np.concatenate([k["rays"] for k in keep])
        normals = np.concatenate([k["normals"] for k in keep])
        want_hits = np.concatenate([k["hits"] for k in keep])
        dev = ds.t["tri"].device
        r = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(dev)
        out = torch.full((len(rays), 6), 0x7B, dtype=torch.int32, device=dev)
        vrt.rtapi.trace(ds.accel, r.data_ptr(), len(rays), out.data_ptr(), vrt.rtapi.MODE_CLOSEST, None, _stream())
        torch.cuda.synchronize()
        hits = out.cpu().numpy().view(_po.HIT_DTYPE).reshape(-1)
        np.testing.assert_array_equal(hits.view(np.uint32), want_hits.view(np.uint32))
        we, ww = mr.hit_weights(tab, idx, rays, hits, normals)
        assert (we != mr.NOT_LISTED).any() and (we == mr.NOT_LISTED).any()
        ge, gw = _hit_weights(vrt, ds, rays, hits, normals)
        np.testing.assert_array_equal(ge, we)
        np.testing.assert_array_equal(gw.view(np.uint32), ww.view(np.uint32))
    assert vrt.rtapi.status(_stream()) == 0


# ---- the index's lifetime ----
def test_index_lifetime(vrt, gpu_device):
    import torch
    b, pairs = mc.hall(vrt, "full")
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    try:
        n = len(pairs)
        info = lambda which: vrt.rtapi.accel_info(ds.accel, which)
        size = lambda: vrt.rtapi._lib().vxrt_accel_bytes(ds.accel)
        base = size()
        assert info(8) == 0
        ds.set_emitters(pairs)
        assert info(7) == n and info(8) == 0 and size() == base + 56 * n
        cam = csr.framing(W, H)
        # the frames that existed need no index and build none
        out = _outputs(gpu_device, W, H)
        vrt.rtapi.render_path_emissive(ds.accel, cam, W, H, 0, H, vrt.rtapi.default_shade_params(), 1, 1,
                                       vrt.rtapi.EmissiveParams(1, 1.0, (C.c_uint32 * 2)(0, 0)), out[0].data_ptr(), 0, 0, None, None, _stream())
        assert info(8) == 0 and size() == base + 56 * n
        first = _frame(_render(vrt, ds, cam, W, H, 1, 1, 7, 0), W, H)
        assert info(8) == n and size() == base + 56 * n + 12 * n
        _check(_frame(_render(vrt, ds, cam, W, H, 1, 1, 7, 0), W, H), first, "the frame that built the index and the next one")
        ds.set_emitters(pairs[:3])
        assert info(7) == 3 and info(8) == 0 and size() == base + 56 * 3
        _render(vrt, ds, cam, W, H, 1, 1, 7, 0)
        assert info(8) == 3 and size() == base + 68 * 3
        # a refit makes the table stale: the frame is refused until the table is set again
        ds.refit(geometry=False)
        assert info(7) == 0
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        assert _raw(vrt, ds.accel, px, cam, _em(vrt)) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
        ds.set_emitters(pairs)
        assert info(8) == 0 and _raw(vrt, ds.accel, px, cam, _em(vrt)) == 0 and info(8) == n
        ds.set_emitters(None)
        assert info(7) == 0 and info(8) == 0 and size() == base
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()


# ---- refusals ----
def _raw(vrt, accel, px, cam14, em, path=None):
    L = vrt.rtapi._lib()
    p = vrt.rtapi.default_shade_params()
    q = path or vrt.rtapi.PathParams(2, 2, 0, 1)
    cam = vrt.rtapi.Camera.from_cam14(cam14)
    return L.vxrt_render_path_emissive_mis(accel, C.byref(cam), W, H, 0, H, C.byref(p), C.byref(q), None if em is None else C.byref(em), px.data_ptr(), None, None,
                                           _stream())


def test_refusals_leave_dst_untouched(vrt, gpu_device):
    import torch
    b, pairs = mc.hall(vrt, "full")
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    try:
        L = vrt.rtapi._lib()
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        cam = csr.framing(W, H)
        buf = torch.zeros(64, dtype=torch.float32, device=gpu_device)
        p = buf.data_ptr()
        rays_mis = lambda a, n=1, scale=1.0, mis=p: L.vxrt_emitter_rays_mis(a, n, p, p, scale, p, p, p, p, mis, _stream())
        weights = lambda a, n=1, mis=p: L.vxrt_emitter_hit_weights(a, n, p, p, p, p, mis, _stream())
        assert _raw(vrt, ds.accel, px, cam, _em(vrt)) == -1                                   # no table
        assert rays_mis(ds.accel) == -1 and weights(ds.accel) == -1
        ds.set_emitters(pairs)
        for bad in (None, _em(vrt, reserved=(1, 0, 0)), _em(vrt, reserved=(0, 7, 0)), _em(vrt, reserved=(0, 0, 1)), _em(vrt, -1.0), _em(vrt, float("nan")),
                    _em(vrt, float("inf"))):
            assert _raw(vrt, ds.accel, px, cam, bad) == -1
        assert _raw(vrt, ds.accel, px, cam, _em(vrt), vrt.rtapi.PathParams(0, 2, 0, 1)) == -1      # what vxrt_render_path refuses
        assert _raw(vrt, ds.accel, px, cam, _em(vrt), vrt.rtapi.PathParams(2, 17, 0, 1)) == -1
        assert _raw(vrt, None, px, cam, _em(vrt)) == -1
        # the two steps: as vxrt_emitter_rays refuses
        assert rays_mis(None) == -1 and rays_mis(ds.accel, mis=None) == -1 and rays_mis(ds.accel, scale=-1.0) == -1
        assert rays_mis(ds.accel, scale=float("nan")) == -1 and rays_mis(ds.accel, n=2 ** 31) == -1
        assert weights(None) == -1 and weights(ds.accel, mis=None) == -1 and weights(ds.accel, n=2 ** 31) == -1
        assert rays_mis(ds.accel, n=0) == 0 and weights(ds.accel, n=0) == 0
        # a stale table
        ds.set_transforms([ec.lamp_transform()], first=ec.LAMP)
        assert _raw(vrt, ds.accel, px, cam, _em(vrt)) == -1 and rays_mis(ds.accel) == -1 and weights(ds.accel) == -1
        ds.set_emitters(pairs)
        ds.refit(geometry=True)
        assert _raw(vrt, ds.accel, px, cam, _em(vrt)) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
        ds.set_emitters(pairs)
        assert _raw(vrt, ds.accel, px, cam, _em(vrt)) == 0
        torch.cuda.synchronize()
        assert (px.cpu().numpy() != MARK).all()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()


def test_alpha_table_is_refused(vrt, golden, gpu_device):
    """golden tex_mix with every material made emissive, so that it has both a texture to put a threshold on and a table: refused while
    the alpha table is set, rendered before and after"""
    import torch
    import shading_ref as sr
    g = golden("tex_mix")
    b = {k: np.array(g[k]).copy() for k in KEYS}
    m = np.frombuffer(np.ascontiguousarray(b["mat"], np.uint8).tobytes(), np.float32).reshape(-1, 22).copy()
    m[:, 9:12] = 1.0
    b["mat"] = m.view(np.uint8).reshape(-1)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        ds.set_emitters(np.array([[0, 0], [0, 1]], np.uint32))
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        cam = csr.golden_cameras(vrt)["g_orbit_1"]
        assert _raw(vrt, ds.accel, px, cam, _em(vrt)) == 0
        torch.cuda.synchronize()
        px.fill_(MARK)
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        assert (mat["tex_id"] >= 0).any()
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1 and vrt.rtapi.accel_info(ds.accel, 7) == 2
        assert _raw(vrt, ds.accel, px, cam, _em(vrt)) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
        ds.set_alpha_test(None)
        assert _raw(vrt, ds.accel, px, cam, _em(vrt)) == 0
        torch.cuda.synchronize()
        assert vrt.rtapi.status(_stream()) == 0
    finally:
        ds.close()
