"""GPU: adaptive sampling -- path frames with a sample count per pixel (vxrt_render_path_adaptive), the variance frame on top of them
(vxrt_render_path_variance_adaptive) and the counts from a variance (vxrt_sample_counts) -- bit for bit: against the GPU's own
vxrt_render_path / vxrt_render_path_variance through the two identities of the definition (uniform, mosaic), and against the restatement
tests/adaptive_ref.py.  No masks, no tolerances (the variance frames: a NaN of the restatement asks for a NaN, as tests/test_gpu_variance.py).
tests/test_adaptive_cpu.py pins the restatement and shows that the cases (tests/adaptive_cases.py) are not vacuous."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import denoise_cases as dc
import motion_cases as mc
import motion_ref as mr
import path_ref as pr
import scenes
import temporal_cases as tc
import variance_cases as vc
import variance_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = ac.W, ac.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
FMARK = -12345.5
CMARK = 0xA5A5A5A5   # marker of a counts output
CHILD = os.environ.get("VXRT_ADAPTIVE_TEST_CHILD") == "1"
f32 = np.float32


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _u32(dev, a):
    """a device copy of uint32 values (torch has no uint32 arithmetic: the bits travel as int32)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(dev)


def _outputs(dev, w, h):
    import torch
    return (torch.full((h, w), MARK, dtype=torch.int32, device=dev), torch.zeros(h * w * 3, dtype=torch.float32, device=dev),
            torch.zeros(1, dtype=torch.int64, device=dev))


def _adaptive(vrt, ds, cam, w, h, counts, cap, bounces, seed=0, shadow=0, y0=0, y1=None, stream=None, out=None):
    """counts: a numpy (h, w) array of raw counts, or a device tensor"""
    dev = ds.t["tri"].device
    px, col, cnt = out = out or _outputs(dev, w, h)
    ct = _u32(dev, counts) if isinstance(counts, np.ndarray) else counts
    vrt.rtapi.render_path_adaptive(ds.accel, cam, w, h, y0, h if y1 is None else y1, vrt.rtapi.default_shade_params(), cap, bounces, ct.data_ptr(), px.data_ptr(),
                                   seed, shadow, col.data_ptr(), cnt.data_ptr(), _stream() if stream is None else stream)
    return out + (ct,)


def _path(vrt, ds, cam, w, h, spp, bounces, seed=0, shadow=0, y0=0, y1=None):
    px, col, cnt = out = _outputs(ds.t["tri"].device, w, h)
    vrt.rtapi.render_path(ds.accel, cam, w, h, y0, h if y1 is None else y1, vrt.rtapi.default_shade_params(), spp, bounces, px.data_ptr(), seed, shadow,
                          col.data_ptr(), cnt.data_ptr(), _stream())
    return out


def _frame(out, w, h, y0=0, y1=None):
    import torch
    y1 = h if y1 is None else y1
    torch.cuda.synchronize()
    px, col, cnt = out[:3]
    return px.cpu().numpy().view(np.uint32)[y0:y1], col.cpu().numpy().reshape(h, w, 3)[y0:y1], int(cnt.item())


def _check(got, want, what):
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": pixels")
    assert got[2] == want[2], "%s: rays traced %d, expected %d" % (what, got[2], want[2])


@pytest.fixture(autouse=True)
def _status_is_clean(vrt):
    yield
    assert vrt.rtapi.status(_stream()) == 0


@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    yield b, ds
    ds.close()


def _case_frame(vrt, ds, cam, case, w=W, h=H, y0=0, y1=None, counts=None):
    counts = ac.counts_of(case, w, h) if counts is None else counts
    return _frame(_adaptive(vrt, ds, cam, w, h, counts, case["cap"], case["bounces"], case["seed"], case["shadow"], y0, y1), w, h, y0, y1)


def _mosaic(vrt, ds, cam, case, w, h, what):
    """the frame with the case's counts against the GPU's own uniform frames: every pixel is the uniform frame's of its count; returns the frame"""
    raw = ac.counts_of(case, w, h)
    got = _case_frame(vrt, ds, cam, case, w, h, counts=raw)
    n_p = ar.clamp(raw, case["cap"])
    want_px, want_col = np.zeros_like(got[0]), np.zeros_like(got[1])
    for v in np.unique(n_p):
        u = _frame(_path(vrt, ds, cam, w, h, int(v), case["bounces"], case["seed"], case["shadow"]), w, h)
        want_px[n_p == v], want_col[n_p == v] = u[0][n_p == v], u[1][n_p == v]
    np.testing.assert_array_equal(got[1].view(np.uint32), want_col.view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got[0], want_px, err_msg=what + ": pixels")
    return got


# ---- 1, 2: the uniform identity and the clamp ----
@pytest.mark.parametrize("name", ["orbit_1", None])
def test_uniform_counts_are_the_path_frame(vrt, hall, name):
    """counts[p] == spp everywhere against the GPU's own vxrt_render_path: pixels, colours, rays traced"""
    b, ds = hall
    cam = None if name is None else csr.hall_cameras(vrt)[name]
    for spp in (1, 3, 4):
        counts = _u32(ds.t["tri"].device, np.full((H, W), spp, np.uint32))
        for bounces in (0, 2):
            for shadow in (0, 1):
                want = _frame(_path(vrt, ds, cam, W, H, spp, bounces, 3, shadow), W, H)
                got = _frame(_adaptive(vrt, ds, cam, W, H, counts, spp, bounces, 3, shadow), W, H)
                _check(got, want, "%s spp %d bounces %d shadow %d" % (name, spp, bounces, shadow))
                assert bounces == 0 or got[2] > W * H


def test_counts_are_clamped_and_ignored_on_misses(vrt, hall):
    b, ds = hall
    cam = csr.hall_cameras(vrt)["orbit_1"]
    cap, bounces, seed, shadow = 3, 2, 3, 1
    full = lambda v: np.full((H, W), v, np.uint32)
    one = _frame(_adaptive(vrt, ds, cam, W, H, full(1), cap, bounces, seed, shadow), W, H)
    top = _frame(_adaptive(vrt, ds, cam, W, H, full(cap), cap, bounces, seed, shadow), W, H)
    _check(one, _frame(_path(vrt, ds, cam, W, H, 1, bounces, seed, shadow), W, H), "counts of 1")
    _check(top, _frame(_path(vrt, ds, cam, W, H, cap, bounces, seed, shadow), W, H), "counts of cap")
    assert one[2] != top[2]
    _check(_frame(_adaptive(vrt, ds, cam, W, H, full(0), cap, bounces, seed, shadow), W, H), one, "raw 0")
    for raw in (cap + 1, ac.U32_MAX, 0x80000000):
        _check(_frame(_adaptive(vrt, ds, cam, W, H, full(raw), cap, bounces, seed, shadow), W, H), top, "raw %d" % raw)
    # counts on the pixels whose primary ray misses change nothing
    miss = (pr.primary(b, cr.rays(cam, W, H))["hits"]["dist"] == cr.LARGE).reshape(H, W)
    assert 100 < miss.sum() < W * H - 100
    case = ac.RESTATED
    raw = ac.counts_of(case)
    base = _case_frame(vrt, ds, cam, case, counts=raw)
    for k, v in enumerate((0, ac.U32_MAX, 4096, 7)):
        other = raw.copy()
        other[miss] = v if k else ac.hashed(W, H, (0, 1, 5, ac.U32_MAX, 4097), 9)[miss]
        _check(_case_frame(vrt, ds, cam, case, counts=other), base, "miss pixels with other counts (%d)" % k)


# ---- 3, 4: the mosaic identity and the restatement (the child process of test_small_batches runs these as well) ----
def test_path_frame_mosaic_against_the_uniform_frames(vrt, po, hall):
    b, ds = hall
    case, cam = ac.MOSAIC, csr.hall_cameras(vrt)["orbit_1"]
    got = _mosaic(vrt, ds, cam, case, W, H, "mosaic")
    want = ar.frame(b, cam, W, H, po.shade_params(), ac.counts_of(case), case["cap"], case["bounces"], case["seed"], case["shadow"])
    _check(got, want, "mosaic against the restatement")


def _against_ref(vrt, po, b, ds, cam, what, w=W, h=H, y0=0, y1=None, case=ac.RESTATED):
    y1 = h if y1 is None else y1
    raw = ac.counts_of(case, w, h)
    got = _case_frame(vrt, ds, cam, case, w, h, y0, y1, raw)
    _check(got, ar.frame(b, cam, w, h, po.shade_params(), raw, case["cap"], case["bounces"], case["seed"], case["shadow"], y0, y1), what)
    return got


@pytest.mark.parametrize("name", ["orbit_1", None])
def test_path_frame_restated_hall(vrt, po, hall, name):
    b, ds = hall
    _against_ref(vrt, po, b, ds, None if name is None else csr.hall_cameras(vrt)[name], "hall %s" % name)


def test_path_frame_restated_textured(vrt, po, golden, gpu_device):
    g = golden("tex_mix")
    b = {k: g[k] for k in KEYS}
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        _against_ref(vrt, po, b, ds, csr.golden_cameras(vrt)["g_orbit_1"], "tex_mix g_orbit_1")
    finally:
        ds.close()


def test_path_frame_restated_odd_size_and_row_window(vrt, po, hall):
    """13 x 7 axis aligned (the centre column and row go through the EXACT launch); rows 13..43, whose other rows keep their marker"""
    b, ds = hall
    _against_ref(vrt, po, b, ds, csr.hall_cameras(vrt, 13, 7)["axis_aligned"], "13x7 axis_aligned", 13, 7)
    cam = csr.orbit(vrt, 2)
    _against_ref(vrt, po, b, ds, cam, "rows 13..43", y0=13, y1=43)
    case = ac.RESTATED
    px = _frame(_adaptive(vrt, ds, cam, W, H, ac.counts_of(case), case["cap"], case["bounces"], case["seed"], case["shadow"], 13, 43), W, H)[0]
    assert (px[:13] == MARK).all() and (px[43:] == MARK).all() and (px[13:43] != MARK).any()


def test_one_bounce_against_the_restatement(vrt, po, hall):
    """bounces = 1: the batch's first depth is its last; with and without light sampling (ac.SCAN has one bounce, against the GPU only)"""
    b, ds = hall
    for shadow in (1, 0):
        _against_ref(vrt, po, b, ds, csr.hall_cameras(vrt)["orbit_1"], "one bounce, shadow %d" % shadow, case=dict(ac.SCAN, shadow=shadow))


# ---- 5: small batches ----
def test_small_batches(vrt):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs the mosaic and restatement tests above with CHILD_BATCH paths per batch
    -- many batches, pixels whose samples straddle two of them, a short last batch and empty trailing ones (tests/test_adaptive_cpu.py
    computes that from the offsets).  The knob line the library prints under VXRT_DEBUG shows that the child took it."""
    assert not CHILD
    env = dict(os.environ, VXRT_PATH_BATCH=str(ac.CHILD_BATCH), VXRT_ADAPTIVE_TEST_CHILD="1", VXRT_DEBUG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "path_frame_mosaic or path_frame_restated"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "5 passed" in r.stdout and ("path_batch=%d " % ac.CHILD_BATCH) in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 6: the levels of the scan ----
def test_scan_of_more_than_one_pass(vrt, hall):
    """a window with more pixels than one pass of the single-workgroup scan covers (ADAPTIVE_SCAN_PASS = PT_SCAN_PASS * PT_SCAN_BLOCK):
    the running carry.  GPU against GPU by the mosaic identity; no restatement at this size."""
    b, ds = hall
    w, h = 1100, 1000
    assert vrt.rtapi.ADAPTIVE_SCAN_PASS < w * h < 2 * vrt.rtapi.ADAPTIVE_SCAN_PASS
    got = _mosaic(vrt, ds, csr.orbit(vrt, 1, 8, w, h), ac.SCAN, w, h, "1100x1000")
    assert got[2] > w * h


@pytest.mark.parametrize("w,h", [(32, 32), (33, 31), (41, 25), (1, 1)])
def test_scan_block_edges(vrt, hall, w, h):
    """exactly one scan block (1,024 pixels), one pixel fewer, one more, and a single pixel"""
    b, ds = hall
    blk = vrt.rtapi.ADAPTIVE_SCAN_BLOCK
    assert w * h in (blk, blk - 1, blk + 1, 1)
    cam = csr.orbit(vrt, 1, 8, w, h)
    got = _mosaic(vrt, ds, cam, ac.SCAN, w, h, "%dx%d" % (w, h))
    assert got[2] > w * h     # (the pixel of the 1 x 1 frame is a hit too)


# ---- 7: degenerate windows ----
def test_degenerate_windows(vrt, hall):
    b, ds = hall
    dev = ds.t["tri"].device
    case = ac.RESTATED
    # every primary ray misses: the background, nothing traced but the primary rays
    w, h = 40, 24
    away = csr.hall_cameras(vrt, w, h)["far_cancel"]
    got = _case_frame(vrt, ds, away, case, w, h)
    _check(got, _frame(_path(vrt, ds, away, w, h, 2, case["bounces"], case["seed"], case["shadow"]), w, h), "all miss")
    assert got[2] == w * h and (got[0] == got[0][0, 0]).all()
    # a normal frame right behind it on the same context
    cam = csr.hall_cameras(vrt)["orbit_1"]
    _check(_case_frame(vrt, ds, cam, case, counts=np.ones((H, W), np.uint32)),
           _frame(_path(vrt, ds, cam, W, H, 1, case["bounces"], case["seed"], case["shadow"]), W, H), "every count is 1")
    # an empty window: 0, dst untouched
    out = _adaptive(vrt, ds, cam, W, H, ac.counts_of(case), case["cap"], case["bounces"], case["seed"], case["shadow"], 7, 7)
    got = _frame(out, W, H)
    assert (got[0] == MARK).all() and got[2] == 0


# ---- 8: two frames in flight ----
def test_two_frames_in_flight(vrt, po, hall):
    import torch
    b, ds = hall
    dev = ds.t["tri"].device
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cams = [csr.orbit(vrt, 1), csr.orbit(vrt, 6)]
        raws = [ac.counts_of(c) for c in ac.IN_FLIGHT]
        cts = [_u32(dev, r) for r in raws]
        outs = [_outputs(dev, W, H) for _ in range(2)]
        torch.cuda.synchronize()
        for rnd in range(2):      # (the second round finds the contexts' buffers grown: no synchronisation at all)
            for i, c in enumerate(ac.IN_FLIGHT):
                _adaptive(vrt, ds, cams[i], W, H, cts[i], c["cap"], c["bounces"], c["seed"], c["shadow"], stream=streams[i].cuda_stream, out=outs[i])
            torch.cuda.synchronize()
            if rnd == 0:
                for o in outs:
                    o[0].fill_(MARK), o[1].zero_(), o[2].zero_()
                torch.cuda.synchronize()
        for i, c in enumerate(ac.IN_FLIGHT):
            want = ar.frame(b, cams[i], W, H, po.shade_params(), raws[i], c["cap"], c["bounces"], c["seed"], c["shadow"])
            _check(_frame(outs[i], W, H), want, "in flight %d" % i)
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)


# ---- 9: refusals ----
def _call(vrt, accel, px, counts, cam, y0=0, y1=H, params="default", path="default"):
    L = vrt.rtapi._lib()
    p = vrt.rtapi.default_shade_params()
    pref = C.byref(p) if params == "default" else params
    q = vrt.rtapi.PathParams(2, 3, 0, 1)
    qref = C.byref(q) if path == "default" else (C.byref(path) if path is not None else None)
    cref = C.byref(cam) if cam is not None else None
    return L.vxrt_render_path_adaptive(accel, cref, W, H, y0, y1, pref, qref, None if counts is None else counts.data_ptr(), px.data_ptr(), None, None, _stream())


def test_refusals(vrt, hall):
    import torch
    b, ds = hall
    dev = ds.t["tri"].device
    px = torch.full((H, W), MARK, dtype=torch.int32, device=dev)
    counts = _u32(dev, np.full((H, W), 2, np.uint32))
    base = csr.framing(W, H)
    good = vrt.rtapi.Camera.from_cam14(base)
    PP = vrt.rtapi.PathParams
    for cam in (good, None):
        assert _call(vrt, ds.accel, px, None, cam) == -1                                   # null counts
        assert _call(vrt, ds.accel, px, counts, cam, path=None) == -1
        for bad in (PP(0, 3, 0, 1), PP(4097, 3, 0, 1), PP(2, vrt.rtapi.PATH_MAX_BOUNCES + 1, 0, 1), PP(2, 3, 0, 2)):
            assert _call(vrt, ds.accel, px, counts, cam, path=bad) == -1
        assert _call(vrt, ds.accel, px, counts, cam, y0=5, y1=3) == -1
        assert _call(vrt, ds.accel, px, counts, cam, y0=0, y1=H + 1) == -1
        assert _call(vrt, ds.accel, px, counts, cam, params=None) == -1
        assert _call(vrt, None, px, counts, cam) == -1
        assert _call(vrt, ds.accel, px, counts, cam, y0=7, y1=7) == 0                      # the empty window
    for i in range(14):
        for v in (float("nan"), float("inf"), -float("inf")):
            c = base.copy()
            c[i] = v
            assert _call(vrt, ds.accel, px, counts, vrt.rtapi.Camera.from_cam14(c)) == -1
    L = vrt.rtapi._lib()
    p, q = vrt.rtapi.default_shade_params(), PP(2, 3, 0, 1)
    assert L.vxrt_render_path_adaptive(ds.accel, C.byref(good), W, H, 0, H, C.byref(p), C.byref(q), counts.data_ptr(), None, None, None, _stream()) == -1   # null dst
    torch.cuda.synchronize()
    assert (px.cpu().numpy() == MARK).all()
    assert vrt.rtapi.status(_stream()) == 0


def test_alpha_table_is_refused(vrt, golden, gpu_device):
    import torch
    import shading_ref as sr
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in KEYS}, gpu_device)
    try:
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        counts = _u32(gpu_device, np.full((H, W), 2, np.uint32))
        cam = vrt.rtapi.Camera.from_cam14(csr.golden_cameras(vrt)["g_orbit_1"])
        assert _call(vrt, ds.accel, px, counts, cam) == -1 and _call(vrt, ds.accel, px, counts, None) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
        ds.set_alpha_test(None)
        assert _call(vrt, ds.accel, px, counts, cam) == 0
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
        counts = _u32(gpu_device, np.full((H, W), 2, np.uint32))
        assert _call(vrt, ds.accel, px, counts, vrt.rtapi.Camera.from_cam14(csr.framing(W, H))) == -1
        assert _call(vrt, ds.accel, px, counts, None) == -1
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all()
    finally:
        ds.close()


# ---- 10: the variance frame ----
AOV = (("noisy", 3), ("direct", 3), ("albedo", 3), ("position", 4), ("normal", 4))
INST = mr.INSTANCES


def _same_floats(got, want, what):
    """bit for bit, except that a NaN of the restatement asks for a NaN of any payload"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what + ": a NaN of the restatement is not a NaN"
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=what)


@pytest.fixture(scope="module")
def moving_hall(vrt):
    return mc.hall(vrt)


def _cameras(vrt, n):
    return [np.array(vrt.rtapi.look_at(e, tc.PATH_CENTRE, (0.0, 1.0, 0.0), 1.0, W, H).cam14(), np.float32) for e in tc.PATH_EYES][:n]


def _v_outputs(dev):
    import torch
    o = {"px": torch.full((H, W), MARK, dtype=torch.int32, device=dev), "col": torch.full((H, W, 3), FMARK, dtype=torch.float32, device=dev),
         "cnt": torch.zeros(1, dtype=torch.int64, device=dev), "hist": torch.full((H * W * 4,), FMARK, dtype=torch.float32, device=dev),
         "mom": torch.full((H * W * 2,), FMARK, dtype=torch.float32, device=dev), "prev": torch.full((H, W, 4), FMARK, dtype=torch.float32, device=dev),
         "var": torch.full((H, W), FMARK, dtype=torch.float32, device=dev)}
    for k, c in AOV:
        o[k] = torch.full((H, W, c), FMARK, dtype=torch.float32, device=dev)
    return o


def _move(ds, k):
    ds.snapshot_motion(INST)
    if k:
        ds.set_transforms([mc.translation(k)], mc.BLOB)


def _v_frame(vrt, ds, hist, cam, cap, bounces, shadow, seed, counts=None, motion=0, dn=dc.PATH_DN, out=None, stream=None):
    """vxrt_render_path_variance_adaptive with device counts, or vxrt_render_path_variance (counts None) with spp = cap; the history and its
    moments are read behind the frame on the same stream"""
    o = out or _v_outputs(ds.device)
    s = _stream() if stream is None else stream
    R = vrt.rtapi
    aov = R.PathAov(*[o[n].data_ptr() for n, _ in AOV])
    head = (ds.accel, cam, W, H, 0, H, R.default_shade_params(), cap, bounces)
    tail = (R.DenoiseParams(*dn), R.TemporalParams(*tc.PATH_TP), R.VarianceParams(*vc.PATH_VP), hist, o["px"].data_ptr(), motion, seed, shadow, o["col"].data_ptr(),
            aov, o["prev"].data_ptr() if motion else None, o["var"].data_ptr(), o["cnt"].data_ptr(), s)
    if counts is None:
        R.render_path_variance(*(head + tail))
    else:
        R.render_path_variance_adaptive(*(head + (counts.data_ptr(),) + tail))
    hist.read_moments(o["mom"].data_ptr(), s)
    hist.read(o["hist"].data_ptr(), s)
    return o


def _host(o):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "px" else int(v.item()) if k == "cnt" else v.cpu().numpy()) for k, v in o.items()}


def _v_check(got, want, what, motion=0):
    _same_floats(got["col"], want["col"], what + ": colours")
    np.testing.assert_array_equal(got["px"], want["px"], err_msg=what + ": pixels")
    assert got["cnt"] == want["rays"], "%s: rays traced %d, restatement %d" % (what, got["cnt"], want["rays"])
    for k, _ in AOV:
        _same_floats(got[k], want[k], what + ": " + k)
    if motion:
        _same_floats(got["prev"], want["prev_position"], what + ": prev_position")
    else:
        assert (got["prev"] == f32(FMARK)).all(), what
    _same_floats(got["var"], want["variance"], what + ": variance")
    _same_floats(got["hist"].reshape(H, W, 4), want["T"], what + ": the history")
    _same_floats(got["mom"].reshape(H, W, 2), want["M"], what + ": the moments")


def test_variance_frame_uniform_identity(vrt, gpu_device, moving_hall):
    """counts == spp everywhere over a 3-frame orbit against vxrt_render_path_variance on a second history: dst, colours, variance, every
    guide output, vxrt_history_read and vxrt_history_read_moments"""
    spp, bounces, shadow, seed = dc.PATH_CONFIGS[0]
    ds = vrt.tracer.DeviceScene(moving_hall, gpu_device)
    try:
        counts = _u32(ds.device, np.full((H, W), spp, np.uint32))
        with vrt.rtapi.History(W, H, moments=True) as ha, vrt.rtapi.History(W, H, moments=True) as hu:
            for k, cam in enumerate(_cameras(vrt, 3)):
                _move(ds, k)
                a = _host(_v_frame(vrt, ds, ha, cam, spp, bounces, shadow, seed + k, counts))
                u = _host(_v_frame(vrt, ds, hu, cam, spp, bounces, shadow, seed + k))
                assert a["cnt"] == u["cnt"] and a["cnt"] > W * H
                for key in a:
                    if key != "cnt":
                        np.testing.assert_array_equal(np.asarray(a[key]).view(np.uint32), np.asarray(u[key]).view(np.uint32), err_msg="frame %d %s" % (k, key))
            assert (a["hist"].reshape(H, W, 4)[..., 3] > 1).any() and (a["var"] > 0).any()
    finally:
        ds.close()


@pytest.mark.parametrize("motion", (0, 1))
def test_variance_frame_against_the_restatement(vrt, po, gpu_device, moving_hall, motion):
    case = ac.VARIANCE
    seq, cams = mc.sequence(moving_hall)[:2], _cameras(vrt, 2)
    raws = [ac.hashed(W, H, case["values"], 20 + k) for k in range(2)]
    ds = vrt.tracer.DeviceScene(moving_hall, gpu_device)
    try:
        ref = vr.History()
        with vrt.rtapi.History(W, H, moments=True) as hist:
            for k, cam in enumerate(cams):
                _move(ds, k)
                got = _host(_v_frame(vrt, ds, hist, cam, case["cap"], case["bounces"], case["shadow"], case["seed"] + k, _u32(ds.device, raws[k]), motion))
                want = ar.variance_frame(seq[k][0], seq[k][1], cam, W, H, po.shade_params(), raws[k], case["cap"], case["bounces"], case["seed"] + k, case["shadow"],
                                         dc.PATH_DN, tc.PATH_TP, vc.PATH_VP, ref, motion)
                _v_check(got, want, "motion %d frame %d" % (motion, k), motion)
            assert (want["T"][..., 3] > 1).any() and (want["variance"] > 0).any()
    finally:
        ds.close()


def test_variance_frame_refusals(vrt, gpu_device, moving_hall):
    import torch
    L = vrt.rtapi._lib()
    R = vrt.rtapi
    spp, bounces, shadow, seed = dc.PATH_CONFIGS[0]
    px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
    counts = _u32(gpu_device, np.full((H, W), 2, np.uint32))
    ds = vrt.tracer.DeviceScene(moving_hall, gpu_device)
    try:
        with R.History(W, H, moments=True) as hist, R.History(W, H) as plain, R.History(W, H // 2, moments=True) as small:
            p, q, d, t, v = R.default_shade_params(), R.PathParams(spp, bounces, seed, shadow), R.DenoiseParams(*dc.PATH_DN), R.TemporalParams(*tc.PATH_TP), \
                R.VarianceParams(*vc.PATH_VP)
            good = R.Camera.from_cam14(_cameras(vrt, 1)[0])

            def call(accel=ds.accel, cam=good, y0=0, y1=H, params=p, path=q, cp=counts.data_ptr(), dn=d, tp=t, vp=v, hh=hist.handle, motion=0, dst=px.data_ptr()):
                ref = [None if x is None else C.byref(x) for x in (cam, params, path, dn, tp, vp)]
                return L.vxrt_render_path_variance_adaptive(accel, ref[0], W, H, y0, y1, ref[1], ref[2], cp, ref[3], ref[4], ref[5], hh, motion, dst, None, None, None,
                                                            None, None, _stream())
            assert call(cp=None) == -1                                                    # null counts
            assert call(hh=plain.handle) == -1                                            # a history without moments
            assert call(motion=1) == -1                                                   # no snapshot
            for kw in ({"cam": None}, {"accel": None}, {"params": None}, {"path": None}, {"dn": None}, {"tp": None}, {"vp": None}, {"hh": None}, {"dst": None}):
                assert call(**kw) == -1, kw
            assert call(vp=R.VarianceParams(0.0, 3, 2, 0)) == -1 and call(path=R.PathParams(4097, 3, 0, 1)) == -1 and call(motion=2) == -1
            assert call(y0=5, y1=3) == -1 and call(hh=small.handle) == -1
            assert call(y0=7, y1=7) == 0                                                  # the empty window
            torch.cuda.synchronize()
            assert (px.cpu().numpy() == MARK).all()
            assert L.vxrt_history_read(hist.handle, px.data_ptr(), _stream()) == -1       # still empty
            assert call() == 0
            torch.cuda.synchronize()
            assert (px.cpu().numpy() != MARK).all()
    finally:
        ds.close()


# ---- 11: vxrt_sample_counts ----
def _sample_counts(vrt, dev, v, prm, prev=None, start=12345678901):
    import torch
    n = len(v)
    vt = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    pt = None if prev is None else _u32(dev, prev)
    out = _u32(dev, np.full(n + 64, CMARK, np.uint32))
    total = torch.full((1,), start, dtype=torch.int64, device=dev)
    vrt.rtapi.sample_counts(n, vt.data_ptr(), vrt.rtapi.SampleCountParams(prm[0], prm[1], prm[2], 0), out.data_ptr(), None if pt is None else pt.data_ptr(),
                            total.data_ptr(), _stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    assert (o[n:] == CMARK).all(), "written past the end of counts"
    return o[:n], int(total.item()) - start


@pytest.mark.parametrize("prm", ac.SAMPLE_PRMS)
def test_sample_counts_against_the_restatement(vrt, gpu_device, prm):
    v = ac.hostile_variances(prm)
    got, total = _sample_counts(vrt, gpu_device, v, prm)
    want, wtotal = ar.sample_counts(v, prm)
    np.testing.assert_array_equal(got, want, err_msg="the hostile table %r" % (prm,))
    assert total == wtotal
    for n in ac.SAMPLE_SIZES:
        vv, pp = ac.sample_inputs(n, prm, n)
        for prev in (pp, None):
            got, total = _sample_counts(vrt, gpu_device, vv, prm, prev)
            want, wtotal = ar.sample_counts(vv, prm, prev)
            np.testing.assert_array_equal(got, want, err_msg="n %d %r prev %r" % (n, prm, prev is not None))
            assert total == wtotal


def test_sample_counts_without_total_and_refusals(vrt, gpu_device):
    import torch
    L = vrt.rtapi._lib()
    SP = vrt.rtapi.SampleCountParams
    n = 300
    v, prev = ac.sample_inputs(n, (0.5, 1, 16), 3)
    vt, pt = torch.from_numpy(v).to(gpu_device), _u32(gpu_device, prev)
    out = _u32(gpu_device, np.full(n, CMARK, np.uint32))
    total = torch.full((1,), 77, dtype=torch.int64, device=gpu_device)
    nan, inf = float("nan"), float("inf")

    def call(nn=n, var=vt.data_ptr(), pr_=pt.data_ptr(), prm=SP(0.5, 1, 16, 0), o=out.data_ptr(), tot=total.data_ptr()):
        return L.vxrt_sample_counts(nn, var, pr_, None if prm is None else C.byref(prm), o, tot, _stream())
    assert call(var=None) == -1 and call(o=None) == -1 and call(prm=None) == -1
    for bad in (SP(0.0, 1, 16, 0), SP(-1.0, 1, 16, 0), SP(nan, 1, 16, 0), SP(inf, 1, 16, 0), SP(0.5, 0, 16, 0), SP(0.5, 17, 16, 0), SP(0.5, 1, 4097, 0),
                SP(0.5, 1, 16, 1)):
        assert call(prm=bad) == -1
    assert call(nn=1 << 31) == -1 and call(nn=(1 << 40) + 5) == -1
    assert call(nn=0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == CMARK).all() and int(total.item()) == 77
    assert call(tot=None) == 0                                                            # without a total
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ar.sample_counts(v, (0.5, 1, 16), prev)[0])
    assert int(total.item()) == 77
    assert call(prm=SP(0.5, 16, 16, 0)) == 0 and call(prm=SP(0.5, 4096, 4096, 0)) == 0    # min_spp = max_spp, and both at the limit


# ---- 12: the closed loop ----
def test_closed_loop_on_one_stream(vrt, po, gpu_device, moving_hall):
    """three frames: vxrt_render_path_variance_adaptive -> its `variance` output -> vxrt_sample_counts (the frame's counts as
    prev_counts) -> the next frame's counts, all enqueued on one stream with no host call that waits in between; then against the
    restatement fed the same sequence"""
    import torch
    lp = ac.LOOP
    n = lp["frames"]
    R = vrt.rtapi
    cams = _cameras(vrt, n)
    ds = vrt.tracer.DeviceScene(moving_hall, gpu_device)
    try:
        prm = R.SampleCountParams(lp["prm"][0], lp["prm"][1], lp["prm"][2], 0)
        cts = [_u32(ds.device, np.full((H, W), lp["first"], np.uint32))] + [_u32(ds.device, np.full((H, W), CMARK, np.uint32)) for _ in range(n)]
        total = torch.zeros(n, dtype=torch.int64, device=ds.device)
        outs = [_v_outputs(ds.device) for _ in range(n)]
        with R.History(W, H, moments=True) as hist, R.History(W, H, moments=True) as warm:
            # (a frame on another history first, so that the contexts' buffers have their size and nothing below synchronises)
            _v_frame(vrt, ds, warm, cams[0], lp["cap"], lp["bounces"], lp["shadow"], lp["seed"], cts[0])
            torch.cuda.synchronize()
            s = _stream()
            for k in range(n):
                _v_frame(vrt, ds, hist, cams[k], lp["cap"], lp["bounces"], lp["shadow"], lp["seed"] + k, cts[k], out=outs[k], stream=s)
                R.sample_counts(W * H, outs[k]["var"].data_ptr(), prm, cts[k + 1].data_ptr(), cts[k].data_ptr(), total[k:].data_ptr(), s)
            got = [_host(o) for o in outs]
            got_counts = [c.cpu().numpy().view(np.uint32).reshape(H, W) for c in cts]
            got_total = total.cpu().numpy()
        ref = vr.History()
        raw = np.full((H, W), lp["first"], np.uint32)
        for k in range(n):
            np.testing.assert_array_equal(got_counts[k], raw, err_msg="the counts of frame %d" % k)
            want = ar.variance_frame(moving_hall, None, cams[k], W, H, po.shade_params(), raw, lp["cap"], lp["bounces"], lp["seed"] + k, lp["shadow"],
                                     dc.PATH_DN, tc.PATH_TP, vc.PATH_VP, ref)
            _v_check(got[k], want, "loop frame %d" % k)
            nxt, tot = ar.sample_counts(want["variance"], lp["prm"], raw)
            assert int(got_total[k]) == tot
            raw = nxt.reshape(H, W)
            assert (np.bincount(nxt, minlength=5) >= 100).sum() >= 3, "the loop's counts for frame %d are (nearly) uniform" % (k + 1)
        np.testing.assert_array_equal(got_counts[n], raw)
    finally:
        ds.close()
