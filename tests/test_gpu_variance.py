"""GPU: variance guidance -- the history with moments and its step (vxrt_temporal_accumulate_moments), the initial variance
(vxrt_history_variance), the variance-guided filter (vxrt_denoise_variance) and the frame (vxrt_render_path_variance) -- against the
restatement tests/variance_ref.py, bit for bit: f32 as u32, pixels, rays traced, the guide outputs, the history and its moments after
every frame, guard floats behind every output.  No masks, no tolerances, with the one exception of tests/test_gpu_temporal.py: where the
restatement gives a NaN the kernel must give a NaN of any payload.  tests/test_variance_cpu.py shows that the cases
(tests/variance_cases.py) are not vacuous and holds the restatement to what the definition is for."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import motion_cases as mc
import motion_ref as mr
import temporal_cases as tc
import variance_cases as vc
import variance_ref as vr

pytestmark = pytest.mark.gpu
W, H = dc.W, dc.H
MARK = 0x5A5A5A
FMARK = -12345.5   # marker of float outputs
GUARD = 64         # floats past the end of an output
AOV = (("noisy", 3), ("direct", 3), ("albedo", 3), ("position", 4), ("normal", 4))
WINDOWS = ((0, H), dc.PATH_WINDOW)
N_FRAMES = vc.N_PATH_FRAMES
INST = mr.INSTANCES
f32 = np.float32


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


def _device(dev, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in arrays]


def _marked(dev, n_floats):
    import torch
    return torch.full((n_floats + GUARD,), FMARK, dtype=torch.float32, device=dev)


def _unguarded(t, n, what):
    """the first n floats of a marked output; nothing may be written behind them"""
    a = t.cpu().numpy()
    assert (a[n:] == f32(FMARK)).all(), "written past the end of " + what
    return a[:n]


# ---- the step and the initial variance ----
def _perturbed(P, N, seed):
    """guides of a previous frame that is not this one (as tests/test_gpu_motion.py makes them, fewer kinds)"""
    rng = np.random.RandomState(seed)
    rows, w = P.shape[:2]
    Q, Nq = P.copy(), N.copy()
    Q[..., :3] += (np.array([0.3, -0.2, 0.25]) + rng.normal(0.0, 0.05, (rows, w, 3))).astype(np.float32)
    Q[..., 3] = 1.0
    Nq[..., :3] += rng.normal(0.0, 0.05, (rows, w, 3)).astype(np.float32)
    k = rows * w
    idx = rng.permutation(k)[: max(1, k // 6) if k > 1 else 0]
    qf, nf = Q.reshape(-1, 4), Nq.reshape(-1, 4)
    for i, p in enumerate(idx):
        m = i % 8
        if m < 4:
            qf[p, 3] = (0.0, -0.0, np.nan, 2.5)[m]
        elif m < 6:
            qf[p, m - 4] = (np.inf, np.nan)[m - 4]
        elif m == 6:
            nf[p, :3] = 0.0
        else:
            nf[p, 1] = np.nan
    return Q, Nq


def _accumulate(vrt, dev, hist, cam, w, h, win, E, P, N, prm, Q=None, Nq=None):
    """the step on device copies: on a history with moments vxrt_temporal_accumulate_moments -- (out, HE read back, HM read back) -- and
    on a plain one vxrt_temporal_accumulate[_motion] -- (out, HE read back)"""
    import torch
    n = (win[1] - win[0]) * w
    t = _device(dev, *((E, P, N) + (() if Q is None else (Q, Nq))))
    out, rd, rm = _marked(dev, n * 4), _marked(dev, n * 4), _marked(dev, n * 2)
    tp = vrt.rtapi.TemporalParams(*prm)
    a = (hist, cam, w, h, win[0], win[1], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    if hist.moments:
        vrt.rtapi.temporal_accumulate_moments(*a, tp, out.data_ptr(), None if Q is None else t[3].data_ptr(), None if Q is None else t[4].data_ptr(), _stream())
        hist.read_moments(rm.data_ptr(), _stream())
    elif Q is None:
        vrt.rtapi.temporal_accumulate(*a, tp, out.data_ptr(), _stream())
    else:
        vrt.rtapi.temporal_accumulate_motion(*a, t[3].data_ptr(), t[4].data_ptr(), tp, out.data_ptr(), _stream())
    hist.read(rd.data_ptr(), _stream())
    torch.cuda.synchronize()
    shape = (win[1] - win[0], w)
    res = (_unguarded(out, n * 4, "out4").reshape(shape + (4,)), _unguarded(rd, n * 4, "vxrt_history_read").reshape(shape + (4,)))
    if hist.moments:
        res += (_unguarded(rm, n * 2, "vxrt_history_read_moments").reshape(shape + (2,)),)
    else:
        assert (rm.cpu().numpy() == f32(FMARK)).all()
    return res


def _variance(vrt, dev, hist, n, npow, sz, vp):
    import torch
    v = _marked(dev, n)
    vrt.rtapi.history_variance(hist, vrt.rtapi.DenoiseParams(1, npow, sz, 1.0), vrt.rtapi.VarianceParams(*vp), v.data_ptr(), _stream())
    torch.cuda.synchronize()
    return _unguarded(v, n, "vxrt_history_variance")


@pytest.mark.parametrize("motion", (0, 1))
@pytest.mark.parametrize("w,h,name", vc.all_sequences())
def test_step_and_initial_variance_against_the_restatement(vrt, gpu_device, w, h, name, motion):
    """frame by frame: out4, vxrt_history_read, vxrt_history_read_moments and vxrt_history_variance under every parameter set; and out4 is
    what the plain step gives on a history without moments"""
    fr, win, prm = tc.frames(w, h, name)
    rows = win[1] - win[0]
    ref = vr.History()
    spatial = temporal = 0
    with vrt.rtapi.History(w, rows, moments=True) as hist, vrt.rtapi.History(w, rows) as plain:
        for k, (cam, E, P, N, _, _) in enumerate(fr):
            Q, Nq = _perturbed(P, N, 100 + k) if motion else (None, None)
            want, wm = vr.step(E, P, N, ref, cam, w, h, win[0], win[1], prm, Q, Nq)
            got, read, mom = _accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm, Q, Nq)
            what = "%dx%d %s frame %d motion %d" % (w, h, name, k, motion)
            _same_floats(got, want, what)
            _same_floats(read, want, what + ": vxrt_history_read")
            _same_floats(mom, wm, what + ": vxrt_history_read_moments")
            pg, pr_ = _accumulate(vrt, gpu_device, plain, cam, w, h, win, E, P, N, prm, Q, Nq)
            np.testing.assert_array_equal(_bits(got), _bits(pg), err_msg=what + ": out4 against the plain step")
            np.testing.assert_array_equal(_bits(read), _bits(pr_), err_msg=what + ": HE against the plain step")
            for vp in vc.VPS:
                for npow, sz in vc.V0_GUIDES:
                    st = {}
                    wv = vr.initial_variance(ref, npow, sz, vp[1], vp[2], st)
                    _same_floats(_variance(vrt, gpu_device, hist, rows * w, npow, sz, vp).reshape(rows, w), wv, what + ": V0 %r %r" % (vp, (npow, sz)))
                    spatial += st["v0_spatial"]
                    temporal += st["v0_temporal"]
    assert (spatial > 0 and temporal > 0) or (w, h) not in vc.BIG


# ---- the filter ----
def _filter(vrt, dev, w, h, t, case, want_variance=True, rc=False):
    import torch
    it, npow, sz, sl, eps = case
    n = w * h
    out, outv = _marked(dev, n * 3), _marked(dev, n)
    nb = vrt.rtapi.denoise_variance_scratch_bytes(w, h)
    scratch = torch.full((nb // 4 + GUARD,), FMARK, dtype=torch.float32, device=dev)
    vrt.rtapi.denoise_variance(w, h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), vrt.rtapi.DenoiseParams(it, npow, sz, sl),
                               vrt.rtapi.VarianceParams(eps, 4, 1), out.data_ptr(), outv.data_ptr() if want_variance else None, scratch.data_ptr(), nb, _stream())
    torch.cuda.synchronize()
    assert (scratch.cpu().numpy()[nb // 4:] == f32(FMARK)).all(), "written past the end of scratch"
    F = _unguarded(out, n * 3, "out").reshape(h, w, 3)
    if not want_variance:
        assert (outv.cpu().numpy() == f32(FMARK)).all()
        return F, None
    return F, _unguarded(outv, n, "out_variance").reshape(h, w)


@pytest.mark.parametrize("w,h", vc.FRAMES)
def test_filter_against_the_restatement(vrt, gpu_device, w, h):
    S, P, N, _, _ = dc.synthetic(w, h)
    V = vc.variance(w, h)
    t = _device(gpu_device, S, V, P, N)
    for case in vc.filter_cases():
        wf, wv = vr.atrous_v(S, V, P, N, *case)
        F, VF = _filter(vrt, gpu_device, w, h, t, case)
        _same_floats(F, wf, "%dx%d %r" % (w, h, case))
        _same_floats(VF, wv, "%dx%d %r: the variance" % (w, h, case))
    case = vc.filter_cases()[-1]
    F, _ = _filter(vrt, gpu_device, w, h, t, case, want_variance=False)
    _same_floats(F, vr.atrous_v(S, V, P, N, *case)[0], "%dx%d without out_variance" % (w, h))
    F, VF = _filter(vrt, gpu_device, w, h, t, (0,) + case[1:])
    np.testing.assert_array_equal(_bits(F), _bits(S))                    # iterations = 0: copies, payloads of NaNs included
    np.testing.assert_array_equal(_bits(VF), _bits(V))


def test_filter_and_variance_refusals(vrt, gpu_device):
    import torch
    L = vrt.rtapi._variance_lib()
    DP, VP = vrt.rtapi.DenoiseParams, vrt.rtapi.VarianceParams
    nan, inf = float("nan"), float("inf")
    w, h = 45, 37
    n = w * h
    S, P, N, _, _ = dc.synthetic(w, h)
    t = _device(gpu_device, S, vc.variance(w, h), P, N)
    out, outv = _marked(gpu_device, n * 3), _marked(gpu_device, n)
    nb = vrt.rtapi.denoise_variance_scratch_bytes(w, h)
    assert nb == 32 * n
    scratch = torch.zeros(nb // 4 + 8, dtype=torch.float32, device=gpu_device)
    bad_vp = (VP(0.0, 4, 1, 0), VP(-1.0, 4, 1, 0), VP(nan, 4, 1, 0), VP(inf, 4, 1, 0), VP(1e-3, 0, 1, 0), VP(1e-3, vrt.rtapi.TEMPORAL_MAX_LEN + 1, 1, 0),
              VP(1e-3, 4, 0, 0), VP(1e-3, 4, 4, 0), VP(1e-3, 4, 1, 1))
    bad_dn = (DP(7, 2, 1.0, 1.0), DP(3, 8, 1.0, 1.0), DP(3, 2, 0.0, 1.0), DP(3, 2, 1.0, nan), DP(3, 2, 1.0, 0.0))

    def call(ww=w, hh=h, off=(0, 0, 0, 0), dn=DP(3, 2, 1.0, 4.0), vp=VP(1e-3, 4, 1, 0), o=out.data_ptr(), ov=outv.data_ptr(), sc=scratch.data_ptr(), sb=nb, null=()):
        a = [None if i in null else t[i].data_ptr() + off[i] for i in range(4)]
        return L.vxrt_denoise_variance(ww, hh, a[0], a[1], a[2], a[3], None if dn is None else C.byref(dn), None if vp is None else C.byref(vp), o, ov, sc, sb,
                                       _stream())
    assert call(dn=None) == -1 and call(vp=None) == -1 and call(o=None) == -1
    for i in range(4):
        assert call(null=(i,)) == -1
    assert call(off=(0, 0, 4, 0)) == -1 and call(off=(0, 0, 0, 8)) == -1                 # guides not 16-byte aligned
    assert call(o=t[0].data_ptr()) == -1 and call(ov=t[1].data_ptr()) == -1              # an output aliases its input
    assert call(sc=None) == -1 and call(sc=scratch.data_ptr() + 4) == -1 and call(sb=nb - 1) == -1
    assert call(ww=65536, hh=32768) == -1
    for bad in bad_vp:
        assert call(vp=bad) == -1
    for bad in bad_dn:
        assert call(dn=bad) == -1
    assert call(ww=0) == 0 and call(hh=0) == 0                                            # the empty window
    # vxrt_history_variance: empty, without moments, bad parameters, null
    fr, win, prm = tc.frames(w, h, "pan")
    cam, E, P, N = fr[0][:4]
    v = _marked(gpu_device, n)
    d, p = DP(1, 2, 1.0, 1.0), VP(1e-3, 4, 1, 0)
    with vrt.rtapi.History(w, h, moments=True) as hist, vrt.rtapi.History(w, h) as plain:
        hv = lambda hh=hist.handle, dn=d, vp=p, ptr=v.data_ptr(): L.vxrt_history_variance(hh, None if dn is None else C.byref(dn), None if vp is None else C.byref(vp),
                                                                                          ptr, _stream())
        assert hv() == -1 and L.vxrt_history_read_moments(hist.handle, v.data_ptr(), _stream()) == -1            # empty
        _accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm)
        _accumulate(vrt, gpu_device, plain, cam, w, h, win, E, P, N, prm)
        assert hv(hh=None) == -1 and hv(dn=None) == -1 and hv(vp=None) == -1 and hv(ptr=None) == -1
        assert hv(hh=plain.handle) == -1 and L.vxrt_history_read_moments(plain.handle, v.data_ptr(), _stream()) == -1
        assert L.vxrt_history_read_moments(hist.handle, None, _stream()) == -1 and L.vxrt_history_read_moments(None, v.data_ptr(), _stream()) == -1
        for bad in bad_vp:
            assert hv(vp=bad) == -1
        for bad in bad_dn:
            assert hv(dn=bad) == -1
        torch.cuda.synchronize()
        assert (v.cpu().numpy() == f32(FMARK)).all() and (out.cpu().numpy() == f32(FMARK)).all() and (outv.cpu().numpy() == f32(FMARK)).all()
        assert hv() == 0 and call() == 0
        hist.reset()
        assert hv() == -1


def test_step_refusals_and_the_two_kinds_of_history(vrt, gpu_device):
    """the refusals of vxrt_temporal_accumulate_moments, the two cross-kind refusals, and the history after them: the next frame is the
    sequence's"""
    import torch
    L = vrt.rtapi._variance_lib()
    w, h = 45, 37
    fr, win, prm = tc.frames(w, h, "pan")
    cam, E, P, N = fr[0][:4]
    t = _device(gpu_device, E, P, N, P, N)
    out = _marked(gpu_device, w * h * 4)
    good_cam, good = vrt.rtapi.Camera.from_cam14(cam), vrt.rtapi.TemporalParams(*prm)
    h0 = C.c_void_p()
    assert L.vxrt_history_create_moments(0, 4, C.byref(h0)) == -1 and L.vxrt_history_create_moments(4, 0, C.byref(h0)) == -1
    assert L.vxrt_history_create_moments(4, 4, None) == -1 and L.vxrt_history_create_moments(65536, 32768, C.byref(h0)) == -1
    with vrt.rtapi.History(w, h, moments=True) as hist, vrt.rtapi.History(w, h) as plain, vrt.rtapi.History(w, h // 2, moments=True) as small:
        def call(f=L.vxrt_temporal_accumulate_moments, hh=hist.handle, c=good_cam, ww=w, fh=h, y0=0, y1=h, off=(0, 0, 0, 0, 0), p=good, null=(), motion=True):
            a = [None if i in null else t[i].data_ptr() + off[i] for i in range(5)]
            a = a if motion else a[:3] + [None, None]
            return f(hh, None if c is None else C.byref(c), ww, fh, y0, y1, a[0], a[1], a[2], a[3], a[4], None if p is None else C.byref(p),
                     None if 5 in null else out.data_ptr(), _stream())
        assert call(hh=None) == -1 and call(c=None) == -1 and call(p=None) == -1
        for i in (0, 1, 2, 5):
            assert call(null=(i,)) == -1
        assert call(null=(3,)) == -1 and call(null=(4,)) == -1                            # one of the two motion guides
        for i in range(1, 5):
            off = [0] * 5
            off[i] = 4 + 4 * (i % 2)
            assert call(off=tuple(off)) == -1                                             # not 16-byte aligned
        bad = np.array(cam, np.float32)
        bad[5] = np.nan
        assert call(c=vrt.rtapi.Camera.from_cam14(bad)) == -1
        assert call(ww=65536, fh=32768, y1=32768) == -1 and call(fh=h + 1, y1=h + 1) == -1
        assert call(ww=0) == -1 and call(fh=0, y1=0) == -1 and call(y0=5, y1=3) == -1 and call(y1=h + 1) == -1
        assert call(p=vrt.rtapi.TemporalParams(0.0, 32, 0.5, 0.9)) == -1 and call(p=vrt.rtapi.TemporalParams(0.1, 32, 0.5, np.nan)) == -1
        assert call(hh=small.handle) == -1                                                # a window larger than the capacity
        # the two kinds do not mix
        assert call(hh=plain.handle) == -1 and call(hh=plain.handle, motion=False) == -1
        assert call(f=L.vxrt_temporal_accumulate_motion) == -1
        assert L.vxrt_temporal_accumulate(hist.handle, C.byref(good_cam), w, h, 0, h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), C.byref(good),
                                          out.data_ptr(), _stream()) == -1
        assert call(y0=7, y1=7) == 0                                                      # the empty window
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == f32(FMARK)).all()
        for hh in (hist, plain, small):
            assert L.vxrt_history_read(hh.handle, out.data_ptr(), _stream()) == -1        # still empty, all of them
        # the sequence goes on as if nothing had been refused, both kinds; then a refusal in mid-sequence
        ref = vr.History()
        for k, (cam, E, P, N, _, _) in enumerate(fr[:3]):
            if k == 2:
                assert call(hh=plain.handle) == -1 and call(f=L.vxrt_temporal_accumulate_motion) == -1 and call(p=None) == -1
            want, wm = vr.step(E, P, N, ref, cam, w, h, win[0], win[1], prm)
            got, read, mom = _accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm)
            _same_floats(got, want, "frame %d after the refusals" % k)
            _same_floats(mom, wm, "frame %d after the refusals: moments" % k)
            pg, _ = _accumulate(vrt, gpu_device, plain, cam, w, h, win, E, P, N, prm)
            np.testing.assert_array_equal(_bits(got), _bits(pg))
        # a reset: the next frame is a first frame, moments included
        hist.reset()
        cam, E, P, N = fr[3][:4]
        fresh = vr.History()
        want, wm = vr.step(E, P, N, fresh, cam, w, h, win[0], win[1], prm)
        got, read, mom = _accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm)
        _same_floats(got, want, "after a reset")
        _same_floats(mom, wm, "after a reset: moments")
        assert (want[..., 3] <= 1).all()


# ---- the frame ----
@pytest.fixture(scope="module")
def hall(vrt):
    return mc.hall(vrt)


def _cameras(vrt):
    return [np.array(vrt.rtapi.look_at(e, tc.PATH_CENTRE, (0.0, 1.0, 0.0), 1.0, W, H).cam14(), np.float32) for e in tc.PATH_EYES][:N_FRAMES]


@pytest.fixture(scope="module")
def reference(vrt, po, hall):
    """the restatement's frames of a (configuration, window, motion, dn) sequence, computed once: frame k has seed + k and sees the blob at
    k steps; its snapshot is the scene of frame k - 1.  What does not depend on motion and dn is shared."""
    cache, inputs = {}, {}
    seq, cams = mc.sequence(hall)[:N_FRAMES], _cameras(vrt)

    def get(cfg, win=(0, H), motion=0, dn=dc.PATH_DN, n=N_FRAMES):
        key = (cfg, win, motion, dn)
        if key not in cache or len(cache[key]) < n:
            spp, bounces, shadow, seed = cfg
            hist = vr.History()
            frames = []
            for k in range(n):
                if (cfg, win, k) not in inputs:
                    inputs[(cfg, win, k)] = vr.path_inputs(seq[k][0], cams[k], W, H, po.shade_params(), spp, bounces, seed + k, shadow, win[0], win[1])
                frames.append(vr.path_frame(seq[k][0], seq[k][1], cams[k], W, H, po.shade_params(), spp, bounces, seed + k, shadow, dn, tc.PATH_TP,
                                            vc.PATH_VP, hist, motion, win[0], win[1], inputs[(cfg, win, k)]))
            cache[key] = frames
        return cache[key]
    return get


def _outputs(dev):
    import torch
    o = {"px": torch.full((H, W), MARK, dtype=torch.int32, device=dev), "col": torch.full((H, W, 3), FMARK, dtype=torch.float32, device=dev),
         "cnt": torch.zeros(1, dtype=torch.int64, device=dev), "hist": _marked(dev, H * W * 4), "mom": _marked(dev, H * W * 2),
         "prev": torch.full((H, W, 4), FMARK, dtype=torch.float32, device=dev), "var": torch.full((H, W), FMARK, dtype=torch.float32, device=dev)}
    for k, c in AOV:
        o[k] = torch.full((H, W, c), FMARK, dtype=torch.float32, device=dev)
    return o


def _move(ds, k):
    """what precedes frame k: the scene as it is becomes the previous frame, then the blob takes its k-th place"""
    ds.snapshot_motion(INST)
    if k:
        ds.set_transforms([mc.translation(k)], mc.BLOB)


def _frame(vrt, ds, hist, cam, cfg, k, win=(0, H), motion=0, dn=dc.PATH_DN, stream=None, out=None, variance=True):
    """frame k of a sequence (seed + k) on a history of either kind: vxrt_render_path_variance on one with moments, else
    vxrt_render_path_temporal[_motion].  Returns the device outputs, the history read behind the frame on the same stream"""
    spp, bounces, shadow, seed = cfg
    o = out or _outputs(ds.device)
    s = _stream() if stream is None else stream
    a = (ds.accel, cam, W, H, win[0], win[1], vrt.rtapi.default_shade_params(), spp, bounces, vrt.rtapi.DenoiseParams(*dn), vrt.rtapi.TemporalParams(*tc.PATH_TP))
    aov = vrt.rtapi.PathAov(*[o[n].data_ptr() for n, _ in AOV])
    if hist.moments:
        vrt.rtapi.render_path_variance(*a, vrt.rtapi.VarianceParams(*vc.PATH_VP), hist, o["px"].data_ptr(), motion, seed + k, shadow, o["col"].data_ptr(), aov,
                                       o["prev"].data_ptr() if motion else None, o["var"].data_ptr() if variance else None, o["cnt"].data_ptr(), s)
        hist.read_moments(o["mom"].data_ptr(), s)
    elif motion:
        vrt.rtapi.render_path_temporal_motion(*a, hist, o["px"].data_ptr(), seed + k, shadow, o["col"].data_ptr(), aov, o["prev"].data_ptr(), o["cnt"].data_ptr(), s)
    else:
        vrt.rtapi.render_path_temporal(*a, hist, o["px"].data_ptr(), seed + k, shadow, o["col"].data_ptr(), aov, o["cnt"].data_ptr(), s)
    hist.read(o["hist"].data_ptr(), s)
    return o


def _host(o):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "px" else int(v.item()) if k == "cnt" else v.cpu().numpy()) for k, v in o.items()}


def _check(got, want, what, win=(0, H), motion=0, variance=True):
    y0, y1 = win
    rows = y1 - y0
    _same_floats(got["col"][y0:y1], want["col"], what + ": colours")
    np.testing.assert_array_equal(got["px"][y0:y1], want["px"], err_msg=what + ": pixels")
    assert got["cnt"] == want["rays"], "%s: rays traced %d, restatement %d" % (what, got["cnt"], want["rays"])
    outside = np.ones(H, bool)
    outside[y0:y1] = False
    assert (got["px"][outside] == MARK).all() and (got["col"][outside] == f32(FMARK)).all(), what + ": rows outside the window"
    for k, _ in AOV:
        _same_floats(got[k][y0:y1], want[k], what + ": " + k)
        assert (got[k][outside] == f32(FMARK)).all(), what + ": " + k + " outside the window"
    if motion:
        _same_floats(got["prev"][y0:y1], want["prev_position"], what + ": prev_position")
        assert (got["prev"][outside] == f32(FMARK)).all(), what
    else:
        assert (got["prev"] == f32(FMARK)).all(), what
    if variance:
        _same_floats(got["var"][y0:y1], want["variance"], what + ": variance")
        assert (got["var"][outside] == f32(FMARK)).all(), what
    else:
        assert (got["var"] == f32(FMARK)).all(), what
    _same_floats(got["hist"][:rows * W * 4].reshape(rows, W, 4), want["T"], what + ": the history")
    _same_floats(got["mom"][:rows * W * 2].reshape(rows, W, 2), want["M"], what + ": the moments")
    assert (got["hist"][rows * W * 4:] == f32(FMARK)).all() and (got["mom"][rows * W * 2:] == f32(FMARK)).all(), what + ": read past the window"


@pytest.mark.parametrize("motion", (0, 1))
@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("cfg", dc.PATH_CONFIGS)
def test_frames_against_the_restatement(vrt, gpu_device, hall, reference, cfg, win, motion):
    """four frames, the camera on its orbit, dolly and cut, the blob moving: pixels, colours, rays traced, every aov, V0, the history"""
    want = reference(cfg, win, motion)
    assert any((w["T"][..., 3] > 1).any() for w in want[1:3])
    ds = vrt.tracer.DeviceScene(hall, gpu_device)
    try:
        with vrt.rtapi.History(W, win[1] - win[0], moments=True) as hist:
            for k, cam in enumerate(_cameras(vrt)):
                _move(ds, k)
                got = _host(_frame(vrt, ds, hist, cam, cfg, k, win, motion))
                _check(got, want[k], "%r rows %r motion %d frame %d" % (cfg, win, motion, k), win, motion)
    finally:
        ds.close()
    # (not vacuous: some frame has pixels on the temporal route, with a variance that is not zero, and pixels on the spatial one)
    hitl = [(w["position"][..., 3] != 0, w["T"][..., 3]) for w in want]
    assert any(((l >= vc.PATH_VP[1]) & hit & (w["variance"] > 0)).sum() > 50 for (hit, l), w in zip(hitl, want))
    assert all(((l < vc.PATH_VP[1]) & hit & (w["variance"] > 0)).sum() > 50 for (hit, l), w in zip(hitl, want))


@pytest.mark.parametrize("motion", (0, 1))
def test_no_iterations_is_the_temporal_frame(vrt, gpu_device, hall, reference, motion):
    """dn->iterations = 0: vxrt_render_path_temporal[_motion] bit for bit -- pixels, colours, rays traced, HE -- with the variance output
    (still V0) and without it"""
    cfg, dn = dc.PATH_CONFIGS[0], (0,) + dc.PATH_DN[1:]
    want = reference(cfg, (0, H), motion, dn, 3)
    ds = vrt.tracer.DeviceScene(hall, gpu_device)
    try:
        with vrt.rtapi.History(W, H, moments=True) as hist, vrt.rtapi.History(W, H) as plain:
            for k, cam in enumerate(_cameras(vrt)[:3]):
                _move(ds, k)
                got = _host(_frame(vrt, ds, hist, cam, cfg, k, motion=motion, dn=dn, variance=(k != 1)))
                _check(got, want[k], "no iterations, motion %d frame %d" % (motion, k), motion=motion, variance=(k != 1))
                other = _host(_frame(vrt, ds, plain, cam, cfg, k, motion=motion, dn=dn))
                for key in ("px", "col", "hist", "prev") + tuple(n for n, _ in AOV):
                    np.testing.assert_array_equal(np.asarray(got[key]).view(np.uint32), np.asarray(other[key]).view(np.uint32), err_msg=key)
                assert got["cnt"] == other["cnt"]
            assert (got["hist"][:H * W * 4].reshape(H, W, 4)[..., 3] > 1).any()
    finally:
        ds.close()


def test_a_reset_history_is_a_fresh_one(vrt, gpu_device, hall, reference):
    cfg = dc.PATH_CONFIGS[0]
    cams = _cameras(vrt)
    ds = vrt.tracer.DeviceScene(hall, gpu_device)
    try:
        _move(ds, 0)
        with vrt.rtapi.History(W, H, moments=True) as hist, vrt.rtapi.History(W, H, moments=True) as fresh:
            first = _host(_frame(vrt, ds, hist, cams[0], cfg, 0))
            _check(first, reference(cfg)[0], "frame 0")
            second = _host(_frame(vrt, ds, hist, cams[1], cfg, 1))
            assert (second["hist"][:H * W * 4].reshape(H, W, 4)[..., 3] > 1).any()
            hist.reset()
            a, b = _host(_frame(vrt, ds, hist, cams[2], cfg, 2)), _host(_frame(vrt, ds, fresh, cams[2], cfg, 2))
            assert a["cnt"] == b["cnt"]
            for key in a:
                if key != "cnt":
                    np.testing.assert_array_equal(np.asarray(a[key]).view(np.uint32), np.asarray(b[key]).view(np.uint32), err_msg=key)
            assert (a["hist"][:H * W * 4].reshape(H, W, 4)[..., 3] <= 1).all()
    finally:
        ds.close()


def test_frame_refusals(vrt, gpu_device, hall, reference):
    import torch
    L = vrt.rtapi._variance_lib()
    cfg = dc.PATH_CONFIGS[0]
    want = reference(cfg)
    cams = _cameras(vrt)
    PP, DP, TP, VP = vrt.rtapi.PathParams, vrt.rtapi.DenoiseParams, vrt.rtapi.TemporalParams, vrt.rtapi.VarianceParams
    nan, inf = float("nan"), float("inf")
    px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
    prev = torch.full((H, W, 4), FMARK, dtype=torch.float32, device=gpu_device)
    ds = vrt.tracer.DeviceScene(hall, gpu_device)
    try:
        with vrt.rtapi.History(W, H, moments=True) as hist, vrt.rtapi.History(W, H // 2, moments=True) as small, vrt.rtapi.History(W, H) as plain:
            assert vrt.rtapi.accel_info(ds.accel, 6) == 0
            p, q, d, t, v = vrt.rtapi.default_shade_params(), PP(cfg[0], cfg[1], cfg[3] + 1, cfg[2]), DP(*dc.PATH_DN), TP(*tc.PATH_TP), VP(*vc.PATH_VP)
            good = vrt.rtapi.Camera.from_cam14(cams[1])

            def call(accel=ds.accel, cam=good, y0=0, y1=H, params=p, path=q, dn=d, tp=t, vp=v, hh=hist.handle, motion=0, dst=px.data_ptr(), pp=None):
                ref = [None if x is None else C.byref(x) for x in (cam, params, path, dn, tp, vp)]
                return L.vxrt_render_path_variance(accel, ref[0], W, H, y0, y1, ref[1], ref[2], ref[3], ref[4], ref[5], hh, motion, dst, None, None, pp, None,
                                                   None, _stream())
            assert call(motion=1) == -1 and call(motion=1, pp=prev.data_ptr()) == -1      # no snapshot
            _move(ds, 0)
            _check(_host(_frame(vrt, ds, hist, cams[0], cfg, 0)), want[0], "frame 0")
            _frame(vrt, ds, plain, cams[0], cfg, 0)
            for kw in ({"cam": None}, {"accel": None}, {"params": None}, {"path": None}, {"dn": None}, {"tp": None}, {"vp": None}, {"hh": None}, {"dst": None}):
                assert call(**kw) == -1, kw
            c = cams[1].copy()
            c[7] = nan
            assert call(cam=vrt.rtapi.Camera.from_cam14(c)) == -1
            for bad in (VP(0.0, 3, 2, 0), VP(nan, 3, 2, 0), VP(inf, 3, 2, 0), VP(1e-3, 0, 2, 0), VP(1e-3, vrt.rtapi.TEMPORAL_MAX_LEN + 1, 2, 0), VP(1e-3, 3, 0, 0),
                        VP(1e-3, 3, 4, 0), VP(1e-3, 3, 2, 7)):
                assert call(vp=bad) == -1
            assert call(motion=2) == -1 and call(motion=-1) == -1 and call(motion=0, pp=prev.data_ptr()) == -1
            assert call(hh=plain.handle) == -1 and call(hh=plain.handle, motion=1) == -1  # a history without moments
            for bad in (TP(0.0, 3, 2.0, 0.9), TP(0.2, 0, 2.0, 0.9), TP(0.2, 3, nan, 0.9)):
                assert call(tp=bad) == -1
            for bad in (DP(7, 5, 2.0, 0.25), DP(3, 8, 2.0, 0.25), DP(3, 5, 0.0, 0.25), DP(3, 5, 2.0, nan)):
                assert call(dn=bad) == -1
            for bad in (PP(0, 3, 0, 1), PP(4097, 3, 0, 1), PP(2, vrt.rtapi.PATH_MAX_BOUNCES + 1, 0, 1), PP(2, 3, 0, 2)):
                assert call(path=bad) == -1
            assert call(y0=5, y1=3) == -1 and call(y1=H + 1) == -1
            assert call(hh=small.handle) == -1                                            # a window larger than the capacity
            assert call(y0=7, y1=7) == 0                                                  # the empty window
            # the existing frames refuse a history with moments
            T = vrt.rtapi._motion_lib()
            b = [C.byref(x) for x in (good, p, q, d, t)]
            assert T.vxrt_render_path_temporal(ds.accel, b[0], W, H, 0, H, b[1], b[2], b[3], b[4], hist.handle, px.data_ptr(), None, None, None, _stream()) == -1
            assert T.vxrt_render_path_temporal_motion(ds.accel, b[0], W, H, 0, H, b[1], b[2], b[3], b[4], hist.handle, px.data_ptr(), None, None, None, None,
                                                      _stream()) == -1
            torch.cuda.synchronize()
            assert (px.cpu().numpy() == MARK).all() and (prev.cpu().numpy() == f32(FMARK)).all()
            assert L.vxrt_history_read(small.handle, px.data_ptr(), _stream()) == -1      # still empty
            _move(ds, 1)
            _check(_host(_frame(vrt, ds, hist, cams[1], cfg, 1)), want[1], "frame 1 after the refusals")
    finally:
        ds.close()


def test_two_moment_histories_on_two_streams(vrt, gpu_device, hall, reference):
    """two sequences interleaved on two streams, two frames in flight, a history each: every frame is the one its sequence gives alone"""
    import torch
    cams = _cameras(vrt)
    want = [reference(cfg) for cfg in dc.PATH_CONFIGS]
    ds = vrt.tracer.DeviceScene(hall, gpu_device)
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=ds.device) for _ in range(2)]
        with vrt.rtapi.History(W, H, moments=True) as h0, vrt.rtapi.History(W, H, moments=True) as h1:
            outs = [[_outputs(ds.device) for _ in range(N_FRAMES)] for _ in range(2)]
            torch.cuda.synchronize()
            for k in range(N_FRAMES):
                torch.cuda.synchronize()          # (the scene moves between frames: a move is ordered behind every frame in flight)
                _move(ds, k)
                for i, hist in enumerate((h0, h1)):
                    _frame(vrt, ds, hist, cams[k], dc.PATH_CONFIGS[i], k, stream=streams[i].cuda_stream, out=outs[i][k])
            torch.cuda.synchronize()
            for i in range(2):
                for k in range(N_FRAMES):
                    _check(_host(outs[i][k]), want[i][k], "stream %d frame %d" % (i, k))
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)
        ds.close()
