"""GPU: motion-aware temporal accumulation -- the snapshot (vxrt_accel_motion_snapshot), the previous-position guide
(vxrt_previous_positions), the step with motion (vxrt_temporal_accumulate_motion) and the frame (vxrt_render_path_temporal_motion) --
against the restatement tests/motion_ref.py, bit for bit: f32 as u32, pixels, rays traced, the history after every frame.  No masks, no
tolerances, with the one exception of tests/test_gpu_temporal.py: where the restatement gives a NaN the kernel must give a NaN of any
payload.  tests/test_motion_cpu.py holds the restatement to the definition's identities and measures what the feature is for."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import motion_cases as mc
import motion_ref as mr
import temporal_cases as tc
import temporal_ref as tr

pytestmark = pytest.mark.gpu
W, H = mc.W, mc.H
MARK = 0x5A5A5A
FMARK = -12345.5   # marker of float outputs
GUARD = 64         # floats past the end of an output
KEYS = ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")
WINDOWS = ((0, H), (8, 40))
INST, GEOM = mr.INSTANCES, mr.GEOMETRY
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


def _marked(dev, n_floats):
    import torch
    return torch.full((n_floats + GUARD,), FMARK, dtype=torch.float32, device=dev)


def _rot(axis, deg, scale=1.0, t=(0.0, 0.0, 0.0)):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(4)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    m[:3, :3] *= scale
    m[:3, 3] = t
    return m.astype(np.float32)


# ---- the guide ----
def _trace(vrt, ds, rays):
    import torch
    from oracle.pyoracle import HIT_DTYPE
    r = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(ds.device)
    out = torch.zeros(len(rays) * 24, dtype=torch.uint8, device=ds.device)
    vrt.rtapi.trace(ds.accel, r.data_ptr(), len(rays), out.data_ptr(), 0, None, _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(HIT_DTYPE).copy()


def _guide(vrt, ds, hits, n=None, rc=False):
    """vxrt_previous_positions on the first n of `hits`: Q4, N4 (n, 4) -- nothing may be written behind them"""
    import torch
    n = len(hits) if n is None else n
    t = torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).reshape(-1).copy()).to(ds.device)
    q, nn = _marked(ds.device, 4 * n), _marked(ds.device, 4 * n)
    L = vrt.rtapi._motion_lib()
    r = L.vxrt_previous_positions(ds.accel, n, t.data_ptr(), q.data_ptr(), nn.data_ptr(), _stream())
    torch.cuda.synchronize()
    q, nn = q.cpu().numpy(), nn.cpu().numpy()
    assert (q[4 * n:] == f32(FMARK)).all() and (nn[4 * n:] == f32(FMARK)).all(), "written past record %d" % n
    if rc:
        return r, q[:4 * n], nn[:4 * n]
    assert r == 0
    return q[:4 * n].reshape(n, 4), nn[:4 * n].reshape(n, 4)


def _rays(g, seed=5):
    """the fixture's rays and a jittered copy: about 4,096 records"""
    rng = np.random.RandomState(seed)
    r = np.array(g["rays"], np.float32)
    j = r.copy()
    j[:, 3:6] += rng.normal(0.0, 0.02, (len(r), 3)).astype(np.float32)
    return np.concatenate([r, j])


def _hostile(hits, n_blas, n_tris, seed=9):
    """records that are no traversal's: misses with wild indices, the occlusion bit, barycentrics that are not finite or negative, and
    indices past the scene's"""
    rng = np.random.RandomState(seed)
    found = hits[hits["dist"] != f32(1e30)]
    h = found[rng.randint(0, len(found), 96)].copy()
    h["dist"][0:8] = 1e30
    h["blasIdx"][0:4], h["triIdx"][4:8] = 0xFFFFFFFF, 0xFFFFFFFF          # (misses: nothing may be read for them)
    h["blasIdx"][8:24] |= 0x80000000
    nan, inf = np.nan, np.inf
    for k, v in enumerate((nan, inf, -inf, -0.75, 3.5, 0.0, -0.0, 1e30)):
        h[("bx", "by", "bz")[k % 3]][24 + 2 * k: 26 + 2 * k] = v
    h["bx"][40:44], h["by"][40:44], h["bz"][40:44] = nan, nan, nan
    h["dist"][44:48] = (nan, inf, -1.0, 0.0)                               # (not misses: only 1e30 is)
    h["blasIdx"][48:56] = (n_blas, n_blas + 1, 0x7FFFFFFF, 0x80000000 | n_blas, 0xFFFFFFFF, 1 << 30, 0x80000000 | 0x7FFFFFFF, n_blas + 1000)
    h["triIdx"][56:64] = (n_tris, n_tris + 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 1 << 30, n_tris * 2, n_tris + 255)
    h["blasIdx"][64:68], h["triIdx"][64:68] = n_blas, n_tris
    return h


def test_guide_against_the_restatement(vrt, golden, gpu_device):
    g = golden("teapot_x3")
    b0 = {k: g[k] for k in KEYS}
    ds = vrt.tracer.DeviceScene(b0, gpu_device)
    try:
        first = [_rot(1, 25.0, 1.1, (1.2, 0.1, -0.2)), _rot(0, -40.0, 0.9, (-0.7, 0.0, 1.1))]      # the snapshot's matrices: no identities
        ds.set_transforms(first, 0)
        b1 = mr.moved(b0, 0, np.stack(first))
        ds.snapshot_motion(INST)
        snap = mr.snapshot(b1)
        then = [_rot(2, 15.0, 0.9, (-0.6, 0.3, 1.0)), _rot(1, 70.0, 1.0, (-0.7, -0.2, -1.2))]      # two instances move on
        ds.set_transforms(then, 1)
        b2 = mr.moved(b1, 1, np.stack(then))
        n_blas, n_tris = b0["blas"].size // 160, b0["tri"].size // 36
        hits = _trace(vrt, ds, _rays(g))
        found = hits["dist"] != f32(1e30)
        assert len(hits) > 4000 and all((found & (hits["blasIdx"] == i)).sum() > 100 for i in range(n_blas)) and (~found).sum() > 100
        hits = np.concatenate([hits, _hostile(hits, n_blas, n_tris)])
        wq, wn = mr.previous_positions(b2, snap, hits)
        bad = (hits["dist"] == f32(1e30)) | ((hits["blasIdx"] & 0x7FFFFFFF) >= n_blas) | (hits["triIdx"] >= n_tris)
        assert (wq[bad] == 0).all() and (wn[bad] == 0).all() and bad[-96:].sum() >= 28 and np.isnan(wq[-96:]).any()
        # (the instances did move: the guide is not where the same records are now)
        cq = mr.previous_positions(b2, mr.snapshot(b2), hits)[0]
        went = ~bad & ((hits["blasIdx"] & 0x7FFFFFFF) != 0)                 # (instances 1 and 2)
        with np.errstate(invalid="ignore"):
            assert (np.abs(wq[went] - cq[went]).max(1) > 0.05).mean() > 0.9
        for n in (1, 255, 256, 257, len(hits)):
            q, nn = _guide(vrt, ds, hits, n)
            _same_floats(q, wq[:n], "Q of the first %d records" % n)
            _same_floats(nn, wn[:n], "N' of the first %d records" % n)
        # the hostile records alone, in front: whatever block they fall into
        order = np.concatenate([np.arange(len(hits) - 96, len(hits)), np.arange(300)])
        q, nn = _guide(vrt, ds, hits[order])
        _same_floats(q, wq[order], "hostile records first: Q")
        _same_floats(nn, wn[order], "hostile records first: N'")
    finally:
        ds.close()


def _put_tri(ds, tri_u8):
    import torch
    ds.t["tri"].copy_(torch.from_numpy(np.ascontiguousarray(tri_u8)).to(ds.t["tri"].device))


def test_snapshot_semantics(vrt, golden, gpu_device):
    import torch
    g = golden("sphere_x6")
    b0 = {k: np.array(g[k]) for k in KEYS}
    ds = vrt.tracer.DeviceScene(b0, gpu_device)
    L = vrt.rtapi._motion_lib()
    info, nbytes = (lambda: vrt.rtapi.accel_info(ds.accel, 6)), (lambda: vrt.rtapi.accel_bytes(ds.accel))
    n_blas, n_tris = b0["blas"].size // 160, b0["tri"].size // 36
    try:
        base = nbytes()
        assert info() == 0
        rays = _rays(g)
        hits = _trace(vrt, ds, rays)
        # no snapshot: refused, outputs untouched
        rc, q, nn = _guide(vrt, ds, hits, rc=True)
        assert rc == -1 and (q == f32(FMARK)).all() and (nn == f32(FMARK)).all()
        # the refusals of the snapshot call: nothing changes
        for what in (GEOM, 4, 5, 8 | INST, 0x80000000):
            assert L.vxrt_accel_motion_snapshot(ds.accel, what, _stream()) == -1
        assert L.vxrt_accel_motion_snapshot(None, INST, _stream()) == -1
        assert info() == 0 and nbytes() == base
        assert L.vxrt_accel_motion_snapshot(ds.accel, 0, _stream()) == 0 and info() == 0          # (nothing to free)
        # INSTANCES: two set_transforms after one snapshot still see the snapshot's matrices
        ds.snapshot_motion(INST)
        assert info() == INST and nbytes() == base + n_blas * 160
        snap = mr.snapshot(b0)
        b1 = mr.moved(b0, 1, _rot(1, 30.0, 1.0, (0.7, 0.2, 1.0))[None])
        ds.set_transforms([_rot(1, 30.0, 1.0, (0.7, 0.2, 1.0))], 1)
        b2 = mr.moved(b1, 4, np.stack([_rot(0, 20.0, 1.2, (-0.6, 0.1, -1.2)), _rot(2, -35.0, 0.8, (0.6, -0.1, -1.1))]))
        ds.set_transforms([_rot(0, 20.0, 1.2, (-0.6, 0.1, -1.2)), _rot(2, -35.0, 0.8, (0.6, -0.1, -1.1))], 4)
        hits = _trace(vrt, ds, rays)
        wq, wn = mr.previous_positions(b2, snap, hits)
        q, nn = _guide(vrt, ds, hits)
        _same_floats(q, wq, "two moves after one snapshot: Q")
        _same_floats(nn, wn, "two moves after one snapshot: N'")
        assert (_bits(wq) != _bits(mr.previous_positions(b2, mr.snapshot(b1), hits)[0])).any()    # (not the matrices in between)
        # a later snapshot replaces the earlier one
        ds.snapshot_motion(INST)
        assert info() == INST and nbytes() == base + n_blas * 160
        q, _ = _guide(vrt, ds, hits)
        _same_floats(q, mr.previous_positions(b2, mr.snapshot(b2), hits)[0], "the second snapshot")
        # GEOMETRY: old vertices after a vertex refit; a snapshot without it follows the current ones
        ds.snapshot_motion(INST | GEOM)
        assert info() == (INST | GEOM) and nbytes() == base + n_blas * 160 + n_tris * 36
        snap = mr.snapshot(b2, INST | GEOM)
        b3 = dict(b2)
        v = np.array(b2["tri"]).view(np.float32).reshape(-1, 3, 3).copy()
        v += (0.03 * np.sin(7.0 * v[..., ::-1])).astype(np.float32)
        b3["tri"] = v.view(np.uint8).reshape(-1)
        _put_tri(ds, b3["tri"])
        ds.refit(geometry=True)
        hits = _trace(vrt, ds, rays)
        old = mr.previous_positions(b3, snap, hits)
        q, nn = _guide(vrt, ds, hits)
        _same_floats(q, old[0], "a geometry snapshot keeps the old vertices: Q")
        _same_floats(nn, old[1], "a geometry snapshot keeps the old vertices: N'")
        ds.snapshot_motion(INST)
        assert info() == INST and nbytes() == base + n_blas * 160
        cur = mr.previous_positions(b3, mr.snapshot(b3, INST), hits)
        assert (_bits(cur[0]) != _bits(old[0])).any()
        q, nn = _guide(vrt, ds, hits)
        _same_floats(q, cur[0], "an instance snapshot reads the current vertices: Q")
        _same_floats(nn, cur[1], "an instance snapshot reads the current vertices: N'")
        # the refusals of the guide call, with a snapshot held
        t = torch.from_numpy(hits.view(np.uint8).reshape(-1).copy()).to(gpu_device)
        o = _marked(gpu_device, 8 * len(hits))
        a, p, s = ds.accel, o.data_ptr(), _stream()
        half = p + 16 * len(hits)
        assert L.vxrt_previous_positions(None, 4, t.data_ptr(), p, half, s) == -1
        assert L.vxrt_previous_positions(a, 4, None, p, half, s) == -1
        assert L.vxrt_previous_positions(a, 4, t.data_ptr(), None, half, s) == -1 and L.vxrt_previous_positions(a, 4, t.data_ptr(), p, None, s) == -1
        assert L.vxrt_previous_positions(a, 4, t.data_ptr(), p + 4, half, s) == -1 and L.vxrt_previous_positions(a, 4, t.data_ptr(), p, half + 8, s) == -1
        assert L.vxrt_previous_positions(a, 0, t.data_ptr(), p, half, s) == 0
        # what = 0 drops the snapshot
        ds.snapshot_motion(0)
        assert info() == 0 and nbytes() == base
        assert L.vxrt_previous_positions(a, 4, t.data_ptr(), p, half, s) == -1
        torch.cuda.synchronize()
        assert (o.cpu().numpy() == f32(FMARK)).all()
    finally:
        ds.close()


# ---- the step ----
def _perturbed(P, N, seed):
    """guides of a previous frame that is not this one: Q = P shifted and jittered with a flag of its own, N' = N jittered; at seeded
    places no previous position (w = 0, -0, NaN and 2.5 count by `!= 0`), coordinates that are not finite, zero and NaN normals"""
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
        m = i % 12
        if m < 5:
            qf[p, 3] = (0.0, -0.0, np.nan, 2.5, 0.0)[m]
        elif m < 9:
            qf[p, (m - 5) % 3] = (np.inf, np.nan, -np.inf, 1e30)[m - 5]
        elif m == 9:
            nf[p, :3] = 0.0
        elif m == 10:
            nf[p, 1] = np.nan
        else:
            nf[p, :3] *= 40.0
    return Q, Nq


def _accumulate(vrt, dev, hist, cam, w, h, win, E, P, N, prm, Q=None, Nq=None):
    """vxrt_temporal_accumulate_motion (or, without Q, vxrt_temporal_accumulate) on device copies: out and the history read back"""
    import torch
    rows = win[1] - win[0]
    t = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (E, P, N) + (() if Q is None else (Q, Nq))]
    out, rd = _marked(dev, rows * w * 4), _marked(dev, rows * w * 4)
    tp = vrt.rtapi.TemporalParams(*prm)
    if Q is None:
        vrt.rtapi.temporal_accumulate(hist, cam, w, h, win[0], win[1], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), tp, out.data_ptr(), _stream())
    else:
        vrt.rtapi.temporal_accumulate_motion(hist, cam, w, h, win[0], win[1], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                             t[4].data_ptr(), tp, out.data_ptr(), _stream())
    hist.read(rd.data_ptr(), _stream())
    torch.cuda.synchronize()
    o, r = out.cpu().numpy(), rd.cpu().numpy()
    n4 = rows * w * 4
    assert (o[n4:] == f32(FMARK)).all() and (r[n4:] == f32(FMARK)).all(), "written past the end of out4"
    return o[:n4].reshape(rows, w, 4), r[:n4].reshape(rows, w, 4)


@pytest.mark.parametrize("w,h,name", tc.all_sequences())
def test_step_against_the_restatement(vrt, gpu_device, w, h, name):
    fr, win, prm = tc.frames(w, h, name)
    ref = tr.History()
    blended = 0
    with vrt.rtapi.History(w, win[1] - win[0]) as hist:
        for k, (cam, E, P, N, _, _) in enumerate(fr):
            Q, Nq = _perturbed(P, N, 100 + k)
            want = mr.step(E, P, N, Q, Nq, ref, cam, w, h, win[0], win[1], prm)
            got, read = _accumulate(vrt, gpu_device, hist, cam, w, h, win, E, P, N, prm, Q, Nq)
            what = "%dx%d %s frame %d" % (w, h, name, k)
            _same_floats(got, want, what)
            _same_floats(read, want, what + ": vxrt_history_read")
            blended += int((want[..., 3] > 1).sum())
            nop = (P[..., 3] != 0) & ~(Q[..., 3] != 0)
            assert (want[..., 3][nop] == 1).all()
    assert blended > 0 or (w, h) not in tc.BIG


@pytest.mark.parametrize("w,h,name", tc.all_sequences())
def test_step_with_the_frames_own_guides_is_the_camera_step(vrt, gpu_device, w, h, name):
    """Q = P, N' = N: vxrt_temporal_accumulate_motion is vxrt_temporal_accumulate, payloads of NaNs included"""
    fr, win, prm = tc.frames(w, h, name)
    with vrt.rtapi.History(w, win[1] - win[0]) as ha, vrt.rtapi.History(w, win[1] - win[0]) as hb:
        for k, (cam, E, P, N, _, _) in enumerate(fr):
            a = _accumulate(vrt, gpu_device, ha, cam, w, h, win, E, P, N, prm)
            b = _accumulate(vrt, gpu_device, hb, cam, w, h, win, E, P, N, prm, P, N)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(_bits(x), _bits(y), err_msg="%dx%d %s frame %d" % (w, h, name, k))


def test_step_refusals(vrt, gpu_device):
    import torch
    L = vrt.rtapi._motion_lib()
    w, h = 45, 37
    fr, win, prm = tc.frames(w, h, "pan")
    cam, E, P, N = fr[0][:4]
    t = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu_device) for a in (E, P, N, P, N)]
    out = _marked(gpu_device, w * h * 4)
    good_cam, good = vrt.rtapi.Camera.from_cam14(cam), vrt.rtapi.TemporalParams(*prm)
    with vrt.rtapi.History(w, h) as hist:
        def call(hh=hist.handle, c=good_cam, ww=w, fh=h, y0=0, y1=h, off=(0, 0, 0, 0, 0), p=good, null=()):
            a = [None if i in null else t[i].data_ptr() + off[i] for i in range(5)]
            return L.vxrt_temporal_accumulate_motion(hh, None if c is None else C.byref(c), ww, fh, y0, y1, a[0], a[1], a[2], a[3], a[4],
                                                     None if p is None else C.byref(p), None if 5 in null else out.data_ptr(), _stream())
        assert call(hh=None) == -1 and call(c=None) == -1 and call(p=None) == -1
        for i in range(6):
            assert call(null=(i,)) == -1
        for i in range(1, 5):
            off = [0] * 5
            off[i] = 4 + 4 * (i % 2)
            assert call(off=tuple(off)) == -1                                           # not 16-byte aligned
        bad = np.array(cam, np.float32)
        bad[5] = np.nan
        assert call(c=vrt.rtapi.Camera.from_cam14(bad)) == -1
        assert call(ww=65536, fh=32768, y1=32768) == -1 and call(fh=h + 1, y1=h + 1) == -1
        assert call(ww=0) == -1 and call(fh=0, y1=0) == -1 and call(y0=5, y1=3) == -1 and call(y1=h + 1) == -1
        assert call(p=vrt.rtapi.TemporalParams(0.0, 32, 0.5, 0.9)) == -1 and call(p=vrt.rtapi.TemporalParams(0.1, 32, 0.5, np.nan)) == -1
        assert call(y0=7, y1=7) == 0                                                    # the empty window
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == f32(FMARK)).all()
        assert L.vxrt_history_read(hist.handle, out.data_ptr(), _stream()) == -1        # still empty
        assert call() == 0


# ---- the frame ----
@pytest.fixture(scope="module")
def hall(vrt):
    return mc.hall(vrt)


@pytest.fixture(scope="module")
def reference(vrt, po, hall):
    """the restatement's six frames of a (configuration, window), computed once: frame k has seed + k"""
    cache = {}
    seq, cams = mc.sequence(hall), mc.cameras()

    def get(cfg, win=(0, H)):
        if (cfg, win) not in cache:
            spp, bounces, shadow, seed = cfg
            hist = tr.History()
            cache[(cfg, win)] = [mr.path_frame(seq[k][0], seq[k][1], cams[k], W, H, po.shade_params(), spp, bounces, seed + k, shadow, dc.PATH_DN, mc.TP,
                                               hist, win[0], win[1]) for k in range(mc.N_FRAMES)]
        return cache[(cfg, win)]
    return get


def _outputs(dev):
    import torch
    return {"px": torch.full((H, W), MARK, dtype=torch.int32, device=dev), "col": torch.full((H, W, 3), FMARK, dtype=torch.float32, device=dev),
            "prev": torch.full((H, W, 4), FMARK, dtype=torch.float32, device=dev), "cnt": torch.zeros(1, dtype=torch.int64, device=dev),
            "hist": torch.full((H * W * 4,), FMARK, dtype=torch.float32, device=dev)}


def _frame(vrt, ds, hist, cam, cfg, k, win=(0, H), motion=True):
    spp, bounces, shadow, seed = cfg
    o = _outputs(ds.device)
    a = (ds.accel, cam, W, H, win[0], win[1], vrt.rtapi.default_shade_params(), spp, bounces, vrt.rtapi.DenoiseParams(*dc.PATH_DN),
         vrt.rtapi.TemporalParams(*mc.TP), hist, o["px"].data_ptr(), seed + k, shadow, o["col"].data_ptr(), None)
    if motion:
        vrt.rtapi.render_path_temporal_motion(*a, o["prev"].data_ptr(), o["cnt"].data_ptr(), _stream())
    else:
        vrt.rtapi.render_path_temporal(*a, o["cnt"].data_ptr(), _stream())
    hist.read(o["hist"].data_ptr(), _stream())
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "px" else int(v.item()) if k == "cnt" else v.cpu().numpy()) for k, v in o.items()}


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("cfg", dc.PATH_CONFIGS)
def test_frames_against_the_restatement(vrt, gpu_device, hall, reference, cfg, win):
    """six frames, the blob moving 1.5 pixels per frame while the camera yaws: pixels, colours, the guide output and the history"""
    want = reference(cfg, win)
    y0, y1 = win
    ds = vrt.tracer.DeviceScene(hall, gpu_device)
    try:
        cams = mc.cameras()
        outside = np.ones(H, bool)
        outside[y0:y1] = False
        with vrt.rtapi.History(W, y1 - y0) as hist:
            for k in range(mc.N_FRAMES):
                ds.snapshot_motion(INST)
                if k:
                    ds.set_transforms([mc.translation(k)], mc.BLOB)
                got = _frame(vrt, ds, hist, cams[k], cfg, k, win)
                what = "%r rows %r frame %d" % (cfg, win, k)
                np.testing.assert_array_equal(got["px"][y0:y1], want[k]["px"], err_msg=what + ": pixels")
                _same_floats(got["col"][y0:y1], want[k]["col"], what + ": colours")
                _same_floats(got["prev"][y0:y1], want[k]["prev_position"], what + ": prev_position")
                assert got["cnt"] == want[k]["rays"], what
                assert (got["px"][outside] == MARK).all() and (got["col"][outside] == f32(FMARK)).all() and (got["prev"][outside] == f32(FMARK)).all(), what
                n4 = (y1 - y0) * W * 4
                _same_floats(got["hist"][:n4].reshape(y1 - y0, W, 4), want[k]["T"], what + ": the history")
                assert (got["hist"][n4:] == f32(FMARK)).all(), what
        # (not vacuous: in the last frame most of the moved blob carries more than two frames of history)
        moved = (np.abs(want[-1]["prev_position"][..., :3] - want[-1]["position"][..., :3]).max(-1) > 1.0) & (want[-1]["position"][..., 3] != 0)
        assert moved.sum() >= 100 and (want[-1]["T"][..., 3][moved] > 2).mean() > 0.5
    finally:
        ds.close()


def test_frame_refusals(vrt, golden, gpu_device, hall):
    import torch
    import camera_secondary_ref as csr
    import shading_ref as sr
    L = vrt.rtapi._motion_lib()
    cfg = dc.PATH_CONFIGS[0]
    cam = mc.cameras()[0]

    def refused(ds, hist):
        px = torch.full((H, W), MARK, dtype=torch.int32, device=gpu_device)
        prev = torch.full((H, W, 4), FMARK, dtype=torch.float32, device=gpu_device)
        with pytest.raises(RuntimeError):
            vrt.rtapi.render_path_temporal_motion(ds.accel, cam, W, H, 0, H, vrt.rtapi.default_shade_params(), cfg[0], cfg[1], vrt.rtapi.DenoiseParams(*dc.PATH_DN),
                                                  vrt.rtapi.TemporalParams(*mc.TP), hist, px.data_ptr(), cfg[3], cfg[2], None, None, prev.data_ptr(), None, _stream())
        torch.cuda.synchronize()
        assert (px.cpu().numpy() == MARK).all() and (prev.cpu().numpy() == f32(FMARK)).all()
        with pytest.raises(RuntimeError):
            hist.read(px.data_ptr(), _stream())       # (the refused frame left the history empty)

    # no snapshot; then a stale accel, which the snapshot call refuses as well
    ds = vrt.tracer.DeviceScene(hall, gpu_device)
    try:
        with vrt.rtapi.History(W, H) as hist:
            refused(ds, hist)
            ds.snapshot_motion(INST)
            assert _frame(vrt, ds, hist, cam, cfg, 0)["cnt"] > 0
            ds.snapshot_motion(0)
            hist.reset()
            refused(ds, hist)
            ds.snapshot_motion(INST)
            v = ds.t["tri"].view(torch.float32).view(-1, 3, 3)
            v[0, 0, 0], v[1, 1, 0] = -3e38, 3e38   # the extent overflows fp32: the refit fails and leaves the accel stale
            with pytest.raises(Exception):
                ds.refit(geometry=True)
            refused(ds, hist)
            assert L.vxrt_accel_motion_snapshot(ds.accel, INST, _stream()) == -1 and vrt.rtapi.accel_info(ds.accel, 6) == INST
            t = torch.zeros(24 * 4, dtype=torch.uint8, device=gpu_device)
            o = _marked(gpu_device, 32)
            assert L.vxrt_previous_positions(ds.accel, 4, t.data_ptr(), o.data_ptr(), o.data_ptr() + 64, _stream()) == -1
    finally:
        ds.close()
    # a non-zero alpha table
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in csr.KEYS}, gpu_device)
    try:
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        ds.snapshot_motion(INST)
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1 and vrt.rtapi.accel_info(ds.accel, 6) == INST      # (the snapshot survives the table)
        cam = csr.golden_cameras(vrt)["g_orbit_1"]
        with vrt.rtapi.History(W, H) as hist:
            refused(ds, hist)
            ds.set_alpha_test(None)
            assert _frame(vrt, ds, hist, cam, cfg, 0)["cnt"] > 0
    finally:
        ds.close()


def test_the_camera_only_frame_is_not_disturbed(vrt, gpu_device, hall):
    """vxrt_render_path_temporal on one accel before a snapshot exists, while one is held and after a motion frame: identical bits"""
    cfg = dc.PATH_CONFIGS[0]
    cams = mc.cameras()
    ds = vrt.tracer.DeviceScene(hall, gpu_device)
    try:
        def two_frames():
            with vrt.rtapi.History(W, H) as hist:
                return [_frame(vrt, ds, hist, cams[k], cfg, k, motion=False) for k in range(2)]
        before = two_frames()
        ds.snapshot_motion(INST | GEOM)
        held = two_frames()
        with vrt.rtapi.History(W, H) as hist:
            _frame(vrt, ds, hist, cams[0], cfg, 0)
        after = two_frames()
        assert (before[1]["hist"].reshape(H, W, 4)[..., 3] > 1).any()
        for other in (held, after):
            for a, b in zip(before, other):
                for k in ("px", "col", "hist"):
                    np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32), err_msg=k)
                assert a["cnt"] == b["cnt"]
    finally:
        ds.close()
