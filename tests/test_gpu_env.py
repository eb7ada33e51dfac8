"""GPU: the environment light (vxrt_envmap_*, vxrt_envmap_lookup, vxrt_env_rays, vxrt_render_path_frame_env), bit for bit against the
restatement tests/env_ref.py: the table, the two steps alone on hostile inputs, the frames of tests/env_cases.py -- pixels, colours,
rays traced, with counts, roulette and the filter chain the guide outputs and the history besides -- the identities of the definition
against the GPU's own vxrt_render_path_frame, every refusal with everything pre-marked, small batches in a child process and two frames
in flight.  No masks, no tolerances (a NaN of the restatement asks for a NaN); guard words behind every output.
tests/test_env_cpu.py pins the restatement and shows that the cases are not vacuous."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_secondary_ref as csr
import env_cases as vc
import env_ref as ev
import motion_cases as moc
import motion_ref as mr
import temporal_ref as tr
import variance_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = vc.W, vc.H
KEYS = csr.KEYS
MARK = 0x5A5A5A
FMARK = -12345.5
GUARD = 64
CHILD = os.environ.get("VXRT_ENV_TEST_CHILD") == "1"
AOV = (("noisy", 3), ("direct", 3), ("albedo", 3), ("position", 4), ("normal", 4))
FLOATS = (("col", 3),) + AOV + (("var", 1), ("prev", 4), ("hist", 4), ("mom", 2))
f32 = np.float32


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _u32(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(dev)


def _f32(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(dev)


def _outputs(dev, w=W, h=H):
    """every output a frame can have, each with GUARD marked words behind it"""
    import torch
    o = {"px": torch.full((h * w + GUARD,), MARK, dtype=torch.int32, device=dev), "cnt": torch.full((1 + GUARD,), MARK, dtype=torch.int64, device=dev)}
    o["cnt"][0] = 0
    for k, c in FLOATS:
        o[k] = torch.full((h * w * c + GUARD,), FMARK, dtype=torch.float32, device=dev)
    return o


def _host(o, w=W, h=H):
    """the outputs on the host, frame-shaped (hist, mom: flat, window-addressed); the guard words must be untouched"""
    import torch
    torch.cuda.synchronize()
    px, cnt = o["px"].cpu().numpy(), o["cnt"].cpu().numpy()
    assert (px[h * w:] == MARK).all() and (cnt[1:] == MARK).all(), "a guard word was written"
    out = {"px": px[:h * w].view(np.uint32).reshape(h, w), "cnt": int(cnt[0])}
    for k, c in FLOATS:
        a = o[k].cpu().numpy()
        assert (a[h * w * c:] == f32(FMARK)).all(), "a guard word of %s was written" % k
        out[k] = a[:h * w * c] if k in ("hist", "mom") else a[:h * w * c].reshape((h, w, c) if c > 1 else (h, w))
    return out


def _descriptor(vrt, o, cam, w, h, spp, bounces, seed, shadow, params=None, counts=None, dn=None, tp=None, hist=None, vp=None, motion=0, y0=0, y1=None):
    R = vrt.rtapi
    return R.PathFrame(w, h, y0, h if y1 is None else y1, params or R.default_shade_params(), R.PathParams(spp, bounces, seed, shadow),
                       o["px"].data_ptr(), cam=cam, counts=None if counts is None else counts.data_ptr(),
                       denoise=None if dn is None else R.DenoiseParams(*dn), aov=R.PathAov(*[o[n].data_ptr() for n, _ in AOV]) if dn is not None else None,
                       temporal=None if tp is None else R.TemporalParams(*tp), history=hist, variance=None if vp is None else R.VarianceParams(*vp, 0),
                       motion=motion, prev_position=o["prev"].data_ptr() if motion else None, colors=o["col"].data_ptr(), variance_out=o["var"].data_ptr() if vp is not None else None, rays_traced=o["cnt"].data_ptr())


def _render(vrt, ds, cam, cfg, env, w=W, h=H, roulette=None, out=None, stream=None, **parts):
    """vxrt_render_path_frame_env (env = None: vxrt_render_path_frame[_ex]) of cfg = (spp, bounces, shadow, seed) into fresh outputs (or
    `out`); a history is read behind the frame on the same stream"""
    o = out or _outputs(ds.device, w, h)
    s = _stream() if stream is None else stream
    spp, bounces, shadow, seed = cfg
    vrt.rtapi.render_path_frame(ds.accel, _descriptor(vrt, o, cam, w, h, spp, bounces, seed, shadow, **parts), s, roulette=roulette, env=env)
    hist = parts.get("hist")
    if hist is not None:
        hist.read(o["hist"].data_ptr(), s)
        if hist.moments:
            hist.read_moments(o["mom"].data_ptr(), s)
    return o


def _same_floats(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what + ": a NaN of the restatement is not a NaN"
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=what)


def _identical(a, b, what):
    assert a["cnt"] == b["cnt"], "%s: rays traced %d and %d" % (what, a["cnt"], b["cnt"])
    for k in a:
        if k != "cnt":
            np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32), err_msg="%s: %s" % (what, k))


def _check(got, want, what, w=W, h=H, y0=0, y1=None):
    """the outputs against the restatement's dict: what it holds is compared over rows [y0, y1), what it lacks must be untouched"""
    y1 = h if y1 is None else y1
    rows = slice(y0, y1)
    _same_floats(got["col"][rows], want["col"], what + ": colours")
    np.testing.assert_array_equal(got["px"][rows], want["px"], err_msg=what + ": pixels")
    assert (got["px"][:y0] == MARK).all() and (got["px"][y1:] == MARK).all(), what + ": a row outside the window was written"
    assert got["cnt"] == want["rays"], "%s: rays traced %d, restatement %d" % (what, got["cnt"], want["rays"])
    for k, key in [(n, n) for n, _ in AOV] + [("var", "variance"), ("prev", "prev_position")]:
        if key in want:
            _same_floats(got[k][rows], want[key], what + ": " + key)
        else:
            assert (got[k] == f32(FMARK)).all(), what + ": %s was written" % key
    n = (y1 - y0) * w
    for k, key, c in (("hist", "T", 4), ("mom", "M", 2)):
        if key in want:
            _same_floats(got[k][:n * c].reshape(y1 - y0, w, c), want[key], what + ": the history's " + key)
            assert (got[k][n * c:] == f32(FMARK)).all()


def _untouched(o, w=W, h=H):
    got = _host(o, w, h)
    return (got["px"] == MARK).all() and got["cnt"] == 0 and all((got[k] == f32(FMARK)).all() for k, _ in FLOATS)


@pytest.fixture(autouse=True)
def _status_is_clean(vrt):
    yield
    assert vrt.rtapi.status(_stream()) == 0


@pytest.fixture(scope="module")
def scenes_(vrt, gpu_device):
    """name -> (scene buffers, DeviceScene) of the open and the closed scene"""
    out = {}
    for name, make in vc.SCENES.items():
        b = make(vrt)
        out[name] = (b, vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device))
    yield out
    for _, ds in out.values():
        ds.close()


@pytest.fixture(scope="module")
def maps(vrt, gpu_device):
    """name -> (the restatement's map, the EnvMap) of the sun and the HDR map, 16 x 16"""
    out = {}
    for name, make in vc.MAPS.items():
        t = make()
        out[name] = (ev.make_map(t), vrt.rtapi.EnvMap(t, _stream()))
    yield out
    for _, m in out.values():
        m.close()


def _env(vrt, maps, name, sample, scale=vc.SCALE):
    """(the restatement's env part, the EnvParams)"""
    ref, dev = maps[name]
    return (ref, scale, sample), vrt.rtapi.EnvParams(dev, scale, sample)


# ---- 1: the table ----
@pytest.mark.parametrize("kind", ("constant", "one_texel", "hdr", "negzero"))
@pytest.mark.parametrize("n", vc.SIZES)
def test_table(vrt, gpu_device, n, kind):
    texels = getattr(vc, kind)(n)
    want = ev.make_map(texels)
    with vrt.rtapi.EnvMap(texels, _stream()) as m:
        q, cum = m.read(_stream())
        assert m.bytes() == 20 * n * n
        only_q = np.zeros(n * n, np.uint32)
        assert vrt.rtapi._lib().vxrt_envmap_read(m.handle, only_q.ctypes.data, None, _stream()) == 0
    np.testing.assert_array_equal(q, want["q"])
    np.testing.assert_array_equal(cum, want["cum"])
    np.testing.assert_array_equal(only_q, want["q"])
    assert int(cum[-1]) == want["Q"]


# ---- 2: the steps alone ----
@pytest.mark.parametrize("name", ("hdr", "sun"))
def test_env_rays(vrt, gpu_device, maps, name):
    """seeds that give t = 0 and t = Q - 1, texels at both ends of a row, normals that face away (skipped), black texels (skipped)"""
    import torch
    ref, dev = maps[name]
    pts, seeds = vc.ray_points(16, ref)
    k = len(pts)
    wr, wt, wG, we, wE, real = ev.env_rays(ref, vc.SCALE, seeds, pts[:, 0:3], pts[:, 3:6])
    dp, dsd = _f32(gpu_device, pts), _u32(gpu_device, seeds)
    fl = {c: torch.full((k * n_ + GUARD,), FMARK, dtype=torch.float32, device=gpu_device) for c, n_ in (("rays", 6), ("tmax", 1), ("G", 3), ("mis", 1))}
    tex = torch.full((k + GUARD,), MARK, dtype=torch.int32, device=gpu_device)

    def run(n):
        vrt.rtapi.env_rays(dev, n, dp.data_ptr(), dsd.data_ptr(), vc.SCALE, fl["rays"].data_ptr(), fl["tmax"].data_ptr(), fl["G"].data_ptr(), tex.data_ptr(),
                           fl["mis"].data_ptr(), _stream())
        torch.cuda.synchronize()
        return {c: v.cpu().numpy() for c, v in fl.items()}, tex.cpu().numpy()
    got, e = run(257)                                        # (no multiple of the workgroup: nothing behind entry 256 is written)
    assert (got["rays"][6 * 257:] == f32(FMARK)).all() and (got["mis"][257:] == f32(FMARK)).all() and (e[257:] == MARK).all()
    vrt.rtapi.env_rays(dev, 0, dp.data_ptr(), dsd.data_ptr(), vc.SCALE, fl["rays"].data_ptr() + 24 * 300, fl["tmax"].data_ptr(), fl["G"].data_ptr(), tex.data_ptr(),
                       fl["mis"].data_ptr(), _stream())
    got, e = run(k)
    for c, n_ in (("rays", 6), ("tmax", 1), ("G", 3), ("mis", 1)):
        assert (got[c][k * n_:] == f32(FMARK)).all(), c
    assert (e[k:] == MARK).all()
    np.testing.assert_array_equal(e[:k].view(np.uint32), we)
    _same_floats(got["rays"][:6 * k].reshape(k, 6), wr, "rays")
    _same_floats(got["tmax"][:k], wt, "tmax")
    _same_floats(got["G"][:3 * k].reshape(k, 3), wG, "Gm")
    _same_floats(got["mis"][:k], wE, "wE")
    assert (~real).sum() > 100 and real.sum() > 100
    assert (dp.cpu().numpy().view(np.uint32) == pts.view(np.uint32)).all()


@pytest.mark.parametrize("n", vc.SIZES)
def test_lookup(vrt, gpu_device, n):
    """the axes, +-0 components, the fold, the poles, NaNs, infinities and the zero vector, then random directions"""
    import torch
    texels = vc.negzero(n)                                   # (hdr with -0.0 texels: Env(w) of one is -0 * scale)
    ref = ev.make_map(texels)
    d = vc.lookup_dirs()
    k = len(d)
    wL, we, wp = ev.lookup(ref, vc.SCALE, d)
    dd = _f32(gpu_device, d)
    L = torch.full((3 * k + GUARD,), FMARK, dtype=torch.float32, device=gpu_device)
    p = torch.full((k + GUARD,), FMARK, dtype=torch.float32, device=gpu_device)
    e = torch.full((k + GUARD,), MARK, dtype=torch.int32, device=gpu_device)
    with vrt.rtapi.EnvMap(texels, _stream()) as m:
        vrt.rtapi.env_lookup(m, k, dd.data_ptr(), vc.SCALE, L.data_ptr(), e.data_ptr(), p.data_ptr(), _stream())
        torch.cuda.synchronize()
    L, p, e = L.cpu().numpy(), p.cpu().numpy(), e.cpu().numpy()
    assert (L[3 * k:] == f32(FMARK)).all() and (p[k:] == f32(FMARK)).all() and (e[k:] == MARK).all()
    np.testing.assert_array_equal(e[:k].view(np.uint32), we)
    _same_floats(L[:3 * k].reshape(k, 3), wL, "Env(w)")
    _same_floats(p[:k], wp, "pe(w)")
    nan = np.isnan(d).any(1)
    assert (we[nan] == 0).all() and (we[(d == 0).all(1)] == 0).all() and len(np.unique(we)) > min(n * n, 500) // 2


# ---- 3: the frames against the restatement ----
def _run_frame(vrt, po, scenes_, maps, name, roulette=None, counts=False):
    scene, map_name, frame, spp, bounces, shadow, seed, sample, cam_name = vc.FRAMES[name]
    b, ds = scenes_[scene]
    w, h, (y0, y1) = vc.window(frame)
    cam = vc.camera(vrt, cam_name, w, h)
    renv, denv = _env(vrt, maps, map_name, sample)
    raw = vc.counts_of(w, h) if counts else None
    rp = None if roulette is None else vrt.rtapi.RouletteParams(1, roulette[0], roulette[1])
    got = _host(_render(vrt, ds, cam, (spp, bounces, shadow, seed), denv, w, h, rp, counts=None if raw is None else _u32(ds.device, raw), y0=y0, y1=y1), w, h)
    want = ev.frame(b, cam, w, h, po.shade_params(), spp, bounces, seed, shadow, renv, raw, roulette, y0=y0, y1=y1)
    return got, want, (w, h, y0, y1)


@pytest.mark.parametrize("name", list(vc.FRAMES))
def test_frame_against_the_restatement(vrt, po, scenes_, maps, name):
    """pixels, colours and rays traced: sample 0 and 1, bounces 0, 1, 3, spp 1, 3, 4, shadow 0 and 1, both cameras, a row window, the
    closed and the open scene; the child process of test_small_batches runs them again"""
    got, want, (w, h, y0, y1) = _run_frame(vrt, po, scenes_, maps, name)
    _check(got, want, name, w, h, y0, y1)


@pytest.mark.parametrize("name", ("open_s0", "open_s1"))
def test_frame_with_counts(vrt, po, scenes_, maps, name):
    got, want, (w, h, y0, y1) = _run_frame(vrt, po, scenes_, maps, name, counts=True)
    _check(got, want, name + " with counts", w, h, y0, y1)


@pytest.mark.parametrize("name", ("open_s0", "open_s1", "open_s1_sun_pinhole"))
@pytest.mark.parametrize("counts", (False, True))
def test_frame_with_roulette(vrt, po, scenes_, maps, name, counts):
    got, want, (w, h, y0, y1) = _run_frame(vrt, po, scenes_, maps, name, roulette=(vc.ROULETTE["first"], vc.ROULETTE["q_min"]), counts=counts)
    _check(got, want, name + " with roulette", w, h, y0, y1)


def _run_chain(vrt, po, scenes_, maps, chain, hist, ref_hist):
    """one frame of open_s1_sun_pinhole's configuration through the filter chain, on a fresh history"""
    scene, map_name, frame, spp, bounces, shadow, seed, sample, cam_name = vc.FRAMES["open_s1_sun_pinhole"]
    b, ds = scenes_[scene]
    cam = vc.camera(vrt, cam_name, W, H)
    renv, denv = _env(vrt, maps, map_name, sample)
    got = _host(_render(vrt, ds, cam, (spp, bounces, shadow, seed), denv, hist=hist, **chain))
    want = ev.frame(b, cam, W, H, po.shade_params(), spp, bounces, seed, shadow, renv, hist=ref_hist, **chain)
    return got, want


def test_frame_denoised(vrt, po, scenes_, maps):
    got, want = _run_chain(vrt, po, scenes_, maps, dict(dn=vc.DN), None, None)
    _check(got, want, "denoised")
    miss = want["position"][..., 3] == 0
    assert miss.any() and (~miss).any() and (want["direct"][miss] > 0).any()


def test_frame_temporal(vrt, po, scenes_, maps):
    with vrt.rtapi.History(W, H) as hist:
        got, want = _run_chain(vrt, po, scenes_, maps, dict(dn=vc.DN, tp=vc.TP), hist, tr.History())
    _check(got, want, "temporal")


def test_frame_variance(vrt, po, scenes_, maps):
    with vrt.rtapi.History(W, H, moments=True) as hist:
        got, want = _run_chain(vrt, po, scenes_, maps, dict(dn=vc.DN, tp=vc.TP, vp=vc.VP), hist, vr.History())
    _check(got, want, "variance")


def test_frame_with_motion(vrt, po, gpu_device, maps):
    """two temporal frames on one history, the blob moved between them and the second reprojected through the snapshot (motion = 1, the
    prepare launch's flavour with motion): the guide outputs, prev_position and the history besides"""
    b = vc.open_scene(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, gpu_device)
    try:
        renv, denv = _env(vrt, maps, "sun", 1)
        cam = vc.camera(vrt, "pinhole", W, H)
        ref = tr.History()
        with vrt.rtapi.History(W, H) as hist:
            for k in range(2):
                cur = b if k == 0 else mr.moved(b, moc.BLOB, moc.translation(2)[None])
                snap = mr.snapshot(b)
                ds.snapshot_motion(mr.INSTANCES)
                if k:
                    ds.set_transforms([moc.translation(2)], moc.BLOB)
                got = _host(_render(vrt, ds, cam, (2, 2, 1, 3 + k), denv, dn=vc.DN, tp=vc.TP, hist=hist, motion=1))
                want = ev.frame(cur, cam, W, H, po.shade_params(), 2, 2, 3 + k, 1, renv, dn=vc.DN, tp=vc.TP, hist=ref, motion=1, snap=snap)
                _check(got, want, "motion frame %d" % k)
        moved = (want["prev_position"][..., :3] != want["position"][..., :3]).any(-1) & (want["position"][..., 3] != 0)
        assert moved.any() and (want["T"][..., 3] > 1).any() and (want["position"][..., 3] == 0).any()
    finally:
        ds.close()


# ---- 4: the identities ----
def test_constant_map_is_the_plain_frame(vrt, scenes_):
    """CONSTANT: every texel c, scale = 1, sample = 0, background = c is vxrt_render_path_frame bit for bit"""
    R = vrt.rtapi
    c = (0.4, 0.35, 0.25)
    with R.EnvMap(vc.constant(16, c), _stream()) as m:
        for scene in ("open", "closed"):
            b, ds = scenes_[scene]
            for cam_name in ("fixed", "pinhole"):
                cam = vc.camera(vrt, cam_name, W, H)
                p = R.default_shade_params()
                p.background[:] = c
                plain = _host(_render(vrt, ds, cam, (3, 3, 1, 3), None, params=p))
                _identical(_host(_render(vrt, ds, cam, (3, 3, 1, 3), R.EnvParams(m, 1.0, 0), params=p)), plain, "constant map, %s, %s" % (scene, cam_name))
                assert plain["cnt"] > W * H


def test_null_env_is_the_ex_entry_point(vrt, scenes_):
    R, L = vrt.rtapi, vrt.rtapi._lib()
    b, ds = scenes_["open"]
    cam = vc.camera(vrt, "pinhole", W, H)
    for rp in (None, R.RouletteParams(1, vc.ROULETTE["first"], vc.ROULETTE["q_min"])):
        plain = _host(_render(vrt, ds, cam, (2, 3, 1, 3), None, roulette=rp))
        o = _outputs(ds.device)
        d = _descriptor(vrt, o, cam, W, H, 2, 3, 3, 1)
        assert L.vxrt_render_path_frame_env(ds.accel, C.byref(d), None if rp is None else C.byref(rp), None, _stream()) == 0
        _identical(_host(o), plain, "env == NULL")


def test_flat_frame_differs_at_miss_pixels_only(vrt, scenes_, maps):
    b, ds = scenes_["open"]
    _, denv = _env(vrt, maps, "hdr", 1)
    plain = _host(_render(vrt, ds, None, (3, 0, 1, 1), None))
    lit = _host(_render(vrt, ds, None, (3, 0, 1, 1), denv))
    bg = np.asarray(vrt.rtapi.default_shade_params().background[:], np.float32)
    miss = (plain["col"].view(np.uint32) == bg.view(np.uint32)).all(-1)
    differs = (plain["col"].view(np.uint32) != lit["col"].view(np.uint32)).any(-1)
    assert miss.any() and (~miss).any() and differs.any() and not (differs & ~miss).any()
    assert lit["cnt"] == plain["cnt"]


# ---- 5: refusals ----
def test_refusals_leave_everything_untouched(vrt, gpu_device, scenes_, maps):
    import torch
    R = vrt.rtapi
    L = R._lib()
    b, ds = scenes_["open"]
    cam = vc.camera(vrt, "pinhole", W, H)
    _, good = _env(vrt, maps, "hdr", 1)
    o = _outputs(gpu_device)

    def call(env, rp=None, edit=None, accel="own", **parts):
        d = _descriptor(vrt, o, parts.pop("cam", cam), W, H, parts.pop("spp", 2), parts.pop("bounces", 2), 3, parts.pop("shadow", 1), **parts)
        if edit:
            edit(d)
        return L.vxrt_render_path_frame_env(ds.accel if accel == "own" else accel, C.byref(d), None if rp is None else C.byref(rp), None if env is None else C.byref(env),
                                            _stream())

    def part(map=maps["hdr"][1], scale=1.0, sample=1, reserved=0):
        e = R.EnvParams(map, scale, sample)
        e.reserved = reserved
        return e

    def setter(**kw):
        def edit(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return edit
    # the part itself
    for bad in (part(map=None), part(sample=2), part(sample=0xFFFFFFFF), part(scale=-1.0), part(scale=float("nan")), part(scale=float("inf")),
                part(scale=float("-inf")), part(reserved=1), part(reserved=0x80000000)):
        assert call(bad) == -1, (bad.map, bad.scale, bad.sample, bad.reserved)
        assert call(bad, edit=setter(y0=5, y1=5)) == -1                                       # (ahead of the empty window)
    # env beside an emitter form
    em = R.EmissiveParams(0, 1.0, (C.c_uint32 * 2)(0, 0))
    mis = R.EmissiveMisParams(1.0, (C.c_uint32 * 3)(0, 0, 0))
    assert call(good, edit=setter(emissive=C.pointer(em))) == -1 and call(good, edit=setter(emissive_mis=C.pointer(mis))) == -1
    # a bad roulette part beside it
    for rp in (R.RouletteParams(2, 1, 0.3), R.RouletteParams(1, 0, 0.3), R.RouletteParams(1, 1, 0.0), R.RouletteParams(1, 1, float("nan"))):
        assert call(good, rp) == -1
    # everything vxrt_render_path_frame_ex refuses
    assert call(good, accel=None) == -1
    assert L.vxrt_render_path_frame_env(ds.accel, None, None, C.byref(good), _stream()) == -1
    assert call(good, edit=setter(size=C.sizeof(R.PathFrame) - 8)) == -1
    assert call(good, edit=setter(reserved=(C.c_uint32 * 4)(0, 0, 1, 0))) == -1
    assert call(good, edit=setter(path=None)) == -1 and call(good, edit=setter(params=None)) == -1 and call(good, edit=setter(dst=None)) == -1
    assert call(good, edit=setter(y0=5, y1=3)) == -1 and call(good, edit=setter(y1=H + 1)) == -1 and call(good, edit=setter(width=0)) == -1
    assert call(good, spp=0) == -1 and call(good, spp=4097) == -1 and call(good, bounces=R.PATH_MAX_BOUNCES + 1) == -1 and call(good, shadow=2) == -1
    assert call(good, dn=vc.DN, tp=vc.TP) == -1                                               # temporal without a history
    assert call(good, edit=setter(variance_out=o["var"].data_ptr()), dn=vc.DN) == -1          # variance_out without variance
    assert call(good, edit=setter(y0=7, y1=7)) == 0                                           # the empty window
    assert _untouched(o) and R.status(_stream()) == 0
    assert call(good) == 0                                                                    # and the frame that is allowed renders
    torch.cuda.synchronize()
    assert (_host(o)["px"] != MARK).all()
    # a bad vxrt_envmap_create makes nothing
    t = vc.hdr(16)
    h = C.c_void_p()
    for bad_n in (0, 2, 3, 12, 512, 1 << 31):
        assert L.vxrt_envmap_create(t.ctypes.data, bad_n, _stream(), C.byref(h)) == -1 and not h.value
    assert L.vxrt_envmap_create(None, 16, _stream(), C.byref(h)) == -1 and L.vxrt_envmap_create(t.ctypes.data, 16, _stream(), None) == -1
    for v in (-1.0, np.nan, np.inf, -np.inf):
        bad = t.copy()
        bad[5, 7, 2] = v
        assert L.vxrt_envmap_create(bad.ctypes.data, 16, _stream(), C.byref(h)) == -1 and not h.value
    black = np.zeros((16, 16, 3), np.float32)
    assert L.vxrt_envmap_create(black.ctypes.data, 16, _stream(), C.byref(h)) == -1 and not h.value
    huge = vc.constant(16)
    huge[8, 8] = 3e38
    assert ev.make_map(huge) is None and L.vxrt_envmap_create(huge.ctypes.data, 16, _stream(), C.byref(h)) == -1 and not h.value
    assert L.vxrt_envmap_destroy(None) == -1 and L.vxrt_envmap_bytes(None) == 0 and L.vxrt_envmap_read(None, None, None, _stream()) == -1
    # the steps alone
    dev = maps["hdr"][1]
    pts = torch.zeros(60, dtype=torch.float32, device=gpu_device)
    sd = torch.zeros(10, dtype=torch.int32, device=gpu_device)
    fo = torch.full((200,), FMARK, dtype=torch.float32, device=gpu_device)
    io = torch.full((10,), MARK, dtype=torch.int32, device=gpu_device)
    rays_args = [dev.handle, 10, pts.data_ptr(), sd.data_ptr(), 1.0, fo.data_ptr(), fo.data_ptr() + 240, fo.data_ptr() + 280, io.data_ptr(), fo.data_ptr() + 400, _stream()]
    look_args = [dev.handle, 10, pts.data_ptr(), 1.0, fo.data_ptr(), io.data_ptr(), fo.data_ptr() + 120, _stream()]
    for fn, args, ptrs, scale_at in ((L.vxrt_env_rays, rays_args, (0, 2, 3, 5, 6, 7, 8, 9), 4), (L.vxrt_envmap_lookup, look_args, (0, 2, 4, 5, 6), 3)):
        for k in ptrs:
            bad = list(args)
            bad[k] = None
            assert fn(*bad) == -1
        for s in (-1.0, float("nan"), float("inf")):
            assert fn(*(args[:scale_at] + [s] + args[scale_at + 1:])) == -1
        assert fn(*(args[:1] + [2 ** 31] + args[2:])) == -1 and fn(*(args[:1] + [2 ** 40] + args[2:])) == -1
        assert fn(*(args[:1] + [0] + args[2:])) == 0
    torch.cuda.synchronize()
    assert (fo.cpu().numpy() == f32(FMARK)).all() and (io.cpu().numpy() == MARK).all() and R.status(_stream()) == 0


def test_alpha_table_is_refused(vrt, golden, gpu_device, maps):
    """a path frame honours no alpha table, so neither does this one"""
    import shading_ref as sr
    g = golden("tex_mix")
    ds = vrt.tracer.DeviceScene({k: g[k] for k in KEYS}, gpu_device)
    try:
        mat = np.frombuffer(np.ascontiguousarray(g["mat"], np.uint8).tobytes(), sr.MAT_DT)
        assert (mat["tex_id"] >= 0).any()
        _, good = _env(vrt, maps, "hdr", 1)
        cam = csr.golden_cameras(vrt, W, H)["g_orbit_1"]
        L = vrt.rtapi._lib()
        o = _outputs(gpu_device)
        d = _descriptor(vrt, o, cam, W, H, 2, 2, 3, 1)
        ds.set_alpha_test([128 if t >= 0 else 0 for t in mat["tex_id"]])
        assert vrt.rtapi.accel_info(ds.accel, 4) == 1
        assert L.vxrt_render_path_frame_env(ds.accel, C.byref(d), None, C.byref(good), _stream()) == -1 and _untouched(o)
        ds.set_alpha_test(None)
        assert L.vxrt_render_path_frame_env(ds.accel, C.byref(d), None, C.byref(good), _stream()) == 0
        assert (_host(o)["px"] != MARK).all()
    finally:
        ds.close()


# ---- 6: small batches, two frames in flight ----
def test_small_batches(vrt):
    """VXRT_PATH_BATCH is read once per process: a fresh child runs the frames again with vc.CHILD_BATCH paths per batch -- batches of
    one sample each whose last workgroup is partly live, and for the counts tail pixels that straddle batches and a short last batch.
    The knob line the library prints under VXRT_DEBUG shows that the child took it."""
    assert not CHILD
    env = dict(os.environ, VXRT_PATH_BATCH=str(vc.CHILD_BATCH), VXRT_ENV_TEST_CHILD="1", VXRT_DEBUG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k",
                        "test_frame_against_the_restatement or test_frame_with_counts"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % (len(vc.FRAMES) + 2) in r.stdout and ("path_batch=%d " % vc.CHILD_BATCH) in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_two_frames_in_flight(vrt, po, scenes_, maps):
    """a frame that samples the map (counts, roulette) and one that only sees it (denoised) on two streams, twice: the second round finds
    the contexts' buffers grown"""
    import torch
    b, ds = scenes_["open"]
    dev, p = ds.device, po.shade_params()
    vrt.rtapi.accel_frames_in_flight(ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        cam = vc.camera(vrt, "pinhole", W, H)
        raw = vc.counts_of(salt=1)
        rl = (vc.ROULETTE["first"], vc.ROULETTE["q_min"])
        r1, d1 = _env(vrt, maps, "sun", 1)
        r0, d0 = _env(vrt, maps, "hdr", 0)
        cfgs = ((4, 3, 1, 3), (2, 2, 0, 5))
        parts = [dict(env=d1, roulette=vrt.rtapi.RouletteParams(1, *rl), counts=_u32(dev, raw)), dict(env=d0, dn=vc.DN)]
        outs = [_outputs(dev) for _ in range(2)]
        torch.cuda.synchronize()
        for rnd in range(2):
            for i in range(2):
                _render(vrt, ds, cam, cfgs[i], w=W, h=H, out=outs[i], stream=streams[i].cuda_stream, **parts[i])
            torch.cuda.synchronize()
            if rnd == 0:
                outs = [_outputs(dev) for _ in range(2)]
                torch.cuda.synchronize()
        (s1, b1, sh1, sd1), (s0, b0, sh0, sd0) = cfgs
        _check(_host(outs[0]), ev.frame(b, cam, W, H, p, s1, b1, sd1, sh1, r1, raw, rl), "in flight, sampled")
        _check(_host(outs[1]), ev.frame(b, cam, W, H, p, s0, b0, sd0, sh0, r0, dn=vc.DN), "in flight, seen")
    finally:
        vrt.rtapi.accel_frames_in_flight(ds.accel, 1)
