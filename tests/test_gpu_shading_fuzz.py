"""GPU: the closest-hit / miss shader under randomised shading inputs (tests/shading_cases.py: materials, textures of odd sizes, per-corner
normals, uv, reflectivities, lights and shade parameters, benign and hostile) through every entry point that instantiates it --
vxrt_shade_rays, the frame kernels (fixed camera, camera form, batch), the mirror bounce, AO, the one-launch diffuse bounce and the
STATS build -- against the oracle: hit records, counts and ray totals bit-equal, RGB8 equal, colours within COLOR_RTOL with NaN in
the same places, vxrt_status 0.  The conversions C leaves undefined run against the constants pinned in tests/test_shading_cpu.py."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_ref as cr
import shading_cases as sc
import test_shading_cpu as pins
from test_gpu_parity import COLOR_RTOL, _bits, gpu_render

pytestmark = pytest.mark.gpu
LDS_VARIANT = os.environ.get("VXRT_SHADING_TEST_VARIANT") == "1"
N_SEEDS = int(os.environ.get("VXRT_FUZZ_SEEDS", "6"))          # (VXRT_FUZZ_SEEDS=n: a soak run over n seeds)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _gpu_params(vrt, p):
    q = vrt.rtapi.ShadeParams()
    q.ambient[:], q.light_color[:], q.light_pos[:], q.background[:] = p.ambient[:], p.light_color[:], p.light_pos[:], p.background[:]
    q.max_depth = p.max_depth
    return q


def _with_depth(po, p, depth):
    a, lc, lp, bg, _ = sc.params_tuple(p)
    return po.shade_params(a, lc, lp, bg, depth)


def _build(vrt, po, gpu_device, seed, family, builder):
    """the case on the tree of the CPU builder or of the GPU builder: (buffers, device scene, parameter sets, extra)"""
    meshes, xf = sc.geometry(seed, family)
    if builder == "cpu":
        s = vrt.scene.from_triangles(meshes, xf)
        b = {k: np.frombuffer(bytes(s.buffers[k]), np.uint8).copy() for k in sc.KEYS}
    else:
        tmp = vrt.tracer.DeviceScene.build_on_gpu(meshes, transforms=xf, device=gpu_device, leaf_max=1 + seed % 4)
        b = {k: tmp.t[k].cpu().numpy().copy() for k in sc.KEYS}
        tmp.close()
    b, plist, extra = sc.decorate(b, seed, family, po, xf, [len(m) for m in meshes])
    return b, vrt.tracer.DeviceScene(b, gpu_device), plist, extra


def _shade_rays(vrt, ds, rays, hits, p):
    import torch
    n = len(rays)
    r = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(ds.device)
    h = torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).copy()).to(ds.device)
    col = torch.zeros(n * 3, dtype=torch.float32, device=ds.device)
    px = torch.zeros(n, dtype=torch.int32, device=ds.device)
    vrt.rtapi.shade_rays(ds.accel, r.data_ptr(), h.data_ptr(), n, _gpu_params(vrt, p), col.data_ptr(), px.data_ptr(), _stream())
    assert vrt.rtapi.status(_stream()) == 0
    return col.cpu().numpy().reshape(n, 3), px.cpu().numpy().view(np.uint32)


def _same(col, px, want_col, want_px, what):
    bad = np.nonzero(np.asarray(px).reshape(-1) != np.asarray(want_px).reshape(-1))[0]
    assert len(bad) == 0, "%s: %d of %d RGB8 values differ, first at %s" % (what, len(bad), np.asarray(px).size, bad[:5])
    np.testing.assert_allclose(col, want_col, rtol=COLOR_RTOL, atol=0, err_msg=what)     # (NaN must coincide: equal_nan compares positions)


def _check_per_ray(vrt, po, b, ds, plist, rays, hits, what):
    for k, p in enumerate(plist):
        col, px = _shade_rays(vrt, ds, rays, hits, p)
        want_col, want_px = po.shade(b, rays, hits, p)
        _same(col, px, want_col, want_px, "%s: vxrt_shade_rays, parameter set %d" % (what, k))


def _check_frames(vrt, po, b, ds, plist, what):
    for k, p in enumerate(plist):
        w, h = sc.FRAME_SIZES[k % 2]
        shadow = k % 2
        gpx, ghits, gcol, nrays = gpu_render(vrt, ds, w, h, shadow=shadow, params=_gpu_params(vrt, p))
        rpx, rhits, rcol, rn = po.render_ex(b, w, h, p, shadow)
        tag = "%s: vxrt_render %dx%d, parameter set %d, shadow %d, max_depth %d" % (what, w, h, k, shadow, p.max_depth)
        assert np.array_equal(_bits(ghits), _bits(rhits)), tag + ": hit records"
        assert nrays == rn, tag + ": rays traced %d, oracle %d" % (nrays, rn)
        _same(gcol, gpx, rcol, rpx, tag)


def _check_batch(vrt, po, b, ds, plist, what):
    """three frames with different parameters in one set of launches (the batch forms take no mirror bounce: max_depth 1)"""
    import torch
    w, h = sc.FRAME_SIZES[0]
    three = [_with_depth(po, p, 1) for p in plist[:3]]
    buf = torch.zeros((3, h, w), dtype=torch.int32, device=ds.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=ds.device)
    vrt.rtapi.render_batch(ds.accel, w, h, [_gpu_params(vrt, p) for p in three], buf.data_ptr(), w * h, 1, cnt.data_ptr(), _stream())
    assert vrt.rtapi.status(_stream()) == 0
    total = 0
    for f, p in enumerate(three):
        rpx, _, _, rn = po.render_ex(b, w, h, p, 1)
        total += rn
        _same(np.zeros(1), buf[f].cpu().numpy().view(np.uint32), np.zeros(1), rpx, "%s: vxrt_render_batch, frame %d" % (what, f))
    assert int(cnt.item()) == total, what + ": vxrt_render_batch rays traced"


def _check_camera(vrt, po, b, ds, p, what):
    import torch
    from oracle.pyoracle import HIT_DTYPE
    w, h = sc.FRAME_SIZES[1]
    cam = np.array(vrt.rtapi.look_at((40.0, 190.0, -160.0), (265.0, 100.0, 0.0), (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32)
    px = torch.zeros((h, w), dtype=torch.int32, device=ds.device)
    hits = torch.zeros(h * w * 24, dtype=torch.uint8, device=ds.device)
    col = torch.zeros(h * w * 3, dtype=torch.float32, device=ds.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=ds.device)
    vrt.rtapi.render_camera(ds.accel, cam, w, h, 0, h, _gpu_params(vrt, p), px.data_ptr(), 1, hits.data_ptr(), col.data_ptr(), cnt.data_ptr(), _stream())
    assert vrt.rtapi.status(_stream()) == 0
    rpx, rhits, rcol, rn = cr.frame(b, cam, w, h, p, 1)
    tag = "%s: vxrt_render_camera, max_depth %d" % (what, p.max_depth)
    assert np.array_equal(_bits(hits.cpu().numpy().view(HIT_DTYPE).reshape(h, w)), _bits(rhits)), tag + ": hit records"
    assert int(cnt.item()) == rn, tag + ": rays traced"
    assert (rhits["dist"] != np.float32(1e30)).sum() >= 50, tag + ": the camera sees the scene"
    _same(col.cpu().numpy().reshape(h, w, 3), px.cpu().numpy().view(np.uint32), rcol, rpx, tag)


def _check_secondary_passes(vrt, po, b, ds, p, seed, what):
    import torch
    w, h = sc.FRAME_SIZES[1]
    q = _gpu_params(vrt, p)
    px = torch.zeros((h, w), dtype=torch.int32, device=ds.device)
    col = torch.zeros(h * w * 3, dtype=torch.float32, device=ds.device)
    cnt = torch.full((h, w), -1, dtype=torch.int32, device=ds.device)
    nr = torch.zeros(1, dtype=torch.int64, device=ds.device)
    spp, radius, sd = (1, 4, 8)[seed % 3], 25.0 + 20.0 * seed, 12345 + seed
    vrt.rtapi.render_ao(ds.accel, w, h, 0, h, q, spp, radius, px.data_ptr(), seed=sd, colors_ptr=col.data_ptr(), unoccluded_ptr=cnt.data_ptr(),
                        rays_ptr=nr.data_ptr(), stream=_stream())
    assert vrt.rtapi.status(_stream()) == 0
    rpx, rcol, rcnt, rn = po.render_ao(b, w, h, p, spp=spp, radius=radius, seed=sd)
    np.testing.assert_array_equal(cnt.cpu().numpy().view(np.uint32), rcnt, err_msg=what + ": vxrt_render_ao unoccluded counts")
    assert int(nr.item()) == rn, what + ": vxrt_render_ao rays traced"
    _same(col.cpu().numpy().reshape(h, w, 3), px.cpu().numpy().view(np.uint32), rcol, rpx, what + ": vxrt_render_ao")
    nr.zero_()
    vrt.rtapi.render_diffuse_bounce(ds.accel, w, h, 0, h, q, px.data_ptr(), seed=sd, colors_ptr=col.data_ptr(), rays_ptr=nr.data_ptr(), stream=_stream())
    assert vrt.rtapi.status(_stream()) == 0
    rpx, rcol, rn = po.render_gi(b, w, h, p, seed=sd)
    assert int(nr.item()) == rn, what + ": vxrt_render_diffuse_bounce rays traced"
    _same(col.cpu().numpy().reshape(h, w, 3), px.cpu().numpy().view(np.uint32), rcol, rpx, what + ": vxrt_render_diffuse_bounce")


def _check_stats(vrt, po, b, ds, p, what):
    """the STATS build of the frame kernels: pixels, and its textured-hit counter against the oracle's count of textured hits"""
    import torch
    w, h = sc.FRAME_SIZES[0]
    p1 = _with_depth(po, p, 1)
    px = torch.zeros((h, w), dtype=torch.int32, device=ds.device)
    c = vrt.rtapi.render_stats(ds.accel, w, h, 0, h, _gpu_params(vrt, p1), px.data_ptr(), 0, _stream())
    assert vrt.rtapi.status(_stream()) == 0
    rpx, rhits, _ = po.render(b, w, h, p1)
    found = rhits["dist"].reshape(-1) != np.float32(1e30)
    tex_id = np.frombuffer(b["triEx"].tobytes(), np.uint32).reshape(-1, 16)[rhits["triIdx"].reshape(-1)[found], 15]
    textured = np.frombuffer(b["mat"].tobytes(), sc.MAT_DT)["tex_id"][tex_id] >= 0
    assert c["textured_hits"] == int(textured.sum()) and 0 < int(textured.sum()) < int(found.sum()), what + ": textured hits"
    assert c["shaded_hits"] == int(found.sum()) and c["pixels"] == w * h, what + ": shaded hits / pixels"
    np.testing.assert_array_equal(px.cpu().numpy().view(np.uint32), rpx, err_msg=what + ": vxrt_render_stats pixels")


@pytest.mark.parametrize("family", ["benign", "hostile"])
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_shading_fuzz(vrt, po, gpu_device, seed, family):
    builder = ("cpu", "gpu")[seed % 2]
    what = "%s seed %d (%s builder)" % (family, seed, builder)
    b, ds, plist, extra = _build(vrt, po, gpu_device, seed, family, builder)
    try:
        rays, hits = sc.per_ray_inputs(po, b, seed, family, extra)
        assert seed >= len(sc.SEEDS) or (hits["dist"] != np.float32(1e30)).sum() > 200
        _check_per_ray(vrt, po, b, ds, plist, rays, hits, what)
        _check_frames(vrt, po, b, ds, plist, what)
        _check_batch(vrt, po, b, ds, plist, what)
        _check_camera(vrt, po, b, ds, plist[seed % len(plist)], what)
        _check_secondary_passes(vrt, po, b, ds, plist[(seed + 1) % len(plist)], seed, what)
        _check_stats(vrt, po, b, ds, plist[0], what)
    finally:
        ds.close()


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_outside_c_family_equals_the_pinned_x86_results(vrt, po, gpu_device, seed):
    """uv * w >= 2^63, +-inf and NaN uv, channels beyond +-2^31 and NaN, NaN / inf shade parameters: vxrt_shade_rays and vxrt_render
    return what the written rule says -- the oracle's result, whose checksum tests/test_shading_cpu.py pins (CPU builder: the
    pinned results are of its tree)."""
    what = "outside_c seed %d" % seed
    b, ds, plist, extra = _build(vrt, po, gpu_device, seed, "outside_c", "cpu")
    try:
        rays, hits = sc.per_ray_inputs(po, b, seed, "outside_c", extra)
        assert pins.outside_c_crc(po, b, plist, rays, hits) == pins.OUTSIDE_C_CRC[seed]
        _check_per_ray(vrt, po, b, ds, plist, rays, hits, what)
        _check_frames(vrt, po, b, ds, plist, what)
    finally:
        ds.close()


def test_pinned_conversions(vrt, po, gpu_device):
    """the constants themselves: every PACK_PINS colour as the background of a miss, every F2U_PINS value as u * w of a textured hit"""
    b, rays, hits, p, want = pins.probe_case(vrt, po)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        _, px = _shade_rays(vrt, ds, rays, hits, p)
        np.testing.assert_array_equal(px, want, err_msg="uint32_t(u * w) for u * w in %s" % ([x for x, _ in pins.F2U_PINS],))
        miss = np.zeros(1, po.HIT_DTYPE)
        miss["dist"] = 1e30
        for colour, packed in pins.PACK_PINS:
            q = po.shade_params(background=colour)
            col, px = _shade_rays(vrt, ds, rays[:1], miss, q)
            assert int(px[0]) == packed, "pack of %s: %#010x, pinned %#010x" % (colour, int(px[0]), packed)
            assert np.array_equal(col[0].view(np.uint32), np.array(colour, np.float32).view(np.uint32)) or np.isnan(colour).any()
    finally:
        ds.close()


def test_shading_fuzz_on_the_lds_staging_variant(vrt, gpu_device):
    """The same file on the library with both LDS-staging variants on (built by build(); tests/test_gpu_variants.py's library):
    one child process, started after this one's launches have drained."""
    if LDS_VARIANT:
        return
    import torch
    torch.cuda.synchronize()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = importlib.import_module("vortex-raytracing_amd.build").build_test_variant()   # (rebuilt when a source or header is newer)
    env = dict(os.environ, VXRT_LIB_DIR=lib, VXRT_SHADING_TEST_VARIANT="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "not lds_staging"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
