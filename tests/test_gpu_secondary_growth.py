"""GPU: the buffers of the secondary tails (csrc/rt_path.hip, csrc/rt_secondary.hip) as they grow.  A frame context allocates the buffers of path, denoised
path and ambient-occlusion frames on first use and grows them, one capacity at a time, when a frame needs more: per pixel, per path,
per occlusion ray; per pixel and per ray of an ambient-occlusion batch; the denoiser's two signal buffers.  Each case below walks ONE
context -- a freshly built DeviceScene, one stream -- through a sequence of frames that allocates the capacities one after the other,
grows them all, and comes back to the small frame that grows nothing.  Every frame of a sequence equals its restatement
(tests/path_ref.py, tests/denoise_ref.py, tests/camera_secondary_ref.py) bit for bit: pixels, colours as u32, rays traced, unoccluded
counts; the status word stays 0.  No masks, no tolerances."""
import numpy as np
import pytest

import camera_secondary_ref as csr
import denoise_cases as dc
import denoise_ref as dr
import path_ref as pr
import scenes

pytestmark = pytest.mark.gpu
MARK = 0x5A5A5A
SEED = 3
# (w, h, spp, bounces, shadow): per-pixel buffers only; + per-path; + occlusion rays; all three capacities grow; nothing grows
PATH_SEQUENCE = ((16, 8, 1, 0, 0), (16, 8, 2, 2, 0), (16, 8, 2, 2, 1), (96, 64, 2, 3, 1), (16, 8, 2, 2, 1))
DN = (2,) + tuple(dc.PATH_DN[1:])   # (iterations, normal_power, sigma_z, sigma_l)
AO_SEQUENCE = ((13, 7, 4), (96, 64, 16), (13, 7, 4))   # (w, h, spp)
CAMERAS = ("orbit_1", None)   # None: the fixed camera


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _camera(vrt, name, w, h):
    return None if name is None else csr.orbit(vrt, 1, 8, w, h)


def _primary_rays(po, cam, w, h):
    import camera_ref as cr
    return po.camera_rays(w, h) if cam is None else cr.rays(cam, w, h)


@pytest.fixture
def hall(vrt, gpu_device):
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    yield b, ds
    ds.close()


def _outputs(dev, w, h):
    import torch
    return (torch.full((h, w), MARK, dtype=torch.int32, device=dev), torch.zeros((h, w, 3), dtype=torch.float32, device=dev),
            torch.full((h, w), 0x7777, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def _host(out):
    import torch
    torch.cuda.synchronize()
    px, col, opn, cnt = out
    return px.cpu().numpy().view(np.uint32), col.cpu().numpy(), opn.cpu().numpy().view(np.uint32), int(cnt.item())


def _same(got, want_px, want_col, want_rays, what):
    px, col, _, rays = got
    print("%s: rays traced %d (restatement %d), pixels that differ %d, colour words that differ %d" % (
        what, rays, want_rays, int((px != want_px).sum()), int((col.view(np.uint32) != np.ascontiguousarray(want_col, np.float32).view(np.uint32)).sum())))
    np.testing.assert_array_equal(col.view(np.uint32), np.ascontiguousarray(want_col, np.float32).view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(px, want_px, err_msg=what + ": pixels")
    assert rays == want_rays, "%s: rays traced %d, restatement %d" % (what, rays, want_rays)


@pytest.mark.parametrize("name", CAMERAS)
@pytest.mark.parametrize("denoised", [False, True])
def test_path_frames_allocate_then_grow_then_fit(vrt, po, hall, name, denoised):
    b, ds = hall
    p, pp = vrt.rtapi.default_shade_params(), po.shade_params()
    want = {}   # (the last frame is the third again: one restatement)
    for i, cfg in enumerate(PATH_SEQUENCE):
        w, h, spp, bounces, shadow = cfg
        cam = _camera(vrt, name, w, h)
        out = _outputs(ds.t["tri"].device, w, h)
        if denoised:
            vrt.rtapi.render_path_denoised(ds.accel, cam, w, h, 0, h, p, spp, bounces, vrt.rtapi.DenoiseParams(*DN), out[0].data_ptr(), SEED, shadow,
                                           out[1].data_ptr(), None, out[3].data_ptr(), _stream())
        else:
            vrt.rtapi.render_path(ds.accel, cam, w, h, 0, h, p, spp, bounces, out[0].data_ptr(), SEED, shadow, out[1].data_ptr(), out[3].data_ptr(), _stream())
        got = _host(out)
        assert vrt.rtapi.status(_stream()) == 0
        if cfg not in want:
            prim = pr.primary(b, _primary_rays(po, cam, w, h))
            if denoised:
                f = dr.path_frame(b, cam, w, h, pp, spp, bounces, SEED, shadow, DN, 0, h, prim)
                want[cfg] = (f["px"], f["col"], f["rays"])
            else:
                want[cfg] = pr.frame(b, cam, w, h, pp, spp, bounces, SEED, shadow, 0, h, prim)[:3]
        _same(got, *want[cfg], "%s %s frame %d %r" % (name, "denoised" if denoised else "path", i, cfg))


@pytest.mark.parametrize("name", CAMERAS)
def test_ao_frames_allocate_then_grow_then_fit(vrt, po, hall, name):
    b, ds = hall
    p, pp = vrt.rtapi.default_shade_params(), po.shade_params()
    radius = csr.RADIUS["mirror_hall"]
    want = {}
    for i, cfg in enumerate(AO_SEQUENCE):
        w, h, spp = cfg
        cam = _camera(vrt, name, w, h)
        out = _outputs(ds.t["tri"].device, w, h)
        if cam is None:
            vrt.rtapi.render_ao(ds.accel, w, h, 0, h, p, spp, radius, out[0].data_ptr(), SEED, out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), _stream())
        else:
            vrt.rtapi.render_ao_camera(ds.accel, cam, w, h, 0, h, p, spp, radius, out[0].data_ptr(), SEED, out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                       _stream())
        got = _host(out)
        assert vrt.rtapi.status(_stream()) == 0
        if cfg not in want:
            want[cfg] = csr.ao_frame(b, cam, w, h, pp, spp, radius, SEED, 0, h, csr.primary(b, _primary_rays(po, cam, w, h), pp))
        rpx, rcol, ropn, rn = want[cfg]
        what = "%s ao frame %d %r" % (name, i, cfg)
        np.testing.assert_array_equal(got[2], ropn, err_msg=what + ": unoccluded")
        _same(got, rpx, rcol, rn, what)
