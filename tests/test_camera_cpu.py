"""CPU: the camera frame's numpy restatement (tests/camera_ref.py) against the oracle, the camera entry points' exports and
declarations, and rtapi.look_at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import camera_ref as cr
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vxrt_render_camera", "vxrt_render_batch_camera", "vxrt_pinhole_rays")


def _rc_args(po, cam14, w, h):
    empty = {k: np.zeros(4, np.uint8) for k in po.RC_BUFFERS}
    empty["tlas_root"] = 0
    return po.rc_args(empty, w, h, cam14)


def _cameras():
    rng = np.random.default_rng(7)
    cams = dict(cr.hostile_cameras(13, 7))
    for i in range(14):
        c = rng.standard_normal(14).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 4))
        cams["random_%d" % i] = c
    cams["rtu_like"] = np.array([0, 100, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * 13 / 7, 2.0], np.float32)
    return cams


@pytest.mark.parametrize("name", sorted(_cameras()))
def test_rays_equal_the_oracle(po, name):
    cam = _cameras()[name]
    for w, h in ((13, 7), (8, 8), (1, 1)):
        got = cr.rays(cam, w, h)
        want = po.rc_camera_rays(_rc_args(po, cam, w, h))
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    got = cr.rays(cam, 13, 7, 2, 5)
    np.testing.assert_array_equal(got.view(np.uint32), cr.rays(cam, 13, 7)[2 * 13:5 * 13].view(np.uint32))


@pytest.mark.parametrize("name", ["rc_cube_x2", "rc_teapot", "rc_teapot_x3", "rc_torus_x2"])
def test_rays_equal_the_reference_goldens(golden, name):
    g = golden(name)
    r = cr.rays(g["cam14"], int(g["width"]), int(g["height"]))
    np.testing.assert_array_equal(r[::5], g["rays"])


def _scene(vrt, golden, name):
    if name == "mirror_hall":
        return scenes.mirror_hall(vrt)
    g = golden(name)
    return {k: g[k] for k in ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")}


# (teapot_x3 and tex_mix have no reflective instance: max_depth > 1 renders what 1 does there, one such case each suffices)
FRAME_CASES = [("mirror_hall", s, d) for s in (0, 1) for d in (1, 2, 3)] + [(n, s, d) for n in ("teapot_x3", "tex_mix") for s in (0, 1) for d in (1, 2)]


@pytest.mark.parametrize("name,shadow,depth", FRAME_CASES)
def test_frame_restatement_equals_render_ex(vrt, po, golden, name, shadow, depth):
    """fed the fixed camera's rays, the restatement reproduces orc_render_ex bit for bit"""
    b = _scene(vrt, golden, name)
    w, h = 40, 24
    p = po.shade_params(max_depth=depth)
    px, hits, col, n = cr.frame_from_rays(b, po.camera_rays(w, h), p, shadow)
    rpx, rhits, rcol, rn = po.render_ex(b, w, h, p, shadow)
    np.testing.assert_array_equal(px, rpx.reshape(-1))
    np.testing.assert_array_equal(col.view(np.uint32), rcol.reshape(-1, 3).view(np.uint32))
    rh = rhits.reshape(-1)
    for k in ("dist", "bx", "by", "bz", "triIdx"):
        np.testing.assert_array_equal(hits[k].view(np.uint32), rh[k].view(np.uint32))
    np.testing.assert_array_equal(hits["blasIdx"] & 0x7fffffff, rh["blasIdx"] & 0x7fffffff)
    assert n == rn
    if name == "mirror_hall" and shadow:
        assert (hits["blasIdx"] >> 31).any()   # some occluded pixels: the shadow path is exercised


def test_library_exports_the_camera_entry_points(vrt):
    lib = C.CDLL(vrt.lib_path("libvortex-hip.so"))
    for s in NEW_SYMBOLS:
        getattr(lib, s)
    hdr = open(os.path.join(ROOT, "include", "vortex_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr), s
    assert "typedef struct vxrt_camera" in hdr


def test_look_at(vrt):
    cam = vrt.rtapi.look_at((0, 0, 10), (0, 0, 0), (0, 1, 0), 45.0, 64, 32)
    c = np.array(cam.cam14(), np.float32)
    f32 = np.float32
    h = f32(2.0) * np.tan(f32(22.5))
    want = np.array([0, 0, 10, 0, 0, -1, 1, 0, 0, 0, 1, 0, h * f32(2.0), h], np.float32)
    np.testing.assert_array_equal(c, want)
    # a tilted view: forward normalised as the reference does (x * (1 / sqrtf(dot)))
    cam = vrt.rtapi.look_at((1, 2, 3), (4, 6, 3), (0, 0, 1), 30.0, 10, 10)
    c = np.array(cam.cam14(), np.float32)
    inv = f32(1.0) / np.sqrt(f32(25.0))
    fwd = np.array([f32(3) * inv, f32(4) * inv, 0], np.float32)
    np.testing.assert_array_equal(c[3:6], fwd)
    r = np.array([fwd[1] * 1 - 0, 0 - fwd[0] * 1, 0], np.float32)   # cross(fwd, (0, 0, 1)), then normalised
    r = r * (f32(1.0) / np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
    np.testing.assert_array_equal(c[6:9], r.astype(np.float32))
    assert c[12] == c[13]


def test_camera_struct_round_trip(vrt):
    v = [float(i) + 0.5 for i in range(14)]
    c = vrt.rtapi.Camera.from_cam14(v)
    assert C.sizeof(c) == 56
    assert c.cam14() == v
