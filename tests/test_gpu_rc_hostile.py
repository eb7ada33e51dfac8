"""The twin's kernel (csrc/rc_kernels.hip) against the restatement oracle/rc_oracle.c on the hand-built scenes of tests/rc_cases.py: by-reference
leaves, every wide-node shape, exact distance ties, boxes that switch the build to the two-wide walk or the libstdc++ slab form, lanes outside
the fast domain in the same wavefront as lanes inside it, TLAS shapes, mirror chains, the conversions C leaves undefined; frame widths that are
no multiple of the 8x8 tile, row windows, tiny frames, more streams than frame contexts, the learned tile order under a moving camera.
Pixels exact, colours to the twin's tolerance (rtol 1e-5, tests/test_rc_twin.py) with NaN / +inf / -inf at identical positions; every buffer is
pre-filled with a sentinel.  tests/test_rc_hostile_cpu.py holds the same cases to the reference's own object code."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rc_cases as rcc

pytestmark = pytest.mark.gpu
PX_SENTINEL = 0x5EA7BEEF
COL_SENTINEL = -12345.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def oracle_frames(po):
    """name -> (case, pixels, colours) of the restatement: computed once, shared, left unchanged"""
    memo = {}

    def get(name):
        if name not in memo:
            c = rcc.case(name, po)
            px, col = po.rc_render(rcc.args(po, c))
            px.setflags(write=False)
            col.setflags(write=False)
            memo[name] = (c, px, col)
        return memo[name]
    return get


def _render(vrt, accel, c, dev, y0=None, y1=None, w=None, h=None, stream=None, colors=True, **over):
    """one frame of case c into sentinel-filled buffers -> (pixels [h, w] u32, colours [h, w, 3] f32 or None); enqueued, not synchronised,
    when a torch stream is given"""
    import torch
    w, h = w or c["w"], h or c["h"]
    y0, y1 = 0 if y0 is None else y0, h if y1 is None else y1
    with torch.cuda.stream(stream or torch.cuda.current_stream()):       # (the fills are ordered before the frame on its own stream)
        px = torch.full((h, w), PX_SENTINEL, dtype=torch.int32, device=dev)
        col = torch.full((h * w * 3,), COL_SENTINEL, dtype=torch.float32, device=dev) if colors else None
    prm = vrt.rtapi.rc_params(over.get("cam", c["cam"]), over.get("light", c["light"]), over.get("spp", c["spp"]), over.get("depth", c["depth"]))
    s = (stream or torch.cuda.current_stream()).cuda_stream
    vrt.rtapi.rc_render_accel(accel, w, h, y0, y1, prm, px.data_ptr(), col.data_ptr() if colors else None, s)
    if stream is not None:
        return px, col
    assert vrt.rtapi.status(s) == 0
    return px.cpu().numpy().view(np.uint32), (col.cpu().numpy().reshape(h, w, 3) if colors else None)


def _same_pixels(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d pixels differ, first (y, x) = %s: kernel %08x, oracle %08x" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _same_colours(got, want, what):
    """finite values to rtol 1e-5; NaN, +inf and -inf at identical positions"""
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(f(got), f(want)), "%s: %s at different positions (%d / %d)" % (what, name, f(got).sum(), f(want).sum())
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-5, atol=0, err_msg=what)
    return bool(np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]))


@pytest.mark.parametrize("name", rcc.NAMES)
def test_hostile_case_matches_the_restatement(vrt, po, gpu_device, oracle_frames, name):
    c, opx, ocol = oracle_frames(name)
    ds = vrt.tracer.RcDeviceScene(c["scene"], gpu_device)
    assert vrt.rtapi.rc_accel_info(ds.accel, 0) == c["info"]
    px, col = _render(vrt, ds.accel, c, gpu_device)
    assert not (px == PX_SENTINEL).any() and not (col == COL_SENTINEL).any()
    _same_pixels(px, opx, name)
    bit_equal = _same_colours(col, ocol, name)
    print("%s: colours %s" % (name, "bit-equal" if bit_equal else "within rtol 1e-5"))
    ds.close()


@pytest.mark.parametrize("name", rcc.NAMES)
def test_row_windows_write_their_rows_only(vrt, po, gpu_device, oracle_frames, name):
    c, opx, ocol = oracle_frames(name)
    h = c["h"]
    ds = vrt.tracer.RcDeviceScene(c["scene"], gpu_device)
    for y0, y1 in ((3, 11), (0, 1), (h - 1, h), (17, 17)):
        px, col = _render(vrt, ds.accel, c, gpu_device, y0, y1)          # (an empty window returns 0: rtapi raises on anything else)
        _same_pixels(px[y0:y1], opx[y0:y1], "%s rows [%d, %d)" % (name, y0, y1))
        _same_colours(col[y0:y1], ocol[y0:y1], "%s rows [%d, %d)" % (name, y0, y1))
        out = np.ones(h, bool)
        out[y0:y1] = False
        assert (px[out] == PX_SENTINEL).all() and (col[out] == COL_SENTINEL).all(), (name, y0, y1)
    ds.close()


@pytest.mark.parametrize("name", rcc.NAMES)
def test_tiny_frames(vrt, po, gpu_device, name):
    """1x1, 7x3 and 9x1: fewer pixels than a tile, one tile with idle lanes on two sides, two tiles one row high"""
    c = rcc.case(name, po)
    ds = vrt.tracer.RcDeviceScene(c["scene"], gpu_device)
    for w, h in ((1, 1), (7, 3), (9, 1)):
        opx, ocol = po.rc_render(rcc.args(po, c, w, h))
        px, col = _render(vrt, ds.accel, c, gpu_device, w=w, h=h)
        _same_pixels(px, opx, "%s %dx%d" % (name, w, h))
        _same_colours(col, ocol, "%s %dx%d" % (name, w, h))
    ds.close()


_WALK_CHILD = r"""
import importlib, sys
import numpy as np
sys.path[:0] = [%r, %r]
import torch
import rc_cases as rcc
from oracle import pyoracle as po
vrt = importlib.import_module("vortex-raytracing_amd")
out, s = {}, torch.cuda.current_stream().cuda_stream
for name in rcc.NAMES:
    c = rcc.case(name, po)
    ds = vrt.tracer.RcDeviceScene(c["scene"], "cuda:0")
    px = torch.full((c["h"], c["w"]), 0x5EA7BEEF, dtype=torch.int32, device="cuda:0")
    vrt.rtapi.rc_render_accel(ds.accel, c["w"], c["h"], 0, c["h"], vrt.rtapi.rc_params(c["cam"], c["light"], c["spp"], c["depth"]), px.data_ptr(), None, s)
    assert vrt.rtapi.status(s) == 0, name
    out[name] = px.cpu().numpy().view(np.uint32)
    out["info_" + name] = np.array(vrt.rtapi.rc_accel_info(ds.accel, 0))
    ds.close()
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("setting", ["VXRC_WIDE=0", "VXRC_LPT=0"])
def test_walk_variants_give_the_same_frames(vrt, po, gpu_device, oracle_frames, tmp_path, setting):
    """the whole case table in a fresh process (both switches are read once per process) with the wide walk / the learned tile order off:
    pixels identical to the default run's, which the test above holds to the restatement"""
    key, val = setting.split("=")
    out = str(tmp_path / "frames.npz")
    r = subprocess.run([sys.executable, "-c", _WALK_CHILD % (ROOT, os.path.join(ROOT, "tests")), out], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=dict(os.environ, **{key: val}))
    assert r.returncode == 0, (setting, r.stdout[-2000:], r.stderr[-2000:])
    with np.load(out) as z:
        for name in rcc.NAMES:
            c, opx, _ = oracle_frames(name)
            ds = vrt.tracer.RcDeviceScene(c["scene"], gpu_device)
            px, _ = _render(vrt, ds.accel, c, gpu_device, colors=False)
            ds.close()
            _same_pixels(z[name], px, "%s with %s against the default run" % (name, setting))
            assert int(z["info_" + name]) == (0 if key == "VXRC_WIDE" else c["info"]), name


def test_more_streams_than_frame_contexts(vrt, po, gpu_device):
    """one layout, 10 frames issued round robin on 5 streams -- one more than the layout has frame contexts, so every fifth frame takes a
    context another stream's frame still holds -- with the camera, samples, depth, frame size and window changing from frame to frame"""
    import torch
    c = rcc.case("mirrors_d3_s3", po)
    ds = vrt.tracer.RcDeviceScene(c["scene"], gpu_device)
    ds.accel
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=gpu_device) for _ in range(5)]
    jobs = []
    for k in range(10):
        w, h = ((97, 61), (203, 131), (64, 40))[k % 3]
        cam = rcc.cam_tilted(w, h, pos=(0.0 + 3 * k, 100.0 - 2 * k, 1.5 * k), yaw=0.05 - 0.02 * k, pitch=0.01 * k)
        y0, y1 = ((0, h), (5, h - 9), (h // 2, h))[k % 3] if k % 2 else (0, h)
        over = {"cam": cam, "spp": 1 + k % 3, "depth": 1 + k % 6}
        px, col = _render(vrt, ds.accel, c, gpu_device, y0, y1, w, h, stream=streams[k % 5], **over)
        jobs.append((k, w, h, y0, y1, over, px, col))
    torch.cuda.synchronize()
    for s in streams:
        assert vrt.rtapi.status(s.cuda_stream) == 0
    for k, w, h, y0, y1, over, px, col in jobs:
        opx, ocol = po.rc_render(rcc.args(po, c, w, h, **over), y0, y1)
        got, gcol = px.cpu().numpy().view(np.uint32), col.cpu().numpy().reshape(h, w, 3)
        _same_pixels(got[y0:y1], opx[y0:y1], "frame %d" % k)
        _same_colours(gcol[y0:y1], ocol[y0:y1], "frame %d" % k)
        out = np.ones(h, bool)
        out[y0:y1] = False
        assert (got[out] == PX_SENTINEL).all() and (gcol[out] == COL_SENTINEL).all(), k
    ds.close()


def test_learned_tile_order_under_a_moving_camera(vrt, po, gpu_device):
    """512 x 520 = 4,160 tiles, the smallest convenient frame above the 4,096 tiles from which a context learns the order of its next frame
    from the cost of its last: three frames on one stream with a different camera each (the order learned for one view is used for the next),
    then another window (the order is dropped) -- every frame exact against the restatement"""
    c = rcc.case("tlas_33", po)
    w, h = 512, 520
    ds = vrt.tracer.RcDeviceScene(c["scene"], gpu_device)
    frames = [(rcc.cam_tilted(w, h), 0, h), (rcc.cam_tilted(w, h, pos=(8.0, 95.0, -20.0), yaw=0.3, pitch=0.05), 0, h),
              (rcc.cam_axis(w, h, pos=(-30.0, 110.0, 25.0)), 0, h), (rcc.cam_tilted(w, h, yaw=-0.2), 16, h - 24)]
    for k, (cam, y0, y1) in enumerate(frames):
        opx, ocol = po.rc_render_mt(rcc.args(po, c, w, h, cam=cam))
        px, col = _render(vrt, ds.accel, c, gpu_device, y0, y1, w, h, cam=cam)
        _same_pixels(px[y0:y1], opx[y0:y1], "frame %d" % k)
        _same_colours(col[y0:y1], ocol[y0:y1], "frame %d" % k)
        assert (px[:y0] == PX_SENTINEL).all() and (px[y1:] == PX_SENTINEL).all() and (col[:y0] == COL_SENTINEL).all() and (col[y1:] == COL_SENTINEL).all()
        assert 0.02 < (opx != opx[0, 0]).mean()
    ds.close()
