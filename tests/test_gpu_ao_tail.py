"""GPU: the tail of an ambient-occlusion frame (render_ao_tail, csrc/rt_secondary.hip) where no other test takes it -- more than one
batch of samples, a short last batch, sample counts around and above one wavefront up to the header's 4096, row windows, frames
without a single hit -- in both camera forms, against the restatements the unbatched frames are held to:

  camera form (vxrt_render_ao_camera)   camera_secondary_ref.ao_frame: unoccluded counts, colours as u32, pixels, rays traced, all equal
  fixed camera (vxrt_render_ao)         pyoracle.render_ao: what test_ambient_occlusion_pass_matches_oracle asserts -- counts, rays traced
                                        and pixels equal, colours within its COLOR_RTOL

The cases and their references are tests/ao_tail_cases.py's; tests/test_ao_tail_cpu.py shows that they are not vacuous.  Output
buffers are marker-filled, vxrt_status is 0 after every frame.

The batch size (VXRT_AO_BATCH, rays) is read once per process, with the other knobs of the secondary tails: the batched tests run
their bodies in a fresh child process each, as test_batches_of_two_two_and_one_samples (tests/test_gpu_path.py) does, with VXRT_DEBUG
set so that the child's line "[vxrt] secondary knobs: ..." shows the parent the values the library took.  The secondary-ray sort
(VXRT_SORT_SECONDARY=1) goes through this file's in-process tests from tests/test_gpu_variants.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ao_tail_cases as atc

pytestmark = pytest.mark.gpu
MARK, OPEN_MARK = 0x5A5A5A, 0x7777
COLOR_RTOL = 1e-5     # (tests/test_gpu_parity.py's: the fixed-camera form's colours)
CHILD = os.environ.get("VXRT_AO_TAIL_TEST_CHILD", "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _outputs(dev, w, h):
    """pixels, colours, unoccluded counts (marker-filled) and the ray counter of a w x h frame"""
    import torch
    return (torch.full((h, w), MARK, dtype=torch.int32, device=dev), torch.full((h * w * 3,), -1.0, dtype=torch.float32, device=dev),
            torch.full((h, w), OPEN_MARK, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def _read(out, w, h):
    import torch
    torch.cuda.synchronize()
    px, col, opn, cnt = out
    return px.cpu().numpy().view(np.uint32), col.cpu().numpy().reshape(h, w, 3), opn.cpu().numpy().view(np.uint32), int(cnt.item())


def _untouched_outside(px, col, opn, case, what):
    for a, mark in ((px, MARK), (col, np.float32(-1.0)), (opn, OPEN_MARK)):
        assert (a[:case.y0] == mark).all() and (a[case.y1:] == mark).all(), what + ": rows outside the window were written"


def _camera_form(vrt, po, ds, case, what=""):
    what = "%s camera form %s" % (case.name, what)
    out = _outputs(ds.t["tri"].device, case.w, case.h)
    vrt.rtapi.render_ao_camera(ds.accel, atc.camera(vrt, case), case.w, case.h, case.y0, case.y1, vrt.rtapi.default_shade_params(), case.spp, atc.RADIUS,
                               out[0].data_ptr(), atc.SEED, out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), _stream())
    px, col, opn, n = _read(out, case.w, case.h)
    assert vrt.rtapi.status(_stream()) == 0, what
    (rpx, rcol, ropn, rn), _ = atc.camera_reference(vrt, po, case)
    w = slice(case.y0, case.y1)
    np.testing.assert_array_equal(opn[w], ropn, err_msg=what + ": unoccluded")
    np.testing.assert_array_equal(col[w].view(np.uint32), rcol.view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(px[w], rpx, err_msg=what + ": pixels")
    assert n == rn, "%s: rays traced %d, restatement %d" % (what, n, rn)
    _untouched_outside(px, col, opn, case, what)


def _fixed_form(vrt, po, ds, case, what=""):
    what = "%s fixed camera %s" % (case.name, what)
    out = _outputs(ds.t["tri"].device, case.w, case.h)
    p = vrt.rtapi.default_shade_params()
    p.light_pos[:] = atc.FIXED_LIGHT
    vrt.rtapi.render_ao(ds.accel, case.w, case.h, case.y0, case.y1, p, case.spp, atc.FIXED_RADIUS, out[0].data_ptr(), seed=atc.SEED, colors_ptr=out[1].data_ptr(),
                        unoccluded_ptr=out[2].data_ptr(), rays_ptr=out[3].data_ptr(), stream=_stream())
    px, col, opn, n = _read(out, case.w, case.h)
    assert vrt.rtapi.status(_stream()) == 0, what
    rpx, rcol, ropn, rn = atc.fixed_reference(vrt, po, case)
    w = slice(case.y0, case.y1)
    np.testing.assert_array_equal(opn[w], ropn[w], err_msg=what + ": unoccluded")
    assert n == rn, "%s: rays traced %d, oracle %d" % (what, n, rn)
    np.testing.assert_allclose(col[w], rcol[w], rtol=COLOR_RTOL, err_msg=what + ": colours")
    np.testing.assert_array_equal(px[w], rpx[w], err_msg=what + ": pixels")
    _untouched_outside(px, col, opn, case, what)


def _both_forms(vrt, po, ds, name, what=""):
    _camera_form(vrt, po, ds, atc.BY_NAME[name], what)
    _fixed_form(vrt, po, ds, atc.BY_NAME[name], what)


@pytest.fixture(scope="module")
def hall(vrt, gpu_device):
    ds = vrt.tracer.DeviceScene(atc.hall(vrt), gpu_device)
    yield ds
    ds.close()


# ---- in process: the knobs the process was started with (none, unless tests/test_gpu_variants.py started it) ----
@pytest.mark.parametrize("name", atc.SAMPLE_COUNTS)
def test_in_process_sample_counts(vrt, po, hall, name):
    _both_forms(vrt, po, hall, name)


@pytest.mark.parametrize("name", atc.ROW_WINDOWS)
def test_in_process_row_windows(vrt, po, hall, name):
    _both_forms(vrt, po, hall, name)


def test_in_process_all_miss_then_a_normal_frame(vrt, po, hall):
    """no pixel of the first frame has a hit: hdr[0] = 0 and every launch of the tail runs on zero live rays; the context then
    renders a normal frame"""
    (_, _, _, rn), fi = atc.camera_reference(vrt, po, atc.BY_NAME["all_miss"])
    assert len(fi) == 0 and rn == 40 * 24
    _camera_form(vrt, po, hall, atc.BY_NAME["all_miss"])
    _both_forms(vrt, po, hall, "spp7", "after the all-miss frame")


@pytest.mark.parametrize("name", atc.LARGE_WINDOWS)
def test_large_windows(vrt, po, hall, name):
    """windows of more than 128 cells of 16 x 16 pixels: with the secondary-ray sort, its scan takes 2 and 3 counters per thread"""
    case = atc.BY_NAME[name]
    assert (8 * atc.n_cells(case) + 1023) // 1024 == {"cells143": 2, "cells272": 3}[name]
    _both_forms(vrt, po, hall, name)


# ---- batched: a fresh child process per batch size ----
def _run_child(mode, rays_per_batch, select):
    env = dict(os.environ, VXRT_AO_BATCH=str(rays_per_batch), VXRT_AO_TAIL_TEST_CHILD=mode, VXRT_DEBUG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", select],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and ("ao_batch=%d " % rays_per_batch) in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]   # the knob reached the library


def test_batches_of_2880_rays(vrt, po, hall):
    """VXRT_AO_BATCH=2880 in a child process.  40 x 24 at 7 spp takes batches of 3, 3 and 1 samples; 13 x 7 at 65 spp 31, 31 and 3, so
    that pixel segments straddle wavefronts in a short last batch whose launches stay sized for 31; the row window 3 and 2; the
    one-row window 72 and 58.  Then a small frame behind a larger one on the same context (the hit records of the larger frame lie
    behind the live ones), and the frame without a hit followed by a normal one."""
    if CHILD != "batch2880":
        if not CHILD:
            _run_child("batch2880", 2880, "batches_of_2880")
        return
    assert os.environ["VXRT_AO_BATCH"] == "2880"
    for name, want in (("spp7", [3, 3, 1]), ("small65", [31, 31, 3]), ("rows", [3, 2]), ("one_row", [72, 58])):
        assert atc.batches(atc.BY_NAME[name], 2880) == want
    for name in ("spp7", "small65", "rows", "one_row", "spp65"):
        _both_forms(vrt, po, hall, name, "2880 rays per batch")
    _both_forms(vrt, po, hall, "spp7", "2880 rays per batch, the larger frame")            # 2,880 rays per batch ...
    _both_forms(vrt, po, hall, "one_row", "2880 rays per batch, behind the larger frame")  # ... then 2,880 and 2,320 of the same buffers
    _both_forms(vrt, po, hall, "small65", "2880 rays per batch, behind the larger frame")  # 2,821, 2,821 and 273
    _camera_form(vrt, po, hall, atc.BY_NAME["all_miss"], "2880 rays per batch")
    _both_forms(vrt, po, hall, "spp7", "2880 rays per batch, after the all-miss frame")


def test_one_sample_per_batch(vrt, po, hall):
    """VXRT_AO_BATCH=1 in a child process: ns = 1, one batch per sample, at 7 and 16 spp"""
    if CHILD != "batch1":
        if not CHILD:
            _run_child("batch1", 1, "one_sample_per_batch")
        return
    assert os.environ["VXRT_AO_BATCH"] == "1"
    for name in ("spp7", "spp16"):
        assert atc.batches(atc.BY_NAME[name], 1) == [1] * atc.BY_NAME[name].spp
        _both_forms(vrt, po, hall, name, "one ray per batch")
