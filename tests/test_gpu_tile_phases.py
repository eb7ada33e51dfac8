"""GPU: whole-tile phases (RT_TILE_PHASES) of the shadow frame kernels that hold the occlusion-only loop.

A wavefront of those kernels takes new jobs only when none of its lanes holds work: the lanes a tile's primary phase leaves idle -- a
pixel that misses, a pixel of the fixed camera's a-priori EXACT list (u == 0 or v == 0), a camera ray deferred out of the fast domain, a
lane outside the window -- stay idle through the tile's occlusion phase.  The parent form handed them the next tile's first primary rays,
and the wavefront held both kinds of ray from then on.  Which lane traces a job never entered a result, so every frame here is the
oracle's, pixel for pixel, hit record for hit record (occlusion bit included), with the oracle's ray count.

The shipped library still refills a wavefront at least half of whose lanes are idle (RT_TILE_REFILL_MIN 32: DESIGN s5 has the
measurement); the variant library of build.py's TEST_VARIANT_FLAGS is built without any partial refill (RT_TILE_REFILL_MIN 65), and it
counts (-DRT_PHASE_COUNT=1): on it every case also reads the phase counts -- passes and node-body runs of the general loop that hold an
any-hit lane are zero, and both pure forms were taken.  That library checks as well (-DRT_OCC_LOOP_CHECK=1): a pass with a primary and
an any-hit ray sets the status word, which every render here asserts to be zero.  The last test runs this file's cases in child
processes on the 8-wavefront kernels, on the variant library, and on both.

Each window is first examined on the CPU, from the oracle's hit mask: it holds a tile with work and an idle lane (the tile that made a
wavefront mixed in the parent form) and, except where the case is "every tile has background", a tile with work and none."""
import os
import subprocess
import sys

import numpy as np
import pytest

import request_programs as rp
from test_gpu_occ_loop import LIGHT_BACK, _params, _tiles_with_hits_and_misses, flat_scene
from test_gpu_parity import _bits, _occlusion_oracle, gpu_render

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATRIUM_LIGHT = (300.0, 480.0, 60.0)
# 64 x 64: the a-priori column x = 32 and row y = 32 are the first of their tiles; 72 x 40 and 40 x 24: x = 36 / 20 and y = 20 / 12 cut
# their tiles in the middle; 70 x 50: the right and bottom tiles hold lanes outside the window
FIXED_SIZES = ((64, 64), (72, 40), (40, 24), (70, 50))
EXPECT_COUNTS = os.environ.get("VXRT_TILE_PHASES_EXPECT_COUNTS") == "1"


def _sync():
    import torch
    torch.cuda.synchronize()


def _counts_reset(vrt):
    """-> does the library count"""
    _sync()
    counting = vrt.rtapi.debug_phase_counts(True) is not None
    assert counting or not EXPECT_COUNTS
    return counting


def _counts_are_pure(vrt, what, occ_form=True):
    """the passes since _counts_reset: none of the general form held an any-hit lane, and both pure forms ran (occ_form: the window
    holds occlusion rays that the main launch traces)"""
    _sync()
    c = vrt.rtapi.debug_phase_counts(True)
    if c is None:
        assert not EXPECT_COUNTS
        return
    print("%s: passes occ %d primary %d mixed %d, node-body runs occ %d primary %d mixed %d" % ((what,) + c))
    assert c[2] == 0 and c[5] == 0, (what, c)
    assert c[1] >= 1 and c[4] >= 1, (what, c)
    if occ_form:
        assert c[0] >= 1 and c[3] >= 1, (what, c)


def _ident_kernels(vrt, ds):
    if os.environ.get("VXRT_IDENT_ROOT") != "0" and os.environ.get("VXRT_SHALLOW") != "0":
        assert vrt.rtapi.accel_info(ds.accel, 5) == 1    # (the identity-root kernels: the ones that hold the occlusion-only loop)


def _tile_kinds(work, idle):
    """per 8 x 8 tile of a window (work, idle: (h, w) masks of the pixels whose lane traces a primary ray in the main launch, and of
    those whose lane stays idle; lanes outside the window are idle): (holds work, holds an idle lane)"""
    h, w = work.shape
    out = []
    for ty in range(0, h, 8):
        for tx in range(0, w, 8):
            a, b = work[ty:ty + 8, tx:tx + 8], idle[ty:ty + 8, tx:tx + 8]
            out.append((bool(a.any()), bool(b.any()) or a.size < 64))
    return out


def _fixed_camera_lanes(w, h, hit_mask):
    """(work, idle) masks of a fixed-camera window: a pixel of the a-priori list never enters the main launch; a lane whose primary ray
    misses is idle through the tile's occlusion phase"""
    ap = np.zeros(((h + 7) // 8) * ((w + 7) // 8) * 64, bool)
    ap[rp.apriori(w, h, 0, h)] = True
    y, x = np.mgrid[0:h, 0:w]
    ap = ap[((y >> 3) * ((w + 7) // 8) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)]
    return hit_mask & ~ap, ~hit_mask | ap


def _has_partial_and_full_tiles(kinds, full=True):
    assert any(a and b for a, b in kinds), kinds         # a tile that leaves lanes idle beside its occlusion rays
    if full:
        assert any(a and not b for a, b in kinds), kinds


class Oracle:
    """the oracle's frames, computed once per (scene, window, light) and left unchanged"""

    def __init__(self, po):
        self.po, self.made = po, {}

    def frame(self, sc, w, h, light):
        key = (sc.name, w, h, tuple(light))
        if key not in self.made:
            pp = self.po.shade_params(light_pos=light)
            rpx, rhits, _, rn = self.po.render_ex(sc, w, h, pp, 1)
            occ, hit = _occlusion_oracle(self.po, sc, w, h, pp, rhits)
            rpx = np.asarray(rpx)
            for a in (rpx, rhits, occ, hit):
                a.setflags(write=False)
            self.made[key] = (rpx, rhits, rn, occ, hit)
        return self.made[key]


@pytest.fixture(scope="module")
def oracle(po):
    return Oracle(po)


@pytest.fixture(scope="module")
def atrium(vrt, gpu_device):
    sc = vrt.scene.procedural("atrium", 5, 0, 3)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    yield sc, ds
    ds.close()


def _frame_equals_oracle(vrt, oracle, sc, ds, w, h, light):
    rpx, rhits, rn, occ, hit = oracle.frame(sc, w, h, light)
    px, hn, _, n = gpu_render(vrt, ds, w, h, shadow=1, params=_params(vrt, light))   # (asserts a zero status word)
    assert np.array_equal(_bits(hn), _bits(rhits)), (sc.name, w, h)
    np.testing.assert_array_equal(gpu_render.occluded, occ)
    assert np.array_equal(px, rpx), (sc.name, w, h)
    assert n == rn
    return occ, hit


@pytest.mark.parametrize("w,h", FIXED_SIZES)
def test_fixed_camera_windows_cut_by_the_a_priori_lines_and_the_window_edge(vrt, oracle, atrium, w, h):
    sc, ds = atrium
    _ident_kernels(vrt, ds)
    hit = oracle.frame(sc, w, h, ATRIUM_LIGHT)[4]
    assert hit.all()                                     # (a closed room: the idle lanes are the a-priori pixels' and the window edge's)
    _has_partial_and_full_tiles(_tile_kinds(*_fixed_camera_lanes(w, h, hit)))
    _counts_reset(vrt)
    occ, _ = _frame_equals_oracle(vrt, oracle, sc, ds, w, h, ATRIUM_LIGHT)
    assert occ.any() and (~occ).any()
    _counts_are_pure(vrt, "atrium %dx%d" % (w, h))


@pytest.mark.parametrize("kind", ["strips", "half"])
def test_frames_with_background(vrt, po, oracle, gpu_device, kind):
    """strips: every tile holds hits and background; half: only the tiles of the lower half do"""
    sc = flat_scene(vrt, po, kind)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    _ident_kernels(vrt, ds)
    w = h = 64
    hit = oracle.frame(sc, w, h, LIGHT_BACK)[4]
    t = _tiles_with_hits_and_misses(hit)
    if kind == "strips":
        assert all(a and b for a, b in t)
    else:
        assert sum(1 for a, b in t if a and not b) >= 16 and sum(1 for a, b in t if a and b) >= 16, t
    _has_partial_and_full_tiles(_tile_kinds(*_fixed_camera_lanes(w, h, hit)), full=kind == "half")
    _counts_reset(vrt)
    occ, _ = _frame_equals_oracle(vrt, oracle, sc, ds, w, h, LIGHT_BACK)
    assert occ.sum() >= 16 and (hit & ~occ).sum() >= 16
    _counts_are_pure(vrt, kind)
    ds.close()


def test_a_caller_camera_frame_with_primary_rays_outside_the_fast_domain(vrt, po, atrium):
    """The fixed camera's pose through the caller-camera kernel at an odd size: the centre column and row hold a zero direction
    component, the main launch defers those rays, and their lanes are idle from the start of their tiles."""
    import torch
    import camera_ref as cr
    import camera_secondary_ref as csr
    from test_gpu_camera import _check, _host_frame, _render_camera
    sc, ds = atrium
    w, h = 71, 41
    cam = np.array((0.0, 100.0, 0.0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 2.0 * w / h, 2.0), np.float32)
    want = cr.frame(sc, cam, w, h, po.shade_params(light_pos=ATRIUM_LIGHT), 1)
    inside = csr.in_fast_domain(cr.rays(cam, w, h)).reshape(h, w)
    hit = (want[1]["dist"] < 1e29).reshape(h, w)
    assert (~inside).sum() == w + h - 1 and (hit & ~inside).any()
    _has_partial_and_full_tiles(_tile_kinds(hit & inside, ~hit | ~inside))
    _counts_reset(vrt)
    got = _host_frame(*_render_camera(vrt, ds, cam, w, h, _params(vrt, ATRIUM_LIGHT), 1), w, h, 0, h)
    assert vrt.rtapi.status(torch.cuda.current_stream().cuda_stream) == 0
    _check(got, want, "atrium through the caller's camera, %d x %d" % (w, h))
    _counts_are_pure(vrt, "caller camera")


def test_a_set_of_three_lights_on_two_streams_equals_the_frames_one_by_one(vrt, po, oracle, gpu_device):
    import torch
    sc = flat_scene(vrt, po, "half")
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    w = h = 64
    lights = (LIGHT_BACK, (-300.0, 100.0, 120.0), (-250.0, 300.0, -90.0))
    plist = [_params(vrt, lp) for lp in lights]
    for lp in lights:
        _frame_equals_oracle(vrt, oracle, sc, ds, w, h, lp)
    assert len({oracle.frame(sc, w, h, lp)[0].tobytes() for lp in lights}) == 3   # (three different frames)
    streams = [torch.cuda.Stream(device=gpu_device) for _ in range(2)]
    bufs = [torch.zeros((3, h, w), dtype=torch.int32, device=gpu_device) for _ in streams]
    _counts_reset(vrt)
    for st, buf in zip(streams, bufs):
        vrt.rtapi.render_batch(ds.accel, w, h, plist, buf.data_ptr(), w * h, 1, None, st.cuda_stream)
    for st in streams:
        st.synchronize()
        assert vrt.rtapi.status(st.cuda_stream) == 0
    _counts_are_pure(vrt, "three lights, two streams")
    for i, lp in enumerate(lights):
        for buf in bufs:
            assert np.array_equal(buf.cpu().numpy().view(np.uint32)[i], oracle.frame(sc, w, h, lp)[0]), i
    ds.close()


def test_a_repeated_frame_runs_the_hinted_kernels(vrt, oracle, gpu_device):
    """The frame, its first repeat (leaves hints) and its second (follows them), on a context of its own: each the oracle's.  No tile
    of this window leaves 32 lanes idle, so every tile's occlusion phase runs in the occlusion-only loop, which writes and follows the
    hints.  The library that counts says so: the frame that is new to its context runs the kernels without hints (nothing counted), the
    first repeat counts its blocked rays, none guided, and leaves a hint for every one of them; in the second repeat most of them stop
    guided (the bound is test_gpu_shadow_hints': at least half) and the occlusion-only loop runs fewer node bodies."""
    from test_gpu_shadow_hints import NONE, _slots
    import torch
    sc = vrt.scene.procedural("atrium", 5, 0, 3)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    w, h = 72, 40
    s = torch.cuda.current_stream().cuda_stream
    occ = oracle.frame(sc, w, h, ATRIUM_LIGHT)[3]
    ap = ~_fixed_camera_lanes(w, h, np.ones((h, w), bool))[0]
    blocked_main = int((occ & ~ap).sum())                # (the a-priori pixels' occlusion rays belong to the EXACT launch)
    counting = _counts_reset(vrt) and vrt.rtapi.debug_shadow_hint_counts(True) is not None
    hints, phases = [], []
    for k in range(3):
        _counts_reset(vrt)
        _frame_equals_oracle(vrt, oracle, sc, ds, w, h, ATRIUM_LIGHT)
        if counting:
            _sync()
            phases.append(vrt.rtapi.debug_phase_counts())
            hints.append(vrt.rtapi.debug_shadow_hint_counts(True, s))
        _counts_are_pure(vrt, "repeat %d" % k)
    if counting:
        left = int((vrt.rtapi.debug_get_shadow_hints(ds.accel, _slots(w, h)[1], s) != NONE).sum())
        print("blocked, guided per frame %r; hints left %d; blocked rays of the main launch %d" % (hints, left, blocked_main))
        assert hints[0] == (0, 0)
        # (every blocked ray the main launch traced left a hint: none of them ran in a mixed pass; a ray deferred to the EXACT launch is not counted)
        assert 1 <= hints[1][0] <= blocked_main and hints[1][1] == 0 and left == hints[1][0]
        assert hints[2][0] == hints[1][0] and left // 2 <= hints[2][1] <= left
        assert phases[2][3] < phases[1][3] == phases[0][3]
    ds.close()


def test_the_eight_wavefront_kernels_and_the_counting_library_pass_the_same_cases(vrt, gpu_device):
    """The 8-wavefront kernels are forced on small frames by VXRT_PACKED=1, read once per process; the counting (and checking) library
    is chosen by VXRT_LIB_DIR, read at import: child processes run this file's other tests with them."""
    if os.environ.get("VXRT_TILE_PHASES_CHILD") == "1":
        return
    d = os.path.join(os.path.dirname(vrt.__file__), "lib_ab", "lds_staging")
    for extra in ({"VXRT_PACKED": "1"}, {"VXRT_LIB_DIR": d, "VXRT_TILE_PHASES_EXPECT_COUNTS": "1"},
                  {"VXRT_LIB_DIR": d, "VXRT_TILE_PHASES_EXPECT_COUNTS": "1", "VXRT_PACKED": "1"}):
        env = dict(os.environ, VXRT_TILE_PHASES_CHILD="1", **extra)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "not eight_wavefront"],
                           env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, "%r\n%s%s" % (extra, r.stdout[-3000:], r.stderr[-2000:])
        print("\n".join(l for l in r.stdout.split("\n") if "passes occ" in l or "blocked, guided" in l))
