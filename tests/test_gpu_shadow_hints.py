"""GPU: shadow hints (RT_SHADOW_HINTS) choose a visiting order and nothing else.

A timed shadow frame of an accel that holds a path table, when it REPEATS the frame its context rendered last (same window, light,
camera, no refit), keeps per hit-record slot the triangle that blocked the slot's occlusion ray; the next repeat lets that ray descend
towards the triangle first.  Any other frame runs without hints.  Whatever the hint words hold -- the frame before, nothing, garbage --
pixels, hit records and the occlusion bit (bit 31 of blasIdx) are the oracle's, and the rays counter is the same.

Frames are 64 x 48 and 70 x 50 (partial tiles at the right and bottom edges).  The atrium (levels 3 and 4) is seen by the fixed camera with
the headline's light: every pixel hits, and the frame has tiles whose occlusion rays are all blocked, tiles where some are and tiles where
none is (the fixture checks that).  The golden teapot is seen by a caller's camera from close by (the caller-camera kernel): the same three
kinds of tiles, and tiles with background beside them, whose wavefronts keep the general loop."""
import os

import numpy as np
import pytest

from test_gpu_parity import _occlusion_oracle

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (70, 50))
ATRIUM_LIGHT = (300.0, 480.0, 60.0)
TEAPOT_EYE, TEAPOT_LIGHT = (0.9, 0.5, 0.0), (0.0, 2.0, 2.0)
CASES = [(name, w, h) for name in ("atrium3", "atrium4", "teapot") for w, h in SIZES]
NONE = 0xFFFFFFFF


def _params(vrt, light):
    p = vrt.rtapi.default_shade_params()
    p.light_pos[:] = light
    return p


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _render(vrt, ds, cam, w, h, params, stream=None):
    """one shadow frame -> (pixels u32 (h, w), raw hit records as bytes (h * w, 24): the occlusion bit included, rays traced)"""
    import torch
    dev = ds.t["tri"].device
    s = _stream() if stream is None else stream
    px = torch.full((h, w), 0x5A5A5A, dtype=torch.int32, device=dev)
    hits = torch.zeros(h * w * 24, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    if cam is None:
        vrt.rtapi.render(ds.accel, w, h, 0, h, params, px.data_ptr(), 1, hits.data_ptr(), None, cnt.data_ptr(), s)
    else:
        vrt.rtapi.render_camera(ds.accel, cam, w, h, 0, h, params, px.data_ptr(), 1, hits.data_ptr(), None, cnt.data_ptr(), s)
    assert vrt.rtapi.status(s) == 0
    return px.cpu().numpy().view(np.uint32), hits.cpu().numpy().reshape(h * w, 24), int(cnt.item())


def _slots(w, h):
    """hit-record slot of every pixel of a w x h frame (tile-major), and the number of slots"""
    tx = (w + 7) // 8
    y, x = np.mgrid[0:h, 0:w]
    return (((y >> 3) * tx + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)).astype(np.int64), tx * ((h + 7) // 8) * 64


def _tile_kinds(occ, hit):
    """tiles all of whose pixels hit, by their occlusion rays: all blocked, some, none"""
    h, w = occ.shape
    full = mixed = none = 0
    for ty in range(0, h, 8):
        for tx in range(0, w, 8):
            o, m = occ[ty:ty + 8, tx:tx + 8], hit[ty:ty + 8, tx:tx + 8]
            if m.all():
                full, mixed, none = full + bool(o.all()), mixed + bool(o.any() and not o.all()), none + bool(not o.any())
    return full, mixed, none


class Case:
    """scene, device scene, camera and the oracle's frame of one case; built once per module"""

    def __init__(self, vrt, po, golden, dev, name, w, h):
        import camera_ref as cr
        from oracle.pyoracle import HIT_DTYPE
        self.w, self.h = w, h
        if name == "teapot":
            self.sc, self.light = golden("teapot"), TEAPOT_LIGHT
            self.cam = np.array(vrt.rtapi.look_at(TEAPOT_EYE, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32)
            rpx, rhits, _, self.rays = cr.frame(self.sc, self.cam, w, h, po.shade_params(light_pos=self.light), 1)
            rhits = rhits.copy()
        else:
            self.sc, self.light, self.cam = vrt.scene.procedural("atrium", int(name[-1]), 0, 3), ATRIUM_LIGHT, None
            pp = po.shade_params(light_pos=self.light)
            rpx, rhits, _, self.rays = po.render_ex(self.sc, w, h, pp, 1)
            occ, _ = _occlusion_oracle(po, self.sc, w, h, pp, rhits)
            rhits = rhits.copy().reshape(h, w)
            rhits["blasIdx"] |= occ.astype(np.uint32) << 31
        self.px = np.asarray(rpx, np.uint32).reshape(h, w)
        self.hits = np.ascontiguousarray(rhits).view(HIT_DTYPE).reshape(h * w)
        self.occ = (self.hits["blasIdx"] >> 31).astype(bool).reshape(h, w)
        self.hit = (self.hits["dist"] < 1e29).reshape(h, w)
        self.n_tris = self.sc["tri"].size // 36
        self.ds = vrt.tracer.DeviceScene(self.sc, dev)
        self.params = _params(vrt, self.light)
        self.used = False                                # a test has rendered on the device scene's context

    def equals_oracle(self, got, what):
        px, hits, n = got
        assert np.array_equal(px, self.px), what
        assert np.array_equal(hits, self.hits.view(np.uint8).reshape(-1, 24)), what
        assert n == self.rays, what


@pytest.fixture(scope="module")
def cases(vrt, po, golden, gpu_device):
    made = {}

    def get(name, w, h):
        if (name, w, h) not in made:
            made[(name, w, h)] = Case(vrt, po, golden, gpu_device, name, w, h)
        return made[(name, w, h)]

    yield get
    for c in made.values():
        c.ds.close()


@pytest.mark.parametrize("name,w,h", CASES)
def test_repeats_of_a_frame_equal_the_first_the_oracle_and_hints_off(vrt, cases, name, w, h):
    c = cases(name, w, h)
    full, mixed, none = _tile_kinds(c.occ, c.hit)
    assert full >= 1 and mixed >= 1 and none >= 1, (full, mixed, none)
    assert vrt.rtapi.accel_info(c.ds.accel, 5) == 1 and vrt.rtapi.accel_info(c.ds.accel, 9) == 1
    slots, n = _slots(w, h)
    c.equals_oracle(_render(vrt, c.ds, c.cam, w, h, c.params), "the frame, new to the context: without hints")
    first = _render(vrt, c.ds, c.cam, w, h, c.params)
    c.equals_oracle(first, "first repeat: from no hints, leaves its own")
    if c.used:                                           # (another test's hints: start from none, as a new context does)
        vrt.rtapi.debug_set_shadow_hints(c.ds.accel, np.full(n, NONE, np.uint32), _stream())
        c.equals_oracle(_render(vrt, c.ds, c.cam, w, h, c.params), "first frame again")
    c.used = True
    # what a frame without hints leaves: hints only where the occlusion ray was blocked, each naming a triangle
    hints = vrt.rtapi.debug_get_shadow_hints(c.ds.accel, n, _stream())[slots]
    assert not (hints[~c.occ] != NONE).any()
    assert (hints[hints != NONE] < c.n_tris).all()
    # Which blocked pixels have one depends on how the tiles met the wavefronts: a wavefront writes hints for a tile whose lanes turned to
    # their occlusion rays together (the occlusion-only loop).  One that was handed part of a tile -- behind a tile with lanes outside the
    # frame, with background, or with a pixel the EXACT launch traces (u == 0 or v == 0) -- holds both kinds of rays from then on and keeps
    # the general loop, which knows no hints.  So: some, not all.
    print("%s %dx%d: %d of %d blocked pixels left a hint" % (name, w, h, int((hints != NONE).sum()), int(c.occ.sum())))
    if c.cam is None:
        assert c.hit.all() and (hints != NONE).sum() >= 1
    second = _render(vrt, c.ds, c.cam, w, h, c.params)
    c.equals_oracle(second, "second repeat: on the first one's hints")
    # hints off (what VXRT_SHADOW_HINTS=0 does, switched inside this process): the same frame, and no hint word read or written -- the words
    # are a marker before and after
    marker = np.full(n, 7, np.uint32)
    vrt.rtapi.debug_set_shadow_hints(c.ds.accel, marker, _stream())
    vrt.rtapi.debug_shadow_hints_enable(0)
    try:
        off = _render(vrt, c.ds, c.cam, w, h, c.params)
    finally:
        vrt.rtapi.debug_shadow_hints_enable(-1)
    assert np.array_equal(vrt.rtapi.debug_get_shadow_hints(c.ds.accel, n, _stream()), marker)
    c.equals_oracle(off, "VXRT_SHADOW_HINTS=0")


HOSTILE = ("none", "zero", "last", "count", "count_plus_1", "random", "one_far_triangle", "mirrored")


@pytest.mark.parametrize("kind", HOSTILE)
@pytest.mark.parametrize("name,w,h", [("atrium4", 70, 50), ("teapot", 64, 48)])
def test_hostile_hints_give_the_same_bits(vrt, cases, name, w, h, kind):
    c = cases(name, w, h)
    slots, n = _slots(w, h)
    # the frame's own hints: the frame, its first repeat (the context holds hints from here on), no hints (another case's words may still
    # be there), the frame again
    c.equals_oracle(_render(vrt, c.ds, c.cam, w, h, c.params), "the frame")
    c.equals_oracle(_render(vrt, c.ds, c.cam, w, h, c.params), "its first repeat")
    c.used = True
    vrt.rtapi.debug_set_shadow_hints(c.ds.accel, np.full(n, NONE, np.uint32), _stream())
    c.equals_oracle(_render(vrt, c.ds, c.cam, w, h, c.params), "the frame that leaves hints")
    real = vrt.rtapi.debug_get_shadow_hints(c.ds.accel, n, _stream())
    assert ((real == NONE) | (real < c.n_tris)).all()
    if kind == "random":
        words = np.random.default_rng(17).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    elif kind == "one_far_triangle":
        # the triangle farthest from the middle of the blockers the frame found
        tri = c.sc["tri"].view(np.float32).reshape(-1, 3, 3).mean(1)
        mid = tri[real[real != NONE]].mean(0)
        words = np.full(n, int(np.argmax(((tri - mid) ** 2).sum(1))), np.uint32)
    elif kind == "mirrored":
        grid = real[slots]
        words = np.full(n, NONE, np.uint32)
        words[slots] = grid[:, ::-1]
        assert (words != real).any()
    else:
        words = np.full(n, {"none": NONE, "zero": 0, "last": c.n_tris - 1, "count": c.n_tris, "count_plus_1": c.n_tris + 1}[kind], np.uint32)
    vrt.rtapi.debug_set_shadow_hints(c.ds.accel, words, _stream())
    assert np.array_equal(vrt.rtapi.debug_get_shadow_hints(c.ds.accel, n, _stream()), words)
    c.equals_oracle(_render(vrt, c.ds, c.cam, w, h, c.params), kind)


def test_a_batch_of_five_lights_on_two_streams_equals_the_frames_one_by_one(vrt, cases, gpu_device):
    import torch
    c = cases("atrium4", 70, 50)
    w, h = c.w, c.h
    lights = [ATRIUM_LIGHT, (300.0, 300.0, 60.0), (200.0, 150.0, 100.0), (400.0, 100.0, -50.0), (120.0, 420.0, -80.0)]
    plist = [_params(vrt, lp) for lp in lights]
    ones = [_render(vrt, c.ds, None, w, h, p)[0] for p in plist]
    c.used = True
    assert len({o.tobytes() for o in ones}) == 5
    vrt.rtapi.accel_frames_in_flight(c.ds.accel, 2)
    try:
        streams = [torch.cuda.Stream(device=gpu_device) for _ in range(2)]
        bufs = [torch.zeros((5, h, w), dtype=torch.int32, device=gpu_device) for _ in range(8)]
        torch.cuda.synchronize()
        # four sets per stream (each stream keeps its context): the set, its first repeat (leaves hints), its second (follows them), then
        # the lights in reverse order -- another set: without hints
        order = lambda k: plist if k < 6 else plist[::-1]
        for k, buf in enumerate(bufs[:6]):
            vrt.rtapi.render_batch(c.ds.accel, w, h, order(k), buf.data_ptr(), w * h, 1, None, streams[k % 2].cuda_stream)
        for st in streams:                               # (each context holds the hints of five frames: blockers under five lights)
            left = vrt.rtapi.debug_get_shadow_hints(c.ds.accel, 5 * _slots(w, h)[1], st.cuda_stream)
            assert all((left[f * _slots(w, h)[1]:(f + 1) * _slots(w, h)[1]] != NONE).sum() >= 1 for f in range(5))
        for k, buf in enumerate(bufs[6:], 6):
            vrt.rtapi.render_batch(c.ds.accel, w, h, order(k), buf.data_ptr(), w * h, 1, None, streams[k % 2].cuda_stream)
        for st in streams:
            st.synchronize()
            assert vrt.rtapi.status(st.cuda_stream) == 0
        for k, buf in enumerate(bufs):
            got = buf.cpu().numpy().view(np.uint32)
            for i in range(5):
                assert np.array_equal(got[i], ones[i] if k < 6 else ones[4 - i]), (k, i)
    finally:
        torch.cuda.synchronize()
        vrt.rtapi.accel_frames_in_flight(c.ds.accel, 1)


def test_hinted_frames_after_a_refit_that_moves_vertices_equal_a_fresh_accels(vrt, gpu_device):
    import torch
    sc = vrt.scene.procedural("atrium", 4, 0, 3)
    ds = vrt.tracer.DeviceScene(sc, gpu_device)
    w, h = 70, 50
    p = _params(vrt, ATRIUM_LIGHT)
    n = _slots(w, h)[1]
    for _ in range(3):
        _render(vrt, ds, None, w, h, p)                  # the frame and two repeats: the context holds hints of the scene as built
    before = vrt.rtapi.debug_get_shadow_hints(ds.accel, n, _stream())
    assert (before != NONE).sum() >= 64
    tri = ds.t["tri"].view(torch.float32)
    i = torch.arange(tri.numel(), device=tri.device, dtype=torch.float32)
    tri.add_(3.0 * torch.sin(i * 0.37))                  # every vertex moves by up to 3 units: other blockers for many pixels
    ds.refit(geometry=True)
    assert vrt.rtapi.accel_info(ds.accel, 9) == 1        # (topology kept: the table stays)
    marker = np.full(n, 7, np.uint32)
    vrt.rtapi.debug_set_shadow_hints(ds.accel, marker, _stream())
    stale = _render(vrt, ds, None, w, h, p)              # the same request, another scene: without hints, the old words untouched
    assert np.array_equal(vrt.rtapi.debug_get_shadow_hints(ds.accel, n, _stream()), marker)
    _render(vrt, ds, None, w, h, p)                      # first repeat: from none
    assert (vrt.rtapi.debug_get_shadow_hints(ds.accel, n, _stream()) == 7).sum() == 0
    again = _render(vrt, ds, None, w, h, p)              # second repeat: on the moved scene's own hints
    fresh_ds = vrt.tracer.DeviceScene({k: ds.t[k].cpu().numpy().copy() for k in ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")}, gpu_device)
    fresh = _render(vrt, fresh_ds, None, w, h, p)
    occ = (fresh[1].view(np.uint32).reshape(-1, 6)[:, 4] >> 31).astype(bool)
    assert occ.sum() >= 64 and (~occ).sum() >= 64
    for got, what in ((stale, "first frame after the refit"), (again, "own hints")):
        assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1]) and got[2] == fresh[2], what
    fresh_ds.close()
    ds.close()


def test_scenes_without_a_table_render_as_before(vrt, po, gpu_device):
    """Several instances, and a single instance deeper than 16 levels: no table, the general kernels or the full-size stacks, the oracle's frames."""
    from test_gpu_occ_loop import BEHIND, SIDE, _shadow_frame_equals_oracle, tilted_chain, two_instance_scene
    from test_gpu_stack_push import _tree_scene
    tris = []
    root = tilted_chain((1,) * 20, tris)
    for sc, light in ((two_instance_scene(vrt), SIDE), (_tree_scene(vrt, root, tris, "chain_20_levels"), BEHIND)):
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        assert vrt.rtapi.accel_info(ds.accel, 9) == 0, sc.name
        if sc.name == "chain_20_levels":
            assert vrt.rtapi.accel_info(ds.accel, 0) > 16
        for w, h in SIZES:
            for _ in range(2):
                _shadow_frame_equals_oracle(vrt, po, sc, ds, w, h, light)
        with pytest.raises(vrt.runtime.VxError):
            vrt.rtapi.debug_get_shadow_hints(ds.accel, 1, _stream())
        ds.close()


def _count_guided_rays():
    """child process, on a library that counts (-DRT_SHADOW_HINT_COUNT=1): blocked rays and rays blocked while guided, frame by frame"""
    import importlib
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    vrt = importlib.import_module("vortex-raytracing_amd")
    sc = vrt.scene.procedural("atrium", 4, 0, 3)
    ds = vrt.tracer.DeviceScene(sc, "cuda:0")
    w, h, p, out = 70, 50, _params(vrt, ATRIUM_LIGHT), []
    assert vrt.rtapi.debug_shadow_hint_counts(True) is not None
    s = torch.cuda.current_stream().cuda_stream
    for k, on in enumerate((1, 1, 1, 0)):
        vrt.rtapi.debug_shadow_hints_enable(on)
        _render(vrt, ds, None, w, h, p)
        out.append(vrt.rtapi.debug_shadow_hint_counts(True, s))
        if k == 1:                                       # the hints the first repeat left
            out.append((int((vrt.rtapi.debug_get_shadow_hints(ds.accel, _slots(w, h)[1], s) != NONE).sum()), 0))
    ds.close()
    print("COUNTS %r" % (out,))


def test_the_second_repeat_takes_guided_steps_to_its_blockers(vrt):
    """The variant library counts (build.py's TEST_VARIANT_FLAGS).  The frame, new to its context: the kernels without hints, which count
    nothing.  First repeat: blocked rays, none guided; it leaves H hints.  Second repeat: every ray that holds a hint follows its own
    blocker's path -- each hinted box holds the blocker, so no hinted slot fails and nothing is popped before the blocker's leaf -- and stops
    guided, if its wavefront takes the occlusion-only loop again (which do depends on how tiles meet wavefronts, see above: 93 % did when
    this was written).  At least half of H, at most H.  Then hints off: nothing counted."""
    import ast
    import subprocess
    import sys
    d = os.path.join(os.path.dirname(vrt.__file__), "lib_ab", "lds_staging")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, VXRT_LIB_DIR=d), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new, first, left, second, off = ast.literal_eval([l for l in r.stdout.split("\n") if l.startswith("COUNTS ")][-1][7:])
    print("blocked, guided: new frame %r, first repeat %r (%d hints left), second repeat %r, hints off %r" % (new, first, left[0], second, off))
    assert new == (0, 0)
    assert first[0] >= 1000 and first[1] == 0 and 500 <= left[0] <= first[0]
    assert second[0] == first[0] and left[0] // 2 <= second[1] <= left[0]
    assert off == (0, 0)


def test_a_frame_under_another_light_runs_without_hints(vrt, cases):
    """The hint words are handed to repeats only.  The same window under another light: the frame equals its hints-off frame and leaves a
    marker in every hint word untouched; back under the first light: again without hints (the context's last frame was the other one)."""
    c = cases("atrium4", 64, 48)
    w, h = c.w, c.h
    n = _slots(w, h)[1]
    other = _params(vrt, (200.0, 150.0, 100.0))
    for _ in range(2):
        c.equals_oracle(_render(vrt, c.ds, None, w, h, c.params), "the frame and its first repeat")
    c.used = True
    marker = np.full(n, 7, np.uint32)
    vrt.rtapi.debug_set_shadow_hints(c.ds.accel, marker, _stream())
    moved = _render(vrt, c.ds, None, w, h, other)
    assert np.array_equal(vrt.rtapi.debug_get_shadow_hints(c.ds.accel, n, _stream()), marker)
    c.equals_oracle(_render(vrt, c.ds, None, w, h, c.params), "back under the first light")
    assert np.array_equal(vrt.rtapi.debug_get_shadow_hints(c.ds.accel, n, _stream()), marker)
    vrt.rtapi.debug_shadow_hints_enable(0)
    try:
        off = _render(vrt, c.ds, None, w, h, other)
    finally:
        vrt.rtapi.debug_shadow_hints_enable(-1)
    assert np.array_equal(moved[0], off[0]) and np.array_equal(moved[1], off[1]) and moved[2] == off[2]
    assert not np.array_equal(moved[0], c.px)


def test_the_device_path_table_leads_every_triangle_to_its_leaf(vrt, golden, gpu_device):
    """The table of a real accel, read back and followed through the scene's own reference-format nodes (not the compact layout the pass
    reads): from the BLAS root, child `leftFirst + slot` with slot = code & 3, code >>= 2, until a leaf; the leaf's range holds the triangle
    and nothing of the code is left."""
    node = np.dtype([("o", "<f4", 3), ("e", "i1", 3), ("imask", "u1"), ("lf", "<u4"), ("ld", "<u4"), ("ch", "u1", (4, 7))])
    for sc in (vrt.scene.procedural("atrium", 4, 0, 3), golden("teapot")):
        ds = vrt.tracer.DeviceScene(sc, gpu_device)
        n_tris = sc["tri"].size // 36
        codes = vrt.rtapi.debug_read_path_table(ds.accel, n_tris, _stream())
        nodes = np.frombuffer(bytes(sc["bvh"]), node)
        root = int(np.frombuffer(bytes(sc["blas"]), np.uint32)[0])      # bvh_offset of the one instance record
        at = np.full(n_tris, root, np.int64)
        code = codes.astype(np.int64)
        for _ in range(17):
            inner = nodes["ld"][at] == 0
            if not inner.any():
                break
            slot = code & 3
            assert (nodes["ch"][at[inner], slot[inner], 0] != 0).all()   # (the hinted slot holds a child)
            at = np.where(inner, root + nodes["lf"][at].astype(np.int64) + slot, at)   # (child indices count from the BLAS's first node)
            code = np.where(inner, code >> 2, code)
        assert (nodes["ld"][at] != 0).all() and (code == 0).all()
        t = np.arange(n_tris)
        assert ((t >= nodes["lf"][at]) & (t < nodes["lf"][at] + nodes["ld"][at])).all(), sc["tri"].size
        ds.close()


if __name__ == "__main__":
    _count_guided_rays()
