"""GPU: what the vxrt_render_path* entry points refuse, and what they let through, as return codes of the C functions (0 against -1) --
every entry point builds a descriptor and goes through render_path_frame, where a null part means "absent", so the parts an entry
point's name promises are its own to check, and check_request answers an empty window before it looks at the path.  One row per
(entry point, defect); after every row dst still holds its fill pattern, except where the row says that the frame is rendered.

Not repeated here: the values of the parameters (spp, bounces, the sigmas, alpha, epsilon, nee, scale), the alpha table and the stale
accel -- test_refusals / test_frame_refusals / test_refusals_leave_dst_untouched / test_alpha_table_is_refused / test_stale_accel_is_refused
of test_gpu_path.py, test_gpu_denoise.py, test_gpu_temporal.py, test_gpu_motion.py, test_gpu_variance.py, test_gpu_adaptive.py,
test_gpu_emissive.py and test_gpu_emissive_mis.py hold them through rtapi -- and the descriptor's own door, which
test_gpu_path_frame.py::test_refusals_leave_everything_untouched holds."""
import ctypes as C

import pytest

import camera_secondary_ref as csr
import path_frame_cases as fc

pytestmark = pytest.mark.gpu
W, H = fc.W, fc.H
MARK = 0x5A5A5A
SPP, BOUNCES, SHADOW, SEED = fc.CONFIG

# entry point -> its arguments behind (accel, cam, width, height, y0, y1, params, path) and in front of stream
ORDER = {
    "path": "dst colors rays",
    "denoised": "dn dst colors aov rays",
    "temporal": "dn tp hist dst colors aov rays",
    "temporal_motion": "dn tp hist dst colors aov prev rays",
    "variance": "dn tp vp hist motion dst colors aov prev var rays",
    "adaptive": "counts dst colors rays",
    "variance_adaptive": "counts dn tp vp hist motion dst colors aov prev var rays",
    "emissive": "em dst colors rays",
    "emissive_mis": "em dst colors rays",
}
# the parts each entry point's name promises
PROMISED = {name: [a for a in order.split() if a in ("dn", "tp", "hist", "vp", "counts", "em")] for name, order in ORDER.items()}
NEEDS_CAMERA = ("temporal", "temporal_motion", "variance", "variance_adaptive")
MOMENTS = ("variance", "variance_adaptive")


@pytest.fixture(scope="module")
def door(vrt, gpu_device):
    """call(name, **overrides) -> the entry point's return code, on the 96 x 64 hall with its emitter table set; px, the frame's dst"""
    import torch
    R = vrt.rtapi
    L = R._lib()
    b, pairs = fc.hall(vrt)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in csr.KEYS}, gpu_device)
    ds.set_emitters(pairs)
    px = torch.full((H * W,), MARK, dtype=torch.int32, device=gpu_device)
    prev = torch.zeros((H * W * 4,), dtype=torch.float32, device=gpu_device)
    counts = torch.full((H * W,), 2, dtype=torch.int32, device=gpu_device)
    hists = {"plain": R.History(W, H), "moments": R.History(W, H, moments=True),
             "small plain": R.History(W, H // 2), "small moments": R.History(W, H // 2, moments=True)}
    keep = {"params": R.default_shade_params(), "path": R.PathParams(SPP, BOUNCES, SEED, SHADOW), "dn": R.DenoiseParams(*fc.DN),
            "tp": R.TemporalParams(*fc.TP), "vp": R.VarianceParams(*fc.VP, 0), "cam": R._camera(fc.cameras(vrt)[0]),
            "emissive": R.EmissiveParams(1, float(fc.SCALE), (C.c_uint32 * 2)(0, 0)), "emissive_mis": R.EmissiveMisParams(float(fc.SCALE), (C.c_uint32 * 3)(0, 0, 0))}

    def call(name, **over):
        a = {"cam": keep["cam"], "y0": 0, "y1": H, "path": keep["path"], "dn": keep["dn"], "tp": keep["tp"], "vp": keep["vp"], "em": keep[name] if name.startswith("emissive") else None,
             "hist": hists["moments" if name in MOMENTS else "plain"], "counts": counts.data_ptr(), "motion": 0, "dst": px.data_ptr(), "colors": None, "aov": None,
             "prev": None, "var": None, "rays": None}
        a.update(over)
        ref = lambda x: None if x is None else C.byref(x)
        conv = {"dn": ref, "tp": ref, "vp": ref, "em": ref, "hist": lambda h: None if h is None else R._history(h)}
        tail = [conv.get(k, lambda x: x)(a[k]) for k in ORDER[name].split()]
        fn = getattr(L, "vxrt_render_" + ("path" if name == "path" else "path_" + name))
        return fn(ds.accel, ref(a["cam"]), W, H, a["y0"], a["y1"], C.byref(keep["params"]), ref(a["path"]), *tail, torch.cuda.current_stream().cuda_stream)

    def untouched():
        return bool((px == MARK).all().item())

    door = type("Door", (), {})()
    door.call, door.untouched, door.px, door.hists, door.prev, door.R, door.cam = call, untouched, px, hists, prev, R, keep["cam"]
    yield door
    torch.cuda.synchronize()
    for h in hists.values():
        h.close()
    ds.close()


def _bad_camera(door):
    v = door.cam.cam14()
    v[10] = float("inf")   # one field that is not finite
    return door.R.Camera.from_cam14(v)


@pytest.mark.parametrize("name", list(ORDER))
def test_refusals(door, name):
    call = door.call
    assert call(name, path=None) == -1, "a null path"
    for part in PROMISED[name]:
        assert call(name, **{part: None}) == -1, "a null " + part
    assert call(name, cam=_bad_camera(door)) == -1, "a camera with a field that is not finite"
    if name in NEEDS_CAMERA:
        assert call(name, cam=None) == -1, "the fixed camera on a form with a history"
        kind = "moments" if name in MOMENTS else "plain"
        assert call(name, hist=door.hists["plain" if kind == "moments" else "moments"]) == -1, "a history of the wrong kind"
        assert call(name, hist=door.hists["small " + kind]) == -1, "a history of another window"
    if name in MOMENTS:
        assert call(name, motion=-1) == -1 and call(name, motion=2) == -1, "motion outside {0, 1}"
        assert call(name, motion=0, prev=door.prev.data_ptr()) == -1, "prev_position with motion = 0"
        # (check_request's refusal, so behind its empty window: the order is the entry points' own, the descriptor refuses this first)
        assert call(name, motion=0, prev=door.prev.data_ptr(), y0=9, y1=9) == 0, "prev_position with motion = 0 on an empty window"
    assert door.untouched()


@pytest.mark.parametrize("name", list(ORDER))
def test_empty_window_comes_before_the_path_tests(door, name):
    R = door.R
    assert door.call(name, y0=7, y1=7, path=R.PathParams(0, BOUNCES, SEED, SHADOW)) == 0, "an empty window with spp = 0"
    assert door.call(name, y0=7, y1=7, path=None) == -1, "an empty window with a null path"
    assert door.call(name, y0=7, y1=7) == 0, "an empty window with everything valid"
    assert door.call(name, y0=H, y1=H) == 0 and door.call(name, y0=0, y1=0) == 0
    assert door.untouched()
    for h in door.hists.values():   # (the histories are still empty: nothing was accumulated either)
        assert R._lib().vxrt_history_read(h.handle, door.prev.data_ptr(), None) == -1


@pytest.mark.parametrize("name", [n for n in ORDER if n not in NEEDS_CAMERA])
def test_fixed_camera_is_accepted(door, name):
    """the forms without a history take cam = NULL: the frame is rendered (rows [8, 24) of it)"""
    import torch
    try:
        assert door.call(name, cam=None, y0=8, y1=24) == 0
        torch.cuda.synchronize()
        px = door.px.view(H, W)
        assert bool((px[8:24] != MARK).all().item()) and bool((px[:8] == MARK).all().item()) and bool((px[24:] == MARK).all().item())
        assert door.R.status(torch.cuda.current_stream().cuda_stream) == 0
    finally:
        door.px.fill_(MARK)
