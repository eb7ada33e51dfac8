"""The requests of tests/test_gpu_launch_geometry.py and tests/test_launch_geometry_cpu.py.  TEST INFRASTRUCTURE ONLY.

Every traversal launch is a persistent grid drawing jobs from eight sharded queue counters.  What a wavefront does there depends on
how many workgroups were launched, which XCD each landed on, how the job count falls across the shards and which shards its
workgroup found dry -- none of which may change a result.  This module holds the list of requests whose job counts are chosen for how
they fall across the shards (SECTIONS, TWIN), the restated shard arithmetic that says so, the runner that executes the list once in
a process, and the comparison of two such runs.  The runner is request_programs' (Env, issue, _alloc, host, untouched): every output
prefilled with markers, guard words behind it, return code and status word read back.

A run is a flat dict  "<section>|<index>|<output>" -> uint32 words.  Names that begin with "_" are observations, not outputs:
  _waves   wavefronts of the main launch that left an entry in the end log (4 x its grid)
  _rays    sum of the rays they started
  _xcds    the distinct physical XCDs they report
  _ctl     the control block a trace left behind (the defer count, the main and the EXACT launch's shard counters)
"""
import os

import numpy as np

import request_programs as rp
from request_programs import frame, mut, req

SHARDS, CHUNK, STRIDE = 8, 64, 32           # QUEUE_SHARDS, RT_CHUNK = RT_TRACE_CHUNK, QUEUE_STRIDE (csrc/rt_internal.h, rt_kernels.hip)
WG_THREADS, EXACT_GRID = 256, 128
END_LOG_WAVES = 8192
TRACE_COUNTS = (1, 63, 64, 65, 513, 4097, 20000)
AXIS_N, AXIS_SEED = 513, 77


# ---- the shard arithmetic, restated ----
def per_shard(n):
    """jobs per shard of the RTU path: ((n + 7) / 8 + 63) & ~63 (trace_on_ctx, frame_args, the kernels' own form for device counts)"""
    return ((n + SHARDS - 1) // SHARDS + 63) & ~63


def shard_jobs(n):
    """jobs of each of the eight shards; 0: the shard lies past the end of the job range (the RTGUARD path)"""
    p = per_shard(n)
    return [max(0, min(p, n - s * p)) for s in range(SHARDS)]


def frame_jobs(w, y0, y1, batch=1):
    return rp.tiles(w, y0, y1)[2] * 64 * batch


def twin_shard_tiles(w, y0, y1):
    """the twin's shards count tiles: ceil(tiles / 8) each"""
    n = rp.tiles(w, y0, y1)[2]
    p = (n + SHARDS - 1) // SHARDS
    return [max(0, min(p, n - s * p)) for s in range(SHARDS)]


def workgroups_needed(jobs):
    return max(1, (jobs + WG_THREADS - 1) // WG_THREADS)


# ---- the requests ----
def _render(w, h, y0=0, y1=None, shadow=0, depth=1):
    return req("render", w=w, h=h, y0=y0, y1=h if y1 is None else y1, shadow=shadow, depth=depth)


def _both(w, h, y0=0, y1=None):
    return [_render(w, h, y0, y1, 0), _render(w, h, y0, y1, 1)]


FRAME_SIZES = [(13, 7), (72, 8), (16, 12), (64, 64), (200, 120), (512, 384)]
WINDOW = (96, 64, 11, 37)
ORACLE_FRAMES = [(72, 8), (200, 120), (512, 384)]     # the sizes the suite does not already hold to the oracle: held to it here
FRAMES = [r for w, h in FRAME_SIZES for r in _both(w, h)] + _both(*WINDOW)


def _camera(cam):
    """the camera kernels, tile_order = batch_order, JOB_RENDER_GI, the mirror arm"""
    out = []
    for w, h in ((16, 12), (72, 8)):
        out += [req("render_camera", cam=cam, w=w, h=h, shadow=0), req("render_camera", cam=cam, w=w, h=h, shadow=1),
                req("rows_batch", w=w, h=h, y0=0, y1=h, nf=3, shadow=0), req("gi", cam=cam, seed=3, w=w, h=h), _render(w, h, depth=3)]
    return out


def _traces(src):
    return ([req("trace", n=n, mode=0, seed=100 + n, tmax=0, src=src) for n in TRACE_COUNTS] +
            [req("trace", n=n, mode=1, seed=200 + n, tmax=1, src=src) for n in TRACE_COUNTS] +
            [req("trace", n=AXIS_N, mode=0, seed=AXIS_SEED, tmax=0, src="axis")])          # everything deferred: 128 EXACT workgroups for 513 jobs


MIS_BIG = frame("mis", 1, 2, 3, 5, w=rp.BIG_W, h=rp.BIG_H)
# trace launches whose job count lives on the device (total_dev), ordered and unordered any-hit
TAILS_HALL = [rp.AO, rp.PATH, rp.EMITTER[("mis", 1)], rp.SPECULAR["mis"], rp.COUNTS["mis"], rp.DENOISED, MIS_BIG]
_CORNELL_AO = req("ao", cam="framing", spp=4, seed=3, radius=40.0)
_CORNELL_PATH = req("path", cam="framing", spp=rp.SPP, bounces=3, seed=rp.SEED, shadow=1)
TAILS_CORNELL = [_CORNELL_AO, _CORNELL_PATH, rp.COUNTS[None], rp.DENOISED]     # (no emitters: the forms that need no table)

# (scene, mutators in front of every request, requests).  cornell: a single identity instance, the identity-root kernels; hall: the
# general kernels.  The third section runs with three frame contexts: n_ctx > 1 changes the defaults of side_reserve and grid_div.
SECTIONS = {
    "cornell": ("cornell", [], FRAMES + _camera("framing") + _traces("fan") + TAILS_CORNELL),
    "hall": ("hall", [mut("emitters", 1)], FRAMES + _camera("orbit_1") + _traces(None) + TAILS_HALL),
    "hall_in_flight": ("hall", [mut("emitters", 1), mut("in_flight", 3)],
                       _both(72, 8) + _both(16, 12) + _both(64, 64) + _both(200, 120) + _both(*WINDOW) +
                       [req("trace", n=513, mode=0, seed=613, tmax=0), req("trace", n=4097, mode=1, seed=4297, tmax=1),
                        rp.AO, rp.PATH, rp.EMITTER[("mis", 1)], rp.SPECULAR["mis"]]),
}
# the twin's frames: (case of rc_cases, w, h); its shards count tiles, 9 tiles give 2, 2, 2, 2, 1 and three shards past the end
TWIN = [(name, w, h) for name in ("tlas_9", "mirrors_d3_s3") for w, h in ((13, 7), (72, 8), (64, 64))]

# The settings of the children: every variable is read once per process.  `grid_max`: VXRT_GRID_MAX of the setting; `frames_one`: a
# frame's main launch is one workgroup (settings 1 and 4); `per_cu`: VXRT_WGS_PER_CU.
SETTINGS = {
    "grid_max_1": dict(env={"VXRT_GRID_MAX": "1", "VXRC_GRID_MAX": "1"}, grid_max=1, frames_one=True),
    "grid_max_2": dict(env={"VXRT_GRID_MAX": "2", "VXRC_GRID_MAX": "2"}, grid_max=2),
    "grid_max_3_packed": dict(env={"VXRT_GRID_MAX": "3", "VXRT_PACKED": "1"}, grid_max=3),
    "grid_div_huge_reserve": dict(env={"VXRT_GRID_DIV": "1000000", "VXRT_SIDE_RESERVE": "1"}, frames_one=True),
    "no_reserve_no_div": dict(env={"VXRT_SIDE_RESERVE": "0", "VXRT_GRID_DIV": "-1"}),
    "shard_rot_3": dict(env={"VXRT_SHARD_ROT": "3"}),
    "shard_rot_max": dict(env={"VXRT_SHARD_ROT": "2147483647"}),
    "wgs_per_cu_1": dict(env={"VXRT_WGS_PER_CU": "1"}, per_cu=1),
    "ordered_any": dict(env={"VXRT_UNORDERED_ANY": "0"}),
}
KNOB_NAMES = sorted({k for s in SETTINGS.values() for k in s["env"]})


def jobs_of(step):
    """jobs of the request's main launch (frames and traces), None for the requests whose launches are not logged"""
    kind, kw = step[1], rp.args_of(step)
    if kind == "trace":
        return AXIS_N if kw.get("src") == "axis" else kw["n"]
    if kind == "render":
        return frame_jobs(kw["w"], kw["y0"], kw["y1"])
    return None


def logged(step):
    """the requests whose main launch is read from the end log: plain / shadow frames of the fixed camera and ray buffers"""
    return step[1] == "trace" or (step[1] == "render" and rp.args_of(step)["depth"] == 1)


def key(section, i, name):
    return "%s|%03d|%s" % (section, i, name)


# ---- running the list ----
def axis_rays(scene, n, seed):
    """axis-parallel rays: a zero direction component puts a ray outside the fast domain, the main launch defers every one of them"""
    rng = np.random.default_rng(seed)
    d = np.zeros((n, 3))
    if scene == "cornell":      # from around the fixed camera's position along +x, the way it looks
        o = np.array((0.0, 100.0, 0.0)) + rng.uniform(-30, 30, (n, 3)) * (0, 1, 1)
        d[:, 0] = 1.0
    else:
        o = rng.uniform((0, 20, -150), (350, 220, 150), (n, 3))
        d[np.arange(n), np.arange(n) % 3] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return np.concatenate([o, d], 1).astype(np.float32)


def make_env(vrt, device, scene):
    env = rp.Env(vrt, device, scene)
    env.device_input(("rays", AXIS_N, AXIS_SEED, "axis"), lambda: axis_rays(scene, AXIS_N, AXIS_SEED))     # (Env.rays finds it under its key)
    return env


def read_log(log):
    """(wavefronts that left an entry, rays they started, their XCDs) of an end log read back (2 x END_LOG_WAVES u64)"""
    e = np.asarray(log, np.uint64).reshape(END_LOG_WAVES, 2)
    used = e[:, 0] != 0
    return int(used.sum()), int((e[used, 1] & np.uint64((1 << 56) - 1)).sum()), sorted(set(int(v) for v in (e[used, 1] >> np.uint64(56))))


def run_sections(vrt, device, sections=None):
    """every request of SECTIONS on a fresh accel of its own, behind the section's mutators -> the flat dict of the module docstring"""
    import torch
    out = {}
    stream = torch.cuda.current_stream().cuda_stream
    for section, (scene, muts, requests) in SECTIONS.items():
        if sections is not None and section not in sections:
            continue
        env = make_env(vrt, device, scene)
        log = torch.zeros(2 * END_LOG_WAVES, dtype=torch.int64, device=device)
        for i, step in enumerate(requests):
            ds = env.fresh()
            try:
                if scene == "cornell":
                    assert env.R.accel_info(ds.accel, 5) == 1, "the cornell box does not take the identity-root kernels"
                for m in muts:
                    assert rp.mutate(env, ds, m)
                if logged(step):
                    log.zero_()
                    env.R.debug_end_log(ds.accel, log.data_ptr())
                rc, o = rp.issue(env, ds, step, stream, {})
                torch.cuda.synchronize()
                got = rp.host(o)
                got["rc"] = np.array([rc & 0xFFFFFFFF], np.uint32)
                got["status"] = np.array([env.R.status(stream)], np.uint32)
                if logged(step):
                    env.R.debug_end_log(ds.accel, None)
                    waves, rays, xcds = read_log(log.cpu().numpy().view(np.uint64))
                    got["_waves"], got["_rays"], got["_xcds"] = np.array([waves], np.uint32), np.array([rays], np.uint64), np.array(xcds, np.uint32)
                    if step[1] == "trace" and not any(m[1] == "in_flight" for m in muts):        # (one context: the trace ran on context 0)
                        got["_ctl"] = env.R.debug_read_control(ds.accel, 0, 32 + 2 * SHARDS * STRIDE, stream)
                for name, a in got.items():
                    out[key(section, i, name)] = a
            finally:
                torch.cuda.synchronize()
                ds.close()
    return out


def run_twin(vrt, po, device):
    """the twin's frames (pixels and colours, marker-filled, guard words behind) -> "twin|<index>|px" / "col" / "status" """
    import torch
    import rc_cases as rcc
    out, s = {}, torch.cuda.current_stream().cuda_stream
    for i, (name, w, h) in enumerate(TWIN):
        c = rcc.case(name, po)
        ds = vrt.tracer.RcDeviceScene(c["scene"], device)
        px = torch.full((w * h + rp.GUARD,), rp.MARK, dtype=torch.int32, device=device)
        col = torch.full((3 * w * h + rp.GUARD,), rp.FMARK, dtype=torch.float32, device=device)
        vrt.rtapi.rc_render_accel(ds.accel, w, h, 0, h, vrt.rtapi.rc_params(c["cam"], c["light"], c["spp"], c["depth"]), px.data_ptr(), col.data_ptr(), s)
        out[key("twin", i, "status")] = np.array([vrt.rtapi.status(s)], np.uint32)
        out[key("twin", i, "px")] = px.cpu().numpy().view(np.uint32).copy()
        out[key("twin", i, "col")] = col.cpu().numpy().view(np.uint32).copy()
        ds.close()
    return out


def run_all(vrt, po, device):
    out = run_sections(vrt, device)
    out.update(run_twin(vrt, po, device))
    return out


# ---- comparing two runs ----
def is_output(k):
    return not k.rsplit("|", 1)[1].startswith("_")


def differences(got, want):
    """the outputs (not the observations) that are not equal word for word, whole: [(key, words that differ or why)]"""
    bad = []
    for k in sorted(set(got) | set(want)):
        if not is_output(k):
            continue
        if k not in got or k not in want:
            bad.append((k, "missing"))
        elif got[k].shape != want[k].shape or got[k].dtype != want[k].dtype:
            bad.append((k, "shape %r %s against %r %s" % (got[k].shape, got[k].dtype, want[k].shape, want[k].dtype)))
        elif not np.array_equal(got[k], want[k]):
            bad.append((k, int((got[k] != want[k]).sum())))
    return bad


def counters_ok(ctl, n, waves, which="main"):
    """the shard counters a trace's launch left (which = "main": the launch over n rays by `waves` wavefronts; "exact": the EXACT
    launch over the ctl[0] deferred rays by `waves` wavefronts): a shard past the end has counter 0; an in-range shard's counter is a
    multiple of the chunk, at least its jobs rounded up to the chunk, at most that plus one chunk per wavefront.  Returns the first
    complaint or None."""
    base = 32 + (SHARDS * STRIDE if which == "exact" else 0)
    q = [int(v) for v in ctl[base:base + SHARDS * STRIDE:STRIDE]]
    for s, (jobs, c) in enumerate(zip(shard_jobs(n), q)):
        if jobs == 0:
            if c != 0:
                return "shard %d lies past the end of %d jobs, counter %d" % (s, n, c)
            continue
        full = (jobs + CHUNK - 1) // CHUNK * CHUNK
        if c % CHUNK or c < full or c > full + CHUNK * waves:
            return "shard %d holds %d jobs of %d, counter %d with %d wavefronts" % (s, jobs, n, c, waves)
    return None


CHILD = r"""
import importlib, sys
import numpy as np
sys.path[:0] = [%r, %r]
import launch_geometry_cases as lg
from oracle import pyoracle as po
vrt = importlib.import_module("vortex-raytracing_amd")
np.savez(sys.argv[1], **lg.run_all(vrt, po, "cuda:0"))
"""


def child_source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return CHILD % (root, os.path.join(root, "tests"))
