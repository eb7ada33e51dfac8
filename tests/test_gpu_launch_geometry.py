"""GPU: every persistent launch gives the same results under any launch geometry (tests/launch_geometry_cases.py).

Every traversal launch -- frames, ray buffers, the trace launches inside the AO, bounce, path and emitter tails, the twin -- is a
persistent grid drawing jobs from eight sharded queue counters; how many workgroups it has, which XCD each lands on, how the job count
falls across the shards and which shards a workgroup found dry decide what a wavefront does there.  The rest of the suite runs every
request under one geometry, the one the occupancy query and the CU count of the box give.  Here:

  the parent   runs the list once under the environment the suite runs in.  Its plain and shadow frames at the sizes no other file
               covers (72 x 8, 200 x 120, 512 x 384), all its ray buffers and the twin's frames are held to the oracle, so "equal to
               the parent" means "equal to the oracle"; the path-family requests are held to their restatements at these
               configurations by their own files.
  a child      per setting of launch_geometry_cases.SETTINGS (every variable is read once per process) runs the same list and writes
               every output to an .npz; the parent compares each with its own as uint32 words, whole -- rows outside windows, guard
               words, return codes and the status word included, no mask, no tolerance.

Not vacuous: the end log (vxrt_debug_end_log) of every plain / shadow frame and ray buffer shows how many wavefronts the main launch
had (4 x its grid), the rays they started and their XCDs; the control block a ray buffer leaves shows what its launches did to the
shard counters.  Each test prints what it compared and what it saw (pytest -s)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import launch_geometry_cases as lg
import rc_cases as rcc
import request_programs as rp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOR_RTOL = 1e-5          # colours of the RTU path and of the twin against their restatements (tests/test_gpu_parity.py, tests/test_rc_twin.py)
EXACT_WAVES = 4 * lg.EXACT_GRID        # the EXACT launch of a ray buffer of at most 262,144 rays: its fixed grid


@pytest.fixture(scope="module")
def parent(vrt, po, gpu_device):
    """the list under the environment of this process: run once, shared, left unchanged"""
    t0 = time.perf_counter()
    out = lg.run_all(vrt, po, gpu_device)
    for a in out.values():
        a.setflags(write=False)
    print("parent: %d arrays of %d requests in %.2f s" % (len(out), _n_requests(), time.perf_counter() - t0))
    return out


def _n_requests():
    return sum(len(s[2]) for s in lg.SECTIONS.values()) + len(lg.TWIN)


def _steps():
    for section, (scene, muts, requests) in lg.SECTIONS.items():
        for i, step in enumerate(requests):
            yield section, scene, muts, i, step


def _get(run, section, i, name):
    return run[lg.key(section, i, name)]


def _body(a, n):
    """the n words of an output in front of its guard words, which must still hold the marker"""
    assert a.size == n + rp.GUARD and (a[n:] == a[-1]).all() and a[-1] in (rp.MARK, int(np.array([rp.FMARK], np.float32).view(np.uint32)[0]))
    return a[:n]


def _check_observations(run, setting=None, cus=None, reference=None):
    """what every process must show: return codes and status zero, something written, the wavefront counts of the logged launches inside
    their bounds (and as the setting says), the shard counters of the ray buffers as a launch can leave them.  Returns the wavefront
    counts seen, by job count."""
    s = setting or {}
    seen = {}
    for section, scene, muts, i, step in _steps():
        what = "%s %d %r" % (section, i, step)
        assert int(_get(run, section, i, "rc")[0]) == 0 and int(_get(run, section, i, "status")[0]) == 0, what
        outs = {k.rsplit("|", 1)[1]: v for k, v in run.items() if k.startswith(lg.key(section, i, "")) and lg.is_output(k)}
        assert not rp.untouched(outs), "nothing written: " + what
        if not lg.logged(step):
            continue
        jobs, waves = lg.jobs_of(step), int(_get(run, section, i, "_waves")[0])
        is_frame = step[1] == "render"
        assert waves % 4 == 0 and 4 <= waves <= 4 * lg.workgroups_needed(jobs), "%d wavefronts for %d jobs: %s" % (waves, jobs, what)
        if s.get("grid_max"):
            assert waves <= 4 * s["grid_max"], "%d wavefronts under VXRT_GRID_MAX=%d: %s" % (waves, s["grid_max"], what)
        if s.get("frames_one") and (is_frame or s.get("grid_max") == 1):
            assert waves == 4, "%d wavefronts where the launch is one workgroup: %s" % (waves, what)
        if s.get("grid_max") and not is_frame and lg.workgroups_needed(jobs) >= s["grid_max"]:       # (a frame's grid also leaves the side launch's reserve)
            assert waves == 4 * s["grid_max"], what
        if s.get("grid_max") == 1 and is_frame and jobs == 4096:
            assert len(_get(run, section, i, "_xcds")) == 1, "one workgroup on several XCDs: " + what
        if s.get("per_cu"):
            assert waves <= 4 * s["per_cu"] * cus, what
            if is_frame and jobs == 196608 and section != "hall_in_flight":
                # one workgroup per CU less the side launch's reserve (one context): a wavefront takes several reservations
                kw = rp.args_of(step)
                side = min(lg.EXACT_GRID, (kw["w"] + kw["h"] - 1 + 255) // 256)       # column W / 2 and row H / 2, one pixel shared
                assert waves == 4 * (cus - side) and waves * 64 * 2 <= jobs, "%d wavefronts on %d CUs: %s" % (waves, cus, what)
        if reference is not None:
            assert int(_get(run, section, i, "_rays")[0]) == int(_get(reference, section, i, "_rays")[0]), "rays started: " + what
        seen.setdefault(("frame " if is_frame else "trace ") + str(jobs), set()).add(waves)
        if lg.key(section, i, "_ctl") in run:
            ctl = _get(run, section, i, "_ctl")
            n = rp.args_of(step)["n"]
            deferred = int(ctl[0])
            assert 0 <= deferred <= n, what
            for which, jobs_q, waves_q in (("main", n, waves), ("exact", deferred, EXACT_WAVES)):
                bad = lg.counters_ok(ctl, jobs_q, waves_q, which)
                assert bad is None, "%s launch: %s: %s" % (which, bad, what)
    return {k: sorted(v) for k, v in seen.items()}


def test_parent_shows_its_launches(parent):
    import torch
    seen = _check_observations(parent, cus=torch.cuda.get_device_properties(0).multi_processor_count)
    print("parent: wavefronts of the main launch by job count:", seen)
    for section, scene, muts, i, step in _steps():
        if step[1] == "trace" and rp.args_of(step).get("src") == "axis" and lg.key(section, i, "_ctl") in parent:
            assert int(_get(parent, section, i, "_ctl")[0]) == lg.AXIS_N, "the axis-parallel rays were not all deferred"
            assert int(_get(parent, section, i, "_rays")[0]) == 0
    big = [len(_get(parent, s, i, "_xcds")) for s, _, _, i, step in _steps() if lg.logged(step) and lg.jobs_of(step) == 196608]
    print("parent: XCDs seen by the 512 x 384 frames:", big)


@pytest.mark.parametrize("section", ["cornell", "hall"])
def test_parent_frames_equal_the_oracle(vrt, po, gpu_device, parent, section):
    scene, _, requests = lg.SECTIONS[section]
    env = rp.Env(vrt, gpu_device, scene)
    held = occluded = 0
    for i, step in enumerate(requests):
        kw = rp.args_of(step)
        if step[1] != "render" or kw["depth"] != 1 or (kw["w"], kw["h"]) not in lg.ORACLE_FRAMES:
            continue
        w, h, n = kw["w"], kw["h"], kw["w"] * kw["h"]
        px, hits, col, rays = po.render_ex_mt(env.buffers, w, h, po.shade_params(), kw["shadow"])
        what = "%s %dx%d shadow %d" % (section, w, h, kw["shadow"])
        np.testing.assert_array_equal(_body(_get(parent, section, i, "dst"), n), px.reshape(-1), err_msg=what + ": pixels")
        got_hits = _body(_get(parent, section, i, "hits"), 6 * n).reshape(n, 6).copy()
        if kw["shadow"]:      # the hit output of a shadow frame carries the occlusion result in bit 31 of blasIdx (include/vortex_hip.h); the pixels show it
            occluded += int((got_hits[:, 4] >> 31).sum())
            got_hits[:, 4] &= 0x7FFFFFFF
        np.testing.assert_array_equal(got_hits, np.ascontiguousarray(hits).view(np.uint32).reshape(n, 6), err_msg=what + ": hit records")
        np.testing.assert_allclose(_body(_get(parent, section, i, "col"), 3 * n).view(np.float32), col.reshape(-1), rtol=COLOR_RTOL, atol=0, err_msg=what + ": colours")
        assert rp.rays_traced({"cnt": _get(parent, section, i, "cnt")}) == rays, what
        assert (hits["dist"] < 1e29).any() and (hits["dist"] >= 1e29).any() or section == "cornell", what
        held += 1
    assert held == 2 * len(lg.ORACLE_FRAMES) and occluded > 0
    print("%s: %d frames equal the oracle (%d occluded pixels in the shadow frames)" % (section, held, occluded))


@pytest.mark.parametrize("section", ["cornell", "hall"])
def test_parent_traces_equal_the_oracle(vrt, po, gpu_device, parent, section):
    scene, _, requests = lg.SECTIONS[section]
    env = lg.make_env(vrt, gpu_device, scene)
    held = hit = 0
    for i, step in enumerate(requests):
        if step[1] != "trace":
            continue
        kw = rp.args_of(step)
        rays = env.rays(kw["n"], kw["seed"], kw.get("src")).cpu().numpy()
        tmax = np.random.default_rng(kw["seed"]).uniform(50, 400, len(rays)).astype(np.float32) if kw["tmax"] else None
        want, _ = po.trace_canonical(env.buffers, rays, tmax=tmax, any_hit=bool(kw["mode"]))
        got = _body(_get(parent, section, i, "hits"), 6 * len(rays))
        np.testing.assert_array_equal(got, want.view(np.uint32).reshape(-1), err_msg="%s %r" % (section, step))
        held, hit = held + 1, hit + int((want["dist"] < 1e29).sum())
    assert held == 2 * len(lg.TRACE_COUNTS) + 1 and hit > 0
    print("%s: %d ray buffers equal the oracle (%d hits)" % (section, held, hit))


def test_parent_twin_frames_equal_the_oracle(po, parent):
    for i, (name, w, h) in enumerate(lg.TWIN):
        c = rcc.case(name, po)
        px, col = po.rc_render(rcc.args(po, c, w, h))
        what = "%s %dx%d" % (name, w, h)
        assert int(_get(parent, "twin", i, "status")[0]) == 0
        np.testing.assert_array_equal(_body(_get(parent, "twin", i, "px"), w * h), px.reshape(-1).view(np.uint32), err_msg=what)
        got, want = _body(_get(parent, "twin", i, "col"), 3 * w * h).view(np.float32), col.reshape(-1)
        for f in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(f(got), f(want)), what
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=COLOR_RTOL, atol=0, err_msg=what)


@pytest.mark.parametrize("name", list(lg.SETTINGS))
def test_a_launch_geometry_does_not_change_a_word(parent, tmp_path, name):
    """the whole list in a fresh process under the setting: every output equal to the parent's word for word, return codes and status
    zero, the rays started equal, the wavefront counts and shard counters showing that the setting took hold"""
    import torch
    setting = lg.SETTINGS[name]
    out = str(tmp_path / "run.npz")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", lg.child_source(), out], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **setting["env"]))
    seconds = time.perf_counter() - t0
    assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-4000:])
    with np.load(out) as z:
        child = {k: z[k] for k in z.files}
    bad = lg.differences(child, parent)
    if bad:
        print("%s: %d outputs differ from the parent's: %r" % (name, len(bad), bad[:40]))
    assert not bad, "%s: %d outputs differ, first %r" % (name, len(bad), bad[0])
    seen = _check_observations(child, setting, torch.cuda.get_device_properties(0).multi_processor_count, parent)
    n_out = sum(lg.is_output(k) for k in child)
    print("%s %r: %d outputs of %d requests equal the parent's in every word; child %.2f s; wavefronts by job count: %r" % (
        name, setting["env"], n_out, _n_requests(), seconds, seen))
