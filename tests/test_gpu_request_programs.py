"""GPU: request sequences on ONE accel (tests/request_programs.py).  A long-lived accel sees every kind of request in some order, and a
frame context's buffers, the accel's keyed caches and its tables survive each of them.  Every request of a program is held, bit for
bit and output for output -- return code, status word, ray counts, rows outside the window and guard words included -- to the same
request on a QUIET TWIN, a fresh accel that has seen only the mutators and history steps before it; after a move also to a fresh accel
rebuilt from the busy accel's buffers.  The suite's other files hold the fresh accel's frames to the restatements; none runs here.
  A   every form through one context, twice (in process; in a child with small path and AO batches)
  B   the accel's keyed caches: uvtab, the a-priori list and its prefix rule, batch_order, the learned tile orders
  C   refits between forms: a stale emitter table, motion with a history, the identity-root kernels swapped out and in, a refused transform
  D   refusals in the middle, the alpha table among them
  E   three contexts handed out round robin to two streams that nothing synchronises
Each test prints how many requests ran and how many twins were computed (pytest -s)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import request_programs as rp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.environ.get("VXRT_REQUEST_PROGRAMS_TEST_CHILD") == "1"


@pytest.fixture(autouse=True)
def _status_is_clean(vrt):
    import torch
    yield
    assert vrt.rtapi.status(torch.cuda.current_stream().cuda_stream) == 0


def _run(vrt, golden, gpu_device, name, streams=None):
    scene, program = rp.PROGRAMS[name]
    runner = rp.Runner(rp.Env(vrt, gpu_device, scene, golden))
    outs = runner.run(program, streams)
    print("program %s: %d steps, %d requests held to %d twins (%d refused), %d to the rebuilt twin" % (
        name, len(program), runner.stats["requests"], runner.stats["twins"], runner.stats["refused"], runner.stats["rebuilt"]), "accel_info", runner.fresh_info)
    assert runner.stats["requests"] == sum(rp.is_request(s) for s in program)
    return runner, outs


def test_program_a_every_form_through_one_context(vrt, golden, gpu_device):
    runner, _ = _run(vrt, golden, gpu_device, "A")
    assert runner.stats["twins"] == len({s for s in rp.A_PROGRAM if rp.is_request(s)})        # (one state: a repeated request costs no twin)


def test_program_a_in_small_batches(vrt):
    """VXRT_PATH_BATCH and VXRT_AO_BATCH are read once per process: a fresh child runs program A -- the twins under the same knobs --
    with batch boundaries inside pixels and several batches per frame on the reused buffers.  The knob line the library prints under
    VXRT_DEBUG shows that the child took them."""
    assert not CHILD
    env = dict(os.environ, VXRT_PATH_BATCH=str(rp.CHILD_PATH_BATCH), VXRT_AO_BATCH=str(rp.CHILD_AO_BATCH), VXRT_REQUEST_PROGRAMS_TEST_CHILD="1", VXRT_DEBUG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "test_program_a_every_form"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and ("path_batch=%d ao_batch=%d " % (rp.CHILD_PATH_BATCH, rp.CHILD_AO_BATCH)) in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    print([l for l in r.stdout.splitlines() if l.startswith("program")])


def test_program_b_keyed_caches(vrt, golden, gpu_device):
    _run(vrt, golden, gpu_device, "B")


def test_program_b_learned_tile_orders(vrt, golden, gpu_device):
    _run(vrt, golden, gpu_device, "B_lpt")


def test_program_c_stale_emitter_table(vrt, golden, gpu_device):
    runner, _ = _run(vrt, golden, gpu_device, "C_emitters")
    assert runner.stats["refused"] == 1


def test_program_c_motion_with_a_history(vrt, golden, gpu_device):
    _run(vrt, golden, gpu_device, "C_motion")


@pytest.mark.parametrize("scene", ["teapot", "cornell"])
def test_program_c_identity_root_swapped(vrt, golden, gpu_device, scene):
    """the five forms on a single identity instance, under a translation, under the identity again and after a geometry refit; the
    program asserts vxrt_accel_info 2 and 5 at every stage"""
    runner, outs = _run(vrt, golden, gpu_device, "C_ident_" + scene)
    if scene == "cornell" and not (os.environ.get("VXRT_LIB_DIR") or os.environ.get("VXRT_IDENT_ROOT") == "0" or os.environ.get("VXRT_SHALLOW") == "0"):
        assert runner.fresh_info[5] == 1            # the identity-root kernels were taken, dropped (info 5 == 0 under the translation) and taken again
    # the stages are not one another: the traced hit records (and, of the cornell box, the plain frame) move with the instance and the vertices
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)
    for form in (rp.C_IDENT[scene][6],) + ((rp.C_IDENT[scene][2],) if scene == "cornell" else ()):
        stages = [v for (state, step), v in sorted(outs.items(), key=lambda kv: kv[0][0]) if step == form]
        assert len(stages) == 4 and form[1] in ("trace", "render")
        assert same(stages[0], stages[2]) and not same(stages[0], stages[1]) and not same(stages[2], stages[3])


def test_program_c_refused_transform(vrt, golden, gpu_device):
    _run(vrt, golden, gpu_device, "C_refused")


def test_program_d_refusals_in_the_middle(vrt, golden, gpu_device):
    runner, _ = _run(vrt, golden, gpu_device, "D")
    assert runner.stats["refused"] == len(rp.REFUSALS)


def test_program_d_alpha_table(vrt, golden, gpu_device):
    runner, _ = _run(vrt, golden, gpu_device, "D_alpha")
    assert runner.stats["refused"] == 4


def test_program_e_several_contexts(vrt, golden, gpu_device):
    import torch
    streams = [torch.cuda.Stream(device=gpu_device) for _ in range(2)]
    _run(vrt, golden, gpu_device, "E", streams)
