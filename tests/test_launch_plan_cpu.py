"""CPU: the arithmetic of a launch's grid (csrc/rt_launch_plan.h: persistent_grid's cap by need, launch_plan's knob defaults, main_grid's
reserve and share) swept by a stand-alone program.

rt_launch_plan.h is the header rt_kernels.hip and rc_kernels.hip compile; plain g++ compiles it too.  tests/launch_plan_check.cpp (its
own main) sweeps what the device holds x side workgroups 0..128 x job counts around the "small window" edge and up to 2^32 - 1 x
VXRT_GRID_DIV x VXRT_SIDE_RESERVE x frame contexts x VXRT_GRID_MAX and asserts the bounds of the grid, the absence of unsigned wrap (against
64-bit signed arithmetic) and, with no VXRT_GRID_MAX, equality with the expressions the header replaced, restated literally.  Built with
-fsanitize=undefined,address: host code only, nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vortex-raytracing_amd", "csrc")


def test_the_plan_keeps_its_bounds_and_the_move_is_a_move(tmp_path):
    exe = str(tmp_path / "launch_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "launch_plan_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # 9 caps x 7 job counts x (129 side counts x 7 divisors x 3 reserves x 2 context counts x 3 maxima; 3 maxima x 2 workgroup sizes)
    assert r.stdout.strip() == "%d plan cases, %d grid cases, 0 failures" % (9 * 7 * 129 * 7 * 3 * 2 * 3, 9 * 7 * 3 * 2), r.stdout
