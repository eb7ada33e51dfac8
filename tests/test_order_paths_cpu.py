"""CPU: the node step without the sorting network (RT_ORDER_PATHS, csrc/rt_order.h) against the step with the network.

rt_order.h is the header the traversal kernels compile; plain g++ compiles it too.  tests/order_paths_check.cpp is a stand-alone program
(its own main) over it: all 16 validity masks x distances from {-1, -0, +0, 1, 2} in every slot (ties in every slot pair) x four path
maxima; where at most one child is valid, path A against the network on the child taken, the entries pushed (none), the new path maximum
and which lanes pop; on every mask, the counting conditions the run's test is made of.  Built with -fsanitize=undefined,address: host code
only, nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vortex-raytracing_amd", "csrc")


def test_path_a_decides_what_the_network_decides(tmp_path):
    exe = str(tmp_path / "order_paths_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "order_paths_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # 16 masks x 625 assignments x 4 maxima; path A sees the masks of at most one valid child (5 of 16)
    assert r.stdout.strip() == "40000 cases, 12500 through path A, 0 failures", r.stdout
