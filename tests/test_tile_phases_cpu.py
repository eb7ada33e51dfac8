"""CPU: the fetch / finish policy of the shadow frame kernels that hold the occlusion-only loop, replayed on random tile masks
(RT_TILE_PHASES, RT_TILE_REFILL_MIN: csrc/rt_kernels.hip).

tests/tile_phases_check.cpp is a stand-alone program (its own main) around the kernel's own fetch rule (csrc/rt_tile_refill.h): one wavefront walks queues of 8x8 tiles whose lanes start a ray or
not (window edge, a-priori list), hit or miss, defer their occlusion ray or trace it.  Under every rule every job is traced once; with
65 (no partial refill) no pass holds a primary and an any-hit ray and no job is handed out while a lane holds work; under 32 and 16 a
partial refill never meets fewer idle lanes than that; the parent's rule (1) mixes behind a partial tile, and in a closed room with one
a-priori column the shift never heals.  What the shipped threshold (32) leaves open is stated there too: behind one tile that
leaves 32 or more lanes idle a wavefront in a closed room stays mixed, as under the parent's rule; behind one that leaves fewer it is 65.  Built with -fsanitize=undefined,address: host code only, nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vortex-raytracing_amd", "csrc")


def test_whole_tile_phases_never_mix_and_the_parents_rule_does(tmp_path):
    exe = str(tmp_path / "tile_phases_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "tile_phases_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # 4,000 queues x 4 rules + 3 hand-made queues x 3 rules; the parent's rule mixed 3,085 of its 4,000 random queues; 560 closed rooms of
    # at least 8 tiles stayed shifted to the end
    assert r.stdout.strip() == "16009 cases, parent rule mixed 3085, sticky 560, 0 failures", r.stdout
