#!/usr/bin/env python3
"""What the wavefronts of the shadow frame kernels with the occlusion-only loop ran (RT_TILE_PHASES): shares of their passes through the
traversal loop, and of the node-body runs inside them, by form -- the occlusion-only form, the general form with no any-hit lane, the
general form holding primary and any-hit rays.  Needs a library that counts (-DRT_PHASE_COUNT=1; choose it with VXRT_LIB_DIR).

Three workloads, one JSON line each:
  headline   sets of five 1920x1080 frames of the level-8 atrium on two streams, as bench.py renders them (--sets of them; the first
             pair runs the kernels without hints, the repeats the hinted ones)
  bunny      the bunny-class 1024x1024 frame of tools/config_bench.py (frames with background)
  camera     one 1920x1080 frame of the atrium through a caller's camera, from beside the fixed camera's position

    VXRT_LIB_DIR=vortex-raytracing_amd/lib_ab/<counting build> python tools/phase_counts.py [--sets 6] [--level 8]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIGHT = (300.0, 480.0, 60.0)      # bench.py's
NAMES = ("occlusion_only", "general_primary_only", "general_mixed")


def shares(c):
    p, n = sum(c[:3]), sum(c[3:])
    return {"passes": dict(zip(NAMES, c[:3])), "node_body_runs": dict(zip(NAMES, c[3:])),
            "pass_share": {k: round(v / max(p, 1), 4) for k, v in zip(NAMES, c[:3])},
            "node_body_run_share": {k: round(v / max(n, 1), 4) for k, v in zip(NAMES, c[3:])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--level", type=int, default=8)
    a = ap.parse_args()
    import numpy as np
    import torch
    vrt = importlib.import_module("vortex-raytracing_amd")
    rt = vrt.rtapi
    if rt.debug_phase_counts() is None:
        raise SystemExit("this library does not count (build it with -DRT_PHASE_COUNT=1 and point VXRT_LIB_DIR at it)")
    dev = "cuda:0"

    def params(light):
        p = rt.default_shade_params()
        p.light_pos[:] = light
        return p

    def report(workload, **kw):
        torch.cuda.synchronize()
        print(json.dumps(dict({"tool": "phase_counts", "workload": workload, "lib": os.environ.get("VXRT_LIB_DIR", "")}, **kw, **shares(rt.debug_phase_counts(True)))), flush=True)

    # headline
    w, h, nf = 1920, 1080, 5
    sc = vrt.scene.procedural("atrium", a.level, 0, 3)
    ds = vrt.tracer.DeviceScene(sc, dev)
    rt.accel_frames_in_flight(ds.accel, 2)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    bufs = [torch.zeros((nf, h, w), dtype=torch.int32, device=dev) for _ in range(2)]
    plist = [params(LIGHT) for _ in range(nf)]
    torch.cuda.synchronize()
    rt.debug_phase_counts(True)
    for k in range(a.sets):
        rt.render_batch(ds.accel, w, h, plist, bufs[k % 2].data_ptr(), h * w, 1, None, streams[k % 2].cuda_stream)
        if k % 2 == 1:
            report("headline", sets=[k - 1, k], frames=2 * nf)
    for s in streams:
        assert rt.status(s.cuda_stream) == 0
    rt.accel_frames_in_flight(ds.accel, 1)

    # one caller-camera frame of the same scene
    cam = np.array(rt.look_at((20.0, 120.0, 15.0), (400.0, 90.0, 0.0), (0.0, 1.0, 0.0), 1.0, w, h).cam14(), np.float32)
    px = torch.zeros((h, w), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    rt.render_camera(ds.accel, cam, w, h, 0, h, params(LIGHT), px.data_ptr(), 1, None, None, None, s)
    assert rt.status(s) == 0
    report("camera", frames=1)
    ds.close()

    # bunny-class frame
    sc = vrt.scene.procedural("bunny", 6, 0, 1)
    ds = vrt.tracer.DeviceScene(sc, dev)
    px = torch.zeros((1024, 1024), dtype=torch.int32, device=dev)
    rt.render(ds.accel, 1024, 1024, 0, 1024, params((20.0, 260.0, -150.0)), px.data_ptr(), 1, None, None, None, s)
    assert rt.status(s) == 0
    report("bunny", frames=1, ident_root_kernels=rt.accel_info(ds.accel, 5))
    ds.close()


if __name__ == "__main__":
    main()
