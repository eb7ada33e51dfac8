"""Ambient-occlusion and diffuse-bounce frames from a camera against their fixed-camera forms, alternating in one process: the
1,048,576-triangle atrium at 1920x1080, the camera scene.rc_camera_like_rtu (it frames what the fixed camera frames).
  gi_fixed   vxrt_render_diffuse_bounce            gi_camera   vxrt_render_diffuse_bounce_camera
  ao_fixed   vxrt_render_ao, 16 spp                ao_camera   vxrt_render_ao_camera, 16 spp (tmax = 0.25 scene radius)
Each round times `--frames` frames of every form back to back (events on the stream); prints the median ms per frame of each form, the
camera / fixed ratios and the run-to-run spread of the fixed forms ((max - min) / median over the rounds) as one JSON line.

    python tools/camera_secondary_time.py [--rounds 12] [--warmup 3] [--frames 5]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("at least 10 alternating rounds")
    import numpy as np
    import torch
    vrt = importlib.import_module("vortex-raytracing_amd")
    rtapi = vrt.rtapi
    w, h, spp = 1920, 1080, 16
    sc = vrt.scene.procedural("atrium", 8, 0, 3)
    assert sc.n_tris == 1048576
    ds = vrt.tracer.DeviceScene(sc, "cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    b = sc.bounds
    radius = 0.25 * 0.5 * float(np.linalg.norm(np.array(b[3:]) - np.array(b[:3])))
    p = rtapi.default_shade_params()
    cam = rtapi.Camera.from_cam14(vrt.scene.rc_camera_like_rtu(w, h))
    px = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    forms = {
        "gi_fixed": lambda c: rtapi.render_diffuse_bounce(ds.accel, w, h, 0, h, p, px.data_ptr(), 3, None, c, s),
        "gi_camera": lambda c: rtapi.render_diffuse_bounce_camera(ds.accel, cam, w, h, 0, h, p, px.data_ptr(), 3, None, c, s),
        "ao_fixed": lambda c: rtapi.render_ao(ds.accel, w, h, 0, h, p, spp, radius, px.data_ptr(), 7, None, None, c, s),
        "ao_camera": lambda c: rtapi.render_ao_camera(ds.accel, cam, w, h, 0, h, p, spp, radius, px.data_ptr(), 7, None, None, c, s),
    }

    def run(kind):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.frames):
            forms[kind](None)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.frames

    rays = {}
    for kind in forms:       # rays traced per frame (its own call: the counter is not part of the timed frames)
        cnt.zero_()
        forms[kind](cnt.data_ptr())
        torch.cuda.synchronize()
        rays[kind] = int(cnt.item())
    for _ in range(a.warmup):
        for kind in forms:
            run(kind)
    ms = {kind: [] for kind in forms}
    for _ in range(a.rounds):
        for kind in forms:
            ms[kind].append(run(kind))
    assert rtapi.status(s) == 0
    out = {kind: {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)), "rays_per_frame": rays[kind]} for kind, v in ms.items()}
    for k in ("gi", "ao"):
        f = out[k + "_fixed"]
        out[k + "_camera_over_fixed_time"] = out[k + "_camera"]["ms_median"] / f["ms_median"]
        out[k + "_fixed_spread"] = (f["ms_max"] - f["ms_min"]) / f["ms_median"]
    print(json.dumps({"tool": "camera_secondary_time", "width": w, "height": h, "ao_spp": spp, "ao_radius": radius, "frames_per_round": a.frames,
                      "rounds": a.rounds, "warmup": a.warmup, **out}))
    ds.close()


if __name__ == "__main__":
    main()
