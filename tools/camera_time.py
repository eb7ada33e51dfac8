"""Camera frames against the fixed-camera frame, alternating in one process: the 1,048,576-triangle atrium, 1920x1080 with shadow
rays, sets of 5 frames in one set of launches.
  fixed    vxrt_render_batch (the RTU test's fixed camera: what bench.py times)
  like     vxrt_render_batch_camera from scene.rc_camera_like_rtu (about the same view)
  orbit    vxrt_render_batch_camera, the camera orbiting the scene (a new view every frame)
Prints Grays/s of each (rays traced / wall time of the set, median over the rounds) as one JSON line.

    python tools/camera_time.py [--rounds 12] [--warmup 3]
"""
import argparse
import importlib
import json
import math
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
    import numpy as np
    import torch
    vrt = importlib.import_module("vortex-raytracing_amd")
    w, h, nf = 1920, 1080, a.frames
    sc = vrt.scene.procedural("atrium", 8, 0, 3)
    ds = vrt.tracer.DeviceScene(sc, "cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    plist = []
    for f in range(nf):
        p = vrt.rtapi.default_shade_params()
        p.light_pos[:] = (10.0 * math.cos(0.3 * f), 10.0, -10.0 + 2.0 * f)
        plist.append(p)
    like = [np.array(vrt.scene.rc_camera_like_rtu(w, h), np.float32)] * nf
    buf = torch.zeros((nf, h, w), dtype=torch.int32, device="cuda:0")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def orbit(k):
        cams = []
        for f in range(nf):
            ang = 0.05 * (k * nf + f)
            eye = (300.0 * math.cos(ang), 120.0, 300.0 * math.sin(ang))
            cams.append(vrt.rtapi.look_at(eye, (0.0, 60.0, 0.0), (0.0, 1.0, 0.0), 1.0, w, h))
        return cams

    def run(kind, k):
        cnt.zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cams = orbit(k) if kind == "orbit" else like
        e0.record()
        if kind == "fixed":
            vrt.rtapi.render_batch(ds.accel, w, h, plist, buf.data_ptr(), h * w, 1, cnt.data_ptr(), s)
        else:
            vrt.rtapi.render_batch_camera(ds.accel, w, h, cams, plist, buf.data_ptr(), h * w, 1, cnt.data_ptr(), s)
        e1.record()
        torch.cuda.synchronize()
        return int(cnt.item()) / (e0.elapsed_time(e1) * 1e-3) / 1e9

    kinds = ("fixed", "like", "orbit")
    for k in range(a.warmup):
        for kind in kinds:
            run(kind, k)
    rates = {kind: [] for kind in kinds}
    for k in range(a.rounds):
        for kind in kinds:
            rates[kind].append(run(kind, k))
    assert vrt.rtapi.status(s) == 0
    out = {kind: {"grays_s_median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for kind, v in rates.items()}
    out["like_over_fixed"] = out["like"]["grays_s_median"] / out["fixed"]["grays_s_median"]
    out["orbit_over_fixed"] = out["orbit"]["grays_s_median"] / out["fixed"]["grays_s_median"]
    print(json.dumps({"tool": "camera_time", "width": w, "height": h, "frames_per_set": nf, "shadow": 1, **out}))
    ds.close()


if __name__ == "__main__":
    main()
