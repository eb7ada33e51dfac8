"""Denoised path frames timed on the 1,048,576-triangle atrium at 1920x1080 from the camera scene.rc_camera_like_rtu, alternating in one
process (path configuration: 3 bounces x 4 spp, shadow = 1; filter: 5 iterations):
  path            vxrt_render_path
  denoised        vxrt_render_path_denoised
Each round times `--frames` frames of every form back to back (events on the stream); prints the median ms per frame and the spread
((max - min) / median over the rounds) of each form, the filter's own time (denoised - path) and share of the frame, and the bytes per
frame the filter's launches request from the vector-memory path, computed from the shapes (every pixel taken as a hit), with the rate
that makes of the filter's time, as one JSON line.  (The shipped iteration kernel is the plain gather: there is no second form to
compare it with.  The LDS-tiled form that lost is recorded in profiles/r10_a_denoise_time.txt.)

    python tools/denoise_time.py [--rounds 12] [--warmup 3] [--frames 5] [--iterations 5]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def requested_bytes(w, h, iterations):
    """bytes the filter's launches ask the vector-memory path for per frame: demodulate (acc, lit, alb, geo in; signal out), then per
    iteration three 16-byte arrays per tap (25 taps + the centre) and the output (a 16-byte signal; the last pass: lit and alb in, a
    4-byte pixel out)"""
    n = w * h
    total = n * (4 * 16 + 16)
    for i in range(iterations):
        total += n * 26 * 48 + n * (16 if i + 1 < iterations else 2 * 16 + 4)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("at least 10 alternating rounds")
    import numpy as np
    import torch
    vrt = importlib.import_module("vortex-raytracing_amd")
    rtapi = vrt.rtapi
    w, h = 1920, 1080
    sc = vrt.scene.procedural("atrium", 8, 0, 3)
    assert sc.n_tris == 1048576
    ds = vrt.tracer.DeviceScene(sc, "cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    p = rtapi.default_shade_params()
    cam = rtapi.Camera.from_cam14(vrt.scene.rc_camera_like_rtu(w, h))
    px = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    b = sc.bounds
    extent = float(np.linalg.norm(np.array(b[3:]) - np.array(b[:3])))
    dn = rtapi.DenoiseParams(a.iterations, 5, extent / 250.0, 0.25)
    forms = {
        "path": lambda: rtapi.render_path(ds.accel, cam, w, h, 0, h, p, 4, 3, px.data_ptr(), 3, 1, None, None, s),
        "denoised": lambda: rtapi.render_path_denoised(ds.accel, cam, w, h, 0, h, p, 4, 3, dn, px.data_ptr(), 3, 1, None, None, None, s),
    }

    def run(kind):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.frames):
            forms[kind]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.frames

    pixels = {}
    for kind in forms:
        forms[kind]()
        torch.cuda.synchronize()
        pixels[kind] = px.cpu().numpy().copy()
    for _ in range(a.warmup):
        for kind in forms:
            run(kind)
    ms = {kind: [] for kind in forms}
    for _ in range(a.rounds):
        for kind in forms:
            ms[kind].append(run(kind))
    assert rtapi.status(s) == 0
    out = {kind: {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)),
                  "spread": float((np.max(v) - np.min(v)) / np.median(v))} for kind, v in ms.items()}
    base = out["path"]["ms_median"]
    f = out["denoised"]["ms_median"] - base
    req = requested_bytes(w, h, a.iterations)
    out["denoised"].update({"filter_ms": f, "filter_share_of_frame": f / out["denoised"]["ms_median"], "requested_bytes_per_frame": req,
                            "requested_tb_per_s": req / (f * 1e-3) / 1e12 if f > 0 else None})
    out["pixels_changed_by_the_filter"] = int((pixels["denoised"] != pixels["path"]).sum())
    print(json.dumps({"tool": "denoise_time", "width": w, "height": h, "iterations": a.iterations, "normal_power": 5, "sigma_z": dn.sigma_z, "sigma_l": dn.sigma_l,
                      "frames_per_round": a.frames, "rounds": a.rounds, "warmup": a.warmup, **out}))
    ds.close()


if __name__ == "__main__":
    main()
