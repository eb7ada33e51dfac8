"""Temporal accumulation timed on the 1,048,576-triangle atrium at 1920x1080 along a slow orbit (the camera scene.rc_camera_like_rtu turned
about the vertical axis through the scene's centre, `--degrees` per frame), alternating in one process (path configuration: 3 bounces x
4 spp, shadow = 1; filter: 5 iterations):
  path            vxrt_render_path
  denoised4       vxrt_render_path_denoised with one iteration less
  denoised        vxrt_render_path_denoised
  temporal        vxrt_render_path_temporal (the same filter behind the accumulation pass)
Every form renders the same cameras.  Each round times `--frames` frames of every form back to back (events on the stream); prints the
median ms per frame and the spread ((max - min) / median over the rounds) of each form, the accumulation pass's own time (temporal -
denoised, per round, median and spread), the yardsticks measured in the same run -- the mean a-trous iteration ((denoised - path) /
iterations) and the last one (denoised - denoised4) -- and the bytes per frame the pass moves at the least (160 B per pixel: E, P, N in; the
signal and the three history entries out; the previous HE, HP, HN once each) with the rate that makes of its time, as one JSON line.

    python tools/temporal_time.py [--rounds 12] [--warmup 3] [--frames 5] [--iterations 5] [--degrees 0.2]
"""
import argparse
import importlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def orbit(cam14, centre, degrees):
    """the camera turned rigidly about the vertical axis through `centre`"""
    a = math.radians(degrees)
    ca, sa = math.cos(a), math.sin(a)

    def rot(v):
        return [ca * v[0] + sa * v[2], v[1], -sa * v[0] + ca * v[2]]
    c = [float(v) for v in cam14]
    pos = rot([c[0] - centre[0], c[1] - centre[1], c[2] - centre[2]])
    return [pos[0] + centre[0], pos[1] + centre[1], pos[2] + centre[2]] + rot(c[3:6]) + rot(c[6:9]) + rot(c[9:12]) + c[12:14]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--degrees", type=float, default=0.2)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("at least 10 alternating rounds")
    if a.iterations < 1:
        ap.error("at least one iteration")
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
    b = sc.bounds
    centre = [0.5 * (b[k] + b[k + 3]) for k in range(3)]
    extent = float(np.linalg.norm(np.array(b[3:]) - np.array(b[:3])))
    cam0 = vrt.scene.rc_camera_like_rtu(w, h)
    n_cams = a.frames * (a.rounds + a.warmup + 1)
    cams = [rtapi.Camera.from_cam14(orbit(cam0, centre, a.degrees * k)) for k in range(n_cams)]
    px = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    hist_out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    dn = rtapi.DenoiseParams(a.iterations, 5, extent / 250.0, 0.25)
    dn4 = rtapi.DenoiseParams(a.iterations - 1, 5, extent / 250.0, 0.25)
    tp = rtapi.TemporalParams(0.1, 32, extent / 250.0, 0.9)
    history = rtapi.History(w, h)
    forms = {
        "path": lambda c: rtapi.render_path(ds.accel, c, w, h, 0, h, p, 4, 3, px.data_ptr(), 3, 1, None, None, s),
        "denoised4": lambda c: rtapi.render_path_denoised(ds.accel, c, w, h, 0, h, p, 4, 3, dn4, px.data_ptr(), 3, 1, None, None, None, s),
        "denoised": lambda c: rtapi.render_path_denoised(ds.accel, c, w, h, 0, h, p, 4, 3, dn, px.data_ptr(), 3, 1, None, None, None, s),
        "temporal": lambda c: rtapi.render_path_temporal(ds.accel, c, w, h, 0, h, p, 4, 3, dn, tp, history, px.data_ptr(), 3, 1, None, None, None, s),
    }

    def run(kind, first):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.frames):
            forms[kind](cams[first + k])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.frames

    first = 0
    for _ in range(a.warmup):
        for kind in forms:
            run(kind, first)
        first += a.frames
    ms = {kind: [] for kind in forms}
    for _ in range(a.rounds):
        for kind in forms:
            ms[kind].append(run(kind, first))
        first += a.frames
    assert rtapi.status(s) == 0
    history.read(hist_out.data_ptr(), s)
    torch.cuda.synchronize()
    hh = hist_out.cpu().numpy()
    hit = hh[..., 3] > 0

    def summary(v):
        return {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)),
                "spread": float((np.max(v) - np.min(v)) / abs(np.median(v)))}
    out = {kind: summary(v) for kind, v in ms.items()}
    diff = lambda x, y: [u - v for u, v in zip(ms[x], ms[y])]
    out["accumulation_pass"] = summary(diff("temporal", "denoised"))
    out["last_iteration"] = summary(diff("denoised", "denoised4"))
    out["mean_iteration"] = summary([d / a.iterations for d in diff("denoised", "path")])
    t = out["accumulation_pass"]["ms_median"]
    req = 160 * w * h
    out["accumulation_pass"].update({"least_bytes_per_frame": req, "least_tb_per_s": req / (t * 1e-3) / 1e12 if t > 0 else None})
    out["history"] = {"hit_pixels": int(hit.sum()), "mean_length": float(hh[..., 3][hit].mean()), "at_max_length": int((hh[..., 3] == tp.max_len).sum())}
    print(json.dumps({"tool": "temporal_time", "width": w, "height": h, "iterations": a.iterations, "degrees_per_frame": a.degrees,
                      "temporal_params": [tp.alpha_min, tp.max_len, tp.sigma_z, tp.normal_min], "frames_per_round": a.frames, "rounds": a.rounds,
                      "warmup": a.warmup, **out}))
    history.close()
    ds.close()


if __name__ == "__main__":
    main()
