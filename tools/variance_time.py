"""Variance guidance timed as tools/temporal_time.py times the temporal frame: the 1,048,576-triangle atrium at 1920x1080 along the same
slow orbit (`--degrees` per frame), 3 bounces x 4 spp, shadow = 1, 5 iterations, alternating in one process:
  temporal        vxrt_render_path_temporal
  temporal0       ... with iterations = 0 (the step remodulates and packs)
  variance0       vxrt_render_path_variance with iterations = 0 and no variance output: the temporal0 frame with T_v for T
  variance0v      ... with the variance output: one launch more, the initial variance V0
  variance4       vxrt_render_path_variance with one iteration less
  variance        vxrt_render_path_variance
Every form renders the same cameras on a history of its own.  Each round times `--frames` frames of every form back to back (events on the
stream); prints the median ms per frame and the spread ((max - min) / median over the rounds) of each form and of the differences that
isolate the three new launches, as one JSON line:
  frame_cost      variance - temporal                       what the feature adds to a frame
  moments_in_step variance0 - temporal0                     T_v against T (the README's temporal step: 0.066 ms)
  initial         variance0v - variance0                    the V0 launch in a frame, most pixels with long histories
  last_pass       variance - variance4                      one atrous_v pass (the README's a-trous pass: 0.122 ms)
  mean_pass       (variance - variance0v) / iterations
and the V0 kernel alone (vxrt_history_variance, `--frames` launches between two events, as many rounds): on the orbit's history, where
nearly every pixel takes the temporal route, and on the first frame after a reset, where every pixel walks its window.

    python tools/variance_time.py [--rounds 12] [--warmup 3] [--frames 5] [--iterations 5] [--degrees 0.2]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from temporal_time import orbit  # noqa: E402


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
    n_cams = a.frames * (a.rounds + a.warmup + 2)
    cams = [rtapi.Camera.from_cam14(orbit(cam0, centre, a.degrees * k)) for k in range(n_cams)]
    px = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    var = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    out4 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    sz = extent / 250.0
    dn, dn0 = rtapi.DenoiseParams(a.iterations, 5, sz, 0.25), rtapi.DenoiseParams(0, 5, sz, 0.25)
    dv, dv4, dv0 = rtapi.DenoiseParams(a.iterations, 5, sz, 4.0), rtapi.DenoiseParams(a.iterations - 1, 5, sz, 4.0), rtapi.DenoiseParams(0, 5, sz, 4.0)
    tp = rtapi.TemporalParams(0.1, 32, sz, 0.9)
    vp = rtapi.VarianceParams(1e-3, 4, 2, 0)
    plain = {k: rtapi.History(w, h) for k in ("temporal", "temporal0")}
    mom = {k: rtapi.History(w, h, moments=True) for k in ("variance0", "variance0v", "variance4", "variance")}

    def temporal(kind, d):
        return lambda c: rtapi.render_path_temporal(ds.accel, c, w, h, 0, h, p, 4, 3, d, tp, plain[kind], px.data_ptr(), 3, 1, None, None, None, s)

    def variance(kind, d, v=None):
        return lambda c: rtapi.render_path_variance(ds.accel, c, w, h, 0, h, p, 4, 3, d, tp, vp, mom[kind], px.data_ptr(), 0, 3, 1, None, None, None, v, None, s)
    forms = {"temporal": temporal("temporal", dn), "temporal0": temporal("temporal0", dn0), "variance0": variance("variance0", dv0),
             "variance0v": variance("variance0v", dv0, var.data_ptr()), "variance4": variance("variance4", dv4), "variance": variance("variance", dv)}

    def run(kind, first):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.frames):
            forms[kind](cams[first + k])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.frames

    def v0_alone(hist):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.frames):
            rtapi.history_variance(hist, dv, vp, var.data_ptr(), s)
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
    hist = mom["variance"]
    hist.read(out4.data_ptr(), s)
    torch.cuda.synchronize()
    hh = out4.cpu().numpy()
    hit = hh[..., 3] > 0
    long_v0 = [v0_alone(hist) for _ in range(a.rounds + a.warmup)][a.warmup:]
    hist.reset()
    forms["variance"](cams[first])
    short_v0 = [v0_alone(hist) for _ in range(a.rounds + a.warmup)][a.warmup:]
    assert rtapi.status(s) == 0

    def summary(v):
        return {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)),
                "spread": float((np.max(v) - np.min(v)) / abs(np.median(v)))}
    out = {kind: summary(v) for kind, v in ms.items()}
    diff = lambda x, y: [u - v for u, v in zip(ms[x], ms[y])]
    out["frame_cost"] = summary(diff("variance", "temporal"))
    out["moments_in_step"] = summary(diff("variance0", "temporal0"))
    out["initial"] = summary(diff("variance0v", "variance0"))
    out["last_pass"] = summary(diff("variance", "variance4"))
    out["mean_pass"] = summary([d / a.iterations for d in diff("variance", "variance0v")])
    out["initial_alone_long_histories"] = summary(long_v0)
    out["initial_alone_after_reset"] = summary(short_v0)
    out["history"] = {"hit_pixels": int(hit.sum()), "mean_length": float(hh[..., 3][hit].mean()),
                      "below_min_len": int((hit & (hh[..., 3] < vp.min_len)).sum())}
    print(json.dumps({"tool": "variance_time", "width": w, "height": h, "iterations": a.iterations, "degrees_per_frame": a.degrees,
                      "temporal_params": [tp.alpha_min, tp.max_len, tp.sigma_z, tp.normal_min], "variance_params": [vp.epsilon, vp.min_len, vp.radius],
                      "sigma_l": [dn.sigma_l, dv.sigma_l], "frames_per_round": a.frames, "rounds": a.rounds, "warmup": a.warmup, **out}))
    for hst in list(plain.values()) + list(mom.values()):
        hst.close()
    ds.close()


if __name__ == "__main__":
    main()
