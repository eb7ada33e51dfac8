"""Emissive geometry timed and measured: the 1,048,576-triangle atrium at 1920x1080 with its largest downward-facing triangles in the upper
part of the scene given an emissive material, 3 bounces x 4 spp, shadow = 1, a static camera, everything in one process.

Timing -- alternating rounds of `--frames` frames per form, events on the stream, median ms per frame and spread ((max - min) / median):
  path            vxrt_render_path                      the frame without emissive geometry
  nee0            vxrt_render_path_emissive, nee = 0    emission at the prepare launch and at bounce hits: no launch more
  nee1            vxrt_render_path_emissive, nee = 1    one emitter ray per live path and depth: a wider ray launch and one any-hit trace more
Payoff -- RMSE of the colours (all pixels, 3 channels) against a `--reference-spp` nee = 0 frame, for nee = 1 at 4 spp and for nee = 0 at the
spp whose traced rays come closest to nee = 1's (both ray counts are reported).
Table -- vxrt_accel_set_emitters for 2 and for 4,097 emitters, host wall time of the synchronous call, median of `--table-runs`.
One JSON line.  `--trace-frames K` renders K frames of path and K of nee1 and nothing else (for a kernel trace in a run of its own).

    python tools/emissive_time.py [--rounds 12] [--warmup 3] [--frames 5]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lit_atrium(vrt, np, n_lights, le=(40.0, 36.0, 28.0)):
    """the atrium's buffers with a second material (emissive) on the n_lights largest triangles that face down and lie in the upper 40 %
    of the scene's height; the (blasIdx, triIdx) pairs of those triangles"""
    sc = vrt.scene.procedural("atrium", 8, 0, 3)
    assert sc.n_tris == 1048576 and sc.n_blas == 1
    b = {k: v.copy() for k, v in sc.buffers.items()}
    tri = b["tri"].view(np.float32).reshape(-1, 3, 3)
    c = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = 0.5 * np.linalg.norm(c, axis=1)
    ex = b["triEx"].view(np.float32).reshape(-1, 16)
    y = tri[:, :, 1].mean(1)
    lo, hi = float(sc.bounds[1]), float(sc.bounds[4])
    ok = (ex[:, 1] < -0.9) & (y > lo + 0.6 * (hi - lo)) & (area > 0)
    if ok.sum() < n_lights:
        ok = (y > lo + 0.6 * (hi - lo)) & (area > 0)
    idx = np.nonzero(ok)[0]
    idx = np.sort(idx[np.argsort(-area[idx])[:n_lights]])
    n_mats = b["mat"].size // 88
    m = b["mat"][:88].copy()
    m.view(np.float32)[9:12] = le
    b["mat"] = np.concatenate([b["mat"], m])
    b["triEx"].view(np.uint32).reshape(-1, 16)[idx, 15] = n_mats
    pairs = np.stack([np.zeros(len(idx), np.uint32), idx.astype(np.uint32)], 1)
    return sc, b, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--lights", type=int, default=64)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--table-runs", type=int, default=9)
    ap.add_argument("--trace-frames", type=int, default=0)
    a = ap.parse_args()
    if a.rounds < 10 and not a.trace_frames:
        ap.error("at least 10 alternating rounds")
    import numpy as np
    import torch
    vrt = importlib.import_module("vortex-raytracing_amd")
    rtapi = vrt.rtapi
    w, h = 1920, 1080
    dev = "cuda:0"
    sc, b, pairs = lit_atrium(vrt, np, a.lights)
    keys = ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")
    ds = vrt.tracer.DeviceScene({k: b[k] for k in keys}, dev)
    ds.set_emitters(pairs)
    s = torch.cuda.current_stream().cuda_stream
    p = rtapi.default_shade_params()
    cam = rtapi.Camera.from_cam14(vrt.scene.rc_camera_like_rtu(w, h))
    spp, bounces, shadow, seed = 4, 3, 1, 3
    px = torch.zeros((h, w), dtype=torch.int32, device=dev)
    col = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    two = rtapi.C.c_uint32 * 2
    em = {0: rtapi.EmissiveParams(0, 1.0, two(0, 0)), 1: rtapi.EmissiveParams(1, 1.0, two(0, 0))}

    def emissive(nee, n_spp=spp, sd=seed, colors=None, count=None):
        rtapi.render_path_emissive(ds.accel, cam, w, h, 0, h, p, n_spp, bounces, em[nee], px.data_ptr(), sd, shadow, colors, count, s)

    forms = {
        "path": lambda: rtapi.render_path(ds.accel, cam, w, h, 0, h, p, spp, bounces, px.data_ptr(), seed, shadow, None, None, s),
        "nee0": lambda: emissive(0),
        "nee1": lambda: emissive(1),
    }
    if a.trace_frames:
        for kind in ("path", "nee1"):
            for _ in range(a.trace_frames):
                forms[kind]()
        torch.cuda.synchronize()
        assert rtapi.status(s) == 0
        ds.close()
        return

    def run(kind):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.frames):
            forms[kind]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.frames

    for _ in range(a.warmup):
        for kind in forms:
            run(kind)
    ms = {kind: [] for kind in forms}
    for _ in range(a.rounds):
        for kind in forms:
            ms[kind].append(run(kind))
    assert rtapi.status(s) == 0

    def summary(v):
        return {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)),
                "spread": float((np.max(v) - np.min(v)) / abs(np.median(v)))}
    out = {kind: summary(v) for kind, v in ms.items()}
    for kind in ("nee0", "nee1"):
        out[kind + "_minus_path"] = summary([u - v for u, v in zip(ms[kind], ms["path"])])
        out[kind + "_minus_path"]["ratio"] = float(np.median(ms[kind]) / np.median(ms["path"]))

    # ---- the payoff at equal traced rays ----
    def traced(nee, n_spp, sd):
        rays.zero_()
        emissive(nee, n_spp, sd, col.data_ptr(), rays.data_ptr())
        torch.cuda.synchronize()
        return int(rays.item())

    ref = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    rays.zero_()
    rtapi.render_path_emissive(ds.accel, cam, w, h, 0, h, p, a.reference_spp, bounces, em[0], px.data_ptr(), 1000003, shadow, ref.data_ptr(), None, s)
    torch.cuda.synchronize()
    rmse = lambda: float(torch.sqrt(torch.mean((col - ref) ** 2)).item())
    r1 = traced(1, spp, seed)
    e1 = rmse()
    r0_4 = traced(0, spp, seed)
    e0_4 = rmse()
    spp0 = max(1, int(round(spp * (r1 - w * h) / max(r0_4 - w * h, 1))))
    r0 = traced(0, spp0, seed)
    e0 = rmse()
    out["payoff"] = {"reference_spp": a.reference_spp, "nee1": {"spp": spp, "rays_traced": r1, "rmse": e1}, "nee0_same_spp": {"spp": spp, "rays_traced": r0_4, "rmse": e0_4},
                     "nee0_equal_rays": {"spp": spp0, "rays_traced": r0, "rmse": e0}, "rays_ratio": r0 / r1, "rmse_ratio_nee1_over_nee0": e1 / e0}

    # ---- the table ----
    _, b2, pairs2 = lit_atrium(vrt, np, 4097)
    ds2 = vrt.tracer.DeviceScene({k: b2[k] for k in keys}, dev)
    table = {}
    for n in (2, 4097):
        t = []
        for _ in range(a.table_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds2.set_emitters(pairs2[:n])
            t.append((time.perf_counter() - t0) * 1e3)
        assert rtapi.accel_info(ds2.accel, 7) == n
        table[str(n)] = summary(t)
    out["table_build_host_ms"] = table
    ds2.close()
    assert rtapi.status(s) == 0
    print(json.dumps({"tool": "emissive_time", "width": w, "height": h, "spp": spp, "bounces": bounces, "shadow": shadow, "lights": int(len(pairs)),
                      "frames_per_round": a.frames, "rounds": a.rounds, "warmup": a.warmup, **out}))
    ds.close()


if __name__ == "__main__":
    main()
