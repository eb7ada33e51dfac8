"""Multiple importance sampling of area lights timed and measured: the 1,048,576-triangle atrium at 1920x1080, 3 bounces x 4 spp,
shadow = 1, a static camera, everything in one process, for two emitter placements:
  small   tools/emissive_time.py's: the 64 largest downward-facing triangles under the roof made emissive -- small, far lights, where
          emitter sampling (nee = 1) is the good estimator;
  panel   one large emissive panel `--gap` units below the highest surface of the scene, over the middle half of its footprint: the
          atrium's counterpart of the test hall's gap, where a vertex next to the panel gives nee = 1 an unbounded sample.

Timing -- alternating rounds of `--frames` frames per form, events on the stream, median ms per frame and spread ((max - min) / median):
  nee1            vxrt_render_path_emissive, nee = 1
  mis             vxrt_render_path_emissive_mis         the same launches with the weighted bounce-ray and scatter kernels
Error -- RMSE of the colours (all pixels, 3 channels) of both, and of nee = 0, at 4 spp against a `--reference-spp` nee = 0 frame, and the
largest colour component of each frame (a firefly shows there).
Index -- host wall time of the call that builds the emitter index (vxrt_emitter_hit_weights on one record, after vxrt_accel_set_emitters)
for 4,097 and 65,536 pairs, median of `--index-runs`, and of the same call with the index held.
One JSON line.  `--trace-frames K` renders K frames of nee1 and K of mis on `--placement` and nothing else (for a kernel trace in a run
of its own).

    python tools/emissive_mis_time.py [--rounds 12] [--warmup 3] [--frames 5]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KEYS = ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")


def panel_atrium(vrt, np, gap, le=(6.0, 5.5, 4.0)):
    """the atrium, untextured, as instance 0 and, as instance 1, a two-triangle emissive panel `gap` units below the top of the scene's box over the
    middle half of its footprint, facing down; the (blasIdx, triIdx) pairs of the panel"""
    sc = vrt.scene.procedural("atrium", 8, 0, 3)
    assert sc.n_tris == 1048576 and sc.n_blas == 1
    tri = sc.buffers["tri"].view(np.float32).reshape(-1, 9)
    x0, y0, z0, x1, y1, z1 = (float(v) for v in sc.bounds)
    xa, xb, za, zb, y = x0 + 0.25 * (x1 - x0), x0 + 0.75 * (x1 - x0), z0 + 0.25 * (z1 - z0), z0 + 0.75 * (z1 - z0), y1 - gap
    panel = np.array([[xa, y, za, xb, y, za, xb, y, zb], [xa, y, za, xb, y, zb, xa, y, zb]], np.float32)
    ex = np.zeros((2, 16), np.float32)
    ex[:, 1] = ex[:, 4] = ex[:, 7] = -1.0           # the shading normal three times: down
    ex[:, 11] = ex[:, 14] = 1.0                      # uv1 = (1, 0), uv2 = (0, 1); texId 0 of the panel's own material
    m = sc.buffers["mat"][:88].copy()
    m.view(np.float32)[3:6] = (0.8, 0.8, 0.8)
    m.view(np.float32)[9:12] = le
    m.view(np.int32)[16] = -1                        # diffuse_tex_id: none
    mats = sc.buffers["mat"].copy()
    mats.view(np.int32).reshape(-1, 22)[:, 16] = -1   # (scene.from_triangles keeps no textures: the atrium's materials lose theirs)
    out = vrt.scene.from_triangles([tri, panel], None, [sc.buffers["triEx"], ex.view(np.uint8).reshape(-1)], [mats, m])
    b = {k: v.copy() for k, v in out.buffers.items()}
    pairs = np.array([[1, sc.n_tris], [1, sc.n_tris + 1]], np.uint32)
    return out, b, pairs


def all_emissive_atrium(vrt, np, n=65536):
    """the atrium with every material emissive, and n of its triangles with an area as pairs: a table to time the index on"""
    sc = vrt.scene.procedural("atrium", 8, 0, 3)
    b = {k: v.copy() for k, v in sc.buffers.items()}
    b["mat"].view(np.float32).reshape(-1, 22)[:, 9:12] = 1.0
    tri = b["tri"].view(np.float32).reshape(-1, 3, 3)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    idx = np.nonzero(area > 0)[0]
    idx = idx[np.random.default_rng(1).permutation(len(idx))[:n]]
    assert len(idx) == n
    return b, np.stack([np.zeros(n, np.uint32), idx.astype(np.uint32)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--lights", type=int, default=64)
    ap.add_argument("--gap", type=float, default=3.0)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--index-runs", type=int, default=9)
    ap.add_argument("--placement", choices=("small", "panel", "both"), default="both")
    ap.add_argument("--trace-frames", type=int, default=0)
    a = ap.parse_args()
    if a.rounds < 10 and not a.trace_frames:
        ap.error("at least 10 alternating rounds")
    import numpy as np
    import torch
    from emissive_time import lit_atrium
    vrt = importlib.import_module("vortex-raytracing_amd")
    rtapi = vrt.rtapi
    w, h = 1920, 1080
    dev = "cuda:0"
    s = torch.cuda.current_stream().cuda_stream
    p = rtapi.default_shade_params()
    cam = rtapi.Camera.from_cam14(vrt.scene.rc_camera_like_rtu(w, h))
    spp, bounces, shadow, seed = 4, 3, 1, 3
    px = torch.zeros((h, w), dtype=torch.int32, device=dev)
    col = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    em = {0: rtapi.EmissiveParams(0, 1.0, (rtapi.C.c_uint32 * 2)(0, 0)), 1: rtapi.EmissiveParams(1, 1.0, (rtapi.C.c_uint32 * 2)(0, 0)),
          "mis": rtapi.EmissiveMisParams(1.0, (rtapi.C.c_uint32 * 3)(0, 0, 0))}

    def summary(v):
        return {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)),
                "spread": float((np.max(v) - np.min(v)) / abs(np.median(v)))}

    def measure(ds):
        def frame(kind, n_spp=spp, sd=seed, colors=None, count=None):
            if kind == "mis":
                rtapi.render_path_emissive_mis(ds.accel, cam, w, h, 0, h, p, n_spp, bounces, em["mis"], px.data_ptr(), sd, shadow, colors, count, s)
            else:
                rtapi.render_path_emissive(ds.accel, cam, w, h, 0, h, p, n_spp, bounces, em[kind], px.data_ptr(), sd, shadow, colors, count, s)

        kinds = (1, "mis")
        if a.trace_frames:
            for kind in kinds:
                for _ in range(a.trace_frames):
                    frame(kind)
            torch.cuda.synchronize()
            assert rtapi.status(s) == 0
            return None

        def run(kind):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.frames):
                frame(kind)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.frames

        for _ in range(a.warmup):
            for kind in kinds:
                run(kind)
        ms = {kind: [] for kind in kinds}
        for _ in range(a.rounds):
            for kind in kinds:
                ms[kind].append(run(kind))
        assert rtapi.status(s) == 0
        out = {"nee1": summary(ms[1]), "mis": summary(ms["mis"]), "mis_minus_nee1": summary([u - v for u, v in zip(ms["mis"], ms[1])])}
        out["mis_minus_nee1"]["ratio"] = float(np.median(ms["mis"]) / np.median(ms[1]))
        ref = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        frame(0, a.reference_spp, 1000003, ref.data_ptr())
        torch.cuda.synchronize()
        err = {}
        for kind, name in ((0, "nee0"), (1, "nee1"), ("mis", "mis")):
            rays.zero_()
            frame(kind, spp, seed, col.data_ptr(), rays.data_ptr())
            torch.cuda.synchronize()
            err[name] = {"spp": spp, "rays_traced": int(rays.item()), "rmse": float(torch.sqrt(torch.mean((col - ref) ** 2)).item()),
                         "largest_component": float(col.max().item())}
        out["error"] = dict(err, reference_spp=a.reference_spp, reference_largest_component=float(ref.max().item()))
        return out

    result = {}
    if a.placement in ("small", "both"):
        _, b, pairs = lit_atrium(vrt, np, a.lights)
        ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, dev)
        ds.set_emitters(pairs)
        result["small"] = measure(ds)
        ds.close()
    if a.placement in ("panel", "both"):
        _, b, pairs = panel_atrium(vrt, np, a.gap)
        ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, dev)
        ds.set_emitters(pairs)
        result["panel"] = measure(ds)
        ds.close()
    if a.trace_frames:
        return

    # ---- the index: the call that builds it, and the same call with the index held ----
    b2, pairs2 = all_emissive_atrium(vrt, np)
    ds2 = vrt.tracer.DeviceScene({k: b2[k] for k in KEYS}, dev)
    rec = [torch.zeros(8, dtype=torch.float32, device=dev) for _ in range(5)]   # one ray, one hit record, one normal, e, wB
    index = {}
    for n in (4097, 65536):
        sub = pairs2[np.random.default_rng(n).permutation(len(pairs2))[:n]]
        build, held = [], []
        for _ in range(a.index_runs):
            ds2.set_emitters(sub)
            assert rtapi.accel_info(ds2.accel, 8) == 0
            for t in (build, held):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rtapi.emitter_hit_weights(ds2.accel, 1, *(t.data_ptr() for t in rec), s)
                t.append((time.perf_counter() - t0) * 1e3)
            assert rtapi.accel_info(ds2.accel, 8) == n
        index[str(n)] = {"build": summary(build), "held": summary(held)}
    torch.cuda.synchronize()
    assert rtapi.status(s) == 0
    ds2.close()
    print(json.dumps({"tool": "emissive_mis_time", "width": w, "height": h, "spp": spp, "bounces": bounces, "shadow": shadow, "lights": a.lights, "gap": a.gap,
                      "frames_per_round": a.frames, "rounds": a.rounds, "warmup": a.warmup, **result, "index_host_ms": index}))


if __name__ == "__main__":
    main()
