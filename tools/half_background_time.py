#!/usr/bin/env python3
"""A synthetic shadow frame in which every 8x8 tile is about half background (the one trade of RT_TILE_PHASES / RT_TILE_REFILL_MIN: such
a tile's occlusion phase runs with the lanes that missed empty).

The fixed camera ((0,100,0), looking along +x) sees, in the plane x = 400, vertical strips over 4 of every 8 pixel columns of the
1920x1080 frame, each cut into 135 cells of two triangles (64,800 triangles); behind the camera a tessellated blocker hides the light
from half of the plane.  Serial frames, timed with events; one JSON line.  Compare libraries with VXRT_LIB_DIR.

    python tools/half_background_time.py [--steps 50] [--rounds 3]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quad_x(x, y0, y1, z0, z1):
    return [[x, y0, z0, x, y1, z0, x, y1, z1], [x, y0, z0, x, y1, z1, x, y0, z1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    vrt = importlib.import_module("vortex-raytracing_amd")
    rt = vrt.rtapi
    w, h, X = 1920, 1080, 400.0
    # the camera ray of pixel (x, y) has direction (1, +-v, u) with u = (2 x - w) / h, v = (2 y - h) / h: it meets the plane at z = X u
    zedge = lambda x: X * (2.0 * (x - 0.5) - w) / h
    ys = np.linspace(100.0 - 1.1 * X, 100.0 + 1.1 * X, 136)
    tris = []
    for k in range(w // 8):
        z0, z1 = zedge(8 * k), zedge(8 * k + 4)
        for j in range(135):
            tris.extend(quad_x(X, float(ys[j]), float(ys[j + 1]), z0, z1))
    g = np.linspace(0.0, 1000.0, 65)
    gy = np.linspace(-1000.0, 1200.0, 65)
    for i in range(64):
        for j in range(64):
            tris.extend(quad_x(-100.0, float(gy[j]), float(gy[j + 1]), float(g[i]), float(g[i + 1])))
    sc = vrt.scene.from_triangles([np.array(tris, np.float32)])
    ds = vrt.tracer.DeviceScene(sc, "cuda:0")
    p = rt.default_shade_params()
    p.light_pos[:] = (-300.0, 100.0, 0.0)
    px = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    rt.render(ds.accel, w, h, 0, h, p, px.data_ptr(), 1, None, None, cnt.data_ptr(), s)
    torch.cuda.synchronize()
    assert rt.status(s) == 0
    rays = int(cnt.item())
    frame = lambda: rt.render(ds.accel, w, h, 0, h, p, px.data_ptr(), 1, None, None, None, s)
    ms = []
    for _ in range(a.rounds):
        for _ in range(5):
            frame()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            frame()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.steps)
    print(json.dumps({"tool": "half_background_time", "lib": os.environ.get("VXRT_LIB_DIR", ""), "tris": len(tris), "ident_root_kernels": rt.accel_info(ds.accel, 5),
                      "rays_per_frame": rays, "hit_fraction": round(rays / (w * h) - 1.0, 3),   # (one occlusion ray per pixel that hits)
                      "ms_per_frame_serial": [round(m, 4) for m in ms], "mrays_s": round(rays / min(ms) / 1e3, 1)}))
    ds.close()


if __name__ == "__main__":
    main()
