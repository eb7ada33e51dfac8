"""Refit against the rebuild it replaces, device-event timed, side by side in one process (DESIGN.md s2 "Refit").
  (a) vxrt_accel_refit(GEOMETRY) on the atrium (1,048,576 triangles, CPU-built tree) and on the 10 M-triangle hairball (GPU-built)
  (b) vxrt_accel_set_transforms + refit on a 1,000-instance scene
  (c) the rebuilds: vxrt_bvh_build + vxrt_accel_build (a's), host instance boxes + vxrt_tlas_build + vxrt_accel_build (b's)
and the atrium's headline frame (1920x1080, shadow rays) before and after a zero-motion refit of its CPU-built tree.
Each figure: median of --reps timed runs after --warmup untimed ones.  usage: python tools/refit_time.py [--reps 10] [--no-hairball] [--out f.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

vrt = importlib.import_module("vortex-raytracing_amd")
rt = vrt.rtapi


def timed(fn, reps, warmup):
    s = torch.cuda.current_stream()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(out)), "min_ms": float(np.min(out)), "max_ms": float(np.max(out)), "reps": reps}


def stream():
    return torch.cuda.current_stream().cuda_stream


def rebuild_blas(ds, n_tris):
    """vxrt_bvh_build of the scene's one mesh into a scratch node buffer + vxrt_accel_build on the result (then freed)."""
    nodes = torch.zeros(2 * n_tris * 52, dtype=torch.uint8, device="cuda:0")
    tri = ds.t["tri"].clone()
    ex = ds.t["triEx"].clone()

    def run():
        info = rt.bvh_build(tri.data_ptr(), ex.data_ptr(), n_tris, nodes.data_ptr(), 2 * n_tris, 0, 0, stream())
        s = rt.VxrtScene()
        for k in ("tlas", "blas", "mat", "tex"):
            setattr(s, k, ds.t[k].data_ptr())
        s.bvh, s.tri, s.triEx = nodes.data_ptr(), tri.data_ptr(), ex.data_ptr()
        s.n_tlas_nodes, s.n_blas, s.n_bvh_nodes, s.n_tris = ds.c.n_tlas_nodes, ds.c.n_blas, info.n_nodes, n_tris
        s.n_mats, s.tex_bytes = ds.c.n_mats, ds.c.tex_bytes
        rt.accel_destroy(rt.accel_build(s, stream()))
    return run


def frame_rate(ds, reps):
    w, h = 1920, 1080
    dst = torch.zeros(w * h, dtype=torch.int32, device="cuda:0")
    p = rt.default_shade_params()
    t = timed(lambda: rt.render(ds.accel, w, h, 0, h, p, dst.data_ptr(), 1, None, None, None, stream()), reps, 3)
    t["frames_per_s"] = 1000.0 / t["median_ms"]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-hairball", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    torch.cuda.init()

    # (a) atrium, CPU-built tree
    t0 = time.time()
    sc = vrt.scene.procedural("atrium", 8)
    ds = vrt.tracer.DeviceScene(sc, "cuda:0")
    res["atrium_scene_load_s"] = time.time() - t0
    res["atrium_frame_before_refit"] = frame_rate(ds, a.reps)
    res["atrium_first_refit_geometry_incl_plan"] = timed(lambda: ds.refit(True), 1, 0)
    res["atrium_refit_geometry"] = timed(lambda: ds.refit(True), a.reps, a.warmup)
    res["atrium_refit_instances"] = timed(lambda: ds.refit(False), a.reps, a.warmup)
    res["atrium_frame_after_refit"] = frame_rate(ds, a.reps)
    res["atrium_rebuild_bvh_build_plus_accel_build"] = timed(rebuild_blas(ds, ds.c.n_tris), a.reps, a.warmup)
    ds.close()
    del ds, sc
    print(json.dumps(res), flush=True)

    # (b) 1,000 instances
    base = np.frombuffer(bytes(vrt.scene.procedural("blob", 2).buffers["tri"]), np.float32).reshape(-1, 9)
    n = 1000
    rng = np.random.default_rng(1)
    xf = []
    for i in range(n):
        m = np.eye(4, dtype=np.float32)
        m[:3, 3] = rng.uniform(-300, 300, 3)
        xf.append(m)
    ds = vrt.tracer.DeviceScene.build_on_gpu([base] * n, device="cuda:0", transforms=xf)
    moved = [m.copy() for m in xf]
    for m in moved:
        m[:3, 3] += np.float32(1.0)
    d_m = torch.from_numpy(np.ascontiguousarray(np.stack(moved).reshape(-1))).to("cuda:0")
    res["inst1000_first_set_transforms_incl_plan"] = timed(lambda: rt.accel_set_transforms(ds.accel, 0, n, d_m.data_ptr(), stream()), 1, 0)
    res["inst1000_set_transforms_plus_refit"] = timed(lambda: rt.accel_set_transforms(ds.accel, 0, n, d_m.data_ptr(), stream()), a.reps, a.warmup)
    res["inst1000_refit_instances"] = timed(lambda: ds.refit(False), a.reps, a.warmup)
    # the rebuild: host boxes (the corner transform of tracer.build_on_gpu) + vxrt_tlas_build + vxrt_accel_build
    info = ds.bvh_info
    tl = torch.zeros(2 * n * 52, dtype=torch.uint8, device="cuda:0")

    def rebuild_tlas():
        b = np.array(list(info.bounds), np.float64)
        corners = np.array([[b[3 * ((c >> k) & 1) + k] for k in range(3)] + [1.0] for c in range(8)])
        boxes = np.zeros((n, 6), np.float32)
        for i, m in enumerate(moved):
            wc = (corners @ m.astype(np.float64).T)[:, :3].astype(np.float32)
            boxes[i, :3], boxes[i, 3:] = wc.min(0), wc.max(0)
        tb = torch.from_numpy(boxes).to("cuda:0")
        ti = rt.tlas_build(tb.data_ptr(), n, tl.data_ptr(), 2 * n, stream())
        s = rt.VxrtScene()
        for k in ("blas", "bvh", "tri", "triEx", "mat", "tex"):
            setattr(s, k, ds.t[k].data_ptr())
        s.tlas = tl.data_ptr()
        s.n_tlas_nodes, s.n_blas, s.n_bvh_nodes, s.n_tris = ti.n_nodes, n, ds.c.n_bvh_nodes, ds.c.n_tris
        s.n_mats, s.tex_bytes = ds.c.n_mats, ds.c.tex_bytes
        rt.accel_destroy(rt.accel_build(s, stream()))
    res["inst1000_rebuild_host_boxes_tlas_build_accel_build"] = timed(rebuild_tlas, a.reps, a.warmup)
    ds.close()
    del ds
    print(json.dumps(res), flush=True)

    # (a) hairball, GPU-built tree
    if not a.no_hairball:
        t0 = time.time()
        tri = vrt.scene.procedural("hairball_fill", 20000, 250, 7)["tri"].view(np.float32).reshape(-1, 9)
        ds = vrt.tracer.DeviceScene.build_on_gpu(tri, device="cuda:0")
        res["hairball_tris"] = int(ds.c.n_tris)
        res["hairball_load_s"] = time.time() - t0
        res["hairball_first_refit_geometry_incl_plan"] = timed(lambda: ds.refit(True), 1, 0)
        res["hairball_refit_geometry"] = timed(lambda: ds.refit(True), a.reps, a.warmup)
        res["hairball_rebuild_bvh_build_plus_accel_build"] = timed(rebuild_blas(ds, ds.c.n_tris), max(3, a.reps // 2), 1)
        ds.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
