"""Russian roulette in path frames timed and measured: the 1,048,576-triangle atrium of tools/emissive_time.py (its 64 small lights in
the scene throughout) at 1920x1080, 4 spp, shadow = 1, a static camera, everything in one process, the forms alternated.

Per row -- `bounces` 3, 8 and 16 of the plain frame, and `bounces` 8 with emissive_mis and the lights -- each without roulette
(vxrt_render_path_frame) and with `--first 2 --q-min 0.05` (vxrt_render_path_frame_ex):
  ms per frame      alternating rounds of `--frames` frames per form, events on the stream, median and spread ((max - min) / median)
  rays_traced       of one frame
  RMSE              of the colours (all pixels, 3 channels) at 4 spp against a `--reference-spp` frame WITHOUT roulette of the same bounces
One JSON line.

`--existing` times the two entry points that existed before, vxrt_render_path and vxrt_render_path_emissive_mis, and nothing else; with
`--root DIR` the package and its library are those of another checkout of the repository, so that two commits can be compared by
alternating processes in one session.

    python tools/roulette_time.py [--rounds 10] [--warmup 2] [--frames 3]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tlas", "blas", "bvh", "tri", "triEx", "mat", "tex")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--lights", type=int, default=64)
    ap.add_argument("--first", type=int, default=2)
    ap.add_argument("--q-min", type=float, default=0.05)
    ap.add_argument("--bounces", type=int, nargs="+", default=[3, 8, 16])
    ap.add_argument("--mis-bounces", type=int, default=8)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--existing", action="store_true")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("at least 10 alternating rounds")
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
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
    spp, shadow, seed = 4, 1, 3
    px = torch.zeros((h, w), dtype=torch.int32, device=dev)
    col = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    ref = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    mis = rtapi.EmissiveMisParams(1.0, (rtapi.C.c_uint32 * 3)(0, 0, 0))
    _, b, pairs = lit_atrium(vrt, np, a.lights)
    ds = vrt.tracer.DeviceScene({k: b[k] for k in KEYS}, dev)
    ds.set_emitters(pairs)

    def summary(v):
        return {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v)),
                "spread": float((np.max(v) - np.min(v)) / abs(np.median(v)))}

    def alternate(forms):
        """forms: name -> a call that renders one frame; the per-form summaries of a.rounds alternating rounds"""
        def run(call):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.frames):
                call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.frames
        for _ in range(a.warmup):
            for call in forms.values():
                run(call)
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, call in forms.items():
                ms[k].append(run(call))
        assert rtapi.status(s) == 0
        return {k: summary(v) for k, v in ms.items()}

    head = {"tool": "roulette_time", "root": os.path.relpath(root, ROOT), "width": w, "height": h, "spp": spp, "shadow": shadow, "lights": a.lights,
            "frames_per_round": a.frames, "rounds": a.rounds, "warmup": a.warmup}
    if a.existing:
        bounces = 3
        out = alternate({"path": lambda: rtapi.render_path(ds.accel, cam, w, h, 0, h, p, spp, bounces, px.data_ptr(), seed, shadow, None, None, s),
                         "emissive_mis": lambda: rtapi.render_path_emissive_mis(ds.accel, cam, w, h, 0, h, p, spp, bounces, mis, px.data_ptr(), seed, shadow, None, None, s)})
        ds.close()
        print(json.dumps(dict(head, bounces=bounces, existing=out)))
        return

    on = rtapi.RouletteParams(1, a.first, a.q_min)

    def frame(bounces, roulette, em=None, n_spp=spp, sd=seed, colors=None, rays=None):
        d = rtapi.PathFrame(w, h, 0, h, p, rtapi.PathParams(n_spp, bounces, sd, shadow), px.data_ptr(), cam=cam, emissive_mis=em, colors=colors, rays_traced=rays)
        rtapi.render_path_frame(ds.accel, d, s, roulette=roulette)

    rows = [("plain_%d" % k, k, None) for k in a.bounces] + [("mis_%d" % a.mis_bounces, a.mis_bounces, mis)]
    forms = {}
    for name, k, em in rows:
        forms[name + "_off"] = lambda k=k, em=em: frame(k, None, em)
        forms[name + "_on"] = lambda k=k, em=em: frame(k, on, em)
    out = alternate(forms)
    for name, k, em in rows:
        frame(k, None, em, a.reference_spp, 1000003, ref.data_ptr())
        for tag, rp in (("_off", None), ("_on", on)):
            cnt.zero_()
            frame(k, rp, em, spp, seed, col.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize()
            out[name + tag]["rays_traced"] = int(cnt.item())
            out[name + tag]["rmse"] = float(torch.sqrt(torch.mean((col - ref) ** 2)).item())
        out[name + "_on"]["ratio_to_off"] = out[name + "_on"]["ms_median"] / out[name + "_off"]["ms_median"]
    assert rtapi.status(s) == 0
    ds.close()
    print(json.dumps(dict(head, first=a.first, q_min=a.q_min, reference_spp=a.reference_spp, **out)))


if __name__ == "__main__":
    main()
