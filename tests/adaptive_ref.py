"""numpy restatement of adaptive sampling: the path frame with a sample count per pixel (vxrt_render_path_adaptive), the variance frame
on top of it (vxrt_render_path_variance_adaptive) and the counts from a variance (vxrt_sample_counts).  TEST INFRASTRUCTURE ONLY.

A thin layer over the unchanged path_ref / variance_ref.  The header's "Adaptive sampling" defines a pixel of the frame with counts as
the vxrt_render_path pixel with spp := n_p, so:
  frame        for every distinct clamped count v, path_ref.frame_from_rays over the rays whose pixel has n_p = v, with spp = v; the
               traced rays of the subsets are summed (every primary ray is in exactly one subset; a miss is the background whatever v)
  variance     variance_ref.path_frame(pre=...) fed that colour: nothing else of vxrt_render_path_variance changes
  counts       sample_counts(): one numpy float32 operation per symbol of the definition
offsets() / straddlers() restate the packing (pixels in window order, a batch = `cap` consecutive paths) for tests/test_adaptive_cpu.py."""
import numpy as np

import camera_ref as cr
import camera_secondary_ref as csr
import denoise_ref as dr
import path_ref as pr
import variance_ref as vr
from camera_ref import po

f32 = np.float32
COUNT_MAX = 4096


def clamp(counts, cap):
    """n_p = min(max(counts, 1), cap) of raw uint32 counts"""
    c = np.asarray(counts).astype(np.uint32)
    return np.minimum(np.maximum(c, np.uint32(1)), np.uint32(cap)).astype(np.uint32)


def frame_from_rays(scene, rays, xs, ys, w, params, counts, cap, bounces, seed=0, shadow=0, prim=None):
    """the frame with counts over `rays` (ray i belongs to pixel (xs[i], ys[i]) and has the raw count counts[i]): pixels (n,) u32,
    colours (n, 3), rays traced"""
    prim = prim or pr.primary(scene, rays)
    xs, ys = np.asarray(xs), np.asarray(ys)
    n_p = clamp(counts, cap)
    n = len(prim["rays"])
    px, col, traced = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), 0
    for v in np.unique(n_p):
        sel = np.nonzero(n_p == v)[0]
        sub = {"rays": prim["rays"][sel], "hits": prim["hits"][sel]}
        p, c, t, _ = pr.frame_from_rays(scene, sub["rays"], xs[sel], ys[sel], w, params, int(v), bounces, seed, shadow, sub)
        px[sel], col[sel] = p, c
        traced += t
    return px, col, traced


def frame(scene, cam14, w, h, params, counts, cap, bounces, seed=0, shadow=0, y0=0, y1=None, prim=None):
    """the frame with counts of rows [y0, y1) seen from cam14 (None: the fixed camera); counts: (h, w) raw, the full frame's.
    pixels (rows, w), colours (rows, w, 3), rays traced"""
    y1 = h if y1 is None else y1
    xs, ys = csr.pixel_grid(w, y0, y1)
    if prim is None:
        prim = pr.primary(scene, po.camera_rays(w, h, y0, y1) if cam14 is None else cr.rays(cam14, w, h, y0, y1))
    c = np.asarray(counts).reshape(h, w)[y0:y1].reshape(-1)
    px, col, n = frame_from_rays(scene, prim["rays"], xs, ys, w, params, c, cap, bounces, seed, shadow, prim)
    return px.reshape(y1 - y0, w), col.reshape(y1 - y0, w, 3), n


def path_inputs(scene, cam14, w, h, params, counts, cap, bounces, seed, shadow, y0=0, y1=None):
    """variance_ref.path_inputs with the frame with counts for the path frame: what variance_ref.path_frame takes as `pre`"""
    y1 = h if y1 is None else y1
    D, A, P, N, prim = dr.path_guides(scene, cam14, w, h, params, shadow, y0, y1)
    _, c, traced = frame(scene, cam14, w, h, params, counts, cap, bounces, seed, shadow, y0, y1, prim)
    return D, A, P, N, prim, c, traced


def variance_frame(scene, snap, cam14, w, h, params, counts, cap, bounces, seed, shadow, dn, tp, vp, hist, motion=0, y0=0, y1=None, pre=None):
    """vxrt_render_path_variance_adaptive: variance_ref.path_frame on the colour of the frame with counts"""
    pre = pre or path_inputs(scene, cam14, w, h, params, counts, cap, bounces, seed, shadow, y0, y1)
    return vr.path_frame(scene, snap, cam14, w, h, params, cap, bounces, seed, shadow, dn, tp, vp, hist, motion, y0, y1, pre)


def sample_counts(variance, prm, prev_counts=None):
    """vxrt_sample_counts: prm = (gain, min_spp, max_spp).  (counts u32, their sum)"""
    gain, lo, hi = f32(prm[0]), int(prm[1]), int(prm[2])
    v = np.ascontiguousarray(variance, np.float32).reshape(-1)
    if prev_counts is None:
        m = np.ones(len(v), np.float32)
    else:
        m = clamp(np.asarray(prev_counts).reshape(-1), COUNT_MAX).astype(np.float32)
    with np.errstate(all="ignore"):
        x = ((v * m).astype(np.float32) * gain).astype(np.float32)
        c = np.ceil(x).astype(np.float32)
        above, below = c > f32(lo), c < f32(hi)       # (both false for a NaN)
    out = np.full(len(v), lo, np.uint32)
    out[above & ~below] = hi
    mid = above & below
    out[mid] = c[mid].astype(np.uint32)
    return out, int(out.astype(np.uint64).sum())


def offsets(n_p, hit):
    """(cnt, off, total) of a window: cnt = n_p where the pixel has a primary hit, else 0; off = its exclusive sum in window order"""
    cnt = np.where(np.asarray(hit).reshape(-1), np.asarray(n_p).reshape(-1), 0).astype(np.uint64)
    inc = np.cumsum(cnt, dtype=np.uint64)
    return cnt, inc - cnt, int(inc[-1]) if len(inc) else 0


def straddlers(cnt, off, cap):
    """the pixels whose samples are in more than one batch of `cap` consecutive paths"""
    cap = np.uint64(cap)
    has = cnt > 0
    first, last = off // cap, (off + cnt - np.uint64(1)) // cap
    return np.nonzero(has & (first != np.where(has, last, first)))[0]
