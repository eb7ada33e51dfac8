"""CPU: the restatement of motion-aware temporal accumulation (tests/motion_ref.py) is held to the identities of the definition, and the
property the feature exists for is measured on it: a moving instance keeps its accumulated history."""
import numpy as np
import pytest

import camera_ref as cr
import motion_cases as mc
import motion_ref as mr
import path_ref as pr
import temporal_cases as tc
import temporal_ref as tr


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h,name", tc.all_sequences())
def test_with_the_frames_own_guides_the_step_is_the_camera_step(w, h, name):
    """T_m with Q = P and N' = N is T, bit for bit (NaN payloads included: the same numpy operations on the same inputs)"""
    fr, win, prm = tc.frames(w, h, name)
    ha, hb = tr.History(), tr.History()
    for k, (cam, E, P, N, _, _) in enumerate(fr):
        want = tr.step(E, P, N, ha, cam, w, h, win[0], win[1], prm)
        got = mr.step(E, P, N, P, N, hb, cam, w, h, win[0], win[1], prm)
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg="%dx%d %s frame %d" % (w, h, name, k))
        for a, b in ((ha.HE, hb.HE), (ha.HP, hb.HP), (ha.HN, hb.HN)):
            np.testing.assert_array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def moving(vrt, po):
    """the six frames of motion_cases with a FIXED camera: per frame the scene, its snapshot, the primary pass and the guides"""
    b = mc.hall(vrt)
    cam = mc.cameras(yaw=False)[0]
    rays = cr.rays(cam, mc.W, mc.H)
    frames = []
    for scene, snap in mc.sequence(b):
        prim = pr.primary(scene, rays)
        hits = prim["hits"]
        hit = hits["dist"] != cr.LARGE
        P = np.zeros((len(rays), 4), np.float32)
        N = np.zeros((len(rays), 4), np.float32)
        I, Nn, _ = cr._normal_and_point(scene, rays[hit], hits[hit])
        P[hit, 0:3], P[hit, 3], N[hit, 0:3] = np.stack(I, 1), 1.0, np.stack(Nn, 1)
        Q, Nq = mr.previous_positions(scene, snap, hits)
        on = (hit & ((hits["blasIdx"] & 0x7fffffff) == mc.BLOB)).reshape(mc.H, mc.W)
        frames.append({"hits": hits, "P": P.reshape(mc.H, mc.W, 4), "N": N.reshape(mc.H, mc.W, 4), "Q": Q.reshape(mc.H, mc.W, 4),
                       "Nq": Nq.reshape(mc.H, mc.W, 4), "on": on})
    return cam, rays, frames


def _project(cam14, X):
    """float64 pinhole projection of world points X (n, 3) to continuous pixel coordinates (pixel centres at integers)"""
    c = np.asarray(cam14, np.float64)
    B = np.stack([c[6:9], c[9:12], c[3:6]], 1)             # columns right, up, forward
    abc = np.linalg.solve(B, (X - c[0:3]).T).T
    return ((abc[:, 0] / abc[:, 2]) / c[12] + 0.5) * mc.W - 0.5, ((abc[:, 1] / abc[:, 2]) / c[13] + 0.5) * mc.H - 0.5


def test_a_translated_instance_is_found_where_it_was(moving):
    """Q of a pixel on the translated blob projects where an independent float64 computation puts the surface point one frame earlier:
    the float64 hit point o + d * dist minus the frame's translation step.  Tolerance: Q and the hit point are each a handful of fp32
    operations on coordinates below 512 (half an ulp, 2^-15 units, each; 64 of them is generous), plus the traversal's dist, whose error
    along the ray barely moves the projection -- 64 * 2^-15 units is 6.3e-4 of a pixel of 3.08 units, against the 1.5 pixels of the motion."""
    cam, rays, frames = moving
    tol = 64 * 2.0 ** -15 / 3.08
    step = np.asarray(mc.STEP, np.float64)
    for k in range(1, mc.N_FRAMES):
        f, g = frames[k], frames[k - 1]
        on = f["on"].reshape(-1)
        assert on.sum() >= 100
        r, d = rays[on].astype(np.float64), f["hits"]["dist"][on].astype(np.float64)
        X = r[:, 0:3] + r[:, 3:6] * d[:, None]
        fx, fy = _project(cam, X - step)
        qx, qy = _project(cam, f["Q"].reshape(-1, 4)[on, 0:3].astype(np.float64))
        assert np.abs(qx - fx).max() < tol and np.abs(qy - fy).max() < tol, (k, np.abs(qx - fx).max(), np.abs(qy - fy).max())
        cx, cy = _project(cam, X)
        assert 1.3 < np.median(np.abs(cx - fx)) < 1.7 and np.abs(cy - fy).max() < 0.2   # (it did move, by about 1.5 pixels along the rows)
        # and that place was on the blob in the previous frame, for every pixel whose four neighbours there are inside the frame
        x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
        inside = (x0 >= 0) & (x0 + 1 < mc.W) & (y0 >= 0) & (y0 + 1 < mc.H)
        near = np.zeros(len(x0), bool)
        for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
            near[inside] |= g["on"][y0[inside] + j, x0[inside] + i]
        assert near[inside].mean() > 0.99


def _eroded(m, r=2):
    out = m.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            s = np.zeros_like(m)
            ys, yd = slice(max(0, dy), m.shape[0] + min(0, dy)), slice(max(0, -dy), m.shape[0] + min(0, -dy))
            xs, xd = slice(max(0, dx), m.shape[1] + min(0, dx)), slice(max(0, -dx), m.shape[1] + min(0, -dx))
            s[yd, xd] = m[ys, xs]
            out &= s
    return out


def test_a_moving_instance_keeps_its_history(moving):
    """Six frames, the blob moving 1.5 pixels per frame under a fixed camera: mean accumulated length of the last frame over the pixels that
    are on the blob in the last two frames and at least 2 pixels inside its silhouette.
    Measured on this restatement: camera-only step 2.628, step with motion 5.838 (of at most 6), over 228 pixels; the threshold is their
    midpoint, 4.233.  Without the feature there is no step with motion to measure."""
    cam, rays, frames = moving
    E = np.zeros((mc.H, mc.W, 3), np.float32)      # (the length does not depend on the signal)
    hc, hm = tr.History(), tr.History()
    for f in frames:
        cam_only = tr.step(E, f["P"], f["N"], hc, cam, mc.W, mc.H, 0, mc.H, mc.TP)
        motion = mr.step(E, f["P"], f["N"], f["Q"], f["Nq"], hm, cam, mc.W, mc.H, 0, mc.H, mc.TP)
    inner = _eroded(frames[-1]["on"]) & _eroded(frames[-2]["on"])
    assert inner.sum() >= 100, inner.sum()
    lc, lm = float(cam_only[..., 3][inner].mean()), float(motion[..., 3][inner].mean())
    print("accumulated length over %d pixels: camera-only %.3f, motion %.3f" % (inner.sum(), lc, lm))
    assert lm > 0.5 * (lc + lm)
