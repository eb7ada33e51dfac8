"""CPU: tests/adaptive_ref.py (the restatement the adaptive GPU tests compare against) is held to the uniform identity of the definition
-- counts equal to the cap everywhere is path_ref.frame bit for bit -- and the cases of tests/test_gpu_adaptive.py
(tests/adaptive_cases.py) are shown to exercise what they are meant to: several distinct clamped counts with the hostile raw values among
them, a mosaic that is no uniform frame, pixels whose samples straddle a batch boundary under the child process's batch size, and a
table for vxrt_sample_counts that reaches every arm of its definition."""
import os
import re

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_ref as ar
import camera_ref as cr
import camera_secondary_ref as csr
import path_ref as pr
import scenes

W, H = ac.W, ac.H
f32 = np.float32


@pytest.fixture(scope="module")
def hall(vrt):
    return scenes.mirror_hall(vrt)


def _same(got, want, what):
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": pixels")
    assert got[2] == want[2], "%s: rays traced %d, %d" % (what, got[2], want[2])


@pytest.mark.parametrize("name", ["orbit_1", None])
def test_uniform_counts_are_the_path_frame(po, vrt, hall, name):
    cam = None if name is None else csr.hall_cameras(vrt)[name]
    prim = pr.primary(hall, po.camera_rays(W, H, 0, H) if cam is None else cr.rays(cam, W, H))
    for spp, bounces, shadow, seed in ((3, 2, 1, 3), (1, 0, 0, 0), (4, 0, 1, 0)):
        want = pr.frame(hall, cam, W, H, po.shade_params(), spp, bounces, seed, shadow, prim=prim)
        for raw in (spp, spp + 1, ac.U32_MAX):
            got = ar.frame(hall, cam, W, H, po.shade_params(), np.full((H, W), raw, np.uint32), spp, bounces, seed, shadow, prim=prim)
            _same(got, want, "%s spp %d bounces %d raw %d" % (name, spp, bounces, raw))


@pytest.mark.parametrize("case", [ac.MOSAIC, ac.RESTATED, ac.VARIANCE] + list(ac.IN_FLIGHT), ids=["mosaic", "restated", "variance", "flight0", "flight1"])
def test_count_maps_are_not_vacuous(case):
    raw = ac.counts_of(case)
    n_p = ar.clamp(raw, case["cap"])
    distinct = np.unique(n_p)
    assert 3 <= len(distinct) <= 4
    assert all((n_p == v).sum() > W * H // 10 for v in distinct)      # every value on a good part of the frame
    if case is ac.RESTATED:
        assert (raw == 0).any() and (raw == ac.U32_MAX).any() and ((raw > case["cap"]) & (raw < 100)).any()
        assert (n_p[raw == 0] == 1).all() and (n_p[raw > case["cap"]] == case["cap"]).all()


def test_the_mosaic_is_no_uniform_frame_and_is_made_of_them(po, vrt, hall):
    case = ac.MOSAIC
    cam = csr.hall_cameras(vrt)["orbit_1"]
    prim = pr.primary(hall, cr.rays(cam, W, H))
    raw = ac.counts_of(case)
    px, col, traced = ar.frame(hall, cam, W, H, po.shade_params(), raw, case["cap"], case["bounces"], case["seed"], case["shadow"], prim=prim)
    made = np.zeros_like(col)
    for v in case["values"]:
        upx, ucol, utraced, _ = pr.frame(hall, cam, W, H, po.shade_params(), v, case["bounces"], case["seed"], case["shadow"], prim=prim)
        assert (ucol.view(np.uint32) != col.view(np.uint32)).any() and utraced != traced, "the mosaic is the uniform frame of %d" % v
        made[raw == v] = ucol[raw == v]
    np.testing.assert_array_equal(made.view(np.uint32), col.view(np.uint32))


@pytest.mark.parametrize("case", [ac.MOSAIC, ac.RESTATED], ids=["mosaic", "restated"])
def test_samples_straddle_the_child_batches(vrt, hall, case):
    """under VXRT_PATH_BATCH = CHILD_BATCH: many batches, pixels whose samples are in two of them, a short last batch and batches past
    the end (the host issues them for cap * pixels paths)"""
    hit = pr.primary(hall, cr.rays(csr.hall_cameras(vrt)["orbit_1"], W, H))["hits"]["dist"] != cr.LARGE
    cnt, off, total = ar.offsets(ar.clamp(ac.counts_of(case), case["cap"]), hit)
    assert 0 < hit.sum() < W * H
    issued = -(-(W * H * case["cap"]) // ac.CHILD_BATCH)
    used = -(-total // ac.CHILD_BATCH)
    assert 2 * len(ar.straddlers(cnt, off, ac.CHILD_BATCH)) >= used - 1 > 0      # (a pixel straddles at least half of the boundaries between batches)
    assert used > 5 and total % ac.CHILD_BATCH != 0 and issued > used


def test_scan_constants_are_the_kernels(vrt):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vortex-raytracing_amd", "csrc", "rt_path.hip")).read()
    block = int(re.search(r"#define PT_SCAN_BLOCK (\d+)u", src).group(1))
    per_pass = int(re.search(r"#define PT_SCAN_PASS (\d+)u", src).group(1))
    assert vrt.rtapi.ADAPTIVE_SCAN_BLOCK == block and vrt.rtapi.ADAPTIVE_SCAN_PASS == block * per_pass


@pytest.mark.parametrize("prm", ac.SAMPLE_PRMS)
def test_sample_counts_on_the_hostile_table(prm):
    gain, lo, hi = prm
    v = ac.hostile_variances(prm)
    got, total = ar.sample_counts(v, prm)
    assert total == int(got.sum()) and got.min() >= lo and got.max() <= hi
    assert (got[np.isnan(v)] == lo).all() and (got[v == np.inf] == hi).all() and (got[v <= 0] == lo).all()      # (v <= 0: negatives, -inf, +-0)
    # a power-of-two gain: the product is exact (or overflows / underflows to what clamps the same), so doubles give the same counts
    fin = np.isfinite(v)
    want = np.clip(np.ceil(v[fin].astype(np.float64) * float(gain)), lo, hi).astype(np.uint32)
    np.testing.assert_array_equal(got[fin], want)
    # exactly on an integer k stays k, one ulp above goes to k + 1
    for k in range(max(lo, 1), min(hi, 5)):
        e = f32(k) / f32(gain)
        on, up = ar.sample_counts(np.array([e, ac._ulp(e, 1)], np.float32), prm)[0]
        assert on == max(k, lo) and up == min(max(k + 1, lo), hi)


def test_sample_counts_previous_counts():
    prm = (0.5, 1, 4096)
    v = np.full(6, 2.0, np.float32)
    prev = np.array([0, 1, 3, 4096, 4097, ac.U32_MAX], np.uint32)
    got, total = ar.sample_counts(v, prm, prev)
    assert list(got) == [1, 1, 3, 4096, 4096, 4096] and total == sum([1, 1, 3, 4096, 4096, 4096])
    assert list(ar.sample_counts(v, prm)[0]) == [1] * 6
    for n in ac.SAMPLE_SIZES:
        vv, pp = ac.sample_inputs(n, prm, n)
        assert len(vv) == n and len(pp) == n
        if n >= 255:
            assert (pp == 0).any() and (pp > 4096).any() and np.isnan(vv).any()
            assert len(np.unique(ar.sample_counts(vv, prm, pp)[0])) > 8
