"""CPU: the restatement of the alpha-tested traversal (tests/alpha_ref.py) is pinned to the oracle, and the cases of
tests/alpha_cases.py are not vacuous.  No GPU.

1. With no table the restatement's loop is orc_trace_canonical: bit-equal hit records on every case, closest and any-hit, with and
   without tmax.
2. With the all-zero table its frames are pyoracle.render_ex's, bit for bit (fixed camera; shadow 0 and 1; the case's max_depth).
3. Non-vacuity, on the reference alone, per case over the rays of its cameras and its ray buffer.

What two of the conditions can mean per case: `tex_mix` (the committed fixture) and `chain20` (scenes.chain_bvh4) have single-triangle
leaves, and chain20 has one instance, so "rejected and accepted candidate in the same leaf" cannot occur in them and "in different
instances" cannot occur in chain20 whatever the alpha pattern or camera.  Those two conditions are asserted wherever the scene's
structure allows them (computed from the buffers, not assumed) -- mirror_hall has both."""
import numpy as np
import pytest

import alpha_cases as ac
import alpha_ref as ar
import camera_ref as cr
from camera_ref import po

LARGE = cr.LARGE


@pytest.mark.parametrize("name", ac.FRAME_CASES)
@pytest.mark.parametrize("any_hit", [False, True])
@pytest.mark.parametrize("with_tmax", [False, True])
def test_no_table_is_the_canonical_traversal(name, any_hit, with_tmax):
    rays, tmax = ac.ray_buffer(name)
    got, _ = ac.ref_trace(name, any_hit, with_tmax, alpha=False)
    want = po.trace_mt(po.trace_canonical, ac.case(name)["scene"], rays, tmax=tmax if with_tmax else None, any_hit=any_hit)
    assert got.tobytes() == want.tobytes()
    assert (want["dist"] != LARGE).sum() > 100


@pytest.mark.parametrize("seed,family", ac.HOSTILE)
def test_no_table_on_the_hostile_scenes(seed, family):
    c = ac.hostile(seed, family)
    for any_hit in (False, True):
        got = ar.trace(c["scene"], c["rays"], any_hit=any_hit)
        assert got.tobytes() == po.trace_mt(po.trace_canonical, c["scene"], c["rays"], any_hit=any_hit).tobytes()


@pytest.mark.parametrize("name", ac.FRAME_CASES)
@pytest.mark.parametrize("shadow", [0, 1])
def test_zero_table_frames_are_render_ex(name, shadow):
    c = ac.case(name)
    zero = ar.tracer(c["scene"], np.zeros(len(c["thresholds"]), np.uint8))
    px, hits, col, n = ar.frame_from_rays(c["scene"], zero, po.camera_rays(ac.W, ac.H), c["params"], shadow)
    rpx, rhits, rcol, rn = po.render_ex(c["scene"], ac.W, ac.H, c["params"], shadow)
    # (orc_render_ex reports the primary hit without the occlusion bit)
    plain = hits.copy()
    plain["blasIdx"] &= 0x7FFFFFFF
    assert plain.tobytes() == rhits.reshape(-1).tobytes()
    np.testing.assert_array_equal(col.view(np.uint32), rcol.reshape(-1, 3).view(np.uint32))
    np.testing.assert_array_equal(px, rpx.reshape(-1))
    assert n == rn


def _all_rays(name):
    """hit records with and without the table and what each ray met: the case's frames (closest hit) and its ray buffer"""
    c = ac.case(name)
    rays = np.concatenate([ac.cam_rays(cam) for cam in c["cams"].values()] + [ac.ray_buffer(name)[0]])
    info, info_any = np.zeros(len(rays), ar.INFO_DT), np.zeros(len(rays), ar.INFO_DT)
    tr = ac.tracer(name)
    return cr._trace(c["scene"], rays), tr(rays, None, False, info), info, tr(rays, None, True, info_any), info_any


@pytest.mark.parametrize("name", ac.FRAME_CASES)
def test_cases_are_not_vacuous(name):
    c = ac.case(name)
    opaque, alpha, info, alpha_any, info_any = _all_rays(name)
    hit_anything = (opaque["dist"] != LARGE) | (alpha["dist"] != LARGE)
    differ = alpha != opaque
    assert differ.sum() >= 0.05 * hit_anything.sum() and hit_anything.sum() > 500
    assert ((info["rejected_before_accept"] >= 2) & (info["accepted"] > 0)).any()            # two or more rejected, then an accept
    assert ((info["rejected"] > 0) & (info["accepted"] == 0) & (alpha["dist"] == LARGE)).any()   # everything rejected: a miss
    assert (info_any["first_rejected"] & (alpha_any["dist"] != LARGE)).any()                 # any-hit: first candidate rejected, a later one stops it
    if ac.has_multi_triangle_leaves(c["scene"]):
        assert info["same_leaf"].any()
    if c["scene"]["blas"].size // 160 > 1:
        assert info["other_instance"].any()
    # shadow frames: a pixel lit only because its occlusion ray passed a hole
    assert any(ac.ref_frame(name, cam, 1)[4].any() for cam in c["cams"])


def test_structural_conditions_occur_somewhere():
    """same leaf / different instances: see the module's docstring; at least one case shows each"""
    got = {k: False for k in ("same_leaf", "other_instance")}
    for name in ac.FRAME_CASES:
        info = _all_rays(name)[2]
        for k in got:
            got[k] = got[k] or bool(info[k].any())
    assert all(got.values()), got


@pytest.mark.parametrize("seed,family", ac.HOSTILE)
def test_hostile_sets_reject_and_accept(seed, family):
    c = ac.hostile(seed, family)
    info = np.zeros(len(c["rays"]), ar.INFO_DT)
    hits = ar.tracer(c["scene"], c["thresholds"])(c["rays"], None, False, info)
    assert (info["rejected"] > 0).any() and (info["accepted"] > 0).any()
    assert (hits != cr._trace(c["scene"], c["rays"])).any()


def test_hostile_sets_use_every_threshold():
    assert {int(t) for s, f in ac.HOSTILE for t in ac.hostile(s, f)["thresholds"]} == {0, 1, 128, 255}


def test_predicate_follows_the_rule():
    """threshold 0 never fetches; T compares with the top byte alone; the texel is shading's"""
    c = ac.case("chain20")
    b = c["scene"]
    n = b["tri"].size // 36
    m = len(c["thresholds"]) - 1
    for T, want in ((1, [t % 3 == 2 for t in range(n)]), (255, [t % 3 == 2 for t in range(n)])):
        thr = np.zeros(m + 1, np.uint8)
        thr[m] = T
        acc = ar.alpha_predicate(b, thr)
        assert [acc(t, 0.3, 0.3, 0.4) for t in range(n)] == want
    assert ar.alpha_predicate(b, np.zeros(m + 1, np.uint8)) is None and ar.alpha_predicate(b, None) is None
