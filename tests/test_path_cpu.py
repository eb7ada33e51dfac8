"""CPU: tests/path_ref.py (the restatement the path-frame GPU tests compare against) is held to the two identities of the definition --
bounces = 1, spp = 1, shadow = 0 is the diffuse-bounce frame, bounces = 0 is the direct frame -- and the cases of
tests/test_gpu_path.py are shown to exercise what they are meant to: at every depth paths that end by a miss, paths that go on and
occlusion rays that are blocked.

The direct-frame identity is asserted for spp = 1, 2 and 4: acc / spp returns Lit exactly when the sum of spp equal terms and the
division are exact, which holds for the powers of two (x + x + x divided by 3 is not always x in fp32)."""
import numpy as np
import pytest

import camera_ref as cr
import camera_secondary_ref as csr
import path_ref as pr
import scenes

KEYS = csr.KEYS
W, H = pr.W, pr.H


@pytest.fixture(scope="module")
def scene_of(vrt, golden):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "mirror_hall":
                cache[name] = scenes.mirror_hall(vrt)
            else:
                g = golden(name)
                cache[name] = {k: g[k] for k in KEYS}
        return cache[name]
    return get


@pytest.fixture(scope="module")
def hall_runs(po, vrt, scene_of):
    """the restatement of the (2, 3, 1) seed 3 case per hall camera, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = pr.frame(scene_of("mirror_hall"), csr.hall_cameras(vrt)[name], W, H, po.shade_params(), 2, 3, 3, 1)
        return cache[name]
    return get


def _same(got, want, what):
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what + ": colours")
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": pixels")
    assert got[2] == want[2], "%s: rays traced %d, %d" % (what, got[2], want[2])


@pytest.mark.parametrize("name", ["framing", "orbit_1", "inside_blob"])
def test_one_bounce_is_the_diffuse_bounce_frame(po, vrt, scene_of, name):
    b, cam, pp = scene_of("mirror_hall"), csr.hall_cameras(vrt)[name], po.shade_params()
    for seed in (0, 7):
        got = pr.frame(b, cam, W, H, pp, 1, 1, seed, 0)
        _same(got, csr.gi_frame(b, cam, W, H, pp, seed), "%s seed %d" % (name, seed))
        assert got[3][0][1] > 0


@pytest.mark.parametrize("w,h,y0,y1,seed", [(13, 7, 0, 7, 0), (96, 64, 11, 37, 0x9E3779B9)])
def test_one_bounce_on_the_fixed_camera_is_the_oracle(po, scene_of, w, h, y0, y1, seed):
    b, pp = scene_of("mirror_hall"), po.shade_params()
    px, col, n, _ = pr.frame(b, None, w, h, pp, 1, 1, seed, 0, y0, y1)
    opx, ocol, on = po.render_gi(b, w, h, pp, seed, y0, y1)
    _same((px, col, n), (opx[y0:y1], ocol[y0:y1], on), "fixed camera")


@pytest.mark.parametrize("name", ["framing", "orbit_1", "inside_blob"])
@pytest.mark.parametrize("shadow", [0, 1])
def test_no_bounce_is_the_direct_frame(po, vrt, scene_of, name, shadow):
    b, cam, pp = scene_of("mirror_hall"), csr.hall_cameras(vrt)[name], po.shade_params()
    want = cr.frame(b, cam, W, H, pp, shadow)
    prim = pr.primary(b, cr.rays(cam, W, H))
    for spp in (1, 2, 4):
        got = pr.frame(b, cam, W, H, pp, spp, 0, 5, shadow, prim=prim)
        _same(got, (want[0], want[2], want[3]), "%s shadow %d spp %d" % (name, shadow, spp))
    if shadow:
        assert (want[1]["blasIdx"] >> 31).any()   # (blocked occlusion rays: the occluded form of Lit is exercised)


@pytest.mark.parametrize("name,want", [("framing", [(7196, 3158, 214), (3158, 1656, 68), (1656, 809, 48)]),
                                       ("orbit_1", [(8140, 3729, 267), (3729, 1930, 99), (1930, 1003, 55)])])
def test_depth_counts_of_the_light_sampled_case(hall_runs, name, want):
    """(live paths, bounce rays that hit, blocked occlusion rays) per depth: some paths end by a miss, some go on, some occlusion rays
    are blocked, at every depth"""
    depths = hall_runs(name)[3]
    assert depths == want
    for live, hit, blocked in depths:
        assert 0 < hit < live and blocked > 0


def test_inside_blob_never_misses_and_is_mostly_in_shadow(hall_runs):
    for live, hit, blocked in hall_runs("inside_blob")[3]:
        assert live > 0 and hit == live and 2 * blocked > hit


def test_beyond_2_60_is_outside_the_fast_domain(vrt):
    assert not csr.in_fast_domain(cr.rays(csr.hall_cameras(vrt)["beyond_2_60"], W, H)).any()


@pytest.mark.parametrize("name", csr.HALL_CAMERA_NAMES)
def test_hall_colours_are_finite(hall_runs, name):
    assert np.isfinite(hall_runs(name)[1]).all()


@pytest.mark.parametrize("name", ["tex_mix", "teapot_x3"])
def test_golden_scenes_keep_paths_alive(po, vrt, scene_of, name):
    for cname, cam in csr.golden_cameras(vrt).items():
        depths = pr.frame(scene_of(name), cam, W, H, po.shade_params(), 2, 3, 3, 1)[3]
        assert depths[2][0] >= 10, "%s %s: %r" % (name, cname, depths)


def test_small_shapes_are_not_vacuous(po, vrt, scene_of):
    """the 13 x 7 frame, the row window and the 16-bounce case of the GPU test"""
    b, pp = scene_of("mirror_hall"), po.shade_params()
    cam = csr.hall_cameras(vrt, 13, 7)["axis_aligned"]
    prim = pr.primary(b, cr.rays(cam, 13, 7))
    outside = ~csr.in_fast_domain(prim["rays"])
    assert outside.sum() == 13 + 7 - 1 and (outside & (prim["hits"]["dist"] != cr.LARGE)).any()
    assert pr.frame(b, cam, 13, 7, pp, 2, 3, 3, 1, prim=prim)[3][0][1] > 0
    assert pr.frame(b, csr.orbit(vrt, 2), W, H, pp, 2, 3, 3, 1, 13, 43)[3][2][1] > 0
    deep = pr.frame(b, csr.hall_cameras(vrt)["inside_blob"], W, H, pp, 1, 16, 0, 1)[3]
    assert deep[15][0] > 0   # (paths alive at the last of 16 depths)
