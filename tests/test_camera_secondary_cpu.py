"""CPU: tests/camera_secondary_ref.py (the restatement the camera AO / diffuse-bounce GPU tests compare against) is pinned to the
oracle where the oracle has an answer -- the fixed camera's rays -- and the cases of tests/test_gpu_camera_secondary.py are shown to
exercise what they are meant to (partly occluded pixels, bounce rays that hit and that miss, primary rays outside the fast domain)."""
import numpy as np
import pytest

import camera_ref as cr
import camera_secondary_ref as csr
import scenes

KEYS = csr.KEYS


@pytest.fixture(scope="module")
def scene_of(vrt, golden):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "mirror_hall":
                cache[name] = scenes.mirror_hall(vrt)
            elif name == "chain20":
                sc = scenes.chain_bvh4(vrt, 20)
                cache[name] = {k: np.frombuffer(bytes(sc.buffers[k]), np.uint8).copy() for k in KEYS}
            else:
                g = golden(name)
                cache[name] = {k: g[k] for k in KEYS}
        return cache[name]
    return get


def _equal_to_oracle(po, b, w, h, y0, y1, spp, radius, seed):
    pp = po.shade_params()
    r = po.camera_rays(w, h, y0, y1)
    xs, ys = csr.pixel_grid(w, y0, y1)
    prim = csr.primary(b, r, pp)
    px, col, opn, n = csr.ao_frame_from_rays(b, r, xs, ys, w, pp, spp, radius, seed, prim)
    opx, ocol, ocnt, on = po.render_ao(b, w, h, pp, spp, radius, seed, y0, y1)
    np.testing.assert_array_equal(px.reshape(y1 - y0, w), opx[y0:y1])
    np.testing.assert_array_equal(col.reshape(y1 - y0, w, 3).view(np.uint32), ocol[y0:y1].view(np.uint32))
    np.testing.assert_array_equal(opn.reshape(y1 - y0, w), ocnt[y0:y1])
    assert n == on
    px, col, n = csr.gi_frame_from_rays(b, r, xs, ys, w, pp, seed, prim)
    opx, ocol, on = po.render_gi(b, w, h, pp, seed, y0, y1)
    np.testing.assert_array_equal(px.reshape(y1 - y0, w), opx[y0:y1])
    np.testing.assert_array_equal(col.reshape(y1 - y0, w, 3).view(np.uint32), ocol[y0:y1].view(np.uint32))
    assert n == on
    return len(prim["fi"])


@pytest.mark.parametrize("name,radius", [("mirror_hall", csr.RADIUS["mirror_hall"]), ("teapot_x3", 0.5), ("tex_mix", 0.5)])
@pytest.mark.parametrize("w,h,y0,y1,spp,seed", [(13, 7, 0, 7, 1, 0), (13, 7, 0, 7, 16, 3), (96, 64, 0, 64, 5, 0), (96, 64, 11, 37, 16, 0x9E3779B9)])
def test_restatement_equals_the_oracle_on_the_fixed_camera(po, scene_of, name, radius, w, h, y0, y1, spp, seed):
    hit = _equal_to_oracle(po, scene_of(name), w, h, y0, y1, spp, radius, seed)
    if name == "mirror_hall":
        assert hit > 0   # (the fixed camera looks into the hall: the secondary rays are exercised)


def test_albedo_restatement_on_textured_hits(po, scene_of, vrt):
    """The fixed camera does not frame the golden scenes, so the texColor restatement is held to the oracle where rays do hit them: the
    orbit cameras of the GPU test.  orc_shade with ambient = 1, no light and no background is texColor * (1 - reflectivity), and the golden instances
    have reflectivity 0."""
    for name in ("tex_mix", "teapot_x3"):
        b = scene_of(name)
        cams = csr.golden_cameras(vrt)
        r = np.concatenate([cr.rays(c, 48, 32) for c in cams.values()])
        hits = cr._trace(b, r)
        f = hits["dist"] != cr.LARGE
        assert f.sum() > 100
        flat = po.shade_params((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1)
        want = po.shade(b, r[f], hits[f], flat)[0]
        np.testing.assert_array_equal(csr.albedo(b, hits[f]).view(np.uint32), want.view(np.uint32))
        if name == "tex_mix":
            import shading_ref as sr
            assert sr.shade(b, r[f], hits[f], flat)[2]["textured"].any()


def _seen(b, cam, w=csr.W, h=csr.H):
    return (cr._trace(b, cr.rays(cam, w, h))["dist"] != cr.LARGE).sum()


def _non_vacuous(po, b, cam, radius, what, w=csr.W, h=csr.H, y0=0, y1=None, spps=(5, 16), seeds=(0, 7), enclosed=False):
    pp = po.shade_params()
    prim = csr.primary(b, cr.rays(cam, w, h, y0, h if y1 is None else y1), pp)
    for spp in spps:
        _, _, opn, _ = csr.ao_frame(b, cam, w, h, pp, spp, radius, 0, y0, y1, prim)
        o = opn.reshape(-1)[prim["fi"]]
        assert ((o > 0) & (o < spp)).any(), "%s spp %d: no partly occluded pixel" % (what, spp)
        assert (o == spp).any(), "%s spp %d: no fully open pixel" % (what, spp)
    for seed in seeds:
        info = {}
        csr.gi_frame(b, cam, w, h, pp, seed, y0, y1, prim, info)
        # (enclosed: a camera inside a closed surface -- no bounce ray can miss, whatever the seed)
        assert info["bounce_found"].any() and (enclosed or not info["bounce_found"].all()), "%s seed %d: bounce rays all hit or all miss" % (what, seed)


@pytest.mark.parametrize("name", csr.HALL_CAMERA_NAMES)
def test_hall_cases_are_not_vacuous(po, vrt, scene_of, name):
    b = scene_of("mirror_hall")
    cam = csr.hall_cameras(vrt)[name]
    if name in ("far_cancel", "beyond_2_60"):   # (those two look past the hall from 2^40 / 2^61 away)
        assert _seen(b, cam) == 0
        return
    assert _seen(b, cam) > 0
    _non_vacuous(po, b, cam, csr.hall_radius(name), name, enclosed=name == "inside_blob")


def test_small_shapes_are_not_vacuous(po, vrt, scene_of):
    """the 13 x 7 frame and the row window of the GPU test"""
    b = scene_of("mirror_hall")
    assert sorted(csr.hall_cameras(vrt)) == sorted(csr.HALL_CAMERA_NAMES)
    _non_vacuous(po, b, csr.hall_cameras(vrt, 13, 7)["axis_aligned"], csr.RADIUS["mirror_hall"], "13x7", 13, 7, spps=(5,), seeds=(0,))
    _non_vacuous(po, b, csr.orbit(vrt, 2), csr.RADIUS["mirror_hall"], "window", y0=11, y1=37, spps=(5,), seeds=(0,))


def test_golden_and_chain_cases_are_not_vacuous(po, vrt, scene_of):
    for name in ("tex_mix", "teapot_x3"):
        for cname, cam in csr.golden_cameras(vrt).items():
            _non_vacuous(po, scene_of(name), cam, csr.RADIUS[name], name + " " + cname, spps=(5,), seeds=(3,))
    _non_vacuous(po, scene_of("chain20"), csr.chain_camera(vrt), csr.RADIUS["chain20"], "chain", spps=(5,), seeds=(1,))


def test_hostile_cameras_leave_the_fast_domain(vrt):
    """What the GPU test's deferral check relies on: these cameras put primary rays outside the fast traversal's domain (the main launch
    defers them to the EXACT launch) -- every ray of beyond_2_60, the centre column / row of axis_aligned at odd sizes."""
    cams = csr.hall_cameras(vrt)
    assert not csr.in_fast_domain(cr.rays(cams["beyond_2_60"], csr.W, csr.H)).any()
    assert not csr.in_fast_domain(cr.rays(cams["far_cancel"], csr.W, csr.H)).all()
    small = csr.in_fast_domain(cr.rays(csr.hall_cameras(vrt, 13, 7)["axis_aligned"], 13, 7)).reshape(7, 13)
    assert not small[:, 6].any() and not small[3, :].any() and small[0, 0]
    assert csr.in_fast_domain(cr.rays(cams["framing"], csr.W, csr.H)).all()
