"""CPU: the case generator of tests/builder_cases.py and the host builder (csrc/scene_builder.cpp, scene.from_triangles) on its
hostile families -- geometry where surface areas overflow, underflow or tie everywhere.  The tree must stay inside the traversal's 32
levels with leaves of a few triangles, its bytes must be the ones the numpy restatement of the quantiser (tests/refit_ref.py) computes
from the triangles, and the oracle on it must find what a loop over every triangle finds.  Also pins the bytes of the scenes the suite
and the benchmark build, and the hit counts the GPU tests (tests/test_gpu_bvh_hostile.py) rely on."""
import hashlib

import numpy as np
import pytest

import builder_cases as bc
import refit_ref as rr
from test_scene_builder import NODE, brute_force, check_tree_fast


def test_families_are_what_they_say():
    for n in (16, 300, 1025):
        for kind in bc.FINITE:
            t = bc.family(kind, n)
            assert t.shape == (n, 9) and t.dtype == np.float32 and np.isfinite(t).all(), kind
            assert np.array_equal(t, bc.family(kind, n)), kind                   # seeded
        v = lambda kind: bc.family(kind, n).reshape(n, 3, 3)
        assert (v("point") == v("point")[0, 0]).all() and (v("dups") == v("dups")[0]).all()
        assert (v("plane")[..., 2] == 3).all() and (v("line")[..., 1] == 100).all() and (v("line")[..., 2] == 0).all()
        assert np.abs(v("subnormal")).max() < np.finfo(np.float32).tiny and np.abs(v("subnormal")).max() > 0
        assert v("range")[0].min() > 9e29 and np.abs(v("range")[1:]).max() < 400
        sc = v("same_centre")
        assert len(np.unique((sc.min(1) + sc.max(1)) / 2, axis=0)) <= 8           # box centres coincide (up to the rounding of c +- u r)
        with np.errstate(over="ignore"):
            ext = np.ptp(v("huge").reshape(-1, 3), axis=0)
            assert np.isfinite(ext).all() and np.isinf(ext[0] * ext[1])
            assert np.isinf(np.ptp(v("overflow").reshape(-1, 3), axis=0)).any() and np.isfinite(v("overflow")).all()
        assert np.isnan(v("nan_vertex")).any(2).sum() == (n + 19) // 20
        assert np.isnan(v("nan_tri")).all((1, 2)).sum() == 3
        assert np.isinf(v("inf_vertex")).sum() == 1
    for kind in bc.BOX_KINDS:
        for n in (1, 2, 3, 300):
            b = bc.boxes(kind, n)
            assert b.shape == (n, 6) and np.isfinite(b).all() and (b[:, 3:] >= b[:, :3]).all(), kind
    b = bc.boxes("nested", 300)
    assert (b[1:, :3] > b[:-1, :3]).all() and (b[1:, 3:] < b[:-1, 3:]).all()
    assert (bc.boxes("coincident", 300) == bc.boxes("coincident", 300)[0]).all()
    f = bc.boxes("flat", 300)
    assert (f[:, 1] == f[:, 4]).all() and (f[::3, :3] == f[::3, 3:]).all() and (f[1::3, 0] < f[1::3, 3]).all()
    assert np.isnan(bc.boxes("nan_box", 300)).sum() == 1


def _max_leaf(sc):
    return int(sc["bvh"].view(NODE)["ld"].max())


@pytest.mark.parametrize("n", [16, 300])
@pytest.mark.parametrize("kind", bc.FINITE)
def test_cpu_builder_on_hostile_families(vrt, po, kind, n):
    tri = bc.family(kind, n)
    sc = vrt.scene.from_triangles([tri])
    depth = check_tree_fast(sc)
    assert depth == sc.info["max_depth"] and depth < 32
    ml = _max_leaf(sc)
    assert ml == sc.info["max_leaf"] and ml <= (15 if kind in bc.INDISTINGUISHABLE else 4)
    rows = lambda t: sorted(r.tobytes() for r in np.ascontiguousarray(t))
    assert rows(sc["tri"].view(np.float32).reshape(-1, 9)) == rows(tri)
    # origin, exponents and every quantised plane against the restatement, from the triangles up
    _, want = rr.refit({k: sc[k] for k in ("tlas", "blas", "bvh", "tri")}, geometry=True)
    assert np.array_equal(want, sc["bvh"])
    rays = bc.rays_at(tri, kind)
    assert len(rays) >= 90
    h, _ = po.trace_canonical(sc, rays)
    hits = int((h["dist"] < 1e29).sum())
    print("%s n %d: depth %d, %d nodes, largest leaf %d, %d of %d aimed rays hit" % (kind, n, depth, sc.n_bvh_nodes, ml, hits, len(rays)))
    if kind in ("plain", "offset", "range", "dups"):        # (`plane`: zero-thickness boxes, grazing hits differ -- DESIGN.md s3)
        assert np.array_equal(h["dist"], brute_force(sc, rays, po))
    if n >= 300:
        assert hits >= 10 if kind in bc.HITTING else hits == 0


# (family, size) pairs the GPU tests trace with a hit cap ("at least 10 of 96 aimed rays" for the hitting families at n >= 300): a hit
# depends on the triangles, not on the tree, so the count on the CPU builder's tree is the count on any correct tree
@pytest.mark.parametrize("kind,n", [(k, n) for k in bc.HITTING for n in (300, 1025)] +
                         [(k, n) for k in ("plain", "dups") for n in bc.SIZES_EDGE if n != 1025])
def test_hit_caps_the_gpu_tests_rely_on(vrt, po, kind, n):
    tri = bc.family(kind, n)
    sc = vrt.scene.from_triangles([tri])
    h, _ = po.trace_canonical(sc, bc.rays_at(tri, kind))
    hits = int((h["dist"] < 1e29).sum())
    print("%s n %d: %d of 96 aimed rays hit" % (kind, n, hits))
    assert hits >= 10


# SHA-256 of bvh + tri + triEx as built by commit 6820a59 ("Emissive path frames: multiple importance sampling of area lights"), the parent
# of the change that gave build_binary its median split of last resort: that split, the stay-put rule of the reinsertion and the
# leaf rule of the collapse act on degenerate nodes only, the trees of the suite and of the benchmark are the same bytes
_PARENT_SHA = {
    ("cornell", 0, 0, 1): "69b12cfb49cb9180068ae83a4304c63cf5aae6038688bc0843445dd05ebbefff",
    ("blob", 3, 0, 2): "cae8158417d78b2cb4043585971dc4c5a65a22350187dd673e04954f69008f29",
    ("atrium", 6, 0, 3): "c1b122b47d89d509948005d960fc90978d5b0f801ee254ce5e6eda18acc39738",
    ("hairball", 60, 20, 7): "9638beb89297e94f719c53d9b4f1a8a8548b880c78684af8e6154049337dc499",
}


@pytest.mark.parametrize("args", list(_PARENT_SHA))
def test_standard_scenes_keep_their_bytes(vrt, monkeypatch, args):
    monkeypatch.delenv("VXRT_SCENE_CACHE", raising=False)
    sc = vrt.scene.procedural(*args)
    assert hashlib.sha256(sc["bvh"].tobytes() + sc["tri"].tobytes() + sc["triEx"].tobytes()).hexdigest() == _PARENT_SHA[args]


def test_the_fallback_split_does_not_depend_on_the_thread_count(vrt, monkeypatch):
    ref = None
    for threads in ("1", "8"):
        monkeypatch.setenv("VXS_THREADS", threads)
        got = [vrt.scene.from_triangles([bc.family(kind, 5000)])["bvh"].tobytes() for kind in ("tiny", "dups", "huge")]
        ref = ref or got
        assert got == ref
