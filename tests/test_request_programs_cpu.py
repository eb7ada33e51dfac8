"""CPU: the request programs of tests/request_programs.py have the properties tests/test_gpu_request_programs.py relies on -- the step
pairs of program A, the window and batch arithmetic behind program B (window_tiles, ensure_apriori and lpt_wanted of
csrc/rt_kernels.hip, restated there), and the shape of the refusal and refit programs."""
import request_programs as rp
import specular_cases as sc


def _requests(program):
    return [s for s in program if rp.is_request(s)]


def _pairs(program):
    r = _requests(program)
    return list(zip(r, r[1:]))


def _kw(step):
    return rp.args_of(step)


def _path_like(step):
    return step[1] in ("path", "frame")


def test_steps_are_well_formed():
    kinds = {"render", "render_camera", "interleaved", "rows_batch", "batch", "batch_camera", "ao", "gi", "trace", "path", "frame", "emitter_rays", "hit_weights"}
    mutators = {"emitters", "alpha", "snapshot", "transforms", "deform", "in_flight"}
    for name, (scene, program) in rp.PROGRAMS.items():
        assert scene in ("hall", "mirror_hall", "teapot", "cornell", "tex_mix")
        for s in program:
            assert s[0] in ("req", "hist", "mut", "info"), (name, s)
            assert s[0] != "mut" or s[1] in mutators
            assert not rp.is_request(s) or (s[1] in kinds and _kw(s)["rc"] in (0, -1))
            hash(s)
        assert any(rp.is_request(s) for s in program)
        if scene != "hall":     # only the hall has emitters
            assert not any(rp.is_request(s) and (s[1] in ("emitter_rays", "hit_weights") or _kw(s).get("form")) for s in program), name


def test_program_a_holds_every_form_twice_behind_different_predecessors():
    reqs = _requests(rp.A_PROGRAM)
    assert rp.A_PROGRAM[0] == rp.mut("emitters", 1) and all(rp.is_request(s) for s in rp.A_PROGRAM[1:])
    before = {}
    for i, s in enumerate(reqs):
        before.setdefault(s, set()).add(reqs[i - 1] if i else None)
    assert all(len(v) >= 2 for v in before.values()), [k for k, v in before.items() if len(v) < 2]
    first_path = next(s for s in reqs if _path_like(s))
    assert reqs[-1] == first_path == rp.PATH
    # the forms of the issue's list
    forms = set(reqs)
    assert {rp.PLAIN, rp.MIRROR, rp.SHADOW_CAM, rp.AO, rp.GI, rp.TRACE_CLOSEST, rp.TRACE_ANY, rp.PATH, rp.DENOISED, rp.NO_BOUNCES, rp.DEEP, rp.FIVE} <= forms
    assert set(rp.EMITTER.values()) | set(rp.SPECULAR.values()) | set(rp.COUNTS.values()) <= forms
    assert {(f, s) for f in ("nee0", "nee1", "mis") for s in (0, 1)} == set(rp.EMITTER) and set(rp.SPECULAR) == set(sc.FORMS)
    assert _kw(rp.MIRROR)["depth"] > 1 and _kw(rp.NO_BOUNCES)["bounces"] == 0 and _kw(rp.DEEP)["bounces"] == 16
    assert _kw(rp.TRACE_CLOSEST)["mode"] == 0 and _kw(rp.TRACE_ANY)["mode"] == 1


def test_program_a_holds_the_pairs_where_a_leftover_would_show():
    pairs = _pairs(rp.A_PROGRAM)
    size = lambda s: (_kw(s).get("w", rp.W), _kw(s).get("h", rp.H))
    plain = lambda s: _path_like(s) and not _kw(s).get("specular") and not _kw(s).get("form") and _kw(s).get("counts") is None and not _kw(s).get("dn")

    def has(pred):
        return any(pred(a, b) for a, b in pairs)
    assert has(lambda a, b: _kw(a).get("specular") and plain(b) and size(a) == size(b))
    assert has(lambda a, b: _kw(a).get("specular") and _kw(a).get("form") == "mis" and _kw(b).get("form") == "nee1" and not _kw(b).get("specular"))
    counts = lambda s: _kw(s).get("counts") is not None
    assert has(lambda a, b: counts(a) and _path_like(b) and not counts(b)) and has(lambda a, b: _path_like(a) and not counts(a) and counts(b))
    assert has(lambda a, b: _path_like(a) and _path_like(b) and _kw(a)["shadow"] == 1 and _kw(b)["shadow"] == 0)
    assert has(lambda a, b: _path_like(a) and _path_like(b) and _kw(a)["bounces"] % 2 == 1 and _kw(b)["bounces"] % 2 == 0 and _kw(b)["bounces"] > 0)
    assert has(lambda a, b: size(a) == (96, 64) and size(b) == (13, 7) and (_kw(b)["y0"], _kw(b)["y1"]) == (2, 6) and _path_like(a) and _path_like(b))
    assert has(lambda a, b: a[1] == "ao" and _path_like(b))
    paths = max(size(s)[0] * size(s)[1] * _kw(s)["spp"] for s in _requests(rp.A_PROGRAM) if _path_like(s))
    assert has(lambda a, b: a[1] == "trace" and _kw(a)["n"] > paths and _path_like(b))
    # in the child a frame takes several batches whose boundaries fall inside pixels
    assert rp.CHILD_PATH_BATCH < rp.W * rp.H * rp.SPP and rp.CHILD_PATH_BATCH % (rp.W * rp.H) != 0 and rp.CHILD_PATH_BATCH % 3 != 0
    assert 1 <= rp.CHILD_AO_BATCH // (rp.W * rp.H) < _kw(rp.AO)["spp"]


def test_program_b_table_has_the_properties_claimed():
    # equal tile counts where W differs
    (w0, h0), (w1, h1), (w2, h2) = rp.B_SIZES
    assert w0 != w1 and w0 * h0 == w1 * h1 and (w0, h0) == (w2, h2)
    assert rp.tiles(w0, 0, h0)[2] == rp.tiles(w1, 0, h1)[2]
    # the a-priori lists of the windows: with the column x = W / 2 every window has entries; without it only the windows that hold row H / 2
    lists = {(w, win): rp.apriori(w, 12, *win) for w in rp.B_WIDTHS for win in rp.B_WINDOWS}
    assert all(len(lists[(16, win)]) > 0 for win in rp.B_WINDOWS)
    assert lists[(13, (0, 6))] == [] and len(lists[(13, (6, 12))]) == 13 and len(lists[(13, (0, 12))]) == 13
    assert len(lists[(16, (0, 6))]) == 6 and len(lists[(16, (6, 12))]) == 6 + 16 - 1 and len({tuple(v) for v in lists.values()}) == len(lists)
    windows = [(k["w"], k["h"], k["y0"], k["y1"]) for k in map(rp.args_of, rp.B_PROGRAM) if "y0" in k]
    assert {(w, 12) + win for w in rp.B_WIDTHS for win in rp.B_WINDOWS} <= set(windows)
    # batches on one window: the held list serves a smaller batch as a prefix and is rebuilt for a larger one
    for kind in ("rows_batch", "batch"):
        held, smaller, larger, key = 0, 0, 0, None
        for s in rp.B_PROGRAM:
            k = rp.args_of(s)
            if s[1] != kind:
                continue
            this = (k["w"], k["h"], k.get("y0"), k.get("y1"))
            if this != key:
                key, held = this, 0
            smaller += 0 < k["nf"] < held
            larger += held != 0 and k["nf"] > held
            held = max(held, k["nf"])
        assert smaller >= 2 and larger >= 1, kind
    assert any(s[1] == "rows_batch" and rp.args_of(s)["nf"] == 1 for s in rp.B_PROGRAM)
    # interleaved: both phases of stride 2, then stride 1
    inter = [(rp.args_of(s)["phase"], rp.args_of(s)["stride"]) for s in rp.B_PROGRAM if s[1] == "interleaved"]
    assert inter == [(0, 2), (1, 2), (0, 1)]
    h = next(rp.args_of(s)["h"] for s in rp.B_PROGRAM if s[1] == "interleaved")
    assert rp.tiles(16, 0, h, 2)[1] == 2 and rp.tiles(16, 8, h, 2)[1] == 1 and rp.tiles(16, 0, h, 1)[1] == 3
    # shadow 0 / 1 and the camera frame, three times each on one window
    for r in (rp._render(), rp._render(shadow=1), rp.req("render_camera", cam="orbit_1", shadow=0)):
        assert rp.B_PROGRAM.count(r) >= 3


def test_learned_tile_orders_need_the_large_frame():
    n = rp.tiles(rp.LPT_W, 0, rp.LPT_H)[2]
    assert n >= rp.lpt_min_tiles() > rp.tiles(96, 0, 64)[2]
    assert rp.LPT_W * rp.LPT_H * 4 < 8 << 20        # (one output of a few megabytes)
    for r in set(rp.B_LPT_PROGRAM):
        k = rp.args_of(r)
        assert (k["w"], k["h"]) == (rp.LPT_W, rp.LPT_H) and k["lean"]
        # three times in a row: the second and third find the order the one before left; and once more behind each of the others
        runs = [i for i in range(len(rp.B_LPT_PROGRAM) - 2) if rp.B_LPT_PROGRAM[i:i + 3] == [r] * 3]
        assert runs and len({rp.B_LPT_PROGRAM[i - 1] for i, s in enumerate(rp.B_LPT_PROGRAM) if s == r and i}) >= 2


def test_refit_programs():
    p = rp.C_EMITTERS
    assert [s[1:3] for s in p if s[0] == "info"] == [(8, "positive"), (7, 0), (7, "positive"), (8, 0), (8, "positive")]
    p = [s for s in p if s[0] != "info"]
    i = p.index(rp.mut("transforms", rp.ec.LAMP, "lamp_moved"))
    assert rp.args_of(p[i + 1])["rc"] == -1 and rp.args_of(p[i + 1])["form"] == "mis" and rp.args_of(p[i - 1])["form"] == "mis"
    assert [rp.args_of(s)["form"] for s in p[i + 2:i + 4]] == ["nee0", None] and p[i + 4] == rp.mut("emitters", 1) and rp.args_of(p[i + 5])["form"] == "mis"
    m = rp.C_MOTION
    assert [s[1] for s in m if s[0] == "mut"] == ["snapshot", "transforms", "snapshot", "transforms"]
    assert sum(s[0] == "hist" for s in m) >= 3 and any(s[1] == "ao" for s in m) and all(rp.args_of(s)["motion"] == 1 for s in m if s[0] == "hist")
    mats = rp._matrices()
    import numpy as np
    assert np.linalg.det(mats["singular"].astype(np.float64)) == 0 and np.linalg.det(mats["lamp_moved"].astype(np.float64)) != 0
    assert not np.array_equal(mats["lamp_moved"], mats["lamp_moved_twice"]) and not np.array_equal(mats["translation"], mats["identity"])
    for program in rp.C_IDENT.values():
        stages = [[]]
        for s in program:
            if s[0] == "mut":
                stages.append([])
            elif rp.is_request(s):
                stages[-1].append(s)
        assert len(stages) == 4 and all(st == stages[0] and len(st) == 5 for st in stages)
        assert {s[1] for s in stages[0]} == {"render", "ao", "path", "trace"}
        info = [s[1:] for s in program if s[0] == "info"]
        assert info[:6] == [(2, 1), (5, "fresh"), (2, 0), (5, 0), (2, 1), (5, "fresh")]
    r = rp.C_REFUSED
    assert [s for s in r if s[0] == "mut"][-1][3] is False and set(rp.CORE) <= set(r[r.index(rp.mut("transforms", rp.ec.LAMP, "singular", ok=False)):])


def test_refusal_programs():
    d = rp.D_PROGRAM
    reqs = _requests(d)
    assert [s for s in reqs if rp.args_of(s)["rc"] == 0] == rp.CORE + rp.CORE[:1]
    for a, b in zip(reqs, reqs[1:]):
        assert rp.args_of(a)["rc"] == 0 or rp.args_of(b)["rc"] == 0                 # a refusal stands between two forms that succeed
    no = [rp.args_of(s) for s in rp.REFUSALS]
    assert any(k.get("null") == "path" for k in no) and any(k.get("spp") == 0 for k in no) and any(k.get("dn") and k.get("specular") for k in no)
    assert any(k.get("y0", 0) > k.get("y1", rp.H) for k in no) and all(k["rc"] == -1 for k in no) and len(rp.REFUSALS) == len(rp.CORE)
    a = rp.D_ALPHA
    on = False
    for s in a:
        if s[0] == "mut":
            on = bool(s[2][0])
        else:
            assert (rp.args_of(s)["rc"] == -1) == (on and s[1] != "render")
    assert sum(rp.args_of(s)["rc"] == -1 for s in _requests(a)) == 4


def test_several_contexts_program():
    e = rp.E_PROGRAM
    muts = [s for s in e if s[0] == "mut"]
    assert muts == [rp.mut("emitters", 1), rp.mut("in_flight", 3), rp.mut("in_flight", 1)]
    i, j = e.index(muts[1]), e.index(muts[2])
    # three contexts round robin under two streams: a form lands on contexts with different pasts
    assert len(e[i + 1:j]) == 2 * len(rp.CORE) and len(e[i + 1:j]) % 3 != 0 and e[j + 1:] == rp.CORE


def test_the_comparison_sees_one_word():
    """Runner._same, untouched and rays_traced on made-up outputs: one differing word, one touched word, a missing output"""
    import numpy as np
    import pytest
    fmark = np.array([rp.FMARK], np.float32).view(np.uint32)[0]
    out = {"dst": np.full(40, rp.MARK, np.uint32), "col": np.full(40, fmark, np.uint32), "cnt": np.full(4, rp.CMARK, np.uint64).view(np.uint32).copy(),
           "rc": np.array([0xFFFFFFFF], np.uint32), "status": np.zeros(1, np.uint32)}
    copy = lambda: {k: v.copy() for k, v in out.items()}
    assert rp.untouched(out) and rp.rays_traced(out) == 0
    rp.Runner._same(copy(), out, "equal")
    for k in out:
        bad = copy()
        bad[k][0] ^= 1
        with pytest.raises(AssertionError):
            rp.Runner._same(bad, out, "one word of " + k)
        assert k in ("rc", "status") or not rp.untouched(bad)
        bad = copy()
        bad[k][-1] ^= 0x80000000
        with pytest.raises(AssertionError):
            rp.Runner._same(bad, out, "the last word of " + k)
    less = copy()
    del less["col"]
    with pytest.raises(AssertionError):
        rp.Runner._same(less, out, "a missing output")
    with pytest.raises(AssertionError):
        rp.Runner._same(out, less, "an output too many")
    counted = copy()
    counted["cnt"][:2] = np.array([rp.CMARK + 192], np.uint64).view(np.uint32)
    assert rp.rays_traced(counted) == 192 and not rp.untouched(counted)
