"""CPU: the requests of tests/launch_geometry_cases.py have the shard shapes claimed for them, from per_shard restated
(((n + 7) / 8 + 63) & ~63 for the RTU path, ceil(tiles / 8) for the twin); the comparison of two runs sees one differing word; the
counter check accepts what a launch can leave and nothing else."""
import numpy as np

import launch_geometry_cases as lg
import request_programs as rp


def _frames(section, w, h):
    return [s for s in lg.SECTIONS[section][2] if s[1] == "render" and (rp.args_of(s)["w"], rp.args_of(s)["h"]) == (w, h) and rp.args_of(s)["depth"] == 1]


def test_frames_fall_across_the_shards_as_claimed():
    assert lg.per_shard(1) == 64 and lg.per_shard(512) == 64 and lg.per_shard(513) == 128       # the restated form itself
    # 13 x 7: two tiles, one per shard; six shards past the end
    assert lg.shard_jobs(lg.frame_jobs(13, 0, 7)) == [64, 64, 0, 0, 0, 0, 0, 0]
    # 72 x 8: nine tiles, 128 jobs per shard: four full, a fifth with 64, three past the end
    assert rp.tiles(72, 0, 8)[2] == 9 and lg.shard_jobs(lg.frame_jobs(72, 0, 8)) == [128, 128, 128, 128, 64, 0, 0, 0]
    # 16 x 12 and 64 x 64: an a-priori list (the side launch and its reserve run); 64 x 64 fills all eight shards exactly
    assert len(rp.apriori(16, 12, 0, 12)) > 0 and len(rp.apriori(64, 64, 0, 64)) > 0 and len(rp.apriori(13, 7, 0, 7)) == 0
    assert lg.shard_jobs(lg.frame_jobs(16, 0, 12)) == [64] * 4 + [0] * 4
    assert lg.shard_jobs(lg.frame_jobs(64, 0, 64)) == [512] * 8 and lg.per_shard(4096) * 8 == 4096
    # 200 x 120: 375 tiles, 3,008 jobs per shard, a short last shard
    assert rp.tiles(200, 0, 120)[2] == 375 and lg.shard_jobs(lg.frame_jobs(200, 0, 120)) == [3008] * 7 + [2944]
    # 96 x 64, rows 11..37: a window inside the frame
    w, h, y0, y1 = lg.WINDOW
    assert 0 < y0 < y1 < h and y0 % 8 and (y1 - y0) % 8 and rp.tiles(w, y0, y1)[:2] == (12, 4)
    # 512 x 384: 196,608 jobs need 768 workgroups -- more than one per CU of a 256-CU device holds at once, so under
    # VXRT_WGS_PER_CU=1 a wavefront takes 196,608 / (256 x 4 x 64) = 3 reservations
    assert lg.frame_jobs(512, 0, 384) == 196608 and lg.workgroups_needed(196608) == 768 > 256
    for section in ("cornell", "hall"):
        for w, h in lg.FRAME_SIZES:
            assert [rp.args_of(s)["shadow"] for s in _frames(section, w, h)] == [0, 1], (section, w, h)
        assert len(_frames(section, 96, 64)) == 2


def test_traces_fall_across_the_shards_as_claimed():
    assert lg.shard_jobs(513) == [128, 128, 128, 128, 1, 0, 0, 0]
    assert lg.shard_jobs(4097) == [576] * 7 + [65]
    assert lg.shard_jobs(1) == [1] + [0] * 7 and lg.shard_jobs(63)[:2] == [63, 0] and lg.shard_jobs(64)[:2] == [64, 0] and lg.shard_jobs(65)[:3] == [64, 1, 0]
    assert lg.shard_jobs(20000) == [2560] * 7 + [2080]
    for n in lg.TRACE_COUNTS:
        assert sum(lg.shard_jobs(n)) == n
    # the axis-parallel buffer: 513 deferred jobs for the EXACT launch's fixed 128 workgroups (n / 8 / 256 workgroups is fewer)
    assert lg.AXIS_N == 513 and lg.workgroups_needed(lg.AXIS_N // 8) < lg.EXACT_GRID
    for scene in ("cornell", "hall"):
        r = lg.axis_rays(scene, lg.AXIS_N, lg.AXIS_SEED)
        assert r.shape == (513, 6) and ((r[:, 3:] == 0).sum(1) == 2).all()
    for section, src in (("cornell", "fan"), ("hall", None)):
        t = [rp.args_of(s) for s in lg.SECTIONS[section][2] if s[1] == "trace"]
        assert sorted(a["n"] for a in t if a["mode"] == 0 and a.get("src") == src) == sorted(lg.TRACE_COUNTS)
        assert sorted(a["n"] for a in t if a["mode"] == 1 and a["tmax"] == 1) == sorted(lg.TRACE_COUNTS)
        assert sum(a.get("src") == "axis" for a in t) == 1


def test_the_twins_shards_count_tiles():
    assert lg.twin_shard_tiles(72, 0, 8) == [2, 2, 2, 2, 1, 0, 0, 0]
    assert lg.twin_shard_tiles(13, 0, 7) == [1, 1, 0, 0, 0, 0, 0, 0]
    assert lg.twin_shard_tiles(64, 0, 64) == [8] * 8
    assert {(w, h) for _, w, h in lg.TWIN} == {(13, 7), (72, 8), (64, 64)} and len({n for n, _, _ in lg.TWIN}) == 2


def test_sections_and_settings_cover_what_they_name():
    assert lg.SECTIONS["cornell"][0] == "cornell" and lg.SECTIONS["hall"][0] == "hall"
    assert rp.mut("in_flight", 3) in lg.SECTIONS["hall_in_flight"][1]
    for section in ("cornell", "hall"):
        kinds = {s[1] for s in lg.SECTIONS[section][2]}
        assert {"render", "render_camera", "rows_batch", "gi", "trace", "ao", "path", "frame"} <= kinds
        assert any(s[1] == "render" and rp.args_of(s)["depth"] == 3 for s in lg.SECTIONS[section][2])
    forms = [rp.args_of(s) for s in lg.SECTIONS["hall"][2] if s[1] == "frame"]
    assert any(a["form"] == "mis" and a.get("specular") for a in forms) and any(a["form"] == "mis" and not a.get("specular") for a in forms)
    assert any(a.get("counts") is not None for a in forms) and any(a.get("dn") for a in forms) and any((a.get("w"), a.get("h")) == (96, 64) for a in forms)
    assert set(lg.KNOB_NAMES) == {"VXRT_GRID_MAX", "VXRC_GRID_MAX", "VXRT_PACKED", "VXRT_GRID_DIV", "VXRT_SIDE_RESERVE", "VXRT_SHARD_ROT", "VXRT_WGS_PER_CU",
                                  "VXRT_UNORDERED_ANY"}
    assert len(lg.SETTINGS) == 9 and lg.SETTINGS["ordered_any"]["env"] == {"VXRT_UNORDERED_ANY": "0"}
    assert all(lg.logged(s) == (lg.jobs_of(s) is not None and rp.args_of(s).get("depth", 1) == 1) for sec in lg.SECTIONS.values() for s in sec[2])


def test_one_differing_word_is_seen():
    rng = np.random.default_rng(1)
    run = {lg.key("hall", 3, "dst"): rng.integers(0, 2 ** 32, 200, dtype=np.uint64).astype(np.uint32),
           lg.key("hall", 3, "rc"): np.array([0], np.uint32), lg.key("twin", 0, "col"): rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32),
           lg.key("hall", 3, "_waves"): np.array([12], np.uint32)}
    same = {k: v.copy() for k, v in run.items()}
    assert lg.differences(same, run) == []
    same[lg.key("hall", 3, "_waves")][0] = 4                    # an observation, not an output
    assert lg.differences(same, run) == []
    for k in (lg.key("hall", 3, "dst"), lg.key("twin", 0, "col"), lg.key("hall", 3, "rc")):
        for word in (0, len(run[k]) - 1):                        # the last word of an output is a guard word
            other = {n: v.copy() for n, v in run.items()}
            other[k][word] ^= 1
            assert lg.differences(other, run) == [(k, 1)]
    missing = dict(run)
    del missing[lg.key("twin", 0, "col")]
    assert lg.differences(missing, run) == [(lg.key("twin", 0, "col"), "missing")] == lg.differences(run, missing)
    assert lg.differences({k: (v[:-1] if v.size > 1 else v) for k, v in run.items()}, run)[0][1].startswith("shape")


def test_the_counter_check():
    def ctl(counters, base=32):
        c = np.zeros(32 + 2 * lg.SHARDS * lg.STRIDE, np.uint32)
        c[base:base + lg.SHARDS * lg.STRIDE:lg.STRIDE] = counters
        return c
    # 513 jobs, one workgroup: every in-range shard handed out and found dry once by each of 4 wavefronts at most
    assert lg.counters_ok(ctl([192, 192, 192, 192, 128, 0, 0, 0]), 513, 4) is None
    assert lg.counters_ok(ctl([128, 128, 128, 128, 64, 0, 0, 0]), 513, 4) is None
    assert lg.counters_ok(ctl([128 + 64 * 4] * 4 + [64 + 64 * 4, 0, 0, 0]), 513, 4) is None
    assert "past the end" in lg.counters_ok(ctl([192, 192, 192, 192, 128, 64, 0, 0]), 513, 4)        # an atomic on a shard past the end
    assert "shard 4" in lg.counters_ok(ctl([192, 192, 192, 192, 0, 0, 0, 0]), 513, 4)                # a shard nobody drew from
    assert "shard 1" in lg.counters_ok(ctl([192, 64, 192, 192, 128, 0, 0, 0]), 513, 4)               # jobs never handed out
    assert "shard 0" in lg.counters_ok(ctl([193, 192, 192, 192, 128, 0, 0, 0]), 513, 4)              # not a multiple of the chunk
    assert "shard 2" in lg.counters_ok(ctl([192, 192, 128 + 64 * 5, 192, 128, 0, 0, 0]), 513, 4)     # more failing draws than wavefronts
    assert lg.counters_ok(ctl([128, 128, 128, 128, 64, 0, 0, 0], 32 + 256), 513, 512, "exact") is None
    assert lg.counters_ok(ctl([0] * 8, 32 + 256), 0, 512, "exact") is None and lg.counters_ok(ctl([64] + [0] * 7, 32 + 256), 0, 512, "exact") is not None


def test_the_end_log_reader():
    log = np.zeros((lg.END_LOG_WAVES, 2), np.uint64)
    log[0] = (1000, 64 | (3 << 56))
    log[1] = (1001, 0 | (3 << 56))           # a wavefront that started no ray still left its clock
    log[7] = (1002, 5 | (6 << 56))
    assert lg.read_log(log.reshape(-1)) == (3, 69, [3, 6])
