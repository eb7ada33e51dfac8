"""CPU: the case table of tests/ao_tail_cases.py (what tests/test_gpu_ao_tail.py renders) is not vacuous, shown from the restatements
alone: every frame but the all-miss one has pixels without a hit and pixels with one; among the latter a partly occluded one; and,
where the table says so, one whose samples are all open or all blocked.  The batch and bin arithmetic the GPU tests rely on is
restated here too, so that a case that no longer splits the way its comment says fails without a GPU."""
import pytest

import ao_tail_cases as atc


@pytest.mark.parametrize("case", [c for c in atc.CASES if c.name != "all_miss"], ids=lambda c: c.name)
def test_case_is_not_vacuous(vrt, po, case):
    pixels, hit, opened, partly, closed = atc.census(vrt, po, case)
    assert pixels == case.w * (case.y1 - case.y0) and opened + partly + closed == hit
    assert 0 < hit < pixels, "%s: %d of %d pixels hit" % (case.name, hit, pixels)
    assert partly > 0, "%s: no partly occluded pixel" % case.name
    if case.open_or_closed:
        assert opened + closed > 0, "%s: no fully open and no fully blocked pixel" % case.name
    (_, _, _, rays), _ = atc.camera_reference(vrt, po, case)
    assert rays == pixels + hit * case.spp
    # the fixed camera's frame of the same window: misses, hits, partly occluded pixels
    _, _, cnt, rays = atc.fixed_reference(vrt, po, case)
    cnt = cnt[case.y0:case.y1]
    hit = (rays - pixels) // case.spp
    assert (rays - pixels) % case.spp == 0 and 0 < hit < pixels
    assert ((cnt > 0) & (cnt < case.spp)).any(), "%s fixed camera: no partly occluded pixel" % case.name


def test_the_all_miss_camera_sees_nothing(vrt, po):
    case = atc.BY_NAME["all_miss"]
    assert atc.census(vrt, po, case) == (case.w * case.h, 0, 0, 0, 0)
    (_, _, opn, rays), _ = atc.camera_reference(vrt, po, case)
    assert rays == case.w * case.h and not opn.any()


def test_batch_and_bin_arithmetic_of_the_table():
    c = atc.BY_NAME
    assert atc.batches(c["spp7"], 2880) == [3, 3, 1] and atc.batches(c["small65"], 2880) == [31, 31, 3]
    assert atc.batches(c["rows"], 2880) == [3, 2] and atc.batches(c["one_row"], 2880) == [72, 58]
    assert atc.batches(c["cells143"], 2880) == [1, 1, 1] and atc.batches(c["spp16"], 1) == [1] * 16
    assert all(atc.batches(k, 32 << 20) == [k.spp] for k in atc.CASES)   # the default: one batch, which is why the knob exists
    assert atc.n_cells(c["cells143"]) == 143 and atc.n_cells(c["cells272"]) == 272
    per = {k.name: (8 * atc.n_cells(k) + 1023) // 1024 for k in atc.CASES}
    assert per["cells143"] == 2 and per["cells272"] == 3 and all(v == 1 for n, v in per.items() if n not in atc.LARGE_WINDOWS)
    assert sorted(atc.SAMPLE_COUNTS + atc.ROW_WINDOWS + atc.LARGE_WINDOWS + ["all_miss"]) == sorted(c)
