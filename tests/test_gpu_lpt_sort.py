"""GPU: the longest-tile-first counting sort (lpt_order_block, csrc/rt_kernels.hip) held to its definition, which whole-frame
comparisons cannot see: within each of the eight bands of tiles, the order is a permutation of the band's tiles and their cost
classes do not increase.

(a) the sort alone, through vxrt_internal_lpt_sort (the launch the raycast twin uses), on cost tables no scene produces;
(b) what a frame context learns from real 1920 x 1080 frames (32,400 tiles, above LPT_MIN_TILES), read with vxrt_debug_read_lpt after
    every frame -- frames on a learned order equal the frame on the static one, and a change of the table's key (shadow rays, a row
    window) starts again from a frame that equals a fresh scene's.

Reference: lpt_cls restated in numpy -- monotone, classes 0..1727.  The order inside a class is left to the atomics and is not
pinned.  Everything is exact; nothing is timed."""
import ctypes as C

import numpy as np
import pytest

import scenes

gpu = pytest.mark.gpu     # (per test: the restatement's own test needs no GPU)
SHARDS = 8            # QUEUE_SHARDS: bands of tiles, workgroups of the sort
SENTINEL = 0xDEADBEEF
GUARD = 0xA5A5A5A5
HOSTILE = np.array([0, 1, 63, 64, 65, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)


def lpt_cls(c):
    """the monotone cost class of csrc/rt_kernels.hip: the value itself below 64, else (exponent - 5) << 6 | the six bits under the
    leading one"""
    c = np.asarray(c, np.uint32).astype(np.int64)
    e = np.frexp(np.maximum(c, 1).astype(np.float64))[1].astype(np.int64) - 1     # position of the leading one (exact: c < 2^53)
    big = ((e - 5) << 6) | ((c >> np.maximum(e - 6, 0)) & 63)
    return np.where(c < 64, c, big)


def test_cost_class_restatement_is_monotone_with_classes_0_to_1727():
    edge = np.unique(np.concatenate([np.arange(0, 4200), HOSTILE.astype(np.int64)] +
                                    [np.array([(1 << k) - 1, 1 << k, (1 << k) + 1, (1 << k) + (1 << (k - 6)) - 1, (1 << k) + (1 << (k - 6))]) for k in range(7, 32)]))
    edge = edge[edge <= 0xFFFFFFFF].astype(np.uint32)
    k = lpt_cls(edge)
    assert (np.diff(k) >= 0).all() and k[0] == 0 and k[-1] == 1727 and lpt_cls([63, 64, 65, 127, 128]).tolist() == [63, 64, 65, 127, 128]
    assert lpt_cls([0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]).tolist() == [(25 << 6) | 63, 26 << 6, 1727]


def _costs(n, rng):
    return {"equal": np.full(n, 1000, np.uint32),
            "distinct": (rng.permutation(n).astype(np.uint32) * np.uint32(3) + np.uint32(1)),
            "log_uniform": np.floor(np.exp2(rng.uniform(0.0, 30.0, n))).astype(np.uint32),
            "hostile": HOSTILE[rng.integers(0, len(HOSTILE), n)]}


def check_bands(cost, order, n, tps, what):
    """order[band] is a permutation of the band's tiles with non-increasing cost classes, for each of the eight bands"""
    cls = lpt_cls(cost[:n])
    for s in range(SHARDS):
        lo, hi = s * tps, min((s + 1) * tps, n)
        if lo >= hi:
            continue
        band = order[lo:hi].astype(np.int64)
        assert np.array_equal(np.sort(band), np.arange(lo, hi)), "%s: band %d [%d, %d) is not a permutation of its tiles" % (what, s, lo, hi)
        k = cls[band]
        assert (k[:-1] >= k[1:]).all(), "%s: band %d is not longest first" % (what, s)


def _sort(vrt):
    L = vrt.rtapi._lib()
    L.vxrt_internal_lpt_sort.restype = C.c_int
    L.vxrt_internal_lpt_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    return L.vxrt_internal_lpt_sort


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


SIZES = [(n, (n + SHARDS - 1) // SHARDS) for n in (1, 5, 7, 8, 9, 255, 256, 257, 2049, 40000)]
SIZES += [(5, 1),       # bands 5..7 are empty (lo >= hi)
          (100, 10)]    # eight bands of ten cover 80 tiles: the order of the other 20 is not the sort's to write


@gpu
@pytest.mark.parametrize("n,tps", SIZES)
def test_sort_alone(vrt, gpu_device, n, tps):
    import torch
    sort = _sort(vrt)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1000 * n + tps)
    pad, clear_dwords = 16, 300     # (300: more words than the workgroup that clears them has threads)
    for name, cost in _costs(n, rng).items():
        what = "n=%d tps=%d %s" % (n, tps, name)
        d_cost = torch.from_numpy(cost.view(np.int32)).to(gpu_device)
        d_order = torch.from_numpy(np.full(n + pad, SENTINEL, np.uint32).view(np.int32)).to(gpu_device)
        d_clear = torch.from_numpy(np.full(clear_dwords + 1, GUARD, np.uint32).view(np.int32)).to(gpu_device)
        assert sort(d_cost.data_ptr(), d_order.data_ptr(), n, tps, d_clear.data_ptr(), clear_dwords, stream) == 0
        torch.cuda.synchronize()
        assert vrt.rtapi.status(stream) == 0
        order, clear = _u32(d_order), _u32(d_clear)
        check_bands(cost, order, n, tps, what)
        assert (order[min(SHARDS * tps, n):] == SENTINEL).all(), what + ": written past the last band"
        assert (clear[:clear_dwords] == 0).all() and clear[clear_dwords] == GUARD, what + ": the words to clear"
        np.testing.assert_array_equal(_u32(d_cost), cost)
        # a null `clear` is accepted: the same order classes, nothing else touched
        d_order2 = torch.from_numpy(np.full(n + pad, SENTINEL, np.uint32).view(np.int32)).to(gpu_device)
        assert sort(d_cost.data_ptr(), d_order2.data_ptr(), n, tps, None, clear_dwords, stream) == 0
        torch.cuda.synchronize()
        order2 = _u32(d_order2)
        check_bands(cost, order2, n, tps, what + " (null clear)")
        assert (order2[min(SHARDS * tps, n):] == SENTINEL).all()


# ---- (b) what a frame context learns from real frames ----
W, H = 1920, 1080


def _read_lpt(vrt, accel, n_tiles, stream):
    L = vrt.rtapi._lib()
    L.vxrt_debug_read_lpt.restype = C.c_int
    L.vxrt_debug_read_lpt.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    cost, order = np.zeros(n_tiles, np.uint32), np.full(n_tiles, SENTINEL, np.uint32)
    cap = L.vxrt_debug_read_lpt(accel, 0, 1, cost.ctypes.data, n_tiles, order.ctypes.data, n_tiles, stream)
    assert cap >= n_tiles, "vxrt_debug_read_lpt returned %d" % cap
    return cost, order


def _tiles(y0, y1):
    n = ((W + 7) // 8) * ((y1 - y0 + 7) // 8)
    per_shard = ((n * 64 + SHARDS - 1) // SHARDS + 63) & ~63     # jobs per queue shard, as the launch computes it
    return n, per_shard >> 6


def _render(vrt, ds, y0, y1, shadow):
    import torch
    px = torch.full((H, W), 0x5A5A5A, dtype=torch.int32, device=ds.t["tri"].device)
    stream = torch.cuda.current_stream().cuda_stream
    vrt.rtapi.render(ds.accel, W, H, y0, y1, vrt.rtapi.default_shade_params(), px.data_ptr(), shadow=shadow, stream=stream)
    torch.cuda.synchronize()
    assert vrt.rtapi.status(stream) == 0
    return px


def _table_holds(vrt, ds, y0, y1, what):
    import torch
    n, tps = _tiles(y0, y1)
    cost, order = _read_lpt(vrt, ds.accel, n, torch.cuda.current_stream().cuda_stream)
    check_bands(cost, order, n, tps, what)
    assert cost.min() != cost.max(), what + ": the cost table is constant"


@gpu
def test_tables_a_context_learns_from_real_frames(vrt, gpu_device):
    import torch
    b = scenes.mirror_hall(vrt)
    ds = vrt.tracer.DeviceScene(b, gpu_device)
    try:
        assert _tiles(0, H) == (32400, 4050)
        first = _render(vrt, ds, 0, H, 0)                      # the static order; its shading launch sorts for the next frame
        _table_holds(vrt, ds, 0, H, "frame 1")
        for k in (2, 3):                                      # the learned order
            assert torch.equal(_render(vrt, ds, 0, H, 0), first), "frame %d differs from frame 1" % k
            _table_holds(vrt, ds, 0, H, "frame %d" % k)
        # the key of the table changes: shadow rays, then a row window (28,800 tiles), then back to the first request
        for y0, y1, shadow, what in ((0, H, 1, "shadow"), (40, 1000, 1, "rows 40..1000"), (0, H, 0, "the first request again")):
            fresh_ds = vrt.tracer.DeviceScene(b, gpu_device)
            try:
                fresh = _render(vrt, fresh_ds, y0, y1, shadow)
            finally:
                fresh_ds.close()
            assert not torch.equal(fresh, torch.full_like(fresh, 0x5A5A5A))
            for k in (1, 2):                                  # static order again, then the order learned under the new key
                assert torch.equal(_render(vrt, ds, y0, y1, shadow), fresh), "%s: frame %d after the change differs from a fresh scene's" % (what, k)
                _table_holds(vrt, ds, y0, y1, "%s, frame %d" % (what, k))
        assert torch.equal(fresh, first)
    finally:
        ds.close()
