"""World_size 2 over gloo: the multi-GPU host logic -- one frame split into contiguous bands cut at equal cost and received in
place on rank 0 (the default of bench.py --gpus N), by interleaved 8-row tile rows, or by equal row bands; each rank rendering its
share with no data-path collective, ONE gather per set of frames assembling the images on rank 0.

CPU tests (not marked gpu): the oracle stands in for the device kernel, so they check the split and the assembly.  The gpu-marked
test runs the same two ranks with the HIP path (vxrt_render_interleaved / vxrt_render on the one GPU of the box, shares gathered
through host memory over gloo) and compares the assembled frame with the oracle's."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sharding():
    import importlib
    sys.path.insert(0, ROOT)
    return importlib.import_module("vortex-raytracing_amd.sharding")


def test_row_bands_are_tile_aligned_and_cover_the_frame():
    sh = _sharding()
    for h in (1, 7, 8, 64, 135, 1080, 2160):
        for world in (1, 2, 3, 4, 8):
            b = sh.row_bands(h, world)
            assert len(b) == world and b[0][0] == 0 and b[-1][1] == h
            for (a0, a1), (b0, b1) in zip(b, b[1:]):
                assert a1 == b0
            assert all(y0 % 8 == 0 or y0 == h for y0, _ in b)
            rows = [y1 - y0 for y0, y1 in b]
            assert max(rows) - min(rows) < 16 or h < 8 * world   # one tile, plus a ragged last tile


def test_interleaved_tile_rows_partition_the_frame_and_reassemble():
    sh = _sharding()
    for h, w, world in ((1080, 24, 8), (1080, 24, 2), (2160, 8, 8), (1076, 16, 3), (45, 16, 4), (7, 8, 2), (64, 8, 16)):
        rows = np.concatenate([sh.interleaved_rows(h, r, world) for r in range(world)])
        assert sorted(rows.tolist()) == list(range(h))
        for r in range(world):
            assert all((y // 8) % world == r for y in sh.interleaved_rows(h, r, world))
        f = torch.arange(h * w, dtype=torch.int32).reshape(h, w)
        parts = [sh.extract_interleaved(f, h, r, world) for r in range(world)]
        assert all(p.shape == (sh.padded_share_rows(h, world), w) for p in parts)
        assert torch.equal(sh.assemble_interleaved(parts, h, w, world), f)
        # the per-frame path of bench.py: padded frame buffers, one packing step per rank, one unpacking step on rank 0 -- in both wire
        # formats (4-byte pixels as they are; 3 bytes per pixel, the top byte of 0x00RRGGBB being zero)
        for wire in ("rgba32", "rgb24"):
            igs = [sh.InterleavedGather(h, w, r, world, "cpu", slots=1, collective=False, wire=wire) for r in range(world)]
            assert igs[0].padded_height == sh.padded_share_rows(h, world) * world and igs[0].padded_height >= h
            assert igs[0].wire_bytes() == sh.padded_share_rows(h, world) * w * (4 if wire == "rgba32" else 3)
            fp = igs[0].new_frame_buffer("cpu")
            f2 = f + 0x00A50000                         # (a colour in every byte of the 24 that travel)
            fp[:h] = f2
            for r in range(world):
                igs[r].gather(fp, 0)
                if wire == "rgba32":
                    assert torch.equal(igs[r].shares[0][0], sh.extract_interleaved(f2, h, r, world))
                igs[0].recv[0][r].copy_(igs[r].shares[0])
            assert torch.equal(igs[0].assemble(0), f2)
            # sets of frames move with the same steps, and a set may be smaller than the slot (the tapered last sets of a run)
            igb = [sh.InterleavedGather(h, w, r, world, "cpu", slots=1, collective=False, batch=3, wire=wire) for r in range(world)]
            fb = igb[0].new_frame_buffer("cpu")
            for k in range(3):
                fb[k, :h] = f + 1000 * k
            for nk in (3, 2, 1):
                for r in range(world):
                    igb[r].gather(fb, 0, k=nk)
                    igb[0].recv[0][r].copy_(igb[r].shares[0])
                got = igb[0].assemble(0, nk)
                assert got.shape == (nk, h, w) and all(torch.equal(got[k], f + 1000 * k) for k in range(nk))
    assert sh.InterleavedGather(16, 8, 0, 2, "cpu").wire == "rgb24" and sh.InterleavedGather(16, 6, 0, 2, "cpu").wire == "rgba32"
    # balance: at 1080p over 8 ranks every rank gets 16 or 17 of the 135 tile rows
    n = [len(sh.interleaved_tile_rows(1080, r, 8)) for r in range(8)]
    assert max(n) - min(n) <= 1 and sum(n) == 135


def test_band_plans_cover_the_frame_and_balance_a_known_cost():
    sh = _sharding()
    for h in (8, 45, 99, 1080, 2160):
        for world in (1, 2, 3, 8):
            b = sh.equal_bands(h, world)
            assert len(b) == world + 1 and b[0] == 0 and b[-1] == h and all(x <= y for x, y in zip(b, b[1:]))
            assert all(x % 8 == 0 or x == h for x in b)
    # a cost that grows 4x over the frame (what the atrium does): equal heights are 45 % off, the planned cut within a tile row's worth
    cost = np.linspace(1.0, 4.0, 1080)
    b = sh.equal_bands(1080, 8)
    t0 = [cost[b[r]:b[r + 1]].sum() for r in range(8)]
    for _ in range(4):
        t = [cost[b[r]:b[r + 1]].sum() for r in range(8)]
        nb = sh.rebalance_bands(b, t, 1080)
        assert nb[0] == 0 and nb[-1] == 1080 and all(y - x >= 8 for x, y in zip(nb, nb[1:])) and all(x % 8 == 0 for x in nb)
        b = nb
    t = [cost[b[r]:b[r + 1]].sum() for r in range(8)]
    assert max(t0) / np.mean(t0) > 1.4 and max(t) / np.mean(t) < 1.04
    # degenerate inputs: more ranks than tile rows keeps every band non-empty where it can; a zero time leaves the plan alone
    assert sh.rebalance_bands([0, 8, 16], [1.0, 0.0], 16) == [0, 8, 16]
    assert sh.rebalance_bands([0, 8, 16, 24], [100.0, 1.0, 1.0], 24) == [0, 8, 16, 24]
    # sets of the timed steps: sizes add up, shrink towards the end, the last one is a single frame
    for k in (1, 2, 5, 20, 37, 200):
        sizes = sh.taper(k, 16, 1, 0.5)
        assert sum(sizes) == k and max(sizes) <= 16 and sizes[-1] == 1 and all(x >= y for x, y in zip(sizes, sizes[1:]))
    assert sh.taper(20) == [10, 5, 2, 2, 1]


def test_the_schedule_of_an_n_rank_run_ends_with_one_frames_bytes_per_link():
    """bench.py --sets auto: the last set is N frames (a rank's share of a frame is 1/N of it: one frame's bytes per link whatever N is),
    the steps before it go out in equal sets of at most 16; runs too short for that, and one rank, get equal sets."""
    sh = _sharding()
    assert sh.auto_sets(20, 8) == [12, 8] and sh.auto_sets(20, 4) == [16, 4] and sh.auto_sets(20, 2) == [9, 9, 2]
    assert sh.auto_sets(200, 8) == [16] * 12 + [8] and sh.auto_sets(6, 2) == [4, 2] and sh.auto_sets(16, 8) == [8, 8]
    assert sh.auto_sets(20, 1) == [10, 10] and sh.auto_sets(10, 8) == [5, 5] and sh.auto_sets(1, 4) == [1]
    for steps in range(1, 70):
        for world in (1, 2, 3, 4, 8):
            sets = sh.auto_sets(steps, world)
            assert sum(sets) == steps and min(sets) >= 1 and max(sets) <= max(16, world)
            if world > 1 and steps >= 2 * world:
                assert sets[-1] == world
                ig = sh.InterleavedGather(1080, 1920, 0, world, "cpu", slots=1, collective=False, batch=1)
                assert ig.wire_bytes(sets[-1]) == sets[-1] * sh.padded_share_rows(1080, world) * 1920 * 3      # = one padded frame's worth of rgb24


def test_band_gather_places_every_band_without_a_copy_of_the_frame():
    """BandGather without the network: rank 0's buffer IS the final image, every other rank's buffer is its band alone, and the render
    target of a rank (pointer, frame stride) addresses its buffer like a full frame."""
    sh = _sharding()
    h, w, world, k = 45, 16, 3, 2
    bounds = [0, 16, 24, 45]
    f = torch.arange(k * h * w, dtype=torch.int32).reshape(k, h, w)
    for r in range(world):
        bg = sh.BandGather(h, w, r, world, bounds, "cpu", [k], collective=False)
        ptr, stride = bg.target(0)
        assert bg.bufs[0].shape == ((k, h, w) if r == 0 else (k, bounds[r + 1] - bounds[r], w))
        # pixel (x, y) of frame j at ptr + 4 * (j * stride + x + y * w): the first pixel of the band is the buffer's first (+ y0 rows on rank 0)
        first = ptr + 4 * (bounds[r] * w)
        assert first == bg.bufs[0].data_ptr() + (4 * bounds[r] * w if r == 0 else 0)
        assert stride == (h * w if r == 0 else (bounds[r + 1] - bounds[r]) * w)


def _worker(rank, world, port, mode, use_hip, q):
    sys.path.insert(0, ROOT)
    import importlib
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    vrt = importlib.import_module("vortex-raytracing_amd")
    sh = vrt.sharding
    sc = vrt.scene.procedural("atrium", 3, 0, 3) if use_hip else vrt.scene.procedural("cornell")
    w, h = (328, 184) if use_hip else (40, 44)
    if use_hip:
        # the HIP path: this rank's share of the frame through the C ABI, into its own full-size frame buffer
        dev = "cuda:0"
        ds = vrt.tracer.DeviceScene(sc, dev)
        p = vrt.rtapi.default_shade_params()
        p.light_pos[:] = (300.0, 480.0, 60.0)
        buf = torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        if mode.startswith("tilerows"):
            vrt.rtapi.render_interleaved(ds.accel, w, h, rank, world, p, buf.data_ptr(), 1, None, None, None, s)
        else:
            y0, y1 = sh.row_bands(h, world)[rank]
            vrt.rtapi.render(ds.accel, w, h, y0, y1, p, buf.data_ptr(), 1, None, None, None, s)
        torch.cuda.synchronize()
        assert vrt.rtapi.status(s) == 0
        frame_local = buf.cpu()
    else:
        from oracle import pyoracle as po
        px, _, _ = po.render(sc, w, h)                      # stand-in for the kernel: full frame, the share is cut out below
        frame_local = torch.from_numpy(px.view(np.int32).copy())
    if mode == "tilerows":
        share = sh.extract_interleaved(frame_local, h, rank, world)
        frame = sh.gather_interleaved(share, h, w, rank, world)
    elif mode == "tilerows_batch":        # what bench.py does with several ranks: 3 frames per set of launches, one collective
        ig = sh.InterleavedGather(h, w, rank, world, "cpu", slots=1, batch=3)
        fb = ig.new_frame_buffer("cpu")
        if use_hip:
            plist = []
            for k in range(3):
                pk = vrt.rtapi.default_shade_params()
                pk.light_pos[:] = (300.0 - 50.0 * k, 480.0, 60.0 + 40.0 * k)
                plist.append(pk)
            dbuf = torch.zeros(fb.shape, dtype=torch.int32, device=dev)
            vrt.rtapi.render_interleaved_batch(ds.accel, w, h, rank, world, plist, dbuf.data_ptr(), ig.frame_stride, 1, None, s)
            torch.cuda.synchronize()
            assert vrt.rtapi.status(s) == 0
            fb.copy_(dbuf.cpu())
        else:
            for k in range(3):
                fb[k, :h] = frame_local + k
        frame = ig.gather(fb, 0)
        if frame is not None:
            frame = frame.clone()
        # a smaller set in the same slot (the tapered last sets of a run): its frames only
        part = ig.gather(fb, 0, k=2)
        if part is not None:
            assert part.shape[0] == 2 and torch.equal(part, frame[:2])
    elif mode == "bands_batch":           # bench.py's default with several ranks: unequal bands, received in place, 3 frames per set
        bounds = [0, 2 * h // 3 // 8 * 8, h]
        bg = sh.BandGather(h, w, rank, world, bounds, dev if use_hip else "cpu", [3], via_cpu=True)
        y0, y1 = bounds[rank], bounds[rank + 1]
        if use_hip:
            plist = []
            for k in range(3):
                pk = vrt.rtapi.default_shade_params()
                pk.light_pos[:] = (300.0 - 50.0 * k, 480.0, 60.0 + 40.0 * k)
                plist.append(pk)
            bg.bufs[0].fill_(0x5A5A5A5A)
            dst, stride = bg.target(0)
            vrt.rtapi.render_rows_batch(ds.accel, w, h, y0, y1, plist, dst, stride, 1, None, s)
            torch.cuda.synchronize()
            assert vrt.rtapi.status(s) == 0
            if rank == 0:      # a rank writes only its band
                assert bool((bg.bufs[0][:, y1:] == 0x5A5A5A5A).all())
        else:
            for k in range(3):
                if rank == 0:
                    bg.bufs[0][k, y0:y1] = frame_local[y0:y1] + k
                else:
                    bg.bufs[0][k] = frame_local[y0:y1] + k
        frame = bg.gather(0, 3)
        if frame is not None:
            frame = frame.clone().cpu()
    elif mode == "tilerows_prepared":     # what bench.py does per frame
        ig = sh.InterleavedGather(h, w, rank, world, "cpu", slots=1)
        fp = ig.new_frame_buffer("cpu")
        fp[:h] = frame_local
        frame = ig.gather(fp, 0)
        if frame is not None:
            frame = frame.clone()
    else:
        y0, y1 = sh.row_bands(h, world)[rank]
        frame = sh.gather_frame(frame_local[y0:y1].contiguous(), h, w, rank, world)
    if rank == 0:
        q.put(frame.numpy().view(np.uint32))
    dist.destroy_process_group()


def _run(mode, use_hip):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, mode, use_hip, q)) for r in range(2)]
    for p in procs:
        p.start()
    frame = q.get(timeout=300)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return frame


def test_two_rank_batch_assembly():
    frames = _run("tilerows_batch", False)
    sys.path.insert(0, ROOT)
    import importlib
    vrt = importlib.import_module("vortex-raytracing_amd")
    from oracle import pyoracle as po
    want, _, _ = po.render(vrt.scene.procedural("cornell"), 40, 44)
    assert frames.shape == (3, 44, 40)
    for k in range(3):
        assert np.array_equal(frames[k], (want.view(np.int32) + k).view(np.uint32))


def test_two_rank_band_assembly():
    frames = _run("bands_batch", False)
    sys.path.insert(0, ROOT)
    import importlib
    vrt = importlib.import_module("vortex-raytracing_amd")
    from oracle import pyoracle as po
    want, _, _ = po.render(vrt.scene.procedural("cornell"), 40, 44)
    assert frames.shape == (3, 44, 40)
    for k in range(3):
        assert np.array_equal(frames[k], (want.view(np.int32) + k).view(np.uint32))


@pytest.mark.gpu
def test_two_rank_band_assembly_on_the_hip_path(po):
    """Two processes share the box's GPU; each renders its band (unequal heights) of THREE frames in one set of launches
    (vxrt_render_rows_batch: rank 0 in place in the final images, rank 1 into its band alone), bands received in place over gloo."""
    frames = _run("bands_batch", True)
    sys.path.insert(0, ROOT)
    import importlib
    vrt = importlib.import_module("vortex-raytracing_amd")
    sc = vrt.scene.procedural("atrium", 3, 0, 3)
    for k in range(3):
        want, _, _, _ = po.render_ex(sc, 328, 184, po.shade_params(light_pos=(300.0 - 50.0 * k, 480.0, 60.0 + 40.0 * k)), 1)
        assert np.array_equal(frames[k], want)


@pytest.mark.gpu
def test_two_rank_batch_assembly_on_the_hip_path(po):
    """Two processes share the box's GPU; each renders its share of THREE frames (a moving light) in one set of launches, one gloo gather."""
    frames = _run("tilerows_batch", True)
    sys.path.insert(0, ROOT)
    import importlib
    vrt = importlib.import_module("vortex-raytracing_amd")
    sc = vrt.scene.procedural("atrium", 3, 0, 3)
    for k in range(3):
        want, _, _, _ = po.render_ex(sc, 328, 184, po.shade_params(light_pos=(300.0 - 50.0 * k, 480.0, 60.0 + 40.0 * k)), 1)
        assert np.array_equal(frames[k], want)


@pytest.mark.parametrize("mode", ["tilerows", "tilerows_prepared", "rows"])
def test_two_rank_frame_assembly(mode):
    frame = _run(mode, False)
    sys.path.insert(0, ROOT)
    import importlib
    vrt = importlib.import_module("vortex-raytracing_amd")
    from oracle import pyoracle as po
    want, _, _ = po.render(vrt.scene.procedural("cornell"), 40, 44)
    assert np.array_equal(frame, want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tilerows", "tilerows_prepared", "rows"])
def test_two_rank_frame_assembly_on_the_hip_path(mode, po):
    """Two processes share the box's GPU; each renders its share with the HIP kernels, gloo gathers, rank 0 assembles."""
    frame = _run(mode, True)
    sys.path.insert(0, ROOT)
    import importlib
    vrt = importlib.import_module("vortex-raytracing_amd")
    want, _, _, _ = po.render_ex(vrt.scene.procedural("atrium", 3, 0, 3), 328, 184, po.shade_params(light_pos=(300.0, 480.0, 60.0)), 1)
    assert np.array_equal(frame, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shard", ["bands", "tilerows"])
def test_bench_two_ranks_end_to_end(shard, tmp_path):
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one process per rank), here with two ranks sharing the
    box's GPU and gloo for the collectives: the band plan / the sets of frames, the assembly and the one JSON line of rank 0, with
    --full's legs (rank 0's counting build, the random rays of every rank); the frame rank 0 assembled in the last timed step
    (--dump-outputs) equals the whole frame rendered by one rank."""
    import importlib
    import json
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2", "--settle-frames", "4", "--level", "4",
           "--dist-backend", "gloo", "--full", "--no-cpu-baseline", "--random-rays", "65536", "--shard", shard, "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["rays_per_step"] > d["config"]["rays_per_step_rank0"] > 0 and d["config"]["shard"] == shard
    if shard == "bands":
        plan = d["config"]["band_plan"]
        assert plan["bounds"][0] == 0 and plan["bounds"][-1] == 1080 and len(plan["bounds"]) == 3 and plan["rounds"] >= 1
        assert d["config"]["sets_of_the_timed_steps"] == [3, 2, 1] and "bands" in d["config"]["parallelism"]
    else:
        # 6 steps on 2 ranks: a last set of 2 frames (one frame's bytes per link), the 4 steps before it as one set; 3 bytes per pixel on the wire
        assert d["config"]["sets_of_the_timed_steps"] == [4, 2] and d["config"]["frames_per_launch_group"] == 4 and "interleaved" in d["config"]["parallelism"]
        assert d["config"]["wire_format"] == "rgb24" and d["config"]["wire_bytes_per_rank_last_set"] == 2 * 544 * 1920 * 3
    assert d["extras"]["random_rays_n"] == 65536 * 2 and d["roofline"]["identity"]["rays"] == d["config"]["rays_per_step"]
    got = np.load(tmp_path / "pixels_rgb.npy")
    assert got.dtype == np.float32 and got.shape == (1080, 1920, 3)
    sys.path.insert(0, ROOT)
    vrt = importlib.import_module("vortex-raytracing_amd")
    ds = vrt.tracer.DeviceScene(vrt.scene.procedural("atrium", 4, 0, 3), "cuda:0")
    params = vrt.rtapi.default_shade_params()
    params.light_pos[:] = (300.0, 480.0, 60.0)
    px = torch.zeros((1080, 1920), dtype=torch.int32, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    vrt.rtapi.render(ds.accel, 1920, 1080, 0, 1080, params, px.data_ptr(), 1, None, None, None, st)
    assert vrt.rtapi.status(st) == 0
    p = px.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got, np.stack([(p >> 16) & 0xFF, (p >> 8) & 0xFF, p & 0xFF], axis=-1).astype(np.float32))
    assert len(np.unique(p)) > 10
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,world,nk", [(1080, 1920, 8, 3), (1076, 328, 3, 2), (45, 16, 4, 1), (2160, 3840, 8, 1)])
def test_wire_kernels_pack_and_unpack_what_the_host_path_does(h, w, world, nk):
    """vxrt_wire_pack / vxrt_wire_unpack (3 bytes per pixel on the link) against the same layout made with torch indexing on host
    tensors: every rank's wire bytes equal, and the frames rank 0 assembles equal the frames the shares were cut from."""
    sh = _sharding()
    g = torch.Generator().manual_seed(h * 31 + w)
    batch = 3
    host = [sh.InterleavedGather(h, w, r, world, "cpu", slots=1, collective=False, batch=batch, wire="rgb24") for r in range(world)]
    dev = [sh.InterleavedGather(h, w, r, world, "cuda:0", slots=1, collective=False, batch=batch, wire="rgb24") for r in range(world)]
    fb = host[0].new_frame_buffer("cpu")
    fb[:, :h] = torch.randint(0, 1 << 24, (batch, h, w), generator=g, dtype=torch.int32)      # 0x00RRGGBB
    fbd = fb.cuda()
    for r in range(world):
        host[r].gather(fb, 0, k=nk)
        dev[r].gather(fbd, 0, k=nk)
        torch.cuda.synchronize()
        assert torch.equal(dev[r].shares[0][:nk].cpu(), host[r].shares[0][:nk])
        host[0].recv[0][r].copy_(host[r].shares[0])
        dev[0].recv[0][r].copy_(dev[r].shares[0])
    want = fb[:nk, :h]
    assert torch.equal(host[0].assemble(0, nk), want)
    got = dev[0].assemble(0, nk)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)
    # the rows of the padded height that no frame has stay zero (byte 3 of every pixel too)
    assert int(dev[0].full[0].view(batch, dev[0].padded_height, w)[:nk, h:].abs().sum().item()) == 0
