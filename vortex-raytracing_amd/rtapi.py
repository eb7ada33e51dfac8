"""ctypes binding of the vxrt_* direct launch API (include/vortex_hip.h level 2): launches on
caller-owned DEVICE pointers and a caller-owned HIP stream.  Used by bench.py and the GPU tests with
torch tensors as plain device memory (`tensor.data_ptr()`), nothing torch-typed crosses the ABI."""
import ctypes as C

from .runtime import hip_lib, check

MODE_CLOSEST, MODE_ANY = 0, 1


class VxrtScene(C.Structure):
    _fields_ = [("tlas", C.c_void_p), ("blas", C.c_void_p), ("bvh", C.c_void_p), ("tri", C.c_void_p),
                ("triEx", C.c_void_p), ("mat", C.c_void_p), ("tex", C.c_void_p),
                ("n_tlas_nodes", C.c_uint32), ("n_blas", C.c_uint32), ("n_bvh_nodes", C.c_uint32),
                ("n_tris", C.c_uint32), ("n_mats", C.c_uint32), ("reserved", C.c_uint32), ("tex_bytes", C.c_uint64)]


class ShadeParams(C.Structure):
    _fields_ = [("ambient", C.c_float * 3), ("light_color", C.c_float * 3), ("light_pos", C.c_float * 3),
                ("background", C.c_float * 3), ("max_depth", C.c_uint32)]


# defaults of the reference host program (tests/regression/raytracing/main.cpp:34-41)
def default_shade_params():
    p = ShadeParams()
    p.ambient[:] = (0.4, 0.4, 0.4)
    p.light_color[:] = (1.0, 1.0, 1.0)
    p.light_pos[:] = (0.0, 10.0, -10.0)
    p.background[:] = (0.4, 0.35, 0.25)
    p.max_depth = 1
    return p


_proto = False


def _lib():
    global _proto
    L = hip_lib()
    if not _proto:
        L.vxrt_accel_build.restype = C.c_int
        L.vxrt_accel_build.argtypes = [C.POINTER(VxrtScene), C.c_void_p, C.POINTER(C.c_void_p)]
        L.vxrt_accel_destroy.restype = C.c_int
        L.vxrt_accel_destroy.argtypes = [C.c_void_p]
        L.vxrt_accel_bytes.restype = C.c_uint64
        L.vxrt_accel_bytes.argtypes = [C.c_void_p]
        L.vxrt_accel_frames_in_flight.restype = C.c_int
        L.vxrt_accel_frames_in_flight.argtypes = [C.c_void_p, C.c_uint32]
        L.vxrt_render.restype = C.c_int
        L.vxrt_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.POINTER(ShadeParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vxrt_render_stats.restype = C.c_int
        L.vxrt_render_ao.restype = C.c_int
        L.vxrt_render_ao.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams),
                                     C.POINTER(AoParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vxrt_render_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(ShadeParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vxrt_trace.restype = C.c_int
        L.vxrt_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.vxrt_status.restype = C.c_int
        L.vxrt_status.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.vxrt_version.restype = C.c_char_p
        _declare_path_family(L)
        _proto = True
    return L


# (the families below once declared their own prototypes; theirs are _lib()'s now, the names stay for callers of the raw library)
_denoise_lib = _temporal_lib = _motion_lib = _variance_lib = _lib


def accel_build(scene, stream=None):
    """Build the device-side acceleration layout for a VxrtScene; returns the opaque handle."""
    h = C.c_void_p()
    check(_lib().vxrt_accel_build(C.byref(scene), stream, C.byref(h)), "vxrt_accel_build")
    return h


class BvhInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("max_leaf", C.c_uint32), ("max_depth", C.c_uint32),
                ("bounds", C.c_float * 6)]


class BvhTooDeep(RuntimeError):
    """vxrt_bvh_build: the Morton-order tree is deeper than the 32 levels the reference's trail supports."""


def bvh_build(tri_ptr, triEx_ptr, n_tris, nodes_ptr, node_capacity, tri_offset=0, leaf_max=0, stream=None):
    """vxrt_bvh_build: BLAS of one mesh on the GPU, in the reference's node format; tri / triEx are reordered in place."""
    L = _lib()
    L.vxrt_bvh_build.restype = C.c_int
    L.vxrt_bvh_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(BvhInfo), C.c_void_p]
    info = BvhInfo()
    rc = L.vxrt_bvh_build(tri_ptr, triEx_ptr, n_tris, tri_offset, leaf_max, nodes_ptr, node_capacity, C.byref(info), stream)
    if rc == -2:
        raise BvhTooDeep("vxrt_bvh_build: tree depth %d exceeds the reference's 32 levels" % info.max_depth)
    check(rc, "vxrt_bvh_build")
    return info


def tlas_build(boxes_ptr, n_instances, nodes_ptr, node_capacity, stream=None):
    """vxrt_tlas_build: TLAS over n_instances world-space boxes (device, 6 floats each), in the reference's node format."""
    L = _lib()
    L.vxrt_tlas_build.restype = C.c_int
    L.vxrt_tlas_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(BvhInfo), C.c_void_p]
    info = BvhInfo()
    rc = L.vxrt_tlas_build(boxes_ptr, n_instances, nodes_ptr, node_capacity, C.byref(info), stream)
    if rc == -2:
        raise BvhTooDeep("vxrt_tlas_build: tree depth %d exceeds the reference's 32 levels" % info.max_depth)
    check(rc, "vxrt_tlas_build")
    return info


def release_scratch():
    """vxrt_bvh_release_scratch: return the builders' grow-only scratch allocation to the device (the next build allocates again)."""
    L = _lib()
    L.vxrt_bvh_release_scratch.restype = None
    L.vxrt_bvh_release_scratch.argtypes = []
    L.vxrt_bvh_release_scratch()


REFIT_INSTANCES, REFIT_GEOMETRY = 1, 2   # VXRT_REFIT_*


def accel_refit(accel, what, stream=None):
    """vxrt_accel_refit: new boxes for moved instances (REFIT_INSTANCES) or moved vertices (REFIT_GEOMETRY), topology kept; raises on
    failure (the accel is then stale until a refit succeeds)."""
    L = _lib()
    L.vxrt_accel_refit.restype = C.c_int
    L.vxrt_accel_refit.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    check(L.vxrt_accel_refit(accel, int(what), stream), "vxrt_accel_refit")


def accel_set_transforms(accel, first, count, ptr, stream=None):
    """vxrt_accel_set_transforms: `count` object-to-world matrices (device, 16 floats each, row-major) into instance records
    first.. (transform + MESA inverse), then the instance refit; raises on failure (a refused matrix leaves every record as it was)."""
    L = _lib()
    L.vxrt_accel_set_transforms.restype = C.c_int
    L.vxrt_accel_set_transforms.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    check(L.vxrt_accel_set_transforms(accel, int(first), int(count), ptr, stream), "vxrt_accel_set_transforms")


def accel_set_alpha_test(accel, thresholds, stream=None):
    """vxrt_accel_set_alpha_test: one threshold byte per material (0 = opaque; T in 1..255 rejects candidates whose texel's top byte is
    below T); None switches the test off.  Raises on a refusal (nothing is changed then)."""
    L = _lib()
    L.vxrt_accel_set_alpha_test.restype = C.c_int
    L.vxrt_accel_set_alpha_test.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    if thresholds is None:
        check(L.vxrt_accel_set_alpha_test(accel, None, 0, stream), "vxrt_accel_set_alpha_test")
        return
    t = [int(v) for v in thresholds]
    if any(v < 0 or v > 255 for v in t):
        raise ValueError("alpha thresholds are bytes")
    buf = (C.c_uint8 * max(len(t), 1))(*t)
    check(L.vxrt_accel_set_alpha_test(accel, buf, len(t), stream), "vxrt_accel_set_alpha_test")


def accel_destroy(accel):
    if accel:
        check(_lib().vxrt_accel_destroy(accel), "vxrt_accel_destroy")


def accel_frames_in_flight(accel, n):
    """vxrt_accel_frames_in_flight: frames this accel keeps in flight (1..8); raises on a bad count."""
    if _lib().vxrt_accel_frames_in_flight(accel, int(n)) != 0:
        raise RuntimeError("vxrt_accel_frames_in_flight(%r) failed" % (n,))


def trace_reference_quirks(image_ptr, image_size, offsets, rays_ptr, n, hits_ptr, mode=MODE_CLOSEST, tmax_ptr=None, stream=None):
    """vxrt_trace_reference_quirks: the RTU's traversal restated literally (stale base_ptr included) on a flat memory image;
    offsets = (tlas, blas, bvh, tri) byte offsets into the image, i.e. the values of the RTX DCRs 0x6..0x9."""
    L = _lib()
    L.vxrt_trace_reference_quirks.restype = C.c_int
    L.vxrt_trace_reference_quirks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    check(L.vxrt_trace_reference_quirks(image_ptr, image_size, offsets[0], offsets[1], offsets[2], offsets[3], rays_ptr, n, tmax_ptr, hits_ptr, mode, stream),
          "vxrt_trace_reference_quirks")


def debug_read_control(accel, ctx=0, n_dwords=800, stream=None):
    """vxrt_debug_read_control: the control block of frame context `ctx` (numpy u32) as the last call left it."""
    import numpy as np
    L = _lib()
    L.vxrt_debug_read_control.restype = C.c_int
    L.vxrt_debug_read_control.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(n_dwords, np.uint32)
    check(L.vxrt_debug_read_control(accel, ctx, out.ctypes.data, n_dwords, stream), "vxrt_debug_read_control")
    return out


def debug_set_shadow_hints(accel, hints, stream=None):
    """vxrt_debug_set_shadow_hints: overwrite the first len(hints) hint words (numpy u32, tile-major like the hit records) of the frame
    context `stream` rendered a hinted shadow frame on last."""
    import numpy as np
    L = _lib()
    L.vxrt_debug_set_shadow_hints.restype = C.c_int
    L.vxrt_debug_set_shadow_hints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    h = np.ascontiguousarray(hints, dtype=np.uint32)
    check(L.vxrt_debug_set_shadow_hints(accel, stream, h.ctypes.data, h.size), "vxrt_debug_set_shadow_hints")


def debug_get_shadow_hints(accel, n, stream=None):
    """vxrt_debug_get_shadow_hints: the first n hint words of that context (numpy u32; 0xFFFFFFFF = no hint)."""
    import numpy as np
    L = _lib()
    L.vxrt_debug_get_shadow_hints.restype = C.c_int
    L.vxrt_debug_get_shadow_hints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    out = np.zeros(int(n), np.uint32)
    check(L.vxrt_debug_get_shadow_hints(accel, stream, out.ctypes.data, out.size), "vxrt_debug_get_shadow_hints")
    return out


def debug_read_path_table(accel, n, stream=None):
    """vxrt_debug_read_path_table: the path codes of triangles 0 .. n - 1 (numpy u32)."""
    import numpy as np
    L = _lib()
    L.vxrt_debug_read_path_table.restype = C.c_int
    L.vxrt_debug_read_path_table.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    out = np.zeros(int(n), np.uint32)
    check(L.vxrt_debug_read_path_table(accel, out.ctypes.data, out.size, stream), "vxrt_debug_read_path_table")
    return out


def debug_shadow_hints_enable(on):
    """vxrt_debug_shadow_hints_enable: 0 = frames without shadow hints, 1 = with, -1 = as VXRT_SHADOW_HINTS says (process-wide)."""
    L = _lib()
    L.vxrt_debug_shadow_hints_enable.restype = C.c_int
    L.vxrt_debug_shadow_hints_enable.argtypes = [C.c_int]
    check(L.vxrt_debug_shadow_hints_enable(int(on)), "vxrt_debug_shadow_hints_enable")


def debug_shadow_hint_counts(reset=False, stream=None):
    """vxrt_debug_shadow_hint_counts: (blocked occlusion rays of hinted frames, those blocked while still guided) since the last
    reset, or None if the library was built without -DRT_SHADOW_HINT_COUNT=1."""
    L = _lib()
    L.vxrt_debug_shadow_hint_counts.restype = C.c_int
    L.vxrt_debug_shadow_hint_counts.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out = (C.c_ulonglong * 2)()
    if L.vxrt_debug_shadow_hint_counts(out, int(bool(reset)), stream) != 0:
        return None
    return int(out[0]), int(out[1])


def debug_phase_counts(reset=False, stream=None):
    """vxrt_debug_phase_counts: (passes through the occlusion-only form, the general form with no any-hit lane, the general form holding
    both kinds of ray; node-body runs inside them, same classes) of the shadow frame kernels with the occlusion-only loop since the last
    reset, or None if the library was built without -DRT_PHASE_COUNT=1."""
    L = _lib()
    L.vxrt_debug_phase_counts.restype = C.c_int
    L.vxrt_debug_phase_counts.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out = (C.c_ulonglong * 6)()
    if L.vxrt_debug_phase_counts(out, int(bool(reset)), stream) != 0:
        return None
    return tuple(int(v) for v in out)


END_LOG_WAVES = 8192   # wavefronts a vxrt_debug_end_log buffer holds: 2 u64 each


def debug_end_log(accel, log_ptr):
    """vxrt_debug_end_log: the main launches enqueued on `accel` from now on leave one entry per wavefront in the device buffer
    `log_ptr` (2 x END_LOG_WAVES u64, zeroed by the caller: [0] the 100 MHz clock at the wavefront's end, [1] rays it started |
    physical XCD << 56), indexed by workgroup x 4 + wavefront; None switches the log off."""
    L = _lib()
    L.vxrt_debug_end_log.restype = C.c_int
    L.vxrt_debug_end_log.argtypes = [C.c_void_p, C.c_void_p]
    check(L.vxrt_debug_end_log(accel, log_ptr), "vxrt_debug_end_log")


def accel_bytes(accel):
    return int(_lib().vxrt_accel_bytes(accel))


def render(accel, width, height, y0, y1, params, dst_ptr, shadow=0, hits_ptr=None, colors_ptr=None, rays_ptr=None, stream=None):
    check(_lib().vxrt_render(accel, width, height, y0, y1, C.byref(params), int(shadow), dst_ptr, hits_ptr,
                             colors_ptr, rays_ptr, stream), "vxrt_render")


def render_interleaved(accel, width, height, phase, stride, params, dst_ptr, shadow=0, hits_ptr=None, colors_ptr=None, rays_ptr=None, stream=None):
    """vxrt_render_interleaved: the tile rows phase, phase + stride, ... of the frame (one rank's share of a frame split over GPUs)."""
    L = _lib()
    L.vxrt_render_interleaved.restype = C.c_int
    L.vxrt_render_interleaved.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams), C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.vxrt_render_interleaved(accel, width, height, int(phase), int(stride), C.byref(params), int(shadow), dst_ptr, hits_ptr,
                                    colors_ptr, rays_ptr, stream), "vxrt_render_interleaved")


def trace_stats(accel, rays_ptr, n, hits_ptr, mode=0, tmax_ptr=None, stream=None):
    """vxrt_trace_stats: counting build of the ray-buffer traversal; returns counts and SURVEY s8d bytes per ray
    (24 B ray read + 52 B per node / instance record + 36 B per triangle + 24 B hit record written)."""
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda:%d" % torch.cuda.current_device())
    L = _lib()
    L.vxrt_trace_stats.restype = C.c_int
    L.vxrt_trace_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    check(L.vxrt_trace_stats(accel, rays_ptr, n, tmax_ptr, hits_ptr, mode, cnt.data_ptr(), stream), "vxrt_trace_stats")
    torch.cuda.synchronize()
    r, nn, ni, nt = (int(v) for v in cnt.tolist()[:4])
    total = 24 * r + 52 * (nn + ni) + 36 * nt + 24 * r
    return {"rays": r, "node_fetches": nn, "inst_fetches": ni, "tri_fetches": nt, "bytes": total, "bytes_per_ray": total / max(r, 1)}


class RcScene(C.Structure):    # vxrc_scene_t
    _fields_ = [(k, C.c_void_p) for k in ("tlas", "blas", "bvh", "tri", "triEx", "triIdx", "tex")] + \
               [(k, C.c_uint32) for k in ("n_tlas_nodes", "n_blas", "n_bvh_nodes", "n_tris", "n_tri_idx", "tlas_root")] + \
               [("tex_bytes", C.c_uint64)]


class RcParams(C.Structure):   # vxrc_params_t
    _fields_ = [("camera_pos", C.c_float * 3), ("camera_forward", C.c_float * 3), ("camera_right", C.c_float * 3),
                ("camera_up", C.c_float * 3), ("viewplane", C.c_float * 2),
                ("samples_per_pixel", C.c_uint32), ("max_depth", C.c_uint32),
                ("light_pos", C.c_float * 3), ("light_color", C.c_float * 3), ("ambient_color", C.c_float * 3),
                ("background_color", C.c_float * 3)]


def rc_params(cam14, light12, spp=1, max_depth=1):
    p = RcParams()
    c = [float(v) for v in cam14]
    p.camera_pos[:] = c[0:3]; p.camera_forward[:] = c[3:6]; p.camera_right[:] = c[6:9]; p.camera_up[:] = c[9:12]; p.viewplane[:] = c[12:14]
    l = [float(v) for v in light12]
    p.light_pos[:] = l[0:3]; p.light_color[:] = l[3:6]; p.ambient_color[:] = l[6:9]; p.background_color[:] = l[9:12]
    p.samples_per_pixel, p.max_depth = int(spp), int(max_depth)
    return p


def rc_render(scene, width, height, y0, y1, params, dst_ptr, colors_ptr=None, stream=None):
    """vxrc_render: the software twin (tests/regression/raycast) on device buffers described by an RcScene."""
    L = _lib()
    L.vxrc_render.restype = C.c_int
    L.vxrc_render.argtypes = [C.POINTER(RcScene), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RcParams),
                              C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.vxrc_render(C.byref(scene), width, height, y0, y1, C.byref(params), dst_ptr, colors_ptr, stream), "vxrc_render")


def rc_accel_build(scene, stream=None):
    """vxrc_accel_build: the twin's acceleration layout for an RcScene; returns the opaque handle."""
    L = _lib()
    L.vxrc_accel_build.restype = C.c_int
    L.vxrc_accel_build.argtypes = [C.POINTER(RcScene), C.c_void_p, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    check(L.vxrc_accel_build(C.byref(scene), stream, C.byref(h)), "vxrc_accel_build")
    return h


def wire_pack(frames_ptr, frame_stride, width, tile_rows_per_rank, world, rank, n_frames, wire_ptr, stream=None):
    """vxrt_wire_pack: this rank's interleaved tile rows of n_frames frames as 3 bytes per pixel."""
    L = _lib()
    L.vxrt_wire_pack.restype = C.c_int
    L.vxrt_wire_pack.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    check(L.vxrt_wire_pack(frames_ptr, frame_stride, width, tile_rows_per_rank, world, rank, n_frames, wire_ptr, stream), "vxrt_wire_pack")


def wire_unpack(wire_all_ptr, wire_stride_bytes, width, tile_rows_per_rank, world, n_frames, frames_ptr, frame_stride, stream=None):
    """vxrt_wire_unpack: the `world` shares expanded and interleaved into n_frames frames of padded height."""
    L = _lib()
    L.vxrt_wire_unpack.restype = C.c_int
    L.vxrt_wire_unpack.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    check(L.vxrt_wire_unpack(wire_all_ptr, wire_stride_bytes, width, tile_rows_per_rank, world, n_frames, frames_ptr, frame_stride, stream), "vxrt_wire_unpack")


def accel_info(accel, which):
    """vxrt_accel_info: 0 -> internal levels of the deepest path (counted up to 17), 1 -> 48-entry stacks (depth class <= 16),
    2 -> single identity instance under the TLAS root, 3 -> ldexp decode, 4 -> a non-zero alpha table is set, 7 -> emitters of a
    valid emitter table (0: none, or stale), 8 -> entries of the emitter index (0: none built since the last set_emitters),
    9 -> the accel holds a path table (shadow hints)."""
    L = _lib()
    L.vxrt_accel_info.restype = C.c_int
    L.vxrt_accel_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    v = C.c_uint64()
    check(L.vxrt_accel_info(accel, which, C.byref(v)), "vxrt_accel_info")
    return int(v.value)


def rc_accel_info(accel, which):
    """vxrc_accel_info: 0 -> the walk takes two levels per fetch (wide nodes), 1 -> internal levels of the deepest tree."""
    L = _lib()
    L.vxrc_accel_info.restype = C.c_int
    L.vxrc_accel_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    v = C.c_uint64()
    check(L.vxrc_accel_info(accel, which, C.byref(v)), "vxrc_accel_info")
    return int(v.value)


def rc_accel_destroy(accel):
    if accel:
        L = _lib()
        L.vxrc_accel_destroy.restype = C.c_int
        L.vxrc_accel_destroy.argtypes = [C.c_void_p]
        check(L.vxrc_accel_destroy(accel), "vxrc_accel_destroy")


def rc_render_accel(accel, width, height, y0, y1, params, dst_ptr, colors_ptr=None, stream=None):
    """vxrc_render_accel: the software twin on a prebuilt layout."""
    L = _lib()
    L.vxrc_render_accel.restype = C.c_int
    L.vxrc_render_accel.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RcParams), C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.vxrc_render_accel(accel, width, height, y0, y1, C.byref(params), dst_ptr, colors_ptr, stream), "vxrc_render_accel")


class AoParams(C.Structure):   # vxrt_ao_params_t
    _fields_ = [("spp", C.c_uint32), ("radius", C.c_float), ("seed", C.c_uint32), ("reserved", C.c_uint32)]


def render_ao(accel, width, height, y0, y1, params, spp, radius, dst_ptr, seed=0, colors_ptr=None, unoccluded_ptr=None,
              rays_ptr=None, stream=None):
    """vxrt_render_ao: primary hit -> Lambert colour x fraction of `spp` occlusion rays (tmax = radius) that reach nothing."""
    ao = AoParams(int(spp), float(radius), int(seed), 0)
    check(_lib().vxrt_render_ao(accel, width, height, y0, y1, C.byref(params), C.byref(ao), dst_ptr, colors_ptr,
                                unoccluded_ptr, rays_ptr, stream), "vxrt_render_ao")


def render_diffuse_bounce(accel, width, height, y0, y1, params, dst_ptr, seed=0, colors_ptr=None, rays_ptr=None, stream=None):
    """vxrt_render_diffuse_bounce: primary hit + one cosine-weighted closest-hit bounce."""
    L = _lib()
    L.vxrt_render_diffuse_bounce.restype = C.c_int
    L.vxrt_render_diffuse_bounce.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams), C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.vxrt_render_diffuse_bounce(accel, width, height, y0, y1, C.byref(params), int(seed), dst_ptr, colors_ptr, rays_ptr, stream),
          "vxrt_render_diffuse_bounce")


STAT_KEYS = ("rays", "node_fetches", "inst_fetches", "tri_fetches", "shaded_hits", "textured_hits", "pixels")


def algorithmic_bytes(c):
    """SURVEY.md s8d per-ray formula summed over one launch of the render kernel: 52 B per node and
    per instance record fetched, 36 B per triangle tested, 64 B triEx + 88 B material (+4 B texel)
    per shaded hit, 4 B per pixel written.  Rays are generated in registers and hit records stay in
    registers, so the formula's 24 B ray read / 24 B hit write do not apply to this kernel."""
    return (52 * (c["node_fetches"] + c["inst_fetches"]) + 36 * c["tri_fetches"]
            + (64 + 88) * c["shaded_hits"] + 4 * c["textured_hits"] + 4 * c["pixels"])


def render_interleaved_batch(accel, width, height, phase, stride, params_list, dst_ptr, dst_frame_stride, shadow=0, rays_ptr=None, stream=None):
    """vxrt_render_interleaved_batch: len(params_list) frames of this share in one set of launches; frame f -> dst + f * dst_frame_stride pixels."""
    L = _lib()
    L.vxrt_render_interleaved_batch.restype = C.c_int
    L.vxrt_render_interleaved_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams), C.c_int,
                                                C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    arr = (ShadeParams * len(params_list))(*params_list)
    check(L.vxrt_render_interleaved_batch(accel, width, height, phase, stride, len(params_list), arr, int(shadow), dst_ptr, dst_frame_stride, rays_ptr, stream),
          "vxrt_render_interleaved_batch")


def render_rows_batch(accel, width, height, y0, y1, params_list, dst_ptr, dst_frame_stride, shadow=0, rays_ptr=None, stream=None):
    """vxrt_render_rows_batch: len(params_list) frames of the row band [y0, y1) in one set of launches.  dst_ptr addresses a full
    frame (pixel (x, y) of frame f at dst + f * dst_frame_stride + x + y * width, in pixels): a caller that keeps only its band
    passes band_ptr - 4 * y0 * width and a frame stride of (y1 - y0) * width."""
    L = _lib()
    L.vxrt_render_rows_batch.restype = C.c_int
    L.vxrt_render_rows_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams), C.c_int,
                                         C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    arr = (ShadeParams * len(params_list))(*params_list)
    check(L.vxrt_render_rows_batch(accel, width, height, y0, y1, len(params_list), arr, int(shadow), dst_ptr, dst_frame_stride, rays_ptr, stream),
          "vxrt_render_rows_batch")


def render_batch(accel, width, height, params_list, dst_ptr, dst_frame_stride, shadow=0, rays_ptr=None, stream=None):
    """vxrt_render_batch: len(params_list) whole frames in one set of launches; frame f -> dst + f * dst_frame_stride pixels."""
    L = _lib()
    L.vxrt_render_batch.restype = C.c_int
    L.vxrt_render_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams), C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    arr = (ShadeParams * len(params_list))(*params_list)
    check(L.vxrt_render_batch(accel, width, height, len(params_list), arr, int(shadow), dst_ptr, dst_frame_stride, rays_ptr, stream), "vxrt_render_batch")


def render_stats(accel, width, height, y0, y1, params, dst_ptr, shadow=0, stream=None, timed=False):
    """Runs the counting build of the render kernels once; returns the counters + algorithmic bytes.  timed=True counts the
    traversal the timed kernel performs (unordered occlusion rays, leaf helpers) instead of the reference-order one."""
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda:%d" % torch.cuda.current_device())
    L = _lib()
    fn = L.vxrt_render_stats_timed if timed else L.vxrt_render_stats
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    check(fn(accel, width, height, y0, y1, C.byref(params), int(shadow), dst_ptr, cnt.data_ptr(), stream), "vxrt_render_stats")
    torch.cuda.synchronize()
    c = dict(zip(STAT_KEYS, [int(v) for v in cnt[:7].tolist()]))
    c["bytes"] = algorithmic_bytes(c)
    return c


def trace(accel, rays_ptr, n, hits_ptr, mode=MODE_CLOSEST, tmax_ptr=None, stream=None):
    check(_lib().vxrt_trace(accel, rays_ptr, n, tmax_ptr, hits_ptr, mode, stream), "vxrt_trace")


def shade_rays(accel, rays_ptr, hits_ptr, n, params, colors_ptr=None, rgb8_ptr=None, stream=None):
    """vxrt_shade_rays: closest-hit / miss shader over (ray, hit record) pairs."""
    L = _lib()
    L.vxrt_shade_rays.restype = C.c_int
    L.vxrt_shade_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ShadeParams), C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.vxrt_shade_rays(accel, rays_ptr, hits_ptr, n, C.byref(params), colors_ptr, rgb8_ptr, stream), "vxrt_shade_rays")


def status(stream=None):
    st = C.c_uint32()
    check(_lib().vxrt_status(stream, C.byref(st)), "vxrt_status")
    return st.value


def version():
    return _lib().vxrt_version().decode()


class Camera(C.Structure):    # vxrt_camera_t: the 14 floats of kernel_arg_t camera_pos .. viewplane
    _fields_ = [("pos", C.c_float * 3), ("forward", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("viewplane", C.c_float * 2)]

    @classmethod
    def from_cam14(cls, cam14):
        c = cls()
        v = [float(x) for x in cam14]
        if len(v) != 14:
            raise ValueError("a camera is 14 floats (pos, forward, right, up, viewplane)")
        c.pos[:] = v[0:3]; c.forward[:] = v[3:6]; c.right[:] = v[6:9]; c.up[:] = v[9:12]; c.viewplane[:] = v[12:14]
        return c

    def cam14(self):
        return list(self.pos) + list(self.forward) + list(self.right) + list(self.up) + list(self.viewplane)


def _camera(cam):
    return cam if isinstance(cam, Camera) else Camera.from_cam14(cam)


def _camera_ref(cam):
    """the `cam` argument of the calls that take the fixed camera as None"""
    return None if cam is None else C.byref(_camera(cam))


def look_at(eye, target, up, vfov_deg, width, height):
    """The camera tracer.cpp:184-202 sets up, in fp32: forward = normalize(target - eye), right = normalize(cross(forward, up)),
    up' = cross(right, forward), viewplane = (h * W / H, h) with h = 2 tan(vfov_deg * 0.5).  As in the reference, normalize multiplies
    by 1 / sqrtf(dot), and the viewplane uses the vfov number as radians: tracer.cpp:198 applies tan() to the degree value it was
    given (its framing distance converts degrees to radians, its viewplane does not).  Returns a Camera."""
    import numpy as np
    f32 = np.float32
    e, t, u = (np.asarray(v, np.float32) for v in (eye, target, up))

    def normalize(v):
        inv = f32(1.0) / np.sqrt(f32(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
        return (v * inv).astype(np.float32)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float32)

    fwd = normalize((t - e).astype(np.float32))
    right = normalize(cross(fwd, u))
    up2 = cross(right, fwd)
    aspect = f32(width) / f32(height)
    vh = f32(2.0) * np.tan(f32(vfov_deg) * f32(0.5))
    vw = f32(vh * aspect)
    return Camera.from_cam14(list(e) + list(fwd) + list(right) + list(up2) + [vw, vh])


def render_camera(accel, cam, width, height, y0, y1, params, dst_ptr, shadow=0, hits_ptr=None, colors_ptr=None, rays_ptr=None, stream=None):
    """vxrt_render_camera: vxrt_render seen from pinhole camera `cam` (a Camera or 14 floats)."""
    L = _lib()
    L.vxrt_render_camera.restype = C.c_int
    L.vxrt_render_camera.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams), C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.vxrt_render_camera(accel, C.byref(_camera(cam)), width, height, y0, y1, C.byref(params), int(shadow), dst_ptr, hits_ptr,
                               colors_ptr, rays_ptr, stream), "vxrt_render_camera")


def render_batch_camera(accel, width, height, cams, params_list, dst_ptr, dst_frame_stride, shadow=0, rays_ptr=None, stream=None):
    """vxrt_render_batch_camera: frame f seen from cams[f] and shaded with params_list[f], written to dst + f * dst_frame_stride pixels."""
    if len(cams) != len(params_list):
        raise ValueError("one camera per frame")
    L = _lib()
    L.vxrt_render_batch_camera.restype = C.c_int
    L.vxrt_render_batch_camera.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Camera), C.POINTER(ShadeParams), C.c_int,
                                           C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    carr = (Camera * len(cams))(*[_camera(c) for c in cams])
    parr = (ShadeParams * len(params_list))(*params_list)
    check(L.vxrt_render_batch_camera(accel, width, height, len(params_list), carr, parr, int(shadow), dst_ptr, dst_frame_stride, rays_ptr, stream),
          "vxrt_render_batch_camera")


def pinhole_rays(cam, width, height, y0, y1, rays_ptr, stream=None):
    """vxrt_pinhole_rays: the rays of rows [y0, y1) of pinhole camera `cam`, 6 floats each, pixel (x, y) at x + (y - y0) * width."""
    L = _lib()
    L.vxrt_pinhole_rays.restype = C.c_int
    L.vxrt_pinhole_rays.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    check(L.vxrt_pinhole_rays(C.byref(_camera(cam)), width, height, y0, y1, rays_ptr, stream), "vxrt_pinhole_rays")


def render_ao_camera(accel, cam, width, height, y0, y1, params, spp, radius, dst_ptr, seed=0, colors_ptr=None, unoccluded_ptr=None,
                     rays_ptr=None, stream=None):
    """vxrt_render_ao_camera: vxrt_render_ao seen from pinhole camera `cam` (a Camera or 14 floats)."""
    L = _lib()
    L.vxrt_render_ao_camera.restype = C.c_int
    L.vxrt_render_ao_camera.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ShadeParams),
                                        C.POINTER(AoParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ao = AoParams(int(spp), float(radius), int(seed), 0)
    check(L.vxrt_render_ao_camera(accel, C.byref(_camera(cam)), width, height, y0, y1, C.byref(params), C.byref(ao), dst_ptr, colors_ptr,
                                  unoccluded_ptr, rays_ptr, stream), "vxrt_render_ao_camera")


def render_diffuse_bounce_camera(accel, cam, width, height, y0, y1, params, dst_ptr, seed=0, colors_ptr=None, rays_ptr=None, stream=None):
    """vxrt_render_diffuse_bounce_camera: vxrt_render_diffuse_bounce seen from pinhole camera `cam` (a Camera or 14 floats)."""
    L = _lib()
    L.vxrt_render_diffuse_bounce_camera.restype = C.c_int
    L.vxrt_render_diffuse_bounce_camera.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.POINTER(ShadeParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.vxrt_render_diffuse_bounce_camera(accel, C.byref(_camera(cam)), width, height, y0, y1, C.byref(params), int(seed), dst_ptr,
                                              colors_ptr, rays_ptr, stream), "vxrt_render_diffuse_bounce_camera")


PATH_MAX_BOUNCES = 16   # VXRT_PATH_MAX_BOUNCES


class PathParams(C.Structure):   # vxrt_path_params_t
    _fields_ = [("spp", C.c_uint32), ("bounces", C.c_uint32), ("seed", C.c_uint32), ("shadow", C.c_uint32)]


def _path_params(spp, bounces, seed, shadow):
    """the PathParams of the render_path* calls' arguments (the seed modulo 2^32)"""
    return PathParams(int(spp), int(bounces), int(seed) & 0xFFFFFFFF, int(shadow))


def render_path(accel, cam, width, height, y0, y1, params, spp, bounces, dst_ptr, seed=0, shadow=0, colors_ptr=None, rays_ptr=None, stream=None):
    """vxrt_render_path: `spp` paths per pixel of `bounces` diffuse bounces each, the light sampled at every vertex with shadow=1, seen
    from pinhole camera `cam` (a Camera or 14 floats; None = the fixed camera of vxrt_render)."""
    L = _lib()
    pp = _path_params(spp, bounces, seed, shadow)
    check(L.vxrt_render_path(accel, _camera_ref(cam), width, height, y0, y1, C.byref(params), C.byref(pp), dst_ptr,
                             colors_ptr, rays_ptr, stream), "vxrt_render_path")


DENOISE_MAX_ITERATIONS = 6   # VXRT_DENOISE_MAX_ITERATIONS


class DenoiseParams(C.Structure):   # vxrt_denoise_params_t
    _fields_ = [("iterations", C.c_uint32), ("normal_power", C.c_uint32), ("sigma_z", C.c_float), ("sigma_l", C.c_float)]


class PathAov(C.Structure):   # vxrt_path_aov_t: device pointers, any of them None
    _fields_ = [("noisy", C.c_void_p), ("direct", C.c_void_p), ("albedo", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p)]


def render_path_denoised(accel, cam, width, height, y0, y1, params, spp, bounces, denoise, dst_ptr, seed=0, shadow=0, colors_ptr=None, aov=None,
                         rays_ptr=None, stream=None):
    """vxrt_render_path_denoised: render_path whose demodulated indirect term goes through `denoise.iterations` passes of the guided a-trous
    filter (`denoise`: a DenoiseParams); `aov` (a PathAov of device pointers, optional) receives the guide buffers of the primary hit."""
    L = _denoise_lib()
    pp = _path_params(spp, bounces, seed, shadow)
    check(L.vxrt_render_path_denoised(accel, _camera_ref(cam), width, height, y0, y1, C.byref(params), C.byref(pp),
                                      C.byref(denoise), dst_ptr, colors_ptr, None if aov is None else C.byref(aov), rays_ptr, stream),
          "vxrt_render_path_denoised")


def denoise_scratch_bytes(width, rows):
    return int(_denoise_lib().vxrt_denoise_scratch_bytes(width, rows))


def denoise(width, rows, signal_ptr, position_ptr, normal_ptr, denoise, out_ptr, scratch_ptr, scratch_bytes, stream=None):
    """vxrt_denoise: the a-trous filter alone over a window of rows x width pixels (signal / out: 3 floats per pixel; position / normal: 4)."""
    check(_denoise_lib().vxrt_denoise(width, rows, signal_ptr, position_ptr, normal_ptr, C.byref(denoise), out_ptr, scratch_ptr, scratch_bytes, stream),
          "vxrt_denoise")


TEMPORAL_MAX_LEN = 1024   # VXRT_TEMPORAL_MAX_LEN


class TemporalParams(C.Structure):   # vxrt_temporal_params_t
    _fields_ = [("alpha_min", C.c_float), ("max_len", C.c_uint32), ("sigma_z", C.c_float), ("normal_min", C.c_float)]


class History:
    """vxrt_history_t: the accumulated signal of the previous frame of one window, for windows of up to width * rows pixels (96 bytes per
    pixel of device memory).  A context manager; `handle` is what the C calls take.  Calls on one history are the caller's to order.
    moments=True: the history also holds the luminance moments of every pixel (112 bytes per pixel) and is the kind the variance-guided
    calls take -- and the only kind: the two do not mix."""

    def __init__(self, width, rows, moments=False):
        h = C.c_void_p()
        if moments:
            check(_variance_lib().vxrt_history_create_moments(int(width), int(rows), C.byref(h)), "vxrt_history_create_moments")
        else:
            check(_temporal_lib().vxrt_history_create(int(width), int(rows), C.byref(h)), "vxrt_history_create")
        self.handle = h
        self.moments = bool(moments)

    def close(self):
        if self.handle:
            check(_temporal_lib().vxrt_history_destroy(self.handle), "vxrt_history_destroy")
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def reset(self):
        """makes the history empty: the next frame starts the accumulation again"""
        check(_temporal_lib().vxrt_history_reset(self.handle), "vxrt_history_reset")

    def read(self, out_ptr, stream=None):
        """vxrt_history_read: (E_acc.rgb, len) per pixel of the last frame's window into device memory; raises for an empty history"""
        check(_temporal_lib().vxrt_history_read(self.handle, out_ptr, stream), "vxrt_history_read")

    def read_moments(self, out_ptr, stream=None):
        """vxrt_history_read_moments: (m1, m2) per pixel of the last frame's window; raises for an empty history or one without moments"""
        check(_variance_lib().vxrt_history_read_moments(self.handle, out_ptr, stream), "vxrt_history_read_moments")


def _history(h):
    return h.handle if isinstance(h, History) else h


def temporal_accumulate(history, cam, width, height, y0, y1, signal_ptr, position_ptr, normal_ptr, temporal, out_ptr, stream=None):
    """vxrt_temporal_accumulate: the accumulation step alone over rows [y0, y1) of a width x height frame seen from `cam` (signal: 3 floats
    per pixel; position / normal: 4; out: 4 = the blended signal and the accumulated length); `temporal`: a TemporalParams."""
    check(_temporal_lib().vxrt_temporal_accumulate(_history(history), C.byref(_camera(cam)), width, height, y0, y1, signal_ptr, position_ptr, normal_ptr,
                                                   C.byref(temporal), out_ptr, stream), "vxrt_temporal_accumulate")


def render_path_temporal(accel, cam, width, height, y0, y1, params, spp, bounces, denoise, temporal, history, dst_ptr, seed=0, shadow=0, colors_ptr=None,
                         aov=None, rays_ptr=None, stream=None):
    """vxrt_render_path_temporal: render_path_denoised whose demodulated indirect term is first blended with `history` (a History),
    reprojected through the camera of the history's previous frame; `temporal`: a TemporalParams.  `cam` must be a camera."""
    pp = _path_params(spp, bounces, seed, shadow)
    check(_temporal_lib().vxrt_render_path_temporal(accel, C.byref(_camera(cam)), width, height, y0, y1, C.byref(params), C.byref(pp), C.byref(denoise),
                                                    C.byref(temporal), _history(history), dst_ptr, colors_ptr, None if aov is None else C.byref(aov),
                                                    rays_ptr, stream), "vxrt_render_path_temporal")


# ---- motion: temporal accumulation that reprojects through moved instances (the header's "Motion") ----
def accel_motion_snapshot(accel, what, stream=None):
    """vxrt_accel_motion_snapshot: "the scene as it is now is the previous frame" -- the accel copies the instance records
    (REFIT_INSTANCES) and the vertices as well (REFIT_INSTANCES | REFIT_GEOMETRY); 0 frees the snapshot.  Raises on a refusal."""
    check(_motion_lib().vxrt_accel_motion_snapshot(accel, int(what), stream), "vxrt_accel_motion_snapshot")


def previous_positions(accel, n, hits_ptr, prev_position_ptr, prev_normal_ptr, stream=None):
    """vxrt_previous_positions: where the surface point of each of n hit records was when the snapshot was taken, and its shading normal
    there (4 floats per record each, device, 16-byte aligned)."""
    check(_motion_lib().vxrt_previous_positions(accel, int(n), hits_ptr, prev_position_ptr, prev_normal_ptr, stream), "vxrt_previous_positions")


def temporal_accumulate_motion(history, cam, width, height, y0, y1, signal_ptr, position_ptr, normal_ptr, prev_position_ptr, prev_normal_ptr, temporal,
                               out_ptr, stream=None):
    """vxrt_temporal_accumulate_motion: temporal_accumulate that reprojects every pixel's previous position (4 floats per pixel) and tests
    the taps against it and the previous normal."""
    check(_motion_lib().vxrt_temporal_accumulate_motion(_history(history), C.byref(_camera(cam)), width, height, y0, y1, signal_ptr, position_ptr,
                                                        normal_ptr, prev_position_ptr, prev_normal_ptr, C.byref(temporal), out_ptr, stream),
          "vxrt_temporal_accumulate_motion")


def render_path_temporal_motion(accel, cam, width, height, y0, y1, params, spp, bounces, denoise, temporal, history, dst_ptr, seed=0, shadow=0,
                                colors_ptr=None, aov=None, prev_position_ptr=None, rays_ptr=None, stream=None):
    """vxrt_render_path_temporal_motion: render_path_temporal whose history is looked up where the accel's motion snapshot puts every
    pixel's surface point; `prev_position_ptr` (optional) receives that position, 4 floats per pixel of the frame."""
    pp = _path_params(spp, bounces, seed, shadow)
    check(_motion_lib().vxrt_render_path_temporal_motion(accel, C.byref(_camera(cam)), width, height, y0, y1, C.byref(params), C.byref(pp),
                                                         C.byref(denoise), C.byref(temporal), _history(history), dst_ptr, colors_ptr,
                                                         None if aov is None else C.byref(aov), prev_position_ptr, rays_ptr, stream),
          "vxrt_render_path_temporal_motion")


# ---- variance guidance: luminance moments in the history steer the a-trous filter (the header's "Variance guidance") ----
class VarianceParams(C.Structure):   # vxrt_variance_params_t
    _fields_ = [("epsilon", C.c_float), ("min_len", C.c_uint32), ("radius", C.c_uint32), ("reserved", C.c_uint32)]


ADAPTIVE_SCAN_BLOCK = 1024                        # PT_SCAN_BLOCK (rt_path.hip): pixels per block of the counts' scan
ADAPTIVE_SCAN_PASS = 1024 * ADAPTIVE_SCAN_BLOCK   # PT_SCAN_PASS blocks: pixels one pass of the single-workgroup scan covers


class SampleCountParams(C.Structure):   # vxrt_sample_count_params_t
    _fields_ = [("gain", C.c_float), ("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("reserved", C.c_uint32)]


MAX_EMITTERS = 65536   # VXRT_MAX_EMITTERS


class EmissiveParams(C.Structure):   # vxrt_emissive_params_t
    _fields_ = [("nee", C.c_uint32), ("scale", C.c_float), ("reserved", C.c_uint32 * 2)]


class EmissiveMisParams(C.Structure):   # vxrt_emissive_mis_params_t
    _fields_ = [("scale", C.c_float), ("reserved", C.c_uint32 * 3)]


class PathFrame(C.Structure):   # vxrt_path_frame_t: what a path frame is made of; a part left None is absent
    _fields_ = [("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("y0", C.c_uint32), ("y1", C.c_uint32), ("motion", C.c_uint32),
                ("cam", C.POINTER(Camera)), ("params", C.POINTER(ShadeParams)), ("path", C.POINTER(PathParams)),
                ("emissive", C.POINTER(EmissiveParams)), ("emissive_mis", C.POINTER(EmissiveMisParams)), ("counts", C.c_void_p),
                ("denoise", C.POINTER(DenoiseParams)), ("aov", C.POINTER(PathAov)), ("temporal", C.POINTER(TemporalParams)), ("history", C.c_void_p),
                ("variance", C.POINTER(VarianceParams)), ("dst", C.c_void_p), ("colors", C.c_void_p), ("prev_position", C.c_void_p),
                ("variance_out", C.c_void_p), ("rays_traced", C.c_void_p), ("reserved", C.c_uint32 * 4)]

    def __init__(self, width, height, y0, y1, params, path, dst, cam=None, emissive=None, emissive_mis=None, counts=None, denoise=None, aov=None,
                 temporal=None, history=None, motion=0, variance=None, colors=None, prev_position=None, variance_out=None, rays_traced=None):
        """`params`, `path` and the optional parts are the structures the render_path* calls take (`cam`: a Camera or 14 floats; `history`:
        a History); `dst`, `counts` and the optional outputs are device pointers.  The structures are kept alive by the frame."""
        super().__init__()
        self.size = C.sizeof(PathFrame)
        self.width, self.height, self.y0, self.y1, self.motion = int(width), int(height), int(y0), int(y1), int(motion)
        self._keep = [None if cam is None else _camera(cam), params, path, emissive, emissive_mis, denoise, aov, temporal, variance]
        for name, part in zip(("cam", "params", "path", "emissive", "emissive_mis", "denoise", "aov", "temporal", "variance"), self._keep):
            if part is not None:
                setattr(self, name, C.pointer(part))
        h = None if history is None else _history(history)
        self.history = h.value if isinstance(h, C.c_void_p) else h
        self.counts, self.dst, self.colors, self.prev_position = counts, dst, colors, prev_position
        self.variance_out, self.rays_traced = variance_out, rays_traced


class SpecularParams(C.Structure):   # vxrt_specular_params_t: rides beside a PathFrame (the header's "Specular vertices")
    _fields_ = [("enable", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def __init__(self, enable=1):
        super().__init__()
        self.enable = int(enable)


class RouletteParams(C.Structure):   # vxrt_roulette_params_t: rides beside a PathFrame (the header's "Russian roulette")
    _fields_ = [("enable", C.c_uint32), ("first", C.c_uint32), ("q_min", C.c_float), ("reserved", C.c_uint32)]

    def __init__(self, enable=1, first=2, q_min=0.05):
        super().__init__()
        self.enable, self.first, self.q_min = int(enable), int(first), float(q_min)


class EnvMap:
    """vxrt_envmap_t: an octahedral radiance map (the header's "Environment light"), made from host texels (n, n, 3) float32 with texel
    (i, j) at [j, i]; n a power of two in 4..256.  A context manager; the map must outlive the frames that read it."""

    def __init__(self, texels, stream=None):
        import numpy as np
        t = np.ascontiguousarray(texels, np.float32)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3:
            raise ValueError("texels must be (n, n, 3)")
        self.n = int(t.shape[0])
        h = C.c_void_p()
        check(_lib().vxrt_envmap_create(t.ctypes.data, self.n, stream, C.byref(h)), "vxrt_envmap_create")
        self.handle = h

    def close(self):
        if self.handle is not None:
            _lib().vxrt_envmap_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def bytes(self):
        return int(_lib().vxrt_envmap_bytes(self.handle))

    def read(self, stream=None):
        """(q, cum): the table's quantised weights and their inclusive prefix sums, (n * n,) uint32 each, in texel order"""
        import numpy as np
        q, cum = np.zeros(self.n * self.n, np.uint32), np.zeros(self.n * self.n, np.uint32)
        check(_lib().vxrt_envmap_read(self.handle, q.ctypes.data, cum.ctypes.data, stream), "vxrt_envmap_read")
        return q, cum


class EnvParams(C.Structure):   # vxrt_env_params_t: rides beside a PathFrame (the header's "Environment light")
    _fields_ = [("map", C.c_void_p), ("scale", C.c_float), ("sample", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, map, scale=1.0, sample=1):
        super().__init__()
        self._keep = map
        self.map = map.handle if isinstance(map, EnvMap) else map
        self.scale, self.sample = float(scale), int(sample)


def env_lookup(map, n, dirs_ptr, scale, radiance_ptr, texel_ptr, pdf_ptr, stream=None):
    """vxrt_envmap_lookup: the map seen along n device directions (n x 3) -> radiance (n x 3: Env(w)), texel (n), pdf (n: the solid-angle
    density of choosing that direction through the table)."""
    check(_lib().vxrt_envmap_lookup(map.handle, int(n), dirs_ptr, float(scale), radiance_ptr, texel_ptr, pdf_ptr, stream), "vxrt_envmap_lookup")


def env_rays(map, n, points_ptr, seeds_ptr, scale, rays_ptr, tmax_ptr, weight_ptr, texel_ptr, mis_ptr, stream=None):
    """vxrt_env_rays: the environment ray alone on device buffers -- points (n x 6: I, N'), seeds (n hash outputs) -> rays (n x 6), tmax
    (n), weight (n x 3: Gm), texel (n), mis (n: wE); a skipped entry has tmax = -1 and zero weights."""
    check(_lib().vxrt_env_rays(map.handle, int(n), points_ptr, seeds_ptr, float(scale), rays_ptr, tmax_ptr, weight_ptr, texel_ptr, mis_ptr, stream), "vxrt_env_rays")


def render_path_frame(accel, frame, stream=None, specular=None, roulette=None, env=None):
    """vxrt_render_path_frame: the path frame `frame` (a PathFrame) describes -- every render_path* call above is the frame with that
    call's parts, and the parts combine: an emitter form with counts, the filter, a history, motion, variance.  Raises on a refusal.
    specular (a SpecularParams): vxrt_render_path_frame_specular -- with enable = 1 the path follows reflective instances (a lobe pick
    per vertex between the mirror ray and the diffuse bounce ray); a frame without the filter chain.
    roulette (a RouletteParams): vxrt_render_path_frame_ex -- with enable = 1 the vertices first .. bounces - 1 end their path with
    probability 1 - max(q_min, largest component of the throughput) and a survivor is divided by what it survived with; not together
    with specular vertices.
    env (an EnvParams): vxrt_render_path_frame_env -- rays that leave the scene see the environment map in place of the background, and
    with sample = 1 every vertex also aims a ray at the map's bright texels, both weighted; not together with an emitter form or
    specular vertices."""
    f = C.byref(frame) if frame is not None else None
    if env is not None:
        if specular is not None:
            raise ValueError("an environment map takes no specular part")
        check(_lib().vxrt_render_path_frame_env(accel, f, None if roulette is None else C.byref(roulette), C.byref(env), stream), "vxrt_render_path_frame_env")
    elif roulette is not None:
        check(_lib().vxrt_render_path_frame_ex(accel, f, None if specular is None else C.byref(specular), C.byref(roulette), stream), "vxrt_render_path_frame_ex")
    elif specular is None:
        check(_lib().vxrt_render_path_frame(accel, f, stream), "vxrt_render_path_frame")
    else:
        check(_lib().vxrt_render_path_frame_specular(accel, f, C.byref(specular), stream), "vxrt_render_path_frame_specular")


def specular_pick(n, vertices_ptr, seeds_ptr, rays_ptr, lobe_ptr, stream=None):
    """vxrt_specular_pick: the lobe pick alone on device buffers -- vertices (n x 10: I, N, dir, reflectivity), seeds (n hash outputs) ->
    lobe (n: 1 mirror, 0 diffuse), rays (n x 6: the mirror ray of lobe 1, zeros for lobe 0)."""
    check(_lib().vxrt_specular_pick(int(n), vertices_ptr, seeds_ptr, rays_ptr, lobe_ptr, stream), "vxrt_specular_pick")


def roulette(n, thr_ptr, seeds_ptr, q_min, thr_out_ptr, alive_ptr, stream=None):
    """vxrt_roulette: the roulette draw alone on device buffers -- thr (n x 3), seeds (n hash outputs) -> alive (n: 1 continues, 0 ended),
    thr_out (n x 3: untouched where q >= 1, thr / q for a survivor, zeros for a dead entry)."""
    check(_lib().vxrt_roulette(int(n), thr_ptr, seeds_ptr, float(q_min), thr_out_ptr, alive_ptr, stream), "vxrt_roulette")


def _declare_path_family(L):
    """The prototypes of the path, denoise, temporal, motion, variance and adaptive families; _lib() calls this once with its own."""
    u32, vp, i32 = C.c_uint32, C.c_void_p, C.c_int
    frame = [vp, C.POINTER(Camera), u32, u32, u32, u32, C.POINTER(ShadeParams), C.POINTER(PathParams)]   # accel, cam, the window, params, path
    dn, tp, vr = C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(VarianceParams)
    step = [vp, C.POINTER(Camera), u32, u32, u32, u32, vp, vp, vp]   # history, cam, the window, signal, position, normal
    protos = {
        "vxrt_render_path": (i32, frame + [vp, vp, vp, vp]),
        "vxrt_render_path_denoised": (i32, frame + [dn, vp, vp, C.POINTER(PathAov), vp, vp]),
        "vxrt_denoise_scratch_bytes": (C.c_uint64, [u32, u32]),
        "vxrt_denoise": (i32, [u32, u32, vp, vp, vp, dn, vp, vp, C.c_uint64, vp]),
        "vxrt_history_create": (i32, [u32, u32, C.POINTER(vp)]),
        "vxrt_history_destroy": (i32, [vp]),
        "vxrt_history_reset": (i32, [vp]),
        "vxrt_history_read": (i32, [vp, vp, vp]),
        "vxrt_temporal_accumulate": (i32, step + [tp, vp, vp]),
        "vxrt_render_path_temporal": (i32, frame + [dn, tp, vp, vp, vp, C.POINTER(PathAov), vp, vp]),
        "vxrt_accel_motion_snapshot": (i32, [vp, u32, vp]),
        "vxrt_previous_positions": (i32, [vp, u32, vp, vp, vp, vp]),
        "vxrt_temporal_accumulate_motion": (i32, step + [vp, vp, tp, vp, vp]),
        "vxrt_render_path_temporal_motion": (i32, frame + [dn, tp, vp, vp, vp, C.POINTER(PathAov), vp, vp, vp]),
        "vxrt_history_create_moments": (i32, [u32, u32, C.POINTER(vp)]),
        "vxrt_history_read_moments": (i32, [vp, vp, vp]),
        "vxrt_temporal_accumulate_moments": (i32, step + [vp, vp, tp, vp, vp]),
        "vxrt_history_variance": (i32, [vp, dn, vr, vp, vp]),
        "vxrt_denoise_variance_scratch_bytes": (C.c_uint64, [u32, u32]),
        "vxrt_denoise_variance": (i32, [u32, u32, vp, vp, vp, vp, dn, vr, vp, vp, vp, C.c_uint64, vp]),
        "vxrt_render_path_variance": (i32, frame + [dn, tp, vr, vp, i32, vp, vp, C.POINTER(PathAov), vp, vp, vp, vp]),
        "vxrt_render_path_adaptive": (i32, frame + [vp, vp, vp, vp, vp]),
        "vxrt_render_path_variance_adaptive": (i32, frame + [vp, dn, tp, vr, vp, i32, vp, vp, C.POINTER(PathAov), vp, vp, vp, vp]),
        "vxrt_sample_counts": (i32, [C.c_uint64, vp, vp, C.POINTER(SampleCountParams), vp, vp, vp]),
        "vxrt_accel_set_emitters": (i32, [vp, vp, u32, vp]),
        "vxrt_accel_read_emitters": (i32, [vp, vp, vp, vp, vp]),
        "vxrt_render_path_emissive": (i32, frame + [C.POINTER(EmissiveParams), vp, vp, vp, vp]),
        "vxrt_emitter_rays": (i32, [vp, C.c_uint64, vp, vp, C.c_float, vp, vp, vp, vp, vp]),
        "vxrt_render_path_emissive_mis": (i32, frame + [C.POINTER(EmissiveMisParams), vp, vp, vp, vp]),
        "vxrt_emitter_rays_mis": (i32, [vp, C.c_uint64, vp, vp, C.c_float, vp, vp, vp, vp, vp, vp]),
        "vxrt_emitter_hit_weights": (i32, [vp, C.c_uint64, vp, vp, vp, vp, vp, vp]),
        "vxrt_render_path_frame": (i32, [vp, C.POINTER(PathFrame), vp]),
        "vxrt_render_path_frame_specular": (i32, [vp, C.POINTER(PathFrame), C.POINTER(SpecularParams), vp]),
        "vxrt_specular_pick": (i32, [C.c_uint64, vp, vp, vp, vp, vp]),
        "vxrt_render_path_frame_ex": (i32, [vp, C.POINTER(PathFrame), C.POINTER(SpecularParams), C.POINTER(RouletteParams), vp]),
        "vxrt_roulette": (i32, [C.c_uint64, vp, vp, C.c_float, vp, vp, vp]),
        "vxrt_envmap_create": (i32, [vp, u32, vp, C.POINTER(vp)]),
        "vxrt_envmap_destroy": (i32, [vp]),
        "vxrt_envmap_bytes": (C.c_uint64, [vp]),
        "vxrt_envmap_read": (i32, [vp, vp, vp, vp]),
        "vxrt_render_path_frame_env": (i32, [vp, C.POINTER(PathFrame), C.POINTER(RouletteParams), C.POINTER(EnvParams), vp]),
        "vxrt_envmap_lookup": (i32, [vp, C.c_uint64, vp, C.c_float, vp, vp, vp, vp]),
        "vxrt_env_rays": (i32, [vp, C.c_uint64, vp, vp, C.c_float, vp, vp, vp, vp, vp, vp]),
    }
    for name, (restype, argtypes) in protos.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes


def temporal_accumulate_moments(history, cam, width, height, y0, y1, signal_ptr, position_ptr, normal_ptr, temporal, out_ptr, prev_position_ptr=None,
                                prev_normal_ptr=None, stream=None):
    """vxrt_temporal_accumulate_moments: temporal_accumulate (or, with both previous-frame guides, temporal_accumulate_motion) on a
    History(moments=True), which then also carries the first and second luminance moments of every pixel."""
    check(_variance_lib().vxrt_temporal_accumulate_moments(_history(history), C.byref(_camera(cam)), width, height, y0, y1, signal_ptr, position_ptr,
                                                           normal_ptr, prev_position_ptr, prev_normal_ptr, C.byref(temporal), out_ptr, stream),
          "vxrt_temporal_accumulate_moments")


def history_variance(history, denoise, variance, variance_ptr, stream=None):
    """vxrt_history_variance: the initial variance V0 of the last frame of a History(moments=True), 1 float per pixel of its window --
    the temporal variance of a pixel with at least variance.min_len frames, a spatial estimate below that."""
    check(_variance_lib().vxrt_history_variance(_history(history), C.byref(denoise), C.byref(variance), variance_ptr, stream), "vxrt_history_variance")


def denoise_variance_scratch_bytes(width, rows):
    return int(_variance_lib().vxrt_denoise_variance_scratch_bytes(width, rows))


def denoise_variance(width, rows, signal_ptr, variance_ptr, position_ptr, normal_ptr, denoise, variance, out_ptr, out_variance_ptr, scratch_ptr,
                     scratch_bytes, stream=None):
    """vxrt_denoise_variance: the variance-guided a-trous filter alone (signal / out: 3 floats per pixel; variance / out_variance: 1;
    position / normal: 4); `variance`: a VarianceParams; out_variance_ptr may be None."""
    check(_variance_lib().vxrt_denoise_variance(width, rows, signal_ptr, variance_ptr, position_ptr, normal_ptr, C.byref(denoise), C.byref(variance),
                                                out_ptr, out_variance_ptr, scratch_ptr, scratch_bytes, stream), "vxrt_denoise_variance")


def render_path_variance(accel, cam, width, height, y0, y1, params, spp, bounces, denoise, temporal, variance, history, dst_ptr, motion=0, seed=0,
                         shadow=0, colors_ptr=None, aov=None, prev_position_ptr=None, variance_ptr=None, rays_ptr=None, stream=None):
    """vxrt_render_path_variance: render_path_temporal (motion=0) or render_path_temporal_motion (motion=1) on a History(moments=True),
    filtered with a per-pixel luminance scale from the variance of the accumulated luminance; `variance`: a VarianceParams;
    `variance_ptr` (optional) receives the initial variance, 1 float per pixel of the frame."""
    pp = _path_params(spp, bounces, seed, shadow)
    check(_variance_lib().vxrt_render_path_variance(accel, C.byref(_camera(cam)), width, height, y0, y1, C.byref(params), C.byref(pp), C.byref(denoise),
                                                    C.byref(temporal), C.byref(variance), _history(history), int(motion), dst_ptr, colors_ptr,
                                                    None if aov is None else C.byref(aov), prev_position_ptr, variance_ptr, rays_ptr, stream),
          "vxrt_render_path_variance")


# ---- adaptive sampling: path frames with a sample count per pixel, counts from a variance (the header's "Adaptive sampling") ----
def render_path_adaptive(accel, cam, width, height, y0, y1, params, spp, bounces, counts_ptr, dst_ptr, seed=0, shadow=0, colors_ptr=None, rays_ptr=None,
                         stream=None):
    """vxrt_render_path_adaptive: render_path whose pixel p takes min(max(counts[p], 1), spp) samples; `counts_ptr`: device, one uint32 per
    pixel of the frame, addressed like dst.  `spp` is the cap."""
    pp = _path_params(spp, bounces, seed, shadow)
    check(_lib().vxrt_render_path_adaptive(accel, _camera_ref(cam), width, height, y0, y1, C.byref(params), C.byref(pp),
                                                    counts_ptr, dst_ptr, colors_ptr, rays_ptr, stream), "vxrt_render_path_adaptive")


def render_path_variance_adaptive(accel, cam, width, height, y0, y1, params, spp, bounces, counts_ptr, denoise, temporal, variance, history, dst_ptr, motion=0,
                                  seed=0, shadow=0, colors_ptr=None, aov=None, prev_position_ptr=None, variance_ptr=None, rays_ptr=None, stream=None):
    """vxrt_render_path_variance_adaptive: render_path_variance whose path frame is render_path_adaptive's (`counts_ptr`, `spp` the cap)."""
    pp = _path_params(spp, bounces, seed, shadow)
    check(_lib().vxrt_render_path_variance_adaptive(accel, C.byref(_camera(cam)), width, height, y0, y1, C.byref(params), C.byref(pp), counts_ptr,
                                                             C.byref(denoise), C.byref(temporal), C.byref(variance), _history(history), int(motion), dst_ptr,
                                                             colors_ptr, None if aov is None else C.byref(aov), prev_position_ptr, variance_ptr, rays_ptr,
                                                             stream), "vxrt_render_path_variance_adaptive")


def sample_counts(n, variance_ptr, prm, counts_ptr, prev_counts_ptr=None, total_ptr=None, stream=None):
    """vxrt_sample_counts: counts[i] = clamp(ceil(variance[i] * m * gain), min_spp, max_spp) for n entries, m = the clamped prev_counts[i]
    (or 1); `prm`: a SampleCountParams; `total_ptr` (optional, device uint64) is incremented by the sum of the counts written."""
    check(_lib().vxrt_sample_counts(int(n), variance_ptr, prev_counts_ptr, C.byref(prm), counts_ptr, total_ptr, stream), "vxrt_sample_counts")


# ---- emissive geometry: the emitter table of an accel, path frames with area lights (the header's "Emissive geometry") ----
def emitter_pairs(buffers, ranges):
    """Host helper: the (blasIdx, triIdx) pairs of a scene's emissive triangles, as vxrt_accel_set_emitters takes them.  `buffers`: the
    scene buffers (triEx, mat as uint8 arrays); `ranges`: per instance record (first triangle, triangle count) -- the reference formats
    do not store them, the caller knows them from the meshes it built the scene from.  Returns an (n, 2) uint32 array, instances in
    order, triangles ascending, of the triangles whose material has a positive emissive component."""
    import numpy as np
    tex_id = np.frombuffer(np.ascontiguousarray(buffers["triEx"], np.uint8).tobytes(), np.uint32).reshape(-1, 16)[:, 15]
    emi = np.frombuffer(np.ascontiguousarray(buffers["mat"], np.uint8).tobytes(), np.float32).reshape(-1, 22)[:, 9:12]
    lit = (emi > 0).any(1)
    out = []
    for inst, (first, count) in enumerate(ranges):
        tris = np.arange(int(first), int(first) + int(count), dtype=np.uint32)
        tris = tris[lit[tex_id[tris]]]
        out.append(np.stack([np.full(len(tris), inst, np.uint32), tris], 1))
    return np.concatenate(out).astype(np.uint32) if out else np.zeros((0, 2), np.uint32)


def accel_set_emitters(accel, pairs, stream=None):
    """vxrt_accel_set_emitters: `pairs` = (n, 2) uint32 (blasIdx, triIdx) of every emissive triangle (see emitter_pairs); None or an
    empty list drops the table.  Raises on a refusal (the previous table is kept then)."""
    import numpy as np
    if pairs is None or len(pairs) == 0:
        check(_lib().vxrt_accel_set_emitters(accel, None, 0, stream), "vxrt_accel_set_emitters")
        return
    p = np.ascontiguousarray(np.asarray(pairs, np.uint32).reshape(-1, 2))
    check(_lib().vxrt_accel_set_emitters(accel, p.ctypes.data, len(p), stream), "vxrt_accel_set_emitters")


def accel_read_emitters(accel, stream=None):
    """vxrt_accel_read_emitters: the valid emitter table as numpy arrays -- tri12 (n, 12) float32 (V0, E1, E2, Le), q (n,), cum (n,) uint32."""
    import numpy as np
    n = accel_info(accel, 7)
    tri, q, cum = np.zeros((n, 12), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    check(_lib().vxrt_accel_read_emitters(accel, tri.ctypes.data, q.ctypes.data, cum.ctypes.data, stream), "vxrt_accel_read_emitters")
    return tri, q, cum


def render_path_emissive(accel, cam, width, height, y0, y1, params, spp, bounces, emissive, dst_ptr, seed=0, shadow=0, colors_ptr=None, rays_ptr=None,
                         stream=None):
    """vxrt_render_path_emissive: render_path with emissive triangles as area lights; `emissive`: an EmissiveParams (nee = 0: emission found
    by the bounce rays, nee = 1: emitter sampling from the accel's table; scale multiplies every material's emissive)."""
    pp = _path_params(spp, bounces, seed, shadow)
    check(_lib().vxrt_render_path_emissive(accel, _camera_ref(cam), width, height, y0, y1, C.byref(params), C.byref(pp),
                                           C.byref(emissive), dst_ptr, colors_ptr, rays_ptr, stream), "vxrt_render_path_emissive")


def emitter_rays(accel, n, points_ptr, seeds_ptr, scale, rays_ptr, tmax_ptr, weight_ptr, emitter_ptr, stream=None):
    """vxrt_emitter_rays: the emitter-sampling step alone on device buffers -- points (n x 6: I, N'), seeds (n hash outputs) -> rays (n x 6),
    tmax (n), weight (n x 3: G), emitter (n: the index chosen)."""
    check(_lib().vxrt_emitter_rays(accel, int(n), points_ptr, seeds_ptr, float(scale), rays_ptr, tmax_ptr, weight_ptr, emitter_ptr, stream), "vxrt_emitter_rays")


# ---- multiple importance sampling of area lights (the header's "Multiple importance sampling") ----
def render_path_emissive_mis(accel, cam, width, height, y0, y1, params, spp, bounces, emissive, dst_ptr, seed=0, shadow=0, colors_ptr=None, rays_ptr=None,
                             stream=None):
    """vxrt_render_path_emissive_mis: render_path_emissive with both estimators in one frame -- the emitter ray of nee = 1 and the emission the
    bounce rays find, each weighted by the balance heuristic; `emissive`: an EmissiveMisParams (scale).  Needs a valid emitter table; the
    first frame after a set_emitters builds the accel's emitter index (accel_info(accel, 8))."""
    pp = _path_params(spp, bounces, seed, shadow)
    check(_lib().vxrt_render_path_emissive_mis(accel, _camera_ref(cam), width, height, y0, y1, C.byref(params), C.byref(pp),
                                               C.byref(emissive), dst_ptr, colors_ptr, rays_ptr, stream), "vxrt_render_path_emissive_mis")


def emitter_rays_mis(accel, n, points_ptr, seeds_ptr, scale, rays_ptr, tmax_ptr, weight_ptr, emitter_ptr, mis_ptr, stream=None):
    """vxrt_emitter_rays_mis: emitter_rays with weight = Gm = G * wE and mis (n) = wE, the emitter ray's balance-heuristic weight."""
    check(_lib().vxrt_emitter_rays_mis(accel, int(n), points_ptr, seeds_ptr, float(scale), rays_ptr, tmax_ptr, weight_ptr, emitter_ptr, mis_ptr, stream),
          "vxrt_emitter_rays_mis")


def emitter_hit_weights(accel, n, rays_ptr, hits_ptr, normals_ptr, emitter_ptr, mis_ptr, stream=None):
    """vxrt_emitter_hit_weights: the bounce ray's side alone on device buffers -- rays (n x 6), hit records (n, as trace writes them), normals
    (n x 3: the facing normal of the vertex each ray left) -> emitter (n: the table entry hit, 0xFFFFFFFF: not listed), mis (n: wB)."""
    check(_lib().vxrt_emitter_hit_weights(accel, int(n), rays_ptr, hits_ptr, normals_ptr, emitter_ptr, mis_ptr, stream), "vxrt_emitter_hit_weights")
