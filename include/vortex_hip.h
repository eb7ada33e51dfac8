/*
 * include/vortex_hip.h -- C ABI of the MI355X-native ray-tracing hot path.
 *
 * Two levels, both exported by libvortex-hip.so (plain pointers and sizes, no torch types):
 *
 *  (1) DROP-IN DRIVER BOUNDARY.  `vx_dev_init(callbacks_t*)` is the one symbol the reference's
 *      dispatcher resolves with dlsym after dlopen("libvortex-$VORTEX_DRIVER.so")
 *      (reference runtime/stub/vortex.cpp:58-82).  It fills the 16 entry points declared in
 *      reference runtime/common/callbacks.h:23-72; each one replaces the simx implementation in
 *      reference runtime/simx/vortex.cpp + runtime/common/callbacks.inc (lines cited per member).
 *      With VORTEX_DRIVER=hip the unmodified host code of tests/regression/raytracing keeps
 *      calling vx_mem_alloc / vx_copy_to_dev / vx_dcr_write / vx_start / vx_ready_wait.
 *
 *  (2) DIRECT LAUNCH API `vxrt_*` for callers that already own device memory and a HIP stream
 *      (bench.py, tests, embedding in another runtime).  `start` of level (1) is implemented on
 *      top of it.  All pointers in vxrt_scene_t / rays / hits / dst are DEVICE pointers; `stream`
 *      is a hipStream_t passed as void* (NULL = default stream).  Launches are asynchronous.
 *
 * Error convention of the reference (callbacks.inc): 0 = success, non-zero (-1) = failure; no
 * exceptions cross this ABI.
 */
#ifndef VORTEX_HIP_H
#define VORTEX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * (1) driver boundary -- mirrors reference runtime/include/vortex.h:27-28 and
 *     runtime/common/callbacks.h:23-72 (same member order; the struct is filled positionally
 *     by the backend and read by the dispatcher, so the order IS the ABI).
 * ---------------------------------------------------------------------------------------- */
typedef void* vx_device_h;
typedef void* vx_buffer_h;

typedef struct {
  int (*dev_open)(vx_device_h* hdevice);                                   /* callbacks.inc:24-36 / simx vortex.cpp:49-78 */
  int (*dev_close)(vx_device_h hdevice);                                   /* callbacks.inc:38-45 */
  int (*dev_caps)(vx_device_h hdevice, uint32_t caps_id, uint64_t* value); /* callbacks.inc:47-58 / vortex.cpp:80-135 */
  int (*mem_alloc)(vx_device_h hdevice, uint64_t size, int flags, vx_buffer_h* hbuffer);   /* callbacks.inc:60-78 / vortex.cpp:209-232 */
  int (*mem_reserve)(vx_device_h hdevice, uint64_t address, uint64_t size, int flags, vx_buffer_h* hbuffer); /* :80-97 / :234-249 */
  int (*mem_free)(vx_buffer_h hbuffer);                                    /* callbacks.inc:99-108 */
  int (*mem_access)(vx_buffer_h hbuffer, uint64_t offset, uint64_t size, int flags);       /* :110-119 */
  int (*mem_address)(vx_buffer_h hbuffer, uint64_t* address);              /* :121-128 */
  int (*mem_info)(vx_device_h hdevice, uint64_t* mem_free, uint64_t* mem_used);            /* :130-146 */
  int (*copy_to_dev)(vx_buffer_h hbuffer, const void* host_ptr, uint64_t dst_offset, uint64_t size);   /* :148-158 / vortex.cpp:276-304 */
  int (*copy_from_dev)(void* host_ptr, vx_buffer_h hbuffer, uint64_t src_offset, uint64_t size);       /* :160-170 / vortex.cpp:306-327 */
  int (*start)(vx_device_h hdevice, vx_buffer_h hkernel, vx_buffer_h harguments);          /* :172-180 / vortex.cpp:329-348 */
  int (*ready_wait)(vx_device_h hdevice, uint64_t timeout);                /* :182-188 / vortex.cpp:350-364 */
  int (*dcr_read)(vx_device_h hdevice, uint32_t addr, uint32_t* value);    /* :190-201 / vortex.cpp:375-377 */
  int (*dcr_write)(vx_device_h hdevice, uint32_t addr, uint32_t value);    /* :203-209 / vortex.cpp:366-373 */
  int (*mpm_query)(vx_device_h hdevice, uint32_t addr, uint32_t core_id, uint64_t* value); /* :211-222 / vortex.cpp:379-391 */
} callbacks_t;

/* The plug-in entry (callbacks.inc:20). */
int vx_dev_init(callbacks_t* callbacks);

/* caps ids (vortex.h:31-45) */
#define VX_CAPS_VERSION 0x0
#define VX_CAPS_NUM_THREADS 0x1
#define VX_CAPS_NUM_WARPS 0x2
#define VX_CAPS_NUM_CORES 0x3
#define VX_CAPS_CACHE_LINE_SIZE 0x4
#define VX_CAPS_GLOBAL_MEM_SIZE 0x5
#define VX_CAPS_LOCAL_MEM_SIZE 0x6
#define VX_CAPS_ISA_FLAGS 0x7
#define VX_CAPS_NUM_MEM_BANKS 0x8
#define VX_CAPS_MEM_BANK_SIZE 0x9
#define VX_CAPS_NUM_CLUSTERS 0xA
#define VX_CAPS_SOCKET_SIZE 0xB
#define VX_CAPS_ISSUE_WIDTH 0xC
#define VX_CAPS_CLOCK_RATE 0xD
#define VX_CAPS_PEAK_MEM_BW 0xE

#define VX_MEM_READ 0x1
#define VX_MEM_WRITE 0x2
#define VX_MEM_READ_WRITE 0x3
#define VX_MAX_TIMEOUT (24 * 60 * 60 * 1000)

/* DCR ids the RTU path uses (hw/VX_types.toml:16-19; written by tracer.cpp:252-256). */
#define VX_DCR_BASE_STARTUP_ADDR0 0x001
#define VX_DCR_BASE_STARTUP_ADDR1 0x002
#define VX_DCR_BASE_STARTUP_ARG0 0x003
#define VX_DCR_BASE_STARTUP_ARG1 0x004
#define VX_DCR_BASE_MPM_CLASS 0x005
#define VX_DCR_BASE_RTX_TLAS_PTR 0x006
#define VX_DCR_BASE_RTX_BLAS_PTR 0x007
#define VX_DCR_BASE_RTX_BVH_PTR 0x008
#define VX_DCR_BASE_RTX_TRI_PTR 0x009
/* Backend extension (no reference counterpart): framebuffer row window rendered by this device,
 * for sharding one frame over several GPUs/processes.  [begin,end); end==0 means dst_height. */
#define VX_DCR_HIP_ROW_BEGIN 0x7F0
#define VX_DCR_HIP_ROW_END 0x7F1
/* Backend extension: 0 = closest-hit only (reference behaviour), 1 = +1 shadow ray toward light_pos. */
#define VX_DCR_HIP_SHADOW_RAYS 0x7F2
/* Backend extension: tile-row stride of the row window.  0/1 = the contiguous rows [ROW_BEGIN, ROW_END); n > 1 = this device
 * renders the 8-row tile rows phase, phase + n, phase + 2n, ... of the frame with phase = ROW_BEGIN / 8 (< n): the split of one
 * frame over n GPUs that balances them (see vxrt_render_interleaved). */
#define VX_DCR_HIP_ROW_STRIDE 0x7F3
/* Backend extension: 1 = REFERENCE-QUIRKS traversal for the RTU test's frames (default 0 = the canonical algorithm).  The frame's
 * camera rays are then traced by vxrt_trace_reference_quirks on a flat image of the device's address space -- every allocation at
 * its address, as the simulator's RAM holds it -- with the RTX DCR values as base pointers, so that the stale base_ptr of
 * rt_traversal.cpp:91-92 reads here what it reads there.  Slow (one thread per ray, the address space copied when an allocation
 * changed); closest-hit frames only (no shadow-ray extension, no row stride). */
#define VX_DCR_HIP_REFERENCE_QUIRKS 0x7F4
/* Backend extension: 1 = render the RTU test's frames from the pinhole camera of kernel_arg_t camera_pos .. viewplane (the fields
 * tracer.cpp:171-202 fills; see vxrt_camera_t) through vxrt_render_camera instead of the fixed GenerateRay of kernel.cpp:28-39.
 * Default 0 = the fixed camera, unchanged.  ROW_BEGIN / ROW_END and samples_per_pixel work as without it; vx_start returns -1 with
 * REFERENCE_QUIRKS set, with a ROW_STRIDE above 1 (there is no interleaved camera form), for a camera field that is not finite and
 * for a value above 1.  With several VORTEX_HIP_DEVICES a camera run stays on the first device, as a restricted run does. */
#define VX_DCR_HIP_CAMERA 0x7F5

/* CSRs answered by mpm_query (read by vx_dump_perf at vx_dev_close: stub/perf.cpp:195-227). */
#define VX_CSR_MPM_BASE 0xB00
#define VX_CSR_MCYCLE 0xB00
#define VX_CSR_MINSTRET 0xB02

/* kernel_arg_t of the RTU test (tests/regression/raytracing/common.h:164-195): 216 bytes.  This
 * is what the host uploads with vx_upload_bytes and what `start` decodes. */
typedef struct {
  uint32_t dst_width;
  uint32_t dst_height;
  uint64_t dst_addr;
  uint64_t tri_addr;
  uint64_t triEx_addr;
  uint64_t triIdx_addr;
  uint64_t mat_addr;
  uint64_t tex_addr;
  uint64_t bvh_addr;
  uint64_t qBvh_addr;
  uint64_t blas_addr;
  uint64_t tlas_addr;
  uint32_t tlas_root;
  float camera_pos[3];
  float camera_forward[3];
  float camera_right[3];
  float camera_up[3];
  float viewplane[2];
  uint32_t samples_per_pixel;
  uint32_t max_depth;
  float light_pos[3];
  float light_color[3];
  float ambient_color[3];
  float background_color[3];
  uint64_t sbt_addr;
} vx_rt_kernel_arg_t;

/* ------------------------------------------------------------------------------------------
 * (2) direct launch API
 * ---------------------------------------------------------------------------------------- */

/* Device-resident scene in the reference's own buffer formats:
 *   tlas, bvh : bvh_quantized_node_t[]  52 B   (common.h:52-67 == sim rt_traversal.h:14-33)
 *   blas      : blas_node_t[]          160 B   (common.h:86-99)
 *   tri       : tri_t[]                 36 B   (geometry.h:1401-1405)
 *   triEx     : tri_ex_t[]              64 B   (common.h:39-43)
 *   mat       : material_info_t[]       88 B   (common.h:20-36)
 *   tex       : 0x00RRGGBB u32 texels, concatenated (surface.cpp:28-55)
 * Counts are element counts and are used for host-side shape checks before every launch. */
typedef struct {
  const void* tlas;
  const void* blas;
  const void* bvh;
  const void* tri;
  const void* triEx;
  const void* mat;
  const void* tex;
  uint32_t n_tlas_nodes;
  uint32_t n_blas;
  uint32_t n_bvh_nodes;
  uint32_t n_tris;
  uint32_t n_mats;
  uint32_t reserved;
  uint64_t tex_bytes;
} vxrt_scene_t;

/* Hit record: the 6 RTU hit attributes (VX_RT_HIT_DIST..TRI_IDX, hw/VX_types.toml:270-285;
 * sim rt_traversal.h:48-52).  dist == 1e30f means miss. */
typedef struct {
  float dist, bx, by, bz;
  uint32_t blasIdx, triIdx;
} vxrt_hit_t;

typedef struct {
  float ambient[3], light_color[3], light_pos[3], background[3];
  uint32_t max_depth;
} vxrt_shade_params_t;

#define VXRT_MODE_CLOSEST 0 /* reference semantics: global closest hit, reference tie order */
#define VXRT_MODE_ANY 1     /* occlusion: stop at first accepted candidate (extension) */

/* Device-side acceleration layout built ONCE per scene from the reference-format buffers above
 * (compact 64-byte nodes with inlined leaf / instance descriptors, edge-form triangles).  The build
 * validates every index the traversal can follow and fails (-1) on a malformed tree instead of
 * letting a kernel fault; so are the indices shading follows (every triangle's texId < n_mats; a textured material's
 * texels inside [tex, tex + tex_bytes) with non-zero dimensions).  With RT_TOP_NODES > 0 (build flag) the first internal
 * nodes in breadth-first order are also laid out as an image each workgroup stages in LDS.
 * The vxrt_scene_t buffers must stay alive and unchanged while the accel
 * is in use (shading reads blas/triEx/mat/tex from them); moved instances or vertices go through vxrt_accel_set_transforms /
 * vxrt_accel_refit below, never through the buffers alone.  Synchronous with respect to `stream`. */
typedef struct vxrt_accel vxrt_accel_t;
int vxrt_accel_build(const vxrt_scene_t* scene, void* stream, vxrt_accel_t** out);
int vxrt_accel_destroy(vxrt_accel_t* accel);
uint64_t vxrt_accel_bytes(const vxrt_accel_t* accel);
/* What the build found (diagnostic): which = 0 -> internal levels on the longest root-to-leaf path, TLAS and BLAS together, counted up
 * to 17; 1 -> 1 if the scene is at most 16 levels deep and its timed launches keep 48-entry traversal stacks (deeper scenes: the
 * reference's 32 levels, 96 entries + the LDS part); 2 -> 1 if the TLAS root is a single identity instance; 3 -> 1 if the scene
 * takes the ldexp decode / generic slab form; 4 -> 1 while a non-zero alpha table is set (vxrt_accel_set_alpha_test); 5 -> 1 if the
 * timed plain / shadow frames take the identity-root kernels (2 holds, 1 holds, 3 and 4 do not); 6 -> the VXRT_REFIT_* mask of the
 * motion snapshot the accel holds (vxrt_accel_motion_snapshot), 0 for none; 7 -> the number of emitters of a valid emitter table
 * (vxrt_accel_set_emitters), 0 for none or a stale one; 9 -> 1 if the accel holds a path table (one 32-bit word per triangle, counted by
 * vxrt_accel_bytes: see vxrt_debug_set_shadow_hints). */
int vxrt_accel_info(const vxrt_accel_t* accel, uint32_t which, uint64_t* value);

/* Refit: new boxes for a scene whose instances or vertices moved, in place, without a rebuild (extension; the reference has no refit,
 * its pieces are blas_node_t::applyTransform + mat4_t::inverted(), common.h:95-98 / geometry.h:1149-1192, the TLAS leaf box of
 * bvh.cpp:290-304 and the quantiser of bvh.cpp:215-264).
 *   VXRT_REFIT_INSTANCES  instance transforms changed: instance boxes + TLAS
 *   VXRT_REFIT_GEOMETRY   triangle vertices changed (same count, same order): edge-form triangles, every BLAS, then instance boxes + TLAS
 * Topology is kept: leftFirst, leafData, imask, node counts and the triangle order are never touched, only boxes move -- every node's
 * origin and exponents and its children's quantised bytes (the builder's quantiser, csrc/bvh_quant.h), in scene.tlas and, for
 * GEOMETRY, scene.bvh, rewritten in place: the caller's buffers stay a valid reference-format scene.  The accel then behaves exactly
 * like vxrt_accel_build on the updated buffers (compact nodes, edge-form triangles, the LDS top-of-tree image, info 2 and 3);
 * info 0 and 1 cannot change.  An instance's object box is the refit's own box of its BLAS root after a GEOMETRY pass, else the
 * union of the root's decoded child boxes (the triangle box for a leaf root); its 8 corners go through `transform` in fp32 without
 * contraction.  The first refit of an accel builds a plan of the trees' levels (one synchronisation, a host copy of the nodes).
 * Ordered after every call already issued on this accel, on any stream; synchronous with respect to `stream` (one host
 * synchronisation at the end), so every later call is ordered after it.
 * what == 0 moves nothing and writes nothing: it returns 0, or -1 for a stale accel (or a tree the plan refuses).
 * Returns -1 for a null accel, unknown bits in `what`, a non-finite vertex or transformed box, or a box that cannot be quantised.
 * A tree with an internal node that has no present child is refused (-1) when the plan is built, before anything is written; the
 * accel is then not stale.
 * A refit that fails after it has started writing marks the accel STALE: every render, trace or stats call on it returns -1
 * without launching anything until a later refit succeeds (a refit of a stale accel redoes the BLAS boxes as well). */
#define VXRT_REFIT_INSTANCES 1u
#define VXRT_REFIT_GEOMETRY 2u
int vxrt_accel_refit(vxrt_accel_t* accel, uint32_t what, void* stream);
/* transforms: DEVICE, count x 16 floats, mat4_t::cell order (row-major, translation in cells 3/7/11).  Writes transform and
 * invTransform (= mat4_t::inverted(), MESA operation order, no contraction) into instance records first .. first+count-1 of the
 * scene's blas buffer, then refits as vxrt_accel_refit(accel, VXRT_REFIT_INSTANCES).  Returns -1 for first + count > n_blas, a
 * non-finite matrix or a singular one (det == 0, for which the reference would silently keep the identity); the matrices are
 * checked before any record is written, so then every record is left as it was. */
int vxrt_accel_set_transforms(vxrt_accel_t* accel, uint32_t first, uint32_t count, const float* transforms, void* stream);

/* Alpha test: cutout textures reject candidates inside the traversal (extension; the reference's any-hit shader holds the test,
 * anyhit.cpp:24-35, with alpha hard-wired to 1, and its COMMIT_CONT path cannot serve as the definition: DESIGN.md s2, "Alpha test").
 * thresholds: HOST, n_mats bytes, one per material.  0 = the material is opaque (no test, no fetch); T in 1..255 = a candidate -- a
 * triangle test that returns d < hit.dist -- on a triangle of that material is REJECTED when the texel the closest-hit shader would
 * sample for it has a top byte below T: texels are 0xAARRGGBB, AA is read by this test alone (shading keeps masking it off), the texel
 * index is computed exactly as vxrt_shade_rays computes it (u, v from uv0..2 and the candidate's barycentrics without contraction,
 * uint32_t(u * (float)tex_width) % tex_width by the conversion rule written there: negative uv wraps, NaN gives 0).  T = 128 is the
 * reference's `alpha < 0.5f` for an 8-bit alpha.  A rejected candidate is treated in every respect as if the triangle test had
 * missed: hit.dist and the record stay, no abandon test, an any-hit ray does not stop, the leaf's next triangle follows.
 * NULL (n_mats is then ignored) or all zeros switches the test off: the accel launches exactly the kernels it launches without it.
 * The thresholds are copied to storage the accel owns, together with each triangle's texId as the scene holds it at this call.  Ordered
 * after every call already issued on this accel, on any stream; synchronous with respect to `stream`, like vxrt_accel_refit.  The table
 * survives vxrt_accel_refit and vxrt_accel_set_transforms.  vxrt_accel_info(accel, 4) is 1 while a non-zero table is set.
 * Returns -1, with nothing changed, for a null or stale accel, n_mats different from the scene's, or a non-zero threshold for a
 * material without a texture (diffuse_tex_id < 0).  vxrt_accel_build has validated every textured material's texel range.
 * While a non-zero table is set:
 *   vxrt_trace (both modes, the rays traced by its EXACT launch included), vxrt_render and vxrt_render_camera (primary rays, the
 *   occlusion rays of shadow != 0 -- light passes through holes -- and the mirror-bounce rays up to max_depth) honour it for every
 *   ray they trace; their optional outputs are as without it;
 *   EVERY OTHER entry point that traces rays returns -1 before it launches anything -- vxrt_render_interleaved, the *_batch and
 *   rows forms, vxrt_render_stats / _stats_timed / _wave_log, vxrt_trace_stats, vxrt_render_ao / _diffuse_bounce and their camera
 *   forms, vxrt_render_path, vxrt_render_path_denoised: none of them silently ignores the table;
 *   vxrt_shade_rays and the ray generators trace nothing and are unaffected.  The vx_* boundary has no access to the table. */
int vxrt_accel_set_alpha_test(vxrt_accel_t* accel, const uint8_t* thresholds /* HOST, n_mats entries, or NULL */, uint32_t n_mats,
                              void* stream);

/* Number of frames (vxrt_render / vxrt_trace calls) this accel keeps in flight, 1..8, default 1.
 * Each in-flight frame has its own hit-record buffer, deferred-ray list and side stream; calls take
 * them round robin, and a call that reuses a context is ordered behind that context's previous
 * call by an event.  With n > 1 and the calls issued on n different streams, the draining tail of
 * one persistent traversal launch overlaps the head of the next frame's (the reference renders one
 * frame per vx_start, tracer.cpp:272-281; this is the knob a frame loop around it would use).
 * Waits for the device to go idle.  Results do not depend on n. */
int vxrt_accel_frames_in_flight(vxrt_accel_t* accel, uint32_t n);

/* Render rows [y0,y1) of the RTU test's frame: camera ray (kernel.cpp:28-39) -> closest hit ->
 * closest/miss shade -> RGB8 pack -> dst[x + y*W] (kernel.cpp:95-106).  `dst` points at pixel
 * (0,0) of the full W x H frame.  shadow != 0 adds one occlusion ray per hit (extension).
 * rays_traced (device u64, may be NULL) is atomically incremented by the number of rays traced.
 * Two launches on `stream`: the persistent traversal kernel leaves 24-byte hit records (tile-major, one
 * contiguous 1,536-byte block per 8x8 tile, written once) in a buffer owned by the frame context, the shading
 * kernel turns them into pixels.
 * hits (optional): the pixel's closest-hit record in pixel order; with shadow != 0, bit 31 of blasIdx is set
 * when the pixel's occlusion ray was blocked (mask it off to compare with a closest-hit record). */
int vxrt_render(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                const vxrt_shade_params_t* params, int shadow, uint32_t* dst,
                vxrt_hit_t* hits /* optional, W*H */, float* colors /* optional, 3*W*H */,
                unsigned long long* rays_traced, void* stream);

/* One rank's share of a frame split over `stride` devices: the 8-row tile rows phase, phase + stride, ... (phase < stride).
 * Same contract as vxrt_render otherwise (dst points at pixel (0,0) of the full frame and only this share's rows are
 * written).  Interleaving balances the ranks: the cost of a tile varies 4x over the frame, mostly with image height. */
int vxrt_render_interleaved(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t phase, uint32_t stride,
                            const vxrt_shade_params_t* params, int shadow, uint32_t* dst, vxrt_hit_t* hits,
                            float* colors, unsigned long long* rays_traced, void* stream);

/* BLAS construction on the GPU, in the reference's formats.  Replaces, for one mesh, BVH::build + the 4-wide collapse + the
 * quantiser of tests/regression/raytracing/bvh.cpp:30-264 (host code run at scene load in the reference; csrc/scene_builder.cpp
 * is the CPU counterpart here).  Morton order, PLOC clustering (mutual nearest neighbours by surface area of the union), 4-wide
 * collapse by the SAH dynamic programme; see csrc/bvh_builder.hip.
 *   tri      device, n_tris x 36 B (tri_t); REORDERED IN PLACE so that a leaf is a range (bvh.cpp:126-128)
 *   triEx    device, n_tris x 64 B (tri_ex_t), reordered alongside; may be NULL
 *   tri_offset  added to every leaf's leftFirst (index of the mesh's first triangle in the scene's buffer, bvh.cpp:260)
 *   leaf_max    largest leaf, 1..15 (0 = 2); a subtree of <= leaf_max triangles becomes a leaf where the surface-area cost of that
 *               is lower than a node over it (2 / 3 / 4 measured equal within 1 % on the 1M-triangle scene: profiles/r03_t_builder_cost_ab.txt)
 *   nodes    device, node_capacity x 52 B (bvh_quantized_node_t), node_capacity >= 2 * n_tris - 1 (the reference allocates
 *            2 * numTris, scene.cpp:40); node 0 is the root, children follow their parent
 * Synchronises `stream` a few times (the cluster count between groups of clustering rounds, the counts at the end).  Returns 0; -1 on bad arguments, allocation failure or a box that cannot
 * be quantised; -2 if the tree is deeper than the 32 levels the reference's trail supports (use the SAH builder).
 * Non-finite input is refused, the rule of vxrt_accel_refit: a NaN or infinite coordinate in any vertex returns -1 (a NaN would
 * otherwise drop out of every min / max and leave a tree, and bounds, that do not cover the triangle).  So does a mesh whose extent
 * along an axis overflows fp32 (no exponent quantises it).  After -1 or -2 tri / triEx may have been reordered, nodes and info hold
 * no tree; the next build is unaffected. */
typedef struct vxrt_bvh_info {
  uint32_t n_nodes, n_leaves, max_leaf, max_depth;
  float bounds[6];        /* of the mesh: lo xyz, hi xyz */
} vxrt_bvh_info_t;
int vxrt_bvh_build(void* tri, void* triEx, uint32_t n_tris, uint32_t tri_offset, uint32_t leaf_max,
                   void* nodes, uint32_t node_capacity, vxrt_bvh_info_t* info, void* stream);
/* TLAS over instances on the GPU (reference: BVH::buildTLAS, bvh.cpp:266-421): instance_boxes = device, n_instances x 6 floats
 * (world-space lo xyz, hi xyz of instance i = blas record i); nodes = device, node_capacity >= 2 * n_instances - 1 entries of 52 B;
 * node 0 is the root, a leaf carries leafData = i, internal nodes UINT32_MAX, imask = 1.  Same return codes as vxrt_bvh_build,
 * the non-finite rule included: a NaN or infinite coordinate in any instance box returns -1. */
int vxrt_tlas_build(const float* instance_boxes, uint32_t n_instances, void* nodes, uint32_t node_capacity,
                    vxrt_bvh_info_t* info, void* stream);
/* The builder keeps one grow-only scratch allocation per process (about 170 B per triangle of the largest build) so that a
 * mesh rebuilt every frame allocates nothing; this returns it to the device. */
void vxrt_bvh_release_scratch(void);

/* n_frames (1..VXRT_MAX_BATCH) consecutive frames of the same share in ONE set of launches: frame f is lit and shaded with
 * params[f] (an array of n_frames entries: e.g. a moving light) and written to dst + f * dst_frame_stride (in pixels; each frame
 * buffer addressed like vxrt_render_interleaved's).  A rank's share of a frame split N ways is small against the machine and takes
 * as long as its slowest tile however small it is; a sequence of frames traced side by side keeps the GPU full, and the assembly
 * of N shares becomes one collective per batch (bench.py --gpus N).  No optional outputs; scenes without reflective instances. */
#define VXRT_MAX_BATCH 32
int vxrt_render_interleaved_batch(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t phase, uint32_t stride, uint32_t n_frames,
                                  const vxrt_shade_params_t* params, int shadow, uint32_t* dst, uint64_t dst_frame_stride,
                                  unsigned long long* rays_traced, void* stream);

/* diagnostic: the traversal launch of vxrt_render_interleaved_batch in the counting build with vxrt_render_wave_log's per-wavefront
 * log ([15] = 100 MHz clock at which the wavefront found every queue shard empty); pixels are not produced.  tools/wave_balance_batch.py */
int vxrt_render_interleaved_batch_wave_log(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t phase, uint32_t stride, uint32_t n_frames,
                                           const vxrt_shade_params_t* params, int shadow, uint32_t* dst, uint64_t dst_frame_stride,
                                           unsigned long long* counters, unsigned long long* wave_log, void* stream);

/* Image assembly of a frame split by interleaved tile rows (north_star: "RCCL gather only for final image assembly"), the two ends of
 * the wire.  Pixels are 0x00RRGGBB (common.h:149-154): the top byte is always zero, so a share travels as 3 bytes per pixel.
 *   vxrt_wire_pack    rank `rank` of `world`: the tile rows rank, rank + world, ... (tile_rows_per_rank of them, 8 rows each; rows
 *                     past the frame's end are whatever the padded frame buffer holds) of n_frames frames -- frame f at
 *                     frames + f * frame_stride, `width` pixels per row -- packed into `wire`:
 *                     [n_frames][tile_rows_per_rank * 8][width][3] bytes (b, g, r).  width must be a multiple of 4.
 *   vxrt_wire_unpack  rank 0: the `world` shares, rank r's at wire_all + r * wire_stride_bytes, expanded and interleaved into
 *                     n_frames frames of tile_rows_per_rank * world * 8 rows (the padded height the shares were rendered into).
 * One launch each, asynchronous on `stream`; they replace a strided extraction copy and an interleaving copy of 4-byte pixels. */
int vxrt_wire_pack(const uint32_t* frames, uint64_t frame_stride, uint32_t width, uint32_t tile_rows_per_rank, uint32_t world, uint32_t rank,
                   uint32_t n_frames, uint8_t* wire, void* stream);
int vxrt_wire_unpack(const uint8_t* wire_all, uint64_t wire_stride_bytes, uint32_t width, uint32_t tile_rows_per_rank, uint32_t world,
                     uint32_t n_frames, uint32_t* frames, uint64_t frame_stride, void* stream);

/* The same for a contiguous band of rows [y0, y1) (0 <= y0 <= y1 <= height; any row, tiles are counted from y0): what a rank
 * renders when the frame is split into bands whose heights are balanced by cost (bench.py --shard bands).  dst addresses every
 * frame as a FULL frame does -- pixel (x, y) of frame f at dst[f * dst_frame_stride + x + y * width] -- and only rows [y0, y1)
 * are written, so a caller that keeps only its band passes (band buffer - y0 * width) and dst_frame_stride = (y1 - y0) * width:
 * the band then lies contiguous in memory, ready to be sent, and rank 0 receives every band straight into its place in the
 * final image (no extraction and no interleaving copy: the grid being sharded is kernel.cpp:128-133). */
int vxrt_render_rows_batch(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, uint32_t n_frames,
                           const vxrt_shade_params_t* params, int shadow, uint32_t* dst, uint64_t dst_frame_stride,
                           unsigned long long* rays_traced, void* stream);

/* The same for whole frames (one rank): n_frames frames of width x height, frame f lit and shaded with params[f], written to
 * dst + f * dst_frame_stride.  Every wavefront then works through n_frames times as many tiles per launch, so a launch's ramp and
 * tail weigh less: +8 % at 1920x1080 with 5 frames per set of launches. */
int vxrt_render_batch(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t n_frames, const vxrt_shade_params_t* params, int shadow,
                      uint32_t* dst, uint64_t dst_frame_stride, unsigned long long* rays_traced, void* stream);

/* A pinhole camera: 14 floats, the layout of kernel_arg_t camera_pos .. viewplane (tracer.cpp:171-202 fills them) and of the head of
 * vxrc_params_t.  The ray of pixel (x, y) of a W x H frame is the reference's GenerateRay (raycast/render.h:192-211), operation for
 * operation (no FMA contraction):
 *   x_ndc = (float)((double)(((float)x + 0.5f) / (float)W) - 0.5), y_ndc likewise with y and H
 *   x_vp = x_ndc * viewplane[0], y_vp = y_ndc * viewplane[1]
 *   pt_cam = (x_vp * right + y_vp * up) + forward, pt_w = pt_cam + pos, d = pt_w - pos, d *= 1 / sqrtf(dot(d, d)); origin = pos
 * Every camera whose 14 fields are finite is legal, degenerate ones included (zero viewplane, a basis that is not orthonormal, a
 * direction that normalises to zero or NaN): such rays are traced as the reference would trace them. */
typedef struct vxrt_camera {
  float pos[3], forward[3], right[3], up[3], viewplane[2];
} vxrt_camera_t;

/* vxrt_render seen from `cam` instead of the RTU test's fixed camera: the same arguments and outputs (closest hit, the optional
 * occlusion ray and its bit 31 in hits[].blasIdx, shading, the mirror bounce up to params->max_depth, the RGB8 pack, colours,
 * rays_traced).  `cam` is a host pointer read during the call; the launches stay asynchronous on `stream` and no host
 * synchronisation is added: the camera's tables are built on the stream in the frame context's own storage, so frames in flight
 * with different cameras do not see each other's.  Returns -1 before anything is launched (dst untouched) for a null camera, a
 * camera field that is not finite, a stale accel, and whatever vxrt_render refuses. */
int vxrt_render_camera(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                       const vxrt_shade_params_t* params, int shadow, uint32_t* dst, vxrt_hit_t* hits /* optional */, float* colors /* optional */,
                       unsigned long long* rays_traced, void* stream);

/* vxrt_render_batch with a camera per frame: frame f is seen from cams[f], lit and shaded with params[f] and written to
 * dst + f * dst_frame_stride -- a fly-through in one set of launches.  The limits of vxrt_render_batch (1..VXRT_MAX_BATCH frames,
 * no optional outputs, no reflective instances with max_depth > 1) and the refusals of vxrt_render_camera apply. */
int vxrt_render_batch_camera(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t n_frames, const vxrt_camera_t* cams,
                             const vxrt_shade_params_t* params, int shadow, uint32_t* dst, uint64_t dst_frame_stride,
                             unsigned long long* rays_traced, void* stream);

/* vxrt_render with the fetch counters compiled in (diagnostic build of the same kernel, never
 * timed): counters = device u64[7]: rays, node fetches, instance fetches, triangle fetches,
 * shaded hits, textured hits, pixels written.  Counts are what the reference logs per ray in
 * RT_mem_accesses (rt_traversal.cpp:54,116,148,158) without its restart re-reads. */
int vxrt_render_stats(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                      const vxrt_shade_params_t* params, int shadow, uint32_t* dst,
                      unsigned long long* counters, void* stream);

/* vxrt_render_stats for the traversal the TIMED kernel performs (same counters): a frame's occlusion rays visit children in
 * slot order instead of near-to-far (the result is a boolean) and idle lanes test a leaf's second triangle, so its node /
 * triangle fetch counts differ from the reference-order ones; bench.py reports both. */
int vxrt_render_stats_timed(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                            const vxrt_shade_params_t* params, int shadow, uint32_t* dst,
                            unsigned long long* counters, void* stream);

/* vxrt_trace with the fetch counters compiled in (slower; never a timed path).  counters: device u64[8], of which
 * [0..3] = rays, node fetches, instance fetches, triangle fetches as the reference accounts them (rt_traversal.cpp:
 * 54,116,148,158, without restart re-reads) -- the inputs of the algorithmic bytes per ray. */
int vxrt_trace_stats(vxrt_accel_t* accel, const float* rays, uint64_t n, const float* tmax,
                     vxrt_hit_t* hits, int mode, unsigned long long* counters, void* stream);

/* Ambient-occlusion frame (extension for BASELINE config 5, "16 spp Monte-Carlo AO"; the reference has no
 * such pass, only its RNG is used: common.h:129-147).  Per pixel with a primary hit: spp cosine-weighted
 * occlusion rays about the shading normal (tmax = radius, any-hit), pixel = Lambert colour of the hit
 * (closest.cpp:57-127, else arm) x unoccluded / spp.  The sampling recipe is fixed in
 * oracle/rt_oracle.c:orc_ao_ray and uses IEEE add/mul/div/sqrt only, so the frame is reproducible bit
 * for bit.  unoccluded (optional): device u32 per pixel.  rays_traced counts primary + occlusion rays. */
typedef struct vxrt_ao_params {
  uint32_t spp;      /* occlusion rays per hit, 1..4096 */
  float radius;      /* tmax of the occlusion rays, > 0 */
  uint32_t seed;     /* user seed mixed into the per-sample WangHash seed */
  uint32_t reserved;
} vxrt_ao_params_t;
int vxrt_render_ao(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                   const vxrt_shade_params_t* params, const vxrt_ao_params_t* ao, uint32_t* dst, float* colors,
                   uint32_t* unoccluded, unsigned long long* rays_traced, void* stream);

/* vxrt_render_ao seen from `cam` (see vxrt_camera_t): orc_render_ao with the pinhole ray of pixel (x, y) in place of the fixed
 * GenerateRay and everything else unchanged -- the seed WangHash((x + y * W) * spp + s + 1 + seed * 0x9E3779B9), the view
 * direction (that ray's direction) the normal is turned against, the 1e-3 push along the facing normal, tmax = radius, any-hit,
 * pixel = Lambert colour of the primary hit x unoccluded / spp, rays_traced = primary + occlusion rays.  `cam` is a host pointer
 * read during the call; no host synchronisation is added to what vxrt_render_ao does.  Returns -1 before anything is launched
 * (dst untouched) for a null camera, a camera field that is not finite, a stale accel, and whatever vxrt_render_ao refuses.  There
 * is no batch form, no interleaved form and no counting build. */
int vxrt_render_ao_camera(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                          const vxrt_shade_params_t* params, const vxrt_ao_params_t* ao, uint32_t* dst, float* colors /* optional */,
                          uint32_t* unoccluded /* optional */, unsigned long long* rays_traced /* optional */, void* stream);

/* One diffuse bounce (extension for BASELINE config 3, "1 bounce diffuse"; absent from the reference): per pixel with
 * a primary hit one cosine-weighted ray about the shading normal -- the vxrt_render_ao recipe with spp = 1, sample 0,
 * no tmax -- traced for its closest hit; pixel = Lambert colour of the primary hit + albedo * (Lambert colour of the
 * bounce hit | background).  Defined by oracle/rt_oracle.c:orc_render_gi, reproducible bit for bit. */
int vxrt_render_diffuse_bounce(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                               const vxrt_shade_params_t* params, uint32_t seed, uint32_t* dst, float* colors,
                               unsigned long long* rays_traced, void* stream);

/* vxrt_render_diffuse_bounce seen from `cam`: orc_render_gi with the pinhole ray of pixel (x, y) in place of the fixed GenerateRay
 * (primary ray and view direction of the bounce recipe); the bounce ray is traced for its closest hit, pixel = Lambert colour of
 * the primary hit + albedo * (Lambert colour of the bounce hit | background), rays_traced = primary + bounce rays.  Contract and
 * refusals as for vxrt_render_ao_camera, with what vxrt_render_diffuse_bounce refuses. */
int vxrt_render_diffuse_bounce_camera(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                      const vxrt_shade_params_t* params, uint32_t seed, uint32_t* dst, float* colors /* optional */,
                                      unsigned long long* rays_traced /* optional */, void* stream);

/* Path-traced frame (extension; absent from the reference): several diffuse bounces, several samples per pixel, the light sampled at
 * every vertex of the path.  vxrt_render_ao's sampling recipe, vxrt_render's occlusion ray and the shading of vxrt_shade_rays, joined
 * by per-path state.  Every + and * below is an fp32 operation without contraction, in the order written, so the frame is
 * reproducible bit for bit (tests/path_ref.py restates it).  cam == NULL: the RTU test's fixed GenerateRay, as vxrt_render uses it;
 * else the pinhole ray of vxrt_camera_t.  params->max_depth is ignored (as vxrt_render_ao and vxrt_render_diffuse_bounce ignore it):
 * the mirror arm is never followed (vxrt_render_path_frame_specular follows it: "Specular vertices" below).  For pixel (x, y) of rows [y0, y1):
 *   r_0 = the camera ray, h_0 = its closest hit; on a miss the pixel is the background and no further ray is traced.
 *   Lit(r, h) = the Lambert colour of the hit as vxrt_shade_rays computes it (term + background * reflectivity, the else arm of
 *     closest.cpp); with shadow != 0 the occlusion ray of vxrt_render is traced first (origin pushed 1e-3 along L, tmax = |L|,
 *     any-hit) and a blocked hit takes the same expression with NdotL forced to 0.   Alb(h) = texColor of the hit (closest.cpp:72-77).
 *   For sample s = 0 .. spp-1:  Lc = Lit(r_0, h_0), thr = Alb(h_0), r = r_0, h = h_0; then for k = 0 .. bounces-1:
 *     r' = the vxrt_render_ao ray of (x, y, W, spp, s) with user seed (seed + k) mod 2^32, leaving the hit point I(r, h) along the shading
 *          normal N(r, h) turned against dir(r); traced for its closest hit, no tmax.
 *     miss:   Lc = Lc + thr * background, and the path ends.
 *     hit h': Lc = Lc + thr * Lit(r', h'), then thr = thr * Alb(h'), r = r', h = h'.
 *     (the primary hit, its Lit and its Alb are computed once per pixel and shared by all samples)
 *   acc = the first sample's Lc; each later sample's Lc is added in ascending s (not from zero: 0 + (-0) would change a sign bit);
 *   colour = acc / (float)spp; pixel = the RGB8 pack of colour.
 *   rays_traced increases by the primary rays of the window + one per occlusion ray of a real hit + one per bounce ray of a live path.
 * Two identities follow: bounces = 1, spp = 1, shadow = 0 is vxrt_render_diffuse_bounce[_camera] bit for bit (colours, pixels, rays
 * traced); bounces = 0 is vxrt_render[_camera] with the same shadow on a frame rendered with max_depth = 1, for every spp whose
 * sum and division are exact (the powers of two; x + x + x divided by 3 is not always x in fp32).
 * dst, colors (optional, 3 floats per pixel of the full frame) and rays_traced (optional) as for vxrt_render.  Asynchronous on `stream`:
 * the primary pass is vxrt_render's launch, the rest runs from per-path state in the frame context's own storage (frames in flight on
 * several streams do not see each other's) in batches of whole samples (host knob VXRT_PATH_BATCH, docs/KNOBS.md); every ray count stays
 * on the device, and the host synchronises the stream only when that storage has to grow.
 * Returns -1 before anything is launched (dst untouched) for a null `path`, spp = 0 or > 4096, bounces > VXRT_PATH_MAX_BOUNCES,
 * shadow > 1, a camera field that is not finite, a stale accel, a non-zero alpha table, and whatever vxrt_render refuses for the
 * window; 0 for an empty window.  There is no batch form, no interleaved form and no counting build. */
#define VXRT_PATH_MAX_BOUNCES 16
typedef struct vxrt_path_params {
  uint32_t spp;      /* samples per pixel, 1..4096 */
  uint32_t bounces;  /* diffuse bounces after the primary hit, 0..VXRT_PATH_MAX_BOUNCES */
  uint32_t seed;     /* user seed of bounce 0; bounce k takes seed + k */
  uint32_t shadow;   /* 0 / 1: sample the light with an occlusion ray at every vertex */
} vxrt_path_params_t;
/* = vxrt_render_path_frame ("Path frames by descriptor" below) with the window, cam, params, path, dst, colors, rays_traced. */
int vxrt_render_path(vxrt_accel_t* accel, const vxrt_camera_t* cam /* NULL = fixed camera */,
                     uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                     const vxrt_shade_params_t* params, const vxrt_path_params_t* path,
                     uint32_t* dst, float* colors /* optional */,
                     unsigned long long* rays_traced /* optional */, void* stream);

/* Denoised path frame (extension; absent from the reference): vxrt_render_path at a few samples per pixel, its stochastic part passed
 * through a guided a-trous filter, and the guide buffers of the primary hit as optional outputs.  Per pixel the path frame is
 * Lc = Lit_0 + Alb_0 * (everything stochastic): Lit_0 is deterministic and Alb_0 carries the texture detail, so only the demodulated
 * indirect term E is filtered.  Every + - * / below is one fp32 operation, in the order written, without contraction (`/` is the
 * correctly rounded division; there is no exp, pow or reciprocal approximation), so the result is reproducible bit for bit
 * (tests/denoise_ref.py restates it).
 *
 * THE FILTER  F = atrous(S, P, N, prm) over a window of rows x width pixels.  S = the signal, 3 floats per pixel; P = (Ix, Iy, Iz, hit),
 * hit != 0 (a NaN included) meaning that the pixel has a primary hit; N = (Nx, Ny, Nz, ignored); prm = vxrt_denoise_params_t.
 * For iteration i = 0 .. iterations-1, with step = 1 << i and sl = sigma_l * 2^-i (one multiplication by the exact power of two), `in`
 * being S for i = 0 and the previous iteration's `out` after that, for every pixel p of the window:
 *   p is not a hit: out[p] = in[p].
 *   else sw = +0, sc = (+0, +0, +0); the taps are visited in the order dy = -2..2 (outer), dx = -2..2 (inner), q = p + step * (dx, dy).
 *   A tap is skipped if q lies outside the window (columns [0, width), the rows of the window only) or q is not a hit; the centre is a
 *   tap like any other.  For a tap that is not skipped:
 *     h  = k[dy+2] * k[dx+2], k = {1/16, 1/4, 3/8, 1/4, 1/16} (the products are exact)
 *     d  = dot(Np, Nq); dn = d > 0 ? d : +0 (so 0 for a NaN), then dn = dn * dn repeated normal_power times
 *     t  = fabsf(dot(Np, Iq - Ip)) / sigma_z;  wz = 1 / (1 + t * t)
 *     u  = fabsf(lum(in[p]) - lum(in[q])) / sl;  wc = 1 / (1 + u * u)
 *     w  = ((h * dn) * wz) * wc;  if w > 0 (false for a NaN): sw = sw + w and sc = sc + w * in[q] per channel
 *   with dot(a, b) = (ax * bx + ay * by) + az * bz and lum(c) = (0.2126f * r + 0.7152f * g) + 0.0722f * b.
 *   out[p] = sw > 0 ? sc / sw (per channel) : in[p].
 * sigma_z and sigma_l must be > 0; +inf is legal and switches the term off (x / inf = 0, weight 1).  Guide values that are not finite
 * or normals that are not unit vectors are legal input: the result is whatever the IEEE operations above give.  iterations = 0: F = S.
 *
 * THE FRAME.  With c = the colour vxrt_render_path defines for the pixel (acc / spp), D = Lit(r_0, h_0), A = Alb(h_0):
 *   demodulate   E_ch = A_ch > 0 ? (c_ch - D_ch) / A_ch : 0
 *   guides       P = (I(r_0, h_0), 1), N = (N(r_0, h_0), 0) for a pixel with a primary hit; a miss has P = 0 (so P.w = 0) and N = 0
 *   filter       F = atrous(E, P, N, dn) over the rows [y0, y1) that are rendered.  A ROW WINDOW IS ITS OWN IMAGE: taps never reach
 *                outside it, so a frame rendered in bands is not the frame rendered whole.
 *   remodulate   colour_ch = D_ch + A_ch * F_ch; a miss is the background; pixel = the RGB8 pack of colour.
 * iterations = 0 is vxrt_render_path bit for bit (no demodulation round trip).  rays_traced as for vxrt_render_path.
 * aov (optional, any member may be NULL): full-frame addressing like `colors`, rows [y0, y1) written.
 * Asynchronous on `stream` like vxrt_render_path (the host synchronises only when the frame context's storage has to grow); the two
 * signal buffers of the iterations live in the frame context, so frames in flight on several streams do not see each other's.
 * Launches after the path tail: one that demodulates and writes the guides (it takes the place of the pack), one per iteration, the
 * last of which remodulates and packs.
 * Returns -1 before anything is launched (dst untouched) for a null `dn`, iterations > VXRT_DENOISE_MAX_ITERATIONS, normal_power > 7,
 * a sigma that is <= 0 or NaN, a non-zero alpha table, and everything vxrt_render_path refuses; 0 for an empty window. */
#define VXRT_DENOISE_MAX_ITERATIONS 6
typedef struct vxrt_denoise_params {
  uint32_t iterations;    /* a-trous passes, 0..VXRT_DENOISE_MAX_ITERATIONS; pass i has stride 2^i */
  uint32_t normal_power;  /* the normal weight is max(0, dot)^(2^normal_power), 0..7 */
  float sigma_z;          /* scale of the distance of a tap's hit point from the centre's tangent plane, > 0 */
  float sigma_l;          /* scale of the luminance difference in the first pass (halved every pass), > 0 */
} vxrt_denoise_params_t;
typedef struct vxrt_path_aov {
  float* noisy;     /* 3 / pixel: vxrt_render_path's colour */
  float* direct;    /* 3 / pixel: Lit_0 | background */
  float* albedo;    /* 3 / pixel: Alb_0 | 0 */
  float* position;  /* 4 / pixel: I, hit flag (1 | 0) */
  float* normal;    /* 4 / pixel: N, 0 */
} vxrt_path_aov_t;
/* = vxrt_render_path_frame with vxrt_render_path's fields and denoise = dn (not NULL), aov. */
int vxrt_render_path_denoised(vxrt_accel_t* accel, const vxrt_camera_t* cam /* NULL = fixed camera */,
                              uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                              const vxrt_shade_params_t* params, const vxrt_path_params_t* path, const vxrt_denoise_params_t* dn,
                              uint32_t* dst, float* colors /* optional */, const vxrt_path_aov_t* aov /* optional */,
                              unsigned long long* rays_traced /* optional */, void* stream);

/* The filter alone, F = atrous(signal, position, normal, dn), on caller-owned DEVICE buffers holding a window of `rows` rows of `width`
 * pixels: signal and out 3 floats per pixel, position and normal 4 floats per pixel and 16-byte aligned.  out must not alias signal.
 * scratch: device memory of at least vxrt_denoise_scratch_bytes(width, rows) bytes, 16-byte aligned (the two (r, g, b, lum) buffers the
 * iterations alternate between; unused and may be NULL with iterations = 0).  Asynchronous on `stream`, no host synchronisation.
 * Returns -1 before anything is launched (out untouched) for a null `dn` or parameters vxrt_render_path_denoised refuses, a window of
 * 2^31 pixels or more, a null or misaligned buffer, and scratch that is too small; 0 for an empty window (width or rows = 0). */
uint64_t vxrt_denoise_scratch_bytes(uint32_t width, uint32_t rows);
int vxrt_denoise(uint32_t width, uint32_t rows, const float* signal, const float* position, const float* normal,
                 const vxrt_denoise_params_t* dn, float* out, void* scratch, uint64_t scratch_bytes, void* stream);

/* Temporal accumulation for denoised path frames (extension; absent from the reference): the demodulated indirect term E of a frame is
 * blended with the accumulated term of the previous frame, fetched where the previous CAMERA saw the pixel's primary hit.  Every
 * + - * / below is one fp32 operation in the order written, without contraction; `/` is the correctly rounded division; floorf and
 * fabsf are exact; min(a, b) = b < a ? b : a and max(a, b) = a < b ? b : a; dot(a, b) = (ax * bx + ay * by) + az * bz as in the filter.
 * The one exception is the reciprocal basis of the previous camera, which the host computes in double precision by the rule below.
 * tests/temporal_ref.py restates all of it.
 *
 * HISTORY.  A vxrt_history_t is opaque, caller-owned and independent of any accel or frame context.  For a window of rows x width
 * pixels it holds two sets of three float4 buffers (a frame reads its predecessor's neighbours while it writes its own): per set
 * HE = (E_acc.rgb, len), HP = (I, hit), HN = (N, .); 96 bytes per pixel, allocated at create.  On the host it keeps the previous
 * frame's vxrt_camera_t and geometry (W, H, y0, y1).  A history is EMPTY after create and after reset, and it counts as empty in a call
 * whose (W, H, y0, y1) differ from the stored ones: another window is an implicit reset.
 *
 * RECIPROCAL BASIS of the previous camera cam'.  With R, U, F = right, up, forward of cam' as doubles:
 *   UF = U x F, FR = F x R, RU = R x U, each component a_y * b_z - a_z * b_y (etc.) as two products and one subtraction;
 *   det = (R_x * UF_x + R_y * UF_y) + R_z * UF_z;  Rr = UF / det, Ur = FR / det, Fr = RU / det per component,
 * each rounded once to fp32 (a magnitude beyond the fp32 range becomes the infinity of its sign).  No special cases: a singular basis
 * gives infinities or NaNs, and the range tests below then reject every pixel.
 *
 * THE STEP  out = T(E, P, N; history, cam', prm) over the window; E = 3 floats per pixel, P = (I, hit) and N as for the filter, prm =
 * vxrt_temporal_params_t.  For pixel p = (x, y) of the window (frame row y0 + y), rows = y1 - y0:
 *   p is not a hit (P.w != 0 is false): out = (E, 0).
 *   else sw = +0, se = (+0, +0, +0), sl = +0, and if the history is not empty:
 *     d = I - pos' per component;  a = dot(d, Rr), b = dot(d, Ur), c = dot(d, Fr).
 *     if c > 0 (false for a NaN):
 *       fx = (((a / c) / viewplane'[0]) + 0.5f) * (float)W - 0.5f
 *       fy = ((((b / c) / viewplane'[1]) + 0.5f) * (float)H - 0.5f) - (float)y0
 *       if fx > -1 && fx < (float)W && fy > -1 && fy < (float)rows  (only now do coordinates become integers):
 *         x0 = floorf(fx), yy = floorf(fy), tx = fx - (float)x0, ty = fy - (float)yy.
 *         The four taps are visited in the order (i, j) = (0,0), (1,0), (0,1), (1,1), q = (x0 + i, yy + j).  A tap is skipped if q lies
 *         outside the window; or HP[q].w != 0 is false or HE[q].w > 0 is false; or dot(N, HN[q]) >= normal_min is false; or
 *         fabsf(dot(N, HP[q].xyz - I)) / sigma_z <= 1 is false.  For a tap that is kept:
 *           w = (i ? tx : 1 - tx) * (j ? ty : 1 - ty);  if w > 0: sw = sw + w, se = se + w * HE[q].rgb per channel, sl = sl + w * HE[q].w.
 *   if sw > 0:  Eh = se / sw per channel, L = sl / sw, L1 = min(L + 1, (float)max_len), al = max(1 / L1, alpha_min),
 *               out = (Eh + al * (E - Eh), L1)
 *   else        out = (E, 1).
 * The new history is HE = out, HP = P, HN = N, cam' = cam, with the call's geometry.  Guide values that are not finite and normals that
 * are not unit vectors are legal input: the result is whatever the operations above give.
 * Parameters: alpha_min in (0, 1]; max_len in 1..VXRT_TEMPORAL_MAX_LEN; sigma_z > 0 (+inf is legal and switches the plane test off);
 * normal_min finite.  Anything else is refused.
 *
 * THE LIMIT.  The step T follows the CAMERA alone: for an instance that moved (vxrt_accel_set_transforms) or vertices that were
 * refitted (vxrt_accel_refit) it looks the previous frame up as if the surface had stood still, and the plane and normal tests then
 * reject most of the stale history.  The step T_m further below ("Motion") follows the surface instead: it takes the previous-frame
 * position of every pixel's hit point from a snapshot of the scene (vxrt_accel_motion_snapshot).  What neither follows: the light
 * (a shadow that moves over a surface is accumulated as if it had not), and anything seen through a mirror bounce.
 * vxrt_history_reset remains the sure way after a cut.
 *
 * THE FRAME.  vxrt_render_path_temporal is vxrt_render_path_denoised with one step more: between demodulation and the first a-trous
 * pass out = T(E, P, N; history, cam', temporal) with the frame's own guides, the filter runs on out.rgb, remodulation and pack are
 * unchanged.  With dn->iterations = 0 the accumulated signal is remodulated directly: colour = D + A * out.rgb, the background for a
 * miss.  The first frame on an empty history with iterations >= 1 is therefore vxrt_render_path_denoised bit for bit.  One launch more
 * per frame; nothing else changes, no rays are traced for it and no host synchronisation is added.
 *
 * Contract of the calls below.  Asynchronous on `stream`.  Calls on one history are the caller's to order (one stream, or events);
 * histories are independent of each other and of vxrt_accel_frames_in_flight.  A call that returns -1 returns before anything is
 * launched and leaves the history, dst and out4 as they were: null pointers, a camera field that is not finite, position / normal not
 * 16-byte aligned, a window of 2^31 pixels or more, a window of more pixels than the history was created for (width * rows), bad
 * parameters, W or H = 0, y0 > y1, y1 > H.  An empty window (y0 == y1) returns 0 and leaves the history as it was. */
#define VXRT_TEMPORAL_MAX_LEN 1024
typedef struct vxrt_temporal_params {
  float alpha_min;     /* lower bound of the weight of the new frame, in (0, 1]; 1 = no accumulation */
  uint32_t max_len;    /* cap of the accumulated length, 1..VXRT_TEMPORAL_MAX_LEN */
  float sigma_z;       /* a tap is kept when its hit point lies within sigma_z of the pixel's tangent plane, > 0 */
  float normal_min;    /* a tap is kept when dot(N, N') >= normal_min; finite */
} vxrt_temporal_params_t;
typedef struct vxrt_history vxrt_history_t;
/* buffers for windows of up to width * rows pixels (96 bytes each); -1 for width or rows = 0, 2^31 pixels or more, or no memory */
int vxrt_history_create(uint32_t width, uint32_t rows, vxrt_history_t** history);
/* frees the buffers; work in flight that uses the history has to be finished (the call waits for the device) */
int vxrt_history_destroy(vxrt_history_t* history);
/* makes the history empty (host state only: nothing is launched) */
int vxrt_history_reset(vxrt_history_t* history);
/* HE of the last frame, (E_acc.rgb, len) per pixel of its window, into out4 (device, rows * width * 4 floats): one copy on `stream`.
 * -1 for an empty history (there is no window to read) or a null pointer. */
int vxrt_history_read(vxrt_history_t* history, float* out4, void* stream);
/* The step alone on caller-owned DEVICE buffers of the window (rows [y0, y1) of a W x H frame seen from `cam`): signal 3 floats per
 * pixel, position and normal 4 floats per pixel and 16-byte aligned, out4 = out, 4 floats per pixel.  `cam` and `prm` are host pointers
 * read during the call. */
int vxrt_temporal_accumulate(vxrt_history_t* history, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                             const float* signal, const float* position, const float* normal, const vxrt_temporal_params_t* prm,
                             float* out4, void* stream);
/* The frame = vxrt_render_path_frame with vxrt_render_path_denoised's fields and temporal, history (neither NULL); cam must not be
 * NULL (the fixed camera has no vxrt_camera_t). */
int vxrt_render_path_temporal(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                              const vxrt_shade_params_t* params, const vxrt_path_params_t* path, const vxrt_denoise_params_t* dn,
                              const vxrt_temporal_params_t* temporal, vxrt_history_t* history,
                              uint32_t* dst, float* colors /* optional */, const vxrt_path_aov_t* aov /* optional */,
                              unsigned long long* rays_traced /* optional */, void* stream);

/* Motion: temporal accumulation that reprojects through moved instances and refitted vertices (extension; absent from the reference).
 * The arithmetic rules are those of the temporal section above: one fp32 operation per symbol, in the order written, no contraction.
 *
 * THE SNAPSHOT.  vxrt_accel_motion_snapshot(accel, what, stream) means "the scene as it is now is the previous frame".  `what` is a mask
 * of the VXRT_REFIT_* bits: with VXRT_REFIT_INSTANCES the accel copies the scene's n_blas instance records (160 bytes each, transform
 * and invTransform included) into storage it owns; with VXRT_REFIT_GEOMETRY it also copies the n_tris tri_t vertices (36 bytes each),
 * which is legal only together with VXRT_REFIT_INSTANCES; what == 0 frees the snapshot.  A later snapshot replaces the earlier one;
 * storage is reallocated only when `what` changes.  Ordered after every call already issued on this accel, on any stream, and
 * synchronous with respect to `stream`, like vxrt_accel_refit.  The snapshot survives vxrt_accel_refit, vxrt_accel_set_transforms and
 * vxrt_accel_set_alpha_test.  Returns -1, with nothing changed, for a null or stale accel, unknown bits in `what`,
 * VXRT_REFIT_GEOMETRY without VXRT_REFIT_INSTANCES, or an allocation failure.  vxrt_accel_info(accel, 6) is the mask held (0: none);
 * vxrt_accel_bytes includes the snapshot.  The intended loop: render frame k, snapshot, move (vxrt_accel_set_transforms /
 * vxrt_accel_refit, any number of calls), render frame k + 1.
 *
 * THE PREVIOUS-POSITION GUIDE of a hit record h.  V0, V1, V2 = the snapshot's vertices of triangle h.triIdx if the snapshot holds
 * geometry, else the scene's current ones (tri_t is v0, v1, v2; the barycentrics weight v1, v2, v0 as in vxrt_shade_rays).  M' and
 * Minv' = transform and invTransform of the snapshot's record h.blasIdx & 0x7fffffff, as cell[4 * row + column].  (bx, by, bz) = h's.
 *   o_c = (V1_c * bx + V2_c * by) + V0_c * bz                                   c = x, y, z
 *   Q_c = ((M'[c][0] * o_x + M'[c][1] * o_y) + M'[c][2] * o_z) + M'[c][3]
 *   n_c = (N1_c * bx + N2_c * by) + N0_c * bz                                   N0..N2 = the CURRENT tri_ex_t normals of h.triIdx
 *   t_c = ((Minv'[0][c] * n_x + Minv'[1][c] * n_y) + Minv'[2][c] * n_z) + 0.0f * 0.0f
 *   N'  = t * (1.0f / sqrtf((t_x * t_x + t_y * t_y) + t_z * t_z))               -- vxrt_shade_rays' shading normal with Minv' for Minv
 * The guide is Q4 = (Q, 1) and N'4 = (N', 0).  A miss (h.dist == 1e30f) gives all zeros in both, and so does a record whose masked
 * blasIdx >= n_blas or whose triIdx >= n_tris: nothing is read for such a record.  Barycentrics that are not finite are legal input; the
 * result is whatever the operations give.
 * vxrt_previous_positions computes the guide for n hit records on the device -- vxrt_trace's, the `hits` output of vxrt_render, any
 * others -- into prev_position4 and prev_normal4 (4 floats per record, 16-byte aligned).  Asynchronous on `stream`.  Returns -1 before
 * anything is launched for an accel without a snapshot, a null or stale accel, a scene without triEx, and null or misaligned buffers;
 * 0 for n == 0.
 *
 * THE STEP WITH MOTION  out = T_m(E, P, N, Q, N'; history, cam', prm) is the step T with three substitutions and nothing else:
 *   d = Q.xyz - pos' replaces d = I - pos';
 *   in the normal test dot(N', HN[q]) replaces dot(N, HN[q]);
 *   in the plane test fabsf(dot(N', HP[q].xyz - Q.xyz)) / sigma_z replaces fabsf(dot(N, HP[q].xyz - I)) / sigma_z.
 * A pixel that is a hit (P.w != 0) but for which Q.w != 0 is false has no previous position and takes out = (E, 1).  The new history is
 * written as by T: HE = out, HP = P, HN = N -- the CURRENT frame's position and normal.  The history's layout, vxrt_history_t and
 * vxrt_history_read are unchanged, and the two steps may alternate on one history.  With Q = P and N' = N, T_m is T bit for bit.
 * vxrt_temporal_accumulate_motion is vxrt_temporal_accumulate with the two guides more (4 floats per pixel of the window each, 16-byte
 * aligned), under the same contract.
 *
 * THE FRAME WITH MOTION.  vxrt_render_path_temporal_motion is vxrt_render_path_temporal with T_m in place of T; Q and N' are the guide
 * of every pixel's primary hit record, computed in the launch that prepares the frame's other guides.  It refuses what that call refuses,
 * and an accel without a snapshot.  No launch, no traced ray and no host synchronisation more than vxrt_render_path_temporal.
 * prev_position (optional): Q4 per pixel, 4 floats, addressed like `colors` (pixel (x, y) of the frame at x + y * width).
 * With a snapshot taken and nothing moved the frame is NOT bit-equal to vxrt_render_path_temporal's: Q is a barycentric interpolation
 * of the vertices, I is o + d * dist, and their bits differ. */
int vxrt_accel_motion_snapshot(vxrt_accel_t* accel, uint32_t what, void* stream);
int vxrt_previous_positions(vxrt_accel_t* accel, uint32_t n, const vxrt_hit_t* hits /* device */,
                            float* prev_position4, float* prev_normal4 /* device, 16-byte aligned */, void* stream);
int vxrt_temporal_accumulate_motion(vxrt_history_t* history, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0,
                                    uint32_t y1, const float* signal, const float* position, const float* normal,
                                    const float* prev_position, const float* prev_normal, const vxrt_temporal_params_t* prm,
                                    float* out4, void* stream);
/* = vxrt_render_path_frame with vxrt_render_path_temporal's fields and motion = 1, prev_position. */
int vxrt_render_path_temporal_motion(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0,
                                     uint32_t y1, const vxrt_shade_params_t* params, const vxrt_path_params_t* path,
                                     const vxrt_denoise_params_t* dn, const vxrt_temporal_params_t* temporal, vxrt_history_t* history,
                                     uint32_t* dst, float* colors /* optional */, const vxrt_path_aov_t* aov /* optional */,
                                     float* prev_position /* optional */, unsigned long long* rays_traced /* optional */, void* stream);

/* Variance guidance: per-pixel luminance moments steer the a-trous filter (extension; absent from the reference).  The luminance
 * edge-stopping term of atrous has one global scale, halved every pass; here every pixel gets its own, from the variance of its
 * accumulated luminance (SVGF: the temporal variance where the history is long, a spatial estimate where it is short), and the variance
 * is filtered along with the signal, so later passes narrow by themselves.  The arithmetic rules are those of the temporal section: one
 * fp32 operation per symbol, in the order written, no contraction; `/` and sqrtf are correctly rounded; min / max / dot / lum as there;
 * (float) of an integer is exact for the ranges allowed.  tests/variance_ref.py restates all of it.
 *
 * A HISTORY WITH MOMENTS (vxrt_history_create_moments) is vxrt_history_create's plus one float2 buffer per set, HM = (m1, m2): 112 bytes
 * per pixel.  The two kinds do not mix: vxrt_temporal_accumulate[_motion] and vxrt_render_path_temporal[_motion] return -1 for a history
 * with moments (its moments would silently go stale), the calls of this section return -1 for one without.  vxrt_history_destroy,
 * vxrt_history_reset and vxrt_history_read work on both.  vxrt_history_read_moments copies HM of the last frame's window, 2 floats per
 * pixel; -1 for an empty history, one without moments or a null pointer.
 *
 * THE STEP WITH MOMENTS  T_v is the step T (given both motion guides: T_m) with additions and nothing else changed.  lE = lum(E) of the
 * pixel's input signal; s1 = s2 = +0.
 *   for every tap that T keeps and whose w > 0, right after sl = sl + w * HE[q].w:  s1 = s1 + w * HM[q].x,  s2 = s2 + w * HM[q].y
 *   if sw > 0:  M1 = s1 / sw, M2 = s2 / sw,  m1 = M1 + al * (lE - M1),  m2 = M2 + al * (lE * lE - M2)
 *   else, a hit pixel:  m1 = lE, m2 = lE * lE   (an empty history, a pixel behind the previous camera or outside its view, no tap kept,
 *                                                a motion pixel for which Q.w != 0 is false)
 *   a pixel that is not a hit:  m1 = m2 = +0
 * The new history is that of T plus HM = (m1, m2); out = (E_acc, len) is bit for bit what T / T_m give on a history without moments fed
 * the same frames.  The temporal variance of a pixel is vt = max(m2 - m1 * m1, 0).
 * vxrt_temporal_accumulate_moments has the contract of vxrt_temporal_accumulate_motion; prev_position and prev_normal are both NULL (T_v
 * over T) or both set (T_v over T_m), one of the two NULL returns -1.
 *
 * THE INITIAL VARIANCE  V0 of the history's current set: A = HE = (E_acc, len), HM, HP, HN as the step just wrote them; dn =
 * vxrt_denoise_params_t (normal_power and sigma_z are used), vp = vxrt_variance_params_t.  For pixel p of the window:
 *   p is not a hit: V0 = 0.     A[p].w >= (float)min_len: V0 = vt.
 *   else sw = s1 = s2 = +0; the taps are visited in the order dy = -radius..radius (outer), dx = -radius..radius (inner), q = p + (dx, dy).
 *   A tap outside the window or not a hit is skipped; the centre is a tap like any other.  For a tap that is not skipped:
 *     dn = the filter's normal weight of (Np, Nq): max(dot, +0) squared normal_power times
 *     t = fabsf(dot(Np, Pq - Pp)) / sigma_z;  wz = 1 / (1 + t * t);  w = dn * wz
 *     if w > 0:  l = lum(A[q].rgb),  sw = sw + w,  s1 = s1 + w * l,  s2 = s2 + w * (l * l)
 *   if sw > 0:  a1 = s1 / sw,  vs = max(s2 / sw - a1 * a1, 0),  V0 = vs * ((float)min_len / A[p].w)
 *   else V0 = vt.
 * vxrt_history_variance writes V0 of the last frame's window, 1 float per pixel: one launch, no host synchronisation; -1 for an empty
 * history, one without moments, bad parameters or a null pointer.
 *
 * THE VARIANCE-GUIDED FILTER  (F, VF) = atrous_v(S, V, P, N, dn, vp); S, P, N, dn as for atrous, V one float per pixel.  For iteration i,
 * step = 1 << i, in / vin = the previous iteration's outputs (S / V for i = 0):
 *   p is not a hit: out[p] = in[p], vout[p] = vin[p].
 *   else the prefiltered variance: gw = gs = +0; dy = -1..1 (outer), dx = -1..1 (inner), q = p + (dx, dy) -- stride 1 whatever step is; a
 *   tap outside the window or not a hit is skipped; c = kk[dy+1] * kk[dx+1], kk = {1/4, 1/2, 1/4}; gw = gw + c, gs = gs + c * vin[q].
 *     g = gs / gw;  den = sigma_l * sqrtf(g) + epsilon      (sigma_l is NOT halved per pass here: the variance shrinks instead)
 *   then the 25 taps of atrous, in its order and with its skips, with u = fabsf(lum(in[p]) - lum(in[q])) / den in place of the division
 *   by sl; w = ((h * dn) * wz) * wc as there; if w > 0: sw = sw + w, sc = sc + w * in[q] per channel, sv = sv + (w * w) * vin[q] (sv from +0).
 *   if sw > 0: out[p] = sc / sw, vout[p] = sv / (sw * sw); else out[p] = in[p], vout[p] = vin[p].
 * A NaN or negative variance is legal input: the result is whatever the operations give (sqrtf of a negative is NaN, and every tap of
 * that pixel is then dropped).  vxrt_denoise_variance has the contract of vxrt_denoise; variance: device, 1 float per pixel; out_variance
 * (optional) receives VF and must not alias variance.  iterations = 0: out and out_variance are copies of signal and variance.
 *
 * THE FRAME.  vxrt_render_path_variance with motion = 0 is vxrt_render_path_temporal with T_v in place of T, with motion = 1
 * vxrt_render_path_temporal_motion with T_v in place of T_m; after the step one launch writes V0, and atrous_v runs on (out.rgb, V0);
 * remodulation and pack are unchanged and stay in the last pass.  With dn->iterations = 0 no variance is computed, except into `variance`
 * if that output is asked for, and the frame is vxrt_render_path_temporal[_motion] bit for bit: pixels, colours, rays traced and HE.
 * variance (optional): V0, 1 float per pixel, addressed like `colors`.  It refuses what that call refuses, and: bad vp, a history
 * without moments, motion > 1, motion = 0 with a non-null prev_position -- before anything is launched, the history and dst left as
 * they were.  One launch more than the temporal frame, no traced ray and no host synchronisation more. */
typedef struct vxrt_variance_params {
  float epsilon;      /* added to the luminance scale of a tap, > 0 and finite */
  uint32_t min_len;   /* accumulated lengths below this take the spatial estimate, 1..VXRT_TEMPORAL_MAX_LEN */
  uint32_t radius;    /* half width of the spatial estimate's window, 1..3 */
  uint32_t reserved;  /* 0 */
} vxrt_variance_params_t;
int vxrt_history_create_moments(uint32_t width, uint32_t rows, vxrt_history_t** history);
int vxrt_history_read_moments(vxrt_history_t* history, float* out2, void* stream);
int vxrt_temporal_accumulate_moments(vxrt_history_t* history, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0,
                                     uint32_t y1, const float* signal, const float* position, const float* normal,
                                     const float* prev_position /* or NULL */, const float* prev_normal /* or NULL */,
                                     const vxrt_temporal_params_t* prm, float* out4, void* stream);
int vxrt_history_variance(vxrt_history_t* history, const vxrt_denoise_params_t* dn, const vxrt_variance_params_t* vp,
                          float* variance /* device, 1 float per pixel of the window */, void* stream);
uint64_t vxrt_denoise_variance_scratch_bytes(uint32_t width, uint32_t rows);
int vxrt_denoise_variance(uint32_t width, uint32_t rows, const float* signal, const float* variance, const float* position,
                          const float* normal, const vxrt_denoise_params_t* dn, const vxrt_variance_params_t* vp, float* out,
                          float* out_variance /* optional */, void* scratch, uint64_t scratch_bytes, void* stream);
/* = vxrt_render_path_frame with vxrt_render_path_temporal's fields and variance = vp (not NULL), variance_out = variance, motion
 * (outside {0, 1}: refused), prev_position. */
int vxrt_render_path_variance(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                              const vxrt_shade_params_t* params, const vxrt_path_params_t* path, const vxrt_denoise_params_t* dn,
                              const vxrt_temporal_params_t* temporal, const vxrt_variance_params_t* vp, vxrt_history_t* history,
                              int motion, uint32_t* dst, float* colors /* optional */, const vxrt_path_aov_t* aov /* optional */,
                              float* prev_position /* optional, motion only */, float* variance /* optional */,
                              unsigned long long* rays_traced /* optional */, void* stream);

/* Adaptive sampling: path frames that take a sample count per pixel from a device buffer, and the kernel that derives such counts from a
 * variance buffer (extension; absent from the reference).  With both, the loop "render, take V0, derive the next frame's counts,
 * render" runs on one stream without a host synchronisation.  tests/adaptive_ref.py restates all of it.
 *
 * THE FRAME WITH COUNTS.  counts: device, one uint32_t per pixel of the full frame, addressed like dst (counts[x + y * W]); only rows
 * [y0, y1) are read, and the host never reads the buffer.  For a pixel p with a primary hit n_p = min(max(counts[p], 1), path->spp): path->spp
 * (1..4096) is the cap, and a value out of range is clamped on the device, not refused.  A pixel whose primary ray misses ignores its
 * count and is the background.  The pixel is then exactly what vxrt_render_path defines for it with spp := n_p, everywhere that
 * definition uses spp:
 *   the bounce ray is the vxrt_render_ao ray of (x, y, W, n_p, s) -- the hash seed is (x + y * W) * n_p + s + 1 + ... in uint32 arithmetic;
 *   the samples s = 0 .. n_p - 1 are summed in ascending s, starting from the first;
 *   colour = acc / (float)n_p;   with bounces = 0: the flat sum of Lit_0, n_p times, divided by n_p.
 * rays_traced follows vxrt_render_path's rule: the primary rays + one per occlusion ray of a real hit + one per bounce ray of a live path.
 * Two identities follow (both are tests):
 *   UNIFORM  counts[p] == path->spp everywhere is vxrt_render_path bit for bit: pixels, colours, rays traced.
 *   MOSAIC   a pixel's value depends on its own n_p only: the frame is, pixel by pixel, the vxrt_render_path frame with spp = n_p of that pixel.
 * vxrt_render_path_variance_adaptive is vxrt_render_path_variance with c, the path frame's colour that demodulation starts from, taken
 * from the frame with counts; nothing else of its definition changes (with counts[p] == path->spp everywhere it is that call bit for
 * bit, HE and HM of the history included; dn->iterations = 0 follows that call's own rule).
 * Both return -1 before anything is launched, dst and the history left as they were, for a null `counts` and for everything the call
 * without counts refuses (a non-zero alpha table included); 0 for an empty window.  Asynchronous on `stream`.  The samples are traced in
 * batches of VXRT_PATH_BATCH consecutive paths of the frame (docs/KNOBS.md), pixels in window order, whatever the counts: per-path
 * storage is bounded by the batch, 8 bytes per path more than vxrt_render_path's, and 12 bytes per pixel of the window for the counts
 * and their 64-bit offsets.  The number of paths stays on the device.
 *
 * COUNTS FROM A VARIANCE.  vxrt_sample_counts is elementwise over n entries; the caller owns the addressing (vxrt_history_variance writes
 * window-addressed, the frame's `variance` output is frame-addressed; with y0 = 0, y1 = H they coincide).  Every symbol is one fp32
 * operation in the order written, ceilf is exact.  For entry i:
 *   m = prev_counts ? (float)min(max(prev_counts[i], 1), 4096) : 1.0f
 *   x = (variance[i] * m) * gain;   c = ceilf(x)
 *   counts[i] = c > (float)min_spp ? (c < (float)max_spp ? (uint32_t)c : max_spp) : min_spp
 * so a NaN gives min_spp (both comparisons are false), +inf gives max_spp, negatives and -0 give min_spp.  The factor m is a HEURISTIC:
 * the variance of the mean of m samples, times m, is about the variance of one sample -- V0 of a frame rendered with prev_counts is
 * roughly that of a mean, blended over the history's frames; nothing here claims more than "about".
 * *total (optional, device) increases by the sum of the counts written (64-bit integer adds, exact in any order), which a caller can
 * read back now and then to set gain against a budget.  One launch, asynchronous on `stream`, no host synchronisation.  Returns -1
 * before the launch for a null variance / counts / prm, gain not > 0 or not finite, min_spp = 0 or > max_spp, max_spp > 4096,
 * reserved != 0, n >= 2^31; 0 for n = 0. */
typedef struct vxrt_sample_count_params {
  float gain;        /* samples per unit of per-sample variance, > 0 and finite */
  uint32_t min_spp;  /* 1 .. max_spp */
  uint32_t max_spp;  /* min_spp .. 4096 */
  uint32_t reserved; /* 0 */
} vxrt_sample_count_params_t;
/* = vxrt_render_path_frame with vxrt_render_path's / vxrt_render_path_variance's fields and counts (not NULL). */
int vxrt_render_path_adaptive(vxrt_accel_t* accel, const vxrt_camera_t* cam /* NULL = fixed camera */,
                              uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                              const vxrt_shade_params_t* params, const vxrt_path_params_t* path /* spp: the cap */,
                              const uint32_t* counts /* device, 1 per pixel of the frame */, uint32_t* dst, float* colors /* optional */,
                              unsigned long long* rays_traced /* optional */, void* stream);
int vxrt_render_path_variance_adaptive(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                       const vxrt_shade_params_t* params, const vxrt_path_params_t* path /* spp: the cap */,
                                       const uint32_t* counts /* device, 1 per pixel of the frame */, const vxrt_denoise_params_t* dn,
                                       const vxrt_temporal_params_t* temporal, const vxrt_variance_params_t* vp, vxrt_history_t* history,
                                       int motion, uint32_t* dst, float* colors /* optional */, const vxrt_path_aov_t* aov /* optional */,
                                       float* prev_position /* optional, motion only */, float* variance /* optional */,
                                       unsigned long long* rays_traced /* optional */, void* stream);
int vxrt_sample_counts(uint64_t n, const float* variance /* device */, const uint32_t* prev_counts /* device, optional */,
                       const vxrt_sample_count_params_t* prm, uint32_t* counts /* device */,
                       unsigned long long* total /* device, optional: incremented */, void* stream);

/* Emissive geometry: area lights in path frames (extension; absent from the reference, whose material_info_t::emissive nothing reads).
 * Two forms of one estimator: emission found by the bounce rays (nee = 0, brute force) and emitter sampling from a device-side table
 * (nee = 1, next-event estimation).  Every entry point that existed before ignores `emissive`, as it always has.  tests/emissive_ref.py
 * restates all of it.  Every symbol below is one fp32 operation in the order written, without contraction: IEEE add / mul / div / sqrt
 * only, pi = 3.14159265f.
 *
 * THE EMITTER TABLE.  An emitter is a pair (blasIdx, triIdx): triangle triIdx of the scene's tri buffer as instance record blasIdx
 * places it, of a material with a positive emissive component (r > 0 || g > 0 || b > 0).  The CALLER lists the pairs: the reference
 * formats store an instance's triangle range nowhere, so the accel cannot derive them, and that the list is complete -- every emissive
 * triangle of every instance, each once -- is the caller's contract: a triangle that is left out still emits for nee = 0 and is dark
 * for nee = 1.  pairs: HOST, n entries.  For entry e, on the device:
 *   V_k = ((m[0] * x + m[1] * y) + m[2] * z) + m[3] per row m of the record's `transform`, for the triangle's vertices k = 0, 1, 2 (the
 *         refit's TransformPosition);   V0 = V_0, E1 = V_1 - V_0, E2 = V_2 - V_0;   Le = the material's emissive
 *   c = cross(E1, E2) = (E1.y * E2.z - E1.z * E2.y, E1.z * E2.x - E1.x * E2.z, E1.x * E2.y - E1.y * E2.x)
 *   area = 0.5f * sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z);   w_e = area * max(max(Le.r, Le.g), Le.b)
 *   wmax = the maximum of w over the table (exact in any order);   q_e = max(1, (uint32_t)((w_e / wmax) * 65535.0f))
 *   cum_e = q_0 + .. + q_e in uint32 (at most 65536 * 65535: no wrap), Q = cum_{n-1}
 * so the table is the same bits whatever order the scan takes: integers are what the quantisation is for.  Emitter e is chosen with
 * probability q_e / Q.  Ordered after every call already issued on the accel, on any stream, and synchronous with respect to `stream`,
 * like vxrt_accel_set_alpha_test.  pairs == NULL or n == 0 drops the table.  Returns -1 with the previous table kept for a null or
 * stale accel, a scene without triEx / mat, n > VXRT_MAX_EMITTERS, blasIdx >= n_blas or triIdx >= n_tris, a pair whose material is not
 * emissive, a vertex or transform that is not finite, and an area or weight that is zero or not finite.
 * The table holds WORLD-SPACE data: a vxrt_accel_refit (what != 0) or vxrt_accel_set_transforms that succeeds makes it STALE, and it
 * stays stale until it is set again.  vxrt_accel_info(accel, 7) is the number of emitters of a valid table, 0 for none or a stale one;
 * vxrt_accel_bytes counts the 56 bytes per entry the accel holds.  vxrt_accel_read_emitters (test / diagnostic; synchronous) copies a
 * valid table to HOST memory: tri12[12 e ..] = V0, E1, E2, Le; q[e]; cum[e] (any of the three may be NULL); -1 without a valid table. */
typedef struct { uint32_t blasIdx, triIdx; } vxrt_emitter_t;
#define VXRT_MAX_EMITTERS 65536u
int vxrt_accel_set_emitters(vxrt_accel_t* accel, const vxrt_emitter_t* pairs /* HOST, or NULL */, uint32_t n, void* stream);
int vxrt_accel_read_emitters(vxrt_accel_t* accel, float* tri12 /* HOST, n x 12 */, uint32_t* q /* HOST */, uint32_t* cum /* HOST */, void* stream);

/* THE EMITTER RAY of a surface point I with the shading normal N' that faces the viewer, from hash output `seed` (0 becomes 1) and the
 * table (n entries, Q), xorshift = the three shifts of common.h:137-147, random_float = xorshift then (float)state * 2.3283064365387e-10f:
 *   r0 = xorshift(state) as uint32;  a = random_float;  b = random_float
 *   t = ((uint64_t)r0 * Q) >> 32;  e = the smallest index with cum_e > t (a binary search over [0, n-1] of at most 17 steps)
 *   if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }      P = (V0 + a * E1) + b * E2
 *   o = I + N' * 0.001f (the bounce ray's origin);  v = P - o;  d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;  d = sqrtf(d2);  w = v / d
 *   tmax = d - 0.001f, any-hit
 *   cosx = max(0, (N'.x * w.x + N'.y * w.y) + N'.z * w.z)      (std::max: a NaN gives 0)
 *   an = 0.5f * |(c.x * w.x + c.y * w.y) + c.z * w.z| with c = cross(E1, E2) as above: the emitter's projected area, both sides emit
 *   G = (((Le * scale) * cosx) * an) / ((3.14159265f * d2) * ((float)q_e / (float)Q)) per channel
 * SKIPPED, i.e. not traced, not counted and without a contribution, if cosx == 0, d2 == 0 or a channel of G is not finite.
 * vxrt_emitter_rays runs this step alone on caller-owned DEVICE buffers: points = n x 6 floats (I, N'), seeds = n hash outputs;
 * rays (n x 6: o, w), tmax (n), weight3 (n x 3: G), emitter (n: e) -- a skipped entry gets the ray (0,0,0; 1,1,1), tmax = -1 and
 * G = 0, its e is still the one chosen.  One launch, asynchronous on `stream`.  Returns -1 before the launch for a null or stale accel,
 * no valid table, a null buffer, scale negative or not finite, n >= 2^31; 0 for n = 0.
 *
 * THE FRAME.  vxrt_render_path_emissive is vxrt_render_path -- the point light, `shadow`, the batches of VXRT_PATH_BATCH, every count on
 * the device, no host synchronisation unless a buffer grows -- with, for Emi(h) = emissive(material of h) * scale where that material
 * has a positive emissive component (elsewhere NOTHING is added, not a zero: -0 + 0 would change a sign bit):
 *   both modes:  Lc starts as Lit(r_0, h_0) + Emi(h_0), formed once per pixel in the prepare launch (bounces = 0: the flat sum of that).
 *   nee = 0, at bounce k:  hit h': Lc = Lc + thr * Lit(r', h'), then Lc = Lc + thr * Emi(h'), then thr = thr * Alb(h').
 *   nee = 1, at bounce k, before the miss / hit arm of vxrt_render_path (no emission is added at bounce hits):  the emitter ray of
 *     (I(r, h), N'(r, h)) with seed = WangHash((x + y * W) * spp + s + 1 + u * 0x9E3779B9), u = ((seed + k) mod 2^32) ^ 0x80000000 -- the
 *     bounce ray's hash input with a user seed no bounce of the frame takes -- is traced unless skipped; unblocked: Lc = Lc + thr * G,
 *     thr as the vertex has it (Alb(h) included).  So every vertex a bounce ray leaves sends one emitter ray, the last vertex none, and
 *     E[nee = 1] = E[nee = 0] for the same `bounces`.
 *   rays_traced also counts the emitter rays that were traced.
 * Returns -1 before anything is launched (dst untouched) for whatever vxrt_render_path refuses (a non-zero alpha table included), a
 * null `em`, nee > 1, a non-zero reserved word, scale negative or not finite, and nee = 1 without a valid table (none set, or stale).
 * The denoised, temporal, variance and adaptive forms of this frame are vxrt_render_path_frame's: "Path frames by descriptor" below.
 * The two forms combined by multiple importance sampling are entry points of their own: "Multiple importance sampling" below. */
typedef struct vxrt_emissive_params {
  uint32_t nee;          /* 0: emission at bounce hits; 1: emitter sampling from the accel's table */
  float scale;           /* multiplies every material's emissive; >= 0 and finite */
  uint32_t reserved[2];  /* 0 */
} vxrt_emissive_params_t;
/* = vxrt_render_path_frame with vxrt_render_path's fields and emissive = em (not NULL). */
int vxrt_render_path_emissive(vxrt_accel_t* accel, const vxrt_camera_t* cam /* NULL = fixed camera */,
                              uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                              const vxrt_shade_params_t* params, const vxrt_path_params_t* path, const vxrt_emissive_params_t* em,
                              uint32_t* dst, float* colors /* optional */, unsigned long long* rays_traced /* optional */, void* stream);
int vxrt_emitter_rays(vxrt_accel_t* accel, uint64_t n, const float* points /* device, n x 6: I, N' */, const uint32_t* seeds /* device */,
                      float scale, float* rays /* device, n x 6 */, float* tmax /* device */, float* weight3 /* device, n x 3 */,
                      uint32_t* emitter /* device */, void* stream);

/* Multiple importance sampling of area lights (extension): the two estimators of "Emissive geometry" in one frame, each weighted by the
 * balance heuristic, so that a sample is bounded by the emitter's radiance where nee = 1 has the unbounded G (a vertex next to a large
 * emitter) and the frame keeps nee = 1's error where nee = 0 needs many samples (small, far emitters).  The conventions are those of
 * "Emissive geometry": every symbol one fp32 IEEE operation in the order written, no contraction, pi = 3.14159265f.
 * tests/emissive_mis_ref.py restates all of it.
 * One direction w from a vertex with facing normal N' has two solid-angle densities: cosx / pi for the bounce ray (cosine-weighted about
 * N') and d2 * (q_e / Q) / an for the emitter ray.  Both weights below are the balance heuristic with numerator and denominator
 * multiplied by an, so nothing is divided by an and a sample in the emitter's own plane (an = 0) stays defined.
 *
 * THE EMITTER-RAY SIDE, with d2, cosx, an, q_e, Q and G of THE EMITTER RAY above:
 *   qf = (float)q_e / (float)Q;   pe = d2 * qf;   pb = (cosx / pi) * an;   wE = pe / (pe + pb);   Gm = G * wE per channel
 * SKIPPED as the emitter ray is, and also if a channel of Gm is not finite.  Mathematically Gm <= Le * scale.
 * vxrt_emitter_rays_mis is vxrt_emitter_rays with weight3 = Gm and one output more, mis (n: wE); a skipped entry gets Gm = 0 and
 * wE = 0.  It refuses what vxrt_emitter_rays refuses, and a null `mis`.
 *
 * THE BOUNCE-RAY SIDE.  A bounce ray (o, w), as stored, that left a vertex with facing normal N' hits h' at distance t, and
 * (h'.blasIdx & 0x7fffffff, h'.triIdx) is entry e of the table; with c = cross(E1, E2) of entry e and qf of entry e as above:
 *   cosx = max(0, (N'.x * w.x + N'.y * w.y) + N'.z * w.z)      (std::max: a NaN gives 0)
 *   an = 0.5f * |(c.x * w.x + c.y * w.y) + c.z * w.z|
 *   pe = (t * t) * qf;   pb = (cosx / pi) * an;   den = pe + pb;   wB = den > 0 ? pb / den : 1
 * A triangle that is not in the table has wB = 1: the caller's contract is unchanged, a triangle left out of the list keeps emitting
 * through bounce rays at full weight.
 * THE EMITTER INDEX finds e: the table's (blasIdx, triIdx, e), 12 bytes per entry, sorted ascending by (blasIdx, triIdx) and, for a pair
 * listed more than once, by e -- so the order is unique.  The lookup takes the smallest position whose key is not below the wanted key
 * (a binary search over [0, n-1] of at most 17 steps) and has found it if the key there is equal; of a pair listed twice it finds
 * the smaller e.  The index holds no world-space data.  It is built when it is first needed after a vxrt_accel_set_emitters -- the first
 * vxrt_render_path_emissive_mis or vxrt_emitter_hit_weights -- from the pair list the accel kept, sorted on the host and uploaded once:
 * that call synchronises `stream` once, like a call whose buffers grow.  From then on vxrt_accel_bytes counts its 12 bytes per entry and
 * vxrt_accel_info(accel, 8) is its entry count (0: none); vxrt_accel_set_emitters drops it.
 * vxrt_emitter_hit_weights runs the lookup and wB alone on caller-owned DEVICE buffers: rays (n x 6: o, w), hits (n records as vxrt_trace
 * writes them; dist is t), normals (n x 3: N') -> emitter (n: e, or 0xFFFFFFFF for a pair that is not listed) and mis (n: wB).  Every
 * record is looked up, whether its material emits or not and whatever its dist.  One launch, asynchronous on `stream` (behind the index's
 * build, if this call is the one that builds it).  Returns -1 before the launch for a null or stale accel, no valid table, a null
 * buffer, n >= 2^31; 0 for n = 0.
 *
 * THE FRAME.  vxrt_render_path_emissive_mis is vxrt_render_path_emissive with nee = 1 -- the same emitter ray per vertex, the same seeds,
 * the same any-hit launch, the same rays_traced -- except that
 *   an unblocked emitter ray adds Lc = Lc + thr * Gm, and
 *   at every bounce hit h' whose material emits, after Lc = Lc + thr * Lit(r', h') (where nee = 0 adds thr * Emi(h')):
 *     Lc = Lc + thr * (Emi(h') * wB) per channel, with N' = the normal of the vertex the bounce ray left, turned against the direction the
 *     path arrived from as the bounce ray's own sampling turns it, w = the bounce ray's direction, t = h'.dist.
 * Emi(h_0) at the primary hit stays at full weight.  Every vertex a bounce ray leaves sends an emitter ray, so every bounce hit is
 * weighted, wE + wB = 1 for one direction up to rounding, and the expectation is that of both forms of "Emissive geometry".  With
 * bounces = 0 the frame is that of nee = 1.
 * Returns -1 before anything is launched (dst untouched) for whatever vxrt_render_path_emissive with nee = 1 refuses (a non-zero alpha
 * table, a missing or stale emitter table included), a null `em`, a non-zero reserved word, scale negative or not finite. */
typedef struct vxrt_emissive_mis_params {
  float scale;           /* multiplies every material's emissive; >= 0 and finite */
  uint32_t reserved[3];  /* 0 */
} vxrt_emissive_mis_params_t;
/* = vxrt_render_path_frame with vxrt_render_path's fields and emissive_mis = em (not NULL). */
int vxrt_render_path_emissive_mis(vxrt_accel_t* accel, const vxrt_camera_t* cam /* NULL = fixed camera */,
                                  uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                  const vxrt_shade_params_t* params, const vxrt_path_params_t* path, const vxrt_emissive_mis_params_t* em,
                                  uint32_t* dst, float* colors /* optional */, unsigned long long* rays_traced /* optional */, void* stream);
int vxrt_emitter_rays_mis(vxrt_accel_t* accel, uint64_t n, const float* points /* device, n x 6: I, N' */, const uint32_t* seeds /* device */,
                          float scale, float* rays /* device, n x 6 */, float* tmax /* device */, float* weight3 /* device, n x 3: Gm */,
                          uint32_t* emitter /* device */, float* mis /* device, n: wE */, void* stream);
int vxrt_emitter_hit_weights(vxrt_accel_t* accel, uint64_t n, const float* rays /* device, n x 6 */, const void* hits /* device, n records */,
                             const float* normals /* device, n x 3: N' */, uint32_t* emitter /* device */, float* mis /* device, n: wB */,
                             void* stream);

/* Path frames by descriptor (extension): every path frame above, and the combinations no entry point above can name, through one call.
 * The descriptor names what the frame is made of; a null part is absent.  The frame is a COMPOSITION of the sections above, and the
 * meaning of every field is that of the argument of the same name of the entry points above:
 *   path alone                              vxrt_render_path                       + counts               vxrt_render_path_adaptive
 *   + denoise (aov optional)                vxrt_render_path_denoised              + emissive             vxrt_render_path_emissive
 *   + temporal, history                     vxrt_render_path_temporal              + emissive_mis         vxrt_render_path_emissive_mis
 *   + motion = 1 (prev_position optional)   vxrt_render_path_temporal_motion
 *   + variance (variance_out optional)      vxrt_render_path_variance, + counts: vxrt_render_path_variance_adaptive
 * and a descriptor that sets exactly the parts of one of these entry points IS that entry point, bit for bit: pixels, colours, guide
 * outputs, the history's contents, rays traced (each is a test).  tests/path_frame_ref.py restates the compositions below from the
 * restatements of the sections they are made of.  Only three things are new:
 *
 * EMITTER FORM x COUNTS.  Pixel p with n_p = min(max(counts[p], 1), path->spp) is exactly the vxrt_render_path_emissive /
 * vxrt_render_path_emissive_mis pixel with spp := n_p, everywhere that definition uses spp -- the emitter ray's hash input
 * (x + y * W) * n_p + s + 1 + u * 0x9E3779B9, u = ((seed + k) mod 2^32) ^ 0x80000000, included.  rays_traced also counts the emitter
 * rays that were traced.  UNIFORM and MOSAIC of "Adaptive sampling" hold as stated there, against the emissive frames.
 *
 * EMITTER FORM x FILTER.  D, the deterministic term that demodulation subtracts and the `direct` guide reports, is Lit_0 + Emi(h_0) as
 * the prepare launch forms it: where the material of h_0 does not emit NOTHING is added (the -0 rule of "Emissive geometry").  The
 * stochastic term (c - D) / A then carries the emitter rays of h_0 -- whose thr is Alb_0 -- as well as the indirect light.  Nothing else
 * of "Denoised path frames", "Temporal accumulation", "Motion" or "Variance guidance" changes.
 *
 * EMITTER TABLE x MOTION.  The table is world-space and goes stale with every vxrt_accel_set_transforms / vxrt_accel_refit, as ever: a
 * frame with nee = 1 or emissive_mis after a move needs vxrt_accel_set_emitters again, and is refused until then.  The motion snapshot
 * does not follow the emitters' own motion: as for the point light, a moved lamp changes the signal and the history follows it at the
 * rate alpha allows.
 *
 * Returns -1 before anything is launched -- dst, the guide outputs and the history untouched, vxrt_status unchanged -- for a null
 * `frame`, size != sizeof(vxrt_path_frame_t), a non-zero reserved word, emissive and emissive_mis both set, motion > 1, prev_position
 * without motion, variance_out without variance, aov / temporal / history / motion / variance without denoise, and for everything the
 * entry point of the same combination refuses: a null path / params / dst, a bad window or camera, temporal without history or the
 * reverse, a history of the wrong kind (moments iff variance) or too small, motion or variance without temporal, motion without a
 * snapshot, bad parameters of any part, a non-zero alpha table, a stale accel, nee = 1 / emissive_mis without a valid table.  0 for an
 * empty window.  Asynchronous on `stream` as the entry points above; a counts frame with nee = 1 / emissive_mis holds 68 bytes more per
 * path of a batch (VXRT_PATH_BATCH, docs/KNOBS.md) for the emitter rays. */
typedef struct vxrt_path_frame {
  uint32_t size;                                   /* sizeof(vxrt_path_frame_t) */
  uint32_t width, height, y0, y1;
  uint32_t motion;                                 /* 0 / 1 */
  const vxrt_camera_t* cam;                        /* NULL = fixed camera */
  const vxrt_shade_params_t* params;
  const vxrt_path_params_t* path;                  /* with counts: spp is the cap */
  const vxrt_emissive_params_t* emissive;          /* at most one of these two */
  const vxrt_emissive_mis_params_t* emissive_mis;
  const uint32_t* counts;                          /* device, addressed like dst; optional */
  const vxrt_denoise_params_t* denoise;            /* optional; the rest of the chain needs it */
  const vxrt_path_aov_t* aov;
  const vxrt_temporal_params_t* temporal;          /* temporal and history: both or neither */
  vxrt_history_t* history;
  const vxrt_variance_params_t* variance;          /* needs temporal and a history with moments */
  uint32_t* dst;
  float* colors;                                   /* optional */
  float* prev_position;                            /* optional, motion only */
  float* variance_out;                             /* optional, variance only */
  unsigned long long* rays_traced;                 /* optional */
  uint32_t reserved[4];                            /* 0 */
} vxrt_path_frame_t;
int vxrt_render_path_frame(vxrt_accel_t* accel, const vxrt_path_frame_t* frame, void* stream);

/* Specular vertices (extension): path frames that follow blas_node_t::reflectivity, as vxrt_render[_camera] follow the reference's mirror
 * arm.  Above, "the mirror arm is never followed": a reflective instance shows term + background * reflectivity.  Here a path vertex can
 * be specular, and a lobe pick decides per sample whether the path leaves it along the mirror ray or along the diffuse bounce ray.
 * Everything is "Path-traced frame" / "Emissive geometry" / "Multiple importance sampling" / "Adaptive sampling" as written, except what
 * follows; every + and * is one fp32 operation without contraction, as ever.  tests/specular_ref.py restates all of it.
 *
 * rho(h) is the `reflectivity` of the hit instance.  A vertex h is SPECULAR iff rho(h) > 0 and rho(h) is finite: NaN, +-inf and
 * rho <= 0 are not specular and behave exactly as above.  A vertex CONTINUES if a bounce ray will leave it: every vertex but the last
 * of a path (the hit at depth index `bounces`; with bounces = 0 every vertex is last).
 *
 * LIT.  A specular vertex that continues adds `term` alone: the r, g, b of shade_terms, NdotL forced to 0 when occluded as above,
 * WITHOUT background * rho -- the mirror ray now supplies what that stood for.  Every other vertex adds Lit as above, unchanged: the
 * vertices that are not specular, and the last vertex, which is the reference's own bounce + 1 >= max_depth arm.
 *
 * THROUGHPUT.  thr = (1, 1, 1) before the primary vertex, and it is updated when a ray LEAVES a vertex, not when the vertex is hit.
 *
 * THE LOBE PICK at a continuing vertex h of depth k, for sample s of pixel (x, y):
 *   seed = WangHash((x + y * W) * spp + s + 1 + u * 0x9E3779B9), u = ((path.seed + k) mod 2^32) ^ 0x40000000 -- the bounce ray's hash
 *   input with another bit flipped than the emitter ray's 0x80000000; with counts spp is the pixel's own n_p, as for the emitter ray;
 *   0 becomes 1.   xi = random_float(seed): one xorshift step, (float)state * 2.3283064365387e-10f.
 *   MIRROR iff h is specular and (rho >= 1.0f or xi < rho); else DIFFUSE.  A vertex that is not specular takes no draw.
 *   mirror:   thr is unchanged; r' = the mirror ray of closest.cpp:96-99 -- R = normalize(dir(r) - (2.0f * N) * dot(N, dir(r))), N NOT
 *             turned, origin I + R * 0.001f -- traced for its closest hit, no tmax; the segment is marked specular.
 *   diffuse:  thr = thr * Alb(h); r' = the vxrt_render_ao ray with user seed (seed + k) as above; the segment is not specular.
 * The mirror lobe is picked with probability rho and weighs 1, the diffuse lobe with 1 - rho and weighs 1, and `term` already carries
 * its (1 - rho): together they estimate term + rho * L(mirror) + (1 - rho) * Alb * L(diffuse), the reference's recursion extended by
 * indirect light.
 *
 * EMITTER FORMS.  With nee = 1 and emissive_mis the emitter ray belongs to the diffuse lobe: a vertex that picks mirror sends none (a
 * skipped ray: tmax = -1, G = 0, not counted in rays_traced), a vertex that picks diffuse sends it exactly as above, with thr after the
 * multiplication.  A SPECULAR SEGMENT that hits an emitting material adds thr * Emi(h') in full in all three forms: nee = 0 as above;
 * nee = 1, where a bounce hit adds no emission otherwise; emissive_mis with wB = 1 and no lookup in the emitter index.  A segment that
 * is not specular is as above, and so is Emi(h_0) at the primary hit.
 * rays_traced is unchanged in kind: the primaries, one per occlusion ray of a real hit, one per bounce ray of a live path (mirror or
 * diffuse), one per emitter ray actually sent.
 *
 * Three identities follow (each is a test):
 *   A  on a scene where no vertex any path meets is specular the frame is the same descriptor's vxrt_render_path_frame bit for bit --
 *      pixels, colours, rays traced: 1 * x is x.
 *   B  bounces = 0 is that frame bit for bit on any scene: every vertex is last.
 *   C  with bounces = 1, spp a power of two and any `shadow`, a pixel whose primary hit has rho = 1 exactly is the vxrt_render_camera
 *      pixel of the same camera with max_depth = 2, pixel and colour: 0 + 1 * Lit(h_1) against term_0 + C_1 * (1 * rho).
 *
 * THE CALL.  vxrt_path_frame_t cannot grow, so the specular part rides beside it.  specular == NULL or enable = 0 IS
 * vxrt_render_path_frame(accel, frame, stream).  With enable = 1 the frame may carry `path`, `cam` or none, `counts`, and at most one
 * emitter form.  Returns -1 before anything is launched -- dst untouched, vxrt_status unchanged -- for enable > 1, a non-zero reserved
 * word, enable = 1 together with any of denoise / aov / temporal / history / motion / variance, and everything vxrt_render_path_frame
 * refuses.  THE FILTER CHAIN IS OUT OF SCOPE on purpose: a mirror's primary-hit albedo, normal and position are the wrong guides,
 * demodulation by Alb_0 no longer factors, and "the guides of the first vertex that is not specular" is a design of its own.
 * Asynchronous on `stream` as vxrt_render_path_frame; a frame with enable = 1 holds 16 bytes more per path of a batch (VXRT_PATH_BATCH,
 * docs/KNOBS.md): Alb and rho of the path's last vertex.
 *
 * vxrt_specular_pick runs the pick and the mirror ray alone on caller-owned DEVICE buffers: vertices = n x 10 floats (I, N, dir(r), rho),
 * seeds = n hash outputs (0 becomes 1) -> lobe (n: 1 mirror, 0 diffuse) and rays (n x 6: the mirror ray for lobe 1, six zeros for lobe
 * 0).  One launch, asynchronous on `stream`.  Returns -1 before the launch for a null buffer or n >= 2^31; 0 for n = 0. */
typedef struct vxrt_specular_params {
  uint32_t enable;       /* 0 / 1 */
  uint32_t reserved[3];  /* 0 */
} vxrt_specular_params_t;
int vxrt_render_path_frame_specular(vxrt_accel_t* accel, const vxrt_path_frame_t* frame, const vxrt_specular_params_t* specular, void* stream);
int vxrt_specular_pick(uint64_t n, const float* vertices /* device, n x 10: I, N, dir, rho */, const uint32_t* seeds /* device */,
                       float* rays /* device, n x 6 */, uint32_t* lobe /* device */, void* stream);

/* Russian roulette (extension): path frames that end dim paths early, unbiased.  Above a path ends only on a miss or after `bounces`
 * vertices; here a vertex may end it by a draw whose survival probability is the path's throughput, and a survivor is divided by it.
 * Everything is "Path-traced frame" / "Emissive geometry" / "Multiple importance sampling" / "Adaptive sampling" / "Path frames by
 * descriptor" as written, except what follows; every operation is one fp32 operation.  tests/roulette_ref.py restates all of it.
 *
 * Vertex j of a path is the hit found by the bounce ray of depth index k = j - 1; the primary hit is vertex 0, shared by all samples,
 * and never takes a draw.  A vertex h' with first <= j < bounces takes a draw -- a bounce ray would leave it; the last vertex,
 * j = bounces, takes none.
 *
 * THE DRAW happens in the scatter step, after everything the step adds at h' above -- the emitter-ray term of the previous vertex,
 * thr * Lit, the emission terms of all three emitter forms -- and after thr = thr * Alb(h'):
 *   m = thr.x; if (thr.y > m) m = thr.y; if (thr.z > m) m = thr.z;
 *   q = m; if (!(q >= q_min)) q = q_min;                  -- a NaN throughput takes q_min
 *   if (q >= 1.0f) the path continues: no draw, thr untouched.  Otherwise
 *   seed = WangHash((x + y * W) * spp + s + 1 + u * 0x9E3779B9), u = ((path.seed + k) mod 2^32) ^ 0x20000000 -- the bounce ray's hash
 *   input with a third bit flipped (0x80000000 is the emitter ray's, 0x40000000 the lobe pick's); with counts spp is the pixel's own
 *   n_p; 0 becomes 1.   xi = random_float(seed), as in the lobe pick.
 *   The path SURVIVES iff xi < q, and then thr = (thr.x / q, thr.y / q, thr.z / q): three correctly rounded fp32 divisions, no
 *   reciprocal.  Otherwise it ends here: its Lc is final and no ray leaves h'.
 *
 * What follows from that:
 *   - with nee = 1 or emissive_mis the emitter ray of a vertex is generated with the bounce ray that leaves it: a killed vertex sends
 *     none, a survivor's carries thr / q.  Everything after the draw is divided by the probability of getting there, so the estimator
 *     is unbiased;
 *   - rays_traced is unchanged in kind: one per bounce ray of a live path, one per occlusion ray of a real hit, one per emitter ray
 *     sent.  A killed path traces no more rays;
 *   - the filter chain is untouched: the primary vertex takes no draw, so c = D + Alb_0 * E factors as before, and denoise, aov,
 *     temporal, history, motion, variance and counts combine with roulette with nothing else changed.
 *
 * THE CALL.  vxrt_path_frame_t and vxrt_specular_params_t cannot grow, so the roulette part rides beside them.  roulette == NULL or
 * enable = 0 IS vxrt_render_path_frame_specular(accel, frame, specular, stream).  With enable = 1 it returns -1 before anything is
 * launched -- dst, the guide outputs and the history untouched, vxrt_status unchanged -- for enable > 1, `first` outside
 * 1..VXRT_PATH_MAX_BOUNCES, a q_min that is not finite, <= 0 or > 1, a non-zero reserved word, everything vxrt_render_path_frame
 * refuses, and roulette together with specular->enable = 1.  THAT LAST REFUSAL IS ON PURPOSE: in a specular frame thr is updated when
 * the ray leaves, one vertex later, and dividing it before or after the albedo gives different bits -- either choice breaks identity A
 * of "Specular vertices" under roulette.  It is a design of its own.  first >= bounces, q_min = 1 and a scene whose albedos have a
 * component >= 1 everywhere are vxrt_render_path_frame bit for bit.  Asynchronous on `stream`; no launch, buffer or synchronisation
 * is added.
 *
 * vxrt_roulette runs the draw alone on caller-owned DEVICE buffers: thr = n x 3 floats, seeds = n hash outputs (0 becomes 1) -> alive
 * (n: 1 continues, 0 ended) and thr_out (n x 3: thr untouched for q >= 1, thr / q for a survivor, three zeros for a dead entry).  One
 * launch, asynchronous on `stream`.  Returns -1 before the launch for a null buffer, n >= 2^31 or a bad q_min; 0 for n = 0. */
typedef struct vxrt_roulette_params {
  uint32_t enable;    /* 0 / 1 */
  uint32_t first;     /* first vertex index that takes a draw, 1..VXRT_PATH_MAX_BOUNCES */
  float    q_min;     /* floor of the survival probability, finite, 0 < q_min <= 1 */
  uint32_t reserved;  /* 0 */
} vxrt_roulette_params_t;
int vxrt_render_path_frame_ex(vxrt_accel_t* accel, const vxrt_path_frame_t* frame, const vxrt_specular_params_t* specular /* may be NULL */,
                              const vxrt_roulette_params_t* roulette /* may be NULL */, void* stream);
int vxrt_roulette(uint64_t n, const float* thr /* device, n x 3 */, const uint32_t* seeds /* device */, float q_min,
                  float* thr_out /* device, n x 3 */, uint32_t* alive /* device */, void* stream);

/* Environment light (extension): an octahedral radiance map lights path frames -- what a ray that leaves the scene sees, in place of the
 * constant params->background, and with sample = 1 a second estimator that aims rays at the map's bright texels, weighted against the
 * bounce ray by the balance heuristic.  The conventions are those of "Emissive geometry": every symbol is one fp32 IEEE operation (add,
 * mul, div, compare, sqrtf) in the order written, without contraction; pi = 3.14159265f; sign(t) = t >= 0 ? 1.0f : -1.0f; max is
 * std::max (a NaN gives 0); xorshift and random_float are those of THE EMITTER RAY.  tests/env_ref.py restates all of it.
 *
 * THE MAP.  vxrt_envmap_t is an object of its own, not part of an accel: it holds world-space directions only, so no refit and no
 * vxrt_accel_set_transforms makes it stale, and one map may light frames of any accel.  It is made from HOST texels: n x n x 3 floats of
 * RGB radiance, texel (i, j) at 3 * (i + j * n); n is a power of two, 4 <= n <= 256 -- at most 65,536 entries, so the cumulative table
 * fits uint32 exactly as the emitter table's does.  The texel square [-1, 1]^2 is the octahedral unfolding with y as the pole (the
 * fixed camera's up).
 * TEXEL OF A DIRECTION w = (x, y, z):
 *   s = (|x| + |y|) + |z|;   px = x / s;  py = y / s;  pz = z / s
 *   u = px;  v = pz;   if (py < 0) { u = (1 - |pz|) * sign(px);  v = (1 - |px|) * sign(pz); }      (px, pz: the values before the fold)
 *   fu = (u * 0.5f + 0.5f) * (float)n;   i = fu >= 0 ? min((uint32_t)fu, n - 1) : 0;   j likewise from v;   e = i + j * n
 *   r2 = (px * px + py * py) + pz * pz;   r = sqrtf(r2)
 * A NaN direction and the zero vector give texel 0.  Env(w) = texel_e * scale per channel.  The solid-angle density of choosing w through
 * the table is
 *   pe(w) = (qf_e * nn4) * (r2 * r),   qf_e = (float)q_e / (float)Q,   nn4 = (float)(n * n) * 0.25f
 * since an area element du dv of the unfolding subtends du dv / r^3, which integrates to 4 pi over the square.
 * THE TABLE, built on the device at creation:
 *   centre of texel (i, j):  u = (((float)i + 0.5f) / (float)n) * 2.0f - 1.0f,  v likewise from j
 *   c = (1 - |u|) - |v|;   if (c < 0) { u' = (1 - |v|) * sign(u);  v' = (1 - |u|) * sign(v); } else { u' = u;  v' = v; }
 *   P = (u', c, v');   r2 = (P.x * P.x + P.y * P.y) + P.z * P.z;   r = sqrtf(r2)
 *   w_e = max(max(L.r, L.g), L.b) / (r2 * r);   wmax = the maximum over the table (exact in any order)
 *   q_e = max(1, (uint32_t)((w_e / wmax) * 65535.0f));   cum_e = q_0 + .. + q_e in uint32;   Q = cum_{n * n - 1}
 * vxrt_envmap_create returns -1 and makes nothing for n out of range or not a power of two, a null pointer, a texel that is negative
 * or not finite, a map with no positive texel, and a weight w_e that is not finite.  It is synchronous with respect to `stream`, like
 * vxrt_accel_set_emitters.  vxrt_envmap_bytes is the device storage held (20 bytes per texel); vxrt_envmap_read (test / diagnostic;
 * synchronous) copies q and cum to HOST memory, either pointer may be NULL.  A map must outlive every frame that reads it.
 *
 * THE ENVIRONMENT RAY of a vertex (I, N') -- N' faces the viewer -- from hash output `seed` (0 becomes 1):
 *   r0 = xorshift(state);  a = random_float;  b = random_float
 *   t = ((uint64_t)r0 * Q) >> 32;   e = the smallest index with cum_e > t;   (i, j) = (e % n, e / n)
 *   u = (((float)i + a) / (float)n) * 2.0f - 1.0f,  v likewise from j and b;   c, the fold and P as for the table;  r2, r of P;  w = P / r
 *   o = I + N' * 0.001f;  tmax = 1e30f;  any-hit
 *   cosx = max(0, (N'.x * w.x + N'.y * w.y) + N'.z * w.z)
 *   pE = (qf_e * nn4) * (r2 * r);   pb = cosx / pi
 *   G = ((L_e * scale) * cosx) / (pi * pE) per channel;   wE = pE / (pE + pb);   Gm = G * wE
 * Any search that returns the smallest index with cum_e > t is legal (the kernels search the row ends first, then the row): the result
 * is defined, the walk is not.  The radiance is texel e's by index, not by a second lookup.  SKIPPED -- not traced, not counted, without
 * a contribution -- if cosx == 0, if every channel of L_e * scale is 0, or if a channel of Gm is not finite.
 *
 * THE FRAME.  vxrt_render_path_frame_env(accel, frame, roulette, env, stream): env == NULL IS vxrt_render_path_frame_ex(accel, frame,
 * NULL, roulette, stream).  With env set the frame is the descriptor's (with the roulette part, if enabled) except for two rules; the
 * background * reflectivity term inside Lit stays params->background (it is the reference's term, and specular vertices are not part
 * of this frame -- there is no specular parameter, on purpose).
 *   Every ray that misses.  A primary miss is Env(dir(r_0)): the pixel, its `colors`, and what the filter chain shows for a miss.  With
 *     sample = 0 a bounce ray w that misses adds Lc = Lc + thr * Env(w) and the path ends; no launch is added.
 *   sample = 1.  Every vertex a bounce ray leaves sends THE ENVIRONMENT RAY (the last vertex none), with
 *     seed = WangHash((x + y * W) * spp + s + 1 + u * 0x9E3779B9), u = ((path.seed + k) mod 2^32) ^ 0x10000000 -- a fourth bit beside
 *     0x80000000, 0x40000000 and 0x20000000; with counts spp is the pixel's own n_p.  It is traced by the any-hit launch the emitter rays
 *     take in their frames, and in the scatter step, before the miss / hit arm, an unblocked ray adds Lc = Lc + thr * Gm, thr as the
 *     vertex has it (Alb included).  A bounce ray w from a vertex with facing normal N' that misses adds Lc = Lc + thr * (Env(w) * wB):
 *       cosx = max(0, (N'.x * w.x + N'.y * w.y) + N'.z * w.z);   pb = cosx / pi;   pe = pe(w) of TEXEL OF A DIRECTION
 *       den = pe + pb;   wB = den > 0 ? pb / den : 1
 *     rays_traced also counts the environment rays that were traced.  Under roulette the ray is generated with the bounce ray that
 *     leaves the vertex: a killed vertex sends none, a survivor's carries thr / q.
 * counts, roulette and the whole filter chain (denoise, aov, temporal, history, motion, variance) combine with it unchanged: D stays
 * Lit_0 (Env(dir(r_0)) at a miss), and the environment rays of h_0 are part of the stochastic term, as in EMITTER FORM x FILTER.
 * A map whose every texel is c, with scale = 1, sample = 0 and params->background = c, is vxrt_render_path_frame bit for bit.
 * Returns -1 before anything is launched, dst untouched, for env together with emissive or emissive_mis (three-way weighting is a
 * design of its own), a null map, sample > 1, a scale that is negative or not finite, a non-zero reserved word, and everything
 * vxrt_render_path_frame_ex refuses (a non-zero alpha table included).  Asynchronous on `stream`; sample = 1 holds and launches what
 * nee = 1 does.
 *
 * The steps alone, on caller-owned DEVICE buffers, one launch each, asynchronous on `stream`; -1 before the launch for a null map or
 * buffer, a scale that is negative or not finite, n >= 2^31; 0 for n = 0:
 *   vxrt_envmap_lookup: dirs (n x 3) -> radiance3 (n x 3: Env(w)), texel (n: e), pdf (n: pe(w)).
 *   vxrt_env_rays: points (n x 6: I, N'), seeds (n hash outputs) -> rays (n x 6: o, w), tmax (n), weight3 (n x 3: Gm), texel (n: e),
 *     mis (n: wE); a skipped entry gets the ray (0,0,0; 1,1,1), tmax = -1, Gm = 0 and wE = 0, and keeps the e it chose. */
typedef struct vxrt_envmap vxrt_envmap_t;
typedef struct vxrt_env_params {
  vxrt_envmap_t* map;    /* not NULL */
  float scale;           /* multiplies every texel; >= 0 and finite */
  uint32_t sample;       /* 0: the map is seen by rays that miss; 1: and sampled, both weighted */
  uint32_t reserved;     /* 0 */
} vxrt_env_params_t;
int vxrt_envmap_create(const float* texels /* HOST, n x n x 3 */, uint32_t n, void* stream, vxrt_envmap_t** map);
int vxrt_envmap_destroy(vxrt_envmap_t* map);
uint64_t vxrt_envmap_bytes(const vxrt_envmap_t* map);
int vxrt_envmap_read(vxrt_envmap_t* map, uint32_t* q /* HOST, n x n, or NULL */, uint32_t* cum /* HOST, n x n, or NULL */, void* stream);
int vxrt_render_path_frame_env(vxrt_accel_t* accel, const vxrt_path_frame_t* frame, const vxrt_roulette_params_t* roulette /* may be NULL */,
                               const vxrt_env_params_t* env /* may be NULL */, void* stream);
int vxrt_envmap_lookup(vxrt_envmap_t* map, uint64_t n, const float* dirs /* device, n x 3 */, float scale, float* radiance3 /* device, n x 3 */,
                       uint32_t* texel /* device */, float* pdf /* device */, void* stream);
int vxrt_env_rays(vxrt_envmap_t* map, uint64_t n, const float* points /* device, n x 6: I, N' */, const uint32_t* seeds /* device */, float scale,
                  float* rays /* device, n x 6 */, float* tmax /* device */, float* weight3 /* device, n x 3: Gm */, uint32_t* texel /* device */,
                  float* mis /* device, n: wE */, void* stream);

/* ---- software twin: the reference's raycast test (tests/regression/raycast) ----
 * Buffers in the reference's formats (raycast/common.h): tlas_node_t 32 B, blas_node_t 160 B (transform,
 * invTransform, bvh_offset@128, tex_offset@136, tex_width@144, tex_height@148, reflectivity@152),
 * bvh_node_t 32 B, tri_t 36 B, tri_ex_t 60 B, triIdx u32, 0x00RRGGBB texels.  Device pointers. */
typedef struct vxrc_scene {
  const void* tlas; const void* blas; const void* bvh; const void* tri; const void* triEx; const void* triIdx; const void* tex;
  uint32_t n_tlas_nodes, n_blas, n_bvh_nodes, n_tris, n_tri_idx, tlas_root;
  uint64_t tex_bytes;
} vxrc_scene_t;
typedef struct vxrc_params {     /* the fields of raycast/common.h:126-150 kernel_arg_t that are not addresses */
  float camera_pos[3], camera_forward[3], camera_right[3], camera_up[3], viewplane[2];
  uint32_t samples_per_pixel, max_depth;
  float light_pos[3], light_color[3], ambient_color[3], background_color[3];
} vxrc_params_t;
/* Acceleration layout of a raycast scene, built once per scene (compact 64-byte BVH2 nodes holding both children's boxes and
 * complete child descriptors; triangles in edge form in leaf order, the triIdx indirection resolved).  The build validates every
 * index the BVH walk follows (children inside their instance's node range and after their parent, leaf ranges inside triIdx,
 * triIdx entries inside tri, bvh_offset of every instance) and fails (-1) on a malformed tree; TLAS indices, instance indices
 * and texture extents are checked where the kernel follows them (status bit 2).  The scene's buffers must stay alive and
 * unchanged while the layout is in use. */
typedef struct vxrc_accel vxrc_accel_t;
int vxrc_accel_build(const vxrc_scene_t* scene, void* stream, vxrc_accel_t** out);
int vxrc_accel_destroy(vxrc_accel_t* accel);
/* What the build decided (diagnostic): which = 0 -> 1 if the walk takes two BVH2 levels per fetch (wide nodes), 0 if it keeps the
 * reference's two-wide walk (a box that is not the union of its children's, an unbounded box, or a tree deeper than 42 internal
 * levels, whose wide walk could need more than the reference's 64 stack entries); which = 1 -> internal nodes on the longest
 * root-to-leaf path, counted up to 43 (0 when the wide layout was not requested). */
int vxrc_accel_info(const vxrc_accel_t* accel, uint32_t which, uint64_t* value);
/* vxrc_render on a prebuilt layout (asynchronous on `stream`; the layout keeps four frame contexts: frames issued round robin on up to
 * four streams overlap). */
int vxrc_render_accel(vxrc_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                      const vxrc_params_t* params, uint32_t* dst, float* colors, void* stream);

/* One-shot form: builds the layout, renders, frees it (synchronises the device).
 * Rows [y0,y1) of the frame kernel.cpp:9-33 renders: GenerateRay (render.h:192-211) -> Trace (:213-275) summed
 * over the samples -> RGB32FtoRGB8 -> dst[x + y*W].  colors (optional): f32 rgb per pixel before packing.
 * A malformed BVH fails the call (-1); a TLAS / instance index or texture extent outside its buffer, a stack deeper than the
 * reference's BVH_STACK_SIZE (64, undefined behaviour there) or a runaway TLAS walk sets vxrt_status bits 2 / 0 / 1.
 *
 * Conversions C leaves undefined.  The twin's Trace casts floats that need not fit, as the RTU shader does: uint32_t(uv * size) in
 * texSample (render.h:10-11) and int(min(c, 1) * 255) in RGB32FtoRGB8 (common.h:106-108).  Every uv, light, ambient, background and
 * reflectivity value is accepted, finite or not, and the frame is what the reference's x86-64 build renders -- by the rule written at
 * vxrt_shade_rays, which the kernel (csrc/rc_kernels.hip: f2u_x86, f2i_x86) and the restatement (oracle/rc_oracle.c) state as range tests
 * instead of casts: u * w at or above 2^63, +-inf and NaN read texel column 0, negative uv wrap, a NaN channel packs as INT_MIN (the
 * bare cast gave 0 on gfx950: an all-NaN colour packed as 0 instead of 0x80000000).  The reference's object code agrees for every class
 * tried; tests/test_rc_hostile_cpu.py pins the values, tests/test_gpu_rc_hostile.py holds the kernel to them. */
int vxrc_render(const vxrc_scene_t* scene, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                const vxrc_params_t* params, uint32_t* dst, float* colors, void* stream);

/* Diagnostic variant of vxrt_render_stats_timed: additionally logs 16 u64 per wavefront of the main traversal launch into
 * wave_log (device u64[16 * 4 * 8 * 256]): [0] first and [1] last 100 MHz clock, [2] rays started, [3] loop iterations,
 * [4] runs of the node body and [5] lanes active in them, [6] runs of the leaf body and [7] lanes active in them,
 * [8] lane node steps served from the LDS top-of-tree image, [9] node-body runs in which every node lane was at the same
 * node, [10] shader clocks inside the node body, [11] inside the instance + leaf part, [12] of the whole wavefront,
 * [13] inside the fetch section (job queue, ray generation), [14] inside the finish section (records, occlusion-ray
 * start), [15] reserved -- to study load balance and lane occupancy of the launch (tools/wave_balance.py). */
int vxrt_render_wave_log(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                         const vxrt_shade_params_t* params, int shadow, uint32_t* dst,
                         unsigned long long* counters, unsigned long long* wave_log, void* stream);

/* Trace n rays (6 floats each: origin, direction) read from HBM, write n hit records.
 * tmax: optional per-ray upper bound (NULL = 1e30); a bound above 1e30 is taken as 1e30 (the reference's hit.dist never
 * exceeds it: rt_traversal.h:7,44-52). */
int vxrt_trace(vxrt_accel_t* accel, const float* rays, uint64_t n, const float* tmax,
               vxrt_hit_t* hits, int mode, void* stream);

/* Closest-hit / miss shader over n (ray, hit record) pairs -- the hit records vxrt_trace wrote for those rays: f32 colour (3 per
 * ray, optional) and packed RGB8 (optional) as closest.cpp:57-127 (no secondary ray) / miss.cpp:9-14 / common.h:149-154 compute
 * them.  The records must come from this accel (their blasIdx / triIdx are followed unchecked).
 *
 * Conversions C leaves undefined.  The reference's shader casts floats that need not fit: uint32_t(u * width) in texSample
 * (rtx_shading.h:7-8) and int(min(c, 1) * 255) in RGB32FtoRGB8 (common.h:149-154).  Every finite or non-finite scene value and shade
 * parameter is accepted, and this shader -- here and in every frame entry point -- returns what the reference's x86-64 build returns,
 * stated as a rule that neither the kernels nor the oracle leave to a cast:
 *   uint32_t(f) = the truncated value modulo 2^32 for -2^63 <= f < 2^63 (negative uv wraps), 0 for NaN and every other f
 *   int(f)      = the truncated value for -2^31 <= f < 2^31, INT_MIN (0x80000000) for NaN and every other f
 * and the pack adds (r << 16) + (g << 8) + b modulo 2^32: an all-NaN colour packs to 0x80000000, a NaN in r or g alone adds nothing.
 * tests/test_shading_cpu.py pins the values, tests/test_gpu_shading_fuzz.py holds the kernels to them. */
int vxrt_shade_rays(vxrt_accel_t* accel, const float* rays, const vxrt_hit_t* hits, uint64_t n, const vxrt_shade_params_t* params,
                    float* colors, uint32_t* rgb8, void* stream);

/* Camera rays of rows [y0, y1) of the RTU test's frame (kernel.cpp:28-39) as a ray buffer: 6 floats per ray, ray of pixel (x, y) at
 * index x + (y - y0) * width. */
int vxrt_camera_rays(uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, float* rays, void* stream);

/* The rays of rows [y0, y1) of pinhole camera `cam` (see vxrt_camera_t), laid out as vxrt_camera_rays': 6 floats per ray, the ray
 * of pixel (x, y) at index x + (y - y0) * width.  `cam` is a host pointer read during the call; -1 for a null or non-finite camera. */
int vxrt_pinhole_rays(const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, float* rays, void* stream);

/* Opt-in REFERENCE-QUIRKS traversal.  vxrt_trace / vxrt_render implement the canonical algorithm: the reference RTU's result
 * wherever the RTU addresses its own data.  With a TLAS deeper than one level it does not: children of a TLAS internal node popped
 * from the short stack are addressed relative to the last BLAS's base_ptr (sim/simx/rt_traversal.cpp:91-92 after :119-120), it reads
 * unrelated memory and loses hits that exist.  What it returns then depends on the memory layout, so this entry point works on what
 * the simulator works on: ONE flat memory image addressed with 32-bit offsets (its RAM) and the four base pointers of the RTX DCRs
 * 0x6..0x9, and restates BVHTraverser::traverse literally (trail[32], 5-entry short stack, restart, re-descent after every
 * accepted candidate, libstdc++ min/max).  One thread per ray; a compatibility mode, not a fast path.  Reads outside the image
 * return zeros; a path deeper than 32 levels sets status bit 0 (undefined behaviour in the reference).
 * mode: VXRT_MODE_CLOSEST = fixed point of the accept loop, VXRT_MODE_ANY = first accepted candidate.  tmax (optional) as vxrt_trace. */
int vxrt_trace_reference_quirks(const void* image, uint64_t image_size, uint32_t tlas_off, uint32_t blas_off, uint32_t bvh_off, uint32_t tri_off,
                                const float* rays, uint64_t n, const float* tmax, vxrt_hit_t* hits, int mode, void* stream);

/* Diagnostic (tests): copies the first n_dwords (<= 800) of the control block of frame context `ctx` to `out` after synchronising
 * `stream`: [0] number of rays the main launch handed to the EXACT launch, [32 + 32 k] queue shard k (k = 0..7) of the main launch,
 * [288 + 32 k] of the EXACT launch over the deferred list, [544 + 32 k] of the a-priori EXACT launch.  A vxrt_trace call leaves the
 * block as its launches left it (the next call clears it). */
int vxrt_debug_read_control(vxrt_accel_t* accel, uint32_t ctx, uint32_t* out, uint32_t n_dwords, void* stream);
/* Tests only: the shadow hints.  A timed shadow frame (fixed or caller camera, single or batch) of an accel that holds a path table
 * (vxrt_accel_info(accel, 9) == 1: built as one identity instance of at most 16 levels with the fma decode) and takes the identity-root
 * kernels (index 5) keeps, per frame context, one word per hit-record slot -- tile-major: tile * 64 + (y & 7) * 8 + (x & 7), a batch's frames
 * one after the other -- that names the triangle which blocked the slot's occlusion ray last (0xFFFFFFFF: none yet).  Only a frame that
 * REPEATS the context's last such frame (same window, same light in every frame of the set, same cameras, no refit in between) is handed
 * the words: its first repeat starts from none and leaves its blockers, the next descends towards them first.  Any other frame runs the
 * kernels without hints and makes the context's words void.  Hints choose a visiting order only: every frame is the same bits whatever the words hold.
 * VXRT_SHADOW_HINTS=0 in the environment renders without them.  set overwrites, get reads, the first n words of the context `stream` rendered such
 * a frame on last (host memory), after synchronising `stream`; -1 if there is none or n exceeds its capacity. */
int vxrt_debug_set_shadow_hints(vxrt_accel_t* accel, void* stream, const uint32_t* hints, uint64_t n);
int vxrt_debug_get_shadow_hints(vxrt_accel_t* accel, void* stream, uint32_t* hints, uint64_t n);
/* Tests only: on = 0 renders without shadow hints whatever the environment says, 1 with them, -1 goes back to the environment
 * (VXRT_SHADOW_HINTS, read once per process).  A frame without hints launches the kernels without them and touches no hint word.
 * Process-wide; takes effect with the next frame. */
int vxrt_debug_shadow_hints_enable(int on);
/* Tests only: the first n words (n <= n_tris) of the accel's path table to `out` (host memory), after synchronising `stream`: per
 * triangle the child slot at each internal level from the BLAS root to the triangle's leaf, 2 bits per level, the root's in the low
 * bits.  -1 if the accel holds no table. */
int vxrt_debug_read_path_table(vxrt_accel_t* accel, uint32_t* out, uint64_t n, void* stream);
/* Diagnostic (libraries built with -DRT_SHADOW_HINT_COUNT=1 only; -1 otherwise): out[0] = occlusion rays of hinted frames that ended
 * blocked in the main launch, out[1] = those of them that were blocked while still guided by their hint (no hinted slot failed its box
 * test, no pending sibling taken); sums over the current device since the last reset.  Synchronises `stream`. */
int vxrt_debug_shadow_hint_counts(unsigned long long* out, int reset, void* stream);
/* Diagnostic (libraries built with -DRT_PHASE_COUNT=1 only; -1 otherwise): what the wavefronts of the shadow frame kernels that hold the
 * occlusion-only loop ran.  out[0..2] = passes through a form of the traversal loop: the occlusion-only form, the general form with no
 * any-hit lane, the general form holding primary and any-hit rays; out[3..5] = the node-body runs inside them, by the same classes (a run
 * of the general form is classed by the lanes that hold work when it starts).  Sums over the current device since the last reset.
 * Synchronises `stream`. */
int vxrt_debug_phase_counts(unsigned long long* out, int reset, void* stream);
/* Diagnostic (tools/xcd_tail.py): from now on every main traversal launch on this layout -- the TIMED kernels included -- leaves per
 * wavefront (index = workgroup * 4 + wavefront of the workgroup) [0] the constant 100 MHz clock at its end and [1] rays it started |
 * physical XCD << 56 in `log` (device memory, 2 u64 per wavefront, room for 8,192 wavefronts); NULL switches it off.  One store per
 * wavefront, at its end.  The pointer is captured by the launches enqueued after the call (no synchronisation): the caller keeps the
 * memory alive until they have run. */
int vxrt_debug_end_log(vxrt_accel_t* accel, unsigned long long* log);
/* Diagnostic (tools/trace_phases.py): vxrt_trace_stats launches keep vxrt_render_wave_log's 16 u64 per wavefront in `log` (device
 * memory, 16 x 8,192 u64) from now on; NULL switches it off. */
int vxrt_debug_trace_wave_log(vxrt_accel_t* accel, unsigned long long* log);
/* Diagnostic (tools/child_counts.py): the wave-log launches (vxrt_render_wave_log, vxrt_render_interleaved_batch_wave_log) count their
 * node-body runs by the largest number of valid children any node lane of the run holds.  out (host memory, 8 u64): [0..3] runs that took
 * the ordered arm with at most 0, 1, 2 and with 3 or 4 valid children, [4..7] the same for the occlusion arm; sums over every wavefront
 * of every such launch on the current device since the last reset.  Synchronises `stream`; reset != 0 zeroes the counts after reading.
 * Frame launches only (the counting build of the timed traversal); the ray-buffer log of vxrt_debug_trace_wave_log is not classed.  The
 * shader clocks the classing takes lie outside the wave log's node-body and leaf-body windows ([10], [11]), which stay comparable with
 * logs taken before the classing existed; they are part of the wavefront's whole time ([12]). */
int vxrt_debug_child_counts(unsigned long long* out, int reset, void* stream);
/* diagnostic (tools/tile_tail.py): what frame context `ctx` learned for sets of `batch` frames -- per-tile cost (loop iterations of the
 * wavefront that traced it in the last launch; start clocks, durations and steal distances behind them after a wave-log launch) and the
 * tile order derived from it.  Returns the capacity in tiles. */
int vxrt_debug_read_lpt(vxrt_accel_t* accel, uint32_t ctx, uint32_t batch, uint32_t* cost, uint32_t cost_cap, uint32_t* order, uint32_t order_cap,
                        void* stream);

/* Status word of the launches on this device since the last call: 0 = ok, bit0 = traversal stack overflow
 * (tree deeper than the 32 levels the reference's own trail supports; the twin: deeper than BVH_STACK_SIZE),
 * bit1 = iteration limit, bit2 = the twin's kernel met an index outside its buffers.  Synchronises `stream`;
 * a non-zero word is cleared by the call (read-and-clear), so one failed run does not fail the next. */
int vxrt_status(void* stream, uint32_t* status);
/* Raw device pointer behind a vx_buffer_h of the hip backend (for zero-copy hand-off to RCCL). */
int vx_hip_buffer_device_ptr(vx_buffer_h hbuffer, void** dev_ptr);

/* Host-side counters of a hip-backend device: which 0 = acceleration layouts built by vx_start so far (one per scene upload,
 * not one per run), 1 = hipMalloc calls made for buffers (buffers up to 4 KB share slabs), 2 = runs split over more than one GPU,
 * 3 = GPUs behind this device, 4 / 5 = joined runs whose MCYCLE came from the device's clock / from the host's, 6 = the last joined run on
 * the host's clock (vx_start -> the stream seen drained), microseconds, 7 = runs whose shares were gathered through RCCL.
 *
 * vx_mpm_query(MCYCLE) = the last run's duration x the shader clock.  The duration is taken on the DEVICE, on its constant 100 MHz clock:
 * vx_start launches a one-thread kernel on a stream of its own that stores the clock (it starts with the run's first launch and delays
 * nothing on the run's stream), the run's last kernel -- the one that sends rays and status back -- reads the clock again.  A host that
 * does other work between vx_start and vx_ready_wait does not lengthen it.  Should the stamp not have landed when the run's last kernel
 * reads it (never observed) the run reports the host's clock (vx_start -> the moment the stream was seen drained); stats 4 / 5 count both.
 *
 * More than one GPU behind ONE vx_device (the unmodified reference host, which opens one device: tracer.cpp:78):
 *   VORTEX_HIP_DEVICES=0,1,2,3   the first index holds the address space (every vx_mem_* / vx_copy_* call), the others keep a copy of the
 * scene's seven buffers (refreshed when one is uploaded again) and their own acceleration layout.  vx_start of a whole frame traces tile
 * rows k, k+n, ... on the k-th listed device and copies them into the first device's output buffer, behind which the run's last kernel
 * waits: vx_ready_wait, vx_copy_from_dev and vx_mpm_query (MINSTRET = rays of all shares) behave as with one GPU.  A run the host restricted
 * itself (DCR 0x7F0-0x7F3), a reference-quirks run and the software twin's kernel stay on the first device.
 *   VORTEX_HIP_GATHER=rccl       the shares travel through RCCL instead of peer copies (north_star: "RCCL gather over xGMI only for final
 * image assembly", from the C host): one communicator per distinct listed GPU (ncclCommInitAll, librccl.so.1 loaded with dlopen at
 * vx_dev_open), per run every share packed into contiguous bytes on its own GPU, ONE group of ncclSend / ncclRecv pairs, the first device
 * placing the received shares into the output buffer's rows.  Default ("copy"): hipMemcpy2DAsync between the devices.  stat 7 counts
 * the runs gathered through RCCL. */
int vx_hip_device_stat(vx_device_h hdevice, uint32_t which, uint64_t* value);

const char* vxrt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VORTEX_HIP_H */
