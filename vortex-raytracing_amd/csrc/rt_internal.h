// Internal to the HIP library (not installed, not part of include/vortex_hip.h): what rt_kernels.hip (traversal, shading, the
// level-2 entry points), rt_accel.hip (acceleration-layout build, refit), rt_secondary.hip (the tails of mirror-bounce and
// ambient-occlusion frames, the binning of secondary rays), rt_path.hip (the tail of a path frame, its entry points) and rt_denoise.hip (the end of a
// denoised path frame's tail: a-trous filter, temporal accumulation, variance guidance) share: the types, and the few host functions one
// unit calls in another.  The constants of the compact layout are in rt_types.h; the device arithmetic of shading, which rt_kernels.hip,
// rt_secondary.hip and rt_path.hip share, is in rt_shading.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include <vector>
#include "rt_types.h"
#include "../../include/vortex_hip.h"

#define STATUS_STACK_OVERFLOW 1u
#define STATUS_ITER_LIMIT 2u
#define STATUS_BAD_SCENE 4u
#define STATUS_FMA_DECODE_DIFFERS 8u   // build-time only: selects the ldexp decode for the scene

// ---------------------------------------------------------------------------------------------
// Device-side acceleration layout, derived once per scene from the reference-format buffers by the
// accel_* kernels of rt_accel.hip (the reference bytes stay the source of truth).
//
// Work descriptor, 32 bit: [31:30] kind, [29:0] payload
//     kind 0  TLAS internal node   payload = compact node index (TLAS nodes come first)
//     kind 1  BLAS internal node   payload = compact node index (n_tlas + index in the bvh buffer)
//     kind 2  BLAS leaf            payload = count<<26 | firstTriangle   (count 1..15; count 0:
//                                  payload = index of the reference leaf node, range read from it)
//     kind 3  instance (TLAS leaf) payload = blasIdx
//     0xFFFFFFFF = empty child slot, 0xFFFFFFFE = ray finished, 0xFFFFFFFD = lane idle
//
// Compact node, 64 B = half a cache line, one per INTERNAL node, TLAS and BLAS nodes in one index space:
//     q0 = origin.xyz, 2^ex as float
//     q1 = plane words lo.x, lo.y, lo.z, hi.x     one byte per child: byte k of word j = plane j of child k
//     q2 = plane words hi.y, hi.z, desc0, desc1   desc k = complete work descriptor of child k
//     q3 = desc2, desc3, 2^ey, 2^ez
//   -> a node visit is four 16-byte loads per lane (the vector-memory return path, not HBM, is what
//      saturates first on MI355X for wider nodes: profiles/r01_b_*), no index arithmetic on children,
//      a leaf or instance never costs a node fetch of its own, and stack entries are 2 dwords.
// Wide triangle, 48 B: v0, edge1 = v1 - v0, edge2 = v2 - v0 (the subtractions of
//     rt_traversal.cpp:272-278 done once), three aligned 16-byte loads.
// ---------------------------------------------------------------------------------------------
struct SceneDev {
  const uint4* nodes_c;      // compact nodes: the TLAS nodes, then the BLAS nodes (one index space, no per-lane base select)
  const uint32_t* ref_tlas;  // reference TLAS nodes (13 dwords each): exponents for the ldexp decode
  uint32_t n_tlas;           // compact index of BLAS node j = n_tlas + j
  const float4* tri_w;       // wide triangles
  const uint32_t* blas_root; // per instance record: descriptor of its BLAS root
  uint32_t tlas_root;        // descriptor of the TLAS root
  uint32_t exact_decode;     // 1: decode child boxes with ldexp instead of the exact-product fma
  const uint32_t* ref_bvh;   // reference bvh nodes (13 dwords each): ranges of leaves > 15 triangles
  const uint32_t* blas;      // reference blas_node_t records (40 dwords each)
  const rt_triex_t* triEx;
  const rt_material_t* mat;
  const uint8_t* tex;
  // top of the tree for LDS staging (accel_top_kernel): the first n_top internal nodes in breadth-first order from the
  // TLAS root, as four planes of n_top uint4 (q0[], q1[], q2[], q3[]: conflict-free ds_read_b128 for neighbouring slots);
  // child descriptors inside the image and the *_top roots address staged nodes by slot (DESC_TOP_FLAG)
  const uint4* top_img;
  uint32_t n_top;
  uint32_t tlas_root_top;
  const uint32_t* blas_root_top;
  uint32_t ident_root;       // 1: the TLAS root is an instance leaf whose inverse transform is the identity (see start_ray)
};

struct HitRec { float dist, bx, by, bz; uint32_t blasIdx, triIdx; };

struct ShadeParams { float amb[3], lcol[3], lpos[3], bg[3]; uint32_t max_depth; };

// Mutable per-frame state.  An accel owns up to MAX_FRAMES_IN_FLIGHT of these and hands them out round
// robin, so that renders issued on different streams overlap on the GPU (the tail of one persistent
// launch, where most wavefronts have drained, is filled by the head of the next frame's launch); a
// context is handed out again only behind the event of its previous render.
#define MAX_FRAMES_IN_FLIGHT 8
struct FrameCtx {
  void* hitbuf = nullptr;      // W*H hit records between the traversal and the shading pass
  uint64_t hitbuf_pixels = 0;
  // shadow hints (RT_SHADOW_HINTS, rt_kernels.hip): per hit-record slot the triangle that blocked the slot's occlusion ray last, 0xFFFFFFFF =
  // none; reset on the stream when the window the slots belong to (hint_key) changes
  uint32_t* hints = nullptr; uint64_t hints_cap = 0; uint32_t hint_key[6] = {0, 0, 0, 0, 0, 0}; bool hints_valid = false; uint64_t hint_seq = 0;
  // what the context's last shadow frame that could take hints was rendered from -- the light of every frame of the set, the cameras of a
  // camera frame, the accel's scene_gen: a frame is handed hints only if it is that frame again (ensure_shadow_hints)
  std::vector<float> hint_sig; uint64_t hint_gen = 0; bool hint_sig_set = false;
  uint32_t* defer = nullptr;   // job list of the EXACT launch
  uint64_t defer_cap = 0;
  uint32_t* ctl = nullptr;     // control block (CTL_DWORDS), zero between frames
  ShadeParams* pbatch = nullptr;   // per-frame shading parameters of a batch launch (VXRT_MAX_BATCH entries)
  float* cam = nullptr; uint64_t cam_floats = 0;   // camera block of the context's camera frames (see CAM_HDR)
  bool ctl_dirty = false;      // a call failed after touching it: clear before the next use
  // mirror-bounce levels (allocated on first use; level 0 only holds `term`, one entry per pixel)
  struct Level {
    float4* term = nullptr; uint64_t cap = 0;
    float* rays = nullptr; HitRec* hits = nullptr; uint32_t* parent = nullptr; float* col = nullptr; uint64_t ray_cap = 0;
    float* srays = nullptr; float* stmax = nullptr; HitRec* shits = nullptr; uint64_t shadow_cap = 0;   // (frames with the shadow extension)
    uint32_t n = 0;
  };
  std::vector<Level> lv;
  uint32_t* bcount = nullptr;  // device: rays appended to the level being built
  // tile cost of the last frame and the order derived from it (render jobs, see lpt_order_kernel)
  // one slot per batch size (slot 1 = single frames): a frame loop that alternates batch sizes keeps what it learned for each
  struct Lpt { uint32_t* cost = nullptr; uint32_t* order = nullptr; uint32_t cap = 0; uint32_t key[6] = {0, 0, 0, 0, 0, 0}; bool valid = false; };
  Lpt lpt[VXRT_MAX_BATCH + 1];
  // ambient-occlusion pass (allocated on first use), one entry per pixel of the window
  float4* ao_geo = nullptr; float4* ao_nrm = nullptr; float4* ao_col = nullptr; uint32_t* ao_cnt = nullptr;
  uint32_t* ao_list = nullptr; uint32_t* ao_hdr = nullptr;   // pixels with a hit; [0] their number, [1] rays of the current batch
  float* ao_rays = nullptr; float* ao_tmax = nullptr; HitRec* ao_hits = nullptr; uint64_t ao_cap = 0, ao_ray_cap = 0;
  uint32_t* bin_hist = nullptr; uint32_t* bin_keys = nullptr; uint32_t* bin_order = nullptr; uint64_t bin_cap = 0, bin_ray_cap = 0;   // secondary-ray binning
  // (every pt_* and mo_* field below is grown and written by rt_path.hip; rt_denoise.hip reads the per-pixel ones)
  // path frames (vxrt_render_path; allocated on first use).  Per pixel of the window: hit point (w = hit?), shading normal, primary
  // direction, Lit, Alb of the primary hit and the accumulator over samples; the pixels with a hit ([0] of pt_hdr their number, [1] / [2]
  // the live paths of even / odd depths).  Per path of a batch: I, N, dir of its last vertex, Lc, thr; the two lists of live paths;
  // the bounce rays and their hit records; with light sampling the occlusion rays, their tmax and hit records.
  float4* pt_geo = nullptr; float4* pt_nrm = nullptr; float4* pt_dir = nullptr; float4* pt_lit = nullptr; float4* pt_alb = nullptr; float4* pt_acc = nullptr;
  uint32_t* pt_list = nullptr; uint32_t* pt_hdr = nullptr; uint64_t pt_cap = 0;
  float4* pt_I = nullptr; float4* pt_N = nullptr; float4* pt_D = nullptr; float4* pt_L = nullptr; float4* pt_T = nullptr;
  uint32_t* pt_live[2] = {nullptr, nullptr}; float* pt_rays = nullptr; HitRec* pt_hits = nullptr; uint64_t pt_path_cap = 0;
  float* pt_srays = nullptr; float* pt_stmax = nullptr; HitRec* pt_shits = nullptr; uint64_t pt_shadow_cap = 0;
  // path frames with per-pixel sample counts (vxrt_render_path_adaptive; allocated on first use).  Per pixel of the window: the clamped
  // count (0 for a miss) and the 64-bit exclusive offset of its first path among the frame's paths in window order; per scan block of
  // PT_SCAN_BLOCK pixels: the block's sum and its 64-bit offset; [0] of pt_ctot the frame's paths.  Per path of a batch: its pixel and
  // its sample index.
  uint32_t* pt_cnt = nullptr; unsigned long long* pt_off = nullptr; uint64_t pt_cnt_cap = 0;
  uint32_t* pt_bsum = nullptr; unsigned long long* pt_boff = nullptr; uint64_t pt_blk_cap = 0;
  unsigned long long* pt_ctot = nullptr;
  uint32_t* pt_spix = nullptr; uint32_t* pt_ssmp = nullptr; uint64_t pt_slot_cap = 0;
  // path frames with emitter sampling (vxrt_render_path_emissive, nee = 1; allocated on first use).  Per live path of a depth: the emitter
  // ray, its tmax and hit record, and G (w = 1: the ray is real, 0: skipped)
  float* pt_erays = nullptr; float* pt_etmax = nullptr; HitRec* pt_ehits = nullptr; float4* pt_eG = nullptr; uint64_t pt_em_cap = 0;
  // path frames with specular vertices (vxrt_render_path_frame_specular; allocated on first use).  Per path of a batch: Alb of its last
  // vertex and that vertex's reflectivity in .w -- in such a frame pt_T is thr BEFORE the last vertex's albedo, pt_D.w marks a specular
  // segment in flight, and .w of pt_alb is the primary hit's reflectivity
  float4* pt_A = nullptr; uint64_t pt_spec_cap = 0;
  // denoised path frames (vxrt_render_path_denoised; allocated on first use): the two signal buffers the a-trous iterations ping-pong
  // between, one float4 (E, lum(E)) per pixel of the window; the guides are pt_geo and pt_nrm
  float4* dn_sig[2] = {nullptr, nullptr}; uint64_t dn_cap = 0;
  // frames with motion (vxrt_render_path_temporal_motion; allocated on first use): the previous-position guide of every pixel's primary
  // hit, Q4 and N'4, written by the prepare launch and read by the temporal step
  float4* mo_pos = nullptr; float4* mo_nrm = nullptr; uint64_t mo_cap = 0;
  void* pool_spill = nullptr; uint64_t pool_spill_bytes = 0;  // ray-pool trace kernel: the part of the slots' stacks that does not fit LDS
  hipStream_t side = nullptr;
  hipEvent_t ev_in = nullptr, ev_side = nullptr, ev_done = nullptr;
  bool busy = false, inited = false, done_recorded = false;
  hipStream_t last_stream = nullptr;
};

struct vxrt_accel {
  SceneDev dev{};
  vxrt_scene_t ref{};
  void* nodes_c = nullptr; void* tri_w = nullptr; void* blas_root = nullptr;
  void* top_img = nullptr; uint32_t* top_roots = nullptr;   // LDS-staged top of the tree: image; [0] n, [1] TLAS root, [2..] BLAS roots
  // path table (accel_path_kernel, rt_accel.hip): per triangle the child slot at each internal level from the BLAS root to its leaf, 2 bits per
  // level, root in the low bits.  Only for an accel built as one identity instance of at most RT_SHALLOW_LEVELS levels with the fma decode
  // (what ident_root_form asks of the build); nullptr otherwise.  A refit keeps the topology, hence the table.
  uint32_t* tri_path = nullptr;
  uint64_t scene_gen = 0;          // counts the refits (vxrt_accel_refit, vxrt_accel_set_transforms), successful or not
  uint64_t hint_seq = 0;           // counts the hinted frames of the accel's contexts (FrameCtx::hint_seq)
  FrameCtx ctx[MAX_FRAMES_IN_FLIGHT];
  uint32_t n_ctx = 1, next_ctx = 0;
  bool stream_seen = false, multi_stream = false; hipStream_t first_stream = nullptr;   // (see release_ctx)
  float* uvtab = nullptr;      // camera tables: u[W] then v[H]
  uint32_t uv_w = 0, uv_h = 0;
  // camera pixels whose primary ray has a zero direction component (u == 0 or v == 0): listed on the
  // host per (W, H, y0, y1) and traced by an EXACT launch on a side stream, concurrently with the main one
  uint32_t* apriori = nullptr; // [0] count, [1..] job ids
  uint32_t* batch_order[VXRT_MAX_BATCH + 1] = {}; uint32_t bo_tiles = 0;   // band-major tile order of a batch of k frames of bo_tiles tiles each, per k
  uint32_t ap_count = 0, ap_key[6] = {0, 0, 0, 0, 0, 0};
  uint64_t ap_cap = 0;
  float max_reflectivity = 0.0f;   // over the instance records: > 0 enables the mirror-bounce path
  unsigned long long* trace_wave_log = nullptr;   // diagnostic (vxrt_debug_trace_wave_log): per-wavefront log of the counting build's ray-buffer launches
  unsigned long long* end_log = nullptr;   // diagnostic (vxrt_debug_end_log): where the main launches leave their wavefronts' end times
  uint32_t levels = 0;             // internal levels on the longest root-to-leaf path (TLAS + BLAS), counted up to RT_SHALLOW_LEVELS + 1
  bool shallow = false;            // levels <= RT_SHALLOW_LEVELS: the timed launches take the SHALLOW instantiations
  int device = 0;
  struct RefitPlan* refit = nullptr;   // vxrt_accel_refit: built at the first refit
  uint32_t blas_status = 0;        // STATUS_FMA_DECODE_DIFFERS of the BLAS region as its last re-layout found it (build or GEOMETRY refit)
  bool stale = false;              // a refit failed after it had started writing: every render / trace refuses until a refit succeeds
  // alpha test (vxrt_accel_set_alpha_test): the caller's per-material thresholds and, derived from them, one byte per triangle
  // (alpha_tri[t] = alpha_mat[triEx[t].texId]: what the traversal reads).  alpha_on: some threshold is non-zero.
  uint8_t* alpha_mat = nullptr; uint8_t* alpha_tri = nullptr;
  bool alpha_on = false;
  // motion snapshot (vxrt_accel_motion_snapshot): the instance records and, with VXRT_REFIT_GEOMETRY, the tri_t vertices of the previous frame
  uint32_t* motion_blas = nullptr; float* motion_tri = nullptr;
  uint32_t motion_what = 0;        // the VXRT_REFIT_* mask held; 0: no snapshot
  // emitter table (vxrt_accel_set_emitters; the definition is in the header, "Emissive geometry"): per entry V0, E1, E2, Le in world space
  // (12 floats), the quantised weight q and its inclusive prefix sum cum; em_Q = cum[em_n - 1].  em_valid: set, and nothing has moved since
  float* em_tri = nullptr; uint32_t* em_q = nullptr; uint32_t* em_cum = nullptr;
  uint32_t em_n = 0, em_Q = 0;
  bool em_valid = false;
  // emitter index (the header's "Multiple importance sampling"): the table's (blasIdx, triIdx, e), three words per entry, sorted by
  // (blasIdx, triIdx, e).  Built by emitter_index_ensure from em_pairs -- the caller's list as the last set took it -- when a MIS frame or
  // vxrt_emitter_hit_weights first needs it; dropped by every set.  em_idx_n: its entries, 0 = none.
  std::vector<vxrt_emitter_t> em_pairs;
  uint32_t* em_idx = nullptr;
  uint32_t em_idx_n = 0;
};

// What the emitter-sampling kernels read of the table (rt_path.hip)
struct EmitterTab { const float* tri; const uint32_t* q; const uint32_t* cum; uint32_t n, Q; };
static inline EmitterTab emitter_tab(const vxrt_accel* a) { return EmitterTab{a->em_tri, a->em_q, a->em_cum, a->em_n, a->em_Q}; }
static inline bool emitters_valid(const vxrt_accel* a) { return a->em_valid && a->em_n != 0u && !a->stale; }
// ... and of the emitter index
struct EmitterIdx { const uint32_t* ent; uint32_t n; };
static inline EmitterIdx emitter_idx(const vxrt_accel* a) { return EmitterIdx{a->em_idx, a->em_idx_n}; }
// rt_accel.hip: the index of a valid table, built here if the accel holds none (one upload and one synchronisation of s; nothing when
// it is held).  0, or -1 when a HIP call failed.
int emitter_index_ensure(vxrt_accel* a, hipStream_t s);

// Environment map (vxrt_envmap_create, rt_env.hip; the definition is in the header, "Environment light"): n x n RGB texels of the
// octahedral unfolding, the quantised weight q of every texel and its inclusive prefix sum cum in texel order; Q = cum[n * n - 1].
// World-space directions only: nothing an accel does makes it stale.
struct vxrt_envmap { float* texels = nullptr; uint32_t* q = nullptr; uint32_t* cum = nullptr; uint32_t n = 0, Q = 0; };
// What the kernels read of it (rt_env.h), with the scale of the call
struct EnvTab { const float* texels; const uint32_t* q; const uint32_t* cum; uint32_t n, Q; float scale; };
static inline EnvTab env_tab(const vxrt_envmap* m, float scale) { return EnvTab{m->texels, m->q, m->cum, m->n, m->Q, scale}; }
// the checks of vxrt_env_params_t every door shares (rt_path.hip, rt_kernels.hip)
static inline bool env_params_ok(const vxrt_env_params_t* e) {
  return e->map && e->map->n != 0u && e->sample <= 1u && e->reserved == 0u && e->scale >= 0.0f && e->scale <= 3.402823466e+38f;
}

// What the previous-position guide reads besides the SceneDev (see the header, "Motion"): the snapshot's instance records, the vertices
// (the snapshot's, or the scene's current ones) and the two bounds a hit record is checked against
struct MotionSrc { const uint32_t* blas; const float* tri; uint32_t n_blas, n_tris; };
static inline MotionSrc motion_src(const vxrt_accel* a) {
  return MotionSrc{a->motion_blas, (a->motion_what & VXRT_REFIT_GEOMETRY) ? (const float*)a->motion_tri : (const float*)a->ref.tri, a->ref.n_blas, a->ref.n_tris};
}

// RT_IDENT_ROOT_KERNEL: accels whose TLAS root is one identity instance take frame kernels that compile the TLAS level out of the
// traversal loop (the IDENT template argument of rt_persistent_kernel).  0 = no such instantiations (the A/B: docs/KNOBS.md).
#ifndef RT_IDENT_ROOT_KERNEL
#define RT_IDENT_ROOT_KERNEL 1
#endif
// the accel's timed plain / shadow frames take the IDENT instantiations (as the accel is now: a refit may change ident_root and the decode)
static inline bool ident_root_form(const vxrt_accel* a) {
  return RT_IDENT_ROOT_KERNEL && a->dev.ident_root != 0u && a->shallow && !a->dev.exact_decode && !a->alpha_on;
}

// ---------------------------------------------------------------------------------------------
// shared device arithmetic: the RGB8 pack of every frame (rt_kernels.hip, rt_secondary.hip, rt_path.hip, rt_denoise.hip)
// ---------------------------------------------------------------------------------------------
// libstdc++ std::min (NaN behaviour is part of parity; std_max is in rt_shading.h)
__device__ __forceinline__ float std_min(float a, float b) { return (b < a) ? b : a; }
// int(f) as x86-64 converts it (the rule of include/vortex_hip.h, vxrt_shade_rays; f2u_x86 is in rt_shading.h)
__device__ __forceinline__ uint32_t f2i_x86(float f) { return (f >= -0x1p31f && f < 0x1p31f) ? (uint32_t)(int)f : 0x80000000u; }
__device__ __forceinline__ uint32_t pack_rgb8(float r, float g, float b) {  // common.h:149-154
  const uint32_t ir = f2i_x86(std_min(r, 1.f) * 255);   // (shifts and sums of the int's bits, mod 2^32: what the 32-bit registers hold)
  const uint32_t ig = f2i_x86(std_min(g, 1.f) * 255);
  const uint32_t ib = f2i_x86(std_min(b, 1.f) * 255);
  return (ir << 16) + (ig << 8) + ib;
}

// ---------------------------------------------------------------------------------------------
// rt_denoise.hip: what render_path_frame (rt_path.hip) checks before a denoised path frame is launched, and the two ends that
// render_path_tail (rt_path.hip) hands such a frame to.  The launches behind them, and their order, are that unit's own.
// ---------------------------------------------------------------------------------------------
struct RenderRequest;
// the checks of vxrt_denoise_params_t / vxrt_variance_params_t every entry point that takes one shares
bool dn_params_ok(const vxrt_denoise_params_t* dn);
bool vr_params_ok(const vxrt_variance_params_t* v);
// temporal accumulation: the parameters, and that the history is of the kind the entry point takes (moments: vxrt_render_path_variance
// takes one with moments, the others one without) and holds a window of `pixels` pixels
bool tp_request_ok(const vxrt_history_t* h, const vxrt_temporal_params_t* t, uint64_t pixels, bool moments = false);
// a camera whose every field is finite: what the entry points of both units that take a camera accept (rt_kernels.hip)
bool camera_ok(const vxrt_camera_t* c);
// End of a denoised path frame's tail in place of rt_path_final_kernel, for a frame with iterations or a history.  n = pixels of the window;
// the context holds the primary hits' P, N, Lit, Alb and the accumulators.  Demodulates into the context's signal buffers (grown here) and
// writes the guide outputs; then the temporal step, the initial variance and the a-trous passes as the request asks for them, the last
// launch of which remodulates, packs and writes dst / colors.  All asynchronous on the request's stream; 0, or -1 when a HIP call failed.
int render_denoise_tail(FrameCtx* c, const RenderRequest& r, uint32_t n);
// The guide outputs only (r.aov), one launch: the frame without iterations and without a history, which rt_path_final_kernel then ends.
int render_denoise_aov(FrameCtx* c, const RenderRequest& r, uint32_t n);

// ---------------------------------------------------------------------------------------------
// rt_kernels.hip <-> rt_secondary.hip, rt_path.hip: a frame as an entry point asks for it, the per-frame control block, growing device
// buffers, the ray-buffer launch the secondary tails trace with, the three tails render_common ends such a frame with and their knobs
// ---------------------------------------------------------------------------------------------
#ifndef QUEUE_SHARDS
#define QUEUE_SHARDS 8u     // one device-scope counter saturates near 90 dequeues/us
#endif
#define QUEUE_STRIDE 32u    // one 128-byte line per shard counter
// per-frame control block: [0] deferral count (own 128-byte line), then the queue counters of the main
// launch, of the EXACT launch over the deferred list and of the a-priori EXACT launch
#define CTL_QUEUE_DWORDS (QUEUE_SHARDS * QUEUE_STRIDE)
#define CTL_DWORDS (32u + 3u * CTL_QUEUE_DWORDS)

// Which build of the kernels a frame runs; the value is their STATS template argument (see rt_persistent_kernel)
enum class Counting { TIMED = 0, REFERENCE_ORDER = 1, TIMED_TRAVERSAL = 2 };

// One frame, or one set of frames, as the vxrt_render* entry points ask for it.  Every field defaults to "absent": an entry point
// sets the ones it means.
struct RenderRequest {
  uint32_t width = 0, height = 0, y0 = 0, y1 = 0;   // rows [y0, y1) of a width x height frame ...
  uint32_t stride = 1;                              // ... of which every stride-th tile row (8 rows), starting with the one at y0
  const vxrt_shade_params_t* params = nullptr;      // `batch` entries
  uint32_t batch = 1;                               // frames in this set of launches
  int shadow = 0;
  uint32_t* dst = nullptr; uint64_t dst_frame_stride = 0;   // frame f goes to dst + f * dst_frame_stride
  vxrt_hit_t* hits = nullptr; float* colors = nullptr;      // optional outputs, single frames
  unsigned long long* counters = nullptr;           // [0] rays traced; the counting builds: all of them
  uint32_t* unoccluded = nullptr;                   // ambient occlusion, optional
  unsigned long long* wave_log = nullptr;           // diagnostic, TIMED_TRAVERSAL only
  const vxrt_ao_params_t* ao = nullptr;             // ambient-occlusion or diffuse-bounce frame
  const vxrt_camera_t* cams = nullptr;              // camera frames: `batch` entries
  const vxrt_path_params_t* path = nullptr;         // path frame (vxrt_render_path)
  const vxrt_emissive_params_t* emissive = nullptr; // ... with emissive geometry (vxrt_render_path_emissive): a plain path frame otherwise
  const vxrt_emissive_mis_params_t* emissive_mis = nullptr; // ... with both estimators of emissive geometry, weighted (vxrt_render_path_emissive_mis)
  const vxrt_specular_params_t* specular = nullptr; // ... whose vertices may be specular (vxrt_render_path_frame_specular with enable = 1; null for enable = 0)
  const vxrt_roulette_params_t* roulette = nullptr; // ... whose dim paths end early (vxrt_render_path_frame_ex with enable = 1; null for enable = 0); never with `specular`
  const vxrt_env_params_t* env = nullptr;           // ... lit by an environment map (vxrt_render_path_frame_env); never with an emitter form or `specular`
  const uint32_t* sample_counts = nullptr;          // ... with a sample count per pixel (vxrt_render_path_adaptive): device, addressed like dst; path->spp is the cap
  const vxrt_denoise_params_t* denoise = nullptr;   // ... denoised (vxrt_render_path_denoised), with its optional guide outputs
  const vxrt_path_aov_t* aov = nullptr;
  const vxrt_temporal_params_t* temporal = nullptr; // ... with temporal accumulation before the filter (vxrt_render_path_temporal), into
  vxrt_history_t* history = nullptr;                //     this history
  bool motion = false;                              // ... through the accel's motion snapshot (vxrt_render_path_temporal_motion), with its
  float* prev_position = nullptr;                   //     optional guide output
  const vxrt_variance_params_t* variance = nullptr; // ... with moments in the history and the variance-guided filter (vxrt_render_path_variance),
  float* variance_out = nullptr;                    //     with its optional output V0
  void* stream = nullptr;
  Counting counting = Counting::TIMED;
  bool honours_alpha = false;                       // the entry point traces every ray of its frame through the accel's alpha table, if one is set
};
#define VXRT_AO_MODE_DIFFUSE_BOUNCE 1u   // internal: vxrt_ao_params_t::reserved

// What has to finish before a buffer that grows is freed.  Each caller passes its own rule, and the rules are correctness, not taste:
// a context's buffers are only read by work on the caller's stream (STREAM), an accel's tables by frames in flight on any stream (DEVICE).
enum class GrowSync { NONE, STREAM, DEVICE };
struct DevBuf { void** ptr; size_t bytes_per_entry; };
// Grow the device buffers that share the capacity *cap (in entries) to `need` entries.  Nothing happens when they hold that many; else
// the wait `sync` names, every old buffer freed, every new one allocated (contents are not kept).  false: a HIP call failed -- the
// buffers are then missing and *cap is 0, unless it was the wait that failed (nothing touched).
template <class C>
static bool grow_device(std::initializer_list<DevBuf> bufs, C* cap, uint64_t need, GrowSync sync, hipStream_t s) {
  if (*cap >= need) return true;
  if (sync == GrowSync::STREAM && hipStreamSynchronize(s) != hipSuccess) return false;
  if (sync == GrowSync::DEVICE && hipDeviceSynchronize() != hipSuccess) return false;
  for (const DevBuf& b : bufs) { (void)hipFree(*b.ptr); *b.ptr = nullptr; }
  *cap = 0;
  for (const DevBuf& b : bufs) if (hipMalloc(b.ptr, (size_t)need * b.bytes_per_entry) != hipSuccess) return false;
  *cap = (C)need;
  return true;
}

// internal mode of trace_on_ctx: any-hit rays whose hit records are only read as "blocked or not" (JOB_TRACE_UNORDERED)
constexpr int MODE_ANY_UNORDERED = 0x100;
// ray buffer -> hit records on frame context c (rt_kernels.hip)
int trace_on_ctx(vxrt_accel_t* a, FrameCtx* c, const float* rays, uint64_t n, const float* tmax, HitRec* hits, int mode, hipStream_t s,
                 const uint32_t* n_dev = nullptr, unsigned long long* stats_counters = nullptr, const uint32_t* order = nullptr);
// a request -> its frame (rt_kernels.hip): what every vxrt_render* entry point ends in, those of rt_path.hip too.  -1: refused before
// anything was launched, or a HIP call failed; 0: rendered, or an empty window
int render_common(vxrt_accel_t* a, const RenderRequest& r);

// rt_secondary.hip: what replaces the plain shading pass of a frame with reflective instances / an ambient-occlusion frame.
// utab / vtab: the tables the traversal used (a camera frame's: the head and the tables of its camera block).
// Each zeroes the context's control block in its first launch.  0, or -1 when a HIP call failed.
int render_bounce_tail(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const ShadeParams& p, const float* utab, const float* vtab);
int render_ao_tail(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const ShadeParams& p, const float* utab, const float* vtab);
// rt_secondary.hip: the three measurement knobs of the secondary tails (docs/KNOBS.md), read from the environment once per process, together
struct SecondaryKnobs {
  uint64_t path_batch;   // paths per batch of a path frame (see render_path_tail); VXRT_PATH_BATCH, default PATH_BATCH_PATHS
  uint64_t ao_batch;     // rays per batch of an ambient-occlusion frame (see render_ao_tail); VXRT_AO_BATCH, parsed as VXRT_PATH_BATCH is
  // VXRT_SORT_SECONDARY=1: trace the secondary rays in (direction octant, origin cell) order instead of generation order.  OFF by
  // default: measured SLOWER on both passes that used it then (diffuse bounce 1.53 -> 1.95 ms, 10M-triangle hairball AO 9.2 -> 16.6 ms,
  // profiles/r02_f_secondary_sort.txt).  The traversal is bound by per-lane VALU work, which coherence does not reduce, and the
  // generation order already puts the 16 samples of one pixel (AO) / 64 neighbouring pixels (bounce) side by side.
  bool sort_secondary;
};
const SecondaryKnobs& secondary_knobs();

// rt_path.hip: what replaces the plain shading pass of a path frame (denoised or not); as the two tails above
int render_path_tail(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const ShadeParams& p, const float* utab, const float* vtab);
extern const uint64_t PATH_BATCH_PATHS;   // paths per batch of a path frame unless VXRT_PATH_BATCH says otherwise
