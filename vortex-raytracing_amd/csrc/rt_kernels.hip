// HIP kernels of the ray-tracing hot path for gfx950 (MI355X): 4-wide quantized-BVH traversal
// (TLAS -> BLAS), Moller-Trumbore, Lambert shade, RGB8 pack.  Hand-written for CDNA4 wave64.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off   (contraction OFF is part of the
// contract: SURVEY.md s7 "FP contraction"; division and sqrt are the correctly rounded forms,
// hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt).  The only fused operation is the
// explicit fma in the child-box decode, where the product is exact (see eval_children).
//
// Semantics restated from the reference (paths relative to the reference repo):
//   traversal     sim/simx/rt_traversal.cpp:26-213 + sim/simx/rt_unit.cpp:98-116,199-202
//   box / tri     sim/simx/rt_traversal.cpp:318-339 / :263-316 ; instance transform :231-261
//   ray gen       tests/regression/raytracing/kernel.cpp:28-39
//   shading       shaders/closest.cpp:57-127, shaders/miss.cpp:9-14, rtx_shading.h:5-18,55-67
//   pixel pack    common.h:149-154, kernel.cpp:95-106
// The trail/short-stack/restart machinery of the simulator is replaced by one pass over a full
// per-lane stack whose entries carry m = max(entry distance along the path); DESIGN.md s3 proves
// this returns the same hit (index included) as the reference's accept-and-re-descend loop.
// What is not timed lives elsewhere: the acceleration-layout build and the refit in rt_accel.hip; the tails of the frames that trace
// secondary rays and their kernels in rt_secondary.hip (mirror bounce, ambient occlusion) and rt_path.hip (path frames, with their entry points), the a-trous
// filter in rt_denoise.hip; the two ray-compaction experiments (VXRT_POOL) in rt_trace_experiments.inc.  The shading arithmetic the frame
// kernels share with those tails (shade_terms, the camera rays, the sample rays) is in rt_shading.h; SceneDev, HitRec, ShadeParams,
// FrameCtx, vxrt_accel, RenderRequest and the seam to the other units in rt_internal.h; the constants of the compact layout in
// rt_types.h.
// Host half (behind the kernels): an entry point describes its frame in a RenderRequest; render_common checks it, prepares the frame
// context's resources, makes a LaunchPlan and launches -- no launch macros: the template arguments are picked by launch_traversal /
// launch_trace and with_decode_and_depth.  This unit's environment knobs are read once, into HostKnobs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_internal.h"
#include "pinhole.h"
#include "rt_shading.h"   // (up here for std_max, which the slab test below takes)
#include "rt_order.h"
#include "rt_tile_refill.h"
#include "rt_launch_plan.h"

// rt_traversal.cpp:318-339 with idir hoisted (1.0f/rd is recomputed per child there; same value).
// EXACT selects the libstdc++ min/max forms; the fast form uses v_min/v_max, which differs only
// when a NaN is present (0*inf), i.e. only if some ray direction component is 0/inf/NaN.
template <bool EXACT>
__device__ __forceinline__ float slab_interval(float tx1, float tx2, float ty1, float ty2, float tz1, float tz2) {
  float tmin, tmax;
  if (EXACT) {
    tmin = std_min(tx1, tx2);
    tmax = std_max(tx1, tx2);
    tmin = std_max(tmin, std_min(ty1, ty2));
    tmax = std_min(tmax, std_max(ty1, ty2));
    tmin = std_max(tmin, std_min(tz1, tz2));
    tmax = std_min(tmax, std_max(tz1, tz2));
  } else {
    tmin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));   // v_min x3, v_max3
    tmax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
  }
  return (tmax < tmin || tmax <= 0) ? RT_LARGE_FLOAT : tmin;
}

template <bool EXACT>
__device__ __forceinline__ float ray_box(float ox, float oy, float oz, float ix, float iy, float iz,
                                         float mnx, float mny, float mnz, float mxx, float mxy, float mxz) {
  float tx1 = (mnx - ox) * ix, tx2 = (mxx - ox) * ix;
  float ty1 = (mny - oy) * iy, ty2 = (mxy - oy) * iy;
  float tz1 = (mnz - oz) * iz, tz2 = (mxz - oz) * iz;
  return slab_interval<EXACT>(tx1, tx2, ty1, ty2, tz1, tz2);
}

// rt_traversal.cpp:263-316 on a wide triangle (v0, edge1, edge2)
__device__ __forceinline__ float ray_tri(float ox, float oy, float oz, float dx, float dy, float dz,
                                         float4 t0, float4 t1, float4 t2, float& bx, float& by, float& bz) {
  const float v0x = t0.x, v0y = t0.y, v0z = t0.z;
  const float e1x = t0.w, e1y = t1.x, e1z = t1.y;
  const float e2x = t1.z, e2y = t1.w, e2z = t2.x;
  float hx = dy * e2z - dz * e2y;
  float hy = dz * e2x - dx * e2z;
  float hz = dx * e2y - dy * e2x;
  float a = e1x * hx + e1y * hy + e1z * hz;
  if (fabsf(a) < RT_EPSILON) return RT_LARGE_FLOAT;
  float f = 1 / a;
  float sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
  float w1 = f * (sx * hx + sy * hy + sz * hz);
  if (w1 < 0 || w1 > 1) return RT_LARGE_FLOAT;
  float qx = sy * e1z - sz * e1y;
  float qy = sz * e1x - sx * e1z;
  float qz = sx * e1y - sy * e1x;
  float w2 = f * (dx * qx + dy * qy + dz * qz);
  if (w2 < 0 || w1 + w2 > 1) return RT_LARGE_FLOAT;
  float tf = f * (e2x * qx + e2y * qy + e2z * qz);
  if (tf <= RT_EPSILON) return RT_LARGE_FLOAT;
  bx = w1;
  by = w2;
  bz = 1 - w1 - w2;
  return tf;
}

// ray_tri without control flow: the same operations in the same order (the build contracts nothing), the four rejections evaluated as
// predicates in the polarity of the returns above -- a comparison with a NaN is false in both forms -- and one select at the end.  1 / a
// of a rejected lane may be inf or NaN; nothing that depends on it survives the select.  With no return between the loads of a
// triangle's three words and their uses, the loads issue together and the test waits for memory once.
__device__ __forceinline__ float ray_tri_flat(float ox, float oy, float oz, float dx, float dy, float dz,
                                              float4 t0, float4 t1, float4 t2, float& bx, float& by, float& bz) {
  const float v0x = t0.x, v0y = t0.y, v0z = t0.z;
  const float e1x = t0.w, e1y = t1.x, e1z = t1.y;
  const float e2x = t1.z, e2y = t1.w, e2z = t2.x;
  float hx = dy * e2z - dz * e2y;
  float hy = dz * e2x - dx * e2z;
  float hz = dx * e2y - dy * e2x;
  float a = e1x * hx + e1y * hy + e1z * hz;
  float f = 1 / a;
  float sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
  float w1 = f * (sx * hx + sy * hy + sz * hz);
  float qx = sy * e1z - sz * e1y;
  float qy = sz * e1x - sx * e1z;
  float qz = sx * e1y - sy * e1x;
  float w2 = f * (dx * qx + dy * qy + dz * qz);
  float tf = f * (e2x * qx + e2y * qy + e2z * qz);
  const bool rejected = (fabsf(a) < RT_EPSILON) | (w1 < 0 || w1 > 1) | (w2 < 0 || w1 + w2 > 1) | (tf <= RT_EPSILON);
  bx = w1;
  by = w2;
  bz = 1 - w1 - w2;
  return rejected ? RT_LARGE_FLOAT : tf;
}

// (Cand, cmpx, order_children -- the visiting order of a node's children -- and the selections of RT_ORDER_PATHS: rt_order.h)

template <int K>
__device__ __forceinline__ float qbyte(uint32_t w) { return (float)((w >> (8 * K)) & 0xffu); }   // v_cvt_f32_ubyteK

// Box test of child K of an internal node (rt_traversal.cpp:59-74).  pl[0..2] = the lo planes of x, y, z
// and pl[3..5] the hi planes, one byte per child.
// Decode: the reference computes origin + ldexp(float(q), e) (:61-67).  float(q) * 2^e is exact for
// an 8-bit q whenever 2^e is representable, so fma(float(q), 2^e, origin) rounds the same exact sum
// once and yields the identical float with one instruction less per coordinate.
// Fast form (!EXACT && !LDEXP): with q_lo <= q_hi the decoded planes, the differences to the origin and
// the products with 1/d are monotone, so min(t_lo, t_hi) IS the plane on the side the ray comes from:
// the caller selects the near/far plane words by the sign of 1/d once per node (6 selects for the four
// children) and the twelve v_min/v_max per child collapse into one v_max3 and one v_min3.  Both
// preconditions are verified per scene by the accel build, which sets exact_decode otherwise (LDEXP form).
template <int K, bool EXACT, bool LDEXP>
__device__ __forceinline__ float child_box(const uint32_t* pl, float px, float py, float pz, float sx, float sy, float sz,
                                           int ex, int ey, int ez, float rox, float roy, float roz, float rix, float riy, float riz) {
  float ax, ay, az, bx, by, bz;
  if (LDEXP) {
    ax = px + ldexpf(qbyte<K>(pl[0]), ex); ay = py + ldexpf(qbyte<K>(pl[1]), ey); az = pz + ldexpf(qbyte<K>(pl[2]), ez);
    bx = px + ldexpf(qbyte<K>(pl[3]), ex); by = py + ldexpf(qbyte<K>(pl[4]), ey); bz = pz + ldexpf(qbyte<K>(pl[5]), ez);
  } else {
    ax = __fmaf_rn(qbyte<K>(pl[0]), sx, px); ay = __fmaf_rn(qbyte<K>(pl[1]), sy, py); az = __fmaf_rn(qbyte<K>(pl[2]), sz, pz);
    bx = __fmaf_rn(qbyte<K>(pl[3]), sx, px); by = __fmaf_rn(qbyte<K>(pl[4]), sy, py); bz = __fmaf_rn(qbyte<K>(pl[5]), sz, pz);
  }
  const float tx1 = (ax - rox) * rix, tx2 = (bx - rox) * rix;
  const float ty1 = (ay - roy) * riy, ty2 = (by - roy) * riy;
  const float tz1 = (az - roz) * riz, tz2 = (bz - roz) * riz;
  if (EXACT || LDEXP) return slab_interval<EXACT>(tx1, tx2, ty1, ty2, tz1, tz2);
  const float tmin = fmaxf(fmaxf(tx1, ty1), tz1);   // pl[0..2] already hold the near planes
  const float tmax = fminf(fminf(tx2, ty2), tz2);
  return (tmax < tmin || tmax <= 0) ? RT_LARGE_FLOAT : tmin;
}
// The fast form (!EXACT && !LDEXP) of child_box without its select: the slab distance tmin whatever the test says, and the test's verdict
// in `enters` (the ray's interval with the box is not empty and not behind the origin).  eval_children_raw's NO_SELECT form.
template <int K>
__device__ __forceinline__ float child_box_raw(const uint32_t* pl, float px, float py, float pz, float sx, float sy, float sz,
                                               float rox, float roy, float roz, float rix, float riy, float riz, bool& enters) {
  const float ax = __fmaf_rn(qbyte<K>(pl[0]), sx, px), ay = __fmaf_rn(qbyte<K>(pl[1]), sy, py), az = __fmaf_rn(qbyte<K>(pl[2]), sz, pz);
  const float bx = __fmaf_rn(qbyte<K>(pl[3]), sx, px), by = __fmaf_rn(qbyte<K>(pl[4]), sy, py), bz = __fmaf_rn(qbyte<K>(pl[5]), sz, pz);
  const float tx1 = (ax - rox) * rix, tx2 = (bx - rox) * rix;
  const float ty1 = (ay - roy) * riy, ty2 = (by - roy) * riy;
  const float tz1 = (az - roz) * riz, tz2 = (bz - roz) * riz;
  const float tmin = fmaxf(fmaxf(tx1, ty1), tz1);
  const float tmax = fminf(fminf(tx2, ty2), tz2);
  enters = !(tmax < tmin || tmax <= 0);
  return tmin;
}

// RT_BOX_NO_SELECT: the box tests feed their verdict into ok[k] as a condition instead of selecting RT_LARGE_FLOAT into the distance and
// comparing that with the hit distance: one v_cndmask per child less.  The same ok[k]: hit_dist <= RT_LARGE_FLOAT (start_ray clamps it, and
// it only shrinks), so `RT_LARGE_FLOAT < hit_dist` is false and a missed box was never ok; where ok[k] holds the distance is tmin in both
// forms, and no caller reads the distance of a child that is not ok (eval_children and the ordered arm overwrite it with +inf, the occlusion
// arm pushes only children that are ok).  0 = the select (the A/B: docs/KNOBS.md).  Taken by the identity-root shadow frame kernels only
// (eval_children_raw's NO_SELECT): there it is worth +1.0 %; no other kernel gained with it in a measurement (the general
// kernels' figures with and without it: DESIGN.md s5, rejected), so every other kernel keeps the select.
#ifndef RT_BOX_NO_SELECT
#define RT_BOX_NO_SELECT 1
#endif

// Box tests of the <=4 children of an internal node, raw form: c[k].d is the slab distance whatever the test said, ok[k] says whether
// child k is to be visited (a real slot whose box the ray enters before its hit distance).
template <bool EXACT, bool LDEXP, bool NO_SELECT = false>
__device__ __forceinline__ void eval_children_raw(const uint4 q0, const uint4 q1, const uint4 q2, const uint4 q3, const uint32_t* __restrict__ ref_node,
                                                  float rox, float roy, float roz, float rix, float riy, float riz,
                                                  float hit_dist, Cand* c, bool* ok) {
  const float px = __uint_as_float(q0.x), py = __uint_as_float(q0.y), pz = __uint_as_float(q0.z);
  // plane scales 2^e as floats (fma decode); the ldexp decode takes the exponents from the reference node
  const float sx = __uint_as_float(q0.w), sy = __uint_as_float(q3.z), sz = __uint_as_float(q3.w);
  int ex = 0, ey = 0, ez = 0;
  if (LDEXP) {
    const uint32_t ew = ref_node[3];
    ex = (int)(int8_t)(ew & 0xff); ey = (int)(int8_t)((ew >> 8) & 0xff); ez = (int)(int8_t)((ew >> 16) & 0xff);
  }
  uint32_t pl[6] = {q1.x, q1.y, q1.z, q1.w, q2.x, q2.y};
  if (!EXACT && !LDEXP) {
    const bool nx = rix < 0, ny = riy < 0, nz = riz < 0;
    pl[0] = nx ? q1.w : q1.x; pl[3] = nx ? q1.x : q1.w;
    pl[1] = ny ? q2.x : q1.y; pl[4] = ny ? q1.y : q2.x;
    pl[2] = nz ? q2.y : q1.z; pl[5] = nz ? q1.z : q2.y;
  }
  const uint32_t desc[4] = {q2.z, q2.w, q3.x, q3.y};   // complete work descriptors, DESC_NONE for an empty slot (:60)
  float d[4];
  bool in[4] = {true, true, true, true};
  if constexpr (NO_SELECT) {
    static_assert(!EXACT && !LDEXP, "the select-free box test is the fast form's");
    d[0] = child_box_raw<0>(pl, px, py, pz, sx, sy, sz, rox, roy, roz, rix, riy, riz, in[0]);
    d[1] = child_box_raw<1>(pl, px, py, pz, sx, sy, sz, rox, roy, roz, rix, riy, riz, in[1]);
    d[2] = child_box_raw<2>(pl, px, py, pz, sx, sy, sz, rox, roy, roz, rix, riy, riz, in[2]);
    d[3] = child_box_raw<3>(pl, px, py, pz, sx, sy, sz, rox, roy, roz, rix, riy, riz, in[3]);
  } else {
    d[0] = child_box<0, EXACT, LDEXP>(pl, px, py, pz, sx, sy, sz, ex, ey, ez, rox, roy, roz, rix, riy, riz);
    d[1] = child_box<1, EXACT, LDEXP>(pl, px, py, pz, sx, sy, sz, ex, ey, ez, rox, roy, roz, rix, riy, riz);
    d[2] = child_box<2, EXACT, LDEXP>(pl, px, py, pz, sx, sy, sz, ex, ey, ez, rox, roy, roz, rix, riy, riz);
    d[3] = child_box<3, EXACT, LDEXP>(pl, px, py, pz, sx, sy, sz, ex, ey, ez, rox, roy, roz, rix, riy, riz);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if constexpr (NO_SELECT) ok[k] = (desc[k] != DESC_NONE) && in[k] && (d[k] < hit_dist);
    else ok[k] = (desc[k] != DESC_NONE) && (d[k] < hit_dist);     // :60, :71
    c[k].d = d[k];
    c[k].desc = desc[k];
  }
}

// ... and the form every caller but the frame kernel's occlusion arm takes: a child that is not to be visited carries +inf.
// (ok implies d < hit_dist <= RT_LARGE_FLOAT < inf, so `c[k].d < inf` IS ok[k], and a child that is visited carries its slab distance.)
template <bool EXACT, bool LDEXP>
__device__ __forceinline__ void eval_children(const uint4 q0, const uint4 q1, const uint4 q2, const uint4 q3, const uint32_t* __restrict__ ref_node,
                                              float rox, float roy, float roz, float rix, float riy, float riz,
                                              float hit_dist, Cand* c) {
  bool ok[4];
  eval_children_raw<EXACT, LDEXP>(q0, q1, q2, q3, ref_node, rox, roy, roz, rix, riy, riz, hit_dist, c, ok);
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k].d = ok[k] ? c[k].d : __builtin_inff();
}

// per-lane fetch counters of the STATS build (algorithmic bytes): what the
// reference logs in RT_mem_accesses (rt_traversal.cpp:54,116,148,158), without restart re-reads.
// A leaf or instance child still counts as one 52-byte node fetch: the reference reads that node.
struct Fetches { unsigned node = 0, inst = 0, tri = 0; };

#define ITER_LIMIT (1u << 22)   // backstop; accepted trees are acyclic (children stored after parents)

// LDS copy of the camera block's head (camera traversal kernels only: the fixed-camera instantiations never reference it)
template <int N>
__device__ __forceinline__ float* cam_lds() { __shared__ float s[N]; return s; }

#ifndef RT_TRI_PREFETCH
#define RT_TRI_PREFETCH 1
#endif
#ifndef RT_WAVES_PER_EU
#define RT_WAVES_PER_EU 6
#endif

// ---------------------------------------------------------------------------------------------
// Persistent traversal kernel.
//
// A fixed grid of wavefronts pulls jobs (pixels of 8x8 tiles, or rays of a ray buffer) from a
// sharded queue, so the launch ends within one job batch of the last job instead of within the
// slowest tile of a static tile->wavefront map (per-tile clocks showed half-empty CUs for the
// second half of a frame).  Idle lanes take new jobs once RT_DEAD_MAX (rendering) / RT_TRACE_DEAD_MAX
// (ray buffers) lanes of the wavefront are not traversing: 64 = whole tiles for rendering, because
// coherent camera rays lose more from sharing a wavefront with another tile than they gain from refilled
// lanes; 16 for incoherent ray buffers.  A tile's lanes trace the primary ray, then (shadow jobs) the
// occlusion ray of the same pixel; any-hit is a per-lane flag.
// Rendering is deferred: this kernel leaves 24-byte hit records, rt_shade_kernel makes pixels.
// Per-ray semantics -- and therefore results -- do not depend on the schedule.
// ---------------------------------------------------------------------------------------------
#ifndef RT_DEAD_MAX
#define RT_DEAD_MAX 64      // render jobs: leave the traversal loop (finish rays, fetch jobs) once this many lanes
#endif                      // are not traversing (finished or idle); 64 = whole-tile batches
#ifndef RT_LEAF_MIN
#define RT_LEAF_MIN 1          // render jobs: lanes of a tile reach their leaves together anyway
#endif
#ifndef RT_TRACE_LEAF_MIN
#define RT_TRACE_LEAF_MIN 24   // incoherent rays: +3.5 % at 16, another 1 % at 24
#endif
#ifndef RT_TRI_LDS
#define RT_TRI_LDS 0        // > 0: triangles of the leaf most lanes of the wavefront hold are staged through LDS (north_star: "triangle vertices staged
#endif                      // through LDS"): leaves of up to RT_TRI_LDS triangles, when at least RT_TRI_LDS_MIN lanes hold the same one.  Measured, off: DESIGN.md s5
#ifndef RT_TRI_LDS_MIN
#define RT_TRI_LDS_MIN 8
#endif
#ifndef RT_UNORDERED_OCCLUSION
#define RT_UNORDERED_OCCLUSION 1
#endif
#ifndef RT_SHADOW_FINISH_MIN
#define RT_SHADOW_FINISH_MIN 65   // > 64: off
#endif
#ifndef RT_TRACE_DEAD_MAX
#define RT_TRACE_DEAD_MAX 16   // ray-buffer jobs (incoherent rays): refill early
#endif
#ifndef RT_CHUNK
#define RT_CHUNK 64         // jobs reserved per global atomic (one 8x8 tile)
#endif
#ifndef RT_TRACE_NT
#define RT_TRACE_NT 0       // ray buffers: rays loaded and hit records stored with the streaming hint
#endif
#ifndef RT_TRACE_CHUNK
#define RT_TRACE_CHUNK 64   // ray buffers: jobs reserved per global atomic (rays have no screen neighbours to keep together)
#endif
#ifndef RT_XCC_HOME
#define RT_XCC_HOME 1         // a wavefront's home queue shard is its physical XCD (0 = blockIdx % 8, which names a group of blocks that share an XCD, not the XCD)
#endif
#ifndef RT_QUEUE_DRY_MASK
#define RT_QUEUE_DRY_MASK 1   // shards a wavefront found handed out are not polled again by the other wavefronts of its workgroup (LDS mask)
#endif
#ifndef RT_STEAL_SPREAD
#define RT_STEAL_SPREAD 0     // order in which a wavefront visits the other shards once its home shard is handed out: +1, +2, ... (0) or bit-reversed distance (1:
                              // the helpers of a drained band spread over the remaining ones; measured -1.4 % serial, +-0 elsewhere: profiles/r04_m_steal_spread_ab.txt)
#endif
// (QUEUE_SHARDS and the layout of the per-frame control block: rt_internal.h)
// Frames (camera tiles + their occlusion rays): 7 wavefronts per SIMD (72 VGPRs, 6 stack levels in LDS).  With frames traced in
// batches -- many tiles per wavefront, so ramp and tail of a launch no longer decide -- occupancy pays: 7 / 8 wavefronts are +5.3 /
// +5.6 % on the headline frame (one frame per launch: +-1 %, measured in round 2), 8 loses 3 % on serial frames, 7 gains 2 %
// there.  Ray buffers (JOB_TRACE): 7 wavefronts with 7 LDS levels -- they need one context slot less, which pays for the seventh
// level -- +2.5 % on random rays, hairball AO and diffuse bounce unchanged (with 6 levels AO lost 2 %): profiles/r02_o_occupancy.txt.
#ifndef RT_WAVES_TRACE
#define RT_WAVES_TRACE 7
#endif
#ifndef RT_LDS_STACK_TRACE
#define RT_LDS_STACK_TRACE 7
#endif
#ifndef RT_WAVES_RENDER
#define RT_WAVES_RENDER 7
#endif
#ifndef RT_LDS_STACK_RENDER
#define RT_LDS_STACK_RENDER 6
#endif
#ifndef RT_WAVES_RENDER_PACKED
#define RT_WAVES_RENDER_PACKED 8
#endif
#ifndef RT_LDS_STACK_RENDER_PACKED
#define RT_LDS_STACK_RENDER_PACKED 5
#endif
#ifndef LDS_STACK
#define LDS_STACK 8         // stack levels kept in LDS per lane (4 KiB per wavefront); deeper ones go to scratch
#endif
#ifndef RT_WG_WAVES
#define RT_WG_WAVES 4       // wavefronts per workgroup of the persistent kernels (the staged top of the tree is shared by them)
#endif
#define RT_WG_THREADS (64 * RT_WG_WAVES)

// JOB_TRACE_UNORDERED: a ray buffer of any-hit rays whose caller only wants "blocked or not" (ambient occlusion, the occlusion rays of a
// bounce level): JOB_TRACE's kernel with the children visited in slot order, as the frame's occlusion rays are (no sorting by distance,
// no path maxima).  vxrt_trace's VXRT_MODE_ANY returns the reference's FIRST accepted candidate and keeps JOB_TRACE.
enum { JOB_RENDER = 0, JOB_RENDER_SHADOW = 1, JOB_TRACE = 2, JOB_RENDER_GI = 3, JOB_TRACE_UNORDERED = 4 };
__host__ __device__ constexpr bool is_trace_job(int job) { return job == JOB_TRACE || job == JOB_TRACE_UNORDERED; }
// JOB_CAM: a render job seen from a caller-supplied pinhole camera (vxrt_render_camera) instead of the fixed GenerateRay: its own
// instantiations, so the fixed-camera kernels do not change.  JOB_RENDER | JOB_CAM, JOB_RENDER_SHADOW | JOB_CAM and
// JOB_RENDER_GI | JOB_CAM (vxrt_render_diffuse_bounce_camera); job_base() names the job without the bit.
// JOB_NOHINTS: the shadow frame job of a launch that carries no shadow hints (RT_SHADOW_HINTS below: the host knob is off, or the accel has
// no path table) -- its own instantiations of the three kernels that know hints, WITHOUT them: such a launch runs the kernel it ran before
// hints existed, instruction for instruction.  No other job is instantiated with the bit.
enum { JOB_CAM = 8, JOB_NOHINTS = 16 };
__host__ __device__ constexpr int job_base(int job) { return job & ~(JOB_CAM | JOB_NOHINTS); }
__host__ __device__ constexpr bool is_cam_job(int job) { return (job & JOB_CAM) != 0; }
// JOB_RENDER_GI: the whole "one diffuse bounce" frame (BASELINE configs[2] as worded; recipe: oracle/rt_oracle.c:orc_render_gi) in ONE
// persistent launch -- a lane traces its pixel's primary ray, shades the hit (closest.cpp's else arm), draws the pixel's bounce ray
// (ao_sample_ray, sample 0 of 1), traces it for its closest hit in the same lane, shades that hit and writes the pixel:
// colour = Lambert(primary) + albedo(primary) * Lambert(bounce hit | background).  Before, the frame was a primary launch, a pass that
// listed the hit pixels, a ray-generation pass, a 2 M-ray trace launch (a short launch with a long tail: 0.61 of the frame's 1.17 ms),
// an accumulation pass and a final pass.
#ifndef RT_WAVES_GI
#define RT_WAVES_GI 7
#endif
#ifndef RT_LDS_STACK_GI
#define RT_LDS_STACK_GI 6
#endif
#ifndef RT_GI_DEAD_MAX
#define RT_GI_DEAD_MAX 64    // (lanes refilled one by one: 16 -> 1.50 ms, 32 -> 1.45, 8 -> 1.72 against 1.18 with whole tiles: profiles/r03_f_gi_fused_ab.txt)
#endif

// RT_BATCH_PUSH: the children a node step leaves pending go onto the lane's stack in ONE operation (push_pending: one count, one
// LDS-or-scratch decision, sp and the register top set once) instead of one push() per child; pop_next() refills the register top outside
// its re-filter loop; the loop's exit test takes one ballot in the common case.  0 = the per-child form (the A/B: docs/KNOBS.md).
#ifndef RT_BATCH_PUSH
#define RT_BATCH_PUSH 1
#endif
// RT_LEAF_FLAT: the triangle test of the plain / shadow frame jobs in its straight-line form (ray_tri_flat: the triangle's 48 bytes arrive
// in one memory round trip instead of two, the four early returns are one select): +1.1 % on the headline frame.  0 = ray_tri (the A/B:
// docs/KNOBS.md).  Ray buffers, the diffuse-bounce job, the EXACT launch and the alpha-tested instantiations keep ray_tri whatever the
// value.  (The triangle LOOP without per-lane control flow -- the leaf lanes of a wavefront walking their leaves in step, a lane that is
// through re-reading its first triangle -- was built on top of it and lost 3 % against this form: DESIGN.md s5, rejected.)
#ifndef RT_LEAF_FLAT
#define RT_LEAF_FLAT 1
#endif
// RT_OCC_OK_MASKS: the occlusion arm of the timed plain / shadow frame jobs' node step takes the validity of the four children from the box
// tests themselves (eval_children_raw) instead of from `d < inf` on distances that were set to +inf for that purpose, and pushes the raw
// distance: 4 selects and 4 compares less per occlusion-ray step, +1.3 % on the headline frame.  0 = the form before (the A/B: docs/KNOBS.md).
// Ray buffers, the diffuse-bounce job, the EXACT launch, the alpha-tested and the counting instantiations keep eval_children whatever the value.
#ifndef RT_OCC_OK_MASKS
#define RT_OCC_OK_MASKS 1
#endif
// RT_OCC_LOOP: the timed shadow frame job's identity-root kernels hold the traversal loop twice, and a wavefront in which every lane that holds work holds
// an any-hit ray (a tile whose primary rays all hit, in its second half) takes the occlusion-only form: the node step is the occlusion arm
// alone (no phase ballot, no ordered arm, no path_m), stack entries are the 4-byte descriptor (twice the levels in the same LDS), pop_next
// takes the top without the re-filter, an accepted candidate ends the ray.  A mixed wavefront takes the general loop.  Same results, same
// visiting order.  0 = one loop (the A/B: docs/KNOBS.md).  Needs RT_BATCH_PUSH, RT_OCC_OK_MASKS, RT_UNORDERED_OCCLUSION and whole-tile batches
// (RT_DEAD_MAX 64, RT_SHADOW_FINISH_MIN off); the general (non-identity-root) kernels, ray buffers, the diffuse-bounce job, the EXACT launch,
// the alpha-tested and the counting instantiations keep the one loop whatever the value.
#ifndef RT_OCC_LOOP
#define RT_OCC_LOOP 1
#endif
#ifndef RT_OCC_LOOP_CHECK
#define RT_OCC_LOOP_CHECK 0
#endif
// RT_ORDER_PATHS: the ordered arm of the node step asks, once per run and for the whole wavefront (a scalar test on the box tests' masks),
// whether any of its lanes holds more than one valid child.  Where none does -- half of the ordered runs of the headline frame
// (profiles/r19_a_child_counts.txt) -- the run skips the +inf selects, the sorting network and the push: a lane with a valid child goes on
// with it (cur, path_m), a lane with none pops; the overflow test stays in front of every step that holds a valid child.  Same results
// (rt_order.h; tests/test_order_paths_cpu.py; RT_ORDER_CHECK in the variant library).  0 = the network always (docs/KNOBS.md).
// Taken by the identity-root shadow frame kernels (fixed and caller camera, 7 and 8 wavefronts), where it is measured and the loops'
// listings stay free of spills and lane moves; every other kernel keeps the network whatever the value (DESIGN.md s5 says why).
#ifndef RT_ORDER_PATHS
#define RT_ORDER_PATHS 1
#endif
// -DRT_ORDER_CHECK=1 (variant libraries only): a run that skips the network evaluates it as well; a difference sets STATUS_ITER_LIMIT
#ifndef RT_ORDER_CHECK
#define RT_ORDER_CHECK 0
#endif
// RT_SHADOW_HINTS: the occlusion-only loop descends first along the path of the triangle that blocked the same pixel's occlusion ray in
// the context's frame before.  The accel holds one 32-bit path code per triangle (accel_path_kernel, rt_accel.hip: the child slot taken at
// each internal level from the BLAS root to the triangle's leaf, 2 bits per level, root in the low bits), the frame context one hint word
// per hit-record slot (the blocker's triangle index, 0xFFFFFFFF = none).  A lane that starts an occlusion ray reads its hint and, if it
// names a triangle, that triangle's code: while the lane is "guided" (F_GUIDED) a node step takes the child in the hinted slot if its box
// test passed and pushes the other valid children in slot order; a hinted slot that failed, or the lane's first pop, ends the guidance.
// This only chooses a visiting order: the set of triangles an any-hit traversal can reach does not depend on it (RT_UNORDERED_OCCLUSION),
// so the occlusion bit is the same whatever the hints hold -- stale, hostile or none.  A blocked ray leaves its blocker in the hint word.
// No register is added: the occlusion-only loop has no use for path_m, which carries the code (and, once the ray is blocked, the blocker).
// The three kernels that hold the occlusion-only loop only; 0 = their listings are the parent form's.  Host knob VXRT_SHADOW_HINTS=0/1.
#ifndef RT_SHADOW_HINTS
#define RT_SHADOW_HINTS 1
#endif
// -DRT_SHADOW_HINT_COUNT=1 (variant libraries only; in build.py's TEST_VARIANT_FLAGS): the hinted kernels count their blocked occlusion rays
// and the ones that stopped while guided (g_hint_counts, two atomics per wavefront and finish section)
#ifndef RT_SHADOW_HINT_COUNT
#define RT_SHADOW_HINT_COUNT 0
#endif
// RT_TILE_PHASES: in the kernels that hold the occlusion-only loop (OCC_LOOP) a wavefront keeps a tile's primary and occlusion phases apart:
// the fetch section hands out jobs only when no lane of the wavefront holds work.  The parent form handed them to whatever lanes were idle,
// and every shadow tile leaves some idle behind its primary phase wherever a pixel misses, belongs to the a-priori EXACT list, is
// defer()ed or lies outside the window: those lanes took the next tile's first primary rays beside this tile's occlusion rays, the rest of
// that tile went to the other lanes at the next finish, and the wavefront stayed shifted by part of a tile -- both kinds of ray in every
// pass, the general loop's ordered arm for all of them, no hints -- for as long as it lived.  With whole-tile phases those lanes stay idle
// through the tile's occlusion phase, as they are through its primary phase.  Which lane traces a job never entered a result, and an
// occlusion ray's answer does not depend on the visiting order: same records, same rays.  Queue reservation, tile-cost accounting, the
// end of the queue, DEAD_MAX and FINISH_MIN are untouched.  0 = every kernel's listing is the parent form's; every kernel without the
// occlusion-only loop is the parent form's at either value.
// RT_TILE_REFILL_MIN: the number of idle lanes from which a partial refill is still taken in those kernels (the one trade: a tile in which
// many lanes miss runs its occlusion phase with those lanes empty).  65 = never (a wavefront all of whose lanes are idle always fetches),
// 1 = the parent form's behaviour.  Shipped: 32 -- a wavefront at least half of whose lanes are idle is refilled as before (a frame whose
// every tile is half background lost 1.9 % with 65 and nothing with 32 or 16); a tile that leaves fewer lanes idle keeps its phases apart
// (the headline's a-priori lines, most silhouette tiles, narrow window edges).  Behind a tile that leaves 32 or more idle the wavefront
// is shifted again and, in full tiles, stays so (tests/tile_phases_check.cpp replays it; the bunny-class frame keeps 16 mixed passes of
// 24,585).  DESIGN.md s5 has the table.  The rule itself is rt_tile_refill.h.  The test variant library is built with 65, where "no pass
// holds both kinds of ray" is an invariant that RT_OCC_LOOP_CHECK and the counters hold.
#ifndef RT_TILE_PHASES
#define RT_TILE_PHASES 1
#endif
#ifndef RT_TILE_REFILL_MIN
#define RT_TILE_REFILL_MIN 32
#endif
// -DRT_PHASE_COUNT=1 (variant libraries only; in build.py's TEST_VARIANT_FLAGS): the kernels that hold the occlusion-only loop count, per
// wavefront, their passes through a loop form and the node-body runs inside them (g_phase_counts, added up once per wavefront at its end)
#ifndef RT_PHASE_COUNT
#define RT_PHASE_COUNT 0
#endif
// (RT_IDENT_ROOT_KERNEL, rt_internal.h: the IDENT instantiations of rt_persistent_kernel)

// -DRT_ISA_MARKS: comment-only markers in the listing (hipcc -S) that delimit the regions of the traversal loop for
// tools/isa_regions.py and tools/isa_sections.py; never set for a build that is run
#ifdef RT_ISA_MARKS
#define RT_MARK(name) asm volatile("; RTMARK " name)
#else
#define RT_MARK(name)
#endif
// marks inside the traversal loop, which a kernel may hold in two forms (RT_OCC_LOOP): those of the occlusion-only form carry the prefix occ_
#define RT_LOOP_MARK(name) do { if constexpr (OCC) { RT_MARK("occ_" name); } else { RT_MARK(name); } } while (0)

// (hit_index, rt_shading.h: hit records of a frame window are kept TILE-MAJOR between the traversal and the shading pass)
// frame row of local row lr: the window's k-th tile row is frame rows y0 + k * row_step ... + 7 (row_step = 8 for a contiguous
// window, 8 * stride for the interleaved tile rows of vxrt_render_interleaved)
__device__ __forceinline__ uint32_t frame_row(uint32_t lr, uint32_t y0, uint32_t row_step) { return y0 + (lr >> 3) * row_step + (lr & 7u); }

// Division of a tile index (< 2^25: render_common refuses larger launches) by a divisor that is the same for the whole launch -- tiles per row,
// tiles per frame of a batch -- as a multiply-high, an add and a shift with constants the host derives once (Granlund & Montgomery 1994:
// L = ceil(log2 d), m = floor(2^32 (2^L - d) / d) + 1, x / d = (mulhi(x, m) + x) >> L; the sum cannot overflow for x < 2^31).  The compiler's
// own expansion of x / d for a runtime d is a float reciprocal + two correction steps, ~20 VALU instructions per division and a hoisted
// reciprocal per divisor held in a VGPR for the whole kernel; a lane derives its pixel from its job three times per pixel.
struct FastDiv { uint32_t d, m, s; };
static FastDiv fast_div_make(uint32_t d) {
  FastDiv f{d ? d : 1u, 1u, 0u};
  while ((1ull << f.s) < f.d) ++f.s;
  f.m = (uint32_t)((((1ull << f.s) - f.d) << 32) / f.d) + 1u;
  return f;
}
__device__ __forceinline__ uint32_t fast_div(uint32_t x, const FastDiv& f) { return (__umulhi(x, f.m) + x) >> f.s; }

struct PersistArgs {
  uint32_t W, H, y0, y1, tiles_x;
  FastDiv div_tiles_x, div_frame_tiles;   // (tiles_x, frame_tiles as divisors: see FastDiv)
  uint32_t row_step;              // frame rows between two consecutive tile rows of the window: 8, or 8 * stride (interleaved)
  uint32_t total;                 // number of jobs (tiles*64 pixels, or rays); an upper bound when total_dev is set
  const uint32_t* total_dev;      // optional: the job count lives in device memory (produced by an earlier kernel of the stream)
  HitRec* hits;                   // render: W*H hit records (occlusion in bit 31 of blasIdx); trace: n records
  const float* rays; const float* tmax; int any_hit;   // trace inputs
  const uint32_t* order;          // trace, optional: queue position -> ray id (rays binned by origin cell and direction octant)
  unsigned long long* counters;   // [0] rays (+ STATS: [1..4])
  uint32_t* status;
  uint32_t* queue;                // QUEUE_SHARDS counters (QUEUE_STRIDE dwords apart), zeroed by the host before the launch
  uint32_t per_shard;             // jobs per shard (multiple of 64)
  const float* utab; const float* vtab;   // camera u per column, v per row (see generate_ray)
  // rays whose slab products can be NaN (a zero / non-finite direction component) are not traced by
  // the main launch: their job id (bit 31 = occlusion phase) is appended here and a second, small
  // launch of the EXACT variant (libstdc++ min/max forms) traces them
  uint32_t* defer_count; uint32_t* defer_list; uint32_t defer_cap;
  // render jobs, optional: longest-processing-time-first order learned from the previous frame of this context
  // (tile_order[queue position] = tile, sorted by cost within each shard's band) and where this frame's cost goes
  const uint32_t* tile_order; uint32_t* tile_cost;
  uint32_t shard_rot;             // diagnostic (VXRT_SHARD_ROT): home shard of block b = (b + shard_rot) % QUEUE_SHARDS
  unsigned long long* wave_log;   // STATS only, optional: 16 u64 per wavefront (see vxrt_render_wave_log in the header)
  // optional, every build (the TIMED kernels too: one store per wavefront when it ends, nothing inside the loop): 2 u64 per wavefront of the main
  // launch -- [0] the constant 100 MHz clock at its end, [1] rays it started | physical XCD << 56 (vxrt_debug_end_log; tools/xcd_tail.py)
  unsigned long long* end_log;
  // batch of frames in one launch (vxrt_render_interleaved_batch): the window's tiles repeat `frame_tiles` apart, frame f = tile /
  // frame_tiles is shaded and lit with pbatch[f]; nullptr = one frame
  const ShadeParams* pbatch; uint32_t frame_tiles;
  // JOB_RENDER_GI: the frame itself (pixel (x, y) at dst[x + y * W]), optional f32 colours, seed of the bounce rays
  // -- and, in their place in a timed plain / shadow frame launch (which has no use for them; the block keeps its size and every other member
  // its offset), RT_SHADOW_HINTS' three words, read by the kernels with the occlusion-only loop only: the accel's path code per triangle, the
  // context's hint words (indexed like `hits`; nullptr = off for this launch), the number of triangles (a hint at or above it names none)
  union { uint32_t* dst; const uint32_t* tri_path; };
  union { float* colors; uint32_t* hints; };
  union { uint32_t gi_seed; uint32_t n_path_tris; };
  // ALPHA instantiations only (vxrt_accel_set_alpha_test): per triangle, the threshold of its material (0 = opaque)
  const uint8_t* alpha_tri;
};

// Domain of the fast (non-EXACT) traversal: every component of 1/d finite, non-zero and at most 2^64 in magnitude, every origin
// component at most 2^60.  The accel build holds node planes to 2^60 as well (else the scene runs the LDEXP instantiation), so
// a slab value (plane - o) * (1/d) stays below 2^125: finite, never NaN.  Rays outside go to the EXACT launch, which evaluates
// the reference's min/max chains literally.  (Comparisons with NaN are false, so NaN / inf components fail these tests.)
#define RT_FAST_INV_MAX 0x1p+64f
#define RT_FAST_POS_MAX 0x1p+60f
__device__ __forceinline__ bool ray_in_fast_domain(float ox, float oy, float oz, float ix, float iy, float iz) {
  return fabsf(ix) <= RT_FAST_INV_MAX && fabsf(iy) <= RT_FAST_INV_MAX && fabsf(iz) <= RT_FAST_INV_MAX && ix != 0.0f && iy != 0.0f && iz != 0.0f &&
         fabsf(ox) <= RT_FAST_POS_MAX && fabsf(oy) <= RT_FAST_POS_MAX && fabsf(oz) <= RT_FAST_POS_MAX;
}

// (vmax_nonan, the one-instruction max of two values neither of which is a NaN: rt_order.h)

// per-lane flag bits
#define F_FOUND 1u
#define F_ANYHIT 2u
#define F_SHADOW 8u      // render job is in its occlusion-ray phase
#define F_WORLD 16u      // the active ray registers hold the world-space ray (TLAS level)
#define F_RESUMED 32u    // EXACT launch: occlusion ray handed over by the main launch (its primary hit record is in memory)
#define F_GUIDED 64u     // RT_SHADOW_HINTS: the lane's occlusion ray still follows its hint's path code, which path_m holds (bit pattern)
#define F_HINTW 128u     // RT_SHADOW_HINTS: the lane's occlusion ray was blocked in the occlusion-only loop; path_m holds the blocker's triangle index

// Register budget is the lever here (profiles/r01_c_*: at 4 waves/SIMD the VALU pipe idles 58 % of
// the time waiting on dependent loads), so a lane keeps in VGPRs only what every step touches: the
// ACTIVE ray (origin + reciprocal direction; world space at TLAS level, object space inside an
// instance), hit distance, path_m, the current work item and the register-cached stack top.  The ray
// direction (triangle tests only), barycentrics / indices of the best hit and blasIdx live in LDS
// next to the stack; the world ray is not stored at all - it is re-derived from the job (ray buffer,
// camera tables, or the pixel's primary hit record) on the rare TLAS-level steps.
// STATS: 0 = the timed kernel; 1 = counting build in the reference's order (ordered occlusion, no leaf helpers: its fetch counts equal
// the canonical restatement's); 2 = counting build of the traversal the timed kernel actually performs (unordered occlusion, helpers)
// PACKED: the instantiation for frames traced in sets that overlap on two streams (bench.py's pipelined mode, batches): 8 wavefronts
// per SIMD (64 VGPRs, 5 stack levels in LDS) instead of 7 -- +1.6 % there, where many tiles per wavefront hide the few spilled
// registers, and -8 % on a serial frame, which keeps 7 (profiles/r03_c_flag_variants.txt)
// SHALLOW: the scene's trees are at most RT_SHALLOW_LEVELS internal levels deep on any root-to-leaf path, TLAS and BLAS together (measured by the
// accel build, accel_depth_kernel), so a lane's stack never holds more than 3 x RT_SHALLOW_LEVELS entries and the part of it that lives in
// scratch is sized for that instead of for the reference's 32 levels: 344 instead of 768 bytes per lane for the 8-wavefront instantiation.
// (The 1,048,576-triangle atrium is 13 levels deep, the 10 M-triangle hairball 15.)  Timed builds only; deeper scenes take the full-size form.
// ALPHA: candidates pass the alpha test before they are accepted (vxrt_accel_set_alpha_test; A.alpha_tri).  Timed builds of the ray-buffer
// and plain / shadow frame jobs only, one value of the speed-only axes (PACKED and SHALLOW false).  With ALPHA false nothing of it is compiled.
// IDENT: the accel's TLAS root is one instance whose inverse transform is the identity (sc.ident_root, checked by the accel build and by every
// refit).  start_ray then puts every ray at BLAS level -- at the BLAS root with its world coordinates, or, for an origin component that is -0,
// through enter_instance -- and nothing ever brings a lane back: no lane holds a TLAS node or an instance descriptor inside the loop, whose
// instance step, "back at TLAS level" test and the ballots that go with them are not compiled.  Timed plain / shadow frame jobs of shallow
// scenes with the fma decode only (launch_traversal); every other scene keeps the general kernels.
// diagnostic (vxrt_debug_child_counts): node-body runs of the wave-log launches on this device by the largest number of valid children any
// node lane of the run holds -- [0..3] ordered arm with 0, 1, 2, >= 3, [4..7] occlusion arm -- summed over their wavefronts
__device__ unsigned long long g_child_counts[8];
// diagnostic (vxrt_debug_shadow_hint_counts; -DRT_SHADOW_HINT_COUNT=1 libraries only): occlusion rays of hinted launches that finished in the
// main kernel blocked, and those of them that were blocked in the occlusion-only loop while still guided (no failed hinted slot, no pop)
__device__ unsigned long long g_hint_counts[2];
// diagnostic (vxrt_debug_phase_counts; -DRT_PHASE_COUNT=1 libraries only): passes of the wavefronts of the kernels that hold the
// occlusion-only loop through [0] that form, [1] the general form with no any-hit lane, [2] the general form holding both kinds of ray (a
// pass is classed where it enters the loop); [3..5] the node-body runs inside them, a run of the general form classed by the lanes that
// hold work when it starts
__device__ unsigned long long g_phase_counts[6];

template <int JOB, int STATS, bool LDEXP, bool EXACT, bool PACKED = false, bool SHALLOW = false, bool ALPHA = false, bool IDENT = false>
__global__ __launch_bounds__(EXACT ? 256 : RT_WG_THREADS, EXACT ? 4 : (is_trace_job(JOB) ? RT_WAVES_TRACE : (job_base(JOB) == JOB_RENDER_GI ? RT_WAVES_GI : (PACKED ? RT_WAVES_RENDER_PACKED : RT_WAVES_RENDER)))) void rt_persistent_kernel(SceneDev sc, ShadeParams p, PersistArgs A) {
  static_assert(!ALPHA || (STATS == 0 && !PACKED && !SHALLOW && job_base(JOB) != JOB_RENDER_GI), "alpha instantiations: see ALPHA above");
  static_assert(!IDENT || (STATS == 0 && !ALPHA && !EXACT && !LDEXP && SHALLOW && (job_base(JOB) == JOB_RENDER || job_base(JOB) == JOB_RENDER_SHADOW)), "identity-root instantiations: see IDENT above");
  // stack levels in LDS: what the instantiation's occupancy leaves room for (160 KB per CU)
  constexpr int LSTK = EXACT ? LDS_STACK : (is_trace_job(JOB) ? RT_LDS_STACK_TRACE : (job_base(JOB) == JOB_RENDER_GI ? RT_LDS_STACK_GI : (PACKED ? RT_LDS_STACK_RENDER_PACKED : RT_LDS_STACK_RENDER)));
  constexpr int WG_WAVES = EXACT ? 4 : RT_WG_WAVES;
  constexpr bool USE_TOP = RT_TOP_NODES > 0 && !EXACT && !LDEXP;   // (the ldexp decode reads exponents from the reference node by index)
  constexpr uint32_t DEAD_MAX = is_trace_job(JOB) ? RT_TRACE_DEAD_MAX : (job_base(JOB) == JOB_RENDER_GI ? RT_GI_DEAD_MAX : RT_DEAD_MAX);
  // render-with-shadow jobs: retire finished primary rays (their lanes continue with the occlusion ray
  // of the same pixel - same traversal code, so no phase mixing) before the whole tile is done
  constexpr uint32_t FINISH_MIN = job_base(JOB) == JOB_RENDER_SHADOW ? RT_SHADOW_FINISH_MIN : 65u;
  const uint32_t lane = threadIdx.x & 63u;
  // EXACT launch: the jobs are the entries of the deferral list the main launch left behind
  const uint32_t n_jobs = EXACT ? min(*A.defer_count, A.defer_cap) : (A.total_dev ? min(*A.total_dev, A.total) : A.total);
  const uint32_t per_shard = (EXACT || A.total_dev) ? (((n_jobs + QUEUE_SHARDS - 1) / QUEUE_SHARDS + 63u) & ~63u) : A.per_shard;

  __shared__ uint2 s_stk[WG_WAVES][LSTK][64];   // stack levels below the register top, 8 B entries, conflict-free rows
  // 0-2 active dir, 3-4 hit bx/by (bz = 1 - bx - by is re-derived when the record is written), 5 distance of the pixel's
  // primary hit while its occlusion ray is traced, 6 hit blasIdx, 7 hit triIdx, 8 blasIdx
  // (ray buffers have no "primary hit kept while the occlusion ray runs": slot 5 is dropped there, 8 slots + 7 stack levels fit 7 workgroups per CU)
  constexpr int NCTX = (!EXACT && is_trace_job(JOB)) ? 8 : 9;
  __shared__ uint32_t s_ctx[WG_WAVES][NCTX][64];
  __shared__ uint32_t s_dry;      // bit s: a wavefront of this workgroup found queue shard s handed out
  if (threadIdx.x == 0) s_dry = 0u;
  // camera frames: the cameras live in LDS (wave-uniform data; a lane reads its frame's camera when it derives a ray)
  float* s_cam = nullptr;
  if constexpr (is_cam_job(JOB)) {
    s_cam = cam_lds<CAM_TAB>();
    for (uint32_t i = threadIdx.x; i < (uint32_t)CAM_TAB; i += blockDim.x) s_cam[i] = A.utab[i];
  }
  __syncthreads();
  uint2* const lstk = &s_stk[threadIdx.x >> 6][0][lane];
  // the same rows as 2 * LSTK rows of 64 dwords (occlusion-only loop).  Formed where it is used, from the lane number through an empty asm
  // statement: as a value of its own it is one more register alive for the whole kernel, which the 8-wavefront kernels reload from scratch
  // in front of every stack access.
  auto lstk4_here = [&]() -> uint32_t* {
    uint32_t l = lane;
    asm volatile("" : "+v"(l));
    return (uint32_t*)lstk - l;
  };
  uint32_t* const ctx = &s_ctx[threadIdx.x >> 6][0][lane];
#define CTX(i) ctx[((NCTX == 8 && (i) > 5) ? (i) - 1 : (i)) * 64]
  // top of the tree staged in LDS (north_star: "BVH nodes staged through LDS"): the first levels are what every ray of every
  // tile walks, and a ds_read_b128 does not queue behind the CU's vector-memory pipeline
  __shared__ uint4 s_top[USE_TOP ? 4 : 1][USE_TOP ? RT_TOP_NODES : 1];
  constexpr bool TRI_LDS = RT_TRI_LDS > 0 && !EXACT && !is_trace_job(JOB);
  __shared__ float4 s_tri[TRI_LDS ? WG_WAVES : 1][TRI_LDS ? 3 * RT_TRI_LDS : 1];
  const uint32_t n_top = USE_TOP ? min(sc.n_top, (uint32_t)RT_TOP_NODES) : 0u;
  if (USE_TOP && n_top) {
    for (uint32_t i = threadIdx.x; i < 4u * n_top; i += (uint32_t)(64 * WG_WAVES)) s_top[i / n_top][i % n_top] = sc.top_img[(size_t)(i / n_top) * RT_TOP_NODES + (i % n_top)];
    __syncthreads();
  }
  const uint32_t root_desc = (USE_TOP && n_top) ? sc.tlas_root_top : sc.tlas_root;
  const uint32_t* const blas_roots = (USE_TOP && n_top) ? sc.blas_root_top : sc.blas_root;
  // single-instance scenes: the BLAS root every ray starts at, fetched once per wavefront (a scalar) instead of once per ray -- a dependent
  // load less on the way from a job to its first node step
  const uint32_t root_blas_desc = is_inst_desc(root_desc) ? blas_roots[root_desc & PAYLOAD_MASK] : DESC_DONE;

  // ---- per-lane ray state in registers ----
  float arx = 0, ary = 0, arz = 0, aix = 0, aiy = 0, aiz = 0;   // active ray: origin, 1/direction
  float hitd = 0, path_m = 0, tos_m = 0;
  uint32_t cur = DESC_IDLE, tos_d = DESC_DONE, job = 0, flags = 0;
  // JOB_RENDER_GI: colour and albedo of the pixel's primary hit and the pixel's bounce ray (world space), kept while that ray is traced
  float g_col[3] = {0.f, 0.f, 0.f}, g_alb[3] = {0.f, 0.f, 0.f}, g_ray[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int sp = 0;                     // entries below the register top (LDS, then scratch)
  // entries past the LDS levels (scratch): the whole stack holds STACK_CAP entries below the register top
  constexpr int STACK_CAP = SHALLOW ? 3 * RT_SHALLOW_LEVELS : LSTK + RT_STACK_ENTRIES;
  static_assert(STACK_CAP > LSTK, "stack");
  uint32_t ovf_d[STACK_CAP - LSTK];
  float ovf_m[STACK_CAP - LSTK];
  // (IDENT implies a timed plain / shadow frame job that is not EXACT and not ALPHA: the static_assert above)
  constexpr bool BOX_NO_SELECT = RT_BOX_NO_SELECT && RT_OCC_OK_MASKS && IDENT && job_base(JOB) == JOB_RENDER_SHADOW;   // (RT_BOX_NO_SELECT above)
  // timed shadow frame jobs, identity-root kernels: the occlusion-only form of the traversal loop beside the general one (RT_OCC_LOOP above)
  // IDENT only: in the general kernels the second loop (with its own instance step) costs the register allocation 17 - 26 more spilled
  // VGPRs, some of them reloaded inside both loops (profiles/r13_a_isa_sections.txt; DESIGN.md s5, rejected)
  constexpr bool OCC_LOOP = RT_OCC_LOOP && IDENT && RT_BATCH_PUSH && RT_UNORDERED_OCCLUSION && RT_OCC_OK_MASKS && job_base(JOB) == JOB_RENDER_SHADOW &&
                            DEAD_MAX >= 64u && FINISH_MIN > 64u && STACK_CAP > 2 * LSTK;
  constexpr bool HINTS = RT_SHADOW_HINTS && OCC_LOOP && (JOB & JOB_NOHINTS) == 0;   // (RT_SHADOW_HINTS above; the host launches the JOB_NOHINTS form when A.hints is null)
  constexpr bool TILE_PHASES = RT_TILE_PHASES && OCC_LOOP;        // (RT_TILE_PHASES above: whole-tile phases, the kernels with the occlusion-only loop only)
  constexpr bool PHASE_COUNT = RT_PHASE_COUNT != 0 && OCC_LOOP;   // (counting variant, RT_PHASE_COUNT above)
  uint32_t ph_cnt[6] = {0u, 0u, 0u, 0u, 0u, 0u};                  // (wave-uniform; g_phase_counts' layout)
  // wave-uniform job-queue state
  bool queue_empty = false;
  // Home shard = the PHYSICAL XCD the wavefront runs on (HW_REG_XCC_ID, 0..7), so that band s of the frame is traced by the same XCD in every
  // launch and finds its part of the BVH in that XCD's L2 from the frame before.  Rounds 1-3 took blockIdx % 8: blocks b and b + 8 do share an
  // XCD, but WHICH one block 0 lands on changes from launch to launch (per-wavefront logs: the group of XCDs a band's wavefronts run on moves
  // by four between consecutive launches, profiles/r04_l_xcd.txt), so an XCD met another band's working set at every launch.  Speed only:
  // any wavefront may take any shard's jobs.  (shard_rot: diagnostic rotation of the XCD -> band map.)
  const uint32_t xcc_id = RT_XCC_HOME ? (uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) : blockIdx.x;   // XCC_ID[3:0]
  const uint32_t shard = (xcc_id + A.shard_rot) % QUEUE_SHARDS;
  uint32_t tries = 0, loc_next = 0, loc_end = 0;
  uint32_t loc_off = 0;           // job id = queue position + loc_off (tile order indirection of render jobs)
  // tile whose cost is being taken for A.tile_cost.  The cost is WORK, not time: loop iterations of the wavefront while it held the tile (a leaf-body
  // run counts three).  Round 3 took the 100 MHz clocks the tile occupied its wavefront -- but a tile's duration says when it ran, not what it
  // is: tiles started as the queue runs dry take 2.5x as long as the same tiles earlier in a launch, the duration of a tile in one set of frames
  // correlates at -0.1 .. -0.2 with its duration in the set before, and an order learned from it puts last set's late (= "slow") tiles first and
  // the truly expensive ones last, every other set (profiles/r04_f_tile_tail.txt).  Iterations are a property of the tile alone.
  uint32_t lpt_tile = 0xFFFFFFFFu, lpt_work = 0; unsigned long long lpt_t0 = 0;
  Fetches fx;
  unsigned nrays = 0, nhit = 0;
  unsigned long long t_first = 0;
  unsigned long long wl_tn = 0, wl_tl = 0, wl_t0 = 0;   // wave_log: shader clocks inside the node body / the leaf body
  unsigned wl_no23 = 0, wl_no3 = 0, wl_iter = 0, wl_node_x = 0, wl_node_l = 0, wl_leaf_x = 0, wl_leaf_l = 0;   // wave_log: lane occupancy of the two bodies
  unsigned wl_cc[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // wave_log: node-body runs by the largest valid-children count of their lanes (0, 1, 2, >= 3): ordered arm, occlusion arm
  unsigned long long wl_tstart = 0, wl_tf = 0, wl_tfin = 0, wl_tmark = 0;   // wave_log: shader clocks in the fetch / finish sections
  unsigned long long wl_tq = 0;   // wave_log: 100 MHz clock at which this wavefront found every queue shard empty
  if (STATS && A.wave_log) { t_first = wall_clock64(); wl_tstart = __builtin_readcyclecounter(); }

  auto pixel_of = [&](uint32_t r, uint32_t& x, uint32_t& y) {
    // (the job id goes through an empty asm statement: the compiler then derives the pixel again wherever it is asked for -- a dozen
    // instructions -- instead of keeping x, y and the table addresses of every lane alive, in scratch, from the start of a ray to its end)
    asm volatile("" : "+v"(r));
    uint32_t tile = r >> 6;
    const uint32_t l = r & 63u;
    if (A.pbatch) tile -= fast_div(tile, A.div_frame_tiles) * A.frame_tiles;   // (a batch of frames: same window, frame_tiles tiles apart)
    const uint32_t ty = fast_div(tile, A.div_tiles_x);
    x = (tile - ty * A.tiles_x) * 8u + (l & 7u);
    y = A.y0 + ty * A.row_step + (l >> 3);
  };
  // where the lane's hit record goes (same reason for the empty asm statement as in pixel_of: the address is formed where it is used -- one
  // multiply-add -- instead of living in two registers, or two scratch slots, for the length of the ray)
  auto hit_slot = [&]() -> HitRec* {
    uint32_t j = job;
    asm volatile("" : "+v"(j));
    return A.hits + j;
  };
  // the lane's hint word (RT_SHADOW_HINTS): the same index, formed where it is used for the same reason
  auto hint_slot = [&]() -> uint32_t* {
    uint32_t j = job;
    asm volatile("" : "+v"(j));
    return A.hints + j;
  };
  // the primary ray of pixel (x, y) of the lane's job
  auto pixel_ray = [&](uint32_t x, uint32_t y, float& ox, float& oy, float& oz, float& dx, float& dy, float& dz) {
    if constexpr (is_cam_job(JOB)) {
      const uint32_t f = A.pbatch ? fast_div(job >> 6, A.div_frame_tiles) : 0u;
      camera_ray(s_cam + f * CAM_HDR, A.vtab + (size_t)f * (A.W + A.H), A.W, x, y, ox, oy, oz, dx, dy, dz);
    } else generate_ray(A.utab[x], A.vtab[y], ox, oy, oz, dx, dy, dz);
  };
  // the lane's world-space ray, re-derived from its job (deterministic: same bits every time)
  auto world_ray = [&](float& ox, float& oy, float& oz, float& dx, float& dy, float& dz, float& tmax_) {
    tmax_ = RT_LARGE_FLOAT;
    if (is_trace_job(JOB)) {
      const float* rp = A.rays + (size_t)job * 6;
      if (RT_TRACE_NT) {   // (a ray is read once, by one lane: streamed past the caches that hold the tree)
        ox = __builtin_nontemporal_load(rp); oy = __builtin_nontemporal_load(rp + 1); oz = __builtin_nontemporal_load(rp + 2);
        dx = __builtin_nontemporal_load(rp + 3); dy = __builtin_nontemporal_load(rp + 4); dz = __builtin_nontemporal_load(rp + 5);
      } else { ox = rp[0]; oy = rp[1]; oz = rp[2]; dx = rp[3]; dy = rp[4]; dz = rp[5]; }
      if (A.tmax) tmax_ = A.tmax[job];
    } else {
      uint32_t x, y;
      pixel_of(job, x, y);
      pixel_ray(x, y, ox, oy, oz, dx, dy, dz);
      if (job_base(JOB) == JOB_RENDER_GI && (flags & F_SHADOW)) {   // bounce phase: the ray drawn when the primary ray finished
        ox = g_ray[0]; oy = g_ray[1]; oz = g_ray[2]; dx = g_ray[3]; dy = g_ray[4]; dz = g_ray[5];
      }
      if (job_base(JOB) == JOB_RENDER_SHADOW && (flags & F_SHADOW)) {
        const float pd = __uint_as_float(CTX(5));   // distance of this pixel's primary hit
        float sox, soy, soz, sdx, sdy, sdz, sdist;
        float lpx = p.lpos[0], lpy = p.lpos[1], lpz = p.lpos[2];
        if (A.pbatch) { const ShadeParams* q = A.pbatch + fast_div(job >> 6, A.div_frame_tiles); lpx = q->lpos[0]; lpy = q->lpos[1]; lpz = q->lpos[2]; }
        shadow_ray(lpx, lpy, lpz, ox, oy, oz, dx, dy, dz, pd, sox, soy, soz, sdx, sdy, sdz, sdist);
        ox = sox; oy = soy; oz = soz; dx = sdx; dy = sdy; dz = sdz;
        tmax_ = sdist;
      }
    }
  };
  // main launch only: hand this lane's ray (in its current phase) over to the EXACT launch
  auto defer = [&](bool counted) {
    const uint32_t slot = atomicAdd(A.defer_count, 1u);
    // (JOB_RENDER_GI: a bounce ray outside the fast domain sends the whole PIXEL to the EXACT launch, which traces its primary ray again
    // -- same hit by construction -- and goes on from there; the primary ray this launch counted is taken back)
    if (job_base(JOB) == JOB_RENDER_GI && (flags & F_SHADOW)) nrays--;
    if (slot < A.defer_cap) A.defer_list[slot] = job | ((flags & F_SHADOW) && job_base(JOB) != JOB_RENDER_GI ? 0x80000000u : 0u);
    if (job_base(JOB) == JOB_RENDER_SHADOW && (flags & F_SHADOW)) {
      // the EXACT launch resumes this pixel's occlusion ray from the primary hit record in memory
      HitRec h;
      h.bx = __uint_as_float(CTX(3)); h.by = __uint_as_float(CTX(4)); h.bz = 1 - h.bx - h.by;
      h.dist = __uint_as_float(CTX(5)); h.blasIdx = CTX(6); h.triIdx = CTX(7);
      *hit_slot() = h;
    }
    if (counted) nrays--;   // the EXACT launch counts the ray when it starts it again
    cur = DESC_IDLE;
  };
  // TLAS leaf (rt_traversal.cpp:109-121): fetch the instance record, move the ray to object space
  auto enter_instance = [&](uint32_t blasIdx, float ox, float oy, float oz, float dx, float dy, float dz) {
    const uint32_t* bp = sc.blas + (size_t)blasIdx * (RT_BLAS_STRIDE / 4);
    uint32_t bw[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) bw[i] = bp[i];
    if (STATS) { fx.node++; fx.inst++; }
    const float m00 = __uint_as_float(bw[1]), m01 = __uint_as_float(bw[2]), m02 = __uint_as_float(bw[3]), m03 = __uint_as_float(bw[4]);
    const float m10 = __uint_as_float(bw[5]), m11 = __uint_as_float(bw[6]), m12 = __uint_as_float(bw[7]), m13 = __uint_as_float(bw[8]);
    const float m20 = __uint_as_float(bw[9]), m21 = __uint_as_float(bw[10]), m22 = __uint_as_float(bw[11]), m23 = __uint_as_float(bw[12]);
    arx = m00 * ox + m01 * oy + m02 * oz + m03;   // :231-261
    ary = m10 * ox + m11 * oy + m12 * oz + m13;
    arz = m20 * ox + m21 * oy + m22 * oz + m23;
    const float cdx = m00 * dx + m01 * dy + m02 * dz;
    const float cdy = m10 * dx + m11 * dy + m12 * dz;
    const float cdz = m20 * dx + m21 * dy + m22 * dz;
    aix = 1.0f / cdx; aiy = 1.0f / cdy; aiz = 1.0f / cdz;
    const bool s2 = ray_in_fast_domain(arx, ary, arz, aix, aiy, aiz);
    if (!EXACT && !s2) { defer(true); return; }   // object-space ray can produce NaN slabs: restart it in the EXACT launch
    flags &= ~F_WORLD;
    CTX(0) = __float_as_uint(cdx); CTX(1) = __float_as_uint(cdy); CTX(2) = __float_as_uint(cdz);
    CTX(8) = blasIdx;
    cur = blas_roots[blasIdx];   // BLAS root: same level, path_m unchanged
  };
  // (re)start the lane's traversal at the TLAS root (rt_traversal.cpp:39-40) with world ray (o, d)
  auto start_ray = [&](float ox, float oy, float oz, float dx, float dy, float dz, float tmax_, bool any_) {
    arx = ox; ary = oy; arz = oz;
    aix = 1.0f / dx; aiy = 1.0f / dy; aiz = 1.0f / dz;
    // the fast slab forms are exact only if no slab product can be NaN or overflow (see ray_in_fast_domain)
    const bool safe = ray_in_fast_domain(ox, oy, oz, aix, aiy, aiz);
    flags = (flags & (F_SHADOW | F_RESUMED)) | F_WORLD | (any_ ? F_ANYHIT : 0u);
    if (!EXACT && !safe) {
      // camera rays with a zero direction component are known before the launch (u == 0 or v == 0): the
      // host lists them and a concurrent EXACT launch traces them; everything else is deferred -- the primary
      // rays of camera frames (JOB_CAM) too: no host list predicts them
      if (!is_trace_job(JOB) && !is_cam_job(JOB) && !(flags & F_SHADOW)) cur = DESC_IDLE; else defer(false);
      return;
    }
    hitd = tmax_ > RT_LARGE_FLOAT ? RT_LARGE_FLOAT : tmax_;   // (a bound above 1e30 is 1e30: a missed box reports 1e30, rt_traversal.cpp:338, and must stay filtered by `d < hit.dist`)
    path_m = -__builtin_inff(); sp = 0; tos_d = DESC_DONE;
    cur = root_desc;
    nrays++;
    // single-instance scenes (the reference's default): the TLAS root is the instance leaf, enter it
    // right away with the ray at hand instead of re-deriving it in the instance step
    if (is_inst_desc(root_desc)) {
      // ... and when that instance's inverse transform is the identity (checked by the accel build: ones on the diagonal, zeros of either sign
      // elsewhere), the object-space ray IS the world ray, bit for bit, so the record fetch, the 18 multiply-adds, three divisions and the
      // second domain check of the instance step are skipped.  Why the bits agree: 1*x is x; adding products that are +-0 leaves a non-zero x
      // alone and turns a zero sum into +0 -- so the only component the arithmetic would change is an origin component that is -0 (it becomes
      // +0); directions have no zero component inside the fast domain.  Rays with a -0 origin component take the general step.
      const bool no_neg_zero = __float_as_uint(ox) != 0x80000000u && __float_as_uint(oy) != 0x80000000u && __float_as_uint(oz) != 0x80000000u;
      if (sc.ident_root && safe && no_neg_zero) {   // (an EXACT launch's rays outside the fast domain -- zero, infinite or NaN components -- take the general step)
        if (STATS) { fx.node++; fx.inst++; }
        flags &= ~F_WORLD;
        CTX(0) = __float_as_uint(dx); CTX(1) = __float_as_uint(dy); CTX(2) = __float_as_uint(dz);
        CTX(8) = root_desc & PAYLOAD_MASK;
        cur = root_blas_desc;
      } else enter_instance(root_desc & PAYLOAD_MASK, ox, oy, oz, dx, dy, dz);
    }
  };
  // (the scratch part of the stack through volatile pointers: the compiler must not speculate its loads into the common path)
  volatile uint32_t* const vovf_d = ovf_d;
  volatile float* const vovf_m = ovf_m;
  auto push = [&](uint32_t d, float m) {
    if (tos_d != DESC_DONE) {
      if (sp < LSTK) lstk[sp * 64] = make_uint2(tos_d, __float_as_uint(tos_m));
      else { ovf_d[sp - LSTK] = tos_d; ovf_m[sp - LSTK] = tos_m; }
      ++sp;
    }
    tos_d = d; tos_m = m;
  };
  // The pending children of one node step, pushed at once: (d0, m0) if p0, then (d1, m1) if p1, then (d2, m2) if p2 -- the stack ends up
  // exactly as after those push() calls.  What goes to memory is the old register top (if there is one) followed by the pushed entries
  // but the last, at consecutive slots from sp on; the last one becomes the register top.  The slots are counted once, sp and the top are
  // set once, and a lane decides once where its slots lie: all in LDS, all in scratch, or (the step that crosses the boundary) entry by
  // entry as push() does.  The three arms are per-lane branches: the compiler keeps them apart in this listing (an arm no lane takes is
  // jumped over with EXEC empty), but nothing in the source forces that -- tools/isa_sections.py shows what a compiler made of it.
  //
  // The occlusion-only form of the traversal loop (`occ`, RT_OCC_LOOP; OCC_LOOP above says which kernels hold it) keeps the descriptor alone:
  // an occlusion ray's hitd is the constant distance to the light until the ray stops, a child is only pushed when its box is entered before
  // hitd, so the path maximum of an entry always passes pop_next's `m < hitd` and is never needed.  Its entries are 4 bytes: the LDS rows
  // of s_stk hold 2 * LSTK of them per lane (rows of 64 dwords, lstk4), the rest goes to ovf_d (STACK_CAP - 2 * LSTK < STACK_CAP - LSTK
  // entries); STACK_CAP and the heights are the same in both forms.  The two layouts never meet: start_ray empties the stack, and a ray's
  // whole traversal lies inside ONE invocation of ONE form of the loop -- with whole-tile batches (DEAD_MAX 64, FINISH_MIN off: required by
  // OCC_LOOP) the loop is only left when no lane holds work, and lanes receive rays outside it.
  auto push_pending = [&](auto occ, bool p0, uint32_t d0, float m0, bool p1, uint32_t d1, float m1, bool p2, uint32_t d2, float m2) {
    constexpr bool OCC = decltype(occ)::value;
    if (!RT_BATCH_PUSH) {
      if (p0) push(d0, m0);
      if (p1) push(d1, m1);
      if (p2) push(d2, m2);
      return;
    }
    if (!(p0 || p1 || p2)) return;
    const bool w_top = tos_d != DESC_DONE;          // the old top goes to slot sp
    const bool w0 = p0 && (p1 || p2), w1 = p1 && p2;   // (d2 is never stored: if it is pushed, it is the new top)
    const int q0 = sp + (w_top ? 1 : 0), q1 = q0 + (w0 ? 1 : 0), end = q1 + (w1 ? 1 : 0);   // slots of d0, of d1; the new sp
    if constexpr (OCC) {
      // 4-byte entries: 2 * LSTK rows of 64 dwords in LDS, then ovf_d
      constexpr int LROWS = 2 * LSTK;
      uint32_t* const lstk4 = lstk4_here();
      if (end <= LROWS) {
        if (w_top) lstk4[sp * 64] = tos_d;
        if (w0) lstk4[q0 * 64] = d0;
        if (w1) lstk4[q1 * 64] = d1;
      } else if (sp >= LROWS) {
        if (w_top) ovf_d[sp - LROWS] = tos_d;
        if (w0) ovf_d[q0 - LROWS] = d0;
        if (w1) ovf_d[q1 - LROWS] = d1;
      } else {
        auto put = [&](int q, uint32_t d) {
          if (q < LROWS) lstk4[q * 64] = d;
          else ovf_d[q - LROWS] = d;
        };
        if (w_top) put(sp, tos_d);
        if (w0) put(q0, d0);
        if (w1) put(q1, d1);
      }
    } else
    if (end <= LSTK) {
      if (w_top) lstk[sp * 64] = make_uint2(tos_d, __float_as_uint(tos_m));
      if (w0) lstk[q0 * 64] = make_uint2(d0, __float_as_uint(m0));
      if (w1) lstk[q1 * 64] = make_uint2(d1, __float_as_uint(m1));
    } else if (sp >= LSTK) {
      if (w_top) { ovf_d[sp - LSTK] = tos_d; ovf_m[sp - LSTK] = tos_m; }
      if (w0) { ovf_d[q0 - LSTK] = d0; ovf_m[q0 - LSTK] = m0; }
      if (w1) { ovf_d[q1 - LSTK] = d1; ovf_m[q1 - LSTK] = m1; }
    } else {
      auto put = [&](int q, uint32_t d, float m) {
        if (q < LSTK) lstk[q * 64] = make_uint2(d, __float_as_uint(m));
        else { ovf_d[q - LSTK] = d; ovf_m[q - LSTK] = m; }
      };
      if (w_top) put(sp, tos_d, tos_m);
      if (w0) put(q0, d0, m0);
      if (w1) put(q1, d1, m1);
    }
    sp = end;
    tos_d = p2 ? d2 : (p1 ? d1 : d0);
    if constexpr (!OCC) tos_m = p2 ? m2 : (p1 ? m1 : m0);
  };
  // entry `i` of the stack's memory part (LDS, then scratch)
  auto stack_load = [&](auto occ, int i, uint32_t& d, float& m) {
    // (LDS-typed pointer: through two plain pointers the compiler merges the arms into flat loads of a selected address)
    if constexpr (decltype(occ)::value) {
      typedef __attribute__((address_space(3))) const uint32_t lds_u32_t;
      if (i < 2 * LSTK) d = ((lds_u32_t*)lstk4_here())[i * 64];
      else d = ovf_d[i - 2 * LSTK];
    } else {
      typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
      typedef __attribute__((address_space(3))) const u32x2_t lds_u32x2_t;
      if (i < LSTK) { const u32x2_t e = ((lds_u32x2_t*)lstk)[i * 64]; d = e.x; m = __uint_as_float(e.y); }
      else { d = ovf_d[i - LSTK]; m = ovf_m[i - LSTK]; }
    }
  };
  // next pending work item of this lane (m < hit.dist: the reference's re-filtering),
  // or DESC_DONE when its stack is exhausted.  The refill of the register top from LDS is not waited for.
  auto pop_next = [&](auto occ) {
    if constexpr (decltype(occ)::value) {
      // (every entry passes the re-filter, see above: the top is taken as it is)
      cur = tos_d;
      tos_d = DESC_DONE;
      if constexpr (HINTS) flags &= ~F_GUIDED;   // (the hint's path ends where the lane first takes a pending sibling)
      if (cur != DESC_DONE && sp > 0) { --sp; float m; stack_load(occ, sp, tos_d, m); }
      return;
    }
    if (RT_BATCH_PUSH) {
      // the candidates are the register top, then the memory part from sp - 1 down.  Entries that the shrunken hit distance filters (rare)
      // are skipped first, reading memory directly; the register top is then refilled ONCE, behind the entry that was taken.
      uint32_t d = tos_d; float m = tos_m;
      while (d != DESC_DONE && !(m < hitd)) {
        if (sp > 0) { --sp; stack_load(occ, sp, d, m); } else d = DESC_DONE;
      }
      cur = d;
      tos_d = DESC_DONE;
      if (d != DESC_DONE) {
        path_m = m;
        if (sp > 0) { --sp; stack_load(occ, sp, tos_d, tos_m); }
      }
      return;
    }
    cur = DESC_DONE;
    while (tos_d != DESC_DONE) {
      const uint32_t d = tos_d;
      const float m = tos_m;
      if (sp > 0) {
        --sp;
        if (sp < LSTK) { const uint2 e = lstk[sp * 64]; tos_d = e.x; tos_m = __uint_as_float(e.y); }
        else { tos_d = ovf_d[sp - LSTK]; tos_m = ovf_m[sp - LSTK]; }
      } else {
        tos_d = DESC_DONE;
      }
      if (m < hitd) { cur = d; path_m = m; break; }
    }
  };

  for (;;) {
    RT_MARK("fetch");
    if (STATS && A.wave_log) wl_tmark = __builtin_readcyclecounter();
    // ================= fetch: hand new jobs to idle lanes =================
    // Jobs are reserved per wavefront in chunks from one of the queue shards (one global atomic per
    // RT_CHUNK jobs); lanes then draw from the wavefront's private range.
    {
      const unsigned long long idle = __ballot(cur == DESC_IDLE);
      // (TILE_PHASES: jobs only to a wavefront none of whose lanes holds work -- the `idle == ~0ull` arm -- or, RT_TILE_REFILL_MIN <= 64, to
      // one with at least that many idle lanes)
      bool refill = is_trace_job(JOB) || FINISH_MIN > 64u || idle == ~0ull || RT_DEAD_MAX < 64;
      if constexpr (TILE_PHASES) refill = tile_refill(idle, (uint32_t)RT_TILE_REFILL_MIN);   // (rt_tile_refill.h)
      if (!queue_empty && idle != 0ull && refill) {
        const uint32_t wl_tries0 = tries; const unsigned long long wl_tpoll0 = (STATS && A.wave_log) ? __builtin_readcyclecounter() : 0ull;
        if (loc_next == loc_end) {   // wave-uniform: reserve the next chunk, stealing from other shards when the home shard is dry
          // shards a wavefront of this WORKGROUP has found handed out (LDS: no memory traffic): not polled again by its other three.  Every
          // wavefront used to poll every shard once before it ends -- 8 failing read-modify-writes each on the eight hottest lines of the
          // system, more than the launch's successful ones, all within its last third: serial frames +6 %, ray buffers +4 %
          // (profiles/r04_h_dry_mask_ab.txt).  Anything that ADDS traffic next to these counters loses, whatever it saves: the same mask
          // published through memory (a word read with agent scope and OR-ed into) -30 %, a look at the counter before the read-modify-write
          // -20 % (agent-scope load) / -47 % (non-temporal load, which turns every queue atomic into a round trip to memory), several tiles per
          // reservation -7 % (neighbouring tiles traced one after the other by ONE wavefront share less than the same tiles traced at the same
          // time by four: the queue's order is what keeps a CU's L1 warm) -- profiles/r04_h_*.txt.
          uint32_t dry = RT_QUEUE_DRY_MASK ? *(volatile uint32_t*)&s_dry : 0u;
          while (tries < QUEUE_SHARDS) {
            // the shards in the order this wavefront visits them: its home shard (its XCD's band), then RT_STEAL_SPREAD ? the others in
            // bit-reversed distance (+4, +2, +6, +1, +5, +3, +7: the helpers of a drained band spread over the remaining ones) : +1, +2, ...
            const uint32_t step = RT_STEAL_SPREAD ? (((tries & 1u) << 2) | (tries & 2u) | ((tries >> 2) & 1u)) : tries;
            const uint32_t sid = (shard + step) % QUEUE_SHARDS;
            if (RT_QUEUE_DRY_MASK && ((dry >> sid) & 1u)) { ++tries; continue; }
            const uint32_t s_lo = sid * per_shard;
            // a shard past the end of the job range costs no atomic (an EXACT launch with nothing deferred used to pay eight per
            // wavefront to find eight empty shards).  Written as an explicit range test: folded into `s_n == 0` on a select, this
            // compiler dropped the `s_lo < n_jobs` half of the condition and the wavefronts ran past the end of the job list.
            // The test is an asm statement the optimiser cannot look into, and its marker comment is what the build check greps for
            // in every instantiation's listing (tests/test_build_guards.py: one RTGUARD before the kernel's first queue atomic).
            uint32_t in_range;
            asm volatile("s_cmp_lt_u32 %1, %2\n\ts_cselect_b32 %0, 1, 0 ; RTGUARD shard_range" : "=s"(in_range)
                         : "s"(__builtin_amdgcn_readfirstlane(s_lo)), "s"(__builtin_amdgcn_readfirstlane(n_jobs)) : "scc");   // (both wave-uniform)
            if (!in_range) { ++tries; continue; }
            const uint32_t s_n = min(per_shard, n_jobs - s_lo);
            uint32_t base = 0;
            constexpr uint32_t CHUNK = (is_trace_job(JOB) && !EXACT) ? (uint32_t)RT_TRACE_CHUNK : (uint32_t)RT_CHUNK;
            if (lane == 0) base = atomicAdd(A.queue + sid * QUEUE_STRIDE, CHUNK);
            base = __shfl(base, 0);
            if (base < s_n) {
              loc_next = s_lo + base; loc_end = s_lo + min(base + CHUNK, s_n);
              break;
            }
            // handed out: tell the workgroup's other wavefronts
            if (RT_QUEUE_DRY_MASK) {
              if (lane == 0) atomicOr(&s_dry, 1u << sid);
              dry |= 1u << sid;
            }
            ++tries;
          }
          if (tries >= QUEUE_SHARDS) { queue_empty = true; if (STATS && A.wave_log && !wl_tq) wl_tq = wall_clock64(); }
          if (STATS && A.wave_log && !USE_TOP && tries != wl_tries0 && lane == 0) wl_no23 += (unsigned)(__builtin_readcyclecounter() - wl_tpoll0);   // (diagnostic: shader clocks of the reservations that met a dry shard)
        }
        uint32_t avail = loc_end - loc_next;
        if (!is_trace_job(JOB) && !EXACT) {
          avail = min(avail, 64u - (loc_next & 63u));     // lanes draw from ONE tile at a time (a reservation may span several)
          if (avail != 0u && (A.tile_order || A.tile_cost)) {
            // the tile these jobs belong to: queue position -> tile through the order of the launch; its cost is taken from here to the next tile's start
            const uint32_t pos = loc_next >> 6;
            const uint32_t tile = A.tile_order ? A.tile_order[pos] : pos;
            loc_off = __builtin_amdgcn_readfirstlane((tile << 6) - (loc_next & ~63u));   // (wave-uniform: a scalar register)
            if (A.tile_cost && tile != lpt_tile) {
              if (lane == 0 && lpt_tile != 0xFFFFFFFFu) A.tile_cost[lpt_tile] = lpt_work;
              if (STATS && A.wave_log) {   // (diagnostic: when the tile was started and how long the one before it took, in 100 MHz clocks, behind the costs)
                const unsigned long long now = wall_clock64();
                if (lane == 0) {
                  if (lpt_tile != 0xFFFFFFFFu) A.tile_cost[2u * (A.total >> 6) + lpt_tile] = (uint32_t)min(now - lpt_t0, 0xFFFFFFFFull);
                  A.tile_cost[(A.total >> 6) + tile] = (uint32_t)now;
                  A.tile_cost[3u * (A.total >> 6) + tile] = tries;   // 0 = taken from the wavefront's home shard, else stolen from the tries-th shard after it
                }
                lpt_t0 = now;
              }
              lpt_tile = tile; lpt_work = 0;
            }
          }
        }
        if (avail != 0u && cur == DESC_IDLE) {
          const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
          if (rank < avail) {
            job = loc_next + rank + loc_off;
            flags = 0;
            if (!EXACT && is_trace_job(JOB) && A.order) job = A.order[job];
            if (EXACT) {
              const uint32_t wd = A.defer_list[job];
              job = wd & 0x7fffffffu;
              if (wd >> 31) { flags = F_SHADOW | F_RESUMED; if (job_base(JOB) == JOB_RENDER_SHADOW) CTX(5) = __float_as_uint(hit_slot()->dist); }
            }
            float ox, oy, oz, dx, dy, dz, tm;
            if (is_trace_job(JOB)) {
              world_ray(ox, oy, oz, dx, dy, dz, tm);
              start_ray(ox, oy, oz, dx, dy, dz, tm, A.any_hit != 0);
            } else {
              uint32_t x, y;
              pixel_of(job, x, y);
              if (x < A.W && y < A.y1) {   // kernel.cpp:62,101
                world_ray(ox, oy, oz, dx, dy, dz, tm);
                start_ray(ox, oy, oz, dx, dy, dz, tm, (flags & F_SHADOW) != 0u);
              }
            }
          }
        }
        loc_next += min(avail, (uint32_t)__popcll(idle));
      }
      if (__ballot(cur != DESC_IDLE) == 0ull) {
        if (queue_empty && loc_next == loc_end) {
          if (!is_trace_job(JOB) && !EXACT && A.tile_cost && lane == 0 && lpt_tile != 0xFFFFFFFFu) {
            A.tile_cost[lpt_tile] = lpt_work;
            if (STATS && A.wave_log) A.tile_cost[2u * (A.total >> 6) + lpt_tile] = (uint32_t)min(wall_clock64() - lpt_t0, 0xFFFFFFFFull);
          }
          break;
        }
        if (STATS && A.wave_log) wl_tf += __builtin_readcyclecounter() - wl_tmark;
        continue;
      }
    }
    if (STATS && A.wave_log) wl_tf += __builtin_readcyclecounter() - wl_tmark;

    // ================= traverse: one step of whatever each lane holds, per iteration =================
    // The loop's text is rt_traverse_loop.inc, written once over the compile-time flag OCC.  A kernel that holds the occlusion-only form
    // (OCC_LOOP) compiles it twice, as the two instantiations of a generic lambda; `occ` = every lane that holds work holds an any-hit ray,
    // for as long as the loop runs -- lanes only receive rays in the fetch and finish sections, defer() only makes a lane idle.  Every
    // other kernel has the text in place, outside any lambda, with OCC false: those kernels' listings are the parent form's (wrapped in
    // the lambda and with the 8-byte push restated through shared helpers they computed the same and ran 2.3 % slower: DESIGN.md s5).
    if constexpr (OCC_LOOP) {
      auto traverse = [&](auto occ) {
        constexpr bool OCC = decltype(occ)::value;
#include "rt_traverse_loop.inc"
      };
      // -DRT_OCC_LOOP_CHECK=1 (variant libraries only): the invariant the two stack layouts rest on -- a lane that holds work in front of
      // the loop holds a ray fresh from start_ray, with an empty stack -- reported as STATUS_ITER_LIMIT, which every test reads as a failure
      if (RT_OCC_LOOP_CHECK && is_work_desc(cur) && (sp != 0 || tos_d != DESC_DONE)) atomicOr(A.status, STATUS_ITER_LIMIT);
      // (is_work_desc: a lane that is finished or idle keeps the flags of its last ray)
      // (TILE_PHASES without partial refills: a pass holds one kind of ray.  The checking variant reports one that holds both.)
      if (RT_OCC_LOOP_CHECK && TILE_PHASES && RT_TILE_REFILL_MIN > 64 && __any(is_work_desc(cur) && (flags & F_ANYHIT) != 0u) && __any(is_work_desc(cur) && (flags & F_ANYHIT) == 0u))
        atomicOr(A.status, STATUS_ITER_LIMIT);
      if constexpr (PHASE_COUNT) {
        if (__all(!is_work_desc(cur) || (flags & F_ANYHIT) != 0u)) ++ph_cnt[0];
        else if (__any(is_work_desc(cur) && (flags & F_ANYHIT) != 0u)) ++ph_cnt[2];
        else ++ph_cnt[1];
      }
      if (__all(!is_work_desc(cur) || (flags & F_ANYHIT) != 0u)) traverse(std::true_type());
      else {
        // (a mixed wavefront: the general loop needs path_m as start_ray left it -- every ray in front of the loop is fresh -- and knows no hints.
        // INVARIANT: while F_GUIDED or F_HINTW is set, path_m holds a bit pattern, not a path maximum; whatever reads path_m as a float must
        // run behind this restore or in a lane without those flags)
        if constexpr (HINTS) { if (flags & F_GUIDED) { path_m = -__builtin_inff(); flags &= ~F_GUIDED; } }
        traverse(std::false_type());
      }
    } else {
      constexpr bool OCC = false;
      const std::false_type occ;
#include "rt_traverse_loop.inc"
    }

    // ================= finish: rays whose traversal ended =================
    RT_MARK("finish");
    if (STATS && A.wave_log) wl_tmark = __builtin_readcyclecounter();
    if (cur == DESC_DONE) {
      const bool found = (flags & F_FOUND) != 0u;
      HitRec h; h.dist = RT_LARGE_FLOAT; h.bx = 0; h.by = 0; h.bz = 0; h.blasIdx = 0; h.triIdx = 0;
      if (is_trace_job(JOB)) {
        if (found) {
          h.dist = hitd; h.bx = __uint_as_float(CTX(3)); h.by = __uint_as_float(CTX(4)); h.bz = 1 - h.bx - h.by;   // rt_traversal.cpp:311-313
          h.blasIdx = CTX(6); h.triIdx = CTX(7);
        }
        if (RT_TRACE_NT) {
          uint32_t* hp = (uint32_t*)hit_slot();
          __builtin_nontemporal_store(__float_as_uint(h.dist), hp); __builtin_nontemporal_store(__float_as_uint(h.bx), hp + 1);
          __builtin_nontemporal_store(__float_as_uint(h.by), hp + 2); __builtin_nontemporal_store(__float_as_uint(h.bz), hp + 3);
          __builtin_nontemporal_store(h.blasIdx, hp + 4); __builtin_nontemporal_store(h.triIdx, hp + 5);
        } else *hit_slot() = h;
        cur = DESC_IDLE;
      } else if (job_base(JOB) == JOB_RENDER_GI) {
        // one diffuse bounce, in the lane (see JOB_RENDER_GI above).  Every step is the code of the pass it replaces:
        // rt_ao_prepare_kernel (colour / albedo / hit point / normal of the primary hit), rt_ao_rays_kernel (the bounce ray) and, for the rest,
        // what the multi-pass form did after its trace launch: shade the bounce hit, colour += albedo * that, pack (orc_render_gi).
        uint32_t x, y;
        pixel_of(job, x, y);
        const size_t e = (size_t)x + (size_t)y * A.W;
        bool write = false;
        float cr = 0.f, cg = 0.f, cb = 0.f;
        if (found) {
          h.dist = hitd; h.bx = __uint_as_float(CTX(3)); h.by = __uint_as_float(CTX(4)); h.bz = 1 - h.bx - h.by;
          h.blasIdx = CTX(6); h.triIdx = CTX(7);
        }
        if (!(flags & F_SHADOW)) {
          float ox, oy, oz, dx, dy, dz;
          pixel_ray(x, y, ox, oy, oz, dx, dy, dz);
          if (!found) {
            cr = p.bg[0]; cg = p.bg[1]; cb = p.bg[2];   // miss.cpp:9-14; no bounce
            write = true;
          } else {
            float r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz, a3[3];
            shade_terms<false>(sc, p, ox, oy, oz, dx, dy, dz, h, false, r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz, nullptr, a3);
            float thr = 1.0f;
            thr *= refl;
            g_col[0] = r + p.bg[0] * thr; g_col[1] = g + p.bg[1] * thr; g_col[2] = b + p.bg[2] * thr;
            g_alb[0] = a3[0]; g_alb[1] = a3[1]; g_alb[2] = a3[2];
            ao_sample_ray(x, y, A.W, 1u, 0u, A.gi_seed, Ix, Iy, Iz, Nx, Ny, Nz, dx, dy, dz, g_ray);
            flags = F_SHADOW;       // (second phase of the pixel)
            start_ray(g_ray[0], g_ray[1], g_ray[2], g_ray[3], g_ray[4], g_ray[5], RT_LARGE_FLOAT, false);
          }
        } else {
          float r, g, b;
          shade_eval<false>(sc, p, g_ray[0], g_ray[1], g_ray[2], g_ray[3], g_ray[4], g_ray[5], h, found, false, r, g, b);
          cr = g_col[0] + g_alb[0] * r; cg = g_col[1] + g_alb[1] * g; cb = g_col[2] + g_alb[2] * b;
          write = true;
        }
        if (write) {
          A.dst[e] = pack_rgb8(cr, cg, cb);
          if (A.colors) { A.colors[3 * e] = cr; A.colors[3 * e + 1] = cg; A.colors[3 * e + 2] = cb; }
          cur = DESC_IDLE;
        }
      } else if (!(flags & F_SHADOW)) {
        // deferred shading: finishing a ray costs one store, not a chain of dependent loads
        if (STATS && found) nhit++;
        if (job_base(JOB) == JOB_RENDER_SHADOW && found) {
          // continue this lane with the pixel's occlusion ray; the record is written when that ray has finished
          // (RT_SHADOW_HINTS: the hint's load is issued first, its round trip lies behind the ray arithmetic)
          uint32_t hint = 0xFFFFFFFFu;
          if constexpr (HINTS) { if (A.hints) hint = *hint_slot(); }
          uint32_t x, y;
          pixel_of(job, x, y);
          float ox, oy, oz, dx, dy, dz, sox, soy, soz, sdx, sdy, sdz, sdist;
          pixel_ray(x, y, ox, oy, oz, dx, dy, dz);
          float lpx = p.lpos[0], lpy = p.lpos[1], lpz = p.lpos[2];
          if (A.pbatch) { const ShadeParams* q = A.pbatch + fast_div(job >> 6, A.div_frame_tiles); lpx = q->lpos[0]; lpy = q->lpos[1]; lpz = q->lpos[2]; }
          shadow_ray(lpx, lpy, lpz, ox, oy, oz, dx, dy, dz, hitd, sox, soy, soz, sdx, sdy, sdz, sdist);
          CTX(5) = __float_as_uint(hitd);
          flags = F_SHADOW;
          start_ray(sox, soy, soz, sdx, sdy, sdz, sdist, true);
          if constexpr (HINTS) {
            // (a ray that start_ray handed to the EXACT launch left the lane idle: it keeps path_m and its flags as start_ray left them)
            if (hint < A.n_path_tris && is_work_desc(cur)) { path_m = __uint_as_float(A.tri_path[hint]); flags |= F_GUIDED; }
          }
        } else {
          if (found) {
            h.dist = hitd; h.bx = __uint_as_float(CTX(3)); h.by = __uint_as_float(CTX(4)); h.bz = 1 - h.bx - h.by;
            h.blasIdx = CTX(6); h.triIdx = CTX(7);
          }
          *hit_slot() = h;   // tile-major: job = tile * 64 + lane
          cur = DESC_IDLE;
        }
      } else if (EXACT && (flags & F_RESUMED)) {
        // occlusion ray handed over by the main launch: the record is in memory already, only the result is added
        if (found) hit_slot()->blasIdx |= 0x80000000u;
        cur = DESC_IDLE;
      } else {
        h.bx = __uint_as_float(CTX(3)); h.by = __uint_as_float(CTX(4)); h.bz = 1 - h.bx - h.by;
        h.dist = __uint_as_float(CTX(5)); h.blasIdx = CTX(6) | (found ? 0x80000000u : 0u); h.triIdx = CTX(7);   // found = occluded
        *hit_slot() = h;
        // (RT_SHADOW_HINTS: a ray blocked in the occlusion-only loop leaves its blocker for the pixel's next frame; unblocked rays write nothing)
        if constexpr (HINTS) { if (A.hints && (flags & F_HINTW) != 0u) *hint_slot() = __float_as_uint(path_m); }
        if constexpr (HINTS && RT_SHADOW_HINT_COUNT != 0) {   // (counting variant: blocked rays, and those that were still guided when they stopped)
          const unsigned long long all = __ballot(true), nb = __ballot(found), ng = __ballot(found && (flags & F_HINTW) != 0u && (flags & F_GUIDED) != 0u);
          if (lane == (uint32_t)__ffsll((long long)all) - 1u) { atomicAdd(&g_hint_counts[0], (unsigned long long)__popcll(nb)); atomicAdd(&g_hint_counts[1], (unsigned long long)__popcll(ng)); }
        }
        cur = DESC_IDLE;
      }
    }
    if (STATS && A.wave_log) wl_tfin += __builtin_readcyclecounter() - wl_tmark;
  }
#undef CTX

  if (STATS && A.wave_log && !EXACT) {
    unsigned s = nrays;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    for (int o = 32; o > 0; o >>= 1) wl_no23 += __shfl_down(wl_no23, o);   // node steps served from the LDS image, all lanes
    if (lane == 0) {
      unsigned long long* w = A.wave_log + 16ull * (blockIdx.x * (uint32_t)WG_WAVES + (threadIdx.x >> 6));
      w[13] = wl_tf; w[14] = wl_tfin; w[15] = wl_tq;
      w[0] = t_first; w[1] = wall_clock64(); w[2] = s; w[8] = wl_no23;
      w[9] = (unsigned long long)wl_no3 | ((unsigned long long)(uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) << 56);   // [63:56] physical XCD
      w[10] = wl_tn; w[11] = wl_tl; w[12] = __builtin_readcyclecounter() - wl_tstart;
      w[3] = wl_iter; w[4] = wl_node_x; w[5] = wl_node_l; w[6] = wl_leaf_x; w[7] = wl_leaf_l;
      // (the 16 words are taken and their layout is read by tools: the child-count classes are summed over the wavefronts, vxrt_debug_child_counts)
#pragma unroll
      for (int k = 0; k < 8; ++k) if (wl_cc[k]) atomicAdd(&g_child_counts[k], (unsigned long long)wl_cc[k]);
    }
  }
  if constexpr (PHASE_COUNT) {   // (the counts are wave-uniform: one lane adds them up)
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) if (ph_cnt[k]) atomicAdd(&g_phase_counts[k], (unsigned long long)ph_cnt[k]);
    }
  }
  if (!EXACT && A.end_log) {
    unsigned s = nrays;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (lane == 0) {
      unsigned long long* w = A.end_log + 2ull * (blockIdx.x * (uint32_t)WG_WAVES + (threadIdx.x >> 6));
      w[0] = wall_clock64();
      w[1] = (unsigned long long)s | ((unsigned long long)(uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) << 56);
    }
  }
  if (A.counters) {
    // one device atomic per WORKGROUP and counter (its wavefronts add up in LDS first): per wavefront, the 7,168 read-modify-writes a frame's
    // launch ends with -- all on one cache line -- cost the frame 40 us (8 %: profiles/r04_p_rays_counter.txt)
    __shared__ unsigned s_cnt[5];
    if (threadIdx.x < 5u) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    unsigned v[5] = {nrays, fx.node, fx.inst, fx.tri, nhit};
#pragma unroll
    for (int k = 0; k < (STATS ? 5 : 1); ++k) {
      unsigned s = v[k];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
      if (lane == 0 && s) atomicAdd(&s_cnt[k], s);
    }
    __syncthreads();
    if (threadIdx.x < (STATS ? 5u : 1u) && s_cnt[threadIdx.x]) atomicAdd(A.counters + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
  }
}

// Tile order for the next frame of a context: within each queue shard's band of tiles (a contiguous part of the
// frame, whose tiles share BVH nodes in the L2 of the XCD that works on it), most expensive first; cost = 100 MHz
// clocks the tile occupied its wavefront in the frame just traced.  A launch ends when its last tile ends, and a
// wavefront only gets about five tiles of a 1080p frame: starting the expensive ones first leaves the cheap ones for
// the tail.  One workgroup of 256 threads per shard, counting sort over 2048 monotone cost classes (5-bit exponent, 6-bit
// mantissa) with a parallel scan.  Runs as the FIRST workgroups of the shading launch (rt_shade_kernel): as a launch of its
// own between the traversal and the shading pass it sat on the critical path of a serial frame for 21 us, most of it one
// thread scanning the 2048 counters (profiles/r02_d_exact_timeline.txt).
// Measured and rejected: one global order dealt round robin to the shards (-4 %: loses the band -> XCD locality) and
// bands cut at equal cost instead of equal size (-7 %: the measured cost of a tile includes the contention on its SIMD).
// `base_order` (optional): the static order the queue positions have without learning (the band-major order of a batch of frames); the
// tiles of queue positions [lo, hi) are then base_order[lo..hi), and it is those that are sorted into order[lo..hi).
//
// Measured and rejected in round 4 (profiles/r04_k_pool_lpt_ab.txt): "cheap tiles last" -- each band's tiles split at one cost threshold, the
// cheap ones (a quarter of the frame's cost) handed out only when every band's expensive tiles are gone, so that what the wavefronts hold
// when the queue runs dry is a cheap tile: serial frames -9 %, a rank's sets of frames -2 .. -5 %.  The end of a launch is not long because of
// WHICH tiles are last: per-wavefront logs show every XCD doing the same number of loop iterations, and one half of the XCDs taking 20 % more
// clocks for each -- whatever band it traces (tools/wave_balance_batch.py, profiles/r04_l_xcd.txt).
__device__ __forceinline__ uint32_t lpt_cls(uint32_t c) {       // monotone cost class: 5-bit exponent, 6-bit mantissa
  if (c < 64u) return c;                                  // exponents 0..5 collapse onto the small values
  const uint32_t e = 31u - (uint32_t)__clz((int)c);       // 6..31
  return ((e - 5u) << 6) | ((c >> (e - 6u)) & 63u);       // 64 .. 1727
}
__device__ void lpt_order_block(uint32_t shard, const uint32_t* __restrict__ cost, uint32_t* __restrict__ order,
                                uint32_t n_tiles, uint32_t tiles_per_shard, uint32_t* hist /* LDS, 2048 + 8 words */,
                                const uint32_t* __restrict__ base_order = nullptr) {
  const uint32_t lo = shard * tiles_per_shard;
  const uint32_t hi = min(lo + tiles_per_shard, n_tiles);
  if (lo >= hi) return;   // (block-uniform)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t i = threadIdx.x; i < 2048u; i += 256u) hist[i] = 0u;
  __syncthreads();
  for (uint32_t t = lo + threadIdx.x; t < hi; t += 256u) atomicAdd(&hist[2047u - lpt_cls(cost[base_order ? base_order[t] : t])], 1u);   // descending
  __syncthreads();
  // exclusive scan of the 2048 counters: 8 consecutive counters per thread, wavefront scan, then the four wavefront totals
  uint32_t v[8], sum = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) { v[k] = hist[threadIdx.x * 8u + k]; sum += v[k]; }
  uint32_t inc = sum;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += y; }
  if (lane == 63u) hist[2048u + wave] = inc;
  __syncthreads();
  uint32_t base = inc - sum;
  for (uint32_t w = 0; w < wave; ++w) base += hist[2048u + w];
#pragma unroll
  for (int k = 0; k < 8; ++k) { hist[threadIdx.x * 8u + k] = base; base += v[k]; }
  __syncthreads();
  for (uint32_t t = lo + threadIdx.x; t < hi; t += 256u) {
    const uint32_t tile = base_order ? base_order[t] : t;
    order[lo + atomicAdd(&hist[2047u - lpt_cls(cost[tile])], 1u)] = tile;
  }
}

// Deferred shading pass: one thread per pixel of rows [y0,y1), x fastest, so hit records are read
// and pixels written fully coalesced.
// (CAM: camera frames -- utab / vtab are the camera block, see CAM_HDR)
template <bool STATS, bool CAM>
__device__ __forceinline__ void shade_pass(SceneDev sc, ShadeParams p, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t row_step,
                                           uint32_t n_rows, const float* __restrict__ utab, const float* __restrict__ vtab,
                                           const HitRec* __restrict__ hb, uint32_t* __restrict__ dst,
                                           HitRec* __restrict__ hits, float* __restrict__ colors,
                                           unsigned long long* counters, uint32_t* __restrict__ ctl_reset,
                                           uint32_t lpt_blocks, const uint32_t* __restrict__ lpt_cost, uint32_t* __restrict__ lpt_order,
                                           uint32_t lpt_tiles, uint32_t lpt_per_shard,
                                           uint32_t batch, const ShadeParams* __restrict__ pbatch, uint64_t dst_frame_stride,
                                           const uint32_t* __restrict__ lpt_base) {
  // the first lpt_blocks workgroups sort the frame's tiles by cost for the context's next frame (see lpt_order_block)
  __shared__ uint32_t s_hist[2048 + 8];
  if (blockIdx.x < lpt_blocks) { lpt_order_block(blockIdx.x, lpt_cost, lpt_order, lpt_tiles, lpt_per_shard, s_hist, lpt_base); return; }
  const uint32_t blk = blockIdx.x - lpt_blocks;
  // last kernel of a frame: every user of the frame's control block (queue counters, deferral count)
  // has finished, so zero it here for the context's next frame instead of paying fill launches per frame
  if (ctl_reset && blk == 0)
    for (uint32_t i = threadIdx.x; i < CTL_DWORDS; i += 256u) ctl_reset[i] = 0u;
  const uint64_t t = (uint64_t)blk * 256u + threadIdx.x;
  const uint64_t n = (uint64_t)W * n_rows * batch;   // local rows of the window (its tile rows x 8; rows past y1 are skipped), per frame of the batch
  unsigned ntex = 0, npix = 0;
  const uint32_t x = (uint32_t)(t % W), vr = (uint32_t)(t / W);   // vr: row of the batch's stacked windows
  const uint32_t frame = batch > 1 ? vr / n_rows : 0u, lr = vr - frame * n_rows, y = frame_row(lr, y0, row_step);
  if (batch > 1 && t < n) { p = pbatch[frame]; dst += (size_t)frame * dst_frame_stride; }
  if (t < n && y < y1) {
    const size_t idx = (size_t)x + (size_t)y * W;
    HitRec h = hb[hit_index(x, vr, (W + 7u) >> 3)];   // tile-major, 192 contiguous bytes per 8 pixels of a row
    const uint32_t occ_bit = h.blasIdx & 0x80000000u;
    const bool occ = occ_bit != 0u;
    h.blasIdx &= 0x7fffffffu;
    const bool found = h.dist != RT_LARGE_FLOAT;
    float ox, oy, oz, dx, dy, dz;
    frame_pixel_ray<CAM>(utab, vtab, W, H, frame, x, y, ox, oy, oz, dx, dy, dz);
    float r, g, b;
    shade_eval<STATS>(sc, p, ox, oy, oz, dx, dy, dz, h, found, occ, r, g, b, &ntex);
    dst[idx] = pack_rgb8(r, g, b);
    if (hits) { HitRec o = h; o.blasIdx |= occ_bit; hits[idx] = o; }   // bit 31 of blasIdx: the pixel's occlusion ray was blocked
    if (colors) { colors[3 * idx] = r; colors[3 * idx + 1] = g; colors[3 * idx + 2] = b; }
    npix = 1;
  }
  if (STATS && counters) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned v[2] = {ntex, npix};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      unsigned s = v[k];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
      if (lane == 0 && s) atomicAdd(counters + 5 + k, (unsigned long long)s);
    }
  }
}
template <bool STATS>
__global__ __launch_bounds__(256) void rt_shade_kernel(SceneDev sc, ShadeParams p, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t row_step,
                                                      uint32_t n_rows, const float* __restrict__ utab, const float* __restrict__ vtab,
                                                      const HitRec* __restrict__ hb, uint32_t* __restrict__ dst,
                                                      HitRec* __restrict__ hits, float* __restrict__ colors,
                                                      unsigned long long* counters, uint32_t* __restrict__ ctl_reset,
                                                      uint32_t lpt_blocks, const uint32_t* __restrict__ lpt_cost, uint32_t* __restrict__ lpt_order,
                                                      uint32_t lpt_tiles, uint32_t lpt_per_shard,
                                                      uint32_t batch = 1, const ShadeParams* __restrict__ pbatch = nullptr, uint64_t dst_frame_stride = 0,
                                                      const uint32_t* __restrict__ lpt_base = nullptr) {
  shade_pass<STATS, false>(sc, p, W, H, y0, y1, row_step, n_rows, utab, vtab, hb, dst, hits, colors, counters, ctl_reset, lpt_blocks, lpt_cost, lpt_order,
                           lpt_tiles, lpt_per_shard, batch, pbatch, dst_frame_stride, lpt_base);
}
// the shading pass of camera frames (vxrt_render_camera / vxrt_render_batch_camera): cam = the frame context's camera block.
// BATCH = false: one frame, whose camera head every lane reads at the same address -- scalar loads, the camera stays in SGPRs
template <bool BATCH>
__global__ __launch_bounds__(256) void rt_shade_camera_kernel(SceneDev sc, ShadeParams p, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t row_step,
                                                             uint32_t n_rows, const float* __restrict__ cam,
                                                             const HitRec* __restrict__ hb, uint32_t* __restrict__ dst,
                                                             HitRec* __restrict__ hits, float* __restrict__ colors, uint32_t* __restrict__ ctl_reset,
                                                             uint32_t lpt_blocks, const uint32_t* __restrict__ lpt_cost, uint32_t* __restrict__ lpt_order,
                                                             uint32_t lpt_tiles, uint32_t lpt_per_shard,
                                                             uint32_t batch, const ShadeParams* __restrict__ pbatch, uint64_t dst_frame_stride,
                                                             const uint32_t* __restrict__ lpt_base) {
  shade_pass<false, true>(sc, p, W, H, y0, y1, row_step, n_rows, cam, cam + CAM_TAB, hb, dst, hits, colors, nullptr, ctl_reset, lpt_blocks, lpt_cost, lpt_order,
                          lpt_tiles, lpt_per_shard, BATCH ? batch : 1u, pbatch, dst_frame_stride, lpt_base);
}

// closest-hit / miss shader of arbitrary (ray, hit record) pairs: what the RTU test's shaders compute for the ray a payload belongs
// to (closest.cpp:57-127 without a secondary ray, miss.cpp:9-14), e.g. for the hit records vxrt_trace returns
__global__ __launch_bounds__(256) void rt_shade_rays_kernel(SceneDev sc, ShadeParams p, uint64_t n, const float* __restrict__ rays,
                                                           const HitRec* __restrict__ hits, float* __restrict__ colors, uint32_t* __restrict__ rgb8) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float* rp = rays + i * 6;
  HitRec h = hits[i];
  h.blasIdx &= 0x7fffffffu;
  float r, g, b;
  shade_eval<false>(sc, p, rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], h, h.dist != RT_LARGE_FLOAT, false, r, g, b);
  if (colors) { colors[3 * i] = r; colors[3 * i + 1] = g; colors[3 * i + 2] = b; }
  if (rgb8) rgb8[i] = pack_rgb8(r, g, b);
}

// ---------------------------------------------------------------------------------------------
// Reference-quirks traversal (opt-in; vxrt_trace_reference_quirks).  The kernels above implement the CANONICAL algorithm (DESIGN.md
// s3), which returns what the reference's RTU returns wherever the reference addresses its own data.  The RTU does not always:
// children of a TLAS internal node that is popped from the short stack are addressed relative to the LAST BLAS's base_ptr
// (rt_traversal.cpp:91-92 after :119-120), so with a TLAS deeper than one level it reads unrelated memory and loses real hits.
// What it then returns depends on what lies at those addresses, i.e. on the memory layout -- so this mode works as the
// simulator does: on ONE flat memory image addressed with 32-bit offsets (the simulated RAM) and the four base pointers of the
// RTX DCRs, and it restates BVHTraverser::traverse literally: trail[32], the 5-entry short stack that forgets its oldest entry,
// the restart from the root when the stack is dry, a full re-descent after every accepted candidate (rt_unit.cpp:199-202),
// libstdc++ min/max in the slab test, the per-test edge subtractions.  One thread per ray: this is a compatibility mode, not a
// fast path.  Reads outside the image return zeros.  rt_traversal.cpp:80-86 spins 2^32 times without effect when
// trail[level] == 4 and no child passes: closed form here.  Depth > 32 overruns trail[] in the reference: status bit, ray ends.
// ---------------------------------------------------------------------------------------------
struct QuirkImage { const uint8_t* mem; uint64_t size; uint32_t tlas_ptr, blas_ptr, bvh_ptr, tri_ptr; };

__device__ __forceinline__ void q_read(const QuirkImage& im, uint32_t* dst, uint32_t addr, uint32_t dwords) {
  if ((uint64_t)addr + 4ull * dwords > im.size || (addr & 3u)) { for (uint32_t i = 0; i < dwords; ++i) dst[i] = 0u; return; }
  const uint32_t* p = (const uint32_t*)(im.mem + addr);
  for (uint32_t i = 0; i < dwords; ++i) dst[i] = p[i];
}

__global__ __launch_bounds__(64) void rt_quirks_trace_kernel(QuirkImage im, const float* __restrict__ rays, const float* __restrict__ tmax, uint64_t n,
                                                            HitRec* __restrict__ out, int any_hit_first, uint32_t* status) {
  const uint64_t r = (uint64_t)blockIdx.x * 64u + threadIdx.x;
  if (r >= n) return;
  const float* rp = rays + r * 6;
  const float ox = rp[0], oy = rp[1], oz = rp[2], dx = rp[3], dy = rp[4], dz = rp[5];
  HitRec hit; hit.dist = tmax ? tmax[r] : RT_LARGE_FLOAT; hit.bx = 0; hit.by = 0; hit.bz = 0; hit.blasIdx = 0; hit.triIdx = 0;
  if (hit.dist > RT_LARGE_FLOAT) hit.dist = RT_LARGE_FLOAT;
  uint8_t trail[RT_MAX_TRAIL];
  for (int i = 0; i < RT_MAX_TRAIL; ++i) trail[i] = 0;
  // ShortStack<TraversalStackEntry, 5> (types.h:1808-1840)
  uint32_t ss_ptr[5]; uint8_t ss_last[5]; uint32_t ss_head = 0, ss_count = 0;
  auto ss_push = [&](uint32_t ptr, uint8_t last) {
    if (ss_count < 5u) ss_count++;            // (a full stack overwrites its oldest entry: head wraps onto it)
    ss_ptr[ss_head] = ptr; ss_last[ss_head] = last;
    ss_head = (ss_head + 1u) % 5u;
  };
  bool accepted = false;
  bool limit = true;
  for (uint32_t guard = 0; guard < (1u << 16); ++guard) {   // one pass of traverse() per accepted candidate (a ray accepts a handful)
    uint32_t level = 0, base_ptr = im.tlas_ptr, node_ptr = im.tlas_ptr, blasIdx = 0;
    float cx = ox, cy = oy, cz = oz, cdx = dx, cdy = dy, cdz = dz;   // cur_ray
    bool finished = false, pending = false;
    float pending_dist = 0.f;
    // findNextParentLevel + pop (rt_traversal.cpp:171-213); true = traversal over
    auto pop = [&]() -> bool {
      int parent = -1;
      for (int i = (int)level - 1; i >= 0; --i) if (i < RT_MAX_TRAIL && trail[i] != 4) { parent = i; break; }
      if (parent < 0) return true;
      trail[parent]++;
      for (int i = parent + 1; i < RT_MAX_TRAIL; ++i) trail[i] = 0;
      if (ss_count == 0u) { base_ptr = im.tlas_ptr; node_ptr = im.tlas_ptr; level = 0; }
      else {
        ss_head = ss_head == 0u ? 4u : ss_head - 1u;
        ss_count--;
        node_ptr = ss_ptr[ss_head];
        if (ss_last[ss_head]) trail[parent] = 4;
        level = (uint32_t)parent + 1u;
      }
      return false;
    };
    uint32_t it = 0;
    for (; it < ITER_LIMIT && !finished && !pending; ++it) {
      uint32_t w[RT_NODE_DWORDS];
      q_read(im, w, node_ptr, RT_NODE_DWORDS);
      const uint32_t imask = w[3] >> 24, leftFirst = w[4], leafData = w[5];
      const bool top = imask == 1u;
      const bool leaf = top ? (leafData != 0xffffffffu) : (leafData != 0u);
      if (!leaf) {
        const float px = __uint_as_float(w[0]), py = __uint_as_float(w[1]), pz = __uint_as_float(w[2]);
        const int ex = (int)(int8_t)(w[3] & 0xff), ey = (int)(int8_t)((w[3] >> 8) & 0xff), ez = (int)(int8_t)((w[3] >> 16) & 0xff);
        const uint8_t* cb = (const uint8_t*)w + 24;
        float dist[4]; uint32_t child[4]; int cnt = 0;
        const float rox = top ? ox : cx, roy = top ? oy : cy, roz = top ? oz : cz;
        const float rdx = top ? dx : cdx, rdy = top ? dy : cdy, rdz = top ? dz : cdz;
        const float ix = 1.0f / rdx, iy = 1.0f / rdy, iz = 1.0f / rdz;
        for (int k = 0; k < 4; ++k) {
          const uint8_t* c = cb + 7 * k;
          if (c[0] == 0) continue;
          const float d = ray_box<true>(rox, roy, roz, ix, iy, iz,
                                        px + ldexpf((float)c[1], ex), py + ldexpf((float)c[2], ey), pz + ldexpf((float)c[3], ez),
                                        px + ldexpf((float)c[4], ex), py + ldexpf((float)c[5], ey), pz + ldexpf((float)c[6], ez));
          if (d < hit.dist) {
            // std::sort(a.dist > b.dist) on <= 4 elements = insertion sort: stable, farthest first (:76-78)
            int j = cnt;
            while (j > 0 && d > dist[j - 1]) { dist[j] = dist[j - 1]; child[j] = child[j - 1]; --j; }
            dist[j] = d; child[j] = (uint32_t)k;
            cnt++;
          }
        }
        if (level >= RT_MAX_TRAIL) { atomicOr(status, STATUS_STACK_OVERFLOW); finished = true; break; }
        const uint32_t kdrop = trail[level];
        const uint32_t drop = kdrop == 4u ? (uint32_t)cnt - 1u : kdrop;     // wraps when cnt == 0 (:81)
        if (drop >= (uint32_t)cnt) cnt = 0; else cnt -= (int)drop;
        if (cnt == 0) finished = pop();
        else {
          const uint32_t nearest = child[cnt - 1];
          cnt--;
          node_ptr = base_ptr + (leftFirst + nearest) * RT_NODE_BYTES;          // base_ptr may be STALE here: the quirk
          if (cnt == 0) trail[level] = 4;
          else for (int q = 0; q < cnt; ++q) ss_push(base_ptr + (leftFirst + child[q]) * RT_NODE_BYTES, q == 0 ? 1 : 0);
          level++;
        }
      } else if (top) {
        blasIdx = leafData;
        uint32_t bw[13];
        q_read(im, bw, im.blas_ptr + blasIdx * RT_BLAS_STRIDE, 13);
        const float m00 = __uint_as_float(bw[1]), m01 = __uint_as_float(bw[2]), m02 = __uint_as_float(bw[3]), m03 = __uint_as_float(bw[4]);
        const float m10 = __uint_as_float(bw[5]), m11 = __uint_as_float(bw[6]), m12 = __uint_as_float(bw[7]), m13 = __uint_as_float(bw[8]);
        const float m20 = __uint_as_float(bw[9]), m21 = __uint_as_float(bw[10]), m22 = __uint_as_float(bw[11]), m23 = __uint_as_float(bw[12]);
        cx = m00 * ox + m01 * oy + m02 * oz + m03; cy = m10 * ox + m11 * oy + m12 * oz + m13; cz = m20 * ox + m21 * oy + m22 * oz + m23;
        cdx = m00 * dx + m01 * dy + m02 * dz; cdy = m10 * dx + m11 * dy + m12 * dz; cdz = m20 * dx + m21 * dy + m22 * dz;
        base_ptr = im.bvh_ptr + bw[0] * RT_NODE_BYTES;
        node_ptr = base_ptr;
      } else {
        for (uint32_t i = 0; i < leafData && !pending; ++i) {
          const uint32_t triIdx = leftFirst + i;
          uint32_t tw[9];
          q_read(im, tw, im.tri_ptr + triIdx * RT_TRI_BYTES, 9);
          const float v0x = __uint_as_float(tw[0]), v0y = __uint_as_float(tw[1]), v0z = __uint_as_float(tw[2]);
          const float4 t0 = make_float4(v0x, v0y, v0z, __uint_as_float(tw[3]) - v0x);
          const float4 t1 = make_float4(__uint_as_float(tw[4]) - v0y, __uint_as_float(tw[5]) - v0z, __uint_as_float(tw[6]) - v0x, __uint_as_float(tw[7]) - v0y);
          const float4 t2 = make_float4(__uint_as_float(tw[8]) - v0z, 0.f, 0.f, 0.f);
          float bx, by, bz;
          const float d = ray_tri(cx, cy, cz, cdx, cdy, cdz, t0, t1, t2, bx, by, bz);
          if (d < hit.dist) {
            pending_dist = d; hit.bx = bx; hit.by = by; hit.bz = bz; hit.blasIdx = blasIdx; hit.triIdx = triIdx;
            ss_count = 0; ss_head = 0;     // :150-153 (an emptied stack pops nothing: head position is irrelevant)
            pending = true;
          }
        }
        if (!pending) finished = pop();
      }
    }
    if (!pending) { limit = !finished; break; }   // traversal completed -- or the iteration backstop ran out (reported below)
    hit.dist = pending_dist;                   // rt_unit.cpp:199-202 COMMIT_ACCEPT, then traverse again from the root with the kept trail
    accepted = true;
    if (any_hit_first) { limit = false; break; }
  }
  if (limit) atomicOr(status, STATUS_ITER_LIMIT);   // the walk did not end within the backstops (the reference would still be spinning)
  if (!accepted) { hit.dist = RT_LARGE_FLOAT; hit.bx = 0; hit.by = 0; hit.bz = 0; hit.blasIdx = 0; hit.triIdx = 0; }
  out[r] = hit;
}

// camera rays of rows [y0, y1) as a ray buffer (kernel.cpp:28-39; u, v in double as there -- IEEE division, so the same bits as the
// host-built tables of the frame kernels): ray (x, y) at index x + (y - y0) * W
__global__ __launch_bounds__(256) void rt_camera_rays_kernel(uint32_t W, uint32_t H, uint32_t y0, uint64_t n, float* __restrict__ rays) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = (uint32_t)(i % W), y = y0 + (uint32_t)(i / W);
  const float u = (float)(((double)x * 2.0 - (double)W) / (double)H), v = (float)(((double)y * 2.0 - (double)H) / (double)H);
  float* o = rays + i * 6;
  generate_ray(u, v, o[0], o[1], o[2], o[3], o[4], o[5]);
}

// rays of rows [y0, y1) of a caller-supplied pinhole camera (vxrt_pinhole_rays; pinhole.h), laid out as rt_camera_rays_kernel's
__global__ __launch_bounds__(256) void rt_pinhole_rays_kernel(vxrt_camera_t c, uint32_t W, uint32_t H, uint32_t y0, uint64_t n, float* __restrict__ rays) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = (uint32_t)(i % W), y = y0 + (uint32_t)(i / W);
  float* o = rays + i * 6;
  o[0] = c.pos[0]; o[1] = c.pos[1]; o[2] = c.pos[2];
  pinhole_dir(pinhole_ndc(x, W) * c.viewplane[0], pinhole_ndc(y, H) * c.viewplane[1], c.pos, c.forward, c.right, c.up, o[3], o[4], o[5]);
}

// the camera block of a camera frame / batch (see CAM_HDR), on the frame's stream: the cameras come by value through the kernel
// arguments, so nothing waits on the host and frames in flight on other contexts keep their own blocks
struct CamBatch { vxrt_camera_t c[VXRT_MAX_BATCH]; };
__global__ __launch_bounds__(256) void rt_camera_prep_kernel(CamBatch b, uint32_t n, uint32_t W, uint32_t H, float* __restrict__ out) {
  const uint32_t per = W + H;
  const uint64_t total = CAM_TAB + (uint64_t)n * per;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
    if (i < CAM_TAB) {   // heads of every slot (slots past n repeat camera 0)
      const uint32_t f = (uint32_t)i / CAM_HDR, k = (uint32_t)i % CAM_HDR;
      const vxrt_camera_t& c = b.c[f < n ? f : 0u];
      out[i] = k < 3 ? c.pos[k] : (k < 6 ? c.forward[k - 3] : (k < 9 ? c.right[k - 6] : c.up[k - 9]));
    } else {
      const uint64_t j = i - CAM_TAB;
      const uint32_t f = (uint32_t)(j / per), t = (uint32_t)(j % per);
      const vxrt_camera_t& c = b.c[f];
      out[i] = t < W ? pinhole_ndc(t, W) * c.viewplane[0] : pinhole_ndc(t - W, H) * c.viewplane[1];
    }
  }
}

struct ShadeBatch { ShadeParams p[VXRT_MAX_BATCH]; };
__global__ void set_batch_params_kernel(ShadeBatch b, uint32_t n, ShadeParams* __restrict__ dst) {
  if (threadIdx.x < n) dst[threadIdx.x] = b.p[threadIdx.x];
}

// Image assembly of a frame split by interleaved tile rows (vxrt_wire_pack / vxrt_wire_unpack in the header): 0x00RRGGBB pixels as 3 bytes on
// the wire.  One thread per 4 pixels = 16 bytes in, 12 bytes out (three aligned words), rows of the share contiguous on the wire.
__global__ __launch_bounds__(256) void wire_pack_kernel(const uint32_t* __restrict__ frames, uint64_t frame_stride, uint32_t W4, uint32_t per, uint32_t world, uint32_t rank,
                                                        uint64_t n_quads, uint32_t* __restrict__ wire) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n_quads) return;
  const uint32_t xq = (uint32_t)(t % W4);
  const uint64_t row = t / W4;                       // row of the wire: frame * per * 8 + j * 8 + y
  const uint32_t rows_per_frame = per * 8u;
  const uint32_t f = (uint32_t)(row / rows_per_frame), lr = (uint32_t)(row - (uint64_t)f * rows_per_frame);
  const uint32_t j = lr >> 3, y = lr & 7u;
  const uint4 p = *(const uint4*)(frames + (size_t)f * frame_stride + ((size_t)(j * world + rank) * 8u + y) * (W4 * 4u) + (size_t)xq * 4u);
  uint32_t* o = wire + t * 3u;
  o[0] = (p.x & 0xFFFFFFu) | (p.y << 24);
  o[1] = ((p.y >> 8) & 0xFFFFu) | (p.z << 16);
  o[2] = ((p.z >> 16) & 0xFFu) | (p.w << 8);
}
__global__ __launch_bounds__(256) void wire_unpack_kernel(const uint32_t* __restrict__ wire_all, uint64_t wire_stride_words, uint32_t W4, uint32_t per, uint32_t world,
                                                          uint64_t quads_per_rank, uint32_t* __restrict__ frames, uint64_t frame_stride) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= quads_per_rank * world) return;
  const uint32_t r = (uint32_t)(t / quads_per_rank);
  const uint64_t q = t - (uint64_t)r * quads_per_rank;
  const uint32_t xq = (uint32_t)(q % W4);
  const uint64_t row = q / W4;
  const uint32_t rows_per_frame = per * 8u;
  const uint32_t f = (uint32_t)(row / rows_per_frame), lr = (uint32_t)(row - (uint64_t)f * rows_per_frame);
  const uint32_t j = lr >> 3, y = lr & 7u;
  const uint32_t* w = wire_all + (size_t)r * wire_stride_words + q * 3u;
  const uint32_t a = w[0], b = w[1], c = w[2];
  uint4 p;
  p.x = a & 0xFFFFFFu;
  p.y = (a >> 24) | ((b & 0xFFFFu) << 8);
  p.z = (b >> 16) | ((c & 0xFFu) << 16);
  p.w = c >> 8;
  *(uint4*)(frames + (size_t)f * frame_stride + ((size_t)(j * world + r) * 8u + y) * (W4 * 4u) + (size_t)xq * 4u) = p;
}

// ---------------------------------------------------------------------------------------------
// host entry points (C ABI, include/vortex_hip.h level 2)
// ---------------------------------------------------------------------------------------------
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

static uint32_t* g_status[16] = {nullptr};

static uint32_t* status_word() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  if (!g_status[dev]) {
    if (hipMalloc((void**)&g_status[dev], sizeof(uint32_t)) != hipSuccess) return nullptr;
    (void)hipMemset(g_status[dev], 0, sizeof(uint32_t));
  }
  return g_status[dev];
}

#define LPT_MIN_TILES 20000u
#define LPT_BATCH_MAX_TILES 100000u
#ifndef EXACT_GRID
#define EXACT_GRID 128   // workgroups of the EXACT launch (it sees a fraction of a percent of the rays)
#endif

// Measurement knobs of the render and trace path (docs/KNOBS.md), read from the environment once per process: on the first call
// that asks for one.  Each keeps the parsing it always had (atoi, atoll, or "first character is 0").  (The three of the secondary
// tails, VXRT_PATH_BATCH, VXRT_AO_BATCH and VXRT_SORT_SECONDARY, are read the same way in rt_secondary.hip, for rt_path.hip as well.)
struct HostKnobs {
  uint32_t shard_rot, lpt_batch_max;
  bool lpt, lpt_batch;                  // on unless the value begins with '0'
  bool unordered_any_off, debug;        // VXRT_UNORDERED_ANY is 0; VXRT_DEBUG is set at all
  bool shadow_hints;                    // on unless VXRT_SHADOW_HINTS begins with '0'
  int lpt_batch_alone, side_reserve, packed, packed_batch, grid_div, pool, wgs_per_cu, grid_max;   // side_reserve, packed: -1 = unset
};
static const HostKnobs& host_knobs() {
  static const HostKnobs knobs = [] {
    const auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    const auto not_off = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
    HostKnobs k;
    k.shard_rot = (uint32_t)num("VXRT_SHARD_ROT", 0);
    k.lpt = not_off("VXRT_LPT");
    k.lpt_batch = not_off("VXRT_LPT_BATCH");
    k.shadow_hints = not_off("VXRT_SHADOW_HINTS");
    { const char* e = getenv("VXRT_LPT_BATCH_MAX"); k.lpt_batch_max = e ? (uint32_t)atoll(e) : LPT_BATCH_MAX_TILES; }
    k.lpt_batch_alone = num("VXRT_LPT_BATCH_ALONE", 1);
    k.side_reserve = num("VXRT_SIDE_RESERVE", -1);
    k.packed = num("VXRT_PACKED", -1);
    k.packed_batch = num("VXRT_PACKED_BATCH", 0);
    k.grid_div = num("VXRT_GRID_DIV", 0);
    k.pool = num("VXRT_POOL", 0);
    { const char* e = getenv("VXRT_UNORDERED_ANY"); k.unordered_any_off = e && atoi(e) == 0; }
    k.wgs_per_cu = num("VXRT_WGS_PER_CU", 0);
    k.grid_max = num("VXRT_GRID_MAX", 0);
    k.debug = getenv("VXRT_DEBUG") != nullptr;
    return k;
  }();
  return knobs;
}

// what the device holds of a persistent kernel at once: occupancy x CUs, queried once per kernel and device
template <class K>
static uint64_t persistent_held(K kernel, int wg_threads = RT_WG_THREADS) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, uint64_t> cache;
  int dev = 0;
  (void)hipGetDevice(&dev);
  uint64_t g = 0;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find({(const void*)kernel, dev});
    if (it != cache.end()) g = it->second;
  }
  if (!g) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, wg_threads, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    // measurement knob (tools/occupancy_sweep.sh): fewer resident workgroups per CU than the kernel allows
    if (const int v = host_knobs().wgs_per_cu; v >= 1 && v < per_cu) per_cu = v;
    g = (uint64_t)per_cu * (uint64_t)cus;
    if (host_knobs().debug) fprintf(stderr, "[vxrt] persistent grid: %d blocks/CU x %d CUs\n", per_cu, cus);
    std::lock_guard<std::mutex> lk(mu);
    cache[{(const void*)kernel, dev}] = g;
  }
  return g;
}
// grid of a persistent launch: what the device holds at once, capped by the job count and by VXRT_GRID_MAX (rt_launch_plan.h)
template <class K>
static uint32_t persistent_grid(K kernel, uint64_t jobs, int wg_threads = RT_WG_THREADS) {
  return plan_persistent_grid(persistent_held(kernel, wg_threads), jobs, (uint32_t)wg_threads, host_knobs().grid_max);
}

// next frame context, ordered on `s` behind its previous use
static FrameCtx* acquire_ctx(vxrt_accel* a, hipStream_t s) {
  if (!a->stream_seen) { a->stream_seen = true; a->first_stream = s; } else if (s != a->first_stream) a->multi_stream = true;
  // the context this stream used last (no event hop: the stream orders the two frames), else one never used, else round robin.
  // (Plain round robin pairs contexts with streams only while the caller's stream rotation and the call count stay in step: an odd
  // number of warm-up frames was enough to put every later frame behind a cross-stream event wait, -3 %.)
  uint32_t pick = a->n_ctx;
  for (uint32_t k = 0; k < a->n_ctx && pick == a->n_ctx; ++k) { const uint32_t i = (a->next_ctx + k) % a->n_ctx; if (a->ctx[i].busy && a->ctx[i].last_stream == s) pick = i; }
  for (uint32_t k = 0; k < a->n_ctx && pick == a->n_ctx; ++k) { const uint32_t i = (a->next_ctx + k) % a->n_ctx; if (!a->ctx[i].busy) pick = i; }
  if (pick == a->n_ctx) pick = a->next_ctx % a->n_ctx;
  a->next_ctx = pick + 1;
  FrameCtx& c = a->ctx[pick];
  if (!c.inited) {   // (a failed attempt is completed by the next one: every piece is created only if still missing)
    // the side stream carries the small EXACT launch over the a-priori list: highest priority, so that its few workgroups are
    // placed before the main launch fills every CU (an EXACT workgroup cannot co-reside with a full persistent grid: LDS)
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (!c.side && hipStreamCreateWithPriority(&c.side, hipStreamNonBlocking, hi) != hipSuccess) return nullptr;
    if (!c.ev_in && hipEventCreateWithFlags(&c.ev_in, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (!c.ev_side && hipEventCreateWithFlags(&c.ev_side, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (!c.ev_done && hipEventCreateWithFlags(&c.ev_done, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (!c.ctl && hipMalloc((void**)&c.ctl, CTL_DWORDS * sizeof(uint32_t)) != hipSuccess) return nullptr;
    if (hipMemset(c.ctl, 0, CTL_DWORDS * sizeof(uint32_t)) != hipSuccess) return nullptr;
    c.inited = true;
  }
  if (c.busy && c.last_stream != s) {   // (same stream: already ordered)
    if (c.done_recorded) { if (hipStreamWaitEvent(s, c.ev_done, 0) != hipSuccess) return nullptr; }
    else if (hipStreamSynchronize(c.last_stream) != hipSuccess) {
      // (the accel's first call on a second stream: see release_ctx.)  The first stream may have been destroyed by its owner in the
      // meantime -- destroying a stream completes its work, but the handle is stale: order behind the whole device instead, and only
      // a failure of that is a failure of the call (the context must not stay unusable behind a dead handle)
      (void)hipGetLastError();
      if (hipDeviceSynchronize() != hipSuccess) return nullptr;
    }
    c.busy = false; c.last_stream = nullptr;
  }
  if (c.ctl_dirty) {
    if (hipMemsetAsync(c.ctl, 0, CTL_DWORDS * sizeof(uint32_t), s) != hipSuccess) return nullptr;
    c.ctl_dirty = false;
  }
  return &c;
}

// The completion event orders a context's next use on ANOTHER stream.  An accel that has only ever seen one stream (serial frames,
// the vx_* sequence) does not pay for it -- an event record is a barrier packet on the stream, ~10 us between a frame's shading
// launch and the next frame's traversal -- and the first call on a second stream waits for the first stream on the host instead.
static int release_ctx(vxrt_accel* a, FrameCtx* c, hipStream_t s) {
  c->done_recorded = a->multi_stream || a->n_ctx > 1;
  if (c->done_recorded && hipEventRecord(c->ev_done, s) != hipSuccess) return -1;
  c->busy = true; c->last_stream = s;
  return 0;
}

extern "C" uint32_t* vxrt_status_word_device(void) { return status_word(); }   // shared with rc_kernels.hip (not part of the public header)

// The longest-first tile order of a frame for the software twin's launch (rc_kernels.hip; internal, not part of the public header): the same
// per-band counting sort the RTU path's shading launch carries (lpt_order_block), as a launch of QUEUE_SHARDS workgroups that also zeroes the
// `clear_dwords` words at `clear` (the twin's queue counters, for its next frame).
__global__ __launch_bounds__(256) void lpt_sort_kernel(const uint32_t* __restrict__ cost, uint32_t* __restrict__ order, uint32_t n_tiles, uint32_t tiles_per_shard,
                                                       uint32_t* __restrict__ clear, uint32_t clear_dwords) {
  __shared__ uint32_t s_hist[2048 + 8];
  if (clear && blockIdx.x == 0) for (uint32_t i = threadIdx.x; i < clear_dwords; i += 256u) clear[i] = 0u;
  lpt_order_block(blockIdx.x, cost, order, n_tiles, tiles_per_shard, s_hist, nullptr);
}
extern "C" int vxrt_internal_lpt_sort(const uint32_t* cost, uint32_t* order, uint32_t n_tiles, uint32_t tiles_per_shard, uint32_t* clear, uint32_t clear_dwords, void* stream) {
  hipLaunchKernelGGL(lpt_sort_kernel, dim3(QUEUE_SHARDS), dim3(256), 0, (hipStream_t)stream, cost, order, n_tiles, tiles_per_shard, clear, clear_dwords);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

#include "rt_trace_experiments.inc"   // rt_pool_trace_kernel, rt_pair_trace_kernel, trace_experiment (VXRT_POOL=1|2)

static ShadeParams shade_params(const vxrt_shade_params_t& in) {
  ShadeParams p;
  for (int i = 0; i < 3; ++i) {
    p.amb[i] = in.ambient[i]; p.lcol[i] = in.light_color[i];
    p.lpos[i] = in.light_pos[i]; p.bg[i] = in.background[i];
  }
  p.max_depth = in.max_depth;
  return p;
}

// The two run-time bits of a scene that select a traversal instantiation -- the ldexp decode (dev.exact_decode) and the depth class
// (shallow: the size of the scratch part of the stack) -- as the template arguments LDEXP and SHALLOW: calls
// f(std::bool_constant<LDEXP>, std::bool_constant<SHALLOW>).  Counting builds have no SHALLOW form: with ALLOW_SHALLOW = false it is
// not instantiated.
template <bool ALLOW_SHALLOW, class F>
static void with_decode_and_depth(const vxrt_accel* a, F&& f) {
  if constexpr (ALLOW_SHALLOW) {
    if (a->shallow) { if (a->dev.exact_decode) f(std::true_type{}, std::true_type{}); else f(std::false_type{}, std::true_type{}); return; }
  }
  if (a->dev.exact_decode) f(std::true_type{}, std::false_type{}); else f(std::false_type{}, std::false_type{});
}

// The two launches of a ray buffer: JOB over every ray, then the EXACT form over the rays it deferred (JOB_TRACE for the unordered
// job too: the EXACT launch keeps the ordered form, a boolean either way).
// (the EXACT launch's grid grows with the ray buffer -- a workgroup per 2,048 rays, up to the machine: how many rays were deferred
// is known on the device only, and a buffer of axis-parallel rays defers all of them; with nothing deferred its wavefronts find
// every shard empty without an atomic and exit)
// (ALPHA: the alpha-tested forms, which have no SHALLOW instantiation)
template <int JOB, int STATS, bool ALPHA = false>
static void launch_trace(const vxrt_accel* a, const ShadeParams& p, const PersistArgs& A, const PersistArgs& X, uint64_t n, hipStream_t s) {
  with_decode_and_depth<STATS == 0 && !ALPHA>(a, [&](auto ld, auto sh) {
    const auto k_main = rt_persistent_kernel<JOB, STATS, decltype(ld)::value, false, false, decltype(sh)::value, ALPHA>;
    const auto k_exact = rt_persistent_kernel<JOB_TRACE, STATS, decltype(ld)::value, true, false, false, ALPHA>;
    hipLaunchKernelGGL(k_main, dim3(persistent_grid(k_main, n)), dim3(RT_WG_THREADS), 0, s, a->dev, p, A);
    hipLaunchKernelGGL(k_exact, dim3(std::max<uint32_t>(EXACT_GRID, persistent_grid(k_exact, n / 8, 256))), dim3(256), 0, s, a->dev, p, X);
  });
}

// ray buffer -> hit records on frame context c (the body of vxrt_trace; also the ray buffers of the secondary tails: declared in
// rt_internal.h, with its default arguments and MODE_ANY_UNORDERED)
int trace_on_ctx(vxrt_accel_t* a, FrameCtx* c, const float* rays, uint64_t n, const float* tmax, HitRec* hits, int mode, hipStream_t s,
                 const uint32_t* n_dev, unsigned long long* stats_counters, const uint32_t* order) {
  uint32_t* st = status_word();
  if (!st) return -1;
  // a non-zero alpha table: the alpha-tested launches, timed build only (callers that cannot honour the table have refused already)
  const bool alpha = a->alpha_on;
  if (alpha && stats_counters) return -1;
  PersistArgs A{};
  A.alpha_tri = alpha ? a->alpha_tri : nullptr;
  const bool unordered = mode == MODE_ANY_UNORDERED;
  A.total = (uint32_t)n; A.hits = hits; A.rays = rays; A.tmax = tmax; A.any_hit = mode == VXRT_MODE_ANY || unordered;
  A.total_dev = n_dev;
  A.end_log = a->end_log;
  A.order = order;
  A.counters = stats_counters;
  A.wave_log = stats_counters ? a->trace_wave_log : nullptr;
  A.status = st;
  A.per_shard = ((A.total + QUEUE_SHARDS - 1) / QUEUE_SHARDS + 63u) & ~63u;
  if (!grow_device({{(void**)&c->defer, sizeof(uint32_t)}}, &c->defer_cap, A.total, GrowSync::STREAM, s)) return -1;
  if (c->ctl_dirty) {
    if (hipMemsetAsync(c->ctl, 0, CTL_DWORDS * sizeof(uint32_t), s) != hipSuccess) return -1;
  }
  // no kernel follows the EXACT launch that could zero the control block again: it stays dirty and the
  // next use of this context clears it with one fill
  c->ctl_dirty = true;
  A.defer_count = c->ctl; A.defer_list = c->defer; A.defer_cap = A.total;
  A.queue = c->ctl + 32;
  PersistArgs X = A;
  X.queue = c->ctl + 32 + CTL_QUEUE_DWORDS;
  X.total_dev = nullptr;   // the EXACT launch takes its count from the deferral list
  X.order = nullptr;
  ShadeParams p{};
  // incoherent rays: the ray-pool kernel (1) or two rays per lane (2) instead of the persistent kernel, timed builds only
  const int pool = host_knobs().pool;
  if ((pool == 1 || pool == 2) && !stats_counters && !alpha) return trace_experiment(pool, a, c, n, s, p, A, X);
  // any-hit rays whose caller only wants "blocked or not": children in slot order
  // (alpha-tested: one form for both -- the ordered one, whose answer to "blocked or not" is the same)
  if (alpha) launch_trace<JOB_TRACE, 0, true>(a, p, A, X, n, s);
  else if (stats_counters) launch_trace<JOB_TRACE, 1>(a, p, A, X, n, s);
  else if (unordered && !host_knobs().unordered_any_off) launch_trace<JOB_TRACE_UNORDERED, 0>(a, p, A, X, n, s);
  else launch_trace<JOB_TRACE, 0>(a, p, A, X, n, s);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------
// render_common, step by step: refusals, frame resources, launch plan, traversal launches, shading launch
// ---------------------------------------------------------------------------------------------

// tile rows of the window: every stride-th tile row of [y0, y1) starting with the one at y0
struct Tiles {
  uint32_t x, y;        // tiles per row, tile rows
  uint32_t row_step;    // frame rows between two consecutive tile rows
  uint32_t per_frame;
  uint64_t total;       // of the whole batch
};
static Tiles window_tiles(const RenderRequest& r) {
  Tiles t;
  t.x = (r.width + 7) / 8; t.y = ((r.y1 - r.y0 + 7) / 8 + r.stride - 1) / r.stride;
  t.row_step = 8u * r.stride;
  t.per_frame = t.x * t.y;
  t.total = (uint64_t)t.x * t.y * r.batch;
  return t;
}

static bool mirror_frame(const vxrt_accel* a, const vxrt_shade_params_t& params) { return params.max_depth > 1 && a->max_reflectivity > 0.0f; }
static bool gi_fused_frame(const RenderRequest& r) { return r.ao && r.ao->reserved == VXRT_AO_MODE_DIFFUSE_BOUNCE; }

// Every refusal that depends on the arguments alone.  It comes BEFORE a frame context is taken (a context taken and not released
// would leave its next user unordered behind whatever this call had already enqueued).  -1: refused; 0: an empty window, nothing
// to do; 1: render.
static int check_request(const vxrt_accel* a, const RenderRequest& r) {
  const bool stats = r.counting != Counting::TIMED;
  if (!a || a->stale || !r.params || !r.dst) return -1;
  // a non-zero alpha table (vxrt_accel_set_alpha_test): only the entry points that honour it render -- plain single frames, timed build
  if (a->alpha_on && (!r.honours_alpha || stats || r.wave_log || r.ao || r.batch != 1 || r.stride != 1)) return -1;
  // camera frames (cams[f] per frame of the batch): whole rows, the timed build only; plain and shadow frames, and single
  // ambient-occlusion / diffuse-bounce frames (`unoccluded` is an output of the ambient-occlusion frame alone)
  if (r.cams && (r.stride != 1 || stats || r.wave_log || (r.unoccluded && !r.ao))) return -1;
  // batch > 1: `params` is an array of `batch` entries, frame f goes to dst + f * dst_frame_stride; plain frames without optional outputs
  // (a batch with the wave log: diagnostic, traversal only -- its shading launch is the single-frame one)
  if (r.batch == 0 || r.batch > VXRT_MAX_BATCH) return -1;
  if (r.batch > 1 && (r.hits || r.colors || r.ao || ((stats || r.wave_log) && !(r.counting == Counting::TIMED_TRAVERSAL && r.wave_log)))) return -1;
  if (r.ao && (stats || r.shadow)) return -1;
  if (r.stride == 0 || (r.stride > 1 && ((r.y0 & 7u) != 0 || r.ao))) return -1;   // interleaved tile rows: tile-aligned start, plain frames only
  if (!a->ref.triEx || !a->ref.mat || a->ref.n_mats == 0) return -1;  // shading needs them (closest.cpp:52-55)
  if (r.width == 0 || r.height == 0 || r.y0 > r.y1 || r.y1 > r.height) return -1;
  if (stats && !r.counters) return -1;
  if (r.y0 == r.y1) return 0;
  if (window_tiles(r).total > 0x1ffffffull) return -1;   // (tile indices stay below 2^25: see FastDiv)
  // the mirror-bounce path: whole single frames, timed build only
  if (mirror_frame(a, r.params[0]) && (stats || r.stride > 1 || r.batch > 1)) return -1;
  if (r.batch > 1)
    for (uint32_t f = 0; f < r.batch; ++f)
      if (mirror_frame(a, r.params[f])) return -1;
  // path frames: whole rows of single frames, the timed build only, colours the one optional output besides the ray count
  if (r.path && (r.path->spp == 0 || r.path->spp > 4096 || r.path->bounces > VXRT_PATH_MAX_BOUNCES || r.path->shadow > 1 || stats || r.wave_log || r.ao ||
                 r.hits || r.unoccluded || r.batch != 1 || r.stride != 1)) return -1;
  // ... with a sample count per pixel: a path frame (a null buffer is vxrt_render_path_adaptive's to refuse: here it means "no counts")
  if (r.sample_counts && !r.path) return -1;
  // ... with emissive geometry: a path frame (with counts, a filter, a history as any other: only vxrt_render_path_frame can ask for
  // them together); the parameters, and for emitter sampling a valid table
  if (r.emissive && (!r.path || r.emissive->nee > 1u ||
                     r.emissive->reserved[0] != 0u || r.emissive->reserved[1] != 0u || !(r.emissive->scale >= 0.0f) || !std::isfinite(r.emissive->scale) ||
                     (r.emissive->nee == 1u && !emitters_valid(a)))) return -1;
  // ... with both estimators of emissive geometry weighted: what the emissive frame with emitter sampling asks for, in a request field
  // of its own (the entry point is its own; the two fields exclude each other)
  if (r.emissive_mis && (!r.path || r.emissive ||
                         r.emissive_mis->reserved[0] != 0u || r.emissive_mis->reserved[1] != 0u || r.emissive_mis->reserved[2] != 0u ||
                         !(r.emissive_mis->scale >= 0.0f) || !std::isfinite(r.emissive_mis->scale) || !emitters_valid(a))) return -1;
  // ... whose vertices may be specular (enable = 1; the entry point passes none for enable = 0): a path frame without the filter chain
  if (r.specular && (!r.path || r.specular->enable != 1u || r.specular->reserved[0] != 0u || r.specular->reserved[1] != 0u || r.specular->reserved[2] != 0u ||
                     r.denoise || r.aov || r.temporal || r.history || r.motion || r.prev_position || r.variance || r.variance_out)) return -1;
  // ... denoised: the filter's parameters (a path frame honours no alpha table, so neither does this one)
  if ((r.denoise || r.aov) && (!r.path || !dn_params_ok(r.denoise))) return -1;
  // ... with temporal accumulation: a camera frame with a history (render_path_frame, rt_path.hip, has checked the history against the window)
  if ((r.temporal || r.history) && (!r.denoise || !r.cams || !r.temporal || !r.history)) return -1;
  // ... through moved instances: the accel holds a motion snapshot
  if ((r.motion || r.prev_position) && (!r.motion || !r.temporal || a->motion_what == 0u)) return -1;
  // ... with variance guidance: a temporal frame (render_path_frame has checked that the history holds moments)
  if ((r.variance || r.variance_out) && (!r.temporal || !vr_params_ok(r.variance))) return -1;
  // one diffuse bounce: a plain frame of the timed build
  if (gi_fused_frame(r) && (stats || r.shadow || r.unoccluded)) return -1;
  // a path frame with Russian roulette (enable = 1; the entry point passes none for enable = 0): its parameters, and no specular
  // vertices beside it -- there thr is updated when the ray leaves, and a division before or after the albedo breaks that section's identity A
  if (r.roulette && (!r.path || r.roulette->enable != 1u || r.roulette->first < 1u || r.roulette->first > VXRT_PATH_MAX_BOUNCES ||
                     !std::isfinite(r.roulette->q_min) || !(r.roulette->q_min > 0.0f) || !(r.roulette->q_min <= 1.0f) || r.roulette->reserved != 0u ||
                     r.specular)) return -1;
  // a path frame lit by an environment map: its parameters, and neither an emitter form (three-way weighting is a design of its own)
  // nor specular vertices beside it
  if (r.env && (!r.path || !env_params_ok(r.env) || r.emissive || r.emissive_mis || r.specular)) return -1;
  return 1;
}

// Longest tile first, learned from this context's previous frame of the same window?
static bool lpt_wanted(const vxrt_accel* a, const RenderRequest& r, uint32_t n_tiles) {
  const HostKnobs& k = host_knobs();
  if (!k.lpt || !(r.counting == Counting::TIMED || r.wave_log)) return false;   // (VXRT_LPT=0 disables)
  // only for frames of more than LPT_MIN_TILES tiles: below, the sort launch costs more than the shorter tail saves
  // (1024x1024, 86 % background: -5 %; 1920x1080: +9 %; 3840x2160: +4 %; the sort on a side stream instead: worse, the
  // two extra event hops cost more than the kernel)
  if (n_tiles < LPT_MIN_TILES) return false;
  // Only with one frame in flight: overlapped frames fill each other's tails already.
  // Single frames in flight on several streams: no difference, measured (round 2).
  if (r.batch == 1) return a->n_ctx == 1;
  // BATCHES of frames: a rank's share of a frame split
  // over GPUs makes short launches -- at 8 ranks a 20-step run is two launches of ~5 tiles per wavefront, whose tails nothing
  // fills -- and the batches of a frame loop repeat: the order is learned from the context's previous batch of the same size
  // (VXRT_LPT_BATCH=0 disables; profiles/r03_h_lpt_batch.txt).
  if (!k.lpt_batch) return false;
  // ... for batches of at most LPT_BATCH_MAX_TILES tiles (about a dozen per resident wavefront): measured on one box, driver-sized
  // runs, rank 0's pipeline of 8 / 4 / 2 ranks (40.8 K / 81.6 K / 162 K tiles per batch): +5.5 % / +2 % / 0; one GPU's batches of
  // five whole frames (162 K tiles, sets overlapping on two streams): -5 % -- sorted by cost, a band's tiles are no longer
  // traced next to their screen neighbours, and there the tails are filled anyway.  (VXRT_LPT_BATCH_MAX: measurement knob)
  if (n_tiles <= k.lpt_batch_max) return true;
  // (a set issued on its own -- one frame context: the samples of one vx_start -- has nothing behind it to fill its tail, whatever its size)
  // (longest tile first also in a large set then: the samples of `rt_host -s 5`, 162 K tiles, 2.25 -> 2.00 ms per vx_start; VXRT_LPT_BATCH_ALONE=0: off)
  return k.lpt_batch_alone && a->n_ctx == 1;
}

// camera tables of the fixed camera (u per column, v per row), rebuilt when the frame size changes
static bool ensure_uv_tables(vxrt_accel* a, uint32_t width, uint32_t height, hipStream_t s) {
  if (a->uv_w == width && a->uv_h == height) return true;
  // kernel.cpp:32-33 evaluated on the host in double, once per column and row
  std::vector<float> tab((size_t)width + height);
  for (uint32_t x = 0; x < width; ++x) tab[x] = (float)(((double)x * 2.0 - (double)width) / (double)height);
  for (uint32_t y = 0; y < height; ++y) tab[width + y] = (float)(((double)y * 2.0 - (double)height) / (double)height);
  a->uv_w = a->uv_h = 0;
  uint64_t none = 0;   // (always replaced.)  DEVICE: frames in flight on other streams read the old table
  if (!grow_device({{(void**)&a->uvtab, sizeof(float)}}, &none, tab.size(), GrowSync::DEVICE, s)) return false;
  if (hipMemcpy(a->uvtab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return false;
  a->uv_w = width; a->uv_h = height;
  return true;
}

// the camera block lives in the frame context and is written on the frame's stream: the fixed camera's tables and a-priori
// list stay untouched, and frames in flight on other contexts keep their own cameras
static bool upload_cameras(FrameCtx* c, const RenderRequest& r, hipStream_t s) {
  const uint64_t need = CAM_TAB + (uint64_t)r.batch * (r.width + r.height);
  if (!grow_device({{(void**)&c->cam, sizeof(float)}}, &c->cam_floats, need, GrowSync::STREAM, s)) return false;
  CamBatch cb;
  for (uint32_t f = 0; f < VXRT_MAX_BATCH; ++f) cb.c[f] = r.cams[f < r.batch ? f : 0];
  const uint32_t g = (uint32_t)std::min<uint64_t>((need + 255) / 256, 1024);
  hipLaunchKernelGGL(rt_camera_prep_kernel, dim3(g), dim3(256), 0, s, cb, r.batch, r.width, r.height, c->cam);
  return hipGetLastError() == hipSuccess;
}

// a batch's per-frame shading parameters (into the context) and its band-major tile order (kept by the accel per batch size)
static bool upload_batch(vxrt_accel* a, FrameCtx* c, const RenderRequest& r, const Tiles& t, hipStream_t s) {
  if (!c->pbatch && hipMalloc((void**)&c->pbatch, VXRT_MAX_BATCH * sizeof(ShadeParams)) != hipSuccess) return false;
  // (by value through the kernel arguments: captured when the launch is enqueued, whatever the caller does with `params` next)
  ShadeBatch sb;
  for (uint32_t f = 0; f < VXRT_MAX_BATCH; ++f) sb.p[f] = shade_params(r.params[f < r.batch ? f : 0]);
  hipLaunchKernelGGL(set_batch_params_kernel, dim3(1), dim3(64), 0, s, sb, r.batch, c->pbatch);
  // tile order of a batch: band-major -- queue shard s (= the XCD that works on it) gets band s of EVERY frame, so that an
  // XCD's L2 keeps holding one band's part of the BVH, as it does for a single frame; frame-major order would hand each XCD
  // whole frames (measured at 8 frames per batch: slower than no batch at all)
  if (a->bo_tiles != t.per_frame) {   // another window: drop the orders of the old one
    if (hipDeviceSynchronize() != hipSuccess) return false;
    for (uint32_t k = 0; k <= VXRT_MAX_BATCH; ++k) { (void)hipFree(a->batch_order[k]); a->batch_order[k] = nullptr; }
    a->bo_tiles = t.per_frame;
  }
  if (!a->batch_order[r.batch]) {
    std::vector<uint32_t> ord;
    ord.reserve(t.total);
    const uint32_t band = (t.per_frame + QUEUE_SHARDS - 1) / QUEUE_SHARDS;
    for (uint32_t sh = 0; sh < QUEUE_SHARDS; ++sh)
      for (uint32_t f = 0; f < r.batch; ++f)
        for (uint32_t k = sh * band; k < std::min(t.per_frame, (sh + 1) * band); ++k) ord.push_back(f * t.per_frame + k);
    if (hipMalloc((void**)&a->batch_order[r.batch], ord.size() * sizeof(uint32_t)) != hipSuccess) return false;
    if (hipMemcpy(a->batch_order[r.batch], ord.data(), ord.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return false;
  }
  return true;
}

// the context's cost and order tables for sets of `batch` frames; A gets the cost table and, once a frame of this window has been
// sorted, the learned order
static bool ensure_lpt_tables(FrameCtx* c, const RenderRequest& r, uint32_t n_tiles, PersistArgs& A, hipStream_t s) {
  FrameCtx::Lpt& L = c->lpt[r.batch];
  const bool grows = L.cap < n_tiles;
  // (cost: n entries + n start clocks + n durations + n steal distances behind them, the latter three written by the wave-log build only)
  if (!grow_device({{(void**)&L.cost, 4 * 4}, {(void**)&L.order, 4}}, &L.cap, n_tiles, GrowSync::STREAM, s)) return false;
  if (grows) L.valid = false;
  // (camera frames learn their own order: they do not share the fixed camera's tiles' costs)
  const uint32_t key[6] = {r.width, r.height, r.y0, r.y1, (uint32_t)r.shadow | (r.stride << 1), (r.ao || r.path ? 1u : 0u) | (r.batch << 1) | (r.cams ? 0x80000000u : 0u)};
  if (memcmp(key, L.key, sizeof key) != 0) { L.valid = false; memcpy(L.key, key, sizeof key); }
  if (!L.cost || !L.order) return false;   // (whatever happened above: no launch with a missing table)
  A.tile_cost = L.cost;
  if (L.valid) A.tile_order = L.order;      // else: the static order (identity, or the batch's band-major order)
  else if (r.batch == 1) A.tile_order = nullptr;
  return true;
}

// Shadow hints (RT_SHADOW_HINTS): the context's hint words for the frame's hit-record slots, handed to the launch in A.  Only a timed shadow
// frame of an accel that takes the identity-root kernels and holds a path table can get them, and only when it REPEATS the frame the context
// rendered last -- same window, same light (every frame of a set), same cameras, no refit since: a hint for another light fails too often,
// and a failed hint costs more than a right one saves (a light that moves 1 - 5 units per frame: 24 - 30 % of the blocked rays still guided,
// the sequence 0.15 - 0.3 % slower than without hints).  Every other launch leaves A without them and takes the kernels without hints
// (JOB_NOHINTS): a sequence whose light, camera or geometry moves runs exactly what it ran before hints existed.  The first repeat of a
// frame starts from 0xFFFFFFFF words (no hint), set on the stream in front of the launch, and leaves its blockers; the second follows them.
// The buffer has a capacity of its own, apart from hitbuf's: most contexts never repeat a frame and never allocate it.
// VXRT_SHADOW_HINTS=0 (host_knobs) leaves the hints out; vxrt_debug_shadow_hints_enable overrides it for the tests.
static std::atomic<int> g_shadow_hints_override{-1};   // -1: as the environment says
static bool ensure_shadow_hints(vxrt_accel* a, FrameCtx* c, const RenderRequest& r, uint64_t slots, PersistArgs& A, hipStream_t s) {
  if (!RT_SHADOW_HINTS || !r.shadow || r.ao || r.path || r.counting != Counting::TIMED || !a->tri_path || !ident_root_form(a)) return true;
  if (const int ov = g_shadow_hints_override.load(); ov == 0 || (ov < 0 && !host_knobs().shadow_hints)) return true;
  // Is this the frame the context rendered last?  Same window, same light in every frame of the set, same cameras, no refit in between.
  const uint32_t key[6] = {r.width, r.height, r.y0, r.y1, (uint32_t)r.shadow | (r.stride << 1), (r.batch << 1) | (r.cams ? 0x80000000u : 0u)};
  std::vector<float> sig;
  sig.reserve((size_t)r.batch * (3 + (r.cams ? 14 : 0)));
  for (uint32_t f = 0; f < r.batch; ++f) {
    sig.insert(sig.end(), r.params[f].light_pos, r.params[f].light_pos + 3);
    if (r.cams) { const float* cf = (const float*)&r.cams[f]; sig.insert(sig.end(), cf, cf + sizeof(vxrt_camera_t) / sizeof(float)); }
  }
  const bool again = c->hint_sig_set && memcmp(key, c->hint_key, sizeof key) == 0 && c->hint_gen == a->scene_gen && sig.size() == c->hint_sig.size() &&
                     memcmp(sig.data(), c->hint_sig.data(), sig.size() * sizeof(float)) == 0;   // (bit patterns: a NaN light never repeats itself)
  if (!again) {
    // another frame: its hints would be stale, and a hint that fails costs more than it saves (profiles/r25_d_moving_light.txt).  The launch
    // goes without (JOB_NOHINTS: the kernel it ran before hints existed); what the context holds is void from here on.
    memcpy(c->hint_key, key, sizeof key); c->hint_sig.swap(sig); c->hint_gen = a->scene_gen; c->hint_sig_set = true;
    c->hints_valid = false;
    return true;
  }
  const bool grows = c->hints_cap < slots;
  if (!grow_device({{(void**)&c->hints, sizeof(uint32_t)}}, &c->hints_cap, slots, GrowSync::STREAM, s)) return false;
  if (grows || !c->hints_valid) {   // the first repeat of a frame starts from no hints and leaves its own
    c->hints_valid = false;
    if (hipMemsetAsync(c->hints, 0xFF, (size_t)c->hints_cap * sizeof(uint32_t), s) != hipSuccess) return false;
    c->hints_valid = true;
  }
  A.hints = c->hints; A.tri_path = a->tri_path; A.n_path_tris = a->ref.n_tris;
  c->hint_seq = ++a->hint_seq;   // (which context a stream hinted last: vxrt_debug_set_shadow_hints)
  return true;
}

// a-priori EXACT list (camera rays with u == 0 or v == 0), rebuilt only when the window changes.  The list of a batch is the
// frames' lists one after the other, so a list built for F frames serves every batch <= F: the launch takes a prefix.
static bool ensure_apriori(vxrt_accel* a, const RenderRequest& r, const Tiles& t, hipStream_t s) {
  if (a->ap_key[0] == r.width && a->ap_key[1] == r.height && a->ap_key[2] == r.y0 && a->ap_key[3] == r.y1 && a->ap_key[4] == r.stride && a->ap_key[5] >= r.batch && a->apriori) return true;
  std::vector<uint32_t> list(1, 0u);
  for (uint32_t k = 0; k < t.per_frame; ++k)
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t x = (k % t.x) * 8u + (l & 7u), y = r.y0 + (k / t.x) * t.row_step + (l >> 3);
      if (x >= r.width || y >= r.y1) continue;
      const float u = (float)(((double)x * 2.0 - (double)r.width) / (double)r.height);
      const float v = (float)(((double)y * 2.0 - (double)r.height) / (double)r.height);
      if (u == 0.0f || v == 0.0f) list.push_back(k * 64u + l);
    }
  const size_t per_frame = list.size() - 1;
  for (uint32_t f = 1; f < r.batch; ++f)
    for (size_t i = 0; i < per_frame; ++i) list.push_back(list[1 + i] + f * t.per_frame * 64u);
  list[0] = (uint32_t)(list.size() - 1);
  if (hipDeviceSynchronize() != hipSuccess) return false;   // (whether or not the list grows: frames in flight read the one it overwrites)
  if (!grow_device({{(void**)&a->apriori, sizeof(uint32_t)}}, &a->ap_cap, list.size(), GrowSync::NONE, s)) return false;
  if (hipMemcpy(a->apriori, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return false;
  a->ap_count = (uint32_t)per_frame;      // per frame
  a->ap_key[0] = r.width; a->ap_key[1] = r.height; a->ap_key[2] = r.y0; a->ap_key[3] = r.y1; a->ap_key[4] = r.stride; a->ap_key[5] = r.batch;
  return true;
}

// Everything the frame's launches read, grown or rebuilt where the request needs it, and the argument block A of the main launch
static bool frame_resources(vxrt_accel* a, FrameCtx* c, const RenderRequest& r, const Tiles& t, bool lpt, PersistArgs& A, hipStream_t s) {
  const uint32_t n_tiles = (uint32_t)t.total;
  // hit-record buffer between the two passes (one per frame in flight)
  const uint64_t pixels = r.batch > 1 ? (uint64_t)n_tiles * 64u : (uint64_t)t.x * ((r.height + 7) / 8 + 1) * 64u;   // tile-major records of any row window of the frame
  if (!grow_device({{&c->hitbuf, sizeof(HitRec)}}, &c->hitbuf_pixels, pixels, GrowSync::STREAM, s)) return false;
  if (!r.cams && !ensure_uv_tables(a, r.width, r.height, s)) return false;
  A.W = r.width; A.H = r.height; A.y0 = r.y0; A.y1 = r.y1; A.tiles_x = t.x; A.row_step = t.row_step; A.total = n_tiles * 64u;
  A.div_tiles_x = fast_div_make(t.x); A.div_frame_tiles = fast_div_make(t.per_frame); A.frame_tiles = t.per_frame;
  A.hits = (HitRec*)c->hitbuf; A.counters = r.counters; A.wave_log = r.wave_log; A.end_log = a->end_log;
  A.utab = a->uvtab; A.vtab = a->uvtab + r.width;
  if (r.cams) {
    if (!upload_cameras(c, r, s)) return false;
    A.utab = c->cam; A.vtab = c->cam + CAM_TAB;
  }
  if (r.batch > 1) {
    if (!upload_batch(a, c, r, t, s)) return false;
    A.pbatch = c->pbatch; A.tile_order = a->batch_order[r.batch];
  }
  if (!grow_device({{(void**)&c->defer, sizeof(uint32_t)}}, &c->defer_cap, A.total, GrowSync::STREAM, s)) return false;
  A.defer_count = c->ctl; A.defer_list = c->defer; A.defer_cap = A.total;
  A.queue = c->ctl + 32;
  A.per_shard = ((A.total + QUEUE_SHARDS - 1) / QUEUE_SHARDS + 63u) & ~63u;
  A.shard_rot = host_knobs().shard_rot;
  A.alpha_tri = a->alpha_on ? a->alpha_tri : nullptr;   // (check_request has refused every request that cannot honour it)
  if (lpt && !ensure_lpt_tables(c, r, n_tiles, A, s)) return false;
  if (!ensure_shadow_hints(a, c, r, pixels, A, s)) return false;
  // (camera frames have no a-priori list: their primary rays outside the fast domain are deferred to the EXACT launch behind the main one)
  return r.cams || ensure_apriori(a, r, t, s);
}

// How the frame's traversal is launched
struct LaunchPlan {
  bool lpt;             // longest tile first (see lpt_wanted); the shading launch then sorts the tiles for the context's next frame
  // frames packed in overlapping sets: the 8-wavefront instantiation (see rt_persistent_kernel); VXRT_PACKED=0/1 forces it
  // (VXRT_PACKED_BATCH, a measurement knob: sets of frames take it even with one frame context)
  bool packed;
  bool side_launch;     // an EXACT launch over the a-priori list on the side stream, concurrent with the main launch
  // the a-priori EXACT launch needs a few workgroups (3,000 rays of a 1080p frame = 12); the main launch leaves that many slots
  // free: a persistent grid that fills every CU (LDS) would otherwise keep them waiting until its first workgroups retire, and
  // the frame would end on them (measured: 33 us after the main launch, profiles/r02_d_exact_timeline.txt)
  uint32_t side_wgs;
  // ... on a serial frame.  With sets of frames overlapping on several streams the a-priori launch cannot get those slots anyway --
  // an EXACT workgroup needs more registers than one retired main workgroup frees, so it only finds room in a tail (measured:
  // it ends when its own main launch begins to drain, profiles/r03_a_pipeline_timeline.txt) -- and nothing waits for it before
  // the other stream's tail: the main launch takes the whole machine then, +1 % (serial: -7 %).  VXRT_SIDE_RESERVE=0/1 forces it.
  bool side_reserve;
  // A window that is small against the machine (one rank's share of a frame split N ways: at 1080p / 8 GPUs 4,080 tiles for 6,096
  // resident wavefronts) makes one launch a single round of tiles -- as long as its slowest tile, about half a full frame -- and a
  // second frame's launch only gets the slots the first one leaves.  With several frames in flight each launch therefore takes
  // its share of the machine (capacity / frames in flight): the frames run side by side, each wavefront working through several
  // tiles, and the machine stays full.  (A full frame, many tiles per wavefront, keeps the whole grid: measured better.)
  // VXRT_GRID_DIV=n forces the divisor for every window; a negative value switches it off.
  uint32_t grid_div;    // the main launch takes at most capacity / grid_div workgroups ...
  bool grid_div_small;  // ... only if its window is small against the machine (see main_grid)
};
static LaunchPlan launch_plan(const vxrt_accel* a, const RenderRequest& r, uint32_t n_tiles, bool lpt, uint32_t ap_count) {
  const HostKnobs& k = host_knobs();
  LaunchPlan plan;
  plan.lpt = lpt;
  plan.packed = k.packed >= 0 ? k.packed != 0 : ((a->n_ctx > 1 || (k.packed_batch && r.batch > 1)) && n_tiles >= LPT_MIN_TILES);
  plan.side_launch = ap_count != 0;
  plan.side_wgs = plan.side_launch ? std::min<uint32_t>(EXACT_GRID, (ap_count + 255u) / 256u) : 0u;
  plan.side_reserve = plan_side_reserve(k.side_reserve, a->n_ctx);
  plan.grid_div = plan_grid_div(k.grid_div, a->n_ctx);
  plan.grid_div_small = plan_grid_div_small(k.grid_div);
  return plan;
}

// grid of the main launch: what the machine holds of `kernel`, less the slots reserved for the side launch, divided as the plan says
template <class K>
static uint32_t main_grid(K kernel, const LaunchPlan& plan, uint32_t total) {
  return plan_main_grid(persistent_held(kernel), total, plan.side_wgs, plan.side_reserve, plan.grid_div, plan.grid_div_small, RT_WG_WAVES,
                        host_knobs().grid_max);
}

// what the three traversal launches of a frame share
struct FrameLaunch {
  const vxrt_accel* a; FrameCtx* c; const LaunchPlan& plan; const ShadeParams& p; hipStream_t s;
  PersistArgs A, X, X0;   // argument blocks of the main launch, of the EXACT launch over what it defers, of the a-priori EXACT launch
};

// EXACT launch over the a-priori list on the side stream, concurrent with the main launch; then the main launch and the EXACT
// launch over whatever the main one deferred.  (The EXACT form knows neither PACKED nor SHALLOW.)
// (ALPHA: the alpha-tested forms -- timed, neither PACKED nor SHALLOW)
// (IDENT: timed plain / shadow frames of an accel whose root is one identity instance -- ident_root_form, rt_internal.h -- take the
// main kernel without the TLAS level; their EXACT launches are the general ones)
template <int JOB, int STATS, bool PACKED, bool ALPHA = false>
static void launch_traversal(const FrameLaunch& l) {
  static_assert(!(PACKED && (job_base(JOB) == JOB_RENDER_GI || STATS != 0)), "only the timed render jobs have a packed form");
  const auto launch = [&](auto k_main, auto k_exact) {
    if (l.plan.side_launch) hipLaunchKernelGGL(k_exact, dim3(l.plan.side_wgs), dim3(256), 0, l.c->side, l.a->dev, l.p, l.X0);
    hipLaunchKernelGGL(k_main, dim3(main_grid(k_main, l.plan, l.A.total)), dim3(RT_WG_THREADS), 0, l.s, l.a->dev, l.p, l.A);
    hipLaunchKernelGGL(k_exact, dim3(EXACT_GRID), dim3(256), 0, l.s, l.a->dev, l.p, l.X);
  };
  if constexpr (RT_IDENT_ROOT_KERNEL && STATS == 0 && !ALPHA && job_base(JOB) != JOB_RENDER_GI) {
    if (ident_root_form(l.a)) {
      // (a shadow frame without hint words runs the kernel without hints: see JOB_NOHINTS)
      if constexpr (RT_SHADOW_HINTS && job_base(JOB) == JOB_RENDER_SHADOW) {
        if (!l.A.hints) {
          launch(rt_persistent_kernel<JOB | JOB_NOHINTS, 0, false, false, PACKED, true, false, true>, rt_persistent_kernel<JOB, 0, false, true, false, false, false>);
          return;
        }
      }
      launch(rt_persistent_kernel<JOB, 0, false, false, PACKED, true, false, true>, rt_persistent_kernel<JOB, 0, false, true, false, false, false>);
      return;
    }
  }
  with_decode_and_depth<STATS == 0 && !ALPHA>(l.a, [&](auto ld, auto sh) {
    launch(rt_persistent_kernel<JOB, STATS, decltype(ld)::value, false, PACKED, decltype(sh)::value, ALPHA>,
           rt_persistent_kernel<JOB, STATS, decltype(ld)::value, true, false, false, ALPHA>);
  });
}
template <int STATS, bool PACKED, int CAM = 0, bool ALPHA = false>
static void launch_render(bool shadow, const FrameLaunch& l) {
  if (shadow) launch_traversal<JOB_RENDER_SHADOW | CAM, STATS, PACKED, ALPHA>(l); else launch_traversal<JOB_RENDER | CAM, STATS, PACKED, ALPHA>(l);
}

// The traversal of the frame: fork the side stream, the three launches, join.  false: a HIP call failed.
static bool traverse_frame(vxrt_accel* a, FrameCtx* c, const RenderRequest& r, const LaunchPlan& plan, const ShadeParams& p, const PersistArgs& A, hipStream_t s) {
  FrameLaunch l{a, c, plan, p, s, A, A, A};
  l.X.queue = c->ctl + 32 + CTL_QUEUE_DWORDS;
  c->ctl_dirty = true;   // until the shading pass that zeroes the block again is enqueued
  if (plan.side_launch) {
    // the side stream starts behind what is queued on `s` (the previous frame's shading pass reads the hit records this launch writes) --
    // unless nothing is: a caller that waits for every frame before it starts the next (the vx_* sequence: vx_ready_wait, then vx_start)
    // finds the stream drained, and the fork's event record -- a barrier packet in front of the main launch, ~12 us -- is not needed
    const bool drained = hipStreamQuery(s) == hipSuccess;
    if (!drained && (hipEventRecord(c->ev_in, s) != hipSuccess || hipStreamWaitEvent(c->side, c->ev_in, 0) != hipSuccess)) return false;
    const uint32_t ap_count = a->ap_count * r.batch;   // the first `batch` frames of the list
    l.X0.queue = c->ctl + 32 + 2 * CTL_QUEUE_DWORDS;
    l.X0.defer_count = a->apriori; l.X0.defer_list = a->apriori + 1; l.X0.defer_cap = ap_count;
  }
  if (gi_fused_frame(r)) {
    // one diffuse bounce: the whole frame in the persistent launches (JOB_RENDER_GI).  (The multi-pass form it replaced -- list the hit
    // pixels, generate the rays, a 2 M-ray trace launch, accumulate, final -- took the same 1.18 ms: profiles/r03_f_gi_fused_ab.txt)
    // (dst, colors and gi_seed share their storage with the shadow hints' three words: ensure_shadow_hints leaves those out of every frame with
    // r.ao, and only the kernels of the timed shadow job read them -- a kernel that read A.dst in such a launch would write into the path table)
    for (PersistArgs* g : {&l.A, &l.X, &l.X0}) { g->dst = r.dst; g->colors = r.colors; g->gi_seed = r.ao->seed; }
    // (a camera frame has no a-priori list -- plan.side_launch is false: its primary rays outside the fast domain are deferred)
    if (r.cams) launch_traversal<JOB_RENDER_GI | JOB_CAM, 0, false>(l); else launch_traversal<JOB_RENDER_GI, 0, false>(l);
  }
  else if (l.A.alpha_tri) { if (r.cams) launch_render<0, false, JOB_CAM, true>(r.shadow != 0, l); else launch_render<0, false, 0, true>(r.shadow != 0, l); }
  else if (r.counting == Counting::TIMED_TRAVERSAL) launch_render<2, false>(r.shadow != 0, l);
  else if (r.counting == Counting::REFERENCE_ORDER) launch_render<1, false>(r.shadow != 0, l);
  else if (r.cams)      launch_render<0, false, JOB_CAM>(r.shadow != 0, l);
  else if (plan.packed) launch_render<0, true>(r.shadow != 0, l);
  else                  launch_render<0, false>(r.shadow != 0, l);
  return !plan.side_launch || (hipEventRecord(c->ev_side, c->side) == hipSuccess && hipStreamWaitEvent(s, c->ev_side, 0) == hipSuccess);
}

// The shading launch of a plain frame; with lpt_sort its first workgroups sort the tiles for the context's next frame
static bool shade_frame(vxrt_accel* a, FrameCtx* c, const RenderRequest& r, const Tiles& t, bool lpt_sort, const ShadeParams& p, const PersistArgs& A, hipStream_t s) {
  const FrameCtx::Lpt& L = c->lpt[r.batch];
  const uint32_t n_tiles = (uint32_t)t.total, n_rows = t.y * 8u;
  const uint64_t npx = (uint64_t)r.width * n_rows * r.batch;
  const uint32_t lpt_blocks = lpt_sort ? QUEUE_SHARDS : 0u;
  const dim3 sgrid((uint32_t)((npx + 255) / 256) + lpt_blocks), block(256);
  const uint32_t* base_order = r.batch > 1 ? (const uint32_t*)a->batch_order[r.batch] : (const uint32_t*)nullptr;
  // (the camera kernels take the camera block for the two tables and have no counters: a launch per signature)
  if (r.cams) {
    hipLaunchKernelGGL(r.batch > 1 ? rt_shade_camera_kernel<true> : rt_shade_camera_kernel<false>, sgrid, block, 0, s, a->dev, p, r.width, r.height, r.y0, r.y1, t.row_step,
                       n_rows, (const float*)A.utab, (const HitRec*)c->hitbuf, r.dst, (HitRec*)r.hits, r.colors, c->ctl, lpt_blocks, (const uint32_t*)L.cost,
                       L.order, n_tiles, A.per_shard >> 6, r.batch, (const ShadeParams*)c->pbatch, r.dst_frame_stride, base_order);
  } else {
    // (the counting build shades single frames only: the one set of frames it sees, the wave-log diagnostic, is traversal only)
    const bool stats = r.counting != Counting::TIMED;
    hipLaunchKernelGGL(stats ? rt_shade_kernel<true> : rt_shade_kernel<false>, sgrid, block, 0, s, a->dev, p, r.width, r.height, r.y0, r.y1, t.row_step,
                       n_rows, A.utab, A.vtab, (const HitRec*)c->hitbuf, r.dst, (HitRec*)r.hits, r.colors, r.counters, c->ctl, lpt_blocks, (const uint32_t*)L.cost,
                       L.order, n_tiles, A.per_shard >> 6, stats ? 1u : r.batch, stats ? (const ShadeParams*)nullptr : (const ShadeParams*)c->pbatch,
                       stats ? (uint64_t)0 : r.dst_frame_stride, base_order);
  }
  return hipGetLastError() == hipSuccess;
}

int render_common(vxrt_accel_t* a, const RenderRequest& r) {
  const int go = check_request(a, r);
  if (go <= 0) return go;
  uint32_t* st = status_word();
  if (!st) return -1;
  const ShadeParams p = shade_params(r.params[0]);
  const Tiles t = window_tiles(r);
  hipStream_t s = (hipStream_t)r.stream;
  FrameCtx* c = acquire_ctx(a, s);
  if (!c) return -1;
  // from here on a failure releases the context the way a success does: its event is recorded behind whatever was enqueued, the
  // context is marked busy on this stream and its control block is cleared before the next use
  auto fail = [&]() -> int { c->ctl_dirty = true; (void)release_ctx(a, c, s); return -1; };
  const bool lpt = lpt_wanted(a, r, (uint32_t)t.total);
  PersistArgs A{};
  A.status = st;
  if (!frame_resources(a, c, r, t, lpt, A, s)) return fail();
  const LaunchPlan plan = launch_plan(a, r, (uint32_t)t.total, lpt, r.cams ? 0u : a->ap_count * r.batch);
  if (!traverse_frame(a, c, r, plan, p, A, s)) return fail();
  // (the tile sort for the next frame rides in the shading launch; the AO / bounce tails have no such launch and skip it)
  const bool mirror = !r.path && mirror_frame(a, r.params[0]);   // (a path frame ignores max_depth)
  const bool lpt_sort = plan.lpt && !r.ao && !r.path && !mirror;
  if (plan.lpt && !lpt_sort) c->lpt[r.batch].valid = false;
  if (gi_fused_frame(r)) {
    // nothing follows: the pixels are written.  The control block stays as the launches left it; the context's next call clears it.
    if (hipGetLastError() != hipSuccess) return fail();
  } else if (r.ao) {
    if (render_ao_tail(a, c, r, p, A.utab, A.vtab) != 0) return fail();
  } else if (r.path) {
    if (render_path_tail(a, c, r, p, A.utab, A.vtab) != 0) return fail();
  } else if (mirror) {
    // reflective instances: the shading pass becomes the level-0 step of the mirror-bounce wavefront
    if (render_bounce_tail(a, c, r, p, A.utab, A.vtab) != 0) return fail();
  } else {
    if (!shade_frame(a, c, r, t, lpt_sort, p, A, s)) return fail();
    if (lpt_sort) c->lpt[r.batch].valid = true;
    c->ctl_dirty = false;
  }
  return release_ctx(a, c, s);
}

// A camera whose every field is finite (what the camera entry points accept, those of rt_denoise.hip too: rt_internal.h)
bool camera_ok(const vxrt_camera_t* c) {
  if (!c) return false;
  const float* f = &c->pos[0];
  for (int i = 0; i < 14; ++i) if (!std::isfinite(f[i])) return false;
  return true;
}

extern "C" {

const char* vxrt_version(void) { return "vortex-rt-mi355x 0.3 (gfx950, compact 64-byte nodes, persistent wavefronts)"; }

int vxrt_render(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                const vxrt_shade_params_t* params, int shadow, uint32_t* dst, vxrt_hit_t* hits,
                float* colors, unsigned long long* rays_traced, void* stream) {
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.shadow = shadow;
  r.dst = dst; r.hits = hits; r.colors = colors; r.counters = rays_traced; r.stream = stream;
  r.honours_alpha = true;
  return render_common(accel, r);
}

// Tile rows phase, phase + stride, phase + 2 stride, ... of the frame (8 rows each): what rank `phase` of `stride` ranks renders when one
// frame is split over GPUs (bench.py --gpus N; DCR 0x7F3 through the vx_* boundary).  Interleaving balances the ranks -- the
// cost of a tile varies 4x across the frame, mostly with height -- where contiguous bands do not.
int vxrt_render_interleaved(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t phase, uint32_t stride,
                            const vxrt_shade_params_t* params, int shadow, uint32_t* dst, vxrt_hit_t* hits,
                            float* colors, unsigned long long* rays_traced, void* stream) {
  if (stride == 0 || phase >= stride) return -1;
  if (accel && accel->alpha_on) return -1;        // (this form does not honour an alpha table: see check_request)
  if ((uint64_t)phase * 8u >= height) return 0;   // more ranks than tile rows: nothing for this one
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = phase * 8u; r.y1 = height; r.stride = stride; r.params = params; r.shadow = shadow;
  r.dst = dst; r.hits = hits; r.colors = colors; r.counters = rays_traced; r.stream = stream;
  return render_common(accel, r);
}

// n_frames frames of the same window in ONE set of launches: frame f is lit and shaded with params[f] and written to dst + f *
// dst_frame_stride.  One rank's share of a frame split N ways is a single round of tiles -- as long as its slowest tile, about half
// a full frame's time however small the share -- so a sequence of frames is traced side by side instead.
int vxrt_render_interleaved_batch(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t phase, uint32_t stride, uint32_t n_frames,
                                  const vxrt_shade_params_t* params, int shadow, uint32_t* dst, uint64_t dst_frame_stride,
                                  unsigned long long* rays_traced, void* stream) {
  if (stride == 0 || phase >= stride || n_frames == 0) return -1;
  if (accel && accel->alpha_on) return -1;
  if ((uint64_t)phase * 8u >= height) return 0;
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = phase * 8u; r.y1 = height; r.stride = stride; r.params = params; r.batch = n_frames; r.shadow = shadow;
  r.dst = dst; r.dst_frame_stride = dst_frame_stride; r.counters = rays_traced; r.stream = stream;
  return render_common(accel, r);
}

// n_frames frames of the row window [y0, y1) in one set of launches: what a rank renders when the frame is split into contiguous
// bands (bench.py --shard bands).  dst addresses each frame as a FULL frame does (pixel (x, y) of frame f at dst[f * dst_frame_stride
// + x + y * width]): only rows [y0, y1) are touched, so a caller that keeps just its band passes (band buffer - y0 * width) and a
// frame stride of (y1 - y0) * width.
int vxrt_render_rows_batch(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, uint32_t n_frames,
                           const vxrt_shade_params_t* params, int shadow, uint32_t* dst, uint64_t dst_frame_stride,
                           unsigned long long* rays_traced, void* stream) {
  if (n_frames == 0) return -1;
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.batch = n_frames; r.shadow = shadow;
  r.dst = dst; r.dst_frame_stride = dst_frame_stride; r.counters = rays_traced; r.stream = stream;
  return render_common(accel, r);
}

// diagnostic: vxrt_render_interleaved_batch's traversal launch with the per-wavefront log of vxrt_render_wave_log (counting build of the
// timed traversal; the pixels are NOT produced: the shading launch of this build knows single frames only)
int vxrt_render_interleaved_batch_wave_log(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t phase, uint32_t stride, uint32_t n_frames,
                                           const vxrt_shade_params_t* params, int shadow, uint32_t* dst, uint64_t dst_frame_stride,
                                           unsigned long long* counters, unsigned long long* wave_log, void* stream) {
  if (stride == 0 || phase >= stride || n_frames == 0 || !wave_log || !counters) return -1;
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = phase * 8u; r.y1 = height; r.stride = stride; r.params = params; r.batch = n_frames; r.shadow = shadow;
  r.dst = dst; r.dst_frame_stride = dst_frame_stride; r.counters = counters; r.wave_log = wave_log; r.stream = stream;
  r.counting = Counting::TIMED_TRAVERSAL;
  return render_common(accel, r);
}

// n_frames whole frames in one set of launches (vxrt_render_interleaved_batch with a single rank)
int vxrt_render_batch(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t n_frames, const vxrt_shade_params_t* params, int shadow,
                      uint32_t* dst, uint64_t dst_frame_stride, unsigned long long* rays_traced, void* stream) {
  return vxrt_render_interleaved_batch(accel, width, height, 0, 1, n_frames, params, shadow, dst, dst_frame_stride, rays_traced, stream);
}

// vxrt_render from a caller-supplied pinhole camera (see the header)
int vxrt_render_camera(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                       const vxrt_shade_params_t* params, int shadow, uint32_t* dst, vxrt_hit_t* hits, float* colors,
                       unsigned long long* rays_traced, void* stream) {
  if (!camera_ok(cam)) return -1;
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.shadow = shadow; r.cams = cam;
  r.dst = dst; r.hits = hits; r.colors = colors; r.counters = rays_traced; r.stream = stream;
  r.honours_alpha = true;
  return render_common(accel, r);
}

// vxrt_render_batch with cams[f] per frame (see the header)
int vxrt_render_batch_camera(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t n_frames, const vxrt_camera_t* cams,
                             const vxrt_shade_params_t* params, int shadow, uint32_t* dst, uint64_t dst_frame_stride,
                             unsigned long long* rays_traced, void* stream) {
  if (!cams || n_frames == 0 || n_frames > VXRT_MAX_BATCH) return -1;
  for (uint32_t f = 0; f < n_frames; ++f) if (!camera_ok(cams + f)) return -1;
  if (!accel || accel->stale || accel->alpha_on || !params || !dst) return -1;
  if (height == 0) return 0;   // (as vxrt_render_batch: no tile row to render)
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = 0; r.y1 = height; r.params = params; r.batch = n_frames; r.shadow = shadow; r.cams = cams;
  r.dst = dst; r.dst_frame_stride = dst_frame_stride; r.counters = rays_traced; r.stream = stream;
  return render_common(accel, r);
}

// Same launches as vxrt_render with the fetch counters compiled in (slower; never the timed path).
// counters: device u64[7] = rays, node fetches, instance fetches, triangle fetches, shaded hits,
// textured hits, pixels written -- the inputs of the algorithmic-bytes formula.
int vxrt_render_stats(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                      const vxrt_shade_params_t* params, int shadow, uint32_t* dst,
                      unsigned long long* counters, void* stream) {
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.shadow = shadow;
  r.dst = dst; r.counters = counters; r.stream = stream; r.counting = Counting::REFERENCE_ORDER;
  return render_common(accel, r);
}

// vxrt_render_stats for the traversal the TIMED kernel performs: occlusion rays of a frame visit children in slot order (the
// result is a boolean, the order cannot change it) and idle lanes test a leaf's second triangle, so node / triangle fetch
// counts differ from the reference-order counts of vxrt_render_stats; both are reported next to each other (bench.py)
int vxrt_render_stats_timed(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                            const vxrt_shade_params_t* params, int shadow, uint32_t* dst,
                            unsigned long long* counters, void* stream) {
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.shadow = shadow;
  r.dst = dst; r.counters = counters; r.stream = stream; r.counting = Counting::TIMED_TRAVERSAL;
  return render_common(accel, r);
}

// diagnostic: vxrt_render_stats that also logs, per wavefront of the main traversal launch, the first
// and last 100 MHz clock and the number of rays it started (wave_log: device u64[13 * waves], waves =
// 4 * blocks of the launch; 13 * 4 * 8 * 256 entries are always enough)
int vxrt_render_wave_log(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                         const vxrt_shade_params_t* params, int shadow, uint32_t* dst,
                         unsigned long long* counters, unsigned long long* wave_log, void* stream) {
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.shadow = shadow;
  r.dst = dst; r.counters = counters; r.wave_log = wave_log; r.stream = stream; r.counting = Counting::TIMED_TRAVERSAL;
  return render_common(accel, r);
}

int vxrt_render_diffuse_bounce(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                               const vxrt_shade_params_t* params, uint32_t seed, uint32_t* dst, float* colors,
                               unsigned long long* rays_traced, void* stream) {
  vxrt_ao_params_t gi{};
  gi.spp = 1; gi.radius = RT_LARGE_FLOAT; gi.seed = seed; gi.reserved = VXRT_AO_MODE_DIFFUSE_BOUNCE;
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.ao = &gi;
  r.dst = dst; r.colors = colors; r.counters = rays_traced; r.stream = stream;
  return render_common(accel, r);
}

int vxrt_render_ao(vxrt_accel_t* accel, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                   const vxrt_shade_params_t* params, const vxrt_ao_params_t* ao, uint32_t* dst, float* colors,
                   uint32_t* unoccluded, unsigned long long* rays_traced, void* stream) {
  if (!ao || ao->spp == 0 || ao->spp > 4096 || !(ao->radius > 0.0f) || ao->reserved != 0) return -1;
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.ao = ao;
  r.dst = dst; r.colors = colors; r.unoccluded = unoccluded; r.counters = rays_traced; r.stream = stream;
  return render_common(accel, r);
}

// vxrt_render_diffuse_bounce / vxrt_render_ao from a caller-supplied pinhole camera (see the header)
int vxrt_render_diffuse_bounce_camera(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                      const vxrt_shade_params_t* params, uint32_t seed, uint32_t* dst, float* colors,
                                      unsigned long long* rays_traced, void* stream) {
  if (!camera_ok(cam)) return -1;
  vxrt_ao_params_t gi{};
  gi.spp = 1; gi.radius = RT_LARGE_FLOAT; gi.seed = seed; gi.reserved = VXRT_AO_MODE_DIFFUSE_BOUNCE;
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.ao = &gi; r.cams = cam;
  r.dst = dst; r.colors = colors; r.counters = rays_traced; r.stream = stream;
  return render_common(accel, r);
}

int vxrt_render_ao_camera(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                          const vxrt_shade_params_t* params, const vxrt_ao_params_t* ao, uint32_t* dst, float* colors,
                          uint32_t* unoccluded, unsigned long long* rays_traced, void* stream) {
  if (!camera_ok(cam)) return -1;
  if (!ao || ao->spp == 0 || ao->spp > 4096 || !(ao->radius > 0.0f) || ao->reserved != 0) return -1;
  RenderRequest r;
  r.width = width; r.height = height; r.y0 = y0; r.y1 = y1; r.params = params; r.ao = ao; r.cams = cam;
  r.dst = dst; r.colors = colors; r.unoccluded = unoccluded; r.counters = rays_traced; r.stream = stream;
  return render_common(accel, r);
}

// vxrt_trace with the fetch counters compiled in (slower; never the timed path): counters = device u64[8],
// [0..3] = {rays, node fetches, instance fetches, triangle fetches}, the inputs of SURVEY s8d's per-ray formula
int vxrt_trace_stats(vxrt_accel_t* a, const float* rays, uint64_t n, const float* tmax,
                     vxrt_hit_t* hits, int mode, unsigned long long* counters, void* stream) {
  if (!a || a->stale || !counters || (n && (!rays || !hits))) return -1;
  if (a->alpha_on) return -1;   // (the counting build has no alpha-tested form)
  if (mode != VXRT_MODE_CLOSEST && mode != VXRT_MODE_ANY) return -1;
  if (n == 0) return 0;
  if (n > 0x7fffffffull) return -1;
  hipStream_t s = (hipStream_t)stream;
  FrameCtx* c = acquire_ctx(a, s);
  if (!c) return -1;
  // (a failure releases the context the way a success does: its event is recorded behind whatever was enqueued, see render_common)
  if (trace_on_ctx(a, c, rays, n, tmax, (HitRec*)hits, mode, s, nullptr, counters) != 0) { c->ctl_dirty = true; (void)release_ctx(a, c, s); return -1; }
  return release_ctx(a, c, s);
}

int vxrt_trace(vxrt_accel_t* a, const float* rays, uint64_t n, const float* tmax,
               vxrt_hit_t* hits, int mode, void* stream) {
  if (!a || a->stale || (n && (!rays || !hits))) return -1;
  if (mode != VXRT_MODE_CLOSEST && mode != VXRT_MODE_ANY) return -1;
  if (n == 0) return 0;
  if (n > 0x7fffffffull) return -1;
  hipStream_t s = (hipStream_t)stream;
  FrameCtx* c = acquire_ctx(a, s);
  if (!c) return -1;
  if (trace_on_ctx(a, c, rays, n, tmax, (HitRec*)hits, mode, s) != 0) { c->ctl_dirty = true; (void)release_ctx(a, c, s); return -1; }
  return release_ctx(a, c, s);
}

// Opt-in compatibility mode: the reference RTU's traversal restated literally, quirks included, on a flat memory image (see
// rt_quirks_trace_kernel).  image: device memory of image_size bytes; the four offsets are what the RTX DCRs 0x6..0x9 hold in the
// simulator (32-bit addresses into its RAM).  hits: n records; a miss has dist 1e30.  mode: VXRT_MODE_CLOSEST = the fixed point of
// the accept loop, VXRT_MODE_ANY = the first accepted candidate.
int vxrt_trace_reference_quirks(const void* image, uint64_t image_size, uint32_t tlas_off, uint32_t blas_off, uint32_t bvh_off, uint32_t tri_off,
                                const float* rays, uint64_t n, const float* tmax, vxrt_hit_t* hits, int mode, void* stream) {
  if (!image || image_size < 64 || (n && (!rays || !hits))) return -1;
  if (mode != VXRT_MODE_CLOSEST && mode != VXRT_MODE_ANY) return -1;
  if (n == 0) return 0;
  if (n > 0x7fffffffull) return -1;
  uint32_t* st = status_word();
  if (!st) return -1;
  QuirkImage im{(const uint8_t*)image, image_size, tlas_off, blas_off, bvh_off, tri_off};
  hipLaunchKernelGGL(rt_quirks_trace_kernel, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, im, rays, tmax, n, (HitRec*)hits,
                     mode == VXRT_MODE_ANY ? 1 : 0, st);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Camera rays of rows [y0, y1) of a W x H frame as a ray buffer (6 floats per ray, ray (x, y) at x + (y - y0) * W): what the frame
// kernels trace, for callers that trace them through vxrt_trace / vxrt_trace_reference_quirks and shade with vxrt_shade_rays.
int vxrt_camera_rays(uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, float* rays, void* stream) {
  if (!rays || width == 0 || height == 0 || y0 > y1 || y1 > height) return -1;
  const uint64_t n = (uint64_t)width * (y1 - y0);
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_camera_rays_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, width, height, y0, n, rays);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int vxrt_pinhole_rays(const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, float* rays, void* stream) {
  if (!camera_ok(cam) || !rays || width == 0 || height == 0 || y0 > y1 || y1 > height) return -1;
  const uint64_t n = (uint64_t)width * (y1 - y0);
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_pinhole_rays_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *cam, width, height, y0, n, rays);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int vxrt_shade_rays(vxrt_accel_t* a, const float* rays, const vxrt_hit_t* hits, uint64_t n, const vxrt_shade_params_t* params,
                    float* colors, uint32_t* rgb8, void* stream) {
  if (!a || a->stale || !params || (n && (!rays || !hits)) || (!colors && !rgb8)) return -1;
  if (!a->ref.triEx || !a->ref.mat || a->ref.n_mats == 0) return -1;
  if (n == 0) return 0;
  if (n > 0x7fffffffull) return -1;
  // a hit record names a triangle and an instance: both must exist (records a caller made up are not trusted)
  ShadeParams p = shade_params(*params);
  p.max_depth = 1;
  hipLaunchKernelGGL(rt_shade_rays_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->dev, p, n, rays, (const HitRec*)hits, colors, rgb8);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// diagnostic (tests): the control block of frame context `ctx` as the last call left it -- [0] deferral count, [32 + 32 k] the
// main launch's queue shard k, [32 + 256 + 32 k] the shards of the EXACT launch over the deferred list, [32 + 512 + 32 k] those of
// the a-priori EXACT launch.  vxrt_trace leaves the block for the next call to clear, so it can be inspected after a trace.
// diagnostic (tools/xcd_tail.py): from now on every main traversal launch on this layout -- the timed kernels included -- leaves, per wavefront,
// the constant 100 MHz clock at its end and its ray count | physical XCD << 56 in `log` (device memory, 2 u64 per wavefront, room for 8,192
// wavefronts: 16 x 8,192 u64; the caller zeroes it between the launches it wants to tell apart, and keeps it alive until they have run); nullptr
// switches it off again.  The EXACT launches do not write.  Costs the timed kernel one store per wavefront at its end.
int vxrt_wire_pack(const uint32_t* frames, uint64_t frame_stride, uint32_t width, uint32_t per, uint32_t world, uint32_t rank, uint32_t n_frames,
                   uint8_t* wire, void* stream) {
  if (!frames || !wire || width == 0 || (width & 3u) != 0 || per == 0 || world == 0 || rank >= world || n_frames == 0) return -1;
  if (((uintptr_t)frames & 15u) != 0 || ((uintptr_t)wire & 3u) != 0 || (frame_stride & 3u) != 0) return -1;   // (16-byte pixel quads, word stores)
  const uint64_t n = (uint64_t)n_frames * per * 8u * (width / 4u);
  if (n > 0xFFFFFFFFull * 256ull) return -1;
  hipLaunchKernelGGL(wire_pack_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frames, frame_stride, width / 4u, per, world, rank, n, (uint32_t*)wire);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int vxrt_wire_unpack(const uint8_t* wire_all, uint64_t wire_stride_bytes, uint32_t width, uint32_t per, uint32_t world, uint32_t n_frames,
                     uint32_t* frames, uint64_t frame_stride, void* stream) {
  if (!frames || !wire_all || width == 0 || (width & 3u) != 0 || per == 0 || world == 0 || n_frames == 0) return -1;
  if (((uintptr_t)frames & 15u) != 0 || ((uintptr_t)wire_all & 3u) != 0 || (frame_stride & 3u) != 0 || (wire_stride_bytes & 3u) != 0) return -1;
  const uint64_t per_rank = (uint64_t)n_frames * per * 8u * (width / 4u);
  if (wire_stride_bytes < per_rank * 12u) return -1;
  const uint64_t n = per_rank * world;
  if (n > 0xFFFFFFFFull * 256ull) return -1;
  hipLaunchKernelGGL(wire_unpack_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)wire_all, wire_stride_bytes / 4u, width / 4u, per, world,
                     per_rank, frames, frame_stride);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// diagnostic (tools/trace_phases.py): the counting build's ray-buffer launches (vxrt_trace_stats) keep vxrt_render_wave_log's 16 u64 per wavefront in
// `log` from now on (device memory, 16 x 8,192 u64; nullptr: off) -- loop iterations, runs of the node / leaf body and the lanes active in them
int vxrt_debug_trace_wave_log(vxrt_accel_t* a, unsigned long long* log) {
  if (!a) return -1;
  a->trace_wave_log = log;
  return 0;
}

int vxrt_debug_child_counts(unsigned long long* out, int reset, void* stream) {
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_child_counts), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    const unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_child_counts), zero, sizeof(zero)) != hipSuccess) return -1;
  }
  return 0;
}

int vxrt_debug_end_log(vxrt_accel_t* a, unsigned long long* log) {
  if (!a) return -1;
  a->end_log = log;   // (captured by the launches enqueued from now on; launches already enqueued keep what they were given)
  return 0;
}

int vxrt_debug_read_control(vxrt_accel_t* a, uint32_t ctx, uint32_t* out, uint32_t n_dwords, void* stream) {
  if (!a || !out || ctx >= MAX_FRAMES_IN_FLIGHT || n_dwords > CTL_DWORDS || !a->ctx[ctx].ctl) return -1;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  return hipMemcpy(out, a->ctx[ctx].ctl, (size_t)n_dwords * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

// diagnostic (tools/tile_tail.py): what frame context `ctx` learned for sets of `batch` frames -- cost[n] (loop iterations of the wavefront
// that traced the tile in the last launch; after a wave-log launch n start clocks, n durations in 100 MHz clocks and n steal distances
// follow) and the order[n] derived from it.  Returns the capacity in tiles, -1 on error.
int vxrt_debug_read_lpt(vxrt_accel_t* a, uint32_t ctx, uint32_t batch, uint32_t* cost, uint32_t cost_cap, uint32_t* order, uint32_t order_cap, void* stream) {
  if (!a || ctx >= MAX_FRAMES_IN_FLIGHT || batch > VXRT_MAX_BATCH) return -1;
  FrameCtx::Lpt& L = a->ctx[ctx].lpt[batch];
  if (!L.cost || !L.order) return -1;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  if (cost && hipMemcpy(cost, L.cost, (size_t)std::min<uint32_t>(cost_cap, 4u * L.cap) * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (order && hipMemcpy(order, L.order, (size_t)std::min(order_cap, L.cap) * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (int)L.cap;
}

// tests: the hint words (RT_SHADOW_HINTS) of the frame context that `stream` rendered a hinted shadow frame on last
static FrameCtx* hinted_ctx_of(vxrt_accel_t* a, hipStream_t s) {
  FrameCtx* pick = nullptr;
  // (a context whose words are void -- it rendered another frame since -- still shows them: the tests look whether they were touched)
  for (FrameCtx& c : a->ctx) if (c.hints && c.last_stream == s && (!pick || c.hint_seq > pick->hint_seq)) pick = &c;
  return pick;
}
int vxrt_debug_set_shadow_hints(vxrt_accel_t* a, void* stream, const uint32_t* hints, uint64_t n) {
  if (!a || !hints) return -1;
  FrameCtx* c = hinted_ctx_of(a, (hipStream_t)stream);
  if (!c || n > c->hints_cap) return -1;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  return hipMemcpy(c->hints, hints, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
int vxrt_debug_read_path_table(vxrt_accel_t* a, uint32_t* out, uint64_t n, void* stream) {
  if (!a || !out || !a->tri_path || n > a->ref.n_tris) return -1;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  return hipMemcpy(out, a->tri_path, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int vxrt_debug_shadow_hints_enable(int on) {
  g_shadow_hints_override.store(on < 0 ? -1 : (on ? 1 : 0));
  return 0;
}
int vxrt_debug_shadow_hint_counts(unsigned long long* out, int reset, void* stream) {
  if (!RT_SHADOW_HINT_COUNT) return -1;   // (the library does not count)
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hint_counts), 2 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    const unsigned long long zero[2] = {0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_hint_counts), zero, sizeof(zero)) != hipSuccess) return -1;
  }
  return 0;
}
int vxrt_debug_phase_counts(unsigned long long* out, int reset, void* stream) {
  if (!RT_PHASE_COUNT) return -1;   // (the library does not count)
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_counts), 6 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    const unsigned long long zero[6] = {0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_counts), zero, sizeof(zero)) != hipSuccess) return -1;
  }
  return 0;
}
int vxrt_debug_get_shadow_hints(vxrt_accel_t* a, void* stream, uint32_t* hints, uint64_t n) {
  if (!a || !hints) return -1;
  FrameCtx* c = hinted_ctx_of(a, (hipStream_t)stream);
  if (!c || n > c->hints_cap) return -1;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  return hipMemcpy(hints, c->hints, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

int vxrt_status(void* stream, uint32_t* status) {
  uint32_t* st = status_word();
  if (!st || !status) return -1;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  if (hipMemcpy(status, st, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  // read-and-clear: a failed run must not poison the runs after it (the word is per device, shared by all launches)
  if (*status != 0u && hipMemset(st, 0, sizeof(uint32_t)) != hipSuccess) return -1;
  return 0;
}

}  // extern "C"
