// Tails of two of the frames that trace secondary rays, and their kernels: what render_common (rt_kernels.hip) runs in place of the
// plain shading pass of a frame with reflective instances (the mirror-bounce wavefront) and of an ambient-occlusion frame, and the
// binning of secondary rays.  The third tail, that of a path frame, is rt_path.hip; the knob reader of all three is here.
// None of it is timed by bench.py, and none of it can
// reach the traversal kernel's unit: the seam is in rt_internal.h -- the ray buffers are traced through trace_on_ctx, buffers grow
// through grow_device -- and the shading arithmetic is that of the frame kernels, rt_shading.h.  Same build flags (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_internal.h"
#include "rt_shading.h"

__global__ void add_counter_kernel(unsigned long long* c, unsigned long long v) { if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(c, v); }

// ---------------------------------------------------------------------------------------------
// Mirror bounce (closest.cpp:95-121) as a wavefront over depth levels.  The reference recurses inside
// the closest-hit shader: C(ray) = term + (reflectivity > 0 && bounce + 1 < max_depth ? C(mirror ray)
// : background) * reflectivity, C(miss) = background.  Here level k holds the rays of bounce k (level 0 =
// the pixels); shading a level appends the next level's rays, and the colours are folded back from the
// deepest level to the pixels in the reference's order of operations, so the result has the same bits.
// Taken only when max_depth > 1 and some instance is reflective (the shipped scene builder has none).
// ---------------------------------------------------------------------------------------------
// Shade level `level`.  LEVEL0: entry = pixel of rows [y0,y1), hit record from the traversal (occlusion
// in bit 31 of blasIdx); else entry i = ray rays[6i..] with hit hits[i] (occluded iff shits[i] hit).
// Entries that bounce leave (term, reflectivity) in term[] and append a ray; the others are final.
// (CAM: camera frames -- utab / vtab are the head and the tables of the camera block, see CAM_HDR; only level 0 derives a primary ray)
template <bool LEVEL0, bool CAM>
__global__ __launch_bounds__(256) void rt_shade_bounce_kernel(SceneDev sc, ShadeParams p, uint32_t level, uint64_t n,
    uint32_t W, uint32_t H, uint32_t y0, const float* __restrict__ utab, const float* __restrict__ vtab,
    const HitRec* __restrict__ hb, const float* __restrict__ rays, const HitRec* __restrict__ shits,
    float4* __restrict__ term, float* __restrict__ col, uint32_t* __restrict__ dst, HitRec* __restrict__ hits_out,
    float* __restrict__ colors_out, uint32_t* next_count, float* __restrict__ next_rays, uint32_t* __restrict__ next_parent,
    uint32_t* __restrict__ ctl_reset) {
  if (ctl_reset && blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < CTL_DWORDS; i += 256u) ctl_reset[i] = 0u;
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  size_t e = (size_t)t;
  float ox, oy, oz, dx, dy, dz;
  HitRec h;
  bool occ;
  if (LEVEL0) {
    const uint32_t x = (uint32_t)(t % W), y = y0 + (uint32_t)(t / W);
    e = (size_t)x + (size_t)y * W;
    h = hb[hit_index(x, y - y0, (W + 7u) >> 3)];
    occ = (h.blasIdx & 0x80000000u) != 0u;
    if (hits_out) hits_out[e] = h;
    h.blasIdx &= 0x7fffffffu;
    frame_pixel_ray<CAM>(utab, vtab, W, H, 0u, x, y, ox, oy, oz, dx, dy, dz);
  } else {
    const float* rp = rays + e * 6;
    ox = rp[0]; oy = rp[1]; oz = rp[2]; dx = rp[3]; dy = rp[4]; dz = rp[5];
    h = hb[e];
    occ = shits != nullptr && shits[e].dist != RT_LARGE_FLOAT;
  }
  float r, g, b;
  bool final_ = true;
  if (h.dist == RT_LARGE_FLOAT) {   // miss.cpp:9-14
    r = p.bg[0]; g = p.bg[1]; b = p.bg[2];
  } else {
    float refl, Ix, Iy, Iz, Nx, Ny, Nz;
    shade_terms<false>(sc, p, ox, oy, oz, dx, dy, dz, h, occ, r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz);
    if (refl > 0.0f && level + 1u < p.max_depth) {   // :95
      final_ = false;
      term[e] = make_float4(r, g, b, refl);
      const uint32_t slot = atomicAdd(next_count, 1u);   // every level has room for one ray per entry of the level before
      mirror_ray(dx, dy, dz, Ix, Iy, Iz, Nx, Ny, Nz, next_rays + (size_t)slot * 6);
      next_parent[slot] = (uint32_t)e;
    } else {
      float thr = 1.0f;
      thr *= refl;                    // :90
      r = r + p.bg[0] * thr;          // :123
      g = g + p.bg[1] * thr;
      b = b + p.bg[2] * thr;
    }
  }
  if (final_) {
    if (LEVEL0) {
      dst[e] = pack_rgb8(r, g, b);
      if (colors_out) { colors_out[3 * e] = r; colors_out[3 * e + 1] = g; colors_out[3 * e + 2] = b; }
    } else {
      col[3 * e] = r; col[3 * e + 1] = g; col[3 * e + 2] = b;
    }
  }
}

// occlusion rays of a bounce level (shadow extension at every depth); a miss gets a ray nothing can hit
__global__ __launch_bounds__(256) void rt_bounce_shadow_rays_kernel(ShadeParams p, uint32_t n, const float* __restrict__ rays,
    const HitRec* __restrict__ hits, float* __restrict__ srays, float* __restrict__ stmax, unsigned long long* rays_traced) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool real = false;
  if (i < n) {
    const float* rp = rays + (size_t)i * 6;
    float* sp = srays + (size_t)i * 6;
    const float d = hits[i].dist;
    if (d == RT_LARGE_FLOAT) {
      sp[0] = 0.f; sp[1] = 0.f; sp[2] = 0.f; sp[3] = 1.f; sp[4] = 1.f; sp[5] = 1.f;
      stmax[i] = -1.0f;
    } else {
      float sdist;
      shadow_ray(p, rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], d, sp[0], sp[1], sp[2], sp[3], sp[4], sp[5], sdist);
      stmax[i] = sdist;
      real = true;
    }
  }
  const unsigned long long m = __ballot(real);
  if (rays_traced && (threadIdx.x & 63u) == 0u && m) atomicAdd(rays_traced, (unsigned long long)__popcll(m));
}

// fold level k into level k-1 (closest.cpp:117): C[parent] = term[parent] + C_k * (1 * reflectivity[parent])
template <bool TO_PIXELS>
__global__ __launch_bounds__(256) void rt_bounce_unwind_kernel(uint32_t n, const uint32_t* __restrict__ parent, const float* __restrict__ col_k,
    const float4* __restrict__ term_prev, float* __restrict__ col_prev, uint32_t* __restrict__ dst, float* __restrict__ colors_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const size_t q = parent[i];
  const float4 t = term_prev[q];
  float thr = 1.0f;
  thr *= t.w;
  const float r = t.x + col_k[3 * (size_t)i] * thr, g = t.y + col_k[3 * (size_t)i + 1] * thr, b = t.z + col_k[3 * (size_t)i + 2] * thr;
  if (TO_PIXELS) {
    dst[q] = pack_rgb8(r, g, b);
    if (colors_out) { colors_out[3 * q] = r; colors_out[3 * q + 1] = g; colors_out[3 * q + 2] = b; }
  } else {
    col_prev[3 * q] = r; col_prev[3 * q + 1] = g; col_prev[3 * q + 2] = b;
  }
}

// ---------------------------------------------------------------------------------------------
// Ambient occlusion (extension, BASELINE config 5; recipe defined in oracle/rt_oracle.c:orc_ao_ray and
// mirrored here operation by operation -- RNG of common.h:129-147, rejection-sampled disk, Duff basis:
// only IEEE add/mul/div/sqrt, so host and device produce the same rays).
// ---------------------------------------------------------------------------------------------
// per pixel of rows [y0,y1): Lambert colour of the primary hit (else arm of closest.cpp), hit point and
// shading normal for the occlusion rays; geo[t] = (I, hit?), nrm[t] = (N, 0), col[t] = (rgb, 0), cnt[t] = 0;
// pixels with a hit are appended to list[] (count in hdr[0]; the order is arbitrary, nothing depends on it)
// (CAM: camera frames -- utab / vtab are the camera block's head and tables, see CAM_HDR)
template <bool CAM>
__global__ __launch_bounds__(256) void rt_ao_prepare_kernel(SceneDev sc, ShadeParams p, uint64_t n, uint32_t W, uint32_t y0,
    const float* __restrict__ utab, const float* __restrict__ vtab, const HitRec* __restrict__ hb,
    float4* __restrict__ geo, float4* __restrict__ nrm, float4* __restrict__ col, uint32_t* __restrict__ cnt,
    uint32_t* __restrict__ list, uint32_t* hdr, uint32_t* ctl_reset, float4* __restrict__ alb /* optional: albedo of the hit */) {
  if (ctl_reset && blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < CTL_DWORDS; i += 256u) ctl_reset[i] = 0u;
  bool hit_c[PREP_CHUNKS];
  uint32_t t_c[PREP_CHUNKS];
#pragma unroll
  for (int c = 0; c < PREP_CHUNKS; ++c) {
    const uint64_t t = ((uint64_t)blockIdx.x * PREP_CHUNKS + c) * 256u + threadIdx.x;
    bool hit = false;
    if (t < n) {
      const uint32_t x = (uint32_t)(t % W), y = y0 + (uint32_t)(t / W);
      HitRec h = hb[hit_index(x, y - y0, (W + 7u) >> 3)];
      h.blasIdx &= 0x7fffffffu;
      float ox, oy, oz, dx, dy, dz;
      if constexpr (CAM) camera_ray(utab, vtab, W, x, y, ox, oy, oz, dx, dy, dz);
      else generate_ray(utab[x], vtab[y], ox, oy, oz, dx, dy, dz);
      float r, g, b;
      if (h.dist == RT_LARGE_FLOAT) {
        r = p.bg[0]; g = p.bg[1]; b = p.bg[2];
        geo[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        nrm[t] = make_float4(0.f, 0.f, 1.f, 0.f);
      } else {
        float refl, Ix, Iy, Iz, Nx, Ny, Nz, a3[3];
        shade_terms<false>(sc, p, ox, oy, oz, dx, dy, dz, h, false, r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz, nullptr, a3);
        float thr = 1.0f;
        thr *= refl;
        r = r + p.bg[0] * thr; g = g + p.bg[1] * thr; b = b + p.bg[2] * thr;
        geo[t] = make_float4(Ix, Iy, Iz, 1.0f);
        nrm[t] = make_float4(Nx, Ny, Nz, 0.f);
        if (alb) alb[t] = make_float4(a3[0], a3[1], a3[2], 0.f);
        hit = true;
      }
      col[t] = make_float4(r, g, b, 0.f);
      cnt[t] = 0u;
    }
    hit_c[c] = hit; t_c[c] = (uint32_t)t;
  }
  wg_append<PREP_CHUNKS>(hit_c, t_c, list, hdr);
}

// samples [s0, s0 + ns) of every listed pixel: ray i = (pixel list[i / ns], sample s0 + i % ns); hdr[1] = number of rays
template <bool CAM>
__global__ __launch_bounds__(256) void rt_ao_rays_kernel(uint64_t cap, uint32_t W, uint32_t y0, const float* __restrict__ utab, const float* __restrict__ vtab,
    const float4* __restrict__ geo, const float4* __restrict__ nrm, const uint32_t* __restrict__ list, uint32_t* hdr,
    uint32_t spp, uint32_t s0, uint32_t ns, uint32_t user_seed, float radius, float* __restrict__ rays, float* __restrict__ tmax) {
  const uint64_t total = (uint64_t)hdr[0] * ns;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i == 0) hdr[1] = (uint32_t)total;
  if (i >= total || i >= cap) return;
  const uint32_t t = list[i / ns], smp = s0 + (uint32_t)(i % ns);
  float* o = rays + (size_t)i * 6;
  const float4 gI = geo[t];
  const uint32_t x = t % W, y = y0 + t / W;
  float ox, oy, oz, vdx, vdy, vdz;
  if constexpr (CAM) camera_ray(utab, vtab, W, x, y, ox, oy, oz, vdx, vdy, vdz);
  else generate_ray(utab[x], vtab[y], ox, oy, oz, vdx, vdy, vdz);
  const float4 gN = nrm[t];
  float r6[6];
  ao_sample_ray(x, y, W, spp, smp, user_seed, gI.x, gI.y, gI.z, gN.x, gN.y, gN.z, vdx, vdy, vdz, r6);
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = r6[k];
  tmax[i] = radius;
}

__global__ __launch_bounds__(256) void rt_ao_accumulate_kernel(uint64_t cap, const uint32_t* __restrict__ list, const uint32_t* __restrict__ hdr, uint32_t ns,
    const HitRec* __restrict__ ohits, uint32_t* __restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const bool live = i < hdr[1] && i < cap;
  // the ns samples of a pixel sit next to each other: the lanes of a wavefront that belong to one pixel add up with a ballot and
  // the first of them does the pixel's atomic (16 spp: 4 atomics per wavefront instead of up to 64)
  const unsigned long long m = __ballot(live && ohits[live ? i : 0].dist == RT_LARGE_FLOAT);
  if (!live) return;
  const uint32_t lane = threadIdx.x & 63u, k = (uint32_t)(i % ns);
  const uint32_t s0 = lane > k ? lane - k : 0u, e0 = min(63u, lane - k + ns - 1u);   // lanes of this pixel in this wavefront (lane - k may wrap: then s0 = 0)
  const uint32_t e = lane >= k ? e0 : min(63u, lane + (ns - 1u - k));
  if (lane == s0) {
    const unsigned long long seg = (~0ull >> (63u - e)) & (~0ull << s0);
    const uint32_t c = (uint32_t)__popcll(m & seg);
    if (c) atomicAdd(cnt + list[i / ns], c);
  }
}

__global__ __launch_bounds__(256) void rt_ao_final_kernel(uint64_t n, uint32_t W, uint32_t y0, const float4* __restrict__ geo, const float4* __restrict__ col,
    const uint32_t* __restrict__ cnt, uint32_t spp, uint32_t* __restrict__ dst, float* __restrict__ colors_out, uint32_t* __restrict__ unoccluded,
    unsigned long long* rays_traced) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  bool hit = false;
  if (t < n) {
    const uint32_t x = (uint32_t)(t % W), y = y0 + (uint32_t)(t / W);
    const size_t e = (size_t)x + (size_t)y * W;
    const float4 c = col[t];
    float r = c.x, g = c.y, b = c.z;
    uint32_t open = 0u;
    if (geo[t].w != 0.f) {
      hit = true;
      open = cnt[t];
      const float f = (float)open / (float)spp;
      r *= f; g *= f; b *= f;
    }
    dst[e] = pack_rgb8(r, g, b);
    if (colors_out) { colors_out[3 * e] = r; colors_out[3 * e + 1] = g; colors_out[3 * e + 2] = b; }
    if (unoccluded) unoccluded[e] = open;
  }
  const unsigned long long m = __ballot(hit);
  if (rays_traced && (threadIdx.x & 63u) == 0u && m) atomicAdd(rays_traced, (unsigned long long)__popcll(m) * spp);
}

// ---------------------------------------------------------------------------------------------
// Secondary rays re-sorted before they are traced (north_star: "ray packets re-sorted ... to tame divergence").
// The rays of a bounce / AO pass leave the compaction in pixel order with directions spread over a hemisphere: a wavefront of
// 64 consecutive rays shares origins but not directions.  Counting sort by key = direction octant x origin cell (the 16x16-pixel
// cell of the ray's pixel: hit points of neighbouring pixels are neighbours in space), so that 64 consecutive queue positions
// hold rays that start in one small region AND point into the same octant.  Only the ORDER in which rays are traced changes:
// the kernel reads ray order[q] and writes hit record order[q], so every result is bit-identical.
// Only the ambient-occlusion tail calls the sort today (render_ao_tail, per batch of samples): the one diffuse bounce it was also
// measured on has since become a single persistent launch without a ray buffer.  It is off by default (VXRT_SORT_SECONDARY=1 turns it
// on); tests/test_gpu_variants.py::test_secondary_ray_sort_stays_bit_equal runs the AO tests with it in child processes -- frames whose
// scan takes one, two and three counters per thread among them, and frames whose batches are sorted one by one.
// ---------------------------------------------------------------------------------------------
#define BIN_CELL_SHIFT 4u   // 16 x 16 pixels
__global__ __launch_bounds__(256) void rt_bin_count_kernel(uint64_t cap, const uint32_t* __restrict__ hdr, const float* __restrict__ rays,
    const uint32_t* __restrict__ list, uint32_t ns, uint32_t W, uint32_t cells_x, uint32_t n_cells, uint32_t* __restrict__ hist, uint32_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= hdr[1] || i >= cap) return;
  const uint32_t t = list[i / ns];
  const uint32_t cell = ((t / W) >> BIN_CELL_SHIFT) * cells_x + ((t % W) >> BIN_CELL_SHIFT);
  const float* r = rays + i * 6;
  const uint32_t oct = (__float_as_uint(r[3]) >> 31) | ((__float_as_uint(r[4]) >> 31) << 1) | ((__float_as_uint(r[5]) >> 31) << 2);
  const uint32_t key = oct * n_cells + cell;
  keys[i] = key;
  atomicAdd(&hist[key], 1u);
}
// exclusive scan of hist[0..n) in place, one workgroup of 1024 threads, `per` consecutive counters per thread
__global__ __launch_bounds__(1024) void rt_bin_scan_kernel(uint32_t* __restrict__ hist, uint32_t n, uint32_t per) {
  __shared__ uint32_t wsum[16];
  const uint32_t lo = threadIdx.x * per, hi = min(lo + per, n);
  uint32_t sum = 0;
  for (uint32_t k = lo; k < hi; ++k) sum += hist[k];
  uint32_t inc = sum;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += y; }
  if (lane == 63u) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = inc - sum;
  for (uint32_t w = 0; w < wave; ++w) base += wsum[w];
  for (uint32_t k = lo; k < hi; ++k) { const uint32_t v = hist[k]; hist[k] = base; base += v; }
}
__global__ __launch_bounds__(256) void rt_bin_scatter_kernel(uint64_t cap, const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ hist, uint32_t* __restrict__ order) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= hdr[1] || i >= cap) return;
  order[atomicAdd(&hist[keys[i]], 1u)] = (uint32_t)i;
}

// ---------------------------------------------------------------------------------------------
// host: the two tails render_common (rt_kernels.hip) ends such a frame with
// ---------------------------------------------------------------------------------------------
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#define AO_BATCH_RAYS (32ull << 20)   // rays per batch of an ambient-occlusion frame

// The three measurement knobs of the secondary tails (SecondaryKnobs, rt_internal.h; docs/KNOBS.md), read from the environment once per
// process, together: on the first call, from this unit or from rt_path.hip, that asks for one.  Each keeps the parsing it always had.
// With VXRT_DEBUG set, the values read go to stderr in one line, so that a test that runs a child process with a knob can see that the
// child took it.
const SecondaryKnobs& secondary_knobs() {
  static const SecondaryKnobs knobs = [] {
    SecondaryKnobs k;
    { const char* e = getenv("VXRT_PATH_BATCH"); const long long v = e ? atoll(e) : 0; k.path_batch = v > 0 ? (uint64_t)v : PATH_BATCH_PATHS; }
    { const char* e = getenv("VXRT_AO_BATCH"); const long long v = e ? atoll(e) : 0; k.ao_batch = v > 0 ? (uint64_t)v : AO_BATCH_RAYS; }
    { const char* e = getenv("VXRT_SORT_SECONDARY"); k.sort_secondary = e && e[0] == '1'; }
    if (getenv("VXRT_DEBUG"))
      fprintf(stderr, "[vxrt] secondary knobs: path_batch=%llu ao_batch=%llu sort_secondary=%d\n", (unsigned long long)k.path_batch,
              (unsigned long long)k.ao_batch, k.sort_secondary ? 1 : 0);
    return k;
  }();
  return knobs;
}

// The buffers of a bounce level for n entries: the terms; unless only_term the rays, hit records, parents and colours; with `shadow`
// the occlusion rays, which a level gets at the first frame with the shadow extension.  Each group has its own capacity.  (No wait
// of its own: hipFree orders itself behind the device, and the tail has waited for the level before.)
static bool level_reserve(FrameCtx::Level& l, uint64_t n, bool shadow, bool only_term) {
  if (!grow_device({{(void**)&l.term, 16}}, &l.cap, n, GrowSync::NONE, nullptr)) return false;
  if (only_term) return true;
  if (!grow_device({{(void**)&l.rays, 24}, {(void**)&l.hits, sizeof(HitRec)}, {(void**)&l.parent, 4}, {(void**)&l.col, 12}}, &l.ray_cap, n, GrowSync::NONE, nullptr)) return false;
  return !shadow || grow_device({{(void**)&l.srays, 24}, {(void**)&l.stmax, 4}, {(void**)&l.shits, sizeof(HitRec)}}, &l.shadow_cap, n, GrowSync::NONE, nullptr);
}

// Tail of a frame with reflective instances (replaces the plain shading pass): shade level 0, then per
// bounce level trace -> (occlusion rays ->) shade, then fold the colours back.  The level sizes come back
// to the host between levels, so this path synchronises the stream (it is not the benchmarked one).
// (utab / vtab: the tables the traversal used; a camera frame's utab is its camera block)
int render_bounce_tail(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const ShadeParams& p, const float* utab, const float* vtab) {
  const SceneDev& sc = a->dev;
  const uint32_t width = r.width, y0 = r.y0, y1 = r.y1;
  const bool shadow = r.shadow != 0;
  uint32_t* dst = r.dst; float* colors = r.colors;
  unsigned long long* rays_traced = r.counters;
  hipStream_t s = (hipStream_t)r.stream;
  const uint64_t npix = (uint64_t)width * (y1 - y0);          // entries of level 0 (addressed by pixel index)
  const uint64_t pix_span = (uint64_t)width * y1;              // term[] of level 0 is indexed by x + y*W
  if (npix > 0x7fffffffull) return -1;
  if (!c->bcount && hipMalloc((void**)&c->bcount, sizeof(uint32_t)) != hipSuccess) return -1;
  if (c->lv.size() < 2) c->lv.resize(2);
  if (!level_reserve(c->lv[0], pix_span, false, true)) return -1;
  if (!level_reserve(c->lv[1], npix, shadow, false)) return -1;
  dim3 block(256);
  if (hipMemsetAsync(c->bcount, 0, sizeof(uint32_t), s) != hipSuccess) return -1;
  const auto k_level0 = r.cams ? rt_shade_bounce_kernel<true, true> : rt_shade_bounce_kernel<true, false>;
  const auto k_deeper = rt_shade_bounce_kernel<false, false>;   // (the deeper levels hold ray buffers, whatever the camera)
  hipLaunchKernelGGL(k_level0, dim3((uint32_t)((npix + 255) / 256)), block, 0, s, sc, p, 0u, npix, width, r.height, y0, utab, vtab,
                     (const HitRec*)c->hitbuf, (const float*)nullptr, (const HitRec*)nullptr, c->lv[0].term, (float*)nullptr, dst, (HitRec*)r.hits, colors,
                     c->bcount, c->lv[1].rays, c->lv[1].parent, c->ctl);
  if (hipGetLastError() != hipSuccess) return -1;
  c->ctl_dirty = false;
  uint32_t depth = 0;   // deepest level that holds rays
  for (uint32_t k = 1; k < p.max_depth; ++k) {
    uint32_t n = 0;
    if (hipMemcpyAsync(&n, c->bcount, sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
    if (hipStreamSynchronize(s) != hipSuccess) return -1;
    if (n == 0) break;
    FrameCtx::Level& L = c->lv[k];
    L.n = n;
    depth = k;
    if (rays_traced) hipLaunchKernelGGL(add_counter_kernel, dim3(1), dim3(64), 0, s, rays_traced, (unsigned long long)n);
    if (trace_on_ctx(a, c, L.rays, n, nullptr, L.hits, VXRT_MODE_CLOSEST, s) != 0) return -1;
    const dim3 grid((n + 255u) / 256u);
    if (shadow) {
      hipLaunchKernelGGL(rt_bounce_shadow_rays_kernel, grid, block, 0, s, p, n, (const float*)L.rays, (const HitRec*)L.hits, L.srays, L.stmax, rays_traced);
      if (trace_on_ctx(a, c, L.srays, n, L.stmax, L.shits, MODE_ANY_UNORDERED, s) != 0) return -1;
    }
    if (c->lv.size() < (size_t)k + 2) c->lv.resize((size_t)k + 2);
    FrameCtx::Level& Nx = c->lv[k + 1];
    const bool more = k + 1 < p.max_depth;
    if (more && !level_reserve(Nx, n, shadow, false)) return -1;
    FrameCtx::Level& Lk = c->lv[k];   // (resize may have moved the vector)
    if (hipMemsetAsync(c->bcount, 0, sizeof(uint32_t), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_deeper, grid, block, 0, s, sc, p, k, (uint64_t)n, width, r.height, y0, utab, vtab,
                       (const HitRec*)Lk.hits, (const float*)Lk.rays, shadow ? (const HitRec*)Lk.shits : (const HitRec*)nullptr, Lk.term, Lk.col,
                       (uint32_t*)nullptr, (HitRec*)nullptr, (float*)nullptr, c->bcount, more ? Nx.rays : (float*)nullptr, more ? Nx.parent : (uint32_t*)nullptr,
                       (uint32_t*)nullptr);
    if (hipGetLastError() != hipSuccess) return -1;
    if (!more) break;
  }
  for (uint32_t k = depth; k >= 1; --k) {
    FrameCtx::Level& L = c->lv[k];
    const dim3 grid((L.n + 255u) / 256u);
    if (k == 1) hipLaunchKernelGGL(rt_bounce_unwind_kernel<true>, grid, block, 0, s, L.n, (const uint32_t*)L.parent, (const float*)L.col, (const float4*)c->lv[0].term, (float*)nullptr, dst, colors);
    else        hipLaunchKernelGGL(rt_bounce_unwind_kernel<false>, grid, block, 0, s, L.n, (const uint32_t*)L.parent, (const float*)L.col, (const float4*)c->lv[k - 1].term, c->lv[k - 1].col, (uint32_t*)nullptr, (float*)nullptr);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Tail of an ambient-occlusion frame (replaces the plain shading pass): the pixels with a hit are listed on
// the device, their occlusion rays are generated in batches of whole samples (<= AO_BATCH_RAYS rays, or VXRT_AO_BATCH) and each
// batch is one any-hit launch whose job count stays in device memory.  No host synchronisation unless a buffer grows.
int render_ao_tail(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const ShadeParams& p, const float* utab, const float* vtab) {
  const SceneDev& sc = a->dev;
  const vxrt_ao_params_t* ao = r.ao;
  const uint32_t width = r.width, y0 = r.y0, y1 = r.y1;
  hipStream_t s = (hipStream_t)r.stream;
  const uint64_t n = (uint64_t)width * (y1 - y0);
  if (ao->reserved == VXRT_AO_MODE_DIFFUSE_BOUNCE) return -1;    // (the diffuse-bounce frame is JOB_RENDER_GI: it has no tail)
  if (n > 0x7fffffffull || ao->spp == 0) return -1;
  uint32_t ns = (uint32_t)std::min<uint64_t>(ao->spp, std::max<uint64_t>(1, secondary_knobs().ao_batch / n));   // samples per batch
  const uint64_t ray_cap = n * ns;
  if (ray_cap > 0x7fffffffull) return -1;
  if (!c->ao_hdr && hipMalloc((void**)&c->ao_hdr, 8) != hipSuccess) return -1;
  if (!grow_device({{(void**)&c->ao_geo, 16}, {(void**)&c->ao_nrm, 16}, {(void**)&c->ao_col, 16}, {(void**)&c->ao_cnt, 4}, {(void**)&c->ao_list, 4}},
                   &c->ao_cap, n, GrowSync::STREAM, s)) return -1;
  if (!grow_device({{(void**)&c->ao_rays, 24}, {(void**)&c->ao_tmax, 4}, {(void**)&c->ao_hits, sizeof(HitRec)}}, &c->ao_ray_cap, ray_cap, GrowSync::STREAM, s)) return -1;
  const dim3 block(256), grid((uint32_t)((n + 255) / 256)), rgrid((uint32_t)((ray_cap + 255) / 256));
  const bool sort_on = secondary_knobs().sort_secondary;
  const uint32_t cells_x = (width + (1u << BIN_CELL_SHIFT) - 1) >> BIN_CELL_SHIFT, cells_y = (y1 - y0 + (1u << BIN_CELL_SHIFT) - 1) >> BIN_CELL_SHIFT;
  const uint32_t n_cells = cells_x * cells_y, n_bins = 8u * n_cells;
  if (sort_on && !(grow_device({{(void**)&c->bin_hist, 4}}, &c->bin_cap, n_bins, GrowSync::STREAM, s) &&
                   grow_device({{(void**)&c->bin_keys, 4}, {(void**)&c->bin_order, 4}}, &c->bin_ray_cap, ray_cap, GrowSync::STREAM, s))) return -1;
  auto bin_rays = [&](uint32_t ns_batch) -> const uint32_t* {   // ao_rays of the current batch -> bin_order
    if (!sort_on) return nullptr;
    if (hipMemsetAsync(c->bin_hist, 0, (size_t)n_bins * 4, s) != hipSuccess) return nullptr;
    hipLaunchKernelGGL(rt_bin_count_kernel, rgrid, block, 0, s, ray_cap, (const uint32_t*)c->ao_hdr, (const float*)c->ao_rays, (const uint32_t*)c->ao_list, ns_batch,
                       width, cells_x, n_cells, c->bin_hist, c->bin_keys);
    hipLaunchKernelGGL(rt_bin_scan_kernel, dim3(1), dim3(1024), 0, s, c->bin_hist, n_bins, (n_bins + 1023u) / 1024u);
    hipLaunchKernelGGL(rt_bin_scatter_kernel, rgrid, block, 0, s, ray_cap, (const uint32_t*)c->ao_hdr, (const uint32_t*)c->bin_keys, c->bin_hist, c->bin_order);
    return c->bin_order;
  };
  if (hipMemsetAsync(c->ao_hdr, 0, 8, s) != hipSuccess) return -1;
  const dim3 pgrid((uint32_t)((n + 256u * PREP_CHUNKS - 1u) / (256u * PREP_CHUNKS)));
  // (the two passes that derive the primary ray again: the camera forms for a camera frame)
  hipLaunchKernelGGL(r.cams ? rt_ao_prepare_kernel<true> : rt_ao_prepare_kernel<false>, pgrid, block, 0, s, sc, p, n, width, y0, utab, vtab, (const HitRec*)c->hitbuf,
                     c->ao_geo, c->ao_nrm, c->ao_col, c->ao_cnt, c->ao_list, c->ao_hdr, c->ctl, (float4*)nullptr);
  if (hipGetLastError() != hipSuccess) return -1;
  c->ctl_dirty = false;
  for (uint32_t s0 = 0; s0 < ao->spp; s0 += ns) {
    const uint32_t k = std::min(ns, ao->spp - s0);
    hipLaunchKernelGGL(r.cams ? rt_ao_rays_kernel<true> : rt_ao_rays_kernel<false>, rgrid, block, 0, s, ray_cap, width, y0, utab, vtab, (const float4*)c->ao_geo,
                       (const float4*)c->ao_nrm, (const uint32_t*)c->ao_list, c->ao_hdr, ao->spp, s0, k, ao->seed, ao->radius, c->ao_rays, c->ao_tmax);
    if (trace_on_ctx(a, c, c->ao_rays, n * k, c->ao_tmax, c->ao_hits, MODE_ANY_UNORDERED, s, c->ao_hdr + 1, nullptr, bin_rays(k)) != 0) return -1;
    hipLaunchKernelGGL(rt_ao_accumulate_kernel, rgrid, block, 0, s, ray_cap, (const uint32_t*)c->ao_list, (const uint32_t*)c->ao_hdr, k,
                       (const HitRec*)c->ao_hits, c->ao_cnt);
  }
  hipLaunchKernelGGL(rt_ao_final_kernel, grid, block, 0, s, n, width, y0, (const float4*)c->ao_geo, (const float4*)c->ao_col, (const uint32_t*)c->ao_cnt,
                     ao->spp, r.dst, r.colors, r.unoccluded, r.counters);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
