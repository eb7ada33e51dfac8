// Tail of a path frame, and its kernels: what render_common (rt_kernels.hip) runs in place of the plain shading pass of
// vxrt_render_path and the entry points built on it.  In this order:
//   - the previous-position guide of frames with motion (motion_guide, vxrt_previous_positions);
//   - the prepare launch and its flavours (camera, motion, emissive);
//   - the kernels of a batch: start, bounce rays (with the emitter ray of emitter sampling), occlusion rays, scatter, accumulate, final;
//   - the same for a sample count per pixel (counts, scan, start, bounce rays, accumulate, divide), and vxrt_sample_counts;
//   - host: the form of the request (path_form), the prepare launch, the depths of one batch, the end of the frame, the two tails
//     (uniform, per-pixel counts);
//   - host: the path API -- render_path_frame, the one builder of a path request, the vxrt_render_path* entry points that go through
//     it, and the single-launch calls (vxrt_specular_pick, vxrt_roulette, vxrt_emitter_rays[_mis], vxrt_emitter_hit_weights, vxrt_sample_counts).
// A denoised frame ends in rt_denoise.hip.  None of it is timed by bench.py, and none of it can reach the traversal kernel's unit: the
// seam is in rt_internal.h, as for rt_secondary.hip, which holds the knob reader (secondary_knobs).  Same build flags (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rt_internal.h"
#include "rt_shading.h"
#include "rt_env.h"

// ---------------------------------------------------------------------------------------------
// Path frames (vxrt_render_path; the definition is in include/vortex_hip.h, the launch sequence in render_path_tail and DESIGN.md s2,
// "Path frames").  The kernels around the ray-buffer launches: per-pixel state of the primary hit, per-path state that survives from
// bounce to bounce, the scatter step and the accumulation over samples.  Every arithmetic step is an existing __device__ function
// (shade_terms, ao_sample_ray, shadow_ray, pack_rgb8, camera_ray / generate_ray).
// Path slot i of a batch of ns samples starting at s0 = (pixel list[i / ns], sample s0 + i % ns); a path's state stays in its slot,
// and the rays of a depth are those of the slots still listed as live (ray q belongs to slot live[q]).
// ---------------------------------------------------------------------------------------------
// per pixel t of rows [y0,y1): geo[t] = (I, hit?), nrm[t] = (N, 0), dir[t] = (direction of the primary ray, 0), lit[t] = (Lit of the
// primary hit with the occlusion bit the shadow frame launch left in its record | background, 0), alb[t] = (Alb, 0); pixels with a hit
// are appended to list[] (count in hdr[0])
// (CAM: camera frames -- utab / vtab are the camera block's head and tables, see CAM_HDR)
// The previous-position guide of hit record h (the header's "Motion", operation for operation): where the surface point under h was
// when the accel's snapshot was taken, Q4 = (Q, 1), and the shading normal it had there, N'4 = (N', 0).  All zeros for a miss and for
// a record that names an instance or a triangle the scene does not have (nothing is read for it).  h.blasIdx: bit 31 is masked here.
__device__ __forceinline__ void motion_guide(const SceneDev& sc, const MotionSrc& m, const HitRec& h, float4& Q4, float4& N4) {
  Q4 = make_float4(0.f, 0.f, 0.f, 0.f); N4 = Q4;
  const uint32_t bi = h.blasIdx & 0x7fffffffu;
  if (h.dist == RT_LARGE_FLOAT || bi >= m.n_blas || h.triIdx >= m.n_tris) return;
  const float* v = m.tri + (size_t)h.triIdx * (RT_TRI_BYTES / 4);        // tri_t: v0, v1, v2
  const uint32_t* bp = m.blas + (size_t)bi * (RT_BLAS_STRIDE / 4);       // invTransform @ word 1, transform @ word 17
  float o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (v[3 + c] * h.bx + v[6 + c] * h.by) + v[c] * h.bz;
  float q[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t* r = bp + 17 + 4 * c;
    q[c] = ((__uint_as_float(r[0]) * o[0] + __uint_as_float(r[1]) * o[1]) + __uint_as_float(r[2]) * o[2]) + __uint_as_float(r[3]);
  }
  // shade_terms' shading normal with the snapshot's invTransform
  const rt_triex_t te = sc.triEx[h.triIdx];
  const float Nx = te.N1[0] * h.bx + te.N2[0] * h.by + te.N0[0] * h.bz;
  const float Ny = te.N1[1] * h.bx + te.N2[1] * h.by + te.N0[1] * h.bz;
  const float Nz = te.N1[2] * h.bx + te.N2[2] * h.by + te.N0[2] * h.bz;
  const float m0 = __uint_as_float(bp[1]), m1 = __uint_as_float(bp[2]), m2 = __uint_as_float(bp[3]);
  const float m4 = __uint_as_float(bp[5]), m5 = __uint_as_float(bp[6]), m6 = __uint_as_float(bp[7]);
  const float m8 = __uint_as_float(bp[9]), m9 = __uint_as_float(bp[10]), m10 = __uint_as_float(bp[11]);
  const float z0 = 0.0f * 0.0f;
  const float Tx = m0 * Nx + m4 * Ny + m8 * Nz + z0;
  const float Ty = m1 * Nx + m5 * Ny + m9 * Nz + z0;
  const float Tz = m2 * Nx + m6 * Ny + m10 * Nz + z0;
  const float inv = 1.0f / sqrtf(Tx * Tx + Ty * Ty + Tz * Tz);
  Q4 = make_float4(q[0], q[1], q[2], 1.0f);
  N4 = make_float4(Tx * inv, Ty * inv, Tz * inv, 0.f);
}

// vxrt_previous_positions: the guide of n hit records, one per thread
__global__ __launch_bounds__(256) void rt_previous_positions_kernel(SceneDev sc, MotionSrc m, uint32_t n, const HitRec* __restrict__ hits,
    float4* __restrict__ pos, float4* __restrict__ nrm) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  float4 Q4, N4;
  motion_guide(sc, m, hits[t], Q4, N4);
  pos[t] = Q4; nrm[t] = N4;
}

// what the MOTION flavour of rt_path_prepare_kernel takes besides: the guide's sources, its two per-pixel buffers of the frame context
// and the caller's optional prev_position (frame addressing)
struct PrepMotion { MotionSrc src; float4* pos; float4* nrm; float* out; };
struct PrepNoMotion {};

// Emi(h) of the header's "Emissive geometry": emissive * scale of the material of triangle triIdx, if it has a positive component
// (false: the material does not emit, and nothing is to be added)
__device__ __forceinline__ bool emission(const SceneDev& sc, uint32_t triIdx, float scale, float (&e3)[3]) {
  const rt_material_t* mat = sc.mat + sc.triEx[triIdx].texId;
  const float r = mat->emissive[0], g = mat->emissive[1], b = mat->emissive[2];
  if (!(r > 0.0f || g > 0.0f || b > 0.0f)) return false;
  e3[0] = r * scale; e3[1] = g * scale; e3[2] = b * scale;
  return true;
}

// what the emissive flavour of the prepare launch takes besides (EMI: lit[t] = Lit_0 + Emi(h_0))
struct PrepEmi { float scale; };
struct PrepNoEmi {};
// ... and the flavour lit by an environment map (ENV: a miss pixel's lit[t] = Env(dir(r_0)) in place of the background)
struct PrepNoEnv {};

// The header's "Specular vertices": a vertex of reflectivity rho is specular iff rho > 0 and rho is finite
__device__ __forceinline__ bool specular_vertex(float rho) { return rho > 0.0f && isfinite(rho); }

// The lobe pick of that section at a continuing vertex of reflectivity rho, from hash output `seed` (0 becomes 1; one xorshift step):
// true = mirror.  A vertex that is not specular takes no draw.
__device__ __forceinline__ bool specular_pick(float rho, uint32_t seed) {
  if (!specular_vertex(rho)) return false;
  if (seed == 0u) seed = 1u;
  const float xi = random_float(seed);
  return rho >= 1.0f || xi < rho;
}

// The prepare launch of every path frame; its kernels are below.
// (MOTION: the frame with motion -- the previous-position guide of the pixel's record, computed where the record is in registers)
// (SPEC: the frame with specular vertices -- alb[t].w = the primary hit's reflectivity, and with spec_cont, i.e. bounces > 0, a specular
//  primary hit continues: lit[t] is `term` alone, without background * reflectivity)
template <bool CAM, bool MOTION, bool EMI, bool SPEC = false, bool ENV = false>
__device__ __forceinline__ void path_prepare(const SceneDev& sc, const ShadeParams& p, uint32_t n, uint32_t W, uint32_t y0,
    const float* __restrict__ utab, const float* __restrict__ vtab, const HitRec* __restrict__ hb,
    float4* __restrict__ geo, float4* __restrict__ nrm, float4* __restrict__ dir, float4* __restrict__ lit, float4* __restrict__ alb,
    uint32_t* __restrict__ list, uint32_t* hdr, uint32_t* ctl_reset, std::conditional_t<MOTION, PrepMotion, PrepNoMotion> mo,
    std::conditional_t<EMI, PrepEmi, PrepNoEmi> em, uint32_t spec_cont = 0u, std::conditional_t<ENV, EnvTab, PrepNoEnv> env = {}) {
  if (ctl_reset && blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < CTL_DWORDS; i += 256u) ctl_reset[i] = 0u;
  bool hit_c[PREP_CHUNKS];
  uint32_t t_c[PREP_CHUNKS];
#pragma unroll
  for (int c = 0; c < PREP_CHUNKS; ++c) {
    const uint64_t t64 = ((uint64_t)blockIdx.x * PREP_CHUNKS + c) * 256u + threadIdx.x;
    const uint32_t t = (uint32_t)t64;
    bool hit = false;
    if (t64 < n) {
      const uint32_t x = t % W, y = y0 + t / W;
      HitRec h = hb[hit_index(x, y - y0, (W + 7u) >> 3)];
      const bool occ = (h.blasIdx & 0x80000000u) != 0u;
      h.blasIdx &= 0x7fffffffu;
      float ox, oy, oz, dx, dy, dz;
      if constexpr (CAM) camera_ray(utab, vtab, W, x, y, ox, oy, oz, dx, dy, dz);
      else generate_ray(utab[x], vtab[y], ox, oy, oz, dx, dy, dz);
      if (h.dist == RT_LARGE_FLOAT) {
        geo[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (ENV) {
          float L[3], pe;
          env_lookup(env, dx, dy, dz, L, pe);
          lit[t] = make_float4(L[0], L[1], L[2], 0.f);
        } else {
          lit[t] = make_float4(p.bg[0], p.bg[1], p.bg[2], 0.f);
        }
      } else {
        float r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz, a3[3];
        shade_terms<false>(sc, p, ox, oy, oz, dx, dy, dz, h, occ, r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz, nullptr, a3);
        if (!(SPEC && spec_cont && specular_vertex(refl))) {
          float thr = 1.0f;
          thr *= refl;
          r = r + p.bg[0] * thr; g = g + p.bg[1] * thr; b = b + p.bg[2] * thr;
        }
        if constexpr (EMI) {
          float e3[3];
          if (emission(sc, h.triIdx, em.scale, e3)) { r = r + e3[0]; g = g + e3[1]; b = b + e3[2]; }
        }
        geo[t] = make_float4(Ix, Iy, Iz, 1.0f);
        nrm[t] = make_float4(Nx, Ny, Nz, 0.f);
        dir[t] = make_float4(dx, dy, dz, 0.f);
        lit[t] = make_float4(r, g, b, 0.f);
        alb[t] = make_float4(a3[0], a3[1], a3[2], SPEC ? refl : 0.f);
        hit = true;
      }
      if constexpr (MOTION) {
        float4 Q4, N4;
        motion_guide(sc, mo.src, h, Q4, N4);
        mo.pos[t] = Q4; mo.nrm[t] = N4;
        if (mo.out) { float* o = mo.out + 4 * ((size_t)x + (size_t)y * W); o[0] = Q4.x; o[1] = Q4.y; o[2] = Q4.z; o[3] = Q4.w; }
      }
    }
    hit_c[c] = hit; t_c[c] = t;
  }
  wg_append<PREP_CHUNKS>(hit_c, t_c, list, hdr);
}

template <bool CAM, bool MOTION = false>
__global__ __launch_bounds__(256) void rt_path_prepare_kernel(SceneDev sc, ShadeParams p, uint32_t n, uint32_t W, uint32_t y0,
    const float* __restrict__ utab, const float* __restrict__ vtab, const HitRec* __restrict__ hb,
    float4* __restrict__ geo, float4* __restrict__ nrm, float4* __restrict__ dir, float4* __restrict__ lit, float4* __restrict__ alb,
    uint32_t* __restrict__ list, uint32_t* hdr, uint32_t* ctl_reset, std::conditional_t<MOTION, PrepMotion, PrepNoMotion> mo) {
  path_prepare<CAM, MOTION, false>(sc, p, n, W, y0, utab, vtab, hb, geo, nrm, dir, lit, alb, list, hdr, ctl_reset, mo, PrepNoEmi{});
}

// (the frame with emissive geometry, vxrt_render_path_emissive: Lit_0 + Emi(h_0) per pixel)
template <bool CAM>
__global__ __launch_bounds__(256) void rt_path_prepare_emissive_kernel(SceneDev sc, ShadeParams p, uint32_t n, uint32_t W, uint32_t y0,
    const float* __restrict__ utab, const float* __restrict__ vtab, const HitRec* __restrict__ hb,
    float4* __restrict__ geo, float4* __restrict__ nrm, float4* __restrict__ dir, float4* __restrict__ lit, float4* __restrict__ alb,
    uint32_t* __restrict__ list, uint32_t* hdr, uint32_t* ctl_reset, float scale) {
  path_prepare<CAM, false, true>(sc, p, n, W, y0, utab, vtab, hb, geo, nrm, dir, lit, alb, list, hdr, ctl_reset, PrepNoMotion{}, PrepEmi{scale});
}

// (the frame with emissive geometry and motion, vxrt_render_path_frame: both flavours at once; a camera frame, as every frame with motion)
__global__ __launch_bounds__(256) void rt_path_prepare_emissive_motion_kernel(SceneDev sc, ShadeParams p, uint32_t n, uint32_t W, uint32_t y0,
    const float* __restrict__ utab, const float* __restrict__ vtab, const HitRec* __restrict__ hb,
    float4* __restrict__ geo, float4* __restrict__ nrm, float4* __restrict__ dir, float4* __restrict__ lit, float4* __restrict__ alb,
    uint32_t* __restrict__ list, uint32_t* hdr, uint32_t* ctl_reset, PrepMotion mo, float scale) {
  path_prepare<true, true, true>(sc, p, n, W, y0, utab, vtab, hb, geo, nrm, dir, lit, alb, list, hdr, ctl_reset, mo, PrepEmi{scale});
}

// (the frame with specular vertices, vxrt_render_path_frame_specular: the pixel's reflectivity goes into alb[t].w; `cont` = bounces > 0)
template <bool CAM, bool EMI>
__global__ __launch_bounds__(256) void rt_path_prepare_specular_kernel(SceneDev sc, ShadeParams p, uint32_t n, uint32_t W, uint32_t y0,
    const float* __restrict__ utab, const float* __restrict__ vtab, const HitRec* __restrict__ hb,
    float4* __restrict__ geo, float4* __restrict__ nrm, float4* __restrict__ dir, float4* __restrict__ lit, float4* __restrict__ alb,
    uint32_t* __restrict__ list, uint32_t* hdr, uint32_t* ctl_reset, float scale, uint32_t cont) {
  if constexpr (EMI)
    path_prepare<CAM, false, true, true>(sc, p, n, W, y0, utab, vtab, hb, geo, nrm, dir, lit, alb, list, hdr, ctl_reset, PrepNoMotion{}, PrepEmi{scale}, cont);
  else
    path_prepare<CAM, false, false, true>(sc, p, n, W, y0, utab, vtab, hb, geo, nrm, dir, lit, alb, list, hdr, ctl_reset, PrepNoMotion{}, PrepNoEmi{}, cont);
}

// (the frame lit by an environment map, vxrt_render_path_frame_env: with or without motion)
template <bool CAM, bool MOTION>
__global__ __launch_bounds__(256) void rt_path_prepare_env_kernel(SceneDev sc, ShadeParams p, uint32_t n, uint32_t W, uint32_t y0,
    const float* __restrict__ utab, const float* __restrict__ vtab, const HitRec* __restrict__ hb,
    float4* __restrict__ geo, float4* __restrict__ nrm, float4* __restrict__ dir, float4* __restrict__ lit, float4* __restrict__ alb,
    uint32_t* __restrict__ list, uint32_t* hdr, uint32_t* ctl_reset, std::conditional_t<MOTION, PrepMotion, PrepNoMotion> mo, EnvTab env) {
  path_prepare<CAM, MOTION, false, false, true>(sc, p, n, W, y0, utab, vtab, hb, geo, nrm, dir, lit, alb, list, hdr, ctl_reset, mo, PrepNoEmi{}, 0u, env);
}

// start of a batch of ns samples: every slot takes its pixel's primary vertex (Lc = Lit, thr = Alb) and is live; hdr[1] = their number
__global__ __launch_bounds__(256) void rt_path_start_kernel(uint32_t cap, uint32_t ns, const uint32_t* __restrict__ list, uint32_t* hdr,
    const float4* __restrict__ geo, const float4* __restrict__ nrm, const float4* __restrict__ dir, const float4* __restrict__ lit, const float4* __restrict__ alb,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT, uint32_t* __restrict__ live) {
  const uint64_t want = (uint64_t)hdr[0] * ns;
  const uint32_t total = want < cap ? (uint32_t)want : cap;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) hdr[1] = total;
  if (i >= total) return;
  const uint32_t t = list[i / ns];
  pI[i] = geo[t]; pN[i] = nrm[t]; pD[i] = dir[t]; pL[i] = lit[t]; pT[i] = alb[t];
  live[i] = i;
}

// (the frame with specular vertices: thr = 1 -- it is multiplied when a ray leaves the vertex -- and pA = (Alb, reflectivity) of the
//  primary vertex, which the specular prepare launch left in alb[t])
__global__ __launch_bounds__(256) void rt_path_start_specular_kernel(uint32_t cap, uint32_t ns, const uint32_t* __restrict__ list, uint32_t* hdr,
    const float4* __restrict__ geo, const float4* __restrict__ nrm, const float4* __restrict__ dir, const float4* __restrict__ lit, const float4* __restrict__ alb,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT, float4* __restrict__ pA,
    uint32_t* __restrict__ live) {
  const uint64_t want = (uint64_t)hdr[0] * ns;
  const uint32_t total = want < cap ? (uint32_t)want : cap;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) hdr[1] = total;
  if (i >= total) return;
  const uint32_t t = list[i / ns];
  pI[i] = geo[t]; pN[i] = nrm[t]; pD[i] = dir[t]; pL[i] = lit[t]; pT[i] = make_float4(1.f, 1.f, 1.f, 0.f); pA[i] = alb[t];
  live[i] = i;
}

// the bounce rays of one depth: ray q leaves the last vertex of slot live[q] (user seed = seed + depth); zeroes the next depth's count
__global__ __launch_bounds__(256) void rt_path_bounce_rays_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t spp, uint32_t s0, uint32_t ns, uint32_t user_seed,
    const uint32_t* __restrict__ list, const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, unsigned long long* rays_traced) {
  const uint32_t total = min(*n_live, cap);
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q == 0) {
    *n_next = 0u;
    if (rays_traced && total) atomicAdd(rays_traced, (unsigned long long)total);   // (every live path traces one)
  }
  if (q >= total) return;
  const uint32_t slot = live[q], t = list[slot / ns], smp = s0 + slot % ns;
  const uint32_t x = t % W, y = y0 + t / W;
  const float4 I = pI[slot], N = pN[slot], D = pD[slot];
  float r6[6];
  ao_sample_ray(x, y, W, spp, smp, user_seed, I.x, I.y, I.z, N.x, N.y, N.z, D.x, D.y, D.z, r6);
  float* o = rays + (size_t)q * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = r6[k];
}

// The emitter ray of the header's "Emissive geometry", operation for operation: from hash output `seed`, the surface point I and the
// facing normal N' (nx, ny, nz).  ray6 = (o, w), tmax, G[3], e = the emitter chosen; false = skipped: the ray nothing can hit, tmax = -1,
// G = 0.  The cumulative table is read from global memory (a binary search of at most 17 steps; n <= 65,536).
// (MIS: the emitter-ray side of the header's "Multiple importance sampling" -- G is Gm = G * wE, wE goes to *wE_out (0 for a skipped ray),
//  and a Gm that is not finite skips the ray as well)
template <bool MIS = false>
__device__ __forceinline__ bool emitter_sample(const EmitterTab& tab, float scale, uint32_t seed, float Ix, float Iy, float Iz, float nx, float ny, float nz,
                                               float (&ray6)[6], float& tmax, float (&G)[3], uint32_t& e_out, float* wE_out = nullptr) {
  if (seed == 0u) seed = 1u;
  seed ^= seed << 13; seed ^= seed >> 17; seed ^= seed << 5;
  const uint32_t r0 = seed;
  float a = random_float(seed);
  float b = random_float(seed);
  const uint32_t t = (uint32_t)(((uint64_t)r0 * tab.Q) >> 32);
  uint32_t lo = 0u, hi = tab.n - 1u;   // the smallest e with cum[e] > t is in [lo, hi] (cum[n - 1] = Q > t)
  for (int k = 0; k < 17; ++k) {
    if (lo >= hi) break;
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (tab.cum[mid] > t) hi = mid; else lo = mid + 1u;
  }
  const uint32_t e = lo;
  e_out = e;
  const float* T = tab.tri + (size_t)e * 12;
  const float v0x = T[0], v0y = T[1], v0z = T[2], e1x = T[3], e1y = T[4], e1z = T[5], e2x = T[6], e2y = T[7], e2z = T[8];
  if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
  const float Px = (v0x + a * e1x) + b * e2x, Py = (v0y + a * e1y) + b * e2y, Pz = (v0z + a * e1z) + b * e2z;
  const float ox = Ix + nx * 0.001f, oy = Iy + ny * 0.001f, oz = Iz + nz * 0.001f;
  const float vx = Px - ox, vy = Py - oy, vz = Pz - oz;
  const float d2 = (vx * vx + vy * vy) + vz * vz;
  const float d = sqrtf(d2);
  const float wx = vx / d, wy = vy / d, wz = vz / d;
  const float cosx = std_max(0.0f, (nx * wx + ny * wy) + nz * wz);
  const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  const float an = 0.5f * fabsf((cx * wx + cy * wy) + cz * wz);
  const float den = (3.14159265f * d2) * ((float)tab.q[e] / (float)tab.Q);
  G[0] = (((T[9] * scale) * cosx) * an) / den;
  G[1] = (((T[10] * scale) * cosx) * an) / den;
  G[2] = (((T[11] * scale) * cosx) * an) / den;
  bool skip = cosx == 0.0f || d2 == 0.0f || !isfinite(G[0]) || !isfinite(G[1]) || !isfinite(G[2]);
  if constexpr (MIS) {
    const float qf = (float)tab.q[e] / (float)tab.Q;
    const float pe = d2 * qf;
    const float pb = (cosx / 3.14159265f) * an;
    const float wE = pe / (pe + pb);
    G[0] = G[0] * wE; G[1] = G[1] * wE; G[2] = G[2] * wE;
    skip = skip || !isfinite(G[0]) || !isfinite(G[1]) || !isfinite(G[2]);
    *wE_out = skip ? 0.0f : wE;
  }
  if (skip) {
    ray6[0] = 0.f; ray6[1] = 0.f; ray6[2] = 0.f; ray6[3] = 1.f; ray6[4] = 1.f; ray6[5] = 1.f;
    tmax = -1.0f;
    G[0] = 0.f; G[1] = 0.f; G[2] = 0.f;
    return false;
  }
  ray6[0] = ox; ray6[1] = oy; ray6[2] = oz; ray6[3] = wx; ray6[4] = wy; ray6[5] = wz;
  tmax = d - 0.001f;
  return true;
}

// rt_path_bounce_rays_kernel of a frame with emitter sampling (nee = 1): besides the bounce ray of slot live[q], the emitter ray of the
// same vertex -- user seed (seed + depth) ^ 0x80000000 in the bounce ray's hash input -- with its tmax and G (w = 1: real; a skipped
// one is not counted).  One atomic per workgroup on the ray counter for the emitter rays, thread 0's for the bounce rays.
// (MIS: the frame of the header's "Multiple importance sampling" -- eG[q] = (Gm, real))
// (SlotSrc: where slot -> (pixel of the window, sample, the spp of the hash inputs) comes from -- SlotUniform, the batches of whole
//  samples of render_path_tail; SlotCounts, the slot tables and the pixel's own count of render_path_counts_tail.  No thread leaves
//  before the barriers: a workgroup past the live count, and every workgroup of a batch without live paths, falls through with real =
//  false in all its lanes and adds nothing.)
struct SlotUniform {
  uint32_t spp, s0, ns; const uint32_t* __restrict__ list;
  __device__ __forceinline__ void get(uint32_t slot, uint32_t& t, uint32_t& smp, uint32_t& n) const { t = list[slot / ns]; smp = s0 + slot % ns; n = spp; }
};
struct SlotCounts {
  const uint32_t* __restrict__ spix; const uint32_t* __restrict__ ssmp; const uint32_t* __restrict__ cnt;
  __device__ __forceinline__ void get(uint32_t slot, uint32_t& t, uint32_t& smp, uint32_t& n) const { t = spix[slot]; smp = ssmp[slot]; n = cnt[t]; }
};
template <bool MIS, class SlotSrc>
__device__ __forceinline__ void path_bounce_emitter_rays(uint32_t cap, uint32_t W, uint32_t y0, const SlotSrc& src, uint32_t user_seed,
    const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, const EmitterTab& tab, float scale,
    float* __restrict__ erays, float* __restrict__ etmax, float4* __restrict__ eG, unsigned long long* rays_traced) {
  __shared__ uint32_t s_real;
  if (threadIdx.x == 0) s_real = 0u;
  __syncthreads();
  const uint32_t total = min(*n_live, cap);
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q == 0) {
    *n_next = 0u;
    if (rays_traced && total) atomicAdd(rays_traced, (unsigned long long)total);   // (every live path traces one bounce ray)
  }
  bool real = false;
  if (q < total) {
    const uint32_t slot = live[q];
    uint32_t t, smp, spp;
    src.get(slot, t, smp, spp);
    const uint32_t x = t % W, y = y0 + t / W;
    const float4 I = pI[slot], N = pN[slot], D = pD[slot];
    float r6[6];
    ao_sample_ray(x, y, W, spp, smp, user_seed, I.x, I.y, I.z, N.x, N.y, N.z, D.x, D.y, D.z, r6);
    float* o = rays + (size_t)q * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = r6[k];
    float nx = N.x, ny = N.y, nz = N.z;
    if (nx * D.x + ny * D.y + nz * D.z > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }   // (N' as ao_sample_ray turns it)
    const uint32_t seed = wang_hash((x + y * W) * spp + smp + 1u + (user_seed ^ 0x80000000u) * 0x9E3779B9u);
    float e6[6], tm, G[3];
    uint32_t e;
    float wE;
    real = emitter_sample<MIS>(tab, scale, seed, I.x, I.y, I.z, nx, ny, nz, e6, tm, G, e, &wE);
    float* eo = erays + (size_t)q * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) eo[k] = e6[k];
    etmax[q] = tm;
    eG[q] = make_float4(G[0], G[1], G[2], real ? 1.0f : 0.0f);
  }
  const unsigned long long m = __ballot(real);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&s_real, (uint32_t)__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && rays_traced && s_real) atomicAdd(rays_traced, (unsigned long long)s_real);
}

__global__ __launch_bounds__(256) void rt_path_bounce_emitter_rays_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t spp, uint32_t s0, uint32_t ns, uint32_t user_seed,
    const uint32_t* __restrict__ list, const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, EmitterTab tab, float scale,
    float* __restrict__ erays, float* __restrict__ etmax, float4* __restrict__ eG, unsigned long long* rays_traced) {
  path_bounce_emitter_rays<false>(cap, W, y0, SlotUniform{spp, s0, ns, list}, user_seed, live, n_live, n_next, pI, pN, pD, rays, tab, scale, erays, etmax, eG, rays_traced);
}

__global__ __launch_bounds__(256) void rt_path_bounce_emitter_rays_mis_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t spp, uint32_t s0, uint32_t ns, uint32_t user_seed,
    const uint32_t* __restrict__ list, const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, EmitterTab tab, float scale,
    float* __restrict__ erays, float* __restrict__ etmax, float4* __restrict__ eG, unsigned long long* rays_traced) {
  path_bounce_emitter_rays<true>(cap, W, y0, SlotUniform{spp, s0, ns, list}, user_seed, live, n_live, n_next, pI, pN, pD, rays, tab, scale, erays, etmax, eG, rays_traced);
}

// rt_path_bounce_rays_kernel of a frame that samples its environment map (the header's "Environment light", sample = 1): besides the
// bounce ray of slot live[q], the environment ray of the same vertex -- user seed (seed + depth) ^ 0x10000000 in the bounce ray's hash
// input -- where path_bounce_emitter_rays writes the emitter ray: erays, etmax, eG[q] = (Gm, real).  The two forms exclude each other,
// so the buffers and the any-hit launch behind them serve both.  The row ends of the map's table are staged in LDS first; as there, no
// thread leaves before the barriers and the environment rays cost one atomic per workgroup.
template <class SlotSrc>
__device__ __forceinline__ void path_bounce_env_rays(uint32_t cap, uint32_t W, uint32_t y0, const SlotSrc& src, uint32_t user_seed,
    const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, const EnvTab& env,
    float* __restrict__ erays, float* __restrict__ etmax, float4* __restrict__ eG, unsigned long long* rays_traced) {
  __shared__ uint32_t s_real;
  __shared__ uint32_t s_rows[ENV_MAX_N];
  if (threadIdx.x == 0) s_real = 0u;
  env_stage_rows(env, s_rows);
  const uint32_t total = min(*n_live, cap);
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q == 0) {
    *n_next = 0u;
    if (rays_traced && total) atomicAdd(rays_traced, (unsigned long long)total);   // (every live path traces one bounce ray)
  }
  bool real = false;
  if (q < total) {
    const uint32_t slot = live[q];
    uint32_t t, smp, spp;
    src.get(slot, t, smp, spp);
    const uint32_t x = t % W, y = y0 + t / W;
    const float4 I = pI[slot], N = pN[slot], D = pD[slot];
    float r6[6];
    ao_sample_ray(x, y, W, spp, smp, user_seed, I.x, I.y, I.z, N.x, N.y, N.z, D.x, D.y, D.z, r6);
    float* o = rays + (size_t)q * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = r6[k];
    float nx = N.x, ny = N.y, nz = N.z;
    if (nx * D.x + ny * D.y + nz * D.z > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }   // (N' as ao_sample_ray turns it)
    const uint32_t seed = wang_hash((x + y * W) * spp + smp + 1u + (user_seed ^ 0x10000000u) * 0x9E3779B9u);
    float e6[6], tm, G[3], wE;
    uint32_t e;
    real = env_sample(env, s_rows, seed, I.x, I.y, I.z, nx, ny, nz, e6, tm, G, e, wE);
    float* eo = erays + (size_t)q * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) eo[k] = e6[k];
    etmax[q] = tm;
    eG[q] = make_float4(G[0], G[1], G[2], real ? 1.0f : 0.0f);
  }
  const unsigned long long m = __ballot(real);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&s_real, (uint32_t)__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && rays_traced && s_real) atomicAdd(rays_traced, (unsigned long long)s_real);
}

__global__ __launch_bounds__(256) void rt_path_bounce_env_rays_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t spp, uint32_t s0, uint32_t ns, uint32_t user_seed,
    const uint32_t* __restrict__ list, const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, EnvTab env,
    float* __restrict__ erays, float* __restrict__ etmax, float4* __restrict__ eG, unsigned long long* rays_traced) {
  path_bounce_env_rays(cap, W, y0, SlotUniform{spp, s0, ns, list}, user_seed, live, n_live, n_next, pI, pN, pD, rays, env, erays, etmax, eG, rays_traced);
}

// The bounce rays of one depth of a frame with specular vertices (the header's "Specular vertices"): per-slot state holds thr BEFORE the
// last vertex's albedo (pT) and that vertex's Alb and reflectivity (pA), and the ray that leaves is chosen by the lobe pick -- user seed
// (seed + depth) ^ 0x40000000 in the bounce ray's hash input.  Mirror: mirror_ray about the unturned normal, thr unchanged, the segment
// marked specular in pD[slot].w.  Diffuse: the ray of rt_path_bounce_rays_kernel, thr = thr * Alb written back, the mark cleared.
// (EM: 0 no emitter ray -- the plain frame and nee = 0; 1 emitter sampling, 2 its weighted twin: the emitter ray of
//  path_bounce_emitter_rays for a vertex that picks diffuse, a skipped one -- tmax = -1, G = 0, not counted -- for one that picks mirror.
//  As there, no thread leaves before the barriers and the emitter rays cost one atomic per workgroup.)
struct SpecNoEm {};
struct SpecEm { EmitterTab tab; float scale; float* erays; float* etmax; float4* eG; };
template <int EM, class SlotSrc>
__device__ __forceinline__ void path_bounce_specular(uint32_t cap, uint32_t W, uint32_t y0, const SlotSrc& src, uint32_t user_seed,
    const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pT, const float4* __restrict__ pA,
    float* __restrict__ rays, const std::conditional_t<EM != 0, SpecEm, SpecNoEm>& em, unsigned long long* rays_traced) {
  __shared__ uint32_t s_real;
  if constexpr (EM != 0) {
    if (threadIdx.x == 0) s_real = 0u;
    __syncthreads();
  }
  const uint32_t total = min(*n_live, cap);
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q == 0) {
    *n_next = 0u;
    if (rays_traced && total) atomicAdd(rays_traced, (unsigned long long)total);   // (every live path traces one bounce ray, mirror or diffuse)
  }
  bool real = false;
  if (q < total) {
    const uint32_t slot = live[q];
    uint32_t t, smp, spp;
    src.get(slot, t, smp, spp);
    const uint32_t x = t % W, y = y0 + t / W;
    const float4 I = pI[slot], N = pN[slot], D = pD[slot], A = pA[slot];
    const bool mirror = specular_vertex(A.w) && specular_pick(A.w, wang_hash((x + y * W) * spp + smp + 1u + (user_seed ^ 0x40000000u) * 0x9E3779B9u));
    float r6[6];
    float4 T = pT[slot];
    if (mirror) {
      mirror_ray(D.x, D.y, D.z, I.x, I.y, I.z, N.x, N.y, N.z, r6);
    } else {
      ao_sample_ray(x, y, W, spp, smp, user_seed, I.x, I.y, I.z, N.x, N.y, N.z, D.x, D.y, D.z, r6);
      T = make_float4(T.x * A.x, T.y * A.y, T.z * A.z, 0.f);
      pT[slot] = T;
    }
    pD[slot].w = mirror ? 1.0f : 0.0f;
    float* o = rays + (size_t)q * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = r6[k];
    if constexpr (EM != 0) {
      float e6[6] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f}, tm = -1.0f, G[3] = {0.f, 0.f, 0.f};
      if (!mirror) {
        float nx = N.x, ny = N.y, nz = N.z;
        if (nx * D.x + ny * D.y + nz * D.z > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }   // (N' as ao_sample_ray turns it)
        const uint32_t seed = wang_hash((x + y * W) * spp + smp + 1u + (user_seed ^ 0x80000000u) * 0x9E3779B9u);
        uint32_t e;
        float wE;
        real = emitter_sample<EM == 2>(em.tab, em.scale, seed, I.x, I.y, I.z, nx, ny, nz, e6, tm, G, e, &wE);
      }
      float* eo = em.erays + (size_t)q * 6;
#pragma unroll
      for (int k = 0; k < 6; ++k) eo[k] = e6[k];
      em.etmax[q] = tm;
      em.eG[q] = make_float4(G[0], G[1], G[2], real ? 1.0f : 0.0f);
    }
  }
  if constexpr (EM != 0) {
    const unsigned long long m = __ballot(real);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&s_real, (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && rays_traced && s_real) atomicAdd(rays_traced, (unsigned long long)s_real);
  }
}

template <int EM>
__global__ __launch_bounds__(256) void rt_path_bounce_specular_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t spp, uint32_t s0, uint32_t ns, uint32_t user_seed,
    const uint32_t* __restrict__ list, const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pT, const float4* __restrict__ pA,
    float* __restrict__ rays, std::conditional_t<EM != 0, SpecEm, SpecNoEm> em, unsigned long long* rays_traced) {
  path_bounce_specular<EM>(cap, W, y0, SlotUniform{spp, s0, ns, list}, user_seed, live, n_live, n_next, pI, pN, pD, pT, pA, rays, em, rays_traced);
}

// (the slot's pixel, sample and the pixel's own sample count, as rt_path_bounce_rays_counts_kernel reads them: the pick's hash input is
//  (x + y * W) * n_p + s + 1 + u * 0x9E3779B9 too)
template <int EM>
__global__ __launch_bounds__(256) void rt_path_bounce_specular_counts_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t user_seed,
    const uint32_t* __restrict__ spix, const uint32_t* __restrict__ ssmp, const uint32_t* __restrict__ cnt,
    const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pT, const float4* __restrict__ pA,
    float* __restrict__ rays, std::conditional_t<EM != 0, SpecEm, SpecNoEm> em, unsigned long long* rays_traced) {
  path_bounce_specular<EM>(cap, W, y0, SlotCounts{spix, ssmp, cnt}, user_seed, live, n_live, n_next, pI, pN, pD, pT, pA, rays, em, rays_traced);
}

// vxrt_specular_pick: the pick and the mirror ray of n caller-supplied vertices (I, N, dir, rho) and hash outputs, one per thread; a
// vertex that picks diffuse gets six zeros
__global__ __launch_bounds__(256) void rt_specular_pick_kernel(uint32_t n, const float* __restrict__ vertices, const uint32_t* __restrict__ seeds,
    float* __restrict__ rays, uint32_t* __restrict__ lobe) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float* v = vertices + (size_t)i * 10;
  float r6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool mirror = specular_pick(v[9], seeds[i]);
  if (mirror) mirror_ray(v[6], v[7], v[8], v[0], v[1], v[2], v[3], v[4], v[5], r6);
  float* o = rays + (size_t)i * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = r6[k];
  lobe[i] = mirror ? 1u : 0u;
}

// The emitter index of the header's "Multiple importance sampling": the position of (blas, tri) among the sorted (blasIdx, triIdx, e)
// -- the smallest position whose key is not below the wanted one, a binary search over [0, n - 1] of at most 17 steps -- and e of that
// position if its key is equal; 0xFFFFFFFF: the pair is not listed
__device__ __forceinline__ uint32_t emitter_lookup(const EmitterIdx& ix, uint32_t blas, uint32_t tri) {
  if (ix.n == 0u) return 0xFFFFFFFFu;
  const uint64_t want = ((uint64_t)blas << 32) | tri;
  uint32_t lo = 0u, hi = ix.n - 1u;
  for (int k = 0; k < 17; ++k) {
    if (lo >= hi) break;
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t key = ((uint64_t)ix.ent[3 * (size_t)mid] << 32) | ix.ent[3 * (size_t)mid + 1];
    if (key < want) lo = mid + 1u; else hi = mid;
  }
  const uint32_t* p = ix.ent + 3 * (size_t)lo;
  return (p[0] == blas && p[1] == tri) ? p[2] : 0xFFFFFFFFu;
}

// wB of the header's "Multiple importance sampling", operation for operation: the bounce ray of direction w that left a vertex with
// facing normal N' (nx, ny, nz) hit entry e of the table at distance t
__device__ __forceinline__ float emitter_hit_weight(const EmitterTab& tab, uint32_t e, float nx, float ny, float nz, float wx, float wy, float wz, float t) {
  const float* T = tab.tri + (size_t)e * 12;
  const float e1x = T[3], e1y = T[4], e1z = T[5], e2x = T[6], e2y = T[7], e2z = T[8];
  const float qf = (float)tab.q[e] / (float)tab.Q;
  const float cosx = std_max(0.0f, (nx * wx + ny * wy) + nz * wz);
  const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  const float an = 0.5f * fabsf((cx * wx + cy * wy) + cz * wz);
  const float pe = (t * t) * qf;
  const float pb = (cosx / 3.14159265f) * an;
  const float den = pe + pb;
  return den > 0.0f ? pb / den : 1.0f;
}

// vxrt_emitter_hit_weights: lookup and wB of n caller-supplied bounce rays, hit records and N', one per thread (bit 31 of blasIdx is
// masked; nothing of the scene is read, so a record may name any pair)
__global__ __launch_bounds__(256) void rt_emitter_hit_weights_kernel(EmitterTab tab, EmitterIdx ix, uint32_t n, const float* __restrict__ rays,
    const HitRec* __restrict__ hits, const float* __restrict__ normals, uint32_t* __restrict__ emitter, float* __restrict__ mis) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const HitRec h = hits[i];
  const uint32_t e = emitter_lookup(ix, h.blasIdx & 0x7fffffffu, h.triIdx);
  float w = 1.0f;
  if (e < tab.n) {
    const float* r = rays + (size_t)i * 6;
    const float* nr = normals + (size_t)i * 3;
    w = emitter_hit_weight(tab, e, nr[0], nr[1], nr[2], r[3], r[4], r[5], h.dist);
  }
  emitter[i] = e < tab.n ? e : 0xFFFFFFFFu;
  mis[i] = w;
}

// vxrt_emitter_rays_mis: rt_emitter_rays_kernel with weight3 = Gm and mis = wE
__global__ __launch_bounds__(256) void rt_emitter_rays_mis_kernel(EmitterTab tab, uint32_t n, const float* __restrict__ points, const uint32_t* __restrict__ seeds, float scale,
    float* __restrict__ rays, float* __restrict__ tmax, float* __restrict__ weight3, uint32_t* __restrict__ emitter, float* __restrict__ mis) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float* pt = points + (size_t)i * 6;
  float e6[6], tm, G[3], wE;
  uint32_t e;
  emitter_sample<true>(tab, scale, seeds[i], pt[0], pt[1], pt[2], pt[3], pt[4], pt[5], e6, tm, G, e, &wE);
  float* o = rays + (size_t)i * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = e6[k];
  tmax[i] = tm;
  weight3[3 * (size_t)i] = G[0]; weight3[3 * (size_t)i + 1] = G[1]; weight3[3 * (size_t)i + 2] = G[2];
  emitter[i] = e;
  mis[i] = wE;
}

// vxrt_emitter_rays: the emitter ray of n caller-supplied (I, N') and hash outputs, one per thread
__global__ __launch_bounds__(256) void rt_emitter_rays_kernel(EmitterTab tab, uint32_t n, const float* __restrict__ points, const uint32_t* __restrict__ seeds, float scale,
    float* __restrict__ rays, float* __restrict__ tmax, float* __restrict__ weight3, uint32_t* __restrict__ emitter) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float* pt = points + (size_t)i * 6;
  float e6[6], tm, G[3];
  uint32_t e;
  emitter_sample(tab, scale, seeds[i], pt[0], pt[1], pt[2], pt[3], pt[4], pt[5], e6, tm, G, e);
  float* o = rays + (size_t)i * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = e6[k];
  tmax[i] = tm;
  weight3[3 * (size_t)i] = G[0]; weight3[3 * (size_t)i + 1] = G[1]; weight3[3 * (size_t)i + 2] = G[2];
  emitter[i] = e;
}

// the occlusion rays of one depth (light sampling): one per bounce ray that hit; a miss gets a ray nothing can hit, which is not
// counted (see rt_bounce_shadow_rays_kernel).  One atomic per workgroup on the ray counter.
__global__ __launch_bounds__(256) void rt_path_occlusion_rays_kernel(ShadeParams p, uint32_t cap, const uint32_t* n_live, const float* __restrict__ rays,
    const HitRec* __restrict__ hits, float* __restrict__ srays, float* __restrict__ stmax, unsigned long long* rays_traced) {
  __shared__ uint32_t s_real;
  if (threadIdx.x == 0) s_real = 0u;
  __syncthreads();
  const uint32_t total = min(*n_live, cap);
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  bool real = false;
  if (q < total) {
    const float* rp = rays + (size_t)q * 6;
    float* sp = srays + (size_t)q * 6;
    const float d = hits[q].dist;
    if (d == RT_LARGE_FLOAT) {
      sp[0] = 0.f; sp[1] = 0.f; sp[2] = 0.f; sp[3] = 1.f; sp[4] = 1.f; sp[5] = 1.f;
      stmax[q] = -1.0f;
    } else {
      float sdist;
      shadow_ray(p, rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], d, sp[0], sp[1], sp[2], sp[3], sp[4], sp[5], sdist);
      stmax[q] = sdist;
      real = true;
    }
  }
  const unsigned long long m = __ballot(real);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&s_real, (uint32_t)__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && rays_traced && s_real) atomicAdd(rays_traced, (unsigned long long)s_real);
}

// the scatter step of one depth.  Miss: Lc = Lc + thr * background, the path ends.  Hit: Lc = Lc + thr * Lit (occluded iff shits[q]
// hit), then thr = thr * Alb and the hit becomes the slot's last vertex; with `next` the slot is appended to the next depth's live list.
// (EMI: the frame with emissive geometry, the header's "Emissive geometry".  1, nee = 0: a hit adds thr * Emi(h') after thr * Lit.
//  2, nee = 1: before the miss / hit arm Lc = Lc + thr * G for an emitter ray that is real -- eG[q].w -- and was not blocked -- ehits[q].)
//  3, the header's "Multiple importance sampling": the emitter ray's term as for 2 -- eG holds Gm -- and a hit whose material emits adds
//  thr * (Emi(h') * wB) after thr * Lit; only those lanes look the hit up in the emitter index and read the vertex the ray left.)
struct ScatterEmi { float scale; const HitRec* ehits; const float4* eG; };
struct ScatterMis { float scale; const HitRec* ehits; const float4* eG; EmitterTab tab; EmitterIdx idx; };
struct ScatterNoEmi {};
// (EMI 4 and 5: the frame lit by an environment map, the header's "Environment light", sample = 0 and 1.  A miss adds thr * Env(w) in
//  place of thr * background -- with 5 weighted by wB, from N' of the vertex the ray left, which a miss leaves in its slot -- and 5 adds
//  the environment ray's term as 2 adds the emitter ray's: eG holds Gm.  The lookup's divisions and square root run in the lanes that
//  missed only.)
struct ScatterEnv { const HitRec* ehits; const float4* eG; EnvTab tab; };
template <int EMI> using ScatterEm = std::conditional_t<EMI >= 4, ScatterEnv, std::conditional_t<EMI == 3, ScatterMis, std::conditional_t<EMI != 0, ScatterEmi, ScatterNoEmi>>>;
// (SPEC: the frame of the header's "Specular vertices".  pT is thr as the ray left with it and is not touched here; a hit that goes on
//  stores its Alb and reflectivity in pA instead, and if it is specular it adds `term` alone.  pD[slot].w marks the segment that arrives:
//  after a specular one a hit whose material emits adds thr * Emi in full in all three emitter forms, without a lookup.)
// The header's "Russian roulette", operation for operation.  roulette_q: the survival probability of throughput t -- its largest
// component as the three compares form it, floored by q_min (a NaN takes q_min).  q >= 1 takes no draw.  roulette_draw: the draw of a
// vertex with q < 1 from hash output `seed` (0 becomes 1; one xorshift step, as the lobe pick) -- true = the path survives and t is
// divided by q, three correctly rounded divisions and no reciprocal.
__device__ __forceinline__ float roulette_q(const float (&t)[3], float q_min) {
  float m = t[0];
  if (t[1] > m) m = t[1];
  if (t[2] > m) m = t[2];
  float q = m;
  if (!(q >= q_min)) q = q_min;
  return q;
}
__device__ __forceinline__ bool roulette_draw(float (&t)[3], float q, uint32_t seed) {
  if (seed == 0u) seed = 1u;
  const float xi = random_float(seed);
  if (!(xi < q)) return false;
  t[0] = t[0] / q; t[1] = t[1] / q; t[2] = t[2] / q;
  return true;
}

// vxrt_roulette: the step alone on n caller-supplied throughputs and hash outputs, one per thread; a dead entry gets three zeros
__global__ __launch_bounds__(256) void rt_roulette_kernel(uint32_t n, const float* __restrict__ thr, const uint32_t* __restrict__ seeds, float q_min,
    float* __restrict__ thr_out, uint32_t* __restrict__ alive) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  float t[3] = {thr[3 * (size_t)i], thr[3 * (size_t)i + 1], thr[3 * (size_t)i + 2]};
  const float q = roulette_q(t, q_min);
  const bool lives = q >= 1.0f || roulette_draw(t, q, seeds[i]);
  float* o = thr_out + 3 * (size_t)i;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = lives ? t[k] : 0.f;
  alive[i] = lives ? 1u : 0u;
}

// (RR: the scatter step of a depth whose hits take the draw of the header's "Russian roulette" -- launched with `next` only, and never
//  with SPEC.  After thr = thr * Alb the vertex forms q; with q < 1 it draws from the bounce ray's hash input with bit 29 of the user seed
//  flipped, which takes the slot's pixel and sample from the slot source the bounce-ray kernels read.  A path that dies keeps its Lc and
//  is not appended; nothing else of its slot is written.)
struct ScatterNoRoulette {};
template <class SlotSrc> struct ScatterRoulette { SlotSrc src; uint32_t W, y0, user_seed; float q_min; };
template <int EMI, bool SPEC = false, bool RR = false, class SlotSrc = SlotUniform>
__device__ __forceinline__ void path_scatter(const SceneDev& sc, const ShadeParams& p, uint32_t cap, const uint32_t* n_live, const uint32_t* __restrict__ live,
    const float* __restrict__ rays, const HitRec* __restrict__ hits, const HitRec* __restrict__ shits,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT,
    uint32_t* __restrict__ next, uint32_t* n_next, const ScatterEm<EMI>& em,
    float4* __restrict__ pA = nullptr, const std::conditional_t<RR, ScatterRoulette<SlotSrc>, ScatterNoRoulette>& rr = {}) {
  static_assert(!(RR && SPEC), "a specular frame takes no roulette (check_request)");
  static_assert(!(EMI >= 4 && SPEC), "a frame lit by an environment map has no specular vertices (check_request)");
  const uint32_t total = min(*n_live, cap);
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  bool go[1] = {false};
  uint32_t val[1] = {0u};
  if (q < total) {
    const uint32_t slot = live[q];
    const float* rp = rays + (size_t)q * 6;
    HitRec h = hits[q];
    h.blasIdx &= 0x7fffffffu;
    float4 L = pL[slot];
    const float4 T = pT[slot];
    bool seg = false;   // (the segment that arrives is specular)
    if constexpr (SPEC) seg = pD[slot].w != 0.f;
    if constexpr (EMI == 2 || EMI == 3 || EMI == 5) {
      const float4 G = em.eG[q];
      if (G.w != 0.f && em.ehits[q].dist == RT_LARGE_FLOAT) { L.x = L.x + T.x * G.x; L.y = L.y + T.y * G.y; L.z = L.z + T.z * G.z; }
    }
    if (h.dist == RT_LARGE_FLOAT) {
      if constexpr (EMI >= 4) {
        float E3[3], pe;
        env_lookup(em.tab, rp[3], rp[4], rp[5], E3, pe);
        if constexpr (EMI == 5) {
          const float4 N = pN[slot], D = pD[slot];   // (the vertex the ray left)
          float nx = N.x, ny = N.y, nz = N.z;
          if (nx * D.x + ny * D.y + nz * D.z > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }   // (N' as ao_sample_ray turns it)
          const float wB = env_miss_weight(pe, nx, ny, nz, rp[3], rp[4], rp[5]);
          E3[0] = E3[0] * wB; E3[1] = E3[1] * wB; E3[2] = E3[2] * wB;
        }
        L.x = L.x + T.x * E3[0]; L.y = L.y + T.y * E3[1]; L.z = L.z + T.z * E3[2];
      } else {
        L.x = L.x + T.x * p.bg[0]; L.y = L.y + T.y * p.bg[1]; L.z = L.z + T.z * p.bg[2];
      }
    } else {
      const bool occ = shits != nullptr && shits[q].dist != RT_LARGE_FLOAT;
      float r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz, a3[3];
      shade_terms<false>(sc, p, rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], h, occ, r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz, nullptr, a3);
      if (!(SPEC && next && specular_vertex(refl))) {
        float thr = 1.0f;
        thr *= refl;
        r = r + p.bg[0] * thr; g = g + p.bg[1] * thr; b = b + p.bg[2] * thr;
      }
      L.x = L.x + T.x * r; L.y = L.y + T.y * g; L.z = L.z + T.z * b;
      if constexpr (SPEC && EMI == 2) {
        float e3[3];
        if (seg && emission(sc, h.triIdx, em.scale, e3)) { L.x = L.x + T.x * e3[0]; L.y = L.y + T.y * e3[1]; L.z = L.z + T.z * e3[2]; }
      }
      if constexpr (EMI == 1) {
        float e3[3];
        if (emission(sc, h.triIdx, em.scale, e3)) { L.x = L.x + T.x * e3[0]; L.y = L.y + T.y * e3[1]; L.z = L.z + T.z * e3[2]; }
      }
      if constexpr (EMI == 3) {
        float e3[3];
        if (emission(sc, h.triIdx, em.scale, e3)) {
          float wB = 1.0f;
          const uint32_t e = seg ? 0xFFFFFFFFu : emitter_lookup(em.idx, h.blasIdx, h.triIdx);
          if (e < em.tab.n) {
            const float4 N = pN[slot], D = pD[slot];   // (the vertex the ray left: overwritten below)
            float nx = N.x, ny = N.y, nz = N.z;
            if (nx * D.x + ny * D.y + nz * D.z > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }   // (N' as ao_sample_ray turns it)
            wB = emitter_hit_weight(em.tab, e, nx, ny, nz, rp[3], rp[4], rp[5], h.dist);
          }
          L.x = L.x + T.x * (e3[0] * wB); L.y = L.y + T.y * (e3[1] * wB); L.z = L.z + T.z * (e3[2] * wB);
        }
      }
      if constexpr (RR) {
        if (next) {
          float t3[3] = {T.x * a3[0], T.y * a3[1], T.z * a3[2]};
          const float q = roulette_q(t3, rr.q_min);
          bool lives = true;
          if (!(q >= 1.0f)) {
            uint32_t t, smp, spp;
            rr.src.get(slot, t, smp, spp);
            const uint32_t x = t % rr.W, y = rr.y0 + t / rr.W;
            lives = roulette_draw(t3, q, wang_hash((x + y * rr.W) * spp + smp + 1u + (rr.user_seed ^ 0x20000000u) * 0x9E3779B9u));
          }
          if (lives) {
            pT[slot] = make_float4(t3[0], t3[1], t3[2], 0.f);
            pI[slot] = make_float4(Ix, Iy, Iz, 1.0f);
            pN[slot] = make_float4(Nx, Ny, Nz, 0.f);
            pD[slot] = make_float4(rp[3], rp[4], rp[5], 0.f);
            go[0] = true; val[0] = slot;
          }
        }
      } else if (next) {
        if constexpr (SPEC) pA[slot] = make_float4(a3[0], a3[1], a3[2], refl);
        else pT[slot] = make_float4(T.x * a3[0], T.y * a3[1], T.z * a3[2], 0.f);
        pI[slot] = make_float4(Ix, Iy, Iz, 1.0f);
        pN[slot] = make_float4(Nx, Ny, Nz, 0.f);
        pD[slot] = make_float4(rp[3], rp[4], rp[5], 0.f);
        go[0] = true; val[0] = slot;
      }
    }
    pL[slot] = L;
  }
  if (next) wg_append<1>(go, val, next, n_next);   // (uniform over the launch)
}

__global__ __launch_bounds__(256) void rt_path_scatter_kernel(SceneDev sc, ShadeParams p, uint32_t cap, const uint32_t* n_live, const uint32_t* __restrict__ live,
    const float* __restrict__ rays, const HitRec* __restrict__ hits, const HitRec* __restrict__ shits,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT,
    uint32_t* __restrict__ next, uint32_t* n_next) {
  path_scatter<0>(sc, p, cap, n_live, live, rays, hits, shits, pI, pN, pD, pL, pT, next, n_next, ScatterNoEmi{});
}

// (the frame with emissive geometry: EMI = 1 for nee = 0, 2 for nee = 1)
template <int EMI>
__global__ __launch_bounds__(256) void rt_path_scatter_emissive_kernel(SceneDev sc, ShadeParams p, uint32_t cap, const uint32_t* n_live, const uint32_t* __restrict__ live,
    const float* __restrict__ rays, const HitRec* __restrict__ hits, const HitRec* __restrict__ shits,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT,
    uint32_t* __restrict__ next, uint32_t* n_next, ScatterEmi em) {
  path_scatter<EMI>(sc, p, cap, n_live, live, rays, hits, shits, pI, pN, pD, pL, pT, next, n_next, em);
}

// (the frame with both estimators weighted, vxrt_render_path_emissive_mis: EMI = 3)
__global__ __launch_bounds__(256) void rt_path_scatter_mis_kernel(SceneDev sc, ShadeParams p, uint32_t cap, const uint32_t* n_live, const uint32_t* __restrict__ live,
    const float* __restrict__ rays, const HitRec* __restrict__ hits, const HitRec* __restrict__ shits,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT,
    uint32_t* __restrict__ next, uint32_t* n_next, ScatterMis em) {
  path_scatter<3>(sc, p, cap, n_live, live, rays, hits, shits, pI, pN, pD, pL, pT, next, n_next, em);
}

// (the frame with specular vertices: EMI as above, 0 for the plain frame)
template <int EMI>
__global__ __launch_bounds__(256) void rt_path_scatter_specular_kernel(SceneDev sc, ShadeParams p, uint32_t cap, const uint32_t* n_live, const uint32_t* __restrict__ live,
    const float* __restrict__ rays, const HitRec* __restrict__ hits, const HitRec* __restrict__ shits,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT, float4* __restrict__ pA,
    uint32_t* __restrict__ next, uint32_t* n_next, std::conditional_t<EMI == 3, ScatterMis, std::conditional_t<EMI != 0, ScatterEmi, ScatterNoEmi>> em) {
  path_scatter<EMI, true>(sc, p, cap, n_live, live, rays, hits, shits, pI, pN, pD, pL, pT, next, n_next, em, pA);
}

// (the depths of a frame with Russian roulette whose hits take a draw: EMI as above; SlotSrc = SlotUniform for the uniform tail,
//  SlotCounts for the counts tail -- the pixel's own count is then the spp of the hash input)
template <int EMI, class SlotSrc>
__global__ __launch_bounds__(256) void rt_path_scatter_roulette_kernel(SceneDev sc, ShadeParams p, uint32_t cap, const uint32_t* n_live, const uint32_t* __restrict__ live,
    const float* __restrict__ rays, const HitRec* __restrict__ hits, const HitRec* __restrict__ shits,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT,
    uint32_t* __restrict__ next, uint32_t* n_next, std::conditional_t<EMI == 3, ScatterMis, std::conditional_t<EMI != 0, ScatterEmi, ScatterNoEmi>> em,
    ScatterRoulette<SlotSrc> rr) {
  path_scatter<EMI, false, true, SlotSrc>(sc, p, cap, n_live, live, rays, hits, shits, pI, pN, pD, pL, pT, next, n_next, em, nullptr, rr);
}

// (the frame lit by an environment map: EMI = 4 for sample = 0, 5 for sample = 1; RR and SlotSrc as for the kernel above -- without
//  roulette the slot source is not read)
template <int EMI, bool RR, class SlotSrc>
__global__ __launch_bounds__(256) void rt_path_scatter_env_kernel(SceneDev sc, ShadeParams p, uint32_t cap, const uint32_t* n_live, const uint32_t* __restrict__ live,
    const float* __restrict__ rays, const HitRec* __restrict__ hits, const HitRec* __restrict__ shits,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT,
    uint32_t* __restrict__ next, uint32_t* n_next, ScatterEnv em, std::conditional_t<RR, ScatterRoulette<SlotSrc>, ScatterNoRoulette> rr) {
  path_scatter<EMI, false, RR, SlotSrc>(sc, p, cap, n_live, live, rays, hits, shits, pI, pN, pD, pL, pT, next, n_next, em, nullptr, rr);
}

// after a batch's last depth: the Lc of its ns samples are added to the pixel's accumulator in ascending s (the frame's first sample
// starts it); one thread per listed pixel
__global__ __launch_bounds__(256) void rt_path_accumulate_kernel(uint32_t n, const uint32_t* __restrict__ list, const uint32_t* __restrict__ hdr, uint32_t ns,
    uint32_t first, const float4* __restrict__ pL, float4* __restrict__ acc) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= min(hdr[0], n)) return;
  const uint32_t t = list[j];
  const float4* L = pL + (size_t)j * ns;
  float4 a = first ? L[0] : acc[t];
  for (uint32_t s = first ? 1u : 0u; s < ns; ++s) { const float4 c = L[s]; a.x = a.x + c.x; a.y = a.y + c.y; a.z = a.z + c.z; }
  acc[t] = a;
}

// colour = acc / spp, pack, write.  flat (bounces = 0): every sample's Lc is the pixel's Lit, summed here the same way.
__global__ __launch_bounds__(256) void rt_path_final_kernel(uint32_t n, uint32_t W, uint32_t y0, const float4* __restrict__ geo, const float4* __restrict__ lit,
    const float4* __restrict__ acc, uint32_t spp, uint32_t flat, uint32_t* __restrict__ dst, float* __restrict__ colors_out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint32_t x = t % W, y = y0 + t / W;
  const size_t e = (size_t)x + (size_t)y * W;
  const float4 c = lit[t];
  float r = c.x, g = c.y, b = c.z;   // (a miss: the background)
  if (geo[t].w != 0.f) {
    if (flat) { for (uint32_t s = 1; s < spp; ++s) { r = r + c.x; g = g + c.y; b = b + c.z; } }
    else { const float4 a = acc[t]; r = a.x; g = a.y; b = a.z; }
    const float f = (float)spp;
    r = r / f; g = g / f; b = b / f;
  }
  dst[e] = pack_rgb8(r, g, b);
  if (colors_out) { colors_out[3 * e] = r; colors_out[3 * e + 1] = g; colors_out[3 * e + 2] = b; }
}

// ---------------------------------------------------------------------------------------------
// Path frames with a sample count per pixel (vxrt_render_path_adaptive; the definition is the header's "Adaptive sampling", the launch
// sequence is in render_path_counts_tail and DESIGN.md s2 "Adaptive sampling").  The paths of the frame are numbered in window order:
// pixel t owns the cnt[t] paths g = off[t] .. off[t] + cnt[t] - 1, sample g - off[t]; batch b owns g in [b * cap, (b + 1) * cap), slot
// g - b * cap.  The numbering comes from a scan in window order, so it is the same from run to run (the atomic-ordered list of hit
// pixels is not).  The scan is three launches and no workgroup waits for another: per-block sums, one workgroup that scans the block
// sums in passes with a running carry, per-pixel offsets.  rt_path_prepare_kernel, rt_path_occlusion_rays_kernel and
// rt_path_scatter_kernel are the uniform frame's: they work on slots and live lists only.
// ---------------------------------------------------------------------------------------------
#define PT_SCAN_BLOCK 1024u   // pixels per scan block: 256 threads x 4 consecutive pixels
#define PT_SCAN_PASS 1024u    // block sums per pass of rt_path_scan_kernel: its threads (one pass covers PT_SCAN_PASS * PT_SCAN_BLOCK pixels)

// cnt[t] = clamp(counts[pixel of t], 1, spp_cap) for a pixel with a hit, 0 for a miss (its count is not read); bsum[block] = the sum of
// the block's cnt (at most 1,024 x 4,096)
__global__ __launch_bounds__(256) void rt_path_counts_kernel(uint32_t n, uint32_t W, uint32_t y0, uint32_t spp_cap, const float4* __restrict__ geo,
    const uint32_t* __restrict__ counts, uint32_t* __restrict__ cnt, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t s_w[4];
  const uint32_t t0 = blockIdx.x * PT_SCAN_BLOCK + threadIdx.x * 4u;
  uint32_t sum = 0u;
#pragma unroll
  for (uint32_t c = 0; c < 4u; ++c) {
    const uint32_t t = t0 + c;
    if (t < n) {
      uint32_t v = 0u;
      if (geo[t].w != 0.f) {
        const uint32_t x = t % W, y = y0 + t / W;
        v = min(max(counts[(size_t)x + (size_t)y * W], 1u), spp_cap);
      }
      cnt[t] = v;
      sum += v;
    }
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// boff[i] = the sum of bsum[0 .. i), 64 bit; *total = the sum of all nb.  ONE workgroup: pass k scans block sums [k * PT_SCAN_PASS,
// (k + 1) * PT_SCAN_PASS) and every thread carries the running total into the next pass; the number of passes is known at entry.
__global__ __launch_bounds__(1024) void rt_path_scan_kernel(uint32_t nb, const uint32_t* __restrict__ bsum, unsigned long long* __restrict__ boff,
    unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_w[PT_SCAN_PASS / 64u];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t passes = (nb + PT_SCAN_PASS - 1u) / PT_SCAN_PASS;
  unsigned long long carry = 0ull;
  for (uint32_t k = 0; k < passes; ++k) {
    const uint32_t i = k * PT_SCAN_PASS + threadIdx.x;
    const unsigned long long v = i < nb ? (unsigned long long)bsum[i] : 0ull;
    unsigned long long inc = v;
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += y; }
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    unsigned long long base = carry, pass_sum = 0ull;
    for (uint32_t w = 0; w < PT_SCAN_PASS / 64u; ++w) { const unsigned long long x = s_w[w]; if (w < wave) base += x; pass_sum += x; }
    if (i < nb) boff[i] = base + (inc - v);
    carry += pass_sum;
    __syncthreads();   // (s_w is written again by the next pass)
  }
  if (threadIdx.x == 0) *total = carry;
}

// off[t] = boff[block of t] + the sum of cnt over the block's pixels before t
__global__ __launch_bounds__(256) void rt_path_offsets_kernel(uint32_t n, const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ boff,
    unsigned long long* __restrict__ off) {
  __shared__ uint32_t s_w[4];
  const uint32_t t0 = blockIdx.x * PT_SCAN_BLOCK + threadIdx.x * 4u;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t v[4], sum = 0u;
#pragma unroll
  for (uint32_t c = 0; c < 4u; ++c) { v[c] = t0 + c < n ? cnt[t0 + c] : 0u; sum += v[c]; }
  uint32_t inc = sum;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += y; }
  if (lane == 63u) s_w[wave] = inc;
  __syncthreads();
  unsigned long long base = boff[blockIdx.x] + (unsigned long long)(inc - sum);
  for (uint32_t w = 0; w < wave; ++w) base += s_w[w];
#pragma unroll
  for (uint32_t c = 0; c < 4u; ++c) {
    if (t0 + c < n) off[t0 + c] = base;
    base += v[c];
  }
}

// start of the batch that owns paths [g0, g0 + cap): slot i is path g = g0 + i, live while g < *total.  Its pixel is the last t with
// off[t] <= g -- a pixel without samples shares its offset with its successor, so that t has samples -- found by a binary search of at
// most 32 steps (n < 2^31); the slot keeps (pixel, sample) and takes the pixel's primary vertex as rt_path_start_kernel does.
// hdr[1] = the batch's live paths (0 for a batch past the end of the frame's paths).
__global__ __launch_bounds__(256) void rt_path_start_counts_kernel(uint32_t cap, unsigned long long g0, uint32_t n, const unsigned long long* __restrict__ total,
    const unsigned long long* __restrict__ off, uint32_t* hdr,
    const float4* __restrict__ geo, const float4* __restrict__ nrm, const float4* __restrict__ dir, const float4* __restrict__ lit, const float4* __restrict__ alb,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT, uint32_t* __restrict__ live,
    uint32_t* __restrict__ spix, uint32_t* __restrict__ ssmp) {
  const unsigned long long tot = *total;
  const unsigned long long left = tot > g0 ? tot - g0 : 0ull;
  const uint32_t n_live = left < (unsigned long long)cap ? (uint32_t)left : cap;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) hdr[1] = n_live;
  if (i >= n_live) return;
  const unsigned long long g = g0 + i;
  uint32_t lo = 0u, hi = n;   // off[lo] <= g < off[hi] (off[n] = *total)
  for (int k = 0; k < 32; ++k) {
    if (hi - lo <= 1u) break;
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  const uint32_t t = lo;
  spix[i] = t; ssmp[i] = (uint32_t)(g - off[t]);
  pI[i] = geo[t]; pN[i] = nrm[t]; pD[i] = dir[t]; pL[i] = lit[t]; pT[i] = alb[t];
  live[i] = i;
}

// (the frame with specular vertices: thr = 1 and pA = (Alb, reflectivity) of the primary vertex, as rt_path_start_specular_kernel)
__global__ __launch_bounds__(256) void rt_path_start_counts_specular_kernel(uint32_t cap, unsigned long long g0, uint32_t n, const unsigned long long* __restrict__ total,
    const unsigned long long* __restrict__ off, uint32_t* hdr,
    const float4* __restrict__ geo, const float4* __restrict__ nrm, const float4* __restrict__ dir, const float4* __restrict__ lit, const float4* __restrict__ alb,
    float4* __restrict__ pI, float4* __restrict__ pN, float4* __restrict__ pD, float4* __restrict__ pL, float4* __restrict__ pT, float4* __restrict__ pA, uint32_t* __restrict__ live,
    uint32_t* __restrict__ spix, uint32_t* __restrict__ ssmp) {
  const unsigned long long tot = *total;
  const unsigned long long left = tot > g0 ? tot - g0 : 0ull;
  const uint32_t n_live = left < (unsigned long long)cap ? (uint32_t)left : cap;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) hdr[1] = n_live;
  if (i >= n_live) return;
  const unsigned long long g = g0 + i;
  uint32_t lo = 0u, hi = n;   // off[lo] <= g < off[hi] (off[n] = *total)
  for (int k = 0; k < 32; ++k) {
    if (hi - lo <= 1u) break;
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  const uint32_t t = lo;
  spix[i] = t; ssmp[i] = (uint32_t)(g - off[t]);
  pI[i] = geo[t]; pN[i] = nrm[t]; pD[i] = dir[t]; pL[i] = lit[t]; pT[i] = make_float4(1.f, 1.f, 1.f, 0.f); pA[i] = alb[t];
  live[i] = i;
}

// rt_path_bounce_rays_kernel with the slot's pixel, sample and the pixel's own sample count in place of slot / ns, s0 + slot % ns and spp
__global__ __launch_bounds__(256) void rt_path_bounce_rays_counts_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t user_seed,
    const uint32_t* __restrict__ spix, const uint32_t* __restrict__ ssmp, const uint32_t* __restrict__ cnt,
    const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, unsigned long long* rays_traced) {
  const uint32_t total = min(*n_live, cap);
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q == 0) {
    *n_next = 0u;
    if (rays_traced && total) atomicAdd(rays_traced, (unsigned long long)total);   // (every live path traces one)
  }
  if (q >= total) return;
  const uint32_t slot = live[q], t = spix[slot], smp = ssmp[slot];
  const uint32_t x = t % W, y = y0 + t / W;
  const float4 I = pI[slot], N = pN[slot], D = pD[slot];
  float r6[6];
  ao_sample_ray(x, y, W, cnt[t], smp, user_seed, I.x, I.y, I.z, N.x, N.y, N.z, D.x, D.y, D.z, r6);
  float* o = rays + (size_t)q * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = r6[k];
}

// rt_path_bounce_emitter_rays_kernel / its MIS twin with the slot's pixel, sample and the pixel's own sample count, as the kernel above
// reads them: the emitter ray's hash input is (x + y * W) * n_p + s + 1 + u * 0x9E3779B9.  The body is path_bounce_emitter_rays, which
// no thread leaves early -- unlike the kernel above, it ends in a barrier and one count per workgroup.
__global__ __launch_bounds__(256) void rt_path_bounce_emitter_rays_counts_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t user_seed,
    const uint32_t* __restrict__ spix, const uint32_t* __restrict__ ssmp, const uint32_t* __restrict__ cnt,
    const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, EmitterTab tab, float scale,
    float* __restrict__ erays, float* __restrict__ etmax, float4* __restrict__ eG, unsigned long long* rays_traced) {
  path_bounce_emitter_rays<false>(cap, W, y0, SlotCounts{spix, ssmp, cnt}, user_seed, live, n_live, n_next, pI, pN, pD, rays, tab, scale, erays, etmax, eG, rays_traced);
}

__global__ __launch_bounds__(256) void rt_path_bounce_emitter_rays_counts_mis_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t user_seed,
    const uint32_t* __restrict__ spix, const uint32_t* __restrict__ ssmp, const uint32_t* __restrict__ cnt,
    const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, EmitterTab tab, float scale,
    float* __restrict__ erays, float* __restrict__ etmax, float4* __restrict__ eG, unsigned long long* rays_traced) {
  path_bounce_emitter_rays<true>(cap, W, y0, SlotCounts{spix, ssmp, cnt}, user_seed, live, n_live, n_next, pI, pN, pD, rays, tab, scale, erays, etmax, eG, rays_traced);
}

// (rt_path_bounce_env_rays_kernel likewise: the environment ray's hash input takes the pixel's own n_p)
__global__ __launch_bounds__(256) void rt_path_bounce_env_rays_counts_kernel(uint32_t cap, uint32_t W, uint32_t y0, uint32_t user_seed,
    const uint32_t* __restrict__ spix, const uint32_t* __restrict__ ssmp, const uint32_t* __restrict__ cnt,
    const uint32_t* __restrict__ live, const uint32_t* n_live, uint32_t* n_next,
    const float4* __restrict__ pI, const float4* __restrict__ pN, const float4* __restrict__ pD, float* __restrict__ rays, EnvTab env,
    float* __restrict__ erays, float* __restrict__ etmax, float4* __restrict__ eG, unsigned long long* rays_traced) {
  path_bounce_env_rays(cap, W, y0, SlotCounts{spix, ssmp, cnt}, user_seed, live, n_live, n_next, pI, pN, pD, rays, env, erays, etmax, eG, rays_traced);
}

// after a batch's last depth, one thread per pixel of the window: the Lc of the pixel's samples that are in the batch [g0, g0 + cap)
// are added to its accumulator in ascending sample order; the pixel's first sample starts it.  A pixel's samples are contiguous in g
// and may straddle batches; the trip count is at most the pixel's count.
__global__ __launch_bounds__(256) void rt_path_accumulate_counts_kernel(uint32_t n, uint32_t cap, unsigned long long g0, const uint32_t* __restrict__ cnt,
    const unsigned long long* __restrict__ off, const float4* __restrict__ pL, float4* __restrict__ acc) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint32_t c = cnt[t];
  if (c == 0u) return;
  const unsigned long long o = off[t], g1 = g0 + cap;
  const unsigned long long lo = o > g0 ? o : g0, hi = o + c < g1 ? o + c : g1;
  if (lo >= hi) return;
  const float4* L = pL + (size_t)(lo - g0);
  const uint32_t k = (uint32_t)(hi - lo);
  const bool first = lo == o;
  float4 a = first ? L[0] : acc[t];
  for (uint32_t s = first ? 1u : 0u; s < k; ++s) { const float4 v = L[s]; a.x = a.x + v.x; a.y = a.y + v.y; a.z = a.z + v.z; }
  acc[t] = a;
}

// after the last batch: acc[t] = acc[t] / (float)cnt[t] per channel (flat, bounces = 0: of the flat sum of Lit_0, formed here as
// rt_path_final_kernel forms it).  What ends the frame then divides by 1.0f, which changes no bit.
__global__ __launch_bounds__(256) void rt_path_divide_counts_kernel(uint32_t n, const uint32_t* __restrict__ cnt, const float4* __restrict__ lit, uint32_t flat,
    float4* __restrict__ acc) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint32_t c = cnt[t];
  if (c == 0u) return;
  float r, g, b;
  if (flat) { const float4 l = lit[t]; r = l.x; g = l.y; b = l.z; for (uint32_t s = 1; s < c; ++s) { r = r + l.x; g = g + l.y; b = b + l.z; } }
  else { const float4 a = acc[t]; r = a.x; g = a.y; b = a.z; }
  const float f = (float)c;
  acc[t] = make_float4(r / f, g / f, b / f, 0.f);
}

// vxrt_sample_counts (the header's "Adaptive sampling"): one entry per thread, every symbol one fp32 operation; the counts written are
// summed per workgroup (at most 256 x 4,096) and added to *total with one 64-bit atomic
__global__ __launch_bounds__(256) void rt_sample_counts_kernel(uint32_t n, const float* __restrict__ variance, const uint32_t* __restrict__ prev, float gain,
    uint32_t min_spp, uint32_t max_spp, uint32_t* __restrict__ counts, unsigned long long* total) {
  __shared__ uint32_t s_w[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t v = 0u;
  if (i < n) {
    const float m = prev ? (float)min(max(prev[i], 1u), 4096u) : 1.0f;
    const float x = (variance[i] * m) * gain;
    const float c = ceilf(x);
    v = c > (float)min_spp ? (c < (float)max_spp ? (uint32_t)c : max_spp) : min_spp;
    counts[i] = v;
  }
  if (total) {   // (uniform over the launch)
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t sum = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
      if (sum) atomicAdd(total, (unsigned long long)sum);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host: the tail render_common (rt_kernels.hip) ends a path frame with
// ---------------------------------------------------------------------------------------------
#include <algorithm>
#include <cmath>

// Paths per batch of a path frame (VXRT_PATH_BATCH).  A path costs 136 bytes of frame-context storage -- 80 of state (I, N, dir, Lc, thr:
// five float4), 24 + 24 of bounce ray and hit record, 2 x 4 of live-list entries -- and 52 more with light sampling (occlusion ray, tmax,
// hit record): 4 Mi paths are 0.53 / 0.73 GiB per frame context, and at 1920x1080 two samples per batch, i.e. ray-buffer launches of up to
// 4 M rays for a machine that holds 0.4 M lanes of the traversal kernel -- launch ramps and tails stay a small part of each.
extern const uint64_t PATH_BATCH_PATHS = 4ull << 20;   // (secondary_knobs, rt_secondary.hip, reads it as VXRT_PATH_BATCH's default)

// What picks the kernels of a path frame, resolved from the request once (render_path_tail) and read by every launch site below.
// emi, the emitter form (the header's "Emissive geometry"): 0 none, 1 emission at bounce hits, 2 emitter sampling -- one emitter ray per
// live path and depth, generated with the bounce ray and traced by a second any-hit launch -- 3, the header's "Multiple importance
// sampling": the launches of 2 with the weighted kernels, whose scatter looks emissive hits up in the emitter index.  scale: that
// form's, 0 without one.  spec: specular vertices; counts: a sample count per pixel; shadow: light sampling; cam: a camera frame.
// roulette (the header's "Russian roulette"): vertices rr_first .. bounces - 1 take a draw with floor q_min; never with spec.
// env (the header's "Environment light"): 0 none, 1 the map is seen by rays that miss (sample = 0), 2 and sampled -- the launches of
// emi = 2 with the environment kernels (sample = 1); never with an emitter form or spec.  map: what the kernels read of it, with the scale.
struct PathForm { int emi; float scale; bool spec, counts, shadow, motion, cam, roulette; uint32_t rr_first; float q_min; int env; EnvTab map; };
static PathForm path_form(const RenderRequest& r) {
  PathForm f;
  f.emi = r.emissive_mis ? 3 : r.emissive ? (r.emissive->nee ? 2 : 1) : 0;
  f.scale = r.emissive_mis ? r.emissive_mis->scale : r.emissive ? r.emissive->scale : 0.0f;
  f.spec = r.specular != nullptr; f.counts = r.sample_counts != nullptr; f.shadow = r.path->shadow != 0; f.motion = r.motion; f.cam = r.cams != nullptr;
  f.roulette = r.roulette != nullptr; f.rr_first = r.roulette ? r.roulette->first : 0u; f.q_min = r.roulette ? r.roulette->q_min : 0.0f;
  f.env = r.env ? (r.env->sample ? 2 : 1) : 0;
  f.map = r.env ? env_tab(r.env->map, r.env->scale) : EnvTab{nullptr, nullptr, nullptr, 0u, 0u, 0.0f};
  return f;
}

// What the kernels of an emitter form take besides, built once per frame behind path_tail_begin (which grows the buffers named here and
// has the index built): rays for the bounce-ray kernels of emi >= 2, hits / weighted for the scatter kernels of emi 1, 2 / 3
struct PathEmitters { SpecEm rays; ScatterEmi hits; ScatterMis weighted; ScatterEnv env; };
static PathEmitters path_emitters(const vxrt_accel* a, const FrameCtx* c, const PathForm& f) {
  return PathEmitters{SpecEm{emitter_tab(a), f.scale, c->pt_erays, c->pt_etmax, c->pt_eG},
                      ScatterEmi{f.scale, (const HitRec*)c->pt_ehits, (const float4*)c->pt_eG},
                      ScatterMis{f.scale, (const HitRec*)c->pt_ehits, (const float4*)c->pt_eG, emitter_tab(a), emitter_idx(a)},
                      ScatterEnv{(const HitRec*)c->pt_ehits, (const float4*)c->pt_eG, f.map}};
}

// The prepare launch of a path frame over the n pixels of its window: which instantiation the form takes, and what that one takes
// besides the arguments all of them share
static void path_prepare_launch(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const PathForm& f, const ShadeParams& p, const float* utab, const float* vtab, uint32_t n) {
  const auto launch = [&](auto kernel, auto... flavour) {
    hipLaunchKernelGGL(kernel, dim3((n + 256u * PREP_CHUNKS - 1u) / (256u * PREP_CHUNKS)), dim3(256), 0, (hipStream_t)r.stream, a->dev, p, n, r.width, r.y0, utab, vtab,
                       (const HitRec*)c->hitbuf, c->pt_geo, c->pt_nrm, c->pt_dir, c->pt_lit, c->pt_alb, c->pt_list, c->pt_hdr, c->ctl, flavour...);
  };
  const PrepMotion mo{motion_src(a), c->mo_pos, c->mo_nrm, r.prev_position};   // (read by the flavours with motion: camera frames, check_request)
  const bool emi = f.emi != 0;
  if (f.spec)   // (no motion: check_request.  `scale` is read by the emissive flavour only; the last argument is bounces > 0)
    launch(f.cam ? (emi ? rt_path_prepare_specular_kernel<true, true> : rt_path_prepare_specular_kernel<true, false>)
                 : (emi ? rt_path_prepare_specular_kernel<false, true> : rt_path_prepare_specular_kernel<false, false>), f.scale, r.path->bounces ? 1u : 0u);
  else if (f.env && f.motion) launch(rt_path_prepare_env_kernel<true, true>, mo, f.map);
  else if (f.env) launch(f.cam ? rt_path_prepare_env_kernel<true, false> : rt_path_prepare_env_kernel<false, false>, PrepNoMotion{}, f.map);
  else if (emi && f.motion) launch(rt_path_prepare_emissive_motion_kernel, mo, f.scale);
  else if (emi) launch(f.cam ? rt_path_prepare_emissive_kernel<true> : rt_path_prepare_emissive_kernel<false>, f.scale);
  else if (f.motion) launch(rt_path_prepare_kernel<true, true>, mo);
  else launch(f.cam ? rt_path_prepare_kernel<true> : rt_path_prepare_kernel<false>, PrepNoMotion{});
}

// What both tails of a path frame begin with: the emitter index of emi = 3, built if the accel holds none (a buffer that grows, with the
// one synchronisation that takes); the context's buffers for n pixels and batches of path_cap paths (per emitter ray -- emi >= 2; per
// pixel; per path -- none without bounces; per occlusion ray -- none without light sampling; grown behind the stream); the zeroed header,
// and the prepare launch
static int path_tail_begin(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const PathForm& f, const ShadeParams& p, const float* utab, const float* vtab, uint64_t n,
                           uint64_t path_cap) {
  hipStream_t s = (hipStream_t)r.stream;
  const uint64_t shadow_cap = f.shadow ? path_cap : 0;
  if (f.emi == 3 && emitter_index_ensure(a, s) != 0) return -1;
  if ((f.emi >= 2 || f.env == 2) && !grow_device({{(void**)&c->pt_erays, 24}, {(void**)&c->pt_etmax, 4}, {(void**)&c->pt_ehits, sizeof(HitRec)}, {(void**)&c->pt_eG, 16}}, &c->pt_em_cap,
                                 path_cap, GrowSync::STREAM, s)) return -1;
  if (!c->pt_hdr && hipMalloc((void**)&c->pt_hdr, 16) != hipSuccess) return -1;
  if (!grow_device({{(void**)&c->pt_geo, 16}, {(void**)&c->pt_nrm, 16}, {(void**)&c->pt_dir, 16}, {(void**)&c->pt_lit, 16}, {(void**)&c->pt_alb, 16},
                    {(void**)&c->pt_acc, 16}, {(void**)&c->pt_list, 4}}, &c->pt_cap, n, GrowSync::STREAM, s)) return -1;
  if (!grow_device({{(void**)&c->pt_I, 16}, {(void**)&c->pt_N, 16}, {(void**)&c->pt_D, 16}, {(void**)&c->pt_L, 16}, {(void**)&c->pt_T, 16}, {(void**)&c->pt_live[0], 4},
                    {(void**)&c->pt_live[1], 4}, {(void**)&c->pt_rays, 24}, {(void**)&c->pt_hits, sizeof(HitRec)}}, &c->pt_path_cap, path_cap, GrowSync::STREAM, s)) return -1;
  if (!grow_device({{(void**)&c->pt_srays, 24}, {(void**)&c->pt_stmax, 4}, {(void**)&c->pt_shits, sizeof(HitRec)}}, &c->pt_shadow_cap, shadow_cap, GrowSync::STREAM, s)) return -1;
  if (f.spec && !grow_device({{(void**)&c->pt_A, 16}}, &c->pt_spec_cap, path_cap, GrowSync::STREAM, s)) return -1;
  if (f.motion && !grow_device({{(void**)&c->mo_pos, 16}, {(void**)&c->mo_nrm, 16}}, &c->mo_cap, n, GrowSync::STREAM, s)) return -1;
  if (hipMemsetAsync(c->pt_hdr, 0, 16, s) != hipSuccess) return -1;
  path_prepare_launch(a, c, r, f, p, utab, vtab, (uint32_t)n);
  if (hipGetLastError() != hipSuccess) return -1;
  c->ctl_dirty = false;
  return 0;
}

// The depths of one batch of at most cap paths, started in c->pt_live[0] with their number in c->pt_hdr[1].  Per depth: bounce rays of
// the live paths -> closest-hit launch -> (light sampling: occlusion rays -> any-hit launch) -> (emi >= 2: the any-hit launch of the
// emitter rays the bounce-ray kernel wrote) -> scatter, which compacts the paths that go on into the next depth's list.
// bounce_rays(d, live, n_live, n_next) launches the tail's bounce-ray kernel for depth d; n_rays is the batch's ray count as
// trace_on_ctx sizes its launch (the live count is read on the device).  slots: the tail's slot source, which the scatter step of a
// depth with Russian roulette reads for its draw -- the hit of depth d is vertex d + 1, and it draws iff rr_first <= d + 1 < bounces;
// every other depth of such a frame takes the scatter kernel it always took.
template <class SlotSrc, class BounceRays>
static int path_batch_depths(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const PathForm& f, const PathEmitters& E, const ShadeParams& p, uint32_t cap,
                             uint64_t n_rays, const SlotSrc& slots, const BounceRays& bounce_rays) {
  hipStream_t s = (hipStream_t)r.stream;
  const dim3 block(256), rgrid((cap + 255u) / 256u);
  const uint32_t bounces = r.path->bounces;
  const HitRec* shits = f.shadow ? (const HitRec*)c->pt_shits : (const HitRec*)nullptr;
  for (uint32_t d = 0; d < bounces; ++d) {
    uint32_t* n_live = c->pt_hdr + 1 + (d & 1u);
    uint32_t* n_next = c->pt_hdr + 1 + ((d + 1u) & 1u);
    const uint32_t* live = c->pt_live[d & 1u];
    uint32_t* next = d + 1u < bounces ? c->pt_live[(d + 1u) & 1u] : (uint32_t*)nullptr;
    bounce_rays(d, live, (const uint32_t*)n_live, n_next);
    if (trace_on_ctx(a, c, c->pt_rays, n_rays, nullptr, c->pt_hits, VXRT_MODE_CLOSEST, s, n_live) != 0) return -1;
    if (f.shadow) {
      hipLaunchKernelGGL(rt_path_occlusion_rays_kernel, rgrid, block, 0, s, p, cap, (const uint32_t*)n_live, (const float*)c->pt_rays, (const HitRec*)c->pt_hits,
                         c->pt_srays, c->pt_stmax, r.counters);
      if (trace_on_ctx(a, c, c->pt_srays, n_rays, c->pt_stmax, c->pt_shits, MODE_ANY_UNORDERED, s, n_live) != 0) return -1;
    }
    if ((f.emi >= 2 || f.env == 2) && trace_on_ctx(a, c, c->pt_erays, n_rays, c->pt_etmax, c->pt_ehits, MODE_ANY_UNORDERED, s, n_live) != 0) return -1;
    // (the specular instantiations: the same launch, per-slot Alb and reflectivity besides)
    const auto scatter = [&](auto kernel, auto... rest) {
      hipLaunchKernelGGL(kernel, rgrid, block, 0, s, a->dev, p, cap, (const uint32_t*)n_live, live, (const float*)c->pt_rays, (const HitRec*)c->pt_hits, shits,
                         c->pt_I, c->pt_N, c->pt_D, c->pt_L, c->pt_T, rest...);
    };
    if (f.roulette && next && d + 1u >= f.rr_first) {
      const ScatterRoulette<SlotSrc> rr{slots, r.width, r.y0, r.path->seed + d, f.q_min};
      if (f.env) scatter(f.env == 2 ? rt_path_scatter_env_kernel<5, true, SlotSrc> : rt_path_scatter_env_kernel<4, true, SlotSrc>, next, n_next, E.env, rr);
      else if (f.emi == 3) scatter(rt_path_scatter_roulette_kernel<3, SlotSrc>, next, n_next, E.weighted, rr);
      else if (f.emi == 2) scatter(rt_path_scatter_roulette_kernel<2, SlotSrc>, next, n_next, E.hits, rr);
      else if (f.emi == 1) scatter(rt_path_scatter_roulette_kernel<1, SlotSrc>, next, n_next, E.hits, rr);
      else scatter(rt_path_scatter_roulette_kernel<0, SlotSrc>, next, n_next, ScatterNoEmi{}, rr);
    } else if (f.env) scatter(f.env == 2 ? rt_path_scatter_env_kernel<5, false, SlotUniform> : rt_path_scatter_env_kernel<4, false, SlotUniform>, next, n_next, E.env,
                              ScatterNoRoulette{});   // (no draw: the slot source is not read, one instantiation serves both tails)
    else if (f.spec && f.emi == 3) scatter(rt_path_scatter_specular_kernel<3>, c->pt_A, next, n_next, E.weighted);
    else if (f.spec && f.emi == 2) scatter(rt_path_scatter_specular_kernel<2>, c->pt_A, next, n_next, E.hits);
    else if (f.spec && f.emi == 1) scatter(rt_path_scatter_specular_kernel<1>, c->pt_A, next, n_next, E.hits);
    else if (f.spec) scatter(rt_path_scatter_specular_kernel<0>, c->pt_A, next, n_next, ScatterNoEmi{});
    else if (f.emi == 3) scatter(rt_path_scatter_mis_kernel, next, n_next, E.weighted);
    else if (f.emi) scatter(f.emi == 2 ? rt_path_scatter_emissive_kernel<2> : rt_path_scatter_emissive_kernel<1>, next, n_next, E.hits);
    else scatter(rt_path_scatter_kernel, next, n_next);
  }
  return 0;
}

// What ends a path frame whose accumulators are filled: colour = acc / spp (flat, bounces = 0: the flat sum of Lit_0 instead).  A
// denoised frame with iterations or a history ends in rt_denoise.hip instead (render_denoise_tail: demodulate, temporal step, initial
// variance, a-trous passes -- that unit owns the order); one without either gets its guide outputs there and ends here as every path frame.
static int path_frame_end(FrameCtx* c, const RenderRequest& r, uint32_t n, uint32_t spp, uint32_t flat) {
  if (r.denoise && (r.denoise->iterations || r.temporal)) return render_denoise_tail(c, r, n);
  if (r.denoise && r.aov && render_denoise_aov(c, r, n) != 0) return -1;   // (no iterations: the guide outputs, then the path frame's own end)
  hipLaunchKernelGGL(rt_path_final_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)r.stream, n, r.width, r.y0, (const float4*)c->pt_geo, (const float4*)c->pt_lit,
                     (const float4*)c->pt_acc, spp, flat, r.dst, r.colors);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Tail of a path frame with one sample count for the window.  Prepare the per-pixel state and the list of hit pixels; then, in batches
// of whole samples (clamp(VXRT_PATH_BATCH / pixels of the window, 1, spp) samples each), per depth: bounce rays of the live paths ->
// closest-hit launch -> (light sampling: occlusion rays -> any-hit launch) -> scatter, which compacts the paths that go on into the next
// depth's list; after the last depth the batch's Lc go into the pixels' accumulators in ascending sample order; at the end divide, pack,
// write.  Every count stays on the device (the launches are sized for the batch's capacity and read the live count): no host
// synchronisation unless a buffer grows.  The depths are path_batch_depths, the end is path_frame_end.
static int render_path_uniform_tail(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const PathForm& f, const ShadeParams& p, const float* utab, const float* vtab) {
  const vxrt_path_params_t& pp = *r.path;
  const uint32_t width = r.width, y0 = r.y0, y1 = r.y1;
  hipStream_t s = (hipStream_t)r.stream;
  const uint64_t n = (uint64_t)width * (y1 - y0);
  if (n > 0x7fffffffull) return -1;
  const uint32_t ns = (uint32_t)std::min<uint64_t>(pp.spp, std::max<uint64_t>(1, secondary_knobs().path_batch / n));   // samples per batch
  const uint64_t path_cap = pp.bounces ? n * ns : 0;
  if (path_cap > 0x7fffffffull) return -1;
  if (path_tail_begin(a, c, r, f, p, utab, vtab, n, path_cap) != 0) return -1;
  const PathEmitters E = path_emitters(a, c, f);
  const uint32_t n32 = (uint32_t)n, cap = (uint32_t)path_cap;
  const dim3 block(256), grid((n32 + 255u) / 256u), rgrid((cap + 255u) / 256u);
  for (uint32_t s0 = 0; pp.bounces && s0 < pp.spp; s0 += ns) {
    const uint32_t k = std::min(ns, pp.spp - s0);   // samples of this batch
    const auto start = [&](auto kernel, auto... rest) {
      hipLaunchKernelGGL(kernel, rgrid, block, 0, s, cap, k, (const uint32_t*)c->pt_list, c->pt_hdr, (const float4*)c->pt_geo, (const float4*)c->pt_nrm,
                         (const float4*)c->pt_dir, (const float4*)c->pt_lit, (const float4*)c->pt_alb, c->pt_I, c->pt_N, c->pt_D, c->pt_L, c->pt_T, rest...);
    };
    if (f.spec) start(rt_path_start_specular_kernel, c->pt_A, c->pt_live[0]);
    else start(rt_path_start_kernel, c->pt_live[0]);
    // slot -> (pixel, sample) through (s0, k).  Specular: the pick, then the mirror or the diffuse ray, and the emitter ray of a vertex
    // that picks diffuse; emi >= 2: the kernel that writes the emitter ray of the same vertex as well
    const auto bounce_rays = [&](uint32_t d, const uint32_t* live, const uint32_t* n_live, uint32_t* n_next) {
      const auto launch = [&](auto kernel, auto... rest) {
        hipLaunchKernelGGL(kernel, rgrid, block, 0, s, cap, width, y0, pp.spp, s0, k, pp.seed + d, (const uint32_t*)c->pt_list, live, n_live, n_next,
                           (const float4*)c->pt_I, (const float4*)c->pt_N, rest..., r.counters);
      };
      const SpecEm& e = E.rays;
      if (f.spec && f.emi == 3) launch(rt_path_bounce_specular_kernel<2>, c->pt_D, c->pt_T, (const float4*)c->pt_A, c->pt_rays, e);
      else if (f.spec && f.emi == 2) launch(rt_path_bounce_specular_kernel<1>, c->pt_D, c->pt_T, (const float4*)c->pt_A, c->pt_rays, e);
      else if (f.spec) launch(rt_path_bounce_specular_kernel<0>, c->pt_D, c->pt_T, (const float4*)c->pt_A, c->pt_rays, SpecNoEm{});
      else if (f.emi >= 2) launch(f.emi == 3 ? rt_path_bounce_emitter_rays_mis_kernel : rt_path_bounce_emitter_rays_kernel, (const float4*)c->pt_D, c->pt_rays,
                                  e.tab, e.scale, e.erays, e.etmax, e.eG);
      else if (f.env == 2) launch(rt_path_bounce_env_rays_kernel, (const float4*)c->pt_D, c->pt_rays, f.map, e.erays, e.etmax, e.eG);
      else launch(rt_path_bounce_rays_kernel, (const float4*)c->pt_D, c->pt_rays);
    };
    if (path_batch_depths(a, c, r, f, E, p, cap, (uint64_t)n * k, SlotUniform{pp.spp, s0, k, c->pt_list}, bounce_rays) != 0) return -1;
    hipLaunchKernelGGL(rt_path_accumulate_kernel, grid, block, 0, s, n32, (const uint32_t*)c->pt_list, (const uint32_t*)c->pt_hdr, k, s0 == 0 ? 1u : 0u,
                       (const float4*)c->pt_L, c->pt_acc);
  }
  return path_frame_end(c, r, n32, pp.spp, pp.bounces == 0 ? 1u : 0u);
}

// Tail of a path frame with a sample count per pixel (r.sample_counts; path->spp is the cap).  The prepare launch of every path frame;
// then the clamped counts and their scan in window order (three launches: block sums, one workgroup over the block sums, per-pixel
// offsets); then batches of cap = clamp(VXRT_PATH_BATCH, 1, pixels * spp) consecutive paths, each the depths of the tail above
// (path_batch_depths) with the kernels that read a slot's pixel and sample from the slot; after the last batch the accumulators are divided by their
// pixel's count and the frame ends as every path frame, with spp = 1.  The number of paths stays on the device, so the host issues
// ceil(pixels * spp / cap) batches whatever the counts: a batch past the end starts with zero live paths and its launches fall through.
// Storage per path is bounded by cap, the emitter rays of a batch with it.  No host synchronisation unless a buffer grows.
static int render_path_counts_tail(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const PathForm& f, const ShadeParams& p, const float* utab, const float* vtab) {
  const vxrt_path_params_t& pp = *r.path;
  const uint32_t width = r.width, y0 = r.y0, y1 = r.y1;
  hipStream_t s = (hipStream_t)r.stream;
  const uint64_t n = (uint64_t)width * (y1 - y0);
  if (n > 0x7fffffffull) return -1;
  const uint64_t all = n * pp.spp;   // (the most paths the counts can ask for)
  const uint64_t batch = std::min<uint64_t>(std::max<uint64_t>(1, secondary_knobs().path_batch), all);
  if (batch > 0x7fffffffull) return -1;
  const uint64_t path_cap = pp.bounces ? batch : 0;
  const uint64_t n_blocks = (n + PT_SCAN_BLOCK - 1u) / PT_SCAN_BLOCK;
  if (!c->pt_ctot && hipMalloc((void**)&c->pt_ctot, 8) != hipSuccess) return -1;
  if (!grow_device({{(void**)&c->pt_cnt, 4}, {(void**)&c->pt_off, 8}}, &c->pt_cnt_cap, n, GrowSync::STREAM, s)) return -1;
  if (!grow_device({{(void**)&c->pt_bsum, 4}, {(void**)&c->pt_boff, 8}}, &c->pt_blk_cap, n_blocks, GrowSync::STREAM, s)) return -1;
  if (!grow_device({{(void**)&c->pt_spix, 4}, {(void**)&c->pt_ssmp, 4}}, &c->pt_slot_cap, path_cap, GrowSync::STREAM, s)) return -1;
  if (path_tail_begin(a, c, r, f, p, utab, vtab, n, path_cap) != 0) return -1;
  const PathEmitters E = path_emitters(a, c, f);
  const uint32_t n32 = (uint32_t)n, cap = (uint32_t)path_cap;
  const dim3 block(256), grid((n32 + 255u) / 256u), rgrid((cap + 255u) / 256u), sgrid((uint32_t)n_blocks);
  hipLaunchKernelGGL(rt_path_counts_kernel, sgrid, block, 0, s, n32, width, y0, pp.spp, (const float4*)c->pt_geo, r.sample_counts, c->pt_cnt, c->pt_bsum);
  hipLaunchKernelGGL(rt_path_scan_kernel, dim3(1), dim3(PT_SCAN_PASS), 0, s, (uint32_t)n_blocks, (const uint32_t*)c->pt_bsum, c->pt_boff, c->pt_ctot);
  hipLaunchKernelGGL(rt_path_offsets_kernel, sgrid, block, 0, s, n32, (const uint32_t*)c->pt_cnt, (const unsigned long long*)c->pt_boff, c->pt_off);
  if (hipGetLastError() != hipSuccess) return -1;
  const uint64_t n_batches = pp.bounces ? (all + batch - 1) / batch : 0;
  for (uint64_t b = 0; b < n_batches; ++b) {
    const unsigned long long g0 = b * batch;   // the batch's first path
    const auto start = [&](auto kernel, auto... rest) {
      hipLaunchKernelGGL(kernel, rgrid, block, 0, s, cap, g0, n32, (const unsigned long long*)c->pt_ctot, (const unsigned long long*)c->pt_off, c->pt_hdr,
                         (const float4*)c->pt_geo, (const float4*)c->pt_nrm, (const float4*)c->pt_dir, (const float4*)c->pt_lit, (const float4*)c->pt_alb,
                         c->pt_I, c->pt_N, c->pt_D, c->pt_L, c->pt_T, rest..., c->pt_live[0], c->pt_spix, c->pt_ssmp);
    };
    if (f.spec) start(rt_path_start_counts_specular_kernel, c->pt_A);
    else start(rt_path_start_counts_kernel);
    // slot -> (pixel, sample) through the slot tables the start kernel filled; the pixel's own count in place of spp.  The kernels are
    // the twins of the tail above, form for form
    const auto bounce_rays = [&](uint32_t d, const uint32_t* live, const uint32_t* n_live, uint32_t* n_next) {
      const auto launch = [&](auto kernel, auto... rest) {
        hipLaunchKernelGGL(kernel, rgrid, block, 0, s, cap, width, y0, pp.seed + d, (const uint32_t*)c->pt_spix, (const uint32_t*)c->pt_ssmp, (const uint32_t*)c->pt_cnt,
                           live, n_live, n_next, (const float4*)c->pt_I, (const float4*)c->pt_N, rest..., r.counters);
      };
      const SpecEm& e = E.rays;
      if (f.spec && f.emi == 3) launch(rt_path_bounce_specular_counts_kernel<2>, c->pt_D, c->pt_T, (const float4*)c->pt_A, c->pt_rays, e);
      else if (f.spec && f.emi == 2) launch(rt_path_bounce_specular_counts_kernel<1>, c->pt_D, c->pt_T, (const float4*)c->pt_A, c->pt_rays, e);
      else if (f.spec) launch(rt_path_bounce_specular_counts_kernel<0>, c->pt_D, c->pt_T, (const float4*)c->pt_A, c->pt_rays, SpecNoEm{});
      else if (f.emi >= 2) launch(f.emi == 3 ? rt_path_bounce_emitter_rays_counts_mis_kernel : rt_path_bounce_emitter_rays_counts_kernel, (const float4*)c->pt_D, c->pt_rays,
                                  e.tab, e.scale, e.erays, e.etmax, e.eG);
      else if (f.env == 2) launch(rt_path_bounce_env_rays_counts_kernel, (const float4*)c->pt_D, c->pt_rays, f.map, e.erays, e.etmax, e.eG);
      else launch(rt_path_bounce_rays_counts_kernel, (const float4*)c->pt_D, c->pt_rays);
    };
    if (path_batch_depths(a, c, r, f, E, p, cap, cap, SlotCounts{c->pt_spix, c->pt_ssmp, c->pt_cnt}, bounce_rays) != 0) return -1;
    hipLaunchKernelGGL(rt_path_accumulate_counts_kernel, grid, block, 0, s, n32, cap, g0, (const uint32_t*)c->pt_cnt, (const unsigned long long*)c->pt_off,
                       (const float4*)c->pt_L, c->pt_acc);
  }
  hipLaunchKernelGGL(rt_path_divide_counts_kernel, grid, block, 0, s, n32, (const uint32_t*)c->pt_cnt, (const float4*)c->pt_lit, pp.bounces == 0 ? 1u : 0u, c->pt_acc);
  if (hipGetLastError() != hipSuccess) return -1;
  // (the accumulators hold the colours: what ends the frame divides by spp = 1 and takes no flat sum; dn_frame passes the same)
  return path_frame_end(c, r, n32, 1u, 0u);
}

// Tail of a path frame (replaces the plain shading pass; the primary pass was the plain or shadow frame launch, whose records carry the
// occlusion bit): the request's form, resolved here once, and the tail of its slot source
int render_path_tail(vxrt_accel_t* a, FrameCtx* c, const RenderRequest& r, const ShadeParams& p, const float* utab, const float* vtab) {
  const PathForm f = path_form(r);
  return f.counts ? render_path_counts_tail(a, c, r, f, p, utab, vtab) : render_path_uniform_tail(a, c, r, f, p, utab, vtab);
}

// ---------------------------------------------------------------------------------------------
// host: the path API (include/vortex_hip.h).  One door builds a path request, render_path_frame; every vxrt_render_path* entry point
// checks that the parts its name promises are there, names them in a descriptor and goes through that door
// ---------------------------------------------------------------------------------------------

// A path frame by descriptor (see the header, "Path frames by descriptor"): the one place that turns arguments into a path request.
// What a descriptor can get wrong before a request exists is refused here -- a null part is "absent", so a part that an entry point
// promises is that entry point's to check; the rest is check_request's (rt_kernels.hip), whose empty window comes before its path tests.
// (specular: vxrt_render_path_frame_specular's part beside the descriptor, already checked and with enable = 1, or null; roulette:
//  vxrt_render_path_frame_ex's, likewise)
static int render_path_frame(vxrt_accel_t* accel, const vxrt_path_frame_t* f, const vxrt_specular_params_t* specular, void* stream,
                             const vxrt_roulette_params_t* roulette = nullptr, const vxrt_env_params_t* env = nullptr) {
  if (!f || f->size != sizeof(vxrt_path_frame_t)) return -1;
  for (int k = 0; k < 4; ++k) if (f->reserved[k] != 0u) return -1;
  if (!f->path || (f->emissive && f->emissive_mis) || f->motion > 1u) return -1;
  if (f->cam && !camera_ok(f->cam)) return -1;
  const bool chain = f->aov || f->temporal || f->history || f->motion || f->variance;   // (the rest of the chain needs the filter's parameters)
  if (chain && !f->denoise) return -1;
  if (f->temporal || f->history || f->motion || f->variance) {   // (a camera frame with a history of its kind that holds the window)
    if (!camera_ok(f->cam)) return -1;
    const uint64_t pixels = f->y0 <= f->y1 ? (uint64_t)f->width * (f->y1 - f->y0) : 0;   // (a bad window is check_request's to refuse)
    if (!tp_request_ok(f->history, f->temporal, pixels, f->variance != nullptr)) return -1;
  }
  RenderRequest req;
  req.width = f->width; req.height = f->height; req.y0 = f->y0; req.y1 = f->y1; req.params = f->params; req.shadow = f->path->shadow ? 1 : 0; req.cams = f->cam; req.path = f->path;
  req.dst = f->dst; req.colors = f->colors; req.counters = f->rays_traced; req.stream = stream;
  req.emissive = f->emissive; req.emissive_mis = f->emissive_mis; req.sample_counts = f->counts;
  req.denoise = f->denoise; req.aov = f->aov; req.temporal = f->temporal; req.history = f->history; req.motion = f->motion == 1u; req.prev_position = f->prev_position;
  req.variance = f->variance; req.variance_out = f->variance_out;
  req.specular = specular; req.roulette = roulette; req.env = env;
  return render_common(accel, req);
}

// the fields every vxrt_render_path* entry point sets alike
static vxrt_path_frame_t path_frame(const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, const vxrt_shade_params_t* params,
                                    const vxrt_path_params_t* path, uint32_t* dst, float* colors, unsigned long long* rays_traced) {
  vxrt_path_frame_t f{};
  f.size = sizeof f; f.width = width; f.height = height; f.y0 = y0; f.y1 = y1; f.cam = cam; f.params = params; f.path = path;
  f.dst = dst; f.colors = colors; f.rays_traced = rays_traced;
  return f;
}

extern "C" {

int vxrt_render_path(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, const vxrt_shade_params_t* params,
                     const vxrt_path_params_t* path, uint32_t* dst, float* colors, unsigned long long* rays_traced, void* stream) {
  const vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  return render_path_frame(accel, &f, nullptr, stream);
}

int vxrt_render_path_denoised(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, const vxrt_shade_params_t* params,
                              const vxrt_path_params_t* path, const vxrt_denoise_params_t* dn, uint32_t* dst, float* colors, const vxrt_path_aov_t* aov,
                              unsigned long long* rays_traced, void* stream) {
  if (!dn) return -1;
  vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  f.denoise = dn; f.aov = aov;
  return render_path_frame(accel, &f, nullptr, stream);
}

int vxrt_render_path_temporal(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, const vxrt_shade_params_t* params,
                              const vxrt_path_params_t* path, const vxrt_denoise_params_t* dn, const vxrt_temporal_params_t* temporal, vxrt_history_t* history,
                              uint32_t* dst, float* colors, const vxrt_path_aov_t* aov, unsigned long long* rays_traced, void* stream) {
  if (!dn || !temporal || !history) return -1;
  vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  f.denoise = dn; f.aov = aov; f.temporal = temporal; f.history = history;
  return render_path_frame(accel, &f, nullptr, stream);
}

int vxrt_render_path_temporal_motion(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                     const vxrt_shade_params_t* params, const vxrt_path_params_t* path, const vxrt_denoise_params_t* dn,
                                     const vxrt_temporal_params_t* temporal, vxrt_history_t* history, uint32_t* dst, float* colors,
                                     const vxrt_path_aov_t* aov, float* prev_position, unsigned long long* rays_traced, void* stream) {
  if (!dn || !temporal || !history) return -1;
  vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  f.denoise = dn; f.aov = aov; f.temporal = temporal; f.history = history; f.motion = 1u; f.prev_position = prev_position;
  return render_path_frame(accel, &f, nullptr, stream);
}

// (motion outside {0, 1} is refused before it becomes the descriptor's unsigned field)
int vxrt_render_path_variance(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, const vxrt_shade_params_t* params,
                              const vxrt_path_params_t* path, const vxrt_denoise_params_t* dn, const vxrt_temporal_params_t* temporal, const vxrt_variance_params_t* vp,
                              vxrt_history_t* history, int motion, uint32_t* dst, float* colors, const vxrt_path_aov_t* aov, float* prev_position, float* variance,
                              unsigned long long* rays_traced, void* stream) {
  if (!dn || !temporal || !vp || !history || motion < 0 || motion > 1) return -1;
  vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  f.denoise = dn; f.aov = aov; f.temporal = temporal; f.history = history; f.motion = (uint32_t)motion; f.prev_position = prev_position;
  f.variance = vp; f.variance_out = variance;
  return render_path_frame(accel, &f, nullptr, stream);
}

int vxrt_render_path_adaptive(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, const vxrt_shade_params_t* params,
                              const vxrt_path_params_t* path, const uint32_t* counts, uint32_t* dst, float* colors, unsigned long long* rays_traced, void* stream) {
  if (!counts) return -1;
  vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  f.counts = counts;
  return render_path_frame(accel, &f, nullptr, stream);
}

int vxrt_render_path_variance_adaptive(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                       const vxrt_shade_params_t* params, const vxrt_path_params_t* path, const uint32_t* counts,
                                       const vxrt_denoise_params_t* dn, const vxrt_temporal_params_t* temporal, const vxrt_variance_params_t* vp,
                                       vxrt_history_t* history, int motion, uint32_t* dst, float* colors, const vxrt_path_aov_t* aov, float* prev_position,
                                       float* variance, unsigned long long* rays_traced, void* stream) {
  if (!counts || !dn || !temporal || !vp || !history || motion < 0 || motion > 1) return -1;
  vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  f.counts = counts;
  f.denoise = dn; f.aov = aov; f.temporal = temporal; f.history = history; f.motion = (uint32_t)motion; f.prev_position = prev_position;
  f.variance = vp; f.variance_out = variance;
  return render_path_frame(accel, &f, nullptr, stream);
}

int vxrt_render_path_emissive(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, const vxrt_shade_params_t* params,
                              const vxrt_path_params_t* path, const vxrt_emissive_params_t* em, uint32_t* dst, float* colors, unsigned long long* rays_traced,
                              void* stream) {
  if (!em) return -1;
  vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  f.emissive = em;
  return render_path_frame(accel, &f, nullptr, stream);
}

int vxrt_render_path_emissive_mis(vxrt_accel_t* accel, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                  const vxrt_shade_params_t* params, const vxrt_path_params_t* path, const vxrt_emissive_mis_params_t* em, uint32_t* dst,
                                  float* colors, unsigned long long* rays_traced, void* stream) {
  if (!em) return -1;
  vxrt_path_frame_t f = path_frame(cam, width, height, y0, y1, params, path, dst, colors, rays_traced);
  f.emissive_mis = em;
  return render_path_frame(accel, &f, nullptr, stream);
}

// A path frame whose vertices may be specular (see the header, "Specular vertices"): the descriptor's frame with the specular kernels in
// its tail.  A null part or enable = 0 is vxrt_render_path_frame; what the part alone can get wrong is refused here, the filter chain
// beside enable = 1 is check_request's to refuse.  So is an output without its part, which only a caller's descriptor can ask for ahead
// of the empty window: the entry points above hand theirs to check_request as they always have.
int vxrt_render_path_frame_specular(vxrt_accel_t* accel, const vxrt_path_frame_t* f, const vxrt_specular_params_t* specular, void* stream) {
  if (f && ((f->prev_position && !f->motion) || (f->variance_out && !f->variance))) return -1;
  if (!specular) return render_path_frame(accel, f, nullptr, stream);
  if (specular->enable > 1u || specular->reserved[0] != 0u || specular->reserved[1] != 0u || specular->reserved[2] != 0u) return -1;
  return render_path_frame(accel, f, specular->enable ? specular : nullptr, stream);
}
int vxrt_render_path_frame(vxrt_accel_t* accel, const vxrt_path_frame_t* f, void* stream) { return vxrt_render_path_frame_specular(accel, f, nullptr, stream); }

// A path frame that ends dim paths early (see the header, "Russian roulette"): the descriptor's frame whose scatter step draws at the
// vertices first .. bounces - 1.  A null part or enable = 0 is vxrt_render_path_frame_specular; with enable = 1 what the part alone can
// get wrong is refused here, and so is the specular part with enable = 1 beside it (check_request refuses the pair as well, behind its
// empty window).  A specular part with enable = 0 is checked as its own entry point checks it.
static bool roulette_q_min_ok(float q_min) { return std::isfinite(q_min) && q_min > 0.0f && q_min <= 1.0f; }
// (what a roulette part with enable != 0 can get wrong alone: both doors that take one ask here)
static bool roulette_part_ok(const vxrt_roulette_params_t* r) {
  return r->enable == 1u && r->first >= 1u && r->first <= VXRT_PATH_MAX_BOUNCES && roulette_q_min_ok(r->q_min) && r->reserved == 0u;
}
int vxrt_render_path_frame_ex(vxrt_accel_t* accel, const vxrt_path_frame_t* f, const vxrt_specular_params_t* specular, const vxrt_roulette_params_t* roulette,
                              void* stream) {
  if (!roulette || roulette->enable == 0u) return vxrt_render_path_frame_specular(accel, f, specular, stream);
  if (!roulette_part_ok(roulette)) return -1;
  if (f && ((f->prev_position && !f->motion) || (f->variance_out && !f->variance))) return -1;
  if (specular && (specular->enable != 0u || specular->reserved[0] != 0u || specular->reserved[1] != 0u || specular->reserved[2] != 0u)) return -1;
  return render_path_frame(accel, f, nullptr, stream, roulette);
}

// A path frame lit by an environment map (see the header, "Environment light"): the descriptor's frame, with the roulette part if it is
// enabled, whose misses see the map and, with sample = 1, whose vertices send an environment ray.  A null part IS
// vxrt_render_path_frame_ex without a specular part.  The descriptor's size comes first -- nothing of a shorter one is read -- then what
// the parts alone can get wrong and an emitter form beside the map: all of it ahead of check_request's empty window, which is why
// check_request, the one place that sees every request, cannot be the only one to refuse them.
int vxrt_render_path_frame_env(vxrt_accel_t* accel, const vxrt_path_frame_t* f, const vxrt_roulette_params_t* roulette, const vxrt_env_params_t* env, void* stream) {
  if (!env) return vxrt_render_path_frame_ex(accel, f, nullptr, roulette, stream);
  if (!f || f->size != sizeof(vxrt_path_frame_t)) return -1;
  if (!env_params_ok(env) || f->emissive || f->emissive_mis) return -1;
  if ((f->prev_position && !f->motion) || (f->variance_out && !f->variance)) return -1;
  const bool rr = roulette && roulette->enable != 0u;
  if (rr && !roulette_part_ok(roulette)) return -1;
  return render_path_frame(accel, f, nullptr, stream, rr ? roulette : nullptr, env);
}

// The single launches below run on caller-owned buffers, asynchronous on `stream`, without a host synchronisation.

// The lobe pick and the mirror ray alone (see the header, "Specular vertices")
int vxrt_specular_pick(uint64_t n, const float* vertices, const uint32_t* seeds, float* rays, uint32_t* lobe, void* stream) {
  if (!vertices || !seeds || !rays || !lobe || n >= 0x80000000ull) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_specular_pick_kernel, dim3(((uint32_t)n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, (uint32_t)n, vertices, seeds, rays, lobe);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The roulette step alone (see the header, "Russian roulette")
int vxrt_roulette(uint64_t n, const float* thr, const uint32_t* seeds, float q_min, float* thr_out, uint32_t* alive, void* stream) {
  if (!thr || !seeds || !thr_out || !alive || n >= 0x80000000ull || !roulette_q_min_ok(q_min)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_roulette_kernel, dim3(((uint32_t)n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, (uint32_t)n, thr, seeds, q_min, thr_out, alive);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The emitter ray alone (see the header, "Emissive geometry"), and its weighted twin ("Multiple importance sampling")
int vxrt_emitter_rays(vxrt_accel_t* a, uint64_t n, const float* points, const uint32_t* seeds, float scale, float* rays, float* tmax, float* weight3,
                      uint32_t* emitter, void* stream) {
  if (!a || !emitters_valid(a) || !points || !seeds || !rays || !tmax || !weight3 || !emitter) return -1;
  if (!(scale >= 0.0f) || !std::isfinite(scale) || n >= 0x80000000ull) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_emitter_rays_kernel, dim3(((uint32_t)n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, emitter_tab(a), (uint32_t)n, points, seeds, scale,
                     rays, tmax, weight3, emitter);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int vxrt_emitter_rays_mis(vxrt_accel_t* a, uint64_t n, const float* points, const uint32_t* seeds, float scale, float* rays, float* tmax, float* weight3,
                          uint32_t* emitter, float* mis, void* stream) {
  if (!a || !emitters_valid(a) || !points || !seeds || !rays || !tmax || !weight3 || !emitter || !mis) return -1;
  if (!(scale >= 0.0f) || !std::isfinite(scale) || n >= 0x80000000ull) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_emitter_rays_mis_kernel, dim3(((uint32_t)n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, emitter_tab(a), (uint32_t)n, points, seeds, scale,
                     rays, tmax, weight3, emitter, mis);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The lookup in the emitter index and the bounce ray's weight alone; the call that finds no index builds it first (one synchronisation
// of `stream`, as for a buffer that grows)
int vxrt_emitter_hit_weights(vxrt_accel_t* a, uint64_t n, const float* rays, const void* hits, const float* normals, uint32_t* emitter, float* mis, void* stream) {
  if (!a || !emitters_valid(a) || !rays || !hits || !normals || !emitter || !mis || n >= 0x80000000ull) return -1;
  if (n == 0) return 0;
  if (emitter_index_ensure(a, (hipStream_t)stream) != 0) return -1;
  hipLaunchKernelGGL(rt_emitter_hit_weights_kernel, dim3(((uint32_t)n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, emitter_tab(a), emitter_idx(a), (uint32_t)n,
                     rays, (const HitRec*)hits, normals, emitter, mis);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Sample counts from a variance buffer (see the header, "Adaptive sampling"): elementwise
int vxrt_sample_counts(uint64_t n, const float* variance, const uint32_t* prev_counts, const vxrt_sample_count_params_t* prm, uint32_t* counts,
                       unsigned long long* total, void* stream) {
  if (!prm || !variance || !counts || n >= 0x80000000ull || prm->reserved != 0u) return -1;
  if (!(prm->gain > 0.0f) || !std::isfinite(prm->gain) || prm->min_spp == 0u || prm->min_spp > prm->max_spp || prm->max_spp > 4096u) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_sample_counts_kernel, dim3(((uint32_t)n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, (uint32_t)n, variance, prev_counts, prm->gain,
                     prm->min_spp, prm->max_spp, counts, total);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The previous-position guide of caller-owned hit records (see the header, "Motion")
int vxrt_previous_positions(vxrt_accel_t* a, uint32_t n, const vxrt_hit_t* hits, float* prev_position4, float* prev_normal4, void* stream) {
  if (!a || a->stale || a->motion_what == 0u || !a->ref.triEx) return -1;
  if (!hits || !prev_position4 || !prev_normal4 || (((uintptr_t)prev_position4 | (uintptr_t)prev_normal4) & 15u) != 0) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_previous_positions_kernel, dim3((n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, a->dev, motion_src(a), n, (const HitRec*)hits,
                     (float4*)prev_position4, (float4*)prev_normal4);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
