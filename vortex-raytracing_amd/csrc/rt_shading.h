// Device arithmetic of shading that the frame kernels (rt_kernels.hip) and the passes of the secondary tails (rt_secondary.hip,
// rt_path.hip) share: the closest-hit / miss shader's terms, the shadow, mirror, camera and sample rays, the tile-major index of a hit
// record, and the workgroup's list append of the two tails' prepare kernels (wg_append, PREP_CHUNKS).
// Each unit compiles its own copy; every function is written once, here, so that all restate the reference in the same operations.
// (shade_terms and shade_eval are plain templates, the rest is __forceinline__: the inliner's decisions inside the frame kernels
// depend on it.)  pack_rgb8, f2i_x86 and std_min, which rt_denoise.hip takes as well, are in rt_internal.h.
#pragma once
#include "rt_internal.h"
#include "pinhole.h"

// libstdc++ std::min / std::max (rt_traversal.cpp:327-337 use them; NaN behaviour is part of parity; std_min is in rt_internal.h)
__device__ __forceinline__ float std_max(float a, float b) { return (a < b) ? b : a; }

// ---------------------------------------------------------------------------------------------
// shading (closest.cpp:57-127 / miss.cpp:9-14)
// ---------------------------------------------------------------------------------------------
// rtx_shading.h:7-8 and common.h:149-154 convert floats that C leaves undefined (NaN, a value outside the target type).  The rule
// (include/vortex_hip.h, vxrt_shade_rays) is what x86-64 g++ makes of them, written as a range test so that neither
// this file nor oracle/rt_oracle.c depends on an out-of-range cast:
//   uint32_t(f) = cvttss2si r64, low half: the truncated value mod 2^32 for -2^63 <= f < 2^63, 0 for NaN and everything else
//   int(f)      = cvttss2si r32: the truncated value for -2^31 <= f < 2^31, INT_MIN (0x80000000) for NaN and everything else
// (f2i_x86 and pack_rgb8, which rt_denoise.hip packs with as well, are in rt_internal.h)
__device__ __forceinline__ uint32_t f2u_x86(float f) { return (f >= -0x1p63f && f < 0x1p63f) ? (uint32_t)(long long)f : 0u; }

// Occlusion ray of the shadow extension (no reference counterpart): from the hit point toward the
// light, origin pushed 1e-3 along L like the reference's mirror bounce (closest.cpp:104), tmax = |L|.
// I, L and dist are computed exactly as shade_eval computes them.
__device__ __forceinline__ void shadow_ray(float lpx, float lpy, float lpz, float ox, float oy, float oz, float dx, float dy, float dz,
                                           float hit_dist, float& sox, float& soy, float& soz, float& sdx, float& sdy, float& sdz, float& sdist) {
  const float Ix = ox + dx * hit_dist, Iy = oy + dy * hit_dist, Iz = oz + dz * hit_dist;
  float Lx = lpx - Ix, Ly = lpy - Iy, Lz = lpz - Iz;
  const float dist = sqrtf(Lx * Lx + Ly * Ly + Lz * Lz);
  const float il = 1.0f / dist;
  Lx *= il; Ly *= il; Lz *= il;
  sox = Ix + Lx * 0.001f; soy = Iy + Ly * 0.001f; soz = Iz + Lz * 0.001f;
  sdx = Lx; sdy = Ly; sdz = Lz;
  sdist = dist;
}

__device__ __forceinline__ void shadow_ray(const ShadeParams& p, float ox, float oy, float oz, float dx, float dy, float dz,
                                           float hit_dist, float& sox, float& soy, float& soz, float& sdx, float& sdy, float& sdz, float& sdist) {
  shadow_ray(p.lpos[0], p.lpos[1], p.lpos[2], ox, oy, oz, dx, dy, dz, hit_dist, sox, soy, soz, sdx, sdy, sdz, sdist);
}

// closest.cpp:57-90 for one hit: the non-reflected diffuse contribution `throughput * diffuse * (1 - reflectivity)`
// with throughput = 1 (:87), the reflectivity (:84), the hit point I and the shading normal N.
// occluded: result of the shadow extension (false = reference).
template <bool STATS = false>
__device__ void shade_terms(const SceneDev& sc, const ShadeParams& p, float ox, float oy, float oz,
                            float dx, float dy, float dz, const HitRec& hit, bool occluded,
                            float& r, float& g, float& b, float& refl_out,
                            float& Ix_o, float& Iy_o, float& Iz_o, float& Nx_o, float& Ny_o, float& Nz_o,
                            unsigned* textured = nullptr, float* albedo3 = nullptr) {
  const uint32_t* bp = sc.blas + (size_t)hit.blasIdx * (RT_BLAS_STRIDE / 4);
  const rt_triex_t te = sc.triEx[hit.triIdx];
  const rt_material_t* mat = sc.mat + te.texId;
  // I = orig + dir * dist (:61)
  const float Ix = ox + dx * hit.dist, Iy = oy + dy * hit.dist, Iz = oz + dz * hit.dist;
  // N = N1*bx + N2*by + N0*bz (:64)
  float Nx = te.N1[0] * hit.bx + te.N2[0] * hit.by + te.N0[0] * hit.bz;
  float Ny = te.N1[1] * hit.bx + te.N2[1] * hit.by + te.N0[1] * hit.bz;
  float Nz = te.N1[2] * hit.bx + te.N2[2] * hit.by + te.N0[2] * hit.bz;
  // transposed 3x3 of invTransform, TransformVector with w = 0 (:65-66, geometry.h:1141-1147,1280-1293)
  const float m0 = __uint_as_float(bp[1]), m1 = __uint_as_float(bp[2]), m2 = __uint_as_float(bp[3]);
  const float m4 = __uint_as_float(bp[5]), m5 = __uint_as_float(bp[6]), m6 = __uint_as_float(bp[7]);
  const float m8 = __uint_as_float(bp[9]), m9 = __uint_as_float(bp[10]), m10 = __uint_as_float(bp[11]);
  const float z0 = 0.0f * 0.0f;
  float Tx = m0 * Nx + m4 * Ny + m8 * Nz + z0;
  float Ty = m1 * Nx + m5 * Ny + m9 * Nz + z0;
  float Tz = m2 * Nx + m6 * Ny + m10 * Nz + z0;
  float inv = 1.0f / sqrtf(Tx * Tx + Ty * Ty + Tz * Tz);
  Nx = Tx * inv; Ny = Ty * inv; Nz = Tz * inv;
  // uv (:69)
  const float u = te.uv1[0] * hit.bx + te.uv2[0] * hit.by + te.uv0[0] * hit.bz;
  const float v = te.uv1[1] * hit.bx + te.uv2[1] * hit.by + te.uv0[1] * hit.bz;
  float cr, cg, cb;
  if (mat->diffuse_tex_id >= 0) {  // :72-77, texSample rtx_shading.h:5-18, RGB8toRGB32F common.h:156-162
    if (STATS) *textured += 1;
    const uint32_t tw = mat->tex_width, th = mat->tex_height;
    uint32_t iu = f2u_x86(u * (float)tw), iv = f2u_x86(v * (float)th);
    iu %= tw; iv %= th;
    const uint32_t texel = ((const uint32_t*)(sc.tex + mat->tex_offset))[iu + iv * tw];
    const float s = 1 / 256.0f;
    cr = (float)(int)((texel >> 16) & 255) * s;
    cg = (float)(int)((texel >> 8) & 255) * s;
    cb = (float)(int)(texel & 255) * s;
  } else {
    cr = mat->diffuse[0]; cg = mat->diffuse[1]; cb = mat->diffuse[2];
  }
  // diffuseLighting (rtx_shading.h:55-67)
  float Lx = p.lpos[0] - Ix, Ly = p.lpos[1] - Iy, Lz = p.lpos[2] - Iz;
  const float dist = sqrtf(Lx * Lx + Ly * Ly + Lz * Lz);
  const float il = 1.0f / dist;
  Lx *= il; Ly *= il; Lz *= il;
  const float att = 1.0f / (1.0f + dist * 0.1f);
  float NdotL = std_max(0.0f, Nx * Lx + Ny * Ly + Nz * Lz);
  if (occluded) NdotL = 0.0f;   // shadow extension: occluded -> no direct term
  const float dr = cr * (p.amb[0] + att * p.lcol[0] * NdotL);
  const float dg = cg * (p.amb[1] + att * p.lcol[1] * NdotL);
  const float db = cb * (p.amb[2] + att * p.lcol[2] * NdotL);
  const float refl = __uint_as_float(bp[38]);   // blas_node_t::reflectivity @152
  const float thr = 1.0f;
  r = 0.0f + thr * dr * (1 - refl);             // :87
  g = 0.0f + thr * dg * (1 - refl);
  b = 0.0f + thr * db * (1 - refl);
  refl_out = refl;
  Ix_o = Ix; Iy_o = Iy; Iz_o = Iz; Nx_o = Nx; Ny_o = Ny; Nz_o = Nz;
  if (albedo3) { albedo3[0] = cr; albedo3[1] = cg; albedo3[2] = cb; }   // texColor (:72-77)
}

// closest.cpp:57-127 without a secondary ray (reflectivity <= 0 or bounce + 1 >= max_depth) / miss.cpp:9-14
template <bool STATS = false>
__device__ void shade_eval(const SceneDev& sc, const ShadeParams& p, float ox, float oy, float oz,
                           float dx, float dy, float dz, const HitRec& hit, bool found, bool occluded,
                           float& r, float& g, float& b, unsigned* textured = nullptr) {
  if (!found) { r = p.bg[0]; g = p.bg[1]; b = p.bg[2]; return; }
  float refl, Ix, Iy, Iz, Nx, Ny, Nz;
  shade_terms<STATS>(sc, p, ox, oy, oz, dx, dy, dz, hit, occluded, r, g, b, refl, Ix, Iy, Iz, Nx, Ny, Nz, textured);
  float thr = 1.0f;
  thr *= refl;                                  // :90
  r = r + p.bg[0] * thr;                        // :123
  g = g + p.bg[1] * thr;
  b = b + p.bg[2] * thr;
}

// closest.cpp:96-99: the mirror ray leaving a hit.  R = normalize(dir - 2.0f * N * dot(N, dir)), origin I + R * 0.001f
__device__ __forceinline__ void mirror_ray(float dx, float dy, float dz, float Ix, float Iy, float Iz, float Nx, float Ny, float Nz,
                                           float* out6) {
  const float nd = Nx * dx + Ny * dy + Nz * dz;
  const float vx = dx - (2.0f * Nx) * nd, vy = dy - (2.0f * Ny) * nd, vz = dz - (2.0f * Nz) * nd;
  const float inv = 1.0f / sqrtf(vx * vx + vy * vy + vz * vz);
  const float Rx = vx * inv, Ry = vy * inv, Rz = vz * inv;
  out6[0] = Ix + Rx * 0.001f; out6[1] = Iy + Ry * 0.001f; out6[2] = Iz + Rz * 0.001f;
  out6[3] = Rx; out6[4] = Ry; out6[5] = Rz;
}

// kernel.cpp:28-39.  u = (x*2.0 - W)/H and v = (y*2.0 - H)/H are evaluated in double and rounded to
// f32 there; they depend on x (resp. y) only, so the host evaluates exactly that expression once per
// column / row (IEEE double division is correctly rounded on both sides) and the kernels read the
// two small tables instead of running an f64 divide per ray.
__device__ __forceinline__ void generate_ray(float u, float v,
                                             float& ox, float& oy, float& oz, float& dx, float& dy, float& dz) {
  // front=(1,0,0); right=cross(front,(0,1,0))=(0,0,1); up=cross(right,front)=(0,1,0)
  const float rx = 0.0f * 0.0f - 0.0f * 1.0f, ry = 0.0f * 0.0f - 1.0f * 0.0f, rz = 1.0f * 1.0f - 0.0f * 0.0f;
  const float ux = ry * 0.0f - rz * 0.0f, uy = rz * 1.0f - rx * 0.0f, uz = rx * 0.0f - ry * 1.0f;
  const float FOV = 1.0f;
  float vx = u * rx + v * ux + FOV * 1.0f;
  float vy = u * ry + v * uy + FOV * 0.0f;
  float vz = u * rz + v * uz + FOV * 0.0f;
  const float inv = 1.0f / sqrtf(vx * vx + vy * vy + vz * vz);
  ox = 0.0f; oy = 100.0f; oz = 0.0f;
  dx = vx * inv; dy = vy * inv; dz = vz * inv;
}

// Camera frames (JOB_CAM, vxrt_render_camera): the frame context's camera block, written on the stream by rt_camera_prep_kernel.  Its
// head holds VXRT_MAX_BATCH cameras of CAM_HDR floats (pos, forward, right, up); behind it, frame f's x_vp[W] then y_vp[H] start at
// CAM_TAB + f * (W + H) (see pinhole.h).  The kernels take the head as `utab` and the tables as `vtab`.
#define CAM_HDR 12
#define CAM_TAB (VXRT_MAX_BATCH * CAM_HDR)
__device__ __forceinline__ void camera_ray(const float* c, const float* tab, uint32_t W, uint32_t x, uint32_t y,
                                           float& ox, float& oy, float& oz, float& dx, float& dy, float& dz) {
  ox = c[0]; oy = c[1]; oz = c[2];
  pinhole_dir(tab[x], tab[W + y], c, c + 3, c + 6, c + 9, dx, dy, dz);
}
// the primary ray of pixel (x, y) of frame `frame` (0 unless a batch): the fixed camera's tables, or the camera block
template <bool CAM>
__device__ __forceinline__ void frame_pixel_ray(const float* utab, const float* vtab, uint32_t W, uint32_t H, uint32_t frame, uint32_t x, uint32_t y,
                                                float& ox, float& oy, float& oz, float& dx, float& dy, float& dz) {
  if constexpr (CAM) camera_ray(utab + frame * CAM_HDR, vtab + (size_t)frame * (W + H), W, x, y, ox, oy, oz, dx, dy, dz);
  else generate_ray(utab[x], vtab[y], ox, oy, oz, dx, dy, dz);
}

__device__ __forceinline__ uint32_t wang_hash(uint32_t s) {   // common.h:129-135
  s = (s ^ 61u) ^ (s >> 16);
  s *= 9u; s = s ^ (s >> 4);
  s *= 0x27d4eb2du;
  s = s ^ (s >> 15);
  return s;
}
__device__ __forceinline__ float random_float(uint32_t& s) {   // common.h:137-147
  s ^= s << 13; s ^= s >> 17; s ^= s << 5;
  return (float)s * 2.3283064365387e-10f;
}

// The occlusion / bounce ray of sample `smp` of pixel (x, y) leaving the hit point I with shading normal N (view direction vd), as
// oracle/rt_oracle.c:orc_ao_ray defines it, operation by operation: o = I + N' * 1e-3, d = cosine-weighted about the normal N'
// that faces the viewer (rejection-sampled disk, Duff et al. basis; only IEEE add / mul / div / sqrt).
__device__ __forceinline__ void ao_sample_ray(uint32_t x, uint32_t y, uint32_t W, uint32_t spp, uint32_t smp, uint32_t user_seed,
                                              float Ix, float Iy, float Iz, float nx, float ny, float nz, float vdx, float vdy, float vdz, float* o6) {
  uint32_t seed = wang_hash((x + y * W) * spp + smp + 1u + user_seed * 0x9E3779B9u);
  if (seed == 0u) seed = 1u;
  float u = 0.0f, v = 0.0f, r2 = 0.0f;
  bool ok = false;
  for (int k = 0; k < 8 && !ok; ++k) {
    const float a = 2.0f * random_float(seed) - 1.0f;
    const float b = 2.0f * random_float(seed) - 1.0f;
    const float q = a * a + b * b;
    if (q < 1.0f) { u = a; v = b; r2 = q; ok = true; }
  }
  const float z = sqrtf(1.0f - r2);
  if (nx * vdx + ny * vdy + nz * vdz > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
  const float sign = nz >= 0.0f ? 1.0f : -1.0f;
  const float a = -1.0f / (sign + nz);
  const float b = nx * ny * a;
  const float tx = 1.0f + sign * nx * nx * a, ty = sign * b, tz = -sign * nx;
  const float bx = b, by = sign + ny * ny * a, bz = -ny;
  o6[0] = Ix + nx * 0.001f; o6[1] = Iy + ny * 0.001f; o6[2] = Iz + nz * 0.001f;
  o6[3] = tx * u + bx * v + nx * z;
  o6[4] = ty * u + by * v + ny * z;
  o6[5] = tz * u + bz * v + nz * z;
}

// Alpha test of a candidate (ALPHA instantiations; the rule is in DESIGN.md s2, "Alpha test"): true = the candidate on triangle triIdx with
// barycentrics (bx, by, bz) is rejected -- its material has a threshold T > 0 and the texel shade_terms would sample there has a top byte
// below T.  u, v, the conversions and the texel address are shade_terms', operation for operation.
// What it loads, in this order: one byte of the per-triangle threshold table (an opaque triangle ends here); then the seven words uv0 .. texId
// of the triangle's tri_ex_t (not its normals), the material's four texture fields (not its colours) and the texel.
__device__ __forceinline__ bool alpha_rejects(const SceneDev& sc, const uint8_t* __restrict__ alpha_tri, uint32_t triIdx, float bx, float by, float bz) {
  const uint32_t T = alpha_tri[triIdx];
  if (T == 0u) return false;
  const rt_triex_t* te = sc.triEx + triIdx;
  const float u0 = te->uv0[0], v0 = te->uv0[1], u1 = te->uv1[0], v1 = te->uv1[1], u2 = te->uv2[0], v2 = te->uv2[1];
  const rt_material_t* mat = sc.mat + te->texId;
  const uint32_t tw = mat->tex_width, th = mat->tex_height;
  const uint64_t off = mat->tex_offset;
  const float u = u1 * bx + u2 * by + u0 * bz;
  const float v = v1 * bx + v2 * by + v0 * bz;
  uint32_t iu = f2u_x86(u * (float)tw), iv = f2u_x86(v * (float)th);
  iu %= tw; iv %= th;
  const uint32_t texel = ((const uint32_t*)(sc.tex + off))[iu + iv * tw];
  return (texel >> 24) < T;
}
// Hit records of a frame window are kept TILE-MAJOR between the traversal and the shading pass: record of pixel (x, y) =
// tile * 64 + lane of the 8x8 tile grid that starts at row y0, i.e. the job id of the traversal kernel.  A wavefront
// therefore writes the 64 records of its tile as one contiguous, 128-byte aligned 1,536-byte block, once (the occlusion
// result is folded into bit 31 of blasIdx before the record is written): no cache line is shared between wavefronts, so no
// XCD writes a partial line back (round 1 wrote pixel-major records + an atomicOr per occluded pixel: 121 MB of HBM
// writes per 1080p frame for 50 MB of records, profiles/r01_k_pmc.txt).
// `lr` = local row of the window: rows are counted through the window's tile rows (8 each) in order.
__device__ __forceinline__ size_t hit_index(uint32_t x, uint32_t lr, uint32_t tiles_x) {
  return ((size_t)(lr >> 3) * tiles_x + (x >> 3)) * 64u + ((lr & 7u) << 3) + (x & 7u);
}

// The hit pixels of a frame are appended to one list.  One atomic per wavefront on the list's counter (32,400 for a 1080p frame, all on
// one address, ~10 ns apart) was 0.3 of the AO prepare kernel's 0.37 ms: a workgroup now counts the hits of 1,024 pixels in LDS and
// appends once.
#define PREP_CHUNKS 4   // pixels per thread of the two prepare kernels: one list-append atomic per 1,024 pixels
// Append value[c] of every thread with flag[c] to list[] (its length in *counter; the order is arbitrary): the workgroup counts in LDS
// and does one atomic.  Every thread of the workgroup calls it.
template <int C>
__device__ __forceinline__ void wg_append(const bool (&flag)[C], const uint32_t (&value)[C], uint32_t* __restrict__ list, uint32_t* counter) {
  __shared__ uint32_t s_cnt[C][4];
  __shared__ uint32_t s_base;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t off[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const unsigned long long m = __ballot(flag[c]);
    off[c] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[c][wv] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int c = 0; c < C; ++c) for (int w = 0; w < 4; ++w) { const uint32_t v = s_cnt[c][w]; s_cnt[c][w] = tot; tot += v; }
    s_base = tot ? atomicAdd(counter, tot) : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (flag[c]) list[s_base + s_cnt[c][wv] + off[c]] = value[c];
}
