// Device arithmetic of the environment light (include/vortex_hip.h, "Environment light"), shared by rt_env.hip (the table, the steps alone)
// and rt_path.hip (the frame): the unfolding, the texel of a direction with its density, the environment ray.  Every function is the
// header's definition operation for operation -- one fp32 operation per symbol, in the order written (-ffp-contract=off).
// Include after rt_internal.h and rt_shading.h (EnvTab, std_max, random_float).
#pragma once

#define ENV_MAX_N 256u   // texels per side at most: the row ends of a map fit 1 KB of LDS

__host__ __device__ __forceinline__ float env_sign(float t) { return t >= 0.0f ? 1.0f : -1.0f; }

// the point P = (u', c, v') of the octahedron |x| + |y| + |z| = 1 under (u, v) of the texel square, and r2 = |P|^2
__host__ __device__ __forceinline__ void env_unfold(float u, float v, float& Px, float& Py, float& Pz, float& r2) {
  const float c = (1.0f - fabsf(u)) - fabsf(v);
  float uf = u, vf = v;
  if (c < 0.0f) { uf = (1.0f - fabsf(v)) * env_sign(u); vf = (1.0f - fabsf(u)) * env_sign(v); }
  Px = uf; Py = c; Pz = vf;
  r2 = (Px * Px + Py * Py) + Pz * Pz;
}

// THE TABLE's weight of texel (i, j) with radiance L: max(max(L.r, L.g), L.b) / (r2 * r) at the texel's centre.  (Host too: creation
// refuses a map with a weight that is not finite before anything is uploaded.)
__host__ __device__ __forceinline__ float env_texel_weight(uint32_t n, uint32_t i, uint32_t j, float Lr, float Lg, float Lb) {
  const float u = (((float)i + 0.5f) / (float)n) * 2.0f - 1.0f;
  const float v = (((float)j + 0.5f) / (float)n) * 2.0f - 1.0f;
  float Px, Py, Pz, r2;
  env_unfold(u, v, Px, Py, Pz, r2);
  const float r = sqrtf(r2);
  float m = (Lr < Lg) ? Lg : Lr;
  m = (m < Lb) ? Lb : m;
  return m / (r2 * r);
}

__device__ __forceinline__ uint32_t env_axis_texel(float t, uint32_t n) {
  const float f = (t * 0.5f + 0.5f) * (float)n;   // (in [0, n] or a NaN: the conversion is defined)
  return f >= 0.0f ? min((uint32_t)f, n - 1u) : 0u;
}

// TEXEL OF A DIRECTION: e, and r2 * r of the point the direction unfolds to (a NaN and the zero vector give texel 0)
__device__ __forceinline__ uint32_t env_texel(uint32_t n, float x, float y, float z, float& r3) {
  const float s = (fabsf(x) + fabsf(y)) + fabsf(z);
  const float px = x / s, py = y / s, pz = z / s;
  float u = px, v = pz;
  if (py < 0.0f) { u = (1.0f - fabsf(pz)) * env_sign(px); v = (1.0f - fabsf(px)) * env_sign(pz); }
  const uint32_t i = env_axis_texel(u, n), j = env_axis_texel(v, n);
  const float r2 = (px * px + py * py) + pz * pz;
  const float r = sqrtf(r2);
  r3 = r2 * r;
  return i + j * n;
}

// pe of texel e at a point with r3 = r2 * r
__device__ __forceinline__ float env_density(const EnvTab& E, uint32_t e, float r3) {
  const float qf = (float)E.q[e] / (float)E.Q;
  const float nn4 = (float)(E.n * E.n) * 0.25f;
  return (qf * nn4) * r3;
}

// Env(w) = texel_e * scale of direction (x, y, z), and pe(w)
__device__ __forceinline__ uint32_t env_lookup(const EnvTab& E, float x, float y, float z, float (&L)[3], float& pe) {
  float r3;
  const uint32_t e = env_texel(E.n, x, y, z, r3);
  const float* T = E.texels + 3 * (size_t)e;
  L[0] = T[0] * E.scale; L[1] = T[1] * E.scale; L[2] = T[2] * E.scale;
  pe = env_density(E, e, r3);
  return e;
}

// wB of a bounce ray w that missed, from a vertex with facing normal N' (nx, ny, nz), given pe(w)
__device__ __forceinline__ float env_miss_weight(float pe, float nx, float ny, float nz, float wx, float wy, float wz) {
  const float cosx = std_max(0.0f, (nx * wx + ny * wy) + nz * wz);
  const float pb = cosx / 3.14159265f;
  const float den = pe + pb;
  return den > 0.0f ? pb / den : 1.0f;
}

// The row ends of the map's cumulative table -- rows[j] = cum[(j + 1) * n - 1] -- staged by a workgroup of at least n threads; ends in
// a barrier every thread of the workgroup must reach
__device__ __forceinline__ void env_stage_rows(const EnvTab& E, uint32_t* rows) {
  if (threadIdx.x < E.n) rows[threadIdx.x] = E.cum[(threadIdx.x + 1u) * E.n - 1u];
  __syncthreads();
}

// THE ENVIRONMENT RAY from hash output `seed`, the surface point I and the facing normal N' (nx, ny, nz).  ray6 = (o, w), tmax, Gm[3],
// e = the texel chosen, wE; false = skipped: the ray nothing can hit, tmax = -1, Gm = 0, wE = 0.  rows: the staged row ends (LDS).  The
// smallest e with cum[e] > t: the row by a binary search over the row ends, then the texel by one over the row -- at most 8 steps each,
// the second half only from global memory.
__device__ __forceinline__ bool env_sample(const EnvTab& E, const uint32_t* rows, uint32_t seed, float Ix, float Iy, float Iz, float nx, float ny, float nz,
                                           float (&ray6)[6], float& tmax, float (&G)[3], uint32_t& e_out, float& wE_out) {
  if (seed == 0u) seed = 1u;
  seed ^= seed << 13; seed ^= seed >> 17; seed ^= seed << 5;
  const uint32_t r0 = seed;
  const float a = random_float(seed);
  const float b = random_float(seed);
  const uint32_t t = (uint32_t)(((uint64_t)r0 * E.Q) >> 32);
  uint32_t lo = 0u, hi = E.n - 1u;   // the row: the smallest j with rows[j] > t (rows[n - 1] = Q > t)
  for (int k = 0; k < 8; ++k) {
    if (lo >= hi) break;
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (rows[mid] > t) hi = mid; else lo = mid + 1u;
  }
  const uint32_t j = lo;
  lo = j * E.n; hi = lo + E.n - 1u;   // the texel: the smallest e of the row with cum[e] > t (the row's last one has)
  for (int k = 0; k < 8; ++k) {
    if (lo >= hi) break;
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (E.cum[mid] > t) hi = mid; else lo = mid + 1u;
  }
  const uint32_t e = lo, i = e - j * E.n;
  e_out = e;
  const float u = (((float)i + a) / (float)E.n) * 2.0f - 1.0f;
  const float v = (((float)j + b) / (float)E.n) * 2.0f - 1.0f;
  float Px, Py, Pz, r2;
  env_unfold(u, v, Px, Py, Pz, r2);
  const float r = sqrtf(r2);
  const float wx = Px / r, wy = Py / r, wz = Pz / r;
  const float cosx = std_max(0.0f, (nx * wx + ny * wy) + nz * wz);
  const float pE = env_density(E, e, r2 * r);
  const float pb = cosx / 3.14159265f;
  const float* T = E.texels + 3 * (size_t)e;
  const float L0 = T[0] * E.scale, L1 = T[1] * E.scale, L2 = T[2] * E.scale;
  const float den = 3.14159265f * pE;
  const float wE = pE / (pE + pb);
  G[0] = ((L0 * cosx) / den) * wE; G[1] = ((L1 * cosx) / den) * wE; G[2] = ((L2 * cosx) / den) * wE;
  const bool skip = cosx == 0.0f || (L0 == 0.0f && L1 == 0.0f && L2 == 0.0f) || !isfinite(G[0]) || !isfinite(G[1]) || !isfinite(G[2]);
  if (skip) {
    ray6[0] = 0.f; ray6[1] = 0.f; ray6[2] = 0.f; ray6[3] = 1.f; ray6[4] = 1.f; ray6[5] = 1.f;
    tmax = -1.0f;
    G[0] = 0.f; G[1] = 0.f; G[2] = 0.f;
    wE_out = 0.0f;
    return false;
  }
  ray6[0] = Ix + nx * 0.001f; ray6[1] = Iy + ny * 0.001f; ray6[2] = Iz + nz * 0.001f; ray6[3] = wx; ray6[4] = wy; ray6[5] = wz;
  tmax = 1e30f;
  wE_out = wE;
  return true;
}
