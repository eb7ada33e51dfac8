// Environment light (include/vortex_hip.h, "Environment light"): the map object and its table, and the two steps alone
// (vxrt_envmap_lookup, vxrt_env_rays).  The frame that the map lights is rt_path.hip's; the device arithmetic both units share is
// rt_env.h.  None of it is timed by bench.py.  Same build flags (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "rt_internal.h"
#include "rt_shading.h"
#include "rt_env.h"

// THE TABLE of a map of n x n texels, at most 65,536: ONE workgroup of 1,024 threads, so that neither the maximum nor the scan waits for
// another workgroup.  Thread i owns the texels e = k * 1024 + i.  Three sweeps: the weights' maximum (no weight is below zero, but a -0
// texel gives a weight of -0, whose bits would beat every positive float: with the sign cleared, which changes no other weight, floats order
// as their bits do and an integer maximum in LDS is exact in any order); q; the inclusive scan in passes of 1,024 entries with a running
// carry, as rt_path_scan_kernel carries it.
__global__ __launch_bounds__(1024) void rt_env_table_kernel(uint32_t n, const float* __restrict__ texels, uint32_t* __restrict__ q, uint32_t* __restrict__ cum,
    uint32_t* __restrict__ Q_out) {
  __shared__ uint32_t s_max;
  __shared__ uint32_t s_w[16];
  const uint32_t nn = n * n;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_max = 0u;
  __syncthreads();
  uint32_t m = 0u;
  for (uint32_t e = threadIdx.x; e < nn; e += 1024u) {
    const float* T = texels + 3 * (size_t)e;
    m = max(m, __float_as_uint(fabsf(env_texel_weight(n, e % n, e / n, T[0], T[1], T[2]))));
  }
  atomicMax(&s_max, m);
  __syncthreads();
  const float wmax = __uint_as_float(s_max);
  uint32_t carry = 0u;
  for (uint32_t base = 0; base < nn; base += 1024u) {   // (uniform trip count: nn is the same in every thread)
    const uint32_t e = base + threadIdx.x;
    uint32_t v = 0u;
    if (e < nn) {
      const float* T = texels + 3 * (size_t)e;
      const float w = env_texel_weight(n, e % n, e / n, T[0], T[1], T[2]);
      v = max(1u, (uint32_t)((w / wmax) * 65535.0f));
      q[e] = v;
    }
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += y; }
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = carry, pass_sum = 0u;
    for (uint32_t w = 0; w < 16u; ++w) { const uint32_t x = s_w[w]; if (w < wave) before += x; pass_sum += x; }
    if (e < nn) cum[e] = before + inc;
    carry += pass_sum;
    __syncthreads();   // (s_w is written again by the next pass)
  }
  if (threadIdx.x == 0) *Q_out = carry;
}

// vxrt_envmap_lookup: Env(w), e and pe(w) of n caller-supplied directions, one per thread
__global__ __launch_bounds__(256) void rt_env_lookup_kernel(EnvTab E, uint32_t n, const float* __restrict__ dirs, float* __restrict__ radiance3,
    uint32_t* __restrict__ texel, float* __restrict__ pdf) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float* d = dirs + 3 * (size_t)i;
  float L[3], pe;
  const uint32_t e = env_lookup(E, d[0], d[1], d[2], L, pe);
  float* o = radiance3 + 3 * (size_t)i;
  o[0] = L[0]; o[1] = L[1]; o[2] = L[2];
  texel[i] = e;
  pdf[i] = pe;
}

// vxrt_env_rays: the environment ray of n caller-supplied (I, N') and hash outputs, one per thread (no thread leaves before the barrier
// that ends the staging of the row ends)
__global__ __launch_bounds__(256) void rt_env_rays_kernel(EnvTab E, uint32_t n, const float* __restrict__ points, const uint32_t* __restrict__ seeds,
    float* __restrict__ rays, float* __restrict__ tmax, float* __restrict__ weight3, uint32_t* __restrict__ texel, float* __restrict__ mis) {
  __shared__ uint32_t s_rows[ENV_MAX_N];
  env_stage_rows(E, s_rows);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float* pt = points + (size_t)i * 6;
  float e6[6], tm, G[3], wE;
  uint32_t e;
  env_sample(E, s_rows, seeds[i], pt[0], pt[1], pt[2], pt[3], pt[4], pt[5], e6, tm, G, e, wE);
  float* o = rays + (size_t)i * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = e6[k];
  tmax[i] = tm;
  weight3[3 * (size_t)i] = G[0]; weight3[3 * (size_t)i + 1] = G[1]; weight3[3 * (size_t)i + 2] = G[2];
  texel[i] = e;
  mis[i] = wE;
}

static bool env_scale_ok(float scale) { return scale >= 0.0f && std::isfinite(scale); }

extern "C" {

// Host texels -> the map.  Everything the texels can get wrong is refused before anything is allocated; then one upload, the table
// kernel, and one read of Q, which is the synchronisation with `stream` the header promises.
int vxrt_envmap_create(const float* texels, uint32_t n, void* stream, vxrt_envmap_t** map) {
  if (!texels || !map || n < 4u || n > ENV_MAX_N || (n & (n - 1u)) != 0u) return -1;
  const uint32_t nn = n * n;
  bool positive = false;
  for (uint32_t e = 0; e < nn; ++e) {
    const float* T = texels + 3 * (size_t)e;
    for (int k = 0; k < 3; ++k) {
      if (!(T[k] >= 0.0f) || !std::isfinite(T[k])) return -1;
      positive = positive || T[k] > 0.0f;
    }
    if (!std::isfinite(env_texel_weight(n, e % n, e / n, T[0], T[1], T[2]))) return -1;
  }
  if (!positive) return -1;
  hipStream_t s = (hipStream_t)stream;
  vxrt_envmap* m = new vxrt_envmap();
  uint32_t* dQ = nullptr;
  bool ok = hipMalloc((void**)&m->texels, (size_t)nn * 12) == hipSuccess && hipMalloc((void**)&m->q, (size_t)nn * 4) == hipSuccess &&
            hipMalloc((void**)&m->cum, (size_t)nn * 4) == hipSuccess && hipMalloc((void**)&dQ, 4) == hipSuccess;
  ok = ok && hipMemcpyAsync(m->texels, texels, (size_t)nn * 12, hipMemcpyHostToDevice, s) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(rt_env_table_kernel, dim3(1), dim3(1024), 0, s, n, (const float*)m->texels, m->q, m->cum, dQ);
    ok = hipGetLastError() == hipSuccess;
  }
  uint32_t Q = 0u;
  ok = ok && hipMemcpyAsync(&Q, dQ, 4, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && Q != 0u;
  (void)hipFree(dQ);
  if (!ok) {
    (void)hipFree(m->texels); (void)hipFree(m->q); (void)hipFree(m->cum);
    delete m;
    return -1;
  }
  m->n = n; m->Q = Q;
  *map = m;
  return 0;
}

// (the map must outlive the frames that read it: nothing is waited for here beyond what hipFree itself waits for)
int vxrt_envmap_destroy(vxrt_envmap_t* map) {
  if (!map) return -1;
  (void)hipFree(map->texels); (void)hipFree(map->q); (void)hipFree(map->cum);
  delete map;
  return 0;
}

uint64_t vxrt_envmap_bytes(const vxrt_envmap_t* map) { return map ? (uint64_t)map->n * map->n * 20u : 0u; }

int vxrt_envmap_read(vxrt_envmap_t* map, uint32_t* q, uint32_t* cum, void* stream) {
  if (!map || map->n == 0u) return -1;
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)map->n * map->n * 4;
  if (q && hipMemcpyAsync(q, map->q, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
  if (cum && hipMemcpyAsync(cum, map->cum, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
  return hipStreamSynchronize(s) == hipSuccess ? 0 : -1;
}

int vxrt_envmap_lookup(vxrt_envmap_t* map, uint64_t n, const float* dirs, float scale, float* radiance3, uint32_t* texel, float* pdf, void* stream) {
  if (!map || map->n == 0u || !dirs || !radiance3 || !texel || !pdf || !env_scale_ok(scale) || n >= 0x80000000ull) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_env_lookup_kernel, dim3(((uint32_t)n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, env_tab(map, scale), (uint32_t)n, dirs, radiance3,
                     texel, pdf);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int vxrt_env_rays(vxrt_envmap_t* map, uint64_t n, const float* points, const uint32_t* seeds, float scale, float* rays, float* tmax, float* weight3, uint32_t* texel,
                  float* mis, void* stream) {
  if (!map || map->n == 0u || !points || !seeds || !rays || !tmax || !weight3 || !texel || !mis || !env_scale_ok(scale) || n >= 0x80000000ull) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(rt_env_rays_kernel, dim3(((uint32_t)n - 1u) / 256u + 1u), dim3(256), 0, (hipStream_t)stream, env_tab(map, scale), (uint32_t)n, points, seeds,
                     rays, tmax, weight3, texel, mis);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
