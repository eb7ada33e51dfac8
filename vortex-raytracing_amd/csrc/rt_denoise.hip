// Guided a-trous filter of denoised path frames (vxrt_render_path_denoised, vxrt_denoise; the definition is in include/vortex_hip.h,
// tests/denoise_ref.py restates it, DESIGN.md s2 "Denoised path frames" has the launch sequence and the measurements).
//
// Per iteration one launch: a 25-tap stencil with stride `step` over three float4 arrays per pixel -- the signal S = (r, g, b, lum), the
// position guide P = (I, hit flag) and the normal guide N.  The luminance travels in the signal's fourth component: the pass that
// writes a signal computes lum() of what it writes, the same three operations the definition applies to a tap, so a tap costs three
// 16-byte loads and no recomputation.  Every tap is gathered from global memory; L1 / L2 serve the 25-fold reuse.  The kernel is bound
// by its arithmetic, not by those loads: the definition's four correctly rounded divisions per tap are half of about 100 VALU
// instructions per tap, and 2,500 per pixel is what an MI355X takes 0.12 ms for at 1920x1080.  A form that stages a 32 x 8 tile and
// its halo in LDS for steps 1 and 2 was measured and is not kept (0.035 ms of a 14.7 ms frame, inside the run-to-run spread: DESIGN.md).
// The last iteration writes the result in the form its caller wants (OUT_RGB: three floats per pixel; OUT_PATH: remodulate with the
// primary hit's Lit and Alb, pack, write pixel and colour), which saves the path frame a pass of its own.
//
// Build: the flags of rt_kernels.hip.  -ffp-contract=off is part of the definition; `/` is the correctly rounded division.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "rt_internal.h"

#define DN_TX 32u   // tile: 32 x 8 pixels, one per thread of a 256-thread workgroup (a wavefront = 2 rows of 32)
#define DN_TY 8u

enum { DN_OUT_SIGNAL = 0, DN_OUT_RGB = 1, DN_OUT_PATH = 2 };

struct DnArgs {
  uint32_t W, rows, step, npow, tiles_x;   // (the grid is one-dimensional: tile = (blockIdx.x % tiles_x, blockIdx.x / tiles_x))
  float sz, sl;                       // sigma_z, sigma_l * 2^-i
  const float4* S; const float4* P; const float4* N;
  float4* out4;                       // DN_OUT_SIGNAL: (r, g, b, lum) per pixel of the window
  float* out3;                        // DN_OUT_RGB: r, g, b per pixel of the window
  const float4* lit; const float4* alb; uint32_t* dst; float* colors; uint32_t y0;   // DN_OUT_PATH: full-frame addressing, window from row y0
};

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// one tap that is inside the window: q's signal, position and normal against the centre's (Pp, Np, lum lp); h = k[dy+2] * k[dx+2]
__device__ __forceinline__ void dn_tap(const float4& Pp, const float4& Np, float lp, const float4& Sq, const float4& Pq, const float4& Nq, float h,
                                       uint32_t npow, float sz, float sl, float& sw, float& sr, float& sg, float& sb) {
  if (Pq.w != 0.f) {
    const float d = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
    float dn = d > 0.f ? d : 0.f;
    for (uint32_t k = 0; k < npow; ++k) dn = dn * dn;
    const float ex = Pq.x - Pp.x, ey = Pq.y - Pp.y, ez = Pq.z - Pp.z;
    const float t = fabsf((Np.x * ex + Np.y * ey) + Np.z * ez) / sz;
    const float wz = 1.0f / (1.0f + t * t);
    const float u = fabsf(lp - Sq.w) / sl;
    const float wc = 1.0f / (1.0f + u * u);
    const float w = ((h * dn) * wz) * wc;
    if (w > 0.f) {
      sw = sw + w;
      sr = sr + w * Sq.x; sg = sg + w * Sq.y; sb = sb + w * Sq.z;
    }
  }
}

// what pixel (x, y) of the window becomes: (r, g, b) = the filtered signal (or the input, see the definition)
template <int OUT>
__device__ __forceinline__ void dn_write(const DnArgs& A, uint32_t x, uint32_t y, float r, float g, float b, bool hit) {
  const size_t p = (size_t)y * A.W + x;
  if constexpr (OUT == DN_OUT_SIGNAL) {
    A.out4[p] = make_float4(r, g, b, dn_lum(r, g, b));
  } else if constexpr (OUT == DN_OUT_RGB) {
    A.out3[3 * p] = r; A.out3[3 * p + 1] = g; A.out3[3 * p + 2] = b;
  } else {
    const float4 D = A.lit[p];
    float cr = D.x, cg = D.y, cb = D.z;   // (a miss: the background)
    if (hit) {
      const float4 a = A.alb[p];
      cr = D.x + a.x * r; cg = D.y + a.y * g; cb = D.z + a.z * b;
    }
    const size_t e = (size_t)x + (size_t)(A.y0 + y) * A.W;
    A.dst[e] = pack_rgb8(cr, cg, cb);
    if (A.colors) { A.colors[3 * e] = cr; A.colors[3 * e + 1] = cg; A.colors[3 * e + 2] = cb; }
  }
}

__device__ __forceinline__ float dn_k(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }

// one iteration: every tap from global memory.  A tap outside the window reads the centre's address instead and is dropped.
template <int OUT>
__global__ __launch_bounds__(256) void rt_dn_iteration_kernel(DnArgs A) {
  const uint32_t bx = blockIdx.x % A.tiles_x, by = blockIdx.x / A.tiles_x;
  const uint32_t x = bx * DN_TX + (threadIdx.x & (DN_TX - 1u)), y = by * DN_TY + threadIdx.x / DN_TX;
  if (x >= A.W || y >= A.rows) return;
  const size_t p = (size_t)y * A.W + x;
  const float4 Sp = A.S[p], Pp = A.P[p];
  if (!(Pp.w != 0.f)) { dn_write<OUT>(A, x, y, Sp.x, Sp.y, Sp.z, false); return; }
  const float4 Np = A.N[p];
  float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t qy = (int64_t)y + (int64_t)dy * A.step;
    if (qy < 0 || qy >= (int64_t)A.rows) continue;   // (uniform over a row of the tile)
    const float ky = dn_k(dy + 2);
    float4 Sq[5], Pq[5], Nq[5];
    bool in[5];
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t qx = (int64_t)x + (int64_t)dx * A.step;
      in[dx + 2] = qx >= 0 && qx < (int64_t)A.W;
      const size_t q = in[dx + 2] ? (size_t)qy * A.W + (size_t)qx : p;
      Sq[dx + 2] = A.S[q]; Pq[dx + 2] = A.P[q]; Nq[dx + 2] = A.N[q];
    }
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx)
      if (in[dx + 2]) dn_tap(Pp, Np, Sp.w, Sq[dx + 2], Pq[dx + 2], Nq[dx + 2], ky * dn_k(dx + 2), A.npow, A.sz, A.sl, sw, sr, sg, sb);
  }
  if (sw > 0.f) dn_write<OUT>(A, x, y, sr / sw, sg / sw, sb / sw, true);
  else dn_write<OUT>(A, x, y, Sp.x, Sp.y, Sp.z, true);
}

// the signal of a stand-alone call: (r, g, b) -> (r, g, b, lum)
__global__ __launch_bounds__(256) void rt_dn_load_kernel(uint32_t n, const float* __restrict__ sig3, float4* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const float r = sig3[3 * (size_t)t], g = sig3[3 * (size_t)t + 1], b = sig3[3 * (size_t)t + 2];
  out[t] = make_float4(r, g, b, dn_lum(r, g, b));
}

// the end of a denoised path frame's tail in place of rt_path_final_kernel (which stays the end of every other path frame): c as that
// kernel computes it, E = A > 0 ? (c - D) / A : 0 per channel with its luminance, and the guide outputs.  No pack.
__global__ __launch_bounds__(256) void rt_dn_demodulate_kernel(uint32_t n, uint32_t W, uint32_t y0, const float4* __restrict__ geo, const float4* __restrict__ nrm,
    const float4* __restrict__ lit, const float4* __restrict__ alb, const float4* __restrict__ acc, uint32_t spp, uint32_t flat, float4* __restrict__ sig,
    vxrt_path_aov_t aov) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint32_t x = t % W, y = y0 + t / W;
  const size_t e = (size_t)x + (size_t)y * W;
  const float4 D = lit[t], G = geo[t];
  const bool hit = G.w != 0.f;
  float r = D.x, g = D.y, b = D.z;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), N = a, E = a;
  if (hit) {
    if (flat) { for (uint32_t s = 1; s < spp; ++s) { r = r + D.x; g = g + D.y; b = b + D.z; } }
    else { const float4 c = acc[t]; r = c.x; g = c.y; b = c.z; }
    const float f = (float)spp;
    r = r / f; g = g / f; b = b / f;
    a = alb[t]; N = nrm[t];
    E.x = a.x > 0.f ? (r - D.x) / a.x : 0.f;
    E.y = a.y > 0.f ? (g - D.y) / a.y : 0.f;
    E.z = a.z > 0.f ? (b - D.z) / a.z : 0.f;
    E.w = dn_lum(E.x, E.y, E.z);
  }
  if (sig) sig[t] = E;
  if (aov.noisy) { aov.noisy[3 * e] = r; aov.noisy[3 * e + 1] = g; aov.noisy[3 * e + 2] = b; }
  if (aov.direct) { aov.direct[3 * e] = D.x; aov.direct[3 * e + 1] = D.y; aov.direct[3 * e + 2] = D.z; }
  if (aov.albedo) { aov.albedo[3 * e] = a.x; aov.albedo[3 * e + 1] = a.y; aov.albedo[3 * e + 2] = a.z; }
  if (aov.position) { float* o = aov.position + 4 * e; o[0] = hit ? G.x : 0.f; o[1] = hit ? G.y : 0.f; o[2] = hit ? G.z : 0.f; o[3] = hit ? G.w : 0.f; }
  if (aov.normal) { float* o = aov.normal + 4 * e; o[0] = N.x; o[1] = N.y; o[2] = N.z; o[3] = 0.f; }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
bool dn_params_ok(const vxrt_denoise_params_t* dn) {
  return dn && dn->iterations <= VXRT_DENOISE_MAX_ITERATIONS && dn->normal_power <= 7u && dn->sigma_z > 0.0f && dn->sigma_l > 0.0f;   // (false for NaN)
}

template <int OUT>
static void dn_launch_iteration(hipStream_t s, const DnArgs& A) {
  const dim3 grid(A.tiles_x * ((A.rows + DN_TY - 1u) / DN_TY)), block(256);
  hipLaunchKernelGGL((rt_dn_iteration_kernel<OUT>), grid, block, 0, s, A);
}

// iterations >= 1 passes from sig[0]; `last` holds the outputs of the final pass (DN_OUT_RGB or DN_OUT_PATH)
static int dn_filter(hipStream_t s, uint32_t W, uint32_t rows, const vxrt_denoise_params_t* dn, float4* const sig[2], const float4* P, const float4* N,
                     int last_out, DnArgs last) {
  const uint32_t tiles_x = (W + DN_TX - 1u) / DN_TX;   // (W * rows < 2^31: at most 2^28 + 2^26 tiles)
  for (uint32_t i = 0; i < dn->iterations; ++i) {
    DnArgs A = last;
    A.W = W; A.rows = rows; A.tiles_x = tiles_x; A.step = 1u << i; A.npow = dn->normal_power;
    A.sz = dn->sigma_z; A.sl = dn->sigma_l * (1.0f / (float)(1u << i));
    A.S = sig[i & 1u]; A.P = P; A.N = N; A.out4 = sig[(i + 1u) & 1u];
    if (i + 1u < dn->iterations) dn_launch_iteration<DN_OUT_SIGNAL>(s, A);
    else if (last_out == DN_OUT_RGB) dn_launch_iteration<DN_OUT_RGB>(s, A);
    else dn_launch_iteration<DN_OUT_PATH>(s, A);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int dn_launch_demodulate(hipStream_t s, uint32_t n, uint32_t W, uint32_t y0, const float4* geo, const float4* nrm, const float4* lit, const float4* alb,
                         const float4* acc, uint32_t spp, uint32_t flat, float4* sig, const vxrt_path_aov_t* aov) {
  vxrt_path_aov_t o;
  memset(&o, 0, sizeof(o));
  if (aov) o = *aov;
  hipLaunchKernelGGL(rt_dn_demodulate_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, n, W, y0, geo, nrm, lit, alb, acc, spp, flat, sig, o);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int dn_launch_path_filter(hipStream_t s, uint32_t W, uint32_t rows, uint32_t y0, const vxrt_denoise_params_t* dn, float4* const sig[2], const float4* geo,
                          const float4* nrm, const float4* lit, const float4* alb, uint32_t* dst, float* colors) {
  DnArgs last{};
  last.lit = lit; last.alb = alb; last.dst = dst; last.colors = colors; last.y0 = y0;
  return dn_filter(s, W, rows, dn, sig, geo, nrm, DN_OUT_PATH, last);
}

extern "C" {

uint64_t vxrt_denoise_scratch_bytes(uint32_t width, uint32_t rows) { return 32ull * width * rows; }

int vxrt_denoise(uint32_t width, uint32_t rows, const float* signal, const float* position, const float* normal, const vxrt_denoise_params_t* dn,
                 float* out, void* scratch, uint64_t scratch_bytes, void* stream) {
  const uint64_t n = (uint64_t)width * rows;
  if (!dn_params_ok(dn) || n > 0x7fffffffull) return -1;
  if (n == 0) return 0;
  if (!signal || !position || !normal || !out || out == signal || (((uintptr_t)position | (uintptr_t)normal) & 15u) != 0) return -1;
  if (dn->iterations && (!scratch || ((uintptr_t)scratch & 15u) != 0 || scratch_bytes < vxrt_denoise_scratch_bytes(width, rows))) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (dn->iterations == 0) return hipMemcpyAsync(out, signal, n * 12u, hipMemcpyDeviceToDevice, s) == hipSuccess ? 0 : -1;
  float4* const sig[2] = {(float4*)scratch, (float4*)scratch + n};
  hipLaunchKernelGGL(rt_dn_load_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, s, (uint32_t)n, signal, sig[0]);
  DnArgs last{};
  last.out3 = out;
  return dn_filter(s, width, rows, dn, sig, (const float4*)position, (const float4*)normal, DN_OUT_RGB, last);
}

}
