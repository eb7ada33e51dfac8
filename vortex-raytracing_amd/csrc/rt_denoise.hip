// Guided a-trous filter of denoised path frames (vxrt_render_path_denoised, vxrt_denoise; the definition is in include/vortex_hip.h,
// tests/denoise_ref.py restates it, DESIGN.md s2 "Denoised path frames" has the launch sequence and the measurements), and below it the
// temporal accumulation that may precede it (vxrt_render_path_temporal, vxrt_temporal_accumulate; DESIGN.md s2 "Temporal accumulation"),
// and below that the variance guidance that builds on both (vxrt_render_path_variance; DESIGN.md s2 "Variance guidance").
//
// One of each: one guided pass (rt_dn_iteration_kernel<OUT, VAR>, VAR = the variance-guided form, with one tap and one write function),
// one host loop that runs it in ping-pong (dn_filter), one accumulation kernel (rt_tp_accumulate_kernel<OUT, MOTION, MOMENTS>), and one
// door for a path frame (render_denoise_tail, which alone knows what follows what); a new form is an argument of these, not a copy.
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
#include <cmath>
#include <type_traits>
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

// atrous_v (VAR): sl = sigma_l (not halved: the variance shrinks instead); S and out4 hold (r, g, b, V)
struct VrArgs : DnArgs {
  float eps;
  float* outv;                        // DN_OUT_RGB: the filtered variance, optional
};
template <bool VAR> using DnKernelArgs = std::conditional_t<VAR, VrArgs, DnArgs>;   // (the plain form does not carry eps / outv)

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the two guide factors of neighbour q against the centre (Pp, Np): dn = max(Np . Nq, 0) after npow squarings, wz = 1 / (1 + t * t) with
// t = |Np . (Pq - Pp)| / sz.  Returned apart: how they are multiplied (with what, in which order) is each caller's part of the definition.
struct DnGuide { float dn, wz; };
__device__ __forceinline__ DnGuide dn_guide_weights(const float4& Pp, const float4& Np, const float4& Pq, const float4& Nq, uint32_t npow, float sz) {
  const float d = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
  float dn = d > 0.f ? d : 0.f;
  for (uint32_t k = 0; k < npow; ++k) dn = dn * dn;
  const float ex = Pq.x - Pp.x, ey = Pq.y - Pp.y, ez = Pq.z - Pp.z;
  const float t = fabsf((Np.x * ex + Np.y * ey) + Np.z * ez) / sz;
  const float wz = 1.0f / (1.0f + t * t);
  return DnGuide{dn, wz};
}

// one tap that is inside the window: q's signal, position and normal against the centre's (Pp, Np, lum lp); h = k[dy+2] * k[dx+2].
// VAR: Sq.w is q's variance, so lum() of the tap is recomputed, sl is the centre's luminance scale, and sv sums the variance.
// (sv is a pack of one float with VAR and of none without: a plain tap with a fifth sum it never touches compiles to other code.)
template <bool VAR, class... SV>
__device__ __forceinline__ void dn_tap(const float4& Pp, const float4& Np, float lp, const float4& Sq, const float4& Pq, const float4& Nq, float h,
                                       uint32_t npow, float sz, float sl, float& sw, float& sr, float& sg, float& sb, SV&... sv) {
  if (Pq.w != 0.f) {
    const DnGuide G = dn_guide_weights(Pp, Np, Pq, Nq, npow, sz);
    const float lq = VAR ? dn_lum(Sq.x, Sq.y, Sq.z) : Sq.w;
    const float u = fabsf(lp - lq) / sl;
    const float wc = 1.0f / (1.0f + u * u);
    const float w = ((h * G.dn) * G.wz) * wc;
    if (w > 0.f) {
      sw = sw + w;
      sr = sr + w * Sq.x; sg = sg + w * Sq.y; sb = sb + w * Sq.z;
      if constexpr (VAR) ((sv = sv + (w * w) * Sq.w), ...);
    }
  }
}

// what pixel (x, y) of the window becomes: (r, g, b) = the filtered signal (or the input, see the definition); VAR: v = its variance
template <int OUT, bool VAR = false>
__device__ __forceinline__ void dn_write(const DnKernelArgs<VAR>& A, uint32_t x, uint32_t y, float r, float g, float b, bool hit, float v = 0.f) {
  const size_t p = (size_t)y * A.W + x;
  if constexpr (OUT == DN_OUT_SIGNAL) {
    A.out4[p] = make_float4(r, g, b, VAR ? v : dn_lum(r, g, b));
  } else if constexpr (OUT == DN_OUT_RGB) {
    A.out3[3 * p] = r; A.out3[3 * p + 1] = g; A.out3[3 * p + 2] = b;
    if constexpr (VAR) { if (A.outv) A.outv[p] = v; }
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

__device__ __forceinline__ float vr_kk(int i) { return i == 1 ? 0.5f : 0.25f; }

// one iteration: every tap from global memory.  A tap outside the window reads the centre's address instead and is dropped.
// VAR: one pass of atrous_v (see "Variance guidance" below) -- the 3 x 3 prefilter of the centre's variance in front, the other tap.
template <int OUT, bool VAR>
__global__ __launch_bounds__(256) void rt_dn_iteration_kernel(DnKernelArgs<VAR> A) {
  const uint32_t bx = blockIdx.x % A.tiles_x, by = blockIdx.x / A.tiles_x;
  const uint32_t x = bx * DN_TX + (threadIdx.x & (DN_TX - 1u)), y = by * DN_TY + threadIdx.x / DN_TX;
  if (x >= A.W || y >= A.rows) return;
  const size_t p = (size_t)y * A.W + x;
  const float4 Sp = A.S[p], Pp = A.P[p];
  if (!(Pp.w != 0.f)) { dn_write<OUT, VAR>(A, x, y, Sp.x, Sp.y, Sp.z, false, Sp.w); return; }
  const float4 Np = A.N[p];
  float lp = Sp.w, sl = A.sl;   // the centre's luminance and the luminance scale of its taps
  if constexpr (VAR) {
    // the prefiltered variance of the centre: 3 x 3 at stride 1, hit taps of the window only (a tap outside reads the centre and is dropped)
    float gw = 0.f, gs = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const int64_t qy = (int64_t)y + dy;
      const bool iny = qy >= 0 && qy < (int64_t)A.rows;
      float Vq[3], Fq[3];
      bool in[3];
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int64_t qx = (int64_t)x + dx;
        in[dx + 1] = iny && qx >= 0 && qx < (int64_t)A.W;
        const size_t q = in[dx + 1] ? (size_t)qy * A.W + (size_t)qx : p;
        Vq[dx + 1] = A.S[q].w; Fq[dx + 1] = A.P[q].w;
      }
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
        if (in[dx + 1] && Fq[dx + 1] != 0.f) {
          const float c = vr_kk(dy + 1) * vr_kk(dx + 1);
          gw = gw + c;
          gs = gs + c * Vq[dx + 1];
        }
    }
    const float g = gs / gw;
    sl = A.sl * sqrtf(g) + A.eps;
    lp = dn_lum(Sp.x, Sp.y, Sp.z);
  }
  float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
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
      if (in[dx + 2]) {
        if constexpr (VAR) dn_tap<VAR>(Pp, Np, lp, Sq[dx + 2], Pq[dx + 2], Nq[dx + 2], ky * dn_k(dx + 2), A.npow, A.sz, sl, sw, sr, sg, sb, sv);
        else dn_tap<VAR>(Pp, Np, lp, Sq[dx + 2], Pq[dx + 2], Nq[dx + 2], ky * dn_k(dx + 2), A.npow, A.sz, sl, sw, sr, sg, sb);
      }
  }
  if (sw > 0.f) dn_write<OUT, VAR>(A, x, y, sr / sw, sg / sw, sb / sw, true, VAR ? sv / (sw * sw) : 0.f);
  else dn_write<OUT, VAR>(A, x, y, Sp.x, Sp.y, Sp.z, true, Sp.w);
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
// Temporal accumulation (vxrt_temporal_accumulate, vxrt_render_path_temporal; the definition is in include/vortex_hip.h,
// tests/temporal_ref.py restates it).  One launch per frame, one thread per pixel of a 32 x 8 tile as in the a-trous kernel: the pixel's
// hit point goes through the previous camera's reciprocal basis (computed on the host in double, passed by value), and up to four taps of
// three 16-byte loads each are gathered from the previous frame's set of history buffers.  Reprojection is a translation locally, so
// the lanes of a row read neighbouring addresses and every history line is used by the four pixels around it out of L1 / L2.  The taps'
// loads are issued before any of them is tested (a tap outside the window reads the pixel's own address and is dropped).  Almost no
// arithmetic: the pass is bound by its 160 B per pixel of compulsory traffic (E, P, N in; the signal and the three history entries out;
// HE, HP, HN of the previous frame once each).  The MOTION instantiations (vxrt_temporal_accumulate_motion, vxrt_render_path_temporal_motion;
// tests/motion_ref.py) read 32 B more per pixel: the previous position and normal of the pixel's surface point.
// ---------------------------------------------------------------------------------------------
enum { TP_OUT_SIGNAL = 0, TP_OUT_LEN = 1, TP_OUT_PATH = 2 };

struct TpArgs {
  uint32_t W, rows, tiles_x, have, max_len;     // have: the history is not empty
  float fW, fH, fy0, frows;                     // (float) of the frame's size, the window's first row and its number of rows
  float pos[3], Rr[3], Ur[3], Fr[3], vp[2];     // previous camera: position, reciprocal basis, viewplane
  float alpha_min, sigma_z, normal_min;
  const float4* E4; const float* E3;            // the frame's signal (E, lum) | a stand-alone call's, 3 floats per pixel
  const float4* P; const float4* N;
  const float4* he; const float4* hp; const float4* hn;   // the previous frame's set
  float4* he_o; float4* hp_o; float4* hn_o;               // this frame's
  float4* sig;                                  // TP_OUT_SIGNAL: (out.rgb, lum) for the first a-trous pass (may be E4: a pixel reads only its own entry)
  float* out4;                                  // TP_OUT_LEN: (out.rgb, len)
  DnArgs path;                                  // TP_OUT_PATH: lit, alb, dst, colors, y0, W
};

// the step with motion, T_m (MOTION instantiations): the two guides more, per pixel of the window
struct TpMotionArgs : TpArgs { const float4* Q; const float4* Nq; };
// the step with moments, T_v (MOMENTS instantiations, over either of the two): HM = (m1, m2) of the previous frame's set and of this frame's
template <class Base> struct TpMomentArgs : Base { const float2* hm; float2* hm_o; };
template <bool MOTION, bool MOMENTS> struct TpKernelArgs { using base = std::conditional_t<MOTION, TpMotionArgs, TpArgs>; using type = std::conditional_t<MOMENTS, TpMomentArgs<base>, base>; };

__device__ __forceinline__ float tp_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// MOTION: the pixel's previous position Q and previous normal N' (two 16-byte loads more, issued with the pixel's other loads) take the
// place of its hit point and normal in the reprojection and in the two tap tests; the history written is the current frame's as ever.
// MOMENTS (the header's "Variance guidance"): the first and second luminance moments travel with the signal -- one 8-byte load per tap,
// issued with the tap's other loads, two multiply-adds per kept tap, one 8-byte store; nothing of the step itself changes.
template <int OUT, bool MOTION = false, bool MOMENTS = false>
__global__ __launch_bounds__(256) void rt_tp_accumulate_kernel(typename TpKernelArgs<MOTION, MOMENTS>::type A) {
  const uint32_t bx = blockIdx.x % A.tiles_x, by = blockIdx.x / A.tiles_x;
  const uint32_t x = bx * DN_TX + (threadIdx.x & (DN_TX - 1u)), y = by * DN_TY + threadIdx.x / DN_TX;
  if (x >= A.W || y >= A.rows) return;
  const size_t p = (size_t)y * A.W + x;
  float er, eg, eb;
  if constexpr (OUT == TP_OUT_LEN) { er = A.E3[3 * p]; eg = A.E3[3 * p + 1]; eb = A.E3[3 * p + 2]; }
  else { const float4 e = A.E4[p]; er = e.x; eg = e.y; eb = e.z; }
  const float4 Pp = A.P[p], Np = A.N[p];
  float4 Qp = Pp, Nq = Np;   // what the reprojection and the tap tests go by
  if constexpr (MOTION) { Qp = A.Q[p]; Nq = A.Nq[p]; }
  const bool hit = Pp.w != 0.f;
  float orr = er, og = eg, ob = eb, olen = hit ? 1.f : 0.f;
  float lE = 0.f, m1 = 0.f, m2 = 0.f;   // (MOMENTS)
  if constexpr (MOMENTS) {
    lE = dn_lum(er, eg, eb);
    if (hit) { m1 = lE; m2 = lE * lE; }
  }
  if (hit && A.have && (!MOTION || Qp.w != 0.f)) {
    const float dx = Qp.x - A.pos[0], dy = Qp.y - A.pos[1], dz = Qp.z - A.pos[2];
    const float a = tp_dot(dx, dy, dz, A.Rr[0], A.Rr[1], A.Rr[2]);
    const float b = tp_dot(dx, dy, dz, A.Ur[0], A.Ur[1], A.Ur[2]);
    const float c = tp_dot(dx, dy, dz, A.Fr[0], A.Fr[1], A.Fr[2]);
    if (c > 0.f) {
      const float fx = (((a / c) / A.vp[0]) + 0.5f) * A.fW - 0.5f;
      const float fy = ((((b / c) / A.vp[1]) + 0.5f) * A.fH - 0.5f) - A.fy0;
      if (fx > -1.f && fx < A.fW && fy > -1.f && fy < A.frows) {
        const float flx = floorf(fx), fly = floorf(fy);
        const float tx = fx - flx, ty = fy - fly;
        const int64_t x0 = (int64_t)flx, yy = (int64_t)fly;   // (-1 .. W - 1, -1 .. rows - 1)
        float4 He[4], Hp[4], Hn[4];
        float2 Hm[4];
        bool in[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t qx = x0 + (k & 1), qy = yy + (k >> 1);
          in[k] = qx >= 0 && qx < (int64_t)A.W && qy >= 0 && qy < (int64_t)A.rows;
          const size_t q = in[k] ? (size_t)qy * A.W + (size_t)qx : p;
          He[k] = A.he[q]; Hp[k] = A.hp[q]; Hn[k] = A.hn[q];
          if constexpr (MOMENTS) Hm[k] = A.hm[q];
        }
        float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!in[k]) continue;
          if (!(Hp[k].w != 0.f) || !(He[k].w > 0.f)) continue;
          if (!(tp_dot(Nq.x, Nq.y, Nq.z, Hn[k].x, Hn[k].y, Hn[k].z) >= A.normal_min)) continue;
          const float ex = Hp[k].x - Qp.x, ey = Hp[k].y - Qp.y, ez = Hp[k].z - Qp.z;
          if (!(fabsf(tp_dot(Nq.x, Nq.y, Nq.z, ex, ey, ez)) / A.sigma_z <= 1.f)) continue;
          const float w = ((k & 1) ? tx : 1.f - tx) * ((k >> 1) ? ty : 1.f - ty);
          if (w > 0.f) {
            sw = sw + w;
            sr = sr + w * He[k].x; sg = sg + w * He[k].y; sb = sb + w * He[k].z;
            sl = sl + w * He[k].w;
            if constexpr (MOMENTS) { s1 = s1 + w * Hm[k].x; s2 = s2 + w * Hm[k].y; }
          }
        }
        if (sw > 0.f) {
          const float hr = sr / sw, hg = sg / sw, hb = sb / sw, L = sl / sw;
          const float L1 = std_min(L + 1.f, (float)A.max_len);
          const float r1 = 1.f / L1;
          const float al = r1 < A.alpha_min ? A.alpha_min : r1;
          orr = hr + al * (er - hr); og = hg + al * (eg - hg); ob = hb + al * (eb - hb);
          olen = L1;
          if constexpr (MOMENTS) {
            const float M1 = s1 / sw, M2 = s2 / sw;
            m1 = M1 + al * (lE - M1); m2 = M2 + al * (lE * lE - M2);
          }
        }
      }
    }
  }
  A.he_o[p] = make_float4(orr, og, ob, olen);
  A.hp_o[p] = Pp;
  A.hn_o[p] = Np;
  if constexpr (MOMENTS) A.hm_o[p] = make_float2(m1, m2);
  if constexpr (OUT == TP_OUT_SIGNAL) A.sig[p] = make_float4(orr, og, ob, dn_lum(orr, og, ob));
  else if constexpr (OUT == TP_OUT_LEN) { float* o = A.out4 + 4 * p; o[0] = orr; o[1] = og; o[2] = ob; o[3] = olen; }
  else dn_write<DN_OUT_PATH>(A.path, x, y, orr, og, ob, hit);
}

// ---------------------------------------------------------------------------------------------
// Variance guidance (vxrt_history_variance, vxrt_denoise_variance, vxrt_render_path_variance; the definition is the header's "Variance
// guidance", tests/variance_ref.py restates it).  Two kernels on the 32 x 8 tile, one pixel per thread.
//   rt_dn_iteration_kernel<OUT, true> (above)
//                           one pass of atrous_v.  The variance travels in the signal's fourth component, S = (r, g, b, V), in place of
//                           the luminance the plain filter keeps there: a tap stays three 16-byte loads, lum() of a tap is recomputed
//                           (three operations against about 100), and the nine prefilter taps are two 4-byte loads each (V and the hit
//                           flag) from lines the 25 taps of step 1 fetch anyway.  No buffer of its own, no fourth gather per tap.
//   rt_vr_initial_kernel    V0 of the history's current set.  A pixel with a long history takes the temporal variance of its own moments:
//                           four loads and five operations.  Only a pixel with a short history walks the (2 radius + 1)^2 window of three
//                           16-byte loads per tap.  The walk sits behind `if (need)`: a wavefront in which no lane needs it branches over
//                           the loop on an empty exec mask, and after the first few frames that is nearly every wavefront; inside a
//                           wavefront that does walk, the trip count is uniform (radius), only the lanes that walk differ.
// ---------------------------------------------------------------------------------------------
struct VrInitArgs {
  uint32_t W, rows, tiles_x, npow, radius, y0;
  float sz, fmin;                               // sigma_z, (float)min_len
  const float4* he; const float2* hm; const float4* hp; const float4* hn;   // the history's current set
  float* out; uint32_t out_stride;              // V0 of pixel p of the window goes to out[p * out_stride] (1: a float buffer; 4: the signal's w) ...
  float* frame_out;                             // ... and, optional, to the frame's `variance` output (full-frame addressing, rows from y0)
};

__global__ __launch_bounds__(256) void rt_vr_initial_kernel(VrInitArgs A) {
  const uint32_t bx = blockIdx.x % A.tiles_x, by = blockIdx.x / A.tiles_x;
  const uint32_t x = bx * DN_TX + (threadIdx.x & (DN_TX - 1u)), y = by * DN_TY + threadIdx.x / DN_TX;
  if (x >= A.W || y >= A.rows) return;
  const size_t p = (size_t)y * A.W + x;
  const float4 Ap = A.he[p], Pp = A.hp[p];
  const float2 Mp = A.hm[p];
  const bool hit = Pp.w != 0.f;
  const float vd = Mp.y - Mp.x * Mp.x;
  const float vt = vd < 0.f ? 0.f : vd;         // max(vd, 0)
  float v0 = hit ? vt : 0.f;
  const bool need = hit && !(Ap.w >= A.fmin);
  if (need) {
    const float4 Np = A.hn[p];
    const int r = (int)A.radius;
    float sw = 0.f, s1 = 0.f, s2 = 0.f;
    for (int dy = -r; dy <= r; ++dy) {
      const int64_t qy = (int64_t)y + dy;
      if (qy < 0 || qy >= (int64_t)A.rows) continue;
      for (int dx = -r; dx <= r; ++dx) {
        const int64_t qx = (int64_t)x + dx;
        if (qx < 0 || qx >= (int64_t)A.W) continue;
        const size_t q = (size_t)qy * A.W + (size_t)qx;
        const float4 Pq = A.hp[q], Nq = A.hn[q], Aq = A.he[q];
        if (!(Pq.w != 0.f)) continue;
        const DnGuide G = dn_guide_weights(Pp, Np, Pq, Nq, A.npow, A.sz);
        const float w = G.dn * G.wz;
        if (w > 0.f) {
          const float l = dn_lum(Aq.x, Aq.y, Aq.z);
          sw = sw + w;
          s1 = s1 + w * l;
          s2 = s2 + w * (l * l);
        }
      }
    }
    if (sw > 0.f) {
      const float a1 = s1 / sw;
      const float sd = s2 / sw - a1 * a1;
      const float vs = sd < 0.f ? 0.f : sd;
      v0 = vs * (A.fmin / Ap.w);
    }
  }
  if (A.out) A.out[p * A.out_stride] = v0;
  if (A.frame_out) A.frame_out[(size_t)x + (size_t)(A.y0 + y) * A.W] = v0;
}

// the signal of a stand-alone call: (r, g, b), V -> (r, g, b, V)
__global__ __launch_bounds__(256) void rt_vr_load_kernel(uint32_t n, const float* __restrict__ sig3, const float* __restrict__ var, float4* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  out[t] = make_float4(sig3[3 * (size_t)t], sig3[3 * (size_t)t + 1], sig3[3 * (size_t)t + 2], var[t]);
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
bool dn_params_ok(const vxrt_denoise_params_t* dn) {
  return dn && dn->iterations <= VXRT_DENOISE_MAX_ITERATIONS && dn->normal_power <= 7u && dn->sigma_z > 0.0f && dn->sigma_l > 0.0f;   // (false for NaN)
}

// the one-dimensional grid of 32 x 8 tiles over a window of W x rows pixels (W * rows < 2^31: at most 2^28 + 2^26 tiles)
static uint32_t dn_tiles_x(uint32_t W) { return (W + DN_TX - 1u) / DN_TX; }
static dim3 dn_grid(uint32_t W, uint32_t rows) { return dim3(dn_tiles_x(W) * ((rows + DN_TY - 1u) / DN_TY)); }

template <bool VAR>
static void dn_launch_iteration(hipStream_t s, int out, const VrArgs& A) {
  const DnKernelArgs<VAR> K = A;   // (the plain form: the DnArgs part)
  const dim3 grid = dn_grid(A.W, A.rows), block(256);
  if (out == DN_OUT_SIGNAL) hipLaunchKernelGGL((rt_dn_iteration_kernel<DN_OUT_SIGNAL, VAR>), grid, block, 0, s, K);
  else if (out == DN_OUT_RGB) hipLaunchKernelGGL((rt_dn_iteration_kernel<DN_OUT_RGB, VAR>), grid, block, 0, s, K);
  else hipLaunchKernelGGL((rt_dn_iteration_kernel<DN_OUT_PATH, VAR>), grid, block, 0, s, K);
}

// iterations >= 1 passes from sig[0]; `A` holds the outputs of the final pass (last_out: DN_OUT_RGB or DN_OUT_PATH).
// vp null: the plain filter, sig = (r, g, b, lum).  vp set: atrous_v, sig = (r, g, b, V).
static int dn_filter(hipStream_t s, uint32_t W, uint32_t rows, const vxrt_denoise_params_t* dn, const vxrt_variance_params_t* vp, float4* const sig[2],
                     const float4* P, const float4* N, int last_out, VrArgs A) {
  A.W = W; A.rows = rows; A.tiles_x = dn_tiles_x(W); A.npow = dn->normal_power; A.sz = dn->sigma_z; A.P = P; A.N = N;
  for (uint32_t i = 0; i < dn->iterations; ++i) {
    A.step = 1u << i;
    A.sl = vp ? dn->sigma_l : dn->sigma_l * (1.0f / (float)(1u << i));   // (atrous_v: the variance shrinks instead)
    A.eps = vp ? vp->epsilon : 0.0f;
    A.S = sig[i & 1u]; A.out4 = sig[(i + 1u) & 1u];
    const int out = i + 1u < dn->iterations ? DN_OUT_SIGNAL : last_out;
    if (vp) dn_launch_iteration<true>(s, out, A);
    else dn_launch_iteration<false>(s, out, A);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- temporal accumulation: the history and the launch ----
struct vxrt_history {
  uint64_t cap = 0;                  // pixels each buffer holds
  float4* he[2] = {nullptr, nullptr}; float4* hp[2] = {nullptr, nullptr}; float4* hn[2] = {nullptr, nullptr};
  float2* hm[2] = {nullptr, nullptr};   // HM = (m1, m2): a history with moments only (vxrt_history_create_moments)
  bool moments = false;
  uint32_t cur = 0;                  // the set the last frame wrote
  bool empty = true;
  vxrt_camera_t cam{};               // of the last frame, with its geometry
  uint32_t W = 0, H = 0, y0 = 0, y1 = 0;
};

static bool tp_params_ok(const vxrt_temporal_params_t* t) {
  return t && t->alpha_min > 0.0f && t->alpha_min <= 1.0f && t->max_len >= 1u && t->max_len <= VXRT_TEMPORAL_MAX_LEN && t->sigma_z > 0.0f &&
         std::isfinite(t->normal_min);   // (the comparisons are false for NaN)
}

bool tp_request_ok(const vxrt_history_t* h, const vxrt_temporal_params_t* t, uint64_t pixels, bool moments) {
  return h && h->moments == moments && tp_params_ok(t) && pixels <= h->cap;
}

bool vr_params_ok(const vxrt_variance_params_t* v) {
  return v && v->epsilon > 0.0f && std::isfinite(v->epsilon) && v->min_len >= 1u && v->min_len <= VXRT_TEMPORAL_MAX_LEN && v->radius >= 1u &&
         v->radius <= 3u && v->reserved == 0u;
}

// the reciprocal basis of camera c (the header's rule: doubles, no contraction, one rounding to fp32 per component)
static void tp_reciprocal_basis(const vxrt_camera_t& c, float Rr[3], float Ur[3], float Fr[3]) {
  const double R[3] = {c.right[0], c.right[1], c.right[2]}, U[3] = {c.up[0], c.up[1], c.up[2]}, F[3] = {c.forward[0], c.forward[1], c.forward[2]};
  auto cross = [](const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
  };
  double UF[3], FR[3], RU[3];
  cross(U, F, UF); cross(F, R, FR); cross(R, U, RU);
  const double det = (R[0] * UF[0] + R[1] * UF[1]) + R[2] * UF[2];
  for (int k = 0; k < 3; ++k) { Rr[k] = (float)(UF[k] / det); Ur[k] = (float)(FR[k] / det); Fr[k] = (float)(RU[k] / det); }
}

// One step on history h: the checks are the caller's (window of at most h->cap pixels, not empty).  Launches, then makes the written set,
// `cam` and the geometry the history's state.
// Q / Nq: both null (the step T) or both set (the step with motion, T_m).  A history with moments takes the MOMENTS instantiations
// (T_v over either): the kind of the history is the caller's to check against the call.
template <int OUT, bool MOTION, bool MOMENTS>
static void tp_launch_kernel(hipStream_t s, dim3 grid, const vxrt_history_t* h, uint32_t prev, uint32_t next, const TpArgs& A, const float4* Q, const float4* Nq) {
  typename TpKernelArgs<MOTION, MOMENTS>::type K{};
  static_cast<TpArgs&>(K) = A;
  if constexpr (MOTION) { K.Q = Q; K.Nq = Nq; }
  if constexpr (MOMENTS) { K.hm = h->hm[prev]; K.hm_o = h->hm[next]; }
  hipLaunchKernelGGL((rt_tp_accumulate_kernel<OUT, MOTION, MOMENTS>), grid, dim3(256), 0, s, K);
}

template <bool MOTION, bool MOMENTS>
static void tp_launch_out(hipStream_t s, dim3 grid, const vxrt_history_t* h, uint32_t prev, uint32_t next, int out, const TpArgs& A, const float4* Q, const float4* Nq) {
  if (out == TP_OUT_SIGNAL) tp_launch_kernel<TP_OUT_SIGNAL, MOTION, MOMENTS>(s, grid, h, prev, next, A, Q, Nq);
  else if (out == TP_OUT_LEN) tp_launch_kernel<TP_OUT_LEN, MOTION, MOMENTS>(s, grid, h, prev, next, A, Q, Nq);
  else tp_launch_kernel<TP_OUT_PATH, MOTION, MOMENTS>(s, grid, h, prev, next, A, Q, Nq);
}

static int tp_launch(hipStream_t s, vxrt_history_t* h, const vxrt_camera_t* cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1,
                     const vxrt_temporal_params_t* t, int out, TpArgs A, const float4* Q = nullptr, const float4* Nq = nullptr) {
  const uint32_t rows = y1 - y0;
  const bool have = !h->empty && h->W == W && h->H == H && h->y0 == y0 && h->y1 == y1;   // (another window: an implicit reset)
  const uint32_t prev = h->cur, next = have ? h->cur ^ 1u : h->cur;
  A.W = W; A.rows = rows; A.tiles_x = dn_tiles_x(W); A.have = have ? 1u : 0u; A.max_len = t->max_len;
  A.fW = (float)W; A.fH = (float)H; A.fy0 = (float)y0; A.frows = (float)rows;
  if (have) {
    for (int k = 0; k < 3; ++k) A.pos[k] = h->cam.pos[k];
    tp_reciprocal_basis(h->cam, A.Rr, A.Ur, A.Fr);
    A.vp[0] = h->cam.viewplane[0]; A.vp[1] = h->cam.viewplane[1];
  }
  A.alpha_min = t->alpha_min; A.sigma_z = t->sigma_z; A.normal_min = t->normal_min;
  A.he = h->he[prev]; A.hp = h->hp[prev]; A.hn = h->hn[prev];
  A.he_o = h->he[next]; A.hp_o = h->hp[next]; A.hn_o = h->hn[next];
  const dim3 grid = dn_grid(W, rows);
  if (h->moments) {
    if (Q) tp_launch_out<true, true>(s, grid, h, prev, next, out, A, Q, Nq);
    else tp_launch_out<false, true>(s, grid, h, prev, next, out, A, Q, Nq);
  } else if (Q) tp_launch_out<true, false>(s, grid, h, prev, next, out, A, Q, Nq);
  else tp_launch_out<false, false>(s, grid, h, prev, next, out, A, Q, Nq);
  if (hipGetLastError() != hipSuccess) return -1;
  h->cur = next; h->empty = false; h->cam = *cam; h->W = W; h->H = H; h->y0 = y0; h->y1 = y1;
  return 0;
}

static void tp_history_free(vxrt_history_t* h) {
  for (int k = 0; k < 2; ++k) { (void)hipFree(h->he[k]); (void)hipFree(h->hp[k]); (void)hipFree(h->hn[k]); (void)hipFree(h->hm[k]); }
  delete h;
}

static int tp_history_create(uint32_t width, uint32_t rows, bool moments, vxrt_history_t** history) {
  const uint64_t n = (uint64_t)width * rows;
  if (!history || n == 0 || n > 0x7fffffffull) return -1;
  vxrt_history_t* h = new vxrt_history;
  bool ok = true;
  for (int k = 0; k < 2 && ok; ++k)
    ok = hipMalloc((void**)&h->he[k], n * 16u) == hipSuccess && hipMalloc((void**)&h->hp[k], n * 16u) == hipSuccess &&
         hipMalloc((void**)&h->hn[k], n * 16u) == hipSuccess && (!moments || hipMalloc((void**)&h->hm[k], n * 8u) == hipSuccess);
  if (!ok) {
    tp_history_free(h);
    return -1;
  }
  h->cap = n;
  h->moments = moments;
  *history = h;
  return 0;
}

// V0 of the history's current set (the checks are the caller's): to out[p * out_stride] and / or to frame_out, full-frame addressing
static int vr_launch_initial(hipStream_t s, const vxrt_history_t* h, const vxrt_denoise_params_t* dn, const vxrt_variance_params_t* vp, float* out,
                             uint32_t out_stride, float* frame_out) {
  VrInitArgs A{};
  A.W = h->W; A.rows = h->y1 - h->y0; A.tiles_x = dn_tiles_x(A.W); A.npow = dn->normal_power; A.radius = vp->radius; A.y0 = h->y0;
  A.sz = dn->sigma_z; A.fmin = (float)vp->min_len;
  A.he = h->he[h->cur]; A.hm = h->hm[h->cur]; A.hp = h->hp[h->cur]; A.hn = h->hn[h->cur];
  A.out = out; A.out_stride = out_stride; A.frame_out = frame_out;
  hipLaunchKernelGGL(rt_vr_initial_kernel, dn_grid(A.W, A.rows), dim3(256), 0, s, A);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the tail of a denoised path frame (path_frame_end in rt_path.hip ends in one of the two functions below) ----
// The window and the buffers every launch of the tail shares, read from the context and the request in this one place.  Per pixel of the
// window: geo = P (w = hit?), nrm = N, lit / alb of the primary hit, acc = the accumulator over samples, sig = the two signal buffers.
struct DnFrame {
  hipStream_t s;
  uint32_t W, H, y0, y1, n;           // rows [y0, y1) of a W x H frame, n = W * (y1 - y0)
  const float4* geo; const float4* nrm; const float4* lit; const float4* alb; const float4* acc;
  uint32_t spp, flat;                 // flat: no bounces, the colour is the flat sum of Lit_0
  float4* sig[2];
  uint32_t* dst; float* colors;       // full-frame addressing
};

static DnFrame dn_frame(const FrameCtx* c, const RenderRequest& r, uint32_t n) {
  // (a frame with per-pixel sample counts has divided its accumulators by each pixel's own count: spp = 1, not flat)
  return DnFrame{(hipStream_t)r.stream, r.width, r.height, r.y0, r.y1, n, c->pt_geo, c->pt_nrm, c->pt_lit, c->pt_alb, c->pt_acc,
                 r.sample_counts ? 1u : r.path->spp, r.sample_counts ? 0u : (r.path->bounces == 0 ? 1u : 0u), {c->dn_sig[0], c->dn_sig[1]}, r.dst, r.colors};
}

// per pixel t of the window: c = the path frame's colour (acc / spp | the flat sum of Lit_0 | the background), the optional guide
// outputs, and with `sig` the demodulated signal (E, lum(E)) the filter starts from
static int dn_launch_demodulate(const DnFrame& f, float4* sig, const vxrt_path_aov_t* aov) {
  vxrt_path_aov_t o;
  memset(&o, 0, sizeof(o));
  if (aov) o = *aov;
  hipLaunchKernelGGL(rt_dn_demodulate_kernel, dim3((f.n + 255u) / 256u), dim3(256), 0, f.s, f.n, f.W, f.y0, f.geo, f.nrm, f.lit, f.alb, f.acc, f.spp, f.flat,
                     sig, o);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// what the pass that ends the frame needs (DN_OUT_PATH, TP_OUT_PATH): it remodulates with lit / alb, packs and writes dst / colors
static VrArgs dn_path_out(const DnFrame& f) {
  VrArgs A{};
  A.W = f.W; A.lit = f.lit; A.alb = f.alb; A.dst = f.dst; A.colors = f.colors; A.y0 = f.y0;
  return A;
}

// out = T(E, P, N; h, the history's camera, t) for the window, one launch: E = sig[0]'s rgb.  filtered: (out.rgb, lum) goes back into sig[0]
// (in place: a pixel reads only its own entry) for the passes; else this launch ends the frame.  The history then holds this frame, its
// camera and the geometry.  Q / Nq (both or neither): the step with motion, T_m.  A history with moments: the step is T_v.
static int tp_launch_path(const DnFrame& f, const RenderRequest& r, bool filtered, const float4* Q, const float4* Nq) {
  TpArgs A{};
  A.E4 = f.sig[0]; A.P = f.geo; A.N = f.nrm; A.sig = f.sig[0];
  A.path = dn_path_out(f);
  return tp_launch(f.s, r.history, r.cams, f.W, f.H, f.y0, f.y1, r.temporal, filtered ? TP_OUT_SIGNAL : TP_OUT_PATH, A, Q, Nq);
}

int render_denoise_aov(FrameCtx* c, const RenderRequest& r, uint32_t n) { return dn_launch_demodulate(dn_frame(c, r, n), nullptr, r.aov); }

// The one place that knows the order: demodulate -> temporal step -> initial variance -> passes.
//   demodulate   the pixels' accumulators into sig[0], and the guide outputs.
//   temporal     (r.temporal) one launch blends sig[0] with the reprojected history, in place, so the ping-pong order stays; without
//                iterations that launch remodulates, packs and writes, and is the end of the frame.
//   variance     (r.variance, which check_request admits with r.temporal only: the history holds moments, the step was T_v) one launch
//                writes V0 of the history's current set into the w of sig[0], if passes follow, and into r.variance_out, if asked for.
//   passes       dn->iterations launches, ping-pong between sig[0] and sig[1] (atrous_v after a variance launch), the last of which
//                remodulates, packs and writes.
int render_denoise_tail(FrameCtx* c, const RenderRequest& r, uint32_t n) {
  if (!grow_device({{(void**)&c->dn_sig[0], 16}, {(void**)&c->dn_sig[1], 16}}, &c->dn_cap, n, GrowSync::STREAM, (hipStream_t)r.stream)) return -1;
  const DnFrame f = dn_frame(c, r, n);
  const bool filtered = r.denoise->iterations != 0;
  if (dn_launch_demodulate(f, f.sig[0], r.aov) != 0) return -1;
  if (r.temporal) {
    if (tp_launch_path(f, r, filtered, r.motion ? c->mo_pos : nullptr, r.motion ? c->mo_nrm : nullptr) != 0) return -1;
    if (r.variance && (filtered || r.variance_out) &&
        vr_launch_initial(f.s, r.history, r.denoise, r.variance, filtered ? &f.sig[0]->w : nullptr, 4, r.variance_out) != 0) return -1;
    if (!filtered) return 0;
  }
  return dn_filter(f.s, f.W, f.y1 - f.y0, r.denoise, r.variance, f.sig, f.geo, f.nrm, DN_OUT_PATH, dn_path_out(f));
}

// ---- the stand-alone calls: what the entry points of a family share behind each one's own refusals ----
// The step alone.  The caller has checked the kind of history and which of the motion guides Q / Nq are null; a null guide passes the
// alignment test, so the test is over exactly the pointers the entry point has.
static int tp_accumulate(vxrt_history_t* h, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, const float* signal,
                         const float* position, const float* normal, const float* Q, const float* Nq, const vxrt_temporal_params_t* prm, float* out4,
                         void* stream) {
  if (!camera_ok(cam) || !tp_params_ok(prm) || !signal || !position || !normal || !out4) return -1;
  if ((((uintptr_t)position | (uintptr_t)normal | (uintptr_t)Q | (uintptr_t)Nq) & 15u) != 0) return -1;
  if (width == 0 || height == 0 || y0 > y1 || y1 > height) return -1;
  if (y0 == y1) return 0;
  const uint64_t n = (uint64_t)width * (y1 - y0);
  if (n > 0x7fffffffull || n > h->cap) return -1;
  TpArgs A{};
  A.E3 = signal; A.P = (const float4*)position; A.N = (const float4*)normal; A.out4 = out4;
  return tp_launch((hipStream_t)stream, h, cam, width, height, y0, y1, prm, TP_OUT_LEN, A, (const float4*)Q, (const float4*)Nq);
}

// The filter alone.  vp null: vxrt_denoise (variance and out_variance are null).  vp set and checked: atrous_v, the variance in and (optional) out.
static int dn_denoise(uint32_t width, uint32_t rows, const float* signal, const float* variance, const float* position, const float* normal,
                      const vxrt_denoise_params_t* dn, const vxrt_variance_params_t* vp, float* out, float* out_variance, void* scratch,
                      uint64_t scratch_bytes, void* stream) {
  const uint64_t n = (uint64_t)width * rows;
  if (!dn_params_ok(dn) || n > 0x7fffffffull) return -1;
  if (n == 0) return 0;
  if (!signal || !position || !normal || !out || out == signal || (((uintptr_t)position | (uintptr_t)normal) & 15u) != 0) return -1;
  if (vp && (!variance || out_variance == variance)) return -1;
  if (dn->iterations && (!scratch || ((uintptr_t)scratch & 15u) != 0 || scratch_bytes < vxrt_denoise_scratch_bytes(width, rows))) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (dn->iterations == 0) {
    if (hipMemcpyAsync(out, signal, n * 12u, hipMemcpyDeviceToDevice, s) != hipSuccess) return -1;
    return !out_variance || hipMemcpyAsync(out_variance, variance, n * 4u, hipMemcpyDeviceToDevice, s) == hipSuccess ? 0 : -1;
  }
  float4* const sig[2] = {(float4*)scratch, (float4*)scratch + n};
  const dim3 grid(((uint32_t)n + 255u) / 256u), block(256);
  if (vp) hipLaunchKernelGGL(rt_vr_load_kernel, grid, block, 0, s, (uint32_t)n, signal, variance, sig[0]);
  else hipLaunchKernelGGL(rt_dn_load_kernel, grid, block, 0, s, (uint32_t)n, signal, sig[0]);
  VrArgs last{};
  last.out3 = out; last.outv = out_variance;
  return dn_filter(s, width, rows, dn, vp, sig, (const float4*)position, (const float4*)normal, DN_OUT_RGB, last);
}

extern "C" {

int vxrt_history_create(uint32_t width, uint32_t rows, vxrt_history_t** history) { return tp_history_create(width, rows, false, history); }

int vxrt_history_create_moments(uint32_t width, uint32_t rows, vxrt_history_t** history) { return tp_history_create(width, rows, true, history); }

int vxrt_history_destroy(vxrt_history_t* h) {
  if (!h) return -1;
  (void)hipDeviceSynchronize();
  tp_history_free(h);
  return 0;
}

int vxrt_history_reset(vxrt_history_t* h) {
  if (!h) return -1;
  h->empty = true;
  return 0;
}

int vxrt_history_read(vxrt_history_t* h, float* out4, void* stream) {
  if (!h || !out4 || h->empty) return -1;
  const uint64_t n = (uint64_t)h->W * (h->y1 - h->y0);
  return hipMemcpyAsync(out4, h->he[h->cur], n * 16u, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? 0 : -1;
}

int vxrt_history_read_moments(vxrt_history_t* h, float* out2, void* stream) {
  if (!h || !out2 || h->empty || !h->moments) return -1;
  const uint64_t n = (uint64_t)h->W * (h->y1 - h->y0);
  return hipMemcpyAsync(out2, h->hm[h->cur], n * 8u, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? 0 : -1;
}

int vxrt_temporal_accumulate(vxrt_history_t* h, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                             const float* signal, const float* position, const float* normal, const vxrt_temporal_params_t* prm,
                             float* out4, void* stream) {
  if (!h || h->moments) return -1;   // (moments would go stale)
  return tp_accumulate(h, cam, width, height, y0, y1, signal, position, normal, nullptr, nullptr, prm, out4, stream);
}

// the step with motion alone (see the header, "Motion"): vxrt_temporal_accumulate's checks, and the two guides more
int vxrt_temporal_accumulate_motion(vxrt_history_t* h, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                    const float* signal, const float* position, const float* normal, const float* prev_position,
                                    const float* prev_normal, const vxrt_temporal_params_t* prm, float* out4, void* stream) {
  if (!h || h->moments || !prev_position || !prev_normal) return -1;
  return tp_accumulate(h, cam, width, height, y0, y1, signal, position, normal, prev_position, prev_normal, prm, out4, stream);
}

// the step with moments alone (see the header, "Variance guidance"): T_v over T (both motion guides null) or over T_m (both set)
int vxrt_temporal_accumulate_moments(vxrt_history_t* h, const vxrt_camera_t* cam, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1,
                                     const float* signal, const float* position, const float* normal, const float* prev_position,
                                     const float* prev_normal, const vxrt_temporal_params_t* prm, float* out4, void* stream) {
  if (!h || !h->moments || (prev_position == nullptr) != (prev_normal == nullptr)) return -1;
  return tp_accumulate(h, cam, width, height, y0, y1, signal, position, normal, prev_position, prev_normal, prm, out4, stream);
}

// V0 of the last frame's window (see the header, "Variance guidance"): one launch
int vxrt_history_variance(vxrt_history_t* h, const vxrt_denoise_params_t* dn, const vxrt_variance_params_t* vp, float* variance, void* stream) {
  if (!h || h->empty || !h->moments || !dn_params_ok(dn) || !vr_params_ok(vp) || !variance) return -1;
  return vr_launch_initial((hipStream_t)stream, h, dn, vp, variance, 1, nullptr);
}

uint64_t vxrt_denoise_scratch_bytes(uint32_t width, uint32_t rows) { return 32ull * width * rows; }

uint64_t vxrt_denoise_variance_scratch_bytes(uint32_t width, uint32_t rows) { return 32ull * width * rows; }

// atrous_v alone: vxrt_denoise's checks, the variance in and (optional) out
int vxrt_denoise_variance(uint32_t width, uint32_t rows, const float* signal, const float* variance, const float* position, const float* normal,
                          const vxrt_denoise_params_t* dn, const vxrt_variance_params_t* vp, float* out, float* out_variance, void* scratch,
                          uint64_t scratch_bytes, void* stream) {
  if (!vr_params_ok(vp)) return -1;
  return dn_denoise(width, rows, signal, variance, position, normal, dn, vp, out, out_variance, scratch, scratch_bytes, stream);
}

int vxrt_denoise(uint32_t width, uint32_t rows, const float* signal, const float* position, const float* normal, const vxrt_denoise_params_t* dn,
                 float* out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return dn_denoise(width, rows, signal, nullptr, position, normal, dn, nullptr, out, nullptr, scratch, scratch_bytes, stream);
}

}
