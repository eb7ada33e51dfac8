// The quantiser of the 52-byte reference node (bvh_quantized_node_t, common.h:52-67), shared by the GPU builder (bvh_builder.hip:
// collapse + emit) and the refit (rt_kernels.hip: vxrt_accel_refit), so that a refit of unchanged geometry rewrites the builder's
// bytes.  Restates bvh.cpp:215-264: origin = the node box's lo corner, per axis one exponent e with every child's planes
// origin + q * 2^e, q in 0..255, floor / ceil -- conservative after the decode's own rounding.  tests/refit_ref.py restates it in numpy.
#ifndef VXRT_BVH_QUANT_H
#define VXRT_BVH_QUANT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// smallest e with extent / 255 <= 2^e (bvh.cpp:215-264 picks ceil(log2(extent / 255))), from the float's own exponent: exact
__device__ __forceinline__ int bb_pick_exp(float extent) {
  if (!(extent > 0.0f) || extent > 3.0e38f) return 0;
  const float q = extent / 255.0f;
  if (q == 0.0f) return -126;   // a subnormal extent whose quotient underflows: the clamp (the CPU builder's log2(0) = -inf)
  int k;
  const float m = frexpf(q, &k);   // extent / 255 = m * 2^k, m in [0.5, 1)
  int e = m == 0.5f ? k - 1 : k;
  return max(-126, min(126, e));
}

// q_lo, q_hi of one axis of one child at scale s = 2^e (inv = 2^-e, both exact: |e| <= 126); false if the child does not fit 8 bits there
__device__ __forceinline__ bool bb_quant_axis(float origin, float s, float inv, float cmin, float cmax, uint32_t& qlo, uint32_t& qhi) {
  float fl = floorf((cmin - origin) * inv), fh = ceilf((cmax - origin) * inv);
  if (!(fl >= 0.0f)) fl = 0.0f;
  if (!(fh >= fl)) fh = fl;
  if (fh > 255.0f) return false;
  int lo = (int)fl, hi = (int)fh;
  if (lo > 255) return false;
  // conservative after the decode's own rounding (origin + q * 2^e rounds once; q * 2^e itself is exact)
  while (lo > 0 && origin + (float)lo * s > cmin) --lo;
  while (hi < 255 && origin + (float)hi * s < cmax) ++hi;
  if (origin + (float)hi * s < cmax) return false;
  qlo = (uint32_t)lo; qhi = (uint32_t)hi;
  return true;
}
__device__ __forceinline__ float bb_pow2(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }   // e in [-126, 127]

// One axis of one node: starting from e (bb_pick_exp of the node's extent), the exponent is bumped until every present child (bit k
// of `present`) fits 8 bits; q_lo / q_hi of child k land in ql[k] / qh[k].  false: no exponent up to 126 fits (the node cannot be
// quantised; the builder's counters[4] & 2).  Fixed-size arrays, constant indices after unrolling: they stay in registers.
__device__ __forceinline__ bool bb_quant_children(float origin, int& e, const float (&cmin)[4], const float (&cmax)[4], uint32_t present,
                                                  uint32_t (&ql)[4], uint32_t (&qh)[4]) {
  for (;;) {
    bool ok = true;
    const float sc = bb_pow2(e), inv = bb_pow2(-e);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (((present >> k) & 1u) && ok) ok = bb_quant_axis(origin, sc, inv, cmin[k], cmax[k], ql[k], qh[k]);
    if (ok) return true;
    if (e >= 126) return false;
    ++e;
  }
}

#endif
