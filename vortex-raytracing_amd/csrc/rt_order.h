// The visiting order of an internal node's children: the stable sorting network of the ordered node step, and the selection that
// replaces it in a run in which no lane holds more than one valid child (order_first_valid, RT_ORDER_PATHS).
// Compiled by hipcc into the traversal kernels (rt_kernels.hip, rt_traverse_loop.inc) and by plain g++ into the stand-alone program
// of tests/test_order_paths_cpu.py, which holds the selection to the network on every validity mask and every distance.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_ORDER_FN __host__ __device__ __forceinline__
#else
#define RT_ORDER_FN inline
#endif

// max of two values neither of which is a NaN: one v_max_f32 (fmaxf adds a canonicalising v_max_f32 x, x for a signalling NaN the
// compiler cannot rule out).  The host form restates the instruction: -0 orders below +0.
RT_ORDER_FN float vmax_nonan(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
#else
  return (a < b || (a == b && __builtin_signbit(a))) ? b : a;
#endif
}

struct Cand { float d; uint32_t desc; };
// visit order: nearer first; equal distance -> higher child index first (stable far->near sort of
// rt_traversal.cpp:76-78 read from the back).  Filtered children carry d = +inf.
// Adjacent compare-exchange with a strict '<' never reorders equal keys, so a 6-comparator bubble
// network over the children laid out [3, 2, 1, 0] gives exactly that order without carrying the index.
RT_ORDER_FN void cmpx(Cand& x, Cand& y) {
  const bool sw = y.d < x.d;
  const Cand tx = x, ty = y;
  x.d = sw ? ty.d : tx.d; x.desc = sw ? ty.desc : tx.desc;
  y.d = sw ? tx.d : ty.d; y.desc = sw ? tx.desc : ty.desc;
}
RT_ORDER_FN void order_children(Cand* c) {   // in: c[k] = child k; out: c[0] nearest ... c[3] farthest
  Cand s0 = c[3], s1 = c[2], s2 = c[1], s3 = c[0];
  cmpx(s0, s1); cmpx(s1, s2); cmpx(s2, s3); cmpx(s0, s1); cmpx(s1, s2); cmpx(s0, s1);
  c[0] = s0; c[1] = s1; c[2] = s2; c[3] = s3;
}

// ---- RT_ORDER_PATHS: what the network returns when few children are valid, without the network ----
// ok[k] = child k is to be visited (eval_children_raw); c[k].d is the raw slab distance, read only where ok[k] holds.
// (Every function reads its arrays into values first and selects among values: with the reads inside the arms of the conditionals the
// compiler merges them into one read through a selected address, and the kernels' c[] and ok[] become arrays in scratch memory.)
RT_ORDER_FN bool order_any_valid(const bool* ok) {
  const bool k0 = ok[0], k1 = ok[1], k2 = ok[2], k3 = ok[3];
  return k0 | k1 | k2 | k3;
}
// at least two / at least three valid children (conditions only: scalar mask arithmetic in the kernels; three: the wave log's classes)
RT_ORDER_FN bool order_two_valid(const bool* ok) {
  const bool k0 = ok[0], k1 = ok[1], k2 = ok[2], k3 = ok[3];
  return (k0 & k1) | ((k0 | k1) & k2) | ((k0 | k1 | k2) & k3);
}
RT_ORDER_FN bool order_three_valid(const bool* ok) {
  const bool k0 = ok[0], k1 = ok[1], k2 = ok[2], k3 = ok[3];
  return (k0 & k1 & k2) | (((k0 & k1) | ((k0 | k1) & k2)) & k3);
}
// the valid child in the lowest slot (one valid child: the child the network leaves in c[0])
RT_ORDER_FN Cand order_first_valid(const Cand* c, const bool* ok) {
  const Cand c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
  const bool k0 = ok[0], k1 = ok[1], k2 = ok[2];
  Cand r;
  r.d = k0 ? c0.d : (k1 ? c1.d : (k2 ? c2.d : c3.d));
  r.desc = k0 ? c0.desc : (k1 ? c1.desc : (k2 ? c2.desc : c3.desc));
  return r;
}
