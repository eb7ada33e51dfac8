// Acceleration layout of a scene: its build from the reference-format buffers (vxrt_accel_build) and its refit in place
// (vxrt_accel_refit / vxrt_accel_set_transforms), and the tables an accel derives from the scene on request (alpha test, motion snapshot,
// emitters).  No ray is traced here: the kernels that read the layout are in rt_kernels.hip.
// Build: as rt_kernels.hip (one hipcc call for the whole library, no relocatable device code).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include "rt_internal.h"
#include "bvh_quant.h"
#include "rt_path_code.h"

// ---------------------------------------------------------------------------------------------
// acceleration-layout build (one pass over the reference-format buffers; validates every index the
// traversal will follow so that a malformed scene is rejected on the host instead of faulting the GPU)
// ---------------------------------------------------------------------------------------------
// one thread per reference node of one buffer.  bases/ends: sorted BLAS node ranges (nb of them).
__global__ void accel_nodes_kernel(const uint32_t* __restrict__ ref, uint32_t n_nodes, uint4* __restrict__ out, int is_tlas,
                                   const uint32_t* __restrict__ bases, const uint32_t* __restrict__ ends, uint32_t nb,
                                   uint32_t n_tris, uint32_t n_blas, uint32_t bias, uint32_t* status) {
  // bias: compact index of this buffer's node 0 (0 for the TLAS pass, n_tlas for the BLAS pass); `out` is already offset by it
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const uint32_t* w = ref + (size_t)i * RT_NODE_DWORDS;
  const uint32_t imask = w[3] >> 24, leftFirst = w[4], leafData = w[5];
  uint32_t base = 0, end = n_nodes;
  if (!is_tlas) {
    bool in = false;
    for (uint32_t j = 0; j < nb; ++j) if (i >= bases[j] && i < ends[j]) { base = bases[j]; end = ends[j]; in = true; }
    if (!in) return;   // node outside every instance's range: unreachable, leave untouched
  }
  if (imask != (is_tlas ? 1u : 0u)) return;   // not a node of this kind (e.g. unused tail): reachable nodes are checked via their parent
  const bool leaf = is_tlas ? (leafData != 0xffffffffu) : (leafData != 0u);
  if (leaf) return;
  const float px = __uint_as_float(w[0]), py = __uint_as_float(w[1]), pz = __uint_as_float(w[2]);
  const float po[3] = {px, py, pz};
  const int ev[3] = {(int)(int8_t)(w[3] & 0xff), (int)(int8_t)((w[3] >> 8) & 0xff), (int)(int8_t)((w[3] >> 16) & 0xff)};
  const uint8_t* bytes = (const uint8_t*)w;
  uint32_t pay[4] = {DESC_NONE, DESC_NONE, DESC_NONE, DESC_NONE};   // complete descriptors of the children
  uint8_t qb[24];
  for (int k = 0; k < 4; ++k) {
    const uint8_t* c = bytes + 24 + 7 * k;
    for (int j = 0; j < 6; ++j) qb[4 * j + k] = c[1 + j];   // plane-major: word j = plane j (lo xyz, hi xyz) of the four children
    if (c[0] == 0) continue;   // meta (rt_traversal.cpp:60)
    // the sign-selected slab form needs lo <= hi per axis (child_box); an inverted box falls back to min/max
    if (c[1] > c[4] || c[2] > c[5] || c[3] > c[6]) atomicOr(status, STATUS_FMA_DECODE_DIFFERS);
    // fma decode must reproduce origin + ldexp(float(q), e) bit for bit (eval_children)
    for (int j = 0; j < 6; ++j) {
      const float q = (float)c[1 + j];
      const float a = po[j % 3] + ldexpf(q, ev[j % 3]);
      const float b = __fmaf_rn(q, ldexpf(1.0f, ev[j % 3]), po[j % 3]);
      if (__float_as_uint(a) != __float_as_uint(b) && !(a != a && b != b)) atomicOr(status, STATUS_FMA_DECODE_DIFFERS);
    }
    const uint64_t ci64 = (uint64_t)base + leftFirst + (uint32_t)k;   // calcNodePtr(base_ptr, leftFirst + childIdx), :91-92
    // children are allocated after their parent by the builders (bvh.cpp:94-97, 371-402): requiring
    // that makes every accepted tree acyclic, so traversal terminates
    if (ci64 >= end || ci64 <= i || ci64 + bias > PAYLOAD_MASK) { atomicOr(status, STATUS_BAD_SCENE); continue; }
    const uint32_t ci = (uint32_t)ci64;
    const uint32_t* cw = ref + (size_t)ci * RT_NODE_DWORDS;
    const uint32_t c_imask = cw[3] >> 24, c_lf = cw[4], c_ld = cw[5];
    if (c_imask != (is_tlas ? 1u : 0u)) { atomicOr(status, STATUS_BAD_SCENE); continue; }
    if (is_tlas) {
      if (c_ld != 0xffffffffu) {
        if (c_ld >= n_blas || c_ld >= 0x3FFFFFF0u) { atomicOr(status, STATUS_BAD_SCENE); continue; }
        pay[k] = DESC(DK_INST, c_ld);
      } else pay[k] = DESC(DK_TLAS, ci + bias);
    } else {
      if (c_ld != 0u) {
        if ((uint64_t)c_lf + c_ld > n_tris) { atomicOr(status, STATUS_BAD_SCENE); continue; }
        pay[k] = DESC(DK_LEAF, (c_ld <= LEAF_MAX_INLINE && c_lf <= LEAF_FIRST_MASK) ? ((c_ld << LEAF_FIRST_BITS) | c_lf) : ci);   // else by reference
        if (!(c_ld <= LEAF_MAX_INLINE && c_lf <= LEAF_FIRST_MASK) && ci > LEAF_FIRST_MASK) { atomicOr(status, STATUS_BAD_SCENE); pay[k] = DESC_NONE; }
      } else pay[k] = DESC(DK_BLAS, ci + bias);
    }
  }
  uint32_t qw[6];
  for (int v = 0; v < 6; ++v) qw[v] = (uint32_t)qb[4 * v] | ((uint32_t)qb[4 * v + 1] << 8) | ((uint32_t)qb[4 * v + 2] << 16) | ((uint32_t)qb[4 * v + 3] << 24);
  uint4* o = out + (size_t)i * CNODE_VEC4;
  o[0] = make_uint4(w[0], w[1], w[2], __float_as_uint(ldexpf(1.0f, ev[0])));
  o[1] = make_uint4(qw[0], qw[1], qw[2], qw[3]);
  o[2] = make_uint4(qw[4], qw[5], pay[0], pay[1]);
  o[3] = make_uint4(pay[2], pay[3], __float_as_uint(ldexpf(1.0f, ev[1])), __float_as_uint(ldexpf(1.0f, ev[2])));
}

__global__ void accel_tris_kernel(const float* __restrict__ tri, uint32_t n, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* t = tri + (size_t)i * 9;
  const float v0x = t[0], v0y = t[1], v0z = t[2];
  // edge1 = v1 - v0, edge2 = v2 - v0 exactly as rt_traversal.cpp:272-278 computes them per test
  out[(size_t)i * 3 + 0] = make_float4(v0x, v0y, v0z, t[3] - v0x);
  out[(size_t)i * 3 + 1] = make_float4(t[4] - v0y, t[5] - v0z, t[6] - v0x, t[7] - v0y);
  out[(size_t)i * 3 + 2] = make_float4(t[8] - v0z, 0.f, 0.f, 0.f);
}

// root descriptors: thread 0 -> TLAS root, thread 1+j -> BLAS root of instance record j
__global__ void accel_roots_kernel(const uint32_t* __restrict__ tlas, const uint32_t* __restrict__ bvh, const uint32_t* __restrict__ blas,
                                   uint32_t n_tlas, uint32_t n_bvh, uint32_t n_blas, uint32_t n_tris, uint32_t* tlas_root, uint32_t* blas_root,
                                   uint32_t* status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {
    const uint32_t imask = tlas[3] >> 24, ld = tlas[5];
    *tlas_root = DESC_DONE;
    if (imask != 1u) atomicOr(status, STATUS_BAD_SCENE);
    else if (ld != 0xffffffffu) {
      if (ld >= n_blas || ld >= 0x3FFFFFF0u) atomicOr(status, STATUS_BAD_SCENE);
      else *tlas_root = DESC(DK_INST, ld);
    } else *tlas_root = DESC(DK_TLAS, 0u);   // compact index 0
  } else if (t - 1 < n_blas) {
    const uint32_t j = t - 1;
    const uint32_t off = blas[(size_t)j * (RT_BLAS_STRIDE / 4)];
    blas_root[j] = DESC_DONE;
    if (off >= n_bvh || off > LEAF_FIRST_MASK) { atomicOr(status, STATUS_BAD_SCENE); return; }
    const uint32_t* w = bvh + (size_t)off * RT_NODE_DWORDS;
    const uint32_t imask = w[3] >> 24, lf = w[4], ld = w[5];
    if (imask != 0u) atomicOr(status, STATUS_BAD_SCENE);
    else if (ld != 0u) {
      if ((uint64_t)lf + ld > n_tris) atomicOr(status, STATUS_BAD_SCENE);
      else blas_root[j] = DESC(DK_LEAF, (ld <= LEAF_MAX_INLINE && lf <= LEAF_FIRST_MASK) ? ((ld << LEAF_FIRST_BITS) | lf) : off);
    } else if ((uint64_t)off + n_tlas > PAYLOAD_MASK) atomicOr(status, STATUS_BAD_SCENE);
    else blas_root[j] = DESC(DK_BLAS, off + n_tlas);
  }
}

// Depth of the scene in INTERNAL levels on a root-to-leaf path, TLAS and BLAS together: what bounds a lane's stack (a node step leaves at most
// three pending siblings; instance and leaf steps leave none).  One pass per level over the compact nodes (children lie after their parents, so
// the trees are acyclic): pass t gives every internal child of a node of level t - 1 the level t; a TLAS leaf hands its level on to the root of
// its instance's BLAS.  `deepest` ends as the last level any node reached.  Only reached nodes are read (unreached slots are not initialised).
__global__ void accel_depth_kernel(const uint4* __restrict__ nodes_c, uint32_t n_nodes, uint32_t tlas_root, const uint32_t* __restrict__ blas_root,
                                   uint32_t level, uint32_t* __restrict__ depth, uint32_t* __restrict__ deepest) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  auto reach = [&](uint32_t d) {
    if (is_inst_desc(d)) d = blas_root[d & PAYLOAD_MASK];
    if (!is_node_desc(d)) return;
    const uint32_t c = d & PAYLOAD_MASK;
    if (c < n_nodes) { atomicMax(&depth[c], level); *deepest = level; }   // (every writer of a pass stores the same value)
  };
  if (level == 1u) {
    if (i == 0) reach(tlas_root);
    return;
  }
  if (i >= n_nodes || depth[i] != level - 1u) return;
  const uint4* np = nodes_c + (size_t)i * CNODE_VEC4;
  const uint4 q2 = np[2], q3 = np[3];
  reach(q2.z); reach(q2.w); reach(q3.x); reach(q3.y);
}

// Path table (vxrt_accel::tri_path; the layout and the pass are rt_path_code.h's): one launch per level, top down, one thread per compact
// node; the host marks the BLAS root (level 1, code 0) first.
__global__ void accel_path_kernel(const uint4* __restrict__ nodes_c, uint32_t n_nodes, uint32_t level, uint32_t* lvl, uint32_t* ncode,
                                  const uint32_t* __restrict__ ref_bvh, uint32_t n_bvh, uint32_t n_tris, uint32_t* __restrict__ tri_path) {
  path_pass_node((const uint32_t*)nodes_c, n_nodes, blockIdx.x * blockDim.x + threadIdx.x, level, lvl, ncode, ref_bvh, n_bvh, n_tris, tri_path);
}

// Top of the tree for LDS staging: breadth-first from the TLAS root through the instance roots, the first `cap` internal
// nodes get slots 0..n-1 (so the levels every ray walks come first).  The image holds their compact nodes as four planes of
// `cap` uint4 with the child descriptors of staged children rewritten to DESC_TOP_FLAG | slot; the *_top roots likewise.
// The global compact nodes stay untouched: kernels that do not stage (EXACT, ldexp decode) start from the plain roots and
// never meet a slot descriptor.  One wavefront; a few hundred nodes, once per scene.
__global__ __launch_bounds__(64) void accel_top_kernel(const uint4* __restrict__ nodes_c, uint32_t tlas_root, const uint32_t* __restrict__ blas_root,
                                                       uint32_t n_blas, uint32_t cap, uint4* __restrict__ img, uint32_t* __restrict__ out_n,
                                                       uint32_t* __restrict__ tlas_root_top, uint32_t* __restrict__ blas_root_top) {
  __shared__ uint32_t q[RT_TOP_MAX];
  __shared__ uint32_t n_s;
  const uint32_t lane = threadIdx.x;
  auto find = [&](uint32_t idx, uint32_t n) -> uint32_t {   // wave-wide search; returns slot or 0xFFFFFFFF
    uint32_t hit = 0xFFFFFFFFu;
    for (uint32_t b = 0; b < n; b += 64u) {
      const unsigned long long m = __ballot(b + lane < n && q[b + lane] == idx);
      if (m) { hit = b + (uint32_t)__ffsll((long long)m) - 1u; break; }
    }
    return hit;
  };
  uint32_t n = 0;
  auto push = [&](uint32_t d) {   // wave-uniform d
    if (!is_node_desc(d)) return;
    const uint32_t idx = d & PAYLOAD_MASK;
    if (n >= cap || find(idx, n) != 0xFFFFFFFFu) return;
    if (lane == 0) q[n] = idx;
    ++n;
    __syncthreads();
  };
  if (is_inst_desc(tlas_root)) push(blas_root[tlas_root & PAYLOAD_MASK]); else push(tlas_root);
  for (uint32_t head = 0; head < n && n < cap; ++head) {
    const uint4* np = nodes_c + (size_t)q[head] * CNODE_VEC4;
    const uint4 q2 = np[2], q3 = np[3];
    const uint32_t d[4] = {q2.z, q2.w, q3.x, q3.y};
    for (int k = 0; k < 4; ++k) {
      if (is_inst_desc(d[k])) push(blas_root[d[k] & PAYLOAD_MASK]); else push(d[k]);
    }
  }
  __syncthreads();
  auto patch = [&](uint32_t d) -> uint32_t {
    if (!is_node_desc(d)) return d;
    const uint32_t slot = find(d & PAYLOAD_MASK, n);
    return slot == 0xFFFFFFFFu ? d : ((d & 0xC0000000u) | DESC_TOP_FLAG | slot);
  };
  for (uint32_t sidx = 0; sidx < n; ++sidx) {
    const uint4* np = nodes_c + (size_t)q[sidx] * CNODE_VEC4;
    uint4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
    q2.z = patch(q2.z); q2.w = patch(q2.w); q3.x = patch(q3.x); q3.y = patch(q3.y);
    if (lane == 0) { img[sidx] = q0; img[cap + sidx] = q1; img[2 * (size_t)cap + sidx] = q2; img[3 * (size_t)cap + sidx] = q3; }
  }
  for (uint32_t j = 0; j < n_blas; ++j) {
    const uint32_t v = patch(blas_root[j]);
    if (lane == 0) blas_root_top[j] = v;
  }
  const uint32_t tr = patch(tlas_root);
  if (lane == 0) { *tlas_root_top = tr; *out_n = n; }
  (void)n_s;
}

// shading inputs (closest.cpp:52-77 dereferences them unchecked; here a scene that would read outside its buffers is rejected
// when the acceleration layout is built): every triangle's texId names a material, and every textured material's texels lie
// inside the texture buffer with non-zero dimensions (texSample takes `% width`, rtx_shading.h:9-10)
__global__ void accel_check_shading_kernel(const rt_triex_t* __restrict__ triEx, uint32_t n_tris, const rt_material_t* __restrict__ mat, uint32_t n_mats,
                                           uint64_t tex_bytes, int have_tex, uint32_t* status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_tris && triEx[i].texId >= n_mats) atomicOr(status, STATUS_BAD_SCENE);
  if (i < n_mats && mat[i].diffuse_tex_id >= 0) {
    const uint64_t w = mat[i].tex_width, h = mat[i].tex_height, off = mat[i].tex_offset;
    if (!have_tex || w == 0 || h == 0 || (off & 3u) != 0 || off > tex_bytes || w * h > (tex_bytes - off) / 4u) atomicOr(status, STATUS_BAD_SCENE);
  }
}

// ---------------------------------------------------------------------------------------------
// refit (vxrt_accel_refit / vxrt_accel_set_transforms): new boxes for a fixed topology, written into the reference nodes in place
// and re-laid out as the build lays them out.  A plan built once per accel lists every tree's leaves and its internal nodes by level
// (the TLAS and each distinct BLAS range); one launch per level from the deepest to the roots, so that the kernel boundary makes the
// children's float boxes visible to their parent ("Refit").
// ---------------------------------------------------------------------------------------------
#define REFIT_ERR_NONFINITE 1u   // a vertex, a transform or a transformed box is not finite
#define REFIT_ERR_QUANT 2u       // a box cannot be quantised (the builder's counters[4] & 2)
#define REFIT_ERR_SINGULAR 4u    // set_transforms: a transform with det == 0 (or a non-finite inverse)
// result block of one refit, device u32: [0] status of the TLAS re-layout, [1] REFIT_ERR_* of the refit, [2] identity root instance,
// [3] staged top-of-tree nodes, [4] staged TLAS root, [5] status of the BLAS re-layout, [6] REFIT_ERR_* of set_transforms' matrices
#define REFIT_RES_WORDS 8

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// origin and exponents of a node whose float box is lo / hi (every node, leaves included: bb_emit_leaf writes them too); imask kept
__device__ __forceinline__ void refit_write_origin(uint32_t* __restrict__ w, const float lo[3], const float hi[3], const int e[3]) {
  w[0] = __float_as_uint(lo[0]); w[1] = __float_as_uint(lo[1]); w[2] = __float_as_uint(lo[2]);
  w[3] = (uint32_t)(uint8_t)(int8_t)e[0] | ((uint32_t)(uint8_t)(int8_t)e[1] << 8) | ((uint32_t)(uint8_t)(int8_t)e[2] << 16) | (w[3] & 0xff000000u);
}
__device__ __forceinline__ void refit_store_box(float* __restrict__ fbox, uint32_t i, const float lo[3], const float hi[3]) {
  float* f = fbox + (size_t)i * 6;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = hi[0]; f[4] = hi[1]; f[5] = hi[2];
}

// min / max over the vertices of triangles [first, first + count)
__device__ __forceinline__ bool refit_tri_box(const float* __restrict__ tri, uint32_t first, uint32_t count, float lo[3], float hi[3]) {
  bool fin = true;
  lo[0] = lo[1] = lo[2] = __builtin_inff(); hi[0] = hi[1] = hi[2] = -__builtin_inff();
  for (uint32_t t = first; t < first + count; ++t) {
    const float* v = tri + (size_t)t * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const float x = v[j];
      fin = fin && isfinite(x);
      lo[j % 3] = fminf(lo[j % 3], x); hi[j % 3] = fmaxf(hi[j % 3], x);
    }
  }
  return fin;
}

// one thread per BLAS leaf of the plan: the box of its triangles
__global__ __launch_bounds__(256) void refit_blas_leaf_kernel(uint32_t* __restrict__ bvh, const float* __restrict__ tri, const uint32_t* __restrict__ leaves,
                                                              uint32_t n, float* __restrict__ fbox, uint32_t* __restrict__ res) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = leaves[j];
  uint32_t* w = bvh + (size_t)i * RT_NODE_DWORDS;
  float lo[3], hi[3];
  if (!refit_tri_box(tri, w[4], w[5], lo, hi)) atomicOr(res + 1, REFIT_ERR_NONFINITE);
  const int e[3] = {bb_pick_exp(hi[0] - lo[0]), bb_pick_exp(hi[1] - lo[1]), bb_pick_exp(hi[2] - lo[2])};
  refit_write_origin(w, lo, hi, e);
  refit_store_box(fbox, i, lo, hi);
}

// TransformPosition (geometry.h:1280-1289): ((c0 x + c1 y) + c2 z) + c3 * 1, fp32, no contraction
__device__ __forceinline__ float refit_row(const float* __restrict__ m, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
}

// one thread per TLAS leaf of the plan: the world box of its instance, the 8 corners of the object box through `transform` (bvh.cpp:
// 290-304).  Object box: the refit's own box of the BLAS root after a GEOMETRY pass (fbox_bvh), else the union of the root's decoded
// child boxes, or the triangle box when the root is a leaf.
__global__ __launch_bounds__(256) void refit_instance_kernel(uint32_t* __restrict__ tlas, const uint32_t* __restrict__ leaves, uint32_t n,
                                                             const uint32_t* __restrict__ blas, const uint32_t* __restrict__ bvh, const float* __restrict__ tri,
                                                             const float* __restrict__ fbox_bvh, float* __restrict__ fbox, uint32_t* __restrict__ res) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = leaves[j];
  uint32_t* w = tlas + (size_t)i * RT_NODE_DWORDS;
  const uint32_t* rec = blas + (size_t)w[5] * (RT_BLAS_STRIDE / 4);
  const uint32_t off = rec[0];
  const uint32_t* r = bvh + (size_t)off * RT_NODE_DWORDS;
  float olo[3], ohi[3];
  bool fin = true;
  if (fbox_bvh) {
    for (int a = 0; a < 3; ++a) { olo[a] = fbox_bvh[(size_t)off * 6 + a]; ohi[a] = fbox_bvh[(size_t)off * 6 + 3 + a]; }
  } else if (r[5] != 0u) {
    fin = refit_tri_box(tri, r[4], r[5], olo, ohi);
  } else {
    const uint8_t* b = (const uint8_t*)r;
    olo[0] = olo[1] = olo[2] = __builtin_inff(); ohi[0] = ohi[1] = ohi[2] = -__builtin_inff();
    for (int k = 0; k < 4; ++k) {
      const uint8_t* c = b + 24 + 7 * k;
      if (c[0] == 0) continue;
      for (int a = 0; a < 3; ++a) {
        const int e = (int)(int8_t)b[12 + a];
        const float o = __uint_as_float(r[a]);
        olo[a] = fminf(olo[a], o + ldexpf((float)c[1 + a], e));
        ohi[a] = fmaxf(ohi[a], o + ldexpf((float)c[4 + a], e));
      }
    }
  }
  const float* m = (const float*)(rec + 17);   // blas_node_t::transform @68
  for (int k = 0; k < 12; ++k) fin = fin && isfinite(m[k]);
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int c = 0; c < 8; ++c) {
    const float x = (c & 1) ? ohi[0] : olo[0], y = (c & 2) ? ohi[1] : olo[1], z = (c & 4) ? ohi[2] : olo[2];
    for (int a = 0; a < 3; ++a) {
      const float p = refit_row(m + 4 * a, x, y, z);
      fin = fin && isfinite(p);
      lo[a] = fminf(lo[a], p); hi[a] = fmaxf(hi[a], p);
    }
  }
  if (!fin) atomicOr(res + 1, REFIT_ERR_NONFINITE);
  const int e[3] = {bb_pick_exp(hi[0] - lo[0]), bb_pick_exp(hi[1] - lo[1]), bb_pick_exp(hi[2] - lo[2])};
  refit_write_origin(w, lo, hi, e);
  refit_store_box(fbox, i, lo, hi);
}

// one thread per internal node of one level (item = node, index of its child 0): the union of its children's float boxes, then
// origin, exponents and the children's bytes with the builder's quantiser.  Meta bytes, leftFirst, leafData, imask stay.
__global__ __launch_bounds__(256) void refit_level_kernel(uint32_t* __restrict__ nodes, const uint2* __restrict__ items, uint32_t n,
                                                          float* __restrict__ fbox, uint32_t* __restrict__ res) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint2 it = items[j];
  uint32_t* w = nodes + (size_t)it.x * RT_NODE_DWORDS;
  uint32_t cw[7];
#pragma unroll
  for (int v = 0; v < 7; ++v) cw[v] = w[6 + v];
  uint8_t* cb = (uint8_t*)cw;   // children: 4 x { meta, lo x y z, hi x y z }
  uint32_t present = 0;
  float cmin[3][4], cmax[3][4];
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool on = cb[7 * k] != 0;
    present |= on ? (1u << k) : 0u;
    const float* f = fbox + (size_t)(it.y + (on ? (uint32_t)k : 0u)) * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      cmin[a][k] = on ? f[a] : 0.0f; cmax[a][k] = on ? f[3 + a] : 0.0f;
      if (on) { lo[a] = fminf(lo[a], cmin[a][k]); hi[a] = fmaxf(hi[a], cmax[a][k]); }
    }
  }
  if (!present) return;
  int e[3] = {bb_pick_exp(hi[0] - lo[0]), bb_pick_exp(hi[1] - lo[1]), bb_pick_exp(hi[2] - lo[2])};
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    uint32_t ql[4] = {0, 0, 0, 0}, qh[4] = {0, 0, 0, 0};
    ok = bb_quant_children(lo[a], e[a], cmin[a], cmax[a], present, ql, qh) && ok;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((present >> k) & 1u) { cb[7 * k + 1 + a] = (uint8_t)ql[k]; cb[7 * k + 4 + a] = (uint8_t)qh[k]; }
  }
  if (!ok) atomicOr(res + 1, REFIT_ERR_QUANT);
  refit_write_origin(w, lo, hi, e);
#pragma unroll
  for (int v = 0; v < 7; ++v) w[6 + v] = cw[v];
  refit_store_box(fbox, it.x, lo, hi);
}

// the flags the host reads after a refit: is the TLAS root a single instance with the identity as inverse (the build's rule), and the
// header of a re-staged top-of-tree image
__global__ void refit_finish_kernel(const uint32_t* __restrict__ blas, uint32_t troot, const uint32_t* __restrict__ top_roots, uint32_t* __restrict__ res) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t id = 0u;
  if (is_inst_desc(troot)) {
    const float* m = (const float*)(blas + (size_t)(troot & PAYLOAD_MASK) * (RT_BLAS_STRIDE / 4) + 1);
    id = 1u;
    for (int i = 0; i < 12; ++i) id = (id && m[i] == ((i % 5 == 0) ? 1.0f : 0.0f)) ? 1u : 0u;
  }
  res[2] = id;
  if (top_roots) { res[3] = top_roots[0]; res[4] = top_roots[1]; }
}

// set_transforms, step 1: one thread per matrix -- transform and mat4_t::inverted() (geometry.h:1149-1192, MESA: operation order kept,
// no contraction) into scratch (32 floats per record: inverse, transform); a non-finite input or inverse, or det == 0, flags res[6]
__global__ __launch_bounds__(256) void refit_xform_kernel(const float* __restrict__ in, uint32_t n, float* __restrict__ out, uint32_t* __restrict__ res) {
#pragma clang fp contract(off)
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  float c[16];
  bool fin = true;
  for (int k = 0; k < 16; ++k) { c[k] = in[(size_t)r * 16 + k]; fin = fin && isfinite(c[k]); }
  const float inv[16] = {
      c[5] * c[10] * c[15] - c[5] * c[11] * c[14] - c[9] * c[6] * c[15] + c[9] * c[7] * c[14] + c[13] * c[6] * c[11] - c[13] * c[7] * c[10],
      -c[1] * c[10] * c[15] + c[1] * c[11] * c[14] + c[9] * c[2] * c[15] - c[9] * c[3] * c[14] - c[13] * c[2] * c[11] + c[13] * c[3] * c[10],
      c[1] * c[6] * c[15] - c[1] * c[7] * c[14] - c[5] * c[2] * c[15] + c[5] * c[3] * c[14] + c[13] * c[2] * c[7] - c[13] * c[3] * c[6],
      -c[1] * c[6] * c[11] + c[1] * c[7] * c[10] + c[5] * c[2] * c[11] - c[5] * c[3] * c[10] - c[9] * c[2] * c[7] + c[9] * c[3] * c[6],
      -c[4] * c[10] * c[15] + c[4] * c[11] * c[14] + c[8] * c[6] * c[15] - c[8] * c[7] * c[14] - c[12] * c[6] * c[11] + c[12] * c[7] * c[10],
      c[0] * c[10] * c[15] - c[0] * c[11] * c[14] - c[8] * c[2] * c[15] + c[8] * c[3] * c[14] + c[12] * c[2] * c[11] - c[12] * c[3] * c[10],
      -c[0] * c[6] * c[15] + c[0] * c[7] * c[14] + c[4] * c[2] * c[15] - c[4] * c[3] * c[14] - c[12] * c[2] * c[7] + c[12] * c[3] * c[6],
      c[0] * c[6] * c[11] - c[0] * c[7] * c[10] - c[4] * c[2] * c[11] + c[4] * c[3] * c[10] + c[8] * c[2] * c[7] - c[8] * c[3] * c[6],
      c[4] * c[9] * c[15] - c[4] * c[11] * c[13] - c[8] * c[5] * c[15] + c[8] * c[7] * c[13] + c[12] * c[5] * c[11] - c[12] * c[7] * c[9],
      -c[0] * c[9] * c[15] + c[0] * c[11] * c[13] + c[8] * c[1] * c[15] - c[8] * c[3] * c[13] - c[12] * c[1] * c[11] + c[12] * c[3] * c[9],
      c[0] * c[5] * c[15] - c[0] * c[7] * c[13] - c[4] * c[1] * c[15] + c[4] * c[3] * c[13] + c[12] * c[1] * c[7] - c[12] * c[3] * c[5],
      -c[0] * c[5] * c[11] + c[0] * c[7] * c[9] + c[4] * c[1] * c[11] - c[4] * c[3] * c[9] - c[8] * c[1] * c[7] + c[8] * c[3] * c[5],
      -c[4] * c[9] * c[14] + c[4] * c[10] * c[13] + c[8] * c[5] * c[14] - c[8] * c[6] * c[13] - c[12] * c[5] * c[10] + c[12] * c[6] * c[9],
      c[0] * c[9] * c[14] - c[0] * c[10] * c[13] - c[8] * c[1] * c[14] + c[8] * c[2] * c[13] + c[12] * c[1] * c[10] - c[12] * c[2] * c[9],
      -c[0] * c[5] * c[14] + c[0] * c[6] * c[13] + c[4] * c[1] * c[14] - c[4] * c[2] * c[13] - c[12] * c[1] * c[6] + c[12] * c[2] * c[5],
      c[0] * c[5] * c[10] - c[0] * c[6] * c[9] - c[4] * c[1] * c[10] + c[4] * c[2] * c[9] + c[8] * c[1] * c[6] - c[8] * c[2] * c[5]};
  const float det = c[0] * inv[0] + c[1] * inv[4] + c[2] * inv[8] + c[3] * inv[12];
  uint32_t err = fin ? 0u : REFIT_ERR_NONFINITE;
  if (det == 0.0f) err |= REFIT_ERR_SINGULAR;
  const float invdet = 1.0f / det;
  float* o = out + (size_t)r * 32;
  for (int k = 0; k < 16; ++k) {
    const float v = inv[k] * invdet;
    if (!isfinite(v)) err |= REFIT_ERR_SINGULAR;
    o[k] = v;
    o[16 + k] = c[k];
  }
  if (err) atomicOr(res + 6, err);
}

// set_transforms, step 2: the records take the new matrices only if every one of them passed step 1
__global__ __launch_bounds__(256) void refit_xform_commit_kernel(const float* __restrict__ xf, uint32_t first, uint32_t n, uint32_t* __restrict__ blas,
                                                                 const uint32_t* __restrict__ res) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 32u || res[6] != 0u) return;
  const uint32_t r = t / 32u, k = t % 32u;
  blas[(size_t)(first + r) * (RT_BLAS_STRIDE / 4) + 1 + k] = __float_as_uint(xf[(size_t)r * 32 + k]);   // invTransform @4, transform @68
}

// The refit plan (vxrt_accel_refit): every tree's leaves and its internal nodes by level, taken once from the topology, which a refit
// never changes.  Items of level L lie in [lv[L], lv[L + 1]) of the items array: (node, index of its child 0).
struct RefitPlan {
  uint32_t* blas_leaves = nullptr; uint32_t n_blas_leaves = 0;
  uint2* blas_items = nullptr; std::vector<uint32_t> blas_lv;
  uint32_t* tlas_leaves = nullptr; uint32_t n_tlas_leaves = 0;
  uint2* tlas_items = nullptr; std::vector<uint32_t> tlas_lv;
  float* fbox_bvh = nullptr; float* fbox_tlas = nullptr;   // one float box per node (scratch)
  uint32_t* ranges = nullptr; uint32_t nb = 0;             // sorted BLAS node ranges for accel_nodes_kernel: bases, then ends
  uint32_t* res = nullptr;                                 // REFIT_RES_WORDS
  float* xf = nullptr; uint32_t xf_cap = 0;                // set_transforms: 32 floats per record
};
static void refit_plan_free(RefitPlan* p) {
  if (!p) return;
  (void)hipFree(p->blas_leaves); (void)hipFree(p->blas_items); (void)hipFree(p->tlas_leaves); (void)hipFree(p->tlas_items);
  (void)hipFree(p->fbox_bvh); (void)hipFree(p->fbox_tlas); (void)hipFree(p->ranges); (void)hipFree(p->res); (void)hipFree(p->xf);
  delete p;
}

static void accel_free(vxrt_accel* a) {
  if (!a) return;
  (void)hipDeviceSynchronize();
  (void)hipFree(a->nodes_c); (void)hipFree(a->tri_w); (void)hipFree(a->blas_root);
  (void)hipFree(a->top_img); (void)hipFree(a->top_roots); (void)hipFree(a->tri_path);
  refit_plan_free(a->refit);
  (void)hipFree(a->uvtab); (void)hipFree(a->apriori);
  (void)hipFree(a->alpha_mat); (void)hipFree(a->alpha_tri);
  (void)hipFree(a->motion_blas); (void)hipFree(a->motion_tri);
  (void)hipFree(a->em_tri); (void)hipFree(a->em_q); (void)hipFree(a->em_cum); (void)hipFree(a->em_idx);
  for (uint32_t k = 0; k <= VXRT_MAX_BATCH; ++k) (void)hipFree(a->batch_order[k]);
  for (FrameCtx& c : a->ctx) {
    (void)hipFree(c.hitbuf); (void)hipFree(c.hints); (void)hipFree(c.defer); (void)hipFree(c.ctl); (void)hipFree(c.bcount);
    for (FrameCtx::Lpt& l : c.lpt) { (void)hipFree(l.cost); (void)hipFree(l.order); }
    (void)hipFree(c.ao_geo); (void)hipFree(c.ao_nrm); (void)hipFree(c.ao_col); (void)hipFree(c.ao_cnt); (void)hipFree(c.ao_rays); (void)hipFree(c.ao_tmax); (void)hipFree(c.ao_hits); (void)hipFree(c.ao_list); (void)hipFree(c.ao_hdr);
    (void)hipFree(c.bin_hist); (void)hipFree(c.bin_keys); (void)hipFree(c.bin_order);
    for (void* q : {(void*)c.pt_geo, (void*)c.pt_nrm, (void*)c.pt_dir, (void*)c.pt_lit, (void*)c.pt_alb, (void*)c.pt_acc, (void*)c.pt_list, (void*)c.pt_hdr,
                    (void*)c.pt_I, (void*)c.pt_N, (void*)c.pt_D, (void*)c.pt_L, (void*)c.pt_T, (void*)c.pt_live[0], (void*)c.pt_live[1], (void*)c.pt_rays,
                    (void*)c.pt_hits, (void*)c.pt_srays, (void*)c.pt_stmax, (void*)c.pt_shits, (void*)c.dn_sig[0], (void*)c.dn_sig[1], (void*)c.mo_pos, (void*)c.mo_nrm,
                    (void*)c.pt_cnt, (void*)c.pt_off, (void*)c.pt_bsum, (void*)c.pt_boff, (void*)c.pt_ctot, (void*)c.pt_spix, (void*)c.pt_ssmp,
                    (void*)c.pt_erays, (void*)c.pt_etmax, (void*)c.pt_ehits, (void*)c.pt_eG, (void*)c.pt_A}) (void)hipFree(q);
    for (FrameCtx::Level& l : c.lv) {
      (void)hipFree(l.rays); (void)hipFree(l.hits); (void)hipFree(l.parent); (void)hipFree(l.term); (void)hipFree(l.col);
      (void)hipFree(l.srays); (void)hipFree(l.stmax); (void)hipFree(l.shits);
    }
    (void)hipFree(c.pbatch); (void)hipFree(c.pool_spill); (void)hipFree(c.cam);
    if (c.side) (void)hipStreamDestroy(c.side);
    if (c.ev_in) (void)hipEventDestroy(c.ev_in);
    if (c.ev_side) (void)hipEventDestroy(c.ev_side);
    if (c.ev_done) (void)hipEventDestroy(c.ev_done);
  }
  delete a;
}

// ---------------------------------------------------------------------------------------------
// emitter table (vxrt_accel_set_emitters; the definition is the header's "Emissive geometry").  Four launches, one wavefront per
// workgroup, no LDS and no workgroup that waits for another: per entry the world-space triangle, its weight and the table's maximum;
// then the quantised weights and their sums per block of EM_BLOCK entries; one wavefront that scans the block sums in passes of EM_PASS
// with a running carry (rt_path_scan_kernel's pattern); the inclusive sums.  Integer sums: the same bits in any order.
// ---------------------------------------------------------------------------------------------
#define EM_BLOCK 64u   // entries per block of the scan: one wavefront
#define EM_PASS 64u    // block sums per pass of accel_emitter_scan_kernel: its one wavefront
#define EM_ERR_INDEX 1u      // blasIdx >= n_blas, triIdx >= n_tris
#define EM_ERR_DARK 2u       // the pair's material has no positive emissive component
#define EM_ERR_NONFINITE 4u  // a vertex or a transform is not finite
#define EM_ERR_AREA 8u       // the area or the weight is zero or not finite
// res: [0] EM_ERR_*, [1] the bits of wmax (weights are positive floats: their bits order as they do)

// tri[12 e ..] = V0, E1, E2, Le; w[e] = area * max(Le); an entry that is refused writes zeros (nothing of the table is used then)
__global__ __launch_bounds__(64) void accel_emitter_tris_kernel(const vxrt_emitter_t* __restrict__ pairs, uint32_t n, const uint32_t* __restrict__ blas,
    uint32_t n_blas, const float* __restrict__ tri, uint32_t n_tris, const rt_triex_t* __restrict__ triEx, const rt_material_t* __restrict__ mat, uint32_t n_mats,
    float* __restrict__ out, float* __restrict__ w, uint32_t* __restrict__ res) {
  const uint32_t e = blockIdx.x * EM_BLOCK + threadIdx.x;
  uint32_t err = 0u;
  float we = 0.0f;
  if (e < n) {
    const vxrt_emitter_t p = pairs[e];
    float o12[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) o12[k] = 0.0f;
    if (p.blasIdx >= n_blas || p.triIdx >= n_tris || triEx[p.triIdx].texId >= n_mats) err = EM_ERR_INDEX;
    else {
      const rt_material_t* mt = mat + triEx[p.triIdx].texId;
      const float lr = mt->emissive[0], lg = mt->emissive[1], lb = mt->emissive[2];
      if (!(lr > 0.0f || lg > 0.0f || lb > 0.0f)) err = EM_ERR_DARK;
      else {
        const float* m = (const float*)(blas + (size_t)p.blasIdx * (RT_BLAS_STRIDE / 4) + 17);   // blas_node_t::transform @68
        const float* v = tri + (size_t)p.triIdx * 9;
        bool fin = true;
        for (int k = 0; k < 12; ++k) fin = fin && isfinite(m[k]);
        float V[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int a = 0; a < 3; ++a) { V[k][a] = refit_row(m + 4 * a, v[3 * k], v[3 * k + 1], v[3 * k + 2]); fin = fin && isfinite(V[k][a]); }
        if (!fin) err = EM_ERR_NONFINITE;
        else {
          const float e1x = __fsub_rn(V[1][0], V[0][0]), e1y = __fsub_rn(V[1][1], V[0][1]), e1z = __fsub_rn(V[1][2], V[0][2]);
          const float e2x = __fsub_rn(V[2][0], V[0][0]), e2y = __fsub_rn(V[2][1], V[0][1]), e2z = __fsub_rn(V[2][2], V[0][2]);
          const float cx = __fsub_rn(__fmul_rn(e1y, e2z), __fmul_rn(e1z, e2y));
          const float cy = __fsub_rn(__fmul_rn(e1z, e2x), __fmul_rn(e1x, e2z));
          const float cz = __fsub_rn(__fmul_rn(e1x, e2y), __fmul_rn(e1y, e2x));
          const float area = __fmul_rn(0.5f, __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)), __fmul_rn(cz, cz))));
          const float lmax = fmaxf(fmaxf(lr, lg), lb);
          we = __fmul_rn(area, lmax);
          if (!(area > 0.0f) || !isfinite(area) || !(we > 0.0f) || !isfinite(we)) { err = EM_ERR_AREA; we = 0.0f; }
          else {
            o12[0] = V[0][0]; o12[1] = V[0][1]; o12[2] = V[0][2]; o12[3] = e1x; o12[4] = e1y; o12[5] = e1z;
            o12[6] = e2x; o12[7] = e2y; o12[8] = e2z; o12[9] = lr; o12[10] = lg; o12[11] = lb;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) out[(size_t)e * 12 + k] = o12[k];
    w[e] = we;
  }
  uint32_t wb = __float_as_uint(we);   // (we >= 0)
  for (int o = 32; o > 0; o >>= 1) { wb = max(wb, (uint32_t)__shfl_down(wb, o)); err |= (uint32_t)__shfl_down(err, o); }
  if (threadIdx.x == 0) {
    if (err) atomicOr(res, err);
    if (wb) atomicMax(res + 1, wb);
  }
}

// q[e] = max(1, (uint32_t)((w[e] / wmax) * 65535.0f)); bsum[block] = the sum of the block's q
__global__ __launch_bounds__(64) void accel_emitter_q_kernel(uint32_t n, const float* __restrict__ w, const uint32_t* __restrict__ res, uint32_t* __restrict__ q,
                                                             uint32_t* __restrict__ bsum) {
  const uint32_t e = blockIdx.x * EM_BLOCK + threadIdx.x;
  const float wmax = __uint_as_float(res[1]);
  uint32_t v = 0u;
  if (e < n) {
    const float x = __fmul_rn(__fdiv_rn(w[e], wmax), 65535.0f);   // (in [0, 65535] for a table without errors; anything else is discarded by the host)
    v = x >= 1.0f && x <= 65535.0f ? (uint32_t)x : 1u;
    q[e] = v;
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if (threadIdx.x == 0) bsum[blockIdx.x] = v;
}

// boff[i] = the sum of bsum[0 .. i).  ONE wavefront: pass k scans block sums [k * EM_PASS, (k + 1) * EM_PASS) and every lane carries the
// running total into the next pass; the number of passes is known at entry.
__global__ __launch_bounds__(64) void accel_emitter_scan_kernel(uint32_t nb, const uint32_t* __restrict__ bsum, uint32_t* __restrict__ boff) {
  const uint32_t lane = threadIdx.x;
  const uint32_t passes = (nb + EM_PASS - 1u) / EM_PASS;
  uint32_t carry = 0u;
  for (uint32_t k = 0; k < passes; ++k) {
    const uint32_t i = k * EM_PASS + lane;
    const uint32_t v = i < nb ? bsum[i] : 0u;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += y; }
    if (i < nb) boff[i] = carry + (inc - v);
    carry += (uint32_t)__shfl(inc, 63);
  }
}

// cum[e] = boff[block of e] + the sum of q over the block's entries up to and including e
__global__ __launch_bounds__(64) void accel_emitter_cum_kernel(uint32_t n, const uint32_t* __restrict__ q, const uint32_t* __restrict__ boff, uint32_t* __restrict__ cum) {
  const uint32_t lane = threadIdx.x, e = blockIdx.x * EM_BLOCK + lane;
  uint32_t inc = e < n ? q[e] : 0u;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += y; }
  if (e < n) cum[e] = boff[blockIdx.x] + inc;
}

// The emitter index (the header's "Multiple importance sampling").  Dropped behind a synchronisation its caller has made: no frame in
// flight reads it.
static void emitter_index_drop(vxrt_accel* a) {
  (void)hipFree(a->em_idx);
  a->em_idx = nullptr; a->em_idx_n = 0u;
}

// Built on the host: at most 65,536 keys of 12 bytes sorted by (blasIdx, triIdx, e) -- a total order, so the same bits whatever the sort
// does -- and uploaded once.  The index is a buffer that grows from nothing: one synchronisation of s, behind which the sorted keys may
// leave the host; with an index held, nothing.  (Frames in flight on other streams do not read an index that does not exist yet.)
int emitter_index_ensure(vxrt_accel* a, hipStream_t s) {
  const uint32_t n = a->em_n;
  if (a->em_idx) return 0;   // (every set drops it: an index held is the table's)
  if (n == 0u || a->em_pairs.size() != n) return -1;
  struct Key { uint32_t b, t, e; };   // (an entry of the index: three words)
  std::vector<Key> ent(n);
  for (uint32_t e = 0; e < n; ++e) ent[e] = Key{a->em_pairs[e].blasIdx, a->em_pairs[e].triIdx, e};
  std::sort(ent.begin(), ent.end(), [](const Key& x, const Key& y) { return x.b != y.b ? x.b < y.b : (x.t != y.t ? x.t < y.t : x.e < y.e); });
  uint32_t* d = nullptr;
  if (hipMalloc((void**)&d, (size_t)n * 12) != hipSuccess) { (void)hipGetLastError(); return -1; }
  const bool ok = hipMemcpyAsync(d, ent.data(), (size_t)n * 12, hipMemcpyHostToDevice, s) == hipSuccess;
  if (hipStreamSynchronize(s) != hipSuccess || !ok) { (void)hipFree(d); return -1; }
  a->em_idx = d; a->em_idx_n = n;
  return 0;
}

extern "C" {

int vxrt_accel_build(const vxrt_scene_t* s, void* stream, vxrt_accel_t** out) {
  if (!s || !out || !s->tlas || !s->blas || !s->bvh || !s->tri) return -1;
  if (s->n_tlas_nodes == 0 || s->n_blas == 0 || s->n_bvh_nodes == 0 || s->n_tris == 0) return -1;
  if ((uint64_t)s->n_tlas_nodes + s->n_bvh_nodes > PAYLOAD_MASK || s->n_tris >= 0x7fffffffu) return -1;   // one compact index space
  hipStream_t st = (hipStream_t)stream;
  // instance node ranges (host side, n_blas is small): sorted unique bvh_offsets
  std::vector<uint32_t> recs((size_t)s->n_blas * (RT_BLAS_STRIDE / 4));
  if (hipStreamSynchronize(st) != hipSuccess) return -1;
  if (hipMemcpy(recs.data(), s->blas, recs.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  std::vector<uint32_t> bases;
  float max_refl = 0.0f;
  for (uint32_t j = 0; j < s->n_blas; ++j) {
    const uint32_t off = recs[(size_t)j * (RT_BLAS_STRIDE / 4)];
    if (off >= s->n_bvh_nodes) return -1;
    bases.push_back(off);
    float refl;
    memcpy(&refl, &recs[(size_t)j * (RT_BLAS_STRIDE / 4) + 38], sizeof(float));   // blas_node_t::reflectivity @152
    if (refl > max_refl) max_refl = refl;
  }
  std::sort(bases.begin(), bases.end());
  bases.erase(std::unique(bases.begin(), bases.end()), bases.end());
  std::vector<uint32_t> ends(bases.size());
  for (size_t j = 0; j < bases.size(); ++j) ends[j] = j + 1 < bases.size() ? bases[j + 1] : s->n_bvh_nodes;

  auto a = new (std::nothrow) vxrt_accel();
  if (!a) return -1;
  a->ref = *s;
  a->max_reflectivity = max_refl;
  (void)hipGetDevice(&a->device);
  uint32_t* d_ranges = nullptr;
  uint32_t* d_status = nullptr;
  uint32_t* d_troot = nullptr;
  constexpr uint32_t TOP_CAP = RT_TOP_NODES;
  // slot descriptors use bit 29 of the payload: only scenes whose compact index space stays below it are staged
  const bool stage_top = TOP_CAP > 0 && (uint64_t)s->n_tlas_nodes + s->n_bvh_nodes < DESC_TOP_FLAG;
  bool ok = hipMalloc(&a->nodes_c, ((size_t)s->n_tlas_nodes + s->n_bvh_nodes) * CNODE_VEC4 * 16) == hipSuccess &&
            (!stage_top || (hipMalloc(&a->top_img, (size_t)TOP_CAP * CNODE_VEC4 * 16) == hipSuccess &&
                            hipMalloc((void**)&a->top_roots, ((size_t)s->n_blas + 2) * sizeof(uint32_t)) == hipSuccess)) &&
            hipMalloc(&a->tri_w, (size_t)s->n_tris * WTRI_FLOATS * 4) == hipSuccess &&
            hipMalloc(&a->blas_root, (size_t)s->n_blas * sizeof(uint32_t)) == hipSuccess &&
            hipMalloc((void**)&d_ranges, bases.size() * 8) == hipSuccess &&
            hipMalloc((void**)&d_status, 8) == hipSuccess && hipMalloc((void**)&d_troot, 4) == hipSuccess;
  uint32_t hstatus = 0, troot = DESC_DONE, hstatus2[2] = {0, 0};   // [1]: what the BLAS re-layout found (kept for the refit)
  if (ok) {
    ok = hipMemcpy(d_ranges, bases.data(), bases.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_ranges + bases.size(), ends.data(), ends.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(d_status, 0, 8) == hipSuccess;
  }
  if (ok) {
    const uint32_t nb = (uint32_t)bases.size();
    hipLaunchKernelGGL(accel_nodes_kernel, dim3((s->n_tlas_nodes + 255) / 256), dim3(256), 0, st, (const uint32_t*)s->tlas, s->n_tlas_nodes,
                       (uint4*)a->nodes_c, 1, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, s->n_tris, s->n_blas, 0u, d_status);
    hipLaunchKernelGGL(accel_nodes_kernel, dim3((s->n_bvh_nodes + 255) / 256), dim3(256), 0, st, (const uint32_t*)s->bvh, s->n_bvh_nodes,
                       (uint4*)a->nodes_c + (size_t)s->n_tlas_nodes * CNODE_VEC4, 0, d_ranges, d_ranges + nb, nb, s->n_tris, s->n_blas, s->n_tlas_nodes, d_status + 1);
    hipLaunchKernelGGL(accel_tris_kernel, dim3((s->n_tris + 255) / 256), dim3(256), 0, st, (const float*)s->tri, s->n_tris, (float4*)a->tri_w);
    hipLaunchKernelGGL(accel_roots_kernel, dim3((s->n_blas + 1 + 255) / 256), dim3(256), 0, st, (const uint32_t*)s->tlas, (const uint32_t*)s->bvh,
                       (const uint32_t*)s->blas, s->n_tlas_nodes, s->n_bvh_nodes, s->n_blas, s->n_tris, d_troot, (uint32_t*)a->blas_root, d_status);
    if (s->triEx && s->mat && s->n_mats) {
      const uint32_t nchk = std::max(s->n_tris, s->n_mats);
      hipLaunchKernelGGL(accel_check_shading_kernel, dim3((nchk + 255) / 256), dim3(256), 0, st, (const rt_triex_t*)s->triEx, s->n_tris,
                         (const rt_material_t*)s->mat, s->n_mats, (uint64_t)s->tex_bytes, s->tex ? 1 : 0, d_status);
    }
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
         hipMemcpy(hstatus2, d_status, 8, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(&troot, d_troot, 4, hipMemcpyDeviceToHost) == hipSuccess;
    hstatus = hstatus2[0] | hstatus2[1];
    a->blas_status = hstatus2[1] & STATUS_FMA_DECODE_DIFFERS;
  }
  uint32_t n_top = 0, troot_top = troot;
  if (ok && stage_top && (hstatus & (STATUS_BAD_SCENE | STATUS_FMA_DECODE_DIFFERS)) == 0) {
    ok = hipMemsetAsync(a->top_img, 0, (size_t)TOP_CAP * CNODE_VEC4 * 16, st) == hipSuccess;
    hipLaunchKernelGGL(accel_top_kernel, dim3(1), dim3(64), 0, st, (const uint4*)a->nodes_c, troot, (const uint32_t*)a->blas_root, s->n_blas, TOP_CAP,
                       (uint4*)a->top_img, a->top_roots, a->top_roots + 1, a->top_roots + 2);
    uint32_t hdr[2] = {0, DESC_DONE};
    ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
         hipMemcpy(hdr, a->top_roots, sizeof hdr, hipMemcpyDeviceToHost) == hipSuccess;
    n_top = hdr[0]; troot_top = hdr[1];
  }
  // depth class of the scene (see accel_depth_kernel): RT_SHALLOW_LEVELS + 1 passes, no host round trip in between -- a scene that still
  // reaches new nodes in the last one is deeper than the class
  uint32_t levels = 0;
  if (ok && (hstatus & STATUS_BAD_SCENE) == 0) {
    const uint32_t nc = s->n_tlas_nodes + s->n_bvh_nodes;
    uint32_t* d_depth = nullptr;
    ok = hipMalloc((void**)&d_depth, ((size_t)nc + 1) * 4) == hipSuccess && hipMemsetAsync(d_depth, 0, ((size_t)nc + 1) * 4, st) == hipSuccess;
    if (ok) {
      for (uint32_t level = 1; level <= RT_SHALLOW_LEVELS + 1u; ++level)
        hipLaunchKernelGGL(accel_depth_kernel, dim3(level == 1u ? 1u : (nc + 255) / 256), dim3(256), 0, st, (const uint4*)a->nodes_c, nc, troot,
                           (const uint32_t*)a->blas_root, level, d_depth, d_depth + nc);
      ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
           hipMemcpy(&levels, d_depth + nc, 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d_depth);
  }
  (void)hipFree(d_ranges); (void)hipFree(d_status); (void)hipFree(d_troot);
  if (!ok || (hstatus & STATUS_BAD_SCENE) != 0) { accel_free(a); return -1; }   // malformed tree: rejected before any traversal
  static const int shallow_env = [] { const char* e = getenv("VXRT_SHALLOW"); return e ? atoi(e) : -1; }();   // (measurement knob: 0 = full-size stacks for every scene)
  a->levels = levels;
  a->shallow = levels <= RT_SHALLOW_LEVELS && shallow_env != 0;
  a->dev.nodes_c = (const uint4*)a->nodes_c; a->dev.ref_tlas = (const uint32_t*)s->tlas; a->dev.n_tlas = s->n_tlas_nodes; a->dev.tri_w = (const float4*)a->tri_w;
  a->dev.blas_root = (const uint32_t*)a->blas_root; a->dev.tlas_root = troot;
  a->dev.ident_root = 0u;
  if (troot >= 0xC0000000u && troot < DESC_IDLE) {   // (an instance descriptor) a single instance under the TLAS root: is its inverse transform (dwords 1-12 of the record) the identity?
    float m[12];
    static const bool ident_off = [] { const char* e = getenv("VXRT_IDENT_ROOT"); return e && e[0] == '0'; }();
    if (!ident_off && hipMemcpy(m, (const uint32_t*)s->blas + (size_t)(troot & PAYLOAD_MASK) * (RT_BLAS_STRIDE / 4) + 1, sizeof m, hipMemcpyDeviceToHost) == hipSuccess) {
      bool id = true;
      for (int i = 0; i < 12; ++i) id = id && m[i] == ((i % 5 == 0) ? 1.0f : 0.0f);     // (m[0], m[5], m[10] on the diagonal; -0 == 0)
      a->dev.ident_root = id ? 1u : 0u;
    }
  }
  a->dev.exact_decode = (hstatus & STATUS_FMA_DECODE_DIFFERS) ? 1u : 0u;
  a->dev.ref_bvh = (const uint32_t*)s->bvh;
  a->dev.blas = (const uint32_t*)s->blas; a->dev.triEx = (const rt_triex_t*)s->triEx;
  a->dev.mat = (const rt_material_t*)s->mat; a->dev.tex = (const uint8_t*)s->tex;
  a->dev.top_img = (const uint4*)a->top_img; a->dev.n_top = n_top; a->dev.tlas_root_top = troot_top;
  a->dev.blas_root_top = n_top ? a->top_roots + 2 : (const uint32_t*)a->blas_root;
  if (getenv("VXRT_DEBUG")) fprintf(stderr, "[vxrt] accel: %u top-of-tree nodes staged for LDS (cap %u)\n", n_top, TOP_CAP);
  // path table: for the accels whose shadow frames take the identity-root kernels as built (see vxrt_accel::tri_path).  Without it the
  // accel renders as it always did, so a failure here only leaves the table out.
  if (RT_SHALLOW_LEVELS <= PATH_LEVELS_MAX && ident_root_form(a)) {
    const uint32_t nc = s->n_tlas_nodes + s->n_bvh_nodes;
    uint32_t root = DESC_DONE;
    uint32_t* d_lvl = nullptr;   // level, then code, per compact node
    bool pok = hipMemcpy(&root, (const uint32_t*)a->blas_root + (troot & PAYLOAD_MASK), 4, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMalloc((void**)&a->tri_path, (size_t)s->n_tris * 4) == hipSuccess && hipMemsetAsync(a->tri_path, 0, (size_t)s->n_tris * 4, st) == hipSuccess;
    if (pok && root < 0x80000000u && (root & PAYLOAD_MASK) < nc) {   // (a root that is a leaf: every code is 0)
      const uint32_t one = 1u;
      pok = hipMalloc((void**)&d_lvl, (size_t)nc * 8) == hipSuccess && hipMemsetAsync(d_lvl, 0, (size_t)nc * 8, st) == hipSuccess &&
            hipMemcpyAsync(d_lvl + (root & PAYLOAD_MASK), &one, 4, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
      if (pok) {
        for (uint32_t level = 1; level <= RT_SHALLOW_LEVELS; ++level)
          hipLaunchKernelGGL(accel_path_kernel, dim3((nc + 255) / 256), dim3(256), 0, st, (const uint4*)a->nodes_c, nc, level, d_lvl, d_lvl + nc,
                             (const uint32_t*)s->bvh, s->n_bvh_nodes, s->n_tris, a->tri_path);
        pok = hipGetLastError() == hipSuccess;
      }
    }
    pok = hipStreamSynchronize(st) == hipSuccess && pok;
    (void)hipFree(d_lvl);
    if (!pok) { (void)hipFree(a->tri_path); a->tri_path = nullptr; }
  }
  *out = a;
  return 0;
}

int vxrt_accel_destroy(vxrt_accel_t* a) {
  if (!a) return 0;
  accel_free(a);
  return 0;
}

uint64_t vxrt_accel_bytes(const vxrt_accel_t* a) {
  if (!a) return 0;
  return (uint64_t)a->ref.n_tlas_nodes * CNODE_VEC4 * 16 + (uint64_t)a->ref.n_bvh_nodes * CNODE_VEC4 * 16 +
         (uint64_t)a->ref.n_tris * WTRI_FLOATS * 4 + (uint64_t)a->ref.n_blas * 4 +
         (a->tri_path ? (uint64_t)a->ref.n_tris * 4 : 0) +   // (the path table)
         ((a->motion_what & VXRT_REFIT_INSTANCES) ? (uint64_t)a->ref.n_blas * RT_BLAS_STRIDE : 0) +   // (the motion snapshot)
         ((a->motion_what & VXRT_REFIT_GEOMETRY) ? (uint64_t)a->ref.n_tris * RT_TRI_BYTES : 0) +
         (uint64_t)a->em_n * 56u +   // (the emitter table: 12 floats, q and cum per entry)
         (uint64_t)a->em_idx_n * 12u;   // (the emitter index, from its build on: blasIdx, triIdx, e per entry)
}

int vxrt_accel_info(const vxrt_accel_t* a, uint32_t which, uint64_t* value) {
  if (!a || !value) return -1;
  switch (which) {
  case 0: *value = a->levels; return 0;            // internal levels on the longest root-to-leaf path, counted up to RT_SHALLOW_LEVELS + 1
  case 1: *value = a->shallow ? 1u : 0u; return 0; // the timed launches take the SHALLOW instantiations (48-entry stacks)
  case 2: *value = a->dev.ident_root; return 0;    // the TLAS root is one identity instance (rays keep their world coordinates)
  case 3: *value = a->dev.exact_decode; return 0;  // the scene takes the ldexp decode / generic slab form
  case 4: *value = a->alpha_on ? 1u : 0u; return 0; // a non-zero alpha table is set (vxrt_accel_set_alpha_test)
  case 5: *value = ident_root_form(a) ? 1u : 0u; return 0; // timed plain / shadow frames take the identity-root kernels (no TLAS level in the loop)
  case 6: *value = a->motion_what; return 0;       // the VXRT_REFIT_* mask of the motion snapshot held (vxrt_accel_motion_snapshot)
  case 7: *value = emitters_valid(a) ? a->em_n : 0u; return 0; // emitters of a valid emitter table (vxrt_accel_set_emitters)
  case 8: *value = a->em_idx_n; return 0;          // entries of the emitter index (0: none built since the last vxrt_accel_set_emitters)
  case 9: *value = a->tri_path ? 1u : 0u; return 0; // the accel holds a path table (shadow hints: see vxrt_accel::tri_path)
  }
  return -1;
}

// alpha_tri[t] = threshold of triangle t's material (texId < n_mats: checked by the build)
__global__ __launch_bounds__(256) void accel_alpha_tri_kernel(const rt_triex_t* __restrict__ triEx, uint32_t n_tris, const uint8_t* __restrict__ thr, uint32_t n_mats,
                                                             uint8_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tris) return;
  const uint32_t m = triEx[t].texId;
  out[t] = m < n_mats ? thr[m] : (uint8_t)0;
}

// The alpha table (see the header).  Every refusal comes before anything is written; then, behind everything already issued on the accel,
// the thresholds go to the accel's own storage and the per-triangle table the traversal reads is derived from them.
int vxrt_accel_set_alpha_test(vxrt_accel_t* a, const uint8_t* thresholds, uint32_t n_mats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!a || a->stale) return -1;
  const vxrt_scene_t& s = a->ref;
  bool any = false;
  if (thresholds) {
    if (n_mats != s.n_mats) return -1;
    for (uint32_t m = 0; m < n_mats; ++m) any = any || thresholds[m] != 0;
  }
  if (any) {
    if (!s.triEx || !s.mat || !s.tex) return -1;
    std::vector<rt_material_t> mats(n_mats);
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(mats.data(), s.mat, (size_t)n_mats * sizeof(rt_material_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (uint32_t m = 0; m < n_mats; ++m)
      if (thresholds[m] != 0 && mats[m].diffuse_tex_id < 0) return -1;   // a cutout needs a texture (whose texel range the build has checked)
    if (!a->alpha_mat && hipMalloc((void**)&a->alpha_mat, std::max<size_t>(s.n_mats, 16)) != hipSuccess) return -1;
    if (!a->alpha_tri && hipMalloc((void**)&a->alpha_tri, std::max<size_t>(s.n_tris, 16)) != hipSuccess) return -1;
  }
  // ordered after every call already issued on this accel, on any stream (frames in flight read the table this call rewrites)
  for (uint32_t k = 0; k < MAX_FRAMES_IN_FLIGHT; ++k) {
    FrameCtx& c = a->ctx[k];
    if (!c.busy || c.last_stream == st) continue;
    if (c.done_recorded) { if (hipStreamWaitEvent(st, c.ev_done, 0) != hipSuccess) return -1; }
    else if (hipDeviceSynchronize() != hipSuccess) return -1;
  }
  if (any) {
    if (hipMemcpyAsync(a->alpha_mat, thresholds, n_mats, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    hipLaunchKernelGGL(accel_alpha_tri_kernel, dim3((s.n_tris + 255) / 256), dim3(256), 0, st, (const rt_triex_t*)s.triEx, s.n_tris,
                       (const uint8_t*)a->alpha_mat, n_mats, a->alpha_tri);
    if (hipGetLastError() != hipSuccess) { a->alpha_on = false; (void)hipStreamSynchronize(st); return -1; }
  }
  if (hipStreamSynchronize(st) != hipSuccess) { a->alpha_on = false; return -1; }
  a->alpha_on = any;
  return 0;
}

// The motion snapshot (see the header, "Motion").  Every refusal comes before anything is changed; then, behind everything already
// issued on the accel, the scene's instance records (and vertices) are copied to the accel's own storage.  Storage that a new mask no
// longer asks for is freed behind a device synchronisation: motion frames in flight on any stream read it.
int vxrt_accel_motion_snapshot(vxrt_accel_t* a, uint32_t what, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!a || a->stale || (what & ~(uint32_t)(VXRT_REFIT_INSTANCES | VXRT_REFIT_GEOMETRY)) != 0u) return -1;
  if ((what & VXRT_REFIT_GEOMETRY) && !(what & VXRT_REFIT_INSTANCES)) return -1;
  const vxrt_scene_t& s = a->ref;
  const size_t blas_bytes = (size_t)s.n_blas * RT_BLAS_STRIDE, tri_bytes = (size_t)s.n_tris * RT_TRI_BYTES;
  // ordered after every call already issued on this accel, on any stream (frames in flight read the snapshot this call rewrites)
  for (uint32_t k = 0; k < MAX_FRAMES_IN_FLIGHT; ++k) {
    FrameCtx& c = a->ctx[k];
    if (!c.busy || c.last_stream == st) continue;
    if (c.done_recorded) { if (hipStreamWaitEvent(st, c.ev_done, 0) != hipSuccess) return -1; }
    else if (hipDeviceSynchronize() != hipSuccess) return -1;
  }
  if (what != a->motion_what) {
    uint32_t* nb = nullptr; float* nt = nullptr;
    const bool want_b = (what & VXRT_REFIT_INSTANCES) && !a->motion_blas, want_t = (what & VXRT_REFIT_GEOMETRY) && !a->motion_tri;
    if ((want_b && hipMalloc((void**)&nb, blas_bytes) != hipSuccess) || (want_t && hipMalloc((void**)&nt, tri_bytes) != hipSuccess)) {
      (void)hipFree(nb); (void)hipFree(nt); (void)hipGetLastError();
      return -1;
    }
    const bool drop_b = !(what & VXRT_REFIT_INSTANCES) && a->motion_blas, drop_t = !(what & VXRT_REFIT_GEOMETRY) && a->motion_tri;
    if ((drop_b || drop_t) && hipDeviceSynchronize() != hipSuccess) { (void)hipFree(nb); (void)hipFree(nt); return -1; }
    if (drop_b) { (void)hipFree(a->motion_blas); a->motion_blas = nullptr; }
    if (drop_t) { (void)hipFree(a->motion_tri); a->motion_tri = nullptr; }
    if (want_b) a->motion_blas = nb;
    if (want_t) a->motion_tri = nt;
    a->motion_what = 0;   // (until the copies below have landed)
  }
  if (what == 0u) return 0;
  bool ok = hipMemcpyAsync(a->motion_blas, s.blas, blas_bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
  if (ok && (what & VXRT_REFIT_GEOMETRY)) ok = hipMemcpyAsync(a->motion_tri, s.tri, tri_bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
  ok = hipStreamSynchronize(st) == hipSuccess && ok;
  a->motion_what = ok ? what : 0u;
  return ok ? 0 : -1;
}

// The emitter table (see the header, "Emissive geometry").  The refusals that need no device work come first; then, behind everything
// already issued on the accel, a NEW table is built next to the one held -- what the device refuses is only known at the end -- and takes
// its place when every entry passed: the previous table is kept by every failure, and freed behind the synchronisation that ends the call.
int vxrt_accel_set_emitters(vxrt_accel_t* a, const vxrt_emitter_t* pairs, uint32_t n, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!a || a->stale || n > VXRT_MAX_EMITTERS) return -1;
  const vxrt_scene_t& s = a->ref;
  const bool drop = !pairs || n == 0u;
  if (!drop && (!s.triEx || !s.mat || s.n_mats == 0u)) return -1;
  // ordered after every call already issued on this accel, on any stream (frames in flight read the table this call replaces)
  for (uint32_t k = 0; k < MAX_FRAMES_IN_FLIGHT; ++k) {
    FrameCtx& c = a->ctx[k];
    if (!c.busy || c.last_stream == st) continue;
    if (c.done_recorded) { if (hipStreamWaitEvent(st, c.ev_done, 0) != hipSuccess) return -1; }
    else if (hipDeviceSynchronize() != hipSuccess) return -1;
  }
  if (drop) {
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    (void)hipFree(a->em_tri); (void)hipFree(a->em_q); (void)hipFree(a->em_cum);
    a->em_tri = nullptr; a->em_q = nullptr; a->em_cum = nullptr; a->em_n = 0u; a->em_Q = 0u; a->em_valid = false;
    emitter_index_drop(a);
    a->em_pairs.clear();
    return 0;
  }
  const uint32_t nb = (n + EM_BLOCK - 1u) / EM_BLOCK;
  float* tri = nullptr; uint32_t* q = nullptr; uint32_t* cum = nullptr;
  vxrt_emitter_t* d_pairs = nullptr; float* w = nullptr; uint32_t* blk = nullptr; uint32_t* res = nullptr;   // scratch: blk = bsum[nb], boff[nb]
  uint32_t hres[2] = {0u, 0u}, Q = 0u;
  bool ok = hipMalloc((void**)&tri, (size_t)n * 48) == hipSuccess && hipMalloc((void**)&q, (size_t)n * 4) == hipSuccess &&
            hipMalloc((void**)&cum, (size_t)n * 4) == hipSuccess && hipMalloc((void**)&d_pairs, (size_t)n * sizeof(vxrt_emitter_t)) == hipSuccess &&
            hipMalloc((void**)&w, (size_t)n * 4) == hipSuccess && hipMalloc((void**)&blk, (size_t)nb * 8) == hipSuccess &&
            hipMalloc((void**)&res, 8) == hipSuccess;
  ok = ok && hipMemcpyAsync(d_pairs, pairs, (size_t)n * sizeof(vxrt_emitter_t), hipMemcpyHostToDevice, st) == hipSuccess &&
       hipMemsetAsync(res, 0, 8, st) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(accel_emitter_tris_kernel, dim3(nb), dim3(EM_BLOCK), 0, st, (const vxrt_emitter_t*)d_pairs, n, (const uint32_t*)s.blas, s.n_blas,
                       (const float*)s.tri, s.n_tris, (const rt_triex_t*)s.triEx, (const rt_material_t*)s.mat, s.n_mats, tri, w, res);
    hipLaunchKernelGGL(accel_emitter_q_kernel, dim3(nb), dim3(EM_BLOCK), 0, st, n, (const float*)w, (const uint32_t*)res, q, blk);
    hipLaunchKernelGGL(accel_emitter_scan_kernel, dim3(1), dim3(EM_PASS), 0, st, nb, (const uint32_t*)blk, blk + nb);
    hipLaunchKernelGGL(accel_emitter_cum_kernel, dim3(nb), dim3(EM_BLOCK), 0, st, n, (const uint32_t*)q, (const uint32_t*)(blk + nb), cum);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(hres, res, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpyAsync(&Q, cum + (n - 1u), 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  }
  ok = hipStreamSynchronize(st) == hipSuccess && ok;   // (the pairs are the caller's again; frames in flight have finished with the table held)
  (void)hipFree(d_pairs); (void)hipFree(w); (void)hipFree(blk); (void)hipFree(res);
  if (!ok || hres[0] != 0u || Q == 0u) {
    (void)hipFree(tri); (void)hipFree(q); (void)hipFree(cum); (void)hipGetLastError();
    if (getenv("VXRT_DEBUG")) fprintf(stderr, "[vxrt] set_emitters refused: ok %d, errors %u\n", (int)ok, hres[0]);
    return -1;
  }
  (void)hipFree(a->em_tri); (void)hipFree(a->em_q); (void)hipFree(a->em_cum);
  a->em_tri = tri; a->em_q = q; a->em_cum = cum; a->em_n = n; a->em_Q = Q; a->em_valid = true;
  emitter_index_drop(a);   // (the index is of the table replaced: the next call that needs one builds it from the pairs kept here)
  a->em_pairs.assign(pairs, pairs + n);
  return 0;
}

int vxrt_accel_read_emitters(vxrt_accel_t* a, float* tri12, uint32_t* q, uint32_t* cum, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!a || !emitters_valid(a)) return -1;
  if (hipStreamSynchronize(st) != hipSuccess) return -1;
  const size_t n = a->em_n;
  if (tri12 && hipMemcpy(tri12, a->em_tri, n * 48, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (q && hipMemcpy(q, a->em_q, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (cum && hipMemcpy(cum, a->em_cum, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return 0;
}

int vxrt_accel_frames_in_flight(vxrt_accel_t* a, uint32_t n) {
  if (!a || n < 1 || n > MAX_FRAMES_IN_FLIGHT) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  a->n_ctx = n; a->next_ctx = 0;
  return 0;
}

// The refit plan, built on the host from the reference nodes (the topology never changes, so this runs once per accel): breadth-first
// from the TLAS root and from every distinct BLAS root (sorted unique bvh_offsets, as the build takes them; a BLAS shared by several
// instances is one tree), each node's level within its own tree; internal nodes are bucketed by level (count, scan, scatter).
// a refit that fails reports where with VXRT_DEBUG set, and leaves no HIP error behind for the caller's next launch to trip over
static int refit_fail(const char* where) {
  const hipError_t e = hipGetLastError();
  if (getenv("VXRT_DEBUG")) fprintf(stderr, "[vxrt] refit failed: %s (%s)\n", where, hipGetErrorString(e));
  return -1;
}

static RefitPlan* refit_plan_build(vxrt_accel* a, hipStream_t st) {
  const vxrt_scene_t& s = a->ref;
  std::vector<uint32_t> tl((size_t)s.n_tlas_nodes * RT_NODE_DWORDS), bv((size_t)s.n_bvh_nodes * RT_NODE_DWORDS), recs((size_t)s.n_blas * (RT_BLAS_STRIDE / 4));
  if (hipStreamSynchronize(st) != hipSuccess ||
      hipMemcpy(tl.data(), s.tlas, tl.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(bv.data(), s.bvh, bv.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(recs.data(), s.blas, recs.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { refit_fail("plan: node copy"); return nullptr; }
  std::vector<uint32_t> bases;
  for (uint32_t j = 0; j < s.n_blas; ++j) bases.push_back(recs[(size_t)j * (RT_BLAS_STRIDE / 4)]);
  std::sort(bases.begin(), bases.end());
  bases.erase(std::unique(bases.begin(), bases.end()), bases.end());
  std::vector<uint32_t> ends(bases.size());
  for (size_t j = 0; j < bases.size(); ++j) ends[j] = j + 1 < bases.size() ? bases[j + 1] : s.n_bvh_nodes;
  // one tree: leaves out, internal nodes (node, child 0) with their level; false on an index the build would have rejected
  auto walk = [](const std::vector<uint32_t>& w, uint32_t root, uint32_t base, uint32_t end, bool tlas, std::vector<uint32_t>& leaves,
                 std::vector<std::pair<uint32_t, uint2>>& items) -> bool {
    std::vector<std::pair<uint32_t, uint32_t>> q{{root, 0u}};
    for (size_t h = 0; h < q.size(); ++h) {
      const uint32_t i = q[h].first, L = q[h].second;
      const uint32_t* n = w.data() + (size_t)i * RT_NODE_DWORDS;
      if (tlas ? n[5] != 0xffffffffu : n[5] != 0u) { leaves.push_back(i); continue; }
      const uint64_t c0 = (uint64_t)base + n[4];
      items.push_back({L, make_uint2(i, (uint32_t)c0)});
      const uint8_t* b = (const uint8_t*)n;
      bool any = false;
      for (uint32_t k = 0; k < 4; ++k) {
        if (b[24 + 7 * k] == 0) continue;
        if (c0 + k >= end || c0 + k <= i) return false;
        q.push_back({(uint32_t)(c0 + k), L + 1u});
        any = true;
      }
      if (!any) return false;   // an internal node without a child has no box to refit from: refused before anything is written
    }
    return true;
  };
  std::vector<uint32_t> bl, tlv;
  std::vector<std::pair<uint32_t, uint2>> bi, ti;
  for (size_t j = 0; j < bases.size(); ++j)
    if (!walk(bv, bases[j], bases[j], ends[j], false, bl, bi)) { refit_fail("plan: BLAS walk"); return nullptr; }
  if (!walk(tl, 0u, 0u, s.n_tlas_nodes, true, tlv, ti)) { refit_fail("plan: TLAS walk"); return nullptr; }
  for (uint32_t i : tlv) if (tl[(size_t)i * RT_NODE_DWORDS + 5] >= s.n_blas) { refit_fail("plan: instance index"); return nullptr; }
  auto bucket = [](const std::vector<std::pair<uint32_t, uint2>>& it, std::vector<uint2>& out, std::vector<uint32_t>& lv) {
    uint32_t depth = 0;
    for (const auto& x : it) depth = std::max(depth, x.first + 1u);
    lv.assign(depth + 1u, 0u);
    for (const auto& x : it) ++lv[x.first + 1u];
    for (uint32_t L = 0; L < depth; ++L) lv[L + 1u] += lv[L];
    std::vector<uint32_t> pos(lv.begin(), lv.end() - 1);
    out.resize(it.size());
    for (const auto& x : it) out[pos[x.first]++] = x.second;
  };
  std::vector<uint32_t> ranges(bases);   // bases, then ends
  ranges.insert(ranges.end(), ends.begin(), ends.end());
  std::vector<uint2> bitems, titems;
  auto p = new (std::nothrow) RefitPlan();
  if (!p) return nullptr;
  bucket(bi, bitems, p->blas_lv);
  bucket(ti, titems, p->tlas_lv);
  p->n_blas_leaves = (uint32_t)bl.size(); p->n_tlas_leaves = (uint32_t)tlv.size(); p->nb = (uint32_t)bases.size();
  auto up = [](void** d, const void* h, size_t bytes) {
    return hipMalloc(d, std::max<size_t>(bytes, 16)) == hipSuccess && (bytes == 0 || hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess);
  };
  const bool ok = up((void**)&p->blas_leaves, bl.data(), bl.size() * 4) && up((void**)&p->blas_items, bitems.data(), bitems.size() * 8) &&
                  up((void**)&p->tlas_leaves, tlv.data(), tlv.size() * 4) && up((void**)&p->tlas_items, titems.data(), titems.size() * 8) &&
                  up((void**)&p->ranges, ranges.data(), ranges.size() * 4) &&
                  hipMalloc((void**)&p->fbox_bvh, (size_t)s.n_bvh_nodes * 24) == hipSuccess &&
                  hipMalloc((void**)&p->fbox_tlas, (size_t)s.n_tlas_nodes * 24) == hipSuccess &&
                  hipMalloc((void**)&p->res, REFIT_RES_WORDS * 4) == hipSuccess;
  if (!ok) { refit_fail("plan: upload"); refit_plan_free(p); return nullptr; }
  return p;
}

// Everything of one refit after the plan exists: the box passes, the re-layout, one host synchronisation, the flags.  `xf_first` /
// `xf_count`: set_transforms' records (its two kernels run first, on the same stream); xf_count == 0 for a plain refit.
static int refit_run(vxrt_accel* a, uint32_t what, hipStream_t st, const float* xf_in, uint32_t xf_first, uint32_t xf_count) {
  ++a->scene_gen;   // (whatever comes of it: hints a frame context holds were written for the scene before this call)
  RefitPlan* p = a->refit;
  const vxrt_scene_t& s = a->ref;
  // ordered after every call already issued on this accel, on any stream
  for (uint32_t k = 0; k < MAX_FRAMES_IN_FLIGHT; ++k) {
    FrameCtx& c = a->ctx[k];
    if (!c.busy || c.last_stream == st) continue;
    if (c.done_recorded) { if (hipStreamWaitEvent(st, c.ev_done, 0) != hipSuccess) return refit_fail("ordering"); }
    else if (hipDeviceSynchronize() != hipSuccess) return refit_fail("ordering");
  }
  const bool geom = (what & VXRT_REFIT_GEOMETRY) != 0u;
  auto grid = [](uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); };
  bool ok = hipMemsetAsync(p->res, 0, REFIT_RES_WORDS * 4, st) == hipSuccess;
  if (ok && xf_count) {
    hipLaunchKernelGGL(refit_xform_kernel, grid(xf_count), dim3(256), 0, st, xf_in, xf_count, p->xf, p->res);
    hipLaunchKernelGGL(refit_xform_commit_kernel, grid((uint64_t)xf_count * 32u), dim3(256), 0, st, (const float*)p->xf, xf_first, xf_count,
                       (uint32_t*)s.blas, (const uint32_t*)p->res);
  }
  if (ok && geom) {
    if (p->n_blas_leaves)
      hipLaunchKernelGGL(refit_blas_leaf_kernel, grid(p->n_blas_leaves), dim3(256), 0, st, (uint32_t*)s.bvh, (const float*)s.tri, p->blas_leaves,
                         p->n_blas_leaves, p->fbox_bvh, p->res);
    for (size_t L = p->blas_lv.size() - 1; L-- > 0;) {
      const uint32_t n = p->blas_lv[L + 1] - p->blas_lv[L];
      if (n) hipLaunchKernelGGL(refit_level_kernel, grid(n), dim3(256), 0, st, (uint32_t*)s.bvh, p->blas_items + p->blas_lv[L], n, p->fbox_bvh, p->res);
    }
  }
  if (ok) {
    if (p->n_tlas_leaves)
      hipLaunchKernelGGL(refit_instance_kernel, grid(p->n_tlas_leaves), dim3(256), 0, st, (uint32_t*)s.tlas, p->tlas_leaves, p->n_tlas_leaves,
                         (const uint32_t*)s.blas, (const uint32_t*)s.bvh, (const float*)s.tri, geom ? (const float*)p->fbox_bvh : (const float*)nullptr,
                         p->fbox_tlas, p->res);
    for (size_t L = p->tlas_lv.size() - 1; L-- > 0;) {
      const uint32_t n = p->tlas_lv[L + 1] - p->tlas_lv[L];
      if (n) hipLaunchKernelGGL(refit_level_kernel, grid(n), dim3(256), 0, st, (uint32_t*)s.tlas, p->tlas_items + p->tlas_lv[L], n, p->fbox_tlas, p->res);
    }
    // the re-layout of vxrt_accel_build over what moved
    hipLaunchKernelGGL(accel_nodes_kernel, grid(s.n_tlas_nodes), dim3(256), 0, st, (const uint32_t*)s.tlas, s.n_tlas_nodes,
                       (uint4*)a->nodes_c, 1, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, s.n_tris, s.n_blas, 0u, p->res);
    if (geom) {
      hipLaunchKernelGGL(accel_nodes_kernel, grid(s.n_bvh_nodes), dim3(256), 0, st, (const uint32_t*)s.bvh, s.n_bvh_nodes,
                         (uint4*)a->nodes_c + (size_t)s.n_tlas_nodes * CNODE_VEC4, 0, p->ranges, p->ranges + p->nb, p->nb, s.n_tris, s.n_blas, s.n_tlas_nodes,
                         p->res + 5);
      hipLaunchKernelGGL(accel_tris_kernel, grid(s.n_tris), dim3(256), 0, st, (const float*)s.tri, s.n_tris, (float4*)a->tri_w);
    }
    if (a->top_img) {   // re-staged whatever the flags say; used only if the scene keeps the fma decode (as the build decides)
      ok = hipMemsetAsync(a->top_img, 0, (size_t)RT_TOP_NODES * CNODE_VEC4 * 16, st) == hipSuccess;
      hipLaunchKernelGGL(accel_top_kernel, dim3(1), dim3(64), 0, st, (const uint4*)a->nodes_c, a->dev.tlas_root, (const uint32_t*)a->blas_root, s.n_blas,
                         (uint32_t)RT_TOP_NODES, (uint4*)a->top_img, a->top_roots, a->top_roots + 1, a->top_roots + 2);
    }
    hipLaunchKernelGGL(refit_finish_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)s.blas, a->dev.tlas_root, (const uint32_t*)a->top_roots, p->res);
  }
  uint32_t res[REFIT_RES_WORDS] = {0};
  ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
       hipMemcpy(res, p->res, sizeof res, hipMemcpyDeviceToHost) == hipSuccess;
  // (from here on the boxes in the scene's buffers and the layout are the refit's: either it all holds, or the accel is stale)
  if (!ok || res[1] != 0u || ((res[0] | res[5]) & STATUS_BAD_SCENE) != 0u) {
    a->stale = true;
    if (getenv("VXRT_DEBUG")) fprintf(stderr, "[vxrt] refit: ok %d, errors %u, status %u / %u\n", (int)ok, res[1], res[0], res[5]);
    return refit_fail("boxes");
  }
  if (geom) a->blas_status = res[5] & STATUS_FMA_DECODE_DIFFERS;
  const uint32_t st_all = (res[0] & STATUS_FMA_DECODE_DIFFERS) | a->blas_status;
  a->dev.exact_decode = st_all ? 1u : 0u;
  static const bool ident_off = [] { const char* e = getenv("VXRT_IDENT_ROOT"); return e && e[0] == '0'; }();
  a->dev.ident_root = ident_off ? 0u : res[2];
  if (a->top_img && !st_all) {
    a->dev.n_top = res[3]; a->dev.tlas_root_top = res[4]; a->dev.blas_root_top = a->top_roots + 2;
  } else {
    a->dev.n_top = 0; a->dev.tlas_root_top = a->dev.tlas_root; a->dev.blas_root_top = (const uint32_t*)a->blas_root;
  }
  a->stale = false;
  if (res[6] == 0u) a->em_valid = false;   // (the emitter table holds world-space data: what moved makes it stale until it is set again)
  return res[6] != 0u ? -1 : 0;   // set_transforms: a matrix was refused, the records are unchanged (and the refit of them holds)
}

static int refit_prepare(vxrt_accel* a, uint32_t what, hipStream_t st) {
  if (!a || (what & ~(uint32_t)(VXRT_REFIT_INSTANCES | VXRT_REFIT_GEOMETRY)) != 0u) return -1;
  if (!a->refit && !(a->refit = refit_plan_build(a, st))) return -1;
  return 0;
}

int vxrt_accel_refit(vxrt_accel_t* a, uint32_t what, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (refit_prepare(a, what, st) != 0) return -1;
  if (what == 0u) return a->stale ? -1 : 0;
  if (a->stale) what |= VXRT_REFIT_GEOMETRY;   // (the BLAS boxes of a failed GEOMETRY refit are not trusted: redo them)
  return refit_run(a, what, st, nullptr, 0, 0);
}

int vxrt_accel_set_transforms(vxrt_accel_t* a, uint32_t first, uint32_t count, const float* transforms, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!a || (count && !transforms) || (uint64_t)first + count > a->ref.n_blas) return -1;
  if (refit_prepare(a, VXRT_REFIT_INSTANCES, st) != 0) return -1;
  RefitPlan* p = a->refit;
  if (count > p->xf_cap) {
    if (hipStreamSynchronize(st) != hipSuccess) return refit_fail("scratch");
    (void)hipFree(p->xf); p->xf = nullptr; p->xf_cap = 0;
    if (hipMalloc((void**)&p->xf, (size_t)count * 32 * sizeof(float)) != hipSuccess) return refit_fail("scratch");
    p->xf_cap = count;
  }
  return refit_run(a, a->stale ? (VXRT_REFIT_INSTANCES | VXRT_REFIT_GEOMETRY) : VXRT_REFIT_INSTANCES, st, transforms, first, count);
}

}  // extern "C"
