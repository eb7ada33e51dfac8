// The path table of an accel (vxrt_accel::tri_path; read by the shadow hints, RT_SHADOW_HINTS in rt_kernels.hip): per triangle, the child
// slot taken at each internal level on the way from the BLAS root to the triangle's leaf -- 2 bits per level, the root's slot in the low
// bits, so 16 levels fill the 32-bit word.  A reader at the root takes slot `code & 3`, goes on with `code >> 2`, and so on.
// Compiled by hipcc into accel_path_kernel (rt_accel.hip) and by plain g++ into the stand-alone program of tests/test_shadow_paths_cpu.py,
// which follows every triangle's code through two small trees.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "rt_types.h"

#if defined(__HIPCC__)
#define RT_PATH_FN __host__ __device__ __forceinline__
#else
#define RT_PATH_FN inline
#endif

#define PATH_LEVELS_MAX 16u
#define CNODE_DWORDS (CNODE_VEC4 * 4)
#define CNODE_DESC0 10   // dwords 10..13 of a compact node: the four child descriptors (q2.z, q2.w, q3.x, q3.y)

RT_PATH_FN uint32_t path_slot(uint32_t code) { return code & 3u; }
RT_PATH_FN uint32_t path_rest(uint32_t code) { return code >> 2; }
// the code of the child in `slot` of a node of `level` (the root is level 1) that carries `code`
RT_PATH_FN uint32_t path_child_code(uint32_t code, uint32_t level, uint32_t slot) { return code | (slot << (2u * (level - 1u))); }

// One node of one pass.  The passes go top down, one per level; pass t touches the nodes of level t (lvl[i] == t; the caller marks the root
// with level 1 and code 0).  Every child gets the node's code with its own slot added: an internal child keeps it in ncode and gets level
// t + 1, a leaf writes it to its triangles -- an inline leaf names them in its descriptor, a leaf by reference (more than LEAF_MAX_INLINE
// triangles) in dwords 4 and 5 of its reference node.  Children lie after their parents and a BLAS is a tree, so a pass only writes
// entries no thread of the same pass reads.  Nothing outside [0, n_nodes), [0, n_bvh) and [0, n_tris) is touched.
RT_PATH_FN void path_pass_node(const uint32_t* nodes_c, uint32_t n_nodes, uint32_t i, uint32_t level, uint32_t* lvl, uint32_t* ncode,
                               const uint32_t* ref_bvh, uint32_t n_bvh, uint32_t n_tris, uint32_t* tri_path) {
  if (i >= n_nodes || level == 0u || level > PATH_LEVELS_MAX || lvl[i] != level) return;
  const uint32_t* d = nodes_c + (size_t)i * CNODE_DWORDS + CNODE_DESC0;
  const uint32_t code = ncode[i];
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t dk = d[k], cc = path_child_code(code, level, k);
    if (dk < 0x80000000u) {                       // an internal node
      const uint32_t c = dk & PAYLOAD_MASK;
      // (c > i: the accel build refuses a tree with a child stored in front of its parent -- accel_nodes_kernel, STATUS_BAD_SCENE -- so the
      // test drops nothing from a tree that was accepted; it keeps the pass finite on the host program's hand-made trees)
      if (c < n_nodes && c > i) { lvl[c] = level + 1u; ncode[c] = cc; }
    } else if ((dk >> 30) == DK_LEAF) {
      uint32_t first = dk & LEAF_FIRST_MASK, count = (dk >> LEAF_FIRST_BITS) & LEAF_MAX_INLINE;
      if (count == 0u) {
        if (first >= n_bvh) continue;
        const uint32_t* rn = ref_bvh + (size_t)first * RT_NODE_DWORDS;
        first = rn[4]; count = rn[5];
      }
      for (uint32_t t = 0; t < count; ++t) if ((uint64_t)first + t < n_tris) tri_path[first + t] = cc;
    }
  }
}
