// Shared host/device plain-data layouts of the reference's scene buffers.
// Sizes are part of the boundary: the host app uploads these bytes as produced by the
// reference's scene builder (tests/regression/raytracing/common.h, geometry.h).
#pragma once
#include <stdint.h>

#define RT_LARGE_FLOAT 1e30f       // rt_traversal.h:7, geometry.h:15
#define RT_EPSILON 1e-6f           // rt_traversal.cpp:7
#define RT_BVH_WIDTH 4             // hw/VX_config.toml:246, raytracing/common.h:18
#define RT_NODE_BYTES 52           // sizeof(bvh_quantized_node_t)
#define RT_NODE_DWORDS 13
#define RT_BLAS_STRIDE 160         // rt_traversal.cpp:112 (hard-coded `* 160`)
#define RT_TRI_BYTES 36
#define RT_MAX_TRAIL 32            // TraversalTrail levels (rt_traversal.h: trail[32]); deeper = undefined behaviour in the reference
#define RT_TRIEX_BYTES 64
#define RT_MAT_BYTES 88
#define RT_MAX_LEVELS 32           // MAX_TRAIL_LEVEL (rt_traversal.h:8): deeper trees are UB in the reference
#define RT_STACK_ENTRIES (3 * RT_MAX_LEVELS)  // <=3 pending siblings per level

#pragma pack(push, 1)
struct rt_child_t { uint8_t meta; uint8_t qaabb[6]; };
#pragma pack(pop)

struct rt_qnode_t {            // common.h:52-67 / sim rt_traversal.h:14-33
  float origin[3];
  int8_t ex, ey, ez;
  uint8_t imask;               // 1 = TLAS node, 0 = BLAS node
  uint32_t leftFirst;          // first child index | first triangle index (already mesh-offset)
  uint32_t leafData;           // BLAS: triCount (0 = internal); TLAS: blasIdx (UINT32_MAX = internal)
  rt_child_t children[RT_BVH_WIDTH];
};
static_assert(sizeof(rt_qnode_t) == RT_NODE_BYTES, "node layout");

struct rt_blas_t {             // common.h:86-99
  uint32_t bvh_offset;
  float invTransform[16];
  float transform[16];
  uint64_t mat_offset;
  uint32_t tex_width, tex_height;
  float reflectivity;
  uint32_t _pad;
};
static_assert(sizeof(rt_blas_t) == RT_BLAS_STRIDE, "blas layout");

struct rt_tri_t { float v0[3], v1[3], v2[3]; };                    // geometry.h:1401-1405
static_assert(sizeof(rt_tri_t) == RT_TRI_BYTES, "tri layout");

struct rt_triex_t {            // common.h:39-43
  float N0[3], N1[3], N2[3];
  float uv0[2], uv1[2], uv2[2];
  uint32_t texId;
};
static_assert(sizeof(rt_triex_t) == RT_TRIEX_BYTES, "triEx layout");

struct rt_material_t {         // common.h:20-36
  float ambient[3], diffuse[3], specular[3], emissive[3];
  float shininess, ior, dissolve, reflectivity;
  int32_t diffuse_tex_id, illum;
  uint32_t tex_width, tex_height;
  uint64_t tex_offset;
};
static_assert(sizeof(rt_material_t) == RT_MAT_BYTES, "material layout");

// ---------------------------------------------------------------------------------------------
// Compact device layout derived from the buffers above (built by rt_accel.hip, traversed by rt_kernels.hip; the layout
// itself is described in rt_internal.h).  Here, and not in rt_internal.h, because every value below is compiled into the
// timed kernels: this header is part of the kernels' source id.
// ---------------------------------------------------------------------------------------------
#define DK_TLAS 0u
#define DK_BLAS 1u
#define DK_LEAF 2u
#define DK_INST 3u
#define DESC(kind, payload) (((kind) << 30) | (payload))
#define DESC_DONE 0xFFFFFFFEu   // traversal of the lane's ray has ended
#define DESC_IDLE 0xFFFFFFFDu   // lane has no ray
#define DESC_NONE 0xFFFFFFFFu   // compact node: empty child slot
#define PAYLOAD_MASK 0x3FFFFFFFu
#define DESC_TOP_FLAG 0x20000000u   // node descriptor: payload = slot of the LDS-staged top-of-tree image (kernels with USE_TOP only)
#define DESC_TOP_SLOT 0x0000FFFFu
#define LEAF_FIRST_BITS 26
#define LEAF_FIRST_MASK 0x03FFFFFFu
#define LEAF_MAX_INLINE 15u
#define CNODE_VEC4 4
#define WTRI_FLOATS 12
#ifndef RT_SHALLOW_LEVELS
#define RT_SHALLOW_LEVELS 16  // internal levels (TLAS + BLAS) up to which a scene takes the SHALLOW instantiations: 48 stack entries instead of 96 + the LDS levels
#endif
#ifndef RT_TOP_NODES
#define RT_TOP_NODES 0      // internal nodes of the top of the tree staged in LDS per workgroup (64 B each); 0 = off
#endif
#define RT_TOP_MAX 1024
static_assert(RT_TOP_NODES <= RT_TOP_MAX, "top-of-tree image");
#ifdef __HIPCC__   // what kind of work a descriptor names (device code of both units)
__device__ __forceinline__ bool is_node_desc(uint32_t d) { return d < 0x80000000u; }
__device__ __forceinline__ bool is_leaf_desc(uint32_t d) { return (d >> 30) == DK_LEAF; }
__device__ __forceinline__ bool is_inst_desc(uint32_t d) { return d >= 0xC0000000u && d < DESC_IDLE; }
__device__ __forceinline__ bool is_work_desc(uint32_t d) { return d < DESC_IDLE; }
#endif
