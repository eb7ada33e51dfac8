// Stand-alone check of the path table's pass (csrc/rt_path_code.h) on the host: two small trees in the compact layout, the level passes run
// node by node as accel_path_kernel runs them thread by thread, then every triangle's code followed from the root -- slot `code & 3`, on
// with `code >> 2` -- until it meets a leaf, which must be the leaf that holds the triangle.  tests/test_shadow_paths_cpu.py builds and
// runs it (with the sanitizers: host code only).
#include <cstdint>
#include <cstdio>
#include <vector>
#include "rt_path_code.h"

struct Tree {
  std::vector<uint32_t> nodes;     // CNODE_DWORDS per internal node
  std::vector<uint32_t> ref_bvh;   // RT_NODE_DWORDS per reference node (only the by-reference leaves' [4], [5] are read)
  uint32_t n_tris = 0;
  uint32_t add_node() { nodes.resize(nodes.size() + CNODE_DWORDS, 0u); for (int k = 0; k < 4; ++k) nodes[nodes.size() - CNODE_DWORDS + CNODE_DESC0 + k] = DESC_NONE; return (uint32_t)(nodes.size() / CNODE_DWORDS) - 1u; }
  uint32_t& child(uint32_t node, uint32_t k) { return nodes[(size_t)node * CNODE_DWORDS + CNODE_DESC0 + k]; }
  uint32_t leaf(uint32_t count) {   // an inline leaf of `count` (1..15) new triangles, or one by reference
    const uint32_t first = n_tris;
    n_tris += count;
    if (count <= LEAF_MAX_INLINE) return DESC(DK_LEAF, (count << LEAF_FIRST_BITS) | first);
    const uint32_t r = (uint32_t)(ref_bvh.size() / RT_NODE_DWORDS);
    ref_bvh.resize(ref_bvh.size() + RT_NODE_DWORDS, 0u);
    ref_bvh[(size_t)r * RT_NODE_DWORDS + 4] = first; ref_bvh[(size_t)r * RT_NODE_DWORDS + 5] = count;
    return DESC(DK_LEAF, r);
  }
};

// a chain of `levels` internal nodes: the chain child sits in slot (level % 4), the other slots hold leaves of varying size, some empty
static Tree chain_tree(uint32_t levels) {
  Tree t;
  uint32_t cur = t.add_node();
  for (uint32_t L = 1; L <= levels; ++L) {
    const uint32_t cs = L % 4u;
    uint32_t next = 0;
    if (L < levels) next = t.add_node();
    for (uint32_t k = 0; k < 4u; ++k) {
      if (k == cs && L < levels) t.child(cur, k) = DESC(DK_BLAS, next);
      else if ((L + k) % 5u == 0u) t.child(cur, k) = DESC_NONE;
      else t.child(cur, k) = t.leaf((L * 7u + k * 3u) % 18u + 1u);   // 1..18 triangles: inline leaves and leaves by reference
    }
    cur = next;
  }
  return t;
}

// a complete 4-ary tree of `levels` internal levels (breadth first: children after their parents), single-triangle and wider leaves below
static Tree full_tree(uint32_t levels) {
  Tree t;
  std::vector<uint32_t> row{t.add_node()};
  for (uint32_t L = 1; L <= levels; ++L) {
    std::vector<uint32_t> nextrow;
    for (uint32_t n : row)
      for (uint32_t k = 0; k < 4u; ++k) {
        if (L < levels) { const uint32_t c = t.add_node(); t.child(n, k) = DESC(DK_BLAS, c); nextrow.push_back(c); }
        else t.child(n, k) = t.leaf(1u + (n + k) % 3u);
      }
    row = nextrow;
  }
  return t;
}

static int check(const char* name, Tree& t, unsigned long& followed) {
  const uint32_t nn = (uint32_t)(t.nodes.size() / CNODE_DWORDS), nb = (uint32_t)(t.ref_bvh.size() / RT_NODE_DWORDS);
  std::vector<uint32_t> lvl(nn, 0u), ncode(nn, 0u), path(t.n_tris, 0xDEADBEEFu);
  lvl[0] = 1u;
  for (uint32_t level = 1; level <= PATH_LEVELS_MAX; ++level)
    for (uint32_t i = 0; i < nn; ++i) path_pass_node(t.nodes.data(), nn, i, level, lvl.data(), ncode.data(), t.ref_bvh.data(), nb, t.n_tris, path.data());
  int bad = 0;
  for (uint32_t tri = 0; tri < t.n_tris; ++tri) {
    uint32_t code = path[tri], d = DESC(DK_BLAS, 0u), steps = 0;
    while (d < 0x80000000u && steps <= PATH_LEVELS_MAX) { d = t.child(d & PAYLOAD_MASK, path_slot(code)); code = path_rest(code); ++steps; }
    bool ok = d != DESC_NONE && (d >> 30) == DK_LEAF && code == 0u;   // (nothing is left of the code at the leaf)
    if (ok) {
      uint32_t first = d & LEAF_FIRST_MASK, count = (d >> LEAF_FIRST_BITS) & LEAF_MAX_INLINE;
      if (count == 0u) { const size_t r = (size_t)first * RT_NODE_DWORDS; first = t.ref_bvh[r + 4]; count = t.ref_bvh[r + 5]; }
      ok = tri >= first && tri < first + count;
    }
    if (!ok) { if (bad < 5) printf("%s: triangle %u: code %08x does not lead to its leaf\n", name, tri, path[tri]); ++bad; }
    ++followed;
  }
  return bad;
}

int main() {
  unsigned long followed = 0;
  Tree a = chain_tree(PATH_LEVELS_MAX), b = full_tree(5);
  const int bad = check("chain", a, followed) + check("full", b, followed);
  printf("%lu triangles followed, %d failures\n", followed, bad);
  return bad ? 1 : 0;
}
