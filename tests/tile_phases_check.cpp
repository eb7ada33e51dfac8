// Stand-alone replay of the fetch / finish policy of the shadow frame kernels that hold the occlusion-only loop (built and run by
// tests/test_tile_phases_cpu.py with g++ -fsanitize=undefined,address): one wavefront walks a queue of 8x8 tiles as rt_persistent_kernel
// does with whole-tile batches (RT_DEAD_MAX 64, RT_SHADOW_FINISH_MIN off) -- fetch hands jobs of ONE tile to idle lanes by rank, the
// traversal loop is left when no lane holds work, finish turns a primary ray that hit into the pixel's occlusion ray and makes every
// other finished lane idle.  The rule under test is the fetch section's own (csrc/rt_tile_refill.h, which the kernel compiles too):
//   parent form (RT_TILE_REFILL_MIN 1):  jobs whenever a lane is idle
//   RT_TILE_PHASES:                      jobs when every lane is idle, or at least RT_TILE_REFILL_MIN (<= 64) lanes are
// Tiles are random: per tile a mask of the lanes that start a primary ray in the main launch (the others: outside the window, on the
// a-priori list), of those that hit, and of the occlusion rays that defer() hands to the EXACT launch (the lane is idle at once).
//
// Shown, per rule: every job is traced once, whatever the rule (which lane traces a job is all that changes); with 65 (no partial refill) no
// pass holds a primary and an any-hit ray, and no job is handed out while a lane holds work; with 32 and 16 a pass is only mixed behind
// a refill of at least that many lanes; the parent's rule does mix them, and a wavefront that is mixed once stays mixed while partial
// tiles keep coming.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "rt_tile_refill.h"

struct Tile { uint64_t start, hit, defer_occ; };

struct Result {
  uint64_t primaries = 0, occlusion = 0;     // rays traced
  uint64_t passes = 0, mixed = 0;            // passes through the traversal loop; those holding both kinds of ray
  uint64_t partial_refills = 0;              // fetches that handed out jobs while a lane held work
  uint32_t min_partial = 65;                 // the fewest idle lanes such a fetch met
  bool mixed_without_partial = false;        // a mixed pass although no partial refill came before it
};


enum Lane : uint8_t { IDLE, PRIMARY, OCC };

static Result replay(const std::vector<Tile>& tiles, uint32_t refill_min) {
  Result r;
  Lane cur[64];
  uint32_t job[64];
  for (int l = 0; l < 64; ++l) { cur[l] = IDLE; job[l] = 0; }
  const uint32_t loc_end = (uint32_t)tiles.size() * 64u;
  uint32_t loc_next = 0;
  bool had_partial = false;
  for (;;) {
    // ---- fetch ----
    uint64_t idle = 0;
    for (int l = 0; l < 64; ++l) if (cur[l] == IDLE) idle |= 1ull << l;
    const bool queue_empty = loc_next == loc_end;
    if (!queue_empty && idle != 0 && tile_refill(idle, refill_min)) {
      if (idle != ~0ull) { ++r.partial_refills; had_partial = true; const uint32_t n = (uint32_t)__builtin_popcountll(idle); if (n < r.min_partial) r.min_partial = n; }
      const uint32_t avail = 64u - (loc_next & 63u);   // lanes draw from ONE tile at a time
      for (int l = 0; l < 64; ++l) {
        if (cur[l] != IDLE) continue;
        const uint32_t rank = (uint32_t)__builtin_popcountll(idle & ((1ull << l) - 1ull));
        if (rank >= avail) continue;
        job[l] = loc_next + rank;
        if ((tiles[job[l] >> 6].start >> (job[l] & 63u)) & 1ull) { cur[l] = PRIMARY; ++r.primaries; }   // (else: start_ray leaves the lane idle)
      }
      const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle);
      loc_next += avail < n_idle ? avail : n_idle;
    }
    bool any = false, prim = false, occ = false;
    for (int l = 0; l < 64; ++l) { any |= cur[l] != IDLE; prim |= cur[l] == PRIMARY; occ |= cur[l] == OCC; }
    if (!any) {
      if (loc_next == loc_end) break;
      continue;
    }
    // ---- traverse: the loop is left when no lane holds work ----
    ++r.passes;
    if (prim && occ) { ++r.mixed; if (!had_partial) r.mixed_without_partial = true; }
    // ---- finish ----
    for (int l = 0; l < 64; ++l) {
      if (cur[l] == PRIMARY) {
        const Tile& t = tiles[job[l] >> 6];
        const uint64_t bit = 1ull << (job[l] & 63u);
        if (t.hit & bit) { ++r.occlusion; cur[l] = (t.defer_occ & bit) ? IDLE : OCC; }   // (a deferred occlusion ray is the EXACT launch's: counted, not traced here)
        else cur[l] = IDLE;
      } else if (cur[l] == OCC) {
        cur[l] = IDLE;
      }
    }
  }
  return r;
}

int main() {
  std::mt19937_64 rng(20251);
  uint64_t cases = 0, failures = 0, parent_mixed_cases = 0, sticky = 0;
  auto fail = [&](const char* what, int kind, size_t n) { ++failures; std::fprintf(stderr, "FAIL %s (kind %d, %zu tiles)\n", what, kind, n); };
  for (int rep = 0; rep < 4000; ++rep) {
    const int kind = rep % 5;
    const size_t n = 1 + rng() % 40;
    std::vector<Tile> tiles(n);
    uint64_t want_prim = 0, want_occ = 0;
    for (size_t i = 0; i < n; ++i) {
      Tile& t = tiles[i];
      const uint64_t a = rng(), b = rng(), c = rng(), d = rng();
      switch (kind) {
        case 0: t.start = ~0ull; t.hit = ~0ull; t.defer_occ = 0; break;                                          // a closed room, no lines
        case 1: t.start = (i % 3 == 0) ? ~(0x0101010101010101ull << (a & 7)) : ~0ull; t.hit = ~0ull; t.defer_occ = 0; break;   // an a-priori column in every third tile
        case 2: t.start = ~0ull; t.hit = a | b; t.defer_occ = 0; break;                                          // background in every tile
        case 3: t.start = (i + 1 == n) ? 0x00000000FFFFFFFFull : ~0ull; t.hit = (i & 1) ? a : ~0ull; t.defer_occ = c & d & a; break;   // some tiles, the window edge, deferred rays
        default: t.start = a | b; t.hit = c; t.defer_occ = d & b & a; break;                                     // everything at once; empty tiles included
      }
      if (rep % 7 == 0 && i % 4 == 1) t.start = 0;       // a tile that starts nothing
      t.hit &= t.start; t.defer_occ &= t.hit;
      want_prim += (uint64_t)__builtin_popcountll(t.start); want_occ += (uint64_t)__builtin_popcountll(t.hit);
    }
    const uint32_t rules[4] = {65u, 32u, 16u, 1u};
    for (uint32_t rule : rules) {
      ++cases;
      const Result r = replay(tiles, rule);
      if (r.primaries != want_prim || r.occlusion != want_occ) fail("every job once", kind, n);
      if (r.mixed_without_partial) fail("a mixed pass without a partial refill", kind, n);
      if (rule == 65u && (r.mixed != 0 || r.partial_refills != 0)) fail("whole-tile phases mix", kind, n);
      if (rule != 65u && r.partial_refills != 0 && r.min_partial < rule) fail("a refill below the threshold", kind, n);
      if (rule == 1u) {
        if (r.mixed != 0) ++parent_mixed_cases;
        // tile 0 leaves lanes idle beside its occlusion rays and tile 1 starts a ray in every lane: those lanes take tile 1's first jobs
        const bool must_mix = n >= 2 && rep % 7 != 0 && ((kind == 1) || (kind == 2 && tiles[0].hit != ~0ull && tiles[0].hit != 0));
        if (must_mix && r.mixed == 0) fail("the parent's rule does not mix behind a partial tile", kind, n);
        if (kind == 0 && r.mixed != 0) fail("the parent's rule mixes full tiles", kind, n);
        // once shifted, shifted for good: a closed room with an a-priori column in tile 0 (kind 1) -- every pass behind the first two
        // holds the rest of one tile beside the first rays of the next
        if (kind == 1 && rep % 7 != 0 && n >= 8) { ++sticky; if (r.mixed + 3 < r.passes) fail("the shift heals", kind, n); }
      }
    }
  }
  // What a threshold of 32 leaves open, on a closed room (ten full tiles) behind ONE tile with background:
  //   exactly 32 lanes idle: refilled, and every later tile then leaves 32 lanes idle at each finish -- mixed to the end, as the parent;
  //   40 lanes idle: refilled; from then on every tile takes THREE passes -- its last 24 rays' occlusion phase beside the next tile's
  //     first 40 primary rays (mixed), those 40 rays' occlusion phase alone (24 lanes idle: below the threshold), then the tile's last 24
  //     primary rays alone (40 lanes idle: refilled again).  It does not heal either, and it runs more passes than the parent's rule;
  //   24 lanes idle: never refilled, never mixed.
  {
    const uint64_t hits[3] = {0x00000000FFFFFFFFull, 0x0000000000FFFFFFull, 0x000000FFFFFFFFFFull};
    for (int k = 0; k < 3; ++k) {
      std::vector<Tile> tiles(11, Tile{~0ull, ~0ull, 0});
      tiles[0].hit = hits[k];
      const Result r32 = replay(tiles, 32u), r65 = replay(tiles, 65u), r1 = replay(tiles, 1u);
      cases += 3;
      if (r65.mixed != 0 || r1.mixed + 3 < r1.passes) fail("one tile with background: 65 / parent", k, tiles.size());
      if (k == 0 && (r32.mixed != r1.mixed || r32.passes != r1.passes)) fail("32 behind a tile of exactly 32 idle lanes is the parent", k, tiles.size());
      if (k == 1 && (r32.mixed != 10 || r32.passes != r65.passes + 10)) fail("32 behind a tile of 40 idle lanes: three passes per later tile, one of them mixed", k, tiles.size());
      if (k == 2 && (r32.mixed != 0 || r32.passes != r65.passes)) fail("32 behind a tile of 24 idle lanes is 65", k, tiles.size());
    }
  }
  std::printf("%llu cases, parent rule mixed %llu, sticky %llu, %llu failures\n", (unsigned long long)cases, (unsigned long long)parent_mixed_cases,
              (unsigned long long)sticky, (unsigned long long)failures);
  return failures ? 1 : 0;
}
