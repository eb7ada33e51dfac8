// Stand-alone check of csrc/rt_launch_plan.h (built and run by tests/test_launch_plan_cpu.py with g++ -fsanitize=undefined,address): the
// integer arithmetic of a persistent launch's grid and of a frame's main launch, swept over
//   what the device holds (occupancy x CUs)   1, 2, 3, 4, 31, 32, 128, 1792, 2048
//   workgroups of the side launch             0 .. 128 (EXACT_GRID)
//   jobs of the launch                        1, 64, 65, 2*64*4*cap - 1, 2*64*4*cap, 2*64*4*cap + 1 (the "small window" edge), 2^32 - 1
//   VXRT_GRID_DIV                             -1, 0, 1, 3, cap, cap + 1, 10^6
//   VXRT_SIDE_RESERVE                         -1 (unset), 0, 1
//   frame contexts                            1, 3
//   VXRT_GRID_MAX                             0 (none), 1, 2
// On every case: 1 <= grid <= max(1, cap); grid <= the workgroups the jobs need; grid <= n under VXRT_GRID_MAX=n; the value equals the
// same plan computed in 64-bit signed arithmetic (no unsigned wrap); and with no VXRT_GRID_MAX it equals the expressions launch_plan,
// main_grid and persistent_grid held before they moved into the header, restated literally below.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include "rt_launch_plan.h"

#define RT_WG_WAVES 4
#define RT_WG_THREADS (64 * RT_WG_WAVES)

// ---- the expressions as they stood in rt_kernels.hip (the occupancy query replaced by its result) ----
static uint32_t old_persistent_grid(uint64_t g, uint64_t jobs, int wg_threads = RT_WG_THREADS) {
  const uint64_t need = (jobs + (uint64_t)wg_threads - 1) / (uint64_t)wg_threads;
  if (g > need) g = need;
  return (uint32_t)(g ? g : 1);
}
struct OldPlan { uint32_t side_wgs; bool side_reserve; uint32_t grid_div; bool grid_div_small; };
struct OldKnobs { int side_reserve, grid_div; };
static OldPlan old_launch_plan(const OldKnobs& k, uint32_t n_ctx, uint32_t side_wgs) {
  OldPlan plan;
  plan.side_wgs = side_wgs;
  plan.side_reserve = k.side_reserve >= 0 ? k.side_reserve != 0 : n_ctx == 1;
  plan.grid_div = k.grid_div > 0 ? (uint32_t)k.grid_div : ((k.grid_div == 0 && n_ctx > 1) ? n_ctx : 1u);
  plan.grid_div_small = k.grid_div == 0;
  return plan;
}
static uint32_t old_main_grid(uint64_t held, const OldPlan& plan, uint32_t total) {
  const uint32_t side_wgs_r = plan.side_reserve ? plan.side_wgs : 0u;
  uint32_t g = old_persistent_grid(held, total + (uint64_t)side_wgs_r * RT_WG_THREADS);
  const uint32_t cap = old_persistent_grid(held, ~0ull >> 8);
  const uint32_t div = (plan.grid_div_small && (uint64_t)total >= 2ull * 64ull * RT_WG_WAVES * cap) ? 1u : plan.grid_div;
  if (div > 1u) g = std::min<uint32_t>(g, std::max<uint32_t>(cap / div, 1u));
  return std::max<uint32_t>(1u, g > side_wgs_r ? g - side_wgs_r : 1u);
}

// ---- the plan in 64-bit signed arithmetic, where nothing here can wrap ----
static int64_t wide_grid(int64_t held, int64_t jobs, int64_t wg_threads, int64_t grid_max) {
  int64_t g = std::min(held, (jobs + wg_threads - 1) / wg_threads);
  if (grid_max >= 1) g = std::min(g, grid_max);
  return std::max<int64_t>(g, 1);
}
static int64_t wide_main_grid(int64_t held, int64_t total, int64_t side_wgs, int side_reserve, int grid_div, int64_t n_ctx, int64_t grid_max) {
  const int64_t side = (side_reserve >= 0 ? side_reserve != 0 : n_ctx == 1) ? side_wgs : 0;
  int64_t g = wide_grid(held, total + side * RT_WG_THREADS, RT_WG_THREADS, grid_max);
  const int64_t cap = wide_grid(held, INT64_C(1) << 56, RT_WG_THREADS, grid_max);
  int64_t div = grid_div > 0 ? grid_div : ((grid_div == 0 && n_ctx > 1) ? n_ctx : 1);
  if (grid_div == 0 && total >= 2 * 64 * RT_WG_WAVES * cap) div = 1;
  if (div > 1) g = std::min(g, std::max<int64_t>(cap / div, 1));
  return std::max<int64_t>(1, g - side);
}

static long failures = 0;
static void fail(const char* what, uint64_t cap, uint32_t side, uint32_t total, int div, int reserve, uint32_t n_ctx, int grid_max, uint32_t got, uint64_t want) {
  if (failures++ < 20)
    std::printf("FAIL %s: cap %llu side %u total %u grid_div %d side_reserve %d n_ctx %u grid_max %d: grid %u, expected %llu\n", what,
                (unsigned long long)cap, side, total, div, reserve, n_ctx, grid_max, got, (unsigned long long)want);
}

int main() {
  const uint64_t caps[] = {1, 2, 3, 4, 31, 32, 128, 1792, 2048};
  long plans = 0, grids = 0;
  for (uint64_t cap : caps) {
    const uint64_t edge = 2ull * 64ull * RT_WG_WAVES * cap;
    const uint32_t totals[] = {1u, 64u, 65u, (uint32_t)(edge - 1), (uint32_t)edge, (uint32_t)(edge + 1), 0xFFFFFFFFu};
    const int divs[] = {-1, 0, 1, 3, (int)cap, (int)cap + 1, 1000000};
    for (uint32_t total : totals) {
      const uint64_t need = ((uint64_t)total + RT_WG_THREADS - 1) / RT_WG_THREADS;
      // a persistent launch of its own (ray buffers, the experiments' 64- and 256-thread kernels)
      for (int grid_max : {0, 1, 2})
        for (uint32_t wg : {64u, 256u}) {
          ++grids;
          const uint32_t g = plan_persistent_grid(cap, total, wg, grid_max);
          const uint64_t need_wg = ((uint64_t)total + wg - 1) / wg;
          if (g < 1u || g > std::max<uint64_t>(1, cap) || g > need_wg) fail("grid bounds", cap, 0, total, 0, 0, 0, grid_max, g, need_wg);
          if (grid_max >= 1 && g > (uint32_t)grid_max) fail("grid max", cap, 0, total, 0, 0, 0, grid_max, g, (uint64_t)grid_max);
          if ((int64_t)g != wide_grid((int64_t)cap, total, wg, grid_max)) fail("grid wide", cap, 0, total, 0, 0, 0, grid_max, g, (uint64_t)wide_grid((int64_t)cap, total, wg, grid_max));
          if (grid_max == 0 && g != old_persistent_grid(cap, total, (int)wg)) fail("grid moved", cap, 0, total, 0, 0, 0, grid_max, g, old_persistent_grid(cap, total, (int)wg));
        }
      for (uint32_t side = 0; side <= 128u; ++side)
        for (int div : divs)
          for (int reserve : {-1, 0, 1})
            for (uint32_t n_ctx : {1u, 3u})
              for (int grid_max : {0, 1, 2}) {
                ++plans;
                const uint32_t g = plan_main_grid(cap, total, side, plan_side_reserve(reserve, n_ctx), plan_grid_div(div, n_ctx), plan_grid_div_small(div),
                                                  RT_WG_WAVES, grid_max);
                if (g < 1u || g > std::max<uint64_t>(1, cap)) fail("bounds", cap, side, total, div, reserve, n_ctx, grid_max, g, cap);
                if (g > need) fail("need", cap, side, total, div, reserve, n_ctx, grid_max, g, need);
                if (grid_max >= 1 && g > (uint32_t)grid_max) fail("max", cap, side, total, div, reserve, n_ctx, grid_max, g, (uint64_t)grid_max);
                const int64_t wide = wide_main_grid((int64_t)cap, total, side, reserve, div, n_ctx, grid_max);
                if ((int64_t)g != wide) fail("wide", cap, side, total, div, reserve, n_ctx, grid_max, g, (uint64_t)wide);
                if (grid_max == 0) {
                  const uint32_t old = old_main_grid(cap, old_launch_plan(OldKnobs{reserve, div}, n_ctx, side), total);
                  if (g != old) fail("moved", cap, side, total, div, reserve, n_ctx, grid_max, g, old);
                }
              }
    }
  }
  std::printf("%ld plan cases, %ld grid cases, %ld failures\n", plans, grids, failures);
  return failures ? 1 : 0;
}
