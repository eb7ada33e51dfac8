// The integer arithmetic of a launch's grid: a persistent grid capped by need (persistent_grid) and the main launch of a frame
// (launch_plan, main_grid: the side launch's reserve, the share of the machine with several frames in flight).  What the device
// holds of a kernel -- occupancy x CUs -- comes in as a number; everything here is a pure function of it, the job counts, the knob
// values and the number of frame contexts.
// Compiled by hipcc into rt_kernels.hip and by plain g++ into the stand-alone program of tests/test_launch_plan_cpu.py, which sweeps
// it and holds the default plan to a literal restatement of the expressions it replaced.
#pragma once
#include <stdint.h>

// VXRT_GRID_MAX=n (n >= 1; 0 or less = none): a measurement knob, no persistent launch takes more than n workgroups
inline uint64_t plan_grid_max(uint64_t g, int grid_max) {
  return (grid_max >= 1 && g > (uint64_t)grid_max) ? (uint64_t)grid_max : g;
}

// grid of a persistent launch: `held` = what the device holds of the kernel at once, capped by the workgroups `jobs` jobs need
inline uint32_t plan_persistent_grid(uint64_t held, uint64_t jobs, uint32_t wg_threads, int grid_max) {
  uint64_t g = held;
  const uint64_t need = (jobs + (uint64_t)wg_threads - 1) / (uint64_t)wg_threads;
  if (g > need) g = need;
  g = plan_grid_max(g, grid_max);
  return (uint32_t)(g ? g : 1);
}

// VXRT_SIDE_RESERVE (-1 = unset): the main launch leaves the side launch's workgroups free on a serial frame (one context)
inline bool plan_side_reserve(int knob, uint32_t n_ctx) { return knob >= 0 ? knob != 0 : n_ctx == 1; }
// VXRT_GRID_DIV (0 = unset): the divisor of the main launch's share; unset, the frames in flight; negative, none
inline uint32_t plan_grid_div(int knob, uint32_t n_ctx) { return knob > 0 ? (uint32_t)knob : ((knob == 0 && n_ctx > 1) ? n_ctx : 1u); }
// ... which, unset, only holds for a window that is small against the machine (plan_main_grid)
inline bool plan_grid_div_small(int knob) { return knob == 0; }

// grid of a frame's main launch: what the machine holds of the kernel, less the slots reserved for the side launch, divided as the
// plan says.  `total` = jobs of the launch, `side_wgs` = workgroups of the side launch (0: none), wg_waves = wavefronts per workgroup.
inline uint32_t plan_main_grid(uint64_t held, uint32_t total, uint32_t side_wgs, bool side_reserve, uint32_t grid_div, bool grid_div_small,
                               uint32_t wg_waves, int grid_max) {
  const uint32_t wg_threads = 64u * wg_waves;
  const uint32_t side_wgs_r = side_reserve ? side_wgs : 0u;
  uint32_t g = plan_persistent_grid(held, total + (uint64_t)side_wgs_r * wg_threads, wg_threads, grid_max);
  const uint32_t cap = plan_persistent_grid(held, ~0ull >> 8, wg_threads, grid_max);
  const uint32_t div = (grid_div_small && (uint64_t)total >= 2ull * 64ull * wg_waves * cap) ? 1u : grid_div;
  if (div > 1u) { const uint32_t share = cap / div > 1u ? cap / div : 1u; if (g > share) g = share; }
  return g > side_wgs_r ? g - side_wgs_r : 1u;
}
