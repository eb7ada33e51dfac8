// The fetch rule of the shadow frame kernels that hold the occlusion-only loop (RT_TILE_PHASES, RT_TILE_REFILL_MIN: rt_kernels.hip): does
// a wavefront whose idle lanes are `idle` take new jobs.  Compiled by hipcc into rt_persistent_kernel's fetch section and by plain g++
// into the stand-alone program of tests/test_tile_phases_cpu.py, which replays the fetch / finish policy around it on random tiles.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_TILE_REFILL_FN __host__ __device__ __forceinline__
#else
#define RT_TILE_REFILL_FN inline
#endif

// every lane is idle, or at least refill_min (<= 64; 65 = never, 1 = whenever a lane is idle) of them are
RT_TILE_REFILL_FN bool tile_refill(unsigned long long idle, uint32_t refill_min) {
  return idle == ~0ull || (refill_min <= 64u && (uint32_t)__builtin_popcountll(idle) >= refill_min);
}
