// The reference's pinhole camera (raycast/render.h:192-211 GenerateRay; the commented-out GenerateRay of the RTU test's kernel.cpp:11-25
// reads the same kernel_arg_t fields), shared by the software twin (rc_kernels.hip) and the RTU frame path's camera frames
// (rt_kernels.hip).  Operation for operation, under -ffp-contract=off:
//   x_ndc = (float)((double)(((float)x + 0.5f) / (float)W) - 0.5)      (likewise y_ndc with y, H)
//   x_vp = x_ndc * viewplane[0], y_vp = y_ndc * viewplane[1]
//   pt_cam = (x_vp * right + y_vp * up) + forward, pt_w = pt_cam + pos, d = pt_w - pos   (add, then subtract: not shortened)
//   d *= 1 / sqrtf(dot(d, d)); origin = pos
// x_vp depends on the column only and y_vp on the row only, so the RTU path keeps them in per-frame tables (as utab / vtab are for the
// fixed camera) and runs only pinhole_dir per ray.
#pragma once
#include <stdint.h>

__host__ __device__ __forceinline__ float pinhole_ndc(uint32_t i, uint32_t n) {
  return (float)((double)(((float)i + 0.5f) / (float)n) - 0.5);
}

// direction of the ray through the view-plane point (x_vp, y_vp) of camera (pos, fwd, right, up); the origin is pos
__device__ __forceinline__ void pinhole_dir(float x_vp, float y_vp, const float* pos, const float* fwd, const float* right, const float* up,
                                            float& dx, float& dy, float& dz) {
  const float cx = x_vp * right[0] + y_vp * up[0] + fwd[0];
  const float cy = x_vp * right[1] + y_vp * up[1] + fwd[1];
  const float cz = x_vp * right[2] + y_vp * up[2] + fwd[2];
  const float wx = cx + pos[0], wy = cy + pos[1], wz = cz + pos[2];
  const float vx = wx - pos[0], vy = wy - pos[1], vz = wz - pos[2];
  const float inv = 1.0f / sqrtf(vx * vx + vy * vy + vz * vz);
  dx = vx * inv; dy = vy * inv; dz = vz * inv;
}
