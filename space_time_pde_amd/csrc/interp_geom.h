// Geometry of one multilinear-interpolation query, shared by the plain interpolation kernels (interp_nd.hip) and the batch
// sampler (sampler.hip), which must agree with them bit for bit: clip, cell index, corner weights and relative coordinates
// with the reference's own fp32 expression sequence (src/regular_nd_grid_interpolation.py:40-62).
#pragma once
#include "common.h"

struct GeomN {
  float om[2][4], rl[2][4];
  int i0[4];
};

// axis k of a query at coordinate x: box [lo, hi] (already shrunk by 1e-6 of its size), cell size cs, n nodes
__device__ __forceinline__ void geom_axis(GeomN& gm, int k, float x, float lo, float hi, float cs, int n) {
  const float q = fmaxf(fminf(x, hi), lo);
  int i0 = (int)floorf(q / cs);
  i0 = i0 < 0 ? 0 : (i0 > n - 2 ? n - 2 : i0);
  const float i0f = (float)i0;
  const float p0 = i0f * cs, p1 = (i0f + 1.f) * cs;
  gm.i0[k] = i0;
  gm.om[0][k] = fabsf(q - p1) / cs;
  gm.om[1][k] = fabsf(q - p0) / cs;
  gm.rl[0][k] = (q - p0) / cs;
  gm.rl[1][k] = (q - p1) / cs;
}

// bit of axis k in corner j of a dim-dimensional cell: the first axis is the most significant (:55-56)
__device__ __forceinline__ int corner_bit(int j, int dim, int k) { return (j >> (dim - 1 - k)) & 1; }

// weight of corner j: the product of the per-axis weights in axis order
__device__ __forceinline__ float corner_weight(const GeomN& gm, int j, int dim) {
  float w = 1.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < dim) {
      const float o = corner_bit(j, dim, k) ? gm.om[1][k] : gm.om[0][k];
      w = (k == 0) ? o : w * o;
    }
  }
  return w;
}
