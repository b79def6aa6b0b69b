// Geometry of one multilinear-interpolation query, shared by the plain interpolation kernels (interp_nd.hip), the batch
// sampler (sampler.hip) and the local-implicit-grid gathers (lig_gather_reduce.hip), which must agree with each other bit for
// bit: clip, cell index, corner weights and relative coordinates with the reference's own fp32 expression sequence
// (src/regular_nd_grid_interpolation.py:40-62), and on top of them what the dim = 3 derivative streams need.  This header is
// the only place where any of it is written; a caller that uses part of a struct leaves the rest to dead-code elimination.
#pragma once
#include "common.h"

struct GeomN {
  float om[2][4], rl[2][4];
  int i0[4];
};

// axis k of a query at coordinate x: box [lo, hi] (already shrunk by 1e-6 of its size), cell size cs, n nodes.
// Returns the clipped coordinate.  The cell index is clamped to [0, n - 2]: only NaN / out-of-box inputs ever hit the clamp.
__device__ __forceinline__ float geom_axis(GeomN& gm, int k, float x, float lo, float hi, float cs, int n) {
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
  return q;
}

// GeomN plus the first-order jets of the weights and relative coordinates with respect to the query coordinate:
// dom[b][k] = d om[b][k] / dx (sign * s / cs) and kap[k] = d rl[b][k] / dx (s / cs), s = derivative of the clip
struct GeomJet : GeomN {
  float dom[2][4], kap[4];
};

__device__ __forceinline__ void geom_axis_jet(GeomJet& gj, int k, float x, float lo, float hi, float cs, int n) {
  const float q = geom_axis(gj, k, x, lo, hi, cs, n);
  // derivative of the clip: min/max backward split ties evenly (quirk a-Q2)
  const float m = fminf(x, hi);
  const float s = (x < hi ? 1.f : (x == hi ? 0.5f : 0.f)) * (m > lo ? 1.f : (m == lo ? 0.5f : 0.f));
  const float i0f = (float)gj.i0[k];
  const float t0 = q - (i0f + 1.f) * cs, t1 = q - i0f * cs;   // signed distance to the position opposite to bit 0 / bit 1
  gj.kap[k] = s / cs;
  gj.dom[0][k] = (t0 > 0.f ? 1.f : (t0 < 0.f ? -1.f : 0.f)) / cs * s;
  gj.dom[1][k] = (t1 > 0.f ? 1.f : (t1 < 0.f ? -1.f : 0.f)) / cs * s;
}

// bit of axis k in corner j of a dim-dimensional cell: the first axis is the most significant (:55-56)
__device__ __forceinline__ int corner_bit(int j, int dim, int k) { return (j >> (dim - 1 - k)) & 1; }

// weight of corner j: the product of the per-axis weights in axis order
__device__ __forceinline__ float corner_weight(const GeomN& gm, int j, int dim) {
  float w = 1.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < dim) {
      const float o0 = gm.om[0][k], o1 = gm.om[1][k];   // both read, then selected: a select of addresses would cost scratch
      const float o = corner_bit(j, dim, k) ? o1 : o0;
      w = (k == 0) ? o : w * o;
    }
  }
  return w;
}
