// Local-implicit-grid glue kernels around the IM-NET layer kernels, for grids of dim = 1, 2, 3, 4.  One set of templated
// device bodies serves every dimension; dim = 3 (the PDE path, with derivative streams) adds a per-point epilogue:
//   gather_row<D> / row_feature<D>   clip + cell index + corner gather + relative coordinates -> augmented MLP input X
//                 (fragment layout)   (src/regular_nd_grid_interpolation.py:48-76, src/local_implicit_grid.py:49)
//                 k_gather_nd<D>      D = 1, 2, 4: X and the corner weight of every row (roww)
//                 k_gather            D = 3: X, the optional row-major image XR, and write_coef()
//                 k_gather_tile       D = 3, 32 latent channels: the same rows through an LDS patch, 16-byte loads / stores
//   write_coef    dim = 3 epilogue: per-point interpolation coefficients, cell id, combined-stream weights
//   point_cell<D> the cell of a point: what the gathers read, what k_cell_nd<D> and write_coef() report
//   dlat_reduce<D>  per-node d-latent sum in a fixed order: k_dlat_reduce (D = 3), k_dlat_reduce_nd<D> (D = 1, 2, 4)
//   k_reduce_fwd / k_reduce_bwd       dim = 3: corner-weighted sum of the MLP output on every derivative stream
//                 (src/local_implicit_grid.py:59 and what the src/pde.py:8-9 sweeps differentiate through) and its adjoint
//   k_reduce_nd / k_reduce_nd_bwd     D = 1, 2, 4: the value-only corner sum and its adjoint
//   k_coef_nd<D> / k_reduce_nd_jet<D> D = 1, 2, forward only: the dim = 3 coefficient record per point and the corner sum of
//                 every derivative stream over the 16 >> D points-per-tile rows
//   k_coef_nd4 / k_reduce_nd4_jet     D = 4, forward only: the record of all four axes per point and the corner sum of one
//                 PASS -- the (3, S2) layer sequence over one axis triple -- into the streams its destination map names
//   k_xbar        d latent: xbar = sum_l W_s,l^T abar_l, scatter-added at the corner nodes or written per row (backward of the
//                 advanced-index gather at src/regular_nd_grid_interpolation.py:65-66); dimension-agnostic
// The geometry itself (clip, cell index, weights, relative coordinates, their jets) is written in interp_geom.h only.
// All of these are HBM/L2-bound byte movers; no MFMA except the small xbar GEMM.
#include "interp_geom.h"

// ---------------------------------------------------------------------------------------------------------
// argument checks shared by the entry points
// ---------------------------------------------------------------------------------------------------------
// every axis holds a cell and a node index (batch included) fits an int32; *nodes = B * prod(n).  int32_nodes = false leaves the
// second condition out (stpde_lig_dlatent_reduce never had it, and which calls an entry point refuses is part of the ABI)
static int check_grid(const char* who, int D, int B, const int* n, size_t* nodes, bool int32_nodes = true) {
  unsigned long long cnt = (unsigned long long)B;
  for (int k = 0; k < D; ++k) {
    if (n[k] < 2) {
      stpde_set_error("%s: grid axis %d has %d nodes (>= 2 per axis)", who, k, n[k]);
      return STPDE_E_BADARG;
    }
    cnt *= (unsigned long long)n[k];
    if (int32_nodes && cnt >= (1ull << 31)) {
      stpde_set_error("%s: latent grid too large for an int32 node index", who);
      return STPDE_E_BADARG;
    }
  }
  *nodes = (size_t)cnt;
  return STPDE_OK;
}

// the features [r(D); latent(C); 1] fit the augmented input: two full tiles and register 0 of the sparse third one
static int check_features(const char* who, int D, int C) {
  if (C < 1 || D + C + 1 > 16 * (XT - 1) + 4) {
    stpde_set_error("%s: D + C + 1 = %d features do not fit the augmented input (<= %d)", who, D + C + 1, 16 * (XT - 1) + 4);
    return STPDE_E_BADARG;
  }
  return STPDE_OK;
}

// ---------------------------------------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------------------------------------
// A row tile holds 16 >> D points; row j of a tile = corner (j & (2^D - 1)) of point tile * (16 >> D) + (j >> D), corners in
// the order of interp_nd.hip (first axis most significant).  Feature f of the augmented input [r(D); latent(C); 1] sits in
// slot f of tiles 0 / 1 and in register 0 of the sparse third tile (x_live()).
//
// Addresses, for D = 1, 2, 3, 4 alike.  Every index below is bounded for EVERY input value, not only for points inside the box
// (tests/lig_nd_model.py restates the bodies; tests/test_lig_nd_host.py runs them on NaN, infinite and huge coordinates):
//   pts     p < P (rows of p >= P are padding: zeros, weight 0, no read; dim = 3 has none: P is even, ntiles = P / 2), k < D
//   latent  batch clamped to B - 1, cell index clamped to [0, n_k - 2] by geom_axis() after the float clip (NaN and huge
//           coordinates end there), corner bit 0 / 1, channel f - D < C: node < B * prod(n), all in 64-bit
//   X, XR   gid < ntiles * XT * 64 (the grid is derived from ntiles alone), one float4 per thread
//   roww    tile * 16 + j < ntiles * 16
//   coef, cell, cw   p < P: one lane per point (corner 0 of the first input tile)
struct GatherArgs {
  stpde_gather_nd_desc d;   // dim = 3: the fields of stpde_gather_desc, ntiles = P / 2
  const float* pts;
  const float* latent;
  float* X;
  float* roww;              // D = 1, 2, 4: corner weight of every row
  float* XR;                // dim = 3 from here on
  float* coef;
  int* cell;
  float* cw;
  float alpha[6];
};

// Geometry of point p of the chunk and its cell = the linear index of the cell's corner-0 node, batch included.  The one place
// that says which cell a point lies in: the gathers read the corners of this cell, k_cell_nd and write_coef() report it.
template <int D>
__device__ __forceinline__ size_t point_cell(const stpde_gather_nd_desc& d, const float* pts, size_t p, GeomJet& gj) {
#pragma unroll
  for (int k = 0; k < D; ++k) geom_axis_jet(gj, k, pts[p * D + k], d.lo_c[k], d.hi_c[k], d.cube[k], d.n[k]);
  unsigned b = ((unsigned)d.p_base + (unsigned)p) / (unsigned)d.N;   // (fits: two non-negative ints)
  b = b > (unsigned)(d.B - 1) ? (unsigned)(d.B - 1) : b;
  size_t node = b;
#pragma unroll
  for (int k = 0; k < D; ++k) node = node * (size_t)d.n[k] + (size_t)gj.i0[k];
  return node;
}

struct GatherRow {
  size_t p, cell, node;   // point of the chunk, its cell, the grid node of this row's corner
  int corner;
  float w;                // corner weight
  GeomJet gj;
};

// row j of row tile `tile`; false for a padding row (p >= P), of which nothing else is set
template <int D>
__device__ __forceinline__ bool gather_row(const GatherArgs& a, size_t tile, int j, GatherRow& r) {
  constexpr int TP = 16 >> D, NC = 1 << D;
  r.p = tile * TP + (j >> D);
  r.corner = j & (NC - 1);
  if (r.p >= (size_t)a.d.P) return false;
  r.cell = point_cell<D>(a.d, a.pts, r.p, r.gj);
  size_t off = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) off = off * (size_t)a.d.n[k] + (size_t)corner_bit(r.corner, D, k);
  r.node = r.cell + off;
  r.w = corner_weight(r.gj, r.corner, D);
  return true;
}

// relative coordinate of the row's corner along axis k = feature k of the augmented input row
template <int D>
__device__ __forceinline__ float row_rel(const GatherRow& r, int k) {
  float val = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (k == d) val = corner_bit(r.corner, D, d) ? r.gj.rl[1][d] : r.gj.rl[0][d];
  return val;
}

// feature f >= D of the augmented input row: latent channels of the corner node, the bias column, zeros
template <int D>
__device__ __forceinline__ float row_feature(const GatherArgs& a, const GatherRow& r, int f) {
  const int C = a.d.C;
  if (f < D + C) return a.latent[r.node * (size_t)C + (size_t)(f - D)];
  return f == D + C ? 1.f : 0.f;  // bias column
}

// dim = 3, one lane per point: coef[p][16] = {om[b][d] (6), dom[b][d] (6), kap[d] (3), 0}, cell[p], and the weights of the
// combined second-order stream cw[p][8] = alpha_k * kappa_a * kappa_b over the canonical pairs
__device__ __forceinline__ void write_coef(const GatherArgs& a, const GatherRow& r) {
  const GeomJet& gj = r.gj;
  float* cf = a.coef + r.p * 16;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    cf[d] = gj.om[0][d];
    cf[3 + d] = gj.om[1][d];
    cf[6 + d] = gj.dom[0][d];
    cf[9 + d] = gj.dom[1][d];
    cf[12 + d] = gj.kap[d];
  }
  cf[15] = 0.f;
  a.cell[r.p] = (int)r.cell;
  if (a.cw) {
    float* cwp = a.cw + r.p * 8;
    const float k0 = gj.kap[0], k1 = gj.kap[1], k2 = gj.kap[2];
    cwp[0] = a.alpha[0] * k0 * k0;
    cwp[1] = a.alpha[1] * k0 * k1;
    cwp[2] = a.alpha[2] * k0 * k2;
    cwp[3] = a.alpha[3] * k1 * k1;
    cwp[4] = a.alpha[4] * k1 * k2;
    cwp[5] = a.alpha[5] * k2 * k2;
    cwp[6] = 0.f;
    cwp[7] = 0.f;
  }
}

// one thread per (tile, xt, lane): writes one float4 of X.  A lane evaluates only what ITS slot needs: the divisions of the cell
// index always, the relative coordinates only in the 16 lanes that hold them (tile 0, lane group 0: features 0 .. D - 1 <= 3),
// the weights and their jets only where roww / the coefficients are written (each use sits in one branch, and the compiler
// sinks the unused rest of geom_axis_jet() into it).  The kernel is bound by its stores, not by the divisions.
template <int D>
__device__ __forceinline__ void gather_rows(const GatherArgs& a) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.d.ntiles * XT * 64) return;
  const int lane = gid & 63;
  const int xt = (gid >> 6) % XT;
  const size_t tile = (gid >> 6) / XT;
  const int g = lane >> 4, j = lane & 15;
  const bool head = xt == 0 && g == 0;
  GatherRow row;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  float w = 0.f;
  if (gather_row<D>(a, tile, j, row)) {
    if (head) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = r < D ? row_rel<D>(row, r) : row_feature<D>(a, row, r);
      if (D != 3)
        w = row.w;
      else if (row.corner == 0)
        write_coef(a, row);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)  // slot (xt, g, r): tiles 0 / 1 in feature order, tile 2 sparse (register 0 only: features 32 + g)
        v[r] = row_feature<D>(a, row, xt < XT - 1 ? 16 * xt + 4 * g + r : (r == 0 ? 16 * xt + g : 16 * XT));
    }
  }
  st4(a.X + gid * 4, v);
  if (D == 3) {
    if (a.XR) st_R(a.XR + (gid >> 6) * 256, lane, v);
  } else if (head)
    a.roww[tile * 16 + j] = w;
}

template <int D>
__global__ __launch_bounds__(256) void k_gather_nd(GatherArgs a) {
  gather_rows<D>(a);
}

__global__ __launch_bounds__(256) void k_gather(GatherArgs a) { gather_rows<3>(a); }

// dim = 3 with the reference's 32 latent channels, one WAVE per row tile (round 3): a lane (g, j) fetches channels
// 8g .. 8g+7 of the grid node of corner row j as two aligned 16-byte loads (k_gather: four dword loads per lane, unaligned by
// the three coordinate features in front of the channels), the 16 x 36 feature rows of the tile go through an LDS patch, and
// BOTH fragment images of the three input tiles leave as coalesced 16-byte stores (k_gather's row-major image is four strided
// dword stores per lane).  The rows and the epilogue are the shared ones.
__global__ __launch_bounds__(256) void k_gather_tile(GatherArgs a) {
  constexpr int RS = 36;                       // floats per row: features 0..35 = rel(3), 32 channels, the ones column
  __shared__ __attribute__((aligned(16))) float rows[4][16 * RS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tile = blockIdx.x * 4 + wv;
  const bool live = tile < a.d.ntiles;
  const int g = lane >> 4, j = lane & 15;
  float* rw = rows[wv];
  GatherRow row;
  if (live && gather_row<3>(a, tile, j, row)) {
    const f32x4 c0 = ld4(a.latent + row.node * 32 + 8 * g), c1 = ld4(a.latent + row.node * 32 + 8 * g + 4);
    float* rj = rw + j * RS;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      rj[3 + 8 * g + k] = c0[k];
      rj[3 + 8 * g + 4 + k] = c1[k];
    }
    if (g == 0) {
#pragma unroll
      for (int f = 0; f < 3; ++f) rj[f] = row_rel<3>(row, f);
      rj[35] = 1.f;                            // bias column
      if (row.corner == 0) write_coef(a, row);
    }
  }
  __syncthreads();
  if (!live) return;
  float* xo = a.X + (size_t)tile * XT * 256 + lane * 4;
  // column-major images: lane (g, j) = features 4g..4g+3 of row j; tile 2 is sparse (register 0: feature 32 + g)
  st4(xo, ld4(rw + j * RS + 4 * g));
  st4(xo + 256, ld4(rw + j * RS + 16 + 4 * g));
  st4(xo + 512, f32x4{rw[j * RS + 32 + g], 0.f, 0.f, 0.f});
  if (a.XR) {
    // row-major images: lane (g, c) = rows 4g..4g+3 of slot c
    float* ro = a.XR + (size_t)tile * XT * 256 + lane * 4;
    const float* r0 = rw + 4 * g * RS;
    st4(ro, f32x4{r0[j], r0[RS + j], r0[2 * RS + j], r0[3 * RS + j]});
    st4(ro + 256, f32x4{r0[16 + j], r0[RS + 16 + j], r0[2 * RS + 16 + j], r0[3 * RS + 16 + j]});
    const int fs = 32 + (j >> 2);
    const bool has = (j & 3) == 0;
    st4(ro + 512, has ? f32x4{r0[fs], r0[RS + fs], r0[2 * RS + fs], r0[3 * RS + fs]} : f32x4{0.f, 0.f, 0.f, 0.f});
  }
}

extern "C" int stpde_lig_gather(const stpde_gather_desc* d, const float* pts, const float* latent, float* X,
                                float* XR, float* coef, int* cell, float* cw, void* stream) {
  if (!d || d->P <= 0 || (d->P & 1) || d->N <= 0 || d->p_base < 0 || d->B <= 0 || !pts || !latent || !X || !coef || !cell) {
    stpde_set_error("lig_gather: bad argument (P even)");
    return STPDE_E_BADARG;
  }
  GatherArgs a{};
  a.d.D = 3, a.d.P = d->P, a.d.N = d->N, a.d.B = d->B, a.d.C = d->C, a.d.p_base = d->p_base, a.d.ntiles = d->P / 2;
  a.d.n[0] = d->n0, a.d.n[1] = d->n1, a.d.n[2] = d->n2;
  for (int k = 0; k < 3; ++k) a.d.lo_c[k] = d->lo_c[k], a.d.hi_c[k] = d->hi_c[k], a.d.cube[k] = d->cube[k];
  for (int k = 0; k < 6; ++k) a.alpha[k] = d->alpha[k];
  size_t nodes;
  int rc = check_features("lig_gather", 3, d->C);
  if (!rc) rc = check_grid("lig_gather", 3, d->B, a.d.n, &nodes);
  if (rc) return rc;
  a.pts = pts, a.latent = latent, a.X = X, a.XR = XR, a.coef = coef, a.cell = cell, a.cw = cw;
  if (d->C == 32) {       // the reference's latent width: one wave per row tile, 16-byte loads and stores
    STPDE_LAUNCH(k_gather_tile, dim3((unsigned)((a.d.ntiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return stpde_check_launch("k_gather_tile");
  }
  const size_t nthreads = (size_t)a.d.ntiles * XT * 64;
  STPDE_LAUNCH(k_gather, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_gather");
}

template <int D>
static int launch_gather_nd(const GatherArgs& a, hipStream_t stream) {
  const size_t nthreads = (size_t)a.d.ntiles * XT * 64;
  STPDE_LAUNCH(k_gather_nd<D>, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_gather_nd");
}

// D, P against ntiles, and the 32-bit limits shared by the n-D entry points
static int check_nd(const char* who, int D, int P, int ntiles) {
  if (D != 1 && D != 2 && D != 4) {
    stpde_set_error("%s: D = %d (1, 2 or 4; dim = 3 has stpde_lig_gather / stpde_lig_reduce_fwd)", who, D);
    return STPDE_E_BADARG;
  }
  const long TP = 16 >> D;
  if (P < 1 || ntiles < 1 || (long)ntiles * TP < (long)P || (long)ntiles > ((long)P + TP - 1) / TP + 3 ||
      (long)ntiles * 16 >= (1L << 31)) {
    stpde_set_error("%s: P = %d points do not fit ntiles = %d row tiles of %ld points (ceil(P / %ld) <= ntiles <= that + 3)", who,
                    P, ntiles, TP, TP);
    return STPDE_E_BADARG;
  }
  return STPDE_OK;
}

// the descriptor checks shared by stpde_lig_gather_nd and stpde_lig_cell_nd
static int check_gather_nd_desc(const char* who, const stpde_gather_nd_desc* d) {
  int rc = check_nd(who, d->D, d->P, d->ntiles);
  if (rc) return rc;
  if (d->N < 1 || d->B < 1 || d->p_base < 0 || (long)d->p_base + d->P >= (1L << 31)) {
    stpde_set_error("%s: bad N / B / p_base (p_base + P must fit 31 bits)", who);
    return STPDE_E_BADARG;
  }
  size_t nodes;
  rc = check_features(who, d->D, d->C);
  return rc ? rc : check_grid(who, d->D, d->B, d->n, &nodes);
}

extern "C" int stpde_lig_gather_nd(const stpde_gather_nd_desc* d, const float* pts, const float* latent, float* X, float* roww,
                                   void* stream) {
  if (!d || !pts || !latent || !X || !roww) {
    stpde_set_error("lig_gather_nd: null pointer");
    return STPDE_E_BADARG;
  }
  int rc = check_gather_nd_desc("lig_gather_nd", d);
  if (rc) return rc;
  GatherArgs a{};
  a.d = *d, a.pts = pts, a.latent = latent, a.X = X, a.roww = roww;
  if (d->D == 1) return launch_gather_nd<1>(a, (hipStream_t)stream);
  if (d->D == 2) return launch_gather_nd<2>(a, (hipStream_t)stream);
  return launch_gather_nd<4>(a, (hipStream_t)stream);
}

// one thread per point: point_cell() as the gather calls it, so cell[p] names exactly the cell whose corners the gather read
template <int D>
__global__ __launch_bounds__(256) void k_cell_nd(GatherArgs a) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)a.d.P) return;
  GeomJet gj;
  a.cell[p] = (int)point_cell<D>(a.d, a.pts, p, gj);
}

template <int D>
static int launch_cell_nd(const GatherArgs& a, hipStream_t stream) {
  STPDE_LAUNCH(k_cell_nd<D>, dim3((unsigned)(((size_t)a.d.P + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_cell_nd");
}

extern "C" int stpde_lig_cell_nd(const stpde_gather_nd_desc* d, const float* pts, int* cell, void* stream) {
  if (!d || !pts || !cell) {
    stpde_set_error("lig_cell_nd: null pointer");
    return STPDE_E_BADARG;
  }
  int rc = check_gather_nd_desc("lig_cell_nd", d);
  if (rc) return rc;
  GatherArgs a{};
  a.d = *d, a.pts = pts, a.cell = cell;
  if (d->D == 1) return launch_cell_nd<1>(a, (hipStream_t)stream);
  if (d->D == 2) return launch_cell_nd<2>(a, (hipStream_t)stream);
  return launch_cell_nd<4>(a, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------
// corner reduction
// ---------------------------------------------------------------------------------------------------------
struct CornerW {
  float w, dw[3], ddw[3];  // ddw index: pair (0,1)->0, (0,2)->1, (1,2)->2
};

__device__ __forceinline__ CornerW corner_weights(const float* cf, int corner) {
  const int bit[3] = {(corner >> 2) & 1, (corner >> 1) & 1, corner & 1};
  float om[3], dm[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    om[d] = bit[d] ? cf[3 + d] : cf[d];
    dm[d] = bit[d] ? cf[9 + d] : cf[6 + d];
  }
  CornerW c;
  c.w = om[0] * om[1] * om[2];
  c.dw[0] = dm[0] * om[1] * om[2];
  c.dw[1] = om[0] * dm[1] * om[2];
  c.dw[2] = om[0] * om[1] * dm[2];
  c.ddw[0] = dm[0] * dm[1] * om[2];
  c.ddw[1] = dm[0] * om[1] * dm[2];
  c.ddw[2] = om[0] * dm[1] * dm[2];
  return c;
}

__device__ __forceinline__ float pair_ddw(const CornerW& c, int d, int e) {
  if (d == e) return 0.f;
  const int s = d + e;  // 1 -> (0,1), 2 -> (0,2), 3 -> (1,2)
  return s == 1 ? c.ddw[0] : (s == 2 ? c.ddw[1] : c.ddw[2]);
}

struct ReduceArgs {
  stpde_jet_cfg cfg;
  int P, n_out;
  int S_mlp;   // streams present in the layer buffers (piecewise-linear activations carry no second-order streams)
  long ldp;
  const float* src;  // fwd: out_pre [tile][S][1][256]; bwd: jets_bar [S][n_out][P]
  const float* coef;
  float* dst;  // fwd: jets [S][n_out][P]; bwd: abar_out [tile][S][1][256]
};

// one thread per (point, channel)
__global__ __launch_bounds__(256) void k_reduce_fwd(ReduceArgs a) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.P * a.n_out) return;
  const int p = gid / a.n_out, ch = gid % a.n_out;
  const int S1 = a.cfg.S1, S2 = a.cfg.S2, S = 1 + S1 + S2;
  float cf[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 v = ld4(a.coef + (size_t)p * 16 + 4 * i);
    cf[4 * i] = v[0];
    cf[4 * i + 1] = v[1];
    cf[4 * i + 2] = v[2];
    cf[4 * i + 3] = v[3];
  }
  const float* kap = cf + 12;
  float y[10];
#pragma unroll
  for (int s = 0; s < 10; ++s) y[s] = 0.f;
  const int tile = p >> 1;
  for (int corner = 0; corner < 8; ++corner) {
    const int j = ((p & 1) << 3) | corner;
    const int lane = ((ch >> 2) << 4) | j;
    const float* base = a.src + (size_t)tile * a.S_mlp * 256 + lane * 4 + (ch & 3);
    float f[10];
#pragma unroll
    for (int s = 0; s < 10; ++s) f[s] = s < a.S_mlp ? base[(size_t)s * 256] : 0.f;
    CornerW c = corner_weights(cf, corner);
    y[0] += c.w * f[0];
    if (S1 == 3) {
#pragma unroll
      for (int d = 0; d < 3; ++d) y[1 + d] += c.dw[d] * f[0] + c.w * kap[d] * f[1 + d];
      if (a.cfg.combo) {
        // combined stream: L y = sum_k alpha_k d2y/dq_a dq_b ; the MLP stream f[4] already carries
        // sum_k alpha_k kappa_a kappa_b d2f/dr_a dr_b
        const float* al = a.cfg.alpha;
        float acc = c.w * f[4];
        acc += (al[1] * c.ddw[0] + al[2] * c.ddw[1] + al[4] * c.ddw[2]) * f[0];
        acc += 2.f * (al[0] * c.dw[0] * kap[0] * f[1] + al[3] * c.dw[1] * kap[1] * f[2] + al[5] * c.dw[2] * kap[2] * f[3]);
        acc += al[1] * (c.dw[0] * kap[1] * f[2] + c.dw[1] * kap[0] * f[1]);
        acc += al[2] * (c.dw[0] * kap[2] * f[3] + c.dw[2] * kap[0] * f[1]);
        acc += al[4] * (c.dw[1] * kap[2] * f[3] + c.dw[2] * kap[1] * f[2]);
        y[4] += acc;
      } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (k < S2) {
          const int d = a.cfg.pair0[k], e = a.cfg.pair1[k];
          const float kd = sel3(d, kap[0], kap[1], kap[2]), ke = sel3(e, kap[0], kap[1], kap[2]);
          const float dwd = sel3(d, c.dw[0], c.dw[1], c.dw[2]), dwe = sel3(e, c.dw[0], c.dw[1], c.dw[2]);
          const float fd = sel3(d, f[1], f[2], f[3]), fe = sel3(e, f[1], f[2], f[3]);
          y[4 + k] += pair_ddw(c, d, e) * f[0] + dwd * ke * fe + dwe * kd * fd + c.w * kd * ke * f[4 + k];
        }
      }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 10; ++s)
    if (s < S) a.dst[((size_t)s * a.n_out + ch) * a.ldp + p] = y[s];
}

// one thread per (row tile, lane of its fragment block): lane (g, j) holds output features 4g..4g+3 of corner row j and
// writes ONE 16-byte store per stream (zeros for features >= n_out) -- the first version had one thread per feature and
// 4-byte stores scattered over the block (1.5 ms per 2^20-point launch for 2.7 GB)
__global__ __launch_bounds__(256) void k_reduce_bwd(ReduceArgs a) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.P * 32) return;
  const int lane = gid & 63;
  const int tile = gid >> 6;
  const int g = lane >> 4, j = lane & 15;
  const int p = tile * 2 + (j >> 3), corner = j & 7;
  const int S1 = a.cfg.S1, S2 = a.cfg.S2, S = 1 + S1 + S2;
  float* base = a.dst + (size_t)tile * a.S_mlp * 256 + lane * 4;
  f32x4 fbv[10];
#pragma unroll
  for (int s = 0; s < 10; ++s) fbv[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (4 * g < a.n_out) {
    float cf[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 v = ld4(a.coef + (size_t)p * 16 + 4 * i);
      cf[4 * i] = v[0];
      cf[4 * i + 1] = v[1];
      cf[4 * i + 2] = v[2];
      cf[4 * i + 3] = v[3];
    }
    const float* kap = cf + 12;
    const CornerW c = corner_weights(cf, corner);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ch = 4 * g + r;
      if (ch >= a.n_out) continue;
      float fb[10];
#pragma unroll
      for (int s = 0; s < 10; ++s) fb[s] = 0.f;
      float yb[10];
#pragma unroll
      for (int s = 0; s < 10; ++s) yb[s] = s < S ? a.src[((size_t)s * a.n_out + ch) * a.ldp + p] : 0.f;
      fb[0] = c.w * yb[0];
      if (S1 == 3) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          fb[0] += c.dw[d] * yb[1 + d];
          fb[1 + d] = c.w * kap[d] * yb[1 + d];
        }
        if (a.cfg.combo) {
          const float* al = a.cfg.alpha;
          const float gg = yb[4];
          fb[0] += (al[1] * c.ddw[0] + al[2] * c.ddw[1] + al[4] * c.ddw[2]) * gg;
          fb[1] += (2.f * al[0] * c.dw[0] * kap[0] + al[1] * c.dw[1] * kap[0] + al[2] * c.dw[2] * kap[0]) * gg;
          fb[2] += (2.f * al[3] * c.dw[1] * kap[1] + al[1] * c.dw[0] * kap[1] + al[4] * c.dw[2] * kap[1]) * gg;
          fb[3] += (2.f * al[5] * c.dw[2] * kap[2] + al[2] * c.dw[0] * kap[2] + al[4] * c.dw[1] * kap[2]) * gg;
          fb[4] = c.w * gg;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          if (k < S2 && !a.cfg.combo) {
            const int d = a.cfg.pair0[k], e = a.cfg.pair1[k];
            const float kd = sel3(d, kap[0], kap[1], kap[2]), ke = sel3(e, kap[0], kap[1], kap[2]);
            const float dwd = sel3(d, c.dw[0], c.dw[1], c.dw[2]), dwe = sel3(e, c.dw[0], c.dw[1], c.dw[2]);
            const float gg = yb[4 + k];
            fb[0] += pair_ddw(c, d, e) * gg;
            const float te = dwd * ke * gg;  // -> f_{1+e}
            const float td = dwe * kd * gg;  // -> f_{1+d}
            fb[1] += (e == 0 ? te : 0.f) + (d == 0 ? td : 0.f);
            fb[2] += (e == 1 ? te : 0.f) + (d == 1 ? td : 0.f);
            fb[3] += (e == 2 ? te : 0.f) + (d == 2 ? td : 0.f);
            fb[4 + k] = c.w * kd * ke * gg;
          }
        }
      }
#pragma unroll
      for (int s = 0; s < 10; ++s) fbv[s][r] = fb[s];
    }
  }
#pragma unroll
  for (int s = 0; s < 10; ++s)
    if (s < a.S_mlp) st4(base + (size_t)s * 256, fbv[s]);
}

static int check_reduce(const stpde_jet_cfg* cfg, int P, int n_out, const void* a, const void* b, const void* c) {
  if (!cfg || P <= 0 || (P & 1) || n_out < 1 || n_out > 16 || !a || !b || !c || (cfg->S1 != 0 && cfg->S1 != 3) ||
      cfg->S2 < 0 || cfg->S2 > 6 || (cfg->S1 == 0 && cfg->S2 != 0)) {
    stpde_set_error("lig_reduce: bad argument");
    return STPDE_E_BADARG;
  }
  return STPDE_OK;
}

extern "C" int stpde_lig_reduce_fwd(const stpde_jet_cfg* cfg, int S_mlp, int P, int n_out, const float* out_pre,
                                    const float* coef, float* jets, long ldp, void* stream) {
  int rc = check_reduce(cfg, P, n_out, out_pre, coef, jets);
  if (rc) return rc;
  if (ldp < P || S_mlp < 1 || S_mlp > 1 + cfg->S1 + cfg->S2) {
    stpde_set_error("lig_reduce_fwd: ldp < P or bad S_mlp");
    return STPDE_E_BADARG;
  }
  ReduceArgs a{*cfg, P, n_out, S_mlp, ldp, out_pre, coef, jets};
  const size_t n = (size_t)P * n_out;
  STPDE_LAUNCH(k_reduce_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_reduce_fwd");
}

extern "C" int stpde_lig_reduce_bwd(const stpde_jet_cfg* cfg, int S_mlp, int P, int n_out, const float* jets_bar,
                                    long ldp, const float* coef, float* abar_out, void* stream) {
  int rc = check_reduce(cfg, P, n_out, jets_bar, coef, abar_out);
  if (rc) return rc;
  if (ldp < P || S_mlp < 1 || S_mlp > 1 + cfg->S1 + cfg->S2) {
    stpde_set_error("lig_reduce_bwd: ldp < P or bad S_mlp");
    return STPDE_E_BADARG;
  }
  ReduceArgs a{*cfg, P, n_out, S_mlp, ldp, jets_bar, coef, abar_out};
  const size_t n = (size_t)P * 32;      // one thread per (row tile, lane): P / 2 tiles x 64 lanes
  STPDE_LAUNCH(k_reduce_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_reduce_bwd");
}

// ---------------------------------------------------------------------------------------------------------
// corner sum of value-only queries on 1-, 2- and 4-d grids (src/local_implicit_grid.py:59 for the [b, n1..nd, c] grids the
// reference states its operator for) over the row weights roww of k_gather_nd, and its adjoint
// ---------------------------------------------------------------------------------------------------------
struct ReduceNdArgs {
  int P, n_out;
  long ldp;
  const float* src;  // out_pre [ntiles][1][1][256]: lane (g, j) holds output features 4g..4g+3 of row j
  const float* roww; // [ntiles][16]
  float* dst;        // y [n_out][ldp]
};

// one thread per (point, channel): the 2^D corner terms in corner order, fp32.  A point's rows all lie in its own tile and
// nothing but its own rows and weights is read, so the result does not depend on how the points were chunked.
// Addresses: p < P <= ntiles * (16 >> D) (checked on the host), ch < n_out <= 16 -> lane < 64; dst index < n_out * ldp.
template <int D>
__global__ __launch_bounds__(256) void k_reduce_nd(ReduceNdArgs a) {
  constexpr int TP = 16 >> D, NC = 1 << D;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.P * a.n_out) return;
  const size_t p = gid / a.n_out;
  const int ch = gid % a.n_out;
  const size_t tile = p / TP;
  const int j0 = (int)(p % TP) << D;
  float y = 0.f;
#pragma unroll
  for (int corner = 0; corner < NC; ++corner) {
    const int j = j0 | corner;
    const int lane = ((ch >> 2) << 4) | j;
    y += a.roww[tile * 16 + j] * a.src[tile * 256 + lane * 4 + (ch & 3)];
  }
  a.dst[(size_t)ch * a.ldp + p] = y;
}

template <int D>
static int launch_reduce_nd(const ReduceNdArgs& a, hipStream_t stream) {
  const size_t n = (size_t)a.P * a.n_out;
  STPDE_LAUNCH(k_reduce_nd<D>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_reduce_nd");
}

extern "C" int stpde_lig_reduce_nd_fwd(int D, int P, int ntiles, int n_out, const float* out_pre, const float* roww, float* y,
                                       long ldp, void* stream) {
  if (!out_pre || !roww || !y) {
    stpde_set_error("lig_reduce_nd_fwd: null pointer");
    return STPDE_E_BADARG;
  }
  int rc = check_nd("lig_reduce_nd_fwd", D, P, ntiles);
  if (rc) return rc;
  if (n_out < 1 || n_out > 16 || ldp < P) {
    stpde_set_error("lig_reduce_nd_fwd: n_out = %d (1..16) or ldp < P", n_out);
    return STPDE_E_BADARG;
  }
  ReduceNdArgs a{P, n_out, ldp, out_pre, roww, y};
  if (D == 1) return launch_reduce_nd<1>(a, (hipStream_t)stream);
  if (D == 2) return launch_reduce_nd<2>(a, (hipStream_t)stream);
  return launch_reduce_nd<4>(a, (hipStream_t)stream);
}

// Adjoint of k_reduce_nd (training backward on 1-, 2- and 4-d grids).  Row numbering is the gather's: row tile * 16 + j =
// point * 2^D + corner.  Addresses, bounded for every input value:
//   abar_out  gid < ntiles * 64, one float4 per thread: all of [ntiles][64][4] is written (zeros for padding rows and features
//             >= n_out -- the buffer held the forward's fc5 rows and the layer kernels read all of it)
//   roww      tile * 16 + j < ntiles * 16, read only where p < P
//   y_bar     (4g + r) * ldp + p with 4g + r < n_out, p < P <= ldp; nothing is read for p >= P
struct ReduceNdBwdArgs {
  int P, ntiles, n_out;
  long ldp;
  const float* ybar;  // [n_out][ldp]
  const float* roww;  // [ntiles][16]
  float* dst;         // abar_out [ntiles][64][4]
};

// adjoint of k_reduce_nd: one thread per (row tile, lane), one 16-byte store
template <int D>
__global__ __launch_bounds__(256) void k_reduce_nd_bwd(ReduceNdBwdArgs a) {
  constexpr int TP = 16 >> D;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.ntiles * 64) return;
  const int lane = gid & 63;
  const size_t tile = gid >> 6;
  const int g = lane >> 4, j = lane & 15;
  const size_t p = tile * TP + (j >> D);
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p < (size_t)a.P && 4 * g < a.n_out) {
    const float w = a.roww[tile * 16 + j];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < a.n_out) v[r] = w * a.ybar[(size_t)(4 * g + r) * a.ldp + p];
  }
  st4(a.dst + gid * 4, v);
}

template <int D>
static int launch_reduce_nd_bwd(const ReduceNdBwdArgs& a, hipStream_t stream) {
  const size_t n = (size_t)a.ntiles * 64;
  STPDE_LAUNCH(k_reduce_nd_bwd<D>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_reduce_nd_bwd");
}

extern "C" int stpde_lig_reduce_nd_bwd(int D, int P, int ntiles, int n_out, const float* y_bar, long ldp, const float* roww,
                                       float* abar_out, void* stream) {
  if (!y_bar || !roww || !abar_out) {
    stpde_set_error("lig_reduce_nd_bwd: null pointer");
    return STPDE_E_BADARG;
  }
  int rc = check_nd("lig_reduce_nd_bwd", D, P, ntiles);
  if (rc) return rc;
  if (n_out < 1 || n_out > 16 || ldp < P) {
    stpde_set_error("lig_reduce_nd_bwd: n_out = %d (1..16) or ldp < P", n_out);
    return STPDE_E_BADARG;
  }
  ReduceNdBwdArgs a{P, ntiles, n_out, ldp, y_bar, roww, abar_out};
  if (D == 1) return launch_reduce_nd_bwd<1>(a, (hipStream_t)stream);
  if (D == 2) return launch_reduce_nd_bwd<2>(a, (hipStream_t)stream);
  return launch_reduce_nd_bwd<4>(a, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------
// coordinate derivatives on 1- and 2-d grids, forward only: the per-point coefficient record and the corner sum of every
// derivative stream (what the src/pde.py:8-9 sweeps differentiate through, for the [b, n1..nd, c] grids of
// src/local_implicit_grid.py:10-61).  Between the two run the layer kernels in their (3, 0) / (3, 2) / (3, 4) / (3, 6) stream
// sets over the 16 >> D points-per-tile image of k_gather_nd<D>; the tangent streams of the axes a grid does not have are
// identically zero there because the plan's `tanc` columns d >= D are zero (lig_jet.py, ImNetPlan).
//
// Addresses, bounded for EVERY input value -- NaN, infinite and huge coordinates included (tests/lig_nd_jet_model.py restates
// both bodies and records every index; tests/test_lig_nd_jet_host.py runs them on such coordinates):
//   k_coef_nd        grid from P alone; p < P; pts p * D + k, k < D; coef p * 16 + i, i < 16.  Nothing but pts is read: the
//                    cell index point_cell() clamps forms no address here.
//   k_reduce_nd_jet  grid from P * n_out alone; p < P <= ntiles * (16 >> D) (checked on the host), ch < n_out <= 16.
//                    coef   p * 16 + i, i < 16
//                    src    tile = p / TP < ntiles, stream s < S_mlp, lane = (ch >> 2) << 4 | j < 64, register ch & 3:
//                           (tile * S_mlp + s) * 256 + lane * 4 + (ch & 3) < ntiles * S_mlp * 256.  No index depends on a
//                           value read from memory: the pair indices come from the descriptor and are checked < D on the host.
//                    dst    (s * n_out + ch) * ldp + p, s < S, p < P <= ldp
// Nothing is read or written for p >= P.
// ---------------------------------------------------------------------------------------------------------
// one thread per point: point_cell<D>() as the gather calls it, so the record describes exactly the cell whose corners the
// gather read.  Layout of the dim = 3 record (write_coef); an axis the grid does not have gets om = 1, dom = 0, kap = 0.
template <int D>
__global__ __launch_bounds__(256) void k_coef_nd(GatherArgs a) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)a.d.P) return;
  GeomJet gj;
  point_cell<D>(a.d, a.pts, p, gj);
  float cf[16];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const bool has = d < D;
    cf[d] = has ? gj.om[0][d] : 1.f;
    cf[3 + d] = has ? gj.om[1][d] : 1.f;
    cf[6 + d] = has ? gj.dom[0][d] : 0.f;
    cf[9 + d] = has ? gj.dom[1][d] : 0.f;
    cf[12 + d] = has ? gj.kap[d] : 0.f;
  }
  cf[15] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) st4(a.coef + p * 16 + 4 * i, f32x4{cf[4 * i], cf[4 * i + 1], cf[4 * i + 2], cf[4 * i + 3]});
}

template <int D>
static int launch_coef_nd(const GatherArgs& a, hipStream_t stream) {
  STPDE_LAUNCH(k_coef_nd<D>, dim3((unsigned)(((size_t)a.d.P + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_coef_nd");
}

static int check_jet_dim(const char* who, int D) {
  if (D != 1 && D != 2) {
    stpde_set_error("%s: D = %d (coordinate derivatives: 1 or 2; dim = 3 has stpde_lig_gather / stpde_lig_reduce_fwd)", who, D);
    return STPDE_E_BADARG;
  }
  return STPDE_OK;
}

extern "C" int stpde_lig_coef_nd(const stpde_gather_nd_desc* d, const float* pts, float* coef, void* stream) {
  if (!d || !pts || !coef) {
    stpde_set_error("lig_coef_nd: null pointer");
    return STPDE_E_BADARG;
  }
  int rc = check_jet_dim("lig_coef_nd", d->D);
  if (!rc) rc = check_gather_nd_desc("lig_coef_nd", d);
  if (rc) return rc;
  GatherArgs a{};
  a.d = *d, a.pts = pts, a.coef = coef;
  return d->D == 1 ? launch_coef_nd<1>(a, (hipStream_t)stream) : launch_coef_nd<2>(a, (hipStream_t)stream);
}

struct ReduceNdJetArgs {
  stpde_jet_cfg cfg;   // the streams of dst
  int P, n_out;
  int S_mlp;           // streams present in src (piecewise-linear activations carry no second-order streams)
  long ldp;
  const float* src;    // out_pre [ntiles][S_mlp][1][256]
  const float* coef;   // [P][16]
  float* dst;          // jets [S][n_out][ldp]
};

// one thread per (point, channel): the 2^D corner terms in corner order with the arithmetic of k_reduce_fwd -- the corner of
// the dim = 3 record is the corner of the cell with bit 0 on the axes the grid does not have, whose om = 1 leaves every
// product as it is.  The streams of those axes are not computed at all (0 * f would turn a NaN of the decoder into a NaN of a
// derivative that is identically zero): they are stored as +0.0.
template <int D>
__global__ __launch_bounds__(256) void k_reduce_nd_jet(ReduceNdJetArgs a) {
  constexpr int TP = 16 >> D, NC = 1 << D;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.P * a.n_out) return;
  const size_t p = gid / a.n_out;
  const int ch = gid % a.n_out;
  const int S1 = a.cfg.S1, S2 = a.cfg.S2, S = 1 + S1 + S2;
  float cf[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 v = ld4(a.coef + p * 16 + 4 * i);
    cf[4 * i] = v[0];
    cf[4 * i + 1] = v[1];
    cf[4 * i + 2] = v[2];
    cf[4 * i + 3] = v[3];
  }
  const float* kap = cf + 12;
  float y[10];
#pragma unroll
  for (int s = 0; s < 10; ++s) y[s] = 0.f;
  const size_t tile = p / TP;
  const int j0 = (int)(p % TP) << D;
#pragma unroll
  for (int corner = 0; corner < NC; ++corner) {
    const int j = j0 | corner;
    const int lane = ((ch >> 2) << 4) | j;
    const float* base = a.src + tile * (size_t)a.S_mlp * 256 + lane * 4 + (ch & 3);
    float f[10];
#pragma unroll
    for (int s = 0; s < 10; ++s) f[s] = s < a.S_mlp ? base[(size_t)s * 256] : 0.f;
    int c3 = 0;   // the corner in the dim = 3 numbering: first axis most significant, absent axes bit 0
#pragma unroll
    for (int k = 0; k < D; ++k) c3 |= corner_bit(corner, D, k) << (2 - k);
    const CornerW c = corner_weights(cf, c3);
    y[0] += c.w * f[0];
    if (S1 == 3) {
#pragma unroll
      for (int d = 0; d < D; ++d) y[1 + d] += c.dw[d] * f[0] + c.w * kap[d] * f[1 + d];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (k < S2) {
          const int d = a.cfg.pair0[k], e = a.cfg.pair1[k];   // < D (checked on the host)
          const float kd = sel3(d, kap[0], kap[1], kap[2]), ke = sel3(e, kap[0], kap[1], kap[2]);
          const float dwd = sel3(d, c.dw[0], c.dw[1], c.dw[2]), dwe = sel3(e, c.dw[0], c.dw[1], c.dw[2]);
          const float fd = sel3(d, f[1], f[2], f[3]), fe = sel3(e, f[1], f[2], f[3]);
          y[4 + k] += pair_ddw(c, d, e) * f[0] + dwd * ke * fe + dwe * kd * fd + c.w * kd * ke * f[4 + k];
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 10; ++s)
    if (s < S) a.dst[((size_t)s * a.n_out + ch) * a.ldp + p] = (s >= 1 + D && s < 4) ? 0.f : y[s];
}

template <int D>
static int launch_reduce_nd_jet(const ReduceNdJetArgs& a, hipStream_t stream) {
  const size_t n = (size_t)a.P * a.n_out;
  STPDE_LAUNCH(k_reduce_nd_jet<D>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_reduce_nd_jet");
}

// the argument checks shared by stpde_lig_reduce_nd_jet_fwd and its adjoint (a, b, c: the three buffers)
static int check_reduce_nd_jet(const char* who, const stpde_jet_cfg* cfg, int S_mlp, int D, int P, int ntiles, int n_out,
                               long ldp, const void* a, const void* b, const void* c) {
  if (!cfg || !a || !b || !c) {
    stpde_set_error("%s: null pointer", who);
    return STPDE_E_BADARG;
  }
  int rc = check_jet_dim(who, D);
  if (!rc) rc = check_nd(who, D, P, ntiles);
  if (rc) return rc;
  if (n_out < 1 || n_out > 16 || ldp < P) {
    stpde_set_error("%s: n_out = %d (1..16) or ldp < P", who, n_out);
    return STPDE_E_BADARG;
  }
  if ((cfg->S1 != 0 && cfg->S1 != 3) || (cfg->S2 != 0 && cfg->S2 != 2 && cfg->S2 != 4 && cfg->S2 != 6) ||
      (cfg->S1 == 0 && cfg->S2 != 0)) {
    stpde_set_error("%s: stream set (S1, S2) = (%d, %d): S1 0 or 3, S2 0, 2, 4 or 6 (with S1 = 3)", who, cfg->S1, cfg->S2);
    return STPDE_E_BADARG;
  }
  if (cfg->combo) {
    stpde_set_error("%s: the combined second-order stream is dim = 3 only", who);
    return STPDE_E_BADARG;
  }
  for (int k = 0; k < cfg->S2; ++k)
    if (cfg->pair0[k] < 0 || cfg->pair0[k] >= D || cfg->pair1[k] < 0 || cfg->pair1[k] >= D) {
      stpde_set_error("%s: pair %d = (%d, %d) names an axis a D = %d grid does not have", who, k, cfg->pair0[k], cfg->pair1[k], D);
      return STPDE_E_BADARG;
    }
  if (S_mlp < 1 || S_mlp > 1 + cfg->S1 + cfg->S2) {
    stpde_set_error("%s: S_mlp = %d outside 1..%d", who, S_mlp, 1 + cfg->S1 + cfg->S2);
    return STPDE_E_BADARG;
  }
  return STPDE_OK;
}

extern "C" int stpde_lig_reduce_nd_jet_fwd(const stpde_jet_cfg* cfg, int S_mlp, int D, int P, int ntiles, int n_out,
                                           const float* out_pre, const float* coef, float* jets, long ldp, void* stream) {
  const int rc = check_reduce_nd_jet("lig_reduce_nd_jet_fwd", cfg, S_mlp, D, P, ntiles, n_out, ldp, out_pre, coef, jets);
  if (rc) return rc;
  ReduceNdJetArgs a{*cfg, P, n_out, S_mlp, ldp, out_pre, coef, jets};
  return D == 1 ? launch_reduce_nd_jet<1>(a, (hipStream_t)stream) : launch_reduce_nd_jet<2>(a, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------
// Adjoint of k_reduce_nd_jet (training through PDE residuals on 1- and 2-d grids): jets_bar [S][n_out][ldp] -> the adjoint of
// the fc5 rows, over the forward's out_pre buffer.  Thread layout of k_reduce_bwd: one thread per (row tile, lane), lane (g, j)
// holds output features 4g..4g+3 of row j and issues one 16-byte store per stream.  Row j of tile t belongs to point
// p = t * (16 >> D) + (j >> D), corner j & (2^D - 1), mapped to the dim = 3 corner numbering as in the forward (first axis most
// significant, the bits of the axes the grid does not have 0); the coefficient algebra is k_reduce_bwd's.  The rows
// jets_bar[1 + k], k >= D, are NEVER read: the forward stores those outputs as the literal +0.0, so their cotangent is
// dropped -- a NaN there reaches nothing -- and the adjoints of the tangent streams k >= D are written as +0.0.
//
// Addresses, bounded for every input value:
//   grid      from ntiles alone: gid < ntiles * 64 (ntiles * 16 < 2^31, ceil(P / TP) <= ntiles <= that + 3: check_nd)
//   abar_out  (tile * S_mlp + s) * 256 + lane * 4 + r, s < S_mlp, lane < 64, r < 4: ALL of [ntiles][S_mlp][256] is written --
//             zeros for features >= n_out, padding rows (p >= P) and the tangent streams of the axes k >= D (the buffer held
//             the forward's fc5 rows and the layer kernels read all of it)
//   coef      p * 16 + i, i < 16, read only for p < P
//   jets_bar  (s * n_out + ch) * ldp + p with s < S, ch = 4g + r < n_out, p < P <= ldp; nothing is read for p >= P
// No index depends on a value read from memory: the pair indices come from the descriptor and are checked < D on the host.
// ---------------------------------------------------------------------------------------------------------
struct ReduceNdJetBwdArgs {
  stpde_jet_cfg cfg;   // the streams of jets_bar
  int P, ntiles, n_out;
  int S_mlp;           // streams of dst (piecewise-linear activations carry no second-order streams)
  long ldp;
  const float* src;    // jets_bar [S][n_out][ldp]
  const float* coef;   // [P][16]
  float* dst;          // abar_out [ntiles][S_mlp][1][256]
};

template <int D>
__global__ __launch_bounds__(256) void k_reduce_nd_jet_bwd(ReduceNdJetBwdArgs a) {
  constexpr int TP = 16 >> D, NC = 1 << D;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.ntiles * 64) return;
  const int lane = gid & 63;
  const size_t tile = gid >> 6;
  const int g = lane >> 4, j = lane & 15;
  const size_t p = tile * TP + (j >> D);
  const int corner = j & (NC - 1);
  const int S1 = a.cfg.S1, S2 = a.cfg.S2, S = 1 + S1 + S2;
  float* base = a.dst + tile * (size_t)a.S_mlp * 256 + lane * 4;
  f32x4 fbv[10];
#pragma unroll
  for (int s = 0; s < 10; ++s) fbv[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p < (size_t)a.P && 4 * g < a.n_out) {
    float cf[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 v = ld4(a.coef + p * 16 + 4 * i);
      cf[4 * i] = v[0];
      cf[4 * i + 1] = v[1];
      cf[4 * i + 2] = v[2];
      cf[4 * i + 3] = v[3];
    }
    const float* kap = cf + 12;
    int c3 = 0;   // the corner in the dim = 3 numbering: first axis most significant, absent axes bit 0
#pragma unroll
    for (int k = 0; k < D; ++k) c3 |= corner_bit(corner, D, k) << (2 - k);
    const CornerW c = corner_weights(cf, c3);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ch = 4 * g + r;
      if (ch >= a.n_out) continue;
      float fb[10];
#pragma unroll
      for (int s = 0; s < 10; ++s) fb[s] = 0.f;
      float yb[10];
#pragma unroll
      for (int s = 0; s < 10; ++s)
        yb[s] = (s < S && !(s >= 1 + D && s < 4)) ? a.src[((size_t)s * a.n_out + ch) * a.ldp + p] : 0.f;
      fb[0] = c.w * yb[0];
      if (S1 == 3) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          fb[0] += c.dw[d] * yb[1 + d];
          fb[1 + d] = c.w * kap[d] * yb[1 + d];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          if (k < S2) {
            const int d = a.cfg.pair0[k], e = a.cfg.pair1[k];   // < D (checked on the host)
            const float kd = sel3(d, kap[0], kap[1], kap[2]), ke = sel3(e, kap[0], kap[1], kap[2]);
            const float dwd = sel3(d, c.dw[0], c.dw[1], c.dw[2]), dwe = sel3(e, c.dw[0], c.dw[1], c.dw[2]);
            const float gg = yb[4 + k];
            fb[0] += pair_ddw(c, d, e) * gg;
            const float te = dwd * ke * gg;  // -> f_{1+e}
            const float td = dwe * kd * gg;  // -> f_{1+d}
#pragma unroll
            for (int x = 0; x < D; ++x) fb[1 + x] += (e == x ? te : 0.f) + (d == x ? td : 0.f);
            fb[4 + k] = c.w * kd * ke * gg;
          }
        }
      }
#pragma unroll
      for (int s = 0; s < 10; ++s) fbv[s][r] = fb[s];
    }
  }
#pragma unroll
  for (int s = 0; s < 10; ++s)
    if (s < a.S_mlp) st4(base + (size_t)s * 256, fbv[s]);
}

template <int D>
static int launch_reduce_nd_jet_bwd(const ReduceNdJetBwdArgs& a, hipStream_t stream) {
  const size_t n = (size_t)a.ntiles * 64;
  STPDE_LAUNCH(k_reduce_nd_jet_bwd<D>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_reduce_nd_jet_bwd");
}

extern "C" int stpde_lig_reduce_nd_jet_bwd(const stpde_jet_cfg* cfg, int S_mlp, int D, int P, int ntiles, int n_out,
                                           const float* jets_bar, long ldp, const float* coef, float* abar_out, void* stream) {
  const int rc = check_reduce_nd_jet("lig_reduce_nd_jet_bwd", cfg, S_mlp, D, P, ntiles, n_out, ldp, jets_bar, coef, abar_out);
  if (rc) return rc;
  ReduceNdJetBwdArgs a{*cfg, P, ntiles, n_out, S_mlp, ldp, jets_bar, coef, abar_out};
  return D == 1 ? launch_reduce_nd_jet_bwd<1>(a, (hipStream_t)stream) : launch_reduce_nd_jet_bwd<2>(a, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------
// coordinate derivatives on 4-d grids (3-d space + time), forward only.  The layer kernels carry three first-order streams, a
// 4-d grid has four axes: a request runs as up to four PASSES, each the (3, S2) layer sequence over one axis triple (a0 < a1 <
// a2) -- the caller's `tanc` packs of the pass hold the skip-block columns a0, a1, a2 -- over the ONE image of k_gather_nd<4>
// (one point = one 16-row tile).  k_coef_nd4 writes the record of all four axes once per chunk; k_reduce_nd4_jet is the corner
// sum of one pass: the weight is the product over all four axes, dw / ddw are taken for the pass's three axes, and a
// destination-stream map says which stream of the caller's jets tensor the value, each first-order slot and each pair goes to
// (-1: not stored), so that the passes of a request fill disjoint streams of one [1 + 4 + npairs][n_out][ldp] tensor.
//
// Addresses, bounded for EVERY input value -- NaN, infinite and huge coordinates included (tests/lig_nd4_jet_model.py restates
// both bodies and records every index; tests/test_lig_nd4_jet_host.py runs them on such coordinates):
//   k_coef_nd4        grid from P alone; p < P; pts p * 4 + k, k < 4; coef p * 24 + i, i < 24.  Nothing but pts is read: the
//                     cell index point_cell() clamps forms no address here.
//   k_reduce_nd4_jet  grid from P * n_out alone; p < P <= ntiles (one point per tile: checked on the host), ch < n_out <= 16.
//                     coef   p * 24 + i, i < 24
//                     src    tile = p < ntiles, stream s < S_mlp, lane = (ch >> 2) << 4 | corner < 64 (corner < 16), register
//                            ch & 3: (p * S_mlp + s) * 256 + lane * 4 + (ch & 3) < ntiles * S_mlp * 256
//                     dst    (t * n_out + ch) * ldp + p with t an entry of the destination map: -1 (skipped) or 0 <= t < S
//                            (checked on the host), p < P <= ldp
//                     No index depends on a value read from memory: axes, pairs and the destination map come from the
//                     descriptor and are checked on the host; they select VALUES (sel4), never addresses of the record.
// Nothing is read or written for p >= P, and a pass writes no stream its map does not name.
// ---------------------------------------------------------------------------------------------------------
// one thread per point: point_cell<4>() as the gather calls it, so the record describes exactly the cell whose corners the
// gather read.  coef[p][24] = {om[0][k], om[1][k], dom[0][k], dom[1][k], kap[k]} at 0 / 4 / 8 / 12 / 16 + k, entries 20 .. 23 = 0.
__global__ __launch_bounds__(256) void k_coef_nd4(GatherArgs a) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)a.d.P) return;
  GeomJet gj;
  point_cell<4>(a.d, a.pts, p, gj);
  float* cf = a.coef + p * 24;
  st4(cf, f32x4{gj.om[0][0], gj.om[0][1], gj.om[0][2], gj.om[0][3]});
  st4(cf + 4, f32x4{gj.om[1][0], gj.om[1][1], gj.om[1][2], gj.om[1][3]});
  st4(cf + 8, f32x4{gj.dom[0][0], gj.dom[0][1], gj.dom[0][2], gj.dom[0][3]});
  st4(cf + 12, f32x4{gj.dom[1][0], gj.dom[1][1], gj.dom[1][2], gj.dom[1][3]});
  st4(cf + 16, f32x4{gj.kap[0], gj.kap[1], gj.kap[2], gj.kap[3]});
  st4(cf + 20, f32x4{0.f, 0.f, 0.f, 0.f});
}

extern "C" int stpde_lig_coef_nd4(const stpde_gather_nd_desc* d, const float* pts, float* coef, void* stream) {
  if (!d || !pts || !coef) {
    stpde_set_error("lig_coef_nd4: null pointer");
    return STPDE_E_BADARG;
  }
  if (d->D != 4) {
    stpde_set_error("lig_coef_nd4: D = %d (the record of all four axes: 4; D = 1, 2 have stpde_lig_coef_nd)", d->D);
    return STPDE_E_BADARG;
  }
  const int rc = check_gather_nd_desc("lig_coef_nd4", d);
  if (rc) return rc;
  GatherArgs a{};
  a.d = *d, a.pts = pts, a.coef = coef;
  STPDE_LAUNCH(k_coef_nd4, dim3((unsigned)(((size_t)a.d.P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_coef_nd4");
}

__device__ __forceinline__ float sel4(int d, float a0, float a1, float a2, float a3) {
  return d == 0 ? a0 : (d == 1 ? a1 : (d == 2 ? a2 : a3));
}

struct ReduceNd4Args {
  stpde_nd4_pass_desc d;
  int slot0[6], slot1[6];   // pair k in slots of the triple: axis[slot0[k]] = pair0[k] (derived on the host)
  int P, n_out;
  long ldp;
  const float* src;    // out_pre [ntiles][S_mlp][1][256]
  const float* coef;   // [P][24]
  float* dst;          // jets [S][n_out][ldp]
};

// one thread per (point, channel): the 16 corner terms in corner order with the arithmetic of k_reduce_nd_jet.  Slot i of the
// pass is axis d.axis[i]: f[1 + i] is the tangent stream of that axis, pair k names two slots.
__global__ __launch_bounds__(256) void k_reduce_nd4_jet(ReduceNd4Args a) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)a.P * a.n_out) return;
  const size_t p = gid / a.n_out;
  const int ch = gid % a.n_out;
  const int S2 = a.d.npairs, S_mlp = a.d.S_mlp;
  float cf[24];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    f32x4 v = ld4(a.coef + p * 24 + 4 * i);
    cf[4 * i] = v[0];
    cf[4 * i + 1] = v[1];
    cf[4 * i + 2] = v[2];
    cf[4 * i + 3] = v[3];
  }
  float ks[3];   // kappa of the pass's three slots
#pragma unroll
  for (int i = 0; i < 3; ++i) ks[i] = sel4(a.d.axis[i], cf[16], cf[17], cf[18], cf[19]);
  float y[10];
#pragma unroll
  for (int s = 0; s < 10; ++s) y[s] = 0.f;
  for (int corner = 0; corner < 16; ++corner) {
    const int lane = ((ch >> 2) << 4) | corner;
    const float* base = a.src + p * (size_t)S_mlp * 256 + lane * 4 + (ch & 3);
    float f[10];
#pragma unroll
    for (int s = 0; s < 10; ++s) f[s] = s < S_mlp ? base[(size_t)s * 256] : 0.f;
    float om[4], dm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int bit = corner_bit(corner, 4, k);
      om[k] = bit ? cf[4 + k] : cf[k];
      dm[k] = bit ? cf[12 + k] : cf[8 + k];
    }
    const float w = om[0] * om[1] * om[2] * om[3];
    float dw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ax = a.d.axis[i];
      dw[i] = (ax == 0 ? dm[0] : om[0]) * (ax == 1 ? dm[1] : om[1]) * (ax == 2 ? dm[2] : om[2]) * (ax == 3 ? dm[3] : om[3]);
    }
    y[0] += w * f[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) y[1 + i] += dw[i] * f[0] + w * ks[i] * f[1 + i];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if (k < S2) {
        const int d = a.slot0[k], e = a.slot1[k];       // slots < 3 (derived on the host from the pair's axes)
        const int ad = a.d.pair0[k], ae = a.d.pair1[k];
        const float kd = sel3(d, ks[0], ks[1], ks[2]), ke = sel3(e, ks[0], ks[1], ks[2]);
        const float dwd = sel3(d, dw[0], dw[1], dw[2]), dwe = sel3(e, dw[0], dw[1], dw[2]);
        const float fd = sel3(d, f[1], f[2], f[3]), fe = sel3(e, f[1], f[2], f[3]);
        float ddw = 0.f;
        if (d != e)
          ddw = ((ad == 0 || ae == 0) ? dm[0] : om[0]) * ((ad == 1 || ae == 1) ? dm[1] : om[1]) *
                ((ad == 2 || ae == 2) ? dm[2] : om[2]) * ((ad == 3 || ae == 3) ? dm[3] : om[3]);
        y[4 + k] += ddw * f[0] + dwd * ke * fe + dwe * kd * fd + w * kd * ke * f[4 + k];
      }
    }
  }
  if (a.d.dst_value >= 0) a.dst[((size_t)a.d.dst_value * a.n_out + ch) * a.ldp + p] = y[0];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (a.d.dst_first[i] >= 0) a.dst[((size_t)a.d.dst_first[i] * a.n_out + ch) * a.ldp + p] = y[1 + i];
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (k < S2 && a.d.dst_pair[k] >= 0) a.dst[((size_t)a.d.dst_pair[k] * a.n_out + ch) * a.ldp + p] = y[4 + k];
}

extern "C" int stpde_lig_reduce_nd4_jet_fwd(const stpde_nd4_pass_desc* d, int D, int P, int ntiles, int n_out, const float* out_pre,
                                            const float* coef, float* jets, long ldp, void* stream) {
  const char* who = "lig_reduce_nd4_jet_fwd";
  if (!d || !out_pre || !coef || !jets) {
    stpde_set_error("%s: null pointer", who);
    return STPDE_E_BADARG;
  }
  if (D != 4) {
    stpde_set_error("%s: D = %d (passes over axis triples of a 4-d grid: 4; D = 1, 2 have stpde_lig_reduce_nd_jet_fwd)", who, D);
    return STPDE_E_BADARG;
  }
  const int rc = check_nd(who, 4, P, ntiles);
  if (rc) return rc;
  if (n_out < 1 || n_out > 16 || ldp < P) {
    stpde_set_error("%s: n_out = %d (1..16) or ldp < P", who, n_out);
    return STPDE_E_BADARG;
  }
  if (d->axis[0] < 0 || d->axis[0] >= d->axis[1] || d->axis[1] >= d->axis[2] || d->axis[2] >= 4) {
    stpde_set_error("%s: axis triple (%d, %d, %d) is not strictly increasing inside 0..3", who, d->axis[0], d->axis[1], d->axis[2]);
    return STPDE_E_BADARG;
  }
  if (d->npairs != 0 && d->npairs != 2 && d->npairs != 4 && d->npairs != 6) {
    stpde_set_error("%s: npairs = %d (the S2 of a stream set: 0, 2, 4 or 6)", who, d->npairs);
    return STPDE_E_BADARG;
  }
  if (d->S_mlp != 4 && d->S_mlp != 4 + d->npairs) {
    stpde_set_error("%s: S_mlp = %d (4, or 4 + npairs = %d)", who, d->S_mlp, 4 + d->npairs);
    return STPDE_E_BADARG;
  }
  if (d->S < 1 || d->S > 15) {
    stpde_set_error("%s: S = %d streams of the jets tensor (1..15)", who, d->S);
    return STPDE_E_BADARG;
  }
  ReduceNd4Args a{};
  a.d = *d;
  for (int k = 0; k < d->npairs; ++k) {
    int s0 = -1, s1 = -1;
    for (int i = 0; i < 3; ++i) {
      if (d->axis[i] == d->pair0[k]) s0 = i;
      if (d->axis[i] == d->pair1[k]) s1 = i;
    }
    if (s0 < 0 || s1 < 0) {
      stpde_set_error("%s: pair %d = (%d, %d) names an axis outside the triple (%d, %d, %d)", who, k, d->pair0[k], d->pair1[k],
                      d->axis[0], d->axis[1], d->axis[2]);
      return STPDE_E_BADARG;
    }
    a.slot0[k] = s0, a.slot1[k] = s1;
  }
  int dsts[10], nd = 0;
  dsts[nd++] = d->dst_value;
  for (int i = 0; i < 3; ++i) dsts[nd++] = d->dst_first[i];
  for (int k = 0; k < d->npairs; ++k) dsts[nd++] = d->dst_pair[k];
  for (int i = 0; i < nd; ++i) {
    if (dsts[i] < -1 || dsts[i] >= d->S) {
      stpde_set_error("%s: destination stream %d outside [-1, %d)", who, dsts[i], d->S);
      return STPDE_E_BADARG;
    }
    for (int j = 0; j < i; ++j)
      if (dsts[i] >= 0 && dsts[i] == dsts[j]) {
        stpde_set_error("%s: destination stream %d named twice", who, dsts[i]);
        return STPDE_E_BADARG;
      }
  }
  a.P = P, a.n_out = n_out, a.ldp = ldp, a.src = out_pre, a.coef = coef, a.dst = jets;
  const size_t n = (size_t)P * n_out;
  STPDE_LAUNCH(k_reduce_nd4_jet, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_reduce_nd4_jet");
}

// ---------------------------------------------------------------------------------------------------------
// xbar = sum_l W_s,l^T abar_l (value stream)  ->  scatter-add into d latent
// ---------------------------------------------------------------------------------------------------------
struct XbarArgs {
  stpde_xbar_desc d;
  const float* abar[8];
  const float* wsl[8];  // [MT_l][XL][256]: A operand of W_s,l^T restricted to the latent channels (row m = channel 16 xl + m)
  const int* cell;
  float* dlatent;
  float* xrows;  // != null: per-row latent adjoints [16 * ntiles][CP] instead of atomics (deterministic path)
  int CP;        // row length of xrows = C rounded up to a multiple of 4
};

constexpr int XPAD = 49;   // padded row length (floats) of the 16 x 48 transpose patch: odd -> conflict-free columns
#ifndef STPDE_XBAR_R
#define STPDE_XBAR_R 4
#endif
constexpr int XR = STPDE_XBAR_R;      // row tiles per wave: every weight fragment fetched from L2 feeds XR * XL * 4 MFMAs

// XL = number of 16-channel output tiles (C <= 16 XL).  The coordinate / bias columns of the augmented input get no
// adjoint (query points carry no gradient), so only the latent channels are contracted.  Round 2: one row tile per wave
// and all 3 augmented-input tiles made the kernel L2-bound on the weight fragments (3 KB of weights per 1 KB of abar).
template <int XL>
__global__ __launch_bounds__(256) void k_xbar(XbarArgs a) {
  const int lane = threadIdx.x & 63;
  const int tile0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * XR;
  if (tile0 >= a.d.ntiles) return;
  const int lo = lane * 4;
  int tl[XR];
#pragma unroll
  for (int t = 0; t < XR; ++t) tl[t] = tile0 + t < a.d.ntiles ? tile0 + t : a.d.ntiles - 1;   // clamp, stores are guarded
  f32x4 acc[XR][XL];
#pragma unroll
  for (int t = 0; t < XR; ++t)
#pragma unroll
    for (int xl = 0; xl < XL; ++xl) acc[t][xl] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int l = 0; l < a.d.nlayers; ++l) {
    const int MT = a.d.MT[l], SP = a.d.SP[l];
    const float* ab = a.abar[l] + lo;  // stream 0 of tile t starts at (size_t)t * SP * MT * 256
    const float* w = a.wsl[l] + lo;
    if (a.d.packed[l]) {
      // packed ADJOINT buffer (bf16 mode, common.h): bf16 blocks, stream 0 first -- two blocks are one K = 32 bf16 MFMA
      // against the weight blocks of the same two output tiles, rounded here
      const char* ab16 = reinterpret_cast<const char*>(a.abar[l]) + lane * 8;
      const size_t tb = blk_tile_bytes(2, a.d.S[l], MT);
      const bf16x4 z4 = to_bf4(f32x4{0.f, 0.f, 0.f, 0.f});
      for (int mt = 0; mt < MT; mt += 2) {
        const bool two = mt + 1 < MT;
        bf16x8 B8[XR];
#pragma unroll
        for (int t = 0; t < XR; ++t) {
          const char* bp = ab16 + tl[t] * tb + (size_t)mt * 512;
          B8[t] = cat8(*reinterpret_cast<const bf16x4*>(bp), two ? *reinterpret_cast<const bf16x4*>(bp + 512) : z4);
        }
#pragma unroll
        for (int xl = 0; xl < XL; ++xl) {
          const f32x4 w0 = ld4(w + ((size_t)mt * XL + xl) * 256);
          const f32x4 w1 = two ? ld4(w + ((size_t)(mt + 1) * XL + xl) * 256) : f32x4{0.f, 0.f, 0.f, 0.f};
          const bf16x8 A8 = cat8(to_bf4(w0), to_bf4(w1));
#pragma unroll
          for (int t = 0; t < XR; ++t) acc[t][xl] = mfma_bf(A8, B8[t], acc[t][xl]);
        }
      }
      continue;
    }
    const size_t tstride = (size_t)SP * MT * 256;     // floats between the value streams of consecutive tiles
    // two output tiles per iteration (MT is even for every hidden layer): their loads are issued together
    for (int mt = 0; mt + 1 < MT; mt += 2) {
      f32x4 B0[XR], B1[XR], w0[XL], w1[XL];
#pragma unroll
      for (int t = 0; t < XR; ++t) {
        B0[t] = ld4(ab + tl[t] * tstride + (size_t)mt * 256);
        B1[t] = ld4(ab + tl[t] * tstride + (size_t)(mt + 1) * 256);
      }
#pragma unroll
      for (int xl = 0; xl < XL; ++xl) {
        w0[xl] = ld4(w + ((size_t)mt * XL + xl) * 256);
        w1[xl] = ld4(w + ((size_t)(mt + 1) * XL + xl) * 256);
      }
#pragma unroll
      for (int t = 0; t < XR; ++t)
#pragma unroll
        for (int xl = 0; xl < XL; ++xl) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][xl] = mfma4(w0[xl][r], B0[t][r], acc[t][xl]);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][xl] = mfma4(w1[xl][r], B1[t][r], acc[t][xl]);
        }
    }
    if (MT & 1) {
      const int mt = MT - 1;
#pragma unroll
      for (int xl = 0; xl < XL; ++xl) {
        f32x4 wv = ld4(w + ((size_t)mt * XL + xl) * 256);
#pragma unroll
        for (int t = 0; t < XR; ++t) {
          f32x4 B = ld4(ab + tl[t] * tstride + (size_t)mt * 256);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][xl] = mfma4(wv[r], B[r], acc[t][xl]);
        }
      }
    }
  }
  const int g = lane >> 4, j = lane & 15;
  if (a.xrows) {
    // deterministic path: rows x channels through a per-wave LDS patch, then row-major, fully coalesced float4 stores;
    // the per-node sums are taken by k_dlat_reduce in a fixed order
    __shared__ float patch[4][16 * XPAD];
    float* pt = patch[threadIdx.x >> 6];
    const int q4 = a.CP >> 2;                       // float4 groups per row
#pragma unroll
    for (int t = 0; t < XR; ++t) {
      if (tile0 + t >= a.d.ntiles) break;
#pragma unroll
      for (int xl = 0; xl < XL; ++xl)
#pragma unroll
        for (int r = 0; r < 4; ++r) pt[j * XPAD + 16 * xl + 4 * g + r] = acc[t][xl][r];
      __builtin_amdgcn_wave_barrier();
      float* dst = a.xrows + (size_t)(tile0 + t) * 16 * a.CP;
      for (int idx = lane; idx < 16 * q4; idx += 64) {
        const int row = idx / q4, c4 = idx - row * q4;
        const float* src = pt + row * XPAD + 4 * c4;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (4 * c4 + r < a.d.C) ? src[r] : 0.f;
        st4(dst + (size_t)row * a.CP + 4 * c4, v);
      }
      __builtin_amdgcn_wave_barrier();
    }
    return;
  }
  const int n1 = a.d.n1, n2 = a.d.n2, C = a.d.C;
#pragma unroll
  for (int t = 0; t < XR; ++t) {
    if (tile0 + t >= a.d.ntiles) break;
    const int p = (tile0 + t) * 2 + (j >> 3), corner = j & 7;
    const size_t node =
        (size_t)a.cell[p] + ((size_t)((corner >> 2) & 1) * n1 + ((corner >> 1) & 1)) * n2 + (corner & 1);
    float* dst = a.dlatent + node * C;
#pragma unroll
    for (int xl = 0; xl < XL; ++xl)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ch = 16 * xl + 4 * g + r;
        if (ch < C) atomicAdd(dst + ch, acc[t][xl][r]);
      }
  }
}

static int launch_xbar(const stpde_xbar_desc* d, const float* const* abar, const float* const* WsL_pack,
                       const int* cell, float* dlatent, float* xrows, void* stream);

extern "C" int stpde_lig_xbar_scatter(const stpde_xbar_desc* d, const float* const* abar,
                                      const float* const* WsL_pack, const int* cell, float* dlatent, void* stream) {
  if (!cell || !dlatent) {
    stpde_set_error("lig_xbar_scatter: bad argument");
    return STPDE_E_BADARG;
  }
  return launch_xbar(d, abar, WsL_pack, cell, dlatent, nullptr, stream);
}

extern "C" int stpde_lig_xbar_rows(const stpde_xbar_desc* d, const float* const* abar, const float* const* WsL_pack,
                                   float* xrows, void* stream) {
  if (!xrows) {
    stpde_set_error("lig_xbar_rows: bad argument");
    return STPDE_E_BADARG;
  }
  return launch_xbar(d, abar, WsL_pack, nullptr, nullptr, xrows, stream);
}

static int launch_xbar(const stpde_xbar_desc* d, const float* const* abar, const float* const* WsL_pack,
                       const int* cell, float* dlatent, float* xrows, void* stream) {
  if (!d || d->ntiles <= 0 || d->nlayers < 1 || d->nlayers > 8 || !abar || !WsL_pack) {
    stpde_set_error("lig_xbar: bad argument");
    return STPDE_E_BADARG;
  }
  int rc = check_features("lig_xbar", 3, d->C);   // (the widest row: the latent of a dim = 3 grid)
  if (rc) return rc;
  XbarArgs a{};
  a.d = *d;
  for (int l = 0; l < d->nlayers; ++l) {
    if (!abar[l] || !WsL_pack[l] || d->MT[l] < 1 || d->SP[l] < 1) {
      stpde_set_error("lig_xbar_scatter: bad layer %d", l);
      return STPDE_E_BADARG;
    }
    a.abar[l] = abar[l];
    a.wsl[l] = WsL_pack[l];
  }
  a.cell = cell;
  a.dlatent = dlatent;
  a.xrows = xrows;
  a.CP = (d->C + 3) / 4 * 4;
  const dim3 grid((d->ntiles + 4 * XR - 1) / (4 * XR));
  if (d->C <= 16)
    STPDE_LAUNCH(k_xbar<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else      // C <= 32 (checked above: the sparse third tile of the augmented input holds features 32..35)
    STPDE_LAUNCH(k_xbar<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_xbar");
}

// ---------------------------------------------------------------------------------------------------------
// Deterministic d latent: per-NODE gather of the per-row adjoints written by k_xbar (xrows), in a fixed order
// (corner 0 .. 2^D - 1, then the points of the owning cell in ascending perm position), instead of fp32 atomics.
// The backward of the advanced-index gather at src/regular_nd_grid_interpolation.py:65-66 is an
// index_put_(accumulate=True), which is deterministic on the reference's CPU path; so is this.
//   perm[q]   point index of the q-th point in (stable) cell order
//   start[c]  first q of the points whose cell (= linear index of the cell's corner-0 node, incl. batch) is c;
//             start has n_nodes + 1 entries
// One group of 16 lanes per node (lane = float4 of channels), 4 nodes per wave.
//
// Addresses, for D = 1, 2, 3, 4 alike (tests/lig_nd_bwd_model.py restates the body):
//   start     cell and cell + 1 with cell < n_nodes: start has n_nodes + 1 entries
//   perm      q in [start[cell], start[cell + 1]) within [0, P) (stpde_lig_cell_sort: start[n_nodes] = P)
//   xrows     row = perm[q] * 2^D + corner < P * 2^D <= 16 * ntiles: inside the [16 * ntiles][CP] rows k_xbar wrote (the
//             buffer of a chunk is 16 * ntiles * CP floats, padding rows of the last tiles included)
//   dlatent   node < n_nodes, channel 4 c4 + r < C
// ---------------------------------------------------------------------------------------------------------
struct DlatNdArgs {
  int n[4];
  int C, CP;
  size_t nnodes;        // B * prod(n)
  const float* xrows;   // [16 * ntiles][CP]   row = 2^D * point + corner
  const int* perm;
  const int* start;
  float* dlatent;       // [B][n_0..n_{D-1}][C], accumulated into (+=)
};

// corners in the order of interp_nd.hip (first axis most significant), fp32
template <int D>
__device__ __forceinline__ void dlat_reduce(const DlatNdArgs& a) {
  constexpr int NC = 1 << D;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int c4 = gid & 15;
  const size_t node = gid >> 4;
  if (node >= a.nnodes || 4 * c4 >= a.CP) return;
  int idx[D];
  size_t stride[D];
  {
    size_t rest = node, s = 1;
#pragma unroll
    for (int k = D - 1; k >= 0; --k) {
      idx[k] = (int)(rest % (size_t)a.n[k]);
      rest /= (size_t)a.n[k];
      stride[k] = s;
      s *= (size_t)a.n[k];
    }
  }
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  bool any = false;
#pragma unroll
  for (int corner = 0; corner < NC; ++corner) {
    bool inside = true;
    size_t off = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const int bit = corner_bit(corner, D, k);
      const int c = idx[k] - bit;                      // the cell for which this node is corner `corner`
      inside = inside && c >= 0 && c <= a.n[k] - 2;
      off += (size_t)bit * stride[k];
    }
    if (!inside) continue;                             // (off <= node then: every bit set has idx[k] >= 1)
    const size_t cell = node - off;
    const int q0 = a.start[cell], q1 = a.start[cell + 1];
    for (int q = q0; q < q1; ++q) {
      const size_t row = (size_t)a.perm[q] * NC + corner;
      acc += ld4(a.xrows + row * a.CP + 4 * c4);
      any = true;
    }
  }
  if (!any) return;
  float* dst = a.dlatent + node * a.C + 4 * c4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (4 * c4 + r < a.C) dst[r] += acc[r];
}

template <int D>
__global__ __launch_bounds__(256) void k_dlat_reduce_nd(DlatNdArgs a) {
  dlat_reduce<D>(a);
}

__global__ __launch_bounds__(256) void k_dlat_reduce(DlatNdArgs a) { dlat_reduce<3>(a); }

template <int D>
static int launch_dlat_reduce_nd(const DlatNdArgs& a, hipStream_t stream) {
  const size_t n = a.nnodes * 16;
  STPDE_LAUNCH(k_dlat_reduce_nd<D>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_dlat_reduce_nd");
}

// the checks and the argument record shared by the two entry points
static int dlat_args(const char* who, int D, int B, const int* n, int C, const float* xrows, const int* perm, const int* start,
                     float* dlatent, DlatNdArgs* a, bool int32_nodes = true) {
  if (B < 1 || C < 1 || C > 64) {
    stpde_set_error("%s: bad B or C = %d (1..64)", who, C);
    return STPDE_E_BADARG;
  }
  *a = DlatNdArgs{};
  for (int k = 0; k < D; ++k) a->n[k] = n[k];
  a->C = C, a->CP = (C + 3) / 4 * 4;
  a->xrows = xrows, a->perm = perm, a->start = start, a->dlatent = dlatent;
  return check_grid(who, D, B, n, &a->nnodes, int32_nodes);
}

extern "C" int stpde_lig_dlatent_reduce(int B, int n0, int n1, int n2, int C, const float* xrows, const int* perm,
                                        const int* start, float* dlatent, void* stream) {
  if (!xrows || !perm || !start || !dlatent) {
    stpde_set_error("lig_dlatent_reduce: null pointer");
    return STPDE_E_BADARG;
  }
  const int n[3] = {n0, n1, n2};
  DlatNdArgs a;
  int rc = dlat_args("lig_dlatent_reduce", 3, B, n, C, xrows, perm, start, dlatent, &a, false);
  if (rc) return rc;
  STPDE_LAUNCH(k_dlat_reduce, dim3((unsigned)((a.nnodes * 16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_dlat_reduce");
}

extern "C" int stpde_lig_dlatent_reduce_nd(int D, int B, const int* n, int C, const float* xrows, const int* perm,
                                           const int* start, float* dlatent, void* stream) {
  if (!n || !xrows || !perm || !start || !dlatent) {
    stpde_set_error("lig_dlatent_reduce_nd: null pointer");
    return STPDE_E_BADARG;
  }
  if (D != 1 && D != 2 && D != 4) {
    stpde_set_error("lig_dlatent_reduce_nd: D = %d (1, 2 or 4; dim = 3 has stpde_lig_dlatent_reduce)", D);
    return STPDE_E_BADARG;
  }
  DlatNdArgs a;
  int rc = dlat_args("lig_dlatent_reduce_nd", D, B, n, C, xrows, perm, start, dlatent, &a);
  if (rc) return rc;
  if (D == 1) return launch_dlat_reduce_nd<1>(a, (hipStream_t)stream);
  if (D == 2) return launch_dlat_reduce_nd<2>(a, (hipStream_t)stream);
  return launch_dlat_reduce_nd<4>(a, (hipStream_t)stream);
}
