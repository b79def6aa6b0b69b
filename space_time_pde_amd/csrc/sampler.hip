// Training batches drawn and produced on the device (include/stpde_hip.h, "N3 on the device"): crop ids and query points from
// Philox4x32-10 with its state in device memory, then ONE gather kernel that writes the low-resolution input grid and the
// interpolated point targets straight from the channels-last dataset -- what RB2DeviceLoader.get() does with a host
// round trip, per-crop slicing, torch.rand, three index_select pairs, the interpolation kernel and two normalisations.
// HBM/L2-bound gather: one thread per low-res voxel / per query point, all 4 channels of a node as one 16-byte load; lanes run
// along x (low-res part: the four channel planes of the output are written 256 contiguous bytes per wave each).
// Built with -ffp-contract=off like the rest of the library: every expression below rounds where the torch stages and
// k_interp round (interp_geom.h is shared with it).
//
// With a low-res pre-filter (gaussian / uniform / maximum, stpde_sampler_filter) the crops ARE materialised: up to three 1-D
// passes (t, then z, then x) over two caller-owned scratch crops [B][nt][nz][nx][4] that ping-pong, then the same gather with
// crop-local addressing (k_sampler_produce_crop).  See "filter passes" below for the arithmetic and the address budget.
// The median pre-filter is not separable: one selection kernel of its own in sampler_median.hip, feeding the same crop gather.
#include "interp_geom.h"

struct SamplerArgs {
  stpde_sampler_desc d;
  stpde_sampler_state* st;
  const float* data;
  const stpde_sampler_tap* tap[3];
  const int* idx;
  const float* pc;
  float* lres;
  float* pv;
  int* idx_out;
  float* pc_out;
  unsigned blocks_lres;
};

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) ---------------------
struct Philox4 {
  unsigned w[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// one thread per Philox call: calls [0, nq0) are the crop-id stream (purpose 0), the rest the coordinate stream (purpose 1)
__global__ __launch_bounds__(256) void k_sampler_draw(SamplerArgs a) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  const unsigned nid = (unsigned)a.d.B, nco = (unsigned)a.d.B * (unsigned)a.d.N * 3u;
  const unsigned nq0 = (nid + 3u) / 4u, nq1 = (nco + 3u) / 4u;
  if (g >= nq0 + nq1) return;
  const unsigned long long seed = a.st->seed, off = a.st->offset;
  const unsigned purpose = g < nq0 ? 0u : 1u, q = purpose ? g - nq0 : g;
  const Philox4 r = philox4x32_10((unsigned)off, (unsigned)(off >> 32), q, purpose, (unsigned)seed, (unsigned)(seed >> 32));
  if (!purpose) {
    const unsigned long long len = (unsigned long long)a.d.rt * a.d.rz * a.d.rx;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4u * q + j < nid) a.idx_out[4u * q + j] = (int)(((unsigned long long)r.w[j] * len) >> 32);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4u * q + j < nco) a.pc_out[4u * q + j] = (float)(r.w[j] >> 8) * 5.9604644775390625e-8f;   // 2^-24, exact
  }
}

// behind k_sampler_draw in stream order: every read of `offset` above has retired when this runs
__global__ void k_sampler_advance(stpde_sampler_state* st) {
  if (blockIdx.x == 0 && threadIdx.x == 0) st->offset = st->offset + 1ull;
}

// ---- produce ---------------------------------------------------------------------------------------------------------------
struct CropOrigin {
  int t0, z0, x0;
  bool clamped;
};
__device__ __forceinline__ CropOrigin crop_origin(const stpde_sampler_desc& d, int raw) {
  const int len = d.rt * d.rz * d.rx;
  const int id = raw < 0 ? 0 : (raw > len - 1 ? len - 1 : raw);   // BEFORE any address is formed
  CropOrigin o;
  o.t0 = id / (d.rz * d.rx);
  o.z0 = (id / d.rx) % d.rz;
  o.x0 = id % d.rx;
  o.clamped = id != raw;
  return o;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ f32x4 normalise(const stpde_sampler_desc& d, f32x4 v) {
  if (d.normalize) {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (v[c] - d.mean[c]) / d.std[c];
  }
  return v;
}

// first node of crop b: in the dataset at the (clamped) origin of its id, or crop b of the filtered scratch
template <bool CROP>
__device__ __forceinline__ const float* crop_base(const SamplerArgs& a, int b, size_t sZ, size_t sT, bool count) {
  if (CROP) return a.data + (size_t)b * a.d.nt * sT;
  const CropOrigin o = crop_origin(a.d, a.idx[b]);
  if (count && o.clamped) atomicAdd(&a.st->oob, 1u);
  return a.data + (size_t)o.t0 * sT + (size_t)o.z0 * sZ + (size_t)o.x0 * 4;
}

// CROP = false: a.data is the dataset [T][Z][X][4], read in place at the crop origin of a.idx[b] (clamped and counted here).
// CROP = true:  a.data is the filtered scratch [B][nt][nz][nx][4]: origin 0 of crop b, crop strides; a.idx is not read (the
//               first filter pass has clamped and counted the ids), so every address comes from b < B and clamped taps alone.
template <bool CROP>
__device__ __forceinline__ void sampler_produce(const SamplerArgs& a) {
  const stpde_sampler_desc& d = a.d;
  const size_t sZ = (size_t)(CROP ? d.nx : d.X) * 4, sT = (size_t)(CROP ? d.nz : d.Z) * sZ;      // strides of z and t in floats
  if (blockIdx.x < a.blocks_lres) {
    // low-resolution grid: voxel v = ((b * ntl + tl) * nzl + zl) * nxl + xl
    const int per = d.ntl * d.nzl * d.nxl;
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= (long)d.B * per) return;
    const int b = (int)(v / per), r = (int)(v % per);
    const int xl = r % d.nxl, zl = (r / d.nxl) % d.nzl, tl = r / (d.nxl * d.nzl);
    const float* base = crop_base<CROP>(a, b, sZ, sT, r == 0);
    const stpde_sampler_tap tt = a.tap[0][tl], tz = a.tap[1][zl], tx = a.tap[2][xl];
    f32x4 val;
    if (d.interp == 0) {
      const int it = clampi(tt.i0, 0, d.nt - 2), iz = clampi(tz.i0, 0, d.nz - 2), ix = clampi(tx.i0, 0, d.nx - 2);
      const float* p = base + (size_t)it * sT + (size_t)iz * sZ + (size_t)ix * 4;
      f32x4 s[2];
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        f32x4 u[2];
#pragma unroll
        for (int dz = 0; dz < 2; ++dz) {
          const f32x4 lo = ld4(p + dz * sZ + dx * 4), hi = ld4(p + sT + dz * sZ + dx * 4);
          u[dz] = lo + (hi - lo) * tt.w;             // stage t
        }
        s[dx] = u[0] + (u[1] - u[0]) * tz.w;         // stage z
      }
      val = s[0] + (s[1] - s[0]) * tx.w;             // stage x
    } else {
      const int it = clampi(tt.i0, 0, d.nt - 1), iz = clampi(tz.i0, 0, d.nz - 1), ix = clampi(tx.i0, 0, d.nx - 1);
      val = ld4(base + (size_t)it * sT + (size_t)iz * sZ + (size_t)ix * 4);
    }
    val = normalise(d, val);
    float* out = a.lres + (size_t)b * 4 * per + r;
#pragma unroll
    for (int c = 0; c < 4; ++c) out[(size_t)c * per] = val[c];
    return;
  }
  // point targets: one thread per query point
  const long p = (long)(blockIdx.x - a.blocks_lres) * 256 + threadIdx.x;
  if (p >= (long)d.B * d.N) return;
  const int b = (int)(p / d.N);
  const float* base = crop_base<CROP>(a, b, sZ, sT, false);
  const int n[3] = {d.nt, d.nz, d.nx};
  const size_t stride[3] = {sT, sZ, 4};
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = a.pc[(size_t)p * 3 + k] * (float)(n[k] - 1);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (d.interp == 0) {
    GeomN gm;
#pragma unroll
    for (int k = 0; k < 3; ++k) geom_axis(gm, k, q[k], d.lo_c[k], d.hi_c[k], d.cube[k], n[k]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      size_t node = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) node += (size_t)(gm.i0[k] + corner_bit(j, 3, k)) * stride[k];
      const f32x4 v = ld4(base + node);
      acc += v * corner_weight(gm, j, 3);
    }
  } else {
    size_t node = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float fi = fminf(fmaxf(floorf(q[k]), 0.f), (float)(n[k] - 2));
      const int i = (int)fi;
      node += (size_t)clampi(q[k] - fi <= 0.5f ? i : i + 1, 0, n[k] - 1) * stride[k];
    }
    acc = ld4(base + node);
  }
  st4(a.pv + (size_t)p * 4, normalise(d, acc));
}

__global__ __launch_bounds__(256) void k_sampler_produce(SamplerArgs a) { sampler_produce<false>(a); }
__global__ __launch_bounds__(256) void k_sampler_produce_crop(SamplerArgs a) { sampler_produce<true>(a); }

static int check_sampler(const stpde_sampler_desc* d, const char* who) {
  if (!d) {
    stpde_set_error("%s: null descriptor", who);
    return STPDE_E_BADARG;
  }
  if (d->B <= 0 || d->N <= 0) {
    stpde_set_error("%s: B and N must be positive (B %d, N %d)", who, d->B, d->N);
    return STPDE_E_BADARG;
  }
  if ((long)d->B * d->N * 3 >= (1l << 31)) {
    stpde_set_error("%s: B * N * 3 must be below 2^31", who);
    return STPDE_E_BADARG;
  }
  if (d->T < 1 || d->Z < 1 || d->X < 1 || d->nt > d->T || d->nz > d->Z || d->nx > d->X) {
    stpde_set_error("%s: crop (%d, %d, %d) larger than the dataset (%d, %d, %d)", who, d->nt, d->nz, d->nx, d->T, d->Z, d->X);
    return STPDE_E_BADARG;
  }
  if (d->nt < 2 || d->nz < 2 || d->nx < 2) {
    stpde_set_error("%s: crop needs >= 2 nodes per axis", who);
    return STPDE_E_BADARG;
  }
  if (d->ntl < 1 || d->nzl < 1 || d->nxl < 1 || d->nt % d->ntl || d->nz % d->nzl || d->nx % d->nxl) {
    stpde_set_error("%s: low-res extents (%d, %d, %d) must divide the crop (%d, %d, %d)", who, d->ntl, d->nzl, d->nxl, d->nt,
                    d->nz, d->nx);
    return STPDE_E_BADARG;
  }
  if (d->rt != d->T - d->nt + 1 || d->rz != d->Z - d->nz + 1 || d->rx != d->X - d->nx + 1) {
    stpde_set_error("%s: ranges (%d, %d, %d) inconsistent with the extents (dataset - crop + 1)", who, d->rt, d->rz, d->rx);
    return STPDE_E_BADARG;
  }
  if ((long)d->rt * d->rz * d->rx >= (1l << 31)) {
    stpde_set_error("%s: len = %ld crop positions, must be below 2^31", who, (long)d->rt * d->rz * d->rx);
    return STPDE_E_BADARG;
  }
  if (d->interp != 0 && d->interp != 1) {
    stpde_set_error("%s: interp must be 0 (linear) or 1 (nearest), got %d", who, d->interp);
    return STPDE_E_BADARG;
  }
  if (d->normalize != 0 && d->normalize != 1) {
    stpde_set_error("%s: normalize must be 0 or 1, got %d", who, d->normalize);
    return STPDE_E_BADARG;
  }
  if (d->normalize)
    for (int c = 0; c < 4; ++c)
      if (d->std[c] == 0.f) {
        stpde_set_error("%s: normalize with a zero std (channel %d)", who, c);
        return STPDE_E_BADARG;
      }
  return STPDE_OK;
}

extern "C" int stpde_sampler_draw(const stpde_sampler_desc* d, stpde_sampler_state* state_dev, int* crop_idx_out,
                                  float* point_coord_out, void* stream) {
  int rc = check_sampler(d, "sampler_draw");
  if (rc) return rc;
  if (!state_dev || !crop_idx_out || !point_coord_out) {
    stpde_set_error("sampler_draw: null pointer");
    return STPDE_E_BADARG;
  }
  SamplerArgs a{};
  a.d = *d;
  a.st = state_dev;
  a.idx_out = crop_idx_out;
  a.pc_out = point_coord_out;
  const unsigned calls = ((unsigned)d->B + 3u) / 4u + ((unsigned)d->B * (unsigned)d->N * 3u + 3u) / 4u;
  STPDE_LAUNCH(k_sampler_draw, dim3((calls + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  rc = stpde_check_launch("k_sampler_draw");
  if (rc) return rc;
  STPDE_LAUNCH(k_sampler_advance, dim3(1), dim3(64), 0, (hipStream_t)stream, state_dev);
  return stpde_check_launch("k_sampler_advance");
}

extern "C" int stpde_sampler_produce(const stpde_sampler_desc* d, stpde_sampler_state* state_dev, const float* data_cl,
                                     const stpde_sampler_tap* taps_t, const stpde_sampler_tap* taps_z,
                                     const stpde_sampler_tap* taps_x, const int* crop_idx, const float* point_coord,
                                     float* lres_out, float* point_value_out, void* stream) {
  int rc = check_sampler(d, "sampler_produce");
  if (rc) return rc;
  if (!state_dev || !data_cl || !taps_t || !taps_z || !taps_x || !crop_idx || !point_coord || !lres_out || !point_value_out) {
    stpde_set_error("sampler_produce: null pointer");
    return STPDE_E_BADARG;
  }
  if (((size_t)data_cl | (size_t)point_value_out) & 15) {
    stpde_set_error("sampler_produce: data_cl and point_value_out must be 16-byte aligned");
    return STPDE_E_BADARG;
  }
  SamplerArgs a{};
  a.d = *d;
  a.st = state_dev;
  a.data = data_cl;
  a.tap[0] = taps_t;
  a.tap[1] = taps_z;
  a.tap[2] = taps_x;
  a.idx = crop_idx;
  a.pc = point_coord;
  a.lres = lres_out;
  a.pv = point_value_out;
  const long voxels = (long)d->B * d->ntl * d->nzl * d->nxl, points = (long)d->B * d->N;
  if (voxels >= (1l << 31)) {
    stpde_set_error("sampler_produce: B * ntl * nzl * nxl must be below 2^31");
    return STPDE_E_BADARG;
  }
  a.blocks_lres = (unsigned)((voxels + 255) / 256);
  const unsigned blocks = a.blocks_lres + (unsigned)((points + 255) / 256);
  STPDE_LAUNCH(k_sampler_produce, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_sampler_produce");
}

// ---- filter passes -----------------------------------------------------------------------------------------------------------
// The low-res pre-filters of RB2DeviceLoader.get() (dataloader_spacetime.lres_filter) on the high-res crop, bit for bit: up to
// three 1-D passes, t then z then x, each reading the fp32 result of the one before.  An axis of radius 0 is skipped (never
// run with one tap).  Boundary: scipy's 'reflect' at the CROP faces (d c b a | a b c d | d c b a, period 2n).
//   weighted (gaussian, uniform):  acc = +0.0f; for k in 0 .. 2r: acc = acc + w[k] * x[reflect(i - r + k)] -- a multiply and an
//                                  add per tap, in this order (-ffp-contract=off): what `out + w[k] * xp.narrow(dim, k, n)` does
//   maximum:                       the first tap, then m = (v > m || v != v) ? v : m per channel: a NaN tap makes m NaN and no later
//                                  tap replaces it (v > NaN is false), as torch.amax; r = 0 copies the node bit for bit
// One thread per (crop voxel, 4 channels): 2r + 1 16-byte loads along the axis, one 16-byte store.  HBM/L2-bound, no MFMA.
//
// Addresses.  The grid is derived from B * nt * nz * nx alone (< 2^31, checked on the host) and every index is bounded for
// EVERY content of crop_idx and of the data:
//   crop_idx  b = v / (nt nz nx) < B
//   origin    FIRST pass only: id clamped into [0, len) by crop_origin() BEFORE (t0, z0, x0) are formed, so t0 + nt <= T,
//             z0 + nz <= Z, x0 + nx <= X; a clamped id is counted in state->oob by the thread of voxel 0 of its crop.  Later
//             passes read scratch crop b at origin 0 and never look at crop_idx.
//   tap       m = (i - r) mod 2n taken into [0, 2n) (i < n, r <= 2^20: no integer overflow), then stepped with wrap-around;
//             j = m < n ? m : 2n - 1 - m is in [0, n) for any r (r >= n and r > 2n included) -> the node read is inside the crop,
//             hence inside the dataset (FIRST) or inside scratch crop b.  Dataset values outside the crop are never read.
//   w         k in [0, 2r] with the table length 2r + 1 checked against the descriptor on the host
//   dst       v * 4 + c < B * nt * nz * nx * 4: the scratch crops hold exactly that
struct FilterArgs {
  stpde_sampler_filter_desc d;
  stpde_sampler_state* st;
  const float* src;   // FIRST: data_cl [T][Z][X][4]; else a scratch crop [B][nt][nz][nx][4]
  const int* idx;     // FIRST only
  const float* w;     // weighted passes only: 2r + 1 weights
  float* dst;         // the other scratch crop
  int axis, r;
};

template <bool MAX, bool FIRST>
__global__ __launch_bounds__(256) void k_sampler_filter_pass(FilterArgs a) {
  const stpde_sampler_filter_desc& d = a.d;
  const int per = d.nt * d.nz * d.nx;
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= (long)d.B * per) return;
  const int b = (int)(v / per), rem = (int)(v % per);
  const int x = rem % d.nx, z = (rem / d.nx) % d.nz, t = rem / (d.nx * d.nz);
  const size_t sZ = (size_t)(FIRST ? d.X : d.nx) * 4, sT = (size_t)(FIRST ? d.Z : d.nz) * sZ;
  const float* base;
  if (FIRST) {
    const int len = d.rt * d.rz * d.rx, raw = a.idx[b];
    const int id = raw < 0 ? 0 : (raw > len - 1 ? len - 1 : raw);   // BEFORE any address is formed
    if (rem == 0 && id != raw) atomicAdd(&a.st->oob, 1u);
    base = a.src + (size_t)(id / (d.rz * d.rx)) * sT + (size_t)((id / d.rx) % d.rz) * sZ + (size_t)(id % d.rx) * 4;
  } else {
    base = a.src + (size_t)b * per * 4;
  }
  // the line of this voxel along the filtered axis: its node 0, the stride between nodes, its length and the voxel's place in it
  const int i = a.axis == 0 ? t : (a.axis == 1 ? z : x), n = a.axis == 0 ? d.nt : (a.axis == 1 ? d.nz : d.nx);
  const size_t sA = a.axis == 0 ? sT : (a.axis == 1 ? sZ : 4);
  const float* line = base + (a.axis == 0 ? 0 : (size_t)t * sT) + (a.axis == 1 ? 0 : (size_t)z * sZ) + (a.axis == 2 ? 0 : (size_t)x * 4);
  const int n2 = 2 * n;
  int m = (i - a.r) % n2;                                           // place of the first tap in the mirrored period
  if (m < 0) m += n2;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k <= 2 * a.r; ++k) {
    const int j = m < n ? m : n2 - 1 - m;                           // in [0, n)
    const f32x4 u = ld4(line + (size_t)j * sA);
    if (MAX) {
      if (k == 0) {
        acc = u;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = (u[c] > acc[c] || u[c] != u[c]) ? u[c] : acc[c];
      }
    } else {
      acc = acc + u * a.w[k];
    }
    m = m + 1 == n2 ? 0 : m + 1;
  }
  st4(a.dst + (size_t)v * 4, acc);
}

template <bool MAX, bool FIRST>
static int launch_filter_pass(const FilterArgs& a, hipStream_t stream) {
  const long voxels = (long)a.d.B * a.d.nt * a.d.nz * a.d.nx;
  STPDE_LAUNCH((k_sampler_filter_pass<MAX, FIRST>), dim3((unsigned)((voxels + 255) / 256)), dim3(256), 0, stream, a);
  return stpde_check_launch("k_sampler_filter_pass");
}

#define STPDE_FILTER_MAX_RADIUS (1 << 20)

extern "C" int stpde_sampler_filter(const stpde_sampler_filter_desc* d, stpde_sampler_state* state_dev, const float* data_cl,
                                    const int* crop_idx, const float* w_t, const float* w_z, const float* w_x, float* scratch_a,
                                    float* scratch_b, void* stream) {
  const char* who = "sampler_filter";
  if (!d) {
    stpde_set_error("%s: null descriptor", who);
    return STPDE_E_BADARG;
  }
  if (d->B <= 0) {
    stpde_set_error("%s: B must be positive (B %d)", who, d->B);
    return STPDE_E_BADARG;
  }
  if (d->T < 1 || d->Z < 1 || d->X < 1 || d->nt > d->T || d->nz > d->Z || d->nx > d->X) {
    stpde_set_error("%s: crop (%d, %d, %d) larger than the dataset (%d, %d, %d)", who, d->nt, d->nz, d->nx, d->T, d->Z, d->X);
    return STPDE_E_BADARG;
  }
  if (d->nt < 2 || d->nz < 2 || d->nx < 2) {
    stpde_set_error("%s: crop needs >= 2 nodes per axis", who);
    return STPDE_E_BADARG;
  }
  if (d->rt != d->T - d->nt + 1 || d->rz != d->Z - d->nz + 1 || d->rx != d->X - d->nx + 1) {
    stpde_set_error("%s: ranges (%d, %d, %d) inconsistent with the extents (dataset - crop + 1)", who, d->rt, d->rz, d->rx);
    return STPDE_E_BADARG;
  }
  if ((long)d->rt * d->rz * d->rx >= (1l << 31)) {
    stpde_set_error("%s: len = %ld crop positions, must be below 2^31", who, (long)d->rt * d->rz * d->rx);
    return STPDE_E_BADARG;
  }
  if ((long)d->B * d->nt * d->nz * d->nx >= (1l << 31)) {
    stpde_set_error("%s: B * nt * nz * nx must be below 2^31", who);
    return STPDE_E_BADARG;
  }
  if (d->kind != STPDE_FILTER_GAUSSIAN && d->kind != STPDE_FILTER_UNIFORM && d->kind != STPDE_FILTER_MAXIMUM) {
    stpde_set_error("%s: kind must be 1 (gaussian), 2 (uniform) or 3 (maximum), got %d (median, 4, is stpde_sampler_median's)", who, d->kind);
    return STPDE_E_BADARG;
  }
  const bool weighted = d->kind != STPDE_FILTER_MAXIMUM;
  const float* w[3] = {w_t, w_z, w_x};
  for (int k = 0; k < 3; ++k) {
    if (d->r[k] < 0 || d->r[k] > STPDE_FILTER_MAX_RADIUS) {
      stpde_set_error("%s: radius %d of axis %d outside [0, 2^20]", who, d->r[k], k);
      return STPDE_E_BADARG;
    }
    const int want = weighted && d->r[k] ? 2 * d->r[k] + 1 : 0;
    if (d->nw[k] != want) {
      stpde_set_error("%s: radius %d of axis %d does not match its table of %d weights (%d expected)", who, d->r[k], k, d->nw[k],
                      want);
      return STPDE_E_BADARG;
    }
    if (want && !w[k]) {
      stpde_set_error("%s: null pointer (weights of axis %d)", who, k);
      return STPDE_E_BADARG;
    }
  }
  if (!state_dev || !data_cl || !crop_idx || !scratch_a || !scratch_b) {
    stpde_set_error("%s: null pointer", who);
    return STPDE_E_BADARG;
  }
  if (((size_t)data_cl | (size_t)scratch_a | (size_t)scratch_b) & 15) {
    stpde_set_error("%s: data_cl and the scratch crops must be 16-byte aligned", who);
    return STPDE_E_BADARG;
  }
  if (scratch_a == scratch_b) {
    stpde_set_error("%s: the two scratch crops must be different buffers", who);
    return STPDE_E_BADARG;
  }
  FilterArgs a{};
  a.d = *d;
  a.st = state_dev;
  a.idx = crop_idx;
  int axes[3], np = 0;
  for (int k = 0; k < 3; ++k)
    if (d->r[k]) axes[np++] = k;
  if (np == 0) {                                    // every axis skipped: a plain copy of the crops (maximum of one tap)
    a.src = data_cl;
    a.dst = scratch_a;
    return launch_filter_pass<true, true>(a, (hipStream_t)stream);
  }
  const float* src = data_cl;
  for (int p = 0; p < np; ++p) {                    // the last pass writes scratch_a
    a.axis = axes[p];
    a.r = d->r[a.axis];
    a.w = w[a.axis];
    a.src = src;
    a.dst = (np - 1 - p) % 2 == 0 ? scratch_a : scratch_b;
    int rc;
    if (weighted)
      rc = p == 0 ? launch_filter_pass<false, true>(a, (hipStream_t)stream) : launch_filter_pass<false, false>(a, (hipStream_t)stream);
    else
      rc = p == 0 ? launch_filter_pass<true, true>(a, (hipStream_t)stream) : launch_filter_pass<true, false>(a, (hipStream_t)stream);
    if (rc) return rc;
    src = a.dst;
  }
  return STPDE_OK;
}

extern "C" int stpde_sampler_produce_filtered(const stpde_sampler_desc* d, const float* crops, const stpde_sampler_tap* taps_t,
                                              const stpde_sampler_tap* taps_z, const stpde_sampler_tap* taps_x,
                                              const float* point_coord, float* lres_out, float* point_value_out, void* stream) {
  int rc = check_sampler(d, "sampler_produce_filtered");
  if (rc) return rc;
  if (!crops || !taps_t || !taps_z || !taps_x || !point_coord || !lres_out || !point_value_out) {
    stpde_set_error("sampler_produce_filtered: null pointer");
    return STPDE_E_BADARG;
  }
  if (((size_t)crops | (size_t)point_value_out) & 15) {
    stpde_set_error("sampler_produce_filtered: crops and point_value_out must be 16-byte aligned");
    return STPDE_E_BADARG;
  }
  SamplerArgs a{};
  a.d = *d;
  a.data = crops;
  a.tap[0] = taps_t;
  a.tap[1] = taps_z;
  a.tap[2] = taps_x;
  a.pc = point_coord;
  a.lres = lres_out;
  a.pv = point_value_out;
  const long voxels = (long)d->B * d->ntl * d->nzl * d->nxl, points = (long)d->B * d->N;
  if ((long)d->B * d->nt * d->nz * d->nx >= (1l << 31)) {
    stpde_set_error("sampler_produce_filtered: B * nt * nz * nx must be below 2^31");
    return STPDE_E_BADARG;
  }
  a.blocks_lres = (unsigned)((voxels + 255) / 256);
  const unsigned blocks = a.blocks_lres + (unsigned)((points + 255) / 256);
  STPDE_LAUNCH(k_sampler_produce_crop, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_sampler_produce_crop");
}
