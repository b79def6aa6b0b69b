// Training batches drawn and produced on the device (include/stpde_hip.h, "N3 on the device"): crop ids and query points from
// Philox4x32-10 with its state in device memory, then ONE gather kernel that writes the low-resolution input grid and the
// interpolated point targets straight from the channels-last dataset -- what RB2DeviceLoader.get() does with a host
// round trip, per-crop slicing, torch.rand, three index_select pairs, the interpolation kernel and two normalisations.
// HBM/L2-bound gather: one thread per low-res voxel / per query point, all 4 channels of a node as one 16-byte load; lanes run
// along x (low-res part: the four channel planes of the output are written 256 contiguous bytes per wave each).
// Built with -ffp-contract=off like the rest of the library: every expression below rounds where the torch stages and
// k_interp round (interp_geom.h is shared with it).
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

__global__ __launch_bounds__(256) void k_sampler_produce(SamplerArgs a) {
  const stpde_sampler_desc& d = a.d;
  const size_t sZ = (size_t)d.X * 4, sT = (size_t)d.Z * sZ;      // strides of z and t in floats
  if (blockIdx.x < a.blocks_lres) {
    // low-resolution grid: voxel v = ((b * ntl + tl) * nzl + zl) * nxl + xl
    const int per = d.ntl * d.nzl * d.nxl;
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= (long)d.B * per) return;
    const int b = (int)(v / per), r = (int)(v % per);
    const int xl = r % d.nxl, zl = (r / d.nxl) % d.nzl, tl = r / (d.nxl * d.nzl);
    const CropOrigin o = crop_origin(d, a.idx[b]);
    if (r == 0 && o.clamped) atomicAdd(&a.st->oob, 1u);
    const stpde_sampler_tap tt = a.tap[0][tl], tz = a.tap[1][zl], tx = a.tap[2][xl];
    f32x4 val;
    if (d.interp == 0) {
      const int it = clampi(tt.i0, 0, d.nt - 2), iz = clampi(tz.i0, 0, d.nz - 2), ix = clampi(tx.i0, 0, d.nx - 2);
      const float* p = a.data + (size_t)(o.t0 + it) * sT + (size_t)(o.z0 + iz) * sZ + (size_t)(o.x0 + ix) * 4;
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
      val = ld4(a.data + (size_t)(o.t0 + it) * sT + (size_t)(o.z0 + iz) * sZ + (size_t)(o.x0 + ix) * 4);
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
  const CropOrigin o = crop_origin(d, a.idx[b]);
  const float* base = a.data + (size_t)o.t0 * sT + (size_t)o.z0 * sZ + (size_t)o.x0 * 4;
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
