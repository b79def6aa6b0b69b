// The median low-res pre-filter of the device batch sampler (include/stpde_hip.h, "N3 on the device, median"): what
// RB2DeviceLoader.get() does with lres_filter(..., 'median') -- unfold every voxel's (2 r_t + 1)(2 r_z + 1)(2 r_x + 1) window and
// torch.median over it -- as ONE selection kernel over the high-res crops.  The output has the layout of the scratch crops of
// csrc/sampler.hip, so stpde_sampler_produce_filtered interpolates both outputs from it.  Not separable, so no 1-D passes.
//
// One workgroup of 256 threads owns a 4 x 8 x 8 tile of output voxels (t, z, x; one voxel per thread, a wave per t plane) and
// stages the tile plus its halo into LDS with the reflection at the crop faces already resolved: a node is one 16-byte slot of
// four order-preserving 32-bit keys (bits ^ (sign ? 0xFFFFFFFF : 0x80000000); every NaN becomes the largest key, 0xFFFFFFFF,
// which no number has).  Each thread then finds the key of rank (W - 1) / 2 of its window per channel:
//   a first walk over the window takes the smallest and the largest key.  A largest key of 0xFFFFFFFF is a NaN in the window: the
//   channel's result is a quiet NaN, as torch.median gives.  The bits above the highest bit in which the smallest and the largest
//   key of any channel differ are common to the whole window, so they are the answer's already;
//   the bits below are fixed MSB first, one per walk: cand = prefix | bit, cnt = number of keys < cand, and the answer has the bit
//   set iff cnt <= rank.  After the last bit the prefix IS the key of that rank (the largest v with #{keys < v} <= rank).
// A walk is W 16-byte LDS reads and W x 4 compare-and-count pairs per thread; no sort, no per-thread array, no scratch memory.
// Zeros keep their sign as two neighbouring keys, so a window whose middle falls among zeros gives the zero of that rank
// (torch.median does not pin which; they compare equal).
//
// LDS image: [4 + 2 r_t][8 + 2 r_z][S] slots, S = 8 when r_x = 0, else 24: the smallest row stride >= 8 + 2 r_x that is 8 mod 16,
// so that the four z rows a 16-lane group of a 16-byte LDS read touches fall into four different quarters of the 64 banks.
// Largest at r = (7, 7, 7): 18 * 22 * 24 * 16 B = 152,064 B of the 160 KiB of a CU (dynamic LDS, raised once per device).
//
// Addresses.  The grid is derived from B and the crop extents alone (blocks = B * ceil(nt/4) * ceil(nz/8) * ceil(nx/8), below
// 2^24, checked on the host) and every index is bounded for EVERY content of crop_idx and of the data:
//   crop      b = block / tiles-per-crop < B
//   origin    id clamped into [0, len) BEFORE (t0, z0, x0) are formed, so t0 + nt <= T, z0 + nz <= Z, x0 + nx <= X; a clamped id is
//             counted once in state->oob, by thread 0 of tile 0 of its crop
//   tap       staged node i of an axis is crop node reflect(o + i - r), o the tile origin (< n), i < tile + 2r <= 22, r <= 7:
//             m = (o + i - r) mod 2n taken into [0, 2n), j = m < n ? m : 2n - 1 - m in [0, n) for any r (r >= n and r > 2n
//             included) -- the index formula of k_sampler_filter_pass.  The node read is inside the crop, hence inside the dataset;
//             dataset values outside the crop are never read
//   LDS       staging writes slot (it * hz + iz) * S + ix with it < ht, iz < hz, ix < 8 + 2 r_x <= S; a walk reads
//             ((lt + dt) * hz + lz + dz) * S + lx + dx with lt + dt < 4 + 2 r_t = ht, lz + dz < hz, lx + dx < 8 + 2 r_x:
//             exactly the slots that were staged, all below ht * hz * S = the dynamic LDS size of the launch
//   dst       only threads whose voxel is inside the crop write, at ((b * nt + t) * nz + z) * nx + x: crops_out holds exactly that
// Apart from the oob count there are no atomics: the result is the same every run.
#include "interp_geom.h"

#define MED_TT 4
#define MED_TZ 8
#define MED_TX 8
#define STPDE_FILTER_MEDIAN_MAX_RADIUS 7

struct MedianArgs {
  stpde_sampler_filter_desc d;
  stpde_sampler_state* st;
  const float* src;   // data_cl [T][Z][X][4]
  const int* idx;
  float* dst;         // [B][nt][nz][nx][4]
  int tiles_t, tiles_z, tiles_x;
  int hz, S;          // rows per plane and slots per row of the LDS image
};

__device__ __forceinline__ int reflect_fold(int i, int n) {
  const int n2 = 2 * n;
  int m = i % n2;
  if (m < 0) m += n2;
  return m < n ? m : n2 - 1 - m;                                    // in [0, n)
}

__device__ __forceinline__ unsigned median_key(float v) {
  const unsigned u = __float_as_uint(v);
  return v != v ? 0xFFFFFFFFu : (u ^ ((u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u));
}

// WX = 2 r_x + 1 known at compile time (the row of a walk is unrolled), or 0: taken from the descriptor
template <int WX>
__global__ __launch_bounds__(256) void k_sampler_median(MedianArgs a) {
  extern __shared__ uint4 med_lds[];
  const stpde_sampler_filter_desc& d = a.d;
  const int rt = d.r[0], rz = d.r[1], rx = d.r[2];
  const int wt = 2 * rt + 1, wz = 2 * rz + 1, wx = WX ? WX : 2 * rx + 1;
  const int ht = MED_TT + 2 * rt, hz = a.hz, hx = MED_TX + 2 * rx, S = a.S;
  const int per = a.tiles_t * a.tiles_z * a.tiles_x;
  const int b = (int)(blockIdx.x / (unsigned)per), tile = (int)(blockIdx.x % (unsigned)per);
  const int ot = (tile / (a.tiles_z * a.tiles_x)) * MED_TT, oz = ((tile / a.tiles_x) % a.tiles_z) * MED_TZ,
            ox = (tile % a.tiles_x) * MED_TX;
  const size_t sZ = (size_t)d.X * 4, sT = (size_t)d.Z * sZ;
  const int len = d.rt * d.rz * d.rx, raw = a.idx[b];
  const int id = raw < 0 ? 0 : (raw > len - 1 ? len - 1 : raw);     // BEFORE any address is formed
  if (tile == 0 && threadIdx.x == 0 && id != raw) atomicAdd(&a.st->oob, 1u);
  const float* base = a.src + (size_t)(id / (d.rz * d.rx)) * sT + (size_t)((id / d.rx) % d.rz) * sZ + (size_t)(id % d.rx) * 4;

  // stage tile + halo, reflection resolved
  const int nodes = ht * hz * hx;
  for (int s = (int)threadIdx.x; s < nodes; s += 256) {
    const int ix = s % hx, iz = (s / hx) % hz, it = s / (hx * hz);
    const int t = reflect_fold(ot + it - rt, d.nt), z = reflect_fold(oz + iz - rz, d.nz), x = reflect_fold(ox + ix - rx, d.nx);
    const f32x4 v = ld4(base + (size_t)t * sT + (size_t)z * sZ + (size_t)x * 4);
    med_lds[(it * hz + iz) * S + ix] = make_uint4(median_key(v[0]), median_key(v[1]), median_key(v[2]), median_key(v[3]));
  }
  __syncthreads();

  const int lx = (int)threadIdx.x % MED_TX, lz = ((int)threadIdx.x / MED_TX) % MED_TZ, lt = (int)threadIdx.x / (MED_TX * MED_TZ);
  const int t = ot + lt, z = oz + lz, x = ox + lx;
  if (t >= d.nt || z >= d.nz || x >= d.nx) return;                   // partial tile; no barrier below
  const uint4* win = med_lds + (lt * hz + lz) * S + lx;
  const int rows = wt * wz, plane = (hz - wz) * S;                   // step from the last row of a t plane to the next plane's first
  const unsigned rank = (unsigned)(wt * wz * wx - 1) / 2u;

  unsigned mn[4], mx[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    mn[c] = 0xFFFFFFFFu;
    mx[c] = 0u;
  }
  {
    const uint4* row = win;
    for (int j = 0, jz = 0; j < rows; ++j) {
#pragma unroll
      for (int k = 0; k < wx; ++k) {
        const uint4 q = row[k];
        mn[0] = min(mn[0], q.x);
        mx[0] = max(mx[0], q.x);
        mn[1] = min(mn[1], q.y);
        mx[1] = max(mx[1], q.y);
        mn[2] = min(mn[2], q.z);
        mx[2] = max(mx[2], q.z);
        mn[3] = min(mn[3], q.w);
        mx[3] = max(mx[3], q.w);
      }
      row += S;
      if (++jz == wz) {
        jz = 0;
        row += plane;
      }
    }
  }
  const unsigned diff = (mn[0] ^ mx[0]) | (mn[1] ^ mx[1]) | (mn[2] ^ mx[2]) | (mn[3] ^ mx[3]);
  const int hb = diff ? 32 - __clz((int)diff) : 0;                   // bits [hb, 32) are common to every key of a channel
  unsigned prefix[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) prefix[c] = (unsigned)(((unsigned long long)mx[c] >> hb) << hb);   // hb <= 32

  for (int bit = hb - 1; bit >= 0; --bit) {
    unsigned cand[4], cnt[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      cand[c] = prefix[c] | (1u << bit);
      cnt[c] = 0u;
    }
    const uint4* row = win;
    for (int j = 0, jz = 0; j < rows; ++j) {
#pragma unroll
      for (int k = 0; k < wx; ++k) {
        const uint4 q = row[k];
        cnt[0] += q.x < cand[0] ? 1u : 0u;
        cnt[1] += q.y < cand[1] ? 1u : 0u;
        cnt[2] += q.z < cand[2] ? 1u : 0u;
        cnt[3] += q.w < cand[3] ? 1u : 0u;
      }
      row += S;
      if (++jz == wz) {
        jz = 0;
        row += plane;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) prefix[c] = cnt[c] <= rank ? cand[c] : prefix[c];
  }

  f32x4 out;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const unsigned k = prefix[c];
    const unsigned u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    out[c] = mx[c] == 0xFFFFFFFFu ? __uint_as_float(0x7FC00000u) : __uint_as_float(u);
  }
  st4(a.dst + ((((size_t)b * d.nt + t) * d.nz + z) * d.nx + x) * 4, out);
}

template <int WX>
static int launch_median(const MedianArgs& a, unsigned blocks, size_t lds, hipStream_t stream) {
  if (lds > 64 * 1024) {
    // more dynamic LDS than the default limit of a launch: raised once per device (a host-side attribute, not a stream operation)
    static bool raised[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
      stpde_set_error("sampler_median: cannot tell the current device");
      return STPDE_E_LAUNCH;
    }
    if (!raised[dev]) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sampler_median<WX>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024) != hipSuccess) {
        (void)hipGetLastError();
        stpde_set_error("sampler_median: the device refuses %zu bytes of LDS per workgroup", lds);
        return STPDE_E_LAUNCH;
      }
      raised[dev] = true;
    }
  }
  STPDE_LAUNCH((k_sampler_median<WX>), dim3(blocks), dim3(256), lds, stream, a);
  return stpde_check_launch("k_sampler_median");
}

extern "C" int stpde_sampler_median(const stpde_sampler_filter_desc* d, stpde_sampler_state* state_dev, const float* data_cl,
                                    const int* crop_idx, float* crops_out, void* stream) {
  const char* who = "sampler_median";
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
  if (d->kind != STPDE_FILTER_MEDIAN) {
    stpde_set_error("%s: kind must be 4 (median), got %d (stpde_sampler_filter runs gaussian / uniform / maximum)", who, d->kind);
    return STPDE_E_BADARG;
  }
  for (int k = 0; k < 3; ++k) {
    if (d->r[k] < 0 || d->r[k] > STPDE_FILTER_MEDIAN_MAX_RADIUS) {
      stpde_set_error("%s: radius %d of axis %d outside [0, %d] (the tile and its halo must fit the LDS of one workgroup)", who,
                      d->r[k], k, STPDE_FILTER_MEDIAN_MAX_RADIUS);
      return STPDE_E_BADARG;
    }
    if (d->nw[k] != 0) {
      stpde_set_error("%s: the median takes no weight tables (nw[%d] = %d, 0 expected)", who, k, d->nw[k]);
      return STPDE_E_BADARG;
    }
  }
  if (!state_dev || !data_cl || !crop_idx || !crops_out) {
    stpde_set_error("%s: null pointer", who);
    return STPDE_E_BADARG;
  }
  if (((size_t)data_cl | (size_t)crops_out) & 15) {
    stpde_set_error("%s: data_cl and crops_out must be 16-byte aligned", who);
    return STPDE_E_BADARG;
  }
  MedianArgs a{};
  a.d = *d;
  a.st = state_dev;
  a.src = data_cl;
  a.idx = crop_idx;
  a.dst = crops_out;
  a.tiles_t = (d->nt + MED_TT - 1) / MED_TT;
  a.tiles_z = (d->nz + MED_TZ - 1) / MED_TZ;
  a.tiles_x = (d->nx + MED_TX - 1) / MED_TX;
  a.hz = MED_TZ + 2 * d->r[1];
  a.S = d->r[2] ? 24 : 8;                           // >= 8 + 2 r_x (r_x <= 7) and 8 mod 16
  // at most 256 tiles per voxel and voxels < 2^31: the product fits a long.  256 threads per block: the launch stays below 2^32 threads
  const long blocks = (long)d->B * a.tiles_t * a.tiles_z * a.tiles_x;
  if (blocks >= (1l << 24)) {
    stpde_set_error("%s: B * ceil(nt/4) * ceil(nz/8) * ceil(nx/8) = %ld tiles, must be below 2^24", who, blocks);
    return STPDE_E_BADARG;
  }
  const size_t lds = (size_t)(MED_TT + 2 * d->r[0]) * a.hz * a.S * sizeof(uint4);
  switch (2 * d->r[2] + 1) {
    case 1: return launch_median<1>(a, (unsigned)blocks, lds, (hipStream_t)stream);
    case 3: return launch_median<3>(a, (unsigned)blocks, lds, (hipStream_t)stream);
    case 7: return launch_median<7>(a, (unsigned)blocks, lds, (hipStream_t)stream);
    case 15: return launch_median<15>(a, (unsigned)blocks, lds, (hipStream_t)stream);
    default: return launch_median<0>(a, (unsigned)blocks, lds, (hipStream_t)stream);
  }
}
