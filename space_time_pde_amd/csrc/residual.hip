// PDE residuals from the jet streams (the algebra of src/pde.py:115-143 after the derivatives are known):
// every equation of a PDELayer is compiled on the host into a straight-line SSA program over the jet atoms
// (y_c, dy_c/dq_d, d2y_c/dq_a dq_b or the combined second-order stream), the query coordinates and constants;
// one thread evaluates all equations of one query point (coalesced [stream][channel][point] reads), and the adjoint
// kernel replays the program and sweeps it backwards (the reverse-mode tape autograd would build from ~100 elementwise
// torch kernels per step).  Pure streaming work: ~S*n_out*4 B read and n_eq*4 B written per point.
#include "common.h"

#define RES_MAX STPDE_RES_MAX_INS

struct ResArgs {
  const stpde_res_ins* prog;   // device
  int nins, n_eq, n_out, P;
  const float* jets;           // [(s * n_out + c) * ld + p]
  long ld_s, ld_c;             // element strides of the stream and channel dimensions
  const float* x;              // [P][3] or null
  float* res;                  // [n_eq][P]
  const float* res_bar;        // [n_eq][P]
  float* jets_bar;             // same layout as jets, zero-filled by the caller
};

// base^n for an integer n: square-and-multiply on |n|, then 1 / r for n < 0.  POWI's value, the x^(n-1) of its adjoint and the
// integer part of POWC all take it, so the three stay the same sequence of IEEE multiplications.
__device__ __forceinline__ float res_ipow(float base, int n) {
  float r = 1.f;
  int e = n < 0 ? -n : n;
  while (e) {
    if (e & 1) r *= base;
    base *= base;
    e >>= 1;
  }
  return n < 0 ? 1.f / r : r;
}

// x^c for a real constant c = n + f, n = trunc(c): the integer part by res_ipow, the fraction through powf.  An integral c -- c = 1, or the c - 1 = 0 of its adjoint -- then costs no rounding of the math library
// (its powf(x, 1) is not x in every bit), and the result keeps pow's conventions: NaN for x < 0 unless f = 0, the sign of x for an
// odd integral c, +0 / +Inf at x = -0 otherwise (hence |x| under the integer part when f != 0).
__device__ __forceinline__ float res_powc(float x, float c) {
  const float n = truncf(c), f = c - n;
  if (fabsf(n) > 64.f) return powf(x, c);
  const float r = res_ipow(f != 0.f ? fabsf(x) : x, (int)n);
  return f != 0.f ? r * powf(x, f) : r;
}

// The opcodes appended after OUT.  They are kept out of the switch of the first 17 (one comparison in front of it instead of
// twenty-two more cases in it): the programs of the equations that compiled before hold none of them.
__device__ __forceinline__ float res_eval_ext(const stpde_res_ins& in, const float* v) {
  switch (in.op) {
    case STPDE_RES_TAN: return tanf(v[in.a]);
    case STPDE_RES_SINH: return sinhf(v[in.a]);
    case STPDE_RES_COSH: return coshf(v[in.a]);
    case STPDE_RES_ASIN: return asinf(v[in.a]);
    case STPDE_RES_ACOS: return acosf(v[in.a]);
    case STPDE_RES_ATAN: return atanf(v[in.a]);
    case STPDE_RES_ATAN2: return atan2f(v[in.a], v[in.b]);
    case STPDE_RES_POWC: return res_powc(v[in.a], in.c);
    case STPDE_RES_POW: return powf(v[in.a], v[in.b]);
    // MIN MAX SIGN STEP: comparisons and selects only; every comparison is false for NaN, which the last operand then carries
    case STPDE_RES_MIN: { const float x = v[in.a], y = v[in.b]; return (x < y || x != x) ? x : y; }
    case STPDE_RES_MAX: { const float x = v[in.a], y = v[in.b]; return (x > y || x != x) ? x : y; }
    case STPDE_RES_SIGN: { const float x = v[in.a]; return x > 0.f ? 1.f : (x < 0.f ? -1.f : (x == 0.f ? 0.f : x)); }
    case STPDE_RES_STEP: { const float x = v[in.a]; return x > 0.f ? 1.f : (x < 0.f ? 0.f : (x == 0.f ? 0.5f : x)); }
    // Masks, 1.0 or 0.0 and never NaN: IEEE comparisons (a NaN operand gives false, true for NE); AND OR NOT read a mask as != 0
    case STPDE_RES_LT: return v[in.a] < v[in.b] ? 1.f : 0.f;
    case STPDE_RES_LE: return v[in.a] <= v[in.b] ? 1.f : 0.f;
    case STPDE_RES_EQ: return v[in.a] == v[in.b] ? 1.f : 0.f;
    case STPDE_RES_NE: return v[in.a] != v[in.b] ? 1.f : 0.f;
    case STPDE_RES_AND: return (v[in.a] != 0.f && v[in.b] != 0.f) ? 1.f : 0.f;
    case STPDE_RES_OR: return (v[in.a] != 0.f || v[in.b] != 0.f) ? 1.f : 0.f;
    case STPDE_RES_NOT: return v[in.a] != 0.f ? 0.f : 1.f;
    case STPDE_RES_SEL: return v[in.a] != 0.f ? v[STPDE_RES_SEL_THEN(in.b)] : v[STPDE_RES_SEL_ELSE(in.b)];
    case STPDE_RES_STEPC: { const float x = v[in.a]; return x > 0.f ? 1.f : (x < 0.f ? 0.f : (x == 0.f ? in.c : x)); }
    default: return v[in.a];
  }
}

// COEF: a CONST with b != 0 is late-bound -- the value of coefficient a, staged per block in coef (k_residual_coef_*); without
// the flag every CONST is its c, whatever b holds (the programs of k_residual_fwd / _bwd carry b = 0).
template <bool COEF>
__device__ __forceinline__ float res_eval(const stpde_res_ins& in, const float* v, const ResArgs& a, int p, const float* coef) {
  if (in.op > STPDE_RES_OUT) return res_eval_ext(in, v);
  switch (in.op) {
    case STPDE_RES_JET: return a.jets[(size_t)in.a * a.ld_s + (size_t)in.b * a.ld_c + p];
    case STPDE_RES_X: return a.x[(size_t)p * 3 + in.a];
    case STPDE_RES_CONST: return (COEF && in.b != 0) ? coef[in.a & (STPDE_RES_MAX_COEF - 1)] : in.c;
    case STPDE_RES_ADD: return v[in.a] + v[in.b];
    case STPDE_RES_SUB: return v[in.a] - v[in.b];
    case STPDE_RES_MUL: return v[in.a] * v[in.b];
    case STPDE_RES_DIV: return v[in.a] / v[in.b];
    case STPDE_RES_NEG: return -v[in.a];
    case STPDE_RES_POWI: return res_ipow(v[in.a], in.b);
    case STPDE_RES_SIN: return sinf(v[in.a]);
    case STPDE_RES_COS: return cosf(v[in.a]);
    case STPDE_RES_EXP: return expf(v[in.a]);
    case STPDE_RES_LOG: return logf(v[in.a]);
    case STPDE_RES_SQRT: return sqrtf(v[in.a]);
    case STPDE_RES_TANH: return tanhf(v[in.a]);
    case STPDE_RES_ABS: return fabsf(v[in.a]);
    default: return v[in.a];   // STPDE_RES_OUT: residual b = value a
  }
}

__global__ __launch_bounds__(256) void k_residual_fwd(ResArgs a) {
  __shared__ stpde_res_ins prog[RES_MAX];
  for (int i = threadIdx.x; i < a.nins; i += 256) prog[i] = a.prog[i];
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.P) return;
  float v[RES_MAX];
  for (int i = 0; i < a.nins; ++i) {
    const stpde_res_ins in = prog[i];
    v[i] = res_eval<false>(in, v, a, p, nullptr);
    if (in.op == STPDE_RES_OUT) a.res[(size_t)in.b * a.P + p] = v[i];
  }
}

// Reverse rules of the appended opcodes (instruction i, its adjoint gi).
__device__ __forceinline__ void res_bwd_ext(const stpde_res_ins& in, int i, const float* v, float* g, float gi) {
  switch (in.op) {
    case STPDE_RES_TAN: g[in.a] += gi * (1.f + v[i] * v[i]); break;
    case STPDE_RES_SINH: g[in.a] += gi * coshf(v[in.a]); break;
    case STPDE_RES_COSH: g[in.a] += gi * sinhf(v[in.a]); break;
    case STPDE_RES_ASIN: g[in.a] += gi / sqrtf(1.f - v[in.a] * v[in.a]); break;
    case STPDE_RES_ACOS: g[in.a] -= gi / sqrtf(1.f - v[in.a] * v[in.a]); break;
    case STPDE_RES_ATAN: g[in.a] += gi / (1.f + v[in.a] * v[in.a]); break;
    case STPDE_RES_ATAN2: {
      const float x = v[in.a], y = v[in.b], d = x * x + y * y;
      const bool origin = x == 0.f && y == 0.f;      // torch: no gradient there
      g[in.a] += origin ? 0.f : gi * y / d;
      g[in.b] -= origin ? 0.f : gi * x / d;
      break;
    }
    case STPDE_RES_POWC: {   // c x^(c-1) without dividing by x; c - 1 is taken in double like torch's scalar exponent
      if (in.c != 0.f) g[in.a] += gi * (in.c * res_powc(v[in.a], (float)((double)in.c - 1.0)));
      break;
    }
    case STPDE_RES_POW: {    // torch.pow: nothing into the base where y == 0, nothing into the exponent where x == 0 and y >= 0
      const float x = v[in.a], y = v[in.b];
      const float gx = y == 0.f ? 0.f : gi * (y * powf(x, y - 1.f));
      const float gy = gi * ((x == 0.f && y >= 0.f) ? 0.f : v[i] * logf(x));
      g[in.a] += gx;
      g[in.b] += gy;
      break;
    }
    case STPDE_RES_MIN: {    // torch.minimum: the smaller operand takes the cotangent, a tie halves it, NaN passes it to both
      const float x = v[in.a], y = v[in.b], h = x == y ? gi * 0.5f : gi;
      g[in.a] += x > y ? 0.f : h;
      g[in.b] += x < y ? 0.f : h;
      break;
    }
    case STPDE_RES_MAX: {
      const float x = v[in.a], y = v[in.b], h = x == y ? gi * 0.5f : gi;
      g[in.a] += x < y ? 0.f : h;
      g[in.b] += x > y ? 0.f : h;
      break;
    }
    case STPDE_RES_SEL: {    // torch.where: the selected operand takes the cotangent, the other exactly +0 -- a select, not
      // gi * mask: a NaN cotangent does not leak into the branch not taken -- and nothing goes into the mask
      const bool then = v[in.a] != 0.f;
      g[STPDE_RES_SEL_THEN(in.b)] += then ? gi : 0.f;
      g[STPDE_RES_SEL_ELSE(in.b)] += then ? 0.f : gi;
      break;
    }
    default: break;   // SIGN, STEP, STEPC, the comparisons and AND OR NOT: adjoint 0
  }
}

// The reverse rule of instruction i at point p (its adjoint register g[i] is complete: every reader comes later in the program).
__device__ __forceinline__ void res_bwd_step(const stpde_res_ins& in, int i, const float* v, float* g, const ResArgs& a, int p) {
  const float gi = g[i];
  if (in.op > STPDE_RES_OUT) {
    res_bwd_ext(in, i, v, g, gi);
    return;
  }
  switch (in.op) {
    case STPDE_RES_OUT: g[in.a] += a.res_bar[(size_t)in.b * a.P + p]; break;
    case STPDE_RES_JET: {
      float* dst = a.jets_bar + (size_t)in.a * a.ld_s + (size_t)in.b * a.ld_c + p;   // this thread owns point p
      *dst += gi;
      break;
    }
    case STPDE_RES_ADD: g[in.a] += gi; g[in.b] += gi; break;
    case STPDE_RES_SUB: g[in.a] += gi; g[in.b] -= gi; break;
    case STPDE_RES_MUL: g[in.a] += gi * v[in.b]; g[in.b] += gi * v[in.a]; break;
    case STPDE_RES_DIV: g[in.a] += gi / v[in.b]; g[in.b] -= gi * v[i] / v[in.b]; break;
    case STPDE_RES_NEG: g[in.a] -= gi; break;
    case STPDE_RES_POWI:   // d(x^n)/dx = n x^(n-1), evaluated without dividing by x (x = 0 is a regular point for n >= 1)
      if (in.b != 0) g[in.a] += gi * (float)in.b * res_ipow(v[in.a], in.b - 1);
      break;
    case STPDE_RES_SIN: g[in.a] += gi * cosf(v[in.a]); break;
    case STPDE_RES_COS: g[in.a] -= gi * sinf(v[in.a]); break;
    case STPDE_RES_EXP: g[in.a] += gi * v[i]; break;
    case STPDE_RES_LOG: g[in.a] += gi / v[in.a]; break;
    case STPDE_RES_SQRT: g[in.a] += gi * 0.5f / v[i]; break;
    case STPDE_RES_TANH: g[in.a] += gi * (1.f - v[i] * v[i]); break;
    case STPDE_RES_ABS: g[in.a] += v[in.a] > 0.f ? gi : (v[in.a] < 0.f ? -gi : 0.f); break;   // torch: sign(0) = 0
    default: break;   // X, CONST: the coordinates are not differentiated on this path
  }
}

__global__ __launch_bounds__(256) void k_residual_bwd(ResArgs a) {
  __shared__ stpde_res_ins prog[RES_MAX];
  for (int i = threadIdx.x; i < a.nins; i += 256) prog[i] = a.prog[i];
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.P) return;
  float v[RES_MAX], g[RES_MAX];
  for (int i = 0; i < a.nins; ++i) {
    v[i] = res_eval<false>(prog[i], v, a, p, nullptr);
    g[i] = 0.f;
  }
  for (int i = a.nins - 1; i >= 0; --i) {
    const stpde_res_ins in = prog[i];
    res_bwd_step(in, i, v, g, a, p);
  }
}

// ---- the same two kernels for programs that read coefficients from device memory (stpde_res_coefs) ----------------
// A block belongs to ONE batch element (grid (ceil(N / 256), B)), so the coefficient values a point sees are uniform over the
// block: thread k stages value[k][per_batch[k] ? b : 0] into LDS next to the program, and a late-bound CONST (b != 0) reads
// coef[a].  The values are read at run time: an in-place update of a coefficient tensor is seen by the next launch (and by the
// next replay of a graph that captured it).
struct CoefArgs {
  int n, N, det;
  int per_batch[STPDE_RES_MAX_COEF];
  const float* value[STPDE_RES_MAX_COEF];
  float* bar[STPDE_RES_MAX_COEF];
};

__device__ __forceinline__ void res_stage_coefs(const CoefArgs& c, int b, float* coef) {
#pragma unroll
  for (int k = 0; k < STPDE_RES_MAX_COEF; ++k)
    if ((int)threadIdx.x == k) coef[k] = k < c.n ? c.value[k][c.per_batch[k] ? b : 0] : 0.f;
}

__global__ __launch_bounds__(256) void k_residual_coef_fwd(ResArgs a, CoefArgs c) {
  __shared__ stpde_res_ins prog[RES_MAX];
  __shared__ float coef[STPDE_RES_MAX_COEF];
  for (int i = threadIdx.x; i < a.nins; i += 256) prog[i] = a.prog[i];
  res_stage_coefs(c, blockIdx.y, coef);
  __syncthreads();
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= c.N) return;
  const int p = blockIdx.y * c.N + q;
  float v[RES_MAX];
  for (int i = 0; i < a.nins; ++i) {
    const stpde_res_ins in = prog[i];
    v[i] = res_eval<true>(in, v, a, p, coef);
    if (in.op == STPDE_RES_OUT) a.res[(size_t)in.b * a.P + p] = v[i];
  }
}

// The adjoint: value replay and reverse sweep as k_residual_bwd (jets_bar is owned per point).  The adjoint register of a
// late-bound CONST is d loss / d coefficient AT this point; where a gradient is wanted (bar[k] != NULL) it is summed over the
// block -- wave_sum, four partials in LDS, (p0 + p1) + (p2 + p3): the shape of k_loss_sum -- and one thread adds the block sum
// into bar[k][per_batch[k] ? b : 0] (fp32 atomic, or the long accumulator in deterministic mode).  The program is uniform over
// the block, so every thread reaches that reduction at the same instruction.  No thread leaves early: the lanes past the
// batch element's last point (live == false) run neither the replay nor the rules -- no load, no store -- and enter every
// reduction with exactly +0.
__global__ __launch_bounds__(256) void k_residual_coef_bwd(ResArgs a, CoefArgs c) {
  __shared__ stpde_res_ins prog[RES_MAX];
  __shared__ float coef[STPDE_RES_MAX_COEF];
  __shared__ float* cbar[STPDE_RES_MAX_COEF];
  __shared__ float part[4];
  for (int i = threadIdx.x; i < a.nins; i += 256) prog[i] = a.prog[i];
  res_stage_coefs(c, blockIdx.y, coef);
#pragma unroll
  for (int k = 0; k < STPDE_RES_MAX_COEF; ++k)
    if ((int)threadIdx.x == k)      // (a null bar[k] stays null: no gradient wanted; a long accumulator is 2 * STPDE_DET_K floats)
      cbar[k] = (k < c.n && c.bar[k]) ? c.bar[k] + (c.per_batch[k] ? (size_t)blockIdx.y * (c.det ? 2 * STPDE_DET_K : 1) : 0) : nullptr;
  __syncthreads();
  const int q = blockIdx.x * 256 + threadIdx.x;
  const bool live = q < c.N;
  const int p = blockIdx.y * c.N + (live ? q : 0);
  float v[RES_MAX], g[RES_MAX];
  if (live) {
    for (int i = 0; i < a.nins; ++i) {
      v[i] = res_eval<true>(prog[i], v, a, p, coef);
      g[i] = 0.f;
    }
  }
  for (int i = a.nins - 1; i >= 0; --i) {
    const stpde_res_ins in = prog[i];
    if (in.op == STPDE_RES_CONST && in.b != 0) {          // uniform over the block
      float* dst = cbar[in.a & (STPDE_RES_MAX_COEF - 1)];
      if (dst) {                                           // uniform as well
        float gi = 0.f;
        if (live) gi = g[i];
        const float s = wave_sum(gi);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) acc_add_f32(dst, 0, (part[0] + part[1]) + (part[2] + part[3]), c.det);
        __syncthreads();                                   // part is written again by the next coefficient
      }
      continue;
    }
    if (live) res_bwd_step(in, i, v, g, a, p);
  }
}

static int res_check(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P, const float* jets) {
  if (!prog_dev || nins <= 0 || nins > RES_MAX || n_eq <= 0 || n_out <= 0 || P <= 0 || !jets) {
    stpde_set_error("residual: bad argument (at most %d program instructions)", RES_MAX);
    return STPDE_E_BADARG;
  }
  return STPDE_OK;
}

extern "C" int stpde_residual_fwd(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P,
                                  const float* jets, long ld_stream, long ld_channel, const float* x, float* res,
                                  void* stream) {
  int rc = res_check(prog_dev, nins, n_eq, n_out, P, jets);
  if (rc) return rc;
  if (!res) {
    stpde_set_error("residual_fwd: null output");
    return STPDE_E_BADARG;
  }
  ResArgs a{prog_dev, nins, n_eq, n_out, P, jets, ld_stream, ld_channel, x, res, nullptr, nullptr};
  STPDE_LAUNCH(k_residual_fwd, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_residual_fwd");
}

extern "C" int stpde_residual_bwd(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P,
                                  const float* jets, long ld_stream, long ld_channel, const float* x,
                                  const float* res_bar, float* jets_bar, void* stream) {
  int rc = res_check(prog_dev, nins, n_eq, n_out, P, jets);
  if (rc) return rc;
  if (!res_bar || !jets_bar) {
    stpde_set_error("residual_bwd: null pointer");
    return STPDE_E_BADARG;
  }
  ResArgs a{prog_dev, nins, n_eq, n_out, P, jets, ld_stream, ld_channel, x, nullptr, res_bar, jets_bar};
  STPDE_LAUNCH(k_residual_bwd, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_residual_bwd");
}

static int res_coef_check(const stpde_res_coefs* coefs, int P, CoefArgs* c) {
  if (!coefs) {
    stpde_set_error("residual_coef: null stpde_res_coefs");
    return STPDE_E_BADARG;
  }
  if (coefs->n < 1 || coefs->n > STPDE_RES_MAX_COEF) {
    stpde_set_error("residual_coef: %d coefficients (1 .. %d)", coefs->n, STPDE_RES_MAX_COEF);
    return STPDE_E_BADARG;
  }
  if (coefs->n_per_batch <= 0 || P % coefs->n_per_batch != 0 || P / coefs->n_per_batch > 65535) {
    stpde_set_error("residual_coef: P = %d points are not B * n_per_batch with n_per_batch = %d (B <= 65535)", P,
                    coefs->n_per_batch);
    return STPDE_E_BADARG;
  }
  c->n = coefs->n;
  c->N = coefs->n_per_batch;
  c->det = coefs->det ? 1 : 0;
  for (int k = 0; k < STPDE_RES_MAX_COEF; ++k) {
    const bool used = k < coefs->n;
    if (used && !coefs->value[k]) {
      stpde_set_error("residual_coef: value[%d] is null", k);
      return STPDE_E_BADARG;
    }
    c->per_batch[k] = used && coefs->per_batch[k] ? 1 : 0;
    c->value[k] = used ? coefs->value[k] : nullptr;
    c->bar[k] = used ? coefs->bar[k] : nullptr;
  }
  return STPDE_OK;
}

extern "C" int stpde_residual_coef_fwd(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P,
                                       const float* jets, long ld_stream, long ld_channel, const float* x, float* res,
                                       const stpde_res_coefs* coefs, void* stream) {
  int rc = res_check(prog_dev, nins, n_eq, n_out, P, jets);
  if (rc) return rc;
  if (!res) {
    stpde_set_error("residual_coef_fwd: null output");
    return STPDE_E_BADARG;
  }
  CoefArgs c;
  rc = res_coef_check(coefs, P, &c);
  if (rc) return rc;
  ResArgs a{prog_dev, nins, n_eq, n_out, P, jets, ld_stream, ld_channel, x, res, nullptr, nullptr};
  STPDE_LAUNCH(k_residual_coef_fwd, dim3((c.N + 255) / 256, P / c.N), dim3(256), 0, (hipStream_t)stream, a, c);
  return stpde_check_launch("k_residual_coef_fwd");
}

extern "C" int stpde_residual_coef_bwd(const stpde_res_ins* prog_dev, int nins, int n_eq, int n_out, int P,
                                       const float* jets, long ld_stream, long ld_channel, const float* x,
                                       const float* res_bar, float* jets_bar, const stpde_res_coefs* coefs, void* stream) {
  int rc = res_check(prog_dev, nins, n_eq, n_out, P, jets);
  if (rc) return rc;
  if (!res_bar || !jets_bar) {
    stpde_set_error("residual_coef_bwd: null pointer");
    return STPDE_E_BADARG;
  }
  CoefArgs c;
  rc = res_coef_check(coefs, P, &c);
  if (rc) return rc;
  ResArgs a{prog_dev, nins, n_eq, n_out, P, jets, ld_stream, ld_channel, x, nullptr, res_bar, jets_bar};
  STPDE_LAUNCH(k_residual_coef_bwd, dim3((c.N + 255) / 256, P / c.N), dim3(256), 0, (hipStream_t)stream, a, c);
  return stpde_check_launch("k_residual_coef_bwd");
}

// ---- loss reductions of the train step (experiments/rb2d/train.py:69-76: l1 / mse / smooth_l1 of prediction vs target
// and of the stacked residuals vs 0), as SUMS (the caller divides by the global element count, so that the same code
// serves the point-sharded multi-GPU step).  One pass, block reduction, one atomic per block.
struct LossArgs {
  int kind;
  int det;             // forward: out is a long accumulator (common.h), not a float
  long n;
  const float* a;
  const float* b;      // null: compare against 0
  float* out;          // forward: scalar accumulator (zero-filled by the caller)
  const float* gscale; // backward: device scalar = d loss / d sum
  float* ga;           // backward: d loss / d a
};

__device__ __forceinline__ float loss_elem(int kind, float d) {
  const float ad = fabsf(d);
  if (kind == STPDE_LOSS_L1) return ad;
  if (kind == STPDE_LOSS_L2) return d * d;
  return ad < 1.f ? 0.5f * d * d : ad - 0.5f;          // smooth_l1, beta = 1 (torch default)
}
__device__ __forceinline__ float loss_grad(int kind, float d) {
  if (kind == STPDE_LOSS_L1) return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (kind == STPDE_LOSS_L2) return 2.f * d;
  return d >= 1.f ? 1.f : (d <= -1.f ? -1.f : d);      // both comparisons are false for NaN: the gradient stays NaN (torch)
}

__global__ __launch_bounds__(256) void k_loss_sum(LossArgs a) {
  __shared__ float part[4];
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256)
    s += loss_elem(a.kind, a.a[i] - (a.b ? a.b[i] : 0.f));
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) acc_add_f32(a.out, 0, (part[0] + part[1]) + (part[2] + part[3]), a.det);
}

__global__ __launch_bounds__(256) void k_loss_grad(LossArgs a) {
  const float g = *a.gscale;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256)
    a.ga[i] = g * loss_grad(a.kind, a.a[i] - (a.b ? a.b[i] : 0.f));
}

extern "C" int stpde_loss_sum(int kind, long n, const float* a, const float* b, float* out_sum, void* stream) {
  const int det = (kind & STPDE_LOSS_DET) ? 1 : 0;
  kind &= ~STPDE_LOSS_DET;
  if (kind < 0 || kind > 2 || n <= 0 || !a || !out_sum) {
    stpde_set_error("loss_sum: bad argument");
    return STPDE_E_BADARG;
  }
  LossArgs args{kind, det, n, a, b, out_sum, nullptr, nullptr};
  long blocks = (n + 1023) / 1024;
  if (blocks > 1024) blocks = 1024;
  STPDE_LAUNCH(k_loss_sum, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, args);
  return stpde_check_launch("k_loss_sum");
}

extern "C" int stpde_loss_grad(int kind, long n, const float* a, const float* b, const float* grad_sum_dev,
                               float* grad_a, void* stream) {
  if (kind < 0 || kind > 2 || n <= 0 || !a || !grad_sum_dev || !grad_a) {
    stpde_set_error("loss_grad: bad argument");
    return STPDE_E_BADARG;
  }
  LossArgs args{kind, 0, n, a, b, nullptr, grad_sum_dev, grad_a};
  long blocks = (n + 1023) / 1024;
  if (blocks > 2048) blocks = 2048;
  STPDE_LAUNCH(k_loss_grad, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, args);
  return stpde_check_launch("k_loss_grad");
}
