// Train-step tail: gradient value clipping + Adam update fused into one pass over a
// parameter tensor.  Replaces torch.nn.utils.clip_grad_value_ + optimizer.step() of the reference
// (experiments/rb2d/train.py:79-83, optim.Adam at :330-333).  Pure HBM streaming: 16 B read (p, g, m, v) and 12 B
// written (p, m, v) per element, float4 accesses, grid-stride.
#include "common.h"

// ---- the two traversals every update kernel is made of -------------------------------------------------------------
// quad(e) updates the four elements from e on with float4 accesses (e a multiple of 4, the pointers 16-byte aligned),
// one(e) a single element.

// Flat pass over n elements: grid-stride over the quads, the n % 4 tail by block 0.
template <class Quad, class One>
__device__ __forceinline__ void flat_pass(long n, Quad quad, One one) {
  const long n4 = n / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) quad(4 * i);
  if (blockIdx.x == 0) {  // tail (n not a multiple of 4)
    const long i = n4 * 4 + threadIdx.x;
    if (i < n) one(i);
  }
}

// Multi-tensor pass: ONE launch updates every parameter tensor of the model.  Block b works on chunk b of the chunk
// table (tensor index, element offset): elements [c.offset, min(c.offset + chunk_elems, n)) of an n-element tensor.
template <class Quad, class One>
__device__ __forceinline__ void chunk_pass(const stpde_adam_chunk& c, long n, int chunk_elems, Quad quad, One one) {
  const long lo = c.offset;
  const long hi = lo + chunk_elems < n ? lo + chunk_elems : n;
  const long n4 = (hi - lo) / 4;           // offsets are multiples of 4 and the pointers 16-byte aligned
  for (long i = threadIdx.x; i < n4; i += 256) quad(lo + 4 * i);
  const long e = lo + 4 * n4 + threadIdx.x;
  if (e < hi) one(e);
}

// grid of a flat pass: one quad per thread, at most 2048 blocks
static dim3 flat_grid(long n) {
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

// argument check of the four table entry points.  desc_ok: the caller's own check of its descriptor; aligned: state block and
// tables must be 16-byte aligned (every entry point but the oldest, stpde_clip_adam_multi, whose contract never said so)
static int check_tables(const char* who, bool desc_ok, bool aligned, const void* state_dev, const void* tensors_dev,
                        const void* chunks_dev, int nchunks, int chunk_elems) {
  if (!desc_ok || !tensors_dev || !chunks_dev || nchunks <= 0 || chunk_elems <= 0 || (chunk_elems & 3)) {
    stpde_set_error("%s: bad argument (chunk_elems must be a positive multiple of 4)", who);
    return STPDE_E_BADARG;
  }
  if (aligned && (((size_t)state_dev | (size_t)tensors_dev | (size_t)chunks_dev) & 15)) {
    stpde_set_error("%s: state block and tables must be 16-byte aligned", who);
    return STPDE_E_BADARG;
  }
  return STPDE_OK;
}

// ---- Adam ----------------------------------------------------------------------------------------------------------
struct AdamArgs {
  stpde_adam_desc d;
  float* p;
  const float* g;
  float* m;
  float* v;
};

__device__ __forceinline__ void adam_elem(const stpde_adam_desc& d, float& p, float g, float& m, float& v) {
  if (d.clip > 0.f) g = fminf(fmaxf(g, -d.clip), d.clip);        // clip_grad_value_
  if (d.weight_decay != 0.f) g = g + d.weight_decay * p;
  m = m + (1.f - d.beta1) * (g - m);                             // torch: exp_avg.lerp_(grad, 1 - beta1)
  v = d.beta2 * v + (1.f - d.beta2) * g * g;                     // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v) / d.bias2_sqrt + d.eps;
  p = p - d.step_size * (m / denom);                             // addcdiv_(exp_avg, denom, value=-lr/bias1)
}

__device__ __forceinline__ void adam_quad(const stpde_adam_desc& d, float* P, const float* G, float* M, float* V, long e) {
  f32x4 p = ld4(P + e), g = ld4(G + e), m = ld4(M + e), v = ld4(V + e);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float pp = p[r], mm = m[r], vv = v[r];
    adam_elem(d, pp, g[r], mm, vv);
    p[r] = pp;
    m[r] = mm;
    v[r] = vv;
  }
  st4(P + e, p);
  st4(M + e, m);
  st4(V + e, v);
}

__device__ __forceinline__ void adam_one(const stpde_adam_desc& d, float* P, const float* G, float* M, float* V, long e) {
  float pp = P[e], mm = M[e], vv = V[e];
  adam_elem(d, pp, G[e], mm, vv);
  P[e] = pp;
  M[e] = mm;
  V[e] = vv;
}

// d carries step_size / bias2_sqrt: the caller's host scalars, or the state block's (the _dev kernels)
__device__ __forceinline__ void adam_flat(const stpde_adam_desc& d, const AdamArgs& a) {
  flat_pass(d.n, [&](long e) { adam_quad(d, a.p, a.g, a.m, a.v, e); }, [&](long e) { adam_one(d, a.p, a.g, a.m, a.v, e); });
}

__device__ __forceinline__ void adam_chunk(const stpde_adam_desc& d, const stpde_adam_tensor& t, const stpde_adam_chunk& c,
                                           int chunk_elems) {
  chunk_pass(c, t.n, chunk_elems, [&](long e) { adam_quad(d, t.p, t.g, t.m, t.v, e); },
             [&](long e) { adam_one(d, t.p, t.g, t.m, t.v, e); });
}

__global__ __launch_bounds__(256) void k_clip_adam(AdamArgs a) { adam_flat(a.d, a); }

// The tensor table holds the four pointers, the length and the bias-correction factors (tensors may have different
// step counts).
__global__ __launch_bounds__(256) void k_clip_adam_multi(stpde_adam_desc d, const stpde_adam_tensor* tensors,
                                                         const stpde_adam_chunk* chunks, int chunk_elems) {
  const stpde_adam_chunk c = chunks[blockIdx.x];
  const stpde_adam_tensor t = tensors[c.tensor];
  d.step_size = t.step_size;
  d.bias2_sqrt = t.bias2_sqrt;
  adam_chunk(d, t, c, chunk_elems);
}

extern "C" int stpde_clip_adam_multi(const stpde_adam_desc* d, const stpde_adam_tensor* tensors_dev,
                                     const stpde_adam_chunk* chunks_dev, int nchunks, int chunk_elems, void* stream) {
  if (int rc = check_tables("clip_adam_multi", d != nullptr, false, nullptr, tensors_dev, chunks_dev, nchunks, chunk_elems))
    return rc;
  STPDE_LAUNCH(k_clip_adam_multi, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, *d, tensors_dev,
               chunks_dev, chunk_elems);
  return stpde_check_launch("k_clip_adam_multi");
}

extern "C" int stpde_clip_adam(const stpde_adam_desc* d, float* param, const float* grad, float* exp_avg,
                               float* exp_avg_sq, void* stream) {
  if (!d || d->n <= 0 || !param || !grad || !exp_avg || !exp_avg_sq || !(d->bias2_sqrt > 0.f)) {
    stpde_set_error("clip_adam: bad argument");
    return STPDE_E_BADARG;
  }
  if (((size_t)param | (size_t)grad | (size_t)exp_avg | (size_t)exp_avg_sq) & 15) {
    stpde_set_error("clip_adam: pointers must be 16-byte aligned");
    return STPDE_E_BADARG;
  }
  AdamArgs a{*d, param, grad, exp_avg, exp_avg_sq};
  STPDE_LAUNCH(k_clip_adam, flat_grid(d->n), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_clip_adam");
}

// ---- device-resident optimizer state (capturable optimizers) -----------------------------------------------------
// A captured launch freezes every by-value argument, so the per-step scalars of a HIP-graph-resident optimizer live in a
// caller-owned stpde_opt_state block: k_opt_advance (ONE workgroup, a launch of its own in front of the update) advances the
// step count and derives the two Adam bias-correction scalars from it in fp64; every block of the update kernel that follows
// on the stream reads the same finished values, so no grid-wide ordering is needed.
__global__ __launch_bounds__(64) void k_opt_advance(stpde_opt_desc d, stpde_opt_state* s) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long t = s->step + 1;
  const double lr = s->lr;
  s->step = t;
  s->step_size = (float)(lr / (1.0 - pow(d.beta1, (double)t)));
  s->bias2_sqrt = (float)sqrt(1.0 - pow(d.beta2, (double)t));
}

extern "C" int stpde_opt_advance(const stpde_opt_desc* d, stpde_opt_state* state_dev, void* stream) {
  if (!d || !state_dev || ((size_t)state_dev & 15) || !(d->beta1 >= 0.0 && d->beta1 < 1.0) ||
      !(d->beta2 >= 0.0 && d->beta2 < 1.0)) {
    stpde_set_error("opt_advance: bad argument (state block 16-byte aligned, 0 <= beta < 1)");
    return STPDE_E_BADARG;
  }
  STPDE_LAUNCH(k_opt_advance, dim3(1), dim3(64), 0, (hipStream_t)stream, *d, state_dev);
  return stpde_check_launch("k_opt_advance");
}

// k_clip_adam with step_size / bias2_sqrt read from the state block (written by the k_opt_advance in front of it)
__global__ __launch_bounds__(256) void k_clip_adam_dev(AdamArgs a, const stpde_opt_state* s) {
  a.d.step_size = s->step_size;
  a.d.bias2_sqrt = s->bias2_sqrt;
  adam_flat(a.d, a);
}

// k_clip_adam_multi with ONE step count for all tensors: the tables hold pointers and lengths only, so the caller builds
// them once and reuses them while the pointers do not change (step_size / bias2_sqrt of the rows are ignored)
__global__ __launch_bounds__(256) void k_clip_adam_multi_dev(stpde_adam_desc d, const stpde_opt_state* s,
                                                             const stpde_adam_tensor* tensors,
                                                             const stpde_adam_chunk* chunks, int chunk_elems) {
  const stpde_adam_chunk c = chunks[blockIdx.x];
  const stpde_adam_tensor t = tensors[c.tensor];
  d.step_size = s->step_size;
  d.bias2_sqrt = s->bias2_sqrt;
  adam_chunk(d, t, c, chunk_elems);
}

static bool adam_desc_ok(const stpde_adam_desc* d) {
  return d && d->beta1 >= 0.f && d->beta1 < 1.f && d->beta2 >= 0.f && d->beta2 < 1.f && d->eps >= 0.f;
}

extern "C" int stpde_clip_adam_dev(const stpde_adam_desc* d, const stpde_opt_state* state_dev, float* param,
                                   const float* grad, float* exp_avg, float* exp_avg_sq, void* stream) {
  if (!adam_desc_ok(d) || d->n <= 0 || !state_dev || !param || !grad || !exp_avg || !exp_avg_sq) {
    stpde_set_error("clip_adam_dev: bad argument");
    return STPDE_E_BADARG;
  }
  if (((size_t)state_dev | (size_t)param | (size_t)grad | (size_t)exp_avg | (size_t)exp_avg_sq) & 15) {
    stpde_set_error("clip_adam_dev: pointers must be 16-byte aligned");
    return STPDE_E_BADARG;
  }
  AdamArgs a{*d, param, grad, exp_avg, exp_avg_sq};
  STPDE_LAUNCH(k_clip_adam_dev, flat_grid(d->n), dim3(256), 0, (hipStream_t)stream, a, state_dev);
  return stpde_check_launch("k_clip_adam_dev");
}

extern "C" int stpde_clip_adam_multi_dev(const stpde_adam_desc* d, const stpde_opt_state* state_dev,
                                         const stpde_adam_tensor* tensors_dev, const stpde_adam_chunk* chunks_dev,
                                         int nchunks, int chunk_elems, void* stream) {
  if (int rc = check_tables("clip_adam_multi_dev", adam_desc_ok(d) && state_dev, true, state_dev, tensors_dev, chunks_dev, nchunks,
                            chunk_elems))
    return rc;
  STPDE_LAUNCH(k_clip_adam_multi_dev, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, *d, state_dev,
               tensors_dev, chunks_dev, chunk_elems);
  return stpde_check_launch("k_clip_adam_multi_dev");
}

// ---- gradient value clipping + SGD (the reference's --optim sgd, experiments/rb2d/train.py:220, :330-333) ------------
// torch.optim.SGD's rule behind clip_grad_value_: 8 B read (p, g) and 4 B written per element without momentum, 12 B / 8 B
// with a momentum buffer.
struct SgdRule {
  float clip, lr, momentum, undamp, weight_decay;
  int nesterov, first;
};

__device__ __forceinline__ SgdRule sgd_rule(const stpde_sgd_desc& d, const stpde_opt_state* s, int first) {
  SgdRule r{d.clip, d.lr, d.momentum, 1.f - d.dampening, d.weight_decay, d.nesterov, first};
  if (s) {                       // device-state form: learning rate and "first step" from the block
    r.lr = (float)s->lr;
    r.first = s->step == 1;
  }
  return r;
}

__device__ __forceinline__ void sgd_elem(const SgdRule& d, float& p, float g, float& b) {
  if (d.clip > 0.f) g = fminf(fmaxf(g, -d.clip), d.clip);        // clip_grad_value_
  if (d.weight_decay != 0.f) g = g + d.weight_decay * p;         // grad.add(param, alpha=weight_decay)
  if (d.momentum != 0.f) {
    b = d.first ? g : d.momentum * b + d.undamp * g;             // buf = clone(grad) | buf.mul_(momentum).add_(grad, alpha=1 - dampening)
    g = d.nesterov ? g + d.momentum * b : b;
  }
  p = p - d.lr * g;                                              // param.add_(grad, alpha=-lr)
}

// B (momentum buffer) is touched only with momentum != 0 (block-uniform branch)
__device__ __forceinline__ void sgd_quad(const SgdRule& d, float* P, const float* G, float* B, long e) {
  const bool mom = d.momentum != 0.f;
  f32x4 p = ld4(P + e), g = ld4(G + e), b = mom ? ld4(B + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float pp = p[r], bb = b[r];
    sgd_elem(d, pp, g[r], bb);
    p[r] = pp;
    b[r] = bb;
  }
  st4(P + e, p);
  if (mom) st4(B + e, b);
}

__device__ __forceinline__ void sgd_one(const SgdRule& d, float* P, const float* G, float* B, long e) {
  const bool mom = d.momentum != 0.f;
  float pp = P[e], bb = mom ? B[e] : 0.f;
  sgd_elem(d, pp, G[e], bb);
  P[e] = pp;
  if (mom) B[e] = bb;
}

struct SgdArgs {
  stpde_sgd_desc d;
  const stpde_opt_state* s;
  float* p;
  const float* g;
  float* b;
};

__global__ __launch_bounds__(256) void k_clip_sgd(SgdArgs a) {
  const SgdRule r = sgd_rule(a.d, a.s, a.d.first_step);
  flat_pass(a.d.n, [&](long e) { sgd_quad(r, a.p, a.g, a.b, e); }, [&](long e) { sgd_one(r, a.p, a.g, a.b, e); });
}

__global__ __launch_bounds__(256) void k_clip_sgd_multi(stpde_sgd_desc d, const stpde_opt_state* s,
                                                        const stpde_sgd_tensor* tensors, const stpde_adam_chunk* chunks,
                                                        int chunk_elems) {
  const stpde_adam_chunk c = chunks[blockIdx.x];
  const stpde_sgd_tensor t = tensors[c.tensor];
  const SgdRule r = sgd_rule(d, s, t.first_step);
  chunk_pass(c, t.n, chunk_elems, [&](long e) { sgd_quad(r, t.p, t.g, t.buf, e); },
             [&](long e) { sgd_one(r, t.p, t.g, t.buf, e); });
}

static bool sgd_desc_ok(const stpde_sgd_desc* d) {
  return d && d->momentum >= 0.f && d->lr >= 0.f && (!d->nesterov || (d->momentum > 0.f && d->dampening == 0.f));
}

extern "C" int stpde_clip_sgd(const stpde_sgd_desc* d, const stpde_opt_state* state_dev, float* param, const float* grad,
                              float* momentum_buf, void* stream) {
  if (!sgd_desc_ok(d) || d->n <= 0 || !param || !grad || (d->momentum != 0.f && !momentum_buf)) {
    stpde_set_error("clip_sgd: bad argument (momentum != 0 needs a buffer; nesterov needs momentum > 0, dampening 0)");
    return STPDE_E_BADARG;
  }
  if (((size_t)state_dev | (size_t)param | (size_t)grad | (size_t)momentum_buf) & 15) {
    stpde_set_error("clip_sgd: pointers must be 16-byte aligned");
    return STPDE_E_BADARG;
  }
  SgdArgs a{*d, state_dev, param, grad, momentum_buf};
  STPDE_LAUNCH(k_clip_sgd, flat_grid(d->n), dim3(256), 0, (hipStream_t)stream, a);
  return stpde_check_launch("k_clip_sgd");
}

extern "C" int stpde_clip_sgd_multi(const stpde_sgd_desc* d, const stpde_opt_state* state_dev,
                                    const stpde_sgd_tensor* tensors_dev, const stpde_adam_chunk* chunks_dev, int nchunks,
                                    int chunk_elems, void* stream) {
  if (int rc = check_tables("clip_sgd_multi", sgd_desc_ok(d), true, state_dev, tensors_dev, chunks_dev, nchunks, chunk_elems))
    return rc;
  STPDE_LAUNCH(k_clip_sgd_multi, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, *d, state_dev, tensors_dev,
               chunks_dev, chunk_elems);
  return stpde_check_launch("k_clip_sgd_multi");
}
