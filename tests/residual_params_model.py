"""Host model of the residual kernels that read coefficients from device memory (k_residual_coef_fwd / k_residual_coef_bwd of
csrc/residual.hip), on top of tests/residual_model.py, which is used as it is.

A late-bound CONST -- op = CONST, b = 1, a = k, c = 0 -- evaluates to ``value[k][p // N]`` for a coefficient per batch element and
to ``value[k][0]`` for a scalar one (P = B * N points, batch-major).  As far as a point is concerned that is a JET read of one more
stream whose row k holds these values.  So the model is a rewrite and nothing else:

``late_bound(prog)``                the k of every late-bound CONST, in program order.
``rewrite(prog, n_streams)``        the program with every late-bound CONST k replaced by JET (n_streams, k).
``expand(jets, values, B)``         jets [S, C, P] with the coefficient stream appended: [S + 1, max(C, K), P], row k of stream S =
                                    values[k] ([] / [1] / [B]) repeated over the N = P / B points of each batch element.
``run`` / ``adjoint``               residual_model.run / .adjoint on the rewritten program and the expanded jets: the values, and
                                    (jets_bar [S, C, P], the per-point coefficient adjoints g [K, P]) -- row k of the appended
                                    stream of the model's jets_bar.  With float32 every exact opcode is the kernel's IEEE operation
                                    in the kernel's order, so the device reproduces residuals and jets_bar bit for bit, and its
                                    per-point coefficient adjoints (the register g[i] of the late-bound CONST) are the model's.
``coef_grad64(g, B, per_batch)``    the reference of a coefficient gradient: the fp64 sum of the float32 model's per-point adjoints,
                                    per batch element [B] or over all points [].
``coef_sum_bound(N, B, per_batch, det)``  what the device's sum may differ from that reference by, in units of 2^-24 * sum |g_p|
                                    over the points that feed one gradient element.

The bound, from the structure of k_residual_coef_bwd.  A block holds 256 consecutive points of ONE batch element (grid
(ceil(N / 256), B)); lanes past the element's last point enter with exactly +0.  The block sums its 256 adjoints by wave_sum -- six
butterfly levels, every lane of a wave ends with the same sum of 64 -- and then (p0 + p1) + (p2 + p3) over the four wave sums: a
tree of depth 6 + 2, in which every input passes 8 additions.  Each addition rounds a partial sum whose magnitude is at most the
sum of |g_p| under it, so the block sum is off by at most 8 * 2^-24 * sum |g_p| of its block (first order, as
residual_model.loss_sum_bound counts).  Then:

* default mode: thread 0 of every block adds the block sum with one fp32 atomic.  A gradient element is fed by
  ``blocks = ceil(N / 256)`` blocks (per batch element) or ``B * ceil(N / 256)`` (scalar), in any order; every atomic rounds a
  partial sum bounded by sum |g_p| of the element: ``blocks`` more roundings.  Bound 8 + blocks.
* deterministic mode: the block sums go exactly into the long accumulator of the element (integer atomics), which is rounded to
  fp32 once.  Bound 8 + 1.

No other term: the adjoint registers themselves are the model's bit for bit (exact-opcode programs), and a NaN or an infinity in
them propagates through the sum in either mode.
"""
import numpy as np

from tests import residual_model as M

F = M.F
U = M.U
CONST = M.OPS["CONST"]
JET = M.OPS["JET"]
BLOCK = 256


def late_bound(prog):
    return [int(a) for op, a, b, c in prog.tolist() if op == CONST and b != 0]


def coef_const(k):
    """The instruction tuple of a late-bound CONST for residual_model.program."""
    return ("CONST", int(k), 1, 0.0)


def rewrite(prog, n_streams):
    out = np.array(prog, dtype=M.DT)
    for i, (op, a, b, c) in enumerate(prog.tolist()):
        if op == CONST and b != 0:
            assert b == 1 and c == 0.0, (i, op, a, b, c)
            out[i] = (JET, n_streams, a, 0.0)
    return out


def expand(jets, values, B, dtype=F):
    """jets [S, C, P] + the coefficient stream; values: list of K arrays of shape [] / [1] / [B]."""
    jets = np.asarray(jets, dtype=dtype)
    S, C, P = jets.shape
    assert P % B == 0
    N = P // B
    out = np.zeros((S + 1, max(C, len(values)), P), dtype=dtype)
    out[:S, :C] = jets
    for k, v in enumerate(values):
        v = np.asarray(v, dtype=dtype).reshape(-1)
        assert v.size in (1, B), (k, v.shape)
        out[S, k] = np.repeat(v, N) if v.size == B and B > 1 else np.full(P, v[0], dtype=dtype)
    return out


def run(prog, jets, x, values, B, dtype=np.float64):
    S = np.shape(jets)[0]
    return M.run(rewrite(prog, S), expand(jets, values, B, dtype), x, dtype)


def adjoint(prog, jets, x, res_bar, values, B, dtype=np.float64):
    """(jets_bar [S, C, P], g [K, P]: d (sum res * res_bar) / d coefficient k at each point)."""
    S, C, _ = np.shape(jets)
    bar = M.adjoint(rewrite(prog, S), expand(jets, values, B, dtype), x, res_bar, dtype)
    return bar[:S, :C], bar[S, :len(values)]


def coef_grad64(g_row, B, per_batch):
    """fp64 sum of one coefficient's per-point adjoints [P]: [B] per batch element, or [] over all points."""
    g = np.asarray(g_row, dtype=np.float64)
    with np.errstate(all="ignore"):
        return g.reshape(B, -1).sum(1) if per_batch else g.sum()


def coef_abs64(g_row, B, per_batch):
    """sum |g_p| over the points that feed each gradient element (the unit of coef_sum_bound is 2^-24 of it)."""
    return coef_grad64(np.abs(np.asarray(g_row, dtype=np.float64)), B, per_batch)


def coef_blocks(N, B, per_batch):
    per_element = -(-N // BLOCK)
    return per_element if per_batch else B * per_element


def coef_sum_bound(N, B, per_batch, det):
    return 8 + (1 if det else coef_blocks(N, B, per_batch))
