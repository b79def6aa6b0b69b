"""Host model of the activation jets of csrc/common.h (act_eval_t / act_eval2_t, act_jet_fwd_w, act_jet_adj_w, swish_beta_adj):
the pre-activation sweep, the fp64 reference, a numpy fp32 transcription and the error bounds that
tests/test_act_jet_host.py (margin, oracle guard, sensitivity) and tests/test_gpu_act_jets.py (element-wise parity of the layer
kernels) share.  Built once, shared, never modified.

``sweep()``      256 x 128 fp32 pre-activations: 64 designed points (both signs of zero, the tails, the seam of the home-made
                 log1p at e = 2^-10 <=> |a| = 6.9315, the softplus threshold 20 +- 1 ulp, exp underflow beyond 87.3 / 103.9),
                 then a seeded fill: uniform [-25, 25], uniform [-110, 110], 1e-3 * randn.  Apart from the exact +-0 no value is
                 0, i.e. none sits on a kink of ReLU / LeakyReLU / ELU, and the kernels under test see the values exactly
                 (selection-matrix weights), so fp32 and fp64 always take the same branch.
``reference``    oracle.jet_ref.act_derivs in fp64 (beta = float32(1.3) for Swish), the forward jet
                 h = s0, h_d = s1 a_d, h_ab = s2 a_a a_b + s1 a_ab, and its adjoint by torch.autograd on that expression.
``model_fp32``   the expression sequences of common.h in numpy fp32 with correctly rounded exp2 / log2 / reciprocal and the same
                 branch thresholds; no fused multiply-adds.  It only sizes the bounds.

Error measure: every element in units of 2^-24 * M, M = the fp64 sum of the absolute values of the terms of that output (the
"ulp of sum|terms|" of tests/test_gpu_fp32x3_products.py), with every |s_k| inside M floored at the natural scale of that
derivative: 1 + |a| for s0, beta^(k-1) for k >= 1 (beta = 1 except for Swish).  The floors are there because the kernels are
accurate absolutely, not relatively, in their tails: tanh(a) = (1 - e) / (1 + e) returns 0 for |a| < 3e-8, and
e = exp2(a * log2 e) carries |a| ulp of relative error from the rounding of its argument.
One floor is TIGHTER than that: softplus' s0 on the negative side is log1p(e) ~ e, and against 1 + |a| nothing that happens to
log1p there is visible at all (a wrong series coefficient, a misplaced seam).  The kernel's log1p promises two things: below the
seam, e < 2^-10, the series is as accurate as e itself; above it, log(fl(1 + e)) carries the rounding of 1 + e, half an ulp of 1.
So for softplus and a < 0 with e^a < 2^-10 the floor of s0 is (1 + |a|) * max(e^a, 2^-100) -- relative to the value, times the
1 + |a| that the rounding of the exponent's argument costs, down to where fp32 underflows -- and 1 + |a| everywhere else.  A seam
moved down to 2^-11 then breaks the bound (the log on 2^-11 <= e < 2^-10: 2^-24 absolute on a value of 2^-10.5); a seam moved up
only makes log1p more accurate, and a threshold moved up from 20 changes nothing fp32 can hold (s = 1 exactly, q < 2.1e-9), so
the sensitivity test moves both DOWN by the factor 2.

BOUNDS[act][direction][order] = 4 x the maximum model_fp32 reaches against the fp64 reference over the stream sets the GPU tests
use (forward (3,2), which contains (0,0) and (3,0); adjoint (3,6), (3,2), (3,0)); the factor 4 covers 1-ulp hardware
transcendentals against correctly rounded ones and FMA contraction.  order = the class of the output stream: 0 value,
1 first-order, 2 second-order (for the adjoint: the adjoint OF that input stream; s3 enters the adjoint of the value stream).
Model maxima measured on the CPU (python -m tests.act_jet_model), next to the bounds:

    activation   forward: model maximum -> bound          adjoint: model maximum -> bound
                 value / first / second                    value / first / second
    softplus     1.7 / 2.25 / 2.07 -> 6.8 / 9 / 8.27       1.92 / 2.72 / 2.27 -> 7.67 / 10.9 / 9.09
    tanh         1.1 / 4.15 / 7.93 -> 4.42 / 16.7 / 31.8   11.5 / 7.66 / 4.1 -> 46.2 / 30.7 / 16.4
    elu          0.284 / 1.46 / 2.3 -> 1.14 / 5.86 / 9.22  2.49 / 2.59 / 1.42 -> 9.96 / 10.4 / 5.7
    swish        1.83 / 3.07 / 2.7 -> 7.34 / 12.3 / 10.9   2.67 / 3.41 / 3.15 -> 10.7 / 13.7 / 12.7
    relu         0 / 0 / 0 -> 0 / 0 / 0                    0 / 0 / 0 -> 0 / 0 / 0
    leakyrelu    0.0134 / 0.0136 / 0.0105 -> 0.0537 / 0.0544 / 0.0422     0.00944 / 0.0136 / 0.0136 -> 0.0378 / 0.0544 / 0.0544
    dbeta        (3,6) 0.300, (3,2) 0.642, (3,0) 2.36 -> 9.45 (4 x the largest)

On an MI355X every kernel family reaches between 0.8 and 1.3 times these model maxima, and d/d beta 0.05 units at most (its
slots are filled with fp32 atomics, so that figure moves from run to run; the others do not)
(profiles/act_jet_errors.json, written by tests/test_gpu_act_jets.py).
The tanh figures are the cancellation of u = 1 - t * t (and of 1 - e near 0), recorded and accepted as it is.  ReLU is exact and
LeakyReLU is one rounding of 0.01f * a: their bounds are what they are, (nearly) zero.
Swish d/d beta (a sum of 32,768 terms, in units of 2^-24 * the fp64 sum of |terms|): the fp32 transcription of swish_beta_adj
summed sequentially in fp32 reaches the figures listed under "dbeta" (one draw of a rounding random walk per stream set, so the
largest of them is the model's reach); DBETA_BOUND is 4 x that.
"""
import numpy as np

F = np.float32
ACTS = ("softplus", "tanh", "elu", "swish", "relu", "leakyrelu")
BETA = F(1.3)
ROWS, FEATS = 256, 128
CANON_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
PAIRS = {0: (), 2: ((0, 1), (2, 2)), 6: CANON_PAIRS}       # (3,2): one mixed pair, one diagonal
FWD_SETS = ((0, 0), (3, 0), (3, 2))
ADJ_SETS = ((3, 6), (3, 2), (3, 0))
LOG2E, LN2, THIRD = F(1.44269504088896341), F(0.693147180559945309), F(0.33333334)
U = 2.0 ** -24

# 4 x the model maxima (see the module docstring); filled in from ``python -m tests.act_jet_model``
BOUNDS = {
    "softplus": {"fwd": (6.8, 9, 8.27), "adj": (7.67, 10.9, 9.09)},
    "tanh": {"fwd": (4.42, 16.7, 31.8), "adj": (46.2, 30.7, 16.4)},
    "elu": {"fwd": (1.14, 5.86, 9.22), "adj": (9.96, 10.4, 5.7)},
    "swish": {"fwd": (7.34, 12.3, 10.9), "adj": (10.7, 13.7, 12.7)},
    "relu": {"fwd": (0, 0, 0), "adj": (0, 0, 0)},
    "leakyrelu": {"fwd": (0.0537, 0.0544, 0.0422), "adj": (0.0378, 0.0544, 0.0544)},
}
DBETA_BOUND = 9.45


def _ulp_steps(x, n):
    x = F(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf))
    return float(x)


_sweep = None


def sweep():
    """[256, 128] fp32: the designed points first, then the seeded random fill."""
    global _sweep
    if _sweep is None:
        mags = [1e-30, 1e-12, 1e-6, 1e-4, _ulp_steps(2.0 ** -10, -1), _ulp_steps(2.0 ** -10, 1), 1e-3, 0.1, 0.5, 1, 2, 5, 6.93,
                6.94, 8, 9, 10, 15, 17, _ulp_steps(20, -1), 20.0, _ulp_steps(20, 1), 25, 40, 80, 87.3, 88.8, 100, 104, 1e3,
                1e4]
        v = [0.0, -0.0] + [s * m for m in mags for s in (1.0, -1.0)]
        rng = np.random.default_rng(20)
        n = ROWS * FEATS - len(v)
        fill = np.concatenate([rng.uniform(-25, 25, 20000), rng.uniform(-110, 110, n - 24000),
                               1e-3 * rng.standard_normal(4000)])
        a = np.concatenate([np.array(v), fill]).astype(F)
        assert a.shape == (ROWS * FEATS,) and np.count_nonzero(a == 0) == 2
        _sweep = a.reshape(ROWS, FEATS)
        _sweep.setflags(write=False)
    return _sweep


_streams = {}


def streams(shape=(ROWS, FEATS), seed=21):
    """Seeded input streams next to the sweep: tan [3] (magnitude in [0.5, 2], random sign), sec [6] (randn), cot [10] (randn)."""
    key = (shape, seed)
    if key not in _streams:
        rng = np.random.default_rng(seed)
        tan = (rng.uniform(0.5, 2.0, (3,) + shape) * rng.choice([-1.0, 1.0], (3,) + shape)).astype(F)
        sec = rng.standard_normal((6,) + shape).astype(F)
        cot = rng.standard_normal((10,) + shape).astype(F)
        for t in (tan, sec, cot):
            t.setflags(write=False)
        _streams[key] = (tan, sec, cot)
    return _streams[key]


def case_inputs(S1, S2, a=None, tan=None, sec=None):
    """pre [S] = (a, tangents, second-order inputs), cot [S], pairs of the stream set (S1, S2)."""
    a = sweep() if a is None else a
    t, sc, cot = streams(a.shape)
    tan = t if tan is None else tan
    sec = sc if sec is None else sec
    pre = [a] + ([tan[d] for d in range(3)] if S1 else []) + [sec[p] for p in range(S2)]
    return pre, [cot[s] for s in range(1 + S1 + S2)], PAIRS[S2]


# ---------------------------------------------------------------------------------------------------------------------
# fp32 transcription of csrc/common.h
# ---------------------------------------------------------------------------------------------------------------------
def _exp2(x):
    return np.exp2(x.astype(np.float64)).astype(F)


def _fast_exp(x):
    return _exp2((x * LOG2E).astype(F))


def _rcp(x):
    return (1.0 / x.astype(np.float64)).astype(F)


def _log1p_unit(e, seam):
    u = F(1) + e
    big = np.log2(u.astype(np.float64)).astype(F) * LN2
    small = e * (F(1) - e * (F(0.5) - e * THIRD))
    return np.where(e < F(seam), small, big).astype(F)


def model_fp32(name, a, beta=BETA, threshold=20.0, seam=9.765625e-4, scale=(1, 1, 1, 1)):
    """(s0, s1, s2, s3) as act_eval_t computes them (act_eval2_t<SOFTPLUS> is the same sequence, two elements at a time).
    ``threshold`` / ``seam`` / ``scale`` (a factor on each s_k) exist for the sensitivity test only."""
    a = np.asarray(a, dtype=F)
    one, zero = np.ones_like(a), np.zeros_like(a)
    with np.errstate(all="ignore"):
        if name == "tanh":
            e = _fast_exp(F(-2) * np.abs(a))
            t0 = (F(1) - e) * _rcp(F(1) + e)
            t = np.where(a < 0, -t0, t0)
            u = F(1) - t * t
            s = t, u, F(-2) * t * u, F(-2) * u * (F(1) - F(3) * t * t)
        elif name == "relu":
            m = np.where(a > 0, one, zero)
            s = a * m, m, zero, zero
        elif name == "leakyrelu":
            m = np.where(a > 0, one, F(0.01) * one)
            s = a * m, m, zero, zero
        elif name == "softplus":
            e = _fast_exp(-np.abs(a))
            inv = _rcp(F(1) + e)
            sg = np.where(a >= 0, inv, e * inv)
            q = e * inv * inv
            big = a > F(threshold)
            s = np.maximum(a, F(0)) + _log1p_unit(e, seam), np.where(big, one, sg), np.where(big, zero, q), \
                np.where(big, zero, q * (F(1) - F(2) * sg))
        elif name == "elu":
            pos = a > 0
            am = np.where(pos, zero, a)
            e = _fast_exp(am)
            s = np.where(pos, a, np.expm1(am.astype(np.float64)).astype(F)), np.where(pos, one, e), np.where(pos, zero, e), \
                np.where(pos, zero, e)
        elif name == "swish":
            prm = F(beta)
            ba = prm * a
            e = _fast_exp(-np.abs(ba))
            inv = _rcp(F(1) + e)
            sg = np.where(ba >= 0, inv, e * inv)
            q = e * inv * inv
            c = F(1) - F(2) * sg
            s = a * sg, sg + ba * q, prm * q * (F(2) + ba * c), prm * prm * q * (F(3) * c + ba * (c * c - F(2) * q))
        else:
            raise KeyError(name)
    return tuple((F(k) * x).astype(F) for k, x in zip(scale, s))


def jet_fwd_fp32(s, pre, pairs):
    """act_jet_fwd_w: h [S] from the fp32 s_k and pre [S]."""
    h = [s[0]]
    if len(pre) > 1:
        h += [s[1] * pre[1 + d] for d in range(3)]
        for p, (e0, e1) in enumerate(pairs):
            h.append(s[2] * pre[1 + e0] * pre[1 + e1] + s[1] * pre[4 + p])
    return h


def jet_adj_fp32(s, pre, hbar, pairs):
    """act_jet_adj_w: abar [S] from the fp32 s_k, pre [S] and hbar [S]."""
    ab = s[1] * hbar[0]
    if len(pre) == 1:
        return [ab]
    d = [s[1] * hbar[1 + k] for k in range(3)]
    ab = ab + s[2] * (pre[1] * hbar[1] + pre[2] * hbar[2] + pre[3] * hbar[3])
    tail = []
    for p, (e0, e1) in enumerate(pairs):
        u, v, hb = pre[1 + e0], pre[1 + e1], hbar[4 + p]
        ab = ab + (s[3] * u * v + s[2] * pre[4 + p]) * hb
        t0, t1 = s[2] * v * hb, s[2] * u * hb
        z = t0 * F(0)
        for k in range(3):
            d[k] = d[k] + ((t0 if e0 == k else z) + (t1 if e1 == k else z))
        tail.append(s[1] * hb)
    return [ab] + d + tail


def swish_beta_terms_fp32(a, pre, hbar, pairs, beta=BETA):
    """swish_beta_adj: the per-element term of d/d beta, fp32."""
    prm = F(beta)
    with np.errstate(all="ignore"):
        z = prm * a
        e = _fast_exp(-np.abs(z))
        inv = _rcp(F(1) + e)
        sg = np.where(z >= 0, inv, e * inv)
        q = e * inv * inv
        c = F(1) - F(2) * sg
        m = q * (F(2) + z * c)
        b0, b1, b2 = a * a * q, a * m, m + z * q * (F(3) * c + z * (c * c - F(2) * q))
        t = b0 * hbar[0]
        if len(pre) > 1:
            t = t + b1 * (pre[1] * hbar[1] + pre[2] * hbar[2] + pre[3] * hbar[3])
            for p, (e0, e1) in enumerate(pairs):
                t = t + (b2 * pre[1 + e0] * pre[1 + e1] + b1 * pre[4 + p]) * hbar[4 + p]
    return t.astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 reference and the scales M
# ---------------------------------------------------------------------------------------------------------------------
def floors(name, a64, s0_64):
    """Natural scale of s0..s3 (the floors of |s_k| inside M)."""
    b = float(BETA) if name == "swish" else 1.0
    f0 = 1.0 + np.abs(a64)
    if name == "softplus":
        e = np.exp(-np.abs(a64))
        f0 = np.where((a64 < 0) & (e < 2.0 ** -10), f0 * np.maximum(e, 2.0 ** -100), f0)
    one = np.ones_like(a64)
    return f0, one, b * one, b * b * one


_ref = {}


def reference(name, S1, S2, a=None, tan=None, sec=None):
    """dict(h [S], abar [S], Mh [S], Mabar [S], dbeta, dbeta_abs) in fp64 numpy for the stream set (S1, S2) on ``a`` (default:
    the sweep; cached then): forward jet from act_derivs, adjoint and d/d beta by torch.autograd, scales by the term lists."""
    import torch
    from oracle.jet_ref import act_derivs
    key = (name, S1, S2)
    shared = a is None and tan is None and sec is None
    if shared and key in _ref:
        return _ref[key]
    pre32, cot32, pairs = case_inputs(S1, S2, a, tan, sec)
    pre = [torch.from_numpy(np.array(p)).double().requires_grad_(True) for p in pre32]
    cot = [torch.from_numpy(np.array(c)).double() for c in cot32]
    beta = torch.tensor(float(BETA), dtype=torch.float64, requires_grad=True)
    s = act_derivs(name, pre[0], beta if name == "swish" else None)
    h = [s[0]]
    if S1:
        h += [s[1] * pre[1 + d] for d in range(3)]
        h += [s[2] * pre[1 + e0] * pre[1 + e1] + s[1] * pre[4 + p] for p, (e0, e1) in enumerate(pairs)]
    loss = sum((c * x).sum() for c, x in zip(cot, h))
    grads = torch.autograd.grad(loss, pre + ([beta] if name == "swish" else []), allow_unused=True)
    abar = [np.zeros(pre32[0].shape) if g is None else g.numpy() for g in grads[:len(pre)]]
    sn = [x.detach().numpy() for x in s]
    p64 = [p.detach().numpy() for p in pre]
    c64 = [c.numpy() for c in cot]
    f = floors(name, p64[0], sn[0])
    Fk = [np.maximum(np.abs(sn[k]), f[k]) for k in range(4)]
    Mh = [Fk[0]]
    Mab = [Fk[1] * np.abs(c64[0])]
    if S1:
        Mh += [Fk[1] * np.abs(p64[1 + d]) for d in range(3)]
        Mh += [Fk[2] * np.abs(p64[1 + e0] * p64[1 + e1]) + Fk[1] * np.abs(p64[4 + p]) for p, (e0, e1) in enumerate(pairs)]
        Mab[0] = Mab[0] + Fk[2] * sum(np.abs(p64[1 + d] * c64[1 + d]) for d in range(3))
        Md = [Fk[1] * np.abs(c64[1 + d]) for d in range(3)]
        tail = []
        for p, (e0, e1) in enumerate(pairs):
            u, v, hb = p64[1 + e0], p64[1 + e1], c64[4 + p]
            Mab[0] = Mab[0] + (Fk[3] * np.abs(u * v) + Fk[2] * np.abs(p64[4 + p])) * np.abs(hb)
            Md[e0] = Md[e0] + Fk[2] * np.abs(v * hb)
            Md[e1] = Md[e1] + Fk[2] * np.abs(u * hb)
            tail.append(Fk[1] * np.abs(hb))
        Mab += Md + tail
    out = dict(h=[x.detach().numpy() for x in h], abar=abar, Mh=Mh, Mabar=Mab, pairs=pairs)
    if name == "swish":
        # d/d beta and the fp64 sum of the absolute values of its terms (one term per element and stream)
        out["dbeta"] = float(grads[-1])
        out["dbeta_abs"] = _dbeta_abs(p64, c64, pairs)
    if shared:
        _ref[key] = out
    return out


def _dbeta_abs(p64, c64, pairs):
    """fp64 sum over elements and streams of |hbar_s * d h_s / d beta| (the closed forms of swish_beta_adj's comment)."""
    b = float(BETA)
    a = p64[0]
    z = b * a
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-z))
    q = sg * (1.0 - sg)
    c = 1.0 - 2.0 * sg
    m = q * (2.0 + z * c)
    b0, b1, b2 = a * a * q, a * m, m + z * q * (3.0 * c + z * (c * c - 2.0 * q))
    tot = np.abs(b0 * c64[0]).sum()
    if len(p64) > 1:
        tot += sum(np.abs(b1 * p64[1 + d] * c64[1 + d]).sum() for d in range(3))
        for p, (e0, e1) in enumerate(pairs):
            tot += (np.abs(b2 * p64[1 + e0] * p64[1 + e1] * c64[4 + p]) + np.abs(b1 * p64[4 + p] * c64[4 + p])).sum()
    return float(tot)


def stream_order(st):
    return 0 if st == 0 else (1 if st < 4 else 2)


def units(got, ref, M):
    """|got - ref| in units of 2^-24 * M (0 where both the error and M are 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, err / (U * M))


def maxima_by_order(got, ref, M):
    """[max units of the value stream, of the first-order streams, of the second-order streams] (None where absent)."""
    out = [None, None, None]
    for st in range(len(got)):
        u = float(np.max(units(got[st], ref[st], M[st])))
        k = stream_order(st)
        out[k] = u if out[k] is None else max(out[k], u)
    return out


def model_maxima(name, **kw):
    """{"fwd": [3], "adj": [3]}: the maxima model_fp32 (with the sensitivity knobs ``kw``) reaches over the stream sets."""
    s = model_fp32(name, sweep(), **kw)
    res = {"fwd": [0.0] * 3, "adj": [0.0] * 3}
    for direction, sets in (("fwd", FWD_SETS), ("adj", ADJ_SETS)):
        for S1, S2 in sets:
            pre, cot, pairs = case_inputs(S1, S2)
            ref = reference(name, S1, S2)
            if direction == "fwd":
                m = maxima_by_order(jet_fwd_fp32(s, pre, pairs), ref["h"], ref["Mh"])
            else:
                m = maxima_by_order(jet_adj_fp32(s, pre, cot, pairs), ref["abar"], ref["Mabar"])
            res[direction] = [a if b is None else max(a, b) for a, b in zip(res[direction], m)]
    return res


def model_dbeta_units(S1, S2):
    """The fp32 transcription of swish_beta_adj summed sequentially in fp32, in units of 2^-24 * the fp64 sum of |terms|."""
    pre, cot, pairs = case_inputs(S1, S2)
    ref = reference("swish", S1, S2)
    t = swish_beta_terms_fp32(pre[0], pre, cot, pairs).reshape(-1)
    total = float(np.cumsum(t, dtype=F)[-1])
    return abs(total - ref["dbeta"]) / (U * ref["dbeta_abs"])


if __name__ == "__main__":
    def up(x):       # 4 x, rounded up to three significant digits
        x = 4.0 * x
        if x == 0:
            return 0.0
        e = 10.0 ** (np.floor(np.log10(x)) - 2)
        return float(np.ceil(x / e) * e)

    lines, table = [], []
    for act in ACTS:
        mx = model_maxima(act)
        lines.append("    %-10s forward %s   adjoint %s" % (act, " / ".join("%.3g" % v for v in mx["fwd"]),
                                                          " / ".join("%.3g" % v for v in mx["adj"])))
        table.append('    "%s": {"fwd": (%s), "adj": (%s)},' % (act, ", ".join("%.3g" % up(v) for v in mx["fwd"]),
                                                                 ", ".join("%.3g" % up(v) for v in mx["adj"])))
    print("\n".join(lines))
    print("\n".join(table))
    db = {s: model_dbeta_units(*s) for s in ADJ_SETS}
    print("dbeta", db, {s: up(v) for s, v in db.items()})
