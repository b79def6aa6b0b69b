"""Host model of the residual evaluator and the loss kernels of csrc/residual.hip (k_residual_fwd, k_residual_bwd, k_loss_sum,
k_loss_grad): one opcode table and one interpreter for all 39 opcodes, shared by the host tests (tests/test_residual_*.py) and
the device tests (tests/test_gpu_residual_*.py).  Everything here is built once, shared and read-only.

``program(*ins)``                            assembles an stpde_res_ins program (pde._RES_DT).  The kernels index their value arrays
                                             with the operand fields unchecked, so a hand-written program is checked here: at most
                                             MAX_INS instructions, every operand (``operands``) an earlier instruction.
``run(prog, jets, x, dtype)``                interprets a program for all points at once.  With dtype = float32 every exact opcode
                                             (below) is the kernel's own IEEE operation in the kernel's order; with float64 it is
                                             the reference.
``adjoint(prog, jets, x, res_bar, dtype)``   the reverse sweep of k_residual_bwd, rule for rule in the same expression order
                                             (``(gi * v[i]) / v[b]`` for the divisor, ``(gi * 0.5) / v[i]`` for the square root,
                                             ``(gi * float(n)) * x^(n-1)`` for the integer power), every adjoint register starting
                                             at +0 and added into (or subtracted from), like the kernel's.
``torch_program(prog, jets, x)``             the same program as a torch graph made of torch's own operators (``**``, torch.sqrt,
                                             torch.maximum, torch.where, ...; sign and Heaviside as PDELayer's torch strategies
                                             evaluate them), so that torch.autograd differentiates it: the adjoint rules are
                                             checked against it, not against a second copy of themselves.

Exact opcodes.  The library is built with -ffp-contract=off and without fast-math, and HIP's fp32 divide and square root are
correctly rounded, so JET X CONST ADD SUB MUL DIV NEG ABS SQRT OUT, POWI (``_powi``: square-and-multiply on |n|, then 1 / r),
POWC with an integral constant, MIN MAX SIGN STEP and LT LE EQ NE AND OR NOT SEL STEPC are fixed sequences of IEEE operations,
comparisons and selects: the device must reproduce the float32 model bit for bit (``same_bits``; ``exact_case``).  The others
(SIN COS EXP LOG TANH TAN SINH COSH ASIN ACOS ATAN ATAN2 POW, POWC with a fraction) go through the device's math library; they are
held to the fp64 model on 32,768-point sweeps (``trans_case``), values in ulps (``ulp_err``) and adjoints in units of 2^-24 of the
sum of the absolute values of the adjoint's terms (``_TERMS``), within ``trans_bound`` of what torch's own float32 evaluation
reaches on the same sweep (``trans_yardstick``).

Conventions, all torch's and its autograd's (the host tests check them against torch's fp64 autograd):

* OUT is never an operand of a later instruction (pde._compile_residual_program memoises the operand, not the OUT), and the
  adjoint of OUT ignores the OUT's own adjoint register.  X and CONST are not differentiated.
* ABS: adjoint 0 at +-0 and NaN.  MIN / MAX: NaN propagates; the winner takes the cotangent, a tie (+0 and -0 tie) halves it, a
  NaN operand passes it to both.
* SIGN: sign(+-0) = +0, sign(NaN) = NaN; STEP: 1, 0, H(+-0) = 1/2, H(NaN) = NaN; STEPC: the same with H(+-0) = c.  Adjoint 0.
* POWC: x^c with the fp32 constant c, the integer part of c by POWI's multiplications and the fraction through the math library
  (``_powc``); adjoint g * (c * x^m), m = fp32(double(c) - 1), nothing where c == 0.
* POW: x^y; g * (y * x^(y-1)) into the base (nothing where y == 0), g * (x^y * log x) into the exponent (nothing where x == 0 and
  y >= 0).
* TAN g (1 + t^2), SINH g cosh, COSH g sinh, ASIN g / sqrt(1 - x^2), ACOS -g / sqrt(1 - x^2), ATAN g / (1 + x^2),
  ATAN2(a, b): d = a^2 + b^2, g b / d into a and -g a / d into b, nothing at a = b = 0.
* LT LE EQ NE: IEEE comparisons into a mask 1.0 / 0.0; a NaN operand gives 0.0, for NE 1.0.  A mask is never NaN.  AND OR NOT: on
  masks, an operand is true where it is != 0.
* SEL: a = mask, b = then | else << 16 (``sel``); value = mask != 0 ? v[then] : v[else].  Adjoint: the selected operand takes the
  cotangent, the other exactly +0 (a select, never cotangent * mask: a NaN cotangent does not reach the operand not taken).
  Nothing reaches a mask, the operands of a comparison or the operand of STEPC.

Losses: ``loss_elem`` / ``loss_grad`` are the expressions of the kernels in float32 (or float64: the reference), and
``loss_sum_bound`` is the relative bound the structure of k_loss_sum gives for a sum of non-negative terms.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
# the STPDE_RES_* enum of include/stpde_hip.h = pde._RES_OPS (asserted by tests/test_residual_model_host.py)
OPS = {name: k for k, name in enumerate(
    "JET X CONST ADD SUB MUL DIV NEG POWI SIN COS EXP LOG SQRT TANH ABS OUT "
    "TAN SINH COSH ASIN ACOS ATAN ATAN2 POWC POW MIN MAX SIGN STEP "
    "LT LE EQ NE AND OR NOT SEL STEPC".split())}
NAMES = {v: k for k, v in OPS.items()}
OPS_EXT = {n: k for n, k in OPS.items() if OPS["OUT"] < k <= OPS["STEP"]}           # only programs compiled with extended=True
OPS_COND = {n: k for n, k in OPS.items() if k > OPS["STEP"]}                          # ... and conditional=True hold these
DT = np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<f4")])             # = pde._RES_DT
MAX_INS = 192                                                                         # = pde._RES_MAX_INS
_LEAF = ("JET", "X", "CONST")
_BINARY = ("ADD", "SUB", "MUL", "DIV", "ATAN2", "POW", "MIN", "MAX", "LT", "LE", "EQ", "NE", "AND", "OR")
_UNARY = {"SIN": np.sin, "COS": np.cos, "EXP": np.exp, "LOG": np.log, "SQRT": np.sqrt, "TANH": np.tanh, "ABS": np.abs,
          "TAN": np.tan, "SINH": np.sinh, "COSH": np.cosh, "ASIN": np.arcsin, "ACOS": np.arccos, "ATAN": np.arctan}
EDGES = (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan)


def sel(then, other):
    """The b field of SEL."""
    return int(then) | int(other) << 16


def sel_operands(b):
    return b & 0xffff, b >> 16


def operands(name, a, b):
    """The value indices an instruction reads (POWI's b is its exponent)."""
    if name in _LEAF:
        return ()
    if name == "SEL":
        return (a,) + sel_operands(b)
    return (a, b) if name in _BINARY else (a,)


def program(*ins):
    """[(name, a, b, c) with trailing fields optional] -> a pde._RES_DT array, checked (see the module docstring)."""
    rows = []
    assert len(ins) <= MAX_INS
    for k, i in enumerate(ins):
        i = tuple(i) + (0, 0, 0.0)[len(i) - 1:]
        for o in operands(i[0], int(i[1]), int(i[2])):
            assert 0 <= o < k, (k, i)
        rows.append((OPS[i[0]], int(i[1]), int(i[2]), float(i[3])))
    return np.array(rows, dtype=DT)


# ---- the interpreter --------------------------------------------------------------------------------------------------------
def _powi(base, n, dtype):
    """res_ipow of csrc/residual.hip: square-and-multiply on |n|, then 1 / r when n < 0."""
    base = base.copy()
    r = np.ones_like(base)
    e = -n if n < 0 else n
    while e:
        if e & 1:
            r = r * base
        base = base * base
        e >>= 1
    return dtype(1) / r if n < 0 else r


def _powc_m(c, dtype):
    """The exponent of POWC's adjoint: double(c) - 1, rounded to fp32 by the kernel (and by torch for an fp32 tensor)."""
    m = np.float64(F(c)) - 1.0
    return dtype(F(m)) if dtype == F else dtype(m)


def _powc(x, c, dtype):
    """res_powc of csrc/residual.hip: x^c with c = n + f, n = trunc(c) -- the integer part by _powi (|x| under it when f != 0),
    times x^f through the math library unless f = 0."""
    c = np.float64(c)
    n = np.trunc(c)
    f = c - n
    if abs(n) > 64:
        return np.power(x, dtype(c))
    r = _powi(np.abs(x) if f != 0 else x, int(n), dtype)
    return r * np.power(x, dtype(f)) if f != 0 else r


def _step(x, h0, dtype):
    return np.where(x > dtype(0), dtype(1), np.where(x < dtype(0), dtype(0), np.where(x == dtype(0), h0, x)))


def _values(prog, jets, x, dtype):
    jets = np.asarray(jets, dtype=dtype)
    x = None if x is None else np.asarray(x, dtype=dtype)
    P = jets.shape[2]
    one, zero = dtype(1), dtype(0)
    v = []
    with np.errstate(all="ignore"):
        for op, a, b, c in prog.tolist():
            name = NAMES[op]
            if name == "JET":
                r = jets[a, b]
            elif name == "X":
                r = x[:, a]
            elif name == "CONST":
                r = np.full(P, F(c), dtype=dtype)        # the program holds fp32 constants
            elif name == "ADD":
                r = v[a] + v[b]
            elif name == "SUB":
                r = v[a] - v[b]
            elif name == "MUL":
                r = v[a] * v[b]
            elif name == "DIV":
                r = v[a] / v[b]
            elif name == "NEG":
                r = -v[a]
            elif name == "POWI":
                r = _powi(v[a], b, dtype)
            elif name == "OUT":
                r = v[a]
            elif name == "ATAN2":
                r = np.arctan2(v[a], v[b])
            elif name == "POWC":
                r = _powc(v[a], F(c), dtype)
            elif name == "POW":
                r = np.power(v[a], v[b])
            elif name == "MIN":
                r = np.where((v[a] < v[b]) | (v[a] != v[a]), v[a], v[b])
            elif name == "MAX":
                r = np.where((v[a] > v[b]) | (v[a] != v[a]), v[a], v[b])
            elif name == "SIGN":
                r = np.where(v[a] > zero, one, np.where(v[a] < zero, dtype(-1), np.where(v[a] == zero, zero, v[a])))
            elif name == "STEP":
                r = _step(v[a], dtype(0.5), dtype)
            elif name == "STEPC":
                r = _step(v[a], dtype(F(c)), dtype)
            elif name == "LT":
                r = np.where(v[a] < v[b], one, zero)
            elif name == "LE":
                r = np.where(v[a] <= v[b], one, zero)
            elif name == "EQ":
                r = np.where(v[a] == v[b], one, zero)
            elif name == "NE":
                r = np.where(v[a] != v[b], one, zero)
            elif name == "AND":
                r = np.where((v[a] != zero) & (v[b] != zero), one, zero)
            elif name == "OR":
                r = np.where((v[a] != zero) | (v[b] != zero), one, zero)
            elif name == "NOT":
                r = np.where(v[a] != zero, zero, one)
            elif name == "SEL":
                t, e = sel_operands(b)
                r = np.where(v[a] != zero, v[t], v[e])
            else:
                r = _UNARY[name](v[a])
            assert r.dtype == dtype, (name, r.dtype)
            v.append(r)
    return v


def run(prog, jets, x, dtype=np.float64):
    """The residuals [n_eq] of P points: jets [S, n_out, P], x [P, 3] or None.  Returned in the order of the OUT indices."""
    v = _values(prog, jets, x, dtype)
    out = {int(b): v[i] for i, (op, a, b, c) in enumerate(prog.tolist()) if NAMES[op] == "OUT"}
    return [out[k] for k in sorted(out)]


def adjoint(prog, jets, x, res_bar, dtype=np.float64):
    """d (sum res * res_bar) / d jets, the sweep of k_residual_bwd: res_bar [n_eq, P] -> jets_bar [S, n_out, P]."""
    v = _values(prog, jets, x, dtype)
    res_bar = np.asarray(res_bar, dtype=dtype)
    P = np.shape(jets)[2]
    g = [np.zeros(P, dtype=dtype) for _ in v]
    jets_bar = np.zeros(np.shape(jets), dtype=dtype)
    half, one, zero = dtype(0.5), dtype(1), dtype(0)
    with np.errstate(all="ignore"):
        for i in range(len(v) - 1, -1, -1):
            op, a, b, c = prog[i].tolist()
            name, gi = NAMES[op], g[i]
            if name == "OUT":
                g[a] = g[a] + res_bar[b]
            elif name == "JET":
                jets_bar[a, b] = jets_bar[a, b] + gi
            elif name == "ADD":
                g[a] = g[a] + gi
                g[b] = g[b] + gi
            elif name == "SUB":
                g[a] = g[a] + gi
                g[b] = g[b] - gi
            elif name == "MUL":
                g[a] = g[a] + gi * v[b]
                g[b] = g[b] + gi * v[a]
            elif name == "DIV":
                g[a] = g[a] + gi / v[b]
                g[b] = g[b] - (gi * v[i]) / v[b]
            elif name == "NEG":
                g[a] = g[a] - gi
            elif name == "POWI":
                if b != 0:
                    g[a] = g[a] + (gi * dtype(b)) * _powi(v[a], b - 1, dtype)
            elif name == "SIN":
                g[a] = g[a] + gi * np.cos(v[a])
            elif name == "COS":
                g[a] = g[a] - gi * np.sin(v[a])
            elif name == "EXP":
                g[a] = g[a] + gi * v[i]
            elif name == "LOG":
                g[a] = g[a] + gi / v[a]
            elif name == "SQRT":
                g[a] = g[a] + (gi * half) / v[i]
            elif name == "TANH":
                g[a] = g[a] + gi * (one - v[i] * v[i])
            elif name == "ABS":
                g[a] = g[a] + np.where(v[a] > zero, gi, np.where(v[a] < zero, -gi, zero))
            elif name == "TAN":
                g[a] = g[a] + gi * (one + v[i] * v[i])
            elif name == "SINH":
                g[a] = g[a] + gi * np.cosh(v[a])
            elif name == "COSH":
                g[a] = g[a] + gi * np.sinh(v[a])
            elif name == "ASIN":
                g[a] = g[a] + gi / np.sqrt(one - v[a] * v[a])
            elif name == "ACOS":
                g[a] = g[a] - gi / np.sqrt(one - v[a] * v[a])
            elif name == "ATAN":
                g[a] = g[a] + gi / (one + v[a] * v[a])
            elif name == "ATAN2":
                d = v[a] * v[a] + v[b] * v[b]
                both0 = (v[a] == zero) & (v[b] == zero)
                ga, gb = np.where(both0, zero, (gi * v[b]) / d), np.where(both0, zero, (gi * v[a]) / d)
                g[a] = g[a] + ga
                g[b] = g[b] - gb
            elif name == "POWC":
                if F(c) != 0:
                    g[a] = g[a] + gi * (dtype(F(c)) * _powc(v[a], _powc_m(c, dtype), dtype))
            elif name == "POW":
                gx = np.where(v[b] == zero, zero, gi * (v[b] * np.power(v[a], v[b] - one)))
                gy = gi * np.where((v[a] == zero) & (v[b] >= zero), zero, v[i] * np.log(v[a]))
                g[a] = g[a] + gx
                g[b] = g[b] + gy
            elif name in ("MIN", "MAX"):
                h = np.where(v[a] == v[b], gi * half, gi)
                lose_a, lose_b = (v[a] > v[b], v[a] < v[b]) if name == "MIN" else (v[a] < v[b], v[a] > v[b])
                ga, gb = np.where(lose_a, zero, h), np.where(lose_b, zero, h)
                g[a] = g[a] + ga
                g[b] = g[b] + gb
            elif name == "SEL":
                t, e = sel_operands(b)
                then = v[a] != zero
                g[t] = g[t] + np.where(then, gi, zero)
                g[e] = g[e] + np.where(then, zero, gi)
            else:       # adjoint 0: the coordinates, constants, SIGN STEP STEPC, masks and the operands of a comparison
                assert name in ("X", "CONST", "SIGN", "STEP") or name in OPS_COND, name
    assert jets_bar.dtype == dtype
    return jets_bar


def torch_program(prog, jets, x):
    """The program as a torch graph over the tensor jets [S, n_out, P] (x [P, 3] or None) -> residuals [n_eq] of [P]."""
    import torch
    from space_time_pde_amd import pde
    un = {"SIN": torch.sin, "COS": torch.cos, "EXP": torch.exp, "LOG": torch.log, "SQRT": torch.sqrt, "TANH": torch.tanh,
          "ABS": torch.abs, "TAN": torch.tan, "SINH": torch.sinh, "COSH": torch.cosh, "ASIN": torch.asin, "ACOS": torch.acos,
          "ATAN": torch.atan, "SIGN": pde._t_sign, "STEP": pde._t_heaviside}
    bi = {"ADD": torch.add, "SUB": torch.sub, "MUL": torch.mul, "DIV": torch.div, "ATAN2": torch.atan2, "POW": torch.pow,
          "MIN": torch.minimum, "MAX": torch.maximum}
    rel = {"LT": torch.lt, "LE": torch.le, "EQ": torch.eq, "NE": torch.ne}
    v, out = [], {}
    for op, a, b, c in prog.tolist():
        name = NAMES[op]
        if name == "JET":
            r = jets[a, b]
        elif name == "X":
            r = x[:, a]
        elif name == "CONST":
            r = torch.full((jets.shape[2],), float(F(c)), dtype=jets.dtype)
        elif name == "NEG":
            r = -v[a]
        elif name == "POWI":
            r = v[a] ** b
        elif name == "POWC":
            r = v[a] ** float(F(c))
        elif name == "OUT":
            r = v[a]
            out[b] = r
        elif name in rel:
            r = rel[name](v[a], v[b]).to(jets.dtype)
        elif name == "AND":
            r = torch.logical_and(v[a] != 0, v[b] != 0).to(jets.dtype)
        elif name == "OR":
            r = torch.logical_or(v[a] != 0, v[b] != 0).to(jets.dtype)
        elif name == "NOT":
            r = torch.logical_not(v[a] != 0).to(jets.dtype)
        elif name == "SEL":
            t, e = sel_operands(b)
            r = torch.where(v[a] != 0, v[t], v[e])
        elif name == "STEPC":
            r = pde._t_heaviside(v[a], float(F(c)))
        elif name in bi:
            r = bi[name](v[a], v[b])
        else:
            r = un[name](v[a])
        v.append(r)
    return [out[k] for k in sorted(out)]


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def same_bits(got, want):
    """Element-wise: bit-equal where ``want`` is not NaN (this covers the finite values, the sign of a zero and the sign of an
    infinity), NaN exactly where ``want`` is NaN (the payload is not compared)."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    nan = np.isnan(want)
    return np.where(nan, np.isnan(got), got.view(np.int32) == want.view(np.int32))


def bit_mismatches(got, want, limit=5):
    """Text for an assertion message: how many elements differ and the first few of them."""
    bad = np.argwhere(~same_bits(got, want))
    got, want = np.asarray(got), np.asarray(want)
    return "%d of %d differ; first: %s" % (len(bad), want.size, [(tuple(int(k) for k in i), float(got[tuple(i)]), float(want[tuple(i)]))
                                                                  for i in bad[:limit]])


def ulp_of(ref64):
    """The spacing of float32 at |ref64| (2^-149 at and below the subnormals)."""
    _, e = np.frexp(np.abs(np.asarray(ref64, dtype=np.float64)))
    return np.maximum(np.ldexp(1.0, e.astype(np.int64) - 24), 2.0 ** -149)


def units_err(got, ref64, unit):
    """|got - ref64| / unit element by element; 0 where both are the same infinity or both NaN, inf where only one is not
    finite, 0 where got == ref64 (so that a unit of 0 under an exact result does not matter)."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    fin = np.isfinite(got) & np.isfinite(ref64)
    with np.errstate(all="ignore"):
        err = np.where(got == ref64, 0.0, np.abs(got - ref64) / unit)
    same = (np.isnan(got) & np.isnan(ref64)) | (~fin & (got == ref64))
    return np.where(fin, err, np.where(same, 0.0, np.inf))


def ulp_err(got, ref64):
    """The error of a float32 result in float32 ulps of the fp64 reference, element by element."""
    return units_err(got, ref64, ulp_of(ref64))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
_cache = {}


def _once(key, make):
    """make(), built once per key and kept read-only: an array, or a tuple / dict of arrays (None allowed)."""
    if key not in _cache:
        out = make()
        for a in out.values() if isinstance(out, dict) else out if isinstance(out, tuple) else (out,):
            if a is not None:
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def normal_operands(n=4096, seed=0):
    """n float32 values, random sign, magnitude log-uniform in [1e-3, 1e3]."""
    def make():
        rng = np.random.default_rng(1000 + seed)
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)).astype(F)
    return _once(("normal", n, seed), make)


def unary_inputs(seed=0):
    """4096 normal-range values, then the seven edge values: [4103]."""
    return _once(("unary", seed), lambda: np.concatenate([normal_operands(4096, seed), np.array(EDGES, dtype=F)]))


def binary_inputs():
    """Two operands [4145]: 4096 independent normal-range pairs, then every pair of the seven edge values."""
    def make():
        e = np.array(EDGES, dtype=F)
        return np.stack([np.concatenate([normal_operands(4096, 0), np.repeat(e, 7)]),
                         np.concatenate([normal_operands(4096, 1), np.tile(e, 7)])])
    return _once(("binary",), make)


def cotangent(n, seed=7):
    return _once(("cot", n, seed), lambda: np.random.default_rng(2000 + seed).standard_normal(n).astype(F))


# ---- one small program per exact opcode -------------------------------------------------------------------------------------
POWI_EXPONENTS = (-3, -1, 0, 1, 2, 3, 7)
CONSTS = (0.1, -2.5, 0.0, -0.0, 1e-30, 3e38)
STEPC_VALUES = (1.0, 0.0, -2.5)
EXACT_CASES_BASE = ("JET", "X", "CONST", "ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQRT", "OUT") + \
    tuple("POWI_%d" % n for n in POWI_EXPONENTS)
EXACT_CASES_EXT = ("MIN", "MAX", "SIGN", "STEP", "POWC_1")
EXACT_CASES_COND = ("LT", "LE", "EQ", "NE", "AND", "OR", "NOT", "SEL", "SEL_NAN_DEFAULT", "SEL_DEAD_SQRT", "SEL_CHAIN") + \
    tuple("STEPC_%d" % k for k in range(len(STEPC_VALUES)))
EXACT_CASES = EXACT_CASES_BASE + EXACT_CASES_EXT + EXACT_CASES_COND
N_EDGE1, N_EDGE2 = len(EDGES), len(EDGES) ** 2


def edge_index(a, b=None):
    """The offset, from the end of unary_inputs() / binary_inputs(), of the edge row with operand a (and b): compare with
    ``is`` semantics for the two zeros and NaN."""
    def pos(v):
        for k, e in enumerate(EDGES):
            if (np.isnan(v) and np.isnan(e)) or (v == e and np.signbit(v) == np.signbit(e)):
                return k
        raise KeyError(v)
    return 4096 + (pos(a) if b is None else 7 * pos(a) + pos(b))


def _binary_with_ties():
    """The binary inputs with the first 64 pairs tied."""
    j = np.array(binary_inputs())
    j[1, :64] = j[0, :64]
    return j


def _exact_program(name):
    """(program, "unary" / "binary" / "ties": the jets of the case)."""
    if name in ("ADD", "SUB", "MUL", "DIV"):
        return program(("JET", 0, 0), ("JET", 0, 1), (name, 0, 1), ("OUT", 2, 0), (name, 1, 1), ("OUT", 4, 1)), "binary"
    if name == "JET":
        return program(("JET", 0, 1), ("JET", 0, 0), ("OUT", 0, 0), ("OUT", 1, 1)), "binary"
    if name == "X":
        return program(("JET", 0, 0), ("X", 2), ("X", 0), ("X", 1), ("OUT", 1, 0), ("OUT", 2, 1), ("OUT", 3, 2)), "unary"
    if name == "CONST":
        ins = [("JET", 0, 0)] + [("CONST", 0, 0, c) for c in CONSTS] + [("OUT", 1 + k, k) for k in range(len(CONSTS))]
        return program(*ins), "unary"
    if name == "OUT":
        return program(("JET", 0, 0), ("OUT", 0, 1), ("OUT", 0, 0)), "unary"
    if name.startswith("POWI_"):
        return program(("JET", 0, 0), ("POWI", 0, int(name[5:])), ("OUT", 1, 0)), "unary"
    if name in ("NEG", "ABS", "SQRT"):
        return program(("JET", 0, 0), (name, 0), ("OUT", 1, 0)), "unary"
    # MIN / MAX also of an operand with itself (a tie on every row); SIGN / STEP / STEPC also as a factor of their operand, so
    # that a cotangent passes the instruction
    if name in ("MIN", "MAX"):
        return program(("JET", 0, 0), ("JET", 0, 1), (name, 0, 1), ("OUT", 2, 0), (name, 1, 1), ("OUT", 4, 1), (name, 1, 0),
                       ("OUT", 6, 2)), "binary"
    if name in ("SIGN", "STEP"):
        return program(("JET", 0, 0), (name, 0), ("OUT", 1, 0), ("MUL", 1, 0), ("OUT", 3, 1)), "unary"
    if name.startswith("STEPC_"):
        c = STEPC_VALUES[int(name[6:])]
        return program(("JET", 0, 0), ("STEPC", 0, 0, c), ("OUT", 1, 0), ("MUL", 1, 0), ("OUT", 3, 1)), "unary"
    if name == "POWC_1":
        return program(("JET", 0, 0), ("POWC", 0, 0, 1.0), ("OUT", 1, 0)), "unary"
    # LT LE EQ NE: of (a, b), (b, a) and (b, b), and the mask as a factor of a so that a cotangent passes it
    if name in ("LT", "LE", "EQ", "NE"):
        return program(("JET", 0, 0), ("JET", 0, 1), (name, 0, 1), ("OUT", 2, 0), (name, 1, 0), ("OUT", 4, 1), (name, 1, 1),
                       ("OUT", 6, 2), ("MUL", 2, 0), ("OUT", 8, 3)), "ties"
    # AND OR NOT: of the masks a <= b and b <= a (both true on a tie, both false with a NaN), again also as factors
    if name in ("AND", "OR", "NOT"):
        ins = [("JET", 0, 0), ("JET", 0, 1), ("LE", 0, 1), ("LE", 1, 0), (name, 2) if name == "NOT" else (name, 2, 3),
               ("OUT", 4, 0), ("MUL", 4, 0), ("OUT", 6, 1)]
        if name != "NOT":
            ins += [(name, 3, 3), ("OUT", 8, 2)]
        return program(*ins), "ties"
    if name == "SEL":                    # a < b ? a : b, then b <= a ? a * b : a
        return program(("JET", 0, 0), ("JET", 0, 1), ("LT", 0, 1), ("SEL", 2, sel(0, 1)), ("OUT", 3, 0),
                       ("LE", 1, 0), ("MUL", 0, 1), ("SEL", 5, sel(6, 0)), ("OUT", 7, 1)), "ties"
    if name == "SEL_NAN_DEFAULT":        # a chain that ends in CONST NaN
        return program(("JET", 0, 0), ("JET", 0, 1), ("CONST", 0, 0, np.nan), ("EQ", 0, 1), ("SEL", 3, sel(1, 2)),
                       ("LT", 0, 1), ("SEL", 5, sel(0, 4)), ("OUT", 6, 0)), "ties"
    if name == "SEL_DEAD_SQRT":          # a > 0 ? sqrt(a) : 0: the dead branch at a = 0 turns its zero cotangent into NaN, as torch's
        return program(("JET", 0, 0), ("CONST", 0, 0, 0.0), ("LT", 1, 0), ("SQRT", 0), ("SEL", 2, sel(3, 1)), ("OUT", 4, 0)), "unary"
    assert name == "SEL_CHAIN", name     # three branches over AND / OR / NOT masks
    return program(("JET", 0, 0), ("JET", 0, 1), ("CONST", 0, 0, 0.0), ("LT", 2, 0), ("LT", 2, 1), ("AND", 3, 4), ("OR", 3, 4),
                   ("NOT", 6), ("NE", 0, 0), ("OR", 7, 8), ("MUL", 0, 1), ("SUB", 0, 1), ("NEG", 0),
                   ("SEL", 9, sel(12, 11)), ("SEL", 5, sel(10, 13)), ("OUT", 14, 0)), "ties"


def exact_case(name):
    """(prog, jets [1, n_out, P] float32, x [P, 3] float32 or None, res_bar [n_eq, P] float32) of one case of EXACT_CASES: 4096
    normal-range rows (unary_inputs / binary_inputs; the LT .. SEL cases with 64 tied pairs) with a random cotangent, then every
    (pair of) edge value(s) 0, -0, 1, -1, +-Inf, NaN with cotangent 1.  The SEL cases also carry NaN, +Inf and -Inf cotangents in
    turn on every fifth row of residual 0, normal-range and edge rows alike: they land on either side of a select."""
    def make():
        prog, inputs = _exact_program(name)
        if inputs == "unary":
            jets, n_edge = unary_inputs(0)[None, None], N_EDGE1
            if name == "SQRT":                  # positive normal-range arguments; the edge rows keep their signs
                jets = np.concatenate([np.abs(jets[..., :4096]), jets[..., 4096:]], -1)
        else:
            jets, n_edge = (_binary_with_ties() if inputs == "ties" else binary_inputs())[None], N_EDGE2
        x = np.ascontiguousarray(np.stack([unary_inputs(k) for k in (1, 2, 3)], 1)) if name == "X" else None
        seed = 11 if name in EXACT_CASES_BASE else 13 if name in EXACT_CASES_EXT else 17 + EXACT_CASES_COND.index(name)
        n_eq, P = int((prog["op"] == OPS["OUT"]).sum()), jets.shape[2]
        cot = np.array(cotangent(n_eq * P, seed).reshape(n_eq, P))
        cot[:, P - n_edge:] = 1.0
        if name.startswith("SEL"):
            for k, val in enumerate((np.nan, np.inf, -np.inf)):
                cot[0, 5 * k + 2::15] = val
        return prog, np.ascontiguousarray(jets, dtype=F), x, cot
    return _once(("exact", name), make)


def mixed_case():
    """dict(prog, jets [1, 2, 257], x [257, 3], cot [2, 257]): two residuals that use every opcode of OPS_COND, the coordinates
    and a constant branch; exact zeros and ties in the first rows.  Every opcode in it is an exact one (bit-equal on the device)."""
    def make():
        prog = program(
            ("JET", 0, 0), ("JET", 0, 1), ("X", 2), ("CONST", 0, 0, 0.0), ("CONST", 0, 0, 0.25),
            ("LT", 3, 0),                      # 5: u > 0
            ("LE", 2, 1),                      # 6: x <= w
            ("EQ", 0, 1),                      # 7: u == w
            ("NE", 2, 3),                      # 8: x != 0
            ("AND", 5, 6), ("OR", 7, 9), ("NOT", 8),      # 9, 10, 11
            ("MUL", 0, 1), ("ABS", 2),         # 12: u w   13: |x|
            ("SEL", 11, sel(4, 13)),           # 14: x == 0 ? 0.25 : |x|
            ("SEL", 10, sel(12, 14)),          # 15
            ("OUT", 15, 0),
            ("STEPC", 0, 0, 1.0), ("STEPC", 1, 0, -0.5), ("MUL", 17, 1), ("ADD", 19, 18),
            ("SEL", 6, sel(20, 0)),            # 21
            ("OUT", 21, 1))
        rng = np.random.default_rng(23)
        jets = rng.uniform(-1, 1, (1, 2, 257)).astype(F)
        x = rng.uniform(-1, 1, (257, 3)).astype(F)
        jets[0, 0, :3] = 0.0                   # H(0) of STEPC
        jets[0, 1, 3:6] = jets[0, 0, 3:6]      # u == w
        x[6:9, 2] = 0.0                        # x == 0
        x[9:12, 2] = jets[0, 1, 9:12]          # x == w
        assert set(prog["op"].tolist()) >= set(OPS_COND.values())
        return dict(prog=prog, jets=jets, x=x, cot=rng.standard_normal((2, 257)).astype(F))
    return _once(("mixed",), make)


def chain_program(nins=MAX_INS):
    """A program of exactly nins exact-opcode instructions: two jets and a constant, then a chain that keeps its values in
    range (every round halves, takes a root and divides), an OUT every 37 instructions and at the end."""
    ins = [("JET", 0, 0), ("JET", 1, 0), ("CONST", 0, 0, 1.5)]
    t, k, n_eq = 0, 0, 0
    steps = [lambda t: ("ADD", t, 0), lambda t: ("MUL", t, 2), lambda t: ("SUB", t, 1), lambda t: ("ABS", t),
             lambda t: ("SQRT", t), lambda t: ("DIV", t, 2), lambda t: ("NEG", t), lambda t: ("POWI", t, 2),
             lambda t: ("ADD", t, 1), lambda t: ("POWI", t, -1), lambda t: ("MUL", t, 0), lambda t: ("POWI", t, 3),
             lambda t: ("ABS", t), lambda t: ("SQRT", t)]
    while len(ins) < nins - 1:
        if len(ins) % 37 == 36:
            ins.append(("OUT", t, n_eq))
            n_eq += 1
        else:
            ins.append(steps[k % len(steps)](t))
            t = len(ins) - 1
            k += 1
    ins.append(("OUT", t, n_eq))
    assert len(ins) == nins
    return program(*ins), n_eq + 1


# ---- sweeps of the opcodes that go through the math library -----------------------------------------------------------------
SWEEP_N = 32768
SWEEP_RANGE = {"SIN": (-8.0, 8.0), "COS": (-8.0, 8.0), "EXP": (-20.0, 20.0), "LOG": (1e-3, 1e3), "TANH": (-10.0, 10.0)}
POWC_EXPONENTS = (1.0 / 3.0, 4.0 / 3.0, 1.5, 2.5, -0.5)
TRANS_CASES_BASE = tuple(SWEEP_RANGE)
TRANS_CASES_EXT = ("TAN", "ATAN", "ATAN2", "SINH", "COSH", "ASIN", "ACOS") + tuple("POWC_%d" % k for k in range(len(POWC_EXPONENTS))) + \
    ("POW", "SINH_TOP", "COSH_TOP")
SINH_MAX = 89.4          # sinh and cosh overflow float32 just above (89.416)
EXP_MAX = 88.72          # exp overflows float32 just above (88.7228): torch's vectorised float32 sinh / cosh return Inf from there
# Per opcode, the fp64 sum of the absolute values of the terms of its adjoint expression in k_residual_bwd, for every operand:
# (operands x [n_in, N], |cotangent| g [N], the instruction's constant c) -> [N] or [n_in, N].  2^-24 of it is the adjoint's unit.
_TERMS = {
    "SIN": lambda x, g, c: g * np.abs(np.cos(x[0])),
    "COS": lambda x, g, c: g * np.abs(np.sin(x[0])),
    "EXP": lambda x, g, c: g * np.exp(x[0]),
    "LOG": lambda x, g, c: g / np.abs(x[0]),
    "TANH": lambda x, g, c: g * (1.0 + np.tanh(x[0]) ** 2),                 # g * (1 - t * t): the terms g and g t t
    "TAN": lambda x, g, c: g * (1.0 + np.tan(x[0]) ** 2),                   # the terms g and g t t
    "ATAN": lambda x, g, c: g / (1.0 + x[0] ** 2),
    "ATAN2": lambda x, g, c: np.stack([g * np.abs(x[1]) / (x[0] ** 2 + x[1] ** 2), g * np.abs(x[0]) / (x[0] ** 2 + x[1] ** 2)]),
    "SINH": lambda x, g, c: g * np.cosh(x[0]),
    "COSH": lambda x, g, c: g * np.abs(np.sinh(x[0])),
    "ASIN": lambda x, g, c: g / np.sqrt(1.0 - x[0] ** 2),
    "ACOS": lambda x, g, c: g / np.sqrt(1.0 - x[0] ** 2),
    "POWC": lambda x, g, c: g * np.abs(c) * x[0] ** (c - 1.0),
    "POW": lambda x, g, c: np.stack([g * np.abs(x[1]) * x[0] ** (x[1] - 1.0), g * x[0] ** x[1] * np.abs(np.log(x[0]))]),
}


def _signed_decades(rng, n, lo, hi):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)


def _near(points, k=4):
    """Every float32 within k ulps of each point."""
    out = []
    for p in points:
        lo = hi = F(p)
        out.append(lo)
        for _ in range(k):
            lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
            out += [lo, hi]
    return np.array(out, dtype=F)


def trans_case(name):
    """(prog, jets [1, n_in, SWEEP_N] float32, cot [1, SWEEP_N] float32) of one sweep of TRANS_CASES_BASE or TRANS_CASES_EXT.

    SIN COS EXP LOG TANH: both ends of SWEEP_RANGE (for tanh also +-0 and the first saturated arguments), then a seeded fill,
    uniform (log-uniform for log).  TAN: 1e-4..1e4 in magnitude with the floats around the first eight poles; ATAN: 1e-6..1e6;
    ATAN2: both operands 1e-3..1e3, every sign pattern; SINH / COSH: up to +-EXP_MAX, both ends and the small arguments included,
    and SINH_TOP / COSH_TOP: the last stretch EXP_MAX..SINH_MAX up to the float32 overflow of sinh itself (cotangent / 8, so that
    the adjoint stays finite in float32); ASIN / ACOS: [-1, 1] with both ends, their neighbours and 0; POWC: bases 1e-3..1e3 for
    each exponent of POWC_EXPONENTS; POW: the same bases, exponents uniform in [-4, 4]."""
    def make():
        n = SWEEP_N
        unary = lambda op: program(("JET", 0, 0), (op, 0), ("OUT", 1, 0))                              # noqa: E731
        if name in TRANS_CASES_BASE:
            lo, hi = SWEEP_RANGE[name]
            head = [lo, hi]
            if name == "TANH":
                head += [0.0, -0.0, 9.0, -9.0, 9.5, -9.5, 1e-30, -1e-30, 1e-4, -1e-4]
            rng = np.random.default_rng(3000 + OPS[name])
            m = n - len(head)
            fill = np.exp(rng.uniform(np.log(lo), np.log(hi), m)) if name == "LOG" else rng.uniform(lo, hi, m)
            a = np.concatenate([np.array(head), fill]).astype(F)[None]
            if name == "LOG":
                a = np.clip(a, F(lo), F(hi))
            return unary(name), np.ascontiguousarray(a[None]), np.array(cotangent(n, OPS[name]))[None]
        rng = np.random.default_rng(4000 + TRANS_CASES_EXT.index(name))
        cot = np.array(cotangent(n, 40 + TRANS_CASES_EXT.index(name)))
        if name == "TAN":
            head = _near([(k + 0.5) * np.pi * s for k in range(8) for s in (1, -1)])
            a = np.concatenate([head, [0.0, -0.0], _signed_decades(rng, n - len(head) - 2, -4, 4)])[None]
            prog = unary("TAN")
        elif name == "ATAN":
            a = np.concatenate([[0.0, -0.0, 1.0, -1.0], _signed_decades(rng, n - 4, -6, 6)])[None]
            prog = unary("ATAN")
        elif name == "ATAN2":
            a = np.stack([_signed_decades(rng, n, -3, 3), _signed_decades(rng, n, -3, 3)])
            prog = program(("JET", 0, 0), ("JET", 0, 1), ("ATAN2", 0, 1), ("OUT", 2, 0))
        elif name in ("SINH", "COSH"):
            head = [EXP_MAX, -EXP_MAX, 0.0, -0.0, 1e-30, -1e-30, 1e-4, -1e-4]
            small = _signed_decades(rng, n // 4, -5, 0)
            a = np.concatenate([head, small, rng.uniform(-EXP_MAX, EXP_MAX, n - len(head) - len(small))])[None]
            a = np.clip(a.astype(F), F(-EXP_MAX), F(EXP_MAX))
            cot = cot * F(0.125)
            prog = unary(name)
        elif name in ("SINH_TOP", "COSH_TOP"):
            head = [SINH_MAX, -SINH_MAX, EXP_MAX, -EXP_MAX]
            a = np.concatenate([head, rng.choice([-1.0, 1.0], n - 4) * rng.uniform(EXP_MAX, SINH_MAX, n - 4)])[None]
            a = np.sign(a) * np.clip(np.abs(a).astype(F), F(EXP_MAX), F(SINH_MAX))
            cot = cot * F(0.125)
            prog = unary(name[:4])
        elif name in ("ASIN", "ACOS"):
            head = np.concatenate([_near([1.0, -1.0, 0.0]), [-0.0]])
            head = head[np.abs(head) <= 1]
            a = np.concatenate([head, rng.uniform(-1.0, 1.0, n - len(head))])[None]
            a = np.clip(a.astype(F), F(-1), F(1))
            prog = unary(name)
        elif name.startswith("POWC_"):
            a = np.concatenate([[1e-3, 1e3, 1.0], 10.0 ** rng.uniform(-3, 3, n - 3)])[None]
            prog = program(("JET", 0, 0), ("POWC", 0, 0, POWC_EXPONENTS[int(name[5:])]), ("OUT", 1, 0))
        else:
            assert name == "POW", name
            a = np.stack([10.0 ** rng.uniform(-3, 3, n), np.concatenate([[-4.0, 4.0, 0.0, 1.0], rng.uniform(-4, 4, n - 4)])])
            prog = program(("JET", 0, 0), ("JET", 0, 1), ("POW", 0, 1), ("OUT", 2, 0))
        jets = np.ascontiguousarray(a[None], dtype=F)
        assert jets.shape == (1, len(a), n), jets.shape
        return prog, jets, np.ascontiguousarray(cot[None], dtype=F)
    return _once(("sweep", name), make)


def trans_reference(name):
    """(prog, jets32, cot32, value64 [SWEEP_N], adjoint64 [n_in, SWEEP_N], adjoint units [n_in, SWEEP_N]) of one sweep: the fp64
    model of the program and of its adjoint on the float32 inputs; unit = 2^-24 * _TERMS of the swept instruction."""
    prog, jets, cot = trans_case(name)
    val, = run(prog, jets.astype(np.float64), None, np.float64)
    adj = adjoint(prog, jets.astype(np.float64), None, cot.astype(np.float64), np.float64)[0]
    op, _, _, c = prog[-2].tolist()
    with np.errstate(all="ignore"):
        terms = _TERMS[NAMES[op]](jets[0].astype(np.float64), np.abs(cot[0].astype(np.float64)), np.float64(F(c)))
    return prog, jets, cot, val, adj, U * np.atleast_2d(terms)


def trans_errors(name, value32, adjoint32):
    """(max value error in ulps, max adjoint error in adjoint units) of a float32 evaluation of the sweep (value [SWEEP_N],
    adjoint [n_in, SWEEP_N]) against the fp64 model."""
    _, _, _, val, adj, unit = trans_reference(name)
    return float(ulp_err(value32, val).max()), float(units_err(adjoint32, adj, unit).max())


def trans_yardstick(name):
    """What torch's own float32 CPU evaluation of the opcode (torch_program: torch.sin, ``**``, torch.pow, ...) and its autograd
    reach on the same sweep against the same fp64 reference: (value, adjoint).  SINH_TOP / COSH_TOP have none of their own --
    torch's vectorised float32 sinh and cosh take exp(|x|), which is Inf on that whole stretch -- and take that of SINH / COSH."""
    import torch
    if name.endswith("_TOP"):
        return trans_yardstick(name[:4])
    prog, jets, cot = trans_case(name)
    jt = torch.from_numpy(np.array(jets)).requires_grad_(True)
    y, = torch_program(prog, jt, None)
    y.backward(torch.from_numpy(np.array(cot[0])))
    return trans_errors(name, y.detach().numpy(), jt.grad.numpy()[0])


def trans_bound(yardstick):
    """What the device may reach: 4 x max(1, yardstick) -- the margin tests/act_jet_model.py gives a correctly rounded
    transcription."""
    return 4.0 * max(1.0, yardstick)


# ---- the all-opcode equation set ------------------------------------------------------------------------------------------
ALL_OPS_VARS = ("x, y, t", "c, u, v, w, p")
ALL_OPS_EQUATIONS = (
    ("exp(-u**2)*cos(v) - tanh(w)/(2 + sin(c))", "transcendental"),
    ("Abs(dif(u,x)) - log(1 + c**2)", "abs_log"),
    ("-dif(v,y) - dif(w,t)", "all_negative"),
    ("1/sqrt(2 + u**2) + p**-2 + x*dif(p,x)", "rsqrt_negpow"),
    ("-u", "neg"),
)


def all_ops_layer():
    from space_time_pde_amd import pde
    layer = pde.PDELayer(*ALL_OPS_VARS)
    for eq, name in ALL_OPS_EQUATIONS:
        layer.add_equation(eq, name)
    return layer


def all_ops_streams(layer):
    """{multi-index: stream} the way PDELayer._residues_from_jets numbers the streams."""
    req_pairs = sorted({mi for prog in layer.eqns_jet.values() for _, mi in prog.atoms if len(mi) == 2})
    stream_of = {(): 0, (0,): 1, (1,): 2, (2,): 3}
    for k, pr in enumerate(req_pairs):
        stream_of[pr] = 4 + k
    return stream_of


def all_ops_program(layer):
    """(program, uses_x, stream_of) of the layer's equations, compiled the way PDELayer._residues_hip compiles them."""
    from space_time_pde_amd import pde
    progs = layer.eqns_jet
    assert all(p is not None for p in progs.values())
    stream_of = all_ops_streams(layer)
    slots = {sym: (stream_of[k[1]], k[0]) for p in progs.values() for k, sym in p.syms.items()}
    comp = pde._compile_residual_program([p.expr for p in progs.values()], list(layer.in_vars), slots)
    assert comp is not None
    return comp[0], comp[1], stream_of


# ---- loss kernels ---------------------------------------------------------------------------------------------------------
LOSS_KINDS = ("l1", "l2", "huber")


def loss_diff(a, b, dtype=F):
    a = np.asarray(a, dtype=dtype)
    return a - (dtype(0) if b is None else np.asarray(b, dtype=dtype))


def loss_elem(kind, d):
    """loss_elem of csrc/residual.hip in the dtype of d."""
    t = d.dtype.type
    with np.errstate(all="ignore"):
        ad = np.abs(d)
        if kind == "l1":
            return ad
        if kind == "l2":
            return d * d
        return np.where(ad < t(1), t(0.5) * d * d, ad - t(0.5))


def loss_grad(kind, d, g):
    """k_loss_grad: g * f'(d) in the dtype of d.  f'(NaN) is 0 for l1 (torch's sign) and NaN for l2 and huber."""
    t = d.dtype.type
    with np.errstate(all="ignore"):
        if kind == "l1":
            f = np.where(d > t(0), t(1), np.where(d < t(0), t(-1), t(0)))
        elif kind == "l2":
            f = t(2) * d
        else:
            f = np.where(d >= t(1), t(1), np.where(d <= t(-1), t(-1), d))
        return t(g) * f


def loss_blocks(n, cap=1024):
    return min((n + 1023) // 1024, cap)


def loss_sum_bound(n, det):
    """Relative bound of k_loss_sum on a sum of non-negative terms: every thread chains ceil(n / (256 blocks)) additions, the wave
    and block tree adds 6 + 2 levels, and every block adds its sum with one fp32 atomic (blocks more roundings) -- or, in
    deterministic mode, exactly into the long accumulator, which is rounded to fp32 once."""
    blocks = loss_blocks(n)
    chain = -(-n // (256 * blocks))
    return (chain + 9) * U if det else (chain + 8 + blocks) * U
