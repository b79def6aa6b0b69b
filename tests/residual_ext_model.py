"""Host model of the opcodes appended to the residual evaluator of csrc/residual.hip after OUT (TAN SINH COSH ASIN ACOS ATAN ATAN2
POWC POW MIN MAX SIGN STEP), shared by tests/test_residual_ext_host.py and tests/test_gpu_residual_ext.py.  It extends
tests/residual_model.py (imported as ``M``, not edited): the same program layout, the same interpreter over all points at once
-- the 17 opcodes of M with M's own expressions -- and M's comparisons (``ulp_err``, ``units_err``, ``same_bits``,
``trans_bound``).

``run`` / ``adjoint`` / ``torch_program`` are those of M for programs that may hold the appended opcodes.  With dtype = float32,
MIN MAX SIGN STEP are the kernel's own comparisons and selects (fixed IEEE sequences: the device must be bit-equal); the others go
through the math library, so the float64 model is their reference and they are held to it in ulps / adjoint units like SIN COS EXP
LOG TANH.  Conventions, all torch's (tests/test_residual_ext_host.py checks the adjoints against torch's fp64 autograd):

* MIN / MAX: NaN propagates; the winner takes the cotangent, a tie (+0 and -0 tie) halves it, a NaN operand passes it to both.
* SIGN: sign(+-0) = +0, sign(NaN) = NaN; STEP: 1, 0, H(+-0) = 1/2, H(NaN) = NaN; both have adjoint 0.
* POWC: x^c with the fp32 constant c, the integer part of c by POWI's multiplications and the fraction through the math library
  (``_powc``: an integral c is an exact opcode); adjoint g * (c * x^m), m = fp32(double(c) - 1), nothing where c == 0.
* POW: x^y; g * (y * x^(y-1)) into the base (nothing where y == 0), g * (x^y * log x) into the exponent (nothing where x == 0 and
  y >= 0).
* TAN g (1 + t^2), SINH g cosh, COSH g sinh, ASIN g / sqrt(1 - x^2), ACOS -g / sqrt(1 - x^2), ATAN g / (1 + x^2),
  ATAN2(a, b): d = a^2 + b^2, g b / d into a and -g a / d into b, nothing at a = b = 0.
"""
import numpy as np

from tests import residual_model as M

F = M.F
U = M.U
OPS_EXT = {"TAN": 17, "SINH": 18, "COSH": 19, "ASIN": 20, "ACOS": 21, "ATAN": 22, "ATAN2": 23, "POWC": 24, "POW": 25,
           "MIN": 26, "MAX": 27, "SIGN": 28, "STEP": 29}                                  # = pde._RES_OPS_EXT
OPS = dict(M.OPS, **OPS_EXT)
NAMES = {v: k for k, v in OPS.items()}
_UNARY = dict(M._UNARY, TAN=np.tan, SINH=np.sinh, COSH=np.cosh, ASIN=np.arcsin, ACOS=np.arccos, ATAN=np.arctan)


def program(*ins):
    """[(name, a, b, c) with trailing fields optional] -> a pde._RES_DT array (M.program with the appended opcodes)."""
    rows = []
    for i in ins:
        i = tuple(i) + (0, 0, 0.0)[len(i) - 1:]
        rows.append((OPS[i[0]], int(i[1]), int(i[2]), float(i[3])))
    return np.array(rows, dtype=M.DT)


def _sign(x, dtype):
    return np.where(x > dtype(0), dtype(1), np.where(x < dtype(0), dtype(-1), np.where(x == dtype(0), dtype(0), x)))


def _step(x, dtype):
    return np.where(x > dtype(0), dtype(1), np.where(x < dtype(0), dtype(0), np.where(x == dtype(0), dtype(0.5), x)))


def _powc_m(c, dtype):
    """The exponent of POWC's adjoint: double(c) - 1, rounded to fp32 by the kernel (and by torch for an fp32 tensor)."""
    m = np.float64(F(c)) - 1.0
    return dtype(F(m)) if dtype == F else dtype(m)


def _powc(x, c, dtype):
    """res_powc of csrc/residual.hip: x^c with c = n + f, n = trunc(c) -- the integer part by M._powi (|x| under it when f != 0),
    times x^f through the math library unless f = 0."""
    c = np.float64(c)
    n = np.trunc(c)
    f = c - n
    if abs(n) > 64:
        return np.power(x, dtype(c))
    r = M._powi(np.abs(x) if f != 0 else x, int(n), dtype)
    return r * np.power(x, dtype(f)) if f != 0 else r


def _values(prog, jets, x, dtype):
    jets = np.asarray(jets, dtype=dtype)
    x = None if x is None else np.asarray(x, dtype=dtype)
    P = jets.shape[2]
    v = []
    with np.errstate(all="ignore"):
        for op, a, b, c in prog.tolist():
            name = NAMES[op]
            if name == "JET":
                r = jets[a, b]
            elif name == "X":
                r = x[:, a]
            elif name == "CONST":
                r = np.full(P, F(c), dtype=dtype)
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
                r = M._powi(v[a], b, dtype)
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
                r = _sign(v[a], dtype)
            elif name == "STEP":
                r = _step(v[a], dtype)
            else:
                r = _UNARY[name](v[a])
            assert r.dtype == dtype, (name, r.dtype)
            v.append(r)
    return v


def run(prog, jets, x, dtype=np.float64):
    """The residuals [n_eq] of P points: jets [S, n_out, P], x [P, 3] or None, in the order of the OUT indices."""
    v = _values(prog, jets, x, dtype)
    out = {int(b): v[i] for i, (op, a, b, c) in enumerate(prog.tolist()) if NAMES[op] == "OUT"}
    return [out[k] for k in sorted(out)]


def adjoint(prog, jets, x, res_bar, dtype=np.float64):
    """The sweep of k_residual_bwd: res_bar [n_eq, P] -> jets_bar [S, n_out, P]; the 17 opcodes of M by M's rules."""
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
                    g[a] = g[a] + (gi * dtype(b)) * M._powi(v[a], b - 1, dtype)
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
            # X, CONST: not differentiated on this path; SIGN, STEP: adjoint 0
    assert jets_bar.dtype == dtype
    return jets_bar


def torch_program(prog, jets, x):
    """The program as a torch graph of torch's own operators (torch.maximum, torch.pow, torch.atan2, ...; sign and Heaviside
    as PDELayer's torch strategies evaluate them), for torch.autograd to differentiate: residuals [n_eq] of [P]."""
    import torch
    from space_time_pde_amd import pde
    un = {"SIN": torch.sin, "COS": torch.cos, "EXP": torch.exp, "LOG": torch.log, "SQRT": torch.sqrt, "TANH": torch.tanh,
          "ABS": torch.abs, "TAN": torch.tan, "SINH": torch.sinh, "COSH": torch.cosh, "ASIN": torch.asin, "ACOS": torch.acos,
          "ATAN": torch.atan, "SIGN": pde._t_sign, "STEP": pde._t_heaviside}
    bi = {"ADD": torch.add, "SUB": torch.sub, "MUL": torch.mul, "DIV": torch.div, "ATAN2": torch.atan2, "POW": torch.pow,
          "MIN": torch.minimum, "MAX": torch.maximum}
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
        elif name in bi:
            r = bi[name](v[a], v[b])
        else:
            r = un[name](v[a])
        v.append(r)
    return [out[k] for k in sorted(out)]


# ---- exact cases: MIN MAX SIGN STEP and POWC with c = 1 -------------------------------------------------------------------------
EXACT_CASES = ("MIN", "MAX", "SIGN", "STEP", "POWC_1")


def exact_case(name):
    """(prog, jets [1, n_out, P] float32, res_bar [n_eq, P] float32): M's 4096 normal-range rows with a random cotangent, then
    every (pair of) edge value(s) 0, -0, 1, -1, +-Inf, NaN with cotangent 1.  MIN / MAX also of an operand with itself (a tie on
    every row); SIGN / STEP also as a factor of their operand, so that a cotangent passes the instruction."""
    if name in ("MIN", "MAX"):
        prog = program(("JET", 0, 0), ("JET", 0, 1), (name, 0, 1), ("OUT", 2, 0), (name, 1, 1), ("OUT", 4, 1), (name, 1, 0),
                       ("OUT", 6, 2))
        jets, n_edge = M.binary_inputs()[None], M.N_EDGE2
    elif name in ("SIGN", "STEP"):
        prog = program(("JET", 0, 0), (name, 0), ("OUT", 1, 0), ("MUL", 1, 0), ("OUT", 3, 1))
        jets, n_edge = M.unary_inputs(0)[None, None], M.N_EDGE1
    else:
        prog = program(("JET", 0, 0), ("POWC", 0, 0, 1.0), ("OUT", 1, 0))
        jets, n_edge = M.unary_inputs(0)[None, None], M.N_EDGE1
    n_eq = int((prog["op"] == OPS["OUT"]).sum())
    P = jets.shape[2]
    cot = np.array(M.cotangent(n_eq * P, 13).reshape(n_eq, P))
    cot[:, P - n_edge:] = 1.0
    return prog, np.ascontiguousarray(jets, dtype=F), cot


# ---- sweeps of the opcodes that go through the math library -----------------------------------------------------------------------
SWEEP_N = M.SWEEP_N
POWC_EXPONENTS = (1.0 / 3.0, 4.0 / 3.0, 1.5, 2.5, -0.5)
TRANS_CASES = ("TAN", "ATAN", "ATAN2", "SINH", "COSH", "ASIN", "ACOS") + tuple("POWC_%d" % k for k in range(len(POWC_EXPONENTS))) + \
    ("POW", "SINH_TOP", "COSH_TOP")
SINH_MAX = 89.4          # sinh and cosh overflow float32 just above (89.416)
EXP_MAX = 88.72          # exp overflows float32 just above (88.7228): torch's vectorised float32 sinh / cosh return Inf from there
_sweeps = {}             # built once, read-only


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
    """(prog, jets [1, n_in, SWEEP_N] float32, cot [1, SWEEP_N] float32) of one sweep.

    TAN: 1e-4..1e4 in magnitude with the floats around the first eight poles; ATAN: 1e-6..1e6; ATAN2: both operands 1e-3..1e3,
    every sign pattern; SINH / COSH: up to +-EXP_MAX, both ends and the small arguments included, and SINH_TOP / COSH_TOP: the
    last stretch EXP_MAX..SINH_MAX up to the float32 overflow of sinh itself (cotangent / 8, so that the adjoint stays finite in
    float32); ASIN / ACOS: [-1, 1] with both ends, their neighbours and 0; POWC: bases 1e-3..1e3
    for each exponent of POWC_EXPONENTS; POW: the same bases, exponents uniform in [-4, 4]."""
    def make():
        rng = np.random.default_rng(4000 + TRANS_CASES.index(name))
        n = SWEEP_N
        cot = np.array(M.cotangent(n, 40 + TRANS_CASES.index(name)))
        if name == "TAN":
            head = _near([(k + 0.5) * np.pi * s for k in range(8) for s in (1, -1)])
            a = np.concatenate([head, [0.0, -0.0], _signed_decades(rng, n - len(head) - 2, -4, 4)])[None]
            prog = program(("JET", 0, 0), ("TAN", 0), ("OUT", 1, 0))
        elif name == "ATAN":
            a = np.concatenate([[0.0, -0.0, 1.0, -1.0], _signed_decades(rng, n - 4, -6, 6)])[None]
            prog = program(("JET", 0, 0), ("ATAN", 0), ("OUT", 1, 0))
        elif name == "ATAN2":
            a = np.stack([_signed_decades(rng, n, -3, 3), _signed_decades(rng, n, -3, 3)])
            prog = program(("JET", 0, 0), ("JET", 0, 1), ("ATAN2", 0, 1), ("OUT", 2, 0))
        elif name in ("SINH", "COSH"):
            head = [EXP_MAX, -EXP_MAX, 0.0, -0.0, 1e-30, -1e-30, 1e-4, -1e-4]
            small = _signed_decades(rng, n // 4, -5, 0)
            a = np.concatenate([head, small, rng.uniform(-EXP_MAX, EXP_MAX, n - len(head) - len(small))])[None]
            a = np.clip(a.astype(F), F(-EXP_MAX), F(EXP_MAX))
            cot = cot * F(0.125)
            prog = program(("JET", 0, 0), (name, 0), ("OUT", 1, 0))
        elif name in ("SINH_TOP", "COSH_TOP"):
            head = [SINH_MAX, -SINH_MAX, EXP_MAX, -EXP_MAX]
            a = np.concatenate([head, rng.choice([-1.0, 1.0], n - 4) * rng.uniform(EXP_MAX, SINH_MAX, n - 4)])[None]
            a = np.sign(a) * np.clip(np.abs(a).astype(F), F(EXP_MAX), F(SINH_MAX))
            cot = cot * F(0.125)
            prog = program(("JET", 0, 0), (name[:4], 0), ("OUT", 1, 0))
        elif name in ("ASIN", "ACOS"):
            head = np.concatenate([_near([1.0, -1.0, 0.0]), [-0.0]])
            head = head[np.abs(head) <= 1]
            a = np.concatenate([head, rng.uniform(-1.0, 1.0, n - len(head))])[None]
            a = np.clip(a.astype(F), F(-1), F(1))
            prog = program(("JET", 0, 0), (name, 0), ("OUT", 1, 0))
        elif name.startswith("POWC_"):
            a = np.concatenate([[1e-3, 1e3, 1.0], 10.0 ** rng.uniform(-3, 3, n - 3)])[None]
            prog = program(("JET", 0, 0), ("POWC", 0, 0, POWC_EXPONENTS[int(name[5:])]), ("OUT", 1, 0))
        else:
            a = np.stack([10.0 ** rng.uniform(-3, 3, n), np.concatenate([[-4.0, 4.0, 0.0, 1.0], rng.uniform(-4, 4, n - 4)])])
            prog = program(("JET", 0, 0), ("JET", 0, 1), ("POW", 0, 1), ("OUT", 2, 0))
        jets = np.ascontiguousarray(a[None], dtype=F)
        assert jets.shape == (1, len(a), n), jets.shape
        return prog, jets, np.ascontiguousarray(cot[None], dtype=F)
    if name not in _sweeps:
        out = make()
        for t in out:
            t.setflags(write=False)
        _sweeps[name] = out
    return _sweeps[name]


def adjoint_units(name, jets, cot):
    """2^-24 of the sum of the absolute values of the terms of the adjoint expression, per operand: [n_in, SWEEP_N] in fp64."""
    x, g = jets[0].astype(np.float64), np.abs(cot[0].astype(np.float64))
    with np.errstate(all="ignore"):
        if name == "TAN":
            t = g * (1.0 + np.tan(x[0]) ** 2)                      # the terms g and g t t
        elif name == "ATAN":
            t = g / (1.0 + x[0] ** 2)
        elif name == "ATAN2":
            d = x[0] ** 2 + x[1] ** 2
            return U * np.stack([g * np.abs(x[1]) / d, g * np.abs(x[0]) / d])
        elif name in ("SINH", "SINH_TOP"):
            t = g * np.cosh(x[0])
        elif name in ("COSH", "COSH_TOP"):
            t = g * np.abs(np.sinh(x[0]))
        elif name in ("ASIN", "ACOS"):
            t = g / np.sqrt(1.0 - x[0] ** 2)
        elif name.startswith("POWC_"):
            c = np.float64(F(POWC_EXPONENTS[int(name[5:])]))
            t = g * np.abs(c) * x[0] ** (c - 1.0)
        else:
            return U * np.stack([g * np.abs(x[1]) * x[0] ** (x[1] - 1.0), g * x[0] ** x[1] * np.abs(np.log(x[0]))])
    return U * t[None]


def trans_reference(name):
    """(prog, jets32, cot32, value64 [SWEEP_N], adjoint64 [n_in, SWEEP_N], adjoint units [n_in, SWEEP_N]) of one sweep: the fp64
    model of the program and of its adjoint on the float32 inputs."""
    prog, jets, cot = trans_case(name)
    val, = run(prog, jets.astype(np.float64), None, np.float64)
    adj = adjoint(prog, jets.astype(np.float64), None, cot.astype(np.float64), np.float64)[0]
    return prog, jets, cot, val, adj, adjoint_units(name, jets, cot)


def trans_errors(name, value32, adjoint32):
    """(max value error in ulps, max adjoint error in adjoint units) of a float32 evaluation of the sweep against the fp64 model."""
    _, _, _, val, adj, unit = trans_reference(name)
    return float(M.ulp_err(value32, val).max()), float(M.units_err(adjoint32, adj, unit).max())


def trans_yardstick(name):
    """What torch's own float32 CPU evaluation of the opcode (torch_program: torch.tan, ``**``, torch.pow, ...) and its autograd
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
