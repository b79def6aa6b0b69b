"""Host model of the opcodes appended to the residual evaluator of csrc/residual.hip after STEP (LT LE EQ NE AND OR NOT SEL STEPC:
Piecewise with relational conditions, Heaviside(a, h0)), shared by tests/test_residual_cond_host.py and
tests/test_gpu_residual_cond.py.  It is built on tests/residual_ext_model.py (imported as ``X``, not edited): an instruction with
one of X's opcodes is handed to X's own interpreter as a one-instruction program over its operands, so its value and its adjoint
rule are X's, expression for expression; only the new opcodes are written out here.

All of them are comparisons and selects, so with dtype = float32 the device must be bit-equal.  Conventions (torch's and its
autograd's, tests/test_residual_cond_host.py checks them against torch's fp64 autograd):

* LT LE EQ NE: IEEE comparisons into a mask 1.0 / 0.0; a NaN operand gives 0.0, for NE 1.0.  A mask is never NaN.
* AND OR NOT: on masks, an operand is true where it is != 0.
* SEL: a = mask, b = then | else << 16; value = mask != 0 ? v[then] : v[else].  Adjoint: the selected operand takes the
  cotangent, the other exactly +0 (a select, never cotangent * mask: a NaN cotangent does not reach the operand not taken).
* STEPC: Heaviside with H(+-0) = c, H(NaN) = NaN.
* Nothing reaches a mask, the operands of a comparison or the operand of STEPC.
"""
import numpy as np

from tests import residual_ext_model as X
from tests import residual_model as M

F = M.F
OPS_COND = {"LT": 30, "LE": 31, "EQ": 32, "NE": 33, "AND": 34, "OR": 35, "NOT": 36, "SEL": 37, "STEPC": 38}    # = pde._RES_OPS_COND
OPS = dict(X.OPS, **OPS_COND)
NAMES = {v: k for k, v in OPS.items()}
MAX_INS = 192                                                                                                      # = pde._RES_MAX_INS
_LEAF = ("JET", "X", "CONST")
_ONE_OPERAND = ("NEG", "POWI", "POWC", "SIN", "COS", "EXP", "LOG", "SQRT", "TANH", "ABS", "TAN", "SINH", "COSH", "ASIN", "ACOS",
                "ATAN", "SIGN", "STEP", "NOT", "STEPC")


def sel(then, other):
    """The b field of SEL."""
    return int(then) | int(other) << 16


def sel_operands(b):
    return b & 0xffff, b >> 16


def operands(name, a, b):
    """The value indices an instruction reads."""
    if name in _LEAF:
        return ()
    if name == "SEL":
        return (a,) + sel_operands(b)
    return (a,) if name in _ONE_OPERAND or name == "OUT" else (a, b)


def program(*ins):
    """[(name, a, b, c) with trailing fields optional] -> a pde._RES_DT array.  The kernels index their value arrays with the
    operand fields unchecked, so a hand-written program is checked here: at most MAX_INS instructions, every operand an earlier
    instruction."""
    rows = []
    assert len(ins) <= MAX_INS
    for k, i in enumerate(ins):
        i = tuple(i) + (0, 0, 0.0)[len(i) - 1:]
        for o in operands(i[0], int(i[1]), int(i[2])):
            assert 0 <= o < k, (k, i)
        rows.append((OPS[i[0]], int(i[1]), int(i[2]), float(i[3])))
    return np.array(rows, dtype=M.DT)


def _mini(name, a, b, c):
    """The instruction as a program of X over its operands as jets [1, 1 or 2, P]: (program, index of the instruction).  (An
    instruction with twice the same operand gets two jets as well: the kernel adds its two terms one after the other.)"""
    if name in _ONE_OPERAND:
        return X.program(("JET", 0, 0), (name, 0, b, c), ("OUT", 1, 0)), 1
    return X.program(("JET", 0, 0), ("JET", 0, 1), (name, 0, 1, c), ("OUT", 2, 0)), 2


def _mask(m, dtype):
    return np.where(m, dtype(1), dtype(0))


def _values(prog, jets, x, dtype):
    jets = np.asarray(jets, dtype=dtype)
    x = None if x is None else np.asarray(x, dtype=dtype)
    one, zero = dtype(1), dtype(0)
    v = []
    with np.errstate(all="ignore"):
        for op, a, b, c in prog.tolist():
            name = NAMES[op]
            if name in _LEAF:
                r = X._values(X.program((name, a, b, c)), jets, x, dtype)[0]
            elif name == "OUT":
                r = v[a]
            elif name == "LT":
                r = _mask(v[a] < v[b], dtype)
            elif name == "LE":
                r = _mask(v[a] <= v[b], dtype)
            elif name == "EQ":
                r = _mask(v[a] == v[b], dtype)
            elif name == "NE":
                r = _mask(v[a] != v[b], dtype)
            elif name == "AND":
                r = _mask((v[a] != zero) & (v[b] != zero), dtype)
            elif name == "OR":
                r = _mask((v[a] != zero) | (v[b] != zero), dtype)
            elif name == "NOT":
                r = np.where(v[a] != zero, zero, one)
            elif name == "SEL":
                t, e = sel_operands(b)
                r = np.where(v[a] != zero, v[t], v[e])
            elif name == "STEPC":
                s = v[a]
                r = np.where(s > zero, one, np.where(s < zero, zero, np.where(s == zero, dtype(F(c)), s)))
            else:
                mini, k = _mini(name, a, b, c)
                r = X._values(mini, np.stack([v[a]] if k == 1 else [v[a], v[b]])[None], None, dtype)[k]
            assert r.dtype == dtype, (name, r.dtype)
            v.append(r)
    return v


def run(prog, jets, x, dtype=np.float64):
    """The residuals [n_eq] of P points: jets [S, n_out, P], x [P, 3] or None, in the order of the OUT indices."""
    v = _values(prog, jets, x, dtype)
    out = {int(b): v[i] for i, (op, a, b, c) in enumerate(prog.tolist()) if NAMES[op] == "OUT"}
    return [out[k] for k in sorted(out)]


def adjoint(prog, jets, x, res_bar, dtype=np.float64):
    """The sweep of k_residual_bwd: res_bar [n_eq, P] -> jets_bar [S, n_out, P]."""
    v = _values(prog, jets, x, dtype)
    res_bar = np.asarray(res_bar, dtype=dtype)
    P = np.shape(jets)[2]
    g = [np.zeros(P, dtype=dtype) for _ in v]
    jets_bar = np.zeros(np.shape(jets), dtype=dtype)
    zero = dtype(0)
    with np.errstate(all="ignore"):
        for i in range(len(v) - 1, -1, -1):
            op, a, b, c = prog[i].tolist()
            name, gi = NAMES[op], g[i]
            if name == "OUT":
                g[a] = g[a] + res_bar[b]
            elif name == "JET":
                jets_bar[a, b] = jets_bar[a, b] + gi
            elif name == "SEL":
                t, e = sel_operands(b)
                then = v[a] != zero
                g[t] = g[t] + np.where(then, gi, zero)
                g[e] = g[e] + np.where(then, zero, gi)
            elif name in OPS_COND or name in ("X", "CONST"):
                pass                      # masks, comparison operands, STEPC: adjoint 0; coordinates are not differentiated
            else:
                # X's rule, applied to the one instruction: its jets_bar of a zero-filled start is the term the kernel adds (an
                # accumulator that starts at +0 is never -0, so adding the term afterwards gives the same bits)
                mini, k = _mini(name, a, b, c)
                bar = X.adjoint(mini, np.stack([v[a]] if k == 1 else [v[a], v[b]])[None], None, gi[None], dtype)[0]
                g[a] = g[a] + bar[0]
                if k == 2:
                    g[b] = g[b] + bar[1]
    assert jets_bar.dtype == dtype
    return jets_bar


def torch_program(prog, jets, x):
    """The program as a torch graph of torch's own operators (comparisons, logical_and / or / not, torch.where; Heaviside as
    PDELayer's torch strategies evaluate it; X.torch_program for X's opcodes), for torch.autograd: residuals [n_eq] of [P]."""
    import torch
    from space_time_pde_amd import pde
    rel = {"LT": torch.lt, "LE": torch.le, "EQ": torch.eq, "NE": torch.ne}
    v, out = [], {}
    for op, a, b, c in prog.tolist():
        name = NAMES[op]
        if name in _LEAF:
            r = X.torch_program(X.program((name, a, b, c), ("OUT", 0, 0)), jets, x)[0]
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
        else:
            mini, k = _mini(name, a, b, c)
            r = X.torch_program(mini, torch.stack([v[a]] if k == 1 else [v[a], v[b]])[None], None)[0]
        v.append(r)
    return [out[k] for k in sorted(out)]


# ---- exact cases: every new opcode -----------------------------------------------------------------------------------------------
STEPC_VALUES = (1.0, 0.0, -2.5)
EXACT_CASES = ("LT", "LE", "EQ", "NE", "AND", "OR", "NOT", "SEL", "SEL_NAN_DEFAULT", "SEL_DEAD_SQRT", "SEL_CHAIN") + \
    tuple("STEPC_%d" % k for k in range(len(STEPC_VALUES)))
_cases = {}


def _binary_with_ties():
    """M's binary inputs (4096 normal-range pairs, then every pair of 0, -0, 1, -1, +-Inf, NaN) with the first 64 pairs tied."""
    j = np.array(M.binary_inputs())
    j[1, :64] = j[0, :64]
    return j[None]


def _cotangent(n_eq, P, n_edge, seed, nonfinite):
    """A random cotangent, 1 on the edge rows; with ``nonfinite`` NaN, +Inf and -Inf in turn on every fifth row of residual 0,
    normal-range and edge rows alike (they land on either side of a select)."""
    cot = np.array(M.cotangent(n_eq * P, seed).reshape(n_eq, P))
    cot[:, P - n_edge:] = 1.0
    if nonfinite:
        for k, val in enumerate((np.nan, np.inf, -np.inf)):
            cot[0, 5 * k + 2::15] = val
    return cot


def exact_case(name):
    """(prog, jets [1, n_out, P] float32, res_bar [n_eq, P] float32), read-only.

    LT LE EQ NE: of (a, b), (b, a) and (b, b), and the mask as a factor of a so that a cotangent passes it.
    AND OR NOT: of the masks a <= b and b <= a (both true on a tie, both false with a NaN), again also as factors.
    SEL: a < b ? a : b, then b <= a ? a * b : a, with NaN / Inf cotangents; SEL_NAN_DEFAULT: a chain that ends in CONST NaN;
    SEL_DEAD_SQRT: a > 0 ? sqrt(a) : 0, whose dead branch at a = 0 turns its zero cotangent into NaN (as torch's does);
    SEL_CHAIN: three branches over AND / OR / NOT masks.  STEPC: like X's STEP, for each H(0) of STEPC_VALUES."""
    if name in _cases:
        return _cases[name]
    nonfinite = name.startswith("SEL")
    if name in ("LT", "LE", "EQ", "NE"):
        prog = program(("JET", 0, 0), ("JET", 0, 1), (name, 0, 1), ("OUT", 2, 0), (name, 1, 0), ("OUT", 4, 1), (name, 1, 1),
                       ("OUT", 6, 2), ("MUL", 2, 0), ("OUT", 8, 3))
        jets, n_edge = _binary_with_ties(), M.N_EDGE2
    elif name in ("AND", "OR", "NOT"):
        ins = [("JET", 0, 0), ("JET", 0, 1), ("LE", 0, 1), ("LE", 1, 0), (name, 2) if name == "NOT" else (name, 2, 3),
               ("OUT", 4, 0), ("MUL", 4, 0), ("OUT", 6, 1)]
        if name != "NOT":
            ins += [(name, 3, 3), ("OUT", 8, 2)]
        prog = program(*ins)
        jets, n_edge = _binary_with_ties(), M.N_EDGE2
    elif name == "SEL":
        prog = program(("JET", 0, 0), ("JET", 0, 1), ("LT", 0, 1), ("SEL", 2, sel(0, 1)), ("OUT", 3, 0),
                       ("LE", 1, 0), ("MUL", 0, 1), ("SEL", 5, sel(6, 0)), ("OUT", 7, 1))
        jets, n_edge = _binary_with_ties(), M.N_EDGE2
    elif name == "SEL_NAN_DEFAULT":
        prog = program(("JET", 0, 0), ("JET", 0, 1), ("CONST", 0, 0, np.nan), ("EQ", 0, 1), ("SEL", 3, sel(1, 2)),
                       ("LT", 0, 1), ("SEL", 5, sel(0, 4)), ("OUT", 6, 0))
        jets, n_edge = _binary_with_ties(), M.N_EDGE2
    elif name == "SEL_DEAD_SQRT":
        prog = program(("JET", 0, 0), ("CONST", 0, 0, 0.0), ("LT", 1, 0), ("SQRT", 0), ("SEL", 2, sel(3, 1)), ("OUT", 4, 0))
        jets, n_edge = M.unary_inputs(0)[None, None], M.N_EDGE1
    elif name == "SEL_CHAIN":
        prog = program(("JET", 0, 0), ("JET", 0, 1), ("CONST", 0, 0, 0.0), ("LT", 2, 0), ("LT", 2, 1), ("AND", 3, 4), ("OR", 3, 4),
                       ("NOT", 6), ("NE", 0, 0), ("OR", 7, 8), ("MUL", 0, 1), ("SUB", 0, 1), ("NEG", 0),
                       ("SEL", 9, sel(12, 11)), ("SEL", 5, sel(10, 13)), ("OUT", 14, 0))
        jets, n_edge = _binary_with_ties(), M.N_EDGE2
    else:
        c = STEPC_VALUES[int(name[6:])]
        prog = program(("JET", 0, 0), ("STEPC", 0, 0, c), ("OUT", 1, 0), ("MUL", 1, 0), ("OUT", 3, 1))
        jets, n_edge = M.unary_inputs(0)[None, None], M.N_EDGE1
    n_eq = int((prog["op"] == OPS["OUT"]).sum())
    P = jets.shape[2]
    out = (prog, np.ascontiguousarray(jets, dtype=F), _cotangent(n_eq, P, n_edge, 17 + EXACT_CASES.index(name), nonfinite))
    for t in out:
        t.setflags(write=False)
    _cases[name] = out
    return out


# ---- one program with every new opcode ---------------------------------------------------------------------------------------------
_mixed = {}


def mixed_case():
    """dict(prog, jets [1, 2, 257], x [257, 3], cot [2, 257]), read-only: two residuals that use every new opcode, the coordinates
    and a constant branch; exact zeros and ties in the first rows.  Every opcode in it is an exact one (bit-equal on the device)."""
    if not _mixed:
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
        _mixed.update(prog=prog, jets=jets, x=x, cot=rng.standard_normal((2, 257)).astype(F))
        assert set(prog["op"].tolist()) >= set(OPS_COND.values())
        for t in _mixed.values():
            t.setflags(write=False)
    return _mixed
