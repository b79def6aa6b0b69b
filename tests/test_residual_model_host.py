"""tests/residual_model.py against torch on the host, and the limit cases of pde._compile_residual_program.

The fp64 adjoint model (the rules of k_residual_bwd) must agree with torch's fp64 autograd of the SAME program built from torch's
own operators, for every opcode: then the device tests, which hold the kernel to the model, cannot share a wrong rule with it.
The float32 model is pinned to torch's conventions at the singular points, and an equation set whose compiled program contains
all 17 opcodes is checked against the lambdified equations in fp64."""
import hashlib
import json
import os
import re

import numpy as np
import pytest
import sympy
import torch

from space_time_pde_amd import pde as P
from tests import residual_model as M


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPCODES = ["JET", "X", "CONST", "ADD", "SUB", "MUL", "DIV", "NEG", "POWI", "SIN", "COS", "EXP", "LOG", "SQRT", "TANH", "ABS", "OUT",
           "TAN", "SINH", "COSH", "ASIN", "ACOS", "ATAN", "ATAN2", "POWC", "POW", "MIN", "MAX", "SIGN", "STEP",
           "LT", "LE", "EQ", "NE", "AND", "OR", "NOT", "SEL", "STEPC"]


def test_header_package_and_model_share_one_opcode_table():
    """One numbering in three places: the header's enum, pde._RES_OPS and the model's OPS."""
    with open(os.path.join(ROOT, "include", "stpde_hip.h")) as f:
        text = f.read()
    enums = re.findall(r"enum \{([^{}]*STPDE_RES_[^{}]*)\};", text)
    assert len(enums) == 1
    header = [t.strip() for t in enums[0].split(",") if t.strip()]
    assert header[0] == "STPDE_RES_JET = 0" and not any("=" in t for t in header[1:])        # numbered 0, 1, 2, ... in order
    header[0] = "STPDE_RES_JET"
    assert header == ["STPDE_RES_" + n for n in OPCODES] and len(OPCODES) == 39
    want = {n: k for k, n in enumerate(OPCODES)}
    assert P._RES_OPS == want and M.OPS == want
    assert [M.OPS[n] for n in M.OPS_EXT] == list(range(17, 30)) and [M.OPS[n] for n in M.OPS_COND] == list(range(30, 39))
    assert "#define STPDE_RES_MAX_INS 192" in text and P._RES_MAX_INS == M.MAX_INS == 192
    assert P._RES_DT == M.DT
    assert M.sel_operands(M.sel(191, 190)) == (191, 190)
    assert len(M.chain_program()[0]) == P._RES_MAX_INS


def _canonical_digest(arrays, dtype):
    """SHA-256 of the arrays as little-endian ``dtype``, every NaN replaced by the one canonical NaN (the models compare the
    position of a NaN, not its payload)."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.array(a, dtype=np.dtype(dtype).newbyteorder("<"))
        a[np.isnan(a)] = np.nan
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _parent_cases():
    """(key, prog, jets, x, cot): every exact case, the mixed case and the 192-instruction chain on the inputs of its device test."""
    for name in M.EXACT_CASES:
        yield (name,) + M.exact_case(name)
    c = M.mixed_case()
    yield "mixed", c["prog"], c["jets"], c["x"], c["cot"]
    prog, n_eq = M.chain_program()
    rng = np.random.default_rng(5)
    yield "chain", prog, rng.uniform(0.5, 2.0, (2, 1, 300)).astype(np.float32), None, rng.standard_normal((n_eq, 300)).astype(np.float32)


def test_folded_model_reproduces_the_parents_exact_results():
    """tests/golden/residual_model_parent.json: digests of ``run`` and ``adjoint``, float32 and float64, recorded with the three
    layered models this one replaced (residual_model, residual_ext_model for MIN .. POWC_1, residual_cond_model for LT .. STEPC_2
    and the mixed case).  These cases hold only IEEE add, subtract, multiply, divide, sqrt, comparisons and selects, so the bits
    do not depend on the numpy build."""
    with open(os.path.join(ROOT, "tests", "golden", "residual_model_parent.json")) as f:
        want = json.load(f)
    cases = list(_parent_cases())
    assert [c[0] for c in cases] == list(want) and len(want) == len(M.EXACT_CASES) + 2 == 39
    for key, prog, jets, x, cot in cases:
        for dt in ("float32", "float64"):
            got = {"run": _canonical_digest(M.run(prog, jets, x, np.dtype(dt).type), dt),
                   "adjoint": _canonical_digest([M.adjoint(prog, jets, x, cot, np.dtype(dt).type)], dt)}
            assert got == want[key][dt], (key, dt)


def _autograd64(prog, jets, x, res_bar):
    jt = torch.from_numpy(np.asarray(jets, dtype=np.float64)).requires_grad_(True)
    xt = None if x is None else torch.from_numpy(np.asarray(x, dtype=np.float64))
    res = M.torch_program(prog, jt, xt)
    cot = torch.from_numpy(np.asarray(res_bar, dtype=np.float64))
    total = sum((r * cot[k]).sum() for k, r in enumerate(res))
    if total.requires_grad:
        total.backward()
    return [r.detach().numpy() for r in res], (np.zeros(jt.shape) if jt.grad is None else jt.grad.numpy())


def _same_class(a, b):
    """NaN where NaN, the same infinity where infinite, finite where finite (the finite values are compared by the caller)."""
    return np.where(np.isfinite(b), np.isfinite(a), np.where(np.isnan(b), np.isnan(a), a == b))


def _cases():
    for name in M.EXACT_CASES_BASE:
        yield (name,) + M.exact_case(name)
    for name in M.TRANS_CASES_BASE:
        prog, jets, cot = M.trans_case(name)
        yield name, prog, jets, None, cot
        e = np.array(M.EDGES, dtype=np.float32)
        yield name + "_edges", M.program(("JET", 0, 0), (name, 0), ("OUT", 1, 0)), e[None, None], None, np.ones((1, len(e)))
    prog, n_eq = M.chain_program()
    rng = np.random.default_rng(5)
    yield "chain", prog, rng.uniform(0.5, 2.0, (2, 1, 300)), None, rng.standard_normal((n_eq, 300))


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_fp64_adjoint_model_matches_torch_autograd(case):
    name, prog, jets, x, res_bar = case
    want_res, want_bar = _autograd64(prog, jets, x, res_bar)
    got_res = M.run(prog, jets, x, np.float64)
    got_bar = M.adjoint(prog, jets, x, res_bar, np.float64)
    assert got_bar.shape == want_bar.shape and len(got_res) == len(want_res)
    for k in range(len(want_res)):
        assert _same_class(got_res[k], want_res[k]).all(), (name, k)
        fin = np.isfinite(want_res[k])
        np.testing.assert_allclose(got_res[k][fin], want_res[k][fin], rtol=1e-13, atol=0)
    assert _same_class(got_bar, want_bar).all(), (name, np.argwhere(~_same_class(got_bar, want_bar))[:5])
    fin = np.isfinite(want_bar)
    # b / b (the a == b companion of DIV: g / b - g / b) and 1 - tanh^2 cancel: judged against the size of the cancelling terms
    scale = np.zeros(got_bar.shape)
    if name == "DIV":
        with np.errstate(all="ignore"):
            scale[0, 1] = np.nan_to_num(np.abs(res_bar[1] / jets[0, 1].astype(np.float64)), nan=0.0, posinf=0.0)
    elif name.startswith("TANH"):
        scale[0, 0] = np.abs(res_bar[0])
    scale = 1e-13 * scale[fin]
    assert (np.abs(got_bar[fin] - want_bar[fin]) <= 1e-12 * np.abs(want_bar[fin]) + scale).all(), name


def test_fp32_model_has_torchs_conventions_at_the_singular_points():
    """abs'(0) = abs'(NaN) = 0, (x^2)'(0) = 0, (x^-1)'(0) = -inf, sqrt'(0) = +inf, d(a / b)/db = NaN at (0, 0) and -inf at
    (1, 0): what torch's float32 autograd gives, and what the float32 model (the kernel's rules) gives."""
    nan, inf = float("nan"), float("inf")
    want = [("ABS", (0.0,), 0, 0.0), ("ABS", (nan,), 0, 0.0), ("POWI_2", (0.0,), 0, 0.0), ("POWI_-1", (0.0,), 0, -inf),
            ("SQRT", (0.0,), 0, inf), ("DIV", (0.0, 0.0), 1, nan), ("DIV", (1.0, 0.0), 1, -inf)]
    for name, at, ch, value in want:
        prog, jets, x, res_bar = M.exact_case(name)
        prog = prog[:4] if name == "DIV" else prog            # a / b alone, without the a == b companion
        res_bar = res_bar[:1]
        i = M.edge_index(*at)
        assert all(np.array_equal(jets[0, k, i], np.float32(a), equal_nan=True) and
                   np.signbit(jets[0, k, i]) == np.signbit(a) for k, a in enumerate(at))
        assert res_bar[0, i] == 1.0
        model = M.adjoint(prog, jets, x, res_bar, np.float32)[0, ch, i]
        jt = torch.from_numpy(np.array(jets)).requires_grad_(True)
        res = M.torch_program(prog, jt, None)
        (res[0] * torch.from_numpy(np.array(res_bar[0]))).sum().backward()
        for got in (model, jt.grad[0, ch, i].item()):
            assert (np.isnan(got) and np.isnan(value)) or got == value, (name, at, got, value)


def test_ulp_err_counts_float32_steps():
    one = np.float32(1.0)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    assert M.ulp_err(np.array([up, down, one]), np.array([1.0, 1.0, 1.0])).tolist() == [1.0, 0.5, 0.0]
    assert M.ulp_err(np.array([np.inf, np.nan, 1.0, np.inf]), np.array([np.inf, np.nan, np.inf, -np.inf])).tolist() == \
        [0.0, 0.0, np.inf, np.inf]
    assert M.ulp_err(np.array([0.0]), np.array([2.0 ** -149])).tolist() == [1.0]
    assert M.same_bits(np.array([0.0, -0.0, np.nan, 1.0], np.float32), np.array([-0.0, -0.0, np.nan, 1.0], np.float32)).tolist() \
        == [False, True, True, True]


def test_transcendental_sweeps_and_yardsticks():
    """The sweeps have the size and the ranges the device tests state, and torch's own float32 evaluation -- the yardstick --
    stays within a few ulp on them (so that 4 x max(1, yardstick) is a bound worth the name)."""
    for name, (lo, hi) in M.SWEEP_RANGE.items():
        x = M.trans_case(name)[1][0, 0]
        assert x.shape == (32768,) and x.dtype == np.float32
        assert x.min() == np.float32(lo) and x.max() == np.float32(hi)
        val, adj = M.trans_yardstick(name)
        print("%s: torch float32 on the CPU reaches %.3f ulp (value), %.3f units (adjoint)" % (name, val, adj))
        assert 0 < val <= 4 and 0 < adj <= 8, (name, val, adj)
    x = M.trans_case("TANH")[1][0, 0]
    assert np.signbit(x[x == 0]).tolist() == [False, True] and (np.tanh(x.astype(np.float64)).astype(np.float32) == 1).any()


# ---- the compiler -----------------------------------------------------------------------------------------------------------
def test_all_opcode_equation_set_compiles_to_all_17_and_matches_lambdify():
    layer = M.all_ops_layer()
    prog, uses_x, stream_of = M.all_ops_program(layer)
    assert {int(op) for op in prog["op"]} == set(range(17)), sorted({M.NAMES[int(op)] for op in prog["op"]})
    assert any(int(b) < 0 for op, a, b, c in prog.tolist() if op == M.OPS["POWI"]), "no negative integer power"
    assert uses_x and len(prog) <= P._RES_MAX_INS
    rng = np.random.default_rng(1)
    n = 64
    jets = rng.standard_normal((len(stream_of), layer.n_out, n))
    x = rng.random((n, 3))
    got = M.run(prog, jets, x, np.float64)
    for k, p in enumerate(layer.eqns_jet.values()):
        cols = [torch.from_numpy(x[:, i]) for i in range(3)]
        atoms = [torch.from_numpy(jets[stream_of[a[1]], a[0]]) for a in p.atoms]
        want = p.fn(*(cols + atoms)).numpy()
        np.testing.assert_allclose(got[k], want, rtol=2e-6, atol=2e-6)   # program constants are fp32


def _sum_of_symbols(n_terms):
    """u0 + u1 + ... : n_terms JET, n_terms - 1 ADD and one OUT = 2 n_terms instructions."""
    syms = sympy.symbols("u0:%d" % n_terms)
    return sympy.Add(*syms), {s: (0, k) for k, s in enumerate(syms)}


def test_program_of_exactly_the_instruction_limit_compiles_and_one_more_does_not():
    assert P._RES_MAX_INS % 2 == 0
    e, slots = _sum_of_symbols(P._RES_MAX_INS // 2)
    comp = P._compile_residual_program([e], [], slots)
    assert comp is not None and len(comp[0]) == P._RES_MAX_INS and not comp[1]
    u0 = next(iter(slots))
    comp = P._compile_residual_program([e, u0], [], slots)                # the shared JET and one more OUT
    assert comp is None
    e, slots = _sum_of_symbols(P._RES_MAX_INS // 2 - 1)
    comp = P._compile_residual_program([e, next(iter(slots))], [], slots)
    assert comp is not None and len(comp[0]) == P._RES_MAX_INS - 1


@pytest.mark.parametrize("expr", ["pi*u", "u**(1/3)", "u**1.5 + 1", "sinh(u)", "atan(u)", "Max(u, 1)", "zoo*u"])
def test_what_the_evaluator_does_not_implement_is_not_compiled(expr):
    u = sympy.Symbol("u")
    e = sympy.sympify(expr, locals={"u": u})
    assert P._compile_residual_program([e], [], {u: (0, 0)}) is None
    assert P._compile_residual_program([u * u], [], {u: (0, 0)}) is not None
