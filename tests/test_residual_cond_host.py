"""Piecewise with relational conditions, And / Or / Not, pi and the other number symbols, Heaviside(a, h0) in PDELayer equations,
everything that needs no GPU: the model of the opcodes appended after STEP (tests/residual_model.py) against torch's fp64
autograd at the ties, zeros, infinities, NaN and with NaN cotangents; the equation strings on both torch strategies against
hand-written torch.where formulas; their device programs (``_compile_residual_program(..., extended=True, conditional=True)``)
through the model against the lambdified functions; and that nothing that compiled before compiles differently."""
import base64
import json
import os
import types

import numpy as np
import pytest
import sympy
import torch

from space_time_pde_amd import local_implicit_grid as lig
from space_time_pde_amd import pde, physics
from tests import residual_model as M
from tests import test_residual_ext_host as E

ROOT = E.ROOT
NAN, INF = float("nan"), float("inf")


# ---- the model against torch's fp64 autograd ----------------------------------------------------------------------------------------
def _against_autograd(prog, jets, cot, what):
    jets = np.asarray(jets, dtype=np.float64)
    cot = np.asarray(cot, dtype=np.float64)
    jt = torch.from_numpy(jets.copy()).requires_grad_(True)
    outs = M.torch_program(prog, jt, None)
    sum((o * torch.from_numpy(cot[k])).sum() for k, o in enumerate(outs)).backward()
    vals = M.run(prog, jets, None, np.float64)
    for k, o in enumerate(outs):
        E._same(vals[k], o.detach().numpy(), "%s value %d" % (what, k))
    E._same(M.adjoint(prog, jets, None, cot, np.float64), jt.grad.numpy(), what + " adjoint")


@pytest.mark.parametrize("name", M.EXACT_CASES_COND)
def test_model_matches_torch_autograd_on_the_exact_cases(name):
    prog, jets, _, cot = M.exact_case(name)
    _against_autograd(prog, jets, cot, name)


def test_the_models_conventions_literally():
    e = M.edge_index
    # comparisons: IEEE, a mask is never NaN, nothing reaches the operands except through the MUL
    for name, fn in (("LT", np.less), ("LE", np.less_equal), ("EQ", np.equal), ("NE", np.not_equal)):
        prog, jets, _, cot = M.exact_case(name)
        val = M.run(prog, jets, None, np.float32)
        assert all(set(np.unique(v)) <= {0.0, 1.0} for v in val[:3])
        assert np.array_equal(val[0], fn(jets[0, 0], jets[0, 1]).astype(np.float32))
        for a, b in ((NAN, 1.0), (1.0, NAN), (NAN, NAN)):
            assert val[0][e(a, b)] == (1.0 if name == "NE" else 0.0)
        assert val[0][e(0.0, -0.0)] == (1.0 if name in ("LE", "EQ") else 0.0)
        assert val[0][:64].tolist() == [1.0 if name in ("LE", "EQ") else 0.0] * 64            # the tied rows
        bar = M.adjoint(prog, jets, None, cot, np.float32)
        assert not bar[0, 1].view(np.int32).any()                                            # b: only ever compared
        with np.errstate(all="ignore"):
            assert M.same_bits(bar[0, 0], np.float32(0) + cot[3] * val[0]).all()                  # (an accumulator from +0)
    # SEL: the operand not taken receives exactly +0, also under a NaN or infinite cotangent
    prog, jets, _, cot = M.exact_case("SEL")
    bar = M.adjoint(prog, jets, None, cot, np.float32)
    a, b = jets[0, 0], jets[0, 1]
    bad = ~np.isfinite(cot[0])
    assert bad.sum() > 500 and (bad & (a < b)).sum() > 100 and (bad & ~(a < b)).sum() > 100
    # residual 0 = a < b ? a : b; residual 1 = b <= a ? a * b : a
    with np.errstate(all="ignore"):
        want_b = (np.float32(0) + np.where(b <= a, cot[1], np.float32(0)) * a) + np.where(a < b, np.float32(0), cot[0])
    assert M.same_bits(bar[0, 1], want_b).all()
    rows = bad & (a < b) & np.isfinite(a)
    assert rows.any() and np.isfinite(bar[0, 1][rows]).all() and np.isnan(bar[0, 0][rows & np.isnan(cot[0])]).all()
    # a dead sqrt(0): the zero cotangent of the branch not taken becomes 0 * 0.5 / 0 = NaN in sqrt's own rule, as in torch
    prog, jets, _, cot = M.exact_case("SEL_DEAD_SQRT")
    val, = M.run(prog, jets, None, np.float32)
    bar = M.adjoint(prog, jets, None, cot, np.float32)[0, 0]
    for z in (0.0, -0.0):
        assert val[e(z)] == 0.0 and np.isnan(bar[e(z)])
    assert val[e(1.0)] == 1.0 and bar[e(1.0)] == 0.5 and np.isnan(bar[e(-1.0)]) and val[e(-1.0)] == 0.0
    # no default: NaN where no condition holds
    prog, jets, _, cot = M.exact_case("SEL_NAN_DEFAULT")
    val, = M.run(prog, jets, None, np.float32)
    assert np.isnan(val[e(1.0, -1.0)]) and val[e(-1.0, 1.0)] == -1.0 and val[e(1.0, 1.0)] == 1.0
    # STEPC
    for k, c in enumerate(M.STEPC_VALUES):
        prog, jets, _, cot = M.exact_case("STEPC_%d" % k)
        val = M.run(prog, jets, None, np.float32)
        for x, w in ((0.0, c), (-0.0, c), (1.0, 1.0), (-1.0, 0.0), (INF, 1.0), (-INF, 0.0)):
            assert val[0][e(x)] == w, (c, x)
        assert np.isnan(val[0][e(NAN)])


def test_hand_written_programs_are_checked_before_they_reach_a_kernel():
    with pytest.raises(AssertionError):
        M.program(("JET", 0, 0), ("LT", 0, 1))                                   # operand 1 is not an earlier instruction
    with pytest.raises(AssertionError):
        M.program(("JET", 0, 0), ("LT", 0, 0), ("SEL", 1, M.sel(0, 2)))


# ---- the equation strings on both torch strategies -------------------------------------------------------------------------------------
MIXED, POS = E.MIXED, E.POS
W = torch.where


class _Field(E._Field):
    """E's closed-form field with four times the wave numbers: on points of [0, 1)^3 u and w of MIXED take both signs often."""

    def __init__(self, off, amp):
        super().__init__(off, amp)
        self.a = 4.0 * self.a


def _num(v, like):
    return torch.as_tensor(float(v), dtype=like.dtype)


# (equation, field, fp64 formula of the jets J[stream][channel]: stream 0 value, 1..3 d/dt d/dz d/dx, 4.. the pairs; J["x"])
STRINGS = [
    ("Piecewise((u, x > 0.5), (w, True))*dif(u,x)", MIXED, lambda J: W(J["x"] > 0.5, J[0][0], J[0][1]) * J[3][0]),
    ("dif(u,t) + Piecewise((u*dif(u,x), u > 0), (0, True))", MIXED,
     lambda J: J[1][0] + W(J[0][0] > 0, J[0][0] * J[3][0], _num(0, J[0][0]))),
    ("dif(Piecewise((u**2, u > 0), (w, True)), x)", MIXED, lambda J: W(J[0][0] > 0, 2 * J[0][0] * J[3][0], J[3][1])),
    ("dif(dif(Piecewise((u**2, x > 0.5), (0, True)), x), x)", MIXED,
     lambda J: W(J["x"] > 0.5, 2 * J[3][0] ** 2 + 2 * J[0][0] * J[4][0], _num(0, J[0][0]))),
    ("Piecewise((u, (u > 0) & (w > 0)), (w, (u > 0) | (x < 0.5)), (1, ~((w >= x) & (u < 0))), (2, Eq(u, w)), (3, Ne(u, w)))", MIXED,
     lambda J: W((J[0][0] > 0) & (J[0][1] > 0), J[0][0], W((J[0][0] > 0) | (J["x"] < 0.5), J[0][1],
                 W(~((J[0][1] >= J["x"]) & (J[0][0] < 0)), _num(1, J[0][0]), W(J[0][0] == J[0][1], _num(2, J[0][0]), _num(3, J[0][0])))))),
    ("Piecewise((1, Eq(u, u)), (0, True)) + Piecewise((w, Ne(x, 2)), (0, True)) + Piecewise((u, ~((u > 0) | (w > 0))), (0, True))", MIXED,
     lambda J: 1 + J[0][1] + W(~((J[0][0] > 0) | (J[0][1] > 0)), J[0][0], _num(0, J[0][0]))),
    ("Piecewise((u, u > 0))", MIXED, lambda J: W(J[0][0] > 0, J[0][0], _num(NAN, J[0][0]))),
    ("Piecewise((sqrt(u), u > 0), (w, x > 0.5))*dif(w,z)", MIXED,
     lambda J: W(J[0][0] > 0, torch.sqrt(J[0][0]), W(J["x"] > 0.5, J[0][1], _num(NAN, J[0][0]))) * J[2][1]),
    ("sin(pi*x)*u", MIXED, lambda J: torch.sin(np.pi * J["x"]) * J[0][0]),
    ("E*u + EulerGamma*w + GoldenRatio + Catalan*x", MIXED,
     lambda J: np.e * J[0][0] + 0.57721566490153286 * J[0][1] + (1 + 5 ** 0.5) / 2 + 0.91596559417721902 * J["x"]),
    ("u**pi", POS, lambda J: torch.exp(np.pi * torch.log(J[0][0]))),
    ("Heaviside(u, 1)*w + Heaviside(w - 1, 0)", POS, lambda J: J[0][1] + W(J[0][1] > 1, 1.0, 0.0).to(J[0][0].dtype)),
    ("Piecewise((dif(dif(u,x),x) + dif(dif(u,z),z), x > 0.5), (dif(dif(u,x),x) + 2*dif(dif(u,z),z), True))", MIXED,
     lambda J: W(J["x"] > 0.5, J[5][0] + J[4][0], J[5][0] + 2 * J[4][0])),
]
_IDS = [s[0][:60] for s in STRINGS]
# which of the new opcodes (or a fp32 constant) each program must hold
EMITS = [{"LT", "SEL"}, {"LT", "SEL"}, {"LT", "SEL"}, {"LT", "SEL"}, {"LT", "LE", "EQ", "AND", "OR", "NOT", "SEL"},
         {"NE", "OR", "NOT", "SEL"}, {"LT", "SEL"}, {"LT", "SEL"}, set(), set(), set(), {"STEPC"}, {"LT", "SEL"}]


def _evaluate(eq, field, n=33):
    layer = E._layer(eq)
    p = layer.eqns_jet["e"]
    assert p is not None, "no jet program"
    fld = _Field(*field)
    layer.update_forward_method(fld)
    x = torch.rand(2, n, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    _, generic = layer(x.clone(), return_residue=True)
    _, pairs = E._streams(p)
    jets = fld.jets(x, pairs)
    jet = layer._residues_from_jets(x, types.SimpleNamespace(jets=jets, pairs_out=[tuple(q) for q in pairs]))
    J = {s: [jets[s, c].reshape(2, n, 1) for c in range(2)] for s in range(jets.shape[0])}
    J["x"] = x[..., 2:3]
    return layer, generic["e"], jet["e"], J


@pytest.mark.parametrize("eq,field,formula", STRINGS, ids=_IDS)
def test_string_evaluates_on_both_torch_strategies_and_equals_its_where_formula(eq, field, formula):
    n0 = dict(lig.stats)
    layer, generic, jet, J = _evaluate(eq, field)
    want = formula(J)
    if "Piecewise((u, u > 0))" in eq or "sqrt(u)" in eq:
        assert torch.isnan(want).any() and not torch.isnan(want).all()           # the missing default is exercised
    else:
        assert torch.isfinite(want).all()
    for got in (generic, jet):
        assert got.shape == (2, 33, 1) and got.dtype == torch.float64
        assert torch.allclose(got.detach(), want, rtol=1e-12, atol=1e-12, equal_nan=True), (got.detach() - want).abs().max()
    assert lig.stats.get("jet_compile_errors", 0) == n0.get("jet_compile_errors", 0)


def test_both_branches_of_the_switch_are_taken_by_the_test_points():
    _, _, _, J = _evaluate(STRINGS[1][0], MIXED)
    frac = (J[0][0] > 0).double().mean().item()
    assert 0.2 < frac < 0.8, frac
    assert 0.2 < (J["x"] > 0.5).double().mean().item() < 0.8


def test_gradients_follow_torch_where_on_both_strategies():
    """d/du of Piecewise((u*u_x, u > 0), (w, True)): u_x and 0 on the generic strategy's lambdified function and on the jet
    strategy's, nothing through the condition, and exactly 0 into the branch not taken."""
    layer = E._layer("Piecewise((u*dif(u,x), u > 0), (w, True))")
    p = layer.eqns_jet["e"]
    u = torch.tensor([[[0.0], [2.0], [-2.0]]], dtype=torch.float64, requires_grad=True)
    w = torch.tensor([[[5.0], [6.0], [7.0]]], dtype=torch.float64, requires_grad=True)
    ux = torch.full_like(u, 3.0)
    vals = {(0, ()): u, (0, (2,)): ux, (1, ()): w}
    out = p.fn(*([None] * 3 + [vals[a] for a in p.atoms]))
    out.sum().backward()
    assert out.detach().reshape(-1).tolist() == [5.0, 6.0, 7.0]
    assert u.grad.reshape(-1).tolist() == [0.0, 3.0, 0.0] and w.grad.reshape(-1).tolist() == [1.0, 0.0, 1.0]


def test_number_branches_take_the_dtype_of_the_tensors():
    u = sympy.Symbol("u")
    fn = pde._lambdify([u], sympy.Piecewise((sympy.Rational(1, 10), u > 0), (0, True)))
    for dt in (torch.float32, torch.float64):
        r = fn(torch.tensor([1.0, -1.0], dtype=dt))
        assert r.dtype == dt and r.tolist() == torch.tensor([0.1, 0.0], dtype=dt).tolist()


def test_layers_with_param_vars_take_piecewise_too():
    layer = pde.PDELayer("t, z, x", "u, w", param_vars="nu")
    layer.add_equation("Piecewise((nu*u, u > nu), (w, True))", "e")
    layer.update_parameters({"nu": torch.tensor(0.1)})
    fld = _Field(*MIXED)
    layer.update_forward_method(lambda q: fld(q.double()).float())
    x = torch.rand(2, 9, 3, generator=torch.Generator().manual_seed(3))
    y, res = layer(x.clone())
    want = torch.where(y[..., :1] > 0.1, 0.1 * y[..., :1], y[..., 1:])
    assert torch.allclose(res["e"], want, rtol=1e-6, atol=1e-7)


# ---- the combined second-order stream ---------------------------------------------------------------------------------------------------
def test_combo_plan_gives_up_its_single_stream_inside_a_piecewise_without_raising():
    before = lig.stats.get("combo_plan_errors", 0)
    # different combinations in the two branches; a second derivative in a condition
    for eq in (STRINGS[-1][0], "Piecewise((2*dif(dif(u,x),x) + 2*dif(dif(u,z),z), dif(dif(u,z),z) > 0), (dif(dif(u,x),x) + dif(dif(u,z),z), True))",
               "Piecewise((u, dif(dif(u,z),z) > 0), (w, True)) + dif(dif(u,x),x) + dif(dif(u,z),z)"):
        layer = E._layer(eq)
        assert layer.eqns_jet["e"] is not None and layer._combo_plan() is None, eq
    # the same combination in both: one stream, and the rewritten program equals the pairs' program
    layer = E._layer("Piecewise((u*(dif(dif(u,x),x) + 2*dif(dif(u,z),z)), x > 0.5), (3*dif(dif(u,x),x) + 6*dif(dif(u,z),z), True))")
    plan = layer._combo_plan()
    assert lig.stats.get("combo_plan_errors", 0) == before
    if plan is not None:
        assert plan["alpha"] == {(1, 1): 1.0, (2, 2): 0.5}
        p, q = layer.eqns_jet["e"], plan["progs"]["e"]
        rng = np.random.default_rng(0)
        val = {k: torch.from_numpy(rng.standard_normal(16)) for k in p.atoms}
        xs = [torch.from_numpy(rng.uniform(0, 1, 16)) for _ in range(3)]
        val[(0, ("L",))] = val[(0, (1, 1))] + 0.5 * val[(0, (2, 2))]
        assert torch.allclose(p.fn(*(xs + [val[a] for a in p.atoms])), q.fn(*(xs + [val[a] for a in q.atoms])), rtol=1e-12, atol=1e-12)


# ---- the compiler -------------------------------------------------------------------------------------------------------------------
def _compile(layer):
    """The one equation of the layer the way PDELayer._residues_hip compiles it: extended=True, conditional=True."""
    p = layer.eqns_jet["e"]
    stream_of, _ = E._streams(p)
    slots = {sym: (stream_of[k[1]], k[0]) for k, sym in p.syms.items()}
    return pde._compile_residual_program([p.expr], list(layer.in_vars), slots, extended=True, conditional=True)


def _layer_program(layer, combo, extended):
    """E._layer_program with the switch of the new opcodes on whenever extended is."""
    progs = layer.eqns_jet
    stream_of = {(): 0, (0,): 1, (1,): 2, (2,): 3}
    if combo:
        progs = layer._combo_plan()["progs"]
        stream_of[("L",)] = 4
    else:
        for k, pr in enumerate(sorted({mi for p in progs.values() for _, mi in p.atoms if len(mi) == 2})):
            stream_of[pr] = 4 + k
    slots = {sym: (stream_of[k[1]], k[0]) for p in progs.values() for k, sym in p.syms.items()}
    return pde._compile_residual_program([p.expr for p in progs.values()], list(layer.in_vars), slots, extended=extended,
                                         conditional=extended)


def _ops(prog):
    return {M.NAMES[o] for o in prog["op"].tolist()}


@pytest.mark.parametrize("k", range(len(STRINGS)), ids=_IDS)
def test_string_compiles_only_when_extended_and_the_program_equals_the_lambdified_function(k):
    eq, field, _ = STRINGS[k]
    layer = E._layer(eq)
    p = layer.eqns_jet["e"]
    # the default compiler and the extended one are what they were: the new opcodes need the switch of their own
    assert E._compile(layer, None) is None and E._compile(layer, False) is None and E._compile(layer, True) is None
    comp = _compile(layer)
    assert comp is not None
    prog, uses_x = comp
    assert EMITS[k] <= _ops(prog) and (EMITS[k] or not (_ops(prog) & set(M.OPS_COND))), _ops(prog)
    for i, (op, a, b, c) in enumerate(prog.tolist()):                                  # SSA: the kernels do not check
        assert all(0 <= o < i for o in M.operands(M.NAMES[op], a, b)), (i, M.NAMES[op], a, b)
    stream_of, pairs = E._streams(p)
    x = torch.rand(1, 65, 3, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    jets = _Field(*field).jets(x, pairs)
    cols = [x[..., i:i + 1] for i in range(3)]
    want = p.fn(*(cols + [jets[stream_of[a[1]], a[0]].reshape(1, 65, 1) for a in p.atoms])).reshape(-1).numpy()
    got, = M.run(prog, jets.numpy(), x.reshape(-1, 3).numpy(), np.float64)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6, equal_nan=True)


def test_the_encodings_the_compiler_emits():
    j, k, x = sympy.Symbol("j"), sympy.Symbol("k"), sympy.Symbol("x")
    slots = {j: (0, 0), k: (0, 1)}

    def comp(e):
        r = pde._compile_residual_program([e], [x], slots, extended=True, conditional=True)
        assert r is not None, e
        return [(M.NAMES[o], a, b, c) for o, a, b, c in r[0].tolist()]

    # > and >= are LT and LE with the operands swapped; the chain is built from the last branch backwards
    got = comp(sympy.Piecewise((j, j > k), (k, j >= 0), (x, True)))
    assert got == [("X", 0, 0, 0.0), ("JET", 0, 0, 0.0), ("CONST", 0, 0, 0.0), ("LE", 2, 1, 0.0), ("JET", 0, 1, 0.0),
                   ("SEL", 3, M.sel(4, 0), 0.0), ("LT", 4, 1, 0.0), ("SEL", 6, M.sel(1, 5), 0.0), ("OUT", 7, 0, 0.0)]
    got = comp(sympy.Piecewise((j, j < k)))                                            # no default: CONST NaN
    assert got[0][0] == "CONST" and np.isnan(got[0][3]) and got[-2] == ("SEL", 3, M.sel(1, 0), 0.0)
    # number symbols: the nearest float32, as an operand and as a POWC exponent; only the atoms are folded
    f32 = lambda v: float(np.float32(v))                                               # noqa: E731
    assert comp(sympy.pi * j)[:2] in ([("CONST", 0, 0, f32(np.pi)), ("JET", 0, 0, 0.0)], [("JET", 0, 0, 0.0), ("CONST", 0, 0, f32(np.pi))])
    assert np.float32(np.pi).view(np.int32) == 0x40490fdb
    assert comp(j ** sympy.pi) == [("JET", 0, 0, 0.0), ("POWC", 0, 0, f32(np.pi)), ("OUT", 1, 0, 0.0)]
    assert comp(j ** sympy.E)[1] == ("POWC", 0, 0, f32(np.e))
    assert [i[0] for i in comp(j ** (2 * sympy.pi))] == ["JET", "CONST", "CONST", "MUL", "POW", "OUT"]
    for s, v in ((sympy.EulerGamma, 0.5772156649015329), (sympy.GoldenRatio, 1.618033988749895), (sympy.Catalan, 0.915965594177219)):
        assert comp(s + j)[:2] in ([("CONST", 0, 0, f32(v)), ("JET", 0, 0, 0.0)], [("JET", 0, 0, 0.0), ("CONST", 0, 0, f32(v))])
    assert [i[0] for i in comp(sympy.sqrt(2) * j)] == [i[0] for i in comp(sympy.sqrt(3) * j)]      # other numbers: as before
    # Heaviside: 1/2 stays STEP with c = 0, any other real h0 is STEPC
    assert comp(sympy.Heaviside(j))[1] == ("STEP", 0, 0, 0.0) and comp(sympy.Heaviside(j, sympy.Rational(1, 2)))[1] == ("STEP", 0, 0, 0.0)
    assert comp(sympy.Heaviside(j, 1))[1] == ("STEPC", 0, 0, 1.0) and comp(sympy.Heaviside(j, 0))[1] == ("STEPC", 0, 0, 0.0)
    assert comp(sympy.Heaviside(j, -sympy.Rational(5, 2)))[1] == ("STEPC", 0, 0, -2.5)
    # a condition shared by two Piecewise is one mask
    got = comp(sympy.Piecewise((j, j > 0), (0, True)) + sympy.Piecewise((k, j > 0), (1, True)))
    assert sum(i[0] == "LT" for i in got) == 1 and sum(i[0] == "SEL" for i in got) == 2


def test_out_of_scope_stays_uncompiled():
    j, k = sympy.Symbol("j"), sympy.Symbol("k")
    for e in (sympy.ITE(j > 0, j > 1, j < 2), sympy.erf(j), j * sympy.zoo, sympy.Heaviside(j, k), sympy.Heaviside(j, sympy.oo),
              sympy.Piecewise((j, sympy.Xor(j > 0, k > 0)), (k, True)), sympy.I * j):
        assert pde._compile_residual_program([e], [], {j: (0, 0), k: (0, 1)}, extended=True, conditional=True) is None, e


# ---- limits ---------------------------------------------------------------------------------------------------------------------------
def test_a_program_over_192_instructions_still_falls_back():
    j = sympy.Symbol("j")
    e = sum(sympy.Piecewise((j ** (n + 2), j > sympy.Rational(n, 100)), (n + 1, True)) for n in range(50))
    assert pde._compile_residual_program([e], [], {j: (0, 0)}, extended=True, conditional=True) is None         # both branches count
    small = sum(sympy.Piecewise((j ** (n + 2), j > sympy.Rational(n, 100)), (n + 1, True)) for n in range(20))
    comp = pde._compile_residual_program([small], [], {j: (0, 0)}, extended=True, conditional=True)
    assert comp is not None and len(comp[0]) <= 192


def test_a_bare_relational_factor_still_raises_at_add_equation():
    layer = pde.PDELayer("t, x", "u")
    with pytest.raises(TypeError):
        layer.add_equation("(x > 0.5)*u")
    assert layer.eqn_num == 0
    layer.add_equation("dif(u,t) + Piecewise((u*dif(u,x), u > 0), (0, True))")         # the issue's example: accepted and callable
    layer.update_forward_method(lambda q: torch.sin(q.sum(-1, keepdim=True)))
    y, res = layer(torch.rand(1, 5, 2, dtype=torch.float64))
    assert torch.isfinite(res["eqn_0"]).all()


# ---- nothing that compiled before compiles differently ------------------------------------------------------------------------------------
def test_programs_of_the_parent_are_byte_identical():
    with open(os.path.join(ROOT, "tests", "golden", "residual_programs_parent.json")) as f:
        want = json.load(f)
    layers = {
        "rb2_bench": (physics.get_rb2_pde_layer(mean=E.MEAN, std=E.STD, t_crop=2., z_crop=1., x_crop=1., use_continuity=True), True),
        "rb2_default": (physics.get_rb2_pde_layer(), True),
        "rb2_ra1e5_pr07": (physics.get_rb2_pde_layer(prandtl=0.7, rayleigh=1e5, t_crop=4., z_crop=0.5, x_crop=3.,
                                                     use_continuity=True), True),
    }
    c5 = pde.PDELayer(*E.C5_VARS)
    for n, e in E.C5_EQS.items():
        c5.add_equation(e, n)
    layers["c5"] = (c5, False)
    assert set(layers) == set(want)
    for key, (layer, combo) in layers.items():
        for extended in (True, False):                      # (_layer_program: with conditional=True where extended)
            prog, uses_x = _layer_program(layer, combo, extended)
            assert prog.tobytes() == base64.b64decode(want[key]["program"]), key
            assert len(prog) == want[key]["nins"] and bool(uses_x) == want[key]["uses_x"]


def test_extended_programs_of_the_parent_are_byte_identical():
    """tests/golden/residual_programs_ext_parent.json: the two layers of tests/test_gpu_residual_ext.py (the upwinded power-law
    system and the graphed step's), compiled with extended=True by the commit before the conditional opcodes."""
    with open(os.path.join(ROOT, "tests", "golden", "residual_programs_ext_parent.json")) as f:
        want = json.load(f)
    assert set(want) == {"upwind", "graphed"}
    for key, w in want.items():
        layer = pde.PDELayer(w["in_vars"], w["out_vars"])
        for n, e in w["equations"]:
            layer.add_equation(e, n)
        assert (layer._combo_plan() is not None) == w["combo"], key
        prog, uses_x = _layer_program(layer, w["combo"], True)
        assert prog.tobytes() == E._layer_program(layer, w["combo"], True)[0].tobytes()       # and without the new switch
        assert prog.tobytes() == base64.b64decode(w["program"]), key
        assert len(prog) == w["nins"] and bool(uses_x) == w["uses_x"]
        assert not (_ops(prog) & set(M.OPS_COND)) and _ops(prog) & {"MAX", "MIN", "POWC"}
