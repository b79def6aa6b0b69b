"""Max / Min / sign / Heaviside, real and expression powers, tan sinh cosh asin acos atan atan2 in PDELayer equations, everything
that needs no GPU: the model of the appended opcodes (tests/residual_model.py) against torch's fp64 autograd at the ties, zeros,
infinities, NaN, base 0 and negative bases; the equation strings that could not run on both torch strategies against hand-written
formulas; their device programs (``_compile_residual_program(..., extended=True)``) through the model against the lambdified
functions; and that nothing that compiled before compiles differently."""
import base64
import json
import os
import types

import numpy as np
import pytest
import sympy
import torch

from space_time_pde_amd import pde, physics
from tests import residual_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---- the model's adjoints against torch's fp64 autograd ---------------------------------------------------------------------------
def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", np.flatnonzero(np.isnan(got) != nan)[:8])
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (what, "infinities")
    ok = ~nan & ~inf
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=1e-300, err_msg=what)


def _against_autograd(prog, jets, cot, what):
    """Values and adjoint of the fp64 model against the same program made of torch's operators, differentiated by autograd."""
    jets = np.asarray(jets, dtype=np.float64)
    cot = np.asarray(cot, dtype=np.float64)
    jt = torch.from_numpy(jets.copy()).requires_grad_(True)
    outs = M.torch_program(prog, jt, None)
    sum((o * torch.from_numpy(cot[k])).sum() for k, o in enumerate(outs)).backward()
    vals = M.run(prog, jets, None, np.float64)
    for k, o in enumerate(outs):
        _same(vals[k], o.detach().numpy(), "%s value %d" % (what, k))
    _same(M.adjoint(prog, jets, None, cot, np.float64), jt.grad.numpy(), what + " adjoint")


@pytest.mark.parametrize("name", ["MIN", "MAX", "SIGN", "STEP"])
def test_min_max_sign_step_at_ties_zeros_infinities_and_nan(name):
    prog, jets, _, cot = M.exact_case(name)
    _against_autograd(prog, jets, cot, name)
    # the conventions, literally (cotangent 1 on the edge rows)
    bar = M.adjoint(prog, jets, None, cot, np.float32)
    val = M.run(prog, jets, None, np.float32)
    if name in ("MIN", "MAX"):
        for a, b in ((0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (1.0, 1.0), (INF, INF), (-INF, -INF)):
            i = M.edge_index(a, b)
            # out 0 = op(a, b), out 1 = op(b, b), out 2 = op(b, a): a gets 1/2 + 1/2, b gets 1/2 + (1/2 + 1/2) + 1/2
            assert bar[0, 0, i] == 1.0 and bar[0, 1, i] == 2.0, (name, a, b)
        i = M.edge_index(1.0, -1.0)
        assert (bar[0, 0, i], bar[0, 1, i]) == ((2.0, 1.0) if name == "MAX" else (0.0, 3.0))
        for a, b in ((NAN, 1.0), (1.0, NAN), (NAN, NAN), (INF, NAN)):
            i = M.edge_index(a, b)
            assert np.isnan(val[0][i]) and np.isnan(val[2][i]), (name, a, b)
            # torch: a NaN operand passes the cotangent to both (op(b, b) is a tie unless b is NaN)
            assert bar[0, 0, i] == 2.0 and bar[0, 1, i] == (4.0 if np.isnan(b) else 3.0), (name, a, b)
    else:
        want = {0.0: 0.0, -0.0: 0.0, 1.0: 1.0, -1.0: -1.0, INF: 1.0, -INF: -1.0} if name == "SIGN" else \
            {0.0: 0.5, -0.0: 0.5, 1.0: 1.0, -1.0: 0.0, INF: 1.0, -INF: 0.0}
        for a, w in want.items():
            i = M.edge_index(a)
            assert val[0][i] == w and (a != 0 or not np.signbit(val[0][i])), (name, a, val[0][i])
            assert bar[0, 0, i] == w or (np.isnan(bar[0, 0, i]) and np.isinf(a) and w == 0), (name, a)   # only through the MUL
        assert np.isnan(val[0][M.edge_index(NAN)])


def _pow_inputs():
    base = np.array([0.0, -0.0, -1.0, -2.5, -0.3, 0.5, 1.0, 2.0, 7.25, 1e-3, 1e3], dtype=np.float64)
    rng = np.random.default_rng(5)
    return np.concatenate([base, rng.choice([-1.0, 1.0], 64) * 10.0 ** rng.uniform(-2, 2, 64)])


@pytest.mark.parametrize("c", [1.0, 1.0 / 3.0, 4.0 / 3.0, 1.5, 2.5, -0.5, -2.0, 3.0, 0.0])
def test_powc_at_base_zero_and_negative_bases(c):
    x = _pow_inputs()
    if c == -0.5:       # torch evaluates x ** -0.5 as rsqrt, -inf at -0; the evaluator's is the IEEE pow, +inf at both zeros
        x = np.delete(x, 1)
    prog = M.program(("JET", 0, 0), ("POWC", 0, 0, c), ("OUT", 1, 0))
    cot = np.random.default_rng(6).standard_normal((1, len(x)))
    _against_autograd(prog, x[None, None], cot, "POWC %r" % c)
    bar = M.adjoint(prog, x[None, None], None, np.ones((1, len(x))), np.float64)[0, 0]
    neg = x < 0
    if c >= 1:          # a regular point: c 0^(c-1), no division by the base
        assert bar[0] == (1.0 if c == 1 else 0.0)
    elif c != 0:
        assert np.isinf(bar[0])
    if c != int(c):
        assert neg.sum() > 20 and np.isnan(bar[neg]).all()


def test_pow_at_base_zero_negative_bases_and_exponent_zero():
    x = _pow_inputs()
    e = np.array([-2.0, -0.5, 0.0, -0.0, 0.5, 1.0, 1.5, 2.0, 3.0])
    a, b = np.repeat(x, len(e)), np.tile(e, len(x))
    prog = M.program(("JET", 0, 0), ("JET", 0, 1), ("POW", 0, 1), ("OUT", 2, 0), ("CONST", 0, 0, 2.0), ("POW", 4, 1), ("OUT", 5, 1))
    cot = np.random.default_rng(7).standard_normal((2, len(a)))
    _against_autograd(prog, np.stack([a, b])[None], cot, "POW")


@pytest.mark.parametrize("name", ["TAN", "SINH", "COSH", "ASIN", "ACOS", "ATAN", "ATAN2"])
def test_math_library_opcodes_against_autograd(name):
    rng = np.random.default_rng(8)
    if name in ("ASIN", "ACOS"):
        x = np.concatenate([[1.0, -1.0, 0.0, -0.0, 0.5], rng.uniform(-1, 1, 59)])      # +-1: an infinite adjoint, like torch's
    else:
        x = np.concatenate([[0.0, -0.0, 1.0, -1.0], rng.uniform(-3, 3, 60)])
    if name == "ATAN2":
        jets = np.stack([x, np.concatenate([[0.0, 1.0, -0.0, 0.0], rng.uniform(-3, 3, 60)])])[None]
        prog = M.program(("JET", 0, 0), ("JET", 0, 1), (name, 0, 1), ("OUT", 2, 0))
    else:
        jets = x[None, None]
        prog = M.program(("JET", 0, 0), (name, 0), ("OUT", 1, 0))
    _against_autograd(prog, jets, rng.standard_normal((1, len(x))), name)
    if name in ("ASIN", "ACOS"):
        bar = M.adjoint(prog, jets, None, np.ones((1, len(x))), np.float64)[0, 0]
        assert bar[0] == bar[1] == (INF if name == "ASIN" else -INF)


# ---- the equation strings ---------------------------------------------------------------------------------------------------------
class _Field:
    """y_c = off + amp sin(a_c . x + b_c) of x = (t, z, x): values and derivatives in closed form, fp64."""

    def __init__(self, off, amp):
        g = torch.Generator().manual_seed(11)
        self.a = 0.5 + torch.rand(2, 3, generator=g, dtype=torch.float64)
        self.b = torch.rand(2, generator=g, dtype=torch.float64)
        self.off, self.amp = off, amp

    def __call__(self, x):
        return self.off + self.amp * torch.sin(x @ self.a.t() + self.b)

    def jets(self, x, pairs):
        ph = (x @ self.a.t() + self.b).reshape(-1, 2).t()
        rows = [self.off + self.amp * torch.sin(ph)]
        rows += [self.amp * self.a[:, d:d + 1] * torch.cos(ph) for d in range(3)]
        rows += [-self.amp * (self.a[:, i:i + 1] * self.a[:, j:j + 1]) * torch.sin(ph) for i, j in pairs]
        return torch.stack(rows)


MIXED, POS = (0.0, 0.9), (1.2, 0.5)        # u, w change sign within (-1, 1) / stay in [0.7, 1.7]
H = lambda a: torch.where(a > 0, 1.0, torch.where(a < 0, 0.0, 0.5)).to(a.dtype)        # noqa: E731
# (equation, field, fp64 formula of the jets J[stream][channel]: stream 0 value, 1..3 d/dt d/dz d/dx; channel 0 u, 1 w)
STRINGS = [
    ("Max(u,0)*dif(u,x)", MIXED, lambda J: torch.clamp(J[0][0], min=0) * J[3][0]),
    ("Min(u,w)", MIXED, lambda J: torch.minimum(J[0][0], J[0][1])),
    ("sign(u)*dif(u,x)", MIXED, lambda J: torch.sign(J[0][0]) * J[3][0]),
    ("Heaviside(u)*dif(w,t)", MIXED, lambda J: H(J[0][0]) * J[1][1]),
    ("dif(Max(u,0),x)", MIXED, lambda J: H(J[0][0]) * J[3][0]),
    ("atan(u)", MIXED, lambda J: torch.atan(J[0][0])),
    ("asin(u)", MIXED, lambda J: torch.asin(J[0][0])),
    ("atan2(u,w)", MIXED, lambda J: torch.atan2(J[0][0], J[0][1])),
    ("dif(Abs(u),x)", MIXED, lambda J: torch.sign(J[0][0]) * J[3][0]),
    ("u**1.5", POS, lambda J: J[0][0] * torch.sqrt(J[0][0])),
    ("u**(1/3)", POS, lambda J: torch.exp(torch.log(J[0][0]) / 3)),
    ("u**Rational(4,3)", POS, lambda J: J[0][0] * torch.exp(torch.log(J[0][0]) / 3)),
    ("u**w", POS, lambda J: torch.exp(J[0][1] * torch.log(J[0][0]))),
    ("u**2.0", MIXED, lambda J: J[0][0] * J[0][0]),
    ("dif(u,x)**2.0", MIXED, lambda J: J[3][0] * J[3][0]),
    ("tan(u)", MIXED, lambda J: torch.sin(J[0][0]) / torch.cos(J[0][0])),
    ("sinh(u)+cosh(w)", MIXED, lambda J: (torch.exp(J[0][0]) - torch.exp(-J[0][0])) / 2 + (torch.exp(J[0][1]) + torch.exp(-J[0][1])) / 2),
    # n-ary with a number, the other inverse function, an upwinded flux with second derivatives
    ("Max(u,w,0.25)-Min(u,w,-0.25,x)", MIXED,
     lambda J: torch.clamp(torch.maximum(J[0][0], J[0][1]), min=0.25) - torch.minimum(torch.clamp(torch.minimum(J[0][0], J[0][1]), max=-0.25), J["x"])),
    ("acos(u)*dif(dif(w,x),x)", MIXED, lambda J: torch.acos(J[0][0]) * J[4][1]),
]
_IDS = [s[0] for s in STRINGS]


def _layer(eq):
    layer = pde.PDELayer("t, z, x", "u, w")
    layer.add_equation(eq, "e")
    return layer


def _streams(prog):
    stream_of = {(): 0, (0,): 1, (1,): 2, (2,): 3}
    pairs = sorted({mi for _, mi in prog.atoms if len(mi) == 2})
    for k, pr in enumerate(pairs):
        stream_of[pr] = 4 + k
    return stream_of, pairs


def _compile(layer, extended):
    p = layer.eqns_jet["e"]
    stream_of, _ = _streams(p)
    slots = {sym: (stream_of[k[1]], k[0]) for k, sym in p.syms.items()}
    if extended is None:
        return pde._compile_residual_program([p.expr], list(layer.in_vars), slots)
    return pde._compile_residual_program([p.expr], list(layer.in_vars), slots, extended=extended)


@pytest.mark.parametrize("eq,field,formula", STRINGS, ids=_IDS)
def test_string_evaluates_on_both_torch_strategies_and_equals_its_formula(eq, field, formula):
    layer = _layer(eq)
    p = layer.eqns_jet["e"]
    assert p is not None, "no jet program"
    fld = _Field(*field)
    layer.update_forward_method(fld)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 33, 3, generator=g, dtype=torch.float64)
    _, generic = layer(x.clone(), return_residue=True)
    _, pairs = _streams(p)
    jets = fld.jets(x, pairs)
    req = types.SimpleNamespace(jets=jets, pairs_out=[tuple(q) for q in pairs])
    jet = layer._residues_from_jets(x, req)
    J = {s: [jets[s, c].reshape(2, 33, 1) for c in range(2)] for s in range(jets.shape[0])}
    J["x"] = x[..., 2:3]
    want = formula(J)
    assert torch.isfinite(want).all()
    for got in (generic["e"], jet["e"]):
        assert got.shape == (2, 33, 1) and got.dtype == torch.float64
        assert torch.allclose(got.detach(), want, rtol=1e-12, atol=1e-12), (got.detach() - want).abs().max()


@pytest.mark.parametrize("eq,field,formula", STRINGS, ids=_IDS)
def test_string_compiles_only_when_extended_and_the_program_equals_the_lambdified_function(eq, field, formula):
    layer = _layer(eq)
    p = layer.eqns_jet["e"]
    assert _compile(layer, None) is None and _compile(layer, False) is None       # the default compiler is what it was
    comp = _compile(layer, True)
    assert comp is not None
    prog, uses_x = comp
    if eq.endswith("**2.0"):                     # an integral Float exponent: the exact POWI
        assert prog["op"].tolist() == [M.OPS["JET"], M.OPS["POWI"], M.OPS["OUT"]] and prog["b"][1] == 2
    else:
        assert set(prog["op"].tolist()) & set(M.OPS_EXT.values())
    stream_of, pairs = _streams(p)
    g = torch.Generator().manual_seed(4)
    x = torch.rand(1, 65, 3, generator=g, dtype=torch.float64)
    jets = _Field(*field).jets(x, pairs)
    cols = [x[..., i:i + 1] for i in range(3)]
    want = p.fn(*(cols + [jets[stream_of[a[1]], a[0]].reshape(1, 65, 1) for a in p.atoms])).reshape(-1).numpy()
    got, = M.run(prog, jets.numpy(), x.reshape(-1, 3).numpy(), np.float64)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)


def test_layer_gradients_agree_between_the_strategies_at_a_tie():
    """Max(u, 0) at u = 0 exactly: half the cotangent reaches u on the generic strategy (torch.maximum), and the jet strategy's
    dif(Max(u,0),x) = Heaviside(u) u_x has H(0) = 1/2."""
    layer = _layer("Max(u,0)+dif(Max(u,0),x)")
    u = torch.tensor([[[0.0], [2.0], [-2.0]]], dtype=torch.float64, requires_grad=True)
    p = layer.eqns_jet["e"]
    ux = torch.full_like(u, 3.0)
    vals = {(0, ()): u, (0, (2,)): ux}
    out = p.fn(*([None] * 3 + [vals[a] for a in p.atoms]))
    out.sum().backward()
    assert out.detach().reshape(-1).tolist() == [1.5, 5.0, 0.0]
    assert u.grad.reshape(-1).tolist() == [0.5, 1.0, 0.0]


def test_abs_under_dif_expands_as_a_real_function():
    layer = _layer("dif(Abs(u),x)")
    p = layer.eqns_jet["e"]
    assert p is not None and not p.expr.has(sympy.re, sympy.im, sympy.Derivative)
    assert p.expr == sympy.sign(p.syms[(0, ())]) * p.syms[(0, (2,))]
    # second order: sign' = 0, as torch.sign's
    p2 = _layer("dif(dif(Abs(u),x),x)").eqns_jet["e"]
    assert p2.expr == sympy.sign(p2.syms[(0, ())]) * p2.syms[(0, (2, 2))]
    # without a dif above it Abs stays what it was
    p3 = _layer("Abs(dif(u,x))-Abs(w)").eqns_jet["e"]
    assert p3.expr == sympy.Abs(p3.syms[(0, (2,))]) - sympy.Abs(p3.syms[(1, ())])


def test_out_of_envelope_stays_uncompiled():
    j = sympy.Symbol("j")
    for e in (j ** sympy.pi, sympy.Piecewise((j, j > 0), (0, True)), sympy.Heaviside(j, 0), sympy.erf(j)):
        assert pde._compile_residual_program([e], [], {j: (0, 0)}, extended=True) is None, e


# ---- nothing that compiled before compiles differently ------------------------------------------------------------------------------
MEAN, STD = (0.01, 0.0, 0.02, -0.01), (0.05, 0.3, 0.15, 0.12)
C5_VARS = ("x, y, t", "c, u, v, w, p")
C5_EQS = {
    "adv_diff": "dif(c,t)+u*dif(c,x)+v*dif(c,y)-0.01*(dif(dif(c,x),x)+dif(dif(c,y),y))",
    "prod_rule": "dif(u*c,x)+dif(v*c,y)",
    "mixed": "dif(dif(c,x),y)-w*p",
    "explicit_x": "x*dif(p,x)+t*dif(dif(p,t),t)",
}


def _layer_program(layer, combo, extended):
    progs = layer.eqns_jet
    stream_of = {(): 0, (0,): 1, (1,): 2, (2,): 3}
    if combo:
        progs = layer._combo_plan()["progs"]
        stream_of[("L",)] = 4
    else:
        for k, pr in enumerate(sorted({mi for p in progs.values() for _, mi in p.atoms if len(mi) == 2})):
            stream_of[pr] = 4 + k
    slots = {sym: (stream_of[k[1]], k[0]) for p in progs.values() for k, sym in p.syms.items()}
    return pde._compile_residual_program([p.expr for p in progs.values()], list(layer.in_vars), slots, extended=extended)


def test_rb2_and_config4_programs_are_byte_identical_to_the_parents_when_extended():
    with open(os.path.join(ROOT, "tests", "golden", "residual_programs_parent.json")) as f:
        want = json.load(f)
    layers = {
        "rb2_bench": (physics.get_rb2_pde_layer(mean=MEAN, std=STD, t_crop=2., z_crop=1., x_crop=1., use_continuity=True), True),
        "rb2_default": (physics.get_rb2_pde_layer(), True),
        "rb2_ra1e5_pr07": (physics.get_rb2_pde_layer(prandtl=0.7, rayleigh=1e5, t_crop=4., z_crop=0.5, x_crop=3.,
                                                     use_continuity=True), True),
    }
    c5 = pde.PDELayer(*C5_VARS)
    for n, e in C5_EQS.items():
        c5.add_equation(e, n)
    layers["c5"] = (c5, False)
    for key, (layer, combo) in layers.items():
        prog, uses_x = _layer_program(layer, combo, True)
        assert prog.tobytes() == base64.b64decode(want[key]["program"]), key
        assert len(prog) == want[key]["nins"] and bool(uses_x) == want[key]["uses_x"]
    # and the all-opcode set of tests/residual_model.py, which has no golden bytes: extended against default
    layer = M.all_ops_layer()
    assert _layer_program(layer, False, True)[0].tobytes() == _layer_program(layer, False, False)[0].tobytes()
