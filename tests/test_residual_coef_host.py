"""Coefficient tensors read inside the HIP residual kernels (PDELayer(device_params=True), stpde_residual_coef_fwd / _bwd),
everything that needs no GPU: the compiler with and without coefficient slots, the host model (tests/residual_params_model.py)
against torch's fp64 autograd, the layer on the CPU, the C ABI's argument checks and what GraphedStep accepts."""
import base64
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from space_time_pde_amd import pde, physics
from tests import residual_model as M
from tests import residual_params_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BURGERS_F = "dif(u,t)+u*dif(u,x)-nu*dif(dif(u,x),x)-amp*sin(x)"
MEAN, STD = (0.01, 0.0, 0.02, -0.01), (0.05, 0.3, 0.15, 0.12)
RB2 = dict(mean=MEAN, std=STD, t_crop=2., z_crop=1., x_crop=1., use_continuity=True)


def _layout(layer, combo):
    progs = layer.eqns_jet
    stream_of = {(): 0, (0,): 1, (1,): 2, (2,): 3}
    if combo:
        plan = layer._combo_plan()
        assert plan is not None
        progs = plan["progs"]
        stream_of[("L",)] = 4
    else:
        pairs = sorted({mi for p in progs.values() for _, mi in p.atoms if len(mi) == 2})
        for k, pr in enumerate(pairs):
            stream_of[pr] = 4 + k
    slots = {sym: (stream_of[k[1]], k[0]) for p in progs.values() for k, sym in p.syms.items()}
    return progs, slots, stream_of


def _compile(layer, combo, coef_slots="layer", **kw):
    progs, slots, stream_of = _layout(layer, combo)
    if coef_slots == "layer":
        coef_slots = {s: k for k, s in enumerate(layer.param_vars)}
    comp = pde._compile_residual_program([p.expr for p in progs.values()], list(layer.in_vars), slots, extended=True,
                                         conditional=True, coef_slots=coef_slots, **kw)
    return comp, stream_of


def _burgers_layer(device_params=False, extra=""):
    layer = pde.PDELayer("x, t", "u", "nu, amp" + extra, device_params=device_params)
    layer.add_equation(BURGERS_F, "burgers")
    return layer


# ---- the compiler -------------------------------------------------------------------------------------------------------------
def test_without_slots_the_compiler_gives_the_parent_commits_bytes():
    with open(os.path.join(ROOT, "tests", "golden", "residual_programs_parent.json")) as f:
        want = json.load(f)
    rb2 = physics.get_rb2_pde_layer(**RB2)
    progs, slots, _ = _layout(rb2, True)
    for kw in (dict(), dict(coef_slots=None)):
        prog, uses_x = pde._compile_residual_program([p.expr for p in progs.values()], list(rb2.in_vars), slots, **kw)
        assert prog.tobytes() == base64.b64decode(want["rb2_bench"]["program"]) and bool(uses_x) == want["rb2_bench"]["uses_x"]
    # an empty mapping changes the return value's length only
    prog3 = pde._compile_residual_program([p.expr for p in progs.values()], list(rb2.in_vars), slots, coef_slots={})
    assert prog3[0].tobytes() == prog.tobytes() and prog3[1] == uses_x and prog3[2] == []
    layer = M.all_ops_layer()
    a, a_x, stream_of = M.all_ops_program(layer)
    progs, slots, _ = _layout(layer, False)
    b = pde._compile_residual_program([p.expr for p in progs.values()], list(layer.in_vars), slots, coef_slots=None)
    assert len(b) == 2 and b[0].tobytes() == a.tobytes() and b[1] == a_x
    assert not ((a["op"] == M.OPS["CONST"]) & ((a["a"] != 0) | (a["b"] != 0))).any()
    # a coefficient symbol without slots is what it was: not compiled
    assert _compile(_burgers_layer(), False, coef_slots=None)[0] is None


@pytest.mark.parametrize("case", ["burgers", "rb2"])
def test_with_slots_every_used_coefficient_is_one_late_bound_const(case):
    if case == "burgers":
        layer, combo, names = _burgers_layer(extra=", unused"), False, ["nu", "amp", "unused"]
        want_used = [0, 1]
    else:
        layer = physics.get_rb2_pde_layer(prandtl=torch.tensor(0.7), rayleigh=torch.tensor([1e6, 1e5]), **RB2)
        combo, names, want_used = True, ["Ra", "Pr"], [0, 1]
    assert [s.name for s in layer.param_vars] == names
    (prog, uses_x, used), _ = _compile(layer, combo)
    assert used == want_used                                       # (burgers: slot 2 is declared and not read)
    const = prog["op"] == M.OPS["CONST"]
    late = const & (prog["b"] != 0)
    assert sorted(prog["a"][late].tolist()) == want_used           # exactly one instruction per used coefficient
    assert (prog["b"][late] == 1).all() and (prog["c"][late] == 0).all()
    assert (prog["a"][const & ~late] == 0).all()
    assert PM.late_bound(prog) == prog["a"][late].tolist()
    assert len(prog) <= pde._RES_MAX_INS and set(prog["op"].tolist()) <= set(M.OPS.values())
    if case == "rb2":
        # (Ra Pr)^(-1/2) is DIV(CONST 1, SQRT(MUL)): exact opcodes only, so the device must match the fp32 model bit for bit
        exact = {M.OPS[n] for n in ("JET", "X", "CONST", "ADD", "SUB", "MUL", "DIV", "NEG", "POWI", "SQRT", "OUT")}
        assert set(prog["op"].tolist()) <= exact
        # slots of a subset: the coefficient left out does not compile
        assert _compile(layer, True, coef_slots={layer.param_vars[0]: 0})[0] is None
    # other numbering, same program up to the a field of the late-bound CONSTs
    (prog2, _, used2), _ = _compile(layer, combo, coef_slots={s: 7 - k for k, s in enumerate(layer.param_vars)})
    assert used2 == sorted(7 - k for k in want_used)
    same = prog.copy()
    same["a"][late] = 7 - same["a"][late]
    assert prog2.tobytes() == same.tobytes()


# ---- the host model against torch's fp64 autograd -------------------------------------------------------------------------------
def _case(case, B, N, seed):
    """(prog, jets64 [S, C, P], x64 [P, 3] or None, cot64 [n_eq, P], [value leaves], [per_batch])."""
    g = torch.Generator().manual_seed(seed)
    if case == "burgers":
        layer = _burgers_layer()
        (prog, uses_x, used), stream_of = _compile(layer, False)
        S, C = max(stream_of.values()) + 1, 1
        vals = [torch.tensor(0.05, dtype=torch.float64), torch.tensor([0.3, -0.2, 0.7][:B], dtype=torch.float64)]
    else:
        layer = physics.get_rb2_pde_layer(prandtl=torch.tensor(0.7), rayleigh=torch.tensor([1e6] * B), **RB2)
        (prog, uses_x, used), stream_of = _compile(layer, True)
        S, C = 5, 4
        vals = [torch.tensor([1e6, 1e5, 3e4][:B], dtype=torch.float64), torch.tensor(0.7, dtype=torch.float64)]
    assert used == [0, 1]
    P = B * N
    jets = torch.randn(S, C, P, generator=g, dtype=torch.float64)
    x = torch.rand(P, 3, generator=g, dtype=torch.float64) if uses_x else None
    n_eq = int((prog["op"] == M.OPS["OUT"]).sum())
    cot = torch.randn(n_eq, P, generator=g, dtype=torch.float64)
    return prog, jets, x, cot, vals, [v.dim() == 1 for v in vals]


@pytest.mark.parametrize("case", ["burgers", "rb2"])
def test_model_values_adjoints_and_coefficient_gradients_match_torch_autograd(case):
    B, N = 3, 7
    prog, jets, x, cot, vals, per_batch = _case(case, B, N, 21)
    S, C, P = jets.shape
    leaves = [v.clone().requires_grad_(True) for v in vals]
    jt = jets.clone().requires_grad_(True)
    rows = [t.repeat_interleave(N) if pb else t.expand(P) for t, pb in zip(leaves, per_batch)]
    pad = [torch.zeros(P, dtype=torch.float64)] * (max(C, len(rows)) - len(rows))
    stream = torch.stack(rows + pad)[None]
    body = jt if C >= len(rows) else torch.cat([jt, torch.zeros(S, len(rows) - C, P, dtype=torch.float64)], 1)
    res = M.torch_program(PM.rewrite(prog, S), torch.cat([body, stream], 0), x)
    (torch.stack(res) * cot).sum().backward()
    values = [v.numpy() for v in vals]
    xn = None if x is None else x.numpy()
    got = PM.run(prog, jets.numpy(), xn, values, B)
    jbar, gco = PM.adjoint(prog, jets.numpy(), xn, cot.numpy(), values, B)
    assert gco.shape == (2, P) and jbar.shape == (S, C, P)

    def rel(a, b):
        return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()

    for k, r in enumerate(res):
        assert rel(got[k], r.detach().numpy()) < 1e-12, k
    assert rel(jbar, jt.grad.numpy()) < 1e-12
    for k, (leaf, pb) in enumerate(zip(leaves, per_batch)):
        want = leaf.grad.numpy()
        have = PM.coef_grad64(gco[k], B, pb)
        assert have.shape == want.shape and np.abs(want).min() > 0
        assert rel(have, want) < 1e-12, k
    # the fp32 model is the same computation in float32
    got32 = PM.run(prog, jets.numpy(), xn, values, B, dtype=np.float32)
    assert got32[0].dtype == np.float32 and rel(got32[0], got[0]) < 1e-4


def test_bound_counts_the_roundings_of_the_reduction():
    assert PM.coef_sum_bound(1, 1, True, False) == 9 and PM.coef_sum_bound(1, 1, False, True) == 9
    assert PM.coef_blocks(257, 3, True) == 2 and PM.coef_blocks(257, 3, False) == 6 and PM.coef_blocks(256, 3, True) == 1
    assert PM.coef_sum_bound(600, 2, True, False) == 11 and PM.coef_sum_bound(600, 2, False, False) == 14
    assert PM.coef_sum_bound(600, 2, False, True) == 9
    # the bound holds for a float32 emulation of the kernel's tree on the worst kind of input (one sign, all magnitudes)
    rng = np.random.default_rng(5)
    g = (10.0 ** rng.uniform(-3, 3, 600)).astype(np.float32)
    blocks = [np.concatenate([g[o:o + 256], np.zeros(256 - len(g[o:o + 256]), np.float32)]) for o in range(0, 600, 256)]
    total = np.float32(0)
    for blk in blocks:
        w = blk.reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, np.arange(64) ^ o]
        total = total + ((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))
    ref = g.astype(np.float64).sum()
    assert abs(float(total) - ref) <= PM.coef_sum_bound(600, 1, True, False) * PM.U * ref


# ---- the layer on the CPU ---------------------------------------------------------------------------------------------------------
def test_cpu_layer_with_the_flag_is_the_layer_without_it():
    import types
    from tests.test_residual_params_host import _Field
    B, N = 3, 17
    g = torch.Generator().manual_seed(2)
    x = torch.rand(B, N, 2, generator=g)
    cot = torch.randn(B, N, 1, generator=g)
    out = []
    for flag in (False, True):
        layer = _burgers_layer(device_params=flag)
        assert layer.device_params is flag
        vals = {"nu": torch.tensor(0.05, requires_grad=True), "amp": torch.tensor([0.3, 0.6, 0.15], requires_grad=True)}
        layer.update_parameters(vals)
        field = _Field(2, 1, torch.float32)
        layer.update_forward_method(field)
        _, generic = layer(x.clone(), return_residue=True)
        req = types.SimpleNamespace(jets=field.jets(x, [(0, 0)]), pairs_out=[(0, 0)])
        jet = layer._residues_from_jets(x, req)
        (jet["burgers"] * cot).sum().backward()
        out.append((generic["burgers"].detach(), jet["burgers"].detach(), vals["nu"].grad, vals["amp"].grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert pde.PDELayer("x, t", "u", "nu").device_params is False
    assert physics.get_rb2_pde_layer(rayleigh=torch.tensor([1e6]), device_params=True).device_params is True
    assert physics.get_rb2_pde_layer(rayleigh=torch.tensor([1e6])).device_params is False
    assert _burgers_layer(device_params=True).device_program_compiles()
    nine = pde.PDELayer("x, t", "u", "a0, a1, a2, a3, a4, a5, a6, a7, a8", device_params=True)
    nine.add_equation("a0*u+a8", "e")
    assert not nine.device_program_compiles()                       # more coefficients than the kernels stage


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_two_entry_points_and_checks_the_record(hiplib):
    from space_time_pde_amd import _lib
    assert hiplib.stpde_version() == _lib.ABI_VERSION == 316
    assert {"stpde_residual_coef_fwd", "stpde_residual_coef_bwd"} <= set(_lib.exported_symbols())
    assert _lib.RES_MAX_COEF == 8 and ctypes.sizeof(_lib.ResCoefs) == 3 * 4 + 8 * 4 + 4 + 8 * 8 + 8 * 8
    hdr = open(os.path.join(ROOT, "include", "stpde_hip.h")).read()
    assert "#define STPDE_RES_MAX_COEF 8" in hdr
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before a launch
    P = 12

    def calls(rec):
        r = None if rec is None else ctypes.byref(rec)
        return (hiplib.stpde_residual_coef_fwd(fake, 4, 1, 1, P, fake, P, P, None, fake, r, None),
                hiplib.stpde_residual_coef_bwd(fake, 4, 1, 1, P, fake, P, P, None, fake, fake, r, None))

    def good():
        rec = _lib.ResCoefs()
        rec.n, rec.n_per_batch = 2, 4
        rec.value[0] = rec.value[1] = 256
        return rec

    bad = [None]
    for n in (0, -1, 9):
        rec = good()
        rec.n = n
        bad.append(rec)
    for npb in (0, -4, 5, 24):                # <= 0, and P % n_per_batch != 0
        rec = good()
        rec.n_per_batch = npb
        bad.append(rec)
    rec = good()
    rec.value[1] = None
    bad.append(rec)
    for rec in bad:
        for rc in calls(rec):
            assert rc == 1                    # STPDE_E_BADARG
            with pytest.raises(ValueError):
                _lib.check(rc)
    # the checks of the old entry points come first and are what they were
    assert hiplib.stpde_residual_coef_fwd(None, 4, 1, 1, P, fake, P, P, None, fake, ctypes.byref(good()), None) == 1
    assert hiplib.stpde_residual_coef_fwd(fake, 193, 1, 1, P, fake, P, P, None, fake, ctypes.byref(good()), None) == 1
    assert hiplib.stpde_residual_coef_bwd(fake, 4, 1, 1, P, fake, P, P, None, fake, None, ctypes.byref(good()), None) == 1


# ---- GraphedStep ----------------------------------------------------------------------------------------------------------------
def test_graphed_step_still_refuses_the_default_layer_and_a_non_leaf_coefficient():
    from space_time_pde_amd.train_step import GraphedStep
    layer = pde.PDELayer("x, t", "u", "nu")
    with pytest.raises(NotImplementedError, match="device_params=True"):
        GraphedStep(None, None, layer, None, None, None, 1)
    log_nu = torch.tensor(-3.0, requires_grad=True)
    layer = pde.PDELayer("x, t", "u", "nu", device_params=True)
    layer.add_equation("dif(u,t)+u*dif(u,x)-nu*dif(dif(u,x),x)", "burgers")
    layer.update_parameters({"nu": log_nu.exp()})
    with pytest.raises(NotImplementedError, match="leaf"):
        GraphedStep(None, None, layer, None, None, None, 1)
    # a layer whose equations the device evaluator does not take is refused as well
    layer = pde.PDELayer("x, t", "u", "nu", device_params=True)
    layer.add_equation("nu*erf(u)", "erf")
    layer.update_parameters({"nu": torch.tensor(0.1, requires_grad=True)})
    with pytest.raises(NotImplementedError, match="evaluator"):
        GraphedStep(None, None, layer, None, None, None, 1)
