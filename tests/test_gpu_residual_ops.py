"""The residual evaluator and the loss kernels of csrc/residual.hip on the device, opcode by opcode and element by element, against
tests/residual_model.py (whose adjoint rules tests/test_residual_model_host.py checks against torch's autograd).

Hand-assembled stpde_res_ins programs are driven through pde._ResidualHip.apply, with the program tensor built the way
PDELayer._residues_hip builds it.

* Exact opcodes (JET X CONST ADD SUB MUL DIV NEG ABS SQRT OUT, POWI with exponents -3 -1 0 1 2 3 7): fixed sequences of IEEE
  operations (-ffp-contract=off, no fast-math, correctly rounded fp32 divide and square root), so values and adjoints are
  BIT-EQUAL to the float32 model on 4096 normal-range rows and on every combination of 0, -0, 1, -1, +-Inf, NaN; NaN exactly where
  the model has NaN.  At the singular points the device also shows torch's conventions literally.
* SIN COS EXP LOG TANH: 32,768-point sweeps against the fp64 model; the device may reach 4 x max(1, yardstick), the yardstick
  being what torch's own float32 CPU evaluation reaches on the same sweep against the same reference (values in ulps, adjoints
  in units of 2^-24 of the sum of the absolute values of the adjoint's terms).  Every measured maximum and its yardstick go to
  test_reports/residual_ops_errors.json (not tracked); a copy of an MI355X run is profiles/residual_ops_errors.json.
  A hardware maximum above its bound is a finding to explain, not a bound to raise.
* All 17 opcodes through the compiler against torch fp64 autograd of the lambdified equations.
* Point counts around the 256-thread block, jets that are a slice of padded rows (the layout lig_jet.lig_jets returns at an odd
  point count: _ResidualHip.backward raised "unexpected jets layout" there until it allocated the adjoint with the strides of the
  jets), two JET instructions on one slot, a program at the 192-instruction limit, and a whole RB2 step at odd point counts.
* stpde_loss_grad bit-equal to g * f'(a - b) at the Huber kink, both zeros, +-Inf and NaN (the Huber gradient of a NaN difference
  was -1 until loss_grad selected its linear branch with comparisons that are false for NaN); stpde_loss_sum against the fp64 sum
  at sizes around the wave, the block and the block cap, to the bound its structure gives, in both accumulation modes.

NaN / Inf here are DATA fed to element-wise kernels: ordinary arithmetic, every index in bounds."""
import json
import os

import numpy as np
import pytest
import torch

from tests import residual_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
REPORT_DIR = "test_reports"
_report = {}


def _record(key, value):
    _report[key] = value
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "residual_ops_errors.json"), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)


def _prog_t(prog):
    return torch.from_numpy(prog.view(np.uint8).copy()).to(DEV)          # as PDELayer._residues_hip


def _n_eq(prog):
    return int((prog["op"] == M.OPS["OUT"]).sum())


def _apply(prog, jets_t, x):
    from space_time_pde_amd import pde
    x2d = None if x is None else torch.from_numpy(np.array(x, dtype=F)).to(DEV)
    return pde._ResidualHip.apply(jets_t, x2d, _prog_t(prog), len(prog), _n_eq(prog))


def _device(prog, jets, x, res_bar):
    """(res [n_eq, P], jets_bar [S, n_out, P]) of the device, as numpy float32."""
    jets_t = torch.from_numpy(np.array(jets, dtype=F)).to(DEV).requires_grad_(True)
    res = _apply(prog, jets_t, x)
    res.backward(torch.from_numpy(np.array(res_bar, dtype=F)).to(DEV))
    torch.cuda.synchronize()
    return res.detach().cpu().numpy(), jets_t.grad.cpu().numpy()


def _assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert M.same_bits(got, want).all(), "%s: %s" % (what, M.bit_mismatches(got, want))


# ---- exact opcodes ----------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
# (case, operands of the edge row, channel of the adjoint, value) with cotangent 1: torch's conventions (checked on the host for
# torch and for the model by tests/test_residual_model_host.py)
CONVENTIONS = {
    "ABS": [((0.0,), 0, 0.0), ((-0.0,), 0, 0.0), ((NAN,), 0, 0.0)],
    "POWI_2": [((0.0,), 0, 0.0)],
    "POWI_-1": [((0.0,), 0, -INF)],
    "SQRT": [((0.0,), 0, INF)],
    "DIV": [((0.0, 0.0), 1, NAN), ((1.0, 0.0), 1, -INF)],
}


@pytest.mark.parametrize("name", M.EXACT_CASES_BASE)
def test_exact_opcode_is_bit_equal_to_the_fp32_model(hiplib, name):
    """Held to bit equality, DIV and SQRT included: the hardware's fp32 divide and square root are correctly rounded here."""
    prog, jets, x, res_bar = M.exact_case(name)
    res, bar = _device(prog, jets, x, res_bar)
    want = np.stack(M.run(prog, jets, x, F))
    want_bar = M.adjoint(prog, jets, x, res_bar, F)
    _assert_bits(res, want, name + " values")
    _assert_bits(bar, want_bar, name + " adjoint")
    if name in ("X", "CONST"):
        assert not bar.view(np.int32).any(), "a program without a path from a JET to an OUT has a +0 gradient"
    if name == "OUT":
        assert np.array_equal(bar[0, 0, :4096], res_bar[0, :4096] + res_bar[1, :4096])
    for at, ch, value in CONVENTIONS.get(name, ()):
        i = M.edge_index(*at)
        got = float(bar[0, ch, i]) if name != "DIV" else None
        if name == "DIV":       # channel 1 also carries the b / b companion of the case: take a / b alone
            _, b1 = _device(prog[:4], jets, x, res_bar[:1])
            got = float(b1[0, ch, i])
        assert (np.isnan(got) and np.isnan(value)) or got == value, (name, at, got, value)


# ---- transcendental opcodes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.TRANS_CASES_BASE)
def test_transcendental_opcode_within_four_times_torchs_own_error(hiplib, name):
    prog, jets, cot, val64, adj64, unit = M.trans_reference(name)
    x = jets[0, 0]
    res, bar = _device(prog, jets, None, cot)
    y_val, y_adj = M.trans_yardstick(name)
    e_val = float(M.ulp_err(res[0], val64).max())
    e_adj = float(M.units_err(bar[0], adj64, unit).max())
    b_val, b_adj = M.trans_bound(y_val), M.trans_bound(y_adj)
    print("%s: value %.3f ulp (yardstick %.3f, bound %.3f); adjoint %.3f units (yardstick %.3f, bound %.3f)"
          % (name, e_val, y_val, b_val, e_adj, y_adj, b_adj))
    _record(name, {"value": {"device_max_ulp": e_val, "cpu_yardstick_ulp": y_val, "bound": b_val},
                   "adjoint": {"device_max_units": e_adj, "cpu_yardstick_units": y_adj, "bound": b_adj}})
    assert e_val <= b_val, (name, "value", e_val, b_val)
    assert e_adj <= b_adj, (name, "adjoint", e_adj, b_adj)
    if name == "TANH":
        zero = np.flatnonzero(x == 0)
        assert np.array_equal(np.signbit(res[0, zero]), np.signbit(x[zero])) and not res[0, zero].any()
        assert (np.abs(res[0]) <= 1).all()


# ---- all opcodes through the compiler ---------------------------------------------------------------------------------------
def test_all_opcodes_through_the_compiler_match_fp64_autograd(hiplib):
    layer = M.all_ops_layer()
    progs = layer.eqns_jet
    stream_of = M.all_ops_streams(layer)
    g = torch.Generator().manual_seed(3)
    n = 1001
    jets0 = torch.randn(len(stream_of), layer.n_out, n, generator=g)
    jets0[:, :, :7] = 0.0                      # exact zeros: |.|' = 0, and p^-2 and its adjoint are infinite on both sides
    x0 = torch.rand(1, n, 3, generator=g)
    shape = (1, n, 1)
    cot0 = {k: torch.randn(shape, generator=g) for k in progs}
    jets = jets0.to(DEV).requires_grad_(True)
    res = layer._residues_hip(x0.to(DEV), jets, progs, stream_of, shape)
    assert res is not None and list(res) == list(progs)
    prog_t, nins, uses_x = next(iter(layer._res_progs.values()))
    ops = {int(o) for o in np.frombuffer(prog_t.cpu().numpy().tobytes(), dtype=M.DT)["op"]}
    assert ops == set(range(17)) and uses_x
    sum((res[k] * cot0[k].to(DEV)).sum() for k in res).backward()
    j64 = jets0.double().requires_grad_(True)
    cols = [x0.double()[..., i:i + 1] for i in range(3)]
    ref = {name: p.fn(*(cols + [j64[stream_of[a[1]], a[0]].reshape(shape) for a in p.atoms])) for name, p in progs.items()}
    sum((ref[k] * cot0[k].double()).sum() for k in ref).backward()
    for k in res:
        assert torch.allclose(res[k].detach().cpu().double(), ref[k].detach(), rtol=2e-5, atol=2e-5), k
    assert not torch.isnan(j64.grad).any()
    assert torch.allclose(jets.grad.cpu().double(), j64.grad, rtol=2e-5, atol=2e-5)


# ---- shapes and layouts -----------------------------------------------------------------------------------------------------
_all_ops = {}


def _all_ops_case():
    """The compiled all-opcode program with seeded inputs for 1001 points (cut to the first P by the tests) and its fp64 model."""
    if not _all_ops:
        prog, uses_x, stream_of = M.all_ops_program(M.all_ops_layer())
        rng = np.random.default_rng(17)
        n_eq = _n_eq(prog)
        _all_ops.update(prog=prog, jets=rng.standard_normal((len(stream_of), 5, 1001)).astype(F),
                        x=rng.random((1001, 3)).astype(F), cot=rng.standard_normal((n_eq, 1001)).astype(F))
        for v in _all_ops.values():
            v.setflags(write=False)
    return _all_ops


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("P", [1, 5, 255, 256, 257, 1001])
def test_point_counts_and_sliced_jets(hiplib, P, pad):
    """pad = 0: dense jets against the fp64 model.  pad > 0: jets = buf[:, :, :P] of a leaf buf [S, n_out, P + pad] whose padding
    holds NaN -- values bit-equal to the dense run, buf.grad bit-equal to the dense gradient in the first P columns and exactly 0
    in the padding."""
    c = _all_ops_case()
    prog, jets, x, cot = c["prog"], c["jets"][:, :, :P], c["x"][:P], c["cot"][:, :P]
    res, bar = _device(prog, jets, x, cot)
    assert res.shape == (_n_eq(prog), P) and bar.shape == jets.shape
    if pad == 0:
        want = np.stack(M.run(prog, jets, x, np.float64))
        want_bar = M.adjoint(prog, jets, x, cot, np.float64)
        np.testing.assert_allclose(res, want, rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(bar, want_bar, rtol=2e-5, atol=2e-5)
        return
    S, n_out = jets.shape[:2]
    buf = torch.full((S, n_out, P + pad), NAN)
    buf[:, :, :P] = torch.from_numpy(np.array(jets))
    buf = buf.to(DEV).requires_grad_(True)
    view = buf[:, :, :P]
    assert view.stride() == ((P + pad) * n_out, P + pad, 1) and not view.is_contiguous()
    res2 = _apply(prog, view, x)
    res2.backward(torch.from_numpy(np.array(cot)).to(DEV))
    torch.cuda.synchronize()
    _assert_bits(res2.detach().cpu().numpy(), res, "values of the sliced jets")
    grad = buf.grad.cpu().numpy()
    _assert_bits(np.ascontiguousarray(grad[:, :, :P]), bar, "gradient of the sliced jets")
    assert not grad[:, :, P:].view(np.int32).any(), "the padding of the gradient is not +0"


def test_two_jet_instructions_on_one_slot_add_their_adjoints(hiplib):
    prog = M.program(("JET", 0, 1), ("JET", 0, 1), ("MUL", 0, 1), ("OUT", 2, 0), ("JET", 0, 0), ("JET", 0, 0), ("SUB", 4, 5),
                     ("OUT", 6, 1), ("OUT", 5, 2))
    jets = M.binary_inputs()[None, :, :4096]
    cot = M.cotangent(3 * 4096, 3).reshape(3, 4096)
    res, bar = _device(prog, jets, None, cot)
    _assert_bits(res, np.stack(M.run(prog, jets, None, F)), "values")
    _assert_bits(bar, M.adjoint(prog, jets, None, cot, F), "adjoint")
    gx = cot[0] * jets[0, 1]
    assert np.array_equal(bar[0, 1], gx + gx)            # d(x * x) through both instructions
    assert np.array_equal(bar[0, 0], (cot[2] - cot[1]) + cot[1])     # the subtrahend's register first, then the minuend's


def test_program_at_the_instruction_limit_is_bit_equal_to_the_model(hiplib):
    from space_time_pde_amd import pde
    prog, n_eq = M.chain_program(pde._RES_MAX_INS)
    assert len(prog) == 192 and not set(M.NAMES[int(o)] for o in prog["op"]) & set(M.TRANS_CASES_BASE)
    rng = np.random.default_rng(5)
    jets = rng.uniform(0.5, 2.0, (2, 1, 300)).astype(F)
    cot = rng.standard_normal((n_eq, 300)).astype(F)
    want, want_bar = np.stack(M.run(prog, jets, None, F)), M.adjoint(prog, jets, None, cot, F)
    assert np.isfinite(want).all() and np.isfinite(want_bar).all() and want_bar.any(axis=2).all()
    res, bar = _device(prog, jets, None, cot)
    _assert_bits(res, want, "values")
    _assert_bits(bar, want_bar, "adjoint")


# ---- end to end at an odd point count ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 257])
def test_rb2_step_at_an_odd_point_count_matches_the_oracle(hiplib, N):
    """lig_jets pads an odd point count and returns a slice: the backward of a PDELayer step must go through it.  The oracle is
    oracle.cpu_ref.lig_pde_step in fp64 with the l2 losses, whose gradient is that of sum(pred * cot_p) + sum(res * cot_r) with
    cot_p = alpha_reg 2 (pred - target) / numel and cot_r = alpha_pde 2 res / numel taken from the oracle's own forward; the
    tolerances are those of tests/test_gpu_lig_jet.py::test_backward_matches_oracle_autograd."""
    from oracle import cpu_ref as O
    from space_time_pde_amd import local_implicit_grid as lig, physics
    from tests.test_gpu_lig_jet import _net, _params64, _relerr
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(1, 3, 4, 5, 32, generator=g)
    pts = 0.02 + 0.96 * torch.rand(1, N, 3, generator=g)
    tgt = torch.randn(1, N, 4, generator=g)
    net = _net("softplus").to(DEV)
    kw = dict(t_crop=2., z_crop=1., x_crop=1., use_continuity=True)
    alpha_reg, alpha_pde = 4.0, 1.0
    out = O.lig_pde_step(_params64(net), "softplus", lat.double(), pts.double(), tgt.double(), O.rb2_oracle(**kw),
                         alpha_reg=alpha_reg, alpha_pde=alpha_pde, loss="l2", backward=True)
    cot_p = alpha_reg * 2.0 * (out["pred"] - tgt.double()) / out["pred"].numel()
    n_res = sum(v.numel() for v in out["residues"].values())
    cot_r = {k: alpha_pde * 2.0 * v / n_res for k, v in out["residues"].items()}
    layer = physics.get_rb2_pde_layer(**kw)
    latd = lat.to(DEV).requires_grad_(True)
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    n0 = lig.stats["hip_jet_calls"]
    pred, res = layer(pts.to(DEV), return_residue=True)
    assert lig.stats["hip_jet_calls"] == n0 + 1, "HIP jet path was not taken"
    assert list(res) == list(cot_r)
    total = (pred * cot_p.float().to(DEV)).sum() + sum((res[k] * cot_r[k].float().to(DEV)).sum() for k in res)
    total.backward()
    torch.cuda.synchronize()
    assert _relerr(pred.detach(), out["pred"]) < 2e-5
    for k, v in out["residues"].items():
        assert (res[k].detach().cpu().double() - v).abs().max().item() < 1e-4 * max(v.abs().max().item(), 1e-3), k
    assert _relerr(latd.grad, out["dlatent"]) < 2e-4
    for k in range(6):
        assert _relerr(net.fc[k].weight.grad, out["grads"][2 * k]) < 2e-4, "dW%d" % k
        assert _relerr(net.fc[k].bias.grad, out["grads"][2 * k + 1]) < 2e-4, "db%d" % k


# ---- loss kernels -----------------------------------------------------------------------------------------------------------
BIG = 2 * 2 ** 20 + 3          # past the 1024-block cap of k_loss_sum and the 2048-block cap of k_loss_grad (1024 elements each)
SUM_SIZES = (1, 63, 64, 255, 256, 257, 1024, 1025, BIG)
W = F(0.37)
_one, _two, _zero = F(1), F(2), F(0)
GRAD_EDGES = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(_one, _zero), np.nextafter(-_one, _zero), np.nextafter(_one, _two),
                       np.nextafter(-_one, -_two), 1e-30, -1e-30, np.inf, -np.inf, np.nan], dtype=F)
FINITE_EDGES = GRAD_EDGES[:10]
_loss = {}


def _loss_data():
    """a = 2 randn, b = randn [BIG], with the finite edge values of a across the block boundaries 256 and 1024."""
    if not _loss:
        rng = np.random.default_rng(23)
        a = (2.0 * rng.standard_normal(BIG)).astype(F)
        b = rng.standard_normal(BIG).astype(F)
        for at in (250, 1018):
            a[at:at + len(FINITE_EDGES)] = FINITE_EDGES
        _loss.update(a=a, b=b)
        for v in _loss.values():
            v.setflags(write=False)
    return _loss["a"], _loss["b"]


def _grad_case(with_target):
    """(a, b) [BIG]: the sweep, with every edge difference -- exactly -- across the block boundary at 256 and in the last
    elements, which the grid-stride loop reaches in its second round."""
    a, b = (np.array(v) for v in _loss_data())
    E = GRAD_EDGES
    for at in (250, BIG - len(E)):
        if with_target:                    # a - b = d / 2 - (-d / 2) = d exactly; NaN against a finite target
            a[at:at + len(E)] = E / 2
            b[at:at + len(E)] = np.where(np.isnan(E), F(0.25), -E / 2)
        else:
            a[at:at + len(E)] = E
    d = M.loss_diff(a, b if with_target else None)
    for at in (250, BIG - len(E)):
        assert M.same_bits(d[at:at + len(E)], E).all()
    return a, (b if with_target else None), d


@pytest.mark.parametrize("with_target", [True, False], ids=["target", "no_target"])
@pytest.mark.parametrize("kind", M.LOSS_KINDS)
def test_loss_grad_is_bit_equal_to_the_fp32_model(hiplib, kind, with_target):
    from space_time_pde_amd import train_step as T
    a, b, d = _grad_case(with_target)
    at = torch.from_numpy(a).to(DEV).requires_grad_(True)
    bt = None if b is None else torch.from_numpy(b).to(DEV)
    (torch.tensor(float(W), device=DEV) * T.loss_sum(at, bt, kind)).backward()
    torch.cuda.synchronize()
    got = at.grad.cpu().numpy()
    _assert_bits(got, M.loss_grad(kind, d, W), "%s gradient" % kind)
    nan = np.isnan(d)
    assert nan.sum() == 2
    if kind == "l1":
        assert not got[nan].view(np.int32).any(), "torch: sign(NaN) = 0"
    else:
        assert np.isnan(got[nan]).all(), "torch: the %s gradient of a NaN difference is NaN, got %r" % (kind, got[nan])


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
@pytest.mark.parametrize("kind", M.LOSS_KINDS)
def test_loss_sum_within_the_bound_of_its_structure(hiplib, monkeypatch, kind, det):
    """Against the fp64 sum of the terms f(a - b) -- of the terms as float32 holds them (the kernel's own element expressions,
    which the bound of the summation does not cover) and of the terms evaluated in fp64 from the same float32 inputs.  All terms
    are non-negative, so the bound is relative to the sum.  Deterministic mode: two runs are bit-identical."""
    from space_time_pde_amd import _lib, train_step as T
    monkeypatch.setattr(_lib, "deterministic", det)
    a, b = _loss_data()
    a_dev, b_dev = torch.from_numpy(np.array(a)).to(DEV), torch.from_numpy(np.array(b)).to(DEV)
    for n in SUM_SIZES:
        for with_target in (True, False):
            bn = b[:n] if with_target else None
            got_t = T.loss_sum(a_dev[:n], b_dev[:n] if with_target else None, kind)
            got = float(got_t.item())
            terms32 = M.loss_elem(kind, M.loss_diff(a[:n], bn)).astype(np.float64).sum()
            terms64 = M.loss_elem(kind, M.loss_diff(a[:n], bn, np.float64)).sum()
            bound = M.loss_sum_bound(n, det)
            print("loss_sum[%s, n=%d, target=%s, det=%s] = %r: %.3f / %.3f units of 2^-24 off (bound %.0f)"
                  % (kind, n, with_target, det, got, abs(got - terms32) / (M.U * terms32), abs(got - terms64) / (M.U * terms64),
                     bound / M.U))
            assert abs(got - terms32) <= bound * terms32, (kind, n, with_target, got, terms32)
            assert abs(got - terms64) <= bound * terms64, (kind, n, with_target, got, terms64)
            if det:
                again = T.loss_sum(a_dev[:n], b_dev[:n] if with_target else None, kind)
                assert torch.equal(again.view(torch.int32), got_t.view(torch.int32)), (kind, n, with_target)


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "det"])
@pytest.mark.parametrize("kind", M.LOSS_KINDS)
def test_loss_of_a_non_contiguous_tensor_equals_that_of_its_copy(hiplib, monkeypatch, kind, det):
    """One block (1000 elements) with fp32 atomics, where the sum has one order; four blocks in deterministic mode."""
    from space_time_pde_amd import _lib, train_step as T
    monkeypatch.setattr(_lib, "deterministic", det)
    a, b = _loss_data()
    rows = 25 if det else 8
    base = torch.from_numpy(np.array(a[:rows * 125])).reshape(125, rows).to(DEV)
    tgt = torch.from_numpy(np.array(b[:rows * 125])).reshape(rows, 125).to(DEV)
    outs = []
    for t in (base.t(), base.t().contiguous()):
        assert t.shape == (rows, 125)
        t = t.detach().requires_grad_(True)
        s = T.loss_sum(t, tgt, kind)
        (torch.tensor(float(W), device=DEV) * s).backward()
        outs.append((s.detach(), t.grad))
    assert not base.t().is_contiguous()
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    d = M.loss_diff(base.t().cpu().numpy(), tgt.cpu().numpy())
    _assert_bits(outs[0][1].cpu().numpy(), M.loss_grad(kind, d, W), "gradient")
