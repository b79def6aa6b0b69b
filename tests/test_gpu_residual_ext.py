"""The opcodes appended to the residual evaluator (TAN SINH COSH ASIN ACOS ATAN ATAN2 POWC POW MIN MAX SIGN STEP) on the device,
against tests/residual_model.py (whose adjoint rules tests/test_residual_ext_host.py checks against torch's autograd), the way
tests/test_gpu_residual_ops.py holds the first 17: hand-assembled programs through pde._ResidualHip.apply.

* MIN MAX SIGN STEP (comparisons and selects) and POWC with c = 1: values and adjoints BIT-EQUAL to the float32 model on 4096
  normal-range rows and on every combination of 0, -0, 1, -1, +-Inf, NaN.
* The opcodes that go through the math library: 32,768-point sweeps against the fp64 model; the device may reach
  4 x max(1, yardstick), the yardstick being what torch's own float32 CPU evaluation and autograd reach on the same sweep (values
  in ulps, adjoints in units of 2^-24 of the sum of the absolute values of the adjoint's terms).  Every maximum and yardstick goes
  to test_reports/residual_ext_errors.json (not tracked); profiles/residual_ext_errors.json is a copy of an MI355X run.  A maximum
  above its bound is a finding to explain, not a bound to raise.  (sinh / cosh: torch's vectorised float32 kernels return Inf above
  log(FLT_MAX) = 88.72, so the sweep with a yardstick of its own ends there and SINH_TOP / COSH_TOP, the stretch up to sinh's own
  overflow at 89.41, are judged with that yardstick.  The math library's powf(x, 1) is not x in every bit, which is why POWC takes
  the integer part of its exponent by multiplications.)
* Point counts around the 256-thread block with jets that are a slice of padded rows.
* End to end: an upwinded system with a power-law advection speed through query_local_implicit_grid and PDELayer, residuals and
  every gradient against the fp64 CPU evaluation of the same layer (reverse-sweep strategy), with the tolerances of the
  user-string tests (G9 / configs[4]), and no torch fallback of the residual algebra; a GraphedStep on such a layer.

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
    with open(os.path.join(REPORT_DIR, "residual_ext_errors.json"), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)


def _n_eq(prog):
    return int((prog["op"] == M.OPS["OUT"]).sum())


def _apply(prog, jets_t, x=None):
    from space_time_pde_amd import pde
    prog_t = torch.from_numpy(prog.view(np.uint8).copy()).to(DEV)          # as PDELayer._residues_hip
    x2d = None if x is None else torch.from_numpy(np.array(x, dtype=F)).to(DEV)
    return pde._ResidualHip.apply(jets_t, x2d, prog_t, len(prog), _n_eq(prog))


def _device(prog, jets, res_bar, x=None):
    jets_t = torch.from_numpy(np.array(jets, dtype=F)).to(DEV).requires_grad_(True)
    res = _apply(prog, jets_t, x)
    res.backward(torch.from_numpy(np.array(res_bar, dtype=F)).to(DEV))
    torch.cuda.synchronize()
    return res.detach().cpu().numpy(), jets_t.grad.cpu().numpy()


def _assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert M.same_bits(got, want).all(), "%s: %s" % (what, M.bit_mismatches(got, want))


# ---- exact opcodes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.EXACT_CASES_EXT)
def test_exact_opcode_is_bit_equal_to_the_fp32_model(hiplib, name):
    prog, jets, _, res_bar = M.exact_case(name)
    res, bar = _device(prog, jets, res_bar)
    _assert_bits(res, np.stack(M.run(prog, jets, None, F)), name + " values")
    _assert_bits(bar, M.adjoint(prog, jets, None, res_bar, F), name + " adjoint")
    if name == "POWC_1":            # x^1 = x and d/dx = 1 x^0 = 1, at 0, -0, the infinities and NaN too
        _assert_bits(res[0], jets[0, 0], "x^1")
        _assert_bits(bar[0, 0], res_bar[0], "d x^1")


# ---- opcodes of the math library ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.TRANS_CASES_EXT)
def test_math_library_opcode_within_four_times_torchs_own_error(hiplib, name):
    prog, jets, cot, _, _, _ = M.trans_reference(name)
    res, bar = _device(prog, jets, cot)
    e_val, e_adj = M.trans_errors(name, res[0], bar[0])
    y_val, y_adj = M.trans_yardstick(name)
    b_val, b_adj = M.trans_bound(y_val), M.trans_bound(y_adj)
    label = name if not name.startswith("POWC_") else "POWC_%.6g" % M.POWC_EXPONENTS[int(name[5:])]
    print("%s: value %.3f ulp (yardstick %.3f, bound %.3f); adjoint %.3f units (yardstick %.3f, bound %.3f)"
          % (label, e_val, y_val, b_val, e_adj, y_adj, b_adj))
    _record(label, {"value": {"device_max_ulp": e_val, "cpu_yardstick_ulp": y_val, "bound": b_val},
                    "adjoint": {"device_max_units": e_adj, "cpu_yardstick_units": y_adj, "bound": b_adj}})
    assert e_val <= b_val, (label, "value", e_val, b_val)
    assert e_adj <= b_adj, (label, "adjoint", e_adj, b_adj)


# ---- shapes and layouts ---------------------------------------------------------------------------------------------------------
_mixed = {}


def _mixed_case():
    """One program with every appended opcode, seeded inputs for 1000 points: channel 0 in (-0.95, 0.95), channel 1 in (0.5, 2)."""
    if not _mixed:
        ins = [("JET", 0, 0), ("JET", 0, 1), ("X", 1)]
        outs = []
        for k, op in enumerate([("TAN", 0), ("SINH", 0), ("COSH", 0), ("ASIN", 0), ("ACOS", 0), ("ATAN", 0), ("ATAN2", 0, 1),
                                ("POWC", 1, 0, 1.5), ("POW", 1, 0), ("MIN", 0, 2), ("MAX", 0, 2), ("SIGN", 0), ("STEP", 0)]):
            ins.append(op)
            outs.append(len(ins) - 1)
        # two residuals that use all of them: a sum of the smooth ones, and the selectors as factors
        acc = outs[0]
        for o in outs[1:9]:
            ins.append(("ADD", acc, o))
            acc = len(ins) - 1
        ins.append(("OUT", acc, 0))
        ins.append(("MUL", outs[9], outs[11]))
        ins.append(("MUL", outs[10], outs[12]))
        ins.append(("SUB", len(ins) - 2, len(ins) - 1))
        ins.append(("OUT", len(ins) - 1, 1))
        rng = np.random.default_rng(19)
        jets = np.stack([rng.uniform(-0.95, 0.95, 1000), rng.uniform(0.5, 2.0, 1000)])[None].astype(F)
        jets[0, 0, :3] = 0.0                           # exact zeros: sign 0, H 1/2, and ties of MIN / MAX with x below
        x = rng.uniform(-1, 1, (1000, 3)).astype(F)
        x[:3, 1] = 0.0
        _mixed.update(prog=M.program(*ins), jets=jets, x=x, cot=rng.standard_normal((2, 1000)).astype(F))
        assert set(_mixed["prog"]["op"].tolist()) >= set(M.OPS_EXT.values())
        for v in _mixed.values():
            v.setflags(write=False)
    return _mixed


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_point_counts_and_sliced_jets(hiplib, P, pad):
    """pad = 0: dense jets against the fp64 model (the tolerance of tests/test_gpu_residual_ops.py).  pad = 3: jets = buf[:, :, :P]
    of a leaf buf whose padding holds NaN -- values and gradient bit-equal to the dense run, the padding's gradient exactly 0."""
    c = _mixed_case()
    prog, jets, x, cot = c["prog"], c["jets"][:, :, :P], c["x"][:P], c["cot"][:, :P]
    res, bar = _device(prog, jets, cot, x)
    assert res.shape == (2, P) and bar.shape == jets.shape
    if pad == 0:
        np.testing.assert_allclose(res, np.stack(M.run(prog, jets, x, np.float64)), rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(bar, M.adjoint(prog, jets, x, cot, np.float64), rtol=2e-5, atol=2e-5)
        return
    buf = torch.full((1, 2, P + pad), float("nan"))
    buf[:, :, :P] = torch.from_numpy(np.array(jets))
    buf = buf.to(DEV).requires_grad_(True)
    view = buf[:, :, :P]
    assert view.stride() == ((P + pad) * 2, P + pad, 1)
    res2 = _apply(prog, view, x)
    res2.backward(torch.from_numpy(np.array(cot)).to(DEV))
    torch.cuda.synchronize()
    _assert_bits(res2.detach().cpu().numpy(), res, "values of the sliced jets")
    grad = buf.grad.cpu().numpy()
    _assert_bits(np.ascontiguousarray(grad[:, :, :P]), bar, "gradient of the sliced jets")
    assert not grad[:, :, P:].view(np.int32).any(), "the padding of the gradient is not +0"


# ---- end to end -----------------------------------------------------------------------------------------------------------------
UPWIND = {
    "upwind_u": "dif(u,t) + Max(u,0)*dif(u,x) + Min(u,0)*dif(u,z) - 0.01*dif(dif(u,x),x)",
    "power_w": "dif(w,t) + sqrt(u**2+w**2+0.001)**1.5*dif(w,x)",
}


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
def test_upwinded_power_law_system_matches_the_fp64_cpu_evaluation(hiplib, prec, monkeypatch):
    """Latent [2, 4, 4, 4, 8], ImNet(nf = 16), 257 points per element.  The reference is the same PDELayer on the CPU in fp64,
    reverse-sweep strategy, over the oracle's local-implicit-grid query; tolerances: residuals 3e-5 of their maximum (G9),
    the functional 2e-4 and every gradient 3e-4 of its maximum (the configs[4] backward test)."""
    from oracle import cpu_ref as O
    from space_time_pde_amd import _lib, implicit_net, lig_jet, local_implicit_grid as lig, pde
    monkeypatch.setattr(lig_jet, "mlp_precision", prec)
    g = torch.Generator().manual_seed(21)
    lat0 = 0.5 * torch.randn(2, 4, 4, 4, 8, generator=g)
    pts = 0.02 + 0.96 * torch.rand(2, 257, 3, generator=g)
    cot_y = torch.randn(2, 257, 2, generator=g)
    cot_r = {k: torch.randn(2, 257, 1, generator=g) for k in UPWIND}
    torch.manual_seed(5)
    net = implicit_net.ImNet(dim=3, in_features=8, out_features=2, nf=16, activation=torch.nn.Softplus).to(DEV)

    def make():
        layer = pde.PDELayer("t, z, x", "u, w")
        for k, e in UPWIND.items():
            layer.add_equation(e, k)
        return layer

    layer = make()
    lat = lat0.to(DEV).requires_grad_(True)
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, lat, q, 0., 1.))
    n0, f0 = lig.stats["hip_jet_calls"], lig.stats.get("residual_torch_fallbacks", 0)
    with _lib.dispatch_trace() as tr:
        pred, res = layer(pts.to(DEV))
        f = (pred * cot_y.to(DEV)).sum() + sum((res[k] * cot_r[k].to(DEV)).sum() for k in cot_r)
        f.backward()
        torch.cuda.synchronize()
    assert lig.stats["hip_jet_calls"] == n0 + 1, "HIP jet path was not taken"
    assert lig.stats.get("residual_torch_fallbacks", 0) == f0
    assert tr.has("k_residual_fwd") and tr.has("k_residual_bwd"), "\n".join(tr.kernels)
    prog_t, nins, _ = next(iter(layer._res_progs.values()))
    ops = set(np.frombuffer(prog_t.cpu().numpy().tobytes(), dtype=M.DT)["op"].tolist())
    assert {M.OPS["MAX"], M.OPS["MIN"], M.OPS["POWC"]} <= ops
    # fp64 on the CPU: the reverse-sweep strategy of the same layer class over the oracle's query
    p64 = [(net.fc[k].weight.detach().cpu().double().requires_grad_(True),
            net.fc[k].bias.detach().cpu().double().requires_grad_(True)) for k in range(6)]
    lat64 = lat0.double().requires_grad_(True)
    act = O.activation_fn("softplus")
    ref_layer = make()
    ref_layer.update_forward_method(lambda q: O.query_lig(lambda x: O.imnet_forward(p64, x, act), lat64, q, 0., 1.))
    y64, r64 = ref_layer(pts.double().clone())
    f64 = (y64 * cot_y.double()).sum() + sum((r64[k] * cot_r[k].double()).sum() for k in cot_r)
    f64.backward()
    for k in UPWIND:
        err = (res[k].detach().cpu().double() - r64[k].detach()).abs().max().item()
        print("%s %s: residual max err %.3e of max %.3e" % (prec, k, err, r64[k].abs().max().item()))
        assert err < 3e-5 * r64[k].abs().max().item(), k
    assert abs(f.item() - f64.item()) < 2e-4 * abs(f64.item())
    assert _relerr(lat.grad, lat64.grad) < 3e-4
    for k in range(6):
        assert _relerr(net.fc[k].weight.grad, p64[k][0].grad) < 3e-4, "dW%d" % k
        assert _relerr(net.fc[k].bias.grad, p64[k][1].grad) < 3e-4, "db%d" % k


def test_graphed_step_on_a_layer_with_the_appended_opcodes_replays_the_eager_step(hiplib):
    """The fixture and the rule of tests/test_gpu_train_loop.py::test_graphed_step_replays_the_eager_step with an upwinded
    momentum equation in the layer: one replay on new inputs equals the eager step."""
    from space_time_pde_amd import implicit_net, local_implicit_grid as lig, pde, unet3d
    from space_time_pde_amd.train_step import GraphedStep, sharded_step
    dev = torch.device(DEV)
    torch.manual_seed(11)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=(4, 16, 16), nf=16, mf=256).to(dev).train()
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)
    layer = pde.PDELayer("t, z, x", "p, b, u, w")
    layer.add_equation("dif(u,x) + dif(w,z)", "continuity")
    layer.add_equation("dif(u,t) + Max(u,0)*dif(u,x) + Min(w,0)*dif(u,z) + dif(p,x) - 0.01*(dif(dif(u,x),x)+dif(dif(u,z),z))", "upwind_u")
    layer.add_equation("dif(b,t) + sqrt(u**2+w**2+0.001)**1.5*dif(b,x) + sign(w)*Abs(b)**(4/3)", "power_b")
    g = torch.Generator().manual_seed(12)
    B, N = 10, 512

    def draw():
        return (torch.randn(B, 4, 4, 16, 16, generator=g).to(dev), (0.02 + 0.96 * torch.rand(B, N, 3, generator=g)).to(dev),
                torch.randn(B, N, 4, generator=g).to(dev))

    params = list(unet.parameters()) + list(net.parameters())

    def eager(crop, pts, tgt):
        for p in params:
            p.grad = None
        loss, reg, pde_ = sharded_step(unet, net, layer, crop, pts, tgt, N, 1.0, 0.0125, "l1", distributed=False)
        torch.cuda.synchronize()
        return [float(loss), float(reg), float(pde_)], [p.grad.clone() for p in params]

    a = draw()
    eager(*a)
    n0, f0 = lig.stats["hip_jet_calls"], lig.stats.get("residual_torch_fallbacks", 0)
    gstep = GraphedStep(unet, net, layer, *a, N, 1.0, 0.0125, "l1")
    assert lig.stats["hip_jet_calls"] > n0 and lig.stats.get("residual_torch_fallbacks", 0) == f0
    grads = [p.grad for p in params]
    nu = len(list(unet.parameters()))
    inputs = draw()
    out = gstep(*inputs)
    torch.cuda.synchronize()
    got = [float(v) for v in out]
    ggrads = [gr.clone() for gr in grads]
    want, wgrads = eager(*inputs)
    for x, y in zip(got, want):
        assert abs(x - y) <= 1e-5 * abs(y), (got, want)
    for k, (x, y) in enumerate(zip(ggrads, wgrads)):
        if k < nu:
            assert (x - y).norm().item() <= 1e-1 * y.norm().item() + 1e-5 * max(v.norm().item() for v in wgrads[:nu]), k
        else:
            assert (x - y).abs().max().item() <= 2e-4 * y.abs().max().item() + 1e-10, k
    assert gstep.replays == 1
