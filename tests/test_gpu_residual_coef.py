"""Coefficient tensors read inside the HIP residual kernels, on the device: k_residual_coef_fwd / k_residual_coef_bwd through the
C ABI against tests/residual_params_model.py, then PDELayer(device_params=True) -- residuals, training steps on a 3-d and on a 2-d
grid, a coefficient behind a leaf, an unused one -- and a captured training step whose coefficients change between replays.

Bounds.  Kernel level: residuals and jets_bar bit-equal to the float32 model (exact-opcode programs); a coefficient gradient
within residual_params_model.coef_sum_bound -- derived there from the kernel's reduction -- of the fp64 sum of the float32 model's
per-point adjoints.  Layer level: the bounds of tests/test_gpu_residual_params.py (residuals rtol = atol = 2e-5, end to end 2e-4
of each gradient's largest magnitude).  Graph: the rule of tests/test_gpu_residual_ext.py's graphed step.

NaN here is DATA fed to element-wise kernels: ordinary arithmetic, every index in bounds (residual_model.program checks the
operands of the hand-written program)."""
import copy
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from tests import residual_model as M
from tests import residual_params_model as PM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SHAPES = [(1, 1), (3, 37), (2, 64), (3, 256), (3, 257), (2, 600)]
RB2 = dict(mean=(0.01, 0.0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1., x_crop=1., use_continuity=True)


# ---- kernel level -----------------------------------------------------------------------------------------------------------------
# two residuals over jets [2 streams, 2 channels], the coordinates, a scalar coefficient c0 and one per batch element c1;
# jet (0, 0) is a factor of both coefficients, so that a NaN in it reaches both gradients
PROG = M.program(
    ("JET", 0, 0), ("JET", 0, 1), ("JET", 1, 0), ("X", 1), PM.coef_const(0), PM.coef_const(1),
    ("MUL", 4, 0), ("MUL", 5, 0), ("MUL", 7, 1), ("ADD", 6, 8), ("OUT", 9, 0),          # c0 j00 + c1 j00 j01
    ("DIV", 2, 5), ("MUL", 4, 3), ("ABS", 12), ("SQRT", 13), ("SUB", 11, 14), ("OUT", 15, 1))   # j10 / c1 - sqrt|c0 x1|
PER_BATCH = (False, True)


@functools.lru_cache(maxsize=None)
def _case(B, N, nan_at=None):
    """Inputs and the float32 model's results, built once: dict(jets [2, 2, P], x [P, 3], cot [2, P], values, res, jets_bar,
    g [2, P])."""
    rng = np.random.default_rng(100 * B + N)
    P = B * N
    jets = rng.uniform(-1, 1, (2, 2, P)).astype(F)
    if nan_at is not None:
        jets[0, 0, nan_at] = np.nan
    x = rng.uniform(0.1, 1, (P, 3)).astype(F)
    cot = rng.standard_normal((2, P)).astype(F)
    values = [np.array(0.37, dtype=F), np.linspace(0.8, 1.9, B).astype(F)]
    out = dict(jets=jets, x=x, cot=cot, values=values)
    out["res"] = np.stack(PM.run(PROG, jets, x, values, B, F))
    out["jets_bar"], out["g"] = PM.adjoint(PROG, jets, x, cot, values, B, F)
    for a in list(out.values()):
        for b in a if isinstance(a, list) else [a]:
            b.setflags(write=False)
    return out


def _jets_on_device(jets, padded):
    """dense, or the slice [:, :, :P] of a buffer with 3 more (NaN) columns per row."""
    t = torch.from_numpy(np.array(jets))
    if not padded:
        return t.to(DEV)
    buf = torch.full(t.shape[:2] + (t.shape[2] + 3,), float("nan"))
    buf[:, :, :t.shape[2]] = t
    return buf.to(DEV)[:, :, :t.shape[2]]


def _record(B, P, values, want, det, bars):
    from space_time_pde_amd import _lib
    rec = _lib.ResCoefs()
    rec.n, rec.n_per_batch, rec.det = len(values), P // B, int(det)
    for k, v in enumerate(values):
        rec.per_batch[k] = int(PER_BATCH[k])
        rec.value[k] = v.data_ptr()
        if bars is not None and want[k]:
            rec.bar[k] = bars[k].data_ptr()
    return rec


def _forward(L, prog_t, jets_t, x_t, B, values):
    from space_time_pde_amd import _lib
    S, C, P = jets_t.shape
    res = torch.full((2, P), float("nan"), device=DEV)
    rec = _record(B, P, values, None, False, None)
    _lib.check(L.stpde_residual_coef_fwd(_lib.ptr(prog_t), len(PROG), 2, C, P, _lib.ptr(jets_t), jets_t.stride(0), jets_t.stride(1),
                                         _lib.ptr(x_t), _lib.ptr(res), ctypes.byref(rec), _lib.stream_ptr()))
    return res


def _backward(L, prog_t, jets_t, x_t, cot_t, B, values, want, det):
    """(jets_bar incl. the padding columns of a padded buffer, [gradient or None per coefficient])."""
    from space_time_pde_amd import _lib
    S, C, P = jets_t.shape
    ld = jets_t.stride(1)
    jbar_buf = torch.zeros(S, C, ld, device=DEV)
    per = 2 * _lib.DET_K if det else 1
    bars = [torch.zeros((B if PER_BATCH[k] else 1) * per, device=DEV) for k in range(2)]
    rec = _record(B, P, values, want, det, bars)
    _lib.check(L.stpde_residual_coef_bwd(_lib.ptr(prog_t), len(PROG), 2, C, P, _lib.ptr(jets_t), jets_t.stride(0), jets_t.stride(1),
                                         _lib.ptr(x_t), _lib.ptr(cot_t), _lib.ptr(jbar_buf), ctypes.byref(rec), _lib.stream_ptr()))
    grads = []
    for k in range(2):
        if not want[k]:
            assert not bars[k].any()
            grads.append(None)
        elif det:
            out = torch.empty(bars[k].numel() // per, device=DEV)
            _lib.check(L.stpde_det_finalize(_lib.ptr(bars[k]), out.numel(), _lib.ptr(out), _lib.stream_ptr()))
            grads.append(out.cpu().numpy())
        else:
            grads.append(bars[k].cpu().numpy())
    return jbar_buf.cpu().numpy(), grads


def _check_grads(case, B, N, grads, want, det, tag):
    for k in range(2):
        if not want[k]:
            continue
        ref = np.atleast_1d(PM.coef_grad64(case["g"][k], B, PER_BATCH[k]))
        unit = PM.U * np.atleast_1d(PM.coef_abs64(case["g"][k], B, PER_BATCH[k]))
        bound = PM.coef_sum_bound(N, B, PER_BATCH[k], det)
        got = grads[k].astype(np.float64)
        assert got.shape == ref.shape, (tag, k)
        nan = np.isnan(ref)
        assert (np.isnan(got) == nan).all(), (tag, k, got, ref)
        err = np.abs(got - ref)[~nan] / unit[~nan]
        print(tag, "coefficient", k, "det" if det else "atomics", "error / unit", err, "bound", bound)
        assert (err <= bound).all(), (tag, k, err, bound)


@pytest.mark.parametrize("B,N", SHAPES)
def test_kernels_match_the_model_and_sum_the_coefficient_gradients_within_the_structural_bound(hiplib, B, N):
    case = _case(B, N)
    P = B * N
    prog_t = torch.from_numpy(PROG.view(np.uint8).copy()).to(DEV)
    x_t = torch.from_numpy(np.array(case["x"])).to(DEV)
    cot_t = torch.from_numpy(np.array(case["cot"])).to(DEV)
    values = [torch.from_numpy(np.array(v)).to(DEV) for v in case["values"]]
    for padded in (False, True):
        jets_t = _jets_on_device(case["jets"], padded)
        assert jets_t.stride(1) == P + (3 if padded else 0)
        res = _forward(hiplib, prog_t, jets_t, x_t, B, values).cpu().numpy()
        assert M.same_bits(res, case["res"]).all(), M.bit_mismatches(res, case["res"])
        for want in ((True, True), (False, True), (True, False)):
            det_runs = []
            for det in (False, True, True):
                jbar, grads = _backward(hiplib, prog_t, jets_t, x_t, cot_t, B, values, want, det)
                assert M.same_bits(jbar[:, :, :P], case["jets_bar"]).all(), M.bit_mismatches(jbar[:, :, :P], case["jets_bar"])
                assert not jbar[:, :, P:].any()                     # the padding columns belong to nobody
                _check_grads(case, B, N, grads, want, det, (B, N, padded, want))
                if det:
                    det_runs.append(grads)
            for a, b in zip(*det_runs):                             # deterministic mode: bit-identical from run to run
                assert (a is None and b is None) or a.tobytes() == b.tobytes()


def test_a_nan_in_one_point_reaches_its_batch_elements_gradient_and_the_scalar_one_only(hiplib):
    B, N = 3, 257
    nan_at = 1 * N + 256                                            # batch element 1, the one live lane of its second block
    case = _case(B, N, nan_at)
    assert np.isnan(case["g"][:, nan_at]).all() and np.isnan(case["g"]).sum() == 2
    prog_t = torch.from_numpy(PROG.view(np.uint8).copy()).to(DEV)
    x_t = torch.from_numpy(np.array(case["x"])).to(DEV)
    cot_t = torch.from_numpy(np.array(case["cot"])).to(DEV)
    values = [torch.from_numpy(np.array(v)).to(DEV) for v in case["values"]]
    jets_t = _jets_on_device(case["jets"], True)
    for det in (False, True):
        jbar, grads = _backward(hiplib, prog_t, jets_t, x_t, cot_t, B, values, (True, True), det)
        assert M.same_bits(jbar[:, :, :B * N], case["jets_bar"]).all()
        assert np.isnan(grads[0]).all() and np.isnan(grads[1]).tolist() == [False, True, False]
        _check_grads(case, B, N, grads, (True, True), det, "nan")   # (the other elements: finite and within the bound)


def test_values_are_read_at_run_time(hiplib):
    B, N = 2, 64
    case = _case(B, N)
    prog_t = torch.from_numpy(PROG.view(np.uint8).copy()).to(DEV)
    x_t = torch.from_numpy(np.array(case["x"])).to(DEV)
    values = [torch.from_numpy(np.array(v)).to(DEV) for v in case["values"]]
    jets_t = _jets_on_device(case["jets"], False)
    res = _forward(hiplib, prog_t, jets_t, x_t, B, values).cpu().numpy()
    assert M.same_bits(res, case["res"]).all()
    for v in values:
        v.mul_(2)
    res2 = _forward(hiplib, prog_t, jets_t, x_t, B, values).cpu().numpy()
    want2 = np.stack(PM.run(PROG, case["jets"], case["x"], [F(2) * v for v in case["values"]], B, F))
    assert M.same_bits(res2, want2).all() and not M.same_bits(res2, case["res"]).all()


def test_old_entry_points_on_a_program_without_coefficients(hiplib):
    from space_time_pde_amd import _lib
    c = M.mixed_case()
    prog, jets, x, cot = c["prog"], c["jets"], c["x"], c["cot"]
    assert not PM.late_bound(prog)
    S, C, P = jets.shape
    prog_t = torch.from_numpy(prog.view(np.uint8).copy()).to(DEV)
    jets_t, x_t, cot_t = (torch.from_numpy(np.array(a)).to(DEV) for a in (jets, x, cot))
    res = torch.empty(2, P, device=DEV)
    jbar = torch.zeros(S, C, P, device=DEV)
    args = (_lib.ptr(prog_t), len(prog), 2, C, P, _lib.ptr(jets_t), C * P, P, _lib.ptr(x_t))
    _lib.check(hiplib.stpde_residual_fwd(*args, _lib.ptr(res), _lib.stream_ptr()))
    _lib.check(hiplib.stpde_residual_bwd(*args, _lib.ptr(cot_t), _lib.ptr(jbar), _lib.stream_ptr()))
    want = np.stack(M.run(prog, jets, x, F))
    assert M.same_bits(res.cpu().numpy(), want).all()
    assert M.same_bits(jbar.cpu().numpy(), M.adjoint(prog, jets, x, cot, F)).all()


# ---- layer level ------------------------------------------------------------------------------------------------------------------
def test_rb2_residuals_with_a_rayleigh_number_per_batch_element_come_from_the_coef_kernel(hiplib):
    """tests/test_gpu_residual_params.py::test_rb2_with_a_rayleigh_number_per_batch_element with device_params=True."""
    from space_time_pde_amd import _lib, local_implicit_grid as lig, physics
    from tests.test_residual_coef_host import _compile
    B, N = 2, 257
    Ra = torch.tensor([1e6, 1e5], device=DEV)
    Pr = torch.tensor(0.7, device=DEV)
    layer = physics.get_rb2_pde_layer(prandtl=Pr, rayleigh=Ra, device_params=True, **RB2)
    plan = layer._combo_plan()
    assert plan is not None
    progs = plan["progs"]
    stream_of = {(): 0, (0,): 1, (1,): 2, (2,): 3, ("L",): 4}
    g = torch.Generator().manual_seed(6)
    jets0 = torch.randn(5, 4, B * N, generator=g)
    x0 = torch.rand(B, N, 3, generator=g)
    shape = (B, N, 1)
    req = types.SimpleNamespace(jets=jets0.to(DEV), pairs_out=["combo"])
    f0 = lig.stats.get("residual_torch_fallbacks", 0)
    with _lib.dispatch_trace() as tr:
        res = layer._residues_from_jets(x0.to(DEV), req)
    assert list(res) == list(progs) and lig.stats.get("residual_torch_fallbacks", 0) == f0
    assert tr.has("k_residual_coef_fwd"), tr.kernels
    (prog, uses_x, used), _ = _compile(layer, True)
    assert used == [0, 1]
    want = PM.run(prog, jets0.numpy(), x0.reshape(-1, 3).numpy(), [Ra.cpu().numpy(), Pr.cpu().numpy()], B, F)
    for k, name in enumerate(progs):
        got = res[name].cpu().numpy().reshape(-1)
        assert M.same_bits(got, want[k]).all(), (name, M.bit_mismatches(got, want[k]))
    j64 = jets0.double()
    cols = [x0.double()[..., i:i + 1] for i in range(3)]
    pv = [Ra.cpu().double().reshape(-1, 1, 1), Pr.cpu().double().reshape(-1, 1, 1)]
    for name, p in progs.items():
        ref = p.fn(*(cols + pv + [j64[stream_of[a[1]], a[0]].reshape(shape) for a in p.atoms]))
        assert torch.allclose(res[name].cpu().double(), ref, rtol=2e-5, atol=2e-5), name
    for b in range(B):
        const = physics.get_rb2_pde_layer(prandtl=0.7, rayleigh=float(Ra[b].item()), **RB2)
        ref = const._residues_from_jets(x0.to(DEV), req)
        for name in ref:
            assert torch.allclose(res[name][b].cpu().double(), ref[name][b].cpu().double(), rtol=2e-5, atol=2e-5), (b, name)
    assert lig.stats.get("residual_torch_fallbacks", 0) == f0


def test_training_step_gradients_of_ra_pr_network_and_latent_with_device_params(hiplib):
    """tests/test_gpu_residual_params.py::test_training_step_gradients_of_ra_pr_network_and_latent_match_the_fp64_oracle --
    its shape, its fp64 oracle, its 2e-4 -- with device_params=True."""
    from oracle import jet_ref as J
    from space_time_pde_amd import _lib, local_implicit_grid as lig, physics
    from tests.test_gpu_lig_jet import _net, _params64, _relerr
    g = torch.Generator().manual_seed(5)
    B, N = 2, 200
    lat = 0.5 * torch.randn(B, 4, 5, 6, 32, generator=g)
    pts = 0.02 + 0.96 * torch.rand(B, N, 3, generator=g)
    tgt = torch.randn(B, N, 4, generator=g)
    net = _net("softplus").to(DEV)
    Ra = torch.tensor([2e3, 8e3], device=DEV, requires_grad=True)
    Pr = torch.tensor(0.7, device=DEV, requires_grad=True)
    layer = physics.get_rb2_pde_layer(prandtl=Pr, rayleigh=Ra, t_crop=2., z_crop=1., x_crop=1., use_continuity=True,
                                      device_params=True)
    plan = layer._combo_plan()
    assert plan is not None
    alpha_reg, alpha_pde = 4.0, 1.0

    def loss_of(pred, res, target):
        r = torch.stack([res[k] for k in res])
        return alpha_reg * ((pred - target) ** 2).mean() + alpha_pde * (r ** 2).mean()

    latd = lat.to(DEV).requires_grad_(True)
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    n0, f0 = lig.stats["hip_jet_calls"], lig.stats.get("residual_torch_fallbacks", 0)
    with _lib.dispatch_trace() as tr:
        pred, res = layer(pts.to(DEV), return_residue=True)
        loss = loss_of(pred, res, tgt.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    assert lig.stats["hip_jet_calls"] == n0 + 1, "HIP jet path was not taken"
    assert lig.stats.get("residual_torch_fallbacks", 0) == f0
    assert tr.has("k_residual_coef_fwd") and tr.has("k_residual_coef_bwd"), tr.kernels

    p64 = [(w.requires_grad_(True), b.requires_grad_(True)) for w, b in _params64(net)]
    lat64 = lat.double().requires_grad_(True)
    Ra64 = Ra.detach().cpu().double().requires_grad_(True)
    Pr64 = Pr.detach().cpu().double().requires_grad_(True)
    pairs = tuple(sorted(plan["alpha"]))
    full = J.lig_jets(p64, "softplus", lat64, pts.double(), 0., 1., second=pairs, beta=torch.tensor(1.3, dtype=torch.float64))
    full = full.permute(0, 3, 1, 2).reshape(full.shape[0], 4, -1)
    Lc = sum(plan["alpha"][p] * full[4 + k] for k, p in enumerate(pairs))
    ref = torch.cat([full[:4], Lc[None]], 0)
    stream_of = {(): 0, (0,): 1, (1,): 2, (2,): 3, ("L",): 4}
    shape = (B, N, 1)
    cols = [pts.double()[..., i:i + 1] for i in range(3)]
    pv = [Ra64.reshape(-1, 1, 1), Pr64.reshape(-1, 1, 1)]
    res64 = {name: p.fn(*(cols + pv + [ref[stream_of[a[1]], a[0]].reshape(shape) for a in p.atoms]))
             for name, p in plan["progs"].items()}
    pred64 = ref[0].t().reshape(B, N, 4)
    loss64 = loss_of(pred64, res64, tgt.double())
    loss64.backward()
    assert list(res) == list(res64)
    assert abs(loss.item() - loss64.item()) < 1e-5 * abs(loss64.item())
    assert Ra.grad.shape == (2,) and Pr.grad.shape == () and Ra64.grad.abs().min() > 0
    print("dRa", Ra.grad.cpu().numpy(), Ra64.grad.numpy(), "dPr", Pr.grad.item(), Pr64.grad.item())
    assert _relerr(Ra.grad, Ra64.grad) < 2e-4
    assert _relerr(Pr.grad, Pr64.grad) < 2e-4
    assert _relerr(latd.grad, lat64.grad) < 2e-4
    for k in range(6):
        assert _relerr(net.fc[k].weight.grad, p64[k][0].grad) < 2e-4, "dW%d" % k
        assert _relerr(net.fc[k].bias.grad, p64[k][1].grad) < 2e-4, "db%d" % k


@pytest.fixture
def nd_train(hiplib):
    from space_time_pde_amd import lig_jet
    prev = lig_jet.set_nd_jets(True), lig_jet.set_nd_jet_backward(True)
    yield lig_jet
    lig_jet.set_nd_jets(prev[0])
    lig_jet.set_nd_jet_backward(prev[1])


@pytest.mark.parametrize("non_leaf", [False, True], ids=["leaf", "exp_of_a_leaf"])
def test_burgers_on_a_2d_grid_with_a_learnable_viscosity_and_device_params(nd_train, non_leaf):
    """tests/test_gpu_residual_params.py::test_burgers_on_a_2d_grid_with_a_learnable_viscosity with device_params=True; then with
    nu = exp(log_nu), the gradient of log_nu.  fp64: the reverse-sweep strategy of the same layer on the CPU."""
    from space_time_pde_amd import _lib, local_implicit_grid as lig, pde
    from tests import lig_nd_jet_bwd_model as BM
    TOL = 2e-4
    lat, pts, mask = BM.make_case(2, (4, 5), 8)
    net0 = BM.make_net(2, 8, "softplus", 1)
    tgt = torch.randn(2, 37, 1, generator=torch.Generator().manual_seed(3))
    layer = pde.PDELayer("t, x", "u", "nu", device_params=True)
    layer.add_equation("dif(u,t)+u*dif(u,x)-nu*dif(dif(u,x),x)", "burgers")

    def loss_of(y, res, target, m):
        return (((y - target) ** 2) * m.unsqueeze(-1)).sum() + ((res["burgers"][..., 0] * m) ** 2).sum()

    def coefficient(leaf):
        return leaf.exp() if non_leaf else leaf

    start = [0.01, 0.03]
    net64 = copy.deepcopy(net0).double()
    lat64 = lat.double().requires_grad_(True)
    leaf64 = torch.tensor(start, dtype=torch.float64)
    leaf64 = (leaf64.log() if non_leaf else leaf64).requires_grad_(True)
    layer.params = {"nu": coefficient(leaf64)}   # (update_parameters takes fp32 only: the oracle's values are set directly)
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net64, lat64, q, 0., 1.))
    y64, res64 = layer(pts.double(), return_residue=True)
    loss64 = loss_of(y64, res64, tgt.double(), mask.double())
    gref = torch.autograd.grad(loss64, [lat64, leaf64] + [t for k in range(6) for t in (net64.fc[k].weight, net64.fc[k].bias)])

    net = copy.deepcopy(net0).to(DEV)
    latd = lat.to(DEV).requires_grad_(True)
    leaf = leaf64.detach().float().to(DEV).requires_grad_(True)
    layer.update_parameters({"nu": coefficient(leaf)})
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    h0, g0, f0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"], lig.stats.get("residual_torch_fallbacks", 0)
    with _lib.dispatch_trace() as tr:
        y, res = layer(pts.to(DEV), return_residue=True)
        loss = loss_of(y, res, tgt.to(DEV), mask.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0
    assert lig.stats.get("residual_torch_fallbacks", 0) == f0
    assert tr.has("k_reduce_nd_jet_bwd<", "D = 2"), tr.kernels
    assert tr.has("k_residual_coef_fwd") and tr.has("k_residual_coef_bwd"), tr.kernels

    def rel(got, want):
        return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()

    grads = [t.grad for k in range(6) for t in (net.fc[k].weight, net.fc[k].bias)]
    err = {"loss": abs(loss.item() - loss64.item()) / abs(loss64.item()), "dlatent": rel(latd.grad, gref[0]),
           "dleaf": rel(leaf.grad, gref[1]), "dW": max(rel(a, b) for a, b in zip(grads, gref[2:]))}
    print("burgers 2-d, device_params, non_leaf =", non_leaf, err, leaf.grad.cpu().numpy(), gref[1].numpy())
    assert leaf.grad.shape == (2,) and gref[1].abs().min() > 0
    assert all(v < TOL for v in err.values()), err


def test_a_declared_coefficient_no_equation_uses_gets_no_gradient(hiplib):
    from space_time_pde_amd import _lib, local_implicit_grid as lig, pde
    B, N = 2, 37
    layer = pde.PDELayer("t, x", "u", "nu, mu", device_params=True)
    layer.add_equation("dif(u,t)+u*dif(u,x)-nu*dif(dif(u,x),x)", "burgers")
    nu = torch.tensor([0.01, 0.03], device=DEV, requires_grad=True)
    mu = torch.tensor(2.0, device=DEV, requires_grad=True)
    layer.update_parameters({"nu": nu, "mu": mu})
    g = torch.Generator().manual_seed(8)
    jets = torch.randn(5, 1, B * N, generator=g).to(DEV).requires_grad_(True)
    x = torch.rand(B, N, 2, generator=g).to(DEV)
    req = types.SimpleNamespace(jets=jets, pairs_out=[(1, 1)])
    f0 = lig.stats.get("residual_torch_fallbacks", 0)
    with _lib.dispatch_trace() as tr:
        res = layer._residues_from_jets(x, req)
        (res["burgers"] ** 2).sum().backward()
    assert lig.stats.get("residual_torch_fallbacks", 0) == f0 and tr.has("k_residual_coef_bwd"), tr.kernels
    assert mu.grad is None and nu.grad is not None and nu.grad.shape == (2,) and jets.grad is not None
    # d/d nu of sum r^2 = sum 2 r (-u_xx), per batch element
    terms = 2 * res["burgers"].detach().double().reshape(B, N) * -jets.detach().double()[4, 0].reshape(B, N)
    want, scale = terms.sum(1), terms.abs().sum(1)                  # (fp32 sums of N terms: a few 2^-24 of sum |term|)
    assert ((nu.grad.double() - want).abs() <= 2e-5 * scale).all(), (nu.grad, want)
    # a non-contiguous [B] view of a leaf is made contiguous per call; the gradient reaches the leaf through the view
    base = torch.tensor([0.01, 7.0, 0.03, 7.0], device=DEV, requires_grad=True)
    layer.update_parameters({"nu": base[::2]})
    assert not layer.params["nu"].is_contiguous()
    res2 = layer._residues_from_jets(x, req)
    assert torch.equal(res2["burgers"], res["burgers"]) and lig.stats.get("residual_torch_fallbacks", 0) == f0
    (res2["burgers"] ** 2).sum().backward()
    assert torch.equal(base.grad[::2], nu.grad) and not base.grad[1::2].any()


def test_layer_backward_in_deterministic_mode_uses_the_long_accumulators(hiplib, monkeypatch):
    """RB2, B x N = 3 x 600 (three blocks per batch element), Ra [B] and Pr []: with ``_lib.deterministic`` the coefficient
    gradients of two backward passes are bit-identical, keep the tensors' shapes and are the default mode's to the bound of the
    two sums (8 + blocks and 8 + 1 units of 2^-24 * sum |g_p|: residual_params_model.coef_sum_bound)."""
    from space_time_pde_amd import _lib, physics
    from tests.test_residual_coef_host import _compile
    B, N = 3, 600
    Ra = torch.tensor([1e4, 3e4, 1e5], device=DEV, requires_grad=True)
    Pr = torch.tensor(0.7, device=DEV, requires_grad=True)
    layer = physics.get_rb2_pde_layer(prandtl=Pr, rayleigh=Ra, device_params=True, **RB2)
    g = torch.Generator().manual_seed(9)
    jets0 = torch.randn(5, 4, B * N, generator=g)
    x = torch.rand(B, N, 3, generator=g).to(DEV)
    cot = torch.randn(4, B * N, generator=g)
    # the float32 model's per-point adjoints give the unit of the bound
    (prog, _, used), _ = _compile(layer, True)
    vals = [Ra.detach().cpu().numpy(), Pr.detach().cpu().numpy()]
    _, gco = PM.adjoint(prog, jets0.numpy(), None, cot.numpy(), vals, B, F)
    per_batch = (True, False)

    def grads(det):
        monkeypatch.setattr(_lib, "deterministic", det)
        Ra.grad = Pr.grad = None
        jets = jets0.to(DEV).requires_grad_(True)
        with _lib.dispatch_trace() as tr:
            res = layer._residues_from_jets(x, types.SimpleNamespace(jets=jets, pairs_out=["combo"]))
            torch.stack([res[k].reshape(-1) for k in res]).backward(cot.to(DEV))
        assert tr.has("k_residual_coef_bwd"), tr.kernels
        assert Ra.grad.shape == (B,) and Pr.grad.shape == ()
        return [Ra.grad.cpu().numpy().copy(), Pr.grad.cpu().numpy().copy()], jets.grad.cpu().numpy()

    (d1, j1), (d2, j2), (n1, j3) = grads(True), grads(True), grads(False)
    assert M.same_bits(j1, j2).all() and M.same_bits(j1, j3).all()
    for k in range(2):
        assert d1[k].tobytes() == d2[k].tobytes(), k
        ref = np.atleast_1d(PM.coef_grad64(gco[k], B, per_batch[k]))
        unit = PM.U * np.atleast_1d(PM.coef_abs64(gco[k], B, per_batch[k]))
        for got, det in ((d1[k], True), (n1[k], False)):
            err = np.abs(np.atleast_1d(got).astype(np.float64) - ref) / unit
            print("layer, coefficient", k, "det" if det else "atomics", err, PM.coef_sum_bound(N, B, per_batch[k], det))
            assert (err <= PM.coef_sum_bound(N, B, per_batch[k], det)).all(), (k, det, err)


# ---- a captured step ------------------------------------------------------------------------------------------------------------------
def test_graphed_step_with_learnable_ra_and_pr_replays_the_eager_step_and_sees_in_place_updates(hiplib):
    """The fixture and the rule of tests/test_gpu_residual_ext.py::test_graphed_step_on_a_layer_with_the_appended_opcodes_replays_
    the_eager_step with RB2 on a Rayleigh number per crop and a Prandtl number, both learnable: one replay on new inputs equals the
    eager step, their gradients included (2e-4 of the largest magnitude, as for the IM-NET's); after Ra is halved in place the next
    replay equals the eager step at the new value."""
    from space_time_pde_amd import implicit_net, local_implicit_grid as lig, physics, unet3d
    from space_time_pde_amd.train_step import GraphedStep, sharded_step
    dev = torch.device(DEV)
    torch.manual_seed(11)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=(4, 16, 16), nf=16, mf=256).to(dev).train()
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)
    B, N = 10, 512
    Ra = torch.logspace(4, 6, B).to(dev).requires_grad_(True)
    Pr = torch.tensor(0.7, device=dev, requires_grad=True)
    layer = physics.get_rb2_pde_layer(rayleigh=Ra, prandtl=Pr, device_params=True, **RB2)
    g = torch.Generator().manual_seed(12)

    def draw():
        return (torch.randn(B, 4, 4, 16, 16, generator=g).to(dev), (0.02 + 0.96 * torch.rand(B, N, 3, generator=g)).to(dev),
                torch.randn(B, N, 4, generator=g).to(dev))

    params = list(unet.parameters()) + list(net.parameters()) + [Ra, Pr]
    nu, nc = len(list(unet.parameters())), len(params) - 2

    def eager(crop, pts, tgt):
        for p in params:
            p.grad = None
        loss, reg, pde_ = sharded_step(unet, net, layer, crop, pts, tgt, N, 1.0, 0.0125, "l1", distributed=False)
        torch.cuda.synchronize()
        return [float(loss), float(reg), float(pde_)], [p.grad.clone() for p in params]

    def compare(got, ggrads, want, wgrads):
        for x, y in zip(got, want):
            assert abs(x - y) <= 1e-5 * abs(y), (got, want)
        for k, (x, y) in enumerate(zip(ggrads, wgrads)):
            if k < nu:
                assert (x - y).norm().item() <= 1e-1 * y.norm().item() + 1e-5 * max(v.norm().item() for v in wgrads[:nu]), k
            elif k < nc:
                assert (x - y).abs().max().item() <= 2e-4 * y.abs().max().item() + 1e-10, k
            else:       # Ra, Pr: no absolute term -- d loss / d Ra is of the order of 1e-10 itself
                assert (x - y).abs().max().item() <= 2e-4 * y.abs().max().item(), (k, x, y)

    a = draw()
    eager(*a)
    n0, f0 = lig.stats["hip_jet_calls"], lig.stats.get("residual_torch_fallbacks", 0)
    gstep = GraphedStep(unet, net, layer, *a, N, 1.0, 0.0125, "l1")
    assert lig.stats["hip_jet_calls"] > n0 and lig.stats.get("residual_torch_fallbacks", 0) == f0
    assert [p.data_ptr() for p in gstep.params] == [p.data_ptr() for p in params]
    grads = list(gstep.grads)
    assert grads[-2].shape == (B,) and grads[-1].shape == () and Ra.grad is grads[-2] and Pr.grad is grads[-1]

    inputs = draw()
    out = gstep(*inputs)
    torch.cuda.synchronize()
    got, ggrads = [float(v) for v in out], [gr.clone() for gr in grads]
    want, wgrads = eager(*inputs)
    assert wgrads[-2].abs().min().item() > 0 and wgrads[-1].abs().item() > 0
    compare(got, ggrads, want, wgrads)
    assert gstep.replays == 1

    Ra.data.mul_(0.5)                                               # in place: the graph holds the tensor's address, not its values
    out = gstep(*inputs)
    torch.cuda.synchronize()
    got2, ggrads2 = [float(v) for v in out], [gr.clone() for gr in grads]
    want2, wgrads2 = eager(*inputs)
    # (the step does depend on Ra: d loss / d Ra goes with Ra^-3/2)
    assert (wgrads2[-2] - wgrads[-2]).abs().max().item() > 1e-2 * wgrads[-2].abs().max().item()
    compare(got2, ggrads2, want2, wgrads2)
    assert gstep.replays == 2
