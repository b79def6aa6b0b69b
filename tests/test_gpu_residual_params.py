"""Equation coefficients as tensors (PDELayer(param_vars=...), update_parameters) on the GPU: the jets come from the HIP
local-implicit-grid path, the residual algebra of such a layer from the lambdified torch functions (the device evaluator reads
constants only; counted as ``residual_torch_fallbacks``).  RB2 with a Rayleigh number per batch element against the fp64
evaluation and against constant-coefficient layers on the device evaluator, then training steps on a 3-d and on a 2-d grid.

Bounds.  Residuals: rtol = atol = 2e-5 (tests/test_gpu_residual_ops.py's compiler test).  End to end: 2e-4 of each gradient's
largest magnitude (tests/test_gpu_lig_jet.py, tests/test_gpu_lig_nd_jet_backward.py)."""
import copy
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- RB2 with a Rayleigh number per batch element ------------------------------------------------------------------------------
RB2 = dict(mean=(0.01, 0.0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1., x_crop=1., use_continuity=True)


def test_rb2_with_a_rayleigh_number_per_batch_element(hiplib):
    from space_time_pde_amd import local_implicit_grid as lig, physics
    B, N = 2, 257
    Ra = torch.tensor([1e6, 1e5], device=DEV)
    Pr = torch.tensor(0.7, device=DEV)
    layer = physics.get_rb2_pde_layer(prandtl=Pr, rayleigh=Ra, **RB2)
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
    res = layer._residues_from_jets(x0.to(DEV), req)
    assert list(res) == list(progs) and lig.stats["residual_torch_fallbacks"] == f0 + 1
    j64 = jets0.double()
    cols = [x0.double()[..., i:i + 1] for i in range(3)]
    pv = [Ra.cpu().double().reshape(-1, 1, 1), Pr.cpu().double().reshape(-1, 1, 1)]
    for name, p in progs.items():
        ref = p.fn(*(cols + pv + [j64[stream_of[a[1]], a[0]].reshape(shape) for a in p.atoms]))
        assert torch.allclose(res[name].cpu().double(), ref, rtol=2e-5, atol=2e-5), name
    for b in range(B):
        const = physics.get_rb2_pde_layer(prandtl=0.7, rayleigh=float(Ra[b].item()), **RB2)
        want = const._residues_from_jets(x0.to(DEV), req)           # (the device evaluator: its coefficients are numbers)
        assert lig.stats["residual_torch_fallbacks"] == f0 + 1
        for name in want:
            assert torch.allclose(res[name][b].cpu().double(), want[name][b].cpu().double(), rtol=2e-5, atol=2e-5), (b, name)


# ---- end to end, dim = 3 --------------------------------------------------------------------------------------------------------
def test_training_step_gradients_of_ra_pr_network_and_latent_match_the_fp64_oracle(hiplib):
    """lat [2, 4, 5, 6, 32], 2 x 200 points, nf = 16 (test_backward_matches_oracle_autograd's shape).  fp64: oracle.jet_ref jets,
    the combined stream as the same combination of the per-pair jets, the lambdified equations, autograd."""
    from oracle import jet_ref as J
    from space_time_pde_amd import local_implicit_grid as lig, physics
    from tests.test_gpu_lig_jet import _net, _params64, _relerr
    g = torch.Generator().manual_seed(5)
    B, N = 2, 200
    lat = 0.5 * torch.randn(B, 4, 5, 6, 32, generator=g)
    pts = 0.02 + 0.96 * torch.rand(B, N, 3, generator=g)
    tgt = torch.randn(B, N, 4, generator=g)
    net = _net("softplus").to(DEV)
    Ra = torch.tensor([2e3, 8e3], device=DEV, requires_grad=True)
    Pr = torch.tensor(0.7, device=DEV, requires_grad=True)
    layer = physics.get_rb2_pde_layer(prandtl=Pr, rayleigh=Ra, t_crop=2., z_crop=1., x_crop=1., use_continuity=True)
    plan = layer._combo_plan()
    assert plan is not None
    alpha_reg, alpha_pde = 4.0, 1.0

    def loss_of(pred, res, target):
        r = torch.stack([res[k] for k in res])
        return alpha_reg * ((pred - target) ** 2).mean() + alpha_pde * (r ** 2).mean()

    latd = lat.to(DEV).requires_grad_(True)
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    n0, f0 = lig.stats["hip_jet_calls"], lig.stats.get("residual_torch_fallbacks", 0)
    pred, res = layer(pts.to(DEV), return_residue=True)
    assert lig.stats["hip_jet_calls"] == n0 + 1, "HIP jet path was not taken"
    assert lig.stats.get("residual_torch_fallbacks", 0) == f0 + 1
    loss = loss_of(pred, res, tgt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()

    p64 = [(w.requires_grad_(True), b.requires_grad_(True)) for w, b in _params64(net)]
    lat64 = lat.double().requires_grad_(True)
    Ra64 = Ra.detach().cpu().double().requires_grad_(True)
    Pr64 = Pr.detach().cpu().double().requires_grad_(True)
    pairs = tuple(sorted(plan["alpha"]))
    full = J.lig_jets(p64, "softplus", lat64, pts.double(), 0., 1., second=pairs, beta=torch.tensor(1.3, dtype=torch.float64))
    full = full.permute(0, 3, 1, 2).reshape(full.shape[0], 4, -1)
    L = sum(plan["alpha"][p] * full[4 + k] for k, p in enumerate(pairs))
    ref = torch.cat([full[:4], L[None]], 0)
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
    assert _relerr(pred.detach(), pred64.detach()) < 2e-5
    assert Ra.grad.shape == (2,) and Pr.grad.shape == () and Ra64.grad.abs().min() > 0
    print("dRa", Ra.grad.cpu().numpy(), Ra64.grad.numpy(), "dPr", Pr.grad.item(), Pr64.grad.item())
    assert _relerr(Ra.grad, Ra64.grad) < 2e-4
    assert _relerr(Pr.grad, Pr64.grad) < 2e-4
    assert _relerr(latd.grad, lat64.grad) < 2e-4
    for k in range(6):
        assert _relerr(net.fc[k].weight.grad, p64[k][0].grad) < 2e-4, "dW%d" % k
        assert _relerr(net.fc[k].bias.grad, p64[k][1].grad) < 2e-4, "db%d" % k


# ---- end to end on a 2-d grid ---------------------------------------------------------------------------------------------------
@pytest.fixture
def nd_train(hiplib):
    from space_time_pde_amd import lig_jet
    prev = lig_jet.set_nd_jets(True), lig_jet.set_nd_jet_backward(True)
    yield lig_jet
    lig_jet.set_nd_jets(prev[0])
    lig_jet.set_nd_jet_backward(prev[1])


def test_burgers_on_a_2d_grid_with_a_learnable_viscosity(nd_train):
    """tests/test_gpu_lig_nd_jet_backward.py's training step (B = 2, N = 37, (4, 5) grid, 8 channels, masked loss) with nu a
    coefficient per batch element.  fp64: the reverse-sweep strategy of the same layer on the CPU."""
    from space_time_pde_amd import _lib, local_implicit_grid as lig, pde
    from tests import lig_nd_jet_bwd_model as BM
    TOL = 2e-4
    lat, pts, mask = BM.make_case(2, (4, 5), 8)
    net0 = BM.make_net(2, 8, "softplus", 1)
    tgt = torch.randn(2, 37, 1, generator=torch.Generator().manual_seed(3))
    layer = pde.PDELayer("t, x", "u", "nu")
    layer.add_equation("dif(u,t)+u*dif(u,x)-nu*dif(dif(u,x),x)", "burgers")

    def loss_of(y, res, target, m):
        return (((y - target) ** 2) * m.unsqueeze(-1)).sum() + ((res["burgers"][..., 0] * m) ** 2).sum()

    net64 = copy.deepcopy(net0).double()
    lat64 = lat.double().requires_grad_(True)
    nu64 = torch.tensor([0.01, 0.03], dtype=torch.float64, requires_grad=True)
    layer.params = {"nu": nu64}               # (update_parameters takes fp32 only: the oracle's values are set directly)
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net64, lat64, q, 0., 1.))
    y64, res64 = layer(pts.double(), return_residue=True)
    loss64 = loss_of(y64, res64, tgt.double(), mask.double())
    gref = torch.autograd.grad(loss64, [lat64, nu64] + [t for k in range(6) for t in (net64.fc[k].weight, net64.fc[k].bias)])

    net = copy.deepcopy(net0).to(DEV)
    latd = lat.to(DEV).requires_grad_(True)
    nu = torch.tensor([0.01, 0.03], device=DEV, requires_grad=True)
    layer.update_parameters({"nu": nu})
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    h0, g0, f0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"], lig.stats.get("residual_torch_fallbacks", 0)
    with _lib.dispatch_trace() as tr:
        y, res = layer(pts.to(DEV), return_residue=True)
        loss = loss_of(y, res, tgt.to(DEV), mask.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0
    assert lig.stats.get("residual_torch_fallbacks", 0) == f0 + 1
    assert tr.has("k_reduce_nd_jet_bwd<", "D = 2"), tr.kernels

    def rel(got, want):
        return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()

    grads = [t.grad for k in range(6) for t in (net.fc[k].weight, net.fc[k].bias)]
    err = {"loss": abs(loss.item() - loss64.item()) / abs(loss64.item()), "dlatent": rel(latd.grad, gref[0]),
           "dnu": rel(nu.grad, gref[1]), "dW": max(rel(a, b) for a, b in zip(grads, gref[2:]))}
    print("burgers 2-d, learnable nu:", err, nu.grad.cpu().numpy(), gref[1].numpy())
    assert nu.grad.shape == (2,) and gref[1].abs().min() > 0
    assert all(v < TOL for v in err.values()), err
