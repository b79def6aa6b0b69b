"""GPU parity of the value-only HIP path for 1-, 2- and 4-d local implicit grids (k_gather_nd -> the IM-NET layer kernels in
their one-stream configuration -> k_reduce_nd) against the CPU oracle on identical fp32 inputs.

Bound: 2e-5 of the tensor's max magnitude -- what the dim = 3 HIP value path is held to against the same oracle
(tests/test_gpu_lig_jet.py, test_value_only_and_nonunit_box / test_edge_cases_empty_single_and_boundary_points).  The LIG
value is continuous across cell faces, so a one-ulp difference in the cell choice at a node cannot open a gap.
Points: B = 2, N = 37 (odd, fills no row tile for any d): 24 random ones, exactly 0, exactly xmax, outside the box on both
sides, grid nodes +-1 ulp (tests/lig_nd_model.py, edge_points).
"""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import lig_nd_model as M

pytestmark = pytest.mark.gpu

TOL = 2e-5
# (d, grid, c): the last two fill the sparse third input tile (d + c + 1 = 36)
CASES = [(1, (5,), 8), (2, (4, 5), 8), (4, (3, 4, 2, 3), 8), (4, (3, 4, 2, 3), 31), (1, (5,), 34)]
BOXES = {1: (3.0,), 2: (2.0, 0.5), 4: (2.0, 1.0, 4.0, 0.5)}
ACT = {"leakyrelu": torch.nn.LeakyReLU, "softplus": torch.nn.Softplus}
_cache = {}


def _relerr(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _setup(d, grid, c, act, xmax=1.0, n=37, nf=16):
    """(net on the GPU, latent, pts, oracle values) of one case; built once, shared, never modified."""
    key = (d, grid, c, act, xmax, n, nf)
    if key not in _cache:
        from space_time_pde_amd import implicit_net
        torch.manual_seed(7 + d)
        net = implicit_net.ImNet(dim=d, in_features=c, out_features=3, nf=nf, activation=ACT[act])
        g = torch.Generator().manual_seed(11 * d + c)
        lat = 0.5 * torch.randn(2, *grid, c, generator=g)
        e0, e1 = (torch.from_numpy(M.edge_points(grid, xmax, seed=s)) for s in (0, 1))
        pts = torch.stack([e0, e1.flip(0)], 0)[:, :n].contiguous()
        p32 = [(net.fc[k].weight.detach().float(), net.fc[k].bias.detach().float()) for k in range(6)]
        box = ((0.,) * d, xmax) if isinstance(xmax, tuple) else (0., xmax)
        ref = O.query_lig(lambda f: O.imnet_forward(p32, f, O.activation_fn(act)), lat, pts, *box)
        _cache[key] = (net.to("cuda:0"), lat, pts, box, ref)
    return _cache[key]


def _query(net, lat, pts, box):
    from space_time_pde_amd import local_implicit_grid as lig
    with torch.no_grad():
        return lig.query_local_implicit_grid(net, lat.to("cuda:0"), pts.to("cuda:0"), *box)


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("act", ["leakyrelu", "softplus"])
@pytest.mark.parametrize("d,grid,c", CASES)
def test_values_match_oracle_on_the_hip_path(hiplib, d, grid, c, act, prec, monkeypatch):
    from space_time_pde_amd import _lib, lig_jet, local_implicit_grid as lig
    monkeypatch.setattr(lig_jet, "mlp_precision", prec)
    net, lat, pts, box, ref = _setup(d, grid, c, act)
    h0, g0 = lig.stats["hip_value_calls"], lig.stats["generic_calls"]
    with _lib.dispatch_trace() as tr:
        y = _query(net, lat, pts, box)
    assert lig.stats["hip_value_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0
    assert tr.has("k_gather_nd", "D = %d" % d) and tr.has("k_reduce_nd", "D = %d" % d), tr.kernels
    assert y.shape == ref.shape
    err = _relerr(y, ref)
    print("d=%d c=%d %s %s: rel err %.3e" % (d, c, act, prec, err))
    assert err < TOL


@pytest.mark.parametrize("d,grid,c", CASES[:3])
def test_nonunit_box(hiplib, d, grid, c):
    from space_time_pde_amd import local_implicit_grid as lig
    net, lat, pts, box, ref = _setup(d, grid, c, "leakyrelu", xmax=BOXES[d])
    h0 = lig.stats["hip_value_calls"]
    y = _query(net, lat, pts, box)
    assert lig.stats["hip_value_calls"] == h0 + 1
    err = _relerr(y, ref)
    print("d=%d box %s: rel err %.3e" % (d, BOXES[d], err))
    assert err < TOL


@pytest.mark.parametrize("d,grid,c", CASES[:4])
def test_chunking_does_not_change_a_bit(hiplib, d, grid, c):
    """one chunk vs. chunks of four row tiles (the smallest), whose ends fall inside batch items"""
    from space_time_pde_amd import lig_jet
    net, lat, pts, box, _ = _setup(d, grid, c, "softplus")
    with torch.no_grad():
        a, _ = lig_jet.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), *box, False, ())
        b, _ = lig_jet.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), *box, False, (), chunk_points=4 * (16 >> d))
        c3, _ = lig_jet.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), *box, False, (), chunk_points=12 * (16 >> d))
    assert a.shape == (1, 3, 74)
    assert torch.equal(a, b) and torch.equal(a, c3)


@pytest.mark.parametrize("d,grid,c", CASES[:3])
def test_one_point_and_one_point_more_than_a_tile(hiplib, d, grid, c):
    from space_time_pde_amd import local_implicit_grid as lig
    for n in (1, (16 >> d) + 1):
        net, lat, pts, box, ref = _setup(d, grid, c, "softplus", n=n)
        h0 = lig.stats["hip_value_calls"]
        y = _query(net, lat, pts, box)
        assert lig.stats["hip_value_calls"] == h0 + 1
        assert y.shape == (2, n, 3) and _relerr(y, ref) < TOL
    with torch.no_grad():
        y = lig.query_local_implicit_grid(net, lat.to("cuda:0"), torch.zeros(2, 0, d, device="cuda:0"), *box)
    assert y.shape == (2, 0, 3)


def test_reference_4d_case_c32_stays_generic(hiplib):
    """d = 4, c = 32: 4 + 32 + 1 = 37 features do not fit the 36 slots of the input image -> composed formulation"""
    from space_time_pde_amd import local_implicit_grid as lig
    net, lat, pts, box, ref = _setup(4, (3, 4, 2, 3), 32, "leakyrelu")
    h0, g0 = lig.stats["hip_value_calls"], lig.stats["generic_calls"]
    y = _query(net, lat, pts, box)
    assert lig.stats["generic_calls"] == g0 + 1 and lig.stats["hip_value_calls"] == h0
    assert _relerr(y, ref) < TOL


def test_bf16_operand_mode_is_routed_to_the_composed_formulation(hiplib, monkeypatch):
    """the value-tile kernels have no one-term bf16 variant: unsupported on this path, stated, not approximated"""
    from space_time_pde_amd import lig_jet, local_implicit_grid as lig
    monkeypatch.setattr(lig_jet, "mlp_precision", "bf16")
    net, lat, pts, box, ref = _setup(2, (4, 5), 8, "softplus")
    h0, g0 = lig.stats["hip_value_calls"], lig.stats["generic_calls"]
    y = _query(net, lat, pts, box)
    assert lig.stats["generic_calls"] == g0 + 1 and lig.stats["hip_value_calls"] == h0
    assert _relerr(y, ref) < TOL
    with pytest.raises(NotImplementedError), torch.no_grad():
        lig_jet.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), *box, False, ())


def test_grad_requiring_latent_takes_the_generic_path_and_its_backward_works(hiplib):
    """same call, latent requires grad, grad mode on: composed formulation; d latent against the oracle's autograd at the
    gradient bound of tests/test_gpu_lig_jet.py (2e-4 of the gradient's max magnitude)"""
    from space_time_pde_amd import lig_jet, local_implicit_grid as lig
    net, lat, pts, box, ref = _setup(2, (4, 5), 8, "softplus")
    latd = lat.to("cuda:0").requires_grad_(True)
    h0, g0 = lig.stats["hip_value_calls"], lig.stats["generic_calls"]
    y = lig.query_local_implicit_grid(net, latd, pts.to("cuda:0"), *box)
    assert lig.stats["generic_calls"] == g0 + 1 and lig.stats["hip_value_calls"] == h0
    assert _relerr(y.detach(), ref) < TOL
    y.sum().backward()
    latc = lat.clone().requires_grad_(True)
    p32 = [(net.fc[k].weight.detach().float().cpu(), net.fc[k].bias.detach().float().cpu()) for k in range(6)]
    O.query_lig(lambda f: O.imnet_forward(p32, f, O.activation_fn("softplus")), latc, pts, *box).sum().backward()
    assert _relerr(latd.grad, latc.grad) < 2e-4
    with pytest.raises(NotImplementedError):          # inside lig_jets the same request is an error, not a fall-back
        lig_jet.lig_jets(net, latd, pts.to("cuda:0"), *box, False, ())
    with pytest.raises(NotImplementedError), torch.no_grad():
        lig_jet.lig_jets(net, latd, pts.to("cuda:0"), *box, True, ())
