"""Value-only HIP path for 1-, 2- and 4-d local implicit grids: everything that needs no GPU -- the plan's slot map and
operand packs for dim != 3, the eligibility decision of query_local_implicit_grid, a host model of every address the two new
kernels form (tests/lig_nd_model.py), and the argument checks of the two new entry points."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from space_time_pde_amd import _lib, implicit_net, lig_jet
from space_time_pde_amd import local_implicit_grid as lig
from space_time_pde_amd.lig_jet import ImNetPlan, XT
from tests import lig_nd_model as M
from tests import mfma_emu as E

FAKE = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch
CMAX = {1: 34, 2: 33, 4: 31}         # widest latent per dim: d + c + 1 <= 36


# ---------------------------------------------------------------------------------------------------------------------
# plan: slot map and packs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,cin", [(1, 8), (2, 8), (4, 8), (1, 34), (2, 33), (4, 31)])
def test_slot_map_and_packs_for_other_dims(dim, cin):
    plan = ImNetPlan.get(dim, cin, 3, 16)
    dz = dim + cin
    # direct construction: features 0..31 in order, features 32.. in register 0 of the sparse third tile (slots 32, 36, 40, 44)
    want = [f if f < 32 else 32 + 4 * (f - 32) for f in range(dz + 1)]
    assert plan.slot.tolist() == want and plan.dz == dz and max(want) < 16 * XT
    g = torch.Generator().manual_seed(dim * 100 + cin)
    params = []
    for lay in plan.layers:
        params += [torch.randn(lay["M"], lay["Kin"], generator=g, dtype=torch.float64).float(),
                   torch.randn(lay["M"], generator=g, dtype=torch.float64).float()]
    packs = plan.pack(params).double().numpy()
    rng = np.random.default_rng(0)
    for l in range(6):
        lay = plan.layers[l]
        W, b = params[2 * l].double().numpy(), params[2 * l + 1].double().numpy()
        KT, MT = lay["KT"], lay["MT"]
        h = rng.standard_normal((16, lay["Kh"]))
        xr = rng.standard_normal((16, dz))
        x = np.zeros((16, 16 * XT))                  # the rows as k_gather_nd writes them: [r(d); latent(c); 1] by slot
        x[:, plan.slot[:dz]] = xr
        x[:, plan.slot[dz]] = 1.0
        ws = plan.pack_view(packs, l, "Ws").reshape(XT, MT, 64, 4)
        assert np.all(ws[XT - 1, :, :, 1:] == 0)     # sparse third tile: register 0 only (x_live)
        out = E.gemm_frag(ws, E.to_frag(x), XT, MT)
        if KT:
            out = out + E.gemm_frag(plan.pack_view(packs, l, "Wh").reshape(KT, MT, 64, 4), E.to_frag(h), KT, MT)
        inp = np.concatenate([h, xr], 1) if lay["skip"] else h
        np.testing.assert_allclose(E.from_frag(out)[:, :lay["M"]], inp @ W.T + b, rtol=1e-10, atol=1e-10)


def test_plan_limits_per_dim():
    for dim, c in CMAX.items():
        ImNetPlan(dim, c, 3, 16)
        with pytest.raises(ValueError):
            ImNetPlan(dim, c + 1, 3, 16)
    with pytest.raises(ValueError):
        ImNetPlan(5, 8, 3, 16)
    with pytest.raises(ValueError):
        ImNetPlan(2, 8, 3, 4)                        # nf not a multiple of 16
    assert lig_jet.MAX_LATENT_CHANNELS == 32         # dim = 3 unchanged


def test_nd_tiles():
    for dim, tp in ((1, 8), (2, 4), (4, 1)):
        for P in (1, tp, tp + 1, 4 * tp, 4 * tp + 1, 37, 74):
            nt = lig_jet.nd_tiles(P, dim)
            need = -(-P // tp)
            assert nt % 4 == 0 and need <= nt <= need + 3


# ---------------------------------------------------------------------------------------------------------------------
# eligibility
# ---------------------------------------------------------------------------------------------------------------------
class _T:
    """Stand-in for a CUDA tensor: the decision reads shapes and flags only."""

    def __init__(self, shape, cuda=True, dtype=torch.float32, requires_grad=False):
        self.shape, self.is_cuda, self.dtype, self.requires_grad = tuple(shape), cuda, dtype, requires_grad

    def dim(self):
        return len(self.shape)


def _case(dim, cin, nf=16, grid=None, **kw):
    net = implicit_net.ImNet(dim=dim, in_features=cin, out_features=3, nf=nf, activation=torch.nn.Softplus)
    grid = grid or (3,) * dim
    return net, _T((2,) + tuple(grid) + (cin,), **kw), _T((2, 37, dim))


def test_eligibility_decision(monkeypatch):
    monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
    with torch.no_grad():
        for dim, c in CMAX.items():
            assert lig._nd_value_eligible(*_case(dim, 8))
            assert lig._nd_value_eligible(*_case(dim, c))                 # at the limit: d + c + 1 == 36
            assert not lig._nd_value_eligible(*_case(dim, c + 1))         # one past it
        assert not lig._nd_value_eligible(*_case(4, 32))                  # the reference's own 4-d test case: generic
        assert not lig._nd_value_eligible(*_case(4, 8, nf=4))             # hidden widths are MFMA tiles
        assert not lig._nd_value_eligible(*_case(3, 8))                   # dim = 3 has its own dispatch
        assert not lig._nd_value_eligible(*_case(2, 8, grid=(4, 1)))      # every axis needs a cell
        assert not lig._nd_value_eligible(*_case(2, 8, cuda=False))
        assert not lig._nd_value_eligible(*_case(2, 8, dtype=torch.float64))
        net, lat, pts = _case(2, 8)
        assert not lig._nd_value_eligible(torch.nn.Linear(10, 3), lat, pts)
        assert not lig._nd_value_eligible(net, lat, _T((2, 37, 3)))
        assert not lig._nd_value_eligible(net, _T((2, 3, 3, 9)), pts)
        # an active jet request for THESE points (PDELayer): derivatives wanted -> composed formulation
        assert not lig._nd_value_eligible(net, lat, pts, lig.JetRequest(pts, True, []))
        assert lig._nd_value_eligible(net, lat, pts, lig.JetRequest(_T((2, 37, 2)), True, []))
        for prec, ok in (("fp32x3", True), ("bf16", False)):
            monkeypatch.setattr(lig_jet, "mlp_precision", prec)
            assert lig._nd_value_eligible(net, lat, pts) is ok
        monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
        net_id = implicit_net.ImNet(dim=2, in_features=8, out_features=3, nf=16, activation=torch.nn.Identity)
        assert not lig._nd_value_eligible(net_id, lat, pts)              # unknown activation
    # grad mode: the parameters of a fresh ImNet require grad -> a backward could follow
    net, lat, pts = _case(2, 8)
    assert not lig._nd_value_eligible(net, lat, pts)
    for p in net.parameters():
        p.requires_grad_(False)
    assert lig._nd_value_eligible(net, lat, pts)
    assert not lig._nd_value_eligible(net, _T(lat.shape, requires_grad=True), pts)       # a grad-requiring latent grid
    assert not lig._nd_value_eligible(net, lat, _T(pts.shape, requires_grad=True))       # point gradients
    with torch.no_grad():
        assert lig._nd_value_eligible(net, _T(lat.shape, requires_grad=True), pts)


def test_cpu_queries_keep_the_composed_formulation():
    net = implicit_net.ImNet(dim=2, in_features=8, out_features=3, nf=16)
    n0, h0 = lig.stats["generic_calls"], lig.stats["hip_value_calls"]
    with torch.no_grad():
        y = lig.query_local_implicit_grid(net, torch.rand(2, 4, 5, 8), torch.rand(2, 37, 2), 0., 1.)
    assert y.shape == (2, 37, 3)
    assert lig.stats["generic_calls"] == n0 + 1 and lig.stats["hip_value_calls"] == h0


# ---------------------------------------------------------------------------------------------------------------------
# host model of the addresses (and of the whole pass) on edge points
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = [(1, (5,), 8, 1.0), (2, (4, 5), 8, (2.0, 0.5)), (4, (3, 4, 2, 3), 8, (2.0, 1.0, 4.0, 0.5)),
         (4, (3, 4, 2, 3), 31, 1.0), (1, (5,), 34, 3.0)]


def _box(dim, xmax):
    """(xmin, xmax) as the oracle takes them: both scalars or both sequences"""
    return ((0.,) * dim, xmax) if isinstance(xmax, tuple) else (0., float(xmax))


def _hostile_points(shape, xmax):
    """the 37 edge points plus what no caller should send: NaN, +-inf, +-huge, on every axis and on one axis only"""
    pts = M.edge_points(shape, xmax)
    d = pts.shape[1]
    bad = [np.full(d, v, np.float32) for v in (np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31)]
    one = pts[3].copy()
    one[d - 1] = np.nan
    return np.concatenate([pts, np.stack(bad + [one])], 0)


@pytest.mark.parametrize("dim,shape,cin,xmax", GRIDS)
def test_host_model_addresses_stay_inside_their_buffers(dim, shape, cin, xmax):
    B = 2
    pts1 = _hostile_points(shape, xmax)
    N = pts1.shape[0]
    pts = np.concatenate([pts1, pts1[::-1]], 0)                      # [B * N, d]
    rng = np.random.default_rng(1)
    latent = rng.standard_normal((B,) + shape + (cin,)).astype(np.float32)
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    tp = 16 >> dim
    # one chunk, and chunks that end inside a tile / inside a batch item (p_base > 0; the last one past B * N on purpose:
    # the batch index must clamp)
    for p0, pc in ((0, B * N), (0, 1), (N - 3, tp + 1), (B * N - 2, 2), (B * N + 5, 3)):
        pc_pts = np.resize(pts[p0:p0 + pc], (pc, dim)) if p0 < B * N else pts[:pc]
        nt = lig_jet.nd_tiles(pc, dim)
        X, cw, t = M.gather_nd(dim, pc_pts, latent, N, p0, lo_c, hi_c, cube, nt)
        assert t["pts"] == set(range(pc * dim))                      # reads every coordinate of the chunk, nothing else
        assert min(t["latent"]) >= 0 and max(t["latent"]) < latent.size
        assert t["X"] == set(range(nt * XT * 256)) and t["cw"] == set(range(nt * 16))   # every element written, none outside
        assert np.isfinite(X).all() and np.isfinite(cw).all()        # (a NaN coordinate ends on the upper face, as fminf does)
        # [row][slot]: lane 16g + j of tile xt holds slots 16 xt + 4g .. + 3 of row j
        rows = X.reshape(nt, XT, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(nt * 16, XT * 16)
        live = pc * (1 << dim)
        assert np.all(rows[live:] == 0) and np.all(cw[live:] == 0)   # padding rows: zeros, weight 0
        slot = ImNetPlan.get(dim, cin, 3, 16).slot
        assert np.all(rows[:live, slot[dim + cin]] == 1)             # the ones column
        dead = np.setdiff1d(np.arange(16 * XT), slot)
        assert np.all(rows[:, dead] == 0)
        np.testing.assert_allclose(cw[:live].reshape(pc, -1).sum(1), 1.0, atol=1e-5)     # partition of unity
        y, tr = M.reduce_nd(dim, pc, 3, np.zeros((nt, 64, 4), np.float32), cw)
        assert max(tr["out_pre"]) < nt * 256 and max(tr["cw"]) < nt * 16 and y.shape == (3, pc)


@pytest.mark.parametrize("dim,shape,cin,xmax", M.D3_GRIDS)
def test_host_model_addresses_stay_inside_their_buffers_dim3(dim, shape, cin, xmax):
    """The same for stpde_lig_gather: k_gather / k_gather_tile are the shared gather body at D = 3 (two points per row tile,
    P even, ntiles = P / 2) plus the per-point coefficient epilogue."""
    B = 2
    pts1 = _hostile_points(shape, xmax)
    N = pts1.shape[0]
    pts = np.concatenate([pts1, pts1[::-1]], 0)                      # [B * N, 3]
    rng = np.random.default_rng(1)
    latent = rng.standard_normal((B,) + shape + (cin,)).astype(np.float32)
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    alpha = (0.5, -1.0, 2.0, 0.25, 3.0, -0.75)
    n_nodes = B * int(np.prod(shape))
    # the chunk starts of the 1-, 2- and 4-d test, the lengths rounded up to the even P this entry point takes
    for p0, pc in ((0, B * N), (0, 2), (N - 3, 4), (B * N - 2, 2), (B * N + 5, 4)):
        pc_pts = np.resize(pts[p0:p0 + pc], (pc, dim)) if p0 < B * N else pts[:pc]
        nt = pc // 2
        X, coef, cell, cw, t = M.gather3(pc_pts, latent, N, p0, lo_c, hi_c, cube, alpha)
        assert t["pts"] == set(range(pc * dim))                      # reads every coordinate of the chunk, nothing else
        assert min(t["latent"]) >= 0 and max(t["latent"]) < latent.size
        assert t["X"] == set(range(nt * XT * 256))                   # every element written, none outside
        # coef, cell and cw start as NaN / -1: finite and non-negative means every element was written
        assert X.shape == (nt, XT, 64, 4) and coef.shape == (pc, 16) and cell.shape == (pc,) and cw.shape == (pc, 8)
        assert np.isfinite(X).all() and np.isfinite(coef).all() and np.isfinite(cw).all()
        assert cell.min() >= 0 and cell.max() < n_nodes
        idx = np.unravel_index(cell, (B,) + shape)                   # a corner-0 node: every corner of it is a node of the grid
        assert all((idx[1 + k] <= shape[k] - 2).all() for k in range(dim))
        assert np.all(coef[:, 15] == 0) and np.all(cw[:, 6:] == 0)
        rows = X.reshape(nt, XT, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(nt * 16, XT * 16)
        slot = ImNetPlan.get(dim, cin, 3, 16).slot
        assert np.all(rows[:, slot[dim + cin]] == 1)                 # the ones column
        assert np.all(rows[:, np.setdiff1d(np.arange(16 * XT), slot)] == 0)
        w = np.stack([np.prod([coef[:, 3 * M.corner_bit(c, 3, k) + k] for k in range(3)], 0) for c in range(8)], 1)
        np.testing.assert_allclose(w.sum(1), 1.0, atol=1e-5)         # partition of unity
        assert M.gather3(pc_pts, latent, N, p0, lo_c, hi_c, cube)[3] is None     # cw not requested


@pytest.mark.parametrize("dim,shape,cin,xmax", GRIDS + M.D3_GRIDS)
def test_host_model_geometry_matches_oracle_bitwise(dim, shape, cin, xmax):
    """cell choice, relative coordinates and corner weights of the model (= the kernel's expression sequence) against the
    oracle's interp_coefficients on the edge points: same fp32 operations, so equal to the last bit except the weight product,
    whose order torch.prod does not promise (1 ulp per factor)."""
    pts = M.edge_points(shape, xmax)
    P = pts.shape[0]
    rng = np.random.default_rng(2)
    latent = rng.standard_normal((1,) + shape + (cin,)).astype(np.float32)
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    nt = lig_jet.nd_tiles(P, dim)
    X, cw, _ = M.gather_nd(dim, pts, latent, P, 0, lo_c, hi_c, cube, nt)
    rows = X.reshape(nt, XT, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(nt * 16, XT * 16)[:P << dim]
    slot = ImNetPlan.get(dim, cin, 3, 16).slot
    v, w, rel = O.interp_coefficients(torch.from_numpy(latent), torch.from_numpy(pts)[None], *_box(dim, xmax))
    np.testing.assert_array_equal(rows[:, slot[:dim]], rel[0].reshape(-1, dim).numpy())
    np.testing.assert_array_equal(rows[:, slot[dim:dim + cin]], v[0].reshape(-1, cin).numpy())
    np.testing.assert_allclose(cw[:P << dim], w[0].reshape(-1).numpy(), rtol=dim * 1.2e-7, atol=1e-12)


def _oracle_weight_jets(shape, pts, xmax, dtype):
    """w [P, 8], dw / dq [P, 8, 3], d2w / dq_a dq_b [P, 8, 3, 3] and d rel_d / dq_d [P, 3] of the oracle's interp_coefficients
    in ``dtype`` by torch autograd (every point's outputs depend on that point alone, so gradients of sums are per point)"""
    q = torch.from_numpy(pts)[None].to(dtype).requires_grad_(True)
    _, w, rel = O.interp_coefficients(torch.zeros((1,) + shape + (1,), dtype=dtype), q, *_box(3, xmax))
    P = pts.shape[0]
    dw, ddw = torch.zeros(P, 8, 3, dtype=dtype), torch.zeros(P, 8, 3, 3, dtype=dtype)
    for c in range(8):
        g, = torch.autograd.grad(w[0, :, c].sum(), q, create_graph=True)
        dw[:, c] = g[0].detach()
        for a in range(3):
            ddw[:, c, a] = torch.autograd.grad(g[0, :, a].sum(), q, retain_graph=True)[0][0]
    drel, = torch.autograd.grad(rel[0, :, 0].sum(), q)
    return w[0].detach(), dw, ddw, drel[0]


BOUND = {"w": 5.6e-8, "dw": 9.2e-8, "ddw": 2.6e-6, "w*kap": 9.4e-8}      # the measurement in the docstring below


@pytest.mark.parametrize("dim,shape,cin,xmax", M.D3_GRIDS)
def test_coefficient_model_matches_oracle(dim, shape, cin, xmax):
    """coef_epilogue (= what the dim = 3 gathers write per point) on the 24 random edge points, all strictly inside a cell and
    inside the box.  om is the oracle's per-axis weight |q - opposite| / cube, read off the oracle's relative coordinates
    (|rel| of the corner with the other bit): bit-equal.  The corner weights and their first and second derivatives, rebuilt
    from coef as corner_weights() of csrc/lig_gather_reduce.hip rebuilds them, and w * kap (the factor the corner sum puts on
    the decoder's derivative streams) against torch autograd through the fp64 oracle.
    Bound: 4 x the fp32 oracle's own distance from the fp64 oracle on these points, relative to the largest magnitude of each
    quantity.  Measured, grid (3, 4, 5) / (4, 3, 3): w 9.4e-8 / 5.6e-8, dw 1.2e-7 / 9.2e-8, ddw 1.0e-5 / 2.6e-6 (autograd's
    second derivative of a product of six factors), w * kap 9.4e-8 / 9.5e-8; BOUND holds the smaller of each pair.  The model
    itself sits at 3.0e-8 (6.0e-8 for w * kap on the second grid).
    Points on a clip bound (where s = 0.5) are tests/test_next_rows.py's clip-tie lattice."""
    pts = M.edge_points(shape, xmax)[:24]
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    coef, cell, cw = M.coef_epilogue(pts, shape, 1, 24, 0, lo_c, hi_c, cube, (0.5, -1.0, 2.0, 0.25, 3.0, -0.75))
    _, _, rel = O.interp_coefficients(torch.zeros((1,) + shape + (1,)), torch.from_numpy(pts)[None], *_box(3, xmax))
    rel = rel[0].numpy()                                             # [P, 8, 3]
    for k in range(3):
        np.testing.assert_array_equal(coef[:, k], np.abs(rel[:, 7, k]))          # om[0]: distance to the bit-1 position
        np.testing.assert_array_equal(coef[:, 3 + k], np.abs(rel[:, 0, k]))      # om[1]: distance to the bit-0 position
    assert np.all(coef[:, 12:15] == 1 / np.asarray(cube, np.float32))            # inside the box: s = 1
    om = lambda c, k: coef[:, 3 * M.corner_bit(c, 3, k) + k].astype(np.float64)
    dm = lambda c, k: coef[:, 6 + 3 * M.corner_bit(c, 3, k) + k].astype(np.float64)
    got_w = np.stack([om(c, 0) * om(c, 1) * om(c, 2) for c in range(8)], 1)
    got_dw = np.stack([np.stack([np.prod([dm(c, k) if k == a else om(c, k) for k in range(3)], 0) for a in range(3)], 1)
                       for c in range(8)], 1)
    got_ddw = np.stack([np.stack([np.stack([np.prod([dm(c, k) if k in (a, b) else om(c, k) for k in range(3)], 0) * (a != b)
                                            for b in range(3)], 1) for a in range(3)], 1) for c in range(8)], 1)
    got_wk = got_w[:, :, None] * coef[:, None, 12:15].astype(np.float64)
    w32, dw32, ddw32, dr32 = _oracle_weight_jets(shape, pts, xmax, torch.float32)
    w64, dw64, ddw64, dr64 = _oracle_weight_jets(shape, pts, xmax, torch.float64)
    rows = (("w", got_w, w32, w64), ("dw", got_dw, dw32, dw64), ("ddw", got_ddw, ddw32, ddw64),
            ("w*kap", got_wk, w32[:, :, None] * dr32[:, None], w64[:, :, None] * dr64[:, None]))
    for name, got, o32, o64 in rows:
        scale = o64.abs().max().item()
        own = (o32.double() - o64).abs().max().item() / scale
        err = np.abs(got - o64.numpy()).max() / scale
        print("%s %s: fp32 oracle vs fp64 oracle %.2e, model vs fp64 oracle %.2e" % (shape, name, own, err))
        assert err <= 4 * BOUND[name], (name, err)


@pytest.mark.parametrize("dim,shape,cin,xmax", [GRIDS[0], GRIDS[1], GRIDS[3]])
def test_host_model_whole_pass_matches_oracle(dim, shape, cin, xmax):
    """gather -> layer passes over the operand packs (MFMA emulation, fp64) -> corner sum, against oracle.query_lig in fp64
    on the same points: layout of X, slot map, packs and the reduction's row indexing agree end to end.  Bound: the model's
    geometry is fp32 (1.2e-7 per operation, a handful of operations, decoder of O(1) Lipschitz constant): 1e-5."""
    pts = M.edge_points(shape, xmax)[[0, 5, 24, 25, 26, 27, 29, 30]]     # random, 0, xmax, outside, a node -1 ulp / +1 ulp
    P = pts.shape[0]
    torch.manual_seed(dim)
    net = implicit_net.ImNet(dim=dim, in_features=cin, out_features=3, nf=16, activation=torch.nn.Softplus)
    plan = ImNetPlan.get(dim, cin, 3, 16)
    params = []
    for k in range(6):
        params += [net.fc[k].weight, net.fc[k].bias]
    packs = plan.pack(params).double().numpy()
    rng = np.random.default_rng(3)
    latent = rng.standard_normal((1,) + shape + (cin,)).astype(np.float32)
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    nt = lig_jet.nd_tiles(P, dim)
    X, cw, _ = M.gather_nd(dim, pts, latent, P, 0, lo_c, hi_c, cube, nt)
    out = M.mlp_rows(plan, packs, X, lambda z: np.logaddexp(0.0, z))
    y, _ = M.reduce_nd(dim, P, 3, out, cw.astype(np.float64))
    p64 = [(net.fc[k].weight.detach().double(), net.fc[k].bias.detach().double()) for k in range(6)]
    ref = O.query_lig(lambda f: O.imnet_forward(p64, f, O.activation_fn("softplus")), torch.from_numpy(latent).double(),
                      torch.from_numpy(pts)[None].double(), *_box(dim, xmax))
    err = np.abs(y.T - ref[0].numpy()).max() / np.abs(ref.numpy()).max()
    assert err < 1e-5, err


# ---------------------------------------------------------------------------------------------------------------------
# argument checks of the two entry points (fake pointers: refused before any launch)
# ---------------------------------------------------------------------------------------------------------------------
def _gd(D=2, P=37, N=37, B=2, C=8, p_base=0, ntiles=None, n=(4, 5, 0, 0)):
    d = _lib.GatherNdDesc()
    d.D, d.P, d.N, d.B, d.C, d.p_base = D, P, N, B, C, p_base
    d.ntiles = lig_jet.nd_tiles(P, D) if ntiles is None else ntiles
    for k in range(4):
        d.n[k], d.lo_c[k], d.hi_c[k], d.cube[k] = n[k], 1e-6, 1 - 1e-6, 0.25
    return d


def test_descriptor_layout():
    assert [f[0] for f in _lib.GatherNdDesc._fields_] == ["D", "P", "N", "B", "C", "p_base", "ntiles", "n", "lo_c", "hi_c",
                                                          "cube"]
    assert ctypes.sizeof(_lib.GatherNdDesc) == 4 * (7 + 4 * 4)
    assert _lib.ABI_VERSION == 316                    # additive symbols: the ABI version stays


@pytest.mark.parametrize("why,kw", [
    ("D = 3", dict(D=3, n=(4, 5, 3, 0))), ("D = 0", dict(D=0)), ("D = 5", dict(D=5, ntiles=4)),
    ("do not fit", dict(P=0)), ("do not fit", dict(P=37, ntiles=9)), ("do not fit", dict(P=37, ntiles=14)),
    ("do not fit", dict(ntiles=0)), ("do not fit", dict(D=4, P=1, ntiles=1 << 27, n=(2, 2, 2, 2))),
    ("axis 1", dict(n=(4, 1, 0, 0))), ("axis 3", dict(D=4, n=(3, 4, 2, 1))),
    ("37 features", dict(D=2, C=34)), ("37 features", dict(D=4, C=32, n=(3, 4, 2, 3))), ("features", dict(C=0)),
    ("p_base", dict(p_base=-1)), ("p_base", dict(p_base=2 ** 31 - 10)), ("p_base", dict(N=0)), ("p_base", dict(B=0)),
    ("too large", dict(B=4, n=(1 << 15, 1 << 15, 0, 0))), ("too large", dict(D=4, B=1, n=(1 << 10,) * 4)),
])
def test_gather_nd_refuses_bad_arguments(hiplib, why, kw):
    d = _gd(**kw)
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_gather_nd(ctypes.byref(d), FAKE, FAKE, FAKE, FAKE, None))
    assert "lig_gather_nd" in str(e.value) and why in str(e.value), str(e.value)


def test_gather_nd_refuses_null_pointers(hiplib):
    d = _gd()
    for k in range(4):
        args = [FAKE] * 4
        args[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_gather_nd(ctypes.byref(d), *args, None))
        assert "null pointer" in str(e.value)
    with pytest.raises(ValueError):
        _lib.check(hiplib.stpde_lig_gather_nd(None, FAKE, FAKE, FAKE, FAKE, None))


@pytest.mark.parametrize("why,args", [
    ("D = 3", (3, 8, 4, 3, 8)), ("do not fit", (2, 37, 9, 3, 37)), ("do not fit", (2, 37, 16, 3, 37)),
    ("do not fit", (1, 0, 4, 3, 8)), ("n_out", (2, 37, 12, 0, 37)), ("n_out", (2, 37, 12, 17, 37)),
    ("ldp", (4, 5, 8, 3, 4)),
])
def test_reduce_nd_refuses_bad_arguments(hiplib, why, args):
    D, P, nt, n_out, ldp = args
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_reduce_nd_fwd(D, P, nt, n_out, FAKE, FAKE, FAKE, ldp, None))
    assert "lig_reduce_nd_fwd" in str(e.value) and why in str(e.value), str(e.value)
    for k in range(3):
        ptrs = [FAKE] * 3
        ptrs[k] = None
        with pytest.raises(ValueError):
            _lib.check(hiplib.stpde_lig_reduce_nd_fwd(2, 37, 12, 3, *ptrs, 37, None))


def test_lig_jets_refuses_what_the_nd_path_does_not_serve():
    """no quiet fall-back inside lig_jets: derivative requests and CPU tensors on dim != 3 are errors there (the dispatch in
    local_implicit_grid routes them to the composed formulation before)"""
    net = implicit_net.ImNet(dim=2, in_features=8, out_features=3, nf=16)
    with pytest.raises(RuntimeError):
        lig_jet.lig_jets(net, torch.rand(1, 4, 5, 8), torch.rand(1, 5, 2), 0., 1., False, ())
