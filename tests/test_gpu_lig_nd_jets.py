"""GPU tests of the coordinate derivatives on 1- and 2-d local implicit grids (opt-in ``lig_jet.nd_jets``: k_gather_nd ->
k_coef_nd -> the IM-NET layer kernels in the request's stream set -> k_reduce_nd_jet) against the fp64 jet oracle, the host
model of the two new kernels (tests/lig_nd_jet_model.py) and the reference-semantics PDE oracle.

Bounds: jets 2e-5 of each stream's largest magnitude -- what the dim = 3 jets are held to (tests/test_gpu_lig_jet.py);
residuals 1e-4 * max(|v|max, 1e-3), the project's residual bound (test_edge_cases_empty_single_and_boundary_points there);
the coefficient record bit for bit; the corner sum on its own 4 * terms * 2^-24 * sum |terms| per element (the model's bound).
Points: B = 2, N = 37 (tests/lig_nd_model.py, edge_points): 24 random ones, exactly 0, exactly xmax, outside the box on both
sides (derivatives exactly 0 there) and grid nodes +-1 ulp.  The node points run but are left out of the comparison with the
fp64 oracle -- derivatives jump across cell faces and fp32 and fp64 may pick different cells; they are compared bit for bit
in the coefficient test and in the NaN test.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from oracle import jet_ref as J
from tests import lig_nd_jet_model as JM
from tests import lig_nd_model as M

pytestmark = pytest.mark.gpu

TOL = 2e-5
# (d, grid, c): the last two fill the sparse third input tile (d + c + 1 = 36)
CASES = [(1, (5,), 8), (2, (4, 5), 8), (1, (5,), 34), (2, (4, 5), 33)]
ALL_PAIRS = {1: [(0, 0)], 2: [(0, 0), (0, 1), (1, 1)]}
ACT = {"leakyrelu": torch.nn.LeakyReLU, "softplus": torch.nn.Softplus}
NCMP = 28                       # rows of edge_points compared with the fp64 oracle: all but the nine node points
_cache = {}


@pytest.fixture
def nd_jets(hiplib):
    from space_time_pde_amd import lig_jet
    prev = lig_jet.set_nd_jets(True)
    yield lig_jet
    lig_jet.set_nd_jets(prev)


def _setup(d, grid, c, act, n=37, n_out=3):
    """(net on the GPU, latent, pts [2, n, d], compare mask [2, n], fp64 parameters) of one case; built once, never modified"""
    key = (d, grid, c, act, n, n_out)
    if key not in _cache:
        from space_time_pde_amd import implicit_net
        torch.manual_seed(7 + d)
        net = implicit_net.ImNet(dim=d, in_features=c, out_features=n_out, nf=16, activation=ACT[act])
        g = torch.Generator().manual_seed(11 * d + c)
        lat = 0.5 * torch.randn(2, *grid, c, generator=g)
        e0, e1 = (torch.from_numpy(M.edge_points(grid, 1.0, seed=s)) for s in (0, 1))
        keep = torch.arange(37) < NCMP
        if n == 37:
            pts, mask = torch.stack([e0, e1.flip(0)], 0), torch.stack([keep, keep.flip(0)], 0)
        else:
            pts, mask = torch.stack([e0[:n], e1[:n]], 0), torch.ones(2, n, dtype=torch.bool)
        p64 = [(net.fc[k].weight.detach().double(), net.fc[k].bias.detach().double()) for k in range(6)]
        _cache[key] = (net.to("cuda:0"), lat, pts.contiguous(), mask, p64)
    return _cache[key]


def _oracle(key, p64, act, lat, pts, pp):
    k = ("oracle",) + key + (tuple(pp),)
    if k not in _cache:
        _cache[k] = J.lig_jets(p64, act, lat.double(), pts.double(), 0., 1., second=pp)       # [1 + d + len(pp), b, p, out]
    return _cache[k]


def _check_against_oracle(jets, ref, d, mask, what):
    """jets [S, n_out, b * p] of the HIP path, ref of the oracle: per stream, on the masked points"""
    S, n_out = jets.shape[0], jets.shape[1]
    got = jets.double().cpu().reshape(S, n_out, *mask.shape)
    for s in range(S):
        if 1 + d <= s < 4:
            assert torch.all(got[s] == 0) and not torch.signbit(got[s]).any(), (what, s)
            continue
        want = ref[s if s <= d else s - 4 + 1 + d].permute(2, 0, 1)      # [out, b, p]
        err = (got[s] - want)[:, mask].abs().max().item() / max(want[:, mask].abs().max().item(), 1e-30)
        print("%s stream %d: rel err %.3e" % (what, s, err))
        assert err < TOL, (what, s, err)


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
@pytest.mark.parametrize("d,grid,c", CASES)
def test_jets_match_oracle_on_the_hip_path(nd_jets, d, grid, c, act, prec, monkeypatch):
    from space_time_pde_amd import _lib, local_implicit_grid as lig
    monkeypatch.setattr(nd_jets, "mlp_precision", prec)
    net, lat, pts, mask, p64 = _setup(d, grid, c, act)
    pairs = ALL_PAIRS[d]
    ptsd = pts.to("cuda:0")
    req = lig.JetRequest(ptsd, True, pairs)
    h0, g0, v0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"], lig.stats["hip_value_calls"]
    with _lib.dispatch_trace() as tr, torch.no_grad(), lig.jet_context(req):
        y = lig.query_local_implicit_grid(net, lat.to("cuda:0"), ptsd, 0., 1.)
    assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0 and lig.stats["hip_value_calls"] == v0
    for k in ("k_gather_nd", "k_coef_nd", "k_reduce_nd_jet"):
        assert tr.has(k, "D = %d" % d), tr.kernels
    assert not tr.has("k_reduce_nd<") and not tr.has("k_reduce_fwd")
    S2 = 2 if d == 1 else 4
    assert req.y is y and req.jets.shape == (1 + 3 + S2, 3, 74) and len(req.pairs_out) == S2 and req.pairs_out[:len(pairs)] == pairs
    assert torch.equal(y, req.jets[0].t().reshape(2, 37, 3))
    ref = _oracle((d, grid, c, act), p64, act, lat, pts, req.pairs_out)
    _check_against_oracle(req.jets, ref, d, mask, "d=%d c=%d %s %s" % (d, c, act, prec))
    # exactly 0, exactly xmax, outside on both sides (rows 24 .. 27 of item 0): the clip is flat, every derivative is exactly 0
    assert torch.all(req.jets[1:, :, 24:28] == 0)


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_stream_sets_without_pairs_and_with_six(nd_jets, d, grid, c):
    """(3, 0) and (3, 6) -- the latter not served by the fused fc3 -> fc5 kernel: per-layer kernels all the way"""
    net, lat, pts, mask, p64 = _setup(d, grid, c, "softplus")
    six = (ALL_PAIRS[d] * 6)[:5]
    for pairs, S in (((), 4), (six, 10)):
        with torch.no_grad():
            jets, pp = nd_jets.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, pairs)
        assert jets.shape == (S, 3, 74) and len(pp) == S - 4
        _check_against_oracle(jets, _oracle((d, grid, c, "softplus"), p64, "softplus", lat, pts, pp), d, mask, "d=%d S=%d" % (d, S))


def _gd(d, grid, c, P, N, p_base):
    from space_time_pde_amd import _lib, lig_jet
    gd = _lib.GatherNdDesc()
    gd.D, gd.P, gd.N, gd.B, gd.C, gd.p_base, gd.ntiles = d, P, N, 2, c, p_base, lig_jet.nd_tiles(P, d)
    lo_c, hi_c, cube = lig_jet.box_constants(grid, 0., 1.)
    for k in range(d):
        gd.n[k], gd.lo_c[k], gd.hi_c[k], gd.cube[k] = grid[k], lo_c[k], hi_c[k], cube[k]
    return gd, (lo_c, hi_c, cube)


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_coefficient_record_bitwise(hiplib, d, grid, c):
    """stpde_lig_coef_nd against the host model on all 74 points (node points +-1 ulp included), as one chunk and as a chunk
    that starts inside batch item 0 and ends in item 1 (p_base != 0)"""
    from space_time_pde_amd import _lib
    _, _, pts, _, _ = _setup(d, grid, c, "softplus")
    flat = pts.reshape(-1, d)
    for p0, pc in ((0, 74), (29, 19)):
        chunk = flat[p0:p0 + pc].contiguous()
        gd, box = _gd(d, grid, c, pc, 37, p0)
        coef, chunk_d = torch.full((pc + 1, 16), 7.0, device="cuda:0"), chunk.to("cuda:0")
        _lib.check(hiplib.stpde_lig_coef_nd(C.byref(gd), _lib.ptr(chunk_d), _lib.ptr(coef), _lib.stream_ptr()))
        want, _ = JM.coef_nd(d, chunk.numpy(), grid, *box)
        got = coef.cpu().numpy()
        assert np.array_equal(got[:pc], want) and np.all(got[pc] == 7.0)      # nothing written past P points


def _cfg(S1, S2, pairs):
    from space_time_pde_amd import _lib
    cfg = _lib.JetCfg()
    cfg.S1, cfg.S2 = S1, S2
    for k, (a, b) in enumerate(pairs):
        cfg.pair0[k], cfg.pair1[k] = a, b
    return cfg


# (d, S1, S2, S_mlp, n_out): full streams, S_mlp < S (piecewise-linear activations), the value alone, more than one lane group
REDUCE_CASES = [(1, 3, 2, 6, 3), (1, 3, 2, 4, 3), (2, 3, 4, 8, 3), (2, 3, 4, 4, 7), (2, 3, 6, 10, 16), (2, 3, 0, 4, 3),
                (1, 0, 0, 1, 5), (2, 3, 2, 1, 3)]


@pytest.mark.parametrize("d,S1,S2,S_mlp,n_out", REDUCE_CASES)
def test_reduction_alone_against_the_model(hiplib, d, S1, S2, S_mlp, n_out):
    """stpde_lig_reduce_nd_jet_fwd driven directly: random fc5 rows (every (tile, stream, lane, register) its own value), the
    coefficient records of the 37 edge points, jets with a padded leading dimension.  Per element within the model's bound
    4 * (number of terms) * 2^-24 * sum |terms| of the fp64 evaluation of the same terms."""
    from space_time_pde_amd import _lib, lig_jet
    grid = (5,) if d == 1 else (4, 5)
    pts = M.edge_points(grid, 1.0)
    P, ldp, S = 37, 40, 1 + S1 + S2
    nt = lig_jet.nd_tiles(P, d)
    coef, _ = JM.coef_nd(d, pts, grid, *lig_jet.box_constants(grid, 0., 1.))
    pairs = (ALL_PAIRS[d] * 6)[:S2]
    rng = np.random.default_rng(100 * d + S2 + S_mlp)
    out_pre = rng.standard_normal((nt, S_mlp, 256)).astype(np.float32)
    jets = torch.full((S, n_out, ldp), 7.0, device="cuda:0")
    cfg = _cfg(S1, S2, pairs)
    out_pre_d, coef_d = torch.from_numpy(out_pre).to("cuda:0"), torch.from_numpy(coef).to("cuda:0")
    with _lib.dispatch_trace() as tr:
        _lib.check(hiplib.stpde_lig_reduce_nd_jet_fwd(C.byref(cfg), S_mlp, d, P, nt, n_out, _lib.ptr(out_pre_d), _lib.ptr(coef_d),
                                                      _lib.ptr(jets), ldp, _lib.stream_ptr()))
    assert tr.has("k_reduce_nd_jet", "D = %d" % d), tr.kernels
    got = jets.double().cpu().numpy()
    want, bound, _ = JM.reduce_nd_jet(d, P, n_out, S1, S2, pairs, S_mlp, out_pre, coef, ldp)
    assert np.all(got[:, :, P:] == 7.0)                               # the padding of the rows is not written
    err = np.abs(got[:, :, :P] - want[:, :, :P])
    worst = (err / np.maximum(bound[:, :, :P], 1e-300)).max()
    print("d=%d (%d, %d) S_mlp=%d n_out=%d: worst err / bound %.3f" % (d, S1, S2, S_mlp, n_out, worst))
    assert np.all(err <= bound[:, :, :P])
    if S1:
        assert np.all(got[1 + d:4, :, :P] == 0) and not np.signbit(got[1 + d:4, :, :P]).any()


@pytest.mark.parametrize("d,grid,c", CASES)
def test_chunking_does_not_change_a_bit(nd_jets, d, grid, c):
    """one chunk vs. chunks of four row tiles (the smallest), whose ends fall inside batch items"""
    net, lat, pts, _, _ = _setup(d, grid, c, "softplus")
    with torch.no_grad():
        a, pa = nd_jets.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, ALL_PAIRS[d])
        b, pb = nd_jets.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, ALL_PAIRS[d], chunk_points=4 * (16 >> d))
    assert pa == pb and a.shape == b.shape and a.shape[0] == 4 + len(pa)
    for s in range(a.shape[0]):
        assert torch.equal(a[s], b[s]), s


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_one_point_one_point_more_than_a_tile_and_none(nd_jets, d, grid, c):
    for n in (1, (16 >> d) + 1):
        net, lat, pts, mask, p64 = _setup(d, grid, c, "softplus", n=n)
        with torch.no_grad():
            jets, pp = nd_jets.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, ALL_PAIRS[d])
        assert jets.shape == (4 + len(pp), 3, 2 * n)
        _check_against_oracle(jets, J.lig_jets(p64, "softplus", lat.double(), pts.double(), 0., 1., second=pp), d, mask,
                              "d=%d n=%d" % (d, n))
    with torch.no_grad():
        jets, pp = nd_jets.lig_jets(net, lat.to("cuda:0"), torch.zeros(2, 0, d, device="cuda:0"), 0., 1., True, ALL_PAIRS[d])
    assert jets.shape == (4 + len(pp), 3, 0)


# ---------------------------------------------------------------------------------------------------------------------
# PDELayer end to end
# ---------------------------------------------------------------------------------------------------------------------
PROBLEMS = {
    "burgers": ("t, x", "u", "dif(u,t) + u*dif(u,x) - 0.01*dif(dif(u,x),x)", [(1, 1)]),
    "poisson": ("x, y", "u, v", "dif(dif(u,x),x) + dif(dif(u,y),y) - v", [(0, 0), (1, 1)]),
}


def _problem(name):
    """(layer of the package, residuals of the reference-semantics oracle, net, latent, pts) on the same fp32 inputs"""
    if name not in _cache:
        from space_time_pde_amd import pde
        in_vars, out_vars, eqn, _ = PROBLEMS[name]
        n_out = len(out_vars.split(","))
        net, lat, pts, _, _ = _setup(2, (4, 5), 8, "softplus", n=NCMP, n_out=n_out)    # random, 0, xmax, outside on both sides
        layer = pde.PDELayer(in_vars, out_vars)
        layer.add_equation(eqn, name)
        ora = O.PDEOracle(in_vars, out_vars)
        ora.add_equation(eqn, name)
        p32 = [(net.fc[k].weight.detach().float().cpu(), net.fc[k].bias.detach().float().cpu()) for k in range(6)]
        ora.forward_method = lambda q: O.query_lig(lambda f: O.imnet_forward(p32, f, O.activation_fn("softplus")), lat, q, 0., 1.)
        y, res = ora(pts.clone())
        _cache[name] = (layer, y.detach(), {k: v.detach() for k, v in res.items()}, net, lat, pts)
    return _cache[name]


def _close(res, want):
    for k, v in want.items():
        err = (res[k].detach().cpu() - v).abs().max().item()
        print("%s: residual err %.3e, |v|max %.3e" % (k, err, v.abs().max().item()))
        assert err < 1e-4 * max(v.abs().max().item(), 1e-3), (k, err)


@pytest.mark.parametrize("name", ["burgers", "poisson"])
def test_pde_layer_end_to_end(nd_jets, name, monkeypatch):
    from space_time_pde_amd import _lib, local_implicit_grid as lig
    layer, y_ref, res_ref, net, lat, pts = _problem(name)
    latd, ptsd = lat.to("cuda:0"), pts.to("cuda:0")
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    seen = []
    real = nd_jets.lig_jets

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((a[5], list(a[6]), kw.get("combo"), out[0].shape[0], out[1]))
        return out

    monkeypatch.setattr(nd_jets, "lig_jets", spy)
    h0, g0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"]
    with _lib.dispatch_trace() as tr, torch.no_grad():
        y, res = layer(ptsd, return_residue=True)
    assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0
    assert tr.has("k_coef_nd", "D = 2") and tr.has("k_reduce_nd_jet", "D = 2"), tr.kernels
    want_pairs = PROBLEMS[name][3]
    # second derivatives as pairs in the (3, 2) stream set -- never as the combined stream
    assert seen == [(True, want_pairs, None, 6, want_pairs + [want_pairs[-1]] * (2 - len(want_pairs)))], seen
    assert (y.cpu() - y_ref).abs().max().item() < TOL * y_ref.abs().max().item()
    _close(res, res_ref)
    # switch off: the same layer on the same inputs is the composed formulation under the reverse sweeps (which need grad
    # mode), counted as a generic call, within the same bound
    nd_jets.set_nd_jets(False)
    h0, g0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"]
    with torch.enable_grad():
        y2, res2 = layer(ptsd.clone(), return_residue=True)
    assert lig.stats["generic_calls"] == g0 + 1 and lig.stats["hip_jet_calls"] == h0 and len(seen) == 1
    _close(res2, res_ref)


def test_grad_requiring_latent_keeps_the_composed_formulation(nd_jets):
    from space_time_pde_amd import local_implicit_grid as lig
    net, lat, pts, _, _ = _setup(2, (4, 5), 8, "softplus")
    latd, ptsd = lat.to("cuda:0").requires_grad_(True), pts.to("cuda:0")
    with pytest.raises(NotImplementedError):           # inside lig_jets the request is an error, not a fall-back
        nd_jets.lig_jets(net, latd, ptsd, 0., 1., True, ())
    with pytest.raises(NotImplementedError), torch.no_grad():
        nd_jets.lig_jets(net, latd, ptsd, 0., 1., True, (), combo={(0, 0): 1.0, (1, 1): 1.0})
    with pytest.raises(ValueError), torch.no_grad():
        nd_jets.lig_jets(net, latd, ptsd, 0., 1., True, [(0, 2)])
    h0, g0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"]
    with lig.jet_context(lig.JetRequest(ptsd, True, [])) as req:
        y = lig.query_local_implicit_grid(net, latd, ptsd, 0., 1.)
    assert lig.stats["generic_calls"] == g0 + 1 and lig.stats["hip_jet_calls"] == h0 and req.jets is None
    y.sum().backward()
    assert latd.grad is not None and latd.grad.abs().sum().item() > 0


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_nan_latent_node_stays_where_it_belongs(nd_jets, d, grid, c):
    """One NaN node of batch item 0: NaN on every stream of a present axis at the points whose cell has that node as a corner
    (the cell of the host model = the kernel's, bit for bit), exactly +0.0 on the streams of absent axes everywhere, every
    other point bit-identical to the clean run."""
    net, lat, pts, _, _ = _setup(d, grid, c, "softplus")
    node = (1,) * d
    bad = lat.clone()
    bad[(0,) + node] = float("nan")
    with torch.no_grad():
        clean, _ = nd_jets.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, ALL_PAIRS[d])
        jets, _ = nd_jets.lig_jets(net, bad.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, ALL_PAIRS[d])
    lo_c, hi_c, cube = nd_jets.box_constants(grid, 0., 1.)
    hit = torch.zeros(74, dtype=torch.bool)
    for p in range(37):                                 # batch item 0 only
        i0 = [M.geom_axis(pts[0, p, k].numpy(), lo_c[k], hi_c[k], cube[k], grid[k])[0] for k in range(d)]
        hit[p] = all(node[k] in (i0[k], i0[k] + 1) for k in range(d))
    assert 0 < int(hit.sum()) < 37
    jets, clean = jets.cpu(), clean.cpu()
    for s in range(jets.shape[0]):
        if 1 + d <= s < 4:
            assert torch.all(jets[s] == 0) and not torch.signbit(jets[s]).any()
        else:
            assert torch.isnan(jets[s][:, hit]).all(), s
    assert torch.equal(jets[:, :, ~hit], clean[:, :, ~hit]) and not torch.isnan(clean).any()


def test_evaluate_lattice_equals_a_direct_call(nd_jets):
    from space_time_pde_amd import inference, local_implicit_grid as lig
    layer, _, _, net, lat, _ = _problem("burgers")
    latd = lat.to("cuda:0")
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    t_seq, x_seq = torch.linspace(0.05, 0.95, 6), torch.linspace(0.0, 1.0, 7)
    h0 = lig.stats["hip_jet_calls"]
    out = inference.evaluate_lattice(layer, latd, [t_seq, x_seq], ("u",))      # grad mode on outside: the jets still serve it
    assert lig.stats["hip_jet_calls"] == h0 + 1 and sorted(out) == ["burgers", "u"]
    batch = torch.stack(torch.meshgrid(t_seq, x_seq, indexing="ij"), -1).reshape(1, 42, 2).expand(2, -1, -1).contiguous()
    with torch.no_grad():
        y, res = layer(batch.to("cuda:0"), return_residue=True)
    assert out["u"].shape == (6, 7) and out["burgers"].shape == (6, 7)
    assert np.array_equal(out["u"], y[0, :, 0].cpu().numpy().reshape(6, 7))
    assert np.array_equal(out["burgers"], res["burgers"][0, :, 0].cpu().numpy().reshape(6, 7))
    h0 = lig.stats["hip_jet_calls"]
    out2 = inference.evaluate_lattice(layer, latd, [t_seq, x_seq], ("u",), pseudo_batch_size=16)     # 3 pseudo-batches
    assert lig.stats["hip_jet_calls"] == h0 + 3
    assert np.array_equal(out2["u"], out["u"]) and np.array_equal(out2["burgers"], out["burgers"])
