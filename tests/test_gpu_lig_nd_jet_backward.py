"""GPU tests of training through the coordinate derivatives on 1- and 2-d local implicit grids (opt-in ``lig_jet.nd_jets`` +
``lig_jet.nd_jet_backward``): k_gather_nd -> k_coef_nd -> the IM-NET layer kernels -> k_reduce_nd_jet, and back through
k_reduce_nd_jet_bwd -> the per-kernel layer / weight-gradient sequence of dim = 3 -> k_xbar -> k_cell_nd -> cell sort ->
k_dlat_reduce_nd, against the fp64 jet oracle differentiated by autograd and the host model of the new kernel.

Bounds: the project's own for the dim = 3 jet backward (tests/test_gpu_lig_jet.py), relative to each tensor's largest magnitude:
2e-5 for every jet stream, 2e-4 for d latent, for each of the 12 parameter gradients and for beta.  The fp32 evaluation of the
oracle itself stays within a quarter of each on these inputs (tests/test_lig_nd_jet_backward_host.py).
Inputs: tests/lig_nd_jet_bwd_model.py (make_case / make_net / cotangent): B = 2, N = 37, nf = 16, 3 outputs, the edge points of
tests/test_gpu_lig_nd_jets.py.  Every test appends the errors it measured to test_reports/lig_nd_jet_train_errors.json.
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import lig_nd_jet_bwd_model as BM
from tests import lig_nd_jet_model as JM
from tests import lig_nd_model as M

pytestmark = pytest.mark.gpu

TOL_JET, TOL_GRAD = 2e-5, 2e-4
CASES = BM.GRAD_CASES
ALL_PAIRS = BM.ALL_PAIRS
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_reports", "lig_nd_jet_train_errors.json")
_cache, _errors = {}, {}


@pytest.fixture
def train(hiplib):
    from space_time_pde_amd import lig_jet
    prev = lig_jet.set_nd_jets(True), lig_jet.set_nd_jet_backward(True)
    yield lig_jet
    lig_jet.set_nd_jets(prev[0])
    lig_jet.set_nd_jet_backward(prev[1])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _errors:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        worst = {k: max(v[k] for v in _errors.values() if k in v) for k in ("jets", "dlatent", "dW", "beta")
                 if any(k in v for v in _errors.values())}
        with open(REPORT, "w") as f:
            json.dump({"bounds": {"jets": TOL_JET, "dlatent": TOL_GRAD, "dW": TOL_GRAD, "beta": TOL_GRAD}, "max": worst,
                       "cases": _errors}, f, indent=1, sort_keys=True)


def _case(d, grid, c, act):
    """(CPU net, latent, pts, mask) of a case, built once and never modified"""
    key = (d, grid, c, act)
    if key not in _cache:
        _cache[key] = (BM.make_net(d, c, act),) + BM.make_case(d, grid, c)
    return _cache[key]


def _ref(d, grid, c, act, pairs):
    """fp64 oracle of a case for the padded pairs: (jets, d latent, [12], d beta), computed once"""
    key = ("ref", d, grid, c, act, tuple(pairs))
    if key not in _cache:
        net, lat, pts, mask = _case(d, grid, c, act)
        _cache[key] = BM.oracle(net, act, lat, pts, pairs, BM.cotangent(d, c, 4 + len(pairs), mask), torch.float64)
    return _cache[key]


def _run(lj, d, grid, c, act, pairs, cot=None, **kw):
    """one forward + backward of lig_jets on the GPU: (jets, padded pairs, d latent, [12 gradients], d beta or None)"""
    net, lat, pts, mask = _case(d, grid, c, act)
    net = copy.deepcopy(net).to("cuda:0")
    latd = lat.to("cuda:0").requires_grad_(True)
    jets, pp = lj.lig_jets(net, latd, pts.to("cuda:0"), 0., 1., True, pairs, **kw)
    cot = BM.cotangent(d, c, jets.shape[0], mask) if cot is None else cot
    (jets * cot.to("cuda:0")).sum().backward()
    grads = [t.grad for k in range(6) for t in (net.fc[k].weight, net.fc[k].bias)]
    return jets.detach(), pp, latd.grad, grads, (net.activ.beta.grad if act == "swish" else None)


def _rel(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def _check(what, d, mask, got, ref):
    """jets on the masked points per stream, d latent, the 12 parameter gradients and beta against the oracle, at the bounds"""
    jets, _, dlat, grads, dbeta = got
    m = mask.reshape(-1)
    err = {"jets": 0.0}
    for s in range(jets.shape[0]):
        if 1 + d <= s < 4:
            assert torch.all(jets[s] == 0) and not torch.signbit(jets[s]).any(), (what, s)
            continue
        err["jets"] = max(err["jets"], _rel(jets[s][:, m.to(jets.device)], ref[0][s][:, m]))
    err["dlatent"] = _rel(dlat, ref[1])
    err["dW"] = max(_rel(g, r) for g, r in zip(grads, ref[2]))
    if dbeta is not None:
        err["beta"] = _rel(dbeta, ref[3])
    print(what, " ".join("%s %.3e" % kv for kv in sorted(err.items())))
    _errors[what] = err
    assert err["jets"] < TOL_JET and err["dlatent"] < TOL_GRAD and err["dW"] < TOL_GRAD and err.get("beta", 0.0) < TOL_GRAD, (what, err)
    return err


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
@pytest.mark.parametrize("d,grid,c", CASES)
def test_gradients_match_the_oracle(train, d, grid, c, act, prec, monkeypatch):
    from space_time_pde_amd import _lib, local_implicit_grid as lig
    monkeypatch.setattr(train, "mlp_precision", prec)
    net, lat, pts, mask = _case(d, grid, c, act)
    net = copy.deepcopy(net).to("cuda:0")
    latd, ptsd = lat.to("cuda:0").requires_grad_(True), pts.to("cuda:0")
    req = lig.JetRequest(ptsd, True, ALL_PAIRS[d])
    h0, g0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"]
    with _lib.dispatch_trace() as tr:
        with lig.jet_context(req):
            y = lig.query_local_implicit_grid(net, latd, ptsd, 0., 1.)
        assert req.y is y and req.jets is not None
        cot = BM.cotangent(d, c, req.jets.shape[0], mask)
        (req.jets * cot.to("cuda:0")).sum().backward()
    assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0
    for k in ("k_gather_nd<", "k_coef_nd<", "k_reduce_nd_jet<", "k_reduce_nd_jet_bwd<", "k_cell_nd<", "k_dlat_reduce_nd<"):
        assert tr.has(k, "D = %d" % d), (k, tr.kernels)
    assert not tr.has("k_reduce_nd_bwd<") and not tr.has("k_reduce_bwd")
    grads = [t.grad for k in range(6) for t in (net.fc[k].weight, net.fc[k].bias)]
    _check("d=%d c=%d %s %s" % (d, c, act, prec), d, mask, (req.jets.detach(), req.pairs_out, latd.grad, grads, None),
           _ref(d, grid, c, act, req.pairs_out))


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_swish_with_learnable_beta(train, d, grid, c):
    got = _run(train, d, grid, c, "swish", ALL_PAIRS[d])
    assert got[4] is not None
    _check("d=%d c=%d swish" % (d, c), d, _case(d, grid, c, "swish")[3], got, _ref(d, grid, c, "swish", got[1]))


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_stream_sets_without_pairs_and_with_six(train, d, grid, c):
    """(3, 0) and (3, 6) -- the latter not served by the fused fc3 -> fc5 kernels: per-layer kernels all the way"""
    for pairs, S in (((), 4), ((ALL_PAIRS[d] * 6)[:5], 10)):
        got = _run(train, d, grid, c, "softplus", pairs)
        assert got[0].shape == (S, 3, 74) and len(got[1]) == S - 4
        _check("d=%d c=%d softplus S=%d" % (d, c, S), d, _case(d, grid, c, "softplus")[3], got, _ref(d, grid, c, "softplus", got[1]))


@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
@pytest.mark.parametrize("d,grid,c", CASES)
def test_weight_columns_of_latent_channels(train, d, grid, c, act):
    """Columns d .. 2 of the raw-input block of fc0 and of every skip weight multiply latent channels 0 .. 2 - d on these
    grids -- the columns a stray tangent row sum would land in -- compared on their own, relative to their own magnitude."""
    got = _run(train, d, grid, c, act, ALL_PAIRS[d])
    ref = _ref(d, grid, c, act, got[1])
    worst = 0.0
    for l in range(5):
        kh = got[3][2 * l].shape[1] - (d + c)
        cols = slice(kh + d, kh + 3)
        worst = max(worst, _rel(got[3][2 * l][:, cols], ref[2][2 * l][:, cols]))
    print("d=%d c=%d %s: latent weight columns rel err %.3e" % (d, c, act, worst))
    _errors["d=%d c=%d %s latent columns" % (d, c, act)] = {"dW": worst}
    assert worst < TOL_GRAD


@pytest.mark.parametrize("d,grid,c", [CASES[1], CASES[3]])
def test_cell_face_points_against_the_fp32_oracle(train, d, grid, c):
    """The (4, 5) grid with a cotangent on EVERY point, the node rows that make_case masks included, so that points on cell
    faces contribute to d latent and to the weight gradients.  The fp64 oracle is no reference there (make_case: fp32 has
    q - node == 0 at a node k / 3, fp64 has 3e-8, and the first derivatives differ by O(1)), the oracle evaluated in fp32 is: its
    geometry is the kernels' expression sequence (the coefficient record agrees with it bit for bit,
    tests/test_lig_nd_jet_host.py), so both pick the same cell and the same abs'(0) = 0.  Bounds: those of the other tests --
    the fp32 oracle is itself within a quarter of them of the exact values where those are comparable."""
    net, lat, pts, _ = _case(d, grid, c, "softplus")
    every = torch.ones(2, 37, dtype=torch.bool)
    cot = BM.cotangent(d, c, 8, every)
    got = _run(train, d, grid, c, "softplus", ALL_PAIRS[d], cot)
    ref = BM.oracle(net, "softplus", lat, pts, got[1], cot, torch.float32)
    ref = (ref[0].double(), ref[1].double(), [g.double() for g in ref[2]], None)
    _check("d=%d c=%d softplus every point vs fp32 oracle" % (d, c), d, every, got, ref)


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_nan_cotangent_on_an_absent_axis_reaches_nothing(train, d, grid, c):
    mask = _case(d, grid, c, "softplus")[3]
    S = 4 + (2 if d == 1 else 4)
    zero = BM.cotangent(d, c, S, mask)
    zero[1 + d:4] = 0.0
    nan = zero.clone()
    nan[1 + d:4] = float("nan")
    with_det = lambda cot: _run(train, d, grid, c, "softplus", ALL_PAIRS[d], cot)
    from space_time_pde_amd import _lib
    prev, _lib.deterministic = _lib.deterministic, True        # weight gradients reproducible: bit for bit comparable
    try:
        a, b = with_det(zero), with_det(nan)
    finally:
        _lib.deterministic = prev
    assert torch.equal(a[2], b[2]) and not torch.isnan(b[2]).any()
    for ga, gb in zip(a[3], b[3]):
        assert torch.equal(ga, gb) and not torch.isnan(gb).any()


def _cfg(S1, S2, pairs):
    from space_time_pde_amd import _lib
    cfg = _lib.JetCfg()
    cfg.S1, cfg.S2 = S1, S2
    for k, (a, b) in enumerate(pairs):
        cfg.pair0[k], cfg.pair1[k] = a, b
    return cfg


# (d, S1, S2, S_mlp, n_out, P): full streams, S_mlp < S (piecewise-linear activations), more than one lane group, one point,
# one point more than a tile
KERNEL_CASES = [(1, 3, 2, 6, 3, 37), (1, 3, 2, 4, 3, 37), (2, 3, 4, 8, 3, 37), (2, 3, 4, 4, 7, 37), (2, 3, 6, 10, 16, 37),
                (2, 3, 0, 4, 3, 37), (1, 3, 0, 4, 3, 1), (2, 3, 2, 6, 3, 5), (1, 3, 4, 8, 16, 9)]


@pytest.mark.parametrize("d,S1,S2,S_mlp,n_out,P", KERNEL_CASES)
def test_adjoint_kernel_alone_against_the_model(hiplib, d, S1, S2, S_mlp, n_out, P):
    """stpde_lig_reduce_nd_jet_bwd through the C ABI: random cotangent with a padded leading dimension and NaN on the rows of
    the absent axes and in the padding, the coefficient records of the edge points, a NaN-prefilled output buffer.  The
    whole buffer -- padding rows, features >= n_out, absent-axis streams included -- bit for bit against the fp32 model, whose
    operation order is the kernel's, and within the model's bound of the fp64 evaluation of the same terms."""
    from space_time_pde_amd import _lib, lig_jet
    grid = (5,) if d == 1 else (4, 5)
    pts = M.edge_points(grid, 1.0)[:P]
    ldp, S = P + 3, 1 + S1 + S2
    nt = lig_jet.nd_tiles(P, d)
    coef, _ = JM.coef_nd(d, pts, grid, *lig_jet.box_constants(grid, 0., 1.))
    pairs = (ALL_PAIRS[d] * 6)[:S2]
    rng = np.random.default_rng(100 * d + S2 + S_mlp + P)
    ybar = rng.standard_normal((S, n_out, ldp)).astype(np.float32)
    ybar[:, :, P:] = np.nan
    ybar[1 + d:4] = np.nan
    out = torch.full((nt + 1, S_mlp, 256), float("nan"), device="cuda:0")
    cfg = _cfg(S1, S2, pairs)
    ybar_d, coef_d = torch.from_numpy(ybar).to("cuda:0"), torch.from_numpy(coef).to("cuda:0")
    with _lib.dispatch_trace() as tr:
        _lib.check(hiplib.stpde_lig_reduce_nd_jet_bwd(C.byref(cfg), S_mlp, d, P, nt, n_out, _lib.ptr(ybar_d), ldp, _lib.ptr(coef_d),
                                                      _lib.ptr(out), _lib.stream_ptr()))
    assert tr.has("k_reduce_nd_jet_bwd<", "D = %d" % d), tr.kernels
    got = out.cpu().numpy()
    assert np.isnan(got[nt]).all()                                      # nothing written past ntiles tiles
    want32, _, _ = BM.reduce_nd_jet_bwd(d, P, nt, n_out, S1, S2, pairs, S_mlp, ybar, coef, ldp, np.float32)
    want64, bound, _ = BM.reduce_nd_jet_bwd(d, P, nt, n_out, S1, S2, pairs, S_mlp, ybar, coef, ldp, np.float64)
    got = got[:nt].reshape(want32.shape)
    assert not np.isnan(got).any()
    assert np.all(np.abs(got - want64) <= bound)
    assert np.array_equal(got.view(np.uint32), want32.view(np.uint32))


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_chunking(train, d, grid, c):
    """chunks of four row tiles (the smallest), whose ends fall inside batch items, against one chunk"""
    a = _run(train, d, grid, c, "softplus", ALL_PAIRS[d])
    b = _run(train, d, grid, c, "softplus", ALL_PAIRS[d], chunk_points=4 * (16 >> d))
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    _check("d=%d c=%d softplus chunked" % (d, c), d, _case(d, grid, c, "softplus")[3], b, _ref(d, grid, c, "softplus", b[1]))


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_recompute_and_second_backward(train, d, grid, c, monkeypatch):
    from space_time_pde_amd import _lib
    monkeypatch.setattr(_lib, "deterministic", True)
    base = _run(train, d, grid, c, "softplus", ALL_PAIRS[d])
    monkeypatch.setattr(train, "force_recompute", True)
    n0 = train.stats["recompute_steps"]
    rec = _run(train, d, grid, c, "softplus", ALL_PAIRS[d])
    assert train.stats["recompute_steps"] == n0 + 1
    assert torch.equal(rec[0], base[0]) and torch.equal(rec[2], base[2])      # the same kernels on the same inputs
    for ga, gb in zip(rec[3], base[3]):
        assert torch.equal(ga, gb)
    rec = _run(train, d, grid, c, "softplus", ALL_PAIRS[d], chunk_points=4 * (16 >> d))     # ... and chunk by chunk
    _check("d=%d c=%d softplus recompute" % (d, c), d, _case(d, grid, c, "softplus")[3], rec, _ref(d, grid, c, "softplus", rec[1]))
    monkeypatch.setattr(train, "force_recompute", False)
    # retain_graph + a second backward: the stash is rebuilt, the gradients accumulate to exactly twice
    net, lat, pts, mask = _case(d, grid, c, "softplus")
    net = copy.deepcopy(net).to("cuda:0")
    latd = lat.to("cuda:0").requires_grad_(True)
    jets, pp = train.lig_jets(net, latd, pts.to("cuda:0"), 0., 1., True, ALL_PAIRS[d])
    loss = (jets * BM.cotangent(d, c, jets.shape[0], mask).to("cuda:0")).sum()
    loss.backward(retain_graph=True)
    loss.backward()
    assert torch.equal(latd.grad, 2 * base[2])
    for k in range(6):
        assert torch.equal(net.fc[k].weight.grad, 2 * base[3][2 * k]) and torch.equal(net.fc[k].bias.grad, 2 * base[3][2 * k + 1])


@pytest.mark.parametrize("d,grid,c", CASES[:2])
def test_determinism(train, d, grid, c, monkeypatch):
    from space_time_pde_amd import _lib
    a, b = (_run(train, d, grid, c, "softplus", ALL_PAIRS[d]) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])            # jets and d latent: always
    monkeypatch.setattr(_lib, "deterministic", True)
    a, b = (_run(train, d, grid, c, "softplus", ALL_PAIRS[d]) for _ in range(2))
    assert torch.equal(a[2], b[2])
    for ga, gb in zip(a[3], b[3]):
        assert torch.equal(ga, gb)
    _check("d=%d c=%d softplus det" % (d, c), d, _case(d, grid, c, "softplus")[3], a, _ref(d, grid, c, "softplus", a[1]))


# ---------------------------------------------------------------------------------------------------------------------
# PDELayer end to end: a regression loss on the value plus an l2 residual loss, backward
# ---------------------------------------------------------------------------------------------------------------------
PROBLEMS = {
    "burgers": ("t, x", "u", "dif(u,t) + u*dif(u,x) - 0.01*dif(dif(u,x),x)", [(1, 1)],
                lambda x, j, p: j[1][0] + j[0][0] * j[2][0] - 0.01 * j[4 + p.index((1, 1))][0]),
    "poisson": ("x, y", "u, v", "dif(dif(u,x),x) + dif(dif(u,y),y) - v", [(0, 0), (1, 1)],
                lambda x, j, p: j[4 + p.index((0, 0))][0] + j[4 + p.index((1, 1))][0] - j[0][1]),
}


def _pde_ref(name):
    """fp64: oracle jets -> the same equation in torch -> autograd.  (loss, d latent, [12 gradients]), computed once"""
    if ("pde", name) not in _cache:
        from oracle import jet_ref as J
        in_vars, out_vars, _, pairs, eqn = PROBLEMS[name]
        n_out = len(out_vars.split(","))
        lat, pts, mask = BM.make_case(2, (4, 5), 8)
        net = BM.make_net(2, 8, "softplus", n_out)
        tgt = torch.randn(2, 37, n_out, generator=torch.Generator().manual_seed(3))
        prm = [t.detach().double().requires_grad_(True) for k in range(6) for t in (net.fc[k].weight, net.fc[k].bias)]
        latd = lat.double().requires_grad_(True)
        pp = pairs + [pairs[-1]] * (2 - len(pairs))
        jets = BM.to_hip_order(J.lig_jets(list(zip(prm[0::2], prm[1::2])), "softplus", latd, pts.double(), 0., 1., second=pp), 2)
        m = mask.reshape(-1).double()
        res = eqn(None, jets, pp)
        y = jets[0].t().reshape(2, 37, n_out)
        loss = (((y - tgt.double()) ** 2) * mask.unsqueeze(-1)).sum() + ((res * m) ** 2).sum()
        g = torch.autograd.grad(loss, [latd] + prm)
        _cache[("pde", name)] = (net, lat, pts, mask, tgt, loss.item(), g[0], list(g[1:]))
    return _cache[("pde", name)]


@pytest.mark.parametrize("name", ["burgers", "poisson"])
def test_pde_layer_training_step(train, name):
    """The masked points carry the loss (the node rows of the (4, 5) grid run and carry none: make_case)."""
    from space_time_pde_amd import _lib, local_implicit_grid as lig, pde
    net0, lat, pts, mask, tgt, loss_ref, dlat_ref, g_ref = _pde_ref(name)
    in_vars, out_vars, eqn, _, _ = PROBLEMS[name]
    layer = pde.PDELayer(in_vars, out_vars)
    layer.add_equation(eqn, name)
    md = mask.to("cuda:0")

    def step(expect_hip):
        net = copy.deepcopy(net0).to("cuda:0")
        latd, ptsd = lat.to("cuda:0").requires_grad_(True), pts.to("cuda:0")
        layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
        h0, g0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"]
        with _lib.dispatch_trace() as tr:
            y, res = layer(ptsd, return_residue=True)
            loss = (((y - tgt.to("cuda:0")) ** 2) * md.unsqueeze(-1)).sum() + ((res[name][..., 0] * md) ** 2).sum()
            loss.backward()
        if expect_hip:
            assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0
            assert tr.has("k_reduce_nd_jet_bwd<", "D = 2"), tr.kernels
        else:
            assert lig.stats["hip_jet_calls"] == h0 and lig.stats["generic_calls"] == g0 + 1
            assert not tr.has("k_reduce_nd_jet_bwd<")
        grads = [t.grad for k in range(6) for t in (net.fc[k].weight, net.fc[k].bias)]
        err = {"loss": abs(loss.item() - loss_ref) / abs(loss_ref), "dlatent": _rel(latd.grad, dlat_ref),
               "dW": max(_rel(g, r) for g, r in zip(grads, g_ref))}
        what = "%s step %s" % (name, "hip" if expect_hip else "composed")
        print(what, err)
        _errors[what] = {k: v for k, v in err.items() if k != "loss"}
        assert err["loss"] < TOL_GRAD and err["dlatent"] < TOL_GRAD and err["dW"] < TOL_GRAD, (what, err)

    step(True)
    train.set_nd_jet_backward(False)      # the same step composed: the reverse sweeps through torch ops
    step(False)


def test_refusals_inside_lig_jets(train, monkeypatch):
    """no quiet fall-back: what the backward does not serve is an error of lig_jets itself"""
    from space_time_pde_amd import implicit_net
    net, lat, pts, _ = _case(2, (4, 5), 8, "softplus")
    net = copy.deepcopy(net).to("cuda:0")
    latd, ptsd = lat.to("cuda:0").requires_grad_(True), pts.to("cuda:0")
    wide = implicit_net.ImNet(dim=2, in_features=33, out_features=3, nf=16, activation=torch.nn.Softplus).to("cuda:0")
    with pytest.raises(NotImplementedError):
        train.lig_jets(wide, torch.randn(2, 4, 5, 33, device="cuda:0").requires_grad_(True), ptsd, 0., 1., True, ())
    with pytest.raises(NotImplementedError):
        train.lig_jets(net, latd, ptsd, 0., 1., True, (), combo={(0, 0): 1.0, (1, 1): 1.0})
    with pytest.raises(NotImplementedError):
        train.lig_jets(net, latd, ptsd, 0., 1., True, (), precision="bf16")
    net4 = implicit_net.ImNet(dim=4, in_features=8, out_features=3, nf=16, activation=torch.nn.Softplus).to("cuda:0")
    with pytest.raises(NotImplementedError):
        train.lig_jets(net4, torch.randn(2, 3, 3, 3, 3, 8, device="cuda:0").requires_grad_(True),
                       torch.rand(2, 37, 4, device="cuda:0"), 0., 1., True, ())
    with pytest.raises(ValueError):
        train.lig_jets(net, latd, ptsd, 0., 1., True, [(0, 2)])
    monkeypatch.setattr(train, "expect_two_phase", True)
    with pytest.raises(NotImplementedError):
        train.lig_jets(net, latd, ptsd, 0., 1., True, ())
    monkeypatch.setattr(train, "expect_two_phase", False)
    train.set_nd_jet_backward(False)      # the switch off: the refusal of the forward-only jets, as before
    with pytest.raises(NotImplementedError):
        train.lig_jets(net, latd, ptsd, 0., 1., True, ())
