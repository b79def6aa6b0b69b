"""GPU tests of the coordinate derivatives on 4-d local implicit grids -- 3-d space + time -- (opt-in ``lig_jet.nd4_jets``:
k_gather_nd<4> -> k_coef_nd4 -> per pass of lig_jet.nd4_passes the IM-NET layer kernels in the pass's stream set with the
tangent constants of its axis triple -> k_reduce_nd4_jet) against the fp64 jet oracle, the host model of the two new kernels
(tests/lig_nd4_jet_model.py) and the reference-semantics PDE oracle.

Bounds: jets 2e-5 of each stream's largest magnitude -- what the dim = 3 and dim <= 2 jets are held to (tests/test_gpu_lig_jet.py,
tests/test_gpu_lig_nd_jets.py); residuals 1e-4 * max(|v|max, 1e-3), the project's residual bound; the coefficient record bit
for bit; the corner sum on its own 4 * terms * 2^-24 * sum |terms| per element (the model's bound, derived there for d = 4).
Points: B = 2, N = 37 (tests/lig_nd_model.py, edge_points): 24 random ones, exactly 0, exactly xmax, outside the box on both
sides (derivatives exactly 0 there) and grid nodes +-1 ulp.  The nine node points run but are left out of the comparison with
the fp64 oracle -- derivatives jump across cell faces and fp32 and fp64 may pick different cells; they are compared bit for bit
in the coefficient test and in the non-finite test.  The measured maxima go to test_reports/lig_nd4_jets_errors.json (not
tracked); a copy of an MI355X run is profiles/lig_nd4_jets_errors.json.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from oracle import jet_ref as J
from tests import lig_nd4_jet_model as JM4
from tests import lig_nd_model as M

pytestmark = pytest.mark.gpu

TOL = 2e-5
GRID = (3, 4, 2, 3)
CASES = [(4, GRID, 8), (4, GRID, 31)]        # the second fills the sparse third input tile (4 + 31 + 1 = 36)
ALL_PAIRS = [(a, b) for a in range(4) for b in range(a, 4)]
NS_PAIRS = [(1, 1), (2, 2), (3, 3)]
ACT = {"leakyrelu": torch.nn.LeakyReLU, "softplus": torch.nn.Softplus}
NCMP = 28                       # rows of edge_points compared with the fp64 oracle: all but the nine node points
REPORT_DIR = "test_reports"
_cache, _report = {}, {}


def _record(key, value):
    _report[key] = value
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "lig_nd4_jets_errors.json"), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)


@pytest.fixture
def nd4(hiplib):
    from space_time_pde_amd import lig_jet
    prev = lig_jet.set_nd4_jets(True)
    yield lig_jet
    lig_jet.set_nd4_jets(prev)


def _setup(c, act, n=37, n_out=3):
    """(net on the GPU, latent, pts [2, n, 4], compare mask [2, n], fp64 parameters) of one case; built once, never modified"""
    key = (c, act, n, n_out)
    if key not in _cache:
        from space_time_pde_amd import implicit_net
        torch.manual_seed(11)
        net = implicit_net.ImNet(dim=4, in_features=c, out_features=n_out, nf=16, activation=ACT[act])
        g = torch.Generator().manual_seed(44 + c)
        lat = 0.5 * torch.randn(2, *GRID, c, generator=g)
        e0, e1 = (torch.from_numpy(M.edge_points(GRID, 1.0, seed=s)) for s in (0, 1))
        keep = torch.arange(37) < NCMP
        if n == 37:
            pts, mask = torch.stack([e0, e1.flip(0)], 0), torch.stack([keep, keep.flip(0)], 0)
        else:
            pts, mask = torch.stack([e0[:n], e1[:n]], 0), torch.ones(2, n, dtype=torch.bool)
        p64 = [(net.fc[k].weight.detach().double(), net.fc[k].bias.detach().double()) for k in range(6)]
        _cache[key] = (net.to("cuda:0"), lat, pts.contiguous(), mask, p64)
    return _cache[key]


def _oracle(c, act, p64, lat, pts):
    k = ("oracle", c, act)
    if k not in _cache:
        _cache[k] = J.lig_jets(p64, act, lat.double(), pts.double(), 0., 1., second=ALL_PAIRS)      # [15, b, p, out]
    return _cache[k]


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
@pytest.mark.parametrize("d,grid,c", CASES)
def test_jets_match_oracle_on_the_hip_path(nd4, d, grid, c, act, prec, monkeypatch):
    """all four first derivatives and all ten pairs: three passes, fifteen streams"""
    from space_time_pde_amd import _lib, local_implicit_grid as lig
    monkeypatch.setattr(nd4, "mlp_precision", prec)
    net, lat, pts, mask, p64 = _setup(c, act)
    ptsd = pts.to("cuda:0")
    req = lig.JetRequest(ptsd, True, ALL_PAIRS)
    h0, g0, v0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"], lig.stats["hip_value_calls"]
    with _lib.dispatch_trace() as tr, torch.no_grad(), lig.jet_context(req):
        y = lig.query_local_implicit_grid(net, lat.to("cuda:0"), ptsd, 0., 1.)
    assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0 and lig.stats["hip_value_calls"] == v0
    assert tr.has("k_gather_nd", "D = 4") and tr.has("k_coef_nd4") and tr.has("k_reduce_nd4_jet"), tr.kernels
    assert not tr.has("k_reduce_nd<") and not tr.has("k_reduce_fwd") and not tr.has("k_reduce_nd_jet")
    assert req.y is y and req.jets.shape == (15, 3, 74) and req.pairs_out == ALL_PAIRS      # no padding visible
    assert torch.equal(y, req.jets[0].t().reshape(2, 37, 3))
    ref = _oracle(c, act, p64, lat, pts)
    got = req.jets.double().cpu().reshape(15, 3, 2, 37)
    worst = 0.0
    for s in range(15):
        want = ref[s].permute(2, 0, 1)                                # [out, b, p]
        err = (got[s] - want)[:, mask].abs().max().item() / max(want[:, mask].abs().max().item(), 1e-30)
        print("c=%d %s %s stream %d: rel err %.3e" % (c, act, prec, s, err))
        worst = max(worst, err)
        assert err < TOL, (c, act, prec, s, err)
    _record("jets c=%d %s %s: worst stream, relative to its largest magnitude" % (c, act, prec), worst)
    # exactly 0, exactly xmax, outside on both sides (rows 24 .. 27 of item 0): the clip is flat, every derivative is exactly +0
    clip = req.jets[1:, :, 24:28]
    assert torch.all(clip == 0) and not torch.signbit(clip).any()


def _gd(c, P, N, p_base):
    from space_time_pde_amd import _lib, lig_jet
    gd = _lib.GatherNdDesc()
    gd.D, gd.P, gd.N, gd.B, gd.C, gd.p_base, gd.ntiles = 4, P, N, 2, c, p_base, lig_jet.nd_tiles(P, 4)
    lo_c, hi_c, cube = lig_jet.box_constants(GRID, 0., 1.)
    for k in range(4):
        gd.n[k], gd.lo_c[k], gd.hi_c[k], gd.cube[k] = GRID[k], lo_c[k], hi_c[k], cube[k]
    return gd, (lo_c, hi_c, cube)


def _coef_on_device(hiplib, c, chunk, N, p0):
    from space_time_pde_amd import _lib
    pc = chunk.shape[0]
    gd, box = _gd(c, pc, N, p0)
    coef, chunk_d = torch.full((pc + 1, 24), 7.0, device="cuda:0"), chunk.contiguous().to("cuda:0")
    _lib.check(hiplib.stpde_lig_coef_nd4(C.byref(gd), _lib.ptr(chunk_d), _lib.ptr(coef), _lib.stream_ptr()))
    got = coef.cpu().numpy()
    assert np.all(got[pc] == 7.0)                                     # nothing written past P points
    return got[:pc], box


def test_coefficient_record_bitwise(hiplib):
    """stpde_lig_coef_nd4 against the host model on all 74 points (node points +-1 ulp included), as one chunk and as a chunk
    that starts inside batch item 0 and ends in item 1 (p_base != 0)"""
    _, _, pts, _, _ = _setup(8, "softplus")
    flat = pts.reshape(-1, 4)
    for p0, pc in ((0, 74), (29, 19)):
        chunk = flat[p0:p0 + pc]
        got, box = _coef_on_device(hiplib, 8, chunk, 37, p0)
        want, _ = JM4.coef_nd4(chunk.numpy(), GRID, *box)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _pass_desc(axis, pairs, S_mlp, S, dst):
    from space_time_pde_amd import _lib
    d = _lib.Nd4PassDesc()
    d.npairs, d.S_mlp, d.S, d.dst_value = len(pairs), S_mlp, S, dst[0]
    for k in range(3):
        d.axis[k], d.dst_first[k] = axis[k], dst[1][k]
    for k, (a, b) in enumerate(pairs):
        d.pair0[k], d.pair1[k], d.dst_pair[k] = a, b, dst[2][k]
    return d


# (triple, padded pairs in axes, S_mlp, n_out, S, partial destination map): full streams with a padded pair, six pairs and every lane
# group, a piecewise-linear activation's S_mlp = 4 < 4 + npairs, and no pairs at all with a single stream stored
REDUCE_CASES = [
    ((0, 1, 3), [(0, 3), (3, 3)], 6, 3, 8, (-1, (1, -1, 4), (6, -1))),
    ((1, 2, 3), [(1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)], 10, 16, 11, (0, (-1, 3, -1), (5, -1, 7, 8, -1, 10))),
    ((0, 2, 3), [(0, 2), (2, 2), (3, 3), (3, 3)], 4, 7, 8, (0, (1, 3, 4), (5, 6, 7, -1))),
    ((0, 1, 2), [], 4, 5, 5, (-1, (-1, -1, 3), ())),
]


@pytest.mark.parametrize("axis,pairs,S_mlp,n_out,S,dst", REDUCE_CASES)
def test_reduction_alone_against_the_model(hiplib, axis, pairs, S_mlp, n_out, S, dst):
    """stpde_lig_reduce_nd4_jet_fwd driven directly, one pass with a partial destination map: random decoder streams in the fc5
    row layout (NaN in the features >= n_out and in the padding tiles: never read), the coefficient records of the 37 edge
    points, jets with a padded leading dimension.  Written streams per element within the model's bound 4 * (number of terms)
    * 2^-24 * sum |terms|; streams mapped to -1 or not named, and rows >= P up to ldp, keep the sentinel bit for bit."""
    from space_time_pde_amd import _lib, lig_jet
    pts = M.edge_points(GRID, 1.0)
    P, ldp = 37, 40
    nt = lig_jet.nd_tiles(P, 4)
    coef, _ = JM4.coef_nd4(pts, GRID, *lig_jet.box_constants(GRID, 0., 1.))
    rng = np.random.default_rng(sum(axis) * 100 + S_mlp + n_out)
    streams = [rng.standard_normal((P * 16, n_out)) for _ in range(S_mlp)]
    out_pre = JM4.out_pre_from_streams(4, streams, nt, n_out).astype(np.float32)
    jets = torch.full((S, n_out, ldp), 7.0, device="cuda:0")
    desc = _pass_desc(axis, pairs, S_mlp, S, dst)
    out_pre_d, coef_d = torch.from_numpy(out_pre).to("cuda:0"), torch.from_numpy(coef).to("cuda:0")
    with _lib.dispatch_trace() as tr:
        _lib.check(hiplib.stpde_lig_reduce_nd4_jet_fwd(C.byref(desc), 4, P, nt, n_out, _lib.ptr(out_pre_d), _lib.ptr(coef_d),
                                                       _lib.ptr(jets), ldp, _lib.stream_ptr()))
    assert tr.has("k_reduce_nd4_jet"), tr.kernels
    got = jets.double().cpu().numpy()
    want, bound, _ = JM4.reduce_nd4_jet(P, n_out, axis, pairs, S_mlp, S, dst, out_pre.astype(np.float64), coef, ldp)
    named = sorted(s for s in (dst[0],) + tuple(dst[1]) + tuple(dst[2]) if s >= 0)
    rest = [s for s in range(S) if s not in named]
    assert np.all(got[rest] == 7.0) and np.all(got[:, :, P:] == 7.0)              # a pass touches nothing it was not given
    err = np.abs(got[named][:, :, :P] - want[named][:, :, :P])
    assert np.isfinite(want[named][:, :, :P]).all()
    worst = (err / np.maximum(bound[named][:, :, :P], 1e-300)).max()
    print("triple %s npairs=%d S_mlp=%d n_out=%d: worst err / bound %.3f" % (axis, len(pairs), S_mlp, n_out, worst))
    _record("corner sum %s npairs=%d S_mlp=%d n_out=%d: worst err / bound" % (axis, len(pairs), S_mlp, n_out), float(worst))
    assert np.all(err <= bound[named][:, :, :P])


@pytest.mark.parametrize("d,grid,c", CASES)
def test_chunking_does_not_change_a_bit(nd4, d, grid, c):
    """one chunk vs. chunks of 16 points = 16 row tiles: N = 37 spans chunks and batch items"""
    net, lat, pts, _, _ = _setup(c, "softplus")
    with torch.no_grad():
        a, pa = nd4.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, ALL_PAIRS)
        b, pb = nd4.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, ALL_PAIRS, chunk_points=16)
    assert pa == pb == ALL_PAIRS and a.shape == b.shape == (15, 3, 74)
    for s in range(15):
        assert torch.equal(a[s], b[s]), s


def test_one_point_five_points_and_none(nd4):
    for n in (1, 5):
        net, lat, pts, mask, p64 = _setup(8, "softplus", n=n)
        with torch.no_grad():
            jets, pp = nd4.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, NS_PAIRS)
        assert jets.shape == (8, 3, 2 * n) and pp == NS_PAIRS
        ref = J.lig_jets(p64, "softplus", lat.double(), pts.double(), 0., 1., second=NS_PAIRS)
        got = jets.double().cpu().reshape(8, 3, 2, n)
        for s in range(8):
            want = ref[s].permute(2, 0, 1)
            assert (got[s] - want).abs().max().item() < TOL * max(want.abs().max().item(), 1e-30), (n, s)
    with torch.no_grad():
        jets, pp = nd4.lig_jets(net, lat.to("cuda:0"), torch.zeros(2, 0, 4, device="cuda:0"), 0., 1., True, NS_PAIRS)
    assert jets.shape == (8, 3, 0) and pp == NS_PAIRS


def test_refusals_inside_lig_jets(nd4):
    """inside lig_jets an unserved request is an error, not a fall-back; outside, the composed formulation answers it"""
    from space_time_pde_amd import local_implicit_grid as lig
    net, lat, pts, _, _ = _setup(8, "softplus")
    latd, ptsd = lat.to("cuda:0").requires_grad_(True), pts.to("cuda:0")
    with pytest.raises(NotImplementedError):           # needs a gradient
        nd4.lig_jets(net, latd, ptsd, 0., 1., True, ())
    with pytest.raises(NotImplementedError), torch.no_grad():
        nd4.lig_jets(net, latd, ptsd, 0., 1., True, (), combo={(1, 1): 1.0, (2, 2): 1.0})
    with pytest.raises(ValueError), torch.no_grad():
        nd4.lig_jets(net, latd, ptsd, 0., 1., True, [(0, 4)])
    with pytest.raises(NotImplementedError), torch.no_grad():
        nd4.lig_jets(net, latd, ptsd, 0., 1., True, (), precision="bf16")
    nd4.set_nd4_jets(False)
    with pytest.raises(NotImplementedError), torch.no_grad():
        nd4.lig_jets(net, latd, ptsd, 0., 1., True, ())
    nd4.set_nd4_jets(True)
    h0, g0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"]
    with lig.jet_context(lig.JetRequest(ptsd, True, [])) as req:
        y = lig.query_local_implicit_grid(net, latd, ptsd, 0., 1.)
    assert lig.stats["generic_calls"] == g0 + 1 and lig.stats["hip_jet_calls"] == h0 and req.jets is None
    y.sum().backward()
    assert latd.grad is not None and latd.grad.abs().sum().item() > 0


def test_non_finite_inputs_stay_where_they_belong(nd4, hiplib):
    """(Run after tests/test_lig_nd4_jet_host.py::test_host_model_addresses_stay_inside_their_buffers: no such input forms an
    address outside a buffer.)  One NaN latent node of batch item 0, and in item 1 one NaN, one +inf and one 1e30 coordinate.
    The run completes.  The model says what such a coordinate is to the kernels -- clipped to the upper face with a flat clip,
    the record of a point at 2.0 there, bit for bit -- and the device agrees: the records match the model bitwise and the jets
    of those points equal, bit for bit, the jets of the run with 2.0 in their place.  The NaN node shows on every stream at
    exactly the points whose cell (the host model's = the kernel's) has it as a corner; every other point is unchanged bit
    for bit."""
    net, lat, pts, _, _ = _setup(8, "softplus")
    node = (1, 1, 0, 1)
    bad_lat = lat.clone()
    bad_lat[(0,) + node] = float("nan")
    hostile, standin = pts.clone(), pts.clone()
    for (p, k), v in {(0, 2): float("nan"), (1, 0): float("inf"), (2, 3): 1e30}.items():
        hostile[1, p, k], standin[1, p, k] = v, 2.0
    with torch.no_grad():
        clean, _ = nd4.lig_jets(net, lat.to("cuda:0"), pts.to("cuda:0"), 0., 1., True, ALL_PAIRS)
        twin, _ = nd4.lig_jets(net, bad_lat.to("cuda:0"), standin.to("cuda:0"), 0., 1., True, ALL_PAIRS)
        jets, _ = nd4.lig_jets(net, bad_lat.to("cuda:0"), hostile.to("cuda:0"), 0., 1., True, ALL_PAIRS)
    torch.cuda.synchronize()
    clean, twin, jets = clean.cpu(), twin.cpu(), jets.cpu()
    # the records of the three points: device = model, hostile = stand-in, bit for bit
    got, box = _coef_on_device(hiplib, 8, hostile[1, :3], 37, 37)
    want, _ = JM4.coef_nd4(hostile[1, :3].numpy(), GRID, *box)
    twin_rec, _ = JM4.coef_nd4(standin[1, :3].numpy(), GRID, *box)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(want.view(np.uint32), twin_rec.view(np.uint32))
    lo_c, hi_c, cube = box
    hit = torch.zeros(74, dtype=torch.bool)
    for p in range(37):                                 # batch item 0 only
        i0 = [M.geom_axis(pts[0, p, k].numpy(), lo_c[k], hi_c[k], cube[k], GRID[k])[0] for k in range(4)]
        hit[p] = all(node[k] in (i0[k], i0[k] + 1) for k in range(4))
    assert 0 < int(hit.sum()) < 37
    assert not torch.isnan(clean).any()
    assert torch.isnan(jets[:, :, hit]).all() and not torch.isnan(jets[:, :, ~hit]).any()
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    three = torch.zeros(74, dtype=torch.bool)
    three[37:40] = True
    assert same(jets[:, :, three], twin[:, :, three])                 # the hostile points: what the model says they are
    assert same(jets[:, :, ~hit & ~three], clean[:, :, ~hit & ~three])     # every other point: unchanged
    # the clipped axis of each hostile point has a flat clip: its first derivative and every pair naming it are exactly +0
    for q, k in ((37, 2), (38, 0), (39, 3)):
        streams = [1 + k] + [5 + i for i, pr in enumerate(ALL_PAIRS) if k in pr]
        assert torch.all(jets[streams, :, q] == 0) and not torch.signbit(jets[streams, :, q]).any()


# ---------------------------------------------------------------------------------------------------------------------
# PDELayer end to end
# ---------------------------------------------------------------------------------------------------------------------
NS_U = ("dif(u,t) + u*dif(u,x) + v*dif(u,y) + w*dif(u,z) + dif(p,x)"
        " - 0.01*(dif(dif(u,x),x) + dif(dif(u,y),y) + dif(dif(u,z),z))")
PROBLEMS = {
    "navier_stokes": [("xmom", NS_U), ("continuity", "dif(u,x) + dif(v,y) + dif(w,z)")],
    # names an input variable: the jets from HIP, the algebra through the lambdified functions
    "named_input": [("named", "dif(u,t) - x*dif(dif(u,z),z) + y*dif(v,y)")],
}


def _problem(name):
    """(layer of the package, residuals of the reference-semantics oracle, net, latent, pts) on the same fp32 inputs"""
    if name not in _cache:
        from space_time_pde_amd import pde
        net, lat, pts, _, _ = _setup(8, "softplus", n=NCMP, n_out=4)      # random, 0, xmax, outside on both sides
        layer, ora = pde.PDELayer("t, x, y, z", "u, v, w, p"), O.PDEOracle("t, x, y, z", "u, v, w, p")
        for eq_name, eqn in PROBLEMS[name]:
            layer.add_equation(eqn, eq_name)
            ora.add_equation(eqn, eq_name)
        p32 = [(net.fc[k].weight.detach().float().cpu(), net.fc[k].bias.detach().float().cpu()) for k in range(6)]
        ora.forward_method = lambda q: O.query_lig(lambda f: O.imnet_forward(p32, f, O.activation_fn("softplus")), lat, q, 0., 1.)
        y, res = ora(pts.clone())
        _cache[name] = (layer, y.detach(), {k: v.detach() for k, v in res.items()}, net, lat, pts)
    return _cache[name]


def _close(res, want, what):
    assert sorted(res) == sorted(want)
    for k, v in want.items():
        err = (res[k].detach().cpu() - v).abs().max().item()
        print("%s %s: residual err %.3e, |v|max %.3e" % (what, k, err, v.abs().max().item()))
        _record("residual %s %s: err / max(|v|max, 1e-3)" % (what, k), err / max(v.abs().max().item(), 1e-3))
        assert err < 1e-4 * max(v.abs().max().item(), 1e-3), (k, err)


def test_pde_layer_end_to_end(nd4, monkeypatch):
    """x-momentum with nu = 0.01 plus continuity on (t, x, y, z) -> (u, v, w, p): all four first derivatives and (x,x), (y,y),
    (z,z) in exactly two layer passes, the residuals in the device program"""
    from space_time_pde_amd import _lib, local_implicit_grid as lig
    layer, y_ref, res_ref, net, lat, pts = _problem("navier_stokes")
    latd, ptsd = lat.to("cuda:0"), pts.to("cuda:0")
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    seen = []
    real = nd4.lig_jets

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((a[5], list(a[6]), kw.get("combo"), out[0].shape[0], out[1]))
        return out

    monkeypatch.setattr(nd4, "lig_jets", spy)
    monkeypatch.setattr(nd4, "profile", {})
    h0, g0, f0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"], lig.stats["residual_torch_fallbacks"]
    with _lib.dispatch_trace() as tr, torch.no_grad():
        y, res = layer(ptsd, return_residue=True)
    assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0
    assert lig.stats["residual_torch_fallbacks"] == f0                # no input variable named: the device program
    assert tr.has("k_coef_nd4") and tr.has("k_reduce_nd4_jet") and tr.has("k_residual"), tr.kernels
    prof = nd4.profile
    assert len(prof["layer1_fwd"]) == 2 and len(prof["reduce_nd4_jet"]) == 2          # exactly two layer passes
    assert len(prof["gather_nd"]) == 1 and len(prof["coef_nd4"]) == 1                 # ... over one gather
    # second derivatives as pairs -- never as the combined stream --, eight streams, no padding visible
    assert seen == [(True, NS_PAIRS, None, 8, NS_PAIRS)], seen
    assert (y.cpu() - y_ref).abs().max().item() < TOL * y_ref.abs().max().item()
    _close(res, res_ref, "hip")
    # switch off: the same layer on the same inputs is the composed formulation under the reverse sweeps (which need grad
    # mode), counted as a generic call, within the same bound
    monkeypatch.setattr(nd4, "profile", None)
    nd4.set_nd4_jets(False)
    h0, g0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"]
    with torch.enable_grad():
        y2, res2 = layer(ptsd.clone(), return_residue=True)
    assert lig.stats["generic_calls"] == g0 + 1 and lig.stats["hip_jet_calls"] == h0 and len(seen) == 1
    _close(res2, res_ref, "composed")


def test_pde_layer_that_names_an_input_takes_the_torch_algebra(nd4):
    """the device residual evaluator addresses coordinates as [P][3]: on four inputs such a program is evaluated by the
    lambdified functions on the HIP jets, and counted"""
    from space_time_pde_amd import local_implicit_grid as lig
    layer, _, res_ref, net, lat, pts = _problem("named_input")
    latd, ptsd = lat.to("cuda:0"), pts.to("cuda:0")
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    h0, g0, f0 = lig.stats["hip_jet_calls"], lig.stats["generic_calls"], lig.stats["residual_torch_fallbacks"]
    with torch.no_grad():
        _, res = layer(ptsd, return_residue=True)
    assert lig.stats["hip_jet_calls"] == h0 + 1 and lig.stats["generic_calls"] == g0
    assert lig.stats["residual_torch_fallbacks"] == f0 + 1
    _close(res, res_ref, "named input")


def test_evaluate_lattice_equals_a_direct_call(nd4):
    from space_time_pde_amd import inference, local_implicit_grid as lig
    layer, _, _, net, lat, _ = _problem("navier_stokes")
    latd = lat.to("cuda:0")
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latd, q, 0., 1.))
    seqs = [torch.linspace(0.05, 0.95, 3), torch.linspace(0.0, 1.0, 3), torch.linspace(0.1, 0.9, 3), torch.linspace(0.2, 1.0, 3)]
    h0 = lig.stats["hip_jet_calls"]
    out = inference.evaluate_lattice(layer, latd, seqs, ("u", "v", "w", "p"))       # grad mode on outside: the jets still serve it
    assert lig.stats["hip_jet_calls"] == h0 + 1 and sorted(out) == ["continuity", "p", "u", "v", "w", "xmom"]
    batch = torch.stack(torch.meshgrid(*seqs, indexing="ij"), -1).reshape(1, 81, 4).expand(2, -1, -1).contiguous()
    with torch.no_grad():
        y, res = layer(batch.to("cuda:0"), return_residue=True)
    for k, name in enumerate(("u", "v", "w", "p")):
        assert out[name].shape == (3, 3, 3, 3) and np.array_equal(out[name], y[0, :, k].cpu().numpy().reshape(3, 3, 3, 3))
    for name in ("xmom", "continuity"):
        assert np.array_equal(out[name], res[name][0, :, 0].cpu().numpy().reshape(3, 3, 3, 3))
    h0 = lig.stats["hip_jet_calls"]
    out2 = inference.evaluate_lattice(layer, latd, seqs, ("u", "v", "w", "p"), pseudo_batch_size=32)     # 3 pseudo-batches
    assert lig.stats["hip_jet_calls"] == h0 + 3
    assert all(np.array_equal(out2[k], out[k]) for k in out)
