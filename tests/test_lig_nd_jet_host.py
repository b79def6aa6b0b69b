"""Coordinate derivatives on 1- and 2-d local implicit grids in HIP (opt-in, ``lig_jet.nd_jets``): everything that needs no
GPU -- the host model of the two new kernels (tests/lig_nd_jet_model.py) against the oracle, every address they form, the
plan's tangent constants, the dispatch decisions, the switch and the argument checks of the two new entry points."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from oracle import jet_ref as J
from space_time_pde_amd import _lib, implicit_net, lig_jet, pde
from space_time_pde_amd import local_implicit_grid as lig
from space_time_pde_amd.lig_jet import ImNetPlan, XT
from tests import lig_nd_jet_model as JM
from tests import lig_nd_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch
GRIDS = [(1, (5,), 8, 1.0), (2, (4, 5), 8, (2.0, 0.5)), (1, (5,), 34, 3.0), (2, (4, 5), 33, 1.0)]
ALL_PAIRS = {1: [(0, 0)], 2: [(0, 0), (0, 1), (1, 1)]}


def _box(dim, xmax):
    return ((0.,) * dim, xmax) if isinstance(xmax, tuple) else (0., float(xmax))


# ---------------------------------------------------------------------------------------------------------------------
# the coefficient record
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,shape,cin,xmax", GRIDS[:2])
def test_coefficient_model_matches_oracle_bitwise(dim, shape, cin, xmax):
    """coef_nd (= what k_coef_nd writes) on all 37 edge points -- exactly 0 and exactly xmax, the points outside the box and
    the nodes +-1 ulp included -- against the quantities of the oracle, evaluated by the oracle's own fp32 expressions
    (oracle/jet_ref.py lig_jets: om = |q - opposite| / cube, dom = sign(q - opposite) / cube * s, kap = s / cube; its om is
    also |rel| of cpu_ref.interp_coefficients at the corner with the other bit): the same fp32 operations, equal to the bit."""
    pts = M.edge_points(shape, xmax)
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    coef, t = JM.coef_nd(dim, pts, shape, lo_c, hi_c, cube)
    assert t["pts"] == set(range(pts.size)) and t["coef"] == set(range(pts.shape[0] * 16))
    q32 = torch.from_numpy(pts)[None]
    _, _, rel = O.interp_coefficients(torch.zeros((1,) + shape + (1,)), q32, *_box(dim, xmax))
    rel = rel[0].numpy()                                             # [P, 2^d, d]
    # the oracle's expression sequence (jet_ref.lig_jets lines "up, dn ... dom"), fp32 torch
    lo, hi = O._bounds(*_box(dim, xmax), dim, "cpu")
    eps = 1e-6 * (hi - lo)
    up, dn = hi - eps, lo + eps
    m = torch.min(q32, up)
    q = torch.max(m, dn)
    one, half, zero = torch.ones_like(q32), 0.5 * torch.ones_like(q32), torch.zeros_like(q32)
    s = torch.where(q32 < up, one, torch.where(q32 == up, half, zero)) * torch.where(m > dn, one, torch.where(m == dn, half, zero))
    cb = (hi - lo) / (torch.tensor(shape).float() - 1)
    i0f = torch.floor(q / cb)
    t0, t1 = q - (i0f + 1) * cb, q - i0f * cb                        # q - opposite position of bit 0 / bit 1
    last = (1 << dim) - 1
    for k in range(dim):
        np.testing.assert_array_equal(coef[:, k], np.abs(rel[:, last, k]))       # om[0]: distance to the bit-1 position
        np.testing.assert_array_equal(coef[:, 3 + k], np.abs(rel[:, 0, k]))      # om[1]: distance to the bit-0 position
        np.testing.assert_array_equal(coef[:, k], (torch.abs(t0) / cb)[0, :, k].numpy())
        np.testing.assert_array_equal(coef[:, 6 + k], (torch.sign(t0) / cb * s)[0, :, k].numpy())
        np.testing.assert_array_equal(coef[:, 9 + k], (torch.sign(t1) / cb * s)[0, :, k].numpy())
        np.testing.assert_array_equal(coef[:, 12 + k], (s / cb)[0, :, k].numpy())
    for k in range(dim, 3):                                          # absent axes: om = 1, dom = 0, kap = 0
        assert np.all(coef[:, [k, 3 + k]] == 1) and np.all(coef[:, [6 + k, 9 + k, 12 + k]] == 0)
    assert np.all(coef[:, 15] == 0)
    assert not np.signbit(coef[:, [6 + k for k in range(dim, 3)] + [12 + k for k in range(dim, 3)] + [15]]).any()
    # exactly 0, exactly xmax (both outside the box shrunk by 1e-6 of its size) and the two points outside (rows 24 .. 27): the
    # clip is flat, every derivative coefficient is exactly zero
    assert np.all(coef[24:28, 6:15] == 0)
    assert np.all(coef[:24, 12:12 + dim] == 1 / np.asarray(cube, np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# a whole pass in fp64 against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _dyadic_case(dim, cin, act, seed):
    """A case on which the model's fp32 geometry is EXACT, so that the fp64 oracle sees the same numbers: cell sizes that are
    powers of two (xmax = 1 or 2, 3 or 5 nodes per axis) and interior points on multiples of 2^-8 away from the nodes (cell
    index, distances, their quotients by the cell size and the products of two weights all fit fp32's 24 bits)."""
    shape, xmax = ((5,), 2.0) if dim == 1 else ((3, 5), 1.0)
    rng = np.random.default_rng(seed)
    hi = np.full(dim, xmax)
    pts = (rng.integers(1, 256, size=(11, dim)) * 2 + 1) / 512.0 * hi    # odd multiples of hi / 512: never a node
    torch.manual_seed(seed)
    net = implicit_net.ImNet(dim=dim, in_features=cin, out_features=3, nf=16, activation=act)
    latent = rng.standard_normal((1,) + shape + (cin,)).astype(np.float32)
    return shape, xmax, pts.astype(np.float32), net, latent


@pytest.mark.parametrize("npairs", ["none", "one", "all"])
@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
@pytest.mark.parametrize("dim,cin", [(1, 8), (2, 8), (2, 33)])
def test_host_model_whole_pass_matches_jet_oracle(dim, cin, act, npairs):
    """M.gather_nd -> oracle.jet_ref.mlp_jets on the gathered rows (fp64) -> the fc5-row layout -> reduce_nd_jet, against
    oracle.jet_ref.lig_jets in fp64 on the same fp32 points, per stream, to 1e-12 of max(1, the stream's largest magnitude):
    the row numbering, the slot map, the coefficient record, the corner numbering and every term of the reduction agree.
    leakyrelu: the layer buffers hold value + tangents only (S_mlp = 4 < S), the second derivatives come from the weight
    cross terms.  The tangent streams of absent axes are NaN in the model's input: loaded, never used."""
    pairs = {"none": [], "one": [(dim - 1, 0)], "all": ALL_PAIRS[dim]}[npairs]
    shape, xmax, pts, net, latent = _dyadic_case(dim, cin, {"softplus": torch.nn.Softplus, "leakyrelu": torch.nn.LeakyReLU}[act],
                                                 10 * dim + len(pairs))
    P = pts.shape[0]
    cfg_out, S, pp = lig_jet.make_cfg(act, 0.0, True, pairs)
    call = lig_jet.JetCall.make(ImNetPlan.get(dim, cin, 3, 16), act, 0.0, True, pairs, None, "fp32", shape,
                                lig_jet.box_constants(shape, 0., xmax), B=1, N=P, need_grad=False)
    assert call.S_out == S and call.S == (4 if act == "leakyrelu" else S) and call.pairs == pp
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    nt = lig_jet.nd_tiles(P, dim)
    X, _, _ = M.gather_nd(dim, pts, latent, P, 0, lo_c, hi_c, cube, nt)
    rows = X.reshape(nt, XT, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(nt * 16, XT * 16)[:P << dim]
    slot = call.plan.slot
    x = torch.from_numpy(rows[:, slot[:dim + cin]].astype(np.float64))
    p64 = [(net.fc[k].weight.detach().double(), net.fc[k].bias.detach().double()) for k in range(6)]
    second = pp if call.S == S else []
    f = [t.numpy() for t in J.mlp_jets(p64, act, x, dim, second)]
    streams = [f[0]] + [f[1 + d] if d < dim else None for d in range(3)] + f[1 + dim:]
    assert len(streams) == call.S
    out_pre = JM.out_pre_from_streams(dim, streams, nt, 3)
    coef, _ = JM.coef_nd(dim, pts, shape, lo_c, hi_c, cube)
    jets, _, _ = JM.reduce_nd_jet(dim, P, 3, cfg_out.S1, cfg_out.S2, pp, call.S, out_pre, coef)
    ref = J.lig_jets(p64, act, torch.from_numpy(latent).double(), torch.from_numpy(pts)[None].double(), *_box(dim, xmax),
                     second=pp)[:, 0].numpy()                       # [1 + dim + len(pp), P, 3]
    assert jets.shape == (S, 3, P) and np.isfinite(jets).all()
    for s in range(S):
        if 1 + dim <= s < 4:
            assert np.all(jets[s] == 0) and not np.signbit(jets[s]).any()
            continue
        want = ref[s if s <= dim else s - 4 + 1 + dim].T
        scale = max(1.0, np.abs(want).max())
        assert np.abs(jets[s] - want).max() <= 1e-12 * scale, (s, np.abs(jets[s] - want).max(), scale)


# ---------------------------------------------------------------------------------------------------------------------
# addresses
# ---------------------------------------------------------------------------------------------------------------------
def _hostile_points(shape, xmax):
    pts = M.edge_points(shape, xmax)
    d = pts.shape[1]
    bad = [np.full(d, v, np.float32) for v in (np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31)]
    one = pts[3].copy()
    one[d - 1] = np.nan
    return np.concatenate([pts, np.stack(bad + [one])], 0)


@pytest.mark.parametrize("dim,shape,cin,xmax", GRIDS[:2])
def test_host_model_addresses_stay_inside_their_buffers(dim, shape, cin, xmax):
    """Every index the two kernels form, for NaN, +-inf, +-3e38 and +-2^31 coordinates and for NaN / inf decoder rows: derived
    from P, ntiles, n_out and the (host-checked) configuration alone, so the same sets whatever the values are."""
    pts = _hostile_points(shape, xmax)
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    tp = 16 >> dim
    rng = np.random.default_rng(0)
    for pc in (pts.shape[0], 1, tp + 1):
        p = pts[-pc:]
        coef, t = JM.coef_nd(dim, p, shape, lo_c, hi_c, cube)
        assert t["pts"] == set(range(pc * dim)) and t["coef"] == set(range(pc * 16))
        assert np.isfinite(coef).all()                                # (a NaN coordinate ends on the upper face, as fminf does)
        nt = lig_jet.nd_tiles(pc, dim)
        for S1, S2, pairs, S_mlp in ((0, 0, [], 1), (3, 0, [], 4), (3, 2, [(0, 0), (dim - 1, 0)], 6), (3, 6, ALL_PAIRS[dim] * 6, 4),
                                     (3, 4, [(dim - 1, dim - 1)] * 4, 8)):
            S, ldp = 1 + S1 + S2, pc + 3
            out_pre = rng.standard_normal((nt, S_mlp, 256)).astype(np.float32)
            out_pre[0, :, ::7] = np.nan
            out_pre[-1, :, ::5] = np.inf
            jets, bound, tr = JM.reduce_nd_jet(dim, pc, 3, S1, S2, pairs[:S2], S_mlp, out_pre, coef, ldp)
            assert tr["coef"] == set(range(pc * 16))
            assert min(tr["out_pre"]) >= 0 and max(tr["out_pre"]) < out_pre.size
            want = {(s * 3 + ch) * ldp + q for s in range(S) for ch in range(3) for q in range(pc)}
            assert tr["jets"] == want and max(want) < S * 3 * ldp     # every stream of every point written once, padding untouched
            # the rows of one point lie in its own tile: the last point reads nothing past tile (pc - 1) // tp
            assert max(tr["out_pre"]) < ((pc - 1) // tp + 1) * S_mlp * 256
            if S1:
                assert np.all(jets[1 + dim:4, :, :pc] == 0)          # absent axes: +0.0 whatever the rows hold (NaN, inf)


# ---------------------------------------------------------------------------------------------------------------------
# plan: tangent constants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,cin", [(1, 8), (2, 8), (1, 34), (2, 33), (3, 8), (3, 32), (4, 8), (4, 31)])
def test_tanc_columns(dim, cin):
    """tanc of layer l = [3][MT][64][4]: block (d, mt), lane (g, j), register r holds W_s,l[16 mt + 4g + r, coordinate d] for
    d < dim and the plan's zero for d >= dim (dim = 1, 2); dim = 3 and dim = 4 hold column d of the skip block for all three d,
    index for index what they held before; sizes and offsets of every pack are what they were."""
    plan = ImNetPlan(dim, cin, 3, 16)
    zero = plan.n_theta
    lane = np.arange(64)
    g = lane >> 4
    for l, lay in enumerate(plan.layers):
        off, size = plan.pack_off[l]["tanc"]
        MT, KT = lay["MT"], lay["KT"]
        assert size == 3 * MT * 256
        names = [n for n in ("Wh", "WhT", "Ws", "WsL", "tanc") if n in plan.pack_off[l]]
        assert names[-1] == "tanc" and off == sum(plan.pack_off[l][n][1] for n in names[:-1]) + plan.pack_off[l][names[0]][0]
        idx = plan.pack_index_np[off:off + size].reshape(3, MT, 64, 4)
        for d in range(3):
            row = 16 * np.arange(MT)[:, None, None] + 4 * g[None, :, None] + np.arange(4)[None, None, :]
            if dim in (1, 2) and d >= dim:
                assert np.all(idx[d] == zero)
                continue
            # column d of the skip block of W_l (feature d sits in slot d), zero for rows past M and for fc5 (no skip block)
            want = np.where((row < lay["M"]) & lay["skip"], lay["w_off"] + row * lay["Kin"] + lay["Kh"] + d, zero)
            np.testing.assert_array_equal(idx[d], want)
    if dim in (1, 2):
        # the values: the Ws column of coordinate d, zeros otherwise
        gen = torch.Generator().manual_seed(dim)
        params = []
        for lay in plan.layers:
            params += [torch.randn(lay["M"], lay["Kin"], generator=gen), torch.randn(lay["M"], generator=gen)]
        packs = plan.pack(params)
        for l, lay in enumerate(plan.layers[:5]):
            tc = plan.pack_view(packs, l, "tanc").reshape(3, lay["MT"], 64, 4)
            # [d][mt][g][j][r] -> [d][16 mt + 4 g + r] at any j: the constant does not depend on the row j
            col = tc.reshape(3, lay["MT"], 4, 16, 4)[:, :, :, 0, :].reshape(3, -1)[:, :lay["M"]]
            for d in range(3):
                want = params[2 * l][:, lay["Kh"] + d] if d < dim else torch.zeros(lay["M"])
                assert torch.equal(col[d], want)


# ---------------------------------------------------------------------------------------------------------------------
# the switch, the call record, the dispatch decisions
# ---------------------------------------------------------------------------------------------------------------------
def test_switch_default_setter_and_record(monkeypatch):
    assert lig_jet.nd_jets is False or os.getenv("STPDE_ND_JETS")     # default off
    prev = lig_jet.set_nd_jets(True)
    try:
        assert lig_jet.nd_jets is True and lig_jet.set_nd_jets(False) is True and lig_jet.nd_jets is False
    finally:
        lig_jet.set_nd_jets(prev)
    plan = ImNetPlan.get(2, 8, 3, 16)
    box = lig_jet.box_constants((4, 5), 0., 1.)
    for on in (False, True):
        monkeypatch.setattr(lig_jet, "nd_jets", on)
        call = lig_jet.JetCall.make(plan, "softplus", 0.0, True, [(0, 0), (1, 1)], None, "fp32", (4, 5), box, B=2, N=37,
                                    need_grad=False)
        monkeypatch.setattr(lig_jet, "nd_jets", not on)               # frozen when the call was made
        assert call.nd_jets is on
        assert (call.cfg.S1, call.cfg.S2, call.S, call.mult, call.pipeline, call.P_pad) == (3, 2, 6, 16, False, 74)
    # the memory plan counts every stream of the request: 6 streams of layer buffers against 1
    v = lig_jet.JetCall.make(plan, "softplus", 0.0, False, [], None, "fp32", (4, 5), box, B=2, N=37, need_grad=False)
    assert lig_jet._buf_floats(call, 1, 4) == 6 * lig_jet._buf_floats(v, 1, 4)
    assert lig_jet._per_point_bytes(call)[0] > 3 * lig_jet._per_point_bytes(v)[0]


def test_switch_default_comes_from_the_environment():
    code = "from space_time_pde_amd import lig_jet; print(int(lig_jet.nd_jets))"
    for val, want in ((None, "0"), ("1", "1"), ("0", "0"), ("off", "0"), ("true", "1")):
        env = {k: v for k, v in os.environ.items() if k != "STPDE_ND_JETS"}
        if val is not None:
            env["STPDE_ND_JETS"] = val
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want, (val, out.stdout, out.stderr)


class _T:
    """Stand-in for a CUDA tensor: the decisions read shapes and flags only."""

    def __init__(self, shape, cuda=True, dtype=torch.float32, requires_grad=False):
        self.shape, self.is_cuda, self.dtype, self.requires_grad = tuple(shape), cuda, dtype, requires_grad

    def dim(self):
        return len(self.shape)


def _case(dim, cin, nf=16, grid=None, **kw):
    net = implicit_net.ImNet(dim=dim, in_features=cin, out_features=3, nf=nf, activation=torch.nn.Softplus)
    grid = grid or (3,) * dim
    return net, _T((2,) + tuple(grid) + (cin,), **kw), _T((2, 37, dim))


def test_eligibility_table(monkeypatch):
    monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
    R = lig.JetRequest

    def ok(net, lat, pts, first=True, pairs=(), combo=None, req_pts=None):
        return lig._nd_jet_eligible(net, lat, pts, R(pts if req_pts is None else req_pts, first, pairs, combo))

    with torch.no_grad():
        monkeypatch.setattr(lig_jet, "nd_jets", False)
        assert not ok(*_case(2, 8))                                   # off: nothing is eligible
        monkeypatch.setattr(lig_jet, "nd_jets", True)
        assert ok(*_case(1, 8)) and ok(*_case(2, 8)) and ok(*_case(1, 34)) and ok(*_case(2, 33))
        assert ok(*_case(2, 8), pairs=[(0, 0), (0, 1), (1, 1)]) and ok(*_case(1, 8), pairs=[(0, 0)])
        assert ok(*_case(2, 8), first=False)                          # a request for the value alone
        assert not ok(*_case(4, 8)) and not ok(*_case(3, 8))          # three tangent streams; dim = 3 has its own dispatch
        assert not ok(*_case(1, 35)) and not ok(*_case(2, 34))        # one feature too many
        assert not ok(*_case(2, 8), pairs=[(1, 2)]) and not ok(*_case(1, 8), pairs=[(0, 1)])     # an axis the grid lacks
        assert not ok(*_case(2, 8), combo={(0, 0): 1.0, (1, 1): 1.0})
        assert not ok(*_case(2, 8, nf=4)) and not ok(*_case(2, 8, grid=(4, 1)))
        assert not ok(*_case(2, 8, cuda=False)) and not ok(*_case(2, 8, dtype=torch.float64))
        net, lat, pts = _case(2, 8)
        assert not lig._nd_jet_eligible(net, lat, pts, None)          # no request
        assert not ok(net, lat, pts, req_pts=_T((2, 37, 2)))          # a request for other points
        assert not ok(torch.nn.Linear(10, 3), lat, pts)
        for prec, want in (("fp32x3", True), ("bf16", False)):
            monkeypatch.setattr(lig_jet, "mlp_precision", prec)
            assert ok(net, lat, pts) is want
        monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
        # the value path keeps refusing points under a jet request, switch on or off
        assert not lig._nd_value_eligible(net, lat, pts, R(pts, True, []))
    # grad mode on: the parameters of a fresh ImNet require grad -> composed
    net, lat, pts = _case(2, 8)
    assert not ok(net, lat, pts)
    for p in net.parameters():
        p.requires_grad_(False)
    assert ok(net, lat, pts)
    assert not ok(net, _T(lat.shape, requires_grad=True), pts)
    pg = _T(pts.shape, requires_grad=True)
    assert not ok(net, lat, pg)
    with torch.no_grad():
        assert ok(net, _T(lat.shape, requires_grad=True), pts)


class _CudaLike(torch.Tensor):
    """A CPU tensor that says it is a CUDA tensor: _jet_request reads the flag, the shape and requires_grad only."""
    is_cuda = property(lambda self: True)


def test_jet_request_for_two_inputs(monkeypatch):
    layer = pde.PDELayer("x, y", "u, v")
    layer.add_equation("dif(dif(u,x),x) + dif(dif(u,y),y) - v", "poisson")
    x = torch.zeros(2, 5, 2).as_subclass(_CudaLike)
    assert x.is_cuda and torch.is_tensor(x)
    monkeypatch.setattr(lig_jet, "nd_jets", False)
    with torch.no_grad():
        assert layer._jet_request(x) is None                          # switch off: the reverse sweeps, as before
    monkeypatch.setattr(lig_jet, "nd_jets", True)
    assert layer._jet_request(x) is None                              # grad mode on: no request (no forward evaluated twice)
    with torch.no_grad():
        req = layer._jet_request(x)
        assert req is not None and req.x is x and req.first and req.combo is None
        assert req.pairs == [(0, 0), (1, 1)]                          # a Laplacian goes as pairs, never as a combined stream
        assert layer._jet_request(torch.zeros(2, 5, 2)) is None       # CPU tensor
        burgers = pde.PDELayer("t, x", "u")
        burgers.add_equation("dif(u,t) + u*dif(u,x) - 0.01*dif(dif(u,x),x)", "burgers")
        req = burgers._jet_request(x)
        assert req.first and req.pairs == [(1, 1)] and req.combo is None
        one = pde.PDELayer("x", "u")
        one.add_equation("dif(dif(u,x),x) - u", "ode")
        assert one._jet_request(torch.zeros(2, 5, 1).as_subclass(_CudaLike)).pairs == [(0, 0)]
    # n_in == 3 is untouched: the combined stream, whatever the switch and the grad mode say
    rb = pde.PDELayer("t, x, z", "u")
    rb.add_equation("dif(u,t) - dif(dif(u,x),x) - 0.25*dif(dif(u,z),z)", "heat")
    x3 = torch.zeros(2, 5, 3).as_subclass(_CudaLike)
    for on in (False, True):
        monkeypatch.setattr(lig_jet, "nd_jets", on)
        assert rb._jet_request(x3).combo == {(1, 1): 1.0, (2, 2): 0.25}


def test_lig_jets_refuses_cpu_tensors_whatever_the_switch(monkeypatch):
    monkeypatch.setattr(lig_jet, "nd_jets", True)
    net = implicit_net.ImNet(dim=2, in_features=8, out_features=3, nf=16)
    with pytest.raises(RuntimeError), torch.no_grad():
        lig_jet.lig_jets(net, torch.rand(1, 4, 5, 8), torch.rand(1, 5, 2), 0., 1., True, ())


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_and_the_abi_version_stays(hiplib):
    for name in ("stpde_lig_coef_nd", "stpde_lig_reduce_nd_jet_fwd"):
        assert name in _lib.exported_symbols() and hasattr(hiplib, name)
    assert _lib.ABI_VERSION == 316 and hiplib.stpde_version() == 316


def _gd(D=2, P=37, N=37, B=2, C=8, p_base=0, ntiles=None, n=(4, 5, 0, 0)):
    d = _lib.GatherNdDesc()
    d.D, d.P, d.N, d.B, d.C, d.p_base = D, P, N, B, C, p_base
    d.ntiles = lig_jet.nd_tiles(P, min(max(D, 1), 4)) if ntiles is None else ntiles
    for k in range(4):
        d.n[k], d.lo_c[k], d.hi_c[k], d.cube[k] = n[k], 1e-6, 1 - 1e-6, 0.25
    return d


@pytest.mark.parametrize("why,kw", [
    ("D = 4", dict(D=4, n=(3, 4, 2, 3))), ("D = 3", dict(D=3, n=(4, 5, 3, 0))), ("D = 0", dict(D=0)),
    ("do not fit", dict(P=0)), ("do not fit", dict(P=37, ntiles=9)), ("axis 1", dict(n=(4, 1, 0, 0))),
    ("37 features", dict(C=34)), ("p_base", dict(p_base=-1)), ("p_base", dict(N=0)),
])
def test_coef_nd_refuses_bad_arguments(hiplib, why, kw):
    d = _gd(**kw)
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_coef_nd(ctypes.byref(d), FAKE, FAKE, None))
    assert "lig_coef_nd" in str(e.value) and why in str(e.value), str(e.value)


def test_coef_nd_refuses_null_pointers(hiplib):
    d = _gd()
    for args in ((None, FAKE), (FAKE, None)):
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_coef_nd(ctypes.byref(d), *args, None))
        assert "null pointer" in str(e.value)
    with pytest.raises(ValueError):
        _lib.check(hiplib.stpde_lig_coef_nd(None, FAKE, FAKE, None))


def _cfg(S1=3, S2=2, pairs=((0, 0), (1, 1)), combo=0):
    c = _lib.JetCfg()
    c.S1, c.S2, c.combo = S1, S2, combo
    for k, (a, b) in enumerate(pairs):
        c.pair0[k], c.pair1[k] = a, b
    return c


# (why, cfg arguments, (S_mlp, D, P, ntiles, n_out, ldp))
GOOD = (6, 2, 37, 12, 3, 37)
REFUSALS = [
    ("D = 4", {}, (6, 4, 5, 8, 3, 5)), ("D = 3", {}, (6, 3, 8, 4, 3, 8)), ("D = 0", {}, (6, 0, 8, 4, 3, 8)),
    ("do not fit", {}, (6, 2, 37, 9, 3, 37)),                          # P > ntiles * TP
    ("do not fit", {}, (6, 2, 37, 16, 3, 37)), ("do not fit", {}, (6, 1, 0, 4, 3, 8)),
    ("n_out", {}, (6, 2, 37, 12, 0, 37)), ("n_out", {}, (6, 2, 37, 12, 17, 37)),
    ("ldp", {}, (6, 2, 37, 12, 3, 36)),
    ("stream set", dict(S1=1, S2=0, pairs=()), (2, 2, 37, 12, 3, 37)), ("stream set", dict(S1=2), GOOD),
    ("stream set", dict(S2=1, pairs=((0, 0),)), (5, 2, 37, 12, 3, 37)), ("stream set", dict(S2=3), GOOD),
    ("stream set", dict(S2=5), GOOD), ("stream set", dict(S2=7), GOOD), ("stream set", dict(S2=-1), GOOD),
    ("stream set", dict(S1=0, S2=2), (1, 2, 37, 12, 3, 37)),
    ("combined", dict(combo=1), GOOD),
    ("pair 1", dict(pairs=((0, 0), (1, 2))), GOOD), ("pair 0", dict(pairs=((2, 2), (1, 1))), GOOD),
    ("pair 0", dict(pairs=((-1, 0), (1, 1))), GOOD), ("pair 1", dict(pairs=((0, 0), (0, 1))), (6, 1, 37, 8, 3, 37)),
    ("S_mlp", {}, (0, 2, 37, 12, 3, 37)), ("S_mlp", {}, (7, 2, 37, 12, 3, 37)),
    ("S_mlp", dict(S1=0, S2=0, pairs=()), (2, 2, 37, 12, 3, 37)),
]


@pytest.mark.parametrize("why,ckw,args", REFUSALS)
def test_reduce_nd_jet_refuses_bad_arguments(hiplib, why, ckw, args):
    S_mlp, D, P, nt, n_out, ldp = args
    cfg = _cfg(**ckw)
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_reduce_nd_jet_fwd(ctypes.byref(cfg), S_mlp, D, P, nt, n_out, FAKE, FAKE, FAKE, ldp, None))
    assert "lig_reduce_nd_jet_fwd" in str(e.value) and why in str(e.value), str(e.value)


def test_reduce_nd_jet_refuses_null_pointers(hiplib):
    cfg = _cfg()
    S_mlp, D, P, nt, n_out, ldp = GOOD
    for k in range(3):
        ptrs = [FAKE] * 3
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_reduce_nd_jet_fwd(ctypes.byref(cfg), S_mlp, D, P, nt, n_out, *ptrs, ldp, None))
        assert "null pointer" in str(e.value)
    with pytest.raises(ValueError):
        _lib.check(hiplib.stpde_lig_reduce_nd_jet_fwd(None, S_mlp, D, P, nt, n_out, FAKE, FAKE, FAKE, ldp, None))
