"""Training backward of the HIP path for 1-, 2- and 4-d local implicit grids: everything that needs no GPU -- a host model
of every address the three new kernels form (tests/lig_nd_bwd_model.py) on hostile points, the model's node / corner / row
bookkeeping against the oracle's autograd, the opt-in switch and the eligibility decision, and the argument checks of the
three new entry points."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from space_time_pde_amd import _lib, implicit_net, lig_jet, nonlinearities
from space_time_pde_amd import local_implicit_grid as lig
from tests import lig_nd_bwd_model as MB
from tests import lig_nd_model as M

FAKE = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch
GRIDS = [(1, (5,), 8, 1.0), (2, (4, 5), 8, (2.0, 0.5)), (4, (3, 4, 2, 3), 8, (2.0, 1.0, 4.0, 0.5)),
         (4, (3, 4, 2, 3), 31, 1.0), (1, (9,), 32, 3.0)]


def _box(dim, xmax):
    return ((0.,) * dim, xmax) if isinstance(xmax, tuple) else (0., float(xmax))


def _hostile_points(shape, xmax):
    """the 37 edge points plus what no caller should send: NaN, +-inf, +-huge, on every axis and on one axis only"""
    pts = M.edge_points(shape, xmax)
    d = pts.shape[1]
    bad = [np.full(d, v, np.float32) for v in (np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31)]
    one = pts[3].copy()
    one[d - 1] = np.nan
    return np.concatenate([pts, np.stack(bad + [one])], 0)


# ---------------------------------------------------------------------------------------------------------------------
# host model of the addresses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,shape,cin,xmax", GRIDS + M.D3_GRIDS)
def test_host_model_addresses_stay_inside_their_buffers(dim, shape, cin, xmax):
    """dim = 3 (k_dlat_reduce and the cell stpde_lig_gather writes are the same bodies at D = 3): that entry point takes an
    even P and ntiles = P / 2, so the chunk lengths are rounded up to even there"""
    B, n_out = 2, 3
    pts1 = _hostile_points(shape, xmax)
    N = pts1.shape[0]
    pts = np.concatenate([pts1, pts1[::-1]], 0)                      # [B * N, d]
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    tp, nc = 16 >> dim, 1 << dim
    cp = (cin + 3) // 4 * 4
    n_nodes = B * int(np.prod(shape))
    rng = np.random.default_rng(4)
    # one chunk; chunks that end inside a tile / inside a batch item (P no multiple of the tile's point count; the last one
    # starts past B * N on purpose: the batch index must clamp); ntiles at ceil + 0 and ceil + 3
    for p0, pc in ((0, B * N), (0, 1), (N - 3, tp + 1), (B * N - 2, 2), (B * N + 5, 3)):
        pc += pc & 1 if dim == 3 else 0
        pc_pts = np.resize(pts[p0:p0 + pc], (pc, dim)) if p0 < B * N else pts[:pc]
        cell, t = MB.cell_nd(dim, pc_pts, shape, B, N, p0, lo_c, hi_c, cube)
        assert t["pts"] == set(range(pc * dim)) and t["cell"] == set(range(pc))
        assert cell.min() >= 0 and cell.max() < n_nodes
        # the cell is a corner-0 node: every axis index <= n_k - 2, so every corner of it is a node of the grid
        idx = np.unravel_index(cell, (B,) + shape)
        assert all((idx[1 + k] <= shape[k] - 2).all() for k in range(dim))
        perm, start = MB.cell_sort(cell, n_nodes)
        assert start.shape == (n_nodes + 1,) and start[-1] == pc and sorted(perm.tolist()) == list(range(pc))
        need = -(-pc // tp)
        for nt in ((need,) if dim == 3 else (need, need + 3)):
            ldp = pc + 5
            ybar = rng.standard_normal((n_out, ldp)).astype(np.float32)
            ybar[:, pc:] = np.nan                                     # beyond the chunk: must not be read
            cw = rng.random(nt * 16).astype(np.float32)
            cw[pc * nc:] = np.nan                                     # (the gather writes 0 there; the adjoint must not need it)
            abar, t = MB.reduce_nd_bwd(dim, pc, nt, n_out, ybar, cw)
            assert t["abar"] == set(range(nt * 256))                  # every float of all ntiles blocks is written
            assert t["cw"] == set(range(pc * nc))
            assert t["ybar"] == {ch * ldp + p for ch in range(n_out) for p in range(pc)}
            rows = abar.reshape(nt, 4, 16, 4).transpose(0, 2, 1, 3).reshape(nt * 16, 16)     # [row][feature 4g + r]
            assert np.isfinite(rows).all()
            assert np.all(rows[pc * nc:] == 0) and np.all(rows[:, n_out:] == 0)
            want = cw[:pc * nc, None] * np.repeat(ybar[:, :pc].T, nc, 0)
            np.testing.assert_array_equal(rows[:pc * nc, :n_out], want)
            # xrows of a chunk: 16 * ntiles rows of CP floats (k_xbar writes the padding rows too)
            xrows = rng.standard_normal((16 * nt, cp)).astype(np.float32)
            xrows[pc * nc:] = np.nan                                  # padding rows belong to no point: never summed
            dlat = np.zeros((n_nodes, cin), np.float32)
            t = MB.dlatent_reduce_nd(dim, B, shape, cin, xrows, perm, start, dlat)
            assert max(t["xrows"]) < pc * nc * cp <= 16 * nt * cp and min(t["xrows"]) >= 0
            assert max(t["perm"]) < pc and max(t["start"]) <= n_nodes
            assert max(t["dlatent"]) < n_nodes * cin
            assert np.isfinite(dlat).all()
            # every live row lands on exactly one node: the sums agree
            np.testing.assert_allclose(dlat.sum(0), xrows[:pc * nc, :cin].sum(0), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("dim,shape,cin,xmax", GRIDS)
def test_model_cell_equals_the_oracles_floor_bitwise(dim, shape, cin, xmax):
    """A latent grid whose only channel holds each node's own linear index (exact in fp32) makes the oracle report, as corner
    value 0, the node floor(q / cube) picked: the model's cell (= the kernel's expression sequence) must be that node."""
    B = 2
    pts = np.stack([M.edge_points(shape, xmax, seed=0), M.edge_points(shape, xmax, seed=1)[::-1]], 0)
    N = pts.shape[1]
    n_nodes = B * int(np.prod(shape))
    ids = torch.arange(n_nodes, dtype=torch.float32).reshape((B,) + shape + (1,))
    v, _, _ = O.interp_coefficients(ids, torch.from_numpy(pts.copy()), *_box(dim, xmax))
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    cell, _ = MB.cell_nd(dim, pts.reshape(B * N, dim), shape, B, N, 0, lo_c, hi_c, cube)
    np.testing.assert_array_equal(cell, v[:, :, 0, 0].reshape(-1).numpy().astype(np.int32))
    # chunked, with p_base inside batch item 1: the same ids
    c2, _ = MB.cell_nd(dim, pts.reshape(B * N, dim)[N + 3:], shape, B, N, N + 3, lo_c, hi_c, cube)
    np.testing.assert_array_equal(c2, cell[N + 3:])


@pytest.mark.parametrize("dim,shape,cin,xmax", GRIDS)
def test_model_dlatent_equals_oracle_autograd(dim, shape, cin, xmax):
    """cell_nd -> cell_sort -> dlatent_reduce_nd on the ORACLE's own per-row adjoints (the gradient of its decoder input,
    latent columns, row = point * 2^d + corner) against the oracle's d latent, fp64, geometry in fp32 on both sides: the
    node / corner / row bookkeeping.  Only the order of an fp64 sum differs: 1e-12."""
    B, n_out = 2, 3
    pts = np.stack([M.edge_points(shape, xmax, seed=0), M.edge_points(shape, xmax, seed=1)[::-1]], 0)
    if cin == 32:
        pts = pts * np.float32(0.5)                      # first half of the box: some nodes receive no point
    N = pts.shape[1]
    P, nc, cp = B * N, 1 << dim, (cin + 3) // 4 * 4
    g = torch.Generator().manual_seed(5)
    lat = torch.randn((B,) + shape + (cin,), generator=g, dtype=torch.float64).requires_grad_(True)
    p64 = O.imnet_init(dim, cin, n_out, 16, seed=3, dtype=torch.float64)
    seen = []

    def dec(f):
        f.retain_grad()
        seen.append(f)
        return O.imnet_forward(p64, f, O.activation_fn("softplus"))

    y = O.query_lig(dec, lat, torch.from_numpy(pts.copy()), *_box(dim, xmax))
    cot = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * cot).sum().backward()
    rowbar = seen[0].grad[:, dim:].numpy()               # [P * 2^d, c]
    lo_c, hi_c, cube = lig_jet.box_constants(shape, 0., xmax)
    n_nodes = B * int(np.prod(shape))
    got = np.zeros((n_nodes, cin))
    # two chunks, the second one starting inside a tile and inside batch item 0
    for p0, pc in ((0, N - 5), (N - 5, P - N + 5)):
        nt = lig_jet.nd_tiles(pc, dim)
        xrows = np.full((16 * nt, cp), np.nan)
        xrows[:pc * nc] = 0
        xrows[:pc * nc, :cin] = rowbar[p0 * nc:(p0 + pc) * nc]
        cell, _ = MB.cell_nd(dim, pts.reshape(P, dim)[p0:p0 + pc], shape, B, N, p0, lo_c, hi_c, cube)
        perm, start = MB.cell_sort(cell, n_nodes)
        MB.dlatent_reduce_nd(dim, B, shape, cin, xrows, perm, start, got)
    want = lat.grad.reshape(n_nodes, cin).numpy()
    if cin == 32:
        assert (np.abs(want).max(1) == 0).any()          # nodes no point touches stay exactly zero
        assert np.all(got[np.abs(want).max(1) == 0] == 0)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("d,grid,c,act", [cs + (a,) for cs in MB.TRAIN_CASES for a in ("softplus", "leakyrelu")]
                         + [(2, (4, 5), 8, "swish")])
def test_bounds_have_margin_on_the_gpu_tests_inputs(d, grid, c, act):
    """The GPU parity test (tests/test_gpu_lig_nd_backward.py) holds the HIP path to 2e-5 (y) / 2e-4 (gradients) of the fp64
    oracle.  On the exact inputs it uses, the fp32 oracle against the fp64 oracle must stay under a QUARTER of each bound:
    then no edge point (a node +-1 ulp, where fp32 and fp64 may pick different cells) eats the bound by itself.
    Measured (fp32 vs fp64 oracle, relative to the max magnitude): y <= 2.7e-7; d latent <= 2.3e-7; parameter gradients
    <= 1.2e-6; swish beta 1.8e-7.  One RANDOM point had to be replaced -- point 22 of (4, (3, 4, 2, 3), 31) with LeakyReLU, which
    sits on the activation's kink (parameter-gradient gap 2.4e-3 with it; tests/lig_nd_bwd_model.py, train_case)."""
    for n in (37, 1, (16 >> d) + 1):
        if n != 37 and (act != "softplus" or c != 8):
            continue
        case = MB.train_case(d, grid, c, act, n=n)
        y32, l32, p32, b32 = MB.oracle_grads(case, torch.float32)
        y64, l64, p64, b64 = MB.oracle_grads(case, torch.float64)
        gaps = [MB.relerr(y32, y64), MB.relerr(l32, l64), max(MB.relerr(a, b) for a, b in zip(p32, p64))]
        if b64 is not None:
            gaps.append(MB.relerr(b32, b64))
        print("d=%d c=%d %s n=%d: y %.2e dlat %.2e dprm %.2e%s" % ((d, c, act, n) + tuple(gaps[:3]) +
                                                                  ((" dbeta %.2e" % gaps[3],) if b64 is not None else ("",))))
        assert gaps[0] < MB.TOL_Y / 4
        assert all(g < MB.TOL_G / 4 for g in gaps[1:])


def test_model_reduce_nd_bwd_is_the_adjoint_of_reduce_nd():
    """<reduce_nd(out), ybar> == <out, reduce_nd_bwd(ybar)> over the live rows and features, fp64"""
    rng = np.random.default_rng(6)
    for dim in (1, 2, 4):
        P, n_out = 37, 3
        nt = lig_jet.nd_tiles(P, dim)
        out = rng.standard_normal((nt, 64, 4))
        cw = rng.random(nt * 16)
        cw[P << dim:] = 0
        ybar = rng.standard_normal((n_out, P))
        y, _ = M.reduce_nd(dim, P, n_out, out, cw)
        abar, _ = MB.reduce_nd_bwd(dim, P, nt, n_out, ybar, cw)
        np.testing.assert_allclose((y * ybar).sum(), (out * abar).sum(), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# the switch and the eligibility decision
# ---------------------------------------------------------------------------------------------------------------------
class _T:
    """Stand-in for a CUDA tensor: the decision reads shapes and flags only."""

    def __init__(self, shape, cuda=True, dtype=torch.float32, requires_grad=False):
        self.shape, self.is_cuda, self.dtype, self.requires_grad = tuple(shape), cuda, dtype, requires_grad

    def dim(self):
        return len(self.shape)


def _case(dim, cin, nf=16, grid=None, act=torch.nn.Softplus, lat_grad=False, pts_grad=False, param_grad=True, **kw):
    net = implicit_net.ImNet(dim=dim, in_features=cin, out_features=3, nf=nf, activation=act)
    for p in net.parameters():
        p.requires_grad_(param_grad)
    grid = grid or (3,) * dim
    return net, _T((2,) + tuple(grid) + (cin,), requires_grad=lat_grad, **kw), _T((2, 37, dim), requires_grad=pts_grad)


def _route(case, req=None):
    """what query_local_implicit_grid does with the case: "hip" or "composed" """
    return "hip" if (lig._nd_value_eligible(*case, req) or lig._nd_train_eligible(*case, req)) else "composed"


def test_switch_is_off_by_default_and_set_returns_the_previous_value(monkeypatch):
    monkeypatch.setattr(lig_jet, "nd_backward", False)
    assert lig_jet.set_nd_backward(True) is False and lig_jet.nd_backward is True
    assert lig_jet.set_nd_backward(0) is True and lig_jet.nd_backward is False


@pytest.mark.parametrize("value,want", [(None, False), ("", False), ("0", False), ("1", True)])
def test_switch_default_comes_from_the_environment(value, want):
    env = {k: v for k, v in os.environ.items() if k != "STPDE_ND_BACKWARD"}
    if value is not None:
        env["STPDE_ND_BACKWARD"] = value
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "from space_time_pde_amd import lig_jet; print(lig_jet.nd_backward)"],
                         cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == str(want)


def test_eligibility_table_switch_off_is_todays_answer(monkeypatch):
    monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
    monkeypatch.setattr(lig_jet, "nd_backward", False)
    for dim in (1, 2, 4):
        for kw in (dict(), dict(lat_grad=True), dict(param_grad=False), dict(param_grad=False, lat_grad=True),
                   dict(param_grad=False, pts_grad=True)):
            case = _case(dim, 8, **kw)
            assert not lig._nd_train_eligible(*case)
            assert _route(case) == ("hip" if lig._nd_value_eligible(*case) else "composed")
        assert _route(_case(dim, 8)) == "composed"                              # parameters require grad
        assert _route(_case(dim, 8, param_grad=False)) == "hip"                 # nothing does: the value path
        assert _route(_case(dim, 8, param_grad=False, lat_grad=True)) == "composed"
        with torch.no_grad():
            assert _route(_case(dim, 8, lat_grad=True)) == "hip"


def test_eligibility_table_switch_on(monkeypatch):
    monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
    monkeypatch.setattr(lig_jet, "nd_backward", True)
    for dim, cmax in ((1, 32), (2, 32), (4, 31)):
        assert lig._nd_train_eligible(*_case(dim, 8))                           # parameters
        assert lig._nd_train_eligible(*_case(dim, 8, param_grad=False, lat_grad=True))       # latent grid only
        assert lig._nd_train_eligible(*_case(dim, cmax, lat_grad=True))         # widest trainable latent
        assert not lig._nd_train_eligible(*_case(dim, 8, param_grad=False))     # nothing requires grad: the value path
        assert _route(_case(dim, 8, param_grad=False)) == "hip"
        with torch.no_grad():                                                   # no backward can follow: the value path
            assert not lig._nd_train_eligible(*_case(dim, 8, lat_grad=True))
            assert _route(_case(dim, 8, lat_grad=True)) == "hip"
        # point gradients: composed, whatever else requires grad
        assert _route(_case(dim, 8, pts_grad=True)) == "composed"
        assert _route(_case(dim, 8, param_grad=False, pts_grad=True)) == "composed"
    # k_xbar<XL> exists for XL = 1, 2: c = 33, 34 (d = 1) and c = 33 (d = 2) evaluate in HIP but train composed
    for dim, c in ((1, 33), (1, 34), (2, 33)):
        assert _route(_case(dim, c)) == "composed"
        assert _route(_case(dim, c, param_grad=False)) == "hip"
    assert _route(_case(4, 32)) == "composed"                                   # 37 features: not even the value path
    # a learnable swish beta alone
    case = _case(2, 8, act=nonlinearities.Swish, param_grad=False)
    assert not lig._nd_train_eligible(*case)
    case[0].activ.beta.requires_grad_(True)
    assert lig._nd_train_eligible(*case)
    # a jet request for THESE points: composed; for other points: no obstacle
    net, lat, pts = _case(2, 8)
    assert _route((net, lat, pts), lig.JetRequest(pts, True, [])) == "composed"
    assert _route((net, lat, pts), lig.JetRequest(_T((2, 37, 2)), True, [])) == "hip"
    # operand modes
    for prec, want in (("fp32x3", "hip"), ("bf16", "composed")):
        monkeypatch.setattr(lig_jet, "mlp_precision", prec)
        assert _route((net, lat, pts)) == want
    monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
    # everything else _nd_value_eligible refuses stays refused
    assert _route(_case(2, 8, nf=4)) == "composed"
    assert _route(_case(3, 8)) == "composed"
    assert _route(_case(2, 8, grid=(4, 1))) == "composed"
    assert _route(_case(2, 8, cuda=False)) == "composed"
    assert _route(_case(2, 8, dtype=torch.float64)) == "composed"
    assert _route((torch.nn.Linear(10, 3), lat, pts)) == "composed"
    assert _route((torch.nn.DataParallel(net), lat, pts)) == "composed"       # a wrapper that reaches the decision: not an ImNet
    assert _route(_case(2, 8, act=torch.nn.Identity)) == "composed"


def test_cpu_training_query_keeps_the_composed_formulation(monkeypatch):
    monkeypatch.setattr(lig_jet, "nd_backward", True)
    net = implicit_net.ImNet(dim=2, in_features=8, out_features=3, nf=16)
    lat = torch.rand(2, 4, 5, 8, requires_grad=True)
    n0, h0 = lig.stats["generic_calls"], lig.stats["hip_value_calls"]
    y = lig.query_local_implicit_grid(net, lat, torch.rand(2, 37, 2), 0., 1.)
    y.sum().backward()
    assert lat.grad is not None and lig.stats["generic_calls"] == n0 + 1 and lig.stats["hip_value_calls"] == h0


def test_memory_plan_counts_rows_per_point():
    """stash / scratch bytes per point scale with the 2^d rows a point owns (dim = 3: 8 rows, unchanged)"""
    per = {}
    for dim in (1, 2, 3, 4):
        grid = (4,) * dim
        meta = lig_jet.JetCall.make(lig_jet.ImNetPlan.get(dim, 8, 3, 16), "softplus", 0.0, False, [], None, "fp32", grid,
                                    lig_jet.box_constants(grid, 0., 1.))
        assert (meta.S, meta.packed_mask) == (1, 0)
        per[dim] = lig_jet._per_point_bytes(meta)
        rows = 1 << dim
        mt = [lay["MT"] for lay in meta.plan.layers]
        tile_fwd = 4 * 256 * (sum(mt[1:]) + mt[0] + 3)
        assert abs(per[dim][0] - tile_fwd * rows / 16) <= 4 * 16 + 4
    assert per[1][0] < per[2][0] < per[3][0] < per[4][0] and per[1][1] < per[2][1] < per[3][1] < per[4][1]


# ---------------------------------------------------------------------------------------------------------------------
# the three entry points: presence, prototypes, refusals (fake pointers: refused before any launch)
# ---------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_descriptor():
    sig = _lib._SIGNATURES
    VP, I = ctypes.c_void_p, ctypes.c_int
    assert sig["stpde_lig_reduce_nd_bwd"] == ([I, I, I, I, VP, ctypes.c_long, VP, VP, VP], I)
    assert sig["stpde_lig_cell_nd"] == ([ctypes.POINTER(_lib.GatherNdDesc), VP, VP, VP], I)
    assert sig["stpde_lig_dlatent_reduce_nd"] == ([I, I, ctypes.POINTER(I), I, VP, VP, VP, VP, VP], I)
    assert ctypes.sizeof(_lib.GatherNdDesc) == 4 * (7 + 4 * 4)      # the descriptor of the gather, unchanged
    assert _lib.ABI_VERSION == 316                                  # additive symbols: the ABI version stays
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "stpde_hip.h")).read()
    for name in ("stpde_lig_reduce_nd_bwd", "stpde_lig_cell_nd", "stpde_lig_dlatent_reduce_nd"):
        assert "int %s(" % name in header


def test_library_exports_the_entry_points(hiplib):
    for name in ("stpde_lig_reduce_nd_bwd", "stpde_lig_cell_nd", "stpde_lig_dlatent_reduce_nd"):
        assert getattr(hiplib, name).restype is ctypes.c_int


def _gd(D=2, P=37, N=37, B=2, C=8, p_base=0, ntiles=None, n=(4, 5, 0, 0)):
    d = _lib.GatherNdDesc()
    d.D, d.P, d.N, d.B, d.C, d.p_base = D, P, N, B, C, p_base
    d.ntiles = lig_jet.nd_tiles(P, D) if ntiles is None else ntiles
    for k in range(4):
        d.n[k], d.lo_c[k], d.hi_c[k], d.cube[k] = n[k], 1e-6, 1 - 1e-6, 0.25
    return d


@pytest.mark.parametrize("why,kw", [
    ("D = 3", dict(D=3, n=(4, 5, 3, 0))), ("D = 0", dict(D=0)), ("D = 5", dict(D=5, ntiles=4)),
    ("do not fit", dict(P=0)), ("do not fit", dict(P=37, ntiles=9)), ("do not fit", dict(P=37, ntiles=14)),
    ("do not fit", dict(ntiles=0)), ("do not fit", dict(D=4, P=1, ntiles=1 << 27, n=(2, 2, 2, 2))),
    ("axis 1", dict(n=(4, 1, 0, 0))), ("axis 3", dict(D=4, n=(3, 4, 2, 1))),
    ("37 features", dict(D=2, C=34)), ("37 features", dict(D=4, C=32, n=(3, 4, 2, 3))), ("features", dict(C=0)),
    ("p_base", dict(p_base=-1)), ("p_base", dict(p_base=2 ** 31 - 10)), ("p_base", dict(N=0)), ("p_base", dict(B=0)),
    ("too large", dict(B=4, n=(1 << 15, 1 << 15, 0, 0))), ("too large", dict(D=4, B=1, n=(1 << 10,) * 4)),
])
def test_cell_nd_refuses_what_gather_nd_refuses(hiplib, why, kw):
    d = _gd(**kw)
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_cell_nd(ctypes.byref(d), FAKE, FAKE, None))
    assert "lig_cell_nd" in str(e.value) and why in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:                           # the same descriptor, the same answer from the gather
        _lib.check(hiplib.stpde_lig_gather_nd(ctypes.byref(d), FAKE, FAKE, FAKE, FAKE, None))
    assert "lig_gather_nd" in str(e.value) and why in str(e.value), str(e.value)


def test_cell_nd_refuses_null_pointers(hiplib):
    d = _gd()
    for args in ((None, FAKE), (FAKE, None)):
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_cell_nd(ctypes.byref(d), *args, None))
        assert "null pointer" in str(e.value)
    with pytest.raises(ValueError):
        _lib.check(hiplib.stpde_lig_cell_nd(None, FAKE, FAKE, None))


@pytest.mark.parametrize("why,args", [
    ("D = 3", (3, 8, 4, 3, 8)), ("do not fit", (2, 37, 9, 3, 37)), ("do not fit", (2, 37, 16, 3, 37)),
    ("do not fit", (1, 0, 4, 3, 8)), ("n_out", (2, 37, 12, 0, 37)), ("n_out", (2, 37, 12, 17, 37)),
    ("ldp", (4, 5, 8, 3, 4)),
])
def test_reduce_nd_bwd_refuses_bad_arguments(hiplib, why, args):
    D, P, nt, n_out, ldp = args
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_reduce_nd_bwd(D, P, nt, n_out, FAKE, ldp, FAKE, FAKE, None))
    assert "lig_reduce_nd_bwd" in str(e.value) and why in str(e.value), str(e.value)


def test_reduce_nd_bwd_refuses_null_pointers(hiplib):
    for k in range(3):
        ptrs = [FAKE] * 3
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_reduce_nd_bwd(2, 37, 12, 3, ptrs[0], 37, ptrs[1], ptrs[2], None))
        assert "null pointer" in str(e.value)


def _n(*v):
    return (ctypes.c_int * 4)(*(tuple(v) + (0,) * (4 - len(v))))


@pytest.mark.parametrize("why,D,B,n,C", [
    ("D = 3", 3, 2, (4, 5, 6), 8), ("D = 0", 0, 2, (4,), 8), ("D = 5", 5, 2, (4, 4, 4, 4), 8),
    ("axis 1", 2, 2, (4, 1), 8), ("axis 0", 1, 2, (1,), 8), ("axis 3", 4, 2, (3, 4, 2, 0), 8),
    ("C = 0", 2, 2, (4, 5), 0), ("C = 65", 2, 2, (4, 5), 65), ("bad B", 2, 0, (4, 5), 8),
    ("too large", 2, 2, (1 << 15, 1 << 15), 8), ("too large", 4, 1, (1 << 10,) * 4, 8), ("too large", 1, 2, (1 << 30,), 8),
])
def test_dlatent_reduce_nd_refuses_bad_arguments(hiplib, why, D, B, n, C):
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_dlatent_reduce_nd(D, B, _n(*n), C, FAKE, FAKE, FAKE, FAKE, None))
    assert "lig_dlatent_reduce_nd" in str(e.value) and why in str(e.value), str(e.value)


def test_dlatent_reduce_nd_refuses_null_pointers(hiplib):
    for k in range(4):
        ptrs = [FAKE] * 4
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_dlatent_reduce_nd(2, 2, _n(4, 5), 8, *ptrs, None))
        assert "null pointer" in str(e.value)
    with pytest.raises(ValueError):
        _lib.check(hiplib.stpde_lig_dlatent_reduce_nd(2, 2, None, 8, FAKE, FAKE, FAKE, FAKE, None))


def test_lig_jets_still_refuses_cpu_tensors_with_the_switch_on(monkeypatch):
    monkeypatch.setattr(lig_jet, "nd_backward", True)
    net = implicit_net.ImNet(dim=2, in_features=8, out_features=3, nf=16)
    with pytest.raises(RuntimeError):
        lig_jet.lig_jets(net, torch.rand(1, 4, 5, 8, requires_grad=True), torch.rand(1, 5, 2), 0., 1., False, ())
