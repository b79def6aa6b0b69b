"""Coordinate derivatives on 4-d local implicit grids -- 3-d space + time -- in HIP (opt-in, ``lig_jet.nd4_jets``): everything
that needs no GPU -- the pass schedule, the host model of the two new kernels (tests/lig_nd4_jet_model.py) assembled over the
schedule against the fp64 oracle, every address the kernels form, the plan's tangent constants per axis triple, the switch,
the dispatch decisions, PDELayer's request on four inputs and the argument checks of the two new entry points."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import jet_ref as J
from space_time_pde_amd import _lib, implicit_net, lig_jet, pde
from space_time_pde_amd import local_implicit_grid as lig
from space_time_pde_amd.lig_jet import ImNetPlan, XT
from tests import lig_nd4_jet_model as JM4
from tests import lig_nd_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch
GRID = (3, 4, 2, 3)
CASES = [(4, GRID, 8), (4, GRID, 31)]                 # the second fills the sparse third input tile: 4 + 31 + 1 = 36
TRIPLES = [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
ALL_PAIRS = [(a, b) for a in range(4) for b in range(a, 4)]
NS_PAIRS = [(1, 1), (2, 2), (3, 3)]                   # incompressible Navier-Stokes on (t, x, y, z): the Laplacian in space
NS_U = ("dif(u,t) + u*dif(u,x) + v*dif(u,y) + w*dif(u,z) + dif(p,x)"
        " - 0.01*(dif(dif(u,x),x) + dif(dif(u,y),y) + dif(dif(u,z),z))")
CONT = "dif(u,x) + dif(v,y) + dif(w,z)"


# ---------------------------------------------------------------------------------------------------------------------
# the pass schedule
# ---------------------------------------------------------------------------------------------------------------------
def _brute_minimum(axes, pairs):
    """the fewest triples whose union holds ``axes`` and of which one holds both axes of every pair"""
    for size in range(1, 5):
        for sub in itertools.combinations(TRIPLES, size):
            if set(axes) <= {a for t in sub for a in t} and all(any(a in t and b in t for t in sub) for a, b in pairs):
                return size
    raise AssertionError


def test_schedule_rules_hold_for_every_request(monkeypatch):
    monkeypatch.delenv("STPDE_S34", raising=False)
    for first in (False, True):
        for mask in range(1 << 10):
            pairs = [ALL_PAIRS[k] for k in range(10) if mask >> k & 1][::-1 if mask & 1 else 1]     # (both orders occur)
            passes = lig_jet.nd4_passes(first, pairs)
            assert passes == lig_jet.nd4_passes(first, list(pairs))                  # deterministic
            wants_first = first or bool(pairs)                                        # a pair brings the tangents, as make_cfg
            assert len(passes) == _brute_minimum(range(4) if wants_first else (), pairs), (first, pairs)
            seen_pairs, seen_first, streams = [], [], []
            for k, (triple, pp, (dv, df, dp)) in enumerate(passes):
                assert triple in TRIPLES and len(df) == 3 and len(dp) == len(pp)
                assert len(pp) in (0, 2, 4, 6)                                       # the S2 of a compiled stream set
                assert dv == (0 if k == 0 else -1)                                   # the value: pass 0 only
                real = [(pr, s) for pr, s in zip(pp, dp) if s >= 0]
                assert [s for _, s in real] == list(dp[:len(real)]) and all(s == -1 for s in dp[len(real):])
                assert all(pr == pp[len(real) - 1] for pr in pp[len(real):])         # padding repeats the last pair
                assert (len(real) >= 1 or not pp) and len(pp) - len(real) <= 1   # an odd count is padded by one, no more
                for (a, b), s in real:
                    assert a in triple and b in triple and pairs[s - 5] == (a, b)
                    seen_pairs.append((a, b))
                for a, s in zip(triple, df):
                    if s >= 0:
                        assert s == 1 + a
                        seen_first.append(a)
                streams += [s for s in (dv,) + tuple(df) + tuple(dp) if s >= 0]
            assert sorted(seen_pairs) == sorted(pairs)                               # every pair in exactly one pass
            assert sorted(seen_first) == (list(range(4)) if wants_first else [])     # every axis stored exactly once
            assert len(set(streams)) == len(streams) and set(streams) == set([0] + [1 + a for a in seen_first]
                                                                             + [5 + i for i in range(len(pairs))])


def test_schedule_of_the_named_requests():
    ns = lig_jet.nd4_passes(True, NS_PAIRS)
    assert len(ns) == 2                                                               # Navier-Stokes: two passes
    assert ns == [((0, 1, 2), [(1, 1), (2, 2)], (0, (1, 2, 3), (5, 6))), ((0, 1, 3), [(3, 3), (3, 3)], (-1, (-1, -1, 4), (7, -1)))]
    # all ten pairs: three triples hold the six mixed pairs -- (0,1) (0,2) (1,2) | (0,3) (1,3) | (2,3) -- and no two do (a triple
    # holds three of them, two triples share one), so the brute-force minimum is 3, not the 4 that every request fits in
    ten = lig_jet.nd4_passes(True, ALL_PAIRS)
    assert len(ten) == 3 == _brute_minimum(range(4), ALL_PAIRS)
    assert [t for t, _, _ in ten] == TRIPLES[:3] and [len(pp) for _, pp, _ in ten] == [6, 4, 2]
    assert len(lig_jet.nd4_passes(True, [])) == 2 and len(lig_jet.nd4_passes(True, [(0, 1), (2, 3)])) == 2
    assert len(lig_jet.nd4_passes(True, [(0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2)])) == 3
    one = lig_jet.nd4_passes(False, [])
    assert one == [((0, 1, 2), [], (0, (-1, -1, -1), ()))]                            # the value alone
    for bad in ([(0, 4)], [(-1, 0)], [(1, 1), (1, 1)], [(0, 1), (1, 0)]):
        with pytest.raises(ValueError):
            lig_jet.nd4_passes(True, bad)


# ---------------------------------------------------------------------------------------------------------------------
# the model over the schedule, in fp64, against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _dyadic_case(cin, act, seed):
    """The grid of the cases with a box that makes the model's fp32 geometry EXACT, so that the fp64 oracle sees the same
    numbers: cell sizes that are powers of two (xmax = (n - 1) / 4 resp. 1 / 2 for the two-node axis) and interior points on odd
    multiples of xmax / 512, never a node."""
    xmax = (0.5, 0.75, 0.5, 0.5)
    rng = np.random.default_rng(seed)
    pts = (rng.integers(1, 256, size=(11, 4)) * 2 + 1) / 512.0 * np.asarray(xmax)
    torch.manual_seed(seed)
    net = implicit_net.ImNet(dim=4, in_features=cin, out_features=3, nf=16, activation=act)
    latent = rng.standard_normal((1,) + GRID + (cin,)).astype(np.float32)
    return xmax, pts.astype(np.float32), net, latent


@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
@pytest.mark.parametrize("d,grid,cin", CASES)
def test_host_model_over_the_schedule_matches_jet_oracle(d, grid, cin, act, monkeypatch):
    """M.gather_nd -> oracle.jet_ref.mlp_jets on the gathered rows (fp64; all four tangents and all ten pairs at once) -> per
    pass of the schedule the streams of its triple in the fc5-row layout -> reduce_nd4_jet into one jets tensor, against
    oracle.jet_ref.lig_jets in fp64 on the same fp32 points: all 1 + 4 + 10 streams to 1e-12 of max(1, the stream's largest
    magnitude).  The row numbering, the slot map, the record of four axes, the corner numbering, the slots of every triple,
    every term of the reduction and the destination map agree.  leakyrelu: the layer buffers hold value + tangents only
    (S_mlp = 4), the second derivatives come from the weight cross terms."""
    monkeypatch.setattr(lig_jet, "nd4_jets", True)
    xmax, pts, net, latent = _dyadic_case(cin, {"softplus": torch.nn.Softplus, "leakyrelu": torch.nn.LeakyReLU}[act], 40 + cin)
    P, S = pts.shape[0], 15
    box = lig_jet.box_constants(grid, 0., xmax)
    call = lig_jet.JetCall.make(ImNetPlan.get(4, cin, 3, 16), act, 0.0, True, ALL_PAIRS, None, "fp32", grid, box, B=1, N=P,
                                need_grad=False)
    passes = lig_jet.nd4_passes(True, ALL_PAIRS)
    assert call.S_out == S and call.pairs == ALL_PAIRS and len(call.passes) == len(passes) == 3
    assert call.S == (4 if act == "leakyrelu" else 10) == max(ps.S for ps in call.passes)
    for ps, (triple, pp, dst) in zip(call.passes, passes):          # the records are the schedule
        assert ps.triple == triple and ps.desc.npairs == len(pp) and ps.desc.S == S and ps.desc.S_mlp == ps.S
        assert (ps.desc.dst_value, tuple(ps.desc.dst_first), tuple(ps.desc.dst_pair)[:len(pp)]) == dst
        assert list(zip(ps.desc.pair0, ps.desc.pair1))[:len(pp)] == pp and tuple(ps.desc.axis) == triple
        assert (ps.cfg.S1, ps.cfg.S2) == (3, 0 if act == "leakyrelu" else len(pp))
        if act != "leakyrelu":                                        # the layer kernels see SLOTS of the triple
            assert [(triple[a], triple[b]) for a, b in list(zip(ps.cfg.pair0, ps.cfg.pair1))[:len(pp)]] == pp
    lo_c, hi_c, cube = box
    nt = lig_jet.nd_tiles(P, 4)
    X, _, _ = M.gather_nd(4, pts, latent, P, 0, lo_c, hi_c, cube, nt)
    rows = X.reshape(nt, XT, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(nt * 16, XT * 16)[:P << 4]
    x = torch.from_numpy(rows[:, call.plan.slot[:4 + cin]].astype(np.float64))
    p64 = [(net.fc[k].weight.detach().double(), net.fc[k].bias.detach().double()) for k in range(6)]
    f = [t.numpy() for t in J.mlp_jets(p64, act, x, 4, ALL_PAIRS)]  # value, four tangents, ten pairs

    def out_pre_of(k, triple, pp):
        streams = [f[0]] + [f[1 + a] for a in triple]
        if act != "leakyrelu":
            streams += [f[5 + ALL_PAIRS.index(pr)] for pr in pp]
        return JM4.out_pre_from_streams(4, streams, nt, 3), len(streams)

    coef, _ = JM4.coef_nd4(pts, grid, lo_c, hi_c, cube)
    jets, _, _ = JM4.assemble(passes, P, 3, S, coef, out_pre_of)
    ref = J.lig_jets(p64, act, torch.from_numpy(latent).double(), torch.from_numpy(pts)[None].double(), (0.,) * 4, xmax,
                     second=ALL_PAIRS)[:, 0].numpy()                # [15, P, 3]
    assert jets.shape == (S, 3, P) and np.isfinite(jets).all()      # every stream of every point written
    for s in range(S):
        want = ref[s].T
        scale = max(1.0, np.abs(want).max())
        assert np.abs(jets[s] - want).max() <= 1e-12 * scale, (s, np.abs(jets[s] - want).max(), scale)


def test_coefficient_model_on_the_edge_points():
    """the record against the dim <= 2 model's geometry axis by axis (the same geom_axis_jet), its zero tail, and the flat clip
    at exactly 0, exactly xmax and outside (rows 24 .. 27): every derivative coefficient exactly zero"""
    pts = M.edge_points(GRID, 1.0)
    lo_c, hi_c, cube = lig_jet.box_constants(GRID, 0., 1.)
    coef, t = JM4.coef_nd4(pts, GRID, lo_c, hi_c, cube)
    assert t["pts"] == set(range(pts.size)) and t["coef"] == set(range(37 * 24))
    for p in range(37):
        for k in range(4):
            _, om, _, dom, kap = M.geom_axis_jet(pts[p, k], lo_c[k], hi_c[k], cube[k], GRID[k])
            assert (coef[p, k], coef[p, 4 + k], coef[p, 8 + k], coef[p, 12 + k], coef[p, 16 + k]) == (om[0], om[1], dom[0], dom[1], kap)
    assert np.all(coef[:, 20:] == 0) and not np.signbit(coef[:, 20:]).any()
    assert np.all(coef[24:28, 8:20] == 0)
    assert np.all(coef[:24, 16:20] == 1 / np.asarray(cube, np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# addresses
# ---------------------------------------------------------------------------------------------------------------------
def _hostile_points():
    pts = M.edge_points(GRID, 1.0)
    bad = [np.full(4, v, np.float32) for v in (np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31)]
    mixed = []
    for k, v in enumerate((np.nan, np.inf, 1e30, -1e30)):
        one = pts[3 + k].copy()
        one[k] = v
        mixed.append(one)
    return np.concatenate([pts, np.stack(bad + mixed)], 0)


def test_host_model_addresses_stay_inside_their_buffers():
    """Every index the two kernels form, for NaN, +-inf, +-1e30, +-3e38 and +-2^31 coordinates and for NaN / inf decoder rows:
    derived from P, n_out and the (host-checked) descriptor alone, so the same sets whatever the values are; a pass touches
    the streams of its map and no other."""
    pts = _hostile_points()
    lo_c, hi_c, cube = lig_jet.box_constants(GRID, 0., 1.)
    rng = np.random.default_rng(0)
    S, n_out = 15, 3
    for pc in (pts.shape[0], 1, 5):
        p = pts[-pc:]
        coef, t = JM4.coef_nd4(p, GRID, lo_c, hi_c, cube)
        assert t["pts"] == set(range(pc * 4)) and t["coef"] == set(range(pc * 24))
        assert np.isfinite(coef).all()                                # (a NaN coordinate ends on the upper face, as fminf does)
        nt, ldp = lig_jet.nd_tiles(pc, 4), pc + 3
        assert pc <= nt
        for first, pairs, piecewise in ((True, ALL_PAIRS, False), (True, ALL_PAIRS, True), (True, NS_PAIRS, False), (True, [], False),
                                        (True, [(2, 3), (0, 1)], False)):
            for triple, pp, dst in lig_jet.nd4_passes(first, pairs):
                S_mlp = 4 if piecewise else 4 + len(pp)
                out_pre = rng.standard_normal((nt, S_mlp, 256)).astype(np.float32)
                out_pre[0, :, ::7] = np.nan
                out_pre[-1, :, ::5] = np.inf
                jets, bound, tr = JM4.reduce_nd4_jet(pc, n_out, triple, pp, S_mlp, S, dst, out_pre, coef, ldp)
                assert tr["coef"] == set(range(pc * 24))
                assert min(tr["out_pre"]) >= 0 and max(tr["out_pre"]) < pc * S_mlp * 256 <= out_pre.size     # its own tile, no further
                named = [s for s in (dst[0],) + tuple(dst[1]) + tuple(dst[2]) if s >= 0]
                want = {(s * n_out + ch) * ldp + q for s in named for ch in range(n_out) for q in range(pc)}
                assert tr["jets"] == want and max(want) < S * n_out * ldp
                untouched = np.ones((S, n_out, ldp), bool)
                untouched[named, :, :pc] = False
                assert np.isnan(jets[untouched]).all()                # (the model's fresh tensor is NaN: nothing else written)


# ---------------------------------------------------------------------------------------------------------------------
# plan: tangent constants per axis triple
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [8, 31])
def test_tanc_arrays_of_the_triples(cin):
    plan = ImNetPlan(4, cin, 3, 16)
    before = (plan.pack_index_np.copy(), [dict(o) for o in plan.pack_off], plan.n_pack, plan.unpack_index_np.copy())
    assert plan.tanc_nd4 == {}                                        # built on demand only
    zero = plan.n_theta
    g = np.arange(64) >> 4
    for triple in TRIPLES:
        arrays = plan.tanc_index(triple)
        assert len(arrays) == 6 and plan.tanc_index(triple) is arrays
        for l, lay in enumerate(plan.layers):
            MT = lay["MT"]
            assert arrays[l].shape == (3, MT, 64, 4) and arrays[l].dtype == np.int64
            row = 16 * np.arange(MT)[:, None, None] + 4 * g[None, :, None] + np.arange(4)[None, None, :]
            for k, a in enumerate(triple):
                # column a_k of the skip block of W_l (feature a sits in slot a), zero for rows past M and for fc5
                want = np.where((row < lay["M"]) & lay["skip"], lay["w_off"] + row * lay["Kin"] + lay["Kh"] + a, zero)
                np.testing.assert_array_equal(arrays[l][k], want)
            if not lay["skip"]:
                assert np.all(arrays[l] == zero)
            if triple == (0, 1, 2):                                   # ... which for (0, 1, 2) is the plan's own "tanc" pack
                off, size = plan.pack_off[l]["tanc"]
                np.testing.assert_array_equal(arrays[l].reshape(-1), plan.pack_index_np[off:off + size])
    assert sorted(plan.tanc_nd4) == TRIPLES
    assert np.array_equal(plan.pack_index_np, before[0]) and [dict(o) for o in plan.pack_off] == before[1]
    assert plan.n_pack == before[2] and np.array_equal(plan.unpack_index_np, before[3])
    for bad in ((0, 1), (0, 0, 1), (1, 0, 2), (0, 1, 4), (-1, 0, 1)):
        with pytest.raises(ValueError):
            plan.tanc_index(bad)
    with pytest.raises(ValueError):
        ImNetPlan(2, 8, 3, 16).tanc_index((0, 1, 2))
    # the values: pack_tanc gathers the columns of the parameters
    gen = torch.Generator().manual_seed(cin)
    params = []
    for lay in plan.layers:
        params += [torch.randn(lay["M"], lay["Kin"], generator=gen), torch.randn(lay["M"], generator=gen)]
    assert plan.pack_tanc(params, []) == {}
    both = plan.pack_tanc(params, [(0, 2, 3), (1, 2, 3)])
    assert sorted(both) == [(0, 2, 3), (1, 2, 3)]
    tc = both[(0, 2, 3)]
    for l, lay in enumerate(plan.layers):
        col = tc[l].reshape(3, lay["MT"], 4, 16, 4)[:, :, :, 0, :].reshape(3, -1)[:, :lay["M"]]
        for k, a in enumerate((0, 2, 3)):
            want = params[2 * l][:, lay["Kh"] + a] if lay["skip"] else torch.zeros(lay["M"])
            assert torch.equal(col[k], want)


def test_tanc_arrays_at_the_benchmarked_width():
    """nf = 32, four outputs, 16 channels (tools/bench_lig_nd4_jets.py): MT = 2 for fc4; the arrays of (0, 1, 2) are the plan's
    own "tanc" packs index for index, and those of (1, 2, 3) differ from them by the column offset alone"""
    plan = ImNetPlan(4, 16, 4, 32)
    assert [lay["MT"] for lay in plan.layers] == [32, 16, 8, 4, 2, 1]
    own, last = plan.tanc_index((0, 1, 2)), plan.tanc_index((1, 2, 3))
    zero = plan.n_theta
    for l, lay in enumerate(plan.layers):
        off, size = plan.pack_off[l]["tanc"]
        assert size == 3 * lay["MT"] * 256
        np.testing.assert_array_equal(own[l].reshape(-1), plan.pack_index_np[off:off + size])
        np.testing.assert_array_equal(last[l], np.where(own[l] == zero, zero, own[l] + 1))
        assert (own[l] != zero).any() == bool(lay["skip"])


# ---------------------------------------------------------------------------------------------------------------------
# the switch, the call record, the dispatch decisions
# ---------------------------------------------------------------------------------------------------------------------
def test_switch_default_setter_and_record(monkeypatch):
    assert lig_jet.nd4_jets is False or os.getenv("STPDE_ND4_JETS")  # default off
    assert lig_jet.ND_JET_DIMS == (1, 2)
    prev = lig_jet.set_nd4_jets(True)
    try:
        assert lig_jet.nd4_jets is True and lig_jet.set_nd4_jets(False) is True and lig_jet.nd4_jets is False
    finally:
        lig_jet.set_nd4_jets(prev)
    plan = ImNetPlan.get(4, 8, 3, 16)
    box = lig_jet.box_constants(GRID, 0., 1.)
    mk = lambda first, pairs, **kw: lig_jet.JetCall.make(plan, "softplus", 0.0, first, pairs, kw.pop("combo", None), "fp32", GRID, box,
                                                         B=2, N=37, need_grad=False, **kw)
    monkeypatch.setattr(lig_jet, "nd4_jets", True)
    call = mk(True, NS_PAIRS)
    monkeypatch.setattr(lig_jet, "nd4_jets", False)                   # frozen when the call was made
    assert call.nd4_jets is True and len(call.passes) == 2
    assert (call.S_out, call.S, call.cfg.S1, call.cfg.S2, call.mult, call.pipeline, call.P_pad, call.pairs) == \
        (8, 6, 3, 2, 4, False, 74, NS_PAIRS)
    with pytest.raises(NotImplementedError):                          # off: such a request cannot be made
        mk(True, NS_PAIRS)
    v = mk(False, [])                                                 # value queries do not care
    assert v.nd4_jets is False and v.passes == () and v.S == 1
    monkeypatch.setattr(lig_jet, "nd_jets", True)                     # ``nd_jets`` alone does not admit d = 4
    with pytest.raises(NotImplementedError):
        mk(True, [])
    monkeypatch.setattr(lig_jet, "nd4_jets", True)
    with pytest.raises(NotImplementedError):
        mk(True, [], combo={(1, 1): 1.0, (2, 2): 1.0})
    with pytest.raises(ValueError):
        mk(True, [(0, 4)])
    with pytest.raises(NotImplementedError):
        lig_jet.JetCall.make(plan, "softplus", 0.0, True, [], None, "bf16", GRID, box, B=2, N=37, need_grad=False)
    # buffers: the wider record instead of the 16-float one, the layer buffers of the widest pass; value queries as before
    names = lambda c: [b[0] for b in lig_jet._forward_buffers(c, 4, False)]
    assert names(call) == ["X", "roww", "coef4"] + ["buf%d" % l for l in range(1, 6)]
    assert dict((b[0], b[1]) for b in lig_jet._forward_buffers(call, 4, False))["coef4"] == 4 * 24
    assert names(v) == ["X", "roww"] + ["buf%d" % l for l in range(1, 6)]
    assert lig_jet._buf_floats(call, 1, 4) == 6 * lig_jet._buf_floats(v, 1, 4)
    ten = mk(True, ALL_PAIRS)
    assert ten.S == 10 and lig_jet._buf_floats(ten, 1, 4) == 10 * lig_jet._buf_floats(v, 1, 4)


def test_switch_default_comes_from_the_environment():
    code = "from space_time_pde_amd import lig_jet; print(int(lig_jet.nd4_jets), int(lig_jet.nd_jets))"
    for val, want in ((None, "0 0"), ("1", "1 0"), ("0", "0 0"), ("off", "0 0"), ("true", "1 0")):
        env = {k: v for k, v in os.environ.items() if k not in ("STPDE_ND4_JETS", "STPDE_ND_JETS")}
        if val is not None:
            env["STPDE_ND4_JETS"] = val
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want, (val, out.stdout, out.stderr)


class _T:
    """Stand-in for a CUDA tensor: the decisions read shapes and flags only."""

    def __init__(self, shape, cuda=True, dtype=torch.float32, requires_grad=False):
        self.shape, self.is_cuda, self.dtype, self.requires_grad = tuple(shape), cuda, dtype, requires_grad

    def dim(self):
        return len(self.shape)


def _case(dim, cin, nf=16, grid=None, n_out=3, **kw):
    net = implicit_net.ImNet(dim=dim, in_features=cin, out_features=n_out, nf=nf, activation=torch.nn.Softplus)
    grid = grid or (3,) * dim
    return net, _T((2,) + tuple(grid) + (cin,), **kw), _T((2, 37, dim))


def test_eligibility_table(monkeypatch):
    monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
    monkeypatch.setattr(lig_jet, "nd_jets", False)
    monkeypatch.setattr(lig_jet, "nd_jet_backward", False)
    R = lig.JetRequest

    def ok(net, lat, pts, first=True, pairs=(), combo=None, req_pts=None):
        return lig._nd_jet_eligible(net, lat, pts, R(pts if req_pts is None else req_pts, first, pairs, combo))

    with torch.no_grad():
        monkeypatch.setattr(lig_jet, "nd4_jets", False)
        assert not ok(*_case(4, 8))                                   # off: nothing is eligible
        monkeypatch.setattr(lig_jet, "nd_jets", True)
        assert not ok(*_case(4, 8)) and ok(*_case(2, 8))              # ``nd_jets`` alone leaves d = 4 ineligible
        monkeypatch.setattr(lig_jet, "nd_jets", False)
        monkeypatch.setattr(lig_jet, "nd4_jets", True)
        assert ok(*_case(4, 8)) and ok(*_case(4, 31)) and ok(*_case(4, 8, grid=GRID))
        assert not ok(*_case(2, 8)) and not ok(*_case(1, 8)) and not ok(*_case(3, 8))     # independent of ``nd_jets``
        assert ok(*_case(4, 8), pairs=ALL_PAIRS) and ok(*_case(4, 8), pairs=NS_PAIRS) and ok(*_case(4, 8), first=False)
        assert ok(*_case(4, 8, n_out=16)) and not ok(*_case(4, 8, n_out=17))
        assert not ok(*_case(4, 32))                                  # 4 + 32 + 1 = 37 features
        assert not ok(*_case(4, 8), pairs=[(3, 4)]) and not ok(*_case(4, 8), pairs=[(-1, 0)])     # an axis the grid lacks
        assert not ok(*_case(4, 8), combo={(1, 1): 1.0, (2, 2): 1.0})
        assert not ok(*_case(4, 8, nf=4)) and not ok(*_case(4, 8, grid=(3, 1, 3, 3)))
        assert not ok(*_case(4, 8, cuda=False)) and not ok(*_case(4, 8, dtype=torch.float64))
        net, lat, pts = _case(4, 8)
        assert not lig._nd_jet_eligible(net, lat, pts, None)          # no request
        assert not ok(net, lat, pts, req_pts=_T((2, 37, 4)))          # a request for other points
        assert not ok(torch.nn.Linear(13, 3), lat, pts)
        for prec, want in (("fp32x3", True), ("bf16", False)):
            monkeypatch.setattr(lig_jet, "mlp_precision", prec)
            assert ok(net, lat, pts) is want
        monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
        assert not lig._nd_value_eligible(net, lat, pts, R(pts, True, []))
    # grad mode on: the parameters of a fresh ImNet require grad -> composed, whatever the training switches say
    net, lat, pts = _case(4, 8)
    assert not ok(net, lat, pts)
    monkeypatch.setattr(lig_jet, "nd_jets", True)
    monkeypatch.setattr(lig_jet, "nd_jet_backward", True)
    req = R(pts, True, [])
    assert not lig._nd_jet_train_eligible(net, _T(lat.shape, requires_grad=True), pts, req)
    net2, lat2, pts2 = _case(2, 8)
    assert lig._nd_jet_train_eligible(net2, lat2, pts2, R(pts2, True, []))          # (d <= 2 trains as before)
    for p in net.parameters():
        p.requires_grad_(False)
    assert ok(net, lat, pts)
    assert not ok(net, _T(lat.shape, requires_grad=True), pts) and not ok(net, lat, _T(pts.shape, requires_grad=True))
    with torch.no_grad():
        assert ok(net, _T(lat.shape, requires_grad=True), pts)


class _CudaLike(torch.Tensor):
    """A CPU tensor that says it is a CUDA tensor: _jet_request reads the flag, the shape and requires_grad only."""
    is_cuda = property(lambda self: True)


def _navier_stokes():
    layer = pde.PDELayer("t, x, y, z", "u, v, w, p")
    layer.add_equation(NS_U, "xmom")
    layer.add_equation(CONT, "continuity")
    return layer


def test_jet_request_for_four_inputs(monkeypatch):
    layer = _navier_stokes()
    x = torch.zeros(2, 5, 4).as_subclass(_CudaLike)
    monkeypatch.setattr(lig_jet, "nd4_jets", False)
    monkeypatch.setattr(lig_jet, "nd_jets", True)
    monkeypatch.setattr(lig_jet, "nd_jet_backward", True)
    with torch.no_grad():
        assert layer._jet_request(x) is None                          # switch off (``nd_jets`` plays no part)
    monkeypatch.setattr(lig_jet, "nd4_jets", True)
    assert layer._jet_request(x) is None                              # grad mode on: no request, whatever the training switches
    with torch.no_grad():
        req = layer._jet_request(x)
        assert req is not None and req.x is x and req.first and req.combo is None
        assert req.pairs == NS_PAIRS                                  # pairs, never the combined stream
        assert layer._jet_request(torch.zeros(2, 5, 4)) is None       # CPU tensor
        assert layer.device_program_compiles()                        # streams 1 .. 4, pairs from 5: the evaluator takes it
        named = pde.PDELayer("t, x, y, z", "u")
        named.add_equation("dif(u,t) - x*dif(dif(u,z),z)", "named")
        assert named._jet_request(x).pairs == [(3, 3)]
        assert not named.device_program_compiles()                    # names an input: coordinates are [P][3] on the device
    # n_in == 3 is untouched: the combined stream, whatever the switch and the grad mode say
    rb = pde.PDELayer("t, x, z", "u")
    rb.add_equation("dif(u,t) - dif(dif(u,x),x) - 0.25*dif(dif(u,z),z)", "heat")
    x3 = torch.zeros(2, 5, 3).as_subclass(_CudaLike)
    for on in (False, True):
        monkeypatch.setattr(lig_jet, "nd4_jets", on)
        assert rb._jet_request(x3).combo == {(1, 1): 1.0, (2, 2): 0.25}


def test_residues_from_jets_reads_four_first_order_streams():
    """streams 1 + d for d < 4 and pairs from stream 5, through the lambdified functions (CPU jets)"""
    layer = pde.PDELayer("t, x, y, z", "u")
    layer.add_equation("dif(u,t) + 2*dif(u,z) - 3*dif(dif(u,y),z) + x", "eq")
    x = torch.arange(24.).reshape(1, 6, 4)
    jets = torch.arange(7 * 6.).reshape(7, 1, 6) ** 1.5
    req = lig.JetRequest(x, True, [(0, 0), (2, 3)])
    req.jets, req.pairs_out = jets, [(0, 0), (2, 3)]
    res = layer._residues_from_jets(x, req)["eq"]
    want = (jets[1, 0] + 2 * jets[4, 0] - 3 * jets[6, 0] + x[0, :, 1]).reshape(1, 6, 1)
    assert torch.allclose(res, want, rtol=1e-6, atol=0)


def test_lig_jets_refuses_cpu_tensors_whatever_the_switch(monkeypatch):
    monkeypatch.setattr(lig_jet, "nd4_jets", True)
    net = implicit_net.ImNet(dim=4, in_features=8, out_features=3, nf=16)
    with pytest.raises(RuntimeError), torch.no_grad():
        lig_jet.lig_jets(net, torch.rand(1, 3, 4, 2, 3, 8), torch.rand(1, 5, 4), 0., 1., True, ())


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_and_the_abi_version_stays(hiplib):
    for name in ("stpde_lig_coef_nd4", "stpde_lig_reduce_nd4_jet_fwd"):
        assert name in _lib.exported_symbols() and hasattr(hiplib, name)
    header = open(os.path.join(ROOT, "include", "stpde_hip.h")).read()
    assert "int stpde_lig_coef_nd4(" in header and "int stpde_lig_reduce_nd4_jet_fwd(" in header and "stpde_nd4_pass_desc" in header
    assert _lib.ABI_VERSION == 316 and hiplib.stpde_version() == 316


def _gd(D=4, P=37, N=37, B=2, C=8, p_base=0, ntiles=None, n=GRID):
    d = _lib.GatherNdDesc()
    d.D, d.P, d.N, d.B, d.C, d.p_base = D, P, N, B, C, p_base
    d.ntiles = lig_jet.nd_tiles(P, min(max(D, 1), 4)) if ntiles is None else ntiles
    for k in range(4):
        d.n[k], d.lo_c[k], d.hi_c[k], d.cube[k] = n[k], 1e-6, 1 - 1e-6, 0.25
    return d


@pytest.mark.parametrize("why,kw", [
    ("D = 2", dict(D=2, n=(4, 5, 0, 0))), ("D = 3", dict(D=3, n=(4, 5, 3, 0))), ("D = 1", dict(D=1, n=(5, 0, 0, 0))), ("D = 0", dict(D=0)),
    ("do not fit", dict(P=0)), ("do not fit", dict(P=37, ntiles=36)), ("axis 2", dict(n=(3, 4, 1, 3))),
    ("37 features", dict(C=32)), ("p_base", dict(p_base=-1)), ("p_base", dict(N=0)),
])
def test_coef_nd4_refuses_bad_arguments(hiplib, why, kw):
    d = _gd(**kw)
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_coef_nd4(ctypes.byref(d), FAKE, FAKE, None))
    assert "lig_coef_nd4" in str(e.value) and why in str(e.value), str(e.value)


def test_coef_nd4_refuses_null_pointers(hiplib):
    d = _gd()
    for args in ((None, FAKE), (FAKE, None)):
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_coef_nd4(ctypes.byref(d), *args, None))
        assert "null pointer" in str(e.value)
    with pytest.raises(ValueError):
        _lib.check(hiplib.stpde_lig_coef_nd4(None, FAKE, FAKE, None))


def _pass(axis=(0, 1, 3), pairs=((0, 3), (3, 3)), S_mlp=None, S=8, dst_value=0, dst_first=(1, 2, 4), dst_pair=(5, 6), npairs=None):
    d = _lib.Nd4PassDesc()
    d.npairs = len(pairs) if npairs is None else npairs
    d.S_mlp, d.S, d.dst_value = 4 + d.npairs if S_mlp is None else S_mlp, S, dst_value
    for k in range(3):
        d.axis[k], d.dst_first[k] = axis[k], dst_first[k]
    for k, (a, b) in enumerate(pairs):
        d.pair0[k], d.pair1[k] = a, b
    for k, s in enumerate(dst_pair):
        d.dst_pair[k] = s
    return d


# (D, P, ntiles, n_out, ldp)
GOOD = (4, 37, 40, 3, 37)
REFUSALS = [
    ("D = 2", {}, (2, 37, 12, 3, 37)), ("D = 3", {}, (3, 8, 4, 3, 8)), ("D = 1", {}, (1, 8, 4, 3, 8)), ("D = 0", {}, (0, 8, 8, 3, 8)),
    ("do not fit", {}, (4, 37, 36, 3, 37)),                            # P > ntiles
    ("do not fit", {}, (4, 37, 44, 3, 37)), ("do not fit", {}, (4, 0, 4, 3, 8)),
    ("n_out", {}, (4, 37, 40, 0, 37)), ("n_out", {}, (4, 37, 40, 17, 37)),
    ("ldp", {}, (4, 37, 40, 3, 36)),
    ("axis triple", dict(axis=(0, 0, 3)), GOOD), ("axis triple", dict(axis=(1, 0, 3)), GOOD), ("axis triple", dict(axis=(0, 1, 4)), GOOD),
    ("axis triple", dict(axis=(-1, 1, 3)), GOOD), ("axis triple", dict(axis=(0, 3, 2)), GOOD),
    ("npairs", dict(npairs=1), GOOD), ("npairs", dict(npairs=3), GOOD), ("npairs", dict(npairs=8), GOOD), ("npairs", dict(npairs=-2), GOOD),
    ("S_mlp", dict(S_mlp=5), GOOD), ("S_mlp", dict(S_mlp=8), GOOD), ("S_mlp", dict(S_mlp=1), GOOD),
    ("S = ", dict(S=0), GOOD), ("S = ", dict(S=16), GOOD),
    ("pair 0", dict(pairs=((0, 2), (3, 3))), GOOD), ("pair 1", dict(pairs=((0, 3), (2, 2))), GOOD),
    ("pair 1", dict(pairs=((0, 3), (3, 4))), GOOD), ("pair 0", dict(pairs=((-1, 0), (3, 3))), GOOD),
    ("destination stream 8", dict(dst_value=8), GOOD), ("destination stream -2", dict(dst_first=(1, -2, 4)), GOOD),
    ("destination stream 9", dict(dst_pair=(5, 9)), GOOD), ("named twice", dict(dst_pair=(5, 5)), GOOD),
    ("named twice", dict(dst_first=(1, 2, 0)), GOOD),
]


@pytest.mark.parametrize("why,dkw,args", REFUSALS)
def test_reduce_nd4_jet_refuses_bad_arguments(hiplib, why, dkw, args):
    D, P, nt, n_out, ldp = args
    d = _pass(**dkw)
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_reduce_nd4_jet_fwd(ctypes.byref(d), D, P, nt, n_out, FAKE, FAKE, FAKE, ldp, None))
    assert "lig_reduce_nd4_jet_fwd" in str(e.value) and why in str(e.value), str(e.value)


def test_reduce_nd4_jet_refuses_null_pointers(hiplib):
    d = _pass()
    D, P, nt, n_out, ldp = GOOD
    for k in range(3):
        ptrs = [FAKE] * 3
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_reduce_nd4_jet_fwd(ctypes.byref(d), D, P, nt, n_out, *ptrs, ldp, None))
        assert "null pointer" in str(e.value)
    with pytest.raises(ValueError):
        _lib.check(hiplib.stpde_lig_reduce_nd4_jet_fwd(None, D, P, nt, n_out, FAKE, FAKE, FAKE, ldp, None))


def test_the_entry_points_of_d_le_2_keep_refusing_four(hiplib):
    """the new work has new names: the d <= 2 entry points answer D = 4 as before"""
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_coef_nd(ctypes.byref(_gd()), FAKE, FAKE, None))
    assert "D = 4" in str(e.value)
