"""Training through the coordinate derivatives on 1- and 2-d local implicit grids in HIP (opt-in ``lig_jet.nd_jet_backward`` on
top of ``lig_jet.nd_jets``): everything that needs no GPU.

* the numpy model of k_reduce_nd_jet_bwd (tests/lig_nd_jet_bwd_model.py) is the exact adjoint of the forward's model, writes
  every float of its output, reads nothing for padding rows or absent axes, and forms no address outside a buffer;
* the fp32 evaluation of the oracle stays within a quarter of the bounds of the GPU tests on their inputs;
* the switch, PDELayer's request policy, the eligibility of a training call;
* the per-kernel driver against the recording library stub of tests/test_lig_chunk_buffers_host.py.
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from space_time_pde_amd import _lib, implicit_net, lig_jet, local_implicit_grid as lig, pde
from tests import lig_nd_jet_bwd_model as BM
from tests import lig_nd_jet_model as JM
from tests import lig_nd_model as M
from tests import test_lig_chunk_buffers_host as CB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(4096)
GRID = {1: (5,), 2: (4, 5)}
# (S1, S2, S_mlp): the stream sets of the forward, and a piecewise-linear activation's S_mlp = 4 < S
STREAM_SETS = [(3, 0, 4), (3, 2, 6), (3, 4, 8), (3, 6, 10), (3, 2, 4), (3, 6, 4)]


def _coef(D, P, seed=0):
    pts = np.concatenate([M.edge_points(GRID[D], 1.0, seed=seed + k) for k in range(-(-P // 37))], 0)[:P]
    return JM.coef_nd(D, pts, GRID[D], *lig_jet.box_constants(GRID[D], 0., 1.))[0]


@pytest.mark.parametrize("n_out", [3, 7, 16])
@pytest.mark.parametrize("S1,S2,S_mlp", STREAM_SETS)
@pytest.mark.parametrize("D", [1, 2])
def test_model_is_the_exact_adjoint_of_the_forward_model(D, S1, S2, S_mlp, n_out):
    """<R f, ybar> = <f, R^T ybar> in fp64 to 1e-12 of the sum of the magnitudes of the terms, for one point, one point more
    than a tile and 37 points; padding rows, features >= n_out and the streams of absent axes exactly 0; NaN in ybar on an
    absent-axis stream and in the padding of its rows changes no bit of the output."""
    S = 1 + S1 + S2
    pairs = (BM.ALL_PAIRS[D] * 6)[:S2]
    for P in (1, (16 >> D) + 1, 37):
        nt, ldp = lig_jet.nd_tiles(P, D), P + 2
        coef = _coef(D, P).astype(np.float64)
        rng = np.random.default_rng(7 * D + S2 + S_mlp + n_out + P)
        f = rng.standard_normal((nt, S_mlp, 64, 4))
        ybar = rng.standard_normal((S, n_out, ldp))
        y, _, _ = JM.reduce_nd_jet(D, P, n_out, S1, S2, pairs, S_mlp, f, coef, ldp)
        abar, _, touched = BM.reduce_nd_jet_bwd(D, P, nt, n_out, S1, S2, pairs, S_mlp, ybar, coef, ldp, np.float64)
        lhs, rhs = (y[:, :, :P] * ybar[:, :, :P]).sum(), (f * abar).sum()
        scale = np.abs(y[:, :, :P] * ybar[:, :, :P]).sum() + np.abs(f * abar).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(scale, 1e-300), (P, lhs, rhs)
        # every float is written; zeros where nothing belongs
        assert touched["abar"] == set(range(nt * S_mlp * 256)) and not np.isnan(abar).any()
        TP = 16 >> D
        for t, j in itertools.product(range(nt), range(16)):
            lanes = [16 * g + j for g in range(4)]
            if t * TP + (j >> D) >= P:
                assert np.all(abar[t][:, lanes] == 0), (t, j)
        feat = (4 * (np.arange(64) >> 4))[:, None] + np.arange(4)[None, :]            # feature of (lane, register)
        assert np.all(abar[:, :, feat >= n_out] == 0)
        assert np.all(abar[:, 1 + D:4] == 0) and not np.signbit(abar[:, 1 + D:4]).any()
        # the cotangent of an absent axis and the padding of the rows are never read
        bad = ybar.copy()
        bad[1 + D:4] = np.nan
        bad[:, :, P:] = np.nan
        abar2, _, touched2 = BM.reduce_nd_jet_bwd(D, P, nt, n_out, S1, S2, pairs, S_mlp, bad, coef, ldp, np.float64)
        assert np.array_equal(abar2.view(np.uint64), abar.view(np.uint64)) and touched2 == touched


def test_piecewise_linear_cross_terms_still_reach_the_first_four_streams():
    """S_mlp = 4 < S: a cotangent on a second-order output alone gives non-zero adjoints of the value and tangent streams"""
    D, P, n_out = 2, 5, 3
    pairs = [(0, 0), (0, 1), (1, 1), (1, 1)]
    ybar = np.zeros((8, n_out, P))
    ybar[5] = 1.0                                           # d2 / dq_0 dq_1 only
    abar, _, _ = BM.reduce_nd_jet_bwd(D, P, lig_jet.nd_tiles(P, D), n_out, 3, 4, pairs, 4, ybar, _coef(D, P).astype(np.float64),
                                      dtype=np.float64)
    assert abar.shape[1] == 4 and all(np.abs(abar[:, s]).max() > 0 for s in (0, 1, 2)) and np.all(abar[:, 3] == 0)


@pytest.mark.parametrize("D", [1, 2])
def test_every_address_is_inside_its_buffer(D):
    """Every P / ntiles combination the entry point lets through (ceil(P / TP) <= ntiles <= that + 3), the corners among
    them -- one point in four tiles, a full last tile, one point more than a tile -- for the widest and the narrowest stream
    set: abar is covered exactly, coef and jets_bar are read for p < P only and inside [0, P * 16) / the rows' P columns."""
    TP = 16 >> D
    for P in (1, 2, TP - 1, TP, TP + 1, 4 * TP, 4 * TP + 1, 37):
        for extra in range(4):
            nt = -(-P // TP) + extra
            for S1, S2, S_mlp, n_out in ((3, 6, 10, 16), (3, 0, 4, 1), (3, 2, 4, 5)):
                S, ldp = 1 + S1 + S2, P + 1
                pairs = (BM.ALL_PAIRS[D] * 6)[:S2]
                _, _, t = BM.reduce_nd_jet_bwd(D, P, nt, n_out, S1, S2, pairs, S_mlp, np.zeros((S, n_out, ldp)),
                                               np.zeros((P, 16)), ldp, np.float64)
                assert t["abar"] == set(range(nt * S_mlp * 256)), (P, nt)
                assert t["coef"] == set(range(P * 16)), (P, nt)
                want = {(s * n_out + ch) * ldp + p for s in range(S) if not (1 + D <= s < 4) for ch in range(n_out) for p in range(P)}
                assert t["jets_bar"] == want, (P, nt)


def _cfg(S1=3, S2=2, pairs=((0, 0), (1, 1)), combo=0):
    c = _lib.JetCfg()
    c.S1, c.S2, c.combo = S1, S2, combo
    for k, (a, b) in enumerate(pairs):
        c.pair0[k], c.pair1[k] = a, b
    return c


GOOD = (6, 2, 37, 12, 3, 37)
REFUSALS = [
    ("D = 4", {}, (6, 4, 5, 8, 3, 5)), ("D = 3", {}, (6, 3, 8, 4, 3, 8)), ("do not fit", {}, (6, 2, 37, 9, 3, 37)),
    ("do not fit", {}, (6, 2, 37, 16, 3, 37)), ("do not fit", {}, (6, 1, 0, 4, 3, 8)), ("n_out", {}, (6, 2, 37, 12, 17, 37)),
    ("ldp", {}, (6, 2, 37, 12, 3, 36)), ("stream set", dict(S2=3), GOOD), ("stream set", dict(S1=0, S2=2), (1, 2, 37, 12, 3, 37)),
    ("combined", dict(combo=1), GOOD), ("pair 1", dict(pairs=((0, 0), (1, 2))), GOOD),
    ("pair 1", dict(pairs=((0, 0), (0, 1))), (6, 1, 37, 8, 3, 37)), ("S_mlp", {}, (0, 2, 37, 12, 3, 37)),
    ("S_mlp", {}, (7, 2, 37, 12, 3, 37)),
]


@pytest.mark.parametrize("why,ckw,args", REFUSALS)
def test_entry_point_refuses_what_the_forward_refuses(hiplib, why, ckw, args):
    S_mlp, D, P, nt, n_out, ldp = args
    cfg = _cfg(**ckw)
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_lig_reduce_nd_jet_bwd(ctypes.byref(cfg), S_mlp, D, P, nt, n_out, FAKE, ldp, FAKE, FAKE, None))
    assert "lig_reduce_nd_jet_bwd" in str(e.value) and why in str(e.value), str(e.value)


def test_new_symbols_null_pointers_and_the_abi_version(hiplib):
    for name in ("stpde_lig_reduce_nd_jet_bwd", "stpde_jet_wgrad_nd", "stpde_jet_tan0_reduce_nd"):
        assert name in _lib.exported_symbols() and hasattr(hiplib, name)
    assert hiplib.stpde_version() == _lib.ABI_VERSION                                # additive symbols: no bump of their own
    cfg = _cfg()
    S_mlp, D, P, nt, n_out, ldp = GOOD
    for k in range(3):
        ptrs = [FAKE] * 3
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(hiplib.stpde_lig_reduce_nd_jet_bwd(ctypes.byref(cfg), S_mlp, D, P, nt, n_out, ptrs[0], ldp, ptrs[1], ptrs[2], None))
        assert "null pointer" in str(e.value)
    for ncoord in (0, 4):
        with pytest.raises(ValueError):
            _lib.check(hiplib.stpde_jet_tan0_reduce_nd(4, 16, FAKE, FAKE, 48, 0, ncoord, None))
        d = _lib.LayerDesc()
        d.ntiles, d.KT, d.MT = 4, 0, 16
        with pytest.raises(ValueError):
            _lib.check(hiplib.stpde_jet_wgrad_nd(ctypes.byref(d), 1, FAKE, None, FAKE, None, FAKE, None, ncoord, None))
    d = _lib.LayerDesc()
    d.ntiles, d.KT, d.MT, d.mfma_bf16, d.cfg.S1 = 4, 16, 8, 1, 3
    with pytest.raises(NotImplementedError):                                           # plain bf16 operands: dim = 3 only
        _lib.check(hiplib.stpde_jet_wgrad_nd(ctypes.byref(d), 4, FAKE, FAKE, FAKE, FAKE, FAKE, None, 2, None))


# ---------------------------------------------------------------------------------------------------------------------
# tolerance margin of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def _padded(d, kind):
    full = BM.ALL_PAIRS[d] + [BM.ALL_PAIRS[d][-1]] * ((2 if d == 1 else 4) - len(BM.ALL_PAIRS[d]))
    return {"none": [], "all": full, "six": (BM.ALL_PAIRS[d] * 6)[:5] + [(BM.ALL_PAIRS[d] * 6)[4]]}[kind]


MARGIN = [(case, act, "all") for case in BM.GRAD_CASES for act in ("softplus", "leakyrelu")] + \
         [(case, "swish", "all") for case in BM.GRAD_CASES[:2]] + \
         [(case, "softplus", kind) for case in BM.GRAD_CASES[:2] for kind in ("none", "six")]


@pytest.mark.parametrize("case,act,kind", MARGIN)
def test_fp32_oracle_stays_within_a_quarter_of_the_gpu_bounds(case, act, kind):
    """oracle.jet_ref.lig_jets in fp32 against fp64 on the exact inputs of tests/test_gpu_lig_nd_jet_backward.py, forward and
    autograd gradients: the gap is what fp32 arithmetic alone costs on these inputs, and the GPU bounds (2e-5 per jet stream,
    2e-4 per gradient, relative to the tensor's largest magnitude) leave four times that.

    Measured (largest over the cases of this test): jets 4.0e-06 (d = 2, c = 8, softplus, all pairs), d latent 2.4e-07,
    parameter gradients 6.3e-06, beta 9.2e-07.  No point had to be replaced in the case builder; the node rows of the
    (4, 5) grid carry no cotangent, for the reason BM.make_case gives."""
    d, grid, c = case
    pairs = _padded(d, kind)
    net = BM.make_net(d, c, act)
    lat, pts, mask = BM.make_case(d, grid, c)
    cot = BM.cotangent(d, c, 4 + len(pairs), mask)
    a = BM.oracle(net, act, lat, pts, pairs, cot, torch.float32)
    b = BM.oracle(net, act, lat, pts, pairs, cot, torch.float64)
    rel = lambda x, y: ((x.double() - y).abs().max() / y.abs().max().clamp_min(1e-300)).item()
    m = mask.reshape(-1)
    ej = max(rel(a[0][s][:, m], b[0][s][:, m]) for s in range(a[0].shape[0]) if not (d < s < 4))
    eg = max([rel(a[1], b[1])] + [rel(x, y) for x, y in zip(a[2], b[2])] + ([rel(a[3], b[3])] if act == "swish" else []))
    print("d=%d c=%d %s %s: jets %.2e, gradients %.2e" % (d, c, act, kind, ej, eg))
    assert ej < 2e-5 / 4 and eg < 2e-4 / 4


# ---------------------------------------------------------------------------------------------------------------------
# the switch, the request policy, the eligibility
# ---------------------------------------------------------------------------------------------------------------------
def test_switch_default_setter_and_record(monkeypatch):
    assert lig_jet.nd_jet_backward is False or os.getenv("STPDE_ND_JET_BACKWARD")
    prev = lig_jet.set_nd_jet_backward(True)
    try:
        assert lig_jet.nd_jet_backward is True and lig_jet.set_nd_jet_backward(False) is True and lig_jet.nd_jet_backward is False
    finally:
        lig_jet.set_nd_jet_backward(prev)
    plan = lig_jet.ImNetPlan.get(2, 8, 3, 16)
    box = lig_jet.box_constants((4, 5), 0., 1.)
    for jets, bwd, ndb in itertools.product((False, True), repeat=3):
        monkeypatch.setattr(lig_jet, "nd_jets", jets)
        monkeypatch.setattr(lig_jet, "nd_jet_backward", bwd)
        monkeypatch.setattr(lig_jet, "nd_backward", ndb)
        call = lig_jet.JetCall.make(plan, "softplus", 0.0, True, [(0, 0)], None, "fp32", (4, 5), box, B=2, N=37)
        monkeypatch.setattr(lig_jet, "nd_jet_backward", not bwd)                       # frozen when the call was made
        assert call.nd_jet_backward is (jets and bwd) and call.nd_jets is jets and call.nd_backward is ndb     # inert without nd_jets
        assert call.pipeline is False


def test_switch_default_comes_from_the_environment():
    code = "from space_time_pde_amd import lig_jet; print(int(lig_jet.nd_jet_backward), int(lig_jet.nd_jets))"
    for val, want in ((None, "0 0"), ("1", "1 0"), ("0", "0 0"), ("off", "0 0"), ("true", "1 0")):
        env = {k: v for k, v in os.environ.items() if k not in ("STPDE_ND_JET_BACKWARD", "STPDE_ND_JETS")}
        if val is not None:
            env["STPDE_ND_JET_BACKWARD"] = val
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want, (val, out.stdout, out.stderr)


class _CudaLike(torch.Tensor):
    """A CPU tensor that says it is a CUDA tensor: _jet_request reads the flag, the shape and requires_grad only."""
    is_cuda = property(lambda self: True)


def test_jet_request_policy_table(monkeypatch):
    burgers = pde.PDELayer("t, x", "u")
    burgers.add_equation("dif(u,t) + u*dif(u,x) - 0.01*dif(dif(u,x),x)", "burgers")
    one = pde.PDELayer("x", "u")
    one.add_equation("dif(dif(u,x),x) - u", "ode")
    for layer, n_in, pairs in ((burgers, 2, [(1, 1)]), (one, 1, [(0, 0)])):
        for grad, jets, bwd, xg in itertools.product((False, True), repeat=4):
            monkeypatch.setattr(lig_jet, "nd_jets", jets)
            monkeypatch.setattr(lig_jet, "nd_jet_backward", bwd)
            x = torch.zeros(2, 5, n_in).as_subclass(_CudaLike).requires_grad_(xg)
            with torch.set_grad_enabled(grad):
                req = layer._jet_request(x)
            want = jets and (not grad or bwd) and not (xg and grad)
            assert (req is not None) is want, (n_in, grad, jets, bwd, xg)
            if req is not None:
                assert req.x is x and req.first and req.pairs == pairs and req.combo is None        # pairs, never the combined stream
    # three inputs: untouched by either switch
    rb = pde.PDELayer("t, x, z", "u")
    rb.add_equation("dif(u,t) - dif(dif(u,x),x) - 0.25*dif(dif(u,z),z)", "heat")
    x3 = torch.zeros(2, 5, 3).as_subclass(_CudaLike)
    for jets, bwd in itertools.product((False, True), repeat=2):
        monkeypatch.setattr(lig_jet, "nd_jets", jets)
        monkeypatch.setattr(lig_jet, "nd_jet_backward", bwd)
        assert rb._jet_request(x3).combo == {(1, 1): 1.0, (2, 2): 0.25}


class _T:
    """Stand-in for a CUDA tensor: the decisions read shapes and flags only."""

    def __init__(self, shape, cuda=True, dtype=torch.float32, requires_grad=False):
        self.shape, self.is_cuda, self.dtype, self.requires_grad = tuple(shape), cuda, dtype, requires_grad

    def dim(self):
        return len(self.shape)


def _case(dim, cin, grid=None, **kw):
    net = implicit_net.ImNet(dim=dim, in_features=cin, out_features=3, nf=16, activation=torch.nn.Softplus)
    return net, _T((2,) + tuple(grid or (3,) * dim) + (cin,), **kw), _T((2, 37, dim))


def test_training_eligibility(monkeypatch):
    monkeypatch.setattr(lig_jet, "mlp_precision", "fp32")
    R = lig.JetRequest

    def ok(net, lat, pts, pairs=(), combo=None):
        return lig._nd_jet_train_eligible(net, lat, pts, R(pts, True, pairs, combo))

    for jets, bwd in ((False, False), (True, False), (False, True)):                   # both switches, or nothing
        monkeypatch.setattr(lig_jet, "nd_jets", jets)
        monkeypatch.setattr(lig_jet, "nd_jet_backward", bwd)
        assert not ok(*_case(2, 8))
    monkeypatch.setattr(lig_jet, "nd_jets", True)
    monkeypatch.setattr(lig_jet, "nd_jet_backward", True)
    monkeypatch.setattr(lig_jet, "nd_backward", False)                                 # plays no part
    assert ok(*_case(1, 8)) and ok(*_case(2, 8)) and ok(*_case(1, 32)) and ok(*_case(2, 32))
    assert ok(*_case(2, 8), pairs=[(0, 0), (0, 1), (1, 1)]) and ok(*_case(2, 8, requires_grad=True))
    assert not lig._nd_jet_eligible(*_case(2, 8), R(None, True, ()))                   # (the forward-only clause says no)
    assert not ok(*_case(1, 33)) and not ok(*_case(2, 33))                             # c = 33: no latent-adjoint kernel
    assert not ok(*_case(4, 8)) and not ok(*_case(3, 8))
    assert not ok(*_case(2, 8), combo={(0, 0): 1.0, (1, 1): 1.0})
    assert not ok(*_case(2, 8), pairs=[(1, 2)])
    net, lat, pts = _case(2, 8)
    assert not lig._nd_jet_train_eligible(net, lat, pts, R(pts, False, ()))            # the value alone: a value query's business
    net, lat, pts = _case(2, 8)
    assert not ok(torch.nn.DataParallel(net), lat, pts)
    assert not lig._nd_jet_train_eligible(net, lat, pts, None) and not lig._nd_jet_train_eligible(net, lat, pts, R(_T((2, 37, 2)), True, ()))
    assert not ok(net, lat, _T(pts.shape, requires_grad=True))                         # point gradients: composed
    with torch.no_grad():
        assert not ok(net, lat, pts)                                                   # nothing to train: the forward-only path
        assert lig._nd_jet_eligible(net, lat, pts, R(pts, True, ()))
    monkeypatch.setattr(lig_jet, "mlp_precision", "bf16")
    assert not ok(net, lat, pts)
    monkeypatch.setattr(lig_jet, "mlp_precision", "fp32x3")
    assert ok(net, lat, pts)


# ---------------------------------------------------------------------------------------------------------------------
# the per-kernel driver against the recording stub
# ---------------------------------------------------------------------------------------------------------------------
def _drive(monkeypatch, dim, streams, fused_tail=True, wgrad=True, dlat=True, recompute=False, precision="fp32"):
    """One training call of two chunks through lig_jet._forward_chunk / _backward_chunk on CPU tensors against the stub:
    forward of both chunks with a stash, then their backward; ``recompute``: per chunk the forward, then the backward."""
    c = dict(precision=precision, tan0_rowsum=True, fused_tail=fused_tail, deterministic_dlatent=True, use_pipeline=True,
             dim=dim, streams=streams, kind="train", nd_jets=True)
    monkeypatch.setattr(lig_jet, "nd_jet_backward", True)
    call = CB.make_call(c, monkeypatch)
    assert call is not None and call.nd_jet_backward and not call.pipeline and call.need_grad
    rec = CB._Recorder()
    plan, P = call.plan, call.B * call.N
    packs, packs16 = CB._packs(plan, call.nsplit if call.bf16 else 0)
    g = torch.Generator().manual_seed(1)
    latent = rec.add_input("latent", torch.rand(call.B, *call.grid_shape, plan.cin, generator=g))
    pts = rec.add_input("pts", torch.rand(P, plan.dim, generator=g))
    jets = rec.add_input("jets", torch.zeros(call.S_out, plan.cout, P))
    jets_bar = rec.add_input("jets_bar", torch.ones(call.S_out, plan.cout, P))
    rec.add_input("packs", packs)
    for (l, name), t in sorted((packs16 or {}).items()):
        rec.add_input("packs16[%d, %s]" % (l, name), t)
    dw_flat = rec.add_input("dw_flat", torch.empty(plan.n_dw)) if wgrad else None
    dlatent = rec.add_input("dlatent", torch.zeros_like(latent)) if dlat else None
    monkeypatch.setattr(lig_jet._lib, "lib", lambda: CB._Stub(rec))
    monkeypatch.setattr(lig_jet, "stream_ptr", lambda: None)
    monkeypatch.setattr(lig_jet, "torch", rec)
    rec.on = True
    chunks = lig_jet._chunk_ranges(call, P)
    assert len(chunks) == 2
    fwd = lambda k: lig_jet._forward_chunk(call, packs, packs16, latent, pts[chunks[k][0]:sum(chunks[k])], jets, chunks[k][0], True)
    bwd = lambda k, s: lig_jet._backward_chunk(call, packs, packs16, s, jets_bar, dw_flat, dlatent, None, None)
    marks = []
    if recompute:
        for k in range(2):
            rec.phase = "forward %d" % k
            s = fwd(k)
            marks.append(len(rec.calls))
            rec.phase = "backward %d" % k
            bwd(k, s)
            marks.append(len(rec.calls))
    else:
        saved = []
        for k in range(2):
            rec.phase = "forward %d" % k
            saved.append(fwd(k))
            marks.append(len(rec.calls))
        for k in range(2):
            rec.phase = "backward %d" % k
            bwd(k, saved[k])
            marks.append(len(rec.calls))
    rec.on = False
    names = [n for n, _ in rec.calls]
    return call, rec, [names[a:b] for a, b in zip([0] + marks[:-1], marks)]


def _fwd_names(tail):
    layers = ["stpde_jet_layer_fwd"] * 2 + ["stpde_jet_tail_fwd_p"] if tail else ["stpde_jet_layer_fwd"] * 5
    return ["stpde_lig_gather_nd", "stpde_lig_coef_nd"] + layers + ["stpde_lig_reduce_nd_jet_fwd"]


def _bwd_names(tail, wgrad, dlat):
    w = ["stpde_jet_wgrad_nd"] if wgrad else []
    if tail:
        seq = w + ["stpde_jet_tail_bwd_p"] + w + w
    else:
        seq = w + ["stpde_jet_layer_bwd"] + w + ["stpde_jet_layer_bwd"] + w + ["stpde_jet_layer_bwd"]
    seq += w + ["stpde_jet_layer_bwd"] + w + ["stpde_jet_layer_bwd"]
    seq += ["stpde_jet_wgrad", "stpde_jet_tan0_reduce_nd"] if wgrad else []
    seq += ["stpde_lig_sort_tmp_bytes", "stpde_lig_xbar_rows", "stpde_lig_cell_nd", "stpde_lig_cell_sort",
            "stpde_lig_dlatent_reduce_nd"] if dlat else []
    return ["stpde_lig_reduce_nd_jet_bwd"] + seq


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("wgrad", [True, False])
@pytest.mark.parametrize("streams,tail", [("first", True), ("pairs", True), ("pairs", False)])
@pytest.mark.parametrize("dim", [1, 2])
def test_entry_point_sequence_of_a_training_call(monkeypatch, dim, streams, tail, wgrad, recompute):
    call, rec, parts = _drive(monkeypatch, dim, streams, fused_tail=tail, wgrad=wgrad, recompute=recompute)
    assert call.tail is tail
    f, b = _fwd_names(tail), _bwd_names(tail, wgrad, True)
    assert parts == ([f, b, f, b] if recompute else [f, f, b, b])
    nt = lig_jet.nd_tiles(call.mult, dim)
    for name, args in rec.calls:
        if name == "stpde_lig_reduce_nd_jet_bwd":       # (cfg_out, S_mlp, D, P, ntiles, n_out, jets_bar, ldp, coef, abar_out)
            assert args[1:6] == [call.S, dim, call.mult, nt, 4] and args[7] == 2 * call.mult
            assert args[6].startswith("input jets_bar") and args[8].startswith("alloc") and args[9].startswith("alloc")
        if name in ("stpde_jet_wgrad_nd", "stpde_jet_tan0_reduce_nd"):
            assert args[-2] == dim, (name, args)         # the coordinate axes of the grid
        if name == "stpde_jet_wgrad":                    # the one plain call: value stream x raw input of layer 0
            assert args[1] == 1
        if name == "stpde_lig_xbar_rows":
            assert args[0]["S"][:5] == [1] + [call.S] * 4 and args[0]["SP"][0] == 1
    assert "stpde_jet_tan0_reduce" not in [n for n, _ in rec.calls]


@pytest.mark.parametrize("dim", [1, 2])
def test_weights_alone_and_the_split_operands(monkeypatch, dim):
    _, _, parts = _drive(monkeypatch, dim, "pairs", dlat=False, precision="fp32x3")
    assert parts[2] == _bwd_names(True, True, False)


@pytest.mark.parametrize("streams", ["first", "pairs"])
@pytest.mark.parametrize("dim", [1, 2])
def test_table_is_what_is_allocated_and_what_the_plan_counts(monkeypatch, dim, streams):
    call, rec, _ = _drive(monkeypatch, dim, streams)
    monkeypatch.setattr(_lib, "lib", lambda: CB._Stub(CB._Recorder()))
    m = call.mult
    got = {}
    for phase, n, dt, _, _ in rec.allocs:
        got.setdefault(phase, []).append((n, dt))
    got = {k: sorted(v) for k, v in got.items()}
    fwd = CB._sizes(lig_jet._forward_buffers(call, m, True))
    bwd = CB._sizes(lig_jet._backward_buffers(call, m) + lig_jet._dlatent_buffers(call, m))
    assert got == {"forward 0": fwd, "forward 1": fwd, "backward 0": bwd, "backward 1": bwd}
    names = [b[0] for b in lig_jet._forward_buffers(call, m, True)]
    assert "coef" in names and "z0" in names and "roww" in names and "cell" not in names
    plan_fwd, plan_bwd = lig_jet._per_point_bytes(call)
    assert plan_fwd * m == CB._nbytes(fwd)
    scratch = lig_jet._dlatent_buffers(call, m)
    uncounted = CB._nbytes(CB._sizes([b for b in scratch if b[0] in ("start", "sort_tmp")]))
    assert plan_bwd * m == CB._nbytes(bwd) - uncounted + lig_jet.SORT_TMP_PLAN_BYTES * m
    # the stash and the chunk sizes follow the same tables
    assert lig_jet._stash_bytes(call, 2 * m) == 2 * m * plan_fwd + m * plan_bwd
