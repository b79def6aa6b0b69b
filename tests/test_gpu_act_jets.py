"""The activation jets of csrc/common.h (act_eval_t / act_eval2_t, act_jet_fwd_w, act_jet_adj_w, swish_beta_adj) element by
element in their tails, through the layer kernels that evaluate them, and NaN through the whole network.

Single layers are driven through the C ABI with a selection matrix as W_h, W_s = 0 and no tangent constants, so that
stpde_jet_layer_fwd returns act_jet(in_pre) and stpde_jet_layer_bwd_to its adjoint exactly, element by element: K = M, so one
identity covers every feature.  The pre-activations are the 32,768-point sweep of tests/act_jet_model.py (the softplus threshold,
the series / log seam of log1p, exp underflow, saturated tanh, both zeros), the reference is oracle.jet_ref.act_derivs in fp64
with its adjoint by autograd, and every output element is held to the bounds of tests/act_jet_model.py (4 x what a correctly
rounded fp32 transcription reaches, in units of 2^-24 of the sum of the absolute values of the output's terms).  Three kernel
families: the per-wave k_layer (KT = MT = 2; run-time activation switch for the (3,6) adjoint), the workgroup-cooperative
k_layer_coop in fp32 (KT = MT = 8) and the same with mfma_bf16 = 3 and the three-term pack -- whose SPL = 3 instantiation exists
for S1 + S2 <= 4; the (3,2) set takes the exact-fp32 kernel there, which the dispatch trace states.

The measured maxima of every case go to test_reports/act_jet_errors.json (not tracked); a copy of an MI355X run is
profiles/act_jet_errors.json.
A hardware maximum above its bound is a finding to explain, not a bound to raise.

NaN: a NaN pre-activation must give the jet and the adjoint the oracle gives, element by element, and one latent node set to NaN
must make every stream, every RB2 residual and every gradient that depends on it NaN and leave every other point bit-identical.
ELU failed both: fmin(NaN, 0) = 0 gave value 0 and slope 1 until act_eval_t<ELU> selected its exponent with the comparison it
already had.  Through the network only d W5[0, :] showed it -- fc5 has no skip connection behind fc4's activation, but its
epilogue multiplies the raw input (bias column) by zero skip weights, 0 * NaN, so the forward streams were NaN all the same.
These tests feed NaN DATA to kernels: ordinary arithmetic, every index in bounds."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import act_jet_model as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
XT = 3
N = A.ROWS * A.FEATS
FAMILIES = {"wave": (2, 0), "coop": (8, 0), "coop_x3": (8, 3)}       # KT = MT, mfma_bf16
REPORT_DIR = "test_reports"
_report = {}


def _record(key, value):
    _report[key] = value
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "act_jet_errors.json"), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)


# ---- fragment images (tests/test_gpu_fp32x3_products.py, for any tile counts): buffers are [tile][S][KT][64][4] ------------
def _to_blocks(streams, kt):
    """list of S arrays [rows, 16 kt] -> [tile][S][kt][64][4]: lane 16g+j = features 4g..4g+3 of row j."""
    x = torch.stack([torch.from_numpy(np.array(s)) for s in streams], 0)            # [S, rows, K]
    S, rows = x.shape[0], x.shape[1]
    x = x.reshape(S, rows // 16, 16, kt, 4, 4)                                       # [s, tile, j, kt, g, r]
    return x.permute(1, 0, 3, 4, 2, 5).reshape(rows // 16, S, kt, 64, 4).contiguous()


def _from_blocks(y, T, S, mt):
    """[tile][S][mt][64][4] -> S arrays [rows, 16 mt] (numpy)."""
    y = y.reshape(T, S, mt, 4, 16, 4)                                                # [tile, s, mt, g, j, r]
    return list(y.permute(1, 0, 4, 2, 3, 5).reshape(S, T * 16, 16 * mt).cpu().numpy())


def _pack_w(W, kt, mt):
    """W [16 mt, 16 kt] -> A-operand pack [kt][mt][64][4] = W[16mt + j, 16kt + 4g + r] (lig_jet.ImNetPlan, "Wh"; the pack of
    W^T is the "WhT" pack of W)."""
    x = W.reshape(mt, 16, kt, 4, 4)                                                  # [mt, j, kt, g, r]
    return x.permute(2, 0, 3, 1, 4).reshape(kt, mt, 64, 4).contiguous()


def _pack_w_split3(pack, kt, mt):
    """lig_jet.ImNetPlan.pack_bf16(nsplit=3): [3][kt/2][mt][64][8] bf16."""
    w = pack.view(kt // 2, 2, mt, 64, 4).permute(0, 2, 3, 1, 4)
    terms, r = [], w
    for _ in range(3):
        h = r.to(torch.bfloat16)
        terms.append(h)
        r = r - h.float()
    return torch.stack(terms, 0).contiguous()


def _desc(T, kt, mt, S1, S2, act, split, first_hidden=0):
    from space_time_pde_amd import _lib
    d = _lib.LayerDesc()
    d.ntiles, d.KT, d.MT, d.first_hidden = T, kt, mt, first_hidden
    d.cfg.S1, d.cfg.S2, d.cfg.act = S1, S2, _lib.ACT_CODES[act]
    d.cfg.act_param = float(A.BETA) if act == "swish" else 0.0
    for p, (e0, e1) in enumerate(A.PAIRS[S2]):
        d.cfg.pair0[p], d.cfg.pair1[p] = e0, e1
    d.mfma_bf16, d.packed = split, 0
    return d


def _check_trace(tr, family, S1, S2):
    if family == "wave":
        assert tr.has("k_layer") and not tr.has("k_layer_coop"), tr.kernels
        return
    assert tr.has("k_layer_coop"), tr.kernels
    x3 = any("k_layer_coop" in k and ("true, 1, false, 3" in k or "SPL = 3" in k) for k in tr.kernels)
    # the three-term kernels are compiled for S1 + S2 <= 4; beyond that "fp32x3" is served by the exact-fp32 kernel
    assert x3 == (family == "coop_x3" and S1 + S2 <= 4), tr.kernels


def _identity_packs(kt, split):
    pack = _pack_w(torch.eye(16 * kt), kt, kt).to(DEV)
    return pack, (_pack_w_split3(pack, kt, kt) if split else None)


def _case(S1, S2, K):
    """The sweep and its companion streams as [N / K, K] arrays: element-wise data, so any row length is the same case."""
    pre, cot, pairs = A.case_inputs(S1, S2)
    return [p.reshape(-1, K) for p in pre], [c.reshape(-1, K) for c in cot], pairs


def _ref(act, S1, S2, K):
    r = A.reference(act, S1, S2)
    return {k: ([x.reshape(-1, K) for x in v] if isinstance(v, list) else v) for k, v in r.items()}


def _assert_bounds(act, direction, got, ref, M, where):
    mx = A.maxima_by_order(got, ref, M)
    print("%s %s: max units by order %s (bounds %s)" % (where, direction, mx, A.BOUNDS[act][direction]))
    for order, v in enumerate(mx):
        assert v is None or v <= A.BOUNDS[act][direction][order], (where, direction, order, v, A.BOUNDS[act][direction][order])
    return mx


@pytest.mark.parametrize("sset", A.FWD_SETS, ids=lambda s: "s%d%d" % s)
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("act", A.ACTS)
def test_forward_jet_elementwise(hiplib, act, family, sset):
    from space_time_pde_amd import _lib
    (S1, S2), (kt, split) = sset, FAMILIES[family]
    S, K = 1 + S1 + S2, 16 * kt
    T = N // K // 16
    pre, _, _ = _case(S1, S2, K)
    pack, w16 = _identity_packs(kt, split)
    inp = _to_blocks(pre, kt).to(DEV)
    X = torch.zeros(T * XT * 256, device=DEV)
    Ws = torch.zeros(XT * kt * 256, device=DEV)
    tanc = torch.zeros(3 * kt * 256, device=DEV)
    out = torch.full((T * S * kt * 256,), float("nan"), device=DEV)
    d = _desc(T, kt, kt, S1, S2, act, split)
    with _lib.dispatch_trace() as tr:
        _lib.check(hiplib.stpde_jet_layer_fwd(C.byref(d), _lib.ptr(inp), _lib.ptr(X), _lib.ptr(pack), _lib.ptr(Ws),
                                              _lib.ptr(tanc), None, None, _lib.ptr(out), None, _lib.ptr(w16), None,
                                              _lib.stream_ptr()))
        torch.cuda.synchronize()
    _check_trace(tr, family, S1, S2)
    got = _from_blocks(out, T, S, kt)
    assert all(np.isfinite(g).all() for g in got)
    ref = _ref(act, S1, S2, K)
    where = "%s/%s/(%d,%d)" % (act, family, S1, S2)
    _record("fwd/" + where, _assert_bounds(act, "fwd", got, ref["h"], ref["Mh"], where))
    if S1 and act in ("relu", "leakyrelu", "elu"):
        # torch's conventions at +0 and -0 (elements 0 and 1 of the sweep): slope 0 / 0.01 / 1, exactly
        slope = {"relu": 0.0, "leakyrelu": 0.01, "elu": 1.0}[act]
        for dd in range(3):
            want = np.float32(slope) * pre[1 + dd][0, :2]
            assert np.array_equal(got[1 + dd][0, :2], want), (where, got[1 + dd][0, :2], want)
        assert np.array_equal(got[0][0, :2], np.zeros(2, np.float32))


@pytest.mark.parametrize("act", ["softplus", "elu"])
def test_first_hidden_layer_regenerates_the_sweep_exactly(hiplib, act):
    """first_hidden = 1: the kernel regenerates layer 0 from X.  The sweep sits in the 32 latent slots of 1,024 rows (r = 0, no
    ones column), W0 copies latent slot f mod 32 to feature f of 128, tanc0 holds one tangent per feature and direction.  The
    z0 stash must be the sweep bit for bit -- except that -0 comes out as +0, as it must from a product summed into an
    accumulator that starts at +0 -- and the layer's output the activation jet of it, to the bounds of the hidden layers."""
    from space_time_pde_amd import _lib
    S1, S2, kt = 3, 2, 8
    S, K, rows = 6, 128, N // 32
    T = rows // 16
    lat = A.sweep().reshape(rows, 32)
    slot = np.array([f if f < 32 else 32 + 4 * (f - 32) for f in range(3, 35)])      # lig_jet.ImNetPlan.slot of latent c
    Xf = np.zeros((rows, 16 * XT), np.float32)
    Xf[:, slot] = lat
    X = torch.from_numpy(Xf).reshape(T, 16, XT, 4, 4).permute(0, 2, 3, 1, 4).contiguous().to(DEV)      # [tile][XT][64][4]
    W0 = torch.zeros(K, 16 * XT)
    W0[torch.arange(K), torch.from_numpy(slot)[torch.arange(K) % 32]] = 1.0
    W0s = W0.reshape(kt, 16, XT, 4, 4).permute(2, 0, 3, 1, 4).contiguous().to(DEV)                    # [XT][KT][64][4]
    rng = np.random.default_rng(22)
    tang = (rng.uniform(0.5, 2.0, (3, K)) * rng.choice([-1.0, 1.0], (3, K))).astype(np.float32)
    tanc0 = torch.from_numpy(tang).reshape(3, kt, 4, 1, 4).expand(3, kt, 4, 16, 4).reshape(3, kt, 64, 4).contiguous().to(DEV)
    pack, _ = _identity_packs(kt, 0)
    Ws = torch.zeros(XT * kt * 256, device=DEV)
    tanc = torch.zeros(3 * kt * 256, device=DEV)
    out = torch.full((T * S * kt * 256,), float("nan"), device=DEV)
    z0 = torch.full((T * kt * 256,), float("nan"), device=DEV)
    d = _desc(T, kt, kt, S1, S2, act, 0, first_hidden=1)
    with _lib.dispatch_trace() as tr:
        _lib.check(hiplib.stpde_jet_layer_fwd(C.byref(d), None, _lib.ptr(X), _lib.ptr(pack), _lib.ptr(Ws), _lib.ptr(tanc),
                                              _lib.ptr(W0s), _lib.ptr(tanc0), _lib.ptr(out), None, None, _lib.ptr(z0),
                                              _lib.stream_ptr()))
        torch.cuda.synchronize()
    assert tr.has("k_layer_coop"), tr.kernels
    a = np.ascontiguousarray(np.tile(lat, (1, 4)))
    got_z0, = _from_blocks(z0, T, 1, kt)
    assert np.array_equal(got_z0.view(np.int32), (a + np.float32(0)).view(np.int32))
    tan = np.broadcast_to(tang[:, None, :], (3, rows, K))
    sec = np.zeros((6, rows, K), np.float32)               # layer 0 is affine: its second-order streams are zero
    ref = A.reference(act, S1, S2, a=a, tan=tan, sec=sec)
    got = _from_blocks(out, T, S, kt)
    where = "%s/first_hidden/(3,2)" % act
    _record("fwd/" + where, _assert_bounds(act, "fwd", got, ref["h"], ref["Mh"], where))


ADJ_CASES = [(act, fam, (3, 0) if act in ("relu", "leakyrelu") else ((3, 6) if fam == "wave" else (3, 2)))
             for act in A.ACTS for fam in FAMILIES]
# the three-term kernels exist for S1 + S2 <= 4 only: (3,0) runs them for the smooth activations too
ADJ_CASES += [(act, "coop_x3", (3, 0)) for act in A.ACTS if act not in ("relu", "leakyrelu")]


@pytest.mark.parametrize("act,family,sset", ADJ_CASES, ids=lambda v: v if isinstance(v, str) else "s%d%d" % v)
def test_adjoint_jet_elementwise(hiplib, act, family, sset):
    from space_time_pde_amd import _lib
    (S1, S2), (kt, split) = sset, FAMILIES[family]
    S, K = 1 + S1 + S2, 16 * kt
    T = N // K // 16
    pre, cot, _ = _case(S1, S2, K)
    pack, w16 = _identity_packs(kt, split)                  # the "WhT" pack of the identity is the identity's pack
    inp = _to_blocks(pre, kt).to(DEV)
    cob = _to_blocks(cot, kt).to(DEV)
    keep = inp.clone()
    out = torch.full((T * S * kt * 256,), float("nan"), device=DEV)
    pbar = torch.zeros(_lib.PBAR_SLOTS, device=DEV) if act == "swish" else None
    d = _desc(T, kt, kt, S1, S2, act, split)
    with _lib.dispatch_trace() as tr:
        _lib.check(hiplib.stpde_jet_layer_bwd_to(C.byref(d), _lib.ptr(cob), _lib.ptr(pack), _lib.ptr(inp), _lib.ptr(out), None,
                                                 _lib.ptr(pbar), _lib.ptr(w16), _lib.stream_ptr()))
        torch.cuda.synchronize()
    _check_trace(tr, family, S1, S2)
    assert torch.equal(inp.view(torch.int32), keep.view(torch.int32))          # _bwd_to leaves the stash intact
    got = _from_blocks(out, T, S, kt)
    assert all(np.isfinite(g).all() for g in got)
    ref = _ref(act, S1, S2, K)
    where = "%s/%s/(%d,%d)" % (act, family, S1, S2)
    rec = {"abar": _assert_bounds(act, "adj", got, ref["abar"], ref["Mabar"], where)}
    if act == "swish":
        # d/d beta: 64 slots of fp32 partial sums, added up here in fp64, against the fp64 sum of 32,768 x S terms in units of
        # 2^-24 of the fp64 sum of their absolute values
        dbeta = float(pbar.double().sum())
        rec["dbeta"] = abs(dbeta - ref["dbeta"]) / (A.U * ref["dbeta_abs"])
        print("%s d/d beta %r (fp64 %r): %.3f units (bound %.3g)" % (where, dbeta, ref["dbeta"], rec["dbeta"], A.DBETA_BOUND))
        assert rec["dbeta"] <= A.DBETA_BOUND, (where, dbeta, ref["dbeta"])
    _record("adj/" + where, rec)


# ---- a NaN pre-activation, element by element -----------------------------------------------------------------------------
NAN_AT = (37, 5)       # row (third row tile), feature of the [N / K, K] view


def _expected_nan(act, direction, pre, cot, pairs):
    """Which streams of the jet (adjoint) at a NaN pre-activation are NaN: the expressions of the jet on the oracle's derivatives
    at NaN (ReLU / LeakyReLU: value NaN, slopes the constants of the a > 0 == False side; everything else NaN)."""
    from oracle.jet_ref import act_derivs
    r, f = NAN_AT
    s = [x.numpy() for x in act_derivs(act, torch.tensor([float("nan")], dtype=torch.float64),
                                       torch.tensor(float(A.BETA), dtype=torch.float64))]
    p1 = [np.array([float(x[r, f])]) for x in pre]
    p1[0] = np.array([np.nan])
    with np.errstate(all="ignore"):
        if direction == "fwd":
            out = A.jet_fwd_fp32(s, p1, pairs)
        else:
            out = A.jet_adj_fp32(s, p1, [np.array([float(c[r, f])]) for c in cot], pairs)
    return [bool(np.isnan(x[0])) for x in out]


@pytest.mark.parametrize("direction", ["fwd", "adj"])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("act", A.ACTS)
def test_nan_pre_activation_elementwise(hiplib, act, family, direction):
    """One NaN in the value stream of the (3,2) set.  Forward: the selection GEMM multiplies the NaN element's jet into every
    feature of its row (0 * NaN), so a stream of that row is NaN throughout exactly where the oracle's jet at NaN is NaN, and
    finite throughout otherwise; adjoint: the element's own adjoints are NaN exactly where the oracle's are.  Everything else is
    bit-identical to the run without the NaN.  ELU returned value 0 and slope 1 here (fmin(NaN, 0) = 0)."""
    from space_time_pde_amd import _lib
    (S1, S2), (kt, split) = (3, 2), FAMILIES[family]
    S, K = 6, 16 * kt
    T = N // K // 16
    pre, cot, pairs = _case(S1, S2, K)
    bad0 = np.array(pre[0])
    bad0[NAN_AT] = np.nan
    pack, w16 = _identity_packs(kt, split)
    d = _desc(T, kt, kt, S1, S2, act, split)
    zeros = [torch.zeros(n, device=DEV) for n in (T * XT * 256, XT * kt * 256, 3 * kt * 256)]
    cob = _to_blocks(cot, kt).to(DEV)
    outs = []
    for a0 in (pre[0], bad0):
        inp = _to_blocks([a0] + pre[1:], kt).to(DEV)
        out = torch.full((T * S * kt * 256,), float("nan"), device=DEV)
        if direction == "fwd":
            _lib.check(hiplib.stpde_jet_layer_fwd(C.byref(d), _lib.ptr(inp), _lib.ptr(zeros[0]), _lib.ptr(pack),
                                                  _lib.ptr(zeros[1]), _lib.ptr(zeros[2]), None, None, _lib.ptr(out), None,
                                                  _lib.ptr(w16), None, _lib.stream_ptr()))
        else:
            _lib.check(hiplib.stpde_jet_layer_bwd_to(C.byref(d), _lib.ptr(cob), _lib.ptr(pack), _lib.ptr(inp), _lib.ptr(out),
                                                     None, None, _lib.ptr(w16), _lib.stream_ptr()))
        torch.cuda.synchronize()
        outs.append(_from_blocks(out, T, S, kt))
    clean, bad = outs
    want = _expected_nan(act, direction, pre, cot, pairs)
    assert all(want) or act in ("relu", "leakyrelu")
    r, f = NAN_AT
    for st in range(S):
        touched = np.zeros(clean[st].shape, dtype=bool)
        if direction == "fwd":
            touched[r, :] = True
        else:
            touched[r, f] = True
        assert np.array_equal(bad[st][~touched].view(np.int32), clean[st][~touched].view(np.int32)), (st, "other elements moved")
        if want[st]:
            assert np.isnan(bad[st][touched]).all(), "stream %d: finite where the oracle is NaN: %r" % (st, bad[st][r, f])
        else:
            assert np.isfinite(bad[st][touched]).all(), "stream %d: NaN where the oracle is finite" % st


# ---- NaN through the network ----------------------------------------------------------------------------------------------
NAN_CASES = [(act, prec) for act in A.ACTS for prec in ("fp32", "fp32x3")] + \
            [(act, "bf16") for act in ("softplus", "leakyrelu", "tanh")]       # the activations the bf16 mode is tested with
NODE = (1, 2, 2, 3)        # batch item, then an interior node of the (4, 5, 6) grid
CHANNEL = 11


def _run_net(act, prec, lat_cpu):
    from space_time_pde_amd import lig_jet, local_implicit_grid as lig, physics
    from tests.test_gpu_lig_jet import _net
    net = _net(act, nf=32 if prec == "bf16" else 16).to(DEV)
    g = torch.Generator().manual_seed(31)
    pts = (0.02 + 0.96 * torch.rand(2, 101, 3, generator=g)).to(DEV)
    tgt = torch.randn(2, 101, 4, generator=g).to(DEV)
    lat = lat_cpu.to(DEV).requires_grad_(True)
    with torch.no_grad():
        jets, pp = lig_jet.lig_jets(net, lat, pts, 0., 1., True, ((1, 1), (2, 2)))
    layer = physics.get_rb2_pde_layer(mean=(0.01, 0.0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1.,
                                      x_crop=1., use_continuity=True)
    layer.update_forward_method(lambda p: lig.query_local_implicit_grid(net, lat, p, 0., 1.))
    n0 = lig.stats["hip_jet_calls"]
    pred, res = layer(pts, return_residue=True)
    assert lig.stats["hip_jet_calls"] == n0 + 1, "HIP jet path was not taken"
    st = torch.stack(list(res.values()), 0)
    loss = torch.nn.functional.l1_loss(pred, tgt) + 0.0125 * torch.nn.functional.l1_loss(st, torch.zeros_like(st))
    loss.backward()
    torch.cuda.synchronize()
    grads = {"dW%d" % k: net.fc[k].weight.grad for k in range(6)}
    grads.update({"db%d" % k: net.fc[k].bias.grad for k in range(6)})
    return dict(jets=jets.reshape(jets.shape[0], jets.shape[1], 2, 101), pred=pred.detach(),
                res={k: v.detach() for k, v in res.items()}, dlat=lat.grad, grads=grads, pts=pts, loss=loss.detach())


@pytest.mark.parametrize("act,prec", NAN_CASES)
def test_nan_latent_node_reaches_every_stream_residual_and_gradient(hiplib, monkeypatch, act, prec):
    from space_time_pde_amd import lig_jet
    monkeypatch.setattr(lig_jet, "mlp_precision", prec)
    g = torch.Generator().manual_seed(30)
    lat0 = 0.5 * torch.randn(2, 4, 5, 6, 32, generator=g)
    lat1 = lat0.clone()
    lat1[NODE + (CHANNEL,)] = float("nan")
    clean, bad = _run_net(act, prec, lat0), _run_net(act, prec, lat1)
    assert torch.isfinite(clean["jets"]).all() and torch.isfinite(clean["loss"]) and torch.isfinite(clean["dlat"]).all()
    # points whose cell has the node as a corner: i0 = floor(q / cube), the reference's own fp32 expression
    pts = clean["pts"].cpu()
    cube = 1.0 / (torch.tensor([4., 5., 6.]) - 1)
    i0 = torch.floor(pts / cube).long()
    node = torch.tensor(NODE[1:])
    hit = torch.zeros(2, 101, dtype=torch.bool)
    hit[NODE[0]] = ((i0[NODE[0]] == node) | (i0[NODE[0]] + 1 == node)).all(-1)
    assert 4 <= int(hit.sum()) <= 60
    hit = hit.to(DEV)
    for s in range(bad["jets"].shape[0]):
        js = bad["jets"][s].permute(1, 2, 0)                                        # [b, p, out]
        assert torch.isnan(js[hit]).all(), "stream %d: finite value at a point that touches the NaN node" % s
        assert torch.equal(js[~hit], clean["jets"][s].permute(1, 2, 0)[~hit]), "stream %d" % s
    assert torch.isnan(bad["pred"][hit]).all() and torch.equal(bad["pred"][~hit], clean["pred"][~hit])
    for k, v in bad["res"].items():
        assert torch.isnan(v[hit]).all(), "residual %s" % k
        assert torch.equal(v[~hit], clean["res"][k][~hit]), "residual %s" % k
    assert torch.isnan(bad["loss"])
    assert torch.isnan(bad["dlat"][NODE]).all(), "d latent of the NaN node"
    # Every parameter gradient is NaN in every entry but one: torch's L1 backward is sign(x), 0 at a NaN, and the first output
    # (pressure) enters the RB2 residuals through derivatives only -- so the value-stream adjoint of that output is 0 at the NaN
    # points and d b5[0], a sum of value-stream adjoints alone, is finite in torch's own backward as well.  d W5[0, :] is not:
    # that 0 multiplies fc4's NaN activations.  (ELU's were 0: this row was finite until act_eval_t<ELU> kept the NaN.)
    for k, v in bad["grads"].items():
        nan = torch.isnan(v)
        if k == "db5":
            assert nan[1:].all() and torch.isfinite(v[0]), v
        else:
            assert nan.all(), "%s: %d of %d elements finite" % (k, int(torch.isfinite(v).sum()), v.numel())
