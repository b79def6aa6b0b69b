"""Element-wise gradients of the FULL-SIZE step: 2^20 query points in one launch, the geometry bench.py times.

tests/test_gpu_interp_generic.py checks predictions and residuals of a full-size step against the oracle, its gradients only
through additivity over the two halves of the points.  Here every gradient element of the 2^20-point single-launch step --
dW0..dW5, db0..db5, d latent -- is compared

  (a) with the fp64 oracle, through a cotangent that is non-zero on exactly 1,024 points chosen to sit on the launch's edges:
      first / last row tiles, both sides of every 2^32-byte and of the first 2^31-element boundary of the largest stash and
      adjoint buffers, first / last tile of the last persistent workgroup's share;
  (b) with the same step run in 4,096-point launch chunks (256 launches; at <= 4,096 points the gradients already meet the
      oracle and the reference vectors: G5b, test_benchmarked_instantiations_backward_vs_fp64_oracle), with the full cotangent.

The loss is LINEAR in the outputs, L = sum_i m_i (c_i . pred_i + 0.0125 sum_k d_ik res_k,i) / N with fixed random c, d: an L1 loss
puts a sign flip on every near-zero residual, and one flipped sign among 1,024 kept points is larger than the fp32 tolerance
(the L1 / loss-sum kernels are pinned in tests/test_residual_program.py).

Tolerances of (a): the G5b ones, same metrics (fp32, fp32x3: 5e-4 max-relative; bf16: 3e-2 Frobenius).  On the 128-wide grid the
second derivatives carry 127^2 and the fp32 REFERENCE itself is only good to ~2e-4 of the residual scale per point, so the fp32
modes are allowed max(5e-4, 4 x the oracle's own fp32-vs-fp64 distance of that tensor) -- the oracle is evaluated in fp32 and in
fp64 on the same points; the factor 4 covers the order of summation (8 corners x 6 layers x MFMA k-order), nothing else.
Tolerances of (b): the additivity bounds of test_full_size_step_subset_vs_oracle_and_additivity (1e-4 max|d latent|, 2e-4
max|g| per parameter tensor): both runs sum the same fp32 terms in another order.

The oracle's own fp32-vs-fp64 distances, per tensor and per case (2e-7 ... 1.9e-5 max-relative: the bound is 5e-4 throughout),
and the sensitivity of (a) to ONE misplaced cotangent row (3e-3 ... 5e-2 on the weight gradients): profiles/
full_size_gradient_parity.txt.  The test prints every distance before it asserts (pytest -s).  Chunk size of (b): 4,096, the
size at which test_config0_c1_step_on_hip_matches_reference pins the gradients of a whole step against the reference."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_reference_fixtures import (_assert_benchmarked_kernels, _assert_mode_kernels, _normerr,  # noqa: E402
                                         _relerr)

from oracle import cpu_ref as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 1 << 20
NT = N // 2                 # row tiles of the launch (a row tile = 2 points)
KEEP = 1024
CHUNK = 4096
RB2 = dict(mean=(0.01, 0.0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1., x_crop=1., use_continuity=True)

CASES = [
    pytest.param("rb2", (32, 128, 128), "fp32", False, id="configs1-fp32-atomics"),
    pytest.param("rb2", (32, 128, 128), "fp32", True, id="configs1-fp32-det"),
    pytest.param("rb2", (32, 128, 128), "fp32x3", True, id="fp32x3-det"),
    pytest.param("rb2", (32, 128, 128), "bf16", True, id="bf16-det"),
    pytest.param("rb2", (64, 256, 256), "bf16", True, id="configs3-bf16-det"),
    pytest.param("c5", (32, 128, 128), "fp32", True, id="configs4-fp32-det"),
]


def _setup(eqs, grid):
    """The step of test_full_size_step_subset_vs_oracle_and_additivity (rb2) / test_config5_full_size_properties (c5): same
    seeds, ImNet(nf = 32, Softplus), N = 2^20 points; plus the fixed random coefficients c, d of the linear loss."""
    from space_time_pde_amd import implicit_net, pde, physics
    seed = 0 if eqs == "rb2" else 5
    g = torch.Generator().manual_seed(seed)
    lat0 = 0.5 * torch.randn(1, *grid, 32, generator=g)
    pts = torch.rand(1, N, 3, generator=g)
    torch.manual_seed(seed)
    if eqs == "rb2":
        net = implicit_net.ImNet(nf=32, activation=torch.nn.Softplus).to(DEV)
        layer = physics.get_rb2_pde_layer(**RB2)
        oracle = O.rb2_oracle(**RB2)
        names = [n for n, _ in O.rb2_equations(**RB2)[2]]
    else:
        import bench
        net = implicit_net.ImNet(dim=3, in_features=32, out_features=5, nf=32, activation=torch.nn.Softplus).to(DEV)
        layer = bench.c5_layer(pde)
        oracle = O.PDEOracle(*bench.C5_VARS)
        for name, eq in bench.C5_EQS.items():
            oracle.add_equation(eq, name)
        names = list(bench.C5_EQS)
    gc = torch.Generator().manual_seed(4242)
    c = torch.randn(1, N, net.out_features, generator=gc)
    d = {k: torch.randn(1, N, 1, generator=gc) for k in sorted(names)}
    return net, layer, oracle, lat0, pts, c, d


def _boundary_tiles(floats_per_tile):
    """Row tiles on either side of every multiple of 2^32 BYTES and of the first 2^31-ELEMENT boundary of a buffer that holds
    ``floats_per_tile`` fp32 per row tile: the tile the boundary falls into (or starts) and both of its neighbours."""
    total = NT * floats_per_tile
    marks = [k * (1 << 30) for k in range(1, total * 4 // (1 << 32) + 1)]      # in floats
    if total > 1 << 31:
        marks.append(1 << 31)
    tiles = set()
    for e in marks:
        t = e // floats_per_tile
        tiles.update(u for u in (t - 1, t, t + 1) if 0 <= u < NT)
    return marks, tiles


def _share_tiles():
    """First and last tile of the LAST workgroup's share when 256 / 512 / 1024 persistent workgroups split the NT tiles into
    contiguous runs and when workgroup w takes every G-th tile from w on."""
    out = set()
    for G in (256, 512, 1024):
        run = -(-NT // G)
        out |= {(G - 1) * run, min(G * run, NT) - 1}                  # contiguous
        out |= {G - 1, (NT - 1) - ((NT - 1) - (G - 1)) % G}           # strided
    return out


def _kept_points(meta):
    """Exactly KEEP point indices: both points of every edge tile, the rest drawn at random (seeded) over the whole launch."""
    from space_time_pde_amd import lig_jet
    # the largest stash and the largest adjoint buffer of one row tile (2 points), from the table the drivers allocate from
    stash = max(n for _, n, _ in lig_jet._forward_buffers(meta, 2))
    adj = max(n for name, n, _ in lig_jet._backward_buffers(meta, 2) if name.startswith("abar"))
    fwd, bwd = lig_jet._per_point_bytes(meta)
    assert 4 * stash <= 2 * fwd and 4 * adj <= 2 * bwd        # both are buffers the memory plan accounts for (tile = 2 points)
    groups = {"first / last row tiles": {0, 1, NT - 2, NT - 1}, "persistent shares": _share_tiles()}
    for what, fl in (("stash", stash), ("adjoint", adj)):
        marks, tiles = _boundary_tiles(fl)
        assert marks and len(tiles) >= 2 * len(marks), (what, fl)      # a 2^20-point launch crosses 2^32 bytes in both
        groups["%s buffer, %d floats per tile, %d boundaries" % (what, fl, len(marks))] = tiles
    edge = sorted(set().union(*groups.values()))
    idx = set()
    for t in edge:
        idx |= {2 * t, 2 * t + 1}
    assert len(idx) < KEEP
    for p in torch.randperm(N, generator=torch.Generator().manual_seed(99)).tolist():
        if len(idx) == KEEP:
            break
        idx.add(p)
    return torch.tensor(sorted(idx)), groups


def _oracle_grads(oracle, params, lat0, pts_sel, c_sel, d_sel, dtype):
    """Gradients of sum_i (c_i . pred_i + 0.0125 sum_k d_ik res_k,i) / N over the kept points from the oracle in ``dtype``.

    The oracle's query_lig gathers the corner latents from the dense grid, and every reverse sweep through that gather makes a
    dense grid-sized gradient (minutes on the 512 MiB grid).  Its four lines are restated here with the gather taken from the
    table of the nodes the kept points touch: cpu_ref.interp_coefficients run on a grid of NODE NUMBERS says which nodes those
    are (and supplies weights and relative coordinates as in query_lig); the forward is checked against cpu_ref.query_lig bit
    for bit.  Returns ({name: gradient}, node numbers): 'dlatent' is [nodes, channels], rows in the order of the node numbers."""
    plist = [(w.detach().to(dtype).clone().requires_grad_(True), b.detach().to(dtype).clone().requires_grad_(True))
             for w, b in params]
    act = O.activation_fn("softplus")
    n_nodes = lat0[..., 0].numel()
    numbers = torch.arange(n_nodes, dtype=torch.float64).reshape(lat0.shape[:-1] + (1,))       # (exact: < 2^53)
    q0 = pts_sel.to(dtype)
    corner = O.interp_coefficients(numbers, q0, 0., 1.)[0][..., 0].long()                      # [1, p, 8]
    nodes, inv = torch.unique(corner, return_inverse=True)
    table = lat0.reshape(n_nodes, -1)[nodes].to(dtype).requires_grad_(True)

    def model(x):
        return O.imnet_forward(plist, x, act)

    def query(q):
        _, w, rel = O.interp_coefficients(numbers, q, 0., 1.)
        feat = torch.cat([rel, table[inv]], dim=-1)
        shp = feat.shape
        out = model(feat.reshape(-1, shp[-1])).reshape(shp[0], shp[1], shp[2], -1)
        return torch.sum(out * w.unsqueeze(-1), dim=-2)

    with torch.no_grad():
        assert torch.equal(query(q0), O.query_lig(model, lat0.to(dtype), q0, 0., 1.))
    oracle.forward_method = query
    y, res = oracle(q0.clone())
    loss = ((y * c_sel.to(dtype)).sum() + 0.0125 * sum((res[k] * d_sel[k].to(dtype)).sum() for k in d_sel)) / N
    loss.backward()
    out = {"dlatent": table.grad}
    for k, (w, b) in enumerate(plist):
        out["dW%d" % k], out["db%d" % k] = w.grad, b.grad
    return out, nodes


@pytest.mark.parametrize("eqs,grid,prec,det", CASES)
def test_full_size_gradients_elementwise(hiplib, eqs, grid, prec, det, monkeypatch):
    from space_time_pde_amd import _lib, lig_jet, local_implicit_grid as lig
    monkeypatch.setattr(lig_jet, "mlp_precision", prec)
    monkeypatch.setattr(_lib, "deterministic", det)
    net, layer, oracle, lat0, pts, c, d = _setup(eqs, grid)
    latd, ptsd, cd = lat0.to(DEV), pts.to(DEV), c.to(DEV)
    dd = {k: v.to(DEV) for k, v in d.items()}
    names = ["dlatent"] + [n % k for k in range(6) for n in ("dW%d", "db%d")]
    seen = {}
    real_lig_jets, real_stash_bytes = lig_jet.lig_jets, lig_jet._stash_bytes

    def spy_jets(*a, **kw):
        jets, pairs = real_lig_jets(*a, **kw)
        seen["jets"] = jets.detach().clone()
        return jets, pairs

    def spy_stash(meta, P):
        seen["meta"] = meta
        return real_stash_bytes(meta, P)

    monkeypatch.setattr(lig_jet, "lig_jets", spy_jets)
    monkeypatch.setattr(lig_jet, "_stash_bytes", spy_stash)

    def run(mask):
        lat = latd.clone().requires_grad_(True)
        for p in net.parameters():
            p.grad = None
        layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, lat, q, 0., 1.))
        n0 = lig.stats["hip_jet_calls"]
        pred, res = layer(ptsd)
        assert lig.stats["hip_jet_calls"] == n0 + 1 and sorted(res) == sorted(dd)
        per_point = (pred * cd).sum(-1, keepdim=True) + 0.0125 * sum(res[k] * dd[k] for k in dd)
        ((per_point if mask is None else per_point * mask).sum() / N).backward()
        torch.cuda.synchronize()
        out = {"dlatent": lat.grad}
        for k in range(6):
            out["dW%d" % k], out["db%d" % k] = net.fc[k].weight.grad.clone(), net.fc[k].bias.grad.clone()
        return out, seen.pop("jets")

    # ---- (b) one 2^20-point launch vs 4,096-point launch chunks, full cotangent ----------------------------------------------------
    r0 = lig_jet.stats["recompute_steps"]
    with _lib.dispatch_trace() as tr:
        one, jets_one = run(None)
    dump = "\n".join(sorted(set(tr.kernels)))
    if eqs == "c5":
        assert tr.has("S1 = 3, S2 = 4") and tr.has("k_residual_bwd") and tr.has("k_tail_fwd") and tr.has("k_tail_bwd"), dump
        assert not tr.has("S1 = 3, S2 = 6"), dump
        print("configs[4] full size: recompute path taken =", lig_jet.stats["recompute_steps"] > r0)
    else:
        if prec == "fp32":
            _assert_benchmarked_kernels(tr, "softplus")
        else:
            _assert_mode_kernels(tr, prec)
        assert lig_jet.stats["recompute_steps"] == r0, "the stash path is the one under test"
    meta = seen["meta"]
    assert meta.chunk >= N or eqs == "c5", meta.chunk                 # ONE launch (configs[4]: the memory plan may split it)
    one_launch = lig_jet.DEFAULT_CHUNK
    monkeypatch.setattr(lig_jet, "DEFAULT_CHUNK", CHUNK)
    many, jets_many = run(None)
    assert seen["meta"].chunk == CHUNK
    monkeypatch.setattr(lig_jet, "DEFAULT_CHUNK", one_launch)
    assert torch.equal(jets_one, jets_many), "forward jets: one launch vs %d-point chunks" % CHUNK
    del jets_one, jets_many
    report = ["%s grid %s %s det=%s" % (eqs, grid, prec, det)]
    fails = []
    for n in names:
        scale = one[n].abs().max().item()
        dist = (one[n] - many[n]).abs().max().item() / scale
        bound = 1e-4 if n == "dlatent" else 2e-4
        report.append("  (b) %-8s one launch vs %d-point chunks: max-abs / max|g| = %.3e (bound %.0e)" % (n, CHUNK, dist, bound))
        if not dist < bound:
            fails.append(report[-1])
    del many

    # ---- (a) cotangent on 1,024 edge + random points vs the fp64 oracle on those points ------------------------------------------
    sel, groups = _kept_points(meta)
    kept_tiles = set((sel // 2).tolist())
    for what, tiles in groups.items():
        assert tiles and tiles <= kept_tiles, what
        report.append("  kept: %s: %d tiles" % (what, len(tiles)))
    mask = torch.zeros(1, N, 1)
    mask[0, sel] = 1.
    assert int(mask.sum()) == KEEP == sel.numel()
    got, _ = run(mask.to(DEV))
    params = [(net.fc[k].weight.detach().cpu(), net.fc[k].bias.detach().cpu()) for k in range(6)]
    args = (oracle, params, lat0, pts[:, sel], c[:, sel], {k: v[:, sel] for k, v in d.items()})
    ref64, nodes = _oracle_grads(*args, torch.float64)
    ref32, nodes32 = _oracle_grads(*args, torch.float32)
    assert torch.equal(nodes, nodes32)
    # d latent: compared on the nodes the kept points touch, exactly zero on every other node
    gl = got["dlatent"].reshape(-1, lat0.shape[-1])
    nodes_d = nodes.to(DEV)
    got["dlatent"] = gl[nodes_d].clone()
    gl[nodes_d] = 0
    stray = int((gl != 0).sum())
    report.append("  (a) d latent: %d nodes touched, %d non-zero entries elsewhere" % (nodes.numel(), stray))
    if stray:
        fails.append(report[-1])
    bf = prec == "bf16"
    err = _normerr if bf else _relerr
    for n in names:
        own = err(ref32[n], ref64[n])                  # the reference's own fp32 error on these points, same metric
        tol = 3e-2 if bf else max(5e-4, 4 * own)
        e = err(got[n], ref64[n])
        report.append("  (a) %-8s HIP vs fp64 oracle %.3e   oracle fp32 vs fp64 %.3e   bound %.3e   (%s)"
                      % (n, e, own, tol, "Frobenius" if bf else "max-rel"))
        if not e < tol:
            fails.append(report[-1])
    print("\n".join(report))
    assert not fails, "\n".join(fails)
