"""Phase-swapped loop order of the exact-fp32 first-hidden-layer weight gradient (csrc/jet_wgrad_impl.h: k_wgrad_coop, MODE 1).

Waves 4 .. 7 of a workgroup -- the second wave of every SIMD -- prepare the next row tile BEFORE the MFMAs of the current one
while their partners run the MFMAs first (stpde_tune "wgrad_fp32_swap": 0 / 1 = swapped, 2 = lock step), and under the swap
every wave fetches its next adjoint operand set in the row-major image straight from memory instead of transposing it through
an LDS patch.  Only data movement and the order of the two phases of an iteration differ: every wave keeps its accumulators,
its tile order and the order of MFMAs into each accumulator, so in deterministic mode (long accumulators, no atomics) every
gradient must be the SAME BITS under both orders, and the same bits from run to run.

Shapes: nf = 32 (KT = 32 hidden k-tiles, MT = 16 output tiles: the benchmarked instantiation, KC = 8), a row tile = 16 corner
rows = 2 query points, all points in one launch chunk.  The launcher walks the tiles with gx workgroup columns (512 / (m-groups x
hidden k-groups), at most one per tile, rounded up to 8); the tile counts below give a workgroup 0 or 1 tiles, exactly 1, exactly
2 (both ring parities), 2 or 3 (ragged), and 5 or 6 (steady state + the branch-free tail that re-produces its own tile).

What this file does NOT see: the phase-swapped loop is compiled for every first-hidden-layer exact-fp32 instantiation with at
most five streams (all six activations, S = (0,0) as well, KC = 8 and 4); the bitwise cases here run softplus and leaky-relu
only.  The dispatch trace names the same instantiation under both settings of the switch, so which loop a launch took is not
observable from Python: the launcher takes the swapped loop when the switch is not 2 and the adjoint buffer holds every stream
(SP == S), which is how lig_jets' backward always calls it (csrc/lig_pipeline.hip: wgrad_l passes S).  `_gx` below restates
the launcher's tile split (launch_wgrad_kc: 512 / (gy * gz), at most one column per tile, rounded up to 8); it does not read it.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_reference_fixtures as F  # noqa: E402  (rel: the max-relative metric of the G5b checks)

from oracle import jet_ref as J  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COMBO = {(1, 1): 1.0, (2, 2): 0.25}       # combined second-order stream: softplus carries S = (3,1), leaky-relu S = (3,0)
SWAPPED, LOCKSTEP = 1, 2


def _gx(ntiles):
    """The tile split of launch_wgrad_kc for the first hidden layer at nf = 32, read from the plan's tile counts."""
    from space_time_pde_amd.lig_jet import ImNetPlan
    lay = ImNetPlan.get(3, 32, 4, 32).layers[1]
    assert (lay["KT"], lay["MT"]) == (32, 16)
    kc = 8                                        # MT >= 16
    gy, gz = -(-lay["MT"] // (2 * kc)), lay["KT"] // 8
    return max(8, -(-min(512 // (gy * gz), ntiles) // 8) * 8)


GX = 128                                          # _gx() of every tile count >= 121 (asserted in the test)
TILES = {"some_none": 5, "one_each": GX, "two_each": 2 * GX, "two_or_three": 2 * GX + 3, "five_or_six": 5 * GX + 37}


def _backward(act, ntiles, swap, det, monkeypatch, nf=32):
    """lig_jets forward + backward of 2 * ntiles points under one setting of the switch -> (gradients, jets, inputs, trace)."""
    from space_time_pde_amd import _lib, implicit_net, lig_jet, nonlinearities
    monkeypatch.setattr(_lib, "deterministic", det)
    P = 2 * ntiles
    g = torch.Generator().manual_seed(100 + ntiles)
    lat = 0.5 * torch.randn(1, 4, 5, 6, 32, generator=g)
    pts = 0.02 + 0.96 * torch.rand(1, P, 3, generator=g)
    cot = torch.randn(5, 4, P, generator=g)       # (the combined stream is returned for leaky-relu too; its MLP carries S = (3,0))
    torch.manual_seed(3)
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=nf, activation=nonlinearities.NONLINEARITIES[act]).to(DEV)
    latd = lat.to(DEV).requires_grad_(True)
    with _lib.tuned(wgrad_fp32_swap=swap), _lib.dispatch_trace() as tr:
        jets, _ = lig_jet.lig_jets(net, latd, pts.to(DEV), 0., 1., True, (), chunk_points=4096, combo=COMBO)
        assert jets.shape == cot.shape, (jets.shape, cot.shape)
        (jets * cot.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    s2 = 1 if act == "softplus" else 0
    dump = "\n".join(tr.kernels)
    assert tr.has("k_wgrad_coop", "false>)", "S1 = 3, S2 = %d" % s2, "MODE = 1", "KC = %d" % (8 if nf == 32 else 4)), dump
    grads = {"dlat": latd.grad.clone()}
    for k in range(6):
        grads["dW%d" % k], grads["db%d" % k] = net.fc[k].weight.grad.clone(), net.fc[k].bias.grad.clone()
    return grads, jets.detach(), (net, lat, pts, cot)


@pytest.mark.parametrize("case", sorted(TILES))
@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
def test_swapped_order_is_bitwise_the_lock_step_order(hiplib, monkeypatch, act, case):
    ntiles = TILES[case]
    gx = _gx(ntiles)
    assert gx == (8 if case == "some_none" else GX)
    lo, hi = ntiles // gx, -(-ntiles // gx)
    assert (lo, hi) == {"some_none": (0, 1), "one_each": (1, 1), "two_each": (2, 2), "two_or_three": (2, 3),
                        "five_or_six": (5, 6)}[case]
    off, _, _ = _backward(act, ntiles, LOCKSTEP, True, monkeypatch)
    on, _, (net, _, _, _) = _backward(act, ntiles, SWAPPED, True, monkeypatch)
    again, _, _ = _backward(act, ntiles, SWAPPED, True, monkeypatch)
    dflt, _, _ = _backward(act, ntiles, 0, True, monkeypatch)
    nh = 16 * 32                                   # fc1.weight = [hidden columns | folded raw-input columns]
    assert net.fc[1].weight.shape[1] > nh and torch.isfinite(on["dW1"]).all() and on["dW1"].abs().max() > 0
    for name in ("hidden", "raw input"):
        cols = slice(0, nh) if name == "hidden" else slice(nh, None)
        assert torch.equal(on["dW1"][:, cols], off["dW1"][:, cols]), "dW1 %s columns: swapped vs lock step" % name
        assert torch.equal(on["dW1"][:, cols], again["dW1"][:, cols]), "dW1 %s columns: swapped, run to run" % name
    for k in on:
        assert torch.equal(on[k], off[k]) and torch.equal(on[k], again[k]) and torch.equal(on[k], dflt[k]), k


@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
def test_swapped_order_at_half_width_is_bitwise_the_lock_step_order(hiplib, monkeypatch, act):
    """nf = 16 (MT = 8 output tiles -> the KC = 4 instantiation: half as many ring blocks per row tile, so TWO dwords of the next
    adjoint set are requested in front of each block of MFMAs; 512 / 2 k-groups = 256 workgroup columns): 2 or 3 tiles each."""
    ntiles = 2 * 256 + 3
    off, _, _ = _backward(act, ntiles, LOCKSTEP, True, monkeypatch, nf=16)
    on, _, _ = _backward(act, ntiles, SWAPPED, True, monkeypatch, nf=16)
    again, _, _ = _backward(act, ntiles, SWAPPED, True, monkeypatch, nf=16)
    assert torch.isfinite(on["dW1"]).all() and on["dW1"].abs().max() > 0
    for k in on:
        assert torch.equal(on[k], off[k]) and torch.equal(on[k], again[k]), k


def test_swapped_order_with_fp32_atomics_matches_the_fp64_oracle(hiplib, monkeypatch):
    """Default (fp32-atomic) flush, switch on, softplus, the ragged 2-or-3-tile split: dW1 (and every other gradient) against the
    fp64 oracle at the G5b bound, 5e-4 max-relative."""
    ntiles = TILES["two_or_three"]
    got, jets, (net, lat, pts, cot) = _backward("softplus", ntiles, SWAPPED, False, monkeypatch)
    p64 = [(net.fc[k].weight.detach().double().cpu().requires_grad_(True),
            net.fc[k].bias.detach().double().cpu().requires_grad_(True)) for k in range(6)]
    lat64 = lat.double().requires_grad_(True)
    pairs = tuple(sorted(COMBO))
    full = J.lig_jets(p64, "softplus", lat64, pts.double(), 0., 1., second=pairs)
    full = full.permute(0, 3, 1, 2).reshape(full.shape[0], 4, -1)
    ref = torch.cat([full[:4], sum(COMBO[p] * full[4 + k] for k, p in enumerate(pairs))[None]], 0)
    (ref * cot.double()).sum().backward()
    err = {"dlat": F.rel(got["dlat"].cpu(), lat64.grad)}
    for k in range(6):
        err["dW%d" % k] = F.rel(got["dW%d" % k].cpu(), p64[k][0].grad)
        err["db%d" % k] = F.rel(got["db%d" % k].cpu(), p64[k][1].grad)
    print("max-relative error vs fp64:", {k: "%.2e" % v for k, v in err.items()})
    assert F.rel(jets.cpu(), ref.detach()) < 5e-4
    assert err["dW1"] < 5e-4, err
    assert max(err.values()) < 5e-4, err
