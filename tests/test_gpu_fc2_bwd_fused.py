"""Fused exact-fp32 backward of the second hidden layer (csrc/jet_fc2_bwd.hip: k_fc2_bwd_fused).

One eight-wave workgroup per row tile produces fc2's weight gradient AND the adjoint of fc1's rows.  A call asks for it
(lig_jet.fc2_fused -> STPDE_F_FC2_FUSED: the training step train_step.sharded_step does, a direct jet call does not unless the
module switch is set, as every case here sets it); stpde_tune "fc2_bwd_fused": 0 / 1 = fused for such a call where
stpde_jet_fc2_bwd_supported says so and weight gradients are asked for, 2 = k_wgrad_quad<..., 8> + k_layer_coop<..., PRO_NONE,
EPI_ADJ, ...>.  Wave w keeps the weight gradient's accumulators, tile order and MFMA order, and
forms output tiles 2w, 2w + 1 of W2^T abar2 in the order of k_layer_coop's main loop (contraction tile ascending, k-step
ascending) before the same layer_epilogue; so in deterministic mode (long accumulators, no fp32 atomics) every gradient must be
the SAME BITS under both settings, and the same bits from run to run.

Shapes: nf = 32 (fc2: KT = 16 input k-tiles, MT = 8 output tiles), a row tile = 16 corner rows = 2 query points, all points in one
launch chunk.  The kernel is persistent over min(256, ntiles) workgroups, tile = blockIdx.x + i * gridDim.x; the tile counts give
a launch of fewer workgroups than CUs (5), exactly one tile each, exactly two, two or three (ragged) and five or six (steady state
plus the last iteration that re-requests its own tile).

In-place safety: the one-call order (lig_jets' default driver, which every case here takes) writes abar1 over the stash of
fc1's rows, block by block, by the wave that read the block.  dW1, dW0 and d latent are computed from abar1 afterwards, so the
bitwise cases below are the check that no block was overwritten before its reader was done with it.

What this file does NOT see: the kernel is compiled for all six activations; the bitwise cases run softplus (S = (3,1)) and
leaky-relu (S = (3,0)).  Swish's beta adjoint is a sum of fp32 atomics over another workgroup split than the two kernels', not
the same bits.
"""
import functools
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
FUSED, SPLIT = 1, 2
NWG = 256                                 # persistent workgroups of the kernel (launch_fc2_fused: min(256, ntiles))
TILES = {"some_none": 5, "one_each": NWG, "two_each": 2 * NWG, "two_or_three": 2 * NWG + 3, "five_or_six": 5 * NWG + 37}
G5B = 5e-4                                # the project's max-relative bound against the fp64 oracle


def _inputs(ntiles, nf, act):
    from space_time_pde_amd import implicit_net, nonlinearities
    P = 2 * ntiles
    g = torch.Generator().manual_seed(100 + ntiles)
    lat = 0.5 * torch.randn(1, 4, 5, 6, 32, generator=g)
    pts = 0.02 + 0.96 * torch.rand(1, P, 3, generator=g)
    cot = torch.randn(5, 4, P, generator=g)       # (the combined stream is returned for leaky-relu too; its MLP carries S = (3,0))
    torch.manual_seed(3)
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=nf, activation=nonlinearities.NONLINEARITIES[act]).to(DEV)
    return net, lat, pts, cot


def _backward(act, ntiles, switch, det, monkeypatch, nf=32, precision=None, wgrad=True, profile=None, ask=True):
    """lig_jets forward + backward of 2 * ntiles points under one setting of the switch -> (gradients, jets, trace).
    profile: a dict makes lig_jet take its per-kernel driver and time every launch into it (what bench.py --full does);
    ask: lig_jet.fc2_fused of the call (None = the module default of a direct call)."""
    from space_time_pde_amd import _lib, lig_jet
    monkeypatch.setattr(_lib, "deterministic", det)
    monkeypatch.setattr(lig_jet, "profile", profile)
    monkeypatch.setattr(lig_jet, "fc2_fused", ask)
    net, lat, pts, cot = _inputs(ntiles, nf, act)
    if not wgrad:
        for p in net.parameters():
            p.requires_grad_(False)
    latd = lat.to(DEV).requires_grad_(True)
    with _lib.tuned(fc2_bwd_fused=switch), _lib.dispatch_trace() as tr:
        jets, _ = lig_jet.lig_jets(net, latd, pts.to(DEV), 0., 1., True, (), chunk_points=4096, combo=COMBO, precision=precision)
        assert jets.shape == cot.shape, (jets.shape, cot.shape)
        (jets * cot.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    grads = {"dlat": latd.grad.clone()}
    if wgrad:
        for k in range(6):
            grads["dW%d" % k], grads["db%d" % k] = net.fc[k].weight.grad.clone(), net.fc[k].bias.grad.clone()
    return grads, jets.detach(), tr


def _took_fused(tr):
    return tr.has("k_fc2_bwd_fused")


def _took_split(tr):
    """the eight-wave weight-gradient launch and the hidden-layer input-gradient launch of the cooperative layer kernel (fc2's is
    the only one: fc3 .. fc5 run in the fused tail kernel, fc1's is EPI = 2)"""
    return tr.has("k_wgrad_quad", "false, 8>)"), tr.has("k_layer_coop", "PRO = 0, EPI = 1,")


@functools.lru_cache(maxsize=None)
def _oracle(ntiles, nf):
    """fp64 gradients and jets of the softplus case (oracle/jet_ref.py), computed once per shape and shared"""
    net, lat, pts, cot = _inputs(ntiles, nf, "softplus")
    p64 = [(net.fc[k].weight.detach().double().cpu().requires_grad_(True),
            net.fc[k].bias.detach().double().cpu().requires_grad_(True)) for k in range(6)]
    lat64 = lat.double().requires_grad_(True)
    pairs = tuple(sorted(COMBO))
    full = J.lig_jets(p64, "softplus", lat64, pts.double(), 0., 1., second=pairs)
    full = full.permute(0, 3, 1, 2).reshape(full.shape[0], 4, -1)
    ref = torch.cat([full[:4], sum(COMBO[p] * full[4 + k] for k, p in enumerate(pairs))[None]], 0)
    (ref * cot.double()).sum().backward()
    grads = {"dlat": lat64.grad}
    for k in range(6):
        grads["dW%d" % k], grads["db%d" % k] = p64[k][0].grad, p64[k][1].grad
    return grads, ref.detach()


def _errors(got, jets, ntiles, nf):
    ref, jets64 = _oracle(ntiles, nf)
    err = {k: F.rel(got[k].cpu(), ref[k]) for k in got}
    err["jets"] = F.rel(jets.cpu(), jets64)
    print("max-relative error vs fp64:", {k: "%.2e" % v for k, v in sorted(err.items())})
    return err


@pytest.mark.parametrize("case", sorted(TILES))
@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
def test_fused_is_bitwise_the_two_kernels(hiplib, monkeypatch, act, case):
    """Deterministic mode: switch 2 against switch 1, fused twice (run to run), and switch 0 -- every gradient torch.equal.
    This is also the in-place check: abar1 goes over the stash of fc1's rows, and dW1, dW0 and d latent -- the consumers of
    abar1 -- are among the gradients compared."""
    ntiles = TILES[case]
    lo, hi = ntiles // min(NWG, ntiles), -(-ntiles // min(NWG, ntiles))
    assert (lo, hi) == {"some_none": (1, 1), "one_each": (1, 1), "two_each": (2, 2), "two_or_three": (2, 3),
                        "five_or_six": (5, 6)}[case]
    off, _, tr_off = _backward(act, ntiles, SPLIT, True, monkeypatch)
    on, _, tr_on = _backward(act, ntiles, FUSED, True, monkeypatch)
    again, _, _ = _backward(act, ntiles, FUSED, True, monkeypatch)
    dflt, _, tr_dflt = _backward(act, ntiles, 0, True, monkeypatch)
    assert _took_fused(tr_on) and _took_fused(tr_dflt) and not _took_fused(tr_off)
    for name in ("dW2", "dW1", "dW0", "dlat"):
        assert torch.isfinite(on[name]).all() and on[name].abs().max() > 0, name
    for k in on:
        assert torch.equal(on[k], off[k]), "%s: fused vs the two kernels" % k
        assert torch.equal(on[k], again[k]), "%s: fused, run to run" % k
        assert torch.equal(on[k], dflt[k]), "%s: switch 1 vs switch 0" % k


@pytest.mark.parametrize("act", ["softplus", "leakyrelu"])
def test_dispatch_follows_the_switch(hiplib, monkeypatch, act):
    s2 = 1 if act == "softplus" else 0
    for switch in (0, FUSED):
        _, _, tr = _backward(act, TILES["some_none"], switch, True, monkeypatch)
        dump = "\n".join(tr.kernels)
        assert tr.has("k_fc2_bwd_fused", "S1 = 3, S2 = %d" % s2), dump
        assert _took_split(tr) == (False, False), dump
    _, _, tr = _backward(act, TILES["some_none"], SPLIT, True, monkeypatch)
    dump = "\n".join(tr.kernels)
    assert not _took_fused(tr), dump
    assert _took_split(tr) == (True, True), dump


def test_a_direct_call_asks_for_it_or_keeps_the_two_kernels(hiplib, monkeypatch):
    """lig_jet.fc2_fused = None (the module default) or False: a direct jet call keeps the two kernels under every setting of the
    library switch -- the instantiations the parity fixtures pin; same bits as a call that asks."""
    ntiles = TILES["two_or_three"]
    asked, _, tr = _backward("softplus", ntiles, 0, True, monkeypatch)
    assert _took_fused(tr)
    for ask in (None, False):
        got, _, tr = _backward("softplus", ntiles, 0, True, monkeypatch, ask=ask)
        assert not _took_fused(tr) and _took_split(tr) == (True, True), "\n".join(tr.kernels)
        for k in got:
            assert torch.equal(got[k], asked[k]), k


def test_the_training_step_takes_it(hiplib, monkeypatch):
    """train_step.sharded_step (what bench.py times) asks for the fused kernel on its own; under switch 2 it runs the two kernels,
    with the same bits in deterministic mode.  U-Net in evaluation mode (running statistics: no state changes between the runs)."""
    from space_time_pde_amd import _lib, implicit_net, lig_jet, physics, unet3d
    from space_time_pde_amd.train_step import sharded_step
    monkeypatch.setattr(_lib, "deterministic", True)
    assert lig_jet.fc2_fused is None
    kw = dict(mean=(0.01, 0.0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1., x_crop=1., use_continuity=True)
    torch.manual_seed(5)
    net = implicit_net.ImNet(nf=32, activation=torch.nn.Softplus).to(DEV)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=(4, 8, 8), nf=16, mf=64).to(DEV).eval()
    crop = torch.randn(1, 4, 4, 8, 8, device=DEV)
    pts = (0.02 + 0.96 * torch.rand(1, 518, 3)).to(DEV)
    tgt = torch.randn(1, 518, 4).to(DEV)
    layer = physics.get_rb2_pde_layer(**kw)
    out = {}
    for switch in (0, SPLIT):
        for p in list(net.parameters()) + list(unet.parameters()):
            p.grad = None
        with _lib.tuned(fc2_bwd_fused=switch), _lib.dispatch_trace() as tr:
            loss, _, _ = sharded_step(unet, net, layer, crop, pts, tgt, pts.shape[1], 1.0, 0.0125, "l1")
            torch.cuda.synchronize()
        assert lig_jet.fc2_fused is None                      # (the step restores the module default)
        assert _took_fused(tr) == (switch == 0), "\n".join(tr.kernels)
        assert _took_split(tr) == ((False, False) if switch == 0 else (True, True)), "\n".join(tr.kernels)
        out[switch] = [loss.clone()] + [p.grad.clone() for p in list(net.parameters()) + list(unet.parameters()) if p.grad is not None]
    assert len(out[0]) == len(out[SPLIT]) > 12 and torch.isfinite(out[0][0])
    for a, b in zip(out[0], out[SPLIT]):
        assert torch.equal(a, b)


def test_per_kernel_driver_follows_the_switch(hiplib, monkeypatch):
    """The per-kernel driver (here: while it profiles) takes the fused call under the name ``layer2_bwd`` (switch 0) and the two
    kernels under switch 2; same bits from both, and the same bits as the one-call driver's."""
    ntiles = TILES["two_or_three"]
    prof_on, prof_off = {}, {}
    on, _, tr_on = _backward("softplus", ntiles, 0, True, monkeypatch, profile=prof_on)
    off, _, tr_off = _backward("softplus", ntiles, SPLIT, True, monkeypatch, profile=prof_off)
    one_call, _, _ = _backward("softplus", ntiles, 0, True, monkeypatch)
    assert "layer2_bwd" in prof_on and "layer2_wgrad" not in prof_on and "layer2_dgrad" not in prof_on, sorted(prof_on)
    assert "layer2_bwd" not in prof_off and "layer2_wgrad" in prof_off and "layer2_dgrad" in prof_off, sorted(prof_off)
    assert _took_fused(tr_on) and not _took_fused(tr_off)
    for k in on:
        assert torch.equal(on[k], off[k]), "%s: per-kernel driver, fused vs the two kernels" % k
        assert torch.equal(on[k], one_call[k]), "%s: per-kernel driver vs one-call driver" % k


def test_not_taken_without_weight_gradients(hiplib, monkeypatch):
    """A latent-only backward (no parameter requires a gradient) runs fc2's input gradient alone."""
    ntiles = TILES["two_or_three"]
    lat_only, _, tr = _backward("softplus", ntiles, FUSED, True, monkeypatch, wgrad=False)
    dump = "\n".join(tr.kernels)
    assert not _took_fused(tr) and not tr.has("k_wgrad_quad"), dump
    assert tr.has("k_layer_coop", "PRO = 0, EPI = 1,"), dump
    assert torch.isfinite(lat_only["dlat"]).all() and lat_only["dlat"].abs().max() > 0


@pytest.mark.parametrize("variant", ["nf16", "fp32x3"])
def test_not_taken_outside_the_envelope(hiplib, monkeypatch, variant):
    """Half width (fc2: 8 x 4 tiles) and the three-term split mode keep their own kernels, and still match the fp64 oracle."""
    ntiles = TILES["two_or_three"]
    nf, precision = (16, None) if variant == "nf16" else (32, "fp32x3")
    got, jets, tr = _backward("softplus", ntiles, FUSED, False, monkeypatch, nf=nf, precision=precision)
    assert not _took_fused(tr), "\n".join(tr.kernels)
    err = _errors(got, jets, ntiles, nf)
    assert max(err.values()) < G5B, err


def test_fused_with_fp32_atomics_matches_the_fp64_oracle(hiplib, monkeypatch):
    """Default (fp32-atomic) flush, fused kernel on, softplus, the ragged 2-or-3-tile split: every gradient against the fp64
    oracle at the G5b bound, 5e-4 max-relative."""
    ntiles = TILES["two_or_three"]
    got, jets, tr = _backward("softplus", ntiles, FUSED, False, monkeypatch)
    assert _took_fused(tr), "\n".join(tr.kernels)
    err = _errors(got, jets, ntiles, 32)
    assert err["dW2"] < G5B and err["dW1"] < G5B, err
    assert max(err.values()) < G5B, err
