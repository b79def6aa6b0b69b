"""Non-finite addends in the long accumulators of the deterministic mode (csrc/common.h: det_add_f32 / det_add_f64 /
det_add_pieces / det_value), through the public C ABI and the Python entry points that sit on it.

A NaN, an infinity or a value too large for the windows MARKS the accumulator, and a marked accumulator reads back as NaN
whatever else was added to it and however many marks it took.  The mark used to be an atomic ADD of 2^62 to the top window:
four marks summed to 2^64 = 0 (mod 2^64) and the accumulator read back FINITE -- and the persistent grids add one partial per
workgroup (k_loss_sum: 1024 blocks at n >= 2^20), so "everything upstream is NaN", the ordinary way a run diverges, gave a
multiple of four marks and a loss of exactly 0.0.  (By the arithmetic of the additive mark: all-NaN input -> 0.0 for every loss
kind, NaN in four blocks -> the finite sum of the other elements, one NaN -> NaN.)  The mark is an atomic MAX now: idempotent.
tests/test_det_accumulator_model.py restates both schemes on the host.

These tests feed NaN / Inf DATA to kernels: ordinary arithmetic, every index in bounds."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")

# k_loss_sum (csrc/residual.hip): 256 threads per block, grid-stride loop, min(ceil(n / 1024), 1024) blocks.  At n = 2^20 that
# is 1024 blocks, and element i is summed by block (i // 256) % 1024: the indices 0, 256, 512, 768 lie in the four different
# blocks 0, 1, 2, 3, each of which adds ONE partial sum to the accumulator.
LOSS_N = 1 << 20
LOSS_CASES = {
    "all_nan": None,
    "one_nan": [(123457, NAN)],
    "nan_in_four_blocks": [(0, NAN), (256, NAN), (512, NAN), (768, NAN)],
    "one_inf": [(777, INF)],
    "inf_and_neg_inf": [(777, INF), (300001, -INF)],
}


def _loss_block(i):
    return (i // 256) % min((LOSS_N + 1023) // 1024, 1024)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("case", list(LOSS_CASES))
@pytest.mark.parametrize("kind", ["l1", "l2", "huber"])
def test_loss_sum_of_non_finite_input_is_not_finite(hiplib, monkeypatch, kind, case, det):
    """train_step.loss_sum on 2^20 elements: the result is not finite in every case, and NaN whenever torch's fp64 sum of the
    same data is NaN -- in deterministic mode (long accumulator + stpde_det_finalize) as in the default one (fp32 atomics: the
    control)."""
    from space_time_pde_amd import _lib, train_step as T
    monkeypatch.setattr(_lib, "deterministic", det)
    g = torch.Generator().manual_seed(11)
    a = 2.0 * torch.randn(LOSS_N, generator=g)
    if LOSS_CASES[case] is None:
        a.fill_(NAN)
    else:
        for i, v in LOSS_CASES[case]:
            a[i] = v
        if case == "nan_in_four_blocks":
            assert len({_loss_block(i) for i, _ in LOSS_CASES[case]}) == 4
    want = T._LOSS_SUMS[kind](a.double(), torch.zeros(LOSS_N, dtype=torch.float64)).item()
    assert not math.isfinite(want)
    got = T.loss_sum(a.to(DEV), None, kind).item()
    print("loss_sum[%s, %s, det=%s] = %r (fp64: %r)" % (kind, case, det, got, want))
    assert not math.isfinite(got), got
    if math.isnan(want):
        assert math.isnan(got), got


@pytest.mark.parametrize("nbad", [1, 2, 4, 300_000])
def test_conv_wgrad_long_accumulator_marks_stay_in_their_accumulator(hiplib, nbad):
    """stpde_conv3d_wgrad with det = 1 + stpde_det_finalize, shaped like test_long_accumulator_finalize_matches_fp64 (1x1x1,
    16 -> 16 channels, 300,000 voxels): NaN in 1, 2, 4 and all voxels of ONE input channel -> the 16 weight-gradient entries of
    that channel are NaN and the other 240 still equal the fp64 sum to that test's bound (a mark does not leak into a
    neighbouring accumulator)."""
    from space_time_pde_amd import _lib, unet3d
    torch.manual_seed(5)
    nv, ci_bad = 300_000, 5
    x = torch.randn(1, 1, 1, nv, 16, device=DEV) * torch.logspace(-6, 6, nv, device=DEV)[None, None, None, :, None]
    gy = torch.randn(1, 1, 1, nv, 16, device=DEV)
    clean = x.clone()
    bad = torch.arange(nv) if nbad == nv else torch.tensor([7, 100_003, 200_001, 299_999][:nbad])
    x[0, 0, 0, bad.to(DEV), ci_bad] = NAN
    d = unet3d._desc(x, 16, 16, 1)
    d.det = 1
    acc = torch.zeros(16 * 16 * 2 * _lib.DET_K, device=DEV)
    _lib.check(hiplib.stpde_conv3d_wgrad(C.byref(d), _lib.ptr(x), _lib.ptr(gy), _lib.ptr(acc), _lib.stream_ptr()))
    out = torch.empty(16 * 16, device=DEV)
    _lib.check(hiplib.stpde_det_finalize(_lib.ptr(acc), 256, _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = out.double().reshape(16, 16)          # [1 tap][co][ci]
    marked = torch.zeros(16, 16, dtype=torch.bool, device=DEV)
    marked[:, ci_bad] = True
    assert torch.isnan(got[marked]).all(), got[marked]
    ref = torch.einsum("vo,vi->oi", gy.double().reshape(nv, 16), clean.double().reshape(nv, 16))
    scale = torch.einsum("vo,vi->oi", gy.double().abs().reshape(nv, 16), clean.double().abs().reshape(nv, 16))
    err = (got - ref).abs()[~marked]
    assert (err <= 3e-6 * scale[~marked]).all(), (err / scale[~marked]).max().item()


def test_batchnorm_statistics_nan_stays_in_its_channel(hiplib, monkeypatch):
    """BatchNorm in deterministic mode (training: the statistics are long accumulators read by det_value): one NaN voxel in one
    channel -> that channel's running mean / variance and output are NaN; every other channel equals the run without the NaN
    bit for bit."""
    from space_time_pde_amd import _lib, unet3d
    monkeypatch.setattr(_lib, "deterministic", True)
    c, c_bad = 32, 9
    g = torch.Generator().manual_seed(3)
    x0 = (1.5 * torch.randn(1, 8, 32, 32, c, generator=g) + 0.3).to(DEV)

    def run(x):
        bn = torch.nn.BatchNorm3d(c).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, c))
            bn.bias.copy_(torch.linspace(-0.2, 0.2, c))
        y = unet3d._bn_act(x, bn, False)
        torch.cuda.synchronize()
        return y.detach(), bn.running_mean.clone(), bn.running_var.clone()

    y0, m0, v0 = run(x0)
    assert torch.isfinite(y0).all() and torch.isfinite(m0).all() and torch.isfinite(v0).all()
    x1 = x0.clone()
    x1[0, 3, 17, 5, c_bad] = NAN
    y1, m1, v1 = run(x1)
    other = torch.arange(c, device=DEV) != c_bad
    assert math.isnan(m1[c_bad].item()) and math.isnan(v1[c_bad].item())
    assert torch.isnan(y1[..., c_bad]).all()
    assert torch.equal(m1[other], m0[other]) and torch.equal(v1[other], v0[other])
    assert torch.equal(y1[..., other], y0[..., other])


def test_imnet_weight_gradients_nan_cotangent_in_four_workgroups(hiplib, monkeypatch):
    """IM-NET weight gradients in deterministic mode: a 4,096-point lig_jets backward whose cotangent is NaN at 4 points ->
    every dW / db reads back NaN (each of them sums over all rows, and a NaN adjoint row makes its products NaN), none finite.

    The four points 0, 1026, 2052, 3078 are the row tiles 0, 513, 1026, 1539 of 2,048.  Every weight-gradient kernel runs a
    grid of 8 ... 768 workgroups over the row tiles, a multiple of 8 (csrc/jet_wgrad_impl.h: 768 / gy, 512 / (gy gz) rounded up to
    8, 256).  Shares made of contiguous tiles hold at most 2048 / 8 = 256 < 513 of them; shares made of every G-th tile put two
    of these tiles together only if G divides 513 k, k <= 3, which a multiple of 4 does not.  So the four NaN rows reach each
    accumulator from four different workgroups."""
    from space_time_pde_amd import _lib, implicit_net, lig_jet
    monkeypatch.setattr(_lib, "deterministic", True)
    P = 4096
    bad = [0, 1026, 2052, 3078]
    tiles = [p // 2 for p in bad]
    for G in range(8, 769, 8):
        share = -(-(P // 2) // G)
        assert len({t // share for t in tiles}) == 4 and len({t % G for t in tiles}) == 4
    g = torch.Generator().manual_seed(7)
    lat = (0.5 * torch.randn(1, 4, 8, 8, 32, generator=g)).to(DEV).requires_grad_(True)
    pts = torch.rand(1, P, 3, generator=g).to(DEV)
    torch.manual_seed(7)
    net = implicit_net.ImNet(nf=32, activation=torch.nn.Softplus).to(DEV)
    jets, _ = lig_jet.lig_jets(net, lat, pts, 0., 1., True, ((1, 1), (2, 2)))
    cot = torch.randn(jets.shape, generator=g).to(DEV)
    cot[:, :, bad] = NAN
    jets.backward(cot)
    torch.cuda.synchronize()
    for k in range(6):
        for name, t in (("dW", net.fc[k].weight.grad), ("db", net.fc[k].bias.grad)):
            nfin = int(torch.isfinite(t).sum())
            assert torch.isnan(t).all(), "%s%d: %d of %d elements finite" % (name, k, nfin, t.numel())
