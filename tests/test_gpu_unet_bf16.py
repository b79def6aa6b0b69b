"""The whole UNet3d with bf16 operands in its 3x3x3 convolutions (``unet3d.set_conv_precision("bf16")``) against an fp64 copy of
the same model whose 3x3x3 convolutions apply the numerics contract of the mode (include/stpde_hip.h, stpde_conv3d_desc.mfma_bf16):
forward on rounded x / W, dx from rounded gy / W, dW from rounded x / gy, dbias from the unrounded gy; everything else plain
fp64 torch.  Also: the distance of the bf16 mode from exact fp64, the mode captured at forward time, the default launching no
bf16 instantiation, and the configs[3] composite step in deterministic mode."""
import copy
import re

import pytest
import torch
import torch.nn.functional as F

from space_time_pde_amd import _lib, unet3d

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF_KERNELS = re.compile(r"k_conv3d_fwd<\d+, \d+, \w+, true>|k_conv3d_wgrad<\d+, \d+, \d+, false, true>|"
                        r"k_conv3d_wgrad_lds<\d+, \d+, \d+, \d+, true>|k_conv3_lds<\w+, \d+, true>|k_conv_fused<[^>]*EPI, true>")
# bf16 mode against exact fp64 at igres (32, 128, 128), eval mode, Frobenius relative error (measured figures: DESIGN 9)
EXACT_CEILING = {"out": 3e-3, "dx": 1e-1, "grads": 1e-1}
# Against the emulated reference the kernels differ only by fp32 accumulation order -- and by the few operands whose fp32 and
# fp64 values round to different bf16 neighbours (one bf16 ulp each).  Measured (eval mode): output 6.5e-6 / 9.8e-6, input
# gradient 2.8e-4 / 6.6e-4, parameter gradients 8.5e-4 / 1.9e-3 at (16,32,32) / (32,128,128); the fp32 mode 14x - 85x farther.
TOL = 6e-3


def _bf(t):
    return t.to(torch.bfloat16).double()


def _cl(t):
    return t.permute(0, 4, 1, 2, 3)


class _EmuConv3(torch.autograd.Function):
    """3x3x3 / pad 1 convolution of a channels-last fp64 tensor under the bf16-operand contract"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return F.conv3d(_cl(_bf(x)), _bf(w), b, padding=1).permute(0, 2, 3, 4, 1).contiguous()

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        g = _cl(_bf(gy))
        dx = torch.nn.grad.conv3d_input(tuple(_cl(x).shape), _bf(w), g, padding=1).permute(0, 2, 3, 4, 1)
        dw = torch.nn.grad.conv3d_weight(_cl(_bf(x)), tuple(w.shape), g, padding=1)
        db = gy.reshape(-1, gy.shape[-1]).sum(0) if ctx.has_b else None
        return dx, dw, db


def _frob(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / max(b.norm().item(), 1e-300)).item()


def _run(model, x, cot, fp64=False):
    """forward + backward of (out * cot).sum(): output, input gradient, parameter gradients by name"""
    for p in model.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    out = model._forward_impl(xin) if fp64 else model(xin)      # (fp64: no fp32 weight packs to prepare)
    (out * cot).sum().backward()
    return out.detach(), xin.grad.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()
                                             if p.grad is not None}


def _reference(unet, x, cot, monkeypatch, emulate):
    ref = copy.deepcopy(unet).double()
    orig = unet3d._conv_cl

    def conv_cl(h, conv):
        if emulate and h.dtype == torch.float64 and conv.weight.shape[2] == 3:
            return _EmuConv3.apply(h, conv.weight, conv.bias)
        return orig(h, conv)

    with monkeypatch.context() as m:
        m.setattr(unet3d, "_conv_cl", conv_cl)
        return _run(ref, x.double(), cot.double(), fp64=True)


def _errors(got, ref):
    """output, input gradient, all parameter gradients as one vector"""
    out, dx, g = got
    rout, rdx, rg = ref
    assert set(g) == set(rg)
    names = sorted(g)
    gcat = torch.cat([g[n].double().reshape(-1) for n in names])
    rcat = torch.cat([rg[n].double().reshape(-1) for n in names])
    return _frob(out, rout), _frob(dx, rdx), _frob(gcat, rcat)


def _model(igres, train=True, seed=0, mf=256):
    torch.manual_seed(seed)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=igres, nf=16, mf=mf).to(DEV)
    unet.train(train)
    x = torch.randn(1, 4, *igres, device=DEV)
    cot = torch.randn(1, 32, *igres, device=DEV)
    return unet, x, cot


def _state(unet):
    return {k: v.clone() for k, v in unet.state_dict().items()}


# Eval mode only.  In training mode this U-Net is not a usable yardstick: it pools down to ONE voxel, its deepest BatchNorms
# normalise over a handful of values and turn one-ulp differences into O(1) ones (measured against the emulated reference at
# (16,32,32): output 1.3e-2, input gradient 0.3, parameter gradients 0.97 -- the fp32 mode 0.11 / 1.3 / 1.0 -- whatever mf).
# The training-mode paths (fused residual blocks, layer-wise kernels) are pinned kernel by kernel in test_gpu_conv_bf16.py and
# as whole steps by the bit-for-bit tests below.
@pytest.mark.parametrize("igres", [(16, 32, 32), (32, 128, 128)])
def test_unet_against_the_emulated_reference(hiplib, monkeypatch, igres):
    train, fused, mf = False, "1", 256
    unet, x, cot = _model(igres, train, mf=mf)
    s0 = _state(unet)
    ref = _reference(unet, x, cot, monkeypatch, True)
    res = {}
    for mode in ("bf16", "fp32"):
        unet.load_state_dict(s0)                       # (BatchNorm running statistics as the reference saw them)
        monkeypatch.setattr(unet3d, "conv_precision", mode)
        with _lib.dispatch_trace() as tr:
            got = _run(unet, x, cot)
            torch.cuda.synchronize()
        assert bool([k for k in tr.kernels if BF_KERNELS.search(k)]) == (mode == "bf16"), "\n".join(tr.kernels)
        res[mode] = _errors(got, ref)
    (o16, d16, g16), (o32, d32, g32) = res["bf16"], res["fp32"]
    print("igres %s train %s fused %s mf %d: bf16 mode out %.2e dx %.2e grads %.2e; fp32 mode out %.2e dx %.2e grads %.2e"
          % (igres, train, fused, mf, o16, d16, g16, o32, d32, g32))
    assert o16 <= TOL and d16 <= TOL and g16 <= TOL, (o16, d16, g16)
    assert o32 >= 10 * o16 and d32 >= 10 * d16 and g32 >= 10 * g16, (o16, o32, d16, d32, g16, g32)


def test_bf16_mode_against_exact_fp64(hiplib, monkeypatch):
    igres = (32, 128, 128)
    unet, x, cot = _model(igres, False, seed=3)
    s0 = _state(unet)
    ref = _reference(unet, x, cot, monkeypatch, False)
    err = {}
    for mode in ("bf16", "fp32"):
        monkeypatch.setattr(unet3d, "conv_precision", mode)
        unet.load_state_dict(s0)
        err[mode] = _errors(_run(unet, x, cot), ref)
    print("vs exact fp64 at %s, eval mode: bf16 mode out %.3e dx %.3e grads %.3e; fp32 mode out %.3e dx %.3e grads %.3e"
          % ((igres,) + err["bf16"] + err["fp32"]))
    o, d, g = err["bf16"]
    assert o <= EXACT_CEILING["out"] and d <= EXACT_CEILING["dx"] and g <= EXACT_CEILING["grads"], (o, d, g)


def test_mode_is_captured_at_forward(hiplib, monkeypatch):
    """forward in bf16, switch to fp32, backward: bit-identical to a run that stays in bf16 (deterministic mode: every
    accumulated sum order-independent)"""
    monkeypatch.setattr(_lib, "deterministic", True)
    for fused in ("1", "0"):
        monkeypatch.setenv("STPDE_FUSED_RESBLOCK", fused)
        unet, x, cot = _model((16, 32, 32), True, seed=5)
        s0 = _state(unet)
        runs = []
        for switch in (False, True):
            unet.load_state_dict(s0)
            for p in unet.parameters():
                p.grad = None
            monkeypatch.setattr(unet3d, "conv_precision", "bf16")
            xin = x.clone().requires_grad_(True)
            out = unet(xin)
            if switch:
                assert unet3d.set_conv_precision("fp32") == "bf16"
            (out * cot).sum().backward()
            runs.append((out.detach(), xin.grad, [p.grad.clone() for p in unet.parameters()]))
        (oa, da, ga), (ob, db, gb) = runs
        assert torch.equal(oa, ob) and torch.equal(da, db)
        for k, (a, b) in enumerate(zip(ga, gb)):
            assert torch.equal(a, b), (fused, k, (a - b).abs().max().item())


def test_default_mode_launches_no_bf16_instantiation(hiplib, monkeypatch):
    assert unet3d.conv_precision == "fp32"
    for fused in ("1", "0"):
        monkeypatch.setenv("STPDE_FUSED_RESBLOCK", fused)
        unet, x, cot = _model((16, 64, 64), True, seed=6)
        with _lib.dispatch_trace() as tr:
            _run(unet, x, cot)
            torch.cuda.synchronize()
        assert any("k_conv" in k for k in tr.kernels), tr.kernels
        assert not [k for k in tr.kernels if BF_KERNELS.search(k)], "\n".join(tr.kernels)


def test_config3_composite_bf16_encoder_deterministic(hiplib, monkeypatch):
    """configs[3] (latent [1, 64, 256, 256, 32], 2^20 points, bf16 MLP) with the bf16 encoder, through sharded_step, twice in
    deterministic mode: losses and every gradient bit-identical and finite; the bf16 LDS kernels carried the wide levels."""
    from space_time_pde_amd import implicit_net, lig_jet, local_implicit_grid as lig, nonlinearities, physics
    from space_time_pde_amd.train_step import sharded_step
    igres, n_pts = (64, 256, 256), 1 << 20
    torch.manual_seed(1)
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32,
                             activation=nonlinearities.NONLINEARITIES["softplus"]).to(DEV)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=igres, nf=16, mf=256).to(DEV).train()
    layer = physics.get_rb2_pde_layer(mean=(0.01, 0.0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1.,
                                      x_crop=1., use_continuity=True)
    g = torch.Generator().manual_seed(0)
    crop = torch.randn(1, 4, *igres, generator=g).to(DEV)
    pts = torch.rand(1, n_pts, 3, generator=g).to(DEV)
    tgt = torch.randn(1, n_pts, 4, generator=g).to(DEV)
    monkeypatch.setattr(lig_jet, "mlp_precision", "bf16")
    monkeypatch.setattr(unet3d, "conv_precision", "bf16")
    monkeypatch.setattr(_lib, "deterministic", True)
    monkeypatch.setenv("STPDE_FUSED_RESBLOCK", "1")
    params = list(unet.parameters()) + list(net.parameters())
    s0 = _state(unet)
    runs = []
    for it in range(2):
        unet.load_state_dict(s0)
        for p in params:
            p.grad = None
        calls = lig.stats["hip_jet_calls"]
        with _lib.dispatch_trace() as tr:
            loss, reg, pde = sharded_step(unet, net, layer, crop, pts, tgt, n_pts, 1.0, 0.0125, "l1")
            torch.cuda.synchronize()
        assert lig.stats["hip_jet_calls"] == calls + 1
        assert tr.has("k_conv3_lds<", ", true>)") and tr.has("k_conv3d_wgrad_lds<", ", true>)"), "\n".join(tr.kernels)
        losses = [float(loss), float(reg), float(pde)]
        assert all(map(lambda v: v == v and abs(v) < float("inf"), losses)), losses
        for k, p in enumerate(params):
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
        runs.append((losses, [p.grad.clone() for p in params]))
    (la, ga), (lb, gb) = runs
    assert la == lb, (la, lb)
    for k, (a, b) in enumerate(zip(ga, gb)):
        assert torch.equal(a, b), (k, (a - b).abs().max().item())
    print("configs[3] composite, bf16 encoder + bf16 MLP, deterministic: loss %.6f reg %.6f pde %.6f" % tuple(la))
