"""bf16-operand mode of the 3x3x3 convolutions (stpde_conv3d_desc.mfma_bf16 = 1) through the C ABI, path by path, against an fp64
reference on operands rounded to bf16 (the numerics contract of include/stpde_hip.h):
  forward         y  = bias + sum_tap bf16(W_tap) . bf16(x_tap)
  input gradient  dx = sum bf16(W^T) . bf16(gy)            (the same kernels on the transposed, tap-flipped pack)
  weight grad.    dW = sum_vox bf16(gy) x bf16(x_shifted),  dbias = fp64 sum of the UNROUNDED gy
Exact data first (small integers / multiples of 1/8: every bf16 instantiation must equal the reference bit for bit -- an A / B
k-map mismatch cannot hide there), then random data (<= 1e-5 / 1e-4 of the largest magnitude, and the fp32 mode at least 10x
farther from the emulated reference than the bf16 mode), kernel equivalence, deterministic mode, dispatch trace.
"""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as F

from space_time_pde_amd import _lib, unet3d

pytestmark = pytest.mark.gpu
R = _lib.BN_REP
DEV = torch.device("cuda:0")


def _bf(t):
    return t.to(torch.bfloat16).double()


def _packs(w):
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    fidx, bidx, _, _ = unet3d._pack_indices(co, ci, k, DEV)
    wflat = torch.cat([w.reshape(-1), w.new_zeros(1)])
    return wflat[fidx].contiguous(), wflat[bidx].contiguous()


def _cl(t):        # channels-last [B, T, Z, X, C] -> [B, C, T, Z, X]
    return t.permute(0, 4, 1, 2, 3)


def _ref_fwd(x, w, b, rnd=True):
    f = _bf if rnd else (lambda t: t.double())
    y = F.conv3d(_cl(f(x)), f(w), None if b is None else b.double(), padding=1)
    return y.permute(0, 2, 3, 4, 1)


def _ref_dgrad(gy, w, ci, rnd=True):
    f = _bf if rnd else (lambda t: t.double())
    shp = (gy.shape[0], ci) + tuple(gy.shape[1:4])
    return torch.nn.grad.conv3d_input(shp, f(w), _cl(f(gy)), padding=1).permute(0, 2, 3, 4, 1)


def _ref_wgrad(x, gy, co, rnd=True):
    f = _bf if rnd else (lambda t: t.double())
    ci = x.shape[-1]
    return torch.nn.grad.conv3d_weight(_cl(f(x)), (co, ci, 3, 3, 3), _cl(f(gy)), padding=1)


def _rel(a, b):
    b = b.double()
    return (a.double() - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _desc(shape, ci, co, bf, det=0):
    d = _lib.Conv3dDesc()
    d.B, d.T, d.Z, d.X = shape
    d.Ci, d.Co, d.ksize, d.det, d.mfma_bf16 = ci, co, 3, det, bf
    return d


def _fwd(shape, x, pack, bias, co, bf):
    """stpde_conv3d_fwd -> (y, trace)"""
    y = torch.full((*shape, co), float("nan"), device=DEV)
    d = _desc(shape, x.shape[-1], co, bf)
    with _lib.dispatch_trace() as tr:
        _lib.check(_lib.lib().stpde_conv3d_fwd(C.byref(d), _lib.ptr(x), _lib.ptr(pack), _lib.ptr(bias), _lib.ptr(y),
                                               _lib.stream_ptr()))
        torch.cuda.synchronize()
    return y, tr


def _wgrad(shape, x, gy, bf, det=0):
    """stpde_conv3d_wgrad_bias -> (dW [co][ci][3][3][3], dbias, trace, raw accumulators)"""
    ci, co = x.shape[-1], gy.shape[-1]
    aw = 2 * _lib.DET_K if det else 1
    dw = torch.zeros(27 * co * ci * aw, device=DEV)
    db = torch.zeros(co * aw, device=DEV)
    d = _desc(shape, ci, co, bf, det)
    with _lib.dispatch_trace() as tr:
        _lib.check(_lib.lib().stpde_conv3d_wgrad_bias(C.byref(d), _lib.ptr(x), _lib.ptr(gy), _lib.ptr(dw), _lib.ptr(db),
                                                      _lib.stream_ptr()))
        torch.cuda.synchronize()
    raw = (dw.clone(), db.clone())
    if det:
        dwf, dbf = torch.empty(27 * co * ci, device=DEV), torch.empty(co, device=DEV)
        _lib.check(_lib.lib().stpde_det_finalize(_lib.ptr(dw), dwf.numel(), _lib.ptr(dwf), _lib.stream_ptr()))
        _lib.check(_lib.lib().stpde_det_finalize(_lib.ptr(db), co, _lib.ptr(dbf), _lib.stream_ptr()))
        torch.cuda.synchronize()
        dw, db = dwf, dbf
    return dw.view(27, co, ci).permute(1, 2, 0).reshape(co, ci, 3, 3, 3), db, tr, raw


def _fused(shape, x, pack, co, bf, bias=None, stats=False, mask=None, det=0):
    """stpde_conv3d_fused, 3x3x3 -> (y, out_sums, m_bsum, done, trace)"""
    a = _lib.Conv3dFusedArgs()
    a.d = _desc(shape, x.shape[-1], co, bf, det)
    y = torch.full((*shape, co), float("nan"), device=DEV)
    sums = torch.zeros(R * 2 * co * (2 * _lib.DET_K if det else 1), device=DEV, dtype=torch.float64)
    bsum = torch.zeros(R * 2 * co * (2 * _lib.DET_K if det else 1), device=DEV)
    a.x, a.w_pack, a.y, a.bias = _lib.ptr(x), _lib.ptr(pack), _lib.ptr(y), _lib.ptr(bias)
    if stats:
        a.out_sums = _lib.ptr(sums)
    if mask is not None:
        m, stat, gam, bet = mask
        a.m, a.m_stat, a.m_gamma, a.m_beta, a.m_bsum = _lib.ptr(m), _lib.ptr(stat), _lib.ptr(gam), _lib.ptr(bet), _lib.ptr(bsum)
    done = C.c_int(1)
    with _lib.dispatch_trace() as tr:
        _lib.check(_lib.lib().stpde_conv3d_fused(C.byref(a), C.byref(done), _lib.stream_ptr()))
        torch.cuda.synchronize()
    return y, sums, bsum, done.value, tr


def _dump(tr):
    return "\n".join(tr.kernels)


# the bf16 instantiations as the library's launch sites name them (literal BF = true as the last template argument)
BF_KERNELS = re.compile(r"k_conv3d_fwd<\d+, \d+, \w+, true>|k_conv3d_wgrad<\d+, \d+, \d+, false, true>|"
                        r"k_conv3d_wgrad_lds<\d+, \d+, \d+, \d+, true>|k_conv3_lds<\w+, \d+, true>|k_conv_fused<[^>]*EPI, true>")


def bf16_kernels(tr):
    return [k for k in tr.kernels if BF_KERNELS.search(k)]


# ---- exact data: every bf16 instantiation equals the reference bit for bit ------------------------------------------------
def _exact(shape, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (*shape, c), generator=g).float().to(DEV)
    w = (torch.randint(-8, 9, (c, c, 3, 3, 3), generator=g).float() / 8).to(DEV)
    return x, w


# (shape, channels, tune overrides, kernel the call must reach)
FWD_EXACT = [((1, 16, 128, 128), 16, {}, "k_conv3d_fwd<1, 4, false, true>"),
             ((2, 8, 32, 64), 32, {}, "k_conv3d_fwd<2, 1, false, true>"),
             ((1, 4, 8, 24), 64, {}, "k_conv3d_fwd<4, 1, true, true>"),
             ((1, 8, 32, 64), 128, {}, "k_conv3d_fwd<4, 1, false, true>")]
FUSED_EXACT = [((1, 8, 32, 64), 16, dict(conv3_lds_minblk=1, conv3_lds_gx=5), "k_conv3_lds<1, 0, true>"),
               ((1, 8, 32, 64), 32, dict(conv3_lds_minblk=1, conv3_lds_gx=5), "k_conv3_lds<2, 0, true>"),
               ((1, 8, 32, 64), 64, dict(conv3_lds_minblk=1, conv3_lds_gx=5), "k_conv3_lds<4, 0, true>"),
               ((1, 8, 32, 64), 32, dict(conv3_lds_off=1), "k_conv_fused<2, 1, K3, DUAL, ONLOAD, EPI, true>"),
               ((1, 16, 128, 128), 16, dict(conv3_lds_off=1), "k_conv_fused<1, 4, K3, DUAL, ONLOAD, EPI, true>")]
WGRAD_EXACT = [((1, 16, 32, 128), 16, {}, "k_conv3d_wgrad_lds<1, 1, 32, 1, true>"),
               ((1, 16, 32, 128), 32, dict(conv_wgrad_lds_gx=7), "k_conv3d_wgrad_lds<2, 2, 32, 2, true>"),
               ((1, 16, 32, 64), 64, {}, "k_conv3d_wgrad_lds<4, 1, 16, 4, true>"),
               ((1, 3, 5, 7), 16, {}, "k_conv3d_wgrad<1, 1, 9, false, true>"),
               ((1, 3, 5, 7), 128, {}, "k_conv3d_wgrad<2, 2, 3, false, true>")]


@pytest.mark.parametrize("case", range(len(FWD_EXACT) + len(FUSED_EXACT)))
def test_exact_data_forward_and_input_gradient_bit_for_bit(hiplib, case):
    shape, c, tune, kern = (FWD_EXACT + FUSED_EXACT)[case]
    x, w = _exact(shape, c, case)
    fp, bp = _packs(w)
    with _lib.tuned(**tune):
        for pack, wref, what in ((fp, w, "forward"), (bp, None, "input gradient")):
            if case < len(FWD_EXACT):
                y, tr = _fwd(shape, x, pack, None, c, 1)
            else:
                y, _, _, _, tr = _fused(shape, x, pack, c, 1)
            assert tr.has(kern), _dump(tr)
            ref = _ref_fwd(x, w, None) if wref is not None else _ref_dgrad(x, w, c)
            assert torch.equal(y.double(), ref), (what, (y.double() - ref).abs().max().item())


@pytest.mark.parametrize("case", range(len(WGRAD_EXACT)))
def test_exact_data_weight_gradient_bit_for_bit(hiplib, case):
    shape, c, tune, kern = WGRAD_EXACT[case]
    g = torch.Generator().manual_seed(100 + case)
    x = torch.randint(-3, 4, (*shape, c), generator=g).float().to(DEV)
    gy = torch.randint(-3, 4, (*shape, c), generator=g).float().to(DEV)
    with _lib.tuned(**tune):
        dw, db, tr, _ = _wgrad(shape, x, gy, 1)
    assert tr.has(kern), _dump(tr)
    assert torch.equal(dw.double(), _ref_wgrad(x, gy, c))
    assert torch.equal(db.double(), gy.double().reshape(-1, c).sum(0))


# ---- random data -----------------------------------------------------------------------------------------------------------
def _rand(shape, ci, co, seed):
    torch.manual_seed(seed)
    x = torch.randn(*shape, ci, device=DEV) + 0.3
    w = torch.randn(co, ci, 3, 3, 3, device=DEV) / (27 * ci) ** 0.5
    b = torch.randn(co, device=DEV)
    return x, w, b


FWD_RANDOM = [((1, 16, 128, 128), 16, 16, "k_conv3d_fwd<1, 4, false, true>"),
              ((1, 16, 128, 128), 32, 32, "k_conv3d_fwd<2, 4, false, true>"),
              ((2, 8, 32, 64), 64, 64, "k_conv3d_fwd<4, 1, false, true>"),
              ((2, 8, 32, 64), 32, 16, "k_conv3d_fwd<1, 1, false, true>"),
              ((1, 4, 8, 24), 32, 32, "k_conv3d_fwd<4, 1, true, true>"),
              ((1, 8, 32, 64), 128, 128, "k_conv3d_fwd<4, 1, false, true>"),
              ((1, 4, 16, 32), 128, 128, "k_conv3d_fwd<4, 1, true, true>")]


@pytest.mark.parametrize("case", range(len(FWD_RANDOM)))
def test_layerwise_forward_and_input_gradient_random(hiplib, case):
    shape, ci, co, kern = FWD_RANDOM[case]
    x, w, b = _rand(shape, ci, co, case)
    fp, bp = _packs(w)
    y16, tr = _fwd(shape, x, fp, b, co, 1)
    assert tr.has(kern), _dump(tr)
    y32, tr32 = _fwd(shape, x, fp, b, co, 0)
    assert tr32.kernels and not bf16_kernels(tr32), _dump(tr32)
    ref = _ref_fwd(x, w, b)
    e16, e32 = _rel(y16, ref), _rel(y32, ref)
    assert e16 <= 1e-5 and e32 >= 10 * e16, (e16, e32)
    # input gradient: the same kernels on the transposed, tap-flipped pack (Co -> Ci)
    gy = torch.randn(*shape, co, device=DEV)
    dx16, tr = _fwd(shape, gy, bp, None, ci, 1)
    dx32, _ = _fwd(shape, gy, bp, None, ci, 0)
    ref = _ref_dgrad(gy, w, ci)
    e16, e32 = _rel(dx16, ref), _rel(dx32, ref)
    assert e16 <= 1e-5 and e32 >= 10 * e16, (e16, e32)


def _mask_inputs(shape, c, seed):
    torch.manual_seed(seed)
    m = torch.randn(*shape, c, device=DEV) + 0.3
    gam, bet = torch.rand(c, device=DEV) + 0.5, 0.3 * torch.randn(c, device=DEV)
    ms = m.double().reshape(-1, c)
    stat = torch.cat([ms.mean(0), 1 / torch.sqrt(ms.var(0, unbiased=False) + 1e-5)]).float().contiguous()
    return m, stat, gam, bet


FUSED_TUNES = {"lds": dict(conv3_lds_minblk=1), "lds_ragged": dict(conv3_lds_minblk=1, conv3_lds_gx=5),
               "per_wave": dict(conv3_lds_off=1)}


@pytest.mark.parametrize("c", [16, 32, 64])
@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("path", sorted(FUSED_TUNES))
def test_fused_epilogues_random(hiplib, c, epi, path):
    shape = (1, 8, 32, 64)
    x, w, b = _rand(shape, c, c, 10 * c + epi)
    fp, _ = _packs(w)
    mask = _mask_inputs(shape, c, c + epi) if epi == 2 else None
    bias = None if epi == 2 else b
    out = {}
    for bf in (1, 0):
        with _lib.tuned(**FUSED_TUNES[path]):
            out[bf] = _fused(shape, x, fp, c, bf, bias=bias, stats=epi == 1, mask=mask)
    y16, sums, bsum, done, tr = out[1]
    assert done == 1
    want = ("k_conv_fused<1, 1, K3, DUAL, ONLOAD, EPI, true>" if path == "per_wave" else
            "k_conv3_lds<%d, %d, true>" % (c // 16, epi))
    assert tr.has(want) or (path == "per_wave" and tr.has("k_conv_fused<", "true>", "EPI = %d" % epi)), _dump(tr)
    assert out[0][4].kernels and not bf16_kernels(out[0][4]), _dump(out[0][4])
    conv = _ref_fwd(x, w, bias)
    if epi == 2:
        m, stat, gam, bet = mask
        xhat = (m.double() - stat[:c].double()) * stat[c:].double()
        pre = xhat * gam.double() + bet.double()
        safe = pre.abs() > 1e-5
        dz = conv * (pre > 0)
        for bf in (1, 0):
            err = ((out[bf][0].double() - dz).abs() * safe).max().item() / conv.abs().max().item()
            out[bf] = out[bf] + (err,)
        e16, e32 = out[1][-1], out[0][-1]
        # BatchNorm-backward sums: the fp64 formula on the gradient the kernel stored (mask / sums from the fp32 result)
        dzs = y16.double().reshape(-1, c)
        xh = xhat.reshape(-1, c)
        tot = bsum.view(R, 2, c).sum(0).double()
        scale = dzs.abs().sum(0)
        assert ((tot[0] - dzs.sum(0)).abs() <= 2e-6 * scale + 1e-4).all()
        assert ((tot[1] - (dzs * xh).sum(0)).abs() <= 1e-5 * scale * (1 + xh.abs().max()) + 1e-4).all()
    else:
        e16, e32 = _rel(y16, conv), _rel(out[0][0], conv)
    assert e16 <= 1e-5 and e32 >= 10 * e16, (e16, e32)
    if epi == 1:
        s = sums.view(R, 2, c).sum(0)
        r = y16.double().reshape(-1, c)
        assert _rel(s[0], r.sum(0)) < 2e-6 and _rel(s[1], (r * r).sum(0)) < 2e-6
        re = conv.reshape(-1, c)
        assert _rel(s[0], re.sum(0)) < 1e-5 and _rel(s[1], (re * re).sum(0)) < 1e-5


@pytest.mark.parametrize("c", [16, 32, 64])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_bf16_lds_kernel_and_per_wave_kernel_are_bit_identical(hiplib, c, epi):
    shape = (2, 8, 32, 64)
    x, w, b = _rand(shape, c, c, 7 * c + epi)
    fp, _ = _packs(w)
    mask = _mask_inputs(shape, c, 3 + epi) if epi == 2 else None
    ys = {}
    for off in (0, 1):
        with _lib.tuned(conv3_lds_off=off, conv3_lds_minblk=1, conv3_lds_gx=24):
            y, _, _, done, tr = _fused(shape, x, fp, c, 1, bias=None if epi == 2 else b, stats=epi == 1, mask=mask)
        assert done == 1
        assert tr.has("k_conv3_lds<%d, %d, true>" % (c // 16, epi)) == (off == 0), _dump(tr)
        assert tr.has("k_conv_fused<", "true>") == (off == 1), _dump(tr)
        ys[off] = y
    assert torch.equal(ys[0], ys[1])


WGRAD_RANDOM = [((1, 16, 32, 128), 16, 16, {}, "k_conv3d_wgrad_lds<1, 1, 32, 1, true>"),
                ((1, 16, 32, 128), 32, 32, dict(conv_wgrad_lds_gx=7), "k_conv3d_wgrad_lds<2, 2, 32, 2, true>"),
                ((2, 8, 32, 128), 16, 32, {}, "k_conv3d_wgrad_lds<1, 2, 32, 2, true>"),
                ((2, 8, 32, 128), 32, 16, dict(conv_wgrad_lds_gx=5), "k_conv3d_wgrad_lds<2, 1, 32, 1, true>"),
                ((1, 16, 32, 64), 64, 64, {}, "k_conv3d_wgrad_lds<4, 1, 16, 4, true>"),
                ((1, 5, 6, 13), 128, 128, {}, "k_conv3d_wgrad<2, 2, 3, false, true>"),
                ((1, 3, 5, 7), 16, 16, {}, "k_conv3d_wgrad<1, 1, 9, false, true>")]


@pytest.mark.parametrize("case", range(len(WGRAD_RANDOM)))
def test_weight_gradient_random(hiplib, case):
    shape, ci, co, tune, kern = WGRAD_RANDOM[case]
    torch.manual_seed(50 + case)
    x = torch.randn(*shape, ci, device=DEV) + 0.3
    gy = torch.randn(*shape, co, device=DEV)
    with _lib.tuned(**tune):
        dw16, db16, tr, _ = _wgrad(shape, x, gy, 1)
        dw32, db32, tr32, _ = _wgrad(shape, x, gy, 0)
    assert tr.has(kern), _dump(tr)
    assert tr32.kernels and not bf16_kernels(tr32), _dump(tr32)
    ref = _ref_wgrad(x, gy, co)
    e16, e32 = _rel(dw16, ref), _rel(dw32, ref)
    assert e16 <= 1e-4 and e32 >= 10 * e16, (e16, e32)
    assert _rel(db16, gy.double().reshape(-1, co).sum(0)) <= 2e-6


def test_deterministic_mode_with_bf16_operands(hiplib):
    """det = 1: weight / bias gradients (long accumulators) and the statistics epilogue bit-identical from run to run"""
    shape, c = (1, 16, 32, 128), 32
    x, w, b = _rand(shape, c, c, 77)
    gy = torch.randn(*shape, c, device=DEV)
    runs = [_wgrad(shape, x, gy, 1, det=1) for _ in range(2)]
    for t in runs:
        assert t[2].has("k_conv3d_wgrad_lds<2, 2, 32, 2, true>"), _dump(t[2])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert _rel(runs[0][0], _ref_wgrad(x, gy, c)) <= 1e-4
    fp, _ = _packs(w)
    with _lib.tuned(conv3_lds_minblk=1, conv3_lds_gx=24):
        st = [_fused(shape, x, fp, c, 1, bias=b, stats=True, det=1) for _ in range(2)]
    assert st[0][4].has("k_conv3_lds<2, 1, true>"), _dump(st[0][4])
    assert torch.equal(st[0][0], st[1][0])
    s1 = [torch.empty(2 * c, device=DEV) for _ in range(2)]
    for t, out in zip(st, s1):
        _lib.check(hiplib.stpde_det_finalize(_lib.ptr(t[1]), 2 * c, _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(s1[0], s1[1])
    r = st[0][0].double().reshape(-1, c)
    assert _rel(s1[0][:c], r.sum(0)) < 1e-5 and _rel(s1[0][c:], (r * r).sum(0)) < 1e-5
    assert _rel(st[0][0], _ref_fwd(x, w, b)) <= 1e-5
