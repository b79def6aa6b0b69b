"""The median pre-filter of the device batch sampler (csrc/sampler_median.hip: stpde_sampler_median,
DeviceBatchSampler(filter_on_device=True, median_on_device=True), lres_median_device): the parts that need no GPU -- the numpy
model (tests/sampler_median_model.py) against dataloader_spacetime.lres_filter, the switches and refusals of the constructor,
the library surface and the argument checks of the entry point."""
import ctypes

import numpy as np
import pytest
import torch

from space_time_pde_amd import _lib
from space_time_pde_amd import dataloader_spacetime as dl
from tests import sampler_median_model as M

FAKE = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch


# ---- the model against the loader's filter -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", [(1, 4), (2, 4), (4, 4), (4, 8)])
def test_model_equals_lres_filter(ds):
    """windows 49 (radius 0 along t), 147, 343 (r_t = 3 on nt = 8) and 1575 (r = 7 on n = 16, r_t = 3); one NaN"""
    x = torch.randn(2, 4, 8, 16, 16, generator=torch.Generator().manual_seed(11))
    x[1, 2, 3, 5, 7] = float("nan")
    want = dl.lres_filter(x, "median", ds[0], ds[1])
    got = torch.from_numpy(M.median_filter(x.numpy(), (ds[0] - 1, ds[1] - 1, ds[1] - 1)))
    assert got.shape == want.shape and got.dtype == want.dtype
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert bool(nan[1, 2].any()) and not bool(nan[0].any()) and not bool(nan[1, :2].any()) and not bool(nan[1, 3].any())
    assert 1 < int(nan.sum()) < nan[1, 2].numel()                      # spread over its window, not over the crop
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))


@pytest.mark.parametrize("n,r", [(2, 1), (2, 2), (2, 7), (5, 4), (5, 5), (6, 7), (8, 7), (16, 7)])
def test_model_reflection_is_the_loaders(n, r):
    assert M.reflect_index(n, r).tolist() == dl._reflect_index(n, r, "cpu").tolist()


# ---- switches and refusals ---------------------------------------------------------------------------------------------------
def _cpu_loader(kind, downsamp_xz=4, nx=16, nz=16, data=(12, 20, 24)):
    return dl.RB2DeviceLoader(torch.randn(4, *data), nx=nx, nz=nz, nt=8, n_samp_pts_per_crop=67, downsamp_xz=downsamp_xz,
                              downsamp_t=2, lres_filter=kind)


@pytest.mark.parametrize("kind", ["median", "gaussian", "uniform", "maximum", "none"])
def test_median_on_device_gets_past_the_filter_checks(kind):
    """what stops a host loader is the device check (the sampler is device-only), for median and for every other kind"""
    with pytest.raises(RuntimeError) as e:
        dl.DeviceBatchSampler(_cpu_loader(kind), 3, filter_on_device=True, median_on_device=True)
    assert not isinstance(e.value, NotImplementedError) and "HIP device" in str(e.value)


def test_filter_on_device_alone_still_refuses_median():
    for kw in ({"filter_on_device": True}, {"filter_on_device": True, "median_on_device": False}):
        with pytest.raises(NotImplementedError) as e:
            dl.DeviceBatchSampler(_cpu_loader("median"), 3, **kw)
        assert "median" in str(e.value) and "RB2DeviceLoader.get()" in str(e.value) and "median_on_device=True" in str(e.value)


def test_median_on_device_alone_is_the_default_refusal():
    with pytest.raises(NotImplementedError) as e:
        dl.DeviceBatchSampler(_cpu_loader("median"), 3, median_on_device=True)
    assert ("DeviceBatchSampler does not filter (lres_filter='median'): RB2DeviceLoader.get() is the path that applies the "
            "low-res filters") in str(e.value)


def test_a_radius_above_seven_is_refused_by_name():
    ld = _cpu_loader("median", downsamp_xz=16, nx=32, nz=32, data=(12, 36, 40))
    with pytest.raises(NotImplementedError) as e:
        dl.DeviceBatchSampler(ld, 3, filter_on_device=True, median_on_device=True)
    assert "radius" in str(e.value) and "15" in str(e.value) and "limit of 7" in str(e.value)
    with pytest.raises(RuntimeError) as e:                             # downsamp 8 (radius 7) is inside the limit
        dl.DeviceBatchSampler(_cpu_loader("median", downsamp_xz=8), 3, filter_on_device=True, median_on_device=True)
    assert "HIP device" in str(e.value)


def test_lres_median_device_is_device_only():
    with pytest.raises(RuntimeError) as e:
        dl.lres_median_device(torch.zeros(1, 2, 2, 2, 4), (1, 1, 1))
    assert "HIP device" in str(e.value)


# ---- the library surface -----------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_and_the_abi_version_stays(hiplib):
    assert hasattr(hiplib, "stpde_sampler_median") and "stpde_sampler_median" in _lib.exported_symbols()
    assert hiplib.stpde_version() == 316 and _lib.ABI_VERSION == 316                      # an additive symbol
    assert ctypes.sizeof(_lib.SamplerFilterDesc) == 68
    assert _lib.FILTER_KINDS == {"gaussian": 1, "uniform": 2, "maximum": 3} and _lib.FILTER_MEDIAN == 4


def _fdesc(**kw):
    d = _lib.SamplerFilterDesc()
    d.T, d.Z, d.X = 12, 20, 24
    d.nt, d.nz, d.nx = 8, 16, 16
    d.rt, d.rz, d.rx = 5, 5, 9
    d.B, d.kind = 3, 4
    for k, r in enumerate((1, 3, 3)):
        d.r[k], d.nw[k] = r, 0
    for k, v in kw.items():
        if k in ("r", "nw"):
            for j in range(3):
                getattr(d, k)[j] = v[j]
        else:
            setattr(d, k, v)
    return d


GOOD = [FAKE, FAKE, FAKE, ctypes.c_void_p(512)]                       # state, data_cl, crop_idx, crops_out


def _median(hiplib, d, ptrs=None):
    return hiplib.stpde_sampler_median(None if d is None else ctypes.byref(d), *(GOOD if ptrs is None else ptrs), None)


BAD = [
    (dict(kind=3), "kind must be 4 (median)"),
    (dict(kind=0), "kind must be 4 (median)"),
    (dict(nw=(0, 7, 0)), "takes no weight tables"),
    (dict(r=(1, 8, 3)), "radius 8 of axis 1 outside [0, 7]"),
    (dict(r=(-1, 3, 3)), "radius -1 of axis 0 outside [0, 7]"),
    (dict(B=0), "B must be positive"),
    (dict(nt=13), "larger than the dataset"),
    (dict(nx=1, rx=24), "crop needs >= 2 nodes"),
    (dict(rz=6), "inconsistent with the extents"),
    (dict(T=1310, Z=1300, X=1300, rt=1303, rz=1285, rx=1285), "below 2^31"),
    (dict(B=2 ** 20), "B * nt * nz * nx must be below 2^31"),
]


@pytest.mark.parametrize("change,why", BAD)
def test_bad_median_descriptors_are_refused_with_a_reason(hiplib, change, why):
    with pytest.raises(ValueError) as e:
        _lib.check(_median(hiplib, _fdesc(**change)))
    assert why in str(e.value) and "sampler_median" in str(e.value), str(e.value)


def test_median_pointers_are_checked(hiplib):
    with pytest.raises(ValueError) as e:
        _lib.check(_median(hiplib, None))
    assert "null descriptor" in str(e.value) and "sampler_median" in str(e.value)
    for k in range(4):
        ptrs = list(GOOD)
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(_median(hiplib, _fdesc(), ptrs))
        assert "null pointer" in str(e.value) and "sampler_median" in str(e.value), k
    for k in (1, 3):                                                 # data_cl, crops_out
        ptrs = list(GOOD)
        ptrs[k] = ctypes.c_void_p(260)
        with pytest.raises(ValueError) as e:
            _lib.check(_median(hiplib, _fdesc(), ptrs))
        assert "16-byte aligned" in str(e.value) and "sampler_median" in str(e.value), k


def test_the_separable_entry_still_refuses_kind_four(hiplib):
    d = _fdesc()
    ptrs = [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ctypes.c_void_p(512)]
    with pytest.raises(ValueError) as e:
        _lib.check(hiplib.stpde_sampler_filter(ctypes.byref(d), *ptrs, None))
    assert "kind must be 1 (gaussian), 2 (uniform) or 3 (maximum)" in str(e.value) and "sampler_filter" in str(e.value)
