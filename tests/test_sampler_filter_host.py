"""Low-res filters in the device batch sampler (csrc/sampler.hip: stpde_sampler_filter / stpde_sampler_produce_filtered,
DeviceBatchSampler(filter_on_device=True)): the parts that need no GPU -- a numpy model of every index the pass kernels form
(tests/sampler_filter_model.py) held inside its buffers and against dataloader_spacetime.lres_filter, the refusals of the
constructor, and the argument checks of the two entry points."""
import ctypes

import numpy as np
import pytest
import torch

from space_time_pde_amd import _lib
from space_time_pde_amd import dataloader_spacetime as dl
from tests import sampler_filter_model as M

FAKE = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch


# ---- the address model ------------------------------------------------------------------------------------------------------
def _inside(launches):
    for mx, first, axis, r, writes, touched, sizes in launches:
        for name, at in touched.items():
            if at.size:
                assert 0 <= int(at.min()) and int(at.max()) < sizes[name], (name, mx, first, axis, r, int(at.min()), int(at.max()))
        dst = np.sort(touched["dst"])
        assert np.array_equal(dst, np.arange(sizes["dst"])), "every scratch element is written exactly once"


@pytest.mark.parametrize("kind", ["uniform", "maximum"])
@pytest.mark.parametrize("ids", [[-5, 16, 2 ** 31 - 1], [2 ** 31 - 1], [-5], [16], [15]])
def test_no_radius_extent_or_crop_id_leaves_a_buffer(kind, ids):
    """crop (2, 5, 4) of a (3, 6, 7) dataset, len = 2 * 2 * 4 = 16: ids -5, len and 2^31 - 1 (and the last valid one); B = 3 and
    B = 1; radii (5, 5, 2): r > 2n on the axis with n = 2, r = n, r < n; (1, 9, 4): r < n, n < r < 2n, r = n; one axis; none"""
    rng = np.random.default_rng(0)
    g = M.Geometry((3, 6, 7), (2, 5, 4), len(ids))
    assert len(g) == 16
    data = rng.standard_normal((3, 6, 7, 4)).astype(np.float32)
    for radii in [(5, 5, 2), (1, 9, 4), (0, 11, 0), (0, 0, 0)]:
        w = [rng.random(2 * r + 1).astype(np.float32) if r else None for r in radii]
        out, launches, oob = M.run_filter(g, data, ids, kind, radii, w)
        assert len(launches) == max(1, sum(1 for r in radii if r))
        assert launches[-1][4] == "a" and launches[0][1] and not any(l[1] for l in launches[1:])
        _inside(launches)
        assert oob == sum(1 for i in ids if not 0 <= i < len(g))
        assert not np.isnan(out).any()


@pytest.mark.parametrize("n,r", [(2, 1), (2, 2), (2, 5), (5, 4), (5, 5), (5, 11), (8, 8), (16, 8)])
def test_model_taps_are_the_loaders_reflect_index(n, r):
    """the tap walk (m = (i - r) mod 2n, stepped with wrap-around, mirrored into [0, n)) against _reflect_index for every i, k"""
    want = dl._reflect_index(n, r, "cpu").numpy()                      # padded axis: entry i + k is tap k of output i
    g = M.Geometry((n, 2, 2), (n, 2, 2), 1)
    data = np.arange(n * 2 * 2 * 4, dtype=np.float32).reshape(n, 2, 2, 4)      # value // 16 = the t index
    _, touched, _ = M.filter_pass(g, data.reshape(-1), np.zeros(1, np.int32), 0, r, None, True, True)
    taps = touched["src"].reshape(2 * r + 1, n * 4, 4)[:, ::4, 0] // 16        # [k, i] for the voxels (i, 0, 0)
    for i in range(n):
        assert taps[:, i].tolist() == want[i:i + 2 * r + 1].tolist(), (i, taps[:, i], want)
        assert 0 <= taps[:, i].min() and taps[:, i].max() < n


# ---- the model against the loader's filter -----------------------------------------------------------------------------------
DATASET = (12, 20, 24)


def _against_lres_filter(kind, downsamp_t, downsamp_xz, data, ids, crop=(8, 16, 16), bits=False):
    ld = dl.RB2DeviceLoader(torch.from_numpy(data), nt=crop[0], nz=crop[1], nx=crop[2], n_samp_pts_per_crop=4,
                            downsamp_t=downsamp_t, downsamp_xz=downsamp_xz, lres_filter=kind)
    want = dl.lres_filter(ld._crops(ids).permute(0, 4, 1, 2, 3), kind, downsamp_t, downsamp_xz).permute(0, 2, 3, 4, 1)
    if kind == "maximum":
        radii, w = (downsamp_t - 1, downsamp_xz - 1, downsamp_xz - 1), [None] * 3
    else:
        w = [None if t is None else t.numpy() for t in dl.filter_axis_weights(kind, downsamp_t, downsamp_xz, "cpu")]
        radii = [0 if t is None else (len(t) - 1) // 2 for t in w]
    g = M.Geometry(DATASET, crop, len(ids))
    got, launches, oob = M.run_filter(g, ld.data_cl.numpy(), ids, kind, radii, w)
    _inside(launches)
    assert oob == 0
    got, want = torch.from_numpy(got), want.contiguous()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))
    if bits:                                                         # the sign of zero too
        assert torch.equal(torch.nan_to_num(got, nan=7.0).view(torch.int32), torch.nan_to_num(want, nan=7.0).view(torch.int32))
    return got, radii, launches


def _data(seed=5):
    return torch.randn(4, *DATASET, generator=torch.Generator().manual_seed(seed)).numpy()


@pytest.mark.parametrize("kind", ["gaussian", "uniform", "maximum"])
@pytest.mark.parametrize("ds", [(2, 4), (4, 4), (1, 4), (1, 1)])
def test_model_equals_lres_filter(kind, ds):
    """(2, 4): the base geometry; (4, 4): gaussian radius 8 = nt; (1, 4): the t axis is skipped; (1, 1): every axis is"""
    got, radii, launches = _against_lres_filter(kind, ds[0], ds[1], _data(), [0, 224, 113])
    assert len(launches) == max(1, sum(1 for r in radii if r))
    if ds == (4, 4) and kind == "gaussian":
        assert radii[0] == 8
    if ds[0] == 1:
        assert radii[0] == 0 and all(l[2] != 0 or l[3] == 0 for l in launches)


@pytest.mark.parametrize("kind", ["gaussian", "uniform", "maximum"])
def test_negative_zero(kind):
    """zeros of both signs over whole regions: a pass that runs gives +0.0 (0 + w * -0 = +0), a skipped one keeps -0.0"""
    data = _data()
    data[:, :, :10, :] = -0.0
    data[:, :, 10:14, :] = 0.0
    got, _, _ = _against_lres_filter(kind, 1, 4, data, [0, 224, 113], bits=kind != "maximum")
    if kind != "maximum":
        assert not torch.signbit(got[got == 0]).any() and int((got == 0).sum()) > 0
    data = _data()
    data[:, 3, 4, 5] = -0.0
    got, _, _ = _against_lres_filter(kind, 1, 1, data, [0, 224, 113], bits=True)       # nothing runs: the copy keeps the bits
    assert bool(torch.signbit(got[0, 3, 4, 5]).all()) and bool((got[0, 3, 4, 5] == 0).all())


@pytest.mark.parametrize("kind", ["gaussian", "maximum"])
def test_one_nan_voxel_spreads_over_its_window(kind):
    data = _data()
    data[1, 1, 9, 11] = np.nan                                        # channel 1; t = 1: in crop 0 only, next to its t face
    got, radii, _ = _against_lres_filter(kind, 2, 4, data, [0, 224, 113])
    nan = torch.isnan(got[0])
    assert not nan[..., 0].any() and not nan[..., 2:].any() and not torch.isnan(got[1:]).any()
    box = [range(max(c - r, 0), min(c + r, n - 1) + 1) for c, r, n in zip((1, 9, 11), radii, (8, 16, 16))]
    want = torch.zeros(8, 16, 16, dtype=torch.bool)
    want[box[0].start:box[0].stop, box[1].start:box[1].stop, box[2].start:box[2].stop] = True
    # reflection only folds taps back onto voxels that are within r of the NaN already: the NaN set is the clipped box
    assert torch.equal(nan[..., 1], want) and int(want.sum()) > 1


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _cpu_loader(kind):
    return dl.RB2DeviceLoader(torch.randn(4, 12, 20, 24), nx=16, nz=16, nt=8, n_samp_pts_per_crop=67, downsamp_xz=4,
                              downsamp_t=2, lres_filter=kind)


def test_filter_on_device_refuses_median_by_name():
    with pytest.raises(NotImplementedError) as e:
        dl.DeviceBatchSampler(_cpu_loader("median"), 3, filter_on_device=True)
    assert "median" in str(e.value) and "RB2DeviceLoader.get()" in str(e.value)


@pytest.mark.parametrize("kind", ["gaussian", "uniform", "maximum", "none"])
def test_filter_on_device_accepts_the_three_kinds(kind):
    """past the filter check: what stops a host loader is the device check (the sampler is device-only)"""
    with pytest.raises(RuntimeError) as e:
        dl.DeviceBatchSampler(_cpu_loader(kind), 3, filter_on_device=True)
    assert not isinstance(e.value, NotImplementedError) and "HIP device" in str(e.value)


def test_the_default_still_refuses_a_filtering_loader():
    for kind in ("gaussian", "uniform", "maximum", "median"):
        for kw in ({}, {"filter_on_device": False}):
            with pytest.raises(NotImplementedError) as e:
                dl.DeviceBatchSampler(_cpu_loader(kind), 3, **kw)
            assert ("DeviceBatchSampler does not filter (lres_filter=%r): RB2DeviceLoader.get() is the path that applies the "
                    "low-res filters" % kind) in str(e.value)


def test_weight_tables_are_the_expressions_of_lres_filter():
    g = dl.filter_axis_weights("gaussian", 2, 4, "cpu")
    assert [w.numel() for w in g] == [9, 17, 17] and all(w.dtype == torch.float32 for w in g)
    k = torch.arange(-8, 9, dtype=torch.float64)
    w = torch.exp(-0.5 * k * k / 4.0)
    assert torch.equal(g[1], (w / w.sum()).float())
    assert dl.filter_axis_weights("gaussian", 1, 4, "cpu")[0] is None                   # sigma = 0: skipped
    u = dl.filter_axis_weights("uniform", 2, 4, "cpu")
    assert [w.numel() for w in u] == [3, 7, 7] and torch.equal(u[2], torch.full((7,), 1.0 / 7))
    assert dl.filter_axis_weights("uniform", 1, 4, "cpu")[0] is None                    # window 1: skipped
    with pytest.raises(ValueError):
        dl.filter_axis_weights("maximum", 2, 4, "cpu")


# ---- the entry points --------------------------------------------------------------------------------------------------------
def _fdesc(**kw):
    d = _lib.SamplerFilterDesc()
    d.T, d.Z, d.X = 12, 20, 24
    d.nt, d.nz, d.nx = 8, 16, 16
    d.rt, d.rz, d.rx = 5, 5, 9
    d.B, d.kind = 3, 1
    for k, (r, nw) in enumerate(((4, 9), (8, 17), (8, 17))):
        d.r[k], d.nw[k] = r, nw
    for k, v in kw.items():
        if k in ("r", "nw"):
            for j in range(3):
                getattr(d, k)[j] = v[j]
        else:
            setattr(d, k, v)
    return d


def _filter(hiplib, d, ptrs=None):
    ptrs = [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ctypes.c_void_p(512)] if ptrs is None else ptrs
    return hiplib.stpde_sampler_filter(None if d is None else ctypes.byref(d), *ptrs, None)


def test_new_entry_points_are_exported_and_the_abi_version_stays(hiplib):
    for name in ("stpde_sampler_filter", "stpde_sampler_produce_filtered"):
        assert hasattr(hiplib, name) and name in _lib.exported_symbols()
    assert hiplib.stpde_version() == 316 and _lib.ABI_VERSION == 316                      # additive symbols
    assert ctypes.sizeof(_lib.SamplerFilterDesc) == 17 * 4
    assert ctypes.sizeof(_lib.SamplerDesc) == (16 + 8 + 9) * 4                             # the old descriptor is untouched
    assert _lib.FILTER_KINDS == {"gaussian": 1, "uniform": 2, "maximum": 3}


BAD = [
    (dict(kind=0), "kind must be 1 (gaussian), 2 (uniform) or 3 (maximum)"),
    (dict(kind=4), "kind must be 1 (gaussian), 2 (uniform) or 3 (maximum)"),
    (dict(nw=(9, 17, 15)), "radius 8 of axis 2 does not match its table of 15 weights"),
    (dict(nw=(0, 17, 17)), "radius 4 of axis 0 does not match its table of 0 weights"),
    (dict(r=(0, 8, 8)), "radius 0 of axis 0 does not match its table of 9 weights"),
    (dict(kind=3), "does not match its table"),                                          # maximum takes no tables
    (dict(r=(-1, 8, 8)), "outside [0, 2^20]"),
    (dict(r=(4, 8, 2 ** 20 + 1), nw=(9, 17, 2 ** 21 + 3)), "outside [0, 2^20]"),
    (dict(B=0), "B must be positive"),
    (dict(nt=13), "larger than the dataset"),
    (dict(nx=1, rx=24), "crop needs >= 2 nodes"),
    (dict(rz=6), "inconsistent with the extents"),
    (dict(T=1310, Z=1300, X=1300, rt=1303, rz=1285, rx=1285), "below 2^31"),
    (dict(B=2 ** 20), "B * nt * nz * nx must be below 2^31"),
]


@pytest.mark.parametrize("change,why", BAD)
def test_bad_filter_descriptors_are_refused_with_a_reason(hiplib, change, why):
    with pytest.raises(ValueError) as e:
        _lib.check(_filter(hiplib, _fdesc(**change)))
    assert why in str(e.value) and "sampler_filter" in str(e.value), str(e.value)


def test_filter_pointers_are_checked(hiplib):
    with pytest.raises(ValueError) as e:
        _lib.check(_filter(hiplib, None))
    assert "null descriptor" in str(e.value)
    good = [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ctypes.c_void_p(512)]
    for k in range(8):                                               # state, data_cl, crop_idx, w_t, w_z, w_x, scratch_a, scratch_b
        ptrs = list(good)
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(_filter(hiplib, _fdesc(), ptrs))
        assert "null pointer" in str(e.value), k
    mx = _fdesc(kind=3, nw=(0, 0, 0))                                # maximum: no tables, their pointers may be null ...
    ptrs = list(good)
    ptrs[3] = ptrs[4] = ptrs[5] = None
    ptrs[6] = None                                                   # ... so what is refused here is scratch_a
    with pytest.raises(ValueError) as e:
        _lib.check(_filter(hiplib, mx, ptrs))
    assert "null pointer" in str(e.value) and "weights" not in str(e.value)
    for k in (1, 6, 7):
        ptrs = list(good)
        ptrs[k] = ctypes.c_void_p(260)
        with pytest.raises(ValueError) as e:
            _lib.check(_filter(hiplib, _fdesc(), ptrs))
        assert "16-byte aligned" in str(e.value)
    ptrs = list(good)
    ptrs[7] = ptrs[6]
    with pytest.raises(ValueError) as e:
        _lib.check(_filter(hiplib, _fdesc(), ptrs))
    assert "different buffers" in str(e.value)


def _sdesc(**kw):
    d = _lib.SamplerDesc()
    d.T, d.Z, d.X = 12, 20, 24
    d.nt, d.nz, d.nx = 8, 16, 16
    d.ntl, d.nzl, d.nxl = 4, 4, 4
    d.rt, d.rz, d.rx = 5, 5, 9
    d.B, d.N, d.interp, d.normalize = 3, 67, 0, 0
    for c in range(4):
        d.mean[c], d.std[c] = 0.0, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_filtered_produce_checks_its_arguments(hiplib):
    entry = hiplib.stpde_sampler_produce_filtered
    for change, why in ((dict(ntl=3), "must divide the crop"), (dict(interp=2), "interp must be 0 (linear) or 1 (nearest)"),
                        (dict(N=0), "B and N must be positive")):
        with pytest.raises(ValueError) as e:
            _lib.check(entry(ctypes.byref(_sdesc(**change)), *([FAKE] * 7), None))
        assert why in str(e.value) and "sampler_produce_filtered" in str(e.value)
    with pytest.raises(ValueError) as e:
        _lib.check(entry(None, *([FAKE] * 7), None))
    assert "null descriptor" in str(e.value)
    for k in range(7):
        ptrs = [FAKE] * 7
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(entry(ctypes.byref(_sdesc()), *ptrs, None))
        assert "null pointer" in str(e.value), k
    ptrs = [FAKE] * 7
    ptrs[0] = ctypes.c_void_p(260)
    with pytest.raises(ValueError) as e:
        _lib.check(entry(ctypes.byref(_sdesc()), *ptrs, None))
    assert "16-byte aligned" in str(e.value)
