"""Device batch sampler (csrc/sampler.hip, dataloader_spacetime.DeviceBatchSampler): the parts that need no GPU -- the two entry
points and their argument checks, and the host model of the generator (Philox4x32-10, counter layout, the two mappings)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from space_time_pde_amd import _lib
from space_time_pde_amd import dataloader_spacetime as dl

FAKE = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch


def _desc(**kw):
    """the descriptor of the GPU tests' geometry: dataset (12, 20, 24), crop (8, 16, 16), low-res (4, 4, 4), ranges (5, 5, 9)"""
    d = _lib.SamplerDesc()
    d.T, d.Z, d.X = 12, 20, 24
    d.nt, d.nz, d.nx = 8, 16, 16
    d.ntl, d.nzl, d.nxl = 4, 4, 4
    d.rt, d.rz, d.rx = 5, 5, 9
    d.B, d.N, d.interp, d.normalize = 3, 67, 0, 0
    for c in range(4):
        d.mean[c], d.std[c] = 0.0, 1.0
    for k, v in kw.items():
        if k == "std":
            for c in range(4):
                d.std[c] = v[c]
        else:
            setattr(d, k, v)
    return d


def _draw(hiplib, d, state=FAKE, idx=FAKE, pc=FAKE):
    return hiplib.stpde_sampler_draw(ctypes.byref(d), state, idx, pc, None)


def _produce(hiplib, d, ptrs=None):
    ptrs = [FAKE] * 9 if ptrs is None else ptrs
    return hiplib.stpde_sampler_produce(ctypes.byref(d), *ptrs, None)


def test_entry_points_are_exported_and_the_abi_version_stays(hiplib):
    for name in ("stpde_sampler_draw", "stpde_sampler_produce"):
        assert hasattr(hiplib, name) and name in _lib.exported_symbols()
    assert hiplib.stpde_version() == 316 and _lib.ABI_VERSION == 316
    assert ctypes.sizeof(_lib.SamplerState) == 32
    assert _lib.SamplerState.seed.offset == 0 and _lib.SamplerState.offset.offset == 8 and _lib.SamplerState.oob.offset == 16
    assert ctypes.sizeof(_lib.SamplerTap) == 8
    assert ctypes.sizeof(_lib.SamplerDesc) == (16 + 8 + 9) * 4
    assert "sampler.hip" in _lib._SOURCES


BAD = [
    (dict(nt=13), "larger than the dataset"),
    (dict(nx=25), "larger than the dataset"),
    (dict(ntl=3), "must divide the crop"),
    (dict(nxl=5), "must divide the crop"),
    (dict(rz=6), "inconsistent with the extents"),
    (dict(rt=4), "inconsistent with the extents"),
    (dict(T=1310, Z=1300, X=1300, rt=1303, rz=1285, rx=1285), "below 2^31"),      # len = 2,151,546,175 >= 2^31
    (dict(B=0), "B and N must be positive"),
    (dict(N=-1), "B and N must be positive"),
    (dict(interp=2), "interp must be 0 (linear) or 1 (nearest)"),
    (dict(interp=-1), "interp must be 0 (linear) or 1 (nearest)"),
    (dict(normalize=1, std=(1.0, 0.0, 1.0, 1.0)), "zero std"),
]


@pytest.mark.parametrize("entry", ["draw", "produce"])
@pytest.mark.parametrize("change,why", BAD)
def test_bad_descriptors_are_refused_with_a_reason(hiplib, entry, change, why):
    d = _desc(**change)
    rc = _draw(hiplib, d) if entry == "draw" else _produce(hiplib, d)
    with pytest.raises(ValueError) as e:
        _lib.check(rc)
    assert why in str(e.value) and "sampler_" + entry in str(e.value), str(e.value)


def test_null_pointers_are_refused(hiplib):
    d = _desc()
    for kw in (dict(state=None), dict(idx=None), dict(pc=None)):
        with pytest.raises(ValueError) as e:
            _lib.check(_draw(hiplib, d, **kw))
        assert "null pointer" in str(e.value)
    for k in range(9):
        ptrs = [FAKE] * 9
        ptrs[k] = None
        with pytest.raises(ValueError) as e:
            _lib.check(_produce(hiplib, d, ptrs))
        assert "null pointer" in str(e.value), k
    for entry in (hiplib.stpde_sampler_draw, hiplib.stpde_sampler_produce):
        with pytest.raises(ValueError) as e:
            _lib.check(entry(None, *([FAKE] * (3 if entry is hiplib.stpde_sampler_draw else 9)), None))
        assert "null descriptor" in str(e.value)
    ptrs = [FAKE] * 9
    ptrs[1] = ctypes.c_void_p(260)                                  # the dataset is read with 16-byte loads
    with pytest.raises(ValueError) as e:
        _lib.check(_produce(hiplib, d, ptrs))
    assert "16-byte aligned" in str(e.value)


def test_zero_std_is_fine_without_normalisation(hiplib):
    """the same descriptor passes the std check when normalize = 0: refused for its null pointer, not for the std"""
    d = _desc(normalize=0, std=(0.0, 0.0, 0.0, 0.0))
    with pytest.raises(ValueError) as e:
        _lib.check(_draw(hiplib, d, state=None))
    assert "std" not in str(e.value) and "null pointer" in str(e.value)


# ---- the host model ---------------------------------------------------------------------------------------------------------
def _hex(counter, key):
    w = dl.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    return " ".join("%08x" % int(v) for v in w)


def test_philox_known_answers():
    """The published Random123 known-answer vectors of philox4x32-10 (kat_vectors: zeros, all ones, digits of pi), which
    this implementation reproduces from the algorithm's definition (two 32x32->64 multiplies by 0xD2511F53 / 0xCD9E8D57 per
    round, key bumped by 0x9E3779B9 / 0xBB67AE85 between the 10 rounds)."""
    assert _hex([0, 0, 0, 0], [0, 0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex([0xffffffff] * 4, [0xffffffff] * 2) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_counter_layout_and_mappings():
    """counter = (offset_lo, offset_hi, q, purpose), key = (seed_lo, seed_hi); id = (word * len) >> 32; coordinate =
    (word >> 8) * 2^-24 with flat element e = word e % 4 of call e / 4"""
    seed, off, B, N, length = 0x0123456789abcdef, 0x00000005fffffffe, 3, 67, 225
    ids, pc = dl.sampler_expected(seed, off, B, N, length)
    assert ids.dtype == torch.int32 and ids.shape == (B,) and pc.dtype == torch.float32 and pc.shape == (B, N, 3)
    key = [seed & 0xffffffff, seed >> 32]
    w0 = dl.philox4x32_10(np.array([off & 0xffffffff, off >> 32, 0, 0], dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert ids.tolist() == [(int(w) * length) >> 32 for w in w0[:B]]
    flat = pc.reshape(-1)
    for e in (0, 1, 5, 602):                                        # 602 = the last element: word 2 of the ragged call 150
        w = dl.philox4x32_10(np.array([off & 0xffffffff, off >> 32, e // 4, 1], dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert float(flat[e]) == (int(w[e % 4]) >> 8) * 2.0 ** -24


def test_ranges_of_the_host_model():
    ids, pc = dl.sampler_expected(7, 3, 64, 1024, 225)
    assert 0 <= int(ids.min()) and int(ids.max()) < 225
    assert float(pc.min()) >= 0.0 and float(pc.max()) < 1.0
    assert len(set(ids.tolist())) > 16                               # 64 draws out of 225 positions do not collapse
    ids1, _ = dl.sampler_expected(7, 3, 64, 4, 1)
    assert ids1.tolist() == [0] * 64                                 # len = 1: every id is 0
    big, _ = dl.sampler_expected(7, 3, 4096, 1, 2 ** 31 - 1)
    assert 0 <= int(big.min()) and int(big.max()) < 2 ** 31 - 1 and int(big.max()) > 2 ** 30
    with pytest.raises(ValueError):
        dl.sampler_expected(0, 0, 4, 4, 2 ** 31)


def test_offsets_give_different_reproducible_draws_and_carry_into_the_high_word():
    a = dl.sampler_expected(5, 2 ** 32 - 1, 8, 16, 225)
    b = dl.sampler_expected(5, 2 ** 32, 8, 16, 225)
    lo0 = dl.sampler_expected(5, 0, 8, 16, 225)                       # offset 2^32 has offset_lo = 0 like offset 0 ...
    assert not torch.equal(a[1], b[1]) and not torch.equal(b[1], lo0[1])     # ... and differs through offset_hi = 1
    assert not torch.equal(a[0], b[0]) or not torch.equal(b[0], lo0[0])
    for off, want in ((2 ** 32 - 1, a), (2 ** 32, b)):
        again = dl.sampler_expected(5, off, 8, 16, 225)
        assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
    seen = {tuple(dl.sampler_expected(5, off, 8, 16, 225)[1].reshape(-1)[:4].tolist()) for off in range(32)}
    assert len(seen) == 32                                           # draws at different offsets differ
    assert not torch.equal(dl.sampler_expected(6, 0, 8, 16, 225)[1], lo0[1])        # and so do seeds
    assert not torch.equal(dl.sampler_expected(5 + 2 ** 32, 0, 8, 16, 225)[1], lo0[1])     # seed_hi is part of the key
    assert torch.equal(dl.sampler_expected(5 + 2 ** 64, 0, 8, 16, 225)[1], lo0[1])          # 64 bits of seed


def test_mean_of_the_uniforms():
    """2^16 draws: |mean - 0.5| <= 5 sigma, sigma = 1 / sqrt(12 * 2^16)"""
    _, pc = dl.sampler_expected(0, 0, 16, 4096, 225)                # 16 * 4096 = 2^16 points; the first coordinate of each
    u = pc[..., 0].double().reshape(-1)
    assert u.numel() == 2 ** 16
    assert abs(float(u.mean()) - 0.5) <= 5.0 / math.sqrt(12 * 2 ** 16)
    allu = pc.double().reshape(-1)                                   # and all 3 * 2^16 of them, with their own sigma
    assert abs(float(allu.mean()) - 0.5) <= 5.0 / math.sqrt(12 * 3 * 2 ** 16)


def test_a_filtering_loader_is_refused_by_name():
    ld = dl.RB2DeviceLoader(torch.randn(4, 12, 20, 24), nx=16, nz=16, nt=8, n_samp_pts_per_crop=67, downsamp_xz=4, downsamp_t=2,
                            lres_filter="gaussian")
    with pytest.raises(NotImplementedError) as e:
        dl.DeviceBatchSampler(ld, 3)
    assert "RB2DeviceLoader.get()" in str(e.value)
    ld.lres_filter = "none"
    with pytest.raises(RuntimeError):                                # no host path: the sampler is device-only
        dl.DeviceBatchSampler(ld, 3)
