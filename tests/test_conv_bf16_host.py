"""bf16-operand mode of the U-Net's 3x3x3 convolutions (stpde_conv3d_desc.mfma_bf16, unet3d.set_conv_precision): the parts
that need no GPU -- descriptor layout, argument checks of the five entry points, the Python switch."""
import ctypes
import os
import subprocess
import sys

import pytest

from space_time_pde_amd import _lib, unet3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch


def test_descriptor_ends_with_mfma_bf16():
    names = [f[0] for f in _lib.Conv3dDesc._fields_]
    assert names[-1] == "mfma_bf16" and names[-2] == "det"
    assert ctypes.sizeof(_lib.Conv3dDesc) == 9 * 4


def _desc(ksize, mode):
    d = _lib.Conv3dDesc()
    d.B, d.T, d.Z, d.X, d.Ci, d.Co, d.ksize = 1, 4, 4, 32, 16, 16, ksize
    d.mfma_bf16 = mode
    return d


def _calls(hiplib, d):
    """the five conv entry points on descriptor d (fake, non-null pointers)"""
    def fused():
        a = _lib.Conv3dFusedArgs()
        a.d = d
        a.x = a.w_pack = a.y = FAKE
        return hiplib.stpde_conv3d_fused(ctypes.byref(a), None, None)
    return {
        "fwd": lambda: hiplib.stpde_conv3d_fwd(ctypes.byref(d), FAKE, FAKE, None, FAKE, None),
        "wgrad": lambda: hiplib.stpde_conv3d_wgrad(ctypes.byref(d), FAKE, FAKE, FAKE, None),
        "wgrad_bias": lambda: hiplib.stpde_conv3d_wgrad_bias(ctypes.byref(d), FAKE, FAKE, FAKE, FAKE, None),
        "wgrad_onload": lambda: hiplib.stpde_conv3d_wgrad_onload(ctypes.byref(d), FAKE, FAKE, FAKE, FAKE, FAKE, None, None,
                                                                 None),
        "fused": fused,
    }


@pytest.mark.parametrize("entry", ["fwd", "wgrad", "wgrad_bias", "wgrad_onload", "fused"])
@pytest.mark.parametrize("ksize,mode,why", [(3, 2, "mfma_bf16 = 2"), (3, 3, "mfma_bf16 = 3"), (3, -1, "mfma_bf16 = -1"),
                                            (1, 1, "ksize 1")])
def test_bad_modes_are_refused_with_a_reason(hiplib, entry, ksize, mode, why):
    d = _desc(ksize, mode)
    with pytest.raises(ValueError) as e:
        _lib.check(_calls(hiplib, d)[entry]())
    assert "mfma_bf16" in str(e.value) and why in str(e.value), str(e.value)


def test_fp32_mode_of_a_1x1x1_descriptor_still_passes_the_mode_check(hiplib):
    """mfma_bf16 = 0 is today's path: the same fake call is refused for its null pointers, not for the mode"""
    d = _desc(1, 0)
    rc = hiplib.stpde_conv3d_fwd(ctypes.byref(d), None, FAKE, None, FAKE, None)
    with pytest.raises(ValueError) as e:
        _lib.check(rc)
    assert "mfma_bf16" not in str(e.value)


def test_set_conv_precision_validates_and_round_trips():
    prev = unet3d.set_conv_precision("bf16")
    try:
        assert unet3d.conv_precision == "bf16" and unet3d._bf16() == 1
        assert unet3d.set_conv_precision("fp32") == "bf16"
        assert unet3d.conv_precision == "fp32" and unet3d._bf16() == 0
        for bad in ("fp16", "BF16", "fp32x3", None, 1):
            with pytest.raises(ValueError):
                unet3d.set_conv_precision(bad)
        assert unet3d.conv_precision == "fp32"
    finally:
        unet3d.set_conv_precision(prev)


def test_descriptor_mode_follows_the_switch_for_3x3x3_only():
    class T:
        shape = (1, 4, 4, 32, 16)
    assert unet3d._desc(T, 16, 16, 3, 1).mfma_bf16 == 1
    assert unet3d._desc(T, 16, 16, 1, 1).mfma_bf16 == 0       # 1x1x1 convolutions have no bf16 mode
    assert unet3d._desc(T, 16, 16, 3).mfma_bf16 == 0


@pytest.mark.parametrize("env,want", [(None, "fp32"), ("bf16", "bf16"), ("fp32", "fp32")])
def test_default_precision_from_the_environment(env, want):
    e = dict(os.environ)
    e.pop("STPDE_UNET_PRECISION", None)
    if env is not None:
        e["STPDE_UNET_PRECISION"] = env
    out = subprocess.run([sys.executable, "-c", "from space_time_pde_amd import unet3d; print(unet3d.conv_precision)"],
                         cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert out.stdout.decode().strip().splitlines()[-1] == want
