"""Resource usage of the exact-fp32 first-hidden-layer weight-gradient kernels (csrc/jet_wgrad_impl.h: k_wgrad_coop, MODE 1).

The kernel holds two loop bodies behind a uniform branch: the lock-step loop (ring reads + MFMAs, then the preparation of the
next row tile, adjoint blocks transposed through an LDS patch) and the phase-swapped loop (waves 4 .. 7 prepare first), which
keeps the next tile's adjoint operand set in flight next to the current one and the 64 accumulator registers.  A workgroup is 8 waves, two per SIMD, so a wave may use
256 registers; a body that does not fit spills to scratch without failing any numerical test.  This reads the metadata note of
the built gfx950 code object: no private segment, at most 256 vector registers (accumulator registers included), for the
softplus instantiation (S = (3,1)) the benchmark times and for the piecewise-linear one (S = (3,0), leaky-relu).
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_dpp_hazard as chk  # noqa: E402  (BUILD, LLVM: where the objects and the binary tools are)

# (object file, mangled-name prefix): k_wgrad_coop<S1, S2, MODE 1, ACT, KC 8, HASX false, BF false, SPL 1, PKM 0>
KERNELS = [("jet_wgrad_s31.hip.o", "_Z12k_wgrad_coopILi3ELi1ELi1ELi2ELi8ELb0ELb0ELi1ELi0E"),      # softplus
           ("jet_wgrad_s30.hip.o", "_Z12k_wgrad_coopILi3ELi0ELi1ELi5ELi8ELb0ELb0ELi1ELi0E")]      # leaky-relu


def _metadata(obj, scratch):
    """{kernel name: {key: int}} from the AMDGPU metadata note of the gfx950 code object embedded in a host object."""
    base = os.path.join(scratch, os.path.basename(obj))
    fat, co = base + ".fat", base + ".co"
    subprocess.run([os.path.join(chk.LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, base + ".tmp"], check=True)
    subprocess.run([os.path.join(chk.LLVM, "clang-offload-bundler"), "--type=o", "--input=" + fat, "--unbundle",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    text = subprocess.run([os.path.join(chk.LLVM, "llvm-readelf"), "--notes", co], stdout=subprocess.PIPE,
                          check=True).stdout.decode(errors="replace")
    out = {}
    # one YAML list item per kernel ("  - .agpr_count: 0" opens it); the keys of an item are sorted, .name among them
    for item in re.split(r"\n\s+- (?=\.\w+:)", text):
        name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
        if name and ".private_segment_fixed_size" in item:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*(?:- )?\.(\w+):\s+(\d+)\s*$", item, re.M)}
    return out


@pytest.mark.parametrize("obj,prefix", KERNELS)
def test_both_loop_bodies_fit_the_register_file_without_scratch(obj, prefix):
    path = os.path.join(chk.BUILD, obj)
    if not os.path.exists(path):
        pytest.skip("no object files next to the library (a tree that received only the built .so)")
    with tempfile.TemporaryDirectory() as scratch:
        meta = _metadata(path, scratch)
    mine = {k: v for k, v in meta.items() if k.startswith(prefix)}
    assert len(mine) == 1, (prefix, sorted(meta)[:8])
    (name, m), = mine.items()
    print(name, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size",
                                   "vgpr_spill_count", "group_segment_fixed_size") if k in m})
    assert m["private_segment_fixed_size"] == 0, m
    assert m.get("vgpr_spill_count", 0) == 0, m
    assert m["vgpr_count"] <= 256, m
