"""Numpy model of the low-res filter passes of the device batch sampler (host-logic tests only).

``filter_pass`` restates k_sampler_filter_pass of csrc/sampler.hip for all of its threads at once -- the same integer arithmetic
for every address (crop-id clamp, crop origin, the reflected tap index, the scratch offsets), the same fp32 expression sequence
for the values -- and records every element index it reads or writes, so a CPU test can show that no crop id, radius or extent
forms an address outside a buffer before the kernel ever runs.  ``run_filter`` restates the pass sequence of
stpde_sampler_filter (which axes run, which scratch crop each pass writes, the plain copy when none runs).
"""
import numpy as np

F32 = np.float32


class Geometry:
    """what stpde_sampler_filter_desc carries: dataset (T, Z, X), crop (nt, nz, nx), B; the ranges follow"""

    def __init__(self, dataset, crop, B):
        self.T, self.Z, self.X = dataset
        self.nt, self.nz, self.nx = crop
        self.rt, self.rz, self.rx = (self.T - self.nt + 1, self.Z - self.nz + 1, self.X - self.nx + 1)
        self.B = B
        self.per = self.nt * self.nz * self.nx

    def __len__(self):
        return self.rt * self.rz * self.rx


def filter_pass(g, src, crop_idx, axis, r, w, is_max, first):
    """One launch.  src: the flat dataset [T*Z*X*4] (first) or a flat scratch crop [B*per*4]; crop_idx int32 [B] (read by a
    first pass only); w fp32 [2r + 1] or None (maximum).  Returns (dst flat [B*per*4] fp32 with NaN where nothing was written,
    touched = {"src", "dst", "crop_idx", "w"} -> int64 arrays of flat element indices, oob = ids counted)."""
    nthreads = (g.B * g.per + 255) // 256 * 256
    v = np.arange(nthreads, dtype=np.int64)
    v = v[v < g.B * g.per]                                           # the kernel's early return
    b, rem = v // g.per, v % g.per
    x, z, t = rem % g.nx, (rem // g.nx) % g.nz, rem // (g.nx * g.nz)
    touched = {"src": [], "dst": [], "crop_idx": [], "w": []}
    oob = 0
    if first:
        sZ = g.X * 4
        sT = g.Z * sZ
        touched["crop_idx"].append(b)
        raw = crop_idx.astype(np.int32)[b]
        ln = np.int32(len(g))
        idc = np.where(raw < 0, np.int32(0), np.where(raw > ln - 1, ln - 1, raw)).astype(np.int64)   # BEFORE any address
        oob = int(np.count_nonzero((rem == 0) & (idc != raw)))
        base = (idc // (g.rz * g.rx)) * sT + ((idc // g.rx) % g.rz) * sZ + (idc % g.rx) * 4
    else:
        sZ = g.nx * 4
        sT = g.nz * sZ
        base = b * g.per * 4
    i = (t, z, x)[axis]
    n = (g.nt, g.nz, g.nx)[axis]
    sA = (sT, sZ, 4)[axis]
    line = base + (0 if axis == 0 else t * sT) + (0 if axis == 1 else z * sZ) + (0 if axis == 2 else x * 4)
    n2 = 2 * n
    m = np.fmod(i - r, n2)                                           # C's %: truncates towards zero
    m = np.where(m < 0, m + n2, m)
    acc = np.zeros((v.size, 4), dtype=F32)
    chan = np.arange(4, dtype=np.int64)
    for k in range(2 * r + 1):
        j = np.where(m < n, m, n2 - 1 - m)
        at = (line + j * sA)[:, None] + chan
        touched["src"].append(at.reshape(-1))
        u = src[np.clip(at, 0, src.size - 1)]                        # (the clip only keeps the MODEL from faulting; the
        if is_max:                                                   #  recorded index is the unclipped one)
            if k == 0:
                acc = u.copy()
            else:
                with np.errstate(invalid="ignore"):
                    acc = np.where((u > acc) | (u != u), u, acc)
        else:
            touched["w"].append(np.array([k]))
            acc = acc + u * F32(w[k])                                # a multiply, then an add, in fp32
        m = np.where(m + 1 == n2, 0, m + 1)
    dst = np.full(g.B * g.per * 4, np.nan, dtype=F32)
    at = (v * 4)[:, None] + chan
    touched["dst"].append(at.reshape(-1))
    ok = (at >= 0) & (at < dst.size)
    dst[at[ok]] = acc[ok]
    return dst, {k_: (np.concatenate(a) if a else np.zeros(0, np.int64)) for k_, a in touched.items()}, oob


def run_filter(g, data_cl, crop_idx, kind, radii, weights):
    """stpde_sampler_filter: data_cl [T, Z, X, 4] fp32, crop_idx [B], kind 'gaussian' / 'uniform' / 'maximum', radii (t, z, x),
    weights: per axis an fp32 array of 2r + 1 entries or None.  Returns (scratch_a as [B, nt, nz, nx, 4], launches, oob) with
    launches = [(is_max, first, axis, r, writes, touched, sizes)], ``writes`` 'a' / 'b', ``sizes`` the element count of every
    buffer the launch touches."""
    is_max = kind == "maximum"
    flat = np.ascontiguousarray(data_cl, dtype=F32).reshape(-1)
    crop_idx = np.asarray(crop_idx, dtype=np.int32)
    scratch = {"a": None, "b": None}
    axes = [k for k in range(3) if radii[k]]
    launches, oob = [], 0

    def launch(src, first, axis, r, w, mx, writes):
        dst, touched, n_oob = filter_pass(g, src, crop_idx, axis, r, w, mx, first)
        sizes = {"src": src.size, "dst": g.B * g.per * 4, "crop_idx": crop_idx.size, "w": 0 if w is None else len(w)}
        launches.append((mx, first, axis, r, writes, touched, sizes))
        scratch[writes] = dst
        return n_oob

    if not axes:                                                     # a plain copy: the maximum of one tap
        oob += launch(flat, True, 0, 0, None, True, "a")
    src = flat
    for p, axis in enumerate(axes):
        writes = "a" if (len(axes) - 1 - p) % 2 == 0 else "b"        # the last pass writes scratch_a
        oob += launch(src, p == 0, axis, radii[axis], None if is_max else weights[axis], is_max, writes)
        src = scratch[writes]
    return scratch["a"].reshape(g.B, g.nt, g.nz, g.nx, 4), launches, oob
