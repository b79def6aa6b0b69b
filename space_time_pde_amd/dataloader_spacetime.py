"""On-device space-time crop pipeline: what RB2DataLoader.__getitem__ does on the host with
numpy + scipy (experiments/rb2d/dataloader_spacetime.py:118-171), done on the GPU with the HIP multilinear
interpolation kernel (``stpde_interp_fwd`` via regular_nd_grid_interpolation): random crop, linear down-sampling to
the low-resolution input grid, random query points with trilinearly interpolated targets, channel normalisation.

``RB2DeviceLoader`` is the batched device pipeline (any [4, T, Z, X] tensor or the reference's ``.npz`` with arrays
p, b, u, w of shape [t, x, z], experiments/rb2d/README.md:18-43); ``RB2DataLoader`` is the drop-in ``Dataset`` with the
reference's constructor signature (:18-21) and ``__getitem__`` tuple (:118-171), including ``lres_filter``
(none / gaussian / uniform / median / maximum with scipy.ndimage's 'reflect' boundary, :96-116), ``lres_interp``
(linear / nearest), ``normalize_output`` / ``normalize_hres`` / ``return_hres``.  Both are checked against vectors
produced by the imported reference loader (tests/golden/n3_dataloader.npz).

``DeviceBatchSampler`` draws whole training batches of an ``RB2DeviceLoader`` on the device with capturable launches
(csrc/sampler.hip), bit-identical to ``RB2DeviceLoader.get()`` on the same crop ids and points -- with
``filter_on_device=True`` also for the gaussian / uniform / maximum pre-filters and with ``median_on_device=True`` for the
median one (csrc/sampler_median.hip; ``lres_median_device`` is that kernel on crops of the caller's own); ``sampler_expected``
is its host model.
"""
import os

import numpy as np
import torch

from .regular_nd_grid_interpolation import regular_nd_grid_interpolation


def _reflect_index(n, r, device):
    """Source indices of an axis of length n padded by r on both sides with scipy.ndimage's mode='reflect'
    (d c b a | a b c d | d c b a: the edge sample is repeated), valid for any r (period 2n)."""
    i = torch.arange(-r, n + r, device=device)
    i = torch.remainder(i, 2 * n)
    return torch.where(i >= n, 2 * n - 1 - i, i)


def _correlate_axis(x, w, dim):
    """1-D correlation of x along ``dim`` with the odd-length weight vector w, 'reflect' boundary."""
    r = (w.numel() - 1) // 2
    n = x.shape[dim]
    xp = x.index_select(dim, _reflect_index(n, r, x.device))
    out = torch.zeros_like(x)
    for k in range(w.numel()):
        out = out + w[k] * xp.narrow(dim, k, n)
    return out


def _window_view(x, sizes):
    """x [..., T, Z, X] -> [..., T, Z, X, prod(sizes)] of the reflect-padded neighbourhoods (odd sizes)."""
    for d, sz in zip((-3, -2, -1), sizes):
        r = (sz - 1) // 2
        if r:
            x = x.index_select(x.dim() + d, _reflect_index(x.shape[d], r, x.device))
    t, z, xx = sizes
    v = x.unfold(-3, t, 1).unfold(-3, z, 1).unfold(-3, xx, 1)      # [..., T, Z, X, t, z, x]
    return v.reshape(v.shape[:-3] + (t * z * xx,))


def filter_axis_weights(kind, downsamp_t, downsamp_xz, device, dtype=torch.float32):
    """The per-axis (t, z, x) correlation weights of the separable pre-filters, ``None`` for an axis the filter skips:
    gaussian = exp(-k^2 / 2 sigma^2), sigma = int(downsamp / 2), |k| <= int(4 sigma + 0.5), normalised in fp64 and then cast
    (skipped when sigma <= 0); uniform = 2 downsamp - 1 taps of 1 / size (skipped when the window is 1).  ``lres_filter`` and
    the device sampler's constructor both take their tables from here."""
    out = []
    if kind == 'gaussian':
        for sigma in (int(downsamp_t / 2), int(downsamp_xz / 2), int(downsamp_xz / 2)):
            if sigma <= 0:
                out.append(None)
                continue
            r = int(4.0 * sigma + 0.5)
            k = torch.arange(-r, r + 1, device=device, dtype=torch.float64)
            w = torch.exp(-0.5 * k * k / (sigma * sigma))
            out.append((w / w.sum()).to(dtype))
    elif kind == 'uniform':
        for sz in (downsamp_t * 2 - 1, downsamp_xz * 2 - 1, downsamp_xz * 2 - 1):
            out.append(torch.full((sz,), 1.0 / sz, device=device, dtype=dtype) if sz > 1 else None)
    else:
        raise ValueError("no weight tables for lres_filter=%r" % (kind,))
    return out


def lres_filter(signal, kind, downsamp_t, downsamp_xz):
    """The reference's pre-filter of the high-res crop (dataloader_spacetime.py:96-116) on a [..., T, Z, X] tensor:
    scipy.ndimage gaussian (sigma = int(downsamp/2) per axis, truncate 4), uniform / median / maximum over a
    (2 downsamp - 1) window, all with the 'reflect' boundary.

    The median unfolds every voxel's whole window (prod(sizes) values per element) before ``torch.median``; it is NOT switched
    over to the HIP selection kernel -- ``lres_median_device`` and ``DeviceBatchSampler(median_on_device=True)`` are."""
    if kind == 'none' or not kind:
        return signal
    sizes = (downsamp_t * 2 - 1, downsamp_xz * 2 - 1, downsamp_xz * 2 - 1)
    if kind in ('gaussian', 'uniform'):
        out = signal
        for dim, w in zip((-3, -2, -1), filter_axis_weights(kind, downsamp_t, downsamp_xz, signal.device, signal.dtype)):
            if w is not None:
                out = _correlate_axis(out, w, signal.dim() + dim)
        return out
    if kind == 'maximum':
        return _window_view(signal, sizes).amax(dim=-1)
    if kind == 'median':
        return _window_view(signal, sizes).median(dim=-1).values     # window sizes are odd: the exact median
    raise NotImplementedError("lres_filter must be one of none/gaussian/uniform/median/maximum")


def lres_median_device(crops_cl, radii):
    """Median filter of channels-last crops [B, nt, nz, nx, 4] (fp32, contiguous, on a HIP device) over the window of
    ``radii`` = (r_t, r_z, r_x), each in [0, 7], 'reflect' boundary at the crop faces: a new tensor of the same shape, equal to
    ``lres_filter(crops.permute(0, 4, 1, 2, 3), 'median', r_t + 1, ...)`` but computed by the selection kernel of
    csrc/sampler_median.hip (``stpde_sampler_median``) without unfolding the windows -- e.g. a whole evaluation crop.  A window
    that holds a NaN gives NaN.  The batch is passed as a dataset [B * nt][nz][nx][4] with crop ids b * nt."""
    import ctypes as C
    from . import _lib
    if not (torch.is_tensor(crops_cl) and crops_cl.is_cuda):
        raise RuntimeError("lres_median_device needs a tensor on a HIP device")
    if crops_cl.dim() != 5 or crops_cl.shape[-1] != 4 or crops_cl.dtype != torch.float32 or not crops_cl.is_contiguous():
        raise ValueError("lres_median_device: crops must be [B, nt, nz, nx, 4] fp32 contiguous, got %s %s"
                         % (tuple(crops_cl.shape), crops_cl.dtype))
    radii = tuple(int(r) for r in radii)
    if len(radii) != 3 or any(not 0 <= r <= _lib.FILTER_MEDIAN_MAX_RADIUS for r in radii):
        raise NotImplementedError("lres_median_device: radii %r, each must be in [0, %d] (downsamp <= %d)"
                                  % (radii, _lib.FILTER_MEDIAN_MAX_RADIUS, _lib.FILTER_MEDIAN_MAX_RADIUS + 1))
    B, nt, nz, nx = crops_cl.shape[:4]
    f = _lib.SamplerFilterDesc()
    f.T, f.Z, f.X = B * nt, nz, nx
    f.nt, f.nz, f.nx = nt, nz, nx
    f.rt, f.rz, f.rx = B * nt - nt + 1, 1, 1
    f.B, f.kind = B, _lib.FILTER_MEDIAN
    for k in range(3):
        f.r[k], f.nw[k] = radii[k], 0
    with _lib.device_of(crops_cl):
        out = torch.empty_like(crops_cl)
        ids = torch.arange(0, B * nt, nt, dtype=torch.int32, device=crops_cl.device)
        state = torch.zeros(4, dtype=torch.int64, device=crops_cl.device)
        _lib.check(_lib.lib().stpde_sampler_median(C.byref(f), _lib.ptr(state), _lib.ptr(crops_cl), _lib.ptr(ids), _lib.ptr(out),
                                                   _lib.stream_ptr()))
    return out


class RB2DeviceLoader:
    def __init__(self, data, nx=128, nz=128, nt=16, n_samp_pts_per_crop=1024, downsamp_xz=4, downsamp_t=4,
                 normalize_output=False, device=None, lres_filter='none', lres_interp='linear'):
        if lres_interp not in ('linear', 'nearest'):
            raise ValueError("lres_interp must be 'linear' or 'nearest'")
        self.lres_filter, self.lres_interp = lres_filter, lres_interp
        self.downsamp_xz, self.downsamp_t = downsamp_xz, downsamp_t
        if isinstance(data, str):
            npz = np.load(data)
            arr = np.stack([npz['p'], npz['b'], npz['u'], npz['w']], axis=0).astype(np.float32)
            data = torch.from_numpy(arr.transpose(0, 1, 3, 2).copy())        # [c, t, z, x] (reference :64-67)
        data = torch.as_tensor(data, dtype=torch.float32)
        if device is not None:
            data = data.to(device)
        if data.dim() != 4 or data.shape[0] != 4:
            raise ValueError("data must be [4, T, Z, X] (p, b, u, w)")
        _, nt_d, nz_d, nx_d = data.shape
        if nx > nx_d or nz > nz_d or nt > nt_d:
            raise ValueError('Resolution in each spatial temporal dimension x ({}), z({}), t({})'
                             'must not exceed dataset limits x ({}) z ({}) t ({})'.format(nx, nz, nt, nx_d, nz_d, nt_d))
        if (nt % downsamp_t != 0) or (nx % downsamp_xz != 0) or (nz % downsamp_xz != 0):
            raise ValueError('nx, nz and nt must be divisible by downsamp factor.')
        self.data = data
        self.data_cl = data.permute(1, 2, 3, 0).contiguous()                  # [T, Z, X, c] for the gather kernels
        self.nx_hres, self.nz_hres, self.nt_hres = nx, nz, nt
        self.nx_lres, self.nz_lres, self.nt_lres = nx // downsamp_xz, nz // downsamp_xz, nt // downsamp_t
        self.n_samp_pts_per_crop = n_samp_pts_per_crop
        self.normalize_output = normalize_output
        self.scale_hres = np.array([nt, nz, nx], dtype=np.int32)
        self.scale_lres = np.array([self.nt_lres, self.nz_lres, self.nx_lres], dtype=np.int32)
        self._ranges = (nt_d - nt + 1, nz_d - nz + 1, nx_d - nx + 1)
        self._mean = data.mean(dim=(1, 2, 3))
        self._std = data.std(dim=(1, 2, 3), unbiased=False)
        dev = data.device
        # low-res lattice in high-res index units: linspace(0, n_hres-1, n_lres) per axis (reference :146-150)
        axes = [torch.linspace(0, n - 1, m, device=dev) for n, m in
                zip((nt, nz, nx), (self.nt_lres, self.nz_lres, self.nx_lres))]
        self._lres_coord = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(1, -1, 3)
        self._lres_taps = []
        for a, n in zip(axes, (nt, nz, nx)):
            i0 = torch.clamp(torch.floor(a.double()).long(), 0, max(n - 2, 0))
            a64 = torch.linspace(0, n - 1, a.numel(), device=dev, dtype=torch.float64)
            self._lres_taps.append((i0, (a64 - i0).float()))
        self._xmax = tuple(float(n - 1) for n in (nt, nz, nx))

    def __len__(self):
        return self._ranges[0] * self._ranges[1] * self._ranges[2]

    @property
    def channel_mean(self):
        return self._mean

    @property
    def channel_std(self):
        return self._std

    def _crops(self, idx):
        """idx [B] flat crop ids -> high-res crops [B, nt, nz, nx, 4] (channels-last)."""
        idx = torch.as_tensor(idx, device=self.data.device).long().reshape(-1)
        nzr, nxr = self._ranges[1], self._ranges[2]
        t0, z0, x0 = idx // (nzr * nxr), (idx // nxr) % nzr, idx % nxr        # C-order meshgrid (reference :82-86)
        crops = [self.data_cl[t:t + self.nt_hres, z:z + self.nz_hres, x:x + self.nx_hres]
                 for t, z, x in zip(t0.tolist(), z0.tolist(), x0.tolist())]
        return torch.stack(crops, 0).contiguous()

    def get(self, idx, generator=None, point_coord=None):
        """Batch of crops.  Returns (lres [B,4,nt_l,nz_l,nx_l], point_coord [B,N,3] in (0,1), point_value [B,N,4])."""
        hres = self._crops(idx)
        B = hres.shape[0]
        dev = hres.device
        zeros = (0., 0., 0.)
        if self.lres_filter and self.lres_filter != 'none':
            # the reference interpolates BOTH the low-res grid and the point targets from the filtered crop (:136-155)
            hres = lres_filter(hres.permute(0, 4, 1, 2, 3), self.lres_filter, self.downsamp_t,
                               self.downsamp_xz).permute(0, 2, 3, 4, 1).contiguous()
        if point_coord is None:
            point_coord = torch.rand(B, self.n_samp_pts_per_crop, 3, generator=generator,
                                     device=dev if generator is None or generator.device.type != "cpu" else "cpu").to(dev)
        scale = torch.tensor(self._xmax, device=dev)
        lcoord = self._lres_coord.expand(B, -1, 3).contiguous()
        pcoord = (point_coord * scale).contiguous()
        if self.lres_interp == 'nearest':
            lres, point_value = self._nearest(hres, lcoord), self._nearest(hres, pcoord)
        else:
            # the low-res lattice is structured (linspace per axis, end points ON the crop faces): separable two-tap
            # resampling per axis, exact at the faces (the general-point kernel clips coordinates by 1e-6 of the box like
            # the reference's own interpolation routine does, which scipy's interpolator -- used here by the reference --
            # does not); the random sample points go through the HIP multilinear-interpolation kernel
            lres = hres
            for dim, (i0, w) in zip((1, 2, 3), self._lres_taps):
                lo, hi = lres.index_select(dim, i0), lres.index_select(dim, i0 + 1)
                shape = [1] * lres.dim()
                shape[dim] = -1
                lres = lo + (hi - lo) * w.view(shape)
            point_value = regular_nd_grid_interpolation(hres, pcoord, zeros, self._xmax)
        lres = lres.reshape(B, self.nt_lres, self.nz_lres, self.nx_lres, 4).permute(0, 4, 1, 2, 3).contiguous()
        if self.normalize_output:
            lres = (lres - self._mean.view(1, 4, 1, 1, 1)) / self._std.view(1, 4, 1, 1, 1)
            point_value = (point_value - self._mean) / self._std
        return lres, point_coord, point_value

    @staticmethod
    def _nearest(hres, coord):
        """scipy RegularGridInterpolator(method='nearest') on the unit-spaced crop lattice: node i + 1 when the
        fractional position inside cell i exceeds 0.5, else node i (ties go down)."""
        n = torch.tensor(hres.shape[1:4], device=hres.device)
        i = torch.minimum(torch.clamp(torch.floor(coord), min=0).long(), n - 2)
        idx = torch.where(coord - i <= 0.5, i, i + 1)
        b = torch.arange(hres.shape[0], device=hres.device).view(-1, 1).expand(idx.shape[:2])
        return hres[b, idx[..., 0], idx[..., 1], idx[..., 2]]

    def hres_crop(self, idx):
        """[B, 4, nt, nz, nx] unfiltered high-resolution crops (the reference's return_hres output)."""
        return self._crops(idx).permute(0, 4, 1, 2, 3).contiguous()

    def __getitem__(self, idx):
        lres, pc, pv = self.get([idx])
        return lres[0], pc[0], pv[0]

    def normalize_grid(self, grid):
        shape = (4,) + (1,) * (grid.dim() - 1)
        return (grid - self._mean.view(shape).to(grid.device)) / self._std.view(shape).to(grid.device)

    def denormalize_grid(self, grid):
        shape = (4,) + (1,) * (grid.dim() - 1)
        return grid * self._std.view(shape).to(grid.device) + self._mean.view(shape).to(grid.device)

    def normalize_points(self, points):
        return (points - self._mean.to(points.device)) / self._std.to(points.device)

    def denormalize_points(self, points):
        return points * self._std.to(points.device) + self._mean.to(points.device)


# ---- batches drawn and produced on the device (csrc/sampler.hip) ----------------------------------------------------------
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on the host, in numpy integers: ``counter`` [..., 4] and ``key`` [..., 2] (uint32
    values, broadcast against each other) -> [..., 4] uint32 words.  The host model of the device generator."""
    c = np.array(np.broadcast_arrays(*[np.asarray(counter, dtype=np.uint64)[..., i] for i in range(4)]), dtype=np.uint64)
    k0, k1 = [np.asarray(key, dtype=np.uint64)[..., i] for i in range(2)]
    c0, c1, c2, c3 = c
    m32 = np.uint64(_M32)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2        # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & m32, (k1 + np.uint64(_PHILOX_W1)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def sampler_expected(seed, offset, batch_size, n_points, length):
    """Host model of ``stpde_sampler_draw``: the crop ids [B] (int32) and point coordinates [B, N, 3] (fp32) that the draw at
    ``offset`` of the generator seeded with ``seed`` produces for ``length`` crop positions -- the same Philox4x32-10, counter
    layout (offset_lo, offset_hi, q, purpose) and integer mappings as the kernel (include/stpde_hip.h), in plain numpy."""
    seed, offset = int(seed) & _M64, int(offset) & _M64
    if not 0 < int(length) < (1 << 31):
        raise ValueError("length must be in [1, 2^31)")
    key = np.array([seed & _M32, seed >> 32], dtype=np.uint64)

    def words(purpose, n):
        q = np.arange((n + 3) // 4, dtype=np.uint64)
        ctr = np.stack([np.full_like(q, offset & _M32), np.full_like(q, offset >> 32), q, np.full_like(q, purpose)], axis=-1)
        return philox4x32_10(ctr, key).reshape(-1)[:n].astype(np.uint64)

    ids = ((words(0, batch_size) * np.uint64(length)) >> np.uint64(32)).astype(np.int32)
    n = batch_size * n_points * 3
    coord = (words(1, n) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)       # 24 bits: exact in fp32
    return torch.from_numpy(ids), torch.from_numpy(coord.reshape(batch_size, n_points, 3))


def _signed64(v):
    v = int(v) & _M64
    return v - (1 << 64) if v >= (1 << 63) else v


class DeviceBatchSampler:
    """Training batches of an ``RB2DeviceLoader`` drawn AND produced on the device by three kernel launches that are legal
    inside a HIP-graph capture (``stpde_sampler_draw`` / ``stpde_sampler_produce``, csrc/sampler.hip): crop positions (uniform,
    with replacement, like the reference's ``RandomSampler(replacement=True)``, train.py:318-321) and query points come from a
    counter-based generator whose state lives in device memory; the low-resolution grid and the interpolated targets are written
    into static buffers straight from the dataset, bit-identical to ``loader.get()`` on the same ids and points.

        sampler = DeviceBatchSampler(loader, batch_size=10, seed=0)
        lres, point_coord, point_value = sampler.draw()          # the static buffers, rewritten by every draw
        ids, pts = sampler.expected(k)                           # host model: what draw number k produced / will produce

    Every buffer a draw touches is allocated here, once: a captured graph replays addresses.  ``GraphedStep(sampler=...)`` puts
    the draw at the head of every replay.

    Loaders with an ``lres_filter`` are refused by default (``RB2DeviceLoader.get()`` filters).  ``filter_on_device=True``
    accepts ``gaussian`` / ``uniform`` / ``maximum``: every batch is then draw -> up to three 1-D filter passes over two
    scratch crops [B, nt, nz, nx, 4] allocated here (``stpde_sampler_filter``) -> the gather from the filtered crops
    (``stpde_sampler_produce_filtered``), still bit-identical to ``loader.get()``.  ``median`` is not separable and has a
    switch of its own, ``median_on_device=True`` (together with ``filter_on_device=True``), because its cost class differs: the
    other filters take microseconds, a selection over hundreds of window values per voxel takes milliseconds.  A batch is then
    draw -> one selection kernel into ONE scratch crop (``stpde_sampler_median``, radii ``downsamp - 1`` <= 7) -> the same
    gather, equal to ``loader.get()`` (NaN where it has NaN).  With any other loader ``median_on_device`` changes nothing.
    The filter kind and its weight tables are fixed HERE: changing ``loader.lres_filter``
    (or the down-sampling factors) afterwards has no effect on the sampler."""

    def __init__(self, loader, batch_size, seed=0, filter_on_device=False, median_on_device=False):
        kind = loader.lres_filter if loader.lres_filter and loader.lres_filter != 'none' else None
        if kind and not filter_on_device:
            raise NotImplementedError("DeviceBatchSampler does not filter (lres_filter=%r): RB2DeviceLoader.get() is the path "
                                      "that applies the low-res filters (filter_on_device=True filters gaussian / uniform / "
                                      "maximum in the sampler)" % (kind,))
        if kind and kind not in ('gaussian', 'uniform', 'maximum') and not (kind == 'median' and median_on_device):
            raise NotImplementedError("DeviceBatchSampler(filter_on_device=True) has no kernel for lres_filter=%r (gaussian / "
                                      "uniform / maximum are built): RB2DeviceLoader.get() is the path that applies it%s"
                                      % (kind, ", or pass median_on_device=True" if kind == 'median' else ""))
        if kind == 'median':
            from ._lib import FILTER_MEDIAN_MAX_RADIUS as rmax
            if max(loader.downsamp_t, loader.downsamp_xz) - 1 > rmax:
                raise NotImplementedError("DeviceBatchSampler(median_on_device=True): window radius downsamp - 1 = %d above the "
                                          "limit of %d (downsamp_t = %d, downsamp_xz = %d; at most %d)"
                                          % (max(loader.downsamp_t, loader.downsamp_xz) - 1, rmax, loader.downsamp_t,
                                             loader.downsamp_xz, rmax + 1))
        if int(batch_size) <= 0:
            raise ValueError("batch_size must be positive")
        if not loader.data_cl.is_cuda:
            raise RuntimeError("DeviceBatchSampler needs a loader on a HIP device (RB2DeviceLoader(..., device='cuda'))")
        from . import _lib
        from .lig_jet import cached_box_constants
        self.loader, self.batch_size = loader, int(batch_size)
        dev = loader.data_cl.device
        B, N = self.batch_size, int(loader.n_samp_pts_per_crop)
        n = (loader.nt_hres, loader.nz_hres, loader.nx_hres)
        nl = (loader.nt_lres, loader.nz_lres, loader.nx_lres)
        d = _lib.SamplerDesc()
        d.T, d.Z, d.X = loader.data_cl.shape[:3]
        d.nt, d.nz, d.nx = n
        d.ntl, d.nzl, d.nxl = nl
        d.rt, d.rz, d.rx = loader._ranges
        d.B, d.N = B, N
        d.interp = 1 if loader.lres_interp == 'nearest' else 0
        d.normalize = 1 if loader.normalize_output else 0
        mean, std = loader._mean.tolist(), loader._std.tolist()
        lo_c, hi_c, cube = cached_box_constants(n, (0., 0., 0.), loader._xmax)      # what get()'s interpolation call uses
        for c in range(4):
            d.mean[c], d.std[c] = mean[c], std[c]
        for k in range(3):
            d.lo_c[k], d.hi_c[k], d.cube[k] = lo_c[k], hi_c[k], cube[k]
        self._desc = d
        # per-axis tap tables [n_lres] of (int32 i0, fp32 w): linear = the loader's own two-tap tables; nearest = the node that
        # _nearest's rule picks for the loader's own fp32 lattice coordinate (the rule is separable), w unused
        lattice = loader._lres_coord.reshape(nl + (3,))
        axes = (lattice[:, 0, 0, 0], lattice[0, :, 0, 1], lattice[0, 0, :, 2])
        self._taps = []
        for k in range(3):
            if d.interp:
                i = torch.clamp(torch.clamp(torch.floor(axes[k]), min=0).long(), max=n[k] - 2)
                i0, w = torch.where(axes[k] - i <= 0.5, i, i + 1), torch.zeros(nl[k], device=dev)
            else:
                i0, w = loader._lres_taps[k]
            tab = torch.stack([i0.to(torch.int32), w.to(torch.float32).contiguous().view(torch.int32)], dim=1)
            self._taps.append(tab.contiguous().to(dev))
        self.lres = torch.zeros(B, 4, *nl, device=dev)
        self.point_coord = torch.zeros(B, N, 3, device=dev)
        self.point_value = torch.zeros(B, N, 4, device=dev)
        self.crop_idx = torch.zeros(B, dtype=torch.int32, device=dev)
        self._state = torch.zeros(4, dtype=torch.int64, device=dev)     # stpde_sampler_state: seed, offset, oob | pad, pad
        self.filter = kind
        if kind:
            f = _lib.SamplerFilterDesc()
            f.T, f.Z, f.X = d.T, d.Z, d.X
            f.nt, f.nz, f.nx = n
            f.rt, f.rz, f.rx = loader._ranges
            f.B, f.kind = B, _lib.FILTER_MEDIAN if kind == 'median' else _lib.FILTER_KINDS[kind]
            if kind in ('maximum', 'median'):
                self._weights = [None, None, None]
                radii = (loader.downsamp_t - 1, loader.downsamp_xz - 1, loader.downsamp_xz - 1)      # window 2 ds - 1
            else:
                # built on the loader's device with lres_filter's own expressions: the very tables get() multiplies by
                self._weights = [None if w is None else w.contiguous()
                                 for w in filter_axis_weights(kind, loader.downsamp_t, loader.downsamp_xz, dev)]
                radii = [0 if w is None else (w.numel() - 1) // 2 for w in self._weights]
            for k in range(3):
                f.r[k] = radii[k]
                f.nw[k] = 0 if self._weights[k] is None else self._weights[k].numel()
            self._fdesc = f
            if kind == 'median':
                self._scratch = (torch.zeros(B, *n, 4, device=dev),)                                   # ONE crop: no ping-pong
            else:
                self._scratch = (torch.zeros(B, *n, 4, device=dev), torch.zeros(B, *n, 4, device=dev))     # ping-pong crops
        self.seed(seed)

    def __len__(self):
        return len(self.loader)

    # -- state --------------------------------------------------------------------------------------------------------------
    def seed(self, seed, offset=0):
        """(Re)start the sequence: Philox key ``seed``, draw counter ``offset``; the out-of-range count is cleared.  Fills on
        the current stream -- not inside a capture (a replay would reset the counter every time)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DeviceBatchSampler.seed() inside a stream capture")
        self._seed = int(seed) & _M64
        self._state[0].fill_(_signed64(seed))
        self._state[1].fill_(_signed64(offset))
        self._state[2:].fill_(0)

    def offset(self):
        """The draw counter, read back from the device (synchronises)."""
        return int(self._state[1].item()) & _M64

    def oob_count(self):
        """Explicit crop ids outside [0, len) that produce() has clamped since the last seed() (synchronises)."""
        return int(self._state[2].item()) & _M32

    def check(self):
        """Raise if any explicit crop id was out of range (they are clamped on the device, never followed)."""
        n = self.oob_count()
        if n:
            raise IndexError("DeviceBatchSampler: %d crop id(s) outside [0, %d) were clamped into range" % (n, len(self)))

    def state_dict(self):
        return {"seed": self._seed, "offset": self.offset()}

    def load_state_dict(self, state):
        self.seed(state["seed"], state["offset"])

    def expected(self, offset):
        """Host model: (crop ids [B] int32, point_coord [B, N, 3] fp32), CPU tensors, of the draw at ``offset``."""
        return sampler_expected(self._seed, offset, self.batch_size, int(self.loader.n_samp_pts_per_crop), len(self))

    # -- launches -----------------------------------------------------------------------------------------------------------
    def _produce(self, crop_idx, point_coord):
        import ctypes as C
        from . import _lib
        if self.filter:
            sa = self._scratch[0]
            if self.filter == 'median':
                _lib.check(_lib.lib().stpde_sampler_median(
                    C.byref(self._fdesc), _lib.ptr(self._state), _lib.ptr(self.loader.data_cl), _lib.ptr(crop_idx), _lib.ptr(sa),
                    _lib.stream_ptr()))
            else:
                w, sb = self._weights, self._scratch[1]
                _lib.check(_lib.lib().stpde_sampler_filter(
                    C.byref(self._fdesc), _lib.ptr(self._state), _lib.ptr(self.loader.data_cl), _lib.ptr(crop_idx),
                    _lib.ptr(w[0]), _lib.ptr(w[1]), _lib.ptr(w[2]), _lib.ptr(sa), _lib.ptr(sb), _lib.stream_ptr()))
            _lib.check(_lib.lib().stpde_sampler_produce_filtered(
                C.byref(self._desc), _lib.ptr(sa), _lib.ptr(self._taps[0]), _lib.ptr(self._taps[1]), _lib.ptr(self._taps[2]),
                _lib.ptr(point_coord), _lib.ptr(self.lres), _lib.ptr(self.point_value), _lib.stream_ptr()))
            return
        _lib.check(_lib.lib().stpde_sampler_produce(
            C.byref(self._desc), _lib.ptr(self._state), _lib.ptr(self.loader.data_cl), _lib.ptr(self._taps[0]),
            _lib.ptr(self._taps[1]), _lib.ptr(self._taps[2]), _lib.ptr(crop_idx), _lib.ptr(point_coord), _lib.ptr(self.lres),
            _lib.ptr(self.point_value), _lib.stream_ptr()))

    def draw(self):
        """Next batch: two library calls on the current stream (three with a filter: draw, filter passes or the median
        selection, produce from the filtered crops), capturable, no allocation, no synchronisation.  Returns the
        static (lres [B,4,nt_l,nz_l,nx_l], point_coord [B,N,3], point_value [B,N,4]); ``crop_idx`` holds the ids."""
        import ctypes as C
        from . import _lib
        with _lib.device_of(self._state):
            _lib.check(_lib.lib().stpde_sampler_draw(C.byref(self._desc), _lib.ptr(self._state), _lib.ptr(self.crop_idx),
                                                     _lib.ptr(self.point_coord), _lib.stream_ptr()))
            self._produce(self.crop_idx, self.point_coord)
        return self.lres, self.point_coord, self.point_value

    def produce(self, crop_idx, point_coord):
        """Explicit mode: the batch of the given crop ids [B] and points [B, N, 3] in [0, 1] (for parity checks, or a sampling
        scheme of the caller's own); the generator state does not move.  A host sequence of ids is range-checked here
        (IndexError); a device tensor is passed through -- the kernel clamps an id outside [0, len) before it forms any
        address and counts it, see check().  Returns (lres, point_coord, point_value): the static outputs and the given points."""
        from . import _lib
        dev = self._state.device
        if not torch.is_tensor(crop_idx):
            ids = [int(i) for i in crop_idx]
            bad = [i for i in ids if not 0 <= i < len(self)]
            if bad:
                raise IndexError("crop id %d outside [0, %d)" % (bad[0], len(self)))
            crop_idx = torch.tensor(ids, dtype=torch.int32, device=dev)
        crop_idx = crop_idx.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        point_coord = torch.as_tensor(point_coord, dtype=torch.float32).to(dev).contiguous()
        if crop_idx.numel() != self.batch_size or tuple(point_coord.shape) != tuple(self.point_coord.shape):
            raise ValueError("produce() needs %d crop ids and points of shape %s" % (self.batch_size,
                                                                                    tuple(self.point_coord.shape)))
        with _lib.device_of(self._state):
            self._produce(crop_idx, point_coord)
        return self.lres, point_coord, self.point_value


class RB2DataLoader(torch.utils.data.Dataset):
    """Drop-in for the reference ``RB2DataLoader`` (experiments/rb2d/dataloader_spacetime.py:12-257): same constructor
    arguments, ``__len__``, ``__getitem__`` tuple ([hres,] lres, point_coord, point_value), ``channel_mean`` /
    ``channel_std`` and the (de)normalisation helpers -- but every crop is cut, filtered and interpolated on ``device``
    (the HIP interpolation kernel) and returned as float32 tensors there, so the feeder never touches scipy.

    ``numpy_rng=True`` draws the sample points with ``np.random.rand`` exactly like the reference (:153), so a seeded
    numpy stream reproduces the reference's samples; the default draws them on the device.

    ``device=None`` (default) keeps the Dataset on the HOST like the reference's: it then works unchanged under the
    reference's ``DataLoader(..., num_workers=1, pin_memory=True)`` (experiments/rb2d/train.py:318-321; forked workers
    must not touch the GPU and pin_memory rejects device tensors).  ``device="cuda"`` opts into the on-device pipeline:
    use it with ``num_workers=0, pin_memory=False`` (``__getitem__`` raises inside a worker process), or call
    ``RB2DeviceLoader.get`` directly for whole batches."""

    def __init__(self, data_dir="./", data_filename="./data/rb2d_ra1e6_s42.npz", nx=128, nz=128, nt=16,
                 n_samp_pts_per_crop=1024, downsamp_xz=4, downsamp_t=4, normalize_output=False, normalize_hres=False,
                 return_hres=False, lres_filter='none', lres_interp='linear', device=None, numpy_rng=False):
        self.data_dir, self.data_filename = data_dir, data_filename
        self.normalize_hres, self.return_hres, self.numpy_rng = normalize_hres, return_hres, numpy_rng
        if device is None:
            device = "cpu"
        self._on_device = torch.device(device).type != "cpu"
        self._impl = RB2DeviceLoader(os.path.join(data_dir, data_filename), nx=nx, nz=nz, nt=nt,
                                     n_samp_pts_per_crop=n_samp_pts_per_crop, downsamp_xz=downsamp_xz,
                                     downsamp_t=downsamp_t, normalize_output=normalize_output, device=device,
                                     lres_filter=lres_filter, lres_interp=lres_interp)
        for k in ("nx_hres", "nz_hres", "nt_hres", "nx_lres", "nz_lres", "nt_lres", "n_samp_pts_per_crop",
                  "normalize_output", "scale_hres", "scale_lres", "lres_filter", "lres_interp", "downsamp_xz",
                  "downsamp_t", "data"):
            setattr(self, k, getattr(self._impl, k))

    def __len__(self):
        return len(self._impl)

    def __getitem__(self, idx):
        if self._on_device and torch.utils.data.get_worker_info() is not None:
            raise RuntimeError("RB2DataLoader(device=%r) cannot be used from DataLoader worker processes: pass "
                               "num_workers=0, pin_memory=False, or keep the dataset on the host (device=None)"
                               % (str(self._impl.data.device),))
        pc = None
        if self.numpy_rng:
            pc = torch.from_numpy(np.random.rand(self.n_samp_pts_per_crop, 3).astype(np.float32))[None]
            pc = pc.to(self._impl.data.device)
        lres, pc, pv = self._impl.get([idx], point_coord=pc)
        out = [lres[0], pc[0], pv[0]]
        if self.return_hres:
            hres = self._impl.hres_crop([idx])[0]
            out = [self._impl.normalize_grid(hres) if self.normalize_hres else hres] + out
        return tuple(out)

    @property
    def channel_mean(self):
        return self._impl.channel_mean

    @property
    def channel_std(self):
        return self._impl.channel_std

    def normalize_grid(self, grid):
        return self._impl.normalize_grid(grid)

    def normalize_points(self, points):
        return self._impl.normalize_points(points)

    def denormalize_grid(self, grid):
        return self._impl.denormalize_grid(grid)

    def denormalize_points(self, points):
        return self._impl.denormalize_points(points)
