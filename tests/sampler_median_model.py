"""Host model of the median pre-filter (csrc/sampler_median.hip: stpde_sampler_median) in numpy: reflect-pad every axis with
the kernel's index formula (i mod 2n taken into [0, 2n), mirrored into [0, n): scipy's 'reflect', any radius), take the sliding
windows, sort each and pick rank (W - 1) / 2; a window that holds a NaN gives NaN."""
import numpy as np


def reflect_index(n, r):
    """source index of every entry of an axis of length n padded by r on both sides"""
    m = np.mod(np.arange(-r, n + r), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def median_filter(x, radii):
    """x [..., T, Z, X] -> the same shape: per element the value of rank (W - 1) / 2 of its (2 r_t + 1)(2 r_z + 1)(2 r_x + 1)
    window ('reflect' boundary), NaN where the window holds one."""
    x = np.asarray(x)
    p = x
    for axis, r in zip((-3, -2, -1), radii):
        p = np.take(p, reflect_index(x.shape[axis], r), axis=axis)
    sizes = tuple(2 * r + 1 for r in radii)
    win = np.lib.stride_tricks.sliding_window_view(p, sizes, axis=(-3, -2, -1))
    win = win.reshape(win.shape[:-3] + (-1,))
    W = win.shape[-1]
    assert W % 2 == 1 and win.shape[:-1] == x.shape
    nan = np.isnan(win).any(axis=-1)
    out = np.sort(win, axis=-1)[..., (W - 1) // 2].copy()             # np.sort puts NaN last: overwritten below
    out[nan] = np.nan
    return out.astype(x.dtype)
