"""The dim = 3 glue kernels of csrc/lig_gather_reduce.hip, bit for bit against the numpy models of the shared bodies:
stpde_lig_gather (k_gather for c = 8, k_gather_tile for c = 32: X, coef, cell, cw and the optional row-major image XR)
against tests/lig_nd_model.py's ``gather3``, and stpde_lig_dlatent_reduce (k_dlat_reduce) against
tests/lig_nd_bwd_model.py's ``dlatent_reduce_nd`` at D = 3.  The models run fp32 numpy with the kernels' own expression
sequence and summation order, so the comparison is np.array_equal.

Shapes: B = 2, the 37 edge points of tests/lig_nd_model.py plus one per batch item (N = 38: the entry point takes an even
point count); the whole list as one chunk, and a second chunk that starts inside batch item 0 and ends inside item 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import lig_nd_bwd_model as MB
from tests import lig_nd_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2
ALPHA = (0.5, -1.0, 2.0, 0.25, 3.0, -0.75)
CHUNKS = [(0, None), (30, 20)]          # (p_base, P): everything; points 30 .. 49 of 76
_cache = {}


def _inputs(shape, cin, xmax):
    """pts [B * 38, 3], latent [B, *shape, cin] (fp32 numpy) and the box constants: built once, shared, never modified"""
    from space_time_pde_amd.lig_jet import box_constants
    key = (shape, cin)
    if key not in _cache:
        e0, e1 = M.edge_points(shape, xmax, seed=0), M.edge_points(shape, xmax, seed=1)[::-1]
        extra = (np.asarray(xmax, np.float32) * np.ones(3, np.float32) * np.float32(0.37))[None]
        pts = np.concatenate([e0, extra, e1, extra], 0).astype(np.float32)
        latent = np.random.default_rng(7).standard_normal((B,) + shape + (cin,)).astype(np.float32)
        _cache[key] = (pts, latent, box_constants(shape, 0., xmax))
    return _cache[key]


def _model(shape, cin, xmax, p0, pc):
    key = (shape, cin, p0, pc)
    if key not in _cache:
        pts, latent, (lo, hi, cube) = _inputs(shape, cin, xmax)
        _cache[key] = M.gather3(pts[p0:p0 + pc], latent, pts.shape[0] // B, p0, lo, hi, cube, ALPHA)[:4]
    return _cache[key]


def _gather(hiplib, shape, cin, xmax, p0, pc, want_cw, want_xr=False):
    from space_time_pde_amd import _lib
    pts, latent, (lo, hi, cube) = _inputs(shape, cin, xmax)
    gd = _lib.GatherDesc()
    gd.P, gd.N, gd.B, gd.C, gd.p_base = pc, pts.shape[0] // B, B, cin, p0
    gd.n0, gd.n1, gd.n2 = shape
    for k in range(3):
        gd.lo_c[k], gd.hi_c[k], gd.cube[k] = lo[k], hi[k], cube[k]
    for k in range(6):
        gd.alpha[k] = ALPHA[k] if want_cw else 0.0
    nan = float("nan")
    X = torch.full((pc // 2, M.XT, 64, 4), nan, device=DEV)
    XR = torch.full_like(X, nan) if want_xr else None
    coef = torch.full((pc, 16), nan, device=DEV)
    cell = torch.full((pc,), -1, device=DEV, dtype=torch.int32)
    cw = torch.full((pc, 8), nan, device=DEV) if want_cw else None
    d_pts, d_lat = torch.from_numpy(pts[p0:p0 + pc]).to(DEV), torch.from_numpy(latent).to(DEV)
    with _lib.dispatch_trace() as tr:
        _lib.check(hiplib.stpde_lig_gather(C.byref(gd), _lib.ptr(d_pts), _lib.ptr(d_lat), _lib.ptr(X), _lib.ptr(XR),
                                           _lib.ptr(coef), _lib.ptr(cell), _lib.ptr(cw), _lib.stream_ptr()))
    torch.cuda.synchronize()
    kern = "k_gather_tile @" if cin == 32 else "k_gather @"
    assert len(tr.kernels) == 1 and tr.has(kern), tr.kernels
    return X, XR, coef, cell, cw


@pytest.mark.parametrize("want_cw", [True, False])
@pytest.mark.parametrize("p0,pc", CHUNKS)
@pytest.mark.parametrize("dim,shape,cin,xmax", M.D3_GRIDS)
def test_gather_equals_the_model_bitwise(hiplib, dim, shape, cin, xmax, p0, pc, want_cw):
    pc = B * 38 if pc is None else pc
    mX, mcoef, mcell, mcw = _model(shape, cin, xmax, p0, pc)
    X, _, coef, cell, cw = _gather(hiplib, shape, cin, xmax, p0, pc, want_cw)
    assert np.array_equal(X.cpu().numpy(), mX)
    assert np.array_equal(coef.cpu().numpy(), mcoef)
    assert np.array_equal(cell.cpu().numpy(), mcell)
    if want_cw:
        assert np.array_equal(cw.cpu().numpy(), mcw)
    if p0:                                   # the chunk names the cells the whole list names
        assert np.array_equal(mcell, _model(shape, cin, xmax, 0, B * 38)[2][p0:p0 + pc])


@pytest.mark.parametrize("dim,shape,cin,xmax", M.D3_GRIDS)
def test_row_major_image_holds_the_same_values(hiplib, dim, shape, cin, xmax):
    """XR (optional output): lane 16 g + c of a tile holds rows 4g .. 4g + 3 of slot c"""
    p0, pc = CHUNKS[1]
    X, XR, coef, cell, cw = _gather(hiplib, shape, cin, xmax, p0, pc, True, want_xr=True)
    mX, mcoef, mcell, mcw = _model(shape, cin, xmax, p0, pc)
    assert np.array_equal(X.cpu().numpy(), mX) and np.array_equal(XR.cpu().numpy(), M.row_major_image(mX))
    assert np.array_equal(coef.cpu().numpy(), mcoef) and np.array_equal(cell.cpu().numpy(), mcell)
    assert np.array_equal(cw.cpu().numpy(), mcw)


@pytest.mark.parametrize("cin", [8, 30])
@pytest.mark.parametrize("dim,shape,c_gather,xmax", M.D3_GRIDS)
def test_dlatent_reduce_equals_the_model_bitwise(hiplib, dim, shape, c_gather, xmax, cin):
    """perm / start from stpde_lig_cell_sort on the gather's own cell output; c = 30 has CP = 32 > c: the last channel group
    is masked.  Nodes that own no point keep their initial value exactly."""
    from space_time_pde_amd import _lib
    P = B * 38
    cell = _gather(hiplib, shape, c_gather, xmax, 0, P, False)[3]
    n_nodes = B * int(np.prod(shape))
    perm = torch.empty(P, device=DEV, dtype=torch.int32)
    start = torch.empty(n_nodes + 1, device=DEV, dtype=torch.int32)
    nb = int(hiplib.stpde_lig_sort_tmp_bytes(P, n_nodes))
    tmp = torch.empty(nb, device=DEV, dtype=torch.uint8)
    _lib.check(hiplib.stpde_lig_cell_sort(P, n_nodes, _lib.ptr(cell), _lib.ptr(perm), _lib.ptr(start), _lib.ptr(tmp), nb,
                                          _lib.stream_ptr()))
    mperm, mstart = MB.cell_sort(cell.cpu().numpy(), n_nodes)
    assert np.array_equal(perm.cpu().numpy(), mperm) and np.array_equal(start.cpu().numpy(), mstart)
    cp = (cin + 3) // 4 * 4
    rng = np.random.default_rng(11 + cin)
    xrows = rng.standard_normal((8 * P, cp)).astype(np.float32)
    init = rng.standard_normal((n_nodes, cin)).astype(np.float32)
    want = init.copy()
    MB.dlatent_reduce_nd(3, B, shape, cin, xrows, mperm, mstart, want)
    dlat, d_xrows = torch.from_numpy(init).to(DEV), torch.from_numpy(xrows).to(DEV)
    with _lib.dispatch_trace() as tr:
        _lib.check(hiplib.stpde_lig_dlatent_reduce(B, shape[0], shape[1], shape[2], cin, _lib.ptr(d_xrows), _lib.ptr(perm),
                                                   _lib.ptr(start), _lib.ptr(dlat), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert len(tr.kernels) == 1 and tr.has("k_dlat_reduce @"), tr.kernels
    got = dlat.cpu().numpy()
    assert np.array_equal(got, want)
    # a node gets a contribution iff it is a corner of a cell that holds a point
    idx = np.stack(np.unravel_index(cell.cpu().numpy(), (B,) + shape), 1)
    touched = np.zeros((B,) + shape, bool)
    for c in range(8):
        off = [M.corner_bit(c, 3, k) for k in range(3)]
        touched[idx[:, 0], idx[:, 1] + off[0], idx[:, 2] + off[1], idx[:, 3] + off[2]] = True
    assert not touched.all()
    assert np.array_equal(got[~touched.reshape(-1)], init[~touched.reshape(-1)])
