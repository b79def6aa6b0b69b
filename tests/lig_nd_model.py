"""Numpy model of the gather side of the HIP path for local implicit grids of every dimension (host-logic tests only).

``gather_nd`` restates the shared gather body of csrc/lig_gather_reduce.hip (gather_rows<D>, D = 1..4: k_gather_nd<D> for
D = 1, 2, 4 and k_gather / k_gather_tile for D = 3) thread by thread -- the same integer arithmetic for every address, the
same fp32 expression sequence for the geometry -- and records every element index it reads or writes, so a CPU test can show
that no input forms an address outside a buffer before the kernel ever runs.  ``coef_epilogue`` restates what the dim = 3
gathers add per point (write_coef: coef, cell, cw), ``gather3`` is the whole of stpde_lig_gather.  ``reduce_nd`` restates
k_reduce_nd, ``mlp_rows`` the layer kernels' one-stream pass over the operand packs (tests/mfma_emu.py).
"""
import numpy as np

from tests import mfma_emu as E

XT = 3
F32 = np.float32
# the dim = 3 cases (dim, grid, c, xmax) shared by the host tests and tests/test_gpu_lig_glue.py: c = 8 reaches k_gather,
# c = 32 k_gather_tile
D3_GRIDS = [(3, (3, 4, 5), 8, (2.0, 1.0, 0.5)), (3, (4, 3, 3), 32, 1.0)]


def corner_bit(j, dim, k):
    return (j >> (dim - 1 - k)) & 1


def geom_axis(x, lo, hi, cs, n):
    """csrc/interp_geom.h geom_axis in fp32; fminf / fmaxf return the other operand for a NaN, as np.fmin / np.fmax do."""
    x, lo, hi, cs = F32(x), F32(lo), F32(hi), F32(cs)
    q = np.fmax(np.fmin(x, hi), lo)
    i0 = int(np.floor(q / cs))
    i0 = 0 if i0 < 0 else (n - 2 if i0 > n - 2 else i0)
    i0f = F32(i0)
    p0, p1 = i0f * cs, (i0f + F32(1)) * cs
    om = (np.abs(q - p1) / cs, np.abs(q - p0) / cs)
    rl = ((q - p0) / cs, (q - p1) / cs)
    return i0, om, rl


def geom_axis_jet(x, lo, hi, cs, n):
    """csrc/interp_geom.h geom_axis_jet in fp32: geom_axis plus the derivative s of the clip (min / max backward split ties
    evenly), kap = s / cs and dom = sign(q - opposite) / cs * s."""
    x, lo, hi, cs = F32(x), F32(lo), F32(hi), F32(cs)
    i0, om, rl = geom_axis(x, lo, hi, cs, n)
    m = np.fmin(x, hi)
    q = np.fmax(m, lo)
    s = F32(1 if x < hi else (0.5 if x == hi else 0)) * F32(1 if m > lo else (0.5 if m == lo else 0))
    i0f = F32(i0)
    t = (q - (i0f + F32(1)) * cs, q - i0f * cs)          # q - opposite position of bit 0 / bit 1
    dom = tuple(F32(1 if tb > 0 else (-1 if tb < 0 else 0)) / cs * s for tb in t)
    return i0, om, rl, dom, s / cs


def coef_epilogue(pts, n, B, N, p_base, lo_c, hi_c, cube, alpha=None):
    """What one lane per point of the dim = 3 gathers writes: pts [P, 3] fp32 -> coef [P, 16] = {om[b][d] (6), dom[b][d] (6),
    kap[d] (3), 0}, cell [P] = node of corner 0 (batch clamped) and, with ``alpha`` (6 weights), cw [P, 8] =
    alpha_k * kap_a * kap_b over the canonical pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), then two zeros; cw is None without."""
    P = pts.shape[0]
    coef = np.full((P, 16), np.nan, dtype=F32)
    cell = np.full(P, -1, dtype=np.int64)
    cw = None if alpha is None else np.full((P, 8), np.nan, dtype=F32)
    for p in range(P):
        g = [geom_axis_jet(pts[p, d], lo_c[d], hi_c[d], cube[d], n[d]) for d in range(3)]
        for d in range(3):
            coef[p, d], coef[p, 3 + d] = g[d][1]
            coef[p, 6 + d], coef[p, 9 + d] = g[d][3]
            coef[p, 12 + d] = g[d][4]
        coef[p, 15] = 0
        node = min((p_base + p) // N, B - 1)
        for d in range(3):
            node = node * n[d] + g[d][0]
        cell[p] = node
        if cw is not None:
            k = [g[d][4] for d in range(3)]
            for i, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                cw[p, i] = F32(F32(alpha[i]) * k[a]) * k[b]
            cw[p, 6:] = 0
    assert cell.max() < 2 ** 31
    return coef, cell.astype(np.int32), cw


def gather3(pts, latent, N, p_base, lo_c, hi_c, cube, alpha=None):
    """stpde_lig_gather: pts [P, 3] (P even), latent [B, n0, n1, n2, C] -> X [P / 2, 3, 64, 4], coef, cell, cw (None without
    ``alpha``) and the index sets of gather_nd; every element of coef, cell and cw is written exactly once (one lane per
    point, p < P)."""
    P = pts.shape[0]
    assert P % 2 == 0
    X, _, touched = gather_nd(3, pts, latent, N, p_base, lo_c, hi_c, cube, P // 2)
    coef, cell, cw = coef_epilogue(pts, latent.shape[1:4], latent.shape[0], N, p_base, lo_c, hi_c, cube, alpha)
    return X, coef, cell, cw, touched


def row_major_image(X):
    """The optional XR output of stpde_lig_gather from X [ntiles, 3, 64, 4]: lane 16 g + c of a tile holds rows 4g .. 4g + 3
    of slot c, where X's lane 16 g + j holds slots 4g .. 4g + 3 of row j."""
    nt = X.shape[0]
    rows = X.reshape(nt, XT, 4, 16, 4).transpose(0, 1, 3, 2, 4).reshape(nt, XT, 16, 16)          # [row j][slot 4g + r]
    return np.ascontiguousarray(rows.reshape(nt, XT, 4, 4, 16).transpose(0, 1, 2, 4, 3)).reshape(nt, XT, 64, 4)


def gather_nd(D, pts, latent, N, p_base, lo_c, hi_c, cube, ntiles):
    """pts [P, D] fp32, latent [B, n_1..n_D, C] fp32 -> X [ntiles, 3, 64, 4], cw [ntiles * 16] (the weight of every row: the
    roww output of k_gather_nd; the dim = 3 kernels do not store it) and the index sets {"pts", "latent", "X", "cw"} of flat
    element indices touched."""
    TP, NC = 16 >> D, 1 << D
    P, B, C = pts.shape[0], latent.shape[0], latent.shape[-1]
    n = latent.shape[1:-1]
    flat_pts, flat_lat = pts.reshape(-1), latent.reshape(-1)
    X = np.full(ntiles * XT * 64 * 4, np.nan, dtype=F32)
    cw = np.full(ntiles * 16, np.nan, dtype=F32)
    touched = {"pts": set(), "latent": set(), "X": set(), "cw": set()}
    nthreads = ntiles * XT * 64
    nblocks = (nthreads + 255) // 256
    for gid in range(nblocks * 256):
        if gid >= ntiles * XT * 64:
            continue
        lane, xt, tile = gid & 63, (gid >> 6) % XT, (gid >> 6) // XT
        g, j = lane >> 4, lane & 15
        p = tile * TP + (j >> D)
        corner = j & (NC - 1)
        v = [F32(0)] * 4
        w = F32(0)
        if p < P:
            geo = []
            for k in range(D):
                touched["pts"].add(p * D + k)
                geo.append(geom_axis(flat_pts[p * D + k], lo_c[k], hi_c[k], cube[k], n[k]))
            b = min((p_base + p) // N, B - 1)
            node = b
            for k in range(D):
                bit = corner_bit(corner, D, k)
                node = node * n[k] + geo[k][0] + bit
                o = geo[k][1][bit]
                w = o if k == 0 else F32(w * o)
            for r in range(4):
                f = 16 * xt + 4 * g + r if xt < XT - 1 else (16 * xt + g if r == 0 else 16 * XT)
                if f < D:
                    v[r] = geo[f][2][corner_bit(corner, D, f)]
                elif f < D + C:
                    touched["latent"].add(node * C + f - D)
                    v[r] = flat_lat[node * C + f - D]
                elif f == D + C:
                    v[r] = F32(1)
        for r in range(4):
            touched["X"].add(gid * 4 + r)
            X[gid * 4 + r] = v[r]
        if xt == 0 and g == 0:
            touched["cw"].add(tile * 16 + j)
            cw[tile * 16 + j] = w
    return X.reshape(ntiles, XT, 64, 4), cw, touched


def reduce_nd(D, P, n_out, out_pre, cw):
    """out_pre [ntiles, 64, 4], cw [ntiles * 16] -> y [n_out, P] and the index sets {"out_pre", "cw"} read."""
    TP, NC = 16 >> D, 1 << D
    flat = out_pre.reshape(-1)
    y = np.zeros((n_out, P), dtype=out_pre.dtype)
    touched = {"out_pre": set(), "cw": set()}
    for gid in range(P * n_out):
        p, ch = gid // n_out, gid % n_out
        tile, j0 = p // TP, (p % TP) << D
        acc = out_pre.dtype.type(0)
        for corner in range(NC):
            j = j0 | corner
            lane = ((ch >> 2) << 4) | j
            touched["cw"].add(tile * 16 + j)
            touched["out_pre"].add(tile * 256 + lane * 4 + (ch & 3))
            acc = acc + cw[tile * 16 + j] * flat[tile * 256 + lane * 4 + (ch & 3)]
        y[ch, p] = acc
    return y, touched


def mlp_rows(plan, packs, X, act):
    """One-stream pass of the layer kernels over the row tiles of X (fp64): the fc5 rows [ntiles, 64, 4]."""
    out = np.zeros((X.shape[0], 64, 4))
    pv = lambda l, name, a, b: plan.pack_view(packs, l, name).reshape(a, b, 64, 4)
    for t in range(X.shape[0]):
        xb = X[t].astype(np.float64)
        mt0 = plan.layers[0]["MT"]
        pre = E.gemm_frag(pv(0, "Ws", XT, mt0), xb, XT, mt0)
        for l in range(1, 6):
            kt, mt = plan.layers[l]["KT"], plan.layers[l]["MT"]
            pre = E.gemm_frag(pv(l, "Wh", kt, mt), act(pre), kt, mt) + E.gemm_frag(pv(l, "Ws", XT, mt), xb, XT, mt)
        out[t] = pre[0]
    return out


def edge_points(grid_shape, xmax, seed=0):
    """The 37 query points of the dim = 1, 2, 4 tests, [37, d] fp32: 24 random ones in the box, the point at exactly 0, the one
    at exactly xmax, one outside the box on either side, and three grid nodes (interior ones where the axis has any) each
    exactly, one ulp below and one ulp above."""
    d = len(grid_shape)
    hi = np.asarray(xmax, dtype=F32) * np.ones(d, dtype=F32)
    rng = np.random.default_rng(seed)
    cube = hi / (np.asarray(grid_shape, dtype=F32) - F32(1))
    rows = [rng.random((24, d), dtype=F32) * hi, np.zeros((1, d), F32), hi[None], (-0.5 * hi)[None], (1.7 * hi)[None]]
    for t in range(3):
        idx = np.asarray([1 + t % max(n - 2, 1) for n in grid_shape], dtype=F32)
        node = idx * cube
        rows += [node[None], np.nextafter(node, F32(-np.inf))[None], np.nextafter(node, F32(np.inf))[None]]
    pts = np.concatenate(rows, 0).astype(F32)
    assert pts.shape == (37, d)
    return pts
