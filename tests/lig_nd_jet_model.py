"""Numpy model of the two kernels that put coordinate derivatives on 1- and 2-d local implicit grids (host-logic tests and the
reference of the GPU tests): ``coef_nd`` restates k_coef_nd<D>, ``reduce_nd_jet`` restates k_reduce_nd_jet<D> of
csrc/lig_gather_reduce.hip thread by thread -- the same integer arithmetic for every address, the same terms in the same
order -- and both record every element index they touch, so a CPU test can show that no input forms an address outside a
buffer before the kernels ever run.  ``out_pre_from_streams`` lays decoder streams out as the fc5 rows the layer kernels
write.  The geometry is tests/lig_nd_model.py's (= csrc/interp_geom.h).
"""
import numpy as np

from tests import lig_nd_model as M

F32 = np.float32


def coef_nd(D, pts, n, lo_c, hi_c, cube):
    """pts [P, D] fp32 -> coef [P, 16] fp32 = {om[0][k], om[1][k], dom[0][k], dom[1][k], kap[k]} at 0 / 3 / 6 / 9 / 12 + k,
    entry 15 = 0; om = 1, dom = 0, kap = 0 for the axes k >= D.  Also the index sets {"pts", "coef"}.  (The kernel computes the
    cell's node index as well, through point_cell<D>(), but forms no address from it: batch and p_base do not enter.)"""
    P = pts.shape[0]
    flat = pts.reshape(-1)
    coef = np.full(P * 16, np.nan, dtype=F32)
    touched = {"pts": set(), "coef": set()}
    nblocks = (P + 255) // 256
    for p in range(nblocks * 256):
        if p >= P:
            continue
        cf = [F32(0)] * 16
        for k in range(3):
            if k < D:
                touched["pts"].add(p * D + k)
                _, om, _, dom, kap = M.geom_axis_jet(flat[p * D + k], lo_c[k], hi_c[k], cube[k], n[k])
            else:
                om, dom, kap = (F32(1), F32(1)), (F32(0), F32(0)), F32(0)
            cf[k], cf[3 + k], cf[6 + k], cf[9 + k], cf[12 + k] = om[0], om[1], dom[0], dom[1], kap
        for i in range(16):
            touched["coef"].add(p * 16 + i)
            coef[p * 16 + i] = cf[i]
    return coef.reshape(P, 16), touched


def _sel(d, a):
    """sel3 of csrc/common.h: a[0] for d = 0, a[1] for d = 1, a[2] otherwise -- bounded for every d"""
    return a[0] if d == 0 else (a[1] if d == 1 else a[2])


def reduce_nd_jet(D, P, n_out, S1, S2, pairs, S_mlp, out_pre, coef, ldp=None):
    """out_pre: the fc5 rows [ntiles][S_mlp][256] (any shape, addressed flat), coef [P, 16] -> (jets [S, n_out, ldp] float64,
    bound [S, n_out, ldp], touched).  The arithmetic is float64 on the given values; ``bound`` is what an fp32 evaluation of
    the same terms in any order may differ by at most: 4 * (number of terms) * 2^-24 * sum |terms| per element (a term is a
    product of at most six fp32 factors, each product and each of the additions rounds once).  pairs: the S2 padded pairs of
    the configuration.  Streams of the axes >= D are written as 0 and are no terms.  touched: {"out_pre", "coef", "jets"}."""
    TP, NC = 16 >> D, 1 << D
    S = 1 + S1 + S2
    ldp = P if ldp is None else ldp
    flat = np.asarray(out_pre).reshape(-1)
    cflat = np.asarray(coef).reshape(-1)
    jets = np.full(S * n_out * ldp, np.nan)
    asum = np.zeros(S * n_out * ldp)
    nterm = np.zeros(S * n_out * ldp)
    touched = {"out_pre": set(), "coef": set(), "jets": set()}
    nblocks = (P * n_out + 255) // 256
    for gid in range(nblocks * 256):
        if gid >= P * n_out:
            continue
        p, ch = gid // n_out, gid % n_out
        cf = []
        for i in range(16):
            touched["coef"].add(p * 16 + i)
            cf.append(float(cflat[p * 16 + i]))
        kap = cf[12:15]
        y, a, nt = [0.0] * 10, [0.0] * 10, [0] * 10

        def acc(s, *terms):
            y[s] += sum(terms)
            a[s] += sum(abs(t) for t in terms)
            nt[s] += len(terms)

        tile, j0 = p // TP, (p % TP) << D
        for corner in range(NC):
            j = j0 | corner
            lane = ((ch >> 2) << 4) | j
            base = tile * S_mlp * 256 + lane * 4 + (ch & 3)
            f = [0.0] * 10
            for s in range(10):
                if s < S_mlp:
                    touched["out_pre"].add(base + s * 256)
                    f[s] = float(flat[base + s * 256])
            bit = [M.corner_bit(corner, D, k) if k < D else 0 for k in range(3)]
            om = [cf[3 + k] if bit[k] else cf[k] for k in range(3)]
            dm = [cf[9 + k] if bit[k] else cf[6 + k] for k in range(3)]
            w = om[0] * om[1] * om[2]
            dw = [dm[0] * om[1] * om[2], om[0] * dm[1] * om[2], om[0] * om[1] * dm[2]]
            ddw = {1: dm[0] * dm[1] * om[2], 2: dm[0] * om[1] * dm[2], 3: om[0] * dm[1] * dm[2]}
            acc(0, w * f[0])
            if S1 == 3:
                for d in range(D):
                    acc(1 + d, dw[d] * f[0], w * kap[d] * f[1 + d])
                for k in range(S2):
                    d, e = pairs[k]
                    kd, ke = _sel(d, kap), _sel(e, kap)
                    dwd, dwe = _sel(d, dw), _sel(e, dw)
                    fd, fe = _sel(d, f[1:4]), _sel(e, f[1:4])
                    acc(4 + k, (0.0 if d == e else ddw[min(max(d + e, 1), 3)]) * f[0], dwd * ke * fe, dwe * kd * fd,
                        w * kd * ke * f[4 + k])
        for s in range(S):
            idx = (s * n_out + ch) * ldp + p
            touched["jets"].add(idx)
            absent = 1 + D <= s < 4
            jets[idx] = 0.0 if absent else y[s]
            asum[idx] = 0.0 if absent else a[s]
            nterm[idx] = 0 if absent else nt[s]
    shape = (S, n_out, ldp)
    return jets.reshape(shape), (4 * nterm * 2.0 ** -24 * asum).reshape(shape), touched


def out_pre_from_streams(D, streams, ntiles, n_out, fill=np.nan):
    """Decoder streams per gather row -> the fc5 rows of the layer kernels, [ntiles, S_mlp, 64, 4] float64.  streams: list of
    S_mlp arrays [rows, n_out] (rows = points * 2^D in gather order: row tile * 16 + j) or None for a stream the test wants
    filled with ``fill`` (the tangent stream of an axis the grid does not have: loaded by the kernel, never used).  Lane (g, j)
    register r of a block holds output feature 4g + r of row j; features >= n_out and padding rows hold ``fill`` too."""
    out = np.full((ntiles, len(streams), 64, 4), fill, dtype=np.float64)
    for s, st in enumerate(streams):
        if st is None:
            continue
        for row in range(st.shape[0]):
            tile, j = row // 16, row % 16
            for ch in range(n_out):
                out[tile, s, ((ch >> 2) << 4) | j, ch & 3] = st[row, ch]
    return out
