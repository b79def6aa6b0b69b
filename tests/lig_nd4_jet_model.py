"""Numpy model of the two kernels that put coordinate derivatives on 4-d local implicit grids -- 3-d space + time -- (host-logic
tests and the reference of the GPU tests): ``coef_nd4`` restates k_coef_nd4, ``reduce_nd4_jet`` restates k_reduce_nd4_jet of
csrc/lig_gather_reduce.hip thread by thread -- the same integer arithmetic for every address, the same terms in the same
order -- and both record every element index they touch, so a CPU test can show that no input forms an address outside a
buffer before the kernels ever run.  ``assemble`` runs the reduction over a whole pass schedule (lig_jet.nd4_passes) into one
jets tensor, as the driver does.  The geometry is tests/lig_nd_model.py's (= csrc/interp_geom.h); the fc5-row layout is
tests/lig_nd_jet_model.py's ``out_pre_from_streams`` with D = 4 (one point = one 16-row tile).
"""
import numpy as np

from tests import lig_nd_model as M
from tests.lig_nd_jet_model import _sel, out_pre_from_streams  # noqa: F401  (re-exported: the D = 4 layout is the generic one)

F32 = np.float32
REC = 24        # floats of the coefficient record


def coef_nd4(pts, n, lo_c, hi_c, cube):
    """pts [P, 4] fp32 -> coef [P, 24] fp32 = {om[0][k], om[1][k], dom[0][k], dom[1][k], kap[k]} at 0 / 4 / 8 / 12 / 16 + k,
    entries 20 .. 23 = 0.  Also the index sets {"pts", "coef"}.  (The kernel computes the cell's node index as well, through
    point_cell<4>(), but forms no address from it: batch and p_base do not enter.)"""
    P = pts.shape[0]
    flat = pts.reshape(-1)
    coef = np.full(P * REC, np.nan, dtype=F32)
    touched = {"pts": set(), "coef": set()}
    nblocks = (P + 255) // 256
    for p in range(nblocks * 256):
        if p >= P:
            continue
        cf = [F32(0)] * REC
        for k in range(4):
            touched["pts"].add(p * 4 + k)
            _, om, _, dom, kap = M.geom_axis_jet(flat[p * 4 + k], lo_c[k], hi_c[k], cube[k], n[k])
            cf[k], cf[4 + k], cf[8 + k], cf[12 + k], cf[16 + k] = om[0], om[1], dom[0], dom[1], kap
        for i in range(REC):
            touched["coef"].add(p * REC + i)
            coef[p * REC + i] = cf[i]
    return coef.reshape(P, REC), touched


def reduce_nd4_jet(P, n_out, axis, pairs, S_mlp, S, dst, out_pre, coef, ldp=None, jets=None):
    """One pass.  axis: the triple; pairs: the npairs (0, 2, 4, 6) padded pairs of the pass IN AXES; dst = (value, (f0, f1, f2),
    (p0, ...)): destination streams or -1; out_pre: the fc5 rows [ntiles][S_mlp][256] (any shape, addressed flat), coef [P, 24]
    -> (jets [S, n_out, ldp] float64, bound, touched).  ``jets``: a (jets, bound) pair of an earlier pass to write into --
    streams the map does not name keep what they hold (NaN in a fresh tensor).

    The arithmetic is float64 on the given values; ``bound`` is what an fp32 evaluation of the same terms in any order may
    differ by at most: 4 * (number of terms) * 2^-24 * sum |terms| per element.  With d = 4 a term is a product of at most SEVEN
    fp32 factors (four weights, two kappas, the stream: six roundings, (1 + u)^6 - 1 < 6.01 u, u = 2^-24), and a sum of n terms
    in any order adds at most (n - 1) u (1 + ...) of the sum of their magnitudes: together < (n + 6) u sum |terms| <=
    4 n u sum |terms| for n >= 2 -- and the streams have n = 16 (value), 32 (first order) and 64 (pairs) terms.
    touched: {"out_pre", "coef", "jets"}."""
    ldp = P if ldp is None else ldp
    npairs = len(pairs)
    assert npairs in (0, 2, 4, 6) and S_mlp in (4, 4 + npairs)
    dst_value, dst_first, dst_pair = dst
    slot = {a: i for i, a in enumerate(axis)}
    flat = np.asarray(out_pre).reshape(-1)
    cflat = np.asarray(coef).reshape(-1)
    if jets is None:
        out, bnd = np.full(S * n_out * ldp, np.nan), np.full(S * n_out * ldp, np.nan)
    else:
        out, bnd = jets[0].reshape(-1), jets[1].reshape(-1)
    touched = {"out_pre": set(), "coef": set(), "jets": set()}
    nblocks = (P * n_out + 255) // 256
    for gid in range(nblocks * 256):
        if gid >= P * n_out:
            continue
        p, ch = gid // n_out, gid % n_out
        cf = []
        for i in range(REC):
            touched["coef"].add(p * REC + i)
            cf.append(float(cflat[p * REC + i]))
        ks = [cf[16 + a] if 0 <= a < 4 else cf[19] for a in axis]      # sel4: bounded for every axis value
        y, a_, nt = [0.0] * 10, [0.0] * 10, [0] * 10

        def acc(s, *terms):
            y[s] += sum(terms)
            a_[s] += sum(abs(t) for t in terms)
            nt[s] += len(terms)

        for corner in range(16):
            lane = ((ch >> 2) << 4) | corner
            base = p * S_mlp * 256 + lane * 4 + (ch & 3)
            f = [0.0] * 10
            for s in range(10):
                if s < S_mlp:
                    touched["out_pre"].add(base + s * 256)
                    f[s] = float(flat[base + s * 256])
            bit = [M.corner_bit(corner, 4, k) for k in range(4)]
            om = [cf[4 + k] if bit[k] else cf[k] for k in range(4)]
            dm = [cf[12 + k] if bit[k] else cf[8 + k] for k in range(4)]
            w = om[0] * om[1] * om[2] * om[3]
            dw = [float(np.prod([dm[k] if k == ax else om[k] for k in range(4)])) for ax in axis]
            acc(0, w * f[0])
            for i in range(3):
                acc(1 + i, dw[i] * f[0], w * ks[i] * f[1 + i])
            for k in range(npairs):
                ad, ae = pairs[k]
                d, e = slot[ad], slot[ae]
                kd, ke = _sel(d, ks), _sel(e, ks)
                dwd, dwe = _sel(d, dw), _sel(e, dw)
                fd, fe = _sel(d, f[1:4]), _sel(e, f[1:4])
                ddw = 0.0 if d == e else float(np.prod([dm[q] if q in (ad, ae) else om[q] for q in range(4)]))
                acc(4 + k, ddw * f[0], dwd * ke * fe, dwe * kd * fd, w * kd * ke * f[4 + k])
        stores = [(dst_value, 0)] + [(dst_first[i], 1 + i) for i in range(3)] + [(dst_pair[k], 4 + k) for k in range(npairs)]
        for t, s in stores:
            if t < 0:
                continue
            idx = (t * n_out + ch) * ldp + p
            touched["jets"].add(idx)
            out[idx] = y[s]
            bnd[idx] = 4 * nt[s] * 2.0 ** -24 * a_[s]
    shape = (S, n_out, ldp)
    return out.reshape(shape), bnd.reshape(shape), touched


def assemble(passes, P, n_out, S, coef, out_pre_of, ldp=None):
    """The whole schedule: passes as lig_jet.nd4_passes returns them, out_pre_of(k, triple, pairs) -> (out_pre, S_mlp) of pass
    k.  Returns (jets, bound, [touched per pass])."""
    jets, tr = None, []
    for k, (triple, pp, dst) in enumerate(passes):
        out_pre, S_mlp = out_pre_of(k, triple, pp)
        a, b, t = reduce_nd4_jet(P, n_out, triple, pp, S_mlp, S, dst, out_pre, coef, ldp, jets)
        jets = (a, b)
        tr.append(t)
    return jets[0], jets[1], tr
