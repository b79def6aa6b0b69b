"""Numpy model of the kernels the training backward adds around k_xbar, for local implicit grids of every dimension (host-logic
tests only).

``cell_nd`` and ``dlatent_reduce_nd`` restate the shared bodies of csrc/lig_gather_reduce.hip for D = 1..4 -- point_cell<D>
(k_cell_nd<D>, and the cell the gathers of every dimension read and the dim = 3 gathers write) and dlat_reduce<D>
(k_dlat_reduce_nd<D> for D = 1, 2, 4, k_dlat_reduce for D = 3) -- and ``reduce_nd_bwd`` restates k_reduce_nd_bwd, thread by
thread: the same integer arithmetic for every address, including the threads of the last block that the bounds test turns
away.  They record every element index they read or write, so a CPU test can show that no input forms an address outside a
buffer before a kernel ever runs.  ``cell_sort`` states what stpde_lig_cell_sort promises (stable order, start = points in
cells < c).  The geometry is tests/lig_nd_model.py's ``geom_axis``.
"""
import numpy as np

from tests.lig_nd_model import F32, corner_bit, geom_axis


def cell_nd(D, pts, n, B, N, p_base, lo_c, hi_c, cube):
    """pts [P, D] fp32, n = the D axis lengths -> cell [P] int32 and the index sets {"pts", "cell"}."""
    P = pts.shape[0]
    flat = pts.reshape(-1)
    cell = np.full(P, -1, dtype=np.int64)
    touched = {"pts": set(), "cell": set()}
    for p in range((P + 255) // 256 * 256):
        if p >= P:
            continue
        i0 = []
        for k in range(D):
            touched["pts"].add(p * D + k)
            i0.append(geom_axis(flat[p * D + k], lo_c[k], hi_c[k], cube[k], n[k])[0])
        node = min((p_base + p) // N, B - 1)
        for k in range(D):
            node = node * n[k] + i0[k]
        touched["cell"].add(p)
        cell[p] = node
    assert cell.max() < 2 ** 31
    return cell.astype(np.int32), touched


def reduce_nd_bwd(D, P, ntiles, n_out, ybar, cw):
    """ybar [n_out, ldp], cw [ntiles * 16] -> abar_out [ntiles, 64, 4] and the index sets {"ybar", "cw", "abar"}."""
    TP = 16 >> D
    ldp = ybar.shape[1]
    fy = ybar.reshape(-1)
    out = np.full(ntiles * 256, np.nan, dtype=ybar.dtype)
    touched = {"ybar": set(), "cw": set(), "abar": set()}
    for gid in range((ntiles * 64 + 255) // 256 * 256):
        if gid >= ntiles * 64:
            continue
        lane, tile = gid & 63, gid >> 6
        g, j = lane >> 4, lane & 15
        p = tile * TP + (j >> D)
        v = [ybar.dtype.type(0)] * 4
        if p < P and 4 * g < n_out:
            touched["cw"].add(tile * 16 + j)
            w = cw[tile * 16 + j]
            for r in range(4):
                if 4 * g + r < n_out:
                    touched["ybar"].add((4 * g + r) * ldp + p)
                    v[r] = w * fy[(4 * g + r) * ldp + p]
        for r in range(4):
            touched["abar"].add(gid * 4 + r)
            out[gid * 4 + r] = v[r]
    return out.reshape(ntiles, 64, 4), touched


def cell_sort(cell, n_nodes):
    """perm [P] = point indices in stable cell order, start [n_nodes + 1] = number of points in cells < c."""
    perm = np.argsort(cell, kind="stable").astype(np.int32)
    start = np.zeros(n_nodes + 1, dtype=np.int32)
    start[1:] = np.cumsum(np.bincount(cell, minlength=n_nodes))
    return perm, start


def dlatent_reduce_nd(D, B, n, C, xrows, perm, start, dlatent):
    """xrows [rows, CP] -> dlatent [B * prod(n), C] accumulated into (+=); returns the index sets
    {"xrows", "perm", "start", "dlatent"} (xrows / dlatent: flat element indices)."""
    NC = 1 << D
    CP = (C + 3) // 4 * 4
    assert xrows.shape[1] == CP
    nnodes = B * int(np.prod(n[:D]))
    fx, fd = xrows.reshape(-1), dlatent.reshape(-1)
    touched = {"xrows": set(), "perm": set(), "start": set(), "dlatent": set()}
    for gid in range((nnodes * 16 + 255) // 256 * 256):
        c4, node = gid & 15, gid >> 4
        if node >= nnodes or 4 * c4 >= CP:
            continue
        idx, stride = [0] * D, [0] * D
        rest, s = node, 1
        for k in range(D - 1, -1, -1):
            idx[k] = rest % n[k]
            rest //= n[k]
            stride[k] = s
            s *= n[k]
        acc = np.zeros(4, dtype=xrows.dtype)
        hit = False
        for corner in range(NC):
            inside, off = True, 0
            for k in range(D):
                bit = corner_bit(corner, D, k)
                c = idx[k] - bit
                inside = inside and 0 <= c <= n[k] - 2
                off += bit * stride[k]
            if not inside:
                continue
            cell = node - off
            touched["start"].update((cell, cell + 1))
            for q in range(start[cell], start[cell + 1]):
                touched["perm"].add(q)
                row = int(perm[q]) * NC + corner
                for r in range(4):
                    touched["xrows"].add(row * CP + 4 * c4 + r)
                acc = acc + fx[row * CP + 4 * c4:row * CP + 4 * c4 + 4]
                hit = True
        if not hit:
            continue
        for r in range(4):
            if 4 * c4 + r < C:
                touched["dlatent"].add(node * C + 4 * c4 + r)
                fd[node * C + 4 * c4 + r] += acc[r]
    return touched


# ---------------------------------------------------------------------------------------------------------------------
# the training cases shared by tests/test_lig_nd_backward_host.py (margin of the bounds) and
# tests/test_gpu_lig_nd_backward.py (parity): built once, shared, never modified
# ---------------------------------------------------------------------------------------------------------------------
# (d, grid, c): c = 31 fills the sparse third input tile for d = 4 (d + c + 1 = 36); c = 32 is the widest trainable latent
TRAIN_CASES = [(1, (5,), 8), (2, (4, 5), 8), (4, (3, 4, 2, 3), 8), (4, (3, 4, 2, 3), 31), (1, (9,), 32)]
TOL_Y, TOL_G = 2e-5, 2e-4         # of the tensor's max magnitude: the bounds of test_value_only_query_backward (dim = 3)
_cases = {}


def train_case(d, grid, c, act, n=37, nf=16):
    """dict(net (CPU fp32 ImNet), lat [2, *grid, c], pts [2, n, d], box, cot [2, n, 3]): 24 random points plus the edge set of
    tests/lig_nd_model.py per batch item; for grid (9,) confined to the first half of the box (some nodes get no point)."""
    import torch
    from space_time_pde_amd import implicit_net, nonlinearities
    from tests.lig_nd_model import edge_points
    key = (d, grid, c, act, n, nf)
    if key not in _cases:
        acts = {"leakyrelu": torch.nn.LeakyReLU, "softplus": torch.nn.Softplus, "swish": nonlinearities.Swish}
        torch.manual_seed(17 + d)
        net = implicit_net.ImNet(dim=d, in_features=c, out_features=3, nf=nf, activation=acts[act])
        g = torch.Generator().manual_seed(13 * d + c)
        lat = 0.5 * torch.randn(2, *grid, c, generator=g)
        e0, e1 = (torch.from_numpy(edge_points(grid, 1.0, seed=s)) for s in (0, 1))
        pts = torch.stack([e0, e1.flip(0)], 0)[:, :n].contiguous()
        if grid == (9,):
            pts = torch.where(pts > 0.5, 0.5 * pts, pts).clamp(max=0.5)
        cot = torch.randn(2, n, 3, generator=g)
        if (d, c, act) == (4, 31, "leakyrelu") and n > 22:
            # random point 22 puts a pre-activation of this decoder within fp32 rounding of LeakyReLU's kink:
            # the fp32 and the fp64 oracle then take different slopes there and their parameter gradients differ by 2.4e-3 of
            # the maximum -- a property of the point, not of any implementation.  The point is replaced (drawn after
            # everything else, so no other value of the case moves); the bounds stay.
            pts[:, 22] = torch.rand(2, d, generator=g)
        _cases[key] = dict(d=d, act=act, net=net, lat=lat, pts=pts, box=(0., 1.), cot=cot)
    return _cases[key]


def oracle_grads(case, dtype):
    """y, d latent, the 12 parameter gradients (w0, b0, ..., w5, b5) and d beta (swish; else None) of oracle.cpu_ref's
    query_lig + imnet_forward in ``dtype`` on the case's fp32 values, for the loss sum(y * cot).  Cached per dtype."""
    import torch
    from oracle import cpu_ref as O
    if ("ref", dtype) not in case:
        net = case["net"]
        prm = [(net.fc[k].weight.detach().to(dtype).requires_grad_(True), net.fc[k].bias.detach().to(dtype).requires_grad_(True))
               for k in range(6)]
        beta = net.activ.beta.detach().to(dtype).requires_grad_(True) if case["act"] == "swish" else None
        lat = case["lat"].detach().clone().to(dtype).requires_grad_(True)
        y = O.query_lig(lambda f: O.imnet_forward(prm, f, O.activation_fn(case["act"], beta)), lat, case["pts"].to(dtype),
                        *case["box"])
        (y * case["cot"].to(dtype)).sum().backward()
        case[("ref", dtype)] = (y.detach(), lat.grad, [t.grad for wb in prm for t in wb], None if beta is None else beta.grad)
    return case[("ref", dtype)]


def relerr(a, b):
    return (a.double().cpu() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)
