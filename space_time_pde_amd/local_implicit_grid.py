"""Local implicit grid query (mirrors src/local_implicit_grid.py:10-61 of the reference).

``query_local_implicit_grid(model, latent_grid, query_pts, xmin, xmax)`` keeps the reference signature.  When it
is called from inside ``PDELayer.__call__`` (which announces the derivatives its equations need through
``jet_context``) with an ``ImNet`` decoder on CUDA tensors and 3-d query points, the whole
gather -> MLP -> corner-weighted sum, INCLUDING the coordinate derivatives, runs in the HIP jet kernels
(lig_jet.py).  A plain call (no PDE layer) on the same kind of inputs runs the value-only HIP path.
Value-only queries on 1-, 2- and 4-d grids (no jet request, nothing that needs a gradient) run in HIP as well: a gather and
a corner sum of their own around the same IM-NET layer kernels (``_nd_value_eligible``).  With ``lig_jet.nd_backward``
(opt-in) such a query also trains in HIP: gradients w.r.t. the latent grid and the IM-NET parameters (``_nd_train_eligible``).
With ``lig_jet.nd_jets`` (opt-in) a PDE layer's derivative request on a 1- or 2-d grid that needs no gradient is answered by
the HIP jet kernels too (``_nd_jet_eligible``), and with ``lig_jet.nd4_jets`` (opt-in, a switch of its own) so is one on a 4-d
grid -- 3-d space + time --, as passes over axis triples; with ``lig_jet.nd_jet_backward`` on top (opt-in) so is one that trains
through the residuals: gradients w.r.t. the latent grid and the IM-NET parameters (``_nd_jet_train_eligible``).
Other decoders / dimensions / requests use the generic composed formulation.
"""
import threading

import torch

from . import lig_jet
from . import regular_nd_grid_interpolation as rgi
from .implicit_net import ImNet

_tls = threading.local()
stats = {"hip_jet_calls": 0, "hip_value_calls": 0, "generic_calls": 0,
         # slower-strategy counters of pde.py (each also warns once): sympy analysis failures and residuals evaluated with
         # the lambdified torch functions instead of the HIP residual program
         "combo_plan_errors": 0, "jet_compile_errors": 0, "residual_torch_fallbacks": 0}


class JetRequest:
    """Set by PDELayer around ``forward_method``: which derivatives of y w.r.t. the points it will need."""

    def __init__(self, x, first, pairs, combo=None):
        self.x, self.first, self.pairs = x, first, list(pairs)
        self.combo = combo     # {pair: alpha}: the equations use second derivatives only through this combination
        self.y = None          # the tensor handed back to the caller
        self.jets = None       # [S, n_out, P]
        self.pairs_out = None  # second-order pairs in stream order (after padding)


class jet_context:
    def __init__(self, req):
        self.req = req

    def __enter__(self):
        self.prev = getattr(_tls, "req", None)
        _tls.req = self.req
        return self.req

    def __exit__(self, *exc):
        _tls.req = self.prev
        return False


def _fast_eligible(model, latent_grid, query_pts):
    return (isinstance(model, ImNet) and model.dim == 3 and latent_grid.dim() == 5 and query_pts.dim() == 3
            and query_pts.shape[-1] == 3 and latent_grid.is_cuda and query_pts.is_cuda
            and latent_grid.dtype == torch.float32 and query_pts.dtype == torch.float32
            and model.nf % 16 == 0 and model.out_features <= 16 and model.in_features <= lig_jet.MAX_LATENT_CHANNELS
            and latent_grid.shape[-1] == model.in_features
            and lig_jet.activation_name(model.activ) is not None)


def _nd_value_eligible(model, latent_grid, query_pts, req=None):
    """A value-only query on a 1-, 2- or 4-d grid that the HIP path serves: ImNet decoder, CUDA fp32, nf a multiple of 16,
    out_features <= 16, the augmented input [r(d); latent(c); 1] within the 36 slots of the layer kernels' input image
    (c <= 34 / 33 / 31 for d = 1 / 2 / 4 -- the reference's own 4-d test case, c = 32, is one channel too wide and stays on
    the composed formulation), every grid axis >= 2 nodes, fp32 or fp32x3 operands, no jet request for these points and
    nothing that needs a gradient (no_grad, or no input / parameter requiring grad).  Jets and point gradients on such grids
    keep the composed formulation; so does the training backward unless ``lig_jet.nd_backward`` is switched on
    (``_nd_train_eligible``)."""
    if not isinstance(model, ImNet) or model.dim not in lig_jet.ND_VALUE_DIMS:
        return False
    d = model.dim
    if not (latent_grid.dim() == d + 2 and query_pts.dim() == 3 and query_pts.shape[-1] == d
            and latent_grid.is_cuda and query_pts.is_cuda
            and latent_grid.dtype == torch.float32 and query_pts.dtype == torch.float32
            and model.nf % 16 == 0 and model.out_features <= 16
            and d + model.in_features + 1 <= lig_jet.MAX_AUG_FEATURES
            and latent_grid.shape[-1] == model.in_features and latent_grid.shape[0] == query_pts.shape[0]
            and min(latent_grid.shape[1:-1]) >= 2
            and lig_jet.mlp_precision in ("fp32", "fp32x3")
            and lig_jet.activation_name(model.activ) is not None):
        return False
    if req is not None and req.x is query_pts:
        return False
    if torch.is_grad_enabled() and (query_pts.requires_grad or latent_grid.requires_grad
                                    or any(p.requires_grad for p in model.parameters())):
        return False
    return True


def _nd_train_eligible(model, latent_grid, query_pts, req=None):
    """A value query on a 1-, 2- or 4-d grid whose TRAINING BACKWARD the HIP path serves (opt-in: ``lig_jet.nd_backward``,
    ``lig_jet.set_nd_backward`` / STPDE_ND_BACKWARD=1; off, this is always False and such a query is composed, as before):
    grad mode on and the latent grid and / or an IM-NET parameter (a learnable swish beta included) requires grad; everything
    ``_nd_value_eligible`` asks for other than its gradient clause (ImNet decoder itself -- not an nn.DataParallel over
    several devices --, CUDA fp32, nf a multiple of 16, out_features <= 16, d + in_features + 1 <= 36, every axis >= 2 nodes,
    fp32 or fp32x3 operands -- not bf16 --, no jet request for these points); in_features <= 32 (the latent-adjoint kernel
    k_xbar<XL> exists for XL = 1, 2, so d = 1 with c = 33, 34 and d = 2 with c = 33 stay composed whenever a gradient is
    needed); and the points themselves carry no gradient.  d latent is the deterministic per-node sum on these grids, whatever
    ``lig_jet.deterministic_dlatent`` says."""
    if not lig_jet.nd_backward or not torch.is_grad_enabled() or query_pts.requires_grad:
        return False
    with torch.no_grad():                   # = _nd_value_eligible without its gradient clause
        if not _nd_value_eligible(model, latent_grid, query_pts, req):
            return False
    if model.in_features > lig_jet.ND_TRAIN_MAX_CHANNELS:
        return False
    return bool(latent_grid.requires_grad or any(p.requires_grad for p in model.parameters()))


def _nd_jet_eligible(model, latent_grid, query_pts, req=None):
    """A query on a 1- or 2-d grid whose COORDINATE DERIVATIVES the HIP path serves (opt-in: ``lig_jet.nd_jets``,
    ``lig_jet.set_nd_jets`` / STPDE_ND_JETS=1; off, this is always False and such a request is composed, as before): an active
    jet request for exactly these points, without a combined second-order stream and with pair indices < d; everything
    ``_nd_value_eligible`` asks for other than its request clause (ImNet decoder, CUDA fp32, nf a multiple of 16, out_features
    <= 16, d + in_features + 1 <= 36, every axis >= 2 nodes, fp32 or fp32x3 operands); and nothing that needs a gradient
    (no_grad, or no point / latent grid / parameter requiring grad; a request that does is ``_nd_jet_train_eligible``'s).
    Point gradients keep the composed formulation.

    d = 4 -- 3-d space + time -- has a switch of its own (opt-in: ``lig_jet.nd4_jets``, ``lig_jet.set_nd4_jets`` /
    STPDE_ND4_JETS=1; ``nd_jets`` alone leaves such a request composed): the same conditions with d = 4 (in_features <= 31,
    pair indices < 4, no combined stream, nothing that needs a gradient); the request runs as passes over axis triples
    (``lig_jet.nd4_passes``)."""
    if req is None or req.x is not query_pts or req.combo:
        return False
    if not isinstance(model, ImNet):
        return False
    if not ((lig_jet.nd_jets and model.dim in lig_jet.ND_JET_DIMS) or (lig_jet.nd4_jets and model.dim == 4)):
        return False
    if any(not (0 <= a < model.dim and 0 <= b < model.dim) for a, b in req.pairs):
        return False
    return _nd_value_eligible(model, latent_grid, query_pts, None)     # (its gradient clause included)


def _nd_jet_train_eligible(model, latent_grid, query_pts, req=None):
    """A derivative request on a 1- or 2-d grid whose TRAINING BACKWARD the HIP path serves (opt-in on top of
    ``lig_jet.nd_jets``: ``lig_jet.nd_jet_backward``, ``lig_jet.set_nd_jet_backward`` / STPDE_ND_JET_BACKWARD=1; off, this is
    always False and such a request is composed, as before; ``lig_jet.nd_backward`` plays no part): grad mode on; everything
    ``_nd_jet_eligible`` asks for other than its gradient clause (an active request for exactly these points, pairs with
    indices < d, no combined stream, ImNet decoder itself -- not an nn.DataParallel --, CUDA fp32, nf a multiple of 16,
    out_features <= 16, every axis >= 2 nodes, fp32 or fp32x3 operands -- not bf16); in_features <= 32 (the latent-adjoint
    kernel k_xbar<XL> exists for XL = 1, 2); and the points themselves carry no gradient.  d = 4, the combined stream, bf16,
    point gradients, wider latents and several devices keep the composed formulation."""
    if not (lig_jet.nd_jets and lig_jet.nd_jet_backward) or not torch.is_grad_enabled() or query_pts.requires_grad:
        return False
    if isinstance(model, torch.nn.DataParallel) or getattr(model, "in_features", 0) > lig_jet.ND_TRAIN_MAX_CHANNELS:
        return False
    if getattr(model, "dim", None) not in lig_jet.ND_JET_DIMS:      # (d = 4, ``nd4_jets``: forward passes only)
        return False
    if req is None or not (req.first or req.pairs):     # (a request for the value alone trains as a value query: ``nd_backward``)
        return False
    with torch.no_grad():                   # = _nd_jet_eligible without its gradient clause
        return _nd_jet_eligible(model, latent_grid, query_pts, req)


def _xmin_is_zero(xmin, xmax=None, shape3=None):
    """The HIP kernels reproduce the reference's cell index, which ignores xmin (quirk a-Q1), for xmin == 0 only; any
    other lower bound takes the generic formulation, which behaves like the reference on every device.  Tensor bounds
    are decided through the (cached, sync-free after the first call) box-constant evaluation."""
    if isinstance(xmin, (int, float)):
        return xmin == 0
    if torch.is_tensor(xmin):
        if torch.is_tensor(xmax) and shape3 is not None:
            try:
                lig_jet.cached_box_constants(shape3, xmin, xmax)
                return True
            except ValueError:
                return False
        return bool((xmin.detach() == 0).all())
    return all(float(v) == 0 for v in xmin)


def _query_data_parallel(dp, latent_grid, query_pts, xmin, xmax, req):
    """The reference's default multi-GPU mechanism (experiments/rb2d/train.py:352-355 wraps the decoder in nn.DataParallel):
    the rows of the decoder input are scattered over ``dp.device_ids``.  Here the QUERY POINTS are: every device gets a
    replica of the IM-NET (``torch.nn.parallel.replicate``: gradients flow back to the wrapped module, summed), a copy of the
    latent grid and its share of the points, and runs the HIP jet path on them; the jets are gathered on the first device.
    One process drives all devices, as nn.DataParallel does.  Costs that come with that mechanism, per CALL: the module is
    re-replicated, the full latent grid is copied to every device and the devices are driven one after another from this
    thread -- it exists so that a reference script with several ``device_ids`` keeps the HIP path instead of dropping to the
    composed formulation, not for speed.  ``train_step.sharded_step`` (one process per GPU, collectives over RCCL) is the
    supported multi-GPU route.  Hardware coverage: on the 1-GPU test box both "devices" are ``cuda:0``
    (tests/test_gpu_lig_jet.py); with two real devices the path has not been run by the builder."""
    devs = list(dp.device_ids)
    B, N = query_pts.shape[0], query_pts.shape[1]
    chunks = [c for c in torch.chunk(query_pts, len(devs), dim=1) if c.shape[1] > 0]
    devs = devs[:len(chunks)]
    replicas = torch.nn.parallel.replicate(dp.module, devs, detach=not torch.is_grad_enabled())
    want_jets = req is not None and req.x is query_pts
    outs, pairs = [], None
    for rep, dev, pts_c in zip(replicas, devs, chunks):
        d = torch.device("cuda", dev)
        with torch.cuda.device(d):
            lat_d, pts_d = latent_grid.to(d), pts_c.to(d).contiguous()
            if want_jets:
                jets, pairs = lig_jet.lig_jets(rep, lat_d, pts_d, xmin, xmax, req.first, req.pairs, combo=req.combo)
            else:
                jets, _ = lig_jet.lig_jets(rep, lat_d, pts_d, xmin, xmax, False, ())
        # [S, n_out, B * n_d] (batch-major) -> [S, n_out, B, n_d] on the output device
        outs.append(jets.reshape(jets.shape[0], jets.shape[1], B, pts_c.shape[1]).to(query_pts.device))
    jets = torch.cat(outs, dim=3).reshape(outs[0].shape[0], outs[0].shape[1], B * N)
    stats["data_parallel_calls"] = stats.get("data_parallel_calls", 0) + 1
    y = jets[0].t().reshape(B, N, jets.shape[1])
    if want_jets:
        stats["hip_jet_calls"] += 1
        req.y, req.jets, req.pairs_out = y, jets, pairs
    else:
        stats["hip_value_calls"] += 1
    return y


def query_local_implicit_grid(model, latent_grid, query_pts, xmin, xmax):
    """Query a local implicit grid: y = sum_j w_j * model([x_rel_j ; latent_j]) (reference :47-59).

    model: nn.Module taking [rows, d+c]; latent_grid [b, n1..nd, c]; query_pts [b, num_pts, d];
    xmin/xmax: float, sequence or tensor bounds of the grid.  Returns [b, num_pts, o].
    """
    req = getattr(_tls, "req", None)
    # the reference wraps its networks in nn.DataParallel (experiments/rb2d/train.py:352-355); on one device that
    # wrapper is the identity, so the HIP path reads the wrapped module's parameters directly
    if isinstance(model, torch.nn.DataParallel) and len(model.device_ids or []) <= 1:
        model = model.module
    if isinstance(model, torch.nn.DataParallel) and _fast_eligible(model.module, latent_grid, query_pts) \
            and _xmin_is_zero(xmin, xmax, tuple(latent_grid.shape[1:4])) \
            and ((req is not None and req.x is query_pts) or not (query_pts.requires_grad and torch.is_grad_enabled())):
        return _query_data_parallel(model, latent_grid, query_pts, xmin, xmax, req)
    if _fast_eligible(model, latent_grid, query_pts) and _xmin_is_zero(xmin, xmax, tuple(latent_grid.shape[1:4])):
        wants_point_grad = query_pts.requires_grad and torch.is_grad_enabled()
        if req is not None and req.x is query_pts:
            jets, pairs = lig_jet.lig_jets(model, latent_grid, query_pts, xmin, xmax, req.first, req.pairs,
                                           combo=req.combo)
            stats["hip_jet_calls"] += 1
            y = jets[0].t().reshape(query_pts.shape[0], query_pts.shape[1], jets.shape[1])
            req.y, req.jets, req.pairs_out = y, jets, pairs
            return y
        if not wants_point_grad:
            jets, _ = lig_jet.lig_jets(model, latent_grid, query_pts, xmin, xmax, False, ())
            stats["hip_value_calls"] += 1
            return jets[0].t().reshape(query_pts.shape[0], query_pts.shape[1], jets.shape[1])
    if (_nd_jet_eligible(model, latent_grid, query_pts, req) or _nd_jet_train_eligible(model, latent_grid, query_pts, req)) \
            and _xmin_is_zero(xmin, xmax, tuple(latent_grid.shape[1:-1])):
        jets, pairs = lig_jet.lig_jets(model, latent_grid, query_pts, xmin, xmax, req.first, req.pairs)
        stats["hip_jet_calls"] += 1
        y = jets[0].t().reshape(query_pts.shape[0], query_pts.shape[1], jets.shape[1])
        req.y, req.jets, req.pairs_out = y, jets, pairs
        return y
    if (_nd_value_eligible(model, latent_grid, query_pts, req) or _nd_train_eligible(model, latent_grid, query_pts, req)) \
            and _xmin_is_zero(xmin, xmax, tuple(latent_grid.shape[1:-1])):
        jets, _ = lig_jet.lig_jets(model, latent_grid, query_pts, xmin, xmax, False, ())
        stats["hip_value_calls"] += 1
        return jets[0].t().reshape(query_pts.shape[0], query_pts.shape[1], jets.shape[1])
    stats["generic_calls"] += 1
    corner_values, weights, x_relative = rgi._coefficients_autograd(latent_grid, query_pts, xmin, xmax) \
        if (query_pts.requires_grad and torch.is_grad_enabled()) else \
        rgi.regular_nd_grid_interpolation_coefficients(latent_grid, query_pts, xmin, xmax)
    feats = torch.cat([x_relative, corner_values], dim=-1)
    shp = feats.shape
    out = model(feats.reshape(-1, shp[-1])).reshape(shp[0], shp[1], shp[2], -1)
    return torch.sum(out * weights.unsqueeze(-1), dim=-2)
