"""Dense-lattice inference: the query loop of experiments/rb2d/evaluation.py:26-74.

``evaluate_feat_grid`` keeps the reference signature and result layout.  Each pseudo-batch is one forward pass of the
HIP jet kernels (value + the residual derivatives, no autograd graph, no stash kept), so the pseudo-batch can be
millions of points instead of the reference's 10^4 (its higher-order autograd graph is O(points) memory).
"""
from collections import defaultdict

import numpy as np
import torch


def evaluate_feat_grid(pde_layer, latent_grid, t_seq, z_seq, x_seq, mins=None, maxs=None, pseudo_batch_size=1 << 20,
                       phys_channels=("p", "b", "u", "w")):
    """Evaluate the (already updated) pde_layer forward method on the lattice t_seq x z_seq x x_seq.

    Returns {channel or equation name: ndarray [len(t_seq), len(z_seq), len(x_seq)]} for batch element 0, exactly like
    the reference.  ``mins`` / ``maxs`` are accepted for signature compatibility (the reference does not use them).
    """
    device = latent_grid.device
    nb = latent_grid.shape[0]
    coord = torch.stack(torch.meshgrid(t_seq, z_seq, x_seq, indexing="ij"), dim=-1).reshape(-1, 3).to(device)
    n_query = coord.shape[0]
    res = defaultdict(list)
    for sid in range(0, n_query, pseudo_batch_size):
        batch = coord[sid:sid + pseudo_batch_size][None].expand(nb, -1, 3).contiguous()
        # HIP jet path: derivatives come from forward-mode streams, no autograd graph (and no stash) is needed.
        # Generic strategy (other forward methods / CPU): the reference's dif() sweeps need grad mode.
        jet = getattr(pde_layer, "_jet_request", lambda x: None)(batch) is not None
        with (torch.no_grad() if jet else torch.enable_grad()):
            pred, residues = pde_layer(batch, return_residue=True)
            pred = pred.detach().cpu().numpy()
        for cid, name in enumerate(phys_channels):
            res[name].append(pred[..., cid])
        for name, val in residues.items():
            res[name].append(val.detach().cpu().numpy()[..., 0])
    shape = [nb, len(t_seq), len(z_seq), len(x_seq)]
    return {k: np.concatenate(v, axis=1).reshape(shape)[0] for k, v in res.items()}


def evaluate_lattice(pde_layer, latent_grid, seqs, channels, pseudo_batch_size=1 << 20):
    """``evaluate_feat_grid`` for a problem of any dimension: evaluate the (already updated) pde_layer forward method on the
    lattice seqs[0] x ... x seqs[d - 1], one 1-D tensor per input variable of the layer, in its ``in_vars`` order.

    Returns {name in ``channels`` (the outputs, in order) or equation name: ndarray [len(seqs[0]), ..., len(seqs[d - 1])]} for
    batch element 0.  Grad mode as in ``evaluate_feat_grid``: off where the layer answers with forward-mode jets (for 1- and
    2-d problems that is the opt-in ``lig_jet.nd_jets``, for 4-d ones ``lig_jet.nd4_jets``; whether it does is asked with grad mode off, the mode those jets
    need), on for the reverse sweeps of the generic strategy.
    """
    device = latent_grid.device
    nb, d = latent_grid.shape[0], len(seqs)
    coord = torch.stack(torch.meshgrid(*seqs, indexing="ij"), dim=-1).reshape(-1, d).to(device)
    n_query = coord.shape[0]
    res = defaultdict(list)
    for sid in range(0, n_query, pseudo_batch_size):
        batch = coord[sid:sid + pseudo_batch_size][None].expand(nb, -1, d).contiguous()
        with torch.no_grad():
            jet = getattr(pde_layer, "_jet_request", lambda x: None)(batch) is not None
        with (torch.no_grad() if jet else torch.enable_grad()):
            pred, residues = pde_layer(batch, return_residue=True)
            pred = pred.detach().cpu().numpy()
        for cid, name in enumerate(channels):
            res[name].append(pred[..., cid])
        for name, val in residues.items():
            res[name].append(val.detach().cpu().numpy()[..., 0])
    shape = [nb] + [len(s) for s in seqs]
    return {k: np.concatenate(v, axis=1).reshape(shape)[0] for k, v in res.items()}
