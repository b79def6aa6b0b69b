"""Host driver of the fused LIG + IM-NET jet path (dim = 3; value queries, and opt-in their training backward, also for
dim = 1, 2, 4; opt-in jets, and opt-in their training backward, also for dim = 1, 2; opt-in jets of forward passes also for
dim = 4, as passes over axis triples) on libstpde_hip.

Computes y = query_local_implicit_grid(imnet, latent, pts) together with its first and selected second
derivatives w.r.t. the query coordinates ("jets") in one forward pass of HIP kernels, and the gradients w.r.t.
the IM-NET parameters and the latent grid in one backward pass.  This replaces, for the hot path,
  * src/local_implicit_grid.py:47-59 + src/regular_nd_grid_interpolation.py:48-76 (gather, weights, rel coords),
  * src/implicit_net.py:48-54 (6 addmm + activations + concats on the [b*p*8, 35] matrix),
  * the 23-25 ``torch.autograd.grad(create_graph=True)`` sweeps of src/pde.py:8-9 and their double backward.

Everything here is plumbing (buffer allocation, weight packing by index gather, launch order); all arithmetic on
query points runs in the HIP library.  There is no fallback: tensors must be CUDA/HIP float32.
"""
import ctypes as C
import dataclasses
import math
import os
import threading

import numpy as np
import torch

from . import _lib
from ._lib import (XT, GatherDesc, GatherNdDesc, ImNetPlanDesc, JetCfg, LayerDesc, LigWorkspace, Nd4PassDesc, XbarDesc, check, ptr,
                   stream_ptr)

_FRAG = 256  # floats per 16x16 fragment block
# widest latent the HIP jet path takes: the augmented input [r(3); latent(c); 1] must fit XT = 3 fragment tiles whose third
# one is sparse (4 live slots): 3 + c + 1 <= 36.  Wider latents run the generic composed formulation.
MAX_LATENT_CHANNELS = 16 * (XT - 1) + 4 - 3 - 1
# the same limit for the value-only path of dim = 1, 2, 4: dim + c + 1 <= MAX_AUG_FEATURES (c <= 34 / 33 / 31)
MAX_AUG_FEATURES = 16 * (XT - 1) + 4
ND_VALUE_DIMS = (1, 2, 4)
# widest latent the training backward on such grids takes: k_xbar<XL> (the latent adjoint) exists for XL = 1, 2
ND_TRAIN_MAX_CHANNELS = 32

# Opt-in: train through value queries on 1-, 2- and 4-d grids in HIP (gradients w.r.t. the latent grid and the IM-NET
# parameters; ``set_nd_backward`` / STPDE_ND_BACKWARD=1, read once here).  Off, a query on such a grid that needs a gradient
# takes the composed formulation (local_implicit_grid.py) and lig_jets refuses it.
nd_backward = os.getenv("STPDE_ND_BACKWARD", "0").strip().lower() not in ("", "0", "false", "no", "off")


def set_nd_backward(on):
    """Switch the HIP training backward of dim = 1, 2, 4 value queries on or off; returns the previous setting."""
    global nd_backward
    prev, nd_backward = nd_backward, bool(on)
    return prev


# Opt-in: coordinate derivatives (first and second-order pairs) of queries on 1- and 2-d grids in HIP, for forward passes that
# need no gradient (``set_nd_jets`` / STPDE_ND_JETS=1, read once here).  Off, lig_jets refuses a derivative request on such a
# grid and PDELayer runs its reverse sweeps through the composed formulation, as before.
ND_JET_DIMS = (1, 2)
nd_jets = os.getenv("STPDE_ND_JETS", "0").strip().lower() not in ("", "0", "false", "no", "off")


def set_nd_jets(on):
    """Switch the HIP coordinate derivatives of dim = 1, 2 queries on or off; returns the previous setting."""
    global nd_jets
    prev, nd_jets = nd_jets, bool(on)
    return prev


# Opt-in: train THROUGH those derivatives -- gradients of a loss on the jets of a 1- or 2-d query (a PDE residual loss) w.r.t.
# the latent grid and the IM-NET parameters in HIP (``set_nd_jet_backward`` / STPDE_ND_JET_BACKWARD=1, read once here).  Takes
# effect only together with ``nd_jets``; independent of ``nd_backward``, which governs value-only queries.  Off, lig_jets
# refuses a derivative request on such a grid that needs a gradient and PDELayer makes no request under grad mode, as before.
nd_jet_backward = os.getenv("STPDE_ND_JET_BACKWARD", "0").strip().lower() not in ("", "0", "false", "no", "off")


def set_nd_jet_backward(on):
    """Switch the HIP training backward of dim = 1, 2 coordinate derivatives on or off (it needs ``nd_jets`` as well); returns
    the previous setting."""
    global nd_jet_backward
    prev, nd_jet_backward = nd_jet_backward, bool(on)
    return prev


# Opt-in: coordinate derivatives of queries on 4-d grids -- 3-d space + time -- in HIP, for forward passes that need no gradient
# (``set_nd4_jets`` / STPDE_ND4_JETS=1, read once here; independent of ``nd_jets``, and ``ND_JET_DIMS`` stays what it is).  The
# layer kernels carry three first-order streams, so such a request runs as up to four PASSES over axis triples (``nd4_passes``).
# Off, lig_jets refuses a derivative request on a 4-d grid and PDELayer runs its reverse sweeps through the composed formulation.
nd4_jets = os.getenv("STPDE_ND4_JETS", "0").strip().lower() not in ("", "0", "false", "no", "off")


def set_nd4_jets(on):
    """Switch the HIP coordinate derivatives of dim = 4 queries on or off; returns the previous setting."""
    global nd4_jets
    prev, nd4_jets = nd4_jets, bool(on)
    return prev


# Optional per-kernel timing (bench.py): set ``profile`` to a dict; every library call then records a pair of
# events on the launch stream under its kernel name.  None = no overhead.
profile = None


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if profile is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if profile is not None:
            self.e1.record()
            profile.setdefault(self.name, []).append((self.e0, self.e1))
        return False


# ------------------------------------------------------------------------------------------------------------
# architecture plan: index maps between nn.Linear parameters and MFMA operand packs
# ------------------------------------------------------------------------------------------------------------
class ImNetPlan:
    """Static layout information for one IM-NET architecture (src/implicit_net.py:31-36)."""

    _cache = {}

    @classmethod
    def get(cls, dim, in_features, out_features, nf):
        key = (dim, in_features, out_features, nf)
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def __init__(self, dim, in_features, out_features, nf):
        # dim = 3: the jet path.  dim = 1, 2, 4: the packs serve the value path (lig_jets with first=False, pairs=()) and its
        # training backward -- the layer kernels index the augmented input by SLOT ("Ws", the latent columns "WsL" of the
        # d-latent GEMM and the unpack map of the weight gradients all go through the slot map), and in their one-stream
        # configuration nothing reads the "tanc" packs (columns 0..2 as coordinate tangents).  dim = 1, 2 (``nd_jets``): the
        # derivative streams run on the same kernels, "tanc" holds zeros for the columns that are no coordinate
        if dim != 3 and dim not in ND_VALUE_DIMS:
            raise ValueError("the HIP path is built for dim=3 query points (value-only queries: dim 1, 2, 4)")
        if nf % 16 != 0:
            raise ValueError("the HIP jet path needs nf to be a multiple of 16 (hidden widths are MFMA tiles)")
        self.dz = dim + in_features
        if self.dz + 1 > MAX_AUG_FEATURES:
            raise ValueError("in_features too large for the augmented input of the HIP path (dim + in_features + 1 <= %d: "
                             "max 32 latent channels for dim=3)" % MAX_AUG_FEATURES)
        if out_features > 16:
            raise ValueError("out_features > 16 not supported by the HIP jet path")
        self.dim, self.cin, self.cout, self.nf = dim, in_features, out_features, nf
        self.xl = (in_features + 15) // 16      # 16-channel tiles of the latent adjoint (k_xbar<XL>)
        # slot of augmented-input feature f (r, latent channels, ones column) in the XT fragment tiles: tiles 0 / 1 in
        # order, tile 2 sparse -- features 32.. sit in register 0 of its fragment (slots 32, 36, 40, 44), so the GEMMs
        # over the augmented input take 9 k-steps instead of 12 (x_live() in csrc/common.h, k_gather)
        f = np.arange(self.dz + 1)
        self.slot = np.where(f < 16 * (XT - 1), f, 16 * (XT - 1) + 4 * (f - 16 * (XT - 1)))
        widths = [16 * nf, 8 * nf, 4 * nf, 2 * nf, nf, out_features]
        self.layers = []
        theta_off = 0
        for l in range(6):
            kh = 0 if l == 0 else widths[l - 1]
            skip = l < 5
            kin = kh + (self.dz if skip else 0)
            m = widths[l]
            lay = dict(M=m, Kh=kh, KT=kh // 16, MT=(m + 15) // 16, skip=skip, Kin=kin, w_off=theta_off,
                       b_off=theta_off + m * kin)
            theta_off += m * kin + m
            self.layers.append(lay)
        self.n_theta = theta_off
        self._build_indices()
        self._dev = {}
        # dim = 4 (``nd4_jets``): {axis triple: [per layer] index array [3][MT][64][4]} of the `tanc` packs of the passes over
        # the triples other than (0, 1, 2) -- BESIDE pack_index_np, built when a derivative request first needs one (tanc_index)
        self.tanc_nd4 = {}

    def tanc_index(self, triple):
        """dim = 4: the index arrays of the tangent constants of a pass over the axis triple (a0 < a1 < a2), one per layer in the
        layout of the "tanc" pack, [3][MT][64][4]: block (k, mt), lane (g, j), register r = W_s,l[16 mt + 4 g + r, coordinate
        a_k] -- column a_k of the skip block (feature a sits in slot a) -- and the plan's zero for rows past M and for fc5, which
        has no skip block.  (0, 1, 2) is what the "tanc" pack itself holds.  Nothing of pack_index_np / pack_off moves."""
        triple = tuple(int(a) for a in triple)
        if self.dim != 4 or len(triple) != 3 or not (0 <= triple[0] < triple[1] < triple[2] < 4):
            raise ValueError("tanc_index: a strictly increasing axis triple of a dim = 4 plan, not %r" % (triple,))
        if triple not in self.tanc_nd4:
            zero = self.n_theta
            g = np.arange(64) >> 4
            out = []
            for lay in self.layers:
                row = 16 * np.arange(lay["MT"])[:, None, None] + 4 * g[None, :, None] + np.arange(4)[None, None, :]
                col = lay["w_off"] + row * lay["Kin"] + lay["Kh"]
                live = (row < lay["M"]) & bool(lay["skip"])
                out.append(np.stack([np.where(live, col + a, zero) for a in triple], 0).astype(np.int64))
            self.tanc_nd4[triple] = out
        return self.tanc_nd4[triple]

    def pack_tanc(self, params, triples):
        """the `tanc` packs of the passes over ``triples``: {triple: [per layer] flat fp32 tensors}; the parameters are
        concatenated once, every pack is one index gather from them.  No triple: nothing is done."""
        if not triples:
            return {}
        dev = params[0].device
        theta = torch.cat([p.detach().reshape(-1).float() for p in params] + [torch.zeros(1, device=dev)])
        out = {}
        for triple in triples:
            key = (str(dev), tuple(triple))
            if key not in self._dev:
                self._dev[key] = [torch.from_numpy(ix.reshape(-1)).to(dev) for ix in self.tanc_index(triple)]
            out[tuple(triple)] = [theta[ix] for ix in self._dev[key]]
        return out

    def _build_indices(self):
        zero = self.n_theta  # index of the appended 0.0
        lane = np.arange(64)
        g, j = lane >> 4, lane & 15
        r = np.arange(4)
        pack_chunks, unpack = [], np.zeros(self.n_theta, dtype=np.int64)
        self.pack_off = []
        self.dw_off = []
        pk, dwo = 0, 0
        for lay in self.layers:
            M, Kh, KT, MT, Kin = lay["M"], lay["Kh"], lay["KT"], lay["MT"], lay["Kin"]
            Mp, Ka = 16 * MT, 16 * (KT + XT)
            aug = np.full((Mp, Ka), zero, dtype=np.int64)
            rows = np.arange(M)[:, None]
            if Kh:
                aug[:M, :Kh] = lay["w_off"] + rows * Kin + np.arange(Kh)[None, :]
            slot = self.slot
            if lay["skip"]:
                aug[:M, 16 * KT + slot[:self.dz]] = lay["w_off"] + rows * Kin + Kh + np.arange(self.dz)[None, :]
            aug[:M, 16 * KT + slot[self.dz]] = lay["b_off"] + np.arange(M)
            # unpack map: theta element -> position in the flat dW_aug buffer
            if Kh:
                unpack[lay["w_off"] + rows * Kin + np.arange(Kh)[None, :]] = dwo + rows * Ka + np.arange(Kh)[None, :]
            if lay["skip"]:
                unpack[lay["w_off"] + rows * Kin + Kh + np.arange(self.dz)[None, :]] = \
                    dwo + rows * Ka + 16 * KT + slot[:self.dz][None, :]
            unpack[lay["b_off"] + np.arange(M)] = dwo + np.arange(M) * Ka + 16 * KT + slot[self.dz]
            offs = {}

            def add(name, arr):
                nonlocal pk
                offs[name] = (pk, arr.size)
                pack_chunks.append(arr.reshape(-1))
                pk += arr.size

            mt = np.arange(MT)
            # A operand of W_h: [KT][MT][lane][r] = aug[16mt + j, 16kt + 4g + r]
            if KT:
                kt = np.arange(KT)
                add("Wh", aug[(16 * mt[None, :, None, None] + j[None, None, :, None]),
                              (16 * kt[:, None, None, None] + 4 * g[None, None, :, None] + r[None, None, None, :])])
                # A operand of W_h^T: [MT][KT][lane][r] = aug[16mt + 4g + r, 16kt + j]
                add("WhT", aug[(16 * mt[:, None, None, None] + 4 * g[None, None, :, None] + r[None, None, None, :]),
                               (16 * kt[None, :, None, None] + j[None, None, :, None])])
            xt = np.arange(XT)
            add("Ws", aug[(16 * mt[None, :, None, None] + j[None, None, :, None]),
                          (16 * (KT + xt)[:, None, None, None] + 4 * g[None, None, :, None] + r[None, None, None, :])])
            # A operand of W_s^T restricted to the latent channels (the only columns of the augmented input that receive
            # an adjoint): [MT][XL][lane][r] = aug[16mt + 4g + r, 16KT + dim + 16xl + j], zero beyond channel cin - 1
            xl = np.arange(self.xl)
            ch = 16 * xl[None, :, None, None] + j[None, None, :, None] + 0 * r[None, None, None, :]
            wsl = aug[(16 * mt[:, None, None, None] + 4 * g[None, None, :, None] + r[None, None, None, :]),
                      (16 * KT + slot[self.dim + np.minimum(ch, self.cin - 1)])]
            add("WsL", np.where(ch < self.cin, wsl, zero))
            # tangent constants W_s[:, d] of the three coordinate streams.  dim = 1, 2: column d >= dim of the augmented input
            # is a latent channel, not a coordinate -- the stream of an axis the grid does not have starts from zeros and stays
            # identically zero (dim = 4 keeps the columns as they were: nothing carries derivative streams there)
            d = np.arange(3)
            tanc = aug[(16 * mt[None, :, None, None] + 4 * g[None, None, :, None] + r[None, None, None, :]),
                       (16 * KT + d)[:, None, None, None] + 0 * mt[None, :, None, None]]
            if self.dim in ND_JET_DIMS:
                tanc[self.dim:] = zero
            add("tanc", tanc)
            self.pack_off.append(offs)
            self.dw_off.append((dwo, Mp, Ka))
            dwo += Mp * Ka
        self.pack_index_np = np.concatenate(pack_chunks)
        self.unpack_index_np = unpack
        self.n_pack = pk
        self.n_dw = dwo

    def device_indices(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.pack_index_np).to(device),
                              torch.from_numpy(self.unpack_index_np).to(device))
        return self._dev[key]

    def pack(self, params):
        """params: 12 tensors (w0, b0, ..., w5, b5) -> flat pack buffer (one index gather)."""
        dev = params[0].device
        pidx, _ = self.device_indices(dev)
        theta = torch.cat([p.detach().reshape(-1).float() for p in params] + [torch.zeros(1, device=dev)])
        return theta[pidx]

    def pack_bf16(self, packs, nsplit=1):
        """bf16 A-operand packs of the hidden-to-hidden weights: block (q, mt) = the fp32 blocks (2q, mt) and (2q+1, mt)
        lane by lane.  nsplit = 1 (config-4 path): rounded to bf16 -- except the forward packs of the three narrow layers
        fc3 ... fc5, which carry TWO terms hi + lo stacked [2][...] for the two-term products of k_tail_fwd_bf (a kernel that
        takes one term reads the hi part, which comes first).  nsplit = 3 ("fp32x3"): each weight split exactly into three
        bf16 terms hi + mid + lo (8 + 8 + 8 mantissa bits), stacked [3][...] -- the weight side of the fp32-accurate
        six-product scheme of k_layer_coop<..., SPL = 3>.  Returns {(l, "Wh"|"WhT"): tensor}."""
        out = {}
        for l in range(1, 6):
            kt, mt = self.layers[l]["KT"], self.layers[l]["MT"]
            for name, (ka, ma) in (("Wh", (kt, mt)), ("WhT", (mt, kt))):
                if ka % 2 == 0:
                    w = self.pack_view(packs, l, name).view(ka // 2, 2, ma, 64, 4).permute(0, 2, 3, 1, 4)
                    nterm = 2 if (nsplit == 1 and l >= 3 and name == "Wh") else nsplit
                    terms, r = [], w
                    for t in range(nterm):
                        h = r.to(torch.bfloat16)
                        terms.append(h)
                        if t + 1 < nterm:
                            r = r - h.float()
                    out[(l, name)] = (torch.stack(terms, 0) if nterm > 1 else terms[0]).contiguous()
        return out

    def pack_view(self, packs, l, name):
        off, n = self.pack_off[l][name]
        return packs[off:off + n]

    def unpack_grads(self, dw_flat, params):
        _, uidx = self.device_indices(dw_flat.device)
        gtheta = dw_flat[uidx]
        out, o = [], 0
        for p in params:
            n = p.numel()
            out.append(gtheta[o:o + n].view_as(p))
            o += n
        return out


# ------------------------------------------------------------------------------------------------------------
# stream configuration
# ------------------------------------------------------------------------------------------------------------
CANON_PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
# stream sets (S1, S2) the fused fc3 -> fc5 kernels (csrc/jet_tail.hip) and the dgrad-first two-phase backward are compiled for
TAIL_SETS = ((0, 0), (3, 0), (3, 1), (3, 2), (3, 4))


def make_cfg(act, act_param, first, pairs, combo=None):
    """Map a derivative request onto a compiled stream configuration; returns (JetCfg, S, padded_pairs).

    combo = {pair: alpha}: ONE combined second-order stream sum_k alpha_k d2/dq_a dq_b instead of one per pair."""
    if combo:
        cfg = JetCfg()
        cfg.S1, cfg.S2, cfg.combo = 3, 1, 1
        for k, pr in enumerate(CANON_PAIRS):
            cfg.alpha[k] = float(combo.get(pr, 0.0))
        cfg.act = _lib.ACT_CODES[act]
        cfg.act_param = float(act_param)
        return cfg, 5, ["combo"]
    pairs = [tuple(sorted(p)) for p in pairs]
    if pairs and not first:
        first = True
    if not first:
        s1, s2, pp = 0, 0, []
    elif not pairs:
        s1, s2, pp = 3, 0, []
    elif len(pairs) <= 2:
        s1, s2, pp = 3, 2, pairs + [pairs[-1]] * (2 - len(pairs))
    elif len(pairs) <= 4 and os.environ.get("STPDE_S34", "1") != "0":
        # (round 5: BASELINE configs[4] names four second derivatives and ran padded to six; STPDE_S34=0 = the padded set)
        s1, s2, pp = 3, 4, pairs + [pairs[-1]] * (4 - len(pairs))
    elif len(pairs) <= 6:
        s1, s2, pp = 3, 6, pairs + [pairs[-1]] * (6 - len(pairs))
    else:
        raise NotImplementedError("more than 6 second-order derivative pairs")
    cfg = JetCfg()
    cfg.S1, cfg.S2 = s1, s2
    for k, (a, b) in enumerate(pp):
        cfg.pair0[k], cfg.pair1[k] = a, b
    cfg.act = _lib.ACT_CODES[act]
    cfg.act_param = float(act_param)
    return cfg, 1 + s1 + s2, pp


# ------------------------------------------------------------------------------------------------------------
# dim = 4: the pass schedule.  The layer kernels carry three first-order streams; a mixed second derivative needs the streams of
# its two axes only, and the four axis triples of {0, 1, 2, 3} hold all six mixed pairs: any request is at most four passes.
# ------------------------------------------------------------------------------------------------------------
ND4_TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


def _nd4_s2(n):
    """pairs of a pass padded to the S2 of a compiled stream set, as make_cfg pads them"""
    if n <= 2:
        return 2 * (n > 0)
    return 4 if (n <= 4 and os.environ.get("STPDE_S34", "1") != "0") else 6


def nd4_passes(first, pairs):
    """The passes of a derivative request on a 4-d grid: [(triple, pairs of the pass, dst_map)], a pure function of the request.

    pairs: distinct second-derivative pairs (a, b), axes < 4, in the caller's order; the caller's jets tensor is
    [1 + 4 + len(pairs)]: value, d/dq_0 .. d/dq_3, then the pairs.  ``first`` -- or any pair, as in make_cfg -- asks for all four
    first-order streams.  triple: the strictly increasing axes whose tangent streams the pass carries.  pairs of the pass: in
    axes, padded to an even count (2, 4, 6) by repeating the last one.  dst_map = (value, (f0, f1, f2), (p0, ...)): the stream of
    the jets tensor that receives the value, the derivative along triple[k] and each pair of the pass, or -1 (not stored).
    Every pair belongs to exactly one pass whose triple holds both its axes -- the first such pass --, every first-order axis
    is stored by the first pass that carries it, the value by pass 0 alone.  The passes are the first subset of ND4_TRIPLES,
    enumerated by size and then in lexicographic order, whose triples hold every requested pair and axis: their number is the
    minimum.  A triple holds six pairs at most, so no pass carries more.  A request for the value alone is one pass that stores
    nothing else (lig_jets serves it on the value path instead)."""
    import itertools
    pairs = [tuple(sorted((int(a), int(b)))) for a, b in pairs]
    if any(not (0 <= a <= b < 4) for a, b in pairs):
        raise ValueError("dim = 4: second-derivative pairs %r name an axis the grid does not have" % (pairs,))
    if len(set(pairs)) != len(pairs):
        raise ValueError("dim = 4: second-derivative pairs %r name a pair twice" % (pairs,))
    axes = set(range(4)) if (first or pairs) else set()
    for size in range(1, 5):
        for sub in itertools.combinations(ND4_TRIPLES, size):
            if axes <= set().union(*sub) and all(any(set(pr) <= set(t) for t in sub) for pr in pairs):
                out, stored = [], set()
                for k, t in enumerate(sub):
                    own = [(pr, 5 + i) for i, pr in enumerate(pairs)
                           if set(pr) <= set(t) and not any(set(pr) <= set(u) for u in sub[:k])]
                    fdst = tuple(1 + a if (a in axes and a not in stored) else -1 for a in t)
                    stored |= set(t)
                    pad = _nd4_s2(len(own)) - len(own)
                    out.append((t, [pr for pr, _ in own] + ([own[-1][0]] * pad if pad else []),
                                (0 if k == 0 else -1, fdst, tuple(s for _, s in own) + (-1,) * pad)))
                return out
    raise AssertionError("unreachable: the four triples hold every pair and every axis")


def box_constants(shape3, xmin, xmax):
    """lo_c, hi_c, cube with the reference's own fp32 expression sequence
    (src/regular_nd_grid_interpolation.py:40-51), evaluated on the host."""
    dim = len(shape3)

    def as_vec(v):
        if isinstance(v, (int, float)):
            return float(v) * torch.ones([dim], dtype=torch.float32)
        if torch.is_tensor(v):
            return v.detach().to("cpu", torch.float32).reshape(-1)
        return torch.tensor(np.asarray(v)).to(torch.float32).reshape(-1)

    lo, hi = as_vec(xmin), as_vec(xmax)
    if lo.numel() != dim or hi.numel() != dim:
        raise ValueError("xmin/xmax must have one entry per grid dimension")
    if bool((lo != 0).any()):
        # quirk a-Q1: the reference computes ind0 = floor(q / cubesize) with no xmin offset, so xmin != 0
        # silently mis-indexes there; the HIP path refuses instead of reproducing or "fixing" it.
        raise ValueError("xmin must be 0 (the reference's cell index ignores xmin)")
    size = torch.tensor(list(shape3)).float()
    eps = 1e-6 * (hi - lo)
    cube = (hi - lo) / (size - 1)
    return (lo + eps).tolist(), (hi - eps).tolist(), cube.tolist()


_box_cache = {}
_box_tensor_cache = {}     # id(xmin) -> (weakref(xmin), weakref(xmax), key, constants)
_box_lock = threading.RLock()   # re-entrant: a weakref callback (_drop) may fire from a GC pass inside the lock


def cached_box_constants(shape3, xmin, xmax):
    """box_constants with a cache, so that device-tensor bounds (train.py:48-49 passes CUDA tensors) do not cost a
    device sync per call.  Tensor entries are keyed on id(xmin) and validated through weak references to BOTH tensor
    objects plus their version counters (an id alone could alias a freed tensor; a WeakKeyDictionary cannot be used
    because its lookups compare keys with ``==``, which is elementwise for tensors); python scalars / sequences are
    keyed by value."""
    shape3 = tuple(shape3)
    if torch.is_tensor(xmin) and torch.is_tensor(xmax):
        import weakref
        key = (shape3, xmin._version, xmax._version)
        with _box_lock:
            ent = _box_tensor_cache.get(id(xmin))
            if ent is not None and ent[0]() is xmin and ent[1]() is xmax and ent[2] == key:
                return ent[3]
        val = box_constants(shape3, xmin, xmax)
        ident = id(xmin)

        def _drop(_ref, ident=ident):
            with _box_lock:
                cur = _box_tensor_cache.get(ident)
                if cur is not None and cur[0] is _ref:
                    del _box_tensor_cache[ident]

        with _box_lock:
            if len(_box_tensor_cache) > 256:
                _box_tensor_cache.clear()
            _box_tensor_cache[ident] = (weakref.ref(xmin, _drop), weakref.ref(xmax), key, val)
        return val
    if torch.is_tensor(xmin) or torch.is_tensor(xmax):
        return box_constants(shape3, xmin, xmax)
    key = (shape3, repr(xmin), repr(xmax))
    with _box_lock:
        if key not in _box_cache:
            if len(_box_cache) > 64:
                _box_cache.clear()
            _box_cache[key] = box_constants(shape3, xmin, xmax)
        return _box_cache[key]


# ------------------------------------------------------------------------------------------------------------
# the autograd function
# ------------------------------------------------------------------------------------------------------------
def _tail_applies(fused_tail, nf, cfg, combo, value_tiles=False):
    """THE predicate of the fused fc3 -> fc4 -> fc5 kernels: the switch, the reference widths, and a training stream set they are
    compiled for (a combined second-order stream needs its per-row weights) or the value-tile pass of a forward-only value query."""
    return bool(fused_tail and nf in (16, 32) and (value_tiles or ((cfg.S1, cfg.S2) in TAIL_SETS and (cfg.S2 != 1 or combo))))


@dataclasses.dataclass(frozen=True, eq=False)
class Nd4Pass:
    """One pass of a derivative request on a 4-d grid (``nd4_passes``) as the driver runs it."""
    triple: tuple           # the axes whose tangent streams the layer kernels carry: slot k of the pass = axis triple[k]
    cfg: JetCfg             # the pass's stream set; its pairs name SLOTS of the triple
    S: int                  # streams of the layer buffers in this pass
    desc: Nd4PassDesc       # what stpde_lig_reduce_nd4_jet_fwd takes: axes, pairs in axes, the destination-stream map


def _nd4_records(act, act_param, first, pairs, S_out):
    """nd4_passes as Nd4Pass records.  A piecewise-linear activation carries value + tangents only, (3, 0): the reduction
    supplies the second derivatives from the weight cross terms, as for every other dimension."""
    linear = act in ("relu", "leakyrelu")
    recs = []
    for triple, pp, (dst_value, dst_first, dst_pair) in nd4_passes(first, pairs):
        cfg, S, padded = make_cfg(act, act_param, True, [] if linear else [(triple.index(a), triple.index(b)) for a, b in pp])
        assert linear or len(padded) == len(pp)
        d = Nd4PassDesc()
        d.npairs, d.S_mlp, d.S, d.dst_value = len(pp), S, S_out, dst_value
        for k in range(3):
            d.axis[k], d.dst_first[k] = triple[k], dst_first[k]
        for k, (a, b) in enumerate(pp):
            d.pair0[k], d.pair1[k], d.dst_pair[k] = a, b, dst_pair[k]
        recs.append(Nd4Pass(triple, cfg, S, d))
    return tuple(recs)


@dataclasses.dataclass(frozen=True, eq=False)
class JetCall:
    """What one jet call is and how it runs, decided ONCE when the call is made (``JetCall.make``) and read by every later
    stage: the forward, its chunks, the backward and a stash rebuild inside the backward.  Frozen -- except ``chunk``."""
    # ---- plan and request
    plan: ImNetPlan         # layout of the IM-NET architecture
    cfg: JetCfg             # streams the layer kernels carry
    cfg_out: JetCfg         # streams the caller gets (second-order ones of a piecewise-linear activation come from the reduction)
    cfg_val: JetCfg         # the value stream alone (layer-0 weight gradient of the split layer-0 adjoint)
    S: int                  # number of MLP streams
    S_out: int              # number of output streams
    pairs: list             # padded second-derivative pairs of the output streams (["combo"]: one combined stream)
    # ---- operands
    bf16: bool              # bf16 A-operand packs of the hidden-to-hidden weights exist ("bf16" and "fp32x3")
    nsplit: int             # bf16 terms per weight: 1, or 3 = the exact split of "fp32x3"
    packed_mask: int        # bit l: the buffer of layer l's rows is PACKED (bit 0: the layer-0 value adjoint); 31 or 0
    # ---- geometry
    B: int                  # batch
    N: int                  # query points per batch entry
    grid_shape: tuple       # nodes per axis of the latent grid
    lo_c: list              # clamp bounds and cell size per axis (box_constants)
    hi_c: list
    cube: list
    P_pad: int              # B * N padded to whole tiles / value-tile passes
    # ---- memory plan
    budget: object          # bytes the stash + scratch of the call may take (None: the free device memory)
    recompute: bool         # keep no stash, rebuild it in the backward (``force_recompute``)
    chunk: int              # points per launch chunk; the ONE field written after construction, through plan_chunk only: by the
    #                         memory plan of LigJetFunction.forward (and by lig_jets for the device-dependent n-D default)
    # ---- gradient need
    need_grad: bool         # a backward can follow (grad mode was on and an input requires grad)
    # ---- switches, frozen when the call is made
    det: bool               # _lib.deterministic: dW in long accumulators
    det_dlatent: bool       # d latent as a per-node sum in a fixed order (False: atomic scatter)
    value_tiles: bool       # forward-only value queries on the value-tile kernels
    tan0_rowsum: bool       # layer-0 tangent adjoints as per-tile row sums
    wgrad_split: bool       # "fp32x3": weight gradients on the split operands too
    fused_tail: bool        # fc3 -> fc5 in one kernel where ``tail`` / a value-tile pass allows
    fc1_fused: bool         # bf16 mode: fused backward of the first hidden layer (STPDE_FC1_FUSED)
    fc2_fused: bool         # exact fp32: fused backward of the second hidden layer where the library serves it (``fc2_fused``)
    nd_backward: bool       # dim = 1, 2, 4: the HIP training backward is allowed
    nd_jets: bool           # dim = 1, 2: coordinate derivatives in HIP are allowed (forward passes that need no gradient)
    nd_jet_backward: bool   # dim = 1, 2: ... and so is their training backward (only together with ``nd_jets``)
    pipeline: bool          # driver: one library call per direction (dim = 3, no per-kernel profile), else kernel by kernel
    # ---- derived, computed once
    tail: bool              # the fused fc3 -> fc5 kernels serve this call's training stream set (_tail_applies)
    SP0: int                # streams of the layer-0 adjoint: value (+ 3 tangents)
    split0: bool            # ... kept as value blocks + tangent row sums
    mult: int               # points a launch chunk is a multiple of
    # ---- dim = 4 derivative requests (``nd4_jets``); cfg / S above are then those of the WIDEST pass: the layer buffers are
    #      sized for it and reused from pass to pass
    nd4_jets: bool = False  # dim = 4: coordinate derivatives in HIP are allowed (forward passes that need no gradient)
    passes: tuple = ()      # the Nd4Pass records of the request; empty for every other call

    @classmethod
    def make(cls, plan, act, act_param, first, pairs, combo, precision, grid_shape, box, budget=None, B=1, N=0,
             chunk_points=None, need_grad=True):
        """The record of a call: needs no device.  box = (lo_c, hi_c, cube); precision / budget None: the module settings.  Reads
        ``_lib.deterministic`` and the module switches -- the only place of this module that does."""
        precision = precision or mlp_precision
        if precision not in ("fp32", "bf16", "fp32x3"):
            raise ValueError("mlp precision must be 'fp32', 'bf16' or 'fp32x3'")
        dim = plan.dim
        if dim != 3 and precision == "bf16":
            # (the value-tile kernels have no one-term bf16 variant; local_implicit_grid routes such a query to the composed ops)
            raise NotImplementedError("dim = %d value queries run with fp32 or fp32x3 operands" % dim)
        # output streams (what the caller gets) vs MLP streams (what the layer kernels carry): for piecewise-linear
        # activations sigma'' = 0 makes every second-order MLP stream identically zero, so only value + gradient streams
        # go through the network and the reduction supplies the second derivatives from the weight cross terms
        passes = ()
        if dim == 4 and (first or len(pairs) or combo):
            # 3-d space + time: the request runs as passes over axis triples.  cfg_out stands for "value + tangents, no combined
            # stream" (nothing reads its pairs), the caller's streams are value, four first-order ones and the pairs as asked
            if not nd4_jets:
                raise NotImplementedError(_ND_VALUE_ONLY % dim)
            if combo:
                raise NotImplementedError("dim = 4: the combined second-order stream is dim = 3 only (ask for the pairs)")
            ppairs = [tuple(sorted((int(a), int(b)))) for a, b in pairs]
            S_out = 1 + 4 + len(ppairs)
            passes = _nd4_records(act, act_param, first, ppairs, S_out)
            cfg_out = make_cfg(act, act_param, True, [])[0]
            cfg, S = max(((ps.cfg, ps.S) for ps in passes), key=lambda cs: cs[1])
        else:
            cfg_out, S_out, ppairs = make_cfg(act, act_param, first, list(pairs), combo)
            cfg, S = cfg_out, S_out
            if act in ("relu", "leakyrelu") and ppairs:
                cfg, S, _ = make_cfg(act, act_param, True, [])
        tail = _tail_applies(fused_tail, plan.nf, cfg, cfg_out.combo)
        # bf16 mode, reference width: the stashes of the hidden layers' output rows and their adjoints in the PACKED form -- all
        # of their consumers are bf16-operand kernels (layers 1-2: k_layer_coop / k_wgrad_coop; fc3 -> fc5: k_tail_fwd_bf /
        # k_tail_bwd_bf and the bf16 variant of k_wgrad_wave).  ``packed_stash = False``: fp32 blocks, fp32 MFMA in fc3 -> fc5.
        # (S > 6 is not served by the bf16 kernels; the packed buffer of fc2's rows is read by the fused fc3 -> fc5 kernels.)
        # Bits 1-4: the layer buffers of fc1 ... fc4's rows; bit 0: the value-stream adjoint of layer 0 as bf16 blocks (needs
        # the tangent row sums: value-only adjoint).  The library serves "all of them" or none.
        packed = (precision == "bf16" and packed_stash and plan.nf == 32 and S <= 6 and tail and cfg.S1 == 3 and tan0_rowsum)
        # tiles hold 2 points, value-only queries run whole value-tile passes (4 tiles).  dim = 1, 2, 4: 16 >> dim points per
        # tile, whole passes; the gather pads the last tiles of a chunk itself (nd_tiles), the points are not padded; default
        # chunk there: the row TILES of the dim = 3 chunk, which lig_jets cuts down to what the device has free
        mult = (8 if S == 1 else 2) if dim == 3 else 4 * (16 >> dim)
        chunk_points = chunk_points or (DEFAULT_CHUNK if dim == 3 else (DEFAULT_CHUNK // 2) * (16 >> dim))
        P, SP0 = B * N, 1 + cfg.S1
        return cls(plan=plan, cfg=cfg, cfg_out=cfg_out, cfg_val=make_cfg(act, act_param, False, [])[0], S=S, S_out=S_out,
                   pairs=ppairs, bf16=precision in ("bf16", "fp32x3"), nsplit=3 if precision == "fp32x3" else 1,
                   packed_mask=31 if packed else 0, B=B, N=N, grid_shape=tuple(grid_shape), lo_c=box[0], hi_c=box[1],
                   cube=box[2], P_pad=P + ((-P) % mult if dim == 3 else 0),
                   budget=budget if budget is not None else memory_budget, recompute=bool(force_recompute),
                   chunk=max(mult, chunk_points // mult * mult), need_grad=bool(need_grad), det=bool(_lib.deterministic),
                   det_dlatent=bool(deterministic_dlatent), value_tiles=bool(value_tiles), tan0_rowsum=bool(tan0_rowsum),
                   wgrad_split=bool(wgrad_split), fused_tail=bool(fused_tail), fc1_fused=fc1_fused_enabled(),
                   fc2_fused=fc2_fused_enabled(),
                   nd_backward=bool(nd_backward), nd_jets=bool(nd_jets),
                   nd_jet_backward=bool(nd_jets and nd_jet_backward),
                   pipeline=bool(use_pipeline and profile is None and dim == 3),
                   tail=tail, SP0=SP0, split0=bool(SP0 == 4 and tan0_rowsum), mult=mult,
                   nd4_jets=bool(nd4_jets), passes=passes)

    def plan_chunk(self, points):
        """the one write of the record: ``chunk``, by the memory plan (LigJetFunction.forward; lig_jets: the n-D default)"""
        object.__setattr__(self, "chunk", points)


def _AW(call):
    """floats of storage per accumulated dW element: 1, or -- deterministic mode -- a long accumulator (_lib.DET_K int64)"""
    return 2 * _lib.DET_K if call.det else 1


def _dw_slice(call, dw_flat, l):
    """layer l's part of the flat dW buffer"""
    off, mp, ka = call.plan.dw_off[l]
    return dw_flat[_AW(call) * off:_AW(call) * (off + mp * ka)]


def _layer_desc(call, ntiles, lay, cfg, first_hidden, bf16=0, packed=0):
    d = LayerDesc()
    d.ntiles, d.KT, d.MT, d.first_hidden, d.cfg = ntiles, lay["KT"], lay["MT"], int(first_hidden), cfg
    d.mfma_bf16 = int(bf16)
    d.packed = int(packed)
    d.det = int(call.det)      # (read by the weight-gradient entry points only)
    return d


def _buf_floats(call, l, nt):
    """floats of the layer buffer of layer l's output rows for nt row tiles: [S][MT] fp32 blocks, or the PACKED form (bf16
    mode: value stream fp32, derivative streams bf16; include/stpde_hip.h, stpde_layer_desc.packed)."""
    mt = call.plan.layers[l]["MT"]
    if (call.packed_mask >> l) & 1:
        return nt * mt * (256 + (call.S - 1) * 128)
    return nt * call.S * mt * _FRAG


def _adj_floats(call, l, nt):
    """floats of the adjoint buffer of layer l's output rows: the size of the layer buffer, or -- packed mode -- a packed
    ADJOINT buffer, every stream bf16 (layer 0: its value stream only)."""
    mt = call.plan.layers[l]["MT"]
    if (call.packed_mask >> l) & 1:
        return nt * (call.S if l else 1) * mt * 128
    return nt * mt * _FRAG if l == 0 else _buf_floats(call, l, nt)


def _pk(call, l, writes):
    """stpde_layer_desc.packed of a call on layer l that writes the buffer of layer `writes` (-1: none)."""
    m = call.packed_mask
    return (1 if (l >= 2 and (m >> (l - 1)) & 1) else 0) | (2 if (writes >= 0 and (m >> writes) & 1) else 0) | \
        (4 if (m >> l) & 1 else 0)


# ------------------------------------------------------------------------------------------------------------
# one C call per direction (include/stpde_hip.h: stpde_lig_imnet_jet_fwd / _bwd); the per-kernel functions below stay as
# the profiling path (bench.py's per-kernel event timings) and are what ``use_pipeline = False`` selects (tests)
# ------------------------------------------------------------------------------------------------------------
use_pipeline = True


def _dp(t):
    return None if t is None else t.data_ptr()


def _plan_desc(call, packs, packs16):
    plan = call.plan
    d = ImNetPlanDesc()
    d.nlayers, d.cin, d.cout, d.nf16 = 6, plan.cin, plan.cout, plan.nf // 16
    pv = plan.pack_view
    for l, lay in enumerate(plan.layers):
        d.KT[l], d.MT[l] = lay["KT"], lay["MT"]
        if lay["KT"]:
            d.Wh[l], d.WhT[l] = pv(packs, l, "Wh").data_ptr(), pv(packs, l, "WhT").data_ptr()
        d.Ws[l], d.WsL[l], d.tanc[l] = (pv(packs, l, n).data_ptr() for n in ("Ws", "WsL", "tanc"))
        if packs16:
            d.Wh16[l], d.WhT16[l] = _dp(packs16.get((l, "Wh"))), _dp(packs16.get((l, "WhT")))
        d.dw_off[l] = plan.dw_off[l][0]
    d.mfma_bf16 = call.nsplit if packs16 else 0
    d.packed_mask = call.packed_mask
    return d


def _gather_desc(call, latent, Pc, p0):
    gd = GatherDesc()
    gd.P, gd.N, gd.B = Pc, call.N, call.B
    gd.n0, gd.n1, gd.n2, gd.C = latent.shape[1], latent.shape[2], latent.shape[3], latent.shape[4]
    for k in range(3):
        gd.lo_c[k], gd.hi_c[k], gd.cube[k] = call.lo_c[k], call.hi_c[k], call.cube[k]
    gd.p_base = p0
    for k in range(6):
        gd.alpha[k] = call.cfg_out.alpha[k]
    return gd


def _flags(call, need_grad, need_wgrad=True):
    """STPDE_F_* of the one-call entry points (the forward reads F_STASH, F_VALUE_TILES and F_FUSED_TAIL only)"""
    bits = ((need_grad, _lib.F_STASH), (call.value_tiles, _lib.F_VALUE_TILES), (call.fused_tail, _lib.F_FUSED_TAIL),
            (call.tan0_rowsum, _lib.F_TAN0_ROWSUM), (call.det_dlatent, _lib.F_DETERMINISTIC), (need_wgrad, _lib.F_WGRAD),
            (not call.wgrad_split, _lib.F_WGRAD_FP32), (not call.fc1_fused, _lib.F_NO_FC1_FUSED), (call.det, _lib.F_DET),
            (call.fc2_fused, _lib.F_FC2_FUSED))
    return sum(bit for on, bit in bits if on)


def nd_tiles(P, dim):
    """Row tiles of P points of a value query on a dim-d grid (dim = 1, 2, 4): 16 >> dim points per tile, rounded up to
    the four tiles of one value-tile pass.  Rows past the last point are padding (zeros, weight 0: stpde_lig_gather_nd)."""
    tp = 16 >> dim
    return (-(-P // tp) + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------------------
# THE table of the device buffers one launch chunk owns: [(name, elements, dtype)] in the order they are allocated.  The four
# chunk drivers allocate from it (``_alloc``) and the memory plan sums it (``_per_point_bytes`` ...): a buffer is allocated and
# counted, or neither.  The one-call and the per-kernel driver differ in the order (the caching allocator, and with it the
# peak, sees it): the ``_ORDER`` rows, keyed by ``call.pipeline``.
# ------------------------------------------------------------------------------------------------------------
_LAYER_BUFS = tuple("buf%d" % l for l in range(1, 6))
_FWD_ORDER = {True: ("X", "cw", "coef", "cell") + _LAYER_BUFS + ("z0",),
              False: ("X", "cw", "roww", "coef", "coef4", "cell", "buf1", "z0") + _LAYER_BUFS[1:]}
_BWD_ORDER = {True: ("abar2x", "abar3x", "abar1x", "abar4x", "abar0x", "tan0", "abar0"),
              False: ("abar0", "abar0x", "tan0", "abar1x", "abar4x", "abar3x", "abar2x")}
_DTYPES = dict(cell=torch.int32, perm=torch.int32, start=torch.int32, sort_tmp=torch.uint8)     # every other one: fp32
# the one size the PLAN estimates: 24 bytes per point for the temporary storage of the cell sort.  What is allocated is the
# library's own answer (stpde_lig_sort_tmp_bytes), and asking for it needs the library.
SORT_TMP_PLAN_BYTES = 24


def _table(order, size):
    """the buffers of ``order`` that exist (size[name] is not None)"""
    return [(k, size[k], _DTYPES.get(k, torch.float32)) for k in order if size.get(k) is not None]


def _chunk_tiles(call, Pc):
    return nd_tiles(Pc, call.plan.dim) if call.plan.dim != 3 else Pc // 2


def _forward_buffers(call, Pc, need_grad=True):
    """Forward chunk: the fragment image X of the augmented input, what the gather records per point (dim = 3: row weights of
    a combined second-order stream, interpolation coefficients, cell index; dim = 1, 2, 4: the corner weight of every row, and
    coefficients for a derivative request only -- dim = 4: the wider record of all four axes, ``coef4``), the five layer buffers
    (dim = 4: of the widest pass, ``call.S`` streams), and -- a backward can follow -- the value stream z0 of the layer-0
    pre-activations."""
    nd, nt = call.plan.dim != 3, _chunk_tiles(call, Pc)
    size = dict(X=nt * XT * _FRAG, cw=Pc * 8 if call.cfg_out.combo else None, roww=nt * 16 if nd else None,
                coef=Pc * 16 if ((not nd or call.S_out > 1) and not call.passes) else None,
                coef4=Pc * 24 if call.passes else None, cell=None if nd else Pc,
                z0=nt * call.plan.layers[0]["MT"] * _FRAG if need_grad else None)
    size.update(("buf%d" % l, _buf_floats(call, l, nt)) for l in range(1, 6))
    return _table(_FWD_ORDER[call.pipeline], size)


def _backward_buffers(call, Pc):
    """Backward chunk, the adjoints that do not go over a stash: fresh ones for layers 2 and 3 (one-call path: always;
    per-kernel path: for the fused fc3 -> fc5 chain), the packed ADJOINT buffers of the bf16 mode (a format of their own), and
    for layer 0 with tangent streams their row sums ``tan0`` or -- ``tan0_rowsum = False`` -- the full four-stream adjoint."""
    nt, mt0, pk = _chunk_tiles(call, Pc), call.plan.layers[0]["MT"], call.packed_mask
    on = {2: call.pipeline or call.tail, 3: call.pipeline or call.tail, 1: pk, 4: pk, 0: pk & 1}
    size = {"abar%dx" % l: _adj_floats(call, l, nt) for l in on if on[l]}
    size["tan0"] = nt * mt0 * 48 if call.split0 else None
    size["abar0"] = nt * call.SP0 * mt0 * _FRAG if (call.SP0 == 4 and not call.split0) else None
    return _table(_BWD_ORDER[call.pipeline], size)


def _dlatent_buffers(call, Pc, estimate=False):
    """Scratch of d latent as a per-node sum in a fixed order (dim = 3: ``det_dlatent``; dim = 1, 2, 4: always, with the cell
    ids the forward does not keep there): the latent adjoint of every row (dim = 1, 2, 4: of all 16 rows of every tile,
    k_xbar writes the padding rows too), the permutation of the points sorted by cell, the first sorted point of every grid
    node, the temporary storage of the sort (``estimate``: what the plan counts for it)."""
    nd = call.plan.dim != 3
    if not (nd or call.det_dlatent):
        return []
    rows, n_nodes = 16 * _chunk_tiles(call, Pc) if nd else 8 * Pc, call.B * math.prod(call.grid_shape)
    tmp = SORT_TMP_PLAN_BYTES * Pc if estimate else int(_lib.lib().stpde_lig_sort_tmp_bytes(Pc, n_nodes))
    size = dict(xrows=rows * ((call.plan.cin + 3) // 4 * 4), perm=Pc, start=n_nodes + 1, sort_tmp=tmp, cell=Pc if nd else None)
    return _table(("xrows", "perm", "start", "sort_tmp", "cell"), size)


def _two_phase_buffers(call, Pc):
    """Extras of the dgrad-first order (one-call path: tiles of 2 points): adjoint buffers of layers 1 and 0 of their own, which
    the packed mode has anyway"""
    return _table(("abar1x", "abar0x"), {"abar%dx" % l: _adj_floats(call, l, Pc // 2)
                                         for l in (1, 0) if not (call.packed_mask >> l) & 1})


def _alloc(table, dev):
    """{name: tensor} of a table on ``dev``, allocated in the table's order"""
    return {name: torch.empty(n, device=dev, dtype=dtype) for name, n, dtype in table}


def _forward_chunk_c(call, packs, packs16, latent, pts_c, jets, p0, need_grad=True):
    """_forward_chunk through ONE library call: this function only allocates the chunk's buffers."""
    Pc = pts_c.shape[0]
    s = _alloc(_forward_buffers(call, Pc, need_grad), pts_c.device)
    s["bufs"] = [None] + [s.pop(name) for name in _LAYER_BUFS]
    ws = LigWorkspace()
    ws.X, ws.coef, ws.cw, ws.cell = (_dp(s.get(k)) for k in ("X", "coef", "cw", "cell"))
    ws.pre[0] = _dp(s.get("z0"))
    for l in range(1, 6):
        ws.pre[l] = s["bufs"][l].data_ptr()
    pd = _plan_desc(call, packs, packs16)
    gd = _gather_desc(call, latent, Pc, p0)
    check(_lib.lib().stpde_lig_imnet_jet_fwd(C.byref(pd), C.byref(call.cfg), C.byref(call.cfg_out), C.byref(gd), ptr(pts_c),
                                             ptr(latent), C.byref(ws), C.c_void_p(jets.data_ptr() + 4 * p0), jets.shape[2],
                                             _flags(call, need_grad), stream_ptr()))
    s.update(p0=p0, Pc=Pc, ws=ws, gd=gd)
    return s


def _backward_chunk_c(call, packs, packs16, saved, jets_bar, dw_flat, dlatent, pbar=None, after_dlatent=None):
    """_backward_chunk through ONE library call (+ allocation of its scratch).

    after_dlatent (callable or None): "dgrad-first" order in TWO calls -- phase A runs the whole input-gradient chain into
    fresh adjoint buffers and finishes d latent, after_dlatent() is called (the point-sharded step starts the all-reduce of
    d latent there), phase B computes the remaining weight gradients while that all-reduce is in flight.  (Both phases on the
    current stream.  Round 4's variant with phase B on a side stream, so that the U-Net backward ran beside it, measured slower
    -- profiles/r4_overlap_timeline.txt -- and was deleted in round 6.)"""
    Pc, ws, gd = saved["Pc"], saved["ws"], saved["gd"]
    # (the stream sets of ``tail`` have SP0 = 1 or 4, what the two-phase order is compiled for)
    two_phase = after_dlatent is not None and call.tail and call.tan0_rowsum
    scratch = _alloc(_backward_buffers(call, Pc) + (_dlatent_buffers(call, Pc) if dlatent is not None else [])
                     + (_two_phase_buffers(call, Pc) if two_phase else []), saved["X"].device)
    for name, t in scratch.items():         # (the table's names are the workspace's)
        setattr(ws, name, t.data_ptr())
    if "sort_tmp" in scratch:
        ws.sort_tmp_bytes = scratch["sort_tmp"].numel()
    pd = _plan_desc(call, packs, packs16)
    flags = _flags(call, True, dw_flat is not None)

    def launch(fl):
        check(_lib.lib().stpde_lig_imnet_jet_bwd(C.byref(pd), C.byref(call.cfg), C.byref(call.cfg_out), C.byref(call.cfg_val),
                                                 C.byref(gd), C.byref(ws), C.c_void_p(jets_bar.data_ptr() + 4 * saved["p0"]),
                                                 jets_bar.shape[2], ptr(dw_flat), ptr(dlatent), ptr(pbar), fl, stream_ptr()))

    if two_phase:
        launch(flags | _lib.F_PHASE_A)
        after_dlatent()
        launch(flags | _lib.F_PHASE_B)
    else:
        launch(flags)
        if after_dlatent is not None:
            after_dlatent()


def _gather_nd_desc(call, latent, Pc, p0, nt):
    gd = GatherNdDesc()
    gd.D, gd.P, gd.N, gd.B, gd.C, gd.p_base, gd.ntiles = call.plan.dim, Pc, call.N, call.B, latent.shape[-1], p0, nt
    for k in range(call.plan.dim):
        gd.n[k], gd.lo_c[k], gd.hi_c[k], gd.cube[k] = latent.shape[1 + k], call.lo_c[k], call.hi_c[k], call.cube[k]
    return gd


def _forward_chunk(call, packs, packs16, latent, pts_c, jets, p0, need_grad=True, tancs=None):
    """Run gather + layers 1..5 + reduce for points [p0, p0+Pc) ; returns the buffers backward needs.

    dim = 4 with derivative streams (``call.passes``): the gather and stpde_lig_coef_nd4 once, then per pass layers 1..5 with
    the pass's stream set and `tanc` packs (``tancs`` = {triple: [per layer]}, ImNetPlan.pack_tanc; (0, 1, 2) is the plan's own
    pack) into the SAME layer buffers, and stpde_lig_reduce_nd4_jet_fwd into the streams of ``jets`` the pass owns."""
    nd = call.plan.dim != 3       # query on a 1-, 2- or 4-d grid: own gather / corner sum, the same layer kernels
    nd4 = bool(call.passes)       # ... with derivative streams on a 4-d grid (``nd4_jets``)
    nd_jet = nd and call.S_out > 1 and not nd4    # ... on a 1- / 2-d grid (``nd_jets``; lig_jets let nothing else through)
    if call.pipeline:
        return _forward_chunk_c(call, packs, packs16, latent, pts_c, jets, p0, need_grad)
    plan, cfg, S = call.plan, call.cfg, call.S
    L, st = _lib.lib(), stream_ptr()
    Pc = pts_c.shape[0]
    nt = _chunk_tiles(call, Pc)
    s = _alloc(_forward_buffers(call, Pc, need_grad), pts_c.device)
    bufs = s["bufs"] = [None] + [s.pop(name) for name in _LAYER_BUFS]
    # (z0 is kept for the layer-1 input-gradient kernel, which then writes the layer-0 adjoint over it: reading 2 KB per row
    # back is cheaper than regenerating it on the fp32 MFMA)
    X, cw, coef, cell, roww, z0 = (s.get(k) for k in ("X", "cw", "coef", "cell", "roww", "z0"))
    if nd:
        gd = _gather_nd_desc(call, latent, Pc, p0, nt)
        with _timed("gather_nd"):
            check(L.stpde_lig_gather_nd(C.byref(gd), ptr(pts_c), ptr(latent), ptr(X), ptr(roww), st))
        if nd4:
            with _timed("coef_nd4"):
                check(L.stpde_lig_coef_nd4(C.byref(gd), ptr(pts_c), ptr(s["coef4"]), st))
        if nd_jet:
            with _timed("coef_nd"):
                check(L.stpde_lig_coef_nd(C.byref(gd), ptr(pts_c), ptr(coef), st))
    else:
        gd = _gather_desc(call, latent, Pc, p0)
        with _timed("gather"):
            check(L.stpde_lig_gather(C.byref(gd), ptr(pts_c), ptr(latent), ptr(X), None, ptr(coef), ptr(cell), ptr(cw), st))
    pv = plan.pack_view
    # forward-only value queries (inference): VALUE-TILE kernels -- four consecutive row tiles share one pass over the
    # weights (the weight operand is what bounds a one-stream pass); same buffers, a quarter of the "tiles"
    vt = S == 1 and not need_grad and (not packs16 or call.nsplit == 3) and nt % 4 == 0 and call.value_tiles
    lcfg, lnt = cfg, nt
    if vt:
        lcfg = JetCfg()
        lcfg.S1, lcfg.S2, lcfg.act, lcfg.act_param = 0, 3, cfg.act, cfg.act_param
        lnt = nt // 4
    def layers(lcfg, lnt, tail_cfg, tc):
        """layers 1 .. 5 over ``lnt`` tiles in the stream set ``lcfg``; tail_cfg: the stream set that decides whether the fused
        fc3 -> fc5 kernel serves them (a value-tile pass runs in its own ``lcfg`` and is decided by the call's);
        tc(l): the tangent constants of layer l"""
        # fc3 -> fc4 -> fc5 in one kernel (inter-layer data in registers) for the reference widths and the training stream sets
        tail = _tail_applies(call.fused_tail, plan.nf, tail_cfg, call.cfg_out.combo, vt)
        for l in range(1, 6):
            lay = plan.layers[l]
            if tail and l == 3:
                arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
                pk_tail = (call.packed_mask >> 2) & 1         # bf16 mode: packed buffers on both sides, bf16-operand kernel
                w16s = arr([packs16[(k, "Wh")] for k in (3, 4, 5)]) if pk_tail else None
                with _timed("tail_fwd"):
                    check(L.stpde_jet_tail_fwd_p(C.byref(lcfg), lnt, plan.nf // 16, ptr(bufs[2]), ptr(X),
                                                 arr([pv(packs, k, "Wh") for k in (3, 4, 5)]),
                                                 arr([pv(packs, k, "Ws") for k in (3, 4, 5)]),
                                                 arr([tc(k) for k in (3, 4, 5)]), arr(bufs[3:6]), ptr(cw),
                                                 3 if pk_tail else 0, w16s, st))
                break
            w16 = packs16.get((l, "Wh")) if packs16 else None
            d = _layer_desc(call, lnt, lay, lcfg, l == 1, call.nsplit if w16 is not None else 0, _pk(call, l, l) & 3)
            with _timed("layer%d_fwd" % l):
                check(L.stpde_jet_layer_fwd(C.byref(d), ptr(bufs[l - 1]), ptr(X), ptr(pv(packs, l, "Wh")),
                                            ptr(pv(packs, l, "Ws")), ptr(tc(l)), ptr(pv(packs, 0, "Ws")),
                                            ptr(tc(0)), ptr(bufs[l]), ptr(cw), ptr(w16),
                                            ptr(z0) if l == 1 else None, st))

    if nd4:
        for ps in call.passes:
            own = None if ps.triple == ND4_TRIPLES[0] else tancs[ps.triple]
            layers(ps.cfg, nt, ps.cfg, (lambda l: pv(packs, l, "tanc")) if own is None else (lambda l: own[l]))
            with _timed("reduce_nd4_jet"):
                check(L.stpde_lig_reduce_nd4_jet_fwd(C.byref(ps.desc), plan.dim, Pc, nt, plan.cout, ptr(bufs[5]), ptr(s["coef4"]),
                                                     C.c_void_p(jets.data_ptr() + 4 * p0), jets.shape[2], st))
        return None     # (forward only: no stash)
    layers(lcfg, lnt, cfg, lambda l: pv(packs, l, "tanc"))
    if nd_jet:
        with _timed("reduce_nd_jet"):
            check(L.stpde_lig_reduce_nd_jet_fwd(C.byref(call.cfg_out), S, plan.dim, Pc, nt, plan.cout, ptr(bufs[5]), ptr(coef),
                                                C.c_void_p(jets.data_ptr() + 4 * p0), jets.shape[2], st))
    elif nd:
        with _timed("reduce_nd"):
            check(L.stpde_lig_reduce_nd_fwd(plan.dim, Pc, nt, plan.cout, ptr(bufs[5]), ptr(roww),
                                            C.c_void_p(jets.data_ptr() + 4 * p0), jets.shape[2], st))
    else:
        with _timed("reduce_fwd"):
            check(L.stpde_lig_reduce_fwd(C.byref(call.cfg_out), S, Pc, plan.cout, ptr(bufs[5]), ptr(coef),
                                         C.c_void_p(jets.data_ptr() + 4 * p0), jets.shape[2], st))
    if nd and not need_grad:    # no stash
        return None
    # (dim = 1, 2, 4, ``nd_backward`` / ``nd_jet_backward``: the backward needs the points again, for the cell ids --
    # stpde_lig_cell_nd; a derivative request keeps its coefficient records ``coef`` in the table's stash like dim = 3)
    s.update(pts_c=pts_c, p0=p0, Pc=Pc)
    return s


def _backward_chunk(call, packs, packs16, saved, jets_bar, dw_flat, dlatent, pbar=None, after_dlatent=None):
    """reduce_bwd -> for l = 5..1: wgrad_l (reads abar_l and the still intact pre-activations of layer l-1), then
    dgrad_l (overwrites them with abar_{l-1}) -> wgrad_0 -> xbar/scatter.

    dim = 1, 2, 4 (``nd_backward``): stpde_lig_reduce_nd_bwd, the same S = 1 wgrad / dgrad sequence over the chunk's
    ``nd_tiles`` row tiles, then xbar_rows -> cell_nd -> cell_sort -> dlatent_reduce_nd.  d latent on these grids is ALWAYS
    the deterministic per-node sum: ``deterministic_dlatent = False`` is ignored, there is no atomic variant.

    dim = 1, 2 with derivative streams (``nd_jet_backward``): stpde_lig_reduce_nd_jet_bwd, then the sequence of dim = 3 with
    ``call.S`` streams over the ``nd_tiles`` row tiles -- the weight gradients through stpde_jet_wgrad_nd /
    stpde_jet_tan0_reduce_nd, which add the row sums of tangent adjoint k to raw-input column k for the axes k < dim only
    (column k >= dim is a latent channel there) -- and the d latent calls of the value path on the value-stream adjoints."""
    if "ws" in saved:
        return _backward_chunk_c(call, packs, packs16, saved, jets_bar, dw_flat, dlatent, pbar, after_dlatent)
    plan, cfg, S = call.plan, call.cfg, call.S
    L, st = _lib.lib(), stream_ptr()
    Pc, p0, nd = saved["Pc"], saved["p0"], plan.dim != 3
    nd_jet = nd and call.S_out > 1
    nt = _chunk_tiles(call, Pc)

    def wgrad(d, SP, abar_out, in_pre, tanc0, dw, cw_):
        """the weight gradient of one layer; a derivative request on a 1- / 2-d grid names its coordinate axes"""
        if nd_jet:
            return L.stpde_jet_wgrad_nd(C.byref(d), SP, ptr(abar_out), ptr(in_pre), ptr(X), ptr(tanc0), ptr(dw), ptr(cw_),
                                        plan.dim, st)
        return L.stpde_jet_wgrad(C.byref(d), SP, ptr(abar_out), ptr(in_pre), ptr(X), ptr(tanc0), ptr(dw), ptr(cw_), st)

    X, bufs, z0 = saved["X"], saved["bufs"], saved["z0"]
    coef, cell, cw = (saved.get(k) for k in ("coef", "cell", "cw"))
    dev = X.device
    pv = plan.pack_view
    SP0, split0, need_wgrad = call.SP0, call.split0, dw_flat is not None
    # adjoint of the fc5 output rows (overwrites the forward's out_pre buffer)
    if nd_jet:
        with _timed("reduce_nd_jet_bwd"):
            check(L.stpde_lig_reduce_nd_jet_bwd(C.byref(call.cfg_out), S, plan.dim, Pc, nt, plan.cout,
                                                C.c_void_p(jets_bar.data_ptr() + 4 * p0), jets_bar.shape[2], ptr(coef),
                                                ptr(bufs[5]), st))
    elif nd:
        with _timed("reduce_nd_bwd"):
            check(L.stpde_lig_reduce_nd_bwd(plan.dim, Pc, nt, plan.cout, C.c_void_p(jets_bar.data_ptr() + 4 * p0),
                                            jets_bar.shape[2], ptr(saved["roww"]), ptr(bufs[5]), st))
    else:
        with _timed("reduce_bwd"):
            check(L.stpde_lig_reduce_bwd(C.byref(call.cfg_out), S, Pc, plan.cout, C.c_void_p(jets_bar.data_ptr() + 4 * p0),
                                         jets_bar.shape[2], ptr(coef), ptr(bufs[5]), st))
    # layer-0 adjoint: the value stream as fragment blocks; the three tangent streams only as per-tile row sums (their
    # layer-0 "input" is the constant column W0[:, d], so only sum_rows matters): 32 + 6 KB per tile instead of 128 KB
    MT0 = plan.layers[0]["MT"]
    adj = _alloc(_backward_buffers(call, Pc), dev)
    # the value-stream-only layer-0 adjoint goes over the z0 stash (same shape; each lane reads before it writes); bf16 mode:
    # a packed ADJOINT buffer (bf16 blocks) of its own
    abar0, tan0 = adj.get("abar0x", adj.get("abar0", z0)), adj.get("tan0")
    # fc5 -> fc4 -> fc3 input gradients in one kernel (adjoints of layers 4 and 3 feed the next GEMM from the registers).
    # Order: wgrad_5 (needs the pre-activations of fc4's output intact), the chain (abar4 in place; abar3 / abar2 into
    # fresh buffers because wgrad_4 / wgrad_3 still need the pre-activations they would overwrite), wgrad_4, wgrad_3.
    # abar[l]: where the adjoint of layer l's output rows lives once it exists -- over the stash, or in a buffer of its own
    abar = {l: adj.get("abar%dx" % l, bufs[l]) for l in range(1, 6)}
    for l in range(5, 0, -1):
        lay = plan.layers[l]
        w16 = packs16.get((l, "WhT")) if packs16 else None
        d = _layer_desc(call, nt, lay, cfg, l == 1, call.nsplit if w16 is not None else 0, _pk(call, l, l - 1))
        # weight gradient: same operand mode as the layer kernels (``wgrad_split = False`` keeps it on exact-fp32 MFMA in
        # "fp32x3" mode, for A/B timing); only the wide layers, MT >= 8, have bf16-pipe weight-gradient kernels --
        # flagging a narrow layer would take it off its per-wave kernel
        dwg = _layer_desc(call, nt, lay, cfg, l == 1, (call.nsplit if call.wgrad_split or call.nsplit == 1 else 0)
                          if (w16 is not None and lay["MT"] >= 8) else 0, _pk(call, l, -1) & 5)
        if (l == 1 and need_wgrad and split0 and w16 is not None and abar0 is not z0
                and call.fc1_fused and L.stpde_jet_fc1_bwd_supported(C.byref(d))):
            # bf16 mode, reference width (round 5): weight gradient + input gradient of the first hidden layer in ONE kernel
            # (csrc/jet_fc1_bwd.hip: one read of the adjoint tile, one activation-jet evaluation per z0 element)
            with _timed("layer1_bwd"):
                check(L.stpde_jet_fc1_bwd(C.byref(d), ptr(abar[1]), ptr(w16), ptr(z0), ptr(pv(packs, 0, "tanc")), ptr(cw),
                                          ptr(X), ptr(abar0), ptr(tan0), ptr(_dw_slice(call, dw_flat, 1)), ptr(pbar), st))
            continue
        if (l == 2 and need_wgrad and call.fc2_fused and not nd and w16 is None
                and L.stpde_jet_fc2_bwd_supported(C.byref(dwg))):
            # exact fp32, reference width: weight gradient + input gradient of the second hidden layer in ONE kernel
            # (csrc/jet_fc2_bwd.hip: abar2 and the stash of fc1's rows read once, their activation jets evaluated once)
            with _timed("layer2_bwd"):
                check(L.stpde_jet_fc2_bwd(C.byref(dwg), ptr(abar[2]), ptr(pv(packs, 2, "WhT")), ptr(bufs[1]), ptr(X), ptr(cw),
                                          ptr(abar[1]), ptr(_dw_slice(call, dw_flat, 2)), ptr(pbar), st))
            continue
        if need_wgrad:
            with _timed("layer%d_wgrad" % l):
                check(wgrad(dwg, S, abar[l], bufs[l - 1] if l > 1 else saved["z0"], pv(packs, 0, "tanc"),
                            _dw_slice(call, dw_flat, l), cw))
        if call.tail and l >= 3:
            if l == 5:
                arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
                pk_tail = (call.packed_mask >> 2) & 1
                w16s = (C.c_void_p * 3)(packs16[(3, "WhT")].data_ptr(), packs16[(4, "WhT")].data_ptr(), None) \
                    if pk_tail else None
                with _timed("tail_dgrad"):
                    check(L.stpde_jet_tail_bwd_p(C.byref(cfg), nt, plan.nf // 16, ptr(bufs[5]),
                                                 arr([pv(packs, k, "WhT") for k in (3, 4, 5)]),
                                                 arr([bufs[2], bufs[3], bufs[4]]), arr([abar[2], abar[3], abar[4]]),
                                                 ptr(cw), ptr(pbar), 3 if pk_tail else 0, w16s, st))
            continue
        if l > 1 and abar[l - 1] is not bufs[l - 1]:       # into a fresh buffer: the stash stays intact
            with _timed("layer%d_dgrad" % l):
                check(L.stpde_jet_layer_bwd_to(C.byref(d), ptr(abar[l]), ptr(pv(packs, l, "WhT")), ptr(bufs[l - 1]),
                                               ptr(abar[l - 1]), ptr(cw), ptr(pbar), ptr(w16), st))
            continue
        with _timed("layer%d_dgrad" % l):
            check(L.stpde_jet_layer_bwd(C.byref(d), ptr(abar[l]), ptr(pv(packs, l, "WhT")),
                                        ptr(bufs[l - 1]) if l > 1 else None, ptr(X), ptr(pv(packs, 0, "Ws")),
                                        ptr(pv(packs, 0, "tanc")), ptr(abar0), ptr(cw), ptr(pbar), ptr(w16),
                                        ptr(tan0) if l == 1 else None, ptr(z0) if l == 1 else None, st))
    if need_wgrad:
        lay = plan.layers[0]
        # (bf16 mode: the adjoint is a packed ADJOINT buffer and the contraction over the rows runs on the bf16 MFMA)
        d = _layer_desc(call, nt, lay, cfg, False, call.packed_mask & 1, _pk(call, 0, -1) & 4)
        dw0 = _dw_slice(call, dw_flat, 0)
        with _timed("layer0_wgrad"):
            if split0:
                d.cfg = call.cfg_val      # value stream x raw input (the S = 1 weight-gradient kernels)
                check(L.stpde_jet_wgrad(C.byref(d), 1, ptr(abar0), None, ptr(X), None, ptr(dw0), None, st))
                if nd_jet:
                    check(L.stpde_jet_tan0_reduce_nd(nt, MT0, ptr(tan0), ptr(dw0), plan.dw_off[0][2], int(call.det), plan.dim, st))
                else:
                    check(L.stpde_jet_tan0_reduce(nt, MT0, ptr(tan0), ptr(dw0), plan.dw_off[0][2], int(call.det), st))
            else:
                check(wgrad(d, SP0, abar0, None, None, dw0, cw))
    if dlatent is not None:
        xd = XbarDesc()
        xd.ntiles, xd.nlayers, xd.C = nt, 5, plan.cin
        xd.n1, xd.n2 = (1, 1) if nd else call.grid_shape[1:3]      # (read by the atomic scatter only)
        ab = (C.c_void_p * 5)()
        wt = (C.c_void_p * 5)()
        for l in range(5):
            xd.MT[l] = plan.layers[l]["MT"]
            xd.SP[l] = (1 if split0 else SP0) if l == 0 else S
            xd.packed[l], xd.S[l] = (call.packed_mask >> l) & 1, (S if l else 1)
            ab[l] = (abar0 if l == 0 else abar[l]).data_ptr()
            wt[l] = pv(packs, l, "WsL").data_ptr()
        if not (nd or call.det_dlatent):
            with _timed("xbar_scatter"):
                check(L.stpde_lig_xbar_scatter(C.byref(xd), ab, wt, ptr(cell), ptr(dlatent), st))
        else:
            # deterministic: per-row adjoints (dim = 1, 2, 4: and the cell id of every point), then a per-node sum in fixed order
            # over the cell-sorted points -- the library calls of the one-call path, scratch allocated OUTSIDE the timed region
            # (with torch.sort / index_add_ / cumsum in here the caching allocator's stalls showed up as a 60-75 ms "kernel")
            sc = _alloc(_dlatent_buffers(call, Pc), dev)
            xrows, perm, start, tmp = (sc[k] for k in ("xrows", "perm", "start", "sort_tmp"))
            cell = sc.get("cell", cell)         # (dim = 1, 2, 4: the forward keeps no cell ids)
            with _timed("xbar_scatter"):
                check(L.stpde_lig_xbar_rows(C.byref(xd), ab, wt, ptr(xrows), st))
                if nd:
                    gd = _gather_nd_desc(call, dlatent, Pc, p0, nt)
                    check(L.stpde_lig_cell_nd(C.byref(gd), ptr(saved["pts_c"]), ptr(cell), st))
                check(L.stpde_lig_cell_sort(Pc, start.numel() - 1, ptr(cell), ptr(perm), ptr(start), ptr(tmp), tmp.numel(), st))
                if nd:
                    check(L.stpde_lig_dlatent_reduce_nd(plan.dim, call.B, (C.c_int * 4)(*call.grid_shape), plan.cin, ptr(xrows),
                                                        ptr(perm), ptr(start), ptr(dlatent), st))
                else:
                    check(L.stpde_lig_dlatent_reduce(*((call.B,) + call.grid_shape), plan.cin, ptr(xrows), ptr(perm),
                                                     ptr(start), ptr(dlatent), st))
    if after_dlatent is not None:      # per-kernel (profiling) path: weight gradients first, nothing left to overlap
        after_dlatent()


# {"dlatent": f(tensor) -> work | None, "dw": f(tensor) -> work | None}: collectives of the point-sharded step, started from
# inside the backward (set / cleared by train_step.sharded_step; the first LigJetFunction.backward of the step consumes them).
sync_hooks = None

# True while train_step.sharded_step runs the FORWARD of a step whose backward will install ``sync_hooks`` (the hooks themselves
# are set only around loss.backward(), i.e. after LigJetFunction.forward has made its memory plan): the plan then budgets the
# dgrad-first scratch of the last chunk (with the test on ``sync_hooks`` alone the term was never counted and a
# step near the limit failed with an out-of-memory error in the backward instead of shrinking its chunks).
expect_two_phase = False

def _chunk_ranges(call, P):
    """[(first point, points)] of the launch chunks: ``call.chunk`` points each."""
    return [(p0, min(call.chunk, P - p0)) for p0 in range(0, P, call.chunk)]

stats = {"recompute_steps": 0}     # calls whose backward rebuilt the stash chunk by chunk (memory plan below)


def _free_bytes(device):
    """Device memory this process can still get: free on the device + what torch's caching allocator holds unused."""
    free, _ = torch.cuda.mem_get_info(device)
    return free + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def _table_bytes(table):
    return sum(n * dtype.itemsize for _, n, dtype in table)


def _per_point_bytes(call):
    """(forward stash, backward scratch) bytes per query point of the jet path: the chunk's buffer tables (``_forward_buffers``
    with a stash; ``_backward_buffers`` + ``_dlatent_buffers``, the sort's temporary storage at the plan's estimate) for
    ``call.mult`` points -- whole tiles, a point owns 8 of a tile's 16 rows, on a dim = 1, 2, 4 grid 2^dim -- over those points.
    Not counted: the up to 3 + 1 padding tiles of a chunk on such a grid (``nd_tiles``; the plan keeps 15 % of headroom), and
    ``start``, one int per grid node whatever the chunk."""
    bwd = [b for b in _backward_buffers(call, call.mult) + _dlatent_buffers(call, call.mult, True) if b[0] != "start"]
    return _table_bytes(_forward_buffers(call, call.mult)) // call.mult, _table_bytes(bwd) // call.mult


def _two_phase_bytes(call):
    """extra bytes per point of the dgrad-first order (last chunk of a sharded_step backward): two more adjoint buffers"""
    return _table_bytes(_two_phase_buffers(call, call.mult)) // call.mult


# Device-memory budget of ONE jet call in bytes (None = whatever the device has free): a call whose forward stash + backward
# scratch would exceed it keeps no stash and rebuilds it chunk by chunk in the backward (+1 forward of compute), with the
# chunk sized so that one chunk's stash + scratch fits half of the budget.  ``STPDE_MEM_BUDGET_GB`` / ``set_memory_budget``
# / ``lig_jets(..., memory_budget=bytes)``: how a rank with less than the 142 GB the default 2^20-point step peaks at
#  runs the same configuration.
memory_budget = (lambda v: int(float(v) * 2 ** 30) if v else None)(os.environ.get("STPDE_MEM_BUDGET_GB"))


def set_memory_budget(nbytes):
    """Budget in bytes for the stash + scratch of one jet call (None: the free device memory); returns the previous one."""
    global memory_budget
    prev, memory_budget = memory_budget, (None if nbytes is None else int(nbytes))
    return prev


def _avail_bytes(call, device):
    free = _free_bytes(device)
    return free if call.budget is None else min(free, call.budget)


def _stash_bytes(call, P):
    fwd, bwd = _per_point_bytes(call)
    last = _chunk_ranges(call, P)[-1][1]
    # (the dgrad-first scratch of the last chunk only when the point-sharded step's hooks are / will be installed: ADVICE r4, r5)
    two = _two_phase_bytes(call) if (sync_hooks or expect_two_phase) else 0
    return P * fwd + min(P, call.chunk) * bwd + last * two


def _recompute_chunk(call, device):
    """Largest power-of-two chunk whose stash + backward scratch takes at most half of the available memory."""
    fwd, bwd = _per_point_bytes(call)
    two = _two_phase_bytes(call) if (sync_hooks or expect_two_phase) else 0
    n = max(1, int(0.5 * _avail_bytes(call, device) / (fwd + bwd + two)))
    c = 1 << (n.bit_length() - 1)
    if call.plan.dim != 3:
        # whole value-tile passes (4 row tiles of 16 >> dim points), and at most the row tiles of the dim = 3 default chunk
        return max(call.mult, min(c, (DEFAULT_CHUNK // 2) * (16 >> call.plan.dim)))
    return max(call.mult, min(c, DEFAULT_CHUNK))


def _nd_chunk_points(call, device):
    """Default launch chunk of a query on a dim-d grid (dim = 1, 2, 4), in points: the row tiles of the dim = 3 default chunk,
    cut down (to a power of two) until one chunk's forward buffers (``_forward_buffers``: all ``call.S`` streams of the request)
    take at most half of the call's memory budget / of the free device memory."""
    tile_bytes = _table_bytes(_forward_buffers(call, call.mult, call.need_grad)) // 4      # (call.mult points: 4 row tiles)
    tiles = DEFAULT_CHUNK // 2
    fit = max(4, int(0.5 * _avail_bytes(call, device) / tile_bytes))
    tiles = min(tiles, 1 << (fit.bit_length() - 1))
    return max(call.mult, tiles * (16 >> call.plan.dim) // call.mult * call.mult)


class LigJetFunction(torch.autograd.Function):
    """jets[S, n_out, P] of the LIG+IM-NET composite; differentiable w.r.t. latent grid and IM-NET parameters.

    Reproducibility.  Run to run on the same inputs: the forward (jets, and therefore a stash rebuilt by recomputation) and
    ``d latent`` (``deterministic_dlatent``, the default: per-node gather in a fixed order) are bit-identical.  The IM-NET
    WEIGHT gradients by default are NOT: every weight-gradient kernel (k_wgrad_coop / k_wgrad_quad / k_wgrad_wave,
    csrc/jet_wgrad_impl.h) finishes with fp32 atomic adds of its workgroups' partial sums into the flat dW buffer, whose order
    varies -- they agree to fp32 summation-order rounding (a few 1e-6 relative).  ``_lib.deterministic`` (STPDE_DETERMINISTIC=1,
    round 6) sends those partial sums -- and the U-Net's, unet3d.py -- to order-independent long accumulators instead: the
    gradients are then bit-identical from run to run (exception: the adjoint of a learnable swish beta)."""

    @staticmethod
    @_lib.guarded
    def forward(ctx, call, latent, pts, act_param, *params):
        # act_param: the learnable swish beta (a tensor input so that autograd routes its gradient) or None
        packs = call.plan.pack(params)
        packs16 = call.plan.pack_bf16(packs, call.nsplit) if call.bf16 else None
        # dim = 4 derivative request: the tangent constants of the passes over the triples other than (0, 1, 2)
        tancs = call.plan.pack_tanc(params, [ps.triple for ps in call.passes if ps.triple != ND4_TRIPLES[0]])
        P = pts.shape[0]
        jets = torch.empty(call.S_out, call.plan.cout, P, device=pts.device)
        # grad mode is always off inside Function.forward and ctx.needs_input_grad ignores torch.no_grad(): whether a
        # backward can follow was decided by lig_jets() before apply()
        need_grad = call.need_grad and any(ctx.needs_input_grad)
        # Memory plan (VERDICT r2 #9 / ADVICE r2): the activation stash of ALL chunks lives until the backward.  When it
        # would not fit the free device memory (or an allocation fails half way), the forward keeps NO stash and the
        # backward re-runs the forward kernels chunk by chunk right before each chunk's backward (the same kernels on the
        # same inputs rebuild the same stash bit for bit -- the same kernels because the rebuild reads the SAME frozen record):
        # +1 forward of compute, memory bounded by one chunk.
        limit = 0.85 * _avail_bytes(call, pts.device)
        if need_grad and not call.recompute and _stash_bytes(call, P) > limit:
            # the stash of all chunks is what it is, the backward scratch is per launch chunk: smaller chunks (down to 2^16
            # points: below that the launches get short) before giving up the stash (configs[4], S = 10 at 2^20 points: 187 GB
            # of stash + 69 GB of scratch per 2^20-point chunk, 17 GB per 2^18-point chunk)
            asked = call.chunk
            while call.chunk > (1 << 16) and _stash_bytes(call, P) > limit:
                call.plan_chunk(call.chunk // 2)
            if _stash_bytes(call, P) > limit:
                call.plan_chunk(asked)
        recompute = need_grad and (call.recompute or _stash_bytes(call, P) > limit)
        if recompute:
            call.plan_chunk(min(call.chunk, _recompute_chunk(call, pts.device)))
        saved = []
        oom = False
        try:
            for p0, n in _chunk_ranges(call, P):
                s = _forward_chunk(call, packs, packs16, latent, pts[p0:p0 + n], jets, p0, need_grad and not recompute, tancs)
                if need_grad and not recompute:
                    saved.append(s)
        except torch.OutOfMemoryError:
            if not need_grad or recompute:
                raise
            oom = True
        if oom:
            # OUTSIDE the except block: while it runs, the exception's traceback pins the failed _forward_chunk
            # frame and its half-allocated buffers, so empty_cache() could not release them and the retry was sized against
            # less memory than there is
            saved, s = [], None
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            recompute = True
            call.plan_chunk(min(call.chunk, _recompute_chunk(call, pts.device)))
            for p0, n in _chunk_ranges(call, P):
                _forward_chunk(call, packs, packs16, latent, pts[p0:p0 + n], jets, p0, False, tancs)
        stats["recompute_steps"] += int(recompute)
        ctx.recompute = recompute
        ctx.call, ctx.packs, ctx.packs16, ctx.saved = call, packs, packs16, saved
        ctx.inputs = (latent, pts) if need_grad else None   # to rebuild the stash if backward runs again (retain_graph)
        ctx.n_params = len(params)
        ctx.prm_shape = act_param.shape if act_param is not None else None
        ctx.lat_shape = latent.shape
        ctx.params = params
        ctx.used = recompute     # nothing stashed: the backward rebuilds every chunk's stash itself
        return jets

    @staticmethod
    @_lib.guarded
    def backward(ctx, jets_bar):
        call = ctx.call
        rebuild = ctx.used
        if rebuild and ctx.inputs is None:
            raise RuntimeError("LigJetFunction.backward: no stash was kept for this call")
        # rebuild: either the memory plan kept no stash (ctx.recompute), or this is a second backward after
        # backward(retain_graph=True) -- the dgrad kernels overwrote the stash in place.  The forward kernels of a chunk are
        # run again right before its backward (same kernels, same inputs -> the same stash, bit for bit).
        ctx.used = True
        jets_bar = jets_bar.contiguous()
        dev = jets_bar.device
        need_wgrad = any(ctx.needs_input_grad[4:])
        need_lat = ctx.needs_input_grad[1]
        # (deterministic mode: long accumulators -- order-independent integer sums -- turned into fp32 after the last chunk)
        dw_flat = torch.zeros(_AW(call) * call.plan.n_dw, device=dev) if need_wgrad else None
        dlatent = torch.zeros(ctx.lat_shape, device=dev) if need_lat else None
        pbar = torch.zeros(_lib.PBAR_SLOTS, device=dev) if ctx.needs_input_grad[3] else None
        # Point-sharded multi-GPU step (train_step.sharded_step sets ``sync_hooks``): the all-reduce of the partial d latent is
        # started as soon as the LAST chunk has finished it and runs behind that chunk's weight gradients (dgrad-first order);
        # the IM-NET gradients are all-reduced in place in their flat buffer before they are unpacked.
        hooks = sync_hooks if (sync_hooks and not sync_hooks.get("used")) else None
        works = []

        def start_dlatent_sync():
            if hooks and need_lat and hooks.get("dlatent"):
                works.append(hooks["dlatent"](dlatent))
                hooks["dlatent_done"] = dlatent      # WHICH tensor is summed over ranks (train_step._SumGradAcrossRanks)

        chunks = ctx.saved
        if rebuild:
            latent, pts = ctx.inputs
            scratch = torch.empty(call.S_out, call.plan.cout, pts.shape[0], device=pts.device)
            chunks = _chunk_ranges(call, pts.shape[0])
        for k, s in enumerate(chunks):
            if rebuild:     # s = (first point, points): the forward kernels of the chunk, right before its backward
                s = _forward_chunk(call, ctx.packs, ctx.packs16, latent, pts[s[0]:s[0] + s[1]], scratch, s[0], True)
            _backward_chunk(call, ctx.packs, ctx.packs16, s, jets_bar, dw_flat, dlatent, pbar,
                            start_dlatent_sync if (hooks and k == len(chunks) - 1) else None)
            s["bufs"] = s["z0"] = None  # release the stash chunk by chunk
        s, ctx.saved = None, []
        grads = [None] * ctx.n_params
        if call.det and need_wgrad:
            acc, dw_flat = dw_flat, torch.empty(call.plan.n_dw, device=dev)
            check(_lib.lib().stpde_det_finalize(ptr(acc), call.plan.n_dw, ptr(dw_flat), stream_ptr()))
            del acc
        if hooks:
            hooks["used"] = True
        if hooks and need_wgrad and hooks.get("dw"):
            works.append(hooks["dw"](dw_flat))
            if pbar is not None:                      # adjoint of the learnable swish beta: same treatment
                works.append(hooks["dw"](pbar))
            hooks["dw_done"] = True
        for wk in works:
            if wk is not None:
                wk.wait()
        if need_wgrad:
            g = call.plan.unpack_grads(dw_flat, ctx.params)
            grads = [gi if need else None for gi, need in zip(g, ctx.needs_input_grad[4:])]
        dprm = pbar.sum().reshape(ctx.prm_shape) if pbar is not None else None
        return (None, dlatent, None, dprm) + tuple(grads)


def activation_name(module):
    """Map an activation module to the library's enum name; returns (name, param) or None if unknown."""
    import torch.nn as nn
    from . import nonlinearities
    if isinstance(module, nonlinearities.Swish):
        return "swish", module.beta
    table = [(nn.Tanh, "tanh"), (nn.ReLU, "relu"), (nn.Softplus, "softplus"), (nn.ELU, "elu"),
             (nn.LeakyReLU, "leakyrelu")]
    for cls, name in table:
        if type(module) is cls:
            if name == "softplus" and (module.beta != 1 or module.threshold != 20):
                return None
            if name == "elu" and module.alpha != 1.0:
                return None
            if name == "leakyrelu" and module.negative_slope != 0.01:
                return None
            return name, 0.0
    return None


# Module-level settings (plain attributes: tests set them with monkeypatch; none of them is read from the environment since
# round 6 -- the environment selects only the operand mode, the memory budget and the A/B switch of the fused fc1 backward).
# They are the DEFAULTS of a call: JetCall.make reads each of them (and ``_lib.deterministic``) once, when lig_jets() is called,
# and every later stage of that call -- its backward and a stash rebuild included -- reads the record.  Setting one between two
# calls works as ever; setting one between a call's forward and its backward has no effect on that call.
# d latent: per-node gather in a fixed order (bit-reproducible, like the reference's CPU index_put_ accumulate); False = the
# fp32-atomic scatter.
deterministic_dlatent = True
# forward-only value queries use the value-tile kernels (4 row tiles per weight pass); False = one tile per pass
value_tiles = True
# layer-0 tangent-stream adjoints as per-tile row sums (False: full fragment blocks)
tan0_rowsum = True
wgrad_split = True
packed_stash = True
# forward of fc3 -> fc4 -> fc5 in one kernel (False: three per-layer kernels)
fused_tail = True

# ``force_recompute = True``: never keep the stash, always rebuild it in the backward (tests; also what the memory plan of
# LigJetFunction.forward switches to on its own when the stash does not fit)
force_recompute = False


def fc1_fused_enabled():
    """bf16 mode: the fused backward of the first hidden layer (csrc/jet_fc1_bwd.hip) is used where the library serves it.
    STPDE_FC1_FUSED=0 (read once per call, by JetCall.make: tests switch it inside one process) runs the input gradient and the weight gradient of
    that layer as two kernels -- the A/B reference of tests/test_gpu_bf16_kernel_variants.py."""
    return os.environ.get("STPDE_FC1_FUSED", "1") != "0"


# Exact fp32, reference width: fc2's weight gradient + input gradient as one kernel (csrc/jet_fc2_bwd.hip; same bits as the two
# kernels in deterministic mode).  None = the caller's default: a direct jet call keeps the two kernels -- the instantiations the
# parity fixtures of tests/test_gpu_reference_fixtures.py pin -- and the training step (train_step.sharded_step, what bench.py
# times) turns it on for its own calls; True / False = for every call.  ``_lib.tune("fc2_bwd_fused", 2)`` overrides it: two kernels.
fc2_fused = None


def fc2_fused_enabled():
    """``fc2_fused`` and the library switch, read once per call by JetCall.make; handed to the one-call entry point as
    STPDE_F_FC2_FUSED and followed by the per-kernel driver, which names the launch ``layer2_bwd``."""
    return bool(fc2_fused) and _lib.tune_value("fc2_bwd_fused") != 2


DEFAULT_CHUNK = 1 << 20   # query points per launch chunk (per-chunk backward scratch: ~50 GB at 2^20; measured on
                          # MI355X: 2^17 / 2^18 / 2^19 / 2^20 points per chunk -> 459.8 / 458.7 / 455.5 / 454.3 ms per step)

# MFMA operand precision of the hidden-to-hidden GEMMs of the wide layers: "fp32" (exact-fp32 MFMA, the default and
# the parity path) or "bf16" (BASELINE config 4: bf16 operands, fp32 accumulation, everything else fp32).
mlp_precision = os.environ.get("STPDE_MLP_PRECISION", "fp32")


def set_mlp_precision(precision):
    """Select "fp32" or "bf16" MFMA operands for subsequent HIP jet calls; returns the previous setting."""
    global mlp_precision
    if precision not in ("fp32", "bf16", "fp32x3"):
        raise ValueError("mlp precision must be 'fp32', 'bf16' or 'fp32x3'")
    prev, mlp_precision = mlp_precision, precision
    return prev


_ND_VALUE_ONLY = "dim = %d queries run in HIP as value-only forward passes (no coordinate derivatives)"


def lig_jets(imnet, latent_grid, query_pts, xmin, xmax, first=True, pairs=(), chunk_points=None, combo=None,
             precision=None, memory_budget=None):
    """HIP evaluation of y and its coordinate derivatives.

    imnet: implicit_net.ImNet (dim=3); latent_grid [b, n0, n1, n2, c]; query_pts [b, p, 3].
    Returns (jets [S, n_out, b*p] with S = 1 + 3*first + len(padded pairs), padded_pairs).
    Stream order: value, d/dq_0, d/dq_1, d/dq_2, then d2/dq_a dq_b per pair.
    combo = {(a, b): alpha}: instead of one stream per pair, ONE combined second-order stream
    sum alpha_ab d2y/dq_a dq_b is carried through the network (S = 5); returned pairs = ["combo"].
    precision: "fp32" | "bf16" MFMA operands of the wide layers (None = module setting ``mlp_precision``).
    memory_budget: bytes the stash + backward scratch of this call may take (None = module setting ``memory_budget``, whose
    None means the free device memory); above it the backward recomputes the forward chunk by chunk (``_recompute_chunk``).

    imnet.dim = 1, 2 or 4 (latent_grid [b, n_1..n_d, c], query_pts [b, p, d], d + c + 1 <= 36): VALUE queries --
    first=False, pairs=(), no combo; fp32 or fp32x3 operands.  Returns (jets [1, n_out, b*p], []).  By default nothing may
    need a gradient (call it under ``torch.no_grad()`` or with no input / parameter requiring grad).  With ``nd_backward``
    (``set_nd_backward(True)`` / STPDE_ND_BACKWARD=1) the result is differentiable w.r.t. the latent grid and the IM-NET
    parameters (a learnable swish beta included) for in_features <= 32: the S = 1 layer / weight-gradient kernels of the
    dim = 3 value path between stpde_lig_reduce_nd_bwd, stpde_lig_cell_nd and stpde_lig_dlatent_reduce_nd.  d latent on these
    grids is always the deterministic per-node sum (``deterministic_dlatent = False`` is ignored; there is no atomic variant),
    the one-call pipeline (``use_pipeline``) stays dim = 3 only, and there are no coordinate derivatives and no point
    gradients (query_pts is detached).  Everything else on such grids is the composed formulation of local_implicit_grid.py.

    imnet.dim = 1 or 2 with ``nd_jets`` (``set_nd_jets(True)`` / STPDE_ND_JETS=1): ``first`` / ``pairs`` (indices < dim) are
    served as well, for calls that need no gradient: stpde_lig_coef_nd and stpde_lig_reduce_nd_jet_fwd around the layer
    kernels in the request's stream set.  Returns (jets [1 + 3 + len(padded pairs), n_out, b*p], padded pairs) in the
    dim = 3 stream order; the streams d/dq_k, k >= dim, are +0.0.  Refused: ``combo``, a call that needs a gradient, bf16
    operands, dim = 4.

    imnet.dim = 4 with ``nd4_jets`` (``set_nd4_jets(True)`` / STPDE_ND4_JETS=1; independent of ``nd_jets``): ``first`` /
    ``pairs`` (distinct, indices < 4, any number of the ten) are served for calls that need no gradient, as up to four passes of
    the layer kernels over axis triples (``nd4_passes``) between one stpde_lig_gather_nd / stpde_lig_coef_nd4 per chunk and one
    stpde_lig_reduce_nd4_jet_fwd per pass.  Returns (jets [1 + 4 + len(pairs), n_out, b*p], the pairs as asked): value,
    d/dq_0 .. d/dq_3, then the pairs in the caller's order, no padding.  Refused: ``combo``, a call that needs a gradient
    (whatever the other switches say), bf16 operands, in_features > 31.

    ... and with ``nd_jet_backward`` on top (``set_nd_jet_backward(True)`` / STPDE_ND_JET_BACKWARD=1; inert without
    ``nd_jets``, independent of ``nd_backward``): such a call may need a gradient -- the jets are differentiable w.r.t. the
    latent grid and the IM-NET parameters (a learnable swish beta included), which is what training with an equation loss on
    a (t, x) or (x, y) model takes.  Backward: stpde_lig_reduce_nd_jet_bwd, the per-kernel layer / weight-gradient sequence
    of dim = 3 in the call's stream set (weight gradients through stpde_jet_wgrad_nd / stpde_jet_tan0_reduce_nd: the tangent
    streams of the axes k >= dim add nothing to the weight columns of latent channels), and the d latent calls of the value
    path -- always the deterministic per-node sum.  A cotangent on the streams d/dq_k, k >= dim, is dropped, whatever it
    holds.  Envelope: dim 1 or 2, in_features <= 32, fp32 or fp32x3 operands, pairs only, no point gradients (query_pts is
    detached), the per-kernel driver, a single device.  Refused with NotImplementedError, never composed behind the caller's
    back: ``combo``, bf16 operands, dim = 4, in_features > 32, and a call made while the point-sharded step's ``sync_hooks`` /
    ``expect_two_phase`` are set (the one-call pipeline, ``use_pipeline``, stays dim = 3 only: such a call never takes it).
    ``force_recompute``, a stash that does not fit and a second backward after ``retain_graph=True`` work as on dim = 3.
    """
    if not (latent_grid.is_cuda and query_pts.is_cuda):
        raise RuntimeError("the HIP jet path needs CUDA/HIP tensors (no CPU fallback)")
    dim = imnet.dim
    wants_jets = bool(first or len(pairs) or combo)
    if dim == 3:
        if latent_grid.dim() != 5 or query_pts.dim() != 3 or query_pts.shape[-1] != 3:
            raise ValueError("lig_jets expects latent_grid [b,n0,n1,n2,c] and query_pts [b,p,3]")
    elif dim in ND_VALUE_DIMS:
        if latent_grid.dim() != dim + 2 or query_pts.dim() != 3 or query_pts.shape[-1] != dim:
            raise ValueError("lig_jets expects latent_grid [b,n_1..n_%d,c] and query_pts [b,p,%d]" % (dim, dim))
        if wants_jets and dim not in ND_JET_DIMS and dim != 4:      # (dim = 4: decided with the call's frozen switch, below)
            raise NotImplementedError(_ND_VALUE_ONLY % dim)
        if min(latent_grid.shape[1:-1]) < 2:
            raise ValueError("every axis of the latent grid needs at least 2 nodes")
    else:
        raise ValueError("lig_jets: dim = %r (3; value-only queries: 1, 2, 4)" % (dim,))
    if latent_grid.dtype != torch.float32 or query_pts.dtype != torch.float32:
        raise ValueError("lig_jets is fp32 only")
    an = activation_name(imnet.activ)
    if an is None:
        raise NotImplementedError("activation %r is not implemented in the HIP jet path" % (imnet.activ,))
    act, prm = an
    prm_tensor = None
    if act == "swish":
        prm_tensor = prm          # learnable beta: a tensor input of the autograd function (its adjoint comes from
        prm = float(prm.detach())  # the dgrad epilogues); the kernels take the current value as a launch constant
    B, N = query_pts.shape[0], query_pts.shape[1]
    if latent_grid.shape[0] != B:
        raise ValueError("batch mismatch between latent_grid and query_pts")
    plan = ImNetPlan.get(imnet.dim, imnet.in_features, imnet.out_features, imnet.nf)
    if latent_grid.shape[-1] != plan.cin:
        raise ValueError("latent channels != imnet.in_features")
    lat = latent_grid.contiguous()
    params = []
    for k in range(6):
        params += [imnet.fc[k].weight, imnet.fc[k].bias]
    need_grad = torch.is_grad_enabled() and (lat.requires_grad or any(p.requires_grad for p in params)
                                             or (prm_tensor is not None and prm_tensor.requires_grad))
    grid_shape = tuple(latent_grid.shape[1:-1])
    call = JetCall.make(plan, act, prm, first, pairs, combo, precision, grid_shape, cached_box_constants(grid_shape, xmin, xmax),
                        memory_budget, B, N, chunk_points, need_grad)
    if dim != 3 and wants_jets:
        # dim = 1, 2 / dim = 4: whether derivative requests are served is one of the call's frozen switches (dim = 4 with
        # ``nd4_jets`` off was refused by JetCall.make, which cannot lay such a request out)
        if not (call.nd4_jets if dim == 4 else call.nd_jets):
            raise NotImplementedError(_ND_VALUE_ONLY % dim)
        if combo:
            raise NotImplementedError("dim = %d: the combined second-order stream is dim = 3 only (ask for the pairs)" % dim)
        if any(not (0 <= a < dim and 0 <= b < dim) for a, b in pairs):
            raise ValueError("dim = %d: second-derivative pairs %r name an axis the grid does not have" % (dim, list(pairs)))
        if need_grad:
            if dim == 4 or not call.nd_jet_backward:
                raise NotImplementedError("dim = %d coordinate derivatives run in HIP as forward passes only: call under "
                                          "torch.no_grad() or without inputs / parameters that require grad" % dim)
            # the training backward of the derivative streams runs on one device (and kernel by kernel: ``JetCall.pipeline`` is
            # dim = 3 only); the point-sharded step is refused when the call is made
            if sync_hooks or expect_two_phase:
                raise NotImplementedError("dim = %d: the training backward of coordinate derivatives does not serve the "
                                          "point-sharded step (sync_hooks / expect_two_phase)" % dim)
    P = B * N
    if P == 0:   # empty query set: nothing to launch (the reference returns an empty [b, 0, o] tensor as well)
        return torch.zeros(call.S_out, plan.cout, 0, device=query_pts.device), call.pairs
    if dim != 3 and need_grad:
        if not (call.nd_jet_backward if wants_jets else call.nd_backward):
            raise NotImplementedError("dim = %d queries run in HIP as value-only forward passes: call under torch.no_grad() or "
                                      "without inputs / parameters that require grad" % dim)
        if plan.cin > ND_TRAIN_MAX_CHANNELS:
            raise NotImplementedError("dim = %d training backward in HIP takes in_features <= %d (the latent-adjoint kernel "
                                      "serves two 16-channel tiles)" % (dim, ND_TRAIN_MAX_CHANNELS))
    if dim != 3 and not chunk_points:
        # (the default chunk of these grids depends on the device's free memory, which the device-free constructor cannot ask for)
        call.plan_chunk(_nd_chunk_points(call, query_pts.device))
    pts = query_pts.detach().reshape(P, dim).contiguous()
    pad = call.P_pad - P
    if pad:
        pts = torch.cat([pts, pts[-1:].expand(pad, 3)], 0)
    jets = LigJetFunction.apply(call, lat, pts, prm_tensor, *params)
    if pad:
        jets = jets[:, :, :P]
    return jets, call.pairs
