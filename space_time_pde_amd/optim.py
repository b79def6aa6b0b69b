"""Fused gradient-value clipping + Adam.

``FusedClipAdam`` is a ``torch.optim.Optimizer`` whose ``step()`` does, for ALL parameter tensors of a group in ONE HIP
kernel launch (``stpde_clip_adam_multi``; ``stpde_clip_adam`` is the single-tensor entry point), what the reference does
with ``clip_grad_value_`` followed by ``optim.Adam.step`` (experiments/rb2d/train.py:79-83): same state names (``step``,
``exp_avg``, ``exp_avg_sq``), so ``state_dict()`` / ``load_state_dict()`` interoperate with ``torch.optim.Adam``
checkpoints written by the reference.

``FusedClipSGD`` is the same for the reference's ``--optim sgd`` (train.py:220, :330-333): ``clip_grad_value_`` +
``torch.optim.SGD`` (momentum, dampening, weight decay, Nesterov) in one launch, state name ``momentum_buffer``.

Both take ``capturable=True``: step count and learning rate then live in device memory (``stpde_opt_state``), a step is
``stpde_opt_advance`` + one update launch with no host read-back and no upload, and ``train_step.GraphedStep(...,
optimizer=opt)`` replays the whole iteration -- forward, backward, clip, update -- from one HIP graph.

Everything the two have in common -- the flat buffers and their aliasing, one step count per group in device memory, what a
stream capture may and may not do, the checkpoint layout -- is ``_FusedClip``; the subclasses hold their update rule only.
"""
import ctypes as C
import math
from collections import defaultdict

import numpy as np
import torch

from . import _lib

_CHUNK = 1 << 16     # elements per block of the multi-tensor kernel
_TENSOR_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"),
                      ("bias2_sqrt", "<f4")])      # = stpde_adam_tensor
_CHUNK_DT = np.dtype([("tensor", "<i4"), ("pad", "<i4"), ("offset", "<i8")])   # = stpde_adam_chunk
_SGD_TENSOR_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("first_step", "<i4"),
                          ("pad", "<i4")])        # = stpde_sgd_tensor
_NO_GRAD_MSG = ("%s(capturable=True): a parameter of the group has no gradient.  torch's optimizers skip such a parameter "
                "and leave its step count alone; the capturable mode keeps ONE step count per group in device memory and "
                "cannot do that -- give every parameter a gradient or construct with capturable=False")


def _host_tables(rows, dtype):
    """Tensor table (``rows``: one tuple per tensor, laid out as ``dtype``) and chunk table (one ``_CHUNK``-element piece of
    one tensor per block) as host byte tensors, and the number of chunks."""
    n = dtype.names.index("n")
    chunks = [(k, 0, off) for k, r in enumerate(rows) for off in range(0, r[n], _CHUNK)]
    return (torch.from_numpy(np.array(rows, dtype=dtype).view(np.uint8)),
            torch.from_numpy(np.array(chunks, dtype=_CHUNK_DT).view(np.uint8))), len(chunks)


class _FusedClip(torch.optim.Optimizer):
    """What ``FusedClipAdam`` and ``FusedClipSGD`` share; a subclass adds its update rule: ``_ROW_DT`` / ``_NPTR`` /
    ``_ROW_TAIL`` / ``_FLAT_STATE``, ``_check_group``, ``_flat_state``, ``_init_state``, ``_loaded_step``,
    ``_sync_host_state``, ``_flat_step``, ``_host_rows``, ``_row_tensors``, ``_launch_flat`` and ``_launch_table``.

    ``flat=True`` (default): on the first step the parameters of a group are moved into ONE contiguous fp32 buffer (every
    ``p.data`` becomes a view of it, values preserved) and the state tensors are views of further buffers allocated once.  A
    step is then: gradients gathered into the flat gradient buffer (``torch._foreach_copy_``: a handful of multi-tensor
    launches; skipped for gradients that already live there, see ``gather_grads``) and ONE launch over the whole buffer -- no
    per-step table build, no host-to-device upload.  ``gather_grads()`` returns that flat gradient buffer with every
    ``p.grad`` re-pointed into it, so a data-parallel step all-reduces exactly the buffer the optimizer reads (reference:
    DDP's bucket, train_ddp.py:401-406).  The per-parameter state keeps torch's names and shapes; ``state_dict()`` returns
    plain (cloned) tensors, so checkpoints interoperate with the reference's optimizers both ways.  A group goes through the
    multi-tensor pointer-table kernel, which is also the ``flat=False`` path, for a step in which some parameter has no
    gradient or the parameters are not at the same point of their history (torch skips a parameter without a gradient; a
    flat pass could not).

    Aliasing: building the flat buffers (first ``step()`` / ``gather_grads()`` after construction, ``load_state_dict`` or
    ``add_param_group``) RE-POINTS every ``p.data`` into the new buffer.  The values are preserved, the storage is not: an
    alias of the old storage taken before that (an EMA copy made with ``p.data`` views, a captured hipGraph, a
    ``DistributedDataParallel`` bucket view) keeps pointing at memory the optimizer no longer updates.  Take such aliases
    after the first step (or after ``prepare()``), or construct with ``flat=False`` (pointer-table kernel, storages untouched).

    ``capturable=True`` adds per group one ``stpde_opt_state`` block in device memory (64-bit step count, fp64 learning rate,
    the two derived Adam scalars) and, with ``flat=False``, pointer tables that are rebuilt only when a pointer changes; a step
    is ``stpde_opt_advance`` + ONE update launch, safe to capture in a HIP graph.  All parameters of a group share the step
    count, so every parameter needs a gradient at every step.  ``group["lr"]`` stays the knob a scheduler turns: a value that
    differs from the last one pushed is written into the block (one fill launch, no synchronisation) by ``step()`` /
    ``sync_lr()`` -- never inside a stream capture, where the fill would be recorded and every replay would reset the rate."""

    def __init__(self, params, defaults):
        # ``flat`` and ``capturable`` travel in ``defaults`` (what Optimizer.__getstate__ serialises), so a deepcopy / pickle
        # of an optimizer comes back in the mode it was built with
        super().__init__(params, defaults)
        self._use_flat = defaults["flat"]
        self._reset()

    def _reset(self):
        self._flat = {}         # group index -> dict(params, P, G, offs, n, gviews, + the subclass's state buffers)
        self._cap = {}          # group index -> dict(blk, lr, key, tab, chk, nchunks, pending, keep, spare)

    @property
    def capturable(self):
        return bool(self.defaults.get("capturable", False))

    # -- checkpoints -----------------------------------------------------------------------------------------------
    def __setstate__(self, state):
        # Optimizer.load_state_dict replaces param_groups with the SAVED groups: a checkpoint written by the reference's
        # torch optimizer (train.py:390-397) has no ``clip_grad`` entry, and carries options (amsgrad, maximize, foreach,
        # ...) this optimizer does not implement -- keep this instance's clip value and refuse (``_check_group``) the options
        # that would change the update rule.
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("clip_grad", self.defaults["clip_grad"])
            group.setdefault("flat", self.defaults.get("flat", True))
            self._check_group(group)
            # a reference-written group may say capturable=False (torch's own flag): this instance's mode holds
            group["capturable"] = self.defaults.get("capturable", False)
        # loaded state tensors are fresh allocations: rebuild the flat views on the next step, and set the device step
        # counts from the loaded state
        self._reset()
        # Optimizer.__getstate__ serialises defaults / state / param_groups only: an instance that comes back from
        # copy.deepcopy or pickle takes its mode from ``defaults`` (it used to come back as flat=True)
        self._use_flat = bool(self.defaults.get("flat", getattr(self, "_use_flat", True)))

    def add_param_group(self, group):
        # flat buffers and device state are rebuilt on the next step, from the host state as a checkpoint would hold it
        # (Optimizer.__init__ comes through here before this instance has either)
        for p in self._unwritten():
            self.state[p].clear()
        super().add_param_group(group)
        if hasattr(self, "_flat"):
            self._reset()

    def _unwritten(self):
        """``_sync_host_state()`` where there is device state to synchronise with: the parameters whose state tensors exist
        (from ``prepare()`` on) but hold nothing yet."""
        if not getattr(self, "_cap", None):
            return []
        ids = self._sync_host_state()
        return [p for g in self.param_groups for p in g["params"] if id(p) in ids] if ids else []

    def state_dict(self):
        drop = {id(p) for p in self._unwritten()}
        sd = super().state_dict()
        ids = [id(p) for g in self.param_groups for p in g["params"]]
        # plain tensors in NEW dicts (the base class hands out the live per-parameter dicts): no views of the flat buffers,
        # no shared step tensor -- what torch's optimizer writes
        sd["state"] = {k: {} if ids[k] in drop else
                       {n: (v.clone() if torch.is_tensor(v) and (v._base is not None or n == "step") else v)
                        for n, v in st.items()} for k, st in sd["state"].items()}
        return sd

    def __getstate__(self):
        drop = self._unwritten()
        st = super().__getstate__()
        if drop:
            st["state"] = defaultdict(dict, st["state"])
            for p in drop:
                st["state"][p] = {}
        return st

    # -- flat buffers ----------------------------------------------------------------------------------------------
    @staticmethod
    def _fp32_cuda(tensors):
        return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)

    def _require(self, ok):
        if not ok:
            raise RuntimeError("%s needs contiguous fp32 CUDA parameters on one device (no CPU fallback)" % type(self).__name__)

    def _flat_group(self, gi, group):
        """Flat buffers of a group (built once): parameters re-pointed into P, gradient views of G, and the subclass's state
        buffers (``_flat_state``).  None where the parameters do not allow it."""
        ent = self._flat.get(gi)
        params = group["params"]
        if ent is not None and len(ent["params"]) == len(params) and all(a is b for a, b in zip(ent["params"], params)):
            return ent
        if not params or not self._fp32_cuda(params) or any(p.device != params[0].device for p in params):
            return None
        offs, tot = [], 0
        for p in params:
            offs.append(tot)
            tot += (p.numel() + 3) // 4 * 4            # every tensor starts 16-byte aligned
        P, G = torch.zeros(tot, device=params[0].device), torch.zeros(tot, device=params[0].device)
        for p, view in zip(params, self._views(P, offs, params)):
            view.copy_(p.data)
            p.data = view
        ent = dict(params=list(params), P=P, G=G, offs=offs, n=tot, gviews=self._views(G, offs, params))
        self._flat_state(group, ent)
        self._flat[gi] = ent
        return ent

    @staticmethod
    def _views(buf, offs, params):
        return [buf[o:o + p.numel()].view_as(p) for p, o in zip(params, offs)]

    def gather_grads(self, group_index=0):
        """Flat gradient buffer of a parameter group with every existing ``p.grad`` copied in and re-pointed to its view
        (so the following ``step()`` finds them in place).  Parameters without a gradient contribute zeros."""
        ent = self._flat_group(group_index, self.param_groups[group_index])
        self._require(ent is not None)
        self._gather(ent)
        return ent["G"]

    @staticmethod
    def _gather(ent):
        src, dst = [], []
        for p, gvw in zip(ent["params"], ent["gviews"]):
            g = p.grad
            if g is None:
                gvw.zero_()
            elif g.data_ptr() != gvw.data_ptr():
                src.append(g)
                dst.append(gvw)
        if src:
            torch._foreach_copy_(dst, src)
            for p, gvw in zip(ent["params"], ent["gviews"]):
                if p.grad is not None:
                    p.grad = gvw

    # -- the state block -------------------------------------------------------------------------------------------
    def _block(self, gi, group, dev):
        cap = self._cap.get(gi)
        if cap is None:
            blk = torch.zeros(4, dtype=torch.float64, device=dev)      # stpde_opt_state: 32 bytes, zero-filled
            cap = self._cap[gi] = dict(blk=blk, lr=None, key=None, tab=None, chk=None, nchunks=0, pending=[], keep=[],
                                       spare=None)
            t = self._loaded_step(group)
            if t:
                blk.view(torch.int64)[0].fill_(int(t))
        return cap

    def _push_lr(self, cap, group):
        lr = float(group["lr"])
        if cap["lr"] != lr:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the learning rate changed inside a stream capture: call prepare() or sync_lr() before "
                                   "capturing (a captured write would reset the rate at every replay)")
            cap["blk"][1].fill_(lr)
            cap["lr"] = lr

    def sync_lr(self):
        """Push every ``group["lr"]`` that changed since the last push into its state block (what ``step()`` does first;
        ``GraphedStep`` calls it before each replay, so a scheduler takes effect without re-capture)."""
        for gi, group in enumerate(self.param_groups):
            cap = self._cap.get(gi)
            if cap is not None:
                self._push_lr(cap, group)

    def device_step(self, group_index=0):
        """Step count of a group, read back from the device (synchronises; for checkpoints and tests)."""
        cap = self._cap.get(group_index)
        return int(cap["blk"].view(torch.int64)[0].item()) if cap is not None else None

    def _advance(self, L, cap, beta1=0.0, beta2=0.0):
        od = _lib.OptDesc()
        od.beta1, od.beta2 = beta1, beta2
        _lib.check(L.stpde_opt_advance(C.byref(od), _lib.ptr(cap["blk"]), _lib.stream_ptr()))

    # -- pointer tables --------------------------------------------------------------------------------------------
    def _reserve_tables(self, cap, params, dtype):
        """A spare pair of table buffers (their sizes depend on the parameter shapes only), allocated OUTSIDE any stream
        capture.  A capture that meets new pointers takes it: memory allocated inside a capture comes from the graph's pool,
        where it may share its address with a temporary of an earlier node -- the replay would overwrite the table before the
        update kernel reads it."""
        if cap["spare"] is None and not torch.cuda.is_current_stream_capturing():
            nchunks = sum((p.numel() + _CHUNK - 1) // _CHUNK for p in params)
            dev = params[0].device
            cap["spare"] = (torch.empty(len(params) * dtype.itemsize, dtype=torch.uint8, device=dev),
                            torch.empty(nchunks * _CHUNK_DT.itemsize, dtype=torch.uint8, device=dev))

    def _table(self, cap, rows, dtype, dev):
        """Device tables for ``rows`` (one tuple per tensor, laid out as ``dtype``): the ones built last time while no
        pointer changed, else rebuilt and uploaded.  Inside a stream capture nothing may be uploaded or allocated for keeps:
        the spare buffers of ``_reserve_tables`` are taken, their contents staged on the host and written by
        ``flush_tables()`` right after the capture -- the captured launch holds their addresses, not their contents.  Tables
        a capture has seen are never rewritten or released (``keep``)."""
        key = tuple(rows)
        capturing = torch.cuda.is_current_stream_capturing()
        if cap["key"] != key:
            host, nchunks = _host_tables(rows, dtype)
            if capturing:
                tabs, cap["spare"] = cap["spare"], None
                if tabs is None or any(t.numel() != h.numel() for t, h in zip(tabs, host)):
                    raise RuntimeError("%s(flat=False): new gradient / state pointers inside a stream capture and no table "
                                       "buffer reserved for them: call prepare() before the capture" % type(self).__name__)
                cap["pending"] += list(zip(tabs, host))
            else:
                self.flush_tables()
                tabs = tuple(h.to(dev) for h in host)
            cap.update(key=key, tab=tabs[0], chk=tabs[1], nchunks=nchunks)
        if capturing and not any(t is cap["tab"] for t in cap["keep"]):
            cap["keep"] += [cap["tab"], cap["chk"]]          # a graph reads these for as long as it lives
        return cap["tab"], cap["chk"], cap["nchunks"]

    def flush_tables(self):
        """Upload the pointer tables that were staged during a stream capture (call once the capture has ended and before
        the first replay; ``GraphedStep`` does)."""
        for cap in self._cap.values():
            for t, h in cap["pending"]:
                t.copy_(h)
            del cap["pending"][:]

    def _check_aligned(self, rows, tensors=()):
        """The kernels use float4 accesses: every pointer column of a table 16-byte aligned, every tensor dense."""
        if any(q & 15 for r in rows for q in r[:self._NPTR]) or not all(t.is_contiguous() for t in tensors):
            raise RuntimeError("%s needs contiguous, 16-byte aligned tensors" % type(self).__name__)

    # -- steps -----------------------------------------------------------------------------------------------------
    def prepare(self):
        """All lazy work of the first step, up front: flat buffers (``flat=True`` re-points every ``p.data`` HERE), state
        tensors, state blocks, the first learning-rate push and spare pointer-table buffers.  A stream capture that follows
        contains launches only and allocates nothing that has to outlive it."""
        for gi, group in enumerate(self.param_groups):
            self._prepare_group(gi, group)
        return self

    def state_tensors(self):
        """Every device tensor a step writes besides the parameters: state blocks and moments / momentum buffers
        (``GraphedStep`` snapshots them around its warm-up)."""
        self.prepare()
        out = [cap["blk"] for cap in self._cap.values()]
        for gi, group in enumerate(self.param_groups):
            ent = self._flat.get(gi) if self._use_flat else None
            if ent is not None:
                out += [ent[k] for k in self._FLAT_STATE if ent[k] is not None]
            else:
                out += [v for p in group["params"] for n, v in self.state[p].items()
                        if torch.is_tensor(v) and v.is_cuda]
        return out

    def _prepare_group(self, gi, group):
        params = group["params"]
        if not params:
            return None, None
        ent = self._flat_group(gi, group) if self._use_flat else None
        if not self.capturable:
            return None, ent
        self._require(ent is not None if self._use_flat else self._fp32_cuda(params))
        cap = self._block(gi, group, params[0].device)       # first: the loaded step is read from the state as it was loaded
        self._init_state(group, ent)
        if ent is None:
            self._reserve_tables(cap, params, self._ROW_DT)
        self._push_lr(cap, group)
        return cap, ent

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        for gi, group in enumerate(self.param_groups):
            if self.capturable:
                self._step_capturable(L, gi, group)
                continue
            ent = self._flat_group(gi, group) if self._use_flat else None
            if ent is not None and all(p.grad is not None for p in ent["params"]):
                how = self._flat_step(group, ent)            # None: the parameters differ, no flat pass can serve them
                if how is not None:
                    self._gather(ent)
                    with _lib.device_of(ent["P"]):
                        self._launch_flat(L, group, None, ent, how)
                    continue
            self._step_table(L, group, ent)
        return loss

    def _step_table(self, L, group, ent):
        """Host-scalar pointer-table launch: parameters with a gradient only, each at its own point of its history.  ONE
        launch for the whole group: tensor table + chunk table (a few KB) are uploaded per step."""
        self._require(self._fp32_cuda(p for p in group["params"] if p.grad is not None))
        rows, keep = self._host_rows(group, ent)
        if not rows:
            return
        self._check_aligned(rows)
        dev = keep[0].device
        host, nchunks = _host_tables(rows, self._ROW_DT)
        tab, chk = host[0].to(dev), host[1].to(dev)
        with _lib.device_of(tab):
            self._launch_table(L, group, None, tab, chk, nchunks)
            tab.record_stream(torch.cuda.current_stream())
            chk.record_stream(torch.cuda.current_stream())

    def _step_capturable(self, L, gi, group):
        cap, ent = self._prepare_group(gi, group)
        if cap is None:
            return
        params = group["params"]
        if any(p.grad is None for p in params):
            raise RuntimeError(_NO_GRAD_MSG % type(self).__name__)
        betas = group.get("betas", (0.0, 0.0))
        with _lib.device_of(cap["blk"]):
            if ent is not None:
                self._gather(ent)
                self._advance(L, cap, *betas)
                self._launch_flat(L, group, cap, ent, None)
                return
            tensors = self._row_tensors(group)
            rows = [tuple(0 if t is None else t.data_ptr() for t in ts) + (ts[0].numel(),) + self._ROW_TAIL for ts in tensors]
            self._check_aligned(rows, [t for ts in tensors for t in ts if t is not None])
            tab, chk, nchunks = self._table(cap, rows, self._ROW_DT, params[0].device)
            self._advance(L, cap, *betas)
            self._launch_table(L, group, cap, tab, chk, nchunks)


class FusedClipAdam(_FusedClip):
    """clip_grad_value_ + Adam over FLAT buffers (round 3); see ``_FusedClip`` for ``flat``, the aliasing
    note and ``capturable``.

    ``exp_avg`` / ``exp_avg_sq`` are views of the flat buffers M / V.  While all parameters of a group are at the same step
    count they share ONE ``step`` tensor and a step is one ``stpde_clip_adam`` launch; once a parameter has missed a gradient
    the step counts differ for good (torch's Adam skips such a parameter) and the pointer-table kernel, with per-tensor bias
    corrections, carries the group.  ``capturable=True``: ``stpde_clip_adam_dev`` over the flat buffers,
    ``stpde_clip_adam_multi_dev`` over the pointer table."""
    _ROW_DT, _NPTR, _ROW_TAIL, _FLAT_STATE = _TENSOR_DT, 4, (0.0, 1.0), ("M", "V")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad=0.0, flat=True,
                 capturable=False):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip_grad=clip_grad,
                                      flat=bool(flat), capturable=bool(capturable)))

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("FusedClipAdam does not implement amsgrad / maximize")

    def _flat_state(self, group, ent):
        params, offs = ent["params"], ent["offs"]
        ent["M"], ent["V"], ent["step"] = torch.zeros_like(ent["P"]), torch.zeros_like(ent["P"]), None
        for name, buf in (("exp_avg", ent["M"]), ("exp_avg_sq", ent["V"])):
            for p, mv in zip(params, self._views(buf, offs, params)):
                st = self.state[p]
                if name in st:
                    mv.copy_(st[name])
                st[name] = mv
        for p in params:
            self.state[p].setdefault("step", torch.tensor(0.0))
        self._share_step(ent)

    def _share_step(self, ent):
        """All parameters at the same step count: ONE shared ``step`` tensor (one host increment per step instead of one
        per parameter); un-shared again (``_unshare_step``) before a pointer-table step could advance them unequally."""
        steps = {float(self.state[p]["step"]) for p in ent["params"]}
        if len(steps) == 1:
            ent["step"] = torch.tensor(steps.pop())
            for p in ent["params"]:
                self.state[p]["step"] = ent["step"]

    def _unshare_step(self, ent):
        if ent.get("step") is not None:
            for p in ent["params"]:
                self.state[p]["step"] = self.state[p]["step"].clone()
            ent["step"] = None

    def _init_state(self, group, ent):
        if ent is None:                                  # (flat: ``_flat_state`` has made them)
            for p in group["params"]:
                st = self.state[p]
                if "step" not in st:
                    st["step"] = torch.tensor(0.0)
                for name in ("exp_avg", "exp_avg_sq"):
                    if name not in st:
                        st[name] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _loaded_step(self, group):
        steps = {float(self.state[p].get("step", 0.0)) for p in group["params"]}     # (no state yet: step 0)
        if len(steps) > 1:
            raise ValueError("FusedClipAdam(capturable=True): the parameters of a group must share one step count, the loaded "
                             "state has %s" % sorted(steps))
        return steps.pop() if steps else 0

    def _sync_host_state(self):
        """Device step counts -> the per-parameter host entries, ``step`` as torch.optim.Adam writes it (one synchronising
        read per group, the only one of the capturable mode)."""
        for gi, group in enumerate(self.param_groups):
            t = self.device_step(gi)
            if t is not None:
                for p in group["params"]:
                    if self.state[p]:
                        self.state[p]["step"] = torch.tensor(float(t))
        return ()

    def _desc(self, group, n=0, t=None):
        """Descriptor of a launch; ``t``: the step count whose bias corrections go in as host scalars (None: they come from
        the table rows or from the state block)."""
        b1, b2 = group["betas"]
        d = _lib.AdamDesc()
        d.n = n
        d.clip, d.beta1, d.beta2, d.eps = float(group["clip_grad"] or 0.0), b1, b2, group["eps"]
        d.weight_decay, d.step_size, d.bias2_sqrt = group["weight_decay"], 0.0, 1.0
        if t is not None:
            d.step_size, d.bias2_sqrt = group["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
        return d

    def _flat_step(self, group, ent):
        if ent["step"] is None:
            self._share_step(ent)
        if ent["step"] is None:
            return None
        ent["step"] += 1
        return float(ent["step"])

    def _launch_flat(self, L, group, cap, ent, t):
        d = self._desc(group, ent["n"], t)
        bufs = (_lib.ptr(ent["P"]), _lib.ptr(ent["G"]), _lib.ptr(ent["M"]), _lib.ptr(ent["V"]), _lib.stream_ptr())
        if cap is None:
            _lib.check(L.stpde_clip_adam(C.byref(d), *bufs))
        else:
            _lib.check(L.stpde_clip_adam_dev(C.byref(d), _lib.ptr(cap["blk"]), *bufs))

    def _host_rows(self, group, ent):
        """Per-tensor step counts: every parameter with a gradient advances its own and gets its own bias corrections."""
        if ent is not None:
            self._unshare_step(ent)
        b1, b2 = group["betas"]
        rows, keep = [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            t = float(st["step"])
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            keep.append(g)
            rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                         group["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)))
        return rows, keep

    def _row_tensors(self, group):
        return [(p, p.grad, st["exp_avg"], st["exp_avg_sq"]) for p in group["params"] for st in (self.state[p],)]

    def _launch_table(self, L, group, cap, tab, chk, nchunks):
        d = self._desc(group)
        tabs = (_lib.ptr(tab), _lib.ptr(chk), nchunks, _CHUNK, _lib.stream_ptr())
        if cap is None:
            _lib.check(L.stpde_clip_adam_multi(C.byref(d), *tabs))
        else:
            _lib.check(L.stpde_clip_adam_multi_dev(C.byref(d), _lib.ptr(cap["blk"]), *tabs))


class FusedClipSGD(_FusedClip):
    """clip_grad_value_ + torch.optim.SGD (momentum, dampening, weight decay, Nesterov) in ONE HIP launch per group: the
    reference's ``--optim sgd`` (experiments/rb2d/train.py:220, :330-333 behind the clipping of :79-83); see ``_FusedClip``
    for ``flat``, the aliasing note and ``capturable``.

    ``flat=True``: parameters, gradients and momentum buffers of a group live in three flat buffers and a step is one
    ``stpde_clip_sgd`` launch; a step in which some parameter has no gradient, or in which only some parameters take their first
    momentum step, goes through the pointer-table kernel (``stpde_clip_sgd_multi``), which is also the ``flat=False`` path.
    The state name is torch's ``momentum_buffer`` (present once a parameter has taken a step with momentum), so checkpoints
    interoperate with ``torch.optim.SGD`` both ways.  ``capturable=True``: the same two entry points with the state block;
    "first step" (``buf = g``) is then decided from the device step count, and ``state_dict()`` / pickling read that count
    back (one synchronising read per group, the only one of the mode) to leave never-used buffers out of the checkpoint."""
    _ROW_DT, _NPTR, _ROW_TAIL, _FLAT_STATE = _SGD_TENSOR_DT, 3, (0, 0), ("B",)

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, clip_grad=0, flat=True,
                 capturable=False):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameters")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=bool(nesterov), clip_grad=clip_grad, flat=bool(flat),
                                      capturable=bool(capturable)))

    def _check_group(self, group):
        group.setdefault("nesterov", False)
        if group.get("maximize"):
            raise ValueError("FusedClipSGD does not implement maximize")
        if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():                   # torch.optim.SGD writes ``momentum_buffer: None`` without momentum
            if st.get("momentum_buffer", 0) is None:
                del st["momentum_buffer"]

    def _flat_state(self, group, ent):
        """Momentum buffers are views of B; a parameter's state names its view once it has taken a step (``_buffer``)."""
        ent["B"] = torch.zeros_like(ent["P"]) if group["momentum"] != 0 else None
        ent["bviews"] = self._views(ent["B"], ent["offs"], ent["params"]) if ent["B"] is not None else []
        for p, b in zip(ent["params"], ent["bviews"]):
            st = self.state[p]
            if torch.is_tensor(st.get("momentum_buffer")):
                b.copy_(st["momentum_buffer"])
                st["momentum_buffer"] = b

    def _buffer(self, ent, k, p):
        """Momentum buffer of parameter k for this step and whether it takes its first step (torch: no buffer in the state)."""
        st = self.state[p]
        first = not torch.is_tensor(st.get("momentum_buffer"))
        if first:
            st["momentum_buffer"] = ent["bviews"][k] if ent is not None else \
                torch.zeros_like(p, memory_format=torch.preserve_format)
        return st["momentum_buffer"], first

    def _init_state(self, group, ent):
        if group["momentum"] != 0:
            for k, p in enumerate(group["params"]):
                self._buffer(ent, k, p)

    # capturable mode keeps no host step entries: the count only says whether the momentum buffers hold anything yet
    def _loaded_step(self, group):
        return 1 if any(torch.is_tensor(self.state[p].get("momentum_buffer")) for p in group["params"]) else 0

    def _sync_host_state(self):
        """ids of the parameters whose momentum buffers exist (from prepare() on) but hold nothing yet: capturable mode before
        the first step (one synchronising read per group)."""
        return {id(p) for gi, g in enumerate(self.param_groups) if self.device_step(gi) == 0 for p in g["params"]}

    def _desc(self, group, n=0, first=0):
        d = _lib.SgdDesc()
        d.n, d.clip, d.lr, d.momentum = n, float(group["clip_grad"] or 0.0), group["lr"], group["momentum"]
        d.dampening, d.weight_decay, d.nesterov, d.first_step = group["dampening"], group["weight_decay"], \
            int(group["nesterov"]), int(first)
        return d

    def _flat_step(self, group, ent):
        """The first-step flag all parameters share (False without momentum), None where they differ."""
        if group["momentum"] == 0:
            return False
        params = ent["params"]
        firsts = {not torch.is_tensor(self.state[p].get("momentum_buffer")) for p in params}
        if len(firsts) != 1:
            return None
        if True in firsts:
            for k, p in enumerate(params):
                self._buffer(ent, k, p)
        return firsts.pop()

    def _launch_flat(self, L, group, cap, ent, first):
        d = self._desc(group, ent["n"], bool(first))
        _lib.check(L.stpde_clip_sgd(C.byref(d), _lib.ptr(cap["blk"]) if cap else None, _lib.ptr(ent["P"]),
                                    _lib.ptr(ent["G"]), _lib.ptr(ent["B"]), _lib.stream_ptr()))

    def _host_rows(self, group, ent):
        """Per-tensor first-step flags."""
        mom = group["momentum"] != 0
        rows, keep = [], []
        for k, p in enumerate(group["params"]):
            if p.grad is None:
                continue
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            keep.append(g)
            buf, first = self._buffer(ent, k, p) if mom else (None, False)
            rows.append((p.data_ptr(), g.data_ptr(), buf.data_ptr() if mom else 0, p.numel(), int(first), 0))
        return rows, keep

    def _row_tensors(self, group):
        mom = group["momentum"] != 0
        return [(p, p.grad, self.state[p]["momentum_buffer"] if mom else None) for p in group["params"]]

    def _launch_table(self, L, group, cap, tab, chk, nchunks):
        d = self._desc(group)
        _lib.check(L.stpde_clip_sgd_multi(C.byref(d), _lib.ptr(cap["blk"]) if cap else None, _lib.ptr(tab), _lib.ptr(chk),
                                          nchunks, _CHUNK, _lib.stream_ptr()))
