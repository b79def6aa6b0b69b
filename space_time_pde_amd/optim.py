"""Fused gradient-value clipping + Adam.

``FusedClipAdam`` is a ``torch.optim.Optimizer`` whose ``step()`` does, for ALL parameter tensors of a group in ONE HIP
kernel launch (``stpde_clip_adam_multi``; ``stpde_clip_adam`` is the single-tensor entry point), what the reference does with ``clip_grad_value_`` followed by ``optim.Adam.step``
(experiments/rb2d/train.py:79-83): same state names (``step``, ``exp_avg``, ``exp_avg_sq``), so
``state_dict()`` / ``load_state_dict()`` interoperate with ``torch.optim.Adam`` checkpoints written by the reference.

``FusedClipSGD`` is the same for the reference's ``--optim sgd`` (train.py:220, :330-333): ``clip_grad_value_`` +
``torch.optim.SGD`` (momentum, dampening, weight decay, Nesterov) in one launch, state name ``momentum_buffer``.

Both take ``capturable=True``: step count and learning rate then live in device memory (``stpde_opt_state``), a step is
``stpde_opt_advance`` + one update launch with no host read-back and no upload, and ``train_step.GraphedStep(...,
optimizer=opt)`` replays the whole iteration -- forward, backward, clip, update -- from one HIP graph.
"""
import ctypes as C
import math

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


class _DeviceState:
    """What ``capturable=True`` adds to an optimizer: per group one ``stpde_opt_state`` block in device memory (64-bit step
    count, fp64 learning rate, the two derived Adam scalars) and, with ``flat=False``, pointer tables that are built once.

    ``group["lr"]`` stays the knob a scheduler turns: a value that differs from the last one pushed is written into the
    block (one fill launch, no synchronisation) by ``step()`` / ``sync_lr()`` -- never inside a stream capture, where the
    fill would be recorded and every replay would reset the rate."""

    def _init_device_state(self):
        self._cap = {}          # group index -> dict(blk, lr, key, tab, chk, nchunks, pending, keep, spare)

    @property
    def capturable(self):
        return bool(self.defaults.get("capturable", False))

    # -- the state block -------------------------------------------------------------------------------------------
    def _block(self, gi, group, dev):
        cap = self._cap.get(gi)
        if cap is None:
            blk = torch.zeros(4, dtype=torch.float64, device=dev)      # stpde_opt_state: 32 bytes, zero-filled
            cap = self._cap[gi] = dict(blk=blk, lr=None, key=None, tab=None, chk=None, nchunks=0, pending=[], keep=[], spare=None)
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

    # -- pointer tables of flat=False ------------------------------------------------------------------------------
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
            chunks = [(k, 0, off) for k, r in enumerate(rows) for off in range(0, r[dtype.names.index("n")], _CHUNK)]
            host = (torch.from_numpy(np.array(rows, dtype=dtype).view(np.uint8)),
                    torch.from_numpy(np.array(chunks, dtype=_CHUNK_DT).view(np.uint8)))
            if capturing:
                tabs, cap["spare"] = cap["spare"], None
                if tabs is None or any(t.numel() != h.numel() for t, h in zip(tabs, host)):
                    raise RuntimeError("%s(flat=False): new gradient / state pointers inside a stream capture and no table "
                                       "buffer reserved for them: call prepare() before the capture" % type(self).__name__)
                cap["pending"] += list(zip(tabs, host))
            else:
                self.flush_tables()
                tabs = tuple(h.to(dev) for h in host)
            cap.update(key=key, tab=tabs[0], chk=tabs[1], nchunks=len(chunks))
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

    def _checked_ptrs(self, tensors):
        ptrs = tuple(t.data_ptr() for t in tensors)
        if any(q & 15 for q in ptrs) or not all(t.is_contiguous() for t in tensors):
            raise RuntimeError("%s needs contiguous, 16-byte aligned tensors" % type(self).__name__)
        return ptrs

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

    def _pull_steps(self):
        """Device step counts -> the per-parameter host entries (one synchronising read per group)."""
        for gi, group in enumerate(self.param_groups):
            t = self.device_step(gi)
            if t is not None:
                self._store_step(group, t)

    def __getstate__(self):
        if self.capturable and getattr(self, "_cap", None):
            self._pull_steps()
        return super().__getstate__()


class FusedClipAdam(_DeviceState, torch.optim.Optimizer):
    """clip_grad_value_ + Adam over FLAT buffers (round 3).

    ``flat=True`` (default): on the first step the parameters of a group are moved into ONE contiguous fp32 buffer (every
    ``p.data`` becomes a view of it, values preserved), and ``exp_avg`` / ``exp_avg_sq`` are views of two more buffers
    allocated once.  A step is then: gradients gathered into the flat gradient buffer (``torch._foreach_copy_``: a
    handful of multi-tensor launches; skipped for gradients that already live there, see ``gather_grads``) and ONE
    ``stpde_clip_adam`` launch over the whole buffer -- no per-step table build, no host-to-device upload.
    ``gather_grads()`` returns that flat gradient buffer with every ``p.grad`` re-pointed into it, so a data-parallel
    step all-reduces exactly the buffer the optimizer reads (reference: DDP's bucket, train_ddp.py:401-406).
    The per-parameter state keeps torch.optim.Adam's names and shapes; ``state_dict()`` returns plain (cloned) tensors,
    so checkpoints interoperate with the reference's Adam both ways.
    A group falls back to the multi-tensor pointer-table kernel for a step in which some parameter has no gradient or the
    step counts differ (torch's Adam skips such parameters; a flat pass could not).

    Aliasing: building the flat buffers (first ``step()`` / ``gather_grads()`` after construction, ``load_state_dict`` or
    ``add_param_group``) RE-POINTS every ``p.data`` into the new buffer.  The values are preserved, the storage is not: an
    alias of the old storage taken before that (an EMA copy made with ``p.data`` views, a captured hipGraph, a
    ``DistributedDataParallel`` bucket view) keeps pointing at memory the optimizer no longer updates.  Take such aliases
    after the first step (or after ``prepare()``), or construct with ``flat=False`` (pointer-table kernel, storages untouched).

    ``capturable=True``: the step count and the learning rate live in device memory (see ``_DeviceState``); a step is
    ``stpde_opt_advance`` + ONE update launch (``stpde_clip_adam_dev`` over the flat buffers, ``stpde_clip_adam_multi_dev``
    over a pointer table that is rebuilt only when a pointer changes), safe to capture in a HIP graph.  All parameters of a
    group share the step count, so every parameter needs a gradient at every step.  ``capturable=False`` is the path
    described above, unchanged."""
    _FLAT_STATE = ("M", "V")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad=0.0, flat=True,
                 capturable=False):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("invalid Adam hyper-parameters")
        # ``flat`` and ``capturable`` travel in ``defaults`` (what Optimizer.__getstate__ serialises), so a deepcopy / pickle
        # of an optimizer comes back in the mode it was built with
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip_grad=clip_grad,
                                      flat=bool(flat), capturable=bool(capturable)))
        self._use_flat = bool(flat)
        self._flat = {}          # id(group) -> dict(P, G, M, V, offs, views...)
        self._init_device_state()

    def __setstate__(self, state):
        # Optimizer.load_state_dict replaces param_groups with the SAVED groups: a checkpoint written by the
        # reference's torch.optim.Adam (train.py:390-397) has no ``clip_grad`` entry, and carries Adam options
        # (amsgrad, maximize, foreach, ...) this optimizer does not implement -- keep this instance's clip value and
        # refuse the options that would change the update rule.
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("clip_grad", self.defaults["clip_grad"])
            group.setdefault("flat", self.defaults.get("flat", True))
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedClipAdam does not implement amsgrad / maximize")
            # a reference-written group may say capturable=False (torch.optim.Adam's own flag): this instance's mode holds
            group["capturable"] = self.defaults.get("capturable", False)
        self._flat = {}          # loaded state tensors are fresh allocations: rebuild the flat views on the next step
        self._init_device_state()   # ... and set the device step counts from the loaded ``step`` entries
        # Optimizer.__getstate__ serialises defaults / state / param_groups only: an instance that comes back from
        # copy.deepcopy or pickle takes its mode from ``defaults`` (it used to come back as flat=True)
        self._use_flat = bool(self.defaults.get("flat", getattr(self, "_use_flat", True)))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._flat = {}
        self._init_device_state()

    def add_param_group(self, group):
        if getattr(self, "_cap", None):
            self._pull_steps()
        super().add_param_group(group)
        if hasattr(self, "_flat"):
            self._flat = {}
            self._init_device_state()

    def state_dict(self):
        if self.capturable and self._cap:
            self._pull_steps()       # the one synchronising read of the capturable mode: ``step`` as torch.optim.Adam writes it
        sd = super().state_dict()
        # plain tensors in NEW dicts (the base class hands out the live per-parameter dicts): no views of the flat buffers,
        # no shared step tensor -- what torch.optim.Adam writes
        sd["state"] = {k: {n: (v.clone() if torch.is_tensor(v) and (v._base is not None or n == "step") else v)
                           for n, v in st.items()} for k, st in sd["state"].items()}
        return sd

    # ---------------------------------------------------------------------------------------------------------
    def _flat_group(self, gi, group):
        """Flat buffers of a group (built once): parameters re-pointed into P, moments into M / V."""
        ent = self._flat.get(gi)
        params = group["params"]
        if ent is not None and len(ent["params"]) == len(params) and all(a is b for a, b in zip(ent["params"], params)):
            return ent
        if not params or not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and
                                 p.device == params[0].device for p in params):
            return None
        dev = params[0].device
        offs, tot = [], 0
        for p in params:
            offs.append(tot)
            tot += (p.numel() + 3) // 4 * 4            # every tensor starts 16-byte aligned
        P, G, M, V = (torch.zeros(tot, device=dev) for _ in range(4))
        pv, gv = [], []
        for p, o in zip(params, offs):
            n = p.numel()
            view = P[o:o + n].view_as(p)
            view.copy_(p.data)
            p.data = view
            pv.append(view)
            gv.append(G[o:o + n].view_as(p))
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
            for name, buf in (("exp_avg", M), ("exp_avg_sq", V)):
                mv = buf[o:o + n].view_as(p)
                if name in st:
                    mv.copy_(st[name])
                st[name] = mv
        ent = dict(params=list(params), P=P, G=G, M=M, V=V, offs=offs, n=tot, gviews=gv, step=None)
        self._share_step(ent)
        self._flat[gi] = ent
        return ent

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

    def gather_grads(self, group_index=0):
        """Flat gradient buffer of a parameter group with every existing ``p.grad`` copied in and re-pointed to its view
        (so the following ``step()`` finds them in place).  Parameters without a gradient contribute zeros."""
        group = self.param_groups[group_index]
        ent = self._flat_group(group_index, group)
        if ent is None:
            raise RuntimeError("gather_grads needs contiguous fp32 CUDA parameters on one device")
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
            b1, b2 = group["betas"]
            ent = self._flat_group(gi, group) if self._use_flat else None
            if ent is not None and all(p.grad is not None for p in ent["params"]):
                if ent["step"] is None:
                    self._share_step(ent)
                if ent["step"] is not None:
                    ent["step"] += 1
                    t = float(ent["step"])
                    self._gather(ent)
                    d = _lib.AdamDesc()
                    d.n = ent["n"]
                    d.clip, d.beta1, d.beta2, d.eps = float(group["clip_grad"] or 0.0), b1, b2, group["eps"]
                    d.weight_decay = group["weight_decay"]
                    d.step_size, d.bias2_sqrt = group["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
                    with _lib.device_of(ent["P"]):
                        _lib.check(L.stpde_clip_adam(C.byref(d), _lib.ptr(ent["P"]), _lib.ptr(ent["G"]),
                                                     _lib.ptr(ent["M"]), _lib.ptr(ent["V"]), _lib.stream_ptr()))
                    continue
            if ent is not None:
                self._unshare_step(ent)
            self._step_table(L, group)
        return loss

    def _step_table(self, L, group):
        """Multi-tensor pointer-table launch: parameters with a gradient only, per-tensor step counts."""
        b1, b2 = group["betas"]
        if True:
            rows, chunks, keep = [], [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError("FusedClipAdam needs contiguous fp32 CUDA parameters (no CPU fallback)")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                t = float(st["step"])
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(g)
                ptrs = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
                if any(q & 15 for q in ptrs):
                    raise RuntimeError("FusedClipAdam needs 16-byte aligned tensors")
                n = p.numel()
                for off in range(0, n, _CHUNK):
                    chunks.append((len(rows), 0, off))
                rows.append(ptrs + (n, group["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)))
            if not rows:
                return
            dev = keep[0].device
            # ONE launch for the whole group: tensor table + chunk table (a few KB) are uploaded per step
            tab = torch.from_numpy(np.array(rows, dtype=_TENSOR_DT).view(np.uint8)).to(dev)
            chk = torch.from_numpy(np.array(chunks, dtype=_CHUNK_DT).view(np.uint8)).to(dev)
            d = _lib.AdamDesc()
            d.n = 0
            d.clip, d.beta1, d.beta2, d.eps = float(group["clip_grad"] or 0.0), b1, b2, group["eps"]
            d.weight_decay, d.step_size, d.bias2_sqrt = group["weight_decay"], 0.0, 1.0
            with _lib.device_of(tab):
                _lib.check(L.stpde_clip_adam_multi(C.byref(d), _lib.ptr(tab), _lib.ptr(chk), len(chunks), _CHUNK,
                                                   _lib.stream_ptr()))
                tab.record_stream(torch.cuda.current_stream())
                chk.record_stream(torch.cuda.current_stream())

    # ---- capturable mode ---------------------------------------------------------------------------------------------
    def _loaded_step(self, group):
        steps = {float(self.state[p]["step"]) for p in group["params"] if "step" in self.state[p]}
        if len(steps) > 1:
            raise ValueError("FusedClipAdam(capturable=True): the parameters of a group must share one step count, the loaded "
                             "state has %s" % sorted(steps))
        return steps.pop() if steps else 0

    def _store_step(self, group, t):
        for p in group["params"]:
            if self.state[p]:
                self.state[p]["step"] = torch.tensor(float(t))

    def _prepare_group(self, gi, group):
        params = group["params"]
        if not params:
            return None, None
        ent = None
        if self._use_flat:
            ent = self._flat_group(gi, group)
            if ent is None and self.capturable:
                raise RuntimeError("FusedClipAdam needs contiguous fp32 CUDA parameters on one device (no CPU fallback)")
        if not self.capturable:
            return None, ent
        if ent is None:
            for p in params:
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError("FusedClipAdam needs contiguous fp32 CUDA parameters (no CPU fallback)")
                st = self.state[p]
                if "step" not in st:
                    st["step"] = torch.tensor(0.0)
                for name in ("exp_avg", "exp_avg_sq"):
                    if name not in st:
                        st[name] = torch.zeros_like(p, memory_format=torch.preserve_format)
        cap = self._block(gi, group, params[0].device)
        if ent is None:
            self._reserve_tables(cap, params, _TENSOR_DT)
        self._push_lr(cap, group)
        return cap, ent

    def _step_capturable(self, L, gi, group):
        cap, ent = self._prepare_group(gi, group)
        if cap is None:
            return
        params = group["params"]
        if any(p.grad is None for p in params):
            raise RuntimeError(_NO_GRAD_MSG % "FusedClipAdam")
        b1, b2 = group["betas"]
        d = _lib.AdamDesc()
        d.n = ent["n"] if ent is not None else 0
        d.clip, d.beta1, d.beta2, d.eps = float(group["clip_grad"] or 0.0), b1, b2, group["eps"]
        d.weight_decay, d.step_size, d.bias2_sqrt = group["weight_decay"], 0.0, 1.0
        with _lib.device_of(cap["blk"]):
            if ent is not None:
                self._gather(ent)
                self._advance(L, cap, b1, b2)
                _lib.check(L.stpde_clip_adam_dev(C.byref(d), _lib.ptr(cap["blk"]), _lib.ptr(ent["P"]), _lib.ptr(ent["G"]),
                                                 _lib.ptr(ent["M"]), _lib.ptr(ent["V"]), _lib.stream_ptr()))
                return
            rows = []
            for p in params:
                st = self.state[p]
                rows.append(self._checked_ptrs((p, p.grad, st["exp_avg"], st["exp_avg_sq"])) + (p.numel(), 0.0, 1.0))
            tab, chk, nchunks = self._table(cap, rows, _TENSOR_DT, params[0].device)
            self._advance(L, cap, b1, b2)
            _lib.check(L.stpde_clip_adam_multi_dev(C.byref(d), _lib.ptr(cap["blk"]), _lib.ptr(tab), _lib.ptr(chk), nchunks,
                                                   _CHUNK, _lib.stream_ptr()))


class FusedClipSGD(_DeviceState, torch.optim.Optimizer):
    """clip_grad_value_ + torch.optim.SGD (momentum, dampening, weight decay, Nesterov) in ONE HIP launch per group: the
    reference's ``--optim sgd`` (experiments/rb2d/train.py:220, :330-333 behind the clipping of :79-83).

    Built like ``FusedClipAdam``.  ``flat=True``: parameters, gradients and momentum buffers of a group live in three flat
    buffers (``p.data`` re-pointed on the first step / ``prepare()``, see the aliasing note there) and a step is one
    ``stpde_clip_sgd`` launch; a step in which some parameter has no gradient, or in which only some parameters take their first
    momentum step, goes through the pointer-table kernel (``stpde_clip_sgd_multi``), which is also the ``flat=False`` path.
    The state name is torch's ``momentum_buffer`` (present once a parameter has taken a step with momentum), so checkpoints
    interoperate with ``torch.optim.SGD`` both ways.  ``capturable=True``: as for ``FusedClipAdam``; "first step" (``buf = g``)
    is then decided from the device step count, and ``state_dict()`` / pickling read that count back (one synchronising read
    per group, the only one of the mode) to leave never-used buffers out of the checkpoint."""
    _FLAT_STATE = ("B",)

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, clip_grad=0, flat=True,
                 capturable=False):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameters")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=bool(nesterov), clip_grad=clip_grad, flat=bool(flat),
                                      capturable=bool(capturable)))
        self._use_flat = bool(flat)
        self._flat = {}
        self._init_device_state()

    def __setstate__(self, state):
        # as FusedClipAdam.__setstate__: a group saved by torch.optim.SGD has no ``clip_grad`` and carries options this
        # optimizer does not implement
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("clip_grad", self.defaults["clip_grad"])
            group.setdefault("flat", self.defaults.get("flat", True))
            group.setdefault("nesterov", False)
            if group.get("maximize"):
                raise ValueError("FusedClipSGD does not implement maximize")
            if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
                raise ValueError("Nesterov momentum requires a momentum and zero dampening")
            group["capturable"] = self.defaults.get("capturable", False)
        self._flat = {}
        self._init_device_state()
        self._use_flat = bool(self.defaults.get("flat", getattr(self, "_use_flat", True)))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():                   # torch.optim.SGD writes ``momentum_buffer: None`` without momentum
            if st.get("momentum_buffer", 0) is None:
                del st["momentum_buffer"]
        self._flat = {}
        self._init_device_state()

    def add_param_group(self, group):
        # as FusedClipAdam: flat buffers and device state are rebuilt on the next step; "has a step been taken" is re-derived
        # from the momentum buffers, so buffers of a prepared but never stepped optimizer are dropped first
        if getattr(self, "_cap", None):
            fresh = self._fresh()
            for g in self.param_groups:
                for p in g["params"]:
                    if id(p) in fresh:
                        self.state[p].pop("momentum_buffer", None)
        super().add_param_group(group)
        if hasattr(self, "_flat"):
            self._flat = {}
            self._init_device_state()

    def _fresh(self):
        """ids of the parameters whose momentum buffers exist (from prepare() on) but hold nothing yet: capturable mode before
        the first step (one synchronising read per group)."""
        if not self.capturable:
            return set()
        return {id(p) for gi, g in enumerate(self.param_groups) if self.device_step(gi) == 0 for p in g["params"]}

    def state_dict(self):
        fresh = self._fresh()
        sd = super().state_dict()
        ids = [id(p) for g in self.param_groups for p in g["params"]]
        sd["state"] = {k: {n: (v.clone() if torch.is_tensor(v) and v._base is not None else v) for n, v in st.items()
                           if not (n == "momentum_buffer" and ids[k] in fresh)} for k, st in sd["state"].items()}
        return sd

    # capturable mode keeps no host step entries: the count only says whether the momentum buffers hold anything yet
    def _loaded_step(self, group):
        return 1 if any(torch.is_tensor(self.state[p].get("momentum_buffer")) for p in group["params"]) else 0

    def _store_step(self, group, t):
        pass

    def __getstate__(self):
        st = dict(torch.optim.Optimizer.__getstate__(self))
        fresh = self._fresh() if getattr(self, "_cap", None) else set()
        st["state"] = {p: {n: v for n, v in ps.items() if not (n == "momentum_buffer" and id(p) in fresh)}
                       for p, ps in st["state"].items()}
        return st

    # ---------------------------------------------------------------------------------------------------------
    def _flat_group(self, gi, group):
        """Flat buffers of a group (built once): parameters re-pointed into P, momentum buffers are views of B."""
        ent = self._flat.get(gi)
        params = group["params"]
        if ent is not None and len(ent["params"]) == len(params) and all(a is b for a, b in zip(ent["params"], params)):
            return ent
        if not params or not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and
                                 p.device == params[0].device for p in params):
            return None
        dev = params[0].device
        offs, tot = [], 0
        for p in params:
            offs.append(tot)
            tot += (p.numel() + 3) // 4 * 4            # every tensor starts 16-byte aligned
        P, G = torch.zeros(tot, device=dev), torch.zeros(tot, device=dev)
        B = torch.zeros(tot, device=dev) if group["momentum"] != 0 else None
        gv, bv = [], []
        for p, o in zip(params, offs):
            n = p.numel()
            view = P[o:o + n].view_as(p)
            view.copy_(p.data)
            p.data = view
            gv.append(G[o:o + n].view_as(p))
            if B is not None:
                b = B[o:o + n].view_as(p)
                st = self.state[p]
                if torch.is_tensor(st.get("momentum_buffer")):
                    b.copy_(st["momentum_buffer"])
                    st["momentum_buffer"] = b
                bv.append(b)
        ent = dict(params=list(params), P=P, G=G, B=B, offs=offs, n=tot, gviews=gv, bviews=bv)
        self._flat[gi] = ent
        return ent

    _gather = staticmethod(FusedClipAdam._gather)
    gather_grads = FusedClipAdam.gather_grads

    def _desc(self, group, n=0, first=0):
        d = _lib.SgdDesc()
        d.n, d.clip, d.lr, d.momentum = n, float(group["clip_grad"] or 0.0), group["lr"], group["momentum"]
        d.dampening, d.weight_decay, d.nesterov, d.first_step = group["dampening"], group["weight_decay"], \
            int(group["nesterov"]), int(first)
        return d

    def _buffer(self, ent, k, p):
        """Momentum buffer of parameter k for this step and whether it takes its first step (torch: no buffer in the state)."""
        st = self.state[p]
        first = not torch.is_tensor(st.get("momentum_buffer"))
        if first:
            st["momentum_buffer"] = ent["bviews"][k] if ent is not None else \
                torch.zeros_like(p, memory_format=torch.preserve_format)
        return st["momentum_buffer"], first

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
            mom = group["momentum"] != 0
            ent = self._flat_group(gi, group) if self._use_flat else None
            params = group["params"]
            if ent is not None and all(p.grad is not None for p in params):
                firsts = {not torch.is_tensor(self.state[p].get("momentum_buffer")) for p in params} if mom else {False}
                if len(firsts) == 1:
                    first = firsts.pop()
                    if mom and first:
                        for k, p in enumerate(params):
                            self._buffer(ent, k, p)
                    self._gather(ent)
                    d = self._desc(group, ent["n"], first)
                    with _lib.device_of(ent["P"]):
                        _lib.check(L.stpde_clip_sgd(C.byref(d), None, _lib.ptr(ent["P"]), _lib.ptr(ent["G"]),
                                                    _lib.ptr(ent["B"]), _lib.stream_ptr()))
                    continue
            self._step_table(L, group, ent)
        return loss

    def _step_table(self, L, group, ent):
        """Multi-tensor pointer-table launch: parameters with a gradient only, per-tensor first-step flags."""
        mom = group["momentum"] != 0
        rows, keep = [], []
        for k, p in enumerate(group["params"]):
            if p.grad is None:
                continue
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("FusedClipSGD needs contiguous fp32 CUDA parameters (no CPU fallback)")
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            keep.append(g)
            buf, first = self._buffer(ent, k, p) if mom else (None, False)
            ptrs = (p.data_ptr(), g.data_ptr(), buf.data_ptr() if mom else 0)
            if any(q & 15 for q in ptrs):
                raise RuntimeError("FusedClipSGD needs 16-byte aligned tensors")
            rows.append(ptrs + (p.numel(), int(first), 0))
        if not rows:
            return
        dev = keep[0].device
        chunks = [(k, 0, off) for k, r in enumerate(rows) for off in range(0, r[3], _CHUNK)]
        tab = torch.from_numpy(np.array(rows, dtype=_SGD_TENSOR_DT).view(np.uint8)).to(dev)
        chk = torch.from_numpy(np.array(chunks, dtype=_CHUNK_DT).view(np.uint8)).to(dev)
        d = self._desc(group)
        with _lib.device_of(tab):
            _lib.check(L.stpde_clip_sgd_multi(C.byref(d), None, _lib.ptr(tab), _lib.ptr(chk), len(chunks), _CHUNK,
                                              _lib.stream_ptr()))
            tab.record_stream(torch.cuda.current_stream())
            chk.record_stream(torch.cuda.current_stream())

    # ---- capturable mode ---------------------------------------------------------------------------------------------
    def _prepare_group(self, gi, group):
        params = group["params"]
        if not params:
            return None, None
        ent = None
        if self._use_flat:
            ent = self._flat_group(gi, group)
            if ent is None and self.capturable:
                raise RuntimeError("FusedClipSGD needs contiguous fp32 CUDA parameters on one device (no CPU fallback)")
        if not self.capturable:
            return None, ent
        for p in params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("FusedClipSGD needs contiguous fp32 CUDA parameters (no CPU fallback)")
        cap = self._block(gi, group, params[0].device)       # (reads the loaded buffers' presence: before the next loop)
        if group["momentum"] != 0:
            for k, p in enumerate(params):
                self._buffer(ent, k, p)
        if ent is None:
            self._reserve_tables(cap, params, _SGD_TENSOR_DT)
        self._push_lr(cap, group)
        return cap, ent

    def _step_capturable(self, L, gi, group):
        cap, ent = self._prepare_group(gi, group)
        if cap is None:
            return
        params = group["params"]
        if any(p.grad is None for p in params):
            raise RuntimeError(_NO_GRAD_MSG % "FusedClipSGD")
        mom = group["momentum"] != 0
        with _lib.device_of(cap["blk"]):
            if ent is not None:
                self._gather(ent)
                self._advance(L, cap)
                d = self._desc(group, ent["n"])
                _lib.check(L.stpde_clip_sgd(C.byref(d), _lib.ptr(cap["blk"]), _lib.ptr(ent["P"]), _lib.ptr(ent["G"]),
                                            _lib.ptr(ent["B"]), _lib.stream_ptr()))
                return
            rows = []
            for p in params:
                ts = (p, p.grad) + ((self.state[p]["momentum_buffer"],) if mom else ())
                rows.append(self._checked_ptrs(ts) + (() if mom else (0,)) + (p.numel(), 0, 0))
            tab, chk, nchunks = self._table(cap, rows, _SGD_TENSOR_DT, params[0].device)
            self._advance(L, cap)
            d = self._desc(group)
            _lib.check(L.stpde_clip_sgd_multi(C.byref(d), _lib.ptr(cap["blk"]), _lib.ptr(tab), _lib.ptr(chk), nchunks,
                                              _CHUNK, _lib.stream_ptr()))
