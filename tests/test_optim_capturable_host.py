"""Capturable optimizers, host side (no GPU): the C ABI of the device-state entry points (stpde_opt_advance,
stpde_clip_adam_dev / _multi_dev, stpde_clip_sgd / _multi) refuses bad arguments before any launch, and the Python layer
refuses what it cannot do -- Nesterov without momentum, a non-capturable optimizer inside ``GraphedStep``."""
import ctypes as C

import pytest
import torch

from space_time_pde_amd import _lib

NEW = ["stpde_opt_advance", "stpde_clip_adam_dev", "stpde_clip_adam_multi_dev", "stpde_clip_sgd", "stpde_clip_sgd_multi"]
OK, ODD = C.c_void_p(4096), C.c_void_p(4096 + 8)        # never dereferenced: every call below is refused before its launch


def _bad(rc):
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_new_symbols_are_exported_and_abi_is_316(hiplib):
    assert _lib.ABI_VERSION == 316 and hiplib.stpde_version() == 316
    for name in NEW:
        assert name in _lib.exported_symbols() and hasattr(hiplib, name), name
    assert C.sizeof(_lib.OptState) == 32 and _lib.OptState.lr.offset == 8 and _lib.OptState.step_size.offset == 16


def _adam(n=64):
    d = _lib.AdamDesc()
    d.n, d.clip, d.beta1, d.beta2, d.eps, d.weight_decay, d.step_size, d.bias2_sqrt = n, 1.0, 0.9, 0.999, 1e-8, 0.0, 0.0, 1.0
    return d


def _sgd(n=64, momentum=0.9):
    d = _lib.SgdDesc()
    d.n, d.clip, d.lr, d.momentum, d.dampening, d.weight_decay, d.nesterov, d.first_step = n, 1.0, 0.1, momentum, 0.0, 0.0, 0, 0
    return d


def test_opt_advance_rejects_bad_arguments(hiplib):
    od = _lib.OptDesc()
    od.beta1, od.beta2 = 0.9, 0.999
    _bad(hiplib.stpde_opt_advance(None, OK, None))
    _bad(hiplib.stpde_opt_advance(C.byref(od), None, None))
    _bad(hiplib.stpde_opt_advance(C.byref(od), ODD, None))
    od.beta2 = 1.0
    _bad(hiplib.stpde_opt_advance(C.byref(od), OK, None))


def test_clip_adam_dev_rejects_bad_arguments(hiplib):
    f = hiplib.stpde_clip_adam_dev
    _bad(f(None, OK, OK, OK, OK, OK, None))
    for k in range(5):                                   # state, param, grad, exp_avg, exp_avg_sq: null, then misaligned
        for bad in (None, ODD):
            a = [OK] * 5
            a[k] = bad
            _bad(f(C.byref(_adam()), *a, None))
    for n in (0, -4):
        _bad(f(C.byref(_adam(n)), OK, OK, OK, OK, OK, None))


def test_clip_adam_multi_dev_rejects_bad_arguments(hiplib):
    f = hiplib.stpde_clip_adam_multi_dev
    _bad(f(None, OK, OK, OK, 1, 1 << 16, None))
    for k in range(3):                                   # state, tensor table, chunk table
        for bad in (None, ODD):
            a = [OK] * 3
            a[k] = bad
            _bad(f(C.byref(_adam()), *a, 1, 1 << 16, None))
    for nchunks, chunk in ((0, 1 << 16), (-1, 1 << 16), (1, 0), (1, -4), (1, 6), (1, 1023)):
        _bad(f(C.byref(_adam()), OK, OK, OK, nchunks, chunk, None))


def test_clip_sgd_rejects_bad_arguments(hiplib):
    f = hiplib.stpde_clip_sgd
    _bad(f(None, None, OK, OK, OK, None))
    for state in (None, OK):                             # host form and device-state form
        _bad(f(C.byref(_sgd()), state, None, OK, OK, None))
        _bad(f(C.byref(_sgd()), state, OK, None, OK, None))
        _bad(f(C.byref(_sgd()), state, OK, OK, None, None))          # momentum != 0 needs a buffer
        for k in range(3):
            a = [OK] * 3
            a[k] = ODD
            _bad(f(C.byref(_sgd()), state, *a, None))
        for n in (0, -1):
            _bad(f(C.byref(_sgd(n)), state, OK, OK, OK, None))
    _bad(f(C.byref(_sgd()), ODD, OK, OK, OK, None))
    d = _sgd(momentum=0.0)
    d.nesterov = 1                                                   # Nesterov needs momentum
    _bad(f(C.byref(d), None, OK, OK, None, None))
    d = _sgd()
    d.nesterov, d.dampening = 1, 0.5                                 # ... and zero dampening
    _bad(f(C.byref(d), None, OK, OK, OK, None))


def test_clip_sgd_multi_rejects_bad_arguments(hiplib):
    f = hiplib.stpde_clip_sgd_multi
    _bad(f(None, None, OK, OK, 1, 1 << 16, None))
    for state in (None, OK):
        for k in range(2):                               # tensor table, chunk table
            for bad in (None, ODD):
                a = [OK] * 2
                a[k] = bad
                _bad(f(C.byref(_sgd()), state, *a, 1, 1 << 16, None))
        for nchunks, chunk in ((0, 1 << 16), (-1, 1 << 16), (1, 0), (1, -4), (1, 6), (1, 1023)):
            _bad(f(C.byref(_sgd()), state, OK, OK, nchunks, chunk, None))
    _bad(f(C.byref(_sgd()), ODD, OK, OK, 1, 1 << 16, None))


def test_fused_clip_sgd_validates_like_torch():
    from space_time_pde_amd.optim import FusedClipSGD
    p = [torch.nn.Parameter(torch.zeros(4))]
    for kw in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1), dict(momentum=-0.1)):
        with pytest.raises(ValueError):
            FusedClipSGD(p, lr=0.1, **kw)
        with pytest.raises(ValueError):
            torch.optim.SGD(p, lr=0.1, **kw)
    with pytest.raises(ValueError):
        FusedClipSGD(p, lr=-1.0)
    opt = FusedClipSGD(p, lr=0.1, momentum=0.9, nesterov=True, clip_grad=1.0, flat=False, capturable=True)
    assert opt.capturable and opt.defaults["capturable"] and not opt.defaults["flat"]
    assert opt.state_dict()["state"] == {}
    sd = torch.optim.SGD(p, lr=0.1, momentum=0.9).state_dict()
    sd["param_groups"][0]["maximize"] = True
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)


def test_capturable_flag_travels_in_defaults():
    import copy
    from space_time_pde_amd.optim import FusedClipAdam, FusedClipSGD
    p = [torch.nn.Parameter(torch.zeros(4))]
    for opt in (FusedClipAdam(p, capturable=True, flat=False), FusedClipSGD(p, lr=0.1, capturable=True, flat=False)):
        twin = copy.deepcopy(opt)
        assert twin.capturable and not twin._use_flat
        # a group written by torch's own optimizer says capturable=False: this instance's mode holds
        ref = (torch.optim.Adam if isinstance(opt, FusedClipAdam) else torch.optim.SGD)(p, lr=0.1)
        opt.load_state_dict(ref.state_dict())
        assert opt.capturable and opt.param_groups[0]["capturable"] is True
    assert not FusedClipAdam(p).capturable


def test_graphed_step_refuses_a_non_capturable_optimizer():
    """Checked before any GPU work: a captured FusedClipAdam(capturable=False) launch would freeze step 1's bias corrections."""
    from space_time_pde_amd.optim import FusedClipAdam
    from space_time_pde_amd.train_step import GraphedStep
    p = [torch.nn.Parameter(torch.zeros(4))]
    x = torch.zeros(1)
    for opt in (FusedClipAdam(p), torch.optim.SGD(p, lr=0.1)):
        with pytest.raises(ValueError, match="capturable"):
            GraphedStep(None, None, None, x, x, x, 1, optimizer=opt)


def test_capture_guards_and_table_staging(monkeypatch):
    """Inside a stream capture a capturable step may launch and nothing else: a changed learning rate is refused (its fill
    would be replayed), new pointers take the table buffers reserved BEFORE the capture (memory allocated inside one may
    alias the graph's temporaries) with their contents staged for ``flush_tables()``, and without a reserve the step refuses."""
    import numpy as np
    from space_time_pde_amd import optim
    p = [torch.nn.Parameter(torch.zeros(4))]
    opt = optim.FusedClipSGD(p, lr=0.1, flat=False, capturable=True)
    cap = dict(blk=None, lr=0.1, key=None, tab=None, chk=None, nchunks=0, pending=[], keep=[], spare=None)
    rows = [(4096, 8192, 0, 4, 0, 0)]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    opt._push_lr(cap, {"lr": 0.1})                                   # unchanged: nothing to do
    with pytest.raises(RuntimeError, match="inside a stream capture"):
        opt._push_lr(cap, {"lr": 0.05})
    with pytest.raises(RuntimeError, match="prepare"):
        opt._table(cap, rows, optim._SGD_TENSOR_DT, "cpu")
    opt._reserve_tables(cap, p, optim._SGD_TENSOR_DT)                # no allocation inside a capture
    assert cap["spare"] is None
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    opt._reserve_tables(cap, p, optim._SGD_TENSOR_DT)
    spare = cap["spare"]
    assert spare[0].numel() == optim._SGD_TENSOR_DT.itemsize and spare[1].numel() == optim._CHUNK_DT.itemsize
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    tab, chk, n = opt._table(cap, rows, optim._SGD_TENSOR_DT, "cpu")
    assert n == 1 and tab is spare[0] and chk is spare[1] and cap["spare"] is None
    assert len(cap["pending"]) == 2 and any(t is tab for t in cap["keep"]) and any(t is chk for t in cap["keep"])
    assert opt._table(cap, rows, optim._SGD_TENSOR_DT, "cpu")[0] is tab and len(cap["keep"]) == 2      # same pointers: reused
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    opt._cap[0] = cap
    opt.flush_tables()
    assert cap["pending"] == []
    assert tab.numpy().tobytes() == np.array(rows, dtype=optim._SGD_TENSOR_DT).tobytes()
    assert chk.numpy().tobytes() == np.array([(0, 0, 0)], dtype=optim._CHUNK_DT).tobytes()
    # new pointers after the capture: a NEW table, the captured one is neither rewritten nor released
    tab2 = opt._table(cap, [(4096, 16384, 0, 4, 0, 0)], optim._SGD_TENSOR_DT, "cpu")[0]
    assert tab2 is not tab and any(t is tab for t in cap["keep"])
    assert tab.numpy().tobytes() == np.array(rows, dtype=optim._SGD_TENSOR_DT).tobytes()
