"""Capturable optimizers on the GPU: FusedClipSGD and FusedClipAdam(capturable=True) against torch's optimizers, the
learning rate following ``group["lr"]`` through a captured graph, and ``GraphedStep(optimizer=...)`` -- the whole training
iteration in one HIP graph -- against the eager iteration, bit for bit."""
import copy

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

DEV = "cuda:0"
# shapes / seed / gradient scale / clip / lr of test_next_rows.test_fused_clip_adam_flat_buffers_and_fallbacks
SHAPES = [(64, 35), (64,), (7,), (16, 16, 3, 3, 3), (33, 5), (1,)]
CLIP, LR, TOL = 0.7, 3e-3, 3e-6          # 3e-6 absolute: the bound of the Adam tests on the same data scale

SGD_SETTINGS = {
    "plain": dict(),
    "momentum": dict(momentum=0.9),
    "momentum_dampening_wd": dict(momentum=0.9, dampening=0.1, weight_decay=0.01),
    "nesterov": dict(momentum=0.9, nesterov=True),
}


def _params(g):
    pa = [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in SHAPES]
    return pa, [p.detach().clone().requires_grad_(True) for p in pa]


def _set_grads(g, *param_lists, scale=2.0):
    grads = [torch.randn(s, generator=g).to(DEV) * scale for s in SHAPES]
    for ps in param_lists:
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()


def _maxdiff(pa, pb):
    return max((p - q).abs().max().item() for p, q in zip(pa, pb))


@pytest.mark.gpu
@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("setting", sorted(SGD_SETTINGS))
def test_fused_clip_sgd_matches_torch(hiplib, setting, flat, capturable):
    """stpde_clip_sgd / stpde_clip_sgd_multi == clip_grad_value_ + torch.optim.SGD over six steps (flat buffer and pointer
    table, host scalars and device state block), and the ``momentum_buffer`` checkpoint goes into torch.optim.SGD and back."""
    from space_time_pde_amd import _lib
    from space_time_pde_amd.optim import FusedClipSGD
    kw = SGD_SETTINGS[setting]
    g = torch.Generator().manual_seed(3)
    pa, pb = _params(g)
    oa = FusedClipSGD(pa, lr=LR, clip_grad=CLIP, flat=flat, capturable=capturable, **kw)
    ob = torch.optim.SGD(pb, lr=LR, **kw)
    for it in range(6):
        _set_grads(g, pa, pb)
        torch.nn.utils.clip_grad_value_(pb, CLIP)
        with _lib.dispatch_trace() as tr:
            oa.step()
        assert tr.has("k_clip_sgd @" if flat else "k_clip_sgd_multi @"), tr.kernels
        assert tr.has("k_opt_advance @") == capturable, tr.kernels
        ob.step()
        err = _maxdiff(pa, pb)
        print("sgd %s flat=%s capturable=%s step %d: max |p - torch| = %.3e" % (setting, flat, capturable, it, err))
        assert err < TOL
    if capturable:
        assert oa.device_step() == 6
    # checkpoint round trip: torch.optim.SGD <- FusedClipSGD and back
    sa = oa.state_dict()
    assert all(v._base is None for st in sa["state"].values() for v in st.values() if torch.is_tensor(v))
    if kw.get("momentum"):
        assert all(set(st) == {"momentum_buffer"} for st in sa["state"].values()) and len(sa["state"]) == len(SHAPES)
    ob2 = torch.optim.SGD(pb, lr=LR, **kw)
    ob2.load_state_dict(sa)
    oa2 = FusedClipSGD(pa, lr=LR, clip_grad=CLIP, flat=flat, capturable=capturable, **kw)
    oa2.load_state_dict(copy.deepcopy(ob2.state_dict()))
    for it in range(2):
        _set_grads(g, pa, pb, scale=1.0)
        torch.nn.utils.clip_grad_value_(pb, CLIP)
        oa2.step()
        ob2.step()
        err = _maxdiff(pa, pb)
        print("sgd %s after the round trip, step %d: %.3e" % (setting, it, err))
        assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False])
def test_capturable_sgd_checkpoint_before_the_first_step_has_no_buffers(hiplib, flat):
    """prepare() allocates the momentum buffers; until the first step they hold nothing and are not written into a checkpoint
    (torch.optim.SGD would take their zeros for history: momentum * 0 + (1 - dampening) * g instead of g)."""
    from space_time_pde_amd.optim import FusedClipSGD
    g = torch.Generator().manual_seed(5)
    pa, pb = _params(g)
    oa = FusedClipSGD(pa, lr=LR, momentum=0.9, dampening=0.5, flat=flat, capturable=True).prepare()
    assert oa.device_step() == 0 and all(st == {} for st in oa.state_dict()["state"].values())
    ob = torch.optim.SGD(pb, lr=LR, momentum=0.9, dampening=0.5)
    ob.load_state_dict(oa.state_dict())
    _set_grads(g, pa, pb)
    oa.step()
    ob.step()
    assert _maxdiff(pa, pb) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False])
def test_capturable_adam_matches_torch(hiplib, flat):
    """FusedClipAdam(capturable=True) -- step count, lr and both bias corrections on the device -- against clip_grad_value_ +
    torch.optim.Adam: six steps, the checkpoint round trip through torch.optim.Adam (which sets the device counter), and the
    refusal of a missing gradient."""
    from space_time_pde_amd import _lib
    from space_time_pde_amd.optim import FusedClipAdam
    g = torch.Generator().manual_seed(3)
    pa, pb = _params(g)
    oa = FusedClipAdam(pa, lr=LR, clip_grad=CLIP, weight_decay=0.01, flat=flat, capturable=True)
    ob = torch.optim.Adam(pb, lr=LR, weight_decay=0.01)
    for it in range(6):
        _set_grads(g, pa, pb)
        torch.nn.utils.clip_grad_value_(pb, CLIP)
        with _lib.dispatch_trace() as tr:
            oa.step()
        assert tr.has("k_opt_advance @") and tr.has("k_clip_adam_dev @" if flat else "k_clip_adam_multi_dev @"), tr.kernels
        ob.step()
        err = _maxdiff(pa, pb)
        print("adam capturable flat=%s step %d: max |p - torch| = %.3e" % (flat, it, err))
        assert err < TOL
    sa = oa.state_dict()
    sb = ob.state_dict()
    assert sa["state"][0].keys() == sb["state"][0].keys()
    assert all(float(st["step"]) == 6.0 and not st["step"].is_cuda for st in sa["state"].values())
    assert all(v._base is None for st in sa["state"].values() for v in st.values() if torch.is_tensor(v))
    ob2 = torch.optim.Adam(pb, lr=LR, weight_decay=0.01)
    ob2.load_state_dict(sa)
    oa2 = FusedClipAdam(pa, lr=LR, clip_grad=CLIP, weight_decay=0.01, flat=flat, capturable=True)
    oa2.load_state_dict(copy.deepcopy(ob2.state_dict()))        # a torch-written Adam checkpoint
    _set_grads(g, pa, pb, scale=1.0)
    torch.nn.utils.clip_grad_value_(pb, CLIP)
    oa2.step()
    ob2.step()
    assert oa2.device_step() == 7
    assert _maxdiff(pa, pb) < TOL
    pa[2].grad = None
    with pytest.raises(RuntimeError, match="ONE step count"):
        oa2.step()
    assert oa2.device_step() == 7


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False])
def test_capturable_adam_tracks_the_host_scalar_path_over_50_steps(hiplib, flat):
    """capturable=True against capturable=False on the same gradients over 50 steps.  Same kernel body (adam_elem); the only
    difference is where step_size and bias2_sqrt are computed: fp64 on the device (pow of the device library) against fp64 in
    Python (libm), both rounded to fp32 -- at most an fp32 rounding apart.  Bound: the project's 3e-6 (not tightened).
    Largest parameter difference observed on the MI355X (first hardware run, flat and table mode): 0.0 -- over these 50 steps
    the device's pow and libm's rounded to the same fp32 scalars every time."""
    from space_time_pde_amd.optim import FusedClipAdam
    g = torch.Generator().manual_seed(3)
    pa, pb = _params(g)
    oa = FusedClipAdam(pa, lr=LR, clip_grad=CLIP, weight_decay=0.01, flat=flat, capturable=True)
    ob = FusedClipAdam(pb, lr=LR, clip_grad=CLIP, weight_decay=0.01, flat=flat, capturable=False)
    worst = 0.0
    for it in range(50):
        _set_grads(g, pa, pb)
        oa.step()
        ob.step()
        worst = max(worst, _maxdiff(pa, pb))
    print("adam capturable vs host scalars, flat=%s, 50 steps: max |dp| = %.3e" % (flat, worst))
    assert oa.device_step() == 50
    assert worst < TOL


HOST_KINDS = {
    "adam": dict(),
    "sgd_momentum": dict(momentum=0.9, dampening=0.1),
    "sgd_plain": dict(),
}
# FusedClipSGD(flat=True): the steps that leave the flat kernel for the pointer table -- a missing gradient (steps 0 and 3)
# and, with momentum, step 1, where parameter 2 takes its first momentum step and the others their second
SGD_TABLE_STEPS = {"sgd_momentum": (0, 1, 3), "sgd_plain": (0, 3)}


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("kind", sorted(HOST_KINDS))
def test_host_scalar_fallbacks_match_torch_across_a_chunk_boundary(hiplib, kind, flat):
    """capturable=False over six steps with a missing gradient at step 0 (parameter 2) and at step 3 (parameter 4), on SHAPES
    plus a tensor of 65543 elements: one past the 65536-element chunk of the table kernels, i.e. a second chunk of one float4
    and a 3-element tail.  Against clip_grad_value_ (on the parameters that have a gradient) + torch.optim.Adam / SGD, which
    skip a parameter without a gradient; and the kernel each step takes: the pointer table for every ``flat=False`` step, for
    every Adam step (the step counts differ from step 0 on and never re-equalise) and for SGD's SGD_TABLE_STEPS, else the
    flat kernel."""
    from space_time_pde_amd import _lib
    from space_time_pde_amd.optim import _CHUNK, FusedClipAdam, FusedClipSGD
    assert _CHUNK == 65536
    shapes = SHAPES + [(_CHUNK + 7,)]
    missing = {0: 2, 3: 4}
    g = torch.Generator().manual_seed(3)
    pa = [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in shapes]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    kw = HOST_KINDS[kind]
    if kind == "adam":
        oa, ob, name = FusedClipAdam(pa, lr=LR, clip_grad=CLIP, flat=flat), torch.optim.Adam(pb, lr=LR), "k_clip_adam"
    else:
        oa, ob, name = FusedClipSGD(pa, lr=LR, clip_grad=CLIP, flat=flat, **kw), torch.optim.SGD(pb, lr=LR, **kw), "k_clip_sgd"
    for it in range(6):
        grads = [torch.randn(s, generator=g).to(DEV) * 2.0 for s in shapes]
        for k, (p, q, gr) in enumerate(zip(pa, pb, grads)):
            p.grad, q.grad = (None, None) if missing.get(it) == k else (gr.clone(), gr.clone())
        torch.nn.utils.clip_grad_value_([q for q in pb if q.grad is not None], CLIP)
        with _lib.dispatch_trace() as tr:
            oa.step()
        table = (not flat) or kind == "adam" or it in SGD_TABLE_STEPS[kind]
        print("%s flat=%s step %d: %s" % (kind, flat, it, tr.kernels))
        assert tr.has(name + "_multi @") == table and tr.has(name + " @") == (not table), (it, tr.kernels)
        assert len(tr.kernels) == 1, tr.kernels
        ob.step()
        err = _maxdiff(pa, pb)
        print("%s flat=%s step %d: max |p - torch| = %.3e" % (kind, flat, it, err))
        assert err < TOL


class _Ops(TorchDispatchMode):
    """Every torch operator dispatched inside the block (copies, fills, uploads included), but for the record_function
    markers torch.optim.Optimizer wraps around every ``step()`` (``profiler.*``: no tensor work)."""

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not str(func).startswith("profiler."):
            self.ops.append(str(func))
        return func(*args, **(kwargs or {}))


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_one_capturable_step_is_two_launches_and_no_upload(hiplib, kind, flat):
    """Dispatch trace of one capturable step once the lazy work is done: exactly the advance kernel and one update kernel
    from the library, and NO torch operator at all -- no copy for a table, no fill, no read-back."""
    from space_time_pde_amd import _lib
    from space_time_pde_amd.optim import FusedClipAdam, FusedClipSGD
    g = torch.Generator().manual_seed(7)
    pa, _ = _params(g)
    if kind == "adam":
        opt, upd = FusedClipAdam(pa, lr=LR, clip_grad=CLIP, flat=flat, capturable=True), "k_clip_adam"
    else:
        opt, upd = FusedClipSGD(pa, lr=LR, momentum=0.9, clip_grad=CLIP, flat=flat, capturable=True), "k_clip_sgd"
    upd += "_dev" if (kind == "adam" and flat) else ("" if flat else "_multi" + ("_dev" if kind == "adam" else ""))
    _set_grads(g, pa)
    opt.step()                                       # lazy work: buffers, state block, lr push, table
    tables = (opt._cap[0]["tab"], opt._cap[0]["chk"])
    for p in pa:                                     # new gradient VALUES at the same addresses
        p.grad.copy_(torch.randn(p.shape, generator=g).to(DEV))
    with _Ops() as ops, _lib.dispatch_trace() as tr:
        opt.step()
    assert len(tr.kernels) == 2 and tr.has("k_opt_advance @") and tr.has(upd + " @"), tr.kernels
    assert ops.ops == [], ops.ops
    assert opt._cap[0]["tab"] is tables[0] and opt._cap[0]["chk"] is tables[1] and (tables[0] is None) == flat
    # a scheduler's change costs one fill, nothing else
    opt.param_groups[0]["lr"] = LR / 2
    with _Ops() as ops:
        opt.step()
    assert len(ops.ops) <= 2 and any("fill_" in o for o in ops.ops) and not any("copy" in o for o in ops.ops), ops.ops
    assert opt.device_step() == 3


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_add_param_group_keeps_the_capturable_state(hiplib, kind, flat):
    """add_param_group after steps were taken: both optimizers rebuild their flat buffers / device state on the next step and
    carry on -- the old group at its step count (Adam) resp. with its momentum history (SGD), the new group from zero."""
    from space_time_pde_amd.optim import FusedClipAdam, FusedClipSGD
    g = torch.Generator().manual_seed(9)
    pa, pb = _params(g)
    if kind == "adam":
        oa = FusedClipAdam(pa[:4], lr=LR, clip_grad=CLIP, flat=flat, capturable=True)
        ob = torch.optim.Adam(pb[:4], lr=LR)
    else:
        oa = FusedClipSGD(pa[:4], lr=LR, momentum=0.9, dampening=0.5, clip_grad=CLIP, flat=flat, capturable=True)
        ob = torch.optim.SGD(pb[:4], lr=LR, momentum=0.9, dampening=0.5)
    for it in range(5):
        if it == 2:
            oa.add_param_group(dict(params=pa[4:]))
            ob.add_param_group(dict(params=pb[4:]))
        _set_grads(g, pa, pb)
        torch.nn.utils.clip_grad_value_(pb, CLIP)
        oa.step()
        ob.step()
        assert _maxdiff(pa, pb) < TOL, it
    # (SGD's count only tells the first step from the later ones: it restarts at 1 for a group with momentum history)
    assert oa.device_step(1) == 3 and oa.device_step(0) == (5 if kind == "adam" else 4)


# ---- the whole iteration in one graph -----------------------------------------------------------------------------------
B, N = 10, 512          # train_default: experiments/rb2d/run_experiment.sh:16, 10 crops x 512 points, latent (4,16,16)


def _models(seed):
    from space_time_pde_amd import implicit_net, physics, unet3d
    dev = torch.device(DEV)
    torch.manual_seed(seed)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=(4, 16, 16), nf=16, mf=256).to(dev).train()
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)

    def layer():
        return physics.get_rb2_pde_layer(mean=(0.01, 0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1.,
                                         x_crop=1., use_continuity=True)
    return unet, net, layer


def _draw(g):
    return (torch.randn(B, 4, 4, 16, 16, generator=g).to(DEV), (0.02 + 0.96 * torch.rand(B, N, 3, generator=g)).to(DEV),
            torch.randn(B, N, 4, generator=g).to(DEV))


@pytest.fixture
def deterministic():
    """_lib.deterministic = True, set before any forward and restored after: every accumulation of the step is then
    order-independent, so two runs of the same kernels on the same data agree bit for bit."""
    from space_time_pde_amd import _lib
    prev = _lib.deterministic
    _lib.deterministic = True
    try:
        yield
    finally:
        _lib.deterministic = prev


@pytest.mark.gpu
def test_learning_rate_follows_the_scheduler_without_recapture(hiplib, deterministic):
    """SGD without momentum inside GraphedStep: p' = p - lr * clip(g).  Two replays on identical inputs and identical (restored)
    parameters, ``group["lr"]`` halved in between (what ReduceLROnPlateau does, train.py:373-383): the second update is half the
    first.  Bound, element-wise, from fp32 rounding alone (u = 2^-24; lr/2 and lr/2 * g are exact halves): each p' carries
    u |p'|, each difference p' - p at most u |d| more, so |d2 - d1 / 2| <= 1.5 u (|p| + |d1|) (1 + o(1)) < 2^-23 (|p| + |d1|)."""
    from space_time_pde_amd.optim import FusedClipSGD
    from space_time_pde_amd.train_step import GraphedStep
    unet, net, layer = _models(21)
    params = list(unet.parameters()) + list(net.parameters())
    a = _draw(torch.Generator().manual_seed(22))
    opt = FusedClipSGD(params, lr=1e-2, clip_grad=1.0, flat=False, capturable=True)
    gstep = GraphedStep(unet, net, layer(), *a, N, 1.0, 0.0125, "l1", optimizer=opt)
    assert opt.device_step() == 0
    p0 = [p.detach().clone() for p in params]
    gstep()
    torch.cuda.synchronize()
    p1 = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, q in zip(params, p0):
            p.copy_(q)
    opt.param_groups[0]["lr"] = 0.5e-2
    gstep()
    torch.cuda.synchronize()
    assert opt.device_step() == 2 and gstep.replays == 2
    moved = 0
    for k, (p, q0, q1) in enumerate(zip(params, p0, p1)):
        d1, d2 = q1 - q0, p.detach() - q0
        moved += int((d1 != 0).sum())
        bound = 2.0 ** -23 * (q0.abs() + d1.abs())
        worst = ((d2 - 0.5 * d1).abs() - bound).max().item()
        assert worst <= 0, (k, worst, d1.abs().max().item())
    assert moved > 0.5 * sum(p.numel() for p in params)


def _optimizer(kind, params, flat):
    from space_time_pde_amd.optim import FusedClipAdam, FusedClipSGD
    if kind == "adam":
        return FusedClipAdam(params, lr=1e-2, clip_grad=1.0, flat=flat, capturable=True)
    return FusedClipSGD(params, lr=1e-2, momentum=0.9, clip_grad=1.0, flat=flat, capturable=True)


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("kind", ["adam", "sgd_momentum"])
def test_whole_iteration_graph_equals_the_eager_iteration(hiplib, deterministic, kind, flat):
    """GraphedStep(optimizer=opt) on the train_default shapes: 3 replays against 3 eager iterations (sharded_step + opt.step())
    of a twin model with the same capturable optimizer class and the same initial state, in the deterministic mode -- the same
    kernels on the same scalars, so every parameter, every moment / momentum buffer and the step count must be BIT-EQUAL.
    Construction alone does not train (parameters, state, step count bit-identical to before), and ``optimizer.zero_grad()``
    between replays changes nothing: the captured update reads the graph's static gradients by address."""
    from space_time_pde_amd import _lib, local_implicit_grid as lig
    from space_time_pde_amd.train_step import GraphedStep, sharded_step
    assert _lib.deterministic
    unet, net, layer = _models(11)
    unet2, net2 = copy.deepcopy(unet), copy.deepcopy(net)
    pa = list(unet.parameters()) + list(net.parameters())
    pb = list(unet2.parameters()) + list(net2.parameters())
    g = torch.Generator().manual_seed(12)
    inputs = [_draw(g) for _ in range(3)]
    oa, ob = _optimizer(kind, pa, flat).prepare(), _optimizer(kind, pb, flat).prepare()
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))
    before = [t.clone() for t in [p.data for p in pa] + oa.state_tensors()]
    n0 = lig.stats["hip_jet_calls"]
    gstep = GraphedStep(unet, net, layer(), *inputs[0], N, 1.0, 0.0125, "l1", optimizer=oa)
    torch.cuda.synchronize()
    assert lig.stats["hip_jet_calls"] > n0
    after = [p.data for p in pa] + oa.state_tensors()
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))   # construction did not train
    assert oa.device_step() == 0
    layer2 = layer()
    for k, inp in enumerate(inputs):
        loss_g = gstep(*inp)[0].clone()
        oa.zero_grad()                                   # the trap of the eager-optimizer arrangement: harmless here
        assert all(p.grad is None for p in pa)
        for p in pb:
            p.grad = None
        loss_e, _, _ = sharded_step(unet2, net2, layer2, *inp, N, 1.0, 0.0125, "l1", distributed=False)
        ob.step()
        torch.cuda.synchronize()
        assert torch.equal(loss_g, loss_e), (k, float(loss_g), float(loss_e))
        bad = [i for i, (p, q) in enumerate(zip(pa, pb)) if not torch.equal(p, q)]
        assert not bad, (k, bad[:8], max((pa[i] - pb[i]).abs().max().item() for i in bad))
    sa, sb = oa.state_tensors(), ob.state_tensors()
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))     # state blocks and moments
    assert oa.device_step() == ob.device_step() == 3 and gstep.replays == 3
    da, db = oa.state_dict(), ob.state_dict()
    for i in da["state"]:
        for name, v in da["state"][i].items():
            assert torch.equal(v, db["state"][i][name]), (i, name)
