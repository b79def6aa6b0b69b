"""Hot-path benchmark: query-points/sec of one MeshfreeFlowNet training step (fwd + PDE residuals + bwd).

    python bench.py --gpus N --steps K --warmup W

N > 1: one rank per GPU over RCCL.  Under ``python -m torch.distributed.run`` (RANK / WORLD_SIZE in the environment) every
process is one rank; a plain ``python bench.py --gpus N`` spawns its N ranks itself (torch.multiprocessing.spawn on
127.0.0.1, as the reference's experiments/rb2d/train_ddp.py:483-494 does) -- both routes run the same ``main``.

A "step" is one pass of the hot path over one batch of synthetic input (experiments/rb2d/train.py:58-77 of the
reference): UNet3d encoder -> latent grid -> local-implicit-grid gather -> IM-NET on every query point with the RB2
residual derivatives -> L1 losses -> backward to all IM-NET and UNet parameters.  Workload = BASELINE.json
configs[1]: input crop [1, 4, 32, 128, 128], latent grid [1, 32, 128, 128, 32] (T, Z, X, C), 2^20 query points,
full Rayleigh-Benard PDE set (3 transport equations + continuity), fp32.  With N GPUs the SAME 2^20 points are
sharded across ranks (strong scaling): every rank runs the (cheap, deterministic) UNet on the same crop, the
partial d(loss)/d(latent grid) and the IM-NET gradients are summed with RCCL all-reduces, and the UNet backward
is replicated.

Prints ONE JSON line (rank 0) with the contract fields (``metric``, ``value``, ``unit``, ``higher_is_better``, ``dtype``,
``ms_per_step`` = wall time of one timed step).  A plain run does only that: set up, warm up, time ``--steps`` steps, write
the outputs (``--dump-outputs DIR``) and print the line.  ``--full`` adds everything else the line used to carry, each
measured after the timed region: ``roofline`` (dominant kernel, HIP-event timed), per-rank and collective diagnostics,
side figures, the fp32x3 second line, ``other_configs`` (child runs) and ``cpu_baseline`` (the CPU oracle = restatement
of the reference path, timed on the host cores on a bounded sample).

``--dump-outputs DIR`` writes what the last timed step returned to its caller -- the losses and the gradient of every
parameter, summed over ranks (the launch-bound workloads: also the parameters after the optimizer step) -- as
``DIR/<name>.npy`` in float32, at most 64 MB in all.  Inputs and initial weights are seeded and the step workloads (c2, c5)
run in the library's deterministic mode (``reproducible_mode``), so the same arguments give the same outputs every run and
two builds can be compared output for output; ``--nondeterministic`` times the library's default mode instead, and the line
says which mode ran (``deterministic``).  The launch-bound workloads (train_default, c1) are not switched -- the
deterministic mode nearly doubles their step time -- and their dumps agree between runs only to the drift of an optimizer
loop fed with fp32-atomic gradients.  The child runs of ``other_configs`` keep the default mode of their earlier figures.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# BASELINE configs[4] / SURVEY 8(d) C5: 3 inputs (x, y, t), 5 outputs (c, u, v, w, p), user strings.  The first is SURVEY's
# advection-diffusion string with k = 0.01; together the four are the set pinned against the imported reference by fixture
# G9 (tests/golden/make_golden.py: g9_generic) -- every channel appears, second derivatives xx, yy, xy, tt.
C5_VARS = ("x, y, t", "c, u, v, w, p")
C5_EQS = {
    "adv_diff": "dif(c,t)+u*dif(c,x)+v*dif(c,y)-0.01*(dif(dif(c,x),x)+dif(dif(c,y),y))",
    "prod_rule": "dif(u*c,x)+dif(v*c,y)",
    "mixed": "dif(dif(c,x),y)-w*p",
    "explicit_x": "x*dif(p,x)+t*dif(dif(p,t),t)",
}
MEAN, STD = (0.01, 0.0, 0.02, -0.01), (0.05, 0.3, 0.15, 0.12)
RB2 = dict(mean=MEAN, std=STD, t_crop=2., z_crop=1., x_crop=1., use_continuity=True)
ALPHA_REG, ALPHA_PDE = 1.0, 0.0125
PEAK_F32_TFLOPS = 157.3      # MI355X_MICROARCH.md: fp32 MFMA = fp32 vector peak


def algorithmic_macs(nf=32, cin=32, cout=4, n_first=3, n_second=2):
    """Per CORNER ROW multiply-accumulates of each kernel (hidden blocks carry all streams,
    the raw-input (skip) blocks only the value stream; 1 MAC = 2 FLOP)."""
    dz = 3 + cin
    widths = [16 * nf, 8 * nf, 4 * nf, 2 * nf, nf, cout]
    S = 1 + n_first + n_second
    macs = {}
    for l in range(1, 6):
        hidden = widths[l - 1] * widths[l]
        skip = dz * widths[l] if l < 5 else 0
        macs["layer%d_fwd" % l] = S * hidden + skip + (dz * widths[0] if l == 1 else 0)
        macs["layer%d_dgrad" % l] = S * hidden
        macs["layer%d_wgrad" % l] = S * hidden + skip
    macs["layer0_wgrad"] = dz * widths[0]
    macs["layer1_bwd"] = macs["layer1_dgrad"] + macs["layer1_wgrad"]       # bf16 mode: one kernel (csrc/jet_fc1_bwd.hip)
    T = sum(widths[l - 1] * widths[l] for l in range(1, 6))          # hidden-to-hidden blocks: every stream
    M = T + dz * sum(widths[:5])                                       # value pass also has the raw-input blocks
    return macs, M, T


def algorithmic_bytes(S, smooth_sp0=4, nf=32, cin=32, cout=4, packed=False):
    """Per CORNER ROW HBM bytes each layer kernel has to move (X = augmented raw input): the roofline numerator of a kernel
    that is HBM-bound.  fp32 stash of S streams, or -- packed=True, the bf16 mode's layer buffers -- a
    packed STASH per feature 4 + 2 (S - 1) bytes (value stream fp32, derivative streams bf16) and a packed ADJOINT 2 S bytes;
    the layer-0 adjoint is its value stream only (bf16), the z0 stash fp32."""
    widths = [16 * nf, 8 * nf, 4 * nf, 2 * nf, nf, 16]     # fc5 output padded to one 16-feature tile
    xb = 3 * 16 * 4
    by = {}
    if packed:
        stash = lambda l: (4 + 2 * (S - 1)) * widths[l] if l < 5 else 4 * S * widths[l]
        adj = lambda l: 2 * S * widths[l] if l < 5 else 4 * S * widths[l]
        for l in range(1, 6):
            by["layer%d_fwd" % l] = (stash(l - 1) if l > 1 else 0) + xb + stash(l) + (4 * widths[0] if l == 1 else 0)
            by["layer%d_dgrad" % l] = adj(l) + ((stash(l - 1) + adj(l - 1)) if l > 1 else xb + (4 + 2) * widths[0])
            by["layer%d_wgrad" % l] = adj(l) + (stash(l - 1) if l > 1 else 4 * widths[0]) + 2 * xb     # (l = 1: the z0 stash)
        by["layer0_wgrad"] = 2 * widths[0] + xb
        # fused backward of the first hidden layer: the adjoint tile once for both products + once more for the raw-input
        # columns' own launch, z0 read, layer-0 adjoint written
        by["layer1_bwd"] = 2 * adj(1) + (4 + 2) * widths[0] + 2 * xb
        return by
    for l in range(1, 6):
        out_b, in_b = 4 * S * widths[l], (4 * S * widths[l - 1] if l > 1 else 0)
        by["layer%d_fwd" % l] = in_b + xb + out_b
        by["layer%d_dgrad" % l] = out_b + (2 * in_b if l > 1 else xb + 4 * smooth_sp0 * widths[0])
        by["layer%d_wgrad" % l] = out_b + (in_b if l > 1 else 4 * widths[0]) + 2 * xb       # (l = 1: the z0 stash)
    by["layer0_wgrad"] = 4 * smooth_sp0 * widths[0] + xb
    return by


def make_inputs(n_pts, dev, seed=0, igres=(32, 128, 128), n_out=4):
    g = torch.Generator().manual_seed(seed)
    crop = torch.randn(1, 4, *igres, generator=g).to(dev)
    pts = torch.rand(1, n_pts, 3, generator=g).to(dev)
    tgt = torch.randn(1, n_pts, n_out, generator=g).to(dev)
    return crop, pts, tgt


DUMP_LIMIT_BYTES = 60 * 10 ** 6      # --dump-outputs: at most 64 MB in all, .npy headers included


def step_outputs(losses, modules, with_params=False):
    """What one step hands its caller: the losses, the gradient of every parameter (and, after an optimizer step, the
    parameters themselves), keyed by file name."""
    out = dict(zip(("loss", "reg_loss", "pde_loss"), losses))
    for prefix, m in modules:
        for name, p in m.named_parameters():
            if p.grad is not None:
                out["grad.%s.%s" % (prefix, name)] = p.grad
            if with_params:
                out["param.%s.%s" % (prefix, name)] = p
    return out


def reproducible_mode(args):
    """Unless ``--nondeterministic`` is given, the benchmarked step runs in the library's deterministic mode:
    every sum the step accumulates with atomics -- U-Net convolution weight / bias gradients, BatchNorm statistics and
    backward sums, IM-NET weight gradients, the loss sums -- goes to order-independent long accumulators, so the same
    arguments give bit-identical losses and gradients run after run.  In the default mode the U-Net's deepest BatchNorm
    levels, which normalise over a handful of voxels, amplify the atomics' summation-order rounding into differences of
    ~0.5 % of its gradient between runs.  Set in ``main`` and not at import: tests import this module for its constants.
    Returns the mode the step runs in (``--nondeterministic`` leaves STPDE_DETERMINISTIC in charge)."""
    from space_time_pde_amd import _lib
    if not args.nondeterministic:
        _lib.deterministic = True
    return bool(_lib.deterministic)


def dump_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES):
    """Write {name: tensor} as DIR/<name>.npy: float64 tensors as float64, everything else as float32.  When the arrays
    together exceed ``limit`` bytes, every array of more than 4096 elements is replaced by a fixed sample of its flattened
    elements: the sorted first k of a permutation seeded by 0, k the same fraction of every array -- the indices depend
    only on the array's size and the total, so two builds run with the same arguments write the same sample."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        t = t.detach()
        host[name] = t.to("cpu", torch.float64 if t.dtype == torch.float64 else torch.float32)
    total = sum(a.numel() * a.element_size() for a in host.values())
    floors = sum(4096 * a.element_size() for a in host.values())     # (an array is never cut below 4096 elements)
    frac = 1.0 if total <= limit else max(0.0, limit - floors) / total
    for name, a in sorted(host.items()):
        if frac < 1.0 and a.numel() > 4096:
            g = torch.Generator().manual_seed(0)
            k = max(4096, int(a.numel() * frac))
            idx = torch.randperm(a.numel(), generator=g)[:k].sort().values
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), a.numpy())


def c5_layer(pde_module):
    layer = pde_module.PDELayer(*C5_VARS)
    for name, eq in C5_EQS.items():
        layer.add_equation(eq, name)
    return layer


def cpu_baseline(act, chunk=1024, nchunks=16):
    """Time the CPU oracle (restatement of the reference's 25-reverse-sweep path) on a bounded sample (~40 s).

    Sample: 16 chunks of 1024 points = the reference's own unit of work (train.py:230 n_samp_pts_per_crop and
    :245 pseudo_batch_size default to 1024), plus ONE chunk of 4096 points for continuity with the rounds-1/2 figure.
    The host may have far more cores than the op-level parallelism of this graph can use (128 threads ran 7x slower
    than 16 on the GPU box), so the thread count is calibrated on a chunk first and reported as ``cores``
    (profiles/r2_cpu_ref_vs_port.json: the restatement takes 1.12-1.30x the time of the imported reference).
    """
    from oracle import cpu_ref
    g = torch.Generator().manual_seed(0)
    latent = 0.5 * torch.randn(1, 32, 128, 128, 32, generator=g)
    params = cpu_ref.imnet_init(nf=32, seed=1)
    pde = cpu_ref.rb2_oracle(**RB2)

    def run(n):
        pts = torch.rand(1, n, 3, generator=g)
        tgt = torch.randn(1, n, 4, generator=g)
        t0 = time.perf_counter()
        cpu_ref.lig_pde_step(params, act, latent, pts, tgt, pde, ALPHA_REG, ALPHA_PDE)
        return time.perf_counter() - t0

    ncpu = os.cpu_count() or 8
    best, best_t = None, 1e30
    run(256)                                   # warm-up (sympy lambdify, allocator)
    for nt in sorted({min(ncpu, c) for c in (8, 16, 32)}):
        torch.set_num_threads(nt)
        t = run(chunk)
        if t < best_t:
            best, best_t = nt, t
    torch.set_num_threads(best)
    times = sorted(run(chunk) for _ in range(nchunks))
    total = sum(times)
    t4k = run(4096)
    return dict(value=nchunks * chunk / total, unit="query-points/s", cores=best, kind="port",
                value_chunk4096=4096 / t4k,
                sample="%d chunks of %d points (the reference's default points per crop, train.py:230) over the same "
                       "[1,32,128,128,32] latent grid (UNet excluded: <1%% of the work), %s, %d threads (best of 8/16/32 on "
                       "this host, %d logical CPUs), %.1f s in total, chunk min / median / max %.2f / %.2f / %.2f s; one "
                       "4096-point chunk: %.2f s; the reference path cannot hold 2^20 points at once and pseudo-batches "
                       "(evaluation.py:54-60)"
                       % (nchunks, chunk, act, best, ncpu, total, times[0], times[len(times) // 2], times[-1], t4k))


def other_configs(args):
    """BASELINE configs[3] and configs[4] in front of the driver: each is a child run of THIS script (its own
    process: configs[4] alone peaks at 192 GB) after the headline's timed region, >= 5 timed steps, same bracket; the child's
    whole line is condensed to ms_per_step / points per second / dominant kernel / its fractions."""
    import gc
    import subprocess
    gc.collect()
    torch.cuda.empty_cache()
    runs = [("configs[3]", ["--igres", "64", "256", "256", "--mlp-precision", "bf16"]),
            ("configs[4]", ["--workload", "c5"]),
            ("train_default", ["--workload", "train_default", "--steps", "50"]),
            ("configs[0]", ["--workload", "c1", "--steps", "50"])]
    steps, warm = max(5, min(args.steps, 8)), 2
    out = {}
    for name, extra in runs:
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(steps), "--warmup", str(warm),
               "--points", str(args.points), "--act", args.act, "--full", "--nondeterministic", "--no-cpu-baseline", "--no-other-configs",
               "--sub"] + extra
        rec = dict(cmd="python bench.py " + " ".join(cmd[2:]))
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                rec["error"] = "rc %d: %s" % (r.returncode, r.stderr[-400:])
            else:
                j = json.loads(line[-1])
                rf = j["roofline"]
                if "dispatches_per_step" in j:          # the launch-bound workloads (small_workload)
                    rec.update({k: j[k] for k in ("ms_per_step", "value", "unit", "steps", "launch_mode", "ms_per_step_eager",
                                                  "ms_per_step_eager_no_readback", "ms_per_step_graph",
                                                  "ms_per_step_graph_no_readback", "graph_error", "dispatches_per_step",
                                                  "kernel_ms_per_step", "step_over_kernel_time", "step_over_kernel_time_eager")})
                    rec.update(workload=j["config"]["workload"], loss=j["config"]["loss"])
                    out[name] = rec
                    continue
                rec.update(workload=j["config"]["workload"], dtype=j["dtype"], steps=j["steps"], warmup=j["warmup"],
                           ms_per_step=round(j["ms_per_step"], 3), value=round(j["value"]), unit=j["unit"],
                           ms_per_step_hip_event_median=j["ms_per_step_hip_event_median"], peak_GB=j["peak_GB"],
                           recompute_steps=j["recompute_steps"], loss=j["config"]["loss"],
                           dominant_kernel=rf["kernel"], dominant_avg_launch_ms=rf["avg_launch_ms"], bound=rf["bound"],
                           frac=rf["frac"], peak=rf["peak"], achieved=rf["achieved"], roof_unit=rf["unit"],
                           executed_frac=rf.get("executed_frac"), kernels=rf["kernels"])
                for side in ("hbm_side", "mfma_side"):
                    if side in rf:
                        rec[side] = {k: rf[side][k] for k in ("achieved", "peak", "unit", "frac") if k in rf[side]}
                for k in ("step_frac_per_gpu", "step_algorithmic_tflops", "stream_set"):
                    if k in rf:
                        rec[k] = rf[k]
        except (subprocess.TimeoutExpired, ValueError, KeyError) as e:
            rec["error"] = "%s: %s" % (type(e).__name__, e)
        out[name] = rec
    return out



SMALL_WORKLOADS = {
    # the reference's own training regime: experiments/rb2d/run_experiment.sh:16 (--batch_size_per_gpu=10 --n_samp_pts_per_crop=512
    # --nonlin=softplus --use_continuity=true --alpha_pde=0.0125) on train.py's defaults (nt=16, nz=nx=128, downsamp_t=4,
    # downsamp_xz=8 -> low-resolution crop / latent grid (4,16,16); unet_nf=16, unet_mf=256, imnet_nf=32, lr=1e-2,
    # clip_grad=1): 5,120 query points per step
    "train_default": dict(batch=10, igres=(4, 16, 16), points=512, name="reference training regime (run_experiment.sh:16): "
                          "10 crops x 512 points, latent [10,4,16,16,32], UNet3d(igres=(4,16,16), nf=16, mf=256)"),
    # BASELINE configs[0] on the GPU (the reference's CPU-runnable case, fixture G8): one 32x32x16 crop, 4096 points
    "c1": dict(batch=1, igres=(16, 32, 32), points=4096, name="BASELINE configs[0]: one low-resolution crop [1,4,16,32,32], 4096 "
               "points, UNet3d(igres=(16,32,32), nf=16, mf=256)"),
}


def small_workload(args):
    """Launch-bound workloads (VERDICT r5 missing #2 / next #4): the WHOLE training iteration of experiments/rb2d/train.py:55-84
    -- zero_grad, U-Net, LIG + IM-NET + RB2 residuals, L1 losses, backward, clip_grad_value_ + Adam (one fused launch), the
    per-step ``loss.item()`` read-back the reference does -- timed (a) eagerly and (b) with forward + backward captured in a HIP
    graph (train_step.GraphedStep) and replayed.  ``value`` is the graph path when the capture succeeds.  Also reported: the
    kernel dispatches of one step and the sum of their device time (torch.profiler / roctracer), so that "step <= 2 x kernel
    time" can be read off the line."""
    spec = SMALL_WORKLOADS[args.workload]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from space_time_pde_amd import _lib, implicit_net, lig_jet, local_implicit_grid as lig, nonlinearities, optim, physics, unet3d
    from space_time_pde_amd.train_step import GraphedStep, sharded_step
    torch.manual_seed(1)
    B, N, igres = spec["batch"], spec["points"], spec["igres"]
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32,
                             activation=nonlinearities.NONLINEARITIES[args.act]).to(dev)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=igres, nf=16, mf=256).to(dev).train()
    layer = physics.get_rb2_pde_layer(**RB2)
    g = torch.Generator().manual_seed(0)
    crop = torch.randn(B, 4, *igres, generator=g).to(dev)
    pts = torch.rand(B, N, 3, generator=g).to(dev)
    tgt = torch.randn(B, N, 4, generator=g).to(dev)
    params = list(unet.parameters()) + list(net.parameters())
    # the forward + backward of the step captured in a HIP graph FIRST (before any optimizer step and any profiler activity in
    # this process): the graph holds the parameters' addresses, so the optimizer below runs with flat=False (pointer-table
    # kernel, storages untouched -- optim.FusedClipAdam's flat mode would re-point every p.data into its own buffer)
    gstep = graph_err = None
    if not args.profile_only:
        try:
            gstep = GraphedStep(unet, net, layer, crop, pts, tgt, N, ALPHA_REG, ALPHA_PDE, "l1")
            ggrads = [p.grad for p in params]
        except Exception as e:  # noqa: BLE001
            graph_err = "%s: %s" % (type(e).__name__, str(e)[:400])
            gstep = None
    opt = optim.FusedClipAdam(params, lr=1e-2, clip_grad=1.0, flat=False)    # train.py:205, :79-83, :330-333

    def eager_step():
        for p in params:
            p.grad = None                                                  # optimizer.zero_grad()
        loss, _, _ = sharded_step(unet, net, layer, crop, pts, tgt, N, ALPHA_REG, ALPHA_PDE, "l1", distributed=False)
        opt.step()
        return loss

    def timed(fn, steps, item=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = fn()
            if item:
                v = loss.item()                                            # train.py:84 ``tot_loss += loss.item()``
        torch.cuda.synchronize()
        last_loss[0] = loss
        return 1e3 * (time.perf_counter() - t0) / steps, float(loss)

    last_loss = [None]
    n0 = lig.stats["hip_jet_calls"]
    for _ in range(max(args.warmup, 3)):
        eager_step()
    if args.profile_only:
        # child run of this workload: kernel dispatches and device time of ONE eager step through torch.profiler (roctracer).
        # In a process of its own: a profiler that is unavailable or crashes must not cost the parent its line.
        from torch.profiler import ProfilerActivity, profile
        nprof = 3
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(nprof):
                eager_step()
            torch.cuda.synchronize()
        kev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower()]
        ksum = sum((getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)) for e in kev) / 1e3 / nprof
        rec = dict(dispatches_per_step=len(kev) / float(nprof), kernel_ms_per_step=ksum)
        print(json.dumps(rec))
        return rec
    import gc
    # eager timings: the headline when the capture failed, diagnostics (--full) beside the graph's otherwise
    ms_eager = ms_eager_async = loss_e = None
    n_eager = max(args.warmup, 3)
    if args.full or gstep is None:
        gc.collect()
        gc.disable()
        ms_eager, loss_e = timed(eager_step, args.steps)
        n_eager += args.steps
        if args.full:
            ms_eager_async, _ = timed(eager_step, args.steps, item=False)
            n_eager += args.steps
        gc.enable()
    assert lig.stats["hip_jet_calls"] == n0 + n_eager, "HIP jet path was not taken"
    # the same iteration with forward + backward replayed from the HIP graph
    ms_graph = ms_graph_async = loss_g = None
    if gstep is not None:
        def graph_step():
            loss, _, _ = gstep()
            for p, gr in zip(params, ggrads):                              # (the graph's static gradient tensors)
                p.grad = gr
            opt.step()
            return loss

        for _ in range(max(args.warmup, 3)):                               # the graph path's own warm-up
            graph_step()
        gc.collect()
        gc.disable()
        ms_graph, loss_g = timed(graph_step, args.steps)
        if args.full:
            ms_graph_async, _ = timed(graph_step, args.steps, item=False)
        gc.enable()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, step_outputs([last_loss[0]], [("unet", unet), ("imnet", net)], with_params=True))
    # dispatches and device time of ONE eager step (--full): a child run of this script (see --profile-only above); the
    # library's own dispatch trace (its kernels only, torch's elementwise / cat / copy launches not seen) if that fails
    disp = ksum = prof_err = None
    if args.full:
        try:
            import subprocess
            cmd = [sys.executable, os.path.abspath(__file__), "--workload", args.workload, "--act", args.act, "--profile-only"]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode == 0 and line:
                j = json.loads(line[-1])
                disp, ksum = j["dispatches_per_step"], j["kernel_ms_per_step"]
            else:
                prof_err = "child rc %d: %s" % (r.returncode, r.stderr[-300:])
        except Exception as e:  # noqa: BLE001
            prof_err = "%s: %s" % (type(e).__name__, e)
        if disp is None:
            with _lib.dispatch_trace() as tr:
                eager_step()
            disp = float(len(tr.kernels))
    ms = ms_graph if ms_graph is not None else ms_eager
    pts_step = B * N
    out = {
        "metric": "query-points/sec (whole training iteration: fwd + PDE-residual bwd + clip + Adam), rb2d",
        "value": pts_step / (ms * 1e-3), "unit": "query-points/s", "n_gpus": 1, "steps": args.steps, "warmup": max(args.warmup, 3),
        "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "deterministic": bool(_lib.deterministic),
        "launch_mode": "HIP graph replay (forward + backward captured once; optimizer launch + loss read-back per step)"
                       if ms_graph is not None else "eager",
        "ms_per_step_eager": None if ms_eager is None else round(ms_eager, 3),
        "ms_per_step_eager_no_readback": None if ms_eager_async is None else round(ms_eager_async, 3),
        "ms_per_step_graph": None if ms_graph is None else round(ms_graph, 3),
        "ms_per_step_graph_no_readback": None if ms_graph_async is None else round(ms_graph_async, 3),
        "graph_error": graph_err,
        "dispatches_per_step": disp, "kernel_ms_per_step": None if ksum is None else round(ksum, 3),
        "step_over_kernel_time": None if not ksum else round(ms / ksum, 2),
        "step_over_kernel_time_eager": None if not ksum or ms_eager is None else round(ms_eager / ksum, 2),
        "profiler_error": prof_err,
        "config": {"workload": spec["name"] + ", RB2 (3 transport + continuity), ImNet nf=32 %s, L1 losses, alpha_pde=0.0125, "
                   "FusedClipAdam(lr=1e-2, clip_grad=1)" % args.act, "points": pts_step, "batch": B,
                   "loss": loss_g if loss_g is not None else loss_e},
        "roofline": {"bound": "launch latency", "kernel": None, "achieved": None, "peak": None, "unit": None, "frac": None,
                     "traffic": None,
                     "note": "a %d-point step is ~%d dispatches of microseconds each: no kernel of this workload is near a "
                             "hardware roof; the figure of merit is step time over the sum of kernel time (below 1 when the "
                             "graph's side-stream branches overlap)" % (pts_step, int(disp))} if args.full else None,
    }
    print(json.dumps(out))
    return out

def _spawn_rank(rank, world, port, argv):
    """One self-spawned rank: the environment torch.distributed.run would have set, then the ordinary main()."""
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    main(argv)


def self_spawn(world, argv):
    """``python bench.py --gpus N`` without a launcher: spawn the N ranks (reference: train_ddp.py:491-494, mp.spawn)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_spawn_rank, args=(world, port, argv), nprocs=world, join=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--act", default="softplus", help="softplus = reference run_experiment.sh:16; leakyrelu = module default")
    ap.add_argument("--chunk", type=int, default=1 << 20, help="points per launch chunk")
    ap.add_argument("--mlp-precision", default="fp32", choices=["fp32", "bf16", "fp32x3"],
                    help="fp32 = the headline / parity path; bf16 = BASELINE configs[3]: bf16 MFMA operands in the "
                         "wide IM-NET layers, fp32 accumulation (NOT the headline metric)")
    ap.add_argument("--igres", type=int, nargs=3, default=[32, 128, 128], metavar=("T", "Z", "X"),
                    help="latent grid; 64 256 256 = BASELINE configs[3]")
    ap.add_argument("--workload", default="c2", choices=["c2", "c5", "train_default", "c1"],
                    help="c2 = BASELINE configs[1] (RB2 + continuity, 4 outputs; with --igres 64 256 256 --mlp-precision bf16: "
                         "configs[3]); c5 = BASELINE configs[4]: 5-output user-string advection-diffusion equation set "
                         "(the strings pinned by fixture G9: products, a mixed second derivative, explicit coordinates)")
    ap.add_argument("--mem-budget-gb", type=float, default=None,
                    help="device-memory budget of the jet call's stash + scratch (lig_jet.set_memory_budget): above it the "
                         "backward recomputes the forward chunk by chunk; the line reports peak_GB either way")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the diagnostics: roofline / per-kernel times, per-rank and "
                         "collective figures, side figures, the fp32x3 line, other_configs, cpu_baseline (off: the plain "
                         "run times the steps and prints the contract fields only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (losses, parameter gradients) as DIR/<name>.npy")
    ap.add_argument("--nondeterministic", action="store_true",
                    help="time the library's default mode (fp32 atomics) instead of its deterministic mode; the outputs of "
                         "two runs then agree only to amplified summation-order rounding.  The launch-bound workloads "
                         "(train_default, c1) are never switched to the deterministic mode")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the `other_configs` block (BASELINE configs[3] and configs[4], each timed by a child run of this "
                         "script after the headline's timed region) and the second headline-grade line `value_fp32x3`")
    ap.add_argument("--sub", action="store_true", help=argparse.SUPPRESS)   # child run of `other_configs`: no side figures
    ap.add_argument("--profile-only", action="store_true", help=argparse.SUPPRESS)   # child run of a launch-bound workload
    ap.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"),
                    help="per-launch HBM bytes of each kernel from the committed rocprofv3 --pmc runs")
    args = ap.parse_args(argv)
    if args.mlp_precision == "bf16" and args.traffic_json == ap.get_default("traffic_json"):
        # the bf16-operand kernels have their own counter passes (taken on configs[3]; the IM-NET launches are the same on
        # either latent grid: 2^20 points, same kernels)
        args.traffic_json = os.path.join(ROOT, "profiles", "pmc_traffic_c4_bf16.json")
    if args.workload in SMALL_WORKLOADS:
        return small_workload(args)
    det = reproducible_mode(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_spawn(args.gpus, list(sys.argv[1:] if argv is None else argv))

    # stdout carries exactly ONE line (the JSON record): libraries that print to file descriptor 1 (RCCL announces its
    # path there when the process group comes up) are sent to stderr until the record is written
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE=%d of the launcher" % (args.gpus, world))
    # test hooks for the 1-GPU box (never set by the driver): all ranks on device 0 / another backend than RCCL, so that
    # `--gpus 2` can be dry-run through gloo where RCCL would refuse two ranks on one device
    if os.environ.get("STPDE_BENCH_ONE_DEVICE") == "1":
        local = 0
    backend = os.environ.get("STPDE_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from space_time_pde_amd import implicit_net, lig_jet, local_implicit_grid as lig, nonlinearities, physics, unet3d

    torch.manual_seed(1)
    c5 = args.workload == "c5"
    n_out = 5 if c5 else 4
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=n_out, nf=32,
                             activation=nonlinearities.NONLINEARITIES[args.act]).to(dev)
    if args.mem_budget_gb is not None:
        lig_jet.set_memory_budget(int(args.mem_budget_gb * 2 ** 30))
    igres = tuple(args.igres)
    lig_jet.set_mlp_precision(args.mlp_precision)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=igres, nf=16, mf=256).to(dev)
    unet.train()
    params = [p for p in net.parameters()]
    uparams = [p for p in unet.parameters()]
    if world > 1:
        for p in params + uparams:
            dist.broadcast(p.data, 0)
    crop, pts_all, tgt_all = make_inputs(args.points, dev, igres=igres, n_out=n_out)
    n_local = args.points // world
    pts = pts_all[:, rank * n_local:(rank + 1) * n_local].contiguous()
    tgt = tgt_all[:, rank * n_local:(rank + 1) * n_local].contiguous()
    del pts_all, tgt_all
    if c5:
        from space_time_pde_amd import pde as pde_module
        layer = c5_layer(pde_module)
    else:
        layer = physics.get_rb2_pde_layer(**RB2)
    lig_jet.DEFAULT_CHUNK = args.chunk
    from space_time_pde_amd.train_step import sharded_step
    uev = []
    pending = []

    def _post(m, i, o):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        uev.append((pending.pop(), e1))

    def step():
        for p in params + uparams:
            p.grad = None
        return sharded_step(unet, net, layer, crop, pts, tgt, args.points, ALPHA_REG, ALPHA_PDE, "l1")

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    sync()
    # timed region: exactly `steps` steps between two barrier + synchronize brackets; nothing but one pair of HIP events
    # per step (on torch's current stream = the stream every kernel of the step is launched on) is recorded inside it
    sev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    import gc
    gc.collect()
    gc.disable()          # no cyclic-garbage pause of the host interpreter inside the timed region (re-enabled right after it)
    t0 = time.perf_counter()
    for k in range(args.steps):
        sev[k][0].record()
        last = step()
        sev[k][1].record()
    sync()
    dt = time.perf_counter() - t0
    gc.enable()
    loss = last[0]
    from space_time_pde_amd import train_step as _ts
    coll_rec = list(_ts.last_collectives)        # (what, bytes) of the collectives of the last timed step
    step_ms_seq = [a.elapsed_time(b) for a, b in sev]
    step_ms = sorted(step_ms_seq)
    step_ms_median = step_ms[len(step_ms) // 2]
    peak_gb = torch.cuda.max_memory_allocated(dev) / 2 ** 30      # warm-up + timed steps (allocated, not reserved)
    recompute_steps = lig_jet.stats["recompute_steps"]
    # ms_per_step and peak_GB of a multi-GPU line: the slowest rank
    tt = torch.tensor([dt, peak_gb], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt, peak_gb_all = tt.tolist()
    assert lig.stats["hip_jet_calls"] >= args.steps + args.warmup, "HIP jet path was not taken"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step_outputs(last, [("unet", unet), ("imnet", net)]))
    coll = [dict(what=w, bytes=int(b)) for w, b in coll_rec]

    # --full: the diagnostics below, each measured after the timed region
    per_rank = side = x3 = roofline = None
    if args.full:
        # Per-rank diagnosis of a multi-GPU line (outside the timed region, VERDICT r3 #3c): what THIS rank's step costs with no
        # collective in it (same shard, same kernels) and what
        # its replicated U-Net costs alone; rank 0 prints the per-rank lists and ms_per_step - max(compute_ms) as the exposed
        # communication (+ load imbalance) of the timed steps.
        def local_step():
            for p in params + uparams:
                p.grad = None
            sharded_step(unet, net, layer, crop, pts, tgt, args.points, ALPHA_REG, ALPHA_PDE, "l1", distributed=False)

        local_step()
        ce = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ce[0].record()
        for _ in range(2):
            local_step()
        ce[1].record()
        torch.cuda.synchronize()
        compute_ms = ce[0].elapsed_time(ce[1]) / 2
        gcot = torch.randn(1, *igres, 32, device=dev).permute(0, 4, 1, 2, 3)
        ue = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        uf, ub = [], []
        for it in range(3):
            for p in uparams:
                p.grad = None
            ue[0].record()
            y = unet(crop)
            ue[1].record()
            y.backward(gcot)
            ue[2].record()
            torch.cuda.synchronize()
            if it:
                uf.append(ue[0].elapsed_time(ue[1]))
                ub.append(ue[1].elapsed_time(ue[2]))
        del y, gcot
        per_rank = torch.tensor([compute_ms, sum(uf) / len(uf), sum(ub) / len(ub), peak_gb], device=dev, dtype=torch.float64)
        if world > 1:
            allr = [torch.zeros_like(per_rank) for _ in range(world)]
            dist.all_gather(allr, per_rank)
            per_rank = torch.stack(allr)
        else:
            per_rank = per_rank[None]
        per_rank = per_rank.cpu().tolist()
        # the collectives of one step (what, bytes) as the step itself recorded them, and what each costs ALONE on this process
        # group (median of 5 all-reduces of the same size, outside the timed region): with per_rank.compute_ms this separates
        # bandwidth / latency of the exchange from load imbalance in a multi-GPU line
        if dist.is_initialized():
            for c in coll:
                buf = torch.zeros(max(1, c["bytes"] // 4), device=dev)
                dist.all_reduce(buf)
                torch.cuda.synchronize()
                ts = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    dist.all_reduce(buf)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                c["alone_ms"] = round(sorted(ts)[2], 3)
                del buf
        # per-kernel HIP-event timings: a SECOND pass outside the timed region (the event pairs around ~70 launches per
        # step would otherwise sit inside it)
        lig_jet.profile = {}
        # (2 until round 5, 4 in round 5: one 120 ms outlier among four launches decided which kernel was "dominant", VERDICT r5
        # weak #3; since round 6 eight steps, and dominance is decided on the MEDIAN launch time)
        nprof = 8
        unet.register_forward_pre_hook(lambda m, i: pending.append(torch.cuda.Event(enable_timing=True)) or pending[-1].record())
        unet.register_forward_hook(_post)
        for _ in range(nprof):
            step()
        sync()
        prof = lig_jet.profile
        lig_jet.profile = None

        # SURVEY 8(d) side figures (outside the timed region, rank 0 of a single-GPU run only): value-only inference rate,
        # the step without the UNet, and the gather stage against its algorithmic 1036 B / point
        side = None
        if rank == 0 and world == 1 and not args.sub:
            import torch.nn.functional as F
            with torch.no_grad():
                latent = unet(crop).permute(0, 2, 3, 4, 1)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            with torch.no_grad():
                lig.query_local_implicit_grid(net, latent, pts, 0., 1.)
                ev[0].record()
                for _ in range(3):
                    lig.query_local_implicit_grid(net, latent, pts, 0., 1.)
                ev[1].record()

            def lig_only_step():
                for p in params:
                    p.grad = None
                lat = latent.detach().requires_grad_(True)
                layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, lat, q, 0., 1.))
                pred, res = layer(pts, return_residue=True)
                st = torch.stack(list(res.values()), 0)
                (ALPHA_REG * F.l1_loss(pred, tgt) + ALPHA_PDE * st.abs().mean()).backward()

            lig_only_step()
            ev[2].record()
            for _ in range(2):
                lig_only_step()
            ev[3].record()
            torch.cuda.synchronize()
            side = dict(inference_value_only_points_per_s=round(3 * args.points / (ev[0].elapsed_time(ev[1]) * 1e-3)),
                        lig_only_step_points_per_s=round(2 * args.points / (ev[2].elapsed_time(ev[3]) * 1e-3)))
        # Second headline-grade line: the SAME step with the wide layers' products as exact-split bf16 MFMAs
        # ("fp32x3": every fp32-tolerance parity test is parametrised over it, tests/test_gpu_reference_fixtures.py), timed over the
        # same --steps with the same bracket as `value`, then two profiled steps for its own dominant-kernel roofline.  `value` /
        # `dtype` above stay the exact-fp32 MFMA path.
        x3 = None
        if rank == 0 and world == 1 and args.mlp_precision == "fp32" and not c5 and not args.sub and not args.no_other_configs:
            if side is not None:
                del latent
            lig_jet.set_mlp_precision("fp32x3")
            try:
                for _ in range(max(1, min(args.warmup, 2))):
                    step()
                sync()
                gc.collect()
                gc.disable()
                t3 = time.perf_counter()
                for _ in range(args.steps):
                    l3 = step()[0]
                sync()
                dt3 = time.perf_counter() - t3
                gc.enable()
                lig_jet.profile = {}
                for _ in range(nprof):
                    step()
                sync()
                x3 = dict(dt=dt3, loss=float(l3), prof=lig_jet.profile)
                lig_jet.profile = None
            finally:
                lig_jet.set_mlp_precision("fp32")
                lig_jet.profile = None

    bf16 = args.mlp_precision == "bf16"
    if rank == 0 and args.full:
        smooth = args.act not in ("relu", "leakyrelu")
        # piecewise-linear activations have identically zero second-order MLP jets.  c5: the equation set needs
        # 4 second-order jets (xx, yy, xy, tt); SURVEY: "replace 32*4 by 32*5 in M and T"
        n2_alg = (4 if c5 else 2) if smooth else 0
        s34 = os.environ.get("STPDE_S34", "1") != "0"    # c5: the four named pairs on the (3,4) stream set (round 5), or padded to (3,6)
        n2_exe = ((4 if s34 else 6) if c5 else 1) if smooth else 0
        macs, M, T = algorithmic_macs(n_second=n2_alg, cout=n_out)
        fwd_flop_pt = 2 * 8 * (M + (3 + n2_alg) * T)
        step_flop_pt = 3 * fwd_flop_pt
        kern = {}
        prof["unet_fwd"] = uev[-nprof:]
        for name, evs in prof.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            kern[name] = dict(launches=len(ms), total_ms=sum(ms), avg_ms=sum(ms) / len(ms), min_ms=min(ms), max_ms=max(ms),
                              median_ms=sorted(ms)[len(ms) // 2])
        # dominant kernel = largest (median launch time x launches): what a rocprofv3 --stats summary of this command puts in
        # its top row, robust against a single slow launch (>= 8 samples per kernel)
        dom = max(kern, key=lambda k: kern[k]["median_ms"] * kern[k]["launches"])
        # A kernel may take several launches per step (launch chunks): achieved = its FLOPs per STEP / its time per step, which is also
        # FLOPs per launch / average launch duration with both averaged over the same launches -- the figure a rocprofv3
        # --stats summary of this command gives
        lps = kern[dom]["launches"] / float(nprof)
        rows_per_launch = 8 * n_local / lps
        flop_launch = 2.0 * macs.get(dom, 0) * rows_per_launch
        ach = flop_launch / (kern[dom]["avg_ms"] * 1e-3) / 1e12
        # what the kernels actually execute: the RB2 equations use d_xx and d_zz only through one common combination,
        # so the network carries ONE second-order stream (none at all for piecewise-linear activations)
        macs_x, _, _ = algorithmic_macs(n_second=n2_exe, cout=n_out)
        exe = 2.0 * macs_x.get(dom, 0) * rows_per_launch / (kern[dom]["avg_ms"] * 1e-3) / 1e12
        traffic, traffic_src = None, None
        try:    # HBM bytes per launch from the committed rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE passes (same chunk size)
            tj = json.load(open(args.traffic_json))
            if tj.get("act") == args.act and dom in tj["kernels"]:
                # the counter passes were taken on a 2^18-point launch; these kernels stream every row tile exactly once,
                # so the bytes of a launch scale with its number of tiles
                scale = rows_per_launch / 8.0 / float(tj["chunk"])
                traffic = tj["kernels"][dom]["hbm_bytes_per_launch"] * scale
                traffic_src = tj.get("source") + ("" if scale == 1 else "; measured on a %d-point launch, scaled x%g to "
                                                      "this launch's tile count" % (tj["chunk"], scale))
        except (OSError, ValueError, KeyError):
            pass
        # `frac` / `achieved` = the MFMA work the kernel EXECUTES over the peak (a utilisation, < 1 by
        # construction); the SURVEY 8(d) algorithmic count (6 streams where 5 run: a work-reduction credit, may approach or
        # exceed 1) is kept beside it as algorithmic_*
        roofline = dict(bound="mfma", kernel=dom, achieved=round(exe, 2), peak=PEAK_F32_TFLOPS, unit="TFLOP/s",
                        frac=round(exe / PEAK_F32_TFLOPS, 4), traffic=traffic, traffic_source=traffic_src,
                        note="achieved / frac = MFMA FLOPs the dominant kernel executes per launch (value + 3 first-order + the ONE "
                             "combined second-order stream RB2 needs) / its average launch time, over the fp32 MFMA peak; "
                             "algorithmic_* = the same with SURVEY 8(d)'s algorithmic count (value + 3 first + 2 second-order "
                             "streams), i.e. including the credit for the stream the combined form does not have to run",
                        executed_tflops=round(exe, 2), executed_frac=round(exe / PEAK_F32_TFLOPS, 4),
                        algorithmic_tflops=round(ach, 2), algorithmic_frac=round(ach / PEAK_F32_TFLOPS, 4),
                        flop_per_launch=2.0 * macs_x.get(dom, 0) * rows_per_launch, algorithmic_flop_per_launch=flop_launch,
                        avg_launch_ms=round(kern[dom]["avg_ms"], 3), median_launch_ms=round(kern[dom]["median_ms"], 3),
                        launch_ms_min_max=[round(kern[dom]["min_ms"], 3), round(kern[dom]["max_ms"], 3)], launches_per_step=lps,
                        launch_samples=kern[dom]["launches"],
                        step_algorithmic_tflops=round(step_flop_pt * args.points / (dt / args.steps) / 1e12 / world, 2),
                        step_frac_per_gpu=round(step_flop_pt * args.points / (dt / args.steps) / 1e12 / world
                                                / PEAK_F32_TFLOPS, 4),
                        step_executed_frac_per_gpu=round(3 * 2 * 8 * (M + (3 + n2_exe) * T) * args.points / (dt / args.steps)
                                                         / 1e12 / world / PEAK_F32_TFLOPS, 4),
                        kernels_note="ms per step of each kernel family, HIP events on the launch stream, from %d extra "
                                     "steps run after the timed region" % nprof,
                        kernels={k: round(v["total_ms"] / nprof, 2) for k, v in sorted(kern.items())})
        roofline["stream_set"] = [3 if (smooth or True) else 0, n2_exe]      # (S1, S2) the MLP kernels carry
        if "gather" in kern:   # the gather stage in isolation is HBM-bound: algorithmic 1036 B per point
            g_ms = kern["gather"]["avg_ms"]
            g_pts = n_local * nprof / float(kern["gather"]["launches"])        # points per launch, averaged like g_ms
            gs = dict(bound="hbm", achieved=round(1036.0 * g_pts / (g_ms * 1e-3) / 1e9, 1),
                      peak=8000.0, unit="GB/s", avg_launch_ms=round(g_ms, 3),
                      note="achieved = algorithmic 12 B coords + 8 x 32 x 4 B corner latents per point / launch time; the kernel "
                           "also writes the column-major fragment image X of the MLP input (1.5 KiB per point; no row-major copy XR since round 5); "
                           "measured_* = HBM bytes of the launch from the committed rocprofv3 FETCH_SIZE (x2) / WRITE_SIZE passes")
            try:
                tj = json.load(open(args.traffic_json))
                if "gather" in tj["kernels"]:
                    mb = tj["kernels"]["gather"]["hbm_bytes_per_launch"] * g_pts / float(tj["chunk"])
                    gs.update(measured_bytes_per_launch=mb, measured_GBps=round(mb / (g_ms * 1e-3) / 1e9, 1),
                              measured_frac=round(mb / (g_ms * 1e-3) / 1e9 / 8000.0, 4))
            except (OSError, ValueError, KeyError):
                pass
            roofline["gather_stage"] = gs
        if side:
            roofline["side_figures"] = side
        if bf16:
            # bf16 operands: the layer kernels are priced against BOTH roofs -- HBM on the bytes of the packed layer buffers
            # (what the kernel has to move) and the dense bf16 MFMA peak on the executed products -- and the line carries the
            # one the dominant kernel sits closer to; the other is kept as a secondary figure
            from space_time_pde_amd import lig_jet as _lj
            pk = bool(getattr(_lj, "packed_stash", False))
            by = algorithmic_bytes(1 + 3 + (1 if smooth else 0), packed=pk).get(dom)
            if by:
                gbs = by * rows_per_launch / (kern[dom]["avg_ms"] * 1e-3) / 1e9
                hbm = dict(achieved=round(gbs, 1), peak=8000.0, unit="GB/s", frac=round(gbs / 8000.0, 4),
                           bytes_per_launch=by * rows_per_launch,
                           bytes_note="algorithmic bytes of the dominant kernel in the %s layer-buffer format"
                                      % ("packed (value fp32 / derivative streams bf16; adjoints bf16)" if pk else "fp32"))
                if traffic:
                    hbm["measured_GBps"] = round(traffic / (kern[dom]["avg_ms"] * 1e-3) / 1e9, 1)
                    hbm["measured_frac"] = round(traffic / (kern[dom]["avg_ms"] * 1e-3) / 1e9 / 8000.0, 4)
                mfma = dict(achieved=round(exe, 2), peak=2500.0, unit="TFLOP/s", frac=round(exe / 2500.0, 4))
                if mfma["frac"] >= hbm["frac"]:
                    roofline.update(bound="mfma", hbm_side=hbm, **mfma)
                else:
                    roofline.update(bound="hbm", mfma_side=mfma, **{k: hbm[k] for k in ("achieved", "peak", "unit", "frac")})
                    roofline["hbm_side"] = hbm
                roofline.update(note="bf16-MFMA mode: the dominant kernel against the dense bf16 MFMA peak (executed products: "
                                     "combined second-order stream) and against HBM (algorithmic bytes of its packed layer "
                                     "buffers / launch time; measured_* = rocprofv3 FETCH_SIZE x2 + WRITE_SIZE of the same "
                                     "configuration when committed); `bound` names the roof it is closer to -- it reaches "
                                     "neither: the first-layer kernels of this mode are bound by VALU work (activation jets) "
                                     "and latency, DESIGN 5a",
                                executed_frac=round(exe / 2500.0, 4))
                roofline.pop("step_frac_per_gpu", None)
        if args.mlp_precision == "fp32x3":
            # exact-split mode: the wide layers issue SIX bf16 MFMA products per fp32 product, so the pipe that bounds them is
            # the bf16 one; price the executed bf16 work against its dense peak (the fp32-MFMA fractions would exceed 1)
            x6 = 6.0 * exe
            roofline.update(achieved=round(x6, 2), peak=2500.0, frac=round(x6 / 2500.0, 4), traffic=None, traffic_source=None,
                            note="fp32x3 mode: achieved = executed bf16 MFMA work of the dominant kernel (6 partial products "
                                 "per fp32 product of the combined-stream jet) / launch time, against the dense bf16 peak; "
                                 "fp32_equivalent_tflops = the fp32 products it stands for",
                            fp32_equivalent_tflops=round(exe, 2))
            roofline.pop("executed_tflops", None)
            roofline.pop("executed_frac", None)
            roofline["step_frac_note"] = "step_frac_per_gpu is the algorithmic fp32 FLOP rate of the step over the fp32-MFMA peak (157.3): a speed-up figure in this mode, not a utilisation"
    if rank == 0:
        out = {
            "metric": ("query-points/sec (fwd+PDE-residual bwd), user-string 5-channel equations, 128^3 latent" if c5 else
                       "query-points/sec (fwd+PDE-residual bwd), rb2d 128^3 latent"),
            "value": args.points * args.steps / dt,
            "unit": "query-points/s",
            "n_gpus": world,
            "rccl_world": dist.get_world_size() if dist.is_initialized() else 1,
            "dist_backend": (dist.get_backend() if dist.is_initialized() else None),
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps,
            "ms_per_step_hip_event_median": round(step_ms_median, 3),
            "ms_per_step_hip_event_min_max": [round(step_ms[0], 3), round(step_ms[-1], 3)],
            "ms_per_step_hip_event_sequence": [round(v, 2) for v in step_ms_seq],
            "peak_GB": round(peak_gb_all, 2),
            "recompute_steps": recompute_steps,
            "collectives_per_step": coll,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": ("bf16 MFMA operands (wide IM-NET layers) / f32 accumulate, stash, epilogues, UNet" if bf16 else
                      "f32 via 3xbf16 split, f32 accumulate (hidden-to-hidden GEMMs of the two wide IM-NET layers -- forward, input "
                      "gradient, weight gradient: every fp32 operand split exactly into three bf16 terms, six partial products on "
                      "the bf16 MFMA pipe; everything else exact f32)"
                      if args.mlp_precision == "fp32x3" else "f32"),
            "data": "synthetic",
            "deterministic": det,
            "config": {"workload": ("BASELINE configs[4]: latent [1,%d,%d,%d,32], 2^%d query points, 5-output user-string "
                                    "equations %s (3 inputs x, y, t; second derivatives xx, yy, xy, tt -> the (3,%d) stream set), "
                                    "ImNet nf=32 out_features=5 %s, L1 losses, backward to ImNet + UNet3d parameters"
                                    % (igres + (args.points.bit_length() - 1, json.dumps(C5_EQS), 4 if os.environ.get("STPDE_S34", "1") != "0" else 6,
                                       args.act))) if c5 else
                                   "BASELINE configs[%d]: latent [1,%d,%d,%d,32], 2^%d query points, RB2 "
                                   "(3 transport + continuity), ImNet nf=32 %s, L1 losses, backward to ImNet + UNet3d parameters"
                                   % ((3 if (bf16 and igres == (64, 256, 256)) else 1,) + igres + (args.points.bit_length() - 1, args.act)),
                       "points": args.points, "parallelism": "points sharded x%d" % world,
                       "unet": "UNet3d(igres=%s, nf=16, mf=256) fwd+bwd inside the timed step" % (igres,),
                       "loss": float(loss)},
        }
        if args.full:
            out["per_rank"] = {
                "compute_ms": [round(r[0], 2) for r in per_rank],
                "unet_fwd_ms": [round(r[1], 2) for r in per_rank], "unet_bwd_ms": [round(r[2], 2) for r in per_rank],
                "peak_GB": [round(r[3], 2) for r in per_rank],
                "exposed_comm_ms": round(1e3 * dt / args.steps - max(r[0] for r in per_rank), 2),
                "note": "compute_ms = this rank's step on its shard with no collective in it (2 steps after the timed "
                        "region); unet_*_ms = its replicated U-Net alone, eager launches with their gaps (inside the "
                        "step the backward runs after the IM-NET backward on the same stream); exposed_comm_ms = "
                        "ms_per_step - max(compute_ms): exchange + load imbalance not hidden behind compute"}
            out["roofline"] = roofline
        if x3 is not None:
            # fp32x3: the wide layers issue SIX bf16 MFMA products per fp32 product, so the pipe that bounds its kernels is the
            # bf16 one: its dominant kernel's executed bf16 work (combined-stream jet) against the dense bf16 peak
            k3 = {}
            for name, evs in x3["prof"].items():
                ms = [a.elapsed_time(b) for a, b in evs]
                k3[name] = dict(launches=len(ms), total_ms=sum(ms), avg_ms=sum(ms) / len(ms), median_ms=sorted(ms)[len(ms) // 2])
            dom3 = max(k3, key=lambda k: k3[k]["median_ms"] * k3[k]["launches"])
            lps3 = k3[dom3]["launches"] / float(nprof)
            rows3 = 8 * n_local / lps3
            exe3 = 2.0 * macs_x.get(dom3, 0) * rows3 / (k3[dom3]["avg_ms"] * 1e-3) / 1e12
            alg3 = 2.0 * macs.get(dom3, 0) * rows3 / (k3[dom3]["avg_ms"] * 1e-3) / 1e12
            ms3 = 1e3 * x3["dt"] / args.steps
            out["value_fp32x3"] = args.points * args.steps / x3["dt"]
            out["ms_per_step_fp32x3"] = ms3
            out["dtype_fp32x3"] = ("f32 via 3xbf16 split, f32 accumulate: every fp32 operand of the hidden-to-hidden GEMMs of the two "
                                   "wide IM-NET layers (forward, input gradient, first-layer weight gradient) split exactly into "
                                   "three bf16 terms, six partial products on the bf16 MFMA pipe; everything else exact f32; same "
                                   "fp32 parity tolerances as `value` (tests parametrised over both modes)")
            out["loss_fp32x3"] = x3["loss"]
            out["roofline_fp32x3"] = dict(
                bound="mfma", kernel=dom3, achieved=round(6.0 * exe3, 2), peak=2500.0, unit="TFLOP/s",
                frac=round(6.0 * exe3 / 2500.0, 4), avg_launch_ms=round(k3[dom3]["avg_ms"], 3), launches_per_step=lps3,
                fp32_equivalent_tflops=round(exe3, 2), algorithmic_fp32_tflops=round(alg3, 2),
                algorithmic_over_fp32_mfma_peak=round(alg3 / PEAK_F32_TFLOPS, 4),
                step_algorithmic_tflops=round(step_flop_pt * args.points / (ms3 * 1e-3) / 1e12, 2),
                step_over_fp32_mfma_peak=round(step_flop_pt * args.points / (ms3 * 1e-3) / 1e12 / PEAK_F32_TFLOPS, 4),
                note="achieved = executed bf16 MFMA work of the dominant kernel (6 partial products per fp32 product of the "
                     "combined-stream jet) / launch time, against the dense bf16 peak; *_over_fp32_mfma_peak = the fp32 FLOP "
                     "rate it stands for over the exact-fp32 MFMA peak (157.3): a speed-up figure, may exceed 1; timed over "
                     "the same --steps as `value`, HIP-event kernel times from %d extra steps" % nprof,
                kernels={k: round(v["total_ms"] / nprof, 2) for k, v in sorted(k3.items())})
        if args.full and world == 1 and not args.sub and not args.no_other_configs and not c5 and args.mlp_precision == "fp32":
            out["other_configs"] = other_configs(args)
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(args.act)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
