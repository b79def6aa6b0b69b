#!/usr/bin/env python
"""Whole training iteration of the reference's own regime (bench.py's ``train_default``: experiments/rb2d/run_experiment.sh:16,
10 crops x 512 points on the (4,16,16) latent grid, lr=1e-2, clip_grad=1, ``loss.item()`` per iteration), timed two ways:

  (a) forward + backward replayed from a HIP graph, then an eager ``FusedClipAdam(flat=False).step()`` on the graph's static
      gradients -- what bench.py times;
  (b) ONE graph with the optimizer inside: ``GraphedStep(optimizer=FusedClipAdam(capturable=True))``.

Both arrangements are built once in this process (each on its own copy of the same model) and then timed alternately,
(a) (b) (a) (b) (a) (b), so that drift of the box hits both alike.  Every sample and the medians go to ``--out`` (JSON); the
last line printed is that JSON.  Condition looked at: median(b) <= median(a) + (max(a) - min(a)).

Run it under a time limit of its own:

    timeout -k 10 600 python tools/bench_graphed_iteration.py --out profiles/graphed_iteration.json
"""
import argparse
import copy
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

RB2 = dict(mean=(0.01, 0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1., x_crop=1., use_continuity=True)
ALPHA_REG, ALPHA_PDE = 1.0, 0.0125
B, N, IGRES = 10, 512, (4, 16, 16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="iterations per sample")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--flat", type=int, default=0, help="(b): 1 = flat buffers inside the graph, 0 = pointer table (as (a))")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_graphed_iteration needs a HIP GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from space_time_pde_amd import implicit_net, local_implicit_grid as lig, optim, physics, unet3d
    from space_time_pde_amd.train_step import GraphedStep
    torch.manual_seed(1)
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=IGRES, nf=16, mf=256).to(dev).train()
    g = torch.Generator().manual_seed(0)
    crop = torch.randn(B, 4, *IGRES, generator=g).to(dev)
    pts = torch.rand(B, N, 3, generator=g).to(dev)
    tgt = torch.randn(B, N, 4, generator=g).to(dev)
    n0 = lig.stats["hip_jet_calls"]

    # (a) the parent's arrangement
    unet_a, net_a = copy.deepcopy(unet), copy.deepcopy(net)
    params_a = list(unet_a.parameters()) + list(net_a.parameters())
    gstep_a = GraphedStep(unet_a, net_a, physics.get_rb2_pde_layer(**RB2), crop, pts, tgt, N, ALPHA_REG, ALPHA_PDE, "l1")
    grads_a = [p.grad for p in params_a]
    opt_a = optim.FusedClipAdam(params_a, lr=1e-2, clip_grad=1.0, flat=False)

    def step_a():
        loss, _, _ = gstep_a()
        for p, gr in zip(params_a, grads_a):             # exactly bench.py's graph_step(): the eager optimizer reads p.grad,
            p.grad = gr                                  # and a training loop's zero_grad() takes it away every iteration
        opt_a.step()
        return loss

    # (b) one graph for the whole iteration
    unet_b, net_b = copy.deepcopy(unet), copy.deepcopy(net)
    params_b = list(unet_b.parameters()) + list(net_b.parameters())
    opt_b = optim.FusedClipAdam(params_b, lr=1e-2, clip_grad=1.0, flat=bool(args.flat), capturable=True)
    gstep_b = GraphedStep(unet_b, net_b, physics.get_rb2_pde_layer(**RB2), crop, pts, tgt, N, ALPHA_REG, ALPHA_PDE, "l1",
                          optimizer=opt_b)
    assert lig.stats["hip_jet_calls"] > n0, "HIP jet path was not taken"

    def step_b():
        return gstep_b()[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            v = fn().item()                              # train.py:84 ``tot_loss += loss.item()``
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps, v

    for fn in (step_a, step_b):
        for _ in range(args.warmup):
            fn().item()
    gc.collect()
    gc.disable()
    sa, sb, la, lb = [], [], None, None
    for _ in range(args.samples):
        ms, la = timed(step_a)
        sa.append(round(ms, 4))
        ms, lb = timed(step_b)
        sb.append(round(ms, 4))
    gc.enable()
    med_a, med_b, spread_a = statistics.median(sa), statistics.median(sb), max(sa) - min(sa)
    out = {
        "workload": "train_default: 10 crops x 512 points, latent [10,4,16,16,32], UNet3d(igres=(4,16,16), nf=16, mf=256), "
                    "lr=1e-2, clip_grad=1, loss.item() per iteration",
        "device": torch.cuda.get_device_name(0),
        "steps_per_sample": args.steps, "warmup": args.warmup,
        "a": "HIP graph (forward + backward) + eager FusedClipAdam(flat=False).step()",
        "b": "one HIP graph: forward + backward + FusedClipAdam(capturable=True, flat=%s)" % bool(args.flat),
        "ms_per_iteration_a": sa, "ms_per_iteration_b": sb,
        "median_ms_a": round(med_a, 4), "median_ms_b": round(med_b, 4), "spread_ms_a": round(spread_a, 4),
        "b_within_spread_of_a": bool(med_b <= med_a + spread_a),
        "steps_taken_b": opt_b.device_step(), "last_loss_a": la, "last_loss_b": lb,
    }
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
