#!/usr/bin/env python
"""``step()`` of the fused optimizers over the parameter set of tools/bench_next_rows.py's N1 row
(``UNet3d(igres=(32,128,128), nf=16, mf=256)`` + ``ImNet(nf=32)``), eight combinations: Adam / SGD with momentum, flat buffers /
pointer table, host scalars / ``capturable=True``.

A sample is a host clock around enough steps to last ``--seconds`` (the count is fixed per combination after the warm-up),
ending in a synchronise; every sample is printed as one JSON line as it is taken, and the last line printed is the JSON of
all samples and the medians (also written to ``--out``).  With ``--paced`` each sample waits for a line on stdin first, so
that a driver can interleave the samples of two builds of the package on one GPU.

Run it under a time limit of its own:

    timeout -k 10 300 python tools/bench_optim_step.py --out profiles/optim_step.json
"""
import argparse
import gc
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

COMBOS = [(kind, flat, cap) for kind in ("adam", "sgd_momentum") for flat in (True, False) for cap in (False, True)]


def name_of(kind, flat, cap):
    return "%s/%s/%s" % (kind, "flat" if flat else "table", "capturable" if cap else "host_scalars")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=1.1, help="least duration of a sample")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--paced", action="store_true", help="take each sample when a line arrives on stdin")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_step needs a HIP GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from space_time_pde_amd import implicit_net, nonlinearities, optim, unet3d
    torch.manual_seed(0)
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32,
                             activation=nonlinearities.NONLINEARITIES["softplus"]).to(dev)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=(32, 128, 128), nf=16, mf=256).to(dev)
    model = list(unet.parameters()) + list(net.parameters())
    grads = [torch.randn_like(p) for p in model]
    out = {"workload": "step() over UNet3d(igres=(32,128,128), nf=16, mf=256) + ImNet(nf=32): %d tensors, %d elements, "
                       "lr=1e-3, clip_grad=1" % (len(model), sum(p.numel() for p in model)),
           "device": torch.cuda.get_device_name(0), "seconds_per_sample": args.seconds, "warmup": args.warmup, "combos": {}}

    def timed(opt, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for kind, flat, cap in COMBOS:
        params = [p.detach().clone().requires_grad_(True) for p in model]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        if kind == "adam":
            opt = optim.FusedClipAdam(params, lr=1e-3, clip_grad=1.0, flat=flat, capturable=cap)
        else:
            opt = optim.FusedClipSGD(params, lr=1e-3, momentum=0.9, clip_grad=1.0, flat=flat, capturable=cap)
        timed(opt, args.warmup)
        steps = max(1, math.ceil(args.seconds * args.warmup / timed(opt, args.warmup)))
        gc.collect()
        gc.disable()
        ms = []
        for _ in range(args.samples):
            if args.paced and not sys.stdin.readline():
                raise SystemExit("bench_optim_step --paced: stdin closed")
            ms.append(round(1e3 * timed(opt, steps) / steps, 5))
            print(json.dumps({"combo": name_of(kind, flat, cap), "ms_per_step": ms[-1]}), flush=True)
        gc.enable()
        out["combos"][name_of(kind, flat, cap)] = {"steps_per_sample": steps, "ms_per_step": ms,
                                                   "median_ms": statistics.median(ms), "spread_ms": round(max(ms) - min(ms), 5)}
        del opt, params
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
