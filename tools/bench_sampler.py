#!/usr/bin/env python
"""Producing a training batch on the device, timed two ways on the reference crop (16 x 128 x 128 -> 4 x 32 x 32 low-res, 1024
query points per crop; synthetic RB2 run [4, 200, 512, 128], normalised outputs):

  per batch, B = 10 and B = 64:
    get   ``RB2DeviceLoader.get(idx)``: host list of crop ids, per-crop slicing, torch.rand, index_select pairs, the interpolation
          kernel, two normalisations (what profiles/r6_next_rows.json's N3 row times);
    draw  ``DeviceBatchSampler.draw()``: three launches, ids and points from the device generator (csrc/sampler.hip);

  per iteration of ``train_default`` (experiments/rb2d/run_experiment.sh:16: 10 crops x 512 points on the (4,16,16) latent grid,
  here crops of 8 x 32 x 32 down-sampled by 2, lr = 1e-2, clip_grad = 1, ``loss.item()`` per iteration):
    (a) ``loader.get()`` in Python, then ``GraphedStep(optimizer=...)`` replayed on the copied-in batch;
    (b) ``GraphedStep(optimizer=..., sampler=...)``: the draw is the head of the graph, one replay is the whole iteration.

``--lres-filter gaussian | uniform | maximum`` turns the reference's low-res pre-filter on in both loaders: ``get()`` then filters
with composed torch ops per batch (``dataloader_spacetime.lres_filter``), ``draw()`` with the filter passes of csrc/sampler.hip
(``DeviceBatchSampler(filter_on_device=True)``); results of such a run belong in ``profiles/sampler_filter.json``.
``--lres-filter median`` does the same with the selection kernel of csrc/sampler_median.hip (``median_on_device=True``); results
belong in ``profiles/sampler_median.json``.  ``get()`` unfolds every voxel's 7 x 7 x 7 window for it -- 14.4 GB per batch of 10, on
which ``torch.median`` then sorts -- so the per-batch pair is timed at B = 10 only (B = 64 would materialise ~92 GB) and wants few
batches per sample (``--batches 3 --batch-warmup 1``); ``get()`` is unchanged from before the kernel existed, so pair member ``get`` IS
the only median path there was.

Both members of a pair are timed alternately, so that drift of the box hits both alike.  Every sample and the medians go to
``--out`` (JSON); the last line printed is that JSON.  No target is attached to these numbers.

Run it under a time limit of its own:

    timeout -k 10 600 python tools/bench_sampler.py --out profiles/sampler_pipeline.json
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
    ap.add_argument("--batches", type=int, default=200, help="batches per sample of the per-batch pair")
    ap.add_argument("--steps", type=int, default=200, help="iterations per sample of the per-iteration pair")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch-warmup", type=int, default=None, help="warm-up calls of the per-batch pair (default: --warmup)")
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--skip-iteration", action="store_true", help="only the per-batch pair")
    ap.add_argument("--lres-filter", default="none", choices=["none", "gaussian", "uniform", "maximum", "median"],
                    help="low-res pre-filter of both loaders (draw() then filters on the device)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler needs a HIP GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from space_time_pde_amd import implicit_net, local_implicit_grid as lig, optim, physics, unet3d
    from space_time_pde_amd.dataloader_spacetime import DeviceBatchSampler, RB2DeviceLoader
    from space_time_pde_amd.train_step import GraphedStep

    def alternate(fa, fb, n, sync_each, warmup=None):
        """samples of (ms per call of fa, of fb), timed alternately"""
        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                r = fn()
                if sync_each:
                    r.item()                             # train.py:84 ``tot_loss += loss.item()``
            torch.cuda.synchronize()
            return round(1e3 * (time.perf_counter() - t0) / n, 4)
        for fn in (fa, fb):
            for _ in range(args.warmup if warmup is None else warmup):
                r = fn()
            torch.cuda.synchronize()
        gc.collect()
        gc.disable()
        sa, sb = [], []
        for _ in range(args.samples):
            sa.append(timed(fa))
            sb.append(timed(fb))
        gc.enable()
        return sa, sb

    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "dataset": "synthetic RB2 run [4, 200, 512, 128] fp32, normalize_output=True, lres_filter %s, linear" % args.lres_filter,
           "lres_filter": args.lres_filter,
           "per_batch": {}}
    data = torch.randn(4, 200, 512, 128, generator=torch.Generator().manual_seed(0))
    ld = RB2DeviceLoader(data, nx=128, nz=128, nt=16, n_samp_pts_per_crop=1024, downsamp_xz=4, downsamp_t=4,
                         normalize_output=True, device=dev, lres_filter=args.lres_filter)
    on_device = args.lres_filter != "none"
    median = args.lres_filter == "median"
    for nb in ((10,) if median else (10, 64)):
        s = DeviceBatchSampler(ld, nb, seed=0, filter_on_device=on_device, median_on_device=median)
        gen = torch.Generator().manual_seed(nb)

        def get():
            idx = torch.randint(0, len(ld), (nb,), generator=gen).tolist()        # the host sampler's ids
            return ld.get(idx)[0]

        sa, sb = alternate(get, lambda: s.draw()[0], args.batches, False, args.batch_warmup)
        out["per_batch"]["B=%d" % nb] = {
            "crop": "16x128x128 -> 4x32x32 low-res + 1024 target points", "batches_per_sample": args.batches,
            "get_ms": sa, "draw_ms": sb, "median_get_ms": statistics.median(sa), "median_draw_ms": statistics.median(sb),
            "draws_taken": s.offset()}
    del ld, data

    if not args.skip_iteration:
        torch.manual_seed(1)
        net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)
        unet = unet3d.UNet3d(in_features=4, out_features=32, igres=IGRES, nf=16, mf=256).to(dev).train()
        data = torch.randn(4, 64, 128, 128, generator=torch.Generator().manual_seed(2))
        ld = RB2DeviceLoader(data, nx=32, nz=32, nt=8, n_samp_pts_per_crop=N, downsamp_xz=2, downsamp_t=2,
                             normalize_output=True, device=dev, lres_filter=args.lres_filter)
        n0 = lig.stats["hip_jet_calls"]
        gen = torch.Generator().manual_seed(3)

        # (a) the batch from get(), outside the graph
        unet_a, net_a = copy.deepcopy(unet), copy.deepcopy(net)
        opt_a = optim.FusedClipAdam(list(unet_a.parameters()) + list(net_a.parameters()), lr=1e-2, clip_grad=1.0, flat=False,
                                    capturable=True)
        first = ld.get(torch.randint(0, len(ld), (B,), generator=gen).tolist())
        gstep_a = GraphedStep(unet_a, net_a, physics.get_rb2_pde_layer(**RB2), *first, N, ALPHA_REG, ALPHA_PDE, "l1",
                              optimizer=opt_a)

        def step_a():
            return gstep_a(*ld.get(torch.randint(0, len(ld), (B,), generator=gen).tolist()))[0]

        # (b) the draw at the head of the graph
        unet_b, net_b = copy.deepcopy(unet), copy.deepcopy(net)
        opt_b = optim.FusedClipAdam(list(unet_b.parameters()) + list(net_b.parameters()), lr=1e-2, clip_grad=1.0, flat=False,
                                    capturable=True)
        s = DeviceBatchSampler(ld, B, seed=0, filter_on_device=on_device, median_on_device=median)
        gstep_b = GraphedStep(unet_b, net_b, physics.get_rb2_pde_layer(**RB2), None, None, None, N, ALPHA_REG, ALPHA_PDE, "l1",
                              optimizer=opt_b, sampler=s)
        assert lig.stats["hip_jet_calls"] > n0, "HIP jet path was not taken"

        sa, sb = alternate(step_a, lambda: gstep_b()[0], args.steps, True)
        out["per_iteration"] = {
            "workload": "train_default: 10 crops (8x32x32 of [4,64,128,128], down-sampled to 4x16x16) x 512 points, "
                        "UNet3d(igres=(4,16,16), nf=16, mf=256), FusedClipAdam(capturable=True, flat=False) inside the graph, "
                        "lr=1e-2, clip_grad=1, loss.item() per iteration",
            "steps_per_sample": args.steps,
            "a": "RB2DeviceLoader.get() in Python + GraphedStep(optimizer=...) replay on the copied-in batch",
            "b": "GraphedStep(optimizer=..., sampler=DeviceBatchSampler): draw + produce captured at the head of the graph",
            "ms_per_iteration_a": sa, "ms_per_iteration_b": sb, "median_ms_a": statistics.median(sa),
            "median_ms_b": statistics.median(sb), "draws_taken_b": s.offset(), "replays_b": gstep_b.replays}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
