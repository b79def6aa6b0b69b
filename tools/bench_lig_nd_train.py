"""Training through local-implicit-grid queries on 2-d and 4-d grids: forward + backward of the HIP path
(``lig_jet.set_nd_backward(True)``: k_gather_nd -> S = 1 IM-NET layer kernels -> k_reduce_nd, and back through k_reduce_nd_bwd,
the S = 1 weight- / input-gradient kernels, k_xbar, k_cell_nd, the cell sort and k_dlat_reduce_nd) against the composed
formulation (HIP coefficient kernel, decoder as ATen ops, corner sum in torch, torch autograd), which is what such a query
runs with the switch off.

    python tools/bench_lig_nd_train.py [--reps 9] [--out profiles/lig_nd_train.json]

Shapes: latent grid [1, 128, 128, 32] (d = 2) and [1, 8, 16, 16, 31] (d = 4), 2^18 points each (nf = 32, softplus, 4 outputs);
gradients w.r.t. the latent grid and all IM-NET parameters of the loss mean(y^2).  Each forward + backward is timed with
device events around it, the two paths alternate inside one process, and the medians over --reps repetitions (after a
warm-up of both) are reported with their spread; the latent gradients of the two paths are compared on the same inputs.
No speed-up is promised: the file records what was measured.  Needs a GPU: there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [dict(name="d2_grid128x128_c32_2^18", d=2, grid=(128, 128), c=32, points=1 << 18),
          dict(name="d4_grid8x16x16x16_c31_2^18", d=4, grid=(8, 16, 16, 16), c=31, points=1 << 18)]


def _time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    y = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lig_nd_train.json"))
    ap.add_argument("--scale", type=int, default=1, help="divide the point counts (rehearsal only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lig_nd_train.py needs a GPU (NOT MEASURED without one)")
    from space_time_pde_amd import implicit_net, lig_jet, local_implicit_grid as lig
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, precision=lig_jet.mlp_precision, shapes={})
    for sh in SHAPES:
        torch.manual_seed(1)
        net = implicit_net.ImNet(dim=sh["d"], in_features=sh["c"], out_features=4, nf=32,
                                 activation=torch.nn.Softplus).to(dev)
        g = torch.Generator().manual_seed(0)
        latent = (0.5 * torch.randn(1, *sh["grid"], sh["c"], generator=g)).to(dev).requires_grad_(True)
        pts = torch.rand(1, sh["points"] // args.scale, sh["d"], generator=g).to(dev)

        def run(hip):
            prev = lig_jet.set_nd_backward(hip)
            try:
                key = "hip_value_calls" if hip else "generic_calls"
                n0 = lig.stats[key]
                latent.grad = None
                net.zero_grad(set_to_none=True)
                y = lig.query_local_implicit_grid(net, latent, pts, 0., 1.)
                assert lig.stats[key] == n0 + 1, "the %s path was not taken" % ("HIP" if hip else "composed")
                (y * y).mean().backward()
                return latent.grad
            finally:
                lig_jet.set_nd_backward(prev)

        ga, gb = run(True).clone(), run(False).clone()          # warm-up of both paths at the timed shape
        torch.cuda.synchronize()
        diff = ((ga - gb).abs().max() / gb.abs().max()).item()
        del ga, gb
        t_hip, t_cmp = [], []
        for _ in range(args.reps):
            t_hip.append(_time(lambda: run(True))[0])
            t_cmp.append(_time(lambda: run(False))[0])
        med_h, med_c = statistics.median(t_hip), statistics.median(t_cmp)
        result["shapes"][sh["name"]] = dict(
            points=pts.shape[1], hip_ms_median=round(med_h, 3), composed_ms_median=round(med_c, 3),
            hip_ms_min_max=[round(min(t_hip), 3), round(max(t_hip), 3)],
            composed_ms_min_max=[round(min(t_cmp), 3), round(max(t_cmp), 3)],
            speedup_composed_over_hip=round(med_c / med_h, 2), max_rel_diff_of_dlatent=diff)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
