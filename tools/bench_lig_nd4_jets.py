"""Second-order PDE residuals on a 4-d local implicit grid -- 3-d space + time: ``lig_jet.nd4_jets`` on (k_gather_nd<4> ->
k_coef_nd4 -> per pass of ``lig_jet.nd4_passes`` the IM-NET layer kernels in the pass's stream set -> k_reduce_nd4_jet, one
forward under no_grad) against the switch off, which is what such a PDELayer call ran before the switch existed and still runs
by default: the composed formulation, 16 corners per point, under the reference's reverse sweeps (one ``autograd.grad`` per
``dif``, grad mode on, O(points) graph memory).

    python tools/bench_lig_nd4_jets.py [--reps 9] [--out profiles/lig_nd4_jets.json]

Problem: incompressible Navier-Stokes on (t, x, y, z) with outputs u, v, w, p -- three momentum equations with a Laplacian in
space each plus continuity: all four first derivatives and (x,x), (y,y), (z,z), two passes -- on an 8 x 16 x 16 x 16 grid with
16 latent channels, nf = 32, softplus.  Points per call: the largest power of two <= 2^16 at which the composed side fits the
device (it keeps a higher-order autograd graph over 16 rows per point); the count that ran is recorded.  Each call is timed
with device events around it, the two paths alternate inside one process, and the medians over --reps repetitions (after a
warm-up of both) are reported with their spread; the residuals of the two paths are compared on the same inputs.  Needs a GPU:
there is no CPU timing.
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID, CHANNELS, POINTS = (8, 16, 16, 16), 16, 1 << 16
NU = 1e-2


def equations():
    def momentum(q, grad_p):
        return "dif(%s,t)+u*dif(%s,x)+v*dif(%s,y)+w*dif(%s,z)+dif(p,%s)-%r*(dif(dif(%s,x),x)+dif(dif(%s,y),y)+dif(dif(%s,z),z))" % (
            q, q, q, q, grad_p, NU, q, q, q)

    return [("momentum_u", momentum("u", "x")), ("momentum_v", momentum("v", "y")), ("momentum_w", momentum("w", "z")),
            ("continuity", "dif(u,x)+dif(v,y)+dif(w,z)")]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lig_nd4_jets.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lig_nd4_jets.py needs a GPU (NOT MEASURED without one)")
    from space_time_pde_amd import implicit_net, lig_jet, local_implicit_grid as lig, pde
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    net = implicit_net.ImNet(dim=4, in_features=CHANNELS, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)
    g = torch.Generator().manual_seed(0)
    latent = (0.5 * torch.randn(1, *GRID, CHANNELS, generator=g)).to(dev)
    all_pts = torch.rand(1, POINTS, 4, generator=g).to(dev)
    layer = pde.PDELayer("t, x, y, z", "u, v, w, p")
    for name, eqn in equations():
        layer.add_equation(eqn, name)
    layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latent, q, 0., 1.))

    def run(hip, pts):
        prev = lig_jet.set_nd4_jets(hip)
        try:
            key = "hip_jet_calls" if hip else "generic_calls"
            n0 = lig.stats[key]
            with (torch.no_grad() if hip else torch.enable_grad()):
                _, res = layer(pts.clone(), return_residue=True)
                res = torch.cat([v.detach() for v in res.values()], -1)
            assert lig.stats[key] == n0 + 1, "the %s path was not taken" % ("HIP jet" if hip else "composed")
            return res
        finally:
            lig_jet.set_nd4_jets(prev)

    # the largest power-of-two point count at which the composed side fits (its warm-up is the probe)
    n, rb = all_pts.shape[1], None
    while rb is None:
        try:
            rb = run(False, all_pts[:, :n])
        except torch.OutOfMemoryError:
            rb = None
        if rb is None:          # (outside the except block: the traceback would pin the failed call's graph)
            gc.collect()
            torch.cuda.empty_cache()
            if n <= 1024:
                raise SystemExit("the composed formulation does not fit 1024 points: NOT MEASURED")
            n //= 2
    pts = all_pts[:, :n].contiguous()
    ra = run(True, pts)                         # warm-up of the HIP path at the timed shape
    torch.cuda.synchronize()
    diff = ((ra - rb).abs().max() / rb.abs().max()).item()
    passes = len(lig_jet.nd4_passes(True, [(1, 1), (2, 2), (3, 3)]))
    del ra, rb
    t_hip, t_cmp = [], []
    for _ in range(args.reps):
        t_hip.append(_time(lambda: run(True, pts))[0])
        t_cmp.append(_time(lambda: run(False, pts))[0])
    med_h, med_c = statistics.median(t_hip), statistics.median(t_cmp)
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
                  problem="incompressible Navier-Stokes residuals in (t, x, y, z), 3 momentum equations + continuity",
                  grid=list(GRID), channels=CHANNELS, nf=32, points=n, points_asked=all_pts.shape[1], layer_passes=passes,
                  hip_ms_median=round(med_h, 3), composed_ms_median=round(med_c, 3),
                  hip_ms_min_max=[round(min(t_hip), 3), round(max(t_hip), 3)],
                  composed_ms_min_max=[round(min(t_cmp), 3), round(max(t_cmp), 3)],
                  speedup_composed_over_hip=round(med_c / med_h, 2), max_rel_diff_of_residuals=diff)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
