"""Tensor-valued equation coefficients: the HIP residual kernels reading them (``PDELayer(device_params=True)``:
k_residual_coef_fwd / k_residual_coef_bwd, one launch each, the coefficient gradients summed inside the backward) against the
switch off -- the lambdified torch functions and their autograd, about 100 elementwise kernels per step, which is what such a
layer ran before the switch existed and still runs by default.

    python tools/bench_residual_params.py [--reps 9] [--out profiles/residual_params.json]

Two cases, each timed in a fresh child process under its own ``timeout`` (the first one that fails ends the run):

* per_call: RB2 (with continuity) with a Rayleigh number per batch element, shape [B], and a scalar Prandtl number, both
  requiring grad; B = 16 x 4096 = 2^16 points on a [16, 4, 16, 16, 32] latent grid, nf = 32, softplus.  One ``PDELayer`` call plus
  the backward of an l2 loss of prediction and residuals, timed with device events; the two settings alternate inside one
  process and the medians over --reps repetitions (after a warm-up of both) are reported with their spread.
* iteration: the reference training regime of ``bench.py --workload train_default`` (10 crops x 512 points, latent grid
  (4, 16, 16), UNet3d nf = 16 / mf = 256, IM-NET nf = 32, l1, alpha_pde = 0.0125) with learnable Ra [10] and Pr []: the eager
  ``sharded_step`` with ``device_params=False`` against one replay of a ``GraphedStep`` with it on (a layer with the switch off
  cannot be captured), wall-clock per iteration over --steps iterations, alternating, medians of --reps.

No speed-up is asserted.  Needs a GPU: there is no CPU timing.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RB2 = dict(mean=(0.01, 0.0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1., x_crop=1., use_continuity=True)
CASE_TIMEOUT = {"per_call": 240, "iteration": 300}


def _spread(ts):
    return dict(ms_median=round(statistics.median(ts), 4), ms_min_max=[round(min(ts), 4), round(max(ts), 4)])


def per_call(args):
    import torch
    from space_time_pde_amd import implicit_net, local_implicit_grid as lig, physics
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    B, N = 16, (1 << 16) // 16 // args.scale
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)
    g = torch.Generator().manual_seed(0)
    latent = (0.5 * torch.randn(B, 4, 16, 16, 32, generator=g)).to(dev).requires_grad_(True)
    pts = (0.02 + 0.96 * torch.rand(B, N, 3, generator=g)).to(dev)
    tgt = torch.randn(B, N, 4, generator=g).to(dev)
    Ra = torch.logspace(4, 6, B).to(dev).requires_grad_(True)
    Pr = torch.tensor(0.7, device=dev, requires_grad=True)
    leaves = [latent, Ra, Pr] + list(net.parameters())
    layers = {flag: physics.get_rb2_pde_layer(rayleigh=Ra, prandtl=Pr, device_params=flag, **RB2) for flag in (False, True)}
    for layer in layers.values():
        layer.update_forward_method(lambda q: lig.query_local_implicit_grid(net, latent, q, 0., 1.))

    def run(flag):
        for t in leaves:
            t.grad = None
        f0 = lig.stats.get("residual_torch_fallbacks", 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pred, res = layers[flag](pts, return_residue=True)
        loss = ((pred - tgt) ** 2).mean() + (torch.stack(list(res.values())) ** 2).mean()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        assert lig.stats.get("residual_torch_fallbacks", 0) == f0 + (0 if flag else 1), "the wrong residual path was taken"
        return e0.elapsed_time(e1), loss.item(), Ra.grad.clone(), Pr.grad.clone()

    a, b = run(True), run(False)            # warm-up of both settings at the timed shape
    diff = dict(loss=abs(a[1] - b[1]) / abs(b[1]), dRa=((a[2] - b[2]).abs().max() / b[2].abs().max()).item(),
                dPr=((a[3] - b[3]).abs() / b[3].abs()).item())
    t_dev, t_torch = [], []
    for _ in range(args.reps):
        t_dev.append(run(True)[0])
        t_torch.append(run(False)[0])
    return dict(problem="RB2 + continuity, Ra [B] and Pr [] learnable; one PDELayer call + backward of an l2 loss",
                batch=B, points=B * N, latent=[B, 4, 16, 16, 32], nf=32, reps=args.reps,
                device_params=_spread(t_dev), torch_functions=_spread(t_torch),
                ratio_torch_over_device=round(statistics.median(t_torch) / statistics.median(t_dev), 3), max_rel_diff=diff)


def iteration(args):
    import torch
    from space_time_pde_amd import implicit_net, optim, physics, unet3d
    from space_time_pde_amd.train_step import GraphedStep, sharded_step
    dev = torch.device("cuda:0")
    B, N = 10, 512
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(B, 4, 4, 16, 16, generator=g).to(dev), (0.02 + 0.96 * torch.rand(B, N, 3, generator=g)).to(dev),
             torch.randn(B, N, 4, generator=g).to(dev))

    def build(flag):
        torch.manual_seed(3)
        unet = unet3d.UNet3d(in_features=4, out_features=32, igres=(4, 16, 16), nf=16, mf=256).to(dev).train()
        net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)
        Ra = torch.logspace(4, 6, B).to(dev).requires_grad_(True)
        Pr = torch.tensor(0.7, device=dev, requires_grad=True)
        layer = physics.get_rb2_pde_layer(rayleigh=Ra, prandtl=Pr, device_params=flag, **RB2)
        params = list(unet.parameters()) + list(net.parameters())      # (the coefficients get gradients; the networks are updated)
        opt = optim.FusedClipAdam(params, lr=1e-2, clip_grad=1.0, capturable=flag)
        return unet, net, layer, opt

    unet0, net0, layer0, opt0 = build(False)
    unet1, net1, layer1, opt1 = build(True)

    def eager_iter():
        opt0.zero_grad()
        sharded_step(unet0, net0, layer0, *batch, N, 1.0, 0.0125, "l1", distributed=False)
        opt0.step()

    for _ in range(3):
        eager_iter()
    torch.cuda.synchronize()
    gstep = GraphedStep(unet1, net1, layer1, *batch, N, 1.0, 0.0125, "l1", optimizer=opt1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    timed(eager_iter), timed(gstep)
    t_graph, t_eager = [], []
    for _ in range(args.reps):
        t_graph.append(timed(gstep))
        t_eager.append(timed(eager_iter))
    return dict(problem="train_default iteration (10 crops x 512 points, latent (4,16,16)) with learnable Ra [10] and Pr []: "
                        "forward, backward, clip, Adam", steps_per_repetition=args.steps, reps=args.reps,
                graphed_device_params=_spread(t_graph), eager_torch_functions=_spread(t_eager),
                ratio_eager_over_graphed=round(statistics.median(t_eager) / statistics.median(t_graph), 3),
                graph_replays=gstep.replays)


CASES = {"per_call": per_call, "iteration": iteration}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20, help="iterations per repetition of the iteration case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_params.json"))
    ap.add_argument("--scale", type=int, default=1, help="divide the per_call point count (rehearsal only)")
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="run ONE case in this process and print its JSON")
    args = ap.parse_args()
    if args.case:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_residual_params.py needs a GPU (NOT MEASURED without one)")
        out = CASES[args.case](args)
        out["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(out))
        return
    result = {}
    for case in ("per_call", "iteration"):
        cmd = ["timeout", "-k", "10", str(CASE_TIMEOUT[case]), sys.executable, os.path.abspath(__file__), "--case", case,
               "--reps", str(args.reps), "--steps", str(args.steps), "--scale", str(args.scale)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
        if run.returncode != 0 or not lines:
            sys.stdout.write(run.stdout)
            raise SystemExit("case %s ended with status %d: nothing written" % (case, run.returncode))
        result[case] = json.loads(lines[-1][7:])
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
