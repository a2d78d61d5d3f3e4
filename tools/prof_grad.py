#!/usr/bin/env python3
"""Timing driver for the analytic velocity-gradient kernels against the
finite-difference route they replace.

For each kernel and shape it times, on cuda:0 and in the same process,
  grad      the gradient kernel at n_trg targets (9 outputs a target),
  vel       the matching velocity kernel at n_trg targets,
  vel x6    the velocity kernel at the 6 n_trg probe points of a central
            difference (listener.vorticity's route to one curl per target),
alternating the three in every round. Each sample is device events around
`--iters` back-to-back launches after a warm-up of every shape; the figure
reported is the median over `--rounds` samples. Prints one JSON line per case
and a markdown table (also written to --out when given)."""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-src", type=int, default=100_000)
    p.add_argument("--n-trg", type=int, nargs="+", default=[100_000, 4096])
    p.add_argument("--kernels", nargs="+",
                   default=["stokeslet", "stresslet", "oseen", "rotlet"])
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--seed", type=int, default=100)
    p.add_argument("--lib", default=None,
                   help="load this build of libskellyhip.so instead of the in-tree one "
                        "(A/B of compile-time knobs)")
    p.add_argument("--out", default=None, help="also write the markdown table here")
    args = p.parse_args()

    from skellysim_amd import _native
    if args.lib:
        _native._LIB_PATH = os.path.abspath(args.lib)
    import skellysim_amd as ska

    if not torch.cuda.is_available():
        sys.exit("prof_grad needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    r_src = to(rng.uniform(-1, 1, (args.n_src, 3)))
    f3 = to(rng.uniform(-1, 1, (args.n_src, 3)))
    f9 = to(rng.uniform(-1, 1, (args.n_src, 9)))

    vel = {
        "stokeslet": lambda t, o: ska.stokeslet_device(r_src, f3, t, 1.0, out=o),
        "stresslet": lambda t, o: ska.stresslet_device(r_src, f9, t, 1.0, out=o),
        "oseen": lambda t, o: ska.oseen_contract_device(r_src, t, f3, 1.0, out=o),
        "rotlet": lambda t, o: ska.rotlet_device(r_src, t, f3, 1.0, out=o),
    }
    grad = {
        "stokeslet": lambda t, o: ska.stokeslet_grad_device(r_src, f3, t, 1.0, out=o),
        "stresslet": lambda t, o: ska.stresslet_grad_device(r_src, f9, t, 1.0, out=o),
        "oseen": lambda t, o: ska.oseen_contract_grad_device(r_src, t, f3, 1.0, out=o),
        "rotlet": lambda t, o: ska.rotlet_grad_device(r_src, t, f3, 1.0, out=o),
    }

    def sample(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters  # ms per launch

    rows = []
    for n_trg in args.n_trg:
        trg_np = rng.uniform(-1, 1, (n_trg, 3))
        probes_np = np.repeat(trg_np, 6, axis=0)  # listener.vorticity's probes
        for k in range(3):
            probes_np[2 * k::6, k] += 1e-7
            probes_np[2 * k + 1::6, k] -= 1e-7
        trg, probes = to(trg_np), to(probes_np)
        g_out = torch.empty((n_trg, 3, 3), dtype=torch.float64, device=dev)
        u_out, u6_out = torch.empty_like(trg), torch.empty_like(probes)
        for name in args.kernels:
            runs = {"grad": lambda: grad[name](trg, g_out),
                    "vel": lambda: vel[name](trg, u_out),
                    "vel_x6": lambda: vel[name](probes, u6_out)}
            for fn in runs.values():  # warm up every shape
                fn()
                fn()
            torch.cuda.synchronize()
            ms = {key: [] for key in runs}
            for _ in range(args.rounds):
                for key, fn in runs.items():
                    ms[key].append(sample(fn))
            med = {key: statistics.median(v) for key, v in ms.items()}
            pairs = float(args.n_src) * n_trg
            row = {
                "kernel": name, "n_src": args.n_src, "n_trg": n_trg,
                "grad_ms": med["grad"], "vel_ms": med["vel"], "vel_x6_ms": med["vel_x6"],
                "grad_ms_min_max": [min(ms["grad"]), max(ms["grad"])],
                "vel_x6_ms_min_max": [min(ms["vel_x6"]), max(ms["vel_x6"])],
                "grad_pairs_per_s": pairs / (med["grad"] * 1e-3),
                "vel_pairs_per_s": pairs / (med["vel"] * 1e-3),
                "grad_over_vel_x6": med["grad"] / med["vel_x6"],
                "iters": args.iters, "rounds": args.rounds,
            }
            rows.append(row)
            print(json.dumps(row), flush=True)

    lines = ["| kernel | n_src | n_trg | grad ms | grad pairs/s | vel ms | vel pairs/s | "
             "vel x6 ms | grad / (vel x6) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['kernel']} | {r['n_src']} | {r['n_trg']} | {r['grad_ms']:.3f} | "
                     f"{r['grad_pairs_per_s']:.3e} | {r['vel_ms']:.3f} | "
                     f"{r['vel_pairs_per_s']:.3e} | {r['vel_x6_ms']:.3f} | "
                     f"{r['grad_over_vel_x6']:.3f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
