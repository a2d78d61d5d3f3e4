#!/usr/bin/env python3
"""Timing driver for the pressure kernels against the velocity kernels of the
same sources and targets.

For each kernel (stokeslet, stresslet, oseen) and shape it times, on cuda:0
and in the same process,
  pressure  the pressure kernel at n_trg targets (1 output a target),
  vel       the matching velocity kernel at n_trg targets (3 outputs),
alternating the two in every round. Each sample is device events around
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
    p.add_argument("--kernels", nargs="+", default=["stokeslet", "stresslet", "oseen"])
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
        sys.exit("prof_pressure needs a GPU")
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
    }
    pressure = {
        "stokeslet": lambda t, o: ska.stokeslet_pressure_device(r_src, f3, t, out=o),
        "stresslet": lambda t, o: ska.stresslet_pressure_device(r_src, f9, t, out=o),
        "oseen": lambda t, o: ska.oseen_contract_pressure_device(r_src, t, f3, out=o),
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
        trg = to(rng.uniform(-1, 1, (n_trg, 3)))
        p_out = torch.empty(n_trg, dtype=torch.float64, device=dev)
        u_out = torch.empty_like(trg)
        for name in args.kernels:
            runs = {"pressure": lambda: pressure[name](trg, p_out),
                    "vel": lambda: vel[name](trg, u_out)}
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
                "pressure_ms": med["pressure"], "vel_ms": med["vel"],
                "pressure_ms_min_max": [min(ms["pressure"]), max(ms["pressure"])],
                "vel_ms_min_max": [min(ms["vel"]), max(ms["vel"])],
                "pressure_pairs_per_s": pairs / (med["pressure"] * 1e-3),
                "vel_pairs_per_s": pairs / (med["vel"] * 1e-3),
                "pressure_over_vel": med["pressure"] / med["vel"],
                "iters": args.iters, "rounds": args.rounds,
            }
            rows.append(row)
            print(json.dumps(row), flush=True)

    lines = ["| kernel | n_src | n_trg | pressure ms (min-max) | pressure pairs/s | "
             "vel ms (min-max) | vel pairs/s | pressure / vel |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(
            f"| {r['kernel']} | {r['n_src']} | {r['n_trg']} | {r['pressure_ms']:.3f} "
            f"({r['pressure_ms_min_max'][0]:.3f}-{r['pressure_ms_min_max'][1]:.3f}) | "
            f"{r['pressure_pairs_per_s']:.3e} | {r['vel_ms']:.3f} "
            f"({r['vel_ms_min_max'][0]:.3f}-{r['vel_ms_min_max'][1]:.3f}) | "
            f"{r['vel_pairs_per_s']:.3e} | {r['pressure_over_vel']:.3f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
