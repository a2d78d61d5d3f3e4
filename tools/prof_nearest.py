#!/usr/bin/env python3
"""Timing driver for the nearest-source kernel, beside the host cKDTree route.

Shapes (defaults):
  shell    128 000 targets x 6 431 sources, ungrouped: config-5 fiber nodes
           against the oocyte shell (tests/golden/oocyte_nodes.npz);
  fibers   128 000 x 128 000 grouped (4 000 fibers of 32 nodes, targets equal
           to sources): SystemFD.min_fiber_gap's launch.
For each it times, on cuda:0,
  device   evaluator.nearest_device on resident tensors: device events around
           `--iters` back-to-back calls after a warm-up, the median over
           `--rounds` samples (the call is the staging, the record packing, the
           pair kernel, the slice reduce and the unpack);
and, on the host and in the same process,
  ckdtree  what SystemFD._fiber_fiber_repulsion spends on proximity:
           scipy.spatial.cKDTree(points).query_pairs(d_max) at its default
           cutoff 0.275 for the fibers shape (the tree finds all pairs under
           the cutoff, not the nearest one: the two are put beside each other,
           not equated), and cKDTree(shell).query(points) for the shell shape.
The figure pairs/s is n_src x n_trg over the device time; ops/pair is counted
from the functor (3 subtractions, 1 multiply, 2 fma, 2 compares in fp64 and 4
32-bit selects). Prints one JSON line per case and a markdown table (also
written to --out when given)."""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

FP64_OPS_PER_PAIR = 8  # 3 sub, 1 mul, 2 fma, 2 cmp (v_add/v_mul/v_fma/v_cmp _f64)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-trg", type=int, default=128_000)
    p.add_argument("--fibers", type=int, default=4000)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--host-rounds", type=int, default=3)
    p.add_argument("--seed", type=int, default=100)
    p.add_argument("--out", default=None, help="also write the markdown table here")
    args = p.parse_args()

    import skellysim_amd as ska
    if not torch.cuda.is_available():
        sys.exit("prof_nearest needs a GPU")
    from scipy.spatial import cKDTree
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    fx = np.load(os.path.join(REPO, "tests", "golden", "oocyte_nodes.npz"))
    shell, normals = fx["nodes"], fx["normals"]
    # fiber nodes inside the shell: straight fibers from random shell nodes
    # along the inward normal, 32 nodes over a length of 1
    n_nodes = args.n_trg // args.fibers
    base = rng.integers(0, len(shell), args.fibers)
    s = np.linspace(0.05, 1.05, n_nodes)
    pts = (shell[base, None, :] + s[None, :, None] * normals[base, None, :]).reshape(-1, 3)
    pts += 1e-3 * rng.normal(size=pts.shape)
    fid = np.repeat(np.arange(args.fibers, dtype=np.int64), n_nodes)

    d_shell, d_pts, d_fid = to(shell), to(pts), to(fid)
    cases = {
        "shell": dict(n_src=len(shell), n_trg=len(pts),
                      device=lambda: ska.nearest_device(d_shell, d_pts),
                      host=lambda: cKDTree(shell).query(pts)),
        "fibers": dict(n_src=len(pts), n_trg=len(pts),
                       device=lambda: ska.nearest_device(d_pts, d_pts, d_fid, d_fid),
                       host=lambda: cKDTree(pts).query_pairs(r=0.275, output_type="ndarray")),
    }

    def sample(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters  # ms per call

    rows = []
    for name, c in cases.items():
        c["device"]()
        c["device"]()  # warm up: code objects, the workspace
        torch.cuda.synchronize()
        ms = [sample(c["device"]) for _ in range(args.rounds)]
        host = []
        for _ in range(args.host_rounds):
            t0 = time.perf_counter()
            found = c["host"]()
            host.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ms)
        pairs = float(c["n_src"]) * c["n_trg"]
        d2, idx = c["device"]()
        torch.cuda.synchronize()
        row = {
            "case": name, "n_src": c["n_src"], "n_trg": c["n_trg"],
            "device_ms": med, "device_ms_min_max": [min(ms), max(ms)],
            "pairs_per_s": pairs / (med * 1e-3),
            "fp64_valu_ops_per_s": FP64_OPS_PER_PAIR * pairs / (med * 1e-3),
            "ckdtree_ms": statistics.median(host), "ckdtree_ms_min_max": [min(host), max(host)],
            "ckdtree_found": int(len(found[0]) if isinstance(found, tuple) else len(found)),
            "min_distance": float(d2.min().sqrt()), "iters": args.iters, "rounds": args.rounds,
        }
        rows.append(row)
        print(json.dumps(row), flush=True)

    lines = ["| case | n_src | n_trg | device ms (min-max) | pairs/s | fp64 VALU ops/s | "
             "host cKDTree ms (min-max) |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(
            f"| {r['case']} | {r['n_src']} | {r['n_trg']} | {r['device_ms']:.3f} "
            f"({r['device_ms_min_max'][0]:.3f}-{r['device_ms_min_max'][1]:.3f}) | "
            f"{r['pairs_per_s']:.3e} | {r['fp64_valu_ops_per_s']:.3e} | {r['ckdtree_ms']:.1f} "
            f"({r['ckdtree_ms_min_max'][0]:.1f}-{r['ckdtree_ms_min_max'][1]:.1f}) |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    main()
