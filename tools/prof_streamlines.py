#!/usr/bin/env python3
"""Timing driver for the listener's two streamline routes on one frame of
BASELINE config-4 shape: `--fibers` x `--nodes` fiber nodes (512 x 64) inside
the 8192-node ellipsoidal periphery of tests/golden, with a synthetic state
(bent fibers with random tensions, a random shell density): the routes' cost
depends on the counts, not on the values.

  device  process_streamlines with "device": true: sources built once, one
          launch of the tracer kernel for all seeds. Timed as a whole request
          (wall clock around the call, which ends with the copy back), and the
          kernel launch alone (device events around
          evaluator.trace_streamlines_device on resident tensors).
  host    the default route: scipy's RK45, one velocity_field call per
          right-hand side. One right-hand side is timed on its own
          (`--rhs-calls` calls of velocity_field at one point); a whole line is
          run for the first `--host-seeds` seeds only if that figure times
          `--host-rhs-estimate` calls a line stays under `--host-budget`
          seconds. The route is a Python loop over the seeds, so its time is
          linear in their number.

`--field vorticity` times the vortex lines instead: the device route is the
`vortexlines` request with "tracer": "device" and its launch
evaluator.trace_vortexlines_device, the streamline launch is timed beside it at
the same shape (`streamline_launch_s`), and the host route is the
`"analytic": true` one (a velocity_gradient_field and a velocity_field call per
right-hand side).

`--lib` loads another build of the library (the workgroup-size sweep builds
it with EXTRA=-DSKELLY_TRACE_BLOCK=512 / 1024); the size in use is printed.
Prints one JSON line per measurement and a markdown table (also written to
--out when given)."""

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


def config4_frame(n_fibers, n_nodes, shell_nodes, shell_normals, rng):
    """A frame as listener.Trajectory decodes it, of config-4 shape."""
    from skellysim_amd.fiber_fd import FiberFD
    from skellysim_amd.listener import eigen_decode
    from skellysim_amd.trajectory import eigen, fiber_map
    # fibers grow inwards from points of the periphery, slightly bent
    base = shell_nodes[rng.choice(len(shell_nodes), n_fibers, replace=False)]
    inward = -shell_normals[rng.choice(len(shell_nodes), n_fibers, replace=False)]
    s = np.linspace(0.0, 1.0, n_nodes)
    maps = []
    for b, d in zip(base, inward):
        d = d / np.linalg.norm(d)
        side = np.cross(d, [0.3, 0.5, 0.8])
        x = 0.95 * b[None, :] + s[:, None] * d[None, :] + \
            0.05 * np.sin(np.pi * s)[:, None] * side[None, :]
        f = FiberFD(x, length=1.0, bending_rigidity=2.5e-3, eta=1.0)
        f.tension = rng.uniform(-1, 1, n_nodes)
        maps.append(fiber_map(f))
    frame = {"time": 0.1, "fibers": ["FiniteDifference", maps],
             "shell": {"solution_vec_": eigen(1e-2 * rng.uniform(-1, 1, 3 * len(shell_nodes)))}}
    return eigen_decode(frame)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--fibers", type=int, default=512)
    p.add_argument("--nodes", type=int, default=64)
    p.add_argument("--seeds", type=int, nargs="+", default=[1, 16, 256])
    p.add_argument("--t-final", type=float, default=1.0)
    p.add_argument("--max-points", type=int, default=4096)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--rhs-calls", type=int, default=3)
    p.add_argument("--host-seeds", type=int, default=1)
    p.add_argument("--host-rhs-estimate", type=int, default=400)
    p.add_argument("--host-budget", type=float, default=120.0)
    p.add_argument("--no-host", action="store_true",
                   help="device route only (the workgroup-size sweep)")
    p.add_argument("--field", choices=["velocity", "vorticity"], default="velocity",
                   help="streamlines (default) or vortex lines")
    p.add_argument("--seed", type=int, default=100)
    p.add_argument("--lib", default=None,
                   help="load this build of libskellyhip.so instead of the in-tree one")
    p.add_argument("--out", default=None, help="also write the markdown table here")
    args = p.parse_args()

    from skellysim_amd import _native
    if args.lib:
        _native._LIB_PATH = os.path.abspath(args.lib)
    if not torch.cuda.is_available():
        sys.exit("prof_streamlines needs a GPU")
    from skellysim_amd import evaluator, listener
    from skellysim_amd.config import _geometry_fields
    from skellysim_amd.flows import streamline_source_sets
    from skellysim_amd.system_fd import HipBackend

    block = _native.lib().skelly_trace_block_size()
    rng = np.random.default_rng(args.seed)
    nodes, normals, _ = _geometry_fields(
        np.load(os.path.join(REPO, "tests", "golden", "ellipsoid_8192_nodes.npz")))
    shell = {"nodes": np.asarray(nodes, float), "normals": np.asarray(normals, float)}
    frame = config4_frame(args.fibers, args.nodes, shell["nodes"], shell["normals"], rng)
    backend = HipBackend()
    # seeds well inside the periphery
    lo, hi = shell["nodes"].min(axis=0), shell["nodes"].max(axis=0)
    all_seeds = 0.5 * (lo + hi) + 0.25 * (hi - lo) * rng.uniform(-1, 1, (max(args.seeds), 3))
    request = {"dt_init": 0.1, "t_final": args.t_final, "abs_err": 1e-10, "rel_err": 1e-6,
               "back_integrate": True}
    vortex = args.field == "vorticity"
    device_key = {"tracer": "device"} if vortex else {"device": True}
    trace = evaluator.trace_vortexlines_device if vortex else evaluator.trace_streamlines_device
    rows = []

    def emit(row):
        row.update(field=args.field, block=block, fibers=args.fibers, nodes=args.nodes,
                   shell_nodes=len(shell["nodes"]), t_final=args.t_final)
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- device route -----------------------------------------------------------
    terms = listener.streamline_terms(frame, 1.0, shell)
    to = lambda a: backend._t(np.ascontiguousarray(a, dtype=np.float64))
    sets = streamline_source_sets(1.0, to=to, **terms)
    for n in args.seeds:
        x0 = all_seeds[:n]
        req = dict(request, x0=x0, max_points=args.max_points, **device_key)
        listener.process_streamlines(frame, req, 1.0, backend, shell, vortex=vortex)  # warm-up
        wall = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lines = listener.process_streamlines(frame, req, 1.0, backend, shell, vortex=vortex)
            wall.append(time.perf_counter() - t0)
        seeds_dev = to(x0)

        def launches(fn):
            """Device-event times of rounds launches after one warm-up, and the last result."""
            took = []
            for _ in range(args.rounds + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(seeds_dev, 1.0, **sets, dt_init=0.1, t_final=args.t_final,
                         max_points=args.max_points)
                e1.record()
                e1.synchronize()
                took.append(e0.elapsed_time(e1) * 1e-3)
            return took[1:], out

        kernel, out = launches(trace)
        count, status = out["count"].cpu().numpy(), out["status"].cpu().numpy()
        row = {"route": "device", "seeds": n, "request_s": statistics.median(wall),
               "request_s_min_max": [min(wall), max(wall)],
               "launch_s": statistics.median(kernel), "launch_s_min_max": [min(kernel), max(kernel)],
               "points": int(count.sum()), "points_max": int(count.max()),
               "status": np.bincount(status, minlength=4).tolist(),
               "line_points": [len(s["time"]) for s in lines[:4]]}
        if vortex:  # the streamline launch at the same shape, in the same run
            other, out = launches(evaluator.trace_streamlines_device)
            row.update(streamline_launch_s=statistics.median(other),
                       streamline_launch_s_min_max=[min(other), max(other)],
                       streamline_points=int(out["count"].sum().item()))
        emit(row)

    # ---- host route -------------------------------------------------------------
    if not args.no_host:
        host_route(args, frame, shell, backend, all_seeds, request, emit)

    lines = [f"| route | seeds | request s (min-max) | launch s (min-max) | points | "
             f"status 0/1/2/3 |", "|---|---|---|---|---|---|"]
    for r in rows:
        if r["route"] == "device":
            lines.append(
                f"| device, block {block} | {r['seeds']} | {r['request_s']:.4f} "
                f"({r['request_s_min_max'][0]:.4f}-{r['request_s_min_max'][1]:.4f}) | "
                f"{r['launch_s']:.4f} ({r['launch_s_min_max'][0]:.4f}-"
                f"{r['launch_s_min_max'][1]:.4f}) | {r['points']} | "
                f"{'/'.join(map(str, r['status']))} |")
            if "streamline_launch_s" in r:
                lo, hi = r["streamline_launch_s_min_max"]
                lines.append(f"| device streamlines, launch alone | {r['seeds']} | | "
                             f"{r['streamline_launch_s']:.4f} ({lo:.4f}-{hi:.4f}) | "
                             f"{r['streamline_points']} | |")
        elif "request_s" in r:
            calls = f"{r['velocity_field_calls']} velocity_field calls"
            if "velocity_gradient_field_calls" in r:
                calls += f", {r['velocity_gradient_field_calls']} velocity_gradient_field calls"
            lines.append(f"| host | {r['seeds']} | {r['request_s']:.2f} ({calls}) | | | |")
        elif "rhs_s" in r:
            lines.append(f"| host, one right-hand side | | {r['rhs_s']:.4f} | | | |")
        else:
            lines.append(f"| host, not run | | est. {r['estimate_s_per_seed']:.0f} a seed | | | |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(table + "\n")


def host_route(args, frame, shell, backend, all_seeds, request, emit):
    from skellysim_amd import listener
    vortex = args.field == "vorticity"
    one = all_seeds[:1]

    def rhs_once():
        listener.velocity_field(frame, one, 1.0, backend, shell)
        if vortex:  # the analytic route: the curl's gradient, and the velocity for the stop
            listener.velocity_gradient_field(frame, one, 1.0, backend, shell)
    rhs_once()
    t0 = time.perf_counter()
    for _ in range(args.rhs_calls):
        rhs_once()
    rhs = (time.perf_counter() - t0) / args.rhs_calls
    what = ("velocity_gradient_field and velocity_field at 1 point" if vortex
            else "velocity_field at 1 point")
    emit({"route": "host", "what": f"one right-hand side ({what})",
          "rhs_s": rhs, "rhs_calls": args.rhs_calls})
    if args.host_seeds and rhs * args.host_rhs_estimate * args.host_seeds <= args.host_budget:
        calls = {"velocity_field": 0, "velocity_gradient_field": 0}
        real = {name: getattr(listener, name) for name in calls}

        def counted(name):
            def call(*a, **k):
                calls[name] += 1
                return real[name](*a, **k)
            return call
        for name in calls:
            setattr(listener, name, counted(name))
        try:
            t0 = time.perf_counter()
            req = dict(request, x0=all_seeds[:args.host_seeds])
            if vortex:
                req["analytic"] = True
            lines = listener.process_streamlines(frame, req, 1.0, backend, shell, vortex=vortex)
            took = time.perf_counter() - t0
        finally:
            for name in calls:
                setattr(listener, name, real[name])
        row = {"route": "host", "seeds": args.host_seeds, "request_s": took,
               "velocity_field_calls": calls["velocity_field"],
               "line_points": [len(s["time"]) for s in lines[:4]]}
        if vortex:
            row["velocity_gradient_field_calls"] = calls["velocity_gradient_field"]
        emit(row)
    else:
        emit({"route": "host", "what": "whole line not run: over --host-budget",
              "estimate_s_per_seed": rhs * args.host_rhs_estimate})


if __name__ == "__main__":
    main()
