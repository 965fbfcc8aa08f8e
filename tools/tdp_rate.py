#!/usr/bin/env python3
"""Time-expanded subset DP (algorithm "tdp", tsp_tdp.hip) on one MI355X:
device time of Context.tsp_tdp at n = 8, 12, 16, 18 and 20 customers on two
instance families, with the nearest-neighbour tour as the upper bound (what
runners.time_expanded uses):
  td     the TSP over the nodes of synth.td_cvrp(n, 1, seed=n) at start 480
         (Euclidean, rush-hour factors: a long horizon, many words per row)
  rand   hourly integers(3, 321) matrices at start 480
Device events around the call, after one warm-up call per shape; median and
min..max of the repeats, the words per row W, the table's bytes and the
2^n n (n-1)/4 W word steps over time.  A shape whose table exceeds
solver.TDP_MAX_WORKSPACE is measured all the same and marked.
  --gap   for the td family at n = 16, seeds 0-4: the optimum and the SA / GA /
          ACO durations at the front-end defaults, with their gaps.
usage: tdp_rate.py [--gap] [--repeats R] [--sizes 8,12,...]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import runners, solver, synth  # noqa: E402
from vrpms_amd.core import TSP, Context  # noqa: E402

START = 480


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return f"median {np.median(ms):10.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)"


def instance(family, n):
    if family == "td":
        return synth.td_cvrp(n, 1, seed=n, start=START).durations
    D = np.random.default_rng(n).integers(3, 321, size=(24, n + 1, n + 1), dtype=np.int64)
    for h in range(24):
        np.fill_diagonal(D[h], 0)
    return D


def rate(args):
    ctx = Context(0)
    for family in ("td", "rand"):
        for n in args.sizes:
            D = instance(family, n)
            bound = runners.nearest_neighbour_duration(D, n, START)
            W = (START % 60 + bound) // 60 + 1
            nbytes = solver.tdp_workspace_bytes(n, START, bound)
            ctx.set_instance(TSP, D, start_times=(START,))
            ref = ctx.tsp_tdp(n, bound)              # warm-up (and the allocator's first block)
            ms = []
            for _ in range(args.repeats):
                t, out = timed(lambda: ctx.tsp_tdp(n, bound))
                assert out == ref
                ms.append(t)
            med = float(np.median(ms))
            steps = (1 << n) * n * (n - 1) / 4 * W
            over = "  OVER TDP_MAX_WORKSPACE" if nbytes > solver.TDP_MAX_WORKSPACE else ""
            print(f"{family:4s} n={n:2d}  W={W:3d}  {stats(ms)}  table {nbytes / 2**20:9.1f} MiB  "
                  f"{steps / (med * 1e-3) / 1e9:7.2f} G word steps/s  bound {bound}  "
                  f"optimum {ref[0] >> 28 & (2**28 - 1)}{over}", flush=True)
            torch.cuda.empty_cache()
    ctx.close()


def gap(args):
    n = 16
    for seed in range(5):
        D = synth.td_cvrp(n, 1, seed=seed, start=START).durations
        cust = list(range(1, n + 1))
        opt = solver.solve_tsp("tdp", D.tolist(), cust, 0, START)["duration"]
        row = [f"td tsp16 seed {seed}: optimum {opt}"]
        for algo in ("sa", "ga", "aco"):
            d = solver.solve_tsp(algo, D.tolist(), cust, 0, START, seed=seed)["duration"]
            row.append(f"{algo} {d} (+{100.0 * (d - opt) / opt:.2f} %)")
        print("  ".join(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gap", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")],
                    default=[8, 12, 16, 18, 20])
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    (gap if a.gap else rate)(a)
