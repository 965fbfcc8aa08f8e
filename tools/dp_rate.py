#!/usr/bin/env python3
"""Held-Karp (algorithm "dp", tsp_dp.hip) on one MI355X: device time of
Context.tsp_dp on symmetric randint(3, 320) matrices of n = 13, 16, 19, 20,
22 and 24 customers (device events around the call, after one warm-up call
per shape; median and min..max of the repeats), the table's bytes and bytes
over time; at n = 13 the brute-force kernel in the same process, the two
alternating.
  --gap   for synth.tsp20(seed), seeds 0-4: the optimum and the SA / GA /
          ACO durations at the front-end defaults, with their gaps.
usage: dp_rate.py [--gap] [--repeats R] [--sizes 13,16,...]"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import solver, synth  # noqa: E402
from vrpms_amd.core import TSP, Context  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return f"median {np.median(ms):9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)"


def rate(args):
    ctx = Context(0)
    for n in args.sizes:
        D = synth.random_symmetric(n + 1, np.random.default_rng(n))
        ctx.set_instance(TSP, D, start_times=(0,))
        nbytes = (1 << n) * (32 if n > 16 else 16) * 4
        ref = ctx.tsp_dp(n)                      # warm-up (and the allocator's first 2 GiB)
        bf_ms, dp_ms = [], []
        for _ in range(args.repeats):
            ms, out = timed(lambda: ctx.tsp_dp(n))
            assert out == ref
            dp_ms.append(ms)
            if n == 13:
                ms, (k, _) = timed(lambda: ctx.bf_run(n, 0, math.factorial(n)))
                assert k == ref[0]
                bf_ms.append(ms)
        med = float(np.median(dp_ms))
        print(f"n={n:2d}  dp  {stats(dp_ms)}  table {nbytes / 2**20:8.1f} MiB  "
              f"{nbytes / (med * 1e-3) / 1e9:8.2f} GB/s of table written  "
              f"optimum {ref[0] >> 28 & (2**28 - 1)}", flush=True)
        if bf_ms:
            print(f"n={n:2d}  bf  {stats(bf_ms)}  ({math.factorial(n):,} tours; "
                  f"bf / dp = {np.median(bf_ms) / med:.1f}x)", flush=True)
    ctx.close()


def gap(args):
    for seed in range(5):
        D = synth.tsp20(seed).durations[0]
        cust = list(range(1, D.shape[0]))
        opt = solver.solve_tsp("dp", D.tolist(), cust, 0)["duration"]
        row = [f"tsp20 seed {seed}: optimum {opt}"]
        for algo in ("sa", "ga", "aco"):
            d = solver.solve_tsp(algo, D.tolist(), cust, 0, seed=seed)["duration"]
            row.append(f"{algo} {d} (+{100.0 * (d - opt) / opt:.2f} %)")
        print("  ".join(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gap", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")],
                    default=[13, 16, 19, 20, 22, 24])
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    (gap if a.gap else rate)(a)
