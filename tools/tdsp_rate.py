#!/usr/bin/env python3
"""Time-expanded partition DP (algorithm "tdsp", vrp_tdsp.hip) on one MI355X:
device time of Context.vrp_tdsp on synth.td_cvrp_het(n, K, seed=n) for n = 8,
12, 16, 18, 20 customers x K = 2, 4, 8 vehicles, sum objective, with the
default upper bound (runners.tdsp_default_bound: what solve_vrp("tdsp") uses).
Device events around the call, after one warm-up call per shape; median and
min..max of the repeats, the bound used, the widest row W, the G distinct
start times and the workspace's bytes.  A shape whose workspace exceeds
solver.TDSP_MAX_WORKSPACE or whose rows exceed 512 words is reported and not
run (the front end refuses it).
The reference for time is the project's own parts at the same shape: for each
distinct start time Context.tsp_tdp (same n, start and bound) on the TSP over
the same nodes, plus Context.vrp_sp (same n, K, demands, capacities) on hour
slice 0 as a static matrix; the ratio is vrp_tdsp over their sum.
  --gap   for synth.td_cvrp_het(12, 4, seed), seeds 0-2: the optimum and the
          SA / GA / ACO primaries at the front-end defaults under a time limit
          of their own (--limit seconds each), with their gaps.
The route kernel's share of the call comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/tdsp_rate.py --sizes 16
--fleets 4), a run of its own.
usage: tdsp_rate.py [--gap] [--repeats R] [--sizes 8,12,...] [--fleets 2,4,8] [--limit S]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import runners, solver, synth  # noqa: E402
from vrpms_amd.core import CVRP, OBJ_SUM, TSP, Context  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def median_ms(fn, repeats):
    ref = fn()                                   # warm-up (and the allocator's first block)
    ms = []
    for _ in range(repeats):
        t, out = timed(fn)
        assert out == ref
        ms.append(t)
    return ms, ref


def rate(args):
    ctx = Context(0)
    for n in args.sizes:
        for K in args.fleets:
            inst = synth.td_cvrp_het(n, K, seed=n)
            D, dem = inst.durations, inst.demand
            caps, starts = inst.capacities.tolist(), inst.start_times.tolist()
            bound = runners.tdsp_default_bound(D, dem, caps, starts, n, False)
            safe = runners.tdsp_safe_bound(D, dem, caps, n)
            distinct = sorted(set(starts))
            G = len(distinct)
            W = max((s % 60 + bound) // 60 + 1 for s in starts)
            nbytes = solver.tdsp_workspace_bytes(n, K, G, max(starts), bound)
            head = (f"n={n:2d} K={K} G={G}  bound {bound} (safe {safe})  W={W:3d}  workspace "
                    f"{nbytes / 2**20:9.1f} MiB")
            if nbytes > solver.TDSP_MAX_WORKSPACE or W > solver.TDP_MAX_WORDS:
                print(f"{head}  NOT RUN: over TDSP_MAX_WORKSPACE or 512 words", flush=True)
                continue
            ctx.set_instance(CVRP, D, dem, caps, starts, objective=OBJ_SUM)
            ms, ref = median_ms(lambda: ctx.vrp_tdsp(n, bound), args.repeats)
            torch.cuda.empty_cache()
            parts = 0.0
            for s in distinct:
                ctx.set_instance(TSP, D, start_times=(s,))
                t, _ = median_ms(lambda: ctx.tsp_tdp(n, bound), args.repeats)
                parts += float(np.median(t))
                torch.cuda.empty_cache()
            ctx.set_instance(CVRP, D[0], dem, caps, starts, objective=OBJ_SUM)
            t, _ = median_ms(lambda: ctx.vrp_sp(n), args.repeats)
            sp = float(np.median(t))
            med = float(np.median(ms))
            print(f"{head}  median {med:10.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, "
                  f"{len(ms)} runs)  parts: {G} x tsp_tdp {parts:.3f} ms + vrp_sp {sp:.3f} ms  "
                  f"ratio {med / (parts + sp):5.2f}  unvisited {ref[0] >> 56} primary "
                  f"{ref[0] >> 28 & (2**28 - 1)}", flush=True)
            torch.cuda.empty_cache()
    ctx.close()


def gap(args):
    for seed in range(3):
        inst = synth.td_cvrp_het(12, 4, seed=seed)
        D = inst.durations.tolist()
        locs = [{"id": i, "demand": int(d)} for i, d in enumerate(inst.demand)]
        caps, starts = inst.capacities.tolist(), inst.start_times.tolist()
        opt = solver.solve_vrp("tdsp", D, locs, caps, starts, with_unvisited=True)
        row = [f"td_cvrp_het(12, 4) seed {seed} sum: optimum {opt['durationSum']} "
               f"(unvisited {len(opt['unvisited'])})"]
        for algo in ("sa", "ga", "aco"):
            h = solver.solve_vrp(algo, D, locs, caps, starts, seed=seed, time_limit=args.limit,
                                 with_unvisited=True)
            row.append(f"{algo} {h['durationSum']} "
                       f"(+{100.0 * (h['durationSum'] - opt['durationSum']) / opt['durationSum']:.2f} %"
                       + (f", {len(h['unvisited'])} unvisited)" if h["unvisited"] else ")"))
        print("  ".join(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gap", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    ap.add_argument("--sizes", type=ints, default=[8, 12, 16, 18, 20])
    ap.add_argument("--fleets", type=ints, default=[2, 4, 8])
    ap.add_argument("--limit", type=float, default=2.0)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    (gap if a.gap else rate)(a)
