#!/usr/bin/env python3
"""Set partitioning (algorithm "sp", vrp_sp.hip) on one MI355X: device time
of Context.vrp_sp on synth.cvrp(n, K, seed=n, slack=1.2) for n = 8, 10, 13,
16, 18, 20 customers x K = 2, 4, 8 vehicles, both objectives (device events
around the call, after one warm-up call per shape; median and min..max of
the repeats), the recurrence's 3^n K submask steps per second, and the
steps of the K - 1 layers that are launched (vehicle 0's is a copy; sets too
heavy for the fleet so far are skipped; counted on the host) per second and
as a fraction of Context.probe_l2_gather()'s measured gather rate at two
gathers per step.
  --gap   for synth.cvrp(16, 4, seed, slack=1.2), seeds 0-2: the optimum and
          the SA / GA / ACO primaries at the front-end defaults under a time
          limit of their own (--limit seconds each), with their gaps.
usage: sp_rate.py [--gap] [--repeats R] [--sizes 8,10,...] [--fleets 2,4,8] [--limit S]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import solver, synth  # noqa: E402
from vrpms_amd.core import CVRP, OBJ_MAX, OBJ_SUM, Context  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def launched_steps(inst, n):
    """Submask steps of the layers vrpms_vrp_sp_run launches: vehicle k >= 1
    prices the 2^|S| submasks of every S that vehicles 0..k can carry."""
    dem = np.zeros(1, dtype=np.int64)
    pc = np.zeros(1, dtype=np.int64)
    for c in range(1, n + 1):
        dem = np.concatenate([dem, dem + int(inst.demand[c])])
        pc = np.concatenate([pc, pc + 1])
    room = np.cumsum(inst.capacities)
    return sum(int((1 << pc[dem <= room[k]]).sum()) for k in range(1, len(room)))


def rate(args):
    ctx = Context(0)
    gathers = ctx.probe_l2_gather()
    print(f"probe_l2_gather: {gathers / 1e9:.1f} G gathers/s = {gathers / 2e9:.1f} G steps/s at "
          f"two gathers per step", flush=True)
    for n in args.sizes:
        for K in args.fleets:
            inst = synth.cvrp(n, K, seed=n, slack=1.2)
            for name, obj in (("sum", OBJ_SUM), ("max", OBJ_MAX)):
                ctx.set_instance(CVRP, inst.durations, inst.demand, inst.capacities,
                                 inst.start_times, objective=obj)
                ref = ctx.vrp_sp(n)                  # warm-up (and the allocator's first block)
                ms = []
                for _ in range(args.repeats):
                    t, out = timed(lambda: ctx.vrp_sp(n))
                    assert out == ref
                    ms.append(t)
                med = float(np.median(ms))
                sps = 3.0 ** n * K / (med * 1e-3)    # the recurrence's steps
                run = launched_steps(inst, n)
                print(f"n={n:2d} K={K} {name}  median {med:10.3f} ms  (min {min(ms):.3f}, max "
                      f"{max(ms):.3f}, {len(ms)} runs)  {sps / 1e9:8.2f} G steps/s  launched "
                      f"{run / 3.0 ** n / K:5.3f} of them: {run / (med * 1e-3) / 1e9:7.2f} G/s, "
                      f"{2 * run / (med * 1e-3) / gathers:6.3f} of the L2-gather probe  "
                      f"unvisited {ref[0] >> 56} primary {ref[0] >> 28 & (2**28 - 1)}", flush=True)
    ctx.close()


def gap(args):
    for seed in range(3):
        inst = synth.cvrp(16, 4, seed=seed, slack=1.2)
        D = inst.durations[0].tolist()
        locs = [{"id": i, "demand": int(d)} for i, d in enumerate(inst.demand)]
        caps, starts = inst.capacities.tolist(), inst.start_times.tolist()
        for objective, field in (("sum", "durationSum"), ("max", "durationMax")):
            opt = solver.solve_vrp("sp", D, locs, caps, starts, objective=objective,
                                   with_unvisited=True)
            row = [f"cvrp(16, 4) seed {seed} {objective}: optimum {opt[field]} "
                   f"(unvisited {len(opt['unvisited'])})"]
            for algo in ("sa", "ga", "aco"):
                h = solver.solve_vrp(algo, D, locs, caps, starts, objective=objective, seed=seed,
                                     time_limit=args.limit, with_unvisited=True)
                row.append(f"{algo} {h[field]} (+{100.0 * (h[field] - opt[field]) / opt[field]:.2f} %"
                           + (f", {len(h['unvisited'])} unvisited)" if h["unvisited"] else ")"))
            print("  ".join(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gap", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    ap.add_argument("--sizes", type=ints, default=[8, 10, 13, 16, 18, 20])
    ap.add_argument("--fleets", type=ints, default=[2, 4, 8])
    ap.add_argument("--limit", type=float, default=2.0)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    (gap if a.gap else rate)(a)
