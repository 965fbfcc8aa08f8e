#!/usr/bin/env python3
"""Latency and rate of the TSP local search with Or-opt and delta pricing (spec
A27) by its second mapping, vrpms_tsp_batch_lso_spread (a
request's starts spread over G workgroups, 256 threads per descent), against
vrpms_tsp_batch_lso (one workgroup per request, four wavefronts on four starts)
on the same instances in the same run.  The instances are
tools/batch_tsp_lso_rate.py's; every launch is timed with device events, one
untimed launch and then `--repeats` timed ones, reported as best, median and
worst.  The four outputs of the two mappings are compared with torch.equal in
every row of every table.

  latency     R = 1 per shape, S = `--starts`, moves = `--moves`: tsp_batch_lso
              against G = 1 and G = S.  The bar: G = S at its worst launch is
              at least 16 times faster than tsp_batch_lso at its best, less the
              two spreads (worst - best of each).  e, how many times faster a
              256-thread descent runs than one wavefront's, is that factor
              over 16 (and 4 T_lso / T_G=1).  Then the selection launch's
              share: the whole call at S = G = 1 and rounds = 0, which stages
              the matrix, builds one start and selects it, over G = S's time.
  auto        R = 1, 16, 64, 256, 1024 at the first shape: the policy of
              solver.batch_lso_spread, G = min(S, max(1, f CUs // R)), at the
              factors f = 1, 2, 4, 8 and 16 against tsp_batch_lso.
  throughput  per `--throughput` shape: G = 1, the 256-thread descent with one
              workgroup per request, against tsp_batch_lso.
  end to end  solver.solve_tsp("lso") on one request, spread None and "auto",
              wall clock, five calls after two untimed.

  --shapes n:H,...         latency shapes, default 50:1,200:1,50:24
  --throughput n:H:R,...   default 50:1:10000,20:24:10000,200:1:256 (empty skips)
  --starts S               descents per request (default 64)
  --rounds C               applied moves a descent may take (default 1000)
  --moves M                the mask of enabled move types (default 31)
  --repeats M              timed launches (default 5)
  --lib PATH               an A/B build's libvrpms.so (tools/ab_build.py)

No hardware counters are read and nothing is traced."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import _lib, solver  # noqa: E402
from vrpms_amd.core import Context, tsp_batch_lso_lds, tsp_batch_lso_spread_lds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="50:1,200:1,50:24")
ap.add_argument("--throughput", default="50:1:10000,20:24:10000,200:1:256")
ap.add_argument("--starts", type=int, default=64)
ap.add_argument("--rounds", type=int, default=1000)
ap.add_argument("--moves", type=int, default=31)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--lib", default=None, help="an A/B build (tools/ab_build.py) instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.load(args.lib)
S, ROUNDS, MOVES, SEED = args.starts, args.rounds, args.moves, 1
LDS = 160 * 1024

AUTO_R = (1, 16, 64, 256, 1024)
FACTORS = (1, 2, 4, 8, 16)

ctx = Context(0)


def instances(n, H, count, seed):
    """tools/batch_tsp_lso_rate.py's family: entries 3..320, start times 0..1439."""
    N = n + 1
    rng = np.random.default_rng(seed)
    mats = rng.integers(3, 321, size=(count, H, N, N), dtype=np.int32)
    mats[:, :, np.arange(N), np.arange(N)] = 0            # every other entry is positive
    starts = rng.integers(0, 1440, size=count, dtype=np.int64)
    return mats, starts


def timed(launch, repeats):
    """One untimed launch, then `repeats` timed by device events -> ([ms], last result)."""
    launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = launch()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms, out


def fmt(ms):
    return f"best {min(ms):10.3f} ms  median {statistics.median(ms):10.3f}  worst {max(ms):10.3f}"


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def lso(bufs, s, rounds=None):
    return timed(lambda: ctx.tsp_batch_lso(*bufs, s, ROUNDS if rounds is None else rounds, MOVES, SEED,
                                           wide=False), args.repeats)


def spread(bufs, s, G, rounds=None):
    return timed(lambda: ctx.tsp_batch_lso_spread(*bufs, s, ROUNDS if rounds is None else rounds, MOVES,
                                                  SEED, G, wide=False), args.repeats)


def device(arrays, count):
    return [torch.tensor(a[:count], dtype=torch.int32, device=ctx.dev) for a in arrays]


shapes = [tuple(int(x) for x in shape.split(":")) for shape in args.shapes.split(",") if shape]
print(f"# {torch.cuda.get_device_name(0)}, {ctx.cus} CUs; at most {ROUNDS} rounds a descent, moves = "
      f"{MOVES}, {args.repeats} timed launches after one untimed, device events")
print(f"# latency: R = 1, S = {S}; tsp_batch_lso against tsp_batch_lso_spread at G = 1 and G = {S}")
data = {}
for n, H in shapes:
    N = n + 1
    if tsp_batch_lso_lds(N, H, False) > LDS:
        print(f"n={n} H={H}: outside the {LDS} B domain: not measured")
        continue
    # the auto table takes its requests from the first shape
    data[(n, H)] = arrays = instances(n, H, 1 if data else max(AUTO_R), 1000 * n + H)
    one = device(arrays, 1)
    old, ref = lso(one, S)
    g1, out1 = spread(one, S, 1)
    gs, outs = spread(one, S, S)
    assert same(ref, out1) and same(ref, outs)
    noise = (max(old) - min(old)) + (max(gs) - min(gs))
    factor = min(old) / max(gs)
    bar = 16.0 * (1.0 - noise / min(old))
    print(f"n={n} H={H}: lds {tsp_batch_lso_lds(N, H, False)} B (tsp_batch_lso), "
          f"{tsp_batch_lso_spread_lds(N, H, False)} B (spread); capped {int(ref[3][0, 1])}")
    print(f"  tsp_batch_lso      {fmt(old)}")
    print(f"  spread G = 1       {fmt(g1)}   e = 4 T_lso / T = {4 * min(old) / min(g1):.2f}")
    print(f"  spread G = {S:<4}    {fmt(gs)}   best to worst {factor:.1f}x (best to best "
          f"{min(old) / min(gs):.1f}x), e = {factor / 16:.2f}; bar 16x less the spreads "
          f"{noise:.3f} ms = {bar:.1f}x: {'PASS' if factor >= bar else 'FAIL'}", flush=True)
    ms, _ = spread(one, 1, 1, rounds=0)
    print(f"  S = G = 1, rounds = 0 (the staging, one start, the selection) {fmt(ms)}: "
          f"{min(ms) / min(gs):.1%} of G = {S}'s best", flush=True)

if data:
    n, H = next(iter(data))
    print(f"# auto: n={n} H={H}, S = {S}: G = min(S, max(1, f CUs // R)) for f = 1, 2, 4, 8, 16 "
          f"against tsp_batch_lso (best ms, and tsp_batch_lso's best over it); solver.batch_lso_spread "
          f"gives G = " + ", ".join(str(solver.batch_lso_spread(R, S, ctx.cus)) for R in AUTO_R) +
          f" at R = " + ", ".join(str(R) for R in AUTO_R))
    for R in AUTO_R:
        bufs = device(data[(n, H)], R)
        old, ref = lso(bufs, S)
        line = f"  R = {R:<5} tsp_batch_lso {fmt(old)};"
        done = {}
        for f in FACTORS:
            G = min(S, max(1, f * ctx.cus // R))
            if G not in done:
                ms, out = spread(bufs, S, G)
                assert same(ref, out)
                done[G] = min(ms)
            line += f"  f = {f}: G = {G} {done[G]:.3f} ({min(old) / done[G]:.2f}x)"
        print(line, flush=True)

through = [tuple(int(x) for x in shape.split(":")) for shape in args.throughput.split(",") if shape]
if through:
    print(f"# throughput: S = {S}: spread G = 1 (256 threads on one descent) against tsp_batch_lso")
for n, H, R in through:
    bufs = device(instances(n, H, R, 1000 * n + H), R)
    old, ref = lso(bufs, S)
    ms, out = spread(bufs, S, 1)
    assert same(ref, out)
    print(f"  n={n} H={H} R={R}: tsp_batch_lso {fmt(old)} -> {R / (min(old) * 1e-3):10,.0f} req/s;  "
          f"G = 1 {fmt(ms)} -> {R / (min(ms) * 1e-3):10,.0f} req/s: {min(ms) / min(old):.2f}x the time",
          flush=True)
    del bufs

print("# end to end: solver.solve_tsp('lso') on one request, wall clock, five calls after two untimed")
for (n, H), (mats, starts) in data.items():
    req = ((mats[0] if H > 1 else mats[0, 0]), list(range(1, n + 1)), 0, int(starts[0]))
    res = {}
    for name in (None, "auto"):
        kw = dict(starts=S, rounds=ROUNDS, moves=MOVES, seed=SEED, spread=name)
        for _ in range(2):
            res[name] = solver.solve_tsp("lso", *req, **kw)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            solver.solve_tsp("lso", *req, **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"  n={n} H={H} spread={name!s:5}: best {min(ts):9.3f} ms  median "
              f"{statistics.median(ts):9.3f}  worst {max(ts):9.3f}", flush=True)
    assert res[None] == res["auto"]
ctx.close()
