#!/usr/bin/env python3
"""Latency and rate of the delta-priced local search over plain separator tours
(spec A28) by its second mapping, vrpms_vrp_batch_lsf_spread (DESIGN.md §4.3x:
a request's starts spread over G workgroups, 256 threads per descent), against
vrpms_vrp_batch_lsf (one workgroup per request, four wavefronts on four starts)
on the same instances in the same run.  The instances are
tools/batch_vrp_lsr_rate.py's at H = 1; every launch is timed
with device events, one untimed launch and then `--repeats` timed ones,
reported as best, median and worst.  Before anything of a table is timed, the
outputs of the two mappings are compared with torch.equal.

  latency     R = 1 per shape, S = `--starts`: vrp_batch_lsf against G = 1 and
              G = S.  The bar: G = S at its worst launch, the selection
              included, lies below vrp_batch_lsf's best divided by 16.  e, how
              many times faster a 256-thread descent runs than one wavefront's,
              is 4 T_lsf / T_G=1.  Then the selection launch's share: the whole
              call at S = G = 1 and rounds = 0, which stages the request twice,
              builds one start and selects it.
  auto        R = 1, 16, 256, 1024 at `--auto-shape`: the policy of
              solver.batch_lsf_spread, G = min(S, max(1, f CUs // R)), at the
              factors f = 1..16 against vrp_batch_lsf.
  throughput  R = `--requests` per `--throughput-shapes`: G = 1, the 256-thread
              descent with one workgroup per request, against vrp_batch_lsf
              (`--throughput-repeats` timed launches).
  end to end  solver.solve_vrp("lsf") on one request, spread None and "auto",
              wall clock, five calls after two untimed.

  --shapes n:K,...             the latency shapes, default 50:8,200:8
  --auto-shape n:K             default 50:8 ("" skips)
  --throughput-shapes n:K,...  default 20:4,50:8
  --starts S                   descents per request (default 64)
  --rounds C                   applied moves a descent may take (default 1000)
  --repeats M                  timed launches (default 5)
  --requests R                 requests of the throughput launches (default 10000; 0 skips)
  --throughput-repeats M       timed throughput launches (default 5)
  --lib PATH                   an A/B build's libvrpms.so (tools/ab_build.py)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import _lib, solver  # noqa: E402
from vrpms_amd.core import (OBJ_SUM, Context, vrp_batch_lsf_lds,  # noqa: E402
                            vrp_batch_lsf_spread_lds)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="50:8,200:8")
ap.add_argument("--auto-shape", default="50:8")
ap.add_argument("--throughput-shapes", default="20:4,50:8")
ap.add_argument("--starts", type=int, default=64)
ap.add_argument("--rounds", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--requests", type=int, default=10000)
ap.add_argument("--throughput-repeats", type=int, default=5)
ap.add_argument("--lib", default=None, help="an A/B build (tools/ab_build.py) instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.load(args.lib)
S, ROUNDS, SEED = args.starts, args.rounds, 1
LDS = 160 * 1024
AUTO_R = (1, 16, 256, 1024)

ctx = Context(0)


def instances(n, K, count, seed):
    """tools/batch_vrp_lsr_rate.py's family at H = 1."""
    N = n + 1
    rng = np.random.default_rng(seed)
    mats = rng.integers(3, 321, size=(count, 1, N, N), dtype=np.int32)
    mats[:, :, np.arange(N), np.arange(N)] = 0            # every other entry is positive
    dem = rng.integers(1, 10, size=(count, N), dtype=np.int64)
    dem[:, 0] = 0
    share = (dem.sum(axis=1) * 12 + 10 * K - 1) // (10 * K)
    caps = np.maximum(share[:, None] + np.arange(K)[None, :] - (K - 1) // 2, 0)
    starts = rng.integers(0, 1440, size=(count, K), dtype=np.int64)
    return mats, dem, caps, starts


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


def lsf(bufs, s, rounds=None, repeats=None):
    return timed(lambda: ctx.vrp_batch_lsf(*bufs, OBJ_SUM, s, ROUNDS if rounds is None else rounds, SEED,
                                           wide=False), repeats or args.repeats)


def spread(bufs, s, G, rounds=None, repeats=None):
    return timed(lambda: ctx.vrp_batch_lsf_spread(*bufs, OBJ_SUM, s, ROUNDS if rounds is None else rounds,
                                                  SEED, G, wide=False), repeats or args.repeats)


def once(bufs, s, G=None):
    """One launch of either mapping, for the comparison before a table is timed."""
    if G is None:
        return ctx.vrp_batch_lsf(*bufs, OBJ_SUM, s, ROUNDS, SEED, wide=False)
    return ctx.vrp_batch_lsf_spread(*bufs, OBJ_SUM, s, ROUNDS, SEED, G, wide=False)


def device(arrays, count):
    return [torch.tensor(a[:count], dtype=torch.int32, device=ctx.dev) for a in arrays]


def parse(text):
    return [tuple(int(x) for x in shape.split(":")) for shape in text.split(",") if shape]


data = {}


def family(n, K, count):
    """At least `count` instances of the shape; drawn again, and so other
    requests, when a later table needs more than the earlier ones did."""
    if (n, K) not in data or len(data[(n, K)][0]) < count:
        data[(n, K)] = instances(n, K, count, 1000 * n + K + 1)
    return data[(n, K)]


def inside(n, K):
    if vrp_batch_lsf_lds(n + 1, K, 1, False) <= LDS:
        return True
    print(f"n={n} K={K}: outside the {LDS} B domain: not measured")
    return False


print(f"# {torch.cuda.get_device_name(0)}, {ctx.cus} CUs; at most {ROUNDS} rounds a descent, objective "
      f"sum, static matrices, {args.repeats} timed launches after one untimed")
print(f"# latency: R = 1, S = {S}; vrp_batch_lsf against vrp_batch_lsf_spread at G = 1 and G = {S}; "
      f"the bar: G = {S}'s worst launch < vrp_batch_lsf's best / 16")
for n, K in parse(args.shapes):
    if not inside(n, K):
        continue
    N = n + 1
    one = device(family(n, K, 1), 1)
    ref = once(one, S)
    assert same(ref, once(one, S, 1)) and same(ref, once(one, S, S)), f"n={n} K={K}: the rows differ"
    old, ref = lsf(one, S)
    g1, out1 = spread(one, S, 1)
    gs, outs = spread(one, S, S)
    assert same(ref, out1) and same(ref, outs)
    bar = min(old) / 16.0
    print(f"n={n} K={K}: lds {vrp_batch_lsf_lds(N, K, 1, False)} B (vrp_batch_lsf), "
          f"{vrp_batch_lsf_spread_lds(N, K, 1, False)} B (spread); identical rows at G = 1 and G = {S}; "
          f"capped {int(ref[4][0, 1])}")
    print(f"  vrp_batch_lsf      {fmt(old)}")
    print(f"  spread G = 1       {fmt(g1)}   e = 4 T_lsf / T = {4 * min(old) / min(g1):.2f}")
    print(f"  spread G = {S:<4}    {fmt(gs)}   best to worst {min(old) / max(gs):.1f}x (best to best "
          f"{min(old) / min(gs):.1f}x); bar: worst {max(gs):.3f} ms < best / 16 = {bar:.3f} ms: "
          f"{'PASS' if max(gs) < bar else 'FAIL'}", flush=True)
    ms, _ = spread(one, 1, 1, rounds=0)
    print(f"  S = G = 1, rounds = 0 (two stagings, one start, the selection) {fmt(ms)}: "
          f"{min(ms) / min(gs):.1%} of the G = {S} call", flush=True)

for n, K in parse(args.auto_shape):
    if not inside(n, K):
        continue
    print(f"# auto: n={n} K={K}, S = {S}: G = min(S, max(1, f CUs // R)) for f = 1..16 against "
          f"vrp_batch_lsf (best ms, and vrp_batch_lsf's best over it); solver.batch_lsf_spread gives G = " +
          ", ".join(str(solver.batch_lsf_spread(R, S, ctx.cus)) for R in AUTO_R) +
          " at R = " + ", ".join(str(R) for R in AUTO_R))
    for R in AUTO_R:
        bufs = device(family(n, K, max(AUTO_R)), R)
        ref = once(bufs, S)
        Gs = {}
        for f in range(1, 17):
            Gs.setdefault(min(S, max(1, f * ctx.cus // R)), f)
        for G in Gs:
            assert same(ref, once(bufs, S, G)), f"R={R} G={G}: the rows differ"
        old, _ = lsf(bufs, S)
        line = f"  R = {R:<5} vrp_batch_lsf {fmt(old)};"
        for G, f in Gs.items():
            ms, _ = spread(bufs, S, G)
            line += f"  f = {f}: G = {G} {min(ms):.3f} ({min(old) / min(ms):.2f}x)"
        print(line, flush=True)
        del bufs

if args.requests:
    R = args.requests
    print(f"# throughput: R = {R}, S = {S}: spread G = 1 (256 threads on one descent) against "
          f"vrp_batch_lsf, {args.throughput_repeats} timed launches after one untimed")
    for n, K in parse(args.throughput_shapes):
        if not inside(n, K):
            continue
        bufs = device(family(n, K, R), R)
        ref = once(bufs, S)
        assert same(ref, once(bufs, S, 1)), f"n={n} K={K}: the rows differ"
        old, _ = lsf(bufs, S, repeats=args.throughput_repeats)
        ms, _ = spread(bufs, S, 1, repeats=args.throughput_repeats)
        print(f"  n={n} K={K}: vrp_batch_lsf {fmt(old)} -> {R / (min(old) * 1e-3):10,.0f} req/s;  "
              f"G = 1 {fmt(ms)} -> {R / (min(ms) * 1e-3):10,.0f} req/s: {min(ms) / min(old):.2f}x the time",
              flush=True)
        del bufs

print("# end to end: solver.solve_vrp('lsf') on one request, wall clock, five calls after two untimed")
for n, K in parse(args.shapes):
    if (n, K) not in data:
        continue
    mats, dem, caps, starts = data[(n, K)]
    req = (mats[0, 0], [{"id": i, "demand": int(d)} for i, d in enumerate(dem[0])], caps[0], starts[0])
    res = {}
    for name in (None, "auto"):
        kw = dict(starts=S, rounds=ROUNDS, seed=SEED, spread=name)
        for _ in range(2):
            res[name] = solver.solve_vrp("lsf", *req, **kw)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            solver.solve_vrp("lsf", *req, **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"  n={n} K={K} spread={name!s:5}: best {min(ts):9.3f} ms  median "
              f"{statistics.median(ts):9.3f}  worst {max(ts):9.3f}", flush=True)
    assert res[None] == res["auto"]
ctx.close()
