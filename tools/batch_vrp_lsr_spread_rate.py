#!/usr/bin/env python3
"""Latency and rate of the local search over separator tours (spec A26) by its
second mapping, vrpms_vrp_batch_lsr_spread (a request's starts
spread over G workgroups, 256 threads per descent), against
vrpms_vrp_batch_lsr (one workgroup per request, four wavefronts on four starts)
on the same instances in the same run.  The instances are
tools/batch_vrp_lsr_rate.py's; every launch is timed with device events, one
untimed launch and then `--repeats` timed ones, reported as best, median and
worst.  The outputs of the two mappings are compared with torch.equal in every
row of every table.

  latency     R = 1 per shape, S = `--starts`: vrp_batch_lsr against G = 1 and
              G = S.  The bar: G = S at its worst launch is at least 16 times
              faster than vrp_batch_lsr at its best, less the run's own spread.
              e, how many times faster a 256-thread descent runs than one
              wavefront's, is that factor over 16 (and 4 T_lsr / T_G=1).  Then
              S = 256 at G = 16 and G = 256, and the selection launch's share:
              the whole call at S = G = 1 and rounds = 0, which stages the
              request twice, builds one start and selects it.
  auto        R = 1, 16, 64, 256, 1024 at the first shape: the policy of
              solver.batch_lsr_spread, G = min(S, max(1, f CUs // R)), at the
              factors f = 1, 2, 4, 8 and 16 against vrp_batch_lsr.
  throughput  R = `--requests` per shape: G = 1, the 256-thread descent with
              one workgroup per request, against vrp_batch_lsr
              (`--throughput-repeats` timed launches).
  end to end  solver.solve_vrp("lsr") on one request, spread None and "auto",
              wall clock, five calls after two untimed.

  --shapes n:K:H,...       default 20:4:24,50:8:1,50:8:24
  --starts S               descents per request (default 64)
  --rounds C               applied moves a descent may take (default 1000)
  --repeats M              timed launches (default 5)
  --requests R             requests of the throughput launches (default 10000; 0 skips)
  --throughput-repeats M   timed throughput launches (default 5)
  --lib PATH               an A/B build's libvrpms.so (tools/ab_build.py)
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
from vrpms_amd.core import (OBJ_SUM, Context, vrp_batch_lsr_lds,  # noqa: E402
                            vrp_batch_lsr_spread_lds)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="20:4:24,50:8:1,50:8:24")
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

AUTO_R = (1, 16, 64, 256, 1024)

ctx = Context(0)


def instances(n, K, H, count, seed):
    N = n + 1
    rng = np.random.default_rng(seed)
    mats = rng.integers(3, 321, size=(count, H, N, N), dtype=np.int32)
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


def lsr(bufs, s, rounds=None, repeats=None):
    return timed(lambda: ctx.vrp_batch_lsr(*bufs, OBJ_SUM, s, ROUNDS if rounds is None else rounds, SEED,
                                           wide=False), repeats or args.repeats)


def spread(bufs, s, G, rounds=None, repeats=None):
    return timed(lambda: ctx.vrp_batch_lsr_spread(*bufs, OBJ_SUM, s, ROUNDS if rounds is None else rounds,
                                                  SEED, G, wide=False), repeats or args.repeats)


def device(arrays, count):
    return [torch.tensor(a[:count], dtype=torch.int32, device=ctx.dev) for a in arrays]


shapes = [tuple(int(x) for x in shape.split(":")) for shape in args.shapes.split(",")]
print(f"# {torch.cuda.get_device_name(0)}, {ctx.cus} CUs; at most {ROUNDS} rounds a descent, objective "
      f"sum, {args.repeats} timed launches after one untimed")
print(f"# latency: R = 1, S = {S}; vrp_batch_lsr against vrp_batch_lsr_spread at G = 1 and G = {S}")
data = {}
for n, K, H in shapes:
    N = n + 1
    if vrp_batch_lsr_lds(N, K, H, False) > LDS:
        print(f"n={n} K={K} H={H}: outside the {LDS} B domain: not measured")
        continue
    data[(n, K, H)] = arrays = instances(n, K, H, max(args.requests, 1024), 1000 * n + K + H)
    one = device(arrays, 1)
    old, ref = lsr(one, S)
    g1, out1 = spread(one, S, 1)
    gs, outs = spread(one, S, S)
    assert same(ref, out1) and same(ref, outs)
    noise = max(max(old) - min(old), max(gs) - min(gs))
    factor = min(old) / max(gs)
    bar = 16.0 * (1.0 - noise / min(old))
    print(f"n={n} K={K} H={H}: lds {vrp_batch_lsr_lds(N, K, H, False)} B (vrp_batch_lsr), "
          f"{vrp_batch_lsr_spread_lds(N, K, H, False)} B (spread); capped {int(ref[4][0, 1])}")
    print(f"  vrp_batch_lsr      {fmt(old)}")
    print(f"  spread G = 1       {fmt(g1)}   e = 4 T_lsr / T = {4 * min(old) / min(g1):.2f}")
    print(f"  spread G = {S:<4}    {fmt(gs)}   best to worst {factor:.1f}x (best to best "
          f"{min(old) / min(gs):.1f}x), e = {min(old) / min(gs) / 16:.2f}; bar 16x less the spread "
          f"{noise:.3f} ms = {bar:.1f}x: {'PASS' if factor >= bar else 'FAIL'}", flush=True)
    old, ref = lsr(one, 256)
    for G in (16, 256):
        ms, out = spread(one, 256, G)
        assert same(ref, out)
        print(f"  S = 256: vrp_batch_lsr {fmt(old)};  G = {G:<3} {fmt(ms)}  {min(old) / min(ms):.1f}x",
              flush=True)
    ms, _ = spread(one, 1, 1, rounds=0)
    print(f"  S = G = 1, rounds = 0 (two stagings, one start, the selection) {fmt(ms)}", flush=True)

if data:
    n, K, H = next(iter(data))
    print(f"# auto: n={n} K={K} H={H}, S = {S}: G = min(S, max(1, f CUs // R)) for f = 1, 2, 4, 8, 16 "
          f"against vrp_batch_lsr (best ms, and vrp_batch_lsr's best over it); solver.batch_lsr_spread "
          f"gives G = " + ", ".join(str(solver.batch_lsr_spread(R, S, ctx.cus)) for R in AUTO_R) +
          f" at R = " + ", ".join(str(R) for R in AUTO_R))
    for R in AUTO_R:
        bufs = device(data[(n, K, H)], R)
        old, ref = lsr(bufs, S)
        line = f"  R = {R:<5} vrp_batch_lsr {fmt(old)};"
        done = set()
        for f in (1, 2, 4, 8, 16):
            G = min(S, max(1, f * ctx.cus // R))
            if G in done:
                continue
            done.add(G)
            ms, out = spread(bufs, S, G)
            assert same(ref, out)
            line += f"  f = {f}: G = {G} {min(ms):.3f} ({min(old) / min(ms):.2f}x)"
        print(line, flush=True)

if args.requests:
    R = args.requests
    print(f"# throughput: R = {R}, S = {S}: spread G = 1 (256 threads on one descent) against "
          f"vrp_batch_lsr, {args.throughput_repeats} timed launches after one untimed")
    for (n, K, H), arrays in data.items():
        bufs = device(arrays, R)
        old, ref = lsr(bufs, S, repeats=args.throughput_repeats)
        ms, out = spread(bufs, S, 1, repeats=args.throughput_repeats)
        assert same(ref, out)
        print(f"  n={n} K={K} H={H}: vrp_batch_lsr {fmt(old)} -> {R / (min(old) * 1e-3):10,.0f} req/s;  "
              f"G = 1 {fmt(ms)} -> {R / (min(ms) * 1e-3):10,.0f} req/s: {min(ms) / min(old):.2f}x the time",
              flush=True)
        del bufs

print("# end to end: solver.solve_vrp('lsr') on one request, wall clock, five calls after two untimed")
for (n, K, H), (mats, dem, caps, starts) in data.items():
    req = ((mats[0] if H > 1 else mats[0, 0]), [{"id": i, "demand": int(d)} for i, d in enumerate(dem[0])],
           caps[0], starts[0])
    res = {}
    for name in (None, "auto"):
        kw = dict(starts=S, rounds=ROUNDS, seed=SEED, spread=name)
        for _ in range(2):
            res[name] = solver.solve_vrp("lsr", *req, **kw)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            solver.solve_vrp("lsr", *req, **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"  n={n} K={K} H={H} spread={name!s:5}: best {min(ts):9.3f} ms  median "
              f"{statistics.median(ts):9.3f}  worst {max(ts):9.3f}", flush=True)
    assert res[None] == res["auto"]
ctx.close()
