#!/usr/bin/env python3
"""Batched exact TSP rate (spec A18): for n = 2..12 customers and R = 10,000
random symmetric matrices, requests/s of one vrpms_tsp_batch_dp launch
(tsp_batch_dp_kernel), best of 3 timed with device events after a warm-up
launch; beside it the single-request path, set_instance + runners.held_karp
looped over 64 of the same requests (wall clock, it synchronises per request),
per request.  The two must agree on those 64 (key and tour).

  --teams 16,32,...   scan these team sizes T (threads per request) instead of
                      the library's n -> T table; a T whose 256 / T tables do
                      not fit the LDS is reported as such
  --sizes 8,9,...     customers n to run (default 2..12)
  --requests R        requests per launch (default 10000)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import runners, synth  # noqa: E402
from vrpms_amd._lib import VrpmsError  # noqa: E402
from vrpms_amd.core import TSP, Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--teams", default="")
ap.add_argument("--sizes", default=",".join(str(n) for n in range(2, 13)))
ap.add_argument("--requests", type=int, default=10000)
ap.add_argument("--single", type=int, default=64, help="requests of the single-request loop")
args = ap.parse_args()
teams = [int(t) for t in args.teams.split(",") if t] or [0]
R = args.requests

ctx = Context(0)


def batched_ms(M):
    """Best of 3 launches by device events; the first launch is not timed."""
    ctx.tsp_batch_dp(M)
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = ctx.tsp_batch_dp(M)
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best, out


print(f"# R = {R} random symmetric matrices per launch; single-request loop over {args.single}")
print("# n  T  batched_ms  batched_req_per_s  single_us_per_req  speedup  parity")
for n in [int(x) for x in args.sizes.split(",")]:
    N = n + 1
    rng = np.random.default_rng(n)
    mats = np.stack([synth.random_symmetric(N, rng) for _ in range(R)])
    M = torch.tensor(mats, dtype=torch.int32, device=ctx.dev)
    # the single-request path on the first requests (two untimed first)
    S = min(args.single, R)
    single = []
    for x in range(-2, S):
        if x == 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        ctx.set_instance(TSP, mats[max(x, 0)], start_times=(0,))
        r = runners.held_karp(ctx, n)
        if x >= 0:
            single.append(r)
    single_us = (time.perf_counter() - t0) / S * 1e6
    for T in teams:
        ctx.set_batch_dp_team(T)
        try:
            ms, (tours, keys) = batched_ms(M)
        except VrpmsError as e:
            print(f"{n:2d} {T:3d}  does not fit: {e}", flush=True)
            continue
        got = list(zip([int(k) & (2**64 - 1) for k in keys[:S].cpu().tolist()],
                       tours[:S].cpu().tolist()))
        ok = got == [(k, t) for k, t in single]
        rate = R / (ms * 1e-3)
        print(f"{n:2d} {T if T else 'auto':>4}  {ms:9.4f}  {rate:14,.0f}  {single_us:10.1f}  "
              f"{single_us * 1e-6 * rate:9.1f}x  {'ok' if ok else 'MISMATCH'}", flush=True)
    ctx.set_batch_dp_team(0)
ctx.close()
