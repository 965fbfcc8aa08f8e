#!/usr/bin/env python3
"""Batched exact VRP rate (spec A19): for n = 2..12 customers, K vehicles and
R = 10,000 random instances (symmetric matrix of 3..320, demands 1..9, K
unequal capacities that carry 1.2 times the total demand together),
requests/s of one vrpms_vrp_batch_sp launch (vrp_batch_sp_kernel), best of 3
timed with device events after an untimed launch; beside it the single-request
path, set_instance + runners.set_partition looped over 64 of the same requests
(wall clock, it synchronises per request), per request.  The two must agree on
those 64 (key and tour).  Where K vehicles do not fit the LDS at n, the largest
fleet that does is run and reported.

  --teams 16,32,...   scan these team sizes T (threads per request) instead of
                      the library's auto team; a T whose 256 / T requests do
                      not fit the LDS is reported as such
  --sizes 8,9,...     customers n to run (default 2..12)
  --vehicles K        fleet size (default 3)
  --requests R        requests per launch (default 10000)
  --objective sum|max
  --lib PATH          an A/B build's libvrpms.so (tools/ab_build.py)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import _lib, runners  # noqa: E402
from vrpms_amd._lib import VrpmsError  # noqa: E402
from vrpms_amd.core import CVRP, OBJ_MAX, OBJ_SUM, Context, vrp_batch_sp_lds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--teams", default="")
ap.add_argument("--sizes", default=",".join(str(n) for n in range(2, 13)))
ap.add_argument("--vehicles", type=int, default=3)
ap.add_argument("--requests", type=int, default=10000)
ap.add_argument("--single", type=int, default=64, help="requests of the single-request loop")
ap.add_argument("--objective", default="sum", choices=("sum", "max"))
ap.add_argument("--lib", default=None, help="an A/B build (tools/ab_build.py) instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.load(args.lib)
teams = [int(t) for t in args.teams.split(",") if t] or [0]
R = args.requests
obj = OBJ_MAX if args.objective == "max" else OBJ_SUM

ctx = Context(0)


def batched_ms(M, dm, cp, T):
    """Best of 3 launches by device events; the first launch is not timed."""
    ctx.vrp_batch_sp(M, dm, cp, obj, T)
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = ctx.vrp_batch_sp(M, dm, cp, obj, T)
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best, out


print(f"# R = {R} random instances per launch, objective {args.objective}; single-request loop "
      f"over {args.single}")
print("# n  K  T  lds_bytes  batched_ms  batched_req_per_s  single_us_per_req  speedup  parity")
for n in [int(x) for x in args.sizes.split(",")]:
    N = n + 1
    K = max(k for k in range(1, args.vehicles + 1) if vrp_batch_sp_lds(n, k) <= 160 * 1024)
    rng = np.random.default_rng(n)
    up = np.triu(rng.integers(3, 321, size=(R, N, N), dtype=np.int64), 1)
    mats = up + up.transpose(0, 2, 1)
    dem = rng.integers(1, 10, size=(R, N), dtype=np.int64)
    dem[:, 0] = 0
    share = (dem.sum(axis=1) * 12 + 10 * K - 1) // (10 * K)
    caps = np.maximum(share[:, None] + np.arange(K)[None, :] - (K - 1) // 2, 0)
    M = torch.tensor(mats, dtype=torch.int32, device=ctx.dev)
    dm = torch.tensor(dem, dtype=torch.int32, device=ctx.dev)
    cp = torch.tensor(caps, dtype=torch.int32, device=ctx.dev)
    # the single-request path on the first requests (two untimed first)
    S = min(args.single, R)
    single = []
    for x in range(-2, S):
        if x == 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        i = max(x, 0)
        ctx.set_instance(CVRP, mats[i], dem[i], caps[i], [0] * K, objective=obj)
        r = runners.set_partition(ctx, n)
        if x >= 0:
            single.append(r)
    single_us = (time.perf_counter() - t0) / S * 1e6
    for T in teams:
        lds = vrp_batch_sp_lds(n, K, T)
        try:
            ms, (tours, keys, _) = batched_ms(M, dm, cp, T)
        except VrpmsError as e:
            print(f"{n:2d} {K:2d} {T:3d}  does not fit: {e}", flush=True)
            continue
        got = list(zip([int(k) & (2**64 - 1) for k in keys[:S].cpu().tolist()],
                       tours[:S].cpu().tolist()))
        ok = got == [(k, t) for k, t in single]
        rate = R / (ms * 1e-3)
        print(f"{n:2d} {K:2d} {T if T else 'auto':>4}  {lds:7d}  {ms:9.4f}  {rate:14,.0f}  "
              f"{single_us:10.1f}  {single_us * 1e-6 * rate:9.1f}x  {'ok' if ok else 'MISMATCH'}",
              flush=True)
ctx.close()
