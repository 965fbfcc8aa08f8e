#!/usr/bin/env python3
"""Batched exact time-dependent TSP rate (spec A20): for n = 2..11 customers,
row widths W and R = 10,000 random hour-indexed matrices, requests/s of one
vrpms_tsp_batch_tdp launch (tsp_batch_tdp_kernel), best of 3 timed with device
events after an untimed launch; beside it the single-request path,
set_instance + runners.time_expanded looped over 64 of the same requests (wall
clock, it synchronises per request), per request.  The two must agree on those
64 (key and tour).  These are kernel rates: the [R][24][N][N] upload is outside
the timed region.

A request of width W leaves at a whole hour with horizon 60 W - 1, its entries
uniform in 1..max(2, 120 W / (n + 1)): tours of about 60 W minutes, so the rows
are populated up to the clip and about half of the tours fall under it.

  --teams 16,32,...   scan these team sizes T (threads per request) instead of
                      the library's n -> T table; a T whose 256 / T requests do
                      not fit the LDS is reported as such
  --sizes 8,9,...     customers n to run (default 2..11)
  --words 1,mid,max   row widths per n: numbers, `max` (the largest W that fits
                      the LDS at that n, at most 512) or `mid` (half of it)
  --requests R        requests per launch (default 10000)

VRPMS_LIB=path/libvrpms.so runs an A/B build (tools/ab_build.py OUT
-DVRPMS_BATCH_TDP_FILL=1 tsp_batch_tdp.hip)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import _lib, runners  # noqa: E402
from vrpms_amd._lib import VrpmsError  # noqa: E402

if os.environ.get("VRPMS_LIB"):
    _lib.load(os.environ["VRPMS_LIB"])

from vrpms_amd.core import TSP, Context, tsp_batch_tdp_lds  # noqa: E402

LDS_BYTES = 160 * 1024
NONE = 2**64 - 1

ap = argparse.ArgumentParser()
ap.add_argument("--teams", default="")
ap.add_argument("--sizes", default=",".join(str(n) for n in range(2, 12)))
ap.add_argument("--words", default="1,mid,max")
ap.add_argument("--requests", type=int, default=10000)
ap.add_argument("--single", type=int, default=64, help="requests of the single-request loop")
args = ap.parse_args()
teams = [int(t) for t in args.teams.split(",") if t] or [0]
R = args.requests

ctx = Context(0)


def max_words(n):
    """The largest W <= 512 whose request fits the LDS alone."""
    lo, hi = 1, 512
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if tsp_batch_tdp_lds(n, 24, mid) <= LDS_BYTES:
            lo = mid
        else:
            hi = mid - 1
    return lo


def batched_ms(M, starts, horizons, W, T):
    """Best of 3 launches by device events; the first launch is not timed."""
    ctx.tsp_batch_tdp(M, starts, horizons, W, T)
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = ctx.tsp_batch_tdp(M, starts, horizons, W, T)
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best, out


print(f"# R = {R} random hour-indexed matrices per launch; single-request loop over {args.single}")
print("# kernel rates: the upload of the matrices is not timed")
print("# n   W     T  lds_bytes  batched_ms  batched_req_per_s  single_us_per_req  speedup  "
      "feasible  parity")
for n in [int(x) for x in args.sizes.split(",")]:
    N = n + 1
    wmax = max_words(n)
    widths = []
    for w in args.words.split(","):
        W = wmax if w == "max" else max(1, wmax // 2) if w == "mid" else int(w)
        if W not in widths:
            widths.append(W)
    for W in widths:
        rng = np.random.default_rng(1000 * n + W)
        hi = max(2, 120 * W // (n + 1))
        mats = rng.integers(1, hi + 1, size=(R, 24, N, N), dtype=np.int32)
        mats[:, :, np.arange(N), np.arange(N)] = 0
        starts = 60 * (np.arange(R, dtype=np.int64) % 30)
        horizons = np.full(R, 60 * W - 1, dtype=np.int64)
        M = torch.from_numpy(mats).to(ctx.dev)
        d_st = torch.from_numpy(starts.astype(np.int32)).to(ctx.dev)
        d_hz = torch.from_numpy(horizons.astype(np.int32)).to(ctx.dev)
        # the single-request path on the first requests (two untimed first)
        S = min(args.single, R)
        single = []
        for x in range(-2, S):
            if x == 0:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            y = max(x, 0)
            ctx.set_instance(TSP, mats[y], start_times=(int(starts[y]),))
            try:
                r = runners.time_expanded(ctx, n, mats[y], int(starts[y]), int(horizons[y]))
            except ValueError:          # no tour within the horizon
                r = (NONE, [0] * n)
            if x >= 0:
                single.append(r)
        single_us = (time.perf_counter() - t0) / S * 1e6
        for T in teams:
            try:
                lds = tsp_batch_tdp_lds(n, 24, W, T)
                ms, (tours, keys) = batched_ms(M, d_st, d_hz, W, T)
            except VrpmsError as e:
                print(f"{n:2d} {W:3d} {T:5d}  does not fit: {e}", flush=True)
                continue
            got = list(zip([int(k) & NONE for k in keys[:S].cpu().tolist()],
                           tours[:S].cpu().tolist()))
            ok = got == [(k, t) for k, t in single]
            feasible = int((keys != -1).sum().item())
            rate = R / (ms * 1e-3)
            print(f"{n:2d} {W:3d} {T if T else 'auto':>5}  {lds:9d}  {ms:10.4f}  {rate:17,.0f}  "
                  f"{single_us:17.1f}  {single_us * 1e-6 * rate:7.1f}x  {feasible:8d}  "
                  f"{'ok' if ok else 'MISMATCH'}", flush=True)
        del M
ctx.close()
