#!/usr/bin/env python3
"""Batched exact time-dependent VRP rate (spec A21): over cells (n customers,
K vehicles, G distinct start times, row width W) and R = 10,000 random
hour-indexed instances, requests/s of one vrpms_vrp_batch_tdsp launch
(vrp_batch_tdsp_kernel), best of 3 timed with device events after an untimed
launch; beside it the unchanged single-request path, set_instance +
runners.td_set_partition looped over 64 of the same requests (wall clock, it
synchronises per request), per request.  The two must agree on those 64 (key
and tour).  These are kernel rates: the upload of the matrices, demands,
capacities, start times and horizons is outside the timed region.

A request of width W has vehicle k leaving at a whole hour, start time number
k % G of its G distinct ones, horizon 60 W - 1, entries uniform in
1..max(2, 120 W / (n / K + 1)) -- routes of about n / K customers take about
60 W minutes, so the rows are populated up to the clip -- demands in 1..3 and
K capacities that together carry them with one unit to spare each.

  --teams 16,32,...   scan these team sizes T (threads per request) besides
                      the library's auto team; a T whose 256 / T requests do
                      not fit the LDS is reported as such
  --sizes 8,9,...     customers n to run (default 2..11)
  --fleets 2:1,3:3    K:G pairs (default 2:1,3:3)
  --words 1,mid,max   row widths per cell: numbers, `max` (the largest W that
                      fits the LDS in that cell, at most 512) or `mid` (half)
  --requests R        requests per launch (default 10000)
  --objective sum|max

VRPMS_LIB=path/libvrpms.so runs an A/B build (tools/ab_build.py OUT
-DVRPMS_BATCH_TDP_FILL=1 vrp_batch_tdsp.hip)."""
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

from vrpms_amd.core import CVRP, OBJ_MAX, OBJ_SUM, Context, vrp_batch_tdsp_lds  # noqa: E402

LDS_BYTES = 160 * 1024
NONE = 2**64 - 1

ap = argparse.ArgumentParser()
ap.add_argument("--teams", default="")
ap.add_argument("--sizes", default=",".join(str(n) for n in range(2, 12)))
ap.add_argument("--fleets", default="2:1,3:3")
ap.add_argument("--words", default="1,mid,max")
ap.add_argument("--requests", type=int, default=10000)
ap.add_argument("--single", type=int, default=64, help="requests of the single-request loop")
ap.add_argument("--objective", default="sum", choices=("sum", "max"))
args = ap.parse_args()
teams = [0] + [int(t) for t in args.teams.split(",") if t]
R = args.requests
OBJ = OBJ_MAX if args.objective == "max" else OBJ_SUM

ctx = Context(0)


def max_words(n, K, G):
    """The largest W <= 512 whose request fits the LDS alone (0: none)."""
    lo, hi = 0, 512
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if vrp_batch_tdsp_lds(n, K, G, 24, mid) <= LDS_BYTES:
            lo = mid
        else:
            hi = mid - 1
    return lo


def batched_ms(bufs, G, W, T):
    """Best of 3 launches by device events; the first launch is not timed."""
    ctx.vrp_batch_tdsp(*bufs, OBJ, G=G, W=W, team=T)
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = ctx.vrp_batch_tdsp(*bufs, OBJ, G=G, W=W, team=T)
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best, out


print(f"# R = {R} random hour-indexed instances per launch; single-request loop over {args.single}; "
      f"objective {args.objective}")
print("# kernel rates: the upload of the instances is not timed")
print("# n  K  G   W     T  lds_bytes  batched_ms  batched_req_per_s  single_us_per_req  speedup  "
      "all_served  parity")
for n in [int(x) for x in args.sizes.split(",")]:
    N = n + 1
    for K, G in [tuple(int(v) for v in f.split(":")) for f in args.fleets.split(",")]:
        wmax = max_words(n, K, G)
        if not wmax:
            print(f"{n:2d} {K:2d} {G:2d}  no row width fits the LDS", flush=True)
            continue
        widths = []
        for w in args.words.split(","):
            W = wmax if w == "max" else max(1, wmax // 2) if w == "mid" else int(w)
            if W <= wmax and W not in widths:
                widths.append(W)
        for W in widths:
            rng = np.random.default_rng(100000 * n + 1000 * K + 100 * G + W)
            hi = max(2, 120 * W * K // (n + K))
            mats = rng.integers(1, hi + 1, size=(R, 24, N, N), dtype=np.int32)
            mats[:, :, np.arange(N), np.arange(N)] = 0
            dem = rng.integers(1, 4, size=(R, N), dtype=np.int32)
            dem[:, 0] = 0
            caps = np.repeat(((dem.sum(axis=1) + K - 1) // K + 1)[:, None], K, axis=1).astype(np.int32)
            hours = (np.arange(R)[:, None] + 7 * (np.arange(K)[None, :] % G)) % 30
            starts = (60 * hours).astype(np.int32)
            horizons = np.full(R, 60 * W - 1, dtype=np.int32)
            bufs = [torch.from_numpy(a).to(ctx.dev) for a in (mats, dem, caps, starts, horizons)]
            # the single-request path on the first requests (two untimed first)
            S = min(args.single, R)
            single = []
            for x in range(-2, S):
                if x == 0:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                y = max(x, 0)
                ctx.set_instance(CVRP, mats[y], dem[y], caps[y], starts[y], objective=OBJ)
                r = runners.td_set_partition(ctx, n, int(horizons[y]))
                if x >= 0:
                    single.append(r)
            single_us = (time.perf_counter() - t0) / S * 1e6
            for T in teams:
                try:
                    lds = vrp_batch_tdsp_lds(n, K, G, 24, W, T)
                    ms, (tours, keys, _) = batched_ms(bufs, G, W, T)
                except VrpmsError as e:
                    print(f"{n:2d} {K:2d} {G:2d} {W:3d} {T:5d}  does not fit: {e}", flush=True)
                    continue
                got = list(zip([int(k) & NONE for k in keys[:S].cpu().tolist()],
                               tours[:S].cpu().tolist()))
                ok = got == [(k, t) for k, t in single]
                served = int(((keys >> 56) == 0).sum().item())
                rate = R / (ms * 1e-3)
                print(f"{n:2d} {K:2d} {G:2d} {W:3d} {T if T else 'auto':>5}  {lds:9d}  {ms:10.4f}  "
                      f"{rate:17,.0f}  {single_us:17.1f}  {single_us * 1e-6 * rate:7.1f}x  "
                      f"{served:10d}  {'ok' if ok else 'MISMATCH'}", flush=True)
            del bufs
ctx.close()
