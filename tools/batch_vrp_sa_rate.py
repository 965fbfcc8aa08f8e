#!/usr/bin/env python3
"""Batched VRP annealing rate (spec A22): for each shape (n customers, K
vehicles, H hour slices) and R = 10,000 random instances (entries 3..320,
demands 1..9, K unequal capacities that carry 1.2 times the total demand
together, start times 0..1439), requests/s of one vrpms_vrp_batch_sa launch
(vrp_batch_sa_kernel) of `--steps` steps: an untimed launch, then `--repeats`
launches timed with device events, reported as best, median and worst.  Beside
it

  * the workgroups per CU the shape's LDS bytes leave room for (160 KiB a CU);
  * solver.solve_vrp_sa_batch end to end on the same requests as host tuples
    (compaction, guards, staging, upload, launch, read-back, result dicts;
    wall clock, one run after one untimed run on a tenth of them);
  * what the library offered before for the same work, per request:
    Context.set_instance + 4 first-fit chains of Context.sa_run with the same
    step count and schedule + argmin + decode, looped over 64 of the same
    requests, three runs (wall clock, it synchronises per request), each run's
    time per request.

The batched launch passes when its time per request is below the loop's best
run by more than the loop's own spread (worst run - best run).

  --shapes n:K:H,...  default 20:4:24,50:8:1,50:8:24
  --requests R        requests per launch (default 10000)
  --steps S           SA steps (default 2000)
  --repeats M         timed launches (default 5)
  --gap               also: 1,000 static requests of (n = 10, K = 3) at --steps
                      against solve_vrp_batch("sp")'s optima: the share that
                      reaches the optimum's key and the mean primary gap
  --lib PATH          an A/B build's libvrpms.so (tools/ab_build.py)
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
from vrpms_amd.core import CVRP, OBJ_SUM, Context, vrp_batch_sa_lds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="20:4:24,50:8:1,50:8:24")
ap.add_argument("--requests", type=int, default=10000)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--single", type=int, default=64, help="requests of the single-request loop")
ap.add_argument("--gap", action="store_true")
ap.add_argument("--lib", default=None, help="an A/B build (tools/ab_build.py) instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.load(args.lib)
R, STEPS, SEED = args.requests, args.steps, 1
LDS = 160 * 1024

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


def schedules(mats):
    """solver.batch_sa_schedule per request, vectorised (no entry is negative)."""
    flat = mats.reshape(mats.shape[0], -1)
    mean = flat.sum(axis=1, dtype=np.int64) / np.count_nonzero(flat, axis=1)
    return (1.0 / (0.5 * mean)).astype(np.float32), (0.5 / 0.002) ** (1.0 / max(1, STEPS))


def single_loop(mats, dem, caps, starts, inv_t0, inv_alpha, S):
    """-> seconds per request of one pass over the first S requests."""
    n, K = dem.shape[1] - 1, caps.shape[1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(S):
        ctx.set_instance(CVRP, mats[i], dem[i], caps[i], starts[i], objective=OBJ_SUM)
        cur = ctx.pack_separators(ctx.random_tours(4, n, SEED), K - 1)
        best = cur.clone()
        ck = torch.empty(4, dtype=torch.int64, device=ctx.dev)
        bk = torch.full((4,), -1, dtype=torch.int64, device=ctx.dev)
        ctx.sa_run(cur, ck, best, bk, STEPS, float(inv_t0[i]), inv_alpha, SEED, 0)
        _, w = ctx.argmin(bk)
        ctx.decode(best[w])
    return (time.perf_counter() - t0) / S


print(f"# R = {R} random instances per launch, {STEPS} steps, objective sum, {args.repeats} timed "
      f"launches after one untimed; single-request loop over {args.single}, three runs")
for shape in args.shapes.split(","):
    n, K, H = (int(x) for x in shape.split(":"))
    N = n + 1
    lds = vrp_batch_sa_lds(N, K, H, False)
    mats, dem, caps, starts = instances(n, K, H, R, 1000 * n + K + H)
    inv_t0, inv_alpha = schedules(mats)
    bufs = [torch.tensor(a, dtype=torch.int32, device=ctx.dev) for a in (mats, dem, caps, starts)]
    it = torch.tensor(inv_t0, dtype=torch.float32, device=ctx.dev)

    def launch():
        return ctx.vrp_batch_sa(*bufs, it, OBJ_SUM, STEPS, inv_alpha, SEED, wide=False)

    launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = launch()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    assert not (out[1] == -1).any().item()
    best, med, worst = min(ms), statistics.median(ms), max(ms)
    print(f"n={n} K={K} H={H}: lds {lds} B -> {LDS // lds} workgroups (x4 wavefronts) per CU by LDS")
    print(f"  kernel  best {best:9.3f} ms  median {med:9.3f}  worst {worst:9.3f}  "
          f"-> {R / (best * 1e-3):12,.0f} req/s, {best * 1e3 / R:8.2f} us/req (best)", flush=True)

    S = min(args.single, R)
    single_loop(mats, dem, caps, starts, inv_t0, inv_alpha, 2)      # untimed
    runs = [single_loop(mats, dem, caps, starts, inv_t0, inv_alpha, S) * 1e6 for _ in range(3)]
    spread = max(runs) - min(runs)
    per_req = worst * 1e3 / R
    verdict = "PASS" if per_req < min(runs) - spread else "FAIL"
    print(f"  loop    {' '.join(f'{r:9.1f}' for r in runs)} us/req  (spread {spread:.1f})  "
          f"batched worst {per_req:.2f} us/req: {min(runs) / per_req:7.1f}x  {verdict}", flush=True)

    reqs = [((mats[x] if H > 1 else mats[x, 0]), [{"id": i, "demand": int(d)} for i, d in
                                                 enumerate(dem[x])], caps[x], starts[x])
            for x in range(R)]
    solver.solve_vrp_sa_batch(reqs[:max(1, R // 10)], steps=STEPS, seed=SEED)     # untimed
    t0 = time.perf_counter()
    res = solver.solve_vrp_sa_batch(reqs, steps=STEPS, seed=SEED)
    dt = time.perf_counter() - t0
    print(f"  solve_vrp_sa_batch end to end {dt:7.3f} s -> {len(res) / dt:10,.0f} req/s, "
          f"{dt / len(res) * 1e6:8.1f} us/req", flush=True)
    del reqs, res, bufs

if args.gap:
    G, n, K = 1000, 10, 3
    mats, dem, caps, starts = instances(n, K, 1, G, 77)
    starts[:] = 0
    reqs = [(mats[x, 0], [{"id": i, "demand": int(d)} for i, d in enumerate(dem[x])], caps[x],
             starts[x]) for x in range(G)]
    sa = solver.solve_vrp_sa_batch(reqs, steps=STEPS, seed=SEED, with_unvisited=True)
    sp = solver.solve_vrp_batch("sp", reqs, with_unvisited=True)
    same = sum((len(a["unvisited"]), a["durationSum"]) == (len(b["unvisited"]), b["durationSum"])
               for a, b in zip(sa, sp))
    served = [(a, b) for a, b in zip(sa, sp) if len(a["unvisited"]) == len(b["unvisited"])]
    gaps = [a["durationSum"] / b["durationSum"] - 1 for a, b in served if b["durationSum"]]
    print(f"# quality, {G} static requests of n={n} K={K} at {STEPS} steps vs solve_vrp_batch('sp'): "
          f"{same / G:.1%} reach the optimum's (unvisited, durationSum); {len(served)} serve as many "
          f"customers, their mean primary gap {statistics.mean(gaps):.3%}, worst {max(gaps):.3%}")
ctx.close()
