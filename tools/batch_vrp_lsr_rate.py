#!/usr/bin/env python3
"""Rate of the batched VRP multi-start local search over separator tours (spec
A26): for each shape (n customers, K vehicles, H hour slices) and R = 10,000
random instances (tools/batch_vrp_ls_rate.py's: entries 3..320, demands 1..9,
K unequal capacities that carry 1.2 times the total demand together, start
times 0..1439), requests/s of one vrpms_vrp_batch_lsr launch
(vrp_batch_lsr_kernel) of `--starts` descents of at most `--rounds` rounds: an
untimed launch, then `--repeats` launches timed with device events, reported
as best, median and worst, with the share of descents the round cap stopped.
Beside it

  * vrpms_vrp_batch_ls (A25, the same descent on tours without separators) on
    the same instances, timed the same way in the same run, and the ratio of
    the two best times;
  * the workgroups per CU the shape's LDS bytes leave room for (160 KiB a CU);
  * solver.solve_vrp_lsr_batch end to end on the same requests as host tuples
    (compaction, guards, staging, upload, launch, read-back, result dicts;
    wall clock, one run after one untimed run on a tenth of them);
  * the same work one request at a time: solver.solve_vrp("lsr") looped over
    `--single` of the same requests (0 skips it), three runs after two untimed
    requests (wall clock, it synchronises per request), each run's time per
    request.

The batched launch passes when its time per request at its worst launch is
below the loop's best run by more than the loop's own spread (worst run - best
run).

  --shapes n:K:H,...  default 20:4:24,50:8:1,50:8:24
  --requests R        requests per launch (default 10000)
  --starts S          descents per request (default 64)
  --rounds C          applied moves a descent may take (default 1000)
  --repeats M         timed launches (default 5)
  --gap               also: 1,000 static requests of (n = 10, K = 3) against
                      solve_vrp_batch("sp")'s optima at S = 4, 16, 64 and 256:
                      the share that reaches the optimum's (unvisited,
                      durationSum), the mean primary gap and the kernel time,
                      vrp_batch_ls beside vrp_batch_lsr
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
from vrpms_amd.core import OBJ_SUM, Context, vrp_batch_lsr_lds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="20:4:24,50:8:1,50:8:24")
ap.add_argument("--requests", type=int, default=10000)
ap.add_argument("--starts", type=int, default=64)
ap.add_argument("--rounds", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--single", type=int, default=64, help="requests of the single-request loop")
ap.add_argument("--gap", action="store_true")
ap.add_argument("--lib", default=None, help="an A/B build (tools/ab_build.py) instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.load(args.lib)
R, S, ROUNDS, SEED = args.requests, args.starts, args.rounds, 1
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


def tuples(mats, dem, caps, starts, H, count):
    return [((mats[x] if H > 1 else mats[x, 0]), [{"id": i, "demand": int(d)} for i, d in
                                                 enumerate(dem[x])], caps[x], starts[x])
            for x in range(count)]


def single_loop(reqs, first, count):
    """-> seconds per request of one pass over requests first .. first + count - 1."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in reqs[first:first + count]:
        solver.solve_vrp("lsr", *r, starts=S, rounds=ROUNDS, seed=SEED)
    return (time.perf_counter() - t0) / count


print(f"# R = {R} random instances per launch, {S} starts, at most {ROUNDS} rounds a descent, "
      f"objective sum, {args.repeats} timed launches after one untimed; single-request loop over "
      f"{args.single}, three runs after two untimed requests")
for shape in args.shapes.split(","):
    n, K, H = (int(x) for x in shape.split(":"))
    N = n + 1
    lds = vrp_batch_lsr_lds(N, K, H, False)
    if lds > LDS:
        print(f"n={n} K={K} H={H}: needs {lds} B of LDS, outside the {LDS} B domain: not measured")
        continue
    mats, dem, caps, starts = instances(n, K, H, R, 1000 * n + K + H)
    bufs = [torch.tensor(a, dtype=torch.int32, device=ctx.dev) for a in (mats, dem, caps, starts)]
    ms, out = timed(lambda: ctx.vrp_batch_lsr(*bufs, OBJ_SUM, S, ROUNDS, SEED, wide=False),
                    args.repeats)
    assert not (out[1] == -1).any().item()
    best, med, worst = min(ms), statistics.median(ms), max(ms)
    capped = int(out[4][:, 1].sum().item())
    print(f"n={n} K={K} H={H} S={S}: lds {lds} B -> {LDS // lds} workgroups (x4 wavefronts) per CU "
          f"by LDS; {capped} of {R * S} descents capped")
    print(f"  kernel  best {best:9.3f} ms  median {med:9.3f}  worst {worst:9.3f}  "
          f"-> {R / (best * 1e-3):12,.0f} req/s, {best * 1e3 / R:8.2f} us/req (best)", flush=True)
    ms25, out25 = timed(lambda: ctx.vrp_batch_ls(*bufs, OBJ_SUM, S, ROUNDS, SEED, wide=False),
                        args.repeats)
    print(f"  vrp_batch_ls  best {min(ms25):9.3f} ms  median {statistics.median(ms25):9.3f}  worst "
          f"{max(ms25):9.3f}; {int(out25[4][:, 1].sum().item())} capped  -> vrp_batch_lsr takes "
          f"{best / min(ms25):.2f}x its time (best to best), (L / n)^3 = {((n + K - 1) / n) ** 3:.2f}",
          flush=True)

    reqs = tuples(mats, dem, caps, starts, H, R)
    Q = min(args.single, R - 2)
    if Q > 0:
        single_loop(reqs, 0, 2)      # untimed
        runs = [single_loop(reqs, 0, Q) * 1e6 for _ in range(3)]
        spread = max(runs) - min(runs)
        per_req = worst * 1e3 / R
        verdict = "PASS" if per_req < min(runs) - spread else "FAIL"
        print(f"  loop    {' '.join(f'{r:9.1f}' for r in runs)} us/req  (spread {spread:.1f})  "
              f"batched worst {per_req:.2f} us/req: {min(runs) / per_req:7.1f}x  {verdict}", flush=True)

    kw = dict(starts=S, rounds=ROUNDS, seed=SEED)
    solver.solve_vrp_lsr_batch(reqs[:max(1, R // 10)], **kw)     # untimed
    t0 = time.perf_counter()
    res = solver.solve_vrp_lsr_batch(reqs, **kw)
    dt = time.perf_counter() - t0
    print(f"  solve_vrp_lsr_batch end to end {dt:7.3f} s -> {len(res) / dt:10,.0f} req/s, "
          f"{dt / len(res) * 1e6:8.1f} us/req", flush=True)
    del reqs, res, bufs

if args.gap:
    Q, n, K = 1000, 10, 3
    mats, dem, caps, starts = instances(n, K, 1, Q, 77)
    starts[:] = 0
    reqs = tuples(mats, dem, caps, starts, 1, Q)
    sp = solver.solve_vrp_batch("sp", reqs, with_unvisited=True)

    def quality(name, got):
        same = sum((len(a["unvisited"]), a["durationSum"]) == (len(b["unvisited"]), b["durationSum"])
                   for a, b in zip(got, sp))
        served = [(a, b) for a, b in zip(got, sp) if len(a["unvisited"]) == len(b["unvisited"])]
        gaps = [a["durationSum"] / b["durationSum"] - 1 for a, b in served if b["durationSum"]]
        return (f"{name}: {same / Q:.1%} reach the optimum's (unvisited, durationSum); {len(served)} "
                f"serve as many customers, their mean primary gap {statistics.mean(gaps):.3%}, worst "
                f"{max(gaps):.3%}")

    bufs = [torch.tensor(a, dtype=torch.int32, device=ctx.dev) for a in (mats, dem, caps, starts)]
    print(f"# quality, {Q} static requests of n={n} K={K} vs solve_vrp_batch('sp')")
    for s in (4, 16, 64, 256):
        for name, launch, solve in (("vrp_batch_lsr", ctx.vrp_batch_lsr, solver.solve_vrp_lsr_batch),
                                    ("vrp_batch_ls", ctx.vrp_batch_ls, solver.solve_vrp_ls_batch)):
            ms, out = timed(lambda: launch(*bufs, OBJ_SUM, s, ROUNDS, SEED, wide=False), args.repeats)
            capped = int(out[4][:, 1].sum().item())
            print("#   " + quality(f"{name} S={s} rounds<={ROUNDS} (kernel best {min(ms):.3f} ms, "
                                   f"worst {max(ms):.3f}; {capped} capped)",
                                   solve(reqs, starts=s, rounds=ROUNDS, seed=SEED,
                                         with_unvisited=True)), flush=True)
ctx.close()
