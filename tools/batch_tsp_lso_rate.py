#!/usr/bin/env python3
"""Batched TSP local search rate (spec A27): for each shape (n customers, H
hour slices, R requests) and R random instances (tools/batch_vrp_ls_rate.py's:
entries 3..320, start times 0..1439), one vrpms_tsp_batch_lso launch
(tsp_batch_lso_kernel) of `--starts` descents of at most `--rounds` rounds: an
untimed launch, then `--repeats` launches timed with device events, reported as
best, median and worst, at moves = 31 (all five types) and at moves = 7.

The comparator is Context.vrp_batch_ls (A25: the same descent, every candidate
a full tour walk) on the same requests as K = 1, zero demands, capacity 0,
vehicle start = the start time, objective sum.  At moves = 7 the two answers
are identical (asserted here: tours, info rows, the keys' primary), so the ratio
of the two times is the price of a candidate and nothing else.  The bar, at the
shape 50:1: the new kernel's worst launch at moves = 7 is below the
comparator's best by more than the two spreads (worst - best) together.
Shapes of more than 100 customers time the comparator `--big-repeats` times
only (a launch of it takes tens of seconds there).

  --shapes n:H:R,...  default 20:24:10000,50:1:10000,50:24:10000,200:1:256
  --starts S          descents per request (default 64)
  --rounds C          applied moves a descent may take (default 1000)
  --repeats M         timed launches (default 5)
  --big-repeats M     timed comparator launches above 100 customers (default 2)
  --gap               also: 1,000 requests against the exact optima, at moves =
                      7 and 31: static n = 12 against solve_tsp_batch("dp"),
                      with tsp_batch_sa's share at no less kernel time beside
                      it, and hour-indexed at the largest n whose 1,000
                      requests all ride solve_tsp_batch("tdp")'s batch
  --lib PATH          an A/B build's libvrpms.so (tools/ab_build.py)

No hardware counters are read and nothing is traced."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vrpms_amd import _lib, solver  # noqa: E402
from vrpms_amd.core import OBJ_SUM, Context, tsp_batch_lso_lds, vrp_batch_ls_lds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="20:24:10000,50:1:10000,50:24:10000,200:1:256")
ap.add_argument("--starts", type=int, default=64)
ap.add_argument("--rounds", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--big-repeats", type=int, default=2)
ap.add_argument("--gap", action="store_true")
ap.add_argument("--lib", default=None, help="an A/B build (tools/ab_build.py) instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.load(args.lib)
S, ROUNDS, SEED = args.starts, args.rounds, 1
LDS = 160 * 1024

ctx = Context(0)


def instances(n, H, count, seed):
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


def line(name, ms, R):
    best, med, worst = min(ms), statistics.median(ms), max(ms)
    return (f"  {name:<22} best {best:10.3f} ms  median {med:10.3f}  worst {worst:10.3f}  "
            f"-> {R / (best * 1e-3):12,.0f} req/s, {best * 1e3 / R:9.2f} us/req (best)")


print(f"# {S} starts, at most {ROUNDS} rounds a descent, {args.repeats} timed launches after one "
      f"untimed, device events; comparator vrp_batch_ls at K = 1, zero demands, objective sum")
for shape in args.shapes.split(","):
    n, H, R = (int(x) for x in shape.split(":"))
    N = n + 1
    lds, lds_old = tsp_batch_lso_lds(N, H, False), vrp_batch_ls_lds(N, 1, H, False)
    if max(lds, lds_old) > LDS:
        print(f"n={n} H={H}: needs {lds} B of LDS, outside the {LDS} B domain: not measured")
        continue
    mats, starts = instances(n, H, R, 1000 * n + H)
    dm = torch.tensor(mats, dtype=torch.int32, device=ctx.dev)
    ds = torch.tensor(starts, dtype=torch.int32, device=ctx.dev)
    zero = torch.zeros((R, N), dtype=torch.int32, device=ctx.dev)
    caps = torch.zeros((R, 1), dtype=torch.int32, device=ctx.dev)
    dst = ds.reshape(R, 1).contiguous()
    print(f"n={n} H={H} R={R} S={S}: lds {lds} B -> {LDS // lds} workgroups (x4 wavefronts) per CU "
          f"by LDS (comparator {lds_old} B -> {LDS // lds_old})", flush=True)
    ms31, out31 = timed(lambda: ctx.tsp_batch_lso(dm, ds, S, ROUNDS, 31, SEED, wide=False),
                        args.repeats)
    assert not (out31[1] == -1).any().item()
    print(line("tsp_batch_lso moves=31", ms31, R) +
          f"; {int(out31[3][:, 1].sum().item())} of {R * S} descents capped", flush=True)
    ms7, out7 = timed(lambda: ctx.tsp_batch_lso(dm, ds, S, ROUNDS, 7, SEED, wide=False),
                      args.repeats)
    print(line("tsp_batch_lso moves=7", ms7, R) +
          f"; {int(out7[3][:, 1].sum().item())} of {R * S} descents capped", flush=True)
    reps = args.repeats if n <= 100 else args.big_repeats
    msc, outc = timed(lambda: ctx.vrp_batch_ls(dm, zero, caps, dst, OBJ_SUM, S, ROUNDS, SEED,
                                               wide=False), reps)
    print(line(f"vrp_batch_ls K=1 ({reps}x)", msc, R), flush=True)
    same = torch.equal(out7[0], outc[0]) and torch.equal(out7[3], outc[4]) and \
        torch.equal(out7[1] >> 28, outc[1] >> 28) and torch.equal(out7[2], outc[2][:, 0])
    spread = (max(ms7) - min(ms7)) + (max(msc) - min(msc))
    verdict = "PASS" if max(ms7) < min(msc) - spread else "FAIL"
    print(f"  answers at moves=7 identical to the comparator's: {same}; comparator best / new worst "
          f"(moves=7) {min(msc) / max(ms7):8.2f}x, best / best {min(msc) / min(ms7):8.2f}x, "
          f"spreads {spread:.3f} ms: {verdict}; moves=31 mean duration "
          f"{out31[2].double().mean().item():.1f} vs moves=7 {out7[2].double().mean().item():.1f}",
          flush=True)
    assert same
    del dm, ds, zero, caps, dst

if args.gap:
    Q = 1000

    def report(name, durs, opt):
        durs, opt = np.asarray(durs, dtype=np.float64), np.asarray(opt, dtype=np.float64)
        return (f"{name}: {np.mean(durs == opt):.1%} reach the optimum, mean gap "
                f"{np.mean(durs / opt - 1):.3%}, worst {np.max(durs / opt - 1):.3%}")

    # static, n = 12, against Held-Karp
    n = 12
    mats, starts = instances(n, 1, Q, 77)
    starts[:] = 0
    reqs = [(mats[x, 0], list(range(1, n + 1)), 0, 0) for x in range(Q)]
    opt = [r["duration"] for r in solver.solve_tsp_batch("dp", reqs)]
    dm = torch.tensor(mats, dtype=torch.int32, device=ctx.dev)
    ds = torch.tensor(starts, dtype=torch.int32, device=ctx.dev)
    print(f"# quality, {Q} static requests of n = {n} vs solve_tsp_batch('dp'); S = {S}")
    lso_ms = {}
    for moves in (7, 31):
        ms, out = timed(lambda: ctx.tsp_batch_lso(dm, ds, S, ROUNDS, moves, SEED, wide=False),
                        args.repeats)
        lso_ms[moves] = min(ms)
        print("#   " + report(f"tsp_batch_lso moves={moves} (kernel best {min(ms):.3f} ms, worst "
                              f"{max(ms):.3f})", out[2].cpu().numpy(), opt), flush=True)
    nz = mats[mats > 0]
    edge = float(nz.mean())
    flat = dm[:, 0].contiguous()
    steps = 64
    while True:   # the first doubling whose best launch takes no less than the local search's
        inv_alpha = (0.5 / 0.002) ** (1.0 / steps)
        ms, out = timed(lambda: ctx.tsp_batch_sa(flat, steps, 1.0 / (0.5 * edge), inv_alpha, SEED),
                        args.repeats)
        if min(ms) >= lso_ms[31] or steps >= 1 << 22:
            break
        steps *= 2
    sa = ((out[1].cpu().numpy().astype(np.uint64) >> np.uint64(28)) & np.uint64(2**28 - 1))
    print("#   " + report(f"tsp_batch_sa steps={steps} (kernel best {min(ms):.3f} ms, worst "
                          f"{max(ms):.3f}; no fewer than moves=31's {lso_ms[31]:.3f} ms)", sa, opt),
          flush=True)
    # hour-indexed, the largest n whose requests all ride tsp_batch_tdp
    for n in range(solver.BATCH_TDP_MAX_CUSTOMERS, 1, -1):
        mats, starts = instances(n, 24, Q, 78)
        cis = [solver.compact_tsp(mats[x], list(range(1, n + 1)), 0, int(starts[x])) for x in range(Q)]
        if all(solver.batch_tdp_fits(ci, solver._check_tdp(ci, None)) for ci in cis):
            break
    reqs = [(mats[x], list(range(1, n + 1)), 0, int(starts[x])) for x in range(Q)]
    opt = [r["duration"] for r in solver.solve_tsp_batch("tdp", reqs)]
    dm = torch.tensor(mats, dtype=torch.int32, device=ctx.dev)
    ds = torch.tensor(starts, dtype=torch.int32, device=ctx.dev)
    print(f"# quality, {Q} hour-indexed requests of n = {n} (the largest whose {Q} requests all ride "
          f"tsp_batch_tdp with the default bound) vs solve_tsp_batch('tdp'); S = {S}")
    for moves in (7, 31):
        ms, out = timed(lambda: ctx.tsp_batch_lso(dm, ds, S, ROUNDS, moves, SEED, wide=False),
                        args.repeats)
        print("#   " + report(f"tsp_batch_lso moves={moves} (kernel best {min(ms):.3f} ms, worst "
                              f"{max(ms):.3f})", out[2].cpu().numpy(), opt), flush=True)
ctx.close()
