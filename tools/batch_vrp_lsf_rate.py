#!/usr/bin/env python3
"""Rate of the batched VRP multi-start local search over plain separator tours
with delta pricing (spec A28) against the walking search it restricts (A26):
for each shape (n customers, K vehicles, R requests; static matrices) and
tools/batch_vrp_lsr_rate.py's random instances (entries 3..320, demands 1..9,
K unequal capacities that carry 1.2 times the total demand together), one
vrpms_vrp_batch_lsf launch of `--starts` descents of at most `--rounds` rounds
and one vrpms_vrp_batch_lsr launch on the same requests: an untimed launch,
then `--repeats` launches timed with device events, reported as best, median
and worst.  The comparator of a shape of `--slow-from` customers or more is
timed `--slow-repeats` times with no untimed launch before.

The two rows differ by design (A28 refuses the moves onto tours that are not
plain), so next to the times stand both kernels' capped counts, their mean
key primaries and the share of requests on which each kernel's key is the
lower, the candidates of a round, 2 L (L - 1), and the mean number of segments
a candidate spans on the answers' tours.

Before anything is timed, equivalence (a) is asserted on an all-roomy copy of
each shape (every capacity the total demand): there the five tensors of the
two kernels must be equal, so the ratio compares two correct kernels.

The bar, at every shape: the new kernel's worst launch lies below the
comparator's best by more than the two spreads (worst - best) together.

  --shapes n:K:R,...  default 20:4:10000,50:8:10000,200:8:256
  --starts S          descents per request (default 64)
  --rounds C          applied moves a descent may take (default 1000)
  --repeats M         timed launches (default 5)
  --gap               also: 1,000 static requests of (n = 10, K = 3) against
                      solve_vrp_batch("sp")'s optima at S = 4, 16, 64 and 256:
                      the share that reaches the optimum's (unvisited,
                      durationSum), the mean primary gap and the kernel time,
                      vrp_batch_lsr beside vrp_batch_lsf
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
from vrpms_amd.core import OBJ_SUM, Context, vrp_batch_lsf_lds, vrp_batch_lsr_lds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="20:4:10000,50:8:10000,200:8:256")
ap.add_argument("--starts", type=int, default=64)
ap.add_argument("--rounds", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--slow-from", type=int, default=200)
ap.add_argument("--slow-repeats", type=int, default=1)
ap.add_argument("--gap", action="store_true")
ap.add_argument("--lib", default=None, help="an A/B build (tools/ab_build.py) instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.load(args.lib)
S, ROUNDS, SEED = args.starts, args.rounds, 1
LDS = 160 * 1024

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


def device(*arrays):
    return [torch.tensor(a, dtype=torch.int32, device=ctx.dev) for a in arrays]


def timed(launch, repeats, untimed=True):
    """`repeats` launches timed by device events, after one untimed -> ([ms], last result)."""
    if untimed:
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


def tuples(mats, dem, caps, starts, count):
    return [(mats[x, 0], [{"id": i, "demand": int(d)} for i, d in enumerate(dem[x])], caps[x],
             starts[x]) for x in range(count)]


def primaries(keys):
    return ((keys.cpu().numpy().astype(np.uint64) >> np.uint64(28)) & np.uint64(2**28 - 1)).astype(np.int64)


def spanned(tours):
    """The mean number of segments a candidate's span [lo, hi] touches."""
    total, count = 0, 0
    for t in tours:
        before = np.concatenate([[0], np.cumsum(np.asarray(t) == 0)])   # separators in t[:x]
        lo, hi = np.triu_indices(len(t), 1)
        total += int((before[hi + 1] - before[lo] + 1).sum())
        count += len(lo)
    return total / count


def line(name, ms):
    return (f"  {name:13s} best {min(ms):10.3f} ms  median {statistics.median(ms):10.3f}  worst "
            f"{max(ms):10.3f}")


print(f"# {S} starts, at most {ROUNDS} rounds a descent, objective sum, static matrices; "
      f"{args.repeats} timed launches after one untimed (the comparator from {args.slow_from} "
      f"customers on: {args.slow_repeats} timed, none untimed)")
for shape in args.shapes.split(","):
    n, K, R = (int(x) for x in shape.split(":"))
    N, L = n + 1, n + K - 1
    lds, lds26 = vrp_batch_lsf_lds(N, K, 1, False), vrp_batch_lsr_lds(N, K, 1, False)
    if lds > LDS:
        print(f"n={n} K={K}: needs {lds} B of LDS, outside the {LDS} B domain: not measured")
        continue
    mats, dem, caps, starts = instances(n, K, R, 1000 * n + K + 1)
    # equivalence (a) first: all-roomy, the rows must be A26's
    Q = min(R, 64)
    roomy = np.repeat(dem[:Q].sum(axis=1)[:, None], K, axis=1)
    rb = device(mats[:Q], dem[:Q], roomy, starts[:Q])
    Se = S if n < args.slow_from else 4
    a = ctx.vrp_batch_lsf(*rb, OBJ_SUM, Se, ROUNDS, SEED, wide=False)
    b = ctx.vrp_batch_lsr(*rb, OBJ_SUM, Se, ROUNDS, SEED, wide=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), f"n={n} K={K}: all-roomy rows differ"
    print(f"n={n} K={K} R={R} S={S}: all-roomy copies of {Q} requests at {Se} starts: the five "
          f"tensors equal vrp_batch_lsr's", flush=True)

    bufs = device(mats, dem, caps, starts)
    ms, out = timed(lambda: ctx.vrp_batch_lsf(*bufs, OBJ_SUM, S, ROUNDS, SEED, wide=False),
                    args.repeats)
    assert not (out[1] == -1).any().item()
    slow = n >= args.slow_from
    ms26, out26 = timed(lambda: ctx.vrp_batch_lsr(*bufs, OBJ_SUM, S, ROUNDS, SEED, wide=False),
                        args.slow_repeats if slow else args.repeats, untimed=not slow)
    p, p26 = primaries(out[1]), primaries(out26[1])
    k, k26 = out[1].cpu().numpy().astype(np.uint64), out26[1].cpu().numpy().astype(np.uint64)
    print(f"  lds {lds} B -> {LDS // lds} workgroups per CU by LDS (vrp_batch_lsr {lds26} B -> "
          f"{LDS // lds26}); {2 * L * (L - 1)} candidates a round on L = {L} tokens, spanning "
          f"{spanned(out[0][:64].cpu().tolist()):.2f} of {K} segments on average")
    print(line("vrp_batch_lsf", ms) + f"  -> {R / (min(ms) * 1e-3):12,.0f} req/s, "
          f"{min(ms) * 1e3 / R:9.2f} us/req (best)")
    print(line("vrp_batch_lsr", ms26) + f"  -> {R / (min(ms26) * 1e-3):12,.0f} req/s, "
          f"{min(ms26) * 1e3 / R:9.2f} us/req (best)")
    print(f"  capped descents of {R * S}: lsf {int(out[4][:, 1].sum().item())}, lsr "
          f"{int(out26[4][:, 1].sum().item())}; mean key primary: lsf {p.mean():.2f}, lsr "
          f"{p26.mean():.2f}; the lower key: lsf on {(k < k26).mean():.1%} of the requests, lsr on "
          f"{(k26 < k).mean():.1%}, equal on {(k == k26).mean():.1%}")
    spreads = (max(ms) - min(ms)) + (max(ms26) - min(ms26))
    verdict = "PASS" if max(ms) < min(ms26) - spreads else "FAIL"
    print(f"  ratio best to best {min(ms26) / min(ms):.2f}x; lsf worst {max(ms):.3f} ms against lsr "
          f"best {min(ms26):.3f} ms less the two spreads {spreads:.3f} ms: {verdict}", flush=True)
    if not slow:
        reqs = tuples(mats, dem, caps, starts, R)
        kw = dict(starts=S, rounds=ROUNDS, seed=SEED)
        solver.solve_vrp_lsf_batch(reqs[:max(1, R // 10)], **kw)     # untimed
        t0 = time.perf_counter()
        res = solver.solve_vrp_lsf_batch(reqs, **kw)
        dt = time.perf_counter() - t0
        print(f"  solve_vrp_lsf_batch end to end {dt:7.3f} s -> {len(res) / dt:10,.0f} req/s, "
              f"{dt / len(res) * 1e6:8.1f} us/req", flush=True)
        del reqs, res
    del bufs, rb

if args.gap:
    Q, n, K = 1000, 10, 3
    mats, dem, caps, starts = instances(n, K, Q, 77)
    starts[:] = 0
    reqs = tuples(mats, dem, caps, starts, Q)
    sp = solver.solve_vrp_batch("sp", reqs, with_unvisited=True)

    def quality(name, got):
        same = sum((len(a["unvisited"]), a["durationSum"]) == (len(b["unvisited"]), b["durationSum"])
                   for a, b in zip(got, sp))
        served = [(a, b) for a, b in zip(got, sp) if len(a["unvisited"]) == len(b["unvisited"])]
        gaps = [a["durationSum"] / b["durationSum"] - 1 for a, b in served if b["durationSum"]]
        return (f"{name}: {same / Q:.1%} reach the optimum's (unvisited, durationSum); {len(served)} "
                f"serve as many customers, their mean primary gap {statistics.mean(gaps):.3%}, worst "
                f"{max(gaps):.3%}")

    bufs = device(mats, dem, caps, starts)
    print(f"# quality, {Q} static requests of n={n} K={K} vs solve_vrp_batch('sp')")
    for s in (4, 16, 64, 256):
        for name, launch, solve in (("vrp_batch_lsf", ctx.vrp_batch_lsf, solver.solve_vrp_lsf_batch),
                                    ("vrp_batch_lsr", ctx.vrp_batch_lsr, solver.solve_vrp_lsr_batch)):
            ms, out = timed(lambda: launch(*bufs, OBJ_SUM, s, ROUNDS, SEED, wide=False), args.repeats)
            capped = int(out[4][:, 1].sum().item())
            print("#   " + quality(f"{name} S={s} rounds<={ROUNDS} (kernel best {min(ms):.3f} ms, "
                                   f"worst {max(ms):.3f}; {capped} capped)",
                                   solve(reqs, starts=s, rounds=ROUNDS, seed=SEED,
                                         with_unvisited=True)), flush=True)
ctx.close()
