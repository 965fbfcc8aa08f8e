"""Drop-in solver front-end for the vrpms HTTP handlers.

Keeps the reference's entry points and result schema:
  calculate_duration(source, target, time_of_day=0)   src/solver.py:7-15
  solve_vrp_problem(**instance)                       src/solver.py:18-27
and adds the two calls the eight handler TODO slots make:
  solve_tsp(algorithm, durations, customers, start_node, start_time, ...)
      -> {'duration': int, 'vehicle': [node, ...]}     api/tsp/ga/index.py:40-44
  solve_vrp(algorithm, durations, locations, capacities, start_times,
            ignored_customers, completed_customers, ...)
      -> {'durationMax': int, 'durationSum': int,
          'vehicles': [{'tour': [0, ..., 0], 'duration': int}, ...]}
                                                       api/vrp/ga/index.py:48-53
`algorithm` is the endpoint name: 'bf', 'ga', 'sa' or 'aco', or 'dp' (TSP
only: the exact Held-Karp subset DP, spec A14), or 'sp' (VRP only: the exact
subset partition DP over all separator tours, spec A15), or 'tdp' (TSP only:
the exact time-expanded subset DP for hour-indexed matrices, spec A16), or
'tdsp' (VRP only: the exact time-expanded partition DP for hour-indexed
matrices with per-vehicle capacities and start times, spec A17).
solve_tsp_batch("dp", requests) answers many small exact TSP requests with
shared launches (spec A18), each answer solve_tsp("dp")'s, and
solve_vrp_batch("sp", requests) many small exact VRP requests (spec A19), each
answer solve_vrp("sp")'s.  All search
and scoring runs in the gfx950 kernels (vrpms_amd.core); this module only
builds the compact instance and maps results
back to matrix indices.  Node ids in results are matrix row indices
(A1), the depot / start node closing every tour as in src/solver.py:24.
"""
from __future__ import annotations

import datetime
import random
import threading
import time
from dataclasses import dataclass

import numpy as np

from . import core, runners
from .core import CVRP, OBJ_MAX, OBJ_SUM, TSP, Context

ALGORITHMS = ("bf", "ga", "sa", "aco", "dp", "sp", "tdp", "tdsp", "ls", "lsr", "lso", "lsf")
# the exact algorithms with kernels of their own: one device, no island model
# (the exhaustive "bf" shares that with them)
EXACT_ALGORITHMS = ("dp", "sp", "tdp", "tdsp")
# exhaustive search over n! giant tours: 13! = 6.2 G tours is ~0.1 s at the
# measured ~64 G evals/s of bf_kernel on one MI355X (bench "search.bf") on a
# static matrix; an hour-indexed one prices every edge at its departure
# hour (several times slower), so it keeps 11 (39.9 M tours).
# vrpms_bf_run itself accepts n <= 15 (nibble-packed tours)
BF_MAX_CUSTOMERS = 13
BF_MAX_CUSTOMERS_TD = 11
# Held-Karp (A14, static TSP only): O(2^n n^2) steps over a table of 2^n rows,
# 2 GiB at 24 customers (vrpms_tsp_dp_workspace)
DP_MAX_CUSTOMERS = 24
# batched Held-Karp (A18): one request's compact table, n 2^(n-1) words, has to
# fit one CU's LDS next to its matrix: 98,304 B at n = 12, 212,992 B at n = 13
# (vrpms_tsp_batch_dp); larger requests of a batch take the single-request path
BATCH_DP_MAX_CUSTOMERS = 12
# set partitioning (A15, static VRP only): 3^n steps per vehicle.  The kernel
# accepts 20 customers; the cap here is a time budget, the largest n <= 20
# whose median Context.vrp_sp time at K = 8 on one MI355X is at most 1 s:
# measured 0.090 s at n = 20 (tools/sp_rate.py), so it is the
# kernel's own limit.  vrpms_vrp_sp_run accepts K <= 64
SP_MAX_CUSTOMERS = 20
SP_MAX_VEHICLES = 64
# batched set partitioning (A19): one request's Held-Karp table, route table and
# K partition layers have to fit one CU's LDS (vrpms_vrp_batch_sp_lds gives the
# bytes for (n, K)): K <= 64 up to 9 customers, 32 at 10, 12 at 11, 1 at 12;
# other requests of a batch take the single-request path
BATCH_SP_MAX_CUSTOMERS = 12
BATCH_SP_LDS_BYTES = 160 * 1024
# time-expanded subset DP (A16, TSP, static or hour-indexed): 2^n n^2 / 4 W
# word steps over a table of 2^n n W words, W the hours from the start to the
# upper bound.  The kernel accepts 20 customers; the cap here follows
# SP_MAX_CUSTOMERS' rule, the largest n <= 20 whose median Context.tsp_tdp time
# on the synth.td_cvrp-derived family is at most 1 s on one MI355X and whose
# table is within TDP_MAX_WORKSPACE: measured 0.018 s at n = 20 with a 12.3 GiB
# table (tools/tdp_rate.py), so it is the kernel's own limit.
# TDP_MAX_WORKSPACE is a policy cap: one request does not claim a large share
# of a shared card.  TDP_MAX_WORDS is the kernel's row limit (W <= 512 hours)
TDP_MAX_CUSTOMERS = 20
TDP_MAX_WORKSPACE = 16 << 30
TDP_MAX_WORDS = 512
# batched time-expanded DP (A20): one request's compact table, n 2^(n-1) rows of
# W hour words, has to fit one CU's LDS next to the matrix slices its words use
# (vrpms_tsp_batch_tdp_lds gives the bytes for (n, H, W)): W = 1 at 11
# customers, up to 3 at 10, 8 at 9, 19 at 8; 12 customers never fit (196,608 B
# at W = 1).  Other requests of a batch take the single-request path
BATCH_TDP_MAX_CUSTOMERS = 11
BATCH_TDP_LDS_BYTES = 160 * 1024
# time-expanded partition DP (A17, VRP, static or hour-indexed, per-vehicle
# start times): G A16 tables, one per distinct start time, each followed by the
# route kernel, then A15's K - 1 partition layers.  The kernel accepts 20
# customers and 64 vehicles; TDSP_MAX_CUSTOMERS follows SP_MAX_CUSTOMERS' rule,
# the largest n <= 20 whose median Context.vrp_tdsp time at K = 8 on
# synth.td_cvrp_het(n, 8, seed=n) with the default upper bound is at most 1 s on
# one MI355X and whose workspace is within TDSP_MAX_WORKSPACE: measured 0.194 s
# at n = 19 with a 12.7 GiB workspace (tools/tdsp_rate.py --sizes 19, DESIGN.md
# §4.3h); n = 20 needs 32.4 GiB there, so the workspace cap decides, not time.
# TDSP_MAX_WORKSPACE is the same policy cap as TDP_MAX_WORKSPACE
TDSP_MAX_CUSTOMERS = 19
TDSP_MAX_VEHICLES = 64
TDSP_MAX_WORKSPACE = 16 << 30
# batched time-expanded partition DP (A21): one request's compact A16 table, the
# slices its words use, G route tables and K partition layers have to fit one
# CU's LDS (vrpms_vrp_batch_tdsp_lds gives the bytes for (n, K, G, H, W));
# DESIGN.md §4.3l has the largest W per (n, K, G).  12 customers never fit.
# Other requests of a batch take the single-request path
BATCH_TDSP_MAX_CUSTOMERS = 11
BATCH_TDSP_LDS_BYTES = 160 * 1024
# batched VRP annealing (A22): one request's whole [H][N][N] matrix (uint16
# cells unless an entry is above 65535), its demand, capacity and start-time
# rows and 4 chains x 3 tours have to fit one CU's LDS (vrpms_vrp_batch_sa_lds
# gives the bytes for (N, K, H, wide)); DESIGN.md §4.3m has the largest N per
# (K, H, wide).  Other requests of a batch take the single-request path
BATCH_SA_MAX_VEHICLES = 64
BATCH_SA_LDS_BYTES = 160 * 1024
# batched VRP GA (A23): next to the instance, 2 pop tours, their keys and the
# sort pairs have to fit the same budget (vrpms_vrp_batch_ga_lds gives the bytes
# for (N, K, H, wide, pop)); DESIGN.md §4.3n has the largest N per (H, wide,
# pop).  A launch has no time limit, so a request of more generations than
# BATCH_GA_MAX_GENERATIONS -- five times the endpoint's default of 400 -- takes
# the unbatched path, which has one
BATCH_GA_MAX_POP = 256
BATCH_GA_MAX_GENERATIONS = 2000
BATCH_GA_LDS_BYTES = BATCH_SA_LDS_BYTES
# batched VRP ACO (A24): next to the instance, tau and eta (4 bytes a cell
# each), `ants` tours and the best-so-far's have to fit the same budget
# (vrpms_vrp_batch_aco_lds gives the bytes for (N, K, H, wide, ants)); DESIGN.md
# §4.3o has the largest N per (H, wide, ants).  A launch has no time limit, so
# a request of more iterations than BATCH_ACO_MAX_ITERATIONS -- ten times the
# endpoint's default of 100 -- takes the unbatched path, which has one
BATCH_ACO_MAX_ANTS = 256
BATCH_ACO_MAX_ITERATIONS = 1000
BATCH_ACO_LDS_BYTES = BATCH_SA_LDS_BYTES
# batched VRP multi-start local search (A25): next to the instance only two
# tours per wavefront (vrpms_vrp_batch_ls_lds gives the bytes for (N, K, H,
# wide), never more than A22's), so the domain contains A22's; DESIGN.md §4.3p
# has the largest N per (H, wide).  A launch has no time limit and there is no
# unbatched local search, so more than BATCH_LS_MAX_STARTS starts or
# BATCH_LS_MAX_ROUNDS rounds is an error, not another path
BATCH_LS_MAX_STARTS = 1024
BATCH_LS_MAX_ROUNDS = 1000
BATCH_LS_LDS_BYTES = BATCH_SA_LDS_BYTES
# batched VRP multi-start local search over separator tours (A26): A25's descent
# on A22's tours of n + K - 1 tokens, two per wavefront
# (vrpms_vrp_batch_lsr_lds gives the bytes for (N, K, H, wide), never more than
# A22's), so the domain contains A22's; DESIGN.md §4.3q has the largest N per
# (H, wide).  As for A25, more than BATCH_LSR_MAX_STARTS starts or
# BATCH_LSR_MAX_ROUNDS rounds is an error, not another path
BATCH_LSR_MAX_STARTS = 1024
BATCH_LSR_MAX_ROUNDS = 1000
BATCH_LSR_LDS_BYTES = BATCH_SA_LDS_BYTES
# A26 by the other mapping (vrp_batch_lsr_spread): the workgroups
# a request's starts may be spread over; the answers do not depend on it
BATCH_LSR_MAX_SPREAD = 1024
# batched VRP multi-start local search over plain separator tours with delta
# pricing (A28): A26's descent restricted to the tours whose separators alone
# decide the routes, static matrices only; next to the instance a wavefront
# keeps two tours, three int32 prefix rows, a segment row and the route tables
# (vrpms_vrp_batch_lsf_lds gives the bytes for (N, K, wide)); DESIGN.md §4.3v
# has the largest N per (K, wide).  As for A25, more than BATCH_LSF_MAX_STARTS
# starts or BATCH_LSF_MAX_ROUNDS rounds is an error, not another path
BATCH_LSF_MAX_STARTS = 1024
BATCH_LSF_MAX_ROUNDS = 1000
BATCH_LSF_LDS_BYTES = BATCH_SA_LDS_BYTES
# A28 by the other mapping (vrp_batch_lsf_spread): the workgroups
# a request's starts may be spread over; the answers do not depend on it
BATCH_LSF_MAX_SPREAD = 1024
# batched TSP multi-start local search with Or-opt and delta pricing (A27): next
# to the matrix a wavefront keeps two tours and two int32 prefix rows (one on an
# hour-indexed matrix); vrpms_tsp_batch_lso_lds gives the bytes for (N, H,
# wide), DESIGN.md §4.3s has the largest N per (H, wide).  As for A25, more than
# BATCH_LSO_MAX_STARTS starts or BATCH_LSO_MAX_ROUNDS rounds is an error, not
# another path
BATCH_LSO_MAX_STARTS = 1024
BATCH_LSO_MAX_ROUNDS = 1000
BATCH_LSO_LDS_BYTES = BATCH_SA_LDS_BYTES
# A27 by the other mapping (tsp_batch_lso_spread): the workgroups
# a request's starts may be spread over; the answers do not depend on it
BATCH_LSO_MAX_SPREAD = 1024
# SA on tours of more than SA_WINDOW_MIN_N customers samples A11 windowed
# moves (second position within SA_WINDOW of the first)
SA_WINDOW, SA_WINDOW_MIN_N = 32, 150


@dataclass
class CompactInstance:
    problem: int
    durations: np.ndarray      # int64 [H][N][N] over compact nodes
    nodes: list                # compact index -> original matrix index
    demand: np.ndarray | None
    capacities: np.ndarray | None
    start_times: np.ndarray

    @property
    def N(self):
        return len(self.nodes)

    @property
    def n(self):
        return self.N - 1


def _matrix(durations) -> np.ndarray:
    """A2/A3: the DB `matrix` payload (api/database.py:45) as int64 [H][N][N]."""
    D = np.asarray(durations)
    if D.dtype == object:
        raise ValueError("duration matrix must be rectangular")
    if D.ndim == 2:
        D = D[None]
    if D.ndim != 3 or D.shape[1] != D.shape[2] or D.shape[1] == 0:
        raise ValueError("duration matrix must be [N][N] or [24][N][N]")
    if D.shape[0] not in (1, 24):
        raise ValueError("hour-indexed duration matrix must have 24 slices")
    if np.issubdtype(D.dtype, np.integer):       # the DB's JSON integers: one check
        if D.size and D.min() < 0:
            raise ValueError("durations must be non-negative integers (minutes)")
        return D.astype(np.int64, copy=False)
    if not np.issubdtype(D.dtype, np.number) or not np.all(np.isfinite(D)):
        raise ValueError("durations must be numbers")
    if np.any(D != np.floor(D)) or np.any(D < 0):
        raise ValueError("durations must be non-negative integers (minutes)")
    return D.astype(np.int64)


def compact_tsp(durations, customers, start_node, start_time=0) -> CompactInstance:
    """A4: node 0 = startNode, then the distinct customers in request order."""
    D = _matrix(durations)
    N = D.shape[1]
    start = int(start_node)
    if not 0 <= start < N:
        raise ValueError(f"startNode {start} outside the {N}-node matrix")
    nodes = [start]
    seen = {start}
    for c in customers or []:
        c = int(c)
        if not 0 <= c < N:
            raise ValueError(f"customer {c} outside the {N}-node matrix")
        if c not in seen:
            seen.add(c)
            nodes.append(c)
    # every node in matrix order (the common request): no copy
    sub = D if nodes == list(range(N)) else D[:, nodes][:, :, nodes]
    return CompactInstance(TSP, sub, nodes, None, None, np.array([int(start_time or 0)]))


def active_customers(locations, ignored_customers, completed_customers):
    """Rows i >= 1 whose location id is not ignored/completed: the solver's
    view of remove_unused_locations (api/helpers.py:11-13); the depot (row 0,
    A1) always stays."""
    disregard = list(ignored_customers or []) + list(completed_customers or [])
    return [i for i, loc in enumerate(locations) if i > 0 and loc.get("id") not in disregard]


def compact_vrp(durations, locations, capacities, start_times, ignored_customers=(),
                completed_customers=()) -> CompactInstance:
    """A1/A5: depot = node 0, customers = active locations; demand defaults to 1."""
    D = _matrix(durations)
    N = D.shape[1]
    locations = list(locations or [])
    if len(locations) != N:
        raise ValueError(f"{len(locations)} locations but a {N}-node duration matrix")
    caps = [int(c) for c in (capacities if capacities is not None else [])]
    starts = [int(s) for s in (start_times if start_times is not None else [])]
    if not caps:
        raise ValueError("at least one vehicle capacity is required")
    if len(starts) != len(caps):
        raise ValueError("capacities and startTimes must have the same length")
    if min(caps) < 0 or min(starts) < 0:
        raise ValueError("capacities and start times must be non-negative")
    nodes = [0] + active_customers(locations, ignored_customers, completed_customers)
    dem = np.array([0] + [int(locations[i].get("demand", 1)) for i in nodes[1:]], dtype=np.int64)
    if dem.min() < 0:
        raise ValueError("demands must be non-negative")
    sub = D[:, nodes][:, :, nodes]
    return CompactInstance(CVRP, sub, nodes, dem, np.array(caps), np.array(starts))


# ---------------------------------------------------------------------------
# device context (one per process; the handlers call in sequentially)
# ---------------------------------------------------------------------------
_CTX: dict = {}
_CTX_LOCK = threading.Lock()


def context(device: int = 0) -> Context:
    """The process-wide context on `device`, one per device (created once;
    the check and the creation are one critical section, so concurrent first
    calls from the request threads and the batcher share a single vrpms_ctx
    per device)."""
    with _CTX_LOCK:
        ctx = _CTX.get(device)
        if ctx is None:
            ctx = _CTX[device] = Context(device)
        return ctx


def load(ctx: Context, ci: CompactInstance, objective: int = OBJ_SUM):
    if ci.problem == TSP:
        ctx.set_instance(TSP, ci.durations, start_times=ci.start_times, objective=objective)
    else:
        ctx.set_instance(CVRP, ci.durations, ci.demand, ci.capacities, ci.start_times,
                         objective=objective)


def _runner(ctx: Context, ci: CompactInstance, algorithm: str, seed: int, knobs: dict):
    """(runner, epochs) for SA / GA / ACO on the loaded instance."""
    n = ci.n
    iters = knobs.get("iteration_count")
    if algorithm == "sa":
        steps = int(iters or knobs.get("steps", 4000))
        # VRP: K - 1 route separators (A10) let the moves place route
        # boundaries instead of leaving them to the greedy split alone
        n_sep = int(knobs.get("separators", len(ci.capacities) - 1 if ci.problem == CVRP else 0))
        # large tours: A11/A12 windowed 2-opt, swap / relocate anywhere
        # (priced in O(1) / route-locally); separators start where first-fit
        # routes end (a feasible start on a tight fleet, where random
        # separator positions would leave customers unserved)
        window = int(knobs.get("window", SA_WINDOW if n > SA_WINDOW_MIN_N else 0))
        r = runners.SARunner(ctx, n, chains=int(knobs.get("chains", 1024)), seed=seed,
                             total_steps=steps, durations=ci.durations, n_sep=n_sep,
                             window=window, window_types=int(knobs.get("window_types", 2)),
                             start="pack" if n_sep > 0 else "random")
        return r, max(1, steps // r.steps_per_epoch)
    if algorithm == "ga":
        pop = int(knobs.get("random_permutation_count") or knobs.get("pop", 256))
        gens = int(iters or 400)
        r = runners.GARunner(ctx, n, islands=int(knobs.get("islands", 8)), pop=max(2, min(pop, 4096)),
                             seed=seed)
        return r, max(1, gens // r.gens_per_epoch)
    if algorithm == "aco":
        its = int(iters or 100)
        r = runners.ACORunner(ctx, n, colonies=int(knobs.get("colonies", 4)),
                              ants=int(knobs.get("ants", 64)), seed=seed)
        return r, max(1, its // r.iters_per_epoch)
    raise ValueError(f"unknown algorithm {algorithm!r}; expected one of {ALGORITHMS}")


def _check_dp(ci: CompactInstance):
    """A14's domain, checked on the host before any device is touched."""
    if ci.problem != TSP:
        raise ValueError("dp solves the TSP only")
    if ci.n > DP_MAX_CUSTOMERS:
        raise ValueError(f"dp (Held-Karp) supports at most {DP_MAX_CUSTOMERS} customers "
                         f"({ci.n} given)")
    if ci.durations.shape[0] != 1:
        raise ValueError("dp (Held-Karp) needs a static duration matrix: with hour-indexed "
                         "durations the earliest arrival per (subset, node) is not an exact state")


def _check_sp(ci: CompactInstance):
    """A15's domain, checked on the host before any device is touched."""
    if ci.problem != CVRP:
        raise ValueError('sp solves the VRP only; use "dp" for the exact TSP')
    if ci.n > SP_MAX_CUSTOMERS:
        raise ValueError(f"sp (set partitioning) supports at most {SP_MAX_CUSTOMERS} customers "
                         f"({ci.n} given)")
    if len(ci.capacities) > SP_MAX_VEHICLES:
        raise ValueError(f"sp (set partitioning) supports at most {SP_MAX_VEHICLES} vehicles "
                         f"({len(ci.capacities)} given)")
    if ci.durations.shape[0] != 1:
        raise ValueError("sp (set partitioning) needs a static duration matrix: with "
                         "hour-indexed durations a route's duration depends on its start time "
                         "and the earliest arrival per (subset, node) is not an exact state")


def tdp_workspace_bytes(n: int, start_time: int, upper_bound: int) -> int:
    """vrpms_tsp_tdp_workspace's formula: 2^n n rows of W uint64 words."""
    return (1 << n) * n * ((int(start_time) % 60 + int(upper_bound)) // 60 + 1) * 8


def _check_tdp(ci: CompactInstance, upper_bound=None):
    """A16's domain and the workspace policy, checked on the host before any
    device is touched -> the upper bound the run uses (None for n <= 1)."""
    if ci.problem != TSP:
        raise ValueError("tdp solves the TSP only")
    if ci.n > TDP_MAX_CUSTOMERS:
        raise ValueError(f"tdp (time-expanded DP) supports at most {TDP_MAX_CUSTOMERS} customers "
                         f"({ci.n} given)")
    if upper_bound is not None and int(upper_bound) < 0:
        raise ValueError("tdp: upper_bound must be non-negative (minutes)")
    if ci.n <= 1:
        return None
    start = int(ci.start_times[0])
    if upper_bound is None:
        upper_bound = runners.nearest_neighbour_duration(ci.durations, ci.n, start)
    upper_bound = int(upper_bound)
    need = tdp_workspace_bytes(ci.n, start, upper_bound)
    if need > TDP_MAX_WORKSPACE:
        raise ValueError(f"tdp (time-expanded DP) would need a table of {need} bytes for {ci.n} "
                         f"customers and an upper bound of {upper_bound} minutes; the cap is "
                         f"{TDP_MAX_WORKSPACE} bytes")
    if (start % 60 + upper_bound) // 60 + 1 > TDP_MAX_WORDS or start + upper_bound >= 2**31:
        raise ValueError(f"tdp (time-expanded DP) supports an upper bound of at most "
                         f"{TDP_MAX_WORDS} hours from the start ({upper_bound} minutes given)")
    return upper_bound


def tdsp_workspace_bytes(n: int, K: int, G: int, max_start: int, upper_bound: int) -> int:
    """vrpms_vrp_tdsp_workspace's formula: one A16 table of 2^n n rows of W
    uint64 words, G + K + 2 arrays of 2^n uint32, and 8 K + 16 bytes."""
    W = (min(59, int(max_start)) + int(upper_bound)) // 60 + 1
    return (1 << n) * n * W * 8 + (4 << n) * (G + K + 2) + 8 * K + 16


def _check_tdsp(ci: CompactInstance, objective: int, upper_bound=None):
    """A17's domain and the workspace policy, checked on the host before any
    device is touched -> the upper bound the run uses (None for n = 0)."""
    if ci.problem != CVRP:
        raise ValueError('tdsp solves the VRP only; use "tdp" for the exact time-dependent TSP')
    if ci.n > TDSP_MAX_CUSTOMERS:
        raise ValueError(f"tdsp (time-expanded partition DP) supports at most "
                         f"{TDSP_MAX_CUSTOMERS} customers ({ci.n} given)")
    K = len(ci.capacities)
    if K > TDSP_MAX_VEHICLES:
        raise ValueError(f"tdsp (time-expanded partition DP) supports at most "
                         f"{TDSP_MAX_VEHICLES} vehicles ({K} given)")
    if upper_bound is not None and int(upper_bound) < 0:
        raise ValueError("tdsp: upper_bound must be non-negative (minutes)")
    if ci.n == 0:
        return None
    if upper_bound is None:
        upper_bound = runners.tdsp_default_bound(ci.durations, ci.demand, ci.capacities,
                                                 ci.start_times, ci.n, objective == OBJ_MAX)
    upper_bound = int(upper_bound)
    starts = [int(s) for s in ci.start_times]
    need = tdsp_workspace_bytes(ci.n, K, len(set(starts)), max(starts), upper_bound)
    if need > TDSP_MAX_WORKSPACE:
        raise ValueError(f"tdsp (time-expanded partition DP) would need a workspace of {need} "
                         f"bytes for {ci.n} customers, {K} vehicles and an upper bound of "
                         f"{upper_bound} minutes; the cap is {TDSP_MAX_WORKSPACE} bytes")
    if (min(59, max(starts)) + upper_bound) // 60 + 1 > TDP_MAX_WORDS or \
            max(starts) + upper_bound >= 2**31:
        raise ValueError(f"tdsp (time-expanded partition DP) supports an upper bound of at most "
                         f"{TDP_MAX_WORDS} hours from the start ({upper_bound} minutes given)")
    return upper_bound


def search_islands(ci: CompactInstance, algorithm: str, devices, seed: int = 0,
                   time_limit: float | None = None, objective: int = OBJ_SUM, **knobs):
    """The island model inside one process: one SA / GA / ACO
    island per device (seed + 1000 d), the same epochs enqueued on every
    device, the E best migrating every 5 epochs device to device
    (islands.exchange_local).  -> (key, compact giant tour) of the best
    island."""
    import torch
    from . import islands
    if ci.n <= 1 or algorithm in ("bf",) + EXACT_ALGORITHMS:
        raise ValueError("search_islands: SA / GA / ACO on two or more customers")
    rs, epochs = [], 1
    for d, dev in enumerate(devices):
        ctx = context(dev)
        load(ctx, ci, objective)
        r, epochs = _runner(ctx, ci, algorithm, seed + 1000 * d, knobs)
        rs.append(r)

    def sync():
        for dev in devices:
            torch.cuda.synchronize(dev)
    key, tour = islands.run_local(rs, epochs, exchange_every=5, E=min(8, rs[0].src()[1].numel()),
                                  time_limit=time_limit, sync=sync if time_limit else None)
    return key, [int(x) for x in tour.cpu().tolist()]


def search(ctx: Context, ci: CompactInstance, algorithm: str, seed: int = 0,
           time_limit: float | None = None, objective: int = OBJ_SUM, **knobs):
    """Run one algorithm on the loaded instance -> (key, compact giant tour).
    `objective` is the loaded one ("tdsp"'s default upper bound depends on it)."""
    n = ci.n
    if algorithm == "dp":
        _check_dp(ci)
    if algorithm == "sp":
        _check_sp(ci)
    if algorithm == "tdp":
        bound = _check_tdp(ci, knobs.get("upper_bound"))
    if algorithm == "tdsp":
        bound = _check_tdsp(ci, objective, knobs.get("upper_bound"))
    if n == 0:
        return None, []
    if algorithm == "sp":
        return runners.set_partition(ctx, n)
    if algorithm == "tdsp":
        return runners.td_set_partition(ctx, n, bound)
    if n == 1:
        return None, [1]
    if algorithm == "dp":
        return runners.held_karp(ctx, n)
    if algorithm == "tdp":
        return runners.time_expanded(ctx, n, ci.durations, int(ci.start_times[0]), bound)
    if algorithm == "bf":
        cap = BF_MAX_CUSTOMERS if ci.durations.shape[0] == 1 else BF_MAX_CUSTOMERS_TD
        if n > cap:
            raise ValueError(f"brute force supports at most {cap} customers "
                             f"({n} given)")
        return runners.brute_force(ctx, n)
    r, epochs = _runner(ctx, ci, algorithm, seed, knobs)
    t0 = time.perf_counter()
    e = 0
    while True:
        r.epoch()
        e += 1
        if time_limit is not None:
            if time.perf_counter() - t0 >= time_limit:
                break
        elif e >= epochs:
            break
    key, tour = r.best()
    return key, [int(x) for x in tour.cpu().tolist()]


def _decode(ctx: Context, tour):
    import torch
    t = torch.tensor(tour, dtype=torch.int16, device=ctx.dev)
    return ctx.decode(t, len(tour))


def tsp_result(ci: CompactInstance, tour, duration) -> dict:
    """The TSP slot dict from a compact tour, mapped back through ci.nodes."""
    return {"duration": duration, "vehicle": [ci.nodes[c] for c in [0] + list(tour) + [0]]}


def _remote():
    """VRPMS_REMOTE set and no local GPU: the GPU box's URL (vrpms_amd.remote)."""
    from . import remote
    if remote.url() is None:
        return None
    import torch
    return None if torch.cuda.is_available() else remote


def _searched(ci, algorithm, seed, time_limit, device, devices, objective, knobs):
    """(context holding the instance, compact tour): one device, or the
    island model across `devices` (two or more) for SA / GA / ACO."""
    if devices is not None and len(devices) > 1 and ci.n > 1 and \
            algorithm not in ("bf",) + EXACT_ALGORITHMS:
        _, tour = search_islands(ci, algorithm, list(devices), seed=seed, time_limit=time_limit,
                                 objective=objective, **knobs)
        return context(devices[0]), tour
    if algorithm in EXACT_ALGORITHMS and devices:
        device = devices[0]
    ctx = context(device)
    load(ctx, ci, objective)
    _, tour = search(ctx, ci, algorithm, seed=seed, time_limit=time_limit, objective=objective,
                     **knobs)
    return ctx, tour


def solve_tsp(algorithm: str, durations, customers, start_node, start_time=0, *, seed: int = 0,
              time_limit: float | None = None, device: int = 0, devices=None, **knobs) -> dict:
    """Result dict of the TSP TODO slot (api/tsp/ga/index.py:40-44).
    `devices` (two or more): SA / GA / ACO as an island model across them;
    "dp" runs on the first of them, "bf" on `device`.  "dp" (exact, at most DP_MAX_CUSTOMERS
    customers, static matrix) ignores `seed` and `time_limit`, as "bf" does;
    its domain is checked before any device or remote is touched.  "tdp"
    (exact, at most TDP_MAX_CUSTOMERS customers, static or hour-indexed matrix)
    does the same; its knob `upper_bound` (minutes, default the
    nearest-neighbour tour's duration) bounds the tour duration, and the table
    it implies must fit TDP_MAX_WORKSPACE.  "lso" (spec A27: a multi-start
    local search with Or-opt moves and delta pricing on a static or
    hour-indexed matrix; knobs `starts`, default 64, at most
    BATCH_LSO_MAX_STARTS, `rounds`, default 1000, at most BATCH_LSO_MAX_ROUNDS,
    and `moves`, the mask of enabled move types, default 31) answers with a
    one-request tsp_batch_lso launch on the first of `devices`:
    solve_tsp_lso_batch's answer for the request.  It ignores `time_limit`; its
    domain (the matrix has to fit the LDS: batch_lso_message) is checked before
    any device or remote is touched.  Its knob `spread` (None, "auto" or
    1..BATCH_LSO_MAX_SPREAD; batch_lso_launch) spreads the request's starts
    over that many workgroups: the same answer, sooner for a lone request."""
    ci = None
    if algorithm == "sp":
        raise ValueError('sp solves the VRP only (set partitioning over a fleet); use "dp" for '
                         'the exact TSP')
    if algorithm == "tdsp":
        raise ValueError('tdsp solves the VRP only (a fleet with per-vehicle start times); use '
                         '"tdp" for the exact time-dependent TSP')
    if algorithm == "ls":
        raise ValueError('ls solves the VRP only (a multi-start local search over the greedy '
                         'split of a giant tour); use solve_vrp("ls") with one vehicle, or sa, '
                         'ga or aco for the TSP')
    if algorithm == "lsr":
        raise ValueError('lsr solves the VRP only (a multi-start local search over giant tours '
                         'with route separators); use solve_vrp("lsr") with one vehicle, or sa, '
                         'ga or aco for the TSP')
    if algorithm == "lsf":
        raise ValueError('lsf solves the VRP only (a multi-start local search over plain giant '
                         'tours with route separators); use solve_vrp("lsf") with one vehicle, or '
                         'lso, sa, ga or aco for the TSP')
    if algorithm == "dp":
        ci = compact_tsp(durations, customers, start_node, start_time)
        _check_dp(ci)
    if algorithm == "tdp":
        ci = compact_tsp(durations, customers, start_node, start_time)
        _check_tdp(ci, knobs.get("upper_bound"))
    if algorithm == "lso":
        ci = compact_tsp(durations, customers, start_node, start_time)
        lso = _single_knobs("lso", ci, knobs)
        if ci.n == 0:              # no customer: answered on the host
            return _heuristic_result(ci, None)
    rem = _remote()
    if rem is not None:
        return rem.solve_tsp(algorithm, durations, customers, start_node, start_time, seed=seed,
                             time_limit=time_limit, **knobs)
    if algorithm == "lso":         # a one-request tsp_batch_lso launch on one device
        return _solve_single("lso", ci, *lso, seed, devices[0] if devices else device)
    if ci is None:
        ci = compact_tsp(durations, customers, start_node, start_time)
    ctx, tour = _searched(ci, algorithm, seed, time_limit, device, devices, OBJ_SUM, knobs)
    _, dur = _decode(ctx, tour)
    return tsp_result(ci, tour, int(dur[0]))


def solve_vrp(algorithm: str, durations, locations, capacities, start_times,
              ignored_customers=(), completed_customers=(), *, seed: int = 0,
              objective: str = "sum", time_limit: float | None = None, device: int = 0,
              devices=None, with_unvisited: bool = False, **knobs) -> dict:
    """Result dict of the VRP TODO slot (api/vrp/ga/index.py:48-53); A7 shapes.
    `devices` (two or more): SA / GA / ACO as an island model across them.
    "sp" (exact over all separator tours: at most SP_MAX_CUSTOMERS customers
    and SP_MAX_VEHICLES vehicles, static matrix) minimises (unvisited,
    primary) only; it runs on the first of `devices`, ignores `seed` and
    `time_limit`, and its domain is checked before any device or remote is
    touched.  "tdsp" (exact over all separator tours: at most
    TDSP_MAX_CUSTOMERS customers and TDSP_MAX_VEHICLES vehicles, static or
    hour-indexed matrix, per-vehicle capacities and start times) does the
    same; its knob `upper_bound` (minutes) bounds every single route and
    defaults to an always-valid bound (runners.tdsp_default_bound); the
    workspace it implies must fit TDSP_MAX_WORKSPACE.  With an `upper_bound`
    below the optimum's primary the answer is the optimum among solutions
    whose every route fits it, which may leave customers unvisited: the
    caller owns that promise.  "ls" (spec A25: a multi-start local search,
    knobs `starts`, default 64, at most BATCH_LS_MAX_STARTS, and `rounds`,
    default 1000, at most BATCH_LS_MAX_ROUNDS) answers with a one-request
    vrp_batch_ls launch on the first of `devices`: solve_vrp_ls_batch's answer
    for the request.  It ignores `time_limit`; its domain (the instance has to
    fit the LDS: batch_ls_message) is checked before any device or remote is
    touched.  "lsr" (spec A26: the same descent on giant tours with K - 1
    route separators, started from first-fit packed tours; the same knobs,
    limits BATCH_LSR_MAX_STARTS and BATCH_LSR_MAX_ROUNDS) answers likewise with
    a one-request vrp_batch_lsr launch: solve_vrp_lsr_batch's answer for the
    request, its domain batch_lsr_message's.  Its knob `spread` (None, "auto"
    or 1..BATCH_LSR_MAX_SPREAD; batch_lsr_launch) spreads the request's starts
    over that many workgroups: the same answer, sooner for a lone request.
    "lsf" (spec A28: "lsr" restricted to the plain tours, whose separators
    alone decide the routes, priced without walking them; static matrices
    only, the same knobs, limits BATCH_LSF_MAX_STARTS and BATCH_LSF_MAX_ROUNDS)
    answers with a one-request vrp_batch_lsf launch: solve_vrp_lsf_batch's
    answer for the request, its domain batch_lsf_message's; an hour-indexed
    request keeps "lsr".  Its knob `spread` (None, "auto" or
    1..BATCH_LSF_MAX_SPREAD; batch_lsf_launch) is "lsr"'s: the same answer by
    vrp_batch_lsf_spread, sooner for a lone request."""
    if algorithm == "dp":
        raise ValueError("dp solves the TSP only (the greedy split of a giant tour does not "
                         "decompose over subsets); use bf, sa, ga or aco for the VRP")
    if algorithm == "tdp":
        raise ValueError("tdp solves the TSP only: per-vehicle start times (one table per "
                         "vehicle) and the capacity split are out of spec A16's scope; use bf, "
                         "sa, ga or aco for a time-dependent VRP, or tdsp for the exact one")
    if algorithm == "lso":
        raise ValueError('lso solves the TSP only (its delta pricing has no fleet and no capacity '
                         'split); use "ls" or "lsr" for a local search on the VRP')
    ci = None
    if algorithm == "sp":
        ci = compact_vrp(durations, locations, capacities, start_times, ignored_customers,
                         completed_customers)
        _check_sp(ci)
    if algorithm == "tdsp":
        ci = compact_vrp(durations, locations, capacities, start_times, ignored_customers,
                         completed_customers)
        _check_tdsp(ci, OBJ_MAX if objective == "max" else OBJ_SUM, knobs.get("upper_bound"))
    if algorithm in ("ls", "lsr", "lsf"):
        if objective not in ("sum", "max"):
            raise ValueError("objective must be 'sum' or 'max'")
        ci = compact_vrp(durations, locations, capacities, start_times, ignored_customers,
                         completed_customers)
        ls = _single_knobs(algorithm, ci, knobs)
    rem = _remote()
    if rem is not None:
        out = rem.solve_vrp(algorithm, durations, locations, capacities, start_times,
                            ignored_customers, completed_customers, seed=seed,
                            objective=objective, time_limit=time_limit, **knobs)
        if with_unvisited:   # the served customers' complement (the remote answers the slot dict)
            served = {c for v in out["vehicles"] for c in v["tour"][1:-1]}
            nodes = [0] + active_customers(list(locations or []), ignored_customers,
                                           completed_customers)
            out["unvisited"] = [c for c in nodes[1:] if c not in served]
        return out
    if algorithm in ("ls", "lsr", "lsf"):   # a one-request launch on one device
        return _solve_single(algorithm, ci, *ls, seed, devices[0] if devices else device, objective,
                             with_unvisited)
    if ci is None:
        ci = compact_vrp(durations, locations, capacities, start_times, ignored_customers,
                         completed_customers)
    ctx, tour = _searched(ci, algorithm, seed, time_limit, device, devices,
                          OBJ_MAX if objective == "max" else OBJ_SUM, knobs)
    K = len(ci.capacities)
    routes = [[] for _ in range(K)]
    unvisited = []
    if tour:
        veh, durs = _decode(ctx, tour)
        for c, v in zip(tour, veh):
            if v == -2:                # A10 separator: a route boundary, not a customer
                continue
            (routes[v] if v >= 0 else unvisited).append(ci.nodes[c])
    else:
        durs = [0] * K
    vehicles = [{"tour": [ci.nodes[0]] + r + [ci.nodes[0]], "duration": int(d)}
                for r, d in zip(routes, durs)]
    out = {"durationMax": int(max(durs) if durs else 0), "durationSum": int(sum(durs)),
           "vehicles": vehicles}
    if with_unvisited:
        out["unvisited"] = unvisited
    return out


# ---------------------------------------------------------------------------
# batched exact solvers (A18-A21): many small requests share launches
# ---------------------------------------------------------------------------
def batch_guard_message(ci: CompactInstance):
    """The int32 range checks vrpms_set_instance applies to this request on the
    single-request path -> the failing one's message, or None: max(start) +
    (N + K + 1) * max_duration < 2^31 (A9, K = 1 for a TSP; it implies the
    batched kernels' own (N + K + 1) * max(D) < 2^31) and, for a VRP,
    max(capacity) + max(demand) < 2^31."""
    mx = int(ci.durations.max()) if ci.durations.size else 0
    K = 1 if ci.problem == TSP else len(ci.capacities)
    if int(ci.start_times.max()) + (ci.N + K + 1) * mx >= 2**31:
        return "start + (N+K+1)*max_duration overflows int32 (A9 guard)"
    if ci.problem == CVRP and int(ci.capacities.max()) + int(ci.demand.max()) >= 2**31:
        return "capacity + demand overflows int32"
    return None


def batch_dp_guard(ci: CompactInstance) -> bool:
    """The request passes batch_guard_message: a TSP the A9 guard with K = 1, a
    VRP (as batch_sp_guard) the A9 guard and capacity + demand."""
    return batch_guard_message(ci) is None


batch_sp_guard = batch_dp_guard


def _stage(ctx: Context, cis, hours: bool = False) -> list:
    """The int32 device buffers of one launch's instances: the matrices
    [R][N][N] ([R][H][N][N] with `hours`) and, for a VRP, the demand [R][N] and
    capacity [R][K] rows.  One staging buffer each, no per-request copies."""
    import torch
    D = cis[0].durations
    host = [np.empty((len(cis),) + (D.shape if hours else D.shape[1:]), dtype=np.int32)]
    if cis[0].problem == CVRP:
        host += [np.empty((len(cis), cis[0].N), dtype=np.int32),
                 np.empty((len(cis), len(cis[0].capacities)), dtype=np.int32)]
    for x, ci in enumerate(cis):
        host[0][x] = ci.durations if hours else ci.durations[0]
        if len(host) > 1:
            host[1][x], host[2][x] = ci.demand, ci.capacities
    return [torch.from_numpy(a).to(ctx.dev) for a in host]


def _td_duration(ci: CompactInstance, tour) -> int:
    """The tour's duration under the A3 clock, on the host (on a static
    matrix: the sum of its edges)."""
    D, H = ci.durations, ci.durations.shape[0]
    t0 = t = int(ci.start_times[0])
    path = [0] + list(tour) + [0]
    for a, b in zip(path, path[1:]):
        t += int(D[(t // 60) % H][a][b])
    return t - t0


def _key_durations(cis, tours, keys) -> list:
    """Per TSP instance the duration its key carries: the primary field (A8: a
    TSP key is duration << 28), exact below the 2^28 - 1 clamp; a clamped one
    is priced on the host, and an all-ones key (no tour) gives None."""
    clamp = (1 << 28) - 1
    durs = []
    for ci, tour, k in zip(cis, tours, keys):
        d = (k >> 28) & clamp
        durs.append(None if k == -1 else _td_duration(ci, tour) if d == clamp else int(d))
    return durs


def batch_dp_launch(ctx: Context, cis):
    """One upload and one tsp_batch_dp launch for compact instances of one
    node count (each passed batch_dp_guard) -> (tours, durations), one row per
    instance (_key_durations)."""
    tours, keys = ctx.tsp_batch_dp(*_stage(ctx, cis))
    tours = tours.cpu().tolist()
    return tours, _key_durations(cis, tours, keys.cpu().tolist())


def batch_tdp_bound(ci: CompactInstance, upper_bound=None):
    """_check_tdp for a request that may ride a tsp_batch_tdp launch -> the
    bound its row width follows from.  One customer has the single path's
    trivial answer whatever `upper_bound` says, so its bound is its one tour's
    duration; no customer has none."""
    bound = _check_tdp(ci, upper_bound)
    if ci.n == 1:
        bound = runners.nearest_neighbour_duration(ci.durations, 1, int(ci.start_times[0]))
    return bound


def batch_tdp_fits(ci: CompactInstance, bound) -> bool:
    """A20's domain: 1..BATCH_TDP_MAX_CUSTOMERS customers and one request of
    (n, H, W) -- W the hour words of `bound` from the request's start -- within
    BATCH_TDP_LDS_BYTES.  Needs the library, no GPU."""
    from .core import tdp_words, tsp_batch_tdp_lds
    if ci.problem != TSP or not 1 <= ci.n <= BATCH_TDP_MAX_CUSTOMERS or bound is None:
        return False
    H = ci.durations.shape[0]
    start = int(ci.start_times[0])
    W = tdp_words(start, bound)
    if H not in (1, 24) or W > TDP_MAX_WORDS or start + int(bound) >= 2**31:
        return False
    return tsp_batch_tdp_lds(ci.n, H, W) <= BATCH_TDP_LDS_BYTES


def batch_tdp_launch(ctx: Context, cis, bounds):
    """One upload and one tsp_batch_tdp launch for compact instances of one
    (N, H) (each passed batch_dp_guard and batch_tdp_fits with its bound), W
    the largest of their row widths -> (tours, durations), one row per
    instance (_key_durations); the duration is None where no tour fits the
    request's bound."""
    starts = np.array([int(ci.start_times[0]) for ci in cis], dtype=np.int64)
    tours, keys = ctx.tsp_batch_tdp(*_stage(ctx, cis, hours=True), starts,
                                    np.array([int(b) for b in bounds], dtype=np.int64))
    tours = tours.cpu().tolist()
    return tours, _key_durations(cis, tours, keys.cpu().tolist())


def batch_sp_fits(ci: CompactInstance) -> bool:
    """A19's LDS domain: 1..BATCH_SP_MAX_CUSTOMERS customers on a static matrix
    whose (n, K) state fits BATCH_SP_LDS_BYTES with the auto team."""
    from .core import vrp_batch_sp_lds
    K = len(ci.capacities)
    if ci.durations.shape[0] != 1 or not 1 <= ci.n <= BATCH_SP_MAX_CUSTOMERS or \
            not 1 <= K <= SP_MAX_VEHICLES:
        return False
    return vrp_batch_sp_lds(ci.n, K) <= BATCH_SP_LDS_BYTES


def batch_sp_launch(ctx: Context, cis, objective: str = "sum"):
    """One upload and one vrp_batch_sp launch for compact instances of one
    (N, K) (each passed batch_sp_guard and batch_sp_fits) -> (tours,
    durations): per instance the n + K tour tokens and the K route
    durations."""
    tours, _, durs = ctx.vrp_batch_sp(*_stage(ctx, cis),
                                      OBJ_MAX if objective == "max" else OBJ_SUM)
    return tours.cpu().tolist(), durs.cpu().tolist()


def sp_result(ci: CompactInstance, tour, durs, with_unvisited: bool = False) -> dict:
    """The VRP slot dict from A15's tour tokens (route 0, a separator 0, ...,
    route K-1, 0, then the unserved customers) and the K route durations,
    compact indices mapped back through ci.nodes."""
    K = len(ci.capacities)
    routes, at = [], 0
    for _ in range(K):
        end = tour.index(0, at)
        routes.append([ci.nodes[c] for c in tour[at:end]])
        at = end + 1
    vehicles = [{"tour": [ci.nodes[0]] + r + [ci.nodes[0]], "duration": int(d)}
                for r, d in zip(routes, durs)]
    out = {"durationMax": int(max(durs)), "durationSum": int(sum(durs)), "vehicles": vehicles}
    if with_unvisited:
        out["unvisited"] = [ci.nodes[c] for c in tour[at:]]
    return out


def batch_tdsp_words(ci: CompactInstance, bound) -> int:
    """The hour words a request's rows need: the largest tdp_words(start_k,
    bound) over its vehicles."""
    return max((int(s) % 60 + int(bound)) // 60 + 1 for s in ci.start_times)


def batch_tdsp_fits(ci: CompactInstance, bound) -> bool:
    """A21's domain: 1..BATCH_TDSP_MAX_CUSTOMERS customers, 1..64 vehicles, a
    static or 24-slice matrix, and the request's own (n, K, G, H, W) -- G its
    distinct start times, W the hour words of `bound` from its starts -- within
    BATCH_TDSP_LDS_BYTES.  Needs the library, no GPU."""
    from .core import vrp_batch_tdsp_lds
    if ci.problem != CVRP or not 1 <= ci.n <= BATCH_TDSP_MAX_CUSTOMERS or bound is None:
        return False
    K, H = len(ci.capacities), ci.durations.shape[0]
    if not 1 <= K <= TDSP_MAX_VEHICLES or H not in (1, 24) or int(bound) < 0:
        return False
    starts = [int(s) for s in ci.start_times]
    if min(starts) < 0 or max(starts) + int(bound) >= 2**31:
        return False
    W = batch_tdsp_words(ci, bound)
    if W > TDP_MAX_WORDS:
        return False
    return vrp_batch_tdsp_lds(ci.n, K, len(set(starts)), H, W) <= BATCH_TDSP_LDS_BYTES


def _check_contract(kernel: str, keys):
    """An all-ones key after a launch of requests that passed the host's
    checks: the kernel refused what the host let through."""
    if (keys == -1).any().item():
        raise RuntimeError(f"{kernel}: a request was outside the launch's contract")


def batch_tdsp_launch(ctx: Context, cis, bounds, objective: str = "sum"):
    """One upload and one vrp_batch_tdsp launch for compact instances of one
    (N, K, H, number of distinct starts) (each passed batch_sp_guard and
    batch_tdsp_fits with its bound), W the largest of their row widths ->
    (tours, durations): per instance the n + K tour tokens and the K route
    durations."""
    starts = np.array([ci.start_times for ci in cis], dtype=np.int64)
    G = max(len(set(row)) for row in starts.tolist())
    W = max(batch_tdsp_words(ci, b) for ci, b in zip(cis, bounds))
    tours, keys, durs = ctx.vrp_batch_tdsp(*_stage(ctx, cis, hours=True), starts,
                                           np.array([int(b) for b in bounds], dtype=np.int64),
                                           OBJ_MAX if objective == "max" else OBJ_SUM, G=G, W=W)
    _check_contract("vrp_batch_tdsp", keys)
    return tours.cpu().tolist(), durs.cpu().tolist()


def _tsp_request(r):
    """A TSP batch request -> (compact_tsp's four arguments, upper bound or None)."""
    if isinstance(r, dict):
        r = (r["durations"], r["customers"], r["start_node"], r.get("start_time", 0),
             r.get("upper_bound"))
    r = tuple(r)
    r += (0,) * (4 - len(r))
    return r[:4], r[4] if len(r) > 4 else None


def _sp_request(r):
    """A VRP batch request -> (compact_vrp's six arguments, None)."""
    if isinstance(r, dict):
        r = (r["durations"], r["locations"], r["capacities"], r["start_times"],
             r.get("ignored_customers", ()), r.get("completed_customers", ()))
    r = tuple(r) + ((),) * (6 - len(r))
    return r[:6], None


def _tdsp_request(r):
    """A VRP batch request -> (compact_vrp's six arguments, upper bound or
    None); a malformed one is refused here, in words of its own."""
    if isinstance(r, dict):
        r = tuple(r.get(k) for k in ("durations", "locations", "capacities", "start_times")) + \
            (r.get("ignored_customers", ()), r.get("completed_customers", ()),
             r.get("upper_bound"))
    seq = (tuple, list, np.ndarray)
    if not isinstance(r, (tuple, list)) or not 4 <= len(r) <= 7 or \
            not all(isinstance(v, seq) for v in r[1:4]):
        raise ValueError("a VRP request is (durations, locations, capacities, "
                         "start_times[, ignored_customers, completed_customers[, "
                         "upper_bound]]) or a dict with those keys")
    r = tuple(r)
    return r[:6] + ((),) * (6 - len(r[:6])), r[6] if len(r) > 6 else None


@dataclass(frozen=True)
class BatchKind:
    """What one batched exact algorithm does differently from the others."""
    problem: int       # TSP or CVRP: compact_tsp / solve_tsp / tsp_result, or the VRP's
    request: object    # request -> (the compact_* arguments, upper bound or None)
    check: object      # (ci, objective code, upper bound) -> the bound of the run, or None
    fits: object       # (ci, bound) -> rides a launch (else: the single-request path)
    key: object        # ci -> what the instances of one launch share
    launch: object     # (ctx, cis, bounds, objective) -> (tours, durations)


BATCH_KINDS = {
    "dp": BatchKind(TSP, lambda r: (_tsp_request(r)[0], None),
                    lambda ci, obj, ub: _check_dp(ci),
                    lambda ci, bound: 2 <= ci.n <= BATCH_DP_MAX_CUSTOMERS,
                    lambda ci: ci.N,
                    lambda ctx, cis, bounds, objective: batch_dp_launch(ctx, cis)),
    "sp": BatchKind(CVRP, _sp_request,
                    lambda ci, obj, ub: _check_sp(ci),
                    lambda ci, bound: batch_sp_fits(ci),
                    lambda ci: (ci.N, len(ci.capacities)),
                    lambda ctx, cis, bounds, objective: batch_sp_launch(ctx, cis, objective)),
    "tdp": BatchKind(TSP, _tsp_request,
                     lambda ci, obj, ub: batch_tdp_bound(ci, ub),
                     batch_tdp_fits,
                     lambda ci: (ci.N, ci.durations.shape[0]),
                     lambda ctx, cis, bounds, objective: batch_tdp_launch(ctx, cis, bounds)),
    "tdsp": BatchKind(CVRP, _tdsp_request, _check_tdsp, batch_tdsp_fits,
                      lambda ci: (ci.N, len(ci.capacities), ci.durations.shape[0],
                                  len(set(int(s) for s in ci.start_times))),
                      batch_tdsp_launch),
}


def _solve_batch(algorithm: str, requests, device: int, objective: str = "sum",
                 with_unvisited: bool = False) -> list:
    """The batch entry points' one loop: every request normalised, compacted,
    checked and guarded on the host (a bad one raises with its index); with no
    local GPU each goes to the GPU box; else those that fit the LDS share one
    launch per group key and the rest take the single-request path."""
    kind = BATCH_KINDS[algorithm]
    tsp = kind.problem == TSP
    compact, single = (compact_tsp, solve_tsp) if tsp else (compact_vrp, solve_vrp)
    shared = {} if tsp else dict(objective=objective, with_unvisited=with_unvisited)
    reqs, cis, bounds, knobs = [], [], [], []
    for x, r in enumerate(requests):
        try:
            r, ub = kind.request(r)
            ci = compact(*r)
            bound = kind.check(ci, OBJ_MAX if objective == "max" else OBJ_SUM, ub)
            msg = batch_guard_message(ci)
            if msg is not None:
                raise ValueError(msg)
        except ValueError as e:
            raise ValueError(f"request {x}: {e}") from None
        reqs.append(r)
        cis.append(ci)
        bounds.append(bound)
        knobs.append(shared if ub is None else dict(shared, upper_bound=ub))
    if _remote() is not None:      # no local GPU: the GPU box answers each request
        return [single(algorithm, *r, **k) for r, k in zip(reqs, knobs)]
    out = [None] * len(cis)
    groups: dict = {}
    for x, ci in enumerate(cis):
        if kind.fits(ci, bounds[x]):
            groups.setdefault(kind.key(ci), []).append(x)
        else:
            out[x] = single(algorithm, *reqs[x], device=device, **knobs[x])
    if groups:
        ctx = context(device)
        for xs in groups.values():
            tours, durs = kind.launch(ctx, [cis[x] for x in xs], [bounds[x] for x in xs],
                                      objective)
            for x, tour, dur in zip(xs, tours, durs):
                if dur is None:
                    raise ValueError(f"request {x}: no tour within upper_bound = "
                                     f"{int(bounds[x])} minutes")
                out[x] = tsp_result(cis[x], tour, dur) if tsp else \
                    sp_result(cis[x], tour, dur, with_unvisited)
    return out


def solve_tsp_batch(algorithm: str, requests, *, device: int = 0) -> list:
    """[solve_tsp(algorithm, *r) for r in requests], element for element, with
    the small requests sharing launches.  `requests`: (durations, customers,
    start_node, start_time) tuples, or dicts with those keys.  "dp" (spec A18)
    and "tdp" (spec A20) have batched kernels.  Every request is compacted and
    checked on the host before anything is launched; a bad one raises
    solve_tsp's message for that algorithm prefixed with its index.

    "dp" (bad: hour-indexed, more than DP_MAX_CUSTOMERS customers, A9 guard):
    requests of 2..BATCH_DP_MAX_CUSTOMERS customers are grouped by node count,
    one upload and one tsp_batch_dp launch per group; none or one customer
    take solve_tsp's trivial path, and 13..24 customers its single-request
    Held-Karp, one by one.

    "tdp" (static or hour-indexed; bad: more than TDP_MAX_CUSTOMERS customers,
    a negative bound, a table or a row above the caps, A9 guard): a request may
    carry a fifth tuple element or an "upper_bound" key, the knob of
    solve_tsp("tdp") (default: the nearest-neighbour tour's duration).
    Requests inside A20's LDS domain (batch_tdp_fits: 1..11 customers, the row
    width the bound implies) are grouped by (node count, hour count), one
    upload and one tsp_batch_tdp launch per group at the group's largest row
    width; no customer, 12..20 customers and an (n, W) outside the LDS take
    solve_tsp("tdp"), one by one."""
    if algorithm not in ("dp", "tdp"):
        raise ValueError(f'solve_tsp_batch: no batched kernel for algorithm {algorithm!r}; only '
                         '"dp" (exact Held-Karp) and "tdp" (exact time-expanded DP) are batched')
    return _solve_batch(algorithm, requests, device)


def solve_vrp_batch(algorithm: str, requests, *, objective: str = "sum",
                    with_unvisited: bool = False, device: int = 0) -> list:
    """[solve_vrp(algorithm, *r, objective=objective, with_unvisited=...) for r
    in requests], element for element, with the small requests sharing
    launches.  `requests`: (durations, locations, capacities, start_times[,
    ignored_customers, completed_customers]) tuples, or dicts with those keys.
    Only "sp" has a batched kernel (spec A19).  Every request is compacted and
    checked on the host before anything is launched; a bad one (hour-indexed,
    more than SP_MAX_CUSTOMERS customers or SP_MAX_VEHICLES vehicles, the int32
    guards) raises solve_vrp("sp")'s message prefixed with its index.  Requests
    of 1..BATCH_SP_MAX_CUSTOMERS customers whose (n, K) fits the LDS
    (batch_sp_fits) are grouped by (N, K), one upload and one vrp_batch_sp
    launch per group, and their result dicts are built on the host from the
    tour tokens and the route durations; no customer, 13..20 customers and
    fleets beyond the LDS take solve_vrp("sp"), one by one.  "tdsp" has a
    batched kernel of its own behind solve_vrp_tdsp_batch (spec A21)."""
    if algorithm != "sp":
        raise ValueError(f'solve_vrp_batch: no batched kernel for algorithm {algorithm!r}; only '
                         '"sp" (exact set partitioning) is batched')
    return _solve_batch("sp", requests, device, objective, with_unvisited)


def solve_vrp_tdsp_batch(requests, *, objective: str = "sum", with_unvisited: bool = False,
                         device: int = 0) -> list:
    """[solve_vrp("tdsp", *r, objective=objective, with_unvisited=...,
    upper_bound=...) for r in requests], element for element, with the small
    requests sharing launches (spec A21).  `requests`: (durations, locations,
    capacities, start_times[, ignored_customers, completed_customers[,
    upper_bound]]) tuples, or dicts with those keys; the upper bound is the
    knob of solve_vrp("tdsp") (default: runners.tdsp_default_bound).  Every
    request is compacted and checked on the host before any device is touched
    (_check_tdsp, batch_sp_guard); a bad one raises solve_vrp("tdsp")'s message
    prefixed with its index.  Requests inside A21's LDS domain
    (batch_tdsp_fits: 1..11 customers, the row width the bound implies) are
    grouped by (node count, fleet size, hour count, number of distinct start
    times), one upload and one vrp_batch_tdsp launch per group at the group's
    largest row width, and their result dicts are built on the host from the
    tour tokens and the route durations; no customer, 12..19 customers and an
    (n, K, G, W) outside the LDS take solve_vrp("tdsp"), one by one."""
    return _solve_batch("tdsp", requests, device, objective, with_unvisited)


# ---------------------------------------------------------------------------
# batched heuristics (A22-A28): one table, one domain, one launch and one loop
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Knob:
    """A knob of a batched heuristic that its domain caps."""
    name: str            # as solve_vrp / solve_tsp take it: the name it travels under
    lo: int
    hi: int
    default: int = 0     # solve_vrp's / solve_tsp's, where the launch is their only path
    takes: str = "{}..{}"  # the domain message's words for the range


@dataclass(frozen=True)
class HeuristicKind:
    """What one batched heuristic does differently from the others."""
    # TSP or CVRP: _tsp_request, compact_tsp, solve_tsp and tsp_result, or
    # _sp_request, compact_vrp, solve_vrp and sa_result
    problem: int
    # the Context method and the contract error's name; core's "<kernel>_lds"
    # sizes one request, and lds_bytes is what that may be
    kernel: str
    lds_bytes: int
    # the capped knobs, in the order the key, the domain and the launch take
    # them; "<kernel>_lds" takes the first lds_knobs of them after the shape
    knobs: tuple = ()
    lds_knobs: int = 0
    # a request outside the domain raises the domain's message (there is no
    # other path); else it takes the single-request solver
    strict: bool = False
    # the tours carry K - 1 separators, and have a token limit
    separators: bool = False
    # "<kernel>_spread" takes up to that many workgroups per request; 0: no such form
    max_spread: int = 0
    # batch_launch names `spread` to the algorithm's launch even when none was
    # asked for; False: only when one was ("lsf", whose launch had no such
    # keyword at first, and whose callers without one call it as they did)
    spread_always: bool = True
    # static matrices only: the algorithm that takes the hour-indexed requests
    static_else: str = ""
    # _check_heuristic applies the int32 guard to a request of no customer
    guard_empty: bool = False
    # (ctx, cis, *the launch's knobs) -> (device buffers after the starts,
    # scalars after the objective); None: no buffer, int(knob) each
    launch_args: object = None


def _ls_knobs(max_starts: int, max_rounds: int, *more) -> tuple:
    """The local searches' `starts` and `rounds` at an algorithm's caps."""
    return (Knob("starts", 1, max_starts, 64, "{}..{} starts"),
            Knob("rounds", 0, max_rounds, 1000, "{}..{} rounds")) + more


def _sa_launch_args(ctx: Context, cis, steps):
    """vrp_batch_sa's own arguments: every request on its batch_sa_schedule."""
    import torch
    sched = [batch_sa_schedule(ci, steps) for ci in cis]
    inv_t0 = torch.from_numpy(np.array([s[0] for s in sched], dtype=np.float32)).to(ctx.dev)
    return (inv_t0,), (int(steps), sched[0][1])


# guard_empty: on solve_tsp's path "lso" applies the A9 guard to a request of no
# customer, on solve_vrp's "ls" and "lsr" return before it.  The table keeps
# what each did when it was written; which of the two is meant is an open question
HEURISTIC_KINDS = {
    "sa": HeuristicKind(CVRP, "vrp_batch_sa", BATCH_SA_LDS_BYTES, launch_args=_sa_launch_args),
    "ga": HeuristicKind(CVRP, "vrp_batch_ga", BATCH_GA_LDS_BYTES,
                        (Knob("random_permutation_count", 2, BATCH_GA_MAX_POP),
                         Knob("iteration_count", 0, BATCH_GA_MAX_GENERATIONS)), lds_knobs=1,
                        launch_args=lambda ctx, cis, pop, gens, pmut:
                        ((), (int(pop), int(gens), float(pmut)))),
    "aco": HeuristicKind(CVRP, "vrp_batch_aco", BATCH_ACO_LDS_BYTES,
                         (Knob("ants", 1, BATCH_ACO_MAX_ANTS),
                          Knob("iteration_count", 1, BATCH_ACO_MAX_ITERATIONS)), lds_knobs=1),
    "ls": HeuristicKind(CVRP, "vrp_batch_ls", BATCH_LS_LDS_BYTES,
                        _ls_knobs(BATCH_LS_MAX_STARTS, BATCH_LS_MAX_ROUNDS), strict=True),
    "lsr": HeuristicKind(CVRP, "vrp_batch_lsr", BATCH_LSR_LDS_BYTES,
                         _ls_knobs(BATCH_LSR_MAX_STARTS, BATCH_LSR_MAX_ROUNDS), strict=True,
                         separators=True, max_spread=BATCH_LSR_MAX_SPREAD),
    "lsf": HeuristicKind(CVRP, "vrp_batch_lsf", BATCH_LSF_LDS_BYTES,
                         _ls_knobs(BATCH_LSF_MAX_STARTS, BATCH_LSF_MAX_ROUNDS), strict=True,
                         separators=True, max_spread=BATCH_LSF_MAX_SPREAD, spread_always=False,
                         static_else="lsr"),
    "lso": HeuristicKind(TSP, "tsp_batch_lso", BATCH_LSO_LDS_BYTES,
                         _ls_knobs(BATCH_LSO_MAX_STARTS, BATCH_LSO_MAX_ROUNDS,
                                   Knob("moves", 1, 31, 31, "a move mask of {}..{}")), strict=True,
                         max_spread=BATCH_LSO_MAX_SPREAD, guard_empty=True),
}


def _domain_message(algorithm: str, ci: CompactInstance, knobs, empty_ok: bool = False):
    """The limit of the algorithm's domain this request fails -> its message,
    or None: the problem, the knobs' ranges, at least one customer (unless
    `empty_ok`) and at most 65534, 1..64 vehicles, a static or 24-slice matrix,
    the token limit of separator tours, and the LDS bytes of one request
    (uint16 cells unless an entry is above 65535).  Where a request outside
    the domain has another path the message is only a verdict.  Needs the
    library, no GPU."""
    kind = HEURISTIC_KINDS[algorithm]
    tsp = kind.problem == TSP
    what = f"{algorithm} (local search)" if kind.strict else algorithm
    if ci.problem != kind.problem:
        return f"{algorithm} solves the {'TSP' if tsp else 'VRP'} only"
    for k, v in zip(kind.knobs, knobs):
        if not k.lo <= int(v) <= k.hi:
            return f"{what} takes {k.takes.format(k.lo, k.hi)} ({v} given)"
    if ci.n < 1:
        return None if empty_ok else f"{what} needs at least one customer"
    if ci.N > 65535:
        return f"{what} supports at most 65534 customers ({ci.n} given)"
    N, K, H, wide = ci.N, 1 if tsp else len(ci.capacities), ci.durations.shape[0], batch_sa_wide(ci)
    if not 1 <= K <= BATCH_SA_MAX_VEHICLES:
        return f"{what} supports 1..{BATCH_SA_MAX_VEHICLES} vehicles ({K} given)"
    if H not in (1, 24):
        return f"{what} needs a static or 24-slice duration matrix ({H} slices given)"
    if kind.static_else and H != 1:
        return (f"{what} needs a static duration matrix ({H} slices given); an hour-indexed "
                f'request keeps "{kind.static_else}"')
    if kind.separators and N + K - 2 > 65535:
        return f"{what} supports at most 65535 tokens ({N + K - 2} given)"
    shape = (N, H, wide) if tsp else (N, K, H, wide)
    need = getattr(core, kind.kernel + "_lds")(*shape, *map(int, knobs[:kind.lds_knobs]))
    if need > kind.lds_bytes:
        held = f"matrix in LDS: {ci.n} customers" if tsp else \
            f"instance in LDS: {ci.n} customers, {K} vehicles"
        return (f"{what} keeps the {held} and {H} hour slice(s) of "
                f"{'int32' if wide else 'uint16'} cells need {need} bytes; the limit is "
                f"{kind.lds_bytes} bytes")
    return None


def _check_heuristic(algorithm: str, ci: CompactInstance, knobs):
    """solve_vrp's / solve_tsp's check where the launch is the only path: the
    domain's message first, then the int32 guards; no customer is inside."""
    msg = _domain_message(algorithm, ci, knobs, empty_ok=True)
    if msg is None and (ci.n or HEURISTIC_KINDS[algorithm].guard_empty):
        msg = batch_guard_message(ci)
    if msg is not None:
        raise ValueError(msg)


def check_range(algorithm: str, name: str, value, says: str = "") -> int:
    """int(value) where the table's range of the algorithm's knob `name` holds
    it, else a ValueError in the words of the batch entry points and of the
    service's batchers; `says` is the caller's word for the knob where that is
    not the table's."""
    k = next(k for k in HEURISTIC_KINDS[algorithm].knobs if k.name == name)
    if not k.lo <= int(value) <= k.hi:
        raise ValueError(f"{says or name} must be in {k.lo}..{k.hi} ({value} given)")
    return int(value)


def _check_spread(spread, cap: int):
    """-> None, "auto" or an int in 1..cap; anything else is a ValueError."""
    if spread is None or (isinstance(spread, str) and spread == "auto"):
        return spread
    if isinstance(spread, (int, np.integer)) and not isinstance(spread, bool) and \
            1 <= int(spread) <= cap:
        return int(spread)
    raise ValueError(f'spread must be None, "auto" or an integer in 1..{cap} ({spread!r} given)')


def _auto_spread(R: int, S: int, cus: int) -> int:
    """min(S, max(1, 16 cus // R)) workgroups per request."""
    return min(int(S), max(1, (16 * int(cus)) // max(int(R), 1)))


def _heuristic_launch(algorithm: str, ctx: Context, cis, knobs, seed: int, objective: str = "sum",
                      spread=None):
    """One upload and one launch of the algorithm's kernel -- of its spread
    form when `spread` says so -- for compact instances of one key -> the rows
    as lists: (tours, veh, durs) for a VRP, (tours, durs) for a TSP."""
    import torch
    kind = HEURISTIC_KINDS[algorithm]
    vrp = kind.problem == CVRP
    if kind.max_spread:
        spread = _check_spread(spread, kind.max_spread)
    bufs = _stage(ctx, cis, hours=True)
    st = [ci.start_times if vrp else int(ci.start_times[0]) for ci in cis]
    bufs.append(torch.from_numpy(np.array(st, dtype=np.int32)).to(ctx.dev))
    more, scalars = kind.launch_args(ctx, cis, *knobs) if kind.launch_args else \
        ((), [int(k) for k in knobs])
    if spread == "auto":
        spread = _auto_spread(len(cis), int(knobs[0]), ctx.cus)
        spread = None if spread == 1 else min(spread, kind.max_spread)
    method = getattr(ctx, kind.kernel if spread is None else kind.kernel + "_spread")
    out = method(*bufs, *more, *([OBJ_MAX if objective == "max" else OBJ_SUM] if vrp else []),
                 *scalars, seed, *([] if spread is None else [spread]), wide=batch_sa_wide(cis[0]))
    _check_contract(kind.kernel, out[1])
    rows = (out[0], out[3], out[2]) if vrp else (out[0], out[2])
    return tuple(t.cpu().tolist() for t in rows)


def batch_launch(algorithm: str, ctx, cis, knobs, seed, objective, spread):
    """batch_<algorithm>_launch as the module has it when called (a caller may
    have put its own there), with the arguments that one takes."""
    kind = HEURISTIC_KINDS[algorithm]
    args = tuple(knobs) + (seed,) + ((objective,) if kind.problem == CVRP else ())
    more = dict(spread=spread) if kind.max_spread and (kind.spread_always or spread is not None) \
        else {}
    return globals()[f"batch_{algorithm}_launch"](ctx, cis, *args, **more)


def _heuristic_result(ci: CompactInstance, row, with_unvisited: bool = False) -> dict:
    """The slot dict from one request's rows of a launch; for no customer
    (`row` None) the trivial one, built on the host."""
    if ci.problem == TSP:
        return tsp_result(ci, *(([], _td_duration(ci, [])) if row is None else row))
    return sa_result(ci, *(([], [], [0] * len(ci.capacities)) if row is None else row),
                     with_unvisited)


def _single_knobs(algorithm: str, ci: CompactInstance, knobs: dict):
    """solve_vrp's / solve_tsp's host side of a one-request launch: the knobs'
    values or their defaults, `spread` checked and kept in `knobs` only as a
    number, then _check_heuristic -> (values, spread)."""
    kind = HEURISTIC_KINDS[algorithm]
    values = tuple(k.default if knobs.get(k.name) is None else int(knobs[k.name])
                   for k in kind.knobs)
    spread = None
    if kind.max_spread:
        spread = _check_spread(knobs.get("spread"), kind.max_spread)
        if isinstance(spread, int):   # only a number travels to a GPU box as a knob
            knobs["spread"] = spread
        else:
            knobs.pop("spread", None)
    _check_heuristic(algorithm, ci, values)
    return values, spread


def _solve_single(algorithm: str, ci: CompactInstance, values, spread, seed, device,
                  objective=None, with_unvisited: bool = False) -> dict:
    """One checked request on a one-request launch; no customer on the host."""
    if ci.n == 0:
        return _heuristic_result(ci, None, with_unvisited)
    rows = batch_launch(algorithm, context(device), [ci], values, seed, objective, spread)
    return _heuristic_result(ci, [r[0] for r in rows], with_unvisited)


def _solve_heuristic_batch(algorithm: str, requests, knobs, seed, device, objective=None,
                           with_unvisited: bool = False, spread=None, launch_knobs=None) -> list:
    """The heuristics' batch entry points' one loop, after each has checked its
    own knobs: every request normalised, compacted and guarded on the host,
    and held against the domain where that is strict (a bad one raises with
    its index); with no local GPU each goes to the GPU box; else no customer is
    answered on the host, the requests inside the domain share one launch per
    key, and the rest take the single-request solver.  `knobs` are the
    table's, `launch_knobs` what the launch takes in their place."""
    kind = HEURISTIC_KINDS[algorithm]
    tsp = kind.problem == TSP
    request, compact, single = (_tsp_request, compact_tsp, solve_tsp) if tsp else \
        (_sp_request, compact_vrp, solve_vrp)
    reqs, cis = [], []
    for x, r in enumerate(requests):
        try:
            r, _ = request(r)
            ci = compact(*r)
            msg = batch_guard_message(ci)
            if msg is None and ci.n and kind.strict:
                msg = _domain_message(algorithm, ci, knobs)
            if msg is not None:
                raise ValueError(msg)
        except ValueError as e:
            raise ValueError(f"request {x}: {e}") from None
        reqs.append(r)
        cis.append(ci)
    shared = dict(seed=seed) if tsp else \
        dict(seed=seed, objective=objective, with_unvisited=with_unvisited)
    shared.update((k.name, int(v)) for k, v in zip(kind.knobs, knobs))
    if isinstance(spread, int):    # "auto" is the GPU box's own to decide
        shared["spread"] = spread
    if _remote() is not None:      # no local GPU: the GPU box answers each request
        return [single(algorithm, *r, **shared) for r in reqs]
    out = [None] * len(cis)
    groups: dict = {}
    key = globals()[f"batch_{algorithm}_key"]
    for x, ci in enumerate(cis):
        if ci.n == 0:
            out[x] = _heuristic_result(ci, None, with_unvisited)
        elif kind.strict or _domain_message(algorithm, ci, knobs) is None:
            groups.setdefault(key(ci, *knobs), []).append(x)
        else:
            out[x] = single(algorithm, *reqs[x], device=device, **shared)
    if groups:
        ctx = context(device)
        for xs in groups.values():
            rows = batch_launch(algorithm, ctx, [cis[x] for x in xs],
                                knobs if launch_knobs is None else launch_knobs, seed, objective,
                                spread)
            for x, *row in zip(xs, *rows):
                out[x] = _heuristic_result(cis[x], row, with_unvisited)
    return out


# ---------------------------------------------------------------------------
# batched VRP annealing (A22): small-fleet requests share launches
# ---------------------------------------------------------------------------
def batch_sa_wide(ci: CompactInstance) -> bool:
    """The request's matrix needs int32 cells in LDS (an entry above 65535)."""
    return bool(ci.durations.size) and int(ci.durations.max()) > 65535


def batch_sa_schedule(ci: CompactInstance, steps: int):
    """(inv_t0, inv_alpha) of a request's four chains: TspBatcher's constants
    -- a starting temperature of half the mean positive entry, cooled to 0.002
    of the mean over `steps` steps -- but from the request's own matrix (all
    hour slices; 1.0 when it has no positive entry), so the company a request
    rides with does not change its answer."""
    nz = ci.durations[ci.durations > 0]
    edge = float(nz.mean()) if nz.size else None
    return (1.0 / (0.5 * edge) if edge else 1.0), (0.5 / 0.002) ** (1.0 / max(1, int(steps)))


def batch_sa_key(ci: CompactInstance):
    """What the instances of one vrp_batch_sa launch share (next to the
    objective, the steps and the seed): (N, K, H, wide)."""
    return ci.N, len(ci.capacities), ci.durations.shape[0], batch_sa_wide(ci)


def batch_sa_fits(ci: CompactInstance) -> bool:
    """A22's LDS domain: a CVRP of at least one customer, 1..64 vehicles and a
    static or 24-slice matrix whose whole instance and twelve tours fit
    BATCH_SA_LDS_BYTES (vrpms_vrp_batch_sa_lds; uint16 cells unless an entry
    is above 65535).  Needs the library, no GPU."""
    return _domain_message("sa", ci, ()) is None


def batch_sa_launch(ctx: Context, cis, steps: int, seed: int, objective: str = "sum"):
    """One upload and one vrp_batch_sa launch for compact instances of one
    batch_sa_key (each passed batch_guard_message and batch_sa_fits), every
    request on its own batch_sa_schedule -> (tours, veh, durs): per instance
    the n + K - 1 tour tokens, each token's vehicle (-1 unvisited, -2 a
    separator) and the K route durations."""
    return _heuristic_launch("sa", ctx, cis, (steps,), seed, objective)


def sa_result(ci: CompactInstance, tour, veh, durs, with_unvisited: bool = False) -> dict:
    """solve_vrp's slot dict from a giant tour's tokens, each token's vehicle
    (-1 unvisited, -2 a separator: vrpms_decode's and vrp_batch_sa's) and the K
    route durations, compact indices mapped back through ci.nodes."""
    K = len(ci.capacities)
    routes = [[] for _ in range(K)]
    unvisited = []
    for c, v in zip(tour, veh):
        if v == -2:
            continue
        (routes[v] if v >= 0 else unvisited).append(ci.nodes[c])
    vehicles = [{"tour": [ci.nodes[0]] + r + [ci.nodes[0]], "duration": int(d)}
                for r, d in zip(routes, durs)]
    out = {"durationMax": int(max(durs) if len(durs) else 0), "durationSum": int(sum(durs)),
           "vehicles": vehicles}
    if with_unvisited:
        out["unvisited"] = unvisited
    return out


def solve_vrp_sa_batch(requests, *, steps: int = 2000, seed: int = 0, objective: str = "sum",
                       with_unvisited: bool = False, device: int = 0) -> list:
    """Simulated annealing for many small-fleet VRP requests, the requests
    that fit sharing launches (spec A22): one workgroup per request, its whole
    instance in LDS, four chains of `steps` steps.  `requests`:
    solve_vrp_batch's (durations, locations, capacities, start_times[,
    ignored_customers, completed_customers]) tuples, or dicts with those keys
    -> one solve_vrp slot dict per request.

    This is NOT solve_vrp("sa")'s answer: four chains with A13's one-word
    moves and a schedule from the request's own matrix (batch_sa_schedule)
    here, 1,024 chains there.  It is deterministic per request: the dict
    depends on the request, `steps`, `seed` and `objective` alone, not on the
    other requests of the call or on its place among them.

    Every request is compacted and passed through batch_guard_message on the
    host before any device is touched; a bad one raises ValueError("request
    {x}: ...").  With no local GPU each request goes to solve_vrp("sa") on the
    GPU box.  Requests inside the LDS domain (batch_sa_fits) are grouped by
    (N, K, H, wide), one upload and one vrp_batch_sa launch per group, and
    their dicts are built on the host from the tour tokens, their vehicles and
    the route durations; no customer has solve_vrp's trivial answer; a
    request outside the domain takes solve_vrp("sa", seed=seed,
    objective=objective), one by one."""
    if objective not in ("sum", "max"):
        raise ValueError("objective must be 'sum' or 'max'")
    if int(steps) < 0:
        raise ValueError("steps must not be negative")
    return _solve_heuristic_batch("sa", requests, (), seed, device, objective, with_unvisited,
                                  launch_knobs=(steps,))


# ---------------------------------------------------------------------------
# batched VRP GA (A23): small-fleet requests share launches
# ---------------------------------------------------------------------------
def batch_ga_key(ci: CompactInstance, pop: int, gens: int):
    """What the instances of one vrp_batch_ga launch share (next to the
    objective, pmut and the seed): (N, K, H, wide, pop, gens)."""
    return batch_sa_key(ci) + (int(pop), int(gens))


def batch_ga_fits(ci: CompactInstance, pop: int, gens: int) -> bool:
    """A23's domain: a CVRP of at least one customer, 1..64 vehicles, a static
    or 24-slice matrix, 2 <= pop <= BATCH_GA_MAX_POP, 0 <= gens <=
    BATCH_GA_MAX_GENERATIONS, and an instance that fits BATCH_GA_LDS_BYTES
    together with its 2 pop tours (vrpms_vrp_batch_ga_lds; uint16 cells unless
    an entry is above 65535).  Needs the library, no GPU."""
    return _domain_message("ga", ci, (pop, gens)) is None


def batch_ga_launch(ctx: Context, cis, pop: int, gens: int, pmut: float, seed: int,
                    objective: str = "sum"):
    """One upload and one vrp_batch_ga launch for compact instances of one
    batch_ga_key (each passed batch_guard_message and batch_ga_fits) ->
    (tours, veh, durs): per instance the n genes of the best member, each
    gene's vehicle (-1 unvisited) and the K route durations."""
    return _heuristic_launch("ga", ctx, cis, (pop, gens, pmut), seed, objective)


def ga_knobs(random_permutation_count=None, iteration_count=None):
    """(pop, gens) as solve_vrp("ga") takes a request's randomPermutationCount
    and iterationCount: 256 / 400 when falsy, pop clamped to 2..4096."""
    return max(2, min(int(random_permutation_count or 256), 4096)), int(iteration_count or 400)


def solve_vrp_ga_batch(requests, *, pop: int = 256, gens: int = 400, pmut: float = 0.2,
                       seed: int = 0, objective: str = "sum", with_unvisited: bool = False,
                       device: int = 0) -> list:
    """A genetic algorithm for many small-fleet VRP requests, the requests
    that fit sharing launches (spec A23): one workgroup per request, its whole
    instance and one population of `pop` separator-free tours in LDS, `gens`
    generations of tournament selection, OX1, a `pmut` mutation and (mu +
    lambda) survivors.  `requests`: solve_vrp_batch's (durations, locations,
    capacities, start_times[, ignored_customers, completed_customers]) tuples,
    or dicts with those keys -> one solve_vrp slot dict per request.

    This is NOT solve_vrp("ga")'s answer: one population with a Philox
    Fisher-Yates start here, 8 islands with migration and another start there.
    It is deterministic per request: the dict depends on the request, `pop`,
    `gens`, `pmut`, `seed` and `objective` alone, not on the other requests of
    the call or on its place among them.

    Every request is compacted and passed through batch_guard_message on the
    host before any device is touched; a bad one raises ValueError("request
    {x}: ...").  With no local GPU each request goes to solve_vrp("ga") on the
    GPU box.  Requests inside the domain (batch_ga_fits) are grouped by (N, K,
    H, wide), one upload and one vrp_batch_ga launch per group, and their
    dicts are built on the host from the genes, their vehicles and the route
    durations; no customer has solve_vrp's trivial answer; a request outside
    the domain (also every request when `pop` is above BATCH_GA_MAX_POP or
    `gens` above BATCH_GA_MAX_GENERATIONS) takes solve_vrp("ga", seed=seed,
    objective=objective, random_permutation_count=pop, iteration_count=gens),
    one by one."""
    if objective not in ("sum", "max"):
        raise ValueError("objective must be 'sum' or 'max'")
    if int(pop) < 2:
        raise ValueError("pop must be at least 2")
    if int(gens) < 0:
        raise ValueError("gens must not be negative")
    if not 0.0 <= float(pmut) <= 1.0:
        raise ValueError("pmut must be a probability")
    return _solve_heuristic_batch("ga", requests, (pop, gens), seed, device, objective,
                                  with_unvisited, launch_knobs=(pop, gens, pmut))


# ---------------------------------------------------------------------------
# batched VRP ACO (A24): small-fleet requests share launches
# ---------------------------------------------------------------------------
def batch_aco_key(ci: CompactInstance, ants: int, iters: int):
    """What the instances of one vrp_batch_aco launch share (next to the
    objective and the seed): (N, K, H, wide, ants, iters)."""
    return batch_sa_key(ci) + (int(ants), int(iters))


def batch_aco_fits(ci: CompactInstance, ants: int, iters: int) -> bool:
    """A24's domain: a CVRP of at least one customer, 1..64 vehicles, a static
    or 24-slice matrix, 1 <= ants <= BATCH_ACO_MAX_ANTS, 1 <= iters <=
    BATCH_ACO_MAX_ITERATIONS, and an instance that fits BATCH_ACO_LDS_BYTES
    together with its pheromone tables and ants + 1 tours
    (vrpms_vrp_batch_aco_lds; uint16 cells unless an entry is above 65535).
    Needs the library, no GPU."""
    return _domain_message("aco", ci, (ants, iters)) is None


def batch_aco_launch(ctx: Context, cis, ants: int, iters: int, seed: int, objective: str = "sum"):
    """One upload and one vrp_batch_aco launch for compact instances of one
    batch_aco_key (each passed batch_guard_message and batch_aco_fits), with
    ACORunner's pheromone parameters -> (tours, veh, durs): per instance the n
    customers of the best-so-far tour, each one's vehicle (-1 unvisited) and
    the K route durations."""
    return _heuristic_launch("aco", ctx, cis, (ants, iters), seed, objective)


def solve_vrp_aco_batch(requests, *, ants: int = 64, iters: int = 100, seed: int = 0,
                        objective: str = "sum", with_unvisited: bool = False,
                        device: int = 0) -> list:
    """An ant colony for many small-fleet VRP requests, the requests that fit
    sharing launches (spec A24): one workgroup per request, its whole
    instance, one colony's pheromone and `ants` separator-free tours in LDS,
    `iters` iterations of roulette construction, evaporation and an
    iteration-best (every fifth: best-so-far) deposit.  `requests`:
    solve_vrp_batch's (durations, locations, capacities, start_times[,
    ignored_customers, completed_customers]) tuples, or dicts with those keys
    -> one solve_vrp slot dict per request.

    This is NOT solve_vrp("aco")'s answer: one colony here (the trajectory of
    ACORunner(colonies=1, ants=ants)), 4 colonies there.  It is deterministic
    per request: the dict depends on the request, `ants`, `iters`, `seed` and
    `objective` alone, not on the other requests of the call or on its place
    among them.

    Every request is compacted and passed through batch_guard_message on the
    host before any device is touched; a bad one raises ValueError("request
    {x}: ...").  With no local GPU each request goes to solve_vrp("aco") on
    the GPU box.  Requests inside the domain (batch_aco_fits) are grouped by
    (N, K, H, wide), one upload and one vrp_batch_aco launch per group, and
    their dicts are built on the host from the tour, its vehicles and the
    route durations; no customer has solve_vrp's trivial answer; a request
    outside the domain (also every request when `ants` is above
    BATCH_ACO_MAX_ANTS or `iters` above BATCH_ACO_MAX_ITERATIONS) takes
    solve_vrp("aco", seed=seed, objective=objective, iteration_count=iters,
    ants=ants), one by one."""
    if objective not in ("sum", "max"):
        raise ValueError("objective must be 'sum' or 'max'")
    if int(ants) < 1:
        raise ValueError("ants must be at least 1")
    if int(iters) < 1:
        raise ValueError("iters must be at least 1")
    return _solve_heuristic_batch("aco", requests, (ants, iters), seed, device, objective,
                                  with_unvisited)


# ---------------------------------------------------------------------------
# batched VRP multi-start local search (A25): small-fleet requests share launches
# ---------------------------------------------------------------------------
def batch_ls_key(ci: CompactInstance, starts: int, rounds: int):
    """What the instances of one vrp_batch_ls launch share (next to the
    objective and the seed): (N, K, H, wide, starts, rounds)."""
    return batch_sa_key(ci) + (int(starts), int(rounds))


def batch_ls_message(ci: CompactInstance, starts: int, rounds: int):
    """The limit of A25's domain this request fails -> its message, or None:
    a CVRP of at least one customer and at most 65534, 1..64 vehicles, a static
    or 24-slice matrix, 1 <= starts <= BATCH_LS_MAX_STARTS, 0 <= rounds <=
    BATCH_LS_MAX_ROUNDS, and an instance that fits BATCH_LS_LDS_BYTES together
    with its eight tours (vrpms_vrp_batch_ls_lds; uint16 cells unless an entry
    is above 65535).  Needs the library, no GPU."""
    return _domain_message("ls", ci, (starts, rounds))


def batch_ls_fits(ci: CompactInstance, starts: int, rounds: int) -> bool:
    """The request is inside A25's domain (batch_ls_message names no limit).
    Needs the library, no GPU."""
    return batch_ls_message(ci, starts, rounds) is None


def _check_ls(ci: CompactInstance, starts, rounds):
    """A25's domain and the int32 guards, checked on the host before any device
    or remote is touched.  No customer is solve_vrp's trivial answer."""
    _check_heuristic("ls", ci, (starts, rounds))


def batch_ls_launch(ctx: Context, cis, starts: int, rounds: int, seed: int, objective: str = "sum"):
    """One upload and one vrp_batch_ls launch for compact instances of one
    batch_ls_key (each passed batch_guard_message and batch_ls_fits) ->
    (tours, veh, durs): per instance the n genes of the best end tour, each
    gene's vehicle (-1 unvisited) and the K route durations."""
    return _heuristic_launch("ls", ctx, cis, (starts, rounds), seed, objective)


def solve_vrp_ls_batch(requests, *, starts: int = 64, rounds: int = 1000, seed: int = 0,
                       objective: str = "sum", with_unvisited: bool = False,
                       device: int = 0) -> list:
    """A multi-start local search for many small-fleet VRP requests, the
    requests sharing launches (spec A25): one workgroup per request, its whole
    instance in LDS, `starts` steepest descents over swap, 2-opt and relocate
    from random separator-free tours, each stopped at a local optimum or after
    `rounds` applied moves; the least (key, start) end tour is the answer.
    `requests`: solve_vrp_batch's (durations, locations, capacities,
    start_times[, ignored_customers, completed_customers]) tuples, or dicts
    with those keys -> one solve_vrp slot dict per request.

    It is deterministic per request: the dict depends on the request,
    `starts`, `rounds`, `seed` and `objective` alone, not on the other requests
    of the call or on its place among them, and is solve_vrp("ls", starts=,
    rounds=)'s.

    Every request is compacted and passed through batch_guard_message and the
    domain (batch_ls_message) on the host before any device is touched.  There
    is no unbatched local search, so a request outside the domain raises
    ValueError("request {x}: ...") naming the limit that failed, as a bad one
    does.  With no local GPU each request goes to solve_vrp("ls") on the GPU
    box.  The requests are grouped by (N, K, H, wide), one upload and one
    vrp_batch_ls launch per group, and their dicts are built on the host from
    the genes, their vehicles and the route durations; no customer has
    solve_vrp's trivial answer."""
    if objective not in ("sum", "max"):
        raise ValueError("objective must be 'sum' or 'max'")
    check_range("ls", "starts", starts)
    check_range("ls", "rounds", rounds)
    return _solve_heuristic_batch("ls", requests, (starts, rounds), seed, device, objective,
                                  with_unvisited)


# ---------------------------------------------------------------------------
# batched TSP multi-start local search with Or-opt and delta pricing (A27)
# ---------------------------------------------------------------------------
def batch_lso_key(ci: CompactInstance, starts: int, rounds: int, moves: int = 31):
    """What the instances of one tsp_batch_lso launch share (next to the
    seed): (N, H, wide, starts, rounds, moves)."""
    return ci.N, ci.durations.shape[0], batch_sa_wide(ci), int(starts), int(rounds), int(moves)


def batch_lso_message(ci: CompactInstance, starts: int, rounds: int, moves: int = 31):
    """The limit of A27's domain this request fails -> its message, or None:
    a TSP of at least one customer and at most 65534, a static or 24-slice
    matrix, 1 <= starts <= BATCH_LSO_MAX_STARTS, 0 <= rounds <=
    BATCH_LSO_MAX_ROUNDS, 1 <= moves <= 31, and a matrix that fits
    BATCH_LSO_LDS_BYTES together with the wavefronts' tours and prefix rows
    (vrpms_tsp_batch_lso_lds; uint16 cells unless an entry is above 65535).
    Needs the library, no GPU."""
    return _domain_message("lso", ci, (starts, rounds, moves))


def batch_lso_fits(ci: CompactInstance, starts: int, rounds: int, moves: int = 31) -> bool:
    """The request is inside A27's domain (batch_lso_message names no limit).
    Needs the library, no GPU."""
    return batch_lso_message(ci, starts, rounds, moves) is None


def _check_lso(ci: CompactInstance, starts, rounds, moves):
    """A27's domain and the A9 guard, checked on the host before any device or
    remote is touched.  No customer is answered on the host."""
    _check_heuristic("lso", ci, (starts, rounds, moves))


def check_lso_spread(spread):
    """`spread` as batch_lso_launch takes it -> None, "auto" or an int in
    1..BATCH_LSO_MAX_SPREAD; anything else is a ValueError."""
    return _check_spread(spread, BATCH_LSO_MAX_SPREAD)


def batch_lso_spread(R: int, S: int, cus: int) -> int:
    """The "auto" policy: the workgroups per request that tsp_batch_lso_spread
    gives a launch of R requests of S starts on a device of `cus` compute
    units, min(S, max(1, 16 cus // R)): up to sixteen workgroups a CU while
    the requests are few.  1 means tsp_batch_lso itself, one workgroup per
    request.  The factor is the largest of 1, 2, 4, 8 and 16 measured (DESIGN
    §4.3t): at every launch size each step up was faster."""
    return _auto_spread(R, S, cus)


def batch_lso_launch(ctx: Context, cis, starts: int, rounds: int, moves: int, seed: int,
                     spread=None):
    """One upload and one tsp_batch_lso launch for compact instances of one
    batch_lso_key (each passed batch_guard_message and batch_lso_fits) ->
    (tours, durs): per instance the n customers of the best end tour and its
    duration.  `spread`: None -- the default -- is that launch; an int in
    1..BATCH_LSO_MAX_SPREAD takes tsp_batch_lso_spread at that many workgroups
    per request (1: one workgroup per request, its 256 threads on one descent
    at a time); "auto" takes batch_lso_spread's for the launch's size and the
    device, and tsp_batch_lso when that is 1.  The rows are the same whichever
    it is."""
    return _heuristic_launch("lso", ctx, cis, (starts, rounds, moves), seed, spread=spread)


def solve_tsp_lso_batch(requests, *, starts: int = 64, rounds: int = 1000, moves: int = 31,
                        seed: int = 0, device: int = 0, spread=None) -> list:
    """A multi-start local search for many TSP requests, the requests sharing
    launches (spec A27): one workgroup per request, its whole matrix (static
    or hour-indexed) in LDS, `starts` steepest descents from random tours over
    the move types `moves` enables (bit 0 swap, 1 2-opt, 2 relocate, 3 and 4
    Or-opt of two and three customers), every candidate priced by a delta
    instead of a tour walk, each descent stopped at a local optimum or after
    `rounds` applied moves; the least (key, start) end tour is the answer.
    `requests`: solve_tsp_batch's (durations, customers, start_node,
    start_time) tuples, or dicts with those keys -> one solve_tsp slot dict per
    request.

    It is deterministic per request: the dict depends on the request,
    `starts`, `rounds`, `moves` and `seed` alone, not on the other requests of
    the call or on its place among them, and is solve_tsp("lso", starts=,
    rounds=, moves=)'s.

    Every request is compacted and passed through batch_guard_message and the
    domain (batch_lso_message) on the host before any device is touched.  There
    is no unbatched form, so a request outside the domain raises
    ValueError("request {x}: ...") naming the limit that failed, as a bad one
    does.  With no local GPU each request goes to solve_tsp("lso") on the GPU
    box.  The requests are grouped by (N, H, wide, starts, rounds, moves), one
    upload and one tsp_batch_lso launch per group; no customer is answered on
    the host.  `spread` is batch_lso_launch's, applied to every group's launch:
    it changes which kernels run, never a dict."""
    spread = check_lso_spread(spread)
    check_range("lso", "starts", starts)
    check_range("lso", "rounds", rounds)
    check_range("lso", "moves", moves)
    return _solve_heuristic_batch("lso", requests, (starts, rounds, moves), seed, device,
                                  spread=spread)


# ---------------------------------------------------------------------------
# batched VRP multi-start local search over separator tours (A26): small-fleet
# requests share launches
# ---------------------------------------------------------------------------
def batch_lsr_key(ci: CompactInstance, starts: int, rounds: int):
    """What the instances of one vrp_batch_lsr launch share (next to the
    objective and the seed): (N, K, H, wide, starts, rounds)."""
    return batch_sa_key(ci) + (int(starts), int(rounds))


def batch_lsr_message(ci: CompactInstance, starts: int, rounds: int):
    """The limit of A26's domain this request fails -> its message, or None:
    a CVRP of at least one customer and at most 65534, 1..64 vehicles, a static
    or 24-slice matrix, 1 <= starts <= BATCH_LSR_MAX_STARTS, 0 <= rounds <=
    BATCH_LSR_MAX_ROUNDS, at most 65535 tokens (customers and K - 1 separators),
    and an instance that fits BATCH_LSR_LDS_BYTES together with its eight tours
    of tokens (vrpms_vrp_batch_lsr_lds; uint16 cells unless an entry is above
    65535).  Needs the library, no GPU."""
    return _domain_message("lsr", ci, (starts, rounds))


def batch_lsr_fits(ci: CompactInstance, starts: int, rounds: int) -> bool:
    """The request is inside A26's domain (batch_lsr_message names no limit).
    Needs the library, no GPU."""
    return batch_lsr_message(ci, starts, rounds) is None


def _check_lsr(ci: CompactInstance, starts, rounds):
    """A26's domain and the int32 guards, checked on the host before any device
    or remote is touched.  No customer is solve_vrp's trivial answer."""
    _check_heuristic("lsr", ci, (starts, rounds))


def check_lsr_spread(spread):
    """`spread` as batch_lsr_launch takes it -> None, "auto" or an int in
    1..BATCH_LSR_MAX_SPREAD; anything else is a ValueError."""
    return _check_spread(spread, BATCH_LSR_MAX_SPREAD)


def batch_lsr_spread(R: int, S: int, cus: int) -> int:
    """The "auto" policy: the workgroups per request that vrp_batch_lsr_spread
    gives a launch of R requests of S starts on a device of `cus` compute
    units, min(S, max(1, 16 cus // R)): up to sixteen workgroups a CU while
    the requests are few.  1 means vrp_batch_lsr itself, one workgroup per
    request.  The factor is the largest of 1, 2, 4, 8 and 16 measured (DESIGN
    §4.3r): at every launch size each step up was faster."""
    return _auto_spread(R, S, cus)


def batch_lsr_launch(ctx: Context, cis, starts: int, rounds: int, seed: int,
                     objective: str = "sum", spread=None):
    """One upload and one vrp_batch_lsr launch for compact instances of one
    batch_lsr_key (each passed batch_guard_message and batch_lsr_fits) ->
    (tours, veh, durs): per instance the n + K - 1 tokens of the best end tour
    (0 a separator), each token's vehicle (-1 unvisited, -2 a separator) and
    the K route durations.  `spread`: None -- the default -- is that launch;
    an int in 1..BATCH_LSR_MAX_SPREAD takes vrp_batch_lsr_spread at that many
    workgroups per request (1: one workgroup per request, its 256 threads on
    one descent at a time); "auto" takes batch_lsr_spread's for the launch's
    size and the device, and vrp_batch_lsr when that is 1.  The rows are the
    same whichever it is."""
    return _heuristic_launch("lsr", ctx, cis, (starts, rounds), seed, objective, spread)


def solve_vrp_lsr_batch(requests, *, starts: int = 64, rounds: int = 1000, seed: int = 0,
                        objective: str = "sum", with_unvisited: bool = False,
                        device: int = 0, spread=None) -> list:
    """A multi-start local search over separator tours for many small-fleet
    VRP requests, the requests sharing launches (spec A26): one workgroup per
    request, its whole instance in LDS, `starts` steepest descents over swap,
    2-opt and relocate on giant tours with K - 1 route separators, from random
    orders packed first-fit into the K routes, each stopped at a local optimum
    or after `rounds` applied moves; the least (key, start) end tour is the
    answer.
    `requests`: solve_vrp_batch's (durations, locations, capacities,
    start_times[, ignored_customers, completed_customers]) tuples, or dicts
    with those keys -> one solve_vrp slot dict per request.

    It is deterministic per request: the dict depends on the request,
    `starts`, `rounds`, `seed` and `objective` alone, not on the other requests
    of the call or on its place among them, and is solve_vrp("lsr", starts=,
    rounds=)'s.

    Every request is compacted and passed through batch_guard_message and the
    domain (batch_lsr_message) on the host before any device is touched.  There
    is no unbatched local search, so a request outside the domain raises
    ValueError("request {x}: ...") naming the limit that failed, as a bad one
    does.  With no local GPU each request goes to solve_vrp("lsr") on the GPU
    box.  The requests are grouped by (N, K, H, wide), one upload and one
    vrp_batch_lsr launch per group, and their dicts are built on the host from
    the tokens, their vehicles and the route durations; no customer has
    solve_vrp's trivial answer.  `spread` is batch_lsr_launch's, applied to
    every group's launch: it changes which kernels run, never a dict."""
    if objective not in ("sum", "max"):
        raise ValueError("objective must be 'sum' or 'max'")
    spread = check_lsr_spread(spread)
    check_range("lsr", "starts", starts)
    check_range("lsr", "rounds", rounds)
    return _solve_heuristic_batch("lsr", requests, (starts, rounds), seed, device, objective,
                                  with_unvisited, spread)


# ---------------------------------------------------------------------------
# batched VRP multi-start local search over plain separator tours with delta
# pricing (A28): static small-fleet requests share launches
# ---------------------------------------------------------------------------
def batch_lsf_key(ci: CompactInstance, starts: int, rounds: int):
    """What the instances of one vrp_batch_lsf launch share (next to the
    objective and the seed): (N, K, H, wide, starts, rounds), H being 1."""
    return batch_sa_key(ci) + (int(starts), int(rounds))


def batch_lsf_message(ci: CompactInstance, starts: int, rounds: int):
    """The limit of A28's domain this request fails -> its message, or None:
    a CVRP of at least one customer and at most 65534, 1..64 vehicles, a static
    matrix (an hour-indexed request is told to keep "lsr"), 1 <= starts <=
    BATCH_LSF_MAX_STARTS, 0 <= rounds <= BATCH_LSF_MAX_ROUNDS, at most 65535
    tokens, and an instance that fits BATCH_LSF_LDS_BYTES together with the
    wavefronts' tours, prefix rows and route tables (vrpms_vrp_batch_lsf_lds;
    uint16 cells unless an entry is above 65535).  Needs the library, no
    GPU."""
    return _domain_message("lsf", ci, (starts, rounds))


def batch_lsf_fits(ci: CompactInstance, starts: int, rounds: int) -> bool:
    """The request is inside A28's domain (batch_lsf_message names no limit).
    Needs the library, no GPU."""
    return batch_lsf_message(ci, starts, rounds) is None


def check_lsf_spread(spread):
    """`spread` as batch_lsf_launch takes it -> None, "auto" or an int in
    1..BATCH_LSF_MAX_SPREAD; anything else is a ValueError."""
    return _check_spread(spread, BATCH_LSF_MAX_SPREAD)


def batch_lsf_spread(R: int, S: int, cus: int) -> int:
    """The "auto" policy: the workgroups per request that vrp_batch_lsf_spread
    gives a launch of R requests of S starts on a device of `cus` compute
    units, min(S, max(1, 16 cus // R)), batch_lsr_spread's.  1 means
    vrp_batch_lsf itself, one workgroup per request.  DESIGN §4.3x has what
    was measured of the factor for this kernel."""
    return _auto_spread(R, S, cus)


def batch_lsf_launch(ctx: Context, cis, starts: int, rounds: int, seed: int,
                     objective: str = "sum", spread=None):
    """One upload and one vrp_batch_lsf launch for compact instances of one
    batch_lsf_key (each passed batch_guard_message and batch_lsf_fits) ->
    (tours, veh, durs), as batch_lsr_launch gives them.  `spread`: None -- the
    default -- is that launch; an int in 1..BATCH_LSF_MAX_SPREAD takes
    vrp_batch_lsf_spread at that many workgroups per request (1: one workgroup
    per request, its 256 threads on one descent at a time); "auto" takes
    batch_lsf_spread's for the launch's size and the device, and vrp_batch_lsf
    when that is 1.  The rows are the same whichever it is."""
    return _heuristic_launch("lsf", ctx, cis, (starts, rounds), seed, objective, spread)


def solve_vrp_lsf_batch(requests, *, starts: int = 64, rounds: int = 1000, seed: int = 0,
                        objective: str = "sum", with_unvisited: bool = False,
                        device: int = 0, spread=None) -> list:
    """A multi-start local search over plain separator tours for many static
    small-fleet VRP requests, the requests sharing launches (spec A28):
    solve_vrp_lsr_batch's mapping, starts, moves and answer, but a move onto a
    tour in which some customer would not fit the route its separators give it
    is no candidate, a start of that kind does not descend, and a candidate is
    priced from prefix rows instead of a walk along the tour.  Where every
    vehicle carries the whole demand the dicts are solve_vrp_lsr_batch's.
    `requests`: solve_vrp_batch's tuples or dicts -> one solve_vrp slot dict per
    request, solve_vrp("lsf", starts=, rounds=)'s.

    Every request is compacted and passed through batch_guard_message and the
    domain (batch_lsf_message) on the host before any device is touched; one
    outside it raises ValueError("request {x}: ...") naming the limit that
    failed -- for an hour-indexed matrix, that "lsr" takes it.  With no local
    GPU each request goes to solve_vrp("lsf") on the GPU box.  The requests
    are grouped by (N, K, wide), one upload and one vrp_batch_lsf launch per
    group; no customer has solve_vrp's trivial answer.  `spread` is
    batch_lsf_launch's, applied to every group's launch: it changes which
    kernels run, never a dict."""
    if objective not in ("sum", "max"):
        raise ValueError("objective must be 'sum' or 'max'")
    spread = check_lsf_spread(spread)
    check_range("lsf", "starts", starts)
    check_range("lsf", "rounds", rounds)
    return _solve_heuristic_batch("lsf", requests, (starts, rounds), seed, device, objective,
                                  with_unvisited, spread)


# ---------------------------------------------------------------------------
# reference entry points (src/solver.py)
# ---------------------------------------------------------------------------
_LOOKUP = None


def set_duration_matrix(durations, location_ids=None):
    """Back calculate_duration with a loaded matrix."""
    global _LOOKUP
    D = _matrix(durations)
    ids = list(location_ids) if location_ids is not None else list(range(D.shape[1]))
    _LOOKUP = (D, {v: i for i, v in enumerate(ids)})


def calculate_duration(source, target, time_of_day: int = 0):
    """src/solver.py:7-15 signature and return dict.  With a matrix loaded
    (set_duration_matrix) this is the A3 lookup D[(t // 60) % H][s][t];
    without one it keeps the reference's stub behaviour (randint(3, 320))."""
    if _LOOKUP is None:
        duration = random.randint(3, 320)
    else:
        D, index = _LOOKUP
        h = (int(time_of_day) // 60) % D.shape[0]
        duration = int(D[h, index[source], index[target]])
    return {"source": source, "target": target, "duration": duration, "units": "minutes"}


def get_current_date():
    """src/utilities/helper.py:4-6."""
    return datetime.date.today().strftime("%d-%m-%Y")


def solve_vrp_problem(durations=None, locations=None, capacities=None, start_times=None,
                      ignored_customers=(), completed_customers=(), algorithm: str = "sa",
                      seed: int | None = None, **knobs):
    """src/solver.py:18-27 return shape: {'tour','total_time','unvisited','date'}.

    With no instance (the reference's no-argument call from main.py) a
    random symmetric 15-node matrix (randint(3, 320), src/solver.py:12) is
    solved as a single-vehicle tour over customers 1..14 (src/solver.py:22-24).
    `tour` concatenates the vehicle routes; `total_time` is durationSum."""
    if durations is None:
        rng = random.Random(seed)
        N = 15
        D = np.zeros((N, N), dtype=np.int64)
        for i in range(N):
            for j in range(i + 1, N):
                D[i, j] = D[j, i] = rng.randint(3, 320)
        durations = D
        locations = [{"id": i} for i in range(N)]
        capacities = [N]
        start_times = [0]
    res = solve_vrp(algorithm, durations, locations, capacities, start_times, ignored_customers,
                    completed_customers, seed=seed or 0, with_unvisited=True, **knobs)
    depot = res["vehicles"][0]["tour"][0] if res["vehicles"] else 0
    tour = [depot]
    for v in res["vehicles"]:
        if len(v["tour"]) > 2:
            tour += v["tour"][1:]          # route customers, back to the depot
    if len(tour) == 1:
        tour.append(depot)
    return {"tour": tour, "total_time": res["durationSum"], "unvisited": res["unvisited"],
            "date": get_current_date()}


__all__ = ["ALGORITHMS", "calculate_duration", "solve_vrp_problem", "solve_tsp", "solve_vrp",
           "compact_tsp", "compact_vrp", "active_customers", "set_duration_matrix",
           "get_current_date"]
