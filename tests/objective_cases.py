"""Cases for the max-duration objective (spec A8, objective 1) on the search
path every non-batched VRP request takes: the five SA kernels, both ACO
constructions and update paths, both GA paths and bf_kernel.

Under objective 1 a tour's key is unv << 56 | min(max, 2^28 - 1) << 28 |
min(sum, 2^28 - 1): the longest route is the primary field.  The kernels read
the objective only in cvrp_key, so every case here is an instance, a start and
a set of knobs at which the C / Python oracle's answer under objective 1
differs from its answer under objective 0.  test_objective_cases_cpu.py proves
that without a GPU; test_objective_max_gpu.py compares the device with the
oracle under objective 1 for equality.

Plain test data; every instance is built once and shared, never modified.
The instance helpers are the existing GPU files' (imported, not restated).
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
from dataclasses import dataclass

import numpy as np

from oracle import spec
from test_hours_gpu import with_hours
from test_sa_td_gpu import _starts as _td_starts
from test_sa_td_gpu import _tight, starts
from test_separators_gpu import _asym, _classes, _starts
from vrpms_amd import synth

OBJ_MAX = spec.OBJ_MAX

# ---------------------------------------------------------------------------
# 1. SA: one small case per kernel and variant
# ---------------------------------------------------------------------------
CHAINS, SEED, STEP0, INV_ALPHA = 8, 21, 7, 1 / 0.99
COLD, HOT = 1 / 200.0, 1e-7


@dataclass(frozen=True)
class SaCase:
    name: str
    maker: object               # () -> synth.Instance
    start: str                  # "pack": first-fit separators, "random": random ones
    steps: int
    window: int
    types: int
    moves: int
    modes: tuple                # forced VRPMS_OPT_SA_ROUTE values that apply besides auto
    hot: bool                   # also run at inv_t0 = 1e-7 (every step accepted)
    expect: dict                # vrpms_instance_layout fields that decide the dispatch
    split2: bool = False        # also with VRPMS_OPT_SPLIT_MODE = 2 (no fast split)

    @property
    def temps(self):
        return (COLD, HOT) if self.hot else (COLD,)


def _h2(inst):
    """An hour-indexed instance cut to two slices (the morning peak's), as
    test_hours_gpu.py does: neither H = 1 nor H = 24."""
    return with_hours(inst, 2, first=7)


# Which kernel the automatic dispatch (VRPMS_OPT_SA_ROUTE = 0) reaches, from
# vrpms_sa_run (search.hip), launch_sa_seg (sa_seg.hip) and launch_sa_td
# (sa_td.hip), is written above each case.  Forced modes: 2 = sa_kernel (one
# wavefront per chain only, so moves = 64), 3 = sa_route_kernel when it applies
# (window > 0, every demand fits the smallest vehicle; else sa_kernel), 4 =
# sa_td_kernel (H = 24, u16).
SA_CASES = [
    # sa_packed_kernel: moves = 64, H = 1 and fast_split_params holds (N <= 128, one
    # capacity, packed fields fit) -- the first branch of vrpms_sa_run, taken before
    # VRPMS_OPT_SA_ROUTE is read, so no forced mode changes it.  With
    # VRPMS_OPT_SPLIT_MODE = 2 the fast split is off and the same chains reach
    # sa_seg_kernel (auto: static symmetric), sa_kernel (2) and, windowed,
    # sa_route_kernel (3): the smallest instance on which those three run.
    SaCase("packed_w0", lambda: synth.cvrp(40, 5, seed=1), "pack", 80, 0, 0, 64, (), False,
           dict(fast=True, symmetric=True, uniform_cap=True), split2=True),
    SaCase("packed_w12", lambda: synth.cvrp(40, 5, seed=2), "pack", 80, 12, 2, 64, (), False,
           dict(fast=True, symmetric=True, uniform_cap=True), split2=True),
    # the same kernel from an infeasible start (random separators leave customers
    # unserved): unv > 0 dominates both duration fields until the chain repairs it
    SaCase("packed_infeasible", lambda: synth.cvrp(40, 5, seed=3), "random", 80, 12, 2, 64, (),
           False, dict(fast=True, symmetric=True, uniform_cap=True), split2=True),
    # sa_seg_kernel<u16, !HET>: N = 141 > 128, so there is no packed matrix and
    # fast_split_params fails; launch_sa_seg accepts (CVRP, H = 1, symmetric, every
    # demand fits).  8 chains x W <= 8 x CUs, so W = moves / 64.
    SaCase("seg_uniform", lambda: synth.cvrp(140, 10, seed=4), "pack", 80, 12, 2, 64, (2, 3), True,
           dict(fast=False, symmetric=True, uniform_cap=True, flex=False)),
    # ... with two wavefronts per chain (W = 2, one move per lane)
    SaCase("seg_uniform_m128", lambda: synth.cvrp(140, 10, seed=5), "pack", 80, 12, 2, 128, (3,),
           True, dict(fast=False, symmetric=True, uniform_cap=True, flex=False)),
    # sa_seg_kernel<u16, HET>: per-vehicle capacities, every demand fits the smallest
    SaCase("seg_het", lambda: _classes(synth.cvrp(140, 10, seed=6), (1.3, 1.0, 0.8)), "pack", 80,
           12, 2, 64, (2, 3), True,
           dict(fast=False, symmetric=True, uniform_cap=False, flex=False)),
    # sa_route_kernel<u16, 1>: asymmetric static matrix, so launch_sa_seg declines
    # (!symmetric) and launch_sa_td declines (H != 24); windowed, one capacity, one
    # start time -> RouteK, four chains per workgroup
    SaCase("route_uniform", lambda: _asym(synth.cvrp(140, 10, seed=7), 1), "pack", 80, 12, 2, 64,
           (2, 3), True, dict(fast=False, symmetric=False, uniform_cap=True, flex=False)),
    # ... with two wavefronts per chain (one chain per workgroup)
    SaCase("route_uniform_m128", lambda: _asym(synth.cvrp(140, 10, seed=8), 2), "pack", 80, 12, 2,
           128, (3,), True, dict(fast=False, symmetric=False, uniform_cap=True, flex=False)),
    # sa_route_kernel<u16, 1, HV>: capacity classes and staggered start times
    SaCase("route_hv", lambda: _starts(_classes(_asym(synth.cvrp(140, 10, seed=9), 3),
                                                (1.3, 1.0, 0.8))), "pack", 80, 12, 2, 64, (2, 3),
           True, dict(fast=False, symmetric=False, uniform_cap=False, flex=False)),
    # sa_route_kernel<u16, HM = 0, HV>: two hour slices, so launch_sa_seg declines
    # (H != 1), launch_sa_td declines (H != 24) and td_full_walk (H == 24) is false
    SaCase("route_hv_hours", lambda: _td_starts(_classes(_h2(synth.td_cvrp(60, 6, seed=10)),
                                                         (1.3, 1.0, 0.8))), "pack", 80, 12, 2, 64,
           (2, 3), True, dict(hour_minor=False, uniform_cap=False, flex=False)),
    # sa_td_kernel<CVRP, FAST>: H = 24 with a u16 matrix (the hour-minor copy exists),
    # 65 tokens fit the LDS, every demand fits every vehicle.  Mode 3 is
    # sa_route_kernel<u16, 24>.
    SaCase("td_fast", lambda: synth.td_cvrp(60, 6, seed=11), "pack", 80, 12, 2, 64, (2, 3, 4), True,
           dict(hour_minor=True, uniform_cap=True, flex=False)),
    # ... per-vehicle capacities and start times (auto stays sa_td_kernel: the uniform
    # long-tour exception needs n > 480); mode 3 is sa_route_kernel<u16, 24, HV>
    SaCase("td_fast_het", lambda: _td_starts(_classes(synth.td_cvrp(60, 6, seed=12),
                                                      (1.3, 1.0, 0.8))), "pack", 80, 12, 2, 64,
           (2, 3, 4), True, dict(hour_minor=True, uniform_cap=False, flex=False)),
    # ... two wavefronts per chain (W = 2 <= kTdMaxWaves)
    SaCase("td_fast_het_m128", lambda: _td_starts(_classes(synth.td_cvrp(60, 6, seed=13),
                                                           (1.3, 1.0, 0.8))), "pack", 80, 12, 2,
           128, (3, 4), True, dict(hour_minor=True, uniform_cap=False, flex=False)),
    # sa_td_kernel<CVRP, !FAST>: the smallest vehicle is below the largest demand
    # (max_dem > min_cap), so the walk takes its per-token capacity branch; the route
    # kernel does not apply, mode 3 falls through to sa_kernel like mode 2
    SaCase("td_tight", lambda: _td_starts(_tight(synth.td_cvrp(60, 6, seed=14), (1.3, 1.0))),
           "pack", 80, 12, 2, 64, (2, 4), True,
           dict(hour_minor=True, uniform_cap=False, flex=True)),
    # sa_kernel<u16, HM = 0, CVRP>: H = 2 (no segment, no hour-row kernel) and window 0
    # (no route kernel): a shape no other kernel takes; mode 2 is the same kernel
    SaCase("sa_kernel_h2", lambda: _h2(synth.td_cvrp(20, 3, seed=15)), "pack", 80, 0, 0, 64, (2,),
           False, dict(hour_minor=False, fast=False)),
]
SA_BY_NAME = {c.name: c for c in SA_CASES}


@functools.lru_cache(maxsize=None)
def sa_case(name):
    """(case, instance, start tours uint16 [CHAINS][n + K - 1])."""
    c = SA_BY_NAME[name]
    inst = c.maker()
    return c, inst, starts(None, inst, c.start, CHAINS)


def oracle_sa(coracle, inst, P, steps, inv_t0, window, types, moves, objective, resync=False,
              inv_alpha=INV_ALPHA, seed=SEED, step0=STEP0):
    """coracle.sa_run from P -> (cur, cur_key, best, best_key)."""
    cur, best = P.copy(), P.copy()
    bk = np.full(P.shape[0], 2**64 - 1, dtype=np.uint64)
    ck = coracle.sa_run(inst.durations, cur, best, bk, steps, inv_t0, inv_alpha, seed, step0,
                        inst.demand, inst.capacities, inst.start_times,
                        problem=0 if inst.problem == "tsp" else 1, objective=objective,
                        window=window, window_types=types, resync=resync, moves=moves)
    return cur, [int(x) for x in ck], best, [int(x) for x in bk]


@functools.lru_cache(maxsize=None)
def sa_reference(name, inv_t0, objective=OBJ_MAX):
    """The C oracle's run of a case; computed once, shared by the tests."""
    from oracle import coracle
    coracle.build()
    c, inst, P = sa_case(name)
    return oracle_sa(coracle, inst, P, c.steps, inv_t0, c.window, c.types, c.moves, objective)


# ---------------------------------------------------------------------------
# 2. The secondary field saturated, the primary not
# ---------------------------------------------------------------------------
SAT_CHAINS, SAT_STEPS, SAT_INV_T0 = 4, 40, 1 / 2.0e6


@functools.lru_cache(maxsize=None)
def saturated():
    """N = 6 (5 customers), K = 3, every demand 1, every capacity 2, symmetric
    durations in [40,000,000, 50,000,000].  A route serves at most 2 customers
    (3 edges, at most 1.5e8 < 2^28 - 1 = 268,435,455); a tour that serves all
    five needs the routes 2 + 2 + 1 (8 edges, at least 3.2e8 > 2^28 - 1).
    start + (N + K + 1) * max_dur <= 5e8 < 2^31 passes the A9 guard; the
    entries force the int32 matrix.  Static and symmetric, so launch_sa_seg
    takes it (sa_seg_kernel<int32>) and mode 2 is sa_kernel<int32>."""
    rng = np.random.default_rng(28)
    N, K = 6, 3
    D = rng.integers(40_000_000, 50_000_001, size=(N, N), dtype=np.int64)
    D = np.triu(D, 1)
    D = D + D.T
    dem = np.array([0] + [1] * (N - 1), dtype=np.int64)
    return synth.Instance("saturated", D[None], dem, np.full(K, 2, dtype=np.int64),
                          np.zeros(K, dtype=np.int64), "cvrp")


@functools.lru_cache(maxsize=None)
def saturated_tours():
    """All 120 orders of the five customers with first-fit separators, uint8
    rows of 7 tokens padded to 8; the SA chains start from rows 0, 37, 74, 111."""
    inst = saturated()
    rows = [spec.pack_separators(list(p), inst.K - 1, inst.demand, inst.capacities)
            for p in itertools.permutations(range(1, inst.N))]
    P = np.zeros((len(rows), 8), dtype=np.uint8)
    P[:, :7] = rows
    return P


def saturated_starts():
    return saturated_tours()[::37, :7].astype(np.uint16)


# ---------------------------------------------------------------------------
# 3. ACO: 1 colony, 8 ants, 2 iterations
# ---------------------------------------------------------------------------
ACO_COLONIES, ACO_ANTS, ACO_ITERS, ACO_SEED, ACO_TAU0 = 1, 8, 2, 13, 1 << 20
ACO_CASES = {
    # N = 41 <= 140: the LDS-staged construction (and, forced, the L2 one); N <= 256:
    # the fused evaporate / deposit / track-best update
    "cvrp40": dict(maker=lambda: synth.cvrp(40, 5, seed=1), bsf_period=0, inject=False,
                   modes=(0, 2)),
    # the best-so-far deposits on iteration 1 ((it + 1) % 2 == 0): an injected
    # nearest-neighbour tour that the max-first key ranks before every ant, so it
    # deposits 2^30 / (1 + its longest route) instead of the iteration best
    "cvrp100_bsf": dict(maker=lambda: synth.cvrp(100, 8, seed=0), bsf_period=2, inject=True,
                        modes=(0,)),
    # N = 261 > 256: segment_argmin, aco_track_best, aco_evaporate and aco_deposit as
    # separate kernels (the L2 construction; nothing is staged).  The best-so-far
    # starts empty, so aco_track_best writes it from the ants by the max-first key
    # and it deposits on iteration 1
    "cvrp260": dict(maker=lambda: synth.cvrp(260, 16, seed=5), bsf_period=2, inject=False,
                    modes=(0,)),
}


@functools.lru_cache(maxsize=None)
def aco_instance(name):
    return ACO_CASES[name]["maker"]()


def nearest_neighbour(inst):
    """The greedy nearest-neighbour order from the depot (ties to the smaller
    index): the injected best-so-far of the bsf cases."""
    D0 = inst.durations[0]
    cur, left, nn = 0, set(range(1, inst.N)), []
    while left:
        cur = min(left, key=lambda c: (D0[cur, c], c))
        nn.append(cur)
        left.remove(cur)
    return nn


@functools.lru_cache(maxsize=None)
def aco_reference(name, objective=OBJ_MAX):
    """oracle/search.py aco_iteration, ACO_ITERS iterations -> per iteration
    (tours, keys, iteration bests, tau, best-so-far tours, best-so-far keys)."""
    from oracle import search
    inst = aco_instance(name)
    bsf = ACO_CASES[name]["bsf_period"]
    sc = search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times,
                       inst.problem, objective)
    eta = search.aco_eta(inst.durations[0])
    tau = [np.full((inst.N, inst.N), ACO_TAU0, dtype=np.int64) for _ in range(ACO_COLONIES)]
    best = aco_best_start(name, objective)
    out = []
    for it in range(ACO_ITERS):
        rt, rk, rib = search.aco_iteration(sc, tau, eta, ACO_ANTS, inst.n, ACO_SEED, it, 3,
                                           1 << 10, 1 << 30, best=best, bsf_period=bsf)
        out.append((rt, [k for ks in rk for k in ks], rib, [t.copy() for t in tau],
                    [list(t) for t in best[0]], list(best[1])))
    return out


def aco_best_start(name, objective=OBJ_MAX):
    """The best-so-far the colony starts with, [tours, keys]: the injected
    nearest-neighbour tour (a migrant-like tour that beats the first ants), or
    empty (zeros, the all-ones key)."""
    from oracle import search
    inst = aco_instance(name)
    if not ACO_CASES[name]["inject"]:
        return [[[0] * inst.n], [2**64 - 1]]
    nn = nearest_neighbour(inst)
    sc = search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times,
                       inst.problem, objective)
    return [[list(nn)], [sc(nn)]]


# ---------------------------------------------------------------------------
# 4. GA and brute force
# ---------------------------------------------------------------------------
GA_ISLANDS, GA_POP, GA_GENS, GA_PMUT, GA_SEED, GA_GEN0 = 2, 64, 3, 0.3, 47, 3
GA_CASES = {
    # the fused one-workgroup-per-island kernel (packed layout) and, forced, the
    # breed / eval_cvrp_words2 / select launches
    "cvrp40": dict(maker=lambda: synth.cvrp(40, 5, seed=1), modes=(0, 2)),
    # H = 24: no packed layout, so launch_ga_fused declines and the three kernels score
    # 2-byte children with vrpms_eval (the non-words path) in either mode
    "td20": dict(maker=lambda: synth.td_cvrp(20, 3, seed=2), modes=(0, 2)),
}


@functools.lru_cache(maxsize=None)
def ga_case(name):
    inst = GA_CASES[name]["maker"]()
    P = synth.random_perms(GA_ISLANDS * GA_POP, inst.n, seed=GA_POP).astype(np.int16)
    return inst, P.reshape(GA_ISLANDS, GA_POP, inst.n)


@functools.lru_cache(maxsize=None)
def ga_reference(name, objective=OBJ_MAX):
    """oracle/search.py ga_generation, GA_GENS generations -> (initial keys,
    populations, keys)."""
    from oracle import search
    inst, P = ga_case(name)
    sc = search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times,
                       inst.problem, objective)
    pops = [[list(int(x) for x in r) for r in P[i]] for i in range(GA_ISLANDS)]
    keys = [[sc(t) for t in pops[i]] for i in range(GA_ISLANDS)]
    k0 = [k for ks in keys for k in ks]
    pm = min(int(round(GA_PMUT * 2**32)), 2**32 - 1)
    for g in range(GA_GENS):
        pops, keys = search.ga_generation(sc, pops, keys, GA_SEED, GA_GEN0 + g, pm)
    return k0, pops, [k for ks in keys for k in ks]


# instance seeds chosen so that the optimum tour under objective 1 is not the
# optimum tour under objective 0 (test_objective_cases_cpu.py asserts it)
BF_CASES = {
    "cvrp8": lambda: synth.cvrp(8, 3, seed=1),
    "td7": lambda: synth.td_cvrp(7, 3, seed=1),
}


@functools.lru_cache(maxsize=None)
def bf_instance(name):
    return BF_CASES[name]()


def bf_windows(n):
    """The whole rank range and two unequal windows that cover it."""
    import math
    full = math.factorial(n)
    cut = full // 3 + 11
    return [(0, full), (0, cut), (cut, full)]


def bf_kw(inst):
    if inst.problem == "tsp":
        return dict(start_times=inst.start_times, problem=0)
    return dict(demand=inst.demand, capacities=inst.capacities, start_times=inst.start_times)


def tsp_instance():
    """A static 9-customer TSP: its A8 key is duration << 28 under either
    objective."""
    D = synth.tsp20(7).durations[:, :10, :10]
    return synth.Instance("tsp9", D, None, None, np.array([30]), "tsp")


# ---------------------------------------------------------------------------
# 5. The front door: solve_vrp(..., objective="max")
# ---------------------------------------------------------------------------
FRONT_KNOBS = {"sa": {"chains": 64, "steps": 300}, "ga": {"pop": 32, "iteration_count": 20},
               "aco": {"ants": 16, "iteration_count": 10}, "bf": {}}
FRONT_SEED = 3


@functools.lru_cache(maxsize=None)
def front(kind):
    """7 customers, 3 vehicles of capacity 10, demands that add up to 30:
    every solution that serves all seven fills every vehicle exactly, so the
    greedy split of its routes' concatenation closes each route where the
    solution does.  Brute force over the 7! giant tours therefore covers every
    such solution -- also those SA reaches through its K - 1 separators -- and
    its optimum bounds every heuristic's from below.  "static": one matrix,
    one start time; "td": 24 hourly matrices, per-vehicle start times.  The
    generator seed is one at which the two objectives' optimum tours differ."""
    base = synth.cvrp(7, 3, seed=4) if kind == "static" else synth.td_cvrp(7, 3, seed=4)
    dem = np.array([0, 4, 3, 3, 5, 5, 6, 4], dtype=np.int64)
    st = np.zeros(3, dtype=np.int64) if kind == "static" else np.array([470, 495, 530])
    return dataclasses.replace(base, demand=dem, capacities=np.full(3, 10, dtype=np.int64),
                               start_times=st)


def front_args(inst):
    """solve_vrp's positional arguments for an instance."""
    D = inst.durations[0] if inst.H == 1 else inst.durations
    locs = [{"id": i, "demand": int(inst.demand[i])} for i in range(inst.N)]
    return D.tolist(), locs, inst.capacities.tolist(), inst.start_times.tolist()
