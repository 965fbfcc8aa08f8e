"""Inputs for the ordered-selection tests: the GA's (mu + lambda) survivors
(ga_fused.hip, ga_select_kernel in search.hip, sort.hpp) and the pool / island
top-E (pool.hip), at the sizes where the code takes another path.

Plain test data, shared by test_selection_cases_cpu.py (which proves with the
Python oracle alone that every input can tell the right rule from a wrong one)
and by test_ga_selection_gpu.py / test_pool_gpu.py (which run them on the
device).  A wrong survivor is still a valid tour with a valid key, so an input
only checks the rule when keys tie where the rule decides: every GA case has
equal keys on both sides of the survival cut, every pool key set has a run of
duplicates longer than E lying across the E-th place.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass

import numpy as np

from oracle import pool as opool
from oracle import search
from vrpms_amd import synth

M64 = (1 << 64) - 1
CHUNK = 2048                 # kTopChunk of pool.hip
LDS_BYTES = 160 * 1024       # per workgroup on CDNA4


# ---------------------------------------------------------------------------
# GA cases
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def instance(kind: str):
    """n5: about ten keys per hundred tours; n9: about half the keys of a
    population distinct; long: 80 customers (two 64-position slots per lane)
    on durations coarsened to 1..5, so that keys still tie; td: hour-indexed,
    outside the packed layout (children travel as rows)."""
    if kind == "n5":
        return synth.cvrp(5, 2, seed=1)
    if kind == "n9":
        return synth.cvrp(9, 3, seed=1)
    if kind == "td":
        return synth.td_cvrp(6, 2, seed=2)
    assert kind == "long"
    x = synth.cvrp(80, 7, seed=3)
    D = np.asarray(x.durations)
    return synth.Instance("cvrp80_coarse", np.where(D > 0, 1 + D // 350, 0), x.demand, x.capacities,
                          x.start_times, "cvrp", x.meta)


def scorer(inst):
    return search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times,
                         inst.problem)


@dataclass(frozen=True)
class GaCase:
    name: str
    kind: str          # instance(kind)
    islands: int
    P: int
    calls: tuple       # generations of each vrpms_ga_generation call, in order
    seed: int          # of the start population and of the GA's Philox streams
    start: str = "random"
    pmut: float = 0.3
    gen0: int = 0

    @property
    def gens(self) -> int:
        return sum(self.calls)

    @property
    def pm(self) -> int:
        return min(int(round(self.pmut * 2**32)), 2**32 - 1)


# Seeds other than 1, where seed 1 does not put a tie across the cut of every
# island (or lets a generation pass without a surviving child): found by
# trying 1, 2, 3, ... against test_selection_cases_cpu.py.
SEEDS = {
    "grid_n9_p16": 8, "grid_n9_p17": 8, "grid_n9_p63": 4, "grid_n9_p129": 2, "grid_n9_p255": 4,
    "grid_n9_p256": 5, "grid_n9_p257": 4, "grid_n9_p320": 2, "grid_n9_p512": 3, "grid_n9_p1023": 2,
    "one_p16": 2, "handin_p257": 4, "past_n9_p2049": 2, "past_td_p300": 2,
    "grid_n5_p2": 114, "grid_n9_p2": 36,
}
# Two members converge at once: only frequent mutation keeps children entering.
PMUT = {"grid_n5_p2": 0.9, "grid_n9_p2": 0.9}


def _ga(name, kind, islands, P, calls, start="random"):
    return GaCase(name, kind, islands, P, tuple(calls), SEEDS.get(name, 1), start,
                  PMUT.get(name, 0.3))


GRID_P = (2, 16, 17, 63, 65, 129, 191, 193, 255, 256, 257, 320, 512, 513, 960, 961, 1023, 1024)
GA_GRID = [_ga(f"grid_{k}_p{P}", k, 2, P, (4,)) for k in ("n5", "n9") for P in GRID_P]
GA_ONE = [_ga(f"one_p{P}", "n5", 2, P, (1,)) for P in (16, 17, 512, 513, 1024)]
GA_HANDIN = [_ga(f"handin_p{P}", "n9", 2, P, (2, 2)) for P in (65, 193, 257, 961)]
GA_PROBE = [_ga(f"probe_p{P}", "n5", 4, P, (3,), start="probe") for P in (256, 1024)]
GA_LONG = [_ga("long_p300", "long", 2, 300, (3,))]
GA_PAST = [_ga(f"past_n9_p{P}", "n9", 1, P, (2,)) for P in (1025, 2048, 2049, 4096)] + \
          [_ga(f"past_td_p{P}", "td", 1, P, (2,)) for P in (300, 1025)]
GA_CASES = GA_GRID + GA_ONE + GA_HANDIN + GA_PROBE + GA_LONG + GA_PAST
GA_BY_NAME = {c.name: c for c in GA_CASES}


def _probe_start(case, inst, sc):
    """Four islands for the sortedness probe of the fused kernel (keys
    non-decreasing <=> sorted by (key, index)): 0 sorted; 1 sorted except
    positions (0, 1); 2 sorted except (P - 2, P - 1); 3 all keys equal."""
    assert case.islands == 4 and inst.n <= 6
    P = case.P
    rng = np.random.default_rng(case.seed)
    perms = [list(p) for p in itertools.permutations(range(1, inst.n + 1))]
    keys = [sc(p) for p in perms]
    lo, hi = min(keys), max(keys)

    def draw(ok, count):
        cand = [i for i in range(len(perms)) if ok(keys[i])]
        pick = sorted((cand[int(j)] for j in rng.integers(0, len(cand), size=count)),
                      key=lambda i: keys[i])        # stable: ties keep their draw order
        return [perms[i] for i in pick]

    best, worst = perms[keys.index(lo)], perms[keys.index(hi)]
    i0 = draw(lambda k: True, P)
    i1 = [best] + draw(lambda k: k > lo, P - 1)
    i1[0], i1[1] = i1[1], i1[0]
    i2 = draw(lambda k: k < hi, P - 1) + [worst]
    i2[P - 2], i2[P - 1] = i2[P - 1], i2[P - 2]
    # the most frequent key that is neither the best nor the worst (children can go either way)
    mid = [k for k in keys if lo < k < hi]
    common = max(sorted(set(mid)), key=mid.count)
    i3 = draw(lambda k: k == common, P)
    return [i0, i1, i2, i3]


@functools.lru_cache(maxsize=None)
def ga_start(name: str):
    """(tours [island][P][n], keys [island][P]) the case starts from."""
    case = GA_BY_NAME[name]
    inst = instance(case.kind)
    sc = scorer(inst)
    if case.start == "probe":
        pops = _probe_start(case, inst, sc)
    else:
        R = synth.random_perms(case.islands * case.P, inst.n, seed=case.seed).astype(np.int64)
        pops = R.reshape(case.islands, case.P, inst.n).tolist()
    return pops, [[sc(t) for t in isl] for isl in pops]


def order_desc_index(K, ck):
    """WRONG: ties broken by descending index."""
    return sorted(search.survivor_order(K, ck), key=lambda p: (p[0], -p[1]))


def order_children_first(K, ck):
    """WRONG: on equal keys the children go before the parents."""
    pop = len(K)
    return sorted(search.survivor_order(K, ck), key=lambda p: (p[0], p[1] < pop, p[1]))


GA_WRONG = {"desc_index": order_desc_index, "children_first": order_children_first}


@functools.lru_cache(maxsize=None)
def ga_replay(name: str, rule: str = ""):
    """The case replayed by oracle/search.py ga_generation under the survivor
    rule `rule` ("" = the right one): (tours, keys, log), log[g][island] the
    2P ordered (key, index) pairs of generation g."""
    case = GA_BY_NAME[name]
    sc = scorer(instance(case.kind))
    order = GA_WRONG[rule] if rule else search.survivor_order
    pops, keys = ga_start(name)
    log = []

    def logged(K, ck):
        o = order(K, ck)
        log[-1].append(o)
        return o

    for g in range(case.gens):
        log.append([])
        pops, keys = search.ga_generation(sc, pops, keys, case.seed, case.gen0 + g, case.pm, logged)
    return pops, keys, log


def ga_fused_lds(N: int, n: int, P: int) -> int:
    """ga_fused_layout (ga_fused.hip) in Python ints: the LDS bytes of the
    fused kernel for an island of P tours of n customers, N nodes."""
    al = lambda x: (x + 15) & ~15       # noqa: E731
    rs = (n + 3) & ~3
    if (rs // 4) % 2 == 0:
        rs += 4
    M = 1
    while M < 2 * P:
        M <<= 1
    off = al(N * N * 8)
    runs = 64 * ((P + 63) // 64)
    for part in (2 * P * rs, P * 8, P * 8, P * 2, P * 4, M * 8, M * 4, 16 * 2 * N, 64, runs * 8,
                 runs * 4):
        off = al(off + part)
    return off


# ---------------------------------------------------------------------------
# Pool key sets
# ---------------------------------------------------------------------------
def topk_levels(count: int, E: int) -> int:
    """Passes of pool.hip topk: chunks of 2048 -> E each, until one chunk."""
    levels = 1
    while count > CHUNK:
        count = -(-count // CHUNK) * E
        levels += 1
    return levels


def dup_run(count: int, E: int, worst: bool):
    """[a, b): where pool_keys puts its long run of one value."""
    L = min(E + 9, count - 6)
    a = max(0, min(CHUNK - L // 2, count - L - (1 if worst else 0)))
    return a, a + L


def pool_keys(count: int, E: int, seed: int, worst: bool = False):
    """count keys for a top-E (worst = False) or worst-E (True) selection:
    random 62-bit values with a third of them tied, 0 and 2^64 - 1 twice each,
    and one value E + 9 times in a row (as far as count allows), next in rank
    after the two extremes at that end -- so the run lies across the E-th
    place (with E = 1 the two zeros do) -- and in memory across the first
    2048-chunk boundary where the pool has one.  worst: the last row holds
    key 0, alone in its chunk when count % 2048 == 1 (its inverted key equals
    the selection's pad key); the run stops short of it, so at count = 2049,
    where that row is all of the second chunk, the run stays in the first."""
    assert count >= 12
    rng = np.random.default_rng(seed)
    k = [int(x) + 16 for x in rng.integers(0, 2**62, size=count)]
    for i in rng.integers(0, count, size=count // 3):
        k[int(i)] = k[0]
    a, b = dup_run(count, E, worst)
    free = [i for i in range(count) if not a <= i < b]
    for i in range(a, b):
        k[i] = M64 - 1 if worst else 7
    k[free[0]] = 0
    k[free[1]] = M64
    if worst:
        assert free[-1] == count - 1
        k[count - 1] = 0
        k[free[-2]] = M64
    else:
        k[free[len(free) // 2]] = 0
        k[free[-1]] = M64
    return k


def pool_rows(count: int, n: int, seed: int):
    """count rows of n tokens in 1..9 (the pool kernels move rows, they do not
    read them); all rows distinct where 9^n allows it."""
    rng = np.random.default_rng(seed + 1000)
    return rng.integers(1, 10, size=(count, n))


ELITE_CASES = [(2048, 1024), (2049, 1024), (4097, 1024), (6145, 1024), (20481, 1024), (1024, 1024),
               (2049, 1), (70000, 1000)]
WORST_CASES = [(2049, 16), (6145, 1024), (20481, 700)]
POOL_N = 5


def elites_desc(tours, keys, E):
    """WRONG: the E best with ties broken by descending index."""
    idx = sorted(range(len(keys)), key=lambda i: (int(keys[i]), -i))[:E]
    return [list(tours[i]) for i in idx], [int(keys[i]) for i in idx]


def inject_worst_desc(tours, keys, mig_tours, mig_keys):
    """WRONG: INJECT_WORST with the worst-E ties broken by descending index."""
    tours, keys = [list(t) for t in tours], [int(k) for k in keys]
    idx = sorted(range(len(keys)), key=lambda i: (-keys[i], -i))[:len(mig_keys)]
    for e, r in enumerate(idx):
        tours[r], keys[r] = list(mig_tours[e]), int(mig_keys[e])
    return tours, keys


def migrants(E: int, n: int, seed: int, values=None):
    """E migrants, keys ascending (they are some pool's elites)."""
    rng = np.random.default_rng(seed + 2000)
    if values is None:
        mk = sorted(int(x) for x in rng.integers(1, 2**62, size=E))
    else:
        mk = sorted(int(values[int(j)]) for j in rng.integers(0, len(values), size=E))
    return rng.integers(1, 10, size=(E, n)), mk


# INJECT_SORTED: (groups, P, E)
SORTED_CASES = [(300, 1, 7), (4, 64, 11), (2, 1500, 9), (1, 4096, 1024), (3, 5, 40), (8, 50, 3)]


def sorted_islands(groups: int, P: int, E: int, seed: int, n: int = POOL_N):
    """`groups` islands of P rows, each sorted by key, and E migrants: all keys
    from one small set (with 0 and 2^64 - 1), so migrants tie with the rows
    they are sorted among and with each other."""
    rng = np.random.default_rng(seed)
    values = [0, M64] + [1000 * int(x) for x in rng.integers(1, 2**40, size=max(2, P // 4))]
    keys = []
    for _ in range(groups):
        keys += sorted(values[int(j)] for j in rng.integers(0, len(values), size=P))
    mt, mk = migrants(E, n, seed, values)
    return pool_rows(groups * P, n, seed), keys, mt, mk


def inject_sorted_desc(tours, keys, mig_tours, mig_keys, groups):
    """WRONG: INJECT_SORTED re-sorting each island with ties by descending slot."""
    tours, keys = [list(t) for t in tours], [int(k) for k in keys]
    P = len(keys) // groups
    for g in range(groups):
        gt, gk = tours[g * P:(g + 1) * P], keys[g * P:(g + 1) * P]
        for e in range(g, len(mig_keys), groups):
            slot = P - 1 - e // groups
            if slot < 0:
                break
            gt[slot], gk[slot] = list(mig_tours[e]), int(mig_keys[e])
        order = sorted(range(P), key=lambda i: (gk[i], -i))
        tours[g * P:(g + 1) * P] = [gt[i] for i in order]
        keys[g * P:(g + 1) * P] = [gk[i] for i in order]
    return tours, keys


# island_pack + island_merge: (world, E, n, identical messages)
MERGE_CASES = [(3, 1024, 3, False), (9, 1024, 1, False), (5, 12, 37, True), (3, 8, 0, False)]


def merge_pools(world: int, E: int, n: int, identical: bool, seed: int = 7):
    """One pool of E + 37 rows per rank, the keys of all ranks from one small
    set, so that keys tie across ranks and across positions."""
    rng = np.random.default_rng(seed + world)
    count = E + 37
    values = [0, M64] + [int(x) for x in rng.integers(1, 2**62, size=E // 3 + 2)]
    pools = []
    for r in range(world):
        if identical and r:
            pools.append(pools[0])
            continue
        keys = [values[int(j)] for j in rng.integers(0, len(values), size=count)]
        pools.append((rng.integers(1, 10, size=(count, n)), keys))
    return pools


def merge_by_position(msgs: bytes, world: int, E: int, n: int):
    """WRONG: island_merge ordering ties by (key, position, rank)."""
    mb = opool.msg_bytes(E, n)
    cands = []
    for r in range(world):
        m = np.frombuffer(msgs[r * mb:(r + 1) * mb], dtype=np.uint8)
        ks = m[:8 * E].view(np.uint64)
        ts = m[8 * E:8 * E + 2 * E * n].view(np.uint16).reshape(E, n)
        cands += [(int(ks[e]), e, r, ts[e].tolist()) for e in range(E)]
    cands.sort(key=lambda c: c[:3])
    return [c[3] for c in cands[:E]], [c[0] for c in cands[:E]]
