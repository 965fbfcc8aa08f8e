"""The premises of tests/objective_cases.py, proved without a GPU with the C
and Python oracles alone: every case tells the max-duration objective (A8,
objective 1) from the sum objective, so a kernel that ignored the objective --
or priced the longest route wrongly where it only breaks ties under "sum" --
cannot pass test_objective_max_gpu.py; and the saturation instance clamps the
secondary key field and never the primary."""
import itertools
import math

import numpy as np
import pytest

import objective_cases as oc
from oracle import search, spec


def _scorer(inst, objective):
    return search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times,
                         inst.problem, objective)


# ---------------------------------------------------------------------------
# SA
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in oc.SA_CASES])
def test_sa_case_tells_the_objectives_apart(coracle, name):
    """The C oracle's final tours under objective 1 differ from those under
    objective 0 in at least half of the chains, at every temperature the case
    runs; the chains moved; and the restatement that walks only what a move
    can change (resync) agrees with the full re-evaluation under objective 1."""
    c, inst, P = oc.sa_case(name)
    L = inst.n + inst.K - 1
    assert P.shape == (oc.CHAINS, L) and P.dtype == np.uint16
    assert (np.sort(P, axis=1) == np.sort(np.concatenate([np.zeros(inst.K - 1, dtype=np.int64),
                                                          np.arange(1, inst.N)]))).all()
    for inv_t0 in c.temps:
        r1 = oc.sa_reference(name, inv_t0, 1)
        r0 = oc.sa_reference(name, inv_t0, 0)
        differ = int((r1[0] != r0[0]).any(axis=1).sum())
        assert 2 * differ >= oc.CHAINS, (name, inv_t0, differ)
        assert (r1[0] != P).any()
        # every reported key is the spec's key of the reported tour under objective 1
        for ch in (0, oc.CHAINS - 1):
            for tour, key in ((r1[0][ch], r1[1][ch]), (r1[2][ch], r1[3][ch])):
                assert key == spec.eval_cvrp(inst.durations, tour, inst.demand, inst.capacities,
                                             inst.start_times, 1)["key"]
        rs = oc.oracle_sa(coracle, inst, P, c.steps, inv_t0, c.window, c.types, c.moves, 1,
                          resync=True)
        assert (rs[0] == r1[0]).all() and rs[1] == r1[1]
        assert (rs[2] == r1[2]).all() and rs[3] == r1[3]


def test_sa_infeasible_case_starts_with_unserved_customers():
    c, inst, P = oc.sa_case("packed_infeasible")
    unv = [spec.eval_cvrp(inst.durations, row, inst.demand, inst.capacities, inst.start_times,
                          1)["unvisited"] for row in P]
    assert min(unv) > 0


def test_sa_cases_cover_the_dispatch_premises():
    """The instance properties vrpms_sa_run's branches test, from the data."""
    for c in oc.SA_CASES:
        _, inst, _ = oc.sa_case(c.name)
        D = np.asarray(inst.durations)
        assert D.max() <= 65535                                  # the u16 matrix
        if "symmetric" in c.expect:
            assert bool((D[0] == D[0].T).all()) == c.expect["symmetric"], c.name
        if "uniform_cap" in c.expect:
            assert (len(set(inst.capacities.tolist())) == 1) == c.expect["uniform_cap"], c.name
        if "flex" in c.expect:
            assert (inst.capacities.min() < inst.demand.max()) == c.expect["flex"], c.name
        if "hour_minor" in c.expect:
            assert (inst.H == 24) == c.expect["hour_minor"], c.name
        if c.expect.get("fast"):
            assert inst.H == 1 and inst.N <= 128, c.name
        assert c.moves in (64, 128) and 60 <= c.steps <= 80


# ---------------------------------------------------------------------------
# the saturation instance
# ---------------------------------------------------------------------------
def test_saturated_instance_by_its_numbers():
    inst = oc.saturated()
    D = inst.durations[0]
    off = D[~np.eye(inst.N, dtype=bool)]
    assert inst.N == 6 and inst.K == 3 and (D == D.T).all()
    assert off.min() >= 40_000_000 and off.max() <= 50_000_000 and off.max() > 65535
    assert (inst.demand[1:] == 1).all() and (inst.capacities == 2).all()
    assert 3 * int(off.max()) < spec.KEY_CLAMP <= 8 * int(off.min())
    assert int(inst.start_times.max()) + (inst.N + inst.K + 1) * int(off.max()) < 2**31


def test_saturated_every_full_tour_clamps_only_the_secondary():
    """All 120 first-fit tours: nobody unserved, sum >= 2^28 - 1 > max, so under
    objective 1 the secondary field is the clamp and the primary is the max."""
    inst, P = oc.saturated(), oc.saturated_tours()
    assert P.shape == (120, 8) and len({tuple(r) for r in P.tolist()}) == 120
    for row in P[:, :7]:
        r = spec.eval_cvrp(inst.durations, row, inst.demand, inst.capacities, inst.start_times, 1)
        assert r["unvisited"] == 0 and r["max"] < spec.KEY_CLAMP <= r["sum"]
        assert spec.unpack_key(r["key"]) == (0, r["max"], spec.KEY_CLAMP)


def test_saturated_sa_visits_only_such_tours(coracle):
    """The C oracle's chains, one step at a time: every current and best tour
    on the way has the secondary at the clamp and the primary below it, the
    chains move, and the stepwise run ends where the 40-step run ends."""
    inst, P = oc.saturated(), oc.saturated_starts()
    assert P.shape == (oc.SAT_CHAINS, 7)
    whole = oc.oracle_sa(coracle, inst, P, oc.SAT_STEPS, oc.SAT_INV_T0, 0, 0, 64, 1)
    cur, best = P.copy(), P.copy()
    bk = np.full(oc.SAT_CHAINS, 2**64 - 1, dtype=np.uint64)
    inv_t = np.float32(oc.SAT_INV_T0)
    primaries = set()
    for s in range(oc.SAT_STEPS):
        ck = coracle.sa_run(inst.durations, cur, best, bk, 1, float(inv_t), oc.INV_ALPHA, oc.SEED,
                            oc.STEP0 + s, inst.demand, inst.capacities, inst.start_times,
                            objective=1)
        inv_t = np.float32(inv_t * np.float32(oc.INV_ALPHA))
        for tour, key in list(zip(cur, ck)) + list(zip(best, bk)):
            r = spec.eval_cvrp(inst.durations, tour, inst.demand, inst.capacities,
                               inst.start_times, 1)
            assert int(key) == r["key"]
            unv, primary, secondary = spec.unpack_key(int(key))
            assert unv == 0 and secondary == spec.KEY_CLAMP and primary == r["max"] < spec.KEY_CLAMP
            assert r["sum"] >= spec.KEY_CLAMP
            primaries.add(primary)
    assert (cur == whole[0]).all() and [int(x) for x in ck] == whole[1]
    assert (best == whole[2]).all() and [int(x) for x in bk] == whole[3]
    # the chains move and improve: 64 moves a step nearly exhaust a 7-token tour's
    # neighbourhood, so they reach the smallest longest route early and then wander
    # over tours of equal keys (the saturated secondary cannot tell them apart)
    start = [spec.eval_cvrp(inst.durations, row, inst.demand, inst.capacities, inst.start_times,
                            1)["max"] for row in P]
    assert (cur != P).any() and all(min(primaries) < s for s in start)
    # under objective 0 it is the primary field of these tours that is the clamp:
    # the state "secondary saturated, primary not" exists under objective 1 only
    k0 = coracle.eval_batch(inst.durations, cur, inst.demand, inst.capacities, inst.start_times,
                            1, 0)[0]
    assert all(spec.unpack_key(int(k))[:2] == (0, spec.KEY_CLAMP) for k in k0)


def test_saturated_c_oracle_scores_like_the_spec(coracle):
    inst, P = oc.saturated(), oc.saturated_tours()
    keys, sums, maxs, unv = coracle.eval_batch(inst.durations, P, inst.demand, inst.capacities,
                                               inst.start_times, 1, 1, n=7)
    for i, row in enumerate(P[:, :7]):
        r = spec.eval_cvrp(inst.durations, row, inst.demand, inst.capacities, inst.start_times, 1)
        assert (int(keys[i]), int(sums[i]), int(maxs[i]), int(unv[i])) == \
            (r["key"], r["sum"], r["max"], 0)


# ---------------------------------------------------------------------------
# ACO, GA, brute force
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.ACO_CASES))
def test_aco_case_tells_the_objectives_apart(name):
    """tau after iteration 1 under objective 1 is not tau under objective 0."""
    r1, r0 = oc.aco_reference(name, 1), oc.aco_reference(name, 0)
    assert any((a != b).any() for a, b in zip(r1[0][3], r0[0][3]))
    inst = oc.aco_instance(name)
    assert (inst.N > 256) == (name == "cvrp260")
    # the deposit is 2^30 / (1 + longest route of the depositing tour)
    key, ant = r1[0][2][0]
    if not oc.ACO_CASES[name]["bsf_period"]:
        t = r1[0][0][0][ant]
        r = spec.eval_cvrp(inst.durations, t, inst.demand, inst.capacities, inst.start_times, 1)
        assert key == r["key"] and spec.unpack_key(key)[1] == r["max"]
        evap = oc.ACO_TAU0 - (oc.ACO_TAU0 >> 3)
        assert int(r1[0][3][0][0, t[0]]) == evap + (1 << 30) // (1 + r["max"])
    elif oc.ACO_CASES[name]["inject"]:
        # the injected tour beats both iterations' ants under the max-first key, so
        # iteration 1's deposit is the best-so-far's and not the iteration best's
        b = oc.aco_best_start(name, 1)
        assert b[1][0] < r1[0][2][0][0] and b[1][0] < r1[1][2][0][0]
        assert r1[1][4] == b[0] and r1[1][5] == b[1]
    else:
        # the empty best-so-far is written from the ants: iteration 0's best, then
        # the better of the two by the max-first key
        assert r1[0][5][0] == r1[0][2][0][0] and r1[0][4][0] == r1[0][0][0][r1[0][2][0][1]]
        assert r1[1][5][0] == min(r1[0][2][0][0], r1[1][2][0][0])
    assert len(r1) == oc.ACO_ITERS == 2


@pytest.mark.parametrize("name", list(oc.GA_CASES))
def test_ga_case_tells_the_objectives_apart(name):
    k1, p1, _ = oc.ga_reference(name, 1)
    k0, p0, _ = oc.ga_reference(name, 0)
    assert k1 != k0 and p1 != p0
    inst, _ = oc.ga_case(name)
    assert (inst.H == 24) == (name == "td20")


@pytest.mark.parametrize("name", list(oc.BF_CASES))
def test_bf_case_optimum_differs_between_objectives(coracle, name):
    inst = oc.bf_instance(name)
    n = inst.n
    kw = oc.bf_kw(inst)
    k1, r1 = coracle.bf(inst.durations, n, 0, math.factorial(n), objective=1, **kw)
    k0, r0 = coracle.bf(inst.durations, n, 0, math.factorial(n), objective=0, **kw)
    assert r1 != r0
    t1, t0 = search.unrank(r1, n), search.unrank(r0, n)
    assert _scorer(inst, 1)(t1) == k1 and _scorer(inst, 0)(t0) == k0
    # the objective-0 optimum is strictly worse under objective 1, and the reverse
    assert _scorer(inst, 1)(t0) > k1 and _scorer(inst, 0)(t1) > k0
    # the Python brute force agrees with the C one under objective 1
    if n <= 7:
        assert search.bf(_scorer(inst, 1), n) == (k1, r1)
    wins = oc.bf_windows(n)
    assert wins[1][1] == wins[2][0] and wins[1][1] - wins[1][0] != wins[2][1] - wins[2][0]
    parts = [coracle.bf(inst.durations, n, a, b, objective=1, **kw) for a, b in wins[1:]]
    assert min(parts) == (k1, r1)


# ---------------------------------------------------------------------------
# the front door's instances
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["static", "td"])
def test_front_instance_every_full_solution_is_a_greedy_split(kind):
    """Demands add up to the fleet's capacity, so a solution that serves all
    customers fills every vehicle: whatever routes it has, the greedy split of
    their concatenation reproduces them (checked on every way of filling the
    three vehicles), and the objectives disagree on the optimum."""
    inst = oc.front(kind)
    assert inst.n == 7 and inst.K == 3 and inst.H == (1 if kind == "static" else 24)
    assert int(inst.demand.sum()) == int(inst.capacities.sum())
    dem, cap = inst.demand, int(inst.capacities[0])
    seen = 0
    for p in itertools.permutations(range(1, 8)):
        # cut p where the loads reach the capacity exactly, if they do
        routes, load, cur = [], 0, []
        for c in p:
            cur.append(c)
            load += int(dem[c])
            if load == cap:
                routes.append(cur)
                cur, load = [], 0
            elif load > cap:
                break
        if len(routes) != 3 or cur:
            continue
        seen += 1
        r = spec.eval_cvrp(inst.durations, p, dem, inst.capacities, inst.start_times, 1)
        assert r["routes"] == routes and r["unvisited"] == 0
    assert seen > 0
    best = {}
    for obj in (0, 1):
        sc = _scorer(inst, obj)
        best[obj] = min(itertools.permutations(range(1, 8)), key=lambda p: (sc(p), p))
    assert best[0] != best[1]
