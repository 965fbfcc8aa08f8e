"""Exact small-fleet VRP by subset partition DP (algorithm "sp", spec A15):
the C entry points vrpms_vrp_sp_workspace / vrpms_vrp_sp_run, Context.vrp_sp,
runners.set_partition, solver.solve_vrp("sp") and the inline route
POST /solve/vrp/sp.

The reference is a numpy restatement of A15 in this file (same recurrence,
same tie rule), itself checked against the enumeration of every separator
tour through the spec's evaluator; the GPU must return the identical key,
tour and routes."""
import ctypes
import functools
import itertools
import json
import threading

import numpy as np
import pytest

from oracle import spec
from vrpms_amd import _lib, remote, runners, service, solver, synth

INF = np.int64(1) << 60


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def hk_table(D, n):
    """A14's g[S][j - 1] for every S of at most n - 1 customers."""
    full = 1 << n
    masks = np.arange(full, dtype=np.int64)
    pc = np.zeros(full, dtype=np.int64)
    for i in range(n):
        pc += (masks >> i) & 1
    g = np.full((full, n), INF, dtype=np.int64)
    g[0] = D[1:n + 1, 0]
    for k in range(1, n):
        Ss = masks[pc == k]
        best = np.full((Ss.shape[0], n), INF, dtype=np.int64)
        for i in range(n):
            idx = np.nonzero((Ss >> i) & 1)[0]
            cand = g[Ss[idx] ^ (1 << i), i][:, None] + D[1:n + 1, i + 1][None, :]   # D[j][i]
            best[idx] = np.minimum(best[idx], cand)
        g[Ss] = best
    return g


def submasks(S, n):
    """Every T subset of S, in increasing order."""
    out = np.zeros(1, dtype=np.int64)
    for i in range(n):
        if (S >> i) & 1:
            out = np.concatenate([out, out | (1 << i)])
    return out


def sp_ref(D, demand, caps, objective="sum", n=None):
    """A15 -> dict(unvisited, primary, routes, durations, tour, key)."""
    D = np.asarray(D, dtype=np.int64)
    n = D.shape[0] - 1 if n is None else n
    K, full = len(caps), 1 << n
    g = hk_table(D, n)
    route = np.zeros(full, dtype=np.int64)
    dem = np.zeros(full, dtype=np.int64)
    for S in range(1, full):
        mem = [i for i in range(n) if (S >> i) & 1]
        route[S] = min(int(D[0, i + 1] + g[S ^ (1 << i), i]) for i in mem)
        dem[S] = sum(int(demand[i + 1]) for i in mem)
    subs = [submasks(S, n) for S in range(full)]

    def joined(k, f_k, S):
        """route[T] (+) f_k[S \\ T] per submask T of S, INF where T is too
        heavy for vehicle k or S \\ T is unreachable (INF is never added to)."""
        T = subs[S]
        a, b = route[T], f_k[S ^ T]
        ok = (dem[T] <= caps[k]) & (b < INF)
        return np.where(ok, a + np.where(ok, b, 0) if objective == "sum" else np.maximum(a, b), INF)

    f = [np.full(full, INF, dtype=np.int64)]
    f[0][0] = 0
    for k in range(K):
        f.append(np.array([joined(k, f[k], S).min() for S in range(full)], dtype=np.int64))
    unv, prim, S = min((n - bin(S).count("1"), int(f[K][S]), S) for S in range(full)
                       if f[K][S] < INF)
    served = S
    routes = [None] * K
    for k in range(K - 1, -1, -1):
        T = int(subs[S][np.argmax(joined(k, f[k], S) == f[k + 1][S])])   # smallest mask attaining it
        r, cur, R = [], 0, T
        while R:                                   # lexicographically smallest optimal route on T
            mem = [i for i in range(n) if (R >> i) & 1]
            vals = [int(D[cur, i + 1] + g[R ^ (1 << i), i]) for i in mem]
            i = mem[vals.index(min(vals))]
            r.append(i + 1)
            cur, R = i + 1, R ^ (1 << i)
        routes[k] = r
        S ^= T
    assert S == 0
    tour = [t for r in routes for t in r + [0]]
    tour += [c for c in range(1, n + 1) if not (served >> (c - 1)) & 1]
    durs = [spec.eval_tsp(D, r) if r else 0 for r in routes]
    dsum, dmax = sum(durs), max(durs)
    assert prim == (dsum if objective == "sum" else dmax)
    key = spec.pack_key(unv, dsum, dmax) if objective == "sum" else spec.pack_key(unv, dmax, dsum)
    return dict(unvisited=unv, primary=prim, routes=routes, durations=durs, tour=tour, key=key)


def obj_id(objective):
    return spec.OBJ_SUM if objective == "sum" else spec.OBJ_MAX


def rescore(D, tour, demand, caps, objective, starts=None):
    starts = [0] * len(caps) if starts is None else starts
    return spec.eval_cvrp(D, tour, demand, caps, starts, obj_id(objective))


def best_over(D, tours, demand, caps, objective):
    """Least (unvisited, primary) over the rows of `tours` (A6/A7 + A10)."""
    _, dsum, dmax, unv = spec.eval_cvrp_batch(D, tours, demand, caps, [0] * len(caps),
                                              obj_id(objective))
    prim = dsum if objective == "sum" else dmax
    r = np.lexsort((prim, unv))[0]
    return int(unv[r]), int(prim[r])


def separator_optimum(D, demand, caps, objective):
    """Every arrangement of 1..n and K separators."""
    n = np.asarray(D).shape[-1] - 1
    tours = np.array(sorted(set(itertools.permutations(list(range(1, n + 1)) + [0] * len(caps)))))
    return best_over(D, tours, demand, caps, objective)


def greedy_split_optimum(D, demand, caps, objective):
    """What bf searches: every giant tour under the greedy split."""
    n = np.asarray(D).shape[-1] - 1
    tours = np.array(list(itertools.permutations(range(1, n + 1))))
    return best_over(D, tours, demand, caps, objective)


def matrix(kind, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "sym":
        return synth.random_symmetric(N, rng)
    if kind == "asym":
        D = rng.integers(3, 321, size=(N, N), dtype=np.int64)
    elif kind == "ties":
        D = rng.integers(1, 3, size=(N, N), dtype=np.int64)
    elif kind == "equal":
        D = np.full((N, N), 7, dtype=np.int64)
    else:
        raise ValueError(kind)
    np.fill_diagonal(D, 0)
    return D


def demands(n, seed, lo=1, hi=9):
    d = np.random.default_rng(1000 + seed).integers(lo, hi + 1, size=n + 1, dtype=np.int64)
    d[0] = 0
    return d


def unequal_cvrp5(seed):
    inst = synth.cvrp(5, 2, seed=seed, slack=1.2)
    caps = [int(inst.capacities[0]) + 2, int(inst.capacities[1]) - 3]
    return inst.durations[0], inst.demand, caps


# the instances on which the optimum is strictly below bf's (the best giant
# tour under the greedy split): name -> (D, demand, caps, objective, sp, bf)
def strict_case(name):
    if name == "balance":
        inst = synth.cvrp(6, 2, seed=0, slack=3.0)
        return inst.durations[0], inst.demand, [int(c) for c in inst.capacities], "max", 2034, 2855
    seed, sp, bf = {"nonmetric0": (0, 816, 839), "nonmetric1": (1, 964, 1040)}[name]
    D = synth.random_symmetric(7, np.random.default_rng(seed))
    return D, np.array([0, 1, 1, 1, 1, 1, 1]), [4, 4], "sum", sp, bf


STRICT = ["balance", "nonmetric0", "nonmetric1"]


def planted(n):
    """Unit demands, capacities 7, 5, 4 (and 1 at n = 17): hidden routes of
    those sizes whose edges, both depot edges included, cost 1, every other
    entry 100..320.  All n customers fit only with every vehicle full, so the
    route sizes are forced, n + K edges cost at least n + K, and the hidden
    routes are the only ones that cost exactly that: a unique optimum."""
    caps = [7, 5, 4] + ([1] if n == 17 else [])
    assert sum(caps) == n
    rng = np.random.default_rng(n)
    D = rng.integers(100, 321, size=(n + 1, n + 1), dtype=np.int64)
    np.fill_diagonal(D, 0)
    order = (rng.permutation(n) + 1).tolist()
    routes, at = [], 0
    for c in caps:
        routes.append(order[at:at + c])
        at += c
        path = [0] + routes[-1] + [0]
        for a, b in zip(path, path[1:]):
            D[a, b] = 1
    dem = np.array([0] + [1] * n)
    return D, dem, caps, routes


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("objective", ["sum", "max"])
@pytest.mark.parametrize("case", ["unequal0", "unequal1", "unequal2", "unservable", "overfull"])
def test_reference_equals_separator_tour_enumeration(case, objective):
    if case.startswith("unequal"):
        D, dem, caps = unequal_cvrp5(int(case[-1]))
    else:
        D, dem, caps = unequal_cvrp5(3)
        dem = dem.copy()
        if case == "unservable":
            dem[3] = max(caps) + 1             # above every capacity
        else:
            caps = [int(dem.sum()) // 3, int(dem.sum()) // 3]   # the fleet carries two thirds
    ref = sp_ref(D, dem, caps, objective)
    assert (ref["unvisited"], ref["primary"]) == separator_optimum(D, dem, caps, objective)
    if not case.startswith("unequal"):
        assert ref["unvisited"] > 0
    e = rescore(D, ref["tour"], dem, caps, objective)
    assert e["key"] == ref["key"] and e["routes"] == ref["routes"]
    assert e["durations"] == ref["durations"] and e["unvisited"] == ref["unvisited"]


@pytest.mark.parametrize("name", STRICT)
def test_reference_is_strictly_below_the_best_greedy_split(name):
    D, dem, caps, objective, sp, bf = strict_case(name)
    ref = sp_ref(D, dem, caps, objective)
    assert (ref["unvisited"], ref["primary"]) == (0, sp)
    assert greedy_split_optimum(D, dem, caps, objective) == (0, bf)
    assert sp < bf


def test_planted_routes_cost_one_per_edge():
    for n in (16, 17):
        D, dem, caps, routes = planted(n)
        tour = [t for r in routes for t in r + [0]]
        e = rescore(D, tour, dem, caps, "sum")
        assert (e["unvisited"], e["sum"], e["routes"]) == (0, n + len(caps), routes)
        assert (D == 1).sum() == n + len(caps) and D[D > 1].min() >= 100


@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


def test_workspace_size(lib):
    b = ctypes.c_uint64()
    for n, K in [(0, 2), (21, 2), (5, 0), (5, 65)]:
        assert lib.vrpms_vrp_sp_workspace(n, K, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    assert b"1 <= K <= 64" in lib.vrpms_last_error()
    assert lib.vrpms_vrp_sp_workspace(5, 2, None) == _lib.VRPMS_EINVAL
    hk = ctypes.c_uint64()
    for K in (1, 2, 64):
        prev = 0
        for n in range(1, 21):
            assert lib.vrpms_vrp_sp_workspace(n, K, ctypes.byref(b)) == _lib.VRPMS_OK
            assert lib.vrpms_tsp_dp_workspace(n, ctypes.byref(hk)) == _lib.VRPMS_OK
            # the Held-Karp table, route, dem, routecap and one array per vehicle
            assert b.value > prev and b.value >= hk.value + (3 + K) * 4 * (1 << n)
            prev = b.value
    prev = 0
    for K in range(1, 65):
        assert lib.vrpms_vrp_sp_workspace(20, K, ctypes.byref(b)) == _lib.VRPMS_OK
        assert b.value > prev
        prev = b.value
    assert prev < 1 << 30


def test_run_rejects_null_ctx_before_any_hip_call(lib):
    assert lib.vrpms_vrp_sp_run(None, 5, None, 0, None, None, None) == _lib.VRPMS_EINVAL
    assert b"ctx is NULL" in lib.vrpms_last_error()


def _locs(N):
    return [{"id": i, "demand": 1} for i in range(N)]


def test_front_end_errors_need_no_gpu():
    assert "sp" in solver.ALGORITHMS
    assert 16 <= solver.SP_MAX_CUSTOMERS <= 20 and solver.SP_MAX_VEHICLES == 64
    N = solver.SP_MAX_CUSTOMERS + 2
    with pytest.raises(ValueError, match=f"at most {solver.SP_MAX_CUSTOMERS} customers"):
        solver.solve_vrp("sp", matrix("sym", N, 0).tolist(), _locs(N), [N, N], [0, 0])
    D6 = matrix("sym", 6, 1)
    with pytest.raises(ValueError, match="at most 64 vehicles"):
        solver.solve_vrp("sp", D6.tolist(), _locs(6), [1] * 65, [0] * 65)
    with pytest.raises(ValueError, match="static"):
        solver.solve_vrp("sp", np.stack([D6] * 24).tolist(), _locs(6), [3, 3], [0, 0])
    with pytest.raises(ValueError, match='use "dp"'):
        solver.solve_tsp("sp", D6.tolist(), [1, 2, 3, 4, 5], 0)
    # the ignored customers do not count against the cap
    n = solver.SP_MAX_CUSTOMERS
    ci = solver.compact_vrp(matrix("sym", N, 0), _locs(N), [N], [0], ignored_customers=[3])
    assert ci.n == n and solver._check_sp(ci) is None


def _store():
    return service.MemoryStore({}, {}, {})


def _vrp_body(N=6, **more):
    body = {"durations": matrix("asym", N, 4).tolist(), "locations": _locs(N),
            "capacities": [3, 2], "startTimes": [0, 5], "ignoredCustomers": [2],
            "completedCustomers": []}
    return json.dumps(dict(body, **more)).encode()


def test_solve_inline_routes_vrp_sp_and_refuses_tsp_sp():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, params["capacities"], params["start_times"],
                     params["ignored_customers"], knobs.get("objective"), len(locations)))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    app = service.App(_store(), solve=fake)
    st, res = app.solve_inline("vrp", "sp", _vrp_body(objective="max"))
    assert st == 200
    assert res == {"success": True, "message": {"durationMax": 2, "durationSum": 3, "vehicles": []}}
    assert seen == [("vrp", "sp", [3, 2], [0, 5], [2], "max", 6)]
    tsp = json.dumps({"durations": [[0, 1], [1, 0]], "customers": [1], "startNode": 0,
                      "startTime": 0}).encode()
    st, res = app.solve_inline("tsp", "sp", tsp)
    assert st == 400 and "no solver /solve/tsp/sp" in res["errors"][0]["reason"]
    assert len(seen) == 1
    # the eight endpoints stay the reference's wire contract
    assert sorted(service.TITLES) == ["aco", "bf", "ga", "sa"]
    assert service.INLINE_ALGORITHMS["vrp"][-1] == "sp" and "sp" not in service.INLINE_ALGORITHMS["tsp"]


def test_sp_is_never_scheduled_as_an_island_model():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((algorithm, knobs.get("devices"), "device" in knobs))
        return {"durationMax": 0, "durationSum": 0, "vehicles": []}

    app = service.App(_store(), solve=fake, devices=[0, 1], island_min_n=0)
    assert app.solve_inline("vrp", "sp", _vrp_body())[0] == 200
    assert app.solve_inline("vrp", "sa", _vrp_body())[0] == 200
    assert seen == [("sp", None, True), ("sa", [0, 1], False)]


def test_remote_forwards_sp_to_the_inline_route():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, knobs.get("objective")))
        return {"durationMax": 4, "durationSum": 7, "vehicles": [{"tour": [0, 1, 0], "duration": 4}]}

    srv = service.serve(service.App(_store(), solve=fake), "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    try:
        base = f"http://127.0.0.1:{srv.server_address[1]}"
        r = remote.solve_vrp("sp", [[0, 1, 2], [1, 0, 3], [2, 3, 0]], _locs(3), [2], [0],
                             objective="max", base=base)
    finally:
        srv.shutdown()
        srv.server_close()
    assert r["durationSum"] == 7 and seen == [("vrp", "sp", "max")]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_sp(ctx, D, dem, caps, objective, starts=None, n=None):
    from vrpms_amd.core import CVRP
    D = np.asarray(D, dtype=np.int64)
    starts = [10 * k for k in range(len(caps))] if starts is None else starts
    ctx.set_instance(CVRP, D, dem, caps, starts, objective=obj_id(objective))
    return runners.set_partition(ctx, D.shape[0] - 1 if n is None else n)


def decoded_routes(ctx, tour, K):
    import torch
    veh, durs = ctx.decode(torch.tensor(tour, dtype=torch.int16, device=ctx.dev), len(tour))
    routes = [[] for _ in range(K)]
    for c, v in zip(tour, veh):
        if v >= 0:
            routes[v].append(c)
    return routes, durs


# name -> (matrix kind, n, seed, demands, capacities)
def ref_case(name):
    kind, n, seed, caps = {
        "n1": ("sym", 1, 1, [9]),
        "n1_k2": ("asym", 1, 2, [0, 9]),
        "n2": ("asym", 2, 3, [9, 9]),
        "n5": ("sym", 5, 4, [14, 12]),               # 32, 64 and 128 submasks at the top:
        "n6": ("asym", 6, 5, [17, 15]),              # below, at and above one wavefront
        "n7": ("sym", 7, 6, [20, 18]),
        "n9": ("sym", 9, 7, [20, 16, 14]),
        "n11": ("asym", 11, 8, [24, 20, 18]),
        "k1": ("sym", 7, 9, [100]),
        "k1_tight": ("sym", 7, 9, [17]),
        "k3_unequal": ("asym", 8, 10, [21, 13, 8]),
        "k3_reversed": ("asym", 8, 10, [8, 13, 21]),
        "k_above_n": ("sym", 3, 11, [9, 9, 9, 9, 9]),
        "cap0": ("sym", 7, 12, [0, 22, 0, 19]),
        "zero_demand": ("asym", 7, 13, [9, 7]),
        "unservable": ("sym", 7, 14, [20, 20]),
        "overfull": ("asym", 8, 15, [11, 9]),
        "equal_matrix": ("equal", 7, 16, [15, 15, 15]),
        "ties": ("ties", 8, 17, [16, 14, 12]),
        "ties_unit": ("ties", 9, 18, [4, 3, 3]),
    }[name]
    D, dem = matrix(kind, n + 1, seed), demands(n, seed)
    if name == "zero_demand":
        dem[[2, 5, 6]] = 0
    if name == "unservable":
        dem[4] = 99
    if name == "ties_unit":
        dem[1:] = 1
    return D, dem, caps


REF_CASES = ["n1", "n1_k2", "n2", "n5", "n6", "n7", "n9", "n11", "k1", "k1_tight", "k3_unequal",
             "k3_reversed", "k_above_n", "cap0", "zero_demand", "unservable", "overfull",
             "equal_matrix", "ties", "ties_unit"]


@functools.lru_cache(maxsize=None)
def ref_of(name, objective):
    D, dem, caps = ref_case(name)
    return sp_ref(D, dem, caps, objective)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", ["sum", "max"])
@pytest.mark.parametrize("name", REF_CASES)
def test_gpu_equals_reference(ctx, name, objective):
    D, dem, caps = ref_case(name)
    ref = ref_of(name, objective)
    if name in ("k1_tight", "unservable", "overfull"):
        assert ref["unvisited"] > 0
    key, tour = gpu_sp(ctx, D, dem, caps, objective)
    print(name, objective, "gpu", key, tour, "ref", ref["key"], ref["tour"])
    assert (key, tour) == (ref["key"], ref["tour"])
    starts = [10 * k for k in range(len(caps))]
    assert key == rescore(D, tour, dem, caps, objective, starts)["key"]
    routes, durs = decoded_routes(ctx, tour, len(caps))
    assert routes == ref["routes"] and durs == ref["durations"]


@pytest.mark.gpu
def test_gpu_serves_the_first_n_customers_of_a_larger_instance(ctx):
    D, dem, caps = matrix("asym", 10, 20), demands(9, 20), [12, 10]
    ref = sp_ref(D, dem, caps, "sum", n=6)
    assert gpu_sp(ctx, D, dem, caps, "sum", n=6) == (ref["key"], ref["tour"])


@pytest.mark.gpu
def test_gpu_one_ample_vehicle_is_held_karp(ctx):
    from vrpms_amd.core import TSP
    D = matrix("asym", 10, 21)
    key, tour = gpu_sp(ctx, D, demands(9, 21), [1000], "sum")
    ctx.set_instance(TSP, D, start_times=(0,))
    hk_key, hk_tour = runners.held_karp(ctx, 9)
    assert tour == hk_tour + [0]
    dur = spec.unpack_key(hk_key)[1]
    assert key == spec.pack_key(0, dur, dur)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", ["sum", "max"])
@pytest.mark.parametrize("n,K,slack", [(8, 2, 1.2), (8, 3, 2.0), (10, 3, 1.3)])
def test_gpu_is_not_above_brute_force(ctx, n, K, slack, objective):
    inst = synth.cvrp(n, K, seed=n + K, slack=slack)
    caps = [int(c) for c in inst.capacities]
    key, tour = gpu_sp(ctx, inst.durations[0], inst.demand, caps, objective, starts=[0] * K)
    bkey, _ = runners.brute_force(ctx, n)
    print(n, K, objective, "sp", spec.unpack_key(key), "bf", spec.unpack_key(bkey))
    assert spec.unpack_key(key)[:2] <= spec.unpack_key(bkey)[:2]
    assert key == rescore(inst.durations[0], tour, inst.demand, caps, objective)["key"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", STRICT)
def test_gpu_is_strictly_below_brute_force(ctx, name):
    D, dem, caps, objective, sp, bf = strict_case(name)
    key, _ = gpu_sp(ctx, D, dem, caps, objective, starts=[0, 0])
    bkey, _ = runners.brute_force(ctx, D.shape[0] - 1)
    assert spec.unpack_key(key)[:2] == (0, sp) and spec.unpack_key(bkey)[:2] == (0, bf)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 17])
def test_gpu_planted_unique_optimum(ctx, n):
    """n = 16 and 17: table rows of 16 and of 32 words, and sets of 15 and
    more customers, whose submasks are cut into several work items."""
    from vrpms_amd.core import CVRP
    D, dem, caps, routes = planted(n)
    if n == 16:
        key, tour = gpu_sp(ctx, D, dem, caps, "sum")
    else:
        ctx.set_instance(CVRP, D, dem, caps, [0] * len(caps), objective=spec.OBJ_SUM)
        key, tour = ctx.vrp_sp(n)
    assert tour == [t for r in routes for t in r + [0]]
    assert key == spec.pack_key(0, n + len(caps), 8)


@pytest.mark.gpu
def test_gpu_cvrp16_routes_are_optimal_tours_and_bound_sa():
    inst = synth.cvrp(16, 4, seed=0, slack=1.2)
    D = inst.durations[0]
    locs = [{"id": i, "demand": int(inst.demand[i])} for i in range(17)]
    caps = [int(c) for c in inst.capacities]
    res = solver.solve_vrp("sp", D.tolist(), locs, caps, [0] * 4, with_unvisited=True)
    assert res["unvisited"] == []
    assert sorted(c for v in res["vehicles"] for c in v["tour"][1:-1]) == list(range(1, 17))
    tour = [t for v in res["vehicles"] for t in v["tour"][1:]]
    e = rescore(D, tour, inst.demand, caps, "sum")
    assert (e["sum"], e["max"], e["unvisited"]) == (res["durationSum"], res["durationMax"], 0)
    assert e["durations"] == [v["duration"] for v in res["vehicles"]]
    for v in res["vehicles"]:
        cust = v["tour"][1:-1]
        assert sum(int(inst.demand[c]) for c in cust) <= caps[0]
        assert v["duration"] == (solver.solve_tsp("dp", D.tolist(), cust, 0)["duration"] if cust else 0)
    sa = solver.solve_vrp("sa", D.tolist(), locs, caps, [0] * 4, seed=1, chains=64, steps=2000,
                          with_unvisited=True)
    print("sp", res["durationSum"], "sa", sa["durationSum"], sa["unvisited"])
    assert (0, res["durationSum"]) <= (len(sa["unvisited"]), sa["durationSum"])


@pytest.mark.gpu
def test_run_errors_launch_nothing(ctx):
    import torch
    from vrpms_amd.core import CVRP, TSP, Context
    lib = ctx.lib
    n = 6
    D, dem, caps = matrix("sym", n + 1, 2), demands(n, 2), [16, 14]
    need = ctypes.c_uint64()
    assert lib.vrpms_vrp_sp_workspace(n, 2, ctypes.byref(need)) == 0
    work = torch.zeros(need.value, dtype=torch.uint8, device=ctx.dev)
    tour = torch.full((n + 2,), -7, dtype=torch.int16, device=ctx.dev)
    key = torch.full((1,), -7, dtype=torch.int64, device=ctx.dev)

    def run(nn=n, nbytes=None, off=0, handle=None):
        return lib.vrpms_vrp_sp_run(ctx.handle if handle is None else handle, nn,
                                    work.data_ptr() + off,
                                    need.value if nbytes is None else nbytes, tour.data_ptr(),
                                    key.data_ptr(), ctx.stream())

    ctx.set_instance(TSP, D, start_times=(0,))
    assert run() == _lib.VRPMS_EINVAL and b"CVRP only" in lib.vrpms_last_error()
    ctx.set_instance(CVRP, np.stack([D] * 24), dem, caps, [0, 0])
    assert run() == _lib.VRPMS_EINVAL and b"static" in lib.vrpms_last_error()
    ctx.set_instance(CVRP, D, dem, caps, [0, 0])
    assert run(nbytes=need.value - 1) == _lib.VRPMS_EINVAL
    assert b"too small" in lib.vrpms_last_error()
    assert run(off=2) == _lib.VRPMS_EINVAL and b"aligned" in lib.vrpms_last_error()
    assert run(nn=n + 1) == _lib.VRPMS_EINVAL and b"min(20, N-1)" in lib.vrpms_last_error()
    assert run(nn=0) == _lib.VRPMS_EINVAL
    for args in [(None, need.value, tour.data_ptr(), key.data_ptr()),
                 (work.data_ptr(), need.value, None, key.data_ptr()),
                 (work.data_ptr(), need.value, tour.data_ptr(), None)]:
        assert lib.vrpms_vrp_sp_run(ctx.handle, n, *args, ctx.stream()) == _lib.VRPMS_EINVAL
        assert b"NULL" in lib.vrpms_last_error()
    with Context(ctx.device) as fresh:      # no instance loaded
        assert run(handle=fresh.handle) == _lib.VRPMS_ESTATE
        assert b"no instance" in lib.vrpms_last_error()
    torch.cuda.synchronize(ctx.dev)
    assert tour.cpu().tolist() == [-7] * (n + 2) and key.cpu().item() == -7
    assert int(work.max().item()) == 0
    # and the same buffers serve a valid call
    assert run() == _lib.VRPMS_OK
    ref = sp_ref(D, dem, caps, "sum")
    assert tour.cpu().tolist() == ref["tour"] and key.cpu().item() == ref["key"]


def _service_instance():
    """A 12-node matrix of which rows 0 (depot), 1, 3, 4, 6, 8, 9, 11 take
    part: locations 2, 5 are ignored, 7 and 10 completed."""
    D = matrix("asym", 12, 30)
    locs = [{"id": 100 + i, "demand": int(d)} for i, d in enumerate(demands(11, 30, 1, 4))]
    active = [1, 3, 4, 6, 8, 9, 11]
    return D, locs, active, [102, 105], [107, 110]


@pytest.mark.gpu
@pytest.mark.parametrize("objective", ["sum", "max"])
def test_solve_vrp_sp_schema_and_optimum(objective):
    D, locs, active, ignored, completed = _service_instance()
    caps, starts = [7, 6, 5], [0, 15, 30]
    res = solver.solve_vrp("sp", D.tolist(), locs, caps, starts, ignored, completed,
                           objective=objective, seed=3, time_limit=0.001, with_unvisited=True)
    assert set(res) == {"durationMax", "durationSum", "vehicles", "unvisited"}
    nodes = [0] + active
    sub = D[np.ix_(nodes, nodes)]
    dem = np.array([0] + [locs[i]["demand"] for i in active])
    ref = sp_ref(sub, dem, caps, objective)
    assert [v["tour"] for v in res["vehicles"]] == [[0] + [nodes[c] for c in r] + [0]
                                                   for r in ref["routes"]]
    assert [v["duration"] for v in res["vehicles"]] == ref["durations"]
    assert res["durationSum"] == sum(ref["durations"])
    assert res["durationMax"] == max(ref["durations"])
    served = {c for r in ref["routes"] for c in r}
    assert res["unvisited"] == [nodes[c] for c in range(1, 8) if c not in served]
    # a device list: sp runs on the first, like dp not as an island model
    again = solver.solve_vrp("sp", D.tolist(), locs, caps, starts, ignored, completed,
                             objective=objective, devices=[0, 0], with_unvisited=True)
    assert again == res
    # no customer left: the empty answer of every algorithm
    none = solver.solve_vrp("sp", D.tolist(), locs, caps, starts, [100 + i for i in range(1, 12)])
    assert none == {"durationMax": 0, "durationSum": 0,
                    "vehicles": [{"tour": [0, 0], "duration": 0}] * 3}


@pytest.mark.gpu
def test_post_solve_vrp_sp_end_to_end():
    D, locs, active, ignored, completed = _service_instance()
    caps, starts = [7, 6, 5], [0, 15, 30]
    want = solver.solve_vrp("sp", D.tolist(), locs, caps, starts, ignored, completed,
                            objective="max")
    srv = service.serve(service.App(_store()), "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    try:
        base = f"http://127.0.0.1:{srv.server_address[1]}"
        got = remote.solve_vrp("sp", D.tolist(), locs, caps, starts, ignored, completed,
                               objective="max", base=base)
        with pytest.raises(ValueError, match="at most 64 vehicles"):
            remote.solve_vrp("sp", D.tolist(), locs, [1] * 65, [0] * 65, base=base)
    finally:
        srv.shutdown()
        srv.server_close()
    assert got == want and set(got) == {"durationMax", "durationSum", "vehicles"}
    assert len(got["vehicles"]) == 3 and got["durationMax"] == max(v["duration"] for v in got["vehicles"])
