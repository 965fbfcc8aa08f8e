"""The original search path under the max-duration objective (A8, objective
1): the five SA kernels, both ACO constructions and update paths, both GA
paths, bf_kernel and solve_vrp(..., objective="max"), each against the C or
Python oracle under objective 1 for equality.  The cases are
tests/objective_cases.py's; test_objective_cases_cpu.py proves, without a
GPU, that each of them gives another answer under objective 0, so a kernel
that ignored the objective or mispriced the longest route cannot pass here.
There are no tolerances: every cost is an integer and every random choice a
Philox word both sides compute."""
import json
import math

import numpy as np
import pytest

import objective_cases as oc
from oracle import search, spec
from test_sa_td_gpu import load, run
from vrpms_amd import synth

pytestmark = pytest.mark.gpu


def torch_():
    import torch
    return torch


def u64(t):
    return [int(x) & (2**64 - 1) for x in t.reshape(-1).cpu().tolist()]


def i64(k):
    """A uint64 key as the int64 a torch tensor holds."""
    return k - (1 << 64) if k >= 1 << 63 else k


def same(a, b):
    return (a[0] == b[0]).all() and a[1] == b[1] and (a[2] == b[2]).all() and a[3] == b[3]


def scorer(inst, objective=1):
    return search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times,
                         inst.problem, objective)


# ---------------------------------------------------------------------------
# 1. SA
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in oc.SA_CASES])
def test_sa_objective_max_matches_c_restatement(ctx, name):
    """cur, cur_key, best and best_key bit-equal to coracle.sa_run(objective=1)
    through the kernel the automatic dispatch reaches (objective_cases.py names
    it per case; the layout fields that decide it are asserted first) and
    through every forced mode that applies, cold and -- for the segment, route
    and hour-row kernels -- hot, where every step is accepted and the tables
    are rebuilt around a zone the max chose."""
    c, inst, P = oc.sa_case(name)
    load(ctx, inst, 1)
    lay = ctx.instance_layout(P.shape[1])
    assert {k: lay[k] for k in c.expect} == c.expect
    for inv_t0 in c.temps:
        want = oc.sa_reference(name, inv_t0)
        args = (c.steps, inv_t0, oc.INV_ALPHA, oc.SEED, oc.STEP0, c.window, c.types, c.moves)
        auto = run(ctx, P, *args, 0)
        assert same(auto, want), (name, inv_t0)
        assert (auto[0] != P).any()
        for mode in c.modes:
            forced = run(ctx, P, *args, mode)
            assert same(forced, want), (name, inv_t0, mode)
        if c.split2:
            # without the fast split the packed kernel declines: auto is sa_seg_kernel
            # (static, symmetric), 2 sa_kernel, 3 (windowed) sa_route_kernel
            ctx.set_split_mode(2)
            try:
                assert not ctx.instance_layout(P.shape[1])["fast"]
                for mode in (0, 2) + ((3,) if c.window else ()):
                    other = run(ctx, P, *args, mode)
                    assert same(other, want), (name, inv_t0, "split2", mode)
            finally:
                ctx.set_split_mode(0)


# ---------------------------------------------------------------------------
# 2. the secondary field saturated, the primary not
# ---------------------------------------------------------------------------
def test_saturated_secondary_scoring_matches_oracle(ctx, coracle):
    """vrpms_eval of all 120 first-fit tours of the saturation instance: keys,
    sums, maxs and unvisited counts equal coracle.eval_batch(objective=1);
    every key has its secondary field at the clamp and its primary below."""
    inst, P = oc.saturated(), oc.saturated_tours()
    load(ctx, inst, 1)
    assert not ctx.instance_layout(7)["use16"]
    dP = torch_().from_numpy(P).to(ctx.dev)
    keys, sums, maxs, unv = ctx.eval(dP, n=7, with_parts=True)
    ref = coracle.eval_batch(inst.durations, P, inst.demand, inst.capacities, inst.start_times,
                             1, 1, n=7)
    got = keys.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got, ref[0])
    np.testing.assert_array_equal(sums.cpu().numpy(), ref[1])
    np.testing.assert_array_equal(maxs.cpu().numpy(), ref[2])
    np.testing.assert_array_equal(unv.cpu().numpy(), ref[3])
    clamp = np.uint64(spec.KEY_CLAMP)
    assert ((got & clamp) == clamp).all() and (((got >> np.uint64(28)) & clamp) < clamp).all()
    assert (sums.cpu().numpy() > spec.KEY_CLAMP).all() and (got >> np.uint64(56) == 0).all()


def test_saturated_secondary_sa_matches_c_restatement(ctx, coracle):
    """4 chains x 40 steps on the saturation instance: the automatic dispatch
    (sa_seg_kernel<int32>: static, symmetric, entries past 65535) and sa_kernel
    (mode 2) equal the C restatement under objective 1."""
    inst, P = oc.saturated(), oc.saturated_starts()
    load(ctx, inst, 1)
    lay = ctx.instance_layout(7)
    assert not lay["use16"] and lay["symmetric"] and not lay["fast"]
    want = oc.oracle_sa(coracle, inst, P, oc.SAT_STEPS, oc.SAT_INV_T0, 0, 0, 64, 1)
    for mode in (0, 2):
        got = run(ctx, P, oc.SAT_STEPS, oc.SAT_INV_T0, oc.INV_ALPHA, oc.SEED, oc.STEP0, 0, 0, 64,
                  mode)
        assert same(got, want), mode
        assert all(spec.unpack_key(k)[2] == spec.KEY_CLAMP > spec.unpack_key(k)[1]
                   for k in got[1] + got[3])


# ---------------------------------------------------------------------------
# 3. ACO
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.ACO_CASES))
def test_aco_objective_max_matches_oracle(ctx, name):
    """Tours, keys, iteration bests, tau after each iteration and the
    best-so-far equal oracle/search.py aco_iteration under objective 1, in
    every construction mode the case lists (all modes give the same arrays)."""
    torch = torch_()
    case = oc.ACO_CASES[name]
    inst = oc.aco_instance(name)
    load(ctx, inst, 1)
    want = oc.aco_reference(name)
    bt0, bk0 = oc.aco_best_start(name)
    for mode in case["modes"]:
        ctx.set_aco_construct(mode)
        try:
            tau, eta = ctx.aco_init(oc.ACO_COLONIES, oc.ACO_TAU0)
            bt = torch.tensor(bt0, dtype=torch.int16, device=ctx.dev)
            bk = torch.tensor([i64(k) for k in bk0], dtype=torch.int64, device=ctx.dev)
            for it in range(oc.ACO_ITERS):
                tours, keys, ib = ctx.aco_iteration(tau, eta, oc.ACO_ANTS, seed=oc.ACO_SEED, it=it,
                                                    evap_shift=3, tau_min=1 << 10,
                                                    tau_max=1 << 30, best_tours=bt, best_keys=bk,
                                                    bsf_period=case["bsf_period"])
                rt, rk, rib, rtau, rbt, rbk = want[it]
                assert tours.cpu().numpy().tolist() == rt, (mode, it)
                assert u64(keys) == rk, (mode, it)
                assert [(a & (2**64 - 1), b) for a, b in ib.cpu().tolist()] == rib, (mode, it)
                got_tau = tau.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
                assert all((got_tau[c] == rtau[c]).all() for c in range(oc.ACO_COLONIES)), (mode, it)
                assert bt.cpu().numpy().tolist() == rbt and u64(bk) == rbk, (mode, it)
        finally:
            ctx.set_aco_construct(0)


# ---------------------------------------------------------------------------
# 4. GA, brute force, TSP
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.GA_CASES))
def test_ga_objective_max_matches_oracle(ctx, name):
    """Populations and keys after GA_GENS generations equal oracle/search.py
    ga_generation under objective 1, fused (auto) and three-kernel (2) alike."""
    torch = torch_()
    inst, P = oc.ga_case(name)
    load(ctx, inst, 1)
    k0, rpop, rkeys = oc.ga_reference(name)
    out = []
    for mode in oc.GA_CASES[name]["modes"]:
        ctx.set_ga_fused(mode)
        try:
            dpop = torch.from_numpy(P.copy()).to(ctx.dev)
            keys = ctx.eval(dpop.view(oc.GA_ISLANDS * oc.GA_POP, inst.n)).view(oc.GA_ISLANDS,
                                                                                oc.GA_POP)
            assert u64(keys) == k0
            ctx.ga_generation(dpop, keys, generations=oc.GA_GENS, pmut=oc.GA_PMUT, seed=oc.GA_SEED,
                              gen0=oc.GA_GEN0)
            out.append((dpop.cpu().numpy().tolist(), u64(keys)))
        finally:
            ctx.set_ga_fused(0)
    for pop, keys in out:
        assert pop == rpop and keys == rkeys
    assert out[0] == out[-1]


@pytest.mark.parametrize("name", list(oc.BF_CASES))
def test_bf_objective_max_matches_c_restatement(ctx, coracle, name):
    """bf_kernel over the whole rank range and over two unequal windows: key,
    rank and tour equal coracle.bf(objective=1)."""
    inst = oc.bf_instance(name)
    n = inst.n
    load(ctx, inst, 1)
    sc = scorer(inst)
    got = []
    for a, b in oc.bf_windows(n):
        k, r = ctx.bf_run(n, a, b)
        assert (k, r) == coracle.bf(inst.durations, n, a, b, objective=1, **oc.bf_kw(inst)), (a, b)
        assert a <= r < b and sc(search.unrank(r, n)) == k
        got.append((k, r))
    assert min(got[1:]) == got[0]
    # the objective is read: objective 0's optimum is another tour
    load(ctx, inst, 0)
    assert ctx.bf_run(n, 0, math.factorial(n))[1] != got[0][1]


def test_tsp_keys_do_not_depend_on_the_objective(ctx, coracle):
    """A TSP key is duration << 28 under either objective: SA (sa_kernel) and
    brute force give the same tours, keys and ranks loaded with 0 and with 1,
    and they are the C oracle's."""
    inst = oc.tsp_instance()
    n, chains = inst.n, 4
    P = synth.random_perms(chains, n, seed=9, dtype=np.uint16)
    want = oc.oracle_sa(coracle, inst, P, 40, oc.COLD, 0, 0, 64, 0)
    full = math.factorial(n)
    bf = coracle.bf(inst.durations, n, 0, full, **oc.bf_kw(inst))
    for objective in (0, 1):
        load(ctx, inst, objective)
        got = run(ctx, P, 40, oc.COLD, oc.INV_ALPHA, oc.SEED, oc.STEP0, 0, 0, 64, 0)
        assert same(got, want), objective
        assert ctx.bf_run(n, 0, full) == bf
        assert bf[0] == spec.tsp_key(spec.eval_tsp(inst.durations, search.unrank(bf[1], n),
                                                   int(inst.start_times[0])))


# ---------------------------------------------------------------------------
# 5. the front door
# ---------------------------------------------------------------------------
_SOLVED = {}


def solved(kind, algo, objective="max"):
    """solve_vrp's answer, computed once per (instance, algorithm, objective)."""
    from vrpms_amd import solver
    key = (kind, algo, objective)
    if key not in _SOLVED:
        _SOLVED[key] = solver.solve_vrp(algo, *oc.front_args(oc.front(kind)), objective=objective,
                                        seed=oc.FRONT_SEED, **oc.FRONT_KNOBS[algo])
    return _SOLVED[key]


def route_cost(D, tour, start):
    t = start
    for a, b in zip(tour, tour[1:]):
        t += int(D[(t // 60) % D.shape[0], a, b])
    return t - start


@pytest.mark.parametrize("algo", ["bf", "sa", "ga", "aco"])
@pytest.mark.parametrize("kind", ["static", "td"])
def test_solve_vrp_objective_max(coracle, kind, algo):
    """The result dict of solve_vrp(algo, ..., objective="max"): the schema,
    every duration recomputed on the host, brute force's durationMax equal to
    the primary field of coracle.bf(objective=1) and no larger than under
    "sum", and no heuristic below brute force (objective_cases.front says why
    that bound holds for SA's separator tours too)."""
    inst = oc.front(kind)
    res = solved(kind, algo)
    assert set(res) == {"durationMax", "durationSum", "vehicles"}
    assert len(res["vehicles"]) == inst.K
    served = []
    for v, st in zip(res["vehicles"], inst.start_times):
        assert v["tour"][0] == v["tour"][-1] == 0
        served += v["tour"][1:-1]
        assert v["duration"] == (route_cost(inst.durations, v["tour"], int(st))
                                 if len(v["tour"]) > 2 else 0)
    assert sorted(served) == list(range(1, inst.N))
    assert res["durationSum"] == sum(v["duration"] for v in res["vehicles"])
    assert res["durationMax"] == max(v["duration"] for v in res["vehicles"])
    bf = solved(kind, "bf")
    key, rank = coracle.bf(inst.durations, inst.n, 0, math.factorial(inst.n), objective=1,
                           **oc.bf_kw(inst))
    assert spec.unpack_key(key) == (0, bf["durationMax"], bf["durationSum"])
    assert bf["durationMax"] <= solved(kind, "bf", "sum")["durationMax"]
    assert res["durationMax"] >= bf["durationMax"]
    if algo == "bf":
        tour = [c for v in res["vehicles"] for c in v["tour"][1:-1]]
        assert tour == search.unrank(rank, inst.n)


def test_solve_inline_objective_max_equals_the_direct_call():
    """POST /solve/vrp/sa with "objective": "max": 200 and solve_vrp's message."""
    from test_service_cpu import store
    from vrpms_amd import service
    D, locs, caps, starts = oc.front_args(oc.front("static"))
    body = {"durations": D, "locations": locs, "capacities": caps, "startTimes": starts,
            "ignoredCustomers": [], "completedCustomers": [], "seed": oc.FRONT_SEED,
            "objective": "max", "knobs": oc.FRONT_KNOBS["sa"]}
    status, resp = service.App(store()).solve_inline("vrp", "sa", json.dumps(body).encode())
    assert status == 200 and resp["success"]
    assert resp["message"] == solved("static", "sa")
