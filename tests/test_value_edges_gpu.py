"""The kernels on the value-range edges of tests/value_edges.py: instances
that sit on the thresholds where vrpms_set_instance and fast_split_params
change layout (uint16 matrix, packed field widths, the prefix-ret load and
duration fields, the vehicle counter, the carry form), on the A9 int32 guards
and on the A8 key clamps.  test_value_edges_cpu.py proves each instance's
premise; here every case first asserts, through vrpms_instance_layout and
vrpms_eval_path, that the device took the layout it aims at, then compares
keys, sums, maxs and unvisited counts for equality with the oracle."""
import numpy as np
import pytest

import value_edges as ve
from oracle import search, spec
from test_eval_gpu import check_batch, check_words, load, upload
from vrpms_amd import _lib

pytestmark = pytest.mark.gpu


def torch_():
    import torch
    return torch


def u64(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint64).reshape(-1)]


@pytest.fixture
def options(ctx):
    """Reset every kernel-variant option a test may force."""
    yield ctx
    ctx.set_words_kernel(0)
    ctx.set_rows_config(0)
    ctx.set_words_ilp(0)
    ctx.set_words_lookahead(0)
    ctx.set_ga_fused(0)
    ctx.set_split_mode(0)


def assert_layout(ctx, e, n):
    """The device chose what the Python model of the host conditions says,
    and (at the edge's own tour length) what the edge was built to reach."""
    lay = ctx.instance_layout(n)
    model = ve.model_layout(e.inst, n)
    assert {k: lay[k] for k in model} == model, e.name
    if n == e.n:
        assert {k: lay[k] for k in e.expect} == e.expect, e.name
    return lay


@pytest.mark.parametrize("name,side", ve.SIDES, ids=ve.SIDE_IDS)
def test_scoring_on_the_edge(ctx, coracle, name, side):
    from vrpms_amd.core import VrpmsError
    e = ve.pair(name)[side]
    if e.refused:                       # one past the largest accepted instance
        with pytest.raises(VrpmsError) as err:
            load(ctx, e.inst)
        assert err.value.code == _lib.VRPMS_ERANGE
        return
    for P, n in ((e.P, e.n), (e.Psep, e.n + e.n_sep)):
        if P is None:
            continue
        load(ctx, e.inst, e.objective)
        assert_layout(ctx, e, n)
        # rows wider than 128 bytes leave the LDS-tile kernels for eval_staged
        path = e.path if P.shape[1] <= 128 else 2
        keys = check_batch(ctx, coracle, e.inst, P, n=n, objective=e.objective, expect_path=path)
        if e.words and e.inst.N <= 256:
            check_words(ctx, coracle, e.inst, P, n, objective=e.objective)
        if "clamp" in e.needs:          # A8: both 28-bit fields saturate, the parts do not
            both = ((keys >> np.uint64(28)) & np.uint64(spec.KEY_CLAMP) == spec.KEY_CLAMP) & \
                (keys & np.uint64(spec.KEY_CLAMP) == spec.KEY_CLAMP)
            assert both.sum() >= ve.WAVE
            sums = ctx.eval(upload(ctx, P), n=n, with_parts=True)[1].cpu().numpy()
            assert (sums[both] > spec.KEY_CLAMP).all()
        if "unv" in e.needs:            # A8: the key holds min(unv, 255), d_unv the count
            unv = ctx.eval(upload(ctx, P), n=n, with_parts=True)[3].cpu().numpy()
            assert (unv == e.quantity).all()
            assert ((keys >> np.uint64(56)) == min(e.quantity, spec.UNV_CLAMP)).all()


@pytest.mark.parametrize("objective", [0, 1])
def test_fast_split_limit_every_rows_and_words_variant(options, coracle, objective):
    """E4 inside, (cap + max_dem + 3) << S == 2^31: every forced (CW, ILP) of
    eval_cvrp_rows2, eval_cvrp_packed, and every (ILP, look-ahead) of
    eval_cvrp_words2, all equal to the oracle."""
    from vrpms_amd.core import VrpmsError
    ctx = options
    e = ve.pair("e4_max" if objective else "e4")[0]
    load(ctx, e.inst, objective)
    lay = assert_layout(ctx, e, e.n)
    assert lay["fast"] and lay["carry"] and (e.inst.capacities[0] + 255 + 3) << lay["pref_S"] == 2**31
    ctx.set_words_kernel(1)             # eval_cvrp_packed MODE 1
    ref = check_batch(ctx, coracle, e.inst, e.P, n=e.n, objective=objective, expect_path=0)
    ctx.set_words_kernel(0)
    for cfg in range(6):
        ctx.set_rows_config(cfg)
        for P, n in ((e.P, e.n), (e.Psep, e.n + e.n_sep)):
            try:
                got = check_batch(ctx, coracle, e.inst, P, n=n, objective=objective, expect_path=0)
            except VrpmsError as err:   # a forced tile that does not fit is refused, never wrong
                assert cfg > 0 and "does not fit" in str(err)
                continue
            if P is e.P:
                np.testing.assert_array_equal(got, ref)
    ctx.set_rows_config(0)
    for ilp, la in ((2, 1), (2, 2)):
        ctx.set_words_ilp(ilp)
        ctx.set_words_lookahead(la)
        for mode in (0, 3):             # the carry form and the sign-compare form
            ctx.set_split_mode(mode)
            check_words(ctx, coracle, e.inst, e.P, e.n, objective=objective)
            check_words(ctx, coracle, e.inst, e.Psep, e.n + e.n_sep, objective=objective)
        ctx.set_split_mode(0)


# ---------------------------------------------------------------------------
# Search kernels on the same FastSplit, against the Python-int replays
# ---------------------------------------------------------------------------
SMALL = ["e4_in", "e4_out", "e3_in"]


def load_small(ctx, kind, objective=0):
    inst = ve.small(kind)
    load(ctx, inst, objective)
    lay = ctx.instance_layout()
    model = ve.model_layout(inst)
    assert {k: lay[k] for k in model} == model
    assert lay["pref_S"] == 8 and lay["fast"] == (kind == "e4_in")
    sc = search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times, "cvrp",
                       objective)
    return inst, sc


@pytest.mark.parametrize("window", [0, 3], ids=["unwindowed", "windowed"])
@pytest.mark.parametrize("kind", SMALL)
def test_sa_on_the_load_field_limit(ctx, kind, window):
    torch = torch_()
    inst, sc = load_small(ctx, kind)
    chains, n = 4, inst.n
    P = ve.synth.random_perms(chains, n, seed=7).astype(np.int16)
    P[0] = [1, 5, 6, 2, 3, 4, 7, 8, 9, 10, 11, 12]      # starts on a full vehicle (e4)
    cur = torch.from_numpy(P).to(ctx.dev)
    best = cur.clone()
    ck = torch.empty(chains, dtype=torch.int64, device=ctx.dev)
    bk = torch.full((chains,), -1, dtype=torch.int64, device=ctx.dev)
    args = dict(steps=12, inv_t0=1 / 8.0, inv_alpha=1 / 0.97, seed=41, step0=2)
    ctx.sa_run(cur, ck, best, bk, window=window, **args)
    ref = search.sa_run(sc, P.tolist(), P.tolist(), [2**64 - 1] * chains, 41, 2, 12, 1 / 8.0,
                        1 / 0.97, window=window)
    assert cur.cpu().numpy().tolist() == ref[0]
    assert u64(ck) == ref[1]
    assert best.cpu().numpy().tolist() == ref[2]
    assert u64(bk) == ref[3]


@pytest.mark.parametrize("fused", [0, 2], ids=["fused", "three_kernels"])
@pytest.mark.parametrize("kind", SMALL)
def test_ga_on_the_load_field_limit(options, kind, fused):
    torch = torch_()
    ctx = options
    inst, sc = load_small(ctx, kind, objective=1)
    ctx.set_ga_fused(fused)
    islands, pop, n = 3, 10, inst.n
    P = ve.synth.random_perms(islands * pop, n, seed=4).astype(np.int16)
    dpop = torch.from_numpy(P.reshape(islands, pop, n).copy()).to(ctx.dev)
    keys = ctx.eval(dpop.view(-1, n)).view(islands, pop)
    rpop = [[list(r) for r in P.reshape(islands, pop, n)[i]] for i in range(islands)]
    rkeys = [[sc(t) for t in rpop[i]] for i in range(islands)]
    assert u64(keys) == [k for ks in rkeys for k in ks]
    pm = min(int(round(0.6 * 2**32)), 2**32 - 1)
    for g in range(4):
        rpop, rkeys = search.ga_generation(sc, rpop, rkeys, 55, g, pm)
    ctx.ga_generation(dpop, keys, generations=4, pmut=0.6, seed=55, gen0=0)
    assert dpop.cpu().numpy().tolist() == rpop
    assert u64(keys) == [k for ks in rkeys for k in ks]


@pytest.mark.parametrize("kind", SMALL)
def test_aco_on_the_load_field_limit(ctx, kind):
    inst, sc = load_small(ctx, kind)
    colonies, ants, tau0 = 2, 8, 1 << 20
    tau, eta = ctx.aco_init(colonies, tau0)
    ref_eta = search.aco_eta(inst.durations[0])
    rtau = [np.full((inst.N, inst.N), tau0, dtype=np.int64) for _ in range(colonies)]
    for it in range(3):
        tours, keys, ib = ctx.aco_iteration(tau, eta, ants, seed=7, it=it, evap_shift=3,
                                            tau_min=1 << 10, tau_max=1 << 30)
        rt, rk, rib = search.aco_iteration(sc, rtau, ref_eta, ants, inst.n, 7, it, 3, 1 << 10,
                                           1 << 30)
        assert tours.cpu().numpy().tolist() == rt
        assert u64(keys) == [k for ks in rk for k in ks]
        assert [(a & (2**64 - 1), b) for a, b in ib.cpu().tolist()] == rib
        got_tau = tau.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        assert all((got_tau[c] == rtau[c]).all() for c in range(colonies))


# ---------------------------------------------------------------------------
# Exact and enumerating kernels on the largest instances the A9 guard admits
# ---------------------------------------------------------------------------
N_EXACT = 6                             # depot + 5 customers: 120 tours, 2,520 with 2 separators


def limit_matrix(kind, bound_edges, seed, H=1, max_dur=None):
    """max_dur = floor((2^31 - 1) / bound_edges), the largest the guard
    admits.  "big": every entry in its upper half, so every key field clamps
    and partial sums pass 2^30; "mixed": half of the entries at most 1,000,
    so the optimum is small while most table states hold huge sums."""
    rng = np.random.default_rng(seed)
    md = (2**31 - 1) // bound_edges if max_dur is None else max_dur
    D = rng.integers(md // 2, md + 1, size=(H, N_EXACT, N_EXACT), dtype=np.int64)
    if kind == "mixed":
        D = np.where(rng.random(D.shape) < 0.5, rng.integers(1, 1001, size=D.shape), D)
    D[:, np.arange(N_EXACT), np.arange(N_EXACT)] = 0
    D[:, 0, 1] = md
    return D, md


def tsp_optimum(D, start):
    """(least duration, the tours attaining it) by enumeration in Python ints."""
    import itertools
    durs = {p: spec.eval_tsp(D, p, start) for p in itertools.permutations(range(1, N_EXACT))}
    best = min(durs.values())
    return best, [list(p) for p, d in durs.items() if d == best]


def cvrp_optimum(D, dem, caps, starts, objective):
    """Least (unvisited, primary) over every arrangement of the customers and
    K separators, each scored by spec.eval_cvrp in Python ints."""
    import itertools
    tokens = list(range(1, N_EXACT)) + [0] * len(caps)
    best = None
    for t in sorted(set(itertools.permutations(tokens))):
        r = spec.eval_cvrp(D, t, dem, caps, starts, objective)
        v = (r["unvisited"], r["max"] if objective else r["sum"])
        best = v if best is None or v < best else best
    return best


def limit_tsp(kind):
    D, md = limit_matrix(kind, N_EXACT + 2, seed=11)
    start = 2**31 - 1 - (N_EXACT + 2) * md
    inst = ve.synth.Instance(f"limit_tsp_{kind}", D, None, None, np.array([start]), "tsp")
    assert ve.accepted(inst) and start + (N_EXACT + 2) * md == 2**31 - 1
    return inst


DEM_EXACT, CAPS_EXACT = np.array([0, 2, 1, 3, 2, 1]), np.array([5, 4])


def limit_cvrp(kind):
    D, md = limit_matrix(kind, N_EXACT + 3, seed=12)
    start = 2**31 - 1 - (N_EXACT + 3) * md
    inst = ve.synth.Instance(f"limit_cvrp_{kind}", D, DEM_EXACT, CAPS_EXACT, np.array([start, 0]),
                             "cvrp")
    assert ve.accepted(inst) and start + (N_EXACT + 3) * md == 2**31 - 1
    return inst


@pytest.mark.parametrize("kind", ["big", "mixed"])
def test_tsp_exact_entries_at_the_int32_limit(ctx, kind):
    torch = torch_()
    import math
    inst = limit_tsp(kind)
    n, start = inst.n, int(inst.start_times[0])
    best, tours = tsp_optimum(inst.durations, start)
    assert (best > spec.KEY_CLAMP) == (kind == "big")
    load(ctx, inst)
    sc = search.Scorer(inst.durations, None, None, inst.start_times, "tsp")
    got = ctx.bf_run(n, 0, math.factorial(n))
    assert got == search.bf(sc, n) and got[0] == spec.tsp_key(best)
    key, tour = ctx.tsp_dp(n)
    assert key == spec.tsp_key(best) and tour in tours
    assert tour == min(tours)                        # the lexicographically smallest optimum
    # the batched entry: N * max(mats) < 2^31 is its caller's promise
    mats = np.stack([limit_matrix(k, N_EXACT, seed=13)[0][0] for k in ("big", "mixed")])
    assert N_EXACT * int(mats.max()) < 2**31 <= N_EXACT * (int(mats.max()) + 1)
    bt, bk = ctx.tsp_batch_dp(torch.tensor(mats, dtype=torch.int32, device=ctx.dev))
    for r in range(2):
        b, ts = tsp_optimum(mats[r], 0)
        assert u64(bk)[r] == spec.tsp_key(b) and bt.cpu().tolist()[r] == min(ts)


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("kind", ["big", "mixed"])
def test_cvrp_exact_entries_at_the_int32_limit(ctx, kind, objective):
    torch = torch_()
    import math
    inst = limit_cvrp(kind)
    n, K = inst.n, inst.K
    args = (inst.durations, inst.demand, inst.capacities, inst.start_times)
    load(ctx, inst, objective)
    sc = search.Scorer(*args, "cvrp", objective)
    assert ctx.bf_run(n, 0, math.factorial(n)) == search.bf(sc, n)
    best = cvrp_optimum(*args, objective)
    key, tour = ctx.vrp_sp(n)
    r = spec.eval_cvrp(inst.durations, tour, *args[1:], objective)
    assert key == r["key"] and (r["unvisited"], r["max"] if objective else r["sum"]) == best
    if kind == "big":
        assert (key >> 28) & spec.KEY_CLAMP == spec.KEY_CLAMP == key & spec.KEY_CLAMP
    M = torch.tensor(inst.durations, dtype=torch.int32, device=ctx.dev)
    dm = torch.tensor(inst.demand[None], dtype=torch.int32, device=ctx.dev)
    cp = torch.tensor(inst.capacities[None], dtype=torch.int32, device=ctx.dev)
    bt, bk, bd = ctx.vrp_batch_sp(M, dm, cp, objective)
    assert (bt.cpu().tolist()[0], u64(bk)[0]) == (tour, key)
    assert bd.cpu().tolist()[0] == r["durations"]    # unclamped


@pytest.mark.parametrize("objective", [0, 1])
def test_time_expanded_entries_with_the_start_time_at_the_int32_limit(ctx, objective):
    """H = 24, start + (N + K + 1) * max_dur == 2^31 - 1 and start + horizon
    == 2^31 - 1: hour indices and clock words next to 2^31."""
    md = 100
    D, _ = limit_matrix("big", 0, seed=14, H=24, max_dur=md)
    horizon = (N_EXACT + 2) * md
    start = 2**31 - 1 - horizon
    inst = ve.synth.Instance("limit_tdp", D, None, None, np.array([start]), "tsp")
    assert ve.accepted(inst)
    load(ctx, inst)
    best, tours = tsp_optimum(D, start)
    key, tour = ctx.tsp_tdp(inst.n, horizon)
    assert key == spec.tsp_key(best) and tour in tours
    horizon = (N_EXACT + 3) * md
    starts = np.array([2**31 - 1 - horizon, 2**31 - 1 - horizon - 61])
    inst = ve.synth.Instance("limit_tdsp", D, DEM_EXACT, CAPS_EXACT, starts, "cvrp")
    assert ve.accepted(inst) and int(starts[0]) + horizon == 2**31 - 1
    load(ctx, inst, objective)
    args = (D, DEM_EXACT, CAPS_EXACT, starts)
    key, tour = ctx.vrp_tdsp(inst.n, horizon)
    r = spec.eval_cvrp(D, tour, *args[1:], objective)
    assert key == r["key"]
    assert (r["unvisited"], r["max"] if objective else r["sum"]) == cvrp_optimum(*args, objective)
