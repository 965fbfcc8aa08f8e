"""Runtime hour counts: every kernel's HM = 0 instantiation (hour_of<0>,
``(t / 60) % H`` with a run-time divisor), which vrpms_set_instance accepts
for any H in [1, 1024] but no H in {1, 24} ever launches.

The oracles (oracle/spec.py A3, oracle/oracle_c.c) define any H.  The CPU
half of this file proves the cases are not vacuous: on every (instance, H,
tours) used below, the spec's keys change for at least 90 % of the tours
when the matrix is misread as slice 0 only, or (H > 24) the hour is taken
modulo 24.  The GPU half compares for equality; there are no tolerances.

Which kernel a case reaches is read from the launchers (eval.hip vrpms_eval,
eval_staged.hip launch_staged / staged_mat, search.hip vrpms_sa_run /
launch_inst) and written beside the case.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

from oracle import search, spec
from vrpms_amd import _lib, synth

gpu = pytest.mark.gpu


def torch_():
    import torch
    return torch


def with_hours(inst, H, first=0, asym=False, seed=0):
    """`inst` (one of synth.td_cvrp's, 24 hourly slices) with H slices:
    slice h is the instance's slice (first + h) % 24, as it is for h < 24 and
    times 2, 3 or 4 (by h // 24) from slice 24 on, so slice 24 differs from
    slice 0 and a kernel that wrapped the hour at 24 reads other durations.
    `first` picks the hour that becomes slice 0: the generator's hours 0..5
    are all its base matrix, so a small H starts at the morning peak
    (first = 7: factors 1.5, 1.8, 1.5, 1.2, 1, ...) to have slices that
    differ.  asym: slice 0 stays symmetric, every other slice gets
    upper-triangle noise -- the instance a kernel trusting
    Instance::symmetric (slice 0 only) for a reversed edge would misprice."""
    D24 = np.asarray(inst.durations, dtype=np.int64)
    assert D24.shape[0] == 24
    h = np.arange(H)
    fac = np.where(h < 24, 1, 2 + (h // 24) % 3)
    D = D24[(first + h) % 24] * fac[:, None, None]
    if asym:
        rng = np.random.default_rng(seed)
        N = D.shape[1]
        D[1:] += np.triu(rng.integers(1, 40, size=(H - 1, N, N)), 1)
    return dataclasses.replace(inst, name=f"{inst.name}_h{H}", durations=D)


def as_tsp(inst, start):
    return synth.Instance(inst.name + "_tsp", inst.durations, None, None, np.array([start]), "tsp")


def het_flex(inst):
    """Per-vehicle capacities with min(cap) < max(demand): the split skips
    vehicles too small for a customer (A6; eval_staged's FLEX variant)."""
    dem = inst.demand.copy()
    dem[5] = 80                                   # only vehicle 2 can carry it
    return dataclasses.replace(inst, demand=dem, capacities=np.array([40, 5, 90, 30, 7, 60]),
                               start_times=np.array([480, 485, 490, 480, 483, 489]))


def sep_start(inst, chains, seed=9):
    """First-fit start tours with K - 1 separators (spec.pack_separators)."""
    P0 = synth.random_perms(chains, inst.n, seed=seed, dtype=np.uint16)
    return np.array([spec.pack_separators(p, inst.K - 1, inst.demand, inst.capacities)
                     for p in P0]).astype(np.int16)


# ---------------------------------------------------------------------------
# the cases: name -> (instance, tours [C][ld], n)
# ---------------------------------------------------------------------------
def _td10(H, tsp):
    inst = with_hours(synth.td_cvrp(10, 2, seed=4), H, first=7 if H < 24 else 0)
    return as_tsp(inst, 415) if tsp else inst


def _td8(tsp):
    inst = with_hours(synth.td_cvrp(8, 2, seed=6), 7, first=7)
    return as_tsp(inst, 415) if tsp else inst


def _route(het, asym):
    base = synth.td_cvrp_het(150, 12, seed=3) if het else synth.td_cvrp(150, 12, seed=3)
    return with_hours(base, 7, first=7, asym=asym, seed=11)


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once and shared (never modified) by the CPU and GPU tests."""
    if name == "cvrp20_h7":           # 7 x 21 x 21 x 2 B: matrix in LDS
        inst = with_hours(synth.td_cvrp(20, 3, seed=3), 7, first=7)
        return inst, synth.random_perms(4000, inst.n, seed=4), inst.n
    if name in ("cvrp60_h25_u8", "cvrp60_h25_u16", "cvrp60_h25_ld61", "cvrp60_h48_u8"):
        H = 48 if "h48" in name else 25   # 25 x 61 x 61 x 2 B > 64 KiB: matrix in L2
        inst = with_hours(synth.td_cvrp(60, 6, seed=5), H)
        P = synth.random_perms(3000 + 5, inst.n, seed=6, ld=inst.n + 1 if "ld61" in name else None,
                               dtype=np.uint16 if "u16" in name else np.uint8)
        return inst, P, inst.n
    if name == "tsp30_h2":
        inst = as_tsp(with_hours(synth.td_cvrp(30, 2, seed=1), 2, first=7), 415)
        return inst, synth.random_perms(3000, inst.n, seed=6), inst.n
    if name == "cvrp40_h7_i32":       # entries past 65,535: the int32 matrix
        inst = with_hours(synth.td_cvrp(40, 4, seed=2), 7, first=7)
        inst = dataclasses.replace(inst, durations=inst.durations * 60)
        return inst, synth.random_perms(2000, inst.n, seed=1), inst.n
    if name == "flex60_h7":
        inst = het_flex(with_hours(synth.td_cvrp(60, 6, seed=4), 7, first=7))
        return inst, synth.random_perms(4096, inst.n, seed=5), inst.n
    if name in ("cvrp40_h1024_u8", "cvrp40_h1024_u16"):
        inst = with_hours(synth.td_cvrp(40, 4, seed=7), 1024)
        P = synth.random_perms(2000, inst.n, seed=8,
                               dtype=np.uint16 if "u16" in name else np.uint8)
        return inst, P, inst.n
    if name.startswith("sa10_"):      # sa10_h2_cvrp, sa10_h25_tsp, ...
        _, h, prob = name.split("_")
        inst = _td10(int(h[1:]), prob == "tsp")
        return inst, synth.random_perms(3, inst.n, seed=7).astype(np.int16), inst.n
    if name.startswith("route150_"):  # route150_uni_sym, route150_het_asym, ...
        _, fleet, mat = name.split("_")
        inst = _route(fleet == "het", mat == "asym")
        return inst, sep_start(inst, 8), inst.n + inst.K - 1
    if name.startswith("bf8_"):
        inst = _td8(name.endswith("tsp"))
        return inst, synth.random_perms(256, inst.n, seed=2), inst.n
    if name == "ga10_h7":
        inst = with_hours(synth.td_cvrp(10, 2, seed=4), 7, first=7)
        return inst, synth.random_perms(32, inst.n, seed=5).astype(np.int16), inst.n
    raise KeyError(name)


EVAL_NAMES = ["cvrp20_h7", "cvrp60_h25_u8", "cvrp60_h25_u16", "cvrp60_h25_ld61", "cvrp60_h48_u8",
              "tsp30_h2", "cvrp40_h7_i32", "flex60_h7", "cvrp40_h1024_u8", "cvrp40_h1024_u16"]
SA_NAMES = [f"sa10_h{H}_{p}" for H in (2, 25) for p in ("cvrp", "tsp")]
ROUTE_NAMES = [f"route150_{f}_{m}" for f in ("uni", "het") for m in ("sym", "asym")]
ALL_NAMES = EVAL_NAMES + SA_NAMES + ROUTE_NAMES + ["bf8_cvrp", "bf8_tsp", "ga10_h7"]


def spec_keys(inst, D, tours):
    if inst.problem == "tsp":
        return spec.eval_tsp_batch(D, tours, int(inst.start_times[0]))
    return spec.eval_cvrp_batch(D, tours, inst.demand, inst.capacities, inst.start_times)[0]


# ---------------------------------------------------------------------------
# CPU: the cases can tell a misread matrix from the right one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_NAMES)
def test_cases_tell_misread_hours_apart(name):
    inst, P, n = case(name)
    tours = P[:, :n].astype(np.int64)
    D = np.asarray(inst.durations)
    H = D.shape[0]
    true = spec_keys(inst, D, tours)
    # every slice read as slice 0 (hour_of<1>, or an index that lost its hour term)
    static = spec_keys(inst, D[:1], tours)
    assert (static != true).mean() >= 0.9
    if H > 24:
        # the hour wrapped at 24 (hour_of<24>): (t // 60) % 24 only reaches slices 0..23
        wrapped = spec_keys(inst, D[:24], tours)
        assert (wrapped != true).mean() >= 0.9
    # and a few rows of the vectorised evaluator against the scalar one
    for i in range(0, tours.shape[0], max(1, tours.shape[0] // 3)):
        if inst.problem == "tsp":
            assert int(true[i]) == spec.eval_tsp(D, tours[i], int(inst.start_times[0]))
        else:
            assert int(true[i]) == spec.eval_cvrp(D, tours[i], inst.demand, inst.capacities,
                                                  inst.start_times)["key"]


def test_with_hours_slices():
    base = synth.td_cvrp(6, 2, seed=0)
    d = with_hours(base, 50).durations
    assert (d[:24] == base.durations).all()
    assert (d[24] == 3 * base.durations[0]).all() and (d[49] == 4 * base.durations[1]).all()
    assert (d[24] != d[0]).any()
    a = with_hours(base, 7, first=7, asym=True).durations
    assert (a[0] == a[0].T).all() and (a[0] == base.durations[7]).all()
    assert all((a[h] != a[h].T).any() for h in range(1, 7))
    assert all((np.diagonal(a[h]) == 0).all() for h in range(7))


# ---------------------------------------------------------------------------
# GPU: scoring
# ---------------------------------------------------------------------------
# vrpms_eval on an hour-indexed instance takes path 2; staged_fits() then
# picks eval_staged, whose staged_mat launches <MatT, HM = 0, ...> for H not
# in {1, 24}, M = 1 by default:
#   cvrp20_h7        <u16, 0, CVRP, !FLEX, u8,  1, aligned, MLDS>  (6 KiB matrix)
#   cvrp60_h25_u8    <u16, 0, CVRP, !FLEX, u8,  1, aligned, !MLDS> (186 KiB)
#   cvrp60_h25_u16   <u16, 0, CVRP, !FLEX, u16, 1, aligned, !MLDS>
#   cvrp60_h25_ld61  <u16, 0, CVRP, !FLEX, u8,  1, !aligned, !MLDS> (ld % 4 = 1)
#   cvrp60_h48_u8    as cvrp60_h25_u8 with 48 slices
#   tsp30_h2         <u16, 0, TSP,  -,     u8,  1, aligned, MLDS>
#   cvrp40_h7_i32    <i32, 0, CVRP, !FLEX, u8,  1, aligned, MLDS>  (47 KiB)
#   flex60_h7        <u16, 0, CVRP, FLEX,  u8,  1, aligned, MLDS>  (52 KiB)
STAGED = [n for n in EVAL_NAMES if "h1024" not in n]


@gpu
@pytest.mark.parametrize("name", STAGED)
def test_eval_staged_runtime_hours(ctx, coracle, name):
    from test_eval_gpu import check_batch
    inst, P, n = case(name)
    check_batch(ctx, coracle, inst, P, n=n, expect_path=2)


@gpu
@pytest.mark.parametrize("name", ["cvrp20_h7", "flex60_h7"])
def test_eval_staged_runtime_hours_max_objective(ctx, coracle, name):
    from test_eval_gpu import check_batch
    inst, P, n = case(name)
    check_batch(ctx, coracle, inst, P, n=n, objective=1, expect_path=2)


@gpu
def test_eval_generic_words_runtime_hours(ctx, coracle):
    """vrpms_eval_words without the packed layout (built for H = 1 only):
    launch_generic<uint8_t, WORDS>, matrix in LDS, eval_generic<u16, LDS,
    CVRP, HM = 0, u8, WORDS>."""
    from test_eval_gpu import check_words
    inst, P, n = case("cvrp20_h7")
    check_words(ctx, coracle, inst, P, n)
    check_words(ctx, coracle, inst, P[:1023], n, objective=1)


@gpu
@pytest.mark.parametrize("name", ["cvrp40_h1024_u8", "cvrp40_h1024_u16"])
def test_eval_generic_rows_max_hours(ctx, coracle, name):
    """H = 1024, N = 41: eval_staged's two H x N depot-leg tables (2 x 82 KiB)
    exceed the 160 KiB of LDS, staged_fits() is false and vrpms_eval falls to
    launch_generic<PermT>: eval_generic<u16, !LDS, CVRP, HM = 0, PermT> in the
    row layout (the 3.4 MB matrix stays in L2)."""
    from test_eval_gpu import check_batch
    inst, P, n = case(name)
    check_batch(ctx, coracle, inst, P, n=n, expect_path=2)


# ---------------------------------------------------------------------------
# GPU: simulated annealing
# ---------------------------------------------------------------------------
def u64(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint64).reshape(-1)]


def scorer(inst, objective=0):
    return search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times,
                         inst.problem, objective)


def load(ctx, inst, objective=0):
    from test_eval_gpu import load as load_
    load_(ctx, inst, objective)


@gpu
@pytest.mark.parametrize("name", SA_NAMES)
def test_sa_kernel_runtime_hours_matches_oracle(ctx, name):
    """window = 0 on H in {2, 25}: launch_sa_seg declines (H != 1),
    launch_sa_td declines (H != 24), the route kernel needs a window, so
    launch_inst<SaK> runs sa_kernel<u16, HM = 0, CVRP | TSP> (matrix in LDS)."""
    torch = torch_()
    inst, P, n = case(name)
    load(ctx, inst)
    chains = P.shape[0]
    cur = torch.from_numpy(P.copy()).to(ctx.dev)
    best = cur.clone()
    ck = torch.empty(chains, dtype=torch.int64, device=ctx.dev)
    bk = torch.full((chains,), -1, dtype=torch.int64, device=ctx.dev)
    seed, inv_t0, inv_alpha = 12345, 1.0 / 200.0, 1.0 / 0.97
    ctx.sa_run(cur, ck, best, bk, steps=20, inv_t0=inv_t0, inv_alpha=inv_alpha, seed=seed, step0=0)
    ref = search.sa_run(scorer(inst), P.tolist(), P.tolist(), [2**64 - 1] * chains, seed, 0, 20,
                        inv_t0, inv_alpha)
    assert cur.cpu().numpy().tolist() == ref[0]
    assert u64(ck) == ref[1]
    assert best.cpu().numpy().tolist() == ref[2]
    assert u64(bk) == ref[3]
    inv_t1 = np.float32(inv_t0)
    for _ in range(20):
        inv_t1 = np.float32(inv_t1 * np.float32(inv_alpha))
    ctx.sa_run(cur, ck, best, bk, steps=10, inv_t0=float(inv_t1), inv_alpha=inv_alpha, seed=seed,
               step0=20)
    ref2 = search.sa_run(scorer(inst), ref[0], ref[2], ref[3], seed, 20, 10, float(inv_t1),
                         inv_alpha)
    assert cur.cpu().numpy().tolist() == ref2[0]
    assert u64(ck) == ref2[1]
    assert best.cpu().numpy().tolist() == ref2[2]
    assert u64(bk) == ref2[3]


def _run_sa(ctx, P, steps, inv_t0, window, types, moves):
    torch = torch_()
    cur = torch.from_numpy(P.copy()).to(ctx.dev)
    best = cur.clone()
    ck = torch.empty(P.shape[0], dtype=torch.int64, device=ctx.dev)
    bk = torch.full((P.shape[0],), -1, dtype=torch.int64, device=ctx.dev)
    ctx.sa_run(cur, ck, best, bk, steps=steps, inv_t0=inv_t0, inv_alpha=1 / 0.99, seed=21,
               step0=7, window=window, window_types=types, moves=moves)
    return cur.cpu().numpy(), u64(ck), best.cpu().numpy(), u64(bk)


@gpu
@pytest.mark.parametrize("moves", [64, 256])
@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_sa_route_kernel_runtime_hours_matches_c_restatement(ctx, coracle, name, moves):
    """Windowed SA on TD-150 x 7 hours.  launch_sa_seg declines (H != 1) and
    launch_sa_td declines (H != 24: no hour-minor rows), so the windowed CVRP
    reaches the route-local kernel through launch_inst's third arm:
      route150_uni_*  sa_route_kernel<u16, HM = 0>        (one capacity, one start time)
      route150_het_*  sa_route_kernel<u16, HM = 0, HV>    (per-vehicle capacities and
                      start times; td_full_walk needs H == 24, so it is false here
                      and the heterogeneous fleet is not sent to sa_kernel)
    moves = 64: four chains per workgroup; 256: four wavefronts per chain.
    *_asym: only slice 0 is symmetric, so Instance::symmetric is true while
    the slices a walk reads are not (the edge caches it selects exist only
    for HM = 1)."""
    inst, P, L = case(name)
    load(ctx, inst)
    chains, steps, inv_t0, window, types = P.shape[0], 60, 1 / 200.0, 32, 2
    got = _run_sa(ctx, P, steps, inv_t0, window, types, moves)
    for resync in (False, True):
        ccur, cbest = P.view(np.uint16).copy(), P.view(np.uint16).copy()
        cbk = np.full(chains, 2**64 - 1, dtype=np.uint64)
        cck = coracle.sa_run(inst.durations, ccur, cbest, cbk, steps, inv_t0, 1 / 0.99, 21, 7,
                             inst.demand, inst.capacities, inst.start_times, window=window,
                             window_types=types, resync=resync, moves=moves)
        assert (got[0].view(np.uint16) == ccur).all()
        assert got[1] == [int(x) for x in cck] and got[3] == [int(x) for x in cbk]
        assert (got[2].view(np.uint16) == cbest).all()
    assert (got[0] != P).any()                  # some move was accepted
    if moves == 64:
        # the same chains by full re-evaluation on the device (sa_kernel<u16, 0, CVRP>,
        # matrix in L2) and with the route kernel forced
        for mode in (2, 3):
            ctx.set_sa_route(mode)
            try:
                other = _run_sa(ctx, P, steps, inv_t0, window, types, moves)
            finally:
                ctx.set_sa_route(0)
            assert (other[0] == got[0]).all() and other[1] == got[1]
            assert (other[2] == got[2]).all() and other[3] == got[3]


# ---------------------------------------------------------------------------
# GPU: brute force, GA, ACO
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["bf8_cvrp", "bf8_tsp"])
def test_bf_runtime_hours_matches_oracle(ctx, coracle, name):
    """launch_inst<BfK>: bf_kernel<u16, HM = 0, CVRP | TSP>, n = 8 at H = 7."""
    inst, _, n = case(name)
    load(ctx, inst)
    full = math.factorial(n)
    best = ctx.bf_run(n, 0, full)
    assert best == search.bf(scorer(inst), n)
    kw = dict(start_times=inst.start_times, problem=0) if inst.problem == "tsp" else \
        dict(demand=inst.demand, capacities=inst.capacities, start_times=inst.start_times)
    assert best == coracle.bf(inst.durations, n, 0, full, **kw)
    parts = [ctx.bf_run(n, a, b) for a, b in [(0, 1000), (1000, 33333), (33333, full)]]
    assert min(parts) == best
    assert scorer(inst)(search.unrank(best[1], n)) == best[0]


@gpu
def test_ga_runtime_hours_matches_oracle(ctx):
    """The fused GA needs the packed layout (H = 1), so H = 7 takes the three
    kernels: ga_breed_kernel<false>, vrpms_eval on the 2-byte children
    (eval_staged<u16, HM = 0, CVRP, !FLEX, u16, 1, aligned, !MLDS>) and
    ga_select_kernel<false>."""
    torch = torch_()
    inst, P, n = case("ga10_h7")
    load(ctx, inst)
    islands, pop = 2, 16
    dpop = torch.from_numpy(P.reshape(islands, pop, n).copy()).to(ctx.dev)
    keys = ctx.eval(dpop.view(islands * pop, n)).view(islands, pop)
    sc = scorer(inst)
    rpop = [[list(r) for r in P.reshape(islands, pop, n)[i]] for i in range(islands)]
    rkeys = [[sc(t) for t in rpop[i]] for i in range(islands)]
    assert u64(keys) == [k for ks in rkeys for k in ks]
    seed, pmut = 99, 0.3
    pm = min(int(round(pmut * 2**32)), 2**32 - 1)
    for g in range(3):
        rpop, rkeys = search.ga_generation(sc, rpop, rkeys, seed, g, pm)
    ctx.ga_generation(dpop, keys, generations=3, pmut=pmut, seed=seed, gen0=0)
    assert dpop.cpu().numpy().tolist() == rpop
    assert u64(keys) == [k for ks in rkeys for k in ks]


@gpu
def test_aco_runtime_hours_matches_oracle(ctx):
    """ACO at H = 7: ants are built from slice 0's eta and scored by
    vrpms_eval on 2-byte tours (eval_staged HM = 0, as the GA's children)."""
    inst, _, n = case("ga10_h7")
    load(ctx, inst)
    colonies, ants, tau0 = 2, 8, 1 << 20
    tau, eta = ctx.aco_init(colonies, tau0)
    ref_eta = search.aco_eta(inst.durations[0])
    assert (eta.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist() == ref_eta.tolist()
    rtau = [np.full((inst.N, inst.N), tau0, dtype=np.int64) for _ in range(colonies)]
    sc = scorer(inst)
    for it in range(3):
        tours, keys, ib = ctx.aco_iteration(tau, eta, ants, seed=7, it=it, evap_shift=3,
                                            tau_min=1 << 10, tau_max=1 << 30)
        rt, rk, rib = search.aco_iteration(sc, rtau, ref_eta, ants, n, 7, it, 3, 1 << 10, 1 << 30)
        assert tours.cpu().numpy().tolist() == rt
        assert u64(keys) == [k for ks in rk for k in ks]
        assert [(a & (2**64 - 1), b) for a, b in ib.cpu().tolist()] == rib
        got_tau = tau.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        assert all((got_tau[c] == rtau[c]).all() for c in range(colonies))


# ---------------------------------------------------------------------------
# GPU: the exact solvers refuse what they do not implement
# ---------------------------------------------------------------------------
@gpu
def test_exact_solvers_refuse_runtime_hours(ctx):
    """tsp_dp and vrp_sp need a static matrix, tsp_tdp and vrp_tdsp H = 1 or
    24: with H = 7 loaded each returns VRPMS_EINVAL, and writes nothing."""
    torch = torch_()
    lib = ctx.lib
    work = torch.zeros(1 << 20, dtype=torch.uint8, device=ctx.dev)

    def guarded(n):
        return (torch.full((n,), -7, dtype=torch.int16, device=ctx.dev),
                torch.full((1,), -7, dtype=torch.int64, device=ctx.dev))

    def untouched(tour, key):
        torch.cuda.synchronize(ctx.dev)
        return (tour == -7).all().item() and (key == -7).all().item() and \
            (work == 0).all().item()

    n = 8
    load(ctx, _td8(True))
    tour, key = guarded(n)
    assert lib.vrpms_tsp_dp_run(ctx.handle, n, work.data_ptr(), work.numel(), tour.data_ptr(),
                                key.data_ptr(), ctx.stream()) == _lib.VRPMS_EINVAL
    assert b"vrpms_tsp_dp_run" in lib.vrpms_last_error() and b"7 hour slices" in lib.vrpms_last_error()
    assert untouched(tour, key)
    assert lib.vrpms_tsp_tdp_run(ctx.handle, n, 600, work.data_ptr(), work.numel(),
                                 tour.data_ptr(), key.data_ptr(), ctx.stream()) == _lib.VRPMS_EINVAL
    assert b"vrpms_tsp_tdp_run" in lib.vrpms_last_error() and b"(it has 7)" in lib.vrpms_last_error()
    assert untouched(tour, key)

    inst = _td8(False)
    load(ctx, inst)
    tour, key = guarded(n + inst.K)
    assert lib.vrpms_vrp_sp_run(ctx.handle, n, work.data_ptr(), work.numel(), tour.data_ptr(),
                                key.data_ptr(), ctx.stream()) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_sp_run" in lib.vrpms_last_error() and b"7 hour slices" in lib.vrpms_last_error()
    assert untouched(tour, key)
    assert lib.vrpms_vrp_tdsp_run(ctx.handle, n, 600, work.data_ptr(), work.numel(),
                                  tour.data_ptr(), key.data_ptr(), ctx.stream()) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_tdsp_run" in lib.vrpms_last_error() and b"(it has 7)" in lib.vrpms_last_error()
    assert untouched(tour, key)
