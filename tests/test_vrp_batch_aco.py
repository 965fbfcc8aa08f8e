"""Batched VRP ACO (spec A24): the C entry points vrpms_vrp_batch_aco_lds /
vrpms_vrp_batch_aco, Context.vrp_batch_aco, solver.batch_aco_key /
batch_aco_fits / solve_vrp_aco_batch and the service's VRP ACO batcher
(App(batch_vrp_aco=True)).

The reference is a24_ref below: I calls of oracle.search.aco_iteration on one
colony with an oracle.search.Scorer, tau = tau0 everywhere, eta of the hour-0
slice and the best-so-far tracked in place, then spec.eval_cvrp for the
durations and vehicles.  Per request the GPU must return the identical key,
tour, route durations and vehicle row, for both objectives."""
import ctypes
import functools
import json

import numpy as np
import pytest

from oracle import spec
from oracle.search import Scorer, aco_eta, aco_iteration
from test_vrp_batch_ga import (SEED, _FakeApp, _body, _concurrently, _fake_launch, _locs, _no_gpu,
                               _rescored, _sized, inst as ga_inst, obj_id)
from vrpms_amd import _lib, core, runners, service, solver
from vrpms_amd.core import CVRP

LDS_BYTES = 160 * 1024
OBJECTIVES = ("sum", "max")
DEFAULTS = dict(tau0=1 << 24, tau_min=1 << 12, tau_max=1 << 30, evap_shift=3, bsf_period=5)


# ---------------------------------------------------------------------------
# instances and their references (computed once, shared, never changed)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inst(case):
    """test_vrp_batch_ga's instances, and two variants of this file on a copy
    of the plain one: "zodd" replaces every off-diagonal entry of the odd rows
    of slice 0 by 4096 + (i * 7 + j) % 900, "zall" those of all rows.  eta =
    floor(2^24 / (1 + d)^2) is 0 from d = 4096 on, so a step out of such a row
    has tot == 0 and takes the first unvisited node."""
    n, K, H, seed, variant = case
    if variant not in ("zodd", "zall"):
        return ga_inst(case)
    D, dem, caps, starts = ga_inst((n, K, H, seed, ""))
    D = D.copy()
    for i in range(n + 1):
        if variant == "zall" or i % 2:
            for j in range(n + 1):
                if i != j:
                    D[0, i, j] = 4096 + (i * 7 + j) % 900
    D.setflags(write=False)
    return D, dem, caps, starts


def step_totals(T, eta, tour):
    """The roulette's total weight at every step of `tour` under pheromone T."""
    N = eta.shape[0]
    vis = np.zeros(N, dtype=bool)
    vis[0] = True
    cur, out = 0, []
    for pick in tour:
        out.append(int(np.where(vis, 0, (T[cur] >> 8) * eta[cur]).sum()))
        vis[pick] = True
        cur = pick
    return out


def a24_ref(D, dem, caps, starts, objective, A, I, seed, **tau_params):
    """Spec A24 -> dict(key, tour, durs, veh, unvisited) and what the
    trajectory went through: `tie` (iterations whose best key two ants share),
    `bsf_other` (best-so-far deposits of a tour other than the iteration
    best), `floor` (the first iteration after which a cell sits at tau_min, or
    None), `over` (iterations after whose deposit a cell is above tau_max),
    `mixed` (some ant's tour had a tot == 0 step and a tot != 0 step),
    `zero_steps` / `steps` (tot == 0 steps / all steps of the iteration bests)."""
    p = dict(DEFAULTS, **tau_params)
    D = spec.as_3d(D)
    N = D.shape[1]
    n = N - 1
    score = Scorer(D, dem, list(caps), list(starts), objective=obj_id(objective))
    tau = [np.full((N, N), p["tau0"], dtype=np.int64)]
    eta = aco_eta(D[0])
    best = ([None], [2**64 - 1])
    tie = bsf_other = over = zero_steps = steps = 0
    floor, mixed = None, False
    for it in range(I):
        before = tau[0].copy()
        tours, keys, ib = aco_iteration(score, tau, eta, A, n, seed, it, p["evap_shift"],
                                        p["tau_min"], p["tau_max"], best=best,
                                        bsf_period=p["bsf_period"])
        k, b = ib[0]
        tie += keys[0].count(k) > 1
        if p["bsf_period"] > 0 and (it + 1) % p["bsf_period"] == 0:
            bsf_other += best[0][0] != tours[0][b]
        over += bool((tau[0] > p["tau_max"]).any())
        if floor is None and (tau[0] == p["tau_min"]).any():
            floor = it
        tots = step_totals(before, eta, tours[0][b])
        zero_steps += tots.count(0)
        steps += len(tots)
        for t in tours[0][:4]:
            tt = step_totals(before, eta, t)
            mixed |= 0 in tt and any(tt)
        assert all(sorted(t) == list(range(1, N)) for t in tours[0])
    final = spec.eval_cvrp(D, best[0][0], dem, list(caps), list(starts), obj_id(objective))
    assert final["key"] == best[1][0]
    return dict(key=best[1][0], tour=best[0][0], durs=final["durations"], veh=final["vehicle_of"],
                unvisited=final["unvisited"], tie=tie, bsf_other=bsf_other, floor=floor, over=over,
                mixed=mixed, zero_steps=zero_steps, steps=steps)


@functools.lru_cache(maxsize=None)
def reference(run, objective):
    """run = (case, A, I, ((parameter, value), ...))."""
    case, A, I, params = run
    return a24_ref(*inst(case), objective, A, I, SEED, **dict(params))


def expected(runs, objective):
    refs = [reference(r, objective) for r in runs]
    return ([r["key"] for r in refs], [r["tour"] for r in refs], [r["durs"] for r in refs],
            [r["veh"] for r in refs])


def lds_bytes(N, K, H, wide, A):
    """DESIGN.md §4.3o restated: the matrix padded to 16 bytes, the demand row
    and the two fleet rows as int32 padded to four words, 64 bytes of
    reduction slots, tau and eta at 4 bytes a cell each, and A + 1 uint16 rows
    of an odd number of words."""
    def pad(x, m):
        return (x + m - 1) // m * m
    n = N - 1
    rs = 2 * (((n + 1) // 2) | 1)
    return pad(H * N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + 64 + \
        2 * 4 * N * N + (A + 1) * 2 * rs


def largest_n_nodes(K, H, wide, A):
    return max(N for N in range(2, 400) if lds_bytes(N, K, H, wide, A) <= LDS_BYTES)


# DESIGN.md §4.3o's domain table (K = 4): (H, wide, A) -> the largest N
DOMAIN = {(24, False, 64): 52, (24, False, 256): 49, (24, True, 64): 39, (24, True, 256): 37,
          (1, False, 4): 127, (1, False, 64): 121, (1, False, 256): 104,
          (1, True, 4): 116, (1, True, 64): 111, (1, True, 256): 97}

# the runs of the GPU comparisons: (case, A, I, parameters other than the defaults)
N_EDGES = [((n, 3, 1, n, ""), 64, 3, ()) for n in (1, 2, 3, 62, 63, 64, 65)] + \
          [((1, 2, 24, 2, "below"), 5, 2, ())]
A_EDGES = [((9, 3, 24, 70, ""), A, 6, ()) for A in (1, 2, 63, 64, 65, 255, 256)]
I_EDGES = [((8, 3, 1, 9, ""), 20, I, ()) for I in (1, 4, 5, 6, 30)] + \
          [((8, 3, 1, 9, ""), 20, 6, (("bsf_period", 0),)), ((8, 3, 1, 9, ""), 20, 6, (("bsf_period", 1),))]
FLOOR = ((8, 3, 24, 71, ""), 20, 16, (("evap_shift", 1),))         # both objectives run
CEILING = ((6, 3, 24, 73, "below"), 16, 6, ())
ZERO = [((7, 3, 1, 5, "zodd"), 16, 6, ()), ((7, 3, 1, 5, "zall"), 16, 6, ())]
HOURS = [((6, 3, 24, s, "hours"), 32, 12, ()) for s in (10, 11)]
FLEETS = [((3, 64, 1, 12, ""), 16, 3, ()), ((9, 5, 24, 13, "zerocap"), 32, 6, ()),
          ((9, 3, 1, 14, "zerodem"), 32, 6, ())]
WAVES = [((64, 4, 1, 74, ""), A, 2, ()) for A in (1, 3, 4, 5, 65, 256)] + [((70, 4, 1, 75, ""), 24, 3, ())]
ALL_RUNS = N_EDGES + A_EDGES + I_EDGES + [FLOOR, CEILING] + ZERO + HOURS + FLEETS + WAVES
SIX = [((10, 3, 24, 20 + x, ""), 48, 6, ()) for x in range(6)]


def run_id(r):
    return "n%d-K%d-H%d-s%d%s-A%d-I%d" % (*r[0], r[1], r[2]) + "".join("-%s%d" % kv for kv in r[3])


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


def test_lds_bytes_formula_monotone_and_refusals(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_vrp_batch_aco_lds
    As = (1, 2, 63, 64, 65, 128, 129, 255, 256)
    for H in (1, 24):
        for wide in (0, 1):
            for K in (1, 4, 5, 64):
                for x, A in enumerate(As):
                    for N in list(range(2, 70)) + [96, 97, 128, 129]:
                        assert f(N, K, H, wide, A, ctypes.byref(b)) == _lib.VRPMS_OK
                        assert b.value == lds_bytes(N, K, H, wide, A) == \
                            core.vrp_batch_aco_lds(N, K, H, wide, A)
                        if N > 2:
                            assert b.value > lds_bytes(N - 1, K, H, wide, A)
                        if x:
                            assert b.value > lds_bytes(N, K, H, wide, As[x - 1])
    for args, word in (((1, 3, 1, 0, 8), b"2 <= N"), ((0, 3, 1, 0, 8), b"2 <= N"),
                       ((65536, 3, 1, 0, 8), b"2 <= N"),
                       ((5, 0, 1, 0, 8), b"1 <= K <= 64"), ((5, 65, 1, 0, 8), b"1 <= K <= 64"),
                       ((5, 3, 2, 0, 8), b"H must be 1 or 24"), ((5, 3, 0, 0, 8), b"H must be 1 or 24"),
                       ((5, 3, 1, 2, 8), b"wide"), ((5, 3, 1, -1, 8), b"wide"),
                       ((5, 3, 1, 0, 0), b"1 <= A <= 256 (0 given)"),
                       ((5, 3, 1, 0, 257), b"1 <= A <= 256 (257 given)")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_aco_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(5, 3, 1, 0, 8, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_aco_lds" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= A <= 256"):
        core.vrp_batch_aco_lds(5, 3, 1, False, 300)
    assert solver.BATCH_ACO_LDS_BYTES == LDS_BYTES and solver.BATCH_ACO_MAX_ANTS == 256
    assert solver.BATCH_ACO_MAX_ITERATIONS == 1000
    # what the formula admits never needs more than the two nodes a lane owns
    assert max(DOMAIN.values()) <= 128 and largest_n_nodes(1, 1, False, 1) <= 128


def test_argument_errors_need_no_gpu(lib):
    """Every argument check comes before the context is looked at, so a
    stand-in block of zeros serves as the non-NULL ctx here."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(4096)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    names = ("m", "d", "cp", "st", "t", "k", "du", "v")

    def f(ctx=c, R=1, N=5, K=2, H=1, obj=0, wide=0, A=8, I=3, tau0=1 << 24, tau_min=1 << 12,
          tau_max=1 << 30, shift=3, bsf=5, **ptrs):
        a = {name: ptrs.get(name, p) for name in names}
        return lib.vrpms_vrp_batch_aco(ctx, a["m"], a["d"], a["cp"], a["st"], R, N, K, H, obj, wide, A,
                                       I, tau0, tau_min, tau_max, shift, bsf, 5, a["t"], a["k"],
                                       a["du"], a["v"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_aco:" in msg and word in msg, (kw, msg)

    refused(b"ctx is NULL", ctx=None)
    refused(b"R must not be negative", R=-1)
    for N in (-1, 0, 1, 65536):
        refused(b"2 <= N", N=N)
    for K in (-1, 0, 65, 1000):
        refused(b"1 <= K <= 64", K=K)
    for H in (0, 2, 12, 25):
        refused(b"H must be 1 or 24", H=H)
    for obj in (-1, 2):
        refused(b"objective", obj=obj)
    for wide in (-1, 2):
        refused(b"wide", wide=wide)
    for A in (-1, 0, 257, 4096):
        refused(b"1 <= A <= 256 (%d given)" % A, A=A)
    for I in (-1, 0):
        refused(b"I must be at least 1 (%d given)" % I, I=I)
    for shift in (-1, 0, 32):
        refused(b"evap_shift must be in [1, 31] (%d given)" % shift, shift=shift)
    refused(b"bsf_period must not be negative (-1 given)", bsf=-1)
    for kw in (dict(tau_min=0), dict(tau_min=(1 << 24) + 1), dict(tau_max=(1 << 24) - 1),
               dict(tau_max=(1 << 30) + 1), dict(tau0=(1 << 30) + 1, tau_max=(1 << 30) + 1),
               dict(tau0=0, tau_min=0), dict(tau_max=2**32 - 1)):
        refused(b"0 < tau_min <= tau0 <= tau_max <= 2^30", **kw)
    for name in names:
        refused(b"NULL", **{name: None})
    refused(b"H must be 1 or 24", R=0, H=3)            # the shape checks also with R = 0
    refused(b"I must be at least 1", R=0, I=0)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert f(R=0, tau0=1 << 30, tau_min=1 << 30, tau_max=1 << 30, shift=31, bsf=0, A=256, I=1) == \
        _lib.VRPMS_OK
    assert buf.raw == bytes(4096) and fake.raw == bytes(1 << 16)


def request(case, base=0):
    """The case as a solve_vrp_aco_batch tuple (H = 1 as a plain [N][N] matrix)."""
    D, dem, caps, starts = inst(case)
    return ((D[0] if D.shape[0] == 1 else D).tolist(), _locs(dem, base), list(caps), list(starts))


def compact(case):
    return solver.compact_vrp(*request(case))


def test_solve_vrp_aco_batch_refusals_need_no_gpu(monkeypatch, lib):
    _no_gpu(monkeypatch)
    good = request((6, 2, 1, 0, ""))
    assert solver.solve_vrp_aco_batch([]) == []
    with pytest.raises(ValueError, match=r"^request 1: capacities and startTimes"):
        solver.solve_vrp_aco_batch([good, (good[0], good[1], [3, 3], [0])])
    with pytest.raises(ValueError, match=r"^request 2: 5 locations but a 7-node"):
        solver.solve_vrp_aco_batch([good, good, {"durations": good[0], "locations": good[1][:5],
                                                 "capacities": [3], "start_times": [0]}])
    big = np.full((7, 7), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_vrp_aco_batch([good, (big.tolist(), good[1], [3, 3], [0, 0])])
    heavy = [{"id": i, "demand": 2**30} for i in range(7)]
    with pytest.raises(ValueError, match=r"^request 0: capacity \+ demand overflows int32"):
        solver.solve_vrp_aco_batch([(good[0], heavy, [2**30, 3], [0, 0])])
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp_aco_batch([good], objective="mean")
    with pytest.raises(ValueError, match="ants"):
        solver.solve_vrp_aco_batch([good], ants=0)
    with pytest.raises(ValueError, match="iters"):
        solver.solve_vrp_aco_batch([good], iters=0)
    # no customer: solve_vrp's trivial answer, built on the host
    none = (good[0], good[1], [3, 3], [0, 7], [1, 2, 3, 4, 5, 6])
    assert solver.solve_vrp_aco_batch([none], with_unvisited=True) == [
        {"durationMax": 0, "durationSum": 0, "unvisited": [],
         "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}]


def test_batch_aco_fits_at_the_lds_edge(lib):
    for (H, wide, A), N in DOMAIN.items():
        assert largest_n_nodes(4, H, wide, A) == N, (H, wide, A, largest_n_nodes(4, H, wide, A))
        assert lds_bytes(N, 4, H, wide, A) <= LDS_BYTES < lds_bytes(N + 1, 4, H, wide, A)
        big = 70000 if wide else 0
        assert solver.batch_aco_fits(_sized(N, 4, H, big), A, 100)
        assert not solver.batch_aco_fits(_sized(N + 1, 4, H, big), A, 100)
        assert solver.batch_aco_key(_sized(N, 4, H, big), A, 100) == (N, 4, H, wide, A, 100)
    small = _sized(6, 2, 24)
    cap = solver.BATCH_ACO_MAX_ITERATIONS
    assert solver.batch_aco_fits(small, 256, cap) and solver.batch_aco_fits(small, 1, 1)
    assert not solver.batch_aco_fits(small, 257, 100)
    assert not solver.batch_aco_fits(small, 0, 100)
    assert not solver.batch_aco_fits(small, 64, 0)
    assert not solver.batch_aco_fits(small, 64, cap + 1)
    # a wide entry halves the cells that fit; 65535 is still narrow
    N = DOMAIN[(24, False, 256)]
    assert not solver.batch_aco_fits(_sized(N, 4, 24, 70000), 256, 100)
    assert solver.batch_aco_fits(_sized(N, 4, 24, 65534), 256, 100)
    # outside the domain whatever the size
    assert not solver.batch_aco_fits(_sized(5, 65, 1), 8, 4)
    none = solver.compact_vrp(np.ones((3, 3), dtype=np.int64), _locs([0, 1, 1]), [3], [0], [1, 2])
    assert none.n == 0 and not solver.batch_aco_fits(none, 8, 4)
    tsp = solver.compact_tsp(np.ones((4, 4), dtype=np.int64), [1, 2, 3], 0, 0)
    assert not solver.batch_aco_fits(tsp, 8, 4)


def test_reference_properties():
    """What the GPU comparisons rely on, checked on the reference itself."""
    refs = {(run, o): reference(run, o) for run in ALL_RUNS for o in OBJECTIVES}
    for (run, o), r in refs.items():
        print(run_id(run), o, {k: r[k] for k in ("key", "unvisited", "tie", "bsf_other", "floor", "over",
                                                 "mixed", "zero_steps", "steps")})
    # a tied iteration best: the lowest ant wins it
    assert sum(r["tie"] for r in refs.values()) > 0
    assert reference(I_EDGES[4], "sum")["tie"] > 0 and reference(A_EDGES[-1], "sum")["tie"] > 0
    # a best-so-far deposit of a tour that is not the iteration best; never with
    # bsf_period = 0, and I = 4 has no best-so-far deposit at all
    assert reference(I_EDGES[4], "sum")["bsf_other"] > 0
    assert reference(I_EDGES[5], "sum")["bsf_other"] == 0 == reference(I_EDGES[1], "sum")["bsf_other"]
    assert I_EDGES[5][3] == (("bsf_period", 0),) and I_EDGES[6][3] == (("bsf_period", 1),)
    # bsf_period changes the trajectory's pheromone: never / default / always are three runs
    assert len({(run[2], run[3]) for run in I_EDGES}) == len(I_EDGES)
    # a cell at tau_min, within the run and not at its start
    fl = reference(FLOOR, "max")["floor"]
    assert fl is not None and 0 < fl < FLOOR[2] - 1
    assert reference(I_EDGES[4], "sum")["floor"] is None       # the default shift is not there by I = 30
    # a cell above tau_max after the deposit, every iteration: primary 0 deposits 2^30
    c = reference(CEILING, "sum")
    assert c["over"] == CEILING[2] and c["unvisited"] == 6 and (c["key"] >> 28) & (2**28 - 1) == 0
    # tot == 0 and tot != 0 steps in one tour; with every row replaced only tot == 0,
    # and every ant builds 1..n
    z = reference(ZERO[0], "sum")
    assert z["mixed"] and 0 < z["zero_steps"] < z["steps"]
    z = reference(ZERO[1], "sum")
    assert not z["mixed"] and z["zero_steps"] == z["steps"] and z["tour"] == list(range(1, 8))
    assert all(r["zero_steps"] == 0 for (run, o), r in refs.items() if run not in ZERO)
    # an unvisited customer, and some but not all
    assert reference(N_EDGES[-1], "sum")["unvisited"] == 1
    assert any(0 < r["unvisited"] < len(r["tour"]) for r in refs.values())
    assert reference(N_EDGES[0], "sum")["tour"] == [1]
    # the hour cases cross an hour and midnight: the static slice gives another answer
    for run in HOURS:
        D, dem, caps, starts = inst(run[0])
        r = reference(run, "sum")
        flat = spec.eval_cvrp(D[:1], r["tour"], dem, list(caps), list(starts))
        assert flat["key"] != r["key"]
        assert any(s >= 23 * 60 and s + d >= 1440 for s, d in zip(starts, r["durs"]) if d)
    # the iterations do something
    assert reference(I_EDGES[4], "sum")["key"] < reference(I_EDGES[0], "sum")["key"]
    # both constructions and their boundary are in the list
    assert {run[0][0] + 1 for run in N_EDGES} >= {63, 64, 65, 66}


def test_vrp_aco_batcher_groups_and_fans_out_errors(lib):
    seen = []
    b = service.VrpAcoBatcher(_FakeApp(), window_s=0.2, iters=7, ants=9, launch=_fake_launch(seen))
    assert isinstance(b, service.VrpSaBatcher) and (b.ants, b.iters) == (9, 7)
    jobs = [((5, 2, 1, x, ""), "sum") for x in range(4)] + [((5, 3, 1, 5, ""), "sum")] * 2 + \
           [((5, 2, 24, 8 + x, ""), "max") for x in range(2)] + \
           [((5, 2, 1, 10, "e65536"), "sum"), ((5, 2, 1, 11, ""), "max")]
    out = _concurrently(lambda x: b.solve(compact(jobs[x][0]), jobs[x][1]), len(jobs))
    assert sorted(seen) == [((6, 2, 1, False, "max"), 1), ((6, 2, 1, False, "sum"), 4),
                            ((6, 2, 1, True, "sum"), 1), ((6, 2, 24, False, "max"), 2),
                            ((6, 3, 1, False, "sum"), 2)]
    assert b.launches == 5 and b.requests == 10
    for job, res in zip(jobs, out):
        K = job[0][1]
        assert res == {"durationMax": 50, "durationSum": 50,
                       "vehicles": [{"tour": [0, 5, 4, 3, 2, 1, 0], "duration": 50}] +
                                   [{"tour": [0, 0], "duration": 0}] * (K - 1)}

    def failing(key, cis):
        if key[1] == 2:
            raise RuntimeError("launch failed")
        return _fake_launch([])(key, cis)

    b = service.VrpAcoBatcher(_FakeApp(), window_s=0.2, launch=failing)
    out = _concurrently(lambda x: b.solve(compact(jobs[x][0]), jobs[x][1]), 6)
    assert all(isinstance(o, RuntimeError) and "launch failed" in str(o) for o in out[:4])
    assert all(isinstance(o, dict) and len(o["vehicles"]) == 3 for o in out[4:])
    # the constructor refuses what the launch would: no clamp
    cap = solver.BATCH_ACO_MAX_ITERATIONS
    for kw in (dict(ants=0), dict(ants=257), dict(iters=0), dict(iters=cap + 1)):
        with pytest.raises(ValueError, match="must be in 1"):
            service.VrpAcoBatcher(_FakeApp(), **kw)
        with pytest.raises(ValueError, match="must be in 1"):
            service.App(service.MemoryStore({}, {}, {}), batch_vrp_aco=True,
                        **{"batch_aco_" + ("ants" if "ants" in kw else "iterations"): list(kw.values())[0]})
    assert b.accepts(_sized(6, 2, 24)) and not b.accepts(_sized(6, 2, 1, 2**29))       # the A9 guard
    edge = service.VrpAcoBatcher(_FakeApp(), ants=256, launch=failing)
    assert edge.accepts(_sized(DOMAIN[(1, False, 256)], 4, 1))
    assert not edge.accepts(_sized(DOMAIN[(1, False, 256)] + 1, 4, 1))
    assert b.accepts(_sized(DOMAIN[(1, False, 256)] + 1, 4, 1))                         # at 64 ants it fits


def test_app_batch_vrp_aco_routes(lib):
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, len(params["capacities"])))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    # the flag is off: the injected solve
    off = service.App(service.MemoryStore({}, {}, {}), solve=fake)
    assert off.vrp_aco_batcher is None
    assert off.solve_inline("vrp", "aco", _body((5, 2, 1, 0, "")))[1]["message"]["durationSum"] == 3
    assert seen == [("vrp", "aco", 2)]
    del seen[:]

    D, locs, caps, starts = request((5, 2, 1, 1, ""), 100)
    store = service.MemoryStore({"7": locs}, {"8": D}, {})
    app = service.App(store, solve=fake, batch_vrp_aco=True, batch_window_s=0.2,
                      batch_vrp_aco_launch=_fake_launch(launched), batch_aco_iterations=7,
                      batch_aco_ants=9)
    assert isinstance(app.vrp_aco_batcher, service.VrpAcoBatcher)
    assert (app.vrp_aco_batcher.ants, app.vrp_aco_batcher.iters) == (9, 7)
    assert app.batcher is None and app.vrp_sa_batcher is None and app.vrp_ga_batcher is None

    def api(**more):
        return json.dumps(dict({"solutionName": "s", "solutionDescription": "d", "locationsKey": 7,
                                "durationsKey": 8, "capacities": caps, "startTimes": starts,
                                "ignoredCustomers": [103], "completedCustomers": []}, **more)).encode()

    def call(x):
        if x == 0:
            return app.post("vrp", "aco", api())
        if x < 4:        # the /solve route's seed and timeLimit do not reach a batched launch
            return app.solve_inline("vrp", "aco", _body((5, 2, 1, x, ""), seed=x, timeLimit=1.0))
        return app.solve_inline("vrp", "aco", _body((5, 2, 1, x, ""), objective="max"))

    out = _concurrently(call, 6)
    assert all(st == 200 for st, _ in out), out
    assert sorted(launched) == [((5, 2, 1, False, "sum"), 1), ((6, 2, 1, False, "max"), 2),
                                ((6, 2, 1, False, "sum"), 3)]
    assert seen == [] and app.vrp_aco_batcher.requests == 6
    # location 103 (row 3) is ignored: compact customers 4..1 are rows 5, 4, 2, 1
    assert out[0][1]["message"] == {
        "durationMax": 40, "durationSum": 40,
        "vehicles": [{"tour": [0, 5, 4, 2, 1, 0], "duration": 40}, {"tour": [0, 0], "duration": 0}]}
    assert out[3][1]["message"]["vehicles"][0]["tour"] == [0, 5, 4, 3, 2, 1, 0]

    # every rule that sends a request down the unbatched path, one by one
    def unbatched(status_and_result, K=2, algorithm="aco"):
        assert status_and_result[0] == 200, status_and_result
        assert seen == [("vrp", algorithm, K)]
        del seen[:]

    body = functools.partial(_body, (5, 2, 1, 1, ""))
    unbatched(app.solve_inline("vrp", "aco", body(knobs={"ants": 32})))               # inline knobs
    wide_fleet = json.dumps({"durations": D, "locations": locs, "capacities": [1] * 65,
                             "startTimes": [0] * 65, "ignoredCustomers": [],
                             "completedCustomers": []}).encode()
    unbatched(app.solve_inline("vrp", "aco", wide_fleet), K=65)                       # the LDS domain
    Nbig = largest_n_nodes(4, 1, False, 9) + 1
    bigD = np.ones((Nbig, Nbig), dtype=np.int64).tolist()
    big = json.dumps({"durations": bigD, "locations": _locs([0] + [1] * (Nbig - 1)),
                      "capacities": [Nbig] * 4, "startTimes": [0] * 4, "ignoredCustomers": [],
                      "completedCustomers": []}).encode()
    unbatched(app.solve_inline("vrp", "aco", big), K=4)
    guard = np.full((6, 6), 2**29, dtype=np.int64).tolist()                           # the A9 guard
    unbatched(app.solve_inline("vrp", "aco", json.dumps(
        {"durations": guard, "locations": locs, "capacities": caps, "startTimes": starts,
         "ignoredCustomers": [], "completedCustomers": []}).encode()))
    unbatched(app.solve_inline("vrp", "sa", body()), algorithm="sa")                  # another algorithm
    unbatched(app.solve_inline("vrp", "ga", body()), algorithm="ga")
    assert len(launched) == 3
    # a bad instance is a 400 in solve_vrp's words
    st, res = app.solve_inline("vrp", "aco", body(startTimes=[0]))
    assert st == 400 and "capacities and startTimes" in res["errors"][0]["reason"]


def test_cli_flags(monkeypatch, capsys):
    made = {}

    class Stop(Exception):
        pass

    def app(store, **kw):
        made.update(kw)
        raise Stop

    monkeypatch.setattr(service, "App", app)
    for argv, want in ((["--batch-vrp-aco"], (True, 100, 64)), ([], (False, 100, 64)),
                       (["--batch-vrp-aco", "--batch-aco-iterations", "1000", "--batch-aco-ants", "256"],
                        (True, 1000, 256)),
                       (["--batch-aco-iterations", "1", "--batch-aco-ants", "1"], (False, 1, 1))):
        with pytest.raises(Stop):
            service.main(argv)
        assert (made["batch_vrp_aco"], made["batch_aco_iterations"], made["batch_aco_ants"]) == want
        assert made["batch_vrp_sa"] is False and made["batch_vrp_ga"] is False
    for argv in (["--batch-aco-ants", "0"], ["--batch-aco-ants", "257"],
                 ["--batch-aco-iterations", "0"], ["--batch-aco-iterations", "1001"],
                 ["--batch-aco-ants", "many"]):
        with pytest.raises(SystemExit):
            service.main(argv)
        assert argv[0] in capsys.readouterr().err


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_batch(ctx, cases, objective, A, I, params=(), wide=None):
    """One vrp_batch_aco launch -> ([key], [tour], [durs], [veh])."""
    import torch
    insts = [inst(c) for c in cases]

    def dev(rows):
        return torch.tensor(np.stack(rows), dtype=torch.int32, device=ctx.dev)

    tours, keys, durs, veh = ctx.vrp_batch_aco(
        dev([D for D, _, _, _ in insts]), dev([d for _, d, _, _ in insts]),
        dev([np.array(c) for _, _, c, _ in insts]), dev([np.array(s) for _, _, _, s in insts]),
        obj_id(objective), A, I, SEED, wide=wide, **dict(params))
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), veh.cpu().tolist())


def gpu_runs(ctx, runs, objective, wide=None):
    """Runs of one (A, I, parameters) in one launch."""
    assert len({r[1:] for r in runs}) == 1 and len(runs) <= 16
    return gpu_batch(ctx, [r[0] for r in runs], objective, *runs[0][1:], wide=wide)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", ALL_RUNS, ids=run_id)
def test_gpu_equals_reference(ctx, run, objective):
    got = gpu_runs(ctx, [run], objective)
    want = expected([run], objective)
    print(run, objective, "gpu", got, "ref", want)
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_staging_width_and_instantiations(ctx, objective):
    """All four instantiations: (uint16 | int32) x (H = 1 | 24)."""
    for H in (1, 24):
        a, b, c = (7, 3, H, 30, ""), (7, 3, H, 31, "e65535"), (7, 3, H, 32, "")
        over = (7, 3, H, 31, "e65536")

        def runs(*cases):
            return [(x, 24, 4, ()) for x in cases]

        assert gpu_runs(ctx, runs(a, b, c), objective, wide=False) == expected(runs(a, b, c), objective)
        assert gpu_runs(ctx, runs(a, over, c), objective, wide=True) == \
            expected(runs(a, over, c), objective)
        assert gpu_runs(ctx, runs(over), objective) == expected(runs(over), objective)   # wide=None
        keys, tours, durs, veh = gpu_runs(ctx, runs(a, over, c), objective, wide=False)
        want = expected(runs(a, over, c), objective)
        assert keys[1] == 2**64 - 1 and tours[1] == [0] * 7 and durs[1] == [0] * 3 and \
            veh[1] == [-1] * 7
        for x in (0, 2):
            assert (keys[x], tours[x], durs[x], veh[x]) == tuple(w[x] for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_batch_independence(ctx, objective):
    want = expected(SIX, objective)
    together = gpu_runs(ctx, SIX, objective)
    assert together == want
    for x, run in enumerate(SIX):
        assert gpu_runs(ctx, [run], objective) == tuple([g[x]] for g in together)
    order = [5, 4, 3, 2, 1, 0, 5, 0, 3, 3, 1, 4]
    mixed = gpu_runs(ctx, [SIX[x] for x in order], objective)
    assert mixed == tuple([g[x] for x in order] for g in together)


# the LDS edge at K = 4: 64 ants where the hour slices bound N, 4 ants at the
# static edge (126 customers a tour: the CPU reference of 64 ants takes seconds)
LDS_EDGES = [(24, False, 64), (24, True, 64), (1, False, 4), (1, True, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,wide,A", LDS_EDGES, ids=lambda v: str(int(v)))
def test_gpu_lds_edge(ctx, H, wide, A):
    import torch
    lib, K, R = ctx.lib, 4, 2
    N = DOMAIN[(H, wide, A)]
    runs = [((N - 1, K, H, 40 + x, ""), A, 2, ()) for x in range(R)]
    for objective in OBJECTIVES:
        assert gpu_runs(ctx, runs, objective, wide=wide) == expected(runs, objective)
    N += 1
    n = N - 1
    M = torch.ones((R, H, N, N), dtype=torch.int32, device=ctx.dev)
    dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
    cp = torch.ones((R, K), dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R, n), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R, K), -7, dtype=torch.int32, device=ctx.dev)
    veh = torch.full((R, n), -7, dtype=torch.int8, device=ctx.dev)
    rc = lib.vrpms_vrp_batch_aco(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(), cp.data_ptr(),
                                 R, N, K, H, 0, int(wide), A, 2, 1 << 24, 1 << 12, 1 << 30, 3, 5, SEED,
                                 tours.data_ptr(), keys.data_ptr(), durs.data_ptr(), veh.data_ptr(),
                                 ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_aco:" in msg and b"bytes of LDS" in msg
    assert str(lds_bytes(N, K, H, wide, A)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item()
    assert (durs == -7).all().item() and (veh == -7).all().item()


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", [A_EDGES[3], WAVES[4]], ids=run_id)
def test_gpu_equals_the_unbatched_runner(ctx, run, objective):
    """With the runner's pheromone parameters the batched row is the
    best-so-far of ACORunner(colonies=1) stepped I times, one iteration each."""
    case, A, I, _ = run
    D, dem, caps, starts = inst(case)
    batched = gpu_runs(ctx, [run], objective)
    ctx.set_instance(CVRP, D, dem, list(caps), list(starts), objective=obj_id(objective))
    r = runners.ACORunner(ctx, case[0], colonies=1, ants=A, seed=SEED)
    assert (r.tau_min, r.tau_max, r.evap_shift, r.bsf_period) == (1 << 12, 1 << 30, 3, 5)
    for _ in range(I):
        r.epoch(1)
    key = int(r.best_key[0].item()) & (2**64 - 1)
    tour = r.best_t[0].cpu().tolist()
    ref = reference(run, objective)
    print(run_id(run), objective, "batched", batched[0][0], "runner", key, "ref", ref["key"])
    assert (key, tour) == (ref["key"], ref["tour"])
    assert (batched[0][0], batched[1][0]) == (key, tour)


def _ref_dict(case, objective, A, I, base=0):
    """The reference as solve_vrp's slot dict (nodes are matrix rows: with no
    customer left out, the compact indices)."""
    r = reference((case, A, I, ()), objective)
    routes = [[] for _ in r["durs"]]
    unv = []
    for c, v in zip(r["tour"], r["veh"]):
        (routes[v] if v >= 0 else unv).append(base + c)
    return {"durationMax": max(r["durs"]), "durationSum": sum(r["durs"]), "unvisited": unv,
            "vehicles": [{"tour": [base] + rt + [base], "duration": d}
                         for rt, d in zip(routes, r["durs"])]}


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_aco_batch_mixed_list(objective):
    A, I = 32, 5
    D7, locs7, caps7, starts7 = request((6, 2, 24, 50, ""), 100)
    inside = {0: (6, 2, 24, 51, ""), 1: (9, 3, 1, 52, ""), 3: (6, 2, 24, 53, ""), 6: (9, 3, 1, 54, "")}
    reqs = [request(inside[0], 100), request(inside[1], 100),
            (D7, locs7, caps7, starts7, [100 + i for i in range(1, 7)]),            # none active
            request(inside[3], 100),
            (D7, locs7, [1] * 65, [0] * 65),                                        # K = 65: outside
            {"durations": D7, "locations": locs7, "capacities": caps7, "start_times": starts7,
             "ignored_customers": [103]},
            request(inside[6], 100)]
    assert not solver.batch_aco_fits(solver.compact_vrp(*reqs[4]), A, I)
    kw = dict(ants=A, iters=I, seed=SEED, objective=objective, with_unvisited=True)
    got = solver.solve_vrp_aco_batch(reqs, **kw)
    assert got[2] == {"durationMax": 0, "durationSum": 0, "unvisited": [],
                      "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    for x, (r, res) in enumerate(zip(reqs, got)):
        if isinstance(r, dict):
            r = (r["durations"], r["locations"], r["capacities"], r["start_times"],
                 r["ignored_customers"])
        _rescored(r, res, objective)
    assert got[4] == solver.solve_vrp("aco", *reqs[4], seed=SEED, objective=objective,
                                      with_unvisited=True, iteration_count=I, ants=A)
    # the answers of the requests inside the domain are A24's
    for x, case in inside.items():
        assert got[x] == _ref_dict(case, objective, A, I)
    # deterministic, and the same alone as in company
    assert solver.solve_vrp_aco_batch(reqs, **kw) == got
    for x in (0, 1, 5):
        assert solver.solve_vrp_aco_batch([reqs[x]], **kw) == [got[x]]
    assert "unvisited" not in solver.solve_vrp_aco_batch([reqs[0]], ants=A, iters=I, seed=SEED)[0]


@pytest.mark.gpu
def test_service_batch_vrp_aco_equals_solve_vrp_aco_batch(monkeypatch):
    windows = []
    sleep = service.time.sleep
    monkeypatch.setattr(service.time, "sleep",
                        lambda s: (windows.append(s) if s == 0.05 else None, sleep(s)))
    A, I = 48, 6
    D, locs, caps, starts = request((8, 3, 1, 59, ""), 100)
    store = service.MemoryStore({"7": locs}, {"8": D}, {})
    app = service.App(store, seed=SEED, batch_vrp_aco=True, batch_window_s=0.05,
                      batch_aco_iterations=I, batch_aco_ants=A)
    api = json.dumps({"solutionName": "s", "solutionDescription": "d", "locationsKey": 7,
                      "durationsKey": 8, "capacities": caps, "startTimes": starts,
                      "ignoredCustomers": [], "completedCustomers": []}).encode()
    cases = [((6, 2, 24, 60 + x, "") if x % 2 else (8, 3, 1, 60 + x, "")) for x in range(24)]

    def call(x):
        if x >= len(cases):
            return app.post("vrp", "aco", api)
        return app.solve_inline("vrp", "aco", _body(cases[x], seed=x + 1, timeLimit=0.001))

    out = _concurrently(call, len(cases) + 4)
    b = app.vrp_aco_batcher
    assert b.requests == 28 and 2 <= b.launches <= 2 * len(windows)
    assert b.launches < b.requests
    for x, (st, res) in enumerate(out):
        assert st == 200, res
        req = request(cases[x], 100) if x < len(cases) else (D, locs, caps, starts)
        assert [res["message"]] == solver.solve_vrp_aco_batch([req], ants=A, iters=I, seed=SEED)
    assert out[0][1]["message"] == {k: v for k, v in _ref_dict(cases[0], "sum", A, I).items()
                                    if k != "unvisited"}
