"""Batched VRP multi-start local search (spec A25): the C entry points
vrpms_vrp_batch_ls_lds / vrpms_vrp_batch_ls, Context.vrp_batch_ls,
solver.batch_ls_key / batch_ls_fits / solve_vrp_ls_batch, solve_vrp("ls") and
the service's local-search batcher (App(batch_vrp_ls=True)).

The reference is a25_ref below: A23's Philox Fisher-Yates starts, per round
spec.apply_move on every (typ, i, j) priced by spec.eval_cvrp_batch, the least
(key, typ, i, j) applied while it improves, the least (key, start) of the end
tours, and spec.eval_cvrp for the durations and vehicles.  Per request the GPU
must return the identical key, tour, route durations, vehicle row and info
row, for both objectives."""
import ctypes
import functools
import json
import threading
import urllib.request

import numpy as np
import pytest

from oracle import spec
from test_vrp_batch_ga import (_FakeApp, _body, _concurrently, _fake_launch, _locs, _no_gpu,
                               _rescored, _sized)
from test_vrp_batch_ga import inst as ga_inst
from vrpms_amd import _lib, core, service, solver

LDS_BYTES = 160 * 1024
OBJECTIVES = ("sum", "max")
SEED = 20251
M32 = 0xFFFFFFFF


def obj_id(objective):
    return spec.OBJ_SUM if objective == "sum" else spec.OBJ_MAX


# ---------------------------------------------------------------------------
# instances and their references (computed once, shared, never changed)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inst(case):
    """tests/test_vrp_batch_ga.py's inst family, plus the variant "ties":
    entries 1..2, so distinct moves give equal keys."""
    n, K, H, seed, variant = case
    if variant != "ties":
        return ga_inst(case)
    D, dem, caps, starts = ga_inst((n, K, H, seed, ""))
    rng = np.random.default_rng(9100 + seed)
    D = rng.integers(1, 3, size=D.shape, dtype=np.int64)
    for h in range(H):
        np.fill_diagonal(D[h], 0)
    D.setflags(write=False)
    return D, dem, caps, starts


@functools.lru_cache(maxsize=None)
def all_moves(n):
    """Every (typ, i, j) of a round in the order ties break by."""
    tri = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return [(0, i, j) for i, j in tri] + [(1, i, j) for i, j in tri] + \
        [(2, i, j) for i in range(n) for j in range(n) if i != j]


def a25_ref(D, dem, caps, starts, objective, S, rounds, seed):
    """Spec A25 -> dict(key, tour, durs, veh, s, capped, unvisited, move_tie,
    end_tie, rounds, moves): move_tie = some round had its least key on two
    moves that give different tours, end_tie = two starts ended on the same
    key, rounds = the number of applied moves of every descent, moves = the
    applied (typ, i, j) of all of them."""
    D = spec.as_3d(D)
    n = D.shape[1] - 1
    skey = spec.seed_key(seed)
    caps, starts, obj = list(caps), list(starts), obj_id(objective)
    moves = all_moves(n)
    ends, capped, move_tie, applied_all, took = [], 0, False, [], []
    for s in range(S):
        t = list(range(1, n + 1))
        for q in range(n - 1, 0, -1):
            j = spec.philox4x32_10((M32, M32, s, q), skey)[0] % (q + 1)
            t[q], t[j] = t[j], t[q]
        k = int(spec.eval_cvrp_batch(D, [t], dem, caps, starts, obj)[0][0])
        applied = 0
        while n >= 2:
            if applied >= rounds:
                capped += 1
                break
            cands = [spec.apply_move(t, *m) for m in moves]
            keys = [int(x) for x in spec.eval_cvrp_batch(D, cands, dem, caps, starts, obj)[0]]
            kmin = min(keys)
            if not kmin < k:
                break
            first = keys.index(kmin)   # the moves are in (typ, i, j) order
            move_tie |= any(kk == kmin and c != cands[first] for kk, c in zip(keys, cands))
            t, k = cands[first], kmin
            took.append(moves[first])
            applied += 1
        ends.append((k, s, t))
        applied_all.append(applied)
    k, s, t = min(ends, key=lambda e: e[:2])
    final = spec.eval_cvrp(D, t, dem, caps, starts, obj)
    assert final["key"] == k
    return dict(key=k, tour=t, durs=final["durations"], veh=final["vehicle_of"], s=s, capped=capped,
                unvisited=final["unvisited"], move_tie=move_tie,
                end_tie=len({e[0] for e in ends}) < len(ends), rounds=applied_all, moves=took)


@functools.lru_cache(maxsize=None)
def reference(run, objective):
    """run = (case, S, rounds)."""
    case, S, rounds = run
    return a25_ref(*inst(case), objective, S, rounds, SEED)


def expected(runs, objective):
    refs = [reference(r, objective) for r in runs]
    return ([r["key"] for r in refs], [r["tour"] for r in refs], [r["durs"] for r in refs],
            [r["veh"] for r in refs], [[r["s"], r["capped"]] for r in refs])


def pad(x, m):
    return (x + m - 1) // m * m


def lds_bytes(N, K, H, wide):
    """DESIGN.md §4.3p restated: the matrix padded to 16 bytes, the demand row
    and the two fleet rows as int32 padded to four words, two uint16 tours of
    n genes padded to eight per wavefront, and 16 bytes per wavefront."""
    return pad(H * N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + \
        4 * 2 * 2 * pad(N - 1, 8) + 4 * 16


def sa_lds_bytes(N, K, H, wide):
    """DESIGN.md §4.3m restated (A22): twelve tours of n + K - 1 tokens and
    four keys."""
    return pad(H * N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + \
        4 * 3 * 2 * pad(N - 1 + K - 1, 8) + 4 * 8


def largest_n_nodes(K, H, wide):
    return max(N for N in range(2, 400) if lds_bytes(N, K, H, wide) <= LDS_BYTES)


# DESIGN.md §4.3p's domain table (K = 4): (H, wide) -> the largest N
DOMAIN = {(24, False): 58, (24, True): 41, (1, False): 281, (1, True): 199}

# the runs of the GPU comparisons: (case, S, rounds)
N_EDGES = [((n, 3, 1, n, ""), 6, 1000) for n in (1, 2, 3, 4, 5, 6, 7, 8, 11, 12)]
WAVES = [((n, 4, 1, 80 + n, ""), 5, 2 if n < 64 else 1) for n in (31, 32, 33, 64, 65)]
S_EDGES = [((9, 3, 24, 70, ""), S, 1000) for S in (1, 3, 4, 5, 8, 9, 64)]
R_EDGES = [((8, 3, 1, 9, ""), 7, rounds) for rounds in (0, 1, 2, 1000)]
TIES = [((7, 2, 1, 3, "ties"), 12, 1000), ((6, 3, 24, 4, "ties"), 9, 1000)]
VARIANTS = [((6, 3, 24, 10, "hours"), 8, 1000), ((6, 3, 24, 11, "hours"), 8, 1000),
            ((9, 5, 24, 13, "zerocap"), 8, 1000), ((9, 3, 1, 14, "zerodem"), 8, 1000),
            ((6, 3, 24, 73, "below"), 8, 1000), ((3, 64, 1, 12, ""), 8, 1000),
            ((7, 3, 1, 31, "e65536"), 8, 1000)]
# the in-place move works by chunks of 64 positions: relocates over more than
# 64 positions either way and a reversal of more than 128
LONG = [((135, 4, 1, seed, ""), 1, 1) for seed in (314, 330, 316)]
ALL_RUNS = N_EDGES + WAVES + S_EDGES + R_EDGES + TIES + VARIANTS + LONG
SIX = [((10, 3, 24, 20 + x, ""), 16, 1000) for x in range(6)]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


GRID_N = list(range(2, 70)) + [96, 97, 128, 129]


def test_lds_bytes_formula_monotone_and_refusals(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_vrp_batch_ls_lds
    for H in (1, 24):
        for wide in (0, 1):
            for K in (1, 4, 5, 64):
                for N in GRID_N:
                    assert f(N, K, H, wide, ctypes.byref(b)) == _lib.VRPMS_OK
                    assert b.value == lds_bytes(N, K, H, wide) == core.vrp_batch_ls_lds(N, K, H, wide)
                    if N > 2:
                        assert b.value >= lds_bytes(N - 1, K, H, wide)
    for args, word in (((1, 3, 1, 0), b"2 <= N"), ((0, 3, 1, 0), b"2 <= N"),
                       ((65536, 3, 1, 0), b"2 <= N"),
                       ((5, 0, 1, 0), b"1 <= K <= 64"), ((5, 65, 1, 0), b"1 <= K <= 64"),
                       ((5, 3, 2, 0), b"H must be 1 or 24"), ((5, 3, 0, 0), b"H must be 1 or 24"),
                       ((5, 3, 1, 2), b"wide"), ((5, 3, 1, -1), b"wide")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_ls_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(5, 3, 1, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_ls_lds" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= K <= 64"):
        core.vrp_batch_ls_lds(5, 65, 1, False)
    assert solver.BATCH_LS_LDS_BYTES == solver.BATCH_SA_LDS_BYTES == LDS_BYTES
    assert solver.BATCH_LS_MAX_STARTS == 1024 and solver.BATCH_LS_MAX_ROUNDS == 1000


def test_lds_need_is_at_most_the_annealers(lib):
    """A25's domain contains A22's: at every point of the grid, and at A22's
    own edge, the bytes are at most vrpms_vrp_batch_sa_lds's."""
    for H in (1, 24):
        for wide in (0, 1):
            for K in (1, 4, 5, 64):
                for N in GRID_N + [278, 279, 286, 287, 1000]:
                    sa = core.vrp_batch_sa_lds(N, K, H, wide)
                    assert sa == sa_lds_bytes(N, K, H, wide)
                    assert core.vrp_batch_ls_lds(N, K, H, wide) <= sa, (N, K, H, wide)


def test_argument_errors_need_no_gpu(lib):
    """Every argument check comes before the context is looked at, so a
    stand-in block of zeros serves as the non-NULL ctx here; its LDS size of
    zero makes every launch that passes the other checks an LDS refusal."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(4096)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    names = ("m", "d", "cp", "st", "t", "k", "du", "v", "i")

    def f(ctx=c, R=1, N=5, K=2, H=1, obj=0, wide=0, S=8, rounds=3, **ptrs):
        a = {name: ptrs.get(name, p) for name in names}
        return lib.vrpms_vrp_batch_ls(ctx, a["m"], a["d"], a["cp"], a["st"], R, N, K, H, obj, wide, S,
                                      rounds, 12345, a["t"], a["k"], a["du"], a["v"], a["i"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_ls:" in msg and word in msg, (kw, msg)

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
    for S in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= S <= 65535 (%d given)" % S, S=S)
    refused(b"rounds must not be negative (-1 given)", rounds=-1)
    for name in names:
        refused(b"NULL", **{name: None})
    refused(b"H must be 1 or 24", R=0, H=3)            # the shape checks also with R = 0
    refused(b"1 <= S <= 65535", R=0, S=0)
    for N, K, H, wide in ((5, 2, 1, 0), (58, 4, 24, 0), (59, 4, 24, 1)):
        refused(b"needs %d bytes of LDS (0 available)" % lds_bytes(N, K, H, wide), N=N, K=K, H=H,
                wide=wide)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, S=65535, rounds=2**31 - 1) == _lib.VRPMS_OK
    assert f(R=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert buf.raw == bytes(4096) and fake.raw == bytes(1 << 16)


def request(case, base=0):
    """The case as a solve_vrp_ls_batch tuple (H = 1 as a plain [N][N] matrix)."""
    D, dem, caps, starts = inst(case)
    return ((D[0] if D.shape[0] == 1 else D).tolist(), _locs(dem, base), list(caps), list(starts))


def compact(case):
    return solver.compact_vrp(*request(case))


def test_batch_ls_fits_at_the_lds_edge(lib):
    for (H, wide), N in DOMAIN.items():
        assert largest_n_nodes(4, H, wide) == N, (H, wide, largest_n_nodes(4, H, wide))
        assert lds_bytes(N, 4, H, wide) <= LDS_BYTES < lds_bytes(N + 1, 4, H, wide)
        big = 70000 if wide else 0
        assert solver.batch_ls_fits(_sized(N, 4, H, big), 64, 1000)
        assert not solver.batch_ls_fits(_sized(N + 1, 4, H, big), 64, 1000)
        assert "bytes" in solver.batch_ls_message(_sized(N + 1, 4, H, big), 64, 1000)
        assert solver.batch_ls_key(_sized(N, 4, H, big), 64, 1000) == (N, 4, H, wide, 64, 1000)
        # A22 fits no more: 57 / 278 customers at uint16 cells
        assert N >= max(M for M in range(2, 400) if sa_lds_bytes(M, 4, H, wide) <= LDS_BYTES)
    assert DOMAIN[(24, False)] - 1 >= 57 and DOMAIN[(1, False)] - 1 >= 278
    small = _sized(6, 2, 24)
    assert solver.batch_ls_fits(small, 1024, 1000) and solver.batch_ls_fits(small, 1, 0)
    assert not solver.batch_ls_fits(small, 1025, 10) and not solver.batch_ls_fits(small, 0, 10)
    assert not solver.batch_ls_fits(small, 64, 1001) and not solver.batch_ls_fits(small, 64, -1)
    assert "starts" in solver.batch_ls_message(small, 1025, 10)
    assert "rounds" in solver.batch_ls_message(small, 64, 1001)
    # a wide entry halves the cells that fit; 65535 is still narrow
    N = DOMAIN[(24, False)]
    assert not solver.batch_ls_fits(_sized(N, 4, 24, 70000), 64, 1000)
    assert solver.batch_ls_fits(_sized(N, 4, 24, 65534), 64, 1000)
    # outside the domain whatever the size
    assert "vehicles" in solver.batch_ls_message(_sized(5, 65, 1), 8, 4)
    none = solver.compact_vrp(np.ones((3, 3), dtype=np.int64), _locs([0, 1, 1]), [3], [0], [1, 2])
    assert none.n == 0 and not solver.batch_ls_fits(none, 8, 4)
    tsp = solver.compact_tsp(np.ones((4, 4), dtype=np.int64), [1, 2, 3], 0, 0)
    assert not solver.batch_ls_fits(tsp, 8, 4)
    b = service.VrpLsBatcher(_FakeApp(), launch=_fake_launch([]))
    assert (b.starts, b.rounds) == (64, 1000)
    assert b.accepts(small) and not b.accepts(_sized(6, 2, 1, 2**29))               # the A9 guard
    assert not b.accepts(_sized(5, 65, 1))
    for kw in (dict(starts=0), dict(starts=1025), dict(rounds=-1), dict(rounds=1001)):
        with pytest.raises(ValueError, match="starts|rounds"):
            service.VrpLsBatcher(_FakeApp(), launch=_fake_launch([]), **kw)


def test_solve_vrp_ls_batch_refusals_need_no_gpu(monkeypatch, lib):
    _no_gpu(monkeypatch)
    good = request((6, 2, 1, 0, ""))
    assert solver.solve_vrp_ls_batch([]) == []
    with pytest.raises(ValueError, match=r"^request 1: capacities and startTimes"):
        solver.solve_vrp_ls_batch([good, (good[0], good[1], [3, 3], [0])])
    with pytest.raises(ValueError, match=r"^request 2: 5 locations but a 7-node"):
        solver.solve_vrp_ls_batch([good, good, {"durations": good[0], "locations": good[1][:5],
                                                "capacities": [3], "start_times": [0]}])
    big = np.full((7, 7), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_vrp_ls_batch([good, (big.tolist(), good[1], [3, 3], [0, 0])])
    heavy = [{"id": i, "demand": 2**30} for i in range(7)]
    with pytest.raises(ValueError, match=r"^request 0: capacity \+ demand overflows int32"):
        solver.solve_vrp_ls_batch([(good[0], heavy, [2**30, 3], [0, 0])])
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp_ls_batch([good], objective="mean")
    for starts in (0, -1, 1025):
        with pytest.raises(ValueError, match=r"starts must be in 1\.\.1024"):
            solver.solve_vrp_ls_batch([good], starts=starts)
    for rounds in (-1, 1001):
        with pytest.raises(ValueError, match=r"rounds must be in 0\.\.1000"):
            solver.solve_vrp_ls_batch([good], rounds=rounds)
    # outside the domain there is no other path: the limit that failed, by request
    with pytest.raises(ValueError, match=r"^request 1: ls \(local search\) supports 1\.\.64 vehicles "
                                         r"\(65 given\)"):
        solver.solve_vrp_ls_batch([good, (good[0], good[1], [1] * 65, [0] * 65)])
    Nbig = DOMAIN[(1, False)] + 1
    bigD = np.ones((Nbig, Nbig), dtype=np.int64).tolist()
    need = lds_bytes(Nbig, 4, 1, False)
    with pytest.raises(ValueError, match=rf"^request 0: ls .* need {need} bytes; the limit is "
                                         rf"{LDS_BYTES} bytes"):
        solver.solve_vrp_ls_batch([(bigD, _locs([0] + [1] * (Nbig - 1)), [Nbig] * 4, [0] * 4)])
    # no customer: solve_vrp's trivial answer, built on the host
    none = (good[0], good[1], [3, 3], [0, 7], [1, 2, 3, 4, 5, 6])
    trivial = {"durationMax": 0, "durationSum": 0, "unvisited": [],
               "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    assert solver.solve_vrp_ls_batch([none], with_unvisited=True) == [trivial]
    assert solver.solve_vrp("ls", *none, with_unvisited=True) == trivial


def test_solve_vrp_ls_and_solve_tsp_ls_errors(monkeypatch, lib):
    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: pytest.fail("the remote was touched"))
    assert "ls" in solver.ALGORITHMS
    D, locs, caps, starts = request((6, 2, 1, 0, ""))
    with pytest.raises(ValueError, match="ls solves the VRP only"):
        solver.solve_tsp("ls", D, [1, 2, 3], 0, 0)
    with pytest.raises(ValueError, match=r"1\.\.64 vehicles \(65 given\)"):
        solver.solve_vrp("ls", D, locs, [1] * 65, [0] * 65)
    with pytest.raises(ValueError, match=r"1\.\.1024 starts \(1025 given\)"):
        solver.solve_vrp("ls", D, locs, caps, starts, starts=1025)
    with pytest.raises(ValueError, match=r"1\.\.1024 starts \(0 given\)"):
        solver.solve_vrp("ls", D, locs, caps, starts, starts=0)
    with pytest.raises(ValueError, match=r"0\.\.1000 rounds \(1001 given\)"):
        solver.solve_vrp("ls", D, locs, caps, starts, rounds=1001)
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp("ls", D, locs, caps, starts, objective="mean")
    big = np.full((7, 7), 2**29, dtype=np.int64).tolist()
    with pytest.raises(ValueError, match="A9 guard"):
        solver.solve_vrp("ls", big, locs, caps, starts)
    Nbig = DOMAIN[(24, False)] + 1
    bigD = np.ones((24, Nbig, Nbig), dtype=np.int64).tolist()
    with pytest.raises(ValueError, match=r"need \d+ bytes; the limit is 163840 bytes"):
        solver.solve_vrp("ls", bigD, _locs([0] + [1] * (Nbig - 1)), [Nbig] * 4, [0] * 4)


def test_app_batch_vrp_ls_routes(monkeypatch, lib):
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, len(params["capacities"]), dict(knobs.get("inline") or {})))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    assert "ls" in service.INLINE_ALGORITHMS["vrp"] and "ls" not in service.INLINE_ALGORITHMS["tsp"]
    assert service.INLINE_ALGORITHMS["vrp"][-1] == "sp" and "ls" not in service.TITLES
    # the flag is off: the injected solve
    off = service.App(service.MemoryStore({}, {}, {}), solve=fake)
    assert off.vrp_ls_batcher is None
    assert off.solve_inline("vrp", "ls", _body((5, 2, 1, 0, "")))[1]["message"]["durationSum"] == 3
    assert seen == [("vrp", "ls", 2, {})]
    del seen[:]
    st, res = off.solve_inline("tsp", "ls", b"{}")
    assert st == 400 and "no solver /solve/tsp/ls" in res["errors"][0]["reason"]

    app = service.App(service.MemoryStore({}, {}, {}), solve=fake, batch_vrp_ls=True,
                      batch_window_s=0.2, batch_vrp_ls_launch=_fake_launch(launched),
                      batch_ls_starts=16, batch_ls_rounds=7)
    assert isinstance(app.vrp_ls_batcher, service.VrpLsBatcher)
    assert isinstance(app.vrp_ls_batcher, service.VrpSaBatcher)
    assert (app.vrp_ls_batcher.starts, app.vrp_ls_batcher.rounds) == (16, 7)
    assert app.vrp_sa_batcher is None and app.vrp_ga_batcher is None and app.vrp_aco_batcher is None

    def call(x):
        if x < 4:
            return app.solve_inline("vrp", "ls", _body((5, 2, 1, x, ""), seed=x, timeLimit=1.0))
        if x < 6:
            return app.solve_inline("vrp", "ls", _body((5, 2, 1, x, ""), objective="max"))
        return app.solve_inline("vrp", "ls", _body((6, 3, 24, x, "")))

    out = _concurrently(call, 8)
    assert all(st == 200 for st, _ in out), out
    assert sorted(launched) == [((6, 2, 1, False, "max"), 2), ((6, 2, 1, False, "sum"), 4),
                                ((7, 3, 24, False, "sum"), 2)]
    assert seen == [] and app.vrp_ls_batcher.requests == 8
    assert out[0][1]["message"]["vehicles"][0]["tour"] == [0, 5, 4, 3, 2, 1, 0]

    # every rule that sends a request down the unbatched path, one by one
    def unbatched(status_and_result, K=2, algorithm="ls", inline=None):
        assert status_and_result[0] == 200, status_and_result
        assert seen == [("vrp", algorithm, K, inline or {})]
        del seen[:]

    body = functools.partial(_body, (5, 2, 1, 1, ""))
    unbatched(app.solve_inline("vrp", "ls", body(knobs={"starts": 8})), inline={"starts": 8})
    unbatched(app.solve_inline("vrp", "ls", body(knobs={"rounds": 0})), inline={"rounds": 0})
    D, locs, caps, starts = request((5, 2, 1, 1, ""), 100)
    wide_fleet = json.dumps({"durations": D, "locations": locs, "capacities": [1] * 65,
                             "startTimes": [0] * 65, "ignoredCustomers": [],
                             "completedCustomers": []}).encode()
    unbatched(app.solve_inline("vrp", "ls", wide_fleet), K=65)                         # the domain
    unbatched(app.solve_inline("vrp", "sa", body()), algorithm="sa")                   # another algorithm
    assert len(launched) == 3
    for knobs in ({"starts": 0}, {"starts": 1025}, {"rounds": -1}, {"rounds": 1001}):
        st, res = app.solve_inline("vrp", "ls", body(knobs=knobs))
        assert st == 400 and "outside" in res["errors"][0]["reason"], res
    # a bad instance is a 400 in solve_vrp's words; so is one outside the domain
    # on the real unbatched path, before any device is touched
    _no_gpu(monkeypatch)
    real = service.App(service.MemoryStore({}, {}, {}), batch_vrp_ls=True, batch_window_s=0.2,
                       batch_vrp_ls_launch=_fake_launch(launched))
    st, res = real.solve_inline("vrp", "ls", body(startTimes=[0]))
    assert st == 400 and "capacities and startTimes" in res["errors"][0]["reason"]
    st, res = real.solve_inline("vrp", "ls", wide_fleet)
    assert st == 400 and "1..64 vehicles (65 given)" in res["errors"][0]["reason"]
    assert len(launched) == 3


def test_cli_flags(monkeypatch, capsys):
    made = {}

    class Stop(Exception):
        pass

    def app(store, **kw):
        made.update(kw)
        raise Stop

    monkeypatch.setattr(service, "App", app)
    for argv, want in ((["--batch-vrp-ls"], (True, 64, 1000)), ([], (False, 64, 1000)),
                       (["--batch-vrp-ls", "--batch-ls-starts", "1024", "--batch-ls-rounds", "0"],
                        (True, 1024, 0))):
        with pytest.raises(Stop):
            service.main(argv)
        assert (made["batch_vrp_ls"], made["batch_ls_starts"], made["batch_ls_rounds"]) == want
        assert made["batch_vrp_aco"] is False
    for argv in (["--batch-ls-starts", "0"], ["--batch-ls-starts", "1025"],
                 ["--batch-ls-rounds", "-1"], ["--batch-ls-rounds", "1001"]):
        with pytest.raises(SystemExit):
            service.main(argv)
    capsys.readouterr()


def _improving(case, tour, key, objective):
    D, dem, caps, starts = inst(case)
    cands = [spec.apply_move(tour, *m) for m in all_moves(len(tour))]
    keys = spec.eval_cvrp_batch(D, cands, dem, list(caps), list(starts), obj_id(objective))[0]
    return min(int(k) for k in keys) < key


def test_reference_properties():
    """What the GPU comparisons rely on, checked on the reference itself."""
    refs = {(run, o): reference(run, o) for run in ALL_RUNS for o in OBJECTIVES}
    # both tie flags, somewhere in the list and on the "ties" runs
    assert any(r["move_tie"] for r in refs.values()) and any(r["end_tie"] for r in refs.values())
    assert all(reference(run, "sum")["move_tie"] and reference(run, "sum")["end_tie"] for run in TIES)
    # the move order: the triangles, then relocate with i != j; 2 n (n - 1) in all
    assert all_moves(3) == [(0, 0, 1), (0, 0, 2), (0, 1, 2), (1, 0, 1), (1, 0, 2), (1, 1, 2),
                            (2, 0, 1), (2, 0, 2), (2, 1, 0), (2, 1, 2), (2, 2, 0), (2, 2, 1)]
    assert all(len(all_moves(n)) == 2 * n * (n - 1) for n in range(1, 14))
    # with the round cap out of reach no descent is capped and the answer
    # admits no improving move
    for run in N_EDGES + S_EDGES + TIES + VARIANTS + R_EDGES[-1:]:
        for o in OBJECTIVES:
            r = refs[(run, o)]
            assert r["capped"] == 0 and max(r["rounds"]) < run[2]
            if run[0][0] >= 2:
                assert not _improving(run[0], r["tour"], r["key"], o), (run, o)
    # the key never rises with S
    keys = [refs[(run, "sum")]["key"] for run in S_EDGES]
    assert keys == sorted(keys, reverse=True) and keys[-1] < keys[0]
    # rounds = 0 caps every descent, a small cap some of them, and the key
    # never rises with the cap
    caps = [refs[(run, "sum")]["capped"] for run in R_EDGES]
    assert caps[0] == 7 and 0 < caps[2] <= caps[1] <= 7 and caps[3] == 0
    keys = [refs[(run, "sum")]["key"] for run in R_EDGES]
    assert keys[0] > keys[1] >= keys[2] >= keys[3]
    assert all(0 < r["capped"] for run in WAVES for r in (refs[(run, "sum")],))
    # the first move of the long runs: a relocate up and one down over more than
    # 64 positions, a reversal of more than 128
    took = [refs[(run, o)]["moves"][0] for run in LONG for o in OBJECTIVES]
    assert any(typ == 2 and j - i > 64 for typ, i, j in took)
    assert any(typ == 2 and i - j > 64 for typ, i, j in took)
    assert any(typ == 1 and j - i + 1 > 128 for typ, i, j in took)
    assert {typ for r in refs.values() for typ, _, _ in r["moves"]} == {0, 1, 2}
    # n = 1 has no moves: not capped even at rounds = 0; start 0 wins every tie
    one = a25_ref(*inst((1, 3, 1, 1, "")), "sum", 5, 0, SEED)
    assert (one["tour"], one["s"], one["capped"]) == ([1], 0, 0)
    # "below": every key equal, no move applied, start 0 the answer
    r = refs[(VARIANTS[4], "max")]
    assert r["unvisited"] == 6 and r["s"] == 0 and r["rounds"] == [0] * 8 and r["end_tie"]
    assert any(0 < r["unvisited"] < len(r["tour"]) for r in refs.values())
    # a winner from every wavefront, and one beyond the first sweep of four
    assert {r["s"] % 4 for r in refs.values()} == {0, 1, 2, 3}
    assert any(r["s"] >= 4 for r in refs.values())
    # the hour cases cross an hour and midnight: the static slice gives another answer
    for run in VARIANTS[:2]:
        D, dem, caps_, starts = inst(run[0])
        r = reference(run, "sum")
        flat = spec.eval_cvrp(D[:1], r["tour"], dem, list(caps_), list(starts))
        assert flat["key"] != r["key"]
        assert any(s >= 23 * 60 and s + d >= 1440 for s, d in zip(starts, r["durs"]) if d)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_batch(ctx, cases, objective, S, rounds, wide=None):
    """One vrp_batch_ls launch -> ([key], [tour], [durs], [veh], [info])."""
    import torch
    insts = [inst(c) for c in cases]

    def dev(rows):
        return torch.tensor(np.stack(rows), dtype=torch.int32, device=ctx.dev)

    tours, keys, durs, veh, info = ctx.vrp_batch_ls(
        dev([D for D, _, _, _ in insts]), dev([d for _, d, _, _ in insts]),
        dev([np.array(c) for _, _, c, _ in insts]), dev([np.array(s) for _, _, _, s in insts]),
        obj_id(objective), S, rounds, SEED, wide=wide)
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), veh.cpu().tolist(), info.cpu().tolist())


def gpu_runs(ctx, runs, objective, wide=None):
    """Runs of one (S, rounds) in one launch."""
    assert len({r[1:] for r in runs}) == 1 and len(runs) <= 16
    return gpu_batch(ctx, [r[0] for r in runs], objective, *runs[0][1:], wide=wide)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", ALL_RUNS, ids=lambda r: "n%d-K%d-H%d-s%d%s-S%d-r%d" % (*r[0], *r[1:]))
def test_gpu_equals_reference(ctx, run, objective):
    got = gpu_runs(ctx, [run], objective)
    want = expected([run], objective)
    print(run, objective, "gpu", got, "ref", want)
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_staging_width_and_refusals(ctx, objective):
    """All four instantiations, (uint16 | int32) x (H = 1 | 24), and the
    refusal row between two healthy requests."""
    import torch
    S, rounds = 6, 1000
    for H in (1, 24):
        a, b, c = (7, 3, H, 30, ""), (7, 3, H, 31, "e65535"), (7, 3, H, 32, "")
        over = (7, 3, H, 31, "e65536")

        def runs(*cases):
            return [(x, S, rounds) for x in cases]

        assert gpu_runs(ctx, runs(a, b, c), objective, wide=False) == expected(runs(a, b, c), objective)
        assert gpu_runs(ctx, runs(a, over, c), objective, wide=True) == \
            expected(runs(a, over, c), objective)
        assert gpu_runs(ctx, runs(over), objective) == expected(runs(over), objective)   # wide=None
        want = expected(runs(a, over, c), objective)
        keys, tours, durs, veh, info = gpu_runs(ctx, runs(a, over, c), objective, wide=False)
        assert keys[1] == 2**64 - 1 and tours[1] == [0] * 7 and durs[1] == [0] * 3 and \
            veh[1] == [-1] * 7 and info[1] == [-1, 0]
        for x in (0, 2):
            assert (keys[x], tours[x], durs[x], veh[x], info[x]) == tuple(w[x] for w in want)
        # a negative entry, under either width
        insts = [inst(x) for x in (a, b, c)]
        mats = np.stack([D for D, _, _, _ in insts]).astype(np.int32)
        mats[1, H - 1, 3, 2] = -1

        def dev(x):
            return torch.tensor(np.asarray(x), dtype=torch.int32, device=ctx.dev)

        for wide in (False, True):
            tours, keys, durs, veh, info = ctx.vrp_batch_ls(
                dev(mats), dev(np.stack([d for _, d, _, _ in insts])),
                dev([c_ for _, _, c_, _ in insts]), dev([s for _, _, _, s in insts]),
                obj_id(objective), S, rounds, SEED, wide=wide)
            want = expected(runs(a, b, c), objective)
            assert keys[1].item() == -1 and tours[1].tolist() == [0] * 7 and \
                durs[1].tolist() == [0] * 3 and veh[1].tolist() == [-1] * 7 and \
                info[1].tolist() == [-1, 0]
            for x in (0, 2):
                assert (int(keys[x].item()) & (2**64 - 1), tours[x].tolist(), durs[x].tolist(),
                        veh[x].tolist(), info[x].tolist()) == tuple(w[x] for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_rounds_zero_is_the_ga_start(ctx, objective):
    """No oracle involved: rounds = 0 is A23's answer at P = S, G = 0."""
    import torch
    for case in ((9, 3, 24, 70, ""), (12, 3, 1, 12, ""), (65, 4, 1, 145, ""), (1, 3, 1, 1, "")):
        D, dem, caps, starts = inst(case)

        def dev(x):
            return torch.tensor(np.asarray(x)[None], dtype=torch.int32, device=ctx.dev)

        args = (dev(D), dev(dem), dev(caps), dev(starts), obj_id(objective))
        for S in (2, 5, 64, 256):
            ga = ctx.vrp_batch_ga(*args, S, 0, 0.2, SEED)
            ls = ctx.vrp_batch_ls(*args, S, 0, SEED)
            for g, l in zip(ga, ls[:4]):
                assert torch.equal(g, l), (case, S)
            assert ls[4][0, 1].item() == (S if case[0] >= 2 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_batch_independence(ctx, objective):
    import torch
    want = expected(SIX, objective)
    together = gpu_runs(ctx, SIX, objective)
    assert together == want
    for x, run in enumerate(SIX[:2]):
        assert gpu_runs(ctx, [run], objective) == tuple([g[x]] for g in together)
    order = [5, 4, 3, 2, 1, 0, 5, 0, 3, 3, 1, 4]
    mixed = gpu_runs(ctx, [SIX[x] for x in order], objective)
    assert mixed == tuple([g[x] for x in order] for g in together)
    # one request at rows 0, 1 and 300 of launches of different company
    case, S, rounds = SIX[0]
    row = tuple(g[0] for g in together)
    for R, at in ((1, 0), (2, 1), (301, 300)):
        cases = [SIX[1 + x % 5][0] for x in range(R)]
        cases[at] = case
        got = gpu_batch(ctx, cases, objective, S, rounds)
        assert tuple(g[at] for g in got) == row, (R, at)
    # R = 0 returns empty tensors
    z = [torch.zeros(shape, dtype=torch.int32, device=ctx.dev)
         for shape in ((0, 24, 11, 11), (0, 11), (0, 3), (0, 3))]
    out = ctx.vrp_batch_ls(*z, obj_id(objective), 8, 5, SEED)
    assert [tuple(t.shape) for t in out] == [(0, 10), (0,), (0, 3), (0, 10), (0, 2)]


@pytest.mark.gpu
def test_gpu_lds_edge(ctx):
    import torch
    lib, K, H, R = ctx.lib, 4, 24, 2
    N = DOMAIN[(H, False)]
    runs = [((N - 1, K, H, 40 + x, ""), 4, 1) for x in range(R)]
    for objective in OBJECTIVES:
        assert gpu_runs(ctx, runs, objective) == expected(runs, objective)
    N += 1
    n = N - 1
    M = torch.ones((R, H, N, N), dtype=torch.int32, device=ctx.dev)
    dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
    cp = torch.ones((R, K), dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R, n), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R, K), -7, dtype=torch.int32, device=ctx.dev)
    veh = torch.full((R, n), -7, dtype=torch.int8, device=ctx.dev)
    info = torch.full((R, 2), -7, dtype=torch.int32, device=ctx.dev)
    rc = lib.vrpms_vrp_batch_ls(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(), cp.data_ptr(),
                                R, N, K, H, 0, 0, 4, 1, SEED, tours.data_ptr(), keys.data_ptr(),
                                durs.data_ptr(), veh.data_ptr(), info.data_ptr(), ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_ls:" in msg and b"bytes of LDS" in msg
    assert str(lds_bytes(N, K, H, False)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item()
    assert (durs == -7).all().item() and (veh == -7).all().item() and (info == -7).all().item()


def _ref_dict(case, objective, S, rounds, base=0):
    """The reference as solve_vrp's slot dict (nodes are matrix rows: with no
    customer left out, the compact indices)."""
    r = reference((case, S, rounds), objective)
    routes = [[] for _ in r["durs"]]
    unv = []
    for c, v in zip(r["tour"], r["veh"]):
        (routes[v] if v >= 0 else unv).append(base + c)
    return {"durationMax": max(r["durs"]), "durationSum": sum(r["durs"]), "unvisited": unv,
            "vehicles": [{"tour": [base] + rt + [base], "duration": d}
                         for rt, d in zip(routes, r["durs"])]}


# solve_vrp_ls_batch reads the seed it is given: the references below use SEED
@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_ls_batch_and_solve_vrp_mixed_list(objective):
    S, rounds = 8, 1000
    D7, locs7, caps7, starts7 = request((6, 2, 24, 50, ""), 100)
    inside = {0: (6, 2, 24, 51, ""), 1: (9, 3, 1, 52, ""), 3: (6, 2, 24, 53, ""), 5: (9, 3, 1, 54, "")}
    reqs = [request(inside[0]), request(inside[1]),
            (D7, locs7, caps7, starts7, [100 + i for i in range(1, 7)]),            # none active
            request(inside[3]),
            {"durations": D7, "locations": locs7, "capacities": caps7, "start_times": starts7,
             "ignored_customers": [103]},
            request(inside[5])]
    kw = dict(starts=S, rounds=rounds, seed=SEED, objective=objective, with_unvisited=True)
    got = solver.solve_vrp_ls_batch(reqs, **kw)
    assert got[2] == {"durationMax": 0, "durationSum": 0, "unvisited": [],
                      "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    for r, res in zip(reqs, got):
        if isinstance(r, dict):
            r = (r["durations"], r["locations"], r["capacities"], r["start_times"],
                 r["ignored_customers"])
        _rescored(r, res, objective)
    # the answers are A25's, through either entry point
    for x, case in inside.items():
        assert got[x] == _ref_dict(case, objective, S, rounds)
        assert solver.solve_vrp("ls", *reqs[x], **kw) == got[x]
    r4 = reqs[4]
    assert solver.solve_vrp("ls", r4["durations"], r4["locations"], r4["capacities"],
                            r4["start_times"], r4["ignored_customers"], **kw) == got[4]
    # deterministic, and the same alone as in company
    assert solver.solve_vrp_ls_batch(reqs, **kw) == got
    for x in (0, 1, 4):
        assert solver.solve_vrp_ls_batch([reqs[x]], **kw) == [got[x]]
    assert "unvisited" not in solver.solve_vrp_ls_batch([reqs[0]], starts=S, seed=SEED)[0]
    assert "unvisited" not in solver.solve_vrp("ls", *reqs[0], starts=S, seed=SEED)


@pytest.mark.gpu
def test_service_batch_vrp_ls_over_http_equals_solve_vrp_ls_batch():
    S, rounds = 8, 1000
    app = service.App(service.MemoryStore({}, {}, {}), seed=SEED, batch_vrp_ls=True,
                      batch_window_s=0.05, batch_ls_starts=S, batch_ls_rounds=rounds)
    srv = service.serve(app, "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    cases = [((6, 2, 24, 60 + x, "") if x % 2 else (9, 3, 1, 52 + x, "")) for x in range(8)]
    try:
        def call(x):
            req = urllib.request.Request(f"http://127.0.0.1:{srv.server_address[1]}/solve/vrp/ls",
                                         data=_body_ls(cases[x]), method="POST")
            with urllib.request.urlopen(req, timeout=120) as resp:
                return resp.status, json.loads(resp.read())

        out = _concurrently(call, len(cases))
    finally:
        srv.shutdown()
        srv.server_close()
        th.join()
    b = app.vrp_ls_batcher
    assert b.requests == 8 and 2 <= b.launches < b.requests
    for x, res in enumerate(out):
        assert not isinstance(res, Exception), res
        assert res[0] == 200 and res[1]["success"], res
        assert [res[1]["message"]] == solver.solve_vrp_ls_batch([request(cases[x], 100)], starts=S,
                                                                rounds=rounds, seed=SEED)
    assert out[0][1]["message"] == {k: v for k, v in _ref_dict(cases[0], "sum", S, rounds).items()
                                    if k != "unvisited"}


def _body_ls(case, base=100, **more):
    D, locs, caps, starts = request(case, base)
    return json.dumps(dict({"durations": D, "locations": locs, "capacities": caps,
                            "startTimes": starts, "ignoredCustomers": [],
                            "completedCustomers": []}, **more)).encode()
