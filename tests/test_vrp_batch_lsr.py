"""Batched VRP multi-start local search over separator tours (spec A26): the C
entry points vrpms_vrp_batch_lsr_lds / vrpms_vrp_batch_lsr,
Context.vrp_batch_lsr, solver.batch_lsr_key / batch_lsr_fits /
solve_vrp_lsr_batch, solve_vrp("lsr") and the service's batcher
(App(batch_vrp_lsr=True)).

The reference is a26_ref below: A25's Philox Fisher-Yates starts packed by
spec.pack_separators, per round spec.apply_move on every (typ, i, j) over the
n + K - 1 tokens priced by spec.eval_cvrp_batch, the least (key, typ, i, j)
applied while it improves, the least (key, start) of the end tours, and
spec.eval_cvrp for the durations and vehicles.  Per request the GPU must return
the identical key, tour, route durations, vehicle row and info row, for both
objectives."""
import ctypes
import functools
import json
import threading
import urllib.request

import numpy as np
import pytest

from oracle import spec
from test_vrp_batch_ga import (_FakeApp, _body, _concurrently, _locs, _no_gpu, _rescored, _sized)
from test_vrp_batch_ls import (LDS_BYTES, M32, OBJECTIVES, SEED, all_moves, obj_id, pad, request,
                               sa_lds_bytes)
from test_vrp_batch_ls import inst as ls_inst
from vrpms_amd import _lib, core, service, solver


# ---------------------------------------------------------------------------
# instances and their references (computed once, shared, never changed)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inst(case):
    """tests/test_vrp_batch_ls.py's inst family, plus the variant "roomy": the
    first vehicle alone carries every customer, so the first fit leaves one
    route of n customers and the K - 1 separators at the end of the tour."""
    n, K, H, seed, variant = case
    if variant != "roomy":
        return ls_inst(case)
    D, dem, caps, starts = ls_inst((n, K, H, seed, ""))
    return D, dem, (int(dem.sum()),) + caps[1:], starts


def a26_ref(D, dem, caps, starts, objective, S, rounds, seed):
    """Spec A26 -> dict(key, tour, durs, veh, s, capped, unvisited, move_tie,
    end_tie, rounds, moves, first): move_tie = some round had its least key on
    two moves that give different tours, end_tie = two starts ended on the same
    key, rounds = the number of applied moves of every descent, moves = the
    applied (typ, i, j) of all of them, first = every start tour."""
    D = spec.as_3d(D)
    n = D.shape[1] - 1
    skey = spec.seed_key(seed)
    caps, starts, obj = list(caps), list(starts), obj_id(objective)
    L = n + len(caps) - 1
    moves = all_moves(L)
    ends, capped, move_tie, applied_all, took, first = [], 0, False, [], [], []
    for s in range(S):
        p = list(range(1, n + 1))
        for q in range(n - 1, 0, -1):
            j = spec.philox4x32_10((M32, M32, s, q), skey)[0] % (q + 1)
            p[q], p[j] = p[j], p[q]
        t = spec.pack_separators(p, len(caps) - 1, dem, caps)
        assert len(t) == L and t.count(0) == len(caps) - 1
        first.append(t)
        k = int(spec.eval_cvrp_batch(D, [t], dem, caps, starts, obj)[0][0])
        applied = 0
        while L >= 2:
            if applied >= rounds:
                capped += 1
                break
            cands = [spec.apply_move(t, *m) for m in moves]
            keys = [int(x) for x in spec.eval_cvrp_batch(D, cands, dem, caps, starts, obj)[0]]
            kmin = min(keys)
            if not kmin < k:
                break
            at = keys.index(kmin)   # the moves are in (typ, i, j) order
            move_tie |= any(kk == kmin and c != cands[at] for kk, c in zip(keys, cands))
            t, k = cands[at], kmin
            took.append(moves[at])
            applied += 1
        ends.append((k, s, t))
        applied_all.append(applied)
    k, s, t = min(ends, key=lambda e: e[:2])
    final = spec.eval_cvrp(D, t, dem, caps, starts, obj)
    assert final["key"] == k
    return dict(key=k, tour=t, durs=final["durations"], veh=final["vehicle_of"], s=s, capped=capped,
                unvisited=final["unvisited"], move_tie=move_tie,
                end_tie=len({e[0] for e in ends}) < len(ends), rounds=applied_all, moves=took,
                first=first)


@functools.lru_cache(maxsize=None)
def reference(run, objective):
    """run = (case, S, rounds)."""
    case, S, rounds = run
    return a26_ref(*inst(case), objective, S, rounds, SEED)


def expected(runs, objective):
    refs = [reference(r, objective) for r in runs]
    return ([r["key"] for r in refs], [r["tour"] for r in refs], [r["durs"] for r in refs],
            [r["veh"] for r in refs], [[r["s"], r["capped"]] for r in refs])


def lds_bytes(N, K, H, wide):
    """DESIGN.md §4.3q restated: the matrix padded to 16 bytes, the demand row
    and the two fleet rows as int32 padded to four words, two uint16 tours of
    n + K - 1 tokens padded to eight per wavefront, and 16 bytes per
    wavefront."""
    return pad(H * N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + \
        4 * 2 * 2 * pad(N - 1 + K - 1, 8) + 4 * 16


def largest_n_nodes(K, H, wide):
    return max(N for N in range(2, 400) if lds_bytes(N, K, H, wide) <= LDS_BYTES)


# DESIGN.md §4.3q's domain table (K = 4): (H, wide) -> the largest N
DOMAIN = {(24, False): 58, (24, True): 41, (1, False): 281, (1, True): 199}

# the runs of the GPU comparisons: (case, S, rounds)
N_EDGES = [((n, 3, 1, n, ""), 6, 1000) for n in (1, 2, 3, 4, 5, 6, 7, 8, 11, 12)] + \
    [((1, 1, 1, 1, ""), 6, 1000)]
# L = n + 3 = 32, 33, 63, 64, 65 tokens
WAVES = [((L - 3, 4, 1, 80 + L, ""), 5, 2 if L < 63 else 1) for L in (32, 33, 63, 64, 65)]
S_EDGES = [((9, 3, 24, 70, ""), S, 1000) for S in (1, 3, 4, 5, 8, 9, 64)]
R_EDGES = [((8, 3, 1, 9, ""), 7, rounds) for rounds in (0, 1, 2, 1000)]
TIES = [((7, 2, 1, 3, "ties"), 12, 1000), ((6, 3, 24, 4, "ties"), 9, 1000)]
VARIANTS = [((6, 3, 24, 10, "hours"), 8, 1000), ((6, 3, 24, 11, "hours"), 8, 1000),
            ((9, 5, 24, 13, "zerocap"), 8, 1000), ((9, 3, 1, 14, "zerodem"), 8, 1000),
            ((6, 3, 24, 73, "below"), 8, 1000), ((3, 64, 1, 12, ""), 4, 1000),
            ((7, 3, 1, 31, "e65536"), 8, 1000)]
# the in-place move works by chunks of 64 positions: on L = 136 tokens, a
# reversal of more than 128 (seeds 336 and 370) and a relocate to more than 64
# positions further on (455, objective max).  A first fit leaves no earlier
# route with room for a customer of a later one, and no such relocate came
# first on 400 seeds of the family, so the fourth case is "roomy": there a
# separator goes 97 positions towards the front under objective max.  The
# seeds were searched on the CPU; test_reference_properties holds them to it
LONG = [((133, 4, 1, seed, ""), 1, 1) for seed in (336, 455, 370)] + [((133, 4, 1, 302, "roomy"), 1, 1)]
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
    f = lib.vrpms_vrp_batch_lsr_lds
    for H in (1, 24):
        for wide in (0, 1):
            for K in (1, 4, 5, 64):
                for N in GRID_N:
                    assert f(N, K, H, wide, ctypes.byref(b)) == _lib.VRPMS_OK
                    assert b.value == lds_bytes(N, K, H, wide) == core.vrp_batch_lsr_lds(N, K, H, wide)
                    assert b.value >= core.vrp_batch_ls_lds(N, K, H, wide)
                    if K == 1:
                        assert b.value == core.vrp_batch_ls_lds(N, K, H, wide)
                    if N > 2:
                        assert b.value >= lds_bytes(N - 1, K, H, wide)
    for args, word in (((1, 3, 1, 0), b"2 <= N"), ((0, 3, 1, 0), b"2 <= N"),
                       ((65536, 3, 1, 0), b"2 <= N"),
                       ((5, 0, 1, 0), b"1 <= K <= 64"), ((5, 65, 1, 0), b"1 <= K <= 64"),
                       ((65535, 3, 1, 0), b"N + K - 2 <= 65535 (65536 given)"),
                       ((65474, 64, 1, 0), b"N + K - 2 <= 65535 (65536 given)"),
                       ((5, 3, 2, 0), b"H must be 1 or 24"), ((5, 3, 0, 0), b"H must be 1 or 24"),
                       ((5, 3, 1, 2), b"wide"), ((5, 3, 1, -1), b"wide")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsr_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    # L = 65535 itself is inside
    assert f(65535, 2, 1, 0, ctypes.byref(b)) == _lib.VRPMS_OK
    assert f(65473, 64, 1, 0, ctypes.byref(b)) == _lib.VRPMS_OK
    assert f(65535, 1, 1, 0, ctypes.byref(b)) == _lib.VRPMS_OK
    assert f(5, 3, 1, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_lsr_lds: bytes is NULL" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= K <= 64"):
        core.vrp_batch_lsr_lds(5, 65, 1, False)
    assert solver.BATCH_LSR_LDS_BYTES == solver.BATCH_SA_LDS_BYTES == LDS_BYTES
    assert solver.BATCH_LSR_MAX_STARTS == solver.BATCH_LS_MAX_STARTS == 1024
    assert solver.BATCH_LSR_MAX_ROUNDS == solver.BATCH_LS_MAX_ROUNDS == 1000


def test_lds_need_is_at_most_the_annealers(lib):
    """A26's domain contains A22's: at every point of the grid, and at A22's
    own edge, the bytes are at most vrpms_vrp_batch_sa_lds's."""
    for H in (1, 24):
        for wide in (0, 1):
            for K in (1, 4, 5, 64):
                for N in GRID_N + [278, 279, 286, 287, 1000]:
                    sa = core.vrp_batch_sa_lds(N, K, H, wide)
                    assert sa == sa_lds_bytes(N, K, H, wide)
                    assert core.vrp_batch_lsr_lds(N, K, H, wide) <= sa, (N, K, H, wide)


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
        return lib.vrpms_vrp_batch_lsr(ctx, a["m"], a["d"], a["cp"], a["st"], R, N, K, H, obj, wide, S,
                                       rounds, 12345, a["t"], a["k"], a["du"], a["v"], a["i"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsr:" in msg and word in msg, (kw, msg)

    refused(b"ctx is NULL", ctx=None)
    refused(b"R must not be negative", R=-1)
    for N in (-1, 0, 1, 65536):
        refused(b"2 <= N", N=N)
    for K in (-1, 0, 65, 1000):
        refused(b"1 <= K <= 64", K=K)
    refused(b"N + K - 2 <= 65535 (65536 given)", N=65535, K=3)
    refused(b"N + K - 2 <= 65535 (65597 given)", N=65535, K=64)
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
    for N, K, H, wide in ((5, 2, 1, 0), (58, 4, 24, 0), (59, 4, 24, 1), (5, 1, 1, 0)):
        refused(b"needs %d bytes of LDS (0 available)" % lds_bytes(N, K, H, wide), N=N, K=K, H=H,
                wide=wide)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, S=65535, rounds=2**31 - 1) == _lib.VRPMS_OK
    assert f(R=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert buf.raw == bytes(4096) and fake.raw == bytes(1 << 16)


def _fake_launch(seen):
    """Customers in descending order on vehicle 0, then the K - 1 separators."""
    def launch(key, cis):
        seen.append((key, len(cis)))
        tours, rest = [], []
        for ci in cis:
            K = len(ci.capacities)
            tours.append(list(range(ci.n, 0, -1)) + [0] * (K - 1))
            rest.append(([0] * ci.n + [-2] * (K - 1), [10 * ci.n] + [0] * (K - 1)))
        return tours, rest
    return launch


def test_batch_lsr_fits_at_the_lds_edge(lib):
    for (H, wide), N in DOMAIN.items():
        assert largest_n_nodes(4, H, wide) == N, (H, wide, largest_n_nodes(4, H, wide))
        assert lds_bytes(N, 4, H, wide) <= LDS_BYTES < lds_bytes(N + 1, 4, H, wide)
        big = 70000 if wide else 0
        assert solver.batch_lsr_fits(_sized(N, 4, H, big), 64, 1000)
        assert not solver.batch_lsr_fits(_sized(N + 1, 4, H, big), 64, 1000)
        assert "bytes" in solver.batch_lsr_message(_sized(N + 1, 4, H, big), 64, 1000)
        assert solver.batch_lsr_key(_sized(N, 4, H, big), 64, 1000) == (N, 4, H, wide, 64, 1000)
        # A22 fits no more: 57 / 278 customers at uint16 cells
        assert N >= max(M for M in range(2, 400) if sa_lds_bytes(M, 4, H, wide) <= LDS_BYTES)
    assert DOMAIN[(24, False)] - 1 >= 57 and DOMAIN[(1, False)] - 1 >= 278
    # the separators count: a fleet of 64 fits fewer nodes than one of 4
    assert largest_n_nodes(64, 1, False) < DOMAIN[(1, False)]
    edge = largest_n_nodes(64, 1, False)
    assert solver.batch_lsr_fits(_sized(edge, 64, 1), 64, 1000)
    assert not solver.batch_lsr_fits(_sized(edge + 1, 64, 1), 64, 1000)
    small = _sized(6, 2, 24)
    assert solver.batch_lsr_fits(small, 1024, 1000) and solver.batch_lsr_fits(small, 1, 0)
    assert not solver.batch_lsr_fits(small, 1025, 10) and not solver.batch_lsr_fits(small, 0, 10)
    assert not solver.batch_lsr_fits(small, 64, 1001) and not solver.batch_lsr_fits(small, 64, -1)
    assert "lsr" in solver.batch_lsr_message(small, 1025, 10)
    assert "starts" in solver.batch_lsr_message(small, 1025, 10)
    assert "rounds" in solver.batch_lsr_message(small, 64, 1001)
    # a wide entry halves the cells that fit; 65535 is still narrow
    N = DOMAIN[(24, False)]
    assert not solver.batch_lsr_fits(_sized(N, 4, 24, 70000), 64, 1000)
    assert solver.batch_lsr_fits(_sized(N, 4, 24, 65534), 64, 1000)
    # outside the domain whatever the size
    assert "vehicles" in solver.batch_lsr_message(_sized(5, 65, 1), 8, 4)
    none = solver.compact_vrp(np.ones((3, 3), dtype=np.int64), _locs([0, 1, 1]), [3], [0], [1, 2])
    assert none.n == 0 and not solver.batch_lsr_fits(none, 8, 4)
    tsp = solver.compact_tsp(np.ones((4, 4), dtype=np.int64), [1, 2, 3], 0, 0)
    assert not solver.batch_lsr_fits(tsp, 8, 4)
    b = service.VrpLsrBatcher(_FakeApp(), launch=_fake_launch([]))
    assert (b.starts, b.rounds) == (64, 1000)
    assert b.accepts(small) and not b.accepts(_sized(6, 2, 1, 2**29))               # the A9 guard
    assert not b.accepts(_sized(5, 65, 1))
    for kw in (dict(starts=0), dict(starts=1025), dict(rounds=-1), dict(rounds=1001)):
        with pytest.raises(ValueError, match="starts|rounds"):
            service.VrpLsrBatcher(_FakeApp(), launch=_fake_launch([]), **kw)


def test_solve_vrp_lsr_batch_refusals_need_no_gpu(monkeypatch, lib):
    _no_gpu(monkeypatch)
    good = request((6, 2, 1, 0, ""))
    assert solver.solve_vrp_lsr_batch([]) == []
    with pytest.raises(ValueError, match=r"^request 1: capacities and startTimes"):
        solver.solve_vrp_lsr_batch([good, (good[0], good[1], [3, 3], [0])])
    with pytest.raises(ValueError, match=r"^request 2: 5 locations but a 7-node"):
        solver.solve_vrp_lsr_batch([good, good, {"durations": good[0], "locations": good[1][:5],
                                                 "capacities": [3], "start_times": [0]}])
    big = np.full((7, 7), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_vrp_lsr_batch([good, (big.tolist(), good[1], [3, 3], [0, 0])])
    heavy = [{"id": i, "demand": 2**30} for i in range(7)]
    with pytest.raises(ValueError, match=r"^request 0: capacity \+ demand overflows int32"):
        solver.solve_vrp_lsr_batch([(good[0], heavy, [2**30, 3], [0, 0])])
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp_lsr_batch([good], objective="mean")
    for starts in (0, -1, 1025):
        with pytest.raises(ValueError, match=r"starts must be in 1\.\.1024"):
            solver.solve_vrp_lsr_batch([good], starts=starts)
    for rounds in (-1, 1001):
        with pytest.raises(ValueError, match=r"rounds must be in 0\.\.1000"):
            solver.solve_vrp_lsr_batch([good], rounds=rounds)
    # outside the domain there is no other path: the limit that failed, by request
    with pytest.raises(ValueError, match=r"^request 1: lsr \(local search\) supports 1\.\.64 vehicles "
                                         r"\(65 given\)"):
        solver.solve_vrp_lsr_batch([good, (good[0], good[1], [1] * 65, [0] * 65)])
    Nbig = DOMAIN[(1, False)] + 1
    bigD = np.ones((Nbig, Nbig), dtype=np.int64).tolist()
    need = lds_bytes(Nbig, 4, 1, False)
    with pytest.raises(ValueError, match=rf"^request 0: lsr .* need {need} bytes; the limit is "
                                         rf"{LDS_BYTES} bytes"):
        solver.solve_vrp_lsr_batch([(bigD, _locs([0] + [1] * (Nbig - 1)), [Nbig] * 4, [0] * 4)])
    # no customer: solve_vrp's trivial answer, built on the host
    none = (good[0], good[1], [3, 3], [0, 7], [1, 2, 3, 4, 5, 6])
    trivial = {"durationMax": 0, "durationSum": 0, "unvisited": [],
               "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    assert solver.solve_vrp_lsr_batch([none], with_unvisited=True) == [trivial]
    assert solver.solve_vrp("lsr", *none, with_unvisited=True) == trivial


def test_solve_vrp_lsr_and_solve_tsp_lsr_errors(monkeypatch, lib):
    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: pytest.fail("the remote was touched"))
    assert "lsr" in solver.ALGORITHMS and "ls" in solver.ALGORITHMS
    D, locs, caps, starts = request((6, 2, 1, 0, ""))
    with pytest.raises(ValueError, match="lsr solves the VRP only"):
        solver.solve_tsp("lsr", D, [1, 2, 3], 0, 0)
    with pytest.raises(ValueError, match=r"lsr .* 1\.\.64 vehicles \(65 given\)"):
        solver.solve_vrp("lsr", D, locs, [1] * 65, [0] * 65)
    with pytest.raises(ValueError, match=r"1\.\.1024 starts \(1025 given\)"):
        solver.solve_vrp("lsr", D, locs, caps, starts, starts=1025)
    with pytest.raises(ValueError, match=r"1\.\.1024 starts \(0 given\)"):
        solver.solve_vrp("lsr", D, locs, caps, starts, starts=0)
    with pytest.raises(ValueError, match=r"0\.\.1000 rounds \(1001 given\)"):
        solver.solve_vrp("lsr", D, locs, caps, starts, rounds=1001)
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp("lsr", D, locs, caps, starts, objective="mean")
    big = np.full((7, 7), 2**29, dtype=np.int64).tolist()
    with pytest.raises(ValueError, match="A9 guard"):
        solver.solve_vrp("lsr", big, locs, caps, starts)
    Nbig = DOMAIN[(24, False)] + 1
    bigD = np.ones((24, Nbig, Nbig), dtype=np.int64).tolist()
    with pytest.raises(ValueError, match=r"need \d+ bytes; the limit is 163840 bytes"):
        solver.solve_vrp("lsr", bigD, _locs([0] + [1] * (Nbig - 1)), [Nbig] * 4, [0] * 4)


def test_app_batch_vrp_lsr_routes(monkeypatch, lib):
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, len(params["capacities"]), dict(knobs.get("inline") or {})))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    assert "lsr" in service.INLINE_ALGORITHMS["vrp"] and "lsr" not in service.INLINE_ALGORITHMS["tsp"]
    assert service.INLINE_ALGORITHMS["vrp"][-1] == "sp" and "lsr" not in service.TITLES
    # the flag is off: the injected solve
    off = service.App(service.MemoryStore({}, {}, {}), solve=fake)
    assert off.vrp_lsr_batcher is None
    assert off.solve_inline("vrp", "lsr", _body((5, 2, 1, 0, "")))[1]["message"]["durationSum"] == 3
    assert seen == [("vrp", "lsr", 2, {})]
    del seen[:]
    st, res = off.solve_inline("tsp", "lsr", b"{}")
    assert st == 400 and "no solver /solve/tsp/lsr" in res["errors"][0]["reason"]

    app = service.App(service.MemoryStore({}, {}, {}), solve=fake, batch_vrp_lsr=True,
                      batch_window_s=0.2, batch_vrp_lsr_launch=_fake_launch(launched),
                      batch_lsr_starts=16, batch_lsr_rounds=7)
    assert isinstance(app.vrp_lsr_batcher, service.VrpLsrBatcher)
    assert isinstance(app.vrp_lsr_batcher, service.VrpLsBatcher)
    assert (app.vrp_lsr_batcher.starts, app.vrp_lsr_batcher.rounds) == (16, 7)
    assert app.vrp_sa_batcher is None and app.vrp_ga_batcher is None and \
        app.vrp_aco_batcher is None and app.vrp_ls_batcher is None

    def call(x):
        if x < 4:
            return app.solve_inline("vrp", "lsr", _body((5, 2, 1, x, ""), seed=x, timeLimit=1.0))
        if x < 6:
            return app.solve_inline("vrp", "lsr", _body((5, 2, 1, x, ""), objective="max"))
        return app.solve_inline("vrp", "lsr", _body((6, 3, 24, x, "")))

    out = _concurrently(call, 8)
    assert all(st == 200 for st, _ in out), out
    assert sorted(launched) == [((6, 2, 1, False, "max"), 2), ((6, 2, 1, False, "sum"), 4),
                                ((7, 3, 24, False, "sum"), 2)]
    assert seen == [] and app.vrp_lsr_batcher.requests == 8
    # the separators of the launch's rows do not reach the answer
    assert out[0][1]["message"]["vehicles"][0]["tour"] == [0, 5, 4, 3, 2, 1, 0]
    assert out[0][1]["message"]["vehicles"][1]["tour"] == [0, 0]

    # every rule that sends a request down the unbatched path, one by one
    def unbatched(status_and_result, K=2, algorithm="lsr", inline=None):
        assert status_and_result[0] == 200, status_and_result
        assert seen == [("vrp", algorithm, K, inline or {})]
        del seen[:]

    body = functools.partial(_body, (5, 2, 1, 1, ""))
    unbatched(app.solve_inline("vrp", "lsr", body(knobs={"starts": 8})), inline={"starts": 8})
    unbatched(app.solve_inline("vrp", "lsr", body(knobs={"rounds": 0})), inline={"rounds": 0})
    D, locs, caps, starts = request((5, 2, 1, 1, ""), 100)
    wide_fleet = json.dumps({"durations": D, "locations": locs, "capacities": [1] * 65,
                             "startTimes": [0] * 65, "ignoredCustomers": [],
                             "completedCustomers": []}).encode()
    unbatched(app.solve_inline("vrp", "lsr", wide_fleet), K=65)                        # the domain
    unbatched(app.solve_inline("vrp", "ls", body()), algorithm="ls")                   # another algorithm
    unbatched(app.solve_inline("vrp", "sa", body()), algorithm="sa")
    assert len(launched) == 3
    for knobs in ({"starts": 0}, {"starts": 1025}, {"rounds": -1}, {"rounds": 1001}):
        st, res = app.solve_inline("vrp", "lsr", body(knobs=knobs))
        assert st == 400 and "outside" in res["errors"][0]["reason"], res
    # the A25 batcher does not take A26's requests, nor the other way round
    both = service.App(service.MemoryStore({}, {}, {}), solve=fake, batch_vrp_ls=True,
                       batch_window_s=0.05, batch_vrp_ls_launch=lambda key, cis: pytest.fail("ls"),
                       batch_vrp_lsr=True, batch_vrp_lsr_launch=_fake_launch(launched))
    assert both.solve_inline("vrp", "lsr", body())[0] == 200
    assert len(launched) == 4 and seen == []
    # a bad instance is a 400 in solve_vrp's words; so is one outside the domain
    # on the real unbatched path, before any device is touched
    _no_gpu(monkeypatch)
    real = service.App(service.MemoryStore({}, {}, {}), batch_vrp_lsr=True, batch_window_s=0.2,
                       batch_vrp_lsr_launch=_fake_launch(launched))
    st, res = real.solve_inline("vrp", "lsr", body(startTimes=[0]))
    assert st == 400 and "capacities and startTimes" in res["errors"][0]["reason"]
    st, res = real.solve_inline("vrp", "lsr", wide_fleet)
    assert st == 400 and "1..64 vehicles (65 given)" in res["errors"][0]["reason"]
    assert len(launched) == 4


def test_cli_flags(monkeypatch, capsys):
    made = {}

    class Stop(Exception):
        pass

    def app(store, **kw):
        made.update(kw)
        raise Stop

    monkeypatch.setattr(service, "App", app)
    for argv, want in ((["--batch-vrp-lsr"], (True, 64, 1000)), ([], (False, 64, 1000)),
                       (["--batch-vrp-lsr", "--batch-lsr-starts", "1024", "--batch-lsr-rounds", "0"],
                        (True, 1024, 0))):
        with pytest.raises(Stop):
            service.main(argv)
        assert (made["batch_vrp_lsr"], made["batch_lsr_starts"], made["batch_lsr_rounds"]) == want
        assert made["batch_vrp_ls"] is False and (made["batch_ls_starts"], made["batch_ls_rounds"]) == \
            (64, 1000)
    for argv in (["--batch-lsr-starts", "0"], ["--batch-lsr-starts", "1025"],
                 ["--batch-lsr-rounds", "-1"], ["--batch-lsr-rounds", "1001"]):
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
    # every tour has its K - 1 separators, from the start to the end
    for (run, o), r in refs.items():
        n, K = run[0][:2]
        assert len(r["tour"]) == n + K - 1 and r["tour"].count(0) == K - 1
        assert sorted(r["tour"])[K - 1:] == list(range(1, n + 1))
        assert [v == -2 for v in r["veh"]] == [c == 0 for c in r["tour"]]
        assert all(len(t) == n + K - 1 and t.count(0) == K - 1 for t in r["first"])
    # the token ranges 32, 33, 63, 64, 65 of the lane edges
    assert [run[0][0] + run[0][1] - 1 for run in WAVES] == [32, 33, 63, 64, 65]
    # with the round cap out of reach no descent is capped and the answer
    # admits no improving move
    for run in N_EDGES + S_EDGES + TIES + VARIANTS + R_EDGES[-1:]:
        for o in OBJECTIVES:
            r = refs[(run, o)]
            assert r["capped"] == 0 and max(r["rounds"]) < run[2]
            if len(r["tour"]) >= 2:
                assert not _improving(run[0], r["tour"], r["key"], o), (run, o)
    # separators are moved: some applied move has a separator at i or j, and
    # some end tour has its separators elsewhere than every start put them
    assert any([i for i, c in enumerate(r["tour"]) if c == 0] not in
               [[i for i, c in enumerate(t) if c == 0] for t in r["first"]] for r in refs.values())
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
    # n = 1: K = 1 has no moves, not capped even at rounds = 0, the start is the
    # answer; K = 3 only chooses the vehicle
    one = a26_ref(*inst((1, 1, 1, 1, "")), "sum", 5, 0, SEED)
    assert (one["tour"], one["s"], one["capped"], one["rounds"]) == ([1], 0, 0, [0] * 5)
    r = refs[(N_EDGES[0], "sum")]
    assert sorted(r["tour"]) == [0, 0, 1] and len({tuple(t) for t in r["first"]}) == 1
    # "below": every key equal, no move applied, start 0 the answer
    r = refs[(VARIANTS[4], "max")]
    assert r["unvisited"] == 6 and r["s"] == 0 and r["rounds"] == [0] * 8 and r["end_tie"]
    assert any(0 < r["unvisited"] < len(r["tour"]) - r["tour"].count(0) for r in refs.values())
    # a winner from every wavefront, and one beyond the first sweep of four
    assert {r["s"] % 4 for r in refs.values()} == {0, 1, 2, 3}
    assert any(r["s"] >= 4 for r in refs.values())
    # the first fit puts a customer on the last route when none has room
    assert any(t != spec.pack_separators([c for c in t if c], run[0][1] - 1, inst(run[0])[1],
                                         [10**9] * run[0][1])
               for (run, o), r in refs.items() for t in r["first"])
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
def _dev(ctx, rows):
    import torch
    return torch.tensor(np.stack([np.asarray(r) for r in rows]), dtype=torch.int32, device=ctx.dev)


def gpu_args(ctx, cases):
    insts = [inst(c) for c in cases]
    return (_dev(ctx, [D for D, _, _, _ in insts]), _dev(ctx, [d for _, d, _, _ in insts]),
            _dev(ctx, [c for _, _, c, _ in insts]), _dev(ctx, [s for _, _, _, s in insts]))


def gpu_batch(ctx, cases, objective, S, rounds, wide=None):
    """One vrp_batch_lsr launch -> ([key], [tour], [durs], [veh], [info])."""
    tours, keys, durs, veh, info = ctx.vrp_batch_lsr(*gpu_args(ctx, cases), obj_id(objective), S,
                                                     rounds, SEED, wide=wide)
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
        assert keys[1] == 2**64 - 1 and tours[1] == [0] * 9 and durs[1] == [0] * 3 and \
            veh[1] == [-1] * 9 and info[1] == [-1, 0]
        for x in (0, 2):
            assert (keys[x], tours[x], durs[x], veh[x], info[x]) == tuple(w[x] for w in want)
        # a negative entry, under either width
        insts = [inst(x) for x in (a, b, c)]
        mats = np.stack([D for D, _, _, _ in insts]).astype(np.int32)
        mats[1, H - 1, 3, 2] = -1
        args = gpu_args(ctx, (a, b, c))
        for wide in (False, True):
            tours, keys, durs, veh, info = ctx.vrp_batch_lsr(
                torch.tensor(mats, dtype=torch.int32, device=ctx.dev), *args[1:],
                obj_id(objective), S, rounds, SEED, wide=wide)
            want = expected(runs(a, b, c), objective)
            assert keys[1].item() == -1 and tours[1].tolist() == [0] * 9 and \
                durs[1].tolist() == [0] * 3 and veh[1].tolist() == [-1] * 9 and \
                info[1].tolist() == [-1, 0]
            for x in (0, 2):
                assert (int(keys[x].item()) & (2**64 - 1), tours[x].tolist(), durs[x].tolist(),
                        veh[x].tolist(), info[x].tolist()) == tuple(w[x] for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_one_vehicle_is_vrp_batch_ls(ctx, objective):
    """No oracle involved: with K = 1 there is no separator, and the tours,
    keys, durations and info are A25's for the same S, rounds and seed."""
    import torch
    for case, S, rounds in (((9, 1, 24, 70, ""), 9, 1000), ((12, 1, 1, 12, ""), 64, 1000),
                            ((65, 1, 1, 145, ""), 5, 2), ((1, 1, 1, 1, ""), 5, 0),
                            ((8, 1, 1, 3, "ties"), 12, 1000), ((8, 1, 1, 9, ""), 7, 1)):
        args = gpu_args(ctx, [case]) + (obj_id(objective), S, rounds, SEED)
        ls = ctx.vrp_batch_ls(*args)
        lsr = ctx.vrp_batch_lsr(*args)
        for x in (0, 1, 2, 4):
            assert torch.equal(ls[x], lsr[x]), (case, S, rounds, x)
        assert torch.equal(ls[3], lsr[3])   # no separator: the vehicles too


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_four_starts_no_round_is_the_annealers_start(ctx, objective):
    """No oracle involved: S = 4 and rounds = 0 leave the four first-fit
    starts, which are vrp_batch_sa's four chains' at steps = 0."""
    import torch
    for case in ((9, 3, 24, 70, ""), (12, 3, 1, 12, ""), (62, 4, 1, 145, ""), (1, 3, 1, 1, ""),
                 (9, 5, 24, 13, "zerocap"), (3, 64, 1, 12, ""), (133, 4, 1, 5, "")):
        args = gpu_args(ctx, [case])
        inv_t0 = torch.ones(1, dtype=torch.float32, device=ctx.dev)
        sa = ctx.vrp_batch_sa(*args, inv_t0, obj_id(objective), 0, 1.0, SEED)
        lsr = ctx.vrp_batch_lsr(*args, obj_id(objective), 4, 0, SEED)
        for a, b in zip(sa, lsr[:4]):
            assert torch.equal(a, b), case
        L = case[0] + case[1] - 1
        assert lsr[4][0, 1].item() == (4 if L >= 2 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_batch_independence(ctx, objective):
    import torch
    want = expected(SIX, objective)
    together = gpu_runs(ctx, SIX, objective)
    assert together == want
    assert gpu_runs(ctx, SIX, objective) == together                  # two launches are identical
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
    out = ctx.vrp_batch_lsr(*z, obj_id(objective), 8, 5, SEED)
    assert [tuple(t.shape) for t in out] == [(0, 12), (0,), (0, 3), (0, 12), (0, 2)]


@pytest.mark.gpu
def test_gpu_lds_edge(ctx):
    import torch
    lib, K, H, R = ctx.lib, 4, 24, 2
    N = DOMAIN[(H, False)]
    runs = [((N - 1, K, H, 40 + x, ""), 4, 1) for x in range(R)]
    for objective in OBJECTIVES:
        assert gpu_runs(ctx, runs, objective) == expected(runs, objective)
    N += 1
    L = N - 1 + K - 1
    M = torch.ones((R, H, N, N), dtype=torch.int32, device=ctx.dev)
    dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
    cp = torch.ones((R, K), dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R, L), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R, K), -7, dtype=torch.int32, device=ctx.dev)
    veh = torch.full((R, L), -7, dtype=torch.int8, device=ctx.dev)
    info = torch.full((R, 2), -7, dtype=torch.int32, device=ctx.dev)
    rc = lib.vrpms_vrp_batch_lsr(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(), cp.data_ptr(),
                                 R, N, K, H, 0, 0, 4, 1, SEED, tours.data_ptr(), keys.data_ptr(),
                                 durs.data_ptr(), veh.data_ptr(), info.data_ptr(), ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_lsr:" in msg and b"bytes of LDS" in msg
    assert str(lds_bytes(N, K, H, False)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item()
    assert (durs == -7).all().item() and (veh == -7).all().item() and (info == -7).all().item()


def _static_requests(count, n, K):
    return [request((n, K, 1, 500 + x, "")) for x in range(count)]


def _score(res):
    return (len(res["unvisited"]), res["durationSum"])


@pytest.mark.gpu
def test_never_below_the_exact_solver():
    """A condition, not a quality bar: on 200 static requests of (8, 3) no
    answer beats the optimum's (unvisited, durationSum), and every answer's
    durations are what spec.eval_cvrp gives its routes."""
    reqs = _static_requests(200, 8, 3)
    exact = solver.solve_vrp_batch("sp", reqs, with_unvisited=True)
    got = solver.solve_vrp_lsr_batch(reqs, starts=16, rounds=1000, seed=SEED, with_unvisited=True)
    hits = 0
    for r, e, g in zip(reqs, exact, got):
        _rescored(r, g, "sum")
        assert _score(g) >= _score(e), (g, e)
        hits += _score(g) == _score(e)
    print("at the optimum:", hits, "of", len(reqs))


def _ref_dict(case, objective, S, rounds, base=0):
    """The reference as solve_vrp's slot dict (nodes are matrix rows: with no
    customer left out, the compact indices)."""
    r = reference((case, S, rounds), objective)
    routes = [[] for _ in r["durs"]]
    unv = []
    for c, v in zip(r["tour"], r["veh"]):
        if v != -2:
            (routes[v] if v >= 0 else unv).append(base + c)
    return {"durationMax": max(r["durs"]), "durationSum": sum(r["durs"]), "unvisited": unv,
            "vehicles": [{"tour": [base] + rt + [base], "duration": d}
                         for rt, d in zip(routes, r["durs"])]}


# solve_vrp_lsr_batch reads the seed it is given: the references below use SEED
@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_lsr_batch_and_solve_vrp_mixed_list(objective):
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
    got = solver.solve_vrp_lsr_batch(reqs, **kw)
    assert got[2] == {"durationMax": 0, "durationSum": 0, "unvisited": [],
                      "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    for r, res in zip(reqs, got):
        if isinstance(r, dict):
            r = (r["durations"], r["locations"], r["capacities"], r["start_times"],
                 r["ignored_customers"])
        _rescored(r, res, objective)
    # the answers are A26's, through either entry point
    for x, case in inside.items():
        assert got[x] == _ref_dict(case, objective, S, rounds)
        assert solver.solve_vrp("lsr", *reqs[x], **kw) == got[x]
    r4 = reqs[4]
    assert solver.solve_vrp("lsr", r4["durations"], r4["locations"], r4["capacities"],
                            r4["start_times"], r4["ignored_customers"], **kw) == got[4]
    # deterministic, and the same alone as in company
    assert solver.solve_vrp_lsr_batch(reqs, **kw) == got
    for x in (0, 1, 4):
        assert solver.solve_vrp_lsr_batch([reqs[x]], **kw) == [got[x]]
    assert "unvisited" not in solver.solve_vrp_lsr_batch([reqs[0]], starts=S, seed=SEED)[0]
    assert "unvisited" not in solver.solve_vrp("lsr", *reqs[0], starts=S, seed=SEED)


@pytest.mark.gpu
def test_service_batch_vrp_lsr_over_http_equals_solve_vrp_lsr_batch():
    S, rounds = 8, 1000
    app = service.App(service.MemoryStore({}, {}, {}), seed=SEED, batch_vrp_lsr=True,
                      batch_window_s=0.05, batch_lsr_starts=S, batch_lsr_rounds=rounds)
    srv = service.serve(app, "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    cases = [((6, 2, 24, 60 + x, "") if x % 2 else (9, 3, 1, 52 + x, "")) for x in range(8)]
    try:
        def call(x):
            req = urllib.request.Request(f"http://127.0.0.1:{srv.server_address[1]}/solve/vrp/lsr",
                                         data=_body(cases[x]), method="POST")
            with urllib.request.urlopen(req, timeout=120) as resp:
                return resp.status, json.loads(resp.read())

        out = _concurrently(call, len(cases))
        # an inline knob takes the unbatched route: solve_vrp("lsr") at that knob
        req = urllib.request.Request(f"http://127.0.0.1:{srv.server_address[1]}/solve/vrp/lsr",
                                     data=_body(cases[0], knobs={"starts": 3}, seed=SEED),
                                     method="POST")
        with urllib.request.urlopen(req, timeout=120) as resp:
            inline = json.loads(resp.read())
    finally:
        srv.shutdown()
        srv.server_close()
        th.join()
    b = app.vrp_lsr_batcher
    assert b.requests == 8 and 2 <= b.launches < b.requests
    for x, res in enumerate(out):
        assert not isinstance(res, Exception), res
        assert res[0] == 200 and res[1]["success"], res
        assert [res[1]["message"]] == solver.solve_vrp_lsr_batch([request(cases[x], 100)], starts=S,
                                                                 rounds=rounds, seed=SEED)
    want = _ref_dict(cases[0], "sum", S, rounds)
    assert out[0][1]["message"] == {k: v for k, v in want.items() if k != "unvisited"}
    assert [inline["message"]] == solver.solve_vrp_lsr_batch([request(cases[0], 100)], starts=3,
                                                             rounds=1000, seed=SEED)
