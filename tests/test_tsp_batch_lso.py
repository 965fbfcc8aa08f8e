"""Batched TSP multi-start local search with Or-opt and delta pricing (spec
A27): the C entry points vrpms_tsp_batch_lso_lds / vrpms_tsp_batch_lso,
Context.tsp_batch_lso, solver.batch_lso_key / batch_lso_fits /
solve_tsp_lso_batch, solve_tsp("lso") and the inline route /solve/tsp/lso.

The reference is a27_ref below: A25's Philox Fisher-Yates starts, per round
every enabled (typ, i, j) -- spec.apply_move for the types 0..2, the list
formula rest[:j] + seg + rest[j:] for the Or-opt types 3 and 4 -- priced by a
full spec.eval_tsp_batch walk (no delta on this side), the least (key, typ, i,
j) applied while it improves, the least (key, start) of the end tours.  Per
request the GPU must return the identical key, tour, duration and info row."""
import ctypes
import functools
import json
import os
import threading
import urllib.request

import numpy as np
import pytest

from oracle import spec
from test_vrp_batch_ga import _no_gpu
from test_vrp_batch_ga import inst as ga_inst
from test_vrp_batch_ls import a25_ref
from vrpms_amd import _lib, core, service, solver

LDS_BYTES = 160 * 1024
SEED = 20251
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# instances and their references (computed once, shared, never changed)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inst(case):
    """case = (n, H, seed, variant) -> (D int64 [H][N][N], start time): the
    matrix and vehicle 0's start time of tests/test_vrp_batch_ga.py's inst at
    K = 1 (entries 1..89, asymmetric and non-metric, 0 on the diagonal; start
    time in 0..1439; its variants "hours", "e65535" and "e65536"), plus
      "ties"   entries 1..2, so distinct moves give equal keys
      "huge"   entries in [2^26, 2^27): every duration is above the key's
               2^28 - 1 clamp
      "t<m>"   the plain instance started at minute m"""
    n, H, seed, variant = case
    base = variant if variant in ("hours", "e65535", "e65536") else ""
    D, _, _, starts = ga_inst((n, 1, H, seed, base))
    t0 = int(starts[0])
    if variant == "ties":
        D = np.random.default_rng(9100 + seed).integers(1, 3, size=D.shape, dtype=np.int64)
    elif variant == "huge":
        D = np.random.default_rng(9200 + seed).integers(2**26, 2**27, size=D.shape, dtype=np.int64)
    elif variant.startswith("t"):
        t0 = int(variant[1:])
    else:
        assert variant == base, variant
    if variant in ("ties", "huge"):
        for h in range(H):
            np.fill_diagonal(D[h], 0)
        D.setflags(write=False)
    return D, t0


def oropt(p, m, i, j):
    """The issue's list formula: the m customers from position i on, put back
    at position j of the rest."""
    seg, rest = p[i:i + m], p[:i] + p[i + m:]
    return rest[:j] + seg + rest[j:]


@functools.lru_cache(maxsize=None)
def all_moves(n, moves=31):
    """Every enabled (typ, i, j) of a round in the order ties break by."""
    tri = [(i, j) for i in range(n) for j in range(i + 1, n)]
    out = []
    for typ in range(5):
        if not (moves >> typ) & 1:
            continue
        if typ < 2:
            out += [(typ, i, j) for i, j in tri]
        else:
            m = typ - 1
            out += [(typ, i, j) for i in range(n - m + 1) for j in range(n - m + 1) if i != j]
    return out


def moved(p, typ, i, j):
    return spec.apply_move(p, typ, i, j) if typ <= 2 else oropt(list(p), typ - 1, i, j)


@functools.lru_cache(maxsize=None)
def move_sources(n, moves=31):
    """Row x: the positions move x reads, i.e. the move applied to 0..n-1, so
    that a round's candidates are one numpy gather of the tour."""
    ident = list(range(n))
    rows = [moved(ident, *mv) for mv in all_moves(n, moves)]
    return np.array(rows, dtype=np.int16).reshape(len(rows), n)


def shuffled(n, s, seed):
    skey = spec.seed_key(seed)
    t = list(range(1, n + 1))
    for q in range(n - 1, 0, -1):
        j = spec.philox4x32_10((M32, M32, s, q), skey)[0] % (q + 1)
        t[q], t[j] = t[j], t[q]
    return t


def a27_ref(D, t0, S, rounds, moves, seed):
    """Spec A27 -> dict(key, tour, dur, s, capped, move_tie, end_tie, rounds,
    moves): move_tie = some round had its least key on two moves that give
    different tours, end_tie = two starts ended on the same key, rounds = the
    number of applied moves of every descent, moves = the applied (typ, i, j)
    of all of them.  Every candidate is a full walk."""
    D = spec.as_3d(D)
    n = D.shape[1] - 1
    mvs = all_moves(n, moves)
    src = move_sources(n, moves)
    ends, capped, move_tie, applied_all, took = [], 0, False, [], []
    for s in range(S):
        t = shuffled(n, s, seed)
        d = int(spec.eval_tsp_batch(D, [t], t0)[0])
        assert d == spec.eval_tsp(D, t, t0)
        k = spec.tsp_key(d)
        applied = 0
        while n >= 2:
            if applied >= rounds:
                capped += 1
                break
            if not mvs:
                break
            cands = np.asarray(t, dtype=np.int64)[src]
            durs = spec.eval_tsp_batch(D, cands, t0)
            keys = [spec.tsp_key(int(x)) for x in durs]
            kmin = min(keys)
            if not kmin < k:
                break
            first = keys.index(kmin)   # the moves are in (typ, i, j) order
            best = cands[first].tolist()
            assert best == moved(t, *mvs[first])
            move_tie |= any(kk == kmin and c.tolist() != best for kk, c in zip(keys, cands)
                            if kk == kmin)
            t, k, d = best, kmin, int(durs[first])
            took.append(mvs[first])
            applied += 1
        ends.append((k, s, t, d))
        applied_all.append(applied)
    k, s, t, d = min(ends, key=lambda e: e[:2])
    assert d == spec.eval_tsp(D, t, t0) and k == spec.tsp_key(d)
    return dict(key=k, tour=t, dur=d, s=s, capped=capped, move_tie=move_tie,
                end_tie=len({e[0] for e in ends}) < len(ends), rounds=applied_all, moves=took)


@functools.lru_cache(maxsize=None)
def reference(run):
    """run = (case, S, rounds, moves)."""
    case, S, rounds, moves = run
    return a27_ref(*inst(case), S, rounds, moves, SEED)


def expected(runs):
    refs = [reference(r) for r in runs]
    return ([r["key"] for r in refs], [r["tour"] for r in refs], [r["dur"] for r in refs],
            [[r["s"], r["capped"]] for r in refs])


def pad(x, m):
    return (x + m - 1) // m * m


def lds_bytes(N, H, wide):
    """DESIGN.md §4.3s restated: the matrix padded to 16 bytes; per wavefront
    two int32 rows of n + 2 words padded to four (one on an hour-indexed
    matrix), a uint16 tour of n + 2 genes and one of n, each padded to eight;
    and 16 bytes per wavefront."""
    n = N - 1
    return pad(H * N * N * (4 if wide else 2), 16) + \
        4 * ((2 if H == 1 else 1) * 4 * pad(n + 2, 4) + 2 * pad(n + 2, 8) + 2 * pad(n, 8)) + 4 * 16


def largest_n_nodes(H, wide):
    return max(N for N in range(2, 400) if lds_bytes(N, H, wide) <= LDS_BYTES)


# DESIGN.md §4.3s's domain table: (H, wide) -> the largest N
DOMAIN = {(1, False): 274, (1, True): 196, (24, False): 58, (24, True): 41}

# the runs of the GPU comparisons: (case, S, rounds, moves)
N_EDGES = [((n, 1, n, ""), 6, 1000, 31) for n in (1, 2, 3, 4, 5, 6, 8, 11, 12)]
WAVES = [((n, 1, 80 + n, ""), 5, 2 if n < 64 else 1, 31) for n in (31, 32, 33, 64, 65)]
S_EDGES = [((9, 24, 70, ""), S, 1000, 31) for S in (1, 3, 4, 5, 8, 9, 64)]
R_EDGES = [((8, 1, 9, ""), 7, rounds, 31) for rounds in (0, 1, 2, 1000)]
MASKS = [((7, 1, 21, ""), 4, 1000, mask) for mask in range(1, 32)] + \
    [((6, 24, 22, ""), 4, 1000, mask) for mask in range(1, 32)]
TIES = [((7, 1, 3, "ties"), 12, 1000, 31), ((6, 24, 4, "ties"), 9, 1000, 31)]
HOURS = [((6, 24, 10, "hours"), 8, 1000, 31), ((6, 24, 11, "hours"), 8, 1000, 31)]
CLOCK = [((7, 24, 40, "t%d" % t), 6, 1000, 31) for t in (0, 59, 61, 1439)]
HUGE = [((7, 1, 50, "huge"), 6, 1000, 31), ((6, 24, 51, "huge"), 6, 1000, 31)]
E65535 = [((7, H, 31, "e65535"), 6, 1000, 31) for H in (1, 24)]
E65536 = [((7, H, 31, "e65536"), 6, 1000, 31) for H in (1, 24)]
# the in-place move works by chunks of 64 positions.  The first move of one
# descent at n = 135: with only the Or-opt types enabled (mask 24) a segment
# moved over more than 64 positions up and one down the tour; with every type
# enabled a reversal of more than 128 positions.  The instance seeds were
# searched with a27_ref; test_reference_properties holds them to that
LONG = [((135, 1, 314, ""), 1, 1, 24), ((135, 1, 304, ""), 1, 1, 24), ((135, 1, 389, ""), 1, 1, 31)]
ALL_RUNS = N_EDGES + WAVES + S_EDGES + R_EDGES + MASKS + TIES + HOURS + CLOCK + HUGE + E65535 + \
    E65536 + LONG
SIX = [((10, 24, 20 + x, ""), 16, 1000, 31) for x in range(6)]


def run_id(r):
    return "n%d-H%d-s%d%s-S%d-r%d-m%d" % (*r[0], *r[1:])


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


GRID_N = list(range(2, 70)) + [96, 97, 128, 129] + list(range(280, 291))


def test_lds_bytes_formula_monotone_and_refusals(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_tsp_batch_lso_lds
    for H in (1, 24):
        for wide in (0, 1):
            for N in GRID_N:
                assert f(N, H, wide, ctypes.byref(b)) == _lib.VRPMS_OK
                assert b.value == lds_bytes(N, H, wide) == core.tsp_batch_lso_lds(N, H, wide)
                if N > 2:
                    assert b.value >= lds_bytes(N - 1, H, wide)
    for args, word in (((1, 1, 0), b"2 <= N"), ((0, 1, 0), b"2 <= N"), ((65536, 1, 0), b"2 <= N"),
                       ((5, 2, 0), b"H must be 1 or 24"), ((5, 0, 0), b"H must be 1 or 24"),
                       ((5, 1, 2), b"wide"), ((5, 1, -1), b"wide")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_tsp_batch_lso_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(5, 1, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_tsp_batch_lso_lds" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="H must be 1 or 24"):
        core.tsp_batch_lso_lds(5, 3, False)
    assert solver.BATCH_LSO_LDS_BYTES == LDS_BYTES
    assert solver.BATCH_LSO_MAX_STARTS == 1024 and solver.BATCH_LSO_MAX_ROUNDS == 1000


def test_argument_errors_need_no_gpu(lib):
    """Every argument check comes before the context is looked at, so a
    stand-in block of zeros serves as the non-NULL ctx here; its LDS size of
    zero makes every launch that passes the other checks an LDS refusal."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(4096)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    names = ("m", "st", "t", "k", "du", "i")

    def f(ctx=c, R=1, N=5, H=1, wide=0, S=8, rounds=3, moves=31, **ptrs):
        a = {name: ptrs.get(name, p) for name in names}
        return lib.vrpms_tsp_batch_lso(ctx, a["m"], a["st"], R, N, H, wide, S, rounds, moves, 12345,
                                       a["t"], a["k"], a["du"], a["i"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_tsp_batch_lso:" in msg and word in msg, (kw, msg)

    refused(b"ctx is NULL", ctx=None)
    refused(b"R must not be negative", R=-1)
    for N in (-1, 0, 1, 65536):
        refused(b"2 <= N", N=N)
    for H in (0, 2, 12, 25):
        refused(b"H must be 1 or 24", H=H)
    for wide in (-1, 2):
        refused(b"wide", wide=wide)
    for S in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= S <= 65535 (%d given)" % S, S=S)
    refused(b"rounds must not be negative (-1 given)", rounds=-1)
    for moves in (-1, 0, 32, 255):
        refused(b"1 <= moves <= 31", moves=moves)
        refused(b"(%d given)" % moves, moves=moves)
    for name in names:
        refused(b"NULL", **{name: None})
    refused(b"H must be 1 or 24", R=0, H=3)            # the shape checks also with R = 0
    refused(b"1 <= S <= 65535", R=0, S=0)
    refused(b"1 <= moves <= 31", R=0, moves=0)
    for N, H, wide in ((5, 1, 0), (58, 24, 0), (59, 24, 1), (274, 1, 0)):
        refused(b"needs %d bytes of LDS (0 available)" % lds_bytes(N, H, wide), N=N, H=H, wide=wide)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, S=65535, rounds=2**31 - 1, moves=1) == _lib.VRPMS_OK
    assert f(R=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert buf.raw == bytes(4096) and fake.raw == bytes(1 << 16)


def request(case):
    """The case as a solve_tsp_lso_batch tuple (H = 1 as a plain [N][N] matrix)."""
    D, t0 = inst(case)
    return ((D[0] if D.shape[0] == 1 else D).tolist(), list(range(1, D.shape[1])), 0, t0)


def _sized(N, H, big=0):
    D = np.ones((H, N, N), dtype=np.int64)
    if big:
        D[0, 0, 1] = big
    return solver.compact_tsp(D if H > 1 else D[0], list(range(1, N)), 0, 0)


def test_batch_lso_fits_at_the_lds_edge_and_the_design_table(lib):
    for (H, wide), N in DOMAIN.items():
        assert largest_n_nodes(H, wide) == N, (H, wide, largest_n_nodes(H, wide))
        assert lds_bytes(N, H, wide) <= LDS_BYTES < lds_bytes(N + 1, H, wide)
        assert core.tsp_batch_lso_lds(N, H, wide) <= LDS_BYTES < core.tsp_batch_lso_lds(N + 1, H, wide)
        big = 70000 if wide else 0
        assert solver.batch_lso_fits(_sized(N, H, big), 64, 1000, 31)
        assert not solver.batch_lso_fits(_sized(N + 1, H, big), 64, 1000, 31)
        assert "bytes" in solver.batch_lso_message(_sized(N + 1, H, big), 64, 1000, 31)
        assert solver.batch_lso_key(_sized(N, H, big), 64, 1000, 7) == (N, H, wide, 64, 1000, 7)
    # the table as DESIGN.md prints it
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "DESIGN.md")) as fh:
        design = fh.read()
    section = design[design.index("### 4.3s"):]
    for (H, wide), N in DOMAIN.items():
        row = "| %d | %s | %d | %d | %d |" % (H, "int32" if wide else "uint16", N, N - 1,
                                             lds_bytes(N, H, wide))
        assert row in section, row
    small = _sized(6, 24)
    assert solver.batch_lso_fits(small, 1024, 1000, 31) and solver.batch_lso_fits(small, 1, 0, 1)
    assert not solver.batch_lso_fits(small, 1025, 10, 31) and not solver.batch_lso_fits(small, 0, 10)
    assert not solver.batch_lso_fits(small, 64, 1001) and not solver.batch_lso_fits(small, 64, -1)
    assert not solver.batch_lso_fits(small, 64, 10, 0) and not solver.batch_lso_fits(small, 64, 10, 32)
    assert "starts" in solver.batch_lso_message(small, 1025, 10)
    assert "rounds" in solver.batch_lso_message(small, 64, 1001)
    assert "mask" in solver.batch_lso_message(small, 64, 10, 32)
    # a wide entry halves the cells that fit; 65535 is still narrow
    N = DOMAIN[(24, False)]
    assert not solver.batch_lso_fits(_sized(N, 24, 70000), 64, 1000)
    assert solver.batch_lso_fits(_sized(N, 24, 65535), 64, 1000)
    # a VRP is outside the domain whatever the size
    vrp = solver.compact_vrp(np.ones((3, 3), dtype=np.int64), [{"id": i} for i in range(3)], [3], [0])
    assert "TSP only" in solver.batch_lso_message(vrp, 8, 4)


def test_algorithm_lists():
    assert "lso" in solver.ALGORITHMS
    assert "lso" in service.INLINE_ALGORITHMS["tsp"] and "lso" not in service.INLINE_ALGORITHMS["vrp"]
    assert service.INLINE_ALGORITHMS["tsp"][-1] == "lso"
    assert service.INLINE_KNOBS["moves"] is int and service.KNOB_RANGES["moves"] == (1, 31)


def test_solve_tsp_lso_batch_refusals_need_no_gpu(monkeypatch, lib):
    _no_gpu(monkeypatch)
    good = request((6, 1, 0, ""))
    assert solver.solve_tsp_lso_batch([]) == []
    with pytest.raises(ValueError, match=r"^request 1: customer 9 outside the 7-node matrix"):
        solver.solve_tsp_lso_batch([good, (good[0], [1, 9], 0, 0)])
    with pytest.raises(ValueError, match=r"^request 2: startNode 7 outside"):
        solver.solve_tsp_lso_batch([good, good, {"durations": good[0], "customers": [1, 2],
                                                 "start_node": 7, "start_time": 0}])
    big = np.full((7, 7), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_tsp_lso_batch([good, (big.tolist(), good[1], 0, 0)])
    for starts in (0, -1, 1025):
        with pytest.raises(ValueError, match=r"starts must be in 1\.\.1024"):
            solver.solve_tsp_lso_batch([good], starts=starts)
    for rounds in (-1, 1001):
        with pytest.raises(ValueError, match=r"rounds must be in 0\.\.1000"):
            solver.solve_tsp_lso_batch([good], rounds=rounds)
    for moves in (0, -1, 32):
        with pytest.raises(ValueError, match=r"moves must be in 1\.\.31"):
            solver.solve_tsp_lso_batch([good], moves=moves)
    # outside the domain there is no other path: the limit that failed, by request
    Nbig = DOMAIN[(1, False)] + 1
    bigD = np.ones((Nbig, Nbig), dtype=np.int64).tolist()
    need = lds_bytes(Nbig, 1, False)
    with pytest.raises(ValueError, match=rf"^request 1: lso .* need {need} bytes; the limit is "
                                         rf"{LDS_BYTES} bytes"):
        solver.solve_tsp_lso_batch([good, (bigD, list(range(1, Nbig)), 0, 0)])
    with pytest.raises(ValueError, match=r"^request 0: hour-indexed duration matrix must have 24"):
        solver.solve_tsp_lso_batch([(np.ones((2, 4, 4), dtype=np.int64).tolist(), [1, 2], 0, 0)])
    # no customer: answered on the host, the start node's own edge included
    none = (good[0], [], 3, 77)
    assert solver.solve_tsp_lso_batch([none]) == [{"duration": 0, "vehicle": [3, 3]}]
    assert solver.solve_tsp("lso", *none) == {"duration": 0, "vehicle": [3, 3]}


def test_solve_tsp_lso_and_solve_vrp_lso_errors(monkeypatch, lib):
    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: pytest.fail("the remote was touched"))
    D, customers, node, t0 = request((6, 1, 0, ""))
    with pytest.raises(ValueError, match=r'lso solves the TSP only.*"ls" or "lsr"'):
        solver.solve_vrp("lso", D, [{"id": i} for i in range(7)], [7], [0])
    with pytest.raises(ValueError, match=r"1\.\.1024 starts \(1025 given\)"):
        solver.solve_tsp("lso", D, customers, node, t0, starts=1025)
    with pytest.raises(ValueError, match=r"1\.\.1024 starts \(0 given\)"):
        solver.solve_tsp("lso", D, customers, node, t0, starts=0)
    with pytest.raises(ValueError, match=r"0\.\.1000 rounds \(1001 given\)"):
        solver.solve_tsp("lso", D, customers, node, t0, rounds=1001)
    with pytest.raises(ValueError, match=r"0\.\.1000 rounds \(-1 given\)"):
        solver.solve_tsp("lso", D, customers, node, t0, rounds=-1)
    for moves in (0, 32):
        with pytest.raises(ValueError, match=rf"mask of 1\.\.31 \({moves} given\)"):
            solver.solve_tsp("lso", D, customers, node, t0, moves=moves)
    big = np.full((7, 7), 2**29, dtype=np.int64).tolist()
    with pytest.raises(ValueError, match="A9 guard"):
        solver.solve_tsp("lso", big, customers, node, t0)
    # no customer: answered on the host, before the remote as well
    assert solver.solve_tsp("lso", D, [], 4, t0) == {"duration": 0, "vehicle": [4, 4]}
    with pytest.raises(ValueError, match=r"1\.\.1024 starts \(0 given\)"):
        solver.solve_tsp("lso", D, [], 4, t0, starts=0)
    Nbig = DOMAIN[(24, False)] + 1
    bigD = np.ones((24, Nbig, Nbig), dtype=np.int64).tolist()
    need = lds_bytes(Nbig, 24, False)
    with pytest.raises(ValueError, match=rf"need {need} bytes; the limit is 163840 bytes"):
        solver.solve_tsp("lso", bigD, list(range(1, Nbig)), 0, 0)
    # "ls" and "lsr" keep pointing the TSP caller elsewhere
    with pytest.raises(ValueError, match="ls solves the VRP only"):
        solver.solve_tsp("ls", D, customers, node, t0)


def _tsp_body(case, **more):
    D, customers, node, t0 = request(case)
    return json.dumps(dict({"durations": D, "customers": customers, "startNode": node,
                            "startTime": t0}, **more)).encode()


def test_inline_route_and_the_moves_knob(monkeypatch, lib):
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, len(params["customers"]), dict(knobs.get("inline") or {})))
        return {"duration": 5, "vehicle": [0, 1, 0]}

    app = service.App(service.MemoryStore({}, {}, {}), solve=fake)
    st, res = app.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, "")))
    assert st == 200 and res["message"] == {"duration": 5, "vehicle": [0, 1, 0]}
    st, res = app.solve_inline("tsp", "lso", _tsp_body((5, 24, 0, ""),
                                                       knobs={"moves": 7, "starts": 8, "rounds": 0}))
    assert st == 200
    st, res = app.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, ""), knobs={"moves": 31}))
    assert st == 200
    assert seen == [("tsp", "lso", 5, {}), ("tsp", "lso", 5, {"moves": 7, "starts": 8, "rounds": 0}),
                    ("tsp", "lso", 5, {"moves": 31})]
    del seen[:]
    for moves in (0, 32, -1):
        st, res = app.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, ""), knobs={"moves": moves}))
        assert st == 400 and "knob moves=%d outside [1, 31]" % moves in res["errors"][0]["reason"], res
    st, res = app.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, ""), knobs={"moves": True}))
    assert st == 400 and "must be an integer" in res["errors"][0]["reason"]
    st, res = app.solve_inline("vrp", "lso", b"{}")
    assert st == 400 and "no solver /solve/vrp/lso" in res["errors"][0]["reason"]
    assert seen == []
    # the real path: a request outside the domain is solve_tsp("lso")'s 400,
    # before any device is touched
    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: None)
    real = service.App(service.MemoryStore({}, {}, {}))
    Nbig = DOMAIN[(1, False)] + 1
    body = json.dumps({"durations": np.ones((Nbig, Nbig), dtype=np.int64).tolist(),
                       "customers": list(range(1, Nbig)), "startNode": 0, "startTime": 0}).encode()
    st, res = real.solve_inline("tsp", "lso", body)
    assert st == 400 and "need %d bytes; the limit is 163840 bytes" % lds_bytes(Nbig, 1, False) in \
        res["errors"][0]["reason"], res
    st, res = real.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, ""), knobs={"starts": 1024,
                                                                             "rounds": 1000}))
    assert st == 400 and "the GPU was touched" in res["errors"][0]["reason"]


def test_remote_forwards_the_moves_knob(monkeypatch, lib):
    """The forwarding table of vrpms_amd.remote is INLINE_KNOBS, and with a
    remote solve_tsp_lso_batch sends one solve_tsp("lso") per request, after
    the host checks and without the requests that have no customer."""
    from vrpms_amd import remote
    out = {}
    remote._options(out, 1, None, {"moves": 7, "starts": 8, "rounds": 0})
    assert out["knobs"] == {"moves": 7, "starts": 8, "rounds": 0}
    sent = []

    class Box:
        @staticmethod
        def solve_tsp(algorithm, durations, customers, start_node, start_time, **kw):
            sent.append((algorithm, list(customers), start_node, start_time, kw))
            return {"duration": 1, "vehicle": [start_node] + list(customers) + [start_node]}

    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: Box)
    a, b = request((6, 1, 0, "")), request((5, 24, 1, ""))
    got = solver.solve_tsp_lso_batch([a, (a[0], [], 2, 5), b], starts=8, rounds=3, moves=7, seed=9)
    assert got == [{"duration": 1, "vehicle": [0] + a[1] + [0]}, {"duration": 0, "vehicle": [2, 2]},
                   {"duration": 1, "vehicle": [0] + b[1] + [0]}]
    knobs = dict(seed=9, time_limit=None, starts=8, rounds=3, moves=7)
    assert sent == [("lso", a[1], 0, a[3], knobs), ("lso", b[1], 0, b[3], knobs)]
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_tsp_lso_batch([a, (np.full((7, 7), 2**29).tolist(), a[1], 0, 0)])
    assert len(sent) == 2


def _improving(D, t0, tour, key, moves):
    """Brute force: some enabled move of `tour`, walked in full by
    spec.eval_tsp, has a key below `key`."""
    return any(spec.tsp_key(spec.eval_tsp(D, moved(tour, *mv), t0)) < key
               for mv in all_moves(len(tour), moves))


def test_reference_against_brute_force_and_a25():
    """a27_ref itself: its end tour admits no improving move of the enabled
    types (every move re-walked by spec.eval_tsp, one by one), and with moves
    = 7 it is a25_ref's tour at K = 1, zero demand, objective sum."""
    for case in ((7, 1, 60, ""), (6, 24, 61, ""), (5, 1, 62, ""), (7, 24, 63, "hours"), (4, 1, 64, ""),
                 (3, 24, 65, ""), (2, 1, 66, "")):
        D, t0 = inst(case)
        n = case[0]
        for moves in (31, 7, 24, 1, 2, 4, 8, 16):
            r = a27_ref(D, t0, 5, 1000, moves, SEED)
            assert r["capped"] == 0 and sorted(r["tour"]) == list(range(1, n + 1))
            assert not _improving(D, t0, r["tour"], r["key"], moves), (case, moves)
            assert r["key"] == spec.tsp_key(spec.eval_tsp(D, r["tour"], t0)) == r["dur"] << 28
        r7 = a27_ref(D, t0, 5, 1000, 7, SEED)
        old = a25_ref(D, np.zeros(n + 1, dtype=np.int64), [0], [t0], "sum", 5, 1000, SEED)
        assert (r7["tour"], r7["s"], r7["capped"], r7["rounds"], r7["moves"]) == \
            (old["tour"], old["s"], old["capped"], old["rounds"], old["moves"]), case
        assert r7["key"] >> 28 == old["key"] >> 28 and old["durs"] == [r7["dur"]]
    # the move order and the counts: the triangles, relocate, then the Or-opt
    # types with (n - m + 1)(n - m) moves, none when n <= m
    assert all_moves(3, 8) == [(3, 0, 1), (3, 1, 0)] and all_moves(3, 16) == []
    assert all_moves(2, 24) == [] and all_moves(4, 16) == [(4, 0, 1), (4, 1, 0)]
    for n in range(1, 14):
        assert len(all_moves(n)) == 2 * n * (n - 1) + \
            sum((n - m + 1) * (n - m) for m in (2, 3) if n > m)
    assert oropt([1, 2, 3, 4, 5, 6], 2, 1, 3) == [1, 4, 5, 2, 3, 6]
    assert oropt([1, 2, 3, 4, 5, 6], 3, 3, 0) == [4, 5, 6, 1, 2, 3]
    assert all(oropt(list(range(9)), 1, i, j) == spec.apply_move(list(range(9)), 2, i, j)
               for i in range(9) for j in range(9) if i != j)


def test_reference_properties():
    """What the GPU comparisons rely on, checked on the reference itself."""
    refs = {run: reference(run) for run in ALL_RUNS}
    # the tie rule is exercised
    assert any(reference(run)["move_tie"] for run in TIES)
    assert all(reference(run)["end_tie"] for run in TIES)
    # with the round cap out of reach no descent is capped
    for run in N_EDGES + S_EDGES + MASKS + TIES + HOURS + CLOCK + HUGE + R_EDGES[-1:]:
        r = refs[run]
        assert r["capped"] == 0 and max(r["rounds"]) < run[2]
    # every type is applied somewhere; the Or-opt types from n = 3 and n = 4 on
    assert {typ for r in refs.values() for typ, _, _ in r["moves"]} == {0, 1, 2, 3, 4}
    for run in MASKS:
        assert all((run[3] >> typ) & 1 for typ, _, _ in refs[run]["moves"])
    for mask in (8, 16, 24):
        assert any(refs[run]["moves"] for run in MASKS if run[3] == mask)
    # the key never rises with S, nor with the round cap
    keys = [refs[run]["key"] for run in S_EDGES]
    assert keys == sorted(keys, reverse=True) and keys[-1] < keys[0]
    caps = [refs[run]["capped"] for run in R_EDGES]
    assert caps[0] == 7 and 0 < caps[2] <= caps[1] <= 7 and caps[3] == 0
    keys = [refs[run]["key"] for run in R_EDGES]
    assert keys[0] > keys[1] >= keys[2] >= keys[3]
    assert all(0 < refs[run]["capped"] for run in WAVES)
    # n = 1 has no moves: not capped even at rounds = 0; start 0 wins every tie
    one = a27_ref(*inst((1, 1, 1, "")), 5, 0, 31, SEED)
    assert (one["tour"], one["s"], one["capped"]) == ([1], 0, 0)
    # "huge": every key is the clamp, no move applied, start 0 the answer, and
    # the duration is reported unclamped
    for run in HUGE:
        r = refs[run]
        assert r["key"] == (2**28 - 1) << 28 and r["s"] == 0 and r["rounds"] == [0] * 6
        assert r["dur"] > 2**28 and r["capped"] == 0
    # a winner from every wavefront, and one beyond the first sweep of four
    assert {r["s"] % 4 for r in refs.values()} == {0, 1, 2, 3}
    assert any(r["s"] >= 4 for r in refs.values())
    # the clock cases cross an hour and midnight: the static slice gives another answer
    for run in HOURS + CLOCK[1:]:
        D, t0 = inst(run[0])
        r = refs[run]
        assert spec.eval_tsp(D[:1], r["tour"], t0) != r["dur"]
    assert any(inst(run[0])[1] + refs[run]["dur"] >= 1440 for run in HOURS + CLOCK)
    # the first move of the long runs
    up, down, rev = (refs[run]["moves"][0] for run in LONG)
    assert up[0] in (3, 4) and up[2] - up[1] > 64
    assert down[0] in (3, 4) and down[1] - down[2] > 64
    assert rev[0] == 1 and rev[2] - rev[1] + 1 > 128


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_batch(ctx, cases, S, rounds, moves, wide=None):
    """One tsp_batch_lso launch -> ([key], [tour], [dur], [info])."""
    import torch
    insts = [inst(c) for c in cases]
    mats = torch.tensor(np.stack([D for D, _ in insts]), dtype=torch.int32, device=ctx.dev)
    st = torch.tensor([t0 for _, t0 in insts], dtype=torch.int32, device=ctx.dev)
    tours, keys, durs, info = ctx.tsp_batch_lso(mats, st, S, rounds, moves, SEED, wide=wide)
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), info.cpu().tolist())


def gpu_runs(ctx, runs, wide=None):
    """Runs of one shape and one (S, rounds, moves) in one launch."""
    assert len({r[1:] for r in runs}) == 1 and len({r[0][:2] for r in runs}) == 1
    return gpu_batch(ctx, [r[0] for r in runs], *runs[0][1:], wide=wide)


def by_launch(runs):
    """The runs grouped by what one launch shares."""
    groups = {}
    for r in runs:
        groups.setdefault((r[0][:2], r[1:]), []).append(r)
    return list(groups.values())


@pytest.mark.gpu
@pytest.mark.parametrize("runs", [N_EDGES, WAVES, S_EDGES, R_EDGES, TIES, HOURS, CLOCK, LONG],
                         ids=["n-edges", "waves", "s-edges", "r-edges", "ties", "hours", "clock", "long"])
def test_gpu_equals_reference(ctx, runs):
    for group in by_launch(runs):
        got = gpu_runs(ctx, group)
        want = expected(group)
        print([run_id(r) for r in group], "gpu", got, "ref", want)
        assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("H", (1, 24))
def test_gpu_every_mask(ctx, H):
    for run in [r for r in MASKS if r[0][1] == H]:
        got = gpu_runs(ctx, [run])
        assert got == expected([run]), run_id(run)


@pytest.mark.gpu
def test_gpu_staging_width_refusals_and_the_clamp(ctx):
    """All four instantiations, (uint16 | int32) x (H = 1 | 24): an entry of
    65535 rides uint16, 65536 is the refusal row there and rides int32;
    a negative entry is refused under either width; durations above 2^28."""
    import torch
    for H in (1, 24):
        a, b, c = (7, H, 30, ""), (7, H, 31, "e65535"), (7, H, 32, "")
        over = (7, H, 31, "e65536")

        def runs(*cases):
            return [(x, 6, 1000, 31) for x in cases]

        assert gpu_runs(ctx, runs(a, b, c), wide=False) == expected(runs(a, b, c))
        assert gpu_runs(ctx, runs(a, over, c), wide=True) == expected(runs(a, over, c))
        assert gpu_runs(ctx, runs(over)) == expected(runs(over))   # wide=None
        want = expected(runs(a, over, c))
        keys, tours, durs, info = gpu_runs(ctx, runs(a, over, c), wide=False)
        assert keys[1] == 2**64 - 1 and tours[1] == [0] * 7 and durs[1] == 0 and info[1] == [-1, 0]
        for x in (0, 2):
            assert (keys[x], tours[x], durs[x], info[x]) == tuple(w[x] for w in want)
        mats = np.stack([inst(x)[0] for x in (a, b, c)]).astype(np.int32)
        mats[1, H - 1, 3, 2] = -1
        st = torch.tensor([inst(x)[1] for x in (a, b, c)], dtype=torch.int32, device=ctx.dev)
        want = expected(runs(a, b, c))
        for wide in (False, True):
            tours, keys, durs, info = ctx.tsp_batch_lso(
                torch.tensor(mats, dtype=torch.int32, device=ctx.dev), st, 6, 1000, 31, SEED, wide=wide)
            assert keys[1].item() == -1 and tours[1].tolist() == [0] * 7 and durs[1].item() == 0 and \
                info[1].tolist() == [-1, 0]
            for x in (0, 2):
                assert (int(keys[x].item()) & (2**64 - 1), tours[x].tolist(), durs[x].item(),
                        info[x].tolist()) == tuple(w[x] for w in want)
    for run in HUGE:
        got = gpu_runs(ctx, [run])
        assert got == expected([run]) and got[3] == [[0, 0]] and got[2][0] > 2**28


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(135, 1, 4, 40), (40, 24, 8, 1000)], ids=["n135-H1", "n40-H24"])
def test_gpu_moves_7_is_vrp_batch_ls_at_one_vehicle(ctx, shape):
    """No oracle involved: the delta pricing over hundreds of rounds against
    the full walks of vrp_batch_ls, K = 1, zero demand, objective sum."""
    import torch
    n, H, S, rounds = shape
    cases = [(n, H, 90 + x, "") for x in range(3)]
    insts = [inst(c) for c in cases]
    mats = torch.tensor(np.stack([D for D, _ in insts]), dtype=torch.int32, device=ctx.dev)
    st = torch.tensor([t0 for _, t0 in insts], dtype=torch.int32, device=ctx.dev)
    zero = torch.zeros((len(cases), n + 1), dtype=torch.int32, device=ctx.dev)
    for cap in (0, 5):
        caps = torch.full((len(cases), 1), cap, dtype=torch.int32, device=ctx.dev)
        old = ctx.vrp_batch_ls(mats, zero, caps, st.reshape(-1, 1).contiguous(), spec.OBJ_SUM, S,
                               rounds, SEED)
        new = ctx.tsp_batch_lso(mats, st, S, rounds, 7, SEED)
        assert torch.equal(new[0], old[0]) and torch.equal(new[3], old[4])
        assert torch.equal(new[1] >> 28, old[1] >> 28) and torch.equal(new[2], old[2][:, 0])
        assert torch.equal(new[1] & (2**28 - 1), torch.zeros_like(new[1]))
    # the descents ran long: some were capped at n = 135, none at n = 40
    assert (new[3][:, 1] == (S if n == 135 else 0)).all().item()
    for x, (D, t0) in enumerate(insts):
        assert spec.eval_tsp(D, new[0][x].tolist(), t0) == new[2][x].item()
    # and the five types end no worse than the three from the same starts
    full = ctx.tsp_batch_lso(mats, st, S, 1000, 31, SEED)
    for x, (D, t0) in enumerate(insts):
        assert spec.eval_tsp(D, full[0][x].tolist(), t0) == full[2][x].item()
        assert sorted(full[0][x].tolist()) == list(range(1, n + 1))


@pytest.mark.gpu
def test_gpu_batch_independence(ctx):
    import torch
    want = expected(SIX)
    together = gpu_runs(ctx, SIX)
    assert together == want
    S, rounds, moves = SIX[0][1:]
    cases = [SIX[x % 6][0] for x in range(300)]
    cases[0] = cases[299] = SIX[3][0]
    stream = torch.cuda.Stream(device=ctx.dev)
    with torch.cuda.stream(stream):
        big = gpu_batch(ctx, cases, S, rounds, moves)
    stream.synchronize()
    for x in range(300):
        src = 3 if x in (0, 299) else x % 6
        assert tuple(g[x] for g in big) == tuple(g[src] for g in together), x
    for x in range(6):
        assert gpu_runs(ctx, [SIX[x]]) == tuple([g[x]] for g in together)
    # R = 0 returns empty tensors
    out = ctx.tsp_batch_lso(torch.zeros((0, 24, 11, 11), dtype=torch.int32, device=ctx.dev),
                            torch.zeros((0,), dtype=torch.int32, device=ctx.dev), 8, 5, 31, SEED)
    assert [tuple(t.shape) for t in out] == [(0, 10), (0,), (0,), (0, 2)]


@pytest.mark.gpu
def test_gpu_lds_edge(ctx):
    import torch
    lib, H, R = ctx.lib, 24, 2
    N = DOMAIN[(H, False)]
    runs = [((N - 1, H, 40 + x, ""), 4, 1, 31) for x in range(R)]
    assert gpu_runs(ctx, runs) == expected(runs)
    N += 1
    n = N - 1
    M = torch.ones((R, H, N, N), dtype=torch.int32, device=ctx.dev)
    st = torch.ones((R,), dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R, n), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R,), -7, dtype=torch.int32, device=ctx.dev)
    info = torch.full((R, 2), -7, dtype=torch.int32, device=ctx.dev)
    rc = lib.vrpms_tsp_batch_lso(ctx.handle, M.data_ptr(), st.data_ptr(), R, N, H, 0, 4, 1, 31, SEED,
                                 tours.data_ptr(), keys.data_ptr(), durs.data_ptr(), info.data_ptr(),
                                 ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_tsp_batch_lso:" in msg and b"bytes of LDS" in msg
    assert str(lds_bytes(N, H, False)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item()
    assert (durs == -7).all().item() and (info == -7).all().item()


def _ref_dict(case, S, rounds, moves):
    r = reference((case, S, rounds, moves))
    return {"duration": r["dur"], "vehicle": [0] + r["tour"] + [0]}


@pytest.mark.gpu
def test_solve_tsp_lso_batch_and_solve_tsp_mixed_list():
    S, rounds = 8, 1000
    D7, cust7, _, t7 = request((6, 24, 50, ""))
    inside = {0: (6, 24, 51, ""), 1: (9, 1, 52, ""), 3: (6, 24, 53, ""), 5: (9, 1, 54, "")}
    reqs = [request(inside[0]), request(inside[1]),
            (D7, [], 2, t7),                                                  # no customer
            request(inside[3]),
            {"durations": D7, "customers": [5, 3, 3, 1], "start_node": 2, "start_time": 1439},
            request(inside[5])]
    kw = dict(starts=S, rounds=rounds, seed=SEED)
    got = solver.solve_tsp_lso_batch(reqs, **kw)
    assert got[2] == {"duration": 0, "vehicle": [2, 2]}
    for r, res in zip(reqs, got):
        if isinstance(r, dict):
            r = (r["durations"], r["customers"], r["start_node"], r["start_time"])
        ci = solver.compact_tsp(*r)
        assert res["vehicle"][0] == res["vehicle"][-1] == ci.nodes[0]
        assert sorted(res["vehicle"][1:-1]) == sorted(ci.nodes[1:])
        tour = [ci.nodes.index(c) for c in res["vehicle"][1:-1]]
        assert res["duration"] == spec.eval_tsp(ci.durations, tour, r[3])
    # the answers are A27's, through either entry point, element for element
    for x, case in inside.items():
        assert got[x] == _ref_dict(case, S, rounds, 31)
        assert solver.solve_tsp("lso", *reqs[x], **kw) == got[x]
    r4 = reqs[4]
    assert solver.solve_tsp("lso", r4["durations"], r4["customers"], r4["start_node"],
                            r4["start_time"], **kw) == got[4]
    assert solver.solve_tsp("lso", *reqs[2], **kw) == got[2]
    # deterministic, the same alone as in company, and the mask is read
    assert solver.solve_tsp_lso_batch(reqs, **kw) == got
    for x in (0, 1, 4):
        assert solver.solve_tsp_lso_batch([reqs[x]], **kw) == [got[x]]
    assert solver.solve_tsp_lso_batch([reqs[1]], moves=1, **kw) == [_ref_dict(inside[1], S, rounds, 1)]
    assert solver.solve_tsp("lso", *reqs[1], moves=7, **kw) == _ref_dict(inside[1], S, rounds, 7)


@pytest.mark.gpu
def test_inline_route_over_http():
    S, rounds = 8, 1000
    app = service.App(service.MemoryStore({}, {}, {}), seed=SEED)
    srv = service.serve(app, "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    case = (9, 1, 52, "")
    try:
        req = urllib.request.Request(
            f"http://127.0.0.1:{srv.server_address[1]}/solve/tsp/lso",
            data=_tsp_body(case, knobs={"starts": S, "rounds": rounds, "moves": 7}), method="POST")
        with urllib.request.urlopen(req, timeout=120) as resp:
            status, res = resp.status, json.loads(resp.read())
    finally:
        srv.shutdown()
        srv.server_close()
        th.join()
    assert status == 200 and res["success"], res
    assert res["message"] == _ref_dict(case, S, rounds, 7)
