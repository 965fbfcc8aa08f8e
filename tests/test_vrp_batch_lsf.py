"""Batched VRP multi-start local search over plain separator tours with delta
pricing (spec A28): the C entry points vrpms_vrp_batch_lsf_lds /
vrpms_vrp_batch_lsf, Context.vrp_batch_lsf, solver.batch_lsf_key /
batch_lsf_message / batch_lsf_fits / solve_vrp_lsf_batch, solve_vrp("lsf") and
the service's batcher (App(batch_vrp_lsf=True)).

The reference is a28_ref below: tests/test_vrp_batch_lsr.py's a26_ref with the
plain filter -- a move whose moved tour is not plain is no candidate -- and the
rule that a start which is not plain ends where it starts, uncapped.  Every
candidate is priced by a full walk (spec.eval_cvrp_batch).  Per request the GPU
must return the identical key, tour, route durations, vehicle row and info row,
for both objectives.  Three equivalences need no oracle: on all-roomy requests
the rows are Context.vrp_batch_lsr's, at K = 1 Context.vrp_batch_ls's, and at
rounds = 0 Context.vrp_batch_lsr's for any capacities -- there but for the
capped count, which A28 keeps at the plain starts (A26 caps every start at
rounds = 0, A28 never caps a start that is not plain)."""
import ctypes
import functools
import json
import threading
import urllib.request

import numpy as np
import pytest

from oracle import spec
from test_vrp_batch_ga import (_FakeApp, _body, _concurrently, _locs, _no_gpu, _rescored, _sized)
from test_vrp_batch_ls import LDS_BYTES, M32, OBJECTIVES, SEED, all_moves, obj_id, pad
from test_vrp_batch_lsr import _fake_launch, a26_ref
from test_vrp_batch_lsr import inst as lsr_inst
from vrpms_amd import _lib, core, service, solver


# ---------------------------------------------------------------------------
# instances and their references (computed once, shared, never changed)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inst(case):
    """tests/test_vrp_batch_lsr.py's inst family, plus the variant "allroomy":
    every vehicle carries the total demand, so every tour is plain; "heavy":
    demands of 2^29 under capacities of 2^30, so a tour's demands sum to 2^32
    and more while a plain segment stays below 2^31; and "nofit": five
    customers of demand 10^9, which no vehicle takes, so no start is plain and
    the last route's load is past 2^32."""
    n, K, H, seed, variant = case
    if variant not in ("allroomy", "heavy", "nofit"):
        return lsr_inst(case)
    D, dem, caps, starts = lsr_inst((n, K, H, seed, ""))
    if variant == "allroomy":
        return D, dem, (int(dem.sum()),) * K, starts
    dem = dem.copy()
    if variant == "heavy":     # every customer 2^29, two to a vehicle of 2^30: all of it plain
        dem[1:] = 2**29
        caps = (2**30,) * K
    else:                      # five customers of 10^9 that fit nowhere, the family's capacities
        dem[1:6] = 10**9
    dem.setflags(write=False)
    return D, dem, caps, starts


def request(case, base=0):
    D, dem, caps, starts = inst(case)
    return ((D[0] if D.shape[0] == 1 else D).tolist(), _locs(dem, base), list(caps), list(starts))


def is_plain(t, dem, caps):
    g, load = 0, 0
    for c in t:
        if c == 0:
            g, load = g + 1, 0
        else:
            load += int(dem[c])
            if load > caps[g]:
                return False
    return True


def plain_mask(cands, dem, caps):
    """is_plain for every row of `cands` at once."""
    c = np.asarray(cands, dtype=np.int64)
    K = len(caps)
    sep = c == 0
    seg = np.cumsum(sep, axis=1) - sep
    loads = np.zeros((c.shape[0], K), dtype=np.int64)
    rows = np.repeat(np.arange(c.shape[0]), c.shape[1])
    np.add.at(loads, (rows, seg.ravel()), np.where(sep, 0, np.asarray(dem, dtype=np.int64)[c]).ravel())
    return (loads <= np.asarray(caps, dtype=np.int64)[None, :]).all(axis=1)


def a28_ref(D, dem, caps, starts, objective, S, rounds, seed):
    """Spec A28 -> a26_ref's dict (without the tie flags) plus plain: whether
    every start tour is plain."""
    D = spec.as_3d(D)
    n = D.shape[1] - 1
    skey = spec.seed_key(seed)
    caps, starts, obj = list(caps), list(starts), obj_id(objective)
    L = n + len(caps) - 1
    moves = all_moves(L)
    ends, capped, applied_all, took, first, plain = [], 0, [], [], [], []
    for s in range(S):
        p = list(range(1, n + 1))
        for q in range(n - 1, 0, -1):
            j = spec.philox4x32_10((M32, M32, s, q), skey)[0] % (q + 1)
            p[q], p[j] = p[j], p[q]
        t = spec.pack_separators(p, len(caps) - 1, dem, caps)
        first.append(t)
        plain.append(is_plain(t, dem, caps))
        k = int(spec.eval_cvrp_batch(D, [t], dem, caps, starts, obj)[0][0])
        applied = 0
        while L >= 2 and plain[-1]:
            if applied >= rounds:
                capped += 1
                break
            cands = [spec.apply_move(t, *m) for m in moves]
            ok = plain_mask(cands, dem, caps)
            keys = [int(x) if good else 2**64 - 1 for x, good in
                    zip(spec.eval_cvrp_batch(D, cands, dem, caps, starts, obj)[0], ok)]
            kmin = min(keys)
            if not kmin < k:
                break
            at = keys.index(kmin)   # the moves are in (typ, i, j) order
            t, k = cands[at], kmin
            took.append(moves[at])
            applied += 1
        ends.append((k, s, t))
        applied_all.append(applied)
    k, s, t = min(ends, key=lambda e: e[:2])
    final = spec.eval_cvrp(D, t, dem, caps, starts, obj)
    assert final["key"] == k
    return dict(key=k, tour=t, durs=final["durations"], veh=final["vehicle_of"], s=s, capped=capped,
                unvisited=final["unvisited"], rounds=applied_all, moves=took, first=first,
                plain=plain, ends=ends)


@functools.lru_cache(maxsize=None)
def reference(run, objective):
    """run = (case, S, rounds)."""
    case, S, rounds = run
    return a28_ref(*inst(case), objective, S, rounds, SEED)


@functools.lru_cache(maxsize=None)
def reference26(run, objective):
    case, S, rounds = run
    return a26_ref(*inst(case), objective, S, rounds, SEED)


ROW = ("key", "tour", "durs", "veh", "s", "capped")


def expected(runs, objective):
    refs = [reference(r, objective) for r in runs]
    return ([r["key"] for r in refs], [r["tour"] for r in refs], [r["durs"] for r in refs],
            [r["veh"] for r in refs], [[r["s"], r["capped"]] for r in refs])


def lds_bytes(N, K, wide):
    """DESIGN.md §4.3v restated, L = N + K - 2 tokens: the matrix padded to 16
    bytes, the demand row and the two fleet rows as int32 padded to four
    words, 16 bytes per wavefront, and per wavefront three int32 rows of L + 2
    and five int32 tables of K + 1 padded to four words, uint16 rows of L + 2,
    L and K + 1 padded to eight, and a byte row of L + 2 padded to eight."""
    L = N - 1 + K - 1
    return pad(N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + 4 * 16 + \
        4 * (4 * (3 * pad(L + 2, 4) + 5 * pad(K + 1, 4)) +
             2 * (pad(L + 2, 8) + pad(L, 8) + pad(K + 1, 8)) + pad(L + 2, 8))


def largest_n_nodes(K, wide):
    return max(N for N in range(2, 400) if lds_bytes(N, K, wide) <= LDS_BYTES)


# DESIGN.md §4.3v's domain table: (K, wide) -> the largest N
DOMAIN = {(1, False): 268, (1, True): 193, (4, False): 267, (4, True): 192, (8, False): 267,
          (8, True): 192, (64, False): 258, (64, True): 186}

# the runs of the GPU comparisons: (case, S, rounds), the H = 1 runs of
# tests/test_vrp_batch_lsr.py's lists and static copies of its S_EDGES
N_EDGES = [((n, 3, 1, n, ""), 6, 1000) for n in (1, 2, 3, 4, 5, 6, 7, 8, 11, 12)] + \
    [((1, 1, 1, 1, ""), 6, 1000)]
WAVES = [((L - 3, 4, 1, 80 + L, ""), 5, 2 if L < 63 else 1) for L in (32, 33, 63, 64, 65)]
S_EDGES = [((9, 3, 1, 70, ""), S, 1000) for S in (1, 3, 4, 5, 8, 9, 64)]
R_EDGES = [((8, 3, 1, 9, ""), 7, rounds) for rounds in (0, 1, 2, 1000)]
TIES = [((7, 2, 1, 3, "ties"), 12, 1000)]
VARIANTS = [((9, 3, 1, 14, "zerodem"), 8, 1000), ((7, 3, 1, 31, "e65536"), 8, 1000),
            ((3, 64, 1, 12, ""), 4, 1000)]
ONE_PLAIN_SHORT = [((12, 4, 1, 41, ""), 6, 1000)]
# demands whose sums pass 2^32 inside one chunk of 64 positions, and across two
HEAVY = [((8, 4, 1, 5, "heavy"), 6, 1000), ((9, 3, 1, 6, "nofit"), 6, 1000),
         ((70, 36, 1, 7, "heavy"), 2, 3)]
# L = 136 tokens: the rows and every candidate cross the chunks of 64 and 128
LONG = [((133, 4, 1, 336, ""), 1, 2)]
ALL_RUNS = N_EDGES + WAVES + S_EDGES + R_EDGES + TIES + VARIANTS + ONE_PLAIN_SHORT + HEAVY + LONG
SIX = [((10, 3, 1, 20 + x, ""), 16, 1000) for x in range(6)]


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
    f = lib.vrpms_vrp_batch_lsf_lds
    for wide in (0, 1):
        for K in (1, 3, 4, 5, 7, 8, 64):
            for N in GRID_N:
                assert f(N, K, wide, ctypes.byref(b)) == _lib.VRPMS_OK
                assert b.value == lds_bytes(N, K, wide) == core.vrp_batch_lsf_lds(N, K, 1, wide)
                assert b.value > core.vrp_batch_lsr_lds(N, K, 1, wide)
                if N > 2:
                    assert b.value >= lds_bytes(N - 1, K, wide)
                if K > 1:
                    assert b.value >= lds_bytes(N, K - 1, wide)
    for args, word in (((1, 3, 0), b"2 <= N"), ((0, 3, 0), b"2 <= N"), ((65536, 3, 0), b"2 <= N"),
                       ((5, 0, 0), b"1 <= K <= 64"), ((5, 65, 0), b"1 <= K <= 64"),
                       ((65535, 3, 0), b"N + K - 2 <= 65535 (65536 given)"),
                       ((5, 3, 2), b"wide"), ((5, 3, -1), b"wide")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsf_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(65535, 2, 0, ctypes.byref(b)) == _lib.VRPMS_OK
    assert f(5, 3, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_lsf_lds: bytes is NULL" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= K <= 64"):
        core.vrp_batch_lsf_lds(5, 65, 1, False)
    with pytest.raises(ValueError, match="H must be 1 .24 given.*vrp_batch_lsr"):
        core.vrp_batch_lsf_lds(5, 3, 24, False)
    assert solver.BATCH_LSF_LDS_BYTES == LDS_BYTES
    assert (solver.BATCH_LSF_MAX_STARTS, solver.BATCH_LSF_MAX_ROUNDS) == (1024, 1000)
    # the domain table's edges
    for (K, wide), N in DOMAIN.items():
        assert largest_n_nodes(K, wide) == N, (K, wide, largest_n_nodes(K, wide))
        assert f(N, K, int(wide), ctypes.byref(b)) == _lib.VRPMS_OK and b.value <= LDS_BYTES
        assert f(N + 1, K, int(wide), ctypes.byref(b)) == _lib.VRPMS_OK and b.value > LDS_BYTES


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
        return lib.vrpms_vrp_batch_lsf(ctx, a["m"], a["d"], a["cp"], a["st"], R, N, K, H, obj, wide, S,
                                       rounds, 12345, a["t"], a["k"], a["du"], a["v"], a["i"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsf:" in msg and word in msg, (kw, msg)

    refused(b"ctx is NULL", ctx=None)
    refused(b"R must not be negative", R=-1)
    for N in (-1, 0, 1, 65536):
        refused(b"2 <= N", N=N)
    for K in (-1, 0, 65, 1000):
        refused(b"1 <= K <= 64", K=K)
    refused(b"N + K - 2 <= 65535 (65536 given)", N=65535, K=3)
    for H in (0, 2, 12, 25):
        refused(b"H must be 1 or 24", H=H)
    refused(b"H must be 1 (24 given)", H=24)
    refused(b"vrpms_vrp_batch_lsr", H=24)
    refused(b"H must be 1 (24 given)", H=24, R=0)
    for obj in (-1, 2):
        refused(b"objective", obj=obj)
    for wide in (-1, 2):
        refused(b"wide", wide=wide)
    for S in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= S <= 65535 (%d given)" % S, S=S)
    refused(b"rounds must not be negative (-1 given)", rounds=-1)
    for name in names:
        refused(b"NULL", **{name: None})
    refused(b"1 <= S <= 65535", R=0, S=0)
    for N, K, wide in ((5, 2, 0), (58, 4, 1), (5, 1, 0), (12, 64, 0)):
        refused(b"needs %d bytes of LDS (0 available)" % lds_bytes(N, K, wide), N=N, K=K, wide=wide)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, S=65535, rounds=2**31 - 1) == _lib.VRPMS_OK
    assert f(R=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert buf.raw == bytes(4096) and fake.raw == bytes(1 << 16)


def test_batch_lsf_fits_at_the_lds_edge(lib):
    for (K, wide), N in DOMAIN.items():
        assert lds_bytes(N, K, wide) <= LDS_BYTES < lds_bytes(N + 1, K, wide)
        big = 70000 if wide else 0
        assert solver.batch_lsf_fits(_sized(N, K, 1, big), 64, 1000)
        assert not solver.batch_lsf_fits(_sized(N + 1, K, 1, big), 64, 1000)
        assert "bytes" in solver.batch_lsf_message(_sized(N + 1, K, 1, big), 64, 1000)
        assert solver.batch_lsf_key(_sized(N, K, 1, big), 64, 1000) == (N, K, 1, wide, 64, 1000)
        # the rows cost nodes: A26 fits more
        assert solver.batch_lsr_fits(_sized(N + 1, K, 1, big), 64, 1000)
    small = _sized(6, 2, 1)
    assert solver.batch_lsf_fits(small, 1024, 1000) and solver.batch_lsf_fits(small, 1, 0)
    assert not solver.batch_lsf_fits(small, 1025, 10) and not solver.batch_lsf_fits(small, 0, 10)
    assert not solver.batch_lsf_fits(small, 64, 1001) and not solver.batch_lsf_fits(small, 64, -1)
    assert "lsf" in solver.batch_lsf_message(small, 1025, 10)
    assert "starts" in solver.batch_lsf_message(small, 1025, 10)
    assert "rounds" in solver.batch_lsf_message(small, 64, 1001)
    # an hour-indexed request is outside whatever its size, and is told where to go
    hours = _sized(6, 2, 24)
    assert not solver.batch_lsf_fits(hours, 64, 1000) and solver.batch_lsr_fits(hours, 64, 1000)
    msg = solver.batch_lsf_message(hours, 64, 1000)
    assert "static duration matrix (24 slices given)" in msg and '"lsr"' in msg
    assert "vehicles" in solver.batch_lsf_message(_sized(5, 65, 1), 8, 4)
    none = solver.compact_vrp(np.ones((3, 3), dtype=np.int64), _locs([0, 1, 1]), [3], [0], [1, 2])
    assert none.n == 0 and not solver.batch_lsf_fits(none, 8, 4)
    tsp = solver.compact_tsp(np.ones((4, 4), dtype=np.int64), [1, 2, 3], 0, 0)
    assert not solver.batch_lsf_fits(tsp, 8, 4)
    b = service.VrpLsfBatcher(_FakeApp(), launch=_fake_launch([]))
    assert (b.starts, b.rounds) == (64, 1000)
    assert b.accepts(small) and not b.accepts(_sized(6, 2, 1, 2**29))               # the A9 guard
    assert not b.accepts(_sized(5, 65, 1)) and not b.accepts(hours)
    for kw in (dict(starts=0), dict(starts=1025), dict(rounds=-1), dict(rounds=1001)):
        with pytest.raises(ValueError, match="starts|rounds"):
            service.VrpLsfBatcher(_FakeApp(), launch=_fake_launch([]), **kw)


def test_solve_vrp_lsf_refusals_with_a_fake_launch(monkeypatch, lib):
    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: None)
    good = request((6, 2, 1, 0, ""))
    assert solver.solve_vrp_lsf_batch([]) == []
    with pytest.raises(ValueError, match=r"^request 1: capacities and startTimes"):
        solver.solve_vrp_lsf_batch([good, (good[0], good[1], [3, 3], [0])])
    big = np.full((7, 7), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_vrp_lsf_batch([good, (big.tolist(), good[1], [3, 3], [0, 0])])
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp_lsf_batch([good], objective="mean")
    for starts in (0, -1, 1025):
        with pytest.raises(ValueError, match=r"starts must be in 1\.\.1024"):
            solver.solve_vrp_lsf_batch([good], starts=starts)
    for rounds in (-1, 1001):
        with pytest.raises(ValueError, match=r"rounds must be in 0\.\.1000"):
            solver.solve_vrp_lsf_batch([good], rounds=rounds)
    with pytest.raises(ValueError, match=r"^request 1: lsf \(local search\) supports 1\.\.64 vehicles "
                                         r"\(65 given\)"):
        solver.solve_vrp_lsf_batch([good, (good[0], good[1], [1] * 65, [0] * 65)])
    hours = request((6, 2, 24, 0, ""))
    with pytest.raises(ValueError, match=r'^request 1: lsf .* static duration matrix \(24 slices '
                                         r'given\); an hour-indexed request keeps "lsr"'):
        solver.solve_vrp_lsf_batch([good, hours])
    with pytest.raises(ValueError, match=r'static duration matrix .* keeps "lsr"'):
        solver.solve_vrp("lsf", *hours)
    Nbig = DOMAIN[(4, False)] + 1
    bigD = np.ones((Nbig, Nbig), dtype=np.int64).tolist()
    need = lds_bytes(Nbig, 4, False)
    with pytest.raises(ValueError, match=rf"^request 0: lsf .* need {need} bytes; the limit is "
                                         rf"{LDS_BYTES} bytes"):
        solver.solve_vrp_lsf_batch([(bigD, _locs([0] + [1] * (Nbig - 1)), [Nbig] * 4, [0] * 4)])
    # no customer: solve_vrp's trivial answer, built on the host
    none = (good[0], good[1], [3, 3], [0, 7], [1, 2, 3, 4, 5, 6])
    trivial = {"durationMax": 0, "durationSum": 0, "unvisited": [],
               "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    assert solver.solve_vrp_lsf_batch([none], with_unvisited=True) == [trivial]
    assert solver.solve_vrp("lsf", *none, with_unvisited=True) == trivial
    # solve_tsp, and solve_vrp's knobs
    assert "lsf" in solver.ALGORITHMS
    D, locs, caps, starts = good
    with pytest.raises(ValueError, match="lsf solves the VRP only"):
        solver.solve_tsp("lsf", D, [1, 2, 3], 0, 0)
    with pytest.raises(ValueError, match=r"lsf .* 1\.\.64 vehicles \(65 given\)"):
        solver.solve_vrp("lsf", D, locs, [1] * 65, [0] * 65)
    with pytest.raises(ValueError, match=r"1\.\.1024 starts \(1025 given\)"):
        solver.solve_vrp("lsf", D, locs, caps, starts, starts=1025)
    with pytest.raises(ValueError, match=r"0\.\.1000 rounds \(1001 given\)"):
        solver.solve_vrp("lsf", D, locs, caps, starts, rounds=1001)
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp("lsf", D, locs, caps, starts, objective="mean")
    # with a fake launch in the module's place the batch groups by key and the
    # one-request path takes the knobs
    seen = []

    def fake(ctx, cis, starts, rounds, seed, objective="sum"):
        seen.append((len(cis), starts, rounds, seed, objective))
        return ([list(range(ci.n, 0, -1)) + [0] * (len(ci.capacities) - 1) for ci in cis],
                [[0] * ci.n + [-2] * (len(ci.capacities) - 1) for ci in cis],
                [[10 * ci.n] + [0] * (len(ci.capacities) - 1) for ci in cis])

    monkeypatch.setattr(solver, "batch_lsf_launch", fake)
    monkeypatch.setattr(solver, "context", lambda device=0: None)
    out = solver.solve_vrp_lsf_batch([good, request((6, 2, 1, 1, "")), request((7, 2, 1, 2, "")), none],
                                     starts=5, rounds=6, seed=7, objective="max")
    assert sorted(seen) == [(1, 5, 6, 7, "max"), (2, 5, 6, 7, "max")]
    assert out[0]["vehicles"][0] == {"tour": [0, 6, 5, 4, 3, 2, 1, 0], "duration": 60}
    assert out[3]["durationSum"] == 0
    del seen[:]
    one = solver.solve_vrp("lsf", *good, starts=3, rounds=4, seed=9)
    assert seen == [(1, 3, 4, 9, "sum")] and one["durationSum"] == 60


def test_app_batch_vrp_lsf_routes_and_cli_flags(monkeypatch, capsys, lib):
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, len(params["capacities"]), dict(knobs.get("inline") or {})))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    assert "lsf" in service.INLINE_ALGORITHMS["vrp"] and "lsf" not in service.INLINE_ALGORITHMS["tsp"]
    assert service.INLINE_ALGORITHMS["vrp"][-1] == "sp" and "lsf" not in service.TITLES
    off = service.App(service.MemoryStore({}, {}, {}), solve=fake)
    assert off.vrp_lsf_batcher is None
    assert off.solve_inline("vrp", "lsf", _body((5, 2, 1, 0, "")))[1]["message"]["durationSum"] == 3
    assert seen == [("vrp", "lsf", 2, {})]
    del seen[:]
    st, res = off.solve_inline("tsp", "lsf", b"{}")
    assert st == 400 and "no solver /solve/tsp/lsf" in res["errors"][0]["reason"]

    app = service.App(service.MemoryStore({}, {}, {}), solve=fake, batch_vrp_lsf=True,
                      batch_window_s=0.2, batch_vrp_lsf_launch=_fake_launch(launched),
                      batch_lsf_starts=16, batch_lsf_rounds=7)
    assert isinstance(app.vrp_lsf_batcher, service.VrpLsfBatcher)
    assert (app.vrp_lsf_batcher.starts, app.vrp_lsf_batcher.rounds) == (16, 7)
    assert app.vrp_lsr_batcher is None and app.vrp_ls_batcher is None

    def call(x):
        if x < 4:
            return app.solve_inline("vrp", "lsf", _body((5, 2, 1, x, ""), seed=x, timeLimit=1.0))
        if x < 6:
            return app.solve_inline("vrp", "lsf", _body((5, 2, 1, x, ""), objective="max"))
        return app.solve_inline("vrp", "lsf", _body((6, 3, 1, x, "")))

    out = _concurrently(call, 8)
    assert all(st == 200 for st, _ in out), out
    assert sorted(launched) == [((6, 2, 1, False, "max"), 2), ((6, 2, 1, False, "sum"), 4),
                                ((7, 3, 1, False, "sum"), 2)]
    assert seen == [] and app.vrp_lsf_batcher.requests == 8
    assert out[0][1]["message"]["vehicles"][0]["tour"] == [0, 5, 4, 3, 2, 1, 0]
    assert out[0][1]["message"]["vehicles"][1]["tour"] == [0, 0]

    def unbatched(status_and_result, K=2, algorithm="lsf", inline=None):
        assert status_and_result[0] == 200, status_and_result
        assert seen == [("vrp", algorithm, K, inline or {})]
        del seen[:]

    body = functools.partial(_body, (5, 2, 1, 1, ""))
    unbatched(app.solve_inline("vrp", "lsf", body(knobs={"starts": 8})), inline={"starts": 8})
    unbatched(app.solve_inline("vrp", "lsf", body(knobs={"rounds": 0})), inline={"rounds": 0})
    unbatched(app.solve_inline("vrp", "lsf", _body((5, 2, 24, 1, ""))))               # hour-indexed
    unbatched(app.solve_inline("vrp", "lsr", body()), algorithm="lsr")                # another algorithm
    assert len(launched) == 3
    for knobs in ({"starts": 0}, {"starts": 1025}, {"rounds": -1}, {"rounds": 1001}):
        st, res = app.solve_inline("vrp", "lsf", body(knobs=knobs))
        assert st == 400 and "outside" in res["errors"][0]["reason"], res
    # on the real unbatched path an hour-indexed request is a 400 naming "lsr"
    _no_gpu(monkeypatch)
    real = service.App(service.MemoryStore({}, {}, {}), batch_vrp_lsf=True, batch_window_s=0.2,
                       batch_vrp_lsf_launch=_fake_launch(launched))
    st, res = real.solve_inline("vrp", "lsf", _body((5, 2, 24, 1, "")))
    assert st == 400 and 'keeps "lsr"' in res["errors"][0]["reason"], res
    assert len(launched) == 3

    # the command line
    made = {}

    class Stop(Exception):
        pass

    def stop(store, **kw):
        made.update(kw)
        raise Stop

    monkeypatch.setattr(service, "App", stop)
    for argv, want in ((["--batch-vrp-lsf"], (True, 64, 1000)), ([], (False, 64, 1000)),
                       (["--batch-vrp-lsf", "--batch-lsf-starts", "1024", "--batch-lsf-rounds", "0"],
                        (True, 1024, 0))):
        with pytest.raises(Stop):
            service.main(argv)
        assert (made["batch_vrp_lsf"], made["batch_lsf_starts"], made["batch_lsf_rounds"]) == want
        assert made["batch_vrp_lsr"] is False
    for argv in (["--batch-lsf-starts", "0"], ["--batch-lsf-starts", "1025"],
                 ["--batch-lsf-rounds", "-1"], ["--batch-lsf-rounds", "1001"]):
        with pytest.raises(SystemExit):
            service.main(argv)
    capsys.readouterr()


def _trajectory_leaves_plain(run, objective):
    """Whether A26's descents of the run apply a move onto a tour that is not
    plain, starting from a plain one."""
    _, dem, caps, _ = inst(run[0])
    r = reference26(run, objective)
    took = iter(r["moves"])
    for t, applied in zip(r["first"], r["rounds"]):
        was = is_plain(t, dem, caps)
        for _ in range(applied):
            t = spec.apply_move(t, *next(took))
            now = is_plain(t, dem, caps)
            if was and not now:
                return True
            was = now
    return False


def test_reference_properties():
    """What the GPU comparisons rely on, checked on the reference itself."""
    refs = {(run, o): reference(run, o) for run in ALL_RUNS for o in OBJECTIVES}
    for (run, o), r in refs.items():
        D, dem, caps, starts = inst(run[0])
        n, K = run[0][:2]
        L = n + K - 1
        assert len(r["tour"]) == L and r["tour"].count(0) == K - 1
        assert [is_plain(t, dem, caps) for t in r["first"]] == r["plain"]
        assert plain_mask(r["first"], dem, caps).tolist() == r["plain"]
        for (k, s, t), applied in zip(r["ends"], r["rounds"]):
            e = spec.eval_cvrp(D, t, dem, list(caps), list(starts), obj_id(o))
            assert e["key"] == k
            if not r["plain"][s]:
                assert t == r["first"][s] and applied == 0
                continue
            # every end tour of a plain start is plain: nobody unvisited, and
            # every customer on the vehicle its separators give it
            assert is_plain(t, dem, caps) and e["unvisited"] == 0
            seps = 0
            for c, v in zip(t, e["vehicle_of"]):
                assert v == (-2 if c == 0 else seps)
                seps += c == 0
            if L >= 2 and applied < run[2]:   # uncapped: no plain move has a lower key
                cands = [spec.apply_move(t, *m) for m in all_moves(L)]
                ok = plain_mask(cands, dem, caps)
                keys = spec.eval_cvrp_batch(D, cands, dem, list(caps), list(starts), obj_id(o))[0]
                assert all(int(x) >= k for x, good in zip(keys, ok) if good), (run, o, s)
        assert r["capped"] == sum(1 for s, a in enumerate(r["rounds"])
                                  if L >= 2 and r["plain"][s] and a >= run[2])
    # all-roomy copies: A28 is A26 field for field
    for case, S, rounds in (((8, 3, 1, 9, "allroomy"), 7, 1000), ((12, 4, 1, 41, "allroomy"), 6, 1000),
                            ((7, 2, 1, 3, "allroomy"), 12, 2)):
        for o in OBJECTIVES:
            a, b = reference((case, S, rounds), o), reference26((case, S, rounds), o)
            assert all(a["plain"])
            for f in ROW + ("rounds", "moves", "first", "unvisited"):
                assert a[f] == b[f], (case, o, f)
    # a kernel that skips the filter fails: A26 steps onto a tour that is not
    # plain, and its row is another
    leaves = [run for run in ALL_RUNS
              if any(_trajectory_leaves_plain(run, o) and
                     any(refs[(run, o)][f] != reference26(run, o)[f] for f in ROW) for o in OBJECTIVES)]
    assert len(leaves) >= 4, leaves
    for case in ((2, 3, 1, 2, ""), (7, 3, 1, 7, ""), (9, 3, 1, 14, "zerodem"), (7, 3, 1, 31, "e65536"),
                 (12, 4, 1, 41, "")):
        assert any(run[0] == case for run in leaves), case
    # starts that are not plain: some in two runs at least, all of them in one
    some = [run for run in ALL_RUNS if not all(refs[(run, "sum")]["plain"])]
    assert len(some) >= 2
    assert refs[(ONE_PLAIN_SHORT[0], "sum")]["plain"].count(False) == 1
    every = [run for run in some if not any(refs[(run, "sum")]["plain"])]
    assert {run[0][0] for run in every if run in N_EDGES} >= {3, 8}
    for run in every:
        r = refs[(run, "sum")]
        assert r["capped"] == 0 and r["rounds"] == [0] * run[1] and r["s"] == min(
            range(run[1]), key=lambda s: (r["ends"][s][0], s))
    # the heavy runs: a total demand of 2^32 and more with every start plain and
    # moves applied; customers that fit nowhere and a last route past 2^32
    for run in HEAVY:
        _, dem, caps, _ = inst(run[0])
        r = refs[(run, "sum")]
        assert sum(int(d) for d in dem) >= 2**32 and int(max(caps)) + int(dem.max()) < 2**31
        if run[0][4] == "heavy":
            assert all(r["plain"]) and sum(r["rounds"]) > 0
        else:
            assert not any(r["plain"]) and r["unvisited"] == 5 and r["capped"] == 0
    # the token ranges of the lane edges, the long run's chunks, K = 64 and K = 1
    assert [run[0][0] + run[0][1] - 1 for run in WAVES] == [32, 33, 63, 64, 65]
    assert LONG[0][0][0] + LONG[0][0][1] - 1 == 136 and refs[(LONG[0], "sum")]["plain"] == [True]
    assert all(refs[(LONG[0], o)]["rounds"] == [2] for o in OBJECTIVES)
    # all three move types are applied, and both objectives give different rows somewhere
    assert {typ for r in refs.values() for typ, _, _ in r["moves"]} == {0, 1, 2}
    assert any(refs[(run, "sum")]["tour"] != refs[(run, "max")]["tour"] for run in ALL_RUNS)
    # rounds: 0 caps the plain starts only
    r0 = refs[(R_EDGES[0], "sum")]
    assert r0["capped"] == sum(r0["plain"]) and r0["rounds"] == [0] * 7


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


def _lists(out):
    tours, keys, durs, veh, info = out
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), veh.cpu().tolist(), info.cpu().tolist())


def gpu_batch(ctx, cases, objective, S, rounds, wide=None, kernel="vrp_batch_lsf"):
    """One launch -> ([key], [tour], [durs], [veh], [info])."""
    return _lists(getattr(ctx, kernel)(*gpu_args(ctx, cases), obj_id(objective), S, rounds, SEED,
                                       wide=wide))


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


ROOMY = [((20, 4, 1, 61, "allroomy"), 8, 1000), ((50, 8, 1, 62, "allroomy"), 8, 1000),
         ((12, 64, 1, 63, "allroomy"), 8, 1000), ((133, 4, 1, 336, "allroomy"), 1, 2),
         ((9, 3, 1, 14, "allroomy"), 8, 1000), ((62, 4, 1, 145, "allroomy"), 5, 3),
         ((7, 2, 1, 3, "allroomy"), 12, 1000)]


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", ROOMY, ids=lambda r: "n%d-K%d-S%d-r%d" % (*r[0][:2], *r[1:]))
def test_gpu_all_roomy_is_vrp_batch_lsr(ctx, run, objective):
    """Equivalence (a), no oracle involved: every capacity carries the total
    demand, every tour is plain, and keys (with the secondary field), tours,
    durations, vehicle rows and info rows are A26's, for any K."""
    case, S, rounds = run
    got = gpu_batch(ctx, [case], objective, S, rounds)
    want = gpu_batch(ctx, [case], objective, S, rounds, kernel="vrp_batch_lsr")
    print(run, objective, "lsf", got[0], got[4], "lsr", want[0], want[4])
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_one_roomy_vehicle_is_vrp_batch_ls(ctx, objective):
    """Equivalence (b), no oracle involved: K = 1 and a capacity of the total
    demand give A25's rows."""
    import torch
    for case, S, rounds in (((12, 1, 1, 12, "allroomy"), 64, 1000), ((65, 1, 1, 145, "allroomy"), 5, 2),
                            ((1, 1, 1, 1, "allroomy"), 5, 0), ((8, 1, 1, 9, "allroomy"), 7, 1)):
        args = gpu_args(ctx, [case]) + (obj_id(objective), S, rounds, SEED)
        ls = ctx.vrp_batch_ls(*args)
        lsf = ctx.vrp_batch_lsf(*args)
        for x in range(5):
            assert torch.equal(ls[x], lsf[x]), (case, S, rounds, x)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_no_round_is_vrp_batch_lsr(ctx, objective):
    """Equivalence (c): at rounds = 0 the keys, tours, durations, vehicle rows
    and winning starts are A26's for the family's capacities, with no oracle
    involved.  A26 caps every start there (L >= 2); A28 caps the plain ones
    only, so its count is the number of plain start tours -- counted on the
    host from the shuffles, pinned by hand where it is known."""
    for case, S, known in (((8, 3, 1, 9, ""), 7, None), ((3, 3, 1, 3, ""), 6, 0),
                           ((8, 3, 1, 8, ""), 6, 0), ((12, 4, 1, 41, ""), 6, 5),
                           ((133, 4, 1, 336, ""), 4, None), ((9, 3, 1, 14, "allroomy"), 9, 9),
                           ((3, 64, 1, 12, ""), 4, None), ((1, 1, 1, 1, ""), 5, 0),
                           ((8, 4, 1, 5, "heavy"), 6, 6), ((9, 3, 1, 6, "nofit"), 6, 0)):
        got = gpu_batch(ctx, [case], objective, S, 0)
        want = gpu_batch(ctx, [case], objective, S, 0, kernel="vrp_batch_lsr")
        assert got[:4] == want[:4], case
        L = case[0] + case[1] - 1
        plain = sum(reference((case, S, 0), objective)["plain"]) if L >= 2 else 0
        assert got[4][0] == [want[4][0][0], plain] and plain <= want[4][0][1], case
        if known is not None:
            assert plain == known, case


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_staging_width_and_refusals(ctx, objective):
    """Both instantiations, uint16 and int32, the refusal row between two
    healthy requests, and the cell 0 -> 0, which prices nothing."""
    import torch
    S, rounds = 6, 1000
    a, b, c = (7, 3, 1, 30, ""), (7, 3, 1, 31, "e65535"), (7, 3, 1, 32, "")
    over = (7, 3, 1, 31, "e65536")

    def runs(*cases):
        return [(x, S, rounds) for x in cases]

    assert gpu_runs(ctx, runs(a, b, c), objective, wide=False) == expected(runs(a, b, c), objective)
    assert gpu_runs(ctx, runs(a, over, c), objective, wide=True) == expected(runs(a, over, c), objective)
    assert gpu_runs(ctx, runs(over), objective) == expected(runs(over), objective)   # wide=None
    want = expected(runs(a, over, c), objective)
    keys, tours, durs, veh, info = gpu_runs(ctx, runs(a, over, c), objective, wide=False)
    assert keys[1] == 2**64 - 1 and tours[1] == [0] * 9 and durs[1] == [0] * 3 and \
        veh[1] == [-1] * 9 and info[1] == [-1, 0]
    for x in (0, 2):
        assert (keys[x], tours[x], durs[x], veh[x], info[x]) == tuple(w[x] for w in want)
    insts = [inst(x) for x in (a, b, c)]
    args = gpu_args(ctx, (a, b, c))
    want = expected(runs(a, b, c), objective)

    def launch(mats, wide):
        return _lists(ctx.vrp_batch_lsf(torch.tensor(mats, dtype=torch.int32, device=ctx.dev), *args[1:],
                                        obj_id(objective), S, rounds, SEED, wide=wide))

    for at, value in (((1, 0, 3, 2), -1), ((1, 0, 0, 0), -1)):   # a negative entry, also at 0 -> 0
        mats = np.stack([D for D, _, _, _ in insts]).astype(np.int32)
        mats[at] = value
        for wide in (False, True):
            keys, tours, durs, veh, info = launch(mats, wide)
            assert keys[1] == 2**64 - 1 and tours[1] == [0] * 9 and durs[1] == [0] * 3 and \
                veh[1] == [-1] * 9 and info[1] == [-1, 0]
            for x in (0, 2):
                assert (keys[x], tours[x], durs[x], veh[x], info[x]) == tuple(w[x] for w in want)
    # a positive 0 -> 0 changes nothing; above 65535 it is refused under uint16 only
    mats = np.stack([D for D, _, _, _ in insts]).astype(np.int32)
    mats[:, 0, 0, 0] = (77, 65535, 1)
    assert launch(mats, False) == want and launch(mats, True) == want
    mats[1, 0, 0, 0] = 65536
    assert launch(mats, True) == want
    keys, tours, durs, veh, info = launch(mats, False)
    assert keys[1] == 2**64 - 1 and info[1] == [-1, 0]
    assert (keys[0], keys[2], tours[0], tours[2]) == (want[0][0], want[0][2], want[1][0], want[1][2])


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
    case, S, rounds = SIX[0]
    row = tuple(g[0] for g in together)
    for R, at in ((1, 0), (2, 1), (301, 300)):
        cases = [SIX[1 + x % 5][0] for x in range(R)]
        cases[at] = case
        got = gpu_batch(ctx, cases, objective, S, rounds)
        assert tuple(g[at] for g in got) == row, (R, at)
    z = [torch.zeros(shape, dtype=torch.int32, device=ctx.dev)
         for shape in ((0, 1, 11, 11), (0, 11), (0, 3), (0, 3))]
    out = ctx.vrp_batch_lsf(*z, obj_id(objective), 8, 5, SEED)
    assert [tuple(t.shape) for t in out] == [(0, 12), (0,), (0, 3), (0, 12), (0, 2)]
    # an hour-indexed batch is refused at the entry point
    hours = [torch.ones(shape, dtype=torch.int32, device=ctx.dev)
             for shape in ((1, 24, 6, 6), (1, 6), (1, 2), (1, 2))]
    with pytest.raises(_lib.VrpmsError, match=r"vrpms_vrp_batch_lsf: H must be 1 \(24 given\)"):
        ctx.vrp_batch_lsf(*hours, obj_id(objective), 8, 5, SEED)


@pytest.mark.gpu
def test_gpu_lds_edge(ctx):
    """The largest N of the domain table launches -- all-roomy, so that A26's
    kernel, which fits more, says what the row is -- and N + 1 is refused
    with the byte count."""
    import torch
    lib, K, R = ctx.lib, 4, 2
    N = DOMAIN[(K, False)]
    cases = [(N - 1, K, 1, 40 + x, "allroomy") for x in range(R)]
    for objective in OBJECTIVES:
        assert gpu_batch(ctx, cases, objective, 2, 1) == \
            gpu_batch(ctx, cases, objective, 2, 1, kernel="vrp_batch_lsr")
    N += 1
    L = N - 1 + K - 1
    M = torch.ones((R, 1, N, N), dtype=torch.int32, device=ctx.dev)
    dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
    cp = torch.ones((R, K), dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R, L), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R, K), -7, dtype=torch.int32, device=ctx.dev)
    veh = torch.full((R, L), -7, dtype=torch.int8, device=ctx.dev)
    info = torch.full((R, 2), -7, dtype=torch.int32, device=ctx.dev)
    rc = lib.vrpms_vrp_batch_lsf(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(), cp.data_ptr(),
                                 R, N, K, 1, 0, 0, 4, 1, SEED, tours.data_ptr(), keys.data_ptr(),
                                 durs.data_ptr(), veh.data_ptr(), info.data_ptr(), ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_lsf:" in msg and b"bytes of LDS" in msg
    assert str(lds_bytes(N, K, False)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item()
    assert (durs == -7).all().item() and (veh == -7).all().item() and (info == -7).all().item()


def _score(res):
    return (len(res["unvisited"]), res["durationSum"])


@pytest.mark.gpu
def test_never_below_the_exact_solver():
    """A condition, not a quality bar: on 200 static requests of (8, 3) no
    answer beats the optimum's (unvisited, durationSum), and every answer's
    durations are what spec.eval_cvrp gives its routes."""
    reqs = [request((8, 3, 1, 500 + x, "")) for x in range(200)]
    exact = solver.solve_vrp_batch("sp", reqs, with_unvisited=True)
    got = solver.solve_vrp_lsf_batch(reqs, starts=16, rounds=1000, seed=SEED, with_unvisited=True)
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


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_lsf_batch_and_solve_vrp_mixed_list(objective):
    S, rounds = 8, 1000
    D7, locs7, caps7, starts7 = request((6, 2, 1, 50, ""), 100)
    inside = {0: (6, 2, 1, 51, ""), 1: (9, 3, 1, 52, ""), 3: (6, 2, 1, 53, ""), 5: (9, 3, 1, 54, "")}
    reqs = [request(inside[0]), request(inside[1]),
            (D7, locs7, caps7, starts7, [100 + i for i in range(1, 7)]),            # none active
            request(inside[3]),
            {"durations": D7, "locations": locs7, "capacities": caps7, "start_times": starts7,
             "ignored_customers": [103]},
            request(inside[5])]
    kw = dict(starts=S, rounds=rounds, seed=SEED, objective=objective, with_unvisited=True)
    got = solver.solve_vrp_lsf_batch(reqs, **kw)
    assert got[2] == {"durationMax": 0, "durationSum": 0, "unvisited": [],
                      "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    for r, res in zip(reqs, got):
        if isinstance(r, dict):
            r = (r["durations"], r["locations"], r["capacities"], r["start_times"],
                 r["ignored_customers"])
        _rescored(r, res, objective)
    for x, case in inside.items():
        assert got[x] == _ref_dict(case, objective, S, rounds)
        assert solver.solve_vrp("lsf", *reqs[x], **kw) == got[x]
    r4 = reqs[4]
    assert solver.solve_vrp("lsf", r4["durations"], r4["locations"], r4["capacities"],
                            r4["start_times"], r4["ignored_customers"], **kw) == got[4]
    assert solver.solve_vrp_lsf_batch(reqs, **kw) == got
    for x in (0, 1, 4):
        assert solver.solve_vrp_lsf_batch([reqs[x]], **kw) == [got[x]]
    assert "unvisited" not in solver.solve_vrp_lsf_batch([reqs[0]], starts=S, seed=SEED)[0]
    assert "unvisited" not in solver.solve_vrp("lsf", *reqs[0], starts=S, seed=SEED)


@pytest.mark.gpu
def test_service_batch_vrp_lsf_over_http_equals_solve_vrp_lsf_batch():
    S, rounds = 8, 1000
    app = service.App(service.MemoryStore({}, {}, {}), seed=SEED, batch_vrp_lsf=True,
                      batch_window_s=0.05, batch_lsf_starts=S, batch_lsf_rounds=rounds)
    srv = service.serve(app, "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    cases = [((6, 2, 1, 60 + x, "") if x % 2 else (9, 3, 1, 52 + x, "")) for x in range(8)]
    try:
        def call(x):
            req = urllib.request.Request(f"http://127.0.0.1:{srv.server_address[1]}/solve/vrp/lsf",
                                         data=_body(cases[x]), method="POST")
            with urllib.request.urlopen(req, timeout=120) as resp:
                return resp.status, json.loads(resp.read())

        out = _concurrently(call, len(cases))
        req = urllib.request.Request(f"http://127.0.0.1:{srv.server_address[1]}/solve/vrp/lsf",
                                     data=_body(cases[0], knobs={"starts": 3}, seed=SEED),
                                     method="POST")
        with urllib.request.urlopen(req, timeout=120) as resp:
            inline = json.loads(resp.read())
    finally:
        srv.shutdown()
        srv.server_close()
        th.join()
    b = app.vrp_lsf_batcher
    assert b.requests == 8 and 2 <= b.launches < b.requests
    for x, res in enumerate(out):
        assert not isinstance(res, Exception), res
        assert res[0] == 200 and res[1]["success"], res
        assert [res[1]["message"]] == solver.solve_vrp_lsf_batch([request(cases[x], 100)], starts=S,
                                                                 rounds=rounds, seed=SEED)
    want = _ref_dict(cases[0], "sum", S, rounds)
    assert out[0][1]["message"] == {k: v for k, v in want.items() if k != "unvisited"}
    assert [inline["message"]] == solver.solve_vrp_lsf_batch([request(cases[0], 100)], starts=3,
                                                             rounds=1000, seed=SEED)
