"""Batched VRP GA (spec A23): the C entry points vrpms_vrp_batch_ga_lds /
vrpms_vrp_batch_ga, Context.vrp_batch_ga, solver.batch_ga_key / batch_ga_fits /
solve_vrp_ga_batch and the service's VRP GA batcher (App(batch_vrp_ga=True)).

The reference is a23_ref below: the Philox Fisher-Yates start, G calls of
oracle.search.ga_generation with an oracle.search.Scorer on island 0, the least
(key, index), and spec.eval_cvrp for the durations and vehicles.  Per request
the GPU must return the identical key, tour, route durations and vehicle row,
for both objectives."""
import ctypes
import functools
import json
import threading

import numpy as np
import pytest

from oracle import spec
from oracle.search import Scorer, ga_generation
from vrpms_amd import _lib, core, service, solver

LDS_BYTES = 160 * 1024
OBJECTIVES = ("sum", "max")
SEED = 20231
M32 = 0xFFFFFFFF


def obj_id(objective):
    return spec.OBJ_SUM if objective == "sum" else spec.OBJ_MAX


def pmut_word(pmut):
    return min(int(round(float(pmut) * 2**32)), 2**32 - 1)


# ---------------------------------------------------------------------------
# instances and their references (computed once, shared, never changed)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inst(case):
    """case = (n, K, H, seed, variant) -> (D int64 [H][N][N], demand [N], caps,
    starts), the inputs of tests/test_vrp_batch_sa.py: entries 1..89 (0 on the
    diagonal), demands 1..9, K unequal capacities around an even share of the
    total demand (so some fleets leave customers unvisited), start times in
    0..1439.  Variants:
      "below"     every capacity below every demand (all unvisited)
      "hours"     entries 20..89 and start times 59, 60, 1439, 23*60+50 cycled
      "e65535" / "e65536"  one entry of that value (hour 0, edge 1 -> 2)
      "zerocap"   a zero capacity in the middle of the fleet
      "zerodem"   a zero-demand customer"""
    n, K, H, seed, variant = case
    N = n + 1
    rng = np.random.default_rng(7000 + 131 * seed + 17 * n + K)
    lo = 20 if variant == "hours" else 1
    D = rng.integers(lo, 90, size=(H, N, N), dtype=np.int64)
    for h in range(H):
        np.fill_diagonal(D[h], 0)
    dem = rng.integers(1, 10, size=N, dtype=np.int64)
    dem[0] = 0
    share = int(dem.sum()) // K
    caps = rng.integers(max(0, share - 2), share + 6, size=K).tolist()
    starts = rng.integers(0, 1440, size=K).tolist()
    if variant == "below":
        caps = [0] * K
    elif variant == "hours":
        starts = [(59, 60, 1439, 23 * 60 + 50)[(k + seed) % 4] for k in range(K)]
    elif variant in ("e65535", "e65536"):
        D[0, 1, 2] = int(variant[1:])
    elif variant == "zerocap":
        caps[K // 2] = 0
    elif variant == "zerodem":
        dem[1 + n // 2] = 0
    else:
        assert variant == "", variant
    D.setflags(write=False)
    dem.setflags(write=False)
    return D, dem, tuple(int(c) for c in caps), tuple(int(s) for s in starts)


def a23_ref(D, dem, caps, starts, objective, P, G, pmut, seed):
    """Spec A23 -> dict(key, tour, durs, veh, unvisited, tie)."""
    D = spec.as_3d(D)
    n = D.shape[1] - 1
    skey = spec.seed_key(seed)
    score = Scorer(D, dem, list(caps), list(starts), objective=obj_id(objective))
    pop = []
    for i in range(P):
        t = list(range(1, n + 1))
        for q in range(n - 1, 0, -1):
            j = spec.philox4x32_10((M32, M32, i, q), skey)[0] % (q + 1)
            t[q], t[j] = t[j], t[q]
        pop.append(t)
    keys = [score(t) for t in pop]
    tie = False
    for g in range(G):
        pops, kk = ga_generation(score, [pop], [keys], seed, g, pmut_word(pmut))
        pop, keys = pops[0], kk[0]
        assert keys == sorted(keys)
        tie |= len(set(keys)) < len(keys)
    best = min(range(P), key=lambda i: (keys[i], i))
    final = spec.eval_cvrp(D, pop[best], dem, list(caps), list(starts), obj_id(objective))
    assert final["key"] == keys[best]
    return dict(key=keys[best], tour=pop[best], durs=final["durations"], veh=final["vehicle_of"],
                unvisited=final["unvisited"], tie=tie)


def breeding(n, P, G, pmut, seed):
    """What the Philox blocks of a run decide whatever the population holds:
    the move types of the mutated children, whether a child has lo == hi, and
    whether one takes the whole of parent A."""
    skey = spec.seed_key(seed)
    types, point, whole = set(), False, False
    for g in range(G if n >= 2 else 0):
        for c in range(P):
            r = spec.philox4x32_10((g, 0, c, 0), skey)
            r2 = spec.philox4x32_10((g, 0, c, 1), skey)
            lo, hi = sorted((r2[0] % n, r2[1] % n))
            point |= lo == hi
            whole |= (lo, hi) == (0, n - 1)
            if r2[2] < pmut_word(pmut):
                types.add(spec.decode_move(r2[3], r[0] ^ r2[0], r[1] ^ r2[1], n)[0])
    return types, point, whole


@functools.lru_cache(maxsize=None)
def reference(run, objective):
    """run = (case, P, G, pmut)."""
    case, P, G, pmut = run
    return a23_ref(*inst(case), objective, P, G, pmut, SEED)


def expected(runs, objective):
    refs = [reference(r, objective) for r in runs]
    return ([r["key"] for r in refs], [r["tour"] for r in refs], [r["durs"] for r in refs],
            [r["veh"] for r in refs])


def lds_bytes(N, K, H, wide, P):
    """DESIGN.md §4.3n restated: the matrix padded to 16 bytes, the demand row
    and the two fleet rows as int32 padded to four words, M = the next power
    of two >= 2P sort pairs of 8 + 4 bytes, 2P keys, four `used` bitmaps of
    ceil(N / 32) words padded to four, 2P uint16 rows of an odd number of
    words, and the two slot -> row maps."""
    def pad(x, m):
        return (x + m - 1) // m * m
    M = 2
    while M < 2 * P:
        M *= 2
    n = N - 1
    rs = 2 * (((n + 1) // 2) | 1)
    return pad(H * N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + 12 * M + \
        2 * 8 * P + 4 * 4 * pad((N + 31) // 32, 4) + 2 * P * 2 * rs + 2 * 2 * P


def largest_n_nodes(K, H, wide, P):
    return max(N for N in range(2, 400) if lds_bytes(N, K, H, wide, P) <= LDS_BYTES)


# DESIGN.md §4.3n's domain table (K = 4): (H, wide, P) -> the largest N
DOMAIN = {(24, False, 64): 55, (24, False, 256): 46, (24, True, 64): 39, (24, True, 256): 34,
          (1, False, 64): 225, (1, False, 256): 119, (1, True, 64): 170, (1, True, 256): 104}

# the runs of the GPU comparisons: (case, P, G, pmut)
N_EDGES = [((n, 3, 1, n, ""), 64, 3, 0.2) for n in (1, 2, 3, 63, 64, 65)] + \
          [((1, 2, 24, 2, "below"), 5, 2, 0.2)]
P_EDGES = [((9, 3, 24, 70, ""), P, 3, 0.2) for P in (2, 3, 63, 64, 65, 255, 256)]
G_EDGES = [((8, 3, 1, 9, ""), 20, G, 0.2) for G in (0, 1, 2, 7)]
PMUTS = [((8, 3, 24, 71, ""), 20, 4, pm) for pm in (0.0, 1.0)]
SKETCH = [((3, 2, 24, 72, ""), 64, 4, 0.2)]            # with P_EDGES' P = 256: the issue's two shapes
HOURS = [((6, 3, 24, s, "hours"), 32, 4, 0.2) for s in (10, 11)]
FLEETS = [((3, 64, 1, 12, ""), 16, 3, 0.2), ((9, 5, 24, 13, "zerocap"), 32, 3, 0.2),
          ((9, 3, 1, 14, "zerodem"), 32, 3, 0.2), ((6, 3, 24, 73, "below"), 16, 3, 0.2)]
# more than 63 customers breed by another mapping (a wavefront per child): its
# wave boundaries, sort padding and the three mutation branches again
WAVES = [((64, 4, 1, 74, ""), P, 2, 0.2) for P in (3, 65, 255, 256)] + \
        [((70, 4, 1, 75, ""), 24, 3, 1.0), ((66, 3, 1, 76, ""), 16, 2, 0.2)]
ALL_RUNS = N_EDGES + P_EDGES + G_EDGES + PMUTS + SKETCH + HOURS + FLEETS + WAVES
SIX = [((10, 3, 24, 20 + x, ""), 48, 3, 0.2) for x in range(6)]


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
    f = lib.vrpms_vrp_batch_ga_lds
    Ps = (2, 3, 63, 64, 65, 128, 129, 255, 256)
    for H in (1, 24):
        for wide in (0, 1):
            for K in (1, 4, 5, 64):
                for x, P in enumerate(Ps):
                    for N in list(range(2, 70)) + [96, 97, 128, 129]:
                        assert f(N, K, H, wide, P, ctypes.byref(b)) == _lib.VRPMS_OK
                        assert b.value == lds_bytes(N, K, H, wide, P) == \
                            core.vrp_batch_ga_lds(N, K, H, wide, P)
                        if N > 2:
                            assert b.value >= lds_bytes(N - 1, K, H, wide, P)
                        if x:
                            assert b.value > lds_bytes(N, K, H, wide, Ps[x - 1])
    for args, word in (((1, 3, 1, 0, 8), b"2 <= N"), ((0, 3, 1, 0, 8), b"2 <= N"),
                       ((65536, 3, 1, 0, 8), b"2 <= N"),
                       ((5, 0, 1, 0, 8), b"1 <= K <= 64"), ((5, 65, 1, 0, 8), b"1 <= K <= 64"),
                       ((5, 3, 2, 0, 8), b"H must be 1 or 24"), ((5, 3, 0, 0, 8), b"H must be 1 or 24"),
                       ((5, 3, 1, 2, 8), b"wide"), ((5, 3, 1, -1, 8), b"wide"),
                       ((5, 3, 1, 0, 1), b"2 <= P <= 256 (1 given)"),
                       ((5, 3, 1, 0, 257), b"2 <= P <= 256 (257 given)")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_ga_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(5, 3, 1, 0, 8, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_ga_lds" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="2 <= P <= 256"):
        core.vrp_batch_ga_lds(5, 3, 1, False, 300)
    assert solver.BATCH_GA_LDS_BYTES == LDS_BYTES and solver.BATCH_GA_MAX_POP == 256


def test_argument_errors_need_no_gpu(lib):
    """Every argument check comes before the context is looked at, so a
    stand-in block of zeros serves as the non-NULL ctx here."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(4096)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    names = ("m", "d", "cp", "st", "t", "k", "du", "v")

    def f(ctx=c, R=1, N=5, K=2, H=1, obj=0, wide=0, P=8, G=3, **ptrs):
        a = {name: ptrs.get(name, p) for name in names}
        return lib.vrpms_vrp_batch_ga(ctx, a["m"], a["d"], a["cp"], a["st"], R, N, K, H, obj, wide, P,
                                      G, 12345, 5, a["t"], a["k"], a["du"], a["v"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_ga:" in msg and word in msg, (kw, msg)

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
    for P in (-1, 0, 1, 257, 4096):
        refused(b"2 <= P <= 256 (%d given)" % P, P=P)
    refused(b"G must not be negative (-1 given)", G=-1)
    for name in names:
        refused(b"NULL", **{name: None})
    refused(b"H must be 1 or 24", R=0, H=3)            # the shape checks also with R = 0
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert buf.raw == bytes(4096) and fake.raw == bytes(1 << 16)


def _no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(solver, "context", boom)
    monkeypatch.setattr(solver, "Context", boom)


def _locs(dem, base=0):
    return [{"id": base + i, "demand": int(d)} for i, d in enumerate(dem)]


def request(case, base=0):
    """The case as a solve_vrp_ga_batch tuple (H = 1 as a plain [N][N] matrix)."""
    D, dem, caps, starts = inst(case)
    return ((D[0] if D.shape[0] == 1 else D).tolist(), _locs(dem, base), list(caps), list(starts))


def compact(case):
    return solver.compact_vrp(*request(case))


def test_solve_vrp_ga_batch_refusals_need_no_gpu(monkeypatch, lib):
    _no_gpu(monkeypatch)
    good = request((6, 2, 1, 0, ""))
    assert solver.solve_vrp_ga_batch([]) == []
    with pytest.raises(ValueError, match=r"^request 1: capacities and startTimes"):
        solver.solve_vrp_ga_batch([good, (good[0], good[1], [3, 3], [0])])
    with pytest.raises(ValueError, match=r"^request 2: 5 locations but a 7-node"):
        solver.solve_vrp_ga_batch([good, good, {"durations": good[0], "locations": good[1][:5],
                                                "capacities": [3], "start_times": [0]}])
    big = np.full((7, 7), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_vrp_ga_batch([good, (big.tolist(), good[1], [3, 3], [0, 0])])
    heavy = [{"id": i, "demand": 2**30} for i in range(7)]
    with pytest.raises(ValueError, match=r"^request 0: capacity \+ demand overflows int32"):
        solver.solve_vrp_ga_batch([(good[0], heavy, [2**30, 3], [0, 0])])
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp_ga_batch([good], objective="mean")
    with pytest.raises(ValueError, match="pop"):
        solver.solve_vrp_ga_batch([good], pop=1)
    with pytest.raises(ValueError, match="gens"):
        solver.solve_vrp_ga_batch([good], gens=-1)
    with pytest.raises(ValueError, match="pmut"):
        solver.solve_vrp_ga_batch([good], pmut=1.5)
    # no customer: solve_vrp's trivial answer, built on the host
    none = (good[0], good[1], [3, 3], [0, 7], [1, 2, 3, 4, 5, 6])
    assert solver.solve_vrp_ga_batch([none], with_unvisited=True) == [
        {"durationMax": 0, "durationSum": 0, "unvisited": [],
         "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}]


def _sized(N, K, H, big=0):
    D = np.ones((H, N, N), dtype=np.int64)
    D[0, 0, 1] += big
    return solver.compact_vrp(D if H > 1 else D[0], _locs([0] + [1] * (N - 1)), [N] * K, [0] * K)


def test_batch_ga_fits_at_the_lds_edge(lib):
    for (H, wide, P), N in DOMAIN.items():
        assert largest_n_nodes(4, H, wide, P) == N, (H, wide, P, largest_n_nodes(4, H, wide, P))
        assert lds_bytes(N, 4, H, wide, P) <= LDS_BYTES < lds_bytes(N + 1, 4, H, wide, P)
        big = 70000 if wide else 0
        assert solver.batch_ga_fits(_sized(N, 4, H, big), P, 400)
        assert not solver.batch_ga_fits(_sized(N + 1, 4, H, big), P, 400)
        assert solver.batch_ga_key(_sized(N, 4, H, big), P, 400) == (N, 4, H, wide, P, 400)
    small = _sized(6, 2, 24)
    cap = solver.BATCH_GA_MAX_GENERATIONS
    assert solver.batch_ga_fits(small, 256, cap) and solver.batch_ga_fits(small, 2, 0)
    assert not solver.batch_ga_fits(small, 257, 400)
    assert not solver.batch_ga_fits(small, 1, 400)
    assert not solver.batch_ga_fits(small, 256, cap + 1)
    # a wide entry halves the cells that fit; 65535 is still narrow
    N = DOMAIN[(24, False, 256)]
    assert not solver.batch_ga_fits(_sized(N, 4, 24, 70000), 256, 400)
    assert solver.batch_ga_fits(_sized(N, 4, 24, 65534), 256, 400)
    # outside the domain whatever the size
    assert not solver.batch_ga_fits(_sized(5, 65, 1), 8, 4)
    none = solver.compact_vrp(np.ones((3, 3), dtype=np.int64), _locs([0, 1, 1]), [3], [0], [1, 2])
    assert none.n == 0 and not solver.batch_ga_fits(none, 8, 4)
    tsp = solver.compact_tsp(np.ones((4, 4), dtype=np.int64), [1, 2, 3], 0, 0)
    assert not solver.batch_ga_fits(tsp, 8, 4)
    assert service.VrpGaBatcher.accepts(small, 64, 10)
    assert not service.VrpGaBatcher.accepts(_sized(6, 2, 1, 2**29), 64, 10)       # the A9 guard
    assert solver.ga_knobs(None, None) == solver.ga_knobs(0, 0) == (256, 400)
    assert solver.ga_knobs(1, 7) == (2, 7) and solver.ga_knobs(10**6, "12") == (4096, 12)


def test_reference_properties():
    """What the GPU comparisons rely on, checked on the reference itself."""
    refs = {(run, o): reference(run, o) for run in ALL_RUNS for o in OBJECTIVES}
    # a (key, index) tie among survivors
    assert any(r["tie"] for r in refs.values())
    assert reference(SKETCH[0], "sum")["tie"] and reference(P_EDGES[-1], "sum")["tie"]
    # all three move types, a one-gene span, a span that is the whole tour
    types, point, whole = set(), False, False
    for case, P, G, pmut in ALL_RUNS:
        t, p, w = breeding(case[0], P, G, pmut, SEED)
        types |= t
        point |= p
        whole |= w
    assert types == {0, 1, 2} and point and whole
    for run in SKETCH + P_EDGES[-1:]:
        t, p, w = breeding(run[0][0], *run[1:], SEED)
        print(run, "move types", t, "lo == hi", p, "whole span", w)
        assert t == {0, 1, 2} and p and w
    assert breeding(8, 20, 4, 0.0, SEED)[0] == set()
    assert breeding(70, 24, 3, 1.0, SEED)[0] == {0, 1, 2}
    # an unvisited customer
    assert reference(N_EDGES[-1], "sum")["unvisited"] == 1
    assert reference(FLEETS[-1], "max")["unvisited"] == 6
    assert any(0 < r["unvisited"] < len(r["tour"]) for r in refs.values())
    # n = 1: every member is [1]; member 0 wins every tie
    assert reference(N_EDGES[0], "sum")["tour"] == [1]
    # the hour cases cross an hour and midnight: the static slice gives another answer
    for run in HOURS:
        D, dem, caps, starts = inst(run[0])
        r = reference(run, "sum")
        flat = spec.eval_cvrp(D[:1], r["tour"], dem, list(caps), list(starts))
        assert flat["key"] != r["key"]
        assert any(s >= 23 * 60 and s + d >= 1440 for s, d in zip(starts, r["durs"]) if d)
    # the generations do something
    a, b = reference(G_EDGES[0], "sum"), reference(G_EDGES[3], "sum")
    assert b["key"] < a["key"]


class _FakeApp:
    devices = [0]
    device = 0
    locks = {0: threading.Lock()}
    seed = 0


def _fake_launch(seen):
    """Customers in descending order on vehicle 0, the others empty."""
    def launch(key, cis):
        seen.append((key, len(cis)))
        tours, rest = [], []
        for ci in cis:
            K = len(ci.capacities)
            tours.append(list(range(ci.n, 0, -1)))
            rest.append(([0] * ci.n, [10 * ci.n] + [0] * (K - 1)))
        return tours, rest
    return launch


def _concurrently(fn, count):
    out = [None] * count

    def go(x):
        try:
            out[x] = fn(x)
        except Exception as e:   # noqa: BLE001 -- the test looks at it
            out[x] = e

    ths = [threading.Thread(target=go, args=(x,)) for x in range(count)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    return out


def _body(case, base=100, **more):
    D, locs, caps, starts = request(case, base)
    return json.dumps(dict({"durations": D, "locations": locs, "capacities": caps,
                            "startTimes": starts, "ignoredCustomers": [],
                            "completedCustomers": []}, **more)).encode()


def test_vrp_ga_batcher_groups_and_fans_out_errors(lib):
    seen = []
    b = service.VrpGaBatcher(_FakeApp(), window_s=0.2, launch=_fake_launch(seen))
    jobs = [((5, 2, 1, x, ""), "sum", 64, 10) for x in range(4)] + \
           [((5, 3, 1, 5, ""), "sum", 64, 10)] * 2 + \
           [((5, 2, 24, 8 + x, ""), "max", 64, 10) for x in range(2)] + \
           [((5, 2, 1, 10, "e65536"), "sum", 64, 10), ((5, 2, 1, 11, ""), "max", 64, 10),
            ((5, 2, 1, 12, ""), "sum", 65, 10), ((5, 2, 1, 13, ""), "sum", 64, 11)]
    out = _concurrently(lambda x: b.solve(compact(jobs[x][0]), *jobs[x][1:]), len(jobs))
    assert sorted(seen) == [((6, 2, 1, False, "max", 64, 10), 1), ((6, 2, 1, False, "sum", 64, 10), 4),
                            ((6, 2, 1, False, "sum", 64, 11), 1), ((6, 2, 1, False, "sum", 65, 10), 1),
                            ((6, 2, 1, True, "sum", 64, 10), 1), ((6, 2, 24, False, "max", 64, 10), 2),
                            ((6, 3, 1, False, "sum", 64, 10), 2)]
    assert b.launches == 7 and b.requests == 12
    for job, res in zip(jobs, out):
        K = job[0][1]
        assert res == {"durationMax": 50, "durationSum": 50,
                       "vehicles": [{"tour": [0, 5, 4, 3, 2, 1, 0], "duration": 50}] +
                                   [{"tour": [0, 0], "duration": 0}] * (K - 1)}

    def failing(key, cis):
        if key[1] == 2:
            raise RuntimeError("launch failed")
        return _fake_launch([])(key, cis)

    b = service.VrpGaBatcher(_FakeApp(), window_s=0.2, launch=failing)
    out = _concurrently(lambda x: b.solve(compact(jobs[x][0]), *jobs[x][1:]), 6)
    assert all(isinstance(o, RuntimeError) and "launch failed" in str(o) for o in out[:4])
    assert all(isinstance(o, dict) and len(o["vehicles"]) == 3 for o in out[4:])


def test_app_batch_vrp_ga_routes(lib):
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, len(params["capacities"])))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    # the flag is off: the injected solve
    off = service.App(service.MemoryStore({}, {}, {}), solve=fake)
    assert off.vrp_ga_batcher is None
    assert off.solve_inline("vrp", "ga", _body((5, 2, 1, 0, "")))[1]["message"]["durationSum"] == 3
    assert seen == [("vrp", "ga", 2)]
    del seen[:]

    D, locs, caps, starts = request((5, 2, 1, 1, ""), 100)
    store = service.MemoryStore({"7": locs}, {"8": D}, {})
    app = service.App(store, solve=fake, batch_vrp_ga=True, batch_window_s=0.2,
                      batch_vrp_ga_launch=_fake_launch(launched))
    assert isinstance(app.vrp_ga_batcher, service.VrpGaBatcher)
    assert isinstance(app.vrp_ga_batcher, service.VrpSaBatcher)
    assert app.batcher is None and app.vrp_sa_batcher is None

    def api(**more):
        return json.dumps(dict({"solutionName": "s", "solutionDescription": "d", "locationsKey": 7,
                                "durationsKey": 8, "capacities": caps, "startTimes": starts,
                                "ignoredCustomers": [103], "completedCustomers": [],
                                "multiThreaded": False, "randomPermutationCount": 32,
                                "iterationCount": 6}, **more)).encode()

    def call(x):
        if x == 0:
            return app.post("vrp", "ga", api())
        if x == 1:       # falsy knobs: solve_vrp's defaults; a junk multiThreaded decides nothing
            return app.post("vrp", "ga", api(multiThreaded="maybe", randomPermutationCount=None,
                                             iterationCount=0))
        if x == 2:       # a population below 2 is clamped
            return app.post("vrp", "ga", api(multiThreaded="false", randomPermutationCount=1))
        if x < 6:
            return app.solve_inline("vrp", "ga", _body((5, 2, 1, x, ""), randomPermutationCount=32,
                                                       iterationCount=6))
        if x < 8:
            return app.solve_inline("vrp", "ga", _body((5, 2, 1, x, ""), objective="max"))
        return app.solve_inline("vrp", "ga", _body((5, 2, 1, x, ""), randomPermutationCount=256,
                                                   iterationCount=solver.BATCH_GA_MAX_GENERATIONS))

    out = _concurrently(call, 9)
    assert all(st == 200 for st, _ in out), out
    cap = solver.BATCH_GA_MAX_GENERATIONS
    assert sorted(launched) == [((5, 2, 1, False, "sum", 2, 6), 1), ((5, 2, 1, False, "sum", 32, 6), 1),
                                ((5, 2, 1, False, "sum", 256, 400), 1),
                                ((6, 2, 1, False, "max", 256, 400), 2),
                                ((6, 2, 1, False, "sum", 32, 6), 3),
                                ((6, 2, 1, False, "sum", 256, cap), 1)]
    assert seen == [] and app.vrp_ga_batcher.requests == 9
    # location 103 (row 3) is ignored: compact customers 4..1 are rows 5, 4, 2, 1
    assert out[0][1]["message"] == {
        "durationMax": 40, "durationSum": 40,
        "vehicles": [{"tour": [0, 5, 4, 2, 1, 0], "duration": 40}, {"tour": [0, 0], "duration": 0}]}
    assert out[3][1]["message"]["vehicles"][0]["tour"] == [0, 5, 4, 3, 2, 1, 0]

    # every rule that sends a request down the unbatched path, one by one
    def unbatched(status_and_result, K=2, algorithm="ga"):
        assert status_and_result[0] == 200, status_and_result
        assert seen == [("vrp", algorithm, K)]
        del seen[:]

    body = functools.partial(_body, (5, 2, 1, 1, ""))
    unbatched(app.solve_inline("vrp", "ga", body(knobs={"pop": 64})))                 # inline knobs
    for mt in (True, "true", "TRUE", 1, "1"):
        unbatched(app.post("vrp", "ga", api(multiThreaded=mt)))                       # multiThreaded
    unbatched(app.solve_inline("vrp", "ga", body(randomPermutationCount=257)))        # pop > 256
    unbatched(app.post("vrp", "ga", api(randomPermutationCount=4096)))
    unbatched(app.solve_inline("vrp", "ga", body(iterationCount=cap + 1)))            # gens > cap
    wide_fleet = json.dumps({"durations": D, "locations": locs, "capacities": [1] * 65,
                             "startTimes": [0] * 65, "ignoredCustomers": [],
                             "completedCustomers": []}).encode()
    unbatched(app.solve_inline("vrp", "ga", wide_fleet), K=65)                        # the LDS domain
    Nbig = DOMAIN[(1, False, 256)] + 1
    bigD = np.ones((Nbig, Nbig), dtype=np.int64).tolist()
    big = json.dumps({"durations": bigD, "locations": _locs([0] + [1] * (Nbig - 1)),
                      "capacities": [Nbig] * 4, "startTimes": [0] * 4, "ignoredCustomers": [],
                      "completedCustomers": []}).encode()
    unbatched(app.solve_inline("vrp", "ga", big), K=4)
    unbatched(app.solve_inline("vrp", "sa", body()), algorithm="sa")                  # another algorithm
    assert len(launched) == 6
    # a bad instance is a 400 in solve_vrp's words
    st, res = app.solve_inline("vrp", "ga", body(startTimes=[0]))
    assert st == 400 and "capacities and startTimes" in res["errors"][0]["reason"]


def test_cli_flag(monkeypatch):
    made = {}

    class Stop(Exception):
        pass

    def app(store, **kw):
        made.update(kw)
        raise Stop

    monkeypatch.setattr(service, "App", app)
    for argv, want in ((["--batch-vrp-ga"], True), ([], False)):
        with pytest.raises(Stop):
            service.main(argv)
        assert made["batch_vrp_ga"] is want and made["batch_vrp_sa"] is False


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_batch(ctx, cases, objective, P, G, pmut, wide=None):
    """One vrp_batch_ga launch -> ([key], [tour], [durs], [veh])."""
    import torch
    insts = [inst(c) for c in cases]

    def dev(rows):
        return torch.tensor(np.stack(rows), dtype=torch.int32, device=ctx.dev)

    tours, keys, durs, veh = ctx.vrp_batch_ga(
        dev([D for D, _, _, _ in insts]), dev([d for _, d, _, _ in insts]),
        dev([np.array(c) for _, _, c, _ in insts]), dev([np.array(s) for _, _, _, s in insts]),
        obj_id(objective), P, G, pmut, SEED, wide=wide)
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), veh.cpu().tolist())


def gpu_runs(ctx, runs, objective, wide=None):
    """Runs of one (P, G, pmut) in one launch."""
    assert len({r[1:] for r in runs}) == 1 and len(runs) <= 16
    return gpu_batch(ctx, [r[0] for r in runs], objective, *runs[0][1:], wide=wide)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", ALL_RUNS, ids=lambda r: "n%d-K%d-H%d-s%d%s-P%d-G%d-pm%g" % (*r[0], *r[1:]))
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
            return [(x, 24, 3, 0.2) for x in cases]

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


@pytest.mark.gpu
def test_gpu_lds_edge(ctx):
    import torch
    lib, K, H, P, R = ctx.lib, 4, 24, 256, 2
    N = DOMAIN[(H, False, P)]
    runs = [((N - 1, K, H, 40 + x, ""), P, 1, 0.2) for x in range(R)]
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
    rc = lib.vrpms_vrp_batch_ga(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(), cp.data_ptr(),
                                R, N, K, H, 0, 0, P, 1, 0, SEED, tours.data_ptr(), keys.data_ptr(),
                                durs.data_ptr(), veh.data_ptr(), ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_ga:" in msg and b"bytes of LDS" in msg
    assert str(lds_bytes(N, K, H, False, P)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item()
    assert (durs == -7).all().item() and (veh == -7).all().item()


def _rescored(req, res, objective):
    """The dict's routes and durations under spec.eval_cvrp: every route alone
    on its vehicle gives its duration, and the unvisited are the rest."""
    ci = solver.compact_vrp(*req)
    back = {node: c for c, node in enumerate(ci.nodes)}
    assert len(res["vehicles"]) == len(ci.capacities)
    served = []
    for k, v in enumerate(res["vehicles"]):
        assert v["tour"][0] == v["tour"][-1] == ci.nodes[0]
        route = [back[c] for c in v["tour"][1:-1]]
        served += route
        e = spec.eval_cvrp(ci.durations, route, ci.demand, [ci.capacities[k]], [ci.start_times[k]])
        assert e["unvisited"] == 0 and e["durations"] == [v["duration"]]
    assert sorted(served + [back[c] for c in res["unvisited"]]) == list(range(1, ci.N))
    durs = [v["duration"] for v in res["vehicles"]]
    assert res["durationSum"] == sum(durs) and res["durationMax"] == max(durs)


def _ref_dict(case, objective, P, G, base=0):
    """The reference as solve_vrp's slot dict (nodes are matrix rows: with no
    customer left out, the compact indices)."""
    r = reference((case, P, G, 0.2), objective)
    routes = [[] for _ in r["durs"]]
    unv = []
    for c, v in zip(r["tour"], r["veh"]):
        (routes[v] if v >= 0 else unv).append(base + c)
    return {"durationMax": max(r["durs"]), "durationSum": sum(r["durs"]), "unvisited": unv,
            "vehicles": [{"tour": [base] + rt + [base], "duration": d}
                         for rt, d in zip(routes, r["durs"])]}


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_ga_batch_mixed_list(objective):
    P, G = 32, 5
    D7, locs7, caps7, starts7 = request((6, 2, 24, 50, ""), 100)
    inside = {0: (6, 2, 24, 51, ""), 1: (9, 3, 1, 52, ""), 3: (6, 2, 24, 53, ""), 6: (9, 3, 1, 54, "")}
    reqs = [request(inside[0], 100), request(inside[1], 100),
            (D7, locs7, caps7, starts7, [100 + i for i in range(1, 7)]),            # none active
            request(inside[3], 100),
            (D7, locs7, [1] * 65, [0] * 65),                                        # K = 65: outside
            {"durations": D7, "locations": locs7, "capacities": caps7, "start_times": starts7,
             "ignored_customers": [103]},
            request(inside[6], 100)]
    assert not solver.batch_ga_fits(solver.compact_vrp(*reqs[4]), P, G)
    kw = dict(pop=P, gens=G, seed=SEED, objective=objective, with_unvisited=True)
    got = solver.solve_vrp_ga_batch(reqs, **kw)
    assert got[2] == {"durationMax": 0, "durationSum": 0, "unvisited": [],
                      "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    for x, (r, res) in enumerate(zip(reqs, got)):
        if isinstance(r, dict):
            r = (r["durations"], r["locations"], r["capacities"], r["start_times"],
                 r["ignored_customers"])
        _rescored(r, res, objective)
    assert got[4] == solver.solve_vrp("ga", *reqs[4], seed=SEED, objective=objective,
                                      with_unvisited=True, random_permutation_count=P,
                                      iteration_count=G)
    # the answers of the requests inside the domain are A23's
    for x, case in inside.items():
        assert got[x] == _ref_dict(case, objective, P, G)
    # deterministic, and the same alone as in company
    assert solver.solve_vrp_ga_batch(reqs, **kw) == got
    for x in (0, 1, 5):
        assert solver.solve_vrp_ga_batch([reqs[x]], **kw) == [got[x]]
    assert "unvisited" not in solver.solve_vrp_ga_batch([reqs[0]], pop=P, gens=G, seed=SEED)[0]


@pytest.mark.gpu
def test_service_batch_vrp_ga_equals_solve_vrp_ga_batch(monkeypatch):
    windows = []
    sleep = service.time.sleep
    monkeypatch.setattr(service.time, "sleep",
                        lambda s: (windows.append(s) if s == 0.05 else None, sleep(s)))
    P, G = 48, 6
    D, locs, caps, starts = request((8, 3, 1, 59, ""), 100)
    store = service.MemoryStore({"7": locs}, {"8": D}, {})
    app = service.App(store, seed=SEED, batch_vrp_ga=True, batch_window_s=0.05)
    api = json.dumps({"solutionName": "s", "solutionDescription": "d", "locationsKey": 7,
                      "durationsKey": 8, "capacities": caps, "startTimes": starts,
                      "ignoredCustomers": [], "completedCustomers": [], "multiThreaded": False,
                      "randomPermutationCount": P, "iterationCount": G}).encode()
    cases = [((6, 2, 24, 60 + x, "") if x % 2 else (8, 3, 1, 60 + x, "")) for x in range(24)]

    def call(x):
        if x >= len(cases):
            return app.post("vrp", "ga", api)
        return app.solve_inline("vrp", "ga", _body(cases[x], randomPermutationCount=P,
                                                   iterationCount=G))

    out = _concurrently(call, len(cases) + 4)
    b = app.vrp_ga_batcher
    assert b.requests == 28 and 2 <= b.launches <= 2 * len(windows)
    assert b.launches < b.requests
    for x, (st, res) in enumerate(out):
        assert st == 200, res
        req = request(cases[x], 100) if x < len(cases) else (D, locs, caps, starts)
        assert [res["message"]] == solver.solve_vrp_ga_batch([req], pop=P, gens=G, seed=SEED)
    assert out[0][1]["message"] == {k: v for k, v in _ref_dict(cases[0], "sum", P, G).items()
                                    if k != "unvisited"}
