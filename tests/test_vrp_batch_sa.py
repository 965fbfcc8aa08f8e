"""Batched VRP annealing (spec A22): the C entry points vrpms_vrp_batch_sa_lds
/ vrpms_vrp_batch_sa, Context.vrp_batch_sa, solver.batch_sa_schedule /
batch_sa_fits / solve_vrp_sa_batch and the service's VRP SA batcher
(App(batch_vrp_sa=True)).

The reference is a22_ref below: A22 restated from oracle.spec (Philox, the
first-fit start, A13's one-word moves, apply_move, the greedy split with
separators and the hour lookup) and oracle.search.accept_threshold.  Per
request the GPU must return the identical key, tour, route durations and
vehicle row, for both objectives."""
import ctypes
import functools
import json
import threading

import numpy as np
import pytest

from oracle import spec
from oracle.search import accept_threshold
from vrpms_amd import _lib, core, service, solver

LDS_BYTES = 160 * 1024
OBJECTIVES = ("sum", "max")
SEED = 20221
M32 = 0xFFFFFFFF
_F = np.float32


def obj_id(objective):
    return spec.OBJ_SUM if objective == "sum" else spec.OBJ_MAX


# ---------------------------------------------------------------------------
# instances and their references (computed once, shared, never changed)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inst(case):
    """case = (n, K, H, seed, variant) -> (D int64 [H][N][N], demand [N], caps,
    starts): entries 1..89 (0 on the diagonal), demands 1..9, K unequal
    capacities around an even share of the total demand (so some fleets leave
    customers unvisited), start times in 0..1439.  Variants:
      "below"     every capacity below every demand (all unvisited)
      "hours"     entries 20..89 and start times 59, 60, 1439, 23*60+50 cycled
      "e65535" / "e65536"  one entry of that value (hour 0, edge 1 -> 2)
      "zerocap"   a zero capacity in the middle of the fleet
      "zerodem"   a zero-demand customer
      "tight"     capacities share - 2 each"""
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
    elif variant == "tight":
        caps = [max(0, share - 2)] * K
    else:
        assert variant == "", variant
    D.setflags(write=False)
    dem.setflags(write=False)
    return D, dem, tuple(int(c) for c in caps), tuple(int(s) for s in starts)


def schedule(D, steps):
    """solver.batch_sa_schedule restated: half the mean positive entry of the
    request's own matrix, cooled by 250 over the steps."""
    nz = D[D > 0]
    inv_t0 = 1.0 / (0.5 * float(nz.mean())) if nz.size else 1.0
    return inv_t0, (0.5 / 0.002) ** (1.0 / max(1, steps))


def a22_ref(D, dem, caps, starts, objective, steps, inv_t0, inv_alpha, seed):
    """Spec A22 -> dict(key, tour, durs, veh, wave, uphill, rejects)."""
    D = spec.as_3d(D)
    n, K = D.shape[1] - 1, len(caps)
    ntok = n + K - 1
    key = spec.seed_key(seed)
    obj = obj_id(objective)

    def score(t):
        return spec.eval_cvrp(D, t, dem, caps, starts, obj)["key"]

    best, uphill, rejects = None, 0, 0
    for w in range(4):
        t = list(range(1, n + 1))
        for i in range(n - 1, 0, -1):
            j = spec.philox4x32_10((M32, M32, w, i), key)[0] % (i + 1)
            t[i], t[j] = t[j], t[i]
        t = spec.pack_separators(t, K - 1, dem, caps)
        assert len(t) == ntok
        ck = score(t)
        bk, bt = ck, t[:]
        invT = _F(inv_t0)
        blocks = None
        for s in range(steps if ntok >= 2 else 0):
            if s & 3 == 0:
                blocks = [spec.philox4x32_10((s >> 2, 0, w, lane), key) for lane in range(64)]
            moves = [spec.decode_move1(b[s & 3], ntok) for b in blocks]
            cands = [spec.apply_move(t, *m) for m in moves]
            keys = spec.eval_cvrp_batch(D, np.array(cands), dem, caps, starts, obj)[0]
            lane = int(np.argmin(keys))          # the first minimum: the least (key, lane)
            kk = score(cands[lane])
            assert kk == int(keys[lane])
            xa = spec.philox4x32_10((s >> 2, 1, w, 0), key)[s & 3]
            acc = kk <= ck
            if not acc:
                acc = (xa >> 8) < accept_threshold(min((kk >> 28) - (ck >> 28), M32), invT)
                uphill += acc
                rejects += not acc
            if acc:
                t, ck = cands[lane], kk
                if ck < bk:
                    bk, bt = ck, t[:]
            invT = _F(invT * _F(inv_alpha))
        if best is None or bk < best[0]:
            best = (bk, bt, w)
    final = spec.eval_cvrp(D, best[1], dem, caps, starts, obj)
    assert final["key"] == best[0]
    return dict(key=best[0], tour=best[1], durs=final["durations"], veh=final["vehicle_of"],
                wave=best[2], uphill=uphill, rejects=rejects, unvisited=final["unvisited"])


@functools.lru_cache(maxsize=None)
def reference(case, objective, steps):
    D, dem, caps, starts = inst(case)
    inv_t0, inv_alpha = schedule(D, steps)
    return a22_ref(D, dem, caps, starts, objective, steps, inv_t0, inv_alpha, SEED)


def expected(cases, objective, steps):
    refs = [reference(c, objective, steps) for c in cases]
    return ([r["key"] for r in refs], [r["tour"] for r in refs], [r["durs"] for r in refs],
            [r["veh"] for r in refs])


def lds_bytes(N, K, H, wide):
    """vrp_batch_sa.hip batch_sa_lds: the matrix padded to 16 bytes, the demand
    row and the two fleet rows as int32 padded to four words, 4 chains x 3
    uint16 tours padded to eight tokens, and the four chains' best keys."""
    def pad(x, m):
        return (x + m - 1) // m * m
    return pad(H * N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + \
        4 * 3 * 2 * pad(N - 1 + K - 1, 8) + 4 * 8


def largest_n_nodes(K, H, wide):
    return max(N for N in range(2, 400) if lds_bytes(N, K, H, wide) <= LDS_BYTES)


# the shapes of the GPU comparisons: (case, steps)
NTOK_EDGES = [((1, 1, 1, 0, ""), 8), ((2, 1, 1, 1, ""), 8), ((1, 2, 24, 2, "below"), 8),
              ((6, 2, 24, 4, ""), 40), ((7, 2, 1, 4, ""), 12), ((7, 3, 24, 5, ""), 12),
              ((58, 6, 1, 6, ""), 12), ((59, 6, 1, 7, ""), 12), ((60, 6, 1, 8, ""), 12)]
STEP_TAILS = [((8, 3, 1, 9, ""), s) for s in (0, 1, 3, 4, 5, 41)]
HOURS = [((6, 3, 24, s, "hours"), 20) for s in (10, 11)]
WIDE_HOURS = [((7, 3, 24, 31, "e65536"), 10)]   # an int32 matrix at H = 24
FLEETS = [((3, 64, 1, 12, ""), 10), ((9, 5, 24, 13, "zerocap"), 10), ((9, 3, 1, 14, "zerodem"), 10),
          ((9, 3, 24, 15, "tight"), 10)]
SIX = [(10, 3, 24, 20 + x, "") for x in range(6)]


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
    f = lib.vrpms_vrp_batch_sa_lds
    Ks = (1, 2, 7, 8, 9, 64)
    for H in (1, 24):
        for wide in (0, 1):
            for x, K in enumerate(Ks):
                for N in range(2, 65):
                    assert f(N, K, H, wide, ctypes.byref(b)) == _lib.VRPMS_OK
                    assert b.value == lds_bytes(N, K, H, wide) == core.vrp_batch_sa_lds(N, K, H, wide)
                    if N > 2:
                        assert b.value >= lds_bytes(N - 1, K, H, wide)
                    if x:
                        assert b.value >= lds_bytes(N, Ks[x - 1], H, wide)
            assert lds_bytes(64, 9, H, wide) > lds_bytes(2, 1, H, wide)
    for args, word in (((1, 3, 1, 0), b"2 <= N"), ((0, 3, 1, 0), b"2 <= N"), ((-5, 3, 24, 1), b"2 <= N"),
                       ((5, 0, 1, 0), b"1 <= K <= 64"), ((5, 65, 1, 0), b"1 <= K <= 64"),
                       ((5, 3, 2, 0), b"H must be 1 or 24"), ((5, 3, 0, 0), b"H must be 1 or 24"),
                       ((5, 3, 1, 2), b"wide"), ((5, 3, 1, -1), b"wide")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_sa_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(5, 3, 1, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_sa_lds" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= K <= 64"):
        core.vrp_batch_sa_lds(5, 65, 1, False)
    assert solver.BATCH_SA_LDS_BYTES == LDS_BYTES


def test_argument_errors_need_no_gpu(lib):
    """Every argument check comes before the context is looked at, so a
    stand-in block of zeros serves as the non-NULL ctx here."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(4096)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    names = ("m", "d", "cp", "st", "it", "t", "k", "du", "v")

    def f(ctx=c, R=1, N=5, K=2, H=1, obj=0, wide=0, steps=3, **ptrs):
        a = {name: ptrs.get(name, p) for name in names}
        return lib.vrpms_vrp_batch_sa(ctx, a["m"], a["d"], a["cp"], a["st"], a["it"], R, N, K, H, obj,
                                      wide, steps, 1.01, 5, a["t"], a["k"], a["du"], a["v"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_sa:" in msg and word in msg, (kw, msg)

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
    refused(b"steps", steps=-1)
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
    """The case as a solve_vrp_sa_batch tuple (H = 1 as a plain [N][N] matrix)."""
    D, dem, caps, starts = inst(case)
    return ((D[0] if D.shape[0] == 1 else D).tolist(), _locs(dem, base), list(caps), list(starts))


def compact(case):
    return solver.compact_vrp(*request(case))


def test_solve_vrp_sa_batch_refusals_need_no_gpu(monkeypatch, lib):
    _no_gpu(monkeypatch)
    good = request((6, 2, 1, 0, ""))
    assert solver.solve_vrp_sa_batch([]) == []
    with pytest.raises(ValueError, match=r"^request 1: capacities and startTimes"):
        solver.solve_vrp_sa_batch([good, (good[0], good[1], [3, 3], [0])])
    with pytest.raises(ValueError, match=r"^request 2: 5 locations but a 7-node"):
        solver.solve_vrp_sa_batch([good, good, {"durations": good[0], "locations": good[1][:5],
                                                "capacities": [3], "start_times": [0]}])
    big = np.full((7, 7), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_vrp_sa_batch([good, (big.tolist(), good[1], [3, 3], [0, 0])])
    with pytest.raises(ValueError, match=r"^request 0: .*A9 guard"):       # the start time counts
        solver.solve_vrp_sa_batch([(good[0], good[1], [3, 3], [0, 2**31 - 100]), good])
    heavy = [{"id": i, "demand": 2**30} for i in range(7)]
    with pytest.raises(ValueError, match=r"^request 0: capacity \+ demand overflows int32"):
        solver.solve_vrp_sa_batch([(good[0], heavy, [2**30, 3], [0, 0])])
    with pytest.raises(ValueError, match="objective"):
        solver.solve_vrp_sa_batch([good], objective="mean")
    with pytest.raises(ValueError, match="steps"):
        solver.solve_vrp_sa_batch([good], steps=-1)
    # no customer: solve_vrp's trivial answer, built on the host
    none = (good[0], good[1], [3, 3], [0, 7], [1, 2, 3, 4, 5, 6])
    assert solver.solve_vrp_sa_batch([none], with_unvisited=True) == [
        {"durationMax": 0, "durationSum": 0, "unvisited": [],
         "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}]


def test_schedule_is_the_requests_own(lib):
    for case in ((6, 2, 24, 4, ""), (8, 3, 1, 9, ""), (6, 3, 24, 10, "hours")):
        for steps in (1, 40, 2000):
            assert solver.batch_sa_schedule(compact(case), steps) == schedule(inst(case)[0], steps)
    zero = solver.compact_vrp(np.zeros((4, 4), dtype=np.int64), _locs([0, 1, 1, 1]), [3], [0])
    assert solver.batch_sa_schedule(zero, 0) == (1.0, 250.0)
    assert solver.batch_sa_schedule(zero, 2)[1] == 250.0 ** 0.5


def _sized(N, K, H, big=0):
    D = np.ones((H, N, N), dtype=np.int64)
    D[0, 0, 1] += big
    return solver.compact_vrp(D if H > 1 else D[0], _locs([0] + [1] * (N - 1)), [N] * K, [0] * K)


def test_batch_sa_fits_at_the_lds_edge(lib):
    for K, H, wide in ((4, 24, False), (4, 1, True)):
        N = largest_n_nodes(K, H, wide)
        assert lds_bytes(N, K, H, wide) <= LDS_BYTES < lds_bytes(N + 1, K, H, wide)
        big = 70000 if wide else 0
        assert solver.batch_sa_fits(_sized(N, K, H, big))
        assert not solver.batch_sa_fits(_sized(N + 1, K, H, big))
        assert solver.batch_sa_key(_sized(N, K, H, big)) == (N, K, H, wide)
    assert largest_n_nodes(4, 24, False) == 58 and largest_n_nodes(4, 1, True) == 198
    # a wide entry halves the cells that fit; 65535 is still narrow
    N = largest_n_nodes(4, 24, False)
    assert not solver.batch_sa_fits(_sized(N, 4, 24, 70000))
    assert solver.batch_sa_fits(_sized(N, 4, 24, 65534))
    # outside the domain whatever the size
    assert not solver.batch_sa_fits(_sized(5, 65, 1))
    none = solver.compact_vrp(np.ones((3, 3), dtype=np.int64), _locs([0, 1, 1]), [3], [0], [1, 2])
    assert none.n == 0 and not solver.batch_sa_fits(none)
    tsp = solver.compact_tsp(np.ones((4, 4), dtype=np.int64), [1, 2, 3], 0, 0)
    assert not solver.batch_sa_fits(tsp)
    assert service.VrpSaBatcher.accepts(_sized(6, 2, 24))
    assert not service.VrpSaBatcher.accepts(_sized(6, 2, 1, 2**29))       # the A9 guard


def test_reference_properties():
    """What the GPU comparisons rely on, checked on the reference itself."""
    refs = {(c, o, s): reference(c, o, s) for c, s in NTOK_EDGES for o in OBJECTIVES}
    assert any(r["unvisited"] > 0 for r in refs.values())
    assert reference((1, 2, 24, 2, "below"), "sum", 8)["unvisited"] == 1
    r = reference((6, 2, 24, 4, ""), "sum", 40)
    print("n=6 K=2 H=24, 40 steps: uphill", r["uphill"], "rejects", r["rejects"])
    assert r["uphill"] > 0 and r["rejects"] > 0
    waves = {k[0][0]: r["wave"] for k, r in refs.items() if k[1] == "sum"}
    print("winning chains", waves)
    assert any(w != 0 for w in waves.values())
    # one token: no step, the four chains tie and chain 0 wins
    one = reference((1, 1, 1, 0, ""), "max", 8)
    assert one["wave"] == 0 and one["tour"] == [1] and one["uphill"] == one["rejects"] == 0
    # the hour cases cross an hour and midnight: the static slice gives another answer
    for case, steps in HOURS:
        D, dem, caps, starts = inst(case)
        r = reference(case, "sum", steps)
        flat = spec.eval_cvrp(D[:1], r["tour"], dem, caps, starts)
        assert flat["key"] != r["key"]
        assert any(s + d >= 1440 for s, d in zip(starts, r["durs"]) if d)


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
            tours.append(list(range(ci.n, 0, -1)) + [0] * (K - 1))
            rest.append(([0] * ci.n + [-2] * (K - 1), [10 * ci.n] + [0] * (K - 1)))
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


def test_vrp_sa_batcher_groups_and_fans_out_errors(lib):
    seen = []
    b = service.VrpSaBatcher(_FakeApp(), window_s=0.2, steps=7, launch=_fake_launch(seen))
    jobs = [((5, 2, 1, x, ""), "sum") for x in range(5)] + [((5, 3, 1, 5, ""), "sum")] * 3 + \
           [((5, 2, 24, 8 + x, ""), "max") for x in range(2)] + [((5, 2, 1, 10, "e65536"), "sum")]
    out = _concurrently(lambda x: b.solve(compact(jobs[x][0]), jobs[x][1]), len(jobs))
    assert sorted(seen) == [((6, 2, 1, False, "sum"), 5), ((6, 2, 1, True, "sum"), 1),
                            ((6, 2, 24, False, "max"), 2), ((6, 3, 1, False, "sum"), 3)]
    assert b.launches == 4 and b.requests == 11
    for (case, _), res in zip(jobs, out):
        K = case[1]
        assert res == {"durationMax": 50, "durationSum": 50,
                       "vehicles": [{"tour": [0, 5, 4, 3, 2, 1, 0], "duration": 50}] +
                                   [{"tour": [0, 0], "duration": 0}] * (K - 1)}

    def failing(key, cis):
        if key[1] == 2:
            raise RuntimeError("launch failed")
        return _fake_launch([])(key, cis)

    b = service.VrpSaBatcher(_FakeApp(), window_s=0.2, launch=failing)
    out = _concurrently(lambda x: b.solve(compact(jobs[x][0]), jobs[x][1]), 8)
    assert all(isinstance(o, RuntimeError) and "launch failed" in str(o) for o in out[:5])
    assert all(isinstance(o, dict) and len(o["vehicles"]) == 3 for o in out[5:])


def test_app_batch_vrp_sa_routes(lib):
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, len(params["capacities"])))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    off = service.App(service.MemoryStore({}, {}, {}), solve=fake)
    assert off.vrp_sa_batcher is None
    assert off.solve_inline("vrp", "sa", _body((5, 2, 1, 0, "")))[1]["message"]["durationSum"] == 3
    assert seen == [("vrp", "sa", 2)]
    del seen[:]

    D, locs, caps, starts = request((5, 2, 1, 1, ""), 100)
    store = service.MemoryStore({"7": locs}, {"8": D}, {})
    app = service.App(store, solve=fake, batch_vrp_sa=True, batch_window_s=0.2, batch_steps=9,
                      batch_vrp_sa_launch=_fake_launch(launched))
    assert isinstance(app.vrp_sa_batcher, service.VrpSaBatcher) and app.vrp_sa_batcher.steps == 9
    assert app.batcher is None and app.exact_vrp_batcher is None
    api = json.dumps({"solutionName": "s", "solutionDescription": "d", "locationsKey": 7,
                      "durationsKey": 8, "capacities": caps, "startTimes": starts,
                      "ignoredCustomers": [103], "completedCustomers": []}).encode()

    def call(x):
        if x == 0:
            return app.post("vrp", "sa", api)
        if x < 6:
            return app.solve_inline("vrp", "sa", _body((5, 2, 1, x, "")))
        return app.solve_inline("vrp", "sa", _body((5, 2, 1, x, ""), objective="max"))

    out = _concurrently(call, 9)
    assert all(st == 200 for st, _ in out), out
    assert sorted(launched) == [((5, 2, 1, False, "sum"), 1), ((6, 2, 1, False, "max"), 3),
                                ((6, 2, 1, False, "sum"), 5)]
    assert seen == [] and app.vrp_sa_batcher.requests == 9
    # location 103 (row 3) is ignored: compact customers 4..1 are rows 5, 4, 2, 1
    assert out[0][1]["message"] == {
        "durationMax": 40, "durationSum": 40,
        "vehicles": [{"tour": [0, 5, 4, 2, 1, 0], "duration": 40}, {"tour": [0, 0], "duration": 0}]}
    assert out[1][1]["message"]["vehicles"][0]["tour"] == [0, 5, 4, 3, 2, 1, 0]
    # outside the domain, another algorithm, or knobs of its own: the injected solve
    wide_fleet = json.dumps({"durations": D, "locations": locs, "capacities": [1] * 65,
                             "startTimes": [0] * 65, "ignoredCustomers": [],
                             "completedCustomers": []}).encode()
    assert app.solve_inline("vrp", "sa", wide_fleet)[0] == 200
    assert app.solve_inline("vrp", "ga", _body((5, 2, 1, 1, "")))[0] == 200
    assert app.solve_inline("vrp", "sa", _body((5, 2, 1, 1, ""), knobs={"steps": 50}))[0] == 200
    assert seen == [("vrp", "sa", 65), ("vrp", "ga", 2), ("vrp", "sa", 2)]
    assert len(launched) == 3
    # a bad instance is a 400 in solve_vrp's words
    st, res = app.solve_inline("vrp", "sa", _body((5, 2, 1, 1, ""), startTimes=[0]))
    assert st == 400 and "capacities and startTimes" in res["errors"][0]["reason"]


def test_cli_flag(monkeypatch):
    made = {}

    class Stop(Exception):
        pass

    def app(store, **kw):
        made.update(kw)
        raise Stop

    monkeypatch.setattr(service, "App", app)
    for argv, want in ((["--batch-vrp-sa", "--batch-steps", "11"], True), ([], False)):
        with pytest.raises(Stop):
            service.main(argv)
        assert made["batch_vrp_sa"] is want and made["batch_tsp"] is False
    assert made["batch_steps"] == 2000


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_batch(ctx, cases, objective, steps, wide=None):
    """One vrp_batch_sa launch -> ([key], [tour], [durs], [veh])."""
    import torch
    insts = [inst(c) for c in cases]

    def dev(rows, dtype=torch.int32):
        return torch.tensor(np.stack(rows), dtype=dtype, device=ctx.dev)

    sched = [schedule(D, steps) for D, _, _, _ in insts]
    tours, keys, durs, veh = ctx.vrp_batch_sa(
        dev([D for D, _, _, _ in insts]), dev([d for _, d, _, _ in insts]),
        dev([np.array(c) for _, _, c, _ in insts]), dev([np.array(s) for _, _, _, s in insts]),
        dev([np.array(s[0], dtype=np.float32) for s in sched], torch.float32),
        obj_id(objective), steps, sched[0][1], SEED, wide=wide)
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), veh.cpu().tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("case,steps", NTOK_EDGES + STEP_TAILS + HOURS + WIDE_HOURS + FLEETS)
def test_gpu_equals_reference(ctx, case, steps, objective):
    got = gpu_batch(ctx, [case], objective, steps)
    want = expected([case], objective, steps)
    print(case, steps, objective, "gpu", got, "ref", want)
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_staging_width(ctx, objective):
    a, b, c = (7, 3, 1, 30, ""), (7, 3, 1, 31, "e65535"), (7, 3, 1, 32, "")
    over = (7, 3, 1, 31, "e65536")
    assert gpu_batch(ctx, [a, b, c], objective, 10, wide=False) == expected([a, b, c], objective, 10)
    assert gpu_batch(ctx, [a, over, c], objective, 10, wide=True) == \
        expected([a, over, c], objective, 10)
    assert gpu_batch(ctx, [over], objective, 10) == expected([over], objective, 10)   # wide=None
    keys, tours, durs, veh = gpu_batch(ctx, [a, over, c], objective, 10, wide=False)
    want = expected([a, over, c], objective, 10)
    assert keys[1] == 2**64 - 1 and tours[1] == [0] * 9 and durs[1] == [0] * 3 and veh[1] == [-1] * 9
    for x in (0, 2):
        assert (keys[x], tours[x], durs[x], veh[x]) == tuple(w[x] for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_batch_independence_and_grid(ctx, objective):
    cases = [SIX[x % 6] for x in range(300)]
    got = gpu_batch(ctx, cases, objective, 10)
    assert got == expected(cases, objective, 10)
    for x, c in enumerate(SIX):
        assert gpu_batch(ctx, [c], objective, 10) == tuple([g[x]] for g in got)


@pytest.mark.gpu
def test_gpu_lds_edge(ctx):
    import torch
    lib, K, H, R = ctx.lib, 4, 24, 2
    N = largest_n_nodes(K, H, False)
    cases = [(N - 1, K, H, 40 + x, "") for x in range(R)]
    for objective in OBJECTIVES:
        assert gpu_batch(ctx, cases, objective, 4) == expected(cases, objective, 4)
    N += 1
    ntok = N - 1 + K - 1
    M = torch.ones((R, H, N, N), dtype=torch.int32, device=ctx.dev)
    dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
    cp = torch.ones((R, K), dtype=torch.int32, device=ctx.dev)
    it = torch.ones((R,), dtype=torch.float32, device=ctx.dev)
    tours = torch.full((R, ntok), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R, K), -7, dtype=torch.int32, device=ctx.dev)
    veh = torch.full((R, ntok), -7, dtype=torch.int8, device=ctx.dev)
    rc = lib.vrpms_vrp_batch_sa(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(), cp.data_ptr(),
                                it.data_ptr(), R, N, K, H, 0, 0, 4, 1.5, SEED, tours.data_ptr(),
                                keys.data_ptr(), durs.data_ptr(), veh.data_ptr(), ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_sa:" in msg and b"bytes of LDS" in msg
    assert str(lds_bytes(N, K, H, False)).encode() in msg
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


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_sa_batch_mixed_list(objective):
    D7, locs7, caps7, starts7 = request((6, 2, 24, 50, ""), 100)
    reqs = [request((6, 2, 24, 51, ""), 100), request((9, 3, 1, 52, "tight"), 100),
            (D7, locs7, caps7, starts7, [100 + i for i in range(1, 7)]),            # none active
            request((6, 2, 24, 53, ""), 100),
            (D7, locs7, [1] * 65, [0] * 65),                                        # K = 65: outside
            {"durations": D7, "locations": locs7, "capacities": caps7, "start_times": starts7,
             "ignored_customers": [103]},
            request((9, 3, 1, 54, "tight"), 100)]
    assert not solver.batch_sa_fits(solver.compact_vrp(*reqs[4]))
    got = solver.solve_vrp_sa_batch(reqs, steps=30, seed=SEED, objective=objective,
                                    with_unvisited=True)
    assert got[2] == {"durationMax": 0, "durationSum": 0, "unvisited": [],
                      "vehicles": [{"tour": [0, 0], "duration": 0}] * 2}
    for x, (r, res) in enumerate(zip(reqs, got)):
        if isinstance(r, dict):
            r = (r["durations"], r["locations"], r["capacities"], r["start_times"],
                 r["ignored_customers"])
        _rescored(r, res, objective)
    assert any(res["unvisited"] for res in got)
    assert got[4] == solver.solve_vrp("sa", *reqs[4], seed=SEED, objective=objective,
                                      with_unvisited=True)
    # the answer of a request inside the domain is A22's
    ref = reference((6, 2, 24, 51, ""), objective, 30)
    assert [v["duration"] for v in got[0]["vehicles"]] == ref["durs"]
    # deterministic, and the same alone as in company
    assert solver.solve_vrp_sa_batch(reqs, steps=30, seed=SEED, objective=objective,
                                     with_unvisited=True) == got
    for x in (0, 1, 5):
        assert solver.solve_vrp_sa_batch([reqs[x]], steps=30, seed=SEED, objective=objective,
                                         with_unvisited=True) == [got[x]]
    assert "unvisited" not in solver.solve_vrp_sa_batch([reqs[0]], steps=30, seed=SEED)[0]


@pytest.mark.gpu
def test_service_batch_vrp_sa_equals_solve_vrp_sa_batch(monkeypatch):
    windows = []
    sleep = service.time.sleep
    monkeypatch.setattr(service.time, "sleep",
                        lambda s: (windows.append(s) if s == 0.05 else None, sleep(s)))
    app = service.App(service.MemoryStore({}, {}, {}), seed=SEED, batch_vrp_sa=True,
                      batch_window_s=0.05, batch_steps=25)
    cases = [((6, 2, 24, 60 + x, "") if x % 2 else (8, 3, 1, 60 + x, "")) for x in range(32)]
    out = _concurrently(lambda x: app.solve_inline("vrp", "sa", _body(cases[x])), 32)
    b = app.vrp_sa_batcher
    assert b.requests == 32 and 2 <= b.launches <= 2 * len(windows)
    assert b.launches < b.requests
    for case, (st, res) in zip(cases, out):
        assert st == 200, res
        assert [res["message"]] == solver.solve_vrp_sa_batch([request(case, 100)], steps=25, seed=SEED)
