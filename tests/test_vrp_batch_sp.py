"""Batched exact VRP (spec A19): the C entry points vrpms_vrp_batch_sp_lds /
vrpms_vrp_batch_sp, Context.vrp_batch_sp, solver.solve_vrp_batch and the
service's exact VRP batcher (App(batch_exact=True)).

The reference is sp_ref of test_vrp_sp.py (A15's recurrence and tie rule in
numpy, itself checked there against the enumeration of every separator tour);
per request the GPU must return the identical key, tour and route durations,
and the identical key and tour as the single-request set-partitioning
kernels."""
import ctypes
import functools
import json
import threading

import numpy as np
import pytest

from oracle import spec
from test_vrp_sp import REF_CASES, demands, matrix, obj_id, ref_case, sp_ref
from vrpms_amd import _lib, core, runners, service, solver

LDS_BYTES = 160 * 1024
TEAMS = (16, 32, 64, 128, 256)
# the n -> T table of vrp_batch_sp.hip before the LDS has its say
TEAM_TABLE = (16, 16, 16, 16, 16, 16, 32, 64, 128, 256, 256, 256, 256)
OBJECTIVES = ("sum", "max")
KINDS = ("sym", "asym", "ties", "equal")


# ---------------------------------------------------------------------------
# instances and their references (computed once, shared, never changed)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inst(case):
    """case: ("ref", name) = test_vrp_sp's ref_case(name), or (kind, n, K,
    seed): a `kind` matrix, demands 1..9 and K unequal capacities around an
    even share of the total demand (so some fleets leave customers unserved
    and some vehicles stay empty) -> (D, demand, caps)."""
    if case[0] == "ref":
        D, dem, caps = ref_case(case[1])
    else:
        kind, n, K, seed = case
        D, dem = matrix(kind, n + 1, seed), demands(n, seed)
        share = int(dem.sum()) // K
        rng = np.random.default_rng(5000 + seed)
        caps = rng.integers(max(0, share - 3), share + 7, size=K).tolist()
    D = np.asarray(D, dtype=np.int64)
    dem = np.asarray(dem, dtype=np.int64)
    D.setflags(write=False)
    dem.setflags(write=False)
    return D, dem, tuple(int(c) for c in caps)


@functools.lru_cache(maxsize=None)
def reference(case, objective):
    D, dem, caps = inst(case)
    r = sp_ref(D, dem, list(caps), objective)
    return r["key"], tuple(r["tour"]), tuple(r["durations"])


def mixed(n, K, R, distinct=10):
    """R cases of (n, K) cycling through `distinct` instances whose kinds
    cycle through KINDS: neighbours in a workgroup differ in kind."""
    return [(KINDS[x % distinct % len(KINDS)], n, K, 100 * n + 7 * K + x % distinct)
            for x in range(R)]


def expected(cases, objective):
    refs = [reference(c, objective) for c in cases]
    return [r[0] for r in refs], [list(r[1]) for r in refs], [list(r[2]) for r in refs]


def lds_bytes(n, K, T):
    """vrp_batch_sp.hip batch_sp_lds_bytes: the binomial table (172 words),
    then per team the 13 x 16-word matrix image, 16 demand words, the
    capacities, the compact Held-Karp table, and route, the capacity-masked
    routes (K >= 2) and the K layers of 2^n words, every part padded to four
    words."""
    def pad4(w):
        return (w + 3) & ~3
    team = 208 + 16 + pad4(K) + pad4(n << (n - 1)) + (1 + (K >= 2) + K) * pad4(1 << n)
    return (172 + (256 // T) * team) * 4


def auto_team(n, K):
    T = TEAM_TABLE[n]
    while T < 256 and lds_bytes(n, K, T) > LDS_BYTES:
        T *= 2
    return T


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


def test_lds_bytes_formula_floor_and_refusals(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_vrp_batch_sp_lds
    # the formula, for every team; at a fixed team it grows with n and with K
    for T in TEAMS:
        for n in range(1, 13):
            for K in range(1, 65):
                assert f(n, K, T, ctypes.byref(b)) == _lib.VRPMS_OK
                assert b.value == lds_bytes(n, K, T)
                if K > 1:
                    assert b.value > lds_bytes(n, K - 1, T)
                if n > 2:
                    assert b.value > lds_bytes(n - 1, K, T)
                elif n == 2:      # one and two customers pad to the same four words
                    assert b.value == lds_bytes(1, K, T)
    # team 0 is the table's team, raised until 256 / T requests fit: what fits
    # at (n, K) fits at every smaller n and K
    fits = {}
    for n in range(1, 13):
        for K in range(1, 65):
            assert f(n, K, 0, ctypes.byref(b)) == _lib.VRPMS_OK
            assert b.value == lds_bytes(n, K, auto_team(n, K)) == core.vrp_batch_sp_lds(n, K)
            fits[n, K] = b.value <= LDS_BYTES
            assert fits[n, K] == (lds_bytes(n, K, 256) <= LDS_BYTES)
            if fits[n, K]:
                assert (K == 1 or fits[n, K - 1]) and (n == 1 or fits[n - 1, K])
    # the floor every layout must admit, and the first fleet beyond it
    assert all(fits[n, 64] for n in range(1, 10))
    assert fits[10, 32] and fits[11, 12] and fits[12, 1]
    assert not fits[12, 64] and not fits[10, 64] and not fits[11, 64]
    for args, word in (((0, 3, 0), b"1 <= n <= 12"), ((13, 3, 0), b"1 <= n <= 12"),
                       ((5, 0, 0), b"1 <= K <= 64"), ((5, 65, 0), b"1 <= K <= 64"),
                       ((5, 3, 8), b"team"), ((5, 3, 48), b"team"), ((5, 3, -16), b"team"),
                       ((5, 3, 512), b"team")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_sp_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(5, 3, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_sp_lds" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= n <= 12"):
        core.vrp_batch_sp_lds(13, 3)
    assert solver.BATCH_SP_MAX_CUSTOMERS == 12 and solver.BATCH_SP_LDS_BYTES == LDS_BYTES


def test_argument_errors_need_no_gpu(lib):
    """Every argument check comes before the context is looked at, so a
    stand-in block of zeros serves as the non-NULL ctx here."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(4096)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)

    def f(ctx=c, m=p, d=p, cp=p, R=1, N=5, K=2, obj=0, team=0, t=p, k=p, du=p):
        return lib.vrpms_vrp_batch_sp(ctx, m, d, cp, R, N, K, obj, team, t, k, du, None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_sp:" in msg and word in msg, (kw, msg)

    refused(b"ctx is NULL", ctx=None)
    refused(b"R must not be negative", R=-1)
    for N in (-1, 0, 1, 14, 50):
        refused(b"2 <= N <= 13", N=N)
    for K in (-1, 0, 65, 1000):
        refused(b"1 <= K <= 64", K=K)
    for obj in (-1, 2):
        refused(b"objective", obj=obj)
    for team in (-1, 8, 48, 255, 512):
        refused(b"team", team=team)
    for name in ("m", "d", "cp", "t", "k", "du"):
        refused(b"NULL", **{name: None})
    # the checks come in this order even with R = 0
    refused(b"2 <= N <= 13", R=0, N=14)
    refused(b"team", R=0, team=3)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, m=None, d=None, cp=None, t=None, k=None, du=None, N=13, K=64, obj=1,
             team=256) == _lib.VRPMS_OK
    assert buf.raw == bytes(4096) and fake.raw == bytes(1 << 16)


def _no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(solver, "context", boom)
    monkeypatch.setattr(solver, "Context", boom)


def _locs(N, demand=1):
    return [{"id": i, "demand": demand} for i in range(N)]


def test_solve_vrp_batch_refusals_need_no_gpu(monkeypatch):
    _no_gpu(monkeypatch)
    D6 = matrix("sym", 6, 0)
    good = (D6.tolist(), _locs(6), [3, 3], [0, 0])
    with pytest.raises(ValueError, match="'bf'"):
        solver.solve_vrp_batch("bf", [good])
    with pytest.raises(ValueError, match='only "sp"'):
        solver.solve_vrp_batch("tdsp", [good])
    td = np.stack([D6] * 24)
    with pytest.raises(ValueError, match=r"^request 1: sp \(set partitioning\) needs a static"):
        solver.solve_vrp_batch("sp", [good, (td.tolist(), _locs(6), [3, 3], [0, 0])])
    D22 = matrix("sym", 22, 0)
    with pytest.raises(ValueError, match=r"^request 2: sp \(set partitioning\) supports at most "
                                         r"20 customers \(21 given\)"):
        solver.solve_vrp_batch("sp", [good, good, {"durations": D22.tolist(), "locations": _locs(22),
                                                   "capacities": [30], "start_times": [0]}])
    with pytest.raises(ValueError, match=r"^request 0: sp \(set partitioning\) supports at most "
                                         r"64 vehicles"):
        solver.solve_vrp_batch("sp", [(D6.tolist(), _locs(6), [1] * 65, [0] * 65), good])
    big = np.full((6, 6), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_vrp_batch("sp", [good, (big.tolist(), _locs(6), [3, 3], [0, 0])])
    with pytest.raises(ValueError, match=r"^request 0: .*A9 guard"):      # the start time counts
        solver.solve_vrp_batch("sp", [(D6.tolist(), _locs(6), [3, 3], [0, 2**31 - 100])])
    with pytest.raises(ValueError, match=r"^request 0: capacity \+ demand overflows int32"):
        solver.solve_vrp_batch("sp", [(D6.tolist(), _locs(6, demand=2**30), [2**30, 3], [0, 0])])
    with pytest.raises(ValueError, match=r"^request 1: capacities and startTimes"):
        solver.solve_vrp_batch("sp", [good, (D6.tolist(), _locs(6), [3, 3], [0])])
    # the single-request path words the domain errors the same way
    with pytest.raises(ValueError, match=r"^sp \(set partitioning\) needs a static"):
        solver.solve_vrp("sp", td.tolist(), _locs(6), [3, 3], [0, 0])
    assert solver.solve_vrp_batch("sp", []) == []


def _ci(n, K=2, kind="asym", seed=0, starts=None, caps=None):
    N = n + 1
    caps = [n] * K if caps is None else caps
    return solver.compact_vrp(matrix(kind, N, seed), _locs(N), caps, starts or [0] * K)


def test_exact_vrp_batcher_accepts(lib):
    acc = service.ExactVrpBatcher.accepts
    assert acc(_ci(1)) and acc(_ci(10, K=32)) and acc(_ci(12, K=1)) and acc(_ci(9, K=64))
    assert acc(_ci(11, K=12))
    assert not acc(_ci(13, K=1)) and not acc(_ci(12, K=64)) and not acc(_ci(10, K=64))
    none = solver.compact_vrp(matrix("sym", 6, 1), _locs(6), [3], [0], [1, 2, 3, 4, 5])
    assert none.n == 0 and not acc(none)
    td = solver.compact_vrp(np.stack([matrix("sym", 6, 1)] * 24), _locs(6), [3, 3], [0, 0])
    assert not acc(td)
    big = solver.compact_vrp(np.full((6, 6), 2**29, dtype=np.int64), _locs(6), [3, 3], [0, 0])
    assert not acc(big) and not solver.batch_sp_guard(big)
    # the guards count the largest start time, and capacity + demand
    assert acc(_ci(5)) and not acc(_ci(5, starts=[0, 2**31 - 100]))
    heavy = solver.compact_vrp(matrix("sym", 6, 1), _locs(6, demand=2**30), [2**30, 1], [0, 0])
    assert not acc(heavy) and not solver.batch_sp_guard(heavy)


class _FakeApp:
    devices = [0]
    device = 0
    locks = {0: threading.Lock()}


def _fake_answer(ci):
    """Customers in descending order on vehicle 0, the others empty."""
    K = len(ci.capacities)
    return list(range(ci.n, 0, -1)) + [0] * K, [ci.n * 10] + [0] * (K - 1)


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


def test_exact_vrp_batcher_groups_by_nodes_fleet_and_objective(lib):
    seen = []

    def launch(key, cis):
        seen.append((key, len(cis)))
        res = [_fake_answer(ci) for ci in cis]
        return [t for t, _ in res], [d for _, d in res]

    b = service.ExactVrpBatcher(_FakeApp(), window_s=0.2, launch=launch)
    jobs =[(5, 2, "sum")] * 5 + [(5, 3, "sum")] * 3 + [(5, 2, "max")] * 2
    cis = []
    for x, (n, K, _) in enumerate(jobs):      # an ignored customer: nodes are not the identity
        cis.append(solver.compact_vrp(matrix("asym", n + 2, x), _locs(n + 2), [9] * K, [0] * K,
                                      [1 + x % 5]))
    assert all(ci.N == 6 and ci.nodes != list(range(6)) for ci in cis)
    out = _concurrently(lambda x: b.solve(cis[x], jobs[x][2]), len(jobs))
    assert sorted(seen) == [((6, 2, "max"), 2), ((6, 2, "sum"), 5), ((6, 3, "sum"), 3)]
    assert b.launches == 3 and b.requests == 10
    for ci, (n, K, _), res in zip(cis, jobs, out):
        first = [0] + [ci.nodes[c] for c in range(5, 0, -1)] + [0]
        assert res == {"durationMax": 50, "durationSum": 50,
                       "vehicles": [{"tour": first, "duration": 50}] +
                                   [{"tour": [0, 0], "duration": 0}] * (K - 1)}


def test_exact_vrp_batcher_launch_error_reaches_exactly_its_group(lib):
    def launch(key, cis):
        if key == (6, 2, "sum"):
            raise RuntimeError("launch failed")
        res = [_fake_answer(ci) for ci in cis]
        return [t for t, _ in res], [d for _, d in res]

    b = service.ExactVrpBatcher(_FakeApp(), window_s=0.2, launch=launch)
    jobs = [(5, 2, "sum")] * 4 + [(5, 2, "max"), (5, 3, "sum"), (6, 2, "sum")]
    cis = [_ci(n, K, seed=x) for x, (n, K, _) in enumerate(jobs)]
    out = _concurrently(lambda x: b.solve(cis[x], jobs[x][2]), len(jobs))
    assert all(isinstance(o, RuntimeError) and "launch failed" in str(o) for o in out[:4])
    for o, (n, K, _) in zip(out[4:], jobs[4:]):
        assert isinstance(o, dict) and o["vehicles"][0]["tour"] == [0] + list(range(n, 0, -1)) + [0]
        assert len(o["vehicles"]) == K and o["durationSum"] == 10 * n


def _store():
    return service.MemoryStore({}, {}, {})


def _vrp_body(N=6, K=2, seed=4, durations=None, **more):
    D = matrix("asym", N, seed).tolist() if durations is None else durations
    body = {"durations": D, "locations": [{"id": 100 + i, "demand": 1} for i in range(N)],
            "capacities": [N] * K, "startTimes": [5 * k for k in range(K)],
            "ignoredCustomers": [102], "completedCustomers": []}
    return json.dumps(dict(body, **more)).encode()


def test_app_has_no_vrp_batcher_by_default_and_tsp_batcher_is_unchanged():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    app = service.App(_store(), solve=fake)
    assert app.exact_vrp_batcher is None and app.exact_batcher is None and app.batcher is None
    st, res = app.solve_inline("vrp", "sp", _vrp_body())
    assert st == 200 and res["message"] == {"durationMax": 2, "durationSum": 3, "vehicles": []}
    assert seen == [("vrp", "sp")]
    # the TSP batchers group by node count as before, through the same hook
    assert service.TspBatcher.group_key({"ci": _ci(4)}) == 5
    assert service.ExactTspBatcher.group_key({"ci": _ci(7)}) == 8
    launched = []

    def launch(N, cis):
        launched.append((N, len(cis)))
        return [list(range(1, N)) for _ in cis]

    on = service.App(_store(), solve=fake, batch_exact=True, batch_window_s=0.01,
                     batch_exact_launch=launch)
    assert isinstance(on.exact_vrp_batcher, service.ExactVrpBatcher)
    tsp = json.dumps({"durations": matrix("asym", 6, 60).tolist(), "customers": [1, 2, 3, 4, 5],
                      "startNode": 0, "startTime": 7}).encode()
    st, res = on.solve_inline("tsp", "dp", tsp)
    assert st == 200 and res["message"]["vehicle"] == [0, 1, 2, 3, 4, 5, 0]
    assert launched == [(6, 1)] and on.exact_vrp_batcher.launches == 0


def test_app_batch_exact_only_vrp_sp_inline_rides(lib):
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, len(locations)))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    def launch(key, cis):
        launched.append((key, len(cis)))
        res = [_fake_answer(ci) for ci in cis]
        return [t for t, _ in res], [d for _, d in res]

    app = service.App(_store(), solve=fake, batch_exact=True, batch_window_s=0.01,
                      batch_exact_vrp_launch=launch)
    st, res = app.solve_inline("vrp", "sp", _vrp_body(objective="max"))
    # location 102 (row 2) is ignored: compact customers 4..1 are rows 5, 4, 3, 1
    assert st == 200 and res["message"] == {
        "durationMax": 40, "durationSum": 40,
        "vehicles": [{"tour": [0, 5, 4, 3, 1, 0], "duration": 40}, {"tour": [0, 0], "duration": 0}]}
    assert launched == [((5, 2, "max"), 1)] and seen == []
    for algo in ("bf", "sa", "tdsp"):
        assert app.solve_inline("vrp", algo, _vrp_body())[0] == 200
    assert app.solve_inline("vrp", "sp", _vrp_body(N=15))[0] == 200           # 13 customers
    td = np.stack([matrix("sym", 6, 1)] * 24).tolist()
    assert app.solve_inline("vrp", "sp", _vrp_body(durations=td))[0] == 200   # hour-indexed
    assert seen == [("vrp", "bf", 6), ("vrp", "sa", 6), ("vrp", "tdsp", 6), ("vrp", "sp", 15),
                    ("vrp", "sp", 6)]
    assert len(launched) == 1


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_batch(ctx, cases, objective, team=0):
    """One vrp_batch_sp launch -> ([key], [tour], [durs])."""
    import torch
    insts = [inst(c) for c in cases]
    M = torch.tensor(np.stack([D for D, _, _ in insts]), dtype=torch.int32, device=ctx.dev)
    dm = torch.tensor(np.stack([d for _, d, _ in insts]), dtype=torch.int32, device=ctx.dev)
    cp = torch.tensor([list(c) for _, _, c in insts], dtype=torch.int32, device=ctx.dev)
    tours, keys, durs = ctx.vrp_batch_sp(M, dm, cp, obj_id(objective), team)
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("name", REF_CASES)
def test_gpu_equals_reference_alone(ctx, name, objective):
    case = ("ref", name)
    got = gpu_batch(ctx, [case], objective)
    print(name, objective, "gpu", got, "ref", reference(case, objective))
    assert got == expected([case], objective)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_equals_reference_in_mixed_batches(ctx, objective):
    """Every REF_CASES instance again, now between neighbours of its (N, K)
    of the other kinds."""
    groups = {}
    for name in REF_CASES:
        D, _, caps = inst(("ref", name))
        groups.setdefault((D.shape[0] - 1, len(caps)), []).append(("ref", name))
    for (n, K), refs in sorted(groups.items()):
        cases = []
        for x, r in enumerate(refs):
            cases += mixed(n, K, 3)[x % 3:] + [r]
        cases += mixed(n, K, 2)
        assert gpu_batch(ctx, cases, objective) == expected(cases, objective), (n, K)


# every n of the domain, so every boundary of the n -> T table has its two
# sides whatever the table is.  R = 1, and R = 5 and 67: no multiple of 16, 8, 4
# or 2 requests per workgroup, 67 a ragged last workgroup at every team size;
# R = 300 at n = 8, and at n = 11, where a workgroup holds one request and a CU
# one workgroup: more workgroups than are resident at once (the ten distinct
# instances of `mixed` repeat, so the reference costs no more)
SIZES = [(n, 3, R) for n in range(1, 12) for R in (1, 5)] + [(12, 1, 1), (12, 1, 5)] + \
        [(n, 3, 67) for n in range(1, 10)] + [(8, 3, 300), (11, 3, 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,R", SIZES)
def test_gpu_every_n_and_batch_size(ctx, n, K, R):
    cases = mixed(n, K, R)
    objective = OBJECTIVES[(n + R) % 2]
    assert gpu_batch(ctx, cases, objective) == expected(cases, objective)


@pytest.mark.gpu
@pytest.mark.parametrize("n,floor", [(9, 64), (10, 32), (11, 12), (12, 1)])
def test_gpu_lds_edge(ctx, n, floor):
    import torch
    lib = ctx.lib
    K = max(k for k in range(1, 65) if core.vrp_batch_sp_lds(n, k) <= LDS_BYTES)
    assert K >= floor
    objective = OBJECTIVES[n % 2]
    cases = mixed(n, K, 2)
    assert gpu_batch(ctx, cases, objective) == expected(cases, objective)
    if K + 1 > 64:
        return
    R, N = 2, n + 1
    M = torch.zeros((R, N, N), dtype=torch.int32, device=ctx.dev)
    dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
    cp = torch.ones((R, K + 1), dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R, n + K + 1), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R, K + 1), -7, dtype=torch.int32, device=ctx.dev)
    rc = lib.vrpms_vrp_batch_sp(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(), R, N, K + 1,
                                0, 0, tours.data_ptr(), keys.data_ptr(), durs.data_ptr(),
                                ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_sp:" in msg and b"bytes of LDS" in msg
    assert str(lds_bytes(n, K + 1, 256)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item() and (durs == -7).all().item()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 11])
@pytest.mark.parametrize("T", TEAMS)
def test_gpu_every_team_equals_auto_and_reference_or_is_refused(ctx, T, n, K):
    """Every instantiated vrp_batch_sp_kernel<T> at sizes from one customer
    (most of a large team idle through every barrier) to n = 11 (one request
    per workgroup only)."""
    import torch
    lib, N, R = ctx.lib, n + 1, 5
    cases = mixed(n, K, R)
    objective = OBJECTIVES[(n + K + T // 16) % 2]
    want = expected(cases, objective)
    assert gpu_batch(ctx, cases, objective) == want
    if lds_bytes(n, K, T) > LDS_BYTES:
        M = torch.zeros((R, N, N), dtype=torch.int32, device=ctx.dev)
        dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
        cp = torch.ones((R, K), dtype=torch.int32, device=ctx.dev)
        tours = torch.full((R, n + K), -7, dtype=torch.int16, device=ctx.dev)
        keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
        durs = torch.full((R, K), -7, dtype=torch.int32, device=ctx.dev)
        rc = lib.vrpms_vrp_batch_sp(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(), R, N, K,
                                    obj_id(objective), T, tours.data_ptr(), keys.data_ptr(),
                                    durs.data_ptr(), ctx.stream())
        assert rc == _lib.VRPMS_EINVAL
        msg = lib.vrpms_last_error()
        assert b"bytes of LDS" in msg and str(lds_bytes(n, K, T)).encode() in msg
        torch.cuda.synchronize(ctx.dev)
        assert (tours == -7).all().item() and (keys == -7).all().item() and (durs == -7).all().item()
    else:
        assert gpu_batch(ctx, cases, objective, team=T) == want


def test_forced_team_refused_set_is_what_the_lds_formula_gives():
    """Which of the team test's launches are refused: sixteen requests of
    n = 9 per workgroup, and T below 256 at n = 11, except T = 128 with one
    vehicle."""
    over = {(n, K, T) for n in (1, 2, 5, 8, 9, 11) for K in (1, 3) for T in TEAMS
            if lds_bytes(n, K, T) > LDS_BYTES}
    assert over == {(9, 1, 16), (9, 3, 16), (11, 1, 16), (11, 1, 32), (11, 1, 64), (11, 3, 16),
                    (11, 3, 32), (11, 3, 64), (11, 3, 128)}


@pytest.mark.gpu
def test_gpu_bit_equal_to_the_single_request_kernels(ctx):
    import torch
    from vrpms_amd.core import CVRP
    for case, objective in [(("ref", "ties"), "sum"), (("ref", "cap0"), "max"),
                            (("asym", 10, 3, 40), "sum")]:
        D, dem, caps = inst(case)
        ctx.set_instance(CVRP, D, dem, list(caps), [0] * len(caps), objective=obj_id(objective))
        key, tour = runners.set_partition(ctx, D.shape[0] - 1)
        keys, tours, _ = gpu_batch(ctx, [case], objective)
        assert (keys, tours) == ([key], [tour])
    # one ample vehicle: the route is tsp_batch_dp's tour, the key its duration twice
    cases = [(kind, 8, 1, 50 + x) for x, kind in enumerate(KINDS)]
    insts = [inst(c) for c in cases]
    M = torch.tensor(np.stack([D for D, _, _ in insts]), dtype=torch.int32, device=ctx.dev)
    dm = torch.tensor(np.stack([d for _, d, _ in insts]), dtype=torch.int32, device=ctx.dev)
    cp = torch.full((len(cases), 1), 1000, dtype=torch.int32, device=ctx.dev)
    tours, keys, durs = ctx.vrp_batch_sp(M, dm, cp)
    ttours, tkeys = ctx.tsp_batch_dp(M)
    assert tours[:, :8].cpu().tolist() == ttours.cpu().tolist()
    assert tours[:, 8].cpu().tolist() == [0] * len(cases)
    for k, tk, d in zip(keys.cpu().tolist(), tkeys.cpu().tolist(), durs.cpu().tolist()):
        dur = spec.unpack_key(tk)[1]
        assert k == spec.pack_key(0, dur, dur) and d == [dur]


@pytest.mark.gpu
@pytest.mark.parametrize("n,K", [(4, 2), (7, 3), (9, 3)])
def test_gpu_isolation(ctx, n, K):
    cases = mixed(n, K, 11, distinct=11)
    keys, tours, durs = gpu_batch(ctx, cases, "sum")
    assert (keys, tours, durs) == expected(cases, "sum")
    for x, c in enumerate(cases):
        assert gpu_batch(ctx, [c], "sum") == ([keys[x]], [tours[x]], [durs[x]])


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,R", [(3, 2, 5), (8, 3, 7), (12, 1, 3)])
def test_gpu_guard_rows_and_erroring_calls(ctx, n, K, R):
    import torch
    lib, N = ctx.lib, n + 1
    cases = mixed(n, K, R)
    insts = [inst(c) for c in cases]
    M = torch.tensor(np.stack([D for D, _, _ in insts]), dtype=torch.int32, device=ctx.dev)
    dm = torch.tensor(np.stack([d for _, d, _ in insts]), dtype=torch.int32, device=ctx.dev)
    cp = torch.tensor([list(c) for _, _, c in insts], dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R + 1, n + K), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R + 1,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R + 1, K), -7, dtype=torch.int32, device=ctx.dev)

    def run(c=ctx.handle, m=M.data_ptr(), d=dm.data_ptr(), p=cp.data_ptr(), r=R, nn=N, kk=K,
            obj=0, team=0, t=tours.data_ptr(), k=keys.data_ptr(), du=durs.data_ptr()):
        return lib.vrpms_vrp_batch_sp(c, m, d, p, r, nn, kk, obj, team, t, k, du, ctx.stream())

    def untouched(rows=slice(None)):
        torch.cuda.synchronize(ctx.dev)
        return (tours[rows] == -7).all().item() and (keys[rows] == -7).all().item() and \
            (durs[rows] == -7).all().item()

    for bad in (dict(c=None), dict(r=-1), dict(nn=1), dict(nn=14), dict(kk=0), dict(kk=65),
                dict(obj=2), dict(team=24), dict(m=None), dict(d=None), dict(p=None), dict(t=None),
                dict(k=None), dict(du=None)):
        assert run(**bad) == _lib.VRPMS_EINVAL, bad
        assert b"vrpms_vrp_batch_sp:" in lib.vrpms_last_error()
    assert untouched()
    assert run(r=0) == _lib.VRPMS_OK
    assert untouched()
    assert run() == _lib.VRPMS_OK
    torch.cuda.synchronize(ctx.dev)
    wkeys, wtours, wdurs = expected(cases, "sum")
    assert tours[:R].cpu().tolist() == wtours and durs[:R].cpu().tolist() == wdurs
    assert [int(k) & (2**64 - 1) for k in keys[:R].cpu().tolist()] == wkeys
    assert untouched(slice(R, R + 1))


def _clamp_matrix():
    D = np.full((3, 3), 2**27, dtype=np.int64)
    np.fill_diagonal(D, 0)
    D[2, 1] += 5                          # 0 -> 1 -> 2 -> 0 is the one optimum of one vehicle
    return D


@pytest.mark.gpu
def test_gpu_key_clamps_and_durs_and_solve_vrp_batch_report_the_durations(ctx):
    import torch
    D = _clamp_matrix()
    assert 3 * 2**27 > 2**28 and (3 + 2 + 1) * int(D.max()) < 2**31
    M = torch.tensor(D[None], dtype=torch.int32, device=ctx.dev)
    dm = torch.tensor([[0, 1, 1]], dtype=torch.int32, device=ctx.dev)
    for caps, objective, wtour, wdurs in [([2, 0], "sum", [1, 2, 0, 0], [3 * 2**27, 0]),
                                          ([1, 1], "max", [2, 0, 1, 0], [2**28, 2**28])]:
        cp = torch.tensor([caps], dtype=torch.int32, device=ctx.dev)
        tours, keys, durs = ctx.vrp_batch_sp(M, dm, cp, obj_id(objective))
        ref = sp_ref(D, [0, 1, 1], caps, objective)
        assert (tours.cpu().tolist(), durs.cpu().tolist()) == ([wtour], [wdurs])
        assert (ref["tour"], ref["durations"]) == (wtour, wdurs)
        key = int(keys.cpu().item()) & (2**64 - 1)
        assert key == ref["key"] and (key >> 28) & (2**28 - 1) == 2**28 - 1
        req = (D.tolist(), _locs(3), caps, [0, 0])
        res = solver.solve_vrp_batch("sp", [req], objective=objective)
        assert res == [solver.solve_vrp("sp", *req, objective=objective)]
        assert res[0]["durationSum"] == sum(wdurs) and res[0]["durationMax"] == max(wdurs)
        assert [v["duration"] for v in res[0]["vehicles"]] == wdurs


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_batch_equals_the_list_comprehension(objective):
    D12 = matrix("asym", 12, 30)
    locs12 = [{"id": 100 + i, "demand": int(d)} for i, d in enumerate(demands(11, 30, 1, 4))]
    D14 = matrix("sym", 14, 31)
    D13 = matrix("asym", 13, 32)
    reqs = [(matrix("asym", 6, 33).tolist(), _locs(6), [3, 2], [0, 5]),
            (D12.tolist(), locs12, [7, 6, 5], [0, 15, 30], [102, 105], [107, 110]),
            (D12.tolist(), locs12, [7, 6], [0, 0], [100 + i for i in range(1, 12)]),   # none active
            (D14.tolist(), _locs(14), [5, 5, 5], [0, 0, 0]),                # 13: single path
            (D13.tolist(), _locs(13), [5, 4, 4], [0, 0, 0]),                # (12, 3): beyond the LDS
            (matrix("ties", 6, 34).tolist(), _locs(6), [2, 2], [3, 3]),     # unserved customers
            {"durations": matrix("sym", 9, 35).tolist(), "locations": _locs(9),
             "capacities": [4, 0, 5], "start_times": [0, 0, 0], "ignored_customers": [3]},
            (matrix("asym", 6, 36).tolist(), _locs(6), [3, 2], [0, 5])]     # a second of (6, 2)
    assert core.vrp_batch_sp_lds(12, 3) > LDS_BYTES
    for with_unvisited in (False, True):
        want = [solver.solve_vrp("sp", *((r["durations"], r["locations"], r["capacities"],
                                          r["start_times"], r["ignored_customers"])
                                         if isinstance(r, dict) else r),
                                 objective=objective, with_unvisited=with_unvisited) for r in reqs]
        got = solver.solve_vrp_batch("sp", reqs, objective=objective, with_unvisited=with_unvisited)
        assert got == want
        assert ("unvisited" in got[0]) == with_unvisited
    assert got[5]["unvisited"] and got[2]["vehicles"] == [{"tour": [0, 0], "duration": 0}] * 2


@pytest.mark.gpu
def test_service_batch_exact_vrp_equals_the_unbatched_answers():
    on = service.App(_store(), batch_exact=True, batch_window_s=0.05)
    off = service.App(_store())
    calls = []
    for x in range(24):
        N, K = (7, 10)[x % 2], (2, 3)[(x // 2) % 2]
        more = {"objective": "max"} if x % 8 >= 4 else {}
        calls.append(_vrp_body(N, K, seed=60 + x, **more))
    out = _concurrently(lambda x: on.solve_inline("vrp", "sp", calls[x]), len(calls))
    assert on.exact_vrp_batcher.requests == 24
    assert 1 <= on.exact_vrp_batcher.launches < on.exact_vrp_batcher.requests
    for body, got in zip(calls, out):
        want = off.solve_inline("vrp", "sp", body)
        assert want[0] == 200 and got == want
