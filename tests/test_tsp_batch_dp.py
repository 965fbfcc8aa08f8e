"""Batched exact TSP (spec A18): the C entry point vrpms_tsp_batch_dp,
Context.tsp_batch_dp, solver.solve_tsp_batch and the service's exact batcher
(App(batch_exact=True)).

The reference is a numpy Held-Karp in this file (A14's recurrence and
lexicographically smallest walk), itself checked against
itertools.permutations + the spec's evaluator; per request the GPU must return
the identical key and tour, and the identical key and tour as the
single-request Held-Karp and the brute-force kernels."""
import ctypes
import functools
import itertools
import json
import threading

import numpy as np
import pytest

from oracle import spec
from vrpms_amd import _lib, runners, service, solver, synth

INF = np.int64(1) << 60


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def held_karp_ref(D):
    """(duration, lexicographically smallest optimal tour) over customers
    1..n of the static matrix D (node 0 = start node)."""
    D = np.asarray(D, dtype=np.int64)
    n = D.shape[0] - 1
    full = 1 << n
    masks = np.arange(full, dtype=np.int64)
    pc = np.zeros(full, dtype=np.int64)
    for i in range(n):
        pc += (masks >> i) & 1
    g = np.full((full, n), INF, dtype=np.int64)      # g[S][j - 1], j not in S
    g[0] = D[1:n + 1, 0]
    for k in range(1, n):
        Ss = masks[pc == k]
        best = np.full((Ss.shape[0], n), INF, dtype=np.int64)
        for i in range(n):
            idx = np.nonzero((Ss >> i) & 1)[0]
            cand = g[Ss[idx] ^ (1 << i), i][:, None] + D[1:n + 1, i + 1][None, :]   # D[j][i]
            best[idx] = np.minimum(best[idx], cand)
        g[Ss] = best
    S, cur, tour, total = full - 1, 0, [], None
    for _ in range(n):
        members = [i for i in range(n) if (S >> i) & 1]
        vals = [int(D[cur, i + 1] + g[S ^ (1 << i), i]) for i in members]
        if total is None:
            total = min(vals)
        i = members[vals.index(min(vals))]           # smallest i attaining g[S][cur]
        tour.append(i + 1)
        cur, S = i + 1, S ^ (1 << i)
    return total, tour


def permutation_optimum(D, n):
    """(min duration, first minimising permutation in lexicographic order)."""
    perms = np.array(list(itertools.permutations(range(1, n + 1))), dtype=np.int64)
    durs = spec.eval_tsp_batch(D, perms)
    r = int(np.argmin(durs))                          # first minimum = lex-smallest
    assert int(durs[r]) == spec.eval_tsp(D, perms[r])
    return int(durs[r]), perms[r].tolist()


KINDS = ("sym", "asym", "ties", "zero", "big")


@functools.lru_cache(maxsize=None)
def _matrix(kind, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "sym":
        D = synth.random_symmetric(N, rng).astype(np.int64)
    elif kind == "asym":
        D = rng.integers(3, 321, size=(N, N), dtype=np.int64)
    elif kind == "ties":
        D = rng.integers(1, 3, size=(N, N), dtype=np.int64)
    elif kind == "zero":
        D = np.zeros((N, N), dtype=np.int64)
    elif kind == "big":                  # entries above 65,535; N * max < 2^31
        D = rng.integers(60000, 9000000, size=(N, N), dtype=np.int64)
    else:
        raise ValueError(kind)
    np.fill_diagonal(D, 0)
    D.setflags(write=False)
    return D


def matrix(kind, N, seed):
    return _matrix(kind, N, seed)


@functools.lru_cache(maxsize=None)
def reference(kind, N, seed):
    """Computed once per matrix and shared by the tests."""
    dur, tour = held_karp_ref(matrix(kind, N, seed))
    return dur, tuple(tour)


def mixed(N, R, seed=0):
    """R (kind, N, seed) triples cycling through KINDS: neighbours in a
    workgroup differ in kind."""
    return [(KINDS[(x + seed) % len(KINDS)], N, 100 * N + (x + seed) // len(KINDS)) for x in range(R)]


def planted(n, seed):
    """Entries uniform in 4..320, the edges of one hidden directed cycle
    through all n + 1 nodes set to 3: that cycle (duration 3 (n + 1)) is the
    unique optimum, any other has an edge >= 4 and none below 3."""
    rng = np.random.default_rng(seed)
    N = n + 1
    D = rng.integers(4, 321, size=(N, N), dtype=np.int64)
    np.fill_diagonal(D, 0)
    hidden = (rng.permutation(n) + 1).tolist()
    path = [0] + hidden + [0]
    for a, b in zip(path, path[1:]):
        D[a, b] = 3
    return D, hidden


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,seed", [("ties", 2, 0), ("ties", 5, 1), ("ties", 7, 2),
                                         ("asym", 8, 3)])
def test_reference_equals_permutation_optimum(kind, n, seed):
    D = matrix(kind, n + 1, seed)
    assert held_karp_ref(D) == permutation_optimum(D, n)


def test_reference_all_zero_matrix_gives_identity_tour():
    assert held_karp_ref(matrix("zero", 8, 0)) == (0, list(range(1, 8)))


def test_planted_cycle_is_the_spec_optimum_value():
    D, hidden = planted(12, 5)
    assert spec.eval_tsp(D, hidden) == 39
    assert D[~np.eye(13, dtype=bool)].min() == 3 and (D == 3).sum() == 13


@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


def test_argument_errors_need_no_gpu(lib):
    """Every argument check comes before the context is looked at, so a
    stand-in block of zeros serves as the non-NULL ctx here."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(4096)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    f = lib.vrpms_tsp_batch_dp
    assert f(None, p, 1, 5, p, p, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_tsp_batch_dp" in lib.vrpms_last_error() and b"ctx is NULL" in lib.vrpms_last_error()
    assert f(c, p, -1, 5, p, p, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_tsp_batch_dp" in lib.vrpms_last_error()
    for N in (-1, 0, 1, 14, 50):
        assert f(c, p, 1, N, p, p, None) == _lib.VRPMS_EINVAL
        assert b"vrpms_tsp_batch_dp" in lib.vrpms_last_error()
        assert b"2 <= N <= 13" in lib.vrpms_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert f(c, args[0], 1, 5, args[1], args[2], None) == _lib.VRPMS_EINVAL
        assert b"vrpms_tsp_batch_dp" in lib.vrpms_last_error() and b"NULL" in lib.vrpms_last_error()
    assert f(c, None, 0, 5, None, None, None) == _lib.VRPMS_OK
    assert f(c, p, 0, 13, p, p, None) == _lib.VRPMS_OK


def _no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(solver, "context", boom)
    monkeypatch.setattr(solver, "Context", boom)


def test_solve_tsp_batch_refusals_need_no_gpu(monkeypatch):
    _no_gpu(monkeypatch)
    good = (matrix("sym", 6, 0).tolist(), [1, 2, 3, 4, 5], 0, 0)
    with pytest.raises(ValueError, match="'sa'"):
        solver.solve_tsp_batch("sa", [good])
    td = np.stack([matrix("sym", 6, 1)] * 24)
    with pytest.raises(ValueError, match=r"^request 1: dp \(Held-Karp\) needs a static"):
        solver.solve_tsp_batch("dp", [good, (td.tolist(), [1, 2, 3, 4, 5], 0, 0)])
    D25 = matrix("sym", 26, 0)
    with pytest.raises(ValueError, match=r"^request 2: dp \(Held-Karp\) supports at most 24"):
        solver.solve_tsp_batch("dp", [good, good, {"durations": D25.tolist(),
                                                   "customers": list(range(1, 26)),
                                                   "start_node": 0, "start_time": 0}])
    big = np.full((6, 6), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 0: .*A9 guard"):
        solver.solve_tsp_batch("dp", [(big.tolist(), [1, 2, 3, 4, 5], 0, 0), good])
    # the single-request path words the first two the same way
    with pytest.raises(ValueError, match=r"^dp \(Held-Karp\) needs a static"):
        solver.solve_tsp("dp", td.tolist(), [1, 2, 3, 4, 5], 0)
    with pytest.raises(ValueError, match=r"^dp \(Held-Karp\) supports at most 24"):
        solver.solve_tsp("dp", D25.tolist(), list(range(1, 26)), 0)
    assert solver.solve_tsp_batch("dp", []) == []
    assert solver.BATCH_DP_MAX_CUSTOMERS == 12
    assert "dp" in solver.ALGORITHMS and solver.DP_MAX_CUSTOMERS == 24


def _ci(N, kind="asym", seed=0, start_time=0):
    return solver.compact_tsp(matrix(kind, N, seed), list(range(1, N)), 0, start_time)


class _FakeApp:
    devices = [0]
    device = 0
    locks = {0: threading.Lock()}


def test_exact_batcher_accepts():
    acc = service.ExactTspBatcher.accepts
    assert acc(_ci(2)) and acc(_ci(13))                 # 1 and 12 customers
    assert not acc(_ci(1)) and not acc(_ci(14))         # 0 and 13 customers
    td = solver.compact_tsp(np.stack([matrix("sym", 6, 1)] * 24), [1, 2, 3, 4, 5], 0, 0)
    assert not acc(td)
    big = solver.compact_tsp(np.full((6, 6), 2**29, dtype=np.int64), [1, 2, 3, 4, 5], 0, 0)
    assert not acc(big)
    # the guard counts the start time, as vrpms_set_instance does
    assert acc(_ci(6)) and not acc(_ci(6, start_time=2**31 - 100))


def test_exact_batcher_groups_by_node_count_one_launch_each():
    seen = []

    def launch(N, cis):
        seen.append((N, len(cis)))
        return [list(range(N - 1, 0, -1)) for _ in cis]      # tours only: durations on the host

    b = service.ExactTspBatcher(_FakeApp(), window_s=0.2, launch=launch)
    cis = [_ci(5, seed=x) for x in range(5)] + [_ci(8, seed=x) for x in range(3)]
    out = [None] * len(cis)

    def go(x):
        out[x] = b.solve(cis[x])

    ths = [threading.Thread(target=go, args=(x,)) for x in range(len(cis))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert sorted(seen) == [(5, 5), (8, 3)]
    assert b.launches == 2 and b.requests == 8
    for ci, res in zip(cis, out):
        path = [0] + list(range(ci.N - 1, 0, -1)) + [0]
        assert res["vehicle"] == path
        assert res["duration"] == sum(int(ci.durations[0][a][c]) for a, c in zip(path, path[1:]))


def test_exact_batcher_launch_error_reaches_every_waiter_of_its_group():
    def launch(N, cis):
        if N == 5:
            raise RuntimeError("launch failed")
        return [list(range(1, N)) for _ in cis]

    b = service.ExactTspBatcher(_FakeApp(), window_s=0.2, launch=launch)
    cis = [_ci(5, seed=x) for x in range(4)] + [_ci(7)]
    out = [None] * len(cis)

    def go(x):
        try:
            out[x] = b.solve(cis[x])
        except RuntimeError as e:
            out[x] = e

    ths = [threading.Thread(target=go, args=(x,)) for x in range(len(cis))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert all(isinstance(o, RuntimeError) and "launch failed" in str(o) for o in out[:4])
    assert out[4]["vehicle"] == [0, 1, 2, 3, 4, 5, 6, 0]


def _store():
    return service.MemoryStore({"L7": [{"id": i} for i in range(7)],
                                "L10": [{"id": i} for i in range(10)]},
                               {"D7": matrix("asym", 7, 50).tolist(),
                                "D10": matrix("ties", 10, 51).tolist()}, {})


def _bf_body(N):
    return json.dumps({"solutionName": "s", "solutionDescription": "d", "locationsKey": f"L{N}",
                       "durationsKey": f"D{N}", "customers": list(range(1, N)), "startNode": 0,
                       "startTime": 0}).encode()


def _dp_body(N, seed=60, start=0, customers=None):
    return json.dumps({"durations": matrix("asym", N, seed).tolist(),
                       "customers": customers or list(range(1, N)), "startNode": start,
                       "startTime": 7}).encode()


def test_app_has_no_exact_batcher_by_default_and_routes_unchanged():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, params["customers"]))
        return {"duration": 1, "vehicle": [0, 1, 0]}

    app = service.App(_store(), solve=fake)
    assert app.exact_batcher is None and app.batcher is None
    st, res = app.solve_inline("tsp", "dp", _dp_body(6))
    assert st == 200 and res["message"] == {"duration": 1, "vehicle": [0, 1, 0]}
    st, res = app.post("tsp", "bf", _bf_body(7))
    assert st == 200 and res["message"] == {"duration": 1, "vehicle": [0, 1, 0]}
    assert seen == [("tsp", "dp", [1, 2, 3, 4, 5]), ("tsp", "bf", [1, 2, 3, 4, 5, 6])]


def test_app_batch_exact_rides_only_what_accepts_says():
    """With the batcher on: dp inline and bf on the endpoint ride the injected
    launch; 13 customers, sa and an hour-indexed matrix reach `solve`."""
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm))
        return {"duration": 1, "vehicle": [0, 1, 0]}

    def launch(N, cis):
        launched.append((N, len(cis)))
        return [list(range(1, N)) for _ in cis]

    app = service.App(_store(), solve=fake, batch_exact=True, batch_window_s=0.01,
                      batch_exact_launch=launch)
    st, res = app.solve_inline("tsp", "dp", _dp_body(6))
    assert st == 200 and res["message"]["vehicle"] == [0, 1, 2, 3, 4, 5, 0]
    st, res = app.post("tsp", "bf", _bf_body(7))
    assert st == 200 and res["message"]["vehicle"] == [0, 1, 2, 3, 4, 5, 6, 0]
    assert launched == [(6, 1), (7, 1)] and seen == []
    assert app.solve_inline("tsp", "dp", _dp_body(14))[0] == 200
    assert app.post("tsp", "sa", _bf_body(7))[0] == 200
    td = json.dumps({"durations": np.stack([matrix("sym", 6, 1)] * 24).tolist(),
                     "customers": [1, 2, 3], "startNode": 0, "startTime": 0}).encode()
    assert app.solve_inline("tsp", "dp", td)[0] == 200
    assert seen == [("tsp", "dp"), ("tsp", "sa"), ("tsp", "dp")] and len(launched) == 2


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_batch(ctx, mats):
    """mats: list of [N][N] -> ([key], [tour]) of one tsp_batch_dp launch."""
    import torch
    M = torch.tensor(np.stack([np.asarray(m) for m in mats]), dtype=torch.int32, device=ctx.dev)
    tours, keys = ctx.tsp_batch_dp(M)
    return [int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist()


def expected(cases):
    refs = [reference(*c) for c in cases]
    return [spec.tsp_key(d) for d, _ in refs], [list(t) for _, t in refs]


# every n of the domain, so every boundary of the n -> T table has its two
# sides whatever the table is: n = 1 and 2 (no layer, one layer), 5 and 6,
# 12 (dynamic LDS above 64 KiB).  R = 1, and R = 5 and 67: no multiple of 16,
# 8, 4 or 2 requests per workgroup, 67 several workgroups with a ragged last.
# The numpy reference bounds R at the large n.
CASES = [(n, R) for n in range(1, 13) for R in (1, 5)] + \
        [(n, 67) for n in (1, 2, 5, 6, 7, 8, 9)] + [(10, 35), (11, 13)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,R", CASES)
def test_gpu_equals_reference(ctx, n, R):
    cases = mixed(n + 1, R, seed=R)
    keys, tours = gpu_batch(ctx, [matrix(*c) for c in cases])
    wkeys, wtours = expected(cases)
    assert tours == wtours
    assert keys == wkeys
    for c, t in zip(cases, tours):
        if c[0] == "zero":
            assert t == list(range(1, n + 1))


@pytest.mark.gpu
def test_gpu_more_workgroups_than_the_chip_holds(ctx):
    """R = 600 at n = 12: one workgroup per request, one per CU at a time."""
    made = [planted(12, 1000 + x) for x in range(600)]
    keys, tours = gpu_batch(ctx, [D for D, _ in made])
    assert tours == [h for _, h in made]
    assert keys == [spec.tsp_key(39)] * 600


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 7, 9])
def test_gpu_isolation(ctx, n):
    cases = mixed(n + 1, 11, seed=3)
    mats = [matrix(*c) for c in cases]
    keys, tours = gpu_batch(ctx, mats)
    for x, m in enumerate(mats):
        k1, t1 = gpu_batch(ctx, [m])
        assert (k1[0], t1[0]) == (keys[x], tours[x])


@pytest.mark.gpu
@pytest.mark.parametrize("n,R", [(3, 5), (8, 7), (12, 3)])
def test_gpu_guard_row_and_erroring_calls(ctx, n, R):
    import torch
    lib, N = ctx.lib, n + 1
    cases = mixed(N, R, seed=1)
    M = torch.tensor(np.stack([matrix(*c) for c in cases]), dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R + 1, n), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R + 1,), -7, dtype=torch.int64, device=ctx.dev)

    def run(c=ctx.handle, m=M.data_ptr(), r=R, nn=N, t=tours.data_ptr(), k=keys.data_ptr()):
        return lib.vrpms_tsp_batch_dp(c, m, r, nn, t, k, ctx.stream())

    assert run(c=None) == _lib.VRPMS_EINVAL
    assert run(r=-1) == _lib.VRPMS_EINVAL
    assert run(nn=1) == _lib.VRPMS_EINVAL and run(nn=14) == _lib.VRPMS_EINVAL
    assert b"2 <= N <= 13" in lib.vrpms_last_error()
    assert run(m=None) == _lib.VRPMS_EINVAL and run(t=None) == _lib.VRPMS_EINVAL
    assert run(k=None) == _lib.VRPMS_EINVAL
    assert run(r=0) == _lib.VRPMS_OK
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item()
    assert run() == _lib.VRPMS_OK
    torch.cuda.synchronize(ctx.dev)
    wkeys, wtours = expected(cases)
    assert tours[:R].cpu().tolist() == wtours
    assert [int(k) & (2**64 - 1) for k in keys[:R].cpu().tolist()] == wkeys
    assert tours[R].cpu().tolist() == [-7] * n and keys[R].cpu().item() == -7


@pytest.mark.gpu
def test_gpu_agrees_with_the_single_request_kernels(ctx):
    from vrpms_amd.core import TSP
    for kind, N, seed in [("ties", 8, 70), ("asym", 12, 71), ("sym", 13, 72)]:
        D = matrix(kind, N, seed)
        ctx.set_instance(TSP, D, start_times=(0,))
        key, tour = runners.held_karp(ctx, N - 1)
        assert gpu_batch(ctx, [D]) == ([key], [tour])
    for kind, N, seed in [("ties", 10, 73), ("asym", 11, 74)]:       # n = 9 and 10
        D = matrix(kind, N, seed)
        ctx.set_instance(TSP, D, start_times=(0,))
        key, tour = runners.brute_force(ctx, N - 1)
        assert gpu_batch(ctx, [D]) == ([key], [tour])


def _clamp_matrix():
    D = np.full((3, 3), 2**27, dtype=np.int64)
    np.fill_diagonal(D, 0)
    D[2, 1] += 5                          # 0 -> 1 -> 2 -> 0 is the one optimum
    return D


@pytest.mark.gpu
def test_gpu_key_clamps_and_solve_tsp_batch_reports_the_duration(ctx):
    D = _clamp_matrix()
    assert 3 * 2**27 > 2**28 and 3 * int(D.max()) < 2**31
    keys, tours = gpu_batch(ctx, [D])
    assert tours == [[1, 2]]
    assert keys == [spec.tsp_key(3 * 2**27)] and (keys[0] >> 28) == 2**28 - 1
    res = solver.solve_tsp_batch("dp", [(D.tolist(), [1, 2], 0, 0)])
    assert res == [{"duration": 3 * 2**27, "vehicle": [0, 1, 2, 0]}]
    assert res == [solver.solve_tsp("dp", D.tolist(), [1, 2], 0, 0)]


@pytest.mark.gpu
def test_solve_tsp_batch_equals_the_list_comprehension():
    D9, D14 = matrix("sym", 9, 80), matrix("asym", 14, 81)
    reqs = [(matrix("asym", 6, 82).tolist(), [1, 2, 3, 4, 5], 0, 0),
            (D9.tolist(), [1, 3, 4, 6, 7, 8], 5, 30),              # a subset, start node 5
            (D9.tolist(), [], 2, 0),                               # no customer
            (D9.tolist(), [4], 2, 11),                             # one customer
            (D14.tolist(), list(range(1, 14)), 0, 0),              # 13 customers: single path
            (matrix("ties", 6, 83).tolist(), [5, 4, 3, 2, 1], 0, 3),
            {"durations": matrix("big", 9, 84).tolist(), "customers": list(range(1, 9)),
             "start_node": 0, "start_time": 0},
            (_clamp_matrix().tolist(), [1, 2], 0, 0)]
    want = [solver.solve_tsp("dp", *((r["durations"], r["customers"], r["start_node"],
                                      r["start_time"]) if isinstance(r, dict) else r))
            for r in reqs]
    assert solver.solve_tsp_batch("dp", reqs) == want


@pytest.mark.gpu
def test_service_batch_exact_equals_the_unbatched_answers():
    on = service.App(_store(), batch_exact=True, batch_window_s=0.05)
    off = service.App(_store())
    calls = []
    for x in range(24):
        N = (7, 10)[x % 2]
        if x % 4 < 2:
            calls.append(("inline", "dp", _dp_body(N, seed=60 + x)))
        else:
            calls.append(("post", "bf", _bf_body(N)))
    out = [None] * len(calls)

    def go(x):
        kind, algo, body = calls[x]
        out[x] = on.solve_inline("tsp", algo, body) if kind == "inline" else \
            on.post("tsp", algo, body)

    ths = [threading.Thread(target=go, args=(x,)) for x in range(len(calls))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert on.exact_batcher.requests == 24
    assert 1 <= on.exact_batcher.launches < on.exact_batcher.requests
    for (kind, algo, body), got in zip(calls, out):
        want = off.solve_inline("tsp", algo, body) if kind == "inline" else \
            off.post("tsp", algo, body)
        assert want[0] == 200 and got == want


# ---------------------------------------------------------------------------
# VRPMS_OPT_BATCH_DP_TEAM: every tsp_batch_dp_kernel<T> at every n, not only
# the n -> T pairs of the launcher's table (which never picks T = 64)
# ---------------------------------------------------------------------------
TEAMS = (16, 32, 64, 128, 256)
TEAM_NS = (1, 2, 5, 8, 9, 10, 11, 12)
LDS_BYTES = 160 * 1024
# 256 / T tables of n 2^(n-1) words do not fit next to each other
TEAM_REFUSED = {(10, 16), (10, 32), (11, 16), (11, 32), (11, 64),
                (12, 16), (12, 32), (12, 64), (12, 128)}


def batch_dp_lds_bytes(n, T):
    """tsp_batch_dp.hip batch_dp_lds_bytes: the binomial table (172 words),
    then per team the 13 x 16-word matrix image and the table padded to four
    words."""
    pad4 = ((n << (n - 1)) + 3) & ~3
    return (172 + (256 // T) * (208 + pad4)) * 4


def test_forced_team_refused_set_is_what_the_lds_formula_gives():
    over = {(n, T) for n in range(1, 13) for T in TEAMS if batch_dp_lds_bytes(n, T) > LDS_BYTES}
    assert over == TEAM_REFUSED
    assert batch_dp_lds_bytes(9, 16) == 161456 <= LDS_BYTES       # the tightest fit
    assert batch_dp_lds_bytes(12, 256) == 99824                   # the auto choice at n = 12


@pytest.mark.gpu
@pytest.mark.parametrize("n,R", [(n, 5) for n in TEAM_NS] + [(8, 67)])
@pytest.mark.parametrize("T", TEAMS)
def test_gpu_forced_team_equals_reference_and_auto_or_is_refused(ctx, T, n, R):
    """T = 256 at n = 1 and 2 leaves most of a team idle through every
    barrier; (n = 9, T = 16) fills the LDS to 161,456 of 163,840 B; R = 67 at
    T = 16 is five workgroups, the last with three of its sixteen teams."""
    import torch
    lib, N = ctx.lib, n + 1
    cases = mixed(N, R, seed=R)
    mats = [matrix(*c) for c in cases]
    auto = gpu_batch(ctx, mats)
    wkeys, wtours = expected(cases)
    assert auto == (wkeys, wtours)
    ctx.set_batch_dp_team(T)
    try:
        if (n, T) in TEAM_REFUSED:
            M = torch.tensor(np.stack(mats), dtype=torch.int32, device=ctx.dev)
            tours = torch.full((R, n), -7, dtype=torch.int16, device=ctx.dev)
            keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
            rc = lib.vrpms_tsp_batch_dp(ctx.handle, M.data_ptr(), R, N, tours.data_ptr(),
                                        keys.data_ptr(), ctx.stream())
            assert rc == _lib.VRPMS_EINVAL
            msg = lib.vrpms_last_error()
            assert b"vrpms_tsp_batch_dp" in msg and b"bytes of LDS" in msg
            assert str(batch_dp_lds_bytes(n, T)).encode() in msg
            torch.cuda.synchronize(ctx.dev)
            assert (tours == -7).all().item() and (keys == -7).all().item()
        else:
            assert batch_dp_lds_bytes(n, T) <= LDS_BYTES
            forced = gpu_batch(ctx, mats)
            assert forced[1] == wtours and forced[0] == wkeys
            assert forced == auto
    finally:
        ctx.set_batch_dp_team(0)
    assert gpu_batch(ctx, mats[:1]) == (wkeys[:1], wtours[:1])      # auto again
