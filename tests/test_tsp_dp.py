"""Exact TSP by Held-Karp subset DP (algorithm "dp", spec A14): the C entry
points vrpms_tsp_dp_workspace / vrpms_tsp_dp_run, Context.tsp_dp,
runners.held_karp, solver.solve_tsp("dp") and the inline route
POST /solve/tsp/dp.

The reference is a numpy Held-Karp in this file (same recurrence, same
lexicographically-smallest walk, vectorised per layer), itself checked
against itertools.permutations + the spec's evaluator; the GPU must return
the identical key and tour, and the identical key and tour as the brute-force
kernel wherever both run."""
import ctypes
import itertools
import json
import multiprocessing as mp
import socket
import threading

import numpy as np
import pytest

from oracle import spec
from vrpms_amd import _lib, frontends, remote, runners, service, solver, synth

INF = np.int64(1) << 60


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def held_karp_ref(D, n=None):
    """(duration, lexicographically smallest optimal tour) over customers
    1..n of the static matrix D (node 0 = start node)."""
    D = np.asarray(D, dtype=np.int64)
    n = D.shape[0] - 1 if n is None else n
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


def matrix(kind, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "sym":
        return synth.random_symmetric(N, rng)
    if kind == "asym":
        D = rng.integers(3, 321, size=(N, N), dtype=np.int64)
    elif kind == "ties":
        D = rng.integers(1, 3, size=(N, N), dtype=np.int64)
    elif kind == "zero":
        return np.zeros((N, N), dtype=np.int64)
    else:
        raise ValueError(kind)
    np.fill_diagonal(D, 0)
    return D


def planted(n=24, seed=7):
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
    D, hidden = planted()
    assert spec.eval_tsp(D, hidden) == 75
    assert D[~np.eye(25, dtype=bool)].min() == 3 and (D == 3).sum() == 25


@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


def test_workspace_size(lib):
    b = ctypes.c_uint64()
    assert lib.vrpms_tsp_dp_workspace(0, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    assert b"1 <= n <= 24" in lib.vrpms_last_error()
    assert lib.vrpms_tsp_dp_workspace(25, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    prev = 0
    for n in range(1, 25):
        assert lib.vrpms_tsp_dp_workspace(n, ctypes.byref(b)) == _lib.VRPMS_OK
        assert b.value >= prev and b.value >= (1 << n) * n * 4
        prev = b.value
    assert prev == 2 << 30


def test_run_rejects_null_ctx_before_any_hip_call(lib):
    assert lib.vrpms_tsp_dp_run(None, 5, None, 0, None, None, None) == _lib.VRPMS_EINVAL
    assert b"ctx is NULL" in lib.vrpms_last_error()


def test_front_end_errors_need_no_gpu():
    D25 = matrix("sym", 26, 0)
    with pytest.raises(ValueError, match="at most 24"):
        solver.solve_tsp("dp", D25.tolist(), list(range(1, 26)), 0)
    td = np.stack([matrix("sym", 6, 1)] * 24)
    with pytest.raises(ValueError, match="static"):
        solver.solve_tsp("dp", td.tolist(), [1, 2, 3, 4, 5], 0)
    locs = [{"id": i} for i in range(6)]
    with pytest.raises(ValueError, match="dp solves the TSP only"):
        solver.solve_vrp("dp", matrix("sym", 6, 1).tolist(), locs, [9], [0])
    assert "dp" in solver.ALGORITHMS and solver.DP_MAX_CUSTOMERS == 24
    assert solver.BF_MAX_CUSTOMERS == 13 and solver.BF_MAX_CUSTOMERS_TD == 11


def _store():
    return service.MemoryStore({}, {}, {})


def _inline_body(N=6):
    return json.dumps({"durations": matrix("asym", N, 4).tolist(), "customers": list(range(1, N)),
                       "startNode": 0, "startTime": 0}).encode()


def test_solve_inline_routes_tsp_dp_and_refuses_vrp_dp():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, params["customers"]))
        return {"duration": 1, "vehicle": [0, 1, 0]}

    app = service.App(_store(), solve=fake)
    st, res = app.solve_inline("tsp", "dp", _inline_body())
    assert st == 200 and res == {"success": True, "message": {"duration": 1, "vehicle": [0, 1, 0]}}
    assert seen == [("tsp", "dp", [1, 2, 3, 4, 5])]
    vrp = json.dumps({"durations": [[0, 1], [1, 0]], "locations": [{"id": 0}, {"id": 1}],
                      "capacities": [1], "startTimes": [0], "ignoredCustomers": [],
                      "completedCustomers": []}).encode()
    st, res = app.solve_inline("vrp", "dp", vrp)
    assert st == 400 and "no solver /solve/vrp/dp" in res["errors"][0]["reason"]
    assert len(seen) == 1
    # the eight endpoints stay the reference's wire contract
    assert sorted(service.TITLES) == ["aco", "bf", "ga", "sa"]


def test_remote_forwards_dp_to_the_inline_route():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm))
        return {"duration": 7, "vehicle": [0, 2, 1, 0]}

    srv = service.serve(service.App(_store(), solve=fake), "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    try:
        base = f"http://127.0.0.1:{srv.server_address[1]}"
        r = remote.solve_tsp("dp", [[0, 1, 2], [1, 0, 3], [2, 3, 0]], [1, 2], 0, 0, base=base)
    finally:
        srv.shutdown()
        srv.server_close()
    assert r == {"duration": 7, "vehicle": [0, 2, 1, 0]} and seen == [("tsp", "dp")]


def _fake_app(store):
    def factory(dev):
        def solve(problem, algorithm, params, knobs, locations, durations):
            return {"duration": len(params["customers"]), "vehicle": [algorithm]}
        return service.App(store, device=dev, solve=solve)
    return factory


def _raw_http(port, data, timeout=30):
    s = socket.create_connection(("127.0.0.1", port), timeout=timeout)
    s.sendall(data)
    out = b""
    try:
        while True:
            b = s.recv(65536)
            if not b:
                break
            out += b
    except socket.timeout:
        pass
    s.close()
    return out


def test_http_pool_serves_solve_tsp_dp():
    store = _store()
    counts = mp.get_context("fork").Array("l", 1)

    def launch_factory(dev):
        def launch(N, host):
            with counts.get_lock():
                counts[dev] += host.shape[0]
            return (np.tile(np.arange(1, N, dtype=np.int16), (host.shape[0], 1)),
                    np.zeros(host.shape[0], dtype=np.int64))
        return launch

    inline = _inline_body()
    with frontends.FrontEndPool(store, workers=1, devices=(0,), slots_per_worker=64, nmax=16,
                                chunk=8, launch_factory=launch_factory,
                                app_factory=_fake_app(store), listen=("127.0.0.1", 0)) as pool:
        got = _raw_http(pool.port, b"POST /solve/tsp/dp HTTP/1.1\r\nConnection: close\r\n"
                        b"Content-Length: %d\r\n\r\n" % len(inline) + inline)
    assert got.startswith(b"HTTP/1.1 200"), got[:300]
    want = _fake_app(store)(0).solve_inline("tsp", "dp", inline)
    assert want[0] == 200 and want[1]["message"] == {"duration": 5, "vehicle": ["dp"]}
    assert json.loads(got.split(b"\r\n\r\n", 1)[1]) == want[1]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_dp(ctx, D, n=None):
    from vrpms_amd.core import TSP
    D = np.asarray(D, dtype=np.int64)
    ctx.set_instance(TSP, D, start_times=(0,))
    return runners.held_karp(ctx, D.shape[0] - 1 if n is None else n)


# n = 1, 2; 5, 6 (layers that do not fill a wavefront's lane groups); 16, 17
# (rows of 16 and of 32 words); 9 and 13 (several chunks per layer)
REF_CASES = [("sym", 1, 10), ("asym", 1, 11), ("sym", 2, 12), ("ties", 2, 13), ("asym", 5, 14),
             ("ties", 5, 15), ("sym", 6, 16), ("ties", 6, 17), ("asym", 9, 18), ("ties", 13, 19),
             ("sym", 16, 20), ("ties", 16, 21), ("asym", 17, 22), ("ties", 17, 23),
             ("zero", 6, 0), ("zero", 17, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed", REF_CASES)
def test_gpu_equals_reference(ctx, kind, n, seed):
    D = matrix(kind, n + 1, seed)
    dur, tour = held_karp_ref(D)
    if kind == "zero":
        assert tour == list(range(1, n + 1))
    key, got = gpu_dp(ctx, D)
    assert (key, got) == (spec.tsp_key(dur), tour)
    assert spec.eval_tsp(D, got) == dur


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,n,seed", [("ties", 11, 10, 30), ("sym", 13, 12, 31),
                                           ("asym", 14, 9, 32)])
def test_gpu_equals_brute_force_key_and_tour(ctx, kind, N, n, seed):
    D = matrix(kind, N, seed)
    key, tour = gpu_dp(ctx, D, n)
    bkey, btour = runners.brute_force(ctx, n)
    assert (key, tour) == (bkey, btour)
    assert key == spec.tsp_key(spec.eval_tsp(D, tour))
    assert sorted(tour) == list(range(1, n + 1))


@pytest.mark.gpu
def test_gpu_int32_matrix_path(ctx):
    D = matrix("asym", 9, 40)
    D[2, 5] = D[7, 1] = 70000          # above 65535: the instance keeps no uint16 matrix
    D[0, 3] = 100000
    dur, tour = held_karp_ref(D)
    assert gpu_dp(ctx, D) == (spec.tsp_key(dur), tour)


@pytest.mark.gpu
def test_gpu_planted_optimum_at_the_cap(ctx):
    """n = 24: the only size whose table offsets pass 2^31 bytes."""
    D, hidden = planted()
    key, tour = gpu_dp(ctx, D)
    assert tour == hidden
    assert key == spec.tsp_key(75)


@pytest.mark.gpu
def test_solve_tsp_dp_schema_and_optimum():
    D = synth.random_symmetric(9, np.random.default_rng(3))
    customers = [1, 3, 4, 6, 7, 8]
    res = solver.solve_tsp("dp", D.tolist(), customers, 5, 30, seed=1, time_limit=0.001)
    assert set(res) == {"duration", "vehicle"}
    v = res["vehicle"]
    assert v[0] == v[-1] == 5 and sorted(v[1:-1]) == customers
    assert res["duration"] == spec.eval_tsp(D[np.ix_(v[:-1], v[:-1])], list(range(1, len(v) - 1)), 30)
    best = min(sum(D[a, b] for a, b in zip((5,) + p, p + (5,)))
               for p in itertools.permutations(customers))
    assert res["duration"] == best
    # a device list: dp runs on the first, like bf not as an island model
    assert solver.solve_tsp("dp", D.tolist(), customers, 5, 30, devices=[0, 0]) == res
    # one and no customer: the front-end's trivial tours
    assert solver.solve_tsp("dp", D.tolist(), [2], 5)["vehicle"] == [5, 2, 5]
    assert solver.solve_tsp("dp", D.tolist(), [], 5)["vehicle"] == [5, 5]


@pytest.mark.gpu
def test_dp_bounds_the_heuristics_on_tsp20():
    inst = synth.tsp20(seed=0)
    D = inst.durations[0]
    cust = list(range(1, 20))
    dp = solver.solve_tsp("dp", D.tolist(), cust, 0)
    assert dp["duration"] == spec.eval_tsp(D, dp["vehicle"][1:-1])
    assert sorted(dp["vehicle"][1:-1]) == cust
    knobs = {"sa": {"chains": 128, "steps": 600}, "ga": {"pop": 64, "iteration_count": 60},
             "aco": {"ants": 32, "iteration_count": 20}}
    for algo, kn in knobs.items():
        h = solver.solve_tsp(algo, D.tolist(), cust, 0, seed=1, **kn)
        assert dp["duration"] <= h["duration"], algo


@pytest.mark.gpu
def test_run_errors_launch_nothing(ctx):
    import torch
    from vrpms_amd.core import CVRP, TSP
    lib = ctx.lib
    n = 6
    need = ctypes.c_uint64()
    assert lib.vrpms_tsp_dp_workspace(n, ctypes.byref(need)) == 0
    work = torch.zeros(need.value, dtype=torch.uint8, device=ctx.dev)
    tour = torch.full((n,), -7, dtype=torch.int16, device=ctx.dev)
    key = torch.full((1,), -7, dtype=torch.int64, device=ctx.dev)

    def run(nn=n, nbytes=None):
        return lib.vrpms_tsp_dp_run(ctx.handle, nn, work.data_ptr(),
                                    need.value if nbytes is None else nbytes, tour.data_ptr(),
                                    key.data_ptr(), ctx.stream())

    inst = synth.cvrp(n, 2, seed=1, slack=1.3)
    ctx.set_instance(CVRP, inst.durations, inst.demand, inst.capacities, inst.start_times)
    assert run() == _lib.VRPMS_EINVAL and b"TSP only" in lib.vrpms_last_error()
    ctx.set_instance(TSP, np.stack([matrix("sym", n + 1, 2)] * 24), start_times=(0,))
    assert run() == _lib.VRPMS_EINVAL and b"static" in lib.vrpms_last_error()
    ctx.set_instance(TSP, matrix("sym", n + 1, 2), start_times=(0,))
    assert run(nbytes=need.value - 1) == _lib.VRPMS_EINVAL
    assert b"too small" in lib.vrpms_last_error()
    assert run(nn=n + 1) == _lib.VRPMS_EINVAL and b"min(24, N-1)" in lib.vrpms_last_error()
    assert run(nn=0) == _lib.VRPMS_EINVAL
    assert lib.vrpms_tsp_dp_run(ctx.handle, n, None, need.value, tour.data_ptr(), key.data_ptr(),
                                ctx.stream()) == _lib.VRPMS_EINVAL
    from vrpms_amd.core import Context
    with Context(ctx.device) as fresh:      # no instance loaded
        assert lib.vrpms_tsp_dp_run(fresh.handle, n, work.data_ptr(), need.value, tour.data_ptr(),
                                    key.data_ptr(), ctx.stream()) == _lib.VRPMS_ESTATE
        assert b"no instance" in lib.vrpms_last_error()
    torch.cuda.synchronize(ctx.dev)
    assert tour.cpu().tolist() == [-7] * n and key.cpu().item() == -7
    assert int(work.max().item()) == 0
    # and the same buffers serve a valid call
    assert run() == _lib.VRPMS_OK
    dur, want = held_karp_ref(matrix("sym", n + 1, 2))
    assert tour.cpu().tolist() == want and key.cpu().item() == spec.tsp_key(dur)
