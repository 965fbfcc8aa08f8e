"""Exact time-dependent TSP by time-expanded subset DP (algorithm "tdp", spec
A16): the C entry points vrpms_tsp_tdp_workspace / vrpms_tsp_tdp_run,
Context.tsp_tdp, runners.time_expanded, solver.solve_tsp("tdp") and the inline
route POST /solve/tsp/tdp.

The reference is a restatement of A16 in this file with Python integers as
bitsets (bit r of a row = clock base + r: the rows' 60-bit hour words laid end
to end), itself checked against itertools.permutations + the spec's evaluator
on duration and on the tie-ruled tour; the GPU must return the identical key
and tour, the same key as the brute-force kernel wherever both run, and the
planted unique optimum beyond brute force's reach."""
import ctypes
import functools
import itertools
import json
import multiprocessing as mp
import socket
import threading

import numpy as np
import pytest

from oracle import spec
from vrpms_amd import _lib, frontends, remote, runners, service, solver, synth

NONE = 2**64 - 1


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def _bits(x):
    while x:
        low = x & -x
        yield low.bit_length() - 1
        x ^= low


def tdp_ref(D, start, upper_bound, n=None):
    """A16 -> (duration, tour) or None when no tour fits `upper_bound`."""
    D = spec.as_3d(D)
    H = D.shape[0]
    n = D.shape[1] - 1 if n is None else n
    h0 = start // 60
    off = start - 60 * h0
    W = (off + upper_bound) // 60 + 1
    keep = (1 << (off + upper_bound + 1)) - 1          # clocks up to start + upper_bound
    hour_bits = [0] * H                                # the words that use slice h
    for w in range(W):
        hour_bits[(h0 + w) % H] |= ((1 << 60) - 1) << (60 * w)

    def slice_of(r):
        return (h0 + r // 60) % H

    def shift(x, i, j):
        # every word moves by its own slice's duration: (x << s) & (2^60 - 1)
        # into word w + q and x >> (60 - s) into w + q + 1 are, laid end to
        # end, the word's bits moved up by d = 60 q + s
        out = 0
        for h in range(H):
            part = x & hour_bits[h]
            if part:
                out |= part << int(D[h, i, j])
        return out & keep

    R = {}
    for j in range(1, n + 1):
        R[1 << (j - 1), j] = (1 << (off + int(D[h0 % H, 0, j]))) & keep
    for S in sorted(range(1, 1 << n), key=lambda s: bin(s).count("1")):
        members = [j for j in range(1, n + 1) if S >> (j - 1) & 1]
        if len(members) < 2:
            continue
        for j in members:
            Sp = S ^ (1 << (j - 1))
            acc = 0
            for i in members:
                if i != j:
                    acc |= shift(R[Sp, i], i, j)
            R[S, j] = acc
    full = (1 << n) - 1
    best = None
    for j in range(1, n + 1):
        for b in _bits(R[full, j]):
            val = b + int(D[slice_of(b), j, 0]) - off
            if val <= upper_bound and (best is None or (val, j, b) < best):
                best = (val, j, b)
    if best is None:
        return None
    dur, j, b = best
    S, tour = full, [j]
    while S != 1 << (j - 1):
        S ^= 1 << (j - 1)
        for i in range(1, n + 1):
            if not S >> (i - 1) & 1:
                continue
            hit = [bp for bp in _bits(R[S, i]) if bp + int(D[slice_of(bp), i, j]) == b]
            if hit:
                j, b = i, hit[0]
                break
        tour.append(j)
    assert b == off + int(D[h0 % H, 0, j])
    return dur, tour[::-1]


def enumeration_optimum(D, n, start):
    """(min duration, the optimal tour whose reversed sequence is
    lexicographically smallest)."""
    perms = np.array(list(itertools.permutations(range(1, n + 1))), dtype=np.int64)
    durs = spec.eval_tsp_batch(D, perms, start)
    best = int(durs.min())
    tour = min((p.tolist() for p in perms[durs == best]), key=lambda p: p[::-1])
    assert spec.eval_tsp(D, tour, start) == best
    return best, tour


def nn_bound(D, n, start):
    return runners.nearest_neighbour_duration(D, n, start)


def earliest_arrival(D, start, n):
    """Held-Karp with the earliest arrival per (subset, node) as the state:
    what A14 would compute on an hourly matrix.  Not exact without FIFO."""
    D = spec.as_3d(D)
    H = D.shape[0]
    ea = {(1 << (j - 1), j): start + int(D[(start // 60) % H, 0, j]) for j in range(1, n + 1)}
    for S in sorted(range(1, 1 << n), key=lambda s: bin(s).count("1")):
        members = [j for j in range(1, n + 1) if S >> (j - 1) & 1]
        if len(members) < 2:
            continue
        for j in members:
            Sp = S ^ (1 << (j - 1))
            ea[S, j] = min(t + int(D[(t // 60) % H, i, j])
                           for i in members if i != j for t in [ea[Sp, i]])
    full = (1 << n) - 1
    return min(t + int(D[(t // 60) % H, j, 0]) for j in range(1, n + 1)
               for t in [ea[full, j]]) - start


def matrix(kind, N, seed, H=24):
    rng = np.random.default_rng(seed)
    if kind == "rand":
        D = rng.integers(3, 321, size=(H, N, N), dtype=np.int64)
    elif kind == "ties":
        D = rng.integers(1, 3, size=(H, N, N), dtype=np.int64)
    elif kind == "zeros":                 # includes zero durations
        D = rng.integers(0, 130, size=(H, N, N), dtype=np.int64)
    elif kind == "allzero":
        D = np.zeros((H, N, N), dtype=np.int64)
    elif kind == "mult60":                # every shift count is 60
        D = 60 * rng.integers(0, 4, size=(H, N, N), dtype=np.int64)
    elif kind == "long":                  # every duration at least an hour
        D = rng.integers(60, 400, size=(H, N, N), dtype=np.int64)
    elif kind == "huge":                  # rows near the kernel's 512-word limit
        D = rng.integers(4900, 5101, size=(H, N, N), dtype=np.int64)
    elif kind == "tdcvrp":                # Euclidean, rush hours: a long horizon
        return synth.td_cvrp(N - 1, 1, seed).durations
    else:
        raise ValueError(kind)
    for h in range(H):
        np.fill_diagonal(D[h], 0)
    return D


def planted(n, seed):
    """Hourly entries uniform in 4..60, every edge of one hidden cycle through
    all n + 1 nodes set to 3 in all 24 slices: that cycle (duration 3 (n + 1))
    is the unique optimum, any other tour has an edge >= 4 and none below 3."""
    rng = np.random.default_rng(seed)
    N = n + 1
    D = rng.integers(4, 61, size=(24, N, N), dtype=np.int64)
    hidden = (rng.permutation(n) + 1).tolist()
    path = [0] + hidden + [0]
    for h in range(24):
        np.fill_diagonal(D[h], 0)
        for a, b in zip(path, path[1:]):
            D[h, a, b] = 3
    return D, hidden


@functools.lru_cache(maxsize=None)
def non_fifo_instances():
    """integers(3, 321, (24, 8, 8)) at start 2323, the first three seeds on
    which the earliest-arrival Held-Karp misses the optimum -> [(D, optimum,
    tour, earliest-arrival value)]."""
    out = []
    for seed in range(60):
        D = matrix("rand", 8, seed)
        ea = earliest_arrival(D, 2323, 7)
        dur, tour = tdp_ref(D, 2323, ea)          # the earliest-arrival tour is a valid bound
        assert dur <= ea
        if dur < ea:
            out.append((D, dur, tour, ea))
            if len(out) == 3:
                break
    return out


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
ENUM_CASES = [("rand", 2, 0, 0), ("rand", 5, 1, 1390), ("rand", 7, 2, 2323), ("ties", 3, 3, 59),
              ("ties", 6, 4, 1390), ("ties", 7, 5, 0), ("zeros", 4, 6, 1501), ("zeros", 7, 7, 47),
              ("tdcvrp", 5, 8, 480), ("tdcvrp", 7, 9, 1390), ("rand", 6, 10, 2999)]


@pytest.mark.parametrize("kind,n,seed,start", ENUM_CASES)
def test_reference_equals_enumeration(kind, n, seed, start):
    D = matrix(kind, n + 1, seed)
    want = enumeration_optimum(D, n, start)
    assert tdp_ref(D, start, nn_bound(D, n, start)) == want
    assert spec.eval_tsp(D, want[1], start) == want[0]


@pytest.mark.parametrize("kind,n,seed,start", [("rand", 6, 20, 1390), ("ties", 6, 21, 7),
                                               ("tdcvrp", 6, 22, 480)])
def test_reference_does_not_depend_on_the_bound(kind, n, seed, start):
    D = matrix(kind, n + 1, seed)
    want = tdp_ref(D, start, nn_bound(D, n, start))
    assert want == enumeration_optimum(D, n, start)
    assert tdp_ref(D, start, want[0]) == want
    assert tdp_ref(D, start, want[0] + 777) == want
    assert tdp_ref(D, start, want[0] - 1) is None


def test_earliest_arrival_is_strictly_worse_on_non_fifo_instances():
    found = non_fifo_instances()
    assert len(found) == 3
    for D, dur, tour, ea in found:
        assert dur < ea and spec.eval_tsp(D, tour, 2323) == dur
        assert enumeration_optimum(D, 7, 2323) == (dur, tour)


def test_nearest_neighbour_bound_is_a_tour_duration():
    D = matrix("rand", 8, 30)
    # by hand: follow the rule and price the tour with the spec
    t, cur, left, tour = 1390, 0, list(range(1, 8)), []
    while left:
        row = D[(t // 60) % 24, cur]
        nxt = min(left, key=lambda c: (row[c], c))
        t += int(row[nxt])
        left.remove(nxt)
        tour.append(nxt)
        cur = nxt
    assert nn_bound(D, 7, 1390) == spec.eval_tsp(D, tour, 1390)


@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


def test_workspace_size(lib):
    b = ctypes.c_uint64()
    for n, start, horizon in [(1, 0, 0), (5, 59, 0), (5, 59, 1), (9, 480, 4000), (20, 1390, 63),
                              (13, 2875, 30000), (20, 0, 60 * 512 - 1)]:
        assert lib.vrpms_tsp_tdp_workspace(n, start, horizon, ctypes.byref(b)) == _lib.VRPMS_OK
        W = (start % 60 + horizon) // 60 + 1
        assert b.value == (1 << n) * n * W * 8
        assert b.value == solver.tdp_workspace_bytes(n, start, horizon)
    for n, start, horizon in [(0, 0, 10), (21, 0, 10), (5, 0, -1), (5, -1, 10),
                              (5, 0, 60 * 512), (5, 59, 60 * 512 - 59), (5, 2**31 - 10, 100)]:
        assert lib.vrpms_tsp_tdp_workspace(n, start, horizon, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    assert lib.vrpms_tsp_tdp_workspace(0, 0, 10, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    assert b"1 <= n <= 20" in lib.vrpms_last_error()
    assert lib.vrpms_tsp_tdp_workspace(5, 0, 10, None) == _lib.VRPMS_EINVAL


def test_run_rejects_null_ctx_before_any_hip_call(lib):
    assert lib.vrpms_tsp_tdp_run(None, 5, 100, None, 0, None, None, None) == _lib.VRPMS_EINVAL
    assert b"ctx is NULL" in lib.vrpms_last_error()


def test_front_end_errors_need_no_gpu():
    D = matrix("ties", 22, 0)
    with pytest.raises(ValueError, match=f"at most {solver.TDP_MAX_CUSTOMERS} customers"):
        solver.solve_tsp("tdp", D.tolist(), list(range(1, 22)), 0)
    # a large constant matrix: the nearest-neighbour bound is 21 * 900 minutes,
    # 316 words a row, 2^20 * 20 * 316 * 8 bytes
    big = np.full((21, 21), 900, dtype=np.int64)
    np.fill_diagonal(big, 0)
    need = (1 << 20) * 20 * (21 * 900 // 60 + 1) * 8
    assert need > solver.TDP_MAX_WORKSPACE == 16 << 30
    with pytest.raises(ValueError, match=f"{need} bytes.*{16 << 30} bytes"):
        solver.solve_tsp("tdp", big.tolist(), list(range(1, 21)), 0)
    # the same request with a bound the table fits is not refused for its size
    assert solver.tdp_workspace_bytes(20, 0, 5000) <= solver.TDP_MAX_WORKSPACE
    with pytest.raises(ValueError, match="at most 512 hours"):
        solver.solve_tsp("tdp", big[:4, :4].tolist(), [1, 2, 3], 0, upper_bound=60 * 512)
    locs = [{"id": i} for i in range(6)]
    with pytest.raises(ValueError, match="tdp solves the TSP only.*per-vehicle start times"):
        solver.solve_vrp("tdp", matrix("ties", 6, 1).tolist(), locs, [9], [0])
    assert "tdp" in solver.ALGORITHMS and 1 <= solver.TDP_MAX_CUSTOMERS <= 20
    assert solver.DP_MAX_CUSTOMERS == 24 and solver.BF_MAX_CUSTOMERS_TD == 11


def _store():
    return service.MemoryStore({}, {}, {})


def _inline_body(N=6):
    return json.dumps({"durations": matrix("rand", N, 4).tolist(), "customers": list(range(1, N)),
                       "startNode": 0, "startTime": 1390}).encode()


def test_solve_inline_routes_tsp_tdp_and_refuses_vrp_tdp():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, params["customers"], params["start_time"]))
        return {"duration": 1, "vehicle": [0, 1, 0]}

    app = service.App(_store(), solve=fake)
    st, res = app.solve_inline("tsp", "tdp", _inline_body())
    assert st == 200 and res == {"success": True, "message": {"duration": 1, "vehicle": [0, 1, 0]}}
    assert seen == [("tsp", "tdp", [1, 2, 3, 4, 5], 1390)]
    vrp = json.dumps({"durations": [[0, 1], [1, 0]], "locations": [{"id": 0}, {"id": 1}],
                      "capacities": [1], "startTimes": [0], "ignoredCustomers": [],
                      "completedCustomers": []}).encode()
    st, res = app.solve_inline("vrp", "tdp", vrp)
    assert st == 400 and "no solver /solve/vrp/tdp" in res["errors"][0]["reason"]
    assert len(seen) == 1
    assert "tdp" in service.INLINE_ALGORITHMS["tsp"] and service.INLINE_ALGORITHMS["vrp"][-1] == "sp"
    assert sorted(service.TITLES) == ["aco", "bf", "ga", "sa"]


def test_remote_forwards_tdp_to_the_inline_route():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, knobs.get("inline")))
        return {"duration": 7, "vehicle": [0, 2, 1, 0]}

    srv = service.serve(service.App(_store(), solve=fake), "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    try:
        base = f"http://127.0.0.1:{srv.server_address[1]}"
        r = remote.solve_tsp("tdp", [[0, 1, 2], [1, 0, 3], [2, 3, 0]], [1, 2], 0, 0, base=base,
                             upper_bound=9)
    finally:
        srv.shutdown()
        srv.server_close()
    assert r == {"duration": 7, "vehicle": [0, 2, 1, 0]}
    assert seen == [("tsp", "tdp", {"upper_bound": 9})]


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


def test_http_pool_serves_solve_tsp_tdp():
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
        got = _raw_http(pool.port, b"POST /solve/tsp/tdp HTTP/1.1\r\nConnection: close\r\n"
                        b"Content-Length: %d\r\n\r\n" % len(inline) + inline)
    assert got.startswith(b"HTTP/1.1 200"), got[:300]
    want = _fake_app(store)(0).solve_inline("tsp", "tdp", inline)
    assert want[0] == 200 and want[1]["message"] == {"duration": 5, "vehicle": ["tdp"]}
    assert json.loads(got.split(b"\r\n\r\n", 1)[1]) == want[1]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def gpu_tdp(ctx, D, start, n=None, upper_bound=None):
    from vrpms_amd.core import TSP
    D = np.asarray(D, dtype=np.int64)
    n = D.shape[-1] - 1 if n is None else n
    ctx.set_instance(TSP, D, start_times=(start,))
    return runners.time_expanded(ctx, n, D, start, upper_bound)


# (kind, n, seed, start, H): n = 1 (no layer), 2 (one layer), 5 (layers that do
# not fill a wavefront), 9 (several chunks per layer); {1, 2} matrices keep
# everything in one word (W = 1) and exercise the tie rule; d = 0; shift count
# 60; q > 0; a row of more words than lanes; hour wrap (1390), h0 >= 24 (2875),
# starts off the hour boundary; a static matrix through the same path; rows so
# long that the layer kernel's workgroup has 8 wavefronts instead of 16
REF_CASES = [("rand", 1, 40, 0, 24), ("rand", 2, 41, 17, 24), ("rand", 5, 42, 1390, 24),
             ("rand", 9, 43, 2875, 24), ("ties", 1, 44, 0, 24), ("ties", 2, 45, 30, 24),
             ("ties", 5, 46, 0, 24), ("ties", 9, 47, 1390, 24), ("allzero", 5, 0, 59, 24),
             ("allzero", 9, 0, 0, 24), ("mult60", 5, 48, 0, 24), ("mult60", 9, 49, 1397, 24),
             ("long", 5, 50, 2875, 24), ("long", 9, 51, 480, 24), ("zeros", 9, 52, 1439, 24),
             ("tdcvrp", 9, 9, 480, 24), ("rand", 9, 54, 45, 1), ("ties", 5, 55, 2875, 1),
             ("long", 5, 56, 1390, 1), ("huge", 5, 57, 480, 24)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,start,H", REF_CASES)
def test_gpu_equals_reference(ctx, kind, n, seed, start, H):
    D = matrix(kind, n + 1, seed, H)
    bound = nn_bound(D, n, start)
    W = (start % 60 + bound) // 60 + 1
    if kind == "ties" and H == 24 and n <= 5:
        assert W == 1
    if kind == "tdcvrp":
        assert W > 64
    if kind == "huge":
        assert 481 < W <= 512
    dur, tour = tdp_ref(D, start, bound)
    key, got = gpu_tdp(ctx, D, start)
    print(kind, n, start, H, "W", W, "ref", dur, tour, "gpu", spec.unpack_key(key), got)
    assert (key, got) == (spec.tsp_key(dur), tour)
    assert spec.eval_tsp(D, got, start) == dur


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,start", [("rand", 8, 60, 1390), ("ties", 7, 61, 7),
                                               ("tdcvrp", 7, 62, 480)])
def test_gpu_does_not_depend_on_the_bound(ctx, kind, n, seed, start):
    D = matrix(kind, n + 1, seed)
    dur, tour = tdp_ref(D, start, nn_bound(D, n, start))
    want = (spec.tsp_key(dur), tour)
    assert gpu_tdp(ctx, D, start) == want                          # nearest-neighbour bound
    assert gpu_tdp(ctx, D, start, upper_bound=dur) == want
    assert gpu_tdp(ctx, D, start, upper_bound=dur + 777) == want
    with pytest.raises(ValueError, match="no tour within upper_bound"):
        gpu_tdp(ctx, D, start, upper_bound=dur - 1)
    assert ctx.tsp_tdp(n, dur - 1) == (NONE, [0] * n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,start", [("rand", 10, 70, 1390), ("zeros", 11, 71, 2875)])
def test_gpu_equals_brute_force_key(ctx, kind, n, seed, start):
    D = matrix(kind, n + 1, seed)
    key, tour = gpu_tdp(ctx, D, start)
    bkey, btour = runners.brute_force(ctx, n)
    print(kind, n, "tdp", spec.unpack_key(key), tour, "bf", spec.unpack_key(bkey), btour)
    assert key == bkey
    assert sorted(tour) == list(range(1, n + 1))
    assert key == spec.tsp_key(spec.eval_tsp(D, tour, start))
    assert spec.eval_tsp(D, btour, start) == spec.eval_tsp(D, tour, start)


@pytest.mark.gpu
def test_gpu_equals_held_karp_on_a_static_matrix(ctx):
    D = synth.random_symmetric(14, np.random.default_rng(80))
    key, tour = gpu_tdp(ctx, D, 0)
    hkey, _ = runners.held_karp(ctx, 13)
    assert key == hkey == spec.tsp_key(spec.eval_tsp(D, tour))
    assert sorted(tour) == list(range(1, 14))


@pytest.mark.gpu
def test_gpu_strictly_below_earliest_arrival(ctx):
    for D, dur, tour, ea in non_fifo_instances():
        assert gpu_tdp(ctx, D, 2323) == (spec.tsp_key(dur), tour)
        assert dur < ea


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,start", [(16, 90, 1390), (20, 91, 2875)])
def test_gpu_planted_optimum_beyond_brute_force(ctx, n, seed, start):
    """n = 20 is the kernel's limit: a table of 2^20 * 20 rows, under 1 GiB
    at the handful of words these durations need."""
    D, hidden = planted(n, seed)
    assert spec.eval_tsp(D, hidden, start) == 3 * (n + 1)
    assert solver.tdp_workspace_bytes(n, start, nn_bound(D, n, start)) < 1 << 30
    key, tour = gpu_tdp(ctx, D, start)
    assert tour == hidden
    assert key == spec.tsp_key(3 * (n + 1))


@pytest.mark.gpu
def test_solve_tsp_tdp_schema_and_optimum():
    D = matrix("rand", 9, 100)
    customers = [1, 3, 4, 6, 7, 8]
    res = solver.solve_tsp("tdp", D.tolist(), customers, 5, 1390, seed=1, time_limit=0.001)
    assert set(res) == {"duration", "vehicle"}
    v = res["vehicle"]
    assert v[0] == v[-1] == 5 and sorted(v[1:-1]) == customers
    nodes = [5] + customers
    sub = D[:, nodes][:, :, nodes]
    dur, tour = enumeration_optimum(sub, 6, 1390)
    assert res == {"duration": dur, "vehicle": [5] + [nodes[c] for c in tour] + [5]}
    # a device list: tdp runs on the first, like dp not as an island model
    assert solver.solve_tsp("tdp", D.tolist(), customers, 5, 1390, devices=[0, 0]) == res
    assert solver.solve_tsp("tdp", D.tolist(), customers, 5, 1390, upper_bound=dur) == res
    with pytest.raises(ValueError, match="no tour within upper_bound"):
        solver.solve_tsp("tdp", D.tolist(), customers, 5, 1390, upper_bound=dur - 1)
    # one and no customer: the front-end's trivial tours
    assert solver.solve_tsp("tdp", D.tolist(), [2], 5)["vehicle"] == [5, 2, 5]
    assert solver.solve_tsp("tdp", D.tolist(), [], 5)["vehicle"] == [5, 5]


@pytest.mark.gpu
def test_post_solve_tsp_tdp_end_to_end():
    D = matrix("rand", 8, 101)
    cust = list(range(1, 8))
    want = solver.solve_tsp("tdp", D.tolist(), cust, 0, 2323)
    assert want["duration"] == enumeration_optimum(D, 7, 2323)[0]
    srv = service.serve(service.App(_store()), "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    try:
        base = f"http://127.0.0.1:{srv.server_address[1]}"
        got = remote.solve_tsp("tdp", D.tolist(), cust, 0, 2323, base=base)
        with pytest.raises(ValueError, match=f"at most {solver.TDP_MAX_CUSTOMERS} customers"):
            remote.solve_tsp("tdp", matrix("ties", 22, 0).tolist(), list(range(1, 22)), 0, base=base)
    finally:
        srv.shutdown()
        srv.server_close()
    assert got == want


@pytest.mark.gpu
def test_run_errors_launch_nothing(ctx):
    import torch
    from vrpms_amd.core import CVRP, TSP, Context
    lib = ctx.lib
    n = 6
    D = matrix("rand", n + 1, 2)
    horizon = nn_bound(D, n, 1390)
    need = ctypes.c_uint64()
    assert lib.vrpms_tsp_tdp_workspace(n, 1390, horizon, ctypes.byref(need)) == 0
    work = torch.zeros(need.value + 8, dtype=torch.uint8, device=ctx.dev)
    tour = torch.full((n,), -7, dtype=torch.int16, device=ctx.dev)
    key = torch.full((1,), -7, dtype=torch.int64, device=ctx.dev)

    def run(nn=n, hz=horizon, nbytes=None, ptr=None):
        return lib.vrpms_tsp_tdp_run(ctx.handle, nn, hz, work.data_ptr() if ptr is None else ptr,
                                     need.value if nbytes is None else nbytes, tour.data_ptr(),
                                     key.data_ptr(), ctx.stream())

    inst = synth.cvrp(n, 2, seed=1, slack=1.3)
    ctx.set_instance(CVRP, inst.durations, inst.demand, inst.capacities, inst.start_times)
    assert run() == _lib.VRPMS_EINVAL and b"TSP only" in lib.vrpms_last_error()
    ctx.set_instance(TSP, D, start_times=(1390,))
    assert run(nbytes=need.value - 1) == _lib.VRPMS_EINVAL
    assert b"too small" in lib.vrpms_last_error()
    assert run(ptr=work.data_ptr() + 4) == _lib.VRPMS_EINVAL
    assert b"8-byte aligned" in lib.vrpms_last_error()
    assert run(nn=n + 1) == _lib.VRPMS_EINVAL and b"min(20, N-1)" in lib.vrpms_last_error()
    assert run(nn=0) == _lib.VRPMS_EINVAL
    assert run(hz=-1) == _lib.VRPMS_EINVAL and b"horizon" in lib.vrpms_last_error()
    assert run(ptr=0) == _lib.VRPMS_EINVAL
    with Context(ctx.device) as fresh:      # no instance loaded
        assert lib.vrpms_tsp_tdp_run(fresh.handle, n, horizon, work.data_ptr(), need.value,
                                     tour.data_ptr(), key.data_ptr(),
                                     ctx.stream()) == _lib.VRPMS_ESTATE
        assert b"no instance" in lib.vrpms_last_error()
    torch.cuda.synchronize(ctx.dev)
    assert tour.cpu().tolist() == [-7] * n and key.cpu().item() == -7
    assert int(work.max().item()) == 0
    # and the same buffers serve a valid call
    assert run() == _lib.VRPMS_OK
    dur, want = tdp_ref(D, 1390, horizon)
    assert tour.cpu().tolist() == want and key.cpu().item() == spec.tsp_key(dur)
