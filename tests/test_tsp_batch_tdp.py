"""Batched exact time-dependent TSP (spec A20): the C entry points
vrpms_tsp_batch_tdp_lds / vrpms_tsp_batch_tdp, Context.tsp_batch_tdp,
solver.solve_tsp_batch("tdp") and the service's exact time-dependent batcher
(App(batch_exact=True)).

The reference is test_tsp_tdp's restatement of A16 (tdp_ref): per request the
GPU must return the identical key and tour, whatever batch the request rides
in, whatever the launch's row width W (at least the request's own) and
whatever the team size; with a W below a request's need, the reference's
answer for the effective horizon min(horizon, 60 W - 1 - start % 60)."""
import ctypes
import functools
import json
import threading

import numpy as np
import pytest

from oracle import spec
from test_tsp_tdp import matrix, non_fifo_instances, planted, tdp_ref
from vrpms_amd import _lib, runners, service, solver, synth
from vrpms_amd.core import tdp_words, tsp_batch_tdp_lds

NONE = 2**64 - 1
LDS_BYTES = 160 * 1024
TEAMS = (16, 32, 64, 128, 256)
# kBatchTdpTeam: the n -> T table before the LDS has its say, and the bytes
# (a fifth of a CU's LDS) the auto team's workgroup is raised to fit
TEAM_TABLE = {1: 16, 2: 16, 3: 16, 4: 16, 5: 16, 6: 32, 7: 32, 8: 128, 9: 256, 10: 256, 11: 256}
TEAM_LDS_BYTES = 32 * 1024


# ---------------------------------------------------------------------------
# cases: (kind, n, seed, start, horizon rule, H); the rule is "nn" (the
# nearest-neighbour tour's duration), "ea" (non_fifo_instances' earliest-
# arrival value) or minutes
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_matrix(kind, n, seed, H=24):
    if kind == "planted":
        D = planted(n, seed)[0]
    elif kind == "nonfifo":
        D = non_fifo_instances()[seed][0]
    else:
        D = matrix(kind, n + 1, seed, H)
    D = np.asarray(D, dtype=np.int64)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def case_horizon(case):
    kind, n, seed, start, rule, H = case
    if rule == "nn":
        return runners.nearest_neighbour_duration(case_matrix(kind, n, seed, H), n, start)
    if rule == "ea":
        return non_fifo_instances()[seed][3]
    return int(rule)


@functools.lru_cache(maxsize=None)
def reference(kind, n, seed, start, horizon, H=24):
    """tdp_ref, computed once per (matrix, start, horizon) and shared -> (key,
    tour): all-ones and zeros when no tour fits."""
    res = tdp_ref(case_matrix(kind, n, seed, H), start, horizon)
    if res is None:
        return NONE, (0,) * n
    return spec.tsp_key(res[0]), tuple(res[1])


def expected(cases, W=None):
    """([key], [tour]) of the cases at a launch of row width W (default: wide
    enough for all): the reference at each case's effective horizon."""
    keys, tours = [], []
    for c in cases:
        hz = case_horizon(c)
        if W is not None:
            hz = min(hz, 60 * W - 1 - c[3] % 60)
        k, t = reference(c[0], c[1], c[2], c[3], hz, c[5])
        keys.append(k)
        tours.append(list(t))
    return keys, tours


def case_words(c):
    return tdp_words(c[3], case_horizon(c))


# neighbours differ in kind, start and horizon, so a launch mixes row widths
# below its W; five or more cases per n, cycled: no multiple of the 1..16
# requests of a workgroup
POOLS = {
    1: [("rand", 1, 40, 0, "nn", 24), ("rand", 1, 41, 17, "nn", 24), ("ties", 1, 44, 0, "nn", 24),
        ("zeros", 1, 3, 1390, "nn", 24), ("long", 1, 5, 2875, "nn", 24)],
    2: [("rand", 2, 40, 0, "nn", 24), ("rand", 2, 41, 17, "nn", 24), ("ties", 2, 45, 30, "nn", 24),
        ("long", 2, 6, 1439, "nn", 24), ("allzero", 2, 0, 59, "nn", 24)],
    4: [("rand", 4, 11, 0, "nn", 24), ("ties", 4, 12, 59, "nn", 24), ("zeros", 4, 6, 1501, "nn", 24),
        ("long", 4, 13, 2875, "nn", 24), ("mult60", 4, 14, 7, "nn", 24)],
    5: [("rand", 5, 42, 1390, "nn", 24), ("long", 5, 50, 2875, "nn", 24),
        ("ties", 5, 46, 0, "nn", 24), ("zeros", 5, 6, 1501, "nn", 24),
        ("allzero", 5, 0, 59, "nn", 24)],
    6: [("mult60", 6, 48, 0, "nn", 24), ("rand", 6, 10, 2999, "nn", 24),
        ("ties", 6, 4, 1390, "nn", 24), ("mult60", 6, 49, 1397, "nn", 24),
        ("zeros", 6, 8, 47, "nn", 24)],
    7: [("nonfifo", 7, 0, 2323, "ea", 24), ("allzero", 7, 0, 0, "nn", 24),
        ("nonfifo", 7, 1, 2323, "ea", 24), ("ties", 7, 5, 0, "nn", 24),
        ("nonfifo", 7, 2, 2323, "ea", 24), ("zeros", 7, 7, 47, "nn", 24)],
    8: [("rand", 8, 60, 2323, "nn", 24), ("ties", 8, 15, 7, "nn", 24),
        ("zeros", 8, 16, 1439, "nn", 24), ("planted", 8, 8, 2875, 40, 24),
        ("allzero", 8, 0, 31, "nn", 24)],
    9: [("zeros", 9, 52, 47, 400, 24), ("ties", 9, 47, 1390, "nn", 24),
        ("planted", 9, 9, 2875, 35, 24), ("allzero", 9, 0, 0, "nn", 24),
        ("zeros", 9, 53, 0, 300, 24)],
    10: [("planted", 10, 10, 2875, 33, 24), ("zeros", 10, 17, 0, 120, 24),
         ("ties", 10, 18, 0, "nn", 24), ("ties", 10, 19, 1390, "nn", 24),
         ("allzero", 10, 0, 30, 0, 24), ("zeros", 10, 17, 0, 179, 24)],
    11: [("ties", 11, 20, 0, "nn", 24), ("ties", 11, 21, 1390, "nn", 24),
         ("planted", 11, 11, 0, 36, 24), ("allzero", 11, 0, 30, 0, 24),
         ("planted", 11, 12, 1380, 40, 24)],
}
STATIC = [("rand", 6, 54, 45, "nn", 1), ("ties", 6, 55, 2875, "nn", 1), ("long", 6, 56, 1390, "nn", 1)]
# the launch row widths the issue names for its cases
NAMED_WORDS = {("zeros", 9, 52, 47, 400, 24): 8, ("planted", 10, 10, 2875, 33, 24): 2,
               ("zeros", 10, 17, 0, 120, 24): 3, ("planted", 11, 11, 0, 36, 24): 1,
               ("ties", 11, 20, 0, "nn", 24): 1, ("ties", 11, 21, 1390, "nn", 24): 1}


def batch_of(n, R, shift=0):
    pool = POOLS[n]
    return [pool[(x + shift) % len(pool)] for x in range(R)]


def lds_formula(n, H, W, T):
    """tsp_batch_tdp.hip batch_tdp_lds_bytes: the binomial table (172 32-bit
    words), then per team n 2^(n-1) rows of W 64-bit words and the staged
    slices -- min(W, 24), or one when H = 1 -- of (n + 1)^2 32-bit words,
    padded to 8 bytes."""
    slices = 1 if H == 1 else min(W, 24)
    mat = (slices * (n + 1) * (n + 1) + 1) // 2 * 2
    return 172 * 4 + (256 // T) * ((n << (n - 1)) * W * 8 + mat * 4)


def auto_team(n, H, W):
    T = TEAM_TABLE[n]
    while T < 256 and lds_formula(n, H, W, T) > TEAM_LDS_BYTES:
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


def test_every_case_is_inside_the_lds_domain(lib):
    for n, pool in POOLS.items():
        W = max(case_words(c) for c in pool)
        assert tsp_batch_tdp_lds(n, 24, W) <= LDS_BYTES, (n, W)
        assert len({c[0] for c in pool}) >= 2 and len({c[3] for c in pool}) >= 2
        if n >= 4:
            assert len({case_words(c) for c in pool}) >= 2 or n == 11, n
    for c, W in NAMED_WORDS.items():
        assert case_words(c) == W, c
    assert tsp_batch_tdp_lds(6, 1, max(case_words(c) for c in STATIC)) <= LDS_BYTES
    assert all(case_words(("ties", 11, s, st, "nn", 24)) == 1 for s, st in ((20, 0), (21, 1390)))


def test_argument_errors_need_no_gpu(lib):
    """Every argument check comes before the context is looked at, so a
    stand-in block of zeros serves as the non-NULL ctx here."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 16)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    f = lib.vrpms_tsp_batch_tdp
    err = lib.vrpms_last_error

    def call(ctx=c, m=p, s=p, h=p, R=1, N=5, H=24, W=3, team=0, t=p, k=p):
        return f(ctx, m, s, h, R, N, H, W, team, t, k, None)

    assert call(ctx=None) == _lib.VRPMS_EINVAL
    assert b"vrpms_tsp_batch_tdp" in err() and b"ctx is NULL" in err()
    assert call(R=-1) == _lib.VRPMS_EINVAL and b"vrpms_tsp_batch_tdp" in err()
    for N in (-1, 0, 1, 13, 14, 50):
        assert call(N=N) == _lib.VRPMS_EINVAL
        assert b"vrpms_tsp_batch_tdp" in err() and b"2 <= N <= 12" in err()
    for H in (-1, 0, 2, 23, 25):
        assert call(H=H) == _lib.VRPMS_EINVAL and b"24 hour slices" in err()
    for W in (-1, 0, 513, 2**31 - 1):
        assert call(W=W) == _lib.VRPMS_EINVAL and b"1 <= W <= 512" in err()
    for team in (-1, 1, 8, 48, 255, 512):
        assert call(team=team) == _lib.VRPMS_EINVAL and b"team must be" in err()
    for name in ("m", "s", "h", "t", "k"):
        assert call(**{name: None}) == _lib.VRPMS_EINVAL
        assert b"vrpms_tsp_batch_tdp" in err() and b"NULL" in err()
    # the refusals hold with R = 0 too; a valid R = 0 call launches nothing
    assert call(R=0, N=13) == _lib.VRPMS_EINVAL and call(R=0, W=0) == _lib.VRPMS_EINVAL
    assert call(R=0, m=None, s=None, h=None, t=None, k=None) == _lib.VRPMS_OK
    assert call(R=0, N=12, H=1, W=512, team=256) == _lib.VRPMS_OK
    assert fake.raw == bytes(1 << 16) and buf.raw == bytes(1 << 16)

    g = lib.vrpms_tsp_batch_tdp_lds
    b = ctypes.c_uint64(77)
    assert g(5, 24, 3, 0, None) == _lib.VRPMS_EINVAL and b"bytes is NULL" in err()
    for n in (-1, 0, 12, 13):
        assert g(n, 24, 1, 0, ctypes.byref(b)) == _lib.VRPMS_EINVAL
        assert b"vrpms_tsp_batch_tdp_lds" in err() and b"1 <= n <= 11" in err()
    assert g(5, 2, 1, 0, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    assert g(5, 24, 0, 0, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    assert g(5, 24, 513, 0, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    assert g(5, 24, 1, 8, ctypes.byref(b)) == _lib.VRPMS_EINVAL
    assert b.value == 77


def test_lds_formula_and_the_domain_boundary(lib):
    for n in range(1, 12):
        for H in (1, 24):
            for W in (1, 2, 3, 8, 19, 23, 24, 25, 100, 512):
                for T in TEAMS:
                    assert tsp_batch_tdp_lds(n, H, W, T) == lds_formula(n, H, W, T), (n, H, W, T)
                assert tsp_batch_tdp_lds(n, H, W) == lds_formula(n, H, W, auto_team(n, H, W))
    # cells that hold for any sane layout: the table alone decides them
    for n, W, fits in [(11, 1, True), (11, 2, False), (10, 3, True), (10, 4, False),
                       (9, 8, True), (9, 9, False)]:
        assert (tsp_batch_tdp_lds(n, 24, W) <= LDS_BYTES) == fits, (n, W)
    with pytest.raises(_lib.VrpmsError, match="1 <= n <= 11"):
        tsp_batch_tdp_lds(12, 24, 1)
    assert 12 * 2**11 * 8 == 196608 > LDS_BYTES
    # this layout's n = 8 boundary: 19 words (155,648 B of table, 6,160 B of
    # slices, 688 B of binomials) fit, 20 words' table alone is the whole LDS
    assert tsp_batch_tdp_lds(8, 24, 19) == 162496 <= LDS_BYTES
    assert tsp_batch_tdp_lds(8, 24, 20) > LDS_BYTES
    assert tsp_batch_tdp_lds(11, 24, 1) == 688 + 90112 + 24 * 6 * 4


def _no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(solver, "context", boom)
    monkeypatch.setattr(solver, "Context", boom)


def _single_message(*args, **knobs):
    with pytest.raises(ValueError) as e:
        solver.solve_tsp("tdp", *args, **knobs)
    return str(e.value)


def test_solve_tsp_batch_refusals_need_no_gpu(monkeypatch):
    _no_gpu(monkeypatch)
    D6 = matrix("rand", 6, 0)
    good = (D6.tolist(), [1, 2, 3, 4, 5], 0, 0)
    with pytest.raises(ValueError, match="'sa'"):
        solver.solve_tsp_batch("sa", [good])
    D22 = matrix("ties", 22, 0)
    many = (D22.tolist(), list(range(1, 22)), 0, 0)
    msg = _single_message(*many)
    assert msg.startswith("tdp (time-expanded DP) supports at most 20 customers")
    with pytest.raises(ValueError) as e:
        solver.solve_tsp_batch("tdp", [good, good, many])
    assert str(e.value) == "request 2: " + msg
    msg = _single_message(*good, upper_bound=-1)
    assert msg == "tdp: upper_bound must be non-negative (minutes)"
    with pytest.raises(ValueError) as e:
        solver.solve_tsp_batch("tdp", [good, good + (-1,)])
    assert str(e.value) == "request 1: " + msg
    with pytest.raises(ValueError) as e:
        solver.solve_tsp_batch("tdp", [{"durations": D6.tolist(), "customers": [1, 2, 3],
                                        "start_node": 0, "upper_bound": -5}, good])
    assert str(e.value) == "request 0: " + msg
    big = np.full((24, 6, 6), 2**29, dtype=np.int64)
    with pytest.raises(ValueError, match=r"^request 1: .*A9 guard"):
        solver.solve_tsp_batch("tdp", [good, (big.tolist(), [1, 2, 3, 4, 5], 0, 0, 100)])
    with pytest.raises(ValueError, match=r"^request 0: tdp \(time-expanded DP\) supports an upper "
                                         r"bound of at most 512 hours"):
        solver.solve_tsp_batch("tdp", [good + (60 * 512,)])
    assert solver.solve_tsp_batch("tdp", []) == []
    assert solver.BATCH_TDP_MAX_CUSTOMERS == 11 and solver.BATCH_TDP_LDS_BYTES == LDS_BYTES
    assert solver.BATCH_DP_MAX_CUSTOMERS == 12 and solver.TDP_MAX_CUSTOMERS == 20


def _ci(n, kind="rand", seed=0, start_time=0, H=24):
    return solver.compact_tsp(matrix(kind, n + 1, seed, H), list(range(1, n + 1)), 0, start_time)


def test_batch_tdp_fits_and_batcher_accepts_at_the_domain_edges(lib):
    acc = service.ExactTdpBatcher.accepts
    for fits in (solver.batch_tdp_fits, acc):
        assert fits(_ci(1), 10) and fits(_ci(11, "ties"), 59) and fits(_ci(11, "ties", H=1), 59)
        assert not fits(_ci(11, "ties"), 60)                 # two words at n = 11
        assert not fits(_ci(11, "ties", start_time=1), 59)   # the start's minute counts
        assert not fits(_ci(12, "ties"), 10)                 # 12 customers never fit
        assert fits(_ci(10), 179) and not fits(_ci(10), 180)
        assert fits(_ci(9), 479) and not fits(_ci(9), 480)
        assert fits(_ci(8), 19 * 60 - 1) and not fits(_ci(8), 19 * 60)
        assert fits(_ci(3), 512 * 60 - 1)                    # 512 words, two requests a workgroup
        assert not fits(_ci(3), 512 * 60)                    # the kernel's row limit
        assert not fits(_ci(0), None) and not fits(_ci(5), None)
    big = solver.compact_tsp(np.full((24, 6, 6), 2**29, dtype=np.int64), [1, 2, 3, 4, 5], 0, 0)
    assert solver.batch_tdp_fits(big, 100) and not acc(big, 100)       # the A9 guard
    assert acc(_ci(6), 100) and not acc(_ci(6, start_time=2**31 - 100), 50)
    # the bound a request rides with: the knob, else nearest neighbour; one
    # customer's is its only tour's duration whatever the knob says
    ci = _ci(5, seed=3, start_time=17)
    assert solver.batch_tdp_bound(ci, 777) == 777
    assert solver.batch_tdp_bound(ci) == runners.nearest_neighbour_duration(ci.durations, 5, 17)
    one = _ci(1, seed=3, start_time=17)
    want = int(one.durations[0, 0, 1]) + int(one.durations[(17 + int(one.durations[0, 0, 1])) // 60 % 24, 1, 0])
    assert solver.batch_tdp_bound(one, 5) == solver.batch_tdp_bound(one) == want
    assert solver.batch_tdp_bound(_ci(0)) is None


def test_a_clamped_key_is_priced_on_the_host_by_one_fallback():
    """A key at the 2^28 - 1 clamp has its duration priced by the one host
    fallback dp and tdp share: the static edge sum for H = 1, the A3 clock for
    H = 24; a key below the clamp is read as it is, an all-ones key is None."""
    tour = [3, 1, 5, 2, 4]
    path = [0] + tour + [0]
    clamped = spec.tsp_key(2**28 - 1)
    static, hourly = _ci(5, seed=4, start_time=1390, H=1), _ci(5, seed=4, start_time=1390)
    edge_sum = sum(int(static.durations[0][a][b]) for a, b in zip(path, path[1:]))
    clock = spec.eval_tsp(hourly.durations, tour, 1390)
    assert clock != sum(int(hourly.durations[0][a][b]) for a, b in zip(path, path[1:]))
    assert solver._td_duration(static, tour) == edge_sum
    assert solver._td_duration(hourly, tour) == clock
    assert solver._key_durations([static, hourly, static, hourly], [tour] * 4,
                                 [clamped, clamped, spec.tsp_key(77), -1]) == \
        [edge_sum, clock, 77, None]


class _FakeApp:
    devices = [0]
    device = 0
    locks = {0: threading.Lock()}


def _together(fn, count):
    out = [None] * count

    def go(x):
        try:
            out[x] = fn(x)
        except Exception as e:
            out[x] = e

    ths = [threading.Thread(target=go, args=(x,)) for x in range(count)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    return out


def test_exact_tdp_batcher_groups_by_node_and_hour_count_one_launch_each():
    seen = []

    def launch(key, cis, bounds):
        seen.append((key, len(cis), sorted(bounds)))
        N = key[0]
        return [list(range(N - 1, 0, -1)) for _ in cis]      # tours only: durations on the host

    b = service.ExactTdpBatcher(_FakeApp(), window_s=0.2, launch=launch)
    cis = [_ci(4, seed=x, start_time=1390 + x) for x in range(5)] + \
          [_ci(7, seed=x) for x in range(3)] + [_ci(4, seed=x, H=1) for x in range(2)]
    out = _together(lambda x: b.solve(cis[x], 100 + x), len(cis))
    assert sorted(seen) == [((5, 1), 2, [108, 109]), ((5, 24), 5, [100, 101, 102, 103, 104]),
                            ((8, 24), 3, [105, 106, 107])]
    assert b.launches == 3 and b.requests == 10
    for ci, res in zip(cis, out):
        tour = list(range(ci.N - 1, 0, -1))
        assert res["vehicle"] == [0] + tour + [0]
        D = ci.durations if ci.durations.shape[0] == 24 else np.stack([ci.durations[0]] * 24)
        assert res["duration"] == spec.eval_tsp(D, tour, int(ci.start_times[0]))


def test_exact_tdp_batcher_launch_error_reaches_every_waiter_of_its_group():
    def launch(key, cis, bounds):
        if key == (5, 24):
            raise RuntimeError("launch failed")
        # (tours, durations): None marks a request no tour fits
        return [list(range(1, key[0])) for _ in cis], [None if b == 0 else 7 for b in bounds]

    b = service.ExactTdpBatcher(_FakeApp(), window_s=0.2, launch=launch)
    cis = [_ci(4, seed=x) for x in range(4)] + [_ci(6), _ci(6, seed=1)]
    out = _together(lambda x: b.solve(cis[x], 50), len(cis))
    assert all(isinstance(o, RuntimeError) and "launch failed" in str(o) for o in out[:4])
    assert out[4] == out[5] == {"duration": 7, "vehicle": [0, 1, 2, 3, 4, 5, 6, 0]}

    def none_fits(key, cis, bounds):
        return [[0] * (key[0] - 1) for _ in cis], [None] * len(cis)

    b = service.ExactTdpBatcher(_FakeApp(), window_s=0.01, launch=none_fits)
    with pytest.raises(ValueError, match="no tour within upper_bound = 3 minutes"):
        b.solve(_ci(4), 3)


def _store():
    return service.MemoryStore({"L7": [{"id": i} for i in range(7)]},
                               {"D7": matrix("rand", 7, 50, 1)[0].tolist()}, {})


def _tdp_body(n, seed=60, start=1390, kind="rand", knobs=None, customers=None, H=24):
    D = matrix(kind, n + 1, seed, H)
    body = {"durations": (D[0] if H == 1 else D).tolist(),
            "customers": list(range(1, n + 1)) if customers is None else customers,
            "startNode": 0, "startTime": start}
    if knobs:
        body["knobs"] = knobs
    return json.dumps(body).encode()


def test_app_has_no_tdp_batcher_by_default_and_routes_unchanged():
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, params["customers"], knobs.get("inline")))
        return {"duration": 1, "vehicle": [0, 1, 0]}

    app = service.App(_store(), solve=fake)
    assert app.exact_tdp_batcher is None and app.exact_batcher is None
    st, res = app.solve_inline("tsp", "tdp", _tdp_body(5, knobs={"upper_bound": 900}))
    assert st == 200 and res["message"] == {"duration": 1, "vehicle": [0, 1, 0]}
    assert seen == [("tsp", "tdp", [1, 2, 3, 4, 5], {"upper_bound": 900})]


def test_app_batch_exact_rides_only_inline_tdp_inside_the_domain():
    seen, launched = [], []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm))
        return {"duration": 1, "vehicle": [0, 1, 0]}

    def launch(key, cis, bounds):
        launched.append((key, len(cis), list(bounds)))
        return [list(range(1, key[0])) for _ in cis]

    def other(*a):
        raise AssertionError("another batcher's launch")

    app = service.App(_store(), solve=fake, batch_exact=True, batch_window_s=0.01,
                      batch_exact_launch=other, batch_exact_vrp_launch=other,
                      batch_exact_tdp_launch=launch)
    st, res = app.solve_inline("tsp", "tdp", _tdp_body(5))
    assert st == 200 and res["message"]["vehicle"] == [0, 1, 2, 3, 4, 5, 0]
    D = matrix("rand", 6, 60)
    assert res["message"]["duration"] == spec.eval_tsp(D, [1, 2, 3, 4, 5], 1390)
    nn = runners.nearest_neighbour_duration(D, 5, 1390)
    # the inline knob reaches the job; a static matrix rides too, in its own group
    st, res = app.solve_inline("tsp", "tdp", _tdp_body(5, knobs={"upper_bound": 4000}))
    assert st == 200
    st, res = app.solve_inline("tsp", "tdp", _tdp_body(5, H=1))
    assert st == 200
    assert [(k, c) for k, c, _ in launched] == [((6, 24), 1), ((6, 24), 1), ((6, 1), 1)]
    assert launched[0][2] == [nn] and launched[1][2] == [4000]
    assert seen == []
    # outside: 12 customers, no customer, a row too wide for the LDS at 9
    # customers, and every other algorithm or route
    assert app.solve_inline("tsp", "tdp", _tdp_body(12, kind="ties"))[0] == 200
    assert app.solve_inline("tsp", "tdp", _tdp_body(5, customers=[]))[0] == 200
    assert app.solve_inline("tsp", "tdp", _tdp_body(9, knobs={"upper_bound": 3000}))[0] == 200
    assert app.solve_inline("tsp", "sa", _tdp_body(5))[0] == 200
    assert app.solve_inline("tsp", "dp", _tdp_body(5))[0] == 200       # hour-indexed dp: unbatched
    body = json.dumps({"solutionName": "s", "solutionDescription": "d", "locationsKey": "L7",
                       "durationsKey": "D7", "customers": [1, 2, 3], "startNode": 0,
                       "startTime": 0}).encode()
    assert app.post("tsp", "sa", body)[0] == 200
    assert seen == [("tsp", "tdp")] * 3 + [("tsp", "sa"), ("tsp", "dp"), ("tsp", "sa")]
    assert len(launched) == 3
    # a bad request gets the unbatched path's message
    st, res = app.solve_inline("tsp", "tdp", _tdp_body(21, kind="ties"))
    assert st == 400 and "supports at most 20 customers" in res["errors"][0]["reason"]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def stack(cases):
    return np.stack([case_matrix(c[0], c[1], c[2], c[5]) for c in cases]).astype(np.int32)


def gpu_batch(ctx, cases, W=None, team=0):
    """([key], [tour]) of one Context.tsp_batch_tdp launch."""
    import torch
    M = torch.from_numpy(stack(cases)).to(ctx.dev)
    tours, keys = ctx.tsp_batch_tdp(M, [c[3] for c in cases], [case_horizon(c) for c in cases],
                                    W=W, team=team)
    return [int(k) & NONE for k in keys.cpu().tolist()], tours.cpu().tolist()


def raw_batch(ctx, cases, W, team=0, horizons=None):
    """One vrpms_tsp_batch_tdp call on buffers with a guard row -> (rc, [key],
    [tour]); the guard row must come back untouched."""
    import torch
    R, n = len(cases), cases[0][1]
    M = torch.from_numpy(stack(cases)).to(ctx.dev)
    st = torch.tensor([c[3] for c in cases], dtype=torch.int32, device=ctx.dev)
    hz = torch.tensor(horizons or [case_horizon(c) for c in cases], dtype=torch.int32,
                      device=ctx.dev)
    tours = torch.full((R + 1, n), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R + 1,), -7, dtype=torch.int64, device=ctx.dev)
    rc = ctx.lib.vrpms_tsp_batch_tdp(ctx.handle, M.data_ptr(), st.data_ptr(), hz.data_ptr(), R,
                                     n + 1, cases[0][5], W, team, tours.data_ptr(),
                                     keys.data_ptr(), ctx.stream())
    torch.cuda.synchronize(ctx.dev)
    assert tours[R].cpu().tolist() == [-7] * n and keys[R].cpu().item() == -7
    return rc, [int(k) & NONE for k in keys[:R].cpu().tolist()], tours[:R].cpu().tolist()


# every n at R = 1 and 5, and 67 up to n = 9: a ragged last workgroup at every
# team size (67 = 4 * 16 + 3 = 2 * 32 + 3 = ... = 66 + 1)
CASES = [(n, R) for n in POOLS for R in (1, 5)] + [(n, 67) for n in POOLS if n <= 9]


@pytest.mark.gpu
@pytest.mark.parametrize("n,R", CASES)
def test_gpu_equals_reference(ctx, n, R):
    cases = batch_of(n, R, shift=R)
    keys, tours = gpu_batch(ctx, cases)
    wkeys, wtours = expected(cases)
    print(n, R, "W", [case_words(c) for c in cases[:7]], "keys", [k >> 28 for k in keys[:7]])
    assert tours == wtours
    assert keys == wkeys
    for c, k, t in zip(cases, keys, tours):
        if c[0] == "nonfifo":     # strictly below the earliest-arrival value
            assert k != NONE and (k >> 28) < case_horizon(c)
        if c[0] == "planted":
            assert t == planted(c[1], c[2])[1] and k == spec.tsp_key(3 * (c[1] + 1))


@pytest.mark.gpu
def test_gpu_static_matrices_equal_reference_and_held_karp(ctx):
    from vrpms_amd.core import TSP
    keys, tours = gpu_batch(ctx, STATIC)
    assert (keys, tours) == expected(STATIC)
    for c, k in zip(STATIC, keys):
        ctx.set_instance(TSP, case_matrix(c[0], c[1], c[2], 1), start_times=(0,))
        hk, _ = runners.held_karp(ctx, c[1])
        assert k == hk != NONE


@pytest.mark.gpu
def test_gpu_horizon_below_the_optimum_fails_that_request_only(ctx):
    cases = batch_of(6, 7)
    wkeys, wtours = expected(cases)
    x = 1
    opt = wkeys[x] >> 28
    assert wkeys[x] != NONE and opt >= 1
    W = max(case_words(c) for c in cases)
    base = [case_horizon(c) for c in cases]
    rc, keys, tours = raw_batch(ctx, cases, W, horizons=base[:x] + [opt - 1] + base[x + 1:])
    assert rc == _lib.VRPMS_OK
    assert keys[x] == NONE and tours[x] == [0] * 6
    assert keys[:x] + keys[x + 1:] == wkeys[:x] + wkeys[x + 1:]
    assert tours[:x] + tours[x + 1:] == wtours[:x] + wtours[x + 1:]
    rc, keys, tours = raw_batch(ctx, cases, W, horizons=base[:x] + [opt] + base[x + 1:])
    assert rc == _lib.VRPMS_OK and (keys, tours) == (wkeys, wtours)


@pytest.mark.gpu
def test_gpu_answers_do_not_depend_on_the_row_width_and_a_small_one_is_safe(ctx):
    cases = batch_of(7, 9)
    words = [case_words(c) for c in cases]
    W = max(words)
    assert tsp_batch_tdp_lds(7, 24, W + 3) <= LDS_BYTES and len(set(words)) >= 3
    want = expected(cases)
    rc, keys, tours = raw_batch(ctx, cases, W)
    assert rc == _lib.VRPMS_OK and (keys, tours) == want
    rc, keys, tours = raw_batch(ctx, cases, W + 3)
    assert rc == _lib.VRPMS_OK and (keys, tours) == want
    assert gpu_batch(ctx, cases, W=W + 3) == want
    # one word short of the widest request: it gets the reference's answer for
    # its effective horizon, everyone narrower their own
    rc, keys, tours = raw_batch(ctx, cases, W - 1)
    clipped = expected(cases, W - 1)
    assert rc == _lib.VRPMS_OK and (keys, tours) == clipped
    for x, w in enumerate(words):
        if w < W:
            assert (keys[x], tours[x]) == (want[0][x], want[1][x])
    # and far short of most: W = 1
    rc, keys, tours = raw_batch(ctx, cases, 1)
    assert rc == _lib.VRPMS_OK and (keys, tours) == expected(cases, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 7, 9])
def test_gpu_isolation(ctx, n):
    cases = batch_of(n, 11, shift=3)
    keys, tours = gpu_batch(ctx, cases)
    assert (keys, tours) == expected(cases)
    for x, c in enumerate(cases[:len(POOLS[n])]):
        k1, t1 = gpu_batch(ctx, [c])
        assert (k1[0], t1[0]) == (keys[x], tours[x])


@pytest.mark.gpu
@pytest.mark.parametrize("n,R", [(2, 5), (8, 7), (11, 3)])
def test_gpu_guard_row_and_erroring_calls(ctx, n, R):
    import torch
    lib, N = ctx.lib, n + 1
    cases = batch_of(n, R, shift=1)
    W = max(case_words(c) for c in cases)
    M = torch.from_numpy(stack(cases)).to(ctx.dev)
    st = torch.tensor([c[3] for c in cases], dtype=torch.int32, device=ctx.dev)
    hz = torch.tensor([case_horizon(c) for c in cases], dtype=torch.int32, device=ctx.dev)
    tours = torch.full((R + 1, n), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R + 1,), -7, dtype=torch.int64, device=ctx.dev)

    def run(c=ctx.handle, m=M.data_ptr(), s=st.data_ptr(), h=hz.data_ptr(), r=R, nn=N, H=24, w=W,
            team=0, t=tours.data_ptr(), k=keys.data_ptr()):
        return lib.vrpms_tsp_batch_tdp(c, m, s, h, r, nn, H, w, team, t, k, ctx.stream())

    assert run(c=None) == _lib.VRPMS_EINVAL
    assert run(r=-1) == _lib.VRPMS_EINVAL
    assert run(nn=1) == _lib.VRPMS_EINVAL and run(nn=13) == _lib.VRPMS_EINVAL
    assert b"2 <= N <= 12" in lib.vrpms_last_error()
    assert run(H=12) == _lib.VRPMS_EINVAL and run(w=0) == _lib.VRPMS_EINVAL
    assert run(w=513) == _lib.VRPMS_EINVAL and run(team=48) == _lib.VRPMS_EINVAL
    for name in ("m", "s", "h", "t", "k"):
        assert run(**{name: None}) == _lib.VRPMS_EINVAL
    over = 512 if n >= 8 else None       # a row width whose table is beyond the LDS
    if over:
        assert run(w=over) == _lib.VRPMS_EINVAL
        msg = lib.vrpms_last_error()
        assert b"bytes of LDS" in msg and str(lds_formula(n, 24, over, 256)).encode() in msg
    assert run(r=0) == _lib.VRPMS_OK
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item()
    assert run() == _lib.VRPMS_OK
    torch.cuda.synchronize(ctx.dev)
    wkeys, wtours = expected(cases)
    assert tours[:R].cpu().tolist() == wtours
    assert [int(k) & NONE for k in keys[:R].cpu().tolist()] == wkeys
    assert tours[R].cpu().tolist() == [-7] * n and keys[R].cpu().item() == -7


@pytest.mark.gpu
def test_gpu_more_workgroups_than_the_chip_holds(ctx):
    """R = 600 at n = 11: one workgroup per request, one per CU at a time."""
    import torch
    made = [planted(11, 1000 + x) for x in range(600)]
    M = torch.from_numpy(np.stack([D for D, _ in made]).astype(np.int32)).to(ctx.dev)
    tours, keys = ctx.tsp_batch_tdp(M, [0] * 600, [36] * 600)
    assert tours.cpu().tolist() == [h for _, h in made]
    assert keys.cpu().tolist() == [spec.tsp_key(36)] * 600


TEAM_NS = (1, 2, 5, 8, 9, 10, 11)


@pytest.mark.gpu
@pytest.mark.parametrize("n", TEAM_NS)
@pytest.mark.parametrize("T", TEAMS)
def test_gpu_forced_team_equals_reference_and_auto_or_is_refused(ctx, T, n):
    """Each team either answers as the auto team and the reference do, or is
    refused with the byte count in the message and nothing written; which of
    the two is what the LDS formula says."""
    R = 5
    wide = batch_of(n, R, shift=2)
    # the launch picks its fill by W (owner rows below 8 words, atomic OR from
    # there): the pool's wide launch, and one of its narrow cases alone
    narrow = [c for c in POOLS[n] if case_words(c) < 8]
    narrow = [narrow[x % len(narrow)] for x in range(R)]
    for cases in (wide, narrow) if narrow != wide else (wide,):
        W = max(case_words(c) for c in cases)
        want = expected(cases)
        rc, keys, tours = raw_batch(ctx, cases, W)
        assert rc == _lib.VRPMS_OK and (keys, tours) == want
        need = lds_formula(n, 24, W, T)
        rc, keys, tours = raw_batch(ctx, cases, W, team=T)
        if need > LDS_BYTES:
            assert rc == _lib.VRPMS_EINVAL
            msg = ctx.lib.vrpms_last_error()
            assert b"vrpms_tsp_batch_tdp" in msg and b"bytes of LDS" in msg
            assert str(need).encode() in msg
            assert keys == [(-7) & NONE] * R and tours == [[-7] * n] * R
        else:
            assert rc == _lib.VRPMS_OK and (keys, tours) == want


def test_forced_team_refused_set_at_the_pools_row_widths(lib):
    """What the GPU test above must see refused."""
    refused = set()
    for n in TEAM_NS:
        W = max(case_words(c) for c in batch_of(n, 5, shift=2))
        refused |= {(n, T) for T in TEAMS if lds_formula(n, 24, W, T) > LDS_BYTES}
    assert {(11, T) for T in (16, 32, 64, 128)} <= refused
    assert {(10, T) for T in (16, 32, 64, 128)} <= refused
    assert not {(n, T) for n in (1, 2) for T in TEAMS} & refused
    assert not {(n, 256) for n in TEAM_NS} & refused


@pytest.mark.gpu
def test_gpu_agrees_with_the_single_request_kernels(ctx):
    from vrpms_amd.core import TSP
    for c in [POOLS[8][0], POOLS[8][2], POOLS[10][0], POOLS[10][1]]:
        D, n, start, hz = case_matrix(c[0], c[1], c[2]), c[1], c[3], case_horizon(c)
        ctx.set_instance(TSP, D, start_times=(start,))
        key, tour = ctx.tsp_tdp(n, hz)
        assert gpu_batch(ctx, [c]) == ([key], [tour])
        assert ([key], [tour]) == tuple(expected([c]))


def _as_args(r):
    if isinstance(r, dict):
        knobs = {"upper_bound": r["upper_bound"]} if "upper_bound" in r else {}
        return (r["durations"], r["customers"], r["start_node"], r.get("start_time", 0)), knobs
    return tuple(r[:4]), ({"upper_bound": r[4]} if len(r) > 4 else {})


@pytest.mark.gpu
def test_solve_tsp_batch_equals_the_list_comprehension(lib):
    D9, D13 = matrix("rand", 9, 80), matrix("ties", 13, 81)
    td = synth.td_cvrp(9, 1, 3).durations
    ci = solver.compact_tsp(td, list(range(1, 10)), 0, 480)
    assert not solver.batch_tdp_fits(ci, solver.batch_tdp_bound(ci))     # its default W: single path
    static = matrix("rand", 7, 85, 1)[0]
    opt = tdp_ref(matrix("zeros", 7, 86), 47, 2000)[0]
    reqs = [(matrix("rand", 6, 82).tolist(), [1, 2, 3, 4, 5], 0, 1390),
            (D9.tolist(), [1, 3, 4, 6, 7, 8], 5, 30),              # a subset, start node 5
            (D9.tolist(), [], 2, 0),                               # no customer
            (D9.tolist(), [4], 2, 11),                             # one customer
            (D9.tolist(), [4], 2, 11, 0),                          # ... whose bound is ignored
            (D13.tolist(), list(range(1, 13)), 0, 0),              # 12 customers: single path
            (td.tolist(), list(range(1, 10)), 0, 480),             # W outside the LDS: single path
            (static.tolist(), [6, 5, 4, 3, 2, 1], 0, 3),           # a static matrix
            {"durations": matrix("zeros", 7, 86).tolist(), "customers": list(range(1, 7)),
             "start_node": 0, "start_time": 47, "upper_bound": opt},     # an explicit bound
            {"durations": matrix("ties", 6, 83).tolist(), "customers": [5, 4, 3, 2, 1],
             "start_node": 0},
            (matrix("rand", 6, 82).tolist(), [1, 2, 3, 4, 5], 0, 2875, 5000)]
    want = []
    for r in reqs:
        args, knobs = _as_args(r)
        want.append(solver.solve_tsp("tdp", *args, **knobs))
    assert solver.solve_tsp_batch("tdp", reqs) == want
    assert want[8]["duration"] == opt
    with pytest.raises(ValueError, match=r"^request 1: no tour within upper_bound = %d" % (opt - 1)):
        solver.solve_tsp_batch("tdp", [reqs[0], dict(reqs[8], upper_bound=opt - 1)])
    with pytest.raises(ValueError, match=r"^no tour within upper_bound = %d" % (opt - 1)):
        solver.solve_tsp("tdp", *_as_args(reqs[8])[0], upper_bound=opt - 1)


@pytest.mark.gpu
def test_service_batch_exact_equals_the_unbatched_answers():
    on = service.App(_store(), batch_exact=True, batch_window_s=0.05)
    off = service.App(_store())
    calls = []
    for x in range(24):
        n = (5, 8)[x % 2]
        knobs = {"upper_bound": 3000 if n == 5 else 1100} if x % 3 == 0 else None
        calls.append(_tdp_body(n, seed=60 + x, start=(1390, 17, 2875)[x % 3], knobs=knobs,
                               H=1 if x % 8 == 7 else 24))
    out = _together(lambda x: on.solve_inline("tsp", "tdp", calls[x]), len(calls))
    assert on.exact_tdp_batcher.requests == 24
    assert 1 <= on.exact_tdp_batcher.launches < on.exact_tdp_batcher.requests
    assert on.exact_batcher.requests == 0
    for body, got in zip(calls, out):
        want = off.solve_inline("tsp", "tdp", body)
        assert want[0] == 200 and got == want
