"""The six batchers of the batched VRP heuristics in vrpms_amd.service (sa, ga,
aco, ls, lsr, lsf) as the service's callers see them: what the real launch
hands to solver.batch_<alg>_launch, the device argument, the group keys, both
call forms of `accepts`, the complete text of every constructor refusal, the
routing of App.solve_inline and App.post, the keywords main() hands to App, and
App's refusal of a keyword it does not know.

The per-algorithm test files check each batcher against its own kernel; this
file states what the six have in common and what those files leave open.  It
needs the library and no GPU.  Every expected text is a literal: what the
service gave when this file was written."""
import functools
import json
import threading

import numpy as np
import pytest

from test_vrp_batch_ga import _FakeApp, _body, _concurrently, _fake_launch, _locs, _no_gpu, _sized
from test_vrp_batch_ga import request
from test_vrp_batch_lsr import _fake_launch as _fake_separator_launch
from vrpms_amd import _lib, core, service, solver

ALGORITHMS = ("sa", "ga", "aco", "ls", "lsr", "lsf")
CLASSES = {"sa": "VrpSaBatcher", "ga": "VrpGaBatcher", "aco": "VrpAcoBatcher",
           "ls": "VrpLsBatcher", "lsr": "VrpLsrBatcher", "lsf": "VrpLsfBatcher"}
ATTRIBUTES = {a: f"vrp_{a}_batcher" for a in ALGORITHMS}
LDS_BYTES = 160 * 1024
SEED = 4242
# a launch's rows as the stand-in launches give them: lsr and lsf carry separators
FAKES = {"sa": _fake_launch, "ga": _fake_launch, "aco": _fake_launch, "ls": _fake_launch,
         "lsr": _fake_separator_launch, "lsf": _fake_separator_launch}


@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


class _Devices(_FakeApp):
    """_FakeApp with devices, locks and a seed of its own."""

    def __init__(self, devices=(0,), seed=SEED):
        self.devices = list(devices)
        self.device = self.devices[0]
        self.locks = {d: threading.Lock() for d in self.devices}
        self.seed = seed


def _cls(algorithm):
    return getattr(service, CLASSES[algorithm])


def _batcher(algorithm, app, window_s=0.05, launch=None, **more):
    """The batcher of `algorithm` at knobs no default has: 777 steps, 5 ants
    and 9 iterations, 16 starts and 7 rounds."""
    knobs = {"sa": dict(steps=777), "ga": {}, "aco": dict(ants=5, iters=9)}.get(
        algorithm, dict(starts=16, rounds=7))
    return _cls(algorithm)(app, window_s=window_s, launch=launch, **knobs, **more)


def _per_key(seen):
    """{group key: its requests} over the launches seen.  A window that closes
    between two requests of one key makes two launches of them, so the tests
    count requests per key, not launches."""
    out = {}
    for key, count in seen:
        out[key] = out.get(key, 0) + count
    return out


def _case(x=0, n=6, K=2, H=1):
    return solver.compact_vrp(*request((n, K, H, x, "")))


# ---------------------------------------------------------------------------
# a. what the real _gpu_launch hands on
# ---------------------------------------------------------------------------
# the launch's arguments between the instances and the seed
LAUNCH_KNOBS = {"sa": (777,), "ga": (48, 11, 0.2), "aco": (5, 9), "ls": (16, 7), "lsr": (16, 7),
                "lsf": (16, 7)}


def _recorder(app, seen):
    def launch(ctx, cis, *args, **kw):
        seen.append((ctx, list(cis), args, kw, {d: lock.locked() for d, lock in app.locks.items()}))
        tours = [list(range(ci.n, 0, -1)) for ci in cis]
        veh = [[0] * ci.n for ci in cis]
        durs = [[10 * ci.n] + [0] * (len(ci.capacities) - 1) for ci in cis]
        return tours, veh, durs
    return launch


@pytest.mark.parametrize("algorithm,spread", [(a, None) for a in ALGORITHMS] +
                         [("lsr", "auto"), ("lsr", 4)])          # only lsr has a spread
def test_gpu_launch_hands_on_its_knobs_the_seed_and_the_objective(monkeypatch, lib, algorithm, spread):
    _no_gpu(monkeypatch)
    app = _Devices((0, 1))
    b = _batcher(algorithm, app, **({"spread": spread} if algorithm == "lsr" else {}))
    # replaced after the batcher was made: the launch is looked up when it runs
    seen = []
    monkeypatch.setattr(solver, f"batch_{algorithm}_launch", _recorder(app, seen))
    monkeypatch.setattr(solver, "context", lambda dev=0: ("ctx", dev))
    ci, cj = _case(0), _case(1)
    more = (48, 11) if algorithm == "ga" else ()
    kw = {"spread": spread} if algorithm == "lsr" else {}
    for objective in ("sum", "max"):
        key = solver.batch_sa_key(ci) + (objective,) + more
        # the default device is the app's first
        out = b._gpu_launch(key, [ci, cj])
        assert out == ([[6, 5, 4, 3, 2, 1]] * 2, [([0] * 6, [60, 0])] * 2)
        ctx, cis, args, kwargs, held = seen.pop()
        assert ctx == ("ctx", 0) and len(cis) == 2 and cis[0] is ci and cis[1] is cj
        assert args == LAUNCH_KNOBS[algorithm] + (SEED, objective) and kwargs == kw
        assert [type(a) for a in args] == [type(a) for a in LAUNCH_KNOBS[algorithm]] + [int, str]
        assert held == {0: True, 1: False}
        b._gpu_launch(key, [cj], 1)
        ctx, cis, args, kwargs, held = seen.pop()
        assert ctx == ("ctx", 1) and len(cis) == 1 and cis[0] is cj
        assert args == LAUNCH_KNOBS[algorithm] + (SEED, objective) and kwargs == kw
        assert held == {0: False, 1: True}
    assert seen == [] and not any(lock.locked() for lock in app.locks.values())
    # and through the queue: solve() on a batcher without an injected launch
    res = b.solve(ci, "max", *more)
    assert res == {"durationMax": 60, "durationSum": 60,
                   "vehicles": [{"tour": [0, 6, 5, 4, 3, 2, 1, 0], "duration": 60},
                                {"tour": [0, 0], "duration": 0}]}
    (ctx, cis, args, kwargs, held), = seen
    assert ctx[0] == "ctx" and cis[0] is ci and held[ctx[1]] and sum(held.values()) == 1
    assert args == LAUNCH_KNOBS[algorithm] + (SEED, "max") and kwargs == kw
    # an objective that is not "max" is "sum"
    b.solve(ci, "mean", *more)
    assert seen[-1][2] == LAUNCH_KNOBS[algorithm] + (SEED, "sum")
    assert b.launches == 2 and b.requests == 2 and sum(b.per_device.values()) == 2


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_a_failing_real_launch_reaches_the_waiter_and_frees_the_lock(monkeypatch, lib, algorithm):
    app = _Devices()
    b = _batcher(algorithm, app)

    def failing(*a, **k):
        raise RuntimeError("launch failed")

    monkeypatch.setattr(solver, f"batch_{algorithm}_launch", failing)
    monkeypatch.setattr(solver, "context", lambda dev=0: "ctx")
    with pytest.raises(RuntimeError, match="launch failed"):
        b.solve(_case(0))
    assert not app.locks[0].locked() and b.launches == 0


# ---------------------------------------------------------------------------
# b. the device argument of an injected launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_an_injected_launch_takes_the_device_only_where_there_are_several(lib, algorithm):
    more = (48, 11) if algorithm == "ga" else ()
    seen = []

    def two(key, cis, dev):
        seen.append((key, len(cis), dev))
        return FAKES[algorithm]([])(key, cis)

    b = _batcher(algorithm, _Devices((3, 5)), 0.1, launch=two)
    cases = [_case(x, K=2 + x % 2) for x in range(6)]
    out = _concurrently(lambda x: b.solve(cases[x], "sum", *more), 6)
    assert all(isinstance(o, dict) for o in out), out
    # two group keys, so at least two launches, which take the devices in turn
    assert _per_key(s[:2] for s in seen) == {solver.batch_sa_key(cases[x]) + ("sum",) + more: 3
                                             for x in (0, 1)}
    assert {s[2] for s in seen} == {3, 5}
    assert b.per_device == {d: sum(s[1] for s in seen if s[2] == d) for d in (3, 5)}
    assert b.launches == len(seen) and b.requests == 6 and sum(b.per_device.values()) == 6

    seen = []
    one = _batcher(algorithm, _Devices((3,)), 0.1, launch=FAKES[algorithm](seen))   # (key, cis) alone
    out = _concurrently(lambda x: one.solve(cases[x], "sum", *more), 6)
    assert all(isinstance(o, dict) for o in out), out
    assert sorted(_per_key(seen).values()) == [3, 3]
    assert one.per_device == {3: 6} and one.launches == len(seen) and one.requests == 6


# ---------------------------------------------------------------------------
# c. group keys
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_group_keys(lib, algorithm):
    seen = []
    b = _batcher(algorithm, _Devices(), 0.1, launch=FAKES[algorithm](seen))
    ci, wide = _case(0), solver.compact_vrp(*request((6, 2, 1, 3, "e65536")))
    for c in (ci, wide, _case(1, K=3), _case(2, H=1 if algorithm == "lsf" else 24)):
        for objective in ("sum", "max"):
            job = {"ci": c, "objective": objective, "pop": 48, "gens": 11}
            want = solver.batch_sa_key(c) + (objective,) + ((48, 11) if algorithm == "ga" else ())
            assert b.group_key(job) == want
    assert solver.batch_sa_key(ci) == (7, 2, 1, False) and solver.batch_sa_key(wide) == (7, 2, 1, True)
    # one shape: the objectives never share a launch, nor do ga's populations or generations
    jobs = [("sum",), ("sum",), ("max",), ("other",)]
    if algorithm == "ga":
        jobs = [j + (48, 11) for j in jobs] + [("sum", 49, 11), ("sum", 48, 12), ("sum", 48, 11)]
    out = _concurrently(lambda x: b.solve(_case(x), *jobs[x]), len(jobs))
    assert all(isinstance(o, dict) for o in out), out
    shape = (7, 2, 1, False)
    if algorithm == "ga":
        assert _per_key(seen) == {shape + ("max", 48, 11): 1, shape + ("sum", 48, 11): 4,
                                  shape + ("sum", 48, 12): 1, shape + ("sum", 49, 11): 1}
    else:
        assert _per_key(seen) == {shape + ("max",): 1, shape + ("sum",): 3}
    if algorithm == "ga":      # solve()'s defaults are solve_vrp's
        del seen[:]
        b.solve(ci)
        assert seen == [(shape + ("sum", 256, 400), 1)]


# ---------------------------------------------------------------------------
# d. both call forms of accepts
# ---------------------------------------------------------------------------
def _lds(algorithm, N, knob):
    more = {"ga": (knob,), "aco": (knob,)}.get(algorithm, ())
    return getattr(core, f"vrp_batch_{algorithm}_lds")(N, 2, 1, False, *more)


def _edge(algorithm, knob):
    """The largest N (K = 2, a static uint16 matrix) whose launch fits the LDS."""
    N = 2
    while _lds(algorithm, N + 1, knob) <= LDS_BYTES:
        N += 1
    assert 2 < N < 400
    return N


def _accepts(algorithm, knob=None):
    """accepts as the service calls it: on the class for sa and ga, on an
    instance at `knob` ants or the batcher's starts and rounds for the rest."""
    if algorithm == "sa":
        return service.VrpSaBatcher.accepts
    if algorithm == "ga":
        return functools.partial(service.VrpGaBatcher.accepts, pop=knob, gens=400)
    if algorithm == "aco":
        return service.VrpAcoBatcher(_Devices(), ants=knob, launch=_fake_launch([])).accepts
    return _batcher(algorithm, _Devices(), launch=_fake_launch([])).accepts


@pytest.mark.parametrize("algorithm,knob", [("sa", None), ("ga", 256), ("ga", 64), ("aco", 256),
                                            ("aco", 64), ("ls", None), ("lsr", None), ("lsf", None)])
def test_accepts_at_the_edges_of_the_domain(lib, algorithm, knob):
    accepts = _accepts(algorithm, knob)
    N = _edge(algorithm, knob)
    assert accepts(_sized(N, 2, 1)) is True and accepts(_sized(N + 1, 2, 1)) is False
    small = _sized(6, 2, 1)
    assert accepts(small) is True
    assert accepts(_sized(6, 2, 1, 2**29)) is False                      # the A9 guard
    assert solver.batch_guard_message(_sized(6, 2, 1, 2**29)) is not None
    assert accepts(_sized(5, 64, 1)) is True and accepts(_sized(5, 65, 1)) is False
    tsp = solver.compact_tsp(np.ones((4, 4), dtype=np.int64), [1, 2, 3], 0, 0)
    assert accepts(tsp) is False
    none = solver.compact_vrp(np.ones((3, 3), dtype=np.int64), _locs([0, 1, 1]), [3], [0], [1, 2])
    assert none.n == 0 and accepts(none) is False
    assert accepts(_sized(6, 2, 24)) is (algorithm != "lsf")              # lsf: static matrices only


def test_accepts_uses_the_knobs_it_is_given(lib):
    small = _sized(6, 2, 1)
    cap = solver.BATCH_GA_MAX_GENERATIONS
    ga = service.VrpGaBatcher.accepts
    assert ga(small) and ga(small, 2, 0) and ga(small, 256, cap)          # the defaults: 256, 400
    assert not ga(small, 1, 400) and not ga(small, 257, 400) and not ga(small, 256, cap + 1)
    assert not ga(small, 256, -1)
    on_an_instance = service.VrpGaBatcher(_Devices(), launch=_fake_launch([])).accepts
    assert on_an_instance(small, 64, 10) and not on_an_instance(small, 257, 10)
    assert service.VrpSaBatcher(_Devices(), launch=_fake_launch([])).accepts(small)
    # an instance's own knobs decide: the edge moves with the ants
    few, many = _edge("aco", 64), _edge("aco", 256)
    assert many < few
    assert _accepts("aco", 64)(_sized(few, 2, 1)) and not _accepts("aco", 256)(_sized(few, 2, 1))
    assert _accepts("aco", 256)(_sized(many, 2, 1))


# ---------------------------------------------------------------------------
# e. the constructors
# ---------------------------------------------------------------------------
def _refusal(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value)


def test_constructor_refusals_in_full(lib):
    app, fake = _Devices(), _fake_launch([])
    aco = functools.partial(service.VrpAcoBatcher, app, launch=fake)
    assert _refusal(lambda: aco(ants=0)) == "ants must be in 1..256 (0 given)"
    assert _refusal(lambda: aco(ants=257)) == "ants must be in 1..256 (257 given)"
    assert _refusal(lambda: aco(iters=0)) == "iters must be in 1..1000 (0 given)"
    assert _refusal(lambda: aco(iters=1001)) == "iters must be in 1..1000 (1001 given)"
    assert _refusal(lambda: aco(ants=0, iters=0)) == "ants must be in 1..256 (0 given)"
    for ants, iters in ((1, 1), (256, 1000)):
        b = aco(ants=ants, iters=iters)
        assert (b.ants, b.iters) == (ants, iters)
    for algorithm in ("ls", "lsr", "lsf"):
        make = functools.partial(_cls(algorithm), app, launch=fake)
        assert _refusal(lambda: make(starts=0)) == "starts must be in 1..1024 (0 given)"
        assert _refusal(lambda: make(starts=1025)) == "starts must be in 1..1024 (1025 given)"
        assert _refusal(lambda: make(rounds=-1)) == "rounds must be in 0..1000 (-1 given)"
        assert _refusal(lambda: make(rounds=1001)) == "rounds must be in 0..1000 (1001 given)"
        assert _refusal(lambda: make(starts=0, rounds=-1)) == "starts must be in 1..1024 (0 given)"
        for starts, rounds in ((1, 0), (1024, 1000)):
            b = make(starts=starts, rounds=rounds)
            assert (b.starts, b.rounds) == (starts, rounds)
    lsr = functools.partial(service.VrpLsrBatcher, app, launch=fake)
    spread = 'spread must be None, "auto" or an integer in 1..1024 '
    assert _refusal(lambda: lsr(spread=0)) == spread + "(0 given)"
    assert _refusal(lambda: lsr(spread=1025)) == spread + "(1025 given)"
    assert _refusal(lambda: lsr(spread=True)) == spread + "(True given)"
    assert _refusal(lambda: lsr(spread="4")) == spread + "('4' given)"
    assert _refusal(lambda: lsr(spread=2.0)) == spread + "(2.0 given)"
    assert _refusal(lambda: lsr(spread=0, starts=0)) == spread + "(0 given)"
    for ok in (None, "auto", 1, 1024):
        assert lsr(spread=ok).spread == ok
    for algorithm in ("ls", "lsf"):          # spread is lsr's alone
        with pytest.raises(TypeError, match="spread"):
            _cls(algorithm)(app, launch=fake, spread=4)


def test_constructor_parameters_and_class_relations(lib):
    app, fake = _Devices(), _fake_launch([])
    b = service.VrpSaBatcher(app, 0.25, 9, 33, fake)
    assert (b.window_s, b.steps, b.max_batch, b._launch) == (0.25, 9, 33, fake)
    b = service.VrpSaBatcher(app)
    assert (b.window_s, b.steps, b.max_batch) == (0.005, 2000, 16384) and b._launch == b._gpu_launch
    b = service.VrpGaBatcher(app, 0.25, launch=fake)
    assert (b.window_s, b.max_batch, b._launch, b.pmut) == (0.25, 16384, fake, 0.2)
    b = service.VrpAcoBatcher(app, 0.25, 9, 5, 33, fake)                    # iters, then ants
    assert (b.window_s, b.iters, b.ants, b.max_batch, b._launch) == (0.25, 9, 5, 33, fake)
    b = service.VrpAcoBatcher(app)
    assert (b.window_s, b.iters, b.ants, b.max_batch) == (0.005, 100, 64, 16384)
    for algorithm in ("ls", "lsr", "lsf"):
        b = _cls(algorithm)(app, 0.25, 7, 16, 33, fake)                     # rounds, then starts
        assert (b.window_s, b.rounds, b.starts, b.max_batch, b._launch) == (0.25, 7, 16, 33, fake)
        b = _cls(algorithm)(app)
        assert (b.window_s, b.rounds, b.starts, b.max_batch) == (0.005, 1000, 64, 16384)
        assert b._launch == b._gpu_launch
    assert service.VrpLsrBatcher(app, 0.25, 7, 16, 33, fake, "auto").spread == "auto"
    for sub in ("ga", "aco", "ls"):
        assert issubclass(_cls(sub), service.VrpSaBatcher)
    for sub in ("lsr", "lsf"):
        assert issubclass(_cls(sub), service.VrpLsBatcher)
    assert issubclass(service.VrpSaBatcher, service.TspBatcher)
    assert not issubclass(service.VrpLsfBatcher, service.VrpLsrBatcher)
    assert not issubclass(service.VrpSaBatcher, service.ExactBatcher)
    # the knobs are the constructor's, as integers
    b = service.VrpLsBatcher(app, starts="8", rounds=3.0, launch=fake)
    assert (b.starts, b.rounds) == (8, 3) and type(b.starts) is int and type(b.rounds) is int
    b = service.VrpAcoBatcher(app, ants="8", iters=3.0, launch=fake)
    assert (b.ants, b.iters) == (8, 3) and type(b.ants) is int and type(b.iters) is int


# ---------------------------------------------------------------------------
# f. the routing matrix
# ---------------------------------------------------------------------------
FLAGS_ON = {f"batch_vrp_{a}": True for a in ALGORITHMS}


def _routing_app(seen, launched, **more):
    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((problem, algorithm, dict(knobs.get("inline") or {})))
        return {"durationMax": 2, "durationSum": 3, "vehicles": [], "duration": 3, "vehicle": []}

    launches = {f"batch_vrp_{a}_launch": FAKES[a](launched[a]) for a in ALGORITHMS}
    D, locs, caps, starts = request((5, 2, 1, 1, ""), 100)
    store = service.MemoryStore({"7": locs}, {"8": D}, {})
    return service.App(store, solve=fake, batch_window_s=0.05, **FLAGS_ON, **launches, **more)


def _api(**more):
    D, locs, caps, starts = request((5, 2, 1, 1, ""), 100)
    return json.dumps(dict({"solutionName": "s", "solutionDescription": "d", "locationsKey": 7,
                            "durationsKey": 8, "capacities": caps, "startTimes": starts,
                            "ignoredCustomers": [], "completedCustomers": []}, **more)).encode()


GA = dict(multiThreaded=False, randomPermutationCount=32, iterationCount=6)


def test_every_route_rides_its_own_batcher_and_no_other(lib):
    seen, launched = [], {a: [] for a in ALGORITHMS}
    app = _routing_app(seen, launched)
    for a in ALGORITHMS:
        assert type(getattr(app, ATTRIBUTES[a])) is _cls(a)
        assert getattr(app, ATTRIBUTES[a]).window_s == 0.05
    assert app.batcher is None and app.exact_batcher is None and app.exact_vrp_batcher is None
    assert app.exact_tdp_batcher is None and app.exact_tdsp_batcher is None
    body = _body((5, 2, 1, 1, ""))
    out = _concurrently(lambda x: app.solve_inline("vrp", ALGORITHMS[x], body), 6)
    assert all(st == 200 for st, _ in out), out
    shape = (6, 2, 1, False, "sum")
    assert launched == {a: [(shape + ((256, 400) if a == "ga" else ()), 1)] for a in ALGORITHMS}
    assert seen == []
    for st, res in out:
        assert res == {"success": True, "message": {
            "durationMax": 50, "durationSum": 50,
            "vehicles": [{"tour": [0, 5, 4, 3, 2, 1, 0], "duration": 50},
                         {"tour": [0, 0], "duration": 0}]}}
    # the objective is the request's; an empty knobs object names no knob
    out = _concurrently(lambda x: app.solve_inline(
        "vrp", ALGORITHMS[x], _body((5, 2, 1, 1, ""), objective="max", knobs={})), 6)
    assert all(st == 200 for st, _ in out), out
    assert all(launched[a][1][0][:5] == (6, 2, 1, False, "max") for a in ALGORITHMS) and seen == []
    assert all(getattr(app, ATTRIBUTES[a]).requests == 2 for a in ALGORITHMS)

    # what rides none of them
    def unbatched(status_and_result, *want):
        assert status_and_result[0] == 200, status_and_result
        assert seen == [want]
        del seen[:]

    tsp = json.dumps({"durations": request((5, 2, 1, 1, ""))[0], "customers": [1, 2, 3],
                      "startNode": 0, "startTime": 0}).encode()
    unbatched(app.solve_inline("tsp", "sa", tsp), "tsp", "sa", {})
    unbatched(app.solve_inline("vrp", "bf", body), "vrp", "bf", {})
    unbatched(app.solve_inline("vrp", "sp", body), "vrp", "sp", {})
    unbatched(app.solve_inline("vrp", "tdsp", body), "vrp", "tdsp", {})
    unbatched(app.post("vrp", "bf", _api()), "vrp", "bf", {})
    st, res = app.solve_inline("vrp", "lso", body)
    assert st == 400 and "no solver /solve/vrp/lso" in res["errors"][0]["reason"] and seen == []
    # any inline knob, the algorithm's own or not
    own = {"sa": "steps", "ga": "pop", "aco": "ants", "ls": "starts", "lsr": "spread", "lsf": "rounds"}
    for a in ALGORITHMS:
        for knob in (own[a], "window"):
            unbatched(app.solve_inline("vrp", a, _body((5, 2, 1, 1, ""), knobs={knob: 3})),
                      "vrp", a, {knob: 3})
    # outside the domain: 65 vehicles; for lsf an hour-indexed matrix too
    D, locs, caps, starts = request((5, 2, 1, 1, ""), 100)
    wide_fleet = json.dumps({"durations": D, "locations": locs, "capacities": [1] * 65,
                             "startTimes": [0] * 65, "ignoredCustomers": [],
                             "completedCustomers": []}).encode()
    for a in ALGORITHMS:
        unbatched(app.solve_inline("vrp", a, wide_fleet), "vrp", a, {})
    unbatched(app.solve_inline("vrp", "lsf", _body((5, 2, 24, 1, ""))), "vrp", "lsf", {})
    assert all(len(launched[a]) == 2 for a in ALGORITHMS)


def test_ga_requests_carry_their_own_population_and_generations(lib):
    seen, launched = [], {a: [] for a in ALGORITHMS}
    app = _routing_app(seen, launched)
    cap = solver.BATCH_GA_MAX_GENERATIONS
    assert solver.ga_knobs(None, None) == (256, 400) and solver.ga_knobs(1, 7) == (2, 7)
    bodies = [dict(), dict(randomPermutationCount=1), dict(randomPermutationCount=256, iterationCount=cap),
              dict(randomPermutationCount=32, iterationCount=6)]

    def call(x):
        if x < 4:
            return app.solve_inline("vrp", "ga", _body((5, 2, 1, x, ""), **bodies[x]))
        if x == 4:
            return app.post("vrp", "ga", _api(**GA))
        if x == 5:       # multiThreaded false, or deciding nothing
            return app.post("vrp", "ga", _api(**dict(GA, multiThreaded="0", iterationCount=None)))
        return app.post("vrp", "ga", _api(**dict(GA, multiThreaded="maybe", randomPermutationCount=0)))

    out = _concurrently(call, 7)
    assert all(st == 200 for st, _ in out), out
    shape = (6, 2, 1, False, "sum")
    assert _per_key(launched["ga"]) == {shape + (2, 400): 1, shape + (32, 6): 2, shape + (32, 400): 1,
                                        shape + (256, 6): 1, shape + (256, 400): 1,
                                        shape + (256, cap): 1}
    assert seen == [] and all(launched[a] == [] for a in ALGORITHMS if a != "ga")

    def unbatched(status_and_result):
        assert status_and_result[0] == 200, status_and_result
        assert seen == [("vrp", "ga", {})]
        del seen[:]

    for mt in (True, "true", 1):
        unbatched(app.post("vrp", "ga", _api(**dict(GA, multiThreaded=mt))))
    unbatched(app.solve_inline("vrp", "ga", _body((5, 2, 1, 1, ""), randomPermutationCount=257)))
    unbatched(app.post("vrp", "ga", _api(**dict(GA, randomPermutationCount=257))))
    unbatched(app.solve_inline("vrp", "ga", _body((5, 2, 1, 1, ""), iterationCount=cap + 1)))
    unbatched(app.post("vrp", "ga", _api(**dict(GA, iterationCount=cap + 1))))
    assert sum(_per_key(launched["ga"]).values()) == 7


def test_the_endpoints_ride_the_same_batchers(lib):
    seen, launched = [], {a: [] for a in ALGORITHMS}
    app = _routing_app(seen, launched, batch_steps=9, batch_aco_iterations=7, batch_aco_ants=3,
                       batch_ls_starts=11, batch_ls_rounds=12, batch_lsr_starts=13,
                       batch_lsr_rounds=14, batch_lsr_spread="auto", batch_lsf_starts=15,
                       batch_lsf_rounds=16, seed=5)
    # App's keywords are the batchers' knobs
    assert app.vrp_sa_batcher.steps == 9 and app.seed == 5
    assert (app.vrp_aco_batcher.iters, app.vrp_aco_batcher.ants) == (7, 3)
    assert (app.vrp_ls_batcher.starts, app.vrp_ls_batcher.rounds) == (11, 12)
    assert (app.vrp_lsr_batcher.starts, app.vrp_lsr_batcher.rounds) == (13, 14)
    assert app.vrp_lsr_batcher.spread == "auto"
    assert (app.vrp_lsf_batcher.starts, app.vrp_lsf_batcher.rounds) == (15, 16)
    assert all(getattr(app, ATTRIBUTES[a]).app is app for a in ALGORITHMS)
    routes = ("sa", "ga", "aco")
    out = _concurrently(lambda x: app.post("vrp", routes[x % 3], _api(**(GA if x % 3 == 1 else {}))), 6)
    assert all(st == 200 for st, _ in out), out
    shape = (6, 2, 1, False, "sum")
    assert _per_key(launched["sa"]) == {shape: 2} and _per_key(launched["aco"]) == {shape: 2}
    assert _per_key(launched["ga"]) == {shape + (32, 6): 2}
    assert seen == [] and all(launched[a] == [] for a in ("ls", "lsr", "lsf"))
    assert out[0][1]["message"]["vehicles"][0]["tour"] == [0, 5, 4, 3, 2, 1, 0]


def test_defaults_and_flags_off(lib):
    off = service.App(service.MemoryStore({}, {}, {}), solve=lambda *a: None)
    assert all(getattr(off, ATTRIBUTES[a]) is None for a in ALGORITHMS)
    one_at_a_time = {a: service.App(service.MemoryStore({}, {}, {}), solve=lambda *a: None,
                                    **{f"batch_vrp_{a}": True,
                                       f"batch_vrp_{a}_launch": _fake_launch([])})
                     for a in ALGORITHMS}
    for a, app in one_at_a_time.items():
        assert [b for b in ALGORITHMS if getattr(app, ATTRIBUTES[b]) is not None] == [a]
        assert getattr(app, ATTRIBUTES[a]).window_s == 0.005
    assert one_at_a_time["sa"].vrp_sa_batcher.steps == 2000
    b = one_at_a_time["aco"].vrp_aco_batcher
    assert (b.iters, b.ants) == (100, 64)
    for a in ("ls", "lsr", "lsf"):
        b = getattr(one_at_a_time[a], ATTRIBUTES[a])
        assert (b.starts, b.rounds) == (64, 1000)
    assert one_at_a_time["lsr"].vrp_lsr_batcher.spread is None
    # a knob out of range is refused where the app is made, flag on
    store = service.MemoryStore({}, {}, {})
    assert _refusal(lambda: service.App(store, batch_vrp_ls=True, batch_ls_starts=0)) == \
        "starts must be in 1..1024 (0 given)"
    assert _refusal(lambda: service.App(store, batch_vrp_lsf=True, batch_lsf_rounds=1001)) == \
        "rounds must be in 0..1000 (1001 given)"
    assert _refusal(lambda: service.App(store, batch_vrp_aco=True, batch_aco_iterations=0)) == \
        "iters must be in 1..1000 (0 given)"
    assert "spread must be" in _refusal(lambda: service.App(store, batch_vrp_lsr=True,
                                                            batch_lsr_spread=0))
    # and not looked at with the flag off
    assert service.App(store, batch_ls_starts=0, batch_lsr_spread=0).vrp_ls_batcher is None


# ---------------------------------------------------------------------------
# g. the command line
# ---------------------------------------------------------------------------
DEFAULT_KEYWORDS = dict(
    device=0, seed=0, max_seconds=None, batch_tsp=False, batch_window_s=pytest.approx(0.005),
    batch_steps=2000, devices=None, batch_exact=False, batch_exact_tdsp=False, batch_vrp_sa=False,
    batch_vrp_ga=False, batch_vrp_aco=False, batch_aco_iterations=100, batch_aco_ants=64,
    batch_vrp_ls=False, batch_ls_starts=64, batch_ls_rounds=1000, batch_vrp_lsr=False,
    batch_lsr_starts=64, batch_lsr_rounds=1000, batch_lsr_spread=None, batch_vrp_lsf=False,
    batch_lsf_starts=64, batch_lsf_rounds=1000)
EVERY_FLAG = ["--batch-vrp-sa", "--batch-vrp-ga", "--batch-vrp-aco", "--batch-aco-iterations", "7",
              "--batch-aco-ants", "3", "--batch-vrp-ls", "--batch-ls-starts", "11",
              "--batch-ls-rounds", "12", "--batch-vrp-lsr", "--batch-lsr-starts", "13",
              "--batch-lsr-rounds", "14", "--batch-vrp-lsf", "--batch-lsf-starts", "15",
              "--batch-lsf-rounds", "16", "--batch-tsp", "--batch-exact", "--batch-exact-tdsp",
              "--batch-window-ms", "20", "--batch-steps", "9"]
EVERY_KEYWORD = dict(
    device=0, seed=0, max_seconds=None, batch_tsp=True, batch_window_s=pytest.approx(0.02),
    batch_steps=9, devices=None, batch_exact=True, batch_exact_tdsp=True, batch_vrp_sa=True,
    batch_vrp_ga=True, batch_vrp_aco=True, batch_aco_iterations=7, batch_aco_ants=3,
    batch_vrp_ls=True, batch_ls_starts=11, batch_ls_rounds=12, batch_vrp_lsr=True,
    batch_lsr_starts=13, batch_lsr_rounds=14, batch_vrp_lsf=True, batch_lsf_starts=15,
    batch_lsf_rounds=16)


def _main_keywords(monkeypatch, argv):
    made = []

    class Stop(Exception):
        pass

    def app(*args, **kw):
        made.append((args, kw))
        raise Stop

    monkeypatch.setattr(service, "App", app)
    with pytest.raises(Stop):
        service.main(argv)
    (args, kw), = made
    assert len(args) == 1 and isinstance(args[0], service.MemoryStore)
    return kw


def test_main_hands_app_these_keywords_and_no_others(monkeypatch):
    assert _main_keywords(monkeypatch, []) == DEFAULT_KEYWORDS
    for text, value in (("auto", "auto"), ("7", 7)):
        kw = _main_keywords(monkeypatch, EVERY_FLAG + ["--batch-lsr-spread", text])
        assert kw == dict(EVERY_KEYWORD, batch_lsr_spread=value)
        assert type(kw["batch_lsr_spread"]) is type(value)
        assert all(type(kw[k]) is int for k in kw if k.endswith(("_starts", "_rounds", "_ants",
                                                                 "_iterations", "_steps")))
    kw = _main_keywords(monkeypatch, ["--device", "2", "--devices", "1,0,1", "--seed", "5",
                                      "--max-seconds", "1.5"])
    assert kw == dict(DEFAULT_KEYWORDS, device=2, devices=[1, 0], seed=5, max_seconds=1.5)
    # the range ends themselves are taken
    kw = _main_keywords(monkeypatch, [
        "--batch-aco-iterations", "1000", "--batch-aco-ants", "256", "--batch-ls-starts", "1",
        "--batch-ls-rounds", "0", "--batch-lsr-starts", "1024", "--batch-lsr-rounds", "1000",
        "--batch-lsf-starts", "1", "--batch-lsf-rounds", "0", "--batch-lsr-spread", "1024"])
    assert kw == dict(DEFAULT_KEYWORDS, batch_aco_iterations=1000, batch_aco_ants=256,
                      batch_ls_starts=1, batch_ls_rounds=0, batch_lsr_starts=1024,
                      batch_lsr_rounds=1000, batch_lsf_starts=1, batch_lsf_rounds=0,
                      batch_lsr_spread=1024)


# (flag, the least and the largest value it takes, texts it refuses)
RANGED = [("--batch-aco-iterations", 1, 1000, ()), ("--batch-aco-ants", 1, 256, ()),
          ("--batch-lsr-spread", 1, 1024, ("Auto", "x", "1.5", ""))] + \
         [(f"--batch-{a}-starts", 1, 1024, ("x",)) for a in ("ls", "lsr", "lsf")] + \
         [(f"--batch-{a}-rounds", 0, 1000, ("x",)) for a in ("ls", "lsr", "lsf")]


@pytest.mark.parametrize("flag,lo,hi,texts", RANGED, ids=[r[0] for r in RANGED])
def test_main_refuses_a_value_out_of_range(monkeypatch, capsys, flag, lo, hi, texts):
    monkeypatch.setattr(service, "App", lambda *a, **k: pytest.fail("the app was made"))
    for value in (lo - 1, hi + 1):             # an integer out of range is told the range
        with pytest.raises(SystemExit) as e:
            service.main([flag, str(value)])
        assert e.value.code == 2
        assert f"argument {flag}: must be in {lo}..{hi} ({value} given)" in capsys.readouterr().err
    for text in texts:
        with pytest.raises(SystemExit) as e:
            service.main([flag, text])
        assert e.value.code == 2
        assert f"argument {flag}: " in capsys.readouterr().err


def test_help_states_every_range_and_its_constant(monkeypatch, capsys):
    monkeypatch.setenv("COLUMNS", "100000")     # no line breaks inside a flag's name
    with pytest.raises(SystemExit) as e:
        service.main(["--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    for a in ("ls", "lsr", "lsf"):
        assert f"--batch-{a}-starts" in text and f"1..1024 (solver.BATCH_{a.upper()}_MAX_STARTS)" in text
        assert f"--batch-{a}-rounds" in text and f"0..1000 (solver.BATCH_{a.upper()}_MAX_ROUNDS)" in text
        assert f"--batch-vrp-{a}" in text and f"vrp_batch_{a} launches" in text
    assert "1..1000 (solver.BATCH_ACO_MAX_ITERATIONS)" in text
    assert "1..256 (solver.BATCH_ACO_MAX_ANTS)" in text
    assert "--batch-lsr-spread {auto,N}" in text and "1..1024 (solver.BATCH_LSR_MAX_SPREAD)" in text


# ---------------------------------------------------------------------------
# h. unknown keywords
# ---------------------------------------------------------------------------
def test_app_refuses_a_keyword_it_does_not_know():
    store = service.MemoryStore({}, {}, {})
    for name in ("batch_vrp_xyz", "batch_vrp_lso", "batch_xyz_starts", "batch_vrp_sa_lunch"):
        with pytest.raises(TypeError, match=name):
            service.App(store, **{name: True})
