"""The host path the six batched heuristics share -- solve_vrp_sa_batch,
solve_vrp_ga_batch, solve_vrp_aco_batch, solve_vrp_ls_batch,
solve_vrp_lsr_batch and solve_tsp_lso_batch -- pinned entry point by entry
point with the remote, the context, the single-request solver and the launch
faked: the request index on a bad request, the keyword dict that reaches a GPU
box or the fallback, the host's answer for no customer, one launch per key in
first-appearance order with the outputs in request order, and what a request
outside the domain does.  Needs the library (the LDS size functions), no GPU."""
import numpy as np
import pytest

from vrpms_amd import solver

SEED, DEVICE = 7, 3


@pytest.fixture(scope="module")
def lib():
    from vrpms_amd import _lib
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


def _matrix(N, tag):
    D = np.random.default_rng(100 + tag).integers(3, 60, size=(N, N))
    np.fill_diagonal(D, 0)
    return D.tolist()


def vrp_request(n, K, tag, ignored=()):
    """n customers, K vehicles; the start times carry `tag`, so the fake
    launch's durations tell the requests apart."""
    return (_matrix(n + 1, tag), [{"id": i, "demand": 1} for i in range(n + 1)], [n] * K,
            [10 * tag + k for k in range(K)], list(ignored), [])


def tsp_request(n, tag, customers=None):
    return (_matrix(n + 1, tag), list(range(1, n + 1)) if customers is None else customers, 0, tag)


def vrp_rows(cis):
    """A launch's (tours, veh, durs): every customer on vehicle 0 in index
    order, the route durations the request's start times."""
    return ([list(range(1, ci.n + 1)) for ci in cis], [[0] * ci.n for ci in cis],
            [[int(s) for s in ci.start_times] for ci in cis])


def vrp_answer(r, with_unvisited):
    n, starts = len(r[1]) - 1, r[3]
    out = {"durationMax": max(starts), "durationSum": sum(starts),
           "vehicles": [{"tour": [0] + (list(range(1, n + 1)) if k == 0 else []) + [0], "duration": s}
                        for k, s in enumerate(starts)]}
    if with_unvisited:
        out["unvisited"] = []
    return out


def tsp_rows(cis):
    return [list(range(1, ci.n + 1)) for ci in cis], [int(ci.start_times[0]) for ci in cis]


def tsp_answer(r, with_unvisited):
    return {"duration": r[3], "vehicle": [0] + list(r[1]) + [0]}


VRP = dict(single="solve_vrp", request=vrp_request, rows=vrp_rows, answer=vrp_answer,
           bad=lambda: vrp_request(4, 2, 0)[:3] + ([0],),
           bad_message="capacities and startTimes must have the same length",
           empty=lambda: vrp_request(4, 2, 5, ignored=[1, 2, 3, 4]),
           empty_answer={"durationMax": 0, "durationSum": 0, "unvisited": [],
                         "vehicles": [{"tour": [0, 0], "duration": 0}] * 2},
           # 65 vehicles: outside every VRP kernel's domain at any size
           outside=lambda: vrp_request(3, 65, 1))
BASE = dict(seed=SEED, objective="max", with_unvisited=True)
# per algorithm: the entry point's own knobs, the keywords that travel to
# solve_vrp / solve_tsp next to `seed` (and, for a VRP, `objective` and
# `with_unvisited`), what the launch gets after (ctx, cis), and the message of
# a request outside the domain (None: it takes the single-request solver)
ALGS = {
    "sa": dict(VRP, knobs=dict(steps=50), travels={}, launch=((50, SEED, "max"), {}), refusal=None),
    "ga": dict(VRP, knobs=dict(pop=8, gens=5, pmut=0.25),
               travels=dict(random_permutation_count=8, iteration_count=5),
               launch=((8, 5, 0.25, SEED, "max"), {}), refusal=None),
    "aco": dict(VRP, knobs=dict(ants=6, iters=4), travels=dict(iteration_count=4, ants=6),
                launch=((6, 4, SEED, "max"), {}), refusal=None),
    "ls": dict(VRP, knobs=dict(starts=8, rounds=3), travels=dict(starts=8, rounds=3),
               launch=((8, 3, SEED, "max"), {}),
               refusal=r"ls \(local search\) supports 1\.\.64 vehicles \(65 given\)"),
    "lsr": dict(VRP, knobs=dict(starts=8, rounds=3), travels=dict(starts=8, rounds=3),
                launch=((8, 3, SEED, "max"), dict(spread=None)), spread=True,
                refusal=r"lsr \(local search\) supports 1\.\.64 vehicles \(65 given\)"),
    "lso": dict(single="solve_tsp", request=lambda n, K, tag: tsp_request(n, tag), rows=tsp_rows,
                answer=tsp_answer, knobs=dict(starts=8, rounds=3, moves=7),
                travels=dict(starts=8, rounds=3, moves=7), launch=((8, 3, 7, SEED), dict(spread=None)),
                spread=True, bad=lambda: tsp_request(4, 0, customers=[1, 99]),
                bad_message="customer 99 outside the 5-node matrix",
                empty=lambda: tsp_request(4, 5, customers=[]),
                empty_answer={"duration": 0, "vehicle": [0, 0]},
                # the smallest way out of the TSP's domain is the LDS: 24 slices
                # of 60 x 60 int32 cells are 345,600 bytes
                outside=lambda: (np.full((24, 60, 60), 70000), list(range(1, 60)), 0, 0),
                refusal=r"lso \(local search\) keeps the matrix in LDS: 59 customers and 24 hour "
                        r"slice\(s\) of int32 cells need \d+ bytes; the limit is 163840 bytes"),
}


def entry(alg):
    return getattr(solver, f"solve_{'tsp' if alg == 'lso' else 'vrp'}_{alg}_batch")


def call(alg, requests, **more):
    a = ALGS[alg]
    kw = dict(a["knobs"], seed=SEED, **more)
    if a["single"] == "solve_vrp":
        kw.update(objective="max", with_unvisited=True)
    return entry(alg)(requests, **kw)


def shared(alg):
    a = ALGS[alg]
    return dict(BASE if a["single"] == "solve_vrp" else dict(seed=SEED), **a["travels"])


def touched(what):
    def fail(*a, **k):
        pytest.fail(f"{what} was touched")
    return fail


class Fakes:
    """_remote, context, the single-request solver and the algorithm's launch,
    each recording its calls; a remote of None means a local GPU."""

    def __init__(self, monkeypatch, alg, remote=None):
        self.alg, self.singles, self.launches, self.devices = alg, [], [], []
        a = ALGS[alg]
        monkeypatch.setattr(solver, "_remote", lambda: remote)
        monkeypatch.setattr(solver, "context", self.context)
        monkeypatch.setattr(solver, "Context", touched("Context"))
        monkeypatch.setattr(solver, a["single"], self.single)
        monkeypatch.setattr(solver, f"batch_{alg}_launch", self.launch)

    def context(self, device=0):
        self.devices.append(device)
        return ("ctx", device)

    def single(self, algorithm, *request, **kw):
        self.singles.append((algorithm, request, kw))
        return {"single": len(self.singles)}

    def launch(self, ctx, cis, *args, **kw):
        self.launches.append((ctx, [ci.N for ci in cis], args, kw))
        return ALGS[self.alg]["rows"](cis)


@pytest.mark.parametrize("alg", list(ALGS))
def test_a_bad_request_raises_with_its_index_before_anything_is_touched(monkeypatch, lib, alg):
    a = ALGS[alg]
    monkeypatch.setattr(solver, "_remote", touched("the remote"))
    monkeypatch.setattr(solver, "context", touched("the context"))
    monkeypatch.setattr(solver, "Context", touched("Context"))
    good = a["request"](4, 2, 1)
    for x in (0, 2):
        with pytest.raises(ValueError) as e:
            call(alg, [good] * x + [a["bad"]()] + [good])
        assert str(e.value) == f"request {x}: {a['bad_message']}"
    # the int32 guard is one of the checks
    big = (np.full((5, 5), 2**29).tolist(),) + good[1:]
    with pytest.raises(ValueError, match=r"^request 1: start \+ \(N\+K\+1\)\*max_duration overflows"):
        call(alg, [good, big])


@pytest.mark.parametrize("alg", list(ALGS))
def test_a_remote_gets_every_request_with_the_shared_knobs(monkeypatch, lib, alg):
    a = ALGS[alg]
    f = Fakes(monkeypatch, alg, remote=object())
    reqs = [a["request"](4, 2, 1), a["request"](3, 1, 2), a["empty"]()]
    assert call(alg, reqs) == [{"single": 1}, {"single": 2}, {"single": 3}]
    assert f.singles == [(alg, tuple(r), shared(alg)) for r in reqs]
    assert f.launches == [] and f.devices == []
    if a.get("spread"):   # only a number travels
        for spread, more in ((4, dict(spread=4)), (np.int64(6), dict(spread=6)), ("auto", {}), (None, {})):
            del f.singles[:]
            call(alg, reqs[:1], spread=spread)
            assert f.singles == [(alg, tuple(reqs[0]), dict(shared(alg), **more))]
            assert type(f.singles[0][2].get("spread", 0)) is int


@pytest.mark.parametrize("alg", list(ALGS))
def test_no_customer_is_answered_on_the_host(monkeypatch, lib, alg):
    a = ALGS[alg]
    f = Fakes(monkeypatch, alg)
    assert call(alg, [a["empty"](), a["empty"]()]) == [a["empty_answer"]] * 2
    assert f.launches == [] and f.singles == [] and f.devices == []


@pytest.mark.parametrize("alg", list(ALGS))
def test_one_launch_per_key_in_first_appearance_order(monkeypatch, lib, alg):
    a = ALGS[alg]
    f = Fakes(monkeypatch, alg)
    # two keys, interleaved, the second key's node count the smaller; a request
    # with no customer among them
    reqs = [a["request"](5, 2, 1), a["request"](3, 2, 2), a["empty"](), a["request"](5, 2, 3),
            a["request"](3, 2, 4), a["request"](5, 2, 5)]
    out = call(alg, reqs, device=DEVICE)
    args, kw = a["launch"]
    assert f.launches == [(("ctx", DEVICE), [6, 6, 6], args, kw), (("ctx", DEVICE), [4, 4], args, kw)]
    assert f.devices == [DEVICE] and f.singles == []
    want = [a["answer"](r, True) for r in reqs]
    want[2] = a["empty_answer"]
    assert out == want
    if a.get("spread"):   # the launch gets the call's, as checked
        for spread, seen in ((5, 5), (np.int64(6), 6), ("auto", "auto")):
            del f.launches[:]
            call(alg, reqs[:1], spread=spread)
            assert f.launches == [(("ctx", 0), [6], args, dict(spread=seen))]


@pytest.mark.parametrize("alg", list(ALGS))
def test_a_request_outside_the_domain(monkeypatch, lib, alg):
    a = ALGS[alg]
    f = Fakes(monkeypatch, alg)
    good, outside = a["request"](4, 2, 1), a["outside"]()
    if a["refusal"] is None:   # the single-request solver, on the call's device
        out = call(alg, [good, outside, good], device=DEVICE)
        assert f.singles == [(alg, tuple(outside), dict(shared(alg), device=DEVICE))]
        assert out == [a["answer"](good, True), {"single": 1}, a["answer"](good, True)]
        assert [l[1] for l in f.launches] == [[5, 5]]
    else:                      # there is no other path: the domain's message
        with pytest.raises(ValueError, match="^request 1: " + a["refusal"] + "$"):
            call(alg, [good, outside, good], device=DEVICE)
        assert f.singles == [] and f.launches == [] and f.devices == []
