"""GPU-box HTTP host for the eight solver endpoints.

The reference serves each algorithm as a Vercel function
(api/{tsp,vrp}/{bf,ga,sa,aco}/index.py): parse the body, fetch the location
set and duration matrix from Supabase, run the algorithm (the
`# TODO: Run algorithm` slot), optionally save the solution, respond.  This
module keeps that request/response contract byte for byte -- banners,
preflight headers, error lists, status lines, the save payload -- and fills
the slot with the GPU solver (vrpms_amd.solver).  One process owns one GPU
context per served device; requests are served by a threading HTTP server,
one at a time per device (App.devices; large requests as an island model
across all of them).  Throughput mode across processes: vrpms_amd.frontends.

Storage is pluggable: anything with the three calls of the reference's
Database classes (api/database.py) works.  `MemoryStore` (JSON-backed, the
default and the one the tests use) returns the reference's exact error
messages; a Supabase adapter is sketched in INTEGRATION.md §6.

  python -m vrpms_amd.service --port 8000 --data instances.json

Deliberate differences: a body that is not JSON gets a 400 with
{'what': 'Invalid request'} (the reference's handler raises and drops the
connection), and a solver exception becomes a 400 {'what': 'Solver error'}.
"""
from __future__ import annotations

import argparse
import inspect
import json
import sys
import threading
import time
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

TITLES = {"bf": "Brute Force", "ga": "Genetic Algorithm", "sa": "Simulated Annealing",
          "aco": "Ant Colony Optimization"}
# algorithms of the inline route POST /solve/<problem>/<algo>: the endpoints'
# and the exact solvers, "dp" (Held-Karp) for the TSP and "sp" (set
# partitioning) for the VRP, and "tdp" (time-expanded subset DP, hour-indexed
# matrices) for the TSP and "tdsp" (its fleet counterpart, per-vehicle start
# times) for the VRP, and the local searches "ls" / "lsr" / "lsf" (VRP) and "lso" (TSP)
# (they have no /api endpoint: the eight endpoints are the reference's wire
# contract)
INLINE_ALGORITHMS = {"tsp": tuple(TITLES) + ("dp", "tdp", "lso"),
                     "vrp": tuple(TITLES) + ("ls", "lsr", "lsf", "tdsp", "sp")}

# (body key, params key) in the order the reference checks them
# (api/parameters.py:4-15 and 34-44); 'auth' is the only optional one
_COMMON = {
    "vrp": [("solutionName", "name"), ("auth", "auth"), ("solutionDescription", "description"),
            ("locationsKey", "locations_key"), ("durationsKey", "durations_key"),
            ("capacities", "capacities"), ("startTimes", "start_times"),
            ("ignoredCustomers", "ignored_customers"),
            ("completedCustomers", "completed_customers")],
    "tsp": [("solutionName", "name"), ("auth", "auth"), ("solutionDescription", "description"),
            ("locationsKey", "locations_key"), ("durationsKey", "durations_key"),
            ("customers", "customers"), ("startNode", "start_node"), ("startTime", "start_time")],
}
# search knobs of solver.solve_tsp / solve_vrp that the /solve route accepts
# in its "knobs" object (vrpms_amd.remote forwards them): name -> type
INLINE_KNOBS = {"steps": int, "separators": int, "window": int, "chains": int,
                "window_types": int, "pop": int, "islands": int, "colonies": int, "ants": int,
                "upper_bound": int, "starts": int, "rounds": int, "spread": int,
                "moves": int}
# their accepted ranges (inclusive): a value from the network outside them is a
# 400, never an allocation (islands = 10**6 or chains = 2**30 would
# exhaust device memory while the request holds every device lock)
KNOB_RANGES = {"steps": (1, 10**8), "separators": (0, 4096), "window": (0, 65535),
               "chains": (1, 1 << 16), "window_types": (0, 7), "pop": (2, 4096),
               "islands": (1, 4096), "colonies": (1, 4096), "ants": (1, 4096),
               "upper_bound": (0, 2**31 - 1), "starts": (1, 1024), "rounds": (0, 1000),
               "spread": (1, 1024), "moves": (1, 31)}


def check_knob(name, value):
    """INLINE_KNOBS[name](value), range-checked by KNOB_RANGES (ValueError)."""
    if isinstance(value, bool) or not isinstance(value, (int, float, str)):
        raise ValueError(f"knob {name} must be an integer")
    v = INLINE_KNOBS[name](value)
    lo, hi = KNOB_RANGES[name]
    if not lo <= v <= hi:
        raise ValueError(f"knob {name}={v} outside [{lo}, {hi}]")
    return v


def multi_threaded(value):
    """The VRP GA `multiThreaded` value (api/parameters.py:20 passes the raw
    JSON through): a JSON boolean as is; the strings "true"/"1" and "false"/
    "0" (any case) and the numbers 1 / 0 as those booleans; anything else is
    None -- the size rule decides (bool("false") was True)."""
    if isinstance(value, bool):
        return value
    if isinstance(value, (int, float)) and value in (0, 1):
        return bool(value)
    if isinstance(value, str) and value.strip().lower() in ("true", "1", "false", "0"):
        return value.strip().lower() in ("true", "1")
    return None
# algorithm knobs (api/parameters.py:18-23; every other algorithm takes none)
_KNOBS = {("vrp", "ga"): [("multiThreaded", "multi_threaded"),
                          ("randomPermutationCount", "random_permutationCount"),
                          ("iterationCount", "iteration_count")]}


def get_parameter(name, content, errors, optional=False):
    """api/helpers.py:5-8."""
    if name not in content and not optional:
        errors += [{"what": "Missing parameter", "reason": f"'{name}' was not provided"}]
    return content.get(name)


def parse(problem: str, algorithm: str, content: dict, errors: list):
    """(common params, algorithm params) exactly as parse_common_*_parameters
    and parse_*_<algo>_parameters build them."""
    common = {key: get_parameter(name, content, errors, optional=(name == "auth"))
              for name, key in _COMMON[problem]}
    knobs = {key: get_parameter(name, content, errors)
             for name, key in _KNOBS.get((problem, algorithm), [])}
    return common, knobs


def remove_unused_locations(locations, ignored_customers, completed_customers):
    """api/helpers.py:11-13."""
    disregard = ignored_customers + completed_customers
    return [loc for loc in locations if loc["id"] not in disregard]


# ---------------------------------------------------------------------------
# storage
# ---------------------------------------------------------------------------
_NOT_FOUND = ("Make sure you are accessing public data or data owned by you. "
              "Check if your authentication token has expired.")
_NOT_PERMITTED = {
    "vrp": ("An authentication token is required to save solutions to database. "
            "Please provide 'auth' with a valid JWT token in the request body. "
            "If you have already provided a token, it has very likely expired."),
    "tsp": ("An authentication token is required to save solutions to database."
            " Please provide 'auth' with a valid JWT token in the request body"),
}


class MemoryStore:
    """In-process stand-in for the Supabase tables the handlers use:
    `locations` {id: [location, ...]}, `durations` {id: matrix},
    `users` {token: email}; saved rows are appended to `solutions`."""

    def __init__(self, locations=None, durations=None, users=None):
        self.locations = dict(locations or {})
        self.durations = dict(durations or {})
        self.users = dict(users or {})
        self.solutions = []
        self._lock = threading.Lock()

    @classmethod
    def from_json(cls, path):
        """{"locations": {"1": [...]}, "durations": {"2": [[...]]}, "users": {...}};
        ids are matched as strings or ints."""
        with open(path) as f:
            raw = json.load(f)
        return cls(raw.get("locations"), raw.get("durations"), raw.get("users"))

    def session(self, auth):
        return _Session(self, auth)

    def _get(self, table, key):
        for k in (key, str(key)):
            try:
                if k in table:
                    return table[k]
            except TypeError:       # unhashable id from the request body
                return None
        return None


class _Session:
    """The per-request Database object of api/database.py."""

    def __init__(self, store: MemoryStore, auth):
        self.store = store
        self.email = store.users.get(auth) if isinstance(auth, str) else None

    def get_locations_by_id(self, key, errors):
        rows = self.store._get(self.store.locations, key)
        if rows is None:
            errors += [{"what": "Database read error",
                        "reason": f"No location set found with given id {key}. " + _NOT_FOUND}]
        return rows

    def get_durations_by_id(self, key, errors):
        m = self.store._get(self.store.durations, key)
        if m is None:
            errors += [{"what": "Database read error",
                        "reason": f"No duration matrix found with given id {key}. " + _NOT_FOUND}]
        return m

    def save_solution(self, problem, data: dict, errors):
        """DatabaseVRP/DatabaseTSP.save_solution: owner from the token."""
        if not self.email:
            errors += [{"what": "Not permitted", "reason": _NOT_PERMITTED[problem]}]
            return
        row = {"name": data["name"], "description": data["description"], "owner": self.email}
        row.update({k: v for k, v in data.items() if k not in ("name", "description")})
        with self.store._lock:
            self.store.solutions.append(row)


# ---------------------------------------------------------------------------
# throughput mode: concurrent small TSP requests share one launch
# ---------------------------------------------------------------------------
class TspBatcher:
    """Coalesces concurrent /api/tsp/sa requests on static matrices into one
    `tsp_batch_sa` launch per node count (one workgroup per request, config
    5 of BASELINE.json).  A request waits at most `window_s` for company.
    Requests in one launch share its seed and temperature schedule (scaled
    to the batch's mean edge), so a batched answer depends on the batch it
    rode in; the unbatched path is deterministic per request.  With several
    devices the launches go to them round-robin (SURVEY.md §8e cfg 5:
    replicas only), one launch thread per device, so they run together."""

    MIN_N, MAX_N = 4, 190        # compact nodes; N*N int32 must fit the LDS
    FIELDS = ()                  # per-job fields a launch takes, one list each, after the instances

    def __init__(self, app, window_s: float = 0.005, steps: int = 2000, max_batch: int = 16384,
                 launch=None):
        self.app = app
        self.window_s = window_s
        self.steps = steps
        self.max_batch = max_batch
        self.launches = 0
        self.requests = 0
        self._launch = launch or self._gpu_launch
        self._q = []
        self._cv = threading.Condition()
        self.devices = list(getattr(app, "devices", None) or [getattr(app, "device", 0)])
        self.per_device = {d: 0 for d in self.devices}
        self._rr = 0
        self._pool = None
        if len(self.devices) > 1:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(len(self.devices), thread_name_prefix="tsp-launch")
        threading.Thread(target=self._loop, daemon=True, name="tsp-batcher").start()

    @classmethod
    def accepts(cls, ci) -> bool:
        """Static matrices of MIN_N..MAX_N nodes that also pass the A9 int32
        guard vrpms_set_instance applies on the unbatched path
        ((N + K + 1) * max_duration < 2^31, K = 1, start time 0 here because
        a static tour's duration does not depend on it); anything else takes
        the unbatched path, so both paths share one error contract."""
        if ci.durations.shape[0] != 1 or not cls.MIN_N <= ci.N <= cls.MAX_N:
            return False
        mx = int(ci.durations.max()) if ci.durations.size else 0
        return (ci.N + 2) * mx < 2**31

    @staticmethod
    def group_key(job):
        """What the jobs of one launch share: the node count."""
        return job["ci"].N

    def _wait(self, job):
        """Queue the job and block until its launch finished."""
        with self._cv:
            self._q.append(job)
            self._cv.notify()
        job["done"].wait()
        if "error" in job:
            raise job["error"]

    def solve(self, ci) -> dict:
        """Blocks until the request's launch finished -> the TSP slot dict."""
        job = {"ci": ci, "done": threading.Event()}
        self._wait(job)
        return self._result(job)

    @staticmethod
    def _result(job) -> dict:
        from . import solver
        duration = job.get("duration")
        if duration is None:  # a launch that returns tours only (tests' stand-in launches)
            duration = solver._td_duration(job["ci"], job["tour"])
        return solver.tsp_result(job["ci"], job["tour"], duration)

    def _loop(self):
        while True:
            with self._cv:
                while not self._q:
                    self._cv.wait()
            time.sleep(self.window_s)          # let concurrent requests join
            with self._cv:
                batch, self._q = self._q[:self.max_batch], self._q[self.max_batch:]
            groups = {}
            for job in batch:
                groups.setdefault(self.group_key(job), []).append(job)
            for key, jobs in groups.items():
                dev = self.devices[self._rr % len(self.devices)]
                self._rr += 1
                if self._pool is None:
                    self._run(key, jobs, dev)
                else:
                    self._pool.submit(self._run, key, jobs, dev)

    def _run(self, key, jobs, dev):
        try:
            args = [key, [j["ci"] for j in jobs]] + [[j[f] for j in jobs] for f in self.FIELDS]
            res = self._launch(*args, dev) if len(self.devices) > 1 else self._launch(*args)
            tours, durs = res if isinstance(res, tuple) else (res, None)
            with self._cv:
                self.launches += 1
                self.requests += len(jobs)
                self.per_device[dev] += len(jobs)
            for x, (j, t) in enumerate(zip(jobs, tours)):
                j["tour"] = t
                if durs is not None and durs[x] is not None:
                    j["duration"] = durs[x]
        except Exception as e:         # every waiter of the group sees it
            for j in jobs:
                j["error"] = e
        for j in jobs:
            j["done"].set()

    def _gpu_launch(self, N, cis, device=None):
        """-> (tours, durations) on `device` (default: the app's first): the
        durations are the kernel's keys' primary term (A8: a TSP key is
        duration << 28), exact below the 2^28 - 1 clamp; a clamped one is
        summed on the host."""
        import numpy as np
        import torch
        from . import solver
        # one int32 staging buffer (no per-request stack of int64 copies);
        # the mean edge over the batch from the same buffer
        host = np.empty((len(cis), N, N), dtype=np.int32)
        for x, ci in enumerate(cis):
            host[x] = ci.durations[0]
        nz = host[host > 0]
        edge = float(nz.mean()) if nz.size else 1.0
        inv_t0 = 1.0 / (0.5 * edge)
        inv_alpha = (0.5 / 0.002) ** (1.0 / max(1, self.steps))
        dev = self.devices[0] if device is None else device
        with self.app.locks[dev]:
            ctx = solver.context(dev)
            mats = torch.from_numpy(host).to(ctx.dev)
            tours, keys = ctx.tsp_batch_sa(mats, self.steps, inv_t0, inv_alpha, self.app.seed)
            tours, keys = tours.cpu().tolist(), keys.cpu().tolist()
        clamp = (1 << 28) - 1
        durs = [None if (k >> 28) & clamp == clamp else (k >> 28) & clamp for k in keys]
        return tours, durs


class ExactBatcher(TspBatcher):
    """What the exact batchers share: one launch of solver.BATCH_KINDS[KIND]
    per group key (the kind's, plus the objective where the jobs carry one).
    The queue, the window, the device round-robin and the error fan-out are
    TspBatcher's.  Unlike the SA batcher's, a batched answer does not depend on
    the batch: it is the unbatched answer of the same request."""

    KIND = None

    def __init__(self, app, window_s: float = 0.005, max_batch: int = 16384, launch=None):
        super().__init__(app, window_s, steps=0, max_batch=max_batch, launch=launch)

    @classmethod
    def accepts(cls, ci, bound=None) -> bool:
        """Requests inside the kind's LDS domain (for their bound, where the
        kind has one) that pass the int32 guards vrpms_set_instance applies on
        the unbatched path; anything else takes the unbatched path, so both
        paths share one error contract."""
        from . import solver
        return solver.BATCH_KINDS[cls.KIND].fits(ci, bound) and \
            solver.batch_guard_message(ci) is None

    @classmethod
    def group_key(cls, job):
        from . import solver
        key = solver.BATCH_KINDS[cls.KIND].key(job["ci"])
        return key + (job["objective"],) if "objective" in job else key

    def _solved(self, ci, **fields):
        """Blocks until the request's launch finished -> its slot dict."""
        from . import solver
        job = {"ci": ci, "done": threading.Event(), **fields}
        self._wait(job)
        if ci.problem != solver.TSP:
            return solver.sp_result(ci, list(job["tour"]), job["duration"])
        if "duration" not in job and "bound" in job and not any(job["tour"]) and ci.n > 0:
            raise ValueError(f"no tour within upper_bound = {job['bound']} minutes")
        return self._result(job)

    def _gpu_launch(self, key, cis, *rest):
        """-> (tours, durations) on the device that follows the job fields in
        `rest` (default: the app's first)."""
        from . import solver
        bounds = rest[0] if self.FIELDS else None
        dev = rest[len(self.FIELDS)] if len(rest) > len(self.FIELDS) else self.devices[0]
        objective = key[-1] if cis[0].problem != solver.TSP else "sum"
        with self.app.locks[dev]:
            return solver.BATCH_KINDS[self.KIND].launch(solver.context(dev), cis, bounds, objective)


def _objective(objective):
    return "max" if objective == "max" else "sum"


class ExactTspBatcher(ExactBatcher):
    """("tsp", "dp") on the inline route and ("tsp", "bf") on the endpoint: one
    `tsp_batch_dp` launch per node count (spec A18: each request's Held-Karp
    table in LDS)."""

    KIND = "dp"
    MIN_N, MAX_N = 2, 13         # 1..12 customers (solver.BATCH_DP_MAX_CUSTOMERS)

    @classmethod
    def accepts(cls, ci) -> bool:
        """Static matrices of 1..12 customers that pass the A9 guard (with the
        request's start time, as vrpms_set_instance applies it)."""
        from . import solver
        return ci.durations.shape[0] == 1 and cls.MIN_N <= ci.N <= cls.MAX_N and \
            solver.batch_dp_guard(ci)

    def solve(self, ci) -> dict:
        return self._solved(ci)


class ExactVrpBatcher(ExactBatcher):
    """("vrp", "sp") on the inline route: one `vrp_batch_sp` launch per (node
    count, fleet size, objective) (spec A19: each request's partition DP in
    LDS).  ("vrp", "bf") does not ride it: bf is the optimum over greedy-split
    giant tours, a different and sometimes worse answer."""

    KIND = "sp"

    def solve(self, ci, objective: str = "sum") -> dict:
        return self._solved(ci, objective=_objective(objective))


class ExactTdpBatcher(ExactBatcher):
    """("tsp", "tdp") on the inline route: one `tsp_batch_tdp` launch per (node
    count, hour count) (spec A20: each request's time-expanded table in LDS).
    A job carries its own upper bound, and the launch takes the group's bounds
    next to its instances."""

    KIND = "tdp"
    FIELDS = ("bound",)

    def solve(self, ci, bound) -> dict:
        return self._solved(ci, bound=int(bound))


class ExactTdspBatcher(ExactBatcher):
    """("vrp", "tdsp") on the inline route: one `vrp_batch_tdsp` launch per
    (node count, fleet size, hour count, number of distinct start times,
    objective) (spec A21: each request's time-expanded partition DP in LDS).
    A job carries its own upper bound and objective, and the launch takes the
    group's bounds next to its instances."""

    KIND = "tdsp"
    FIELDS = ("bound",)

    def solve(self, ci, bound, objective: str = "sum") -> dict:
        return self._solved(ci, bound=int(bound), objective=_objective(objective))


class _on_class_or_instance:
    """A method bound to the instance it is looked up on, and to the class
    when looked up there: VrpSaBatcher.accepts(ci) and batcher.accepts(ci)."""

    def __init__(self, fn):
        self.fn = fn

    def __get__(self, obj, cls):
        return self.fn.__get__(cls if obj is None else obj)


class VrpSaBatcher(TspBatcher):
    """Coalesces concurrent /api/vrp/sa and /solve/vrp/sa requests into one
    `vrp_batch_sa` launch per (node count, fleet size, hour count, cell width,
    objective) (spec A22: one workgroup per request, its whole instance in
    LDS, four chains of `steps` steps).  The queue, the window, the device
    round-robin and the error fan-out are TspBatcher's.  Unlike TspBatcher's,
    a batched answer does not depend on the batch: every request runs on its
    own temperature schedule and chain counters, so it is
    solver.solve_vrp_sa_batch([request], steps, the app's seed)'s.  It is not
    the unbatched endpoint's answer (four chains here, 1,024 there).  A launch
    returns (tours, [(veh, durs), ...]): the second list rides TspBatcher's
    per-job duration field.

    It is also all that the batchers of the other VRP heuristics do.  A
    subclass names its ALGORITHM of solver.HEURISTIC_KINDS and the KNOBS its
    launch takes, which begin with the knobs of the kind's domain: those in
    JOB (name -> default) travel with a job and end its group key, the others
    are attributes of the batcher, set by its constructor."""

    ALGORITHM = "sa"
    KNOBS = ("steps",)
    JOB = {}
    spread = None                # the launch's, where the algorithm has a spread form

    def __init__(self, app, window_s: float = 0.005, steps: int = 2000, max_batch: int = 16384,
                 launch=None):
        self._start(app, window_s, max_batch, launch, steps=steps)

    def _start(self, app, window_s, max_batch, launch, **own):
        """What every constructor ends in: the batcher's own knobs become its
        attributes, one that the domain ranges is refused outside that range
        (the launch would refuse it: no clamp), then TspBatcher's start."""
        from . import solver
        ranged = dict(zip(self.KNOBS, solver.HEURISTIC_KINDS[self.ALGORITHM].knobs))
        for name, value in own.items():
            if name in ranged:
                value = solver.check_range(self.ALGORITHM, ranged[name].name, value, name)
            setattr(self, name, value)
        TspBatcher.__init__(self, app, window_s, own.get("steps", 0), max_batch, launch)

    @classmethod
    def _job(cls, given, named) -> dict:
        """A job's knobs: JOB under what a caller gave by position or by name."""
        if len(given) > len(cls.JOB) or not set(named) <= set(cls.JOB):
            raise TypeError(f"{cls.__name__}: a job's knobs are {tuple(cls.JOB)}")
        return {k: int(v) for k, v in {**cls.JOB, **dict(zip(cls.JOB, given)), **named}.items()}

    @_on_class_or_instance
    def _knobs(self, job, count=None) -> tuple:
        """The first `count` (default: all) of KNOBS: the job's, else the batcher's."""
        return tuple(job[k] if k in job else getattr(self, k) for k in self.KNOBS[:count])

    @_on_class_or_instance
    def accepts(self, ci, *knobs, **named) -> bool:
        """Requests inside the algorithm's domain, at the job's knobs and the
        batcher's own (so on the class only where the domain has none of the
        latter), that pass the int32 guards vrpms_set_instance applies on the
        unbatched path.  Anything else takes the unbatched path, so both paths
        share one error contract: a local search's raises the domain's message."""
        from . import solver
        domain = len(solver.HEURISTIC_KINDS[self.ALGORITHM].knobs)
        knobs = self._knobs(self._job(knobs, named), domain)
        return solver._domain_message(self.ALGORITHM, ci, knobs) is None and \
            solver.batch_guard_message(ci) is None

    @classmethod
    def group_key(cls, job):
        """The shape, the objective, then the job's own knobs."""
        from . import solver
        return solver.batch_sa_key(job["ci"]) + (job["objective"],) + tuple(job[k] for k in cls.JOB)

    def solve(self, ci, objective: str = "sum", *knobs, **named) -> dict:
        """Blocks until the request's launch finished -> the VRP slot dict."""
        from . import solver
        job = {"ci": ci, "done": threading.Event(), "objective": _objective(objective),
               **self._job(knobs, named)}
        self._wait(job)
        veh, durs = job["duration"]
        return solver.sa_result(ci, list(job["tour"]), veh, durs)

    def _gpu_launch(self, key, cis, device=None):
        """-> (tours, [(veh, durs), ...]) of the launch solver has under the
        algorithm's name when this runs, on `device` (default: the app's first)."""
        from . import solver
        dev = self.devices[0] if device is None else device
        objective, *job = key[len(key) - len(self.JOB) - 1:]
        with self.app.locks[dev]:
            tours, veh, durs = solver.batch_launch(
                self.ALGORITHM, solver.context(dev), cis, self._knobs(dict(zip(self.JOB, job))),
                self.app.seed, objective, self.spread)
        return tours, list(zip(veh, durs))


class VrpGaBatcher(VrpSaBatcher):
    """Coalesces concurrent /api/vrp/ga and /solve/vrp/ga requests into one
    `vrp_batch_ga` launch per (node count, fleet size, hour count, cell width,
    objective, population, generations) (spec A23: one workgroup per request,
    its whole instance and one population in LDS).  The population and the
    generation count are the request's own randomPermutationCount and
    iterationCount, through solve_vrp's defaults and clamp (solver.ga_knobs).
    The queue, the window, the device round-robin and the error fan-out are
    TspBatcher's.  A batched answer does not depend on the batch: it is
    solver.solve_vrp_ga_batch([request], pop=, gens=, seed=the app's,
    objective=)'s.  It is NOT the unbatched endpoint's answer, which breeds 8
    islands from another start."""

    ALGORITHM = "ga"
    KNOBS = ("pop", "gens", "pmut")
    JOB = {"pop": 256, "gens": 400}     # solve_vrp's defaults (solver.ga_knobs)
    pmut = 0.2                          # solve_vrp_ga_batch's default


class VrpAcoBatcher(VrpSaBatcher):
    """Coalesces concurrent /api/vrp/aco and /solve/vrp/aco requests into one
    `vrp_batch_aco` launch per (node count, fleet size, hour count, cell
    width, objective) (spec A24: one workgroup per request, its whole
    instance and one colony in LDS).  Every launch runs `ants` ants for
    `iters` iterations, the batcher's own (the endpoint has no knob for
    either).  The queue, the window, the device round-robin and the error
    fan-out are TspBatcher's.  A batched answer does not depend on the batch:
    it is solver.solve_vrp_aco_batch([request], ants=, iters=, seed=the
    app's, objective=)'s.  It is NOT the unbatched endpoint's answer, which
    runs 4 colonies."""

    ALGORITHM = "aco"
    KNOBS = ("ants", "iters")

    def __init__(self, app, window_s: float = 0.005, iters: int = 100, ants: int = 64,
                 max_batch: int = 16384, launch=None):
        self._start(app, window_s, max_batch, launch, ants=ants, iters=iters)


class VrpLsBatcher(VrpSaBatcher):
    """Coalesces concurrent /solve/vrp/ls requests into one `vrp_batch_ls`
    launch per (node count, fleet size, hour count, cell width, objective)
    (spec A25: one workgroup per request, its whole instance in LDS, a
    multi-start local search).  Every launch descends from `starts` starts
    for at most `rounds` rounds each, the batcher's own; a request that names
    either inline takes the unbatched path.  The queue, the window, the device
    round-robin and the error fan-out are TspBatcher's.  A batched answer does
    not depend on the batch: it is solver.solve_vrp_ls_batch([request],
    starts=, rounds=, seed=the app's, objective=)'s, which is also the
    unbatched route's at the same knobs and seed."""

    ALGORITHM = "ls"
    KNOBS = ("starts", "rounds")

    def __init__(self, app, window_s: float = 0.005, rounds: int = 1000, starts: int = 64,
                 max_batch: int = 16384, launch=None):
        self._start(app, window_s, max_batch, launch, starts=starts, rounds=rounds)


class VrpLsrBatcher(VrpLsBatcher):
    """Coalesces concurrent /solve/vrp/lsr requests into one `vrp_batch_lsr`
    launch per (node count, fleet size, hour count, cell width, objective)
    (spec A26: VrpLsBatcher's local search on giant tours with route
    separators).  Every launch descends from `starts` starts for at most
    `rounds` rounds each, the batcher's own; a request that names either
    inline takes the unbatched path.  A batched answer does not depend on the
    batch: it is solver.solve_vrp_lsr_batch([request], starts=, rounds=,
    seed=the app's, objective=)'s, which is also the unbatched route's at the
    same knobs and seed.  `spread` (None, "auto" or 1..1024) is
    solver.batch_lsr_launch's: how many workgroups a request's starts are
    spread over, which changes a launch's time and no answer."""

    ALGORITHM = "lsr"

    def __init__(self, app, window_s: float = 0.005, rounds: int = 1000, starts: int = 64,
                 max_batch: int = 16384, launch=None, spread=None):
        from . import solver
        self.spread = solver.check_lsr_spread(spread)
        super().__init__(app, window_s, rounds, starts, max_batch, launch)


class VrpLsfBatcher(VrpLsBatcher):
    """Coalesces concurrent /solve/vrp/lsf requests into one `vrp_batch_lsf`
    launch per (node count, fleet size, cell width, objective) (spec A28:
    VrpLsrBatcher's local search restricted to the plain separator tours of a
    static matrix, priced without walking them).  Every launch descends from
    `starts` starts for at most `rounds` rounds each, the batcher's own; a
    request that names either inline takes the unbatched path, and so does an
    hour-indexed one, which is told there that "lsr" takes it.  A batched
    answer does not depend on the batch: it is
    solver.solve_vrp_lsf_batch([request], starts=, rounds=, seed=the app's,
    objective=)'s, which is also the unbatched route's at the same knobs and
    seed."""

    ALGORITHM = "lsf"


def _coalesce(requests, launches, answer="") -> str:
    """The help of a --batch-vrp-<algorithm> flag."""
    return (f"coalesce concurrent small-fleet VRP {requests} into {launches}{answer}; "
            f"{'it' if answer else 'the answer'} depends on the request alone, not on the batch "
            f"it rode in")


def _coalesce_ls(a, requests, matrix="static or hour-indexed matrix") -> str:
    return _coalesce(f"{requests} (/solve/vrp/{a}, {matrix}, 1..64 vehicles, an instance that fits "
                     f"the LDS)", f"vrp_batch_{a} launches of --batch-{a}-starts starts and at most "
                                  f"--batch-{a}-rounds rounds a descent")


# The batched VRP heuristics of App and main(): algorithm -> (its batcher, {a
# parameter of its constructor: the App keyword that it comes from}, the help
# of its flag).  For each, App also takes batch_vrp_<algorithm> (off by default)
# and batch_vrp_<algorithm>_launch and keeps the batcher, or None, as
# vrp_<algorithm>_batcher; main() has --batch-vrp-<algorithm> and a flag, the
# keyword with dashes, for every knob here that the algorithm's domain ranges.
HEURISTIC_BATCHERS = {
    "sa": (VrpSaBatcher, {"steps": "batch_steps"}, _coalesce(
        "SA requests (/api/vrp/sa and /solve/vrp/sa, static or hour-indexed matrix, 1..64 "
        "vehicles, an instance that fits the LDS)", "vrp_batch_sa launches of --batch-steps steps",
        ": four chains per request, so the answer differs from the unbatched endpoint's")),
    "ga": (VrpGaBatcher, {}, _coalesce(
        "GA requests (/api/vrp/ga and /solve/vrp/ga, static or hour-indexed matrix, 1..64 "
        "vehicles, randomPermutationCount up to 256, iterationCount up to "
        "solver.BATCH_GA_MAX_GENERATIONS, multiThreaded not true, an instance and population "
        "that fit the LDS)", "vrp_batch_ga launches",
        ": one population per request, so the answer differs from the unbatched endpoint's")),
    "aco": (VrpAcoBatcher, {"iters": "batch_aco_iterations", "ants": "batch_aco_ants"}, _coalesce(
        "ACO requests (/api/vrp/aco and /solve/vrp/aco, static or hour-indexed matrix, 1..64 "
        "vehicles, an instance and colony that fit the LDS)",
        "vrp_batch_aco launches of --batch-aco-ants ants and --batch-aco-iterations iterations",
        ": one colony per request, so the answer differs from the unbatched endpoint's")),
    "ls": (VrpLsBatcher, {"starts": "batch_ls_starts", "rounds": "batch_ls_rounds"},
           _coalesce_ls("ls", "local-search requests")),
    "lsr": (VrpLsrBatcher, {"starts": "batch_lsr_starts", "rounds": "batch_lsr_rounds",
                            "spread": "batch_lsr_spread"},
            _coalesce_ls("lsr", "requests of the local search over separator tours")),
    "lsf": (VrpLsfBatcher, {"starts": "batch_lsf_starts", "rounds": "batch_lsf_rounds"},
            _coalesce_ls("lsf", "requests of the local search over plain separator tours",
                         "static matrix")),
}
# what a ranged knob's flag says before the range and the solver constant behind it
_KNOB_HELP = {"iters": "iterations of a {} launch", "ants": "ants of a {} launch",
              "starts": "starts of a {} launch",
              "rounds": "applied moves a descent of a {} launch may take"}


def _heuristic_keywords() -> dict:
    """{App keyword: default} of HEURISTIC_BATCHERS, a knob's default being its
    constructor's."""
    out = {}
    for algorithm, (cls, knobs, _) in HEURISTIC_BATCHERS.items():
        out.update({f"batch_vrp_{algorithm}": False, f"batch_vrp_{algorithm}_launch": None})
        defaults = inspect.signature(cls).parameters
        out.update((keyword, defaults[name].default) for name, keyword in knobs.items())
    return out


# ---------------------------------------------------------------------------
# the endpoint logic
# ---------------------------------------------------------------------------
class App:
    """Parse -> fetch -> solve -> save -> respond for one endpoint call.
    `solve` is injectable (tests); by default it is the GPU solver.

    `devices` (default [device]): the GPUs this process serves.  Each has
    its own context and lock; a request takes the first free device (one
    request per device at a time), and a large SA / GA / ACO request (more
    than `island_min_n` customers) with two or more devices takes them all
    and runs as an island model across them (solver.search_islands).  The
    VRP GA endpoint's `multiThreaded` (api/parameters.py:20, the reference's
    only parallelism knob) decides that for its request instead: true runs
    the island model over every device, false one device.  A device listed
    twice (one GPU standing in for two) is locked once.

    `heuristics`: the keywords of HEURISTIC_BATCHERS -- batch_vrp_<algorithm>,
    batch_vrp_<algorithm>_launch and the batchers' knobs (batch_aco_ants,
    batch_ls_starts, batch_lsr_spread, ...), each at its batcher's default; any
    other keyword is a TypeError."""

    def __init__(self, store, device: int = 0, seed: int = 0, max_seconds: float | None = None,
                 solve=None, batch_tsp: bool = False, batch_window_s: float = 0.005,
                 batch_steps: int = 2000, batch_launch=None, devices=None,
                 island_min_n: int = 150, batch_exact: bool = False, batch_exact_launch=None,
                 batch_exact_vrp_launch=None, batch_exact_tdp_launch=None,
                 batch_exact_tdsp: bool = False, batch_exact_tdsp_launch=None, **heuristics):
        options = dict(_heuristic_keywords(), batch_steps=batch_steps)
        for name in heuristics.keys() - options.keys():
            raise TypeError(f"App.__init__() got an unexpected keyword argument '{name}'")
        options.update(heuristics)
        self.store = store
        self.devices = list(devices) if devices else [device]
        self.device = self.devices[0]
        self.seed = seed
        self.max_seconds = max_seconds
        self.island_min_n = island_min_n
        self.locks = {d: threading.Lock() for d in self.devices}
        self.gpu_lock = self.locks[self.device]
        self._rr = 0
        self._rr_lock = threading.Lock()
        self._solve = solve or self._gpu_solve
        self.batcher = TspBatcher(self, batch_window_s, batch_steps, launch=batch_launch) \
            if batch_tsp else None
        # exact small-TSP requests share tsp_batch_dp launches (off by default)
        self.exact_batcher = ExactTspBatcher(self, batch_window_s, launch=batch_exact_launch) \
            if batch_exact else None
        # and exact small-fleet VRP requests vrp_batch_sp launches
        self.exact_vrp_batcher = ExactVrpBatcher(self, batch_window_s,
                                                 launch=batch_exact_vrp_launch) \
            if batch_exact else None
        # and exact time-dependent small-TSP requests tsp_batch_tdp launches
        self.exact_tdp_batcher = ExactTdpBatcher(self, batch_window_s,
                                                 launch=batch_exact_tdp_launch) \
            if batch_exact else None
        # exact time-dependent small-fleet requests share vrp_batch_tdsp
        # launches: opt-in on its own (batch_exact alone leaves tdsp scheduled)
        self.exact_tdsp_batcher = ExactTdspBatcher(self, batch_window_s,
                                                   launch=batch_exact_tdsp_launch) \
            if batch_exact_tdsp else None
        # small-fleet requests of a VRP heuristic share its vrp_batch_<algorithm>
        # launches (each off by default: for sa, ga and aco the batched answer
        # is not the unbatched endpoint's)
        for algorithm, (cls, knobs, _) in HEURISTIC_BATCHERS.items():
            own = {name: options[keyword] for name, keyword in knobs.items()}
            batcher = cls(self, batch_window_s, launch=options[f"batch_vrp_{algorithm}_launch"],
                          **own) if options[f"batch_vrp_{algorithm}"] else None
            setattr(self, f"vrp_{algorithm}_batcher", batcher)

    def _scheduled(self, problem, algorithm, params, knobs, locations, durations):
        """Run the solve on a device: all of them (in order, as an island
        model) for a large SA / GA / ACO request when there are several, else
        the first free one (round-robin start), waiting for one if all are
        busy."""
        n = len(params.get("customers") or []) if problem == "tsp" else \
            max(0, len(locations or []) - 1)
        from .solver import EXACT_ALGORITHMS
        knobs = dict(knobs)
        mt = multi_threaded(knobs.get("multi_threaded"))
        islands = n > self.island_min_n if mt is None else mt
        if len(self.devices) > 1 and algorithm not in ("bf",) + EXACT_ALGORITHMS and islands:
            held = sorted(set(self.devices))   # each lock once, in one global order
            for d in held:
                self.locks[d].acquire()
            try:
                knobs["devices"] = list(self.devices)
                return self._solve(problem, algorithm, params, knobs, locations, durations)
            finally:
                for d in reversed(held):
                    self.locks[d].release()
        with self._rr_lock:
            start = self._rr
            self._rr = (self._rr + 1) % len(self.devices)
        order = self.devices[start:] + self.devices[:start]
        dev = next((d for d in order if self.locks[d].acquire(blocking=False)), None)
        if dev is None:
            dev = order[0]
            self.locks[dev].acquire()
        try:
            knobs["device"] = dev
            return self._solve(problem, algorithm, params, knobs, locations, durations)
        finally:
            self.locks[dev].release()

    def _batched_tsp(self, params, durations, batcher=None):
        """The compact instance when this request rides `batcher` (default:
        the SA batcher), else None."""
        batcher = self.batcher if batcher is None else batcher
        if batcher is None:
            return None
        from . import solver
        ci = solver.compact_tsp(durations, params["customers"], params["start_node"],
                                params["start_time"] or 0)
        return ci if batcher.accepts(ci) else None

    def _batched_vrp(self, problem, algorithm, params, knobs, locations, durations):
        """A thunk that solves this request on the batcher of its VRP
        heuristic, else None: the algorithm's flag is on, the request names no
        inline knob of its own, its multiThreaded (a ga request's) is not true,
        and its instance -- for ga also its population (at most 256) and
        generations (at most the cap) -- is inside the batcher's domain
        (outside it the unbatched path answers, a local search's with the
        domain's message)."""
        batcher = getattr(self, f"vrp_{algorithm}_batcher") \
            if problem == "vrp" and algorithm in HEURISTIC_BATCHERS else None
        if batcher is None or knobs.get("inline") or \
                multi_threaded(knobs.get("multi_threaded")) is True:
            return None
        from . import solver
        # the only knobs that travel with a request are ga's, under these names
        job = solver.ga_knobs(knobs.get("random_permutationCount"),
                              knobs.get("iteration_count")) if batcher.JOB else ()
        ci = solver.compact_vrp(durations, locations, params["capacities"], params["start_times"],
                                params["ignored_customers"], params["completed_customers"])
        if not batcher.accepts(ci, *job):
            return None
        objective = knobs.get("objective", "sum")
        return lambda: batcher.solve(ci, objective, *job)

    def _exact_batcher(self, problem, algorithm):
        """The exact batcher of an inline (problem, algorithm), or None."""
        return {("tsp", "dp"): self.exact_batcher, ("vrp", "sp"): self.exact_vrp_batcher,
                ("tsp", "tdp"): self.exact_tdp_batcher,
                ("vrp", "tdsp"): self.exact_tdsp_batcher}.get((problem, algorithm))

    def _batched(self, batcher, params, knobs, locations, durations):
        """batcher.solve's arguments when this inline request rides the exact
        `batcher`, else None.  Where the kind has an upper bound, a request
        outside its domain raises here what the unbatched path raises for it."""
        from . import solver
        kind = solver.BATCH_KINDS[batcher.KIND]
        objective = knobs.get("objective", "sum")
        if kind.problem == solver.TSP:
            ci = solver.compact_tsp(durations, params["customers"], params["start_node"],
                                    params["start_time"] or 0)
        else:
            ci = solver.compact_vrp(durations, locations, params["capacities"],
                                    params["start_times"], params["ignored_customers"],
                                    params["completed_customers"])
        args = [ci]
        if batcher.FIELDS:
            args.append(kind.check(ci, solver.OBJ_MAX if objective == "max" else solver.OBJ_SUM,
                                   knobs["inline"].get("upper_bound")))
        if not batcher.accepts(*args):
            return None
        return args if kind.problem == solver.TSP else args + [objective]

    def _gpu_solve(self, problem, algorithm, params, knobs, locations, durations):
        """knobs may carry "seed", "time_limit" and "objective" (the /solve
        route's options, vrpms_amd.remote); the endpoints use the app's."""
        from . import solver
        seed = int(knobs.get("seed", self.seed))
        tl = knobs.get("time_limit", self.max_seconds)
        devs = knobs.get("devices") or [knobs.get("device", self.device)]
        dv = dict(device=devs[0], devices=devs if len(devs) > 1 else None)
        extra = dict(knobs.get("inline") or {})
        if problem == "tsp":
            return solver.solve_tsp(algorithm, durations, params["customers"],
                                    params["start_node"], params["start_time"] or 0,
                                    seed=seed, time_limit=tl, **dv, **extra)
        if knobs.get("random_permutationCount"):
            extra["random_permutation_count"] = int(knobs["random_permutationCount"])
        if knobs.get("iteration_count"):
            extra["iteration_count"] = int(knobs["iteration_count"])
        return solver.solve_vrp(algorithm, durations, locations, params["capacities"],
                                params["start_times"], params["ignored_customers"],
                                params["completed_customers"], seed=seed,
                                objective=knobs.get("objective", "sum"),
                                time_limit=tl, **dv, **extra)

    def post(self, problem: str, algorithm: str, raw: bytes):
        """-> (status, response dict) for a POST body."""
        text = raw.decode("utf-8") if raw else ""
        try:
            content = json.loads(text) if text else dict()
        except ValueError as e:
            return 400, {"success": False,
                         "errors": [{"what": "Invalid request", "reason": str(e)}]}
        if not isinstance(content, dict):
            return 400, {"success": False, "errors": [
                {"what": "Invalid request", "reason": "the body must be a JSON object"}]}
        errors = []
        params, knobs = parse(problem, algorithm, content, errors)
        if errors:
            return 400, {"success": False, "errors": errors}
        db = self.store.session(params["auth"])
        locations = db.get_locations_by_id(params["locations_key"], errors)
        durations = db.get_durations_by_id(params["durations_key"], errors)
        if errors:
            return 400, {"success": False, "errors": errors}
        try:
            batcher = {("tsp", "sa"): self.batcher,
                       ("tsp", "bf"): self.exact_batcher}.get((problem, algorithm))
            ci = self._batched_tsp(params, durations, batcher) if batcher is not None else None
            vrp = self._batched_vrp(problem, algorithm, params, knobs, locations, durations)
            if ci is not None:
                result = batcher.solve(ci)
            elif vrp is not None:
                result = vrp()
            else:
                result = self._scheduled(problem, algorithm, params, knobs, locations, durations)
        except Exception as e:   # bad instance shape, GPU unavailable, ...
            return 400, {"success": False,
                         "errors": [{"what": "Solver error", "reason": str(e)}]}
        if params["auth"]:
            if problem == "vrp":
                data = {"name": params["name"], "description": params["description"],
                        "durationMax": result["durationMax"], "durationSum": result["durationSum"],
                        "locations": remove_unused_locations(locations, params["ignored_customers"],
                                                             params["completed_customers"]),
                        "vehicles": result["vehicles"]}
            else:
                data = {"name": params["name"], "description": params["description"],
                        "duration": result["duration"], "locations": locations,
                        "vehicle": result["vehicle"]}
            db.save_solution(problem, data, errors)
        if errors:
            return 400, {"success": False, "errors": errors}
        return 200, {"success": True, "message": result}


    def solve_inline(self, problem: str, algorithm: str, raw: bytes):
        """POST /solve/{tsp,vrp}/<algo>: the instance inline (no DB) -- what a
        host without a GPU sends to the GPU box (vrpms_amd.remote).  <algo> is
        an endpoint name or, for tsp only, "dp" (exact Held-Karp, up to 24
        customers on a static matrix) or "tdp" (exact time-expanded DP, up to
        solver.TDP_MAX_CUSTOMERS customers, hour-indexed matrices too; knob
        "upper_bound") or "lso" (multi-start local search with Or-opt, spec A27;
        knobs "starts", "rounds", "moves" and "spread": the workgroups the
        starts are spread over, the same body sooner), or, for vrp only, "lsr"
        and "lsf" (multi-start local searches over separator tours, spec A26 and
        A28; knobs "starts", "rounds" and "spread", the latter as for "lso"), "sp" (exact set partitioning, up to solver.SP_MAX_CUSTOMERS customers and 64 vehicles
        on a static matrix) or "tdsp" (exact time-expanded partition DP, up
        to solver.TDSP_MAX_CUSTOMERS customers and 64 vehicles, hour-indexed
        matrices and per-vehicle start times; knob "upper_bound":
        INLINE_ALGORITHMS).  Body: the
        solve_tsp / solve_vrp arguments in the request's camelCase names
        ("durations" is the DB's `matrix` payload); response as the
        handlers': {"success": true, "message": result} or a 400 error list."""
        try:
            content = json.loads(raw.decode("utf-8")) if raw else {}
            if not isinstance(content, dict):
                raise ValueError("the body must be a JSON object")
        except ValueError as e:
            return 400, {"success": False,
                         "errors": [{"what": "Invalid request", "reason": str(e)}]}
        if algorithm not in INLINE_ALGORITHMS.get(problem, ()):
            return 400, {"success": False, "errors": [
                {"what": "Invalid request", "reason": f"no solver /solve/{problem}/{algorithm}"}]}
        names = (["durations", "customers", "startNode", "startTime"] if problem == "tsp" else
                 ["durations", "locations", "capacities", "startTimes", "ignoredCustomers",
                  "completedCustomers"])
        errors = []
        vals = {name: get_parameter(name, content, errors) for name in names}
        if errors:
            return 400, {"success": False, "errors": errors}
        if problem == "tsp":
            params = {"customers": vals["customers"], "start_node": vals["startNode"],
                      "start_time": vals["startTime"]}
            knobs, locations = {}, None
        else:
            params = {"capacities": vals["capacities"], "start_times": vals["startTimes"],
                      "ignored_customers": vals["ignoredCustomers"] or [],
                      "completed_customers": vals["completedCustomers"] or []}
            knobs = {"random_permutationCount": content.get("randomPermutationCount"),
                     "iteration_count": content.get("iterationCount")}
            locations = vals["locations"]
        # the remote front-end's options (vrpms_amd.remote): seed, time limit
        # (capped by the box's own), objective
        try:
            if "seed" in content:
                knobs["seed"] = int(content["seed"])
            if content.get("timeLimit") is not None:
                tl = float(content["timeLimit"])
                knobs["time_limit"] = tl if self.max_seconds is None else min(tl, self.max_seconds)
            if problem == "vrp" and "objective" in content:
                if content["objective"] not in ("sum", "max"):
                    raise ValueError("objective must be 'sum' or 'max'")
                knobs["objective"] = content["objective"]
            inline = content.get("knobs") or {}
            if not isinstance(inline, dict):
                raise ValueError("knobs must be a JSON object")
            bad = sorted(k for k in inline if k not in INLINE_KNOBS)
            if bad:
                raise ValueError(f"unknown knob(s) {bad}; known: {sorted(INLINE_KNOBS)}")
            knobs["inline"] = {k: check_knob(k, v) for k, v in inline.items()}
        except (TypeError, ValueError) as e:
            return 400, {"success": False,
                         "errors": [{"what": "Invalid request", "reason": str(e)}]}
        try:
            batcher = self._exact_batcher(problem, algorithm)
            args = self._batched(batcher, params, knobs, locations, vals["durations"]) \
                if batcher is not None else None
            vrp = self._batched_vrp(problem, algorithm, params, knobs, locations,
                                    vals["durations"])
            if args is not None:
                result = batcher.solve(*args)
            elif vrp is not None:
                result = vrp()
            else:
                result = self._scheduled(problem, algorithm, params, knobs, locations,
                                         vals["durations"])
        except Exception as e:
            return 400, {"success": False,
                         "errors": [{"what": "Solver error", "reason": str(e)}]}
        return 200, {"success": True, "message": result}


def endpoint_handler(app: App, problem: str, algorithm: str):
    """A BaseHTTPRequestHandler class for one endpoint, with the reference's
    GET banner, POST contract and (VRP GA only) preflight response."""
    banner = f"Hi, this is the {problem.upper()} {TITLES[algorithm]} endpoint"

    class Handler(BaseHTTPRequestHandler):
        def log_message(self, *a):
            pass

        def do_GET(self):
            self.send_response(200)
            self.send_header("Content-type", "text/plain")
            self.end_headers()
            self.wfile.write(banner.encode("utf-8"))

        def do_POST(self):
            n = int(self.headers.get("Content-Length", 0))
            status, body = app.post(problem, algorithm, self.rfile.read(n))
            self.send_response(status)
            self.send_header("Content-type", "application/json")
            self.end_headers()
            self.wfile.write(json.dumps(body).encode("utf-8"))

    if (problem, algorithm) == ("vrp", "ga"):
        def do_OPTIONS(self):   # api/vrp/ga/index.py: the header is sent twice there too
            self.send_response(200, "ok")
            self.send_header("Access-Control-Allow-Origin", "*")
            self.send_header("Access-Control-Allow-Methods", "*")
            self.send_header("Access-Control-Allow-Headers", "*")
            self.send_header("Access-Control-Allow-Headers", "*")
            self.end_headers()
        Handler.do_OPTIONS = do_OPTIONS
    return Handler


def router(app: App):
    """One server for every route: /api (api/index.py) and
    /api/{tsp,vrp}/{bf,ga,sa,aco}."""
    routes = {f"/api/{p}/{a}": endpoint_handler(app, p, a)
              for p in ("tsp", "vrp") for a in TITLES}

    class Router(BaseHTTPRequestHandler):
        def log_message(self, *a):
            pass

        def _dispatch(self, method):
            path = self.path.split("?", 1)[0].rstrip("/")
            if path == "/api" and method == "GET":
                self.send_response(200)
                self.send_header("Content-type", "text/plain")
                self.end_headers()
                self.wfile.write(b"Hello!")
                return
            if path.startswith("/solve/") and method == "POST":   # vrpms_amd.remote
                _, _, problem, algorithm = (path.split("/") + ["", ""])[:4]
                n = int(self.headers.get("Content-Length", 0))
                status, body = app.solve_inline(problem, algorithm, self.rfile.read(n))
                self.send_response(status)
                self.send_header("Content-type", "application/json")
                self.end_headers()
                self.wfile.write(json.dumps(body).encode("utf-8"))
                return
            cls = routes.get(path)
            fn = getattr(cls, "do_" + method, None) if cls else None
            if fn is None:
                self.send_error(404 if cls is None else 501)
                return
            fn(self)

        def do_GET(self):
            self._dispatch("GET")

        def do_POST(self):
            self._dispatch("POST")

        def do_OPTIONS(self):
            self._dispatch("OPTIONS")

    return Router


def serve(app: App, host: str = "127.0.0.1", port: int = 8000) -> ThreadingHTTPServer:
    return ThreadingHTTPServer((host, port), router(app))


def _int_in(lo: int, hi: int):
    """An argparse type: an integer in lo..hi (anything else is an error, not a clamp)."""
    def parse(text):
        v = int(text)
        if not lo <= v <= hi:
            raise argparse.ArgumentTypeError(f"must be in {lo}..{hi} ({v} given)")
        return v
    return parse


def _lsr_spread(text):
    """An argparse type: "auto" or an integer in 1..1024 (solver.BATCH_LSR_MAX_SPREAD)."""
    from . import solver
    return text if text == "auto" else _int_in(1, solver.BATCH_LSR_MAX_SPREAD)(text)


def main(argv=None):
    from . import solver
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--data", help="MemoryStore JSON (locations / durations / users)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--devices", default=None,
                    help="comma-separated GPUs to serve (default: --device); large SA / GA / ACO "
                         "requests run as an island model across them")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-seconds", type=float, default=None,
                    help="wall-time cap per solve (default: the algorithm's own budget)")
    ap.add_argument("--batch-tsp", action="store_true",
                    help="coalesce concurrent /api/tsp/sa requests into one launch")
    ap.add_argument("--batch-exact", action="store_true",
                    help="coalesce concurrent exact small-TSP requests (/solve/tsp/dp and "
                         "/api/tsp/bf, static matrix, 1..12 customers) into tsp_batch_dp "
                         "launches, and exact small-fleet VRP requests (/solve/vrp/sp, static "
                         "matrix, 1..12 customers, a fleet that fits the LDS) into vrp_batch_sp "
                         "launches, and exact time-dependent small-TSP requests (/solve/tsp/tdp, "
                         "static or hour-indexed matrix, 1..11 customers, an upper bound whose "
                         "hour words fit the LDS) into tsp_batch_tdp launches; the answers equal "
                         "the unbatched ones")
    ap.add_argument("--batch-exact-tdsp", action="store_true",
                    help="coalesce concurrent exact time-dependent small-fleet requests "
                         "(/solve/vrp/tdsp, static or hour-indexed matrix, 1..11 customers, a "
                         "fleet and an upper bound whose state fits the LDS) into vrp_batch_tdsp "
                         "launches; the answers equal the unbatched ones")
    defaults = _heuristic_keywords()
    for a, (cls, knobs, text) in HEURISTIC_BATCHERS.items():
        ap.add_argument(f"--batch-vrp-{a}", action="store_true", help=text)
        # a flag for every knob of the batcher's that the domain ranges
        ranged = dict(zip(cls.KNOBS, solver.HEURISTIC_KINDS[a].knobs))
        for name, keyword in knobs.items():
            if name in ranged:
                k, (batch, _, word) = ranged[name], keyword.upper().rpartition("_")
                ap.add_argument("--" + keyword.replace("_", "-"), type=_int_in(k.lo, k.hi),
                                default=defaults[keyword],
                                help=f"{_KNOB_HELP[name].format(f'vrp_batch_{a}')}, {k.lo}..{k.hi} "
                                     f"(solver.{batch}_MAX_{word})")
    ap.add_argument("--batch-lsr-spread", type=_lsr_spread, default=None, metavar="{auto,N}",
                    help="spread the starts of every request of a vrp_batch_lsr launch over N "
                         "workgroups, 1..1024 (solver.BATCH_LSR_MAX_SPREAD), or over as many as "
                         "keep the device busy (auto: solver.batch_lsr_spread); the answers are "
                         "the same, a window that caught few requests answers sooner")
    ap.add_argument("--batch-window-ms", type=float, default=5.0)
    ap.add_argument("--batch-steps", type=int, default=2000)
    ap.add_argument("--workers", type=int, default=0,
                    help="throughput mode (BASELINE cfg 5): W front-end processes listen on "
                         "--port together (SO_REUSEPORT) and feed one GPU-owner process per "
                         "device (vrpms_amd.frontends.FrontEndPool); /api/tsp/sa requests are "
                         "batched into tsp_batch_sa launches")
    args = ap.parse_args(argv)
    store = MemoryStore.from_json(args.data) if args.data else MemoryStore()
    devices = [int(x) for x in args.devices.split(",")] if args.devices else None
    if devices:   # a GPU listed twice would only queue behind itself
        devices = list(dict.fromkeys(devices))
    if args.workers > 0:
        from .frontends import FrontEndPool, _default_app
        if devices and len(devices) > 1:
            # each GPU owner holds one device: large requests run on one
            print("vrpms_amd service: --workers serves every device through its own owner "
                  "process; requests are not run as an island model across --devices",
                  file=sys.stderr, flush=True)
        # --batch-tsp is implied (the owners batch /api/tsp/sa); --max-seconds
        # caps every unbatched solve in the owners' App
        pool = FrontEndPool(store, workers=args.workers, devices=devices or [args.device],
                            steps=args.batch_steps, seed=args.seed,
                            window_s=args.batch_window_ms * 1e-3, listen=(args.host, args.port),
                            app_factory=_default_app(store, args.seed, args.batch_steps,
                                                     args.max_seconds))
        print(f"vrpms_amd service ({args.workers} front-end processes) on "
              f"http://{args.host}:{pool.port}/api", flush=True)
        try:
            pool.serve_forever()
        except KeyboardInterrupt:
            pass
        finally:
            pool.close()
        return
    app = App(store, device=args.device, seed=args.seed, max_seconds=args.max_seconds,
              batch_tsp=args.batch_tsp, batch_window_s=args.batch_window_ms * 1e-3,
              devices=devices, batch_exact=args.batch_exact,
              batch_exact_tdsp=args.batch_exact_tdsp,
              **{k: getattr(args, k) for k in _heuristic_keywords() if hasattr(args, k)})
    srv = serve(app, args.host, args.port)
    print(f"vrpms_amd service on http://{args.host}:{args.port}/api", flush=True)
    try:
        srv.serve_forever()
    except KeyboardInterrupt:
        pass
    srv.server_close()


if __name__ == "__main__":
    main()
