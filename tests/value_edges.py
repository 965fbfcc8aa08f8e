"""Instances that sit on the value-range thresholds of the host's layout
choices (vrpms_set_instance in capi.hip, fast_split_params in eval.hip), each
as an inside / outside pair: the last value a layout admits and one past it.

Plain test data, shared by test_value_edges_cpu.py (which proves, with Python
ints and oracle/spec.py alone, that every instance sits where it claims and
that its tours reach the states the edge is about) and test_value_edges_gpu.py
(which scores them on the device).  `model_layout` restates the host
conditions in Python ints; the GPU tests compare it, and each edge's
hand-written `expect`, with vrpms_instance_layout before comparing any cost.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import spec
from vrpms_amd import synth

C_RANDOM = 519          # random tours per batch (not a multiple of any tile)
C_CRAFTED = 256         # crafted tours per batch, half of them "refused at cap + 1"
WAVE = 64               # a premise must hold on at least one wavefront of tours


# ---------------------------------------------------------------------------
# The host conditions, in Python ints
# ---------------------------------------------------------------------------
def bits_for(v: int) -> int:
    b = 1
    while b < 31 and (1 << b) <= v:
        b += 1
    return b


def field_bits(bound: int) -> int:
    """Smallest S in [1, 31] with 2^S > bound (31 when there is none)."""
    s = 1
    while s < 31 and (1 << s) <= bound:
        s += 1
    return s


def stats(inst):
    D = np.asarray(inst.durations)
    cvrp = inst.problem == "cvrp"
    dem = [int(x) for x in inst.demand[1:]] if cvrp and inst.N > 1 else [0]
    cap = [int(x) for x in inst.capacities] if cvrp else [2**31 - 1]
    return dict(max_dur=int(D.max()), max_dem=max(dem) if cvrp else 0,
                min_dem=min(dem) if cvrp else 0, cap0=cap[0], min_cap=min(cap), max_cap=max(cap),
                max_start=max(int(x) for x in inst.start_times))


def accepted(inst) -> bool:
    """The A9 guards of vrpms_set_instance."""
    s = stats(inst)
    if inst.problem == "cvrp" and s["max_cap"] + s["max_dem"] >= 2**31:
        return False
    return s["max_start"] + (inst.N + inst.K + 1) * s["max_dur"] < 2**31


def model_layout(inst, n: int | None = None) -> dict:
    """What vrpms_instance_layout must report (the fields the model covers)."""
    s = stats(inst)
    N, H, K = inst.N, inst.H, inst.K
    n = N - 1 if n is None else n
    cvrp = inst.problem == "cvrp"
    D = np.asarray(inst.durations)
    out = dict(use16=s["max_dur"] <= 65535)
    elem = 2 if out["use16"] else 4
    out["tier"] = 1 if H * N * N * elem <= 64 * 1024 else 2
    out["hour_minor"] = out["use16"] and H == 24
    out["uniform_cap"] = (not cvrp) or len(set(int(c) for c in inst.capacities)) == 1
    out["flex"] = cvrp and s["min_cap"] < s["max_dem"]
    out["symmetric"] = bool((D[0] == D[0].T).all())
    out["sym_all"] = bool((D == D.transpose(0, 2, 1)).all())
    out.update(pack_w=0, pref_S=0, pref_lim=0, fast=False, ks=0, B=0, carry=False)
    if cvrp and H == 1 and N <= 128:
        w = bits_for(s["max_dur"])
        if 2 * w + bits_for(s["max_dem"]) <= 32:
            out["pack_w"], out["tier"] = w, 0
            S = field_bits((N + 1) * s["max_dur"])
            if out["uniform_cap"] and ((s["cap0"] + s["max_dem"] + 1) << S) < 2**32:
                out["pref_S"] = S
                out["pref_lim"] = (s["cap0"] + 1) << S
    if out["pref_S"] and s["max_dem"] <= s["cap0"]:
        ks = field_bits((n + K + 1) * max(s["max_dur"], 1))
        B = 31 - ks
        if B >= 1 and (1 << B) > max(K, n) and \
                ((s["cap0"] + s["max_dem"] + 3) << out["pref_S"]) <= 2**31:
            out.update(fast=True, ks=ks, B=B, carry=s["min_dem"] >= 1)
    return out


# ---------------------------------------------------------------------------
# One edge instance with its tours
# ---------------------------------------------------------------------------
@dataclass
class Edge:
    name: str
    inst: synth.Instance
    P: np.ndarray | None            # [C][ld] tours, `n` tokens used (None: instance is refused)
    n: int
    quantity: int                   # the governing quantity ...
    limit: int                      # ... and the last value its layout admits
    expect: dict                    # layout fields this side must show
    path: int | None = None         # vrpms_eval_path of P
    objective: int = 0
    needs: tuple = ()               # of "close", "refuse", "exhaust", "saturate", "clamp", "unv"
    Psep: np.ndarray | None = None  # tours with A10 separators ...
    n_sep: int = 0                  # ... `n + n_sep` tokens used
    words: bool = True              # also through to_words + eval_words
    refused: bool = False           # vrpms_set_instance must answer VRPMS_ERANGE
    fillers: tuple = field(default_factory=tuple)


def rand_matrix(N, max_dur, rng, sym=True, H=1):
    """Durations in the upper half of [0, max_dur] (routes fill the duration
    field), zero diagonal; customer 1 has both depot legs at max_dur."""
    lo = max_dur // 2
    D = rng.integers(lo, max_dur + 1, size=(H, N, N), dtype=np.int64)
    if sym:
        D = np.triu(D, 1)
        D = D + D.transpose(0, 2, 1)
    D[:, np.arange(N), np.arange(N)] = 0
    D[:, 1, 0] = D[:, 0, 1] = max_dur
    return D


# Large customers lowered to the bottom of their range, per edge: chosen (with
# oracle/spec.py alone, test_value_edges_cpu.py checks the outcome) so that the
# total demand sits where about half of the tours exhaust mixed_fleet's fleet.
TRIM = {"e1_td": 2, "e2_w12": 1, "e2_w14": 2, "e1_cvrp": 7, "e2_w15": 5, "e4": 32, "e7_carry": 31}


def make_demands(N, max_dem, rng, trim=0):
    """demand[0] = 0; customer 1 carries max_dem; the last customers are the
    filler pool 1, 1, 1, 2, 2, 4, 8, ... (every power of two below max_dem),
    which closes any gap below max_dem exactly; the rest are large, `trim` of
    them at the bottom of their range."""
    pool = [1, 1, 1, 2, 2]
    p = 4
    while p < max_dem:
        pool.append(p)
        p *= 2
    pool = [x for x in pool if x <= max_dem]
    nb = N - 1 - len(pool)
    assert nb >= 8, "too few large customers"
    lo = max(1, (3 * max_dem) // 4)
    big = [int(rng.integers(lo, max_dem + 1)) for _ in range(nb)]
    big[0] = max_dem
    big[2:2 + trim] = [lo] * len(big[2:2 + trim])
    dem = np.array([0] + big + pool, dtype=np.int64)
    fillers = tuple(range(1 + nb, N))
    return dem, fillers


def craft_row(row, dem, cap, fillers, one_next, rng):
    """`row` reordered so that its first route ends at load == cap exactly;
    with `one_next` the next customer has demand 1 (refused at cap + 1)."""
    fl = set(fillers)
    route, load = [], 0
    for c in (int(x) for x in row if int(x) not in fl):
        if load + int(dem[c]) > cap:
            break
        route.append(c)
        load += int(dem[c])
    else:
        return None                         # everything large fits: no closure
    used = []
    for f in sorted(fillers, key=lambda f: -int(dem[f])):
        if int(dem[f]) <= cap - load:
            used.append(f)
            load += int(dem[f])
    if load != cap:
        return None
    route += used
    rng.shuffle(route)
    taken = set(route)
    rest = [int(x) for x in row if int(x) not in taken]
    if one_next:
        ones = [c for c in rest if int(dem[c]) == 1]
        if not ones:
            return None
        rest.remove(ones[0])
        rest.insert(0, ones[0])
    return list(route) + rest


def pad4(n):
    return (n + 3) // 4 * 4


def tour_batch(inst, fillers, seed, n_sep=3, crafted=True, dtype=np.uint8):
    """(P, Psep): random permutations plus crafted rows, ld a multiple of 4;
    Psep repeats a stride of them with n_sep separators (token 0) inserted."""
    rng = np.random.default_rng(seed)
    n = inst.n
    C = C_RANDOM + (C_CRAFTED if crafted else 0)
    P = synth.random_perms(C, n, seed=seed, ld=pad4(n), dtype=dtype)
    if crafted:
        cap = int(inst.capacities[0])
        for i in range(C_CRAFTED):
            r = craft_row(P[C_RANDOM + i, :n], inst.demand, cap, fillers, i % 2 == 0, rng)
            if r is not None:
                P[C_RANDOM + i, :n] = r
    Psep = None
    if n_sep:
        rows = P[::2, :n]
        Psep = np.zeros((rows.shape[0], pad4(n + n_sep)), dtype=dtype)
        for i, row in enumerate(rows):
            t = list(row)
            for _ in range(n_sep):
                t.insert(int(rng.integers(0, len(t) + 1)), 0)
            Psep[i, :n + n_sep] = t
    return P, Psep


def tour_facts(inst, row):
    """What one tour does under the greedy split (oracle/spec.py, Python
    ints): closes a route at load == cap with a token after it, refuses a
    customer at load + dem == cap + 1, runs out of vehicles, its longest
    route, and its durationSum / durationMax / unvisited."""
    r = spec.eval_cvrp(inst.durations, row, inst.demand, inst.capacities, inst.start_times)
    dem, cap = inst.demand, inst.capacities
    load = [sum(int(dem[c]) for c in rt) for rt in r["routes"]]
    close = refuse = False
    last = -1                               # vehicle of the previous customer token
    for i, c in enumerate(int(x) for x in row):
        v = r["vehicle_of"][i]
        if c == 0:
            last = -1                       # closed by the separator, not by a refusal
            continue
        if last >= 0 and v != last:         # c did not join vehicle `last`
            # load[last] is final here: the route closed when c was refused
            close |= load[last] == int(cap[last])
            refuse |= load[last] + int(dem[c]) == int(cap[last]) + 1
        last = v if v >= 0 else last
        if v == -1:
            break
    return dict(close=close, refuse=refuse, exhaust=r["unvisited"] > 0,
                longest=max(r["durations"]), sum=r["sum"], max=r["max"], unv=r["unvisited"])


def cvrp_inst(name, D, dem, cap, K, start=0):
    caps = np.full(K, cap, dtype=np.int64) if np.isscalar(cap) else np.asarray(cap, dtype=np.int64)
    st = np.full(K, start, dtype=np.int64) if np.isscalar(start) else np.asarray(start, dtype=np.int64)
    return synth.Instance(name, D, dem, caps, st, "cvrp")


def fleet_for(dem, cap, extra=0):
    """Vehicles that the demands need at the least (plus `extra`)."""
    return max(1, -(-int(dem.sum()) // int(cap)) + extra)


def mixed_fleet(inst, P):
    """`inst` with as many vehicles as the median tour of P uses when it has
    vehicles to spare: about half of the tours then exhaust the fleet and
    half do not, so both outcomes share wavefronts."""
    cap, st = int(inst.capacities[0]), int(inst.start_times[0])
    spare = cvrp_inst(inst.name, inst.durations, inst.demand, cap, inst.n, st)
    used = [sum(1 for rt in spec.eval_cvrp(spare.durations, row[:inst.n], spare.demand,
                                           spare.capacities, spare.start_times)["routes"] if rt)
            for row in P]
    return cvrp_inst(inst.name, inst.durations, inst.demand, cap, int(np.median(used)), st)


# ---------------------------------------------------------------------------
# E1: uint16 matrix, max_dur 65535 | 65536
# ---------------------------------------------------------------------------
def _e1(kind):
    out = []
    for side, md in (("in", 65535), ("out", 65536)):
        rng = np.random.default_rng(101)
        u16 = md <= 65535
        if kind == "tsp":               # eval_tsp_staged<u16 | i32>
            D = rand_matrix(40, md, rng)
            inst = synth.Instance("e1_tsp", D, None, None, np.array([7]), "tsp")
            P = synth.random_perms(C_RANDOM, inst.n, seed=11, ld=pad4(inst.n))
            out.append(Edge(f"e1_tsp_{side}", inst, P, inst.n, md, 65535,
                            dict(use16=u16, tier=1), path=1, words=False))
            continue
        H, N = (24, 20) if kind == "td" else (1, 48)
        D = rand_matrix(N, md, rng, H=H)
        dem, fl = make_demands(N, 15, rng, TRIM.get(f"e1_{kind}", 0))
        inst = cvrp_inst(f"e1_{kind}", D, dem, 40, fleet_for(dem, 40, 1), start=415)
        P, Psep = tour_batch(inst, fl, seed=12)
        inst = mixed_fleet(inst, P)
        out.append(Edge(f"e1_{kind}_{side}", inst, P, inst.n, md, 65535,
                        dict(use16=u16, pack_w=0, hour_minor=u16 and H == 24), path=2,
                        needs=("close", "refuse", "exhaust"), Psep=Psep, n_sep=3, fillers=fl))
    return tuple(out)


# ---------------------------------------------------------------------------
# E2: pack64 field widths, 2w + bits(max_dem) = 32 | 33
# ---------------------------------------------------------------------------
E2_SPLITS = ((15, 3), (14, 15), (12, 255), (8, 65535), (1, 2**30 - 1))


def _e2(w, max_dem):
    out = []
    bits = bits_for(max_dem)
    assert max_dem == (1 << bits) - 1 and 2 * w + bits == 32
    for side in ("in", "out"):
        rng = np.random.default_rng(200 + w)
        N = 64
        D = rand_matrix(N, (1 << w) - 1, rng)
        dem, fl = make_demands(N, max_dem, rng, TRIM.get(f"e2_w{w}", 0))
        # capacity + demand must stay below 2^31: at w = 1 the capacity lies in [max_dem, 2^30]
        cap = max_dem if w == 1 else (5 * max_dem) // 2
        if side == "out":
            dem[2] = 1 << bits              # one bit more than the demand field holds
        inst = cvrp_inst(f"e2_w{w}", D, dem, cap, fleet_for(dem, cap))
        P, Psep = tour_batch(inst, fl, seed=20 + w)
        inst = mixed_fleet(inst, P)
        q = 2 * bits_for(int(D.max())) + bits_for(int(dem.max()))
        exp = dict(use16=True, pack_w=w, tier=0) if side == "in" else dict(pack_w=0, pref_S=0, tier=1)
        out.append(Edge(f"e2_w{w}_{side}", inst, P, inst.n, q, 32, exp, path=0 if side == "in" else 2,
                        needs=("close", "refuse", "exhaust"), Psep=Psep, n_sep=3, fillers=fl))
    return tuple(out)


# ---------------------------------------------------------------------------
# E3 / E4 / E7: the load field above S = 19, N = 100 (E3: 116), max_dur 4095, max_dem 255
# ---------------------------------------------------------------------------
def _load_field(name, cap, exp, q, limit, sym=True, zeros=False, seed=300, objective=0, N=100):
    rng = np.random.default_rng(seed)
    D = rand_matrix(N, 4095, rng, sym=sym)
    if not sym:
        D[0, 2:, 0] = rng.integers(3000, 4096, size=N - 2)     # expensive returns
    dem, fl = make_demands(N, 255, rng, TRIM.get(name if name.startswith("e7") else name.split("_")[0], 0))
    if zeros:
        dem[3:16:4] = 0
    inst = cvrp_inst(name, D, dem, cap, fleet_for(dem, cap))
    P, Psep = tour_batch(inst, fl, seed=seed + 1)
    inst = mixed_fleet(inst, P)
    assert field_bits((N + 1) * 4095) == 19
    return Edge(name, inst, P, inst.n, q(cap), limit, exp, path=0, objective=objective,
                needs=("close", "refuse", "exhaust"), Psep=Psep, n_sep=3, fillers=fl)


def _e3():
    q = lambda cap: (cap + 255 + 1) << 19       # noqa: E731
    return (_load_field("e3_in", 7935, dict(pack_w=12, pref_S=19, pref_lim=7936 << 19, fast=False),
                        q, 2**32 - 2**19, N=116),
            _load_field("e3_out", 7936, dict(pack_w=12, pref_S=0, fast=False), q, 2**32 - 2**19,
                        N=116))


def _e4(objective=0):
    q = lambda cap: (cap + 255 + 3) << 19       # noqa: E731
    return (_load_field("e4_in", 3838, dict(pack_w=12, pref_S=19, fast=True, carry=True), q, 2**31,
                        objective=objective),
            _load_field("e4_out", 3839, dict(pack_w=12, pref_S=19, pref_lim=3840 << 19, fast=False),
                        q, 2**31, objective=objective))


def _e7():
    """E4 inside on an asymmetric matrix: every demand >= 1 (the fit test is
    the add's carry) | some demands 0 (the sign-compare form)."""
    q = lambda cap: (cap + 255 + 3) << 19       # noqa: E731
    return (_load_field("e7_carry", 3838, dict(fast=True, carry=True, symmetric=False), q, 2**31,
                        sym=False, seed=700),
            _load_field("e7_zero_dem", 3838, dict(fast=True, carry=False, symmetric=False), q,
                        2**31, sym=False, zeros=True, seed=700))


# ---------------------------------------------------------------------------
# E5: the duration field S, one route that fills it
# ---------------------------------------------------------------------------
def _e5(asym):
    out = []
    N, S = 64, 19
    md0 = ((1 << S) - 1) // (N + 1)
    for side, md in (("in", md0), ("out", md0 + 1)):
        rng = np.random.default_rng(500)
        D = np.full((1, N, N), md, dtype=np.int64)
        D[0, np.arange(N), np.arange(N)] = 0
        if asym:
            # ret(a) = md for odd a, ret(b) = 0 for even b, dur(a, b) = 0 between
            # them: the edge term dur + ret(b) - ret(a) reaches -md
            odd, even = np.arange(1, N, 2), np.arange(2, N, 2)
            D[0, even, 0] = 0
            D[0][np.ix_(odd, even)] = 0
        dem = np.array([0] + [1] * (N - 1), dtype=np.int64)
        inst = cvrp_inst("e5_asym" if asym else "e5", D, dem, N - 1, 2)
        P, Psep = tour_batch(inst, (), seed=51, crafted=False)
        out.append(Edge(f"{inst.name}_{side}", inst, P, inst.n, md, md0,
                        dict(pref_S=S if side == "in" else S + 1, fast=True, symmetric=not asym),
                        path=0, needs=("saturate",) if side == "in" and not asym else (),
                        Psep=Psep, n_sep=3))
    return tuple(out)


# ---------------------------------------------------------------------------
# E6: the vehicle counter above ks, 2^B = max(K, n) + 1
# ---------------------------------------------------------------------------
def _e6_fleet():
    """K decides: N = 100, max_dur 23000 (ks = 23 on both sides), K = 255
    (2^8 = K + 1) | 256.  With 99 tokens no tour can close 255 routes, so
    the counter starts at 2^B - K = 1 and never reaches the exhausted bit.
    (N = 100 and not 128: the row tile must fit the LDS next to the matrix.)"""
    out = []
    for side, K in (("in", 255), ("out", 256)):
        rng = np.random.default_rng(600)
        N = 100
        D = rand_matrix(N, 23000, rng)
        dem = np.array([0] + [int(rng.integers(2, 4)) for _ in range(N - 1)], dtype=np.int64)
        dem[-5:] = [1, 1, 1, 2, 2]
        inst = cvrp_inst("e6_fleet", D, dem, 3, K)      # a route holds one or two customers
        P, _ = tour_batch(inst, tuple(range(N - 5, N)), seed=61, n_sep=0)
        assert field_bits((inst.n + K + 1) * 23000) == 23
        exp = dict(pack_w=15, fast=True, ks=23, B=8) if side == "in" else \
            dict(pack_w=15, pref_S=22, fast=False)
        out.append(Edge(f"e6_fleet_{side}", inst, P, inst.n, max(K, inst.n) + 1, 1 << 8, exp, path=0,
                        needs=("close", "refuse"), fillers=tuple(range(N - 5, N))))
    return tuple(out)


def _e6_tokens():
    """n decides: tours of 255 tokens (127 customers, 128 separators) | 256,
    K = 120, through the word layout; most tours exhaust the fleet and then
    count every later customer in the same field."""
    out = []
    for side, n_sep in (("in", 128), ("out", 129)):
        rng = np.random.default_rng(650)
        N, K = 128, 120
        D = rand_matrix(N, 20000, rng)
        dem = np.array([0] + [int(rng.integers(1, 4)) for _ in range(N - 1)], dtype=np.int64)
        inst = cvrp_inst("e6_tokens", D, dem, 3, K)
        n = inst.n + n_sep
        C = C_RANDOM
        P = np.zeros((C, pad4(n)), dtype=np.uint8)
        for i in range(C):
            t = np.concatenate([np.arange(1, N), np.zeros(n_sep, dtype=np.int64)])
            # a share keeps the separators apart from the customers: fewer empty routes
            P[i, :n] = rng.permutation(t) if i % 3 else np.concatenate(
                [rng.permutation(np.arange(1, N)), np.zeros(n_sep, dtype=np.int64)])
        assert field_bits((n + K + 1) * 20000) == 23
        exp = dict(fast=True, ks=23, B=8) if side == "in" else dict(pref_S=22, fast=False)
        out.append(Edge(f"e6_tokens_{side}", inst, None, n, max(K, n) + 1, 1 << 8, exp,
                        needs=("exhaust",), Psep=P, n_sep=0))
    return tuple(out)


# ---------------------------------------------------------------------------
# E8: the A9 int32 guards, largest accepted | refused
# ---------------------------------------------------------------------------
def _e8_time():
    out = []
    N, K, md = 12, 3, 2**27 - 1                 # (N + K + 1) * md = 2^31 - 16
    for side, start in (("in", 15), ("out", 16)):
        rng = np.random.default_rng(800)
        D = rand_matrix(N, md, rng)
        dem = np.array([0] + [int(rng.integers(1, 4)) for _ in range(N - 1)], dtype=np.int64)
        inst = cvrp_inst("e8_time", D, dem, 9, K, start=start)
        P = synth.random_perms(C_RANDOM, inst.n, seed=81, ld=pad4(inst.n))
        out.append(Edge(f"e8_time_{side}", inst, P if side == "in" else None, inst.n,
                        start + (N + K + 1) * md, 2**31 - 1, dict(use16=False, pack_w=0), path=2,
                        needs=("clamp",), refused=side == "out"))
    return tuple(out)


def _e8_cap():
    out = []
    md = 2**30 - 1
    for side, cap in (("in", 2**30), ("out", 2**30 + 1)):
        rng = np.random.default_rng(810)
        N = 64
        D = rand_matrix(N, 1000, rng)
        dem, fl = make_demands(N, md, rng, TRIM.get("e8_cap", 0))
        inst = cvrp_inst("e8_cap", D, dem, cap, fleet_for(dem, cap))
        P, Psep = tour_batch(inst, fl, seed=82)
        inst = mixed_fleet(inst, P)
        out.append(Edge(f"e8_cap_{side}", inst, P if side == "in" else None, inst.n, cap + md,
                        2**31 - 1, dict(pack_w=0, uniform_cap=True, flex=False), path=2,
                        needs=("close", "refuse", "exhaust"), Psep=Psep if side == "in" else None,
                        n_sep=3, refused=side == "out", fillers=fl))
    return tuple(out)


def _e8_het():
    """One vehicle at the capacity limit, one tiny: eval_cvrp_packed MODE 0."""
    out = []
    for side, big in (("in", 2**31 - 1 - 255), ("out", 2**31 - 255)):
        rng = np.random.default_rng(820)
        N = 64
        D = rand_matrix(N, 4095, rng)
        dem, fl = make_demands(N, 255, rng)
        caps = [1, 600, big, 3, 600]
        inst = cvrp_inst("e8_het", D, dem, caps, len(caps), start=[0, 5, 0, 9, 2])
        P, Psep = tour_batch(inst, fl, seed=83, crafted=False)
        out.append(Edge(f"e8_het_{side}", inst, P if side == "in" else None, inst.n, big + 255,
                        2**31 - 1, dict(pack_w=12, pref_S=0, uniform_cap=False, flex=True), path=0,
                        Psep=Psep if side == "in" else None, n_sep=3, refused=side == "out"))
    return tuple(out)


def _e8_hour():
    """H = 24 with the start time at the limit: hour indices near 2^31 / 60."""
    out = []
    N, K, md = 12, 3, 100
    for side, start in (("in", 2**31 - 1 - (N + K + 1) * md), ("out", 2**31 - (N + K + 1) * md)):
        rng = np.random.default_rng(830)
        D = rand_matrix(N, md, rng, H=24)
        dem = np.array([0] + [int(rng.integers(1, 4)) for _ in range(N - 1)], dtype=np.int64)
        inst = cvrp_inst("e8_hour", D, dem, 9, K, start=[start, start - 61, start - 3000])
        P = synth.random_perms(C_RANDOM, inst.n, seed=84, ld=pad4(inst.n))
        out.append(Edge(f"e8_hour_{side}", inst, P if side == "in" else None, inst.n,
                        start + (N + K + 1) * md, 2**31 - 1, dict(use16=True, hour_minor=True),
                        path=2, refused=side == "out"))
    return tuple(out)


# ---------------------------------------------------------------------------
# E9: the key's unvisited field holds 255, d_unv the true count
# ---------------------------------------------------------------------------
def _e9():
    out = []
    rng = np.random.default_rng(900)
    N = 300
    D = rand_matrix(N, 900, rng)
    dem = np.array([0] + [1] * (N - 1), dtype=np.int64)
    inst = cvrp_inst("e9", D, dem, 1, 1)
    P = synth.random_perms(C_RANDOM, inst.n, seed=91, dtype=np.uint16)
    for side, n in (("in", 256), ("out", 257)):     # one visited, n - 1 unvisited
        out.append(Edge(f"e9_{side}", inst, P, n, n - 1, 255, dict(pack_w=0, tier=2), path=2,
                        needs=("unv",), words=False))
    return tuple(out)


BUILDERS = {"e1_tsp": lambda: _e1("tsp"), "e1_cvrp": lambda: _e1("cvrp"), "e1_td": lambda: _e1("td"),
            **{f"e2_w{w}": functools.partial(_e2, w, d) for w, d in E2_SPLITS},
            "e3": _e3, "e4": _e4, "e4_max": lambda: _e4(1), "e5": lambda: _e5(False),
            "e5_asym": lambda: _e5(True), "e6_fleet": _e6_fleet, "e6_tokens": _e6_tokens,
            "e7": _e7, "e8_time": _e8_time, "e8_cap": _e8_cap, "e8_het": _e8_het,
            "e8_hour": _e8_hour, "e9": _e9}


@functools.lru_cache(maxsize=None)
def pair(name):
    """(inside, outside) of one edge; built once per session."""
    return BUILDERS[name]()


SIDES = [(name, side) for name in BUILDERS for side in (0, 1)]
SIDE_IDS = [f"{name}-{'in' if side == 0 else 'out'}" for name, side in SIDES]


# ---------------------------------------------------------------------------
# Small cases for the search kernels: n = 12, max_dur 15 (S = 8), max_dem
# 2^22 - 1, so the load field still reaches its limit
# ---------------------------------------------------------------------------
def small(kind):
    md = 2**22 - 2
    cap = {"e4_in": 2**23 - 3 - md, "e4_out": 2**23 - 2 - md, "e3_in": 2**24 - 2 - md}[kind]
    rng = np.random.default_rng(40)
    N = 13
    D = rand_matrix(N, 15, rng, sym=False)
    dem = np.array([0] + [int(rng.integers(2**21, md)) for _ in range(N - 1)], dtype=np.int64)
    dem[1] = md                         # with customer 5 it fills an e4 vehicle (cap = md + 1)
    dem[2] = 2**21 + 5
    dem[3] = 2**22 - 1 - dem[2]         # 2 and 3 fill one too
    dem[5:7] = 1                        # ... and one of these is then refused at cap + 1
    K = fleet_for(dem, cap)
    return cvrp_inst(f"small_{kind}", D, dem, cap, K)
