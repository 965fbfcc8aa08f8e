"""The TSP local search with Or-opt and delta pricing (spec A27) by its second
mapping: the C entry points vrpms_tsp_batch_lso_spread_lds /
vrpms_tsp_batch_lso_spread_work / vrpms_tsp_batch_lso_spread,
Context.tsp_batch_lso_spread, solver.batch_lso_spread and the `spread` argument
of batch_lso_launch / solve_tsp_lso_batch / solve_tsp("lso"), and the inline
knob "spread" on /solve/tsp/lso.

The mapping is free under A27, so there is no new reference: per request the
GPU must return the identical key, tour, duration and info row as
tests/test_tsp_batch_lso.py's a27_ref, and as tsp_batch_lso itself, for every
number of workgroups per request."""
import ctypes
import functools
import json
import threading
import urllib.request

import numpy as np
import pytest

from oracle import spec
from test_tsp_batch_lso import (ALL_RUNS, DOMAIN, E65535, E65536, GRID_N, HUGE, LDS_BYTES, LONG, MASKS,
                                R_EDGES, S_EDGES, SEED, SIX, _tsp_body, all_moves, by_launch, expected,
                                inst, lds_bytes, move_sources, pad, reference, request, run_id, shuffled)
from test_vrp_batch_ga import _no_gpu
from vrpms_amd import _lib, core, service, solver

# the runs this file adds: (case, S, rounds, moves).  Under the 256-thread share
# a round's enabled moves are numbered in (typ, i, j) order and thread t takes
# the ids [t per, (t + 1) per), per = ceil(moves / 256); wavefront t // 64
IDLE = ((9, 1, 70, ""), 6, 1000, 31)         # 242 moves, per = 1, 14 idle threads
PER2 = ((10, 24, 71, ""), 6, 1000, 31)       # 308 moves, the first per = 2, 102 idle threads
PER4 = ((16, 1, 72, ""), 4, 1000, 31)        # 872 moves, per = 4
TIES_A = ((9, 1, 5, "ties"), 8, 1000, 31)    # equal least keys in different wavefronts' shares
TIES_B = ((10, 24, 6, "ties"), 8, 1000, 31)
# no (n <= 120, mask) has a type boundary inside a thread's share AND one
# between two wavefronts, so there is a case of each:
MASK_IN = ((10, 1, 73, ""), 6, 1000, 29)       # 263 moves, per = 2; the types end at 45, 135, 207: all odd
MASK_BETWEEN = ((9, 24, 74, ""), 6, 1000, 28)  # 170 moves, per = 1; relocate ends at 72, Or-opt 2 at 128
NEW_RUNS = [IDLE, PER2, PER4, TIES_A, TIES_B, MASK_IN, MASK_BETWEEN]
# all 31 masks at n = 7 on the clock (the parent's MASKS have n = 7 at H = 1 only)
MASKS_24 = [((7, 24, 23, ""), 4, 1000, mask) for mask in range(1, 32)]
# S and G of the group edges.  The parent's S_EDGES instance is won by start 0
# at every S; the seeds 305 and 307 were searched with a27_ref so that the last
# start wins: at G >= S it is the last workgroup's only start
GROUP_G = (1, 2, 4, 5, 9, 64)
GROUP_RUNS = [r for r in S_EDGES if r[1] in (1, 5, 9)] + \
    [((9, 24, 305, ""), 5, 1000, 31), ((9, 24, 307, ""), 9, 1000, 31)]


def spread_lds_bytes(N, H, wide):
    """DESIGN.md §4.3t restated: the matrix padded to 16 bytes; per wavefront
    two int32 rows of n + 2 words padded to four (one on an hour-indexed
    matrix) and a uint16 tour of n + 2 genes padded to eight; and two sets of
    four 16-byte round records."""
    n = N - 1
    return pad(H * N * N * (4 if wide else 2), 16) + \
        4 * ((2 if H == 1 else 1) * 4 * pad(n + 2, 4) + 2 * pad(n + 2, 8)) + 2 * 4 * 16


def work_bytes(R, N, G):
    return R * G * (24 + 2 * pad(N - 1, 8))


def largest_spread_nodes(H, wide):
    return max(N for N in range(2, 400) if spread_lds_bytes(N, H, wide) <= LDS_BYTES)


@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_lds_is_at_most_tsp_batch_lso_s(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_tsp_batch_lso_spread_lds
    for H in (1, 24):
        for wide in (0, 1):
            for N in GRID_N:
                assert f(N, H, wide, ctypes.byref(b)) == _lib.VRPMS_OK
                assert b.value == spread_lds_bytes(N, H, wide) == core.tsp_batch_lso_spread_lds(N, H, wide)
                assert b.value <= core.tsp_batch_lso_lds(N, H, wide) == lds_bytes(N, H, wide)
                # the difference is the four best tours less four records
                assert lds_bytes(N, H, wide) - b.value == 4 * 2 * pad(N - 1, 8) - 64
            # up to eight customers a best tour is one record long: the two meet
            for N in range(2, 10):
                assert spread_lds_bytes(N, H, wide) == lds_bytes(N, H, wide)
            assert spread_lds_bytes(10, H, wide) < lds_bytes(10, H, wide)
    # at A27's own edges, and the new formula's
    for (H, wide), N in DOMAIN.items():
        assert core.tsp_batch_lso_spread_lds(N, H, wide) <= core.tsp_batch_lso_lds(N, H, wide) <= LDS_BYTES
        top = largest_spread_nodes(H, wide)
        assert N <= top and core.tsp_batch_lso_spread_lds(top, H, wide) <= LDS_BYTES < \
            core.tsp_batch_lso_spread_lds(top + 1, H, wide)
    # the same refusals, the same codes
    for args, word in (((1, 1, 0), b"2 <= N"), ((0, 1, 0), b"2 <= N"), ((65536, 1, 0), b"2 <= N"),
                       ((5, 2, 0), b"H must be 1 or 24"), ((5, 0, 0), b"H must be 1 or 24"),
                       ((5, 1, 2), b"wide"), ((5, 1, -1), b"wide")):
        b.value = 77
        assert lib.vrpms_tsp_batch_lso_lds(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL
        assert word in lib.vrpms_last_error()
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_tsp_batch_lso_spread_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(65535, 1, 0, ctypes.byref(b)) == _lib.VRPMS_OK
    assert f(5, 1, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_tsp_batch_lso_spread_lds: bytes is NULL" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="H must be 1 or 24"):
        core.tsp_batch_lso_spread_lds(5, 3, False)


def test_workspace_bytes(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_tsp_batch_lso_spread_work
    for R in (0, 1, 3, 10000):
        for N in (2, 5, 8, 9, 10, 17, 58, 274):
            for G in (1, 2, 64, 1024, 65535):
                assert f(R, N, G, ctypes.byref(b)) == _lib.VRPMS_OK
                assert b.value == work_bytes(R, N, G) == core.tsp_batch_lso_spread_work(R, N, G)
                assert b.value % 8 == 0
    assert work_bytes(1, 9, 1) == 24 + 2 * 8 and work_bytes(1, 10, 1) == 24 + 2 * 16
    assert f(32767, 65535, 65535, ctypes.byref(b)) == _lib.VRPMS_OK
    assert b.value == 32767 * 65535 * (24 + 2 * 65536)
    for args, word in (((-1, 5, 1), b"R must not be negative"), ((1, 1, 1), b"2 <= N"),
                       ((1, 65536, 1), b"2 <= N"),
                       ((1, 5, 0), b"1 <= G <= 65535 (0 given)"),
                       ((1, 5, 65536), b"1 <= G <= 65535 (65536 given)"),
                       ((1, 5, -1), b"1 <= G <= 65535 (-1 given)"),
                       ((32769, 5, 65535), b"R * G = %d records are above 2^31 - 1" % (32769 * 65535))):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_tsp_batch_lso_spread_work" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(1, 5, 1, None) == _lib.VRPMS_EINVAL
    assert b"bytes is NULL" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= G <= 65535"):
        core.tsp_batch_lso_spread_work(1, 5, 0)


def test_argument_errors_need_no_gpu(lib):
    """As tests/test_tsp_batch_lso.py's: every argument check comes before the
    context is looked at, so a block of zeros serves as the non-NULL ctx; its
    LDS size of zero makes every launch that passes the other checks an LDS
    refusal."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 16)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    assert p % 8 == 0
    names = ("m", "st", "t", "k", "du", "i")

    def f(ctx=c, R=1, N=5, H=1, wide=0, S=8, rounds=3, moves=31, G=2, work=p, wb=1 << 16, **ptrs):
        a = {name: ptrs.get(name, p) for name in names}
        return lib.vrpms_tsp_batch_lso_spread(ctx, a["m"], a["st"], R, N, H, wide, S, rounds, moves,
                                              12345, G, work, wb, a["t"], a["k"], a["du"], a["i"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_tsp_batch_lso_spread:" in msg and word in msg, (kw, msg)

    # the existing entry point's
    refused(b"ctx is NULL", ctx=None)
    refused(b"R must not be negative", R=-1)
    for N in (-1, 0, 1, 65536):
        refused(b"2 <= N <= 65535 (%d given)" % N, N=N)
    for H in (0, 2, 12, 25):
        refused(b"H must be 1 or 24 (%d given)" % H, H=H)
    for wide in (-1, 2):
        refused(b"(%d given)" % wide, wide=wide)
        refused(b"wide", wide=wide)
    for S in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= S <= 65535 (%d given)" % S, S=S)
    refused(b"rounds must not be negative (-1 given)", rounds=-1)
    for moves in (-1, 0, 32, 255):
        refused(b"1 <= moves <= 31", moves=moves)
        refused(b"(%d given)" % moves, moves=moves)
    for name in names:
        refused(b"NULL matrix/start/tour/key/duration/info buffer", **{name: None})
    refused(b"H must be 1 or 24", R=0, H=3)            # the shape checks also with R = 0
    refused(b"1 <= S <= 65535", R=0, S=0)
    refused(b"1 <= moves <= 31", R=0, moves=0)
    # the new ones
    for G in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= G <= 65535 (%d given)" % G, G=G)
    refused(b"1 <= G <= 65535", R=0, G=0)
    refused(b"the workspace is NULL", work=None)
    refused(b"8-byte aligned", work=p + 4)
    need = work_bytes(1, 5, 2)
    refused(b"the workspace has %d bytes" % (need - 1), wb=need - 1)
    refused(b"need %d" % need, wb=0)
    # the clamp is to min(G, S): 3 starts need 3 records, whatever G says
    refused(b"need %d" % work_bytes(7, 5, 3), R=7, S=3, G=64, wb=work_bytes(7, 5, 3) - 1)
    refused(b"bytes of LDS", R=7, S=3, G=64, wb=work_bytes(7, 5, 3))
    refused(b"R * min(G, S) = %d workgroups are above 2^31 - 1" % (32769 * 65535), R=32769, S=65535,
            G=65535, wb=2**64 - 1)
    refused(b"bytes of LDS", R=32768, S=65535, G=65535, wb=2**64 - 1)
    for N, H, wide in ((5, 1, 0), (58, 24, 0), (59, 24, 1), (274, 1, 0)):
        refused(b"needs %d bytes of LDS (0 available)" % spread_lds_bytes(N, H, wide), N=N, H=H,
                wide=wide)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, G=65535, work=None, wb=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert buf.raw == bytes(1 << 16) and fake.raw == bytes(1 << 16)


def test_auto_policy_table():
    assert solver.BATCH_LSO_MAX_SPREAD == 1024
    # min(S, max(1, 16 cus // R)): the factor 16 is DESIGN.md §4.3t's, measured
    for (R, S, cus), want in (((1, 64, 256), 64), ((1, 1024, 256), 1024), ((16, 64, 256), 64),
                              ((512, 64, 256), 8), ((10000, 64, 256), 1), ((3, 64, 256), 64),
                              ((64, 64, 256), 64), ((65, 64, 256), 63), ((2048, 64, 256), 2),
                              ((2049, 64, 256), 1), ((4096, 64, 256), 1), ((1, 1, 256), 1),
                              ((100, 1024, 304), 48)):
        assert solver.batch_lso_spread(R, S, cus) == want, (R, S, cus)


def test_spread_values_are_checked_before_a_device_is_touched(monkeypatch, lib):
    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: pytest.fail("the remote was touched"))
    real_launch = solver.batch_lso_launch
    monkeypatch.setattr(solver, "batch_lso_launch", lambda *a, **k: pytest.fail("a launch was reached"))
    good = request((6, 1, 0, ""))
    for bad in (0, 1025, True, "x", 2.0, -1, "8"):
        with pytest.raises(ValueError, match=r'spread must be None, "auto" or an integer in 1\.\.1024'):
            solver.solve_tsp_lso_batch([good], spread=bad)
        with pytest.raises(ValueError, match=r'spread must be None, "auto" or an integer in 1\.\.1024'):
            solver.solve_tsp("lso", *good, spread=bad)
        with pytest.raises(ValueError, match="spread must be"):
            real_launch(None, [], 8, 3, 31, 0, spread=bad)
    for ok in (None, "auto", 1, 4, 1024, np.int64(7)):
        assert solver.check_lso_spread(ok) == ok


def test_the_launch_sees_the_spread_it_was_given(monkeypatch, lib):
    seen = []

    def launch(ctx, cis, starts, rounds, moves, seed, spread=None):
        seen.append((len(cis), starts, rounds, moves, seed, spread))
        return [list(range(1, ci.n + 1)) for ci in cis], [0] * len(cis)

    monkeypatch.setattr(solver, "batch_lso_launch", launch)
    monkeypatch.setattr(solver, "context", lambda dev=0: "ctx")
    monkeypatch.setattr(solver, "_remote", lambda: None)
    reqs = [request((6, 1, x, "")) for x in range(3)]
    solver.solve_tsp_lso_batch(reqs, starts=8, rounds=3, seed=5)
    solver.solve_tsp_lso_batch(reqs, starts=8, rounds=3, seed=5, spread="auto")
    solver.solve_tsp_lso_batch(reqs[:1], starts=8, rounds=3, moves=7, seed=5, spread=7)
    solver.solve_tsp("lso", *reqs[0], starts=9, rounds=2, seed=6)
    solver.solve_tsp("lso", *reqs[0], starts=9, rounds=2, seed=6, spread=1024)
    solver.solve_tsp("lso", *reqs[0], starts=9, rounds=2, seed=6, spread="auto")
    assert seen == [(3, 8, 3, 31, 5, None), (3, 8, 3, 31, 5, "auto"), (1, 8, 3, 7, 5, 7),
                    (1, 9, 2, 31, 6, None), (1, 9, 2, 31, 6, 1024), (1, 9, 2, 31, 6, "auto")]


def test_batch_lso_launch_chooses_the_kernels(monkeypatch, lib):
    """None and an "auto" of 1 are tsp_batch_lso; a number, 1 included, is
    tsp_batch_lso_spread at that number; "auto" asks batch_lso_spread."""
    torch = pytest.importorskip("torch")
    calls = []

    class Ctx:
        dev = "cpu"
        cus = 256

        def _out(self, R):
            return (torch.zeros((R, 6), dtype=torch.int16), torch.zeros(R, dtype=torch.int64),
                    torch.zeros(R, dtype=torch.int32), None)

        def tsp_batch_lso(self, mats, *a, wide=None):
            calls.append(("lso", mats.shape[0]) + a[1:])
            return self._out(mats.shape[0])

        def tsp_batch_lso_spread(self, mats, *a, wide=None):
            calls.append(("spread", mats.shape[0]) + a[1:])
            return self._out(mats.shape[0])

    ci = solver.compact_tsp(*request((6, 1, 0, "")))
    for R, spread in ((1, None), (1, 1), (1, 5), (1, "auto"), (16, "auto"), (300, "auto"),
                      (2048, "auto"), (2049, "auto")):
        solver.batch_lso_launch(Ctx(), [ci] * R, 64, 9, 31, 3, spread=spread)
    assert calls == [("lso", 1, 64, 9, 31, 3), ("spread", 1, 64, 9, 31, 3, 1),
                     ("spread", 1, 64, 9, 31, 3, 5), ("spread", 1, 64, 9, 31, 3, 64),
                     ("spread", 16, 64, 9, 31, 3, 64), ("spread", 300, 64, 9, 31, 3, 13),
                     ("spread", 2048, 64, 9, 31, 3, 2), ("lso", 2049, 64, 9, 31, 3)]


def test_inline_knob_and_its_forwarding(monkeypatch, lib):
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append(dict(knobs.get("inline") or {}))
        return {"duration": 5, "vehicle": [0, 1, 0]}

    assert service.INLINE_KNOBS["spread"] is int and service.KNOB_RANGES["spread"] == (1, 1024)
    app = service.App(service.MemoryStore({}, {}, {}), solve=fake)
    for spread in (1, 4, 1024):
        st, _ = app.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, ""), knobs={"spread": spread}))
        assert st == 200 and seen.pop() == {"spread": spread}
    for spread in (0, 1025, -1, "auto", None, True, [4]):
        st, res = app.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, ""), knobs={"spread": spread}))
        assert st == 400 and res["errors"][0]["what"] == "Invalid request", (spread, res)
    assert seen == []
    # the service's own solve hands the knob to solver.solve_tsp
    got = []

    def solve_tsp(algorithm, durations, customers, start_node, start_time, **kw):
        got.append((algorithm, kw.get("spread"), kw.get("starts")))
        return {"duration": 5, "vehicle": [0, 1, 0]}

    monkeypatch.setattr(solver, "solve_tsp", solve_tsp)
    real = service.App(service.MemoryStore({}, {}, {}))
    st, _ = real.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, ""), knobs={"spread": 4, "starts": 8}))
    assert st == 200
    st, _ = real.solve_inline("tsp", "lso", _tsp_body((5, 1, 0, ""), knobs={"starts": 8}))
    assert st == 200 and got == [("lso", 4, 8), ("lso", None, 8)]
    monkeypatch.undo()
    # the forwarding table of vrpms_amd.remote is INLINE_KNOBS
    from vrpms_amd import remote
    out = {}
    remote._options(out, 1, None, {"spread": 4, "starts": 8, "moves": 7})
    assert out["knobs"] == {"spread": 4, "starts": 8, "moves": 7}
    # with a remote only a number travels: "auto" is the GPU box's own decision
    sent = []

    class Box:
        @staticmethod
        def solve_tsp(algorithm, durations, customers, start_node, start_time, **kw):
            sent.append(kw)
            return {"duration": 1, "vehicle": [start_node] + list(customers) + [start_node]}

    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: Box)
    a = request((6, 1, 0, ""))
    base = dict(seed=9, time_limit=None, starts=8, rounds=3, moves=7)
    for spread, more in ((None, {}), ("auto", {}), (4, {"spread": 4}), (np.int64(6), {"spread": 6})):
        solver.solve_tsp_lso_batch([a], starts=8, rounds=3, moves=7, seed=9, spread=spread)
        assert sent.pop() == dict(base, **more)
        solver.solve_tsp("lso", *a, starts=8, rounds=3, moves=7, seed=9, spread=spread)
        assert sent.pop() == dict(base, **more) and sent == []


@functools.lru_cache(maxsize=None)
def rounds_under_the_share(run):
    """a27_ref's descents once more with its moves alone, noting what the
    256-thread share makes of every round: thread t prices the ids [t per, (t +
    1) per), wavefront t // 64 -> dict(n, moves, per, idle = the threads
    without a move, won = the wavefronts whose share held an applied move,
    cross = the rounds whose least key sat on moves of different wavefronts
    that give different tours, key, s, tour)."""
    case, S, rounds, mask = run
    D, t0 = inst(case)
    D = spec.as_3d(D)
    n = D.shape[1] - 1
    mvs, src = all_moves(n, mask), move_sources(n, mask)
    per = -(-len(mvs) // 256)
    wave = [(x // per) // 64 for x in range(len(mvs))]
    won, cross, ends = set(), 0, []
    for s in range(S):
        t = shuffled(n, s, SEED)
        k = spec.tsp_key(int(spec.eval_tsp_batch(D, [t], t0)[0]))
        applied = 0
        while n >= 2 and mvs and applied < rounds:
            cands = np.asarray(t, dtype=np.int64)[src]
            keys = [spec.tsp_key(int(x)) for x in spec.eval_tsp_batch(D, cands, t0)]
            kmin = min(keys)
            if not kmin < k:
                break
            at = keys.index(kmin)
            best = cands[at].tolist()
            won.add(wave[at])
            cross += any(kk == kmin and wave[x] != wave[at] and cands[x].tolist() != best
                         for x, kk in enumerate(keys))
            t, k = best, kmin
            applied += 1
        ends.append((k, s, t))
    k, s, t = min(ends, key=lambda e: e[:2])
    return dict(n=n, moves=len(mvs), per=per, idle=256 - -(-len(mvs) // per), won=won, cross=cross,
                key=k, s=s, tour=t)


def type_ends(n, mask):
    """The id one past the last move of every enabled type but the last."""
    typs = [typ for typ, _, _ in all_moves(n, mask)]
    return [x for x in range(1, len(typs)) if typs[x] != typs[x - 1]]


def test_reference_properties_under_the_256_thread_share(lib):
    """What the GPU cases claim to exercise, checked on the reference: the share
    is vrpms_tsp_batch_lso_spread's (lso_share_wg), per = ceil(moves / 256)."""
    assert lib.vrpms_tsp_batch_lso_spread is not None
    got = {run: rounds_under_the_share(run) for run in NEW_RUNS}
    for run, r in got.items():   # the same descents as a27_ref's
        ref = reference(run)
        assert (r["key"], r["s"], r["tour"]) == (ref["key"], ref["s"], ref["tour"]), run
        assert ref["capped"] == 0
    shape = {run: (r["n"], r["moves"], r["per"], r["idle"]) for run, r in got.items()}
    assert shape[IDLE] == (9, 242, 1, 14)
    assert shape[PER2] == (10, 308, 2, 102)
    assert len(all_moves(9)) <= 256 < len(all_moves(10))          # n = 10 is the first per = 2
    assert shape[PER4] == (16, 872, 4, 38)
    assert shape[TIES_A] == (9, 242, 1, 14) and shape[TIES_B] == (10, 308, 2, 102)
    # the winning move lay in every wavefront's share at some round
    assert got[PER4]["won"] == {0, 1, 2, 3} and got[IDLE]["won"] == {0, 1, 2, 3}
    assert got[PER2]["won"] >= {0, 1, 2}                          # 154 busy threads: wavefront 3 is idle
    # rounds whose least key sat on moves of different wavefronts that give
    # different tours: the (key, wavefront) choice is put to the test
    assert got[TIES_A]["cross"] == 14 and got[TIES_B]["cross"] == 11
    assert got[TIES_A]["won"] == {0, 1, 2} and got[TIES_B]["won"] == {0, 1}
    # with MASK_BETWEEN's wavefront 2 -- the Or-opt 3 moves alone -- winning rounds
    assert got[MASK_BETWEEN]["won"] == {0, 1, 2} and got[MASK_IN]["cross"] == 4
    assert reference(TIES_A)["move_tie"] and reference(TIES_B)["move_tie"]
    # a type boundary inside one thread's share: every type of MASK_IN ends on
    # an odd id at per = 2, so one thread prices the last move of a type and
    # the first of the next
    assert shape[MASK_IN] == (10, 263, 2, 124) and type_ends(10, 29) == [45, 135, 207]
    assert all(e % 2 for e in type_ends(10, 29))
    # a type boundary between two wavefronts: Or-opt 2 ends at id 128 at per =
    # 1, so wavefront 2 starts on the first Or-opt 3 move; relocate ends inside
    # wavefront 1
    assert shape[MASK_BETWEEN] == (9, 170, 1, 86) and type_ends(9, 28) == [72, 128]
    for run in (MASK_IN, MASK_BETWEEN):   # and the types on both sides are applied
        assert len({typ for typ, _, _ in reference(run)["moves"]}) >= 2, run
    # the group edges: G > S, G not dividing S, and the answer's start held by
    # the last workgroup
    assert sorted({r[1] for r in GROUP_RUNS}) == [1, 5, 9]
    assert [reference(r)["s"] for r in GROUP_RUNS] == [0, 0, 0, 4, 8]
    last = {(r[1], G) for r in GROUP_RUNS for G in GROUP_G
            if 1 < min(G, r[1]) and reference(r)["s"] % min(G, r[1]) == min(G, r[1]) - 1}
    assert last == {(5, 5), (5, 9), (5, 64), (9, 9), (9, 64)}
    # info's capped count sums over the groups: R_EDGES cap some descents
    assert reference(R_EDGES[0])["capped"] == 7 and 0 < reference(R_EDGES[2])["capped"]
    # the long runs keep four copies equal over more than 64 positions
    assert all(r[0][0] == 135 and r[1] == 1 and r[2] == 1 for r in LONG)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _lists(out):
    tours, keys, durs, info = out
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), info.cpu().tolist())


def gpu_args(ctx, cases):
    import torch
    insts = [inst(c) for c in cases]
    return (torch.tensor(np.stack([D for D, _ in insts]), dtype=torch.int32, device=ctx.dev),
            torch.tensor([t0 for _, t0 in insts], dtype=torch.int32, device=ctx.dev))


def gpu_spread(ctx, cases, S, rounds, moves, G, wide=None):
    """One tsp_batch_lso_spread launch -> ([key], [tour], [dur], [info])."""
    return _lists(ctx.tsp_batch_lso_spread(*gpu_args(ctx, cases), S, rounds, moves, SEED, G, wide=wide))


def gpu_runs(ctx, runs, G, wide=None):
    """Runs of one shape and one (S, rounds, moves) in one launch."""
    assert len({r[1:] for r in runs}) == 1 and len({r[0][:2] for r in runs}) == 1
    return gpu_spread(ctx, [r[0] for r in runs], *runs[0][1:], G, wide=wide)


_OTHERS = [r for r in ALL_RUNS if r not in MASKS]


@pytest.mark.gpu
@pytest.mark.parametrize("runs", [_OTHERS, [r for r in MASKS if r[0][1] == 1],
                                  [r for r in MASKS if r[0][1] == 24]],
                         ids=["all-but-masks", "masks-H1", "masks-H24"])
def test_gpu_equals_reference_on_the_existing_runs(ctx, runs):
    """Every run of the parent's ALL_RUNS, the LONG ones included, at G = S."""
    assert len(_OTHERS) + len(MASKS) == len(ALL_RUNS) and all(r in _OTHERS for r in LONG)
    for group in by_launch(runs):
        got = gpu_runs(ctx, group, group[0][1])
        want = expected(group)
        print([run_id(r) for r in group], "gpu", got, "ref", want)
        assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("run", NEW_RUNS, ids=run_id)
def test_gpu_equals_reference_on_the_new_runs(ctx, run):
    want = expected([run])
    for G in (1, 2, run[1]):
        got = gpu_runs(ctx, [run], G)
        print(run_id(run), G, "gpu", got, "ref", want)
        assert got == want, G


@pytest.mark.gpu
def test_gpu_every_mask_on_the_clock_at_n_7(ctx):
    for run in MASKS_24:
        for G in (1, run[1]):
            assert gpu_runs(ctx, [run], G) == expected([run]), (run_id(run), G)


@pytest.mark.gpu
def test_gpu_group_edges(ctx):
    """The clamp to min(G, S), the ragged last stride, the answer in the last
    workgroup, and the capped count summed over the groups."""
    for run in GROUP_RUNS:
        want = expected([run])
        for G in GROUP_G:
            assert gpu_runs(ctx, [run], G) == want, (run[1], G)
    for run in R_EDGES:
        want = expected([run])
        for G in (1, 3, 7):
            assert gpu_runs(ctx, [run], G) == want, (run, G)
    assert expected([R_EDGES[0]])[3][0][1] == 7


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(12, 1), (9, 24)], ids=["n12-H1", "n9-H24"])
def test_gpu_equals_tsp_batch_lso(ctx, shape):
    """No oracle involved: all four tensors of the two mappings are equal, the
    capped counts included."""
    import torch
    n, H = shape
    cases = [(n, H, 200 + x, "ties" if x % 8 == 7 else "") for x in range(40)]
    args = gpu_args(ctx, cases)
    S = 16
    for rounds in (1000, 2):
        old = ctx.tsp_batch_lso(*args, S, rounds, 31, SEED)
        assert (old[3][:, 1] > 0).any().item() == (rounds == 2)   # some descents are capped at 2
        for G in (1, 3, 16):
            new = ctx.tsp_batch_lso_spread(*args, S, rounds, 31, SEED, G)
            for x, (a, b) in enumerate(zip(old, new)):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (rounds, G, x)
    # two launches are identical
    again = ctx.tsp_batch_lso_spread(*args, S, 2, 31, SEED, 16)
    assert all(torch.equal(a, b) for a, b in zip(new, again))
    # R = 0 returns empty tensors
    z = (torch.zeros((0, 24, 11, 11), dtype=torch.int32, device=ctx.dev),
         torch.zeros((0,), dtype=torch.int32, device=ctx.dev))
    out = ctx.tsp_batch_lso_spread(*z, 8, 5, 31, SEED, 4)
    assert [tuple(t.shape) for t in out] == [(0, 10), (0,), (0,), (0, 2)]
    assert [t.dtype for t in out] == [t.dtype for t in ctx.tsp_batch_lso(*z, 8, 5, 31, SEED)]


@pytest.mark.gpu
def test_gpu_staging_width_refusals_and_the_clamp(ctx):
    """The parent's staging cases through the new entry: all four
    instantiations, (uint16 | int32) x (H = 1 | 24); an entry of 65535 rides
    uint16, 65536 is the refusal row there and rides int32; a negative entry is
    refused under either width; durations above 2^28.  Refusal rows sit beside
    good rows in one launch."""
    import torch
    for H in (1, 24):
        a, b, c = (7, H, 30, ""), (7, H, 31, "e65535"), (7, H, 32, "")
        over = (7, H, 31, "e65536")

        def runs(*cases):
            return [(x, 6, 1000, 31) for x in cases]

        for G in (1, 4):
            assert gpu_runs(ctx, runs(a, b, c), G, wide=False) == expected(runs(a, b, c))
            assert gpu_runs(ctx, runs(a, over, c), G, wide=True) == expected(runs(a, over, c))
            assert gpu_runs(ctx, runs(over), G) == expected(runs(over))   # wide=None
            want = expected(runs(a, over, c))
            keys, tours, durs, info = gpu_runs(ctx, runs(a, over, c), G, wide=False)
            assert keys[1] == 2**64 - 1 and tours[1] == [0] * 7 and durs[1] == 0 and info[1] == [-1, 0]
            for x in (0, 2):
                assert (keys[x], tours[x], durs[x], info[x]) == tuple(w[x] for w in want)
            mats = np.stack([inst(x)[0] for x in (a, b, c)]).astype(np.int32)
            mats[1, H - 1, 3, 2] = -1
            st = gpu_args(ctx, (a, b, c))[1]
            want = expected(runs(a, b, c))
            for wide in (False, True):
                keys, tours, durs, info = _lists(ctx.tsp_batch_lso_spread(
                    torch.tensor(mats, dtype=torch.int32, device=ctx.dev), st, 6, 1000, 31, SEED, G,
                    wide=wide))
                assert keys[1] == 2**64 - 1 and tours[1] == [0] * 7 and durs[1] == 0 and \
                    info[1] == [-1, 0]
                for x in (0, 2):
                    assert (keys[x], tours[x], durs[x], info[x]) == tuple(w[x] for w in want)
    for run in HUGE:
        for G in (1, 6):
            got = gpu_runs(ctx, [run], G)
            assert got == expected([run]) and got[3] == [[0, 0]] and got[2][0] > 2**28
    for run in E65535 + E65536:
        assert gpu_runs(ctx, [run], 3) == expected([run])


@pytest.mark.gpu
def test_gpu_batch_independence(ctx):
    """A request's row is the same alone, as row 0 and as row 7 of eight, and
    at two values of G."""
    want = expected(SIX)
    S = SIX[0][1]
    eight = [SIX[3]] + [SIX[x % 6] for x in range(6)] + [SIX[3]]
    for G in (3, S):
        assert gpu_runs(ctx, SIX, G) == want
        got = gpu_runs(ctx, eight, G)
        alone = gpu_runs(ctx, [SIX[3]], G)
        assert alone == tuple([w[3]] for w in want)
        for x in (0, 7):
            assert tuple(g[x] for g in got) == tuple(g[0] for g in alone), (G, x)
        for x in range(1, 7):
            assert tuple(g[x] for g in got) == tuple(w[x - 1] for w in want), (G, x)


@pytest.mark.gpu
@pytest.mark.parametrize("H,wide", sorted(DOMAIN), ids=lambda v: str(int(v)))
def test_gpu_lds_edge(ctx, H, wide):
    """The largest N of the new formula launches: at the parent's own edge the
    two kernels agree; past it, where only the new mapping fits, the tour is a
    permutation whose walk is the duration.  One node more is refused on the
    host, nothing launched and nothing written."""
    import torch
    lib, R, G, S = ctx.lib, 2, 2, 2
    top = largest_spread_nodes(H, wide)
    old_top = DOMAIN[(H, wide)]
    assert old_top <= top
    variant = "e65536" if wide else ""
    for N in sorted({old_top, top}):
        cases = [(N - 1, H, 40 + x, variant) for x in range(R)]
        args = gpu_args(ctx, cases)
        new = ctx.tsp_batch_lso_spread(*args, S, 1, 31, SEED, G, wide=wide)
        if N <= old_top:
            old = ctx.tsp_batch_lso(*args, S, 1, 31, SEED, wide=wide)
            assert all(torch.equal(a, b) for a, b in zip(old, new)), N
        keys, tours, durs, info = _lists(new)
        for x, case in enumerate(cases):
            D, t0 = inst(case)
            assert sorted(tours[x]) == list(range(1, N))
            assert spec.eval_tsp(D, tours[x], t0) == durs[x] and keys[x] == spec.tsp_key(durs[x])
            assert 0 <= info[x][0] < S and 0 <= info[x][1] <= S
        one = _lists(ctx.tsp_batch_lso_spread(*args, S, 1, 31, SEED, 1, wide=wide))
        assert one == (keys, tours, durs, info)
    N, n = top + 1, top
    M = torch.ones((R, H, N, N), dtype=torch.int32, device=ctx.dev)
    st = torch.ones((R,), dtype=torch.int32, device=ctx.dev)
    wb = work_bytes(R, N, G)
    work = torch.full((wb,), -7, dtype=torch.int8, device=ctx.dev)
    tours = torch.full((R, n), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R,), -7, dtype=torch.int32, device=ctx.dev)
    info = torch.full((R, 2), -7, dtype=torch.int32, device=ctx.dev)
    rc = lib.vrpms_tsp_batch_lso_spread(ctx.handle, M.data_ptr(), st.data_ptr(), R, N, H, int(wide), S,
                                        1, 31, SEED, G, work.data_ptr(), wb, tours.data_ptr(),
                                        keys.data_ptr(), durs.data_ptr(), info.data_ptr(), ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_tsp_batch_lso_spread:" in msg and b"bytes of LDS" in msg
    assert str(spread_lds_bytes(N, H, wide)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item() and (work == -7).all().item()
    assert (durs == -7).all().item() and (info == -7).all().item()


@pytest.mark.gpu
def test_solve_tsp_and_solve_tsp_lso_batch_with_a_spread():
    S, rounds = 8, 1000
    D7, cust7, _, t7 = request((6, 24, 50, ""))
    reqs = [request((6, 24, 51, "")), request((9, 1, 52, "")),
            (D7, [], 2, t7),                                                  # no customer
            request((6, 24, 53, "")),
            {"durations": D7, "customers": [5, 3, 3, 1], "start_node": 2, "start_time": 1439},
            request((9, 1, 54, ""))]
    kw = dict(starts=S, rounds=rounds, seed=SEED)
    default = solver.solve_tsp_lso_batch(reqs, **kw)
    for spread in (None, 1, 4, "auto"):
        assert solver.solve_tsp_lso_batch(reqs, spread=spread, **kw) == default, spread
        for x in (0, 1, 2, 5):
            assert solver.solve_tsp("lso", *reqs[x], spread=spread, **kw) == default[x], (spread, x)
    # the answers are A27's and the mask is read under a spread too
    for x, case in ((0, (6, 24, 51, "")), (1, (9, 1, 52, ""))):
        r = reference((case, S, rounds, 31))
        assert default[x] == {"duration": r["dur"], "vehicle": [0] + r["tour"] + [0]}
    r = reference(((9, 1, 52, ""), S, rounds, 1))
    assert solver.solve_tsp_lso_batch(reqs[1:2], moves=1, spread=4, **kw) == \
        [{"duration": r["dur"], "vehicle": [0] + r["tour"] + [0]}] != default[1:2]


def _post(port, case, **kw):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/solve/tsp/lso", data=_tsp_body(case, **kw),
                                 method="POST")
    with urllib.request.urlopen(req, timeout=120) as resp:
        return resp.status, json.loads(resp.read())


@pytest.mark.gpu
def test_inline_spread_over_http_gives_the_same_body():
    S, rounds, case = 8, 1000, (9, 1, 52, "")
    app = service.App(service.MemoryStore({}, {}, {}), seed=SEED)
    srv = service.serve(app, "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    try:
        port = srv.server_address[1]
        plain = _post(port, case, knobs={"starts": S, "rounds": rounds})
        knob = _post(port, case, knobs={"starts": S, "rounds": rounds, "spread": 4})
    finally:
        srv.shutdown()
        srv.server_close()
        th.join()
    assert plain[0] == 200 and plain[1]["success"], plain
    r = reference((case, S, rounds, 31))
    assert plain[1]["message"] == {"duration": r["dur"], "vehicle": [0] + r["tour"] + [0]}
    assert knob == plain
