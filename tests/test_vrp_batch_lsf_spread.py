"""The delta-priced local search over plain separator tours (spec A28) by its
second mapping: the C entry points
vrpms_vrp_batch_lsf_spread_lds / vrpms_vrp_batch_lsf_spread_work /
vrpms_vrp_batch_lsf_spread, Context.vrp_batch_lsf_spread,
solver.check_lsf_spread / batch_lsf_spread and the `spread` argument of
batch_lsf_launch / solve_vrp_lsf_batch / solve_vrp("lsf"), and the inline knob
"spread" of /solve/vrp/lsf.

The mapping is free under A28, so there is no new reference: per request the
GPU must return the identical key, tour, route durations, vehicle row and info
row as Context.vrp_batch_lsf on the same buffers, and as
tests/test_vrp_batch_lsf.py's a28_ref where that file computes it, for every
number of workgroups per request."""
import ctypes
import json
import threading
import urllib.request

import numpy as np
import pytest

from test_vrp_batch_ga import _body, _no_gpu
from test_vrp_batch_ls import LDS_BYTES, OBJECTIVES, SEED, obj_id, pad
from test_vrp_batch_lsf import (ALL_RUNS, DOMAIN, GRID_N, ROOMY, SIX, expected, gpu_args, inst, lds_bytes,
                                reference, request)
from test_vrp_batch_lsr_spread import IDLE, PER2, TIES_A
from vrpms_amd import _lib, core, service, solver

# the 256-thread share's own edges on static matrices: (case, S, rounds).  A
# round of L tokens has 2 L (L - 1) moves, per = ceil(moves / 256) a thread.
# IDLE: L = 11, 220 moves, 36 idle threads; PER2: L = 12, 264 moves, the first
# per = 2; TIES_A: L = 16, equal keys in different wavefronts' shares
PER4 = ((20, 4, 1, 1, ""), 4, 1000)        # L = 23: 1012 moves, per = 4
SHARE_RUNS = [IDLE, PER2, TIES_A, PER4]


def spread_lds_bytes(N, K, wide):
    """DESIGN.md §4.3x restated, L = N + K - 2 tokens: the instance as
    vrp_batch_lsf keeps it, per wavefront three int32 rows of L + 2 and five
    int32 tables of K + 1 padded to four words, uint16 rows of L + 2 and K + 1
    padded to eight and a byte row of L + 2 padded to eight, and two sets of
    four 16-byte round records."""
    L = N - 1 + K - 1
    return pad(N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + \
        4 * 4 * (3 * pad(L + 2, 4) + 5 * pad(K + 1, 4)) + \
        4 * 2 * (pad(L + 2, 8) + pad(K + 1, 8)) + 4 * pad(L + 2, 8) + 2 * 4 * 16


def work_bytes(R, N, K, G):
    return R * G * (16 + 2 * pad(N - 1 + K - 1, 8))


@pytest.fixture(scope="module")
def lib():
    from vrpms_amd.build import build_library
    build_library()
    return _lib.load()


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_lds_is_at_most_vrp_batch_lsf_s(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_vrp_batch_lsf_spread_lds
    for wide in (0, 1):
        for K in (1, 3, 4, 5, 7, 8, 64):
            for N in GRID_N:
                L = N - 1 + K - 1
                assert f(N, K, wide, ctypes.byref(b)) == _lib.VRPMS_OK
                assert b.value == spread_lds_bytes(N, K, wide) == core.vrp_batch_lsf_spread_lds(N, K, 1, wide)
                old = core.vrp_batch_lsf_lds(N, K, 1, wide)
                assert old == lds_bytes(N, K, wide) and b.value <= old
                assert old - b.value == 8 * pad(L, 8) - 64
    # the smallest tour row is where the two meet
    assert core.vrp_batch_lsf_spread_lds(2, 1, 1, False) == core.vrp_batch_lsf_lds(2, 1, 1, False)
    assert core.vrp_batch_lsf_spread_lds(2, 1, 1, True) == core.vrp_batch_lsf_lds(2, 1, 1, True)
    # at A28's own edges
    for (K, wide), N in DOMAIN.items():
        assert core.vrp_batch_lsf_spread_lds(N, K, 1, wide) <= core.vrp_batch_lsf_lds(N, K, 1, wide) \
            <= LDS_BYTES
    # the same refusals, the same words
    old = lib.vrpms_vrp_batch_lsf_lds
    for args, word in (((1, 3, 0), b"2 <= N"), ((0, 3, 0), b"2 <= N"), ((65536, 3, 0), b"2 <= N"),
                       ((5, 0, 0), b"1 <= K <= 64"), ((5, 65, 0), b"1 <= K <= 64"),
                       ((65535, 3, 0), b"N + K - 2 <= 65535 (65536 given)"),
                       ((65474, 64, 0), b"N + K - 2 <= 65535 (65536 given)"),
                       ((5, 3, 2), b"wide"), ((5, 3, -1), b"wide")):
        b.value = 77
        assert old(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        theirs = lib.vrpms_last_error()
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsf_spread_lds" in msg and word in msg, (args, msg)
        assert msg == theirs.replace(b"vrpms_vrp_batch_lsf_lds", b"vrpms_vrp_batch_lsf_spread_lds")
        assert b.value == 77
    assert f(65535, 2, 0, ctypes.byref(b)) == _lib.VRPMS_OK
    assert f(5, 3, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_lsf_spread_lds: bytes is NULL" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= K <= 64"):
        core.vrp_batch_lsf_spread_lds(5, 65, 1, False)
    with pytest.raises(ValueError, match="H must be 1 .24 given.*vrp_batch_lsr_spread"):
        core.vrp_batch_lsf_spread_lds(5, 3, 24, False)


def test_workspace_bytes(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_vrp_batch_lsf_spread_work
    for R in (0, 1, 3, 10000):
        for N, K in ((2, 1), (5, 2), (8, 3), (9, 1), (10, 1), (58, 4), (267, 4), (3, 64)):
            for G in (1, 2, 64, 1024, 65535):
                assert f(R, N, K, G, ctypes.byref(b)) == _lib.VRPMS_OK
                assert b.value == work_bytes(R, N, K, G) == core.vrp_batch_lsf_spread_work(R, N, K, G)
                assert b.value == core.vrp_batch_lsr_spread_work(R, N, K, G)   # the same record
                assert b.value % 16 == 0
    assert work_bytes(1, 8, 3, 1) == 16 + 2 * 16 and work_bytes(1, 7, 3, 1) == 16 + 2 * 8
    assert f(32767, 65535, 2, 65535, ctypes.byref(b)) == _lib.VRPMS_OK
    assert b.value == 32767 * 65535 * (16 + 2 * 65536)
    for args, word in (((-1, 5, 2, 1), b"R must not be negative"), ((1, 1, 2, 1), b"2 <= N"),
                       ((1, 5, 0, 1), b"1 <= K <= 64"), ((1, 5, 65, 1), b"1 <= K <= 64"),
                       ((1, 65535, 3, 1), b"N + K - 2 <= 65535"),
                       ((1, 5, 2, 0), b"1 <= G <= 65535 (0 given)"),
                       ((1, 5, 2, 65536), b"1 <= G <= 65535 (65536 given)"),
                       ((1, 5, 2, -1), b"1 <= G <= 65535"),
                       ((32769, 5, 2, 65535), b"R * G = %d records are above 2^31 - 1" % (32769 * 65535))):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsf_spread_work" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(1, 5, 2, 1, None) == _lib.VRPMS_EINVAL
    assert b"bytes is NULL" in lib.vrpms_last_error()


def test_argument_errors_need_no_gpu(lib):
    """As tests/test_vrp_batch_lsf.py's: every argument check comes before the
    context is looked at, so a block of zeros serves as the non-NULL ctx; its
    LDS size of zero makes every launch that passes the other checks an LDS
    refusal."""
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 16)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    assert p % 8 == 0
    names = ("m", "d", "cp", "st", "t", "k", "du", "v", "i")

    def f(ctx=c, R=1, N=5, K=2, H=1, obj=0, wide=0, S=8, rounds=3, G=2, work=p, wb=1 << 16, **ptrs):
        a = {name: ptrs.get(name, p) for name in names}
        return lib.vrpms_vrp_batch_lsf_spread(ctx, a["m"], a["d"], a["cp"], a["st"], R, N, K, H, obj,
                                              wide, S, rounds, 12345, G, work, wb, a["t"], a["k"],
                                              a["du"], a["v"], a["i"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsf_spread:" in msg and word in msg, (kw, msg)

    # vrpms_vrp_batch_lsf's
    refused(b"ctx is NULL", ctx=None)
    refused(b"R must not be negative", R=-1)
    for N in (-1, 0, 1, 65536):
        refused(b"2 <= N", N=N)
    for K in (-1, 0, 65, 1000):
        refused(b"1 <= K <= 64", K=K)
    refused(b"N + K - 2 <= 65535 (65536 given)", N=65535, K=3)
    for H in (0, 2, 12, 25):
        refused(b"H must be 1 or 24", H=H)
    refused(b"H must be 1 (24 given)", H=24)
    refused(b"vrpms_vrp_batch_lsr", H=24)
    refused(b"H must be 1 (24 given)", H=24, R=0)
    for obj in (-1, 2):
        refused(b"objective", obj=obj)
    for wide in (-1, 2):
        refused(b"wide", wide=wide)
    for S in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= S <= 65535 (%d given)" % S, S=S)
    refused(b"rounds must not be negative (-1 given)", rounds=-1)
    for name in names:
        refused(b"NULL", **{name: None})
    refused(b"1 <= S <= 65535", R=0, S=0)
    # the spread's own, in vrpms_vrp_batch_lsr_spread's order
    for G in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= G <= 65535 (%d given)" % G, G=G)
    refused(b"1 <= G <= 65535", R=0, G=0)
    refused(b"1 <= S <= 65535", S=0, G=0)                 # the search before G
    refused(b"1 <= G <= 65535", G=0, m=None)              # G before the buffers
    refused(b"NULL matrix", m=None, work=None)            # the buffers before the workspace
    refused(b"the workspace is NULL", work=None)
    refused(b"8-byte aligned", work=p + 4)
    need = work_bytes(1, 5, 2, 2)
    refused(b"the workspace has %d bytes" % (need - 1), wb=need - 1)
    refused(b"need %d" % need, wb=0)
    # the clamp is to min(G, S): 3 starts need 3 records, whatever G says
    refused(b"need %d" % work_bytes(7, 5, 2, 3), R=7, S=3, G=64, wb=work_bytes(7, 5, 2, 3) - 1)
    refused(b"bytes of LDS", R=7, S=3, G=64, wb=work_bytes(7, 5, 2, 3))
    refused(b"R * min(G, S) = %d workgroups are above 2^31 - 1" % (32769 * 65535), R=32769, S=65535,
            G=65535, wb=2**64 - 1)
    refused(b"bytes of LDS", R=32768, S=65535, G=65535, wb=2**64 - 1)
    for N, K, wide in ((5, 2, 0), (58, 4, 1), (5, 1, 0), (12, 64, 0)):
        refused(b"needs %d bytes of LDS (0 available)" % spread_lds_bytes(N, K, wide), N=N, K=K,
                wide=wide)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, G=65535, work=None, wb=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert buf.raw == bytes(1 << 16) and fake.raw == bytes(1 << 16)


def test_spread_values_and_the_auto_policy(monkeypatch, lib):
    assert solver.BATCH_LSF_MAX_SPREAD == 1024
    assert solver.HEURISTIC_KINDS["lsf"].max_spread == 1024
    for ok in (None, "auto", 1, 4, 1024, np.int64(7)):
        got = solver.check_lsf_spread(ok)
        assert got == ok and (ok is None or isinstance(got, (int, str)))
    assert type(solver.check_lsf_spread(np.int64(7))) is int
    words = 'spread must be None, "auto" or an integer in 1..1024 '
    for bad, given in ((0, "0"), (1025, "1025"), (True, "True"), ("4", "'4'"), (2.0, "2.0")):
        with pytest.raises(ValueError) as e:
            solver.check_lsf_spread(bad)
        assert str(e.value) == words + f"({given} given)"
        with pytest.raises(ValueError) as e:
            solver._check_spread(bad, 1024)
        assert str(e.value) == words + f"({given} given)"
    # before a device or a remote is touched
    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: pytest.fail("the remote was touched"))
    good = request((6, 2, 1, 0, ""))
    for bad in (0, 1025, "x", 1.5, -1, True, "8"):
        with pytest.raises(ValueError, match=r'spread must be None, "auto" or an integer in 1\.\.1024'):
            solver.solve_vrp_lsf_batch([good], spread=bad)
        with pytest.raises(ValueError, match=r'spread must be None, "auto" or an integer in 1\.\.1024'):
            solver.solve_vrp("lsf", *good, spread=bad)
        with pytest.raises(ValueError, match="spread must be"):
            solver.batch_lsf_launch(None, [], 8, 3, 0, spread=bad)
    # the shared policy, min(S, max(1, 16 cus // R))
    for (R, S, cus), want in (((1, 64, 256), 64), ((1, 1024, 256), 1024), ((512, 64, 256), 8),
                              ((10000, 64, 256), 1), ((65, 64, 256), 63), ((2048, 64, 256), 2),
                              ((2049, 64, 256), 1), ((1, 1, 256), 1), ((100, 1024, 304), 48)):
        assert solver.batch_lsf_spread(R, S, cus) == want == solver.batch_lsr_spread(R, S, cus)


def _rows(cis):
    return ([list(range(ci.n, 0, -1)) + [0] * (len(ci.capacities) - 1) for ci in cis],
            [[0] * ci.n + [-2] * (len(ci.capacities) - 1) for ci in cis],
            [[10 * ci.n] + [0] * (len(ci.capacities) - 1) for ci in cis])


def test_the_launch_sees_the_spread_it_was_given(monkeypatch, lib):
    seen = []

    def launch(ctx, cis, *args, **kwargs):
        seen.append((len(cis), args, kwargs))
        return _rows(cis)

    monkeypatch.setattr(solver, "batch_lsf_launch", launch)
    monkeypatch.setattr(solver, "context", lambda dev=0: "ctx")
    monkeypatch.setattr(solver, "_remote", lambda: None)
    reqs = [request((6, 2, 1, x, "")) for x in range(3)]
    # with no spread the launch's keywords are what they were before it had one
    solver.solve_vrp_lsf_batch(reqs, starts=8, rounds=3, seed=5)
    solver.solve_vrp("lsf", *reqs[0], starts=9, rounds=2, seed=6)
    solver.solve_vrp("lsf", *reqs[0], starts=9, rounds=2, seed=6, spread=None)
    assert seen == [(3, (8, 3, 5, "sum"), {}), (1, (9, 2, 6, "sum"), {}), (1, (9, 2, 6, "sum"), {})]
    del seen[:]
    solver.solve_vrp_lsf_batch(reqs, starts=8, rounds=3, seed=5, spread=5)
    solver.solve_vrp_lsf_batch(reqs, starts=8, rounds=3, seed=5, spread=np.int64(6))
    solver.solve_vrp_lsf_batch(reqs[:1], starts=8, rounds=3, seed=5, objective="max", spread="auto")
    solver.solve_vrp("lsf", *reqs[0], starts=9, rounds=2, seed=6, spread=5)
    solver.solve_vrp("lsf", *reqs[0], starts=9, rounds=2, seed=6, spread=np.int64(6))
    solver.solve_vrp("lsf", *reqs[0], starts=9, rounds=2, seed=6, spread="auto")
    assert seen == [(3, (8, 3, 5, "sum"), {"spread": 5}), (3, (8, 3, 5, "sum"), {"spread": 6}),
                    (1, (8, 3, 5, "max"), {"spread": "auto"}), (1, (9, 2, 6, "sum"), {"spread": 5}),
                    (1, (9, 2, 6, "sum"), {"spread": 6}), (1, (9, 2, 6, "sum"), {"spread": "auto"})]
    assert all(type(kw["spread"]) in (int, str) for _, _, kw in seen)
    # only a number stays in the knobs a remote would get
    sent = []

    class Remote:
        def solve_vrp(self, algorithm, *request, **kw):
            sent.append((algorithm, {k: v for k, v in kw.items() if k in ("starts", "rounds", "spread")}))
            return {"durationMax": 1, "durationSum": 1, "vehicles": []}

    monkeypatch.setattr(solver, "_remote", lambda: Remote())
    for spread in (None, 5, np.int64(6), "auto"):
        solver.solve_vrp("lsf", *reqs[0], starts=9, rounds=2, spread=spread)
        solver.solve_vrp_lsf_batch(reqs[:1], starts=9, rounds=2, spread=spread)
    solver.solve_vrp("lsf", *reqs[0], starts=9, rounds=2)
    knobs = {"starts": 9, "rounds": 2}
    assert sent == [("lsf", knobs)] * 2 + [("lsf", dict(knobs, spread=5))] * 2 + \
        [("lsf", dict(knobs, spread=6))] * 2 + [("lsf", knobs)] * 3
    assert all(type(k.get("spread", 0)) is int for _, k in sent)


def test_batch_lsf_launch_chooses_the_kernels(monkeypatch, lib):
    """None and an "auto" of 1 are vrp_batch_lsf; a number, 1 included, is
    vrp_batch_lsf_spread at that number; "auto" asks the shared policy."""
    torch = pytest.importorskip("torch")
    calls = []

    class Ctx:
        dev = "cpu"
        cus = 256

        def _out(self, R):
            return (torch.zeros((R, 7), dtype=torch.int16), torch.zeros(R, dtype=torch.int64),
                    torch.zeros((R, 2), dtype=torch.int32), torch.zeros((R, 7), dtype=torch.int8), None)

        def vrp_batch_lsf(self, mats, *a, wide=None):
            calls.append(("lsf", mats.shape[0]) + a[3:])
            return self._out(mats.shape[0])

        def vrp_batch_lsf_spread(self, mats, *a, wide=None):
            calls.append(("spread", mats.shape[0]) + a[3:])
            return self._out(mats.shape[0])

    ci = solver.compact_vrp(*request((6, 2, 1, 0, "")))
    for R, spread in ((1, None), (1, 1), (1, 5), (1, "auto"), (300, "auto"), (2048, "auto"),
                      (2049, "auto")):
        solver.batch_lsf_launch(Ctx(), [ci] * R, 64, 9, 3, "sum", spread=spread)
    solver.batch_lsf_launch(Ctx(), [ci], 64, 9, 3, "max")
    assert calls == [("lsf", 1, 0, 64, 9, 3), ("spread", 1, 0, 64, 9, 3, 1), ("spread", 1, 0, 64, 9, 3, 5),
                     ("spread", 1, 0, 64, 9, 3, 64), ("spread", 300, 0, 64, 9, 3, 13),
                     ("spread", 2048, 0, 64, 9, 3, 2), ("lsf", 2049, 0, 64, 9, 3), ("lsf", 1, 1, 64, 9, 3)]


def test_inline_knob_reaches_the_solver(lib):
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append((algorithm, dict(knobs.get("inline") or {})))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    app = service.App(service.MemoryStore({}, {}, {}), solve=fake, batch_vrp_lsf=True,
                      batch_window_s=0.01, batch_vrp_lsf_launch=lambda key, cis: pytest.fail("batched"))
    assert app.vrp_lsf_batcher.spread is None
    for spread in (1, 4, 1024):   # a request that names it takes the unbatched path, with it
        st, _ = app.solve_inline("vrp", "lsf", _body((5, 2, 1, 1, ""), knobs={"spread": spread}))
        assert st == 200 and seen.pop() == ("lsf", {"spread": spread})
    for spread in (0, 1025, "auto", True):
        st, res = app.solve_inline("vrp", "lsf", _body((5, 2, 1, 1, ""), knobs={"spread": spread}))
        assert st == 400 and res["errors"][0]["what"] == "Invalid request", (spread, res)
    assert seen == []


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _lists(out):
    tours, keys, durs, veh, info = out
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), veh.cpu().tolist(), info.cpu().tolist())


def groups(S):
    """The workgroups per request a run of S starts is launched at: each of 1,
    2, 3, S - 1 and S inside 1..S once, then S + 1 and 1024, which the entry
    point clamps to S."""
    return sorted({G for G in (1, 2, 3, S - 1, S) if 1 <= G <= S}) + [S + 1, 1024]


def both(ctx, args, G_list, kernel="vrp_batch_lsf"):
    """The oracle launch and one spread launch per G on the same buffers, all
    five tensors equal -> the oracle's rows as lists."""
    import torch
    old = getattr(ctx, kernel)(*args)
    for G in G_list:
        new = getattr(ctx, kernel + "_spread")(*args, G)
        for x, (a, b) in enumerate(zip(old, new)):
            assert a.dtype == b.dtype and a.shape == b.shape, (G, x)
            assert torch.equal(a, b), (G, x, a.cpu().tolist(), b.cpu().tolist())
    return _lists(old)


def run_args(ctx, runs, objective):
    assert len({r[1:] for r in runs}) == 1
    return gpu_args(ctx, [r[0] for r in runs]) + (obj_id(objective), *runs[0][1:], SEED)


_ID = "n%d-K%d-H%d-s%d%s-S%d-r%d"


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", ALL_RUNS, ids=lambda r: _ID % (*r[0], *r[1:]))
def test_gpu_equals_vrp_batch_lsf_and_the_reference(ctx, run, objective):
    got = both(ctx, run_args(ctx, [run], objective), groups(run[1]))
    want = expected([run], objective)
    print(run, objective, groups(run[1]), "gpu", got, "ref", want)
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", SHARE_RUNS, ids=lambda r: _ID % (*r[0], *r[1:]))
def test_gpu_share_edges(ctx, run, objective):
    """L = 11, 12, 16 (ties) and 23 at G = 1 and G = S: idle threads, the first
    per = 2, equal keys across the record exchange, per = 4."""
    case, S, _ = run
    L = case[0] + case[1] - 1
    moves = 2 * L * (L - 1)
    assert (L, moves, -(-moves // 256)) in ((11, 220, 1), (12, 264, 2), (16, 480, 2), (23, 1012, 4))
    got = both(ctx, run_args(ctx, [run], objective), (1, S))
    want = expected([run], objective)
    print(run, objective, "gpu", got, "ref", want)
    assert got == want
    ref = reference(run, objective)
    assert sum(ref["rounds"]) > 0 and any(ref["plain"])      # moves were applied under the share


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_1024_starts_on_1024_workgroups(ctx, objective):
    case = (5, 2, 1, 77, "")
    got = both(ctx, gpu_args(ctx, [case]) + (obj_id(objective), 1024, 1000, SEED), (1024, 1023, 7))
    assert 0 <= got[4][0][0] < 1024 and got[0][0] < 2**64 - 1


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_seven_requests_one_of_them_refused(ctx, objective):
    """The six SIX requests and, at row 3, a copy of the first with a negative
    entry, which the staging check refuses, at G = 3: r = block / G and g =
    block % G.  Every row equals its one-request launch, the refused one is
    vrp_batch_lsf's."""
    import torch
    case, S, rounds = SIX[0]
    cases = [r[0] for r in SIX[:3]] + [case] + [r[0] for r in SIX[3:]]
    args = gpu_args(ctx, cases)
    mats = np.stack([inst(c)[0] for c in cases]).astype(np.int32)
    mats[3, 0, 3, 2] = -1
    tail = (obj_id(objective), S, rounds, SEED)
    for wide in (False, True):
        full = (torch.tensor(mats, dtype=torch.int32, device=ctx.dev),) + args[1:] + tail
        old = ctx.vrp_batch_lsf(*full, wide=wide)
        new = ctx.vrp_batch_lsf_spread(*full, 3, wide=wide)
        for x, (a, b) in enumerate(zip(old, new)):
            assert torch.equal(a, b), (wide, x)
        keys, tours, durs, veh, info = _lists(new)
        assert keys[3] == 2**64 - 1 and tours[3] == [0] * 12 and durs[3] == [0] * 3 and \
            veh[3] == [-1] * 12 and info[3] == [-1, 0]
        want = expected(SIX, objective)
        for x, at in enumerate((0, 1, 2, 4, 5, 6)):
            row = (keys[at], tours[at], durs[at], veh[at], info[at])
            assert row == tuple(w[x] for w in want), at
            alone = _lists(ctx.vrp_batch_lsf_spread(*gpu_args(ctx, [cases[at]]), *tail, 3, wide=wide))
            assert row == tuple(g[0] for g in alone), at
    # R = 0 returns empty tensors
    z = [torch.zeros(shape, dtype=torch.int32, device=ctx.dev)
         for shape in ((0, 1, 11, 11), (0, 11), (0, 3), (0, 3))]
    out = ctx.vrp_batch_lsf_spread(*z, obj_id(objective), 8, 5, SEED, 4)
    assert [tuple(t.shape) for t in out] == [(0, 12), (0,), (0, 3), (0, 12), (0, 2)]
    # an hour-indexed batch is refused at the entry point
    hours = [torch.ones(shape, dtype=torch.int32, device=ctx.dev)
             for shape in ((1, 24, 6, 6), (1, 6), (1, 2), (1, 2))]
    with pytest.raises(_lib.VrpmsError, match=r"vrpms_vrp_batch_lsf_spread: H must be 1 \(24 given\)"):
        ctx.vrp_batch_lsf_spread(*hours, obj_id(objective), 8, 5, SEED, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_all_roomy_is_vrp_batch_lsr_spread(ctx, objective):
    """Every capacity carries the total demand: every tour is plain and the
    rows are A26's, by either mapping."""
    import torch
    for case, S, rounds in ROOMY:
        args = gpu_args(ctx, [case]) + (obj_id(objective), S, rounds, SEED)
        lsr = ctx.vrp_batch_lsr_spread(*args, 3)
        for G in (1, 3):
            lsf = ctx.vrp_batch_lsf_spread(*args, G)
            for x in range(5):
                assert torch.equal(lsr[x], lsf[x]), (case, G, x)


@pytest.mark.gpu
def test_gpu_lds_edge(ctx):
    """The largest N of A28's domain table launches by the spread mapping too.
    The entry point itself, which needs 8 align8(L) - 64 bytes fewer, takes a
    few nodes more -- there A26's kernel, which fits more still, says what the
    all-roomy row is -- and refuses the first N past its own bytes with the
    byte count, nothing written."""
    import torch
    lib, K, R, G = ctx.lib, 4, 2, 2
    N = DOMAIN[(K, False)]
    cases = [(N - 1, K, 1, 40 + x, "allroomy") for x in range(R)]
    for objective in OBJECTIVES:
        both(ctx, gpu_args(ctx, cases) + (obj_id(objective), 2, 1, SEED), (G,))
    N = min(N for N in range(N + 1, 400) if spread_lds_bytes(N, K, False) > LDS_BYTES)
    assert spread_lds_bytes(N - 1, K, False) <= LDS_BYTES < lds_bytes(N - 1, K, False)
    cases = [(N - 2, K, 1, 40 + x, "allroomy") for x in range(R)]
    for objective in OBJECTIVES:
        lsr = ctx.vrp_batch_lsr(*gpu_args(ctx, cases), obj_id(objective), 2, 1, SEED)
        lsf = ctx.vrp_batch_lsf_spread(*gpu_args(ctx, cases), obj_id(objective), 2, 1, SEED, G)
        assert all(torch.equal(a, b) for a, b in zip(lsr, lsf))
    L = N - 1 + K - 1
    M = torch.ones((R, 1, N, N), dtype=torch.int32, device=ctx.dev)
    dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
    cp = torch.ones((R, K), dtype=torch.int32, device=ctx.dev)
    wb = work_bytes(R, N, K, G)
    work = torch.full((wb,), -7, dtype=torch.int8, device=ctx.dev)
    tours = torch.full((R, L), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R, K), -7, dtype=torch.int32, device=ctx.dev)
    veh = torch.full((R, L), -7, dtype=torch.int8, device=ctx.dev)
    info = torch.full((R, 2), -7, dtype=torch.int32, device=ctx.dev)
    rc = lib.vrpms_vrp_batch_lsf_spread(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(),
                                        cp.data_ptr(), R, N, K, 1, 0, 0, 4, 1, SEED, G, work.data_ptr(),
                                        wb, tours.data_ptr(), keys.data_ptr(), durs.data_ptr(),
                                        veh.data_ptr(), info.data_ptr(), ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_lsf_spread:" in msg and b"bytes of LDS" in msg
    assert str(spread_lds_bytes(N, K, False)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item() and (work == -7).all().item()
    assert (durs == -7).all().item() and (veh == -7).all().item() and (info == -7).all().item()


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_and_solve_vrp_lsf_batch_with_a_spread(objective):
    S, rounds = 8, 1000
    D7, locs7, caps7, starts7 = request((6, 2, 1, 50, ""), 100)
    reqs = [request((6, 2, 1, 51, "")), request((9, 3, 1, 52, "")),
            (D7, locs7, caps7, starts7, [100 + i for i in range(1, 7)]),            # none active
            request((6, 2, 1, 53, "")),
            {"durations": D7, "locations": locs7, "capacities": caps7, "start_times": starts7,
             "ignored_customers": [103]},
            request((9, 3, 1, 54, ""))]
    kw = dict(starts=S, rounds=rounds, seed=SEED, objective=objective, with_unvisited=True)
    default = solver.solve_vrp_lsf_batch(reqs, **kw)
    for spread in (None, 1, 4, "auto"):
        assert solver.solve_vrp_lsf_batch(reqs, spread=spread, **kw) == default, spread
        for x in (0, 1, 2, 5):
            assert solver.solve_vrp("lsf", *reqs[x], spread=spread, **kw) == default[x], (spread, x)


def _post(port, case, **kw):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/solve/vrp/lsf", data=_body(case, **kw),
                                 method="POST")
    with urllib.request.urlopen(req, timeout=120) as resp:
        return resp.status, json.loads(resp.read())


@pytest.mark.gpu
def test_service_inline_spread_over_http_gives_the_same_body():
    S = 8
    cases = [(6, 2, 1, 61, ""), (9, 3, 1, 52, "")]
    app = service.App(service.MemoryStore({}, {}, {}), seed=SEED)
    srv = service.serve(app, "127.0.0.1", 0)
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    try:
        port = srv.server_address[1]
        knob = [_post(port, c, knobs={"spread": 4, "starts": S}, seed=SEED) for c in cases]
        noknob = [_post(port, c, knobs={"starts": S}, seed=SEED) for c in cases]
    finally:
        srv.shutdown()
        srv.server_close()
        th.join()
    for x, case in enumerate(cases):
        st, body = noknob[x]
        assert st == 200 and body["success"]
        assert knob[x] == (200, body)
