"""The local search over separator tours (spec A26) by its second mapping
(DESIGN.md §4.3r): the C entry points vrpms_vrp_batch_lsr_spread_lds /
vrpms_vrp_batch_lsr_spread_work / vrpms_vrp_batch_lsr_spread,
Context.vrp_batch_lsr_spread, solver.batch_lsr_spread and the `spread` argument
of batch_lsr_launch / solve_vrp_lsr_batch / solve_vrp("lsr"), the inline knob
"spread" and the service's --batch-lsr-spread.

The mapping is free under A26, so there is no new reference: per request the
GPU must return the identical key, tour, route durations, vehicle row and info
row as tests/test_vrp_batch_lsr.py's a26_ref, and as vrp_batch_lsr itself, for
every number of workgroups per request."""
import ctypes
import functools
import json
import threading
import urllib.request

import numpy as np
import pytest

from oracle import spec
from test_vrp_batch_ga import _FakeApp, _body, _no_gpu
from test_vrp_batch_ls import LDS_BYTES, M32, OBJECTIVES, SEED, all_moves, obj_id, pad, request
from test_vrp_batch_lsr import (ALL_RUNS, DOMAIN, GRID_N, R_EDGES, S_EDGES, SIX, TIES, _fake_launch,
                                expected, gpu_args, inst, lds_bytes, reference)
from vrpms_amd import _lib, core, service, solver

# the runs this file adds: (case, S, rounds).  Under the 256-thread share a
# round of L tokens has 2 L (L - 1) moves, per = ceil(moves / 256) a thread
IDLE = ((9, 3, 1, 1, ""), 8, 1000)         # L = 11: 220 moves, 36 idle threads
PER2 = ((10, 3, 1, 1, ""), 8, 1000)        # L = 12: 264 moves, the first per = 2
TIES_A = ((13, 4, 1, 1, "ties"), 6, 1000)  # L = 16: 480 moves, per = 2
TIES_B = ((13, 4, 24, 2, "ties"), 6, 1000)
PER4 = ((20, 4, 24, 1, ""), 4, 1000)       # L = 23: 1012 moves, per = 4
NEW_RUNS = [IDLE, PER2, TIES_A, TIES_B, PER4]


def spread_lds_bytes(N, K, H, wide):
    """DESIGN.md §4.3r restated: the instance as vrp_batch_lsr keeps it, one
    tour row per wavefront and two sets of four 16-byte round records."""
    return pad(H * N * N * (4 if wide else 2), 16) + 4 * pad(N, 4) + 2 * 4 * pad(K, 4) + \
        4 * 2 * pad(N - 1 + K - 1, 8) + 2 * 4 * 16


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
def test_lds_is_at_most_vrp_batch_lsr_s(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_vrp_batch_lsr_spread_lds
    for H in (1, 24):
        for wide in (0, 1):
            for K in (1, 3, 4, 64):
                for N in GRID_N:
                    assert f(N, K, H, wide, ctypes.byref(b)) == _lib.VRPMS_OK
                    assert b.value == spread_lds_bytes(N, K, H, wide) == \
                        core.vrp_batch_lsr_spread_lds(N, K, H, wide)
                    assert b.value <= core.vrp_batch_lsr_lds(N, K, H, wide) == lds_bytes(N, K, H, wide)
    # the smallest tour row is where the two meet
    assert core.vrp_batch_lsr_spread_lds(2, 1, 1, False) == core.vrp_batch_lsr_lds(2, 1, 1, False)
    # at A26's own edges
    for (H, wide), N in DOMAIN.items():
        assert core.vrp_batch_lsr_spread_lds(N, 4, H, wide) <= core.vrp_batch_lsr_lds(N, 4, H, wide) \
            <= LDS_BYTES
    # the same refusals, the same codes
    for args, word in (((1, 3, 1, 0), b"2 <= N"), ((0, 3, 1, 0), b"2 <= N"),
                       ((65536, 3, 1, 0), b"2 <= N"),
                       ((5, 0, 1, 0), b"1 <= K <= 64"), ((5, 65, 1, 0), b"1 <= K <= 64"),
                       ((65535, 3, 1, 0), b"N + K - 2 <= 65535 (65536 given)"),
                       ((65474, 64, 1, 0), b"N + K - 2 <= 65535 (65536 given)"),
                       ((5, 3, 2, 0), b"H must be 1 or 24"), ((5, 3, 0, 0), b"H must be 1 or 24"),
                       ((5, 3, 1, 2), b"wide"), ((5, 3, 1, -1), b"wide")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        assert lib.vrpms_vrp_batch_lsr_lds(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL
        assert word in lib.vrpms_last_error()
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsr_spread_lds" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(65535, 2, 1, 0, ctypes.byref(b)) == _lib.VRPMS_OK
    assert f(5, 3, 1, 0, None) == _lib.VRPMS_EINVAL
    assert b"vrpms_vrp_batch_lsr_spread_lds: bytes is NULL" in lib.vrpms_last_error()
    with pytest.raises(_lib.VrpmsError, match="1 <= K <= 64"):
        core.vrp_batch_lsr_spread_lds(5, 65, 1, False)


def test_workspace_bytes(lib):
    b = ctypes.c_uint64()
    f = lib.vrpms_vrp_batch_lsr_spread_work
    for R in (0, 1, 3, 10000):
        for N, K in ((2, 1), (5, 2), (8, 3), (9, 1), (10, 1), (58, 4), (281, 4), (3, 64)):
            for G in (1, 2, 64, 1024, 65535):
                assert f(R, N, K, G, ctypes.byref(b)) == _lib.VRPMS_OK
                assert b.value == work_bytes(R, N, K, G) == core.vrp_batch_lsr_spread_work(R, N, K, G)
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
                       ((32769, 5, 2, 65535), b"above 2^31 - 1")):
        b.value = 77
        assert f(*args, ctypes.byref(b)) == _lib.VRPMS_EINVAL, args
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsr_spread_work" in msg and word in msg, (args, msg)
        assert b.value == 77
    assert f(1, 5, 2, 1, None) == _lib.VRPMS_EINVAL
    assert b"bytes is NULL" in lib.vrpms_last_error()


def test_argument_errors_need_no_gpu(lib):
    """As tests/test_vrp_batch_lsr.py's: every argument check comes before the
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
        return lib.vrpms_vrp_batch_lsr_spread(ctx, a["m"], a["d"], a["cp"], a["st"], R, N, K, H, obj,
                                              wide, S, rounds, 12345, G, work, wb, a["t"], a["k"],
                                              a["du"], a["v"], a["i"], None)

    def refused(word, **kw):
        assert f(**kw) == _lib.VRPMS_EINVAL, kw
        msg = lib.vrpms_last_error()
        assert b"vrpms_vrp_batch_lsr_spread:" in msg and word in msg, (kw, msg)

    # the existing entry point's
    refused(b"ctx is NULL", ctx=None)
    refused(b"R must not be negative", R=-1)
    for N in (-1, 0, 1, 65536):
        refused(b"2 <= N", N=N)
    for K in (-1, 0, 65, 1000):
        refused(b"1 <= K <= 64", K=K)
    refused(b"N + K - 2 <= 65535 (65536 given)", N=65535, K=3)
    for H in (0, 2, 12, 25):
        refused(b"H must be 1 or 24", H=H)
    for obj in (-1, 2):
        refused(b"objective", obj=obj)
    for wide in (-1, 2):
        refused(b"wide", wide=wide)
    for S in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= S <= 65535 (%d given)" % S, S=S)
    refused(b"rounds must not be negative (-1 given)", rounds=-1)
    for name in names:
        refused(b"NULL", **{name: None})
    refused(b"H must be 1 or 24", R=0, H=3)
    refused(b"1 <= S <= 65535", R=0, S=0)
    # the new ones
    for G in (-1, 0, 65536, 1 << 20):
        refused(b"1 <= G <= 65535 (%d given)" % G, G=G)
    refused(b"1 <= G <= 65535", R=0, G=0)
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
    for N, K, H, wide in ((5, 2, 1, 0), (58, 4, 24, 0), (59, 4, 24, 1), (5, 1, 1, 0)):
        refused(b"needs %d bytes of LDS (0 available)" % spread_lds_bytes(N, K, H, wide), N=N, K=K,
                H=H, wide=wide)
    assert f(R=0) == _lib.VRPMS_OK
    assert f(R=0, G=65535, work=None, wb=0, **{name: None for name in names}) == _lib.VRPMS_OK
    assert buf.raw == bytes(1 << 16) and fake.raw == bytes(1 << 16)


def test_auto_policy_table():
    assert solver.BATCH_LSR_MAX_SPREAD == 1024
    # min(S, max(1, 16 cus // R)): the factor 16 is DESIGN.md §4.3r's, measured
    for (R, S, cus), want in (((1, 64, 256), 64), ((1, 1024, 256), 1024), ((16, 64, 256), 64),
                              ((512, 64, 256), 8), ((10000, 64, 256), 1), ((3, 64, 256), 64),
                              ((64, 64, 256), 64), ((65, 64, 256), 63), ((2048, 64, 256), 2),
                              ((2049, 64, 256), 1), ((4096, 64, 256), 1), ((1, 1, 256), 1),
                              ((100, 1024, 304), 48)):
        assert solver.batch_lsr_spread(R, S, cus) == want, (R, S, cus)


def test_spread_values_are_checked_before_a_device_is_touched(monkeypatch, lib):
    _no_gpu(monkeypatch)
    monkeypatch.setattr(solver, "_remote", lambda: pytest.fail("the remote was touched"))
    good = request((6, 2, 1, 0, ""))
    for bad in (0, 1025, "x", 1.5, -1, True, "8"):
        with pytest.raises(ValueError, match=r'spread must be None, "auto" or an integer in 1\.\.1024'):
            solver.solve_vrp_lsr_batch([good], spread=bad)
        with pytest.raises(ValueError, match=r'spread must be None, "auto" or an integer in 1\.\.1024'):
            solver.solve_vrp("lsr", *good, spread=bad)
        with pytest.raises(ValueError, match="spread must be"):
            solver.batch_lsr_launch(None, [], 8, 3, 0, spread=bad)
        with pytest.raises(ValueError, match="spread must be"):
            service.VrpLsrBatcher(_FakeApp(), launch=_fake_launch([]), spread=bad)
    for ok in (None, "auto", 1, 4, 1024, np.int64(7)):
        assert solver.check_lsr_spread(ok) == ok
        assert service.VrpLsrBatcher(_FakeApp(), launch=_fake_launch([]), spread=ok).spread == ok
    assert service.VrpLsrBatcher(_FakeApp(), launch=_fake_launch([])).spread is None


def test_the_launch_sees_the_spread_it_was_given(monkeypatch, lib):
    seen = []

    def launch(ctx, cis, starts, rounds, seed, objective="sum", spread=None):
        seen.append((len(cis), starts, rounds, seed, objective, spread))
        rows = _fake_launch([])(None, cis)
        return rows[0], [v for v, _ in rows[1]], [d for _, d in rows[1]]

    monkeypatch.setattr(solver, "batch_lsr_launch", launch)
    monkeypatch.setattr(solver, "context", lambda dev=0: "ctx")
    monkeypatch.setattr(solver, "_remote", lambda: None)
    reqs = [request((6, 2, 1, x, "")) for x in range(3)]
    solver.solve_vrp_lsr_batch(reqs, starts=8, rounds=3, seed=5)
    solver.solve_vrp_lsr_batch(reqs, starts=8, rounds=3, seed=5, spread="auto")
    solver.solve_vrp_lsr_batch(reqs[:1], starts=8, rounds=3, seed=5, objective="max", spread=7)
    solver.solve_vrp("lsr", *reqs[0], starts=9, rounds=2, seed=6)
    solver.solve_vrp("lsr", *reqs[0], starts=9, rounds=2, seed=6, spread=1024)
    solver.solve_vrp("lsr", *reqs[0], starts=9, rounds=2, seed=6, spread="auto")
    assert seen == [(3, 8, 3, 5, "sum", None), (3, 8, 3, 5, "sum", "auto"), (1, 8, 3, 5, "max", 7),
                    (1, 9, 2, 6, "sum", None), (1, 9, 2, 6, "sum", 1024), (1, 9, 2, 6, "sum", "auto")]
    # the batcher launches with the app's
    del seen[:]
    for spread in (None, "auto", 16):
        b = service.VrpLsrBatcher(_FakeApp(), starts=8, rounds=3, spread=spread)
        ci = solver.compact_vrp(*reqs[0])
        b._gpu_launch((7, 2, 1, False, "max"), [ci, ci])
    assert seen == [(2, 8, 3, 0, "max", None), (2, 8, 3, 0, "max", "auto"), (2, 8, 3, 0, "max", 16)]


def test_batch_lsr_launch_chooses_the_kernels(monkeypatch, lib):
    """None and an "auto" of 1 are vrp_batch_lsr; a number, 1 included, is
    vrp_batch_lsr_spread at that number; "auto" asks batch_lsr_spread."""
    torch = pytest.importorskip("torch")
    calls = []

    class Ctx:
        dev = "cpu"
        cus = 256

        def _out(self, R):
            return (torch.zeros((R, 7), dtype=torch.int16), torch.zeros(R, dtype=torch.int64),
                    torch.zeros((R, 2), dtype=torch.int32), torch.zeros((R, 7), dtype=torch.int8), None)

        def vrp_batch_lsr(self, mats, *a, wide=None):
            calls.append(("lsr", mats.shape[0]) + a[3:])
            return self._out(mats.shape[0])

        def vrp_batch_lsr_spread(self, mats, *a, wide=None):
            calls.append(("spread", mats.shape[0]) + a[3:])
            return self._out(mats.shape[0])

    ci = solver.compact_vrp(*request((6, 2, 1, 0, "")))
    for R, spread in ((1, None), (1, 1), (1, 5), (1, "auto"), (16, "auto"), (300, "auto"),
                      (2048, "auto"), (2049, "auto")):
        solver.batch_lsr_launch(Ctx(), [ci] * R, 64, 9, 3, "sum", spread=spread)
    assert calls == [("lsr", 1, 0, 64, 9, 3), ("spread", 1, 0, 64, 9, 3, 1), ("spread", 1, 0, 64, 9, 3, 5),
                     ("spread", 1, 0, 64, 9, 3, 64), ("spread", 16, 0, 64, 9, 3, 64),
                     ("spread", 300, 0, 64, 9, 3, 13), ("spread", 2048, 0, 64, 9, 3, 2),
                     ("lsr", 2049, 0, 64, 9, 3)]


def test_inline_knob_and_cli_flag(monkeypatch, capsys, lib):
    seen = []

    def fake(problem, algorithm, params, knobs, locations, durations):
        seen.append(dict(knobs.get("inline") or {}))
        return {"durationMax": 2, "durationSum": 3, "vehicles": []}

    assert service.INLINE_KNOBS["spread"] is int and service.KNOB_RANGES["spread"] == (1, 1024)
    launched = []
    app = service.App(service.MemoryStore({}, {}, {}), solve=fake, batch_vrp_lsr=True,
                      batch_window_s=0.01, batch_vrp_lsr_launch=_fake_launch(launched),
                      batch_lsr_spread="auto")
    assert app.vrp_lsr_batcher.spread == "auto"
    body = functools.partial(_body, (5, 2, 1, 1, ""))
    for spread in (1, 4, 1024):   # a request that names it takes the unbatched path, with it
        st, _ = app.solve_inline("vrp", "lsr", body(knobs={"spread": spread}))
        assert st == 200 and seen.pop() == {"spread": spread} and launched == []
    for spread in (0, 1025, -1, "auto", None, True, [4]):
        st, res = app.solve_inline("vrp", "lsr", body(knobs={"spread": spread}))
        assert st == 400 and res["errors"][0]["what"] == "Invalid request", (spread, res)
    assert seen == [] and launched == []
    # the forwarding table of vrpms_amd.remote is INLINE_KNOBS
    from vrpms_amd import remote
    out = {}
    remote._options(out, 1, None, {"spread": 4, "starts": 8})
    assert out["knobs"] == {"spread": 4, "starts": 8}

    made = {}

    class Stop(Exception):
        pass

    def stop(store, **kw):
        made.update(kw)
        raise Stop

    monkeypatch.setattr(service, "App", stop)
    for argv, want in (([], None), (["--batch-lsr-spread", "auto"], "auto"),
                       (["--batch-lsr-spread", "1"], 1), (["--batch-lsr-spread", "1024"], 1024)):
        with pytest.raises(Stop):
            service.main(argv)
        assert made["batch_lsr_spread"] == want and made["batch_lsr_spread"].__class__ is want.__class__
    for bad in ("0", "1025", "x", "1.5", "Auto", ""):
        with pytest.raises(SystemExit):
            service.main(["--batch-lsr-spread", bad])
    capsys.readouterr()


@functools.lru_cache(maxsize=None)
def rounds_under_the_share(run, objective):
    """a26_ref's descents once more, noting what the 256-thread share makes of
    every round: thread t prices the ids [t per, (t + 1) per), wavefront
    t // 64 -> dict(L, moves, per, won = the wavefronts whose share held an
    applied move, cross = the rounds whose least key sat on moves of different
    wavefronts that give different tours, key, s, tour)."""
    case, S, rounds = run
    D, dem, caps, starts = inst(case)
    D = spec.as_3d(D)
    n = D.shape[1] - 1
    skey = spec.seed_key(SEED)
    caps, starts, obj = list(caps), list(starts), obj_id(objective)
    L = n + len(caps) - 1
    moves = all_moves(L)
    per = -(-len(moves) // 256)
    wave = [(x // per) // 64 for x in range(len(moves))]
    won, cross, ends = set(), 0, []
    for s in range(S):
        p = list(range(1, n + 1))
        for q in range(n - 1, 0, -1):
            j = spec.philox4x32_10((M32, M32, s, q), skey)[0] % (q + 1)
            p[q], p[j] = p[j], p[q]
        t = spec.pack_separators(p, len(caps) - 1, dem, caps)
        k = int(spec.eval_cvrp_batch(D, [t], dem, caps, starts, obj)[0][0])
        applied = 0
        while L >= 2 and applied < rounds:
            cands = [spec.apply_move(t, *m) for m in moves]
            keys = [int(x) for x in spec.eval_cvrp_batch(D, cands, dem, caps, starts, obj)[0]]
            kmin = min(keys)
            if not kmin < k:
                break
            at = keys.index(kmin)
            won.add(wave[at])
            cross += any(kk == kmin and wave[x] != wave[at] and cand != cands[at]
                         for x, (kk, cand) in enumerate(zip(keys, cands)))
            t, k = cands[at], kmin
            applied += 1
        ends.append((k, s, t))
    k, s, t = min(ends, key=lambda e: e[:2])
    return dict(L=L, moves=len(moves), per=per, won=won, cross=cross, key=k, s=s, tour=t)


def test_reference_properties_under_the_256_thread_share(lib):
    """What the GPU cases claim to exercise, checked on the reference: the share
    is vrpms_vrp_batch_lsr_spread's (batch_ls_share_wg), per = ceil(moves / 256)."""
    assert lib.vrpms_vrp_batch_lsr_spread is not None
    got = {(run, o): rounds_under_the_share(run, o) for run in NEW_RUNS + TIES for o in OBJECTIVES}
    for (run, o), r in got.items():   # the same descents as a26_ref's
        ref = reference(run, o)
        assert (r["key"], r["s"], r["tour"]) == (ref["key"], ref["s"], ref["tour"]), (run, o)
    shape = {run: (got[(run, "sum")]["L"], got[(run, "sum")]["moves"], got[(run, "sum")]["per"])
             for run in NEW_RUNS + TIES}
    assert shape[IDLE] == (11, 220, 1) and 256 - 220 == 36
    assert shape[PER2] == (12, 264, 2)
    assert 2 * 11 * 10 <= 256 < 2 * 12 * 11          # L = 12 is the first per = 2
    assert shape[TIES_A] == shape[TIES_B] == (16, 480, 2)
    assert shape[PER4] == (23, 1012, 4)
    assert [shape[run] for run in TIES] == [(8, 112, 1)] * 2
    # per = 4 on L = 23: a thread's four ids straddle the swap / 2-opt and the
    # 2-opt / relocate boundaries (253 and 506 are no multiples of 4)
    tri = 23 * 22 // 2
    assert tri % 4 and (2 * tri) % 4
    # the winning move lay in every wavefront's share at some round
    for o in OBJECTIVES:
        assert got[(TIES_A, o)]["won"] == {0, 1, 2, 3}
        assert got[(PER4, o)]["won"] == {0, 1, 2, 3}
    # rounds whose least key sat on moves of different wavefronts that give
    # different tours: the (key, wavefront) choice is put to the test
    assert [got[(TIES_A, o)]["cross"] for o in OBJECTIVES] == [11, 11]
    assert sorted(got[(TIES_B, o)]["cross"] for o in OBJECTIVES) == [12, 16]
    assert [got[(TIES[0], o)]["cross"] for o in OBJECTIVES] == [8, 8]
    assert sorted(got[(TIES[1], o)]["cross"] for o in OBJECTIVES) == [4, 5]
    # info's capped count sums over the groups: R_EDGES cap some descents
    assert [reference(run, "sum")["capped"] for run in R_EDGES][0] == 7
    assert 0 < reference(R_EDGES[2], "sum")["capped"] <= reference(R_EDGES[1], "sum")["capped"]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _lists(out):
    tours, keys, durs, veh, info = out
    return ([int(k) & (2**64 - 1) for k in keys.cpu().tolist()], tours.cpu().tolist(),
            durs.cpu().tolist(), veh.cpu().tolist(), info.cpu().tolist())


def gpu_spread(ctx, cases, objective, S, rounds, G, wide=None):
    """One vrp_batch_lsr_spread launch -> ([key], [tour], [durs], [veh], [info])."""
    return _lists(ctx.vrp_batch_lsr_spread(*gpu_args(ctx, cases), obj_id(objective), S, rounds, SEED, G,
                                           wide=wide))


def gpu_runs(ctx, runs, objective, G, wide=None):
    assert len({r[1:] for r in runs}) == 1 and len(runs) <= 16
    return gpu_spread(ctx, [r[0] for r in runs], objective, *runs[0][1:], G, wide=wide)


_ID = "n%d-K%d-H%d-s%d%s-S%d-r%d"


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", ALL_RUNS, ids=lambda r: _ID % (*r[0], *r[1:]))
def test_gpu_equals_reference_on_the_existing_runs(ctx, run, objective):
    want = expected([run], objective)
    for G in (1, 3):
        got = gpu_runs(ctx, [run], objective, G)
        print(run, objective, G, "gpu", got, "ref", want)
        assert got == want, G


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("run", NEW_RUNS, ids=lambda r: _ID % (*r[0], *r[1:]))
def test_gpu_equals_reference_on_the_new_runs(ctx, run, objective):
    want = expected([run], objective)
    for G in (1, 2, run[1]):
        got = gpu_runs(ctx, [run], objective, G)
        print(run, objective, G, "gpu", got, "ref", want)
        assert got == want, G


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_group_edges(ctx, objective):
    """The clamp to min(G, S), the ragged last stride, and the capped count
    summed over the groups."""
    for run in S_EDGES:
        S = run[1]
        want = expected([run], objective)
        for G in sorted({1, 2, 3, 4, 5, S, S + 1, 64}):
            assert gpu_runs(ctx, [run], objective, G) == want, (S, G)
    for run in R_EDGES:
        want = expected([run], objective)
        assert gpu_runs(ctx, [run], objective, 3) == want, run
    assert expected([R_EDGES[0]], objective)[4] == [[expected([R_EDGES[0]], objective)[4][0][0], 7]]


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_equals_vrp_batch_lsr(ctx, objective):
    """No oracle involved: all five tensors of the two mappings are equal."""
    import torch
    case, S, rounds = SIX[0]

    def both(cases, G):
        args = gpu_args(ctx, cases) + (obj_id(objective), S, rounds, SEED)
        old = ctx.vrp_batch_lsr(*args)
        new = ctx.vrp_batch_lsr_spread(*args, G)
        for x, (a, b) in enumerate(zip(old, new)):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (len(cases), G, x)
        return new

    six = [r[0] for r in SIX]
    for G in (1, 2, 5, 16, 64):
        first = both(six, G)
        again = ctx.vrp_batch_lsr_spread(*gpu_args(ctx, six), obj_id(objective), S, rounds, SEED, G)
        assert all(torch.equal(a, b) for a, b in zip(first, again))     # two launches are identical
    order = [5, 4, 3, 2, 1, 0, 5, 0, 3, 3, 1, 4]
    both([six[x] for x in order], 3)
    company = [SIX[1 + x % 5][0] for x in range(301)]                   # R = 301, one request at row 300
    company[300] = case
    for G in (1, 4):
        out = both(company, G)
        alone = both([case], G)
        assert all(torch.equal(a[300], b[0]) for a, b in zip(out, alone))
    # R = 0 returns empty tensors
    z = [torch.zeros(shape, dtype=torch.int32, device=ctx.dev)
         for shape in ((0, 24, 11, 11), (0, 11), (0, 3), (0, 3))]
    out = ctx.vrp_batch_lsr_spread(*z, obj_id(objective), 8, 5, SEED, 4)
    assert [tuple(t.shape) for t in out] == [(0, 12), (0,), (0, 3), (0, 12), (0, 2)]
    assert [t.dtype for t in out] == [t.dtype for t in ctx.vrp_batch_lsr(*z, obj_id(objective), 8, 5, SEED)]


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_gpu_staging_width_and_refusals(ctx, objective):
    """All four instantiations, (uint16 | int32) x (H = 1 | 24), and the
    refusal row between two healthy requests, at G = 1 and G = 3."""
    import torch
    S, rounds = 6, 1000
    for H in (1, 24):
        a, b, c = (7, 3, H, 30, ""), (7, 3, H, 31, "e65535"), (7, 3, H, 32, "")
        over = (7, 3, H, 31, "e65536")

        def runs(*cases):
            return [(x, S, rounds) for x in cases]

        for G in (1, 3):
            assert gpu_runs(ctx, runs(a, b, c), objective, G, wide=False) == \
                expected(runs(a, b, c), objective)
            assert gpu_runs(ctx, runs(a, over, c), objective, G, wide=True) == \
                expected(runs(a, over, c), objective)
            assert gpu_runs(ctx, runs(over), objective, G) == expected(runs(over), objective)
            want = expected(runs(a, over, c), objective)
            keys, tours, durs, veh, info = gpu_runs(ctx, runs(a, over, c), objective, G, wide=False)
            assert keys[1] == 2**64 - 1 and tours[1] == [0] * 9 and durs[1] == [0] * 3 and \
                veh[1] == [-1] * 9 and info[1] == [-1, 0]
            for x in (0, 2):
                assert (keys[x], tours[x], durs[x], veh[x], info[x]) == tuple(w[x] for w in want)
            # a negative entry, under either width
            insts = [inst(x) for x in (a, b, c)]
            mats = np.stack([D for D, _, _, _ in insts]).astype(np.int32)
            mats[1, H - 1, 3, 2] = -1
            args = gpu_args(ctx, (a, b, c))
            want = expected(runs(a, b, c), objective)
            for wide in (False, True):
                keys, tours, durs, veh, info = _lists(ctx.vrp_batch_lsr_spread(
                    torch.tensor(mats, dtype=torch.int32, device=ctx.dev), *args[1:],
                    obj_id(objective), S, rounds, SEED, G, wide=wide))
                assert keys[1] == 2**64 - 1 and tours[1] == [0] * 9 and durs[1] == [0] * 3 and \
                    veh[1] == [-1] * 9 and info[1] == [-1, 0]
                for x in (0, 2):
                    assert (keys[x], tours[x], durs[x], veh[x], info[x]) == tuple(w[x] for w in want)


@pytest.mark.gpu
def test_gpu_lds_edge(ctx):
    import torch
    lib, K, H, R, G = ctx.lib, 4, 24, 2, 2
    N = DOMAIN[(H, False)]
    assert N == 58
    runs = [((N - 1, K, H, 40 + x, ""), 4, 1) for x in range(R)]
    for objective in OBJECTIVES:
        assert gpu_runs(ctx, runs, objective, G) == expected(runs, objective)
    N += 1
    L = N - 1 + K - 1
    M = torch.ones((R, H, N, N), dtype=torch.int32, device=ctx.dev)
    dm = torch.ones((R, N), dtype=torch.int32, device=ctx.dev)
    cp = torch.ones((R, K), dtype=torch.int32, device=ctx.dev)
    wb = work_bytes(R, N, K, G)
    work = torch.full((wb,), -7, dtype=torch.int8, device=ctx.dev)
    tours = torch.full((R, L), -7, dtype=torch.int16, device=ctx.dev)
    keys = torch.full((R,), -7, dtype=torch.int64, device=ctx.dev)
    durs = torch.full((R, K), -7, dtype=torch.int32, device=ctx.dev)
    veh = torch.full((R, L), -7, dtype=torch.int8, device=ctx.dev)
    info = torch.full((R, 2), -7, dtype=torch.int32, device=ctx.dev)
    rc = lib.vrpms_vrp_batch_lsr_spread(ctx.handle, M.data_ptr(), dm.data_ptr(), cp.data_ptr(),
                                        cp.data_ptr(), R, N, K, H, 0, 0, 4, 1, SEED, G, work.data_ptr(),
                                        wb, tours.data_ptr(), keys.data_ptr(), durs.data_ptr(),
                                        veh.data_ptr(), info.data_ptr(), ctx.stream())
    assert rc == _lib.VRPMS_EINVAL
    msg = lib.vrpms_last_error()
    assert b"vrpms_vrp_batch_lsr_spread:" in msg and b"bytes of LDS" in msg
    assert str(spread_lds_bytes(N, K, H, False)).encode() in msg
    torch.cuda.synchronize(ctx.dev)
    assert (tours == -7).all().item() and (keys == -7).all().item() and (work == -7).all().item()
    assert (durs == -7).all().item() and (veh == -7).all().item() and (info == -7).all().item()


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solve_vrp_and_solve_vrp_lsr_batch_with_a_spread(objective):
    S, rounds = 8, 1000
    D7, locs7, caps7, starts7 = request((6, 2, 24, 50, ""), 100)
    reqs = [request((6, 2, 24, 51, "")), request((9, 3, 1, 52, "")),
            (D7, locs7, caps7, starts7, [100 + i for i in range(1, 7)]),            # none active
            request((6, 2, 24, 53, "")),
            {"durations": D7, "locations": locs7, "capacities": caps7, "start_times": starts7,
             "ignored_customers": [103]},
            request((9, 3, 1, 54, ""))]
    kw = dict(starts=S, rounds=rounds, seed=SEED, objective=objective, with_unvisited=True)
    default = solver.solve_vrp_lsr_batch(reqs, **kw)
    assert solver.solve_vrp_lsr_batch(reqs, spread="auto", **kw) == default
    assert solver.solve_vrp_lsr_batch(reqs, spread=3, **kw) == default
    for x in (0, 1, 5):
        assert solver.solve_vrp("lsr", *reqs[x], **kw) == default[x]
        assert solver.solve_vrp("lsr", *reqs[x], spread=4, **kw) == default[x]
        assert solver.solve_vrp("lsr", *reqs[x], spread="auto", **kw) == default[x]
    assert solver.solve_vrp("lsr", *reqs[2], spread=4, **kw) == default[2]


def _post(port, case, **kw):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/solve/vrp/lsr", data=_body(case, **kw),
                                 method="POST")
    with urllib.request.urlopen(req, timeout=120) as resp:
        return resp.status, json.loads(resp.read())


@pytest.mark.gpu
def test_service_spread_over_http_gives_the_same_bodies():
    S, rounds = 8, 1000
    cases = [(6, 2, 24, 61, ""), (9, 3, 1, 52, "")]
    bodies = {}
    for name, extra in (("plain", {}), ("auto", dict(batch_lsr_spread="auto")),
                        ("five", dict(batch_lsr_spread=5))):
        app = service.App(service.MemoryStore({}, {}, {}), seed=SEED, batch_vrp_lsr=True,
                          batch_window_s=0.01, batch_lsr_starts=S, batch_lsr_rounds=rounds, **extra)
        srv = service.serve(app, "127.0.0.1", 0)
        th = threading.Thread(target=srv.serve_forever, daemon=True)
        th.start()
        try:
            port = srv.server_address[1]
            bodies[name] = [_post(port, c) for c in cases]
            if name == "plain":   # the inline knob: the unbatched route at that spread
                bodies["knob"] = [_post(port, c, knobs={"spread": 4, "starts": S}, seed=SEED)
                                  for c in cases]
                bodies["noknob"] = [_post(port, c, knobs={"starts": S}, seed=SEED) for c in cases]
        finally:
            srv.shutdown()
            srv.server_close()
            th.join()
        assert app.vrp_lsr_batcher.requests == len(cases)
    for x, case in enumerate(cases):
        st, plain = bodies["plain"][x]
        assert st == 200 and plain["success"]
        assert [plain["message"]] == solver.solve_vrp_lsr_batch([request(case, 100)], starts=S,
                                                                rounds=rounds, seed=SEED)
        for name in ("auto", "five", "knob", "noknob"):
            assert bodies[name][x] == (200, plain), name
