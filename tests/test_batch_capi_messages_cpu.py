"""The C entry points of the eight batched heuristic solvers (vrp_batch_sa, _ga,
_aco, _ls, _lsr, _lsr_spread, tsp_batch_lso, _lso_spread), their eight _lds
functions and the two _work functions: the complete vrpms_last_error() text of
every refusal they can give without a device, and which refusal wins when two
arguments are wrong at once.

No GPU is needed: every argument check comes before the context is looked at,
so a block of zeros serves as the non-NULL ctx (as in the solvers' own
test_argument_errors_need_no_gpu), and its LDS size of zero turns every launch
that passes the other checks into the LDS refusal.  The one refusal behind
that, vrp_batch_aco's N > 128, cannot be reached this way.

Every expected string is a literal: the entry point's name, then the text the
library gave when this file was written."""
import ctypes

import pytest

from vrpms_amd import _lib

VRP = ("sa", "ga", "aco", "ls", "lsr", "lsr_spread")
TSP = ("lso", "lso_spread")
NAME = {"sa": b"vrpms_vrp_batch_sa", "ga": b"vrpms_vrp_batch_ga", "aco": b"vrpms_vrp_batch_aco",
        "ls": b"vrpms_vrp_batch_ls", "lsr": b"vrpms_vrp_batch_lsr",
        "lsr_spread": b"vrpms_vrp_batch_lsr_spread", "lso": b"vrpms_tsp_batch_lso",
        "lso_spread": b"vrpms_tsp_batch_lso_spread"}
# the buffers of every launch, in the order of its NULL test, and that test's text
VRP_BUFFERS = ("m", "d", "cp", "st", "t", "k", "du", "v")
BUFFERS = {"sa": ("m", "d", "cp", "st", "it0", "t", "k", "du", "v"), "ga": VRP_BUFFERS,
           "aco": VRP_BUFFERS, "ls": VRP_BUFFERS + ("i",), "lsr": VRP_BUFFERS + ("i",),
           "lsr_spread": VRP_BUFFERS + ("i",), "lso": ("m", "st", "t", "k", "du", "i"),
           "lso_spread": ("m", "st", "t", "k", "du", "i")}
NULL_BUFFER = {
    "sa": b": NULL matrix/demand/capacity/start/inv_t0/tour/key/duration/vehicle buffer",
    "ga": b": NULL matrix/demand/capacity/start/tour/key/duration/vehicle buffer",
    "aco": b": NULL matrix/demand/capacity/start/tour/key/duration/vehicle buffer",
    "ls": b": NULL matrix/demand/capacity/start/tour/key/duration/vehicle/info buffer",
    "lsr": b": NULL matrix/demand/capacity/start/tour/key/duration/vehicle/info buffer",
    "lsr_spread": b": NULL matrix/demand/capacity/start/tour/key/duration/vehicle/info buffer",
    "lso": b": NULL matrix/start/tour/key/duration/info buffer",
    "lso_spread": b": NULL matrix/start/tour/key/duration/info buffer"}
DEFAULTS = dict(R=1, N=5, K=2, H=1, obj=0, wide=0, steps=3, P=12, A=7, G=2, I=1, S=8, rounds=3, moves=31,
                tau0=1 << 20, tau_min=1 << 10, tau_max=1 << 28, evap_shift=3, bsf_period=0, wb=1 << 16)

CTX = b": ctx is NULL"
BYTES = b": bytes is NULL"
R_NEG = b": R must not be negative"
N_1 = b": needs 2 <= N <= 65535 (1 given)"
N_BIG = b": needs 2 <= N <= 65535 (65536 given)"
K_0 = b": one lane per route needs 1 <= K <= 64 (0 given)"
K_65 = b": one lane per route needs 1 <= K <= 64 (65 given)"
L_BIG = b": positions are uint16: needs N + K - 2 <= 65535 (65536 given)"
H_0 = b": H must be 1 or 24 (0 given)"
H_2 = b": H must be 1 or 24 (2 given)"
WIDE_NEG = b": wide must be 0 (uint16 matrix) or 1 (int32) (-1 given)"
WIDE_2 = b": wide must be 0 (uint16 matrix) or 1 (int32) (2 given)"
OBJ = b": objective must be VRPMS_OBJ_SUM or VRPMS_OBJ_MAX"
S_0 = b": 1 <= S <= 65535 (0 given)"
S_BIG = b": 1 <= S <= 65535 (65536 given)"
ROUNDS = b": rounds must not be negative (-1 given)"
MOVES_0 = b": 1 <= moves <= 31, bit t enabling move type t (0 given)"
MOVES_32 = b": 1 <= moves <= 31, bit t enabling move type t (32 given)"
G_0 = b": 1 <= G <= 65535 (0 given)"
G_BIG = b": 1 <= G <= 65535 (65536 given)"

# the shape bound only its owner has, checked after `wide` (ga, aco) or after K (lsr)
OWN = {"ga": ((dict(P=1), b": one lane per member needs 2 <= P <= 256 (1 given)"),
              (dict(P=257), b": one lane per member needs 2 <= P <= 256 (257 given)")),
       "aco": ((dict(A=0), b": one lane per ant needs 1 <= A <= 256 (0 given)"),
               (dict(A=257), b": one lane per ant needs 1 <= A <= 256 (257 given)")),
       "lsr": ((dict(N=65535, K=3), L_BIG),), "lsr_spread": ((dict(N=65535, K=3), L_BIG),)}
# the solver's own arguments, checked after the objective in this order; a pair
# of them wrong at once gives the earlier one's text
LS_KNOBS = ((dict(S=0), S_0), (dict(S=65536), S_BIG), (dict(rounds=-1), ROUNDS), (dict(S=0, rounds=-1), S_0))
LSO_KNOBS = LS_KNOBS + ((dict(moves=0), MOVES_0), (dict(moves=32), MOVES_32),
                        (dict(rounds=-1, moves=0), ROUNDS))
KNOBS = {
    "sa": ((dict(steps=-1), b": steps must not be negative"),),
    "ga": ((dict(G=-1), b": G must not be negative (-1 given)"),),
    "aco": ((dict(I=0), b": I must be at least 1 (0 given)"),
            (dict(evap_shift=0), b": evap_shift must be in [1, 31] (0 given)"),
            (dict(evap_shift=32), b": evap_shift must be in [1, 31] (32 given)"),
            (dict(bsf_period=-1), b": bsf_period must not be negative (-1 given)"),
            (dict(tau_min=0),
             b": needs 0 < tau_min <= tau0 <= tau_max <= 2^30 (0, 1048576, 268435456 given)"),
            (dict(tau0=3, tau_min=4), b": needs 0 < tau_min <= tau0 <= tau_max <= 2^30 (4, 3, 268435456 given)"),
            (dict(tau_max=(1 << 30) + 1),
             b": needs 0 < tau_min <= tau0 <= tau_max <= 2^30 (1024, 1048576, 1073741825 given)"),
            (dict(I=0, evap_shift=0), b": I must be at least 1 (0 given)"),
            (dict(evap_shift=0, bsf_period=-1), b": evap_shift must be in [1, 31] (0 given)"),
            (dict(bsf_period=-1, tau_min=0), b": bsf_period must not be negative (-1 given)")),
    "ls": LS_KNOBS, "lsr": LS_KNOBS,
    "lsr_spread": LS_KNOBS + ((dict(G=0), G_0), (dict(G=65536), G_BIG), (dict(rounds=-1, G=0), ROUNDS)),
    "lso": LSO_KNOBS,
    "lso_spread": LSO_KNOBS + ((dict(G=0), G_0), (dict(G=65536), G_BIG), (dict(moves=0, G=0), MOVES_0))}

# LDS bytes at (5, 2, 1, 0), at (59, 4, 24, 1) -- ga at P = 12, aco at A = 7 --
# and at the largest N with K = 2, H = 24, wide = 1 (65534 for the lsr pair,
# whose tour has N + K - 2 positions), where H N N 4 is far above 2^32
LDS = {"sa": (352, 336016, 412306112672), "ga": (1104, 337920, 412307718800),
       "aco": (488, 363288, 446664278184), "ls": (320, 335536, 412305588416),
       "lsr": (320, 335536, 412293005792), "lsr_spread": (320, 335088, 412292481568),
       "lso": (512, 336224, 412306374816), "lso_spread": (512, 335776, 412305850592)}
MIDDLE = {"ga": b" at P = 12", "aco": b" at A = 7"}


def lds_refusals(fn):
    """(arguments, the LDS refusal's text less the name) at the three shapes of LDS[fn]"""
    big = 65534 if fn.startswith("lsr") else 65535
    out = []
    for (N, K, H, wide), need in zip(((5, 2, 1, 0), (59, 4, 24, 1), (big, 2, 24, 1)), LDS[fn]):
        shape = b"N = %d, K = %d, H = %d" % (N, K, H) if fn in VRP else b"N = %d, H = %d" % (N, H)
        kw = dict(N=N, K=K, H=H, wide=wide) if fn in VRP else dict(N=N, H=H, wide=wide)
        out.append((kw, b": a request of " + shape + (b" (int32 matrix)" if wide else b" (uint16 matrix)") +
                    MIDDLE.get(fn, b"") + b" needs %d bytes of LDS (0 available)" % need, need))
    return out


@pytest.fixture(scope="module")
def call():
    """call(fn, **overrides) -> (code, vrpms_last_error(), the _lds / _work value): `fn` is an
    entry point's name less "vrpms_vrp_batch_" / "vrpms_tsp_batch_", every argument has a good
    default, a block of zeros is the context and another serves as every buffer."""
    from vrpms_amd.build import build_library
    build_library()
    lib = _lib.load()
    fake = ctypes.create_string_buffer(1 << 12)
    buf = ctypes.create_string_buffer(1 << 16)
    c, p = ctypes.addressof(fake), ctypes.addressof(buf)
    assert p % 8 == 0

    def call(fn, **kw):
        a = dict(DEFAULTS, ctx=c, work=p, **{name: p for name in BUFFERS.get(fn, ())})
        out = ctypes.c_uint64(77)
        a["bytes"] = ctypes.byref(out)
        a.update(kw)
        if a["work"] == "odd":
            a["work"] = p + 4
        if fn in VRP:
            head = (a["ctx"], a["m"], a["d"], a["cp"], a["st"])
            shape = (a["R"], a["N"], a["K"], a["H"], a["obj"], a["wide"])
            tail = (a["t"], a["k"], a["du"], a["v"])
        if fn == "sa":
            rc = lib.vrpms_vrp_batch_sa(*head, a["it0"], *shape, a["steps"], 0.999, 12345, *tail, None)
        elif fn == "ga":
            rc = lib.vrpms_vrp_batch_ga(*head, *shape, a["P"], a["G"], 1 << 30, 12345, *tail, None)
        elif fn == "aco":
            rc = lib.vrpms_vrp_batch_aco(*head, *shape, a["A"], a["I"], a["tau0"], a["tau_min"], a["tau_max"],
                                         a["evap_shift"], a["bsf_period"], 12345, *tail, None)
        elif fn in ("ls", "lsr"):
            rc = getattr(lib, "vrpms_vrp_batch_" + fn)(*head, *shape, a["S"], a["rounds"], 12345, *tail,
                                                       a["i"], None)
        elif fn == "lsr_spread":
            rc = lib.vrpms_vrp_batch_lsr_spread(*head, *shape, a["S"], a["rounds"], 12345, a["G"], a["work"],
                                                a["wb"], *tail, a["i"], None)
        elif fn in TSP:
            spread = (a["G"], a["work"], a["wb"]) if fn == "lso_spread" else ()
            rc = getattr(lib, "vrpms_tsp_batch_" + fn)(a["ctx"], a["m"], a["st"], a["R"], a["N"], a["H"],
                                                       a["wide"], a["S"], a["rounds"], a["moves"], 12345,
                                                       *spread, a["t"], a["k"], a["du"], a["i"], None)
        elif fn in ("ga_lds", "aco_lds"):
            rc = getattr(lib, "vrpms_vrp_batch_" + fn)(a["N"], a["K"], a["H"], a["wide"],
                                                       a["P" if fn == "ga_lds" else "A"], a["bytes"])
        elif fn in ("lso_lds", "lso_spread_lds"):
            rc = getattr(lib, "vrpms_tsp_batch_" + fn)(a["N"], a["H"], a["wide"], a["bytes"])
        elif fn == "lso_spread_work":
            rc = lib.vrpms_tsp_batch_lso_spread_work(a["R"], a["N"], a["G"], a["bytes"])
        elif fn == "lsr_spread_work":
            rc = lib.vrpms_vrp_batch_lsr_spread_work(a["R"], a["N"], a["K"], a["G"], a["bytes"])
        else:
            rc = getattr(lib, "vrpms_vrp_batch_" + fn)(a["N"], a["K"], a["H"], a["wide"], a["bytes"])
        assert buf.raw == bytes(1 << 16) and fake.raw == bytes(1 << 12)   # nothing was written
        return rc, lib.vrpms_last_error(), out.value

    return call


def refusals(call, fn, name, cases):
    for kw, text in cases:
        rc, msg, out = call(fn, **kw)
        assert (rc, msg, out) == (_lib.VRPMS_EINVAL, name + text, 77), (fn, kw)


def shape_cases(fn):
    """the shape checks of fn's launch, _lds and (less H and wide) _work alike"""
    vrp = fn in VRP
    cases = [(dict(N=1), N_1), (dict(N=65536), N_BIG), (dict(H=0), H_0), (dict(H=2), H_2),
             (dict(wide=-1), WIDE_NEG), (dict(wide=2), WIDE_2),
             (dict(N=1, H=2), N_1), (dict(H=2, wide=2), H_2)]
    if vrp:
        cases += [(dict(K=0), K_0), (dict(K=65), K_65), (dict(N=1, K=0), N_1), (dict(K=0, H=2), K_0),
                  (dict(N=65535, K=65), K_65)]
    for kw, text in OWN.get(fn, ()):
        cases.append((kw, text))
        if fn.startswith("lsr"):   # L follows K and comes before H and wide
            cases += [(dict(kw, H=2), text), (dict(kw, wide=2), text)]
        else:                      # P and A come last
            cases += [(dict(kw, H=2), H_2), (dict(kw, wide=2), WIDE_2)]
    return cases


@pytest.mark.parametrize("fn", VRP + TSP)
def test_launch_refusals_and_their_order(call, fn):
    name, vrp = NAME[fn], fn in VRP
    first = BUFFERS[fn][0]
    knob, knob_text = KNOBS[fn][0]
    cases = [(dict(ctx=None), CTX), (dict(ctx=None, R=-1), CTX), (dict(R=-1), R_NEG), (dict(R=-1, N=1), R_NEG)]
    cases += shape_cases(fn)
    if vrp:   # shape, then objective, then the solver's own
        cases += [(dict(obj=-1), OBJ), (dict(obj=2), OBJ), (dict(wide=2, obj=2), WIDE_2),
                  (dict(knob, obj=2), OBJ)]
        cases += [(dict(kw, obj=2), text) for kw, text in OWN.get(fn, ())[:1]]
    else:
        cases += [(dict(knob, wide=2), WIDE_2)]
    cases += list(KNOBS[fn])
    # then the buffers, but only with requests to serve
    cases += [({b: None}, NULL_BUFFER[fn]) for b in BUFFERS[fn]]
    cases += [(dict(knob, **{first: None}), knob_text), (dict(knob, R=0), knob_text), (dict(R=0, H=2), H_2)]
    if fn.endswith("_spread"):   # G is the last of the solver's own; the workspace follows the buffers
        rec = 32 if fn == "lsr_spread" else 40   # a record of N = 5 (K = 2)
        cases += [(dict(R=0, G=0), G_0), (dict(G=0, work=None), G_0), ({"G": 0, first: None}, G_0),
                  ({"work": None, first: None}, NULL_BUFFER[fn]),
                  (dict(R=32769, S=65535, G=65535, wb=2**64 - 1),
                   b": R * min(G, S) = 2147516415 workgroups are above 2^31 - 1"),
                  (dict(R=32769, S=65535, G=65535, work=None),
                   b": R * min(G, S) = 2147516415 workgroups are above 2^31 - 1"),
                  (dict(work=None), b": the workspace is NULL"),
                  (dict(work=None, wb=0), b": the workspace is NULL"),
                  (dict(work="odd"), b": the workspace must be 8-byte aligned"),
                  (dict(work="odd", wb=0), b": the workspace must be 8-byte aligned"),
                  (dict(wb=0), b": the workspace has 0 bytes, R = 1 requests of min(G, S) = 2 workgroups "
                   b"need %d" % (2 * rec)),
                  (dict(wb=15), b": the workspace has 15 bytes, R = 1 requests of min(G, S) = 2 workgroups "
                   b"need %d" % (2 * rec)),
                  (dict(R=7, S=3, G=64, wb=100), b": the workspace has 100 bytes, R = 7 requests of "
                   b"min(G, S) = 3 workgroups need %d" % (21 * rec))]
    # and the LDS last of all
    cases += [(dict(kw, wb=2**64 - 1), text) for kw, text, _ in lds_refusals(fn)]
    refusals(call, fn, name, cases)
    # no requests: no buffer is looked at
    nothing = {b: None for b in BUFFERS[fn]}
    assert call(fn, R=0, **nothing)[0] == _lib.VRPMS_OK
    if fn.endswith("_spread"):
        assert call(fn, R=0, G=65535, work=None, wb=0, **nothing)[0] == _lib.VRPMS_OK


@pytest.mark.parametrize("fn", VRP + TSP)
def test_lds_refusals_and_values(call, fn):
    cases = [(dict(bytes=None), BYTES), (dict(bytes=None, N=1), BYTES)] + shape_cases(fn)
    refusals(call, fn + "_lds", NAME[fn] + b"_lds", cases)
    for kw, _, need in lds_refusals(fn):
        assert call(fn + "_lds", **kw)[::2] == (_lib.VRPMS_OK, need), (fn, kw)


@pytest.mark.parametrize("fn", ("lsr_spread", "lso_spread"))
def test_work_refusals_and_values(call, fn):
    cases = [(dict(bytes=None), BYTES), (dict(bytes=None, R=-1), BYTES), (dict(R=-1), R_NEG),
             (dict(R=-1, N=1), R_NEG), (dict(N=1), N_1), (dict(N=65536), N_BIG), (dict(N=1, G=0), N_1),
             (dict(G=0), G_0), (dict(G=65536), G_BIG), (dict(R=32769, G=65536), G_BIG),
             (dict(R=32769, G=65535), b": R * G = 2147516415 records are above 2^31 - 1")]
    if fn == "lsr_spread":
        cases += [(dict(K=0), K_0), (dict(K=65), K_65), (dict(N=1, K=0), N_1), (dict(N=65535, K=3), L_BIG),
                  (dict(K=0, G=0), K_0)]
    refusals(call, fn + "_work", NAME[fn] + b"_work", cases)
    want = {"lsr_spread": (64, 281496450105360), "lso_spread": (80, 281513629188120)}[fn]
    assert call(fn + "_work")[::2] == (_lib.VRPMS_OK, want[0])
    assert call(fn + "_work", R=0)[::2] == (_lib.VRPMS_OK, 0)
    assert call(fn + "_work", R=32767, N=65535, G=65535)[::2] == (_lib.VRPMS_OK, want[1])
