"""GPU parity of the population / island kernels (csrc/pool.hip) against
oracle/pool.py: Philox start tours, elite selection, the three injection
modes, island messages byte for byte, the multi-rank merge and the local
exchange; ACO's device-side colony-best tracking."""
import numpy as np
import pytest

import selection_cases as sc
from oracle import pool as opool
from oracle import search
from vrpms_amd import synth

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


def torch_():
    import torch
    return torch


def u64(t):
    return [int(x) & M64 for x in t.reshape(-1).cpu().tolist()]


def i64(vals):
    torch = torch_()
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in vals], dtype=torch.int64)


@pytest.mark.parametrize("n,ld,dt", [(1, 1, "i16"), (2, 4, "u8"), (13, 16, "u8"), (100, 100, "u8"),
                                     (100, 100, "i16"), (1000, 1000, "i16")])
def test_random_tours_match_oracle(ctx, n, ld, dt):
    torch = torch_()
    dtype = torch.uint8 if dt == "u8" else torch.int16
    T = ctx.random_tours(77, n, seed=2**40 + 5, stream_id=3, ld=ld, dtype=dtype).cpu().numpy()
    T = T.astype(np.int64) & (0xFF if dt == "u8" else 0xFFFF)
    for r in (0, 1, 38, 76):
        assert T[r, :n].tolist() == opool.philox_tour(n, 2**40 + 5, r, 3)
        assert (T[r, n:] == 0).all()
    assert all(sorted(row[:n]) == list(range(1, n + 1)) for row in T.tolist())


def _keys(rng, count, dup=True):
    k = rng.integers(0, 2**62, size=count, dtype=np.int64).astype(np.uint64)
    if dup:
        k[rng.integers(0, count, size=count // 3)] = k[0]      # ties resolved by index
        k[rng.integers(0, count, size=5)] = np.uint64(M64)
    return [int(x) for x in k]


@pytest.mark.parametrize("count,E", [(7, 7), (300, 16), (5000, 32), (70000, 8)])
def test_pool_elites_match_oracle(ctx, count, E):
    torch = torch_()
    rng = np.random.default_rng(count)
    n = 5
    keys = _keys(rng, count)
    tours = rng.integers(1, 6, size=(count, n))
    t, k = ctx.pool_elites(torch.tensor(tours, dtype=torch.int16, device=ctx.dev),
                           i64(keys).to(ctx.dev), E)
    rt, rk = opool.pool_elites(tours.tolist(), keys, E)
    assert u64(k) == rk and t.cpu().tolist() == rt


@pytest.mark.parametrize("mode", [opool.INJECT_WORST, opool.INJECT_SORTED, opool.INJECT_BETTER])
def test_pool_inject_matches_oracle(ctx, mode):
    torch = torch_()
    rng = np.random.default_rng(mode)
    groups, P, n, E = 4, 50, 9, 11
    count = groups * P
    keys = _keys(rng, count)
    if mode == opool.INJECT_SORTED:   # GA islands are kept sorted by (key, index)
        keys = [k for g in range(groups) for k in sorted(keys[g * P:(g + 1) * P])]
    tours = rng.integers(1, 10, size=(count, n))
    mk = sorted(_keys(rng, E, dup=False))
    mt = rng.integers(1, 10, size=(E, n))
    dt = torch.tensor(tours, dtype=torch.int16, device=ctx.dev)
    dk = i64(keys).to(ctx.dev)
    ctx.pool_inject(dt, dk, mode, torch.tensor(mt, dtype=torch.int16, device=ctx.dev),
                    i64(mk).to(ctx.dev), groups)
    rt, rk = opool.pool_inject(tours.tolist(), keys, mode, mt.tolist(), mk, groups)
    assert u64(dk) == rk and dt.cpu().tolist() == rt


def test_island_pack_bytes_and_merge_match_oracle(ctx):
    torch = torch_()
    rng = np.random.default_rng(11)
    world, count, n, E = 5, 400, 37, 12
    pools = [(rng.integers(1, 38, size=(count, n)), _keys(rng, count)) for _ in range(world)]
    msgs = []
    for tours, keys in pools:
        m = ctx.island_pack(torch.tensor(tours, dtype=torch.int16, device=ctx.dev),
                            i64(keys).to(ctx.dev), E)
        got = bytes(m.cpu().numpy().tobytes())
        assert got == opool.island_pack(tours.tolist(), keys, E, n)
        msgs.append(m)
    assert ctx.island_msg_bytes(E, n) == opool.msg_bytes(E, n)
    t, k = ctx.island_merge(torch.cat(msgs), world, E, n)
    rt, rk = opool.island_merge(b"".join(bytes(m.cpu().numpy().tobytes()) for m in msgs), world,
                                E, n)
    assert u64(k) == rk and t.cpu().tolist() == rt


def test_local_exchange_equals_oracle(ctx):
    torch = torch_()
    rng = np.random.default_rng(5)
    n, E = 20, 6
    src_t = rng.integers(1, 21, size=(64, n))
    src_k = _keys(rng, 64)
    dst_t = rng.integers(1, 21, size=(64, n))
    dst_k = _keys(rng, 64)
    s = (torch.tensor(src_t, dtype=torch.int16, device=ctx.dev), i64(src_k).to(ctx.dev))
    d = (torch.tensor(dst_t, dtype=torch.int16, device=ctx.dev), i64(dst_k).to(ctx.dev))
    assert ctx.island_world() == 0
    ctx.island_exchange(s, d, opool.INJECT_WORST, E)
    msg = opool.island_pack(src_t.tolist(), src_k, E, n)
    mt, mk = opool.island_merge(msg, 1, E, n)
    rt, rk = opool.pool_inject(dst_t.tolist(), dst_k, opool.INJECT_WORST, mt, mk)
    assert u64(d[1]) == rk and d[0].cpu().tolist() == rt


def test_aco_colony_best_tracking_on_device(ctx):
    from vrpms_amd.core import CVRP
    torch = torch_()
    inst = synth.cvrp(12, 3, seed=1, slack=0.95)
    ctx.set_instance(CVRP, inst.durations, inst.demand, inst.capacities, inst.start_times)
    colonies, ants = 3, 8
    tau, eta = ctx.aco_init(colonies, 1 << 20)
    bt = torch.zeros((colonies, inst.n), dtype=torch.int16, device=ctx.dev)
    bk = torch.full((colonies,), -1, dtype=torch.int64, device=ctx.dev)
    ref_k = [M64] * colonies
    ref_t = [[0] * inst.n for _ in range(colonies)]
    for it in range(4):
        tours, keys, ib = ctx.aco_iteration(tau, eta, ants, seed=9, it=it, best_tours=bt,
                                            best_keys=bk)
        T = tours.cpu().tolist()
        for c, (k, a) in enumerate(ib.cpu().tolist()):
            k &= M64
            if k < ref_k[c]:
                ref_k[c], ref_t[c] = k, T[c][a]
    assert u64(bk) == ref_k and bt.cpu().tolist() == ref_t
    sc = search.Scorer(inst.durations, inst.demand, inst.capacities, inst.start_times, "cvrp")
    assert all(sc(t) == k for t, k in zip(ref_t, ref_k))


# --- selection at its level, chunk, tie and size edges (tests/selection_cases.py;
# --- the premises of every input are proved in test_selection_cases_cpu.py) ----

def dev16(ctx, rows):
    return torch_().tensor(np.asarray(rows), dtype=torch_().int16, device=ctx.dev)


def vrpms_error():
    from vrpms_amd._lib import VrpmsError
    return VrpmsError


@pytest.mark.parametrize("count,E", sc.ELITE_CASES)
def test_pool_elites_levels_and_ties_match_oracle(ctx, count, E):
    """topk over 1 to 7 levels of 2048 -> E (3 at (6145, 1024); 5 at (20481,
    1024), where the result lands in the second buffer; 7 at (70000, 1000)), E
    up to the limit 1024 and E == count, with a run of E + 9 equal keys across
    the E-th place and across the first chunk boundary, beside 0 and 2^64 - 1."""
    n = sc.POOL_N
    keys = sc.pool_keys(count, E, seed=count + E)
    rows = sc.pool_rows(count, n, count)
    t, k = ctx.pool_elites(dev16(ctx, rows), i64(keys).to(ctx.dev), E)
    rt, rk = opool.pool_elites(rows.tolist(), keys, E)
    assert u64(k) == rk and t.cpu().tolist() == rt


def test_pool_elites_outside_the_limits_raise(ctx):
    rows = dev16(ctx, sc.pool_rows(3000, 5, 1))
    keys = i64(sc.pool_keys(3000, 1024, seed=1)).to(ctx.dev)
    with pytest.raises(vrpms_error()):
        ctx.pool_elites(rows, keys, 1025)
    with pytest.raises(vrpms_error()):
        ctx.pool_elites(rows[:600], keys[:600], 601)


@pytest.mark.parametrize("count,E", sc.WORST_CASES)
def test_pool_inject_worst_multi_chunk_matches_oracle(ctx, count, E):
    """INJECT_WORST over several chunks and levels (inverted keys): the E worst
    by (key descending, index ascending), with a run of equal keys across the
    E-th worst place and key 0 -- whose inverted value equals the pad key -- as
    the one real entry of the last chunk."""
    n = sc.POOL_N
    keys = sc.pool_keys(count, E, seed=count + E, worst=True)
    rows = sc.pool_rows(count, n, count)
    mt, mk = sc.migrants(E, n, count)
    dt, dk = dev16(ctx, rows), i64(keys).to(ctx.dev)
    ctx.pool_inject(dt, dk, opool.INJECT_WORST, dev16(ctx, mt), i64(mk).to(ctx.dev))
    rt, rk = opool.pool_inject(rows.tolist(), keys, opool.INJECT_WORST, mt.tolist(), mk)
    assert u64(dk) == rk and dt.cpu().tolist() == rt


@pytest.mark.parametrize("groups,P,E", sc.SORTED_CASES)
def test_pool_inject_sorted_sizes_match_oracle(ctx, groups, P, E):
    """INJECT_SORTED at P = 1, a power of two, P above the 1024 threads,
    P = 4096 (LDS exactly 65536 bytes), more migrants than slots (the surplus
    is dropped) and fewer migrants than islands; migrants tie with the rows
    they are sorted among."""
    rows, keys, mt, mk = sc.sorted_islands(groups, P, E, seed=P)
    dt, dk = dev16(ctx, rows), i64(keys).to(ctx.dev)
    ctx.pool_inject(dt, dk, opool.INJECT_SORTED, dev16(ctx, mt), i64(mk).to(ctx.dev), groups)
    rt, rk = opool.pool_inject(rows.tolist(), keys, opool.INJECT_SORTED, mt.tolist(), mk, groups)
    assert u64(dk) == rk and dt.cpu().tolist() == rt


def test_pool_inject_sorted_outside_the_limits_raises(ctx):
    rows, keys, mt, mk = sc.sorted_islands(1, 4097, 4, seed=3)
    dt, dk = dev16(ctx, rows), i64(keys).to(ctx.dev)
    m = (dev16(ctx, mt), i64(mk).to(ctx.dev))
    with pytest.raises(vrpms_error()):          # M = 8192: too large for the LDS sort
        ctx.pool_inject(dt, dk, opool.INJECT_SORTED, *m, 1)
    with pytest.raises(vrpms_error()):          # 4097 = 17 * 241
        ctx.pool_inject(dt, dk, opool.INJECT_SORTED, *m, 16)
    assert u64(dk) == keys and dt.cpu().tolist() == rows.tolist()


def test_pool_inject_better_more_migrants_than_rows_and_equal_keys(ctx):
    """INJECT_BETTER with E > count (the migrants past the last row are
    ignored), and a migrant whose key equals the row's does not replace it."""
    n, count, E = 7, 5, 9
    rows = sc.pool_rows(count, n, 1)
    mt = sc.pool_rows(E, n, 2)
    keys = [50, 0, 70, sc.M64, 90]
    mk = [50, 0, 69, sc.M64, 91, 1, 2, 3, 4]       # equal, equal, better, equal, worse
    dt, dk = dev16(ctx, rows), i64(keys).to(ctx.dev)
    ctx.pool_inject(dt, dk, opool.INJECT_BETTER, dev16(ctx, mt), i64(mk).to(ctx.dev))
    rt, rk = opool.pool_inject(rows.tolist(), keys, opool.INJECT_BETTER, mt.tolist(), mk)
    assert rk == [50, 0, 69, sc.M64, 90] and rt[0] == rows[0].tolist() and rt[2] == mt[2].tolist()
    assert u64(dk) == rk and dt.cpu().tolist() == rt


def _pack(ctx, tours, keys, E, n):
    """island_pack; with n == 0 through the C entry point, since an empty
    tensor has no address to hand over (the rows are never read)."""
    torch = torch_()
    dk = i64(keys).to(ctx.dev)
    if n:
        return ctx.island_pack(dev16(ctx, tours), dk, E)
    import ctypes

    from vrpms_amd import _lib
    hold = torch.zeros(8, dtype=torch.int16, device=ctx.dev)
    msg = torch.empty(ctx.island_msg_bytes(E, 0), dtype=torch.uint8, device=ctx.dev)
    p = _lib.Pool(hold.data_ptr(), dk.data_ptr(), len(keys), 0, 1)
    _lib.check(ctx.lib.vrpms_island_pack(ctx.handle, ctypes.byref(p), E, msg.data_ptr(),
                                         ctx.stream()))
    torch.cuda.synchronize()
    return msg


def _merge(ctx, msgs, world, E, n):
    torch = torch_()
    if n:
        t, k = ctx.island_merge(msgs, world, E, n)
        return t.cpu().tolist(), u64(k)
    from vrpms_amd import _lib
    hold = torch.zeros(8, dtype=torch.int16, device=ctx.dev)
    k = torch.empty(E, dtype=torch.int64, device=ctx.dev)
    _lib.check(ctx.lib.vrpms_island_merge(ctx.handle, msgs.data_ptr(), world, E, 0,
                                          hold.data_ptr(), k.data_ptr(), ctx.stream()))
    assert (hold == 0).all()
    return [[] for _ in range(E)], u64(k)


@pytest.mark.parametrize("world,E,n,identical", sc.MERGE_CASES)
def test_island_merge_levels_ties_and_empty_rows_match_oracle(ctx, world, E, n, identical):
    """island_pack byte for byte and island_merge by (key, rank, position):
    3 x 1024 and 9 x 1024 candidates (2 and 4 levels), identical messages from
    every rank (the state after one exchange), and messages without rows."""
    torch = torch_()
    pools = sc.merge_pools(world, E, n, identical)
    msgs = []
    for tours, keys in pools:
        m = _pack(ctx, tours, keys, E, n)
        assert bytes(m.cpu().numpy().tobytes()) == opool.island_pack(tours.tolist(), keys, E, n)
        msgs.append(m)
    assert ctx.island_msg_bytes(E, n) == opool.msg_bytes(E, n) == msgs[0].numel()
    allm = torch.cat(msgs)
    rt, rk = opool.island_merge(bytes(allm.cpu().numpy().tobytes()), world, E, n)
    assert _merge(ctx, allm, world, E, n) == (rt, rk)


def test_local_exchange_all_modes_growing_scratch(ctx):
    """island_exchange without a communicator == pack -> merge -> inject of
    the oracle, in all three modes on one context with E, n and the pools
    growing from call to call: the message sizes (none a multiple of 16 before
    padding) put the work area at another offset each time, and the last call
    needs more scratch than any pool test before it, so the scratch is
    reallocated between calls (every time on a fresh context)."""
    assert ctx.island_world() == 0
    calls = [(opool.INJECT_WORST, 1, 70, 64, 3, 5), (opool.INJECT_BETTER, 1, 300, 4, 5, 7),
             (opool.INJECT_SORTED, 4, 3000, 4 * 2048, 7, 9),
             (opool.INJECT_WORST, 1, 5000, 90000, 1001, 11)]
    for mode, groups, src_count, dst_count, E, n in calls:
        assert (E * 8 + E * n * 2) % 16 and n % 2
        if mode == opool.INJECT_SORTED:
            dst_t, dst_k, _, _ = sc.sorted_islands(groups, dst_count // groups, E, seed=n, n=n)
        else:
            dst_t, dst_k = sc.pool_rows(dst_count, n, n), sc.pool_keys(max(dst_count, 12), E, n,
                                                                         worst=True)[:dst_count]
        src_t, src_k = sc.pool_rows(src_count, n, n + 1), sc.pool_keys(src_count, E, seed=n + 1)
        s = (dev16(ctx, src_t), i64(src_k).to(ctx.dev))
        d = (dev16(ctx, dst_t), i64(dst_k).to(ctx.dev))
        ctx.island_exchange(s, d, mode, E, groups)
        msg = opool.island_pack(src_t.tolist(), src_k, E, n)
        mt, mk = opool.island_merge(msg, 1, E, n)
        rt, rk = opool.pool_inject(dst_t.tolist(), dst_k, mode, mt, mk, groups)
        assert u64(d[1]) == rk and d[0].cpu().tolist() == rt, (mode, E, n)
        assert u64(s[1]) == src_k and s[0].cpu().tolist() == src_t.tolist()


@pytest.mark.parametrize("n,n_sep,dt,count,ld", [
    (1280, 0, "i16", 65, 1280),     # the last row length shuffled in LDS (64 rows x 2560 B = 160 KiB)
    (1281, 0, "i16", 65, 1284),     # the first one shuffled in place in HBM
    (1275, 6, "i16", 65, 1281),     # ... with separators
    (250, 5, "u8", 64, 255), (250, 5, "u8", 65, 255),       # the last uint8 token
])
def test_random_tours_size_edges_match_oracle(ctx, n, n_sep, dt, count, ld):
    torch = torch_()
    dtype = torch.uint8 if dt == "u8" else torch.int16
    T = ctx.random_tours(count, n, seed=2**41 + 9, stream_id=5, ld=ld, dtype=dtype, n_sep=n_sep)
    T = T.cpu().numpy().astype(np.int64) & (0xFF if dt == "u8" else 0xFFFF)
    L = n + n_sep
    assert (64 * L * 2 <= sc.LDS_BYTES) == (L <= 1280)
    for r in range(count):          # every row: one lane each, 64 to a block, one row in the second block
        assert T[r, :L].tolist() == opool.philox_tour(n, 2**41 + 9, r, 5, n_sep), r
    assert (T[:, L:] == 0).all()


def test_random_tours_token_past_uint8_raises(ctx):
    torch = torch_()
    with pytest.raises(vrpms_error()):
        ctx.random_tours(4, 250, seed=1, dtype=torch.uint8, n_sep=6)
