"""The premises of tests/selection_cases.py, proved without a GPU by the Python
oracle alone (oracle/search.py ga_generation, oracle/pool.py): every case
reaches the code path it is named for, has keys tied where the selection rule
decides, and gives another result under each wrong rule -- ties by descending
index, children before parents, worst-E ties by descending index, merge ties
by (key, position, rank).  A kernel with one of those rules cannot pass the
GPU comparison of the same case."""
import numpy as np
import pytest

import selection_cases as sc
import value_edges as ve
from oracle import pool as opool

GA_NAMES = [c.name for c in sc.GA_CASES]


@pytest.mark.parametrize("name", GA_NAMES)
def test_ga_case_ties_across_the_cut_and_children_survive(name):
    case = sc.GA_BY_NAME[name]
    P = case.P
    pops, keys, log = sc.ga_replay(name)
    assert len(log) == case.gens and all(len(g) == case.islands for g in log)
    for island in range(case.islands):
        # the tie the index must break: equal keys at ranks P - 1 and P of the 2P pairs
        assert any(g[island][P - 1][0] == g[island][P][0] for g in log), (name, island)
        for gi, g in enumerate(log):
            entered = sum(i >= P for _, i in g[island][:P])
            # a last generation may keep all its parents once they share one key
            # (a child at that key loses the tie, a worse one loses outright)
            converged = gi == case.gens - 1 and gi > 0 and \
                g[island][0][0] == g[island][P - 1][0] and entered == 0
            assert entered > 0 or converged, (name, island, gi)
    n = sc.instance(case.kind).n
    assert all(sorted(t) == list(range(1, n + 1)) for isl in pops for t in isl)
    assert all(k == sorted(k) for k in keys)


@pytest.mark.parametrize("rule", list(sc.GA_WRONG))
@pytest.mark.parametrize("name", GA_NAMES)
def test_ga_case_tells_a_wrong_survivor_rule_apart(name, rule):
    right, wrong = sc.ga_replay(name), sc.ga_replay(name, rule)
    assert (right[0], right[1]) != (wrong[0], wrong[1])
    # ... in every island, so no island's selection can go wrong unseen
    case = sc.GA_BY_NAME[name]
    for island in range(case.islands):
        assert right[0][island] != wrong[0][island], (name, rule, island)


def test_ga_cases_reach_the_paths_they_are_named_for():
    for kind in ("n5", "n9", "long", "td"):
        inst = sc.instance(kind)
        assert ve.model_layout(inst, inst.n)["fast"] == (kind != "td")
    assert (sc.instance("n5").n, sc.instance("n5").K) == (5, 2)
    assert (sc.instance("n9").n, sc.instance("n9").K) == (9, 3)
    assert (sc.instance("long").n, sc.instance("long").K) == (80, 7)
    for case in sc.GA_CASES:
        inst = sc.instance(case.kind)
        fused = case.P <= 1024 and case.kind != "td"
        assert fused == (case not in sc.GA_PAST)
        if fused:       # mode 0 takes the fused kernel only when the island fits the LDS
            assert sc.ga_fused_lds(inst.N, inst.n, case.P) <= sc.LDS_BYTES, case.name
    lds = {c.name: sc.ga_fused_lds(sc.instance(c.kind).N, sc.instance(c.kind).n, c.P)
           for c in sc.GA_CASES}
    assert lds["grid_n5_p2"] == 1472 and lds["grid_n5_p1024"] == 84512
    assert lds["grid_n9_p1024"] == 85152 and lds["long_p300"] == 128288
    assert sorted(c.P for c in sc.GA_GRID[:len(sc.GRID_P)]) == sorted(sc.GRID_P)
    # both sides of every threshold of the selection
    M = lambda P: 1 << (2 * P - 1).bit_length()      # noqa: E731
    assert (M(16), M(17), M(512), M(513), M(1024)) == (32, 64, 1024, 2048, 2048)
    assert {(P + 63) // 64 for P in sc.GRID_P} >= {1, 2, 3, 4, 5, 8, 9, 15, 16}
    assert all(P % 64 == 1 for P in (65, 129, 193))         # a last run of one real pair
    assert (M(1025), M(2048), M(2049), M(4096)) == (4096, 4096, 8192, 8192)
    assert 12 * M(2048) <= 65536 < 12 * M(2049) <= sc.LDS_BYTES


@pytest.mark.parametrize("case", sc.GA_PROBE, ids=lambda c: c.name)
def test_probe_islands_are_sorted_as_named(case):
    _, keys = sc.ga_start(case.name)
    P = case.P
    bad = [[i for i in range(1, P) if k[i - 1] > k[i]] for k in keys]
    assert bad == [[], [1], [P - 1], []]
    assert len(set(keys[3])) == 1 and len(set(keys[0])) > 3
    for k, (a, b) in ((keys[1], (0, 1)), (keys[2], (P - 2, P - 1))):
        k = list(k)
        k[a], k[b] = k[b], k[a]
        assert k == sorted(k)


@pytest.mark.parametrize("count,E", sc.ELITE_CASES + sc.WORST_CASES)
def test_pool_keys_hold_the_edges(count, E):
    worst = (count, E) in sc.WORST_CASES
    keys = sc.pool_keys(count, E, seed=count + E, worst=worst)
    assert len(keys) == count and min(keys) == 0 and max(keys) == sc.M64
    assert keys.count(0) == 2 and keys.count(sc.M64) == 2
    a, b = sc.dup_run(count, E, worst)
    v = keys[a]
    assert keys[a:b] == [v] * (b - a) and keys.count(v) == b - a
    order = sorted(range(count), key=lambda i: (-keys[i], i) if worst else (keys[i], i))
    if count > E:       # the run lies across the E-th place ...
        assert keys[order[E - 1]] == keys[order[E]]
    if count >= E + 15 and E > 2:
        assert b - a > E and keys[order[E]] == v
    if count > sc.CHUNK + 1 or (count > sc.CHUNK and not worst):
        assert a < sc.CHUNK < b      # ... and across a chunk boundary (its pairs meet at level 2)
    if worst:           # key 0 as the one real entry of the last chunk
        assert count % sc.CHUNK == 1 and keys[count - 1] == 0
        assert opool.worst_order(keys, E) != sorted(range(count), key=lambda i: (-keys[i], -i))[:E]


def test_pool_cases_take_the_levels_they_are_named_for():
    lv = {c: sc.topk_levels(*c) for c in sc.ELITE_CASES + sc.WORST_CASES}
    assert lv[(2048, 1024)] == 1 and lv[(2049, 1024)] == 2 and lv[(4097, 1024)] == 3
    assert lv[(6145, 1024)] == 3 and lv[(20481, 1024)] == 5 and lv[(70000, 1000)] == 7
    assert lv[(2049, 16)] == 2 and lv[(20481, 700)] == 4
    assert sc.topk_levels(70000, 8) == 2            # the deepest before these cases
    assert sc.topk_levels(3 * 1024, 1024) == 2 and sc.topk_levels(9 * 1024, 1024) == 4


@pytest.mark.parametrize("count,E", sc.ELITE_CASES)
def test_elite_cases_tell_descending_index_apart(count, E):
    keys = sc.pool_keys(count, E, seed=count + E)
    rows = sc.pool_rows(count, sc.POOL_N, count).tolist()
    assert opool.pool_elites(rows, keys, E) != sc.elites_desc(rows, keys, E)


@pytest.mark.parametrize("count,E", sc.WORST_CASES)
def test_worst_cases_tell_descending_index_apart(count, E):
    keys = sc.pool_keys(count, E, seed=count + E, worst=True)
    rows = sc.pool_rows(count, sc.POOL_N, count).tolist()
    mt, mk = sc.migrants(E, sc.POOL_N, count)
    assert opool.pool_inject(rows, keys, opool.INJECT_WORST, mt.tolist(), mk) != \
        sc.inject_worst_desc(rows, keys, mt.tolist(), mk)


@pytest.mark.parametrize("groups,P,E", sc.SORTED_CASES)
def test_sorted_cases_tell_descending_slot_apart(groups, P, E):
    rows, keys, mt, mk = sc.sorted_islands(groups, P, E, seed=P)
    assert all(keys[g * P:(g + 1) * P] == sorted(keys[g * P:(g + 1) * P]) for g in range(groups))
    assert mk == sorted(mk)
    right = opool.pool_inject(rows.tolist(), keys, opool.INJECT_SORTED, mt.tolist(), mk, groups)
    assert right != (rows.tolist(), keys)
    if P > 1:           # one row per island: nothing to order
        assert right != sc.inject_sorted_desc(rows.tolist(), keys, mt.tolist(), mk, groups)
    placed = min(E, groups * P)
    assert (placed < E) == ((groups, P, E) == (3, 5, 40))          # the surplus is dropped
    assert (E < groups) == ((groups, P, E) in ((300, 1, 7), (8, 50, 3)))    # islands left alone


@pytest.mark.parametrize("world,E,n,identical", sc.MERGE_CASES)
def test_merge_cases_tell_position_before_rank_apart(world, E, n, identical):
    pools = sc.merge_pools(world, E, n, identical)
    msgs = [opool.island_pack(t.tolist(), k, E, n) for t, k in pools]
    assert identical == (len(set(msgs)) == 1)
    right = opool.island_merge(b"".join(msgs), world, E, n)
    if n:               # without rows both orders give the same E keys
        assert right != sc.merge_by_position(b"".join(msgs), world, E, n)
    if identical:       # every elite world times: the E best are the first ones, each from every rank
        t, k = opool.pool_elites(pools[0][0].tolist(), pools[0][1], E)
        assert sorted(right[1]) == sorted((k * world))[:E] and all(x in t for x in right[0])
    ks = np.frombuffer(b"".join(m[:8 * E] for m in msgs), dtype=np.uint64)
    assert len(set(ks.tolist())) < len(ks) // 2                     # keys tie across ranks
