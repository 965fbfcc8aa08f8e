"""The GA's (mu + lambda) survivor selection on the device against the Python
replay (oracle/search.py ga_generation), at every population size where the
code takes another path: block_sort_pairs / block_sort_pairs_waves over the
unsorted first generation, merge_select_inplace and merge_select (with and
without idle wavefronts) from the second, the sortedness probe, and
ga_select_kernel past the fused kernel's limit.

The inputs come from tests/selection_cases.py; test_selection_cases_cpu.py
proves that each one has keys tied across the survival cut in every island and
gives another population under a wrong tie rule.  Populations and keys are
compared for exact equality."""
import pytest

import selection_cases as sc

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


def torch_():
    import torch
    return torch


def u64(t):
    return [int(x) & M64 for x in t.reshape(-1).cpu().tolist()]


def load(ctx, inst):
    from vrpms_amd.core import CVRP
    ctx.set_instance(CVRP, inst.durations, inst.demand, inst.capacities, inst.start_times)


def run(ctx, case, mode):
    """The case's calls with VRPMS_OPT_GA_FUSED = mode: (tours, keys) as lists."""
    torch = torch_()
    inst = sc.instance(case.kind)
    pops, keys0 = sc.ga_start(case.name)
    ctx.set_ga_fused(mode)
    try:
        dpop = torch.tensor(pops, dtype=torch.int16).to(ctx.dev)
        keys = ctx.eval(dpop.view(case.islands * case.P, inst.n)).view(case.islands, case.P)
        assert u64(keys) == [k for ks in keys0 for k in ks]
        gen0 = case.gen0
        for gens in case.calls:
            ctx.ga_generation(dpop, keys, generations=gens, pmut=case.pmut, seed=case.seed, gen0=gen0)
            gen0 += gens
        return dpop.cpu().tolist(), u64(keys)
    finally:
        ctx.set_ga_fused(0)


def check(ctx, case, fused=True):
    """Mode 0 == mode 2 == the replay.  fused: mode 0 is the fused kernel (the
    instance has the packed layout and the island fits the LDS)."""
    inst = sc.instance(case.kind)
    load(ctx, inst)
    fast = ctx.instance_layout(inst.n)["fast"]
    if fused:
        assert fast and case.P <= 1024
        assert sc.ga_fused_lds(inst.N, inst.n, case.P) <= sc.LDS_BYTES
    rpop, rkeys, _ = sc.ga_replay(case.name)
    rkeys = [k for ks in rkeys for k in ks]
    auto, three = run(ctx, case, 0), run(ctx, case, 2)
    assert auto[1] == three[1] == rkeys
    assert auto[0] == three[0] == rpop
    return fast


@pytest.mark.parametrize("case", sc.GA_GRID, ids=lambda c: c.name)
def test_ga_survivors_match_oracle_on_the_size_grid(ctx, case):
    """2 islands, 4 generations from an unsorted start: a full sort in
    generation 0 (block_sort_pairs for M < 64 and M = 2048, else
    block_sort_pairs_waves), then merge_select_inplace (P <= 256; 1 to 4 runs,
    a last run of one pair at 65, 129, 193), merge_select with idle wavefronts
    (257..960) or without (961..1024).  LDS of ga_fused_layout: 1472 B (n = 5,
    P = 2) to 85152 B (n = 9, P = 1024); over 64 KiB from P = 960 on, all
    inside the 160 KiB the fused kernel may take."""
    check(ctx, case)


@pytest.mark.parametrize("case", sc.GA_ONE, ids=lambda c: c.name)
def test_ga_one_generation_is_the_full_sort_alone(ctx, case):
    """One generation from an unsorted start: only the full-sort paths run
    (M = 32, 64, 1024, 2048, 2048).  LDS: at most 84512 B (n = 5, P = 1024)."""
    check(ctx, case)


@pytest.mark.parametrize("case", sc.GA_HANDIN, ids=lambda c: c.name)
def test_ga_sorted_hand_in_continues_the_trajectory(ctx, case):
    """Two calls of two generations, the second with gen0 advanced: it is handed
    sorted parents and merges from its first generation.  Together they equal
    one replay of four generations.  LDS: at most 82304 B (n = 9, P = 961)."""
    assert case.calls == (2, 2)
    check(ctx, case)


@pytest.mark.parametrize("case", sc.GA_PROBE, ids=lambda c: c.name)
def test_ga_sortedness_probe_per_island(ctx, case):
    """One launch, four islands: sorted, sorted except positions (0, 1), sorted
    except (P - 2, P - 1), all keys equal -- the first and last merge at once,
    the two in the middle must sort first (the probe is a block-wide OR).
    LDS: 21536 B (P = 256) and 84512 B (P = 1024), n = 5."""
    check(ctx, case)


@pytest.mark.parametrize("case", sc.GA_LONG, ids=lambda c: c.name)
def test_ga_long_rows_large_island(ctx, case):
    """n = 80, K = 7, P = 300, 3 generations: two 64-position slots per lane
    (H = 2) with the merge_select that has idle wavefronts.  LDS of
    ga_fused_layout: 128288 B (the packed matrix alone takes 52488 B)."""
    inst = sc.instance(case.kind)
    assert (inst.n + 63) // 64 == 2 and 256 < case.P <= 960
    assert sc.ga_fused_lds(inst.N, inst.n, case.P) == 128288
    check(ctx, case)


@pytest.mark.parametrize("case", sc.GA_PAST, ids=lambda c: c.name)
def test_ga_three_kernel_path_past_the_fused_limit(ctx, case):
    """P > 1024, or an hour-indexed instance: both modes take breed / score /
    ga_select_kernel, so here the oracle alone carries the comparison (mode 0
    == mode 2 only shows the option changes nothing).  n = 9 children travel as
    words (ga_select_kernel<true>), the time-dependent ones as rows (<false>);
    M = 4096 (LDS 48 KiB) and M = 8192 (96 KiB, past the default dynamic-LDS
    limit) at P = 1025, 2048 | 2049, 4096."""
    fast = check(ctx, case, fused=False)
    assert fast == (case.kind != "td")


@pytest.mark.parametrize("P", [1, 4097])
def test_ga_population_outside_the_limits_raises(ctx, P):
    from vrpms_amd._lib import VrpmsError
    torch = torch_()
    inst = sc.instance("n9")
    load(ctx, inst)
    dpop = torch.ones((1, P, inst.n), dtype=torch.int16, device=ctx.dev)
    keys = torch.zeros((1, P), dtype=torch.int64, device=ctx.dev)
    for mode in (0, 2):
        ctx.set_ga_fused(mode)
        try:
            with pytest.raises(VrpmsError):
                ctx.ga_generation(dpop, keys, generations=1, pmut=0.3, seed=1, gen0=0)
        finally:
            ctx.set_ga_fused(0)
    assert (dpop == 1).all() and (keys == 0).all()
