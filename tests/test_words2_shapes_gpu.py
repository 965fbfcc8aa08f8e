"""eval_cvrp_words2 at the edges of its workgroup shapes.

launch_words2 runs the kernel as one 1024-lane workgroup per CU or, when two
copies of the packed matrix fit the LDS, as two workgroups of 768 or 1024
lanes; every lane scores two candidates, so a workgroup pass covers 1536 or
2048 tours.  The cases sit on the last lane, the second candidate of a lane
re-pointed past the end, one tour into the next workgroup and several passes
per workgroup, for both sizes, so they hold whichever shape the launcher
picks.  Bar: keys, durationSum, durationMax and unvisited equal the C oracle's
through the public path (to_words + eval_words).
"""
import dataclasses

import numpy as np
import pytest

from vrpms_amd import synth

pytestmark = pytest.mark.gpu

EDGES = [1, 767, 768, 769, 1023, 1025, 1535, 1537, 2047, 2049]


def _torch():
    import torch
    return torch


@pytest.fixture
def wctx(ctx):
    """The session context; the lookahead option is back on auto afterwards."""
    yield ctx
    ctx.set_words_lookahead(0)


def load(ctx, inst, objective=0):
    from vrpms_amd.core import CVRP
    ctx.set_instance(CVRP, inst.durations, inst.demand, inst.capacities, inst.start_times,
                     objective=objective)


def reference(coracle, inst, P, objective=0):
    return coracle.eval_batch(inst.durations, P, inst.demand, inst.capacities, inst.start_times,
                              problem=1, objective=objective, n=inst.n)


def check(ctx, inst, dP, ref, objective=0):
    """dP: the tours on the device; ref: the oracle's four arrays for them."""
    load(ctx, inst, objective)
    words = ctx.to_words(dP, n=inst.n)
    keys, sums, maxs, unv = ctx.eval_words(words, inst.n, with_parts=True)
    np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), ref[0])
    np.testing.assert_array_equal(sums.cpu().numpy(), ref[1])
    np.testing.assert_array_equal(maxs.cpu().numpy(), ref[2])
    np.testing.assert_array_equal(unv.cpu().numpy(), ref[3])


@pytest.fixture(scope="module")
def edge_case(coracle):
    """CVRP-100, K = 8: 2049 tours and the oracle's result per objective;
    every edge size is a prefix of them."""
    inst = synth.cvrp(100, 8, seed=21)
    P = synth.random_perms(max(EDGES), inst.n, seed=22)
    return inst, P, {obj: reference(coracle, inst, P, obj) for obj in (0, 1)}


@pytest.mark.parametrize("C", EDGES)
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("la", [0, 1, 2])
def test_workgroup_edges(wctx, edge_case, la, objective, C):
    inst, P, refs = edge_case
    wctx.set_words_lookahead(la)
    dP = _torch().from_numpy(P[:C]).to(wctx.dev)
    check(wctx, inst, dP, [r[:C] for r in refs[objective]], objective)


@pytest.mark.parametrize("n,K", [(100, 8), (9, 3)])
def test_several_passes_per_workgroup(wctx, coracle, n, K):
    """More tours than two rounds of the full grid, with a ragged last pass.
    The batch draws each position's tour from 65536 scored ones, so a pass
    that read or wrote another pass's rows shows.  n = 9: no block of full
    words, a partial last word, the tail path only."""
    torch = _torch()
    cus = torch.cuda.get_device_properties(wctx.dev).multi_processor_count
    C = 2 * cus * 2048 + 1537
    inst = synth.cvrp(n, K, seed=n)
    base = synth.random_perms(1 << 16, inst.n, seed=n + 1)
    ref = reference(coracle, inst, base)
    idx = np.random.default_rng(n + 2).integers(0, base.shape[0], size=C)
    d_idx = torch.from_numpy(idx).to(wctx.dev)
    dP = torch.from_numpy(base).to(wctx.dev)[d_idx].contiguous()
    check(wctx, inst, dP, [r[idx] for r in ref])


@pytest.mark.parametrize("n,K", [(110, 9), (101, 9), (100, 9)])
@pytest.mark.parametrize("la", [0, 1, 2])
def test_one_and_two_table_copies(wctx, coracle, n, K, la):
    """Either side of the rule for two workgroups per CU.  N = n + 1 = 111
    and 102: two copies of the matrix (2 * 8 N^2 bytes) do not fit 160 KiB
    of LDS, 102 by 2.6 KB; N = 101 is the largest at which they do."""
    inst = synth.cvrp(n, K, seed=n + 3)
    wctx.set_words_lookahead(la)
    P = synth.random_perms(4097, inst.n, seed=la)
    check(wctx, inst, _torch().from_numpy(P).to(wctx.dev), reference(coracle, inst, P))


@pytest.mark.parametrize("slack", [0.9, 1.0])
@pytest.mark.parametrize("la", [0, 1, 2])
def test_exact_rewalk_under_tight_fleet(wctx, coracle, la, slack):
    """A fleet too small for the demand (slack 0.9: every tour) or barely
    enough (1.0: most tours, a wave mixes both): the lanes that met the fleet
    limit are re-walked exactly (redo_exact) and leave customers unvisited."""
    inst = synth.cvrp(100, 8, seed=23, slack=slack)
    wctx.set_words_lookahead(la)
    P = synth.random_perms(1537, inst.n, seed=24)
    ref = reference(coracle, inst, P, objective=la % 2)
    assert (ref[3] > 0).any(), "the instance must exhaust the fleet on some tour"
    check(wctx, inst, _torch().from_numpy(P).to(wctx.dev), ref, objective=la % 2)


@pytest.mark.parametrize("la", [0, 1, 2])
def test_zero_demand_step(wctx, coracle, la):
    """Zero-demand customers: the compare form of the split step, not the
    carry form."""
    inst = synth.cvrp(100, 8, seed=25)
    dem = inst.demand.copy()
    dem[1::7] = 0
    inst = dataclasses.replace(inst, demand=dem)
    wctx.set_words_lookahead(la)
    P = synth.random_perms(1537, inst.n, seed=26)
    check(wctx, inst, _torch().from_numpy(P).to(wctx.dev), reference(coracle, inst, P))
