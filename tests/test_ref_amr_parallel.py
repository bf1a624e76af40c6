"""Pins tests/ref_amr_parallel.py on the CPU: the sort-and-index statistics against a literal restatement of the reference's rank walk
(d4est_estimator_stats.c:379-418), and the repartition slices against the global arrays they must tile."""
import numpy as np
import pytest

from tests import ref_amr_parallel as RP


def _values(n, seed):
    """positive values (the rank walk tells a found value by `> 0`) with ties"""
    rng = np.random.RandomState(seed)
    v = rng.uniform(1e-3, 10.0, n)
    v[rng.randint(0, n, n // 5)] = v[0]
    return v


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("G", [100, 137, 1000])
def test_rank_walk_is_sorted_entry_G_minus_k(world, G):
    """G >= 100: k >= 1 for every percentile 1 .. 100"""
    v = _values(G, 7 * G + world)
    s = np.sort(v)
    rng = np.random.RandomState(G + world)
    cuts = np.sort(np.concatenate([[0, G], rng.randint(0, G + 1, world - 1)]))
    uneven = [v[cuts[r]:cuts[r + 1]] for r in range(world)]
    for pct in range(1, 101):
        k = RP.global_id_from_end(G, pct)
        assert 1 <= k <= G
        walked = RP.rank_walk(RP.even_chunks(s, world), pct)
        assert walked is not None and walked == s[G - k], (world, G, pct)
        got = RP.stats_global(uneven, pct)
        assert got[3] == walked and got[2] == s[-1] and got[1] == got[0] / G
        assert abs(got[0] - v.sum()) <= G * 2.0 ** -52 * v.sum()


def test_rank_walk_over_an_empty_rank_and_k_zero():
    v = _values(40, 3)
    s = np.sort(v)
    chunks = [s[:25], s[25:25], s[25:]]
    for pct in (5, 50, 100):
        assert RP.rank_walk(chunks, pct) == s[40 - RP.global_id_from_end(40, pct)]
    # k = 0: the reference aborts (:396); the statistics give -1
    assert RP.global_id_from_end(40, 2) == 0 and RP.rank_walk(chunks, 2) is None
    assert RP.stats_global([v[:10], v[10:]], 2)[3] == -1.0
    assert RP.stats_global([[], []], 5) == (0.0, -1.0, -1.0, -1.0)


def test_the_global_index_is_not_the_one_rank_index():
    """d4est_estimator_stats.c:249 against :379 / :391"""
    from tests import ref_amr as R
    assert R.percentile_index(10, 5) == 9 and 10 - RP.global_id_from_end(10, 5) == 10       # one rank: the maximum; several: no entry
    assert R.percentile_index(200, 10) == 180 and 200 - RP.global_id_from_end(200, 10) == 180


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_repartition_slices_tile_the_global_arrays(world):
    from disco4est_amd import parallel as P
    rng = np.random.RandomState(world)
    deg = rng.randint(1, 5, 41)
    field = rng.uniform(-1, 1, int(((deg + 1) ** 3).sum()))
    old = RP.by_elements(len(deg), world)
    new = RP.first_of(P.partition_by_dofs(deg, world))
    assert np.array_equal(new, P.first_of(P.partition_by_dofs(deg, world)))
    for first in (old, new):
        assert first[0] == 0 and first[-1] == len(deg) and (np.diff(first) >= 0).all()
        assert np.array_equal(np.concatenate(RP.shard_elements(deg, first)), deg)
        assert np.array_equal(np.concatenate(RP.shard_nodes(field, deg, first)), field)
        for sh_d, sh_f in zip(RP.shard_elements(deg, first), RP.shard_nodes(field, deg, first)):
            assert len(sh_f) == int(((sh_d + 1) ** 3).sum())
    # every element is either kept or in exactly one message
    covered = np.zeros(len(deg), dtype=np.int64)
    for s, r, lo, hi in RP.messages(old, new):
        assert s != r and old[s] <= lo < hi <= old[s + 1] and new[r] <= lo < hi <= new[r + 1]
        covered[lo:hi] += 1
    for r in range(world):
        lo, hi = max(old[r], new[r]), min(old[r + 1], new[r + 1])
        if hi > lo:
            covered[lo:hi] += 1
    assert (covered == 1).all()
    assert RP.messages(old, old) == []
