"""fcx.parallel.boundary_terms (FCX_OPT_ATMOS_INVARIANT): max_terms and every rank's left_pos
against a brute-force count, on random maps and ranges with empty ranks, ranks inside one
atmosphere cell and cells spread over three or more ranks; LocalAtmos keeps its constructor."""
import numpy as np
import pytest

from fcx.parallel import (AtmosMap, BlockedRandomAtmosMap, LocalAtmos, PeriodicAtmosMap, apple_range, boundary_slots,
                          boundary_terms, local_atmos, synthetic_atmos_map)


def brute(ranges, idx):
    """by definition: per rank, the cells of its first atmosphere cell below its offset (ranges
    are contiguous in rank order); K over the atmosphere cells held by two or more ranks"""
    left_pos, holders = [], {}
    for off, size in ranges:
        if size == 0:
            left_pos.append(0)
            continue
        left_pos.append(int(np.count_nonzero(idx[:off] == idx[off])))
        for a in np.unique(idx[off: off + size]):
            holders[int(a)] = holders.get(int(a), 0) + 1
    counts = np.bincount(idx)
    shared = [int(counts[a]) for a, h in holders.items() if h >= 2]
    return max(shared + [1]), left_pos, len(shared)


def random_map(rng, n, lo, hi):
    runs = rng.integers(lo, hi + 1, n)
    idx = np.repeat(np.arange(n, dtype=np.int32), runs)[:n]
    return np.ascontiguousarray(idx)


def random_ranges(rng, n, world, p_empty):
    cuts = np.sort(rng.integers(0, n + 1, world - 1))
    for k in range(world - 1):  # some ranks empty
        if k and rng.random() < p_empty:
            cuts[k] = cuts[k - 1]
    edges = np.concatenate([[0], cuts, [n]])
    return [(int(edges[k]), int(edges[k + 1] - edges[k])) for k in range(world)]


@pytest.mark.parametrize("seed", range(40))
def test_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 400))
    lo, hi = [(1, 5), (1, 40), (3, 3), (20, 64)][seed % 4]
    idx = random_map(rng, n, lo, hi)
    world = int(rng.integers(1, 9))
    ranges = random_ranges(rng, n, world, 0.3)
    k, pos = boundary_terms(ranges, lambda x: idx[x])
    want_k, want_pos, _ = brute(ranges, idx)
    assert (k, pos) == (want_k, want_pos), (ranges, idx.tolist())


def test_cells_over_many_ranks_and_empty_ranks():
    """one atmosphere cell of 11 exchange cells cut by five ranks, two of them empty, a rank of
    one cell and a rank of two inside it"""
    idx = np.array([0, 0, 0] + [1] * 11 + [2, 2, 3], np.int32)
    ranges = [(0, 5), (5, 0), (5, 1), (6, 2), (8, 0), (8, 9)]
    k, pos = boundary_terms(ranges, lambda x: idx[x])
    assert k == 11 and pos == [0, 0, 2, 3, 0, 5]
    assert brute(ranges, idx)[:2] == (k, pos)
    slots = boundary_slots(ranges, lambda x: idx[x])
    assert slots[2][0] == slots[2][1] == slots[3][0] == slots[3][1] >= 0  # ranks inside the cell: one slot
    amap = AtmosMap(idx, np.ones(idx.size), 4)
    for r in range(len(ranges)):
        la = local_atmos(amap, r, len(ranges), ranges=ranges)
        assert la.max_terms == 11 and la.left_pos == pos[r]


def test_nothing_shared():
    idx = np.repeat(np.arange(6, dtype=np.int32), 4)
    ranges = [(0, 8), (8, 8), (16, 8)]
    assert boundary_terms(ranges, lambda x: idx[x]) == (1, [0, 0, 0])
    assert boundary_terms([(0, 24)], lambda x: idx[x]) == (1, [0])
    assert boundary_terms([(0, 0), (0, 0)], lambda x: idx[x]) == (1, [0, 0])


@pytest.mark.parametrize("world", [2, 3, 8])
def test_local_atmos_fills_both(world):
    n = 24_012
    amap = synthetic_atmos_map(n)
    ranges = [apple_range(n, r, world) for r in range(world)]
    want_k, want_pos, shared = brute(ranges, amap.atmos_index)
    assert shared > 0
    for r in range(world):
        la = local_atmos(amap, r, world)  # APPLE ranges
        assert (la.max_terms, la.left_pos) == (want_k, want_pos[r])
        assert (la.left >= 0) == (la.left_pos > 0)
        # an explicit range without the others: left_pos from the map, K not worked out
        lb = local_atmos(amap, r, world, *ranges[r])
        assert (lb.max_terms, lb.left_pos) == (0, want_pos[r])
    for m in (PeriodicAtmosMap(), BlockedRandomAtmosMap()):
        g = m.global_map(n)
        k, pos, _ = brute(ranges, g.atmos_index)
        for r in range(world):
            la = m.local(*ranges[r], r, world, n, ranges=ranges)
            assert (la.max_terms, la.left_pos) == (k, pos[r])
            assert (m.local(*ranges[r], r, world, n).max_terms, m.local(*ranges[r], r, world, n).left_pos) == (0, 0)


def test_empty_rank_carries_max_terms_in_every_map_class():
    """a rank without cells between two that share an atmosphere cell: its LocalAtmos has the run's
    K (it takes part in the exchange with slots of the same width), from local_atmos and from the
    two structured maps alike"""
    n = 4096 + 37
    for m in (PeriodicAtmosMap(), BlockedRandomAtmosMap()):
        g = m.global_map(n)
        cut = next(i for i in range(n // 2, n) if g.atmos_index[i - 1] == g.atmos_index[i])
        ranges = [(0, cut), (0, 0), (cut, n - cut)]
        k, pos, shared = brute(ranges, g.atmos_index)
        assert shared == 1 and k >= 3
        for r in range(3):
            la = m.local(*ranges[r], r, 3, n, ranges=ranges)
            lb = local_atmos(g, r, 3, ranges=ranges)
            assert (la.max_terms, la.left_pos) == (lb.max_terms, lb.left_pos) == (k, pos[r]), (type(m).__name__, r)
        assert m.local(0, 0, 1, 3, n).max_terms == 0  # without the ranges K is not worked out


def test_local_atmos_constructor_unchanged():
    """the nine positional fields of existing callers still build a LocalAtmos; the new ones
    come last and default to 0"""
    la = LocalAtmos(0, 4, 0, 2, np.zeros(4, np.int32), np.ones(4), -1, -1, 0)
    assert (la.left_pos, la.max_terms) == (0, 0)
    names = [f.name for f in LocalAtmos.__dataclass_fields__.values()]
    assert names == ["offset", "size", "atmos_offset", "n_atmos", "atmos_index", "weight", "left", "right",
                     "n_boundaries", "left_pos", "max_terms"]
    empty = local_atmos(synthetic_atmos_map(100), 1, 3, ranges=[(0, 50), (50, 0), (50, 50)])
    assert empty.size == 0 and empty.left_pos == 0 and empty.max_terms >= 1
