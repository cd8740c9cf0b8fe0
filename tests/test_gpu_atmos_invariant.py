"""FCX_OPT_ATMOS_INVARIANT on the GPU: sharded engines in one process whose shared atmosphere
cells are completed term by term (atmos_terms_kernel, the ordered finish) and must have the BITS
of a one-rank engine over the global grid -- the oracle of every comparison here, the parent's
behaviour, which other tests pin to the sequential SCRIP sum.

The "all-reduce" is that of test_sharded_engines_one_process: total = sum(shared) copied back
into every shard's region; no communicator is involved (tests/test_gpu_atmos_invariant_ranks.py
goes through the product's own exchange).  Bit-identical means equal uint64 views (uint32 for
fp32 outputs).  Every test asserts that an atmosphere cell was actually shared.

test_control_* run the same cases with the option off and require a shared cell whose bits differ
from the one-rank engine's: the defect the option removes is visible to these comparisons.  On a
library without the feature every other test of the file fails for lack of the API."""
import dataclasses
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fcx import _lib  # noqa: E402
from fcx.basic import PHASE_ALL  # noqa: E402
from fcx.engine import Engine  # noqa: E402
from fcx.parallel import (apple_range, boundary_terms, local_atmos, owned_atmos_mask,  # noqa: E402
                          synthetic_atmos_map)
from fcx.synthetic import as_dtype, build_case  # noqa: E402
from test_gpu_multirank import random_run_map  # noqa: E402

FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
N = 20_011
SEED = 911
T_STEP = 7200
PATHS = {"fused": {}, "unfused": {"specialize": 0}, "nohalo": {"atmos_halo": 0},
         "records": {"atm_records": 1, "zero_copy": 0}, "arrays": {"atm_records": 0, "zero_copy": 0}}


# The 3..5-cell map of the N-cell cases.  Its seed is chosen on the host, from the map and the CPU
# oracle's fluxes alone: every APPLE cut of 2, 3, 4 and 8 ranks falls inside an atmosphere cell
# (so each world shares cells), and the cell cut by 2 ranks has two exchange cells on the left
# and three on the right, where (a + b) + (c + d + e) and the sequential sum round differently in
# 4 or 5 of the 6 fields for every variant -- with one cell on the right the two associations are
# the same sum and the control could show nothing.
MAP_SEED = 1245


def shared_map():
    return synthetic_atmos_map(N, seed=MAP_SEED)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def shard_of(full, lo, hi, variant, T, seed):
    """cells [lo, hi) of a float64 case, copied (test_gpu_multirank.shard_case for any T, and
    without aliasing the global arrays)"""
    case = build_case(variant, n=hi - lo, T=T, bias=True, seed=seed)
    moved = {}
    for key, a in full.lf.field.items():
        if id(a) not in moved:
            moved[id(a)] = np.array(np.asarray(a)[lo:hi], copy=True)
        case.lf.field[key] = moved[id(a)]
    init_date, corr = full.corrections
    case.corrections = (init_date, np.ascontiguousarray(corr[lo:hi]))
    return case


class Rig:
    """One engine over `case` and the local map la: atmosphere outputs (surface type `s`), the
    boundary region, the step, the finish."""

    def __init__(self, case, la, T=1, invariant=False, options=None, host_outs=False, output_use=None, region=None,
                 outs=None):
        import torch

        self.case, self.la, self.T = case, la, T
        s = 1 if T == 1 else 0
        dtype = case.lf.dtype
        n_out = max(la.n_atmos, 1)
        if outs is not None:
            self.outs = outs
        elif host_outs:
            self.outs = {name: np.full(n_out, np.nan, dtype=dtype) for name, _ in FIELDS}
        else:
            self.outs = {name: torch.full((n_out,), float("nan"), dtype=getattr(torch, dtype), device="cuda:0")
                         for name, _ in FIELDS}
        self.stride = len(FIELDS) * (1 + la.max_terms) if invariant else len(FIELDS)
        self.region = region if region is not None else torch.zeros(max(la.n_boundaries, 1) * self.stride,
                                                                    dtype=torch.float64, device="cuda:0")
        atmos = {"local": la, "fields": [(2, s, g, name, self.outs[name]) for name, g in FIELDS],
                 "shared": (self.region, self.stride), "invariant": invariant}
        torch.cuda.synchronize()  # the fills above (torch's stream) before the engine's own stream writes
        self.eng = Engine(case.lf, T, case.methods, corrections=case.corrections,
                          averages=case.averages if T > 1 else (), atmos=atmos, options=options or None,
                          output_use=output_use)
        assert self.eng.atmos_invariant() == bool(invariant)
        assert self.eng.atmos_columns() == self.stride

    def run(self):
        self.eng.upload(PHASE_ALL)
        self.eng.run(PHASE_ALL, T_STEP)
        self.eng.synchronize()

    def finish(self, total):
        import torch

        self.region.copy_(total)
        # the copy is queued on torch's stream, the finish on the engine's own (non-blocking)
        # stream: the finish must not read or zero the region before the copy has landed
        torch.cuda.synchronize()
        self.eng.atmos_finish()
        self.eng.synchronize()
        assert float(self.region.abs().sum()) == 0.0, "the whole region is zero after the finish"

    def results(self, fluxes=True):
        """(atmosphere outputs, flux outputs) on the host"""
        self.eng.download(PHASE_ALL)
        self.eng.synchronize()
        atm = {name: (o if isinstance(o, np.ndarray) else o.cpu().numpy())[: self.la.n_atmos].copy()
               for name, o in self.outs.items()}
        flux = {k: np.array(self.case.lf.field[k], copy=True) for k in self.case.outputs} if fluxes else {}
        return atm, flux

    def close(self):
        self.eng.close()


def convert(case, dtype):
    return case if dtype == "float64" else as_dtype(case, dtype)


def one_rank(full, amap, T, dtype, options, host_outs=False):
    """the oracle: ONE engine over the global grid, the option off"""
    rig = Rig(convert(full, dtype), local_atmos(amap, 0, 1), T=T, options=options, host_outs=host_outs)
    rig.eng.step(PHASE_ALL, T_STEP)
    out = rig.results()
    rig.close()
    return out


def sharded(full, amap, ranges, variant, T=1, dtype="float64", invariant=True, options=None, host_outs=False, seed=SEED,
            output_use=None, hook=None):
    """the shards' (LocalAtmos, atmosphere outputs, flux outputs) after one step, slot sum, finish"""
    world = len(ranges)
    rigs = []
    for r, (off, size) in enumerate(ranges):
        la = local_atmos(amap, r, world, ranges=ranges)
        case = convert(shard_of(full, off, off + size, variant, T, seed), dtype)
        rigs.append(Rig(case, la, T=T, invariant=invariant, options=options, host_outs=host_outs, output_use=output_use))
    for rig in rigs:
        rig.run()
    if hook:
        hook(rigs)
    total = sum(rig.region for rig in rigs)
    out = []
    for rig in rigs:
        rig.finish(total)
        out.append((rig.la,) + rig.results(fluxes=output_use is None))
        rig.close()
    return out


def compare(shards, ranges, oracle):
    """[(rank, field, local atmosphere cell)] of the shared cells whose bits differ from the
    one-rank engine's; interior atmosphere cells and every flux output must be bit-identical"""
    atm1, flux1 = oracle
    n_shared, differing = 0, []
    for r, (la, atm, flux) in enumerate(shards):
        if la.size == 0:
            continue
        edge = np.zeros(la.n_atmos, bool)
        edge[0] = la.left >= 0
        edge[-1] = edge[-1] or la.right >= 0
        n_shared += int(edge.sum())
        for name, _ in FIELDS:
            want = atm1[name][la.atmos_offset: la.atmos_offset + la.n_atmos]
            same = bits(atm[name]) == bits(want)
            assert same[~edge].all(), f"rank {r} {name}: an interior atmosphere cell differs"
            differing += [(r, name, int(c)) for c in np.flatnonzero(~same & edge)]
        off, size = ranges[r]
        for k, a in flux.items():
            assert np.array_equal(bits(a), bits(flux1[k][off: off + size])), f"rank {r} flux {k} differs"
    assert n_shared > 0, "no atmosphere cell was shared: the case proves nothing"
    return differing


@functools.lru_cache(maxsize=None)
def global_t1(variant, fused):
    """the T = 1 case of a variant, its map and the one-rank engine's outputs (computed once)"""
    full = build_case(variant, n=N, T=1, bias=True, seed=SEED)
    pristine = {k: np.array(a, copy=True) for k, a in full.lf.field.items()}
    amap = shared_map()
    oracle = one_rank(full, amap, 1, "float64", None if fused else {"specialize": 0})
    for k, a in full.lf.field.items():  # the shards start from the inputs, not from this step's outputs
        np.asarray(a)[:] = pristine[k]
    return full, amap, oracle


def apple(n, world):
    return [apple_range(n, r, world) for r in range(world)]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_worlds_and_variants(variant, world, path):
    """1: every atmosphere cell of every field and every exchange-grid output bit-identical to the
    one-rank engine; fused, unfused, crossing records + fix-up, records on and off"""
    full, amap, oracle = global_t1(variant, path != "unfused")
    ranges = apple(N, world)
    shards = sharded(full, amap, ranges, variant, options=PATHS[path], host_outs=path in ("records", "arrays"))
    assert compare(shards, ranges, oracle) == []


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_control_option_off_differs(variant, world):
    """2: the same cases with the option off: sums of partial sums, so some shared cell's bits
    differ from the one-rank engine's (fixed seed) -- test 1 can see the defect"""
    full, amap, oracle = global_t1(variant, True)
    ranges = apple(N, world)
    differing = compare(sharded(full, amap, ranges, variant, invariant=False), ranges, oracle)
    print(f"{variant} x{world}: {len(differing)} shared (rank, field, cell) differ with the option off")
    assert differing, "with the option off every shared cell happened to round alike: pick another seed"


@pytest.mark.parametrize("lengths", [(20, 64), (130, 140)])
def test_long_segments(lengths):
    """3: 20..64 cells per atmosphere cell (fix-up with recomputed heads) and 130..140 (atmos_kernel),
    3 shards, K from boundary_terms"""
    n, world, variant = 20_003, 3, "CCLM"
    full = build_case(variant, n=n, T=1, bias=True, seed=17)
    amap = random_run_map(n, lengths, seed=lengths[1])
    ranges = apple(n, world)
    k, pos = boundary_terms(ranges, lambda x: amap.atmos_index[x])
    assert lengths[0] <= k <= lengths[1] and max(pos) > 0
    shards = sharded(full, amap, ranges, variant, seed=17)
    assert all(la.max_terms == k and la.left_pos == pos[r] for r, (la, _, _) in enumerate(shards))
    oracle = one_rank(full, amap, 1, "float64", None)
    assert compare(shards, ranges, oracle) == []


def special_ranges(kind, amap):
    """tiny_middle and empty_middle of tests/test_gpu_exchange_ranks.py"""
    idx, n = amap.atmos_index, amap.atmos_index.shape[0]
    if kind == "empty_middle":
        k = next(i for i in range(n // 2, n) if idx[i - 1] == idx[i])
        return [(0, k), (0, 0), (k, n - k)]
    starts = np.flatnonzero(np.diff(np.concatenate([[-1], idx])))  # first cell of each run
    lens = np.diff(np.concatenate([starts, [n]]))
    c0 = int(starts[np.flatnonzero(lens >= 4)[len(starts) // 3 // 2]])
    return [(0, c0 + 1), (c0 + 1, 2), (c0 + 3, n - c0 - 3)]


@pytest.mark.parametrize("kind", ["tiny_middle", "empty_middle"])
def test_rank_inside_one_cell_and_empty_rank(kind):
    """4: a rank whose two cells lie inside one atmosphere cell shared with both neighbours
    (left == right, left_pos > 0 on two ranks), and an empty middle rank"""
    variant = "MOM5"
    full, amap, oracle = global_t1(variant, True)
    ranges = special_ranges(kind, amap)
    shards = sharded(full, amap, ranges, variant)
    las = [la for la, _, _ in shards]
    if kind == "tiny_middle":
        assert las[1].n_atmos == 1 and las[1].left == las[1].right >= 0
        assert las[1].left_pos > 0 and las[2].left_pos > las[1].left_pos
    else:
        assert las[1].size == 0 and las[0].right == las[2].left >= 0 and las[2].left_pos > 0
    assert compare(shards, ranges, oracle) == []


@pytest.mark.parametrize("path", ["fused", "unfused"])
def test_two_surface_types_register_averages(path):
    """5: water + ice, the type-0 averages accumulated, 3 shards"""
    n, world, variant, T = 20_011, 3, "CCLM", 2
    full = build_case(variant, n=n, T=T, bias=True, seed=913)
    amap = shared_map()
    ranges = apple(n, world)
    shards = sharded(full, amap, ranges, variant, T=T, options=PATHS[path], seed=913)
    oracle = one_rank(full, amap, T, "float64", PATHS[path])
    assert compare(shards, ranges, oracle) == []


@pytest.mark.parametrize("kind", ["f32", "f32_math", "cr_math"])
def test_fp32_and_cr_engines(kind):
    """6: a plain fp32 engine, FCX_OPT_F32_MATH, and an fp64 engine with FCX_OPT_CR_MATH, 2 shards:
    rounded once from the ordered fp64 sum, the bits of the one-rank engine of the same kind"""
    n, world, variant = 20_011, 2, "CCLM"
    dtype = "float64" if kind == "cr_math" else "float32"
    options = {"f32": None, "f32_math": {"f32_math": 1}, "cr_math": {"cr_math": 1}}[kind]
    full = build_case(variant, n=n, T=1, bias=True, seed=SEED)
    amap = shared_map()
    ranges = apple(n, world)
    shards = sharded(full, amap, ranges, variant, dtype=dtype, options=options)
    assert all(a.dtype == np.dtype(dtype) for _, atm, _ in shards for a in atm.values())
    oracle = one_rank(full, amap, 1, dtype, options)
    assert compare(shards, ranges, oracle) == []


def test_zero_wind_minus_zero_terms():
    """7: UATM = VATM = 0 on every exchange cell of one shared atmosphere cell: the UMOM and VMOM
    terms are -0.0 there, arrive as +0.0 through the sum, and the ordered sum from +0.0 has the
    one-rank engine's bits all the same"""
    n, world, variant = 20_011, 2, "CCLM"
    full = build_case(variant, n=n, T=1, bias=True, seed=SEED)
    amap = shared_map()
    ranges = apple(n, world)
    cut = ranges[1][0]
    cell = amap.atmos_index[cut]
    assert amap.atmos_index[cut - 1] == cell  # the cut lies inside it
    cells = np.flatnonzero(amap.atmos_index == cell)
    done = set()
    for (s, g, name), a in full.lf.field.items():
        if name in ("UATM", "VATM") and id(a) not in done:
            done.add(id(a))
            np.asarray(a)[cells] = 0.0
    seen = {}

    def hook(rigs):  # the terms of the shared cell as the shards stored them
        for rig in rigs:
            seen[rig.la.offset] = rig.region.cpu().numpy().reshape(rig.la.n_boundaries, rig.stride).copy()

    shards = sharded(full, amap, ranges, variant, hook=hook)
    k = shards[0][0].max_terms
    for col in (4, 5):  # UMOM, VMOM: every stored term of the cell is a zero, some of them -0.0
        terms = np.concatenate([reg[0, len(FIELDS) + col * k: len(FIELDS) + (col + 1) * k] for reg in seen.values()])
        assert not terms.any()
    minus = sum(int(np.signbit(reg[0, len(FIELDS) + 4 * k: len(FIELDS) + 6 * k]).sum()) for reg in seen.values())
    print(f"zero wind: {minus} of the shared cell's momentum terms are -0.0")
    assert minus > 0, "no -0.0 term was formed: the case does not cover the sign of zero"
    oracle = one_rank(full, amap, 1, "float64", None)
    assert compare(shards, ranges, oracle) == []
    la1, atm1, _ = shards[1]
    assert la1.left >= 0 and bits(atm1["UMOM"])[0] == bits(oracle[0]["UMOM"])[cell]


def test_unread_accumulated_fields_keep_their_store():
    """8: the accumulated T = 1 fields declared FCX_OUT_UNREAD: with the option on fcx_output_info
    reports them stored (1, FCX_OUT_DEVICE behaviour; without it 2, the store is dropped), and the
    atmosphere results are those of case 1"""
    variant, world = "MOM5", 3
    full, amap, oracle = global_t1(variant, True)
    ranges = apple(N, world)
    use = {(1, g, name): "unread" for name, g in FIELDS}
    infos = {}
    for invariant in (True, False):
        la = local_atmos(amap, 1, world, ranges=ranges)
        off, size = ranges[1]
        rig = Rig(shard_of(full, off, off + size, variant, 1, SEED), la, invariant=invariant, output_use=use)
        rig.run()
        infos[invariant] = {name: rig.eng.output_info(1, g, name) for name, g in FIELDS}
        rig.close()
    assert set(infos[True].values()) == {1}, infos[True]
    assert 2 in infos[False].values(), infos[False]  # the parent's behaviour: some store is dropped
    shards = sharded(full, amap, ranges, variant, output_use=use)
    assert compare(shards, ranges, oracle) == []


def test_guard_bands():
    """9: the boundary region and the atmosphere outputs carved out of one allocation between
    sentinel bands: the terms launch and the finish write nothing outside [n_boundaries][stride]
    and the outputs' cells"""
    import torch
    from guards import GuardedArena

    variant, world, rank = "CCLM", 3, 1
    full, amap, oracle = global_t1(variant, True)
    ranges = apple(N, world)
    la = local_atmos(amap, rank, world, ranges=ranges)
    assert la.left >= 0 and la.right >= 0
    stride = len(FIELDS) * (1 + la.max_terms)
    cells = la.n_boundaries * stride
    off, size = ranges[rank]
    case = shard_of(full, off, off + size, variant, 1, SEED)
    # every field array 3 sentinel cells longer than its grid, the region and the atmosphere
    # outputs exactly their length, bands between all of them
    arena = GuardedArena.for_case(case, "torch", extra=[cells] + [la.n_atmos] * len(FIELDS), tail=3)
    region = arena.empty(cells, "region", tail=0)
    region.zero_()
    outs = {name: arena.empty(la.n_atmos, ("atm", name), tail=0) for name, _ in FIELDS}
    arena.snapshot()
    rig = Rig(case, la, invariant=True, region=region, outs=outs)
    rig.run()  # the flux launch, the terms launch
    torch.cuda.synchronize()
    assert arena.check() == []
    terms = region.cpu().numpy().reshape(la.n_boundaries, stride)
    assert terms[la.left, len(FIELDS):].any() and terms[la.right, len(FIELDS):].any()
    rig.finish(region.clone())  # (this rank's terms alone: the bounds are what is checked)
    assert arena.check() == []
    atm = {name: o.cpu().numpy().copy() for name, o in outs.items()}
    flux = arena.outputs(case)
    rig.close()
    for k, a in flux.items():  # the flux outputs are untouched by the option
        assert np.array_equal(bits(a), bits(oracle[1][k][off: off + size])), k
    inner = slice(1, la.n_atmos - 1)
    for name, _ in FIELDS:
        want = oracle[0][name][la.atmos_offset: la.atmos_offset + la.n_atmos]
        assert np.array_equal(bits(atm[name][inner]), bits(want[inner])), name
    arena.close()


def test_budgets_merge_to_the_one_rank_bytes():
    """10: fcx_atmos_integrals of 3 shards merged (fcx_sum_merge), areas by the owned_atmos_mask
    rule, against the one-rank engine's struct for every accumulated field.

    A cell shared by two ranks is summed on both, with area 0.0 on the rank that does not own it
    (fcx_set_atmos_areas): a zero term, and n_terms counts zeros by its definition (fcx.h: "the
    finite terms (zeros included) ... add up to the cells summed").  So the merged struct equals
    the one-rank engine's in its 68 limbs and its three non-finite counts -- 568 of the 576 bytes,
    everything the value is made of -- and its n_terms is larger by exactly the number of such
    second holdings, which is asserted too."""
    variant, world = "RCO", 3
    full, amap, _ = global_t1(variant, True)
    area = np.random.default_rng(5).uniform(0.5, 1.5, amap.n_atmos)
    ranges = apple(N, world)
    one = Rig(shard_of(full, 0, N, variant, 1, SEED), local_atmos(amap, 0, 1))
    one.eng.set_atmos_areas(area)
    one.run()
    want = one.eng.atmos_integrals(PHASE_ALL)
    one.close()
    assert len(want) == len(FIELDS) and all(len(bytes(s)) == 576 for s in want)
    merged, dup = {}, 0
    for invariant in (True, False):
        rigs = []
        for r, (off, size) in enumerate(ranges):
            la = local_atmos(amap, r, world, ranges=ranges)
            rig = Rig(shard_of(full, off, off + size, variant, 1, SEED), la, invariant=invariant)
            rig.eng.set_atmos_areas(area[la.atmos_offset: la.atmos_offset + la.n_atmos] * owned_atmos_mask(la))
            rig.run()
            rigs.append(rig)
        dup = sum(int(rig.la.left >= 0) for rig in rigs)
        assert dup > 0
        total = sum(rig.region for rig in rigs)
        sums = None
        for rig in rigs:
            rig.finish(total)
            part = rig.eng.atmos_integrals(PHASE_ALL)
            sums = part if sums is None else [a + b for a, b in zip(sums, part)]
            rig.close()
        merged[invariant] = sums
    for (name, _), s, w in zip(FIELDS, merged[True], want):
        assert np.array_equal(s.words()[:68], w.words()[:68]), f"{name}: the limbs differ"
        assert (s.n_nan, s.n_pinf, s.n_ninf) == (w.n_nan, w.n_pinf, w.n_ninf) == (0, 0, 0), name
        assert w.n_terms == amap.n_atmos and s.n_terms == w.n_terms + dup, (name, s.n_terms, w.n_terms, dup)
        assert bits(np.array([s.value]))[0] == bits(np.array([w.value]))[0], name
    off = sum(not np.array_equal(s.words()[:68], w.words()[:68]) for s, w in zip(merged[False], want))
    print(f"budget fields whose limbs differ from the one-rank engine's with the option off: {off} of {len(FIELDS)}")



def test_argument_errors():
    """11: each refusal names what is wrong (fcx_commit; tests/test_atmos_invariant_abi.py has the
    same from fcx_plan_check without a GPU), and the option is FCX_E_STATE after commit"""
    variant, world = "CCLM", 2
    full, amap, _ = global_t1(variant, True)
    ranges = apple(N, world)
    la = local_atmos(amap, 1, world, ranges=ranges)
    off, size = ranges[1]
    case = shard_of(full, off, off + size, variant, 1, SEED)
    own = int(np.count_nonzero(la.atmos_index == 0))

    def refused(la_bad, *words, region=None):
        with pytest.raises(_lib.FcxError) as ex:
            Rig(case, la_bad, invariant=True, region=region).close()
        assert ex.value.status == 1, str(ex.value)  # FCX_E_ARG
        for w in words:
            assert w in str(ex.value), str(ex.value)

    assert la.left_pos > 0
    refused(dataclasses.replace(la, max_terms=la.left_pos + own - 1), f"left_pos {la.left_pos}", f"{own} exchange cells",
            f"max_terms {la.left_pos + own - 1}")
    refused(dataclasses.replace(la, max_terms=4097), "max_terms 4097", "4096")
    import torch

    # a caller stride one column short of fields x (1 + K)
    stride = len(FIELDS) * (1 + la.max_terms) - 1
    buf = torch.zeros(la.n_boundaries * (stride + 1), dtype=torch.float64, device="cuda:0")
    outs = {name: torch.zeros(la.n_atmos, dtype=torch.float64, device="cuda:0") for name, _ in FIELDS}
    with pytest.raises(_lib.FcxError) as ex:
        Engine(case.lf, 1, case.methods, corrections=case.corrections,
               atmos={"local": la, "fields": [(2, 1, g, name, outs[name]) for name, g in FIELDS],
                      "shared": (buf, stride), "invariant": True}).close()
    assert ex.value.status == 1 and f"stride {stride}" in str(ex.value) and f"max_terms {la.max_terms}" in str(ex.value)
    perm = np.random.default_rng(5).permutation(la.n_atmos).astype(np.int32)
    unsorted = dataclasses.replace(la, atmos_index=perm[la.atmos_index], left=-1, right=-1)
    refused(unsorted, "sorted atmosphere map", "unsorted")
    rig = Rig(case, la, invariant=True)
    try:
        assert rig.eng.lib.fcx_set_option(rig.eng.h, _lib.FCX_OPT_ATMOS_INVARIANT, 0) == 2  # FCX_E_STATE
        assert rig.eng.atmos_invariant()
        assert rig.eng.lib.fcx_set_atmos_terms(rig.eng.h, 8, 0) == 2
    finally:
        rig.close()
