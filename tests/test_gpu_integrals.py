"""Exact field integrals on the device (fcx_field_integrals, fcx_atmos_integrals) against their
host twin (fcx_sum_add_terms on the same arrays).  Every comparison is of the 576 bytes of the
canonical fcx_exact_sum: there is no tolerance anywhere but in the conservation test, whose
bound is derived in its docstring.  The shapes are the range tests': lane, wave and layout-tile
edges, two blocks, tile-blocked mirrors at 8200 cells."""
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import received  # noqa: E402
from guards import GuardedArena  # noqa: E402
from fcx import _lib  # noqa: E402
from fcx.basic import PHASE_ALL, PHASE_EARLY, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, ExactSum  # noqa: E402
from fcx.parallel import apple_range, local_atmos, synthetic_atmos_map  # noqa: E402
from fcx.synthetic import as_dtype, build_case  # noqa: E402

STEP_T = 3600
TAIL = 37
SIZES = (1, 3, 127, 128, 129, 4095, 4096, 4097, 8200)
MIRRORS = {"zero_copy": 0}  # device mirrors of the host arrays (tile-blocked from two tiles on)
APART = (1, 64, 256, 4096)  # cancelling partners in different lanes, waves, blocks and tiles
ATM = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))


def engine_of(case, **kw):
    return Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                  averages=case.averages, **kw)


def typed(case, dtype):
    return as_dtype(case, "float32") if dtype == "float32" else case


def same(got, want, label):
    assert bytes(got) == bytes(want), (label, got, want)


def areas_for(n, rng):
    """positive, negative and zero areas (all are allowed), at least n + TAIL of them; past n: NaN-free
    junk the engine must not keep"""
    a = rng.uniform(0.5, 2.0, n + TAIL)
    a[rng.integers(0, n)] = 0.0
    a[rng.integers(0, n)] *= -1.0
    a[n:] = 1e300
    return a


def patterns(n, dtype, rng):
    """(label, values[n]).  fp32 patterns use the float formats' own ranges."""
    f32 = dtype == "float32"
    big, tiny, emin, emax = (3e38, 1e-45, -149, 127) if f32 else (1e308, 5e-324, -1074, 1023)
    base = rng.uniform(-1.0, 1.0, n).astype(dtype)
    yield "uniform", base
    with np.errstate(over="ignore", under="ignore"):
        yield "exponents", np.ldexp(rng.uniform(-1.0, 1.0, n), rng.integers(emin, emax + 1, n)).astype(dtype)
    yield "denormals", (rng.integers(-1000, 1000, n) * tiny).astype(dtype)
    z = np.zeros(n, dtype)
    z[::2] = -0.0
    yield "zeros", z
    for d in APART:
        for p in sorted({0, max(n - d - 2, 0), 4095 - (d > 1)}):
            if p + d >= n:
                continue
            one = p + d + 1 if p + d + 1 < n else None  # (no room: the pair alone, a sum of +0.0)
            x = np.zeros(n, dtype)
            x[p], x[p + d] = big, -big
            if one is not None:
                x[one] = 1.0
            yield f"big+1-big@{p}+{d}", x
            x = base.copy()
            x[p], x[p + d] = 1e16, -1e16
            if one is not None:
                x[one] = 1.0
            yield f"1e16@{p}+{d}", x
    x = base.copy()
    x[:: max(n // 7, 1)] = big  # a sum beyond the format's largest number
    yield "overflow", x
    for v in (np.nan, np.inf, -np.inf):
        x = base.copy()
        x[[0, n // 2, n - 1]] = v
        yield f"{v}", x
    x = base.copy()
    x[0], x[n - 1] = np.inf, (np.nan if n > 1 else np.inf)
    x[n // 2] = -np.inf if n > 2 else x[n // 2]
    yield "mixed non-finite", x


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_twin(n, dtype, weighted):
    """Device-bound fields carved out of one guarded allocation, TAIL sentinel cells (NaN) longer
    than their grid; QATM starts 8 (fp32: 4) bytes off a 16-B boundary, so it is read value by
    value.  Every pattern in TSUR, 16 more slots in the same request (17 fields: two launches)."""
    case = typed(build_case("CCLM", n=n, T=1), dtype)
    rng = np.random.default_rng(1000 + n)
    arena = GuardedArena.for_case(case, "torch", tail=TAIL, offset=8 if dtype == "float64" else 4,
                                  only=(0, 1, "QATM"))
    eng = engine_of(case)
    try:
        area = areas_for(n, rng)
        for g in (1, 2, 3):
            eng.set_areas(g, area)
        a = area[:n] if weighted else None
        others = [k for k in case.lf.field if k[2] != "TSUR" and k not in case.outputs][:16]
        assert len(others) == 16 and (1, 1, "QATM") in others
        slots = [(1, 1, "TSUR")] + others
        for k in others:
            x = np.ldexp(rng.uniform(-1.0, 1.0, n), rng.integers(-60, 60, n)).astype(dtype)
            x[rng.integers(0, n)] = rng.choice([np.nan, np.inf, 9.0])
            arena._store(arena.region(next(r.key for r in arena.regions
                                           if case.lf.field[r.key] is case.lf.field[k])), x)
        want_others = [ExactSum.of(arena.host(case.lf.field[k], n), a) for k in others]
        arena.snapshot()
        tsur = arena.region((1, 1, "TSUR"))
        for label, x in patterns(n, dtype, rng):
            arena._store(tsur, x)
            got = eng.field_integrals(slots, weighted=weighted)
            want = ExactSum.of(x, a)
            same(got[0], want, (n, dtype, weighted, label))
            assert got[0].n_terms + got[0].n_nan + got[0].n_pinf + got[0].n_ninf == n
            if not weighted and label.startswith("big+1-big"):
                assert got[0].value == (1.0 if (x == 1.0).any() else 0.0)
            for k, g_, w_ in zip(others, got[1:], want_others):
                same(g_, w_, (n, dtype, weighted, label, k))
        assert eng.field_integrals([]) == []
        arena._store(tsur, np.ones(n, dtype))
        arena.snapshot()
        eng.field_integrals(slots, weighted=weighted)
        assert arena.check() == []  # no band and no field was written
    finally:
        eng.close()
        arena.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_more_partials_than_the_finishing_launch_has_groups(dtype):
    """61,445 cells are 16 layout tiles: 16 blocks with one field in the launch, where the first
    two of the finishing launch's 14 groups take two partials each.  A negative total borrows
    through every higher limb."""
    n = 15 * 4096 + 5
    case = typed(build_case("CCLM", n=n, T=1), dtype)
    rng = np.random.default_rng(14)
    area = rng.uniform(0.5, 2.0, n)
    emin, emax = (-149, 127) if dtype == "float32" else (-1074, 1023)
    with np.errstate(over="ignore", under="ignore"):
        fields = {"TSUR": np.ldexp(rng.uniform(-1.0, 1.0, n), rng.integers(emin, emax + 1, n)).astype(dtype),
                  "PATM": -np.abs(rng.uniform(1.0, 2.0, n)).astype(dtype),
                  "QATM": rng.uniform(-1.0, 1.0, n).astype(dtype)}
    for name, x in fields.items():
        case.lf.field[(1, 1, name)][:] = x
    eng = engine_of(case, options=MIRRORS)
    try:
        eng.set_areas(1, area)
        eng.upload(PHASE_ALL)
        eng.synchronize()
        for weighted in (True, False):
            for name, x in fields.items():
                got = eng.field_integrals([(1, 1, name)], weighted=weighted)[0]
                same(got, ExactSum.of(x, area if weighted else None), (dtype, weighted, name))
        assert eng.field_integrals([(1, 1, "PATM")], weighted=False)[0].value < 0.0
    finally:
        eng.close()


def _after_step(case, options, areas, arena=False, weighted=True):
    """{slot: ExactSum} of every input and output of the step == the twin on the host arrays"""
    keep = None
    if arena:
        from fcx.host_alloc import Arena

        keep = Arena()
        keep.adopt(case.lf)
    eng = engine_of(case, options={**options, "check_finite": 3})
    try:
        for g in (1, 2, 3):
            eng.set_areas(g, areas)
        eng.step(PHASE_ALL, STEP_T)
        slots = eng.check_fields(PHASE_ALL)
        assert set(case.outputs) <= set(slots)
        got = eng.field_integrals(slots, weighted=weighted)
        for k, g in zip(slots, got):
            n = case.lf.grid_size[k[1] - 1]
            same(g, ExactSum.of(np.asarray(case.lf.field[k])[:n], areas[:n] if weighted else None), (options, k))
        return dict(zip(slots, got)), eng.device_layout(), eng.zero_copy_active()
    finally:
        eng.close()
        if keep is not None:
            keep.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_layouts_give_the_same_bytes(dtype):
    """The same data in tile-blocked mirrors (three tiles), contiguous mirrors, zero-copy through
    the staging arena, library memory in place and library memory moved by spans."""
    def case():
        return typed(build_case("MOM5", n=8200, T=2, bias=True), dtype)

    areas = np.random.default_rng(5).uniform(0.5, 2.0, 8200)
    tiled, (tile, stride), zc = _after_step(case(), MIRRORS, areas)
    assert stride > tile and not zc
    flat, (tile, stride), zc = _after_step(case(), {**MIRRORS, "tiled_layout": 0}, areas)
    assert stride == tile and not zc
    staged, _, _ = _after_step(case(), {"zero_copy": 1}, areas)
    inplace, (tile, stride), zc = _after_step(case(), {"zero_copy": 1}, areas, arena=True)
    assert stride == tile and zc
    spans, _, _ = _after_step(case(), {"zero_copy": 0}, areas, arena=True)
    for other in (flat, staged, inplace, spans):
        assert other.keys() == tiled.keys()
        for k in tiled:
            same(other[k], tiled[k], k)
    _after_step(case(), MIRRORS, areas, weighted=False)


def test_separate_grids_use_each_grids_size_and_areas():
    case = build_case("CCLM", n=4100, T=1, sep_grids=(4097, 130))
    rng = np.random.default_rng(6)
    areas = [rng.uniform(0.5, 2.0, n) for n in case.lf.grid_size]
    eng = engine_of(case, options=MIRRORS)
    try:
        eng.step(PHASE_ALL, STEP_T)
        with pytest.raises(_lib.FcxError) as ex:
            eng.field_integrals([(1, 2, "UMOM")])
        assert ex.value.status == 2 and "exchange grid u" in str(ex.value)
        for g in (1, 2, 3):
            eng.set_areas(g, areas[g - 1])
        slots = [(1, 1, "HSEN"), (1, 2, "UMOM"), (1, 3, "VMOM")]
        for k, got in zip(slots, eng.field_integrals(slots)):
            same(got, ExactSum.of(case.lf.field[k], areas[k[1] - 1]), k)
        eng.set_areas(2, 2.0 * areas[1])  # replaced after the first upload
        same(eng.field_integrals([(1, 2, "UMOM")])[0], ExactSum.of(case.lf.field[(1, 2, "UMOM")], 2.0 * areas[1]), "replaced")
    finally:
        eng.close()


def test_received_field_is_read_from_its_exchange_grid_array():
    n = 8200
    n_src, src, dst, w = received.links("weighted", n)
    case = build_case("CCLM", n=n, T=1)
    source = received.source_values("TATM", n_src, np.float64)
    twin = received.expand(src, dst, w, source, n)
    rm = {"grid": 1, "n_src": n_src, "src": src, "dst": dst, "w": w,
          "fields": [(PHASE_NORMAL, 1, 1, "TATM", source)]}
    case.lf.field[(1, 1, "TATM")][:] = -1.0  # the engine no longer reads the exchange-grid array
    areas = np.random.default_rng(7).uniform(0.5, 2.0, n)
    eng = engine_of(case, received=[rm], options=MIRRORS)
    try:
        eng.set_areas(1, areas)
        eng.step(PHASE_ALL, STEP_T)
        got = eng.field_integrals([(1, 1, "TATM"), (0, 1, "TATM")])
        same(got[0], ExactSum.of(twin, areas), "TATM(1,t)")
        same(got[1], ExactSum.of(twin, areas), "TATM(0,t)")
    finally:
        eng.close()


def test_outputs_the_host_cannot_see():
    n = 4097
    areas = np.random.default_rng(8).uniform(0.5, 2.0, n)
    plain = build_case("MOM5", n=n, T=1, bias=True)
    eng = engine_of(plain, options=MIRRORS)
    eng.step(PHASE_ALL, STEP_T)
    eng.close()
    qsur = plain.lf.field[(1, 1, "QSUR")].copy()

    case = build_case("MOM5", n=n, T=1, bias=True)
    eng = engine_of(case, options=MIRRORS, output_use={(1, 1, "QSUR"): "device"})
    try:
        eng.set_areas(1, areas)
        eng.step(PHASE_ALL, STEP_T)
        same(eng.field_integrals([(1, 1, "QSUR")])[0], ExactSum.of(qsur, areas), "FCX_OUT_DEVICE QSUR")
    finally:
        eng.close()

    case = build_case("MOM5", n=n, T=1, bias=True)
    eng = engine_of(case, options=MIRRORS, output_use={(1, 1, "QSUR"): "unread"})
    try:
        eng.set_areas(1, areas)
        eng.step(PHASE_ALL, STEP_T)
        assert eng.output_info(1, 1, "QSUR") == 2  # the store was left out: the array is stale
        with pytest.raises(_lib.FcxError) as ex:
            eng.field_integrals([(1, 1, "TSUR"), (1, 1, "QSUR")])
        assert ex.value.status == 2 and "QSUR(1,t)" in str(ex.value) and "stale" in str(ex.value)
        with pytest.raises(_lib.FcxError) as ex:
            eng.field_integrals([(2, 1, "HLAT")])
        assert ex.value.status == 1 and "HLAT(2,t)" in str(ex.value) and "not bound" in str(ex.value)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_constants_equal_an_array_of_the_value(dtype):
    """fp64: a wave-uniform constant (no array, the launch carries the value); fp32: a constant
    the engine filled an array for.  Both are the twin's sum of n copies of the value the
    kernels see."""
    n = 4097
    case = typed(build_case("CCLM", n=n, T=1), dtype)
    value = 280.1  # (not a float)
    case.lf.set_constant("TATM", 1, 1, value)
    areas = np.random.default_rng(9).uniform(0.5, 2.0, n)
    eng = engine_of(case, options=MIRRORS)
    try:
        eng.set_areas(1, areas)
        eng.step(PHASE_ALL, STEP_T)
        kind = eng.constant_info(1, 1, "TATM")
        assert kind == (1 if dtype == "float64" else 2)
        held = np.full(n, value, dtype)
        for weighted in (True, False):
            got = eng.field_integrals([(1, 1, "TSUR"), (1, 1, "TATM")], weighted=weighted)[1]
            same(got, ExactSum.of(held, areas if weighted else None), (dtype, weighted))
        assert eng.constant_info(1, 1, "TATM") == kind  # it stays a value
    finally:
        eng.close()


def atmos_rig(n, dtype, options, amap, variant="CCLM"):
    case = typed(build_case(variant, n=n, T=1, bias=variant != "CCLM"), dtype)
    la = local_atmos(amap, 0, 1)
    outs = {name: np.full(la.n_atmos, np.nan, dtype) for name, _ in ATM}
    atm = {"local": la, "fields": [(PHASE_EARLY if name == "RBBR" else PHASE_NORMAL, 1, g, name, outs[name])
                                   for name, g in ATM]}
    return case, outs, engine_of(case, atmos=atm, options=options)


@pytest.mark.parametrize("dtype, records", [("float64", 0), ("float64", 1), ("float32", 0)])
def test_atmosphere_outputs(dtype, records):
    """Plain (tile-blocked) arrays, per-cell records forced at a small grid, an fp32 engine."""
    n = 8200 * 4  # > 4096 atmosphere cells: two tiles of the atmosphere pool
    amap = synthetic_atmos_map(n)
    case, outs, eng = atmos_rig(n, dtype, {**MIRRORS, "atm_records": records}, amap, variant="MOM5")
    try:
        assert eng.atm_records() == bool(records)
        a_atm = np.random.default_rng(10).uniform(0.5, 2.0, amap.n_atmos)
        with pytest.raises(_lib.FcxError) as ex:
            eng.atmos_integrals(PHASE_ALL)
        assert ex.value.status == 2 and "atmosphere" in str(ex.value)
        eng.set_atmos_areas(a_atm)
        eng.upload(PHASE_ALL)
        eng.run(PHASE_ALL, STEP_T)
        early, normal = eng.atmos_integrals(PHASE_EARLY), eng.atmos_integrals(PHASE_NORMAL)
        both, plain = eng.atmos_integrals(PHASE_ALL), eng.atmos_integrals(PHASE_ALL, weighted=False)
        assert (len(early), len(normal), len(both), len(plain)) == (1, 5, 6, 6)
        eng.download(PHASE_ALL)
        eng.synchronize()
        for (name, _), s, p in zip(ATM, both, plain):
            same(s, ExactSum.of(outs[name], a_atm), (dtype, records, name))
            same(p, ExactSum.of(outs[name]), (dtype, records, name, "unweighted"))
            assert s.n_terms == amap.n_atmos
        same(early[0], ExactSum.of(outs["RBBR"], a_atm), "early")
        for s, (name, _) in zip(normal, [a for a in ATM if a[0] != "RBBR"]):
            same(s, ExactSum.of(outs[name], a_atm), ("normal", name))
        assert both == eng.atmos_integrals(PHASE_ALL)  # ... and after the download too
    finally:
        eng.close()


def shard_of(whole, offset, size):
    """cells [offset, offset + size) of a CCLM T = 1 case as a case of its own"""
    part = build_case("CCLM", n=size, T=1)
    for k, a in part.lf.field.items():
        a[:] = whole.lf.field[k][offset:offset + size]
    return part


def test_decomposition_independence():
    """One engine over 24,012 cells against two and three engines over its APPLE shards, the
    shards' sums merged in every order and as a raw limb-wise sum normalised once: the same 576
    bytes for every flux of a CCLM step."""
    import itertools

    n = 24_012
    areas = np.random.default_rng(11).uniform(0.5, 2.0, n)

    def fluxes(case, a):
        eng = engine_of(case, options=MIRRORS)
        try:
            for g in (1, 2, 3):
                eng.set_areas(g, a)
            eng.step(PHASE_ALL, STEP_T)
            return eng.field_integrals(sorted(set(case.outputs)))
        finally:
            eng.close()

    whole = build_case("CCLM", n=n, T=1)
    slots = sorted(set(whole.outputs))
    single = fluxes(whole, areas)
    assert len(slots) >= 6 and all(s.n_terms == n for s in single)
    pristine = build_case("CCLM", n=n, T=1)
    for world in (2, 3):
        parts = []
        for r in range(world):
            off, size = apple_range(n, r, world)
            parts.append(fluxes(shard_of(pristine, off, size), areas[off:off + size]))
        for f, k in enumerate(slots):
            for order in itertools.permutations(range(world)):
                total = ExactSum()
                for r in order:
                    total = total + parts[r][f]
                same(total, single[f], (world, order, k))
            raw = sum(parts[r][f].words() for r in range(world))  # what MPI_SUM on INTEGER(8) gives
            same(ExactSum.from_raw(raw), single[f], (world, "raw", k))


def exact_int(s):
    """the exact value of a canonical sum in units of 2^-1088"""
    return sum(int(l) << (32 * k) for k, l in enumerate(s.limbs))


def test_conservation_within_the_derived_bound():
    """After a CCLM T = 1 step with the accumulation, sum_x A_x F_x on the exchange grid against
    sum_a A_a F_a on the atmosphere grid, with A_x = fl(w_x A_a(x)), both sums exact.

    Derivation (u = 2^-53, every |d| <= u).  Exchange side: A_x = w_x A_a (1 + d1) and the term is
    fl(A_x F_x) = w_x A_a F_x (1 + d1)(1 + d2).  Atmosphere side: the engine forms
    F_a = sum_{x in a} fl(w_x F_x) in double over the run of the cell, at most L cells; whatever
    the association, a product passes through at most L - 1 additions, so
    F_a = sum_x w_x F_x (1 + d3)(1 + t_x) with |t_x| <= (L - 1) u + O(u^2), and the term is
    fl(A_a F_a) = A_a F_a (1 + d4).  The integrals themselves add nothing.  So
      |sum_x t_x - sum_a t_a| <= sum_x |w_x A_a F_x| * ((L - 1) + 4) u + O(u^2)
                               = (L + 3) u S + O(u^2),   S = sum_x |A_x F_x| (1 + O(u)).
    The test uses (L + 4) u S with S = fsum |A_x F_x| of the downloaded fluxes: the extra u S is
    some 2^52 times the second-order terms and the rounding of S.  No term may overflow or be
    subnormal for the model to hold; the fields here are of order 1e-5 .. 1e3."""
    n = 8200
    amap = synthetic_atmos_map(n)
    rng = np.random.default_rng(12)
    a_atm = rng.uniform(0.5, 2.0, amap.n_atmos) * 1e9
    a_x = amap.weight * a_atm[amap.atmos_index]
    L = int(np.bincount(amap.atmos_index).max())
    assert 3 <= L <= 5
    case, outs, eng = atmos_rig(n, "float64", MIRRORS, amap)
    try:
        for g in (1, 2, 3):
            eng.set_areas(g, a_x)
        eng.set_atmos_areas(a_atm)
        eng.step(PHASE_ALL, STEP_T)
        exch = eng.field_integrals([(1, g, name) for name, g in ATM])
        atmo = eng.atmos_integrals(PHASE_ALL)
        for (name, g), sx, sa in zip(ATM, exch, atmo):
            f = case.lf.field[(1, g, name)]
            assert sx.n_terms == n and sa.n_terms == amap.n_atmos
            s_abs = math.fsum(np.abs(a_x * f))
            assert s_abs > 0.0
            diff = Fraction(abs(exact_int(sx) - exact_int(sa)), 1 << 1088)
            bound = Fraction(L + 4, 1 << 53) * Fraction(s_abs)
            print(f"{name}: |difference| / S = {float(diff / Fraction(s_abs)):.3e}, bound {float(bound / Fraction(s_abs)):.3e}")
            assert diff <= bound, (name, float(diff), float(bound))
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_integral_calls_change_no_field_and_repeat(dtype):
    n = 8200
    amap = synthetic_atmos_map(n)
    case, outs, eng = atmos_rig(n, dtype, MIRRORS, amap)
    try:
        rng = np.random.default_rng(13)
        for g in (1, 2, 3):
            eng.set_areas(g, rng.uniform(0.5, 2.0, n))
        eng.set_atmos_areas(rng.uniform(0.5, 2.0, amap.n_atmos))
        eng.step(PHASE_ALL, STEP_T)
        before = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}
        before.update({("atm", k): v.copy() for k, v in outs.items()})
        slots = sorted(set(case.outputs))
        for baseline in (0, 1, 0):  # the all-LDS baseline gives the same bits as the windows
            eng.set_option("sum_baseline", baseline)
            first = eng.field_integrals(slots), eng.atmos_integrals(PHASE_ALL)
            assert first == (eng.field_integrals(slots), eng.atmos_integrals(PHASE_ALL))
            if baseline == 0:
                ref = first
            assert first == ref
        eng.download(PHASE_ALL)
        eng.synchronize()
        for k, v in before.items():
            now = outs[k[1]] if k[0] == "atm" else case.lf.field[k]
            assert np.asarray(now).tobytes() == v.tobytes(), k
    finally:
        eng.close()


def test_the_drivers_budget_lines_are_the_twin_of_what_was_put():
    """fcx.driver.run(budgets=...) on the Baltic set-up (two surface types, averaged and
    default-valued sends, regridded fields): every line's integral is the twin's value on the array
    the coupler was handed, with the areas Setup.engine(areas=...) declared."""
    import namelists
    from namelists import regrid_matrices
    from fcx import driver
    from fcx.setup import setup_from_namelist
    from fcx.synthetic import SyntheticCoupler, corrections

    grids = (3001, 2999, 3011)
    rng = np.random.default_rng(15)
    areas = {g: rng.uniform(0.5, 2.0, grids[g - 1] + 9) for g in (1, 2, 3)}  # (longer than the grid)
    setup = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=grids)
    eng = setup.engine(corrections=(20000101, corrections(grids[0])), regrid=regrid_matrices(grids), areas=areas)
    coupler = SyntheticCoupler.for_setup(setup)
    lines = []
    try:
        driver.run(setup, eng, coupler, num_timesteps=1, budgets=lines.append)
    finally:
        eng.close()
    by_name = {f.name: f for f in setup.output_field}
    assert len(lines) == len(setup.output_field) and {ln.split()[1] for ln in lines} == set(by_name)
    for ln in lines:
        f = by_name[ln.split()[1]]
        n = grids[f.which_grid - 1]
        want = ExactSum.of(np.asarray(coupler.sent[(f.name, 0)])[:n], areas[f.which_grid][:n]).value
        assert float(ln.split("integral = ")[1].split()[0]) == want, ln
