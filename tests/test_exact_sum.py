"""The exact sum on the host, no GPU: fcx_exact_sum's layout, the host twin of the integral kernels
(fcx_sum_add_terms) against math.fsum -- which is exact and correctly rounded --, canonical
uniqueness under permutation and splitting, the rounding of fcx_sum_value at exact midpoints, the
argument checks of the entry points, and the driver's budget lines."""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import namelists
from fcx import _lib, driver
from fcx.basic import IDX
from fcx.engine import Engine, ExactSum
from fcx.parallel import local_atmos, owned_atmos_mask, synthetic_atmos_map
from fcx.setup import setup_from_namelist
from fcx.synthetic import SyntheticCoupler, build_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_O = os.path.join(ROOT, "components.flux_calculator_amd", "lib", "fortran", "flux_calculator_calculate.o")
E_ARG, E_STATE = 1, 2
GRIDS = (301, 299, 311)


def _err():
    return _lib.load().fcx_last_error().decode(errors="replace")


def _raw_engine(T=1, n=64):
    lib = _lib.load()
    h = ctypes.c_void_p()
    gs = (ctypes.c_int32 * 3)(n, n, n)
    _lib.check(lib.fcx_create(0, T, gs, ctypes.byref(h)))
    return lib, h


def same_float(a, b):
    return (a == b and math.copysign(1.0, a) == math.copysign(1.0, b)) or (math.isnan(a) and math.isnan(b))


def finite_value(s):
    """the limbs of s rounded: the sum of its finite terms, whatever was left out"""
    w = s.words()
    w[68:] = 0
    return ExactSum.from_raw(w).value


def fsum_of(x, a=None):
    """math.fsum of the finite IEEE terms (numpy's elementwise multiply is the IEEE product);
    beyond DBL_MAX fsum raises, where the exact sum rounds to an infinity"""
    with np.errstate(all="ignore"):
        t = np.asarray(x, dtype=np.float64) if a is None else np.asarray(a) * np.asarray(x, dtype=np.float64)
    t = t[np.isfinite(t)]
    try:
        return math.fsum(t)
    except OverflowError:
        return math.copysign(math.inf, math.fsum(t / 4.0))


def test_layout_and_constants():
    assert ctypes.sizeof(_lib.ExactSumC) == 576 and _lib.FCX_SUM_LIMBS == 68
    assert Engine.OPTIONS["sum_baseline"] == _lib.FCX_OPT_SUM_BASELINE == 25
    s = ExactSum.of(np.array([5e-324]))
    assert s.limbs[0] == 16384 and not any(s.limbs[1:]) and s.n_terms == 1  # the smallest denormal
    s = ExactSum.of(np.array([np.finfo(np.float64).max]))
    assert [k for k, l in enumerate(s.limbs) if l] == [64, 65]  # DBL_MAX touches limbs 64 and 65
    s = ExactSum.of(np.array([-5e-324]))  # two's complement over the 68 limbs
    assert s.limbs[0] == 2**32 - 16384 and all(l == 2**32 - 1 for l in s.limbs[1:67]) and s.limbs[67] == -1
    assert s.value == -5e-324
    assert ExactSum().value == 0.0 and math.copysign(1.0, ExactSum().value) == 1.0


def test_host_entry_points_validate_their_arguments():
    lib = _lib.load()
    s = _lib.ExactSumC()
    x = np.ones(4)
    v = ctypes.c_double()
    assert lib.fcx_sum_clear(None) == E_ARG
    assert lib.fcx_sum_add_terms(None, x.ctypes.data, None, 4) == E_ARG
    assert lib.fcx_sum_add_terms(s, None, None, 4) == E_ARG
    assert lib.fcx_sum_add_terms(s, x.ctypes.data, None, -1) == E_ARG
    assert lib.fcx_sum_add_terms_f32(s, None, None, 1) == E_ARG
    assert lib.fcx_sum_add_terms(s, None, None, 0) == 0
    assert lib.fcx_sum_merge(None, s) == E_ARG
    assert lib.fcx_sum_value(None, ctypes.byref(v)) == E_ARG and lib.fcx_sum_value(s, None) == E_ARG


def test_areas_and_device_calls_validate_their_arguments():
    lib, h = _raw_engine(n=64)
    try:
        a = np.ones(64)
        assert lib.fcx_set_areas(None, 1, a.ctypes.data, 64) == E_ARG
        for g in (0, 4):
            assert lib.fcx_set_areas(h, g, a.ctypes.data, 64) == E_ARG
        assert lib.fcx_set_areas(h, 1, a.ctypes.data, 63) == E_ARG and "64 cells" in _err()
        assert lib.fcx_set_areas(h, 1, None, 64) == E_ARG
        for bad in (np.nan, np.inf, -np.inf):
            a[17] = bad
            assert lib.fcx_set_areas(h, 2, a.ctypes.data, 64) == E_ARG
            assert "cell 17" in _err() and "grid u" in _err(), _err()
        a[17], a[3] = -1.0, 0.0  # negative and zero areas are allowed, before commit too
        assert lib.fcx_set_areas(h, 2, a.ctypes.data, 64) == 0
        assert lib.fcx_set_areas(h, 2, np.ones(80).ctypes.data, 80) == 0  # longer, and replaced
        assert lib.fcx_set_atmos_areas(h, a.ctypes.data, 64) == E_STATE and "fcx_set_atmos_map" in _err()
        idx, w = np.zeros(64, np.int32), np.full(64, 1.0 / 64)
        _lib.check(lib.fcx_set_atmos_map(h, 1, idx.ctypes.data, w.ctypes.data))
        assert lib.fcx_set_atmos_areas(h, a.ctypes.data, 2) == E_ARG
        assert lib.fcx_set_atmos_areas(h, np.array([np.nan]).ctypes.data, 1) == E_ARG and "cell 0" in _err()
        assert lib.fcx_set_atmos_areas(h, a.ctypes.data, 1) == 0

        out = (_lib.ExactSumC * 2)()
        ok = np.array((1, 1, IDX["TSUR"]), dtype=np.int32)
        assert lib.fcx_field_integrals(None, 1, ok.ctypes.data, 1, out) == E_ARG
        assert lib.fcx_field_integrals(h, 1, None, 1, out) == E_ARG
        assert lib.fcx_field_integrals(h, 1, ok.ctypes.data, 1, None) == E_ARG
        assert lib.fcx_field_integrals(h, -1, ok.ctypes.data, 1, out) == E_ARG
        assert lib.fcx_field_integrals(h, 1, ok.ctypes.data, 2, out) == E_ARG
        for bad in ((-1, 1, 11), (11, 1, 11), (1, 0, 11), (1, 4, 11), (1, 1, 0), (1, 1, 36)):
            s = np.array(((1, 1, 11), bad), dtype=np.int32).reshape(-1)
            assert lib.fcx_field_integrals(h, 2, s.ctypes.data, 0, out) == E_ARG, bad
            assert "slot 1" in _err() and "out of range" in _err(), _err()
        assert lib.fcx_field_integrals(h, 1, ok.ctypes.data, 1, out) == E_STATE  # not committed
        assert "fcx_commit" in _err()
        n = ctypes.c_int32()
        assert lib.fcx_atmos_integrals(None, 3, 1, 2, out, ctypes.byref(n)) == E_ARG
        assert lib.fcx_atmos_integrals(h, 3, 1, 2, out, None) == E_ARG
        assert lib.fcx_atmos_integrals(h, 3, 1, 2, None, ctypes.byref(n)) == E_ARG
        assert lib.fcx_atmos_integrals(h, 3, 1, -1, out, ctypes.byref(n)) == E_ARG
        assert lib.fcx_atmos_integrals(h, 3, 2, 2, out, ctypes.byref(n)) == E_ARG
        for phase in (0, 4):
            assert lib.fcx_atmos_integrals(h, phase, 1, 2, out, ctypes.byref(n)) == E_ARG
        assert lib.fcx_atmos_integrals(h, 3, 1, 2, out, ctypes.byref(n)) == E_STATE
        assert "fcx_commit" in _err()
        assert lib.fcx_set_option(h, 25, 1) == 0 and lib.fcx_set_option(h, 25, 2) == E_ARG
    finally:
        lib.fcx_destroy(h)


def _patterns(rng):
    n = 20_000
    yield "uniform", rng.uniform(-1.0, 1.0, n)
    yield "exponents", np.ldexp(rng.uniform(-1.0, 1.0, n), rng.integers(-1074, 1024, n))
    yield "denormals", rng.integers(-2**52, 2**52, n) * 5e-324
    yield "1e308 + 1 - 1e308", np.array([1e308, 1.0, -1e308])
    yield "1e16 + 1 - 1e16", np.array([1e16, 1.0, -1e16])
    z = np.zeros(64)
    z[::3] = -0.0
    yield "zeros", z
    yield "negative zeros", np.full(5, -0.0)
    yield "empty", np.zeros(0)
    yield "beyond DBL_MAX", np.array([1e308] * 4 + [3.0])
    yield "beyond -DBL_MAX", np.array([-1.7e308] * 3)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_twin_against_fsum(dtype, weighted):
    rng = np.random.default_rng(20)
    for label, x in _patterns(rng):
        with np.errstate(over="ignore", under="ignore"):
            x = x.astype(dtype)
        a = rng.uniform(0.25, 4.0, x.shape[0]) * rng.choice([1.0, 1.0, -1.0, 0.0], x.shape[0]) if weighted else None
        s = ExactSum.of(x, a)
        want = fsum_of(x, a)
        assert same_float(finite_value(s), want), (label, s, want)
        if s.n_nan + s.n_pinf + s.n_ninf == 0:
            assert same_float(s.value, want)
        assert s.n_terms + s.n_nan + s.n_pinf + s.n_ninf == x.shape[0]
        if label in ("zeros", "negative zeros", "empty"):
            assert same_float(s.value, 0.0) and not any(s.limbs)


def test_exact_cancellation_and_overflow_that_comes_back():
    assert ExactSum.of(np.array([1e308, 1.0, -1e308])).value == 1.0
    assert ExactSum.of(np.array([1e16, 1.0, -1e16])).value == 1.0
    up = ExactSum.of(np.array([1.5e308, 1.5e308, 2.0 ** -1074]))
    assert up.value == math.inf and (up.n_pinf, up.n_ninf, up.n_nan) == (0, 0, 0)  # the limbs stay exact
    down = ExactSum.of(np.array([-1.5e308, -1.0e308]))
    back = up + down
    assert back.value == 0.5e308 and back.n_terms == 5
    assert (back + ExactSum.of(np.array([-0.5e308]))).value == 2.0 ** -1074
    assert (-up).value == -math.inf and (up + (-up)).value == 0.0 and not any((up + (-up)).limbs)


def test_non_finite_terms_are_counted_and_stay_out():
    x = np.array([1.0, np.nan, np.inf, 2.0, -np.inf, np.inf, -0.0])
    s = ExactSum.of(x)
    assert (s.n_terms, s.n_nan, s.n_pinf, s.n_ninf) == (3, 1, 2, 1)
    assert bytes(s)[:544] == bytes(ExactSum.of(np.array([1.0, 2.0])))[:544]  # the limbs: 3.0 alone
    assert math.isnan(s.value)
    assert ExactSum.of(np.array([1.0, np.inf])).value == math.inf
    assert ExactSum.of(np.array([1.0, -np.inf, -np.inf])).value == -math.inf
    assert math.isnan(ExactSum.of(np.array([np.inf, -np.inf])).value)
    # a product that overflows, and 0 * Inf, are non-finite terms too
    s = ExactSum.of(np.array([1e308, 5.0, np.inf]), np.array([10.0, 1.0, 0.0]))
    assert (s.n_terms, s.n_nan, s.n_pinf, s.n_ninf) == (1, 1, 1, 0)
    s32 = ExactSum.of(np.array([1.0, np.inf, np.nan], np.float32))
    assert (s32.n_terms, s32.n_nan, s32.n_pinf) == (1, 1, 1)


def test_fp32_terms_are_widened_exactly_and_multiplied_in_double():
    rng = np.random.default_rng(21)
    x = rng.uniform(-3.0, 3.0, 5000).astype(np.float32)
    a = rng.uniform(0.5, 2.0, 5000)
    assert ExactSum.of(x, a) == ExactSum.of(x.astype(np.float64), a)
    assert ExactSum.of(x) == ExactSum.of(x.astype(np.float64))


@pytest.mark.parametrize("pattern", ["uniform", "exponents", "cancelling"])
def test_canonical_form_is_unique(pattern):
    """Any permutation of the terms, any split into 2, 3 or 7 pieces merged in any order, and a
    raw limb-wise sum of the pieces normalised once: the same 576 bytes."""
    rng = np.random.default_rng(22)
    n = 4000
    v = np.ldexp(rng.uniform(-1.0, 1.0, n // 2), rng.integers(-300, 300, n // 2))
    x = {"uniform": rng.uniform(-1.0, 1.0, n),
         "exponents": np.ldexp(rng.uniform(-1.0, 1.0, n), rng.integers(-1074, 1024, n)),
         "cancelling": np.concatenate([v, -v[::-1] * (1.0 + 2.0 ** -40)])}[pattern]
    x[[5, 77]] = np.nan, -np.inf
    a = rng.uniform(0.5, 2.0, n)
    whole = ExactSum.of(x, a)
    for _ in range(3):
        p = rng.permutation(n)
        assert ExactSum.of(x[p], a[p]) == whole
    for pieces in (2, 3, 7):
        cuts = np.sort(rng.integers(0, n + 1, pieces - 1))
        parts = [ExactSum.of(xs, as_) for xs, as_ in zip(np.split(x, cuts), np.split(a, cuts))]
        orders = itertools.permutations(range(pieces)) if pieces < 7 else [rng.permutation(7) for _ in range(6)]
        for order in orders:
            total = ExactSum()
            for k in order:
                total = total + parts[k]
            assert bytes(total) == bytes(whole), (pieces, order)
        tree = (parts[0] + parts[1]) + sum(parts[2:], ExactSum()) if pieces > 2 else parts[0] + parts[1]
        assert tree == whole
        raw = sum(q.words() for q in parts)  # MPI_SUM on INTEGER(8)
        assert ExactSum.from_raw(raw) == whole
    # adding in place, chunk after chunk, is the same sum again
    s = ExactSum()
    for xs, as_ in zip(np.split(x, 5), np.split(a, 5)):
        s.add_terms(xs, as_)
    assert s == whole


def test_a_raw_sum_of_many_ranks_normalises():
    """2^30 ranks holding the same canonical sum: the raw limbs (below 2^62) normalise to 2^30 x."""
    part = ExactSum.of(np.array([-1.0 - 2.0 ** -52, 2.0 ** -1074, 3e290]))
    raw = part.words() * (1 << 30)
    assert np.abs(raw[:68].astype(object)).max() < 2 ** 62
    total = ExactSum.from_raw(raw)
    assert total.n_terms == 3 << 30
    scaled = ExactSum.of(np.array([(-1.0 - 2.0 ** -52) * 2.0 ** 30, 2.0 ** -1044, 3e290 * 2.0 ** 30]))
    assert bytes(total)[:544] == bytes(scaled)[:544] and total.value == scaled.value


def test_value_rounds_to_nearest_even_at_exact_midpoints():
    u = 2.0 ** -53  # half an ulp of 1.0
    tiny = 2.0 ** -1000
    cases = [
        ([1.0, u], 1.0),                              # a tie: to even, down
        ([1.0, u, tiny], 1.0 + 2 * u),                # one digit above the midpoint
        ([1.0, u, -tiny], 1.0),                       # one digit below
        ([1.0 + 2 * u, u], 1.0 + 4 * u),              # a tie: to even, up
        ([1.0 + 2 * u, u, -tiny], 1.0 + 2 * u),
        ([1.0 + 2 * u, u, tiny], 1.0 + 4 * u),
        ([-1.0, -u], -1.0), ([-1.0, -u, -tiny], -1.0 - 2 * u), ([-1.0 - 2 * u, -u], -1.0 - 4 * u),
        ([2.0 - 2 * u, u], 2.0),                      # a tie that carries into the next binade
        ([2.0 ** -1074, 2.0 ** -1074], 2.0 ** -1073),  # denormals add exactly
        ([2.0 ** -1022, -(2.0 ** -1074)], 2.0 ** -1022 - 2.0 ** -1074),
        ([np.finfo(np.float64).max, 2.0 ** 969], np.finfo(np.float64).max),  # below the midpoint to Inf
        ([np.finfo(np.float64).max, 2.0 ** 970], math.inf),                  # the midpoint: to even = Inf
        ([np.finfo(np.float64).max, 2.0 ** 970, -tiny], np.finfo(np.float64).max),
    ]
    for terms, want in cases:
        got = ExactSum.of(np.array(terms)).value
        assert same_float(got, want), (terms, got, want)
        if max(abs(t) for t in terms) < 1e300:  # (fsum refuses an intermediate overflow)
            assert same_float(got, math.fsum(terms)), terms


def test_owned_atmos_mask_counts_a_shared_cell_once():
    amap = synthetic_atmos_map(1000)
    for world in (1, 2, 3, 7):
        owned = np.zeros(amap.n_atmos)
        shared = 0
        for r in range(world):
            la = local_atmos(amap, r, world)
            m = owned_atmos_mask(la)
            assert m.shape == (la.n_atmos,) and set(m) <= {0.0, 1.0}
            owned[la.atmos_offset: la.atmos_offset + la.n_atmos] += m
            shared += la.left >= 0
        assert (owned == 1.0).all() and (world == 1 or shared > 0)


class _StubEngine:
    """Counts what the driver asks of an engine."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append(name)
            return []
        return call


def test_the_driver_makes_no_integral_call_without_budgets():
    setup = setup_from_namelist(namelists.CCLM_REGRID, mype=1, grid_size=GRIDS)
    stub = _StubEngine()
    driver.run(setup, stub, SyntheticCoupler.for_setup(setup), num_timesteps=1)
    assert "step" in stub.calls and not {"field_integrals", "atmos_integrals"} & set(stub.calls)
    lines, asked = [], []
    stub = _StubEngine()

    def field_integrals(slots):
        asked.append(list(slots))
        return [ExactSum.of(np.array([float(k)])) for k in range(len(slots))]

    stub.field_integrals = field_integrals
    driver.run(setup, stub, SyntheticCoupler.for_setup(setup), num_timesteps=2, budgets=lines.append)
    assert len(lines) == 2 * len(setup.output_field) and "atmos_integrals" not in stub.calls
    assert sum(len(a) for a in asked) == 2 * len(setup.output_field)
    names = {f.name for f in setup.output_field}
    assert all(ln.split()[0] == "budget" and ln.split()[1] in names and "integral = " in ln for ln in lines)
    assert "field_ranges" not in stub.calls  # (and no log: no range call either)


def test_the_drivers_budget_line_names_the_atmosphere_twin():
    setup = setup_from_namelist(namelists.CCLM_REGRID, mype=1, grid_size=GRIDS)
    sent = [f for f in setup.output_field if not f.early]
    assert sent
    twin = sent[0]
    stub = _StubEngine()
    stub.atmos_twins = lambda phase: [tuple(twin.slot)] if phase == 2 else []
    stub.field_integrals = lambda slots: [ExactSum.of(np.array([1.0, 2.0 ** -60])) for _ in slots]
    stub.atmos_integrals = lambda phase: [ExactSum.of(np.array([1.0]))]
    lines = []
    driver.run(setup, stub, SyntheticCoupler.for_setup(setup), num_timesteps=1, budgets=lines.append)
    hit = [ln for ln in lines if "atmosphere = " in ln]
    assert len(hit) == 1 and hit[0].split()[1] == twin.name
    assert hit[0].endswith(f"difference = {2.0 ** -60!r}")  # of the exact sums, not of the rounded values


@pytest.mark.skipif(not os.path.exists(SHIM_O), reason="Fortran shim not built (needs flang + reference module)")
def test_dropin_module_exports_the_budget_routines():
    out = subprocess.run(["nm", SHIM_O], capture_output=True, text=True, check=True).stdout.lower()
    for name in ("fcx_declare_areas", "fcx_field_integral_of"):
        assert f"_qmflux_calculator_calculatep{name}" in out, name
    for c in ("fcx_set_areas", "fcx_field_integrals", "fcx_sum_value"):
        assert f" u {c}" in out, c


def test_setup_engine_cuts_a_grid_files_global_areas_to_the_ranks_window():
    """Setup.engine(areas={grid: what fcx.io.read_scrip_grid returns}): cells grid_offset ..
    grid_offset + grid_size of the global "area" are declared.  Every cell outside that window is
    NaN here, so a slice that is off by one is refused by fcx_set_areas, which names the cell."""
    setup = setup_from_namelist(namelists.CCLM_REGRID, mype=1, grid_size=GRIDS)

    def grid(g, offset, shift=0):
        n = GRIDS[g - 1]
        area = np.full(offset + n + 7, np.nan)
        area[offset:offset + n] = 1.0 + np.arange(n)
        return {"grid_size_global": area.shape[0], "area": area, "grid_size": n, "grid_offset": offset + shift}

    eng = setup.engine(commit=False, areas={1: grid(1, 40), 2: grid(2, 0), 3: np.ones(GRIDS[2])})
    eng.close()
    for shift, cell in ((1, GRIDS[0] - 1), (-1, 0)):
        with pytest.raises(_lib.FcxError) as ex:
            setup.engine(commit=False, areas={1: grid(1, 40, shift)})
        assert ex.value.status == E_ARG and f"cell {cell} of exchange grid t" in str(ex.value)


def test_the_variant_build_links_the_makefiles_translation_units():
    """tools/build_variant.sh builds the A/B libraries from its own list of translation units: one
    the Makefile links and the script leaves out gives a library whose load fails on an undefined
    symbol (ctypes binds at load time)."""
    import re

    pkg = os.path.join(ROOT, "components.flux_calculator_amd")
    make = open(os.path.join(pkg, "Makefile")).read().replace("\\\n", " ")
    objs = re.search(r"^OBJS\s*:=(.*)$", make, re.M).group(1)
    script = open(os.path.join(pkg, "tools", "build_variant.sh")).read()
    units = re.search(r'^UNITS="([^"]*)"', script, re.M).group(1).split()
    assert sorted(units) == sorted(re.findall(r"obj/(\w+)\.o", objs)) and "fcx_integrals" in units
