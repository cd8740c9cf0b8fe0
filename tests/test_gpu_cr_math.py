"""An fp64 engine with FCX_OPT_CR_MATH on the device: every launch family of fcx_kernels_cr.hip
held to the correctly rounded values of tests/golden/cr_math.npz.

The inputs of a case are rows of the fixture's cell table (cr_expect.Fixture.fill), so the
correctly rounded value of every transcendental site of every cell is known without a wide
reference at test time.

PRIMARY GATE, every cell: QSUR (CCLM), RCO's MEVA (+ bias) and the HLAT over it, and the CCLM and
MOM5 HSEN are bit-identical to cr_expect.expected fed the fixture's results.  Beside it
parity.assert_tight against the live C oracle passes for the whole case: a correctly rounded
value is inside its derived bound, and the seeded, exact and construction gates, which do not
depend on the sites, pin every other field and the type-0 averages.

Shapes: those of tests/test_gpu_ulp_gate.py."""
import os

import numpy as np
import pytest

import cr_expect
import oracle_lib
from parity import assert_tight, bits_equal

pytestmark = pytest.mark.gpu

from fcx.basic import IDX, PHASE_ALL, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.synthetic import build_case  # noqa: E402
from fcx.workload import ATM_FIELDS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_T = 3600 * 24 * 31  # inside February of 1961: month 2 bias slice
VARIANTS = ("CCLM", "MOM5", "RCO")
CR = {"cr_math": 1}
FX = cr_expect.Fixture(os.path.join(ROOT, "tests", "golden", "cr_math.npz"))


def fixture_case(variant, **kw):
    return FX.fill(build_case(variant, bias=True, **kw))


def engine_of(case, options=None, **kw):
    return Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                  averages=case.averages, regrid=case.regrid, options=options or None, **kw)


def stepped(case, options):
    eng = engine_of(case, options)
    try:
        if options and "cr_math" in options:
            assert eng.cr_math() == bool(options["cr_math"])
        eng.step(PHASE_ALL, STEP_T)
        return {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}
    finally:
        eng.close()


def hold(case, got, label):
    """the primary gate, then assert_tight against the live oracle"""
    want = cr_expect.expected(case, STEP_T, FX.exp, FX.pow)
    assert want, label
    for k, v in want.items():
        ok = bits_equal(got[k], v)
        assert ok.all(), (f"{label}: {k} is not the correctly rounded value in {int((~ok).sum())} of {ok.size} "
                          f"cells, first {np.nonzero(~ok)[0][:5].tolist()}")
    ref = oracle_lib.run_case(case, "c", current_step_time=STEP_T)
    assert_tight(case, got, ref, STEP_T, "cr_" + label, report=False)
    return ref


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", ["default", "generic", "one_cell"])
@pytest.mark.parametrize("n", [1, 2, 3, 129, 300, 4097])
def test_single_type(variant, mode, n):
    """T = 1: the specialised kernels, specialize=0 (VAR = 0) and cells_per_thread=1"""
    options = {"default": {}, "generic": {"specialize": 0}, "one_cell": {"cells_per_thread": 1}}[mode]
    case = fixture_case(variant, n=n, T=1)
    hold(case, stepped(case, {**options, **CR}), f"{variant}_T1_n{n}_{mode}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("T", [2, 3])
def test_multi_type(variant, T):
    """T = 2, 3 at n = 300: the register averages, ta_exner formed once per cell"""
    case = fixture_case(variant, n=300, T=T)
    hold(case, stepped(case, CR), f"{variant}_T{T}_n300")


@pytest.mark.parametrize("variant", VARIANTS)
def test_separate_uv_grids(variant):
    """(n, nu, nv) = (300, 310, 290), T = 2: uv_grid's QSUR on grids of their own"""
    case = fixture_case(variant, n=300, T=2, sep_grids=(310, 290))
    got = stepped(case, CR)
    hold(case, got, f"{variant}_T2_sep")
    if variant != "RCO":
        assert {(s, g, "QSUR") for s in (1, 2) for g in (1, 2, 3)} <= set(got)


def group_of(T, lengths, options, host_atm=False):
    """the three variants with the fused accumulation on one stream, uploaded (host_atm: the
    atmosphere outputs are host arrays, which the per-cell record layout needs)"""
    import torch

    from fcx.parallel import local_atmos
    from test_gpu_multirank import random_run_map

    n = 300
    la = local_atmos(random_run_map(n, lengths, seed=41), 0, 1)
    cases, engines, keep = [], [], []
    stream = torch.cuda.current_stream().cuda_stream
    for v, opt in zip(VARIANTS, options):
        c = fixture_case(v, n=n, T=T)
        if host_atm:
            o = {name: np.full(la.n_atmos, np.nan) for name, _ in ATM_FIELDS}
        else:
            o = {name: torch.full((la.n_atmos,), float("nan"), dtype=torch.float64, device="cuda:0") for name, _ in ATM_FIELDS}
        atmos = {"local": la, "fields": [(PHASE_NORMAL, 0 if T >= 2 else 1, g, name, o[name]) for name, g in ATM_FIELDS]}
        engines.append(engine_of(c, {"atmos_in_run": 0, "timing": 0, "host_staging": 0, **opt}, atmos=atmos, stream=stream))
        cases.append(c)
        keep.append(o)
    for e in engines:
        e.upload(PHASE_ALL)
    return cases, engines, keep


def run_and_download(engines):
    run_group(engines, PHASE_ALL, STEP_T)
    for e in engines:
        e.run_atmos(PHASE_ALL)
        e.download(PHASE_ALL)
        e.synchronize()


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("lengths", [(3, 5), (1, 10)])
def test_group_launch(lengths, T):
    """The three variants in ONE fcx_run_group launch with the fused accumulation, n = 300: runs of
    3-5 cells (halo tiles) and of 1-10 cells (crossing records and the fix-up).  It merges."""
    cases, engines, keep = group_of(T, lengths, [CR] * 3)
    try:
        run_and_download(engines)
        assert all(e.cr_math() and e.fused_accumulation(PHASE_ALL) for e in engines)
        assert [e.last_group_size() for e in engines] == [3, 3, 3]
        for v, c in zip(VARIANTS, cases):
            got = {k: np.array(c.lf.field[k], copy=True) for k in c.outputs}
            hold(c, got, f"group_{v}_T{T}_runs{lengths[0]}-{lengths[1]}")
        for o in keep:
            assert all(bool(np.isfinite(x.cpu().numpy()).all()) for x in o.values())
    finally:
        for e in engines:
            e.close()


def test_group_launch_dense_records():
    """the group launch whose members keep per-cell records of their atmosphere outputs
    (FCX_OPT_ATM_RECORDS on halo tiles: cells_atmos_group_kernel's dense-record form)"""
    cases, engines, keep = group_of(1, (3, 5), [{**CR, "atm_records": 1}] * 3, host_atm=True)
    try:
        run_and_download(engines)
        assert all(np.isfinite(a).all() for o in keep for a in o.values())
        assert all(e.cr_math() and e.atm_records() and e.fused_accumulation(PHASE_ALL) for e in engines)
        assert [e.last_group_size() for e in engines] == [3, 3, 3]
        for v, c in zip(VARIANTS, cases):
            got = {k: np.array(c.lf.field[k], copy=True) for k in c.outputs}
            hold(c, got, f"group_records_{v}")
    finally:
        for e in engines:
            e.close()


def test_group_keeps_the_policies_apart():
    """an engine with the option off does not merge with two that have it on"""
    cases, engines, _ = group_of(1, (3, 5), [CR, {}, CR])
    try:
        run_and_download(engines)
        assert [e.cr_math() for e in engines] == [True, False, True]
        assert [e.last_group_size() for e in engines] == [2, 0, 2]
        for v, c, on in zip(VARIANTS, cases, (True, False, True)):
            got = {k: np.array(c.lf.field[k], copy=True) for k in c.outputs}
            if on:
                hold(c, got, f"mixed_group_{v}")
            else:
                same = stepped(fixture_case(v, n=300, T=1), None)
                assert all(bits_equal(got[k], same[k]).all() for k in got)
    finally:
        for e in engines:
            e.close()


def test_per_call_subroutines():
    """the fcx_calc_* sequence of a CCLM and an RCO T = 2 case, once"""
    for variant in ("CCLM", "RCO"):
        case = fixture_case(variant, n=300, T=2)
        for k in case.outputs:  # (every output array defined before the first call reads it)
            case.lf.field[k][:] = 0.0
        eng = engine_of(case, CR)
        calls = [("fcx_calc_flux_radiation_blackbody", ())] + [("fcx_calc_spec_vapor_surface", (g,)) for g in (1, 2, 3)] + \
                [("fcx_calc_flux_mass_evap", (STEP_T,)), ("fcx_calc_flux_heat_latent", ()),
                 ("fcx_calc_flux_heat_sensible", ()), ("fcx_calc_flux_momentum_east", (2,)),
                 ("fcx_calc_flux_momentum_north", (3,))] + \
                [("fcx_average_across_surface_types", (g, IDX[name])) for _, g, name in case.averages]
        try:
            for name, args in calls:
                assert getattr(eng.lib, name)(eng.h, *args) == 0, (name, eng.lib.fcx_last_error())
            got = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}
        finally:
            eng.close()
        hold(case, got, f"per_call_{variant}")


def test_against_the_live_oracle():
    """Every cell where the device's QSUR (RCO MEVA, HSEN) differs from the live oracle's is a cell
    where this host's math.exp (math.pow) of the fixture's argument differs from the fixture's
    result: each difference belongs to the host's libm, cell by cell, hard cases included.  The
    share of such cells among the cells that are ordinary draws for the site is at most 0.5 % (a
    site's hard cases are chosen within 1e-4 ulp of a rounding midpoint, where a libm that is good
    to an ulp misrounds almost every other one: over all rows the libm alone is past the cap, which
    tests/test_cr_math.py measures on the CPU)."""
    n = FX.n
    rows = FX.rows(n)
    kind = FX["kind"][rows]
    libm_exp_differs = {"qsur": ~bits_equal(cr_expect.libm_exp(FX["qsur_arg"]), FX["qsur_res"])[rows],
                        "rco": ~bits_equal(cr_expect.libm_exp(FX["rco_arg"]), FX["rco_res"])[rows]}
    libm_pow_differs = ~bits_equal(cr_expect.libm_pow(FX["exner_x"], FX.y), FX["exner_res"])[rows]
    for variant, key, by, bit in (("CCLM", (1, 1, "QSUR"), libm_exp_differs["qsur"], 1),
                                  ("CCLM", (1, 1, "HSEN"), libm_pow_differs, 4), ("MOM5", (1, 1, "HSEN"), libm_pow_differs, 4),
                                  ("RCO", (1, 1, "MEVA"), libm_exp_differs["rco"], 2)):
        ordinary = (kind & bit) == 0
        case = fixture_case(variant, n=n, T=1)
        got = stepped(case, CR)
        ref = hold(case, got, f"live_{variant}")
        differs = ~bits_equal(got[key], ref[key])
        assert not (differs & ~by).any(), (variant, key, np.nonzero(differs & ~by)[0][:5].tolist())
        share = differs[ordinary].mean()
        print(f"{variant} {key[2]}: differs from the live oracle in {int(differs.sum())} of {n} cells, "
              f"{int(differs[ordinary].sum())} of {int(ordinary.sum())} ordinary draws")
        assert share <= 0.005, (variant, key, share)


@pytest.mark.parametrize("variant,T", [("CCLM", 1), ("RCO", 1), ("MOM5", 2)])
def test_default_untouched(variant, T):
    """with the option off the outputs are the bits of an engine that was never given it"""
    never = stepped(fixture_case(variant, n=1025, T=T), None)
    off = stepped(fixture_case(variant, n=1025, T=T), {"cr_math": 0})
    assert never.keys() == off.keys()
    for k in never:
        assert bits_equal(never[k], off[k]).all(), k
