"""FCX_OPT_F32_MATH on the GPU: an fp32 engine whose fluxes are computed in double.

The witness is the project's own fp64 engine.  For c32 = as_dtype(case, "float32") the TWIN is
an fp64 engine on as_dtype(c32, "float64"), its corrections and constants rounded to float32 and
widened first (what the fp32 engine does at commit).  The wide kernels run the same double
operations in the same order on the same values, so there is no tolerance:

    every flux output of a whole-phase launch == np.float32(twin output), bit for bit
    (uint32 views; NaN matches NaN).

assert_tight holds the twin to the oracle in the same test, which closes the chain to the
reference.  Float arithmetic fails the rule in most cells; a ragged-tail, conversion, pair-order
or halo mistake fails it in the cells it touches."""
import json
import os

import numpy as np
import pytest

import oracle_lib
from parity import assert_tight, error_report

pytestmark = pytest.mark.gpu

from fcx import _lib  # noqa: E402
from fcx.basic import IDX, PHASE_ALL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.parallel import local_atmos  # noqa: E402
from fcx.synthetic import as_dtype, build_case  # noqa: E402
from test_gpu_fp32 import OUT  # noqa: E402  (the reports go beside the fp32 engine's)

STEP_T = 3600 * 24 * 31
ATM_FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
WIDE = {"f32_math": 1}
E_STATE = 2


def twin_of(c32):
    """the fp64 case whose values are the fp32 engine's: every array widened exactly, the
    corrections and the recorded constants rounded to float32 and widened"""
    twin = as_dtype(c32, "float64")
    if twin.corrections is not None:
        init_date, corr = twin.corrections
        twin.corrections = (init_date, np.asarray(corr, dtype=np.float32).astype(np.float64))
    twin.lf.constant = {k: float(np.float32(v)) for k, v in twin.lf.constant.items()}
    return twin


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same32(got, want64):
    """per cell: got (float32) has the bits of np.float32(want64); NaN matches NaN"""
    got = np.ascontiguousarray(got)
    assert got.dtype == np.float32, got.dtype
    with np.errstate(over="ignore"):
        want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return (np.isnan(got) & np.isnan(want)) | (~np.isnan(got) & ~np.isnan(want) & (bits32(got) == bits32(want)))


def engine_of(case, options=None, **kw):
    return Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                  averages=case.averages, regrid=case.regrid, options=options or None, **kw)


def construction(case32, key):
    """assert_tight's "construction" sum of a type-0 average, acc += x_s * FARE_s in float64 in
    type order, over the engine's own stored floats, rounded once"""
    _, g, name = key
    acc = np.zeros(case32.lf.grid_size[g - 1])
    for s in range(1, case32.num_surface_types + 1):
        acc = acc + np.asarray(case32.lf.field[(s, g, name)], np.float64) * np.asarray(case32.lf.field[(s, g, "FARE")],
                                                                                      np.float64)
    return acc


def run_wide_and_twin(case, options=None, label="", t=STEP_T, atmos=None):
    """The wide engine and its twin over one whole-phase step; the twin rule on every output, the
    twin itself through assert_tight.  Returns (c32, wide outputs, twin outputs, oracle, which rule
    each type-0 average met)."""
    c32 = as_dtype(case, "float32")
    twin = twin_of(c32)
    opts = dict(options or {})
    ew = engine_of(c32, {**opts, **WIDE}, **(atmos(c32) if atmos else {}))
    try:
        assert ew.f32_math()
        ew.step(PHASE_ALL, t)
    finally:
        ew.close()
    et = engine_of(twin, opts)
    try:
        assert not et.f32_math()
        et.step(PHASE_ALL, t)
    finally:
        et.close()
    got = {k: np.array(c32.lf.field[k], copy=True) for k in c32.outputs}
    got64 = {k: np.array(twin.lf.field[k], copy=True) for k in twin.outputs}
    ref = oracle_lib.run_case(twin, "c", current_step_time=t)
    assert_tight(twin, got64, ref, t, f"f32math twin {label}", report=False)
    averages = {}
    for k in c32.outputs:
        ok = same32(got[k], got64[k])
        if k[0] == 0 and not ok.all():  # a plan that re-reads the stored fields: all cells alike
            ok = same32(got[k], construction(c32, k))
            averages[k] = "construction over the stored floats"
        elif k[0] == 0:
            averages[k] = "np.float32(twin): formed in the launch from unrounded values"
        bad = np.nonzero(~ok)[0]
        assert bad.size == 0, (f"{label}: {k} is not np.float32(twin) in {bad.size} of {ok.size} cells, first "
                               f"{bad[:6].tolist()}: got {got[k][bad[:3]].tolist()} twin {got64[k][bad[:3]].tolist()}")
    return c32, got, got64, ref, averages


def column(got, ref):
    return {"%d:%d:%s" % key: {"norm": n, "mixed": m, "max_rel": r} for key, (n, m, r) in error_report(got, ref).items()}


# ---------------------------------------------------------------- T = 1 with bias
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
@pytest.mark.parametrize("n", [1, 3, 4099, 32_768])
def test_t1_bias(variant, n):
    """The T = 1 specialised wide kernels: the partial-vector path and the ragged last lane of
    four.  At 32,768 cells the three-column report of test_gpu_fp32.py is written beside the fp32
    engine's (f32math_error_<variant>.json), and the kernel's own column -- against the fp64
    oracle on the rounded inputs -- is asserted cell by cell, with no allowance: at most half an
    fp32 ulp (2**-24 |twin|, or half the smallest subnormal) plus the twin's own deviation."""
    case = build_case(variant, n=n, T=1, bias=True)
    c32, got, got64, ref, _ = run_wide_and_twin(case, label=f"{variant} n={n}")
    if n != 32_768:
        return
    ref_orig = oracle_lib.run_case(case, "c", current_step_time=STEP_T)
    wide64 = {k: np.asarray(v, dtype=np.float64) for k, v in got.items()}
    report = {"f32math_kernel_vs_fp64_original_inputs": column(wide64, ref_orig),
              "f32math_kernel_vs_fp64_rounded_inputs": column(wide64, ref),
              "input_rounding_only": column(ref, ref_orig),
              "twin_fp64_engine_vs_fp64_rounded_inputs": column(got64, ref),
              "rule": "|x - ref| <= 2**-24 |twin| + 2**-150 + |twin - ref| per cell, ref = fp64 oracle on the "
                      "fp32-rounded inputs, twin = the fp64 engine on them"}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"f32math_error_{variant}.json"), "w") as f:
        json.dump(report, f, indent=1)
    for k, r in ref.items():
        r = np.asarray(r, dtype=np.float64)
        allow = 2.0 ** -24 * np.abs(got64[k]) + 2.0 ** -150 + np.abs(got64[k] - r)
        over = np.abs(wide64[k] - r) > allow
        assert not over.any(), f"{variant}: {k} over half an fp32 ulp of the twin in {int(over.sum())} cells"


def test_one_cell_per_lane():
    run_wide_and_twin(build_case("CCLM", n=1001, T=1, bias=True), {"cells_per_thread": 1}, "CCLM cells_per_thread=1")


@pytest.mark.parametrize("variant", ["CCLM", "RCO"])
def test_t3_averages(variant):
    """Three surface types and the type-0 averages: each average is, for all its cells alike,
    np.float32(twin) (formed in the launch from the unrounded fluxes) or the construction sum
    over the engine's stored floats (a plan that re-reads them).  Which one is reported."""
    _, got, _, _, averages = run_wide_and_twin(build_case(variant, n=3001, T=3, bias=True), label=f"{variant} T=3")
    assert averages and set(averages) == {k for k in got if k[0] == 0}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"f32math_averages_{variant}.json"), "w") as f:
        json.dump({"%d:%d:%s" % k: v for k, v in averages.items()}, f, indent=1)
    print(f"{variant} T=3 averages:", averages)


def test_separate_grids():
    run_wide_and_twin(build_case("MOM5", n=2003, T=2, sep_grids=(1999, 2011), bias=True), label="MOM5 separate u/v")


# ---------------------------------------------------------------- fused accumulation
def atmos_kw(la, outs):
    return lambda c: {"atmos": {"local": la, "fields": [(2, 1, g, k, outs[k]) for k, g in ATM_FIELDS]}}


def fused(variant, n, lengths, opts, label):
    from test_gpu_multirank import random_run_map

    amap = random_run_map(n, lengths, seed=lengths[1] + 5)
    la = local_atmos(amap, 0, 1)
    outs = {k: np.full(la.n_atmos, np.nan, np.float32) for k, _ in ATM_FIELDS}
    c32, got, _, _, _ = run_wide_and_twin(build_case(variant, n=n, T=1, bias=True, seed=23), opts, label,
                                          atmos=atmos_kw(la, outs))
    for k, g in ATM_FIELDS:
        flux = np.asarray(c32.lf.field[(1, g, k)], dtype=np.float64)
        want = oracle_lib.atmos_accumulate(amap.atmos_index, amap.weight, flux, amap.n_atmos).astype(np.float32)
        np.testing.assert_array_equal(outs[k], want, err_msg=f"{label}: atmosphere {k}")


FUSED_MODES = {"default": {}, "nohalo": {"atmos_halo": 0}, "capped": {"max_blocks": 64}}
FUSED_LENGTHS = [(1, 5), (1, 10), (40, 64), (0, 5)]


@pytest.mark.parametrize("lengths", FUSED_LENGTHS)
@pytest.mark.parametrize("mode", list(FUSED_MODES))
def test_fused_accumulation(mode, lengths):
    """Halo tiles, crossing records and their fix-up, a grid cap, empty atmosphere cells.  The
    per-type fluxes follow the twin rule; each atmosphere output is the fp32 engine's rule: the
    sequential fp64 sum of the engine's own stored fp32 fluxes, rounded once.  (The variant
    rotates over the cross, so each of the three wide fused kernels meets every mode.)"""
    variant = ("CCLM", "MOM5", "RCO")[(list(FUSED_MODES).index(mode) + FUSED_LENGTHS.index(lengths)) % 3]
    fused(variant, 70_001, lengths, FUSED_MODES[mode], f"{variant} {mode} runs{lengths}")


def test_fused_accumulation_pipelined():
    fused("MOM5", 300_001, (1, 10), {"pipeline_chunks": 4, "pipeline_min_chunk": 65536, "zero_copy": 0},
          "MOM5 pipelined")


# ---------------------------------------------------------------- group launch
def test_group_launch():
    """CCLM + MOM5 + RCO wide engines as one launch: every output is the bits of the same engines
    run singly."""
    import torch

    from fcx.workload import Workload

    res = []
    for grouped in (False, True):
        wl = Workload(20_011, 0, 1, ("CCLM", "MOM5", "RCO"), types=1, precision="f32w", bias=True, atmos=True,
                      atmos_map="random")
        try:
            assert all(e.f32_math() for e in wl.engines)
            for k in range(2):
                (wl.run_group if grouped else wl.run)(3600 * k)
            torch.cuda.synchronize()
            if grouped:
                assert wl.engines[0].last_group_size() == 3
            wl.download()
            got = {}
            for i, (case, outs) in enumerate(zip(wl.cases, wl.atm_outs)):
                got.update({(i,) + k: np.array(case.lf.field[k], copy=True) for k in case.outputs})
                got.update({(i, "atm", name): np.array(outs[name], copy=True) for name, _ in ATM_FIELDS})
            res.append(got)
        finally:
            wl.close()
    assert res[0].keys() == res[1].keys()
    for k in res[0]:
        assert res[0][k].dtype == np.float32 and np.isfinite(res[0][k]).all(), k
        np.testing.assert_array_equal(bits32(res[0][k]), bits32(res[1][k]), err_msg=str(k))


# ---------------------------------------------------------------- regridding
def test_regridding_staged():
    """The staged case of test_fp32_regridding_staged with the option on: the regridded arrays
    are the REAL(4) sequential sum of the engine's own t-grid values (regridding stays in float);
    every output passes the fp32 gate against the fp64 oracle."""
    from test_gpu_fp32 import check, regrid_f32

    rng = np.random.default_rng(7)
    case = build_case("CCLM", n=600, T=2, bias=False, sep_grids=(550, 520))
    nt, nu, nv = case.grid_size
    mats = {}
    for which, (ns, nd) in {2: (nt, nu), 3: (nt, nv)}.items():
        nnz = 3 * nd
        mats[which] = (rng.integers(1, ns + 1, nnz), np.repeat(np.arange(1, nd + 1), 3)[rng.permutation(nnz)],
                       rng.uniform(0.0, 1.0, nnz))
    case.regrid = {"matrices": mats}
    for s in (1, 2):
        case.methods["which_spec_vapor_surface_u"][s - 1] = "none"
        case.lf.put_to[(s, 1, "QSUR")] = 2
        case.lf.put_to[(s, 1, "MEVA")] = 4
        case.lf.allocate_localvar("MEVA", s, 3, value=np.nan)
        case.outputs.append((s, 3, "MEVA"))
    c32 = as_dtype(case, "float32")
    ref = oracle_lib.run_case(as_dtype(c32, "float64"), "c", current_step_time=STEP_T, regrid=True)
    eng = engine_of(c32, WIDE)
    try:
        eng.step(1, STEP_T)
        eng.step(2, STEP_T)
    finally:
        eng.close()
    check({k: np.array(c32.lf.field[k], dtype=np.float64) for k in c32.outputs}, ref, "f32math regrid")
    for s in (1, 2):
        src, dst, w = mats[2]
        want = regrid_f32(src, dst, w, np.asarray(c32.lf.field[(s, 1, "QSUR")]), nu)
        np.testing.assert_array_equal(np.asarray(c32.lf.field[(s, 2, "QSUR")]), want, err_msg=f"QSUR u s={s}")
        src, dst, w = mats[3]
        want = regrid_f32(src, dst, w, np.asarray(c32.lf.field[(s, 1, "MEVA")]), nv)
        np.testing.assert_array_equal(np.asarray(c32.lf.field[(s, 3, "MEVA")]), want, err_msg=f"MEVA v s={s}")


# ---------------------------------------------------------------- per call
def test_per_call_subroutines():
    """The fcx_calc_* sequence of a CCLM T = 2 case: a value read back from an array is the stored
    float, widened.  Before each call the wide engine's current arrays are copied, widened, into
    the twin's arrays; the twin makes the same call; the wide engine's result is np.float32(twin)."""
    c32 = as_dtype(build_case("CCLM", n=1001, T=2, bias=True), "float32")
    twin = twin_of(c32)
    for c in (c32, twin):  # (every output array defined before the first call reads it)
        for k in c.outputs:
            c.lf.field[k][:] = 0.0
    ew, et = engine_of(c32, WIDE), engine_of(twin)
    calls = [("fcx_calc_flux_radiation_blackbody", ())] + [("fcx_calc_spec_vapor_surface", (g,)) for g in (1, 2, 3)] + \
            [("fcx_calc_flux_mass_evap", (STEP_T,)), ("fcx_calc_flux_heat_latent", ()),
             ("fcx_calc_flux_heat_sensible", ()), ("fcx_calc_flux_momentum_east", (2,)),
             ("fcx_calc_flux_momentum_north", (3,))] + \
            [("fcx_average_across_surface_types", (g, IDX[name])) for _, g, name in c32.averages]
    try:
        for name, args in calls:
            done = set()
            for k, a in c32.lf.field.items():
                if id(a) not in done:
                    done.add(id(a))
                    twin.lf.field[k][:] = a
            for e in (ew, et):
                assert getattr(e.lib, name)(e.h, *args) == 0, (name, e.lib.fcx_last_error())
            for k in c32.outputs:
                ok = same32(c32.lf.field[k], twin.lf.field[k])
                assert ok.all(), f"{name}{args}: {k} is not np.float32(twin) in {int((~ok).sum())} cells"
    finally:
        ew.close()
        et.close()
    for k in c32.outputs:
        assert np.isfinite(c32.lf.field[k]).all(), k


# ---------------------------------------------------------------- unread outputs and constants
def test_unread_outputs_halo_launch():
    """MOM5, T = 1, the halo launch on the random map with all seven exchange-grid outputs
    unread: the atmosphere outputs are the bits of an undeclared wide engine's."""
    from test_gpu_output_use import ALL_SEVEN, N32, atmos_of, pair

    pair(lambda: as_dtype(build_case("MOM5", n=N32, T=1, bias=True), "float32"), ALL_SEVEN,
         extra=lambda c: atmos_of(c, N32, 1, dtype=np.float32), engine_kw={"options": dict(WIDE)},
         check=lambda eng, case: eng.f32_math() or pytest.fail("option not applied"), label="f32math MOM5 unread")


def test_constant_fields():
    """CCLM with FICE and PSUR constant (values that are not floats: rounded once): every output
    is the bits of a wide engine that binds the filled arrays."""
    from test_gpu_constant_fields import declare, poison, same, snapshot

    n, res = 1027, []
    for use in (True, False):
        case = as_dtype(build_case("CCLM", n=n, T=1, bias=True), "float32")
        declare(case, {(1, "FICE"): 0.3, (0, "PSUR"): 101325.7})
        eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, use_constants=use, options=WIDE)
        try:
            assert eng.f32_math()
            if use:
                assert set(k[2] for k in eng.constants) == {"FICE", "PSUR"}
                poison(eng)
            eng.step(PHASE_ALL, STEP_T)
            res.append(snapshot(case))
        finally:
            eng.close()
    same(res[0], res[1], "f32math constants")


# ---------------------------------------------------------------- the option itself
def test_applied_at_commit():
    c32 = as_dtype(build_case("CCLM", n=257, T=1), "float32")
    eng = engine_of(c32)
    try:
        assert not eng.f32_math()
        with pytest.raises(_lib.FcxError) as ex:
            eng.set_option("f32_math", 1)
        assert ex.value.status == E_STATE and "f32_math" in str(ex.value)
        assert not eng.f32_math()
    finally:
        eng.close()


def test_algorithmic_bytes_are_the_fp32_engines():
    for variant, T in (("CCLM", 1), ("MOM5", 2)):
        nbytes = []
        for opts in (None, WIDE):
            c32 = as_dtype(build_case(variant, n=10_000, T=T, bias=True), "float32")
            eng = engine_of(c32, opts)
            try:
                nbytes.append(eng.algorithmic_bytes(PHASE_ALL))
            finally:
                eng.close()
        assert nbytes[0] == nbytes[1] > 0, (variant, T, nbytes)
