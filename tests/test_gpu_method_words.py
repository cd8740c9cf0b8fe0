"""The run-time method bytes of the parameter block -- m_rbbr, m_hlat, bias_adds -- and the
remap records' rec_pos reach the kernels as aligned words decoded with shifts
(fcx_kernels.hip type_methods, RecEmit; the layout pinned in fcx_internal.h).  A wrong shift
or offset selects a wrong method, so every value of the three bytes runs on every kernel
family and is held to the oracle: the 1e-10 gate and the tight fp64 gates of tests/parity.py
for fp64, the fp32 norm gate for fp32.

Values: m_rbbr StBo / zero / none; m_hlat water / ice / zero / none; bias_adds 0 (no
corrections), 1, and 2 (a 'copy' alias of MEVA, T = 2).  The bias is compared on both sides of
a month boundary (31 January and 1 February 1961: two different slices of the corrections).
Sizes: n = 1, 127, 129, 499 -- odd, so the last lane's partial vector runs; 129 crosses a
4-wave block's first wave tile, 499 a 124-cell halo tile and a block.  The atmosphere map is the
benchmark's random one (runs of 3-5 cells)."""
import numpy as np
import pytest

import oracle_lib
from parity import FP32_NORM_GATE, assert_parity, assert_tight, error_report

pytestmark = pytest.mark.gpu

fcx = pytest.importorskip("fcx")
from fcx.basic import PHASE_ALL, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.parallel import BlockedRandomAtmosMap, local_atmos, synthetic_model_map  # noqa: E402
from fcx.synthetic import as_dtype, build_case  # noqa: E402
from fcx.workload import ATM_FIELDS  # noqa: E402

T_JAN = 3600 * 24 * 30  # 31 January 1961: month 1 slice
T_FEB = 3600 * 24 * 31  # 1 February 1961: month 2 slice
TIMES = (T_JAN, T_FEB)
SIZES = (1, 127, 129, 499)
VARIANTS = ("CCLM", "MOM5", "RCO")
# (m_rbbr, m_hlat, bias): every value of each byte at least once; bias 2 needs a second type
COMBOS = {
    "stbo_water_b1": ("StBo", "water", True),
    "zero_ice_b0": ("zero", "ice", False),
    "none_zero_b1": ("none", "zero", True),
    "stbo_none_b0": ("StBo", "none", False),
}
_ORACLE = {}


def methods_of(combo, extra=None):
    rbbr, hlat, _ = COMBOS[combo]
    m = dict(which_flux_radiation_blackbody=rbbr, which_flux_heat_latent=hlat)
    m.update(extra or {})
    return m


def oracle(case, t, key):
    """the oracle's outputs of a case, computed once per (case key, time)"""
    if (key, t) not in _ORACLE:
        _ORACLE[(key, t)] = oracle_lib.run_case(case, "c", current_step_time=t)
    return _ORACLE[(key, t)]


def outputs(case):
    return {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}


def hold(case, got, t, label, key):
    ref = oracle(case, t, key)
    assert_parity(got, ref, label=label)
    assert_tight(case, got, ref, t, label, report=False)


def atm_names(case):
    """the fluxes sent to the atmosphere that the case produces (method not 'none')"""
    return [(name, g) for name, g in ATM_FIELDS if case.lf.associated(1, g, name)
            and ((1, 1, name) in case.outputs or (1, g, name) in case.outputs)]


def check_atmos(case, amap, outs, label):
    """the fused accumulation of the engine's own fluxes, bit for bit in link order"""
    for name, g in atm_names(case):
        want = oracle_lib.atmos_accumulate(amap.atmos_index, amap.weight, np.asarray(case.lf.field[(1, g, name)]),
                                           amap.n_atmos)
        np.testing.assert_array_equal(outs[name], want, err_msg=f"{label} atmos {name}")


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("n", SIZES)
def test_generic_kernel(combo, n):
    """VAR = 0, TM = 1: MEVA MOM5, HSEN RCO, momentum CCLM -- a mix no specialisation takes, so
    all eight method bytes are decoded at run time."""
    mix = dict(which_flux_mass_evap="MOM5", which_flux_heat_sensible="RCO", which_flux_momentum="CCLM")
    case = build_case("CCLM", n=n, T=1, bias=COMBOS[combo][2], per_type={1: methods_of(combo, mix)})
    eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, averages=case.averages)
    try:
        for t in TIMES:
            eng.step(PHASE_ALL, t)
            hold(case, outputs(case), t, f"generic {combo} n={n} t={t}", ("generic", combo, n))
    finally:
        eng.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("combo", list(COMBOS))
def test_specialised_fused(variant, combo):
    """T = 1, VAR = 1/2/3 with the exchange -> atmosphere accumulation in the launch
    (cells_atmos_kernel): RBBR and HLAT methods and the bias count stay run-time bytes."""
    for n in SIZES:
        case = build_case(variant, n=n, T=1, bias=COMBOS[combo][2], per_type={1: methods_of(combo)})
        amap = BlockedRandomAtmosMap().global_map(n)
        names = atm_names(case)
        outs = {name: np.full(amap.n_atmos, np.nan) for name, _ in names}
        atmos = {"local": local_atmos(amap, 0, 1), "fields": [(PHASE_NORMAL, 1, g, name, outs[name]) for name, g in names]}
        eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, averages=case.averages, atmos=atmos)
        try:
            for t in TIMES:
                eng.step(PHASE_ALL, t)
                label = f"fused {variant} {combo} n={n} t={t}"
                hold(case, outputs(case), t, label, ("spec", variant, combo, n))
                check_atmos(case, amap, outs, label)
        finally:
            eng.close()


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("n", SIZES)
def test_specialised_group(combo, n):
    """The three T = 1 specialisations as members of ONE fcx_run_group launch
    (cells_atmos_group_kernel), each member with its own parameter block."""
    import torch

    amap = BlockedRandomAtmosMap().global_map(n)
    la = local_atmos(amap, 0, 1)
    stream = torch.cuda.current_stream().cuda_stream
    cases, engines, keep = [], [], []
    try:
        for v in VARIANTS:
            c = build_case(v, n=n, T=1, bias=COMBOS[combo][2], per_type={1: methods_of(combo)})
            names = atm_names(c)
            o = {name: np.full(amap.n_atmos, np.nan) for name, _ in names}
            atmos = {"local": la, "fields": [(PHASE_NORMAL, 1, g, name, o[name]) for name, g in names]}
            engines.append(Engine(c.lf, 1, c.methods, corrections=c.corrections, averages=c.averages, atmos=atmos,
                                  stream=stream, options={"atmos_in_run": 0, "timing": 0, "host_staging": 0}))
            cases.append(c)
            keep.append(o)
        for e in engines:
            e.upload(PHASE_ALL)
        for t in TIMES:
            run_group(engines, PHASE_ALL, t)
            for e in engines:
                e.run_atmos(PHASE_ALL)
                e.download(PHASE_ALL)
                e.synchronize()
            assert [e.last_group_size() for e in engines] == [len(VARIANTS)] * len(VARIANTS)  # one merged launch
            for v, c, o in zip(VARIANTS, cases, keep):
                label = f"group {v} {combo} n={n} t={t}"
                hold(c, outputs(c), t, label, ("spec", v, combo, n))
                check_atmos(c, amap, o, label)
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("variant", ["CCLM", "MOM5"])
@pytest.mark.parametrize("alias", [False, True], ids=["b1", "b2_copy"])
@pytest.mark.parametrize("n", SIZES)
def test_two_types(variant, alias, n):
    """T = 2, water + ice: the two types carry different m_hlat bytes (TM = 0 kernels).  alias:
    type 2's MEVA is a 'copy' of type 1's, so type 1 adds the bias twice (bias_adds 2) and the
    launch falls to the generic multi-type kernel."""
    per_type = {2: dict(which_flux_mass_evap="copy")} if alias else None
    case = build_case(variant, n=n, T=2, bias=True, per_type=per_type)
    eng = Engine(case.lf, 2, case.methods, corrections=case.corrections, averages=case.averages)
    try:
        for t in TIMES:
            eng.step(PHASE_ALL, t)
            hold(case, outputs(case), t, f"T2 {variant} alias={alias} n={n} t={t}", ("t2", variant, alias, n))
    finally:
        eng.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("combo", list(COMBOS))
def test_fp32(variant, combo):
    """The fp32 engine's specialised kernels (4 cells per lane) read the same words."""
    for n in SIZES:
        case = build_case(variant, n=n, T=1, bias=COMBOS[combo][2], per_type={1: methods_of(combo)})
        c32 = as_dtype(case, "float32")
        c64 = as_dtype(c32, "float64")  # exactly the inputs the fp32 kernel saw
        eng = Engine(c32.lf, 1, c32.methods, corrections=c32.corrections, averages=c32.averages)
        try:
            for t in TIMES:
                eng.step(PHASE_ALL, t)
                got = {k: np.array(c32.lf.field[k], dtype=np.float64) for k in c32.outputs}
                ref = oracle_lib.run_case(c64, "c", current_step_time=t)
                assert set(got) == set(ref)
                bad = {k: v for k, v in error_report(got, ref).items() if not v[0] <= FP32_NORM_GATE}
                assert not bad, f"fp32 {variant} {combo} n={n} t={t}: norm-wise error over {FP32_NORM_GATE}: {bad}"
        finally:
            eng.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [129, 499])
def test_remap_records(variant, n):
    """Remap records written by the T = 1 flux launch itself (REC kernels): rec_pos places the
    register slots in the record.  HLAT, RBBR, MEVA, VMOM in this order, so the positions differ
    from the slot numbers; the remap of the engine's own fluxes bit for bit."""
    fields = (("HLAT", 1), ("RBBR", 1), ("MEVA", 1), ("VMOM", 3))
    case = build_case(variant, n=n, T=1, bias=True)
    mmap = synthetic_model_map(n, max(n // 4, 1), links_per_cell=2, seed=12)
    outs = {k: np.full(mmap.n_model, np.nan) for k, _ in fields}
    remap = {"n_dst": mmap.n_model, "src": mmap.src, "dst": mmap.dst, "w": mmap.weight,
             "fields": [(PHASE_NORMAL, 1, g, name, outs[name]) for name, g in fields]}
    eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, remaps=[remap], options={"remap_pack": 1})
    try:
        for t in TIMES:
            eng.step(PHASE_ALL, t)
            assert eng.remap_info(0)[1] == 2  # the records came from the flux launch
            label = f"records {variant} n={n} t={t}"
            hold(case, outputs(case), t, label, ("rec", variant, n))
            for name, g in fields:
                want = oracle_lib.remap_apply(mmap.src, mmap.dst, mmap.weight, np.asarray(case.lf.field[(1, g, name)]),
                                              mmap.n_model)
                np.testing.assert_array_equal(outs[name], want, err_msg=f"{label} {name}")
    finally:
        eng.close()
