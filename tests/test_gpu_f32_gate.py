"""The plain fp32 engines (FCX_PRECISION_F32 without FCX_OPT_F32_MATH) held to the tight gates of
tests/parity.py::assert_tight_f32, case for case as tests/test_gpu_ulp_gate.py holds the fp64
ones: every output cell bit-identical to the float32 restatement tests/f32_expect.py (pinned to
fcx_physics.h's host build by tests/test_f32_expect.py), bit-identical to it seeded with the
device's own QSUR, or inside a bound derived from 1-ulp expf / logf.  FP32_NORM_GATE beside it
lets a constant wrong in its 6th digit, a contracted FMA, a constant folded in float and a
reordered sum through; these do not.

Each test names the instantiation of fcx_kernels.hip process<> it reaches.  Every case has the
bias on and steps inside February.  parity.write_report keeps a report per case,
f32_gate_<label>.json, and the worst figures over the module, f32_gate_summary.json."""
import numpy as np
import pytest

from parity import assert_tight_f32, write_report

pytestmark = pytest.mark.gpu

fcx = pytest.importorskip("fcx")
from fcx import _lib  # noqa: E402
from fcx.basic import PHASE_ALL, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine  # noqa: E402
from fcx.parallel import local_atmos  # noqa: E402
from fcx.synthetic import as_dtype, build_case  # noqa: E402
from fcx.workload import ATM_FIELDS, Workload  # noqa: E402

STEP_T = 3600 * 24 * 31  # inside February of 1961: month 2 bias slice
MARCH_T = 3600 * 24 * (31 + 28)  # the first second of March 1961: month 3
VARIANTS = ("CCLM", "MOM5", "RCO")
SUMMARY = {}


def tight(c32, got, label, t=STEP_T):
    """assert_tight_f32; the module's worst figures per field and gate"""
    rep = assert_tight_f32(c32, got, t, label)
    for key, v in rep.items():
        name = ("avg " if key.startswith("0:") else "") + key.split(":")[2] + " [" + v["gate"] + "]"
        s = SUMMARY.setdefault(name, {"cells": 0, "bit_identical_cells": 0, "worst_ratio": 0.0, "cases": 0})
        s["cells"] += v["cells"]
        s["bit_identical_cells"] += int(round(v["bit_identical_share"] * v["cells"]))
        s["worst_ratio"] = max(s["worst_ratio"], v["worst_ratio"])
        s["cases"] += 1
    write_report("f32_gate_summary", SUMMARY)
    return rep


def outputs(c32):
    got = {k: np.array(c32.lf.field[k], copy=True) for k in c32.outputs}
    assert all(v.dtype == np.float32 for v in got.values())
    return got


def fused(c32, options=None, t=STEP_T, **kw):
    eng = Engine(c32.lf, c32.num_surface_types, c32.methods, corrections=c32.corrections,
                 averages=c32.averages, regrid=c32.regrid, options=options, **kw)
    try:
        eng.step(PHASE_ALL, t)
    finally:
        eng.close()
    return outputs(c32)


def case32(variant, **kw):
    return as_dtype(build_case(variant, bias=True, **kw), "float32")


MODES = {"default": None, "generic": {"specialize": 0}, "one_cell": {"cells_per_thread": 1}}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [1, 3, 5, 255, 257, 300, 4099])
def test_single_type(variant, mode, n):
    """T = 1.  default: cells_kernel<4, merged, VAR = 1/2/3, float, TM = 1> (4 cells per lane,
    16-B loads); generic: specialize=0, VAR = 0; one_cell: cells_per_thread=1, C = 1.  n = 1, 3,
    5: partial 4-cell lanes; 255, 257: one cell either side of a 256-cell tile; 4099: several
    blocks and a tail; 300: the calm, T_a == T_s and vel ~ 11 cells of fcx/synthetic.py."""
    c32 = case32(variant, n=n, T=1)
    tight(c32, fused(c32, MODES[mode]), f"{variant}_T1_n{n}_{mode}")


def test_month_boundary():
    """One engine over the month boundary: February's bias slice, then March's (CCLM, T = 1)."""
    c32 = case32("CCLM", n=300, T=1)
    eng = Engine(c32.lf, 1, c32.methods, corrections=c32.corrections, averages=c32.averages)
    try:
        eng.step(PHASE_ALL, STEP_T)
        feb = outputs(c32)
        tight(c32, feb, "CCLM_T1_n300_february")
        eng.step(PHASE_ALL, MARCH_T)
        march = outputs(c32)
        tight(c32, march, "CCLM_T1_n300_march", t=MARCH_T)
    finally:
        eng.close()
    assert not np.array_equal(feb[(1, 1, "MEVA")], march[(1, 1, "MEVA")])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("n", [300, 4099])
def test_multi_type(variant, T, n):
    """T = 2, 3: cells_kernel<4, merged, VAR, float, TM = 0, RAVG> -- the type-0 averages in
    float registers, ta_exner / rate_num / mom_num formed once per cell (kDerive), the next
    type's prefetch.  Type 2 is ice: HLAT uses float(kLs)."""
    c32 = case32(variant, n=n, T=T)
    tight(c32, fused(c32), f"{variant}_T{T}_n{n}")


def test_ten_surface_types():
    c32 = case32("MOM5", n=777, T=10)
    tight(c32, fused(c32), "MOM5_T10_n777")


@pytest.mark.parametrize("variant", VARIANTS)
def test_separate_uv_grids(variant):
    """(n, nu, nv) = (300, 310, 290), T = 2: the non-merged uv_grid<float> path; the UMOM / VMOM
    averages are not register averages there but the S_AVG pass of process<> over the stored
    floats; QSUR of the u and v grids is the device's own array of that grid in the seeded run."""
    c32 = case32(variant, n=300, T=2, sep_grids=(310, 290))
    tight(c32, fused(c32), f"{variant}_T2_sep")


@pytest.mark.parametrize("per_type", [
    {2: dict(which_flux_mass_evap="copy", which_flux_heat_latent="water")},
    {2: dict(which_flux_mass_evap="zero", which_flux_heat_sensible="zero",
             which_flux_momentum="zero", which_flux_radiation_blackbody="zero")},
    {3: dict(which_flux_mass_evap="copy", which_flux_heat_latent="copy",
             which_flux_heat_sensible="copy", which_flux_momentum="copy",
             which_flux_radiation_blackbody="copy", which_spec_vapor_surface_t="copy",
             which_spec_vapor_surface_u="copy", which_spec_vapor_surface_v="copy")},
    {1: dict(which_flux_mass_evap="RCO"), 2: dict(which_flux_heat_sensible="RCO")},
], ids=["meva_copy", "zero", "all_copy", "mixed_rco"])
def test_method_edges(per_type, request):
    """The four per_type sets of test_gpu_ulp_gate.py::test_method_edges, T = 3, n = 1025: the
    generic VAR = 0 float kernel.  An average over a 'copy' alias is no register average: it goes
    through the S_AVG pass (meva_copy, all_copy); the bias added once more per alias and zeros<>
    at R = float are held too."""
    c32 = case32("CCLM", n=1025, T=3, per_type=per_type)
    tight(c32, fused(c32), "edges_" + request.node.callspec.id)


def run_map(n, lengths):
    from test_gpu_multirank import random_run_map

    return local_atmos(random_run_map(n, lengths, seed=lengths[1] + 5), 0, 1)


ACC_MODES = {"default": {}, "nohalo": {"atmos_halo": 0}, "capped": {"max_blocks": 64}}
ACC_LENGTHS = [(1, 9), (40, 64)]
ACC_CASES = [(m, ln, T) for m in ACC_MODES for ln in ACC_LENGTHS for T in (1, 2)]


@pytest.mark.parametrize("mode,lengths,T", ACC_CASES,
                         ids=[f"{m}-runs{ln[0]}_{ln[1]}-T{T}" for m, ln, T in ACC_CASES])
def test_fused_accumulation(mode, lengths, T):
    """70,001 cells with the exchange -> atmosphere accumulation fused into the flux launch:
    cells_atmos_kernel<4, float, VAR, TM = 1> with halo tiles (default), crossing records and the
    fix-up (atmos_halo: 0, runs of 40-64 cells), a grid-stride cap (max_blocks: 64); T = 2: the
    fused register-average kernel.  One variant per combination, rotating over the cross so that
    each kernel meets every mode.  The fluxes are held here; the atmosphere outputs stay with
    the bit-exact accumulation tests."""
    n = 70_001
    i = ACC_CASES.index((mode, lengths, T))
    variant = VARIANTS[(list(ACC_MODES).index(mode) + ACC_LENGTHS.index(lengths) + T) % 3]
    c32 = case32(variant, n=n, T=T, seed=23)
    la = run_map(n, lengths)
    outs = {k: np.full(max(la.n_atmos, 1), np.nan, np.float32) for k, _ in ATM_FIELDS}
    atmos = {"local": la, "fields": [(PHASE_NORMAL, 0 if T >= 2 else 1, g, k, outs[k]) for k, g in ATM_FIELDS]}
    eng = Engine(c32.lf, T, c32.methods, corrections=c32.corrections, averages=c32.averages, atmos=atmos,
                 options=dict(ACC_MODES[mode]))
    try:
        assert eng.fused_accumulation(PHASE_ALL), (i, variant)
        eng.step(PHASE_ALL, STEP_T)
    finally:
        eng.close()
    assert all(np.isfinite(o[:la.n_atmos]).all() for o in outs.values())
    tight(c32, outputs(c32), f"fusedacc_{variant}_T{T}_{mode}_runs{lengths[0]}-{lengths[1]}")


@pytest.mark.parametrize("T", [1, 2])
def test_group_launch(T):
    """The three variants in ONE fcx_run_group launch (cells_atmos_group_kernel, float), n = 300,
    the random map's runs of 3-5 cells."""
    import torch

    wl = Workload(300, 0, 1, VARIANTS, types=T, precision="f32", bias=True, atmos=True, atmos_map="random")
    try:
        wl.run_group(STEP_T)
        torch.cuda.synchronize()
        wl.download()
        assert [e.last_group_size() for e in wl.engines] == [3, 3, 3]  # one merged launch
        for v, c in zip(VARIANTS, wl.cases):
            tight(c, outputs(c), f"group_{v}_T{T}")
    finally:
        wl.close()


def test_unaligned_device_pointers():
    """Device float arrays 4-byte but not 16-byte aligned: the scalar load path (CCLM, n = 1001)."""
    torch = pytest.importorskip("torch")
    host = as_dtype(build_case("CCLM", n=1001, T=1, bias=True), "float32")
    c32 = as_dtype(build_case("CCLM", n=1001, T=1, bias=True, device="cuda:0"), "float32")
    shifted = {}
    for key, a in list(c32.lf.field.items()):
        if id(a) not in shifted:
            assert a.dtype == torch.float32
            b = torch.empty(a.shape[0] + 1, dtype=torch.float32, device="cuda:0")[1:]
            b.copy_(a)
            shifted[id(a)] = b
        c32.lf.field[key] = shifted[id(a)]
    eng = Engine(c32.lf, 1, c32.methods, corrections=c32.corrections, averages=c32.averages)
    try:
        eng.run(PHASE_ALL, STEP_T)
        eng.synchronize()
        got = {k: c32.lf.to_numpy(*k) for k in c32.outputs}
    finally:
        eng.close()
    tight(host, got, "CCLM_T1_unaligned")


def test_declared_constant():
    """FICE of the ice type declared a constant (MOM5, T = 2, register averages: the engine binds
    an array it filled).  The engine's own host array is overwritten with NaN after the commit;
    the restatement runs on a twin case that still holds the value."""
    from test_gpu_constant_fields import declare, poison

    def make():
        c = case32("MOM5", n=4100, T=2)
        declare(c, {(2, "FICE"): 1.0})
        return c

    c32, twin = make(), make()
    eng = Engine(c32.lf, 2, c32.methods, corrections=c32.corrections, averages=c32.averages, use_constants=True)
    try:
        assert {k[2] for k in eng.constants} == {"FICE"}
        poison(eng)
        eng.step(PHASE_ALL, STEP_T)
    finally:
        eng.close()
    tight(twin, outputs(c32), "MOM5_T2_constant_FICE")


def test_device_kept_output():
    """QSUR declared FCX_OUT_DEVICE (CCLM, T = 1): no download, the host array untouched; the
    gate reads the device array behind the slot, and MEVA / UMOM / VMOM are held to the
    restatement seeded with it."""
    from test_gpu_output_use import read_device

    n = 4099
    c32 = case32("CCLM", n=n, T=1)
    key = (1, 1, "QSUR")
    c32.lf.field[key][:] = -1.0
    eng = Engine(c32.lf, 1, c32.methods, corrections=c32.corrections, averages=c32.averages,
                 output_use={key: _lib.FCX_OUT_DEVICE})
    try:
        eng.step(PHASE_ALL, STEP_T)
        q = read_device(eng, key, n, dtype=np.float32)
    finally:
        eng.close()
    assert (c32.lf.field[key] == -1.0).all()  # kept on the device: not downloaded
    got = outputs(c32)
    got[key] = q
    tight(c32, got, "CCLM_T1_device_QSUR")
