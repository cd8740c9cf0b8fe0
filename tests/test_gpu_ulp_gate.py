"""libfcx (HIP, gfx950) held to the tight fp64 gates of tests/parity.py::assert_tight: every
output cell bit-identical to the oracle, bit-identical to the oracle seeded with the device's
own QSUR, or inside a bound derived from the 1-ulp exp/log of the three transcendental sites
of fcx_physics.h.  The 1e-10 gate beside it lets a constant wrong in its 12th digit, a
contracted FMA, a non-IEEE sqrt or division and a reordered sum through; these do not.

Each test names the path of fcx_kernels.hip process<> it reaches.  Sizes are at least 300
(the calm, T_a == T_s and vel ~ 11 cells of fcx/synthetic.py exist from there); the smaller
ones are for the partial vectors only.  parity.write_report keeps a report per case,
ulp_gate_<label>.json, and the worst figures over the module, ulp_gate_summary.json."""
import numpy as np
import pytest

import oracle_lib
from parity import assert_tight, write_report

pytestmark = pytest.mark.gpu

fcx = pytest.importorskip("fcx")
from fcx.basic import PHASE_ALL, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.synthetic import build_case  # noqa: E402
from fcx.workload import ATM_FIELDS, Workload  # noqa: E402

STEP_T = 3600 * 24 * 31  # inside February of 1961: month 2 bias slice
VARIANTS = ("CCLM", "MOM5", "RCO")
SUMMARY = {}


def tight(case, got, label):
    """assert_tight against the plain oracle; the module's worst figures per field and gate"""
    ref = oracle_lib.run_case(case, "c", current_step_time=STEP_T)
    rep = assert_tight(case, got, ref, STEP_T, label)
    for key, v in rep.items():
        name = ("avg " if key.startswith("0:") else "") + key.split(":")[2] + " [" + v["gate"] + "]"
        s = SUMMARY.setdefault(name, {"cells": 0, "bit_identical_cells": 0, "worst_ratio": 0.0, "cases": 0})
        s["cells"] += v["cells"]
        s["bit_identical_cells"] += int(round(v["bit_identical_share"] * v["cells"]))
        s["worst_ratio"] = max(s["worst_ratio"], v["worst_ratio"])
        s["cases"] += 1
    write_report("ulp_gate_summary", SUMMARY)
    return rep


def fused(case, options=None):
    eng = Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                 averages=case.averages, regrid=case.regrid, options=options)
    eng.step(PHASE_ALL, STEP_T)
    got = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}
    eng.close()
    return got


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", ["default", "generic", "one_cell"])
@pytest.mark.parametrize("n", [1, 2, 3, 129, 300, 4097])
def test_single_type(variant, mode, n):
    """T = 1, bias on.  default: the specialised VAR = 1/2/3, TM = 1, C = 2 instance; generic:
    specialize=0, VAR = 0 (methods read at run time); one_cell: cells_per_thread=1.  n = 1, 2, 3:
    partial vectors; 129: one cell past a wave tile; 4097: several blocks and a tail."""
    options = {"default": None, "generic": {"specialize": 0}, "one_cell": {"cells_per_thread": 1}}[mode]
    case = build_case(variant, n=n, T=1, bias=True)
    tight(case, fused(case, options), f"{variant}_T1_n{n}_{mode}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("n", [300, 4097])
def test_multi_type(variant, T, n):
    """T = 2, 3: the type-0 averages in registers (RAVG), ta_exner / rate_num / mom_num formed
    once per cell (kDerive), the next type's prefetch.  Type 2 is ice: HLAT uses kLs."""
    case = build_case(variant, n=n, T=T, bias=True)
    tight(case, fused(case), f"{variant}_T{T}_n{n}")


def test_ten_surface_types():
    case = build_case("MOM5", n=777, T=10, bias=True)
    tight(case, fused(case), "MOM5_T10_n777")


@pytest.mark.parametrize("variant", VARIANTS)
def test_separate_uv_grids(variant):
    """(n, nu, nv) = (300, 310, 290), T = 2: the non-merged uv_grid path; QSUR of the u and v
    grids is the device's own array of that grid in the seeded run."""
    case = build_case(variant, n=300, T=2, bias=True, sep_grids=(310, 290))
    tight(case, fused(case), f"{variant}_T2_sep")


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("lengths", [(3, 5), (1, 10)])
def test_timed_kernel(lengths, T):
    """The three variants in ONE fcx_run_group launch with the fused exchange -> atmosphere
    accumulation, n = 300.  Runs of 3-5 cells (the benchmark's random map): halo tiles; runs of
    1-10 cells: crossing records and the fix-up.  The flux outputs are held to the tight gates;
    the atmosphere outputs stay with the bit-exact accumulation tests."""
    import torch

    n = 300
    if lengths == (3, 5):
        wl = Workload(n, 0, 1, VARIANTS, types=T, bias=True, atmos=True, atmos_map="random")
        wl.run_group(STEP_T)
        torch.cuda.synchronize()
        wl.download()
        cases, engines = wl.cases, wl.engines
    else:
        from fcx.parallel import local_atmos
        from test_gpu_multirank import random_run_map

        la = local_atmos(random_run_map(n, lengths, seed=41), 0, 1)
        cases, engines, keep = [], [], []
        stream = torch.cuda.current_stream().cuda_stream
        for v in VARIANTS:
            c = build_case(v, n=n, T=T, bias=True)
            o = {name: torch.full((la.n_atmos,), float("nan"), dtype=torch.float64, device="cuda:0")
                 for name, _ in ATM_FIELDS}
            atmos = {"local": la, "fields": [(PHASE_NORMAL, 0 if T >= 2 else 1, g, name, o[name])
                                             for name, g in ATM_FIELDS]}
            engines.append(Engine(c.lf, T, c.methods, corrections=c.corrections, averages=c.averages, atmos=atmos,
                                  stream=stream,  # (one stream: engines on different streams are not merged)
                                  options={"atmos_in_run": 0, "timing": 0, "host_staging": 0}))
            cases.append(c)
            keep.append(o)
        for e in engines:
            e.upload(PHASE_ALL)
        run_group(engines, PHASE_ALL, STEP_T)
        for e in engines:
            e.run_atmos(PHASE_ALL)
            e.download(PHASE_ALL)
            e.synchronize()
    try:
        assert [e.last_group_size() for e in engines] == [len(VARIANTS)] * len(VARIANTS)  # one merged launch
        for v, c in zip(VARIANTS, cases):
            got = {k: np.array(c.lf.field[k], copy=True) for k in c.outputs}
            tight(c, got, f"group_{v}_T{T}_runs{lengths[0]}-{lengths[1]}")
    finally:
        for e in engines:
            e.close()


def test_unaligned_device_pointers():
    """Device arrays 8-byte but not 16-byte aligned: the scalar load path (CCLM, n = 1001)."""
    torch = pytest.importorskip("torch")
    case_h = build_case("CCLM", n=1001, T=1, bias=False)
    case = build_case("CCLM", n=1001, T=1, bias=False, device="cuda:0")
    shifted = {}
    for key, a in list(case.lf.field.items()):
        if id(a) not in shifted:
            b = torch.empty(a.shape[0] + 1, dtype=torch.float64, device="cuda:0")[1:]
            b.copy_(a)
            shifted[id(a)] = b
        case.lf.field[key] = shifted[id(a)]
    eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, averages=case.averages)
    eng.run(PHASE_ALL, STEP_T)
    eng.synchronize()
    got = {k: case.lf.to_numpy(*k) for k in case.outputs}
    eng.close()
    tight(case_h, got, "CCLM_T1_unaligned")


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
    """The four per_type sets of test_gpu_parity.py::test_method_edges, T = 3, n = 1025.  A 'copy'
    alias is the aliased type-1 array and takes its class; the bias added once more per aliased
    copy is reproduced by the seeded oracle.  All four sets classify cleanly: none copies the
    bounded RCO MEVA (which gate_of would refuse), the copied HSEN of all_copy gets no further
    operation and keeps its bound."""
    case = build_case("CCLM", n=1025, T=3, bias=True, per_type=per_type)
    tight(case, fused(case), "edges_" + request.node.callspec.id)
