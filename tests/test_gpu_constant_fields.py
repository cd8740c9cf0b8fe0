"""Namelist-constant input fields on the GPU (fcx_bind_constant).

The oracle is a TWIN: the same case with the same arrays, every declared field filled with its
value, bound as ordinary arrays (use_constants=False).  A constant differs from such an array
in nothing but where the engine takes it from, so every output of the constant engine is
bit-identical to the twin's (parity.bits_equal, no tolerance).  In the constant engine the
declared host arrays are overwritten with NaN once the engine is committed: finite outputs equal
to the twin's show that the arrays are never read again.  One T = 2 case is also held to
parity.assert_tight against the C oracle.

fcx_constant_info after the run says where the flux pass took the constant from.  1: a
wave-uniform value of the parameter block, no device array and no HBM stream -- the fp64
generic and CCLM kernels without register averages.  2: a device array the engine filled --
the kernel families that take no uniforms (fp32, MOM5, RCO: they spilled or lost a wave per
SIMD with the uniform path; the register-average kernels: the T = 2 step was 2.6 % slower
with it) and every constant something outside the flux pass reads (a regrid source, FARE,
an averaged, accumulated or remapped field, fcx_device_ptr).  Each test names the kind it
expects, so the uniform cases do run the mask, held-input and dead-lane logic."""
import ctypes

import numpy as np
import pytest

import namelists
import oracle_lib
from parity import assert_tight, bits_equal

pytestmark = pytest.mark.gpu

from fcx import _lib, driver, host_alloc  # noqa: E402
from fcx.basic import IDX, PHASE_ALL, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.parallel import BlockedRandomAtmosMap, synthetic_model_map  # noqa: E402
from fcx.setup import setup_from_namelist  # noqa: E402
from fcx.synthetic import SyntheticCoupler, as_dtype, build_case, corrections  # noqa: E402

T_STEP = 3600 * 24 * 45
# a typical value of every kernel input (SURVEY 8d ranges); FICE, UATM and VATM also run at 0.0
TYPICAL = {"TSUR": 285.25, "FICE": 1.0, "PSUR": 101325.0, "PATM": 100817.5, "QATM": 0.0081, "TATM": 283.6,
           "UATM": 3.5, "VATM": -2.25, "AMOI": 1.5e-3, "AMOM": 1.2e-3, "CMOI": 1.3e-3, "CHEA": 1.1e-3,
           "CMOM": 1.4e-3}
ZERO = ("FICE", "UATM", "VATM")  # open water, calm
ATMOS = ("PSUR", "PATM", "QATM", "TATM", "UATM", "VATM", "AMOI", "AMOM")
READS = {"CCLM": ("TSUR", "FICE", "PSUR", "PATM", "QATM", "TATM", "UATM", "VATM", "AMOI", "AMOM"),
         "MOM5": ("TSUR", "FICE", "PSUR", "PATM", "QATM", "TATM", "UATM", "VATM", "CMOI", "CHEA", "CMOM"),
         "RCO": ("TSUR", "QATM", "TATM", "UATM", "VATM")}
ATM_FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))


def declare(case, consts):
    """consts: {(s, name): value}: filled and recorded on every grid that has the field (an
    atmosphere field is declared for type 0 and reaches its aliases)."""
    lf = case.lf
    for (s, name), v in consts.items():
        for g in (1, 2, 3):
            if (s, g, name) in lf.field and lf.constant.get((s, g, name)) != v:
                lf.set_constant(name, s, g, v)


def poison(eng):
    """NaN into every host array the engine declared constant (after commit)."""
    seen = set()
    for key in eng.constants:
        a = eng.lf.field[key]
        if isinstance(a, np.ndarray) and id(a) not in seen:
            seen.add(id(a))
            a[:] = np.nan


def snapshot(case, extra=None):
    got = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}
    for k, a in (extra or {}).items():
        got[k] = np.array(a, copy=True)
    return got


def same(got, twin, label):
    assert got.keys() == twin.keys(), label
    for k in got:
        assert np.all(np.isfinite(got[k])), f"{label}: {k} not finite"
        bad = ~bits_equal(got[k], twin[k])
        assert not bad.any(), f"{label}: {k} differs from the twin in {int(bad.sum())} cells, first {int(np.argmax(bad))}"


def step_once(eng):
    eng.step(PHASE_ALL, T_STEP)


def pair(make, consts, run=step_once, engine_kw=None, extra=None, check=None, label="", kind=1):
    """The constant engine and its twin over two builds of the same case; returns both
    snapshots.  make() -> case (deterministic); extra(case) -> {key: array} of further outputs
    and engine keywords (atmos=, remaps=) as (kw, arrays); check(eng, case) runs on the constant
    engine before it is closed; kind: fcx_constant_info of every declared constant after the run."""
    out = []
    for use in (True, False):
        case = make()
        declare(case, consts)
        kw, arrays = extra(case) if extra else ({}, {})
        kw = dict(kw, **(engine_kw or {}))
        eng = Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                     averages=case.averages, use_constants=use, **kw)
        try:
            if use:
                assert eng.constants, label
                poison(eng)
            else:
                assert not eng.constants
            run(eng)
            if use:
                for key in eng.constants:
                    assert eng.constant_info(*key) == kind, (label, key, eng.constant_info(*key), kind)
            if use and check:
                check(eng, case)
            out.append((snapshot(case, arrays), case))
        finally:
            eng.close()
    same(out[0][0], out[1][0], label)
    return out[0], out[1]


# ---------------------------------------------------------------- each kernel input, T = 1
@pytest.mark.parametrize("specialize", [1, 0])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_each_input_in_turn(variant, specialize):
    """Every input the variant reads, one at a time with its typical value, FICE / UATM / VATM
    also at 0.0, then all bottom-side inputs together; 1 and 2 cells per lane."""
    cases = [{(0 if name in ATMOS else 1, name): TYPICAL[name]} for name in READS[variant]]
    cases += [{(0 if name in ATMOS else 1, name): 0.0} for name in READS[variant] if name in ZERO]
    cases.append({(1, name): TYPICAL[name] for name in READS[variant] if name not in ATMOS})
    for consts in cases:
        for cpt in (2, 1):
            pair(lambda: build_case(variant, n=300, T=1, bias=True), consts,
                 engine_kw={"options": {"specialize": specialize, "cells_per_thread": cpt}},
                 kind=1 if (variant == "CCLM" or not specialize) else 2,
                 label=f"{variant} spec={specialize} cpt={cpt} {consts}")


@pytest.mark.parametrize("n", [1, 3, 127, 129])
@pytest.mark.parametrize("variant,name", [("CCLM", "AMOI"), ("MOM5", "FICE"), ("RCO", "TATM")])
def test_partial_vectors_and_tiles(variant, name, n):
    s = 0 if name in ATMOS else 1
    for cpt in (2, 1):
        pair(lambda: build_case(variant, n=n, T=1, bias=True), {(s, name): TYPICAL[name]},
             engine_kw={"options": {"cells_per_thread": cpt}}, kind=1 if variant == "CCLM" else 2,
             label=f"{variant} {name} n={n} cpt={cpt}")


@pytest.mark.parametrize("specialize", [1, 0])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_separate_uv_grids(variant, specialize):
    """u and v grids of their own (310, 290): the generic kernel, whose uv_grid pass takes its
    own uniform values (kind 1 for every variant)."""
    uv = [x for x in ("TSUR", "FICE", "PSUR", "UATM", "VATM", "AMOM", "CMOM") if x in READS[variant]]
    cases = [{(0 if name in ATMOS else 1, name): TYPICAL[name]} for name in uv]
    cases.append({(0, "UATM"): 0.0, (0, "VATM"): 0.0})
    for consts in cases:
        pair(lambda: build_case(variant, n=300, T=1, bias=True, sep_grids=(310, 290)), consts,
             engine_kw={"options": {"specialize": specialize}}, label=f"{variant} sep spec={specialize} {consts}")


# ---------------------------------------------------------------- T = 2, the Baltic shape
def atmos_of(case, n, s0, fields=ATM_FIELDS, dtype=np.float64):
    la = BlockedRandomAtmosMap().local(0, n, 0, 1, n, ranges=[(0, n)])
    outs = {name: np.full(max(la.n_atmos, 1), np.nan, dtype=dtype) for name, _ in fields}
    kw = {"atmos": {"local": la, "fields": [(PHASE_NORMAL, s0, g, name, outs[name]) for name, g in fields]}}
    return kw, {("atm", name): a for name, a in outs.items()}


def test_baltic_shape_t2():
    """MOM5 water + ice, ice FICE = 1.0 constant, bias, register averages, the fused accumulation
    on a random map (runs of 3-5 cells) at n = 4100: one layout tile and a partial wave tile."""
    n = 4100
    (got, _), (_, case) = pair(lambda: build_case("MOM5", n=n, T=2, bias=True), {(2, "FICE"): 1.0},
                               extra=lambda c: atmos_of(c, n, 0), label="Baltic T=2", kind=2)
    # (the twin's case: its host arrays still hold the inputs)
    ref = oracle_lib.run_case(case, "c", current_step_time=T_STEP)
    assert_tight(case, {k: got[k] for k in case.outputs}, ref, T_STEP, "constant FICE, T=2", report=False)


# ---------------------------------------------------------------- T = 3, held inputs
@pytest.mark.parametrize("averages", [True, False])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5"])
def test_three_types_mixed_constants_and_arrays(variant, averages):
    """FICE: type 1 an array, type 2 the constant 1.0, type 3 the constant 0.5.  PSUR: one
    constant aliased into every type.  TATM: an array in types 1 and 3, a constant in type 2.
    Without the type-0 averages the CCLM launch is the multi-type kernel that takes uniforms
    (kind 1: the held-input logic tells arrays from constants and constants from each other);
    with them, and for MOM5, the launch streams the filled arrays (kind 2)."""
    n = 4100

    def make():
        case = build_case(variant, n=n, T=3, bias=True)
        lf = case.lf
        own = np.full(n, TYPICAL["TATM"])
        for g in (1, 2, 3):
            lf.set_array("TATM", 2, g, own, allocated=(g == 1))
        if not averages:
            case.averages = []
            case.outputs = [k for k in case.outputs if k[0] != 0]
        return case

    pair(make, {(2, "FICE"): 1.0, (3, "FICE"): 0.5, (0, "PSUR"): TYPICAL["PSUR"], (2, "TATM"): TYPICAL["TATM"]},
         extra=(lambda c: atmos_of(c, n, 0)) if averages else None, label=f"{variant} T=3 averages={averages}",
         kind=1 if (variant == "CCLM" and not averages) else 2)


# ---------------------------------------------------------------- group launch
def test_group_launch_with_a_different_constant_per_member():
    torch = pytest.importorskip("torch")
    stream = torch.cuda.current_stream(torch.device("cuda", 0))  # one stream: the members merge
    n = 12_345
    consts = {"CCLM": {(0, "AMOI"): TYPICAL["AMOI"]}, "MOM5": {(1, "FICE"): 0.0}, "RCO": {(0, "VATM"): 0.0}}
    res = []
    for use in (True, False):
        cases, engines, arrays = [], [], {}
        try:
            for v in ("CCLM", "MOM5", "RCO"):
                c = build_case(v, n=n, T=1, bias=True)
                declare(c, consts[v])
                kw, outs = atmos_of(c, n, 1)
                e = Engine(c.lf, 1, c.methods, corrections=c.corrections, use_constants=use, stream=stream.cuda_stream,
                           options={"atmos_in_run": 0, "host_staging": 0, "atm_records": 1}, **kw)
                if use:
                    poison(e)
                e.upload(PHASE_ALL)
                cases.append(c)
                engines.append(e)
                arrays.update({(v,) + k: a for k, a in outs.items()})
            run_group(engines, PHASE_ALL, T_STEP)
            assert [e.last_group_size() for e in engines] == [3, 3, 3]
            if use:  # CCLM takes the uniform, the MOM5 and RCO members their filled arrays
                assert [e.constant_info(*next(iter(e.constants))) for e in engines] == [1, 2, 2]
            for e in engines:
                e.run_atmos(PHASE_ALL)  # (a no-op: the accumulation rode in the launch)
                e.download(PHASE_ALL)
                e.synchronize()
            torch.cuda.synchronize()
            got = {k: np.array(a, copy=True) for k, a in arrays.items()}
            for v, c in zip(("CCLM", "MOM5", "RCO"), cases):
                got.update({(v,) + k: np.array(c.lf.field[k], copy=True) for k in c.outputs})
            res.append(got)
        finally:
            for e in engines:
                e.close()
    same(res[0], res[1], "group of three")


# ---------------------------------------------------------------- fp32
@pytest.mark.parametrize("n", [1000, 1027])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5"])
def test_fp32_engine_rounds_the_value_once(variant, n):
    """0.3 and 101325.7 are not floats: the constant is what a bound float array holds."""
    consts = {(1, "FICE"): 0.3, (0, "PSUR"): 101325.7}
    res = []
    for use in (True, False):
        case = as_dtype(build_case(variant, n=n, T=1, bias=True), "float32")
        declare(case, consts)
        assert case.lf.field[(1, 1, "FICE")].dtype == np.float32
        kw, arrays = atmos_of(case, n, 1, dtype=np.float32)
        eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, use_constants=use, **kw)
        try:
            if use:
                assert set(k[2] for k in eng.constants) == {"FICE", "PSUR"}
                poison(eng)
            eng.step(PHASE_ALL, T_STEP)
            if use:  # the fp32 kernels take no uniforms: the filled float array
                assert all(eng.constant_info(*k) == 2 for k in eng.constants)
            res.append(snapshot(case, arrays))
        finally:
            eng.close()
    same(res[0], res[1], f"fp32 {variant} n={n}")


# ---------------------------------------------------------------- transports
def _upload_field_step(eng):
    lf = eng.lf
    done = set()
    for (s, g, name), a in lf.field.items():
        if id(a) in done or not (name in TYPICAL or name == "FARE"):
            continue
        done.add(id(a))
        eng.upload_field(s, g, name)  # (a constant slot: a no-op success)
    eng.step(PHASE_ALL, T_STEP)


def _async_step(eng):
    eng.step_async(PHASE_ALL, T_STEP)
    eng.synchronize()


BALTIC = {(2, "FICE"): 1.0, (0, "PSUR"): TYPICAL["PSUR"]}  # T = 2, register averages: filled arrays
CALM = {(1, "FICE"): 0.0, (0, "PSUR"): TYPICAL["PSUR"]}    # CCLM, T = 1: wave-uniform values


@pytest.mark.parametrize("how", ["step", "step_async", "upload_field"])
def test_caller_heap_arrays(how):
    run = {"step": step_once, "step_async": _async_step, "upload_field": _upload_field_step}[how]
    pair(lambda: build_case("MOM5", n=5003, T=2, bias=True), BALTIC, run=run, label=f"heap {how}", kind=2)
    pair(lambda: build_case("CCLM", n=5003, T=1, bias=True), CALM, run=run, label=f"heap {how} CCLM")


@pytest.mark.parametrize("zero_copy", [1, 0])
def test_library_memory(zero_copy):
    """fcx_host_malloc arrays used in place (zero-copy) and moved as spans (zero-copy off)."""
    with host_alloc.Arena() as arena:
        def make():
            case = build_case("MOM5", n=5003, T=2, bias=True)
            arena.adopt(case.lf)
            return case

        def check(eng, case):
            if zero_copy:
                assert eng.zero_copy_active()

        pair(make, BALTIC, engine_kw={"options": {"zero_copy": zero_copy}}, check=check,
             label=f"library memory zero_copy={zero_copy}", kind=2)

        def make1():
            case = build_case("CCLM", n=5003, T=1, bias=True)
            arena.adopt(case.lf)
            return case

        pair(make1, CALM, engine_kw={"options": {"zero_copy": zero_copy}}, check=check,
             label=f"library memory zero_copy={zero_copy} CCLM")


def test_pipelined_step():
    """n = 600,000: the host-bound step takes the chunk pipeline; the constant has no chunk copies."""
    pair(lambda: build_case("CCLM", n=600_000, T=1, bias=True), {(1, "FICE"): 0.0}, label="pipelined")


def test_unbound_slot_plus_constant():
    """Raw ABI: the slot never sees an array."""
    n = 777
    res = []
    for use in (True, False):
        case = build_case("MOM5", n=n, T=2, bias=True)
        if use:
            for g in (1, 2, 3):
                case.lf.field.pop((2, g, "FICE"))
        else:
            assert np.all(case.lf.field[(2, 1, "FICE")] == 1.0)
        eng = Engine(case.lf, 2, case.methods, corrections=case.corrections, averages=case.averages, commit=False)
        try:
            if use:
                for g in (1, 2, 3):
                    eng.bind_constant(2, g, "FICE", 1.0)
            eng.commit()
            if use:
                assert eng.constant_info(2, 1, "FICE") == 2 and eng.constant_info(1, 1, "FICE") == 0
            eng.step(PHASE_ALL, T_STEP)
            res.append(snapshot(case))
        finally:
            eng.close()
    same(res[0], res[1], "unbound + constant")


# ---------------------------------------------------------------- consumers outside the flux pass
def read_device(eng, s, g, name, n, dtype=np.float64):
    """The engine's device array of a slot, cell order (fcx_device_ptr + fcx_device_layout)."""
    tile, stride = eng.device_layout()
    p = eng.device_ptr(s, g, name)
    assert p
    elems = ((n - 1) // tile) * stride + (n - 1) % tile + 1
    raw = np.empty(elems, dtype=dtype)
    _lib.check(eng.lib.fcx_memcpy(ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(p), raw.nbytes, 2))
    j = np.arange(n)
    return raw[(j // tile) * stride + j % tile]


@pytest.mark.parametrize("n", [300, 4100])
def test_device_array_holds_the_value(n):
    """fcx_device_ptr of a constant slot: kind 2, the value in every cell, tiled or plain."""
    for tiled in (1, 0):
        case = build_case("MOM5", n=n, T=2, bias=True)
        declare(case, BALTIC)
        eng = Engine(case.lf, 2, case.methods, corrections=case.corrections, averages=case.averages,
                     options={"tiled_layout": tiled})
        try:
            poison(eng)
            eng.step(PHASE_ALL, T_STEP)
            assert eng.constant_info(2, 1, "FICE") == 2 and eng.constant_info(1, 1, "PSUR") == 2
            assert eng.constant_info(1, 1, "FICE") == 0
            assert np.all(read_device(eng, 2, 1, "FICE", n) == 1.0)
            assert np.all(read_device(eng, 1, 1, "PSUR", n) == TYPICAL["PSUR"])
            assert eng.device_ptr(1, 1, "PSUR") == eng.device_ptr(0, 1, "PSUR")
            assert eng.constant_info(2, 1, "FICE") == 2 and eng.constant_info(0, 1, "PSUR") == 2
            eng.step(PHASE_ALL, T_STEP)  # (and the step still runs on the values)
        finally:
            eng.close()
    # read by the flux pass only, as a uniform: no device array until one is asked for
    case = build_case("CCLM", n=n, T=1, bias=True)
    declare(case, CALM)
    eng = Engine(case.lf, 1, case.methods, corrections=case.corrections)
    try:
        poison(eng)
        eng.step(PHASE_ALL, T_STEP)
        assert eng.constant_info(1, 1, "FICE") == 1 and eng.constant_info(0, 1, "PSUR") == 1
        assert np.all(read_device(eng, 1, 1, "FICE", n) == 0.0)
        assert eng.constant_info(1, 1, "FICE") == 2 and eng.constant_info(0, 1, "PSUR") == 1
        eng.step(PHASE_ALL, T_STEP)  # (the step still runs on the value)
        assert np.all(np.isfinite(case.lf.field[(1, 1, "HSEN")]))
    finally:
        eng.close()
    c32 = as_dtype(build_case("MOM5", n=n, T=1), "float32")
    declare(c32, {(1, "FICE"): 0.3})
    eng = Engine(c32.lf, 1, c32.methods)
    try:
        assert np.all(read_device(eng, 1, 1, "FICE", n, np.float32) == np.float32(0.3))
    finally:
        eng.close()


def test_constant_as_regrid_source():
    """TSUR(1) on the t grid constant and put to the u and v grids (do_regridding)."""
    nt, nu, nv = 300, 310, 290

    def make():
        case = build_case("MOM5", n=nt, T=1, bias=True, sep_grids=(nu, nv))
        case.lf.put_to[(1, 1, "TSUR")] = 2 | 4
        case.outputs += [(1, 2, "TSUR"), (1, 3, "TSUR")]  # the destinations: ordinary arrays
        case.lf.set_constant("TSUR", 1, 1, TYPICAL["TSUR"])
        return case

    def run(eng):
        eng.do_regridding("TSUR", 1)
        eng.step(PHASE_ALL, T_STEP)

    regrid = namelists.regrid_matrices((nt, nu, nv))  # interpolations: TSUR stays a temperature
    pair(make, {}, run=run, engine_kw={"regrid": regrid}, label="regrid source", kind=2)


def test_constant_fare_in_averages():
    """FARE of both types constant: the register averages of the fused step and an explicit
    fcx_average_across_surface_types read the filled arrays."""
    def run(eng):
        eng.step(PHASE_ALL, T_STEP)
        for g, name in ((1, "HLAT"), (1, "TSUR"), (2, "UMOM")):
            _lib.check(eng.lib.fcx_average_across_surface_types(eng.h, g, IDX[name]))

    pair(lambda: build_case("CCLM", n=4100, T=2, bias=True), {(1, "FARE"): 0.25, (2, "FARE"): 0.75}, run=run,
         label="constant FARE", kind=2)


def test_constant_tsur_accumulated_and_remapped():
    n = 3001
    mmap = synthetic_model_map(n, 400, links_per_cell=2)

    def extra(case):
        kw, arrays = atmos_of(case, n, 1, fields=(("TSUR", 1), ("HSEN", 1)))
        outs = {k: np.full(mmap.n_model, np.nan) for k in ("TSUR", "MEVA")}
        kw["remaps"] = [{"n_dst": mmap.n_model, "src": mmap.src, "dst": mmap.dst, "w": mmap.weight,
                         "fields": [(PHASE_NORMAL, 1, 1, name, outs[name]) for name in outs]}]
        arrays.update({("remap", k): a for k, a in outs.items()})
        return kw, arrays

    (got, case), _ = pair(lambda: build_case("RCO", n=n, T=1, bias=True), {(1, "TSUR"): TYPICAL["TSUR"]},
                          extra=extra, label="TSUR accumulated and remapped", kind=2)
    want = oracle_lib.remap_apply(mmap.src, mmap.dst, mmap.weight, np.full(n, TYPICAL["TSUR"]), mmap.n_model)
    np.testing.assert_array_equal(got[("remap", "TSUR")], want)


def test_per_call_subroutines_with_a_constant():
    """The reference's call sequence, one subroutine at a time (each uploads what it reads)."""
    def make():
        return build_case("MOM5", n=1500, T=2, bias=True)

    averages = make().averages

    def run(eng):
        lib, h = eng.lib, eng.h
        _lib.check(lib.fcx_calc_flux_radiation_blackbody(h))
        for g in (1, 2, 3):
            _lib.check(lib.fcx_calc_spec_vapor_surface(h, g))
        _lib.check(lib.fcx_calc_flux_mass_evap(h, T_STEP))
        _lib.check(lib.fcx_calc_flux_heat_latent(h))
        _lib.check(lib.fcx_calc_flux_heat_sensible(h))
        _lib.check(lib.fcx_calc_flux_momentum_east(h, 2))
        _lib.check(lib.fcx_calc_flux_momentum_north(h, 3))
        for _, g, name in averages:
            _lib.check(lib.fcx_average_across_surface_types(h, g, IDX[name]))

    # (the per-call launches are the MOM5 kernels without register averages: filled arrays)
    pair(make, BALTIC, run=run, label="per-call", kind=2)


# ---------------------------------------------------------------- bytes
def test_bytes_of_a_constant():
    """A kernel-uniform constant is not streamed: fcx_algorithmic_bytes falls by 8 n per distinct
    uniform stream (FICE and PSUR of a CCLM step: two).  It has no place among the in-place
    host bytes and needs no staging image.  The fp32 kernels take no uniforms (DESIGN.md
    section 3: they spilled), so there the filled float array is streamed and the bytes are the
    twin's, not 4 n fewer; likewise the T = 2 register-average launch."""
    n = 5003
    with host_alloc.Arena() as arena:
        vals = {}
        for use in (True, False):
            for lib_mem in (True, False):
                case = build_case("CCLM", n=n, T=1, bias=True)
                declare(case, CALM)
                if lib_mem:
                    arena.adopt(case.lf)
                eng = Engine(case.lf, 1, case.methods, corrections=case.corrections,
                             use_constants=use, options={"zero_copy": 1 if lib_mem else 0})
                try:
                    eng.step(PHASE_ALL, T_STEP)
                    vals[(use, lib_mem)] = (eng.algorithmic_bytes(), eng.staging_bytes(), eng.zero_copy_bytes())
                finally:
                    eng.close()
    for lib_mem in (True, False):
        c, t = vals[(True, lib_mem)], vals[(False, lib_mem)]
        assert t[0] - c[0] == 2 * 8 * n, (c, t)
        assert c[1] <= t[1] and c[2] <= t[2], (c, t)
    # in place, the twin maps two arrays more (FICE, PSUR) than the constant engine
    assert vals[(False, True)][2] - vals[(True, True)][2] == 2 * 8 * n, vals
    t2 = []
    for use in (True, False):
        case = build_case("MOM5", n=n, T=2, bias=True)
        declare(case, BALTIC)
        eng = Engine(case.lf, 2, case.methods, corrections=case.corrections, averages=case.averages, use_constants=use)
        try:
            eng.step(PHASE_ALL, T_STEP)
            t2.append(eng.algorithmic_bytes())
        finally:
            eng.close()
    assert t2[0] == t2[1]
    b32 = []
    for use in (True, False):
        case = as_dtype(build_case("MOM5", n=n, T=1, bias=True), "float32")
        declare(case, {(1, "FICE"): 0.0})
        eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, use_constants=use)
        try:
            eng.step(PHASE_ALL, T_STEP)
            b32.append(eng.algorithmic_bytes())
        finally:
            eng.close()
    assert b32[0] == b32[1]


# ---------------------------------------------------------------- the time loop
def test_time_loop_with_the_namelist_constant():
    grids = (3001, 2999, 3011)
    regrid = namelists.regrid_matrices(grids)
    corr = (20000101, corrections(grids[0]))
    sent = []
    for use in (True, False):
        s = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=grids)
        assert s.local_field.constant == {(2, 1, "FICE"): 1.0}
        eng = s.engine(corrections=corr, regrid=regrid, use_constants=use)
        c = SyntheticCoupler.for_setup(s)
        try:
            assert (eng.constant_info(2, 1, "FICE") != 0) == use
            if use:
                poison(eng)
            driver.run(s, eng, c)
        finally:
            eng.close()
        sent.append(c.sent)
    assert sent[0].keys() == sent[1].keys() and sent[0]
    for k in sent[0]:
        assert np.all(np.isfinite(sent[0][k])), k
        assert bits_equal(sent[0][k], sent[1][k]).all(), k
