"""Namelist-constant input fields (val_bottom_var_* / val_atmos_var_*, flux_calculator.F90:
444-549) on the host, no GPU: the C ABI of fcx_bind_constant (arguments, state, aliases by
address, a constant standing in for a missing array, a written constant refused by the plan
check) and the Python set-up that records the constants."""
import ctypes

import numpy as np
import pytest

import namelists
from fcx import _lib
from fcx.basic import IDX
from fcx.engine import Engine
from fcx.setup import setup_from_namelist
from fcx.synthetic import build_case

E_ARG, E_STATE, E_MISSING = 1, 2, 5


def _status(fn, *args):
    r = fn(*args)
    return r, _lib.load().fcx_last_error().decode(errors="replace")


def _raw_engine(T=2, n=64):
    lib = _lib.load()
    h = ctypes.c_void_p()
    gs = (ctypes.c_int32 * 3)(n, n, n)
    _lib.check(lib.fcx_create(0, T, gs, ctypes.byref(h)))
    return lib, h


@pytest.mark.parametrize("s,g,var", [(-1, 1, "FICE"), (99, 1, "FICE"), (1, 0, "FICE"), (1, 4, "FICE"),
                                     (1, 1, 0), (1, 1, 1000)])
def test_bad_slot_is_an_argument_error(s, g, var):
    lib, h = _raw_engine()
    try:
        v = IDX[var] if isinstance(var, str) else var
        r, msg = _status(lib.fcx_bind_constant, h, s, g, v, 1.0)
        assert r == E_ARG and "out of range" in msg, (r, msg)
    finally:
        lib.fcx_destroy(h)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_value_is_an_argument_error(value):
    lib, h = _raw_engine()
    try:
        r, msg = _status(lib.fcx_bind_constant, h, 1, 1, IDX["FICE"], value)
        assert r == E_ARG and "finite" in msg and "FICE" in msg, (r, msg)
    finally:
        lib.fcx_destroy(h)


def test_null_engine_is_an_argument_error():
    lib = _lib.load()
    assert lib.fcx_bind_constant(None, 1, 1, IDX["FICE"], 1.0) == E_ARG
    k = ctypes.c_int32()
    assert lib.fcx_constant_info(None, 1, 1, IDX["FICE"], ctypes.byref(k)) == E_ARG


def test_constant_info_before_commit_is_a_state_error():
    lib, h = _raw_engine()
    try:
        _lib.check(lib.fcx_bind_constant(h, 1, 1, IDX["FICE"], 0.0))
        k = ctypes.c_int32()
        r, msg = _status(lib.fcx_constant_info, h, 1, 1, IDX["FICE"], ctypes.byref(k))
        assert r == E_STATE, (r, msg)
    finally:
        lib.fcx_destroy(h)


def _mom5_without_ice_fice():
    case = build_case("MOM5", n=64, T=2)
    for g in (1, 2, 3):
        case.lf.field.pop((2, g, "FICE"))
    return case


def test_a_constant_stands_in_for_a_missing_array():
    case = _mom5_without_ice_fice()
    e = Engine(case.lf, 2, case.methods, averages=case.averages, commit=False)
    try:
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_MISSING and "FICE" in str(ex.value), str(ex.value)
        for g in (1, 2, 3):
            e.bind_constant(2, g, "FICE", 1.0)
        e.plan_check()
    finally:
        e.close()


def test_a_written_constant_is_refused_by_name():
    """QSUR(1, t) is computed by the CCLM method: declared constant, every plan that stores it is
    refused with the slot's name; so is the target of a 'copy' method."""
    case = build_case("MOM5", n=64, T=2)
    assert case.methods["which_spec_vapor_surface_t"][0] == "CCLM"
    e = Engine(case.lf, 2, case.methods, averages=case.averages, commit=False)
    try:
        e.plan_check()
        e.bind_constant(1, 1, "QSUR", 0.01)
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE, str(ex.value)
        assert "constant field QSUR(1,t)" in str(ex.value) and "written" in str(ex.value), str(ex.value)
    finally:
        e.close()
    case = build_case("MOM5", n=64, T=2, sep_grids=(66, 62),
                      per_type={2: {"which_flux_radiation_blackbody": "copy"}})
    e = Engine(case.lf, 2, case.methods, averages=case.averages, commit=False)
    try:
        e.plan_check()
        # the copy target as a slot of its own (not the type-1 array, which the plan writes)
        _lib.check(e.lib.fcx_bind_field(e.h, 2, 1, IDX["RBBR"], None, 0, 0))
        e.bind_constant(2, 1, "RBBR", 300.0)
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE, str(ex.value)
        assert "constant field RBBR(2,t)" in str(ex.value) and "'copy'" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_commit_refuses_a_written_constant_before_any_gpu_contact():
    """fcx_commit runs the same check (validation, then the dry plans) before it touches the
    device, so the error needs no GPU."""
    case = build_case("MOM5", n=64, T=2)
    e = Engine(case.lf, 2, case.methods, averages=case.averages, commit=False)
    try:
        e.bind_constant(1, 1, "MEVA", 0.0)
        with pytest.raises(_lib.FcxError) as ex:
            e.commit()
        assert ex.value.status == E_STATE and "constant field MEVA(1,t)" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_a_constant_regrid_destination_and_average_output_are_refused():
    case = build_case("CCLM", n=64, T=2, sep_grids=(66, 62))
    case.lf.put_to[(1, 1, "TSUR")] = 2  # TSUR(1) t -> u: its u-grid array is a destination
    e = Engine(case.lf, 2, case.methods, averages=case.averages, commit=False)
    try:
        e.plan_check()
        e.bind_constant(1, 2, "TSUR", 280.0)
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE and "TSUR(1,u)" in str(ex.value) and "regridding destination" in str(ex.value)
    finally:
        e.close()
    case = build_case("CCLM", n=64, T=2)
    e = Engine(case.lf, 2, case.methods, averages=case.averages, commit=False)
    try:
        e.bind_constant(0, 1, "HLAT", 0.0)  # the type-0 output of an average
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE and "constant field HLAT(0,t)" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_aliases_follow_the_address():
    """One array bound to (0,g,PSUR), (1,g,PSUR) and (2,g,PSUR); (0,1,PSUR) declared constant: the
    slots of types 1 and 2 are that constant too, so the plan check passes with the array gone.
    The control: the same engine without the array ever bound to types 1 and 2 lacks PSUR."""
    case = build_case("MOM5", n=64, T=2)
    lf = case.lf
    assert lf.field[(0, 1, "PSUR")] is lf.field[(1, 1, "PSUR")] is lf.field[(2, 1, "PSUR")]
    # the same set-up with the array popped from types 1 and 2 fails, naming PSUR ...
    popped = build_case("MOM5", n=64, T=2)
    for s in (1, 2):
        for g in (1, 2, 3):
            popped.lf.field.pop((s, g, "PSUR"))
    e = Engine(popped.lf, 2, popped.methods, averages=popped.averages, commit=False)
    try:
        e.bind_constant(0, 1, "PSUR", 101325.0)
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_MISSING and "PSUR" in str(ex.value)
    finally:
        e.close()
    # ... and with raw calls: bind one address to the three slots, declare type 0 constant, free
    # the array: the plan check, which needs PSUR of types 1 and 2, still passes, and a later
    # bind of the same address is an ordinary array again (the constant let go of it)
    lib = _lib.load()
    e = Engine(popped.lf, 2, popped.methods, averages=popped.averages, commit=False)
    try:
        a = np.full(64, 101325.0)
        for s in (0, 1, 2):
            for g in (1, 2, 3):
                _lib.check(lib.fcx_bind_field(e.h, s, g, IDX["PSUR"], ctypes.c_void_p(a.ctypes.data), 64, 0))
        _lib.check(lib.fcx_bind_constant(e.h, 0, 1, IDX["PSUR"], 101325.0))
        del a
        e.plan_check()
    finally:
        e.close()


def test_set_constant_fills_the_array_and_marks_every_alias():
    case = build_case("MOM5", n=64, T=2)
    lf = case.lf
    lf.set_constant("FICE", 2, 1, 1.0)
    assert lf.constant == {(2, g, "FICE"): 1.0 for g in (1, 2, 3)}  # merged grids: one array
    assert np.all(lf.field[(2, 1, "FICE")] == 1.0)
    lf.set_constant("PSUR", 0, 1, 101325.0)
    assert {k for k in lf.constant if k[2] == "PSUR"} == {(s, g, "PSUR") for s in (0, 1, 2) for g in (1, 2, 3)}
    lf.alias("FICE", 1, 1, from_s=2)
    assert lf.constant[(1, 1, "FICE")] == 1.0
    lf.set_array("FICE", 1, 1, np.zeros(64))
    assert (1, 1, "FICE") not in lf.constant
    with pytest.raises(ValueError):
        lf.set_constant("FICE", 2, 1, float("nan"))
    e = Engine(lf, 2, case.methods, averages=case.averages, commit=False)
    assert e.constants[(2, 1, "FICE")] == 1.0 and e.constants[(0, 1, "PSUR")] == 101325.0
    e.plan_check()
    e.close()
    twin = Engine(lf, 2, case.methods, averages=case.averages, commit=False, use_constants=False)
    assert twin.constants == {}
    twin.close()
    lf.field[(2, 1, "FICE")][3] = 0.5  # a host that wrote the array has no constant any more
    with pytest.warns(RuntimeWarning, match="FICE"):
        e = Engine(lf, 2, case.methods, averages=case.averages, commit=False)
    assert not any(k[2] == "FICE" for k in e.constants) and (0, 1, "PSUR") in e.constants
    assert (2, 1, "FICE") in e.dropped_constants
    e.close()


def test_setup_records_the_constants():
    s = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=(301, 299, 311))
    assert s.local_field.constant == {(2, 1, "FICE"): 1.0}
    assert np.all(s.local_field.field[(2, 1, "FICE")] == 1.0)
    assert not any(f.var == "FICE" and f.surface_type == 2 for f in s.input_field)
    # PSUR as a constant instead of a received field.  A field nobody sends is not regridded
    # (prepare_regridding runs over the input fields only, flux_calculator.F90 STEP 1.5), so the
    # u and v grids, whose CCLM methods need PSUR too, get the same namelist value.
    patch = ("  val_atmos_var_t(2) = 101325.0\n  name_atmos_var_u = 'PSUR'\n  val_atmos_var_u(1) = 101325.0\n"
             "  name_atmos_var_v = 'PSUR'\n  val_atmos_var_v(1) = 101325.0\n")
    text = namelists.CCLM_REGRID.replace("  regrid_t_to_u(2,1,:)", patch + "  regrid_t_to_u(2,1,:)")
    assert "val_atmos_var_t(2)" in text
    s = setup_from_namelist(text, mype=1, grid_size=(301, 299, 311))
    assert s.local_field.constant == {(t, g, "PSUR"): 101325.0 for t in (0, 1) for g in (1, 2, 3)}
    assert s.local_field.field[(1, 1, "PSUR")] is s.local_field.field[(0, 1, "PSUR")]
    assert not any(f.var == "PSUR" for f in s.input_field)
    assert (1, 1, "PSUR") not in s.local_field.put_to
    e = s.engine(regrid=namelists.regrid_matrices((301, 299, 311)), commit=False)
    assert set(e.constants) == set(s.local_field.constant)
    e.plan_check()
    e.close()
