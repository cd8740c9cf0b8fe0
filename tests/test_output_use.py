"""What the host does with a computed output (fcx_set_output_use) on the host, no GPU: the C
ABI's argument and state errors, the plan check that names a declared slot which is unbound, a
constant or written by no plan, and the Python set-up that finds the outputs no output_field
entry sends (the reference builds output_field from its send_to_* / name_send_* tables only,
flux_calculator.F90:668-768, basic:170-284)."""
import ctypes

import pytest

import namelists
from fcx import _lib
from fcx.basic import IDX
from fcx.engine import Engine
from fcx.setup import setup_from_namelist
from fcx.synthetic import build_case

E_ARG, E_STATE = 1, 2
HOST, DEVICE, UNREAD = _lib.FCX_OUT_HOST, _lib.FCX_OUT_DEVICE, _lib.FCX_OUT_UNREAD
FLUXES = ("MEVA", "HLAT", "HSEN", "RBBR", "UMOM", "VMOM")


def _status(fn, *args):
    r = fn(*args)
    return r, _lib.load().fcx_last_error().decode(errors="replace")


def _raw_engine(T=2, n=64):
    lib = _lib.load()
    h = ctypes.c_void_p()
    gs = (ctypes.c_int32 * 3)(n, n, n)
    _lib.check(lib.fcx_create(0, T, gs, ctypes.byref(h)))
    return lib, h


@pytest.mark.parametrize("s,g,var", [(-1, 1, "QSUR"), (99, 1, "QSUR"), (1, 0, "QSUR"), (1, 4, "QSUR"),
                                     (1, 1, 0), (1, 1, 1000)])
def test_bad_slot_is_an_argument_error(s, g, var):
    lib, h = _raw_engine()
    try:
        v = IDX[var] if isinstance(var, str) else var
        r, msg = _status(lib.fcx_set_output_use, h, s, g, v, UNREAD)
        assert r == E_ARG and "out of range" in msg, (r, msg)
    finally:
        lib.fcx_destroy(h)


@pytest.mark.parametrize("use", [-1, 3, 100])
def test_a_use_outside_the_enum_is_an_argument_error(use):
    lib, h = _raw_engine()
    try:
        r, msg = _status(lib.fcx_set_output_use, h, 1, 1, IDX["QSUR"], use)
        assert r == E_ARG and "QSUR(1,t)" in msg and "0..2" in msg, (r, msg)
        for ok in (HOST, DEVICE, UNREAD):
            assert lib.fcx_set_output_use(h, 1, 1, IDX["QSUR"], ok) == 0
    finally:
        lib.fcx_destroy(h)


def test_null_engine_and_info_before_commit():
    lib, h = _raw_engine()
    try:
        k = ctypes.c_int32()
        assert lib.fcx_set_output_use(None, 1, 1, IDX["QSUR"], UNREAD) == E_ARG
        assert lib.fcx_output_info(None, 1, 1, IDX["QSUR"], ctypes.byref(k)) == E_ARG
        assert lib.fcx_output_info(h, 1, 1, IDX["QSUR"], None) == E_ARG
        r, msg = _status(lib.fcx_output_info, h, 1, 1, IDX["QSUR"], ctypes.byref(k))
        assert r == E_STATE and "fcx_commit" in msg, (r, msg)
    finally:
        lib.fcx_destroy(h)


def test_the_plan_check_accepts_qsur_and_a_per_type_flux():
    case = build_case("MOM5", n=64, T=2, bias=True)
    e = Engine(case.lf, 2, case.methods, averages=case.averages, commit=False,
               output_use={(1, 1, "QSUR"): UNREAD, (2, 1, "HSEN"): "unread", (1, 1, "MEVA"): "device"})
    try:
        assert e.output_use == {(1, 1, "QSUR"): UNREAD, (2, 1, "HSEN"): UNREAD, (1, 1, "MEVA"): DEVICE}
        e.plan_check()
        e.set_output_use(2, 1, "HSEN", HOST)  # a declaration can be taken back before the commit
        e.plan_check()
    finally:
        e.close()


def test_the_plan_check_names_an_unbound_slot():
    case = build_case("CCLM", n=64, T=1)
    e = Engine(case.lf, 1, case.methods, commit=False)
    try:
        assert (2, 1, "HLAT") not in case.lf.field
        e.set_output_use(2, 1, "HLAT", UNREAD)  # accepted: the slot may still be bound
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE and "HLAT(2,t)" in str(ex.value) and "not bound" in str(ex.value)
        with pytest.raises(_lib.FcxError) as ex:  # fcx_commit runs the same check before any GPU contact
            e.commit()
        assert ex.value.status == E_STATE and "HLAT(2,t)" in str(ex.value)
    finally:
        e.close()


def test_the_plan_check_names_a_slot_no_plan_writes():
    """TSUR is an input; RBBR of a type whose method is 'none' is computed by nothing."""
    case = build_case("CCLM", n=64, T=1)
    e = Engine(case.lf, 1, case.methods, commit=False)
    try:
        e.set_output_use(1, 1, "TSUR", DEVICE)
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE and "TSUR(1,t)" in str(ex.value) and "no plan writes" in str(ex.value)
        with pytest.raises(_lib.FcxError) as ex:
            e.commit()
        assert ex.value.status == E_STATE and "TSUR(1,t)" in str(ex.value)
    finally:
        e.close()
    case = build_case("CCLM", n=64, T=1)
    methods = dict(case.methods, which_flux_radiation_blackbody=["none"])
    e = Engine(case.lf, 1, methods, commit=False, output_use={(1, 1, "RBBR"): UNREAD})
    try:
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE and "RBBR(1,t)" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_the_plan_check_names_a_declared_constant():
    case = build_case("MOM5", n=64, T=2)
    case.lf.set_constant("FICE", 2, 1, 1.0)
    e = Engine(case.lf, 2, case.methods, averages=case.averages, commit=False)
    try:
        assert (2, 1, "FICE") in e.constants
        e.set_output_use(2, 1, "FICE", UNREAD)
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE and "constant field FICE(2,t)" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_unsent_outputs_of_the_baltic_set_up():
    s = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=(301, 299, 311))
    unsent = s.unsent_outputs()
    assert set(unsent) <= set(s.computed_slots())
    # QSUR is an intermediate: on t for water and ice, on u and v for the type that computes it
    for slot in ((1, 1, "QSUR"), (2, 1, "QSUR"), (1, 2, "QSUR"), (1, 3, "QSUR")):
        assert slot in unsent, (slot, unsent)
    lf = s.local_field
    sent = {id(lf.field[f.slot]) for f in s.output_field}
    for slot in s.computed_slots():
        if slot[2] in FLUXES and id(lf.field[slot]) in sent:
            assert slot not in unsent, slot
    for f in s.output_field:  # per-type MEVA / HLAT / HSEN go to the bottom model, momentum is uniform
        assert f.slot not in unsent, f
    assert not any(slot[2] in ("MEVA", "HLAT", "HSEN", "UMOM", "VMOM") for slot in unsent), unsent
    e = s.engine(regrid=namelists.regrid_matrices((301, 299, 311)), commit=False, select_outputs=True)
    try:
        assert e.output_use == {slot: UNREAD for slot in unsent}
        e.plan_check()
    finally:
        e.close()
    e = s.engine(regrid=namelists.regrid_matrices((301, 299, 311)), commit=False)
    assert e.output_use == {}  # the default declares nothing
    e.close()


def test_unsent_outputs_of_the_regrid_set_up_leave_the_regrid_sources_out():
    s = setup_from_namelist(namelists.CCLM_REGRID, mype=1, grid_size=(301, 299, 311))
    unsent = s.unsent_outputs()
    for g in (1, 2, 3):
        assert (1, g, "QSUR") in unsent, unsent
    # UMOM(u) and VMOM(v) are regridded to the t grid, whose arrays are what is sent
    assert s.local_field.put_to.get((1, 2, "UMOM")) and s.local_field.put_to.get((1, 3, "VMOM"))
    assert (1, 2, "UMOM") not in unsent and (1, 3, "VMOM") not in unsent
    assert not any(slot[2] in FLUXES for slot in unsent), unsent
    e = s.engine(regrid=namelists.regrid_matrices((301, 299, 311)), commit=False, select_outputs=True)
    try:
        e.plan_check()
    finally:
        e.close()
