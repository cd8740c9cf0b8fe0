"""Field ranges and the non-finite guard on the host, no GPU: the four entry points validate their
arguments, FCX_OPT_CHECK_FINITE (23) takes 0..3, fcx_check_fields pins after fcx_plan_check which
buffers a checked phase covers, and the Python driver makes no range call without a log."""
import ctypes

import numpy as np
import pytest

import namelists
import received
from fcx import _lib, driver
from fcx.basic import IDX, PHASE_ALL, PHASE_EARLY, PHASE_NORMAL
from fcx.engine import Engine
from fcx.setup import setup_from_namelist
from fcx.synthetic import SyntheticCoupler, build_case

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


def _slots(*triples):
    return np.array(triples, dtype=np.int32).reshape(-1)


def test_status_and_option_constants():
    assert _lib.FCX_E_NONFINITE == 7 and _lib.FCX_OPT_CHECK_FINITE == 23
    assert Engine.OPTIONS["check_finite"] == 23
    assert ctypes.sizeof(_lib.FieldRangeC) == 40  # 40 B per field through the page-locked buffer


def test_field_ranges_validates_its_arguments():
    lib, h = _raw_engine()
    try:
        out = (_lib.FieldRangeC * 2)()
        ok = _slots((1, 1, IDX["TSUR"]))
        assert lib.fcx_field_ranges(None, 1, ok.ctypes.data, out) == E_ARG
        assert lib.fcx_field_ranges(h, 1, None, out) == E_ARG
        assert lib.fcx_field_ranges(h, 1, ok.ctypes.data, None) == E_ARG
        assert lib.fcx_field_ranges(h, -1, ok.ctypes.data, out) == E_ARG
        for bad in ((-1, 1, 11), (11, 1, 11), (1, 0, 11), (1, 4, 11), (1, 1, 0), (1, 1, 36)):
            s = _slots((1, 1, 11), bad)
            assert lib.fcx_field_ranges(h, 2, s.ctypes.data, out) == E_ARG, bad
            assert "slot 1" in _err() and "out of range" in _err(), _err()
        assert lib.fcx_field_ranges(h, 1, ok.ctypes.data, out) == E_STATE  # not committed
        assert "fcx_commit" in _err()
    finally:
        lib.fcx_destroy(h)


def test_atmos_ranges_check_fields_and_check_result_validate_their_arguments():
    lib, h = _raw_engine()
    try:
        out = (_lib.FieldRangeC * 4)()
        n = ctypes.c_int32()
        assert lib.fcx_atmos_ranges(None, 3, 4, out, ctypes.byref(n)) == E_ARG
        assert lib.fcx_atmos_ranges(h, 3, 4, out, None) == E_ARG
        assert lib.fcx_atmos_ranges(h, 3, 4, None, ctypes.byref(n)) == E_ARG
        assert lib.fcx_atmos_ranges(h, 3, -1, out, ctypes.byref(n)) == E_ARG
        for phase in (0, 4):
            assert lib.fcx_atmos_ranges(h, phase, 4, out, ctypes.byref(n)) == E_ARG
        assert lib.fcx_atmos_ranges(h, 3, 4, out, ctypes.byref(n)) == E_STATE
        slots = np.zeros(30, np.int32)
        assert lib.fcx_check_fields(None, 3, 10, slots.ctypes.data, ctypes.byref(n)) == E_ARG
        assert lib.fcx_check_fields(h, 3, 10, slots.ctypes.data, None) == E_ARG
        assert lib.fcx_check_fields(h, 3, 10, None, ctypes.byref(n)) == E_ARG
        assert lib.fcx_check_fields(h, 0, 10, slots.ctypes.data, ctypes.byref(n)) == E_ARG
        assert lib.fcx_check_fields(h, 3, 10, slots.ctypes.data, ctypes.byref(n)) == E_STATE  # no plan check yet
        assert "fcx_plan_check" in _err()
        cell = ctypes.c_int64(5)
        assert lib.fcx_check_result(None, None, None, None, None, ctypes.byref(cell), None) == E_ARG
        assert lib.fcx_check_result(h, None, None, None, None, ctypes.byref(cell), None) == 0
        assert cell.value == -1  # nothing has been checked
    finally:
        lib.fcx_destroy(h)


def test_option_23_takes_0_to_3_and_option_20_stays_unknown():
    lib, h = _raw_engine()
    try:
        for v in (0, 1, 2, 3):
            assert lib.fcx_set_option(h, 23, v) == 0
        for v in (4, -1):
            assert lib.fcx_set_option(h, 23, v) == E_ARG
        assert lib.fcx_set_option(h, 20, 1) == E_ARG and "unknown" in _err()
    finally:
        lib.fcx_destroy(h)


def test_environment_sets_the_default(monkeypatch):
    case = build_case("CCLM", n=64, T=1)
    monkeypatch.setenv("FCX_CHECK_FINITE", "1")
    e = Engine(case.lf, 1, case.methods, commit=False)
    try:
        e.plan_check()
        got = e.check_fields(PHASE_ALL)
        assert got and (1, 1, "TSUR") not in got and (1, 1, "MEVA") in got  # outputs only
    finally:
        e.close()
    monkeypatch.setenv("FCX_CHECK_FINITE", "7")  # not a value: the default stays off
    e = Engine(case.lf, 1, case.methods, commit=False)
    try:
        e.plan_check()
        assert e.check_fields(PHASE_ALL) == []
    finally:
        e.close()


def _first_slots(lf, slots):
    """the slots' buffers, each under its first slot in (surface type, grid, variable) order"""
    by_array = {}
    for (s, g, name), a in lf.field.items():
        key = (s, g, IDX[name])
        if id(a) not in by_array or key < by_array[id(a)][0]:
            by_array[id(a)] = (key, (s, g, name))
    return sorted({by_array[id(lf.field[slot])] for slot in slots})


@pytest.mark.parametrize("which, mype", [("MOM5_BALTIC", 0), ("CCLM_REGRID", 1)])
def test_check_fields_on_the_namelist_set_ups(which, mype):
    """Bit 0 lists exactly the buffers the step stores (the calculations' outputs, regrid
    destinations, averaged type-0 fields), each once, in slot order; bit 1 puts the inputs first;
    a cap too small is an argument error that still reports the count."""
    setup = setup_from_namelist(getattr(namelists, which), mype=mype, grid_size=GRIDS)
    lf = setup.local_field
    e = setup.engine(regrid=namelists.regrid_matrices(GRIDS), commit=False, check_finite=1)
    try:
        with pytest.raises(_lib.FcxError) as ex:
            e.check_fields(PHASE_ALL)
        assert ex.value.status == E_STATE
        e.plan_check()
        outs = e.check_fields(PHASE_ALL)
        want = [slot for _, slot in _first_slots(lf, setup.computed_slots())]
        assert outs == want, (set(outs) ^ set(want))
        early, normal = e.check_fields(PHASE_EARLY), e.check_fields(PHASE_NORMAL)
        assert set(early) | set(normal) == set(outs) and any(v == "RBBR" for _, _, v in early)
        assert not any(v == "RBBR" for _, _, v in normal)
        e.set_option("check_finite", 3)
        both = e.check_fields(PHASE_ALL)
        ins = both[: len(both) - len(outs)]
        assert both[len(ins):] == outs and ins and not set(ins) & set(outs)
        assert ins == [slot for _, slot in _first_slots(lf, ins)]  # each buffer once, in slot order
        # a received field some flux reads is an input (ALBE, which no calculation reads, is not)
        read = [f for f in setup.input_field if f.var in ("TATM", "QATM", "PSUR", "TSUR", "UATM")]
        assert read
        for f in read:
            assert _first_slots(lf, [f.slot])[0][1] in ins, f.name
        assert not any(v == "ALBE" for _, _, v in ins)
        e.set_option("check_finite", 2)
        assert e.check_fields(PHASE_ALL) == ins
        n = ctypes.c_int32()
        small = np.zeros(3, np.int32)
        assert e.lib.fcx_check_fields(e.h, PHASE_ALL, 1, small.ctypes.data, ctypes.byref(n)) == E_ARG
        assert n.value == len(ins) and "cap" in _err()
        e.set_option("check_finite", 0)
        assert e.check_fields(PHASE_ALL) == []
    finally:
        e.close()


def test_dropped_stores_constants_and_received_fields():
    """An FCX_OUT_UNREAD QSUR whose store the whole-phase plan drops is absent from the outputs, an
    FCX_OUT_DEVICE one is present; a wave-uniform constant is absent from the inputs, a received
    field's slot is present."""
    n = 64

    def engine(use, **kw):
        case = build_case("CCLM", n=n, T=1)
        return case, Engine(case.lf, 1, case.methods, commit=False, options={"check_finite": 3},
                            output_use={(1, 1, "QSUR"): use}, **kw)

    case, e = engine("unread")
    try:
        e.plan_check()
        got = e.check_fields(PHASE_NORMAL)
        assert (1, 1, "QSUR") not in got and (1, 1, "MEVA") in got and (0, 1, "TATM") in got
    finally:
        e.close()
    case, e = engine("device")
    try:
        e.plan_check()
        assert (1, 1, "QSUR") in e.check_fields(PHASE_NORMAL)
    finally:
        e.close()
    # TATM as a namelist constant of the fp64 CCLM launch: a wave-uniform value, nothing to read
    case = build_case("CCLM", n=n, T=1)
    case.lf.set_constant("TATM", 1, 1, 280.0)
    e = Engine(case.lf, 1, case.methods, commit=False, options={"check_finite": 3})
    try:
        assert (1, 1, "TATM") in e.constants
        e.plan_check()
        got = e.check_fields(PHASE_NORMAL)
        assert not any(v == "TATM" for _, _, v in got) and (0, 1, "QATM") in got
    finally:
        e.close()
    # ... and received on the model's grid: its exchange-grid array is what the phase reads
    case = build_case("CCLM", n=n, T=1)
    e = Engine(case.lf, 1, case.methods, commit=False, options={"check_finite": 3})
    try:
        n_src, src, dst, w = received.links("unit", n)
        mid = e.add_receive_map(1, n_src, src, dst, w)
        source = np.zeros(n_src)
        e.bind_received(mid, PHASE_NORMAL, 1, 1, "TATM", source)
        e.plan_check()
        assert (0, 1, "TATM") in e.check_fields(PHASE_NORMAL)  # (the buffer's first slot: type 0)
    finally:
        e.close()


class _StubEngine:
    """Counts what the driver asks of an engine."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append(name)
            return []
        return call


def test_the_driver_without_a_log_makes_no_range_call():
    text = namelists.CCLM_REGRID  # verbosity_level = 2 (DEBUG)
    setup = setup_from_namelist(text, mype=1, grid_size=GRIDS)
    assert setup.nml["verbosity_level"] == 2
    stub = _StubEngine()
    driver.run(setup, stub, SyntheticCoupler.for_setup(setup), num_timesteps=1)
    assert "step" in stub.calls and "field_ranges" not in stub.calls
    lines = []
    stub = _StubEngine()
    stub.field_ranges = lambda slots: [type("R", (), {"min": 0.0, "max": 1.0})() for _ in slots]
    driver.run(setup, stub, SyntheticCoupler.for_setup(setup), num_timesteps=1, log=lines.append)
    assert len(lines) == len(setup.input_field) + len(setup.output_field)
    # at STANDARD a log changes nothing
    quiet = setup_from_namelist(text.replace("verbosity_level = 2", "verbosity_level = 1"), mype=1, grid_size=GRIDS)
    stub = _StubEngine()
    driver.run(quiet, stub, SyntheticCoupler.for_setup(quiet), num_timesteps=1, log=lines.append)
    assert "field_ranges" not in stub.calls
