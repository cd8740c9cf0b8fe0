"""Receive-side maps on the host, no GPU (fcx_add_receive_map / fcx_bind_received): the numpy
restatement the GPU tests compare against checked on hand-written values, the argument and
state errors of the C ABI, the named FCX_E_STATE errors of fcx_plan_check, aliases by address,
and the Python set-up that allocates the model-grid sources."""
import ctypes

import numpy as np
import pytest

import namelists
import received
from fcx import _lib
from fcx.basic import IDX, PHASE_ALL, PHASE_EARLY, PHASE_NORMAL
from fcx.engine import Engine
from fcx.setup import setup_from_namelist
from fcx.synthetic import build_case

E_ARG, E_STATE = 1, 2


def _err(lib):
    return lib.fcx_last_error().decode(errors="replace")


def _raw_engine(T=1, n=(64, 64, 64)):
    lib = _lib.load()
    h = ctypes.c_void_p()
    gs = (ctypes.c_int32 * 3)(*n)
    _lib.check(lib.fcx_create(0, T, gs, ctypes.byref(h)))
    return lib, h


def _add(lib, h, grid, n_src, src, dst, w):
    src, dst = np.asarray(src, np.int32), np.asarray(dst, np.int32)
    w = np.asarray(w, np.float64)
    mid = ctypes.c_int32(-7)
    r = lib.fcx_add_receive_map(h, grid, n_src, src.size, ctypes.c_void_p(src.ctypes.data),
                                ctypes.c_void_p(dst.ctypes.data), ctypes.c_void_p(w.ctypes.data), ctypes.byref(mid))
    return r, mid.value


def test_restatement_on_hand_written_values():
    """5 exchange cells: cell 0 one link of weight 1 from a -0.0 source, cell 1 one weighted
    link, cell 2 empty, cell 3 two links given in the order (0.25 * x2, then 0.5 * x0 later in
    the list), cell 4 one unit link."""
    x = np.array([-0.0, 3.0, 8.0])
    src = np.array([0, 1, 2, 1, 0])
    dst = np.array([0, 1, 3, 4, 3])
    w = np.array([1.0, 0.5, 0.25, 1.0, 0.5])
    out = received.expand(src, dst, w, x, 5)
    assert out.tolist() == [0.0, 1.5, 0.0, 2.0, 3.0]
    assert not np.signbit(out[0]) and not np.signbit(out[3]), "0.0 + (-0.0) is +0.0"
    # link order: (0.0 + 0.1 * 3) + 0.2 * 8 is not (0.0 + 0.2 * 8) + 0.1 * 3 in the last bit
    a = received.expand([1, 2], [0, 0], [0.1, 0.2], x, 1)[0]
    b = received.expand([2, 1], [0, 0], [0.2, 0.1], x, 1)[0]
    assert a == (0.0 + 0.1 * 3.0) + 0.2 * 8.0 and b == (0.0 + 0.2 * 8.0) + 0.1 * 3.0
    # fp32: w * (double)x32 summed in double, rounded to float once
    x32 = np.array([0.1, 0.7, 1.3], np.float32)
    o32 = received.expand([0, 1], [0, 0], [0.3, 0.6], x32, 1, np.float32)
    assert o32.dtype == np.float32
    assert o32[0] == np.float32((0.0 + 0.3 * float(x32[0])) + 0.6 * float(x32[1]))


def test_map_argument_errors_name_the_link():
    lib, h = _raw_engine()
    try:
        r, _ = _add(lib, h, 1, 4, [0, 4, 1], [0, 1, 2], [1, 1, 1])
        assert r == E_ARG and "link 1" in _err(lib) and "outside" in _err(lib), _err(lib)
        r, _ = _add(lib, h, 1, 4, [0, 1, -1], [0, 1, 2], [1, 1, 1])
        assert r == E_ARG and "link 2" in _err(lib), _err(lib)
        r, _ = _add(lib, h, 1, 4, [0, 1, 1], [0, 64, 2], [1, 1, 1])
        assert r == E_ARG and "link 1" in _err(lib), _err(lib)
        for bad in (np.nan, np.inf, -np.inf):
            r, _ = _add(lib, h, 1, 4, [0, 1, 1], [0, 1, 2], [1, 1, bad])
            assert r == E_ARG and "link 2" in _err(lib) and "finite" in _err(lib), _err(lib)
        r, _ = _add(lib, h, 1, 0, [], [], [])
        assert r == E_ARG and "n_src" in _err(lib), _err(lib)
        r, _ = _add(lib, h, 4, 4, [0], [0], [1])
        assert r == E_ARG and "grid" in _err(lib), _err(lib)
        r, mid = _add(lib, h, 2, 4, [0, 3], [0, 63], [1, 0.5])
        assert r == 0 and mid == 0
        r, mid = _add(lib, h, 1, 1, [], [], [])  # a map without links: every cell 0.0
        assert r == 0 and mid == 1
    finally:
        lib.fcx_destroy(h)


def test_bind_argument_errors():
    lib, h = _raw_engine()
    try:
        r, mid = _add(lib, h, 1, 4, [0, 3], [0, 63], [1, 0.5])
        assert r == 0
        a = np.zeros(4)
        p = ctypes.c_void_p(a.ctypes.data)
        v = IDX["PSUR"]
        assert lib.fcx_bind_received(h, mid, PHASE_ALL, 0, 1, v, p, 4, 0) == E_ARG and "phase" in _err(lib)
        assert lib.fcx_bind_received(h, mid, 0, 0, 1, v, p, 4, 0) == E_ARG
        assert lib.fcx_bind_received(h, mid + 1, PHASE_NORMAL, 0, 1, v, p, 4, 0) == E_ARG and "unknown" in _err(lib)
        assert lib.fcx_bind_received(h, -1, PHASE_NORMAL, 0, 1, v, p, 4, 0) == E_ARG
        assert lib.fcx_bind_received(h, mid, PHASE_NORMAL, 0, 1, v, p, 3, 0) == E_ARG and "shorter" in _err(lib)
        assert lib.fcx_bind_received(h, mid, PHASE_NORMAL, 0, 1, v, None, 4, 0) == E_ARG
        assert lib.fcx_bind_received(h, mid, PHASE_NORMAL, 0, 4, v, p, 4, 0) == E_ARG and "out of range" in _err(lib)
        assert lib.fcx_bind_received(h, mid, PHASE_NORMAL, 11, 1, v, p, 4, 0) == E_ARG
        assert lib.fcx_bind_received(None, mid, PHASE_NORMAL, 0, 1, v, p, 4, 0) == E_ARG
        assert lib.fcx_bind_received(h, mid, PHASE_NORMAL, 0, 1, v, p, 4, 0) == 0
        # the source of one declaration cannot be the exchange-grid array of a slot
        b = np.zeros(64)
        _lib.check(lib.fcx_bind_field(h, 1, 1, IDX["TSUR"], ctypes.c_void_p(b.ctypes.data), 64, 0))
        r = lib.fcx_bind_received(h, mid, PHASE_NORMAL, 0, 1, IDX["QATM"], ctypes.c_void_p(b.ctypes.data), 64, 0)
        assert r == E_ARG and "exchange-grid field" in _err(lib), _err(lib)
        k, m = ctypes.c_int32(), ctypes.c_int32()
        assert lib.fcx_received_info(h, 0, 1, v, ctypes.byref(k), ctypes.byref(m)) == E_STATE  # before commit
        assert lib.fcx_received_info(None, 0, 1, v, ctypes.byref(k), ctypes.byref(m)) == E_ARG
        assert lib.fcx_receive(h, PHASE_NORMAL) == E_STATE and "fcx_commit" in _err(lib)
        assert lib.fcx_receive(None, PHASE_NORMAL) == E_ARG
    finally:
        lib.fcx_destroy(h)


def _cclm(n=64, **kw):
    case = build_case("CCLM", n=n, T=1, **kw)
    return case, Engine(case.lf, 1, case.methods, commit=False)


def _declare_atmos(e, n, names=received.ATMOS, grid=1):
    n_src, src, dst, w = received.links("unit", n)
    mid = e.add_receive_map(grid, n_src, src, dst, w)
    srcs = {v: np.zeros(n_src) for v in names}
    for v in names:
        e.bind_received(mid, PHASE_NORMAL, 0, grid, v, srcs[v])
    return mid, srcs


def test_plan_check_passes_with_received_atmosphere_fields():
    case, e = _cclm()
    try:
        _declare_atmos(e, 64)
        # a slot without any array becomes bound by its declaration
        n_src, src, dst, w = received.links("weighted", 64)
        mid = e.add_receive_map(1, n_src, src, dst, w)
        for g in (1, 2, 3):
            _lib.check(e.lib.fcx_bind_field(e.h, 1, g, IDX["FICE"], None, 0, 0))
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == 5 and "FICE" in str(ex.value)
        fice = np.zeros(n_src)
        for g in (1, 2, 3):
            e.bind_received(mid, PHASE_NORMAL, 1, g, "FICE", fice)
        with pytest.raises(_lib.FcxError) as ex:  # slots of the u and v grids through the t grid's map
            e.plan_check()
        assert ex.value.status == E_STATE and "FICE(1,u)" in str(ex.value) and "t grid" in str(ex.value), str(ex.value)
    finally:
        e.close()
    case, e = _cclm()
    try:
        _declare_atmos(e, 64)
        e.plan_check()
    finally:
        e.close()


def test_received_and_constant_is_a_named_state_error():
    case, e = _cclm()
    try:
        _declare_atmos(e, 64)
        e.plan_check()
        # (1, t, PSUR) aliases the type-0 array: it turned received with it, so it cannot be a constant
        e.bind_constant(1, 1, "PSUR", 101325.0)
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE, str(ex.value)
        assert "received field PSUR(0,t)" in str(ex.value) and "constant" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_a_received_slot_a_flux_writes_is_refused_by_name():
    case, e = _cclm()
    try:
        n_src, src, dst, w = received.links("unit", 64)
        mid = e.add_receive_map(1, n_src, src, dst, w)
        e.plan_check()
        e.bind_received(mid, PHASE_NORMAL, 1, 1, "HSEN", np.zeros(n_src))
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE, str(ex.value)
        assert "received field HSEN(1,t)" in str(ex.value) and "written" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_a_map_of_the_wrong_grid_is_a_named_state_error():
    case = build_case("CCLM", n=64, T=1, sep_grids=(66, 62))
    e = Engine(case.lf, 1, case.methods, commit=False)
    try:
        n_src, src, dst, w = received.links("unit", 62)
        mid = e.add_receive_map(3, n_src, src, dst, w)  # a map onto the v grid ...
        e.bind_received(mid, PHASE_NORMAL, 0, 2, "UATM", np.zeros(n_src))  # ... for a u-grid slot
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE, str(ex.value)
        assert "UATM(0,u)" in str(ex.value) and "v grid" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_two_declarations_of_one_buffer_must_agree():
    case, e = _cclm()
    try:
        mid, srcs = _declare_atmos(e, 64)
        e.bind_received(mid, PHASE_NORMAL, 1, 1, "PSUR", srcs["PSUR"])  # the alias, declared alike: fine
        e.plan_check()
        e.bind_received(mid, PHASE_EARLY, 1, 1, "QATM", srcs["QATM"])  # the alias in another phase
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE, str(ex.value)
        assert "QATM(0,t)" in str(ex.value) and "QATM(1,t)" in str(ex.value) and "different" in str(ex.value)
    finally:
        e.close()
    case, e = _cclm()
    try:
        mid, srcs = _declare_atmos(e, 64)
        e.bind_received(mid, PHASE_NORMAL, 1, 1, "TATM", np.zeros_like(srcs["TATM"]))  # another source
        with pytest.raises(_lib.FcxError) as ex:
            e.plan_check()
        assert ex.value.status == E_STATE and "TATM" in str(ex.value), str(ex.value)
    finally:
        e.close()


def test_calls_after_commit_are_state_errors():
    """fcx_commit needs the device; the state rule is the one every set-up call shares, checked
    here through fcx_plan_check's own guard and on the GPU in test_gpu_received.py."""
    lib, h = _raw_engine()
    try:
        r, mid = _add(lib, h, 1, 4, [0], [0], [1])
        assert r == 0
        assert lib.fcx_receive(h, 1) == E_STATE
    finally:
        lib.fcx_destroy(h)


def test_setup_allocates_sources_with_the_fields_phases():
    n, atm, oce = received.geometric(12)
    setup = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=(n, n - 3, n + 5))
    assert setup.source_field == {}
    rec = setup.received({"A": {1: atm}, "M": {1: oce}})
    by_letter = {"A": atm[0], "M": oce[0]}
    want = {f.name for f in setup.input_field}
    assert set(setup.source_field) == want and want
    for f in setup.input_field:
        a = setup.source_field[f.name]
        assert a.shape == (by_letter[f.name[1]],) and a.dtype == np.float64, f.name
    assert len(rec) == 2 and {m["n_src"] for m in rec} == {atm[0], oce[0]}
    phases = {(s, g, var): ph for m in rec for ph, s, g, var, _ in m["fields"]}
    for f in setup.input_field:
        assert phases[f.slot] == (PHASE_EARLY if f.early else PHASE_NORMAL), f.name
    assert phases[(1, 1, "TSUR")] == PHASE_EARLY and phases[(0, 1, "PSUR")] == PHASE_NORMAL
    # the declarations pass the plan check of the set-up's own engine
    setup2 = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=(n, n - 3, n + 5))
    e = setup2.engine(regrid=namelists.regrid_matrices((n, n - 3, n + 5)), receive_maps={"A": {1: atm}, "M": {1: oce}},
                      commit=False)
    try:
        e.plan_check()
    finally:
        e.close()
    # a set-up without receive_maps is what it was
    setup3 = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=(n, n - 3, n + 5))
    e = setup3.engine(regrid=namelists.regrid_matrices((n, n - 3, n + 5)), commit=False)
    try:
        assert setup3.source_field == {} and e.receive_maps == []
        e.plan_check()
    finally:
        e.close()
